// parakeet.cpp_amd/csrc/kernels/tdt_kws_stream.hip -- streaming TDT keyword spotting: the walk of kernels/tdt_kws.hip stopped at a chunk boundary and
// picked up again, and a hit rule that needs no future frame.
//
// The specification is tests/tdt_kws_stream_ref.py (ChunkWalk + OnlinePick).  The lattice, its normalisation and the recurrence are section 5.5.8's: one
// lattice per (stream, keyword) pair over the chunk's c frames, built by the act / heads / keep / norm launches of tdt_kws.hip; every arc costs
// w = fl(fl(x - top) + fl(dl[i] - dmax)) <= 0; column 0 is entered at every frame with +0.0; candidates blank 0 .. D-1 then label 0 .. D-1, strict >;
// every state carries the frame of its first token.  Frames are numbered from the start of the session and the session has no last frame: the end of
// a match is t + max(dur, 1) - 1, unclamped.  Every score is compared bit for bit, every span and event exactly.
//
//   tdt_kws_chunk_kernel  ONE WAVE per pair, lane u owns column u (L <= 64), advancing by anti-diagonals over the chunk's frames [t0, t0 + c) ALONE:
//       step d has lane u at frame t0 + d - u.  The offered candidates live in tdt_kws_kernel's per-wave LDS ring [slot][2 D + 1][64], but the slot of a
//       cell is its FRAME modulo dur_max + 2, not its diagonal, so what a later chunk may read -- every column's candidates and start frame of the last
//       dur_max + 1 frames -- is the ring itself: at entry every lane loads its column of the pair's carried ring from global memory ((dur_max + 2)
//       (2 D + 1) L dwords per pair, [slot][value][column]: coalesced), at exit it stores it back, with plain vector stores.  A chunk shorter than
//       dur_max writes only its own frames' slots, so the older frames go back as they came.  The carried ring starts at -inf (a start frame is read only
//       behind a candidate that won): a source frame before frame 0 offers nothing, and is skipped anyway.  A pull of lane u at frame t reads its own slots of frames t - 1 .. t - max(dur_max, 1)
//       and lane u - 1's of frames t .. t - dur_max, while lane u - 1 writes frame t + 1 and lane u frame t: dur_max + 2 slots keep them apart.  One
//       workgroup barrier per step (a single wave: a wait on the LDS counter).  Lane L - 1 folds EXIT over its own D label candidates and leaves
//       (E, Bs, Ee) of the frame in LDS behind the ring (and in rows[b][c], when the caller asks for them).
//     The online rule is the tail of the same kernel, by the same wave: every lane reads the chunk's c exit rows from LDS in order (one broadcast
//       read each) and keeps the pair's pending hit and the end of the last hit that left in registers; lane 0 stores the events that leave, their count, and the pending hit back into
//       the pair's carried state.  At most one event leaves per frame, so c slots hold them.
//
// Bounds: lanes u >= L load column L - 1 in bounds and store nothing; a load's local frame is clamped to [0, c - 1]; cell (t, u) of pair b is element
// cell_off[b] + t (L + 1) + u < cells, label element lab_off[b] + t L + u < labs (u < L); ring element (dur_max + 2) (2 D + 1) id_off[b] + j L + u with
// j < (dur_max + 2) (2 D + 1), u < L; LDS ring index < (dur_max + 2) (2 D + 1) 64, stage index < 3 c; event slot n < c; rows entry b c + t.
//
// Code object (hipcc -O3 --offload-arch=gfx950, from the .s of -save-temps):
//   tdt_kws_chunk_kernel  55 VGPR 106 SGPR  LDS 0 B + the ring + 12 c bytes  scratch 0 B; 0 VGPR spills, 39 SGPRs spilled to VGPR lanes
//   (the ring: (dur_max + 2) (2 D + 1) 256 bytes of dynamic LDS, 16896 bytes for 5 durations up to 4, 43520 bytes at the limits; 744 bytes of rows at c = 62)
#include "decode_dev.hpp"
#include "tdt_lattice_dev.hpp"

namespace pk {

__global__ __launch_bounds__(64) void tdt_kws_chunk_kernel(TdtKwsChunkArgs a) {
    extern __shared__ float kring[];                                // [dur_max + 2][2 D + 1][64]: blank candidates, label candidates, start frame; then [c][3]
    const TdtLattice &lt = a.lt;
    const int b = blockIdx.x, u = threadIdx.x;
    const int c = a.c, t0 = a.t0, L = lt.id_off[b + 1] - lt.id_off[b], U1 = L + 1, D = lt.D;
    const int64_t c0 = lt.cell_off[b];
    const float *lab = lt.lab + lt.lab_off[b], *blk = lt.blk + c0, *dl = lt.dl + c0 * D;
    const int R = a.dur_max + 2, K = 2 * D + 1;
    int *stage = reinterpret_cast<int *>(kring + R * K * 64);
    float *gring = a.ring + (int64_t)R * K * lt.id_off[b];
    const float NEG = -__builtin_huge_valf();
    int dur[8], bstep[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { dur[i] = i < D ? lt.durations[i] : 1; bstep[i] = dur[i] > 1 ? dur[i] : 1; }
    const int uc = u < L ? u : L - 1;                               // the column this lane loads (lanes past the keyword load in bounds and store nothing)

    for (int j = 0; j < R * K; ++j) kring[j * 64 + u] = gring[(int64_t)j * L + uc];       // the carried ring: this lane's column

    float nb, nl, nd[8];                                            // the own cell's values of the NEXT step
    auto fetch = [&](int tl) {
        const int tt = tl < 0 ? 0 : tl < c ? tl : c - 1;
        const int64_t cell = (int64_t)tt * U1 + uc;
        nb = blk[cell]; nl = lab[(int64_t)tt * L + uc];
#pragma unroll
        for (int i = 0; i < 8; ++i) nd[i] = i < D ? dl[cell * D + i] : 0.0f;
    };
    fetch(-u);
    int sm = (t0 - u) % R;                                          // this lane's frame % R, kept by increment: the slot of frame t - k is sm - k (+ R when negative)
    if (sm < 0) sm += R;
    auto slot = [&](int k) { const int q = sm - k; return (q < 0 ? q + R : q) * K; };
    __syncthreads();
    for (int d = 0; d < c + L - 1; ++d, sm = sm + 1 == R ? 0 : sm + 1) {
        const int tl = d - u, t = t0 + tl;                          // frame of the chunk, frame of the session
        const float xb = nb, xl = nl;
        float xd[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) xd[i] = nd[i];
        fetch(tl + 1);
        const bool active = u < L && tl >= 0 && tl < c;
        float best = NEG;
        int org = 0;
        if (u == 0) { best = 0.0f; org = t; }                       // ENTER
        else if (active) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (i < D && t - bstep[i] >= 0) {
                    const int s = slot(bstep[i]);
                    const float cand = kring[(s + i) * 64 + u];
                    if (cand > best) { best = cand; org = __float_as_int(kring[(s + 2 * D) * 64 + u]); }
                }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (i < D && t - dur[i] >= 0) {
                    const int s = slot(dur[i]);
                    const float cand = kring[(s + D + i) * 64 + u - 1];
                    if (cand > best) { best = cand; org = __float_as_int(kring[(s + 2 * D) * 64 + u - 1]); }
                }
            }
        }
        if (active) {
            float e = NEG;
            int ee = 0;
            const int s = sm * K;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (i < D) {
                    const float cb = best + (xb + xd[i]), cl = best + (xl + xd[i]);
                    kring[(s + i) * 64 + u] = cb;
                    kring[(s + D + i) * 64 + u] = cl;
                    if (cl > e) { e = cl; ee = t + bstep[i] - 1; }
                }
            }
            kring[(s + 2 * D) * 64 + u] = __int_as_float(org);
            if (u == L - 1) {                                       // EXIT
                stage[3 * tl] = __float_as_int(e); stage[3 * tl + 1] = org; stage[3 * tl + 2] = ee;
                if (a.rows) a.rows[(int64_t)b * c + tl] = make_int4(__float_as_int(e), org, ee, 0);
            }
        }
        __syncthreads();
    }
    if (u < L)
        for (int j = 0; j < R * K; ++j) gring[(int64_t)j * L + u] = kring[j * 64 + u];

    // the online rule over the chunk's frames, every lane alike (lane L - 1's rows are visible since the loop's last barrier)
    const int4 p = a.pend[b];
    float ps = __int_as_float(p.x);
    int pst = p.y, pen = p.z, has = p.w, n = 0, last = a.last_end[b];       // last: the end of the last hit that left (-1: none yet)
    int4 *ev = a.ev + (int64_t)b * c;
    const float min_score = a.min_score;
    const int64_t patience = a.patience;
    auto emit = [&]() {
        if (u == 0) ev[n] = make_int4(__float_as_int(ps), pst, pen, 0);
        ++n; has = 0; last = pen;
    };
    for (int j = 0; j < c; ++j) {
        const int t = t0 + j;
        const float e = __int_as_float(stage[3 * j]);
        const int bs = stage[3 * j + 1], ee = stage[3 * j + 2];
        if (has && (int64_t)t > (int64_t)pen + patience) emit();
        if (e > NEG && e >= min_score && bs > last) {
            if (has && !(bs <= pen && pst <= ee)) emit();           // a span that does not meet the pending one lies after it
            if (!has || e > ps) { ps = e; pst = bs; pen = ee; has = 1; }
        }
    }
    if (u == 0) {
        a.pend[b] = has ? make_int4(__float_as_int(ps), pst, pen, 1) : make_int4(__float_as_int(NEG), 0, 0, 0);
        a.n_ev[b] = n;
        a.last_end[b] = last;
    }
}

void launch_tdt_kws_chunk(const TdtKwsChunkArgs &a, hipStream_t s) {
    if (!kws_ring_limits_ok(a.lt, a.dur_max) || a.c < 1 || a.c > kKwsChunkMaxFrames || a.t0 < 0 || a.patience < 0) {
        fprintf(stderr, "parakeet_amd: internal error: launch_tdt_kws_chunk outside the kernel's limits (dur_max %d, D %d, c %d, t0 %d, patience %d)\n",
                a.dur_max, a.lt.D, a.c, a.t0, a.patience);
        abort();
    }
    const size_t lds = kws_ring_lds_bytes(a.dur_max, a.lt.D) + (size_t)a.c * 3 * sizeof(int);
    hipLaunchKernelGGL(tdt_kws_chunk_kernel, dim3(a.lt.B), dim3(64), lds, s, a);
}

}  // namespace pk
