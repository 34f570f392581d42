// parakeet.cpp_amd/csrc/kernels/tdt_kws.hip -- TDT keyword spotting on the device: where in an utterance was each keyword said, through the TDT head
// (DESIGN.md section 5.5.8).
//
// The specification is tests/tdt_kws_ref.py (normalise + walk + pick).  The lattice is the alignment's (section 5.5.2, kernels/tdt_align.hip), one per
// (clip, keyword) pair, with the prediction net teacher-forced over [blank, keyword...]; every arc costs its log-prob relative to the greedy decision of its
// cell, w = fl(fl(x - top) + fl(dl[i] - dmax)) <= 0; column 0 may be entered at any frame with +0.0, the match ends on the last token's label arc at any
// frame; max-plus in pull form, candidates blank 0 .. D-1 then label 0 .. D-1, strict >; every state carries the frame at which its first token was
// emitted, so there are no back-pointers.  Every score is compared bit for bit, every span and count exactly.
//
//   tdt_kws_act_kernel    lattice_act_row<true> (tdt_lattice_dev.hpp): the alignment's row with one indirection, pair b takes the prediction net's rows of
//       slot net_of[b], so the net runs once per distinct keyword of a group and not once per pair.
//   tdt_kws_keep_kernel   tdt_lattice_keep_kernel that also stores top = fl(+0.0 - lse), the log-prob of the row's largest token logit
//       (fl(fl(m - m) - lse) with the m, lse of wave_row_max_lse).  A copy: built on one row template both kernels came out of the compiler in another
//       instruction order (profiles/kws_shared_walk.md), and the alignment's code object stays what it was.
//   tdt_kws_norm_kernel   one thread per cell, in place: lab -= top, blk -= top, dl[i] -= max_i dl[i].  A pass of its own so that the host-lattice entry
//       point and the model's share one walk, and the diagnostic entry point can return the values before it.
//   tdt_kws_kernel        ONE WAVE per pair, lane u owns column u (L <= 64), advancing by anti-diagonals d = t + u as tdt_align_kernel does.  A finished
//       cell (t, u) with value a offers its successors the 2 D candidates fl(a + w): blank arc i, label arc i.  It computes them itself, from the 2 + D
//       values of ITS OWN cell, and keeps them with its start frame in a per-wave LDS ring of dur_max + 2 diagonals x (2 D + 1) dwords x 64 lanes
//       ([slot][value][lane]: conflict-free).  A cell's pull is then 2 D LDS reads -- its own lane's blank candidates, lane u - 1's label candidates, read
//       from LDS directly: no ds_bpermute, no DPP either -- and no memory access: the only global loads of a diagonal are the own cell's values, and
//       those of diagonal d + 1 are requested before diagonal d is computed.  One workgroup barrier per diagonal (a single wave: it costs a wait on the
//       LDS counter); diagonal d + 1 overwrites the slot of d - dur_max - 1, which diagonal d was the last to read.  Lane 0 (column 0) writes the ENTER
//       state (+0.0, t).  Lane L - 1 folds EXIT over its own D label candidates and stores (E, Bs, Ee) as one 16-byte vector store per frame into the
//       scratch [pairs][T].
//     Picking is the tail of the same kernel, by the same wave: ctc_kws_kernel's (kernels/ctc_kws.hip), COPIED with the span's end read from the entry
//       (Ee[t]) where the CTC form uses t itself -- a shared header would have had to change ctc_kws_kernel's code object.
//
// Bounds: lanes u >= L do nothing; a load's frame is clamped to [0, T - 1]; cell (t, u) of pair b is element cell_off[b] + t (L + 1) + u < cells, label
// element lab_off[b] + t L + u < labs (u < L); scratch entry cell_off[b] - lab_off[b] + t < sum of T; ring index < (dur_max + 2) (2 D + 1) 64.
//
// Code objects (hipcc -O3 --offload-arch=gfx950, from the .s of -save-temps):
//   tdt_kws_kernel        56 VGPR 106 SGPR  LDS 0 B + the ring  scratch 0 B; 0 VGPR spills, 54 SGPRs spilled to VGPR lanes
//   tdt_kws_act_kernel    46 VGPR  24 SGPR  LDS 0 B             scratch 0 B; 0 VGPR spills, 0 SGPR spills
//   tdt_kws_keep_kernel   49 VGPR  38 SGPR  LDS 0 B             scratch 0 B; 0 VGPR spills, 0 SGPR spills
//   tdt_kws_norm_kernel   22 VGPR  24 SGPR  LDS 0 B             scratch 0 B; 0 VGPR spills, 0 SGPR spills
//   (the ring: (dur_max + 2) (2 D + 1) 256 bytes of dynamic LDS, 16896 bytes for 5 durations up to 4, 43520 bytes at the limits)
#include "decode_dev.hpp"
#include "tdt_lattice_dev.hpp"

namespace pk {

__global__ __launch_bounds__(256) void tdt_kws_act_kernel(TdtLattice lt, const int *__restrict__ ep_row0, const float *__restrict__ ep,
                                                          const float *__restrict__ pp, const int *__restrict__ net_of, int n_net, int J, int64_t row0,
                                                          int n, float *__restrict__ z) {
    lattice_act_row<true>(lt, ep_row0, ep, pp, net_of, n_net, J, row0, n, z);
}

__global__ __launch_bounds__(256) void tdt_kws_keep_kernel(TdtLattice lt, float *__restrict__ top, const int *__restrict__ ids,
                                                           const float *__restrict__ logits, int V, int blank, int64_t row0, int n) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int64_t r = row0 + i;
    const int b = lattice_row_owner(lt.cell_off, lt.B, r);
    const int U = lt.id_off[b + 1] - lt.id_off[b], U1 = U + 1;
    const int64_t c = r - lt.cell_off[b];
    const int t = (int)(c / U1), u = (int)(c - (int64_t)t * U1);
    const float *x = logits + i * (int64_t)(V + lt.D);
    const RowLse rl = wave_row_max_lse(x, V, lane);
    const float m = rl.m, lse = rl.lse;
    if (lane == 0) lt.blk[r] = (x[blank] - m) - lse;
    if (lane == 1 && u < U) lt.lab[lt.lab_off[b] + (int64_t)t * U + u] = (x[ids[lt.id_off[b] + u]] - m) - lse;
    if (lane == 2) top[r] = 0.0f - lse;                             // (m - m) - lse of the row's largest logit
    wave_logsoftmax_argmax(x + V, lt.D, lt.dl + r * lt.D, lane);    // (D <= 8: lanes 0 .. D-1 store the duration log-probs)
}

__global__ __launch_bounds__(256) void tdt_kws_norm_kernel(TdtLattice lt, const float *__restrict__ top, int64_t cells) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= cells) return;
    const int b = lattice_row_owner(lt.cell_off, lt.B, r);
    const int U = lt.id_off[b + 1] - lt.id_off[b], U1 = U + 1, D = lt.D;
    const int64_t c = r - lt.cell_off[b];
    const int t = (int)(c / U1), u = (int)(c - (int64_t)t * U1);
    const float g = top[r];
    lt.blk[r] = lt.blk[r] - g;
    if (u < U) {
        float *l = lt.lab + lt.lab_off[b] + (int64_t)t * U + u;
        *l = *l - g;
    }
    float *d = lt.dl + r * D;
    float dm = d[0];
    for (int i = 1; i < D; ++i) dm = fmaxf(dm, d[i]);
    for (int i = 0; i < D; ++i) d[i] = d[i] - dm;
}

__global__ __launch_bounds__(64) void tdt_kws_kernel(TdtKwsArgs a) {
    extern __shared__ float kring[];                                // [dur_max + 2][2 D + 1][64]: blank candidates, label candidates, start frame
    const TdtLattice &lt = a.lt;
    const int b = blockIdx.x, u = threadIdx.x;
    const int T = lt.T[b], L = lt.id_off[b + 1] - lt.id_off[b], U1 = L + 1, D = lt.D;
    const int64_t c0 = lt.cell_off[b];
    const float *lab = lt.lab + lt.lab_off[b], *blk = lt.blk + c0, *dl = lt.dl + c0 * D;
    int4 *eb = a.eb + (c0 - lt.lab_off[b]);
    const int R = a.dur_max + 2, K = 2 * D + 1;
    const float NEG = -__builtin_huge_valf();
    int dur[8], bstep[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { dur[i] = i < D ? lt.durations[i] : 1; bstep[i] = dur[i] > 1 ? dur[i] : 1; }
    const int uc = u < L ? u : L - 1;                               // the column this lane loads (lanes past the keyword load in bounds and store nothing)

    float nb, nl, nd[8];                                            // the own cell's values of the NEXT diagonal
    auto fetch = [&](int t) {
        const int tt = t < 0 ? 0 : t < T ? t : T - 1;
        const int64_t cell = (int64_t)tt * U1 + uc;
        nb = blk[cell]; nl = lab[(int64_t)tt * L + uc];
#pragma unroll
        for (int i = 0; i < 8; ++i) nd[i] = i < D ? dl[cell * D + i] : 0.0f;
    };
    fetch(-u);
    int dm = 0;                                                     // d % R, kept by increment: the slot of diagonal d - k is dm - k (+ R when negative)
    auto slot = [&](int k) { const int q = dm - k; return (q < 0 ? q + R : q) * K; };
    for (int d = 0; d < T + L - 1; ++d, dm = dm + 1 == R ? 0 : dm + 1) {
        const int t = d - u;
        const float xb = nb, xl = nl;
        float xd[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) xd[i] = nd[i];
        fetch(t + 1);
        const bool active = u < L && t >= 0 && t < T;
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
                    const int s = slot(dur[i] + 1);
                    const float cand = kring[(s + D + i) * 64 + u - 1];
                    if (cand > best) { best = cand; org = __float_as_int(kring[(s + 2 * D) * 64 + u - 1]); }
                }
            }
        }
        if (active) {
            float e = NEG;
            int ee = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (i < D) {
                    const float cb = best + (xb + xd[i]), cl = best + (xl + xd[i]);
                    kring[(dm * K + i) * 64 + u] = cb;
                    kring[(dm * K + D + i) * 64 + u] = cl;
                    if (cl > e) { e = cl; ee = tdt_token_end(t, dur[i], T); }
                }
            }
            kring[(dm * K + 2 * D) * 64 + u] = __int_as_float(org);
            if (u == L - 1) eb[t] = make_int4(__float_as_int(e), org, ee, 0);      // EXIT
        }
        __syncthreads();
    }
    __threadfence_block();
    __syncthreads();                                                // lane L - 1's stores are read by every lane from here on

    const int H = a.max_hits;
    const float min_score = a.min_score;
    int *start = a.start + (int64_t)b * H, *end = a.end + (int64_t)b * H;
    float *score = a.score + (int64_t)b * H;
    const int lane = u;
    int n = 0, ps = 0, pe = -1;                                     // hits so far; the span of the last one
    for (int h = 0; h < H; ++h) {
        float bv = NEG;
        int bt = 0x7fffffff;
        for (int t = lane; t < T; t += 64) {
            const int4 v = eb[t];
            float e = __int_as_float(v.x);
            if (n > 0 && e > NEG && v.y <= pe && ps <= v.z) {       // [Bs[t], Ee[t]] meets the last hit: masked from now on
                e = NEG;
                eb[t].x = __float_as_int(NEG);
            }
            if (e > NEG && e >= min_score && e > bv) { bv = e; bt = t; }
        }
        wave_butterfly([&](auto off) {
            constexpr int OFF = decltype(off)::value;
            const float ov = wave_xor<OFF>(bv);
            const int ot = wave_xor_i<OFF>(bt);
            if (ov > bv || (ov == bv && ot < bt)) { bv = ov; bt = ot; }
        });
        if (!(bv > NEG)) break;                                     // (uniform: every lane holds the same pair)
        const int4 hit = eb[bt];
        ps = hit.y; pe = hit.z;
        if (lane == 0) { start[h] = ps; end[h] = pe; score[h] = bv; }
        ++n;
    }
    if (lane == 0) a.n_hits[b] = n;
    if (lane >= n && lane < H) { start[lane] = 0; end[lane] = 0; score[lane] = NEG; }
}

void launch_tdt_kws_act(const TdtLattice &lt, const int *ep_row0, const float *ep, const float *pp, const int *net_of, int n_net, int J, int64_t row0, int n,
                        float *z, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(tdt_kws_act_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, lt, ep_row0, ep, pp, net_of, n_net, J, row0, n, z);
}

void launch_tdt_kws_keep(const TdtLattice &lt, float *top, const int *ids, const float *logits, int V, int blank, int64_t row0, int n, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(tdt_kws_keep_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, lt, top, ids, logits, V, blank, row0, n);
}

void launch_tdt_kws_norm(const TdtLattice &lt, const float *top, int64_t cells, hipStream_t s) {
    if (cells <= 0) return;
    hipLaunchKernelGGL(tdt_kws_norm_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, lt, top, cells);
}

void launch_tdt_kws(const TdtKwsArgs &a, hipStream_t s) {
    if (!kws_ring_limits_ok(a.lt, a.dur_max) || a.max_hits < 1 || a.max_hits > kKwsMaxHits) {
        fprintf(stderr, "parakeet_amd: internal error: launch_tdt_kws outside the kernel's limits (dur_max %d, D %d, max_hits %d)\n", a.dur_max, a.lt.D,
                a.max_hits);
        abort();
    }
    hipLaunchKernelGGL(tdt_kws_kernel, dim3(a.lt.B), dim3(64), kws_ring_lds_bytes(a.dur_max, a.lt.D), s, a);
}

}  // namespace pk
