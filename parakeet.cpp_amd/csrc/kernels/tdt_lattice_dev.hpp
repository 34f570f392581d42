// parakeet.cpp_amd/csrc/kernels/tdt_lattice_dev.hpp -- code shared by the kernels over the TDT lattice (DESIGN.md sections 5.5.2, 5.5.3, 5.5.5): the
// anti-diagonal walk as a function template over its fold (tdt_total_kernel calls it), the launch checks of the two walk kernels, the joint activation row of
// the lattice and of the beam, the activation row body of the alignment's and the keyword spotting's lattice kernels, a label arc's end frame.
#pragma once
#include <cstdio>
#include <cstdlib>

#include "decode_dev.hpp"

namespace pk {

// z = relu(enc_proj[t] + pred_proj) of one row by one wave, as the decode loop's joint activation forms it (decode_dev.hpp SK_ACT: enc_proj +
// (pred_proj [+ bias]), > 0 ? s : 0), natural columns.  float4 where J allows (rows of J floats behind 16-byte aligned bases), one add and one compare per
// element either way.  The scalar form is unreachable and no test can run it: Model::validate_config refuses a joint_hidden that is no multiple of 64.
__device__ __forceinline__ void joint_act_row(const float *__restrict__ er, const float *__restrict__ pr, float *__restrict__ zr, int J, int lane) {
    if ((J & 3) == 0) {
        for (int j = 4 * lane; j < J; j += 256) {
            const float4 e = *reinterpret_cast<const float4 *>(er + j), p = *reinterpret_cast<const float4 *>(pr + j);
            float4 s;
            s.x = e.x + p.x; s.y = e.y + p.y; s.z = e.z + p.z; s.w = e.w + p.w;
            s.x = s.x > 0.0f ? s.x : 0.0f; s.y = s.y > 0.0f ? s.y : 0.0f; s.z = s.z > 0.0f ? s.z : 0.0f; s.w = s.w > 0.0f ? s.w : 0.0f;
            *reinterpret_cast<float4 *>(zr + j) = s;
        }
    } else {
        for (int j = lane; j < J; j += 64) {
            const float s = er[j] + pr[j];
            zr[j] = s > 0.0f ? s : 0.0f;
        }
    }
}

// owner (utterance, or keyword spotting pair) of lattice row r: the last b with cell_off[b] <= r (cell_off ascending, cell_off[B] = rows in all)
__device__ __forceinline__ int lattice_row_owner(const int64_t *__restrict__ cell_off, int B, int64_t r) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (cell_off[mid] <= r) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The body of a kernel over lattice rows [row0, row0 + n), one wave per row, four rows per workgroup of 256: z[i] = joint_act_row of the row's frame and
// prediction-net row.  Owner b reads the net's rows pp[u B + b], or with NET_OF pp[u n_net + net_of[b]] (the net run once per distinct keyword).
template <bool NET_OF>
__device__ __forceinline__ void lattice_act_row(const TdtLattice &lt, const int *__restrict__ ep_row0, const float *__restrict__ ep,
                                                const float *__restrict__ pp, const int *__restrict__ net_of, int n_net, int J, int64_t row0, int n,
                                                float *__restrict__ z) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int64_t r = row0 + i;
    const int b = lattice_row_owner(lt.cell_off, lt.B, r);
    const int U1 = lt.id_off[b + 1] - lt.id_off[b] + 1;
    const int64_t c = r - lt.cell_off[b];
    const int t = (int)(c / U1), u = (int)(c - (int64_t)t * U1);
    int64_t pr;
    if constexpr (NET_OF) pr = (int64_t)u * n_net + net_of[b];
    else pr = (int64_t)u * lt.B + b;
    joint_act_row(ep + ((int64_t)ep_row0[b] + t) * J, pp + pr * J, z + i * J, J, lane);
}

// last frame of a token emitted at frame t by a label arc of duration dur, in an utterance of T frames
__device__ __forceinline__ int tdt_token_end(int t, int dur, int T) {
    const int e = t + (dur > 1 ? dur : 1) - 1;
    return e < T ? e : T - 1;
}

// The fold of the forward total: a left fold with dlaef from -inf over the candidates of a cell (or of END); `code` is the arc (i = blank arc i, D + i =
// label arc i), which this fold does not keep.  (The alignment's max-plus walk is written out in tdt_align.hip: see its header.)
struct TdtLogSum {
    float v = -__builtin_huge_valf();
    __device__ __forceinline__ void take(float cand, int) { v = dlaef(v, cand); }
};

// The walk over utterance b's lattice by its workgroup of NT threads; every thread must call it.  Anti-diagonals d = t + u, alpha in `ring` (dynamic LDS,
// (dur_max + 2) diagonals of u_max + 1 floats), ONE barrier per diagonal, a cell's candidates blank 0 .. D-1 then label 0 .. D-1, each alpha[src] +
// (x + dl) as two fp32 adds: the header of tdt_align.hip describes it.
// A candidate whose source frame is < 0 is skipped: it is -inf, which neither fold takes (dlaef(a, -inf) = a bit for bit).
// A cell starts from d == 0 ? 0 : -inf.  Cell (0, 0) is the one cell that is not a fold, and it has no candidate with a source frame >= 0, so seeding it
// before the candidates (as tdt_align_kernel does) and setting it after them are the same thing.
// `tail` keeps alpha of the last kTdtAlignMaxDur frames of columns U - 1 and U, which is what END pulls from.  END is folded by thread 0 alone: frames
// ascending, blank before label, then by i; its fold is returned (meaningful in thread 0 only).
// dur[] / bstep[] are wave-uniform and live in SGPRs.  The cell loops index them by unrolled constants only; END's loops run i to D, and the compiler resolves
// that index without private memory (scratch 0 bytes in both kernels: the figures in tdt_align.hip / tdt_total.hip).
template <int NT, typename Fold>
__device__ __forceinline__ Fold tdt_lattice_walk(const TdtLattice &lt, int b, int u_max, int dur_max, float *ring, float (*tail)[kTdtAlignMaxDur]) {
    const int tid = threadIdx.x;
    const int T = lt.T[b], i0 = lt.id_off[b], U = lt.id_off[b + 1] - i0, U1 = U + 1, D = lt.D;
    const int64_t c0 = lt.cell_off[b];
    const float *lab = lt.lab + lt.lab_off[b], *blk = lt.blk + c0, *dl = lt.dl + c0 * D;
    const int R = dur_max + 2, pitch = u_max + 1;
    const float NEG = -__builtin_huge_valf();
    int dur[8], bstep[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { dur[i] = i < D ? lt.durations[i] : 1; bstep[i] = dur[i] > 1 ? dur[i] : 1; }
    if (tid < 2 * kTdtAlignMaxDur) (&tail[0][0])[tid] = NEG;
    __syncthreads();
    const int t_tail = T - kTdtAlignMaxDur;
    int dm = 0;                                                     // d % R, kept by increment: the slot of diagonal d - k is dm - k (+ R when negative)
    auto slot = [&](int k) { const int q = dm - k; return (q < 0 ? q + R : q) * pitch; };
    for (int d = 0; d < T + U; ++d, dm = dm + 1 == R ? 0 : dm + 1) {
        const int lo = d - (T - 1) > 0 ? d - (T - 1) : 0, hi = d < U ? d : U;
        float *cur = ring + dm * pitch;
        for (int u = lo + tid; u <= hi; u += NT) {
            const int t = d - u;
            Fold f;
            if (d == 0) f.v = 0.0f;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int ts = t - bstep[i];
                if (i < D && ts >= 0) {
                    const int64_t sc = (int64_t)ts * U1 + u;
                    const float w = blk[sc] + dl[sc * D + i];
                    f.take(ring[slot(bstep[i]) + u] + w, i);
                }
            }
            if (u >= 1) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int ts = t - dur[i];
                    if (i < D && ts >= 0) {
                        const int64_t sc = (int64_t)ts * U1 + (u - 1);
                        const float w = lab[(int64_t)ts * U + (u - 1)] + dl[sc * D + i];
                        f.take(ring[slot(dur[i] + 1) + (u - 1)] + w, D + i);
                    }
                }
            }
            cur[u] = f.v;
            if (u >= U - 1 && t >= t_tail) tail[u - (U - 1)][t - t_tail] = f.v;
        }
        __syncthreads();
    }
    Fold end;
    if (tid == 0) {
        for (int t = t_tail > 0 ? t_tail : 0; t < T; ++t) {
            for (int i = 0; i < D; ++i) {
                if (t + bstep[i] >= T) {
                    const int64_t sc = (int64_t)t * U1 + U;
                    end.take(tail[1][t - t_tail] + (blk[sc] + dl[sc * D + i]), i);
                }
            }
            if (U >= 1) {
                for (int i = 0; i < D; ++i) {
                    if (t + dur[i] >= T) {
                        const int64_t sc = (int64_t)t * U1 + (U - 1);
                        end.take(tail[0][t - t_tail] + (lab[(int64_t)t * U + (U - 1)] + dl[sc * D + i]), D + i);
                    }
                }
            }
        }
    }
    return end;
}

// host side of both launches: the limits the walks are built for (refused by the host before anything is allocated) -> the dynamic LDS of the ring
inline size_t tdt_walk_launch_checks(const char *who, const TdtLattice &lt, int u_max, int dur_max) {
    if (dur_max < 0 || dur_max > kTdtAlignMaxDur || u_max < 0 || u_max > kTdtAlignMaxTokens || lt.D < 1 || lt.D > 8) {
        fprintf(stderr, "parakeet_amd: internal error: %s outside the kernel's limits (dur_max %d, u_max %d, D %d)\n", who, dur_max, u_max, lt.D);
        abort();
    }
    return (size_t)(dur_max + 2) * (u_max + 1) * sizeof(float);
}

// The spotting walks' LDS ring (tdt_kws.hip, tdt_kws_stream.hip), [dur_max + 2][2 D + 1][64] dwords: the limits it is built for (refused by the host before
// anything is allocated; each launcher adds its own) and its dynamic LDS in bytes.
inline bool kws_ring_limits_ok(const TdtLattice &lt, int dur_max) { return dur_max >= 0 && dur_max <= kTdtAlignMaxDur && lt.D >= 1 && lt.D <= 8; }
inline size_t kws_ring_lds_bytes(int dur_max, int D) { return (size_t)(dur_max + 2) * (2 * D + 1) * 64 * sizeof(float); }

}  // namespace pk
