// parakeet.cpp_amd/csrc/kernels/tdt_total.hip -- the forward-algorithm total of a GIVEN token string under the TDT head.
//
// The specification is tests/tdt_total_ref.py: the lattice and the arcs of the TDT forced alignment (kernels/tdt_align.hip, tests/tdt_align_ref.py),
// walked sum-product in pull form: alpha[0][0] = 0, every other cell a left fold with lae (m + dlogf(1 + dexpf(n - m)), m where n == -inf: the one
// kernels/ctc_align.hip uses) from -inf over the candidates blank 0 .. D-1 then label 0 .. D-1, each alpha[src] + (x + dl) as two fp32 adds; a blank
// of duration 0 and a blank of duration 1 are two arcs to t + 1 and both are summed.  END is the same fold over the source frames in ascending
// order, blank before label, then by i.  The value is compared bit for bit.
//
//   tdt_total_kernel<NT>      one workgroup of NT threads per hypothesis, advancing by anti-diagonals d = t + u exactly as tdt_align_kernel does:
//       alpha lives in LDS as a ring of dur_max + 2 diagonals of u_max + 1 floats, indexed [d % ring][u], ONE barrier per diagonal (diagonal d + 1
//       overwrites the slot of d - dur_max - 1, which diagonal d was the last to read).  Thread i takes the cells u = lo + i, lo + i + NT, ...; a
//       cell's 2 D candidates read the source cell's values from memory (2 + D floats per cell) and its alpha from the ring.  Nothing is written
//       per cell: no back-pointers, no back-trace.  END is folded by thread 0 from the alpha of the last kTdtAlignMaxDur frames of columns U - 1
//       and U, kept in a small LDS table.  total[b] = END, ok[b] = END > -inf.
//       The fold skips a candidate whose source frame is < 0; the specification folds -inf there, and lae(a, -inf) = a bit for bit.
//
// Limits (host side: tdt_total.cpp refuses with PK_ERR_UNSUPPORTED before anything is allocated): those of the alignment -- durations in
//   [0, kTdtAlignMaxDur = 8], 1 <= D <= 8, U_b <= kTdtAlignMaxTokens = 1535 (ring of (8 + 2) x 1536 x 4 = 61440 bytes of LDS), scratch of a call or of
//   a group of hypotheses <= 1 GiB (formula: tdt_total.hpp, the alignment's without the back-pointer bytes).
//
// Code objects (hipcc -O3 --offload-arch=gfx950, from the .s of -save-temps):
//   tdt_total_kernel< 64>       37 VGPR 106 SGPR  LDS 64 B + the ring  scratch 0 B; 0 VGPR spills, 41 SGPRs spilled to VGPR lanes
//   tdt_total_kernel<256>       37 VGPR 106 SGPR  LDS 64 B + the ring  scratch 0 B; 0 VGPR spills, 41 SGPRs spilled to VGPR lanes
//   (as in tdt_align_kernel the durations and blank steps are wave-uniform and live in SGPRs; nothing goes to private memory)
//   (the ring: (dur_max + 2) (u_max + 1) 4 bytes of dynamic LDS, 3 KB for 90 tokens and durations up to 4, 61440 bytes at the limits)
#include "../pk_devmath.h"
#include "kernels.hpp"

namespace pk {

namespace {

// log(exp a + exp b) = m + log(1 + exp(n - m)), m = max, n = min; m where n == -inf   (lae of tests/ctc_beam_ref.py, align_lae of ctc_align.hip)
__device__ __forceinline__ float total_lae(float a, float b) {
    const float m = fmaxf(a, b), n = fminf(a, b);
    if (!(n > -__builtin_huge_valf())) return m;
    return m + dlogf(1.0f + dexpf(n - m));
}

}  // namespace

template <int NT>
__global__ __launch_bounds__(NT) void tdt_total_kernel(TdtTotalArgs a) {
    extern __shared__ float ring[];                                 // [dur_max + 2][u_max + 1]
    __shared__ float tail[2][kTdtAlignMaxDur];                      // alpha[T - 8 + j][U - 1 + c]: what END pulls from
    const TdtLattice &lt = a.lt;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int T = lt.T[b], i0 = lt.id_off[b], U = lt.id_off[b + 1] - i0, U1 = U + 1, D = lt.D;
    const int64_t c0 = lt.cell_off[b];
    const float *lab = lt.lab + lt.lab_off[b], *blk = lt.blk + c0, *dl = lt.dl + c0 * D;
    const int R = a.dur_max + 2, pitch = a.u_max + 1;
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
            float acc = NEG;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int ts = t - bstep[i];
                if (i < D && ts >= 0) {
                    const int64_t sc = (int64_t)ts * U1 + u;
                    const float w = blk[sc] + dl[sc * D + i];
                    acc = total_lae(acc, ring[slot(bstep[i]) + u] + w);
                }
            }
            if (u >= 1) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int ts = t - dur[i];
                    if (i < D && ts >= 0) {
                        const int64_t sc = (int64_t)ts * U1 + (u - 1);
                        const float w = lab[(int64_t)ts * U + (u - 1)] + dl[sc * D + i];
                        acc = total_lae(acc, ring[slot(dur[i] + 1) + (u - 1)] + w);
                    }
                }
            }
            if (d == 0) acc = 0.0f;                                 // alpha[0][0]: the one cell that is not a fold
            cur[u] = acc;
            if (u >= U - 1 && t >= t_tail) tail[u - (U - 1)][t - t_tail] = acc;
        }
        __syncthreads();
    }
    if (tid == 0) {
        float end = NEG;
        for (int t = t_tail > 0 ? t_tail : 0; t < T; ++t) {
            for (int i = 0; i < D; ++i) {
                if (t + bstep[i] >= T) {
                    const int64_t sc = (int64_t)t * U1 + U;
                    end = total_lae(end, tail[1][t - t_tail] + (blk[sc] + dl[sc * D + i]));
                }
            }
            if (U >= 1) {
                for (int i = 0; i < D; ++i) {
                    if (t + dur[i] >= T) {
                        const int64_t sc = (int64_t)t * U1 + (U - 1);
                        end = total_lae(end, tail[0][t - t_tail] + (lab[(int64_t)t * U + (U - 1)] + dl[sc * D + i]));
                    }
                }
            }
        }
        a.total[b] = end;
        a.ok[b] = end > NEG ? 1 : 0;
    }
}

void launch_tdt_total(const TdtTotalArgs &a, hipStream_t s) {
    if (a.dur_max < 0 || a.dur_max > kTdtAlignMaxDur || a.u_max < 0 || a.u_max > kTdtAlignMaxTokens || a.lt.D < 1 || a.lt.D > 8) {
        fprintf(stderr, "parakeet_amd: internal error: launch_tdt_total outside the kernel's limits (dur_max %d, u_max %d, D %d)\n", a.dur_max, a.u_max, a.lt.D);
        abort();
    }
    if (a.lt.B <= 0) return;
    const size_t lds = (size_t)(a.dur_max + 2) * (a.u_max + 1) * sizeof(float);
    if (a.u_max + 1 <= kTdtAlignThreads[0]) hipLaunchKernelGGL(tdt_total_kernel<64>, dim3(a.lt.B), dim3(64), lds, s, a);
    else hipLaunchKernelGGL(tdt_total_kernel<256>, dim3(a.lt.B), dim3(256), lds, s, a);
}

}  // namespace pk
