// parakeet.cpp_amd/csrc/kernels/tdt_align.hip -- TDT forced alignment of a GIVEN token string on the device.
//
// The specification is tests/tdt_align_ref.py: the T x (U + 1) lattice of joint evaluations (frame t, prediction net after ids[:u]), blank arc i
// to (t + max(dur[i], 1), u), label arc i to (t + dur[i], u + 1), one terminal END; a max-plus walk in pull form, candidates blank 0 .. D-1 then
// label 0 .. D-1, each alpha[src] + (x + dl) as two fp32 adds, strict > (the earlier candidate stays).  Every value is compared bit for bit.
//
//   tdt_lattice_act_kernel    z = relu(enc_proj[t] + pred_proj[u]) for a chunk of lattice rows: the A operand of the heads product on the fp32 GEMM.
//       One wave per row: lattice_act_row<false> (tdt_lattice_dev.hpp; the keyword spotting's kernel is the <true> form), the row itself joint_act_row.
//   tdt_lattice_keep_kernel   one wave per row of the heads product's output [V + D]: the canonical log-softmax (wave_row_max_lse: row
//       maximum, dexpf_nonpos, 64 strided partial sums in index order, wave_sum64, dlogf; the duration head through wave_logsoftmax_argmax's
//       low-8 form, exactly the decision kernel's) and only 2 + D values leave: the label log-prob of ids[u], the blank's, the D duration
//       log-probs.  The chunk's logits are the only place a whole row exists.
//   tdt_align_kernel<NT>      one workgroup of NT threads per utterance, advancing by anti-diagonals d = t + u: every predecessor of a cell lies
//       on an earlier diagonal (blank i on d - max(dur, 1), label i on d - dur - 1, so also the dur = 0 label arc from (t, u - 1)).  alpha lives
//       in LDS as a ring of dur_max + 2 diagonals of u_max + 1 floats, indexed [d % ring][u]; ONE barrier per diagonal (diagonal d + 1 overwrites
//       the slot of d - dur_max - 1, which diagonal d was the last to read).  Thread i takes the cells u = lo + i, lo + i + NT, ... of the
//       diagonal; a cell's 2 D candidates read the source cell's values from memory (L2: 2 + D floats per cell) and its alpha from the ring.
//       Back-pointers: one byte per cell in global memory (the arc's index, 255 = unreachable).  END is evaluated by thread 0 from the alpha of
//       the last kTdtAlignMaxDur frames of columns U - 1 and U, kept in a small LDS table; the back-trace is thread 0 walking the bytes (one
//       dependent load per arc, <= T + U of them), conf[k] = dexpf(lab[start[k]][k]) by all threads afterwards.
//       The walk is written out here and is, line for line, tdt_lattice_walk (tdt_lattice_dev.hpp, which tdt_total_kernel calls) with a max-plus fold
//       and the back-pointer byte: built on that function the kernel measured 1 - 3 % slower at batch shapes (profiles/tdt_lattice_walk.md), so the
//       two are kept apart and a fix to one walk has to be made in the other.
//
// Limits (host side: tdt_align.cpp refuses with PK_ERR_UNSUPPORTED before anything is allocated):
//   durations 0 <= dur[i] <= kTdtAlignMaxDur = 8, 1 <= D <= 8; U_b <= kTdtAlignMaxTokens = 1535 -- from the LDS arithmetic
//   (8 + 2) diagonals x 1536 cells x 4 bytes = 61440 bytes <= the 64 KB a workgroup may take, not from a measurement;
//   scratch of a call <= 1 GiB (formula: tdt_align.hpp).
//
// Code objects (hipcc -O3 --offload-arch=gfx950, from the .s of -save-temps):
//   tdt_align_kernel< 64>       39 VGPR 106 SGPR  LDS 80 B + the ring  scratch 0 B; 0 VGPR spills, 47 SGPRs spilled to VGPR lanes
//   tdt_align_kernel<256>       39 VGPR 106 SGPR  LDS 80 B + the ring  scratch 0 B; 0 VGPR spills, 47 SGPRs spilled to VGPR lanes
//   (the durations and blank steps are wave-uniform and live in SGPRs; the back-trace indexes the durations through the kernel argument, so no
//    array is indexed by a run-time value and nothing goes to private memory)
//   tdt_lattice_act_kernel      46 VGPR  24 SGPR  LDS  0 B             scratch 0 B; 0 VGPR spills, 0 SGPR spills
//   tdt_lattice_keep_kernel     49 VGPR  36 SGPR  LDS  0 B             scratch 0 B; 0 VGPR spills, 0 SGPR spills
//   (the ring: (dur_max + 2) (u_max + 1) 4 bytes of dynamic LDS, 3 KB for 90 tokens and durations up to 4, 61440 bytes at the limits)
#include "decode_dev.hpp"
#include "tdt_lattice_dev.hpp"

namespace pk {

__global__ __launch_bounds__(256) void tdt_lattice_act_kernel(TdtLattice lt, const int *__restrict__ ep_row0, const float *__restrict__ ep,
                                                              const float *__restrict__ pp, int J, int64_t row0, int n, float *__restrict__ z) {
    lattice_act_row<false>(lt, ep_row0, ep, pp, nullptr, 0, J, row0, n, z);
}

__global__ __launch_bounds__(256) void tdt_lattice_keep_kernel(TdtLattice lt, const int *__restrict__ ids, const float *__restrict__ logits, int V,
                                                               int blank, int64_t row0, int n) {
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
    wave_logsoftmax_argmax(x + V, lt.D, lt.dl + r * lt.D, lane);    // (D <= 8: lanes 0 .. D-1 store the duration log-probs)
}

template <int NT>
__global__ __launch_bounds__(NT) void tdt_align_kernel(TdtAlignArgs a) {
    extern __shared__ float ring[];                                 // [dur_max + 2][u_max + 1]
    __shared__ float tail[2][kTdtAlignMaxDur];                      // alpha[T - 8 + j][U - 1 + c]: what END pulls from
    __shared__ int s_end[4];
    const TdtLattice &lt = a.lt;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int T = lt.T[b], i0 = lt.id_off[b], U = lt.id_off[b + 1] - i0, U1 = U + 1, D = lt.D;
    const int64_t c0 = lt.cell_off[b];
    const float *lab = lt.lab + lt.lab_off[b], *blk = lt.blk + c0, *dl = lt.dl + c0 * D;
    unsigned char *bp = a.bp + c0;
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
            float best = NEG;
            int arg = 255;
            if (d == 0) best = 0.0f;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int ts = t - bstep[i];
                if (i < D && ts >= 0) {
                    const int64_t sc = (int64_t)ts * U1 + u;
                    const float w = blk[sc] + dl[sc * D + i];
                    const float cand = ring[slot(bstep[i]) + u] + w;
                    if (cand > best) { best = cand; arg = i; }
                }
            }
            if (u >= 1) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int ts = t - dur[i];
                    if (i < D && ts >= 0) {
                        const int64_t sc = (int64_t)ts * U1 + (u - 1);
                        const float w = lab[(int64_t)ts * U + (u - 1)] + dl[sc * D + i];
                        const float cand = ring[slot(dur[i] + 1) + (u - 1)] + w;
                        if (cand > best) { best = cand; arg = D + i; }
                    }
                }
            }
            cur[u] = best;
            bp[(int64_t)t * U1 + u] = (unsigned char)arg;
            if (u >= U - 1 && t >= t_tail) tail[u - (U - 1)][t - t_tail] = best;
        }
        __syncthreads();
    }
    if (tid == 0) {
        float end = NEG;
        int et = 0, ecode = 255;
        for (int t = t_tail > 0 ? t_tail : 0; t < T; ++t) {
            for (int i = 0; i < D; ++i) {
                if (t + bstep[i] >= T) {
                    const int64_t sc = (int64_t)t * U1 + U;
                    const float cand = tail[1][t - t_tail] + (blk[sc] + dl[sc * D + i]);
                    if (cand > end) { end = cand; et = t; ecode = i; }
                }
            }
            if (U >= 1) {
                for (int i = 0; i < D; ++i) {
                    if (t + dur[i] >= T) {
                        const int64_t sc = (int64_t)t * U1 + (U - 1);
                        const float cand = tail[0][t - t_tail] + (lab[(int64_t)t * U + (U - 1)] + dl[sc * D + i]);
                        if (cand > end) { end = cand; et = t; ecode = D + i; }
                    }
                }
            }
        }
        const int ok = end > NEG ? 1 : 0;
        a.score[b] = end;
        a.ok[b] = ok;
        s_end[0] = ok;
        if (ok) {
            int t = et, u = U, code = ecode;
            for (int guard = 0; guard <= T + U; ++guard) {          // every arc moves to an earlier diagonal: at most T + U of them
                const bool label = code >= D;
                const int i = label ? code - D : code;
                if (label) {
                    if (u == 0) break;                              // (no label arc enters column 0; keeps the stores inside the utterance's arrays)
                    --u;
                    a.start[i0 + u] = t;
                    a.end[i0 + u] = tdt_token_end(t, lt.durations[i], T);      // (through the kernel argument: dur[] / bstep[] are indexed by constants only and stay in registers)
                    a.dur_idx[i0 + u] = i;
                }
                if ((t == 0 && u == 0) || u < 0) break;
                code = bp[(int64_t)t * U1 + u];
                if (code == 255) break;                             // (unreachable from a finite END; keeps the walk inside the lattice)
                const int dc = lt.durations[code >= D ? code - D : code];
                t -= code >= D ? dc : (dc > 1 ? dc : 1);
                if (t < 0) break;
            }
        }
    }
    __syncthreads();
    if (s_end[0]) {
        for (int k = tid; k < U; k += NT) a.conf[i0 + k] = dexpf(lab[(int64_t)a.start[i0 + k] * U + k]);
    }
}

void launch_tdt_lattice_act(const TdtLattice &lt, const int *ep_row0, const float *ep, const float *pp, int J, int64_t row0, int n, float *z, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(tdt_lattice_act_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, lt, ep_row0, ep, pp, J, row0, n, z);
}

void launch_tdt_lattice_keep(const TdtLattice &lt, const int *ids, const float *logits, int V, int blank, int64_t row0, int n, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(tdt_lattice_keep_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, lt, ids, logits, V, blank, row0, n);
}

void launch_tdt_align(const TdtAlignArgs &a, hipStream_t s) {
    const size_t lds = tdt_walk_launch_checks("launch_tdt_align", a.lt, a.u_max, a.dur_max);
    if (a.u_max + 1 <= kTdtAlignThreads[0]) hipLaunchKernelGGL(tdt_align_kernel<64>, dim3(a.lt.B), dim3(64), lds, s, a);
    else hipLaunchKernelGGL(tdt_align_kernel<256>, dim3(a.lt.B), dim3(256), lds, s, a);
}

}  // namespace pk
