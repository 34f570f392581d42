// parakeet.cpp_amd/csrc/kernels/rnnt_lattice.hip -- forced alignment and forward-algorithm total of a GIVEN token string under the plain RNN-T
// head, on the device.
//
// The specification is tests/rnnt_lattice_ref.py: the T x (U + 1) lattice of joint evaluations (frame t, prediction net after ids[:u]), blank arc
// to (t + 1, u) with weight blk[t][u], label arc to (t, u + 1) with weight lab[t][u], END = the blank out of (T - 1, U).  Pull form, candidates
// blank from (t - 1, u) then label from (t, u - 1), each fl(alpha[src] + x); max-plus with a strict > (the alignment) or a left fold with dlaef
// (the total).  Every value is compared bit for bit.
//
//   rnnt_walk_kernel<FOLD, MULTI>   one workgroup per utterance, advancing by anti-diagonals d = t + u.  Thread u owns COLUMN u for the whole
//       walk: at step d its cell is (d - u, u).  Both predecessors of a cell lie on diagonal d - 1, so no ring of diagonals exists: a thread keeps
//       the two values that LEAVE its last cell, ob = fl(alpha + blk[t][u]) (the blank candidate of its own next cell) and ol = fl(alpha +
//       lab[t][u]) (the label candidate of its right neighbour's next cell), in two VGPRs.  A step is: ol of lane u - 1 by ONE v_mov_b32 with the
//       DPP modifier wave_shr:1 (lane 0 keeps the "old" operand, -inf), the fold of the two candidates, the two adds that form the new ob / ol.
//       alpha itself is never stored.  A cell outside the lattice (t < 0, t >= T, u > U) is -inf, which neither fold takes, so the candidates
//       need no predicate: a thread that has not started, or has finished, carries -inf.
//       MULTI = false (U + 1 <= 64): one wave, no LDS, no barrier.  MULTI = true (up to 16 waves, U <= kRnntMaxTokens = 1023): the one value
//       that crosses a wave boundary -- ol of lane 63 -- goes through xl[2][16] floats of LDS, double-buffered by the parity of d, ONE barrier
//       per diagonal (step d writes xl[d & 1] before the barrier, step d + 1 reads it after, step d + 2 writes it again behind barrier d + 1).
//       Lattice values: thread u reads blk[t][u] and lab[t][u] of its own column, t = d - u: consecutive steps are U + 1 resp. U floats apart
//       and no address depends on alpha.  They are requested kRnntPipe = 16 diagonals ahead into a register ring (2 x 16 VGPRs, indexed by the
//       unrolled step, so by constants).  Why 16: the dependent chain of a max-plus step is the DPP move, a compare, a select and an add, about
//       40 clocks for one wave, and a load that misses the vector cache but hits L2 -- the keep kernel has just written the lattice -- returns in
//       500 - 700 clocks; 16 steps cover that, and 32 loads in flight stay under the 6-bit vmcnt counter's 63.  The log-sum step is several times
//       longer (dexpf, dlogf) and is covered with room to spare.  Lanes of one wave touch 64 different cache lines per load, but the line lane u
//       reads at step d is the line lane u + 1 reads at step d + 1: every line is fetched from L2 once per wave and reused from the vector cache.
//       Back-pointers (FOLD = max): ONE BIT per cell, 1 = the label arc.  A thread collects the bits of 32 consecutive frames of its column in a
//       VGPR and stores the dword with a plain vector store when t & 31 == 31 or t == T - 1: layout [u][ceil(T / 32)] dwords per utterance, 1/8
//       of the TDT walk's byte per cell, and every dword of the utterance's block is written.
//       END = ob of thread U after the last step -> value[b]; the log-sum form also writes ok[b].
//   rnnt_trace_kernel               one thread per utterance: ok[b] = score[b] > -inf (score is value[b] as the walk left it), then from (T - 1, U)
//       back to (0, 0) along the bits.  The current dword stays in a register and is reloaded only when the column changes or t crosses a
//       multiple of 32: U + T / 32 dependent loads, not T + U.  Token k leaving at frame t: start[k] = end[k] = t, conf[k] = dexpf(lab[t][k]).
//   rnnt_lattice_keep_kernel        one wave per row of the heads product's output [V]: wave_row_max_lse (the decision kernel's canonical
//       log-softmax) and two values leave, the blank's log-prob and that of ids[u].  tdt_lattice_keep_kernel cannot be launched with D = 0 (its
//       duration log-softmax reads logits[V ..]), so the RNN-T keep lives here; the activation rows are tdt_lattice_act_kernel's, unchanged.
//
// Limits (host side: rnnt_lattice.cpp refuses with PK_ERR_UNSUPPORTED before anything is allocated): U_b <= kRnntMaxTokens = 1023 (one thread per
//   column, 1024 threads per workgroup); scratch of a call or of a group of hypotheses <= 1 GiB (formula: rnnt_lattice.hpp).
//
// Code objects (hipcc -O3 --offload-arch=gfx950, from the .s of -save-temps):
//   rnnt_walk_kernel<max, one wave>     112 VGPR  34 SGPR  LDS   0 B  scratch 0 B; 0 VGPR spills, 0 SGPR spills
//   rnnt_walk_kernel<max, 16 waves>     111 VGPR  35 SGPR  LDS 128 B  scratch 0 B; 0 VGPR spills, 0 SGPR spills
//   rnnt_walk_kernel<sum, one wave>      96 VGPR  41 SGPR  LDS   0 B  scratch 0 B; 0 VGPR spills, 0 SGPR spills
//   rnnt_walk_kernel<sum, 16 waves>      97 VGPR  45 SGPR  LDS 128 B  scratch 0 B; 0 VGPR spills, 0 SGPR spills
//   rnnt_trace_kernel                    25 VGPR  30 SGPR  LDS   0 B  scratch 0 B; 0 VGPR spills, 0 SGPR spills
//   rnnt_lattice_keep_kernel             45 VGPR  31 SGPR  LDS   0 B  scratch 0 B; 0 VGPR spills, 0 SGPR spills
//   (the register ring is 32 of the walk's VGPRs, the 64-bit addresses of the 32 loads in flight most of the rest; 112 <= the 128 a workgroup of
//    1024 threads may take per lane; each walk holds 16 wave_shr:1 moves, one per unrolled step, and the 16-wave forms 16 s_barrier)
#include "decode_dev.hpp"
#include "tdt_lattice_dev.hpp"

namespace pk {

constexpr int kRnntPipe = 16;                   // diagonals a cell's two lattice values are requested ahead of their use

// the value of lane - 1; lane 0 of the wave keeps edge
__device__ __forceinline__ float lane_below_f(float x, float edge) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(x), 0x138, 0xF, 0xF, false));      // wave_shr:1
}

template <int FOLD, bool MULTI>
__global__ __launch_bounds__(MULTI ? 1024 : 64) void rnnt_walk_kernel(RnntWalkArgs a) {
    __shared__ float xl[2][16];                                     // [d & 1][wave]: ol of lane 63 (MULTI only)
    const TdtLattice &lt = a.lt;
    const int b = blockIdx.x, u = threadIdx.x, lane = u & 63, w = u >> 6;
    const int T = lt.T[b], U = lt.id_off[b + 1] - lt.id_off[b], U1 = U + 1;
    const float *blk = lt.blk + lt.cell_off[b], *lab = lt.lab + lt.lab_off[b];
    const int W32 = (T + 31) >> 5;
    unsigned *bits = nullptr;
    if constexpr (FOLD == RNNT_FOLD_MAX) bits = a.bits + a.bits_off[b] + (int64_t)u * W32;     // (dereferenced by columns u <= U only)
    const float NEG = -__builtin_huge_valf();
    const bool col = u <= U, lcol = u < U;
    const int n_diag = T + U;
    // the two lattice values of this column's cell on diagonal d; -inf outside the lattice (and for lab in column U, which has no label arc)
    auto fetch = [&](int d, float &xb, float &xlab) {
        const int t = d - u;
        xb = NEG; xlab = NEG;
        if (col && t >= 0 && t < T) {
            xb = blk[(int64_t)t * U1 + u];
            if (lcol) xlab = lab[(int64_t)t * U + u];
        }
    };
    float rb[kRnntPipe], rl[kRnntPipe];
#pragma unroll
    for (int j = 0; j < kRnntPipe; ++j) fetch(j, rb[j], rl[j]);
    float ob = NEG, ol = NEG;
    unsigned word = 0;
    for (int d0 = 0; d0 < n_diag; d0 += kRnntPipe) {
#pragma unroll
        for (int j = 0; j < kRnntPipe; ++j) {
            const int d = d0 + j;
            if (d < n_diag) {                                       // (uniform over the workgroup: the DPP move and the barrier see every lane)
                const int t = d - u;
                float left = lane_below_f(ol, NEG);
                if constexpr (MULTI) {
                    if (lane == 0 && w > 0 && d > 0) left = xl[(d + 1) & 1][w - 1];     // written by step d - 1 (at d = 0 nothing is: the cell is outside the lattice)
                }
                float al;
                bool label = false;
                if constexpr (FOLD == RNNT_FOLD_MAX) {
                    label = left > ob;
                    al = label ? left : ob;
                } else {
                    al = dlaef(ob, left);                           // (= dlaef(dlaef(-inf, ob), left) bit for bit)
                }
                const bool inside = col && t >= 0 && t < T;
                if (d == 0 && u == 0) al = 0.0f;
                if (!inside) al = NEG;
                ob = al + rb[j];
                ol = al + rl[j];
                if constexpr (FOLD == RNNT_FOLD_MAX) {
                    if (inside) {
                        word |= (label ? 1u : 0u) << (t & 31);
                        if ((t & 31) == 31 || t == T - 1) { bits[t >> 5] = word; word = 0; }
                    }
                }
                fetch(d + kRnntPipe, rb[j], rl[j]);
                if constexpr (MULTI) {
                    if (lane == 63) xl[d & 1][w] = ol;
                    __syncthreads();
                }
            }
        }
    }
    if (u == U) {                                                   // its last cell was (T - 1, U) on the last diagonal: ob is END
        a.value[b] = ob;
        if constexpr (FOLD == RNNT_FOLD_SUM) a.ok[b] = ob > NEG ? 1 : 0;
    }
}

__global__ __launch_bounds__(64) void rnnt_trace_kernel(RnntWalkArgs a) {
    const TdtLattice &lt = a.lt;
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= lt.B) return;
    const int ok = a.value[b] > -__builtin_huge_valf() ? 1 : 0;
    a.ok[b] = ok;
    if (!ok) return;
    const int T = lt.T[b], i0 = lt.id_off[b], U = lt.id_off[b + 1] - i0;
    const int W32 = (T + 31) >> 5;
    const float *lab = lt.lab + lt.lab_off[b];
    const unsigned *bits = a.bits + a.bits_off[b];
    int t = T - 1, u = U;
    unsigned word = bits[(int64_t)u * W32 + (t >> 5)];
    for (int guard = 0; guard < T + U && (t | u) != 0; ++guard) {   // every arc moves to the diagonal before: T + U - 1 of them
        if ((word >> (t & 31)) & 1u) {
            if (u == 0) break;                                      // (no label arc enters column 0; keeps the stores inside the utterance's arrays)
            --u;
            a.start[i0 + u] = t;
            a.end[i0 + u] = t;
            a.conf[i0 + u] = dexpf(lab[(int64_t)t * U + u]);
            word = bits[(int64_t)u * W32 + (t >> 5)];
        } else {
            if (t == 0) break;                                      // (unreachable from a finite END; keeps the walk inside the lattice)
            --t;
            if ((t & 31) == 31) word = bits[(int64_t)u * W32 + (t >> 5)];
        }
    }
}

__global__ __launch_bounds__(256) void rnnt_lattice_keep_kernel(TdtLattice lt, const int *__restrict__ ids, const float *__restrict__ logits, int V,
                                                                int blank, int64_t row0, int n) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int64_t r = row0 + i;
    const int b = lattice_row_owner(lt.cell_off, lt.B, r);
    const int U = lt.id_off[b + 1] - lt.id_off[b], U1 = U + 1;
    const int64_t c = r - lt.cell_off[b];
    const int t = (int)(c / U1), u = (int)(c - (int64_t)t * U1);
    const float *x = logits + i * (int64_t)V;
    const RowLse rl = wave_row_max_lse(x, V, lane);
    if (lane == 0) lt.blk[r] = (x[blank] - rl.m) - rl.lse;
    if (lane == 1 && u < U) lt.lab[lt.lab_off[b] + (int64_t)t * U + u] = (x[ids[lt.id_off[b] + u]] - rl.m) - rl.lse;
}

void launch_rnnt_lattice_keep(const TdtLattice &lt, const int *ids, const float *logits, int V, int blank, int64_t row0, int n, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(rnnt_lattice_keep_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, lt, ids, logits, V, blank, row0, n);
}

void launch_rnnt_walk(const RnntWalkArgs &a, int fold, hipStream_t s) {
    if (a.u_max < 0 || a.u_max > kRnntMaxTokens || a.lt.D != 0 || (fold != RNNT_FOLD_MAX && fold != RNNT_FOLD_SUM)) {
        fprintf(stderr, "parakeet_amd: internal error: launch_rnnt_walk outside the kernel's limits (u_max %d, D %d, fold %d)\n", a.u_max, a.lt.D, fold);
        abort();
    }
    if (a.lt.B <= 0) return;
    const dim3 g(a.lt.B), wide(64 * ((a.u_max + 1 + 63) / 64));
    const bool mx = fold == RNNT_FOLD_MAX;
    if (a.u_max + 1 <= 64) {
        if (mx) hipLaunchKernelGGL((rnnt_walk_kernel<RNNT_FOLD_MAX, false>), g, dim3(64), 0, s, a);
        else hipLaunchKernelGGL((rnnt_walk_kernel<RNNT_FOLD_SUM, false>), g, dim3(64), 0, s, a);
    } else {
        if (mx) hipLaunchKernelGGL((rnnt_walk_kernel<RNNT_FOLD_MAX, true>), g, wide, 0, s, a);
        else hipLaunchKernelGGL((rnnt_walk_kernel<RNNT_FOLD_SUM, true>), g, wide, 0, s, a);
    }
}

void launch_rnnt_trace(const RnntWalkArgs &a, hipStream_t s) {
    if (a.lt.B <= 0) return;
    hipLaunchKernelGGL(rnnt_trace_kernel, dim3((unsigned)((a.lt.B + 63) / 64)), dim3(64), 0, s, a);
}

}  // namespace pk
