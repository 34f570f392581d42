// parakeet.cpp_amd/csrc/kernels/tdt_tree.hip -- the forward-algorithm totals of the token strings of a clip on ONE prefix tree per clip (DESIGN.md
// section 5.5.3a): a lattice column is a tree node (clip, ids[:u]) instead of (hypothesis, u), so a column that several hypotheses share is computed
// once -- its prediction-net row, its joint rows, its kept log-probs and its forward values alpha[t][node].
//
// The specification stays tests/tdt_total_ref.py: every hypothesis's total is, bit for bit, what tdt_total_kernel gives on the chain of columns from
// the root to the hypothesis's end node.  A cell's value depends on its (clip, prefix) alone and is formed by the operations of tdt_lattice_walk in
// their order: a left fold with dlaef from -inf over blank arcs 0 .. D-1 then label arcs 0 .. D-1, each alpha[src] + (x + dl) as two fp32 adds.
//
// Layout (host API included): clip c owns nodes [node_off[c], node_off[c + 1]), node 0 the empty prefix, parent[k] < k, token[k] on the edge into k;
// blk [T][n], dl [T][n][D], lab [T][n - 1] with column k - 1 the log-prob of token[k] at the cell of parent[k].  A chain is tdt_total's packing.
//
//   tdt_tree_total_kernel<NT>  one workgroup of NT threads per clip.  Column = node, anti-diagonal d = t + depth[node]: a blank arc comes from
//       (t - max(dur, 1), node) on diagonal d - max(dur, 1), a label arc from (t - dur, parent) on d - dur - 1, so every predecessor lies on an earlier
//       diagonal.  The nodes are visited in DEPTH order (a host table: s_node / s_parent / s_depth, level starts dstart), so the cells of diagonal d
//       are one contiguous range of that table and thread i takes entries first + i, first + i + NT, ...: the work of a diagonal is its live cells
//       and nothing else.  alpha lives in LDS as a ring of dur_max + 2 diagonals of n_max floats indexed [d % ring][node], ONE barrier per diagonal
//       (diagonal d + 1 overwrites the slot of d - dur_max - 1, which d was the last to read).
//       END is per hypothesis and its end nodes sit at any depth, so alpha of the last max(dur_max, 1) frames of EVERY column outlives the ring in a
//       second LDS table [max(dur_max, 1)][n_max] -- LDS, not global memory: the cell that forms a value stores it twice and END needs no fence.
//       After the walk thread i folds END of hypotheses i, i + NT, ...: frames ascending, blank before label, then by i (5.5.3's order).
//   tdt_tree_act_kernel    z = relu(enc_proj[t] + pred_proj[node]) (joint_act_row) for a chunk of tree-lattice rows, one wave per row.
//   tdt_tree_keep_kernel   one wave per row of the heads product's output [V + D]: wave_row_max_lse and wave_logsoftmax_low8 as
//       tdt_lattice_keep_kernel takes them; the blank's log-prob, the D duration log-probs and one label log-prob per CHILD of the node (CSR) leave.
//   tdt_tree_gather_kernel the prediction net's lock-step by DEPTH: row j of step u takes the (h, c) its parent's row left at step u - 1 (zeros at the root).
//
// Limits (host side: tdt_tree.cpp refuses with PK_ERR_UNSUPPORTED before anything is allocated): n_b <= kTdtTreeMaxNodes = 1536 (the U + 1 limit of the
//   chain walk), durations in [0, 8], 1 <= D <= 8, scratch of a group <= 1 GiB.  LDS at the limits: ring 10 x 1536 x 4 = 61440 bytes + table
//   8 x 1536 x 4 = 49152 bytes = 110592 of the CU's 160 KB (one workgroup per CU there; 3.4 KB for 90 nodes and durations up to 4).
//
// Code objects (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage):
//   tdt_tree_total_kernel< 64>  37 VGPR 106 SGPR  LDS the ring + the kept table  scratch 0 B; 0 VGPR spills, 37 SGPRs spilled to VGPR lanes
//   tdt_tree_total_kernel<256>  37 VGPR 106 SGPR  LDS the ring + the kept table  scratch 0 B; 0 VGPR spills, 37 SGPRs spilled to VGPR lanes
//   (as in tdt_total_kernel the durations and blank steps are wave-uniform and live in SGPRs; nothing goes to private memory)
//   tdt_tree_act_kernel         46 VGPR  26 SGPR  LDS 0 B  scratch 0 B; no spills
//   tdt_tree_keep_kernel        45 VGPR  38 SGPR  LDS 0 B  scratch 0 B; no spills
//   tdt_tree_gather_kernel      16 VGPR  30 SGPR  LDS 0 B  scratch 0 B; no spills
#include "decode_dev.hpp"
#include "tdt_lattice_dev.hpp"

namespace pk {

// (clip, frame, node) of tree-lattice row r = cell_off[c] + t n_c + k
struct TreeRow { int c, t, k, n0, nb; };
__device__ __forceinline__ TreeRow tree_row_of(const TdtTree &tr, int64_t r) {
    TreeRow o;
    o.c = lattice_row_owner(tr.cell_off, tr.C, r);
    o.n0 = tr.node_off[o.c];
    o.nb = tr.node_off[o.c + 1] - o.n0;
    const int64_t q = r - tr.cell_off[o.c];
    o.t = (int)(q / o.nb);
    o.k = (int)(q - (int64_t)o.t * o.nb);
    return o;
}

__global__ __launch_bounds__(256) void tdt_tree_act_kernel(TdtTree tr, const float *__restrict__ ep, const float *__restrict__ pp, int J, int64_t row0, int n,
                                                           float *__restrict__ z) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const TreeRow w = tree_row_of(tr, row0 + i);
    joint_act_row(ep + ((int64_t)tr.row0[w.c] + w.t) * J, pp + (int64_t)tr.ppos[w.n0 + w.k] * J, z + i * J, J, lane);
}

__global__ __launch_bounds__(256) void tdt_tree_keep_kernel(TdtTree tr, const float *__restrict__ logits, int V, int blank, int64_t row0, int n) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int64_t r = row0 + i;
    const TreeRow w = tree_row_of(tr, r);
    const float *x = logits + i * (int64_t)(V + tr.D);
    const RowLse rl = wave_row_max_lse(x, V, lane);
    const float m = rl.m, lse = rl.lse;
    const float dlv = wave_logsoftmax_low8(x + V, tr.D, lane);      // lane l: the duration log-prob of index l & 7
    if (lane < tr.D) tr.dl[r * tr.D + lane] = dlv;
    if (lane == 0) tr.blk[r] = (x[blank] - m) - lse;
    float *labrow = tr.lab + tr.lab_off[w.c] + (int64_t)w.t * (w.nb - 1);
    const int g = w.n0 + w.k;
    for (int j = tr.child_off[g] + lane; j < tr.child_off[g + 1]; j += 64) {
        const int ch = tr.child[j];                                 // clip-local node, >= 1
        labrow[ch - 1] = (x[tr.token[w.n0 + ch]] - m) - lse;
    }
}

// grid (rows of the step, L); h / c [L][stride / Hp][Hp], a row's float4s copied as they lie (h is in the sigma layout: a copy keeps it)
__global__ __launch_bounds__(256) void tdt_tree_gather_kernel(const int *__restrict__ pslot, int Hp, int64_t stride, const float *__restrict__ hs,
                                                              const float *__restrict__ cs, float *__restrict__ hd, float *__restrict__ cd) {
    const int j = blockIdx.x, p = pslot[j];
    const int64_t lo = (int64_t)blockIdx.y * stride;
    float4 *h4 = reinterpret_cast<float4 *>(hd + lo + (int64_t)j * Hp), *c4 = reinterpret_cast<float4 *>(cd + lo + (int64_t)j * Hp);
    if (p < 0) {
        for (int q = threadIdx.x; q < Hp / 4; q += 256) h4[q] = c4[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float4 *hp4 = reinterpret_cast<const float4 *>(hs + lo + (int64_t)p * Hp), *cp4 = reinterpret_cast<const float4 *>(cs + lo + (int64_t)p * Hp);
    for (int q = threadIdx.x; q < Hp / 4; q += 256) { h4[q] = hp4[q]; c4[q] = cp4[q]; }
}

template <int NT>
__global__ __launch_bounds__(NT) void tdt_tree_total_kernel(TdtTreeTotalArgs a) {
    extern __shared__ float lds[];                                  // ring [dur_max + 2][n_max], then kept [max(dur_max, 1)][n_max]
    const TdtTree &tr = a.tr;
    const int c = blockIdx.x, tid = threadIdx.x;
    const int h0 = a.hyp_off[c], h1 = a.hyp_off[c + 1];
    if (h0 == h1) return;                                           // a clip without hypotheses is not walked (uniform: before any barrier)
    const int T = tr.T[c], n0 = tr.node_off[c], nb = tr.node_off[c + 1] - n0, nl = nb - 1, D = tr.D;
    const int64_t c0 = tr.cell_off[c];
    const float *lab = tr.lab + tr.lab_off[c], *blk = tr.blk + c0, *dl = tr.dl + c0 * D;
    const int *s_node = tr.s_node + n0, *s_parent = tr.s_parent + n0, *s_depth = tr.s_depth + n0, *dstart = tr.dstart + n0 + c;
    const int R = a.dur_max + 2, pitch = a.n_max, KT = a.dur_max > 1 ? a.dur_max : 1;
    float *ring = lds, *kept = lds + R * pitch;
    const float NEG = -__builtin_huge_valf();
    int dur[8], bstep[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { dur[i] = i < D ? tr.durations[i] : 1; bstep[i] = dur[i] > 1 ? dur[i] : 1; }
    const int t_tail = T - KT;                                      // kept[t - t_tail][node] for t >= t_tail: every frame END pulls from
    const int depth_max = s_depth[nb - 1];
    int dm = 0;                                                     // d % R, kept by increment: the slot of diagonal d - k is dm - k (+ R when negative)
    auto slot = [&](int k) { const int q = dm - k; return (q < 0 ? q + R : q) * pitch; };
    for (int d = 0; d < T + depth_max; ++d, dm = dm + 1 == R ? 0 : dm + 1) {
        const int lo = d - (T - 1) > 0 ? d - (T - 1) : 0, hi = d < depth_max ? d : depth_max;
        const int last = dstart[hi + 1];
        float *cur = ring + dm * pitch;
        for (int e = dstart[lo] + tid; e < last; e += NT) {
            const int k = s_node[e], p = s_parent[e], t = d - s_depth[e];
            TdtLogSum f;
            if (d == 0) f.v = 0.0f;                                 // (the root at frame 0: the one cell of diagonal 0)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int ts = t - bstep[i];
                if (i < D && ts >= 0) {
                    const int64_t sc = (int64_t)ts * nb + k;
                    const float w = blk[sc] + dl[sc * D + i];
                    f.take(ring[slot(bstep[i]) + k] + w, i);
                }
            }
            if (p >= 0) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int ts = t - dur[i];
                    if (i < D && ts >= 0) {
                        const int64_t sc = (int64_t)ts * nb + p;
                        const float w = lab[(int64_t)ts * nl + (k - 1)] + dl[sc * D + i];
                        f.take(ring[slot(dur[i] + 1) + p] + w, D + i);
                    }
                }
            }
            cur[k] = f.v;
            if (t >= t_tail) kept[(t - t_tail) * pitch + k] = f.v;
        }
        __syncthreads();
    }
    for (int h = h0 + tid; h < h1; h += NT) {
        const int e = a.hyp_end[h], p = tr.parent[n0 + e];
        TdtLogSum end;
        for (int t = t_tail > 0 ? t_tail : 0; t < T; ++t) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (i < D && t + bstep[i] >= T) {
                    const int64_t sc = (int64_t)t * nb + e;
                    end.take(kept[(t - t_tail) * pitch + e] + (blk[sc] + dl[sc * D + i]), i);
                }
            }
            if (p >= 0) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    if (i < D && t + dur[i] >= T) {
                        const int64_t sc = (int64_t)t * nb + p;
                        end.take(kept[(t - t_tail) * pitch + p] + (lab[(int64_t)t * nl + (e - 1)] + dl[sc * D + i]), D + i);
                    }
                }
            }
        }
        a.total[h] = end.v;
        a.ok[h] = end.v > NEG ? 1 : 0;
    }
}

void launch_tdt_tree_act(const TdtTree &tr, const float *ep, const float *pp, int J, int64_t row0, int n, float *z, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(tdt_tree_act_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, tr, ep, pp, J, row0, n, z);
}

void launch_tdt_tree_keep(const TdtTree &tr, const float *logits, int V, int blank, int64_t row0, int n, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(tdt_tree_keep_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, tr, logits, V, blank, row0, n);
}

void launch_tdt_tree_gather(const int *pslot, int n, int L, int Hp, int64_t stride, const float *hs, const float *cs, float *hd, float *cd, hipStream_t s) {
    if (n <= 0) return;
    if (Hp % 4 != 0) { fprintf(stderr, "parakeet_amd: internal error: launch_tdt_tree_gather: pred_hidden %d is no multiple of 4\n", Hp); abort(); }
    hipLaunchKernelGGL(tdt_tree_gather_kernel, dim3(n, L), dim3(256), 0, s, pslot, Hp, stride, hs, cs, hd, cd);
}

size_t tdt_tree_total_lds_bytes(int n_max, int dur_max) { return (size_t)(dur_max + 2 + (dur_max > 1 ? dur_max : 1)) * n_max * sizeof(float); }

void launch_tdt_tree_total(const TdtTreeTotalArgs &a, hipStream_t s) {
    if (a.dur_max < 0 || a.dur_max > kTdtAlignMaxDur || a.n_max < 1 || a.n_max > kTdtTreeMaxNodes || a.tr.D < 1 || a.tr.D > 8) {
        fprintf(stderr, "parakeet_amd: internal error: launch_tdt_tree_total outside the kernel's limits (dur_max %d, n_max %d, D %d)\n", a.dur_max, a.n_max, a.tr.D);
        abort();
    }
    if (a.tr.C <= 0) return;
    const size_t lds = tdt_tree_total_lds_bytes(a.n_max, a.dur_max);
    static DynLdsSlots slots64, slots256;
    if (a.n_max <= kTdtAlignThreads[0]) {
        ensure_dyn_lds(slots64, reinterpret_cast<const void *>(&tdt_tree_total_kernel<64>), lds);
        hipLaunchKernelGGL(tdt_tree_total_kernel<64>, dim3(a.tr.C), dim3(64), lds, s, a);
    } else {
        ensure_dyn_lds(slots256, reinterpret_cast<const void *>(&tdt_tree_total_kernel<256>), lds);
        hipLaunchKernelGGL(tdt_tree_total_kernel<256>, dim3(a.tr.C), dim3(256), lds, s, a);
    }
}

}  // namespace pk
