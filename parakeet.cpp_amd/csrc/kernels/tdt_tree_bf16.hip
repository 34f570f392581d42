// parakeet.cpp_amd/csrc/kernels/tdt_tree_bf16.hip -- the PREFIX-TREE TDT lattice of the TOLERANCE-class mode (pk_config.gemm_bf16 with
// pk_model_set_tdt_lattice_bf16 and pk_model_set_tdt_total_shared): ONE launch takes the joint of every tree-lattice row of
// a group of clips from enc_proj and the prediction net's rows to the values tdt_tree_total_kernel reads.  No activation row and no logits row ever
// reaches memory.
//
// For tree-lattice row r = cell_off[c] + t n_c + k (the numbering of tree_row_of in tdt_tree.hip), n0 = node_off[c]:
//     z[j]     = bf16_rne(s > 0 ? s : 0),  s = fl32(ep[row0[c] + t][j] + pp[ppos[n0 + k]][j])
//     logit[n] = fl32-accumulated sum_j z[j] W16[n][j] on v_mfma_f32_32x32x16_bf16, + bld[n] in fp32;  W16 = bf16_rne(wld)
//     blk[r] = logit[blank] - lse_V,  dl[r][i] = logit[V + i] - lse_D
//     lab[lab_off[c] + t (n_c - 1) + ch - 1] = logit[token[n0 + ch]] - lse_V   for EVERY child ch of node k
//
// Contract.  A value depends on its own (ep row, pp row, column) alone and is formed by the operations of tdt_lattice_bf16_kernel in their order, so
// blk / dl / lab are BIT-EQUAL to what that kernel gives for the same (frame, prefix) on any chain through the node, and the totals of the tree walk
// equal the unshared ones bit for bit in this mode too.  Steps 2 to 5 below are therefore that kernel's, statement for statement: the transposed
// contraction (weight columns x lattice rows), the waves on disjoint quarters of the weight stream through the four-step register ring, z in LDS in
// MFMA fragment order, no barrier between the z build and the end of the walk, the per-lane running (max, sum) with rescaling, the 8-partial merge.
// They are a COPY, not a shared header: with steps 2 to 5 moved into a device header and the capture as a template policy the chain kernel computed
// the same bits but took 4 more VGPRs in every form (<4> 508 -> 512, <3> 426 -> 430, <2> 328 -> 332; no spills, scratch 0 either way), so the chain
// kernel is left exactly as it was.  tests/test_gpu_tdt_tree_bf16.py holds the two to each other bit for bit.
//
// What is new.
//   1. Row decode: threads 0 .. R-1 find (clip, t, node) by bisection over cell_off and write the LDS row tables -- the ep row row0[c] + t, the pp
//      row ppos[n0 + k], the node's range [cbeg, cend) in the children table and the first word of the row's lab values.
//   4. Multi-column capture.  A chain row wants one label column, held in a register; a tree row wants one per child, 0 .. n_c - 1 of them.  The host
//      stages every node's children SORTED BY TOKEN (child_s / child_tok beside child_off; siblings' tokens are distinct), and a wave's column
//      blocks ascend (w, w + 4, ...), so each lane keeps ONE monotone cursor per row into that list: after a block's 32 biased logits are formed it
//      visits the children whose token lies below the block's end -- those below its start belong to another wave's block and are skipped, those
//      inside are taken by the lane half (g) whose accumulator registers hold the column, selected out of the 32 values by an unrolled compare
//      chain -- and stores the RAW logit to the child's final lab word.  After the merge barrier thread i < R walks row i's children once more and
//      subtracts the row's lse in place (fl(logit - lse): the chain kernel's subtraction).  The writer and the reader are in one workgroup: a
//      block-scope fence before the barrier orders them.  Nothing per child lives in LDS or registers, so a node's fan-out is bounded by the tree's
//      own limit (kTdtTreeMaxNodes) alone.  On a chain (one child per row) the cursor costs one compare per block and one table read per row.
//
// LDS beside z per row is 124 bytes as in the chain kernel (16 partials, 9 captures -- blank and 8 durations --, 4 ints and lab's base), so
// tdt_tree_bf16_rows is tdt_lattice_bf16_rows: 128 rows up to J = 512, 96 up to J = 736 (tdt-600m: 640), 64 up to J = 1120.
//
// Bounds: row tables are written for all R rows (past the last row: pp row -1, which zero-fills z, and an empty child range); z index < RS (J / 16) 64;
// captures [9][R], D <= 8; the weight stream of wave w ends inside block NCB - 1 of the packed copy (the ring re-reads its last step); bld is read at
// c < V + D only; a cursor stays inside [cbeg, cend] and reads child_tok / child_s below cend only; lab words are those of the row's own children.
//
// Limits (launcher): J % 32 == 0 and J <= 1120, 1 <= D <= 8, 0 <= blank < V; tokens in [0, V) (the host checks them).
//
// Code objects (hipcc -O3 --offload-arch=gfx950, from the .s of -save-temps):
//   tdt_tree_lattice_bf16_kernel<4>   508 VGPR 106 SGPR  LDS 0 B + 128 (2 J + 124) dynamic  scratch 0 B; 0 VGPR spills, 7 SGPRs spilled to VGPR lanes
//   tdt_tree_lattice_bf16_kernel<3>   434 VGPR 106 SGPR  LDS 0 B +  96 (2 J + 124) dynamic  scratch 0 B; 0 VGPR spills, 9 SGPRs spilled to VGPR lanes
//   tdt_tree_lattice_bf16_kernel<2>   336 VGPR 106 SGPR  LDS 0 B +  64 (2 J + 124) dynamic  scratch 0 B; 0 VGPR spills, 7 SGPRs spilled to VGPR lanes
//   (the chain kernel's 508 / 426 / 328 with the cursor and its token per row subtile in place of the one wanted column; one workgroup per CU)
#include "../pk_devmath.h"
#include "kernels.hpp"
#include "tdt_lattice_dev.hpp"

namespace pk {

typedef float tt_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 tt_bf16x8 __attribute__((ext_vector_type(8)));

static constexpr int TT_ROW_BYTES = 124;            // LDS beside z per lattice row: 16 partials, 9 captures, 4 ints and lab's base
static constexpr size_t TT_LDS_MAX = 150 * 1024;    // (the cap of tdt_lattice_bf16.hip and the bf16 attention kernels)
static constexpr int TT_NONE = 0x7FFFFFFF;          // "no child left": above every column

__device__ __forceinline__ int tt_rowidx(int r, int g) { return (r & 3) + 8 * (r >> 2) + 4 * g; }     // row of accumulator register r (32x32 C layout)

template <int RS>
__global__ __launch_bounds__(256) void tdt_tree_lattice_bf16_kernel(TdtTreeLatticeBf16Args a) {
    constexpr int R = 32 * RS;
    constexpr float L2E = 1.44269502162933349609375f;
    extern __shared__ __attribute__((aligned(16))) unsigned char tt_smem[];
    const TdtTree &tr = a.tr;
    const int J = a.J, KS = J >> 4, V = a.V, D = tr.D, VD = V + D, blank = a.blank;
    tt_bf16x8 *zL = reinterpret_cast<tt_bf16x8 *>(tt_smem);                         // [RS][KS][64]
    float *part = reinterpret_cast<float *>(tt_smem + (size_t)R * J * 2);           // [4 waves][2 halves][m, s][R]
    float *cap = part + 16 * R;                                                     // [blank, D durations (8)][R]
    int64_t *labr = reinterpret_cast<int64_t *>(cap + 9 * R);                       // [R] first lab word of the row: child ch is word labr + ch - 1
    int *epr = reinterpret_cast<int *>(labr + R), *ppr = epr + R;                   // [R] each: ep row, pp row (-1 past the last row)
    int *cbeg = ppr + R, *cend = cbeg + R;                                          // [R] each: the node's children are entries [cbeg, cend) of child_s / child_tok
    const float NEG = -__builtin_huge_valf();

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 31, g = lane >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * R;

    if (tid < R) {                                                  // 1. the rows of this tile
        const int64_t r = row0 + tid;
        int e = -1, p = -1, cb = 0, ce = 0;
        int64_t lr = 0;
        if (r < a.cells) {
            const int c = lattice_row_owner(tr.cell_off, tr.C, r);
            const int n0 = tr.node_off[c], nb = tr.node_off[c + 1] - n0;
            const int64_t q = r - tr.cell_off[c];
            const int t = (int)(q / nb), k = (int)(q - (int64_t)t * nb);
            e = tr.row0[c] + t;
            p = tr.ppos[n0 + k];
            cb = tr.child_off[n0 + k]; ce = tr.child_off[n0 + k + 1];
            lr = tr.lab_off[c] + (int64_t)t * (nb - 1);
        }
        epr[tid] = e; ppr[tid] = p; cbeg[tid] = cb; cend[tid] = ce; labr[tid] = lr;
    }
    __syncthreads();
    {                                                               // 2. z, fragment order; chunk q: row q % 32 of subtile st, k chunk ch of 8
        const int NCH = J >> 3;
        for (int q = tid; q < R * NCH; q += 256) {
            const int rn = q & 31, rest = q >> 5, ch = rest % NCH, st = rest / NCH, row = 32 * st + rn;
            tt_bf16x8 v;
            if (ppr[row] >= 0) {
                const float4 *e4 = reinterpret_cast<const float4 *>(a.ep + (int64_t)epr[row] * J + 8 * ch);
                const float4 *p4 = reinterpret_cast<const float4 *>(a.pp + (int64_t)ppr[row] * J + 8 * ch);
                const float4 e0 = e4[0], e1 = e4[1], p0 = p4[0], p1 = p4[1];
                const float s[8] = {e0.x + p0.x, e0.y + p0.y, e0.z + p0.z, e0.w + p0.w, e1.x + p1.x, e1.y + p1.y, e1.z + p1.z, e1.w + p1.w};
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = (__bf16)(s[k] > 0.0f ? s[k] : 0.0f);
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = (__bf16)0.0f;
            }
            zL[((int64_t)st * KS + (ch >> 1)) * 64 + 32 * (ch & 1) + rn] = v;
        }
    }
    __syncthreads();

    // 3. / 4. this wave's column blocks
    const tt_bf16x8 *W = static_cast<const tt_bf16x8 *>(a.w16);
    const int NCB = (VD + 63) >> 6;
    const int nblk = wave < NCB ? (NCB - wave + 3) >> 2 : 0;
    float m_run[RS], s_run[RS];
    int cur[RS], nt[RS];                                            // the lane's cursor into row 32 st + n's children and the token there (TT_NONE: none left)
#pragma unroll
    for (int st = 0; st < RS; ++st) {
        m_run[st] = NEG; s_run[st] = 0.0f;
        cur[st] = cbeg[32 * st + n];
        nt[st] = cur[st] < cend[32 * st + n] ? a.child_tok[cur[st]] : TT_NONE;
    }

    if (nblk > 0) {
        // the wave's weight stream: step (block, ks) is 128 vectors, a block KS steps, the wave's next block 4 blocks on.  Past the last step the
        // ring re-reads the last one.
        const int total = nblk * KS;
        const tt_bf16x8 *pf = W + (int64_t)wave * KS * 128 + lane;
        int pf_i = 0, pf_ks = 0;
        auto fetch = [&](tt_bf16x8 (&dst)[2]) {
            dst[0] = pf[0];
            dst[1] = pf[64];
            if (pf_i + 1 < total) {
                ++pf_i;
                if (++pf_ks == KS) { pf_ks = 0; pf += (int64_t)3 * KS * 128 + 128; }
                else pf += 128;
            }
        };
        tt_bf16x8 a0[2], a1[2], a2[2], a3[2];
        fetch(a0); fetch(a1); fetch(a2); fetch(a3);
        for (int bi = 0; bi < nblk; ++bi) {
            tt_f32x16 acc[2][RS];
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int st = 0; st < RS; ++st)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[h][st][r] = 0.0f;
            for (int ks = 0; ks < KS; ++ks) {
                const tt_bf16x8 *zp = zL + ks * 64 + lane;
#pragma unroll
                for (int st = 0; st < RS; ++st) {
                    const tt_bf16x8 zb = zp[st * KS * 64];
                    acc[0][st] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[0], zb, acc[0][st], 0, 0, 0);
                    acc[1][st] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[1], zb, acc[1][st], 0, 0, 0);
                }
                a0[0] = a1[0]; a0[1] = a1[1]; a1[0] = a2[0]; a1[1] = a2[1]; a2[0] = a3[0]; a2[1] = a3[1];
                fetch(a3);
            }
            // the block's 64 columns c0 + 32 h + tt_rowidx(r, g) of the lane's RS rows
            const int c0 = 64 * (wave + 4 * bi);
            const bool pure = c0 + 64 <= V;                         // (wave-uniform) label columns only
            const bool has_blank = blank >= c0 && blank < c0 + 64;
            float bv[2][16];
            if (pure) {
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float4 b4 = *reinterpret_cast<const float4 *>(a.bld + c0 + 32 * h + 8 * k + 4 * g);
                        bv[h][4 * k] = b4.x; bv[h][4 * k + 1] = b4.y; bv[h][4 * k + 2] = b4.z; bv[h][4 * k + 3] = b4.w;
                    }
            } else {
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int c = c0 + 32 * h + tt_rowidx(r, g);
                        bv[h][r] = a.bld[c < VD ? c : VD - 1];      // (a padding column is masked below)
                    }
            }
#pragma unroll
            for (int st = 0; st < RS; ++st) {
                const int row = 32 * st + n;
                float x[2][16];
                float bm = NEG;
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int c = c0 + 32 * h + tt_rowidx(r, g);
                        float v = acc[h][st][r] + bv[h][r];
                        if (!pure) {
                            if (c >= V && c < VD) cap[(1 + c - V) * R + row] = v;
                            if (c >= V) v = NEG;
                        }
                        if (has_blank && c == blank) cap[row] = v;
                        x[h][r] = v;
                        bm = fmaxf(bm, v);
                    }
                // the row's children up to the end of this block: column w = 32 h + tt_rowidx(r, g') of the block sits in register (h, r) of lane
                // half g' = (w >> 2) & 1, r = (w & 3) + 4 ((w & 31) >> 3)
                while (nt[st] < c0 + 64) {
                    const int w = nt[st] - c0;
                    if (w >= 0 && ((w >> 2) & 1) == g) {
                        const int sel = 16 * (w >> 5) + (w & 3) + 4 * ((w & 31) >> 3);
                        float v = 0.0f;
#pragma unroll
                        for (int h = 0; h < 2; ++h)
#pragma unroll
                            for (int r = 0; r < 16; ++r) v = sel == 16 * h + r ? x[h][r] : v;
                        tr.lab[labr[row] + a.child_s[cur[st]] - 1] = v;
                    }
                    ++cur[st];
                    nt[st] = cur[st] < cend[row] ? a.child_tok[cur[st]] : TT_NONE;
                }
                const float m_new = fmaxf(m_run[st], bm);
                const float msub = m_new > NEG ? m_new : 0.0f;      // no label column seen yet: every term below is exp2(-inf) = 0
                float bs = 0.0f;
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int r = 0; r < 16; ++r) bs += __builtin_amdgcn_exp2f((x[h][r] - msub) * L2E);
                s_run[st] = s_run[st] * __builtin_amdgcn_exp2f((m_run[st] - msub) * L2E) + bs;
                m_run[st] = m_new;
            }
        }
    }
#pragma unroll
    for (int st = 0; st < RS; ++st) {
        float *p = part + (size_t)(wave * 2 + g) * 2 * R + 32 * st + n;
        p[0] = m_run[st];
        p[R] = s_run[st];
    }
    __threadfence_block();                                          // the raw lab words above, before a thread of another wave reads them below
    __syncthreads();

    if (tid < R && ppr[tid] >= 0) {                                 // 5. row tid of the tile
        const int64_t r = row0 + tid;
        float M = NEG;
#pragma unroll
        for (int p = 0; p < 8; ++p) M = fmaxf(M, part[(size_t)p * 2 * R + tid]);
        float S = 0.0f;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const float mp = part[(size_t)p * 2 * R + tid];
            if (mp > NEG) S += part[(size_t)p * 2 * R + R + tid] * dexpf(mp - M);
        }
        const float lse = M + dlogf(S);
        tr.blk[r] = cap[tid] - lse;
        float *lab = tr.lab + labr[tid] - 1;
        for (int j = cbeg[tid]; j < cend[tid]; ++j) {
            const int ch = a.child_s[j];
            lab[ch] = lab[ch] - lse;
        }
        float dm = NEG;
        for (int i = 0; i < D; ++i) dm = fmaxf(dm, cap[(1 + i) * R + tid]);
        float ds = 0.0f;
        for (int i = 0; i < D; ++i) ds += dexpf(cap[(1 + i) * R + tid] - dm);
        const float lse_d = dm + dlogf(ds);
        for (int i = 0; i < D; ++i) tr.dl[r * D + i] = cap[(1 + i) * R + tid] - lse_d;
    }
}

static size_t tt_lds_bytes(int J, int rs) { return (size_t)32 * rs * ((size_t)J * 2 + TT_ROW_BYTES); }

int tdt_tree_bf16_rows(int J) {
    if (J <= 0 || J % 32) return 0;
    for (int rs = 4; rs >= 2; --rs)
        if (tt_lds_bytes(J, rs) <= TT_LDS_MAX) return 32 * rs;
    return 0;
}

template <int RS>
static void tt_launch(const TdtTreeLatticeBf16Args &a, hipStream_t s) {
    auto kern = &tdt_tree_lattice_bf16_kernel<RS>;
    static DynLdsSlots slots;
    const size_t lds = tt_lds_bytes(a.J, RS);
    ensure_dyn_lds(slots, reinterpret_cast<const void *>(kern), lds);
    hipLaunchKernelGGL(kern, dim3((unsigned)((a.cells + 32 * RS - 1) / (32 * RS))), dim3(256), lds, s, a);
}

void launch_tdt_tree_lattice_bf16(const TdtTreeLatticeBf16Args &a, hipStream_t s) {
    const int rows = tdt_tree_bf16_rows(a.J);
    if (rows == 0 || a.tr.D < 1 || a.tr.D > 8 || a.blank < 0 || a.blank >= a.V || a.cells < 0) {
        fprintf(stderr, "parakeet_amd: internal error: tdt_tree_lattice_bf16 outside the kernel's limits (J %d, D %d, V %d, blank %d)\n", a.J, a.tr.D, a.V, a.blank);
        abort();
    }
    if (a.cells == 0) return;
    if (rows == 128) tt_launch<4>(a, s);
    else if (rows == 96) tt_launch<3>(a, s);
    else tt_launch<2>(a, s);
}

}  // namespace pk
