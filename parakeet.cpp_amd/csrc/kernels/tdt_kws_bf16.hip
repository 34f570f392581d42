// parakeet.cpp_amd/csrc/kernels/tdt_kws_bf16.hip -- the TDT keyword spotting lattice of the TOLERANCE-class mode (pk_config.gemm_bf16 with
// pk_model_set_tdt_kws_bf16): ONE launch takes the joint of every lattice row of a group of (clip, keyword) pairs from
// enc_proj and the prediction net's rows to the NORMALISED arcs tdt_kws_kernel walks.  No activation row, no logits row, no top[] and no
// log-probability is ever formed: the walk reads every arc relative to the greedy decision of its cell, and in those differences the log-sum-exp
// of the row cancels, lab - top = logit[id] - max_n logit[n].
//
// For lattice row r = (pair p, t, u), clip rows from ep_row0[p], net slot k = net_of[p] (the numbering of lattice_act_row<true> / tdt_kws_keep_kernel):
//     z[j]     = bf16_rne(s > 0 ? s : 0),  s = fl32(ep[ep_row0[p] + t][j] + pp[u n_net + k][j])
//     logit[n] = fl32-accumulated sum_j z[j] W16[n][j] on v_mfma_f32_32x32x16_bf16, + bld[n] in fp32;  W16 = bf16_rne(wld)
//     M  = max_{n < V} logit[n] (the blank included),  Md = max_{i < D} logit[V + i]
//     blk[r] = fl(logit[blank] - M),  lab[..] = fl(logit[ids[u]] - M) (u < L),  dl[r][i] = fl(logit[V + i] - Md)
// M and Md are maxima over the very fp32 values that are subtracted (the captured ones are copies of the registers the maximum saw), so every stored
// value is <= 0 and the row's greedy arcs are exactly 0; + 0.0f after the subtraction turns the one -0.0 that could arise ((-0.0) - (+0.0)) into +0.0.
//
// Work split.  A workgroup of 4 waves owns R = 32 RS consecutive lattice rows.  Spotting lattices are many small pairs (T x (L + 1) rows, L mostly
// 2 .. 8), so a tile usually spans several pairs and both edges of a keyword: nothing in the tile is per pair, every row carries its own tables.
//   1. Threads 0 .. R-1 decode their row -- pair by bisection over cell_off, then t, u -- into LDS tables: the ep row, the pp row u n_net +
//      net_of[p], the label column ids[u] (-1 at u = L) and lab's index.
//   2. All threads build z in LDS in MFMA fragment order [RS][J / 16][64 lanes][8 bf16] (tdt_lattice_bf16.hip's layout).
//   3. The contraction is TRANSPOSED (weight columns x lattice rows): a lane's 16 accumulators are 16 weight columns of ONE lattice row, so a row's
//      maximum is in-lane.  Wave w takes the 64-column blocks w, w + 4, ... of the load-order bf16 copy tdt_lattice_bf16_pack_kernel writes (the
//      model's packed buffer is shared with the alignment kernel), streamed from L2 through a four-step register ring that runs across block edges.
//      No barrier between the z build and the end of the walk.
//   4. The epilogue of a block is MAX-ONLY: + bias, v_max_f32 into the lane's running maximum, and the captures.  No v_exp_f32, no running sum, no
//      rescaling when a later block raises the maximum -- a new maximum costs nothing, wherever it arrives.  The label capture (one compare per
//      accumulator) runs only in the blocks that hold a label of one of the tile's rows (a wave-uniform ballot; with a vocabulary of 8193 and a few
//      keywords per tile that is a handful of 129 blocks); the blank's block and the blocks past V (durations, masked to -inf for the maximum;
//      the zero padding likewise) are wave-uniform branches as well.
//   5. One barrier; thread i < R takes the maximum of row i's 8 partial maxima (4 waves x 2 accumulator halves, [8][R] floats: half the partials
//      of the alignment kernel), the maximum of the D captured duration logits, and stores the 2 + D differences (1 + D where u = L).
// LDS beside z is 92 bytes per row (8 partial maxima, 10 captures, 3 ints, lab's index) where the alignment kernel needs 124,
// so under the same 150 KB cap a workgroup takes 128 rows up to J = 544 (the alignment kernel: 512), 96 up to J = 736 (tdt-600m's 640) and 64 up
// to J = 1152 (1120) (tdt_kws_bf16_rows).  The cost of a workgroup is the weight stream, so rows per workgroup are arithmetic per weight byte.
// LDS would admit 160 rows up to J = 416 and 192 up to J = 352, but those forms do not fit the register file: the compiler spills 1 and 9 VGPRs
// to scratch (10 and 12 accumulators of 16 beside the ring), so they are not built.
//
// Bounds: row tables are written for all R rows (past the last row: pp row -1, which zero-fills z and stores nothing); z index < RS (J / 16) 64;
// captures [10][R], D <= 8; the weight stream of wave w ends inside block NCB - 1 of the packed copy (the ring re-reads its last step); bld is read
// at c < V + D only.
//
// Limits (launcher): J % 32 == 0 and J <= 1152, 1 <= D <= 8, 0 <= blank < V; 1 <= L <= 64 is the walk's and checked by the host.
//
// Code objects (hipcc -O3 --offload-arch=gfx950, from the .s of -save-temps):
//   tdt_kws_bf16_kernel<4>   512 VGPR 100 SGPR  LDS 0 B + 128 (2 J + 92) dynamic  scratch 0 B; 0 VGPR spills, 0 SGPR spills
//   tdt_kws_bf16_kernel<3>   332 VGPR 100 SGPR  LDS 0 B +  96 (2 J + 92) dynamic  scratch 0 B; 0 VGPR spills, 0 SGPR spills
//   tdt_kws_bf16_kernel<2>   320 VGPR  98 SGPR  LDS 0 B +  64 (2 J + 92) dynamic  scratch 0 B; 0 VGPR spills, 0 SGPR spills
//   (VGPR counts include the 2 RS accumulators of 16 and the four-step ring; no v_exp_f32 in any of the three.  One workgroup per CU at every J:
//    above 256 VGPRs a SIMD holds one wave, whatever LDS would admit.)
#include "kernels.hpp"
#include "tdt_lattice_dev.hpp"

namespace pk {

typedef float tk_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 tk_bf16x8 __attribute__((ext_vector_type(8)));

static constexpr int TK_ROW_BYTES = 92;             // LDS beside z per lattice row: 8 partial maxima, 10 captures, 3 ints and lab's index
static constexpr size_t TK_LDS_MAX = 150 * 1024;    // (the cap of tdt_lattice_bf16.hip and the bf16 attention kernels)

__device__ __forceinline__ int tk_rowidx(int r, int g) { return (r & 3) + 8 * (r >> 2) + 4 * g; }     // row of accumulator register r (32x32 C layout)

template <int RS>
__global__ __launch_bounds__(256) void tdt_kws_bf16_kernel(TdtKwsBf16Args a) {
    constexpr int R = 32 * RS;
    extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
    const TdtLattice &lt = a.lt;
    const int J = a.J, KS = J >> 4, V = a.V, D = lt.D, VD = V + D, blank = a.blank;
    tk_bf16x8 *zL = reinterpret_cast<tk_bf16x8 *>(tk_smem);                         // [RS][KS][64]
    int64_t *labi = reinterpret_cast<int64_t *>(tk_smem + (size_t)R * J * 2);       // [R] index into lab, -1 at u = L and past the last row
    float *part = reinterpret_cast<float *>(labi + R);                              // [4 waves][2 halves][R] partial maxima
    float *cap = part + 8 * R;                                                      // [blank, ids[u], D durations (8)][R]
    int *epr = reinterpret_cast<int *>(cap + 10 * R), *ppr = epr + R, *idc = ppr + R;   // [R] each: ep row, pp row (-1 past the last row), column ids[u] (-1 none)
    const float NEG = -__builtin_huge_valf();

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 31, g = lane >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * R;

    if (tid < R) {                                                  // 1. the rows of this tile
        const int64_t r = row0 + tid;
        int e = -1, p = -1, ic = -1;
        int64_t li = -1;
        if (r < a.cells) {
            const int b = lattice_row_owner(lt.cell_off, lt.B, r);
            const int i0 = lt.id_off[b], L = lt.id_off[b + 1] - i0, L1 = L + 1;
            const int64_t c = r - lt.cell_off[b];
            const int t = (int)(c / L1), u = (int)(c - (int64_t)t * L1);
            e = a.ep_row0[b] + t;
            p = u * a.n_net + a.net_of[b];
            if (u < L) { ic = a.ids[i0 + u]; li = lt.lab_off[b] + (int64_t)t * L + u; }
        }
        epr[tid] = e; ppr[tid] = p; idc[tid] = ic; labi[tid] = li;
    }
    __syncthreads();
    {                                                               // 2. z, fragment order; chunk q: row q % 32 of subtile st, k chunk ch of 8
        const int NCH = J >> 3;
        for (int q = tid; q < R * NCH; q += 256) {
            const int rn = q & 31, rest = q >> 5, ch = rest % NCH, st = rest / NCH, row = 32 * st + rn;
            tk_bf16x8 v;
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
    const tk_bf16x8 *W = static_cast<const tk_bf16x8 *>(a.w16);
    const int NCB = (VD + 63) >> 6;
    const int nblk = wave < NCB ? (NCB - wave + 3) >> 2 : 0;
    float m_run[RS];
    int my_idc[RS];
#pragma unroll
    for (int st = 0; st < RS; ++st) { m_run[st] = NEG; my_idc[st] = idc[32 * st + n]; }

    if (nblk > 0) {
        // the wave's weight stream: step (block, ks) is 128 vectors, a block KS steps, the wave's next block 4 blocks on.  Past the last step the
        // ring re-reads the last one.
        const int total = nblk * KS;
        const tk_bf16x8 *pf = W + (int64_t)wave * KS * 128 + lane;
        int pf_i = 0, pf_ks = 0;
        auto fetch = [&](tk_bf16x8 (&dst)[2]) {
            dst[0] = pf[0];
            dst[1] = pf[64];
            if (pf_i + 1 < total) {
                ++pf_i;
                if (++pf_ks == KS) { pf_ks = 0; pf += (int64_t)3 * KS * 128 + 128; }
                else pf += 128;
            }
        };
        tk_bf16x8 a0[2], a1[2], a2[2], a3[2];
        fetch(a0); fetch(a1); fetch(a2); fetch(a3);
        for (int bi = 0; bi < nblk; ++bi) {
            tk_f32x16 acc[2][RS];
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int st = 0; st < RS; ++st)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[h][st][r] = 0.0f;
            for (int ks = 0; ks < KS; ++ks) {
                const tk_bf16x8 *zp = zL + ks * 64 + lane;
#pragma unroll
                for (int st = 0; st < RS; ++st) {
                    const tk_bf16x8 zb = zp[st * KS * 64];
                    acc[0][st] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[0], zb, acc[0][st], 0, 0, 0);
                    acc[1][st] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[1], zb, acc[1][st], 0, 0, 0);
                }
                a0[0] = a1[0]; a0[1] = a1[1]; a1[0] = a2[0]; a1[1] = a2[1]; a2[0] = a3[0]; a2[1] = a3[1];
                fetch(a3);
            }
            // the block's 64 columns c0 + 32 h + tk_rowidx(r, g) of the lane's RS rows
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
                        const int c = c0 + 32 * h + tk_rowidx(r, g);
                        bv[h][r] = a.bld[c < VD ? c : VD - 1];      // (a padding column is masked below)
                    }
            }
#pragma unroll
            for (int st = 0; st < RS; ++st) {
                const int row = 32 * st + n;
                const bool lab_here = my_idc[st] >= c0 && my_idc[st] < c0 + 64;
                const bool any_lab = __ballot(lab_here) != 0;      // (wave-uniform) some row of this subtile has its label in the block
                float bm = m_run[st];
                if (pure && !any_lab && !has_blank) {               // the common block: bias and maximum alone
#pragma unroll
                    for (int h = 0; h < 2; ++h)
#pragma unroll
                        for (int r = 0; r < 16; ++r) bm = fmaxf(bm, acc[h][st][r] + bv[h][r]);
                } else {
#pragma unroll
                    for (int h = 0; h < 2; ++h)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int c = c0 + 32 * h + tk_rowidx(r, g);
                            float v = acc[h][st][r] + bv[h][r];
                            if (!pure) {
                                if (c >= V && c < VD) cap[(2 + c - V) * R + row] = v;
                                if (c >= V) v = NEG;
                            }
                            if (c == my_idc[st]) cap[R + row] = v;
                            if (has_blank && c == blank) cap[row] = v;
                            bm = fmaxf(bm, v);
                        }
                }
                m_run[st] = bm;
            }
        }
    }
#pragma unroll
    for (int st = 0; st < RS; ++st) part[(wave * 2 + g) * R + 32 * st + n] = m_run[st];
    __syncthreads();

    if (tid < R && ppr[tid] >= 0) {                                 // 5. row tid of the tile
        const int64_t r = row0 + tid;
        float M = part[tid];
#pragma unroll
        for (int p = 1; p < 8; ++p) M = fmaxf(M, part[p * R + tid]);
        lt.blk[r] = (cap[tid] - M) + 0.0f;
        if (labi[tid] >= 0) lt.lab[labi[tid]] = (cap[R + tid] - M) + 0.0f;
        float dm = cap[2 * R + tid];
        for (int i = 1; i < D; ++i) dm = fmaxf(dm, cap[(2 + i) * R + tid]);
        for (int i = 0; i < D; ++i) lt.dl[r * D + i] = (cap[(2 + i) * R + tid] - dm) + 0.0f;
    }
}

static size_t tk_lds_bytes(int J, int rs) { return (size_t)32 * rs * ((size_t)J * 2 + TK_ROW_BYTES); }

static int tk_rs(int J) {
    if (J <= 0 || J % 32) return 0;
    for (int rs : {4, 3, 2})
        if (tk_lds_bytes(J, rs) <= TK_LDS_MAX) return rs;
    return 0;
}

int tdt_kws_bf16_rows(int J) { return 32 * tk_rs(J); }

template <int RS>
static void tk_launch(const TdtKwsBf16Args &a, hipStream_t s) {
    auto kern = &tdt_kws_bf16_kernel<RS>;
    static DynLdsSlots slots;
    const size_t lds = tk_lds_bytes(a.J, RS);
    ensure_dyn_lds(slots, reinterpret_cast<const void *>(kern), lds);
    hipLaunchKernelGGL(kern, dim3((unsigned)((a.cells + 32 * RS - 1) / (32 * RS))), dim3(256), lds, s, a);
}

void launch_tdt_kws_bf16(const TdtKwsBf16Args &a, hipStream_t s) {
    const int rs = tk_rs(a.J);
    if (rs == 0 || a.lt.D < 1 || a.lt.D > 8 || a.blank < 0 || a.blank >= a.V || a.cells < 0 || a.n_net < 1) {
        fprintf(stderr, "parakeet_amd: internal error: tdt_kws_bf16 outside the kernel's limits (J %d, D %d, V %d, blank %d, n_net %d)\n", a.J, a.lt.D, a.V,
                a.blank, a.n_net);
        abort();
    }
    if (a.cells == 0) return;
    if (rs == 4) tk_launch<4>(a, s);
    else if (rs == 3) tk_launch<3>(a, s);
    else tk_launch<2>(a, s);
}

}  // namespace pk
