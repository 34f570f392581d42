// parakeet.cpp_amd/csrc/kernels/tdt_lattice_bf16.hip -- the TDT lattice of the TOLERANCE-class mode (pk_config.gemm_bf16 with
// pk_model_set_tdt_lattice_bf16): ONE launch takes the joint of every lattice row of a ragged batch from enc_proj and the
// prediction net's rows to the 2 + D log-probs the walks read.  No activation row and no logits row ever reaches memory.
//
// For lattice row r = (b, t, u) (the numbering of lattice_act_row<false> / tdt_lattice_keep_kernel):
//     z[j]     = bf16_rne(s > 0 ? s : 0),  s = fl32(ep[ep_row0[b] + t][j] + pp[u B + b][j])
//     logit[n] = fl32-accumulated sum_j z[j] W16[n][j] on v_mfma_f32_32x32x16_bf16, + bld[n] in fp32;  W16 = bf16_rne(wld)
//     blk[r] = logit[blank] - lse_V,  lab[..] = logit[ids[u]] - lse_V (u < U),  dl[r][i] = logit[V + i] - lse_D
// with lse_V over the columns n < V and lse_D over V <= n < V + D.  The specification is tests/tdt_lattice_bf16_ref.py.
//
// Work split.  A workgroup of 4 waves owns R = 32 RS consecutive lattice rows (RS = 4, 3 or 2: as many as fit LDS beside the row tables, see
// tdt_lattice_bf16_rows; 128 rows up to J = 512, 96 at tdt-600m's J = 640, 64 up to J = 1120).  Its cost is the weight stream -- all
// (V + D) J bf16 values once per workgroup -- so the rows per workgroup set the arithmetic per weight byte, and LDS, which holds the z operand, is
// what caps them.
//   1. Threads 0 .. R-1 decode their row (owner by bisection, t, u) into LDS tables: the ep row, the pp row, the column ids[u] and lab's index.
//   2. All threads build z in LDS in MFMA fragment order [RS][J / 16][64 lanes][8 bf16] -- lane (row n, k half g) of a B operand is 16
//      contiguous bytes, a wave's read of one fragment one contiguous KB.  Rows are t-major, so a tile shares a few ep rows in L2.
//   3. The contraction is TRANSPOSED (weight columns x lattice rows), so a lane's 16 accumulator registers are 16 weight columns of ONE lattice
//      row and the row statistics are in-lane.  Wave w takes the 64-column blocks w, w + 4, ...: per k-step of 16 two A fragments straight from
//      L2 (the copy is packed in load order [block][k-step][half][lane][8 bf16], see tdt_lattice_bf16_pack_kernel: 2 KB per step, contiguous
//      along the wave's stream) feed 2 RS MFMAs against the RS B fragments from LDS.  The waves read disjoint quarters of the weights, so the
//      workgroup streams them once and nothing of W is staged in LDS; four steps are in flight in a register ring that runs across block edges.
//      The waves never meet inside the walk: no barrier between the z build and the end.
//   4. After a block's K loop: + bias, capture of the columns blank / ids[u] / V .. V + D - 1 into LDS as they pass, and the lane's running
//      (max, sum) over the label columns it has seen.  The maximum may arrive in any block: the sum is rescaled by exp(m_old - m_new) before
//      the block's terms are added, and a lane that has seen no label column yet (m = -inf) subtracts 0 instead, so nothing forms inf - inf.
//      Blocks past V (duration columns, the zero padding to a multiple of 64) go through the same code with those columns masked to -inf.
//   5. One barrier; thread i < R merges the 8 partial (max, sum) pairs of row i (4 waves x 2 accumulator halves), takes the logs, the duration
//      log-softmax from the D captured logits, and stores 2 + D floats (1 + D where u = U).
// exp inside the walk is v_exp_f32 on (x - m) * log2(e); the merge and the duration head use dexpf / dlogf.
//
// Limits (launcher): J % 32 == 0 and J <= 1120, 1 <= D <= 8, 0 <= blank < V.
//
// Code objects (hipcc -O3 --offload-arch=gfx950, from the .s of -save-temps):
//   tdt_lattice_bf16_kernel<4>    508 VGPR 106 SGPR  LDS 0 B + 128 (2 J + 124) dynamic  scratch 0 B; 0 VGPR spills, 3 SGPRs spilled to VGPR lanes
//   tdt_lattice_bf16_kernel<3>    426 VGPR 106 SGPR  LDS 0 B +  96 (2 J + 124) dynamic  scratch 0 B; 0 VGPR spills, 5 SGPRs spilled to VGPR lanes
//   tdt_lattice_bf16_kernel<2>    328 VGPR 106 SGPR  LDS 0 B +  64 (2 J + 124) dynamic  scratch 0 B; 0 VGPR spills, 2 SGPRs spilled to VGPR lanes
//   tdt_lattice_bf16_pack_kernel   16 VGPR  28 SGPR  LDS 0 B                            scratch 0 B; 0 VGPR spills, 0 SGPR spills
//   (VGPR counts include the accumulation registers: 2 RS accumulators of 16, the block's 32 biased logits and exponentials per row subtile, the
//    four-step ring.  One workgroup per CU at every J: LDS admits no second one from J = 320 up (tdt-600m: 96 x 1404 = 134784 bytes), the registers
//    none below.  With one wave per SIMD the epilogue's VALU work is not hidden behind another wave's MFMAs.)
#include "../pk_devmath.h"
#include "kernels.hpp"
#include "tdt_lattice_dev.hpp"

namespace pk {

typedef float tl_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 tl_bf16x8 __attribute__((ext_vector_type(8)));

static constexpr int TL_ROW_BYTES = 124;            // LDS beside z per lattice row: 16 partials, 10 captures, 3 ints and lab's index
static constexpr size_t TL_LDS_MAX = 150 * 1024;    // (the cap the bf16 attention kernels keep as well)

__device__ __forceinline__ int tl_rowidx(int r, int g) { return (r & 3) + 8 * (r >> 2) + 4 * g; }     // row of accumulator register r (32x32 C layout)

// wld [VD][J] fp32 -> the load-order bf16 copy: vector ((cb KS + ks) 2 + h) 64 + lane holds W16[64 cb + 32 h + lane % 32][16 ks + 8 (lane / 32) + 0 .. 7],
// zero for the columns past VD of the last block
__global__ __launch_bounds__(256) void tdt_lattice_bf16_pack_kernel(const float *__restrict__ w, int VD, int J, tl_bf16x8 *__restrict__ out, int64_t n_vec) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_vec) return;
    const int KS = J >> 4, lane = (int)(i & 63), h = (int)(i >> 6) & 1;
    const int64_t q = i >> 7;
    const int ks = (int)(q % KS), cb = (int)(q / KS);
    const int col = 64 * cb + 32 * h + (lane & 31), k = 16 * ks + 8 * (lane >> 5);
    tl_bf16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (__bf16)(col < VD ? w[(int64_t)col * J + k + e] : 0.0f);
    out[i] = v;
}

template <int RS>
__global__ __launch_bounds__(256) void tdt_lattice_bf16_kernel(TdtLatticeBf16Args a) {
    constexpr int R = 32 * RS;
    constexpr float L2E = 1.44269502162933349609375f;
    extern __shared__ __attribute__((aligned(16))) unsigned char tl_smem[];
    const TdtLattice &lt = a.lt;
    const int J = a.J, KS = J >> 4, V = a.V, D = lt.D, VD = V + D, blank = a.blank;
    tl_bf16x8 *zL = reinterpret_cast<tl_bf16x8 *>(tl_smem);                         // [RS][KS][64]
    float *part = reinterpret_cast<float *>(tl_smem + (size_t)R * J * 2);           // [4 waves][2 halves][m, s][R]
    float *cap = part + 16 * R;                                                     // [blank, ids[u], D durations (8)][R]
    int64_t *labi = reinterpret_cast<int64_t *>(cap + 10 * R);                      // [R] index into lab, -1 at u = U and past the last row
    int *epr = reinterpret_cast<int *>(labi + R), *ppr = epr + R, *idc = ppr + R;   // [R] each: ep row, pp row (-1 past the last row), column ids[u] (-1 none)
    const float NEG = -__builtin_huge_valf();

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 31, g = lane >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * R;

    if (tid < R) {                                                  // 1. the rows of this tile
        const int64_t r = row0 + tid;
        int e = -1, p = -1, ic = -1;
        int64_t li = -1;
        if (r < a.cells) {
            const int b = lattice_row_owner(lt.cell_off, lt.B, r);
            const int i0 = lt.id_off[b], U = lt.id_off[b + 1] - i0, U1 = U + 1;
            const int64_t c = r - lt.cell_off[b];
            const int t = (int)(c / U1), u = (int)(c - (int64_t)t * U1);
            e = a.ep_row0[b] + t;
            p = u * lt.B + b;
            if (u < U) { ic = a.ids[i0 + u]; li = lt.lab_off[b] + (int64_t)t * U + u; }
        }
        epr[tid] = e; ppr[tid] = p; idc[tid] = ic; labi[tid] = li;
    }
    __syncthreads();
    {                                                               // 2. z, fragment order; chunk q: row q % 32 of subtile st, k chunk ch of 8
        const int NCH = J >> 3;
        for (int q = tid; q < R * NCH; q += 256) {
            const int rn = q & 31, rest = q >> 5, ch = rest % NCH, st = rest / NCH, row = 32 * st + rn;
            tl_bf16x8 v;
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
    const tl_bf16x8 *W = static_cast<const tl_bf16x8 *>(a.w16);
    const int NCB = (VD + 63) >> 6;
    const int nblk = wave < NCB ? (NCB - wave + 3) >> 2 : 0;
    float m_run[RS], s_run[RS];
    int my_idc[RS];
#pragma unroll
    for (int st = 0; st < RS; ++st) { m_run[st] = NEG; s_run[st] = 0.0f; my_idc[st] = idc[32 * st + n]; }

    if (nblk > 0) {
        // the wave's weight stream: step (block, ks) is 128 vectors, a block KS steps, the wave's next block 4 blocks on.  Past the last step the
        // ring re-reads the last one.
        const int total = nblk * KS;
        const tl_bf16x8 *pf = W + (int64_t)wave * KS * 128 + lane;
        int pf_i = 0, pf_ks = 0;
        auto fetch = [&](tl_bf16x8 (&dst)[2]) {
            dst[0] = pf[0];
            dst[1] = pf[64];
            if (pf_i + 1 < total) {
                ++pf_i;
                if (++pf_ks == KS) { pf_ks = 0; pf += (int64_t)3 * KS * 128 + 128; }
                else pf += 128;
            }
        };
        tl_bf16x8 a0[2], a1[2], a2[2], a3[2];
        fetch(a0); fetch(a1); fetch(a2); fetch(a3);
        for (int bi = 0; bi < nblk; ++bi) {
            tl_f32x16 acc[2][RS];
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int st = 0; st < RS; ++st)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[h][st][r] = 0.0f;
            for (int ks = 0; ks < KS; ++ks) {
                const tl_bf16x8 *zp = zL + ks * 64 + lane;
#pragma unroll
                for (int st = 0; st < RS; ++st) {
                    const tl_bf16x8 zb = zp[st * KS * 64];
                    acc[0][st] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[0], zb, acc[0][st], 0, 0, 0);
                    acc[1][st] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[1], zb, acc[1][st], 0, 0, 0);
                }
                a0[0] = a1[0]; a0[1] = a1[1]; a1[0] = a2[0]; a1[1] = a2[1]; a2[0] = a3[0]; a2[1] = a3[1];
                fetch(a3);
            }
            // the block's 64 columns c0 + 32 h + tl_rowidx(r, g) of the lane's RS rows
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
                        const int c = c0 + 32 * h + tl_rowidx(r, g);
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
                        const int c = c0 + 32 * h + tl_rowidx(r, g);
                        float v = acc[h][st][r] + bv[h][r];
                        if (!pure) {
                            if (c >= V && c < VD) cap[(2 + c - V) * R + row] = v;
                            if (c >= V) v = NEG;
                        }
                        if (c == my_idc[st]) cap[R + row] = v;
                        if (has_blank && c == blank) cap[row] = v;
                        x[h][r] = v;
                        bm = fmaxf(bm, v);
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
        lt.blk[r] = cap[tid] - lse;
        if (labi[tid] >= 0) lt.lab[labi[tid]] = cap[R + tid] - lse;
        float dm = NEG;
        for (int i = 0; i < D; ++i) dm = fmaxf(dm, cap[(2 + i) * R + tid]);
        float ds = 0.0f;
        for (int i = 0; i < D; ++i) ds += dexpf(cap[(2 + i) * R + tid] - dm);
        const float lse_d = dm + dlogf(ds);
        for (int i = 0; i < D; ++i) lt.dl[r * D + i] = cap[(2 + i) * R + tid] - lse_d;
    }
}

static size_t tl_lds_bytes(int J, int rs) { return (size_t)32 * rs * ((size_t)J * 2 + TL_ROW_BYTES); }

int tdt_lattice_bf16_rows(int J) {
    if (J <= 0 || J % 32) return 0;
    for (int rs = 4; rs >= 2; --rs)
        if (tl_lds_bytes(J, rs) <= TL_LDS_MAX) return 32 * rs;
    return 0;
}

size_t tdt_lattice_bf16_weight_bytes(int VD, int J) { return (size_t)((VD + 63) / 64) * 64 * J * 2; }

void launch_tdt_lattice_bf16_pack(const float *wld, int VD, int J, void *w16, hipStream_t s) {
    const int64_t n_vec = (int64_t)(tdt_lattice_bf16_weight_bytes(VD, J) / 16);
    hipLaunchKernelGGL(tdt_lattice_bf16_pack_kernel, dim3((unsigned)((n_vec + 255) / 256)), dim3(256), 0, s, wld, VD, J, static_cast<tl_bf16x8 *>(w16), n_vec);
}

template <int RS>
static void tl_launch(const TdtLatticeBf16Args &a, hipStream_t s) {
    auto kern = &tdt_lattice_bf16_kernel<RS>;
    static DynLdsSlots slots;
    const size_t lds = tl_lds_bytes(a.J, RS);
    ensure_dyn_lds(slots, reinterpret_cast<const void *>(kern), lds);
    hipLaunchKernelGGL(kern, dim3((unsigned)((a.cells + 32 * RS - 1) / (32 * RS))), dim3(256), lds, s, a);
}

void launch_tdt_lattice_bf16(const TdtLatticeBf16Args &a, hipStream_t s) {
    const int rows = tdt_lattice_bf16_rows(a.J);
    if (rows == 0 || a.lt.D < 1 || a.lt.D > 8 || a.blank < 0 || a.blank >= a.V || a.cells < 0) {
        fprintf(stderr, "parakeet_amd: internal error: tdt_lattice_bf16 outside the kernel's limits (J %d, D %d, V %d, blank %d)\n", a.J, a.lt.D, a.V, a.blank);
        abort();
    }
    if (a.cells == 0) return;
    if (rows == 128) tl_launch<4>(a, s);
    else if (rows == 96) tl_launch<3>(a, s);
    else tl_launch<2>(a, s);
}

}  // namespace pk
