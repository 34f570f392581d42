// parakeet.cpp_amd/csrc/kernels/gemm_mxfp8.hip -- MXFP8 (OCP MX: e4m3 elements, one E8M0 scale per 32 k) products on the block-scaled matrix
// instruction of gfx950, v_mfma_scale_f32_32x32x64_f8f6f4, and the quantiser that makes their operands.  DESIGN.md section 5.2.1.
//
// out[M][N] = epi(sum over 32-k blocks of 2^(ea + ew) sum_k qa[m][k] qw[n][k] + bias), fp32 accumulation.  The bf16 K loop of this project runs
// at what a CU pulls from L2 into LDS; this one moves half the bytes per flop through the same pipe:
//  * Both operands live in HBM in the order the loads want (kernels.hpp: 1 KB blocks of 8 rows x 128 k, the 16-byte chunks of a row already
//    XOR-swizzled), so one global_load_lds_dwordx4 of a wave copies ONE CONTIGUOUS KB into LDS as it lies -- no staging registers, no ds_write
//    (the LDS store width lesson of round 2 does not arise: nothing is stored from registers), and the image is the one whose ds_read_b128
//    fragment reads gemm_bf16_glds.hpp found conflict-free.  A K tile is 128 k = two MFMA steps; two LDS buffers, the DMA of K tile kt + 2 issued
//    behind the barrier that frees tile kt's buffer (that kernel's schedule: a whole K tile of MFMAs for it to land).
//  * A lane's fragment of one step is two ds_read_b128 of its row: 16 k of each of the step's two MX blocks (lane half h: k 16 h .. + 15 and
//    32 + 16 h .. + 15), and it supplies ONE scale byte: lanes 0-31 the first block's of their row, lanes 32-63 the second's.  The
//    scale bytes never touch LDS: they are stored so that a lane's aligned dword holds its scales of four consecutive steps (two K tiles), are
//    requested two K tiles ahead straight into a VGPR, and a shift puts the step's byte where the instruction reads it (opsel 0).
//  * The MFMA operands are SWAPPED (acc = mfma(W fragment, A fragment)): lane (lr = lane & 31, h = lane >> 5) then owns output ROW lr of its
//    32-row tile and, per register quad q, the four consecutive columns 8 q + 4 h .. + 3 -- every epilogue runs from registers:
//      MX_EPI_F32    float4 stores;
//      MX_EPI_RESID  out = resid + alpha (acc + bias), float4 in, float4 out (in place: a lane reads and writes its own elements);
//      MX_EPI_MX     the tile quantises its own output into the NEXT product's A operand.  The 32 columns of a (row, column tile) sit in the two
//                    lanes lr and lr + 32: the block amax is one v_permlane32_swap, two more hand each lane one whole 16-byte chunk of the row,
//                    which it stores at the chunk's swizzled place; lane h = 0 adds the scale byte.  A separate quantise pass over [M][f] would
//                    cost about what the product saves.
//  * 256 x 256 tiles on 8 waves of 64 x 128 (fc1 of tdt-600m at 32 x 30 s: 2.94 rounds of the 256 CUs), 192 x 256 on 8 waves of 96 x 64 for the
//    residual product (fc2: 252 tiles, one round).  Grouped tile order and the XCD remap are gemm_bf16_glds.hpp's.
// NaN / Inf inputs of the quantiser are out of scope: a block that holds one has no defined result.
#include "../pk_devmath.h"
#include "kernels.hpp"
#include <cstdio>
#include <cstdlib>

namespace pk {

typedef int mx_i32x8 __attribute__((ext_vector_type(8)));
typedef int mx_i32x4 __attribute__((ext_vector_type(4)));
typedef float mx_f32x16 __attribute__((ext_vector_type(16)));

// scale byte and 2^-e of a block whose largest magnitude is amax (>= 0, finite): e = clamp(floor(log2 amax) - 8, -127, 127), byte = e + 127.
// floor(log2) is the exponent field; a zero or subnormal amax clamps to -127 like every amax below 2^-118.
__device__ __forceinline__ unsigned mx_scale_byte(float amax) {
    const unsigned ef = __builtin_bit_cast(unsigned, amax) >> 23;
    return ef > 8u ? ef - 8u : 0u;
}
__device__ __forceinline__ float mx_inv_scale(unsigned sb) { return __builtin_bit_cast(float, (254u - sb) << 23); }   // 2^(127 - sb): a normal float for every byte
// four values, scaled (exact: a power of two), clamped to the e4m3 range, rounded to nearest even by v_cvt_pk_fp8_f32 -> four bytes, k ascending
__device__ __forceinline__ unsigned mx_pack4(float a, float b, float c, float d, float inv) {
    auto cl = [&](float v) { return fminf(fmaxf(v * inv, -448.0f), 448.0f); };
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(cl(a), cl(b), 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(cl(c), cl(d), w, true);
    return (unsigned)w;
}

// ---- the quantiser: one thread per (row, block of 32 k) -------------------------------------------------------------------------------------
template <bool SRC16>
__global__ __launch_bounds__(256) void mx_quantize_kernel(const void *src, int64_t rows, int K, int64_t ld, uint8_t *q, uint8_t *sc) {
    const int kbs = K >> 5;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= rows * kbs) return;
    const int64_t r = t / kbs;
    const int kb = (int)(t - r * kbs);
    float v[32];
    if constexpr (SRC16) {
        const uint4 *p = reinterpret_cast<const uint4 *>(reinterpret_cast<const uint16_t *>(src) + r * ld + kb * 32);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint4 u = p[i];
            const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[8 * i + 2 * e] = __builtin_bit_cast(float, w[e] << 16);
                v[8 * i + 2 * e + 1] = __builtin_bit_cast(float, w[e] & 0xFFFF0000u);
            }
        }
    } else {
        const float4 *p = reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(src) + r * ld + kb * 32);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float4 u = p[i];
            v[4 * i] = u.x; v[4 * i + 1] = u.y; v[4 * i + 2] = u.z; v[4 * i + 3] = u.w;
        }
    }
    float amax = 0.0f;
#pragma unroll
    for (int i = 0; i < 32; ++i) amax = fmaxf(amax, fabsf(v[i]));
    const unsigned sb = mx_scale_byte(amax);
    const float inv = mx_inv_scale(sb);
    unsigned w[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = mx_pack4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3], inv);
    *reinterpret_cast<uint4 *>(q + mx_elem_at(r, kb * 32, K)) = make_uint4(w[0], w[1], w[2], w[3]);
    *reinterpret_cast<uint4 *>(q + mx_elem_at(r, kb * 32 + 16, K)) = make_uint4(w[4], w[5], w[6], w[7]);
    sc[mx_scale_at(r, kb, rows)] = (uint8_t)sb;
}

void launch_mx_quantize(const void *src, int src_bf16, int64_t rows, int K, int64_t ld, uint8_t *q, uint8_t *sc, hipStream_t s) {
    if (rows <= 0 || K <= 0 || K % 32 != 0 || ld < K || ld % (src_bf16 ? 8 : 4) != 0 || rows * (int64_t)(K >> 5) > ((int64_t)1 << 38)) {
        fprintf(stderr, "launch_mx_quantize: rows > 0, K %% 32 == 0, ld >= K and a multiple of 16 bytes (rows %lld, K %d, ld %lld)\n", (long long)rows, K, (long long)ld);
        abort();
    }
    const unsigned grid = (unsigned)((rows * (K >> 5) + 255) / 256);
    if (src_bf16) hipLaunchKernelGGL(mx_quantize_kernel<true>, dim3(grid), dim3(256), 0, s, src, rows, K, ld, q, sc);
    else hipLaunchKernelGGL(mx_quantize_kernel<false>, dim3(grid), dim3(256), 0, s, src, rows, K, ld, q, sc);
}

// ---- the product ------------------------------------------------------------------------------------------------------------------------------
template <int WGM, int WGN, int TM, int TN, int EPI, bool SILU>
__device__ __forceinline__ void mx_epilogue(const MxGemmArgs &g, mx_f32x16 (&acc)[TM][TN], int m0, int n0) {
    constexpr int WM = TM * 32, WN = TN * 32;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave / WGN, wn = wave % WGN, lr = lane & 31, h = lane >> 5;
    const int cw = __builtin_amdgcn_readfirstlane(n0 + wn * WN);    // first output column of this wave
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int cb = cw + j * 32;                                 // wave-uniform; N % 32 == 0 (launcher): the column tile is inside N or outside
        if (cb >= g.N) continue;
        float4 bs[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) bs[q] = g.bias ? *reinterpret_cast<const float4 *>(g.bias + cb + 8 * q + 4 * h) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int row = m0 + wm * WM + i * 32 + lr;
            const bool rok = row < g.M;
            float v[4][4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                v[q][0] = acc[i][j][4 * q] + bs[q].x; v[q][1] = acc[i][j][4 * q + 1] + bs[q].y;
                v[q][2] = acc[i][j][4 * q + 2] + bs[q].z; v[q][3] = acc[i][j][4 * q + 3] + bs[q].w;
                if constexpr (SILU) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[q][e] = fast_siluf(v[q][e]);
                }
            }
            if constexpr (EPI == MX_EPI_F32) {
                if (rok) {
                    float *o = g.out + (int64_t)row * g.ldo + cb + 4 * h;
#pragma unroll
                    for (int q = 0; q < 4; ++q) *reinterpret_cast<float4 *>(o + 8 * q) = make_float4(v[q][0], v[q][1], v[q][2], v[q][3]);
                }
            } else if constexpr (EPI == MX_EPI_RESID) {             // resid + y, y = v * alpha rounded on its own (gemm_epi.hpp)
                if (rok) {
                    const float *rp = g.resid + (int64_t)row * g.ldr + cb + 4 * h;
                    float *o = g.out + (int64_t)row * g.ldo + cb + 4 * h;
                    float4 r[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) r[q] = *reinterpret_cast<const float4 *>(rp + 8 * q);
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        *reinterpret_cast<float4 *>(o + 8 * q) =
                            make_float4(r[q].x + v[q][0] * g.alpha, r[q].y + v[q][1] * g.alpha, r[q].z + v[q][2] * g.alpha, r[q].w + v[q][3] * g.alpha);
                }
            } else {
                // this lane's 16 of the block's 32 values; the other 16 are in lane ^ 32: whichever half a swap hands over, the larger of the two is the block's
                float am = 0.0f;
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int e = 0; e < 4; ++e) am = fmaxf(am, fabsf(v[q][e]));
                const unsigned ab = __builtin_bit_cast(unsigned, am);
                const auto mm = __builtin_amdgcn_permlane32_swap(ab, ab, false, false);
                const unsigned sb = mx_scale_byte(__builtin_bit_cast(float, mm[0] > mm[1] ? mm[0] : mm[1]));   // (non-negative floats order as integers)
                const float inv = mx_inv_scale(sb);
                unsigned d[4];                                      // d[q] = columns 8 q + 4 h .. + 3
#pragma unroll
                for (int q = 0; q < 4; ++q) d[q] = mx_pack4(v[q][0], v[q][1], v[q][2], v[q][3], inv);
                // lanes 0-31 give up columns 16 .. 31 of their half (d[2], d[3]) for the other half's columns 0 .. 15 (its d[0], d[1]): lane h then holds the
                // 16 consecutive columns 16 h .. 16 h + 15 = one chunk
                const auto s0 = __builtin_amdgcn_permlane32_swap(d[0], d[2], false, false);
                const auto s1 = __builtin_amdgcn_permlane32_swap(d[1], d[3], false, false);
                if (rok) {
                    *reinterpret_cast<uint4 *>(g.outq + mx_elem_at(row, cb + 16 * h, g.N)) = make_uint4(s0[0], s0[1], s1[0], s1[1]);
                    if (h == 0) g.outs[mx_scale_at(row, cb >> 5, g.M)] = (uint8_t)sb;
                }
            }
        }
    }
}

template <int WGM, int WGN, int TM, int TN, int EPI, bool SILU>
__global__ __launch_bounds__(64 * WGM * WGN) void gemm_mxfp8_kernel(MxGemmArgs g, int tiles_n, int n_tiles) {
    constexpr int BK = 128;                                         // bytes = k per tile row of a K tile: two MFMA steps of 64
    constexpr int NW = WGM * WGN, WM = TM * 32, WN = TN * 32, BM = WGM * WM, BN = WGN * WN;
    constexpr int BUF = (BM + BN) * BK;                             // bytes per staging buffer
    constexpr int NBLK = (BM + BN) / 8, NBPW = NBLK / NW;           // 1 KB blocks of 8 rows per K tile / per wave
    static_assert(NBLK % NW == 0, "blocks must split evenly over the waves");
    extern __shared__ __attribute__((aligned(16))) unsigned char mx_smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wv / WGN, wn = wv % WGN, lr = lane & 31, h = lane >> 5;
    const int nkt = (g.K + 127) >> 7, nsteps = g.K >> 6, ngrp = (g.K + 255) >> 8;
    const int64_t arows = mx_rows(g.M), wrows = mx_rows(g.N);

    // the XCD-aware remap and the grouped tile order of gemm_bf16_glds.hpp (one tile per workgroup: the grid is n_tiles)
    int m0, n0;
    {
        const int xq = n_tiles >> 3, xr = n_tiles & 7, xcd = (int)blockIdx.x & 7, idx = (int)blockIdx.x >> 3;
        const int bid = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + idx;
        constexpr int GROUPM = 4;
        const int tiles_m = n_tiles / tiles_n, per_group = GROUPM * tiles_n;
        const int grp = bid / per_group, first_m = grp * GROUPM;
        const int gsz = (tiles_m - first_m) < GROUPM ? (tiles_m - first_m) : GROUPM;
        const int in = bid - grp * per_group;
        m0 = (first_m + in % gsz) * BM;
        n0 = (in / gsz) * BN;
    }

    // DMA sources: wave w copies blocks w, w + NW, ... of the stacked tile (rows 0 .. BM-1 = A rows, BM .. = W rows); lane q brings the q-th 16 bytes
    // of the block.  Block rows past the operand's end re-read its last block (never stored: rows >= M, columns >= N).
    const uint8_t *src[NBPW];
#pragma unroll
    for (int i = 0; i < NBPW; ++i) {
        const int b = wv + NW * i;
        const bool is_a = 8 * b < BM;
        int64_t rb = is_a ? (m0 >> 3) + b : (n0 >> 3) + (b - BM / 8);
        const int64_t lim = (is_a ? arows : wrows) >> 3;
        rb = rb < lim ? rb : lim - 1;
        src[i] = (is_a ? g.Aq : g.Wq) + rb * nkt * 1024 + lane * 16;
    }
    auto dma = [&](int kt, int buf) {
#pragma unroll
        for (int i = 0; i < NBPW; ++i) {
            unsigned char *dst = mx_smem + buf * BUF + (wv + NW * i) * 1024;       // wave-uniform
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src[i] + (int64_t)kt * 1024),
                                             (__attribute__((address_space(3))) void *)dst, 16, 0, 0);
        }
    };
    // scale dwords: this lane's row of every operand tile, k half h; group = 256 k = four steps
    const uint8_t *sa[TM], *sw[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        int64_t r = m0 + wm * WM + i * 32 + lr;
        r = r < arows ? r : arows - 1;
        sa[i] = g.As + r * 8 + 4 * h;
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        int64_t r = n0 + wn * WN + j * 32 + lr;
        r = r < wrows ? r : wrows - 1;
        sw[j] = g.Ws + r * 8 + 4 * h;
    }
    unsigned sca[TM], scw[TN], sca_n[TM], scw_n[TN];
    auto load_scales = [&](int grp, unsigned (&a)[TM], unsigned (&w)[TN]) {
#pragma unroll
        for (int i = 0; i < TM; ++i) a[i] = *reinterpret_cast<const unsigned *>(sa[i] + (int64_t)grp * arows * 8);
#pragma unroll
        for (int j = 0; j < TN; ++j) w[j] = *reinterpret_cast<const unsigned *>(sw[j] + (int64_t)grp * wrows * 8);
    };

    mx_f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    // fragment addresses: tile row (a multiple of 32) + lr, logical chunks 4 s + 2 h and + 1 at physical chunk ^ fx, fx = (row >> 1) & 7
    const int fx = (lr >> 1) & 7;
    const int fa_base = (wm * WM + lr) * BK, fb_base = (BM + wn * WN + lr) * BK;
    // (the instruction is two 32 x 32 x 32 halves: registers 0-3 of lane half h are k 16 h .. + 15 of the step's FIRST block, registers 4-7 the same of
    //  its second block; the scale of the first block comes from lanes 0-31, of the second from lanes 32-63 -- measured, tests/test_gpu_mxfp8_gemm.py)
    auto frag = [&](int off, int s) {
        const int c = 4 * s + h;
        const mx_i32x4 lo = *reinterpret_cast<const mx_i32x4 *>(mx_smem + off + ((c ^ fx) << 4));
        const mx_i32x4 hi = *reinterpret_cast<const mx_i32x4 *>(mx_smem + off + (((c + 2) ^ fx) << 4));
        return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    };
#define MX_WAIT_VM0() __builtin_amdgcn_s_waitcnt(0x0F70)           /* vmcnt(0): this wave's LDS-DMA and scale loads have landed */

    dma(0, 0);
    if (nkt > 1) dma(1, 1);
    load_scales(0, sca, scw);
#pragma unroll
    for (int i = 0; i < TM; ++i) sca_n[i] = 0;
#pragma unroll
    for (int j = 0; j < TN; ++j) scw_n[j] = 0;
    MX_WAIT_VM0();
    __syncthreads();
    int cur = 0;
    for (int kt = 0; kt < nkt; ++kt) {
        if ((kt & 1) == 0 && (kt >> 1) + 1 < ngrp) load_scales((kt >> 1) + 1, sca_n, scw_n);    // two K tiles ahead: long landed when it is used
        const int nsub = nsteps - 2 * kt < 2 ? nsteps - 2 * kt : 2;                              // (K % 128 == 64: the last K tile holds one step)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (s < nsub) {
                const int sh = 8 * (2 * (kt & 1) + s);
                mx_i32x8 fa[TM], fb[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) fa[i] = frag(cur * BUF + fa_base + i * 32 * BK, s);
#pragma unroll
                for (int j = 0; j < TN; ++j) fb[j] = frag(cur * BUF + fb_base + j * 32 * BK, s);
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)   // C^T: lane = output row.  e4m3 x e4m3 (cbsz = blgp = 0), each lane's scale in byte 0
                        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fb[j], fa[i], acc[i][j], 0, 0, 0, (int)(scw[j] >> sh), 0, (int)(sca[i] >> sh));
            }
        }
        MX_WAIT_VM0();                 // K tile kt + 1 (issued a whole tile ago) is in LDS, the next scale dwords in their registers
        __syncthreads();               // ... for every wave; and every wave is done reading buffer `cur`
        if (kt + 2 < nkt) dma(kt + 2, cur);
        if (kt & 1) {
#pragma unroll
            for (int i = 0; i < TM; ++i) sca[i] = sca_n[i];
#pragma unroll
            for (int j = 0; j < TN; ++j) scw[j] = scw_n[j];
        }
        cur ^= 1;
    }
#undef MX_WAIT_VM0
    mx_epilogue<WGM, WGN, TM, TN, EPI, SILU>(g, acc, m0, n0);
}

MxTile gemm_mxfp8_tile(int epi) { return epi == MX_EPI_RESID ? MxTile{192, 256} : MxTile{256, 256}; }

template <int WGM, int WGN, int TM, int TN, int EPI, bool SILU>
static void launch_mx_kernel(const MxGemmArgs &a, hipStream_t s) {
    constexpr int BM = WGM * TM * 32, BN = WGN * TN * 32;
    constexpr size_t lds = 2 * (size_t)(BM + BN) * 128;
    const int tiles_m = (a.M + BM - 1) / BM, tiles_n = (a.N + BN - 1) / BN;
    auto kern = &gemm_mxfp8_kernel<WGM, WGN, TM, TN, EPI, SILU>;
    static DynLdsSlots slots;
    ensure_dyn_lds(slots, reinterpret_cast<const void *>(kern), lds);
    hipLaunchKernelGGL(kern, dim3(tiles_m * tiles_n), dim3(64 * WGM * WGN), lds, s, a, tiles_n, tiles_m * tiles_n);
}

void launch_gemm_mxfp8(const MxGemmArgs &a, int epi, hipStream_t s) {
    const char *why = nullptr;
    if (a.M <= 0 || a.N <= 0 || a.K <= 0 || a.K % 64 != 0 || a.N % 32 != 0) why = "M, N, K > 0, K % 64 == 0, N % 32 == 0";
    else if (!a.Aq || !a.As || !a.Wq || !a.Ws) why = "both operands as MX bytes + scale bytes";
    else if (epi == MX_EPI_MX ? !(a.outq && a.outs) : !(a.out && a.ldo >= a.N && a.ldo % 4 == 0)) why = "an output (fp32 rows: ldo >= N, a multiple of 4)";
    else if (epi == MX_EPI_RESID && (a.silu || !a.resid || a.ldr < a.N || a.ldr % 4 != 0)) why = "the residual epilogue: resid, ldr >= N and a multiple of 4, no SiLU";
    else if (epi == MX_EPI_F32 && a.silu) why = "SiLU comes with the MX output";
    else if (epi < MX_EPI_F32 || epi > MX_EPI_RESID) why = "epi";
    else if (((int64_t)(a.M + 255) / 256) * ((a.N + 255) / 256) * 2 > ((int64_t)1 << 30)) why = "too many tiles";
    if (why) {
        fprintf(stderr, "launch_gemm_mxfp8: %s (M %d, N %d, K %d, epi %d)\n", why, a.M, a.N, a.K, epi);
        abort();
    }
    if (epi == MX_EPI_RESID) launch_mx_kernel<2, 4, 3, 2, MX_EPI_RESID, false>(a, s);
    else if (epi == MX_EPI_F32) launch_mx_kernel<4, 2, 2, 4, MX_EPI_F32, false>(a, s);
    else if (a.silu) launch_mx_kernel<4, 2, 2, 4, MX_EPI_MX, true>(a, s);
    else launch_mx_kernel<4, 2, 2, 4, MX_EPI_MX, false>(a, s);
}

}  // namespace pk
