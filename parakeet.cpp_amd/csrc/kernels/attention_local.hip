// parakeet.cpp_amd/csrc/kernels/attention_local.hip -- limited-context ("band") relative-position attention core:
//     S[i][j] = ( (q_i + u_h) . k_j  +  (q_i + v_h) . Pl_h[j - i + left] ) / sqrt(hd)     for j in [max(0, i - left), min(T - 1, i + right)]
//     ctx_i   = softmax_j(S[i][:]) V                                                        (keys outside the band: weight exactly 0)
// Pl is the local position table [left + right + 1][d]: row r is the projected sinusoid of position i - j = left - r (engine.cpp:
// ensure_local_pos_table), the same float formula as the full table, so a row is bit for bit the full table's row of that position.
// The kernel is relpos_attention_kernel (attention.hip) restricted to a key WINDOW: the workgroup of query rows i0 .. i0 + 31 keeps the
// columns [jlo, jhi] = [i0 - left, i0 + 31 + right] (clamped to the utterance) of its score block, at most left + right + 32 of them,
// whatever T is.  Window column c is key jlo + c; the content tiles, the lane-strided softmax sweeps and the AV chain run over c exactly
// as the full kernel runs over j, and every entry outside a row's own band is an exact zero of the softmax and of the AV chain.  So when
// the band covers the utterance (left, right >= T - 1: jlo = 0, the window = all keys) every score, every softmax sum and every ctx
// chain is the full kernel's, bit for bit (tests/test_gpu_local_attention.py).
#include "../pk_devmath.h"
#include "kernels.hpp"

namespace pk {

typedef float f32x4 __attribute__((ext_vector_type(4)));
static constexpr int RB = 32;   // query rows per workgroup (the ragged unit lists are built with 32-row units)

__device__ __forceinline__ float f4e_l(const float4 &v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }

template <int HD, int VCH, bool RAG, int OCC>
__global__ __launch_bounds__(256, OCC) void relpos_local_attention_kernel(const float *__restrict__ qkv, int ldq, int d, int T,
                                                                      const float *__restrict__ pos /*[left+right+1][d], sigma columns*/,
                                                                      const float *__restrict__ bias_u, const float *__restrict__ bias_v,
                                                                      float scale, float *__restrict__ ctx, int PITS, int n_rb, int n_bh,
                                                                      int ctx_bf16, int left, int right, SeqRag rg) {
    __builtin_amdgcn_s_setprio(3);
    constexpr int KQ = HD / 4;
    constexpr int NQ4 = HD / 16;
    constexpr int VPIT = HD + 16;
    constexpr int NDV = HD / 32;
    constexpr int NLV = VCH * KQ / 256;
    static_assert((VCH * KQ) % 256 == 0 && VCH % 4 == 0, "V chunk must split evenly over 256 threads");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int SPLANE = RB * PITS + 8;
    float *S = smem;                        // [4][SPLANE] score planes over the window columns c
    float *VS = smem + 4 * SPLANE;          // [VCH][VPIT] V chunk
    const int H = d / HD;
    int h, i0;
    int64_t row0;
    if constexpr (RAG) {                    // the same unit walk and XCD placement as the full kernel's ragged form
        const int id = blockIdx.x, xcd = id & 7, k = id >> 3;
        h = (k / rg.units.count) * 8 + xcd;
        if (h >= H) return;
        const RagUnit un = rg.units.u[k % rg.units.count];
        i0 = un.r0;
        T = rg.T[un.b];
        row0 = rg.T_off[un.b];
    } else {
        const int id = blockIdx.x, xcd = id & 7, k = id >> 3;
        const int rbk = k % n_rb, bh = (k / n_rb) * 8 + xcd;
        if (bh >= n_bh) return;
        h = bh % H;
        i0 = rbk * RB;
        row0 = (int64_t)(bh / H) * T;
    }
    const int rows = (T - i0) < RB ? (T - i0) : RB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, kq = lane >> 4;
    const int rt = wave & 1, cp = wave >> 1;
    const int jlo = i0 - left > 0 ? i0 - left : 0;                                   // the block's key window [jlo, jhi]
    const int jhi = i0 + RB - 1 + right < T - 1 ? i0 + RB - 1 + right : T - 1;
    const int W = jhi - jlo + 1, Wpad4 = (W + 3) & ~3;
    const int NP = left + right + 1;                                                 // rows of the local table
    const float *qb = qkv + row0 * ldq + h * HD;
    const float *kb = qb + d + (int64_t)jlo * ldq, *vb = qb + 2 * d + (int64_t)jlo * ldq;   // window key / value row c = key jlo + c
    const float *pb = pos + h * HD;
    auto sidx = [&](int il, int c) { return (c & 3) * SPLANE + il * PITS + (c >> 2); };

    float4 vf[NLV];
    auto v_issue = [&](int c0) {
#pragma unroll
        for (int i = 0; i < NLV; ++i) {
            const int e = tid + 256 * i, gr = c0 + e / KQ;
            vf[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (gr < W) vf[i] = *reinterpret_cast<const float4 *>(vb + (int64_t)gr * ldq + 4 * (e % KQ));
        }
    };
    auto v_commit = [&]() {
#pragma unroll
        for (int i = 0; i < NLV; ++i) {
            const int e = tid + 256 * i;
            lds_store16(VS + (e / KQ) * VPIT + 4 * (e % KQ), vf[i]);
        }
    };
    auto load_tile = [&](const float *base, int64_t ld, int r0, int limit, float4 (&f)[NQ4]) {
        const int r = r0 + l15;
        const bool ok = r >= 0 && r < limit;
        const float *p = base + (int64_t)(ok ? r : 0) * ld + 4 * kq;
#pragma unroll
        for (int q = 0; q < NQ4; ++q) f[q] = ok ? *reinterpret_cast<const float4 *>(p + 16 * q) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    };
    auto mma_pair = [&](const float4 (&a)[NQ4], const float4 (&b0)[NQ4], const float4 (&b1)[NQ4], f32x4 &c0, f32x4 &c1) {
        c0 = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        c1 = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int q = 0; q < NQ4; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(f4e_l(a[q], e), f4e_l(b0[q], e), c0, 0, 0, 0);
                c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(f4e_l(a[q], e), f4e_l(b1[q], e), c1, 0, 0, 0);
            }
    };
    float4 qx[NQ4];
    auto load_q_biased = [&](const float *bias) {
        load_tile(qb, ldq, i0 + rt * 16, T, qx);
        const float *br = bias + h * HD + kq;
#pragma unroll
        for (int f = 0; f < NQ4; ++f)
            qx[f] = make_float4(qx[f].x + br[16 * f], qx[f].y + br[16 * f + 4], qx[f].z + br[16 * f + 8], qx[f].w + br[16 * f + 12]);
    };
    load_q_biased(bias_u);
    const int il_base = rt * 16 + 4 * kq;
    float4 bA0[NQ4], bA1[NQ4], bB0[NQ4], bB1[NQ4];

    // ---- phase 1: content scores (q+u) K^T over the window columns ----
    {
        const int nct = (W + 15) / 16;
        auto store = [&](int t, const f32x4 &a0, const f32x4 &a1) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int il = il_base + r;
                const int c0 = t * 16 + l15, c1 = c0 + 32;
                if (c0 < Wpad4) S[sidx(il, c0)] = c0 < W ? a0[r] : 0.0f;               // columns W..Wpad4-1: zero pad of the AV chain
                if (t + 2 < nct && c1 < Wpad4) S[sidx(il, c1)] = c1 < W ? a1[r] : 0.0f;
            }
        };
        if (cp < nct) { load_tile(kb, ldq, cp * 16, W, bA0); load_tile(kb, ldq, (cp + 2) * 16, W, bA1); }
        for (int t = cp; t < nct; t += 8) {
            f32x4 a0, a1;
            if (t + 4 < nct) { load_tile(kb, ldq, (t + 4) * 16, W, bB0); load_tile(kb, ldq, (t + 6) * 16, W, bB1); }
            mma_pair(qx, bA0, bA1, a0, a1);
            store(t, a0, a1);
            if (t + 4 < nct) {
                if (t + 8 < nct) { load_tile(kb, ldq, (t + 8) * 16, W, bA0); load_tile(kb, ldq, (t + 10) * 16, W, bA1); }
                mma_pair(qx, bB0, bB1, a0, a1);
                store(t + 4, a0, a1);
            }
        }
    }
    load_q_biased(bias_v);
    // ---- phase 2: position scores (q+v) Pl^T added at column c = p - left + i - jlo for the in-band pairs only.  This wave's rows
    //      w_lo .. w_hi need table rows p in [wpmin, wpmax] (at most left + right + 1 of them) ----
    const int w_lo = i0 + rt * 16, w_hi = (w_lo + 15) < (T - 1) ? (w_lo + 15) : (T - 1);
    const int wpmin = jlo - w_hi + left > 0 ? jlo - w_hi + left : 0;
    const int wpmax = jhi - w_lo + left < NP - 1 ? jhi - w_lo + left : NP - 1;
    const int npt = (w_lo < T) ? (wpmax - wpmin) / 16 + 1 : 0;
    if (cp < npt) { load_tile(pb, d, wpmin + cp * 16, NP, bA0); load_tile(pb, d, wpmin + (cp + 2) * 16, NP, bA1); }
    __syncthreads();                                              // content scores complete
    {
        auto rmw = [&](int t, const f32x4 &a0, const f32x4 &a1) {
            int ad[8];
            bool ok[8];
            float v[8];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int il = il_base + r, i = i0 + il;
                const int pa = wpmin + t * 16 + l15, ca = pa - left + i - jlo;
                const int pc = pa + 32, cc = ca + 32;
                ok[r] = i < T && pa < NP && ca >= 0 && ca < W;
                ok[4 + r] = t + 2 < npt && i < T && pc < NP && cc >= 0 && cc < W;
                ad[r] = ok[r] ? sidx(il, ca) : 0;
                ad[4 + r] = ok[4 + r] ? sidx(il, cc) : 0;
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = S[ad[q]];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (ok[r]) S[ad[r]] = (v[r] + a0[r]) * scale;
                if (ok[4 + r]) S[ad[4 + r]] = (v[4 + r] + a1[r]) * scale;
            }
        };
        for (int t = cp; t < npt; t += 8) {
            f32x4 a0, a1;
            if (t + 4 < npt) { load_tile(pb, d, wpmin + (t + 4) * 16, NP, bB0); load_tile(pb, d, wpmin + (t + 6) * 16, NP, bB1); }
            mma_pair(qx, bA0, bA1, a0, a1);
            rmw(t, a0, a1);
            if (t + 4 < npt) {
                if (t + 8 < npt) { load_tile(pb, d, wpmin + (t + 8) * 16, NP, bA0); load_tile(pb, d, wpmin + (t + 10) * 16, NP, bA1); }
                mma_pair(qx, bB0, bB1, a0, a1);
                rmw(t + 4, a0, a1);
            }
        }
    }
    v_issue(0);
    __syncthreads();
    // ---- phase 3: softmax over each row's own band [clo, chi] of window columns, one wavefront per row, the full kernel's lane-strided
    //      sweeps over c = lane, lane + 64, ...; columns outside the band take no part in the maximum and become exact zeros ----
    {
        constexpr int NSR = RB / 4;
        float mx[NSR], sm[NSR];
        int clo[NSR], chi[NSR];
#pragma unroll
        for (int k = 0; k < NSR; ++k) {
            const int i = i0 + wave + 4 * k;
            clo[k] = (i - left > jlo ? i - left : jlo) - jlo;
            chi[k] = i < T ? (i + right < jhi ? i + right : jhi) - jlo : -1;     // rows past T: an empty band (never stored)
            mx[k] = -__builtin_huge_valf();
        }
        for (int c = lane; c < W; c += 64)
#pragma unroll
            for (int k = 0; k < NSR; ++k)
                if (c >= clo[k] && c <= chi[k]) mx[k] = fmaxf(mx[k], S[sidx(wave + 4 * k, c)]);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
            for (int k = 0; k < NSR; ++k) mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], off, 64));
#pragma unroll
        for (int k = 0; k < NSR; ++k) sm[k] = 0.0f;
        for (int c = lane; c < W; c += 64) {
            float e[NSR];
#pragma unroll
            for (int k = 0; k < NSR; ++k) e[k] = S[sidx(wave + 4 * k, c)] - mx[k];
            if (ctx_bf16 == 1) {
#pragma unroll
                for (int k = 0; k < NSR; ++k) e[k] = __builtin_amdgcn_exp2f(e[k] * 1.44269502162933349609375f);
            } else {
#pragma unroll
                for (int k = 0; k < NSR; ++k) e[k] = dexpf_nonpos(e[k]);
            }
#pragma unroll
            for (int k = 0; k < NSR; ++k) {
                if (!(c >= clo[k] && c <= chi[k])) e[k] = 0.0f;         // (whatever the exponential made of an out-of-band score)
                S[sidx(wave + 4 * k, c)] = e[k];
                sm[k] = sm[k] + e[k];
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
            for (int k = 0; k < NSR; ++k) sm[k] = sm[k] + __shfl_xor(sm[k], off, 64);
#pragma unroll
        for (int k = 0; k < NSR; ++k) sm[k] = chi[k] >= clo[k] ? sm[k] : 1.0f;   // (an in-band row holds its maximum: sum >= 1)
        if (ctx_bf16 == 1) {
#pragma unroll
            for (int k = 0; k < NSR; ++k) sm[k] = __builtin_amdgcn_rcpf(sm[k]);
            for (int c = lane; c < W; c += 64) {
                float e[NSR];
#pragma unroll
                for (int k = 0; k < NSR; ++k) e[k] = S[sidx(wave + 4 * k, c)] * sm[k];
#pragma unroll
                for (int k = 0; k < NSR; ++k) S[sidx(wave + 4 * k, c)] = e[k];
            }
        } else {
            for (int c = lane; c < W; c += 64) {
                float e[NSR];
#pragma unroll
                for (int k = 0; k < NSR; ++k) e[k] = S[sidx(wave + 4 * k, c)];
#pragma unroll
                for (int k = 0; k < NSR; ++k) e[k] = e[k] / sm[k];
#pragma unroll
                for (int k = 0; k < NSR; ++k) S[sidx(wave + 4 * k, c)] = e[k];
            }
        }
    }
    v_commit();
    lds_store_fence();
    __syncthreads();
    // ---- phase 4: ctx = softmax(S) V over the window columns (natural order from jlo; zero probabilities outside each row's band) ----
    f32x4 acc[NDV];
#pragma unroll
    for (int m = 0; m < NDV; ++m) acc[m] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const float *sa = S + kq * SPLANE + (rt * 16 + l15) * PITS;
    const float *vrow = VS + kq * VPIT + cp * 16 + l15;
    for (int c0r = 0; c0r < W; c0r += VCH) {
        const bool more = c0r + VCH < W;
        if (more) v_issue(c0r + VCH);
        const int s_end = ((W - c0r < VCH ? W - c0r : VCH) + 3) / 4;
        for (int s4 = 0; s4 < s_end; s4 += 4) {
            const float4 a = *reinterpret_cast<const float4 *>(sa + c0r / 4 + s4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (s4 + e < s_end) {
#pragma unroll
                    for (int m = 0; m < NDV; ++m)
                        acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4e_l(a, e), vrow[(s4 + e) * 4 * VPIT + m * 32], acc[m], 0, 0, 0);
                }
            }
        }
        if (more) {
            __syncthreads();
            v_commit();
            lds_store_fence();
            __syncthreads();
        }
    }
#pragma unroll
    for (int m = 0; m < NDV; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int il = il_base + r;
            if (il < rows) {
                const int64_t orow = (row0 + i0 + il) * d;
                const int col = h * HD + (cp + 2 * m) * 16 + l15;
                if (ctx_bf16 == 1) reinterpret_cast<__bf16 *>(ctx)[orow + col] = (__bf16)acc[m][r];
                else if (ctx_bf16 == 2) ctx[orow + ((col & ~15) | ((col & 3) << 2) | ((col >> 2) & 3))] = acc[m][r];
                else ctx[orow + col] = acc[m][r];
            }
        }
}

static int local_pits(int W) {                                     // the full kernel's score-plane row pitch (pits / 4 odd)
    int pits = (W + 3) / 4;
    pits = (pits + 3) & ~3;
    if (((pits / 4) & 1) == 0) pits += 4;
    return pits;
}

template <int HD, int VCH, int OCC>
static void launch_local(const float *qkv, int B, int T, int d, int n_heads, const float *pos, const float *bias_u, const float *bias_v,
                         float *ctx, hipStream_t s, int ctx_bf16, int left, int right, int W, const SeqRag &rag) {
    const float scale = 1.0f / sqrtf((float)HD);                   // src/encoder.cpp:126
    const int pits = local_pits(W);
    const int n_rb = (T + RB - 1) / RB, n_bh = B * n_heads;
    dim3 grid(((n_bh + 7) / 8) * 8 * n_rb);
    if (rag.units.u) grid = dim3((unsigned)(((n_heads + 7) / 8) * 8 * (int64_t)rag.units.count));
    const size_t lds = (size_t)(4 * (RB * pits + 8) + VCH * (HD + 16)) * sizeof(float);
    if (rag.units.u) {
        static DynLdsSlots slots_r;
        ensure_dyn_lds(slots_r, reinterpret_cast<const void *>(&relpos_local_attention_kernel<HD, VCH, true, OCC>), lds);
        hipLaunchKernelGGL((relpos_local_attention_kernel<HD, VCH, true, OCC>), grid, dim3(256), lds, s, qkv, 3 * d, d, T, pos, bias_u, bias_v, scale, ctx,
                           pits, n_rb, n_bh, ctx_bf16, left, right, rag);
        return;
    }
    static DynLdsSlots slots;
    ensure_dyn_lds(slots, reinterpret_cast<const void *>(&relpos_local_attention_kernel<HD, VCH, false, OCC>), lds);
    hipLaunchKernelGGL((relpos_local_attention_kernel<HD, VCH, false, OCC>), grid, dim3(256), lds, s, qkv, 3 * d, d, T, pos, bias_u, bias_v, scale, ctx,
                       pits, n_rb, n_bh, ctx_bf16, left, right, rag);
}

static int local_vch(int hd) { return hd == 128 ? 32 : 64; }
static size_t local_lds_bytes(int W, int hd) { return (size_t)(4 * (RB * local_pits(W) + 8) + local_vch(hd) * (hd + 16)) * sizeof(float); }

int relpos_local_attention_max_span(int hd) {
    if (hd != 32 && hd != 64 && hd != 96 && hd != 128) return -1;
    int span = -1;                                                  // left + right: the window of a block is left + right + 32 columns
    while (local_lds_bytes(span + 1 + RB, hd) <= 160 * 1024) ++span;
    return span;
}

void launch_relpos_local_attention(const float *qkv, int B, int T, int d, int n_heads, const float *pos, const float *bias_u, const float *bias_v,
                                   float *ctx, hipStream_t s, int ctx_bf16, int left, int right, const SeqRag &rag) {
    const int hd = d / n_heads;
    const int t_lds = rag.units.u ? rag.T_max : T;
    const int W = t_lds < left + right + RB ? t_lds : left + right + RB;   // widest window of any block of the launch (LDS sizing)
    const int occ = (int)((size_t)160 * 1024 / local_lds_bytes(W, hd));
    if (hd == 64) {
        if (occ >= 4) launch_local<64, 64, 4>(qkv, B, T, d, n_heads, pos, bias_u, bias_v, ctx, s, ctx_bf16, left, right, W, rag);
        else launch_local<64, 64, 3>(qkv, B, T, d, n_heads, pos, bias_u, bias_v, ctx, s, ctx_bf16, left, right, W, rag);
    } else if (hd == 128) launch_local<128, 32, 2>(qkv, B, T, d, n_heads, pos, bias_u, bias_v, ctx, s, ctx_bf16, left, right, W, rag);
    else if (hd == 32) launch_local<32, 64, 4>(qkv, B, T, d, n_heads, pos, bias_u, bias_v, ctx, s, ctx_bf16, left, right, W, rag);
    else if (hd == 96) launch_local<96, 64, 2>(qkv, B, T, d, n_heads, pos, bias_u, bias_v, ctx, s, ctx_bf16, left, right, W, rag);
}

}  // namespace pk
