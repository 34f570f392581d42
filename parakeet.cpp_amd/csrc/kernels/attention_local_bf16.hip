// parakeet.cpp_amd/csrc/kernels/attention_local_bf16.hip -- limited-context ("band") relative-position attention of the TOLERANCE-class mode
// (pk_config.gemm_bf16 with pk_model_set_local_attention_bf16): the band form of attention_bf16.hip.  Query row i of a T-frame utterance attends
// to the keys j in [max(0, i - left), min(T - 1, i + right)] only, Pl the layer's LOCAL table [left + right + 1][d] (row r = position left - r):
//     S[i][j] = ( (q_i + u_h) . k_j  +  (q_i + v_h) . Pl_h[j - i + left] ) / sqrt(hd) ,   ctx_i = softmax_j(S[i][.]) V
// Operands and roundings are the full bf16 kernel's (tests/attention_ref.py): q, k, v, Pl as bf16, ONE biased query bf16(float(q) + u) for both
// score terms, the position term as qu . Pl_p + c_h[p] with c_h[p] = (v_h - u_h) . Pl_p in fp32 (pos_cvec_kernel on the local table), fp32
// accumulation and softmax, probabilities rounded to bf16 as the PV operand, ctx stored as bf16.
// Kept from the full kernel: one workgroup = 128 query rows of one (utterance, head) as 4 waves x 32 rows; the three contractions TRANSPOSED
// (keys x queries) on v_mfma_f32_32x32x16_bf16, so the row statistics are in-lane plus one lane ^ 32 exchange and the probability registers
// are the PV B operand as they lie; K and V tiles staged in LDS once per workgroup (V sub-blocked for ds_read_b64_tr_b16, double-buffered, one
// barrier per key tile); position blocks through the wave-private skew strip at pitch 34; the XCD-aware block mapping and SeqRag's units.
// New here:
//   * Band walk.  The workgroup stages only the key tiles the union of its rows' bands touches, t in [max(0, 128 qb - left) / 32,
//     min(nkt - 1, (128 qb + 127 + right) / 32)]: O(left + right + 128) work, not O(T).  Every wave has its own narrower range
//     [max(0, i0w - left) / 32, min(nkt - 1, (i0w + 31 + right) / 32)]; outside it the wave stages and meets the barriers, nothing else.
//   * Local position rows.  Pair (i, j) of wave tile (i0w, t) reads local row j - i + left = (jj - n + 31) + (32 t - i0w + left - 31): block m
//     of the wave holds the rows (left - 31 - i0w) + 32 m + [0, 32), tile t reads blocks t and t + 1 -- the full kernel's "one new block per key
//     tile" with the base taken from left instead of T - 1.  Rows outside [0, left + right] are clamped on load: masked pairs only.  The c band
//     in LDS covers the rows the workgroup reaches, 32 (tiles walked) + 128 floats: nothing of size T is in LDS, so there is no length limit.
//   * Mask.  A score is -inf when j - i > right, i - j > left or j >= T.  A tile wholly inside the band of all 32 rows of the wave skips the
//     pass (wave-uniform test).
//   * Edge tiles.  At a band edge some rows of a wave have no live key in the tile (left 40, right 0: the first tile of a wave holds keys for
//     its first 8 rows only): their running maximum is still -inf and exp2(-inf - (-inf)) would be NaN.  The maximum that is SUBTRACTED is
//     replaced by 0 while the row has seen no live key (alpha = exp2(-inf) = 0, probabilities exp2(-inf) = 0); every valid row has its own
//     key j = i in some tile, so its normaliser ends positive.
#include "../pk_devmath.h"
#include "kernels.hpp"

namespace pk {

typedef float lb_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 lb_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 lb_bf16x4 __attribute__((ext_vector_type(4)));
typedef short lb_s16x4 __attribute__((ext_vector_type(4)));

static constexpr int LB_QB = 128;       // query rows per workgroup (4 waves x 32)
static constexpr int LB_SKP = 34;       // skew strip pitch (floats)

__device__ __forceinline__ int lb_rowidx(int r, int g) { return (r & 3) + 8 * (r >> 2) + 4 * g; }     // row of accumulator register r (32x32 C layout)

// key tiles a workgroup walks at most: 4 (its 128 rows) + ceil(left / 32) + ceil(right / 32)
static inline int lb_max_tiles(int left, int right) { return 4 + (left + 31) / 32 + (right + 31) / 32; }

template <int HD, bool RAG>
__global__ __launch_bounds__(256, 2) void relpos_local_attention_bf16_kernel(const __bf16 *__restrict__ qkv, int ldq, int d, int T,
                                                                             const __bf16 *__restrict__ pos /*[left + right + 1][d]*/,
                                                                             const float *__restrict__ cvec /*[H][left + right + 1]*/,
                                                                             const float *__restrict__ bias_u, float scale_log2e, __bf16 *__restrict__ ctx,
                                                                             int n_qb, int n_bh, int left, int right, SeqRag rg) {
    constexpr int NK = HD / 16;          // MFMA k-steps of a contraction over the head dimension
    constexpr int NDT = HD / 32;         // 32-wide dv tiles of ctx^T
    constexpr int VCH = HD / 8;          // 16-byte chunks per V row
    constexpr int NV = 32 * VCH / 256;   // V chunks per thread per key tile
    static_assert(NV >= 1, "HD >= 64");
    extern __shared__ __attribute__((aligned(16))) unsigned char lb_smem[];
    constexpr int KP = HD * 2 + 16;      // K tile row pitch in bytes (+16: the row-per-lane 16-byte fragment reads spread over the banks)
    __bf16 *Vimg = reinterpret_cast<__bf16 *>(lb_smem);                          // [2][32 * HD]   sub-blocked V tiles
    unsigned char *Kimg = lb_smem + 2 * 32 * HD * 2;                             // [2][32 keys][KP bytes]  K tiles, natural rows
    float *skew = reinterpret_cast<float *>(Kimg + 2 * 32 * KP);                 // [4][64 * LB_SKP]
    float *cb = skew + 4 * 64 * LB_SKP;                                          // [32 (tiles walked) + 128]  c band of this workgroup
    __builtin_amdgcn_s_setprio(3);

    const int H = d / HD;
    int h, qb;
    int64_t row0;                                                   // first row of this utterance in the (packed) row axis of qkv / ctx
    if constexpr (RAG) {   // ragged batch (kernels.hpp: SeqRag; attention_bf16.hip has the same mapping): this utterance's own length
        const int id = blockIdx.x, xcd = id & 7, k = id >> 3;
        h = (k / rg.units.count) * 8 + xcd;
        if (h >= H) return;
        const RagUnit un = rg.units.u[k % rg.units.count];
        qb = un.r0 / LB_QB;
        T = rg.T[un.b];
        row0 = rg.T_off[un.b];
    } else {   // the query blocks of one (utterance, head) take consecutive slots of ONE XCD (block id % 8 = XCD): neighbours share K / V tiles in its L2
        const int id = blockIdx.x, xcd = id & 7, k = id >> 3;
        qb = k % n_qb;
        const int bh = (k / n_qb) * 8 + xcd;
        if (bh >= n_bh) return;
        h = bh % H;
        row0 = (int64_t)(bh / H) * T;
    }
    const int nkt = (T + 31) / 32, Pl = left + right + 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 31, g = lane >> 5;
    const int i0 = qb * LB_QB, i0w = i0 + 32 * wave;                // first query row of the workgroup / of this wave
    const bool active = i0w < T;                                    // wave-uniform
    // key tiles of the workgroup, and of this wave (an inactive wave has none: it only stages)
    const int t_lo = (i0 > left ? i0 - left : 0) >> 5;
    const int t_hi = min(nkt - 1, (i0 + LB_QB - 1 + right) >> 5);
    const int tw_lo = (i0w > left ? i0w - left : 0) >> 5;
    const int tw_hi = active ? min(nkt - 1, (i0w + 31 + right) >> 5) : -1;
    const __bf16 *qrow = qkv + row0 * ldq + h * HD;                 // q of (b, h); k at + d, v at + 2 d
    const __bf16 *prow = pos + h * HD;
    float *sk = skew + wave * 64 * LB_SKP;
    const int base0 = left - 31 - i0w;                              // local row of band row 0 of block 0 for this wave
    const int cb_len = 32 * (t_hi - t_lo + 1) + 128;

    for (int i = tid; i < cb_len; i += 256) {                       // c band: local row (left - 127 - i0 + 32 t_lo) + i
        int p = left - (LB_QB - 1) - i0 + 32 * t_lo + i;
        p = p < 0 ? 0 : (p > Pl - 1 ? Pl - 1 : p);
        cb[i] = cvec[(int64_t)h * Pl + p];
    }
    // V / K tile staging (workgroup-cooperative): chunk c = tid + 256 i -> key c / VCH, 8 columns at 8 (c % VCH); rows past T - 1 are clamped
    float4 vreg[NV], kst[NV];
    auto kv_load = [&](int t) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = tid + 256 * i, key = c / VCH, ch = c % VCH;
            int kr = 32 * t + key;
            kr = kr < T ? kr : T - 1;
            const __bf16 *r = qrow + (int64_t)kr * ldq + 8 * ch;
            vreg[i] = *reinterpret_cast<const float4 *>(r + 2 * d);
            kst[i] = *reinterpret_cast<const float4 *>(r + d);
        }
    };
    auto kv_store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = tid + 256 * i, key = c / VCH, ch = c % VCH;
            const int q4 = key >> 2, pq = q4 >> 1, gq = q4 & 1, dv16 = ch >> 1, dt = dv16 >> 1, dvh = dv16 & 1;
            const int blk = (pq * NDT + dt) * 4 + gq * 2 + dvh;
            lds_store16(Vimg + buf * 32 * HD + blk * 64 + (key & 3) * 16 + (ch & 1) * 8, vreg[i]);
            lds_store16(Kimg + buf * 32 * KP + key * KP + ch * 16, kst[i]);
        }
    };
    // position block m: A operand straight from L2, lane (row n, half g) takes the 8 k of step s at 16 s + 8 g
    lb_bf16x8 preg[NK], qreg[NK];
    auto p_load = [&](int m) {
        int pr = base0 + 32 * m + n;
        pr = pr < 0 ? 0 : (pr > Pl - 1 ? Pl - 1 : pr);
        const __bf16 *p = prow + (int64_t)pr * d + 8 * g;
#pragma unroll
        for (int s = 0; s < NK; ++s) preg[s] = *reinterpret_cast<const lb_bf16x8 *>(p + 16 * s);
    };
    // the 16 c values of block m this lane adds (band rows lb_rowidx(r, g): four runs of four floats), read before the strip stores
    auto c_load = [&](int m, float (&cv)[16]) {
        const float4 *c4 = reinterpret_cast<const float4 *>(cb + 96 - 32 * wave + 32 * (m - t_lo) + 4 * g);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float4 c = c4[2 * k];
            cv[4 * k] = c.x; cv[4 * k + 1] = c.y; cv[4 * k + 2] = c.z; cv[4 * k + 3] = c.w;
        }
    };

    kv_load(t_lo);
    if (active) {
        int qr = i0w + n;
        qr = qr < T ? qr : T - 1;
        const __bf16 *qp = qrow + (int64_t)qr * ldq + 8 * g;
        const float *bu = bias_u + h * HD + 8 * g;
#pragma unroll
        for (int s = 0; s < NK; ++s) {
            const lb_bf16x8 raw = *reinterpret_cast<const lb_bf16x8 *>(qp + 16 * s);
#pragma unroll
            for (int e = 0; e < 8; ++e) qreg[s][e] = (__bf16)((float)raw[e] + bu[16 * s + e]);        // (q + u) as the reference forms it, rounded once
        }
        p_load(tw_lo);
    }
    kv_store(t_lo & 1);
    lds_store_fence();
    __syncthreads();                                                // tile t_lo and the c band are in LDS
    if (active) {   // the wave's first block (+ c) into strip half tw_lo & 1; block tw_lo + 1 waits in registers for the wave's first tile
        lb_f32x16 ga;
#pragma unroll
        for (int r = 0; r < 16; ++r) ga[r] = 0.0f;
#pragma unroll
        for (int s = 0; s < NK; ++s) ga = __builtin_amdgcn_mfma_f32_32x32x16_bf16(preg[s], qreg[s], ga, 0, 0, 0);
        float cv[16];
        c_load(tw_lo, cv);
#pragma unroll
        for (int r = 0; r < 16; ++r) sk[(32 * (tw_lo & 1) + lb_rowidx(r, g)) * LB_SKP + n] = ga[r] + cv[r];
        p_load(tw_lo + 1);
    }

    lb_f32x16 O[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) O[dt][r] = 0.0f;
    float m_run = -__builtin_huge_valf(), l_run = 0.0f;

    for (int t = t_lo; t <= t_hi; ++t) {
        const bool more = t < t_hi;
        if (more) kv_load(t + 1);
        if (t >= tw_lo && t <= tw_hi) {                             // (wave-uniform) this wave's band reaches tile t
            // ---- content scores, transposed: S^T[key][query], and position block t + 1: two independent chains of NK MFMAs, issued alternately ----
            lb_f32x16 sa, ga;
#pragma unroll
            for (int r = 0; r < 16; ++r) { sa[r] = 0.0f; ga[r] = 0.0f; }
            float cv[16];
            c_load(t + 1, cv);                                      // (under the MFMA chains)
            const unsigned char *kb = Kimg + (t & 1) * 32 * KP + n * KP + 16 * g;
#pragma unroll
            for (int s = 0; s < NK; ++s) {
                const lb_bf16x8 ka = *reinterpret_cast<const lb_bf16x8 *>(kb + 32 * s);
                sa = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, qreg[s], sa, 0, 0, 0);
                ga = __builtin_amdgcn_mfma_f32_32x32x16_bf16(preg[s], qreg[s], ga, 0, 0, 0);
            }
            if (t < tw_hi) p_load(t + 2);
            {   // block t + 1 (+ c) into the wave's skew strip, half (t + 1) & 1; then the skewed read of blocks t and t + 1
                const int m = t + 1;
#pragma unroll
                for (int r = 0; r < 16; ++r) sk[(32 * (m & 1) + lb_rowidx(r, g)) * LB_SKP + n] = ga[r] + cv[r];
            }
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            float sv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int jj = lb_rowidx(r, g);
                const int xr = jj - n + 31;                          // band row relative to block t: 0 .. 62
                const int phys = 32 * ((t + (xr >> 5)) & 1) + (xr & 31);
                sv[r] = (sa[r] + sk[phys * LB_SKP + n]) * scale_log2e;            // (content + position) * scale, in the exp2 domain
            }
            const int dj = 32 * t - i0w;                             // j - i of (key 0, query 0) of this wave tile
            if (dj + 31 > right || 31 - dj > left || 32 * t + 32 > T) {   // (wave-uniform) some pair of the tile is outside the band or past the end
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int jj = lb_rowidx(r, g), o = dj + jj - n;
                    sv[r] = (o <= right && -o <= left && 32 * t + jj < T) ? sv[r] : -__builtin_huge_valf();
                }
            }
            float mloc = -__builtin_huge_valf();
#pragma unroll
            for (int r = 0; r < 16; ++r) mloc = fmaxf(mloc, sv[r]);
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                 // the strip half of block t is overwritten next iteration
            // ---- online softmax: lanes n and n + 32 hold the two halves of query n's keys ----
            mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
            const float m_new = fmaxf(m_run, mloc);
            const float m_sub = m_new == -__builtin_huge_valf() ? 0.0f : m_new;    // a row with no live key so far: alpha and its probabilities are 0, not NaN
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_sub);
            float psum = 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                sv[r] = __builtin_amdgcn_exp2f(sv[r] - m_sub);
                psum = psum + sv[r];
            }
            l_run = l_run * alpha + psum;
            m_run = m_new;
            if (__ballot(alpha != 1.0f) != 0ull) {                  // (wave-uniform) the running maximum moved for some query: rescale ctx^T
#pragma unroll
                for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) O[dt][r] = O[dt][r] * alpha;
            }
            // ---- ctx^T += V^T P^T : two k-steps of 16 keys; the probability registers are the B operand as they lie ----
            const __bf16 *vb = Vimg + (t & 1) * 32 * HD + lane * 4;
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                lb_bf16x8 pB;
#pragma unroll
                for (int e = 0; e < 8; ++e) pB[e] = (__bf16)sv[8 * st + e];
#pragma unroll
                for (int dt = 0; dt < NDT; ++dt) {
                    const lb_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) lb_s16x4 *)(vb + ((2 * st) * NDT + dt) * 256));
                    const lb_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) lb_s16x4 *)(vb + ((2 * st + 1) * NDT + dt) * 256));
                    lb_s16x4 both[2] = {lo, hi};
                    lb_bf16x8 vA;
                    __builtin_memcpy(&vA, both, 16);
                    O[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vA, pB, O[dt], 0, 0, 0);
                }
            }
        }
        if (more) {
            kv_store((t + 1) & 1);
            lds_store_fence();
        }
        __syncthreads();                                            // tile t + 1 visible; every wave is done with tile t's image
    }
    if (!active) return;
    l_run = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = __builtin_amdgcn_rcpf(l_run);
    const int i = i0w + n;
    if (i < T) {
        __bf16 *orow = ctx + (row0 + i) * d + h * HD + 4 * g;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                lb_bf16x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = (__bf16)(O[dt][4 * rq + e] * inv);
                *reinterpret_cast<lb_bf16x4 *>(orow + 32 * dt + 8 * rq) = o;          // dv = 32 dt + 8 rq + 4 g + e
            }
    }
}

size_t relpos_local_attention_bf16_lds_bytes(int left, int right, int hd) {
    if (hd != 64 && hd != 128) return 0;
    return (size_t)2 * 32 * hd * 2 + (size_t)2 * 32 * (hd * 2 + 16) + (size_t)4 * 64 * LB_SKP * 4 + (size_t)(32 * lb_max_tiles(left, right) + 128) * 4;
}
int relpos_local_attention_bf16_block_rows(int) { return LB_QB; }

template <int HD>
static void launch_local_att_bf16(const void *qkv, int B, int T, int d, int n_heads, const void *pos, const float *cvec, const float *bias_u, void *ctx,
                                  hipStream_t s, int left, int right, const SeqRag &rag) {
    if (rag.units.u) T = rag.T_max;
    const int n_qb = (T + LB_QB - 1) / LB_QB, n_bh = B * n_heads;
    const float scale_log2e = (1.0f / sqrtf((float)HD)) * 1.44269504088896340736f;
    const size_t lds = relpos_local_attention_bf16_lds_bytes(left, right, HD);
    if (rag.units.u) {
        auto kern = &relpos_local_attention_bf16_kernel<HD, true>;
        static DynLdsSlots slots_r;
        ensure_dyn_lds(slots_r, reinterpret_cast<const void *>(kern), lds);
        const dim3 grid((unsigned)(((n_heads + 7) / 8) * 8 * (int64_t)rag.units.count));
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, static_cast<const __bf16 *>(qkv), 3 * d, d, T, static_cast<const __bf16 *>(pos), cvec, bias_u,
                           scale_log2e, static_cast<__bf16 *>(ctx), n_qb, n_bh, left, right, rag);
        return;
    }
    auto kern = &relpos_local_attention_bf16_kernel<HD, false>;
    static DynLdsSlots slots;
    ensure_dyn_lds(slots, reinterpret_cast<const void *>(kern), lds);
    const dim3 grid((unsigned)(((n_bh + 7) / 8) * 8 * (int64_t)n_qb));
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, static_cast<const __bf16 *>(qkv), 3 * d, d, T, static_cast<const __bf16 *>(pos), cvec, bias_u,
                       scale_log2e, static_cast<__bf16 *>(ctx), n_qb, n_bh, left, right, rag);
}

void launch_relpos_local_attention_bf16(const void *qkv_bf16, int B, int T, int d, int n_heads, const void *pos_bf16, const float *cvec, const float *bias_u,
                                        void *ctx_bf16, hipStream_t s, int left, int right, const SeqRag &rag) {
    const int hd = d / n_heads;
    if (hd == 128) launch_local_att_bf16<128>(qkv_bf16, B, T, d, n_heads, pos_bf16, cvec, bias_u, ctx_bf16, s, left, right, rag);
    else if (hd == 64) launch_local_att_bf16<64>(qkv_bf16, B, T, d, n_heads, pos_bf16, cvec, bias_u, ctx_bf16, s, left, right, rag);
}

}  // namespace pk
