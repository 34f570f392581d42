// parakeet.cpp_amd/csrc/kernels/neural_lm.hip -- the two kernels of the Transformer LM (neural_lm.cpp) that are its own:
// the embedding stage and the output head fused with the log-softmax and the target pick.  Its third, the causal attention, is an instantiation
// of the band kernel (attention.hip: CAUSAL).  Everything is fp32; ordinary launches on the caller's stream.
#include "../pk_devmath.h"
#include "kernels.hpp"

namespace pk {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- embedding: h[r] = tok_emb[x_r] + pos_emb[i_r] over the packed positions, 16 bytes per access --------------------------------------------------
// One thread per float4 of the output.  The BOS shift happens here: position 0 of a string reads bos, position i its token i - 1; the thread of a row's
// first float4 also writes the row's target (token i, or eos at the end term) for the head kernel.
__global__ __launch_bounds__(256) void nlm_embed_kernel(const float *__restrict__ tok_emb, const float *__restrict__ pos_emb, const int32_t *__restrict__ ids,
                                                        const int32_t *__restrict__ id_off, const int32_t *__restrict__ row_off,
                                                        const int32_t *__restrict__ row_str, int bos, int eos, int d4, int64_t rows, float *__restrict__ h,
                                                        int32_t *__restrict__ tgt) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t r = e / d4;
    if (r >= rows) return;
    const int c = (int)(e - r * d4);
    const int b = row_str[r], i = (int)(r - row_off[b]), o = id_off[b], n = id_off[b + 1] - o;
    const int x = i == 0 ? bos : ids[o + i - 1];
    const float4 t = reinterpret_cast<const float4 *>(tok_emb + (int64_t)x * d4 * 4)[c];
    const float4 p = reinterpret_cast<const float4 *>(pos_emb + (int64_t)i * d4 * 4)[c];
    reinterpret_cast<float4 *>(h + r * d4 * 4)[c] = make_float4(t.x + p.x, t.y + p.y, t.z + p.z, t.w + p.w);
    if (c == 0) tgt[r] = i < n ? ids[o + i] : eos;
}

void launch_nlm_embed(const float *tok_emb, const float *pos_emb, const int32_t *ids, const int32_t *id_off, const int32_t *row_off, const int32_t *row_str,
                      int bos, int eos, int d, int64_t rows, float *h, int32_t *tgt, hipStream_t s) {
    const int d4 = d / 4;
    const int64_t n = rows * d4;
    hipLaunchKernelGGL(nlm_embed_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, tok_emb, pos_emb, ids, id_off, row_off, row_str, bos, eos, d4, rows, h,
                       tgt);
}

// ---- head: lp[r] = logit_r[tgt_r] - logsumexp_c logit_r[c], the logits in registers only ------------------------------------------------------------
// A workgroup (four waves) owns HM = 64 rows and walks every 64-column tile of W.  Per tile a K loop in chunks of 32 stages the rows and the weight
// rows in LDS and runs v_mfma_f32_16x16x4_f32: wave w holds rows 16 w .. 16 w + 15 against the tile's four 16-column blocks, each accumulator the
// natural-k fma chain from zero the project's fp32 GEMMs produce (step s of chunk c consumes k = 32 c + 4 s + kq).  LDS holds a staged row "k-planar":
// the element of k = 4 s + kq of the chunk sits at kq * 8 + s, so one 16-byte read is a lane's operand of four consecutive steps.
// C layout: column = lane & 15, row = 4 (lane >> 4) + r.  So a lane sees, of each of its four rows, the columns = lane & 15 (mod 16): it keeps a running
// (maximum, sum of exponentials) over THOSE columns alone -- no exchange inside the walk -- and the 16 lanes of a row merge theirs once at the end
// (xor 8, 4, 2, 1).  The order of every operation depends on the column index only: a row's bits do not depend on which rows it is packed with.
// Columns >= V of the last tile take part in nothing; a lane that saw no column carries (-inf, 0).
static constexpr int HM = 64, HN = 64, HK = 32, HPIT = 36;

__device__ __forceinline__ float nlm_rescale(float s, float m, float m_new) {        // s e^(m - m_new); nothing summed yet: 0
    return m > -__builtin_huge_valf() ? s * dexpf_nonpos(m - m_new) : 0.0f;
}

__global__ __launch_bounds__(256) void nlm_head_logp_kernel(const float *__restrict__ h, int64_t ldh, const float *__restrict__ W, int64_t ldw,
                                                            const float *__restrict__ bias, const int32_t *__restrict__ tgt, int64_t rows, int V, int d,
                                                            float *__restrict__ lp) {
    __shared__ __attribute__((aligned(16))) float As[HM * HPIT], Ws[HN * HPIT];
    const float NEG = -__builtin_huge_valf();
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, kq = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * HM;
    // staging: thread -> two (row, float4 j) slots of the 64 x 32 chunk of each operand
    const int sr0 = tid >> 3, sj = tid & 7;                         // rows sr0 and sr0 + 32, floats 4 sj .. 4 sj + 3 of the chunk
    float m[4], sm[4], tl[4];
    int tg[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t rr = row0 + wave * 16 + 4 * kq + r;
        m[r] = NEG; sm[r] = 0.0f; tl[r] = NEG;
        tg[r] = rr < rows ? tgt[rr] : -1;
    }
    const int nk = d / HK;
    for (int n0 = 0; n0 < V; n0 += HN) {
        f32x4 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        float4 ga[2], gw[2];
        auto fetch = [&](int kc) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int sr = sr0 + 32 * i;
                const int64_t gr = row0 + sr;
                const int gc = n0 + sr;
                ga[i] = gr < rows ? *reinterpret_cast<const float4 *>(h + gr * ldh + kc * HK + 4 * sj) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                gw[i] = gc < V ? *reinterpret_cast<const float4 *>(W + (int64_t)gc * ldw + kc * HK + 4 * sj) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
        };
        fetch(0);
        for (int kc = 0; kc < nk; ++kc) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                float *a = As + (sr0 + 32 * i) * HPIT + sj, *w = Ws + (sr0 + 32 * i) * HPIT + sj;
                a[0] = ga[i].x; a[8] = ga[i].y; a[16] = ga[i].z; a[24] = ga[i].w;
                w[0] = gw[i].x; w[8] = gw[i].y; w[16] = gw[i].z; w[24] = gw[i].w;
            }
            __syncthreads();
            if (kc + 1 < nk) fetch(kc + 1);                         // the next chunk's loads fly under this chunk's chains
            const float *ap = As + (wave * 16 + l15) * HPIT + kq * 8;
            const float4 a0 = *reinterpret_cast<const float4 *>(ap), a1 = *reinterpret_cast<const float4 *>(ap + 4);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float *bp = Ws + (t * 16 + l15) * HPIT + kq * 8;
                const float4 b0 = *reinterpret_cast<const float4 *>(bp), b1 = *reinterpret_cast<const float4 *>(bp + 4);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, b0.x, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, b0.y, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, b0.z, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, b0.w, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, b1.x, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, b1.y, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, b1.z, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, b1.w, acc[t], 0, 0, 0);
            }
            __syncthreads();
        }
        // the tile's 4 x 4 logits of this lane into its running state: the columns in ascending order, one rescale per tile
        float bv[4];
        bool in[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int c = n0 + t * 16 + l15;
            in[t] = c < V;
            bv[t] = (bias && in[t]) ? bias[c] : 0.0f;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float x[4], mx = m[r];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                x[t] = bias ? acc[t][r] + bv[t] : acc[t][r];
                if (in[t]) mx = fmaxf(mx, x[t]);
                if (in[t] && n0 + t * 16 + l15 == tg[r]) tl[r] = x[t];
            }
            if (in[0]) {                                            // (the lane's first column of the tile exists: mx is finite)
                float s = nlm_rescale(sm[r], m[r], mx);
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (in[t]) s = s + dexpf_nonpos(x[t] - mx);
                sm[r] = s;
                m[r] = mx;
            }
        }
    }
    // the 16 lanes of a row: (m, s) pairs merged pairwise, the same value on both sides of every exchange; the target's logit sits in one lane
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float mo = __shfl_xor(m[r], off, 64), so = __shfl_xor(sm[r], off, 64), to = __shfl_xor(tl[r], off, 64);
            const float mn = fmaxf(m[r], mo);
            const float a = nlm_rescale(sm[r], m[r], mn), b = nlm_rescale(so, mo, mn);
            sm[r] = a + b;                                           // (commutative: both sides of the exchange get the same bits)
            m[r] = mn;
            tl[r] = fmaxf(tl[r], to);
        }
    if (l15 == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t rr = row0 + wave * 16 + 4 * kq + r;
            if (rr < rows) lp[rr] = tl[r] - (m[r] + dlogf(sm[r]));
        }
    }
}

void launch_nlm_head_logp(const float *h, int64_t ldh, const float *W, int64_t ldw, const float *bias, const int32_t *tgt, int64_t rows, int V, int d,
                          float *lp, hipStream_t s) {
    hipLaunchKernelGGL(nlm_head_logp_kernel, dim3((unsigned)((rows + HM - 1) / HM)), dim3(256), 0, s, h, ldh, W, ldw, bias, tgt, rows, V, d, lp);
}

}  // namespace pk
