// parakeet.cpp_amd/csrc/kernels/ctc_beam.hip -- CTC prefix beam search on the device.
//
// The reference's roadmap "Beam search decoding -- CTC prefix beam search ... with configurable width" (README.md:494).  Three kernels (the walk in two instantiations) over the [rows][V]
// log-softmax rows that logsoftmax_argmax_kernel writes; every value they produce is specified operation by operation
// (tests/ctc_beam_ref.py is that specification in Python) and compared bit for bit.
//
//   ctc_topk_kernel        one wavefront per row: the K best non-blank (value, id) pairs, sorted (value down, id up), + lp[blank].
//                          K passes of a 64-bit key minimum (key = inverted order-preserving image of the value << 32 | id); rows of up to
//                          1280 columns are held in registers (20 per lane), longer rows are re-read (L2 resident).
//   ctc_beam_walk_kernel   one 256-thread workgroup per utterance, frames in order (ragged extents through SeqRag).  Beam state (double
//                          buffered) and the candidate keys live in LDS.  Candidate e = i * (K + 1) + j (prefix of rank i; j = 0 stay, j > 0
//                          extension by the frame's (j-1)-th token) belongs to thread e % 256 for the whole walk, which keeps its
//                          p_b / p_nb / score in registers and publishes one 64-bit key (score, parent rank, stay / extend, token id: exactly
//                          the selection order, unique per candidate).  The table is indexed by e itself -- consecutive threads write
//                          consecutive 8-byte words (no bank conflict), and the rank count reads one word for all lanes (a broadcast).
//                          Selection: rank of a candidate = number of smaller keys; rank < W survives and IS its place in the next beam, so
//                          no sort, no atomics, and a new prefix gets node 1 + t W + rank of the pool (parent, token) -- at most W per frame.
//                          Prefix identity = (64-bit chained hash of the token string, length), kept per beam entry together with the
//                          parent string's hash: an extension that equals a beam prefix is found by hash however its nodes were linked.
//                          TWO barriers per frame: candidates -> [barrier] -> rank / next beam / next frame's tokens -> [barrier].
//     <kLm = true>         the same walk with n-gram LM shallow fusion: a beam entry carries two more values, the LM
//                          automaton's state and the prefix's LM score (512 bytes of LDS more); an extension costs one lookup -- per back-off
//                          level a 16-byte state record, a binary search over the state's sorted arc tokens and an 8-byte arc record, all
//                          dependent global loads of the candidate's own thread, ended by the dense table of the empty context -- and only
//                          live extensions that are not merged away look up (at most W K per frame and utterance).  Keys order by score + lm.
//   ctc_beam_align_kernel  one workgroup per (utterance, hypothesis): walks the node chain back into ids, then the max-plus forced alignment
//                          on the 2 L + 1 lattice (alpha double buffered in LDS, one barrier per frame, one back-pointer byte per cell in
//                          global scratch) and its back-trace into start / end / conf.
//
// Code objects (hipcc -O3 --offload-arch=gfx950, from the .s of -save-temps):
//   ctc_topk_kernel<20>    56 VGPR   70 SGPR  LDS 0        no scratch, no spill
//   ctc_topk_kernel<0>     24 VGPR   34 SGPR  LDS 0        no scratch, no spill
//   ctc_beam_walk_kernel<false>  91 VGPR  106 SGPR  LDS 11536 B  no scratch; 0 VGPR spills, 2 SGPRs spilled to VGPR lanes
//   ctc_beam_walk_kernel<true>  103 VGPR  106 SGPR  LDS 12048 B  no scratch; 0 VGPR spills, 13 SGPRs spilled to VGPR lanes
//   ctc_beam_align_kernel  18 VGPR   57 SGPR  LDS dynamic (5 Tmax + 2 words with timestamps, else 0)  no scratch, no spill
#include <type_traits>

#include "kernels.hpp"
#include "ngram_lm_dev.hpp"
#include "../pk_devmath.h"

namespace pk {

namespace {

constexpr unsigned long long kBeamDead = ~0ull;                    // key of a candidate that is not selectable (merged away, or score -inf)

// order-preserving image of a float, inverted: a LARGER value gives a SMALLER word.  (+ 0: -0.0 and 0.0 are one value)
__device__ __forceinline__ unsigned beam_ord_desc(float v) {
    unsigned u = __float_as_uint(v + 0.0f);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~u;
}
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long k) {
    wave_butterfly([&](auto off) {
        constexpr int O = decltype(off)::value;
        const unsigned hi = (unsigned)wave_xor_i<O>((int)(unsigned)(k >> 32)), lo = (unsigned)wave_xor_i<O>((int)(unsigned)k);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        if (o < k) k = o;
    });
    return k;
}
// hash of (string + c) from the hash of the string: the splitmix64 finaliser (a bijection) of h + golden * (c + 1)
__device__ __forceinline__ unsigned long long beam_hash(unsigned long long h, int c) {
    unsigned long long z = h + 0x9E3779B97F4A7C15ull * (unsigned long long)(unsigned)(c + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

}  // namespace

// ---- top-K per row ---------------------------------------------------------------------------------------------------
template <int NPL>
__global__ __launch_bounds__(256) void ctc_topk_kernel(const float *__restrict__ lp, int64_t rows, int V, int blank, int K,
                                                       float *__restrict__ tk_val, int *__restrict__ tk_id, float *__restrict__ lpb) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float *x = lp + row * V;
    float reg[NPL > 0 ? NPL : 1];
    if constexpr (NPL > 0) {
#pragma unroll
        for (int u = 0; u < NPL; ++u) {
            const int i = lane + 64 * u;
            reg[u] = i < V ? x[i] : 0.0f;
        }
    }
    unsigned long long last = 0;
    for (int k = 0; k < K; ++k) {
        unsigned long long best = kBeamDead;
        auto consider = [&](float v, int i) {
            const unsigned long long key = ((unsigned long long)beam_ord_desc(v) << 32) | (unsigned)i;
            if (i != blank && (k == 0 || key > last) && key < best) best = key;
        };
        if constexpr (NPL > 0) {
#pragma unroll
            for (int u = 0; u < NPL; ++u) {
                const int i = lane + 64 * u;
                if (i < V) consider(reg[u], i);
            }
        } else {
            for (int i = lane; i < V; i += 64) consider(x[i], i);
        }
        best = wave_min_u64(best);
        last = best;
        if (lane == 0) {
            const int id = (int)(unsigned)(best & 0xffffffffu);     // K <= V - 1: a token is always left
            tk_id[row * K + k] = id;
            tk_val[row * K + k] = x[id];                            // (the value's own bits, not the key's canonical zero)
        }
    }
    if (lane == 0) lpb[row] = x[blank];
}
void launch_ctc_beam_topk(const float *lp, int64_t rows, int V, int blank, int K, float *tk_val, int *tk_id, float *lpb, hipStream_t s) {
    const dim3 grid((unsigned)((rows + 3) / 4));
    if (V <= 64 * 20) hipLaunchKernelGGL(ctc_topk_kernel<20>, grid, dim3(256), 0, s, lp, rows, V, blank, K, tk_val, tk_id, lpb);
    else hipLaunchKernelGGL(ctc_topk_kernel<0>, grid, dim3(256), 0, s, lp, rows, V, blank, K, tk_val, tk_id, lpb);
}

// ---- the walk ----------------------------------------------------------------------------------------------------------
namespace {
constexpr int kBeamCPT = (kBeamMaxWidth * (kBeamMaxPrune + 1) + 255) / 256;      // candidates per thread (5)
struct BeamLds {
    unsigned long long key[kBeamMaxWidth * (kBeamMaxPrune + 1)];
    unsigned long long hash[2][kBeamMaxWidth], phash[2][kBeamMaxWidth];
    float pb[2][kBeamMaxWidth], pnb[2][kBeamMaxWidth], tot[2][kBeamMaxWidth];
    int node[2][kBeamMaxWidth], last[2][kBeamMaxWidth], len[2][kBeamMaxWidth];
    float fval[2][kBeamMaxPrune], flpb[2];
    int fid[2][kBeamMaxPrune];
    int nb[2];
};
// n-gram LM shallow fusion (kLm): two more values per beam entry, the LM automaton's state after the prefix and the
// prefix's LM score lm = sum over its tokens of (alpha * lookup + beta), a function of the token string alone
struct BeamLmLds {
    BeamLds b;
    int lmstate[2][kBeamMaxWidth];
    float lm[2][kBeamMaxWidth];
};
__device__ __forceinline__ BeamLds &beam_lds(BeamLds &s) { return s; }
__device__ __forceinline__ BeamLds &beam_lds(BeamLmLds &s) { return s.b; }
__device__ __forceinline__ const BeamWalkArgs &beam_args(const BeamWalkArgs &a) { return a; }
__device__ __forceinline__ const BeamWalkArgs &beam_args(const BeamLmWalkArgs &a) { return a.w; }
}  // namespace

// kLm: a candidate is selectable exactly as without; its key orders by f = sc + lm where the unfused walk orders by sc.  Merges, node pool,
// hashes and barriers are one code.  (The unfused instantiation takes BeamWalkArgs alone: its kernarg is not the fused one's.)
template <bool kLm>
__global__ __launch_bounds__(256) void ctc_beam_walk_kernel(std::conditional_t<kLm, BeamLmWalkArgs, BeamWalkArgs> la) {
    __shared__ std::conditional_t<kLm, BeamLmLds, BeamLds> sl;
    BeamLds &s = beam_lds(sl);
    const BeamWalkArgs &a = beam_args(la);
    const int b = blockIdx.x, tid = threadIdx.x;
    int T = a.T;
    int64_t in0 = (int64_t)b * T;                                   // first frame of this utterance in the (packed) frame axis
    if (a.rg.T) { in0 = a.rg.T_off[b]; T = a.rg.T[b]; }             // ragged batch
    const int W = a.W, K = a.K, KP = K + 1;
    const float NEG = -__builtin_huge_valf();
    int2 *nodes = a.nodes + (int64_t)b * a.node_pitch;
    int ci[kBeamCPT], cj[kBeamCPT];                                 // this thread's candidates: prefix rank, move
#pragma unroll
    for (int u = 0; u < kBeamCPT; ++u) {
        const int e = tid + 256 * u;
        ci[u] = e / KP;
        cj[u] = e - ci[u] * KP;
    }
    if (tid == 0) {
        s.pb[0][0] = 0.0f; s.pnb[0][0] = NEG; s.tot[0][0] = 0.0f;
        s.node[0][0] = 0; s.last[0][0] = -1; s.len[0][0] = 0;
        s.hash[0][0] = 0x243F6A8885A308D3ull; s.phash[0][0] = 0;
        if constexpr (kLm) { sl.lmstate[0][0] = la.lm.start; sl.lm[0][0] = 0.0f; }
        s.nb[0] = 1;
        nodes[0] = make_int2(-1, -1);                               // the empty prefix
    }
    if (T > 0) {
        if (tid < K) { s.fval[0][tid] = a.tk_val[in0 * K + tid]; s.fid[0][tid] = a.tk_id[in0 * K + tid]; }
        else if (tid == K) s.flpb[0] = a.lpb[in0];
    }
    __syncthreads();
    for (int t = 0; t < T; ++t) {
        const int cur = t & 1, nxt = cur ^ 1;
        float pv = 0.0f;                                            // next frame's tokens: loaded here, stored after the rank count
        int pi = 0;
        if (t + 1 < T) {
            if (tid < K) { pv = a.tk_val[(in0 + t + 1) * K + tid]; pi = a.tk_id[(in0 + t + 1) * K + tid]; }
            else if (tid == K) pv = a.lpb[in0 + t + 1];
        }
        const int nb = s.nb[cur];
        float npb[kBeamCPT], npnb[kBeamCPT], sc[kBeamCPT], nlm[kBeamCPT];         // (nlm / nls: kLm only)
        int nls[kBeamCPT];
        unsigned long long key[kBeamCPT];
#pragma unroll
        for (int u = 0; u < kBeamCPT; ++u) {
            const int i = ci[u], j = cj[u];
            key[u] = kBeamDead;
            npb[u] = NEG; npnb[u] = NEG; sc[u] = NEG; nlm[u] = 0.0f; nls[u] = 0;
            if (i >= nb) continue;
            const int last = s.last[cur][i], len = s.len[cur][i];
            bool dead = false;
            int tok = 0;
            if (j == 0) {                                           // p stays: blank, the repeat of its last token, and an extension that IS p
                npb[u] = s.tot[cur][i] + s.flpb[cur];
                float rep = NEG, mrg = NEG;
                if (last >= 0) {
                    int ks = -1;
                    for (int k = 0; k < K; ++k) if (s.fid[cur][k] == last) ks = k;
                    if (ks >= 0) {
                        const float v = s.fval[cur][ks];
                        rep = s.pnb[cur][i] + v;
                        const unsigned long long ph = s.phash[cur][i];
                        for (int q = 0; q < nb; ++q)
                            if (s.len[cur][q] == len - 1 && s.hash[cur][q] == ph) mrg = (s.last[cur][q] == last ? s.pb[cur][q] : s.tot[cur][q]) + v;
                    }
                }
                npnb[u] = dlaef(rep, mrg);
                sc[u] = dlaef(npb[u], npnb[u]);
                if constexpr (kLm) { nlm[u] = sl.lm[cur][i]; nls[u] = sl.lmstate[cur][i]; }           // its LM state and score stay with it
            } else {                                                // p + c
                tok = s.fid[cur][j - 1];
                npnb[u] = (tok == last ? s.pb[cur][i] : s.tot[cur][i]) + s.fval[cur][j - 1];
                sc[u] = npnb[u];
                const unsigned long long h2 = beam_hash(s.hash[cur][i], tok);
                for (int q = 0; q < nb; ++q) dead = dead || (s.len[cur][q] == len + 1 && s.hash[cur][q] == h2);
                if constexpr (kLm) {                                // one lookup, only for a live extension that is not merged away
                    if (!dead && sc[u] > NEG) {
                        const float lp = beam_lm_lookup(la.lm, sl.lmstate[cur][i], tok, nls[u]);
                        nlm[u] = __fadd_rn(sl.lm[cur][i], __fadd_rn(__fmul_rn(la.lm.alpha, lp), la.lm.beta));    // three roundings, no fma
                    }
                }
            }
            if (!dead && sc[u] > NEG) {
                float f = sc[u];
                if constexpr (kLm) f = __fadd_rn(sc[u], nlm[u]);
                key[u] = ((unsigned long long)beam_ord_desc(f) << 32) | ((unsigned)i << 25) | (j ? (1u << 24) : 0u) | (unsigned)tok;
            }
            s.key[tid + 256 * u] = key[u];
        }
        __syncthreads();                                            // barrier 1 of 2: every candidate's key is in LDS
        const int n = nb * KP;
        int rk[kBeamCPT], valid = 0;
#pragma unroll
        for (int u = 0; u < kBeamCPT; ++u) rk[u] = 0;
        for (int q = 0; q < n; ++q) {
            const unsigned long long kq = s.key[q];
            valid += kq != kBeamDead;
#pragma unroll
            for (int u = 0; u < kBeamCPT; ++u) rk[u] += kq < key[u];
        }
#pragma unroll
        for (int u = 0; u < kBeamCPT; ++u) {
            const int r = rk[u];
            if (key[u] == kBeamDead || r >= W) continue;
            const int i = ci[u], j = cj[u];
            s.pb[nxt][r] = npb[u]; s.pnb[nxt][r] = npnb[u]; s.tot[nxt][r] = sc[u];
            if constexpr (kLm) { sl.lm[nxt][r] = nlm[u]; sl.lmstate[nxt][r] = nls[u]; }
            if (j == 0) {
                s.node[nxt][r] = s.node[cur][i]; s.last[nxt][r] = s.last[cur][i]; s.len[nxt][r] = s.len[cur][i];
                s.hash[nxt][r] = s.hash[cur][i]; s.phash[nxt][r] = s.phash[cur][i];
            } else {
                const int tok = s.fid[cur][j - 1], nd = 1 + t * W + r;
                nodes[nd] = make_int2(s.node[cur][i], tok);
                s.node[nxt][r] = nd; s.last[nxt][r] = tok; s.len[nxt][r] = s.len[cur][i] + 1;
                s.hash[nxt][r] = beam_hash(s.hash[cur][i], tok); s.phash[nxt][r] = s.hash[cur][i];
            }
        }
        if (tid == 0) s.nb[nxt] = valid < W ? valid : W;
        if (t + 1 < T) {
            if (tid < K) { s.fval[nxt][tid] = pv; s.fid[nxt][tid] = pi; }
            else if (tid == K) s.flpb[nxt] = pv;
        }
        __syncthreads();                                            // barrier 2 of 2: the next beam is complete
    }
    const int fin = T & 1, nb = s.nb[fin];
    if (tid < a.N) {
        const int64_t o = (int64_t)b * a.N + tid;
        const bool have = tid < nb;
        a.hyp_node[o] = have ? s.node[fin][tid] : 0;
        a.hyp_len[o] = have ? s.len[fin][tid] : 0;
        a.hyp_score[o] = have ? s.tot[fin][tid] : NEG;
        if constexpr (kLm) la.hyp_lm[o] = have ? sl.lm[fin][tid] : 0.0f;
    }
}
void launch_ctc_beam_walk(const BeamWalkArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(ctc_beam_walk_kernel<false>, dim3(a.B), dim3(256), 0, s, a);
}
void launch_ctc_beam_lm_walk(const BeamLmWalkArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(ctc_beam_walk_kernel<true>, dim3(a.w.B), dim3(256), 0, s, a);
}

// ---- back-trace + forced alignment --------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ctc_beam_align_kernel(BeamAlignArgs a) {
    extern __shared__ __attribute__((aligned(16))) float ba_sm[];
    const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    int T = a.T;
    int64_t in0 = (int64_t)b * T;
    if (a.rg.T) { in0 = a.rg.T_off[b]; T = a.rg.T[b]; }
    const int64_t h = (int64_t)b * a.N + j, o0 = h * a.pitch;
    const int L = a.hyp_len[h];
    const int2 *nodes = a.nodes + (int64_t)b * a.node_pitch;
    int *tok = reinterpret_cast<int *>(ba_sm);                      // [pitch]   (timestamps only)
    float *al = ba_sm + a.pitch;                                    // [2][2 pitch + 1]
    const int AP = 2 * a.pitch + 1;
    if (tid == 0) {
        int nd = a.hyp_node[h];
        for (int k = L - 1; k >= 0; --k) {
            const int2 e = nodes[nd];
            a.ids[o0 + k] = e.y;
            if (a.timestamps) tok[k] = e.y;
            nd = e.x;
        }
        a.lens[h] = L;
    }
    if (!a.timestamps || L == 0 || L > T) return;                   // (L > T cannot come out of the walk: one frame per token at least)
    __syncthreads();
    const float NEG = -__builtin_huge_valf();
    const int S = 2 * L + 1;
    unsigned char *bp = a.bp + h * a.bp_pitch;
    const float *row0 = a.lp + in0 * a.V;
    for (int s = tid; s < S; s += 256) al[s] = s == 0 ? row0[a.blank] : (s == 1 ? row0[tok[0]] : NEG);
    __syncthreads();
    for (int t = 1; t < T; ++t) {
        const float *src = al + ((t - 1) & 1) * AP;
        float *dst = al + (t & 1) * AP;
        const float *row = a.lp + (in0 + t) * a.V;
        for (int s = tid; s < S; s += 256) {
            float best = src[s];
            int p = 0;
            if (s >= 1 && src[s - 1] > best) { best = src[s - 1]; p = 1; }
            if ((s & 1) && s >= 3 && tok[s >> 1] != tok[(s >> 1) - 1] && src[s - 2] > best) { best = src[s - 2]; p = 2; }
            dst[s] = best + row[(s & 1) ? tok[s >> 1] : a.blank];
            bp[(int64_t)t * S + s] = (unsigned char)p;
        }
        __syncthreads();                                            // one barrier per frame (alpha is double buffered)
    }
    if (tid == 0) {
        const float *fin = al + ((T - 1) & 1) * AP;
        int s = S - 1;
        if (fin[S - 2] > fin[S - 1]) s = S - 2;
        int lastk = -1;
        for (int t = T - 1; t >= 0; --t) {
            if (s & 1) {
                const int k = s >> 1;
                if (k != lastk) { a.end[o0 + k] = t; lastk = k; }
                a.start[o0 + k] = t;
            }
            if (t > 0) s -= bp[(int64_t)t * S + s];
        }
        __threadfence_block();
    }
    __syncthreads();
    for (int k = tid; k < L; k += 256) a.conf[o0 + k] = dexpf(a.lp[(in0 + a.start[o0 + k]) * a.V + tok[k]]);
}
void launch_ctc_beam_align(const BeamAlignArgs &a, hipStream_t s) {
    const size_t lds = a.timestamps ? (size_t)(5 * a.pitch + 2) * sizeof(float) : 0;
    hipLaunchKernelGGL(ctc_beam_align_kernel, dim3(a.N, a.B), dim3(256), lds, s, a);
}

}  // namespace pk
