// parakeet.cpp_amd/csrc/kernels/attention_dev.hpp -- device code and sizing rules shared by the fp32 relative-position attention kernels:
// the 32-row "block" form and its limited-context "band" instantiation (attention.hip: relpos_attention_kernel, BAND = true for the
// band) and the register "strip" form (attention.hip: relpos_attention_strip_kernel).  Every piece below exists once:
// workgroup placement, the operand tile load, the biased Q load, the natural-k MFMA chains, the V chunk stager, the ctx store, and the four
// phases over a score block in LDS (content pass, shifted read-modify-write pass, lane-strided softmax, AV steps).
#pragma once
#include "../pk_devmath.h"
#include "kernels.hpp"

namespace pk {

typedef float f32x4 __attribute__((ext_vector_type(4)));
static constexpr int RB = 32;   // query rows per workgroup of the block / band form (the ragged unit lists are built with 32-row units)

// Phase stamps for tools/ubench/attn_bench.cpp (-DATT_TRACE): shader clock of lane 0 of every wave at the phase boundaries; nw = waves per
// workgroup of the kernel that stamps.  Production: nothing.
#ifdef ATT_TRACE
__device__ long long *att_trace;    // [workgroup][wave][8]
#define ATT_STAMP(nw, i) do { if (att_trace && (threadIdx.x & 63) == 0) att_trace[((long long)blockIdx.x * (nw) + (threadIdx.x >> 6)) * 8 + (i)] = clock64(); } while (0)
#else
#define ATT_STAMP(nw, i) do { } while (0)
#endif

// ---- host: head sizes and the LDS footprint of a score block -----------------------------------------------------------------------------
inline bool att_hd_supported(int hd) { return hd == 32 || hd == 64 || hd == 96 || hd == 128; }
// floats per score-plane row for `cols` key columns: four columns per float4 step, padded so that pitch / 4 is odd (conflict-free row sweeps)
inline int att_score_pitch(int cols) {
    int pits = (cols + 3) / 4;
    pits = (pits + 3) & ~3;
    if (((pits / 4) & 1) == 0) pits += 4;
    return pits;
}
__host__ __device__ inline int att_score_plane(int pits) { return RB * pits + 8; }     // +8: the four planes start 8 banks apart
inline int att_block_vch(int hd) { return hd == 128 ? 32 : 64; }    // V chunk rows of the block form (hd 64 also has a 32-row build)
// LDS bytes of one workgroup: the [32][cols] score block (four k-planes) + one V chunk of vch rows (pitch hd + 16)
inline size_t att_block_lds_bytes(int cols, int hd, int vch) {
    return (size_t)(4 * att_score_plane(att_score_pitch(cols)) + vch * (hd + 16)) * sizeof(float);
}

// launch KERNEL with `lds` bytes of dynamic LDS, raising its per-device limit first where needed (one slot array per kernel instantiation)
template <auto KERNEL, typename... Args>
inline void att_launch_dyn_lds(dim3 grid, dim3 block, size_t lds, hipStream_t s, Args... args) {
    static DynLdsSlots slots;
    ensure_dyn_lds(slots, reinterpret_cast<const void *>(KERNEL), lds);
    hipLaunchKernelGGL(KERNEL, grid, block, lds, s, args...);
}

__device__ __forceinline__ float f4e(const float4 &v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }

// ---- placement -----------------------------------------------------------------------------------------------------------------------------
// Block b runs on XCD b % 8 (observed dispatch rule).  The row blocks of one (utterance, head) share K, V and the P band: they get
// consecutive slots on ONE XCD so the second..last read those rows from that XCD's L2 instead of HBM.  Ragged batch (kernels.hpp: SeqRag):
// XCD x takes head x (+ 8, ...) of EVERY utterance, the 32-row units of one utterance in consecutive slots -- the same L2 sharing -- and T
// becomes this utterance's own length.  ROWS: query rows per workgroup of a uniform launch.
// false: a padding slot of the grid; the whole workgroup returns, before any barrier.
struct AttPlace {
    int h, i0, T;       // head, first query row of the workgroup, frames of this utterance
    int64_t row0;       // first row of this utterance in the (packed) row axis of qkv / ctx
};
template <bool RAG, int ROWS>
__device__ __forceinline__ bool att_place(int H, int T, int n_rb, int n_bh, const SeqRag &rg, AttPlace &p) {
    const int id = blockIdx.x, xcd = id & 7, k = id >> 3;
    if constexpr (RAG) {
        p.h = (k / rg.units.count) * 8 + xcd;
        if (p.h >= H) return false;
        const RagUnit un = rg.units.u[k % rg.units.count];
        p.i0 = un.r0;
        p.T = rg.T[un.b];
        p.row0 = rg.T_off[un.b];
    } else {
        const int rbk = k % n_rb, bh = (k / n_rb) * 8 + xcd;
        if (bh >= n_bh) return false;
        p.h = bh % H;
        p.i0 = rbk * ROWS;
        p.T = T;
        p.row0 = (int64_t)(bh / H) * T;
    }
    return true;
}

// ---- operands ------------------------------------------------------------------------------------------------------------------------------
// one 16-row operand tile straight from global (sigma columns): lane (row l15, quarter kq) takes float4 #kq of every 16-feature block;
// rows outside [0, limit) are zeros
template <int NQ4>
__device__ __forceinline__ void att_load_tile(const float *base, int64_t ld, int row0, int limit, int l15, int kq, float4 (&f)[NQ4]) {
    const int r = row0 + l15;
    const bool ok = r >= 0 && r < limit;
    const float *p = base + (int64_t)(ok ? r : 0) * ld + 4 * kq;
#pragma unroll
    for (int q = 0; q < NQ4; ++q) f[q] = ok ? *reinterpret_cast<const float4 *>(p + 16 * q) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}
// the Q fragments of 16 query rows, (q + bias) as the reference forms them (src/encoder.cpp:141-142); element e of fragment f <-> k = 16f + 4e + kq.
// bias: bias_u / bias_v, this head's row at hoff; biased false (no position table, bias may be null): q alone
template <int NQ4>
__device__ __forceinline__ void att_load_q_biased(const float *qb, int ldq, int row0, int T, const float *bias, int hoff, bool biased, int l15, int kq,
                                                  float4 (&qx)[NQ4]) {
    att_load_tile(qb, ldq, row0, T, l15, kq, qx);
    if (biased) {
        const float *br = bias + hoff + kq;
#pragma unroll
        for (int f = 0; f < NQ4; ++f)
            qx[f] = make_float4(qx[f].x + br[16 * f], qx[f].y + br[16 * f + 4], qx[f].z + br[16 * f + 8], qx[f].w + br[16 * f + 12]);
    }
}
// 16x16 accumulator chains over K = 16 NQ4 from zero (natural k: step 4q+e consumes k = 16q + 4e + kq): one, and two independent ones
template <int NQ4>
__device__ __forceinline__ void att_mma_one(const float4 (&a)[NQ4], const float4 (&b)[NQ4], f32x4 &c) {
    c = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int q = 0; q < NQ4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) c = __builtin_amdgcn_mfma_f32_16x16x4f32(f4e(a[q], e), f4e(b[q], e), c, 0, 0, 0);
}
template <int NQ4>
__device__ __forceinline__ void att_mma_pair(const float4 (&a)[NQ4], const float4 (&b0)[NQ4], const float4 (&b1)[NQ4], f32x4 &c0, f32x4 &c1) {
    c0 = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    c1 = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int q = 0; q < NQ4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(f4e(a[q], e), f4e(b0[q], e), c0, 0, 0, 0);
            c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(f4e(a[q], e), f4e(b1[q], e), c1, 0, 0, 0);
        }
}

// ---- V chunk: cooperative coalesced loads -> registers (issue) -> LDS (commit), NT threads, VCH natural rows of pitch HD + 16 ----------------
template <int HD, int VCH, int NT>
__device__ __forceinline__ void att_v_issue(const float *vb, int ldq, int row0, int limit, float4 (&vf)[VCH * (HD / 4) / NT]) {
    constexpr int KQ = HD / 4;
    static_assert((VCH * KQ) % NT == 0 && VCH % 4 == 0, "V chunk must split evenly over the workgroup's threads");
#pragma unroll
    for (int i = 0; i < VCH * KQ / NT; ++i) {
        const int e = threadIdx.x + NT * i, gr = row0 + e / KQ;
        vf[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (gr < limit) vf[i] = *reinterpret_cast<const float4 *>(vb + (int64_t)gr * ldq + 4 * (e % KQ));
    }
}
template <int HD, int VCH, int NT>
__device__ __forceinline__ void att_v_commit(float *VS, const float4 (&vf)[VCH * (HD / 4) / NT]) {
    constexpr int KQ = HD / 4;
#pragma unroll
    for (int i = 0; i < VCH * KQ / NT; ++i) {
        const int e = threadIdx.x + NT * i;
        lds_store16(VS + (e / KQ) * (HD + 16) + 4 * (e % KQ), vf[i]);
    }
}

// one ctx element in the layout the consumer asked for: 0 fp32, 1 bf16 (out_proj's operand, rounded here, RNE), 2 fp32 in sigma columns
// (GemmArgs::a_sigma)
__device__ __forceinline__ void att_store_ctx(float *ctx, int64_t orow, int col, float v, int ctx_bf16) {
    if (ctx_bf16 == 1) reinterpret_cast<__bf16 *>(ctx)[orow + col] = (__bf16)v;
    else if (ctx_bf16 == 2) ctx[orow + sigma_col(col)] = v;
    else ctx[orow + col] = v;
}

// ---- the score block of the block / band form and its four phases ----------------------------------------------------------------------------
// [RB rows][W columns], "k-planar" over the column index c (element (il, c) at plane c & 3, il * pits + (c >> 2)) because it is the A operand
// of softmax(S) V: one ds_read_b128 feeds four MFMA steps.  Column c is key jlo + c of the workgroup's window (the full form: jlo = 0, W = T).
struct AttScores {
    float *s;
    int plane, pits;
    __device__ __forceinline__ int idx(int il, int c) const { return (c & 3) * plane + il * pits + (c >> 2); }
};
struct AttWave {        // a wave of the 4-wave workgroup: lane = (kq, l15); 16-row tile rt, column-tile parity cp; il_base: C-layout row of register 0
    int lane, l15, kq, wave, rt, cp, il_base;
};
__device__ __forceinline__ AttWave att_wave() {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    return AttWave{lane, lane & 15, lane >> 4, wave, wave & 1, wave >> 1, (wave & 1) * 16 + 4 * (lane >> 4)};   // C layout: column = lane & 15, row = 4*(lane>>4) + r
}

// phase 1: content scores (q+u) K^T -> S; this wave's column tiles are t = cp, cp+2, ... (pairs, one pair ahead).  kb: key row of column 0.
// Columns W .. Wpad4-1 are the zero pad of the AV chain; without a position term (has_pos false) the scale is applied here.
template <int NQ4>
__device__ __forceinline__ void att_content_pass(const AttScores &sc, const AttWave &w, const float *kb, int ldq, int W, const float4 (&qx)[NQ4],
                                                 bool has_pos, float scale) {
    float *S = sc.s;
    const int Wpad4 = (W + 3) & ~3, nct = (W + 15) / 16;
    float4 bA0[NQ4], bA1[NQ4], bB0[NQ4], bB1[NQ4];                  // two operand-tile pairs: one computing, one in flight
    auto load = [&](int t, float4 (&f)[NQ4]) { att_load_tile(kb, ldq, t * 16, W, w.l15, w.kq, f); };
    auto store = [&](int t, const f32x4 &a0, const f32x4 &a1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int il = w.il_base + r;
            const int c0 = t * 16 + w.l15, c1 = c0 + 32;
            if (c0 < Wpad4) S[sc.idx(il, c0)] = c0 < W ? (has_pos ? a0[r] : a0[r] * scale) : 0.0f;
            if (t + 2 < nct && c1 < Wpad4) S[sc.idx(il, c1)] = c1 < W ? (has_pos ? a1[r] : a1[r] * scale) : 0.0f;
        }
    };
    if (w.cp < nct) { load(w.cp, bA0); load(w.cp + 2, bA1); }
    for (int t = w.cp; t < nct; t += 8) {
        f32x4 a0, a1;
        if (t + 4 < nct) { load(t + 4, bB0); load(t + 6, bB1); }
        att_mma_pair(qx, bA0, bA1, a0, a1);
        store(t, a0, a1);
        if (t + 4 < nct) {
            if (t + 8 < nct) { load(t + 8, bA0); load(t + 10, bA1); }
            att_mma_pair(qx, bB0, bB1, a0, a1);
            store(t + 4, a0, a1);
        }
    }
}

// phase 2: position scores (q+v) P^T, shifted, combined and scaled.  The wave's own tile grid over the table rows starts at wpmin, tiles
// t = cp, cp+2, ... of npt; table row p of query row i lands in column p - cshift + i.  pb: row 0 of the table (NP rows, pitch d).
// The first tiles are requested ahead of the barrier that completes the content scores (in flight across it).
template <int NQ4>
__device__ __forceinline__ void att_shift_pass(const AttScores &sc, const AttWave &w, const float *pb, int d, int NP, int wpmin, int npt, int cshift,
                                               int i0, int T, int W, const float4 (&qx)[NQ4], float scale) {
    float *S = sc.s;
    float4 bA0[NQ4], bA1[NQ4], bB0[NQ4], bB1[NQ4];
    auto load = [&](int t, float4 (&f)[NQ4]) { att_load_tile(pb, d, wpmin + t * 16, NP, w.l15, w.kq, f); };
    if (w.cp < npt) { load(w.cp, bA0); load(w.cp + 2, bA1); }
    __syncthreads();                                              // content scores complete
    ATT_STAMP(4, 3);                                                // (q+v), first P tiles requested, barrier
    auto rmw = [&](int t, const f32x4 &a0, const f32x4 &a1) {
        // the eight score elements are READ together, then combined, then stored (distinct addresses: four rows x two column tiles); one by one
        // every read would wait behind the previous element's store (see the softmax sweep below)
        int ad[8];
        bool ok[8];
        float v[8];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int il = w.il_base + r, i = i0 + il;
            const int pa = wpmin + t * 16 + w.l15, ca = pa - cshift + i;
            const int pc = pa + 32, cc = ca + 32;
            ok[r] = i < T && pa < NP && ca >= 0 && ca < W;
            ok[4 + r] = t + 2 < npt && i < T && pc < NP && cc >= 0 && cc < W;
            ad[r] = ok[r] ? sc.idx(il, ca) : 0;
            ad[4 + r] = ok[4 + r] ? sc.idx(il, cc) : 0;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = S[ad[q]];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (ok[r]) S[ad[r]] = (v[r] + a0[r]) * scale;                   // (content + pos) * scale, src/encoder.cpp:157-160
            if (ok[4 + r]) S[ad[4 + r]] = (v[4 + r] + a1[r]) * scale;
        }
    };
    for (int t = w.cp; t < npt; t += 8) {
        f32x4 a0, a1;
        if (t + 4 < npt) { load(t + 4, bB0); load(t + 6, bB1); }
        att_mma_pair(qx, bA0, bA1, a0, a1);
        rmw(t, a0, a1);
        if (t + 4 < npt) {
            if (t + 8 < npt) { load(t + 8, bA0); load(t + 10, bA1); }
            att_mma_pair(qx, bB0, bB1, a0, a1);
            rmw(t + 4, a0, a1);
        }
    }
}

// Which columns of a row take part in its softmax.  Full: all of them (every test below folds away).  Band: row k of the wave keeps
// [clo[k], chi[k]]; columns outside take no part in the maximum and become exact zeros; an empty band (rows past T, never stored) divides by 1.
struct AttRowsFull {
    __device__ __forceinline__ bool in(int, int) const { return true; }
    __device__ __forceinline__ bool empty(int) const { return false; }
};
struct AttRowsBand {
    int clo[RB / 4], chi[RB / 4];
    __device__ __forceinline__ bool in(int k, int c) const { return c >= clo[k] && c <= chi[k]; }
    __device__ __forceinline__ bool empty(int k) const { return chi[k] < clo[k]; }      // (an in-band row holds its maximum: sum >= 1)
};

// phase 3: softmax, one wavefront per row, the canonical max / sum64 butterflies.  Each wave owns rows wave, wave+4, ...: all NSR of them go
// through the three sweeps TOGETHER, so the 2 x 6 dependent cross-lane butterfly stages and the exp / divide chains of different rows overlap
// instead of queueing up.  (Rows past T in the last block hold zeros: they are swept too and never stored.)
template <typename ROWS>
__device__ __forceinline__ void att_softmax(const AttScores &sc, const AttWave &w, int W, int ctx_bf16, const ROWS &rows) {
    float *S = sc.s;
    const int lane = w.lane, wave = w.wave;
    constexpr int NSR = RB / 4;
    float mx[NSR], sm[NSR];
#pragma unroll
    for (int k = 0; k < NSR; ++k) mx[k] = -__builtin_huge_valf();
    for (int c = lane; c < W; c += 64)
#pragma unroll
        for (int k = 0; k < NSR; ++k)
            if (rows.in(k, c)) mx[k] = fmaxf(mx[k], S[sc.idx(wave + 4 * k, c)]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int k = 0; k < NSR; ++k) mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], off, 64));
#pragma unroll
    for (int k = 0; k < NSR; ++k) sm[k] = 0.0f;
    // The NSR rows' values are READ first, then transformed, then stored: written element by element (read, exp, store, next row) the compiler
    // has to keep every read behind the previous row's store -- both are LDS floats -- and the eight exp chains ran one after the other, each
    // behind its own LDS round trip (round 4, from the ISA: profiles/r04_attn_phases.txt).  Same values, same per-row summation order.
    for (int c = lane; c < W; c += 64) {
        float e[NSR];
#pragma unroll
        for (int k = 0; k < NSR; ++k) e[k] = S[sc.idx(wave + 4 * k, c)] - mx[k];          // S <= row maximum
        if (ctx_bf16 == 1) {    // bf16 mode (tolerance-class, see GemmArgs::fast_act): hardware exp2 instead of the fixed polynomial
#pragma unroll
            for (int k = 0; k < NSR; ++k) e[k] = __builtin_amdgcn_exp2f(e[k] * 1.44269502162933349609375f);
        } else {
#pragma unroll
            for (int k = 0; k < NSR; ++k) e[k] = dexpf_nonpos(e[k]);
        }
#pragma unroll
        for (int k = 0; k < NSR; ++k) {
            if (!rows.in(k, c)) e[k] = 0.0f;                        // (whatever the exponential made of an out-of-band score)
            S[sc.idx(wave + 4 * k, c)] = e[k];
            sm[k] = sm[k] + e[k];
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)                      // the canonical sum64 butterfly, NSR rows side by side
#pragma unroll
        for (int k = 0; k < NSR; ++k) sm[k] = sm[k] + __shfl_xor(sm[k], off, 64);
#pragma unroll
    for (int k = 0; k < NSR; ++k) sm[k] = rows.empty(k) ? 1.0f : sm[k];
    if (ctx_bf16 == 1) {                                         // bf16 mode: one hardware reciprocal per row, a multiplication per element
#pragma unroll
        for (int k = 0; k < NSR; ++k) sm[k] = __builtin_amdgcn_rcpf(sm[k]);
        for (int c = lane; c < W; c += 64) {
            float e[NSR];
#pragma unroll
            for (int k = 0; k < NSR; ++k) e[k] = S[sc.idx(wave + 4 * k, c)] * sm[k];
#pragma unroll
            for (int k = 0; k < NSR; ++k) S[sc.idx(wave + 4 * k, c)] = e[k];
        }
    } else {
        for (int c = lane; c < W; c += 64) {
            float e[NSR];
#pragma unroll
            for (int k = 0; k < NSR; ++k) e[k] = S[sc.idx(wave + 4 * k, c)];
#pragma unroll
            for (int k = 0; k < NSR; ++k) e[k] = e[k] / sm[k];
#pragma unroll
            for (int k = 0; k < NSR; ++k) S[sc.idx(wave + 4 * k, c)] = e[k];
        }
    }
}

// phase 4, the steps of one V chunk: acc[m] += A[:, k] V[k][tile m] for the chunk's s_end k-quads (zero rows pad the last one), natural key
// order.  sa: this lane's row of the k-planar probabilities at the chunk's first column (k = 4s + kq at float s); vrow: V[kq][this lane's column
// of tile 0] in the staged chunk; mstride: floats between the lane's column tiles (16: every tile; 32: every second one).  GLOBAL_A: sa is global memory.
template <int NDV, int VPIT, bool GLOBAL_A = false>
__device__ __forceinline__ void att_av_steps(const float *sa, const float *vrow, int s_end, int mstride, f32x4 (&acc)[NDV]) {
    for (int s4 = 0; s4 < s_end; s4 += 4) {
        float4 a = *reinterpret_cast<const float4 *>(sa + s4);
        // global planes (the SG builds): keep the 16-byte load whole.  The steps below use its elements conditionally, and split into
        // per-element loads it costs two serial round trips per four steps (6.8 % of the hd 32 kernel at T = 1400).  LDS reads stay as they are.
        if constexpr (GLOBAL_A) asm volatile("" : "+v"(a.x), "+v"(a.y), "+v"(a.z), "+v"(a.w));
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (s4 + e < s_end) {
#pragma unroll
                for (int m = 0; m < NDV; ++m)
                    acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4e(a, e), vrow[(s4 + e) * 4 * VPIT + m * mstride], acc[m], 0, 0, 0);
            }
        }
    }
}

}  // namespace pk
