// parakeet.cpp_amd/csrc/kernels/attention.hip -- relative-position multi-head attention core
// (reference ConformerAttention::rel_position_attention, src/encoder.cpp:135-171, with rel_shift
// :85-109 applied in closed form):
//     S[i][j] = ( (q_i + u_h) . k_j  +  (q_i + v_h) . P_h[j - i + T - 1] ) / sqrt(hd)
//     ctx_i   = softmax_j(S[i][:]) V
// The "block" form: one workgroup per (utterance, head, block of 32 query rows), 4 wavefronts.  All three contractions run on the
// fp32 MFMA v_mfma_f32_16x16x4_f32 (natural-k fma chains = the oracle's order); 16x16 tiles give every wave the same
// number of tiles in each phase.
//   * Q, K and the projected position table P arrive in the "sigma" column layout (the producing GEMMs write it: inside
//     every block of 16 features the 4x4 index matrix is transposed), so the float4 a lane loads holds exactly its
//     k = 4s+kq operands of four consecutive MFMA steps: the A / B fragments of QK^T and QP^T come STRAIGHT from L2 with
//     16-byte loads -- no LDS staging, no barriers, each wave streams its own tiles with the next pair's loads in flight.
//   * The [32][T] score block lives in LDS only.  The [B][H][T][2T-1] position-score tensor the reference materialises is
//     never formed: each 16x16 position tile is added straight into its shifted column j = p - (T-1) + i.  The block is
//     "k-planar" over the key index (element (i, j) at plane j&3, i*pitch + (j>>2)) because it is the A operand of
//     softmax(S) V: one ds_read_b128 feeds four MFMA steps.
//   * V streams through LDS in chunks of VCH rows (coalesced 16-byte loads, natural rows, pitch = 16 mod 32 banks).
// Softmax is one wavefront per row with the canonical max / sum64 butterflies.  3 barriers per workgroup (+2 per extra V chunk).
// (Round 2 also tried V as a straight-from-L2 B operand -- one dword per lane per MFMA step, a register block of 8 steps ahead: bit-equal,
// no V copy in LDS and no chunk barriers, but the gathers are slower than the LDS copy: AV phase 10 k -> 23 k clocks per wave at T = 126,
// 52 k -> 112 k at T = 376 / hd = 128.  Not kept.)
//
// The limited-context ("band") form is the SAME kernel, instantiated with BAND = true (launch_relpos_local_attention below):
//     S[i][j] = ( (q_i + u_h) . k_j  +  (q_i + v_h) . Pl_h[j - i + left] ) / sqrt(hd)     for j in [max(0, i - left), min(T - 1, i + right)]
//     ctx_i   = softmax_j(S[i][:]) V                                                        (keys outside the band: weight exactly 0)
// Pl is the local position table [left + right + 1][d]: row r is the projected sinusoid of position i - j = left - r (engine.cpp:
// ensure_local_pos_table), the same float formula as the full table, so a row is bit for bit the full table's row of that position.
// Shared, literally (attention_dev.hpp): placement, operand loads, the content pass, the shifted pass, the softmax sweeps, the AV steps, the
// ctx store -- all over the columns c of a key WINDOW [jlo, jhi], column c = key jlo + c.  What differs, under `if constexpr (BAND)`:
//   * the window: the full form's is every key (jlo = 0, W = T, closed-form table rows wpmin / wpmax); the band form's is
//     [i0 - left, i0 + 31 + right] clamped to the utterance, at most left + right + 32 columns whatever T is, the table rows clamped to Pl;
//   * the table row the window starts at: the full form reads its table from pos_row0 (a ragged unit: rg.pos_T - T), the band form from row 0;
//   * the softmax policy: every column (AttRowsFull) or each row's own band [clo, chi] (AttRowsBand; outside: exact zeros);
//   * the band form has neither the global-scratch score planes (SG) nor the no-position mode (pos == nullptr).
// So when the band covers the utterance (left, right >= T - 1) every score, every softmax sum and every ctx chain is the full form's, bit
// for bit (tests/test_gpu_local_attention.py).
#include "attention_dev.hpp"

namespace pk {

#ifndef ATT_OCC
#define ATT_OCC 4                 // workgroups per CU the hd <= 64 kernel is compiled for (register budget 168 / 128 VGPRs for 3 / 4)
#endif

// SG (long sequences, > ~85 s of audio): the score block of a workgroup lives in a global scratch area instead of LDS -- the same
// code, indexing and barriers (a workgroup's own global writes are visible to it after __syncthreads()), so the same bits; slower,
// but the length is then bounded by HBM, not by the 160 KB of LDS.
// RAG: the ragged-batch form (per-unit utterance extents, kernels.hpp: SeqRag) is its own instantiation -- the uniform kernel sits exactly at
// its 128-VGPR budget (four workgroups per CU) and must not carry a single extra live value (round 4: the shared form spilled more dwords per
// lane and lost 2.5 %; today the hd 64 LDS builds at four workgroups per CU spill nothing uniform or in the band form and 4 dwords ragged; every
// count: profiles/attention_phases_resources.md).
// OCC: workgroups per CU the instantiation is register-budgeted for (128 / 168 / 256 VGPRs for 4 / 3 / 2).  The launcher picks the largest the
// LDS footprint of the sequence length allows anyway: a 30 s utterance (T = 376: 71 KB of score planes + V chunk, two workgroups per CU)
// gains nothing from the spills of the 128-VGPR build.
// BAND: the limited-context form (left / right; s_scratch and pos_row0 unused).  The full form ignores left / right.
// CAUSAL (neural_lm.cpp: the Transformer LM's attention): the band form without a position term and with left = i, right = 0 for query row i --
// the window of a block is keys [0, i0 + 31], so key tiles wholly above the diagonal are neither loaded nor multiplied, and inside the diagonal tile
// AttRowsBand keeps a row's columns j > i out of its maximum and turns them into exact zeros.  pos / bias_u / bias_v / left / right are unused.
template <int HD, int VCH, bool SG = false, bool RAG = false, int OCC = (HD <= 64 ? ATT_OCC : 2), bool BAND = false, bool CAUSAL = false>
__global__ __launch_bounds__(256, OCC) void relpos_attention_kernel(const float *__restrict__ qkv, int ldq, int d, int T,
                                                               const float *__restrict__ pos /*[2T-1][d] (band: [left+right+1][d]), sigma columns*/,
                                                               const float *__restrict__ bias_u, const float *__restrict__ bias_v,
                                                               float scale, float *__restrict__ ctx, int PITS, int n_rb, int n_bh,
                                                               float *__restrict__ s_scratch, int ctx_bf16, int pos_row0, SeqRag rg, int left, int right) {
    static_assert(!(BAND && SG), "the band form keeps its score block in LDS");
    static_assert(!CAUSAL || BAND, "the causal form is an instantiation of the band form");
    __builtin_amdgcn_s_setprio(3);        // ahead of the overlapped decode-loop waves in the SIMD's arbitration (gemm_pipe.hpp)
    constexpr int NQ4 = HD / 16;          // float4 fragments per lane for K = HD (one per block of 16 features)
    constexpr int VPIT = HD + 16;         // V rows, natural layout (pitch = 16 mod 32 banks)
    constexpr int NDV = HD / 32;          // 16-wide ctx column tiles per wave (HD/16 tiles over 2 column parities)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int SPLANE = att_score_plane(PITS);
    const AttScores sc{SG ? s_scratch + (size_t)blockIdx.x * 4 * SPLANE : smem, SPLANE, PITS};     // [4][SPLANE] score planes
    float *VS = SG ? smem : smem + 4 * SPLANE;                                                       // [VCH][VPIT] V chunk
    const int H = d / HD;
    AttPlace pl;
    if (!att_place<RAG, RB>(H, T, n_rb, n_bh, rg, pl)) return;
    const int h = pl.h, i0 = pl.i0;
    const int64_t row0 = pl.row0;
    T = pl.T;
    if constexpr (RAG && !BAND) pos_row0 = rg.pos_T - T;            // this utterance's window of the table built for rg.pos_T frames
    const int rows = (T - i0) < RB ? (T - i0) : RB;
    const AttWave w = att_wave();
    // the key window [jlo, jhi] of this block, W columns; NP rows of position table
    int jlo = 0, jhi = T - 1;
    if constexpr (CAUSAL) { left = i0 + RB; right = 0; }            // every key up to the row itself: jlo = 0, jhi = the block's last row
    if constexpr (BAND) {
        jlo = i0 - left > 0 ? i0 - left : 0;
        jhi = i0 + RB - 1 + right < T - 1 ? i0 + RB - 1 + right : T - 1;
    }
    const int W = BAND ? jhi - jlo + 1 : T;
    const int NP = BAND ? left + right + 1 : 2 * T - 1;
    const bool has_pos = !CAUSAL && (BAND || pos != nullptr);
    const float *qb = qkv + row0 * ldq + h * HD;                    // q rows of this (b,h) (sigma columns)
    const float *kb = qb + d + (int64_t)jlo * ldq, *vb = qb + 2 * d + (int64_t)jlo * ldq;   // k (sigma columns), v (natural): row c = key jlo + c
    const float *pb = CAUSAL ? nullptr : pos + (BAND ? (int64_t)0 : (int64_t)pos_row0 * d) + h * HD;           // row p of THIS length's table (engine.cpp: ensure_pos_tables)

    // ---- phase 0: the Q fragments of this wave's 16 rows.  Only ONE biased copy is live at a time -- (q+u) for the content scores, then
    //      q is fetched again (L2) and (q+v) formed for the position scores -- and the first V chunk is requested after the score phases:
    //      the register budget of four workgroups per CU (128 VGPRs) has no room for both copies plus the V prefetch beside the four
    //      operand tiles of the score loops (round 2: 168 -> 134 VGPRs, 86.9 -> 82.3 us per layer at T = 126).
    float4 qx[NQ4];                                                 // (q+u), later (q+v)
    ATT_STAMP(4, 0);
    att_load_q_biased(qb, ldq, i0 + w.rt * 16, T, bias_u, h * HD, has_pos, w.l15, w.kq, qx);
    ATT_STAMP(4, 1);                                                // Q load + bias
    att_content_pass(sc, w, kb, ldq, W, qx, has_pos, scale);
    ATT_STAMP(4, 2);                                                // QK^T -> S
    if (has_pos) att_load_q_biased(qb, ldq, i0 + w.rt * 16, T, bias_v, h * HD, true, w.l15, w.kq, qx);
    // ---- phase 2: this wave's 16 query rows w_lo .. w_hi need the table rows p = j - i + (T - 1 | left) of their in-window keys: [wpmin, wpmax]
    const int w_lo = i0 + w.rt * 16, w_hi = (w_lo + 15) < (T - 1) ? (w_lo + 15) : (T - 1);
    int wpmin = T - 1 - w_hi, wpmax = 2 * T - 2 - w_lo;
    if constexpr (BAND) {
        wpmin = jlo - w_hi + left > 0 ? jlo - w_hi + left : 0;
        wpmax = jhi - w_lo + left < NP - 1 ? jhi - w_lo + left : NP - 1;
    }
    const int npt = (has_pos && w_lo < T) ? (wpmax - wpmin) / 16 + 1 : 0;
    // (contains the barrier that completes the content scores, and stamp 3: every thread calls it, also with npt == 0 / without a table)
    att_shift_pass(sc, w, pb, d, NP, wpmin, npt, BAND ? left + jlo : T - 1, i0, T, W, qx, scale);
    ATT_STAMP(4, 4);                                                // QP^T shifted rmw
    float4 vf[VCH * (HD / 4) / 256];
    att_v_issue<HD, VCH, 256>(vb, ldq, 0, W, vf);                   // first V chunk: in flight across the softmax
    __syncthreads();
    ATT_STAMP(4, 5);                                                // barrier
    if constexpr (BAND) {
        AttRowsBand band;
#pragma unroll
        for (int k = 0; k < RB / 4; ++k) {
            const int i = i0 + w.wave + 4 * k;
            band.clo[k] = (i - left > jlo ? i - left : jlo) - jlo;
            band.chi[k] = i < T ? (i + right < jhi ? i + right : jhi) - jlo : -1;     // rows past T: an empty band (never stored)
        }
        att_softmax(sc, w, W, ctx_bf16, band);
    } else {
        att_softmax(sc, w, W, ctx_bf16, AttRowsFull{});
    }
    ATT_STAMP(4, 6);                                                // softmax
    att_v_commit<HD, VCH, 256>(VS, vf);
    lds_store_fence();
    __syncthreads();
    // ---- phase 4: ctx = softmax(S) V  (k = window column, natural order; NDV independent 16-column tiles per wave) ---------------
    f32x4 acc[NDV];
#pragma unroll
    for (int m = 0; m < NDV; ++m) acc[m] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const float *sa = sc.s + w.kq * SPLANE + (w.rt * 16 + w.l15) * PITS;     // A: row il = rt*16 + l15, k = 4s + kq at float s
    const float *vrow = VS + w.kq * VPIT + w.cp * 16 + w.l15;                // B: V[4s + kq - c0r][dv tile (cp + 2m)]
    for (int c0r = 0; c0r < W; c0r += VCH) {
        const bool more = c0r + VCH < W;
        if (more) att_v_issue<HD, VCH, 256>(vb, ldq, c0r + VCH, W, vf);
        const int s_end = ((W - c0r < VCH ? W - c0r : VCH) + 3) / 4;            // k-steps in this chunk (zero rows pad the last one)
        att_av_steps<NDV, VPIT, SG>(sa + c0r / 4, vrow, s_end, 32, acc);
        if (more) {
            __syncthreads();
            att_v_commit<HD, VCH, 256>(VS, vf);
            lds_store_fence();
            __syncthreads();
        }
    }
#pragma unroll
    for (int m = 0; m < NDV; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int il = w.il_base + r;
            if (il < rows) att_store_ctx(ctx, (row0 + i0 + il) * d, h * HD + (w.cp + 2 * m) * 16 + w.l15, acc[m][r], ctx_bf16);
        }
    ATT_STAMP(4, 7);                                                // V commit, barrier, AV, store
}

// ---- the "strip" form: T <= 128, the scores never leave the registers until they are probabilities --------------------------------------------
// The kernel above touches every score in LDS nine times (content store, the shifted read-modify-write, three softmax sweeps, the AV read) and
// needs two workgroup barriers only because two waves share a row strip.  Here ONE wave owns 16 query rows x all (<= 128) key columns:
//   * the eight 16x16 content tiles are eight accumulator quads, strip[t] (32 VGPRs), each its own natural-k chain from zero: the same bits;
//   * rel_shift is a fixed skew inside a tile.  The wave's position tile grid starts at wpmin = T - 1 - (i_s + 15), so element (row m, column c) of
//     content tile t is element (row m, column (c - m - 1) & 15) of position tile t when c <= m and of tile t + 1 otherwise: the same register r of
//     the same 16-lane group (C layout: row = 4 kq + r, column = lane & 15).  The SOURCE lane picks the tile (column s serves tile t when
//     s >= 15 - m), one ds_bpermute_b32 per register rotates the row group by m + 1;
//   * softmax in registers, in the summation tree of the kernel above: virtual lane v = j & 63 holds e[v] + e[v + 64] = strip[q] + strip[q + 4]
//     (q = v >> 4; absent columns +0.0), the xor-32 / xor-16 stages are the register adds [q] + [q ^ 2], [q] + [q ^ 1], xor 8 .. 1 run across the
//     16 lanes of the group; the maximum is order-independent; IEEE divide per element;
//   * the probabilities go ONCE into a wave-private k-planar LDS region (PW columns at a time) and come back as the A operand of the AV chains
//     (one ds_read_b128 per four k-steps): the wave's own LDS traffic is in order, no barrier.  V is staged per workgroup as above.
// The only workgroup barriers left are those of the V chunks.  NW waves = 16 NW query rows per workgroup; the ragged form keeps the engine's
// 32-row units (NW = 2).  Placement, operand loads, the single chain, the V stager, the AV steps and the ctx store are attention_dev.hpp's.
static constexpr int STRIP_T = 128;   // longest sequence of the strip form

template <int HD, int VCH, int NW, int PW, bool RAG, int OCC>
__global__ __launch_bounds__(64 * NW, OCC) void relpos_attention_strip_kernel(const float *__restrict__ qkv, int ldq, int d, int T,
                                                                            const float *__restrict__ pos /*[2T-1][d], sigma columns*/,
                                                                            const float *__restrict__ bias_u, const float *__restrict__ bias_v,
                                                                            float scale, float *__restrict__ ctx, int n_rb, int n_bh, int ctx_bf16,
                                                                            int pos_row0, SeqRag rg) {
    __builtin_amdgcn_s_setprio(3);
    constexpr int NT = 64 * NW;
    constexpr int NQ4 = HD / 16, VPIT = HD + 16, NDV = HD / 16;
    constexpr int NCT = STRIP_T / 16;                               // key tiles of a strip
    constexpr int PPIT = PW / 4 + 4, PPLANE = 16 * PPIT + 4;        // probabilities: [4 planes][16 rows][PW / 4]; rows 16, planes 4 banks apart
    static_assert(VCH % 16 == 0 && PW % VCH == 0 && STRIP_T % PW == 0, "V chunks tile a probability piece, pieces tile the strip");
    static_assert(!RAG || NW == 2, "the units of a ragged batch are 32-row blocks");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int H = d / HD;
    AttPlace pl;
    if (!att_place<RAG, 16 * NW>(H, T, n_rb, n_bh, rg, pl)) return;
    const int h = pl.h, i0 = pl.i0;
    const int64_t row0 = pl.row0;
    T = pl.T;
    if constexpr (RAG) pos_row0 = rg.pos_T - T;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, kq = lane >> 4;
    const int i_s = i0 + wave * 16;                                 // first query row of this wave's strip
    const bool active = i_s < T;                                    // a strip wholly past T only helps to stage V
    const int P = 2 * T - 1;
    const int nct = (T + 15) / 16;
    const float *qb = qkv + row0 * ldq + h * HD;
    const float *kb = qb + d, *vb = qb + 2 * d;
    const float *pb = pos + (int64_t)pos_row0 * d + h * HD;
    float *VS = smem;                                               // [VCH][VPIT] V chunk
    float *PS = smem + VCH * VPIT + wave * 4 * PPLANE;              // this wave's probabilities

    float4 vf[VCH * (HD / 4) / NT];
    float4 qx[NQ4];
    ATT_STAMP(NW, 0);
    f32x4 st[NCT];                                                  // the strip: tile t, register r <-> row 4 kq + r, column 16 t + l15
#pragma unroll
    for (int t = 0; t < NCT; ++t) st[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (active) {
        float4 bA[NQ4], bB[NQ4];                                    // one operand tile computing, one in flight
        att_load_q_biased(qb, ldq, i_s, T, bias_u, h * HD, pos != nullptr, l15, kq, qx);
        ATT_STAMP(NW, 1);                                           // Q load + bias
        // ---- content scores (q+u) K^T ----
        att_load_tile(kb, ldq, 0, T, l15, kq, bA);
#pragma unroll
        for (int t = 0; t < NCT; ++t) {
            // (all NCT tiles, straight-line: a tile past T loads nothing and multiplies zeros.  Branching on nct costs registers across the
            //  blocks -- spills at the 128 VGPRs of four workgroups per CU)
            if (t + 1 < NCT) att_load_tile(kb, ldq, (t + 1) * 16, T, l15, kq, (t & 1) ? bA : bB);
            att_mma_one(qx, (t & 1) ? bB : bA, st[t]);
            __builtin_amdgcn_sched_barrier(0);                       // one tile ahead, no further
        }
        ATT_STAMP(NW, 2);                                           // QK^T
        // ---- position scores (q+v) P^T, skewed into place, combined, scaled; columns >= T zero (the pad of the AV chain, +0.0 in the row sum) ----
        if (pos) {
            att_load_q_biased(qb, ldq, i_s, T, bias_v, h * HD, true, l15, kq, qx);
            const int wpmin = T - 1 - (i_s + 15);                    // may be negative: rows outside [0, P) load as zeros and are never selected
            f32x4 pprev = f32x4{0.0f, 0.0f, 0.0f, 0.0f}, pcur;
            att_load_tile(pb, d, wpmin, P, l15, kq, bA);
#pragma unroll
            for (int u = 0; u <= NCT; ++u) {
                if (u + 1 <= NCT) att_load_tile(pb, d, wpmin + (u + 1) * 16, P, l15, kq, (u & 1) ? bA : bB);
                att_mma_one(qx, (u & 1) ? bB : bA, pcur);
                if (u >= 1) {
                    const int t = u - 1, j = t * 16 + l15;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int m = 4 * kq + r;
                        const float x = l15 >= 15 - m ? pprev[r] : pcur[r];
                        const int sl = ((lane & 48) | ((l15 - m - 1) & 15)) << 2;              // source lane: same 16-lane group, column (c - m - 1) & 15
                        const float a = __int_as_float(__builtin_amdgcn_ds_bpermute(sl, __float_as_int(x)));
                        st[t][r] = j < T ? (st[t][r] + a) * scale : 0.0f;                      // (content + pos) * scale, src/encoder.cpp:157-160
                    }
                }
                pprev = pcur;
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
#pragma unroll
            for (int t = 0; t < NCT; ++t) {
                const int j = t * 16 + l15;
#pragma unroll
                for (int r = 0; r < 4; ++r) st[t][r] = j < T ? st[t][r] * scale : 0.0f;
            }
        }
        ATT_STAMP(NW, 3);                                           // QP^T, skew, combine
    } else {
        ATT_STAMP(NW, 1); ATT_STAMP(NW, 2); ATT_STAMP(NW, 3);
    }
    att_v_issue<HD, VCH, NT>(vb, ldq, 0, T, vf);                    // first V chunk: in flight across the softmax (the score passes have no registers to spare)
    if (active) {
        // ---- softmax in registers (rows past T hold finite values and are never stored) ----
        float mx[4], sm[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            mx[r] = -__builtin_huge_valf();
#pragma unroll
            for (int t = 0; t < NCT; ++t)
                if (t * 16 + l15 < T) mx[r] = fmaxf(mx[r], st[t][r]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) mx[r] = fmaxf(mx[r], wave_xor<8>(mx[r]));
#pragma unroll
        for (int r = 0; r < 4; ++r) mx[r] = fmaxf(mx[r], wave_xor<4>(mx[r]));
#pragma unroll
        for (int r = 0; r < 4; ++r) mx[r] = fmaxf(mx[r], wave_xor<2>(mx[r]));
#pragma unroll
        for (int r = 0; r < 4; ++r) mx[r] = fmaxf(mx[r], wave_xor<1>(mx[r]));
#pragma unroll
        for (int t = 0; t < NCT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float x = st[t][r] - mx[r];
                const float e = ctx_bf16 == 1 ? __builtin_amdgcn_exp2f(x * 1.44269502162933349609375f) : dexpf_nonpos(x);
                st[t][r] = t * 16 + l15 < T ? e : 0.0f;
            }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float s0 = st[0][r] + st[4][r], s1 = st[1][r] + st[5][r], s2 = st[2][r] + st[6][r], s3 = st[3][r] + st[7][r];   // j = v, then v + 64
            const float t0 = s0 + s2, t1 = s1 + s3;                  // xor 32
            sm[r] = t0 + t1;                                         // xor 16
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) sm[r] = sm[r] + wave_xor<8>(sm[r]);
#pragma unroll
        for (int r = 0; r < 4; ++r) sm[r] = sm[r] + wave_xor<4>(sm[r]);
#pragma unroll
        for (int r = 0; r < 4; ++r) sm[r] = sm[r] + wave_xor<2>(sm[r]);
#pragma unroll
        for (int r = 0; r < 4; ++r) sm[r] = sm[r] + wave_xor<1>(sm[r]);
        if (ctx_bf16 == 1) {                                         // bf16 mode: one hardware reciprocal per row, a multiplication per element
#pragma unroll
            for (int r = 0; r < 4; ++r) sm[r] = __builtin_amdgcn_rcpf(sm[r]);
#pragma unroll
            for (int t = 0; t < NCT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) st[t][r] = st[t][r] * sm[r];
        } else {
#pragma unroll
            for (int t = 0; t < NCT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) st[t][r] = st[t][r] / sm[r];
        }
    }
    ATT_STAMP(NW, 4);                                               // softmax
    att_v_commit<HD, VCH, NT>(VS, vf);
    lds_store_fence();
    __syncthreads();
    ATT_STAMP(NW, 5);                                               // V commit, barrier
    // ---- ctx = softmax(S) V: NDV 16-column tiles per wave, natural key order ----
    f32x4 acc[NDV];
#pragma unroll
    for (int m = 0; m < NDV; ++m) acc[m] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const float *vrow = VS + kq * VPIT + l15;                       // B: V[4s + kq - c0r][16 m + l15]
#pragma unroll
    for (int c = 0; c < STRIP_T / VCH; ++c) {
        const int c0r = c * VCH;
        if (c0r < T) {
            const bool more = c0r + VCH < T;
            if (more) att_v_issue<HD, VCH, NT>(vb, ldq, c0r + VCH, T, vf);
            if (active) {
                if (c0r % PW == 0) {                                 // the next PW columns of probabilities -> this wave's k-planar region
#pragma unroll
                    for (int tt = 0; tt < PW / 16; ++tt) {
                        const int t = c0r / 16 + tt;
                        if (t < nct) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) PS[(l15 & 3) * PPLANE + (4 * kq + r) * PPIT + 4 * tt + (l15 >> 2)] = st[t][r];
                        }
                    }
                    lds_store_fence();                               // wave-private: the wave's own stores, then its own reads
                }
                const int s_end = ((T - c0r < VCH ? T - c0r : VCH) + 3) / 4;
                att_av_steps<NDV, VPIT>(PS + kq * PPLANE + l15 * PPIT + (c0r % PW) / 4, vrow, s_end, 16, acc);    // A: row l15, k = 4s + kq at float s
            }
            if (more) {
                __syncthreads();
                att_v_commit<HD, VCH, NT>(VS, vf);
                lds_store_fence();
                __syncthreads();
            }
        }
    }
    ATT_STAMP(NW, 6);                                               // P write, AV
#pragma unroll
    for (int m = 0; m < NDV; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = i_s + 4 * kq + r;
            if (i < T) att_store_ctx(ctx, (row0 + i) * d, h * HD + m * 16 + l15, acc[m][r], ctx_bf16);
        }
    ATT_STAMP(NW, 7);                                               // store
}

// grid of a launch: 8 XCD lanes x ceil(n_bh / 8) x n_rb row blocks; ragged: 8 XCD lanes x ceil(n_heads / 8) x the batch's 32-row units
static dim3 att_grid(int n_bh, int n_rb, int n_heads, const SeqRag &rag) {
    if (rag.units.u) return dim3((unsigned)(((n_heads + 7) / 8) * 8 * (int64_t)rag.units.count));
    return dim3(((n_bh + 7) / 8) * 8 * n_rb);
}

template <int HD, int VCH, int OCC = (HD <= 64 ? ATT_OCC : 2)>
static void launch_att(const float *qkv, int B, int T, int d, int n_heads, const float *pos, const float *bias_u, const float *bias_v,
                       float *ctx, float scale_arg, hipStream_t s, float *scratch, int ctx_bf16, int pos_row0, const SeqRag &rag) {
    const float scale = scale_arg > 0.0f ? scale_arg : 1.0f / sqrtf((float)HD);   // src/encoder.cpp:126
    if (rag.units.u) T = rag.T_max;                                // the score block is laid out for the longest utterance of the batch
    const int pits = att_score_pitch(T);
    const int n_rb = (T + RB - 1) / RB, n_bh = B * n_heads;
    const dim3 grid = att_grid(n_bh, n_rb, n_heads, rag);
    auto go = [&](auto ragged) {
        constexpr bool RAG = decltype(ragged)::value;
        if (scratch)
            hipLaunchKernelGGL((relpos_attention_kernel<HD, VCH, true, RAG, OCC>), grid, dim3(256), (size_t)VCH * (HD + 16) * sizeof(float), s, qkv, 3 * d, d, T, pos,
                               bias_u, bias_v, scale, ctx, pits, n_rb, n_bh, scratch, ctx_bf16, pos_row0, rag, 0, 0);
        else
            att_launch_dyn_lds<relpos_attention_kernel<HD, VCH, false, RAG, OCC>>(grid, dim3(256), att_block_lds_bytes(T, HD, VCH), s, qkv, 3 * d, d, T, pos, bias_u,
                                                                                  bias_v, scale, ctx, pits, n_rb, n_bh, (float *)nullptr, ctx_bf16, pos_row0, rag, 0, 0);
    };
    if (rag.units.u) go(std::true_type{});
    else go(std::false_type{});
}

// LDS bytes one workgroup needs for T frames: the [32][T] score block (four k-planes) + one V chunk.  0: unsupported head size.
size_t relpos_attention_lds_bytes(int T, int hd) { return att_hd_supported(hd) ? att_block_lds_bytes(T, hd, att_block_vch(hd)) : 0; }
// bytes of global scratch the long-sequence variant needs (0: unsupported head size)
size_t relpos_attention_scratch_bytes(int B, int T, int n_heads, int hd) {
    return relpos_attention_scratch_bytes_units((T + RB - 1) / RB, T, B * n_heads, hd);
}
size_t relpos_attention_scratch_bytes_units(int64_t n_units, int T_max, int n_heads, int hd) {
    if (!att_hd_supported(hd)) return 0;
    return (size_t)((n_heads + 7) / 8) * 8 * (size_t)n_units * 4 * (size_t)att_score_plane(att_score_pitch(T_max)) * sizeof(float);
}
// longest sequence whose score block fits the 160 KB of LDS of a CU (hd 64: 1064 frames = 85 s of audio; hd 128: 1104)
int relpos_attention_max_frames(int hd) {
    int T = 0;
    while (relpos_attention_lds_bytes(T + 8, hd) && relpos_attention_lds_bytes(T + 8, hd) <= 160 * 1024) T += 8;
    return T;
}

// The strip form's shape (tools/ubench/attn_bench sweeps them with -D): waves per workgroup of the uniform form, V chunk rows, columns of
// probabilities handed to the AV chains at a time.  4 / 32 / 64: 31 KB of LDS per workgroup, four workgroups per CU.
#ifndef ATT_STRIP_NW
#define ATT_STRIP_NW 4
#endif
#ifndef ATT_STRIP_VCH
#define ATT_STRIP_VCH 32
#endif
#ifndef ATT_STRIP_PW
#define ATT_STRIP_PW 64
#endif
#ifndef ATT_STRIP_DEFAULT
#define ATT_STRIP_DEFAULT 1       // 1: launches the strip form covers take it; 0: only on request (ATT_FORM_STRIP)
#endif

// Which kernel a launch runs: every threshold of the choice lives here (the launcher switches on it, pk_diag_relpos_attention_form reports
// it).  t_longest: T of a uniform batch, the longest utterance of a ragged one.  -1: the form asked for does not cover the launch.
int relpos_attention_form(int t_longest, int hd, bool scratch, int want) {
    const bool strip_ok = !scratch && t_longest >= 1 && t_longest <= STRIP_T && (hd == 64 || hd == 32);
    if (want == ATT_FORM_STRIP) return strip_ok ? ATT_FORM_STRIP : -1;
    if (want == ATT_FORM_BLOCK) return ATT_FORM_BLOCK;
    return (ATT_STRIP_DEFAULT && strip_ok) ? ATT_FORM_STRIP : ATT_FORM_BLOCK;
}

template <int HD>
static void launch_att_strip(const float *qkv, int B, int T, int d, int n_heads, const float *pos, const float *bias_u, const float *bias_v,
                             float *ctx, float scale_arg, hipStream_t s, int ctx_bf16, int pos_row0, const SeqRag &rag) {
    const float scale = scale_arg > 0.0f ? scale_arg : 1.0f / sqrtf((float)HD);
    constexpr int VCH = ATT_STRIP_VCH, PW = ATT_STRIP_PW, NW = ATT_STRIP_NW;
    auto lds_bytes = [](int nw) { return (size_t)(VCH * (HD + 16) + nw * 4 * (16 * (PW / 4 + 4) + 4)) * sizeof(float); };
    if (rag.units.u) {                                              // the engine's units are 32-row blocks: two strips per workgroup
        att_launch_dyn_lds<relpos_attention_strip_kernel<HD, VCH, 2, PW, true, 4>>(att_grid(0, 0, n_heads, rag), dim3(128), lds_bytes(2), s, qkv, 3 * d, d, rag.T_max,
                                                                                   pos, bias_u, bias_v, scale, ctx, 0, 0, ctx_bf16, pos_row0, rag);
        return;
    }
    const int n_rb = (T + 16 * NW - 1) / (16 * NW), n_bh = B * n_heads;
    att_launch_dyn_lds<relpos_attention_strip_kernel<HD, VCH, NW, PW, false, 4>>(att_grid(n_bh, n_rb, n_heads, rag), dim3(64 * NW), lds_bytes(NW), s, qkv, 3 * d, d, T,
                                                                                 pos, bias_u, bias_v, scale, ctx, n_rb, n_bh, ctx_bf16, pos_row0, rag);
}

void launch_relpos_attention(const float *qkv, int B, int T, int d, int n_heads, const float *pos, const float *bias_u,
                             const float *bias_v, float *ctx, hipStream_t s, float scale, float *scratch, int ctx_bf16, int pos_row0, const SeqRag &rag,
                             int form) {
    const int hd = d / n_heads;
    if (relpos_attention_form(rag.units.u ? rag.T_max : T, hd, scratch != nullptr, form) == ATT_FORM_STRIP) {
        if (hd == 64) launch_att_strip<64>(qkv, B, T, d, n_heads, pos, bias_u, bias_v, ctx, scale, s, ctx_bf16, pos_row0, rag);
        else launch_att_strip<32>(qkv, B, T, d, n_heads, pos, bias_u, bias_v, ctx, scale, s, ctx_bf16, pos_row0, rag);
        return;
    }
    // V chunk rows: 64 keeps the footprint at ~39 KB for 10 s clips (4 workgroups per CU at hd = 64).  Between ~10.5 and ~16 s (T = 132 .. 200:
    // the longest clip of a mixed batch, 15 s uniform batches) the 64-row chunk costs the fourth resident workgroup; a 32-row chunk (two more
    // barriers per extra chunk, the same chains: same bits) keeps it
    if (hd == 64) {
        const int t_lds = rag.units.u ? rag.T_max : T;
        auto occ = [&](int vch) {
            const int n = (int)((size_t)160 * 1024 / att_block_lds_bytes(t_lds, 64, vch));
            return n < ATT_OCC ? n : ATT_OCC;
        };
        // (measured on a 5-15 s mixed batch, T_max = 185: 32-row chunks at four workgroups per CU 1.69 ms, 64-row chunks at three without spills 1.77,
        //  64-row chunks at three on the 128-VGPR build 1.85)
        if (!scratch && occ(32) > occ(64)) launch_att<64, 32>(qkv, B, T, d, n_heads, pos, bias_u, bias_v, ctx, scale, s, scratch, ctx_bf16, pos_row0, rag);
        // LDS allows at most three workgroups per CU whatever the chunk (T > 200): the register budget of three (the kernel needs 128-136 VGPRs: no spills)
        else if (!scratch && occ(64) <= 3) launch_att<64, 64, 3>(qkv, B, T, d, n_heads, pos, bias_u, bias_v, ctx, scale, s, scratch, ctx_bf16, pos_row0, rag);
        else launch_att<64, 64>(qkv, B, T, d, n_heads, pos, bias_u, bias_v, ctx, scale, s, scratch, ctx_bf16, pos_row0, rag);
    } else if (hd == 128) launch_att<128, 32>(qkv, B, T, d, n_heads, pos, bias_u, bias_v, ctx, scale, s, scratch, ctx_bf16, pos_row0, rag);
    else if (hd == 32) launch_att<32, 64>(qkv, B, T, d, n_heads, pos, bias_u, bias_v, ctx, scale, s, scratch, ctx_bf16, pos_row0, rag);
    else if (hd == 96) launch_att<96, 64>(qkv, B, T, d, n_heads, pos, bias_u, bias_v, ctx, scale, s, scratch, ctx_bf16, pos_row0, rag);
}

// ---- the band form's launcher ------------------------------------------------------------------------------------------------------------------
template <int HD, int VCH, int OCC>
static void launch_local(const float *qkv, int B, int T, int d, int n_heads, const float *pos, const float *bias_u, const float *bias_v,
                         float *ctx, hipStream_t s, int ctx_bf16, int left, int right, int W, const SeqRag &rag) {
    const float scale = 1.0f / sqrtf((float)HD);                   // src/encoder.cpp:126
    const int n_rb = (T + RB - 1) / RB, n_bh = B * n_heads;
    auto go = [&](auto ragged) {
        att_launch_dyn_lds<relpos_attention_kernel<HD, VCH, false, decltype(ragged)::value, OCC, true>>(
            att_grid(n_bh, n_rb, n_heads, rag), dim3(256), att_block_lds_bytes(W, HD, VCH), s, qkv, 3 * d, d, T, pos, bias_u, bias_v, scale, ctx, att_score_pitch(W),
            n_rb, n_bh, (float *)nullptr, ctx_bf16, 0, rag, left, right);
    };
    if (rag.units.u) go(std::true_type{});
    else go(std::false_type{});
}

int relpos_local_attention_max_span(int hd) {
    if (!att_hd_supported(hd)) return -1;
    int span = -1;                                                  // left + right: the window of a block is left + right + 32 columns
    while (att_block_lds_bytes(span + 1 + RB, hd, att_block_vch(hd)) <= 160 * 1024) ++span;
    return span;
}

void launch_relpos_local_attention(const float *qkv, int B, int T, int d, int n_heads, const float *pos, const float *bias_u, const float *bias_v,
                                   float *ctx, hipStream_t s, int ctx_bf16, int left, int right, const SeqRag &rag) {
    const int hd = d / n_heads;
    const int t_lds = rag.units.u ? rag.T_max : T;
    const int W = t_lds < left + right + RB ? t_lds : left + right + RB;   // widest window of any block of the launch (LDS sizing)
    const int occ = (int)((size_t)160 * 1024 / att_block_lds_bytes(W, hd, att_block_vch(hd)));
    if (hd == 64) {
        if (occ >= 4) launch_local<64, 64, 4>(qkv, B, T, d, n_heads, pos, bias_u, bias_v, ctx, s, ctx_bf16, left, right, W, rag);
        else launch_local<64, 64, 3>(qkv, B, T, d, n_heads, pos, bias_u, bias_v, ctx, s, ctx_bf16, left, right, W, rag);
    } else if (hd == 128) launch_local<128, 32, 2>(qkv, B, T, d, n_heads, pos, bias_u, bias_v, ctx, s, ctx_bf16, left, right, W, rag);
    else if (hd == 32) launch_local<32, 64, 4>(qkv, B, T, d, n_heads, pos, bias_u, bias_v, ctx, s, ctx_bf16, left, right, W, rag);
    else if (hd == 96) launch_local<96, 64, 2>(qkv, B, T, d, n_heads, pos, bias_u, bias_v, ctx, s, ctx_bf16, left, right, W, rag);
}

// ---- the causal form's launcher (always ragged: packed sequences of rag.T[b] <= 512 positions) ----------------------------------------------------
template <int HD, int VCH>
static void launch_causal(const float *qkv, int d, int n_heads, float scale, float *ctx, hipStream_t s, const SeqRag &rag) {
    const int W = rag.T_max;                                        // the widest window of any block: every key of the longest sequence
    att_launch_dyn_lds<relpos_attention_kernel<HD, VCH, false, true, 2, true, true>>(
        att_grid(0, 0, n_heads, rag), dim3(256), att_block_lds_bytes(W, HD, VCH), s, qkv, 3 * d, d, rag.T_max, (const float *)nullptr, (const float *)nullptr,
        (const float *)nullptr, scale, ctx, att_score_pitch(W), 0, 0, (float *)nullptr, 0, 0, rag, 0, 0);
}
size_t causal_attention_lds_bytes(int T_max, int hd) { return att_hd_supported(hd) ? att_block_lds_bytes(T_max, hd, att_block_vch(hd)) : 0; }
void launch_causal_attention(const float *qkv, int d, int n_heads, float scale, float *ctx, hipStream_t s, const SeqRag &rag) {
    const int hd = d / n_heads;
    if (hd == 64) launch_causal<64, 64>(qkv, d, n_heads, scale, ctx, s, rag);
    else if (hd == 128) launch_causal<128, 32>(qkv, d, n_heads, scale, ctx, s, rag);
    else if (hd == 32) launch_causal<32, 64>(qkv, d, n_heads, scale, ctx, s, rag);
    else if (hd == 96) launch_causal<96, 64>(qkv, d, n_heads, scale, ctx, s, rag);
}

}  // namespace pk
