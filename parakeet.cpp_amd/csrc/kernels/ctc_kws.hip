// parakeet.cpp_amd/csrc/kernels/ctc_kws.hip -- CTC keyword spotting on the device: where in an utterance was each keyword said.
//
// The specification is tests/ctc_kws_ref.py (walk + pick): max-plus on the 2 L - 1 state lattice of a keyword (no leading or trailing blank) with a free
// start (state 0 may be entered at any frame with value +0.0) and a free end (the last state's value is read at every frame); the cost of a symbol at a
// frame is fl(lp - g), g the row's maximum; candidates in the order stay / previous state / skip / enter, strict >; every state carries the frame at
// which its path entered, so one row of (a, b) is the whole state.  Every score is compared bit for bit, every span and count exactly.
//
//   ctc_rowmax_kernel   g[r] = max_v lp[r][v], one wave per row (four rows per workgroup), wave_max64.  A maximum is exact in any order.
//
//   ctc_kws_kernel      ONE WAVE per (keyword, utterance): grid n_kw x B, 64 threads.  Lane i keeps the token state 2 i and the blank state 2 i + 1
//       (value and entry frame each) in registers for the whole walk; L <= 64.  Per frame the only cross-lane traffic is lane i - 1's four registers,
//       moved by four v_mov_b32 with the DPP modifier wave_shr:1 (lane 0 keeps the "old" operand: -inf / 0): no ds_bpermute, no LDS, no barrier, no
//       back-pointer memory.  The blank state 2 L - 1 of lane L - 1 and the lanes past L are computed and never read.
//       The frame loop is sequential and latency-bound, so what a frame reads from memory -- lp[t][ids[i]] per lane, the blank's column and g[t]
//       (both wave-uniform) -- is requested kKwsAhead = 8 frames ahead, a whole chunk of 8 frames at a time into a second set of registers; the dependent
//       chain of a frame is the subtract, the DPP moves and the compare / select / add sequence.
//       Lane L - 1 stores (E[t], Bs[t]) = its token state as one 8-byte vector store per frame into the scratch [B][n_kw][T_b].
//     Picking is the tail of the same kernel by the same wave (one launch less, and the rows are still in the cache): after a workgroup fence,
//       max_hits sweeps over the T_b entries, lane l reading t = l, l + 64, ...; a sweep first applies the mask of the hit before it (an entry whose span
//       meets the hit's gets -inf written back by the lane that reads it again in the next sweep, so no lane depends on another lane's store),
//       keeps the lane's best (larger score, earlier frame on a tie because frames ascend), then a six-step DPP butterfly argmax over (score, frame)
//       with the lowest-frame tie rule.  Unused slots are filled 0 / 0 / -inf here.
//
// The row maximum is its own pass over the rows, so the host-rows entry point and the model's share one path.
//
// Bounds: the frame index of a request is clamped to T - 1, token columns are checked on the host to lie in [0, V), a lane past the keyword reads
// the blank's column; scratch entry (b, k, t) is n_kw * T_off[b] + k * T_b + t < n_kw * sum T, in 64 bits.
//
// Code objects (hipcc -O3 --offload-arch=gfx950, from the .s of -save-temps):
//   ctc_kws_kernel      60 VGPR   72 SGPR  LDS 0 B  scratch 0 B; 0 VGPR spills, 0 SGPRs spilled to VGPR lanes
//   ctc_rowmax_kernel   22 VGPR   24 SGPR  LDS 0 B  scratch 0 B; 0 VGPR spills, 0 SGPRs spilled to VGPR lanes
#include "kernels.hpp"
#include "../pk_devmath.h"

namespace pk {

namespace {

// the value of lane - 1 (lane 0: `edge`), one v_mov_b32 with the DPP modifier wave_shr:1
__device__ __forceinline__ int lane_below_i(int x, int edge) { return __builtin_amdgcn_update_dpp(edge, x, 0x138, 0xF, 0xF, false); }
__device__ __forceinline__ float lane_below(float x, float edge) { return __int_as_float(lane_below_i(__float_as_int(x), __float_as_int(edge))); }

}  // namespace

__global__ __launch_bounds__(256) void ctc_rowmax_kernel(const float *__restrict__ lp, float *__restrict__ g, int64_t rows, int V) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;                                          // (a whole wave)
    const int lane = threadIdx.x & 63;
    const float *row = lp + r * V;
    float m = -__builtin_huge_valf();
    for (int v = lane; v < V; v += 64) m = fmaxf(m, row[v]);
    m = wave_max64(m);
    if (lane == 0) g[r] = m;
}

__global__ __launch_bounds__(64) void ctc_kws_kernel(CtcKwsArgs a) {
    constexpr int AH = kKwsAhead;
    const int k = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    int T = a.T;
    int64_t in0 = (int64_t)b * T;
    if (a.rg.T) { in0 = a.rg.T_off[b]; T = a.rg.T[b]; }
    const int i0 = a.kw_off[k], L = a.kw_off[k + 1] - i0;
    const int V = a.V, blank = a.blank;
    const float NEG = -__builtin_huge_valf();
    const int tok = lane < L ? a.ids[i0 + lane] : blank;
    const bool may_skip = lane >= 1 && lane < L && tok != a.ids[i0 + (lane >= 1 ? lane - 1 : 0)];
    const float *lp = a.lp + in0 * V;
    const float *g = a.g + in0;
    int2 *eb = a.eb + (in0 * a.n_kw + (int64_t)k * T);

    float nt[AH], nb[AH], ng[AH];                                   // the next chunk's log-probs: token column, blank column, row maximum
    auto fetch = [&](int t0) {
#pragma unroll
        for (int j = 0; j < AH; ++j) {
            const int tt = t0 + j < T ? t0 + j : T - 1;
            const float *row = lp + (int64_t)tt * V;
            nt[j] = row[tok]; nb[j] = row[blank]; ng[j] = g[tt];
        }
    };
    float a0 = NEG, a1 = NEG;                                       // token state 2 i, blank state 2 i + 1
    int b0 = 0, b1 = 0;
    fetch(0);
    for (int t0 = 0; t0 < T; t0 += AH) {
        float xt[AH], xb[AH], xg[AH];
#pragma unroll
        for (int j = 0; j < AH; ++j) { xt[j] = nt[j]; xb[j] = nb[j]; xg[j] = ng[j]; }
        if (t0 + AH < T) fetch(t0 + AH);
#pragma unroll
        for (int j = 0; j < AH; ++j) {
            const int t = t0 + j;
            if (t < T) {                                            // (uniform)
                const float c0 = xt[j] - xg[j], c1 = xb[j] - xg[j];
                const float pa1 = lane_below(a1, NEG), pa0 = lane_below(a0, NEG);
                const int pb1 = lane_below_i(b1, 0), pb0 = lane_below_i(b0, 0);
                float best = a0;                                    // stay
                int org = b0;
                if (pa1 > best) { best = pa1; org = pb1; }          // previous state: the blank of lane i - 1
                if (may_skip && pa0 > best) { best = pa0; org = pb0; }   // skip: the token of lane i - 1, where it differs
                if (lane == 0 && 0.0f > best) { best = 0.0f; org = t; }  // enter
                float bb = a1;                                      // the blank: stay, or this lane's token
                int bo = b1;
                if (a0 > bb) { bb = a0; bo = b0; }
                a0 = best + c0; b0 = org;
                a1 = bb + c1; b1 = bo;
                if (lane == L - 1) eb[t] = make_int2(__float_as_int(a0), b0);
            }
        }
    }
    __threadfence_block();
    __syncthreads();                                                // lane L - 1's stores are read by every lane from here on

    const int H = a.max_hits;
    const float min_score = a.min_score;
    const int64_t ob = (int64_t)b * a.n_kw + k;
    int *start = a.start + ob * H, *end = a.end + ob * H;
    float *score = a.score + ob * H;
    int n = 0, ps = 0, pe = -1;                                     // hits so far; the span of the last one
    for (int h = 0; h < H; ++h) {
        float bv = NEG;
        int bt = 0x7fffffff;
        for (int t = lane; t < T; t += 64) {
            const int2 v = eb[t];
            float e = __int_as_float(v.x);
            if (n > 0 && e > NEG && v.y <= pe && ps <= t) {         // [Bs[t], t] meets the last hit: masked from now on
                e = NEG;
                eb[t].x = __float_as_int(NEG);
            }
            if (e > NEG && e >= min_score && e > bv) { bv = e; bt = t; }
        }
        wave_butterfly([&](auto off) {
            constexpr int OFF = decltype(off)::value;
            const float ov = wave_xor<OFF>(bv);
            const int ot = wave_xor_i<OFF>(bt);
            if (ov > bv || (ov == bv && ot < bt)) { bv = ov; bt = ot; }
        });
        if (!(bv > NEG)) break;                                     // (uniform: every lane holds the same pair)
        ps = eb[bt].y; pe = bt;
        if (lane == 0) { start[h] = ps; end[h] = pe; score[h] = bv; }
        ++n;
    }
    if (lane == 0) a.n_hits[ob] = n;
    if (lane >= n && lane < H) { start[lane] = 0; end[lane] = 0; score[lane] = NEG; }
}

void launch_ctc_rowmax(const float *lp, float *g, int64_t rows, int V, hipStream_t s) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(ctc_rowmax_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, lp, g, rows, V);
}

void launch_ctc_kws(const CtcKwsArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(ctc_kws_kernel, dim3(a.n_kw, a.B), dim3(64), 0, s, a);
}

}  // namespace pk
