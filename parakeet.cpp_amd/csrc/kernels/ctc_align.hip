// parakeet.cpp_amd/csrc/kernels/ctc_align.hip -- CTC forced alignment of a GIVEN token string on the device.
//
// The specification is tests/ctc_beam_ref.py::viterbi_align (max-plus on the 2 L + 1 state lattice, fp32, one add per cell, predecessor ties
// stay / previous / skip, end state the last blank unless the last token's state is strictly better) and, for the optional log-likelihood,
// tests/ctc_align_ref.py::forward_total (the same lattice with lae(lae(stay, prev), skip) + lp per cell).  Every value is compared bit for bit.
//
//   ctc_align_kernel<NT, SP, TOTAL>   one workgroup of NT threads per utterance.  Thread i owns the SP contiguous states [i SP, (i + 1) SP) for
//       the whole walk: their alpha values (and the forward pass's, TOTAL) live in REGISTERS, the ids of its SP / 2 token states too, and the
//       permission to skip onto them is one bit each.  A strip starts on a blank state, which has no skip, so per frame a thread needs only the
//       LAST value of its left neighbour: every thread publishes it (max-plus value, forward value) in a double-buffered LDS table, ONE barrier per frame.  LDS does not
//       grow with T or L.  The frame's log-probs (blank + SP / 2 gathered columns) are loaded one frame ahead of their use.
//       Band: a strip whose first state is past 2 t + 1 (not reachable yet) or whose last state can no longer reach the end
//       (S - 1 - s > 2 (T - 1 - t) + 1) skips the frame: the first kind holds -inf and would compute -inf, the second kind feeds only
//       cells that cannot reach the end either.  The result is unchanged (tests/test_ctc_align_ref.py checks that rule in the reference).
//       What the band saves is the arithmetic and the gathers, and at SP = 32 the skipped strips' back-pointer stores; at SP < 16 lanes share
//       a dword and skipped strips store zeros.  The scratch is sized for the full T x ceil(S / 16) lattice either way: only the band is read.
//       Back-pointers: 2 bits per cell, 16 cells per dword, row t of an utterance = ceil(S / 16) dwords.  A thread packs its SP cells; for
//       SP < 16 the 16 / SP lanes of one dword OR their fields together with cross-lane moves and one of them stores it, so a wave
//       stores whole consecutive dwords.
//       Back-trace: kAlignTraceFrames (64) frames per step.  In 64 frames the path moves down at most 126 states, so the rows' dwords that
//       can be visited (at most 9 per row) are staged in LDS by the whole workgroup, then one thread walks them there: no dependent global load
//       per frame.  start[k] / end[k] are stored when the path enters / leaves token k; conf[k] = dexpf(lp[start[k]][ids[k]]) by all threads.
//
// Scratch: sum over the utterances of T_b * ceil((2 L_b + 1) / 16) * 4 bytes of back-pointers (one hour, T = 45000, L = 15000: 337.7 MB),
// capped at kAlignMaxScratch = 1 GiB by the host side (ctc_align.hpp), which also picks the narrowest shape that holds the longest string:
//   64 x 4 (S <= 256: a 10 s clip, one wave), 256 x 8 (S <= 2048), 1024 x 32 (S <= 32768, L <= 16383).
//
// Code objects (hipcc -O3 --offload-arch=gfx950, from the .s of -save-temps):
//   ctc_align_kernel<  64,  4, false>   40 VGPR   77 SGPR  LDS  3604 B  scratch   0 B; 0 VGPR spills, 0 SGPRs spilled to VGPR lanes
//   ctc_align_kernel<  64,  4, true >   43 VGPR   94 SGPR  LDS  3604 B  scratch   0 B; 0 VGPR spills, 0 SGPRs spilled to VGPR lanes
//   ctc_align_kernel< 256,  8, false>   46 VGPR   81 SGPR  LDS  6676 B  scratch   0 B; 0 VGPR spills, 0 SGPRs spilled to VGPR lanes
//   ctc_align_kernel< 256,  8, true >   64 VGPR  100 SGPR  LDS  6676 B  scratch   0 B; 0 VGPR spills, 0 SGPRs spilled to VGPR lanes
//   ctc_align_kernel<1024, 32, false>  127 VGPR  106 SGPR  LDS 18964 B  scratch   0 B; 0 VGPR spills, 2 SGPRs spilled to VGPR lanes
//   ctc_align_kernel<1024, 32, true >  128 VGPR  106 SGPR  LDS 18964 B  scratch 132 B; 32 VGPR spills, 112 SGPRs spilled to VGPR lanes
//   (the forward pass at 1024 x 32 does not load a frame ahead: with the 17 more registers it spilled about twice as many VGPRs)
#include "kernels.hpp"
#include "../pk_devmath.h"

namespace pk {

namespace {

constexpr int kTraceDw = 10;                                       // dwords of one staged back-pointer row (9 can be visited, see above)

}  // namespace

template <int NT, int SP, bool TOTAL>
__global__ __launch_bounds__(NT) void ctc_align_kernel(CtcAlignArgs a) {
    static_assert(SP % 2 == 0 && (SP == 32 || 16 % SP == 0), "a strip starts on a blank state and packs into whole dwords");
    constexpr int NJ = SP / 2;                                      // token states of a strip
    constexpr int G = SP >= 16 ? 1 : 16 / SP;                       // lanes that share one back-pointer dword
    constexpr bool PF = !(TOTAL && SP >= 32);                       // log-probs loaded a frame ahead (not where the registers run out)
    __shared__ float2 xch[2][NT];                                   // (alpha, forward value) of the last state of every strip
    __shared__ unsigned tr[kAlignTraceFrames * kTraceDw];
    __shared__ float fin[4];
    __shared__ int s_cur;
    const int b = blockIdx.x, tid = threadIdx.x;
    int T = a.T;
    int64_t in0 = (int64_t)b * T;
    if (a.rg.T) { in0 = a.rg.T_off[b]; T = a.rg.T[b]; }
    const int i0 = a.id_off[b], L = a.id_off[b + 1] - i0, S = 2 * L + 1, RW = (S + kAlignBpCells - 1) / kAlignBpCells;
    const int *ids = a.ids + i0;
    unsigned *bp = a.bp + a.bp_off[b];
    const int V = a.V, blank = a.blank, base = tid * SP;
    const float NEG = -__builtin_huge_valf();

    int tok[NJ];
    unsigned skipm = 0;                                             // bit j: the strip's j-th token differs from the token before it
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = (base >> 1) + j;                              // state base + 2 j + 1 is token k
        tok[j] = k < L ? ids[k] : blank;
        if (k >= 1 && k < L && ids[k] != ids[k - 1]) skipm |= 1u << j;
    }
    float al[SP], ta[TOTAL ? SP : 1];
    {
        const float *row = a.lp + in0 * V;
#pragma unroll
        for (int u = 0; u < SP; ++u) {
            const int s = base + u;
            float v = NEG;
            if (s == 0) v = row[blank];
            else if (s == 1 && L > 0) v = row[tok[0]];
            al[u] = v;
            if constexpr (TOTAL) ta[u] = v;
        }
    }
    // the frame's cells of this strip are worth computing (see the header: band)
    auto live = [&](int t) { return base < S && base <= 2 * t + 1 && base + SP - 1 >= S - 1 - (2 * (T - 1 - t) + 1); };
    float eb_n = 0.0f, e_n[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) e_n[j] = 0.0f;
    auto fetch = [&](int t) {
        const float *row = a.lp + (in0 + t) * V;
        eb_n = row[blank];
#pragma unroll
        for (int j = 0; j < NJ; ++j) e_n[j] = row[tok[j]];
    };
    if (PF && T > 1 && live(1)) fetch(1);
    xch[0][tid] = make_float2(al[SP - 1], TOTAL ? ta[TOTAL ? SP - 1 : 0] : NEG);
    __syncthreads();
    for (int t = 1; t < T; ++t) {
        if (!PF && live(t)) fetch(t);
        const float eb = eb_n;
        float e[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) e[j] = e_n[j];
        if (PF && t + 1 < T && live(t + 1)) fetch(t + 1);
        unsigned long long bits = 0;
        const bool is_live = live(t);
        if (is_live) {
            float2 nb = make_float2(NEG, NEG);                      // the state before the strip (a token state: the strip starts on a blank)
            if (tid) nb = xch[(t - 1) & 1][tid - 1];
#pragma unroll
            for (int u = SP - 1; u >= 0; --u) {                     // downwards: al[u - 1], al[u - 2] are still the previous frame's
                const bool token = u & 1, may_skip = token && ((skipm >> (u >> 1)) & 1u);
                const float prev = u >= 1 ? al[u >= 1 ? u - 1 : 0] : nb.x;
                const float skip = u >= 2 ? al[u >= 2 ? u - 2 : 0] : nb.x;   // (u = 1; a blank, u = 0, never skips)
                const float ev = token ? e[u >> 1] : eb;
                float best = al[u];
                unsigned p = 0;
                if (prev > best) { best = prev; p = 1; }
                if (may_skip && skip > best) { best = skip; p = 2; }
                al[u] = best + ev;
                bits |= (unsigned long long)p << (2 * u);
                if constexpr (TOTAL) {
                    const float tprev = u >= 1 ? ta[u >= 1 ? u - 1 : 0] : nb.y;
                    const float tskip = u >= 2 ? ta[u >= 2 ? u - 2 : 0] : nb.y;
                    float x = dlaef(ta[u], tprev);
                    if (token) x = dlaef(x, may_skip ? tskip : NEG);
                    ta[u] = x + ev;
                }
            }
        }
        xch[t & 1][tid] = make_float2(al[SP - 1], TOTAL ? ta[TOTAL ? SP - 1 : 0] : NEG);
        unsigned *row = bp + (int64_t)t * RW;
        if constexpr (G == 1) {
#pragma unroll
            for (int q = 0; q < SP / 16; ++q) {
                const int d = tid * (SP / 16) + q;
                if (d < RW && is_live) row[d] = (unsigned)(bits >> (32 * q));   // (a skipped strip's dwords are never read by the back-trace)
            }
        } else {
            unsigned v = (unsigned)bits << ((tid & (G - 1)) * 2 * SP);
#pragma unroll
            for (int o = 1; o < G; o <<= 1) v |= (unsigned)__shfl_xor((int)v, o);
            const int d = tid / G;
            if ((tid & (G - 1)) == 0 && d < RW) row[d] = v;
        }
        __syncthreads();                                            // one barrier per frame (the exchange table is double buffered)
    }
#pragma unroll
    for (int u = 0; u < SP; ++u) {
        const int s = base + u;
        if (s == S - 1) { fin[0] = al[u]; fin[2] = TOTAL ? ta[TOTAL ? u : 0] : NEG; }
        if (s == S - 2) { fin[1] = al[u]; fin[3] = TOTAL ? ta[TOTAL ? u : 0] : NEG; }
    }
    __syncthreads();
    if (tid == 0) {
        int se = S - 1;
        if (L > 0 && fin[1] > fin[0]) se = S - 2;
        const float sc = se == S - 1 ? fin[0] : fin[1];
        const bool okv = sc > NEG;
        a.score[b] = okv ? sc : NEG;
        a.ok[b] = okv ? 1 : 0;
        if constexpr (TOTAL) a.total[b] = L > 0 ? dlaef(fin[0 + 2], fin[1 + 2]) : fin[2];
        s_cur = okv ? se : -1;
    }
    __syncthreads();
    if (s_cur < 0 || L == 0) return;                                // (uniform) cannot be aligned: the caller's zeros stay; no token: nothing to trace
    int *start = a.start + i0, *end = a.end + i0;
    int lastk = -1;                                                 // (thread 0) the token whose end frame is known
    for (int t_hi = T - 1; t_hi >= 1;) {
        const int t_lo = t_hi - (kAlignTraceFrames - 1) > 1 ? t_hi - (kAlignTraceFrames - 1) : 1, nfr = t_hi - t_lo + 1;
        const int s_hi = s_cur;
        const int s_lo = s_hi - 2 * (nfr - 1) > 0 ? s_hi - 2 * (nfr - 1) : 0;
        const int d_lo = s_lo >> 4, nd = (s_hi >> 4) - d_lo + 1;    // nd <= 9 <= kTraceDw, d_lo + nd <= RW
        for (int i = tid; i < nfr * nd; i += NT) {
            const int r = i / nd, d = i - r * nd;
            tr[r * kTraceDw + d] = bp[(int64_t)(t_lo + r) * RW + d_lo + d];
        }
        __syncthreads();
        if (tid == 0) {
            int s = s_hi;
            for (int t = t_hi; t >= t_lo; --t) {
                const unsigned p = (tr[(t - t_lo) * kTraceDw + (s >> 4) - d_lo] >> ((s & 15) * 2)) & 3u;
                if (s & 1) {
                    const int k = s >> 1;
                    if (k != lastk) { end[k] = t; lastk = k; }
                    if (p) start[k] = t;
                }
                s -= (int)(p < 2u ? p : 2u);
                if (s < 0) s = 0;                                   // (cannot happen: states 0 and 1 have no such predecessor)
            }
            s_cur = s;
        }
        t_hi = t_lo - 1;
        __syncthreads();
    }
    if (tid == 0) {
        const int s = s_cur;                                        // frame 0: state 0 or 1
        if (s & 1) {
            const int k = s >> 1;
            if (k != lastk) end[k] = 0;
            start[k] = 0;
        }
        __threadfence_block();
    }
    __syncthreads();
    for (int k = tid; k < L; k += NT) a.conf[i0 + k] = dexpf(a.lp[(in0 + start[k]) * V + ids[k]]);
}

void launch_ctc_align(const CtcAlignArgs &a, int shape, hipStream_t s) {
    const dim3 grid(a.B);
    const bool tot = a.total != nullptr;
    switch (shape) {
    case 0:
        if (tot) hipLaunchKernelGGL((ctc_align_kernel<64, 4, true>), grid, dim3(64), 0, s, a);
        else hipLaunchKernelGGL((ctc_align_kernel<64, 4, false>), grid, dim3(64), 0, s, a);
        break;
    case 1:
        if (tot) hipLaunchKernelGGL((ctc_align_kernel<256, 8, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((ctc_align_kernel<256, 8, false>), grid, dim3(256), 0, s, a);
        break;
    default:
        if (tot) hipLaunchKernelGGL((ctc_align_kernel<1024, 32, true>), grid, dim3(1024), 0, s, a);
        else hipLaunchKernelGGL((ctc_align_kernel<1024, 32, false>), grid, dim3(1024), 0, s, a);
        break;
    }
}

}  // namespace pk
