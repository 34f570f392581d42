// parakeet.cpp_amd/csrc/kernels/resample.hip -- polyphase form of the host's Kaiser-windowed sinc resampler on the device.
//
// The specification is tests/resample_ref.py: with g = gcd(src, dst), up = dst / g, down = src / g, output i = q * up + r of a clip of n input
// samples has the centre c = q * down + (r * down) / up and reads the taps j = c - 15 + k, k = 0 .. 31, skipping j < 0 and j >= n;
// sum += (double)x[j] * T[r][k] and wsum += T[r][k] for k ascending, every operation rounded on its own (the build has -ffp-contract=off), and
// out = wsum > 1e-10 ? (float)(sum / wsum) : 0.  The table T[up][32] is built on the host in fp64 (resample.cpp) from the expressions of
// sinc_resample (wav.cpp); the kernel evaluates no transcendental.  Compared bit for bit.
//
//   resample_kernel<LDS_TAB>   a workgroup of 256 lanes owns `run` consecutive outputs [i0, i0 + cnt) of ONE clip (found by a binary search over the
//       clips' first workgroups).  Their taps cover the input samples [c(i0) - 15, c(i0 + cnt - 1) + 16]: at most run * down / up + 33 floats, staged
//       into LDS with coalesced loads, zero outside [0, n) (those taps are skipped, never read as zeros).  Lane t then walks the outputs t, t + 256, ...
//       The phase and the centre come from one 32-bit division per output: r0 = i0 mod up and q0 = i0 / up are workgroup-uniform (one 64-bit
//       division), r = (r0 + t) mod up, and the integer part of r * down / up is the table coff[r], so the centre relative to the staged span is
//       ((r0 + t) / up) * down + coff[r] - coff[r0].
//       LDS_TAB (up <= 160 rows): the table is staged into LDS, rows padded to 33 doubles -- consecutive lanes read consecutive rows at the same
//       tap, and a row stride of 66 dwords puts the 32 lanes of a ds_read_b64 group on 32 different bank pairs (64 dwords would put them on one).
//       The span is read at a lane stride of down / up floats (3 at 48 kHz, 2.76 at 44.1 kHz): odd or fractional, no systematic conflict.
//       Otherwise (640 rows at 11.025 kHz, 16 000 rows = 4 MB at 15 999 Hz) the rows are read from global memory: 256-byte rows, L2-resident.
//       Outputs whose 32 taps all lie inside the clip take an unrolled loop without the per-tap test; both loops add the same terms in the same order.
//
// Bounds: x is read at in_off + j for 0 <= j < n only; y is written at out_off + i0 + t for t < cnt <= out_len - i0; the staged span is
// c(i0 + cnt - 1) - c(i0) + 32 <= ceil((run - 1) * down / up) + 32 <= span_cap floats (the launcher sizes run from span_cap; a workgroup whose span
// would not fit returns without writing); LDS is span_cap * 4 bytes after the table's up * (33 * 8 + 4) bytes.
#include "kernels.hpp"

namespace pk {

namespace {

constexpr int kRowPitch = kResampleTaps + 1;    // doubles per table row in LDS

template <bool LDS_TAB>
__global__ __launch_bounds__(kResampleThreads) void resample_kernel(ResampleArgs a) {
    extern __shared__ double smem[];
    const int tid = threadIdx.x, up = a.up, down = a.down;
    // LDS: [up][33] doubles, [up] ints (rounded up to 8 bytes), then the span
    const double *tab = a.tab;
    const int *coff = a.coff;
    float *xs = reinterpret_cast<float *>(smem);
    if (LDS_TAB) {
        double *ts = smem;
        int *cs = reinterpret_cast<int *>(smem + (size_t)up * kRowPitch);
        xs = reinterpret_cast<float *>(cs + ((up + 1) & ~1));
        for (int e = tid; e < up * kResampleTaps; e += kResampleThreads) ts[(e >> 5) * kRowPitch + (e & 31)] = a.tab[e];
        for (int e = tid; e < up; e += kResampleThreads) cs[e] = a.coff[e];
        tab = ts; coff = cs;
    }
    // the clip of this workgroup: the last one whose first workgroup is <= blockIdx.x (clips without outputs own none and are never found)
    const int64_t wg = blockIdx.x;
    int lo = 0, hi = a.n_clips - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.clip[mid].wg0 <= wg) lo = mid; else hi = mid - 1;
    }
    const ResampleClip c = a.clip[lo];
    const int64_t i0 = (wg - c.wg0) * a.run, n = c.in_len;
    const int64_t left = c.out_len - i0;
    const int cnt = left < a.run ? (int)left : a.run;
    if (cnt <= 0) return;
    const int64_t q0 = i0 / up;
    const unsigned r0 = (unsigned)(i0 - q0 * up);
    const int co0 = a.coff[r0];
    const int64_t base = q0 * down + co0 - (kResampleTaps / 2 - 1);          // input index of xs[0]: tap 0 of output i0
    const unsigned rl = r0 + (unsigned)(cnt - 1), ql = rl / (unsigned)up;
    const int64_t span64 = (int64_t)ql * down + a.coff[rl - ql * (unsigned)up] - co0 + kResampleTaps;
    if (span64 > a.span_cap) return;
    const int span = (int)span64;
    const float *x = a.x + c.in_off;
    for (int e = tid; e < span; e += kResampleThreads) {
        const int64_t j = base + e;
        xs[e] = (j >= 0 && j < n) ? x[j] : 0.0f;
    }
    __syncthreads();
    const int ld = LDS_TAB ? kRowPitch : kResampleTaps;
    float *y = a.y + c.out_off + i0;
    for (int t = tid; t < cnt; t += kResampleThreads) {
        const unsigned rr = r0 + (unsigned)t, dq = rr / (unsigned)up, r = rr - dq * (unsigned)up;
        const int d = (int)(dq * (unsigned)down) + coff[r] - co0;              // centre of this output minus the centre of output i0
        const int64_t j0 = base + d;                                            // input index of tap 0
        const float *xp = xs + d;
        const double *w = tab + (size_t)r * ld;
        double sum = 0.0, wsum = 0.0;
        if (j0 >= 0 && j0 + kResampleTaps <= n) {
#pragma unroll
            for (int k = 0; k < kResampleTaps; ++k) {
                const double wk = w[k];
                sum += (double)xp[k] * wk;
                wsum += wk;
            }
        } else {
            for (int k = 0; k < kResampleTaps; ++k) {
                const int64_t j = j0 + k;
                if (j < 0 || j >= n) continue;
                const double wk = w[k];
                sum += (double)xp[k] * wk;
                wsum += wk;
            }
        }
        y[t] = wsum > 1e-10 ? (float)(sum / wsum) : 0.0f;
    }
}

}  // namespace

void launch_resample(const ResampleArgs &a, hipStream_t s) {
    if (a.n_wg <= 0) return;
    const bool lds_tab = a.up <= kResampleLdsRows;
    const size_t tab_bytes = lds_tab ? (size_t)a.up * kRowPitch * 8 + (size_t)((a.up + 1) & ~1) * 4 : 0;
    const size_t lds = tab_bytes + (size_t)a.span_cap * 4;
    if (lds_tab) hipLaunchKernelGGL(resample_kernel<true>, dim3((unsigned)a.n_wg), dim3(kResampleThreads), lds, s, a);
    else hipLaunchKernelGGL(resample_kernel<false>, dim3((unsigned)a.n_wg), dim3(kResampleThreads), lds, s, a);
}

}  // namespace pk
