// parakeet.cpp_amd/csrc/kernels/vad.hip -- energy voice-activity segmentation of a packed ragged batch of 16 kHz clips.
//
// The specification is tests/vad_ref.py, reproduced bit for bit.  A clip of n samples has F = ceil(n / 160) frames; a workgroup of 256 lanes owns one
// CHUNK of kVadRun = 256 consecutive frames of ONE clip (found by a binary search over the clips' first chunks, as in resample.hip), in every kernel:
//
//   vad_energy_kernel    e[f] = sum of x * x over the frame's 160 samples (zeros past n).  Eight lanes share a frame: lane l reads the five float4
//       at floats 4 * (l + 8 k), k = 0 .. 4, of the frame -- the eight lanes of a frame read 128 consecutive bytes per load and a clip starts on a
//       128-byte boundary of the staged buffer, so every load instruction takes whole cache lines and every sample is read once.  The lane adds its
//       20 squares in ascending sample order (fp32, no fused multiply-add), then the eight partial sums are added as a tree: lanes l and l ^ 4, then
//       l ^ 2, then l ^ 1.  Nothing in that order depends on the clip's place in the batch or on the launch.  The kernel also counts the top byte
//       of every key into the clip's first histogram.
//   vad_hist_kernel<P>   pass P = 1 .. 3 of the radix select: the keys that share the 8 P bits found so far are counted by their next byte.
//   vad_pick_kernel      one workgroup per clip: the bin of pass P that holds the wanted rank becomes the next byte of the key, the rank becomes
//       the rank inside that bin.  After pass 3 the key is the exact order statistic: the noise floor.
//   vad_decide_kernel    speech0 = e > fmaxf(abs_thr, floor * ratio).
//   vad_smooth_kernel<M> the three smoothing rules, one launch each.  All three ask, for every frame, for the nearest flagged frame at or before
//       it and at or after it: inside the chunk a max / min scan through LDS, across chunks the chunks' (first, last) flagged frames that the
//       previous launch left in global memory, searched outwards 256 chunks at a time until one is found.
//         M = 0  flags = speech0:     a non-speech frame between speech frames L < f < R with R - L - 1 < min_silence becomes speech;  writes NOT speech1
//         M = 1  flags = NOT speech1: a speech frame whose run (L + 1 .. R - 1) is shorter than min_speech becomes non-speech;         writes speech2
//         M = 2  flags = speech2:     a frame is covered when the run that ends at L, padded and snapped, reaches it, or the run that starts at R
//                                     does (padding is monotonic, so no farther run covers a frame the nearest does not);            writes speech3
//       Runs of speech3 are the padded runs with the overlapping and touching ones merged.
//   vad_count_kernel / vad_emit_kernel   run starts and run ends per chunk, then every chunk adds up the counts of the clip's chunks before it
//       and writes its starts and ends into the clip's slots; the clip's last chunk writes the number of runs.
//
// Bounds: a lane touches frame f of clip c only when f < F; x is read at in_off + j for j < n only (float4 loads only where j + 3 < n); the
// per-frame arrays are indexed frame_off + f, the per-chunk arrays by blockIdx.x < n_chunks; a clip has at most (F + 1) / 2 runs (maximal runs of
// a flag array are separated by at least one frame) and the emit kernel tests the slot against that capacity before it writes.
#include "kernels.hpp"

namespace pk {

namespace {

constexpr int kNone = 0x7fffffff;

__device__ __forceinline__ uint32_t vad_key(float e) { return e != e ? 0xffffffffu : __float_as_uint(e); }

struct VadChunk { VadClip c; int ci; int f0; int64_t chunk; };

// the clip and the first frame of this workgroup's chunk
__device__ __forceinline__ VadChunk vad_chunk(const VadArgs &a) {
    const int64_t k = blockIdx.x;
    int lo = 0, hi = a.n_clips - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.clip[mid].chunk0 <= k) lo = mid; else hi = mid - 1;
    }
    VadChunk r;
    r.c = a.clip[lo]; r.ci = lo; r.chunk = k;
    r.f0 = (int)(k - r.c.chunk0) * kVadRun;
    return r;
}

// adds the workgroup's 256 LDS bins to the clip's histogram of pass P
__device__ __forceinline__ void vad_flush_hist(const VadArgs &a, int ci, int pass, const uint32_t *bins) {
    const uint32_t v = bins[threadIdx.x];
    if (v) atomicAdd(a.hist + ((size_t)ci * 4 + pass) * 256 + threadIdx.x, v);
}

__global__ __launch_bounds__(kVadThreads) void vad_energy_kernel(VadArgs a) {
    __shared__ uint32_t bins[256];
    const int tid = threadIdx.x, l = tid & 7, g = tid >> 3;
    bins[tid] = 0;
    __syncthreads();
    const VadChunk ch = vad_chunk(a);
    const float *x = a.x + ch.c.in_off;
    const int64_t n = ch.c.n;
    for (int it = 0; it < kVadRun / 32; ++it) {
        const int f = ch.f0 + it * 32 + g;
        const bool live = f < ch.c.F;
        float4 v[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int64_t j = (int64_t)f * kVadFrame + 4 * (l + 8 * k);
            if (live && j + 3 < n) {
                v[k] = *reinterpret_cast<const float4 *>(x + j);
            } else {
                v[k].x = (live && j < n) ? x[j] : 0.0f;
                v[k].y = (live && j + 1 < n) ? x[j + 1] : 0.0f;
                v[k].z = (live && j + 2 < n) ? x[j + 2] : 0.0f;
                v[k].w = 0.0f;
            }
        }
        float acc = v[0].x * v[0].x;
        acc += v[0].y * v[0].y; acc += v[0].z * v[0].z; acc += v[0].w * v[0].w;
#pragma unroll
        for (int k = 1; k < 5; ++k) { acc += v[k].x * v[k].x; acc += v[k].y * v[k].y; acc += v[k].z * v[k].z; acc += v[k].w * v[k].w; }
        acc += __shfl_xor(acc, 4);
        acc += __shfl_xor(acc, 2);
        acc += __shfl_xor(acc, 1);
        if (live && l == 0) {
            a.energy[ch.c.frame_off + f] = acc;
            atomicAdd(&bins[vad_key(acc) >> 24], 1u);
        }
    }
    __syncthreads();
    vad_flush_hist(a, ch.ci, 0, bins);
}

template <int P>
__global__ __launch_bounds__(kVadThreads) void vad_hist_kernel(VadArgs a) {
    __shared__ uint32_t bins[256];
    const int tid = threadIdx.x;
    bins[tid] = 0;
    __syncthreads();
    const VadChunk ch = vad_chunk(a);
    const int f = ch.f0 + tid;
    if (f < ch.c.F) {
        const uint32_t key = vad_key(a.energy[ch.c.frame_off + f]);
        if ((key >> (32 - 8 * P)) == a.sel[ch.ci].prefix) atomicAdd(&bins[(key >> (24 - 8 * P)) & 255u], 1u);
    }
    __syncthreads();
    vad_flush_hist(a, ch.ci, P, bins);
}

// one workgroup per clip: bin t of pass `pass` holds the rank when (keys in the bins before t) <= rank < (... up to and including t)
__global__ __launch_bounds__(kVadThreads) void vad_pick_kernel(VadArgs a, int pass) {
    __shared__ uint32_t inc[256];
    const int tid = threadIdx.x, ci = blockIdx.x;
    const VadClip c = a.clip[ci];
    if (c.F <= 0) return;
    const uint32_t own = a.hist[((size_t)ci * 4 + pass) * 256 + tid];
    inc[tid] = own;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const uint32_t v = tid >= d ? inc[tid - d] : 0u;
        __syncthreads();
        inc[tid] += v;
        __syncthreads();
    }
    const uint32_t rank = pass == 0 ? (uint32_t)c.rank : a.sel[ci].rank;
    const uint32_t prefix = pass == 0 ? 0u : a.sel[ci].prefix;
    const uint32_t before = inc[tid] - own;
    __syncthreads();                                           // (every lane has read sel before the one below writes it)
    if (before <= rank && rank < inc[tid]) {
        VadSelect s;
        s.prefix = (prefix << 8) | (uint32_t)tid;
        s.rank = rank - before;
        a.sel[ci] = s;
    }
}

// leaves the chunk's first / last flagged frame (clip-relative) in first[chunk] / last[chunk]; every lane of the workgroup calls it
__device__ __forceinline__ void vad_summary(bool flag, int f, int F, int32_t *first, int32_t *last, int64_t chunk) {
    __shared__ int lo, hi;
    if (threadIdx.x == 0) { lo = F; hi = -1; }
    __syncthreads();
    if (flag) { atomicMin(&lo, f); atomicMax(&hi, f); }
    __syncthreads();
    if (threadIdx.x == 0) { first[chunk] = lo; last[chunk] = hi; }
}

__global__ __launch_bounds__(kVadThreads) void vad_decide_kernel(VadArgs a) {
    const VadChunk ch = vad_chunk(a);
    const int f = ch.f0 + threadIdx.x;
    const float floor_e = __uint_as_float(a.sel[ch.ci].prefix);
    const float thr = fmaxf(a.abs_thr, floor_e * a.ratio);
    bool sp = false;
    if (f < ch.c.F) {
        sp = a.energy[ch.c.frame_off + f] > thr;              // (false for a NaN energy)
        a.flag[0][ch.c.frame_off + f] = sp ? 1 : 0;
    }
    vad_summary(sp, f, ch.c.F, a.first[0], a.last[0], ch.chunk);
}

// L = the nearest flagged frame at or before f (-1: none in the clip), R = the nearest at or after f (F: none); every lane calls it
__device__ __forceinline__ void vad_nearest(bool flag, int f, const VadChunk &ch, const int32_t *first, const int32_t *last, int &L, int &R) {
    __shared__ int sl[kVadThreads], sr[kVadThreads];
    __shared__ int carry;
    const int tid = threadIdx.x;
    sl[tid] = flag ? f : -1;
    sr[tid] = flag ? f : kNone;
    __syncthreads();
    for (int d = 1; d < kVadThreads; d <<= 1) {
        const int vl = tid >= d ? sl[tid - d] : -1;
        const int vr = tid + d < kVadThreads ? sr[tid + d] : kNone;
        __syncthreads();
        sl[tid] = max(sl[tid], vl);
        sr[tid] = min(sr[tid], vr);
        __syncthreads();
    }
    L = sl[tid];
    R = sr[tid];
    const bool need_l = sl[0] < 0, need_r = sr[kVadThreads - 1] == kNone;   // workgroup-uniform
    const int64_t c_lo = ch.c.chunk0, c_hi = ch.c.chunk0 + (ch.c.F + kVadRun - 1) / kVadRun;   // the clip's chunks
    int cl = -1, cr = ch.c.F;
    if (need_l) {
        for (int64_t top = ch.chunk; top > c_lo; top -= kVadThreads) {       // chunks top - 256 .. top - 1
            if (tid == 0) carry = -1;
            __syncthreads();
            const int64_t k = top - 1 - tid;
            if (k >= c_lo) { const int v = last[k]; if (v >= 0) atomicMax(&carry, v); }
            __syncthreads();
            cl = carry;
            __syncthreads();
            if (cl >= 0) break;
        }
    }
    if (need_r) {
        for (int64_t bot = ch.chunk + 1; bot < c_hi; bot += kVadThreads) {   // chunks bot .. bot + 255
            if (tid == 0) carry = ch.c.F;
            __syncthreads();
            const int64_t k = bot + tid;
            if (k < c_hi) { const int v = first[k]; if (v < ch.c.F) atomicMin(&carry, v); }
            __syncthreads();
            cr = carry;
            __syncthreads();
            if (cr < ch.c.F) break;
        }
    }
    if (L < 0) L = cl;
    if (R == kNone) R = cr;
}

__device__ __forceinline__ int vad_pad_start(int s, int pad) { const int p = s - pad; return p <= 0 ? 0 : (p / kVadGrid) * kVadGrid; }
__device__ __forceinline__ int vad_pad_end(int e, int pad, int F) {
    const int64_t q = (int64_t)e + pad;
    const int p = q < F - 1 ? (int)q : F - 1;
    const int r = ((p + 1 + kVadGrid - 1) / kVadGrid) * kVadGrid - 1;
    return r < F - 1 ? r : F - 1;
}

template <int MODE>
__global__ __launch_bounds__(kVadThreads) void vad_smooth_kernel(VadArgs a) {
    constexpr int in = MODE & 1, out = in ^ 1;
    const VadChunk ch = vad_chunk(a);
    const int f = ch.f0 + threadIdx.x, F = ch.c.F;
    const bool live = f < F;
    const bool flag = live && a.flag[in][ch.c.frame_off + f] != 0;
    int L, R;
    vad_nearest(flag, f, ch, a.first[in], a.last[in], L, R);
    bool res = false;
    if (live) {
        if (MODE == 0) {            // flag = speech0; res = NOT speech1
            const bool speech1 = flag || (L >= 0 && R < F && R - L - 1 < a.min_silence);
            res = !speech1;
        } else if (MODE == 1) {     // flag = NOT speech1; res = speech2
            res = !flag && (R - 1) - (L + 1) + 1 >= a.min_speech;
        } else {                    // flag = speech2; res = speech3
            res = flag || (L >= 0 && vad_pad_end(L, a.pad, F) >= f) || (R < F && vad_pad_start(R, a.pad) <= f);
        }
        a.flag[out][ch.c.frame_off + f] = res ? 1 : 0;
    }
    if (MODE != 2) vad_summary(res, f, F, a.first[out], a.last[out], ch.chunk);
}

// is frame f the first / the last frame of a run of speech3 (flag[1])
__device__ __forceinline__ void vad_edges(const VadArgs &a, const VadChunk &ch, int f, bool &st, bool &en) {
    st = en = false;
    if (f >= ch.c.F) return;
    const uint8_t *d = a.flag[1] + ch.c.frame_off;
    if (!d[f]) return;
    st = f == 0 || !d[f - 1];
    en = f == ch.c.F - 1 || !d[f + 1];
}

__global__ __launch_bounds__(kVadThreads) void vad_count_kernel(VadArgs a) {
    __shared__ int ns, ne;
    if (threadIdx.x == 0) { ns = 0; ne = 0; }
    __syncthreads();
    const VadChunk ch = vad_chunk(a);
    bool st, en;
    vad_edges(a, ch, ch.f0 + threadIdx.x, st, en);
    if (st) atomicAdd(&ns, 1);
    if (en) atomicAdd(&ne, 1);
    __syncthreads();
    if (threadIdx.x == 0) { a.n_start[ch.chunk] = ns; a.n_end[ch.chunk] = ne; }
}

__global__ __launch_bounds__(kVadThreads) void vad_emit_kernel(VadArgs a) {
    __shared__ int ss[kVadThreads], se[kVadThreads];
    __shared__ int base_s, base_e;
    const int tid = threadIdx.x;
    if (tid == 0) { base_s = 0; base_e = 0; }
    const VadChunk ch = vad_chunk(a);
    const int f = ch.f0 + tid;
    bool st, en;
    vad_edges(a, ch, f, st, en);
    ss[tid] = st ? 1 : 0;
    se[tid] = en ? 1 : 0;
    __syncthreads();
    for (int d = 1; d < kVadThreads; d <<= 1) {
        const int vs = tid >= d ? ss[tid - d] : 0, ve = tid >= d ? se[tid - d] : 0;
        __syncthreads();
        ss[tid] += vs;
        se[tid] += ve;
        __syncthreads();
    }
    int ps = 0, pe = 0;                                        // starts / ends in the clip's chunks before this one
    for (int64_t k = ch.c.chunk0 + tid; k < ch.chunk; k += kVadThreads) { ps += a.n_start[k]; pe += a.n_end[k]; }
    if (ps) atomicAdd(&base_s, ps);
    if (pe) atomicAdd(&base_e, pe);
    __syncthreads();
    const int cap = (ch.c.F + 1) / 2;
    if (st) { const int slot = base_s + ss[tid] - 1; if (slot < cap) a.run_start[ch.c.run_off + slot] = f; }
    if (en) { const int slot = base_e + se[tid] - 1; if (slot < cap) a.run_end[ch.c.run_off + slot] = f; }
    if (tid == kVadThreads - 1 && ch.f0 + kVadRun >= ch.c.F) a.n_runs[ch.ci] = base_s + ss[tid];   // the clip's last chunk
}

}  // namespace

void launch_vad(const VadArgs &a, hipStream_t s) {
    if (a.n_chunks <= 0) return;
    const dim3 grid((unsigned)a.n_chunks), clips((unsigned)a.n_clips), block(kVadThreads);
    hipLaunchKernelGGL(vad_energy_kernel, grid, block, 0, s, a);
    hipLaunchKernelGGL(vad_pick_kernel, clips, block, 0, s, a, 0);
    hipLaunchKernelGGL(vad_hist_kernel<1>, grid, block, 0, s, a);
    hipLaunchKernelGGL(vad_pick_kernel, clips, block, 0, s, a, 1);
    hipLaunchKernelGGL(vad_hist_kernel<2>, grid, block, 0, s, a);
    hipLaunchKernelGGL(vad_pick_kernel, clips, block, 0, s, a, 2);
    hipLaunchKernelGGL(vad_hist_kernel<3>, grid, block, 0, s, a);
    hipLaunchKernelGGL(vad_pick_kernel, clips, block, 0, s, a, 3);
    hipLaunchKernelGGL(vad_decide_kernel, grid, block, 0, s, a);
    hipLaunchKernelGGL(vad_smooth_kernel<0>, grid, block, 0, s, a);
    hipLaunchKernelGGL(vad_smooth_kernel<1>, grid, block, 0, s, a);
    hipLaunchKernelGGL(vad_smooth_kernel<2>, grid, block, 0, s, a);
    hipLaunchKernelGGL(vad_count_kernel, grid, block, 0, s, a);
    hipLaunchKernelGGL(vad_emit_kernel, grid, block, 0, s, a);
}

}  // namespace pk
