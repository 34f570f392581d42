// parakeet.cpp_amd/csrc/kernels/endpoint.hip -- endpointing on live audio: utterance boundaries from the log-mel rows a streaming push leaves on the
// device.
//
// The specification is tests/endpoint_ref.py (levels, sliding_floor, OnlineEndpoint); every level, floor and decision is compared bit for bit, every
// event exactly.  Frames are numbered from the session's last reset; the S streams are independent.
//
//   endpoint_chunk_kernel  ONE WORKGROUP of 4 waves per stream, over the call's n rows [t0, t0 + n):
//     1. level: wave w sums rows w, w + 4, ...: lane l adds bins l, l + 64, ... in ascending order from +0.0f (every load of a wave is 64 consecutive
//        floats of the row), then the 64 lane sums fold as a tree, l with l ^ 32, 16, 8, 4, 2, 1: lane 0's chain is (own + higher) at every level, the
//        specification's order.  Nothing in the order depends on S, n or the launch.
//     2. keys: LDS holds the keys of frames t0 - (W - 1) .. t0 + n - 1: the carried window in front (slot f % W of the stream's ring in global memory; a
//        frame before the reset is 0xFFFFFFFF, which a minimum ignores), the chunk's own keys behind it.
//     3. floor: log2(W) doubling passes between two LDS buffers leave m[j] = min key[j .. j + len) with len the largest power of two <= W; the floor of
//        chunk frame i is min(m[i], m[i + W - len]): the exact minimum of the W keys that end at the frame.  (A minimum of unsigned keys has no rounding:
//        any order gives the same bits.)  Then, one thread per frame: thr = fmaxf(abs_thr, floor + margin), speech0 = level > thr; the frame's key goes
//        into its ring slot (the last W frames of the chunk only: one writer per slot, and a chunk shorter than W writes its own slots alone).
//     4. rule: thread 0 walks the n decisions in order with the stream's five words of state in registers and stores the events as they are emitted
//        (at most one per frame, so n slots hold them), their number and the state.  Plain vector stores throughout.
//   endpoint_close_kernel  one workgroup per stream, a no-op where mask[s] == 0.
//
// Bounds: row element (s n + i) F + b with i < n, b < F; ring slot s W + f % W with f >= 0; LDS key index < W - 1 + n (a read past it is replaced by
// the identity); event slot s n + k with k < n; state word s 8 + j with j < 5; h / c element (l S + s) Hp + i with l < Ln, i < Hp.
//
// Code object (hipcc -O3 --offload-arch=gfx950, from the .s of -save-temps):
//   endpoint_chunk_kernel  24 VGPR 56 SGPR  LDS 0 B + 8 (W - 1 + n) + 8 n bytes dynamic  scratch 0 B; no spills
//   endpoint_close_kernel  11 VGPR 24 SGPR  LDS 0 B  scratch 0 B; no spills
//   (the dynamic LDS: 2.6 KiB for W = 300, n = 16; 16.0 KiB at the limits W = 1024, n = 512)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#include "kernels.hpp"

namespace pk {

// the order-preserving map fp32 -> uint32: a negative value has all its bits inverted, a non-negative one its sign bit set; a NaN is the largest key
__device__ __forceinline__ unsigned ep_key(float x) {
    const unsigned b = __float_as_uint(x);
    if ((b & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ep_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

__global__ __launch_bounds__(256) void endpoint_chunk_kernel(EndpointChunkArgs a) {
    extern __shared__ unsigned ep_lds[];                            // keys [2][W - 1 + n], speech0 [n], level [n]
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.n, F = a.F, W = a.W, t0 = a.t0, M = W - 1 + n;
    unsigned *src = ep_lds, *dst = ep_lds + M;
    int *sp = reinterpret_cast<int *>(ep_lds + 2 * M);
    float *lv = reinterpret_cast<float *>(sp + n);
    unsigned *ring = a.ring + (int64_t)s * W;

    for (int j = tid; j < W - 1; j += 256) {                         // the carried window
        const int f = t0 - (W - 1) + j;
        src[j] = f >= 0 ? ring[f % W] : 0xFFFFFFFFu;
    }
    const float *rows = a.rows + (int64_t)s * n * F;
    for (int i = wave; i < n; i += 4) {                              // the levels
        const float *r = rows + (int64_t)i * F;
        float acc = 0.0f;
        for (int b = lane; b < F; b += 64) acc = acc + r[b];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) acc = acc + __shfl_xor(acc, o);
        if (lane == 0) { lv[i] = acc; src[W - 1 + i] = ep_key(acc); }
    }
    __syncthreads();

    int len = 1;                                                    // src[j] = min key[j .. j + len)
    for (; 2 * len <= W; len *= 2) {
        for (int j = tid; j < M; j += 256) {
            const unsigned x = src[j], y = j + len < M ? src[j + len] : 0xFFFFFFFFu;
            dst[j] = x < y ? x : y;
        }
        __syncthreads();
        unsigned *t = src; src = dst; dst = t;
    }
    for (int i = tid; i < n; i += 256) {
        const unsigned x = src[i], y = src[i + W - len];
        const float fl = ep_unkey(x < y ? x : y), level = lv[i];
        const float thr = fmaxf(a.abs_thr, fl + a.margin);
        const int speech = level > thr ? 1 : 0;
        sp[i] = speech;
        if (i >= n - W) ring[(t0 + i) % W] = ep_key(level);
        const int64_t o = (int64_t)s * n + i;
        if (a.level) a.level[o] = level;
        if (a.floor) a.floor[o] = fl;
        if (a.speech0) a.speech0[o] = speech;
    }
    __syncthreads();

    if (tid == 0) {                                                 // the online rule over the chunk's frames, in order
        int *st = a.state + (int64_t)s * kEndpointStateWords;
        int in_utt = st[0], run_speech = st[1], run_sil = st[2], utt_start = st[3], last_speech = st[4], ne = 0;
        int4 *ev = a.ev + (int64_t)s * n;
        for (int i = 0; i < n; ++i) {
            const int f = t0 + i, speech = sp[i];
            if (!in_utt) {
                run_speech = speech ? run_speech + 1 : 0;
                if (run_speech == a.min_speech) {
                    in_utt = 1; utt_start = f - a.min_speech + 1; last_speech = f; run_sil = 0;
                    ev[ne++] = make_int4(1, utt_start, f, f);                               // START
                }
            } else {
                if (speech) { last_speech = f; run_sil = 0; } else ++run_sil;
                if (run_sil == a.min_silence) {
                    ev[ne++] = make_int4(2 | 1 << 8, utt_start, last_speech, f);            // END, SILENCE
                    in_utt = 0; run_speech = 0;
                } else if (f - utt_start + 1 == a.max_utterance) {
                    ev[ne++] = make_int4(2 | 2 << 8, utt_start, f, f);                      // END, MAX_LENGTH
                    in_utt = 0; run_speech = 0;
                }
            }
        }
        st[0] = in_utt; st[1] = run_speech; st[2] = run_sil; st[3] = utt_start; st[4] = last_speech;
        a.n_ev[s] = ne;
    }
}

__global__ __launch_bounds__(256) void endpoint_close_kernel(const unsigned char *mask, int S, float *h, float *c, int Ln, int Hp, int *token, int blank,
                                                             int *state) {
    const int s = blockIdx.x, tid = threadIdx.x;
    const unsigned m = mask[s];
    if ((m & 1u) && h) {
        for (int l = 0; l < Ln; ++l) {
            const int64_t row = ((int64_t)l * S + s) * Hp;
            for (int i = tid; i < Hp; i += 256) { h[row + i] = 0.0f; c[row + i] = 0.0f; }
        }
        if (tid == 0) token[s] = blank;
    }
    if ((m & 2u) && state && tid == 0) {
        int *st = state + (int64_t)s * kEndpointStateWords;
        st[0] = 0; st[1] = 0; st[2] = 0;
    }
}

void launch_endpoint_chunk(const EndpointChunkArgs &a, hipStream_t s) {
    if (a.S < 1 || a.n < 1 || a.n > kEndpointMaxFrames || a.F < 1 || a.F > kEndpointMaxBins || a.W < 1 || a.W > kEndpointMaxWindow || a.t0 < 0 ||
        a.min_speech < 1 || a.min_silence < 1 || a.max_utterance < a.min_speech + 1) {
        fprintf(stderr, "parakeet_amd: internal error: launch_endpoint_chunk outside the kernel's limits (S %d, n %d, F %d, W %d, t0 %d)\n", a.S, a.n, a.F,
                a.W, a.t0);
        abort();
    }
    const size_t lds = ((size_t)2 * (a.W - 1 + a.n) + 2 * (size_t)a.n) * 4;
    hipLaunchKernelGGL(endpoint_chunk_kernel, dim3(a.S), dim3(256), lds, s, a);
}

void launch_endpoint_close(const unsigned char *mask, int S, float *h, float *c, int Ln, int Hp, int *token, int blank, int *state, hipStream_t s) {
    hipLaunchKernelGGL(endpoint_close_kernel, dim3(S), dim3(256), 0, s, mask, S, h, c, Ln, Hp, token, blank, state);
}

}  // namespace pk
