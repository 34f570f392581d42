// parakeet.cpp_amd/csrc/dec_pack.hpp -- host-side layouts of the decode-loop weights (kernels/decode_gemv.hip, kernels/decode_gemv_bf16.hip).
// The loader (engine.cpp upload_weights) and the kernel-level diagnostic (capi_diag.cpp pk_diag_skinny_gemm) pack through these functions.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace pk {

// fp32 -> bf16, round to nearest even (what v_cvt_pk_bf16_f32 does to the activations on the device)
inline uint16_t bf16_rne(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// "sigma" K layout of the fp32 decode-loop operands (kernels/decode_gemv.hip): inside every block of 16 input features the
// 4x4 index matrix is transposed, so one float4 holds a lane's k = 4s+kq operands of four consecutive MFMA steps.
inline int dec_sigma(int k) { return (k & ~15) | ((k & 3) << 2) | ((k >> 2) & 3); }

inline std::vector<float> pack_sigma(const float *w, int rows, int K) {
    std::vector<float> p((size_t)rows * K);
    for (int r = 0; r < rows; ++r)
        for (int k = 0; k < K; ++k) p[(size_t)r * K + dec_sigma(k)] = w[(size_t)r * K + k];
    return p;
}

// bf16 decode weights (tolerance-class mode) in the LOAD ORDER of skinny_gemm_bf16_kernel: per (16-output tile, 32-k block) one 1 KB block
// [lane][8] -- lane (col = lane & 15, kq = lane >> 4) holds W[row(tile, col)][32 blk + 8 kq .. + 7], so a wave's load instruction reads 1 KB of
// consecutive addresses and a tile's weight stream is one contiguous run.  cell: the tile's columns are (gate, unit) pairs of the LSTM,
// row = (col >> 2) * Hp + 4 tile + (col & 3); otherwise row = 16 tile + col (clamped to the last row: the kernel never stores those columns).
// The values stay fp32 here; the caller rounds them to bf16 (Model::upload_gemm_weight).
inline std::vector<float> pack_dec16(const float *w, int rows, int K, bool cell) {
    const int n_tiles = cell ? rows / 16 : (rows + 15) / 16, nblk = K / 32, hp = rows / 4;
    std::vector<float> p((size_t)n_tiles * nblk * 512);
    for (int t = 0; t < n_tiles; ++t)
        for (int blk = 0; blk < nblk; ++blk)
            for (int lane = 0; lane < 64; ++lane) {
                const int col = lane & 15, kq = lane >> 4;
                int row = cell ? (col >> 2) * hp + 4 * t + (col & 3) : 16 * t + col;
                row = row < rows ? row : rows - 1;
                const float *src = w + (size_t)row * K + 32 * blk + 8 * kq;
                float *dst = p.data() + (((size_t)t * nblk + blk) * 64 + lane) * 8;
                for (int e = 0; e < 8; ++e) dst[e] = src[e];
            }
    return p;
}

}  // namespace pk
