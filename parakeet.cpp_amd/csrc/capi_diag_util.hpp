// parakeet.cpp_amd/csrc/capi_diag_util.hpp -- what the pk_diag_* translation units (capi_diag.cpp, capi_diag_gemm.cpp) share: the one set of
// helpers an operand is staged with on its way to the device and back, and the few checks and copies the product diagnostics repeat.
#pragma once
#include <algorithm>
#include <cstring>
#include <initializer_list>

#include "capi_util.hpp"
#include "dec_pack.hpp"

namespace pk {
namespace diag {

// What a word (fp32) / an element (bf16) nothing stored to holds: every output buffer is filled with it before the launch, every pad behind
// an operand row too (a NaN, so a kernel that reads a pad shows in its results).
constexpr uint32_t kDiagFill32 = PK_DIAG_MEL_FILL;
constexpr uint16_t kDiagFill16 = (uint16_t)(kDiagFill32 >> 16);

// The one way an operand is staged: its device buffer reserved and filled from the host.  src == nullptr (an optional operand the caller
// left out) only reserves the buffer.
inline void up(DevBuf &buf, const void *src, size_t bytes) {
    buf.reserve(bytes);
    if (src) PK_HIP(hipMemcpy(buf.p, src, bytes, hipMemcpyHostToDevice));
}
// ... rounded to bf16 on the host (nearest even), as the weights are at upload and as the producing kernels of the bf16 mode store activations
inline void up16(DevBuf &buf, const float *src, size_t n) {
    std::vector<uint16_t> h(n);
    for (size_t i = 0; i < n; ++i) h[i] = bf16_rne(src[i]);
    up(buf, h.data(), n * 2);
}
// ... several vectors of n floats one behind the other in one buffer (LayerNorm gamma / beta, ...); a null one leaves its slot unwritten
inline void up_rows(DevBuf &buf, std::initializer_list<const float *> rows, size_t n) {
    buf.reserve(rows.size() * n * 4);
    float *dst = buf.as<float>();
    for (const float *r : rows) {
        if (r) PK_HIP(hipMemcpy(dst, r, n * 4, hipMemcpyHostToDevice));
        dst += n;
    }
}
inline void down(void *dst, const DevBuf &buf, size_t bytes) { PK_HIP(hipMemcpy(dst, buf.p, bytes, hipMemcpyDeviceToHost)); }
// a bf16 array of the device, widened to fp32
inline void down16(float *dst, const DevBuf &buf, size_t n) {
    std::vector<uint16_t> h(n);
    down(h.data(), buf, n * 2);
    for (size_t i = 0; i < n; ++i) {
        const uint32_t u = (uint32_t)h[i] << 16;
        memcpy(&dst[i], &u, 4);
    }
}

// An output buffer of `words` 32-bit words (`n` bf16 elements), reserved and filled with the pattern.  A count of zero reserves one.
inline void filled(DevBuf &buf, int64_t words) {
    const size_t n = (size_t)std::max<int64_t>(words, 1);
    buf.reserve(n * 4);
    PK_HIP(hipMemsetD32(buf.p, kDiagFill32, n));
}
inline void filled16(DevBuf &buf, int64_t n_el) {
    const size_t n = (size_t)std::max<int64_t>(n_el, 1);
    buf.reserve(n * 2);
    PK_HIP(hipMemsetD16(buf.p, kDiagFill16, n));
}

// An fp32 operand at its pitch, the words of every row past `cols` replaced by the pattern
inline void up_padded(DevBuf &buf, const float *src, int64_t rows, int64_t cols, int64_t ld) {
    std::vector<float> h(src, src + (size_t)rows * ld);
    for (int64_t i = 0; i < rows; ++i)
        for (int64_t k = cols; k < ld; ++k) memcpy(&h[(size_t)i * ld + k], &kDiagFill32, 4);
    up(buf, h.data(), h.size() * 4);
}
// A bf16 operand at its pitch: rounded on the host, every element of a row past `cols` the pattern.  BLOCKED: in 32 x 16 blocks, the rows
// past `rows` (up to a multiple of 32) the pattern too; TILES8: in 8-row operand tiles (ld == cols: no padding).
enum Rows16 { ROWS16_ROW_MAJOR, ROWS16_BLOCKED, ROWS16_TILES8 };
inline void up16_padded(DevBuf &buf, const float *src, int64_t rows, int64_t cols, int64_t ld, Rows16 layout = ROWS16_ROW_MAJOR) {
    const int64_t prow = layout == ROWS16_BLOCKED ? (rows + 31) / 32 * 32 : rows;
    std::vector<uint16_t> h((size_t)prow * ld, kDiagFill16);
    for (int64_t i = 0; i < rows; ++i)
        for (int64_t k = 0; k < cols; ++k) {
            const size_t at = layout == ROWS16_BLOCKED ? (size_t)((i >> 5) * (ld >> 4) + (k >> 4)) * 512 + (size_t)(i & 31) * 16 + (size_t)(k & 15)
                            : layout == ROWS16_TILES8 ? (size_t)((i >> 3) * (ld >> 5) + (k >> 5)) * 256 + (size_t)((i & 7) + 8 * ((k >> 3) & 3)) * 8 + (size_t)(k & 7)
                                                      : (size_t)i * ld + k;
            h[at] = bf16_rne(src[(size_t)i * ld + k]);
        }
    up(buf, h.data(), h.size() * 2);
}

// LayerNorm gamma / beta of n columns, and (g2 / b2) those of a second norm, in one buffer -> where each lies on the device
struct NormVecs { const float *g, *b, *g2, *b2; };
inline NormVecs up_norms(DevBuf &buf, size_t n, const float *g, const float *b, const float *g2 = nullptr, const float *b2 = nullptr) {
    if (g2 || b2) up_rows(buf, {g, b, g2, b2}, n);
    else up_rows(buf, {g, b}, n);
    const float *p = buf.as<float>();
    return {p, p + n, p + 2 * n, p + 3 * n};
}

// The depthwise-conv tail of a GLU product over d channels: the depthwise weights [9][d], then the five per-channel vectors, in `par`;
// the caches are the caller's device buffers.
inline DwTail stage_dw_tail(DevBuf &par, size_t d, const float *dw_w, const float *dw_bias, const float *bn_mean, const float *bn_rstd, const float *bn_g,
                            const float *bn_b, const float *cache_in, float *cache_out, int has_cache, int c, int out_sigma = 0) {
    par.reserve((9 + 5) * d * 4);
    float *pp = par.as<float>();
    PK_HIP(hipMemcpy(pp, dw_w, 9 * d * 4, hipMemcpyHostToDevice));
    const float *five[5] = {dw_bias, bn_mean, bn_rstd, bn_g, bn_b};
    for (int i = 0; i < 5; ++i) PK_HIP(hipMemcpy(pp + (9 + i) * d, five[i], d * 4, hipMemcpyHostToDevice));
    return DwTail{cache_in, cache_out, has_cache, c, pp, pp + 9 * d, pp + 10 * d, pp + 11 * d, pp + 12 * d, pp + 13 * d, out_sigma};
}

// What the product diagnostics refuse about sigma_cols, and the copy of a diag struct's remap_* / sigma_cols into the launch arguments
inline void need_sigma_cols(int sigma_cols, int N) {
    need(sigma_cols >= 0 && sigma_cols % 16 == 0 && sigma_cols <= N, "sigma_cols: a multiple of 16, <= N");
}
template <class D>
void set_remap(GemmArgs &g, const D &d) {
    g.remap_rows = d.remap_rows; g.remap_gs = d.remap_gs; g.remap_rs = d.remap_rs; g.remap_cs = d.remap_cs;
    g.sigma_cols = d.sigma_cols;
}

// Every offset an M x N product may write lies inside an output of `cap` elements: remapped (remap_rows > 0), in 32-row blocks at pitch ldo
// (blocked_rows: the rows rounded up to 32), or row-major at pitch ldo.
inline void need_output_fits(int M, int N, int remap_rows, int64_t remap_gs, int64_t remap_rs, int64_t remap_cs, int64_t ldo, int64_t cap, bool blocked_rows = false) {
    if (remap_rows > 0) {
        need(remap_gs >= 0 && remap_rs >= 0 && remap_cs >= 0, "remap strides");
        const int64_t last = (int64_t)((M - 1) / remap_rows) * remap_gs + (int64_t)(std::min(M, remap_rows) - 1) * remap_rs + (int64_t)(N - 1) * remap_cs;
        need(last < cap, "out_words: the remapped output must fit");
    } else if (blocked_rows) {
        need((int64_t)((M + 31) / 32) * 32 * ldo <= cap, "out_words: the blocked output (rows rounded up to 32) must fit");
    } else {
        need(remap_rows == 0 && ldo >= N && (int64_t)(M - 1) * ldo + N <= cap, "ldo >= N, out_words >= (M - 1) ldo + N elements");
    }
}

// A form table through the (out, cap) listing of the pk_diag_*_forms entry points: fills what fits, returns the table's length
template <class T>
int copy_forms(const T *table, int n, int32_t *out, int cap) {
    for (int i = 0; out && i < n && i < cap; ++i) out[i] = (int32_t)table[i];
    return n;
}

}  // namespace diag
}  // namespace pk
