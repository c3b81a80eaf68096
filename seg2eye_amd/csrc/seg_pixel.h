// What the eye segmenter's kernels share (segment.hip, seg_loss.hip): the load forms of a pixel's logits, the pixel's
// softmax terms, the checks every logits entry makes in the order the header states, and the dispatch over dtype and load form.
#pragma once
#include "common.h"

namespace {

constexpr int SEG_MAX_CLS = 16;
constexpr int SEG_THREADS = 256;
constexpr long SEG_MAX_PIXELS = 2147483647L;                // N H W (and N Ho Wo, P) at most: pixel indices are formed in 32-bit pieces

// One lane per pixel; the ncls <= 16 logits of a pixel are one vector load where the channel pitch allows it
//   PITCH4  C == 4: 8 bytes of bf16, 16 bytes of fp32        PITCH8  bf16, C == 8: 16 bytes        ANY  ncls scalar loads
// (the vector forms need the tensor aligned to the pixel's bytes; the launcher looks and takes ANY otherwise).  Channels at and past
// ncls are loaded with the vector but never enter a result: every use is behind `c < ncls`.
enum { SEG_ANY = 0, SEG_PITCH4 = 1, SEG_PITCH8 = 2 };
template <int MODE> struct SegSlots { static constexpr int N = MODE == SEG_PITCH4 ? 4 : MODE == SEG_PITCH8 ? 8 : SEG_MAX_CLS; };

// the logits of pixel p: z[c] for c < ncls, -inf behind them (so that a maximum or an argmax never sees a pad channel)
template <typename T, int MODE>
__device__ __forceinline__ void seg_load(const T* __restrict__ x, size_t p, int C, int ncls, float* z) {
    constexpr int NS = SegSlots<MODE>::N;
    if constexpr (MODE == SEG_PITCH4 && std::is_same<T, float>::value) {
        float f[4];
        unpack16<float>(*(const u32x4_t*)(x + p * 4), f);
#pragma unroll
        for (int c = 0; c < 4; ++c) z[c] = c < ncls ? f[c] : -INFINITY;
    } else if constexpr (MODE == SEG_PITCH4) {
        const u32x2_t r = *(const u32x2_t*)(x + p * 4);
        const uint32_t r0 = r[0], r1 = r[1];
        const float f[4] = {bf16_bits_to_f32(r0 & 0xffffu), __builtin_bit_cast(float, r0 & 0xffff0000u),
                            bf16_bits_to_f32(r1 & 0xffffu), __builtin_bit_cast(float, r1 & 0xffff0000u)};
#pragma unroll
        for (int c = 0; c < 4; ++c) z[c] = c < ncls ? f[c] : -INFINITY;
    } else if constexpr (MODE == SEG_PITCH8) {
        float f[8];
        unpack16<bf16_t>(*(const u32x4_t*)(x + p * 8), f);
#pragma unroll
        for (int c = 0; c < 8; ++c) z[c] = c < ncls ? f[c] : -INFINITY;
    } else {
        const T* px = x + p * (size_t)C;
#pragma unroll
        for (int c = 0; c < NS; ++c) z[c] = c < ncls ? load1<T>(px + (c < ncls ? c : 0)) : -INFINITY;
    }
}

// d[c] for c < ncls and zeros up to the pitch, as the pixel's vector
template <typename T, int MODE>
__device__ __forceinline__ void seg_store(T* __restrict__ y, size_t p, int C, int ncls, const float* d) {
    constexpr int NS = SegSlots<MODE>::N;
    if constexpr (MODE == SEG_PITCH4 && std::is_same<T, float>::value) {
        *(u32x4_t*)(y + p * 4) = pack16<float>(d);
    } else if constexpr (MODE == SEG_PITCH4) {
        *(u32x2_t*)(y + p * 4) = u32x2_t{pack2_bf16(d[0], d[1]), pack2_bf16(d[2], d[3])};
    } else if constexpr (MODE == SEG_PITCH8) {
        *(u32x4_t*)(y + p * 8) = pack16<bf16_t>(d);
    } else {
        T* py = y + p * (size_t)C;
#pragma unroll
        for (int c = 0; c < NS; ++c)
            if (c < ncls) store1<T>(py + c, d[c]);
        for (int c = ncls; c < C; ++c) store1<T>(py + c, 0.f);
    }
}

// max_c z, e[c] = exp(z[c] - max) (0 behind ncls), -> sum_c e[c]
template <int NS>
__device__ __forceinline__ float seg_softmax_terms(const float* z, int ncls, float& m, float* e) {
    m = z[0];
#pragma unroll
    for (int c = 1; c < NS; ++c) m = fmaxf(m, z[c]);        // (the slots behind ncls hold -inf)
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < NS; ++c) { e[c] = c < ncls ? expf(z[c] - m) : 0.f; s += e[c]; }
    return s;
}

// the checks every logits entry shares after its own pointer check, in the order the header states
int seg_check(const char* name, int dtype, int N, int H, int W, int C, int ncls) {
    S2E_CHECK_DTYPE(dtype, name);
    if (N < 1 || H < 1 || W < 1) S2E_FAIL(S2E_ERR_ARG, "%s: N=%d H=%d W=%d (every size must be at least 1)", name, N, H, W);
    if (ncls < 1 || ncls > SEG_MAX_CLS) S2E_FAIL(S2E_ERR_UNSUPPORTED, "%s: ncls=%d (1 to %d classes)", name, ncls, SEG_MAX_CLS);
    if (C < ncls) S2E_FAIL(S2E_ERR_ARG, "%s: channel pitch C=%d is below ncls=%d", name, C, ncls);
    if ((long)N * H * W > SEG_MAX_PIXELS) S2E_FAIL(S2E_ERR_UNSUPPORTED, "%s: N=%d H=%d W=%d is beyond the index limit (N H W <= 2^31 - 1)", name, N, H, W);
    return S2E_OK;
}

// the load form of a tensor: the vector forms where the pitch fits one and the base is aligned to the pixel's bytes
int seg_mode(int dtype, int C, const void* a, const void* b = nullptr) {
    const size_t esz = dtype == S2E_BF16 ? 2 : 4;
    const uintptr_t bits = (uintptr_t)a | (uintptr_t)b;
    if (C == 4 && (bits & (4 * esz - 1)) == 0) return SEG_PITCH4;
    if (C == 8 && dtype == S2E_BF16 && (bits & 15) == 0) return SEG_PITCH8;
    return SEG_ANY;
}

// f(T{}, int_c<MODE>{}) for the dtype and the load form
template <typename F> int seg_dispatch(int dtype, int mode, const char* name, F&& f) {
    return s2e_with_dtype(dtype, name, [&](auto t) { using T = decltype(t);
        if (mode == SEG_PITCH4) return f(T{}, int_c<SEG_PITCH4>{});
        if constexpr (std::is_same<T, bf16_t>::value) { if (mode == SEG_PITCH8) return f(T{}, int_c<SEG_PITCH8>{}); }
        return f(T{}, int_c<SEG_ANY>{}); });
}

}  // namespace
