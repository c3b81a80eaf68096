// What ssim.hip and msssim.hip share: the 11-tap window, the 16 x 32 tile, what a loaded number means
// and the two separable passes over a staged (T + 10)^2 tile, forward (five products) and backward (three maps).  Every LDS pass
// has a half-wave on 32 consecutive words of one row: no bank conflicts.
#pragma once
#include "common.h"

namespace {

constexpr int SS_TAPS = 11, SS_R = SS_TAPS - 1;             // window taps; rows / columns a window reaches past its first
constexpr int SS_TH = 16, SS_TW = 32;                        // outputs of one workgroup (256 threads: two rows of 32 each)
constexpr int SS_IH = SS_TH + SS_R, SS_IW = SS_TW + SS_R;    // the staged tile: 26 x 42
constexpr float SS_C1 = 0.01f * 0.01f, SS_C2 = 0.03f * 0.03f;

// the window, computed once on the host in fp64 and passed by value: the taps sit in scalar registers
struct SsimWin { float g[SS_TAPS]; };

// what a loaded number means: T in [-1, 1] -> u = (x + 1) / 2; uint8 0..255 -> u = a / 255.  centre: u of the tile's first pixel;
// delta: u - centre from the loaded numbers themselves.  (The numbers may be stored as another type than T: a 2 x 2 mean of uint8
// pixels is a float that still counts 0..255.)
template <typename T> struct SsimIn {
    static __device__ __forceinline__ float centre(float xc) { return (xc + 1.f) * 0.5f; }
    static __device__ __forceinline__ float delta(float x, float xc) { return (x - xc) * 0.5f; }
};
template <> struct SsimIn<uint8_t> {
    static __device__ __forceinline__ float centre(float xc) { return xc / 255.f; }
    static __device__ __forceinline__ float delta(float x, float xc) { return (x - xc) / 255.f; }
};

// stage the 26 x 42 tile whose first pixel is (ty0, tx0) of two H x W images stored as X, in In's units, about (xc, yc): rows of 42
// consecutive elements; past the image: zero, read by no valid output.  No barrier.
template <typename In, typename X>
__device__ __forceinline__ void ssim_stage_pair(const X* __restrict__ xs, const X* __restrict__ ys, int H, int W, int ty0, int tx0, float xc,
                                                float yc, float (&su)[SS_IH][SS_IW], float (&sv)[SS_IH][SS_IW]) {
    for (int i = threadIdx.x; i < SS_IH * SS_IW; i += 256) {
        const int r = i / SS_IW, c = i - r * SS_IW, gy = ty0 + r, gx = tx0 + c;
        float du = 0.f, dv = 0.f;
        if (gy < H && gx < W) {
            const size_t o = (size_t)gy * W + gx;
            du = In::delta(load1<X>(xs + o), xc);
            dv = In::delta(load1<X>(ys + o), yc);
        }
        su[r][c] = du; sv[r][c] = dv;
    }
}

// forward, horizontal: the five products of every staged row at the 32 output columns (a half-wave reads 32 consecutive words).  No barrier.
__device__ __forceinline__ void ssim_hpass5(const float (&su)[SS_IH][SS_IW], const float (&sv)[SS_IH][SS_IW], float (&sh)[5][SS_IH][SS_TW],
                                            const SsimWin& win) {
    for (int i = threadIdx.x; i < SS_IH * SS_TW; i += 256) {
        const int r = i / SS_TW, c = i - r * SS_TW;
        float mu = 0.f, mv = 0.f, uu = 0.f, vv = 0.f, uv = 0.f;
#pragma unroll
        for (int k = 0; k < SS_TAPS; ++k) {
            const float a = su[r][c + k], b = sv[r][c + k], w = win.g[k];
            const float wa = w * a, wb = w * b;
            mu += wa; mv += wb;
            uu = fmaf(wa, a, uu); vv = fmaf(wb, b, vv); uv = fmaf(wa, b, uv);
        }
        sh[0][r][c] = mu; sh[1][r][c] = mv; sh[2][r][c] = uu; sh[3][r][c] = vv; sh[4][r][c] = uv;
    }
}

// forward, vertical: the five window means of output (ty, tx) of the tile
__device__ __forceinline__ void ssim_vpass5(const float (&sh)[5][SS_IH][SS_TW], int ty, int tx, const SsimWin& win, float (&m)[5]) {
#pragma unroll
    for (int j = 0; j < 5; ++j) m[j] = 0.f;
#pragma unroll
    for (int k = 0; k < SS_TAPS; ++k) {
        const float w = win.g[k];
#pragma unroll
        for (int j = 0; j < 5; ++j) m[j] = fmaf(w, sh[j][ty + k][tx], m[j]);
    }
}

// backward, horizontal: pixel column c takes tap k from the position k columns to its left (staged column c + 10 - k).  No barrier.
__device__ __forceinline__ void ssim_hpass3(const float (&sm)[3][SS_IH][SS_IW], float (&sh)[3][SS_IH][SS_TW], const SsimWin& win) {
    for (int i = threadIdx.x; i < SS_IH * SS_TW; i += 256) {
        const int r = i / SS_TW, c = i - r * SS_TW;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < SS_TAPS; ++k) {
            const float w = win.g[k];
            s0 = fmaf(w, sm[0][r][c + SS_R - k], s0);
            s1 = fmaf(w, sm[1][r][c + SS_R - k], s1);
            s2 = fmaf(w, sm[2][r][c + SS_R - k], s2);
        }
        sh[0][r][c] = s0; sh[1][r][c] = s1; sh[2][r][c] = s2;
    }
}

// backward, vertical: the three correlations at pixel (ty, tx) of the tile
__device__ __forceinline__ void ssim_vpass3(const float (&sh)[3][SS_IH][SS_TW], int ty, int tx, const SsimWin& win, float& s0, float& s1,
                                            float& s2) {
    s0 = 0.f; s1 = 0.f; s2 = 0.f;
#pragma unroll
    for (int k = 0; k < SS_TAPS; ++k) {
        const float w = win.g[k];
        s0 = fmaf(w, sh[0][ty + SS_R - k][tx], s0);
        s1 = fmaf(w, sh[1][ty + SS_R - k][tx], s1);
        s2 = fmaf(w, sh[2][ty + SS_R - k][tx], s2);
    }
}

// stage the saved maps of one image for the backward: position (r, c) of the tile = (py0 - 10 + r, px0 - 10 + c), zero outside the
// Ho x Wo valid map; A' = A + 2 cu B + cv C.  No barrier.
__device__ __forceinline__ void ssim_stage_maps(const float* __restrict__ mA, const float* __restrict__ mB, const float* __restrict__ mC, int Ho,
                                                int Wo, int py0, int px0, float cu, float cv, float (&sm)[3][SS_IH][SS_IW]) {
    for (int i = threadIdx.x; i < SS_IH * SS_IW; i += 256) {
        const int r = i / SS_IW, c = i - r * SS_IW, qy = py0 - SS_R + r, qx = px0 - SS_R + c;
        float a = 0.f, b = 0.f, cc = 0.f;
        if (qy >= 0 && qy < Ho && qx >= 0 && qx < Wo) {
            const size_t o = (size_t)qy * Wo + qx;
            b = mB[o]; cc = mC[o];
            a = fmaf(2.f * cu, b, fmaf(cv, cc, mA[o]));
        }
        sm[0][r][c] = a; sm[1][r][c] = b; sm[2][r][c] = cc;
    }
}

inline SsimWin ssim_window() {
    double g[SS_TAPS], sum = 0.0;
    for (int i = 0; i < SS_TAPS; ++i) { const double d = i - SS_R / 2; g[i] = exp(-d * d / (2.0 * 1.5 * 1.5)); sum += g[i]; }
    SsimWin w;
    for (int i = 0; i < SS_TAPS; ++i) w.g[i] = (float)(g[i] / sum);
    return w;
}

// tiles of an h x w field (the outputs forward, the input pixels backward)
inline long ssim_tiles_x(int w) { return (w + SS_TW - 1) / SS_TW; }
inline long ssim_tiles(int h, int w) { return (long)((h + SS_TH - 1) / SS_TH) * ssim_tiles_x(w); }

}  // namespace
