// Structural similarity (SSIM, Wang et al. 2004) of two single-channel image batches and its gradient: an 11-tap
// Gaussian window (sigma 1.5), "valid" placement, data range 1.  Separable: a workgroup stages one (T + 10)^2 tile in LDS, runs the
// horizontal 11-tap pass into LDS and the vertical pass per output.  Two launches forward (tiles, then a fold of the per-tile fp64
// partial sums in index order), one backward; no atomics, launch shapes from (N, H, W) alone, the same input gives the same bits.
//
// Cancellation.  sigma^2 = E[u^2] - mu^2 loses everything in fp32 on a bright flat region.  The variances and the covariance do not
// change when a constant is subtracted from u and v, so every tile takes its moments about its own first pixel (cu, cv): the staged
// values are du = u - cu, formed from the loaded numbers BEFORE the map to [0, 1] ((x - xc) / 2: exact or one small relative
// rounding), and the means are put back as mu = cu + mean(du).  The backward does the same to the saved maps: with
// A' = A + 2 cu B + cv C the gradient is sum g (A') + 2 du sum g B + dv sum g C, three correlations of small numbers.
#include "common.h"

namespace {

constexpr int SS_TAPS = 11, SS_R = SS_TAPS - 1;             // window taps; rows / columns a window reaches past its first
constexpr int SS_TH = 16, SS_TW = 32;                        // outputs of one workgroup (256 threads: two rows of 32 each)
constexpr int SS_IH = SS_TH + SS_R, SS_IW = SS_TW + SS_R;    // the staged tile: 26 x 42
constexpr float SS_C1 = 0.01f * 0.01f, SS_C2 = 0.03f * 0.03f;

// the window, computed once on the host in fp64 and passed by value: the taps sit in scalar registers
struct SsimWin { float g[SS_TAPS]; };

// what a loaded number means: T in [-1, 1] -> u = (x + 1) / 2; uint8 0..255 -> u = a / 255.  centre: u of the tile's first pixel;
// delta: u - centre from the loaded numbers themselves
template <typename T> struct SsimIn {
    static __device__ __forceinline__ float centre(float xc) { return (xc + 1.f) * 0.5f; }
    static __device__ __forceinline__ float delta(float x, float xc) { return (x - xc) * 0.5f; }
};
template <> struct SsimIn<uint8_t> {
    static __device__ __forceinline__ float centre(float xc) { return xc / 255.f; }
    static __device__ __forceinline__ float delta(float x, float xc) { return (x - xc) / 255.f; }
};

// the block's sum of v (fp64), valid in thread 0: lanes by shuffles, then the four waves in order
__device__ __forceinline__ double ssim_block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// ---------------------------------------------------------------------------------------- forward
// grid (tiles, N).  part[n][tile] = sum of S over the tile's valid positions; maps (when not null): A = dS/dmu_u, B = dS/dE[u^2],
// C = dS/dE[uv] per position, three (N, H - 10, W - 10) fp32 planes one after the other.
template <typename T>
__global__ __launch_bounds__(256) void ssim_fwd_kernel(const T* __restrict__ x, const T* __restrict__ y, SsimWin win, double* __restrict__ part,
                                                       float* __restrict__ maps, int N, int H, int W, int tiles_x) {
    __shared__ float su[SS_IH][SS_IW], sv[SS_IH][SS_IW];
    __shared__ float sh[5][SS_IH][SS_TW];
    __shared__ double red[4];
    using In = SsimIn<T>;
    const int n = blockIdx.y, tile = blockIdx.x;
    const int ty0 = (tile / tiles_x) * SS_TH, tx0 = (tile % tiles_x) * SS_TW;      // first output = first input pixel of the tile: inside the image
    const int Ho = H - SS_R, Wo = W - SS_R;
    const T* xs = x + (size_t)n * H * W;
    const T* ys = y + (size_t)n * H * W;
    const float xc = load1<T>(xs + (size_t)ty0 * W + tx0), yc = load1<T>(ys + (size_t)ty0 * W + tx0);
    const float cu = In::centre(xc), cv = In::centre(yc);

    for (int i = threadIdx.x; i < SS_IH * SS_IW; i += 256) {                       // rows of 42 consecutive elements
        const int r = i / SS_IW, c = i - r * SS_IW, gy = ty0 + r, gx = tx0 + c;
        float du = 0.f, dv = 0.f;                                                  // past the image: read by no valid output
        if (gy < H && gx < W) {
            const size_t o = (size_t)gy * W + gx;
            du = In::delta(load1<T>(xs + o), xc);
            dv = In::delta(load1<T>(ys + o), yc);
        }
        su[r][c] = du; sv[r][c] = dv;
    }
    __syncthreads();
    // horizontal pass: the five products of every staged row at the 32 output columns (a half-wave reads 32 consecutive words)
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
    __syncthreads();
    // vertical pass, S and its three derivatives: thread (ty, tx) serves rows ty and ty + 8
    const int tx = threadIdx.x & (SS_TW - 1), tyb = threadIdx.x / SS_TW;
    const size_t plane = (size_t)Ho * Wo;
    double acc = 0.0;
#pragma unroll
    for (int h = 0; h < SS_TH / 8; ++h) {
        const int ty = tyb + 8 * h, oy = ty0 + ty, ox = tx0 + tx;
        float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < SS_TAPS; ++k) {
            const float w = win.g[k];
#pragma unroll
            for (int j = 0; j < 5; ++j) m[j] = fmaf(w, sh[j][ty + k][tx], m[j]);
        }
        if (oy < Ho && ox < Wo) {
            const float su2 = m[2] - m[0] * m[0], sv2 = m[3] - m[1] * m[1], suv = m[4] - m[0] * m[1];   // about (cu, cv): small numbers
            const float mu = cu + m[0], mv = cv + m[1];
            const float a1 = 2.f * mu * mv + SS_C1, a2 = 2.f * suv + SS_C2;
            const float b1 = mu * mu + mv * mv + SS_C1, b2 = su2 + sv2 + SS_C2;
            const float inv = 1.f / (b1 * b2);
            const float S = a1 * a2 * inv;
            acc += (double)S;
            if (maps) {
                // S = f(mu_u, mu_v, su2, sv2, suv):  B = f_su2 = -S / b2,  C = f_suv = 2 a1 / (b1 b2),
                // f_mu_u = 2 (mu_v b1 - mu_u a1) / b1^2 * a2 / b2 with mu_v b1 - mu_u a1 = (mu_v - mu_u) (mu_v (mu_u + mu_v) + C1) (no
                // cancellation left), and through su2 = E[u^2] - mu_u^2, suv = E[uv] - mu_u mu_v:  A = f_mu_u - 2 mu_u B - mu_v C
                const float B = -S / b2, C = 2.f * a1 * inv;
                const float dm = (m[1] - m[0]) + (cv - cu);
                const float fmu = 2.f * dm * (mv * (mu + mv) + SS_C1) / (b1 * b1) * (a2 / b2);
                const float A = fmu - 2.f * mu * B - mv * C;
                const size_t o = (size_t)n * plane + (size_t)oy * Wo + ox;
                maps[o] = A;
                maps[(size_t)N * plane + o] = B;
                maps[2 * (size_t)N * plane + o] = C;
            }
        }
    }
    const double s = ssim_block_sum(acc, red);
    if (threadIdx.x == 0) part[(size_t)n * gridDim.x + tile] = s;
}

// ssim[n] = (sum of image n's partials, in index order) / positions; one thread per image adds, the loads run ahead of it
__global__ __launch_bounds__(64) void ssim_fold_kernel(const double* __restrict__ part, int tiles, double positions, float* __restrict__ ssim) {
    if (threadIdx.x != 0) return;
    const double* p = part + (size_t)blockIdx.x * tiles;
    double s = 0.0;
#pragma unroll 8
    for (int i = 0; i < tiles; ++i) s += p[i];
    ssim[blockIdx.x] = (float)(s / positions);
}

// ---------------------------------------------------------------------------------------- backward
// grid (tiles over the INPUT pixels, N).  dx[n, p] = gssim[n] / positions * du/dx * sum_q g(p - q) (A(q) + 2 u(p) B(q) + v(p) C(q)),
// q over the window positions that cover p (q = p - 10 .. p on both axes, zero outside the valid map).
template <typename T>
__global__ __launch_bounds__(256) void ssim_bwd_kernel(const T* __restrict__ x, const T* __restrict__ y, const float* __restrict__ maps,
                                                       const float* __restrict__ gssim, SsimWin win, T* __restrict__ dx,
                                                       int N, int H, int W, int tiles_x) {
    __shared__ float sm[3][SS_IH][SS_IW];
    __shared__ float sh[3][SS_IH][SS_TW];
    using In = SsimIn<T>;
    const int n = blockIdx.y, tile = blockIdx.x;
    const int py0 = (tile / tiles_x) * SS_TH, px0 = (tile % tiles_x) * SS_TW;      // first pixel of the tile: inside the image
    const int Ho = H - SS_R, Wo = W - SS_R;
    const size_t plane = (size_t)Ho * Wo;
    const T* xs = x + (size_t)n * H * W;
    const T* ys = y + (size_t)n * H * W;
    const float xc = load1<T>(xs + (size_t)py0 * W + px0), yc = load1<T>(ys + (size_t)py0 * W + px0);
    const float cu = In::centre(xc), cv = In::centre(yc);
    const float* mA = maps + (size_t)n * plane;
    const float* mB = mA + (size_t)N * plane;
    const float* mC = mB + (size_t)N * plane;

    for (int i = threadIdx.x; i < SS_IH * SS_IW; i += 256) {                       // staged position (r, c) = (py0 - 10 + r, px0 - 10 + c)
        const int r = i / SS_IW, c = i - r * SS_IW, qy = py0 - SS_R + r, qx = px0 - SS_R + c;
        float a = 0.f, b = 0.f, cc = 0.f;
        if (qy >= 0 && qy < Ho && qx >= 0 && qx < Wo) {
            const size_t o = (size_t)qy * Wo + qx;
            b = mB[o]; cc = mC[o];
            a = fmaf(2.f * cu, b, fmaf(cv, cc, mA[o]));                            // A' = A + 2 cu B + cv C
        }
        sm[0][r][c] = a; sm[1][r][c] = b; sm[2][r][c] = cc;
    }
    __syncthreads();
    // horizontal pass: pixel column c takes tap k from the position k columns to its left (staged column c + 10 - k)
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
    __syncthreads();
    const int tx = threadIdx.x & (SS_TW - 1), tyb = threadIdx.x / SS_TW;
    const float scale = gssim[n] / (float)plane * In::delta(1.f, 0.f);             // (du/dx = 1/2)
#pragma unroll
    for (int h = 0; h < SS_TH / 8; ++h) {
        const int ty = tyb + 8 * h, py = py0 + ty, px = px0 + tx;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < SS_TAPS; ++k) {
            const float w = win.g[k];
            s0 = fmaf(w, sh[0][ty + SS_R - k][tx], s0);
            s1 = fmaf(w, sh[1][ty + SS_R - k][tx], s1);
            s2 = fmaf(w, sh[2][ty + SS_R - k][tx], s2);
        }
        if (py < H && px < W) {
            const size_t o = (size_t)py * W + px;
            const float du = In::delta(load1<T>(xs + o), xc), dv = In::delta(load1<T>(ys + o), yc);
            store1<T>(dx + (size_t)n * H * W + o, scale * fmaf(2.f * du, s1, fmaf(dv, s2, s0)));
        }
    }
}

SsimWin ssim_window() {
    double g[SS_TAPS], sum = 0.0;
    for (int i = 0; i < SS_TAPS; ++i) { const double d = i - SS_R / 2; g[i] = exp(-d * d / (2.0 * 1.5 * 1.5)); sum += g[i]; }
    SsimWin w;
    for (int i = 0; i < SS_TAPS; ++i) w.g[i] = (float)(g[i] / sum);
    return w;
}

// tiles of an h x w field (the outputs forward, the input pixels backward)
inline long ssim_tiles_x(int w) { return (w + SS_TW - 1) / SS_TW; }
inline long ssim_tiles(int h, int w) { return (long)((h + SS_TH - 1) / SS_TH) * ssim_tiles_x(w); }

// the size checks every entry shares, after its own pointer checks: S2E_ERR_UNSUPPORTED
int ssim_check_size(const char* name, int N, int H, int W) {
    if (H < SS_TAPS || W < SS_TAPS) S2E_FAIL(S2E_ERR_UNSUPPORTED, "%s: H=%d W=%d (an image smaller than the 11 x 11 window has no position)", name, H, W);
    if (N > 65535 || (long)N * H * W >= (1L << 31) || ssim_tiles(H, W) >= (1L << 31))
        S2E_FAIL(S2E_ERR_UNSUPPORTED, "%s: N=%d H=%d W=%d is beyond the launch limits (N <= 65535, N H W < 2^31)", name, N, H, W);
    return S2E_OK;
}

template <typename T>
int ssim_fwd_launch(const char* name, const T* x, const T* y, int N, int H, int W, float* ssim, float* maps, void* ws, size_t ws_bytes,
                    hipStream_t st) {
    if (const int rc = ssim_check_size(name, N, H, W)) return rc;
    if (ws_bytes < s2e_ssim_workspace_bytes(N, H, W)) S2E_FAIL(S2E_ERR_ARG, "%s: workspace of %zu bytes, needs %zu", name, ws_bytes, s2e_ssim_workspace_bytes(N, H, W));
    const int Ho = H - SS_R, Wo = W - SS_R, tiles = (int)ssim_tiles(Ho, Wo);
    ssim_fwd_kernel<T><<<dim3(tiles, N), 256, 0, st>>>(x, y, ssim_window(), (double*)ws, maps, N, H, W, (int)ssim_tiles_x(Wo));
    S2E_CHECK_LAUNCH("ssim_fwd_kernel");
    ssim_fold_kernel<<<N, 64, 0, st>>>((const double*)ws, tiles, (double)Ho * (double)Wo, ssim);
    S2E_CHECK_LAUNCH("ssim_fold_kernel");
    return S2E_OK;
}

}  // namespace

extern "C" size_t s2e_ssim_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || H < SS_TAPS || W < SS_TAPS) return 0;
    return (size_t)N * (size_t)ssim_tiles(H - SS_R, W - SS_R) * sizeof(double);
}

extern "C" int s2e_ssim_fwd(int dtype, const void* x, const void* y, int N, int H, int W, float* ssim, float* maps, void* workspace,
                            size_t workspace_bytes, void* stream) {
    if (!x || !y || !ssim || !workspace || N <= 0) S2E_FAIL(S2E_ERR_ARG, "s2e_ssim_fwd: bad argument");
    S2E_CHECK_DTYPE(dtype, "s2e_ssim_fwd");
    return s2e_with_dtype(dtype, "s2e_ssim_fwd", [&](auto t) { using T = decltype(t);
        return ssim_fwd_launch<T>("s2e_ssim_fwd", (const T*)x, (const T*)y, N, H, W, ssim, maps, workspace, workspace_bytes, (hipStream_t)stream); });
}

extern "C" int s2e_ssim_u8(const uint8_t* a, const uint8_t* b, int N, int H, int W, float* ssim, void* workspace, size_t workspace_bytes,
                           void* stream) {
    if (!a || !b || !ssim || !workspace || N <= 0) S2E_FAIL(S2E_ERR_ARG, "s2e_ssim_u8: bad argument");
    return ssim_fwd_launch<uint8_t>("s2e_ssim_u8", a, b, N, H, W, ssim, nullptr, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int s2e_ssim_bwd(int dtype, const void* x, const void* y, const float* maps, const float* gssim, int N, int H, int W, void* dx,
                            void* stream) {
    if (!x || !y || !maps || !gssim || !dx || N <= 0) S2E_FAIL(S2E_ERR_ARG, "s2e_ssim_bwd: bad argument");
    S2E_CHECK_DTYPE(dtype, "s2e_ssim_bwd");
    if (const int rc = ssim_check_size("s2e_ssim_bwd", N, H, W)) return rc;
    hipStream_t st = (hipStream_t)stream;
    return s2e_with_dtype(dtype, "s2e_ssim_bwd", [&](auto t) { using T = decltype(t);
        ssim_bwd_kernel<T><<<dim3((int)ssim_tiles(H, W), N), 256, 0, st>>>((const T*)x, (const T*)y, maps, gssim, ssim_window(), (T*)dx,
                                                                           N, H, W, (int)ssim_tiles_x(W));
        S2E_CHECK_LAUNCH("ssim_bwd_kernel"); return S2E_OK; });
}
