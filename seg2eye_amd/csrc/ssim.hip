// Structural similarity (SSIM, Wang et al. 2004) of two single-channel image batches and its gradient: an 11-tap
// Gaussian window (sigma 1.5), "valid" placement, data range 1.  Separable: a workgroup stages one (T + 10)^2 tile in LDS, runs the
// horizontal 11-tap pass into LDS and the vertical pass per output.  Two launches forward (tiles, then the fold of the per-tile fp64
// partials: DESIGN 8 #3), one backward; launch shapes from (N, H, W) alone.
//
// Cancellation.  sigma^2 = E[u^2] - mu^2 loses everything in fp32 on a bright flat region.  The variances and the covariance do not
// change when a constant is subtracted from u and v, so every tile takes its moments about its own first pixel (cu, cv): the staged
// values are du = u - cu, formed from the loaded numbers BEFORE the map to [0, 1] ((x - xc) / 2: exact or one small relative
// rounding), and the means are put back as mu = cu + mean(du).  The backward does the same to the saved maps: with
// A' = A + 2 cu B + cv C the gradient is sum g (A') + 2 du sum g B + dv sum g C, three correlations of small numbers.
#include "ssim_tile.h"

namespace {

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

    ssim_stage_pair<In, T>(xs, ys, H, W, ty0, tx0, xc, yc, su, sv);
    __syncthreads();
    ssim_hpass5(su, sv, sh, win);
    __syncthreads();
    // vertical pass, S and its three derivatives: thread (ty, tx) serves rows ty and ty + 8
    const int tx = threadIdx.x & (SS_TW - 1), tyb = threadIdx.x / SS_TW;
    const size_t plane = (size_t)Ho * Wo;
    double acc = 0.0;
#pragma unroll
    for (int h = 0; h < SS_TH / 8; ++h) {
        const int ty = tyb + 8 * h, oy = ty0 + ty, ox = tx0 + tx;
        float m[5];
        ssim_vpass5(sh, ty, tx, win, m);
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
    const double s = block_sum4(acc, red);
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

    ssim_stage_maps(mA, mB, mC, Ho, Wo, py0, px0, cu, cv, sm);
    __syncthreads();
    ssim_hpass3(sm, sh, win);
    __syncthreads();
    const int tx = threadIdx.x & (SS_TW - 1), tyb = threadIdx.x / SS_TW;
    const float scale = gssim[n] / (float)plane * In::delta(1.f, 0.f);             // (du/dx = 1/2)
#pragma unroll
    for (int h = 0; h < SS_TH / 8; ++h) {
        const int ty = tyb + 8 * h, py = py0 + ty, px = px0 + tx;
        float s0, s1, s2;
        ssim_vpass3(sh, ty, tx, win, s0, s1, s2);
        if (py < H && px < W) {
            const size_t o = (size_t)py * W + px;
            const float du = In::delta(load1<T>(xs + o), xc), dv = In::delta(load1<T>(ys + o), yc);
            store1<T>(dx + (size_t)n * H * W + o, scale * fmaf(2.f * du, s1, fmaf(dv, s2, s0)));
        }
    }
}

// the size checks every entry shares, after its own pointer checks: S2E_ERR_UNSUPPORTED
int ssim_check_size(const char* name, int N, int H, int W) {
    if (H < SS_TAPS || W < SS_TAPS) S2E_FAIL(S2E_ERR_UNSUPPORTED, "%s: H=%d W=%d (an image smaller than the 11 x 11 window has no position)", name, H, W);
    return s2e_check_image_batch(name, N, H, W);           // (with N >= 1, N H W < 2^31 bounds the tiles of the grid.x too: tiles <= H W)
}

template <typename T>
int ssim_fwd_launch(const char* name, const T* x, const T* y, int N, int H, int W, float* ssim, float* maps, void* ws, size_t ws_bytes,
                    hipStream_t st) {
    if (const int rc = ssim_check_size(name, N, H, W)) return rc;
    S2E_CHECK_BYTES(name, "workspace", ws_bytes, s2e_ssim_workspace_bytes(N, H, W));
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
