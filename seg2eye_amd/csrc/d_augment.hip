// Differentiable augmentation of the discriminator's input: the (2N,H,W,8) [one-hot | image | 0] tensor of
// s2e_onehot_nhwc's cpad == 8 path, written through a per-sample colour / translation / cutout transform.  HBM- and launch-bound:
// one lane per pixel, the 8 channels as one (bf16) or two (fp32) 16-byte stores; the per-sample sums go through per-block fp64
// partials that the consuming launch folds.
#include "common.h"

constexpr int AUG_PPB = 2048;                             // pixels per partial-sum block: 8 per thread
constexpr int AUG_PMAX = 64;                              // partial sums per image at most (one wave folds them)

// partial sums per image (the grid.x of the sum launches, the fold length of the consuming ones)
static inline int aug_partials(long hw) { const long p = (hw + AUG_PPB - 1) / AUG_PPB; return (int)(p < 1 ? 1 : (p > AUG_PMAX ? AUG_PMAX : p)); }

// One parameter row [b, c, ty, tx, y0, x0, ch, cw] as the kernels use it.  The six integers arrive as floats: clamped to +-2^30 before
// the conversion (a NaN becomes a bound), and every comparison below runs in 64 bits, so no row can wrap a coordinate -- a pixel is read
// only after its source was found inside the image.
struct AugRow { float b, c; long long ty, tx, y0, x0, y1, x1; };
__device__ __forceinline__ long long aug_int(float v) { return (long long)fminf(fmaxf(v, -1073741824.f), 1073741824.f); }
__device__ __forceinline__ AugRow aug_row(const float* __restrict__ params, int n) {
    const float* p = params + (size_t)n * 8;
    AugRow r;
    r.b = p[0]; r.c = p[1];
    r.ty = aug_int(p[2]); r.tx = aug_int(p[3]);
    r.y0 = aug_int(p[4]); r.x0 = aug_int(p[5]);
    r.y1 = r.y0 + aug_int(p[6]); r.x1 = r.x0 + aug_int(p[7]);
    return r;
}
// output pixel (y, x): is it visible, and where is its source
__device__ __forceinline__ bool aug_visible(const AugRow& r, int y, int x, int H, int W, int& sy, int& sx) {
    const long long yy = (long long)y - r.ty, xx = (long long)x - r.tx;
    const bool inside = yy >= 0 && yy < H && xx >= 0 && xx < W;
    const bool cut = y >= r.y0 && y < r.y1 && x >= r.x0 && x < r.x1;
    sy = (int)yy; sx = (int)xx;
    return inside && !cut;
}

// sum of the P partials of image `img` in index order (fp64), the same value in every thread of the block
__device__ __forceinline__ double aug_fold(const double* __restrict__ part, int img, int P, double* sh) {
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < P; ++i) s += part[(size_t)img * P + i];
        sh[0] = s;
    }
    __syncthreads();
    return sh[0];
}

// ---------------------------------------------------------------------------------------- forward
// part[img][bx] = sum of image img's pixels bx, bx + P, ... (img < N: fake, else real), img = blockIdx.y
template <typename T>
__global__ __launch_bounds__(256) void aug_mean_kernel(const T* __restrict__ fake, const T* __restrict__ real, double* __restrict__ part,
                                                       int N, int hw) {
    __shared__ double sh[4];
    const int img = blockIdx.y;
    const T* src = (img < N ? fake + (size_t)img * hw : real + (size_t)(img - N) * hw);
    float a = 0.f;                                         // (a thread adds hw / (256 P) <= a few hundred values of one image: fp32, then fp64)
    double s = 0.0;
    int k = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < hw; i += gridDim.x * 256) {
        a += load1<T>(src + i);
        if (++k == 8) { s += (double)a; a = 0.f; k = 0; }
    }
    s = block_sum4(s + (double)a, sh);
    if (threadIdx.x == 0) part[(size_t)img * gridDim.x + blockIdx.x] = s;
}

// out (2N,H,W,8): image blockIdx.y, one lane per pixel.  COLOR: c * v + o with o = (1 - c) * mean + b folded from part; otherwise a copy.
template <typename T, bool COLOR>
__global__ __launch_bounds__(256) void aug_fwd_kernel(const uint8_t* __restrict__ label, const T* __restrict__ fake, const T* __restrict__ real,
        const float* __restrict__ params, const double* __restrict__ part, T* __restrict__ out, int N, int H, int W, int ncls, int P) {
    __shared__ double sh[1];
    const int img = blockIdx.y, n = img < N ? img : img - N, hw = H * W;
    const AugRow r = aug_row(params, n);
    float c = 1.f, o = -0.f;
    if constexpr (COLOR) {
        const double mean = aug_fold(part, img, P, sh) / (double)hw;
        c = r.c;
        o = (float)((1.0 - (double)r.c) * mean + (double)r.b);
        if (o == 0.f) o = -0.f;                             // v + (-0) == v for every v, -0 included: c == 1, b == 0 copies the source's bits
    }
    const uint8_t* lb = label + (size_t)n * hw;
    const T* src = (img < N ? fake : real) + (size_t)n * hw;
    T* dst = out + (size_t)img * hw * 8;
    for (int pix = blockIdx.x * 256 + threadIdx.x; pix < hw; pix += gridDim.x * 256) {
        const int y = pix / W, x = pix - y * W;
        int sy, sx;
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = 0.f;
        if (aug_visible(r, y, x, H, W, sy, sx)) {
            const int s = sy * W + sx;
            const int cls = lb[s];
            const float px = load1<T>(src + s);
            const float im = COLOR ? fmaf(c, px, o) : px;
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = k == ncls ? im : ((k < ncls && k == cls) ? 1.f : 0.f);
        }
        *(u32x4_t*)(dst + (size_t)pix * 8) = pack16<T>(v);
        if constexpr (Vec<T>::N == 4) *(u32x4_t*)(dst + (size_t)pix * 8 + 4) = pack16<T>(v + 4);
    }
}

// ---------------------------------------------------------------------------------------- backward
// part[n][bx] = sum over the visible output pixels bx, bx + P, ... of sample n of g[n, y, x, ncls]
template <typename T>
__global__ __launch_bounds__(256) void aug_gsum_kernel(const T* __restrict__ g, const float* __restrict__ params, double* __restrict__ part,
                                                       int H, int W, int ncls) {
    __shared__ double sh[4];
    const int n = blockIdx.y, hw = H * W;
    const AugRow r = aug_row(params, n);
    const T* gs = g + (size_t)n * hw * 8 + ncls;
    float a = 0.f;
    double s = 0.0;
    int k = 0;
    for (int pix = blockIdx.x * 256 + threadIdx.x; pix < hw; pix += gridDim.x * 256) {
        const int y = pix / W, x = pix - y * W;
        int sy, sx;
        if (aug_visible(r, y, x, H, W, sy, sx)) a += load1<T>(gs + (size_t)pix * 8);
        if (++k == 8) { s += (double)a; a = 0.f; k = 0; }
    }
    s = block_sum4(s + (double)a, sh);
    if (threadIdx.x == 0) part[(size_t)n * gridDim.x + blockIdx.x] = s;
}

// dfake[n, sy, sx] = c * g[n, sy + ty, sx + tx, ncls] where that output pixel is visible (else 0)  +  (1 - c) / (H W) * S_n
template <typename T, bool COLOR>
__global__ __launch_bounds__(256) void aug_bwd_kernel(const T* __restrict__ g, const float* __restrict__ params, const double* __restrict__ part,
                                                      T* __restrict__ dfake, int H, int W, int ncls, int P) {
    __shared__ double sh[1];
    const int n = blockIdx.y, hw = H * W;
    const AugRow r = aug_row(params, n);
    float c = 1.f, k = 0.f;
    if constexpr (COLOR) {
        c = r.c;
        k = (float)((1.0 - (double)r.c) / (double)hw * aug_fold(part, n, P, sh));
    }
    const T* gs = g + (size_t)n * hw * 8 + ncls;
    T* dst = dfake + (size_t)n * hw;
    for (int s = blockIdx.x * 256 + threadIdx.x; s < hw; s += gridDim.x * 256) {
        const int sy = s / W, sx = s - sy * W;
        const long long y = sy + r.ty, x = sx + r.tx;       // the one output pixel this source feeds
        const bool vis = y >= 0 && y < H && x >= 0 && x < W && !(y >= r.y0 && y < r.y1 && x >= r.x0 && x < r.x1);
        float v = 0.f;
        if (vis) v = load1<T>(gs + ((size_t)y * W + (size_t)x) * 8);
        store1<T>(dst + s, COLOR ? fmaf(c, v, k) : v);
    }
}

// blocks along the pixels of one image for the one-lane-per-pixel launches: ~4096 blocks over the `images` of the launch
static inline int aug_grid_x(long hw, int images) {
    const long want = (hw + 255) / 256, cap = 4096 / images;
    return (int)(want < cap ? want : (cap < 1 ? 1 : cap));
}

static int aug_check(const char* name, int dtype, bool ptrs, int N, int H, int W, int ncls, int cpad) {
    if (!ptrs || N <= 0 || H <= 0 || W <= 0 || ncls <= 0) S2E_FAIL(S2E_ERR_ARG, "%s: bad argument", name);
    S2E_CHECK_DTYPE(dtype, name);
    if (cpad != 8 || ncls >= 8) S2E_FAIL(S2E_ERR_UNSUPPORTED, "%s: cpad=%d ncls=%d (needs cpad == 8 and ncls < 8)", name, cpad, ncls);
    if (2L * N * H * W >= (1L << 31) || 2L * N > 65535) S2E_FAIL(S2E_ERR_UNSUPPORTED, "%s: too many pixels for 32-bit indices", name);
    return S2E_OK;
}

extern "C" size_t s2e_d_input_aug_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)2 * N * aug_partials((long)H * W) * sizeof(double);
}

extern "C" int s2e_d_input_aug(int dtype, const uint8_t* label, const void* fake, const void* real, const float* params, void* out,
                               double* ws, int N, int H, int W, int ncls, int cpad, int color, void* stream) {
    if (const int rc = aug_check("s2e_d_input_aug", dtype, label && fake && real && params && out && (ws || !color), N, H, W, ncls, cpad)) return rc;
    if ((uintptr_t)out & 15) S2E_FAIL(S2E_ERR_ARG, "s2e_d_input_aug: out must be 16-byte aligned");
    const int hw = H * W, P = aug_partials(hw);
    const dim3 grid(aug_grid_x(hw, 2 * N), 2 * N);
    hipStream_t st = (hipStream_t)stream;
    return s2e_with_dtype(dtype, "s2e_d_input_aug", [&](auto t) { using T = decltype(t);
        if (color) {
            aug_mean_kernel<T><<<dim3(P, 2 * N), 256, 0, st>>>((const T*)fake, (const T*)real, ws, N, hw);
            S2E_CHECK_LAUNCH("aug_mean_kernel");
            aug_fwd_kernel<T, true><<<grid, 256, 0, st>>>(label, (const T*)fake, (const T*)real, params, ws, (T*)out, N, H, W, ncls, P);
        } else {
            aug_fwd_kernel<T, false><<<grid, 256, 0, st>>>(label, (const T*)fake, (const T*)real, params, nullptr, (T*)out, N, H, W, ncls, P);
        }
        S2E_CHECK_LAUNCH("aug_fwd_kernel"); return S2E_OK; });
}

extern "C" int s2e_d_input_aug_bwd(int dtype, const void* gout, const float* params, void* dfake, double* ws,
                                   int N, int H, int W, int ncls, int cpad, int color, void* stream) {
    if (const int rc = aug_check("s2e_d_input_aug_bwd", dtype, gout && params && dfake && (ws || !color), N, H, W, ncls, cpad)) return rc;
    const int hw = H * W, P = aug_partials(hw);
    const dim3 grid(aug_grid_x(hw, N), N);
    hipStream_t st = (hipStream_t)stream;
    return s2e_with_dtype(dtype, "s2e_d_input_aug_bwd", [&](auto t) { using T = decltype(t);
        if (color) {
            aug_gsum_kernel<T><<<dim3(P, N), 256, 0, st>>>((const T*)gout, params, ws, H, W, ncls);
            S2E_CHECK_LAUNCH("aug_gsum_kernel");
            aug_bwd_kernel<T, true><<<grid, 256, 0, st>>>((const T*)gout, params, ws, (T*)dfake, H, W, ncls, P);
        } else {
            aug_bwd_kernel<T, false><<<grid, 256, 0, st>>>((const T*)gout, params, nullptr, (T*)dfake, H, W, ncls, P);
        }
        S2E_CHECK_LAUNCH("aug_bwd_kernel"); return S2E_OK; });
}
