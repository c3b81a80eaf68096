// Region-aware reconstruction error: the statistics {count, sum |d|, sum d^2} of d = x - y per image and label class, the
// class-balanced loss built from them, and its gradient.  A segmented reduction keyed by a uint8 label map that may be of another size
// than the images (validation: 640 x 400 images, the network's label): pixel (r, c) has class label[(r Hl) / H, (c Wl) / W], integers.
// Two launches forward (per-block, per-class fp64 partial records written with plain stores; one fold that adds them in index order and
// writes the statistics, the loss and the per-class gradient coefficients), one element-wise launch backward.  HBM- and launch-bound:
// 16-byte loads per lane where the image starts on a 16-byte boundary, single elements otherwise; no atomics, the same input gives the
// same bits; launch shapes from (N, H, W, Hl, Wl, ncls) alone.  A class >= ncls matches no accumulator and no coefficient: a label is
// only ever COMPARED, never used as an index.
#include "common.h"

namespace {

constexpr int RG_MAXC = 8;                                  // classes at most: the accumulators of a lane sit in registers
constexpr int RG_PPB = 4096;                                // pixels of one block: 16 per thread, one to four 16-byte loads per image

// elements of T in 16 bytes (Vec<T>::N of common.h, and 16 for the uint8 entry)
template <typename T> struct RgVec { static constexpr int N = 16 / (int)sizeof(T); };

template <typename T> __device__ __forceinline__ void rg_unpack(u32x4_t r, float* f) { unpack16<T>(r, f); }
template <> __device__ __forceinline__ void rg_unpack<uint8_t>(u32x4_t r, float* f) {
    const uint32_t w[4] = {r[0], r[1], r[2], r[3]};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f[4 * j] = (float)(w[j] & 0xffu); f[4 * j + 1] = (float)((w[j] >> 8) & 0xffu);
        f[4 * j + 2] = (float)((w[j] >> 16) & 0xffu); f[4 * j + 3] = (float)(w[j] >> 24);
    }
}

// where the class of an image pixel is read: image n's label plane and the integer nearest-below map onto it
struct RgLabel {
    const uint8_t* lb;
    int H, W, Hl, Wl;
    bool ident, small;                                      // same size: the pixel's own index; small: r Hl and c Wl fit 32 bits
    __device__ __forceinline__ int at(int p) const {
        if (ident) return lb[p];
        const unsigned r = (unsigned)p / (unsigned)W, c = (unsigned)p - r * (unsigned)W;
        unsigned lr, lc;
        if (small) { lr = r * (unsigned)Hl / (unsigned)H; lc = c * (unsigned)Wl / (unsigned)W; }
        else { lr = (unsigned)((unsigned long long)r * (unsigned)Hl / (unsigned)H); lc = (unsigned)((unsigned long long)c * (unsigned)Wl / (unsigned)W); }
        return lb[(size_t)lr * Wl + lc];                    // lr < Hl, lc < Wl because r < H, c < W
    }
};
__device__ __forceinline__ RgLabel rg_label(const uint8_t* label, int n, int H, int W, int Hl, int Wl, int small) {
    return RgLabel{label + (size_t)n * Hl * Wl, H, W, Hl, Wl, Hl == H && Wl == W, small != 0};
}

// V consecutive pixels g .. g + V - 1 of one image, values and classes: one 16-byte load per image where the image is aligned (`vec`)
// and the group lies inside the block's range, single elements otherwise.  A pixel at or past `end` reads nothing and gets class
// 255, which no accumulator and no coefficient matches.
template <typename T, int V>
__device__ __forceinline__ void rg_load(const T* xs, const T* ys, const RgLabel& L, int g, int end, bool vec, float* a, float* b, int* l) {
    if (vec && g + V <= end) {
        rg_unpack<T>(*(const u32x4_t*)(xs + g), a);
        rg_unpack<T>(*(const u32x4_t*)(ys + g), b);
#pragma unroll
        for (int j = 0; j < V; ++j) l[j] = L.at(g + j);
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const bool in = g + j < end;
            a[j] = in ? load1<T>(xs + g + j) : 0.f;
            b[j] = in ? load1<T>(ys + g + j) : 0.f;
            l[j] = in ? L.at(g + j) : 255;
        }
    }
}

// ---------------------------------------------------------------------------------------- forward: partial records
// grid (blocks along the image, N).  part[n][block][c][3] = {count, sum |d|, sum d^2} of the block's pixels of class c < ncls.
// d, |d| and d^2 are fp32 from the loaded values (exact integers for uint8); every sum over pixels is fp64.
template <typename T>
__global__ __launch_bounds__(256) void region_part_kernel(const T* __restrict__ x, const T* __restrict__ y, const uint8_t* __restrict__ label,
                                                          double* __restrict__ part, int H, int W, int Hl, int Wl, int ncls, int small) {
    __shared__ double red[4][RG_MAXC][3];
    constexpr int V = RgVec<T>::N;
    const int n = blockIdx.y, hw = H * W;
    const int p0 = blockIdx.x * RG_PPB, end = min(p0 + RG_PPB, hw);
    const T* xs = x + (size_t)n * hw;
    const T* ys = y + (size_t)n * hw;
    const RgLabel L = rg_label(label, n, H, W, Hl, Wl, small);
    const bool vec = (((uintptr_t)xs | (uintptr_t)ys) & 15) == 0;       // (p0 is a multiple of 4096 elements: the block keeps the image's alignment)
    double cnt[RG_MAXC], s1[RG_MAXC], s2[RG_MAXC];
#pragma unroll
    for (int c = 0; c < RG_MAXC; ++c) { cnt[c] = 0.0; s1[c] = 0.0; s2[c] = 0.0; }
    for (int g = p0 + (int)threadIdx.x * V; g < end; g += 256 * V) {
        float a[V], b[V];
        int l[V];
        rg_load<T, V>(xs, ys, L, g, end, vec, a, b, l);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float d = a[j] - b[j];
            const double ad = (double)fabsf(d), sq = (double)(d * d);
#pragma unroll
            for (int c = 0; c < RG_MAXC; ++c) {
                const bool m = l[j] == c;
                cnt[c] += m ? 1.0 : 0.0;
                s1[c] += m ? ad : 0.0;
                s2[c] += m ? sq : 0.0;
            }
        }
    }
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < RG_MAXC; ++c) {
        if (c < ncls) {
            const double t0 = wave_sum(cnt[c]), t1 = wave_sum(s1[c]), t2 = wave_sum(s2[c]);
            if ((threadIdx.x & 63) == 0) { red[wave][c][0] = t0; red[wave][c][1] = t1; red[wave][c][2] = t2; }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < ncls * 3) {                                  // the four waves in order
        const int c = threadIdx.x / 3, k = threadIdx.x - 3 * c;
        part[((size_t)n * gridDim.x + blockIdx.x) * (ncls * 3) + threadIdx.x] = ((red[0][c][k] + red[1][c][k]) + red[2][c][k]) + red[3][c][k];
    }
}

// ---------------------------------------------------------------------------------------- forward: the fold
// One wave.  Thread (c, k) adds image after image the B partials of its entry in index order, writes stats[n][c][k] and keeps the
// batch's total; with `weights` thread 0 then forms  loss = sum_present w_c m_c / sum_present w_c,  m_c = F_c / n_c,  and
// coef[c] = w_c / (n_c sum_present w)  (0 for an absent class, and for all when no weighted class is present), in fp64, stored as fp32.
__global__ __launch_bounds__(64) void region_fold_kernel(const double* __restrict__ part, int N, int B, int ncls, int norm,
                                                         const float* __restrict__ weights, double* __restrict__ stats,
                                                         float* __restrict__ loss, float* __restrict__ coef) {
    __shared__ double tot[RG_MAXC][3];
    const int per = ncls * 3, t = threadIdx.x;
    if (t < per) {
        double total = 0.0;
        for (int n = 0; n < N; ++n) {
            const double* p = part + (size_t)n * B * per + t;
            double s = 0.0;
#pragma unroll 8
            for (int b = 0; b < B; ++b) s += p[(size_t)b * per];
            stats[(size_t)n * per + t] = s;
            total += s;
        }
        tot[t / 3][t % 3] = total;
    }
    if (!weights) return;
    __syncthreads();
    if (t != 0) return;
    const int kf = norm == 0 ? 1 : 2;
    double sw = 0.0, acc = 0.0;
    for (int c = 0; c < ncls; ++c)
        if (tot[c][0] > 0.0) { sw += (double)weights[c]; acc += (double)weights[c] * (tot[c][kf] / tot[c][0]); }
    const bool any = sw > 0.0;
    loss[0] = any ? (float)(acc / sw) : 0.f;
    for (int c = 0; c < ncls; ++c) coef[c] = (any && tot[c][0] > 0.0) ? (float)((double)weights[c] / (tot[c][0] * sw)) : 0.f;
}

// ---------------------------------------------------------------------------------------- backward
// grid as the partial kernel's.  dx[p] = (g k_l) f'(d):  f' = sign(d) (0 at d == 0; a NaN d stays NaN) for l1, 2 d for l2;  k_l = 0 for a
// class >= ncls.
template <typename T>
__global__ __launch_bounds__(256) void region_bwd_kernel(const T* __restrict__ x, const T* __restrict__ y, const uint8_t* __restrict__ label,
                                                         const float* __restrict__ coef, const float* __restrict__ gloss, T* __restrict__ dx,
                                                         int H, int W, int Hl, int Wl, int ncls, int norm, int small) {
    constexpr int V = RgVec<T>::N;
    const int n = blockIdx.y, hw = H * W;
    const int p0 = blockIdx.x * RG_PPB, end = min(p0 + RG_PPB, hw);
    const T* xs = x + (size_t)n * hw;
    const T* ys = y + (size_t)n * hw;
    T* ds = dx + (size_t)n * hw;
    const RgLabel L = rg_label(label, n, H, W, Hl, Wl, small);
    const bool vec = (((uintptr_t)xs | (uintptr_t)ys | (uintptr_t)ds) & 15) == 0;
    const float g = gloss[0];
    float k[RG_MAXC];
#pragma unroll
    for (int c = 0; c < RG_MAXC; ++c) k[c] = c < ncls ? g * coef[c] : 0.f;
    for (int i = p0 + (int)threadIdx.x * V; i < end; i += 256 * V) {
        float a[V], b[V], v[V];
        int l[V];
        rg_load<T, V>(xs, ys, L, i, end, vec, a, b, l);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float d = a[j] - b[j];
            float kk = 0.f;
#pragma unroll
            for (int c = 0; c < RG_MAXC; ++c) kk = l[j] == c ? k[c] : kk;
            const float f = norm == 0 ? (d != d ? d : (float)((d > 0.f) - (d < 0.f))) : 2.f * d;
            v[j] = kk * f;
        }
        if (vec && i + V <= end) {
            *(u32x4_t*)(ds + i) = pack16<T>(v);
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j)
                if (i + j < end) store1<T>(ds + i + j, v[j]);
        }
    }
}

// ---------------------------------------------------------------------------------------- host
inline long rg_blocks(long hw) { return (hw + RG_PPB - 1) / RG_PPB; }

// the checks every entry shares, after its own pointer / dtype / norm checks: S2E_ERR_UNSUPPORTED
int region_check_size(const char* name, int N, int H, int W, int Hl, int Wl, int ncls) {
    if (ncls < 1 || ncls > RG_MAXC) S2E_FAIL(S2E_ERR_UNSUPPORTED, "%s: ncls=%d (1 to 8 classes)", name, ncls);
    if (H < 1 || W < 1 || Hl < 1 || Wl < 1) S2E_FAIL(S2E_ERR_UNSUPPORTED, "%s: H=%d W=%d Hl=%d Wl=%d (every size must be at least 1)", name, H, W, Hl, Wl);
    if (N > 65535 || (long)H * W > (1L << 24) || (long)N * H * W >= (1L << 31))
        S2E_FAIL(S2E_ERR_UNSUPPORTED, "%s: N=%d H=%d W=%d is beyond the launch limits (N <= 65535, H W <= 2^24, N H W < 2^31)", name, N, H, W);
    return S2E_OK;
}
inline int rg_small(int H, int W, int Hl, int Wl) { return (long)H * Hl < (1L << 32) && (long)W * Wl < (1L << 32); }

template <typename T>
int region_fwd_launch(const char* name, const T* x, const T* y, const uint8_t* label, int N, int H, int W, int Hl, int Wl, int ncls, int norm,
                      const float* weights, double* stats, float* loss, float* coef, void* ws, size_t ws_bytes, hipStream_t st) {
    if (const int rc = region_check_size(name, N, H, W, Hl, Wl, ncls)) return rc;
    S2E_CHECK_BYTES(name, "workspace", ws_bytes, s2e_region_workspace_bytes(N, H, W, ncls));
    const int B = (int)rg_blocks((long)H * W);
    region_part_kernel<T><<<dim3(B, N), 256, 0, st>>>(x, y, label, (double*)ws, H, W, Hl, Wl, ncls, rg_small(H, W, Hl, Wl));
    S2E_CHECK_LAUNCH("region_part_kernel");
    region_fold_kernel<<<1, 64, 0, st>>>((const double*)ws, N, B, ncls, norm, weights, stats, loss, coef);
    S2E_CHECK_LAUNCH("region_fold_kernel");
    return S2E_OK;
}

}  // namespace

extern "C" size_t s2e_region_workspace_bytes(int N, int H, int W, int ncls) {
    if (N <= 0 || H < 1 || W < 1 || ncls < 1 || ncls > RG_MAXC) return 0;
    return (size_t)N * (size_t)rg_blocks((long)H * W) * (size_t)ncls * 3 * sizeof(double);
}

extern "C" int s2e_region_loss_fwd(int dtype, const void* x, const void* y, const uint8_t* label, int N, int H, int W, int Hl, int Wl, int ncls,
                                   int norm, const float* weights, double* stats, float* loss, float* coef, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    if (!x || !y || !label || !weights || !stats || !loss || !coef || !workspace || N <= 0) S2E_FAIL(S2E_ERR_ARG, "s2e_region_loss_fwd: bad argument");
    S2E_CHECK_DTYPE(dtype, "s2e_region_loss_fwd");
    if (norm != S2E_REGION_L1 && norm != S2E_REGION_L2) S2E_FAIL(S2E_ERR_ARG, "s2e_region_loss_fwd: bad norm %d", norm);
    return s2e_with_dtype(dtype, "s2e_region_loss_fwd", [&](auto t) { using T = decltype(t);
        return region_fwd_launch<T>("s2e_region_loss_fwd", (const T*)x, (const T*)y, label, N, H, W, Hl, Wl, ncls, norm, weights, stats, loss, coef,
                                    workspace, workspace_bytes, (hipStream_t)stream); });
}

extern "C" int s2e_region_stats_u8(const uint8_t* a, const uint8_t* b, const uint8_t* label, int N, int H, int W, int Hl, int Wl, int ncls,
                                   double* stats, void* workspace, size_t workspace_bytes, void* stream) {
    if (!a || !b || !label || !stats || !workspace || N <= 0) S2E_FAIL(S2E_ERR_ARG, "s2e_region_stats_u8: bad argument");
    return region_fwd_launch<uint8_t>("s2e_region_stats_u8", a, b, label, N, H, W, Hl, Wl, ncls, S2E_REGION_L1, nullptr, stats, nullptr, nullptr,
                                      workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int s2e_region_loss_bwd(int dtype, const void* x, const void* y, const uint8_t* label, const float* coef, const float* gloss,
                                   int N, int H, int W, int Hl, int Wl, int ncls, int norm, void* dx, void* stream) {
    if (!x || !y || !label || !coef || !gloss || !dx || N <= 0) S2E_FAIL(S2E_ERR_ARG, "s2e_region_loss_bwd: bad argument");
    S2E_CHECK_DTYPE(dtype, "s2e_region_loss_bwd");
    if (norm != S2E_REGION_L1 && norm != S2E_REGION_L2) S2E_FAIL(S2E_ERR_ARG, "s2e_region_loss_bwd: bad norm %d", norm);
    if (const int rc = region_check_size("s2e_region_loss_bwd", N, H, W, Hl, Wl, ncls)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int B = (int)rg_blocks((long)H * W);
    return s2e_with_dtype(dtype, "s2e_region_loss_bwd", [&](auto t) { using T = decltype(t);
        region_bwd_kernel<T><<<dim3(B, N), 256, 0, st>>>((const T*)x, (const T*)y, label, coef, gloss, (T*)dx, H, W, Hl, Wl, ncls, norm,
                                                         rg_small(H, W, Hl, Wl));
        S2E_CHECK_LAUNCH("region_bwd_kernel"); return S2E_OK; });
}
