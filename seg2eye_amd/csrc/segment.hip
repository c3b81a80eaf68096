// The eye segmenter's three memory-bound pieces: the weighted softmax cross-entropy of NHWC logits against a uint8 label
// map with its gradient, the uint8 mask of bilinearly resized logits, and the confusion matrix of two masks.
//
// One lane per pixel; the ncls <= 16 logits of a pixel are one vector load where the channel pitch allows it
//   PITCH4  C == 4: 8 bytes of bf16, 16 bytes of fp32        PITCH8  bf16, C == 8: 16 bytes        ANY  ncls scalar loads
// (the vector forms need the tensor aligned to the pixel's bytes; the launcher looks and takes ANY otherwise).  Channels at and past
// ncls are loaded with the vector but never enter a result: every use is behind `c < ncls`.
//
// s2e_seg_ce_fwd    two launches: per-workgroup fp64 partials {sum w (lse - z_l), sum w} with plain stores, then one workgroup folds them
//                   in index order.  The launch shape follows from N H W alone, nothing is atomic: the same input gives the same bits.
// s2e_seg_ce_bwd    one launch; the softmax is recomputed, g and the denominator are read from device memory.
// s2e_seg_argmax_u8 one launch; the four taps of an output pixel are four pixel loads, the resized logits live in registers only.
// s2e_seg_confusion_u8  one launch; a workgroup counts into ncls^2 LDS words (a lane merges runs of equal (truth, pred) pairs of its
//                   16 consecutive pixels first: masks are piecewise constant) and adds its non-zero cells with one 64-bit integer
//                   atomic each.  Integer sums do not depend on their order.
#include "seg_pixel.h"

namespace {

constexpr int SEG_CE_BLOCKS = 512;                          // workgroups (and partial pairs) of the forward at most: two per CU
constexpr int SEG_CE_DEPTH = 4;                             // pixels of a lane whose loads are in flight together in the forward
constexpr int SEG_CONF_BLOCKS = 256;                        // one per CU: a workgroup ends with up to ncls^2 atomics on the same few cells

// ---------------------------------------------------------------------------------------- cross-entropy
// grid (blocks <= SEG_CE_BLOCKS), 256 threads, a grid-stride walk of the P pixels.  part[2 b] = the workgroup's sum of w (lse - z_l),
// part[2 b + 1] = its sum of w, over the pixels whose label is < ncls.
template <typename T, int MODE>
__global__ __launch_bounds__(SEG_THREADS) void seg_ce_fwd_kernel(const T* __restrict__ x, const uint8_t* __restrict__ label, const float* __restrict__ weights,
                                                                 long P, int C, int ncls, double* __restrict__ part) {
    constexpr int NS = SegSlots<MODE>::N;
    __shared__ float sw[SEG_MAX_CLS];
    __shared__ double red[2][SEG_THREADS / 64];
    if (threadIdx.x < SEG_MAX_CLS) sw[threadIdx.x] = (int)threadIdx.x < ncls ? weights[threadIdx.x] : 0.f;
    __syncthreads();
    double num = 0.0, den = 0.0;
    // SEG_CE_DEPTH pixels of a lane per step, their label and logits loads all issued before the first is used: at two waves per SIMD
    // the walk is bound by load latency, not by bytes.  A pixel past P re-reads pixel P - 1 and counts as ignored.
    const long stride = (long)gridDim.x * SEG_THREADS;
    for (long p0 = (long)blockIdx.x * SEG_THREADS + threadIdx.x; p0 < P; p0 += SEG_CE_DEPTH * stride) {
        int l[SEG_CE_DEPTH];
        float z[SEG_CE_DEPTH][NS];
#pragma unroll
        for (int u = 0; u < SEG_CE_DEPTH; ++u) {
            const long p = p0 + u * stride;
            const long pc = p < P ? p : P - 1;
            l[u] = p < P ? (int)label[pc] : 255;
            seg_load<T, MODE>(x, (size_t)pc, C, ncls, z[u]);
        }
#pragma unroll
        for (int u = 0; u < SEG_CE_DEPTH; ++u) {
            if (l[u] >= ncls) continue;                      // ignored: 255 and every other value that names no class
            float e[NS], m;
            const float s = seg_softmax_terms<NS>(z[u], ncls, m, e);
            float zl = z[u][0];
#pragma unroll
            for (int c = 1; c < NS; ++c) zl = c == l[u] ? z[u][c] : zl;
            const double w = (double)sw[l[u]];
            num += w * ((double)logf(s) - (double)(zl - m)); // lse - z_l = log(sum) - (z_l - max)
            den += w;
        }
    }
    num = wave_sum(num);
    den = wave_sum(den);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][wave] = num; red[1][wave] = den; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int i = 0; i < SEG_THREADS / 64; ++i) { a += red[0][i]; b += red[1][i]; }
        part[2 * (size_t)blockIdx.x] = a;
        part[2 * (size_t)blockIdx.x + 1] = b;
    }
}

// loss = (sum of the numerators, in index order) / (sum of the denominators); 0 when nothing was counted.  One workgroup: the partials
// come into LDS with one round of loads, then wave 0 adds the numerators and wave 1 the denominators, each in index order.  (A single
// thread walking global memory paid a load latency per step: the forward at N = 16, 320 x 200 took 28.8 us with it, 15.2 us without.)
__global__ __launch_bounds__(SEG_THREADS) void seg_ce_fold_kernel(const double* __restrict__ part, int blocks, float* __restrict__ loss,
                                                                  float* __restrict__ denom) {
    __shared__ double sp[2 * SEG_CE_BLOCKS];
    __shared__ double tot[2];
    for (int i = threadIdx.x; i < 2 * blocks; i += SEG_THREADS) sp[i] = part[i];
    __syncthreads();
    const int which = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0 && which < 2) {
        double s = 0.0;
        for (int i = 0; i < blocks; ++i) s += sp[2 * i + which];
        tot[which] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        loss[0] = tot[1] > 0.0 ? (float)(tot[0] / tot[1]) : 0.f;
        denom[0] = (float)tot[1];
    }
}

// grid (ceil(P / 256)), one pixel per lane: dz[p][c] = g w[l] / denom (softmax_c - [c == l]); +0 for an ignored pixel, behind ncls,
// and everywhere when the denominator is 0
template <typename T, int MODE>
__global__ __launch_bounds__(SEG_THREADS) void seg_ce_bwd_kernel(const T* __restrict__ x, const uint8_t* __restrict__ label, const float* __restrict__ weights,
                                                                 const float* __restrict__ denom, const float* __restrict__ gloss, long P, int C, int ncls,
                                                                 T* __restrict__ dx) {
    constexpr int NS = SegSlots<MODE>::N;
    __shared__ float sw[SEG_MAX_CLS];
    if (threadIdx.x < SEG_MAX_CLS) sw[threadIdx.x] = (int)threadIdx.x < ncls ? weights[threadIdx.x] : 0.f;
    __syncthreads();
    const long p = (long)blockIdx.x * SEG_THREADS + threadIdx.x;
    if (p >= P) return;
    const float den = denom[0];
    const int l = label[p];
    float d[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) d[c] = 0.f;
    const float coef = (l < ncls && den > 0.f) ? gloss[0] * sw[l < ncls ? l : 0] / den : 0.f;
    if (coef != 0.f) {                                       // (a NaN coefficient is not 0: it reaches the gradient)
        float z[NS], e[NS], m;
        seg_load<T, MODE>(x, (size_t)p, C, ncls, z);
        const float inv = 1.f / seg_softmax_terms<NS>(z, ncls, m, e);
#pragma unroll
        for (int c = 0; c < NS; ++c) d[c] = c < ncls ? coef * (e[c] * inv - (c == l ? 1.f : 0.f)) : 0.f;
    }
    seg_store<T, MODE>(dx, (size_t)p, C, ncls, d);
}

// ---------------------------------------------------------------------------------------- argmax of the resized logits
// the tap rule of bilinear_resize (label_ops.hip): F.interpolate(mode='bilinear', align_corners=False)
struct SegTap { int i0, i1; float l; };
__device__ __forceinline__ SegTap seg_tap(int d, float scale, int n_in) {
    float f = ((float)d + 0.5f) * scale - 0.5f;
    f = f < 0.f ? 0.f : f;
    SegTap t;
    t.i0 = min((int)f, n_in - 1);
    t.i1 = t.i0 + (t.i0 < n_in - 1 ? 1 : 0);
    t.l = f - (float)t.i0;
    return t;
}

// grid (ceil(Wo / 256), Ho, N), one output pixel per lane.  same: (Ho, Wo) == (h, w), the plain argmax (no tap arithmetic at all).
template <typename T, int MODE>
__global__ __launch_bounds__(SEG_THREADS) void seg_argmax_kernel(const T* __restrict__ x, int h, int w, int C, int ncls, int Ho, int Wo, float sy, float sx,
                                                                 int same, uint8_t* __restrict__ mask) {
    constexpr int NS = SegSlots<MODE>::N;
    const int ox = blockIdx.x * SEG_THREADS + threadIdx.x, oy = blockIdx.y, n = blockIdx.z;
    if (ox >= Wo) return;
    const size_t base = (size_t)n * h * w;
    float v[NS];
    if (same) {
        seg_load<T, MODE>(x, base + (size_t)oy * w + ox, C, ncls, v);
    } else {
        const SegTap ty = seg_tap(oy, sy, h), tx = seg_tap(ox, sx, w);
        float a[NS], b[NS], c[NS], d[NS];
        seg_load<T, MODE>(x, base + (size_t)ty.i0 * w + tx.i0, C, ncls, a);
        seg_load<T, MODE>(x, base + (size_t)ty.i0 * w + tx.i1, C, ncls, b);
        seg_load<T, MODE>(x, base + (size_t)ty.i1 * w + tx.i0, C, ncls, c);
        seg_load<T, MODE>(x, base + (size_t)ty.i1 * w + tx.i1, C, ncls, d);
#pragma unroll
        for (int k = 0; k < NS; ++k)
            v[k] = k < ncls ? (1.f - ty.l) * ((1.f - tx.l) * a[k] + tx.l * b[k]) + ty.l * ((1.f - tx.l) * c[k] + tx.l * d[k]) : -INFINITY;
    }
    int best = 0;
    float bv = v[0];
#pragma unroll
    for (int k = 1; k < NS; ++k)
        if (k < ncls && v[k] > bv) { bv = v[k]; best = k; }  // strictly greater: a tie stays with the lower class
    mask[((size_t)n * Ho + oy) * Wo + ox] = (uint8_t)best;
}

// ---------------------------------------------------------------------------------------- confusion matrix
// grid (blocks <= SEG_CONF_BLOCKS), 256 threads.  A lane takes 16 consecutive pixels of both masks per step (one 16-byte load each when
// `vec`, the masks being 16-byte aligned), merges runs of equal cells and counts them in LDS; pixels behind the last whole group of 16
// (all of them without `vec`) go one per lane.  conf[t * ncls + q] += the workgroup's count of (truth t, pred q), t, q < ncls.
__device__ __forceinline__ void seg_conf_count(uint32_t* hist, int ncls, int t, int q, int& key, uint32_t& run) {
    const int k = (t < ncls && q < ncls) ? t * ncls + q : -1;
    if (k == key) { ++run; return; }
    if (key >= 0) atomicAdd(&hist[key], run);
    key = k;
    run = 1u;
}
__global__ __launch_bounds__(SEG_THREADS) void seg_confusion_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ truth, long P, int ncls,
                                                                    int vec, unsigned long long* __restrict__ conf) {
    __shared__ uint32_t hist[SEG_MAX_CLS * SEG_MAX_CLS];
    const int cells = ncls * ncls;
    for (int i = threadIdx.x; i < cells; i += SEG_THREADS) hist[i] = 0u;
    __syncthreads();
    const long groups = vec ? P / 16 : 0;
    int key = -1;
    uint32_t run = 0u;
    for (long g = (long)blockIdx.x * SEG_THREADS + threadIdx.x; g < groups; g += (long)gridDim.x * SEG_THREADS) {
        const u32x4_t a = *(const u32x4_t*)(truth + 16 * g), b = *(const u32x4_t*)(pred + 16 * g);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t ta = a[i], pb = b[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) seg_conf_count(hist, ncls, (int)((ta >> (8 * j)) & 0xffu), (int)((pb >> (8 * j)) & 0xffu), key, run);
        }
    }
    for (long p = 16 * groups + (long)blockIdx.x * SEG_THREADS + threadIdx.x; p < P; p += (long)gridDim.x * SEG_THREADS)
        seg_conf_count(hist, ncls, (int)truth[p], (int)pred[p], key, run);
    if (key >= 0) atomicAdd(&hist[key], run);
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += SEG_THREADS)
        if (hist[i]) atomicAdd(&conf[i], (unsigned long long)hist[i]);
}

// ---------------------------------------------------------------------------------------- launchers
int seg_ce_blocks(long P) { const long b = (P + SEG_THREADS - 1) / SEG_THREADS; return (int)(b < SEG_CE_BLOCKS ? b : SEG_CE_BLOCKS); }

}  // namespace

extern "C" size_t s2e_seg_ce_workspace_bytes(int N, int H, int W) {
    if (N < 1 || H < 1 || W < 1 || (long)N * H * W > SEG_MAX_PIXELS) return 0;
    return (size_t)seg_ce_blocks((long)N * H * W) * 2 * sizeof(double);
}

extern "C" int s2e_seg_ce_fwd(int dtype, const void* logits, const uint8_t* label, const float* weights, int N, int H, int W, int C, int ncls,
                              float* loss, float* denom, void* workspace, size_t workspace_bytes, void* stream) {
    if (!logits || !label || !weights || !loss || !denom) S2E_FAIL(S2E_ERR_ARG, "s2e_seg_ce_fwd: bad argument");
    if (const int rc = seg_check("s2e_seg_ce_fwd", dtype, N, H, W, C, ncls)) return rc;
    const size_t need = s2e_seg_ce_workspace_bytes(N, H, W);
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 7))
        S2E_FAIL(S2E_ERR_ARG, "s2e_seg_ce_fwd: workspace of %zu bytes, needs %zu (8-byte aligned)", workspace ? workspace_bytes : (size_t)0, need);
    const long P = (long)N * H * W;
    const int blocks = seg_ce_blocks(P);
    hipStream_t st = (hipStream_t)stream;
    const int rc = seg_dispatch(dtype, seg_mode(dtype, C, logits), "s2e_seg_ce_fwd", [&](auto t, auto mode) { using T = decltype(t);
        seg_ce_fwd_kernel<T, decltype(mode)::value><<<blocks, SEG_THREADS, 0, st>>>((const T*)logits, label, weights, P, C, ncls, (double*)workspace);
        S2E_CHECK_LAUNCH("seg_ce_fwd_kernel"); return S2E_OK; });
    if (rc) return rc;
    seg_ce_fold_kernel<<<1, SEG_THREADS, 0, st>>>((const double*)workspace, blocks, loss, denom);
    S2E_CHECK_LAUNCH("seg_ce_fold_kernel");
    return S2E_OK;
}

extern "C" int s2e_seg_ce_bwd(int dtype, const void* logits, const uint8_t* label, const float* weights, const float* denom, const float* gloss,
                              int N, int H, int W, int C, int ncls, void* dlogits, void* stream) {
    if (!logits || !label || !weights || !denom || !gloss || !dlogits) S2E_FAIL(S2E_ERR_ARG, "s2e_seg_ce_bwd: bad argument");
    if (const int rc = seg_check("s2e_seg_ce_bwd", dtype, N, H, W, C, ncls)) return rc;
    const long P = (long)N * H * W;
    hipStream_t st = (hipStream_t)stream;
    return seg_dispatch(dtype, seg_mode(dtype, C, logits, dlogits), "s2e_seg_ce_bwd", [&](auto t, auto mode) { using T = decltype(t);
        seg_ce_bwd_kernel<T, decltype(mode)::value><<<ceil_div(P, SEG_THREADS), SEG_THREADS, 0, st>>>((const T*)logits, label, weights, denom, gloss, P, C, ncls,
                                                                                                      (T*)dlogits);
        S2E_CHECK_LAUNCH("seg_ce_bwd_kernel"); return S2E_OK; });
}

extern "C" int s2e_seg_argmax_u8(int dtype, const void* logits, int N, int h, int w, int C, int ncls, int Ho, int Wo, uint8_t* mask, void* stream) {
    if (!logits || !mask) S2E_FAIL(S2E_ERR_ARG, "s2e_seg_argmax_u8: bad argument");
    if (const int rc = seg_check("s2e_seg_argmax_u8", dtype, N, h, w, C, ncls)) return rc;
    if (Ho < 1 || Wo < 1) S2E_FAIL(S2E_ERR_ARG, "s2e_seg_argmax_u8: Ho=%d Wo=%d (every size must be at least 1)", Ho, Wo);
    if ((long)N * Ho * Wo > SEG_MAX_PIXELS || Ho > 65535 || N > 65535)
        S2E_FAIL(S2E_ERR_UNSUPPORTED, "s2e_seg_argmax_u8: N=%d Ho=%d Wo=%d is beyond the launch limits (N, Ho <= 65535, N Ho Wo <= 2^31 - 1)", N, Ho, Wo);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(ceil_div(Wo, SEG_THREADS), Ho, N);
    const float sy = (float)h / (float)Ho, sx = (float)w / (float)Wo;
    const int same = (Ho == h && Wo == w) ? 1 : 0;
    return seg_dispatch(dtype, seg_mode(dtype, C, logits), "s2e_seg_argmax_u8", [&](auto t, auto mode) { using T = decltype(t);
        seg_argmax_kernel<T, decltype(mode)::value><<<grid, SEG_THREADS, 0, st>>>((const T*)logits, h, w, C, ncls, Ho, Wo, sy, sx, same, mask);
        S2E_CHECK_LAUNCH("seg_argmax_kernel"); return S2E_OK; });
}

extern "C" int s2e_seg_confusion_u8(const uint8_t* pred, const uint8_t* truth, long P, int ncls, int64_t* conf, void* stream) {
    if (!pred || !truth || !conf || ((uintptr_t)conf & 7)) S2E_FAIL(S2E_ERR_ARG, "s2e_seg_confusion_u8: bad argument");
    if (P < 1) S2E_FAIL(S2E_ERR_ARG, "s2e_seg_confusion_u8: P=%ld (at least one pixel)", P);
    if (ncls < 1 || ncls > SEG_MAX_CLS) S2E_FAIL(S2E_ERR_UNSUPPORTED, "s2e_seg_confusion_u8: ncls=%d (1 to %d classes)", ncls, SEG_MAX_CLS);
    if (P > SEG_MAX_PIXELS) S2E_FAIL(S2E_ERR_UNSUPPORTED, "s2e_seg_confusion_u8: P=%ld is beyond the index limit (P <= 2^31 - 1 per call)", P);
    const int vec = (((uintptr_t)pred | (uintptr_t)truth) & 15) == 0 ? 1 : 0;
    const long items = vec ? (P + 15) / 16 : P;
    const long b = (items + SEG_THREADS - 1) / SEG_THREADS;
    const int blocks = (int)(b < SEG_CONF_BLOCKS ? b : SEG_CONF_BLOCKS);
    seg_confusion_kernel<<<blocks, SEG_THREADS, 0, (hipStream_t)stream>>>(pred, truth, P, ncls, vec, (unsigned long long*)conf);
    S2E_CHECK_LAUNCH("seg_confusion_kernel");
    return S2E_OK;
}
