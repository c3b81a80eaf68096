// Loss reductions (hinge GAN, feature-matching L1), their element-wise gradients, the flat-arena
// Adam step, and the library's error/version entry points.
#include "common.h"
#include <float.h>
#include <limits.h>
#include <stdarg.h>
#include <stdlib.h>

// ------------------------------------------------------------------------------------ error state
static thread_local char g_err[512] = "";
void s2e_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* s2e_last_error(void) { return g_err; }
int s2e_deterministic(void) {
    static const int v = s2e_env_flag("S2E_DETERMINISTIC", false);
    return v;
}
int s2e_cu_count(void) {
    static const int n = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
        return v;
    }();
    return n;
}
extern "C" int s2e_version(void) { return 1; }

// ------------------------------------------------------------------------------------ zero fill (see common.h)
__global__ void s2e_zero_kernel(uint32_t* __restrict__ p, size_t n_words) {
    const size_t nv = n_words / 4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (size_t)gridDim.x * blockDim.x)
        ((u32x4_t*)p)[i] = u32x4_t{0, 0, 0, 0};
    for (size_t i = nv * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += (size_t)gridDim.x * blockDim.x) p[i] = 0;
}
int s2e_zero_async(void* ptr, size_t bytes, hipStream_t st) {
    if (bytes == 0) return S2E_OK;
    if (!ptr || (bytes & 3) || ((uintptr_t)ptr & 15))
        S2E_FAIL(S2E_ERR_ARG, "s2e_zero_async: need a 16-byte aligned pointer and a size that is a multiple of 4");
    const size_t words = bytes / 4;
    size_t blocks = (words / 4 + 255) / 256 + 1;
    if (blocks > 4096) blocks = 4096;
    s2e_zero_kernel<<<(int)blocks, 256, 0, st>>>((uint32_t*)ptr, words);
    S2E_CHECK_LAUNCH("s2e_zero_kernel");
    return S2E_OK;
}

// ------------------------------------------------------------------------------------ loss reduce
constexpr bool loss_has_b(int mode) { return mode == S2E_LOSS_L1 || mode == S2E_LOSS_L1_NANGRAD; }      // the two-operand modes
template <int MODE> __device__ __forceinline__ float loss_term(float a, float b) {
    if (MODE == S2E_LOSS_NEG_MEAN) return -a;
    if (MODE == S2E_LOSS_HINGE_REAL) return -fminf(a - 1.f, 0.f);
    if (MODE == S2E_LOSS_HINGE_FAKE) return -fminf(-a - 1.f, 0.f);
    return fabsf(a - b);
}
template <int MODE> __device__ __forceinline__ float loss_dterm(float a, float b) {
    if (MODE == S2E_LOSS_NEG_MEAN) return -1.f;
    // torch.min(x, 0) (loss.py:68,71) splits the gradient 0.5/0.5 at an exact tie x == 0
    if (MODE == S2E_LOSS_HINGE_REAL) { const float x = a - 1.f; return x < 0.f ? -1.f : (x == 0.f ? -0.5f : 0.f); }
    if (MODE == S2E_LOSS_HINGE_FAKE) { const float x = -a - 1.f; return x < 0.f ? 1.f : (x == 0.f ? 0.5f : 0.f); }
    const float d = a - b;
    // S2E_LOSS_L1: torch l1_loss backward = sign(a-b), and torch's sign(NaN) is 0.  S2E_LOSS_L1_NANGRAD departs from torch on purpose:
    // a NaN difference gives a NaN gradient, so that a non-finite feature reaches the gradient guard as it reaches the
    // loss value instead of vanishing as a zero; every other input gives S2E_LOSS_L1's bits
    if (MODE == S2E_LOSS_L1_NANGRAD) return d > 0.f ? 1.f : (d < 0.f ? -1.f : (d == d ? 0.f : d));
    return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
}

template <typename T, int MODE>
__global__ __launch_bounds__(256) void loss_reduce_kernel(const T* __restrict__ a, const T* __restrict__ b, long n, float scale,
                                                          float* __restrict__ out) {
    constexpr int VEC = Vec<T>::N;
    __shared__ float red[4];
    float s = 0.f;
    // 16-B vector path only when both pointers are 16-B aligned (a fake/real half of an odd-sized map is not)
    const bool al = ((((uintptr_t)a) | (loss_has_b(MODE) ? (uintptr_t)b : 0)) & 15) == 0;
    const long nv = al ? n / VEC : 0;
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += (long)gridDim.x * blockDim.x) {
        float fa[VEC], fb[VEC];
        unpack16<T>(*(const u32x4_t*)(a + v * VEC), fa);
        if (loss_has_b(MODE)) unpack16<T>(*(const u32x4_t*)(b + v * VEC), fb);
#pragma unroll
        for (int j = 0; j < VEC; ++j) s += loss_term<MODE>(fa[j], loss_has_b(MODE) ? fb[j] : 0.f);
    }
    for (long i = nv * VEC + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        s += loss_term<MODE>(load1<T>(a + i), loss_has_b(MODE) ? load1<T>(b + i) : 0.f);   // tail / unaligned
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, scale * (red[0] + red[1] + red[2] + red[3]));
}

template <typename T, int MODE>
__global__ __launch_bounds__(256) void loss_grad_kernel(const T* __restrict__ a, const T* __restrict__ b, long n, float scale,
                                 const float* __restrict__ gscale, T* __restrict__ da, int accumulate) {
    constexpr int VEC = Vec<T>::N;
    if (gscale) scale *= *gscale;
    // 16-byte vectors when every pointer is 16-byte aligned (round 5: element by element -- 2-byte loads and stores -- the eight
    // feature-matching gradients of a G step took 12 us each for 2 ... 17 MB)
    const bool al = ((((uintptr_t)a) | ((uintptr_t)da) | (loss_has_b(MODE) ? (uintptr_t)b : 0)) & 15) == 0;
    const long nv = al ? n / VEC : 0;
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += (long)gridDim.x * blockDim.x) {
        float fa[VEC], fb[VEC], g[VEC];
        unpack16<T>(*(const u32x4_t*)(a + v * VEC), fa);
        if (loss_has_b(MODE)) unpack16<T>(*(const u32x4_t*)(b + v * VEC), fb);
        if (accumulate) unpack16<T>(*(const u32x4_t*)(da + v * VEC), g);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const float d = scale * loss_dterm<MODE>(fa[j], loss_has_b(MODE) ? fb[j] : 0.f);
            g[j] = accumulate ? d + g[j] : d;
        }
        *(u32x4_t*)(da + v * VEC) = pack16<T>(g);
    }
    for (long i = nv * VEC + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        float g = scale * loss_dterm<MODE>(load1<T>(a + i), loss_has_b(MODE) ? load1<T>(b + i) : 0.f);
        if (accumulate) g += load1<T>(da + i);
        store1<T>(da + i, g);
    }
}

template <typename T>
static int loss_dispatch(bool grad, int mode, const T* a, const T* b, long n, float scale, const float* gscale, void* out,
                         int accumulate, hipStream_t st) {
    // one 16-byte vector per thread and trip.  The reduction ends with ONE float atomic per block on a single address, and
    // same-address atomics serialise at ~12 ns each: 1024 blocks cost the feature-matching sums more (13 us) than their 2 ... 17 MB
    // of reads -- at most 256 blocks
    const int grid = s2e_grid1d(n / Vec<T>::N + 1, grad ? 2048 : 256);
    auto go = [&](auto MM) { if (grad) loss_grad_kernel<T, MM><<<grid, 256, 0, st>>>(a, b, n, scale, gscale, (T*)out, accumulate);
                             else loss_reduce_kernel<T, MM><<<grid, 256, 0, st>>>(a, b, n, scale, (float*)out); };
    switch (mode) {
        case S2E_LOSS_NEG_MEAN: go(int_c<S2E_LOSS_NEG_MEAN>{}); break;
        case S2E_LOSS_HINGE_REAL: go(int_c<S2E_LOSS_HINGE_REAL>{}); break;
        case S2E_LOSS_HINGE_FAKE: go(int_c<S2E_LOSS_HINGE_FAKE>{}); break;
        case S2E_LOSS_L1: go(int_c<S2E_LOSS_L1>{}); break;
        case S2E_LOSS_L1_NANGRAD: go(int_c<S2E_LOSS_L1_NANGRAD>{}); break;
        default: S2E_FAIL(S2E_ERR_ARG, "loss: bad mode %d", mode);
    }
    S2E_CHECK_LAUNCH("loss kernel");
    return S2E_OK;
}

extern "C" int s2e_loss_reduce(int dtype, int mode, const void* a, const void* b, long n, float scale, float* out, void* stream) {
    if (!a || !out || n <= 0 || (loss_has_b(mode) && !b)) S2E_FAIL(S2E_ERR_ARG, "s2e_loss_reduce: bad argument");
    return s2e_with_dtype(dtype, "s2e_loss_reduce", [&](auto t) { using T = decltype(t);
        return loss_dispatch<T>(false, mode, (const T*)a, (const T*)b, n, scale, nullptr, out, 0, (hipStream_t)stream); });
}
extern "C" int s2e_loss_grad(int dtype, int mode, const void* a, const void* b, long n, float scale, const float* gscale,
                             void* da, int accumulate, void* stream) {
    if (!a || !da || n <= 0 || (loss_has_b(mode) && !b)) S2E_FAIL(S2E_ERR_ARG, "s2e_loss_grad: bad argument");
    return s2e_with_dtype(dtype, "s2e_loss_grad", [&](auto t) { using T = decltype(t);
        return loss_dispatch<T>(true, mode, (const T*)a, (const T*)b, n, scale, gscale, da, accumulate, (hipStream_t)stream); });
}

// ------------------------------------------------------------------------------------ Adam over a flat arena
// Hyper-parameters live in DEVICE memory (hyper[0..5] = lr, beta1, beta2, eps, completed steps, grad_scale)
// so that a captured hipGraph replays with the current learning rate and bias corrections.
// GUARD (s2e_adam_flat_guarded; `guard` is the record s2e_grad_guard wrote, seg2eye_hip.h): coefficient guard[3] == 0 -- a skipped
// step -- ends the whole launch before it touches p, m or v; any other coefficient multiplies grad_scale, ONE fp32 multiply, and every
// later expression is the unguarded one (a coefficient of 1 gives the unguarded bits).  Without GUARD `guard` is not read.
template <bool GUARD>
__device__ __forceinline__ float adam_grad_scale(const float* __restrict__ hyper, const float* __restrict__ guard) {
    if constexpr (GUARD) return hyper[5] * guard[3];
    else return hyper[5];
}
template <bool GUARD>
__global__ __launch_bounds__(256) void adam_flat_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
        float* __restrict__ v, long n, const float* __restrict__ hyper, const float* __restrict__ guard) {
    if constexpr (GUARD) { if (guard[3] == 0.f) return; }   // (uniform over the launch)
    const float lr = hyper[0], beta1 = hyper[1], beta2 = hyper[2], eps = hyper[3], t = hyper[4] + 1.f, grad_scale = adam_grad_scale<GUARD>(hyper, guard);
    const float wd = hyper[6];                              // torch.optim.Adam's L2 term: g += weight_decay * p
    const float bc1 = 1.f - powf(beta1, t), bc2 = 1.f - powf(beta2, t);
    const float lr_bc1 = lr / bc1, rsqrt_bc2 = 1.f / sqrtf(bc2);
    const long nv = n / 4;
    // beta1 == 0 (the reference's TTUR setting, pix2pix_model.py:98-108) and no weight decay: m_t = g_t * grad_scale EXACTLY, whatever m_{t-1}
    // was (0 * m + 1 * g), and bc1 = 1 -- so the first moment is neither read nor written: 20 instead of 28 bytes per parameter, the
    // same bits in p and v.  (The caller can form m from g when it wants to save it: optim.FlatAdam.state_dict.)
    if (beta1 == 0.f && wd == 0.f) {
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long)gridDim.x * blockDim.x) {
            f32x4_t pp = ((f32x4_t*)p)[i], gg = ((const f32x4_t*)g)[i], vv = ((f32x4_t*)v)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float gr = gg[j] * grad_scale + wd * pp[j];
                const float mj = beta1 * 0.f + (1.f - beta1) * gr;
                vv[j] = beta2 * vv[j] + (1.f - beta2) * gr * gr;
                pp[j] -= lr_bc1 * mj / (sqrtf(vv[j]) * rsqrt_bc2 + eps);
            }
            ((f32x4_t*)p)[i] = pp; ((f32x4_t*)v)[i] = vv;
        }
        if (blockIdx.x == 0)
            for (long i = nv * 4 + threadIdx.x; i < n; i += blockDim.x) {
                const float gr = g[i] * grad_scale + wd * p[i];
                const float vi = beta2 * v[i] + (1.f - beta2) * gr * gr;
                v[i] = vi;
                p[i] -= lr_bc1 * ((1.f - beta1) * gr) / (sqrtf(vi) * rsqrt_bc2 + eps);
            }
        return;
    }
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long)gridDim.x * blockDim.x) {
        f32x4_t pp = ((f32x4_t*)p)[i], gg = ((const f32x4_t*)g)[i], mm = ((f32x4_t*)m)[i], vv = ((f32x4_t*)v)[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float gr = gg[j] * grad_scale + wd * pp[j];
            mm[j] = beta1 * mm[j] + (1.f - beta1) * gr;
            vv[j] = beta2 * vv[j] + (1.f - beta2) * gr * gr;
            pp[j] -= lr_bc1 * mm[j] / (sqrtf(vv[j]) * rsqrt_bc2 + eps);
        }
        ((f32x4_t*)p)[i] = pp; ((f32x4_t*)m)[i] = mm; ((f32x4_t*)v)[i] = vv;
    }
    if (blockIdx.x == 0)
        for (long i = nv * 4 + threadIdx.x; i < n; i += blockDim.x) {
            const float gr = g[i] * grad_scale + wd * p[i];
            const float mi = beta1 * m[i] + (1.f - beta1) * gr;
            const float vi = beta2 * v[i] + (1.f - beta2) * gr * gr;
            m[i] = mi; v[i] = vi;
            p[i] -= lr_bc1 * mi / (sqrtf(vi) * rsqrt_bc2 + eps);
        }
}
// a skipped step is not a step: the guarded tick counts completed steps only (bias corrections, the average's start_step)
template <bool GUARD> __global__ void adam_tick_kernel(float* hyper, const float* guard) {
    if constexpr (GUARD) { if (guard[3] == 0.f) return; }
    hyper[4] += 1.f;
}

template <bool GUARD>
static int adam_flat_launch(const char* name, float* p, const float* g, float* m, float* v, long n, float* hyper, const float* guard,
                            hipStream_t st) {
    if (!p || !g || !m || !v || !hyper || (GUARD && !guard) || n <= 0) S2E_FAIL(S2E_ERR_ARG, "%s: bad argument", name);
    if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) S2E_FAIL(S2E_ERR_ARG, "%s: arenas must be 16-byte aligned", name);
    const int grid = s2e_grid1d(n / 4 + 1, 4096);
    adam_flat_kernel<GUARD><<<grid, 256, 0, st>>>(p, g, m, v, n, hyper, guard);
    S2E_CHECK_LAUNCH("adam_flat_kernel");
    adam_tick_kernel<GUARD><<<1, 1, 0, st>>>(hyper, guard);         // after every block has read hyper[4]
    S2E_CHECK_LAUNCH("adam_tick_kernel");
    return S2E_OK;
}
extern "C" int s2e_adam_flat(float* p, const float* g, float* m, float* v, long n, float* hyper, void* stream) {
    return adam_flat_launch<false>("s2e_adam_flat", p, g, m, v, n, hyper, nullptr, (hipStream_t)stream);
}
extern "C" int s2e_adam_flat_guarded(float* p, const float* g, float* m, float* v, long n, float* hyper, const float* guard, void* stream) {
    return adam_flat_launch<true>("s2e_adam_flat_guarded", p, g, m, v, n, hyper, guard, (hipStream_t)stream);
}

// ---- the same step with an exponential moving average of the parameters folded in (optim.FlatAdam(ema_decay=...)).
// The Adam expressions are adam_flat_kernel's, term for term and in its order, in all four places (both branches, vector body and
// scalar tail): p, v and m come out with the bits that kernel gives.  The average costs its own read and write (8 bytes per
// parameter: 28 instead of 20 at beta1 = 0, 36 instead of 28 otherwise) -- the new p is in registers when it is needed.
// ema_hyper (DEVICE memory, like hyper) = {decay, start_step}: the launch that performs step t = hyper[4] + 1 copies (ema = p_new,
// ema is not read) while t <= start_step and averages afterwards, ema = decay * ema + (1 - decay) * p_new.
__device__ __forceinline__ float ema_of(float e, float pn, float decay, float one_minus) { return decay * e + one_minus * pn; }

// GUARD: as in adam_flat_kernel; a skipped step leaves ema alone too.
template <bool GUARD>
__global__ __launch_bounds__(256) void adam_flat_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
        float* __restrict__ v, float* __restrict__ ema, long n, const float* __restrict__ hyper, const float* __restrict__ ema_hyper,
        const float* __restrict__ guard) {
    if constexpr (GUARD) { if (guard[3] == 0.f) return; }   // (uniform over the launch)
    const float lr = hyper[0], beta1 = hyper[1], beta2 = hyper[2], eps = hyper[3], t = hyper[4] + 1.f, grad_scale = adam_grad_scale<GUARD>(hyper, guard);
    const float wd = hyper[6];
    const float bc1 = 1.f - powf(beta1, t), bc2 = 1.f - powf(beta2, t);
    const float lr_bc1 = lr / bc1, rsqrt_bc2 = 1.f / sqrtf(bc2);
    const float decay = ema_hyper[0], one_minus = 1.f - decay;
    const bool copy = t <= ema_hyper[1];                    // (uniform over the launch)
    const long nv = n / 4;
    if (beta1 == 0.f && wd == 0.f) {
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long)gridDim.x * blockDim.x) {
            f32x4_t pp = ((f32x4_t*)p)[i], gg = ((const f32x4_t*)g)[i], vv = ((f32x4_t*)v)[i], ee = pp;
            if (!copy) ee = ((f32x4_t*)ema)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float gr = gg[j] * grad_scale + wd * pp[j];
                const float mj = beta1 * 0.f + (1.f - beta1) * gr;
                vv[j] = beta2 * vv[j] + (1.f - beta2) * gr * gr;
                pp[j] -= lr_bc1 * mj / (sqrtf(vv[j]) * rsqrt_bc2 + eps);
                ee[j] = copy ? pp[j] : ema_of(ee[j], pp[j], decay, one_minus);
            }
            ((f32x4_t*)p)[i] = pp; ((f32x4_t*)v)[i] = vv; ((f32x4_t*)ema)[i] = ee;
        }
        if (blockIdx.x == 0)
            for (long i = nv * 4 + threadIdx.x; i < n; i += blockDim.x) {
                const float gr = g[i] * grad_scale + wd * p[i];
                const float vi = beta2 * v[i] + (1.f - beta2) * gr * gr;
                v[i] = vi;
                float pi = p[i];
                pi -= lr_bc1 * ((1.f - beta1) * gr) / (sqrtf(vi) * rsqrt_bc2 + eps);
                p[i] = pi;
                ema[i] = copy ? pi : ema_of(ema[i], pi, decay, one_minus);
            }
        return;
    }
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long)gridDim.x * blockDim.x) {
        f32x4_t pp = ((f32x4_t*)p)[i], gg = ((const f32x4_t*)g)[i], mm = ((f32x4_t*)m)[i], vv = ((f32x4_t*)v)[i], ee = pp;
        if (!copy) ee = ((f32x4_t*)ema)[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float gr = gg[j] * grad_scale + wd * pp[j];
            mm[j] = beta1 * mm[j] + (1.f - beta1) * gr;
            vv[j] = beta2 * vv[j] + (1.f - beta2) * gr * gr;
            pp[j] -= lr_bc1 * mm[j] / (sqrtf(vv[j]) * rsqrt_bc2 + eps);
            ee[j] = copy ? pp[j] : ema_of(ee[j], pp[j], decay, one_minus);
        }
        ((f32x4_t*)p)[i] = pp; ((f32x4_t*)m)[i] = mm; ((f32x4_t*)v)[i] = vv; ((f32x4_t*)ema)[i] = ee;
    }
    if (blockIdx.x == 0)
        for (long i = nv * 4 + threadIdx.x; i < n; i += blockDim.x) {
            const float gr = g[i] * grad_scale + wd * p[i];
            const float mi = beta1 * m[i] + (1.f - beta1) * gr;
            const float vi = beta2 * v[i] + (1.f - beta2) * gr * gr;
            m[i] = mi; v[i] = vi;
            float pi = p[i];
            pi -= lr_bc1 * mi / (sqrtf(vi) * rsqrt_bc2 + eps);
            p[i] = pi;
            ema[i] = copy ? pi : ema_of(ema[i], pi, decay, one_minus);
        }
}

template <bool GUARD>
static int adam_flat_ema_launch(const char* name, float* p, const float* g, float* m, float* v, float* ema, long n, float* hyper,
                                const float* ema_hyper, const float* guard, hipStream_t st) {
    if (!p || !g || !m || !v || !ema || !hyper || !ema_hyper || (GUARD && !guard) || n <= 0) S2E_FAIL(S2E_ERR_ARG, "%s: bad argument", name);
    if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15)
        S2E_FAIL(S2E_ERR_ARG, "%s: arenas must be 16-byte aligned", name);
    const int grid = s2e_grid1d(n / 4 + 1, 4096);      // (s2e_adam_flat's grid)
    adam_flat_ema_kernel<GUARD><<<grid, 256, 0, st>>>(p, g, m, v, ema, n, hyper, ema_hyper, guard);
    S2E_CHECK_LAUNCH("adam_flat_ema_kernel");
    adam_tick_kernel<GUARD><<<1, 1, 0, st>>>(hyper, guard);         // after every block has read hyper[4]
    S2E_CHECK_LAUNCH("adam_tick_kernel");
    return S2E_OK;
}
extern "C" int s2e_adam_flat_ema(float* p, const float* g, float* m, float* v, float* ema, long n, float* hyper, const float* ema_hyper,
                                 void* stream) {
    return adam_flat_ema_launch<false>("s2e_adam_flat_ema", p, g, m, v, ema, n, hyper, ema_hyper, nullptr, (hipStream_t)stream);
}
extern "C" int s2e_adam_flat_ema_guarded(float* p, const float* g, float* m, float* v, float* ema, long n, float* hyper,
                                         const float* ema_hyper, const float* guard, void* stream) {
    return adam_flat_ema_launch<true>("s2e_adam_flat_ema_guarded", p, g, m, v, ema, n, hyper, ema_hyper, guard, (hipStream_t)stream);
}

// ---- the gradient guard (optim.FlatAdam(clip_norm=..., skip_nonfinite=...)): one pass over the gradient arena that yields its global
// norm and the first non-finite element, and from them the coefficient the guarded Adam launches above apply (record layout and
// rule: seg2eye_hip.h).  Two launches, partials then their fold: DESIGN 8 #3.
// The sum of squares is fp64 from the first product on: a finite gradient never overflows it (3e19^2 does overflow fp32), and the
// rounding error of the whole sum stays below the one rounding of the result to fp32.
struct GuardPartial { double sumsq; int first_bad; int pad; };      // one per block of the partial launch, in the caller's workspace

__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
// block-wide {sum, min} of the 256 threads' values, valid in thread 0: wave butterflies, then the four waves in wave order
__device__ __forceinline__ void guard_block_combine(double& s, int& bad) {
    __shared__ double red_s[4];
    __shared__ int red_b[4];
    s = wave_sum(s);
    bad = wave_min_i32(bad);
    if ((threadIdx.x & 63) == 0) { red_s[threadIdx.x >> 6] = s; red_b[threadIdx.x >> 6] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        s = ((red_s[0] + red_s[1]) + red_s[2]) + red_s[3];
        bad = min(min(red_b[0], red_b[1]), min(red_b[2], red_b[3]));
    }
}
// the element test -- true for +-inf and NaN -- and the finite elements' contribution; never inferred from the sum
__device__ __forceinline__ void guard_element(float x, long i, double& s, int& bad) {
    if (!(fabsf(x) <= FLT_MAX)) bad = min(bad, (int)i);
    else s += (double)x * (double)x;
}

__global__ __launch_bounds__(256) void grad_guard_partial_kernel(const float* __restrict__ g, long n, GuardPartial* __restrict__ part) {
    const long nv = n / 4;
    double s = 0.0;
    int bad = INT_MAX;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long)gridDim.x * blockDim.x) {
        const f32x4_t gg = ((const f32x4_t*)g)[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) guard_element(gg[j], i * 4 + j, s, bad);
    }
    if (blockIdx.x == 0)
        for (long i = nv * 4 + threadIdx.x; i < n; i += blockDim.x) guard_element(g[i], i, s, bad);
    guard_block_combine(s, bad);
    if (threadIdx.x == 0) part[blockIdx.x] = GuardPartial{s, bad, 0};
}

// ONE block.  Thread t adds the records [t * chunk, (t + 1) * chunk) in block order, then the block combine: the order depends on
// nothing but nparts, so two runs over the same arena write the same bits.
__global__ __launch_bounds__(256) void grad_guard_final_kernel(const GuardPartial* __restrict__ part, int nparts,
        const float* __restrict__ hyper, float* __restrict__ guard, int* __restrict__ first_bad) {
    const int chunk = (nparts + 255) / 256;
    double s = 0.0;
    int bad = INT_MAX;
    for (int k = threadIdx.x * chunk; k < min(nparts, (int)(threadIdx.x + 1) * chunk); ++k) {
        s += part[k].sumsq;
        bad = min(bad, part[k].first_bad);
    }
    guard_block_combine(s, bad);
    if (threadIdx.x != 0) return;
    const float max_norm = guard[0];
    const bool has_bad = bad != INT_MAX, skipped = has_bad && guard[1] != 0.f;
    const double norm = fabs((double)hyper[5]) * sqrt(s);   // the norm of the gradient Adam would consume (finite elements)
    float c = 1.f;
    if (skipped) c = 0.f;
    else if (has_bad) c = __builtin_nanf("");               // unguarded behaviour, on purpose: the step poisons the weights
    else if (max_norm > 0.f) c = (float)fmin(1.0, (double)max_norm / (norm + 1e-6));     // clip_grad_norm_, norm_type = 2
    guard[2] = (float)norm;
    guard[3] = c;
    guard[4] += skipped ? 1.f : 0.f;
    guard[5] += c < 1.f && !has_bad ? 1.f : 0.f;
    guard[6] = skipped ? guard[6] + 1.f : 0.f;
    guard[7] = 0.f;
    *first_bad = has_bad ? bad : -1;
}

extern "C" size_t s2e_grad_guard_workspace_bytes(long n) {
    return n > 0 ? (size_t)s2e_grid1d(n / 4 + 1, 4096) * sizeof(GuardPartial) : 0;
}
extern "C" int s2e_grad_guard(const float* g, long n, const float* hyper, float* guard, int* first_bad, void* workspace,
                              size_t workspace_bytes, void* stream) {
    if (!g || !hyper || !guard || !first_bad || !workspace || n <= 0) S2E_FAIL(S2E_ERR_ARG, "s2e_grad_guard: bad argument");
    if (n >= (long)INT_MAX) S2E_FAIL(S2E_ERR_ARG, "s2e_grad_guard: first_bad is an int: n must be below 2^31 - 1");
    if (((uintptr_t)g & 15) || ((uintptr_t)workspace & 7)) S2E_FAIL(S2E_ERR_ARG, "s2e_grad_guard: the arena must be 16-byte, the workspace 8-byte aligned");
    if (workspace_bytes < s2e_grad_guard_workspace_bytes(n))
        S2E_FAIL(S2E_ERR_ARG, "s2e_grad_guard: workspace of %zu bytes, %zu needed", workspace_bytes, s2e_grad_guard_workspace_bytes(n));
    const int grid = s2e_grid1d(n / 4 + 1, 4096);           // (s2e_adam_flat's grid)
    grad_guard_partial_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(g, n, (GuardPartial*)workspace);
    S2E_CHECK_LAUNCH("grad_guard_partial_kernel");
    grad_guard_final_kernel<<<1, 256, 0, (hipStream_t)stream>>>((const GuardPartial*)workspace, grid, hyper, guard, first_bad);
    S2E_CHECK_LAUNCH("grad_guard_final_kernel");
    return S2E_OK;
}

// ---- data-parallel gradient exchange, 'direct' form (seg2eye_amd/distributed.py): the owner of a bucket shard adds the P copies the
// all-to-all delivered, in rank order, fp32 accumulation, ONE rounding to the payload dtype -- every replica gets the same bits from the
// all-gather that follows.  recv: [world][shard] elements; out: [shard].  One 16-byte vector per thread.
template <typename T>
__global__ __launch_bounds__(256) void shard_sum_kernel(const T* __restrict__ recv, T* __restrict__ out, int world, long shard) {
    constexpr int VEC = Vec<T>::N;
    const long nv = shard / VEC;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long)gridDim.x * blockDim.x) {
        float a[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) a[j] = 0.f;
        for (int r = 0; r < world; ++r) {
            float f[VEC];
            unpack16<T>(*(const u32x4_t*)(recv + (size_t)r * shard + i * VEC), f);
#pragma unroll
            for (int j = 0; j < VEC; ++j) a[j] += f[j];
        }
        *(u32x4_t*)(out + i * VEC) = pack16<T>(a);
    }
    if (blockIdx.x == 0)
        for (long i = nv * VEC + threadIdx.x; i < shard; i += blockDim.x) {
            float a = 0.f;
            for (int r = 0; r < world; ++r) a += load1<T>(recv + (size_t)r * shard + i);
            store1<T>(out + i, a);
        }
}

extern "C" int s2e_shard_sum(int dtype, const void* recv, void* out, int world, long shard, void* stream) {
    if (!recv || !out || world <= 0 || shard <= 0) S2E_FAIL(S2E_ERR_ARG, "s2e_shard_sum: bad argument");
    if ((((uintptr_t)recv | (uintptr_t)out) & 15) || shard % s2e_vec_lanes(dtype) != 0)
        S2E_FAIL(S2E_ERR_ARG, "s2e_shard_sum: buffers and the shard size must be 16-byte multiples");
    return s2e_with_dtype(dtype, "s2e_shard_sum", [&](auto t) { using T = decltype(t);
        shard_sum_kernel<T><<<s2e_grid1d(shard / Vec<T>::N + 1, 2048), 256, 0, (hipStream_t)stream>>>((const T*)recv, (T*)out, world, shard);
        S2E_CHECK_LAUNCH("shard_sum_kernel"); return S2E_OK; });
}
