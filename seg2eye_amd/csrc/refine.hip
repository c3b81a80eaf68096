// The residual refiner's four memory-bound pieces: everything around the network of  prediction = clamp(reference
// frame + residual, -1, 1)  -- the network input, the loss on the challenge's error with its gradient, and the submission bytes.
//
// The uint8 planes (N, H, W) are read as the store holds them; a frame's fp32 value exists in registers only:
//   norm(v) = fl(fl(v * fl(2 / 255)) - 1)          two fp32 roundings, never one fused multiply-add (numpy's `image *= 2.0 / 255.0;
//                                                   image -= 1.0` on a float32 array), so a bf16 network still adds its residual to
//                                                   the frame's exact fp32 value
// A flip byte != 0 mirrors every plane of that image horizontally: the pixel (y, x) of the network's side (x, res, dres, out) reads
// the planes at (y, W - 1 - x).
//
// A lane takes RF_V = 4 consecutive pixels of one image: one 32-bit load per plane where W is a multiple of 4 and the planes start on
// 4-byte boundaries (the four then lie in one row, mirrored or not: a mirrored group is one aligned word read backwards), four byte
// loads otherwise; a one-channel res / dres is one 8- or 16-byte access per lane where it is aligned, C strided elements otherwise.
//   s2e_refine_input       one launch.  The planes come in as words (4 pixels a lane); the wide NHWC pixels go out one pixel a lane, so
//                          that a wave's store is one contiguous run: the bytes change lanes by wave shuffles in between.
//   s2e_refine_head_fwd    two launches: grid.y = image, per-workgroup fp64 partials {sum d^2, sum |d|} with plain stores, then one
//                          workgroup folds them in index order.  Nothing is atomic: the same input gives the same bits.
//   s2e_refine_head_bwd    one launch, the prediction recomputed.
//   s2e_refine_predict_u8  one launch.
#include "common.h"

// Nothing in this file may be contracted into a fused multiply-add: the normalisation is two roundings, and the tests compare it with
// == against numpy.  The arithmetic is written with plain operators under this pragma: HIP's __fmul_rn / __fsub_rn are operators
// compiled in their own header, under the default contraction, and a product and a difference made by them did fuse (v_fma_f32).
#pragma clang fp contract(off)

namespace {

constexpr int RF_THREADS = 256;
constexpr int RF_V = 4;                                     // pixels of a lane
constexpr int RF_TILE = RF_THREADS * RF_V;                  // pixels of a workgroup and step
constexpr int RF_FWD_STEPS = 4;                             // steps of a forward workgroup: 4096 pixels per partial pair
constexpr int RF_MAX_CLS = 16;

__device__ __forceinline__ float rf_norm(uint32_t v) {
    const float scaled = (float)v * (float)(2.0 / 255.0);
    return scaled - 1.0f;
}
// torch.clamp(s, -1, 1): a NaN stays a NaN
__device__ __forceinline__ float rf_clamp(float s) { return s < -1.0f ? -1.0f : (s > 1.0f ? 1.0f : s); }

// how the uint8 planes of one image are addressed
struct RfPlane {
    int HW, W;
    bool flipped, vec;
    // where the plane holds the image-flat pixel p
    __device__ __forceinline__ int src(int p) const {
        if (!flipped) return p;
        const int y = p / W;
        return 2 * y * W + W - 1 - p;                       // y W + (W - 1 - (p - y W))
    }
    // the bytes of the pixels p0 .. p0 + 3 (p0 a multiple of 4), pixel p0 in the low byte; a pixel at or past HW gives 0
    __device__ __forceinline__ uint32_t load4(const uint8_t* __restrict__ pl, int p0) const {
        if (vec) {                                          // W % 4 == 0: HW % 4 == 0 too, the group is inside the image or past it
            if (p0 >= HW) return 0u;
            if (!flipped) return *(const uint32_t*)(pl + p0);
            const int y = p0 / W;
            return __builtin_bswap32(*(const uint32_t*)(pl + (2 * y * W + W - 4 - p0)));
        }
        uint32_t w = 0u;
#pragma unroll
        for (int j = 0; j < RF_V; ++j)
            if (p0 + j < HW) w |= (uint32_t)pl[src(p0 + j)] << (8 * j);
        return w;
    }
};
__device__ __forceinline__ RfPlane rf_plane(const uint8_t* flip, int n, int HW, int W, int vec) {
    return RfPlane{HW, W, flip != nullptr && flip[n] != 0, vec != 0};
}
__device__ __forceinline__ uint32_t rf_byte(uint32_t w, int j) { return (w >> (8 * j)) & 0xffu; }

// four consecutive elements of a one-channel tensor in one access
template <typename T> struct RfRow;
template <> struct RfRow<float> {
    static __device__ __forceinline__ void load4(const float* p, float* f) { unpack16<float>(*(const u32x4_t*)p, f); }
    static __device__ __forceinline__ void store4(float* p, const float* f) { *(u32x4_t*)p = pack16<float>(f); }
};
template <> struct RfRow<bf16_t> {
    static __device__ __forceinline__ void load4(const bf16_t* p, float* f) {
        const u32x2_t r = *(const u32x2_t*)p;
        const uint32_t r0 = r[0], r1 = r[1];
        f[0] = bf16_bits_to_f32(r0 & 0xffffu); f[1] = __builtin_bit_cast(float, r0 & 0xffff0000u);
        f[2] = bf16_bits_to_f32(r1 & 0xffffu); f[3] = __builtin_bit_cast(float, r1 & 0xffff0000u);
    }
    static __device__ __forceinline__ void store4(bf16_t* p, const float* f) { *(u32x2_t*)p = u32x2_t{pack2_bf16(f[0], f[1]), pack2_bf16(f[2], f[3])}; }
};

// channel 0 of the pixels p0 .. p0 + 3 of an NHWC tensor (rs: the image's first element); 0 for a pixel at or past HW
template <typename T>
__device__ __forceinline__ void rf_load_res4(const T* __restrict__ rs, int C, int p0, int HW, bool rvec, float* r) {
    if (rvec) {                                             // C == 1, HW % 4 == 0, aligned
        if (p0 < HW) RfRow<T>::load4(rs + p0, r);
        else { r[0] = 0.f; r[1] = 0.f; r[2] = 0.f; r[3] = 0.f; }
        return;
    }
#pragma unroll
    for (int j = 0; j < RF_V; ++j) r[j] = p0 + j < HW ? load1<T>(rs + (size_t)(p0 + j) * C) : 0.f;
}

// one NHWC pixel of C channels: v0, v1, v2 in the first LIVE channels, +0 behind them.  wide: C sizeof(T) is a multiple of 16 and the
// tensor starts on a 16-byte boundary (LIVE <= 3 fits the first 16 bytes of either type)
template <typename T, int LIVE>
__device__ __forceinline__ void rf_store_pixel(T* __restrict__ px, int C, float v0, float v1, float v2, bool wide) {
    constexpr int VN = Vec<T>::N;
    if (wide) {
        float f[VN];
#pragma unroll
        for (int j = 0; j < VN; ++j) f[j] = 0.f;
        f[0] = v0;
        if (LIVE > 1) f[1] = v1;
        if (LIVE > 2) f[2] = v2;
        *(u32x4_t*)px = pack16<T>(f);
        for (int c = VN; c < C; c += VN) *(u32x4_t*)(px + c) = u32x4_t{0u, 0u, 0u, 0u};
    } else {
        for (int c = 0; c < C; ++c)
            store1<T>(px + c, c == 0 ? v0 : (LIVE > 1 && c == 1) ? v1 : (LIVE > 2 && c == 2) ? v2 : 0.f);
    }
}

// ---------------------------------------------------------------------------------------- the network input
// grid (ceil(HW / 1024), N).  A wave owns 256 consecutive pixels: lane l loads the words of the pixels 4 l .. 4 l + 3 of the three
// planes, then for j = 0 .. 3 the wave writes the pixels 64 j + l, whose bytes lie in lane 16 j + l / 4 at position l % 4.
template <typename T>
__global__ __launch_bounds__(RF_THREADS) void refine_input_kernel(const uint8_t* __restrict__ tmask, const uint8_t* __restrict__ rimg,
                                                                  const uint8_t* __restrict__ rmask, const uint8_t* __restrict__ flip,
                                                                  const uint8_t* __restrict__ levels, int ncls, int HW, int W, int C, int vec,
                                                                  int wide, T* __restrict__ x) {
    __shared__ uint32_t lev[RF_MAX_CLS];
    if (threadIdx.x < RF_MAX_CLS) lev[threadIdx.x] = (int)threadIdx.x < ncls ? (uint32_t)levels[threadIdx.x] : 0u;
    __syncthreads();
    const int n = blockIdx.y, lane = threadIdx.x & 63;
    const RfPlane P = rf_plane(flip, n, HW, W, vec);
    const size_t img = (size_t)n * HW;
    const int t0 = blockIdx.x * RF_TILE + (int)(threadIdx.x >> 6) * (64 * RF_V);
    const int p0 = t0 + RF_V * lane;
    const uint32_t wt = P.load4(tmask + img, p0), wi = P.load4(rimg + img, p0), wm = P.load4(rmask + img, p0);
#pragma unroll
    for (int j = 0; j < RF_V; ++j) {
        const int from = 16 * j + (lane >> 2), k = lane & 3;
        const uint32_t ct = rf_byte(__shfl(wt, from, 64), k), vi = rf_byte(__shfl(wi, from, 64), k), cm = rf_byte(__shfl(wm, from, 64), k);
        const int q = t0 + 64 * j + lane;
        if (q >= HW) continue;                              // (after the shuffles: every lane takes part in them)
        const uint32_t lt = (int)ct < ncls ? lev[ct] : 0u, lm = (int)cm < ncls ? lev[cm] : 0u;      // a label names a class or takes level 0
        rf_store_pixel<T, 3>(x + (img + q) * C, C, rf_norm(lt), rf_norm(vi), rf_norm(lm), wide != 0);
    }
}

// ---------------------------------------------------------------------------------------- the loss terms
// p = clamp(fl(r + norm(rimg)), -1, 1), d = fl(p - norm(truth)), both fp32; m = the clamp passes the gradient (inclusive, as torch.clamp)
__device__ __forceinline__ float rf_diff(float r, uint32_t vref, uint32_t vtruth, bool& m) {
    const float s = r + rf_norm(vref);
    m = s >= -1.0f && s <= 1.0f;
    return rf_clamp(s) - rf_norm(vtruth);
}

// grid (ceil(HW / 4096), N).  part[(n B + b) 2 + {0, 1}] = the workgroup's {sum d^2, sum |d|}: d is fp32, its square and every sum fp64.
template <typename T>
__global__ __launch_bounds__(RF_THREADS) void refine_head_fwd_kernel(const T* __restrict__ res, int C, const uint8_t* __restrict__ rimg,
                                                                     const uint8_t* __restrict__ truth, const uint8_t* __restrict__ flip,
                                                                     int HW, int W, int vec, int rvec, double* __restrict__ part) {
    __shared__ double red2[4], red1[4];
    const int n = blockIdx.y;
    const RfPlane P = rf_plane(flip, n, HW, W, vec);
    const size_t img = (size_t)n * HW;
    const T* rs = res + img * C;
    const int b0 = blockIdx.x * (RF_TILE * RF_FWD_STEPS) + RF_V * (int)threadIdx.x;
    uint32_t wi[RF_FWD_STEPS], wt[RF_FWD_STEPS];
    float r[RF_FWD_STEPS][RF_V];
#pragma unroll
    for (int it = 0; it < RF_FWD_STEPS; ++it) {             // every load of the lane first: the walk is bound by load latency
        const int p0 = b0 + it * RF_TILE;
        wi[it] = P.load4(rimg + img, p0);
        wt[it] = P.load4(truth + img, p0);
        rf_load_res4<T>(rs, C, p0, HW, rvec != 0, r[it]);
    }
    double s2 = 0.0, s1 = 0.0;
#pragma unroll
    for (int it = 0; it < RF_FWD_STEPS; ++it) {
        const int p0 = b0 + it * RF_TILE;
#pragma unroll
        for (int j = 0; j < RF_V; ++j) {
            bool m;
            const double d = (double)rf_diff(r[it][j], rf_byte(wi[it], j), rf_byte(wt[it], j), m);
            if (p0 + j < HW) { s2 += d * d; s1 += fabs(d); }
        }
    }
    const double t2 = block_sum4(s2, red2), t1 = block_sum4(s1, red1);
    if (threadIdx.x == 0) {
        double* o = part + ((size_t)n * gridDim.x + blockIdx.x) * 2;
        o[0] = t2;
        o[1] = t1;
    }
}

// One workgroup.  Thread t adds, for the images t, t + 256, ..., the B partial pairs of the image in index order: sumsq[n] (fp64, for the
// backward) and score[n] = 127.5 sqrt(sumsq[n]) / HW; the scores and the sums of |d| of a thread's images add up in that order, the
// threads by block_sum4:  terms = {mean_n score, sum |d| / (N HW), 1471 mean_n score}.
__global__ __launch_bounds__(RF_THREADS) void refine_head_fold_kernel(const double* __restrict__ part, int N, int B, double hw,
                                                                      float* __restrict__ score, double* __restrict__ sumsq,
                                                                      float* __restrict__ terms) {
    __shared__ double reds[4], reda[4];
    double ts = 0.0, ta = 0.0;
    for (int n = threadIdx.x; n < N; n += RF_THREADS) {
        const double* p = part + (size_t)n * B * 2;
        double s2 = 0.0, s1 = 0.0;
#pragma unroll 8
        for (int b = 0; b < B; ++b) { s2 += p[2 * (size_t)b]; s1 += p[2 * (size_t)b + 1]; }
        const double sc = 127.5 * sqrt(s2) / hw;
        sumsq[n] = s2;
        score[n] = (float)sc;
        ts += sc;
        ta += s1;
    }
    const double es = block_sum4(ts, reds), ea = block_sum4(ta, reda);
    if (threadIdx.x == 0) {
        const double eds = es / (double)N;
        terms[0] = (float)eds;
        terms[1] = (float)(ea / ((double)N * hw));
        terms[2] = (float)(1471.0 * eds);
    }
}

// grid (ceil(HW / 1024), N).  dres[p][0] = m (kE_n d + kL sign(d)),  kE_n = g lambda_eds 127.5 / (N HW sqrt(sumsq[n])) (0 where
// sumsq[n] is not above 0),  kL = g lambda_l1 / (N HW), both formed in fp64 and used as fp32; channels 1 .. C - 1 are +0.
template <typename T>
__global__ __launch_bounds__(RF_THREADS) void refine_head_bwd_kernel(const T* __restrict__ res, int C, const uint8_t* __restrict__ rimg,
                                                                     const uint8_t* __restrict__ truth, const uint8_t* __restrict__ flip,
                                                                     int N, int HW, int W, int vec, int rvec, int wide,
                                                                     const double* __restrict__ sumsq, const float* __restrict__ gloss,
                                                                     float lambda_eds, float lambda_l1, T* __restrict__ dres) {
    const int n = blockIdx.y;
    const int p0 = blockIdx.x * RF_TILE + RF_V * (int)threadIdx.x;
    if (p0 >= HW) return;
    const RfPlane P = rf_plane(flip, n, HW, W, vec);
    const size_t img = (size_t)n * HW;
    const uint32_t wi = P.load4(rimg + img, p0), wt = P.load4(truth + img, p0);
    float r[RF_V], v[RF_V];
    rf_load_res4<T>(res + img * C, C, p0, HW, rvec != 0, r);
    const double g = (double)gloss[0], S = sumsq[n], cnt = (double)N * (double)HW;
    const float kE = S > 0.0 ? (float)(g * (double)lambda_eds * 127.5 / (cnt * sqrt(S))) : 0.f;
    const float kL = (float)(g * (double)lambda_l1 / cnt);
#pragma unroll
    for (int j = 0; j < RF_V; ++j) {
        bool m;
        const float d = rf_diff(r[j], rf_byte(wi, j), rf_byte(wt, j), m);
        const float sg = (float)((d > 0.f) - (d < 0.f));
        v[j] = m ? kE * d + kL * sg : 0.f;
    }
    T* ds = dres + img * C;
    if (rvec) {                                             // (one flag for res and dres: the launcher looks at both pointers)
        RfRow<T>::store4(ds + p0, v);
    } else {
#pragma unroll
        for (int j = 0; j < RF_V; ++j)
            if (p0 + j < HW) rf_store_pixel<T, 1>(ds + (size_t)(p0 + j) * C, C, v[j], 0.f, 0.f, wide != 0);
    }
}

// grid (ceil(HW / 1024), N).  out = (uint8)fl(127.5 fl(p + 1)), truncated: the reference's `(255. / 2. * (prediction + 1.0)).astype(np.uint8)`
template <typename T>
__global__ __launch_bounds__(RF_THREADS) void refine_predict_kernel(const T* __restrict__ res, int C, const uint8_t* __restrict__ rimg,
                                                                    const uint8_t* __restrict__ flip, int HW, int W, int vec, int rvec, int ovec,
                                                                    uint8_t* __restrict__ out) {
    const int n = blockIdx.y;
    const int p0 = blockIdx.x * RF_TILE + RF_V * (int)threadIdx.x;
    if (p0 >= HW) return;
    const RfPlane P = rf_plane(flip, n, HW, W, vec);
    const size_t img = (size_t)n * HW;
    const uint32_t wi = P.load4(rimg + img, p0);
    float r[RF_V];
    rf_load_res4<T>(res + img * C, C, p0, HW, rvec != 0, r);
    uint32_t packed = 0u;
#pragma unroll
    for (int j = 0; j < RF_V; ++j) {
        const float p = rf_clamp(r[j] + rf_norm(rf_byte(wi, j)));
        int q = (int)(127.5f * (p + 1.0f));
        q = q < 0 ? 0 : (q > 255 ? 255 : q);                 // (p is in [-1, 1]: only a NaN residual gets here out of range)
        packed |= (uint32_t)q << (8 * j);
    }
    uint8_t* o = out + img + p0;
    if (ovec) {
        *(uint32_t*)o = packed;
    } else {
#pragma unroll
        for (int j = 0; j < RF_V; ++j)
            if (p0 + j < HW) o[j] = (uint8_t)(packed >> (8 * j));
    }
}

// ---------------------------------------------------------------------------------------- host
// the checks every entry shares, after its own pointer checks
int refine_check(const char* name, int dtype, int N, int H, int W, int C, int cmin) {
    S2E_CHECK_DTYPE(dtype, name);
    if (N < 1 || H < 1 || W < 1) S2E_FAIL(S2E_ERR_ARG, "%s: N=%d H=%d W=%d (every size must be at least 1)", name, N, H, W);
    if (C < cmin) S2E_FAIL(S2E_ERR_ARG, "%s: C=%d (at least %d channel%s)", name, C, cmin, cmin > 1 ? "s" : "");
    if ((long)H * W > (1L << 30)) S2E_FAIL(S2E_ERR_UNSUPPORTED, "%s: H=%d W=%d is beyond the launch limits (H W <= 2^30)", name, H, W);
    return s2e_check_image_batch(name, N, H, W);
}

inline bool rf_aligned(const void* p, size_t a) { return p == nullptr || ((uintptr_t)p & (a - 1)) == 0; }
// one 32-bit load per plane and group: the rows are whole groups and every plane starts on a word
inline int rf_vec(int W, const void* a, const void* b, const void* c) { return W % 4 == 0 && rf_aligned(a, 4) && rf_aligned(b, 4) && rf_aligned(c, 4); }
// one access per group of a one-channel tensor
template <typename T> int rf_rvec(long HW, int C, const void* a, const void* b) {
    return C == 1 && HW % 4 == 0 && rf_aligned(a, 4 * sizeof(T)) && rf_aligned(b, 4 * sizeof(T));
}
// 16-byte stores of a pixel
template <typename T> int rf_wide(int C, const void* p) { return (C * sizeof(T)) % 16 == 0 && rf_aligned(p, 16); }
inline long rf_fwd_blocks(long HW) { return (HW + RF_TILE * RF_FWD_STEPS - 1) / (RF_TILE * RF_FWD_STEPS); }

}  // namespace

extern "C" int s2e_refine_input(int dtype, const uint8_t* tmask, const uint8_t* rimg, const uint8_t* rmask, const uint8_t* flip,
                                const uint8_t* levels, int ncls, int N, int H, int W, int C, void* x, void* stream) {
    if (!tmask || !rimg || !rmask || !levels || !x) S2E_FAIL(S2E_ERR_ARG, "s2e_refine_input: bad argument");
    if (const int rc = refine_check("s2e_refine_input", dtype, N, H, W, C, 3)) return rc;
    if (ncls < 1 || ncls > RF_MAX_CLS) S2E_FAIL(S2E_ERR_UNSUPPORTED, "s2e_refine_input: ncls=%d (1 to %d classes)", ncls, RF_MAX_CLS);
    const int HW = H * W;
    const dim3 grid(ceil_div(HW, RF_TILE), N);
    hipStream_t st = (hipStream_t)stream;
    return s2e_with_dtype(dtype, "s2e_refine_input", [&](auto t) { using T = decltype(t);
        refine_input_kernel<T><<<grid, RF_THREADS, 0, st>>>(tmask, rimg, rmask, flip, levels, ncls, HW, W, C, rf_vec(W, tmask, rimg, rmask),
                                                            rf_wide<T>(C, x), (T*)x);
        S2E_CHECK_LAUNCH("refine_input_kernel"); return S2E_OK; });
}

extern "C" size_t s2e_refine_head_workspace_bytes(int N, int H, int W) {
    if (N < 1 || H < 1 || W < 1 || N > 65535 || (long)H * W > (1L << 30) || (long)N * H * W >= (1L << 31)) return 0;
    return (size_t)N * (size_t)rf_fwd_blocks((long)H * W) * 2 * sizeof(double);
}

extern "C" int s2e_refine_head_fwd(int dtype, const void* res, int C, const uint8_t* rimg, const uint8_t* truth, const uint8_t* flip,
                                   int N, int H, int W, float* score, double* sumsq, float* terms, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    if (!res || !rimg || !truth || !score || !sumsq || !terms || !workspace || ((uintptr_t)workspace & 7) || ((uintptr_t)sumsq & 7))
        S2E_FAIL(S2E_ERR_ARG, "s2e_refine_head_fwd: bad argument");
    if (const int rc = refine_check("s2e_refine_head_fwd", dtype, N, H, W, C, 1)) return rc;
    S2E_CHECK_BYTES("s2e_refine_head_fwd", "workspace", workspace_bytes, s2e_refine_head_workspace_bytes(N, H, W));
    const int HW = H * W, B = (int)rf_fwd_blocks(HW);
    hipStream_t st = (hipStream_t)stream;
    const int rc = s2e_with_dtype(dtype, "s2e_refine_head_fwd", [&](auto t) { using T = decltype(t);
        refine_head_fwd_kernel<T><<<dim3(B, N), RF_THREADS, 0, st>>>((const T*)res, C, rimg, truth, flip, HW, W, rf_vec(W, rimg, truth, nullptr),
                                                                     rf_rvec<T>(HW, C, res, nullptr), (double*)workspace);
        S2E_CHECK_LAUNCH("refine_head_fwd_kernel"); return S2E_OK; });
    if (rc) return rc;
    refine_head_fold_kernel<<<1, RF_THREADS, 0, st>>>((const double*)workspace, N, B, (double)HW, score, sumsq, terms);
    S2E_CHECK_LAUNCH("refine_head_fold_kernel");
    return S2E_OK;
}

extern "C" int s2e_refine_head_bwd(int dtype, const void* res, int C, const uint8_t* rimg, const uint8_t* truth, const uint8_t* flip,
                                   int N, int H, int W, const double* sumsq, const float* gloss, float lambda_eds, float lambda_l1,
                                   void* dres, void* stream) {
    if (!res || !rimg || !truth || !sumsq || !gloss || !dres || ((uintptr_t)sumsq & 7)) S2E_FAIL(S2E_ERR_ARG, "s2e_refine_head_bwd: bad argument");
    if (const int rc = refine_check("s2e_refine_head_bwd", dtype, N, H, W, C, 1)) return rc;
    const int HW = H * W;
    const dim3 grid(ceil_div(HW, RF_TILE), N);
    hipStream_t st = (hipStream_t)stream;
    return s2e_with_dtype(dtype, "s2e_refine_head_bwd", [&](auto t) { using T = decltype(t);
        refine_head_bwd_kernel<T><<<grid, RF_THREADS, 0, st>>>((const T*)res, C, rimg, truth, flip, N, HW, W, rf_vec(W, rimg, truth, nullptr),
                                                               rf_rvec<T>(HW, C, res, dres), rf_wide<T>(C, dres), sumsq, gloss, lambda_eds,
                                                               lambda_l1, (T*)dres);
        S2E_CHECK_LAUNCH("refine_head_bwd_kernel"); return S2E_OK; });
}

extern "C" int s2e_refine_predict_u8(int dtype, const void* res, int C, const uint8_t* rimg, const uint8_t* flip, int N, int H, int W,
                                     uint8_t* out, void* stream) {
    if (!res || !rimg || !out) S2E_FAIL(S2E_ERR_ARG, "s2e_refine_predict_u8: bad argument");
    if (const int rc = refine_check("s2e_refine_predict_u8", dtype, N, H, W, C, 1)) return rc;
    const int HW = H * W;
    const dim3 grid(ceil_div(HW, RF_TILE), N);
    hipStream_t st = (hipStream_t)stream;
    return s2e_with_dtype(dtype, "s2e_refine_predict_u8", [&](auto t) { using T = decltype(t);
        refine_predict_kernel<T><<<grid, RF_THREADS, 0, st>>>((const T*)res, C, rimg, flip, HW, W, rf_vec(W, rimg, nullptr, nullptr),
                                                              rf_rvec<T>(HW, C, res, nullptr), HW % 4 == 0 && rf_aligned(out, 4), out);
        S2E_CHECK_LAUNCH("refine_predict_kernel"); return S2E_OK; });
}
