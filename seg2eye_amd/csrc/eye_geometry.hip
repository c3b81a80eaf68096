// Eye geometry: the integer moments of a label map's rim pixels, from which the host fits the pupil's and the iris'
// ellipse, and the repaint of a mask from fitted conics.  The rules are stated in include/seg2eye_hip.h.  Everything is per image; the
// moments are integer sums (no result depends on the order of an add), the repaint is a copy or a class byte chosen by fp64 comparisons
// in a stated association, so two calls give the same bytes.
//
// No workgroup ever waits for another: the phases are kernels, and a kernel reads only what an earlier launch wrote.
//   first     one lane per EG_PER groups of four consecutive pixels; per curve the rim pixels' n, sum x, sum y, reduced over the workgroup
//             (wave shuffles, then one LDS add per wave) and stored plainly at first[n][k][block][0..2]
//   centred   the same walk; each workgroup first adds up the image's `first` partials (B K 3 words, written by the launch before) and
//             takes the origin from them, then stores the 15 sums of (x - ox)^i (y - oy)^j at sums[n][k][block][0..14]
//   fold      one workgroup per (image, curve): the B partials added up, the origin computed again from the same integers, rim written
// A lane keeps its pixels' labels and the set of its neighbours' classes in registers between the load and the K curves: the labels
// are read once per pass (the rows above and below come from L2).
#include "common.h"

namespace {

constexpr int EG_MAX_CLS = 16;
constexpr int EG_MAX_SIDE = 1024;                            // |x - ox| <= 1023: a fourth power below 2^40, 2^20 of them below 2^60
constexpr int EG_MAX_CURVES = 4;
constexpr int EG_THREADS = 256;
constexpr int EG_PER = 4;                                    // groups of four pixels per lane and pass
constexpr int EG_BLOCK_PIX = EG_THREADS * EG_PER * 4;        // pixels of a workgroup: 4096
constexpr int EG_SUMS = 15;                                  // i + j <= 4, in the header's order
constexpr int EG_FIRST = 3;                                  // n, sum x, sum y
constexpr int EG_SLOTS = EG_FIRST + EG_SUMS;                 // a row of rim: n, ox, oy, then the centred sums
constexpr int EG_PAINT_PIX = EG_THREADS * 4;

struct EgCurves { uint16_t in[EG_MAX_CURVES], out[EG_MAX_CURVES]; };
struct EgPaint { uint8_t cls[EG_MAX_CURVES]; };

typedef unsigned long long u64;

__device__ __forceinline__ long long eg_wave_sum(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the origin of n points with coordinate sum s: the mean rounded half up, in non-negative integers; 0 where there is no point
__device__ __forceinline__ long long eg_origin(long long n, long long s) { return n > 0 ? (2 * s + n) / (2 * n) : 0; }

__device__ __forceinline__ uint32_t eg_bit(int l) { return l < EG_MAX_CLS ? 1u << l : 0u; }

// Four pixels from linear index p of one image (lab: its first pixel).  c[j]: the label, 255 past the image; nb[j]: the set of the
// classes below 16 among the pixel's four neighbours inside the frame.  VEC: W is a multiple of 4 and the image 4-byte aligned, so the
// four pixels lie in one row and each row is one aligned word; otherwise bytes, and the four may span two rows.
template <bool VEC>
__device__ __forceinline__ void eg_load4(const uint8_t* __restrict__ lab, int H, int W, int HW, int p, int* c, uint32_t* nb, int* x, int* y) {
    int u[4], d[4], left = 255, right = 255;
    if (VEC) {
        const uint32_t w = *(const uint32_t*)(lab + p);
        const uint32_t wu = p >= W ? *(const uint32_t*)(lab + p - W) : 0xFFFFFFFFu;
        const uint32_t wd = p + W < HW ? *(const uint32_t*)(lab + p + W) : 0xFFFFFFFFu;
#pragma unroll
        for (int j = 0; j < 4; ++j) { c[j] = (w >> (8 * j)) & 255; u[j] = (wu >> (8 * j)) & 255; d[j] = (wd >> (8 * j)) & 255; }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int q = p + j;
            c[j] = q < HW ? lab[q] : 255;
            u[j] = (q < HW && q >= W) ? lab[q - W] : 255;
            d[j] = q + W < HW ? lab[q + W] : 255;
        }
    }
    if (p > 0) left = lab[p - 1];
    if (p + 4 < HW) right = lab[p + 4];
    const int y0 = p / W, x0 = p - y0 * W;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int xx = x0 + j, yy = y0;
        if (!VEC) while (xx >= W) { xx -= W; ++yy; }         // (at most four turns: W >= 1)
        x[j] = xx; y[j] = yy;
        const int l = j > 0 ? c[j - 1] : left, r = j < 3 ? c[j + 1] : right;
        uint32_t m = eg_bit(u[j]) | eg_bit(d[j]);            // (255 where there is no row above / below)
        if (xx > 0) m |= eg_bit(l);
        if (xx < W - 1) m |= eg_bit(r);
        nb[j] = m;
    }
}

// the workgroup's sums of acc[0..CNT) into dst[0..CNT): s_acc is CNT words of LDS, zero on entry and zero again on return.  hit: this
// lane met a rim pixel; a wave without one (most waves of an eye mask) has nothing to add and skips the shuffles.
template <int CNT>
__device__ __forceinline__ void eg_block_store(long long* acc, bool hit, u64* s_acc, long long* __restrict__ dst) {
    if (__any(hit)) {
#pragma unroll
        for (int i = 0; i < CNT; ++i) {
            const long long v = eg_wave_sum(acc[i]);
            if ((threadIdx.x & 63) == 0 && v) atomicAdd(&s_acc[i], (u64)v);
        }
    }
    __syncthreads();
    if (threadIdx.x < CNT) { dst[threadIdx.x] = (long long)s_acc[threadIdx.x]; s_acc[threadIdx.x] = 0; }
    __syncthreads();
}

// grid (B, N), B = ceil(H W / EG_BLOCK_PIX).  first: [N][K][B][3] int64, sums: [N][K][B][15] int64, two sections of the workspace.
// CENTRED false: writes `first`.  CENTRED true: reads `first` (whole lines of it were written by the launch before, none by this one)
// and writes `sums` about the origin of `first` summed over the B blocks.
template <bool VEC, bool CENTRED>
__global__ __launch_bounds__(EG_THREADS) void eg_moments_kernel(const uint8_t* __restrict__ labels, int H, int W, int K, EgCurves cv,
                                                                 long long* __restrict__ first, long long* __restrict__ sums) {
    __shared__ u64 s_acc[EG_SUMS];
    __shared__ u64 s_first[EG_MAX_CURVES * 3];
    const int n = blockIdx.y, B = gridDim.x, HW = H * W;
    const uint8_t* lab = labels + (size_t)n * HW;
    if (threadIdx.x < EG_SUMS) s_acc[threadIdx.x] = 0;
    if (threadIdx.x < EG_MAX_CURVES * 3) s_first[threadIdx.x] = 0;
    __syncthreads();
    if (CENTRED) {                                           // lane t: word t % 16 of (curve, slot), blocks t / 16, t / 16 + 16, ...
        const int w = threadIdx.x & 15;
        if (w < K * 3) {
            const long long* src = first + ((size_t)(n * K + w / 3) * B) * EG_FIRST + w % 3;
            long long s = 0;
            for (int b = threadIdx.x >> 4; b < B; b += EG_THREADS / 16) s += src[(size_t)b * EG_FIRST];
            if (s) atomicAdd(&s_first[w], (u64)s);
        }
        __syncthreads();
    }
    int c[EG_PER][4], x[EG_PER][4], y[EG_PER][4];
    uint32_t nb[EG_PER][4];
#pragma unroll
    for (int g = 0; g < EG_PER; ++g) {
        const int p = blockIdx.x * EG_BLOCK_PIX + (g * EG_THREADS + threadIdx.x) * 4;
        if (p < HW) eg_load4<VEC>(lab, H, W, HW, p, c[g], nb[g], x[g], y[g]);
        else
#pragma unroll
            for (int j = 0; j < 4; ++j) { c[g][j] = 255; nb[g][j] = 0; x[g][j] = 0; y[g][j] = 0; }
    }
    for (int k = 0; k < K; ++k) {
        const uint32_t in = cv.in[k], out = cv.out[k];
        const size_t slot = (size_t)(n * K + k) * B + blockIdx.x;
        if (!CENTRED) {
            long long acc[3] = {0, 0, 0};
#pragma unroll
            for (int g = 0; g < EG_PER; ++g)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((eg_bit(c[g][j]) & in) && (nb[g][j] & out)) { acc[0] += 1; acc[1] += x[g][j]; acc[2] += y[g][j]; }
            eg_block_store<EG_FIRST>(acc, acc[0] != 0, s_acc, first + slot * EG_FIRST);
        } else {
            const long long cnt = (long long)s_first[3 * k];
            const int ox = (int)eg_origin(cnt, (long long)s_first[3 * k + 1]), oy = (int)eg_origin(cnt, (long long)s_first[3 * k + 2]);
            long long acc[EG_SUMS];
#pragma unroll
            for (int i = 0; i < EG_SUMS; ++i) acc[i] = 0;
#pragma unroll
            for (int g = 0; g < EG_PER; ++g)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((eg_bit(c[g][j]) & in) && (nb[g][j] & out)) {
                        const int u = x[g][j] - ox, v = y[g][j] - oy;            // |u|, |v| <= 1023: a cube fits 32 bits
                        const int uu = u * u, uv = u * v, vv = v * v;
                        acc[0] += 1;
                        acc[1] += u;       acc[2] += v;
                        acc[3] += uu;      acc[4] += uv;      acc[5] += vv;
                        acc[6] += uu * u;  acc[7] += uu * v;  acc[8] += u * vv;  acc[9] += vv * v;
                        acc[10] += (long long)uu * uu; acc[11] += (long long)uu * uv; acc[12] += (long long)uu * vv;
                        acc[13] += (long long)uv * vv; acc[14] += (long long)vv * vv;
                    }
            eg_block_store<EG_SUMS>(acc, acc[0] != 0, s_acc, sums + slot * EG_SUMS);
        }
    }
}

// grid (N K), EG_THREADS threads: rim[n][k][0..18) = n, ox, oy, the 15 centred sums, from the B partials
__global__ __launch_bounds__(EG_THREADS) void eg_fold_kernel(const long long* __restrict__ first, const long long* __restrict__ sums, int B,
                                                             long long* __restrict__ rim) {
    __shared__ u64 s_sum[EG_SLOTS];
    if (threadIdx.x < EG_SLOTS) s_sum[threadIdx.x] = 0;
    __syncthreads();
    const long long* a = first + (size_t)blockIdx.x * B * EG_FIRST;
    const long long* b = sums + (size_t)blockIdx.x * B * EG_SUMS;
    for (int i = threadIdx.x; i < B * EG_FIRST; i += EG_THREADS) {
        const long long v = a[i];
        if (v) atomicAdd(&s_sum[i % EG_FIRST], (u64)v);
    }
    for (int i = threadIdx.x; i < B * EG_SUMS; i += EG_THREADS) {
        const long long v = b[i];
        if (v) atomicAdd(&s_sum[EG_FIRST + i % EG_SUMS], (u64)v);
    }
    __syncthreads();
    if (threadIdx.x < EG_SLOTS) {
        const long long cnt = (long long)s_sum[0];
        const long long v = (long long)s_sum[threadIdx.x];
        rim[(size_t)blockIdx.x * EG_SLOTS + threadIdx.x] = (threadIdx.x == 1 || threadIdx.x == 2) ? eg_origin(cnt, v) : v;
    }
}

// grid (ceil(H W / EG_PAINT_PIX), N): one lane per four consecutive pixels.  VEC: H W a multiple of 4, labels and out 4-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(EG_THREADS) void eg_paint_kernel(const uint8_t* __restrict__ labels, int H, int W, int ncls, int K,
                                                               const double* __restrict__ conic, const int32_t* __restrict__ origin,
                                                               const uint8_t* __restrict__ valid, EgPaint paint, uint32_t keep, int base,
                                                               uint8_t* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double s_q[EG_MAX_CURVES * 6];
    __shared__ int s_o[EG_MAX_CURVES * 2];
    __shared__ int s_ok;
    const int n = blockIdx.y, HW = H * W;
    if (threadIdx.x < K * 6) s_q[threadIdx.x] = conic[(size_t)n * K * 6 + threadIdx.x];
    if (threadIdx.x < K * 2) s_o[threadIdx.x] = origin[(size_t)n * K * 2 + threadIdx.x];
    if (threadIdx.x == 0) {
        int ok = 1;
        for (int k = 0; k < K; ++k) ok &= valid[(size_t)n * K + k] != 0;
        s_ok = ok;
    }
    __syncthreads();
    const int p = (blockIdx.x * EG_THREADS + threadIdx.x) * 4;
    if (p >= HW) return;
    const uint8_t* lab = labels + (size_t)n * HW;
    uint8_t* dst = out + (size_t)n * HW;
    int c[4];
    if (VEC) {
        const uint32_t w = *(const uint32_t*)(lab + p);
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = (w >> (8 * j)) & 255;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = p + j < HW ? lab[p + j] : 255;
    }
    if (s_ok) {
        int y = p / W, x = p - y * W;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (c[j] < ncls && !((keep >> c[j]) & 1u)) {
                int cls = base;
                for (int k = 0; k < K; ++k) {
                    const double* q = s_q + 6 * k;
                    const double u = (double)((long long)x - s_o[2 * k]), v = (double)((long long)y - s_o[2 * k + 1]);
                    const double au = q[0] * u, bu = q[1] * u, cw = q[2] * v, du = q[3] * u, ev = q[4] * v;
                    const double t0 = au * u, t1 = bu * v, t2 = cw * v;
                    const double Q = ((((t0 + t1) + t2) + du) + ev) + q[5];
                    if (Q <= 0.0) cls = paint.cls[k];                            // (a NaN compares false)
                }
                c[j] = cls;
            }
            if (++x == W) { x = 0; ++y; }
        }
    }
    if (VEC) {
        *(uint32_t*)(dst + p) = (uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16 | (uint32_t)c[3] << 24;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (p + j < HW) dst[p + j] = (uint8_t)c[j];
    }
}

// ---------------------------------------------------------------------------------------- launchers
// the checks of the shape, in the order the header states; in / out: the curves' sets (rim moments), paint / base: the repaint's classes
int eg_check(const char* name, int N, int H, int W, int K, int ncls, const uint16_t* in, const uint16_t* out, const uint8_t* paint, int base) {
    if (N < 1 || H < 1 || W < 1) S2E_FAIL(S2E_ERR_ARG, "%s: N=%d H=%d W=%d (every size must be at least 1)", name, N, H, W);
    if (K < 1 || K > EG_MAX_CURVES) S2E_FAIL(S2E_ERR_UNSUPPORTED, "%s: K=%d (1 to %d curves)", name, K, EG_MAX_CURVES);
    if (ncls < 1 || ncls > EG_MAX_CLS) S2E_FAIL(S2E_ERR_UNSUPPORTED, "%s: ncls=%d (1 to %d classes)", name, ncls, EG_MAX_CLS);
    const unsigned all = (1u << ncls) - 1u;
    for (int k = 0; in && k < K; ++k) {
        if (!in[k] || !out[k]) S2E_FAIL(S2E_ERR_ARG, "%s: curve %d: in=0x%x out=0x%x (an empty class set)", name, k, (unsigned)in[k], (unsigned)out[k]);
        if (in[k] & out[k]) S2E_FAIL(S2E_ERR_ARG, "%s: curve %d: in=0x%x out=0x%x (the sets overlap)", name, k, (unsigned)in[k], (unsigned)out[k]);
        if ((in[k] | out[k]) & ~all)
            S2E_FAIL(S2E_ERR_ARG, "%s: curve %d: in=0x%x out=0x%x (a class at or above ncls=%d)", name, k, (unsigned)in[k], (unsigned)out[k], ncls);
    }
    for (int k = 0; paint && k < K; ++k)
        if (paint[k] >= ncls) S2E_FAIL(S2E_ERR_ARG, "%s: paint[%d]=%d (a class below ncls=%d)", name, k, (int)paint[k], ncls);
    if (paint && (base < 0 || base >= ncls)) S2E_FAIL(S2E_ERR_ARG, "%s: base=%d (a class below ncls=%d)", name, base, ncls);
    if (H > EG_MAX_SIDE || W > EG_MAX_SIDE) S2E_FAIL(S2E_ERR_UNSUPPORTED, "%s: H=%d W=%d (each at most %d)", name, H, W, EG_MAX_SIDE);
    return s2e_check_image_batch(name, N, H, W);
}

int eg_blocks(int H, int W) { return ceil_div((long)H * W, EG_BLOCK_PIX); }
// the workspace: `first`, then `sums` on the next 256 bytes
size_t eg_first_bytes(int N, int H, int W, int K) { return s2e_align256((size_t)N * K * eg_blocks(H, W) * EG_FIRST * sizeof(long long)); }
size_t eg_sums_bytes(int N, int H, int W, int K) { return s2e_align256((size_t)N * K * eg_blocks(H, W) * EG_SUMS * sizeof(long long)); }

}  // namespace

extern "C" size_t s2e_rim_moments_workspace_bytes(int N, int H, int W, int K) {
    if (N < 1 || H < 1 || W < 1 || K < 1 || K > EG_MAX_CURVES || H > EG_MAX_SIDE || W > EG_MAX_SIDE || N > 65535 || (long)N * H * W >= (1L << 31)) return 0;
    return eg_first_bytes(N, H, W, K) + eg_sums_bytes(N, H, W, K);
}

extern "C" int s2e_rim_moments(const uint8_t* labels, int N, int H, int W, int ncls, int K, const uint16_t* in_sets, const uint16_t* out_sets,
                               int64_t* rim, void* workspace, size_t workspace_bytes, void* stream) {
    const char* name = "s2e_rim_moments";
    if (!labels || !in_sets || !out_sets || !rim || !workspace) S2E_FAIL(S2E_ERR_ARG, "%s: bad argument", name);
    const size_t need = s2e_rim_moments_workspace_bytes(N, H, W, K);     // (0 for a shape the checks below refuse)
    if (workspace_bytes < need || ((uintptr_t)workspace & 7) || ((uintptr_t)rim & 7))
        S2E_FAIL(S2E_ERR_ARG, "%s: workspace of %zu bytes, needs %zu (workspace and rim 8-byte aligned)", name, workspace_bytes, need);
    if (const int rc = eg_check(name, N, H, W, K, ncls, in_sets, out_sets, nullptr, 0)) return rc;
    EgCurves cv{};
    for (int k = 0; k < K; ++k) { cv.in[k] = in_sets[k]; cv.out[k] = out_sets[k]; }
    hipStream_t st = (hipStream_t)stream;
    long long* first = (long long*)workspace;
    long long* sums = (long long*)((char*)workspace + eg_first_bytes(N, H, W, K));
    const int B = eg_blocks(H, W);
    const bool vec = W % 4 == 0 && ((uintptr_t)labels & 3) == 0;
    if (vec) eg_moments_kernel<true, false><<<dim3(B, N), EG_THREADS, 0, st>>>(labels, H, W, K, cv, first, sums);
    else eg_moments_kernel<false, false><<<dim3(B, N), EG_THREADS, 0, st>>>(labels, H, W, K, cv, first, sums);
    S2E_CHECK_LAUNCH("eg_moments_kernel (first)");
    if (vec) eg_moments_kernel<true, true><<<dim3(B, N), EG_THREADS, 0, st>>>(labels, H, W, K, cv, first, sums);
    else eg_moments_kernel<false, true><<<dim3(B, N), EG_THREADS, 0, st>>>(labels, H, W, K, cv, first, sums);
    S2E_CHECK_LAUNCH("eg_moments_kernel (centred)");
    eg_fold_kernel<<<N * K, EG_THREADS, 0, st>>>(first, sums, B, (long long*)rim);
    S2E_CHECK_LAUNCH("eg_fold_kernel");
    return S2E_OK;
}

extern "C" int s2e_ellipse_paint(const uint8_t* labels, int N, int H, int W, int ncls, int K, const double* conic, const int32_t* origin,
                                 const uint8_t* valid, const uint8_t* paint, int keep, int base, uint8_t* out, void* stream) {
    const char* name = "s2e_ellipse_paint";
    if (!labels || !conic || !origin || !valid || !paint || !out) S2E_FAIL(S2E_ERR_ARG, "%s: bad argument", name);
    if (((uintptr_t)conic & 7) || ((uintptr_t)origin & 3)) S2E_FAIL(S2E_ERR_ARG, "%s: conic must be 8-byte and origin 4-byte aligned", name);
    if (const int rc = eg_check(name, N, H, W, K, ncls, nullptr, nullptr, paint, base)) return rc;
    EgPaint pc{};
    for (int k = 0; k < K; ++k) pc.cls[k] = paint[k];
    const long HW = (long)H * W;
    const dim3 grid(ceil_div(HW, EG_PAINT_PIX), N);
    const uint32_t keep_set = (uint32_t)keep & 0xFFFFu;
    if (HW % 4 == 0 && (((uintptr_t)labels | (uintptr_t)out) & 3) == 0)
        eg_paint_kernel<true><<<grid, EG_THREADS, 0, (hipStream_t)stream>>>(labels, H, W, ncls, K, conic, origin, valid, pc, keep_set, base, out);
    else
        eg_paint_kernel<false><<<grid, EG_THREADS, 0, (hipStream_t)stream>>>(labels, H, W, ncls, K, conic, origin, valid, pc, keep_set, base, out);
    S2E_CHECK_LAUNCH("eg_paint_kernel");
    return S2E_OK;
}
