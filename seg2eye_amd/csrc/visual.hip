// Side-by-side validation panels on the device: what the reference's visualize_sidebyside builds on the host with
// five cv2.resize calls, several min / max passes and a make_grid per sample (util/visualizer.py:131-166,
// data/postprocessor.py:75-130, util/tester.py:72-90), as three launches that read the batch and write finished uint8 panels.
//
//   R(t)      cv2.INTER_LINEAR on the float64 image: lin_tap's float weights, a horizontal then a vertical pass in double
//   norm(t)   over the WHOLE resized batch: min >= -1-eps and max <= 1+eps -> t;  else min >= 0 -> t / max * 2 - 1;  else an error
//   cells     [ style | label | target_original | fake | heat ], each norm(R(.)) at h x w;  style = the first min(ns, 4) images in
//             make_grid(nrow=2, padding=0) order (1 -> the image, 2 -> one row, 3 / 4 -> 2 x 2 with a missing cell 0), then the
//             mean of three replicated channels in fp32, ((a + a) + a) / 3;  heat = |fk - tg| / max|fk - tg| * 2 - 1 (all -1
//             when the maximum is 0, where the reference divides by zero)
//   byte      clamp(trunc((v + 1) * 128), 0, 255)
//
// Launch 1 reduces min / max of the four resized tensors, launch 2 max|fk - tg| with the norm branches decided on the device from
// launch 1's values, launch 3 composes.  No host synchronisation or branch in between; each launch recomputes its bilinear samples
// (four loads and a few fp64 operations).  One partial per workgroup in `ws`, which every workgroup of the next launch folds itself
// (DESIGN 8 #3); fp64 min / max do not depend on the order, so here the tree is not part of the result.  Every value operation is a separate IEEE operation (no contraction), in the order the
// reference's torch / numpy calls perform them, so the bytes agree with the CPU restatement exactly.
#include "common.h"
#pragma clang fp contract(off)

namespace {

constexpr int SBS_THREADS = 256;         // 4 waves
constexpr int SBS_MAX_PARTIALS = 256;    // workgroups of launches 1 and 2 = partials the next launch folds (one per thread)
constexpr int SBS_MAX_COMPOSE = 1024;    // workgroups of launch 3 (each folds the partials once, then strides over the panel)
constexpr int SBS_RANGE_WORDS = 9;       // per workgroup: {min, -max} of the four tensors, then the NaN bits
enum { T_STYLE = 0, T_LABEL = 1, T_TARGET = 2, T_FAKE = 3 };      // = the tensor's status bit, and its cell for 0..3

struct SbsGeom {
    const void* fake; const float* style; const uint8_t* label; const uint8_t* target;
    int ns, k, cols;                     // style images per sample; k = min(ns, 4) of them form a grid of `cols` columns
    int n, H, W, Ht, Wt, GH, GW, h, w;   // GH x GW: the style grid
    double sy, sx, syt, sxt, syg, sxg;   // cv2: scale = 1. / (dst / (double)src), per source geometry
};

// One IEEE operation each, defined HERE, under this file's contract(off).  The header's __dmul_rn / __dadd_rn / ... are plain `x * y`
// and `x + y` compiled under the default contraction mode: after inlining, a __dmul_rn feeding a __dsub_rn becomes ONE v_fma_f64
// (seen in this file's ISA for the tap position below), so they do not keep two roundings apart; operators written under
// contract(off) carry no contract flag and are never fused.  The divisions are the correctly rounded IEEE sequences (div_scale /
// div_fmas / div_fixup), whose internal fused multiply-adds are the only ones in this file's ISA.
__device__ __forceinline__ double dadd(double a, double b) { return a + b; }
__device__ __forceinline__ double dsub(double a, double b) { return a - b; }
__device__ __forceinline__ double dmul(double a, double b) { return a * b; }
__device__ __forceinline__ double ddiv(double a, double b) { return a / b; }
__device__ __forceinline__ float fadd(float a, float b) { return a + b; }
__device__ __forceinline__ float fsub(float a, float b) { return a - b; }
__device__ __forceinline__ float fdiv(float a, float b) { return a / b; }

// One axis of cv2's INTER_LINEAR: metric.hip's lin_tap, restated with those operators -- there the tap position
// (d + 0.5) * scale - 0.5 is one fused multiply-add, which numpy's two roundings (oracle._cv2_linear_taps) are not.
struct LinTap { int s0, s1; float w0, w1; };
__device__ __forceinline__ LinTap lin_tap(int d, double scale, int n_src) {
    float f = (float)dsub(dmul(dadd((double)d, 0.5), scale), 0.5);
    int s = (int)floorf(f);
    f = fsub(f, (float)s);
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= n_src - 1) { f = 0.f; s = n_src - 1; }
    LinTap t;
    t.s0 = s; t.s1 = s + 1 < n_src ? s + 1 : n_src - 1;              // both inside [0, n_src)
    t.w0 = fsub(1.f, f); t.w1 = f;
    return t;
}

template <typename At>
__device__ __forceinline__ double bilinear(At at, LinTap ty, LinTap tx) {
    const double v00 = at(ty.s0, tx.s0), v01 = at(ty.s0, tx.s1), v10 = at(ty.s1, tx.s0), v11 = at(ty.s1, tx.s1);
    const double top = dadd(dmul(v00, (double)tx.w0), dmul(v01, (double)tx.w1));
    const double bot = dadd(dmul(v10, (double)tx.w0), dmul(v11, (double)tx.w1));
    return dadd(dmul(top, (double)ty.w0), dmul(bot, (double)ty.w1));
}

// R(tensor t)[n][oy][ox].  Every index is clamped into its source by lin_tap; a style-grid position past the k-th image reads nothing.
template <typename T>
__device__ __forceinline__ double sample(const SbsGeom& g, int t, int n, int oy, int ox) {
    if (t == T_STYLE) {
        const float* p = g.style + (size_t)n * g.ns * g.H * g.W;
        return bilinear([&](int y, int x) -> double {
            const int cy = y >= g.H, cx = x >= g.W, cell = cy * g.cols + cx;
            if (cell >= g.k) return 0.0;
            const float a = p[((size_t)cell * g.H + (y - cy * g.H)) * g.W + (x - cx * g.W)];
            return (double)fdiv(fadd(fadd(a, a), a), 3.f);        // torch.mean over three equal channels, fp32
        }, lin_tap(oy, g.syg, g.GH), lin_tap(ox, g.sxg, g.GW));
    }
    if (t == T_TARGET) {
        const uint8_t* p = g.target + (size_t)n * g.Ht * g.Wt;
        return bilinear([&](int y, int x) -> double { return (double)p[(size_t)y * g.Wt + x]; },
                        lin_tap(oy, g.syt, g.Ht), lin_tap(ox, g.sxt, g.Wt));
    }
    const LinTap ty = lin_tap(oy, g.sy, g.H), tx = lin_tap(ox, g.sx, g.W);
    if (t == T_LABEL) {
        const uint8_t* p = g.label + (size_t)n * g.H * g.W;
        return bilinear([&](int y, int x) -> double { return (double)p[(size_t)y * g.W + x]; }, ty, tx);
    }
    const T* p = (const T*)g.fake + (size_t)n * g.H * g.W;
    return bilinear([&](int y, int x) -> double { return (double)load1<T>(p + (size_t)y * g.W + x); }, ty, tx);
}

// min over the workgroup of each m[i], OR of the flags; every thread gets the result.  red: 4 * (N + 1) doubles of LDS.
template <int N>
__device__ __forceinline__ void block_min(double (&m)[N], int& flags, double* red) {
#pragma unroll
    for (int i = 0; i < N; ++i)
        for (int o = 32; o > 0; o >>= 1) m[i] = fmin(m[i], __shfl_xor(m[i], o, 64));
    for (int o = 32; o > 0; o >>= 1) flags |= __shfl_xor(flags, o, 64);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) red[wave * (N + 1) + i] = m[i];
        red[wave * (N + 1) + N] = (double)flags;
    }
    __syncthreads();
#pragma unroll
    for (int wv = 0; wv < SBS_THREADS / 64; ++wv) {
#pragma unroll
        for (int i = 0; i < N; ++i) m[i] = fmin(m[i], red[wv * (N + 1) + i]);
        flags |= (int)red[wv * (N + 1) + N];
    }
    __syncthreads();                                         // (red is used again)
}

// m[2t] = min, m[2t + 1] = -max (exact; one kind of reduction for both); a NaN sets the tensor's bit instead, as torch.min / max
// would hand it on to comparisons that then all fail
struct Ranges { double m[8]; int nan; };
__device__ __forceinline__ void ranges_init(Ranges& r) {
#pragma unroll
    for (int i = 0; i < 8; ++i) r.m[i] = __builtin_huge_val();
    r.nan = 0;
}
template <int Tn>
__device__ __forceinline__ void ranges_add(Ranges& r, double v) {
    if (v != v) { r.nan |= 1 << Tn; return; }
    r.m[2 * Tn] = fmin(r.m[2 * Tn], v);
    r.m[2 * Tn + 1] = fmin(r.m[2 * Tn + 1], -v);
}

// ImageProcessor.normalize's branch per tensor: mx == 0 -> unchanged, else t / mx * 2 - 1 (mx > 1 + eps there); err: the status bits
struct Norms { double mx_style, mx_label, mx_target, mx_fake; int err; };
__device__ __forceinline__ Norms fold_ranges(const double* __restrict__ ws, int nb, double* red) {
    Ranges r;
    ranges_init(r);
    for (int b = threadIdx.x; b < nb; b += SBS_THREADS) {
#pragma unroll
        for (int i = 0; i < 8; ++i) r.m[i] = fmin(r.m[i], ws[(size_t)b * SBS_RANGE_WORDS + i]);
        r.nan |= (int)ws[(size_t)b * SBS_RANGE_WORDS + 8];
    }
    block_min<8>(r.m, r.nan, red);
    Norms q;
    q.err = 0;
    double mx[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const double lo = r.m[2 * t], hi = -r.m[2 * t + 1];
        mx[t] = 0.0;
        if ((r.nan >> t) & 1) q.err |= 1 << t;
        else if (lo >= -1.0 - 1e-6 && hi <= 1.0 + 1e-6) {}
        else if (lo >= 0.0) mx[t] = hi;
        else q.err |= 1 << t;
    }
    q.mx_style = mx[T_STYLE]; q.mx_label = mx[T_LABEL]; q.mx_target = mx[T_TARGET]; q.mx_fake = mx[T_FAKE];
    return q;
}
__device__ __forceinline__ double norm1(double t, double mx) {
    return mx == 0.0 ? t : dadd(dmul(ddiv(t, mx), 2.0), -1.0);     // torch.div, torch.mul, torch.add: three roundings
}

struct PixelAt { int n, oy, ox; };
__device__ __forceinline__ PixelAt pixel_at(long i, int h, int w) {
    PixelAt p;
    p.ox = (int)(i % w);
    const long r = i / w;
    p.oy = (int)(r % h);
    p.n = (int)(r / h);
    return p;
}

// launch 1: ws[b][0..8] = this workgroup's {min, -max} of R(style grid), R(label), R(target_original), R(fake) and its NaN bits
template <typename T>
__global__ __launch_bounds__(SBS_THREADS) void sbs_ranges_kernel(SbsGeom g, double* __restrict__ ws) {
    __shared__ double red[4 * 9];
    Ranges r;
    ranges_init(r);
    const long total = (long)g.n * g.h * g.w;
    for (long i = (long)blockIdx.x * SBS_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * SBS_THREADS) {
        const PixelAt p = pixel_at(i, g.h, g.w);
        ranges_add<T_STYLE>(r, sample<T>(g, T_STYLE, p.n, p.oy, p.ox));
        ranges_add<T_LABEL>(r, sample<T>(g, T_LABEL, p.n, p.oy, p.ox));
        ranges_add<T_TARGET>(r, sample<T>(g, T_TARGET, p.n, p.oy, p.ox));
        ranges_add<T_FAKE>(r, sample<T>(g, T_FAKE, p.n, p.oy, p.ox));
    }
    block_min<8>(r.m, r.nan, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) ws[(size_t)blockIdx.x * SBS_RANGE_WORDS + i] = r.m[i];
        ws[(size_t)blockIdx.x * SBS_RANGE_WORDS + 8] = (double)r.nan;
    }
}

// launch 2: emax[b] = -max over this workgroup's pixels of |fk - tg| (<= 0; a NaN, which launch 3 reports, is skipped)
template <typename T>
__global__ __launch_bounds__(SBS_THREADS) void sbs_maxerr_kernel(SbsGeom g, const double* __restrict__ ws, int nb, double* __restrict__ emax) {
    __shared__ double red[4 * 9];
    const Norms q = fold_ranges(ws, nb, red);
    double m[1] = {0.0};
    int none = 0;
    const long total = (long)g.n * g.h * g.w;
    for (long i = (long)blockIdx.x * SBS_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * SBS_THREADS) {
        const PixelAt p = pixel_at(i, g.h, g.w);
        const double fk = norm1(sample<T>(g, T_FAKE, p.n, p.oy, p.ox), q.mx_fake);
        const double tg = norm1(sample<T>(g, T_TARGET, p.n, p.oy, p.ox), q.mx_target);
        m[0] = fmin(m[0], -fabs(dsub(fk, tg)));
    }
    block_min<1>(m, none, red);
    if (threadIdx.x == 0) emax[blockIdx.x] = m[0];
}

template <typename T>
__device__ __forceinline__ uint32_t panel_byte(const SbsGeom& g, const Norms& q, double max_e, int n, int oy, int p) {
    const int cell = p / g.w, ox = p - cell * g.w;
    double v;
    if (cell == 0) v = norm1(sample<T>(g, T_STYLE, n, oy, ox), q.mx_style);
    else if (cell == 1) v = norm1(sample<T>(g, T_LABEL, n, oy, ox), q.mx_label);
    else if (cell == 2) v = norm1(sample<T>(g, T_TARGET, n, oy, ox), q.mx_target);
    else if (cell == 3) v = norm1(sample<T>(g, T_FAKE, n, oy, ox), q.mx_fake);
    else {
        const double fk = norm1(sample<T>(g, T_FAKE, n, oy, ox), q.mx_fake);
        const double tg = norm1(sample<T>(g, T_TARGET, n, oy, ox), q.mx_target);
        const double e = fabs(dsub(fk, tg));
        v = max_e == 0.0 ? -1.0 : dadd(dmul(ddiv(e, max_e), 2.0), -1.0);
    }
    const double u = dmul(dadd(v, 1.0), 128.0);
    return !(u >= 0.0) ? 0u : (u >= 255.0 ? 255u : (uint32_t)(int)u);          // truncation toward zero; a NaN (reported) -> 0
}

// launch 3: the panels.  One lane per ALIGNED dword of a panel row: a row starts at any byte (row_stride need not be a multiple of
// 4), so slot j of a row covers bytes 4j - lead .. 4j - lead + 3 of it, lead = the row address's low two bits; a slot wholly
// inside the row is one dword store, the ragged first and last slots store their bytes singly.  With w no multiple of 4 a dword
// spans two cells: the cell is chosen per pixel.
template <typename T>
__global__ __launch_bounds__(SBS_THREADS) void sbs_compose_kernel(SbsGeom g, const double* __restrict__ ws, int nb, int row_stride, long panel_stride,
                                                                  int slots, int* __restrict__ status, uint8_t* __restrict__ out) {
    __shared__ double red[4 * 9];
    const Norms q = fold_ranges(ws, nb, red);
    double m[1] = {0.0};
    int none = 0;
    const double* emax = ws + (size_t)nb * SBS_RANGE_WORDS;
    for (int b = threadIdx.x; b < nb; b += SBS_THREADS) m[0] = fmin(m[0], emax[b]);
    block_min<1>(m, none, red);
    const double max_e = -m[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) status[0] = q.err;
    const int pw = 5 * g.w;
    const long items = (long)g.n * g.h * slots;
    for (long i = (long)blockIdx.x * SBS_THREADS + threadIdx.x; i < items; i += (long)gridDim.x * SBS_THREADS) {
        const PixelAt s = pixel_at(i, g.h, slots);                      // (.ox: the slot)
        uint8_t* row = out + (size_t)s.n * panel_stride + (size_t)s.oy * row_stride;
        const int p0 = 4 * s.ox - (int)((uintptr_t)row & 3);
        uint32_t b[4], packed = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = p0 + j;
            b[j] = (p >= 0 && p < pw) ? panel_byte<T>(g, q, max_e, s.n, s.oy, p) : 0u;
            packed |= b[j] << (8 * j);
        }
        if (p0 >= 0 && p0 + 3 < pw) *(uint32_t*)(row + p0) = packed;
        else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (p0 + j >= 0 && p0 + j < pw) row[p0 + j] = (uint8_t)b[j];
        }
    }
}

int sbs_partials(int n, int h, int w) {
    const long blocks = ((long)n * h * w + SBS_THREADS - 1) / SBS_THREADS;
    return (int)(blocks < SBS_MAX_PARTIALS ? blocks : SBS_MAX_PARTIALS);
}

template <typename T>
int sbs_launch(const SbsGeom& g, int row_stride, long panel_stride, double* ws, int* status, uint8_t* out, hipStream_t st) {
    const int nb = sbs_partials(g.n, g.h, g.w);
    sbs_ranges_kernel<T><<<nb, SBS_THREADS, 0, st>>>(g, ws);
    S2E_CHECK_LAUNCH("sbs_ranges_kernel");
    sbs_maxerr_kernel<T><<<nb, SBS_THREADS, 0, st>>>(g, ws, nb, ws + (size_t)nb * SBS_RANGE_WORDS);
    S2E_CHECK_LAUNCH("sbs_maxerr_kernel");
    const int slots = (5 * g.w + 2) / 4 + 1;                 // aligned dwords a row can touch, whatever its first byte's alignment
    const long blocks = ((long)g.n * g.h * slots + SBS_THREADS - 1) / SBS_THREADS;
    sbs_compose_kernel<T><<<(int)(blocks < SBS_MAX_COMPOSE ? blocks : SBS_MAX_COMPOSE), SBS_THREADS, 0, st>>>(
        g, ws, nb, row_stride, panel_stride, slots, status, out);
    S2E_CHECK_LAUNCH("sbs_compose_kernel");
    return S2E_OK;
}

}  // namespace

extern "C" long s2e_sidebyside_ws_bytes(int n, int h, int w) {
    if (n <= 0 || h <= 0 || w <= 0) S2E_FAIL(S2E_ERR_ARG, "s2e_sidebyside_ws_bytes: n, h and w must be positive (got %d, %d, %d)", n, h, w);
    return (long)sbs_partials(n, h, w) * (SBS_RANGE_WORDS + 1) * (long)sizeof(double);
}

extern "C" int s2e_sidebyside_u8(int fake_dtype, const void* fake, const float* style, int ns, const uint8_t* label,
                                 const uint8_t* target_original, int n, int H, int W, int Ht, int Wt, int h, int w,
                                 int row_stride, long panel_stride, void* ws, int* status, uint8_t* out, void* stream) {
#define SBS_NEED(cond, name) do { if (!(cond)) S2E_FAIL(S2E_ERR_ARG, "s2e_sidebyside_u8: bad argument %s", name); } while (0)
    SBS_NEED(fake_dtype == S2E_F32 || fake_dtype == S2E_BF16, "fake_dtype");
    SBS_NEED(fake, "fake (null)");
    SBS_NEED(style, "style (null)");
    SBS_NEED(ns >= 1, "ns (< 1)");
    SBS_NEED(label, "label (null)");
    SBS_NEED(target_original, "target_original (null)");
    SBS_NEED(n > 0, "n (<= 0)");
    SBS_NEED(H > 0, "H (<= 0)");
    SBS_NEED(W > 0, "W (<= 0)");
    SBS_NEED(Ht > 0, "Ht (<= 0)");
    SBS_NEED(Wt > 0, "Wt (<= 0)");
    SBS_NEED(h > 0, "h (<= 0)");
    SBS_NEED(w > 0, "w (<= 0)");
    SBS_NEED(H <= (1 << 20) && W <= (1 << 20) && Ht <= (1 << 24) && Wt <= (1 << 24) && h <= (1 << 24) && w <= (1 << 24), "size (too large)");
    SBS_NEED(row_stride >= 5 * w, "row_stride (< 5 w)");
    SBS_NEED(panel_stride >= (long)(h - 1) * row_stride + 5 * w, "panel_stride (panels overlap)");
    SBS_NEED(ws && ((uintptr_t)ws & 7) == 0, "ws (null or not 8-byte aligned)");
    SBS_NEED(status && ((uintptr_t)status & 3) == 0, "status (null or not 4-byte aligned)");
    SBS_NEED(out, "out (null)");
#undef SBS_NEED
    SbsGeom g;
    g.fake = fake; g.style = style; g.label = label; g.target = target_original;
    g.ns = ns; g.k = ns < 4 ? ns : 4; g.cols = g.k == 1 ? 1 : 2;
    g.n = n; g.H = H; g.W = W; g.Ht = Ht; g.Wt = Wt; g.h = h; g.w = w;
    g.GH = (g.k <= 2 ? 1 : 2) * H; g.GW = g.cols * W;
    g.sy = 1.0 / ((double)h / (double)H); g.sx = 1.0 / ((double)w / (double)W);
    g.syt = 1.0 / ((double)h / (double)Ht); g.sxt = 1.0 / ((double)w / (double)Wt);
    g.syg = 1.0 / ((double)h / (double)g.GH); g.sxg = 1.0 / ((double)w / (double)g.GW);
    hipStream_t st = (hipStream_t)stream;
    return s2e_with_dtype(fake_dtype, "s2e_sidebyside_u8", [&](auto t) {
        return sbs_launch<decltype(t)>(g, row_stride, panel_stride, (double*)ws, status, out, st); });
}
