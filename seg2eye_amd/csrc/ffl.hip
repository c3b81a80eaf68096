// Focal frequency loss (Jiang, Dai, Wu, Loy, ICCV 2021) of two single-channel image batches and its gradient: the
// orthonormal 2-D DFT of d = x - y as two dense real matrix products on the exact-fp32 matrix instruction v_mfma_f32_16x16x4_f32.
// Only the Wh = W/2 + 1 non-redundant columns of the Hermitian spectrum are carried, with multiplicity m(kx) = 1 for kx = 0 and for
// kx = W/2 when W is even, 2 otherwise.
//
// With C_n[k][j] = cos(2 pi (k j mod n) / n) / sqrt(n) and S_n likewise with sin (the tables, filled on the device, zero-padded):
//   row transform      [P | Q] = d [C_W | S_W]                     (H x 2 Whp;  P + i Q = conj of the row DFT)
//   column transform   [Zre; Zc] = [C_H -S_H; S_H C_H] [P; Q]      (2 Hp x Whp; Z = Zre - i Zc, so dist = Zre^2 + Zc^2)
//   column inverse     [Ure; Uc] = [C_H S_H; -S_H C_H] [Vre; Vc]   with V = coef[n] gout[n] dist^(alpha/2) (Zre, Zc)
//   row inverse        dx = [Ure | Uc] [m C_W; m S_W]              (H x W)
// Forward, three launches: rows, columns (whose epilogue keeps Z when asked and writes one fp64 partial sum of m dist^(1 + alpha/2)
// and one fp32 partial maximum of dist per block, plain stores), the per-image fold in index order.  Backward, two launches.
// Every padded row and column of the intermediates is written as an exact zero (the tables are zero there), so only the image loads
// and the dx stores look at H and W.  No atomics, no host synchronisation, launch shapes from (N, H, W) alone, the same input gives
// the same bits.
//
// One workgroup of four waves owns a BM x BN output tile; K advances 64 at a time through LDS (k-major, rows padded so that the two
// k rows a half-wave reads sit on disjoint banks), the next stage's loads in flight in registers meanwhile.  A wave holds 2 x 2 tiles
// of 16 x 16 and deals the groups of 4 k round-robin to FOUR accumulator sets: 16 independent accumulators keep the 16x16x4 form at
// its issue rate, and each k-ordered fmaf chain is K/4 long instead of K; the sets are added pairwise at the end.
#include "common.h"

namespace {

constexpr int FF_BK = 64;                  // K per LDS stage
constexpr int FF_MAX = 1024;               // largest H or W
constexpr float FF_MAX_ALPHA = 4.f;
enum { FF_A0 = 0, FF_A1 = 1, FF_A2 = 2, FF_AX = 3 };    // alpha = 0, 1, 2: 1, sqrt, identity; anything else: exp2(alpha/2 log2 dist)

struct FflGeom { int H, W, Wh, Hp, Wp, Whp; };
inline int ff_up(int v, int m) { return (v + m - 1) / m * m; }
inline FflGeom ffl_geom(int H, int W) { return FflGeom{H, W, W / 2 + 1, ff_up(H, 64), ff_up(W, 64), ff_up(W / 2 + 1, 32)}; }
// the tables, floats: C_H [Hp][Hp], S_H [Hp][Hp], [C_W | S_W] [Wp][2 Whp], [m C_W; m S_W] [2 Whp][Wp]
inline size_t ffl_table_floats(const FflGeom& g) { return 2 * (size_t)g.Hp * g.Hp + 4 * (size_t)g.Wp * g.Whp; }
inline int ffl_col_blocks(const FflGeom& g) { return (g.Hp / 64) * (g.Whp / 32); }
inline bool ffl_legal_hw(int H, int W) { return H >= 2 && W >= 2 && H <= FF_MAX && W <= FF_MAX; }
inline bool ffl_legal(int N, int H, int W) { return ffl_legal_hw(H, W) && N > 0 && N <= 65535 && (long)N * H * W < (1L << 31); }
inline int ffl_amode(float a) { return a == 0.f ? FF_A0 : a == 1.f ? FF_A1 : a == 2.f ? FF_A2 : FF_AX; }

// dist^(alpha/2); ha = alpha / 2.  alpha = 0 is 1 everywhere, dist = 0 included; for alpha > 0 a bin with dist = 0 has weight 0
__device__ __forceinline__ float ffl_wpow(float dist, int mode, float ha) {
    if (mode == FF_A0) return 1.f;
    if (mode == FF_A1) return sqrtf(dist);
    if (mode == FF_A2) return dist;
    return dist > 0.f ? exp2f(ha * log2f(dist)) : 0.f;
}

// what a loaded pair means: T in its own units, d = x - y; uint8 0..255, d = (a - b) / 255 (the difference is exact)
template <typename T> __device__ __forceinline__ float ffl_diff(T x, T y) { return (float)x - (float)y; }
template <> __device__ __forceinline__ float ffl_diff<uint8_t>(uint8_t x, uint8_t y) { return (float)((int)x - (int)y) / 255.f; }

// 4 or 2 floats as they were loaded
__device__ __forceinline__ void ff_copy(f32x4_t t, float (&v)[4]) { v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3]; }
__device__ __forceinline__ void ff_copy(f32x2_t t, float (&v)[2]) { v[0] = t[0]; v[1] = t[1]; }

// ---------------------------------------------------------------------------------------- tables
// cos and sin of 2 pi (k j mod n) / n, times n^-1/2: the argument reduced in integers (k, j < 1024), evaluated in fp64 (sincospi: exact
// at the quarter turns), rounded once to fp32
__device__ __forceinline__ void ffl_cs(int k, int j, int n, float& c, float& s) {
    const int r = (k * j) % n;
    double ds, dc;
    sincospi(2.0 * (double)r / (double)n, &ds, &dc);
    const double sc = 1.0 / sqrt((double)n);
    c = (float)(dc * sc); s = (float)(ds * sc);
}

__global__ __launch_bounds__(256) void ffl_tables_kernel(float* __restrict__ t, FflGeom g) {
    const size_t nh = (size_t)g.Hp * g.Hp, nw = 2 * (size_t)g.Wp * g.Whp, total = 2 * nh + 2 * nw;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        float c = 0.f, s = 0.f, v = 0.f;
        if (i < 2 * nh) {                                                  // C_H, then S_H
            const size_t e = i < nh ? i : i - nh;
            const int k = (int)(e / g.Hp), j = (int)(e % g.Hp);
            if (k < g.H && j < g.H) { ffl_cs(k, j, g.H, c, s); v = i < nh ? c : s; }
        } else if (i < 2 * nh + nw) {                                      // [C_W | S_W]: row = pixel column, column = kx (twice)
            const size_t e = i - 2 * nh;
            const int col = (int)(e / (2 * g.Whp)), q = (int)(e % (2 * g.Whp)), kx = q < g.Whp ? q : q - g.Whp;
            if (col < g.W && kx < g.Wh) { ffl_cs(col, kx, g.W, c, s); v = q < g.Whp ? c : s; }
        } else {                                                           // [m C_W; m S_W]: row = kx (twice), column = pixel column
            const size_t e = i - 2 * nh - nw;
            const int q = (int)(e / g.Wp), col = (int)(e % g.Wp), kx = q < g.Whp ? q : q - g.Whp;
            if (col < g.W && kx < g.Wh) {
                ffl_cs(col, kx, g.W, c, s);
                const float m = (kx == 0 || 2 * kx == g.W) ? 1.f : 2.f;
                v = m * (q < g.Whp ? c : s);
            }
        }
        t[i] = v;
    }
}

// ---------------------------------------------------------------------------------------- the products
// grid (N-tiles, M-tiles, images), 256 threads = WM x WN waves.  Local row lr of the A tile, 0 <= lr < BM; the wave (wm, wn) owns the rows
// wm 16 + i BM/2 + [0, 16), i = 0, 1, and the columns wn 32 + jn 16 + [0, 16), jn = 0, 1.  Op says what local row lr of M-tile mt is.
template <int BM, int BN, int WM, int WN, typename Op>
__global__ __launch_bounds__(256) void ffl_gemm_kernel(Op op) {
    static_assert(WM * WN == 4 && WM * 32 == BM && WN * 32 == BN, "four waves of 2 x 2 tiles cover the block");
    constexpr int LDA = BM + 16, LDB = BN + 16, AP = BM / 64, KP = FF_BK / 16, PER = BN / 16;
    __shared__ float As[FF_BK][LDA];
    __shared__ float Bs[FF_BK][LDB];
    __shared__ double redd[4];
    __shared__ float redf[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave / WN, wn = wave % WN;
    const int nt = blockIdx.x, mt = blockIdx.y, img = blockIdx.z;
    const int ar = tid >> 2, ak = (tid & 3) * 4;                           // A: 4 consecutive k from ak (+ 16 q) of row ar (+ 64 p)
    const int bk = tid >> 4, bn = (tid & 15) * PER;                        // B: PER consecutive columns of row bk (+ 16 q)
    typename Op::RawA ra[AP][KP];
    typename Op::RawB rb[KP];
    f32x4_t acc[4][2][2];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[s][i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int ksteps = op.ksteps;
    const float scale = op.scale(img);
    // fetch only loads (what was loaded is RawA / RawB); a stage's values are formed from it when the stage goes to LDS, one stage of
    // products later: arithmetic on a loaded value right behind the load would wait for it there, ahead of the products
    auto fetch = [&](int k0) {
#pragma unroll
        for (int q = 0; q < KP; ++q) {
#pragma unroll
            for (int p = 0; p < AP; ++p) op.fetch_a(img, mt, ar + 64 * p, k0 + 16 * q + ak, ra[p][q]);
            op.fetch_b(img, k0 + 16 * q + bk, nt * BN + bn, rb[q]);
        }
    };
    fetch(0);
    for (int kt = 0; kt < ksteps; ++kt) {
        const int k0 = kt * FF_BK;
#pragma unroll
        for (int q = 0; q < KP; ++q) {
#pragma unroll
            for (int p = 0; p < AP; ++p) {
                float v[4];
                op.value_a(mt, ar + 64 * p, k0 + 16 * q + ak, ra[p][q], v);
#pragma unroll
                for (int j = 0; j < 4; ++j) As[16 * q + ak + j][ar + 64 * p] = v[j];
            }
            float w[PER];
            op.value_b(k0 + 16 * q + bk, rb[q], scale, w);
#pragma unroll
            for (int j = 0; j < PER; ++j) Bs[16 * q + bk][bn + j] = w[j];
        }
        __syncthreads();
        if (kt + 1 < ksteps) fetch((kt + 1) * FF_BK);
#pragma unroll
        for (int s = 0; s < FF_BK / 4; ++s) {                              // groups of 4 k, dealt round-robin to the accumulator sets
            const int k = 4 * s + (lane >> 4);
            float a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = As[k][wm * 16 + i * (BM / 2) + (lane & 15)];
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = Bs[k][wn * 32 + j * 16 + (lane & 15)];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[s & 3][i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[s & 3][i][j], 0, 0, 0);
        }
        __syncthreads();
    }
    f32x4_t c[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) c[i][j] = (acc[0][i][j] + acc[1][i][j]) + (acc[2][i][j] + acc[3][i][j]);
    // element e of c[i][j]: local row wm 16 + i BM/2 + (lane >> 4) 4 + e, column nt BN + wn 32 + j 16 + (lane & 15)
    op.finish(img, mt, nt, wm * 16 + (lane >> 4) * 4, nt * BN + wn * 32 + (lane & 15), c, redd, redf);
}

// d [C_W | S_W]: M = Hp (rows of the image, zero past H), K = Wp (columns of the image, zero past W), N = 2 Whp
template <typename T> struct FfRowFwd {
    const T* x; const T* y; const float* tw; float* out; int H, W, Hp, Whp2, ksteps;
    struct RawA { T x[4], y[4]; };
    typedef f32x4_t RawB;
    __device__ __forceinline__ float scale(int) const { return 1.f; }
    // (every load is issued, from a clamped address, and the value chosen afterwards: a load under a per-lane condition becomes a branch
    // with its own wait, one dependent round trip per element)
    __device__ __forceinline__ void fetch_a(int img, int mt, int lr, int k, RawA& raw) const {
        const int r = mt * 64 + lr;
        const size_t row = ((size_t)img * H + (r < H ? r : H - 1)) * W;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t o = row + (k + j < W ? k + j : W - 1);
            raw.x[j] = x[o]; raw.y[j] = y[o];
        }
    }
    __device__ __forceinline__ void value_a(int mt, int lr, int k, const RawA& raw, float (&v)[4]) const {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (mt * 64 + lr < H && k + j < W) ? ffl_diff<T>(raw.x[j], raw.y[j]) : 0.f;
    }
    __device__ __forceinline__ void fetch_b(int, int k, int n, RawB& raw) const { raw = *(const f32x4_t*)(tw + (size_t)k * Whp2 + n); }
    __device__ __forceinline__ void value_b(int, RawB raw, float, float (&v)[4]) const { ff_copy(raw, v); }
    __device__ __forceinline__ void finish(int img, int mt, int, int row, int col, const f32x4_t (&c)[2][2], double*, float*) const {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    out[((size_t)img * Hp + mt * 64 + row + i * 32 + e) * Whp2 + col + j * 16] = c[i][j][e];
    }
};

// the A operand of both column products: local row lr < 64 is row ky = mt 64 + lr of the upper block row (real parts), lr >= 64 of the
// lower one; sgn = +1: [C -S; S C], sgn = -1: its transpose [C S; -S C] (C and S are symmetric)
struct FfColA {
    const float* ch; const float* sh; int Hp; float sgn;
    // (one load from a chosen table, its sign applied afterwards: no load under a condition, see FfRowFwd)
    __device__ __forceinline__ void fetch(int mt, int lr, int k, f32x4_t& raw) const {
        const int pm = lr >> 6, ky = mt * 64 + (lr & 63), pk = k >= Hp ? 1 : 0, r = k - pk * Hp;
        raw = *(const f32x4_t*)((pm == pk ? ch : sh) + (size_t)ky * Hp + r);
    }
    __device__ __forceinline__ void value(int lr, int k, f32x4_t raw, float (&v)[4]) const {
        const int pm = lr >> 6, pk = k >= Hp ? 1 : 0;
        const float f = pm == pk ? 1.f : pm == 0 ? -sgn : sgn;
        v[0] = f * raw[0]; v[1] = f * raw[1]; v[2] = f * raw[2]; v[3] = f * raw[3];
    }
};

// [C -S; S C] [P; Q]: M = 2 Hp as 64 + 64 paired rows per block, K = 2 Hp, N = Whp.  The wave's c[0] and c[1] are Zre and Zc of the SAME bins.
struct FfColFwd {
    FfColA a; const float* pq; float* z; double* part; float* pmax; int H, W, Wh, Hp, Whp, ksteps, mode; float ha;
    typedef f32x4_t RawA;
    typedef f32x2_t RawB;
    __device__ __forceinline__ float scale(int) const { return 1.f; }
    __device__ __forceinline__ void fetch_a(int, int mt, int lr, int k, RawA& raw) const { a.fetch(mt, lr, k, raw); }
    __device__ __forceinline__ void value_a(int, int lr, int k, RawA raw, float (&v)[4]) const { a.value(lr, k, raw, v); }
    __device__ __forceinline__ void fetch_b(int img, int k, int n, RawB& raw) const {
        const int pk = k >= Hp ? 1 : 0, r = k - pk * Hp;
        raw = *(const f32x2_t*)(pq + ((size_t)img * Hp + r) * (2 * Whp) + pk * Whp + n);
    }
    __device__ __forceinline__ void value_b(int, RawB raw, float, float (&v)[2]) const { ff_copy(raw, v); }
    __device__ __forceinline__ void finish(int img, int mt, int nt, int row, int col, const f32x4_t (&c)[2][2], double* redd, float* redf) const {
        double sum = 0.0;
        float mx = 0.f;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int kx = col + j * 16;
            const double m = kx >= Wh ? 0.0 : (kx == 0 || 2 * kx == W) ? 1.0 : 2.0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int ky = mt * 64 + row + e;
                const float re = c[0][j][e], im = c[1][j][e];
                const float dist = fmaf(re, re, im * im);
                sum += m * ((double)dist * (double)ffl_wpow(dist, mode, ha));
                mx = fmaxf(mx, dist);
                if (z) {
                    z[((size_t)img * 2 * Hp + ky) * Whp + kx] = re;
                    z[((size_t)img * 2 * Hp + Hp + ky) * Whp + kx] = im;
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { sum += __shfl_xor(sum, o, 64); mx = fmaxf(mx, __shfl_xor(mx, o, 64)); }     // (wave_sum's adds, interleaved with the max: apart, the kernel compiles to other code)
        if ((threadIdx.x & 63) == 0) { redd[threadIdx.x >> 6] = sum; redf[threadIdx.x >> 6] = mx; }
        __syncthreads();
        if (threadIdx.x == 0) {
            const size_t b = (size_t)img * gridDim.y * gridDim.x + (size_t)mt * gridDim.x + nt;
            part[b] = (redd[0] + redd[1]) + (redd[2] + redd[3]);           // not block_sum4's ((r0 + r1) + r2) + r3, on purpose: changing it changes bits
            pmax[b] = fmaxf(fmaxf(redf[0], redf[1]), fmaxf(redf[2], redf[3]));
        }
    }
};

// [C S; -S C] [Vre; Vc], V = coef[n] gout[n] dist^(alpha/2) (Zre, Zc) formed on load: M = 2 Hp paired, K = 2 Hp, N = Whp; U = [Ure | Uc] (Hp x 2 Whp)
struct FfColInv {
    FfColA a; const float* z; const float* coef; const float* gout; float* u; int Hp, Whp, ksteps, mode; float ha;
    typedef f32x4_t RawA;
    struct RawB { f32x2_t re, im; };
    __device__ __forceinline__ float scale(int img) const { return coef[img] * gout[img]; }
    __device__ __forceinline__ void fetch_a(int, int mt, int lr, int k, RawA& raw) const { a.fetch(mt, lr, k, raw); }
    __device__ __forceinline__ void value_a(int, int lr, int k, RawA raw, float (&v)[4]) const { a.value(lr, k, raw, v); }
    __device__ __forceinline__ void fetch_b(int img, int k, int n, RawB& raw) const {
        const int pk = k >= Hp ? 1 : 0, r = k - pk * Hp;
        const size_t o = ((size_t)img * 2 * Hp + r) * Whp + n;
        raw.re = *(const f32x2_t*)(z + o); raw.im = *(const f32x2_t*)(z + o + (size_t)Hp * Whp);
    }
    __device__ __forceinline__ void value_b(int k, const RawB& raw, float s, float (&v)[2]) const {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float dist = fmaf(raw.re[j], raw.re[j], raw.im[j] * raw.im[j]);
            v[j] = (s * ffl_wpow(dist, mode, ha)) * (k >= Hp ? raw.im[j] : raw.re[j]);
        }
    }
    __device__ __forceinline__ void finish(int img, int mt, int, int row, int col, const f32x4_t (&c)[2][2], double*, float*) const {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    u[((size_t)img * Hp + mt * 64 + row + e) * (2 * Whp) + i * Whp + col + j * 16] = c[i][j][e];
    }
};

// [Ure | Uc] [m C_W; m S_W]: M = Hp, K = 2 Whp, N = Wp; dx (of T) where the pixel exists
template <typename T> struct FfRowInv {
    const float* u; const float* twt; T* dx; int H, W, Hp, Wp, Whp2, ksteps;
    typedef f32x4_t RawA;
    typedef f32x4_t RawB;
    __device__ __forceinline__ float scale(int) const { return 1.f; }
    __device__ __forceinline__ void fetch_a(int img, int mt, int lr, int k, RawA& raw) const {
        raw = *(const f32x4_t*)(u + ((size_t)img * Hp + mt * 64 + lr) * Whp2 + k);
    }
    __device__ __forceinline__ void value_a(int, int, int, RawA raw, float (&v)[4]) const { ff_copy(raw, v); }
    __device__ __forceinline__ void fetch_b(int, int k, int n, RawB& raw) const { raw = *(const f32x4_t*)(twt + (size_t)k * Wp + n); }
    __device__ __forceinline__ void value_b(int, RawB raw, float, float (&v)[4]) const { ff_copy(raw, v); }
    __device__ __forceinline__ void finish(int img, int mt, int, int row, int col, const f32x4_t (&c)[2][2], double*, float*) const {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = mt * 64 + row + i * 32 + e, cc = col + j * 16;
                    if (r < H && cc < W) store1<T>(dx + ((size_t)img * H + r) * W + cc, c[i][j][e]);
                }
    }
};

// grid N.  One thread adds the image's partial sums and takes the partial maxima in index order:
// ffl[n] = sum / (H W max^(alpha/2)); coef[n] (when not null) = 2 / (H W max^(alpha/2)): dx = gout coef Re(inverse DFT of dist^(alpha/2) Z).
// An image whose maximum is 0 has x = y: everything 0.
__global__ __launch_bounds__(64) void ffl_fold_kernel(const double* __restrict__ part, const float* __restrict__ pmax, int blocks, double hw, float alpha,
                                                      float* __restrict__ ffl, float* __restrict__ coef) {
    if (threadIdx.x != 0) return;
    const int n = blockIdx.x;
    double s = 0.0;
    float mx = 0.f;
    for (int i = 0; i < blocks; ++i) { s += part[(size_t)n * blocks + i]; mx = fmaxf(mx, pmax[(size_t)n * blocks + i]); }
    double f = 0.0, cf = 0.0;
    if (mx > 0.f) {
        const double den = hw * (alpha == 0.f ? 1.0 : pow((double)mx, 0.5 * (double)alpha));
        f = s / den; cf = 2.0 / den;
    }
    ffl[n] = (float)f;
    if (coef) coef[n] = (float)cf;
}

// ---------------------------------------------------------------------------------------- host
struct FflWs { size_t pq, part, pmax, total; };                            // byte offsets of the sections of the workspace
inline FflWs ffl_ws(int N, const FflGeom& g) {
    FflWs w{};
    const size_t blocks = (size_t)N * ffl_col_blocks(g);
    w.pq = 0;                                                              // [P | Q] forward, [Ure | Uc] backward: N Hp 2 Whp floats
    w.part = s2e_align256((size_t)N * g.Hp * 2 * g.Whp * sizeof(float));
    w.pmax = w.part + s2e_align256(blocks * sizeof(double));
    w.total = w.pmax + s2e_align256(blocks * sizeof(float));
    return w;
}

int ffl_check_hw(const char* name, int H, int W) {
    if (H < 2 || W < 2 || H > FF_MAX || W > FF_MAX)
        S2E_FAIL(S2E_ERR_UNSUPPORTED, "%s: H=%d W=%d (2 to %d rows and columns expected)", name, H, W, FF_MAX);
    return S2E_OK;
}

// the checks the three entries share, after their own pointer and dtype checks
int ffl_check(const char* name, int N, int H, int W, float alpha, size_t tables_bytes, size_t ws_bytes) {
    if (!(alpha >= 0.f) || !__builtin_isfinite(alpha) || alpha > FF_MAX_ALPHA)
        S2E_FAIL(S2E_ERR_ARG, "%s: alpha=%g (a finite number in [0, %g] expected)", name, (double)alpha, (double)FF_MAX_ALPHA);
    if (const int rc = ffl_check_hw(name, H, W)) return rc;
    if (const int rc = s2e_check_image_batch(name, N, H, W)) return rc;
    S2E_CHECK_BYTES(name, "tables", tables_bytes, s2e_ffl_tables_bytes(H, W));
    S2E_CHECK_BYTES(name, "workspace", ws_bytes, s2e_ffl_workspace_bytes(N, H, W));
    return S2E_OK;
}

template <typename T>
int ffl_fwd_launch(const char* name, const T* x, const T* y, int N, int H, int W, float alpha, const float* tables, size_t tables_bytes, float* ffl,
                   float* coef, float* spectrum, size_t spectrum_bytes, void* ws, size_t ws_bytes, hipStream_t st) {
    if (const int rc = ffl_check(name, N, H, W, alpha, tables_bytes, ws_bytes)) return rc;
    if (spectrum) S2E_CHECK_BYTES(name, "spectrum", spectrum_bytes, s2e_ffl_spectrum_bytes(N, H, W));
    const FflGeom g = ffl_geom(H, W);
    const FflWs w = ffl_ws(N, g);
    const float* ch = tables;
    const float* sh = ch + (size_t)g.Hp * g.Hp;
    const float* tw = sh + (size_t)g.Hp * g.Hp;
    float* pq = (float*)((char*)ws + w.pq);
    double* part = (double*)((char*)ws + w.part);
    float* pmax = (float*)((char*)ws + w.pmax);
    FfRowFwd<T> r{x, y, tw, pq, H, W, g.Hp, 2 * g.Whp, ff_up(W, FF_BK) / FF_BK};
    ffl_gemm_kernel<64, 64, 2, 2, FfRowFwd<T>><<<dim3(2 * g.Whp / 64, g.Hp / 64, N), 256, 0, st>>>(r);
    S2E_CHECK_LAUNCH("ffl_gemm_kernel (rows)");
    FfColFwd c{FfColA{ch, sh, g.Hp, 1.f}, pq, spectrum, part, pmax, H, W, g.Wh, g.Hp, g.Whp, 2 * g.Hp / FF_BK, ffl_amode(alpha), 0.5f * alpha};
    ffl_gemm_kernel<128, 32, 4, 1, FfColFwd><<<dim3(g.Whp / 32, g.Hp / 64, N), 256, 0, st>>>(c);
    S2E_CHECK_LAUNCH("ffl_gemm_kernel (columns)");
    ffl_fold_kernel<<<N, 64, 0, st>>>(part, pmax, ffl_col_blocks(g), (double)H * (double)W, alpha, ffl, coef);
    S2E_CHECK_LAUNCH("ffl_fold_kernel");
    return S2E_OK;
}

}  // namespace

extern "C" size_t s2e_ffl_tables_bytes(int H, int W) {
    if (!ffl_legal_hw(H, W)) return 0;
    return ffl_table_floats(ffl_geom(H, W)) * sizeof(float);
}

extern "C" size_t s2e_ffl_workspace_bytes(int N, int H, int W) {
    if (!ffl_legal(N, H, W)) return 0;
    return ffl_ws(N, ffl_geom(H, W)).total;
}

extern "C" size_t s2e_ffl_spectrum_bytes(int N, int H, int W) {
    if (!ffl_legal(N, H, W)) return 0;
    const FflGeom g = ffl_geom(H, W);
    return (size_t)N * 2 * g.Hp * g.Whp * sizeof(float);
}

extern "C" int s2e_ffl_tables(int H, int W, float* tables, size_t tables_bytes, void* stream) {
    const char* name = "s2e_ffl_tables";
    if (!tables) S2E_FAIL(S2E_ERR_ARG, "s2e_ffl_tables: bad argument");
    if (const int rc = ffl_check_hw(name, H, W)) return rc;
    S2E_CHECK_BYTES(name, "tables", tables_bytes, s2e_ffl_tables_bytes(H, W));
    const FflGeom g = ffl_geom(H, W);
    ffl_tables_kernel<<<s2e_grid1d((long)ffl_table_floats(g), 1024), 256, 0, (hipStream_t)stream>>>(tables, g);
    S2E_CHECK_LAUNCH("ffl_tables_kernel");
    return S2E_OK;
}

extern "C" int s2e_ffl_fwd(int dtype, const void* x, const void* y, int N, int H, int W, float alpha, const float* tables, size_t tables_bytes,
                           float* ffl, float* coef, float* spectrum, size_t spectrum_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !y || !tables || !ffl || !coef || !workspace || N <= 0) S2E_FAIL(S2E_ERR_ARG, "s2e_ffl_fwd: bad argument");
    S2E_CHECK_DTYPE(dtype, "s2e_ffl_fwd");
    return s2e_with_dtype(dtype, "s2e_ffl_fwd", [&](auto t) { using T = decltype(t);
        return ffl_fwd_launch<T>("s2e_ffl_fwd", (const T*)x, (const T*)y, N, H, W, alpha, tables, tables_bytes, ffl, coef, spectrum, spectrum_bytes,
                                 workspace, workspace_bytes, (hipStream_t)stream); });
}

extern "C" int s2e_ffl_u8(const uint8_t* a, const uint8_t* b, int N, int H, int W, float alpha, const float* tables, size_t tables_bytes, float* ffl,
                          void* workspace, size_t workspace_bytes, void* stream) {
    if (!a || !b || !tables || !ffl || !workspace || N <= 0) S2E_FAIL(S2E_ERR_ARG, "s2e_ffl_u8: bad argument");
    return ffl_fwd_launch<uint8_t>("s2e_ffl_u8", a, b, N, H, W, alpha, tables, tables_bytes, ffl, nullptr, nullptr, 0, workspace, workspace_bytes,
                                   (hipStream_t)stream);
}

extern "C" int s2e_ffl_bwd(int dtype, const float* spectrum, const float* coef, const float* gout, int N, int H, int W, float alpha,
                           const float* tables, size_t tables_bytes, void* workspace, size_t workspace_bytes, void* dx, void* stream) {
    const char* name = "s2e_ffl_bwd";
    if (!spectrum || !coef || !gout || !tables || !workspace || !dx || N <= 0) S2E_FAIL(S2E_ERR_ARG, "s2e_ffl_bwd: bad argument");
    S2E_CHECK_DTYPE(dtype, name);
    if (const int rc = ffl_check(name, N, H, W, alpha, tables_bytes, workspace_bytes)) return rc;
    const FflGeom g = ffl_geom(H, W);
    const float* ch = tables;
    const float* sh = ch + (size_t)g.Hp * g.Hp;
    const float* twt = sh + (size_t)g.Hp * g.Hp + 2 * (size_t)g.Wp * g.Whp;
    float* u = (float*)workspace;
    hipStream_t st = (hipStream_t)stream;
    FfColInv c{FfColA{ch, sh, g.Hp, -1.f}, spectrum, coef, gout, u, g.Hp, g.Whp, 2 * g.Hp / FF_BK, ffl_amode(alpha), 0.5f * alpha};
    ffl_gemm_kernel<128, 32, 4, 1, FfColInv><<<dim3(g.Whp / 32, g.Hp / 64, N), 256, 0, st>>>(c);
    S2E_CHECK_LAUNCH("ffl_gemm_kernel (columns, inverse)");
    return s2e_with_dtype(dtype, name, [&](auto e) { using T = decltype(e);
        FfRowInv<T> r{u, twt, (T*)dx, H, W, g.Hp, g.Wp, 2 * g.Whp, 2 * g.Whp / FF_BK};
        ffl_gemm_kernel<64, 64, 2, 2, FfRowInv<T>><<<dim3(g.Wp / 64, g.Hp / 64, N), 256, 0, st>>>(r);
        S2E_CHECK_LAUNCH("ffl_gemm_kernel (rows, inverse)");
        return S2E_OK; });
}
