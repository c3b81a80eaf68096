// Multi-scale structural similarity (MS-SSIM, Wang, Simoncelli, Bovik 2003) of two single-channel image batches and its gradient
// (DESIGN 3.17), on the window, the tile and the separable passes of ssim.hip (ssim_tile.h).  Level 0 is the image, level j + 1 the
// 2 x 2 mean, stride 2, of level j (a trailing odd row or column dropped); levels below the last score the contrast-structure term
// cs = (2 suv + C2) / (su2 + sv2 + C2), the last one the full S; msssim[n] = prod_j max(m_j[n], F)^w_j with m_j the level's mean.
//
// Forward, three launches: the pyramid (one workgroup emits every level of its block, fp32, in the INPUT's units: pooling commutes
// with the affine map to [0, 1]); the moment passes for the tiles of all levels (a by-value table tells a block its level; one fp64
// partial per tile, the three derivative maps per level when the caller wants a gradient; moments about each tile's first pixel at
// every level); the fold (per image: each level's partials in index order, the clamped product, the backward coefficients).
// Backward, two launches: the coarse levels' gradients g_j (fp32, at their own resolution), then level 0, which adds
// sum_j 4^-j g_j(p >> j) while it writes dx.  No atomics, launch shapes from (N, H, W, levels) alone, the same input gives the same bits.
#include "ssim_tile.h"

namespace {

constexpr int MS_MAXL = 5;
constexpr float MS_FLOOR = 1e-3f;     // F: a level's mean below it counts as F and passes no gradient (a policy, not a measurement: DESIGN 3.17)

// one level as a block sees it.  tile0 / tiles / tiles_x: the level's share of the launch's tiles (of positions forward, of pixels
// backward); pix_off: floats before the level in one image's part of the pyramid (levels 1..); map_off: floats before the level's maps
struct MsLevel { int H, W, tile0, tiles, tiles_x, pad; long pix_off, map_off; };
struct MsTable { int levels, total; MsLevel lv[MS_MAXL]; };
struct MsWeights { float w[MS_MAXL]; };

// the level tile `tile` belongs to (static indices only: the table stays in scalar registers)
__device__ __forceinline__ int ms_pick(const MsTable& t, int tile, MsLevel& me) {
    int j = 0;
    me = t.lv[0];
#pragma unroll
    for (int k = 1; k < MS_MAXL; ++k)
        if (k < t.levels && tile >= t.lv[k].tile0) { me = t.lv[k]; j = k; }
    return j;
}

// ---------------------------------------------------------------------------------------- pyramid
// grid (16 x 16 blocks of level-1 pixels, N).  pyr: [x: levels 1..L-1][y: levels 1..L-1], each level (N, H_j, W_j) fp32.  A pixel of
// level j + 1 that exists has its four sources in level j (2 H_{j+1} <= H_j), so every thread only asks whether ITS pixel exists.
template <typename T>
__global__ __launch_bounds__(256) void msssim_pyramid_kernel(const T* __restrict__ x, const T* __restrict__ y, float* __restrict__ pyr, long half,
                                                             MsTable t, int blocks_x) {
    __shared__ float s1[2][16][16], s2[2][8][8], s3[2][4][4];
    const int n = blockIdx.y, by = blockIdx.x / blocks_x, bx = blockIdx.x - by * blocks_x, tid = threadIdx.x;
    {
        const int H0 = t.lv[0].H, W0 = t.lv[0].W, H1 = t.lv[1].H, W1 = t.lv[1].W;
        const int ly = tid >> 4, lx = tid & 15, i = 16 * by + ly, j = 16 * bx + lx;
        float a = 0.f, b = 0.f;
        if (i < H1 && j < W1) {
            const size_t o = (size_t)n * H0 * W0 + (size_t)(2 * i) * W0 + 2 * j;
            a = ((load1<T>(x + o) + load1<T>(x + o + 1)) + (load1<T>(x + o + W0) + load1<T>(x + o + W0 + 1))) * 0.25f;
            b = ((load1<T>(y + o) + load1<T>(y + o + 1)) + (load1<T>(y + o + W0) + load1<T>(y + o + W0 + 1))) * 0.25f;
            const size_t d = (size_t)t.lv[1].pix_off + (size_t)n * H1 * W1 + (size_t)i * W1 + j;
            pyr[d] = a; pyr[half + d] = b;
        }
        s1[0][ly][lx] = a; s1[1][ly][lx] = b;
    }
    if (t.levels <= 2) return;
    __syncthreads();
    if (tid < 64) {
        const int H2 = t.lv[2].H, W2 = t.lv[2].W, ly = tid >> 3, lx = tid & 7, i = 8 * by + ly, j = 8 * bx + lx;
        const float a = ((s1[0][2 * ly][2 * lx] + s1[0][2 * ly][2 * lx + 1]) + (s1[0][2 * ly + 1][2 * lx] + s1[0][2 * ly + 1][2 * lx + 1])) * 0.25f;
        const float b = ((s1[1][2 * ly][2 * lx] + s1[1][2 * ly][2 * lx + 1]) + (s1[1][2 * ly + 1][2 * lx] + s1[1][2 * ly + 1][2 * lx + 1])) * 0.25f;
        if (i < H2 && j < W2) {
            const size_t d = (size_t)t.lv[2].pix_off + (size_t)n * H2 * W2 + (size_t)i * W2 + j;
            pyr[d] = a; pyr[half + d] = b;
        }
        s2[0][ly][lx] = a; s2[1][ly][lx] = b;
    }
    if (t.levels <= 3) return;
    __syncthreads();
    if (tid < 16) {
        const int H3 = t.lv[3].H, W3 = t.lv[3].W, ly = tid >> 2, lx = tid & 3, i = 4 * by + ly, j = 4 * bx + lx;
        const float a = ((s2[0][2 * ly][2 * lx] + s2[0][2 * ly][2 * lx + 1]) + (s2[0][2 * ly + 1][2 * lx] + s2[0][2 * ly + 1][2 * lx + 1])) * 0.25f;
        const float b = ((s2[1][2 * ly][2 * lx] + s2[1][2 * ly][2 * lx + 1]) + (s2[1][2 * ly + 1][2 * lx] + s2[1][2 * ly + 1][2 * lx + 1])) * 0.25f;
        if (i < H3 && j < W3) {
            const size_t d = (size_t)t.lv[3].pix_off + (size_t)n * H3 * W3 + (size_t)i * W3 + j;
            pyr[d] = a; pyr[half + d] = b;
        }
        s3[0][ly][lx] = a; s3[1][ly][lx] = b;
    }
    if (t.levels <= 4) return;
    __syncthreads();
    if (tid < 4) {
        const int H4 = t.lv[4].H, W4 = t.lv[4].W, ly = tid >> 1, lx = tid & 1, i = 2 * by + ly, j = 2 * bx + lx;
        if (i < H4 && j < W4) {
            const float a = ((s3[0][2 * ly][2 * lx] + s3[0][2 * ly][2 * lx + 1]) + (s3[0][2 * ly + 1][2 * lx] + s3[0][2 * ly + 1][2 * lx + 1])) * 0.25f;
            const float b = ((s3[1][2 * ly][2 * lx] + s3[1][2 * ly][2 * lx + 1]) + (s3[1][2 * ly + 1][2 * lx] + s3[1][2 * ly + 1][2 * lx + 1])) * 0.25f;
            const size_t d = (size_t)t.lv[4].pix_off + (size_t)n * H4 * W4 + (size_t)i * W4 + j;
            pyr[d] = a; pyr[half + d] = b;
        }
    }
}

// ---------------------------------------------------------------------------------------- forward
// grid (tiles of positions of all levels, N).  part[n][tile] = the tile's sum of cs (levels below the last) or S (the last level); maps
// (when not null), per level three (N, H_j - 10, W_j - 10) fp32 planes: A, B, C as in ssim.hip on the last level, and for a cs level
// B = -cs / b2, C = 2 / b2, A = -2 mu_u B - mu_v C (cs does not depend on the means but through su2 = E[u^2] - mu_u^2, suv = E[uv] - mu_u mu_v).
template <typename T>
__global__ __launch_bounds__(256) void msssim_fwd_kernel(const T* __restrict__ x, const T* __restrict__ y, const float* __restrict__ pyr, long half,
                                                         SsimWin win, MsTable t, double* __restrict__ part, float* __restrict__ maps, int N) {
    __shared__ float su[SS_IH][SS_IW], sv[SS_IH][SS_IW];
    __shared__ float sh[5][SS_IH][SS_TW];
    __shared__ double red[4];
    using In = SsimIn<T>;
    const int n = blockIdx.y, tile = blockIdx.x;
    MsLevel me;
    const int level = ms_pick(t, tile, me);
    const int lt = tile - me.tile0, H = me.H, W = me.W;
    const int ty0 = (lt / me.tiles_x) * SS_TH, tx0 = (lt % me.tiles_x) * SS_TW;    // first output = first input pixel of the tile: inside the level
    const int Ho = H - SS_R, Wo = W - SS_R;
    const size_t first = (size_t)ty0 * W + tx0;
    float xc, yc;
    if (level == 0) {
        const T* xs = x + (size_t)n * H * W;
        const T* ys = y + (size_t)n * H * W;
        xc = load1<T>(xs + first); yc = load1<T>(ys + first);
        ssim_stage_pair<In, T>(xs, ys, H, W, ty0, tx0, xc, yc, su, sv);
    } else {
        const float* xs = pyr + me.pix_off + (size_t)n * H * W;
        const float* ys = xs + half;
        xc = xs[first]; yc = ys[first];
        ssim_stage_pair<In, float>(xs, ys, H, W, ty0, tx0, xc, yc, su, sv);
    }
    const float cu = In::centre(xc), cv = In::centre(yc);
    __syncthreads();
    ssim_hpass5(su, sv, sh, win);
    __syncthreads();
    const bool last = level == t.levels - 1;
    const int tx = threadIdx.x & (SS_TW - 1), tyb = threadIdx.x / SS_TW;
    const size_t plane = (size_t)Ho * Wo;
    float* mp = maps ? maps + me.map_off : nullptr;
    double acc = 0.0;
#pragma unroll
    for (int h = 0; h < SS_TH / 8; ++h) {
        const int ty = tyb + 8 * h, oy = ty0 + ty, ox = tx0 + tx;
        float m[5];
        ssim_vpass5(sh, ty, tx, win, m);
        if (oy < Ho && ox < Wo) {
            const float su2 = m[2] - m[0] * m[0], sv2 = m[3] - m[1] * m[1], suv = m[4] - m[0] * m[1];   // about (cu, cv): small numbers
            const float mu = cu + m[0], mv = cv + m[1];
            const float a2 = 2.f * suv + SS_C2, b2 = su2 + sv2 + SS_C2;
            float A, B, C;
            if (last) {                                                            // the full S, as ssim_fwd_kernel
                const float a1 = 2.f * mu * mv + SS_C1, b1 = mu * mu + mv * mv + SS_C1;
                const float inv = 1.f / (b1 * b2);
                const float S = a1 * a2 * inv;
                acc += (double)S;
                B = -S / b2; C = 2.f * a1 * inv;
                const float dm = (m[1] - m[0]) + (cv - cu);
                const float fmu = 2.f * dm * (mv * (mu + mv) + SS_C1) / (b1 * b1) * (a2 / b2);
                A = fmu - 2.f * mu * B - mv * C;
            } else {
                const float cs = a2 / b2;
                acc += (double)cs;
                B = -cs / b2; C = 2.f / b2;
                A = -2.f * mu * B - mv * C;
            }
            if (mp) {
                const size_t o = (size_t)n * plane + (size_t)oy * Wo + ox;
                mp[o] = A;
                mp[(size_t)N * plane + o] = B;
                mp[2 * (size_t)N * plane + o] = C;
            }
        }
    }
    const double s = block_sum4(acc, red);
    if (threadIdx.x == 0) part[(size_t)n * t.total + tile] = s;
}

// grid N.  Lane j adds level j's partials in index order (the levels side by side); thread 0 forms the clamped product.
// terms[n][j] = m_j (before the clamp); coef[n][j] (when not null) = d msssim[n] / d m_j = w_j msssim[n] / m_j, 0 where m_j < F.
__global__ __launch_bounds__(64) void msssim_fold_kernel(const double* __restrict__ part, MsTable t, MsWeights wt, float* __restrict__ msssim,
                                                         float* __restrict__ terms, float* __restrict__ coef) {
    __shared__ double sm[MS_MAXL];
    const int n = blockIdx.x;
    int start = 0, cnt = 0;
    double positions = 1.0;
#pragma unroll
    for (int j = 0; j < MS_MAXL; ++j)
        if (j < t.levels && (int)threadIdx.x == j) {
            start = t.lv[j].tile0; cnt = t.lv[j].tiles;
            positions = (double)(t.lv[j].H - SS_R) * (double)(t.lv[j].W - SS_R);
        }
    const double* p = part + (size_t)n * t.total + start;
    double s = 0.0;
#pragma unroll 8
    for (int i = 0; i < cnt; ++i) s += p[i];
    if (threadIdx.x < MS_MAXL) sm[threadIdx.x] = s / positions;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double prod = 1.0;
#pragma unroll
    for (int j = 0; j < MS_MAXL; ++j)
        if (j < t.levels) prod *= pow(fmax(sm[j], (double)MS_FLOOR), (double)wt.w[j]);
    msssim[n] = (float)prod;
#pragma unroll
    for (int j = 0; j < MS_MAXL; ++j)
        if (j < t.levels) {
            terms[(size_t)n * t.levels + j] = (float)sm[j];
            if (coef) coef[(size_t)n * t.levels + j] = sm[j] >= (double)MS_FLOOR ? (float)((double)wt.w[j] * prod / sm[j]) : 0.f;
        }
}

// ---------------------------------------------------------------------------------------- backward
// With G_j(p) = sum_q g(p - q) (A_j(q) + 2 u_j(p) B_j(q) + v_j(p) C_j(q)) (ssim_bwd_kernel's three correlations on level j's maps) and
// g_j = gout[n] coef[n][j] / P_j * G_j:  dx(p) = 1/2 sum_j 4^-j g_j(p >> j), over the levels whose field holds p >> j.
// FINAL = false: grid (tiles of pixels of levels 1.., N); writes g_j into gbuf (laid out as one image's part of the pyramid).
// FINAL = true:  grid (tiles of pixels of level 0, N); adds the coarse levels from gbuf and writes dx.
template <typename T, bool FINAL>
__global__ __launch_bounds__(256) void msssim_bwd_kernel(const T* __restrict__ x, const T* __restrict__ y, const float* __restrict__ pyr, long half,
                                                         const float* __restrict__ maps, const float* __restrict__ gout,
                                                         const float* __restrict__ coef, SsimWin win, MsTable t, float* __restrict__ gbuf,
                                                         T* __restrict__ dx, int N) {
    __shared__ float sm[3][SS_IH][SS_IW];
    __shared__ float sh[3][SS_IH][SS_TW];
    using In = SsimIn<T>;
    const int n = blockIdx.y, tile = FINAL ? (int)blockIdx.x : (int)blockIdx.x + t.lv[1].tile0;
    MsLevel me = t.lv[0];
    const int level = FINAL ? 0 : ms_pick(t, tile, me);
    const int lt = tile - me.tile0, H = me.H, W = me.W;
    const int py0 = (lt / me.tiles_x) * SS_TH, px0 = (lt % me.tiles_x) * SS_TW;    // first pixel of the tile: inside the level
    const int Ho = H - SS_R, Wo = W - SS_R;
    const size_t plane = (size_t)Ho * Wo, first = (size_t)py0 * W + px0;
    const T* xs0 = x + (size_t)n * H * W;                                          // (read when FINAL)
    const T* ys0 = y + (size_t)n * H * W;
    const float* xsj = pyr + me.pix_off + (size_t)n * H * W;                       // (read when not FINAL)
    const float* ysj = xsj + half;
    const float xc = FINAL ? load1<T>(xs0 + first) : xsj[first], yc = FINAL ? load1<T>(ys0 + first) : ysj[first];
    const float cu = In::centre(xc), cv = In::centre(yc);
    const float* mA = maps + me.map_off + (size_t)n * plane;
    const float* mB = mA + (size_t)N * plane;
    const float* mC = mB + (size_t)N * plane;

    ssim_stage_maps(mA, mB, mC, Ho, Wo, py0, px0, cu, cv, sm);
    __syncthreads();
    ssim_hpass3(sm, sh, win);
    __syncthreads();
    const int tx = threadIdx.x & (SS_TW - 1), tyb = threadIdx.x / SS_TW;
    const float scale = gout[n] * coef[(size_t)n * t.levels + level] / (float)plane;
#pragma unroll
    for (int h = 0; h < SS_TH / 8; ++h) {
        const int ty = tyb + 8 * h, py = py0 + ty, px = px0 + tx;
        float s0, s1, s2;
        ssim_vpass3(sh, ty, tx, win, s0, s1, s2);
        if (py < H && px < W) {
            const size_t o = (size_t)py * W + px;
            if (FINAL) {
                const float du = In::delta(load1<T>(xs0 + o), xc), dv = In::delta(load1<T>(ys0 + o), yc);
                float g = scale * fmaf(2.f * du, s1, fmaf(dv, s2, s0));
                float f = 0.25f;
#pragma unroll
                for (int k = 1; k < MS_MAXL; ++k, f *= 0.25f) {
                    const int qy = py >> k, qx = px >> k;
                    if (k < t.levels && qy < t.lv[k].H && qx < t.lv[k].W)          // (a dropped row or column: nothing from deeper levels)
                        g = fmaf(f, gbuf[t.lv[k].pix_off + ((size_t)n * t.lv[k].H + qy) * t.lv[k].W + qx], g);
                }
                store1<T>(dx + (size_t)n * H * W + o, In::delta(1.f, 0.f) * g);    // (du/dx = 1/2)
            } else {
                const float du = In::delta(xsj[o], xc), dv = In::delta(ysj[o], yc);
                gbuf[me.pix_off + (size_t)n * H * W + o] = scale * fmaf(2.f * du, s1, fmaf(dv, s2, s0));
            }
        }
    }
}

// ---------------------------------------------------------------------------------------- host
// the sizes of every level and the two tile tables; legal: 1 <= levels <= 5 and the last level holds a window
struct MsGeom {
    int levels, H[MS_MAXL], W[MS_MAXL];
    long pix[MS_MAXL], half;          // floats before level j (>= 1) in one image's part of the pyramid; that part's floats
    long map[MS_MAXL], maps;          // floats before level j's maps; all maps' floats
    long ftiles, btiles;              // tiles of positions / of pixels over all levels
};

MsGeom ms_geom(int N, int H, int W, int levels) {
    MsGeom g{};
    g.levels = levels;
    for (int j = 0; j < levels; ++j) {
        g.H[j] = H >> j; g.W[j] = W >> j;
        g.pix[j] = g.half; g.map[j] = g.maps;
        if (j) g.half += (long)N * g.H[j] * g.W[j];
        g.maps += 3L * N * (g.H[j] - SS_R) * (g.W[j] - SS_R);
        g.ftiles += ssim_tiles(g.H[j] - SS_R, g.W[j] - SS_R);
        g.btiles += ssim_tiles(g.H[j], g.W[j]);
    }
    return g;
}

MsTable ms_table(const MsGeom& g, bool positions) {
    MsTable t{};
    t.levels = g.levels;
    int tile0 = 0;
    for (int j = 0; j < g.levels; ++j) {
        const int h = positions ? g.H[j] - SS_R : g.H[j], w = positions ? g.W[j] - SS_R : g.W[j];
        t.lv[j] = MsLevel{g.H[j], g.W[j], tile0, (int)ssim_tiles(h, w), (int)ssim_tiles_x(w), 0, g.pix[j], g.map[j]};
        tile0 += t.lv[j].tiles;
    }
    t.total = tile0;
    return t;
}

inline bool ms_legal(int N, int H, int W, int levels) {
    return N > 0 && levels >= 1 && levels <= MS_MAXL && H > 0 && W > 0 && (H >> (levels - 1)) >= SS_TAPS && (W >> (levels - 1)) >= SS_TAPS;
}

// the checks every entry shares, after its own pointer and dtype checks: the levels, the weights (null: the entry takes none), the sizes
int ms_check(const char* name, int N, int H, int W, int levels, const float* weights) {
    if (levels < 1 || levels > MS_MAXL) S2E_FAIL(S2E_ERR_ARG, "%s: levels=%d (1 to %d levels expected)", name, levels, MS_MAXL);
    if (weights)
        for (int j = 0; j < levels; ++j)
            if (!(weights[j] > 0.f) || !__builtin_isfinite(weights[j]))
                S2E_FAIL(S2E_ERR_ARG, "%s: weights[%d]=%g (every weight must be positive and finite)", name, j, (double)weights[j]);
    const int Hl = H > 0 ? H >> (levels - 1) : 0, Wl = W > 0 ? W >> (levels - 1) : 0;
    if (Hl < SS_TAPS || Wl < SS_TAPS)
        S2E_FAIL(S2E_ERR_UNSUPPORTED, "%s: H=%d W=%d levels=%d (level %d is %d x %d: smaller than the 11 x 11 window, it has no position)", name, H, W,
                 levels, levels - 1, Hl, Wl);
    return s2e_check_image_batch(name, N, H, W);
}

template <typename T>
int msssim_fwd_launch(const char* name, const T* x, const T* y, int N, int H, int W, int levels, const float* weights, float* msssim, float* terms,
                      float* coef, float* maps, size_t maps_bytes, void* pyr, size_t pyr_bytes, void* ws, size_t ws_bytes, hipStream_t st) {
    if (const int rc = ms_check(name, N, H, W, levels, weights)) return rc;
    S2E_CHECK_BYTES(name, "workspace", ws_bytes, s2e_msssim_workspace_bytes(N, H, W, levels));
    S2E_CHECK_BYTES(name, "pyramid", pyr ? pyr_bytes : 0, s2e_msssim_pyramid_bytes(N, H, W, levels));
    if (maps) S2E_CHECK_BYTES(name, "maps", maps_bytes, s2e_msssim_maps_bytes(N, H, W, levels));
    const MsGeom g = ms_geom(N, H, W, levels);
    const MsTable t = ms_table(g, true);
    MsWeights wt{};
    for (int j = 0; j < levels; ++j) wt.w[j] = weights[j];
    if (levels > 1) {
        const int bx = (g.W[1] + 15) / 16, by = (g.H[1] + 15) / 16;
        msssim_pyramid_kernel<T><<<dim3(bx * by, N), 256, 0, st>>>(x, y, (float*)pyr, g.half, t, bx);
        S2E_CHECK_LAUNCH("msssim_pyramid_kernel");
    }
    msssim_fwd_kernel<T><<<dim3(t.total, N), 256, 0, st>>>(x, y, (const float*)pyr, g.half, ssim_window(), t, (double*)ws, maps, N);
    S2E_CHECK_LAUNCH("msssim_fwd_kernel");
    msssim_fold_kernel<<<N, 64, 0, st>>>((const double*)ws, t, wt, msssim, terms, coef);
    S2E_CHECK_LAUNCH("msssim_fold_kernel");
    return S2E_OK;
}

}  // namespace

extern "C" size_t s2e_msssim_workspace_bytes(int N, int H, int W, int levels) {
    if (!ms_legal(N, H, W, levels)) return 0;
    return (size_t)N * (size_t)ms_geom(N, H, W, levels).ftiles * sizeof(double);
}

extern "C" size_t s2e_msssim_pyramid_bytes(int N, int H, int W, int levels) {
    if (!ms_legal(N, H, W, levels)) return 0;
    return 2 * (size_t)ms_geom(N, H, W, levels).half * sizeof(float);
}

extern "C" size_t s2e_msssim_maps_bytes(int N, int H, int W, int levels) {
    if (!ms_legal(N, H, W, levels)) return 0;
    return (size_t)ms_geom(N, H, W, levels).maps * sizeof(float);
}

extern "C" int s2e_msssim_fwd(int dtype, const void* x, const void* y, int N, int H, int W, int levels, const float* weights, float* msssim,
                              float* terms, float* coef, float* maps, size_t maps_bytes, void* pyramid, size_t pyramid_bytes, void* workspace,
                              size_t workspace_bytes, void* stream) {
    if (!x || !y || !weights || !msssim || !terms || !coef || !workspace || N <= 0) S2E_FAIL(S2E_ERR_ARG, "s2e_msssim_fwd: bad argument");
    S2E_CHECK_DTYPE(dtype, "s2e_msssim_fwd");
    return s2e_with_dtype(dtype, "s2e_msssim_fwd", [&](auto t) { using T = decltype(t);
        return msssim_fwd_launch<T>("s2e_msssim_fwd", (const T*)x, (const T*)y, N, H, W, levels, weights, msssim, terms, coef, maps, maps_bytes, pyramid,
                                    pyramid_bytes, workspace, workspace_bytes, (hipStream_t)stream); });
}

extern "C" int s2e_msssim_u8(const uint8_t* a, const uint8_t* b, int N, int H, int W, int levels, const float* weights, float* msssim, float* terms,
                             void* pyramid, size_t pyramid_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    if (!a || !b || !weights || !msssim || !terms || !workspace || N <= 0) S2E_FAIL(S2E_ERR_ARG, "s2e_msssim_u8: bad argument");
    return msssim_fwd_launch<uint8_t>("s2e_msssim_u8", a, b, N, H, W, levels, weights, msssim, terms, nullptr, nullptr, 0, pyramid, pyramid_bytes,
                                      workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int s2e_msssim_bwd(int dtype, const void* x, const void* y, const void* pyramid, const float* maps, const float* coef, const float* gout,
                              int N, int H, int W, int levels, void* gbuf, size_t gbuf_bytes, void* dx, void* stream) {
    const char* name = "s2e_msssim_bwd";
    if (!x || !y || !maps || !coef || !gout || !dx || N <= 0) S2E_FAIL(S2E_ERR_ARG, "s2e_msssim_bwd: bad argument");
    S2E_CHECK_DTYPE(dtype, name);
    if (const int rc = ms_check(name, N, H, W, levels, nullptr)) return rc;
    const size_t need = s2e_msssim_pyramid_bytes(N, H, W, levels) / 2;
    if (need && !pyramid) S2E_FAIL(S2E_ERR_ARG, "s2e_msssim_bwd: bad argument");
    S2E_CHECK_BYTES(name, "gradient buffer", gbuf ? gbuf_bytes : 0, need);
    const MsGeom g = ms_geom(N, H, W, levels);
    const MsTable t = ms_table(g, false);
    hipStream_t st = (hipStream_t)stream;
    return s2e_with_dtype(dtype, name, [&](auto e) { using T = decltype(e);
        if (levels > 1) {
            msssim_bwd_kernel<T, false><<<dim3(t.total - t.lv[0].tiles, N), 256, 0, st>>>((const T*)x, (const T*)y, (const float*)pyramid, g.half, maps,
                                                                                         gout, coef, ssim_window(), t, (float*)gbuf, (T*)dx, N);
            S2E_CHECK_LAUNCH("msssim_bwd_kernel (coarse levels)");
        }
        msssim_bwd_kernel<T, true><<<dim3(t.lv[0].tiles, N), 256, 0, st>>>((const T*)x, (const T*)y, (const float*)pyramid, g.half, maps, gout, coef,
                                                                          ssim_window(), t, (float*)gbuf, (T*)dx, N);
        S2E_CHECK_LAUNCH("msssim_bwd_kernel (level 0)");
        return S2E_OK; });
}
