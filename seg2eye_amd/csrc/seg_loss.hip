// The eye segmenter's boundary-aware terms: signed Euclidean distance maps and the boundary band of a uint8 label map,
// and one fused loss -- boundary-weighted cross-entropy, generalised Dice, Kervadec's surface term -- that evaluates a pixel's softmax
// once for all three, with its gradient.
//
// s2e_seg_dist_maps  two launches, no atomics, integers until the last step: the same input gives the same bits.
//   column pass  a lane owns one (image, class, column): it walks the column down, then up, and keeps the vertical distance to the
//                nearest pixel of the class (low 16 bits) and to the nearest pixel outside it (high 16 bits); 0xFFFF: none in this
//                column.  Lanes of a wave own consecutive x: label loads and workspace stores coalesce.  workspace[n][y][c][x] uint32.
//   row pass     a workgroup owns one (image, row).  Four classes at a time it squares those column distances into LDS and every lane
//                takes min over x' of (x - x')^2 + g(x')^2, brute force: of the class's own set where l_p != c, of the complement
//                where l_p == c.  A set that is empty in the whole image leaves the sentinel: phi = +0.
// s2e_seg_loss_fwd   two launches in the pattern of s2e_seg_ce_fwd: grid.y = image, workgroups walk the image's pixels grid-stride and
//                store fp64 partials with plain stores; one workgroup folds them in index order and writes loss, terms and saved.
// s2e_seg_loss_bwd   one launch, the softmax recomputed; the per-image Dice coefficients come from `saved`.
#include "seg_pixel.h"
#include "seg_dist.h"

namespace {

constexpr int LOSS_BLOCKS = 512;                             // workgroups of the loss forward at most, over all images: two per CU
constexpr int LOSS_DEPTH = 2;                                // pixels of a lane whose loads are in flight together in the forward
constexpr int LOSS_HEAD = 4;                                 // partials ahead of the per-class ones: CE numerator, sum w, |P|, surface numerator

// ---------------------------------------------------------------------------------------- distance maps
// grid (ceil(W / 64), N, ncls), 64 threads.  ws[((n H + y) ncls + c) W + x] = d_in | d_out << 16, vertical distances in this column
__global__ __launch_bounds__(DIST_COL_THREADS) void seg_dist_col_kernel(const uint8_t* __restrict__ label, int H, int W, int ncls, uint32_t* __restrict__ ws) {
    const int x = blockIdx.x * DIST_COL_THREADS + threadIdx.x, n = blockIdx.y, c = blockIdx.z;
    if (x >= W) return;
    const uint8_t* lab = label + (size_t)n * H * W + x;
    uint32_t* col = ws + ((size_t)n * H * ncls + c) * W + x;
    const size_t pitch = (size_t)ncls * W;
    int in = -1, out = -1;                                   // the last row seen of the class / outside it; -1: none yet
    for (int y0 = 0; y0 < H; y0 += DIST_COL_DEPTH) {
        int l[DIST_COL_DEPTH];
#pragma unroll
        for (int u = 0; u < DIST_COL_DEPTH; ++u) l[u] = lab[(size_t)min(y0 + u, H - 1) * W];
#pragma unroll
        for (int u = 0; u < DIST_COL_DEPTH; ++u) {
            const int y = y0 + u;
            if (y < H) {
                if (l[u] == c) in = y; else out = y;
                col[y * pitch] = dist_to_last(y, in) | dist_to_last(y, out) << 16;
            }
        }
    }
    in = -1; out = -1;                                       // now the next row below
    for (int y0 = H - 1; y0 >= 0; y0 -= DIST_COL_DEPTH) {
        int l[DIST_COL_DEPTH];
        uint32_t v[DIST_COL_DEPTH];
#pragma unroll
        for (int u = 0; u < DIST_COL_DEPTH; ++u) {
            const int y = max(y0 - u, 0);
            l[u] = lab[(size_t)y * W];
            v[u] = col[y * pitch];
        }
#pragma unroll
        for (int u = 0; u < DIST_COL_DEPTH; ++u) {
            const int y = y0 - u;
            if (y >= 0) {
                if (l[u] == c) in = y; else out = y;
                const uint32_t di = min(v[u] & 0xFFFFu, dist_to_last(y, in));
                const uint32_t dn = min(v[u] >> 16, dist_to_last(y, out));
                col[y * pitch] = di | dn << 16;
            }
        }
    }
}

// grid (H, N), W rounded up to whole waves and at most 256 threads (a 40-pixel row takes one wave, not four).  phi (N, H, W, ncls) fp32;
// band (N, H, W) or NULL
__global__ __launch_bounds__(SEG_THREADS) void seg_dist_row_kernel(const uint8_t* __restrict__ label, const uint32_t* __restrict__ ws, int H, int W, int ncls,
                                                                   uint32_t r2, int vec, float* __restrict__ phi, uint8_t* __restrict__ band) {
    __shared__ u32x4_t s_in[DIST_MAX_SIDE];                  // [x'][j]: g^2 to class c0 + j, DIST_NONE where the column has none
    __shared__ uint32_t s_out[DIST_MAX_SIDE][4];             // the same to the complement of class c0 + j
    const int y = blockIdx.x, n = blockIdx.y;
    const size_t row = ((size_t)n * H + y) * W;
    const uint32_t* wrow = ws + row * ncls;
    for (int c0 = 0; c0 < ncls; c0 += 4) {
        if (c0) __syncthreads();
        for (int i = threadIdx.x; i < 4 * W; i += blockDim.x) {
            const int j = i / W, xs = i - j * W;             // consecutive lanes, consecutive x of one class: coalesced
            uint32_t a = DIST_NONE, b = DIST_NONE;
            if (c0 + j < ncls) {
                const uint32_t v = wrow[(size_t)(c0 + j) * W + xs], gi = v & 0xFFFFu, go = v >> 16;
                a = dist_sq16(gi);
                b = dist_sq16(go);
            }
            ((uint32_t*)s_in)[4 * xs + j] = a;
            s_out[xs][j] = b;
        }
        __syncthreads();
        for (int x = threadIdx.x; x < W; x += blockDim.x) {
            const int l = label[row + x];
            const int own = l - c0;                          // the slot of the pixel's own class in this group, if it is one of the four
            const bool has_own = own >= 0 && own < 4 && l < ncls;
            const int slot = has_own ? own : 0;
            uint32_t m[4] = {DIST_NONE, DIST_NONE, DIST_NONE, DIST_NONE}, mo = DIST_NONE;
            for (int xs = 0; xs < W; ++xs) {
                const uint32_t dx = (uint32_t)((x - xs) * (x - xs));
                const u32x4_t g = s_in[xs];
                m[0] = min(m[0], dx + g[0]);
                m[1] = min(m[1], dx + g[1]);
                m[2] = min(m[2], dx + g[2]);
                m[3] = min(m[3], dx + g[3]);
                mo = min(mo, dx + s_out[xs][slot]);
            }
            float f[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool mine = has_own && j == own;
                const uint32_t mm = mine ? mo : m[j];
                f[j] = mm >= DIST_NONE ? 0.f : mine ? 1.f - sqrtf((float)mm) : sqrtf((float)mm);
            }
            float* out = phi + (row + x) * ncls + c0;
            if (vec) {
                *(f32x4_t*)out = f32x4_t{f[0], f[1], f[2], f[3]};
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (c0 + j < ncls) out[j] = f[j];
            }
            if (band) {
                if (has_own) band[row + x] = (mo < DIST_NONE && mo <= r2) ? 1 : 0;
                else if (l >= ncls && c0 == 0) band[row + x] = 0;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------- the fused loss
// phi of pixel p: f[c] for c < ncls (the slots behind are never used); vec: ncls == 4 and the map is 16-byte aligned, one load
template <int NS>
__device__ __forceinline__ void loss_load_phi(const float* __restrict__ phi, size_t p, int ncls, int vec, float* f) {
    if (vec) {
        const f32x4_t v = *(const f32x4_t*)(phi + 4 * p);
        f[0] = v[0]; f[1] = v[1]; f[2] = v[2]; f[3] = v[3];
    } else {
#pragma unroll
        for (int c = 0; c < NS; ++c) f[c] = c < ncls ? phi[p * ncls + (c < ncls ? c : 0)] : 0.f;
    }
}

// grid (blocks, N), 256 threads; workgroup (b, n) walks pixels b 256 + t, + blocks 256, ... of image n.  K = 4 + 3 ncls doubles at
// part[(n blocks + b) K]: {sum w b (lse - z_l), sum w, |P|, sum_c p phi} then per class {I, sum p, G}, over the counted pixels.
// phi_vec: phi is read as one 16-byte load (ncls == 4, aligned); phi / band NULL: the term is off.
template <typename T, int MODE>
__global__ __launch_bounds__(SEG_THREADS) void seg_loss_fwd_kernel(const T* __restrict__ x, const uint8_t* __restrict__ label, const float* __restrict__ weights,
                                                                   const float* __restrict__ phi, const uint8_t* __restrict__ band, int HW, int C, int ncls,
                                                                   int phi_vec, float alpha, double* __restrict__ part) {
    constexpr int NS = SegSlots<MODE>::N;
    __shared__ float sw[SEG_MAX_CLS];
    __shared__ double red[LOSS_HEAD + 3 * SEG_MAX_CLS][SEG_THREADS / 64];
    if (threadIdx.x < SEG_MAX_CLS) sw[threadIdx.x] = (int)threadIdx.x < ncls ? weights[threadIdx.x] : 0.f;
    __syncthreads();
    const size_t base = (size_t)blockIdx.y * HW;
    double num = 0.0, den = 0.0, cnt = 0.0, surf = 0.0, I[NS], S[NS], G[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) { I[c] = 0.0; S[c] = 0.0; G[c] = 0.0; }
    const int stride = gridDim.x * SEG_THREADS;
    for (long p0 = (long)blockIdx.x * SEG_THREADS + threadIdx.x; p0 < HW; p0 += (long)LOSS_DEPTH * stride) {
        int l[LOSS_DEPTH], bd[LOSS_DEPTH];
        float z[LOSS_DEPTH][NS], f[LOSS_DEPTH][NS];
#pragma unroll
        for (int u = 0; u < LOSS_DEPTH; ++u) {                // a pixel past the image re-reads its last pixel and counts as ignored
            const long p = p0 + (long)u * stride;
            const size_t pc = base + (size_t)(p < HW ? p : HW - 1);
            l[u] = p < HW ? (int)label[pc] : 255;
            bd[u] = band ? (int)band[pc] : 0;
            seg_load<T, MODE>(x, pc, C, ncls, z[u]);
            if (phi) loss_load_phi<NS>(phi, pc, ncls, phi_vec, f[u]);
        }
#pragma unroll
        for (int u = 0; u < LOSS_DEPTH; ++u) {
            if (l[u] >= ncls) continue;
            float e[NS], m;
            const float s = seg_softmax_terms<NS>(z[u], ncls, m, e);
            const float inv = 1.f / s;
            float zl = z[u][0];
#pragma unroll
            for (int c = 1; c < NS; ++c) zl = c == l[u] ? z[u][c] : zl;
            const double w = (double)sw[l[u]];
            num += w * (double)(1.f + alpha * (float)bd[u]) * ((double)logf(s) - (double)(zl - m));
            den += w;
            cnt += 1.0;
#pragma unroll
            for (int c = 0; c < NS; ++c) {
                if (c < ncls) {
                    const double pc = (double)(e[c] * inv);
                    S[c] += pc;
                    if (c == l[u]) { I[c] += pc; G[c] += 1.0; }
                    if (phi) surf += pc * (double)f[u][c];
                }
            }
        }
    }
    double* out = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (LOSS_HEAD + 3 * ncls);
    const double t0 = block_sum4(num, red[0]), t1 = block_sum4(den, red[1]), t2 = block_sum4(cnt, red[2]), t3 = block_sum4(surf, red[3]);
    if (threadIdx.x == 0) { out[0] = t0; out[1] = t1; out[2] = t2; out[3] = t3; }
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        if (c < ncls) {                                      // (uniform: every lane takes the same barriers)
            const double a = block_sum4(I[c], red[LOSS_HEAD + 3 * c]), b = block_sum4(S[c], red[LOSS_HEAD + 3 * c + 1]),
                         g = block_sum4(G[c], red[LOSS_HEAD + 3 * c + 2]);
            if (threadIdx.x == 0) { out[LOSS_HEAD + 3 * c] = a; out[LOSS_HEAD + 3 * c + 1] = b; out[LOSS_HEAD + 3 * c + 2] = g; }
        }
    }
}

// One workgroup.  tot: N rows of K + 3 doubles (the image's K totals, then A_n, D_n, dice_n).
//   1  every (image, k): the sum of the image's partials in index order
//   2  every image: A = sum v I, D = sum v U with U = sum p + G, v = 1 / G^2 where G > 0; dice = 1 - 2 A / D
//   3  four lanes, one each: the sums over the images, in index order, of the CE numerator, sum w, |P|, the surface numerator;
//      a fifth: the number of images with a counted pixel and the sum of their dice
//   4  loss, terms, and for the backward saved[(n 2 + 0) ncls + c] = kI, saved[(n 2 + 1) ncls + c] = kU, then 1 / sum w, 1 / (|P| ncls)
__global__ __launch_bounds__(SEG_THREADS) void seg_loss_fold_kernel(const double* __restrict__ part, double* tot, int N, int blocks, int ncls,
                                                                    float lambda_ce, float lambda_dice, float lambda_surf, float* __restrict__ loss,
                                                                    float* __restrict__ terms, float* __restrict__ saved) {
    __shared__ double g[6];
    const int K = LOSS_HEAD + 3 * ncls, KT = K + 3;
    for (long i = threadIdx.x; i < (long)N * K; i += SEG_THREADS) {
        const long n = i / K, k = i - n * K;
        const double* src = part + (size_t)n * blocks * K + k;
        double s = 0.0;
        for (int b = 0; b < blocks; ++b) s += src[(size_t)b * K];
        tot[n * KT + k] = s;
    }
    __syncthreads();
    for (int n = threadIdx.x; n < N; n += SEG_THREADS) {
        double* t = tot + (size_t)n * KT;
        double A = 0.0, D = 0.0;
        for (int c = 0; c < ncls; ++c) {
            const double Ic = t[LOSS_HEAD + 3 * c], Sc = t[LOSS_HEAD + 3 * c + 1], Gc = t[LOSS_HEAD + 3 * c + 2];
            const double v = Gc > 0.0 ? 1.0 / (Gc * Gc) : 0.0;
            A += v * Ic;
            D += v * (Sc + Gc);
        }
        t[K] = A;
        t[K + 1] = D;
        t[K + 2] = t[2] > 0.0 ? 1.0 - 2.0 * A / D : 0.0;
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        if (wave < 4) {
            const int k = wave;
            double s = 0.0;
            for (int n = 0; n < N; ++n) s += tot[(size_t)n * KT + k];
            g[k] = s;
        }
        if (wave == 0) {                                     // (the first wave again: a workgroup has four)
            double nc = 0.0, ds = 0.0;
            for (int n = 0; n < N; ++n)
                if (tot[(size_t)n * KT + 2] > 0.0) { nc += 1.0; ds += tot[(size_t)n * KT + K + 2]; }
            g[4] = nc;
            g[5] = ds;
        }
    }
    __syncthreads();
    const double ncnt = g[4];
    const double inv_w = g[1] > 0.0 ? 1.0 / g[1] : 0.0, s_surf = g[2] > 0.0 ? 1.0 / (g[2] * (double)ncls) : 0.0;
    if (threadIdx.x == 0) {
        const double ce = g[0] * inv_w, dice = ncnt > 0.0 ? g[5] / ncnt : 0.0, surf = g[3] * s_surf;
        terms[0] = (float)ce;
        terms[1] = (float)dice;
        terms[2] = (float)surf;
        loss[0] = (float)((double)lambda_ce * ce + (double)lambda_dice * dice + (double)lambda_surf * surf);
        saved[(size_t)N * 2 * ncls] = (float)inv_w;
        saved[(size_t)N * 2 * ncls + 1] = (float)s_surf;
    }
    for (long i = threadIdx.x; i < (long)N * ncls; i += SEG_THREADS) {
        const long n = i / ncls, c = i - n * ncls;
        const double* t = tot + (size_t)n * KT;
        double kI = 0.0, kU = 0.0;
        if (t[2] > 0.0) {
            const double Gc = t[LOSS_HEAD + 3 * c + 2], v = Gc > 0.0 ? 1.0 / (Gc * Gc) : 0.0, A = t[K], D = t[K + 1];
            const double f = (double)lambda_dice / ncnt;
            kI = -f * 2.0 * v / D;
            kU = f * 2.0 * A * v / (D * D);
        }
        saved[(n * 2 + 0) * ncls + c] = (float)kI;
        saved[(n * 2 + 1) * ncls + c] = (float)kU;
    }
}

// grid (ceil(HW / 256), N), one pixel per lane:
//   a_c = kI_nc [c == l] + kU_nc + lambda_surf s phi_c;   dz_c = g (p_c sum_k p_k (a_c - a_k) + lambda_ce w_l b / sum w (p_c - [c == l]))
// (sum_k p_k (a_c - a_k) equals the header's a_c - sum_k a_k p_k, since sum p = 1).  +0 for an ignored pixel and behind ncls
template <typename T, int MODE>
__global__ __launch_bounds__(SEG_THREADS) void seg_loss_bwd_kernel(const T* __restrict__ x, const uint8_t* __restrict__ label, const float* __restrict__ weights,
                                                                   const float* __restrict__ phi, const uint8_t* __restrict__ band, const float* __restrict__ saved,
                                                                   const float* __restrict__ gloss, int N, int HW, int C, int ncls, int phi_vec,
                                                                   float lambda_ce, float lambda_surf, float alpha, T* __restrict__ dx) {
    constexpr int NS = SegSlots<MODE>::N;
    __shared__ float sw[SEG_MAX_CLS], skI[SEG_MAX_CLS], skU[SEG_MAX_CLS];
    const int n = blockIdx.y;
    if (threadIdx.x < SEG_MAX_CLS) {
        const bool on = (int)threadIdx.x < ncls;
        sw[threadIdx.x] = on ? weights[threadIdx.x] : 0.f;
        skI[threadIdx.x] = on ? saved[((size_t)n * 2 + 0) * ncls + threadIdx.x] : 0.f;
        skU[threadIdx.x] = on ? saved[((size_t)n * 2 + 1) * ncls + threadIdx.x] : 0.f;
    }
    __syncthreads();
    const int q = blockIdx.x * SEG_THREADS + threadIdx.x;
    if (q >= HW) return;
    const size_t p = (size_t)n * HW + q;
    const int l = label[p];
    float d[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) d[c] = 0.f;
    if (l < ncls) {
        const float g = gloss[0];
        const float ce = lambda_ce * sw[l] * (1.f + (band ? alpha * (float)band[p] : 0.f)) * saved[(size_t)N * 2 * ncls];
        const float ks = lambda_surf * saved[(size_t)N * 2 * ncls + 1];
        float z[NS], e[NS], f[NS], a[NS], m;
        seg_load<T, MODE>(x, p, C, ncls, z);
        if (phi) loss_load_phi<NS>(phi, p, ncls, phi_vec, f);
        const float inv = 1.f / seg_softmax_terms<NS>(z, ncls, m, e);
        // With sum p = 1, a_c - sum_k a_k p_k = sum_k p_k (a_c - a_k), and that is the form taken: where classes tie (bf16 logits near
        // 80 stand 0.5 apart) or the softmax is one-hot, the plain form leaves a rounding residue of the size of a where the sum is 0,
        // the pairwise form cancels exactly.  a is taken relative to the class of the largest logit, piece by piece, so that equal
        // pieces drop out before they are rounded together; likewise p_l - 1 is -(the sum of the other classes' p).
        int top = 0;
        float f_top = phi ? f[0] : 0.f;
#pragma unroll
        for (int c = 1; c < NS; ++c)
            if (c < ncls && z[c] == m) { top = c; f_top = phi ? f[c] : 0.f; }
        const float kU_top = skU[top], kI_l = skI[l], kI_top = top == l ? kI_l : 0.f;
        float others = 0.f;
#pragma unroll
        for (int c = 0; c < NS; ++c) {
            e[c] *= inv;
            a[c] = c < ncls ? (skU[c] - kU_top) + ((c == l ? kI_l : 0.f) - kI_top) + (phi ? ks * (f[c] - f_top) : 0.f) : 0.f;
            others += c == l ? 0.f : e[c];
        }
#pragma unroll
        for (int c = 0; c < NS; ++c) {
#pragma clang fp contract(off)                               // (a fused multiply-add keeps one product unrounded: tied classes would not cancel)
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < NS; ++k) acc += e[k] * (a[c] - a[k]);    // (e is 0 behind ncls)
            d[c] = c < ncls ? g * (e[c] * acc + ce * (c == l ? -others : e[c])) : 0.f;
        }
    }
    seg_store<T, MODE>(dx, p, C, ncls, d);
}

// ---------------------------------------------------------------------------------------- launchers
int loss_blocks(int N, long HW) {
    const long want = (HW + SEG_THREADS - 1) / SEG_THREADS, cap = LOSS_BLOCKS / N > 1 ? LOSS_BLOCKS / N : 1;
    return (int)(want < cap ? want : cap);
}

bool loss_scalar_ok(float v) { return v >= 0.f && v <= 3.0e38f; }     // finite and not negative (a NaN fails both comparisons)

// what forward and backward check alike after their own pointer check
int loss_check(const char* name, int dtype, const void* phi, const void* band, int N, int H, int W, int C, int ncls, float lambda_ce, float lambda_dice,
               float lambda_surf, float alpha) {
    if (const int rc = seg_check(name, dtype, N, H, W, C, ncls)) return rc;
    if (const int rc = s2e_check_image_batch(name, N, H, W)) return rc;
    if (!loss_scalar_ok(lambda_ce) || !loss_scalar_ok(lambda_dice) || !loss_scalar_ok(lambda_surf) || !loss_scalar_ok(alpha))
        S2E_FAIL(S2E_ERR_ARG, "%s: lambda_ce=%g lambda_dice=%g lambda_surf=%g edge_alpha=%g (finite and not negative)", name, lambda_ce, lambda_dice, lambda_surf, alpha);
    if (!phi && lambda_surf != 0.f) S2E_FAIL(S2E_ERR_ARG, "%s: lambda_surf=%g without phi", name, lambda_surf);
    if (!band && alpha != 0.f) S2E_FAIL(S2E_ERR_ARG, "%s: edge_alpha=%g without band", name, alpha);
    return S2E_OK;
}

}  // namespace

extern "C" size_t s2e_seg_dist_workspace_bytes(int N, int H, int W, int ncls) {
    if (N < 1 || H < 1 || W < 1 || ncls < 1 || ncls > SEG_MAX_CLS || H > DIST_MAX_SIDE || W > DIST_MAX_SIDE || N > 65535 ||
        (long)N * H * W * ncls >= (1L << 31))
        return 0;
    return (size_t)N * H * W * ncls * sizeof(uint32_t);
}

extern "C" int s2e_seg_dist_maps(const uint8_t* label, int N, int H, int W, int ncls, int radius, float* phi, uint8_t* band, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    const char* name = "s2e_seg_dist_maps";
    if (!label || !phi || !workspace) S2E_FAIL(S2E_ERR_ARG, "%s: bad argument", name);
    const size_t need = s2e_seg_dist_workspace_bytes(N, H, W, ncls);     // (0 for a shape the checks below refuse)
    S2E_CHECK_BYTES(name, "workspace", workspace_bytes, need);
    if (((uintptr_t)workspace & 3) || ((uintptr_t)phi & 3)) S2E_FAIL(S2E_ERR_ARG, "%s: workspace and phi must be 4-byte aligned", name);
    if (N < 1 || H < 1 || W < 1) S2E_FAIL(S2E_ERR_ARG, "%s: N=%d H=%d W=%d (every size must be at least 1)", name, N, H, W);
    if (radius < 0) S2E_FAIL(S2E_ERR_ARG, "%s: radius=%d (0 or more)", name, radius);
    if (ncls < 1 || ncls > SEG_MAX_CLS) S2E_FAIL(S2E_ERR_UNSUPPORTED, "%s: ncls=%d (1 to %d classes)", name, ncls, SEG_MAX_CLS);
    if (H > DIST_MAX_SIDE || W > DIST_MAX_SIDE) S2E_FAIL(S2E_ERR_UNSUPPORTED, "%s: H=%d W=%d (each at most %d)", name, H, W, DIST_MAX_SIDE);
    if (const int rc = s2e_check_image_batch(name, N, H, W)) return rc;
    if ((long)N * H * W * ncls >= (1L << 31))
        S2E_FAIL(S2E_ERR_UNSUPPORTED, "%s: N=%d H=%d W=%d ncls=%d is beyond the index limit (N H W ncls < 2^31)", name, N, H, W, ncls);
    hipStream_t st = (hipStream_t)stream;
    seg_dist_col_kernel<<<dim3(ceil_div(W, DIST_COL_THREADS), N, ncls), DIST_COL_THREADS, 0, st>>>(label, H, W, ncls, (uint32_t*)workspace);
    S2E_CHECK_LAUNCH("seg_dist_col_kernel");
    const long r = radius < 2048 ? radius : 2048;                        // (r^2 beyond 2 * 1023^2 already takes every pixel that has a distance)
    const int vec = ncls == 4 && ((uintptr_t)phi & 15) == 0;            // a pixel's four phi as one 16-byte store
    const int row_threads = dist_row_threads(W, SEG_THREADS);
    seg_dist_row_kernel<<<dim3(H, N), row_threads, 0, st>>>(label, (const uint32_t*)workspace, H, W, ncls, (uint32_t)(r * r), vec, phi, band);
    S2E_CHECK_LAUNCH("seg_dist_row_kernel");
    return S2E_OK;
}

extern "C" size_t s2e_seg_loss_workspace_bytes(int N, int H, int W, int ncls) {
    if (N < 1 || H < 1 || W < 1 || ncls < 1 || ncls > SEG_MAX_CLS || N > 65535 || (long)N * H * W >= (1L << 31)) return 0;
    const size_t K = LOSS_HEAD + 3 * (size_t)ncls;
    return ((size_t)N * loss_blocks(N, (long)H * W) * K + (size_t)N * (K + 3)) * sizeof(double);
}

extern "C" int s2e_seg_loss_fwd(int dtype, const void* logits, const uint8_t* label, const float* weights, const float* phi, const uint8_t* band,
                                int N, int H, int W, int C, int ncls, float lambda_ce, float lambda_dice, float lambda_surf, float edge_alpha,
                                float* loss, float* terms, float* saved, void* workspace, size_t workspace_bytes, void* stream) {
    const char* name = "s2e_seg_loss_fwd";
    if (!logits || !label || !weights || !loss || !terms || !saved) S2E_FAIL(S2E_ERR_ARG, "%s: bad argument", name);
    if (const int rc = loss_check(name, dtype, phi, band, N, H, W, C, ncls, lambda_ce, lambda_dice, lambda_surf, edge_alpha)) return rc;
    const size_t need = s2e_seg_loss_workspace_bytes(N, H, W, ncls);
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 7))
        S2E_FAIL(S2E_ERR_ARG, "%s: workspace of %zu bytes, needs %zu (8-byte aligned)", name, workspace ? workspace_bytes : (size_t)0, need);
    const int HW = H * W, blocks = loss_blocks(N, HW), K = LOSS_HEAD + 3 * ncls;
    if (lambda_surf == 0.f) phi = nullptr;                               // a term that is off reads nothing: the same bits with and without its input
    if (edge_alpha == 0.f) band = nullptr;
    const int phi_vec = phi && ncls == 4 && ((uintptr_t)phi & 15) == 0;
    double* part = (double*)workspace;
    double* tot = part + (size_t)N * blocks * K;
    hipStream_t st = (hipStream_t)stream;
    const int rc = seg_dispatch(dtype, seg_mode(dtype, C, logits), name, [&](auto t, auto mode) { using T = decltype(t);
        seg_loss_fwd_kernel<T, decltype(mode)::value><<<dim3(blocks, N), SEG_THREADS, 0, st>>>((const T*)logits, label, weights, phi, band, HW, C, ncls, phi_vec,
                                                                                              edge_alpha, part);
        S2E_CHECK_LAUNCH("seg_loss_fwd_kernel"); return S2E_OK; });
    if (rc) return rc;
    seg_loss_fold_kernel<<<1, SEG_THREADS, 0, st>>>(part, tot, N, blocks, ncls, lambda_ce, lambda_dice, lambda_surf, loss, terms, saved);
    S2E_CHECK_LAUNCH("seg_loss_fold_kernel");
    return S2E_OK;
}

extern "C" int s2e_seg_loss_bwd(int dtype, const void* logits, const uint8_t* label, const float* weights, const float* phi, const uint8_t* band,
                                const float* saved, const float* gloss, int N, int H, int W, int C, int ncls, float lambda_ce, float lambda_surf,
                                float edge_alpha, void* dlogits, void* stream) {
    const char* name = "s2e_seg_loss_bwd";
    if (!logits || !label || !weights || !saved || !gloss || !dlogits) S2E_FAIL(S2E_ERR_ARG, "%s: bad argument", name);
    if (const int rc = loss_check(name, dtype, phi, band, N, H, W, C, ncls, lambda_ce, 0.f, lambda_surf, edge_alpha)) return rc;
    const int HW = H * W;
    if (lambda_surf == 0.f) phi = nullptr;
    if (edge_alpha == 0.f) band = nullptr;
    const int phi_vec = phi && ncls == 4 && ((uintptr_t)phi & 15) == 0;
    hipStream_t st = (hipStream_t)stream;
    return seg_dispatch(dtype, seg_mode(dtype, C, logits, dlogits), name, [&](auto t, auto mode) { using T = decltype(t);
        seg_loss_bwd_kernel<T, decltype(mode)::value><<<dim3(ceil_div(HW, SEG_THREADS), N), SEG_THREADS, 0, st>>>(
            (const T*)logits, label, weights, phi, band, saved, gloss, N, HW, C, ncls, phi_vec, lambda_ce, lambda_surf, edge_alpha, (T*)dlogits);
        S2E_CHECK_LAUNCH("seg_loss_bwd_kernel"); return S2E_OK; });
}
