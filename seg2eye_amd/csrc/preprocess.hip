// Device-side preprocessing of OpenEDS frames: Pillow's bicubic resize of 8-bit single-channel images, bit for bit,
// followed by the horizontal flip and the [0, 255] -> [-1, 1] conversion; and cv2's nearest resize of the label maps.
//
// The rule (Pillow, src/libImaging/Resample.c, 8 bits per channel; the tables are built on the host, ops/preprocess.py):
//   per axis: output index i reads `count` source pixels from `xmin` on, bounds[i] = {xmin, count}, with the fixed-point taps
//             k[i][0..count) (2^22 = 1.0; rows of `ksize` = 2 * ceil(2 * max(in / out, 1)) + 1 ints, zero past `count`)
//   a pass  : clamp((2^21 + sum pixel * k) >> 22, 0, 255) in 32-bit integers, stored as uint8
//   order   : the horizontal pass, then the vertical pass on its uint8 result; a pass whose size does not change is skipped
//   flip    : out[y][x] = r[y][Wo - 1 - x] of the RESULT r;  float value: lut[r] (256 fp32, filled by the host)
//
// Shape: one workgroup (256 threads) per band of `bh` output rows of one frame.
//   1. the band's source rows -- one contiguous byte range of the frame -- go to LDS image S with 16-byte loads (byte loads for
//      the chunks that cross the ends of the tensor); S keeps the range's offset inside its first 16 bytes, so no row is re-aligned;
//   2. the horizontal pass writes LDS image T: rows x TP bytes (TP = Wo rounded up to 4), one dword (4 pixels) per work item;
//   3. the vertical pass reads one dword of T per tap (lanes read consecutive dwords: conflict-free ds_read_b32), clamps, flips,
//      looks the four values up in the LDS copy of the table and stores 16 bytes of fp32 (+ 4 bytes of uint8) per lane.
// LDS budget, chosen by the host (plan_band): 1024 (table) + rows * W + 30 rounded up to 16 (S: the range's lead-in and its rounding
// to whole 16-byte chunks) + rows * TP (T) bytes, where rows is the most source rows a band needs.  The band height is the largest
// of 1..16 that keeps this within 32 KiB (several workgroups per CU and, at the training sizes, 16-20 bands per frame); when not
// even one row fits, band height 1 may take up to 64 KiB -- at 640 x 400 that admits every ksize up to about 97 -- and past that
// the entry point returns S2E_ERR_UNSUPPORTED.
// No MFMA, no workspace, no atomics; every index read from a table is clamped to the frame before it is used.
#include "common.h"

namespace {

constexpr int PREC = 22;
constexpr int THREADS = 256;
constexpr int LDS_PREFERRED = 32 * 1024, LDS_MAX = 64 * 1024;
constexpr int LUT_BYTES = 256 * 4;

struct BicubicArgs {
    const uint8_t* src; const uint8_t* flip;
    const int32_t* kx; const int32_t* bx; const int32_t* ky; const int32_t* by;
    const float* lut; float* out; uint8_t* out_u8;
    long total;                 // bytes of src: M * H * W
    int H, W, Ho, Wo, ksx, ksy, bh, rows_max, TP, s_bytes;
};

__device__ __forceinline__ int clip8(int acc) {
    const int v = acc >> PREC;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__global__ __launch_bounds__(THREADS) void resize_bicubic_u8_kernel(const BicubicArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    float* lut = (float*)smem;
    const int tid = threadIdx.x, frame = blockIdx.y;
    const int oy0 = blockIdx.x * a.bh, oy1 = min(oy0 + a.bh, a.Ho);
    const bool hpass = a.kx != nullptr, vpass = a.ky != nullptr;
    // the band's source rows [r0, r1)
    int r0 = oy0, r1 = oy1;
    if (vpass) {
        r0 = a.by[2 * oy0];
        r1 = a.by[2 * (oy1 - 1)] + a.by[2 * (oy1 - 1) + 1];
    }
    r0 = max(0, min(r0, a.H - 1));
    r1 = max(r0 + 1, min(min(r1, a.H), r0 + a.rows_max));
    const int rows = r1 - r0;
    uint8_t* S = smem + LUT_BYTES;                                  // the source byte range, at its offset within 16 bytes
    uint8_t* T = S + a.s_bytes;                                     // rows x TP
    for (int i = tid; i < 256; i += THREADS) lut[i] = a.lut[i];

    // ---- 1. source rows -> S
    const long g_begin = ((long)frame * a.H + r0) * a.W, g_end = g_begin + (long)rows * a.W;   // byte offsets into src
    const int lead = (int)((uintptr_t)(a.src + g_begin) & 15);
    const long c_begin = g_begin - lead;                            // 16-byte aligned address; may lie before the tensor
    const int chunks = (int)((g_end - c_begin + 15) >> 4);
    for (int c = tid; c < chunks; c += THREADS) {
        const long o = c_begin + 16L * c;
        if (o >= 0 && o + 16 <= a.total) {
            *(u32x4_t*)(S + 16 * c) = *(const u32x4_t*)(a.src + o);
        } else {
            for (int j = 0; j < 16; ++j)
                S[16 * c + j] = (o + j >= 0 && o + j < a.total) ? a.src[o + j] : (uint8_t)0;
        }
    }
    __syncthreads();
    const uint8_t* Srow0 = S + lead;

    // ---- 2. horizontal pass: S -> T, four output pixels (one dword) per item
    const int nq = a.TP >> 2;
    for (int i = tid; i < rows * nq; i += THREADS) {
        const int r = i / nq, q = i - r * nq;
        const uint8_t* srow = Srow0 + (size_t)r * a.W;
        uint32_t packed = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ox = 4 * q + j;
            int v = 0;
            if (ox < a.Wo) {
                if (hpass) {
                    const int xmin = max(0, min(a.bx[2 * ox], a.W));
                    const int cnt = max(0, min(min(a.bx[2 * ox + 1], a.ksx), a.W - xmin));
                    const int32_t* k = a.kx + (size_t)ox * a.ksx;
                    int acc = 1 << (PREC - 1);
                    for (int t = 0; t < cnt; ++t) acc += (int)srow[xmin + t] * k[t];
                    v = clip8(acc);
                } else {
                    v = srow[ox];
                }
            }
            packed |= (uint32_t)v << (8 * j);
        }
        *(uint32_t*)(T + (size_t)r * a.TP + 4 * q) = packed;
    }
    __syncthreads();

    // ---- 3. vertical pass out of T, flip, table, store
    const bool flip = a.flip[frame] != 0;
    const size_t obase = (size_t)frame * a.Ho * a.Wo;
    const bool vec = (a.Wo & 3) == 0 && ((uintptr_t)a.out & 15) == 0 && (!a.out_u8 || ((uintptr_t)a.out_u8 & 3) == 0);
    for (int i = tid; i < (oy1 - oy0) * nq; i += THREADS) {
        const int ry = i / nq, q = i - ry * nq, oy = oy0 + ry;
        int v[4];
        if (vpass) {
            const int ymin = max(r0, min(a.by[2 * oy], r1));
            const int cnt = max(0, min(min(a.by[2 * oy + 1], a.ksy), r1 - ymin));
            const int32_t* k = a.ky + (size_t)oy * a.ksy;
            const uint32_t* col = (const uint32_t*)(T + (size_t)(ymin - r0) * a.TP) + q;
            int acc0 = 1 << (PREC - 1), acc1 = acc0, acc2 = acc0, acc3 = acc0;
            for (int t = 0; t < cnt; ++t) {
                const uint32_t d = col[(size_t)t * nq];
                const int w = k[t];
                acc0 += (int)(d & 255u) * w;
                acc1 += (int)((d >> 8) & 255u) * w;
                acc2 += (int)((d >> 16) & 255u) * w;
                acc3 += (int)(d >> 24) * w;
            }
            v[0] = clip8(acc0); v[1] = clip8(acc1); v[2] = clip8(acc2); v[3] = clip8(acc3);
        } else {
            const uint32_t d = *((const uint32_t*)(T + (size_t)ry * a.TP) + q);
            v[0] = d & 255u; v[1] = (d >> 8) & 255u; v[2] = (d >> 16) & 255u; v[3] = d >> 24;
        }
        const size_t row = obase + (size_t)oy * a.Wo;
        if (vec) {                                                   // (Wo % 4 == 0: all four pixels exist)
            const int x0 = flip ? a.Wo - 4 - 4 * q : 4 * q;
            if (flip) { const int t0 = v[0], t1 = v[1]; v[0] = v[3]; v[1] = v[2]; v[2] = t1; v[3] = t0; }
            const f32x4_t f = {lut[v[0]], lut[v[1]], lut[v[2]], lut[v[3]]};
            *(f32x4_t*)(a.out + row + x0) = f;
            if (a.out_u8)
                *(uint32_t*)(a.out_u8 + row + x0) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ox = 4 * q + j;
                if (ox < a.Wo) {
                    const int x = flip ? a.Wo - 1 - ox : ox;
                    a.out[row + x] = lut[v[j]];
                    if (a.out_u8) a.out_u8[row + x] = (uint8_t)v[j];
                }
            }
        }
    }
}

// out[m][oy][ox] = src[m][ys[oy]][xs[ox]], flipped per frame; four output pixels per thread
__global__ __launch_bounds__(THREADS) void resize_nearest_u8_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ flipv,
                                                                    const int32_t* __restrict__ ys, const int32_t* __restrict__ xs,
                                                                    uint8_t* __restrict__ out, int M, int H, int W, int Ho, int Wo) {
    const int nq = (Wo + 3) >> 2;
    const long item = (long)blockIdx.x * THREADS + threadIdx.x;
    if (item >= (long)M * Ho * nq) return;
    const int q = (int)(item % nq);
    const long my = item / nq;
    const int oy = (int)(my % Ho), m = (int)(my / Ho);
    const bool flip = flipv[m] != 0;
    const int sy = max(0, min(ys[oy], H - 1));
    const uint8_t* srow = src + ((size_t)m * H + sy) * W;
    uint8_t* orow = out + ((size_t)m * Ho + oy) * Wo;
    uint32_t packed = 0;
    const int x0 = 4 * q;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = x0 + j;                                        // output position; its source column is mirrored when flipped
        if (x < Wo) {
            const int ox = flip ? Wo - 1 - x : x;
            const uint8_t v = srow[max(0, min(xs[ox], W - 1))];
            packed |= (uint32_t)v << (8 * j);
        }
    }
    if ((Wo & 3) == 0 && ((uintptr_t)out & 3) == 0) {
        *(uint32_t*)(orow + x0) = packed;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x0 + j < Wo) orow[x0 + j] = (uint8_t)(packed >> (8 * j));
    }
}

// Pillow's window of output index i (precompute_coeffs), in double precision like the host tables
void axis_window(int in, int out, int i, int* xmin, int* count) {
    const double scale = (double)in / (double)out, fscale = scale < 1.0 ? 1.0 : scale, support = 2.0 * fscale;
    const double center = ((double)i + 0.5) * scale;
    int lo = (int)(center - support + 0.5), hi = (int)(center + support + 0.5);
    if (lo < 0) lo = 0;
    if (hi > in) hi = in;
    *xmin = lo;
    *count = hi - lo;
}

int axis_ksize(int in, int out) {
    const double scale = (double)in / (double)out, fscale = scale < 1.0 ? 1.0 : scale;
    return 2 * (int)ceil(2.0 * fscale) + 1;
}

// the most source rows a band of bh output rows needs
int band_rows(int H, int Ho, int bh) {
    if (H == Ho) return bh < Ho ? bh : Ho;
    int most = 1;
    for (int oy0 = 0; oy0 < Ho; oy0 += bh) {
        const int oy1 = oy0 + bh < Ho ? oy0 + bh : Ho;
        int lo, n0, hi, n1;
        axis_window(H, Ho, oy0, &lo, &n0);
        axis_window(H, Ho, oy1 - 1, &hi, &n1);
        if (hi + n1 - lo > most) most = hi + n1 - lo;
    }
    return most;
}

// S holds up to 15 bytes of lead-in plus the range, rounded up to whole 16-byte chunks
size_t band_s_bytes(int rows, int W) { return ((size_t)rows * W + 30 + 15) & ~(size_t)15; }
size_t band_lds_bytes(int rows, int W, int TP) { return LUT_BYTES + band_s_bytes(rows, W) + (size_t)rows * TP; }

// band height and its row count; false when not even one output row fits
bool plan_band(int H, int W, int Ho, int TP, int* bh, int* rows) {
    for (int b = Ho < 16 ? Ho : 16; b >= 1; --b) {
        const int r = band_rows(H, Ho, b);
        if (band_lds_bytes(r, W, TP) <= (size_t)(b == 1 ? LDS_MAX : LDS_PREFERRED)) { *bh = b; *rows = r; return true; }
    }
    return false;
}

}  // namespace

extern "C" int s2e_resize_bicubic_u8(const uint8_t* src, const uint8_t* flip, int M, int H, int W, int Ho, int Wo,
                                     const int32_t* kx, const int32_t* bx, const int32_t* ky, const int32_t* by, const float* lut,
                                     float* out, uint8_t* out_u8, void* stream) {
    if (!src || !flip || !lut || !out || M <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0)
        S2E_FAIL(S2E_ERR_ARG, "s2e_resize_bicubic_u8: bad argument");
    if ((W != Wo && (!kx || !bx)) || (H != Ho && (!ky || !by)))
        S2E_FAIL(S2E_ERR_ARG, "s2e_resize_bicubic_u8: a pass that changes the size needs its tap and bounds tables");
    if (M > 65535 || (long)H * W > (1L << 30) || (long)Ho * Wo > (1L << 30))
        S2E_FAIL(S2E_ERR_UNSUPPORTED, "s2e_resize_bicubic_u8: %d frames of %d x %d -> %d x %d: too large", M, H, W, Ho, Wo);
    BicubicArgs a;
    a.src = src; a.flip = flip; a.lut = lut; a.out = out; a.out_u8 = out_u8;
    a.kx = W != Wo ? kx : nullptr; a.bx = W != Wo ? bx : nullptr;
    a.ky = H != Ho ? ky : nullptr; a.by = H != Ho ? by : nullptr;
    a.total = (long)M * H * W;
    a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo;
    a.ksx = axis_ksize(W, Wo); a.ksy = axis_ksize(H, Ho);
    a.TP = (Wo + 3) & ~3;
    if (!plan_band(H, W, Ho, a.TP, &a.bh, &a.rows_max))
        S2E_FAIL(S2E_ERR_UNSUPPORTED, "s2e_resize_bicubic_u8: %d x %d -> %d x %d: one output row's %d source rows do not fit %d bytes of LDS",
                 H, W, Ho, Wo, band_rows(H, Ho, 1), LDS_MAX);
    a.s_bytes = (int)band_s_bytes(a.rows_max, W);
    const dim3 grid(ceil_div(Ho, a.bh), M);
    resize_bicubic_u8_kernel<<<grid, THREADS, band_lds_bytes(a.rows_max, W, a.TP), (hipStream_t)stream>>>(a);
    S2E_CHECK_LAUNCH("resize_bicubic_u8_kernel");
    return S2E_OK;
}

extern "C" int s2e_resize_nearest_u8(const uint8_t* src, const uint8_t* flip, int M, int H, int W, int Ho, int Wo,
                                     const int32_t* ys, const int32_t* xs, uint8_t* out, void* stream) {
    if (!src || !flip || !ys || !xs || !out || M <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0)
        S2E_FAIL(S2E_ERR_ARG, "s2e_resize_nearest_u8: bad argument");
    const long items = (long)M * Ho * ((Wo + 3) >> 2);
    if (items > (long)THREADS * 0x7fffffffL) S2E_FAIL(S2E_ERR_UNSUPPORTED, "s2e_resize_nearest_u8: grid too large");
    resize_nearest_u8_kernel<<<ceil_div(items, THREADS), THREADS, 0, (hipStream_t)stream>>>(src, flip, ys, xs, out, M, H, W, Ho, Wo);
    S2E_CHECK_LAUNCH("resize_nearest_u8_kernel");
    return S2E_OK;
}
