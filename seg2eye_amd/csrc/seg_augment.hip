// Paired augmentation of the segmenter's training data: one launch warps a batch of (frame, label map) pairs of uint8
// planes by one affine transform per pair -- the frame bilinearly, the label map by the nearest source pixel --, draws up to eight
// line occluders on the frame and sends the frame through a per-pair table (gamma, contrast, brightness).  The rule is stated in
// include/seg2eye_hip.h: integers throughout, so a numpy restatement gives the same bits (tests/_seg_augment_ref.py).
//
// Shape: grid (M, ceil(H * ceil(W / 4) / 256)); a workgroup stays within one pair, so the pair's six coefficients are scalar loads,
// its lines -- clamped once, by the first L lanes -- and its two tables sit in LDS.  A lane owns four consecutive output pixels of a
// row: 20 byte gathers (four taps of the frame and one of the label map per pixel; neighbours in a row of the source share lines of
// the L1 / L2), then 16 bytes of fp32 and 4 bytes each of the uint8 outputs.  VEC: W is a multiple of 4 and every output is aligned to
// its store (16 / 4 / 4 bytes); otherwise element stores.  The inputs are read by bytes either way.
// No workspace, no atomics.  In bounds for ANY int32 parameters: a source position is clamped in 64 bits before it is an index.
#include "common.h"

namespace {

constexpr int AUG_THREADS = 256;
constexpr int AUG_MAX_SIDE = 4096;                           // x, y < 2^12: A * x + A * y + A below 2^45
constexpr int AUG_MAX_LINES = 8;
constexpr int AUG_LINE_LO = -4096, AUG_LINE_HI = 8191;       // end points: |x - x0| <= 8191, |dx| <= 12287, so t and c fit 32 bits

struct AugArgs {
    const uint8_t* img; const uint8_t* lab;
    const int32_t* affine; const int32_t* lines;
    const float* lut_f32; const uint8_t* lut_u8;
    float* out_f32; uint8_t* out_u8; uint8_t* out_lab;
    int H, W, L;
};

__device__ __forceinline__ int aug_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int aug_clamp64(long long v, long long hi) { return (int)(v < 0 ? 0 : (v > hi ? hi : v)); }

template <bool VEC>
__global__ __launch_bounds__(AUG_THREADS) void augment_pairs_kernel(const AugArgs a) {
    __shared__ float s_lutf[256];
    __shared__ uint8_t s_lutb[256];
    __shared__ int s_line[AUG_MAX_LINES][5];                 // x0, y0, dx, dy, value
    __shared__ long long s_len2[AUG_MAX_LINES], s_w2len[AUG_MAX_LINES];
    const int m = blockIdx.x, tid = threadIdx.x, H = a.H, W = a.W;
    const bool image = a.out_f32 || a.out_u8;
    const int L = image ? a.L : 0;
    if (a.out_f32) s_lutf[tid] = a.lut_f32[(size_t)m * 256 + tid];
    if (a.out_u8) s_lutb[tid] = a.lut_u8[(size_t)m * 256 + tid];
    if (tid < L) {
        const int32_t* p = a.lines + ((size_t)m * L + tid) * 6;
        const int x0 = aug_clamp(p[0], AUG_LINE_LO, AUG_LINE_HI), y0 = aug_clamp(p[1], AUG_LINE_LO, AUG_LINE_HI);
        const int dx = aug_clamp(p[2], AUG_LINE_LO, AUG_LINE_HI) - x0, dy = aug_clamp(p[3], AUG_LINE_LO, AUG_LINE_HI) - y0;
        const long long width = aug_clamp(p[4], 0, 255), len2 = (long long)dx * dx + (long long)dy * dy;
        s_line[tid][0] = x0; s_line[tid][1] = y0; s_line[tid][2] = dx; s_line[tid][3] = dy; s_line[tid][4] = p[5] & 255;
        s_len2[tid] = len2;
        s_w2len[tid] = (width >= 1 && len2 > 0) ? width * width * len2 : -1;      // -1: no 4 c^2 is below it, the line covers nothing
    }
    __syncthreads();
    const int nq = (W + 3) >> 2;
    const int item = blockIdx.y * AUG_THREADS + tid;         // H * nq <= 2^22
    if (item >= H * nq) return;
    const int y = item / nq, xb = 4 * (item - y * nq);
    const int32_t* A = a.affine + (size_t)m * 6;
    const long long a0 = A[0], a3 = A[3];
    const long long bx = (long long)A[1] * y + A[2], by = (long long)A[4] * y + A[5];
    const long long sx_max = (long long)(W - 1) << 16, sy_max = (long long)(H - 1) << 16;
    const size_t plane = (size_t)m * H * W;
    const uint8_t* img = image ? a.img + plane : nullptr;    // (an input without its output may be NULL)
    const uint8_t* lab = a.out_lab ? a.lab + plane : nullptr;
    int v[4] = {0, 0, 0, 0}, c[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = xb + j;
        if (!VEC && x >= W) continue;
        const int sx = aug_clamp64(bx + a0 * x, sx_max), sy = aug_clamp64(by + a3 * x, sy_max);        // <= 4095 << 16: 32 bits now
        if (a.out_lab) c[j] = lab[(size_t)((sy + 0x8000) >> 16) * W + ((sx + 0x8000) >> 16)];
        if (!image) continue;
        const int x0 = sx >> 16, y0 = sy >> 16, fx = (sx & 0xffff) >> 8, fy = (sy & 0xffff) >> 8;
        const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
        const uint8_t* r0 = img + (size_t)y0 * W;
        const uint8_t* r1 = img + (size_t)y1 * W;
        const int p00 = r0[x0], p01 = r0[x1], p10 = r1[x0], p11 = r1[x1];
        int val = ((p00 * (256 - fx) + p01 * fx) * (256 - fy) + (p10 * (256 - fx) + p11 * fx) * fy + 0x8000) >> 16;
        for (int k = 0; k < L; ++k) {
            const long long w2len = s_w2len[k];
            if (w2len < 0) continue;                          // (the same for the whole workgroup)
            const int ux = x - s_line[k][0], uy = y - s_line[k][1], dx = s_line[k][2], dy = s_line[k][3];
            const long long t = (long long)ux * dx + (long long)uy * dy, cr = (long long)ux * dy - (long long)uy * dx;
            if (t >= 0 && t <= s_len2[k] && 4 * cr * cr <= w2len) val = s_line[k][4];
        }
        v[j] = val;
    }
    const size_t o = plane + (size_t)y * W + xb;
    if (VEC) {
        if (a.out_f32) {
            const f32x4_t f = {s_lutf[v[0]], s_lutf[v[1]], s_lutf[v[2]], s_lutf[v[3]]};
            *(f32x4_t*)(a.out_f32 + o) = f;
        }
        if (a.out_u8)
            *(uint32_t*)(a.out_u8 + o) = (uint32_t)s_lutb[v[0]] | (uint32_t)s_lutb[v[1]] << 8 | (uint32_t)s_lutb[v[2]] << 16 | (uint32_t)s_lutb[v[3]] << 24;
        if (a.out_lab) *(uint32_t*)(a.out_lab + o) = (uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16 | (uint32_t)c[3] << 24;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (xb + j >= W) continue;
            if (a.out_f32) a.out_f32[o + j] = s_lutf[v[j]];
            if (a.out_u8) a.out_u8[o + j] = s_lutb[v[j]];
            if (a.out_lab) a.out_lab[o + j] = (uint8_t)c[j];
        }
    }
}

}  // namespace

extern "C" int s2e_augment_pairs(const uint8_t* img, const uint8_t* lab, int M, int H, int W, const int32_t* affine, const int32_t* lines, int L,
                                 const float* lut_f32, const uint8_t* lut_u8, float* out_f32, uint8_t* out_u8, uint8_t* out_lab, void* stream) {
    const char* name = "s2e_augment_pairs";
    const bool image = out_f32 || out_u8;
    if (!affine) S2E_FAIL(S2E_ERR_ARG, "%s: bad argument (affine is NULL)", name);
    if (!image && !out_lab) S2E_FAIL(S2E_ERR_ARG, "%s: bad argument (no output: out_f32, out_u8 and out_lab are all NULL)", name);
    if (image && !img) S2E_FAIL(S2E_ERR_ARG, "%s: bad argument (an image output without img)", name);
    if (out_lab && !lab) S2E_FAIL(S2E_ERR_ARG, "%s: bad argument (out_lab without lab)", name);
    if (M < 1 || H < 1 || W < 1) S2E_FAIL(S2E_ERR_ARG, "%s: M=%d H=%d W=%d (every size must be at least 1)", name, M, H, W);
    if (L < 0 || (L > 0 && !lines)) S2E_FAIL(S2E_ERR_ARG, "%s: L=%d lines without the lines array", name, L);
    if (out_f32 && !lut_f32) S2E_FAIL(S2E_ERR_ARG, "%s: out_f32 without lut_f32", name);
    if (out_u8 && !lut_u8) S2E_FAIL(S2E_ERR_ARG, "%s: out_u8 without lut_u8", name);
    if ((((uintptr_t)affine | (uintptr_t)lines | (uintptr_t)lut_f32 | (uintptr_t)out_f32) & 3) != 0)
        S2E_FAIL(S2E_ERR_ARG, "%s: affine, lines, lut_f32 and out_f32 must be 4-byte aligned", name);
    const void* ins[2] = {img, lab};
    const void* outs[3] = {out_f32, out_u8, out_lab};
    for (const void* o : outs)
        for (const void* i : ins)
            if (o && o == i) S2E_FAIL(S2E_ERR_ARG, "%s: an output is its own input (the warp reads pixels other lanes write)", name);
    if (H > AUG_MAX_SIDE || W > AUG_MAX_SIDE) S2E_FAIL(S2E_ERR_UNSUPPORTED, "%s: H=%d W=%d (each at most %d)", name, H, W, AUG_MAX_SIDE);
    if (L > AUG_MAX_LINES) S2E_FAIL(S2E_ERR_UNSUPPORTED, "%s: L=%d (at most %d lines per frame)", name, L, AUG_MAX_LINES);
    AugArgs a;
    a.img = img; a.lab = lab; a.affine = affine; a.lines = lines; a.lut_f32 = lut_f32; a.lut_u8 = lut_u8;
    a.out_f32 = out_f32; a.out_u8 = out_u8; a.out_lab = out_lab;
    a.H = H; a.W = W; a.L = L;
    const dim3 grid(M, ceil_div((long)H * ((W + 3) >> 2), AUG_THREADS));               // (y: at most 2^14)
    const bool vec = W % 4 == 0 && ((uintptr_t)out_f32 & 15) == 0 && (((uintptr_t)out_u8 | (uintptr_t)out_lab) & 3) == 0;
    if (vec) augment_pairs_kernel<true><<<grid, AUG_THREADS, 0, (hipStream_t)stream>>>(a);
    else augment_pairs_kernel<false><<<grid, AUG_THREADS, 0, (hipStream_t)stream>>>(a);
    S2E_CHECK_LAUNCH("augment_pairs_kernel");
    return S2E_OK;
}
