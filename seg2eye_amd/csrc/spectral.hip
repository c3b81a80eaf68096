// Spectral normalisation (torch.nn.utils.spectral_norm semantics: 1 power iteration per forward in
// train mode, eps 1e-12, dim 0) for ALL spectral-normed convs of a network: the power iteration.  The sigma-aware weight
// packers are in weight_pack.hip, the gradient through W = W_orig / sigma in weight_grad.hip.
//
//   train:  t = W^T u;  v = t / max(|t|, eps);  s = W v;  u = s / max(|s|, eps);  sigma = u . s
//   eval :  s = W v;  sigma = u . s                              (u, v untouched)
//
// W is the (Cout) x (Cin*kh*kw) row-major view of weight_orig (fp32, lives in the flat parameter arena).
// HBM-bound, and W / sigma never exists in memory: the packers divide on the fly while converting to the MFMA layout.
//
// TRAIN: ONE READ OF W AND ONE LAUNCH PER ITERATION.  s is linear in v, so W t = max(|t|, eps) * W v: a workgroup that owns
// a COLUMN STRIP of W (all rows x SN_SC columns) holds everything for its share of both products.  With the strip in registers
// it forms t_J = sum_i W[i, J] u_i -- complete inside the workgroup, no other one touches those columns, so t is stored as plain
// fp32 -- and then adds sum_{j in J} W[i, j] t_j into the row accumulators y_i.  The two norms are applied afterwards, by the
// next iteration's launch or by the finaliser:  v = t / nt,  s = y / nt,  u = s / max(|s|, eps),  sigma = |s|^2 / max(|s|, eps),
// with nt = max(|t|, eps).  I iterations are I + 1 launches for every bank.
//
// Same inputs, same bits: u, v and sigma are a function of (W, u, v, iterations) alone.
//   * y is summed over the strips with 64-bit INTEGER atomics on fixed-point values: integer addition is associative, so the sums
//     come out bit-identical whatever order the workgroups finish in -- run to run, across graph replays and on every data-parallel
//     replica (fp32 atomics made sigma differ by ~1e-7 between runs, which bf16 weight rounding and the InstanceNorm chain amplified
//     to ~0.05 on the generated image).
//   * y = W t has magnitude ~sigma^2 where s = W v had ~sigma, so one word at 2^-40 would lose the small-sigma layers (sigma 1e-2:
//     a row sum of a 1024-row layer is ~3e-6 against a quantum of 9e-13).  Every partial is therefore SPLIT: a coarse word in units
//     of 2^-20 and the residual (< 2^-21) in units of 2^-60, added into two accumulators.  Both are signed sums, so no carries
//     are needed: y = hi * 2^-20 + lo * 2^-60, formed in double.  Range 2^43, resolution 8.7e-19: sigma from 1e-2 to 1e2 -- the
//     O(1..100) of the networks here and two decades below -- keeps > 40 bits under a row sum; nothing is carried between calls.
//   * |t|^2 is the sum, in strip order, of the strips' |t_J|^2 (stored per strip, never added atomically); every other sum
//     (t_J over the rows, the norms) runs in a fixed order inside one workgroup.
// The scratch is zero at creation and every call leaves it zero again, so no zero-fill launch is needed.
#include "common.h"
#include <stdlib.h>

// Channels-last masters (L.taps > 1: weight_orig stored [co][tap][ci]): W's MEMORY columns run (tap, ci) while the
// module's `weight_v` buffer keeps torch's (ci, tap) order -- state_dict, replica broadcast and the reference's u, v tests see
// no difference.  t is internal and stays in memory order; only the places that touch v translate.
__device__ __forceinline__ int sn_vidx(const s2e_sn_layer& L, int col) {
    return L.taps > 1 ? (col % L.cin) * L.taps + col / L.cin : col;
}

static constexpr int SN_NT = 1024;     // threads of the one-block-per-layer finalisers
__device__ __forceinline__ float sn_block_sum(float q, float* red) {
    q = wave_sum(q);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = q;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < SN_NT / 64; ++w) tot += red[w];
    return tot;
}
__device__ __forceinline__ float sn_block_sum256(float q, float* red) {
    q = wave_sum(q);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = q;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// ------------------------------------------------------------------------------------ train: one pass over W per iteration
static constexpr int SN_SC = 32;       // columns of a strip: 128 B per row = one cache line, one 16-byte load for each of 8 lanes
static constexpr int SN_SR = 1024;     // rows of a strip held in registers: 32 sweeps of 32 rows, 32 x 16 B per thread (128 VGPRs);
                                       // every spectral-normed conv here has <= 1024 rows; a taller layer is walked in chunks of SN_SR
static constexpr int SN_SCALAR_NS = 2; // sweeps per chunk of a layer that takes the scalar loads (the encoder's first conv has 64 rows)
static constexpr int SN_BR = 32;       // eval: rows per block of the W v pass, two batches of 16 row loads in flight together
static constexpr int SN_BC = 1024;     // eval: columns per block, four consecutive ones (one 16-byte load per row) per thread
// which = 0: the tiles of the eval W v pass; 1: the train strip (rows held in registers x columns)
extern "C" int s2e_sn_block_shape(int which, int* rows, int* cols) {
    if (rows) *rows = which ? SN_SR : SN_BR;
    if (cols) *cols = which ? SN_SC : SN_BC;
    return S2E_OK;
}

__device__ __forceinline__ void sn_fix2_add(long long* hi, long long* lo, float v) {
    const double d = (double)v;
    const long long h = __double2ll_rn(d * 0x1p20);
    const long long l = __double2ll_rn((d - (double)h * 0x1p-20) * 0x1p60);      // (exact: h has at most 24 significant bits)
    atomicAdd((unsigned long long*)hi, (unsigned long long)h);
    atomicAdd((unsigned long long*)lo, (unsigned long long)l);
}
__device__ __forceinline__ float sn_unfix2(long long hi, long long lo) { return (float)((double)hi * 0x1p-20 + (double)lo * 0x1p-60); }
// y of iteration k: [coarse | residual] x rows, three buffers in rotation.  Launch k adds into buffer k % 3, reads (k - 1) % 3 and
// clears (k + 1) % 3 -- two would not do: the buffer a launch reads is read by ALL its workgroups, so none of them may clear it.
__device__ __forceinline__ long long* sn_ybuf(const s2e_sn_layer& L, int k) { return L.y + (size_t)(k % 3) * 2 * L.rows; }
// the sum over the 8 lanes that share a row (an aligned group of 8), valid in all 8: three DPP adds
__device__ __forceinline__ float sn_sum8(float v) {
#define S2E_DPP_ADD(ctrl) v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, 0xF, 0xF, false))
    S2E_DPP_ADD(0xB1);             // quad_perm [1,0,3,2]
    S2E_DPP_ADD(0x4E);             // quad_perm [2,3,0,1]
    S2E_DPP_ADD(0x141);            // row_half_mirror
#undef S2E_DPP_ADD
    return v;
}

struct alignas(16) sn_strip_lds {
    float u[SN_SR];                // this iteration's u over the rows of the chunk, zero past the matrix
    float y[SN_SR];                // the strip's row sums of the chunk
    float tp[32][SN_SC];           // the 32 row sweeps' partial t_J, folded in sweep order
    float t[SN_SC];                // t_J
    float red[8];
};

// Thread (rl = tid / 8, cg = tid % 8) owns columns col0 + 4 cg .. + 3 of rows rl + 32 m, m < NS: NS sweeps cover the layer's rows, or
// one CHUNK of 32 NS of them -- a layer with more rows than the strip holds is walked in chunks, re-reading the strip from cache for
// the second product.  Rows past the matrix are CLAMPED to its last row and weighted with zero (u = 0; their row sums
// are never flushed), column groups past it to its last four and weighted with zero (t_J = 0), so that all NS loads of a thread are
// unconditional and in flight together (a guarded load per row compiles to a branch and a wait per row: 2.6 TB/s instead of 4.5).
// A thread's 16-byte loads need cols % 4 == 0 and an aligned matrix: every layer of the networks here but the encoder's first conv
// (9 columns), which takes the scalar loads (VEC = false) in chunks of 32 SN_SCALAR_NS rows.
template <int NS, bool VEC>
__device__ __forceinline__ void sn_onepass_body(const s2e_sn_layer& L, const int col0, const int k, const float eps, sn_strip_lds& sh) {
    const int tid = threadIdx.x, cg = tid & 7, rl = tid >> 3;
    const int rows = L.rows, cols = L.cols, nstrips = (cols + SN_SC - 1) / SN_SC;
    constexpr int CH = 32 * NS;
    const int nchunks = (rows + CH - 1) / CH;
    long long* ycur = sn_ybuf(L, k);
    const long long* yprv = sn_ybuf(L, k + 2);
    f32x4_t w[NS];
    auto load = [&](int row0) {
        // buffer loads: one resource per chunk (uniform) and ONE running 32-bit byte offset per thread -- a 64-bit address per load
        // would hold 2 NS registers beside the strip's 4 NS.  Row rl + 32 m is clamped to the chunk's last row; a chunk spans
        // 32 NS * cols * 4 < 2^31 bytes for any cols < 2^19.
        const int nr = min(rows - row0, CH), col = col0 + 4 * cg;
        const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)(L.w + (size_t)row0 * cols), 0, nr * cols * 4, 0x00020000);
        const unsigned lim = 4u * (nr - 1) * cols, step = 128u * cols;
        unsigned off = min(4u * rl * cols, lim);
        if constexpr (VEC) {
            const unsigned cc = 4u * min(col, cols - 4);
#pragma unroll
            for (int m = 0; m < NS; ++m) {
                w[m] = __builtin_bit_cast(f32x4_t, __builtin_amdgcn_raw_buffer_load_b128(rw, (int)(off + cc), 0, 0));
                off = min(off + step, lim);
            }
        } else {
#pragma unroll
            for (int m = 0; m < NS; ++m) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    w[m][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rw, (int)(off + 4u * min(col + j, cols - 1)), 0, 0));
                off = min(off + step, lim);
            }
        }
    };
    // One chunk (every layer of the networks here): the strip is requested BEFORE u is formed -- a chain of these launches is
    // latency-bound, and the norms (a pass over the previous y plus two block reductions) otherwise sit in front of the weight
    // loads' latency -- and stays in registers for both products.  More chunks: each is loaded for each product.
    const bool chunked = (NS == 32 || !VEC) && nchunks > 1;
    if (!chunked) load(0);
    if (k >= 2 && col0 == 0) {                               // the layer's first block clears the buffer the NEXT launch adds into
        long long* ynxt = sn_ybuf(L, k + 1);
        for (int i = tid; i < 2 * rows; i += 256) ynxt[i] = 0;
    }
    // ---- u: L.u for k = 0; else the previous launch's y, normalised twice (s = y / nt, u = s / max(|s|, eps)) -- every block
    // recomputes the two norms from the layer's <= 288 strip sums and <= 1024 row accumulators in the same order: the same bits
    float inv_nt = 1.f, inv_u = 1.f;
    float sv[4];                                             // s (k > 0) or u (k = 0) of rows tid + 256 q of the first chunk
    if (k > 0) {
        const float* tq = L.tq + (size_t)((k - 1) & 1) * nstrips;
        float qt = 0.f;
        for (int i = tid; i < nstrips; i += 256) qt += tq[i];
        inv_nt = 1.f / fmaxf(sqrtf(sn_block_sum256(qt, sh.red)), eps);
        long long a[4][2];
#pragma unroll
        for (int q = 0; q < 4; ++q) { const int i = min(tid + 256 * q, rows - 1); a[q][0] = yprv[i]; a[q][1] = yprv[rows + i]; }
        float qs = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) { sv[q] = tid + 256 * q < rows ? sn_unfix2(a[q][0], a[q][1]) * inv_nt : 0.f; qs += sv[q] * sv[q]; }
        for (int i = tid + SN_SR; i < rows; i += 256) { const float s = sn_unfix2(yprv[i], yprv[rows + i]) * inv_nt; qs += s * s; }
        inv_u = 1.f / fmaxf(sqrtf(sn_block_sum256(qs, sh.red + 4)), eps);
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) sv[q] = tid + 256 * q < rows ? L.u[tid + 256 * q] : 0.f;
    }

    // ---- t_J = sum_i W[i, J] u_i
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    auto dot_u = [&](int row0) {                             // sh.u = u over the chunk's rows (zero past the matrix); acc += the chunk's W^T u
        if (row0 == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) sh.u[tid + 256 * q] = sv[q] * inv_u;
        } else {
            for (int j = tid; j < CH; j += 256) {
                const int i = row0 + j;
                float uu = 0.f;
                if (i < rows) uu = k > 0 ? sn_unfix2(yprv[i], yprv[rows + i]) * inv_nt * inv_u : L.u[i];
                sh.u[j] = uu;
            }
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < NS; ++m) {
            const float uu = sh.u[rl + 32 * m];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += w[m][j] * uu;
        }
    };
    if (!chunked) dot_u(0);
    else
        for (int c = 0; c < nchunks; ++c) { load(c * CH); dot_u(c * CH); __syncthreads(); }
    // the 32 threads that share a column group fold through LDS, in sweep order
    *(f32x4_t*)&sh.tp[rl][4 * cg] = f32x4_t{acc[0], acc[1], acc[2], acc[3]};
    __syncthreads();
    if (tid < 64) {                                          // (wave 0)
        float tc = 0.f;
        if (tid < SN_SC && col0 + tid < cols) {
#pragma unroll
            for (int r = 0; r < 32; ++r) tc += sh.tp[r][tid];
            L.t[col0 + tid] = tc;
        }
        if (tid < SN_SC) sh.t[tid] = tc;
        const float q = wave_sum(tc * tc);
        if (tid == 0) L.tq[(size_t)(k & 1) * nstrips + col0 / SN_SC] = q;
    }
    __syncthreads();
    // ---- y_i += sum_{j in J} W[i, j] t_j
    const f32x4_t tv = *(const f32x4_t*)&sh.t[4 * cg];
    auto add_rows = [&](int row0) {
#pragma unroll
        for (int m = 0; m < NS; ++m) {
            const float p = sn_sum8((w[m][0] * tv[0] + w[m][1] * tv[1]) + (w[m][2] * tv[2] + w[m][3] * tv[3]));
            if (cg == 0) sh.y[rl + 32 * m] = p;
        }
        // one pair of atomics per row per block; consecutive lanes add to consecutive rows (512 contiguous bytes per instruction)
        __syncthreads();
        const int nr = min(rows - row0, CH);
        for (int i = tid; i < nr; i += 256) sn_fix2_add(ycur + row0 + i, ycur + rows + row0 + i, sh.y[i]);
    };
    if (!chunked) add_rows(0);
    else
        for (int c = 0; c < nchunks; ++c) { load(c * CH); add_rows(c * CH); __syncthreads(); }
}

// strip_map = {layer, first column of the strip} per block
__global__ __launch_bounds__(256, 2) void sn_onepass_kernel(const s2e_sn_layer* __restrict__ layers, const int* __restrict__ strip_map,
                                                            int k, float eps) {
    __shared__ sn_strip_lds sh;
    const int* bm = strip_map + 2 * blockIdx.x;
    const s2e_sn_layer L = layers[bm[0]];
    const int sweeps = (min(L.rows, SN_SR) + 31) / 32;
    if ((L.cols & 3) || ((uintptr_t)L.w & 15)) sn_onepass_body<SN_SCALAR_NS, false>(L, bm[1], k, eps, sh);
    else if (sweeps <= 1) sn_onepass_body<1, true>(L, bm[1], k, eps, sh);
    else if (sweeps <= 2) sn_onepass_body<2, true>(L, bm[1], k, eps, sh);
    else if (sweeps <= 4) sn_onepass_body<4, true>(L, bm[1], k, eps, sh);
    else if (sweeps <= 8) sn_onepass_body<8, true>(L, bm[1], k, eps, sh);
    else if (sweeps <= 16) sn_onepass_body<16, true>(L, bm[1], k, eps, sh);
    else sn_onepass_body<32, true>(L, bm[1], k, eps, sh);
}

// one block per layer, after the last iteration: v = t / nt, s = y / nt, u = s / max(|s|, eps), sigma = |s|^2 / max(|s|, eps);
// everything the iterations wrote is cleared
__global__ __launch_bounds__(SN_NT) void sn_onepass_finalize_kernel(const s2e_sn_layer* __restrict__ layers, float* __restrict__ sigma,
                                                                    int last, float eps) {
    __shared__ float red[2][SN_NT / 64];
    const s2e_sn_layer L = layers[blockIdx.x];
    const int nstrips = (L.cols + SN_SC - 1) / SN_SC;
    const long long* yl = sn_ybuf(L, last);
    const float* tq = L.tq + (size_t)(last & 1) * nstrips;
    float qt = 0.f;
    for (int i = threadIdx.x; i < nstrips; i += SN_NT) qt += tq[i];
    const float inv_nt = 1.f / fmaxf(sqrtf(sn_block_sum(qt, red[0])), eps);
    float q = 0.f;
    for (int i = threadIdx.x; i < L.rows; i += SN_NT) { const float s = sn_unfix2(yl[i], yl[L.rows + i]) * inv_nt; q += s * s; }
    const float tot = sn_block_sum(q, red[1]);
    const float inv = 1.f / fmaxf(sqrtf(tot), eps);
    for (int i = threadIdx.x; i < L.rows; i += SN_NT) L.u[i] = sn_unfix2(yl[i], yl[L.rows + i]) * inv_nt * inv;
    if (threadIdx.x == 0) sigma[blockIdx.x] = tot * inv;                // u . s = |s|^2 / max(|s|, eps)
    for (int j = threadIdx.x; j < L.cols; j += SN_NT) { L.v[sn_vidx(L, j)] = L.t[j] * inv_nt; L.t[j] = 0.f; }
    __syncthreads();                                                    // (every thread has read its tq and y)
    for (int i = threadIdx.x; i < 2 * nstrips; i += SN_NT) L.tq[i] = 0.f;
    for (int i = threadIdx.x; i < 6 * L.rows; i += SN_NT) L.y[i] = 0;
}

// ------------------------------------------------------------------------------------ eval: s = W v, sigma = u . s
// The partial dot products of the blocks are combined with 64-bit integer atomics on fixed-point values (2^-40 units: |partial| < 2^22
// fits with room to spare, the quantisation of 9e-13 is far below fp32 resolution of the values being summed).
static constexpr float SN_FIX = 1099511627776.0f;          // 2^40
static constexpr float SN_UNFIX = 1.0f / 1099511627776.0f;
__device__ __forceinline__ void sn_fix_add(long long* dst, float v) {
    atomicAdd((unsigned long long*)dst, (unsigned long long)__double2ll_rn((double)v * (double)SN_FIX));
}
__device__ __forceinline__ float sn_unfix(long long q) { return (float)((double)q * (double)SN_UNFIX); }

// ---- s += W v over a [SN_BR x SN_BC] block; block_map = {layer, row0, col0}
__global__ __launch_bounds__(256) void sn_gemv_kernel(const s2e_sn_layer* __restrict__ layers, const int* __restrict__ block_map) {
    __shared__ float red[SN_BR][4];
    const int* bm = block_map + 3 * blockIdx.x;
    const s2e_sn_layer L = layers[bm[0]];
    const int row0 = bm[1], col = bm[2] + 4 * threadIdx.x;
    const int nr = min(L.rows - row0, SN_BR);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if ((L.cols & 3) == 0 && ((uintptr_t)L.w & 15) == 0 && ((uintptr_t)L.v & 15) == 0) {
        const int cc = min(col, L.cols - 4);                   // a thread past the matrix re-reads its last columns, weighted with zero
        f32x4_t v4;
        if (L.taps > 1) { const int j0 = sn_vidx(L, cc); v4 = f32x4_t{L.v[j0], L.v[j0 + L.taps], L.v[j0 + 2 * L.taps], L.v[j0 + 3 * L.taps]}; }   // (cin % 4 == 0: one tap)
        else v4 = *(gptr_f32x4_t)((gptr_f32_t)L.v + cc);
        const float on = col < L.cols ? 1.f : 0.f;
        const f32x4_t vv = {v4[0] * on, v4[1] * on, v4[2] * on, v4[3] * on};
        gptr_f32_t wp = (gptr_f32_t)L.w + (size_t)row0 * L.cols + cc;
#pragma unroll
        for (int b = 0; b < SN_BR; b += 16) {
            f32x4_t w[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) w[k] = *(gptr_f32x4_t)(wp + (size_t)min(b + k, nr - 1) * L.cols);
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const float q = wave_sum_last((w[k][0] * vv[0] + w[k][1] * vv[1]) + (w[k][2] * vv[2] + w[k][3] * vv[3]));
                if (lane == 63) red[b + k][wave] = q;
            }
        }
    } else {
        gptr_f32_t wp = (gptr_f32_t)L.w + (size_t)row0 * L.cols + col;
        for (int r = 0; r < SN_BR; ++r) {
            float q = 0.f;
            if (r < nr)
                for (int j = 0; j < 4; ++j) if (col + j < L.cols) q += wp[(size_t)r * L.cols + j] * L.v[sn_vidx(L, col + j)];
            q = wave_sum(q);
            if (lane == 0) red[r][wave] = q;
        }
    }
    __syncthreads();
    if (threadIdx.x < nr) sn_fix_add(L.s + row0 + threadIdx.x, red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3]);
}

// ---- one block per layer: sigma = u . s; the accumulator is left cleared (each thread clears what it alone read)
__global__ __launch_bounds__(SN_NT) void sn_finalize_kernel(const s2e_sn_layer* __restrict__ layers, float* __restrict__ sigma) {
    __shared__ float red[SN_NT / 64];
    const s2e_sn_layer L = layers[blockIdx.x];
    float q = 0.f;
    for (int i = threadIdx.x; i < L.rows; i += SN_NT) { q += L.u[i] * sn_unfix(L.s[i]); L.s[i] = 0; }
    const float tot = sn_block_sum(q, red);
    if (threadIdx.x == 0) sigma[blockIdx.x] = tot;
}

extern "C" int s2e_sn_power_iteration(const s2e_sn_layer* layers, int n_layers, const int* strip_map, int n_strips,
                                      const int* block_map, int n_blocks,
                                      void* scratch, size_t scratch_bytes, float* sigma, int train, int iterations,
                                      float eps, void* stream) {
    if (!layers || !block_map || !strip_map || !scratch || !sigma || n_layers <= 0 || n_blocks <= 0 || n_strips <= 0 || iterations < 1)
        S2E_FAIL(S2E_ERR_ARG, "s2e_sn_power_iteration: bad argument");
    hipStream_t st = (hipStream_t)stream;
    (void)scratch_bytes;                                     // the accumulators in `scratch` are cleared by the kernels themselves
    if (train) {                                             // I + 1 launches
        for (int it = 0; it < iterations; ++it) sn_onepass_kernel<<<n_strips, 256, 0, st>>>(layers, strip_map, it, eps);
        sn_onepass_finalize_kernel<<<n_layers, SN_NT, 0, st>>>(layers, sigma, iterations - 1, eps);
    } else {
        sn_gemv_kernel<<<n_blocks, 256, 0, st>>>(layers, block_map);
        sn_finalize_kernel<<<n_layers, SN_NT, 0, st>>>(layers, sigma);
    }
    S2E_CHECK_LAUNCH("sn power-iteration kernels");
    return S2E_OK;
}
