// Spectral normalisation (torch.nn.utils.spectral_norm semantics: 1 power iteration per forward in
// train mode, eps 1e-12, dim 0) for ALL spectral-normed convs of a network, the sigma-aware weight
// packers, and the fused gradient through W = W_orig / sigma.
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

// ------------------------------------------------------------------------------------ weight packers
#include "conv_plane.h"
// OIHW fp32 -> MFMA B-operand layout in the compute dtype, divided by *sigma when sigma != NULL.
// Both directions go through LDS so that global reads AND writes are contiguous runs.
// Every element of the padded matrix is written exactly once per call (padding rows / channels / K tail as
// zeros), so no separate zero-fill is needed.
// Thread mapping as in the gradient re-layout kernels below: no per-element integer division.
// forward pack : out[row][(tap)*cin_pad + ci]   one block = 4 rows (one per wave) x 64 (padded) ci
template <typename T>
__device__ __forceinline__ void pack_fwd_block(const float* __restrict__ w, T* __restrict__ out, const float* __restrict__ sigma,
                                               int cout, int cin, int taps, int cin_pad, int kpad, int bx, int by, float* lds) {
    // lds: [4][64 * taps]
    const int r = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = bx * 4 + r, ci0 = by * 64;             // padded row count is a multiple of 32
    const bool valid = row < cout;
    const int nci = valid ? max(0, min(64, cin - ci0)) : 0;       // real channels in this chunk
    const int ncp = min(64, cin_pad - ci0);                        // channels incl. structural-zero padding
    const float inv = sigma ? 1.f / *sigma : 1.f;
    float* my = lds + r * 64 * taps;
    const float* src = w + ((size_t)row * cin + ci0) * taps;
    for (int k = lane; k < nci * taps; k += 64) my[k] = src[k] * inv;
    __syncthreads();
    T* dst = out + (size_t)row * kpad + ci0 + lane;
    if (lane < ncp)
        for (int tap = 0; tap < taps; ++tap) dst[(size_t)tap * cin_pad] = (T)(lane < nci ? my[lane * taps + tap] : 0.f);
    if (by == 0)                                             // K tail [taps*cin_pad, kpad)
        for (int k = taps * cin_pad + lane; k < kpad; k += 64) out[(size_t)row * kpad + k] = (T)0.f;
}
// transposed pack: out[ci][(tap)*cout + co]     one block = 64 co x 8 (padded) ci rows
template <typename T>
__device__ __forceinline__ void pack_tr_block(const float* __restrict__ w, T* __restrict__ out, const float* __restrict__ sigma,
                                              int cout, int cin, int taps, int rows_pad, int kpad, int bx, int by, float* lds) {
    // lds: [64 co][8*taps + 1]
    const int q = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int co0 = bx * 64, ci0 = by * 8;
    const int nco = min(64, cout - co0);
    const int nci = max(0, min(8, cin - ci0)), ncp = min(8, rows_pad - ci0);
    const int run = nci * taps, ld = 8 * taps + 1;
    const float inv = sigma ? 1.f / *sigma : 1.f;
    for (int m = q; m < nco; m += 4) {                       // wave q stages co rows q, q+4, ...: contiguous runs
        const float* src = w + ((size_t)(co0 + m) * cin + ci0) * taps;
        for (int k = lane; k < run; k += 64) lds[m * ld + k] = src[k] * inv;
    }
    __syncthreads();
    if (lane < nco)
        for (int cil = 0; cil < ncp; ++cil) {
            T* dst = out + (size_t)(ci0 + cil) * kpad + co0 + lane;
            for (int tap = q; tap < taps; tap += 4)          // wave q writes taps q, q+4, ...: 64 consecutive co each
                dst[(size_t)tap * cout] = (T)(cil < nci ? lds[lane * ld + cil * taps + tap] : 0.f);
        }
    if (bx == 0) {                                           // K tail [taps*cout, kpad) of this block's rows
        const int tail = kpad - taps * cout;
        for (int cil = q; cil < ncp; cil += 4)
            for (int k = lane; k < tail; k += 64) out[(size_t)(ci0 + cil) * kpad + taps * cout + k] = (T)0.f;
    }
}

// forward pack from a CHANNELS-LAST source w[co][tap][ci] (cin_pad == cin, cin % 8 == 0): the source row IS the packed row, so the
// pack is a streaming convert of the (rows_pad x kpad) output: a thread owns 8 consecutive columns (two 16-byte loads, one
// 16/32-byte store), a block 2048 consecutive elements of the flattened output; padding rows / the K tail are written as zeros.
static constexpr int PACK_CL_ELEMS = 2048;
template <typename T>
__device__ __forceinline__ void pack_fwd_cl_block(const float* __restrict__ w, T* __restrict__ out, const float* __restrict__ sigma,
                                                  int cout, int K, int rows_pad, int kpad, int bx) {
    const long idx = (long)bx * PACK_CL_ELEMS + 8 * threadIdx.x;
    if (idx >= (long)rows_pad * kpad) return;
    const int row = (int)(idx / kpad), col = (int)(idx - (long)row * kpad);      // (kpad % 8 == 0: the 8 columns share a row)
    const float inv = sigma ? 1.f / *sigma : 1.f;
    float f[8];
    if (row < cout && col < K) {                                                  // (K % 8 == 0: all 8 real or all 8 padding)
        const f32x4_t a = *(const f32x4_t*)(w + (size_t)row * K + col), b = *(const f32x4_t*)(w + (size_t)row * K + col + 4);
        f[0] = a[0] * inv; f[1] = a[1] * inv; f[2] = a[2] * inv; f[3] = a[3] * inv;
        f[4] = b[0] * inv; f[5] = b[1] * inv; f[6] = b[2] * inv; f[7] = b[3] * inv;
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = 0.f;
    }
    if constexpr (std::is_same<T, float>::value) {
        *(u32x4_t*)(out + idx) = pack16<float>(f);
        *(u32x4_t*)(out + idx + 4) = pack16<float>(f + 4);
    } else {
        *(u32x4_t*)(out + idx) = pack16<bf16_t>(f);
    }
}

// transposed pack from a CHANNELS-LAST source w[co][tap][ci] (cin_pad == cin): one block = 64 co x 64 ci of ONE tap, a plain
// tile transpose -- rows of 64 consecutive ci in, rows of 64 consecutive co out.  by = tap * ceil(rows_pad / 64) + ci chunk.
// out_fwd != NULL (round 6): the FORWARD pack of the same weight, [co][tap * cin + ci] with row pitch kpad_f, is written from the same
// tile -- the fp32 master is read once for both layouts (a G step packs 93 M parameters both ways: 372 MB of reads saved).  Only the
// weight's own elements are written there: the padding rows / K tail of that matrix are the caller's to zero, once.
template <typename T>
__device__ __forceinline__ void pack_tr_cl_block(const float* __restrict__ w, T* __restrict__ out, const float* __restrict__ sigma,
                                                 int cout, int cin, int taps, int rows_pad, int kpad, int bx, int by, float* lds,
                                                 T* __restrict__ out_fwd = nullptr, int kpad_f = 0) {
    // lds: [64 co][65]
    const int q = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int gyc = (rows_pad + 63) / 64;
    const int tap = by / gyc, ci0 = (by - tap * gyc) * 64, co0 = bx * 64;
    const float inv = sigma ? 1.f / *sigma : 1.f;
    for (int m = q; m < 64; m += 4) {
        const int co = co0 + m, ci = ci0 + lane;
        lds[m * 65 + lane] = (co < cout && ci < cin) ? w[((size_t)co * taps + tap) * cin + ci] * inv : 0.f;
    }
    __syncthreads();
    if (out_fwd && ci0 + lane < cin)
        for (int m = q; m < 64; m += 4)
            if (co0 + m < cout) out_fwd[(size_t)(co0 + m) * kpad_f + (size_t)tap * cin + ci0 + lane] = (T)lds[m * 65 + lane];
    if (co0 + lane < cout)
        for (int cil = q; cil < 64; cil += 4)
            if (ci0 + cil < rows_pad) out[(size_t)(ci0 + cil) * kpad + (size_t)tap * cout + co0 + lane] = (T)lds[lane * 65 + cil];
    if (bx == 0 && tap == 0) {                               // K tail [taps*cout, kpad) of this block's rows
        const int tail = kpad - taps * cout;
        for (int cil = q; cil < 64; cil += 4)
            if (ci0 + cil < rows_pad)
                for (int k = lane; k < tail; k += 64) out[(size_t)(ci0 + cil) * kpad + taps * cout + k] = (T)0.f;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void pack_fwd_kernel(const float* __restrict__ w, T* __restrict__ out, const float* __restrict__ sigma,
                                                       int cout, int cin, int taps, int cin_pad, int kpad) {
    extern __shared__ float lds[];
    pack_fwd_block<T>(w, out, sigma, cout, cin, taps, cin_pad, kpad, blockIdx.x, blockIdx.y, lds);
}
template <typename T>
__global__ __launch_bounds__(256) void pack_tr_kernel(const float* __restrict__ w, T* __restrict__ out, const float* __restrict__ sigma,
                                                      int cout, int cin, int taps, int rows_pad, int kpad) {
    extern __shared__ float lds[];
    pack_tr_block<T>(w, out, sigma, cout, cin, taps, rows_pad, kpad, blockIdx.x, blockIdx.y, lds);
}
template <typename T>
__global__ __launch_bounds__(256) void pack_fwd_cl_kernel(const float* __restrict__ w, T* __restrict__ out, const float* __restrict__ sigma,
                                                          int cout, int K, int rows_pad, int kpad) {
    pack_fwd_cl_block<T>(w, out, sigma, cout, K, rows_pad, kpad, blockIdx.x);
}
template <typename T>
__global__ __launch_bounds__(256) void pack_tr_cl_kernel(const float* __restrict__ w, T* __restrict__ out, const float* __restrict__ sigma,
                                                         int cout, int cin, int taps, int rows_pad, int kpad) {
    extern __shared__ float lds[];
    pack_tr_cl_block<T>(w, out, sigma, cout, cin, taps, rows_pad, kpad, blockIdx.x, blockIdx.y, lds);
}
// the PLANE layout (conv_plane.h): bf16 only
__global__ __launch_bounds__(256) void pack_plane_kernel(const float* __restrict__ w, bf16_t* __restrict__ out, const float* __restrict__ sigma,
                                                         int cout, int cin, int taps, int transposed) {
    pack_plane_block(w, out, sigma, cout, cin, taps, transposed, blockIdx.x);
}
// every conv of a network in one launch: block_map = {job, bx, by} per block (s2e_pack_block_map)
template <typename T>
__global__ __launch_bounds__(256) void pack_batch_kernel(const s2e_pack_job* __restrict__ jobs, const int* __restrict__ block_map,
                                                         const float* __restrict__ sigma_base, int dtype) {
    extern __shared__ float lds[];
    const int* bm = block_map + 3 * blockIdx.x;
    const s2e_pack_job J = jobs[bm[0]];
    const float* sg = J.sigma_index >= 0 ? sigma_base + J.sigma_index : nullptr;
    if (J.transposed & S2E_PACK_PLANE) {                     // the PLANE layout (conv_plane.hip's weights)
        if constexpr (std::is_same<T, bf16_t>::value) pack_plane_block(J.w, (bf16_t*)J.out, sg, J.cout, J.cin, J.taps, J.transposed, bm[1]);
    } else if (J.transposed == 2) {                                 // channels-last source (s2e_pack_job: transposed bit 1), forward
        const int kpad = (J.taps * J.cin + (dtype == S2E_BF16 ? 63 : 31)) / (dtype == S2E_BF16 ? 64 : 32) * (dtype == S2E_BF16 ? 64 : 32);
        const int rows = J.cout <= 32 ? 32 : (J.cout <= 64 ? 64 : (J.cout + 127) / 128 * 128);
        pack_fwd_cl_block<T>(J.w, (T*)J.out, sg, J.cout, J.taps * J.cin, rows, kpad, bm[1]);
    } else if (J.transposed & 2) {                           // ... transposed
        const int kpad = (J.taps * J.cout + (dtype == S2E_BF16 ? 63 : 31)) / (dtype == S2E_BF16 ? 64 : 32) * (dtype == S2E_BF16 ? 64 : 32);
        const int rows = J.cin_pad <= 32 ? 32 : (J.cin_pad <= 64 ? 64 : (J.cin_pad + 127) / 128 * 128);
        const int kpad_f = (J.taps * J.cin + (dtype == S2E_BF16 ? 63 : 31)) / (dtype == S2E_BF16 ? 64 : 32) * (dtype == S2E_BF16 ? 64 : 32);
        pack_tr_cl_block<T>(J.w, (T*)J.out, sg, J.cout, J.cin, J.taps, rows, kpad, bm[1], bm[2], lds, (T*)J.out_fwd, kpad_f);
    } else if (!J.transposed) {
        const int kpad = (J.taps * J.cin_pad + (dtype == S2E_BF16 ? 63 : 31)) / (dtype == S2E_BF16 ? 64 : 32) * (dtype == S2E_BF16 ? 64 : 32);
        pack_fwd_block<T>(J.w, (T*)J.out, sg, J.cout, J.cin, J.taps, J.cin_pad, kpad, bm[1], bm[2], lds);
    } else {
        const int kpad = (J.taps * J.cout + (dtype == S2E_BF16 ? 63 : 31)) / (dtype == S2E_BF16 ? 64 : 32) * (dtype == S2E_BF16 ? 64 : 32);
        const int rows = J.cin_pad <= 32 ? 32 : (J.cin_pad <= 64 ? 64 : (J.cin_pad + 127) / 128 * 128);
        pack_tr_block<T>(J.w, (T*)J.out, sg, J.cout, J.cin, J.taps, rows, kpad, bm[1], bm[2], lds);
    }
}

extern "C" int s2e_pack_conv_weight(int dtype, const float* w, void* packed, const float* sigma, int cout, int cin, int kh, int kw,
                                    int cin_pad, int transposed, void* stream) {
    if (!w || !packed || cout <= 0 || cin <= 0 || kh <= 0 || kw <= 0 || cin_pad < cin)
        S2E_FAIL(S2E_ERR_ARG, "s2e_pack_conv_weight: bad argument");
    S2E_CHECK_DTYPE(dtype, "s2e_pack_conv_weight");
    const int taps = kh * kw;
    if (taps > 64) S2E_FAIL(S2E_ERR_UNSUPPORTED, "s2e_pack_conv_weight: kernel %dx%d too large", kh, kw);
    const bool tr = (transposed & 1) != 0;
    if (transposed & S2E_PACK_PLANE) {                       // the PLANE layout (conv_plane.h): bf16, no channel padding, K a multiple of 32
        if (dtype != S2E_BF16 || cin_pad != cin || (tr ? cout : cin) % 32 != 0)
            S2E_FAIL(S2E_ERR_UNSUPPORTED, "s2e_pack_conv_weight: the plane layout needs bf16, cin_pad == cin and a K dimension that is a multiple of 32");
        const long units = s2e_plane_pack_units(cout, cin, taps, transposed);
        pack_plane_kernel<<<ceil_div(units, 256), 256, 0, (hipStream_t)stream>>>(w, (bf16_t*)packed, sigma, cout, cin, taps, transposed);
        S2E_CHECK_LAUNCH("pack_plane_kernel");
        return S2E_OK;
    }
    const int rows = s2e_conv_cout_pad(tr ? cin_pad : cout);
    const int kpad = s2e_conv_k_pad(dtype, taps * (tr ? cout : cin_pad));
    hipStream_t st = (hipStream_t)stream;
    if (transposed & 2) {                                    // source in channels-last order w[co][tap][ci]
        if (cin_pad != cin) S2E_FAIL(S2E_ERR_UNSUPPORTED, "s2e_pack_conv_weight: a channels-last source needs cin_pad == cin");
        if (cin % 8) S2E_FAIL(S2E_ERR_UNSUPPORTED, "s2e_pack_conv_weight: a channels-last source needs cin %% 8 == 0");
    }
    return s2e_with_dtype(dtype, "s2e_pack_conv_weight", [&](auto t) { using T = decltype(t);
        if ((transposed & 2) && !tr) {                       // channels-last, forward: the source row IS the packed row: a streaming convert
            const int grid = ceil_div((long)rows * kpad, PACK_CL_ELEMS);
            pack_fwd_cl_kernel<T><<<grid, 256, 0, st>>>(w, (T*)packed, sigma, cout, taps * cin, rows, kpad);
        } else if (transposed & 2) {
            dim3 grid(ceil_div(cout, 64), taps * ceil_div(rows, 64));
            const size_t lds = (size_t)64 * 65 * sizeof(float);
            pack_tr_cl_kernel<T><<<grid, 256, lds, st>>>(w, (T*)packed, sigma, cout, cin, taps, rows, kpad);
        } else if (!transposed) {
            dim3 grid(rows / 4, ceil_div(cin_pad, 64));
            const size_t lds = (size_t)4 * 64 * taps * sizeof(float);
            pack_fwd_kernel<T><<<grid, 256, lds, st>>>(w, (T*)packed, sigma, cout, cin, taps, cin_pad, kpad);
        } else {
            dim3 grid(ceil_div(cout, 64), ceil_div(rows, 8));
            const size_t lds = (size_t)64 * (8 * taps + 1) * sizeof(float);
            pack_tr_kernel<T><<<grid, 256, lds, st>>>(w, (T*)packed, sigma, cout, cin, taps, rows, kpad);
        }
        S2E_CHECK_LAUNCH((transposed & 2) ? "pack kernels (channels-last source)" : "pack kernels"); return S2E_OK; });
}

extern "C" long s2e_pack_block_map(int dtype, const s2e_pack_job* jobs_host, int n_jobs, int* block_map_host) {
    if (!jobs_host || n_jobs < 0) return S2E_ERR_ARG;
    long nb = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const s2e_pack_job& J = jobs_host[j];
        int gx, gy;
        if (J.transposed & S2E_PACK_PLANE) { gx = ceil_div(s2e_plane_pack_units(J.cout, J.cin, J.taps, J.transposed), 256); gy = 1; }
        else if (J.transposed == 2)  { gx = ceil_div((long)s2e_conv_cout_pad(J.cout) * s2e_conv_k_pad(dtype, J.taps * J.cin), PACK_CL_ELEMS); gy = 1; }
        else if (J.transposed & 2) { gx = ceil_div(J.cout, 64);   gy = J.taps * ceil_div(s2e_conv_cout_pad(J.cin_pad), 64); }
        else if (!J.transposed) { gx = s2e_conv_cout_pad(J.cout) / 4; gy = ceil_div(J.cin_pad, 64); }
        else                    { gx = ceil_div(J.cout, 64);      gy = ceil_div(s2e_conv_cout_pad(J.cin_pad), 8); }
        if (block_map_host)
            for (int y = 0; y < gy; ++y)
                for (int x = 0; x < gx; ++x) {
                    int* e = block_map_host + 3 * (nb + (long)y * gx + x);
                    e[0] = j; e[1] = x; e[2] = y;
                }
        nb += (long)gx * gy;
    }
    return nb;
}

extern "C" int s2e_pack_conv_weights(int dtype, const s2e_pack_job* jobs, const int* block_map, int n_blocks, int max_taps,
                                     const float* sigma_base, void* stream) {
    if (!jobs || !block_map || n_blocks <= 0 || max_taps <= 0) S2E_FAIL(S2E_ERR_ARG, "s2e_pack_conv_weights: bad argument");
    S2E_CHECK_DTYPE(dtype, "s2e_pack_conv_weights");
    if (max_taps > 16) S2E_FAIL(S2E_ERR_UNSUPPORTED, "s2e_pack_conv_weights: more than 16 taps");
    size_t lds = (size_t)64 * (8 * max_taps + 1) * sizeof(float);
    if (lds < (size_t)64 * 65 * sizeof(float)) lds = (size_t)64 * 65 * sizeof(float);      // (the channels-last tile transpose)
    hipStream_t st = (hipStream_t)stream;
    return s2e_with_dtype(dtype, "s2e_pack_conv_weights", [&](auto t) {
        pack_batch_kernel<decltype(t)><<<n_blocks, 256, lds, st>>>(jobs, block_map, sigma_base, dtype);
        S2E_CHECK_LAUNCH("batched pack kernel"); return S2E_OK; });
}

// ------------------------------------------------------------------------------------ gradient through W = W_orig / sigma
// Given gwp = dL/dW (packed order: [co][tap*cin_pad + ci], fp32, from s2e_conv2d_wgrad):
//   dL/dW_orig = gW / sigma - (<gW, W_orig> / sigma^2) * u v^T          (sigma = u^T W_orig v, u, v constants)
// written in OIHW order.  Kernel 1: dot = <gW, W_orig>;  kernel 2: the element-wise combination.
__global__ __launch_bounds__(256) void sn_grad_dot_kernel(const float* __restrict__ gwp, const float* __restrict__ w, float* __restrict__ dot,
                                                          int cout, int cin, int taps, int cin_pad) {
    __shared__ float red[4];
    const long total = (long)cout * cin * taps;
    float q = 0.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int tap = (int)(i % taps);
        const long r = i / taps;
        const int ci = (int)(r % cin), co = (int)(r / cin);
        q += w[i] * gwp[(size_t)co * taps * cin_pad + (size_t)tap * cin_pad + ci];
    }
    q = wave_sum(q);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = q;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(dot, red[0] + red[1] + red[2] + red[3]);
}
__global__ __launch_bounds__(256) void sn_grad_apply_kernel(const float* __restrict__ gwp, const float* __restrict__ u, const float* __restrict__ v,
        const float* __restrict__ sigma, const float* __restrict__ dot, float* __restrict__ out, int cout, int cin, int taps, int cin_pad,
        int accumulate) {
    const long total = (long)cout * cin * taps;
    const float inv = 1.f / *sigma;
    const float c = *dot * inv * inv;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int tap = (int)(i % taps);
        const long r = i / taps;
        const int ci = (int)(r % cin), co = (int)(r / cin);
        const float g = gwp[(size_t)co * taps * cin_pad + (size_t)tap * cin_pad + ci] * inv - c * u[co] * v[(size_t)ci * taps + tap];
        out[i] = accumulate ? out[i] + g : g;
    }
}

// Tiled variants for taps > 1: the packed gradient is [co][tap][ci] while W_orig / the output are [co][ci][tap].  A tile
// of SNG_ROWS co rows x 64 ci goes through LDS so that BOTH sides move as contiguous runs; thread (wave r, lane) owns
// row r: its lane index is the ci on the packed side and the flat run index (lane + 64 j) on the OIHW side, so no
// per-element integer division is needed (the element-wise kernels above spend ~150 instructions per element on
// 64-bit / and %: they were ALU-bound, not HBM-bound).  Blocks loop over tiles.
static constexpr int SNG_ROWS = 4;     // co rows per tile = waves per block
__global__ __launch_bounds__(256) void sn_grad_dot_tiled_kernel(const float* __restrict__ gwp, const float* __restrict__ w, float* __restrict__ dot,
                                                                int cout, int cin, int taps, int cin_pad) {
    extern __shared__ float lds[];                          // [SNG_ROWS][64 * taps]
    __shared__ float red[4];
    const int chunks = (cin + 63) / 64, rgroups = (cout + SNG_ROWS - 1) / SNG_ROWS, tiles = rgroups * chunks;
    const int r = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* my = lds + r * 64 * taps;
    float q = 0.f;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int rg = t / chunks, ci0 = (t - rg * chunks) * 64, co = rg * SNG_ROWS + r;
        const int nci = min(64, cin - ci0), run = nci * taps;
        const bool rv = co < cout;
        const float* wrow = w + ((size_t)co * cin + ci0) * taps;
        const float* grow = gwp + (size_t)co * taps * cin_pad + ci0 + lane;
        __syncthreads();
        if (rv)
            for (int k = lane; k < run; k += 64) my[k] = wrow[k];
        __syncthreads();
        if (rv && lane < nci)
            for (int tap = 0; tap < taps; ++tap) q += grow[(size_t)tap * cin_pad] * my[lane * taps + tap];
    }
    q = wave_sum(q);
    if (lane == 0) red[r] = q;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(dot, red[0] + red[1] + red[2] + red[3]);
}
// out[co][ci][tap] (+)= gwp[co][tap][ci] / sigma - (dot / sigma^2) u[co] v[ci*taps + tap];   u == NULL: plain re-layout
__global__ __launch_bounds__(256) void grad_unpack_tiled_kernel(const float* __restrict__ gwp, const float* __restrict__ u, const float* __restrict__ v,
        const float* __restrict__ sigma, const float* __restrict__ dot, float* __restrict__ out, int cout, int cin, int taps, int cin_pad,
        int accumulate) {
    extern __shared__ float lds[];                          // [SNG_ROWS][64 * taps]
    const int chunks = (cin + 63) / 64, rgroups = (cout + SNG_ROWS - 1) / SNG_ROWS, tiles = rgroups * chunks;
    const int r = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* my = lds + r * 64 * taps;
    const float inv = u ? 1.f / *sigma : 1.f;
    const float c = u ? *dot * inv * inv : 0.f;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int rg = t / chunks, ci0 = (t - rg * chunks) * 64, co = rg * SNG_ROWS + r;
        const int nci = min(64, cin - ci0), run = nci * taps;
        const bool rv = co < cout;
        const float* grow = gwp + (size_t)co * taps * cin_pad + ci0 + lane;
        __syncthreads();
        if (rv && lane < nci)
            for (int tap = 0; tap < taps; ++tap) my[lane * taps + tap] = grow[(size_t)tap * cin_pad];
        __syncthreads();
        if (rv) {
            float* orow = out + ((size_t)co * cin + ci0) * taps;
            const float cu = u ? c * u[co] : 0.f;
            const float* vrow = v + (size_t)ci0 * taps;
            for (int k = lane; k < run; k += 64) {
                float gg = my[k] * inv;
                if (u) gg -= cu * vrow[k];
                orow[k] = accumulate ? orow[k] + gg : gg;
            }
        }
    }
}

// ---- all layers of a step at once: block_map = {job, first tile, number of tiles}; same tile bodies as above
__global__ __launch_bounds__(256) void grad_dot_batch_kernel(const s2e_grad_job* __restrict__ jobs, const int* __restrict__ block_map, float* __restrict__ dots) {
    extern __shared__ float lds[];
    __shared__ float red[4];
    const int* bm = block_map + 3 * blockIdx.x;
    const s2e_grad_job J = jobs[bm[0]];
    if (!J.w_orig) return;                                  // plain re-layout job: nothing to reduce
    const int taps = J.taps, cin = J.cin, cout = J.cout, cin_pad = J.cin_pad;
    const int chunks = (cin + 63) / 64;
    const int r = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* my = lds + r * 64 * taps;
    float q = 0.f;
    for (int t = bm[1]; t < bm[1] + bm[2]; ++t) {
        const int rg = t / chunks, ci0 = (t - rg * chunks) * 64, co = rg * SNG_ROWS + r;
        const int nci = min(64, cin - ci0), run = nci * taps;
        const bool rv = co < cout;
        const float* wrow = J.w_orig + ((size_t)co * cin + ci0) * taps;
        const float* grow = J.gw_packed + (size_t)co * taps * cin_pad + ci0 + lane;
        __syncthreads();
        if (rv)
            for (int k = lane; k < run; k += 64) my[k] = wrow[k];
        __syncthreads();
        if (rv && lane < nci)
            for (int tap = 0; tap < taps; ++tap) q += grow[(size_t)tap * cin_pad] * my[lane * taps + tap];
    }
    q = wave_sum(q);
    if (lane == 0) red[r] = q;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(dots + J.dot_index, red[0] + red[1] + red[2] + red[3]);
}
__global__ __launch_bounds__(256) void grad_unpack_batch_kernel(const s2e_grad_job* __restrict__ jobs, const int* __restrict__ block_map, const float* __restrict__ dots) {
    extern __shared__ float lds[];
    const int* bm = block_map + 3 * blockIdx.x;
    const s2e_grad_job J = jobs[bm[0]];
    const int taps = J.taps, cin = J.cin, cout = J.cout, cin_pad = J.cin_pad;
    const int chunks = (cin + 63) / 64;
    const int r = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* my = lds + r * 64 * taps;
    const bool sn = J.w_orig != nullptr;
    const float inv = sn ? 1.f / *J.sigma : 1.f;
    const float c = sn ? dots[J.dot_index] * inv * inv : 0.f;
    for (int t = bm[1]; t < bm[1] + bm[2]; ++t) {
        const int rg = t / chunks, ci0 = (t - rg * chunks) * 64, co = rg * SNG_ROWS + r;
        const int nci = min(64, cin - ci0), run = nci * taps;
        const bool rv = co < cout;
        const float* grow = J.gw_packed + (size_t)co * taps * cin_pad + ci0 + lane;
        __syncthreads();
        if (rv && lane < nci)
            for (int tap = 0; tap < taps; ++tap) my[lane * taps + tap] = grow[(size_t)tap * cin_pad];
        __syncthreads();
        if (rv) {
            float* orow = J.out + ((size_t)co * cin + ci0) * taps;
            const float cu = sn ? c * J.u[co] : 0.f;
            const float* vrow = sn ? J.v + (size_t)ci0 * taps : nullptr;
            for (int k = lane; k < run; k += 64) {
                float gg = my[k] * inv;
                if (sn) gg -= cu * vrow[k];
                orow[k] += gg;
            }
        }
    }
}
static constexpr int GRAD_TILES_PER_BLOCK = 8;
extern "C" long s2e_grad_block_map(const s2e_grad_job* jobs_host, int n_jobs, int* block_map_host) {
    if (!jobs_host || n_jobs < 0) return S2E_ERR_ARG;
    long nb = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const s2e_grad_job& J = jobs_host[j];
        const int tiles = ceil_div(J.cout, SNG_ROWS) * ceil_div(J.cin, 64);
        for (int t0 = 0; t0 < tiles; t0 += GRAD_TILES_PER_BLOCK, ++nb)
            if (block_map_host) {
                int* e = block_map_host + 3 * nb;
                e[0] = j; e[1] = t0; e[2] = tiles - t0 < GRAD_TILES_PER_BLOCK ? tiles - t0 : GRAD_TILES_PER_BLOCK;
            }
    }
    return nb;
}
extern "C" int s2e_weight_grads_batched(const s2e_grad_job* jobs, const int* block_map, int n_blocks, int max_taps, int any_sn,
                                        float* dots, void* stream) {
    if (!jobs || !block_map || n_blocks <= 0 || max_taps <= 0 || (any_sn && !dots)) S2E_FAIL(S2E_ERR_ARG, "s2e_weight_grads_batched: bad argument");
    if (max_taps > 64) S2E_FAIL(S2E_ERR_UNSUPPORTED, "s2e_weight_grads_batched: more than 64 taps");
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)SNG_ROWS * 64 * max_taps * sizeof(float);
    if (any_sn) grad_dot_batch_kernel<<<n_blocks, 256, lds, st>>>(jobs, block_map, dots);
    grad_unpack_batch_kernel<<<n_blocks, 256, lds, st>>>(jobs, block_map, dots);
    S2E_CHECK_LAUNCH("batched weight-gradient kernels");
    return S2E_OK;
}

// grad[co][ci][tap] (+)= gwp[co][tap*cin_pad + ci]: packed wgrad output -> OIHW gradient (no spectral norm)
__global__ __launch_bounds__(256) void unpack_grad_kernel(const float* __restrict__ gwp, float* __restrict__ out, int cout, int cin, int taps,
                                                          int cin_pad, int accumulate) {
    const long total = (long)cout * cin * taps;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int tap = (int)(i % taps);
        const long r = i / taps;
        const int ci = (int)(r % cin), co = (int)(r / cin);
        const float g = gwp[(size_t)co * taps * cin_pad + (size_t)tap * cin_pad + ci];
        out[i] = accumulate ? out[i] + g : g;
    }
}
extern "C" int s2e_unpack_weight_grad(const float* gw_packed, float* gw_oihw, int cout, int cin, int kh, int kw, int cin_pad,
                                      int accumulate, void* stream) {
    if (!gw_packed || !gw_oihw || cout <= 0 || cin <= 0 || cin_pad < cin) S2E_FAIL(S2E_ERR_ARG, "s2e_unpack_weight_grad: bad argument");
    const long total = (long)cout * cin * kh * kw;
    const int grid = s2e_grid1d(total, 2048);
    const int taps = kh * kw;
    if (taps > 1 && taps <= 64) {
        const int tiles = ceil_div(cout, SNG_ROWS) * ceil_div(cin, 64);
        grad_unpack_tiled_kernel<<<tiles < 2048 ? tiles : 2048, 256, (size_t)SNG_ROWS * 64 * taps * sizeof(float), (hipStream_t)stream>>>(
            gw_packed, nullptr, nullptr, nullptr, nullptr, gw_oihw, cout, cin, taps, cin_pad, accumulate);
    } else
        unpack_grad_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(gw_packed, gw_oihw, cout, cin, taps, cin_pad, accumulate);
    S2E_CHECK_LAUNCH("unpack_grad_kernel");
    return S2E_OK;
}

extern "C" int s2e_sn_weight_grad(const float* gw_packed, const float* w_orig, const float* u, const float* v, const float* sigma,
                                  float* dot_ws, float* gw_orig, int cout, int cin, int kh, int kw, int cin_pad, int accumulate,
                                  void* stream) {
    if (!gw_packed || !w_orig || !u || !v || !sigma || !dot_ws || !gw_orig || cout <= 0 || cin <= 0 || cin_pad < cin)
        S2E_FAIL(S2E_ERR_ARG, "s2e_sn_weight_grad: bad argument");
    hipStream_t st = (hipStream_t)stream;
    const long total = (long)cout * cin * kh * kw;
    const int grid = s2e_grid1d(total, 2048);
    const int taps = kh * kw;
    if (taps > 1 && taps <= 64) {
        const int tiles = ceil_div(cout, SNG_ROWS) * ceil_div(cin, 64);
        const size_t lds = (size_t)SNG_ROWS * 64 * taps * sizeof(float);
        sn_grad_dot_tiled_kernel<<<tiles < 1024 ? tiles : 1024, 256, lds, st>>>(gw_packed, w_orig, dot_ws, cout, cin, taps, cin_pad);
        grad_unpack_tiled_kernel<<<tiles < 2048 ? tiles : 2048, 256, lds, st>>>(gw_packed, u, v, sigma, dot_ws, gw_orig, cout, cin, taps, cin_pad, accumulate);
    } else {
        sn_grad_dot_kernel<<<grid, 256, 0, st>>>(gw_packed, w_orig, dot_ws, cout, cin, taps, cin_pad);
        sn_grad_apply_kernel<<<grid, 256, 0, st>>>(gw_packed, u, v, sigma, dot_ws, gw_orig, cout, cin, taps, cin_pad, accumulate);
    }
    S2E_CHECK_LAUNCH("sn_weight_grad kernels");
    return S2E_OK;
}


// ------------------------------------------------------------------------------------ the same gradient IN PLACE (channels-last masters)
// With the fp32 masters stored in the packed order [co][tap][ci] the weight-gradient kernels accumulate straight into the
// parameter's slice of the gradient arena; what is left of the chain rule above is element-wise and in place:
//     g[i] = g[i] / sigma - (<g, W_orig> / sigma^2) u[row] v[col]           (row = i / K, col = i % K, K = taps * cin)
// Launch 1: every block stores the partial dot product of its 16 Ki-element chunk (plain store).  Launch 2: every block of a
// layer first adds that layer's partials in the same fixed order (deterministic: no float atomics), then rewrites its chunk.
// 16 bytes of traffic per element, all of it contiguous (the OIHW re-layout moved 20, half of it in 4-byte strides).
static constexpr int SNI_CHUNK = 16384;     // elements per block: 256 threads x 16 float4
__global__ __launch_bounds__(256) void sn_grad_inplace_dot_kernel(const s2e_sngrad_job* __restrict__ jobs, const int* __restrict__ block_map,
                                                                  float* __restrict__ partials) {
    __shared__ float red[4];
    const int* bm = block_map + 2 * blockIdx.x;
    const s2e_sngrad_job J = jobs[bm[0]];
    const long total = (long)J.rows * J.cin * J.taps;
    const long i0 = (long)bm[1] * SNI_CHUNK, i1 = i0 + SNI_CHUNK < total ? i0 + SNI_CHUNK : total;
    float q = 0.f;
    for (long i = i0 + 4 * threadIdx.x; i < i1; i += 1024) {         // (total % 4 == 0: cin % 8 == 0)
        const f32x4_t a = *(const f32x4_t*)(J.g + i), b = *(const f32x4_t*)(J.w + i);
        q += (a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3]);
    }
    q = wave_sum(q);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = q;
    __syncthreads();
    if (threadIdx.x == 0) partials[J.part0 + bm[1]] = (red[0] + red[1]) + (red[2] + red[3]);
    // the layer's first block also lays v out in W's MEMORY order for the second launch (one 16-byte load per four columns there
    // instead of four strided ones)
    if (bm[1] == 0) {
        const int K = J.cin * J.taps;
        float* vm = partials + J.vmem0;
        for (int col = threadIdx.x; col < K; col += 256) { const int tap = col / J.cin, ci = col - tap * J.cin; vm[col] = J.v[(size_t)ci * J.taps + tap]; }
    }
}
__global__ __launch_bounds__(256) void sn_grad_inplace_apply_kernel(const s2e_sngrad_job* __restrict__ jobs, const int* __restrict__ block_map,
                                                                    const float* __restrict__ partials) {
    __shared__ float red[4];
    const int* bm = block_map + 2 * blockIdx.x;
    const s2e_sngrad_job J = jobs[bm[0]];
    float q = 0.f;
    for (int k = threadIdx.x; k < J.nparts; k += 256) q += partials[J.part0 + k];
    q = wave_sum(q);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = q;
    __syncthreads();
    const float dot = (red[0] + red[1]) + (red[2] + red[3]);
    const float inv = 1.f / *J.sigma;
    const float c = dot * inv * inv;
    const int K = J.cin * J.taps;
    const float* vm = partials + J.vmem0;
    const long total = (long)J.rows * K;
    const long i0 = (long)bm[1] * SNI_CHUNK, i1 = i0 + SNI_CHUNK < total ? i0 + SNI_CHUNK : total;
    long i = i0 + 4 * threadIdx.x;
    int row = (int)(i / K), col = (int)(i - (long)row * K);          // (one 64-bit division per thread; then stepped)
    for (; i < i1; i += 1024, col += 1024) {
        while (col >= K) { col -= K; ++row; }
        const float cu = c * J.u[row];
        const f32x4_t vv = *(const f32x4_t*)(vm + col);             // (v in memory order: written by the first launch)
        f32x4_t a = *(const f32x4_t*)(J.g + i);
        a[0] = a[0] * inv - cu * vv[0];
        a[1] = a[1] * inv - cu * vv[1];
        a[2] = a[2] * inv - cu * vv[2];
        a[3] = a[3] * inv - cu * vv[3];
        *(f32x4_t*)(J.g + i) = a;
    }
}
extern "C" long s2e_sngrad_block_map(s2e_sngrad_job* jobs_host, int n_jobs, int* block_map_host) {
    if (!jobs_host || n_jobs < 0) return S2E_ERR_ARG;
    long nb = 0;
    for (int j = 0; j < n_jobs; ++j) {
        s2e_sngrad_job& J = jobs_host[j];
        const long total = (long)J.rows * J.cin * J.taps;
        const int chunks = (int)((total + SNI_CHUNK - 1) / SNI_CHUNK);
        J.part0 = (int)nb; J.nparts = chunks;                // (one partial per block: the block index IS the slot)
        for (int c = 0; c < chunks; ++c, ++nb)
            if (block_map_host) { block_map_host[2 * nb] = j; block_map_host[2 * nb + 1] = c; }
    }
    long off = (nb + 3) / 4 * 4;                             // behind the partials: every layer's v in memory order
    for (int j = 0; j < n_jobs; ++j) { jobs_host[j].vmem0 = (int)off; off += (long)jobs_host[j].cin * jobs_host[j].taps; }
    return nb;
}
extern "C" long s2e_sngrad_scratch_floats(const s2e_sngrad_job* jobs_host, int n_jobs) {
    if (!jobs_host || n_jobs <= 0) return 0;
    const s2e_sngrad_job& J = jobs_host[n_jobs - 1];        // (after s2e_sngrad_block_map: the last layer's v region ends the scratch)
    return (long)J.vmem0 + (long)J.cin * J.taps;
}
extern "C" int s2e_sn_grads_inplace(const s2e_sngrad_job* jobs, const int* block_map, int n_blocks, float* partials, void* stream) {
    if (!jobs || !block_map || n_blocks <= 0 || !partials) S2E_FAIL(S2E_ERR_ARG, "s2e_sn_grads_inplace: bad argument");
    // (cin % 8 == 0 of every job is the caller's to guarantee: the jobs live in device memory)
    hipStream_t st = (hipStream_t)stream;
    sn_grad_inplace_dot_kernel<<<n_blocks, 256, 0, st>>>(jobs, block_map, partials);
    sn_grad_inplace_apply_kernel<<<n_blocks, 256, 0, st>>>(jobs, block_map, partials);
    S2E_CHECK_LAUNCH("in-place spectral-norm gradient kernels");
    return S2E_OK;
}
