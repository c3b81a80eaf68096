// From a packed weight gradient to the parameter's gradient, with or without spectral norm's chain rule.
// Given gwp = dL/dW (packed order: [co][tap*cin_pad + ci], fp32, from s2e_conv2d_wgrad) and W = W_orig / sigma:
//   dL/dW_orig = gW / sigma - (<gW, W_orig> / sigma^2) * u v^T          (sigma = u^T W_orig v, u, v constants)
// written in OIHW order.  Kernel 1: dot = <gW, W_orig>;  kernel 2: the element-wise combination.  Without spectral norm only the
// re-layout of kernel 2 is left.  Channels-last masters need no re-layout: their chain rule runs in place (end of this file).
#include "common.h"

// The packed gradient is [co][tap][ci] while W_orig / the output are [co][ci][tap].  A tile of SNG_ROWS co rows x 64 ci goes through
// LDS so that BOTH sides move as contiguous runs; thread (wave r, lane) owns row r: its lane index is the ci on the packed side
// and the flat run index (lane + 64 j) on the OIHW side, so no per-element integer division is needed (element-wise kernels spent
// ~150 instructions per element on 64-bit / and %: they were ALU-bound, not HBM-bound).  The two tile bodies below are the only
// copy of that index arithmetic: the per-layer kernels stride over the grid with them, the batched kernels walk their
// {job, first tile, number of tiles} block-map entry.  `my` is this wave's LDS row of 64 * taps floats.  The bodies' pointers are
// NOT __restrict__: the per-layer kernels' own qualifiers carry through the inlining, and the batched kernels read theirs from the
// job and never had any -- with them the batched pair unrolls further (22 -> 36 and 37 -> 56 VGPRs) and ran ~1 us per call slower.
static constexpr int SNG_ROWS = 4;     // co rows per tile = waves per block
struct grad_tile {
    int co, ci0, nci, run;             // this wave's row, the tile's first ci, its real channels, nci * taps
    bool rv;                           // row inside the matrix (the last row group may be ragged)
    int lane;
};
__device__ __forceinline__ grad_tile grad_tile_of(int cout, int cin, int taps, int t) {
    const int chunks = (cin + 63) / 64;
    const int rg = t / chunks;
    grad_tile T;
    T.co = rg * SNG_ROWS + (threadIdx.x >> 6);
    T.ci0 = (t - rg * chunks) * 64;
    T.nci = min(64, cin - T.ci0);
    T.run = T.nci * taps;
    T.rv = T.co < cout;
    T.lane = threadIdx.x & 63;
    return T;
}
// q + this lane's share of <gW, W_orig> over tile t, added tap by tap (q runs on across a block's tiles: one chain of adds per lane)
__device__ __forceinline__ float grad_dot_tile(const float* gwp, const float* w, int cout, int cin, int taps, int cin_pad, int t,
                                               float* my, float q) {
    const grad_tile T = grad_tile_of(cout, cin, taps, t);
    const float* wrow = w + ((size_t)T.co * cin + T.ci0) * taps;
    const float* grow = gwp + (size_t)T.co * taps * cin_pad + T.ci0 + T.lane;
    __syncthreads();
    if (T.rv)
        for (int k = T.lane; k < T.run; k += 64) my[k] = wrow[k];
    __syncthreads();
    if (T.rv && T.lane < T.nci)
        for (int tap = 0; tap < taps; ++tap) q += grow[(size_t)tap * cin_pad] * my[T.lane * taps + tap];
    return q;
}
// out[co][ci][tap] (+)= gwp[co][tap][ci] * inv - c u[co] v[ci*taps + tap] over tile t;   u == NULL: plain re-layout (inv = 1)
__device__ __forceinline__ void grad_unpack_tile(const float* gwp, const float* u, const float* v, float inv, float c, float* out,
                                                 int cout, int cin, int taps, int cin_pad, int accumulate, int t, float* my) {
    const grad_tile T = grad_tile_of(cout, cin, taps, t);
    const float* grow = gwp + (size_t)T.co * taps * cin_pad + T.ci0 + T.lane;
    __syncthreads();
    if (T.rv && T.lane < T.nci)
        for (int tap = 0; tap < taps; ++tap) my[T.lane * taps + tap] = grow[(size_t)tap * cin_pad];
    __syncthreads();
    if (T.rv) {
        float* orow = out + ((size_t)T.co * cin + T.ci0) * taps;
        const float cu = u ? c * u[T.co] : 0.f;
        const float* vrow = u ? v + (size_t)T.ci0 * taps : nullptr;
        for (int k = T.lane; k < T.run; k += 64) {
            float gg = my[k] * inv;
            if (u) gg -= cu * vrow[k];
            orow[k] = accumulate ? orow[k] + gg : gg;
        }
    }
}
__host__ __device__ static inline int grad_tiles(int cout, int cin) { return ((cout + SNG_ROWS - 1) / SNG_ROWS) * ((cin + 63) / 64); }

// ---- one layer: blocks stride over the tiles
__global__ __launch_bounds__(256) void sn_grad_dot_tiled_kernel(const float* __restrict__ gwp, const float* __restrict__ w, float* __restrict__ dot,
                                                                int cout, int cin, int taps, int cin_pad) {
    extern __shared__ float lds[];                          // [SNG_ROWS][64 * taps]
    __shared__ float red[4];
    const int r = threadIdx.x >> 6, lane = threadIdx.x & 63, tiles = grad_tiles(cout, cin);
    float q = 0.f;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) q = grad_dot_tile(gwp, w, cout, cin, taps, cin_pad, t, lds + r * 64 * taps, q);
    q = wave_sum(q);
    if (lane == 0) red[r] = q;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(dot, red[0] + red[1] + red[2] + red[3]);
}
__global__ __launch_bounds__(256) void grad_unpack_tiled_kernel(const float* __restrict__ gwp, const float* __restrict__ u, const float* __restrict__ v,
        const float* __restrict__ sigma, const float* __restrict__ dot, float* __restrict__ out, int cout, int cin, int taps, int cin_pad,
        int accumulate) {
    extern __shared__ float lds[];                          // [SNG_ROWS][64 * taps]
    const int r = threadIdx.x >> 6, tiles = grad_tiles(cout, cin);
    const float inv = u ? 1.f / *sigma : 1.f;
    const float c = u ? *dot * inv * inv : 0.f;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x)
        grad_unpack_tile(gwp, u, v, inv, c, out, cout, cin, taps, cin_pad, accumulate, t, lds + r * 64 * taps);
}

// ---- all layers of a step at once: block_map = {job, first tile, number of tiles}; the batch always accumulates
__global__ __launch_bounds__(256) void grad_dot_batch_kernel(const s2e_grad_job* __restrict__ jobs, const int* __restrict__ block_map, float* __restrict__ dots) {
    extern __shared__ float lds[];
    __shared__ float red[4];
    const int* bm = block_map + 3 * blockIdx.x;
    const s2e_grad_job J = jobs[bm[0]];
    if (!J.w_orig) return;                                  // plain re-layout job: nothing to reduce
    const int r = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float q = 0.f;
    for (int t = bm[1]; t < bm[1] + bm[2]; ++t) q = grad_dot_tile(J.gw_packed, J.w_orig, J.cout, J.cin, J.taps, J.cin_pad, t, lds + r * 64 * J.taps, q);
    q = wave_sum(q);
    if (lane == 0) red[r] = q;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(dots + J.dot_index, red[0] + red[1] + red[2] + red[3]);
}
__global__ __launch_bounds__(256) void grad_unpack_batch_kernel(const s2e_grad_job* __restrict__ jobs, const int* __restrict__ block_map, const float* __restrict__ dots) {
    extern __shared__ float lds[];
    const int* bm = block_map + 3 * blockIdx.x;
    const s2e_grad_job J = jobs[bm[0]];
    const int r = threadIdx.x >> 6;
    const float* u = J.w_orig ? J.u : nullptr;              // (a plain job's u, v, sigma are never read)
    const float inv = u ? 1.f / *J.sigma : 1.f;
    const float c = u ? dots[J.dot_index] * inv * inv : 0.f;
    for (int t = bm[1]; t < bm[1] + bm[2]; ++t)
        grad_unpack_tile(J.gw_packed, u, J.v, inv, c, J.out, J.cout, J.cin, J.taps, J.cin_pad, 1, t, lds + r * 64 * J.taps);
}
static constexpr int GRAD_TILES_PER_BLOCK = 8;
extern "C" long s2e_grad_block_map(const s2e_grad_job* jobs_host, int n_jobs, int* block_map_host) {
    if (!jobs_host || n_jobs < 0) return S2E_ERR_ARG;
    long nb = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const s2e_grad_job& J = jobs_host[j];
        const int tiles = grad_tiles(J.cout, J.cin);
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

// ---- the per-layer entries: grid capped at 1024 blocks for the dot, 2048 for the unpack
// grad[co][ci][tap] (+)= gwp[co][tap*cin_pad + ci]: packed wgrad output -> OIHW gradient (no spectral norm)
extern "C" int s2e_unpack_weight_grad(const float* gw_packed, float* gw_oihw, int cout, int cin, int kh, int kw, int cin_pad,
                                      int accumulate, void* stream) {
    if (!gw_packed || !gw_oihw || cout <= 0 || cin <= 0 || kh <= 0 || kw <= 0 || cin_pad < cin) S2E_FAIL(S2E_ERR_ARG, "s2e_unpack_weight_grad: bad argument");
    const int taps = kh * kw;
    if (taps > 64) S2E_FAIL(S2E_ERR_UNSUPPORTED, "s2e_unpack_weight_grad: more than 64 taps");
    const int tiles = grad_tiles(cout, cin);
    grad_unpack_tiled_kernel<<<tiles < 2048 ? tiles : 2048, 256, (size_t)SNG_ROWS * 64 * taps * sizeof(float), (hipStream_t)stream>>>(
        gw_packed, nullptr, nullptr, nullptr, nullptr, gw_oihw, cout, cin, taps, cin_pad, accumulate);
    S2E_CHECK_LAUNCH("grad_unpack_tiled_kernel");
    return S2E_OK;
}
extern "C" int s2e_sn_weight_grad(const float* gw_packed, const float* w_orig, const float* u, const float* v, const float* sigma,
                                  float* dot_ws, float* gw_orig, int cout, int cin, int kh, int kw, int cin_pad, int accumulate,
                                  void* stream) {
    if (!gw_packed || !w_orig || !u || !v || !sigma || !dot_ws || !gw_orig || cout <= 0 || cin <= 0 || kh <= 0 || kw <= 0 || cin_pad < cin)
        S2E_FAIL(S2E_ERR_ARG, "s2e_sn_weight_grad: bad argument");
    const int taps = kh * kw;
    if (taps > 64) S2E_FAIL(S2E_ERR_UNSUPPORTED, "s2e_sn_weight_grad: more than 64 taps");
    hipStream_t st = (hipStream_t)stream;
    const int tiles = grad_tiles(cout, cin);
    const size_t lds = (size_t)SNG_ROWS * 64 * taps * sizeof(float);
    sn_grad_dot_tiled_kernel<<<tiles < 1024 ? tiles : 1024, 256, lds, st>>>(gw_packed, w_orig, dot_ws, cout, cin, taps, cin_pad);
    grad_unpack_tiled_kernel<<<tiles < 2048 ? tiles : 2048, 256, lds, st>>>(gw_packed, u, v, sigma, dot_ws, gw_orig, cout, cin, taps, cin_pad, accumulate);
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
