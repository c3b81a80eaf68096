// Style reference rankings: the distances between M target label maps and K candidate label maps, and the k nearest
// candidates of every target.  Both are integer work, so every result is exact and the same from run to run.
//
// s2e_mask_dist is a byte GEMM with a very long reduction axis: dist[m][k] = sum_p f(a[m][p], b[k][p]) over P = H W label bytes, on
// v_mfma_i32_16x16x64_i8.  Both operands are contiguous along p, so a lane's 16-byte fragment is 16 consecutive bytes of one row
// (row lane & 15, bytes 16 (lane >> 4) .. + 15 of the 64-byte step); A and B are indexed by the same p, so whatever order the
// instruction gives the 64 bytes of a step, the sum is the same.  C/D is the map every 16x16 MFMA has: column lane & 15 (the B row, a
// candidate), row 4 (lane >> 4) + register (the A row, a target).
//   l2        sum a^2 + sum b^2 - 2 sum a b: the product on the matrix cores, the two norms by v_dot4 on the fragments the lane holds
//   mismatch  P - sum_c sum_p [a = c][b = c]: the 0/1 operand bytes of one class at a time are built in registers
// One WAVE owns a 64 x 64 tile of the output (4 x 4 MFMA tiles, fragments straight from global memory: 8 loads feed 16 MFMAs) over one
// chunk of the pixel axis; the four waves of a workgroup take four consecutive chunks of one tile and add their tiles in LDS, and the
// workgroups of a tile are combined with atomicAdd on int32, which is associative: bit-exact in any order.
// The entry point zeroes dist first.  Bytes at and past P of a row are replaced in registers (0 for l2, 255 for mismatch: no class), a
// row past M or K re-reads the last valid row and is never written, so nothing outside the caller's rows is touched.
//
// s2e_rank_topk: one workgroup per row sorts the row's (distance, index) keys in LDS (bitonic, 64-bit keys: the biased distance above
// the index, so ascending keys are ascending distance with ties to the lower index) and writes the first k.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4_t;

constexpr int SR_TILE = 64;                                 // targets and candidates of one wave's tile: 4 x 4 MFMA tiles
constexpr int SR_SUB = SR_TILE / 16;
constexpr int SR_STEP = 64;                                 // bytes of a row one MFMA contracts
constexpr int SR_WAVES = 4;                                 // waves of a workgroup: four consecutive pixel chunks of one tile
constexpr int SR_LD = SR_TILE + 1;                          // row stride of the workgroup's tile in LDS, in words
constexpr int SR_MIN_STEPS = 8;                             // a chunk is at least this many steps
constexpr int SR_TARGET_WAVES = 2048;                       // waves to aim for: the two a SIMD holds at this kernel's registers, on 256 CUs
                                                            // (measured at 64 x 640 x 256 000: 4096 and 1024 are slower)
constexpr int SR_MAX_DIM = 65535 * SR_TILE;                 // M, K at most: the grid's y and z
constexpr int SR_MAX_CAND = 4096;                           // candidates of one top-k launch: 32 KiB of 8-byte keys in LDS
constexpr int SR_TOPK_THREADS = 1024;

// 16 bytes of a row at byte `off` (a multiple of 16), bytes at and past P replaced by `fill`.  off + 16 <= pitch always holds for
// off < P, because pitch >= P is a multiple of 16: a load never leaves the row.
__device__ __forceinline__ u32x4_t sr_load(const uint8_t* row, long off, long P, uint32_t fill) {
    if (off >= P) return u32x4_t{fill, fill, fill, fill};
    u32x4_t v = *(const u32x4_t*)(row + off);
    if (off + 16 > P) {
        const int valid = (int)(P - off);                   // 1 .. 15
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int nv = min(max(valid - 4 * w, 0), 4);
            const uint32_t mask = nv >= 4 ? 0xffffffffu : ((1u << (8 * nv)) - 1u);
            v[w] = (v[w] & mask) | (fill & ~mask);
        }
    }
    return v;
}

// 0x01 in every byte of x that equals the byte replicated in c4, 0x00 elsewhere
__device__ __forceinline__ uint32_t sr_eq_bytes(uint32_t x, uint32_t c4) {
    const uint32_t t = x ^ c4;
    const uint32_t nz = ((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t;        // bit 7 of a byte: the byte of t is not zero
    return (~nz >> 7) & 0x01010101u;
}
__device__ __forceinline__ i32x4_t sr_onehot(u32x4_t v, uint32_t c4) {
    return i32x4_t{(int)sr_eq_bytes(v[0], c4), (int)sr_eq_bytes(v[1], c4), (int)sr_eq_bytes(v[2], c4), (int)sr_eq_bytes(v[3], c4)};
}
__device__ __forceinline__ uint32_t sr_sumsq(u32x4_t v, uint32_t acc) {
#pragma unroll
    for (int w = 0; w < 4; ++w) acc = __builtin_amdgcn_udot4(v[w], v[w], acc, false);
    return acc;
}

// One wave: the tile at (m0, n0) over pixel chunk `chunk`, added into the workgroup's `tile` in LDS.  METRIC 0: l2, 1: mismatch.
template <int METRIC>
__device__ __forceinline__ void sr_wave_tile(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int M, int K, long P, long pitch,
                                             int ncls, int chunk_steps, int chunk, int m0, int n0, uint32_t* tile) {
    const int lane = threadIdx.x & 63;
    const int r = lane & 15, g = lane >> 4;
    const int mt = min(SR_SUB, (M - m0 + 15) >> 4), nt = min(SR_SUB, (K - n0 + 15) >> 4);      // the 16-row groups that hold a row: wave-uniform
    const uint8_t* pa[SR_SUB];
    const uint8_t* pb[SR_SUB];
#pragma unroll
    for (int i = 0; i < SR_SUB; ++i) {
        pa[i] = a + (size_t)min(m0 + 16 * i + r, M - 1) * (size_t)pitch;
        pb[i] = b + (size_t)min(n0 + 16 * i + r, K - 1) * (size_t)pitch;
    }
    const long nsteps = (P + SR_STEP - 1) / SR_STEP;
    const long s0 = (long)chunk * chunk_steps, s1 = min(s0 + (long)chunk_steps, nsteps);
    const uint32_t fill = METRIC == 0 ? 0u : 0xffffffffu;

    i32x4_t acc[SR_SUB][SR_SUB];
    uint32_t na[SR_SUB], nb[SR_SUB];
#pragma unroll
    for (int i = 0; i < SR_SUB; ++i) {
        na[i] = 0u; nb[i] = 0u;
#pragma unroll
        for (int j = 0; j < SR_SUB; ++j) acc[i][j] = i32x4_t{0, 0, 0, 0};
    }
    u32x4_t fa[SR_SUB], fb[SR_SUB], qa[SR_SUB], qb[SR_SUB];
    auto load = [&](long s, u32x4_t* ua, u32x4_t* ub) {
        const long off = s * SR_STEP + 16 * g;
#pragma unroll
        for (int i = 0; i < SR_SUB; ++i) {
            ua[i] = i < mt ? sr_load(pa[i], off, P, fill) : u32x4_t{fill, fill, fill, fill};
            ub[i] = i < nt ? sr_load(pb[i], off, P, fill) : u32x4_t{fill, fill, fill, fill};
        }
    };
    if (s0 < s1) load(s0, fa, fb);
    for (long s = s0; s < s1; ++s) {
        if (s + 1 < s1) load(s + 1, qa, qb);                                     // the next step's fragments are in flight under this step's MFMAs
        if constexpr (METRIC == 0) {
#pragma unroll
            for (int i = 0; i < SR_SUB; ++i) { na[i] = sr_sumsq(fa[i], na[i]); nb[i] = sr_sumsq(fb[i], nb[i]); }
#pragma unroll
            for (int i = 0; i < SR_SUB; ++i)
                if (i < mt) {
#pragma unroll
                    for (int j = 0; j < SR_SUB; ++j)
                        if (j < nt)
                            acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4_t, fa[i]), __builtin_bit_cast(i32x4_t, fb[j]),
                                                                              acc[i][j], 0, 0, 0);
                }
        } else {
            for (int c = 0; c < ncls; ++c) {
                const uint32_t c4 = 0x01010101u * (uint32_t)c;
                i32x4_t oa[SR_SUB], ob[SR_SUB];
#pragma unroll
                for (int i = 0; i < SR_SUB; ++i) { oa[i] = sr_onehot(fa[i], c4); ob[i] = sr_onehot(fb[i], c4); }
#pragma unroll
                for (int i = 0; i < SR_SUB; ++i)
                    if (i < mt) {
#pragma unroll
                        for (int j = 0; j < SR_SUB; ++j)
                            if (j < nt) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(oa[i], ob[j], acc[i][j], 0, 0, 0);
                    }
            }
        }
        if (s + 1 < s1) {
#pragma unroll
            for (int i = 0; i < SR_SUB; ++i) { fa[i] = qa[i]; fb[i] = qb[i]; }
        }
    }

    // the chunk's share of every distance: into the workgroup's tile in LDS, which then goes to dist with one atomicAdd per element
    // (uint32: wraps like int32, and the total fits)
    uint32_t base = 0u;
    if constexpr (METRIC == 0) {
#pragma unroll
        for (int i = 0; i < SR_SUB; ++i) {                                      // the four 16-byte groups of a row: every lane gets the row's norm
            na[i] += __shfl_xor(na[i], 16, 64); na[i] += __shfl_xor(na[i], 32, 64);
            nb[i] += __shfl_xor(nb[i], 16, 64); nb[i] += __shfl_xor(nb[i], 32, 64);
        }
    } else {
        base = (uint32_t)(min(P, s1 * SR_STEP) - s0 * SR_STEP);                 // the chunk's pixels
    }
#pragma unroll
    for (int i = 0; i < SR_SUB; ++i) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t na_row = METRIC == 0 ? (uint32_t)__shfl((int)na[i], 4 * g + q, 64) : 0u;       // lane 4 g + q holds row 4 g + q of group i
            const int row = m0 + 16 * i + 4 * g + q;
#pragma unroll
            for (int j = 0; j < SR_SUB; ++j) {
                const int col = n0 + 16 * j + r;
                const uint32_t d = (uint32_t)acc[i][j][q];
                const uint32_t v = METRIC == 0 ? na_row + nb[j] - 2u * d : base - d;
                if (i < mt && j < nt && row < M && col < K) atomicAdd(&tile[(16 * i + 4 * g + q) * SR_LD + 16 * j + r], v);
            }
        }
    }
}

// grid (ceil(nchunks / 4), ceil(K / 64), ceil(M / 64)), 256 threads.
template <int METRIC>
__global__ __launch_bounds__(256) void mask_dist_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int M, int K, long P,
                                                        long pitch, int ncls, int chunk_steps, int nchunks, uint32_t* __restrict__ dist) {
    __shared__ uint32_t tile[SR_TILE * SR_LD];                                  // the workgroup's four partial tiles, summed
    const int chunk = blockIdx.x * SR_WAVES + (threadIdx.x >> 6);
    const int m0 = blockIdx.z * SR_TILE, n0 = blockIdx.y * SR_TILE;
    for (int e = threadIdx.x; e < SR_TILE * SR_LD; e += 64 * SR_WAVES) tile[e] = 0u;
    __syncthreads();
    if (chunk < nchunks)                                                        // (wave-uniform; a wave without a chunk only keeps the barriers)
        sr_wave_tile<METRIC>(a, b, M, K, P, pitch, ncls, chunk_steps, chunk, m0, n0, tile);
    __syncthreads();
    for (int e = threadIdx.x; e < SR_TILE * SR_TILE; e += 64 * SR_WAVES) {
        const int row = m0 + (e >> 6), col = n0 + (e & 63);
        if (row < M && col < K) atomicAdd(dist + (size_t)row * K + col, tile[(e >> 6) * SR_LD + (e & 63)]);
    }
}

__global__ __launch_bounds__(256) void sr_zero_kernel(uint32_t* __restrict__ p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = 0u;
}

// grid (M), 1024 threads.  n: the power of two >= max(K, 2) that is sorted; slots past K, and the excluded candidate, hold the largest key.
__global__ __launch_bounds__(SR_TOPK_THREADS) void rank_topk_kernel(const int32_t* __restrict__ dist, int K, int k, const int32_t* __restrict__ exclude,
                                                                    int32_t* __restrict__ idx, int32_t* __restrict__ val, int n) {
    __shared__ unsigned long long key[SR_MAX_CAND];
    const size_t row = blockIdx.x;
    const int tid = threadIdx.x;
    int ex = exclude ? exclude[row] : -1;
    if (ex < 0 || ex >= K) ex = -1;
    for (int i = tid; i < n; i += SR_TOPK_THREADS) {
        unsigned long long kk = ~0ull;
        if (i < K && i != ex) kk = ((unsigned long long)((uint32_t)dist[row * K + i] ^ 0x80000000u) << 32) | (uint32_t)i;
        key[i] = kk;
    }
    __syncthreads();
    for (int size = 2; size <= n; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (n >> 1); t += SR_TOPK_THREADS) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;       // i < j < n
                const bool up = (i & size) == 0;
                const unsigned long long x = key[i], y = key[j];
                if ((x > y) == up) { key[i] = y; key[j] = x; }
            }
            __syncthreads();
        }
    }
    const int count = K - (ex >= 0 ? 1 : 0);
    for (int j = tid; j < k; j += SR_TOPK_THREADS) {
        int32_t oi = -1, ov = -1;
        if (j < count) { const unsigned long long kk = key[j]; oi = (int32_t)(uint32_t)kk; ov = (int32_t)((uint32_t)(kk >> 32) ^ 0x80000000u); }
        idx[row * (size_t)k + j] = oi;
        val[row * (size_t)k + j] = ov;
    }
}

}  // namespace

extern "C" int s2e_mask_dist(const uint8_t* a, const uint8_t* b, int M, int K, long P, long pitch, int ncls, int metric, int32_t* dist,
                             void* stream) {
    if (!a || !b || !dist) S2E_FAIL(S2E_ERR_ARG, "s2e_mask_dist: bad argument");
    if (metric != S2E_RANK_L2 && metric != S2E_RANK_MISMATCH) S2E_FAIL(S2E_ERR_ARG, "s2e_mask_dist: bad metric %d", metric);
    if (M < 1 || K < 1 || P < 1) S2E_FAIL(S2E_ERR_ARG, "s2e_mask_dist: M=%d K=%d P=%ld (every size must be at least 1)", M, K, P);
    if (pitch < P) S2E_FAIL(S2E_ERR_ARG, "s2e_mask_dist: pitch=%ld is below P=%ld", pitch, P);
    if ((pitch & 15) || ((uintptr_t)a & 15) || ((uintptr_t)b & 15) || ((uintptr_t)dist & 3))
        S2E_FAIL(S2E_ERR_ARG, "s2e_mask_dist: a, b and pitch must be multiples of 16 bytes, dist of 4");
    const int max_cls = metric == S2E_RANK_L2 ? 128 : 16;
    if (ncls < 1 || ncls > max_cls) S2E_FAIL(S2E_ERR_UNSUPPORTED, "s2e_mask_dist: ncls=%d (1 to %d classes for this metric)", ncls, max_cls);
    if ((long)(ncls - 1) * (ncls - 1) * P > 2147483647L || P > 2147483647L)     // ((ncls - 1)^2 <= 16129: the product fits a long)
        S2E_FAIL(S2E_ERR_UNSUPPORTED, "s2e_mask_dist: (ncls-1)^2 P = %d^2 x %ld does not fit int32", ncls - 1, P);
    if (M > SR_MAX_DIM || K > SR_MAX_DIM) S2E_FAIL(S2E_ERR_UNSUPPORTED, "s2e_mask_dist: M=%d K=%d is beyond the launch limits (at most %d each)", M, K, SR_MAX_DIM);
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)M * (size_t)K;
    sr_zero_kernel<<<s2e_grid1d((long)n, 4096), 256, 0, st>>>((uint32_t*)dist, n);
    S2E_CHECK_LAUNCH("sr_zero_kernel");
    // the split of the pixel axis: from the sizes alone (and any split gives the same bits)
    const long nsteps = (P + SR_STEP - 1) / SR_STEP;
    const long tiles = (long)ceil_div(M, SR_TILE) * ceil_div(K, SR_TILE);
    long want = SR_TARGET_WAVES / tiles;
    if (want < 1) want = 1;
    long chunk_steps = (nsteps + want - 1) / want;
    if (chunk_steps < SR_MIN_STEPS) chunk_steps = SR_MIN_STEPS;
    const long nchunks = (nsteps + chunk_steps - 1) / chunk_steps;              // <= 4096
    const dim3 grid((unsigned)ceil_div(nchunks, SR_WAVES), (unsigned)ceil_div(K, SR_TILE), (unsigned)ceil_div(M, SR_TILE));
    if (metric == S2E_RANK_L2)
        mask_dist_kernel<0><<<grid, 64 * SR_WAVES, 0, st>>>(a, b, M, K, P, pitch, ncls, (int)chunk_steps, (int)nchunks, (uint32_t*)dist);
    else
        mask_dist_kernel<1><<<grid, 64 * SR_WAVES, 0, st>>>(a, b, M, K, P, pitch, ncls, (int)chunk_steps, (int)nchunks, (uint32_t*)dist);
    S2E_CHECK_LAUNCH("mask_dist_kernel");
    return S2E_OK;
}

extern "C" int s2e_rank_topk_max_candidates(void) { return SR_MAX_CAND; }

extern "C" int s2e_rank_topk(const int32_t* dist, int M, int K, int k, const int32_t* exclude, int32_t* idx, int32_t* val, void* stream) {
    if (!dist || !idx || !val) S2E_FAIL(S2E_ERR_ARG, "s2e_rank_topk: bad argument");
    if (M < 1 || K < 1 || k < 1) S2E_FAIL(S2E_ERR_ARG, "s2e_rank_topk: M=%d K=%d k=%d (every size must be at least 1)", M, K, k);
    if (K > SR_MAX_CAND) S2E_FAIL(S2E_ERR_UNSUPPORTED, "s2e_rank_topk: K=%d candidates, one launch takes %d (rank chunks, then the winners)", K, SR_MAX_CAND);
    int n = 2;
    while (n < K) n <<= 1;
    rank_topk_kernel<<<M, SR_TOPK_THREADS, 0, (hipStream_t)stream>>>(dist, K, k, exclude, idx, val, n);
    S2E_CHECK_LAUNCH("rank_topk_kernel");
    return S2E_OK;
}
