// The weight packers: OIHW (or channels-last) fp32 masters -> the MFMA B-operand layouts in the compute dtype, one conv or every conv
// of a network per launch.  Spectral norm enters only as an optional 1 / sigma: W / sigma never exists in memory, the packers
// divide on the fly while converting.
#include "common.h"
#include "conv_plane.h"
// OIHW fp32 -> MFMA B-operand layout in the compute dtype, divided by *sigma when sigma != NULL.
// Both directions go through LDS so that global reads AND writes are contiguous runs.
// Every element of the padded matrix is written exactly once per call (padding rows / channels / K tail as
// zeros), so no separate zero-fill is needed.
// Thread mapping as in the gradient re-layout kernels of weight_grad.hip: no per-element integer division.
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
