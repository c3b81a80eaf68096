// Shared device/host helpers for the Seg2Eye gfx950 kernels.
// gfx950 (CDNA4) only: 64-wide wavefronts, MFMA, 160 KiB LDS per CU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <type_traits>
#include "../../include/seg2eye_hip.h"

typedef __bf16 bf16_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) short s16x4_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
// native 16-B vector used for ALL type-punned 16-B global/LDS accesses: HIP's uint4 struct copies lower to
// memcpy (defeats SROA), and without may_alias clang's TBAA miscompiles float memory read through it
typedef __attribute__((ext_vector_type(4), may_alias)) uint32_t u32x4_t;
typedef __attribute__((ext_vector_type(2), may_alias)) uint32_t u32x2_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;

// ---------------------------------------------------------------- error reporting (host)
void s2e_set_error(const char* fmt, ...);
#define S2E_FAIL(code, ...) do { s2e_set_error(__VA_ARGS__); return (code); } while (0)
#define S2E_CHECK_LAUNCH(name) do { hipError_t e_ = hipGetLastError(); \
    if (e_ != hipSuccess) S2E_FAIL(S2E_ERR_LAUNCH, "%s: launch failed: %s", name, hipGetErrorString(e_)); } while (0)

// ---------------------------------------------------------------- 16-byte vector <-> float lanes
template <typename T> struct Vec;
template <> struct Vec<float>  { static constexpr int N = 4; };
template <> struct Vec<bf16_t> { static constexpr int N = 8; };

__device__ __forceinline__ float bf16_bits_to_f32(uint32_t b16) { return __builtin_bit_cast(float, b16 << 16); }
__device__ __forceinline__ uint32_t f32_to_bf16_bits(float f) {
    bf16_t h = (bf16_t)f;                                   // v_cvt_pk_bf16_f32: RNE, NaN stays NaN
    return (uint32_t)__builtin_bit_cast(unsigned short, h);
}

// NOTE: take the vector BY VALUE and index with []: hipcc (ROCm 7.2) miscompiles
// __builtin_bit_cast(float, r.x) on a const-reference ext-vector (loads element 0 only).
template <typename T> __device__ __forceinline__ void unpack16(u32x4_t r, float* f);
template <> __device__ __forceinline__ void unpack16<float>(u32x4_t r, float* f) {
    const uint32_t r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
    f[0] = __builtin_bit_cast(float, r0); f[1] = __builtin_bit_cast(float, r1);
    f[2] = __builtin_bit_cast(float, r2); f[3] = __builtin_bit_cast(float, r3);
}
template <> __device__ __forceinline__ void unpack16<bf16_t>(u32x4_t r, float* f) {
    const uint32_t r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
    f[0] = bf16_bits_to_f32(r0 & 0xffffu); f[1] = __builtin_bit_cast(float, r0 & 0xffff0000u);
    f[2] = bf16_bits_to_f32(r1 & 0xffffu); f[3] = __builtin_bit_cast(float, r1 & 0xffff0000u);
    f[4] = bf16_bits_to_f32(r2 & 0xffffu); f[5] = __builtin_bit_cast(float, r2 & 0xffff0000u);
    f[6] = bf16_bits_to_f32(r3 & 0xffffu); f[7] = __builtin_bit_cast(float, r3 & 0xffff0000u);
}
template <typename T> __device__ __forceinline__ u32x4_t pack16(const float* f);
template <> __device__ __forceinline__ u32x4_t pack16<float>(const float* f) {
    return u32x4_t{__builtin_bit_cast(uint32_t, f[0]), __builtin_bit_cast(uint32_t, f[1]),
                   __builtin_bit_cast(uint32_t, f[2]), __builtin_bit_cast(uint32_t, f[3])};
}
template <> __device__ __forceinline__ u32x4_t pack16<bf16_t>(const float* f) {
    return u32x4_t{f32_to_bf16_bits(f[0]) | (f32_to_bf16_bits(f[1]) << 16),
                   f32_to_bf16_bits(f[2]) | (f32_to_bf16_bits(f[3]) << 16),
                   f32_to_bf16_bits(f[4]) | (f32_to_bf16_bits(f[5]) << 16),
                   f32_to_bf16_bits(f[6]) | (f32_to_bf16_bits(f[7]) << 16)};
}
typedef __attribute__((ext_vector_type(2))) float f32x2_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
// two floats -> one dword of two bf16 (RNE) in ONE v_cvt_pk_bf16_f32 (pack16 converts element by element: cvt + shift + or per pair)
__device__ __forceinline__ uint32_t pack2_bf16(float lo, float hi) {
    const f32x2_t v = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));
}
template <typename T> __device__ __forceinline__ float load1(const T* p) { return (float)*p; }
template <typename T> __device__ __forceinline__ void store1(T* p, float v) { *p = (T)v; }

__device__ __forceinline__ float lrelu02(float v) { return v > 0.f ? v : 0.2f * v; }
// LeakyReLU(0.2) on 16 B of packed T.  PK (bf16): round each pair with one v_cvt_pk_bf16_f32 (pack2_bf16) instead of pack16's
// element-wise form; the bits are the same, the instructions are not, and each user keeps the form it was tuned with.
template <typename T, bool PK = false>
__device__ __forceinline__ u32x4_t lrelu16(u32x4_t r) {
    float f[Vec<T>::N];
    unpack16<T>(r, f);
#pragma unroll
    for (int j = 0; j < Vec<T>::N; ++j) f[j] = lrelu02(f[j]);
    if constexpr (PK) return u32x4_t{pack2_bf16(f[0], f[1]), pack2_bf16(f[2], f[3]), pack2_bf16(f[4], f[5]), pack2_bf16(f[6], f[7])};
    else return pack16<T>(f);
}

// ---------------------------------------------------------------- address spaces, LDS-DMA, counted waits
typedef const __attribute__((address_space(1))) void* gptr_t;            // global
typedef const __attribute__((address_space(1))) float* gptr_f32_t;
typedef const __attribute__((address_space(1))) f32x4_t* gptr_f32x4_t;
typedef __attribute__((address_space(3))) void* lptr_t;                  // LDS
// 16 zero bytes: the source of the LDS-DMA lanes that are out of bounds (padding taps, rows / channels past the tensor)
__device__ __attribute__((aligned(16))) const uint32_t s2e_zero16[4] = {0u, 0u, 0u, 0u};
// LDS-DMA, 16 B per lane: the wave's 1 KiB lands lane-linear at dst (wave-uniform); src is per lane.  (conv_patch.hip calls the
// builtin itself: through this helper its code changes.)
__device__ __forceinline__ void lds_dma16(const void* src, void* dst) {
    __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)dst, 16, 0, 0);
}
// all but the newest N vector-memory operations (LDS-DMA included) of this wave are done
template <int N> __device__ __forceinline__ void wait_vmcnt() {
    static_assert(N >= 0 && N <= 63, "vmcnt is a 6-bit counter");
    asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory");
}
// (the kernels' ladders over a run-time count -- conv_duo, conv_patch, conv_stream, conv_wgrad_flat -- stay with their kernels: their
// shapes differ, and conv_duo's compiles to other code through a shared recursive form)
// (the multi-job kernels' search for a workgroup's job -- conv_wgrad.hip twice, conv_wgrad_flat.hip, conv_c8.hip -- stays written out in
// each: through a shared helper, by pointer or by reference to the argument block, all four compile to other code)
// ds_read_b64_tr_b16, the hardware 4x16 transpose read (lane roles: conv_wgrad.hip)
__device__ __forceinline__ u32x2_t lds_tr16_b64(const char* p) {
    s16x4_t v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4_t __attribute__((address_space(3)))*)p);
    return __builtin_bit_cast(u32x2_t, v);
}
// two bf16 from two LDS addresses into one register: the low half by ds_read_u16 (zero-extended), the high half by
// ds_read_u16_d16_hi into a second register, OR-ed after the wait.  (A d16_hi read does NOT preserve the other half on
// this target -- with SRAM ECC the destination's unused half is written as zero -- so the pair cannot share a register.)
#define S2E_U16_PAIR(lo, hi, addr, off_lo, off_hi) \
    asm volatile("ds_read_u16 %0, %1 offset:%2" : "=v"(lo) : "v"(addr), "n"(off_lo) : "memory"); \
    asm volatile("ds_read_u16_d16_hi %0, %1 offset:%2" : "=v"(hi) : "v"(addr), "n"(off_hi) : "memory")

// ---------------------------------------------------------------- 32x32 MFMA on 16-B operands
template <typename T> struct Mfma;
template <> struct Mfma<bf16_t> {
    static __device__ __forceinline__ void run(u32x4_t a, u32x4_t b, f32x16_t& acc) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a),
                                                      __builtin_bit_cast(bf16x8_t, b), acc, 0, 0, 0);
    }
};
template <> struct Mfma<float> {
    // lane half h holds 4 consecutive k; MFMA t pairs element t of half 0 with element t of half 1.
    // A and B use the same (permuted) k order, so the contraction is exact.
    // (vectors by value + whole-vector bit_cast: see the note at unpack16)
    static __device__ __forceinline__ void run(u32x4_t a, u32x4_t b, f32x16_t& acc) {
        const f32x4_t fa = __builtin_bit_cast(f32x4_t, a), fb = __builtin_bit_cast(f32x4_t, b);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[0], fb[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[1], fb[1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[2], fb[2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[3], fb[3], acc, 0, 0, 0);
    }
};

// ---------------------------------------------------------------- wave / block reductions
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// the fp64 form the loss and metric kernels take their per-workgroup partials with: the same xor butterfly, 32 down to
// 1, the total in every lane.  The order of these adds is part of every result that goes through them.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// a 256-thread block's sum of v (fp64), valid in thread 0: the lanes by the butterfly above, then the four waves as
// ((r0 + r1) + r2) + r3.  That order is part of the result: another association gives other bits.  red: four doubles of LDS; one
// barrier.  (The butterfly is written out, not a call of wave_sum: through the call its users schedule one instruction elsewhere.)
__device__ __forceinline__ double block_sum4(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// sum over the 64 lanes in six DPP adds (VALU only, unlike the ds_bpermute butterflies above); the total is valid in LANE 63 only
__device__ __forceinline__ float wave_sum_last(float v) {
#define S2E_DPP_ADD(ctrl, rmask) v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, rmask, 0xF, false))
    S2E_DPP_ADD(0xB1, 0xF);        // quad_perm [1,0,3,2]
    S2E_DPP_ADD(0x4E, 0xF);        // quad_perm [2,3,0,1]
    S2E_DPP_ADD(0x141, 0xF);       // row_half_mirror
    S2E_DPP_ADD(0x140, 0xF);       // row_mirror: every lane of a 16-lane row holds the row's sum
    S2E_DPP_ADD(0x142, 0xA);       // row_bcast15 into rows 1 and 3
    S2E_DPP_ADD(0x143, 0xC);       // row_bcast31 into rows 2 and 3
#undef S2E_DPP_ADD
    return v;
}

// XCD-aware bijective remap of a 1-D grid: blocks that share (bid % 8) sit on one XCD
// (observed round-robin placement; speed only, never correctness) and get a contiguous
// range of logical tile ids, so neighbouring tiles reuse operand panels in that XCD's L2.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

// compile-time loop: f(integral_constant<int, I>) for I in [0, N) -- indices stay constants, so small
// per-thread arrays are always register-allocated (never scratch / LDS-promoted)
template <int I> using int_c = std::integral_constant<int, I>;
template <int I, int N, typename F> __device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) { f(int_c<I>{}); static_for<I + 1, N>(f); }
}

// Zero-fill as a KERNEL, never hipMemsetAsync: inside a captured hipGraph (ROCm 7.x) memset nodes were
// observed to race with neighbouring kernel nodes (first replay fine, later replays corrupt), while
// kernel nodes are strictly ordered.  bytes must be a multiple of 4; ptr 4-byte aligned.
__global__ void s2e_zero_kernel(uint32_t* __restrict__ p, size_t n_words);
int s2e_zero_async(void* ptr, size_t bytes, hipStream_t st);

static inline int ceil_div(long a, long b) { return (int)((a + b - 1) / b); }
// a byte count rounded up to the 256 bytes every section of a workspace starts on
static inline size_t s2e_align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
// do the byte ranges [a, a + na) and [b, b + nb) overlap?  (NULL or empty: no range.)  Jobs of one call may write the same dw / dbias
static inline bool s2e_ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    if (!a || !b || !na || !nb) return false;
    return (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
}

// ---------------------------------------------------------------- dtype dispatch and launch geometry (host)
// f(T{}) with T the element type of dtype; any other dtype is S2E_ERR_ARG "<name>: bad dtype <dtype>".  A launcher whose dtype must be
// refused ahead of its other checks says S2E_CHECK_DTYPE there: the dispatcher refuses only where it is called.
template <typename F> static inline int s2e_with_dtype(int dtype, const char* name, F&& f) {
    if (dtype == S2E_BF16) return f(bf16_t{});
    if (dtype == S2E_F32) return f(float{});
    S2E_FAIL(S2E_ERR_ARG, "%s: bad dtype %d", name, dtype);
}
#define S2E_CHECK_DTYPE(dtype, name) do { if ((dtype) != S2E_BF16 && (dtype) != S2E_F32) S2E_FAIL(S2E_ERR_ARG, "%s: bad dtype %d", name, dtype); } while (0)
static inline int s2e_vec_lanes(int dtype) { return dtype == S2E_BF16 ? 8 : 4; }      // elements of a 16-byte vector (Vec<T>::N)
static inline int s2e_k_tile(int dtype) { return dtype == S2E_BF16 ? 64 : 32; }       // K elements of one MFMA tile step; s2e_conv_k_pad pads to it
// 256-thread blocks for n items of a grid-stride kernel, at most cap
static inline int s2e_grid1d(long n, int cap = 8192) { const long b = (n + 255) / 256; return (int)(b < cap ? b : cap); }
static inline int s2e_pow2_shift(int v) { for (int b = 0; b < 31; ++b) if ((1 << b) == v) return b; return -1; }   // log2 of a power of two, else -1
// a caller's buffer (what: a string literal, "workspace") of `have` bytes where the launch needs `need`
#define S2E_CHECK_BYTES(name, what, have, need) do { if ((have) < (need)) \
    S2E_FAIL(S2E_ERR_ARG, "%s: " what " of %zu bytes, needs %zu", name, (size_t)(have), (size_t)(need)); } while (0)
// N single-channel H x W images, one grid.y per image and 32-bit pixel indices over the batch
static inline int s2e_check_image_batch(const char* name, int N, int H, int W) {
    if (N > 65535 || (long)N * H * W >= (1L << 31))
        S2E_FAIL(S2E_ERR_UNSUPPORTED, "%s: N=%d H=%d W=%d is beyond the launch limits (N <= 65535, N H W < 2^31)", name, N, H, W);
    return S2E_OK;
}

// S2E_DETERMINISTIC=1 (read once per process): every gradient of the train step is summed in a fixed order -- the generic weight
// gradient's partial tiles for every split launch, one reduction pass instead of several combined with float atomics, the patch
// weight gradient's bias sums through the workspace -- so that two runs of a trainer produce the same bits.
// Costs ~0.5 ms per step; off by default.  (The logged loss VALUES and the bilinear resize's backward still use float atomics.)
int s2e_deterministic(void);

// compute units of the current device (read once per process); 256 when there is no device (planning calls on a CPU-only machine)
int s2e_cu_count(void);

// Environment switches (DESIGN.md section 4 lists every one).  Callers keep the value in a function-local static: read once per process.
static inline int s2e_env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
static inline bool s2e_env_flag(const char* name, bool dflt) { return s2e_env_int(name, dflt) != 0; }
// the value when it is set and >= lo, else the default
static inline int s2e_env_int_ge(const char* name, int lo, int dflt) { const int v = s2e_env_int(name, dflt); return v >= lo ? v : dflt; }
static inline long s2e_env_long(const char* name, long dflt) { const char* e = getenv(name); return e ? atol(e) : dflt; }
static inline double s2e_env_double(const char* name, double dflt) { const char* e = getenv(name); return e ? atof(e) : dflt; }
