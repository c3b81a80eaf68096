/* seg2eye_hip.h -- C ABI of libseg2eye_hip.so (gfx950 / MI355X kernels for the Seg2Eye
 * G+D train-step hot path).
 *
 * The reference (mcbuehler/Seg2Eye) has NO native code and no FFI: every op on
 * the path is a stock torch call.  Each entry point below therefore replaces a *group of torch
 * calls* in the reference, cited as file:line under /root/reference.  The host-side mirror of the
 * reference's plugin boundary (models.networks.define_G/define_D, Pix2PixModel, Pix2PixTrainer)
 * lives in seg2eye_amd/ and binds these symbols with ctypes.
 *
 * Conventions
 *  - extern "C", plain pointers and ints; no torch / C++ types.  All pointers are DEVICE pointers
 *    owned by the caller.  The library never allocates or frees device memory, never synchronises,
 *    launches only on the given stream (a hipStream_t passed as void*), uses the current device.
 *  - Every function returns S2E_OK (0) or a negative S2E_ERR_*; s2e_last_error() gives the
 *    thread-local message.  Re-entrant; no mutable globals.
 *  - dtype: S2E_F32 or S2E_BF16 = storage type of activations / packed weights and the MFMA input
 *    type; accumulation, statistics, losses and weight gradients are always fp32 (or fp64 where
 *    noted).
 *  - Activations are NHWC contiguous: element (n, y, x, c) at ((n*H + y)*W + x)*C + c.  That is the
 *    storage of a torch channels_last tensor of logical shape (N, C, H, W).
 *  - Label maps are uint8 (N, H, W), values < 4.
 */
#ifndef SEG2EYE_HIP_H
#define SEG2EYE_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define S2E_OK 0
#define S2E_ERR_ARG (-1)
#define S2E_ERR_LAUNCH (-2)
#define S2E_ERR_UNSUPPORTED (-3)

enum { S2E_F32 = 0, S2E_BF16 = 1 };
enum { S2E_ACT_NONE = 0, S2E_ACT_LRELU = 1, S2E_ACT_TANH = 2 };          /* LeakyReLU slope 0.2 */
enum { S2E_AUX_NONE = 0, S2E_AUX_RELU_MASK = 1, S2E_AUX_LRELU_GRAD = 2 }; /* y *= (aux>0 ? 1 : 0 | 0.2) */
enum { S2E_NORM_SPADE_STYLE = 0, S2E_NORM_PLAIN_IN = 1,
       S2E_NORM_SPADE_STYLE_BATCH = 2,     /* s2e_modulate_bwd only: stats are BATCH statistics (BatchNorm SPADE) */
       S2E_NORM_ACCUMULATE_DX = 0x100 };   /* s2e_modulate_bwd only, OR-ed into mode: dx += instead of dx = (dx holds the
                                              gradient another consumer of the same x has already written) */
enum { S2E_LOSS_NEG_MEAN = 0, S2E_LOSS_HINGE_REAL = 1, S2E_LOSS_HINGE_FAKE = 2, S2E_LOSS_L1 = 3,
       S2E_LOSS_L1_NANGRAD = 4 };          /* L1 whose GRADIENT is NaN for a NaN difference (torch's, and S2E_LOSS_L1's, is 0) */

int s2e_version(void);
const char* s2e_last_error(void);

/* ------------------------------------------------------------------ convolution (implicit GEMM, MFMA)
 * Replaces nn.Conv2d forward / backward at: models/networks/generator.py:30,48 (fc, conv_img),
 * architecture.py:24-27 (conv_0, conv_1, conv_s), normalization.py:85-89 (mlp_gamma, mlp_beta),
 * discriminator.py:84-96 (4x4 convs), encoder.py:23-28,37-39 (3x3 s2 convs).
 *
 * x is (N, Hi, Wi, Cin), y is (N, Ho, Wo, Cout); both NHWC.
 * transposed = 0:  y[n,oy,ox,co] = sum_{ky,kx,ci} x[n, oy*stride-pad+ky, ox*stride-pad+kx, ci] * W[co][ky][kx][ci]
 * transposed = 1 (data gradient of a conv with this stride/pad; x plays grad_out, y plays grad_in):
 *                  y[n,oy,ox,co] = sum x[n, (oy+pad-ky)/stride, (ox+pad-kx)/stride, ci] * W[co][ky][kx][ci]
 *                  over taps where the division is exact and in range.
 * W is the packed matrix written by s2e_pack_conv_weight: row co, column (ky*KW+kx)*Cin + ci.
 * Prologue:  in_act  applied to x as it is loaded (S2E_ACT_NONE | S2E_ACT_LRELU).
 * Epilogue:  v = acc + bias[co] (bias may be NULL) + residual[n,oy,ox,co] (may be NULL);
 *            v = out_act(v);  v *= aux-derived mask (aux has y's shape; may be NULL).
 * stride in {1,2}.  Any Cin / Cout; the 16-byte vector path needs Cin % (16/sizeof(T)) == 0. */
typedef struct {
    int N, Hi, Wi, Cin;
    int Ho, Wo, Cout;
    int KH, KW, stride, pad;
    int transposed;
    int in_act, out_act, aux_mode;
} s2e_conv_desc;

int s2e_conv_cout_pad(int cout);                 /* rows of a packed weight matrix    */
int s2e_conv_k_pad(int dtype, int k);            /* columns of a packed weight matrix */
/* w_oihw: fp32 (cout, cin, kh, kw) contiguous (torch layout).  cin_pad >= cin: channels
 * cin..cin_pad-1 of the activation are structural zeros (e.g. the 5->8 padded D input).
 * sigma: NULL, or a DEVICE fp32 scalar: the packed weight is w / *sigma (spectral norm applied on
 * the fly; W/sigma is never materialised in fp32).
 * transposed = 0: packed[co][(ky*kw+kx)*cin_pad + ci]           (cout_pad(cout) x k_pad(kh*kw*cin_pad))
 * transposed = 1: packed[ci][(ky*kw+kx)*cout + co]              (cout_pad(cin_pad) x k_pad(kh*kw*cout))
 * transposed | 2: the SOURCE is stored channels-last, w[co][ky][kx][ci] (the fp32 masters of a trainer: DESIGN 3.4b); needs
 * cin_pad == cin and cin % 8 == 0.  Same outputs; the forward pack is then a streaming convert, the transposed one a tile
 * transpose per tap.  transposed | 4 (bf16, cin_pad == cin, K dimension a multiple of 32): the PLANE layout of s2e_conv2d_plane
 * (csrc/conv_plane.h), ceil(rows / 64) * 64 x taps * K elements.  s2e_pack_job.transposed takes the same values. */
int s2e_pack_conv_weight(int dtype, const float* w_oihw, void* packed, const float* sigma, int cout, int cin,
                         int kh, int kw, int cin_pad, int transposed, void* stream);
/* Batched weight pack: every conv of a network in ONE launch (a network packs 20-50 weight matrices per
 * forward; as separate 8 us launches that was 1.6 ms of a 35 ms step).  jobs / block_map are DEVICE arrays the
 * caller builds once: fill a host s2e_pack_job array, call s2e_pack_block_map to count (block_map_host NULL)
 * and then fill the {job, bx, by} triples, upload both.  sigma_index >= 0 divides by sigma_base[sigma_index]
 * (the sigma array s2e_sn_power_iteration wrote for this forward).  Outputs as s2e_pack_conv_weight. */
typedef struct s2e_pack_job {
    const float* w;          /* OIHW fp32 */
    void* out;               /* packed matrix, compute dtype, s2e_conv_cout_pad(rows) x s2e_conv_k_pad(...) */
    int sigma_index;         /* or -1 */
    int cout, cin, taps, cin_pad, transposed;
    void* out_fwd;           /* transposed == 3 jobs (channels-last source, transposed pack) only, or NULL: the forward pack of the same
                              * weight ([co][tap * cin + ci], row pitch s2e_conv_k_pad(taps * cin)) is written from the same read of the
                              * master (round 6).  Only the weight's own elements: zero that matrix's padding once yourself. */
} s2e_pack_job;
long s2e_pack_block_map(int dtype, const s2e_pack_job* jobs_host, int n_jobs, int* block_map_host);
int s2e_pack_conv_weights(int dtype, const s2e_pack_job* jobs, const int* block_map, int n_blocks, int max_taps,
                          const float* sigma_base, void* stream);

/* The bytes of `workspace` the kernel this shape routes to needs (0: none): the fp32 partial slabs of a layer split over K
 * because its output tiling alone cannot fill the chip (implicit GEMM, and the patch kernel's channel-chunk splits; a finishing
 * kernel sums the slabs and applies the epilogue), or the stream-K kernel's two partial tiles per CU.  Deterministic, no atomics;
 * the caller allocates (no initialisation needed) and s2e_conv2d refuses a smaller workspace with S2E_ERR_ARG. */
size_t s2e_conv2d_workspace_bytes(int dtype, const s2e_conv_desc* d);
/* Which kernel s2e_conv2d / s2e_conv2d_wgrad run for this shape (for profilers and tests; the choice is made inside the
 * library from the shape alone): S2E_KERNEL_GENERIC = implicit GEMM (conv_igemm.hip / conv_wgrad.hip),
 * S2E_KERNEL_SMALL = the 1-channel streaming kernels and the 8-channel first layer of the PatchGAN (conv_c8.hip), S2E_KERNEL_PATCH = the patch-resident kernels (3x3 / 4x4 stride 1, and the
 * 4x4 stride-2 pad-2 layers through the space-to-depth view). */
enum { S2E_KERNEL_GENERIC = 0, S2E_KERNEL_SMALL = 1, S2E_KERNEL_PATCH = 2 };
int s2e_conv2d_kernel_kind(int dtype, const s2e_conv_desc* d);
int s2e_conv2d_wgrad_kernel_kind(int dtype, const s2e_conv_desc* d);
int s2e_conv2d(int dtype, const void* x, const void* w_packed, const float* bias, const void* residual,
               const void* aux, void* y, const s2e_conv_desc* d, void* workspace, size_t workspace_bytes,
               void* stream);
/* Plane-patch convolution (round 6; csrc/conv_plane.hip): netE's 3x3 stride-2 convs (reference models/networks/encoder.py:23-39)
 * forward and data gradient, and the learned 1x1 shortcuts (architecture.py:26-27,53-56), patch-resident with the input patch of a
 * stride-2 layer stored as four parity planes in LDS (9 taps executed, each a shifted view of one plane) and the weights streamed
 * from L2 straight into registers.  s2e_conv2d_plane_supported: 0, or the mode (> 0) this kernel runs the shape in -- the caller
 * then packs the weight in the PLANE layout (s2e_pack_conv_weight with transposed | 4: s2e_conv_plane_weight_elems(d) bf16 elements,
 * for a 4-KB block per (64 rows, 32-channel chunk, tap) in MFMA fragment order) and calls s2e_conv2d_plane instead of s2e_conv2d;
 * same operands and epilogue contract otherwise (bias, residual OR mask, LeakyReLU), no workspace.  S2E_CONV_PLANE (environment, bit
 * mask of modes) = 0 disables it.  bf16 only. */
int s2e_conv2d_plane_supported(int dtype, const s2e_conv_desc* d);
size_t s2e_conv_plane_weight_elems(const s2e_conv_desc* d);
int s2e_conv2d_plane(int dtype, const void* x, const void* w_plane, const float* bias, const void* residual, const void* aux,
                     void* y, const s2e_conv_desc* d, void* stream);
/* The forward convolution TOGETHER with the InstanceNorm partial sums of its output y (round 4; SURVEY 7 step 5: the statistics of
 * a large map -- normalization.py:94 of the reference, nn.InstanceNorm2d on the tensor the previous conv produced,
 * architecture.py:53-60 -- come out of the producer's epilogue instead of a pass over y).  s2e_conv2d_stats_slots: the partial-sum
 * slots per sample the launch writes, or 0 when this shape's kernel has no such epilogue (then: s2e_conv2d + s2e_in_stats).
 * part: (N, slots, Cout, 2) floats {sum y, sum y^2} over the slot's pixels, of the values as stored (rounded to the compute
 * dtype); uninitialised on entry.  Feed it to s2e_in_stats_from_partials.  residual as in s2e_conv2d; no mask operand. */
int s2e_conv2d_stats_slots(int dtype, const s2e_conv_desc* d);
int s2e_conv2d_stats(int dtype, const void* x, const void* w_packed, const float* bias, const void* residual, void* y,
                     const s2e_conv_desc* d, float* part, void* stream);
/* Weight gradient of the forward conv described by d (d->transposed must be 0):
 * dw[co][(ky*KW+kx)*Cin + ci] += sum_{n,oy,ox} gy[n,oy,ox,co] * in_act(x)[n, oy*s-p+ky, ox*s-p+kx, ci]
 * dw: fp32 (Cout x KH*KW*Cin), row-major, ACCUMULATED into (caller zeroes it); split over pixels:
 * generic shapes split 16 ways or more (S2E_WGRAD_PARTIAL: the threshold; 2 = every split launch, 0 = never) store
 * their 128x128 partial tiles in `workspace` and a second kernel sums them in a fixed order into dw (deterministic);
 * below the threshold, or given no workspace, the splits add into dw with fp32 atomics.  dbias: NULL, or fp32 (Cout) ACCUMULATED with the bias gradient
 * sum_{n,oy,ox} gy[n,oy,ox,co] from the gy tiles the kernel stages anyway (no extra pass over gy).
 * The 1-channel shapes (Cout == 1 or Cin == 1: conv_img, the PatchGAN heads, the encoder's first layer)
 * run as HBM streams whose per-block partial rows go through `workspace` and are summed by a second
 * kernel; the big bf16 3x3 stride-1 layers (patch-resident kernel, one workgroup per CU) store their per-workgroup
 * partial tiles there too (<= 75 MB) and fold them into dw with a reduction pass.
 * s2e_conv2d_wgrad_workspace_bytes(d) is 0 for a shape that needs none (workspace may then be NULL; a patch-kernel or
 * generic shape given no workspace falls back to atomics).  The caller allocates; no initialisation needed. */
size_t s2e_conv2d_wgrad_workspace_bytes(int dtype, const s2e_conv_desc* d);
int s2e_conv2d_wgrad(int dtype, const void* x, const void* gy, float* dw, float* dbias, const s2e_conv_desc* d,
                     void* workspace, size_t workspace_bytes, void* stream);

/* Every GENERIC weight gradient of a backward pass in ONE launch (round 6; VERDICT r5 #3: launches, not microseconds): the learned 1x1
 * shortcuts (reference models/networks/architecture.py:26-27), netE's stride-2 layers (encoder.py:23-39), the PatchGAN's 4x4 layers
 * (discriminator.py:84-96) and the 8x8 maps each ran as a 30-160 us launch that fills the chip badly and ends with a tail, plus a
 * reduction launch for the split ones; here their workgroups run side by side (csrc/conv_wgrad.hip, conv_wgrad_multi_kernel), followed
 * by ONE reduction launch for all jobs that store partial tiles.  Same sums as s2e_conv2d_wgrad job by job (dw / dbias ACCUMULATED).
 * Jobs may share dw and / or dbias (any overlap of the Cout x KH*KW*Cin and Cout float ranges): every job's sum is added; where
 * several jobs add into one element the result depends on their order in the last bit.
 * bf16, Cin and Cout multiples of 8, shapes s2e_conv2d_wgrad would run in its generic kernel (s2e_conv2d_wgrad_multi_supported).
 * workspace: s2e_conv2d_wgrad_multi_workspace_bytes(jobs) (uninitialised; less or none: those jobs add with fp32 atomics). */
typedef struct s2e_wgrad_multi_job {
    const void* x; const void* gy; float* dw; float* dbias;
    s2e_conv_desc d;                                   /* the forward conv (transposed = 0) */
} s2e_wgrad_multi_job;
int s2e_conv2d_wgrad_multi_supported(int dtype, const s2e_conv_desc* d);
size_t s2e_conv2d_wgrad_multi_workspace_bytes(int dtype, const s2e_wgrad_multi_job* jobs, int n_jobs);
int s2e_conv2d_wgrad_multi(int dtype, const s2e_wgrad_multi_job* jobs, int n_jobs, void* workspace, size_t workspace_bytes, void* stream);
/* Which kernel a job of s2e_conv2d_wgrad_multi runs in: 0 = the generic 128 x 128 tile kernel (partial tiles in the workspace + one reduction);
 * 1..5 = the flat-slab patch-resident kernel of csrc/conv_wgrad_flat.hip (round 6: 1 = 1x1, 2 = 3x3 stride 1, 3 = 3x3 stride 2 pad 1,
 * 4 = 4x4 stride 1 pad 2, 5 = 4x4 stride 2 pad 2; Cin a multiple of 64, no input activation; fp32 atomics into dW, no workspace) -- the
 * weight-gradient half of encoder.py:26-40 and discriminator.py:78-93's stride-2 / 4x4 layers; 6 = the 8-channel 4x4 stride-2 kernel of
 * csrc/conv_c8.hip (the PatchGAN's first layer, discriminator.py:78-85; fp32 atomics, no workspace); -1 = not a job of that call.
 * S2E_WGRAD_FLAT (environment, bit k = kind k) selects the kinds that leave the generic kernel. */
int s2e_conv2d_wgrad_multi_kind(int dtype, const s2e_conv_desc* d);

/* ------------------------------------------------------------------ spectral normalisation
 * torch.nn.utils.spectral_norm as applied at architecture.py:30-34 and normalization.py:25-26
 * (n_power_iterations=1, eps 1e-12, dim 0), for ALL spectral-normed convs of a
 * network at once.  Per layer, W = weight_orig viewed (rows=Cout) x (cols=Cin*kh*kw), row-major:
 *   train != 0 (per iteration): v = normalize(W^T u); u = normalize(W v); sigma = u . (W v)   (u, v updated in place)
 *   train == 0:                 sigma = u . (W v)                                              (u, v untouched)
 * layers: DEVICE array of n_layers descriptors.  sigma: fp32 [n_layers] out.
 * train: `iterations` launches of one kernel, each reading every W ONCE (a workgroup owns a column strip of W and forms its share of
 * both products from it), plus one finalising launch.  strip_map: DEVICE int32 [n_strips][2] = {layer, first column}, covering
 * every layer's columns in strips of the width s2e_sn_block_shape(1, ..) reports (its rows: how many rows of a strip are held in
 * registers; taller layers are walked in chunks).  Any order; neighbours in the map run together, so strips of ONE layer, which
 * all add into that layer's y, are best kept apart.
 * eval: two launches.  block_map: DEVICE int32 [n_blocks][3] = {layer, row0, col0} covering every layer with the tiles
 * s2e_sn_block_shape(0, ..) reports.
 * The workgroups' partial sums are combined with INTEGER atomics on fixed-point values, every other sum runs in a fixed order, so u, v
 * and sigma are a function of (W, u, v, iterations) alone: identical run to run and on every data-parallel replica.  The
 * accumulators live in `scratch`, which must be ZERO on the first call (the kernels leave it zero again: no fill per call). */
typedef struct {
    const float* w; float* u; float* v;
    float* t;                         /* train: t = W^T u of the latest iteration, [cols] */
    long long* s;                     /* eval: W v in units of 2^-40, [rows]; may alias y */
    int rows, cols;
    float* tq;                        /* train: |t_J|^2 of every strip, [2][ceil(cols / strip width)] (by iteration parity) */
    long long* y;                     /* train: W t as [3][2][rows] (buffers in rotation x {units of 2^-20, residual in units of 2^-60}) */
    int cin, taps;                    /* taps > 1: w is stored channels-last, [co][tap][ci] (cols = taps * cin, cin % 4 == 0), while v
                                       * keeps torch's (ci, tap) order: the kernels translate.  0, 0: w's columns are v's order. */
} s2e_sn_layer;
int s2e_sn_block_shape(int which, int* rows, int* cols);   /* which = 0: tiles of block_map (eval, W v); 1: the strip of strip_map (train) */
int s2e_sn_power_iteration(const s2e_sn_layer* layers, int n_layers, const int* strip_map, int n_strips,
                           const int* block_map, int n_blocks,
                           void* scratch, size_t scratch_bytes, float* sigma, int train, int iterations,
                           float eps, void* stream);
/* Gradient through W = W_orig / sigma (sigma = u^T W_orig v; u, v constants):
 *   gw_orig (=|+=) gW / sigma - (<gW, W_orig> / sigma^2) * u v^T     in OIHW order,
 * with gW given in the packed order of s2e_conv2d_wgrad ([co][(tap)*cin_pad + ci]).  dot_ws: 1 float of scratch, ZERO-FILLED by the caller.
 * accumulate != 0 adds into gw_orig (e.g. straight into the optimizer's gradient arena). */
int s2e_sn_weight_grad(const float* gw_packed, const float* w_orig, const float* u, const float* v, const float* sigma,
                       float* dot_ws, float* gw_orig, int cout, int cin, int kh, int kw, int cin_pad, int accumulate,
                       void* stream);
/* The same chain rule IN PLACE, for masters stored channels-last ([co][tap][ci] = the packed order, so that s2e_conv2d_wgrad
 * accumulates straight into the parameter's gradient): g = g / sigma - (<g, W_orig> / sigma^2) u v^T for every job, two
 * launches, deterministic (per-block partial dot products, added in a fixed order).  g and w: the (rows x taps*cin) matrices in
 * memory order, cin % 8 == 0; u (rows), v (cin*taps, torch's (ci, tap) order), sigma: as above.  s2e_sngrad_block_map fills
 * part0 / nparts / vmem0 of the HOST jobs and the {job, chunk} pairs; partials: s2e_sngrad_scratch_floats floats (one per block, then
 * every layer's v re-ordered to W's memory order by the first launch), no initialisation needed. */
typedef struct s2e_sngrad_job {
    float* g; const float* w; const float* u; const float* v; const float* sigma;
    int rows, cin, taps, part0, nparts, vmem0;
} s2e_sngrad_job;
long s2e_sngrad_block_map(s2e_sngrad_job* jobs_host, int n_jobs, int* block_map_host);
long s2e_sngrad_scratch_floats(const s2e_sngrad_job* jobs_host, int n_jobs);     /* size of `partials`, after s2e_sngrad_block_map */
int s2e_sn_grads_inplace(const s2e_sngrad_job* jobs, const int* block_map, int n_blocks, float* partials, void* stream);
/* gw_oihw[co][ci][ky][kx] (=|+=) gw_packed[co][(ky*kw+kx)*cin_pad + ci]: packed weight gradient -> torch layout. */
int s2e_unpack_weight_grad(const float* gw_packed, float* gw_oihw, int cout, int cin, int kh, int kw, int cin_pad,
                           int accumulate, void* stream);
/* The two calls above for EVERY conv of a step in two launches (a step has ~95 of them, most a few microseconds of
 * work: as separate launches they cost 1.2 ms).  jobs / block_map are DEVICE arrays (host side: fill s2e_grad_job[],
 * s2e_grad_block_map to count with block_map_host NULL and then to fill {job, first tile, tiles} triples, upload).
 * w_orig != NULL marks a spectral-normed layer (u, v, sigma, dot_index must then be set; dots: zero-filled scratch with
 * one float per such layer).  Every job ACCUMULATES into its out. */
typedef struct s2e_grad_job {
    const float* gw_packed;      /* [cout][taps*cin_pad] fp32 from s2e_conv2d_wgrad */
    float* out;                  /* OIHW fp32 gradient (e.g. the parameter's slice of the gradient arena) */
    const float* w_orig;         /* spectral norm: weight_orig (OIHW); NULL: plain re-layout */
    const float* u;
    const float* v;
    const float* sigma;
    int cout, cin, taps, cin_pad, dot_index, reserved;
} s2e_grad_job;
long s2e_grad_block_map(const s2e_grad_job* jobs_host, int n_jobs, int* block_map_host);
int s2e_weight_grads_batched(const s2e_grad_job* jobs, const int* block_map, int n_blocks, int max_taps, int any_sn,
                             float* dots, void* stream);

/* ------------------------------------------------------------------ InstanceNorm statistics
 * nn.InstanceNorm2d(affine=False) statistics, normalization.py:73 / :41 (biased variance, eps 1e-5).
 * x (N, HW, C) -> stats (N, C, 2) fp32 = {mean, rstd}.  ws: s2e_in_stats_workspace_bytes(...) bytes of scratch, no
 * initialisation needed: the row-walking blocks write per-block partial sums there (no atomics) and the finalising kernel
 * adds them in a fixed order in fp64 -- the statistics are bit-reproducible.  On return the first N*C*2 doubles of ws hold
 * {sum x, sum x^2} per (n, c) (BatchNorm SPADE combines them over the batch). */
size_t s2e_in_stats_workspace_bytes(int dtype, int N, int HW, int C);
int s2e_in_stats(int dtype, const void* x, int N, int HW, int C, float eps, double* ws, float* stats, void* stream);

/* {mean, rstd} (and, in ws, the fp64 {sum x, sum x^2}) from P partial-sum slots per sample written by another kernel
 * (s2e_conv2d_stats): part (N, P, C, 2) floats, ws N*C*2 doubles, stats (N, C, 2) floats; HW = pixels per sample.  The slots of a
 * (sample, channel) are added in a fixed order in fp64: bit-reproducible. */
int s2e_in_stats_from_partials(const float* part, int N, int P, int C, int HW, float eps, double* ws, float* stats, void* stream);

/* ------------------------------------------------------------------ SPADE+Style modulation / IN+LeakyReLU
 * mode S2E_NORM_SPADE_STYLE (SPADE_STYLE_Block.forward normalization.py:184-192 + SPADE.forward :91-105
 * + ApplyStyle.forward :163-169, optionally followed by architecture.py:61 LeakyReLU):
 *     out = 0.5*( (x-mean)*rstd*(1+gamma) + beta + x*(1+s0) + s1 ),  gamma = gb[..., :C], beta = gb[..., C:]
 *     style (N, 2C) fp32 = {s0 | s1} (already through FC + LeakyReLU, normalization.py:135-141)
 * mode S2E_NORM_PLAIN_IN (InstanceNorm2d + LeakyReLU of discriminator.py:91-94, encoder.py IN):
 *     out = (x-mean)*rstd            (gb, style unused; may be NULL)
 * lrelu != 0 applies LeakyReLU(0.2) to out: slope 0.2 unless the argument is > 0 (torch's convention), so every backward
 * below takes 0.2 AT zero too -- an exactly constant channel gets the same gradient whichever kernel its map size selects. */
int s2e_modulate_fwd(int dtype, int mode, const void* x, const void* gb, const float* stats, const float* style,
                     void* out, int N, int HW, int C, int lrelu, int style_ld, void* stream);
/* The [gamma | beta] conv of a SPADE and the SPADE+Style modulation in ONE kernel (SPADE.forward normalization.py:97-105 +
 * ApplyStyle.forward :163-169 + SPADE_STYLE_Block.forward :184-192 [+ LeakyReLU architecture.py:61]):
 *     [gamma | beta] = conv3x3(actv; nh -> 2C, pad 1) + bias          (w_packed: s2e_pack_conv_weight of [W_gamma; W_beta],
 *                                                                     rows 0..C-1 gamma, C..2C-1 beta; bias fp32 [2C] or NULL)
 *     out = 0.5*( (x-mean)*rstd*(1+gamma) + beta + x*(1+s0) + s1 )    [LeakyReLU(0.2) if lrelu]
 * gamma and beta go from the fp32 accumulators straight into the result: they are never written to memory (SURVEY 8(d):
 * "need never exist in HBM").  gamma_out: NULL (no-grad forward), or (N,H,W,C): gamma is stored for s2e_modulate_bwd's
 * gamma-only form (its `out` argument).  actv (N,H,W,nh), x / out (N,H,W,C) NHWC; stats (N,C,2); style / style_ld as s2e_modulate_fwd.
 * Taken shapes (s2e_spade_conv_modulate_supported != 0): C % 64 == 0, nh a multiple of the 128-byte K row, enough
 * 256-pixel x 64-channel tiles to fill the chip (S2E_SPADE_ANY_TILES: any tile count -- tests).  Other shapes return
 * S2E_ERR_UNSUPPORTED: run s2e_conv2d + s2e_modulate_fwd.
 * flags, of every entry point of the fused launch and of the host functions in front of them (ops.spade_style_fused): */
#define S2E_SPADE_ANY_TILES 1   /* the fused launch at any tile count (tests; the duo kernel leaves such a launch to conv_patch.hip) */
#define S2E_SPADE_DENSE     2   /* the dense launch whatever the label map; read by the host only, the library never sees it matter */
#define S2E_SPADE_ANY_RECTS 4   /* the label-sparse form at any rectangle count; read by the host only */
#define S2E_SPADE_X_HALF    8   /* x is the tensor BEFORE the nearest 2x upsampling: (N, H/2, W/2, C), see below */
int s2e_spade_conv_modulate_supported(int dtype, int N, int H, int W, int C, int nh, int flags);
int s2e_spade_conv_modulate(int dtype, const void* actv, const void* w_packed, const float* bias, const void* x,
                            const float* stats, const float* style, int style_ld, void* out, void* gamma_out,
                            int N, int H, int W, int C, int nh, int lrelu, int flags, void* stream);
/* Backward of s2e_modulate_fwd / s2e_spade_conv_modulate given g = dL/dout: ONE entry point.  Writes dx (N,HW,C), dgb (N,HW,2C) =
 * [dgamma | dbeta] (the operand of the conv's weight / data gradients) and ACCUMULATES dstyle (N,2C) fp32 (SPADE_STYLE modes only;
 * gb, style, dgb, dstyle may be NULL in PLAIN_IN mode).
 * style_ld (forward and backward): floats between consecutive samples' rows of style AND dstyle; 0 = dense (2C).  A
 * generator keeps the style codes of all its SPADE+Style layers as column slices of ONE (N, sum 2C) matrix
 * (one GEMM for all style FCs, networks/stylebank.py), hence the leading dimension.
 * ws: s2e_modulate_bwd_workspace_bytes(...) bytes of scratch, no initialisation needed (N*C*4 fp64 sums, N*C float4
 * coefficients, then the row-walking blocks' partial sums: plain stores, added up in a fixed order -- no atomics).
 * mode: S2E_NORM_PLAIN_IN, S2E_NORM_SPADE_STYLE, or S2E_NORM_SPADE_STYLE_BATCH: `stats` holds the same {mean, rstd} of the whole
 *   batch for every sample (param_free_norm = BatchNorm2d, normalization.py:74-75) and the normalisation's backward sums over N*HW.
 *   | S2E_NORM_ACCUMULATE_DX: dx = dx_add + this layer's gradient.  dx_add NULL or == dx: in place (dx holds another consumer's
 *   gradient of the same x).  dx_add apart from dx: dx_add is left alone -- a relayed gradient (architecture.py:53-60: the block
 *   input feeds both SPADEs and the shortcut) whose tensor a queued weight-gradient job still has to read; refused without the flag.
 * out: NULL: gb = (N,HW,2C) [gamma | beta], the LeakyReLU mask is recomputed from them.  Else (SPADE_STYLE modes only, the forward
 *   went through s2e_spade_conv_modulate): gb = gamma alone, (N,HW,C) (what that call stored in gamma_out; beta was never written),
 *   and the mask is taken from the sign of the forward's output `out` (N,HW,C).
 * stage: 0 = the whole backward.  1 and 2 split it for BatchNorm SPADE under data parallelism (the per-channel sums of the
 *   normalisation's backward must be summed over ALL replicas' samples, as torch SyncBatchNorm does -- the 2C-float exchange of
 *   SURVEY 8 f4):
 *   stage 1: the row-walking pass only: dgb written, the per-(n,c) fp64 sums left in ws as (N,C,4) {S0, S1, S2, S3};
 *   (caller: all-reduce sum over samples of S0, S1 across the replicas and fold the difference into ws[0,:,0:2])
 *   stage 2: coefficients + dx, with the normalisation count batch_count (= world * N * HW; 0 = N * HW) in BATCH mode.
 * x_up_w != 0 (`out` given, stage 0, per-sample statistics, even H and W): x is (N, H/2, W/2, C) with W = x_up_w -- the generator's
 *   nearest 2x upsampling in front of the block folded into the read of x, as S2E_SPADE_X_HALF does in the forward launches; g, gamma, out,
 *   dx, dgb are at full resolution -- unless dx_quad != 0 (SPADE_STYLE mode): then dx (and dx_add) is (N, H/2, W/2, C), the gradient
 *   w.r.t. the half-resolution x itself (each element the sum over the 2 x 2 pixels it was replicated to: the upsampling's
 *   backward folded in). */
int s2e_modulate_bwd(int dtype, int mode, const void* g, const void* x, const void* gb, const void* out,
                     const float* stats, const float* style, void* dx, const void* dx_add, void* dgb, float* dstyle, double* ws,
                     int N, int HW, int C, int lrelu, int style_ld, int stage, double batch_count, int x_up_w,
                     int dx_quad, void* stream);
size_t s2e_modulate_bwd_workspace_bytes(int dtype, int N, int HW, int C);
/* InstanceNorm2d(affine=False) [+ LeakyReLU 0.2] as ONE call each way (reference discriminator.py:91-94, encoder.py:23-39 via
 * normalization.py:38-50): out = [lrelu]((x - mean) * rstd); stats (N,C,2) {mean, rstd} out (forward) / in (backward).
 * Maps of up to 1280 pixels take one launch per call (a block owns all rows of its sample and channels); larger ones run
 * s2e_in_stats + s2e_modulate_fwd / s2e_modulate_bwd in PLAIN_IN mode.  ws: s2e_in_stats_workspace_bytes (forward),
 * s2e_modulate_bwd_workspace_bytes (backward); no initialisation needed. */
int s2e_instance_norm_fwd(int dtype, const void* x, void* out, float* stats, double* ws, int N, int HW, int C,
                          float eps, int lrelu, void* stream);
int s2e_instance_norm_bwd(int dtype, const void* g, const void* x, const float* stats, void* dx, double* ws,
                          int N, int HW, int C, int lrelu, void* stream);
/* The weight (and bias) gradients of MANY 8-channel-input 3x3 convs in one call -- a generator's 19 mlp_shared convs
 * (normalization.py:97, backward): x = the one-hot label map at the layer's resolution (N,H,W,8), gy = d(hidden activation),
 * masked (N,H,W,128), both bf16.  dw_oihw fp32 (128, ncls, 3, 3) -- the parameter's own layout -- and dbias fp32 (128) are
 * ACCUMULATED into.  jobs is a HOST array (it travels in the kernel arguments).  _supported: bf16, 128 output channels, a map
 * whose best 128-pixel slab covers it to >= 80 % (16 x 16 and up). */
typedef struct s2e_wgrad_c8_job {
    const void* x; const void* gy; float* dw_oihw; float* dbias;
    int H, W, ncls;
    /* round 6, both or neither (H, W multiples of 16): only the pixels of the 16 x 16 rectangles rect_list[0 .. *rect_count) (device
     * memory; rectangle r = (n * (H/16) + ty) * (W/16) + tx) contribute -- the label-sparse SPADE backward, whose d(actv) exists
     * on those rectangles only: gy outside them is never read (it need not be initialised) */
    const int* rect_list; const int* rect_count;
} s2e_wgrad_c8_job;
int s2e_wgrad_c8_batch_supported(int dtype, int H, int W, int cout);
size_t s2e_wgrad_c8_batch_workspace_bytes(int N, const s2e_wgrad_c8_job* jobs, int n_jobs);
int s2e_wgrad_c8_batch(int dtype, int N, const s2e_wgrad_c8_job* jobs, int n_jobs, void* workspace, size_t workspace_bytes,
                       void* stream);
/* The patch-resident 3x3 stride-1 pad-1 weight gradients of MANY layers as ONE persistent launch (csrc/conv_wgrad_batch.hip; the
 * weight-gradient half of architecture.py:24-25 / normalization.py:88-89's convolutions, which torch's autograd runs layer by layer).
 * Job: x (N,H,W,Cin) and gy (N,H,W,Cout) bf16; dw fp32 (Cout, 9*Cin) row-major in (tap, ci) order -- a channels-last parameter
 * gradient -- and dbias fp32 (Cout) or NULL are ACCUMULATED into.  rect_list / rect_count (both or neither): restrict the job to the
 * pixels of the 16 x 16 rectangles rect_list[0 .. *rect_count) (device memory, read by the kernel: label-sparse SPADE backward).
 * All jobs' (tile, 128-pixel slab) units are dealt evenly to one workgroup per CU; a dW tile with a single owner is added without
 * atomics or workspace, the others through <= 3 partial tiles per workgroup (WB_SLOTS) and a fix-up launch.  No two jobs of a call may share
 * dw.  jobs is a HOST array.  _supported: bf16, H % 8 == 0, W % 16 == 0 (16 with a list), Cin % 64 == 0, Cout % 8 == 0, Cout >= 64.
 * flags & S2E_WGRAD_BATCH_DW_ZERO: the caller vouches that dw holds zeros (a gradient arena cleared at the start of the step, no other
 * contribution yet): a tile with a single owner is then STORED instead of read, added and stored.
 * workspace: s2e_wgrad_batch_workspace_bytes() (independent of the jobs), uninitialised. */
#define S2E_WGRAD_BATCH_DW_ZERO 1
typedef struct s2e_wgrad_batch_job {
    const void* x; const void* gy; float* dw; float* dbias;
    const int* rect_list; const int* rect_count;
    int N, H, W, Cin, Cout;
    int flags;                                         /* S2E_WGRAD_BATCH_DW_ZERO */
} s2e_wgrad_batch_job;
int s2e_wgrad_batch_supported(int dtype, int N, int H, int W, int Cin, int Cout);
size_t s2e_wgrad_batch_workspace_bytes(void);
int s2e_wgrad_batch(int dtype, const s2e_wgrad_batch_job* jobs, int n_jobs, void* workspace, size_t workspace_bytes, void* stream);
/* Label-sparse form of the fused launch.  gamma / beta at a pixel depend only on the labels of its 5x5 neighbourhood, so a
 * rectangle of the fused launch's tiling (s2e_spade_conv_modulate_rect: tw x th pixels) whose pixels and in-image 2-pixel halo
 * all carry ONE class takes them from a per-class table instead of the convolution -- exact up to fp32 summation order, and
 * the common case on eye-region maps (72 % of the rectangles at 256^2 on the bench's maps):
 *   s2e_label_rect_classify     : cls[r] = class | 255 per rectangle r = (n*tiles_y + ty)*tiles_x + tx of the nearest-downsampled
 *                                 (h x w) label map; compact lists of the dense and of the uniform rectangles, in rectangle
 *                                 order; counts[2] = {dense, uniform} (written).  Once per label batch and resolution.
 *   s2e_spade_conv_modulate_sparse: s2e_spade_conv_modulate over the rectangles dense_list[0 .. counts[0]) only.
 *   s2e_spade_class_table       : table[class][cy][cx][2C] fp32 = the SPADE's [gamma | beta] branch (mlp_shared -> ReLU -> the packed
 *                                 [gamma | beta] conv, with all biases) on a map that is ONE class everywhere, per position class
 *                                 (cy, cx) in {0, 1, interior, H-2, H-1}^2: zero padding makes the two outermost pixel rings differ.
 *                                 w_sh fp32 (nh, ncls, 3, 3), nh <= 128; w_packed as the conv launches take it.
 *   s2e_spade_modulate_uniform  : the modulation of the rectangles uni_list[0 .. counts[1]) with gamma | beta from that table.
 * Together the two launches write every pixel of out (and gamma_out) exactly once.
 * S2E_SPADE_X_HALF of the conv launches / x_up of the uniform one: x is (N, H/2, W/2, C) -- the nearest 2x upsampling that precedes the
 * block in the generator (generator.py:77-92) is folded into the read of x, the upsampled tensor is never read (H, W even;
 * out and gamma_out are at full resolution). */
int s2e_spade_conv_modulate_rect(int dtype, int N, int H, int W, int C, int nh, int flags, int* tw, int* th);
/* Label-sparse BACKWARD of the SPADE branch (round 4; csrc/spade_sparse_bwd.hip has the algebra): in a 16 x 16 rectangle whose pixels and
 * 2-pixel halo carry one class and lie inside the image, mlp_shared's gradients need only nine shifted sums of d[gamma | beta] and
 * the [gamma | beta] conv's weight gradient is a rank-1 update per class; the branch's convolutions (normalization.py:97-103
 * differentiated) run on the other rectangles only.
 *   s2e_label_rect_lists_bwd : cls from s2e_label_rect_classify (16 x 16 rectangles) -> work_list (dense, or uniform on the image
 *                              border), ui_list (uniform-interior), counts[2] (written).
 *   s2e_conv2d_rects         : s2e_conv2d over the rectangles rect_list[0 .. *rect_count) only (the other pixels of y are not
 *                              written); s2e_conv2d_rects_supported: does this shape's kernel take a list (16 x 16 rectangles)?
 *   s2e_spade_uniform_sums   : R (S2E_UNI_REPLICAS, ncls, 9, 2C) fp32, ZEROED by the caller, += sum over the uniform-interior
 *                              rectangles of class c of dgb[q - t + 1] (tap t = 3 ky + kx); fp32 atomics, spread over the replicas
 *                              (a thousand rectangles add to four class slots); s2e_spade_uniform_grads folds the replicas.
 *   s2e_spade_uniform_grads  : for up to 16 layers at once: A (ncls, nh) fp32 ZEROED scratch; dw_sh (nh, ncls, 3, 3) / db_sh (nh)
 *                              ACCUMULATED; w_gb = the [gamma | beta] conv's fp32 weight (2C, nh, 3, 3) with element strides
 *                              (w_sc, w_sk, w_st) for (co, k, tap); dw_gb / db_gb: NULL, or the same-strided weight gradient and
 *                              the bias gradient, ACCUMULATED with the uniform rectangles' rank-1 part.  act_bf16: the hidden
 *                              activation is stored in bf16 (its ReLU mask is taken from the rounded value). */
#define S2E_UNI_REPLICAS 16
typedef struct s2e_spade_uni_job {
    const float* R; float* A; const float* w_gb; long w_sc, w_sk, w_st;
    const float* w_sh; const float* b_sh; float* dw_sh; float* db_sh; float* dw_gb; float* db_gb;
    int C2, nh, ncls, act_bf16;
} s2e_spade_uni_job;
int s2e_label_rect_lists_bwd(const uint8_t* cls, int N, int tiles_y, int tiles_x, int* work_list, int* ui_list, int* counts, void* stream);
int s2e_conv2d_rects_supported(int dtype, const s2e_conv_desc* d);
int s2e_conv2d_rects(int dtype, const void* x, const void* w_packed, const float* bias, const void* residual, const void* aux, void* y,
                     const s2e_conv_desc* d, const int* rect_list, const int* rect_count, void* stream);
/* s2e_conv2d_wgrad restricted to the pixels of rect_list[0 .. *rect_count) (16 x 16 rectangles): the [gamma | beta] conv's weight
 * gradient on the rectangles that cross a label boundary; s2e_conv2d_wgrad_rects_workspace_bytes = 0: this shape takes no list. */
size_t s2e_conv2d_wgrad_rects_workspace_bytes(int dtype, const s2e_conv_desc* d);
int s2e_conv2d_wgrad_rects(int dtype, const void* x, const void* gy, float* dw, float* dbias, const s2e_conv_desc* d,
                           const int* rect_list, const int* rect_count, void* workspace, size_t workspace_bytes, void* stream);
int s2e_spade_uniform_sums(int dtype, const void* dgb, int N, int H, int W, int C2, int ncls, const uint8_t* cls, const int* ui_list,
                           const int* counts, float* R, void* stream);
int s2e_spade_uniform_grads(const s2e_spade_uni_job* jobs_host, int n_jobs, void* stream);
int s2e_label_rect_classify(const uint8_t* label, int N, int H, int W, int h, int w, int tw, int th,
                            uint8_t* cls, int* dense_list, int* uni_list, int* counts, void* stream);
int s2e_spade_conv_modulate_sparse(int dtype, const void* actv, const void* w_packed, const float* bias, const void* x,
                                   const float* stats, const float* style, int style_ld, void* out, void* gamma_out,
                                   int N, int H, int W, int C, int nh, int lrelu, int flags, const int* dense_list,
                                   const int* counts, void* stream);
int s2e_spade_class_table(int dtype, const float* w_sh, const float* b_sh, const void* w_packed, const float* bias,
                          float* table, int ncls, int nh, int C, void* stream);
/* s2e_spade_class_table for every label-sparse layer of a forward in one launch (tables at table_base + table_off bytes). */
typedef struct s2e_class_table_job {
    const float* w_sh; const float* b_sh; const void* w_packed; const float* bias;
    long table_off;
    int nh, C;
} s2e_class_table_job;
long s2e_class_table_block_map(const s2e_class_table_job* jobs_host, int n_jobs, int* block_map_host);
int s2e_spade_class_table_batch(int dtype, const s2e_class_table_job* jobs, const int* block_map, int n_blocks,
                                void* table_base, int ncls, void* stream);
int s2e_spade_modulate_uniform(int dtype, const void* x, const float* stats, const float* style, int style_ld,
                               const float* table, const uint8_t* cls, const int* uni_list, const int* counts,
                               void* out, void* gamma_out, int N, int H, int W, int C, int tw, int th, int lrelu, int x_up,
                               void* stream);
/* out[c] += sum_m g[m][c]  (conv bias gradient).  g (M, C); out fp32 (C). */
int s2e_colsum(int dtype, const void* g, long M, int C, float* out, void* stream);

/* ------------------------------------------------------------------ label-map ops
 * conv3x3(pad 1) of the nearest-downsampled ONE-HOT label map, without materialising the one-hot:
 * out[n,y,x,co] = bias[co] + sum_{ky,kx in bounds} weight[co][label_h[n,y+ky-1,x+kx-1]][ky][kx]
 * with label_h[y][x] = label[y*(H/h)][x*(W/w)] (F.interpolate 'nearest', integer ratio), then ReLU
 * if relu != 0.  Replaces SPADE.mlp_shared (normalization.py:85-88,97-98) and the generator's
 * fc conv on the downsampled segmap (generator.py:72-73).  weight: the conv's fp32 OIHW weight
 * (Cout, ncls, 3, 3) as it sits in the parameter arena (each block gathers its table from it into LDS). */
/* All label convs of a generator forward in one launch (the 19 mlp_shared convs of the SPADE layers, normalization.py:97, most of
 * them a few microseconds of work): jobs is a DEVICE array (cout <= 128 each; outputs at out_base + out_off bytes, so the table
 * is built once and the per-forward output buffer is one allocation); block_map DEVICE int32 triples from
 * s2e_label_conv_block_map (block_map_host NULL: count only).  Same numbers as s2e_label_conv3x3 per job. */
typedef struct s2e_label_conv_job {
    const float* weight;     /* (cout, ncls, 3, 3) fp32 */
    const float* bias;       /* (cout) fp32 or NULL */
    long out_off;            /* bytes from out_base to this job's (N, h, w, cout) output */
    int h, w, cout, relu;
} s2e_label_conv_job;
long s2e_label_conv_block_map(int dtype, const s2e_label_conv_job* jobs_host, int n_jobs, int N, int* block_map_host);
int s2e_label_conv3x3_batch(int dtype, const uint8_t* label, const s2e_label_conv_job* jobs, const int* block_map,
                            int n_blocks, void* out_base, int N, int H, int W, int ncls, void* stream);
int s2e_label_conv3x3(int dtype, const uint8_t* label, const float* weight, const float* bias, void* out,
                      int N, int H, int W, int h, int w, int ncls, int Cout, int relu, void* stream);
/* out (N,h,w,cpad): channels [0,ncls) one-hot of the nearest-downsampled label, channel ncls =
 * img[n,y,x] when img != NULL (img is (N,h,w) of T), remaining channels 0.  Builds the
 * discriminator input cat([seg, image]) (pix2pix_model.py:328-336) and the one-hot operand for
 * the mlp_shared / fc weight gradients. */
int s2e_onehot_nhwc(int dtype, const uint8_t* label, const void* img, void* out,
                    int N, int H, int W, int h, int w, int ncls, int cpad, void* stream);
/* Differentiable augmentation of the discriminator's input (an extension: the reference has none).
 * s2e_d_input_aug writes what two s2e_onehot_nhwc calls (h = H, w = W, cpad = 8) write -- out (2N,H,W,8) of T, images [0, N) from
 * `fake`, [N, 2N) from `real`, both (N,H,W) of T -- through a per-sample transform.  params: (N, 8) fp32 rows
 * [b, c, ty, tx, y0, x0, ch, cw], the last six integers stored exactly; row i serves fake i AND real i.  Output pixel (y, x) of
 * sample n has the source (sy, sx) = (y - ty, x - tx) and is VISIBLE when the source lies inside the image and (y, x) lies
 * outside the rectangle [y0, y0 + ch) x [x0, x0 + cw) (which may stick out of the image).  A visible pixel carries the one-hot
 * of label[n, sy, sx], the image channel c * v[sy, sx] + o with o = (1 - c) * mean(v) + b (the mean of THAT image, fake's and
 * real's apart; one fp32 multiply-add per pixel, o computed once per image) and zero pad channels; every other pixel is 8
 * zeros.  The row [0, 1, 0, 0, 0, 0, 0, 0] gives s2e_onehot_nhwc's bits.
 * color == 0: b and c are NOT read (taken as 0 and 1): no mean, one launch; color != 0: the means of the 2N images first (per-block
 * fp64 partial sums in ws, plain stores, folded in index order by the launch that consumes them): two launches.  The launches
 * depend on `color` alone, never on the rows' values (a captured graph keeps its shape).
 * s2e_d_input_aug_bwd: gout = the gradient of out, (2N,H,W,8) of T; dfake (N,H,W) of T =
 *   c * gout[n, sy + ty, sx + tx, ncls] where that output pixel is visible (else 0)  +  (1 - c) / (H W) * S_n,
 * S_n = the sum of gout[n, :, :, ncls] over sample n's visible pixels (first half only).  color == 0: one launch, no sum;
 * otherwise two.  Bit-reproducible: no atomics.
 * ws: s2e_d_input_aug_workspace_bytes(N, H, W) bytes (either call; 0 for a size <= 0), uninitialised; may be NULL when color == 0.
 * Before any launch: S2E_ERR_ARG on a null pointer, a size <= 0, a bad dtype or a misaligned out; S2E_ERR_UNSUPPORTED on
 * cpad != 8, ncls >= 8 or 2 N H W >= 2^31 pixels. */
size_t s2e_d_input_aug_workspace_bytes(int N, int H, int W);
int s2e_d_input_aug(int dtype, const uint8_t* label, const void* fake, const void* real, const float* params, void* out,
                    double* ws, int N, int H, int W, int ncls, int cpad, int color, void* stream);
int s2e_d_input_aug_bwd(int dtype, const void* gout, const float* params, void* dfake, double* ws,
                        int N, int H, int W, int ncls, int cpad, int color, void* stream);
/* nn.Upsample(scale_factor=2) nearest (generator.py:50): (N,h,w,C) -> (N,2h,2w,C); bwd sums 2x2. */
int s2e_upsample2x_fwd(int dtype, const void* x, void* y, int N, int h, int w, int C, void* stream);
int s2e_upsample2x_bwd(int dtype, const void* gy, void* gx, int N, int h, int w, int C, void* stream);
/* F.avg_pool2d(k=3, s=2, p=1, count_include_pad=False) (discriminator.py:46-49), NHWC.
 * Ho = (H+1)/2, Wo = (W+1)/2 (floor((H+2-3)/2)+1). */
int s2e_avgpool3x3s2_fwd(int dtype, const void* x, void* y, int N, int H, int W, int C, void* stream);
int s2e_avgpool3x3s2_bwd(int dtype, const void* gy, void* gx, int N, int H, int W, int C, void* stream);
/* F.interpolate(x, size=(Ho, Wo), mode='bilinear') (align_corners=False) of single-channel images: the encoder's front end
 * (encoder.py:54-55 resizes every style image to 256 x 256).  x: fp32 (N,H,W); y: (N,Ho,Wo) of dtype -- what the first conv
 * consumes.  bwd: gx fp32 (N,H,W), ZERO-FILLED by the caller, is accumulated into (fp32 atomics). */
int s2e_bilinear_resize_fwd(int dtype, const float* x, void* y, int N, int H, int W, int Ho, int Wo, void* stream);
int s2e_bilinear_resize_bwd(int dtype, const void* gy, float* gx, int N, int H, int W, int Ho, int Wo, void* stream);
/* gx = gy * (1 - y*y)   (backward of torch.tanh, generator.py:100). */
int s2e_tanh_bwd(int dtype, const void* gy, const void* y, void* gx, long n, void* stream);
/* gx = gy * (y > 0 ? 1 : 0.2): backward of LeakyReLU(0.2) (discriminator.py:85, nn.LeakyReLU) given its
 * OUTPUT y (LeakyReLU preserves sign, so the mask of the output equals the mask of the input). */
int s2e_lrelu_bwd(int dtype, const void* gy, const void* y, void* gx, long n, void* stream);

/* ------------------------------------------------------------------ losses
 * Scalar reductions of GANLoss hinge (loss.py:66-77) and the GAN feature-matching L1
 * (pix2pix_model.py:231-241).  out[0] += scale * sum_i f(a_i, b_i):
 *   NEG_MEAN: -a      HINGE_REAL: -min(a-1,0)      HINGE_FAKE: -min(-a-1,0)      L1: |a-b|
 * (pass scale = coefficient / n for a mean).  b is only read for L1 and L1_NANGRAD.
 * L1_NANGRAD is L1 in everything but one case of s2e_loss_grad: where a_i - b_i is NaN the derivative is NaN, not the 0 that
 * torch's sign() and L1 give -- a deliberate departure, used under the gradient guard so that a non-finite feature reaches the
 * gradient arena (and s2e_grad_guard) instead of vanishing.  Every other input gives L1's bits. */
int s2e_loss_reduce(int dtype, int mode, const void* a, const void* b, long n, float scale, float* out, void* stream);
/* da_i (=|+=) scale * upstream * d f(a_i,b_i)/d a_i ; upstream = *gscale (a DEVICE fp32 scalar, the
 * gradient of the total loss w.r.t. this term; NULL means 1) so no host sync is needed;
 * accumulate != 0 adds into da. */
int s2e_loss_grad(int dtype, int mode, const void* a, const void* b, long n, float scale, const float* gscale,
                  void* da, int accumulate, void* stream);

/* ------------------------------------------------------------------ style FCs (ApplyStyle / FC: models/networks/normalization.py:144-169)
 * All SPADE+Style layers' style codes from one latent batch:  big[n][s] = LeakyReLU_slope(b[s] + sum_k w[n][k] W[s][k]),
 * w fp32 (N x K) = the latent codes, W fp32 (S x K) / b fp32 (S) = the layers' FC weights / biases stacked along S, big fp32
 * (N x S).  N <= 32, K in {8, 16, 32, 64} (s2e_style_fc_supported).  Backward: dpre = (dbig + gbig) * LeakyReLU'(big)
 * (gbig may be NULL); gW (S x K) and gb (S) are ACCUMULATED into; dw (N x K), when not NULL, is WRITTEN -- a fixed-order
 * two-level sum over S through `workspace` (s2e_style_fc_bwd_workspace_bytes; no initialisation needed). */
int s2e_style_fc_supported(int N, int K);
size_t s2e_style_fc_bwd_workspace_bytes(int N, int K, int S);
int s2e_style_fc_fwd(const float* w, const float* W, const float* b, float* big, int N, int K, int S, float slope, void* stream);
int s2e_style_fc_bwd(const float* dbig, const float* gbig, const float* big, const float* w, const float* W, float* gW, float* gb,
                     float* dw, void* workspace, size_t workspace_bytes, int N, int K, int S, float slope, void* stream);

/* The encoder's head (models/networks/encoder.py:68-71: fc_mu / fc_var on LeakyReLU(x).view(M, -1)) on the NHWC feature map:
 *     y[m][n] = b[n] + sum_{p,c} LeakyReLU_slope(x[m][p][c]) * W[n][c*P + p]      (torch flattens (c, p))
 * x (M, P, C) in `dtype`; W (N x C*P), b, y (M x N), dy: fp32.  M <= 64, N <= 32 (s2e_fc_head_supported).  Backward, one pass:
 * dx (M, P, C) in `dtype` is WRITTEN (NULL: skipped), dW (N x C*P) and db (N) are ACCUMULATED into (NULL: skipped). */
int s2e_fc_head_supported(int M, int N);
size_t s2e_fc_head_fwd_workspace_bytes(int M, int P, int C, int N);
/* workspace (uninitialised, s2e_fc_head_fwd_workspace_bytes) given: two small launches -- 256 columns of W x 8 samples per block, the
 * partial (8, N) tiles added in a fixed order -- instead of one block per sample (NULL): 128 instead of 32 blocks, W read 4x not 32x. */
int s2e_fc_head_fwd(int dtype, const void* x, const float* W, const float* b, float* y, int M, int P, int C, int N, float slope,
                    void* workspace, size_t workspace_bytes, void* stream);
int s2e_fc_head_bwd(int dtype, const void* x, const float* W, const float* dy, void* dx, float* dW, float* db, int M, int P, int C,
                    int N, float slope, void* stream);

/* ------------------------------------------------------------------ optimizer
 * torch.optim.Adam step (pix2pix_model.py:92-110: TTUR betas (0, 0.9), eps 1e-8, --weight_decay as Adam's L2 term)
 * over one flat fp32 arena: g = g*grad_scale + weight_decay*p; m = b1*m + (1-b1)*g; v = b2*v + (1-b2)*g*g;
 * p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps), bc1 = 1-b1^t, bc2 = 1-b2^t, t = steps+1.
 * hyper: 7 fp32 in DEVICE memory {lr, beta1, beta2, eps, completed steps, grad_scale, weight_decay}; the call
 * increments hyper[4].  Device-resident so a captured hipGraph replays with current values;
 * grad_scale multiplies g first (1/world_size after a sum all-reduce).
 * With beta1 == 0 and weight_decay == 0 (the reference's TTUR default) m_t = g_t*grad_scale whatever m was: the kernel then neither
 * reads nor writes m (same bits in p and v, 20 instead of 28 bytes per parameter); a caller that saves m forms it from g. */
int s2e_adam_flat(float* p, const float* g, float* m, float* v, long n, float* hyper, void* stream);
/* The same step with an exponential moving average of the parameters kept in a fifth arena (an extension: the reference keeps
 * none).  p, v and m get exactly the bits s2e_adam_flat gives them from the same inputs -- both branches, vector body and scalar
 * tail -- and hyper is used and ticked in the same way.  ema_hyper: 2 fp32 in DEVICE memory {decay, start_step}, read by the launch
 * (graph-capturable; a changed decay or a resumed step count needs no host branch).  With t = hyper[4] + 1, the step this launch
 * performs:  t <= start_step: ema = p_new (ema is not read);  otherwise ema = decay * ema + (1 - decay) * p_new, in fp32, in that
 * written form.  8 more bytes per parameter than s2e_adam_flat (28 at beta1 == 0 and weight_decay == 0, else 36) and no launch of
 * its own.  ema must be 16-byte aligned like the other arenas and must not overlap them; S2E_ERR_ARG on a null pointer, a
 * misaligned arena or n <= 0, before any launch. */
int s2e_adam_flat_ema(float* p, const float* g, float* m, float* v, float* ema, long n, float* hyper, const float* ema_hyper,
                      void* stream);
/* The gradient guard (an extension: the reference has none): skip a step whose gradient holds a non-finite element, clip by the
 * global norm, report both -- without a host round trip.  s2e_grad_guard examines the gradient arena g[0..n) and writes the guard
 * record; the guarded steps below read one word of it.
 *   guard: 8 fp32 in DEVICE memory, first_bad: one int32 in DEVICE memory.
 *     guard[0] in   max_norm; <= 0: no clipping
 *     guard[1] in   skip_nonfinite, 0 or 1
 *     guard[2] out  norm = |hyper[5]| * sqrt(sum g_i^2) over the FINITE elements: the norm of the gradient Adam would consume (hyper[5]
 *                   = grad_scale); squares and sum in fp64, rounded to fp32 once
 *     guard[3] out  the coefficient c this step applies:
 *                     0    a skipped step: skip_nonfinite != 0 and a non-finite element exists;
 *                     NaN  a non-finite element exists and skip_nonfinite == 0 (the step poisons the parameters, as an unguarded one);
 *                     min(1, max_norm / (norm + 1e-6))  otherwise when max_norm > 0, in fp64 from the fp64 norm, rounded once
 *                          (torch.nn.utils.clip_grad_norm_ with norm_type = 2);
 *                     1    otherwise
 *     guard[4] out  steps skipped so far             guard[5] out  steps clipped (c < 1) so far
 *     guard[6] out  consecutive skipped steps; 0 after a step that ran         guard[7] reserved, written as 0
 *     first_bad out the smallest i with !(|g[i]| <= FLT_MAX) -- an element test, never inferred from the sum --, or -1
 *   The counters accumulate in the record: the caller zeroes it once.  Two launches, no atomics: per-block {fp64 sum, first index}
 *   records in `workspace` (s2e_grad_guard_workspace_bytes(n) bytes, 8-byte aligned, owned by the caller), combined in a fixed order by
 *   a one-block launch -- the same arena gives the same bits.  Reads g once (4 bytes per element).
 * s2e_adam_flat_guarded / s2e_adam_flat_ema_guarded: s2e_adam_flat / s2e_adam_flat_ema with grad_scale = hyper[5] * guard[3] (one fp32
 * multiply; c == 1 gives the unguarded bits).  With guard[3] == 0 the launch returns before it touches p, m, v or ema and hyper[4] is
 * NOT incremented: a skipped step is not a step.
 * All four: S2E_ERR_ARG (s2e_grad_guard_workspace_bytes: 0) on a null pointer, a misaligned arena, n <= 0 (s2e_grad_guard: also
 * n >= 2^31 - 1) or a workspace that is too small, before any launch. */
size_t s2e_grad_guard_workspace_bytes(long n);
int s2e_grad_guard(const float* g, long n, const float* hyper, float* guard, int* first_bad, void* workspace,
                   size_t workspace_bytes, void* stream);
int s2e_adam_flat_guarded(float* p, const float* g, float* m, float* v, long n, float* hyper, const float* guard, void* stream);
int s2e_adam_flat_ema_guarded(float* p, const float* g, float* m, float* v, float* ema, long n, float* hyper,
                              const float* ema_hyper, const float* guard, void* stream);

/* ------------------------------------------------------------------ data-parallel gradient exchange (new: the reference is single-GPU;
 * its only multi-GPU hook is the nn.DataParallel wrap of models/networks/__init__.py:46-47)
 * The 'direct' exchange of seg2eye_amd/distributed.py (all-to-all of the bucket shards, owner sum, all-gather): the owner's sum of the
 * `world` copies of its shard -- recv[r][i], r in rank order, fp32 accumulation, one rounding to dtype -- as ONE launch (round 5 did
 * it with view().sum() and three staging copies).  shard * sizeof(dtype) must be a multiple of 16. */
int s2e_shard_sum(int dtype, const void* recv, void* out, int world, long shard, void* stream);

/* ------------------------------------------------------------------ OpenEDS validation metric
 * What the reference's Tester and its --lambda_openeds loss compute on the host (util/tester.py:44-47,93-97;
 * data/postprocessor.py:58-73,92-107; models/networks/loss.py:102-155), as device passes:
 *   to255(x) = (int)(((x + 1) * 255) / 2)   -- fp32, truncation toward zero ([-1,1] -> 0..255)
 *   s2e_openeds_error   : err[n] = sqrt(sum_pixels (to255(fake) - to255(target))^2) / (H*W)   (calculate_mse_for_tensors)
 *   s2e_openeds_error_u8: the same on images that already are 0..255                         (calculate_mse_for_images)
 *   s2e_resize_to255    : bilinear resize of (N,H,W) single-channel images to (N,Ho,Wo) by OpenCV's INTER_LINEAR rule for the
 *                         float64 image the reference hands it (data/postprocessor.py:108-114: half-pixel centres, edge clamp,
 *                         float32 tap weights, float64 horizontal-then-vertical sums), then ((v+1)*255)/2 in float64 and the
 *                         truncation -> uint8                                                  (to_255resized_imagebatch)
 * The squared-difference sums are exact 64-bit integers; err: fp32 [N]. */
int s2e_openeds_error(int dtype, const void* fake, const void* target, int N, int H, int W, float* err, void* stream);
int s2e_openeds_error_u8(const uint8_t* produced, const uint8_t* target, int N, int H, int W, float* err, void* stream);
int s2e_resize_to255(int dtype, const void* x, int N, int H, int W, uint8_t* out, int Ho, int Wo, void* stream);

/* ------------------------------------------------------------------ structural similarity (an extension: the reference has none)
 * SSIM (Wang et al. 2004) of two single-channel batches x, y (N,H,W) and its gradient with respect to x.  u = (x + 1) / 2 and
 * v = (y + 1) / 2 for images of T in [-1, 1] (no clamp), u = a / 255 for the uint8 entry.  Window: 11 taps exp(-(i-5)^2 / (2 1.5^2))
 * normalised to sum 1 in fp64, as the outer product; "valid" placement only, (H-10)(W-10) positions.  With the window-weighted
 * means mu_u, mu_v, E[u^2], E[v^2], E[uv] of a position, su2 = E[u^2] - mu_u^2, sv2 likewise, suv = E[uv] - mu_u mu_v and
 *   S = (2 mu_u mu_v + C1)(2 suv + C2) / ((mu_u^2 + mu_v^2 + C1)(su2 + sv2 + C2)),   C1 = 0.01^2, C2 = 0.03^2 (data range 1),
 * ssim[n] (fp32) = the mean of S over image n's positions.  fp32 arithmetic from the loaded values, the moments taken about each
 * tile's first pixel; the sum toward ssim[n] in fp64: per-tile partials in `workspace` (plain stores), folded in index order by a
 * second launch.  maps (may be NULL: nothing is saved): 3 N (H-10)(W-10) fp32 -- the planes A = dS/dmu_u, B = dS/dE[u^2],
 * C = dS/dE[uv], each (N,H-10,W-10) -- for s2e_ssim_bwd:
 *   dx[n,p] (of T) = gssim[n] / positions * 1/2 * sum_q g(x)g(p - q) (A(q) + 2 u(p) B(q) + v(p) C(q)),    q over the positions covering p.
 * Two launches forward, one backward; no atomics, no synchronisation, launch shapes from (N, H, W) alone, bit-reproducible.
 * workspace: s2e_ssim_workspace_bytes(N, H, W) bytes (0 for N <= 0 or an image below 11 x 11), uninitialised.
 * Before any launch: S2E_ERR_ARG on a null pointer (maps of s2e_ssim_fwd excepted), N <= 0, a bad dtype or a short workspace;
 * S2E_ERR_UNSUPPORTED on H < 11, W < 11, N > 65535 or N H W >= 2^31. */
size_t s2e_ssim_workspace_bytes(int N, int H, int W);
int s2e_ssim_fwd(int dtype, const void* x, const void* y, int N, int H, int W, float* ssim, float* maps, void* workspace,
                 size_t workspace_bytes, void* stream);
int s2e_ssim_u8(const uint8_t* a, const uint8_t* b, int N, int H, int W, float* ssim, void* workspace, size_t workspace_bytes, void* stream);
int s2e_ssim_bwd(int dtype, const void* x, const void* y, const float* maps, const float* gssim, int N, int H, int W, void* dx, void* stream);

/* ------------------------------------------------------------------ multi-scale structural similarity (an extension: the reference has none)
 * MS-SSIM (Wang, Simoncelli, Bovik 2003) of two single-channel batches x, y (N,H,W) and its gradient with respect to x, on the window,
 * the placement, the units and the constants of s2e_ssim_*.  levels L in 1..5.  Level 0 is the image; level j + 1 is the 2 x 2 mean,
 * stride 2, of level j, a trailing odd row or column dropped: H_j = H >> j, W_j = W >> j, P_j = (H_j - 10)(W_j - 10) positions.  Legal
 * sizes have H >> (L-1) >= 11 and W >> (L-1) >= 11.  For image n:
 *   m_j[n] = the mean over level j's positions of cs = (2 suv + C2) / (su2 + sv2 + C2) for j < L-1, of the full S for j = L-1,
 *   msssim[n] (fp32) = prod_j max(m_j[n], F)^weights[j],   F = 1e-3 (a level at or below the floor counts as F and passes no gradient).
 * weights: a HOST array of L positive finite floats (they travel by value); the published five are 0.0448, 0.2856, 0.3001, 0.2363, 0.1333.
 * terms (N,L) fp32 = m_j[n] before the clamp; coef (N,L) fp32 = d msssim[n] / d m_j[n] = weights[j] msssim[n] / m_j[n], 0 where m_j[n] < F.
 * Forward, three launches (two when L = 1): the pyramid (levels 1..L-1 of both images, fp32 in the input's own units, into `pyramid`);
 * the moment passes of the tiles of all levels (one fp64 partial per tile into `workspace`; when maps is not NULL the planes A, B, C of
 * every level, level j's three (N,H_j-10,W_j-10) planes after those of the levels before it); the fold, per image, each level's partials
 * in index order.  s2e_msssim_bwd, two launches (one when L = 1): g_j = gout[n] coef[n][j] / P_j * (s2e_ssim_bwd's three correlations on
 * level j's maps) for the levels 1..L-1 into gbuf (fp32, (N,H_j,W_j) per level), then
 *   dx[n,p] (of T) = 1/2 sum_j 4^-j g_j(p >> j),    over the levels whose field holds p >> j.
 * No atomics, no synchronisation, launch shapes from (N, H, W, levels) alone, bit-reproducible.
 * Sizes: s2e_msssim_workspace_bytes, s2e_msssim_pyramid_bytes (0 when L = 1: pyramid and gbuf may then be NULL) and s2e_msssim_maps_bytes;
 * each is 0 for N <= 0, levels outside 1..5 or an illegal size.  gbuf needs half of s2e_msssim_pyramid_bytes.  All uninitialised.
 * Before any launch: S2E_ERR_ARG on a null pointer (maps of s2e_msssim_fwd excepted), N <= 0, a bad dtype, levels outside 1..5, a weight
 * that is not positive and finite, a short buffer; S2E_ERR_UNSUPPORTED on a last level below 11 x 11, N > 65535 or N H W >= 2^31. */
size_t s2e_msssim_workspace_bytes(int N, int H, int W, int levels);
size_t s2e_msssim_pyramid_bytes(int N, int H, int W, int levels);
size_t s2e_msssim_maps_bytes(int N, int H, int W, int levels);
int s2e_msssim_fwd(int dtype, const void* x, const void* y, int N, int H, int W, int levels, const float* weights, float* msssim,
                   float* terms, float* coef, float* maps, size_t maps_bytes, void* pyramid, size_t pyramid_bytes, void* workspace,
                   size_t workspace_bytes, void* stream);
int s2e_msssim_u8(const uint8_t* a, const uint8_t* b, int N, int H, int W, int levels, const float* weights, float* msssim, float* terms,
                  void* pyramid, size_t pyramid_bytes, void* workspace, size_t workspace_bytes, void* stream);
int s2e_msssim_bwd(int dtype, const void* x, const void* y, const void* pyramid, const float* maps, const float* coef, const float* gout,
                   int N, int H, int W, int levels, void* gbuf, size_t gbuf_bytes, void* dx, void* stream);

/* ------------------------------------------------------------------ focal frequency loss (an extension: the reference has none)
 * The focal frequency loss (Jiang, Dai, Wu, Loy, ICCV 2021) of two single-channel batches x, y (N,H,W) and its gradient with respect to
 * x: whole image, per image, no log, the per-image maximum (the paper's patch_factor, ave_spectrum, log_matrix and batch_matrix variants
 * are not built).  Values in the tensor's own units, no clamp; u = a / 255 for the uint8 entry.  For image n:
 *   1. d = x - y, formed in fp32 from the loaded values (the DFT is linear: only d is transformed).
 *   2. Z[ky,kx] = (H W)^-1/2 sum_{r,c} d[r,c] exp(-2 pi i (ky r / H + kx c / W)): the orthonormal 2-D DFT, H W complex bins.
 *   3. dist = Re Z^2 + Im Z^2.
 *   4. the focal weight w = dist^(alpha/2) / max over the image's H W bins of dist^(alpha/2): a constant of the step, no gradient flows
 *      through it.  alpha in [0, 4].  alpha = 0: w = 1 everywhere, bins with dist = 0 included; alpha > 0: a bin with dist = 0 has w = 0;
 *      an image whose maximum is 0 (x == y) has w = 0 everywhere.
 *   5. ffl[n] (fp32) = 1 / (H W) sum_bins w dist, the sum in fp64.
 *   6. dx[n] (of T) = gout[n] 2 / (H W) Re(inverse orthonormal 2-D DFT of w Z).  y gets none.
 * So ffl[n] = mean((x - y)^2) at alpha = 0 (Parseval), ffl and dx are exactly 0 for x == y, and ffl is symmetric in x and y.
 * The kernels carry only the Wh = W/2 + 1 non-redundant columns of the Hermitian spectrum, with multiplicity 1 for kx = 0 and for
 * kx = W/2 when W is even, 2 otherwise, forward and backward; the maximum over the half is the maximum over the whole.
 * Each transform is a dense real matrix product on the exact-fp32 matrix instruction (v_mfma_f32_16x16x4_f32) with the DFT matrices
 * cos, sin (2 pi (k j mod n) / n) n^-1/2, n = H and n = W, which s2e_ffl_tables fills on the device (one launch): the argument reduced in
 * integers, evaluated in fp64, rounded once to fp32, zero-padded to the tile size.  The tables depend on (H, W) only.
 * s2e_ffl_fwd, three launches: the row transform of d; the column transform, the 2H x 2H block matrix [C -S; S C], whose epilogue keeps
 * Z in `spectrum` when that is not NULL and writes one fp64 partial sum of m dist^(1 + alpha/2) and one fp32 partial maximum of dist per
 * block into `workspace` (plain stores); the per-image fold in index order: ffl[n] = sum / (H W max^(alpha/2)) and the backward's
 * coef[n] = 2 / (H W max^(alpha/2)), both 0 when max = 0.  s2e_ffl_bwd, two launches: the column inverse transform of
 * coef[n] gout[n] dist^(alpha/2) Z (dist recomputed from Z), then the row inverse transform with the multiplicities, which writes dx.
 * alpha = 0, 1, 2 take 1, sqrt and the identity for dist^(alpha/2), any other alpha exp2(alpha/2 log2 dist).
 * No atomics, no synchronisation, launch shapes from (N, H, W) alone, bit-reproducible.
 * Sizes: s2e_ffl_tables_bytes(H, W), s2e_ffl_workspace_bytes(N, H, W) (forward and backward take the same) and
 * s2e_ffl_spectrum_bytes(N, H, W); each is 0 where the call would be illegal.  workspace and spectrum are uninitialised.
 * Before any launch: S2E_ERR_ARG on a null pointer (the spectrum of s2e_ffl_fwd excepted), N <= 0, a bad dtype, alpha negative,
 * non-finite or above 4; S2E_ERR_UNSUPPORTED on H < 2 or W < 2, H or W above 1024, N > 65535 or N H W >= 2^31; S2E_ERR_ARG on a short
 * buffer. */
size_t s2e_ffl_tables_bytes(int H, int W);
size_t s2e_ffl_workspace_bytes(int N, int H, int W);
size_t s2e_ffl_spectrum_bytes(int N, int H, int W);
int s2e_ffl_tables(int H, int W, float* tables, size_t tables_bytes, void* stream);
int s2e_ffl_fwd(int dtype, const void* x, const void* y, int N, int H, int W, float alpha, const float* tables, size_t tables_bytes,
                float* ffl, float* coef, float* spectrum, size_t spectrum_bytes, void* workspace, size_t workspace_bytes, void* stream);
int s2e_ffl_u8(const uint8_t* a, const uint8_t* b, int N, int H, int W, float alpha, const float* tables, size_t tables_bytes, float* ffl,
               void* workspace, size_t workspace_bytes, void* stream);
int s2e_ffl_bwd(int dtype, const float* spectrum, const float* coef, const float* gout, int N, int H, int W, float alpha,
                const float* tables, size_t tables_bytes, void* workspace, size_t workspace_bytes, void* dx, void* stream);

/* ------------------------------------------------------------------ region-aware reconstruction error (an extension: the reference has none)
 * Statistics of d = x - y per image and label class, the class-balanced loss built from them, and its gradient with respect to x.
 * x, y: single-channel batches (N,H,W) of T in [-1, 1] (or uint8 0..255 for s2e_region_stats_u8); label: uint8 (N,Hl,Wl); ncls in 1..8.
 * Pixel (n, r, c) has class l = label[n, (r Hl) / H, (c Wl) / W] (integer division); a pixel with l >= ncls belongs to no region: it
 * enters no count and no sum and gets a zero gradient (a label is compared, never used as an index).
 *   stats[n][c][3] (fp64) = {count, sum |d|, sum d^2} over image n's pixels of class c.  d, |d|, d^2 are fp32 from the loaded values,
 *   every sum over pixels is fp64; for uint8 images all three numbers are exact.
 *   With f = |d| (norm S2E_REGION_L1) or d^2 (S2E_REGION_L2), n_c = sum_n count[n][c], and the classes with n_c > 0 called present:
 *   loss[0] (fp32) = sum_present w_c (sum_n sum f [n][c] / n_c) / sum_present w_c,   coef[c] (fp32) = w_c / (n_c sum_present w) for a
 *   present class, else 0;  loss = 0 and coef = 0 when no class of positive weight is present.  weights: ncls fp32, >= 0, on the device.
 *   s2e_region_loss_bwd:  dx[p] (of T) = gloss[0] coef[l(p)] f'(d(p)),  f' = sign(d) (0 at d == 0, NaN for a NaN d) or 2 d.
 * A NaN or inf difference puts NaN or inf into its class's sums, the loss and that pixel's gradient; nothing is special-cased.
 * Forward: two launches (per-block, per-class partial records in `workspace`, plain stores; one fold in index order); backward: one.
 * No atomics, no synchronisation, launch shapes from (N, H, W, Hl, Wl, ncls) alone, bit-reproducible.
 * workspace: s2e_region_workspace_bytes(N, H, W, ncls) bytes (0 for N <= 0, H < 1, W < 1 or ncls outside 1..8), uninitialised.
 * Before any launch, in this order: S2E_ERR_ARG on a null pointer or N <= 0, then a bad dtype, then a bad norm; S2E_ERR_UNSUPPORTED
 * on ncls outside 1..8, then H, W, Hl or Wl < 1, then N > 65535, H W > 2^24 or N H W >= 2^31; S2E_ERR_ARG on a short workspace. */
enum { S2E_REGION_L1 = 0, S2E_REGION_L2 = 1 };
size_t s2e_region_workspace_bytes(int N, int H, int W, int ncls);
int s2e_region_loss_fwd(int dtype, const void* x, const void* y, const uint8_t* label, int N, int H, int W, int Hl, int Wl, int ncls,
                        int norm, const float* weights, double* stats, float* loss, float* coef, void* workspace,
                        size_t workspace_bytes, void* stream);
int s2e_region_stats_u8(const uint8_t* a, const uint8_t* b, const uint8_t* label, int N, int H, int W, int Hl, int Wl, int ncls,
                        double* stats, void* workspace, size_t workspace_bytes, void* stream);
int s2e_region_loss_bwd(int dtype, const void* x, const void* y, const uint8_t* label, const float* coef, const float* gloss,
                        int N, int H, int W, int Hl, int Wl, int ncls, int norm, void* dx, void* stream);

/* ------------------------------------------------------------------ style reference rankings
 * The reference's --style_ref file ranks, for every target mask, a person's style frames "by their L2 distance to the target
 * segmentation mask" (refinenet/README.md); it ships no program that does so.  Two integer entry points, exact and run-to-run identical.
 *   s2e_mask_dist: a (M, pitch) and b (K, pitch) uint8 are rows of label maps of P <= pitch bytes; bytes P .. pitch-1 of a row may
 *       hold anything and influence nothing.  dist (M, K) int32 is OVERWRITTEN with
 *         S2E_RANK_L2        sum_p (a[m][p] - b[k][p])^2           (as sum a^2 + sum b^2 - 2 sum a b, the product on v_mfma_i32_16x16x64_i8)
 *         S2E_RANK_MISMATCH  #{p : a[m][p] != b[k][p]}             (as P - sum_c sum_p [a = c][b = c], c < ncls)
 *       Two launches: dist is zeroed, then one kernel whose workgroups split the pixel axis and add their partial tiles with
 *       int32 atomicAdd (associative: any order gives the same bits).  A byte >= ncls (>= 128 for l2) in the data gives an unspecified
 *       distance; nothing is read or written out of bounds.
 *       Before any launch, in this order: S2E_ERR_ARG on a null pointer, an unknown metric, M, K or P < 1, pitch < P, then a, b or
 *       pitch not a multiple of 16 bytes (dist: of 4); S2E_ERR_UNSUPPORTED on ncls outside 1..128 (l2) or 1..16 (mismatch), then
 *       (ncls-1)^2 P > 2^31 - 1 or P > 2^31 - 1, then M or K above 65535 * 64.
 *   s2e_rank_topk: for every row of dist (M, K) int32 the min(k, K') candidates of smallest (distance, index) -- distance ascending,
 *       ties to the lower index: one total order -- into idx (M, k) and val (M, k) int32; unused slots hold -1.  exclude: NULL, or (M,)
 *       int32 naming one candidate per row that is not returned (a value outside 0..K-1 names none); K' counts the rest.  One launch,
 *       one workgroup per row, the keys sorted in LDS: K <= s2e_rank_topk_max_candidates() (above it: rank chunks, then the winners).
 *       S2E_ERR_ARG on a null dist, idx or val, then M, K or k < 1; S2E_ERR_UNSUPPORTED on K above the limit. */
enum { S2E_RANK_L2 = 0, S2E_RANK_MISMATCH = 1 };
int s2e_mask_dist(const uint8_t* a, const uint8_t* b, int M, int K, long P, long pitch, int ncls, int metric, int32_t* dist, void* stream);
int s2e_rank_topk_max_candidates(void);
int s2e_rank_topk(const int32_t* dist, int M, int K, int k, const int32_t* exclude, int32_t* idx, int32_t* val, void* stream);

/* ------------------------------------------------------------------ eye segmenter: loss, mask, confusion matrix
 * The masks `style_rank --seg_file` reads come from a small encoder-decoder built on the convolutions above (networks/segmenter.py);
 * these are its three memory-bound pieces.  logits: (N, H, W, C) NHWC of dtype, channel pitch C >= ncls, 1 <= ncls <= 16; channels at
 * and past ncls may hold anything (NaN included) and influence nothing.  label: (N, H, W) uint8; a value >= ncls (255 is the documented
 * "ignore") marks a pixel that is not counted and is never used as an index.  No float atomics: the same input gives the same bits.
 *   s2e_seg_ce_fwd: loss[0] = sum_p w[l_p] (lse_p - z_{p,l_p}) / sum_p w[l_p] over the counted pixels, lse in fp32 with the maximum
 *       subtracted -- F.cross_entropy(weight=w, ignore_index=..., reduction='mean') -- and denom[0] = sum_p w[l_p] for the backward;
 *       a denominator of 0 gives loss 0.  weights: fp32 (ncls).  Two launches: per-workgroup fp64 partials into `workspace`
 *       (s2e_seg_ce_workspace_bytes(N, H, W) bytes, 8-byte aligned), then one fold in index order.
 *   s2e_seg_ce_bwd: dlogits[p][c] = gloss[0] w[l_p] (softmax_c(z_p) - [c == l_p]) / denom[0] in dtype, the softmax recomputed; +0 for
 *       ignored pixels, for channels >= ncls, and everywhere when denom[0] is 0.  gloss, denom: one fp32 each, on the device.  One launch.
 *   s2e_seg_argmax_u8: mask (N, Ho, Wo) uint8 = argmax_c of the ncls logits resized bilinearly in fp32 by the rule of
 *       s2e_bilinear_resize_fwd (F.interpolate(mode='bilinear', align_corners=False): source coordinate (d + 0.5) in / out - 0.5,
 *       clamped at 0); a tie goes to the lowest class; (Ho, Wo) == (h, w) is the plain argmax.  One launch, the resized logits are
 *       never stored.
 *   s2e_seg_confusion_u8: conf (ncls x ncls) int64, row = truth, column = pred, += the counts of the P pixel pairs; the caller zeroes
 *       it before the first call.  A pair with either value >= ncls is skipped.  One launch: LDS counts per workgroup, then one 64-bit
 *       integer atomic per non-zero cell.
 * Before any launch, in this order: S2E_ERR_ARG on a null pointer (conf also: not 8-byte aligned), an unknown dtype, N, H, W (P) < 1;
 * S2E_ERR_UNSUPPORTED on ncls outside 1..16; S2E_ERR_ARG on C < ncls; S2E_ERR_UNSUPPORTED on N H W > 2^31 - 1 (P > 2^31 - 1 per
 * call: accumulate more with further calls); then s2e_seg_ce_fwd: S2E_ERR_ARG on a missing, short or misaligned workspace;
 * s2e_seg_argmax_u8: S2E_ERR_ARG on Ho or Wo < 1, S2E_ERR_UNSUPPORTED on N Ho Wo > 2^31 - 1, N or Ho > 65535. */
size_t s2e_seg_ce_workspace_bytes(int N, int H, int W);
int s2e_seg_ce_fwd(int dtype, const void* logits, const uint8_t* label, const float* weights, int N, int H, int W, int C, int ncls,
                   float* loss, float* denom, void* workspace, size_t workspace_bytes, void* stream);
int s2e_seg_ce_bwd(int dtype, const void* logits, const uint8_t* label, const float* weights, const float* denom, const float* gloss,
                   int N, int H, int W, int C, int ncls, void* dlogits, void* stream);
int s2e_seg_argmax_u8(int dtype, const void* logits, int N, int h, int w, int C, int ncls, int Ho, int Wo, uint8_t* mask, void* stream);
int s2e_seg_confusion_u8(const uint8_t* pred, const uint8_t* truth, long P, int ncls, int64_t* conf, void* stream);

/* ------------------------------------------------------------------ eye segmenter: distance maps and the boundary-aware loss
 * logits, label and ncls as in the section above.  Everything is per image: distances never cross images and the frame edge is no
 * boundary.  No atomics: the same input gives the same bits.
 *   s2e_seg_dist_maps: for pixel p and class c let m be the smallest squared integer distance |p - q|^2 to a pixel q with l_q != c
 *       when l_p == c (a label >= ncls is "not c" for every c), to a pixel q with l_q == c otherwise.  phi (N, H, W, ncls) fp32 =
 *       1 - sqrtf(m) when l_p == c (+0 where the pixel touches another class), +sqrtf(m) otherwise, +0 for a class that is absent from
 *       the image or fills it (Kervadec's one_hot2dist).  band (N, H, W) uint8, or NULL = 1 where l_p < ncls, the complement of its
 *       class is not empty and its m <= radius^2 (decided on the integers), else 0.  Two launches: a column pass writes the vertical
 *       distances as uint16 pairs into `workspace` (s2e_seg_dist_workspace_bytes(N, H, W, ncls) bytes, 4-byte aligned), a row pass
 *       takes the minimum over the row.  rint(sqrtf(m)^2) == m over the whole supported range.
 *       Before any launch, in this order: S2E_ERR_ARG on a null label, phi or workspace, a short or misaligned workspace (a shape
 *       refused below needs 0 bytes), N, H or W < 1, radius < 0; S2E_ERR_UNSUPPORTED on ncls outside 1..16, H or W > 1024 (the uint16
 *       distances and the exact-sqrt range), N > 65535 or N H W >= 2^31, N H W ncls >= 2^31.
 *   s2e_seg_loss_fwd: with P the counted pixels, p the softmax over the first ncls channels (fp32, maximum subtracted), g the one-hot
 *       of the label on P, b_p = 1 + edge_alpha band_p:
 *         terms[0] CE      = sum_P w[l_p] b_p (lse_p - z_{p,l_p}) / sum_P w[l_p]                (0 when the denominator is 0)
 *         terms[1] Dice    = mean over the images n with a counted pixel of 1 - 2 sum_c v I / sum_c v U, I_nc = sum p g,
 *                            U_nc = sum (p + g), v_nc = 1 / G_nc^2 where G_nc = sum g > 0, else 0    (0 when there is no such image)
 *         terms[2] Surface = sum_P sum_c p_{p,c} phi_{p,c} / (|P| ncls)                          (0 when lambda_surf is 0)
 *         loss[0] = lambda_ce CE + lambda_dice Dice + lambda_surf Surface
 *       phi may be NULL when lambda_surf is 0 and band when edge_alpha is 0; a term that is off reads nothing, so the call gives the
 *       same bits with and without its input.  saved (N 2 ncls + 2 floats) takes, for the backward, per image and class
 *       kI = -(lambda_dice / N_cnt) 2 v / D_n and kU = (lambda_dice / N_cnt) 2 A_n v / D_n^2 (A_n = sum_c v I, D_n = sum_c v U) at
 *       saved[(n 2 + 0) ncls + c] and saved[(n 2 + 1) ncls + c], then 1 / sum_P w and 1 / (|P| ncls) (0 where the sum is 0).  Two
 *       launches: grid.y = image, per-workgroup fp64 partials with plain stores into `workspace`
 *       (s2e_seg_loss_workspace_bytes(N, H, W, ncls) bytes, 8-byte aligned), then one fold in index order.
 *   s2e_seg_loss_bwd: with a_{p,c} = kI_nc [c == l_p] + kU_nc + lambda_surf saved_s phi_{p,c}:
 *         dlogits[p][c] = gloss[0] (p_c (a_c - sum_k a_k p_k) + lambda_ce w[l_p] b_p (p_c - [c == l_p]) / sum w)
 *       in dtype, the softmax recomputed; +0 for ignored pixels and for channels >= ncls.  One launch.
 *       Both, before any launch, in this order: S2E_ERR_ARG on a null pointer other than phi and band, an unknown dtype, N, H, W < 1;
 *       S2E_ERR_UNSUPPORTED on ncls outside 1..16; S2E_ERR_ARG on C < ncls; S2E_ERR_UNSUPPORTED on N H W > 2^31 - 1, N > 65535;
 *       S2E_ERR_ARG on a negative or non-finite lambda or edge_alpha, on lambda_surf != 0 without phi, on edge_alpha != 0 without
 *       band; then s2e_seg_loss_fwd: S2E_ERR_ARG on a missing, short or misaligned workspace. */
size_t s2e_seg_dist_workspace_bytes(int N, int H, int W, int ncls);
int s2e_seg_dist_maps(const uint8_t* label, int N, int H, int W, int ncls, int radius, float* phi, uint8_t* band, void* workspace,
                      size_t workspace_bytes, void* stream);
size_t s2e_seg_loss_workspace_bytes(int N, int H, int W, int ncls);
int s2e_seg_loss_fwd(int dtype, const void* logits, const uint8_t* label, const float* weights, const float* phi, const uint8_t* band,
                     int N, int H, int W, int C, int ncls, float lambda_ce, float lambda_dice, float lambda_surf, float edge_alpha,
                     float* loss, float* terms, float* saved, void* workspace, size_t workspace_bytes, void* stream);
int s2e_seg_loss_bwd(int dtype, const void* logits, const uint8_t* label, const float* weights, const float* phi, const uint8_t* band,
                     const float* saved, const float* gloss, int N, int H, int W, int C, int ncls, float lambda_ce, float lambda_surf,
                     float edge_alpha, void* dlogits, void* stream);

/* ------------------------------------------------------------------ mask cleaner: connected components, nearest-class fill
 * labels: (N, H, W) uint8, 1 <= ncls <= 16, conn 4 or 8.  Everything is per image: nothing crosses images and the frame edge joins
 * nothing.  The rule:
 *   components  pixels of one label c < ncls that are conn-adjacent form a component; a pixel with a label >= ncls (255 is the
 *       documented "ignore") belongs to none and is never used as an index.  A component's id is the smallest linear index y W + x
 *       among its pixels -- a property of the map, not of the algorithm.
 *   kept        modes[c]: 0 (all) every component of class c is kept; 1 (largest) only the one of largest area, among equal areas
 *       the one with the smallest id; 2 (border) those that hold a pixel of the image's first or last row or column.
 *   fill        every pixel that is not kept -- of a removed component or with a label >= ncls -- becomes argmin over c of (d^2_c, c),
 *       compared lexicographically, d^2_c the smallest squared integer distance to a kept pixel of class c, over the classes that
 *       keep a pixel in this image: a tie goes to the lower class.  Kept pixels do not change; an image that keeps no pixel comes
 *       back unchanged.
 *   stats       (N, ncls, 4) int32, or NULL: per image and class the components found, the pixels before, the pixels removed, the
 *       pixels after (before - removed + filled in).
 *   s2e_mask_components: comp (N, H, W) int32 = the id of the pixel's component, -1 for a label >= ncls.  Three launches on `comp`
 *       itself: union-find per 32 x 32 tile in LDS, a min-union along the tile borders, a flatten; one tile per image skips the second.
 *   s2e_mask_clean: out (N, H, W) uint8.  Seven launches (six for one tile per image): those three, the per-class decision, the kept
 *       map, and the column and row pass of s2e_seg_dist_maps' scheme, the row pass only where a row has a pixel that is not kept.
 *       workspace: s2e_mask_clean_workspace_bytes(N, H, W, ncls) bytes, 8-byte aligned.  modes is a HOST pointer to ncls bytes, read
 *       before the first launch, so that a bad byte is refused here and not met by a kernel.
 * No workgroup waits for another; ids are minima, areas integer sums, the ties are ruled above: two calls give the same bytes.
 * Before any launch, in this order: S2E_ERR_ARG on a null labels, out, comp, modes or workspace, on a short workspace or one that is
 * not 8-byte aligned (a shape refused below needs 0 bytes), on N, H or W < 1, on conn other than 4 and 8; S2E_ERR_UNSUPPORTED on ncls
 * outside 1..16; S2E_ERR_ARG on a mode byte above 2; S2E_ERR_UNSUPPORTED on H or W > 1024 (the uint16 distances, as in
 * s2e_seg_dist_maps), on N > 65535 or N H W >= 2^31. */
size_t s2e_mask_clean_workspace_bytes(int N, int H, int W, int ncls);
int s2e_mask_components(const uint8_t* labels, int N, int H, int W, int ncls, int conn, int32_t* comp, void* stream);
int s2e_mask_clean(const uint8_t* labels, int N, int H, int W, int ncls, int conn, const uint8_t* modes, uint8_t* out, int32_t* stats,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ eye geometry: rim moments and the repaint from conics
 * labels: (N, H, W) uint8, 1 <= ncls <= 16, H and W at most 1024.  Everything is per image: nothing crosses images, and a pixel of the
 * frame's edge has no neighbour beyond it.  Every result is an integer or a copy.  The rules:
 *   curves      curve k, 0 <= k < K <= 4, is a pair of class sets (in_sets[k], out_sets[k]), bit c = class c.  Both arrays are HOST
 *       pointers to K uint16, read before the first launch, so that a bad set is refused here and not met by a kernel: a set must not
 *       be empty, the two must not overlap, and neither may name a class >= ncls.  For the OpenEDS classes (0 skin, 1 sclera, 2 iris,
 *       3 pupil) the limbus is in {2, 3} out {1} and the pupil's edge in {3} out {2}: where a lid covers the iris or the pupil there
 *       is no rim pixel.
 *   rim pixel   a pixel whose label l < ncls is in in_sets[k] and one of whose four neighbours inside the frame has a label l' < ncls
 *       in out_sets[k].  A label >= ncls (255 is the documented "ignore") is in no set and is never used as an index.
 *   s2e_rim_moments: rim (N, K, 18) int64, 8-byte aligned.  Over the rim pixels (x, y) of curve k in image n:
 *         rim[0] = n, their number;  rim[1] = ox = floor((2 sum x + n) / (2 n)),  rim[2] = oy likewise (0, 0 when n = 0);
 *         rim[3 + m] = sum (x - ox)^i (y - oy)^j for i + j <= 4, by degree and then by j:
 *           m = 0: (0,0)   1: (1,0)  2: (0,1)   3: (2,0)  4: (1,1)  5: (0,2)   6: (3,0)  7: (2,1)  8: (1,2)  9: (0,3)
 *               10: (4,0)  11: (3,1)  12: (2,2)  13: (1,3)  14: (0,4)
 *       With H, W <= 1024, |x - ox| <= 1023: a term is below 2^40 and a sum of at most 2^20 of them below 2^60.  The origin needs the
 *       whole image before a centred sum can start: three launches -- the first moments and the centred sums as per-workgroup integer
 *       partials with plain stores into `workspace` (s2e_rim_moments_workspace_bytes(N, H, W, K) bytes, 8-byte aligned), then one fold.
 *       No workgroup waits for another and no launch reads a line it writes.
 *   s2e_ellipse_paint: out (N, H, W) uint8, another buffer than labels.  conic (N, K, 6) double = (A, B, C, D, E, F) of curve k about
 *       origin (N, K, 2) int32 = (ox, oy); valid (N, K) uint8; all three on the device.  paint: a HOST pointer to K class bytes; keep:
 *       a class set (bit c = class c); base: a class.  An image with any valid byte 0 comes back unchanged.  Otherwise a pixel whose
 *       label is >= ncls or in keep is unchanged; every other pixel becomes base and then, for k ascending, paint[k] where Q_k <= 0,
 *         Q_k = ((((A u) u + (B u) v) + (C v) v) + D u) + E v) + F,   u = (double)(x - ox), v = (double)(y - oy),
 *       in fp64, every product and sum rounded once and none fused; a NaN compares false.  One launch, one lane per four pixels.
 * Before any launch, in this order: S2E_ERR_ARG on a null pointer, on a short workspace or a workspace, rim or conic that is not 8-byte
 * aligned (origin: 4-byte; a shape refused below needs 0 bytes), on N, H or W < 1; S2E_ERR_UNSUPPORTED on K outside 1..4, on ncls outside
 * 1..16; S2E_ERR_ARG on a curve whose sets are empty, overlap or name a class >= ncls, on paint[k] or base >= ncls;
 * S2E_ERR_UNSUPPORTED on H or W > 1024 (the int64 bound above), on N > 65535 or N H W >= 2^31. */
size_t s2e_rim_moments_workspace_bytes(int N, int H, int W, int K);
int s2e_rim_moments(const uint8_t* labels, int N, int H, int W, int ncls, int K, const uint16_t* in_sets, const uint16_t* out_sets,
                    int64_t* rim, void* workspace, size_t workspace_bytes, void* stream);
int s2e_ellipse_paint(const uint8_t* labels, int N, int H, int W, int ncls, int K, const double* conic, const int32_t* origin,
                      const uint8_t* valid, const uint8_t* paint, int keep, int base, uint8_t* out, void* stream);

/* ------------------------------------------------------------------ residual refiner: input, loss, gradient, submission bytes
 * The reference's last stage (refinenet/): the top-ranked frame of the same person plus a learned residual, clamped to [-1, 1].  These
 * are the four memory-bound pieces around the network.  tmask, rimg, rmask, truth: (N, H, W) uint8 planes as the store holds them.
 * flip: NULL (no flip) or N bytes, the convention of s2e_resize_bicubic_u8: flip[n] != 0 mirrors EVERY plane of image n horizontally --
 * the pixel (y, x) of x / res / dres / out reads the planes at (y, W - 1 - x).  A frame is normalised in fp32 with two roundings,
 *   norm(v) = fl(fl(v * fl(2 / 255)) - 1)      (refinenet/dataset.py:53-58 on a float32 array; never a fused multiply-add),
 * in registers: no fp32 copy of a frame exists in memory, and a bf16 network's residual is added to the frame's exact fp32 value.
 *   s2e_refine_input: x (N, H, W, C) NHWC of dtype, C >= 3: channel 0 = norm(levels[tmask]), 1 = norm(rimg), 2 = norm(levels[rmask]),
 *       channels 3 .. C - 1 = +0; bf16 is one round-to-nearest-even of the fp32 value.  levels: ncls uint8 grey levels on the device
 *       (the reference's class means as its uint8 array stores them: 125, 103, 76, 34); a label >= ncls takes level 0 and is never
 *       used as an index (the reference leaves such a pixel uninitialised).  One launch.
 *   s2e_refine_head_fwd: res (N, H, W, C) of dtype, C >= 1, channel 0 live (the others are never read).  Per pixel, in fp32,
 *       p = clamp(fl(res + norm(rimg)), -1, 1), d = fl(p - norm(truth)); per image, in fp64, sumsq[n] = sum d^2 and
 *       score[n] = 127.5 sqrt(sumsq[n]) / (H W)  (refinenet/model.py:52-57 per_image_score);
 *       terms = { eds_loss = mean_n score[n],  l1 = sum |d| / (N H W),  1471 eds_loss }.  Two launches: grid.y = image, per-workgroup
 *       fp64 partials with plain stores into `workspace` (s2e_refine_head_workspace_bytes(N, H, W) bytes, 8-byte aligned), then one
 *       fold in index order.  No atomics: the same input gives the same bits.
 *   s2e_refine_head_bwd: dres (N, H, W, C) of dtype; channel 0 =
 *         m gloss[0] (lambda_eds 127.5 d / (N H W sqrt(sumsq[n])) + lambda_l1 sign(d) / (N H W)),
 *       m = 1 where -1 <= fl(res + norm(rimg)) <= 1 (inclusive, as torch.clamp passes gradients), else 0; sign(0) = 0; the first term
 *       is 0 for an image whose sumsq[n] is 0 (torch gives NaN there); channels 1 .. C - 1 = +0.  sumsq: what the forward wrote;
 *       gloss: one fp32 on the device.  One launch, the prediction recomputed.
 *   s2e_refine_predict_u8: out (N, H, W) uint8 = (uint8)fl(127.5 fl(p + 1)), TRUNCATED (refinenet/evaluate_refinenet.py:105), so a zero
 *       residual gives back v - 1 for 47 of the 256 grey levels v.  One launch.
 * Before any launch, in this order: S2E_ERR_ARG on a null pointer other than flip (workspace, sumsq also: not 8-byte aligned), an
 * unknown dtype, N, H or W < 1, C below the minimum; S2E_ERR_UNSUPPORTED on H W > 2^30, N > 65535, N H W >= 2^31; then
 * s2e_refine_input: S2E_ERR_UNSUPPORTED on ncls outside 1..16; s2e_refine_head_fwd: S2E_ERR_ARG on a short workspace (a shape refused
 * above needs 0 bytes). */
int s2e_refine_input(int dtype, const uint8_t* tmask, const uint8_t* rimg, const uint8_t* rmask, const uint8_t* flip,
                     const uint8_t* levels, int ncls, int N, int H, int W, int C, void* x, void* stream);
size_t s2e_refine_head_workspace_bytes(int N, int H, int W);
int s2e_refine_head_fwd(int dtype, const void* res, int C, const uint8_t* rimg, const uint8_t* truth, const uint8_t* flip,
                        int N, int H, int W, float* score, double* sumsq, float* terms, void* workspace, size_t workspace_bytes,
                        void* stream);
int s2e_refine_head_bwd(int dtype, const void* res, int C, const uint8_t* rimg, const uint8_t* truth, const uint8_t* flip,
                        int N, int H, int W, const double* sumsq, const float* gloss, float lambda_eds, float lambda_l1,
                        void* dres, void* stream);
int s2e_refine_predict_u8(int dtype, const void* res, int C, const uint8_t* rimg, const uint8_t* flip, int N, int H, int W,
                          uint8_t* out, void* stream);

/* ------------------------------------------------------------------ side-by-side validation panels
 * The reference's visualize_sidebyside (util/visualizer.py:131-166) for a batch of n samples, as three launches on the caller's
 * stream with no host synchronisation between them: out[i] = [ style | label | target_original | fake | heat ], five h x w cells of
 * uint8 side by side.  With R = the cv2.INTER_LINEAR resize of s2e_resize_to255 (float64 image, float weights) and norm =
 * ImageProcessor.normalize over the WHOLE resized batch (min >= -1-1e-6 and max <= 1+1e-6: unchanged; else min >= 0: t / max * 2 - 1;
 * else a range error), every cell is norm(R(.)):
 *   style  (n, ns, H, W) fp32: the first min(ns, 4) images of a sample in make_grid(nrow=2, padding=0) order (1: the image, 2: one
 *          row, 3 / 4: 2 x 2, a missing cell 0), then the fp32 mean of three replicated channels, ((a + a) + a) / 3
 *   label  (n, H, W) uint8;  target_original (n, Ht, Wt) uint8;  fake (n, H, W) of fake_dtype (S2E_F32 or S2E_BF16)
 *   heat = |fk - tg| / max_batch |fk - tg| * 2 - 1 from the normalised fake and target cells; all -1 where that maximum is 0
 *   byte = clamp(trunc((v + 1) * 128), 0, 255).  All value arithmetic is float64, one rounding per operation, in the reference's order.
 * out: row y of panel i starts at out + i * panel_stride + y * row_stride (bytes; row_stride >= 5 w, any alignment), so the panels
 * may be the top rows of a larger buffer.  ws: s2e_sidebyside_ws_bytes(n, h, w) bytes, 8-byte aligned, holds the per-workgroup
 * min / max partials (no atomics; bitwise reproducible).  status: one int the last launch ALWAYS writes -- 0, or bit 0 style, bit 1
 * label, bit 2 target_original, bit 3 fake set where that tensor holds a NaN or fails normalize's range check (the panel bytes are
 * then unspecified; nothing is read or written out of bounds).
 * S2E_ERR_ARG (s2e_sidebyside_ws_bytes: -1) before any launch on a null pointer, a size <= 0, ns < 1, row_stride < 5 w, panels
 * that overlap, a misaligned ws or status. */
long s2e_sidebyside_ws_bytes(int n, int h, int w);
int s2e_sidebyside_u8(int fake_dtype, const void* fake, const float* style, int ns, const uint8_t* label,
                      const uint8_t* target_original, int n, int H, int W, int Ht, int Wt, int h, int w,
                      int row_stride, long panel_stride, void* ws, int* status, uint8_t* out, void* stream);

/* ------------------------------------------------------------------ device-side preprocessing of OpenEDS frames
 * What the dataset's transform does on the host (data/base_dataset.py:51-80, 'fixed' mode), bit for bit:
 *   s2e_resize_bicubic_u8: Pillow's Image.resize(BICUBIC) of M single-channel uint8 frames (M,H,W) -> (M,Ho,Wo), then the
 *       per-frame horizontal flip of the result (flip[m] != 0: out[y][x] = r[y][Wo-1-x]) and out = lut[r] (lut: 256 fp32 --
 *       ToTensor + Normalize evaluated by the caller for every byte value).  out_u8 (NULL = skip): the flipped uint8 frames.
 *       Pillow's rule is integer arithmetic: per axis, output index i sums `count` source pixels from `xmin` on,
 *       bounds[i] = {xmin, count}, times the fixed-point taps k[i][0..count) (2^22 = 1.0), and a pass stores
 *       clamp((2^21 + sum) >> 22, 0, 255); the horizontal pass runs first, the vertical pass on its uint8 result.  The caller
 *       builds the tables (seg2eye_amd/ops/preprocess.py: bicubic_coeffs): kx int32 [Wo][ksize(W,Wo)], bx int32 [Wo][2], ky int32
 *       [Ho][ksize(H,Ho)], by int32 [Ho][2], ksize(in,out) = 2*ceil(2*max(in/out,1)) + 1.  A pass whose size does not change is
 *       skipped and its two tables may be NULL.  Indices read from the tables are clamped to the frame.
 *       S2E_ERR_UNSUPPORTED when the source rows of ONE output row (ksize(H,Ho) rows of W + Wo bytes) exceed 64 KiB of LDS.
 *   s2e_resize_nearest_u8: out[m][y][x] = src[m][ys[y]][xs[x']], x' = flip[m] ? Wo-1-x : x -- cv2.INTER_NEAREST with the index
 *       tables ys int32 [Ho], xs int32 [Wo] built by the caller (src = min(int(dst * in / out), in - 1)).
 * Both: S2E_ERR_ARG on a NULL pointer or a size <= 0, before any launch. */
int s2e_resize_bicubic_u8(const uint8_t* src, const uint8_t* flip, int M, int H, int W, int Ho, int Wo,
                          const int32_t* kx, const int32_t* bx, const int32_t* ky, const int32_t* by, const float* lut,
                          float* out, uint8_t* out_u8, void* stream);
int s2e_resize_nearest_u8(const uint8_t* src, const uint8_t* flip, int M, int H, int W, int Ho, int Wo,
                          const int32_t* ys, const int32_t* xs, uint8_t* out, void* stream);

/* ------------------------------------------------------------------ paired augmentation of frames and label maps
 * One launch warps M pairs of uint8 planes (M, H, W) -- a frame and its label map -- by one affine transform per pair, draws line
 * occluders on the frame and sends the frame through a table.  Integers throughout (64-bit where a product may pass 32), so that a
 * numpy restatement gives the same bits (tests/_seg_augment_ref.py).  For pair m and OUTPUT pixel (x, y):
 *   source   affine (M, 6) int32 = A0 .. A5 in Q16 (65536 = 1.0): sx = A0 x + A1 y + A2, sy = A3 x + A4 y + A5, then sx clamped to
 *            [0, (W - 1) << 16] and sy to [0, (H - 1) << 16]: the edge is replicated, for the frame and the label map alike
 *   label    out_lab = lab[m][(sy + 0x8000) >> 16][(sx + 0x8000) >> 16]
 *   frame    x0 = sx >> 16, fx = (sx & 0xffff) >> 8, x1 = min(x0 + 1, W - 1), the same for y; with pYX = img[m][yY][xX]
 *            v = ((p00 (256 - fx) + p01 fx) (256 - fy) + (p10 (256 - fx) + p11 fx) fy + 0x8000) >> 16
 *   lines    lines (M, L, 6) int32 = (x0, y0, x1, y1, width, value) per line, in OUTPUT coordinates, the frame only, a later line
 *            over an earlier one.  The end points are clamped to [-4096, 8191], width to [0, 255], value is taken & 255.  With
 *            dx = x1 - x0, dy = y1 - y0, len2 = dx^2 + dy^2, t = (x - x0) dx + (y - y0) dy, c = (x - x0) dy - (y - y0) dx the pixel is
 *            covered iff width >= 1, len2 > 0, 0 <= t <= len2 and 4 c^2 <= width^2 len2; a covered pixel takes v = value
 *   output   out_f32 = lut_f32[m][v], out_u8 = lut_u8[m][v]   (lut_f32 (M, 256) float, lut_u8 (M, 256) uint8)
 * Any int32 coefficients and line entries are in bounds: the launcher cannot read them, the kernel clamps.  img with out_f32 and out_u8
 * may be NULL (labels only), or lab with out_lab (frames only); each of out_f32 and out_u8 may be NULL on its own, with its table.
 * Before any launch, in this order: S2E_ERR_ARG on a NULL affine, on no output at all, on an image output without img, on out_lab
 * without lab, on M, H or W < 1, on L < 0 or L > 0 without lines, on out_f32 without lut_f32 or out_u8 without lut_u8, on affine, lines,
 * lut_f32 or out_f32 off 4-byte alignment, on an output pointer equal to an input pointer; S2E_ERR_UNSUPPORTED on H or W > 4096, on
 * L > 8.  Planes of any other alignment and width work: outputs off 16 / 4 / 4 bytes or W % 4 != 0 take element stores. */
int s2e_augment_pairs(const uint8_t* img, const uint8_t* lab, int M, int H, int W, const int32_t* affine, const int32_t* lines, int L,
                      const float* lut_f32, const uint8_t* lut_u8, float* out_f32, uint8_t* out_u8, uint8_t* out_lab, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SEG2EYE_HIP_H */
