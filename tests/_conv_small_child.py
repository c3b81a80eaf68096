#!/usr/bin/env python3
"""The degenerate-channel convolutions of csrc/conv_small.hip -- Cout == 1 (the image conv, the PatchGAN heads) and Cin == 1 (the
encoder's first layer): forward, data gradient and weight gradient -- against fp64, element by element and kernel by kernel:
fwd_cout1_kernel, fwd_cout1_mfma_kernel, fwd_cin1_kernel, dgrad_cout1_kernel, tap_gemm_kernel<KS, DGRAD>, wgrad_cout1_kernel,
wgrad_cin1_kernel, small_wgrad_reduce_kernel and the band staging they share.

Run by tests/test_conv_small_fp64_gpu.py as a child process per environment (the library reads S2E_DETERMINISTIC once per process):

    python tests/_conv_small_child.py --groups mfma_a,mfma_b,cout1,band,tap             (bf16)
    python tests/_conv_small_child.py --groups cout1_f32,band_f32,wgrad_f32             (fp32)
    python tests/_conv_small_child.py --groups wgrad,wgrad_f32                          (also under S2E_DETERMINISTIC=1)
    python tests/_conv_small_child.py --groups ... --plan                               (no GPU: routes and workspace sizes only)

Everything goes through the C ABI (seg2eye_amd._lib): s2e_conv2d, s2e_conv2d_wgrad, the kind and workspace queries and
s2e_pack_conv_weight (into a NaN-filled matrix: the pack's contract is that it writes every element, padding included, and
tap_gemm_kernel relies on the zero columns 9..15 of a 3x3 weight).

Plan mirrors.  small_conv_kind / small_wgrad_kind, band_plan, cout1_mfma_plan, the capped grid of fwd_cout1_kernel, the weight
gradients' grid (SMALL_WS_CAP) and the slab count of the reduce kernel are mirrored below; fwd_plan() / wgrad_plan() name the kernel
a case runs in.  Every case asserts that the library's kernel kind is S2E_KERNEL_SMALL and (weight gradients) that the workspace is
grid * KS*KS*C*4 bytes.  The mirrors also count what a case exercises (COUNTERS); no counter may be zero over the shipped lists.

Reference, forward and data gradient.  fp64 of exactly what the kernel multiplies, epilogue in the kernels' order (epilogue64 of
tests/_conv_generic_child.py).  With in_act = LRELU the operand follows the kernel the mirror names: the matrix-core forms
(fwd_cout1_mfma_kernel, tap_gemm_kernel) round lrelu(x) back to bf16 (operand64); fwd_cout1_kernel, fwd_cin1_kernel and every fp32
case multiply the fp32 value 0.2f * x.
Bound, per element: |got - ref| <= rel |ref| + C_ACC A, rel = 2^-8 (bf16 outputs) or 2^-23 (fp32), A the absolute-value twin, C_ACC =
2^-16 of tests/_conv3x3_child.py (256 fp32 roundings of at most 2^-24 A each, linear; its derivation needs K <= 9216 and K <= 8192
here).  Why these kernels sit inside it: the vector kernels' longest dependent chain is KS*KS*vec <= 128 FMAs (fwd_cout1_kernel: a
lane's taps x its 8 / 4 channels; fwd_cin1 / dgrad_cout1: 16 taps) followed by log2 G <= 6 shuffle adds and at most three epilogue
adds -- <= 137 roundings, each of at most 2^-24 A, against the 256 allowed.  The dot-then-stencil kernel's MFMA adds Cin / wk / 16 <= 8
K-steps of 16 exact products (<= 8 roundings, plus the MFMA's internal ones, which the derivation of C_ACC covers), and its stencil adds
16 taps in each of wk <= 4 slabs and then the slabs: <= 16 * 4 + 4 = 68 roundings, with bias and residual <= 80.  tap_gemm_kernel is
one K-step.  tanh outputs and fp32 outputs are treated as in _conv_generic_child.py: tanh is 1-Lipschitz and passes A unchanged (tanhf's
own error, a few fp32 ulps of a value <= 1, is inside rel |ref| + C_ACC A since A >= |pre-activation| >= |tanh|), fp32 outputs use rel =
2^-23.

Reference, weight gradient.  dw and dbias start non-zero (the ABI accumulates); ref = start + the fp64 sum over pixels of
gy * in_act(x), in_act(x) the fp32 value 0.2f * x (the kernels apply lrelu02 to the unpacked value); dbias = start + the fp64 column
sum of gy (s2e_colsum).  Bound, per element: |got - (start + ref)| <= 2^-23 |start + ref| + c_w A, A = sum over pixels of |gy| |x|.

c_w, from the summation the kernels do (linear worst case: a rounding of a partial sum is at most u = 2^-24 times the partial sum of
absolute values, which is at most A, so a term that passes through D additions collects at most D u A; c_w = 1.01 D u, the 1.01 for the
second-order terms (1 + u)^D - 1 - D u, D < 2^14):
    D = T                      a thread's serial FMA chain: (items per workgroup) x ceil(largest item's pixels / pixel slots)
      + 2                      the fp32 rounding of 0.2f * x, and of the product should the compiler not contract the FMA
      + log2(64 / G)           block_partial_out: shuffle tree over the lanes of a wave that share a channel group
      + 3                      the four waves through LDS (the first stores 0 + acc, exact)
      + ceil(nb / (16 slabs))  small_wgrad_reduce_kernel: the four-way unrolled chain of one of a0..a3 over its slab's rows ...
      + 3                      ... the tail loop on a0
      + 2 + 2                  (a0 + a1) + (a2 + a3), and the same over the four row phases
      + 2 slabs                one float atomic per slab into dw, each rounding a value of at most |start| + A <= 2 A
                               (every case asserts |start| <= A element-wise)
wgrad_plan() computes D per case from the mirror (wgrad_depth), so a long chain does not loosen the bound of a short one.  dbias:
s2e_colsum's chain is at most 64 rows per thread (vector form) or ceil(M / (256 blocks' threads)) (scalar form, Cout == 1), an 8-step
fold, and one atomic per block at 2 u each: colsum_depth().
A dropped pixel changes an element by about A / npix (npix = N * Ho * Wo); every case asserts npix * (2^-22 + c_w) <= 1/2, i.e.
bound <= 2^-23 |start + ref| + c_w A <= (2^-22 + c_w) A <= A / (2 npix): half a dropped term is already outside the bound.
CPU check of c_w before any GPU run: emulate_wgrad() below redoes the kernels' summation order in numpy fp32 (threads, shuffles, waves,
workspace rows, reduce phases, slabs) for EMULATED = (WGRAD[3], WGRAD_F32[0]); tests/test_conv_small_plan_host.py asserts it inside the
bound.  Its worst error / bound: 0.004 (bf16 512 -> 1 4x4, 232 blocks, 7 slabs) and 0.03 (fp32 1 -> 4 3x3 stride 2).

Guards.  Outputs live in Guarded buffers and start as NaN (dw / dbias: as their start values); the workspace is exactly the queried
size, NaN-poisoned and guarded; a workspace 256 bytes short, or NULL, must return S2E_ERR_ARG with a message and leave dw bit-unchanged.
Forward and data-gradient cases run twice and must be bit-identical; weight gradients must be bit-identical (dw; dbias comes from
s2e_colsum's atomics) only where the mirror says one slab, which S2E_DETERMINISTIC=1 forces -- otherwise the slabs meet in float
atomics and only the bound applies.  Prints 'conv small ok: ...' last."""
import argparse
import ctypes as C
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch                                   # noqa: E402
import torch.nn.functional as F                # noqa: E402

from _conv3x3_child import BF16_RNE, C_ACC, Guarded, check_close, workspace                      # noqa: E402
from _conv_generic_child import (ACT_LRELU, ACT_NONE, ACT_TANH, AUX_LRELU_GRAD, AUX_NONE, AUX_RELU_MASK, F32_RNE, S2E_BF16,   # noqa: E402
                                 S2E_F32, Ep, Geo, add_counters, ceil_div, conv64, desc_fields, ep_name, epilogue64, geo_name, k_of,
                                 operand64, operands, out_hw, weight64)

KERNEL_SMALL = 1                               # S2E_KERNEL_SMALL
ERR_ARG = -1                                   # S2E_ERR_ARG
K_MAX = 8192                                   # 16 taps x 512 channels: inside the 9216 of C_ACC's derivation
assert C_ACC == 2.0 ** -16 and K_MAX <= 9216     # the docstring's count of roundings is against this constant
SMALL_NONE, FWD_COUT1, FWD_CIN1, DGRAD_COUT1, WGRAD_COUT1, WGRAD_CIN1 = 0, 1, 2, 3, 4, 5
SMALL_WS_CAP = 8 << 20
MFMA_CAND = (32, 24, 16, 12, 9, 8, 7, 6)
U32 = 2.0 ** -24
SWITCHES = ('S2E_DETERMINISTIC', 'S2E_CONV_C8')


def vec_of(dt):
    return 8 if dt == S2E_BF16 else 4


def pow2_le64(g):
    return 1 <= g <= 64 and g & (g - 1) == 0


def deterministic(env=None):
    v = (os.environ if env is None else env).get('S2E_DETERMINISTIC')
    try:
        return v is not None and int(v) != 0
    except ValueError:
        return False


# ---- plan mirrors (csrc/conv_small.hip)
def c8s2_takes(f, dt):
    """s2e_c8s2_fwd_ok / s2e_c8s2_dgrad_ok (conv_c8.hip) by shape alone: kinds 6 and 7, which no case here may be"""
    N, Hi, Wi, Cin, Ho, Wo, Cout, KH, KW, stride, pad, tr = f[:12]
    return dt == S2E_BF16 and KH == 4 and KW == 4 and stride == 2 and pad == 2 and {Cin, Cout} == {8, 64}


def small_conv_kind(f, dt):
    """s2e_small_conv_kind for a descriptor that conv_c8.hip does not take"""
    N, Hi, Wi, Cin, Ho, Wo, Cout, KH, KW, stride, pad, tr, in_act, out_act, aux = f
    vec = vec_of(dt)
    if not (KH == KW and KH in (3, 4)):
        return SMALL_NONE
    assert not c8s2_takes(f, dt), 'a conv_c8.hip shape'
    if not tr and Cout == 1 and Cin % vec == 0 and pow2_le64(Cin // vec) and aux == AUX_NONE:
        return FWD_COUT1
    if not tr and Cin == 1 and Cout % vec == 0 and pow2_le64(Cout // vec) and aux == AUX_NONE:
        return FWD_CIN1
    if tr and stride == 1 and Cin == 1 and Cout % vec == 0 and pow2_le64(Cout // vec) and in_act == ACT_NONE and out_act == ACT_NONE:
        return DGRAD_COUT1
    return SMALL_NONE


def small_wgrad_kind(f, dt):
    """s2e_small_wgrad_kind"""
    N, Hi, Wi, Cin, Ho, Wo, Cout, KH, KW, stride, pad = f[:11]
    vec = vec_of(dt)
    if not (KH == KW and KH in (3, 4)):
        return SMALL_NONE
    if Cout == 1 and stride == 1 and Cin % vec == 0 and pow2_le64(Cin // vec):
        return WGRAD_COUT1
    if Cin == 1 and Cout % vec == 0 and pow2_le64(Cout // vec):
        return WGRAD_CIN1
    return SMALL_NONE


def band_plan(N, H, W, h1, w1, s, org, flip, KS, target):
    """band_plan: the work items of a band kernel over the wide tensor (N, H, W, C); (h1, w1) the 1-channel tensor"""
    segw = min(W, 256)
    segs = ceil_div(W, segw)
    rows = max(1, min(8, ceil_div(N * H * segs, target)))
    rows = min(rows, H)
    bands = ceil_div(H, rows)
    return dict(N=N, H=H, W=W, h1=h1, w1=w1, s=s, org=org, flip=flip, KS=KS, segw=segw, segs=segs, rows=rows, bands=bands,
                items=N * bands * segs, pc=(segw - 1) * s + KS, last_rows=H - (bands - 1) * rows, last_cols=W - (segs - 1) * segw)


def band_item_shapes(bd):
    """the distinct (rows, columns) of a band plan's items"""
    return sorted({(nr, nc) for nr in (bd['rows'], bd['last_rows']) for nc in (bd['segw'], bd['last_cols'])})


def band_patch_elems(bd, nr, nc):
    """elements band_stage_each copies for an item of nr x nc pixels"""
    return ((nr - 1) * bd['s'] + bd['KS']) * ((nc - 1) * bd['s'] + bd['KS'])


def cout1_mfma_fits(t, KS, wk):
    return (t + KS - 1) ** 2 * ((KS * KS) | 1) * 4 * wk <= 48 * 1024


def cout1_mfma_allowed(KS, wk):
    """the candidates of cout1_mfma_plan that fit in 48 KB of LDS"""
    return tuple(t for t in MFMA_CAND if cout1_mfma_fits(t, KS, wk))


def cout1_mfma_plan(f):
    """cout1_mfma_plan: (rectangle, wk, NKW) or None"""
    N, Hi, Wi, Cin, Ho, Wo, Cout, KH, KW, stride, pad = f[:11]
    if stride != 1 or KH != KW or Cin not in (64, 128, 256, 512):
        return None
    wk = 4 if Cin >= 256 else 1
    pick = 0
    for t in MFMA_CAND:
        tt = min(t, max(Ho, Wo))
        if not cout1_mfma_fits(tt, KH, wk):
            continue
        pick = tt
        if N * ceil_div(Ho, tt) * ceil_div(Wo, tt) >= 256:
            break
    return (pick, wk, Cin // 16 // wk) if pick else None


def fwd_plan(f, dt):
    """The kernel s2e_conv2d runs a forward / data-gradient descriptor in, with its launch numbers; None: not a small shape."""
    N, Hi, Wi, Cin, Ho, Wo, Cout, KH, KW, stride, pad, tr, in_act, out_act, aux = f
    kind = small_conv_kind(f, dt)
    if kind == SMALL_NONE:
        return None
    KS, vec = KH, vec_of(dt)
    if kind == FWD_COUT1:
        mp = cout1_mfma_plan(f) if dt == S2E_BF16 else None
        if mp:
            t, wk, nkw = mp
            return dict(kind=kind, kernel='fwd_cout1_mfma', KS=KS, t=t, wk=wk, nkw=nkw, tiles_x=ceil_div(Wo, t), tiles_y=ceil_div(Ho, t),
                        grid=N * ceil_div(Wo, t) * ceil_div(Ho, t), PP=(t + KS - 1) ** 2, rounded_in_act=True,
                        lds=wk * (t + KS - 1) ** 2 * ((KS * KS) | 1) * 4)
        G = Cin // vec
        ppb, M = 256 // G, N * Ho * Wo
        g = ceil_div(M, ppb)
        return dict(kind=kind, kernel='fwd_cout1', KS=KS, G=G, ppb=ppb, M=M, grid=max(1, min(g, 4096)), capped=g > 4096, rounded_in_act=False)
    fwd = kind == FWD_CIN1
    bd = band_plan(N, Ho, Wo, Hi, Wi, stride, -pad, 0, KS, 1024) if fwd else band_plan(N, Ho, Wo, Hi, Wi, 1, pad - (KS - 1), 1, KS, 1024)
    tap = dt == S2E_BF16 and Cout % 32 == 0
    G = Cout // vec
    return dict(kind=kind, kernel=('tap_gemm_fwd' if fwd else 'tap_gemm_dgrad') if tap else ('fwd_cin1' if fwd else 'dgrad_cout1'), KS=KS,
                band=bd, grid=min(bd['items'], 1024), G=G, ppb=256 // G, C=Cout, rounded_in_act=tap)


def wgrad_plan(f, dt, det=None):
    """The weight-gradient launch of a small shape: band, grid, workspace, slabs of the reduce kernel, and the depth of its sums."""
    N, Hi, Wi, Cin, Ho, Wo, Cout, KH, KW, stride, pad = f[:11]
    kind = small_wgrad_kind(f, dt)
    if kind == SMALL_NONE:
        return None
    det = deterministic() if det is None else det
    c = Cin if kind == WGRAD_COUT1 else Cout
    nout = KH * KW * c
    cap = SMALL_WS_CAP // (nout * 4)
    gmax = max(1, min(1024, cap))
    bd = (band_plan(N, Hi, Wi, Ho, Wo, 1, pad - (KH - 1), 1, KH, gmax) if kind == WGRAD_COUT1
          else band_plan(N, Ho, Wo, Hi, Wi, stride, -pad, 0, KH, gmax))
    grid = min(bd['items'], gmax)
    slabs = 1 if det else max(1, min(8, grid // 32))
    G = c // vec_of(dt)
    pl = dict(kind=kind, kernel='wgrad_cout1' if kind == WGRAD_COUT1 else 'wgrad_cin1', KS=KH, band=bd, grid=grid, gmax=gmax,
              ws_capped=cap < 1024, workspace=grid * nout * 4, nout=nout, slabs=slabs, G=G, ppb=256 // G, C=c,
              lds=nout * 4 + ((bd['rows'] - 1) * bd['s'] + KH) * bd['pc'] * 4)
    pl['depth'] = wgrad_depth(pl)
    pl['c_w'] = 1.01 * pl['depth'] * U32
    return pl


def wgrad_depth(pl):
    """D of the docstring: the most additions a term of the sum passes through"""
    bd = pl['band']
    T = ceil_div(bd['items'], pl['grid']) * ceil_div(bd['rows'] * bd['segw'], pl['ppb'])
    return (T + 2 + int(math.log2(64 // pl['G'])) + 3 + ceil_div(pl['grid'], 16 * pl['slabs']) + 3 + 4 + 2 * pl['slabs'])


def colsum_depth(M, Cc, dt):
    """s2e_colsum (csrc/norm_modulate.hip): thread chain, fold, one atomic per block (2 u each: |start| <= A)"""
    vec = vec_of(dt)
    if Cc % vec:
        grid = min(M // 1024 + 1, 256)
        return ceil_div(M, grid * 256) + 6 + 3 + 2 * grid
    cgb = min(Cc // vec, 256)
    rpp = 256 // cgb
    return 64 + 8 + 2 * ceil_div(M, rpp * 64)


# ---- what a case exercises
BAND_COUNTERS = ('rows_1', 'rows_2_7', 'rows_8', 'ragged_last_band', 'segs_1', 'segs_2plus', 'W_256', 'W_257', 'items_gt_grid',
                 'patch_le_256', 'patch_gt_1024', 'stride2_fwd_cin1', 'stride2_wgrad_cin1', 'flip_pad0', 'flip_padKm1',
                 'G1_walk_wraps_rows', 'G64', 'item_px_lt_slots', 'inflight_pair_half_dead',
                 'kernel_fwd_cin1', 'kernel_dgrad_cout1', 'kernel_tap_gemm_fwd', 'kernel_tap_gemm_dgrad', 'kernel_wgrad_cout1',
                 'kernel_wgrad_cin1')
TAP_COUNTERS = ('ncb_1', 'ncb_2', 'ncb_16', 'npix_mod32', 'npix_lt32', 'ks3', 'ks4', 'fwd_bias', 'fwd_res', 'fwd_lrelu', 'fwd_tanh',
                'fwd_in_lrelu', 'dgrad_aux_none', 'dgrad_relu_mask', 'dgrad_lrelu_grad')
MFMA_COUNTERS = tuple('rect_wk%d_%d' % (wk, t) for wk in (1, 4) for t in sorted(set(cout1_mfma_allowed(3, wk)) | set(cout1_mfma_allowed(4, wk)))) + (
    'clamp_lt6', 'ragged_x', 'ragged_y', 'pp_mod32', 'nrb_lt4_wk1', 'nkw4_wk1', 'nkw8_wk1', 'nkw4_wk4', 'nkw8_wk4', 'ks3_wk1', 'ks4_wk1',
    'ks3_wk4', 'ks4_wk4', 'cin64', 'cin128', 'cin256', 'cin512', 'res', 'tanh', 'lrelu', 'in_lrelu')
COUT1_COUNTERS = ('bf16_cin8', 'bf16_cin16', 'bf16_cin32', 'f32_cin4', 'f32_cin8', 'f32_cin16', 'f32_cin32', 'f32_cin64', 'f32_cin128', 'f32_cin256',
                  'bf16_stride2_cin64', 'bf16_stride2_cin512', 'grid_cap_taken', 'grid_cap_not_taken', 'ks3', 'ks4', 'in_lrelu', 'res', 'tanh')
WGRAD_COUNTERS = ('kind4_ks3', 'kind4_ks4', 'kind5_ks3', 'kind5_ks4', 'kind5_stride1', 'kind5_stride2', 'gmax_ws_cap', 'gmax_1024', 'slabs_1',
                  'slabs_2_7', 'slabs_8', 'nb_not_multiple_of_4slabs', 'nb_lt_4', 'unrolled_loop_entered', 'unrolled_loop_not_entered',
                  'nout_mod64', 'in_lrelu')
COUNTERS = dict(band=BAND_COUNTERS, tap=TAP_COUNTERS, mfma=MFMA_COUNTERS, cout1=COUT1_COUNTERS, wgrad=WGRAD_COUNTERS)


def band_counters(pl, f, wgrad):
    c = dict.fromkeys(BAND_COUNTERS, 0)
    bd, ppb = pl['band'], pl['ppb']
    c['kernel_' + pl['kernel']] = 1
    c['rows_1'], c['rows_2_7'], c['rows_8'] = int(bd['rows'] == 1), int(2 <= bd['rows'] <= 7), int(bd['rows'] == 8)
    c['ragged_last_band'] = int(bd['H'] % bd['rows'] != 0)
    c['segs_1'], c['segs_2plus'] = int(bd['segs'] == 1), int(bd['segs'] >= 2)
    c['W_256'], c['W_257'] = int(bd['W'] == 256), int(bd['W'] == 257)
    c['items_gt_grid'] = int(bd['items'] > pl['grid'])
    shapes = band_item_shapes(bd)
    c['patch_le_256'] = int(any(band_patch_elems(bd, nr, nc) <= 256 for nr, nc in shapes))
    c['patch_gt_1024'] = int(any(band_patch_elems(bd, nr, nc) > 1024 for nr, nc in shapes))
    c['stride2_fwd_cin1'] = int(bd['s'] == 2 and not wgrad)
    c['stride2_wgrad_cin1'] = int(bd['s'] == 2 and wgrad)
    pad, KS = f[10], bd['KS']
    c['flip_pad0'], c['flip_padKm1'] = int(bd['flip'] == 1 and pad == 0), int(bd['flip'] == 1 and pad == KS - 1)
    vector = not pl['kernel'].startswith('tap_gemm')                   # (the matrix-core form has no Walk and no pixel slots)
    # a slot's second pixel lies several rows down: needs rows * columns > 256 with < 128 columns, i.e. about 200k pixels at 1024 items --
    # more than a weight-gradient case may have (wgrad_bounds), so a data-gradient case sets it; the Walk code is the same
    c['G1_walk_wraps_rows'] = int(vector and pl['G'] == 1 and any(2 * nc <= ppb < nr * nc for nr, nc in shapes))
    c['G64'] = int(vector and pl['G'] == 64)
    c['item_px_lt_slots'] = int(vector and any(nr * nc < ppb for nr, nc in shapes))
    # SMALL_INFLIGHT = 2: a slot with an odd number of pixels ends on a pair whose second pixel is dead
    c['inflight_pair_half_dead'] = int(wgrad and any(ceil_div(nr * nc - ty, ppb) % 2 == 1 for nr, nc in shapes for ty in (0, min(ppb, nr * nc) - 1)))
    return c


def tap_counters(pl, f, ep):
    c = dict.fromkeys(TAP_COUNTERS, 0)
    shapes = band_item_shapes(pl['band'])
    ncb = pl['C'] // 32
    if ncb in (1, 2, 16):
        c['ncb_%d' % ncb] = 1
    c['npix_mod32'] = int(any(nr * nc % 32 for nr, nc in shapes))
    c['npix_lt32'] = int(any(nr * nc < 32 for nr, nc in shapes))
    c['ks%d' % pl['KS']] = 1
    if pl['kernel'] == 'tap_gemm_fwd':
        c['fwd_bias'], c['fwd_res'] = int(ep.bias), int(ep.res)
        c['fwd_lrelu'], c['fwd_tanh'], c['fwd_in_lrelu'] = int(ep.out_act == ACT_LRELU), int(ep.out_act == ACT_TANH), int(ep.in_act == ACT_LRELU)
    else:
        c['dgrad_aux_none'], c['dgrad_relu_mask'] = int(ep.aux == AUX_NONE), int(ep.aux == AUX_RELU_MASK)
        c['dgrad_lrelu_grad'] = int(ep.aux == AUX_LRELU_GRAD)
    return c


def mfma_counters(pl, f, ep):
    c = dict.fromkeys(MFMA_COUNTERS, 0)
    Cin, Ho, Wo = f[3], f[4], f[5]
    t, wk, KS = pl['t'], pl['wk'], pl['KS']
    if t in MFMA_CAND:
        c['rect_wk%d_%d' % (wk, t)] = 1
    c['clamp_lt6'] = int(t < 6)
    c['ragged_x'], c['ragged_y'] = int(Wo % t != 0), int(Ho % t != 0)
    c['pp_mod32'] = int(pl['PP'] % 32 != 0)
    c['nrb_lt4_wk1'] = int(wk == 1 and ceil_div(pl['PP'], 32) < 4)
    c['nkw%d_wk%d' % (pl['nkw'], wk)] = 1
    c['ks%d_wk%d' % (KS, wk)] = 1
    c['cin%d' % Cin] = 1
    c['res'], c['tanh'], c['lrelu'] = int(ep.res), int(ep.out_act == ACT_TANH), int(ep.out_act == ACT_LRELU)
    c['in_lrelu'] = int(ep.in_act == ACT_LRELU)
    return c


def cout1_counters(pl, f, ep, dt):
    c = dict.fromkeys(COUT1_COUNTERS, 0)
    Cin, stride = f[3], f[9]
    name = '%s_cin%d' % ('bf16' if dt == S2E_BF16 else 'f32', Cin)
    if stride == 1 and name in c:
        c[name] = 1
    if dt == S2E_BF16 and stride == 2 and Cin in (64, 512):
        c['bf16_stride2_cin%d' % Cin] = 1
    c['grid_cap_taken'], c['grid_cap_not_taken'] = int(pl['capped']), int(not pl['capped'])
    c['ks%d' % pl['KS']] = 1
    c['in_lrelu'], c['res'], c['tanh'] = int(ep.in_act == ACT_LRELU), int(ep.res), int(ep.out_act == ACT_TANH)
    return c


def wgrad_counters(pl, f, in_act):
    c = dict.fromkeys(WGRAD_COUNTERS, 0)
    kind, KS, stride = pl['kind'], pl['KS'], f[9]
    c['kind%d_ks%d' % (kind, KS)] = 1
    if kind == WGRAD_CIN1:
        c['kind5_stride%d' % stride] = 1
    c['gmax_ws_cap'], c['gmax_1024'] = int(pl['ws_capped']), int(not pl['ws_capped'])
    nb, slabs = pl['grid'], pl['slabs']
    c['slabs_1'], c['slabs_2_7'], c['slabs_8'] = int(slabs == 1), int(2 <= slabs <= 7), int(slabs == 8)
    c['nb_not_multiple_of_4slabs'] = int(nb % (4 * slabs) != 0)
    c['nb_lt_4'] = int(nb < 4)
    c['unrolled_loop_entered'] = int(nb > 12 * slabs)                  # b + 3 * stride < nb at b = 0, stride = 4 * slabs
    c['unrolled_loop_not_entered'] = int(nb <= 12 * slabs)
    c['nout_mod64'] = int(pl['nout'] % 64 != 0)
    c['in_lrelu'] = int(in_act == ACT_LRELU)
    return c


def fwd_case_counters(pl, f, ep, dt):
    """{family: counters} of one forward / data-gradient launch"""
    if pl['kernel'] == 'fwd_cout1_mfma':
        return {'mfma': mfma_counters(pl, f, ep)}
    if pl['kernel'] == 'fwd_cout1':
        return {'cout1': cout1_counters(pl, f, ep, dt)}
    out = {'band': band_counters(pl, f, False)}
    if pl['kernel'].startswith('tap_gemm'):
        out['tap'] = tap_counters(pl, f, ep)
    return out


# ---- the cases.  Geo(N, H, W, cin, cout, k, s, p, dgrad): N x H x W the FORWARD conv's input
E = Ep
LIN = E(in_act=ACT_LRELU)
# dot-then-stencil: every rectangle the LDS cap allows, per wk; both NKW under both wk; KS 3 and 4
MFMA_A = [
    (Geo(32, 32, 256, 64, 1, 3, 1, 1, False), [E(bias=True, out_act=ACT_TANH)]),                        # wk 1, rectangle 32 (256 tiles)
    (Geo(16, 96, 96, 64, 1, 3, 1, 1, False), [E(bias=True, res=True)]),                                 # 24
    (Geo(16, 64, 64, 128, 1, 4, 1, 2, False), [E(bias=True, in_act=ACT_LRELU)]),                         # 16 at 65 x 65: ragged both ways
    (Geo(16, 48, 48, 64, 1, 4, 1, 1, False), [E(res=True, out_act=ACT_LRELU)]),                          # 12 at 47 x 47
]
MFMA_B = [
    (Geo(16, 36, 36, 128, 1, 3, 1, 1, False), [E(bias=True, out_act=ACT_TANH), LIN]),                   # 9
    (Geo(29, 17, 17, 64, 1, 3, 1, 1, False), [E(bias=True)]),                                            # 8: 4 N tiles of 9, 9 N of 8
    (Geo(29, 15, 15, 128, 1, 3, 1, 1, False), [E(res=True)]),                                            # 7
    (Geo(2, 13, 10, 64, 1, 4, 1, 2, False), [E(bias=True, res=True, out_act=ACT_LRELU)]),                # 6 at 14 x 11
    (Geo(3, 5, 4, 64, 1, 3, 1, 1, False), [E(bias=True), LIN]),                                          # clamp: t = 5, PP = 49: NRB = 2 < 4
    (Geo(16, 64, 64, 256, 1, 3, 1, 1, False), [E(bias=True)]),                                           # wk 4: 16
    (Geo(16, 48, 48, 256, 1, 3, 1, 1, False), [E(bias=True, in_act=ACT_LRELU)]),                         # 12
    (Geo(16, 37, 37, 512, 1, 4, 1, 1, False), [E(bias=True, res=True)]),                                 # 9 at 36 x 36 (4x4: 16 and 12 do not fit)
    (Geo(29, 17, 17, 256, 1, 4, 1, 2, False), [E(out_act=ACT_TANH)]),                                    # 8 at 18 x 18
    (Geo(29, 15, 15, 512, 1, 3, 1, 1, False), [E(bias=True, out_act=ACT_LRELU)]),                        # 7
    (Geo(2, 11, 9, 512, 1, 4, 1, 2, False), [E(bias=True), LIN]),                                        # 6 at 12 x 10
    (Geo(2, 4, 3, 256, 1, 4, 1, 2, False), [E(bias=True)]),                                              # clamp: t = 5 at 5 x 4
]
# the vector kernel: what the matrix-core plan does not take
COUT1 = [
    (Geo(2, 11, 13, 8, 1, 3, 1, 1, False), [E(bias=True), E(res=True, out_act=ACT_TANH, in_act=ACT_LRELU)]),
    (Geo(2, 11, 13, 16, 1, 4, 1, 2, False), [E(bias=True, res=True, out_act=ACT_LRELU)]),
    (Geo(3, 9, 7, 32, 1, 3, 1, 1, False), [E(bias=True, in_act=ACT_LRELU)]),
    (Geo(2, 21, 19, 64, 1, 3, 2, 1, False), [E(bias=True), LIN]),                                        # stride 2: reachable from the C ABI only
    (Geo(1, 16, 15, 512, 1, 4, 2, 1, False), [E(bias=True, res=True, out_act=ACT_TANH)]),
]
COUT1_F32 = [
    (Geo(2, 9, 11, 4, 1, 3, 1, 1, False), [E(bias=True), E(res=True, out_act=ACT_TANH, in_act=ACT_LRELU)]),
    (Geo(2, 9, 11, 8, 1, 4, 1, 2, False), [E(bias=True, res=True)]),
    (Geo(2, 9, 11, 16, 1, 3, 1, 1, False), [E(out_act=ACT_LRELU)]),
    (Geo(2, 9, 11, 32, 1, 4, 1, 1, False), [E(bias=True, in_act=ACT_LRELU)]),
    (Geo(2, 9, 11, 64, 1, 3, 2, 1, False), [E(bias=True)]),
    (Geo(2, 9, 11, 64, 1, 3, 1, 1, False), [E(bias=True)]),
    (Geo(2, 9, 11, 128, 1, 3, 1, 1, False), [E(res=True)]),
    (Geo(2, 96, 97, 256, 1, 3, 1, 1, False), [E(bias=True, out_act=ACT_TANH)]),                          # G = 64: M = 18624 > 16384: the cap
]
# band kernels, vector forms: bf16 with 8 / 16 channels (no whole 32-channel block)
BAND = [
    (Geo(8, 129, 12, 1, 8, 3, 1, 1, False), [E(bias=True, out_act=ACT_LRELU), E(res=True, in_act=ACT_LRELU)]),      # rows 2, ragged
    (Geo(16, 600, 8, 1, 8, 3, 1, 1, False), [E(bias=True)]),                                             # rows 8, items 1200 > 1024
    (Geo(16, 450, 40, 8, 1, 3, 1, 1, True), [E(aux=AUX_RELU_MASK)]),                                     # G 1, 8 x 40 items: the walk wraps rows
    (Geo(3, 180, 257, 1, 8, 3, 1, 1, False), [E(bias=True, out_act=ACT_TANH)]),                          # W 257: rows 2, patch 4 x 258
    (Geo(2, 20, 256, 16, 1, 4, 1, 2, True), [E(), E(aux=AUX_LRELU_GRAD)]),                               # dx 256 wide
    (Geo(2, 41, 37, 1, 16, 4, 2, 1, False), [E(bias=True, res=True)]),                                   # stride 2
    (Geo(2, 23, 19, 1, 8, 3, 2, 1, False), [LIN]),
    (Geo(2, 12, 9, 8, 1, 3, 1, 0, True), [E(), E(aux=AUX_RELU_MASK)]),                                   # flip, pad 0
    (Geo(2, 12, 9, 16, 1, 4, 1, 3, True), [E(aux=AUX_LRELU_GRAD)]),                                      # flip, pad KS - 1
    (Geo(2, 12, 9, 8, 1, 3, 1, 2, True), [E()]),
]
BAND_F32 = [
    (Geo(8, 129, 12, 1, 4, 3, 1, 1, False), [E(bias=True, res=True, out_act=ACT_LRELU)]),
    (Geo(2, 30, 21, 1, 256, 4, 2, 2, False), [E(bias=True, in_act=ACT_LRELU)]),                          # G 64
    (Geo(2, 19, 23, 1, 64, 3, 1, 1, False), [E(bias=True, out_act=ACT_TANH)]),
    (Geo(2, 19, 23, 256, 1, 4, 1, 1, True), [E(aux=AUX_RELU_MASK)]),
    (Geo(3, 180, 257, 4, 1, 3, 1, 1, True), [E(), E(aux=AUX_LRELU_GRAD)]),
    (Geo(2, 12, 9, 4, 1, 4, 1, 0, True), [E()]),
]
# taps as one K-step: bf16, whole 32-channel blocks
TAP = [
    (Geo(2, 19, 23, 1, 32, 3, 1, 1, False), [E(bias=True), E(res=True, out_act=ACT_LRELU), E(bias=True, res=True, out_act=ACT_TANH), LIN]),
    (Geo(2, 5, 5, 1, 64, 4, 1, 2, False), [E(bias=True, in_act=ACT_LRELU)]),                             # 6-pixel rows: npix < 32
    (Geo(2, 21, 23, 1, 512, 4, 2, 1, False), [E(bias=True, out_act=ACT_LRELU)]),                         # NCB 16, stride 2
    (Geo(8, 129, 12, 1, 64, 3, 1, 1, False), [E(bias=True, res=True)]),                                  # rows 2, ragged
    (Geo(16, 600, 8, 1, 32, 4, 2, 1, False), [E(bias=True)]),                                            # 300 x 4 out: rows 5
    (Geo(3, 180, 257, 1, 32, 3, 1, 1, False), [E(bias=True, in_act=ACT_LRELU)]),                         # 257: patch > 1024
    (Geo(2, 19, 23, 32, 1, 3, 1, 1, True), [E(), E(aux=AUX_RELU_MASK), E(aux=AUX_LRELU_GRAD)]),
    (Geo(2, 12, 9, 64, 1, 4, 1, 0, True), [E(aux=AUX_RELU_MASK)]),                                       # flip, pad 0
    (Geo(2, 12, 9, 512, 1, 4, 1, 3, True), [E(aux=AUX_LRELU_GRAD)]),                                     # flip, pad KS - 1, NCB 16
    (Geo(16, 600, 8, 64, 1, 3, 1, 1, True), [E()]),                                                      # rows 8, items > grid
    (Geo(2, 20, 256, 32, 1, 3, 1, 1, True), [E(aux=AUX_RELU_MASK)]),                                     # 256 wide
]
# weight gradients: (geometry of the forward conv, in_act)
WGRAD = [
    (Geo(2, 12, 10, 64, 1, 3, 1, 1, False), ACT_NONE),                                                   # kind 4
    (Geo(2, 12, 9, 8, 1, 4, 1, 0, False), ACT_LRELU),                                                    # flip with pad 0; G = 1
    (Geo(1, 3, 9, 16, 1, 4, 1, 3, False), ACT_NONE),                                                     # flip with pad KS - 1; 3 blocks
    (Geo(8, 225, 4, 512, 1, 4, 1, 2, False), ACT_NONE),                                                  # 512 ch, 4x4: at most 256 blocks; emulated on the CPU
    (Geo(4, 130, 12, 512, 1, 4, 1, 1, False), ACT_LRELU),                                                # rows 3 under the 256-block cap, ragged
    (Geo(16, 600, 8, 8, 1, 3, 1, 1, False), ACT_NONE),                                                   # rows 8, 1200 items on 1024 blocks
    (Geo(1, 100, 257, 16, 1, 3, 1, 1, False), ACT_NONE),                                                 # W 257
    (Geo(2, 50, 256, 8, 1, 3, 1, 1, False), ACT_LRELU),                                                  # W 256
    (Geo(3, 37, 41, 1, 64, 3, 2, 1, False), ACT_NONE),                                                   # kind 5, stride 2
    (Geo(2, 45, 20, 1, 16, 4, 2, 2, False), ACT_LRELU),
    (Geo(2, 23, 21, 1, 512, 4, 1, 1, False), ACT_NONE),                                                  # kind 5 at the workspace cap, G 64
    (Geo(2, 40, 11, 1, 32, 3, 1, 1, False), ACT_LRELU),
    (Geo(16, 300, 8, 1, 8, 3, 1, 1, False), ACT_NONE),                                                   # kind 5, G 1, rows 5
]
WGRAD_F32 = [
    (Geo(2, 17, 13, 1, 4, 3, 2, 1, False), ACT_LRELU),                                                   # nout 36; emulated on the CPU
    (Geo(2, 12, 10, 4, 1, 3, 1, 1, False), ACT_NONE),                                                    # nout 36, kind 4
    (Geo(2, 50, 19, 256, 1, 4, 1, 2, False), ACT_LRELU),                                                 # G 64
    (Geo(3, 37, 41, 1, 64, 4, 1, 2, False), ACT_NONE),
    (Geo(1, 100, 257, 4, 1, 3, 1, 1, False), ACT_NONE),
]
FWD_GROUPS = {'mfma_a': MFMA_A, 'mfma_b': MFMA_B, 'cout1': COUT1, 'band': BAND, 'tap': TAP, 'cout1_f32': COUT1_F32, 'band_f32': BAND_F32}
WGRAD_GROUPS = {'wgrad': WGRAD, 'wgrad_f32': WGRAD_F32}
EMULATED = (('wgrad', 3), ('wgrad_f32', 0))
# the kernel every case of a group is written for
GROUP_KERNELS = {'mfma_a': {'fwd_cout1_mfma'}, 'mfma_b': {'fwd_cout1_mfma'}, 'cout1': {'fwd_cout1'}, 'cout1_f32': {'fwd_cout1'},
                 'band': {'fwd_cin1', 'dgrad_cout1'}, 'band_f32': {'fwd_cin1', 'dgrad_cout1'}, 'tap': {'tap_gemm_fwd', 'tap_gemm_dgrad'},
                 'wgrad': {'wgrad_cout1', 'wgrad_cin1'}, 'wgrad_f32': {'wgrad_cout1', 'wgrad_cin1'}}

# routes that must NOT be the small kernels: (what, query, dtype, descriptor fields)
_N = (ACT_NONE, ACT_NONE, AUX_NONE)
NEGATIVE = [
    ('24 channels in bf16: C / vec = 3', 'fwd', S2E_BF16, (2, 9, 9, 24, 9, 9, 1, 3, 3, 1, 1, 0) + _N),
    ('24 channels out of 1 in bf16', 'fwd', S2E_BF16, (2, 9, 9, 1, 9, 9, 24, 3, 3, 1, 1, 0) + _N),
    ('1024 channels in bf16: C / vec = 128', 'fwd', S2E_BF16, (2, 9, 9, 1024, 9, 9, 1, 3, 3, 1, 1, 0) + _N),
    ('512 channels in fp32: C / vec = 128', 'fwd', S2E_F32, (2, 9, 9, 1, 9, 9, 512, 3, 3, 1, 1, 0) + _N),
    ('5x5', 'fwd', S2E_BF16, (2, 9, 9, 64, 9, 9, 1, 5, 5, 1, 2, 0) + _N),
    ('1x1', 'fwd', S2E_BF16, (2, 9, 9, 64, 9, 9, 1, 1, 1, 1, 0, 0) + _N),
    ('Cout == 1 forward with an aux operand', 'fwd', S2E_BF16, (2, 9, 9, 64, 9, 9, 1, 3, 3, 1, 1, 0, ACT_NONE, ACT_NONE, AUX_RELU_MASK)),
    ('Cout == 1 data gradient at stride 2', 'fwd', S2E_BF16, (2, 5, 5, 1, 9, 9, 64, 3, 3, 2, 1, 1) + _N),
    ('Cout == 1 weight gradient at stride 2', 'wgrad', S2E_BF16, (2, 9, 9, 64, 5, 5, 1, 3, 3, 2, 1, 0) + _N),
    ('5x5 weight gradient', 'wgrad', S2E_BF16, (2, 9, 9, 64, 9, 9, 1, 5, 5, 1, 2, 0) + _N),
    ('1x1 weight gradient', 'wgrad', S2E_F32, (2, 9, 9, 1, 9, 9, 64, 1, 1, 1, 0, 0) + _N),
    ('24-channel weight gradient in bf16', 'wgrad', S2E_BF16, (2, 9, 9, 24, 9, 9, 1, 3, 3, 1, 1, 0) + _N),
]


def group_dt(name):
    return S2E_F32 if name.endswith('_f32') else S2E_BF16


def wgrad_fields(g, in_act):
    return desc_fields(g, Ep(in_act=in_act))


def coverage(det=False):
    """the counters summed over the shipped lists, from the mirrors alone: {family: {counter: n}}"""
    tot = {fam: dict.fromkeys(names, 0) for fam, names in COUNTERS.items()}
    for name, cases in FWD_GROUPS.items():
        dt = group_dt(name)
        for g, eps in cases:
            for ep in eps:
                f = desc_fields(g, ep)
                for fam, c in fwd_case_counters(fwd_plan(f, dt), f, ep, dt).items():
                    add_counters(tot[fam], c)
    for name, cases in WGRAD_GROUPS.items():
        dt = group_dt(name)
        for g, in_act in cases:
            f = wgrad_fields(g, in_act)
            pl = wgrad_plan(f, dt, det)
            add_counters(tot['wgrad'], wgrad_counters(pl, f, in_act))
            add_counters(tot['band'], band_counters(pl, f, True))
    return tot


def zero_counters(tot):
    return ['%s.%s' % (fam, k) for fam, c in tot.items() for k, v in c.items() if v == 0]


def kernel_label(pl):
    k = pl['kernel']
    if k == 'fwd_cout1_mfma':
        return 'fwd_cout1_mfma<%d,%d> t=%d wk=%d grid=%d' % (pl['KS'], pl['nkw'], pl['t'], pl['wk'], pl['grid'])
    if k == 'fwd_cout1':
        return 'fwd_cout1<%d> G=%d grid=%d%s' % (pl['KS'], pl['G'], pl['grid'], ' (cap)' if pl['capped'] else '')
    bd = pl['band']
    s = '%s<%d> rows=%d segs=%d items=%d grid=%d' % (k, pl['KS'], bd['rows'], bd['segs'], bd['items'], pl['grid'])
    return s + (' slabs=%d' % pl['slabs'] if 'slabs' in pl else '')


# ---- fp64 references (CPU)
def small_operand64(x, in_act, dtype, rounded):
    """what the kernel multiplies for the stored x: the matrix-core forms round lrelu(x) back to the compute dtype, the others keep
    the fp32 value 0.2f * x"""
    if in_act == ACT_NONE or rounded:
        return operand64(x, in_act, dtype)
    xf = x.float()
    return torch.where(xf > 0, xf, xf * 0.2).double()


def small_reference(x, w, g, in_act, dtype, rounded):
    """(convolution, its absolute-value twin) of the launch of geometry g"""
    hw = (g.H, g.W) if g.dgrad else out_hw(g)
    xo, wq = small_operand64(x, in_act, dtype, rounded), weight64(w, dtype)
    return conv64(xo, wq, g.k, g.s, g.p, g.dgrad, hw), conv64(xo.abs(), wq.abs(), g.k, g.s, g.p, g.dgrad, hw)


def tap_windows(xp, g, ho, wo):
    """the KS*KS shifted (N, Ho, Wo, Ci) views of the padded input"""
    for ky in range(g.k):
        for kx in range(g.k):
            yield xp[:, ky:ky + (ho - 1) * g.s + 1:g.s, kx:kx + (wo - 1) * g.s + 1:g.s]


def wgrad64(xa, gy, g):
    """dw[co][(ky*K+kx)*Ci + ci] = sum over pixels of gy[n, oy, ox, co] * xa[n, oy*s-p+ky, ox*s-p+kx, ci], in the dtype of its arguments"""
    ho, wo = out_hw(g)
    xp = F.pad(xa, (0, 0, g.p, g.p, g.p, g.p))
    gm = gy.reshape(-1, g.cout).t().contiguous()
    cols = [gm @ win.reshape(-1, g.cin) for win in tap_windows(xp, g, ho, wo)]
    return torch.stack(cols, 1).reshape(g.cout, g.k * g.k * g.cin)


def wgrad_operands(g, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    ho, wo = out_hw(g)
    x = torch.randn(g.N, g.H, g.W, g.cin, generator=gen).to(dtype)
    gy = torch.randn(g.N, ho, wo, g.cout, generator=gen).to(dtype)
    dw0 = torch.randn(g.cout, g.k * g.k * g.cin, generator=gen) * 0.5
    db0 = torch.randn(g.cout, generator=gen) * 0.5
    return x, gy, dw0, db0


def wgrad_reference(x, gy, g, in_act):
    """(dw, A_w, dbias, A_b) in fp64, without the start values"""
    xf = x.float()
    xa = (torch.where(xf > 0, xf, xf * 0.2) if in_act == ACT_LRELU else xf).double()
    g64 = gy.double()
    return wgrad64(xa, g64, g), wgrad64(xa.abs(), g64.abs(), g), g64.sum((0, 1, 2)), g64.abs().sum((0, 1, 2))


def wgrad_bounds(pl, g, dt, A, dw0, Ab, db0):
    """c_w and the dbias constant of a case, with the conditions they rest on"""
    ho, wo = out_hw(g)
    npix = g.N * ho * wo
    c_w = pl['c_w']
    assert npix * (2.0 ** -22 + c_w) <= 0.5, '%s: %d pixels: a dropped pixel term (A / npix) would be inside the bound' % (geo_name(g), npix)
    assert bool((dw0.double().abs() <= A).all()) and bool((db0.double().abs() <= Ab).all()), '%s: |start| > A' % geo_name(g)
    return c_w, 1.01 * colsum_depth(npix, g.cout, dt) * U32


def check_wgrad(got, start, ref, A, c, what):
    """every element: |got - (start + ref)| <= 2^-23 |start + ref| + c A; returns the worst error / bound"""
    gd = got.detach().double().cpu().reshape(ref.shape)
    want = start.double().reshape(ref.shape) + ref
    bound = F32_RNE * want.abs() + c * A
    err = (gd - want).abs()
    ok = err <= bound
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError('%s: %d of %d elements outside the bound; first at %s: got %r, want %r, A %r, bound %.3e'
                             % (what, bad.shape[0], ok.numel(), i, float(gd[i]), float(want[i]), float(A[i]), float(bound[i])))
    return float((err / bound).max())


# ---- the kernels' summation order in numpy fp32 (CPU check of c_w)
def _fma32(acc, a, b):
    """fp32 fma: the product of two fp32 values is exact in fp64"""
    return (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)


def emulate_wgrad(x, gy, dw0, g, in_act, dt):
    """dw as wgrad_cout1_kernel / wgrad_cin1_kernel + small_wgrad_reduce_kernel sum it (slabs added in index order), as float32"""
    f = wgrad_fields(g, in_act)
    pl = wgrad_plan(f, dt, False)
    bd, G, ppb, KS, NT, Cc = pl['band'], pl['G'], pl['ppb'], g.k, g.k * g.k, pl['C']
    ho, wo = out_hw(g)
    xf = x.float()
    xa = (torch.where(xf > 0, xf, xf * 0.2) if in_act == ACT_LRELU else xf)
    if pl['kind'] == WGRAD_COUT1:             # wide = in_act(x) at q; tap t of pixel q = gy[q + pad - k]
        wide = xa.numpy()
        gp = F.pad(gy.float()[..., 0], (KS - 1, KS - 1, KS - 1, KS - 1)).numpy()
        taps = np.stack([gp[:, KS - 1 + g.p - ky:KS - 1 + g.p - ky + g.H, KS - 1 + g.p - kx:KS - 1 + g.p - kx + g.W]
                         for ky in range(KS) for kx in range(KS)], -1)
    else:                                     # wide = gy at o; tap t of pixel o = in_act(x)[o * s - p + k]
        wide = gy.float().numpy()
        xp = F.pad(xa, (0, 0, g.p, g.p, g.p, g.p))
        taps = np.stack([w_[..., 0].numpy() for w_ in tap_windows(xp, g, ho, wo)], -1)
    ws = np.zeros((pl['grid'], NT, Cc), np.float32)
    for b in range(pl['grid']):
        acc = np.zeros((ppb, NT, Cc), np.float32)
        for item in range(b, bd['items'], pl['grid']):
            sg, rest = item % bd['segs'], item // bd['segs']
            band, n = rest % bd['bands'], rest // bd['bands']
            y0, x0 = band * bd['rows'], sg * bd['segw']
            nr, nc = min(bd['rows'], bd['H'] - y0), min(bd['segw'], bd['W'] - x0)
            tp = taps[n, y0:y0 + nr, x0:x0 + nc].reshape(nr * nc, NT)
            wd = wide[n, y0:y0 + nr, x0:x0 + nc].reshape(nr * nc, Cc)
            for i0 in range(0, nr * nc, ppb):
                m = min(ppb, nr * nc - i0)
                acc[:m] = _fma32(acc[:m], tp[i0:i0 + m, :, None], wd[i0:i0 + m, None, :])
        v = acc.reshape(4, 64 // G, NT, Cc)                       # [wave][slot in wave]
        off = 1
        while off < 64 // G:                                      # __shfl_xor butterfly over the lanes that share tx
            v = v + v[:, np.arange(64 // G) ^ off]
            off <<= 1
        v = v[:, 0]
        ws[b] = ((v[0] + v[1]) + v[2]) + v[3]
    ws = ws.reshape(pl['grid'], -1) if pl['kind'] == WGRAD_COUT1 else ws.transpose(0, 2, 1).reshape(pl['grid'], -1)
    nb, slabs = pl['grid'], pl['slabs']
    dw = dw0.float().numpy().reshape(-1).copy()
    zero = np.zeros_like(dw)
    for sl in range(slabs):
        red = []
        for ph in range(4):
            a, stride, b = [zero.copy() for _ in range(4)], 4 * slabs, sl * 4 + ph
            while b + 3 * stride < nb:
                for u in range(4):
                    a[u] = a[u] + ws[b + u * stride]
                b += 4 * stride
            while b < nb:
                a[0] = a[0] + ws[b]
                b += stride
            red.append((a[0] + a[1]) + (a[2] + a[3]))
        dw = dw + ((red[0] + red[1]) + (red[2] + red[3]))
    return torch.from_numpy(dw), pl


def emulated_ratio(group, index):
    """worst error / bound of the fp32 emulation of shipped case `index` of `group`"""
    g, in_act = WGRAD_GROUPS[group][index]
    dt = group_dt(group)
    dtype = torch.bfloat16 if dt == S2E_BF16 else torch.float32
    x, gy, dw0, db0 = wgrad_operands(g, dtype, wgrad_seed(group, index))
    ref, A, rb, Ab = wgrad_reference(x, gy, g, in_act)
    got, pl = emulate_wgrad(x, gy, dw0, g, in_act, dt)
    c_w, _ = wgrad_bounds(pl, g, dt, A, dw0, Ab, db0)
    return check_wgrad(got, dw0, ref, A, c_w, 'emulated %s' % geo_name(g))


def wgrad_seed(group, index):
    return 3000 + 41 * index + (700 if group.endswith('_f32') else 0)


# ---- the library
def lib():
    from seg2eye_amd import _lib as L
    return L, L.lib()


def make_desc(f):
    L, _ = lib()
    return L.ConvDesc(*f)


def check_fwd_route(group, g, ep, dt):
    """kernel kind of the library against the mirror; returns the plan"""
    _, lb = lib()
    f = desc_fields(g, ep)
    what = '%s %s' % (geo_name(g), ep_name(ep))
    assert k_of(g) <= K_MAX, '%s: K = %d' % (what, k_of(g))
    pl = fwd_plan(f, dt)
    assert pl is not None and pl['kernel'] in GROUP_KERNELS[group], '%s: the mirror says %s, the case is written for %s' % (
        what, pl and pl['kernel'], sorted(GROUP_KERNELS[group]))
    d = make_desc(f)
    kind = lb.s2e_conv2d_kernel_kind(dt, C.byref(d))
    assert kind == KERNEL_SMALL, '%s: kernel kind %d, not S2E_KERNEL_SMALL' % (what, kind)
    wsb = int(lb.s2e_conv2d_workspace_bytes(dt, C.byref(d)))
    assert wsb == 0, '%s: the small forward kernels take no workspace, the library asks for %d bytes' % (what, wsb)
    return pl


def check_wgrad_route(group, g, in_act, dt):
    _, lb = lib()
    f = wgrad_fields(g, in_act)
    what = 'wgrad %s' % geo_name(g)
    pl = wgrad_plan(f, dt)
    assert pl is not None and pl['kernel'] in GROUP_KERNELS[group], what
    d = make_desc(f)
    kind = lb.s2e_conv2d_wgrad_kernel_kind(dt, C.byref(d))
    assert kind == KERNEL_SMALL, '%s: kernel kind %d, not S2E_KERNEL_SMALL' % (what, kind)
    wsb = int(lb.s2e_conv2d_wgrad_workspace_bytes(dt, C.byref(d)))
    assert wsb == pl['workspace'], '%s: the library asks for %d bytes of workspace, the mirror says grid %d x %d x 4 = %d' % (
        what, wsb, pl['grid'], pl['nout'], pl['workspace'])
    return pl


def check_negative():
    """the routes that must not be the small kernels"""
    _, lb = lib()
    for what, query, dt, f in NEGATIVE:
        d = make_desc(f)
        if query == 'fwd':
            assert small_conv_kind(f, dt) == SMALL_NONE, what
            kind = lb.s2e_conv2d_kernel_kind(dt, C.byref(d))
        else:
            assert small_wgrad_kind(f, dt) == SMALL_NONE, what
            kind = lb.s2e_conv2d_wgrad_kernel_kind(dt, C.byref(d))
        assert kind != KERNEL_SMALL, '%s: routed to the small kernels' % what
    return len(NEGATIVE)


def pack(w, dtype, dt, transposed, dev):
    """s2e_pack_conv_weight into a NaN-filled matrix: the pack writes every element, padding rows and the K tail as zeros"""
    L, lb = lib()
    cout, cin, kh, kw = w.shape
    rows = lb.s2e_conv_cout_pad(cin if transposed else cout)
    kpad = lb.s2e_conv_k_pad(dt, kh * kw * (cout if transposed else cin))
    out = torch.full((rows, kpad), float('nan'), dtype=dtype, device=dev)
    wd = w.float().contiguous().to(dev)
    L.check(lb.s2e_pack_conv_weight(dt, wd.data_ptr(), out.data_ptr(), None, cout, cin, kh, kw, cin, int(transposed),
                                    torch.cuda.current_stream().cuda_stream), 's2e_pack_conv_weight')
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out.float()).any()), 's2e_pack_conv_weight left elements of the padded matrix unwritten'
    return out


RESULTS = []
WORST = {}


def report(group, what, pl, worst, extra=''):
    WORST[group] = max(WORST.get(group, 0.0), worst)
    line = '  %-10s %-52s kernel=%-58s worst err/bound %.3f%s' % (group, what, kernel_label(pl), worst, extra)
    RESULTS.append(line)
    print(line, flush=True)


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def run_fwd_case(group, g, eps, dt, dev, seed, totals):
    L, lb = lib()
    dtype = torch.bfloat16 if dt == S2E_BF16 else torch.float32
    rel = BF16_RNE if dt == S2E_BF16 else F32_RNE
    x, w, bias, res, aux = operands(g, dtype, seed)
    xd, bd, resd, auxd = x.to(dev), bias.to(dev), res.to(dev), aux.to(dev)
    wp = pack(w, dtype, dt, g.dgrad, dev)
    pairs = {}
    stream = torch.cuda.current_stream().cuda_stream
    for ep in eps:
        what = '%s %s %s' % ('bf16' if dt == S2E_BF16 else 'f32', geo_name(g), ep_name(ep))
        pl = check_fwd_route(group, g, ep, dt)
        f = desc_fields(g, ep)
        for fam, c in fwd_case_counters(pl, f, ep, dt).items():
            add_counters(totals.setdefault(fam, {}), c)
        key = (ep.in_act, pl['rounded_in_act'])
        if key not in pairs:
            pairs[key] = small_reference(x, w, g, ep.in_act, dtype, pl['rounded_in_act'])
        ref, A = epilogue64(pairs[key][0], pairs[key][1], bias, res, aux, ep)
        d = make_desc(f)
        outs = []
        for rep in range(2):
            y = Guarded(tuple(res.shape), dtype, dev, float('nan'))
            L.check(lb.s2e_conv2d(dt, xd.data_ptr(), wp.data_ptr(), bd.data_ptr() if ep.bias else None, resd.data_ptr() if ep.res else None,
                                  auxd.data_ptr() if ep.aux != AUX_NONE else None, y.ptr(), C.byref(d), None, 0, stream), 's2e_conv2d')
            y.check('%s y (launch %d)' % (what, rep))
            outs.append(y.t.clone())
        worst = check_close(outs[0], ref, A, what, rel=rel)
        assert torch.equal(bits(outs[0]), bits(outs[1])), '%s: two launches differ' % what
        report(group, what, pl, worst)


def run_wgrad_case(group, index, g, in_act, dt, dev, totals):
    L, lb = lib()
    dtype = torch.bfloat16 if dt == S2E_BF16 else torch.float32
    what = 'wgrad %s %s%s' % ('bf16' if dt == S2E_BF16 else 'f32', geo_name(g), ' in-lrelu' if in_act else '')
    pl = check_wgrad_route(group, g, in_act, dt)
    f = wgrad_fields(g, in_act)
    add_counters(totals.setdefault('wgrad', {}), wgrad_counters(pl, f, in_act))
    add_counters(totals.setdefault('band', {}), band_counters(pl, f, True))
    x, gy, dw0, db0 = wgrad_operands(g, dtype, wgrad_seed(group, index))
    ref, A, rb, Ab = wgrad_reference(x, gy, g, in_act)
    c_w, c_b = wgrad_bounds(pl, g, dt, A, dw0, Ab, db0)
    xd, gyd = x.to(dev), gy.to(dev)
    d = make_desc(f)
    need = pl['workspace']
    stream = torch.cuda.current_stream().cuda_stream
    outs = []
    for rep in range(2):
        dw = Guarded(tuple(dw0.shape), torch.float32, dev, dw0)
        db = Guarded(tuple(db0.shape), torch.float32, dev, db0)
        ws = workspace(need, dev)
        L.check(lb.s2e_conv2d_wgrad(dt, xd.data_ptr(), gyd.data_ptr(), dw.ptr(), db.ptr(), C.byref(d), ws.ptr(), need, stream), 's2e_conv2d_wgrad')
        for b_, nm in ((dw, 'dw'), (db, 'dbias'), (ws, 'workspace')):
            b_.check('%s %s (launch %d)' % (what, nm, rep))
        outs.append((dw.t.clone(), db.t.clone()))
    worst = check_wgrad(outs[0][0], dw0, ref, A, c_w, what + ' dw')
    worst_b = check_wgrad(outs[0][1], db0, rb, Ab, c_b, what + ' dbias')
    worst = max(worst, check_wgrad(outs[1][0], dw0, ref, A, c_w, what + ' dw (second launch)'))
    bitwise = pl['slabs'] == 1
    if bitwise:
        assert torch.equal(bits(outs[0][0]), bits(outs[1][0])), '%s: one slab, and two launches differ' % what
    # a short or missing workspace: S2E_ERR_ARG with a message, dw untouched
    for wsb in (need - 256, None):
        dw = Guarded(tuple(dw0.shape), torch.float32, dev, dw0)
        ws = workspace(max(wsb or 0, 0), dev)
        rc = lb.s2e_conv2d_wgrad(dt, xd.data_ptr(), gyd.data_ptr(), dw.ptr(), None, C.byref(d), ws.ptr() if wsb is not None else None,
                                 max(wsb, 0) if wsb is not None else need, stream)
        torch.cuda.synchronize()
        msg = lb.s2e_last_error()
        assert rc == ERR_ARG and msg, '%s: workspace %s returned %d (%r)' % (what, 'NULL' if wsb is None else '256 bytes short', rc, msg)
        dw.check('%s dw (refused launch)' % what)
        assert torch.equal(bits(dw.t.cpu()), bits(dw0.float())), '%s: a refused launch changed dw' % what
    report(group, what, pl, worst, '  dbias %.3f  D=%d%s' % (worst_b, pl['depth'], '  x2 bitwise' if bitwise else ''))
    WORST[group] = max(WORST[group], worst_b)


def plan_only(names):
    """--plan: every case's route and workspace against the mirror, on the library alone (no GPU)"""
    n = 0
    for name in names:
        dt = group_dt(name)
        if name in FWD_GROUPS:
            for g, eps in FWD_GROUPS[name]:
                for ep in eps:
                    check_fwd_route(name, g, ep, dt)
                    n += 1
        else:
            for g, in_act in WGRAD_GROUPS[name]:
                check_wgrad_route(name, g, in_act, dt)
                n += 1
    return n + check_negative()


def print_counters(title, c):
    print('  %s: %s' % (title, ', '.join('%s=%d' % kv for kv in c.items())), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--groups', required=True)
    ap.add_argument('--plan', action='store_true', help='routes and workspace sizes only, without a GPU')
    args = ap.parse_args()
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    names = args.groups.split(',')
    lib()
    sw = ' '.join('%s=%s' % (k, os.environ[k]) for k in SWITCHES if k in os.environ) or 'defaults'
    if args.plan:
        print('conv small plan ok: %d routes, groups %s (%s)' % (plan_only(names), args.groups, sw), flush=True)
        return
    dev = torch.device('cuda', 0)
    check_negative()
    for name in names:
        totals = {}
        dt = group_dt(name)
        if name in FWD_GROUPS:
            for i, (g, eps) in enumerate(FWD_GROUPS[name]):
                run_fwd_case(name, g, eps, dt, dev, 2000 + 37 * i + (500 if dt == S2E_F32 else 0), totals)
        else:
            for i, (g, in_act) in enumerate(WGRAD_GROUPS[name]):
                run_wgrad_case(name, i, g, in_act, dt, dev, totals)
        for fam, c in totals.items():
            print_counters('%s counters of group %s' % (fam, name), c)
        print('  worst err/bound of group %s: %.3f' % (name, WORST[name]), flush=True)
    zero = zero_counters(coverage(False))
    assert not zero, 'counters that no shipped case exercises: %s' % zero
    print('conv small ok: %d checks, %d negative routes, groups %s (%s)' % (len(RESULTS), len(NEGATIVE), args.groups, sw), flush=True)


if __name__ == '__main__':
    main()
