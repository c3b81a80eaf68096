#!/usr/bin/env python3
"""The two generic convolution kernels -- csrc/conv_stream.hip (persistent stream-K, with its fix-up launch) and csrc/conv_igemm.hip
(implicit GEMM: three loaders, BN = 128 / 64 / 32, split-K with conv_finish_kernel, the stride-2 parity-class mode) -- against fp64,
element by element: forward convs and data gradients, k in {1, 3, 4}, stride 1 and 2, every epilogue.

Run by tests/test_conv_generic_fp64_gpu.py as a child process per environment, because the library reads its switches once per
process (S2E_CONV_STREAM, S2E_CONV_PATCH, S2E_CONV_DUO, S2E_IGEMM_GLDS, S2E_IGEMM_S2CLASS):

    python tests/_conv_generic_child.py --groups fwd_small,fwd_big,dgrad          (S2E_CONV_STREAM=2: the stream-K kernel)
    python tests/_conv_generic_child.py --groups fwd_small_f32,extra,subset       (S2E_CONV_STREAM=0: the implicit GEMM)
    python tests/_conv_generic_child.py --groups defaults                         (no switch: the shipped thresholds)
    python tests/_conv_generic_child.py --groups ... --plan                       (no GPU: routes and workspace sizes only)

Reference.  fp64 on the CPU (torch's conv2d / conv_transpose2d as the engine) from exactly what the kernel multiplies: bf16 or fp32
inputs as float64, weights rounded to the compute dtype as s2e_pack_conv_weight rounds them (RNE), fp32 bias as float64; with
in_act = LRELU the operand is the compute-dtype rounding of the fp32 product 0.2f * x (lrelu16 rounds it back before the MFMA).
Epilogue in the kernels' order: bias, residual, out_act (LeakyReLU or tanh), then the mask -- x1 / x0 (RELU_MASK) or x1 / x0.2
(LRELU_GRAD), decided by aux > 0.

Bound, per element:  |got - ref| <= rel |ref| + C_ACC * A,  rel = 2^-8 (bf16 outputs) or 2^-23 (fp32).  A is the same computation
on |x| and |w| plus |bias| and |residual|; LeakyReLU and tanh are 1-Lipschitz and pass it unchanged, the mask multiplies it.
C_ACC = 2^-16 is the constant of tests/_conv3x3_child.py, whose derivation holds for K <= 9216: every case here has K <= 9216.
Split-K and stream-K add one fp32 rounding of at most 2^-24 A per slab or slot that conv_finish_kernel / the fix-up kernel adds --
at most 64 of them here, a quarter of C_ACC if they all lined up, and the accumulation they replace is correspondingly shorter.

Guards.  y lives in a Guarded buffer and starts as NaN; the workspace is exactly s2e_conv2d_workspace_bytes long, NaN-poisoned and
guarded; every case is launched twice and the two results must be bit-identical (both kernels sum in a fixed order).

Route.  stream_plan() mirrors sk_fill_units / s2e_conv_stream_plan, igemm_plan() mirrors plan_splits; every case asserts that
s2e_conv2d_kernel_kind is GENERIC and that s2e_conv2d_workspace_bytes is what the mirror of the kernel it is written for says.
The mirrors also count what a case exercises (stream_counters, igemm_counters); with 256 CUs no counter over the shipped lists may be
zero.  Prints 'conv generic ok: ...' last."""
import argparse
import ctypes as C
import os
import sys
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch                                   # noqa: E402
import torch.nn.functional as F                # noqa: E402

from _conv3x3_child import BF16_RNE, C_ACC, GUARD, PATTERN, Guarded, check_close, workspace   # noqa: E402,F401

F32_RNE = 2.0 ** -23
K_MAX = 9216                                   # the derivation of C_ACC holds up to here
KERNEL_GENERIC = 0                             # S2E_KERNEL_GENERIC
ACT_NONE, ACT_LRELU, ACT_TANH = 0, 1, 2
AUX_NONE, AUX_RELU_MASK, AUX_LRELU_GRAD = 0, 1, 2
S2E_F32, S2E_BF16 = 0, 1
SWITCHES = ('S2E_CONV_STREAM', 'S2E_CONV_PATCH', 'S2E_CONV_DUO', 'S2E_IGEMM_GLDS', 'S2E_IGEMM_S2CLASS', 'S2E_DETERMINISTIC')

# N x H x W of the FORWARD conv's input, cin -> cout of the forward conv; dgrad: the launch is that conv's data gradient
Geo = namedtuple('Geo', 'N H W cin cout k s p dgrad')
Ep = namedtuple('Ep', 'bias res out_act aux in_act', defaults=(False, False, ACT_NONE, AUX_NONE, ACT_NONE))


def ceil_div(a, b):
    return -(-a // b)


def out_hw(g):
    """the forward conv's output map"""
    return (g.H + 2 * g.p - g.k) // g.s + 1, (g.W + 2 * g.p - g.k) // g.s + 1


def desc_fields(g, ep):
    """s2e_conv_desc of the launch: (N, Hi, Wi, Cin, Ho, Wo, Cout, KH, KW, stride, pad, transposed, in_act, out_act, aux_mode)"""
    ho, wo = out_hw(g)
    if g.dgrad:
        return (g.N, ho, wo, g.cout, g.H, g.W, g.cin, g.k, g.k, g.s, g.p, 1, ep.in_act, ep.out_act, ep.aux)
    return (g.N, g.H, g.W, g.cin, ho, wo, g.cout, g.k, g.k, g.s, g.p, 0, ep.in_act, ep.out_act, ep.aux)


def k_of(g):
    return g.k * g.k * (g.cout if g.dgrad else g.cin)


def geo_name(g):
    return '%dx%dx%d %d%s%d %dx%d/%d/%d' % (g.N, g.H, g.W, g.cin, '<-' if g.dgrad else '->', g.cout, g.k, g.k, g.s, g.p)


def ep_name(ep):
    parts = (['in-lrelu'] if ep.in_act else []) + (['bias'] if ep.bias else []) + (['res'] if ep.res else [])
    parts += {ACT_NONE: [], ACT_LRELU: ['lrelu'], ACT_TANH: ['tanh']}[ep.out_act]
    parts += {AUX_NONE: [], AUX_RELU_MASK: ['relu-mask'], AUX_LRELU_GRAD: ['lrelu-grad']}[ep.aux]
    return '+'.join(parts) or 'none'


# ---- plan mirrors
def env_flag(name, default=True):
    v = os.environ.get(name)
    if v is None:
        return default
    try:
        return int(v) != 0
    except ValueError:
        return False                                             # atoi of a non-number


def stream_plan(f, cus, mode=2):
    """sk_fill_units + s2e_conv_stream_plan (csrc/conv_stream.hip) for a bf16 descriptor; None: the kernel declines the shape.
    mode: S2E_CONV_STREAM (2 = every shape it can run, 1 = the shipped thresholds)."""
    N, Hi, Wi, Cin, Ho, Wo, Cout, KH, KW, stride, pad, tr, in_act, out_act, aux = f
    if mode <= 0 or Cin % 8 or Cout % 8 or Cout <= 32 or in_act != ACT_NONE:
        return None
    if KH * KW > 32 or out_act == ACT_TANH or (tr and stride == 2 and (KH < 2 or KW < 2)):
        return None
    kpad = ceil_div(KH * KW * Cin, 64) * 64
    bn = 128 if Cout > 64 else 64
    tiles_n = ceil_div(Cout, bn)
    if tr and stride == 2:                                       # per output-parity class: (K-steps per tile, tiles, K)
        cls = []
        for c in range(4):
            qy, qx = c >> 1, c & 1
            mq = N * ((Ho - qy + 1) // 2) * ((Wo - qx + 1) // 2)
            nky, nkx = (KH - ((qy + pad) & 1) + 1) >> 1, (KW - ((qx + pad) & 1) + 1) >> 1
            cls.append((max(1, ceil_div(nky * nkx * Cin, 64)), ceil_div(mq, 128) * tiles_n, nky * nkx * Cin))
    else:
        cls = [(kpad // 64, ceil_div(N * Ho * Wo, 128) * tiles_n, KH * KW * Cin)]
    units, tiles = sum(nk * t for nk, t, _ in cls), sum(t for _, t, _ in cls)
    if units >= (1 << 31) - 4096:
        return None
    G = max(1, min(units, cus))
    whole = all(nk == cls[0][0] for nk, _, _ in cls) and tiles >= 8 * G
    rq, rr, rmul = (tiles // G, tiles % G, cls[0][0]) if whole else (units // G, units % G, 1)
    cout_pad = ceil_div(Cout, bn) * bn
    if N * Hi * Wi * Cin * 2 >= (1 << 31) or cout_pad * kpad * 2 >= (1 << 31):
        return None
    if mode < 2 and (len(cls) > 1 or cls[0][0] < 16 or units // cls[0][0] < 64):
        return None
    return dict(kernel='stream', bn=bn, cls=cls, cls_nk=[c[0] for c in cls], units=units, tiles=tiles, G=G, rq=rq, rr=rr, rmul=rmul,
                whole_tiles=whole, workspace=0 if whole else 2 * G * 128 * bn * 4, fixup=(not whole) and G > 1)


STREAM_COUNTERS = ('tiles_cut_0', 'tiles_cut_1', 'tiles_cut_2', 'tiles_cut_3plus', 'ranges_inside_one_tile', 'ranges_head_tail_both_slots',
                   'ranges_head_whole_tail', 'ranges_head_whole', 'ranges_whole_tail', 'whole_tiles_with_remainder', 'G_eq_units', 'G_eq_1',
                   'class_launches_mixed_K', 'classes_padded_last_kstep', 'launches_with_fixup', 'launches_without_fixup')
IGEMM_COUNTERS = ('unsplit', 'unsplit_nk_lt_8', 'split_full_last', 'split_short_last', 's2_class', 's2_masked', 'bn128', 'bn64', 'bn32',
                  'loader_glds', 'loader_register', 'loader_gather', 'finish_vector', 'finish_scalar', 'epilogue_scalar')


def stream_counters(pl):
    """What one launch of the plan `pl` exercises: how the range boundaries cut its tiles, and the shapes of its ranges."""
    c = dict.fromkeys(STREAM_COUNTERS, 0)
    ends = np.cumsum(np.concatenate([np.full(t, nk, dtype=np.int64) for nk, t, _ in pl['cls']]))
    starts = ends - np.concatenate([np.full(t, nk, dtype=np.int64) for nk, t, _ in pl['cls']])
    i = np.arange(pl['G'] + 1, dtype=np.int64)
    b = (i * pl['rq'] + np.minimum(i, pl['rr'])) * pl['rmul']                     # sk_begin
    assert b[-1] == pl['units'] and bool((np.diff(b) > 0).all())
    cuts = np.searchsorted(b, ends, 'left') - np.searchsorted(b, starts, 'right')  # boundaries strictly inside a tile
    for name, n in (('tiles_cut_0', (cuts == 0).sum()), ('tiles_cut_1', (cuts == 1).sum()), ('tiles_cut_2', (cuts == 2).sum()),
                    ('tiles_cut_3plus', (cuts >= 3).sum())):
        c[name] = int(n)
    lo, hi = b[:-1], b[1:]
    first, last = np.searchsorted(ends, lo, 'right'), np.searchsorted(ends, hi - 1, 'right')
    nseg = last - first + 1
    head_p = ~((lo == starts[first]) & (hi >= ends[first]))                       # the first segment is not a whole tile
    tail_p = hi < ends[last]
    c['ranges_inside_one_tile'] = int(((nseg == 1) & head_p).sum())
    c['ranges_head_tail_both_slots'] = int(((nseg == 2) & head_p & tail_p).sum())
    c['ranges_head_whole_tail'] = int(((nseg >= 3) & head_p & tail_p).sum())
    c['ranges_head_whole'] = int(((nseg >= 2) & head_p & ~tail_p).sum())
    c['ranges_whole_tail'] = int(((nseg >= 2) & ~head_p & tail_p).sum())
    c['whole_tiles_with_remainder'] = int(pl['whole_tiles'] and pl['rr'] != 0)
    c['G_eq_units'] = int(pl['G'] == pl['units'])
    c['G_eq_1'] = int(pl['G'] == 1)
    c['class_launches_mixed_K'] = int(len(set(pl['cls_nk'])) > 1)
    c['classes_padded_last_kstep'] = sum(1 for nk, t, k in pl['cls'] if t and k % 64) if len(pl['cls']) > 1 else 0
    c['launches_with_fixup'] = int(pl['fixup'] and int((cuts > 0).sum()) > 0)
    c['launches_without_fixup'] = int(not c['launches_with_fixup'])
    return c


def igemm_plan(f, dtype, s2class_on=None, glds_on=None):
    """plan_splits + launch_conv (csrc/conv_igemm.hip): tiles, splits, K-tiles per split, workspace, loader, finish form."""
    N, Hi, Wi, Cin, Ho, Wo, Cout, KH, KW, stride, pad, tr, in_act, out_act, aux = f
    s2class_on = env_flag('S2E_IGEMM_S2CLASS') if s2class_on is None else s2class_on
    glds_on = env_flag('S2E_IGEMM_GLDS') if glds_on is None else glds_on
    vec, kt = (8, 64) if dtype == S2E_BF16 else (4, 32)
    bn = 128 if Cout > 64 else (64 if Cout > 32 else 32)
    M = N * Ho * Wo
    tiles_n = ceil_div(Cout, bn)
    tiles = ceil_div(M, 128) * tiles_n
    nk = ceil_div(KH * KW * Cin, kt)
    s2 = bool(s2class_on and glds_on and tr and stride == 2 and in_act == ACT_NONE and Cin % vec == 0 and KH >= 2 and KW >= 2)
    if s2:
        tiles = sum(ceil_div(N * ((Ho - (c >> 1) + 1) // 2) * ((Wo - (c & 1) + 1) // 2), 128) for c in range(4)) * tiles_n
        per, splits = nk, 1
    else:
        s = 1
        if tiles < 512 and nk >= 8:
            s = ceil_div(512, tiles)
            min_per = 16 if ((nk < 32 and tiles >= 256) or tiles <= 4) else 4
            s = max(1, min(s, nk // min_per))
        per = ceil_div(nk, s)
        splits = ceil_div(nk, per)
    loader = 'gather' if Cin % vec else ('glds' if (s2 or (glds_on and in_act == ACT_NONE)) else 'register')
    return dict(kernel='igemm', bn=bn, tiles=tiles, nk=nk, splits=splits, kt_per_split=per, s2_class=s2, loader=loader,
                masked_s2=bool(tr and stride == 2 and not s2), cvec=Cout % vec == 0,
                workspace=splits * M * Cout * 4 if splits > 1 else 0)


def igemm_counters(pl):
    c = dict.fromkeys(IGEMM_COUNTERS, 0)
    split = pl['splits'] > 1
    c['unsplit'] = int(not split)
    c['unsplit_nk_lt_8'] = int(not split and pl['nk'] < 8 and not pl['s2_class'])
    c['split_full_last'] = int(split and pl['nk'] % pl['kt_per_split'] == 0)
    c['split_short_last'] = int(split and pl['nk'] % pl['kt_per_split'] != 0)
    c['s2_class'], c['s2_masked'] = int(pl['s2_class']), int(pl['masked_s2'])
    c['bn%d' % pl['bn']] = 1
    c['loader_' + pl['loader']] = 1
    c['finish_vector'], c['finish_scalar'] = int(split and pl['cvec']), int(split and not pl['cvec'])
    c['epilogue_scalar'] = int(not split and not pl['cvec'])
    return c


def add_counters(total, c):
    for k, v in c.items():
        total[k] = total.get(k, 0) + v
    return total


# ---- fp64 reference (CPU)
def conv64(x, w, k, s, p, transposed, hw_out):
    """The convolution (transposed: the data gradient / transposed convolution) of NHWC x with the FORWARD conv's OIHW weight w, in
    the dtype of its arguments: forward (N, H, W, Ci) -> (N, Ho, Wo, Co); transposed (N, Hg, Wg, Co) -> (N, hw_out, Ci)."""
    xn = x.permute(0, 3, 1, 2)
    if not transposed:
        y = F.conv2d(xn, w, stride=s, padding=p)
    else:
        oph = hw_out[0] - ((x.shape[1] - 1) * s - 2 * p + k)
        opw = hw_out[1] - ((x.shape[2] - 1) * s - 2 * p + k)
        assert 0 <= oph < max(s, 2) and 0 <= opw < max(s, 2), 'not the data gradient of a conv with this geometry'
        y = F.conv_transpose2d(xn, w, stride=s, padding=p, output_padding=(oph, opw))
    y = y.permute(0, 2, 3, 1).contiguous()
    assert tuple(y.shape[1:3]) == tuple(hw_out), (tuple(y.shape), hw_out)
    return y


def operand64(x, in_act, dtype):
    """what the MFMA multiplies for the stored input x: x itself, or LeakyReLU(0.2) of it rounded back to the compute dtype"""
    if in_act == ACT_NONE:
        return x.double()
    assert in_act == ACT_LRELU
    xf = x.float()
    return torch.where(xf > 0, xf, xf * 0.2).to(dtype).double()              # (0.2f * x in fp32, then RNE)


def weight64(w, dtype):
    return w.float().to(dtype).double()


def conv_pair(x, w, g, in_act, dtype):
    """(convolution, the same of absolute values) for the launch of geometry g"""
    hw = (g.H, g.W) if g.dgrad else out_hw(g)
    xo, wq = operand64(x, in_act, dtype), weight64(w, dtype)
    return conv64(xo, wq, g.k, g.s, g.p, g.dgrad, hw), conv64(xo.abs(), wq.abs(), g.k, g.s, g.p, g.dgrad, hw)


def mask64(aux, mode):
    pos = aux.double() > 0
    if mode == AUX_RELU_MASK:
        return torch.where(pos, 1.0, 0.0).double()
    if mode == AUX_LRELU_GRAD:
        return torch.where(pos, 1.0, 0.2).double()
    return None


def epilogue64(conv, a0, bias, res, aux, ep):
    """bias, residual, out_act, mask -- and the absolute-value twin: returns (ref, A)"""
    ref, A = conv.clone(), a0.clone()
    if ep.bias:
        ref += bias.double()
        A += bias.double().abs()
    if ep.res:
        ref += res.double()
        A += res.double().abs()
    if ep.out_act == ACT_LRELU:
        ref = torch.where(ref > 0, ref, 0.2 * ref)
    elif ep.out_act == ACT_TANH:
        ref = torch.tanh(ref)
    m = mask64(aux, ep.aux)
    if m is not None:
        ref, A = ref * m, A * m
    return ref, A


def reference(x, w, bias, res, aux, g, ep, dtype):
    conv, a0 = conv_pair(x, w, g, ep.in_act, dtype)
    return epilogue64(conv, a0, bias, res, aux, ep)


def operands(g, dtype, seed):
    """CPU tensors of a case: x (the launch's input: the forward input, or the output gradient), the forward OIHW weight (fp32),
    bias (fp32), residual and mask operand (output shape, storage dtype; the mask operand has exact zeros and negative zeros)"""
    gen = torch.Generator().manual_seed(seed)
    ho, wo = out_hw(g)
    xs, ys = ((g.N, ho, wo, g.cout), (g.N, g.H, g.W, g.cin)) if g.dgrad else ((g.N, g.H, g.W, g.cin), (g.N, ho, wo, g.cout))
    x = torch.randn(*xs, generator=gen).to(dtype)
    w = torch.randn(g.cout, g.cin, g.k, g.k, generator=gen) * float(k_of(g)) ** -0.5
    bias = torch.randn(ys[-1], generator=gen) * 0.5
    res = (torch.randn(*ys, generator=gen) * 0.7 + 0.2).to(dtype)
    aux = torch.randn(*ys, generator=gen)
    aux = torch.where(aux.abs() < 0.1, torch.zeros_like(aux) * aux.sign(), aux).to(dtype)
    return x, w, bias, res, aux


# ---- the cases: (geometry, [epilogues])
E = Ep
FWD_SMALL = [
    (Geo(1, 8, 8, 64, 40, 3, 1, 1, False), [E(bias=True, res=True, out_act=ACT_LRELU), E(aux=AUX_RELU_MASK)]),
    (Geo(2, 16, 16, 264, 136, 3, 1, 1, False), [E(bias=True), E(res=True, aux=AUX_LRELU_GRAD), E(out_act=ACT_LRELU)]),
    (Geo(1, 10, 12, 8, 40, 1, 1, 0, False), [E(), E(bias=True, res=True), E(bias=True, out_act=ACT_LRELU), E(aux=AUX_RELU_MASK),
                                             E(aux=AUX_LRELU_GRAD), E(res=True, aux=AUX_RELU_MASK)]),
    (Geo(3, 33, 35, 64, 136, 4, 2, 2, False), [E(bias=True, out_act=ACT_LRELU), E(res=True)]),
    (Geo(2, 17, 17, 256, 512, 4, 1, 2, False), [E(bias=True), E(bias=True, res=True, aux=AUX_RELU_MASK)]),
]
FWD_BIG = [
    (Geo(3, 173, 173, 128, 64, 1, 1, 0, False), [E(), E(bias=True, res=True, out_act=ACT_LRELU)]),
    (Geo(2, 161, 179, 16, 40, 3, 1, 1, False), [E(bias=True, aux=AUX_LRELU_GRAD), E(res=True)]),
    (Geo(4, 260, 259, 8, 64, 1, 1, 0, False), [E(bias=True, res=True, out_act=ACT_LRELU), E(res=True, aux=AUX_LRELU_GRAD)]),
]
DGRAD = [
    (Geo(2, 9, 9, 64, 32, 4, 1, 2, True), [E(), E(aux=AUX_RELU_MASK)]),
    (Geo(2, 15, 22, 40, 24, 4, 2, 2, True), [E(aux=AUX_LRELU_GRAD), E(bias=True)]),
    (Geo(3, 33, 31, 72, 136, 3, 2, 1, True), [E(), E(res=True, aux=AUX_RELU_MASK)]),
    (Geo(4, 65, 63, 64, 72, 4, 2, 2, True), [E(aux=AUX_RELU_MASK), E(res=True)]),
    (Geo(6, 66, 61, 40, 24, 3, 2, 1, True), [E(aux=AUX_LRELU_GRAD), E(bias=True, out_act=ACT_LRELU)]),
]
# the shipped thresholds send these to stream-K: >= 16 K-steps per tile, >= 64 tiles, no classes
DEFAULTS = [
    (Geo(2, 64, 64, 64, 64, 4, 1, 2, False), [E(bias=True, out_act=ACT_LRELU)]),
    (Geo(2, 33, 33, 1024, 520, 1, 1, 0, False), [E(bias=True, res=True)]),
]
# implicit GEMM only: BN = 32 with the scalar epilogue and the scalar finish, the gather loader, the register-staged loader, tanh
EXTRA = [
    (Geo(5, 13, 11, 64, 5, 3, 1, 1, False), [E(bias=True, out_act=ACT_TANH), E(bias=True, res=True, aux=AUX_LRELU_GRAD)]),
    (Geo(5, 13, 11, 64, 20, 3, 1, 1, False), [E(bias=True, res=True), E(aux=AUX_RELU_MASK)]),
    (Geo(2, 13, 11, 64, 32, 3, 1, 1, False), [E(bias=True, out_act=ACT_LRELU)]),
    (Geo(3, 19, 23, 8, 20, 3, 2, 1, False), [E(bias=True, res=True, out_act=ACT_TANH, aux=AUX_RELU_MASK)]),      # unsplit, scalar epilogue
    (Geo(2, 19, 23, 5, 24, 3, 1, 1, False), [E(bias=True, out_act=ACT_LRELU), E(in_act=ACT_LRELU)]),
    (Geo(2, 19, 23, 1, 24, 4, 2, 2, False), [E(bias=True)]),
    (Geo(2, 19, 23, 24, 5, 3, 2, 1, True), [E(aux=AUX_RELU_MASK)]),                                              # transposed gather
    (Geo(2, 16, 16, 264, 136, 3, 1, 1, False), [E(bias=True, in_act=ACT_LRELU)]),
    (Geo(3, 33, 35, 64, 136, 4, 2, 2, False), [E(in_act=ACT_LRELU, out_act=ACT_LRELU)]),
    (Geo(1, 8, 8, 64, 40, 3, 1, 1, False), [E(bias=True, out_act=ACT_TANH)]),
]
# repeated under S2E_IGEMM_S2CLASS=0 (masked all-taps walk, may split) and S2E_IGEMM_GLDS=0 (register-staged loader)
SUBSET = [DGRAD[1], DGRAD[2], DGRAD[3], FWD_SMALL[0], FWD_SMALL[1], EXTRA[1]]
SUBSET_F32 = [DGRAD[1], DGRAD[2], FWD_SMALL[1], EXTRA[1]]

STREAM_GROUPS = {'fwd_small': FWD_SMALL, 'fwd_big': FWD_BIG, 'dgrad': DGRAD}
DEFAULT_GROUPS = {'defaults': DEFAULTS}
IGEMM_GROUPS = {'fwd_small': FWD_SMALL, 'fwd_big': FWD_BIG, 'dgrad': DGRAD, 'extra': EXTRA, 'subset': SUBSET,
                'fwd_small_f32': FWD_SMALL, 'fwd_big_f32': FWD_BIG, 'dgrad_f32': DGRAD, 'extra_f32': EXTRA, 'subset_f32': SUBSET_F32}


def group_dtype(name):
    return torch.float32 if name.endswith('_f32') else torch.bfloat16


def route_of_env(env=None):
    """which kernel the cases of this process are written for, from S2E_CONV_STREAM: 'stream' (2), 'igemm' (0), 'defaults' (unset)"""
    v = (os.environ if env is None else env).get('S2E_CONV_STREAM')
    return {None: 'defaults', '2': 'stream', '0': 'igemm'}[v]


def groups_of(route):
    return {'stream': STREAM_GROUPS, 'igemm': IGEMM_GROUPS, 'defaults': DEFAULT_GROUPS}[route]


def plan_of(route, f, dt, cus, s2class_on=None, glds_on=None):
    """the mirror of the kernel a case of `route` is written for; None: that kernel declines the case (the case is wrong)"""
    if route == 'igemm':
        return igemm_plan(f, dt, s2class_on, glds_on)
    return stream_plan(f, cus, 2 if route == 'stream' else 1) if dt == S2E_BF16 else None


def coverage(cus):
    """the counters summed over the shipped lists: (stream-K over STREAM_GROUPS, implicit GEMM over IGEMM_GROUPS with and without
    the class mode / LDS-DMA for the subsets)"""
    sc, ic = dict.fromkeys(STREAM_COUNTERS, 0), dict.fromkeys(IGEMM_COUNTERS, 0)
    for cases in STREAM_GROUPS.values():
        for g, eps in cases:
            for ep in eps:
                add_counters(sc, stream_counters(stream_plan(desc_fields(g, ep), cus, 2)))
    for name, cases in IGEMM_GROUPS.items():
        dt = S2E_F32 if name.endswith('_f32') else S2E_BF16
        for g, eps in cases:
            for ep in eps:
                f = desc_fields(g, ep)
                add_counters(ic, igemm_counters(igemm_plan(f, dt, True, True)))
                if name.startswith('subset'):
                    add_counters(ic, igemm_counters(igemm_plan(f, dt, False, True)))
                    add_counters(ic, igemm_counters(igemm_plan(f, dt, True, False)))
    return sc, ic


def kernel_label(pl):
    if pl['kernel'] == 'stream':
        return 'stream-bn%d G=%d%s' % (pl['bn'], pl['G'], ' whole-tiles' if pl['whole_tiles'] else (' +fixup' if pl['fixup'] else ''))
    return 'igemm-bn%d-%s%s%s' % (pl['bn'], pl['loader'], '-s2class' if pl['s2_class'] else '',
                                  ' splits=%d' % pl['splits'] if pl['splits'] > 1 else '')


# ---- the library
def lib():
    from seg2eye_amd import _lib as L
    return L, L.lib()


def make_desc(f):
    L, _ = lib()
    return L.ConvDesc(*f)


def check_route(route, g, ep, dt, cus):
    """kernel kind and workspace of the library against the mirror; returns (plan, workspace bytes)"""
    L, lb = lib()
    f = desc_fields(g, ep)
    what = '%s %s' % (geo_name(g), ep_name(ep))
    assert k_of(g) <= K_MAX, '%s: K = %d is past the derivation of C_ACC' % (what, k_of(g))
    pl = plan_of(route, f, dt, cus)
    assert pl is not None, '%s: the %s kernel declines this case' % (what, route)
    d = make_desc(f)
    kind = lb.s2e_conv2d_kernel_kind(dt, C.byref(d))
    assert kind == KERNEL_GENERIC, '%s: kernel kind %d, the case is written for the generic kernels' % (what, kind)
    wsb = int(lb.s2e_conv2d_workspace_bytes(dt, C.byref(d)))
    assert wsb == pl['workspace'], '%s: the library asks for %d bytes of workspace, the %s mirror says %d' % (what, wsb, pl['kernel'], pl['workspace'])
    return pl, wsb


RESULTS = []
WORST = {}


def run_case(group, route, g, eps, dtype, dev, seed, cus, totals):
    L, lb = lib()
    from seg2eye_amd import ops
    dt = S2E_BF16 if dtype == torch.bfloat16 else S2E_F32
    rel = BF16_RNE if dtype == torch.bfloat16 else F32_RNE
    x, w, bias, res, aux = operands(g, dtype, seed)
    xd, bd, resd, auxd = x.to(dev), bias.to(dev), res.to(dev), aux.to(dev)
    wp = ops.pack_weight(w.to(dev), dtype, g.cin, g.dgrad)
    pairs = {}
    yshape = tuple(res.shape)
    stream = torch.cuda.current_stream().cuda_stream
    for ep in eps:
        what = '%s %s %s' % ('bf16' if dt == S2E_BF16 else 'f32', geo_name(g), ep_name(ep))
        pl, wsb = check_route(route, g, ep, dt, cus)
        add_counters(totals, stream_counters(pl) if pl['kernel'] == 'stream' else igemm_counters(pl))
        if ep.in_act not in pairs:
            pairs[ep.in_act] = conv_pair(x, w, g, ep.in_act, dtype)
        ref, A = epilogue64(pairs[ep.in_act][0], pairs[ep.in_act][1], bias, res, aux, ep)
        d = make_desc(desc_fields(g, ep))
        outs = []
        for rep in range(2):
            y = Guarded(yshape, dtype, dev, float('nan'))
            ws = workspace(wsb, dev)
            L.check(lb.s2e_conv2d(dt, xd.data_ptr(), wp.data_ptr(), bd.data_ptr() if ep.bias else None, resd.data_ptr() if ep.res else None,
                                  auxd.data_ptr() if ep.aux != AUX_NONE else None, y.ptr(), C.byref(d), ws.ptr(), wsb, stream), 's2e_conv2d')
            y.check('%s y (launch %d)' % (what, rep))
            ws.check('%s workspace (launch %d)' % (what, rep))
            outs.append(y.t.clone())
        worst = check_close(outs[0], ref, A, what, rel=rel)
        assert torch.equal(outs[0].view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                           outs[1].view(torch.int16 if dtype == torch.bfloat16 else torch.int32)), '%s: two launches differ' % what
        WORST[group] = max(WORST.get(group, 0.0), worst)
        line = '  %-13s %-58s kernel=%-34s ws=%-9d worst err/bound %.3f' % (group, what, kernel_label(pl), wsb, worst)
        RESULTS.append(line)
        print(line, flush=True)


def plan_only(route, names, cus):
    """--plan: every case's route and workspace against the mirror, on the library alone (no GPU)"""
    n = 0
    for name in names:
        dt = S2E_F32 if name.endswith('_f32') else S2E_BF16
        for g, eps in groups_of(route)[name]:
            for ep in eps:
                check_route(route, g, ep, dt, cus)
                n += 1
    return n


def library_cus():
    """The CU count the library plans with, from a shape stream-K takes under every setting that has it on: bf16 1x1 1024 -> 1024 at
    32 x 32 asks for two 128 x 128 fp32 partial tiles per CU.  With stream-K off nothing here depends on the count."""
    _, lb = lib()
    d = make_desc((1, 32, 32, 1024, 32, 32, 1024, 1, 1, 1, 0, 0, 0, 0, 0))
    ws = int(lb.s2e_conv2d_workspace_bytes(S2E_BF16, C.byref(d)))
    return ws // (2 * 128 * 128 * 4) if route_of_env() != 'igemm' else 256


def print_counters(title, c):
    print('  %s: %s' % (title, ', '.join('%s=%d' % kv for kv in c.items())), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--groups', required=True)
    ap.add_argument('--plan', action='store_true', help='routes and workspace sizes only, without a GPU')
    args = ap.parse_args()
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    names = args.groups.split(',')
    route = route_of_env()
    lib()
    sw = ' '.join('%s=%s' % (k, os.environ[k]) for k in SWITCHES if k in os.environ) or 'defaults'
    if args.plan:
        cus = library_cus()
        n = plan_only(route, names, cus)
        print('conv generic plan ok: %d cases, groups %s, %d CUs (%s)' % (n, args.groups, cus, sw), flush=True)
        return
    dev = torch.device('cuda', 0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for name in names:
        totals = {}
        for i, (g, eps) in enumerate(groups_of(route)[name]):
            run_case(name, route, g, eps, group_dtype(name), dev, 1000 + 37 * i + (500 if name.endswith('_f32') else 0), cus, totals)
        print_counters('counters of group %s' % name, totals)
        print('  worst err/bound of group %s: %.3f' % (name, WORST[name]), flush=True)
    sc, ic = coverage(cus)
    print_counters('stream-K counters over the shipped lists at %d CUs' % cus, sc)
    print_counters('implicit-GEMM counters over the shipped lists', ic)
    if cus == 256:
        zero = [k for k, v in list(sc.items()) + list(ic.items()) if v == 0]
        assert not zero, 'counters that no shipped case exercises: %s' % zero
    else:
        print('  %d CUs, not 256: the coverage counters are printed, not asserted' % cus, flush=True)
    print('conv generic ok: %d checks, groups %s (%s)' % (len(RESULTS), args.groups, sw), flush=True)


if __name__ == '__main__':
    main()
