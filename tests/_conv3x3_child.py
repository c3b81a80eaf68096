#!/usr/bin/env python3
"""The bf16 3x3 stride-1 convolution kernels -- csrc/conv_duo.hip (forward, data gradient, fused SPADE), csrc/conv_patch.hip (the
same shapes with the duo plan off) and csrc/conv_wgrad_patch.hip (weight gradient) -- against fp64, element by element.

Run by tests/test_conv3x3_fp64_gpu.py as a child process per environment, because the library reads its switches once per process
(S2E_CONV_DUO, S2E_CONV_PATCH, S2E_SPADE_FUSED_TILES, S2E_DUO_MF16, S2E_WGRAD_PATCH, S2E_DETERMINISTIC):

    python tests/_conv3x3_child.py --groups fwd,dgrad,rects,fused,fused_lists,cap,bench,wgrad,wgrad_rects,wgrad_det

Reference.  fp64 on the CPU from exactly the values the kernel sees: bf16 inputs / residual / mask operand, weights rounded to bf16 as
s2e_pack_conv_weight rounds them (RNE), fp32 bias / statistics / style as float64.

Bound, per element of a bf16 output (y, dx, the fused `out`, the stored gamma):
    |got - ref| <= 2^-8 |ref| + C_ACC * A
2^-8 |ref| is the RNE rounding of the fp32 result to bf16.  A is the same computation on absolute values -- the convolution of |x|
with |w|, plus |bias| and |residual|, through the epilogue -- so that every fp32 partial sum and every epilogue intermediate is at most
A in magnitude.  C_ACC = 2^-16 (256 fp32 ulps) covers the fp32 accumulation: products of bf16 operands are exact in fp32, a K-step adds
16 or 32 of them into an accumulator (one rounding of at most 2^-24 A), and K = 9 Cin <= 9216 makes at most 576 such roundings per
element -- whose random-walk sum is ~24 x 2^-24 A, a tenth of the allowance; the epilogue adds a handful more.  A wrong tap, channel,
constant or rectangle is off by about one term, i.e. by ~A / sqrt(K) >> 2^-16 A.  fp32 weight / bias gradients: C_ACC * (A_w + |start|),
A_w the fp64 weight gradient of |x| and |gy|.  InstanceNorm partial sums: the slots of a (sample, channel) summed in fp64 against the
fp64 sums of the STORED bf16 y, within C_ACC of the sums of |y| and y^2.

Guards.  Every output lives inside one byte tensor with GUARD bytes of PATTERN on both sides that must come back unchanged; outputs
the call overwrites and every workspace start as NaN (the library says workspaces need no initialisation); accumulated outputs start
non-zero; list forms start as SENTINEL outside the listed rectangles, which must stay bit-identical.  Prints 'conv3x3 ok: ...' last."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch                                   # noqa: E402
import torch.nn.functional as F                # noqa: E402

C_ACC = 2.0 ** -16                             # fp32 accumulation allowance, x A (see above)
BF16_RNE = 2.0 ** -8                           # RNE rounding of a bf16 result, x |ref|
GUARD = 1 << 18                                # bytes of PATTERN on each side of every output and workspace
PATTERN = 0xA5
SENTINEL = -77.0                               # bf16-exact; what a list form must leave outside its rectangles
KERNEL_PATCH = 2                               # S2E_KERNEL_PATCH
DUO_DEFAULT_MIN_ITEMS = 256                    # duo_min_items() of conv_duo.hip without S2E_CONV_DUO


def env_int(name, default):
    v = os.environ.get(name)
    return int(v) if v is not None else default


def duo_min_items():
    return env_int('S2E_CONV_DUO', DUO_DEFAULT_MIN_ITEMS)


def mf16_on():
    return env_int('S2E_DUO_MF16', 1) != 0


def duo_takes_fused(N, H, W, C_, nh, flags, tw, th):
    """The rule of s2e_spade_conv_modulate_duo (csrc/conv_duo.hip:882-888): whether the duo kernel runs a fused launch that
    s2e_spade_conv_modulate has planned with tw x th rectangles (else conv_patch.hip's fused kernel runs it)."""
    from seg2eye_amd._lib import SPADE_ANY_TILES
    if duo_min_items() <= 0 or nh % 32 != 0 or C_ % 64 != 0 or (flags & SPADE_ANY_TILES):
        return False
    if not (tw == 16 and th == 16 and H % 16 == 0 and W % 16 == 0):           # duo_rect_ok
        return False
    if N * (H // th) * (W // tw) * (C_ // 64) < duo_min_items():
        return False
    return N * H * W * nh * 2 < (1 << 31) and N * H * W * C_ * 2 < (1 << 31)


def wgrad_slab(H, W):
    """The slab width s2e_wgrad_patch_plan picks (csrc/conv_wgrad_patch.hip): the best-filling of 64 x 2, 32 x 4, 16 x 8."""
    best, best_fill = 0, 0.0
    for tw in (64, 32, 16):
        th = 128 // tw
        fill = H * W / float(-(-H // th) * th * -(-W // tw) * tw)
        if fill > best_fill + 1e-9:
            best, best_fill = tw, fill
    return best if best_fill >= 0.8 else 0


# ---- fp64 references (CPU)
def conv3x3_64(x, w):
    """3x3 stride-1 pad-1 convolution in fp64: x (N, H, W, Ci), w (Co, Ci, 3, 3), both float64 on the CPU -> (N, H, W, Co)."""
    n, h, wd, ci = x.shape
    co = w.shape[0]
    wm = w.permute(2, 3, 1, 0).reshape(9 * ci, co)              # rows (ky, kx, ci)
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    out = torch.empty(n, h, wd, co, dtype=torch.float64)
    rows = max(1, (1 << 22) // (wd * 9 * ci))                   # <= 32 MB of im2col at a time
    for b in range(n):
        for y0 in range(0, h, rows):
            y1 = min(h, y0 + rows)
            cols = torch.cat([xp[b, y0 + ky:y1 + ky, kx:kx + wd] for ky in range(3) for kx in range(3)], dim=-1)
            out[b, y0:y1] = (cols.reshape(-1, 9 * ci) @ wm).view(y1 - y0, wd, co)
    return out


def dgrad3x3_64(gy, w):
    """Data gradient of the forward conv with weight w (Co, Ci, 3, 3): gy (N, H, W, Co) -> dx (N, H, W, Ci)."""
    return conv3x3_64(gy, w.flip(2, 3).transpose(0, 1))


def wgrad3x3_64(x, gy):
    """Weight gradient in the library's layout: (Co, 9 Ci), columns (ky, kx, ci)."""
    n, h, wd, ci = x.shape
    co = gy.shape[-1]
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    g = gy.reshape(-1, co).t().contiguous()
    out = torch.empty(co, 9, ci, dtype=torch.float64)
    for t in range(9):
        ky, kx = divmod(t, 3)
        out[:, t] = g @ xp[:, ky:ky + h, kx:kx + wd].reshape(-1, ci)
    return out.reshape(co, 9 * ci)


def lrelu(v):
    return torch.where(v > 0, v, 0.2 * v)


def rect_mask(n, h, w, ids):
    """(n, h, w, 1) bool: the pixels of the 16 x 16 rectangles `ids` (r = (n * h/16 + ty) * w/16 + tx)."""
    m = torch.zeros(n * (h // 16) * (w // 16), dtype=torch.bool)
    if len(ids):
        m[torch.as_tensor(ids, dtype=torch.long)] = True
    return m.view(n, h // 16, w // 16).repeat_interleave(16, 1).repeat_interleave(16, 2).unsqueeze(-1)


def fused_ref(actv, wq, bias, x_full, stats, s0, s1, lrelu_on):
    """SPADE + Style modulation after the [gamma | beta] conv, in fp64, and its absolute-value twin:
    returns (out, A_out, gamma, A_gamma)."""
    C_ = x_full.shape[-1]
    gb = conv3x3_64(actv, wq)
    ab = conv3x3_64(actv.abs(), wq.abs())
    b = bias if bias is not None else torch.zeros(2 * C_, dtype=torch.float64)
    gamma, beta = gb[..., :C_] + b[:C_], gb[..., C_:] + b[C_:]
    mean, rstd = stats[:, None, None, :, 0], stats[:, None, None, :, 1]
    s0_, s1_ = s0[:, None, None, :], s1[:, None, None, :]
    out = 0.5 * ((x_full - mean) * rstd * (1 + gamma) + beta + x_full * (1 + s0_) + s1_)
    a_gamma = 1 + b[:C_].abs() + ab[..., :C_]
    a_out = 0.5 * ((x_full.abs() + mean.abs()) * rstd * a_gamma + b[C_:].abs() + ab[..., C_:] + x_full.abs() * (1 + s0_.abs()) + s1_.abs())
    if lrelu_on:
        out = lrelu(out)
    return out, a_out, gamma, a_gamma


# ---- the library
def lib():
    from seg2eye_amd import _lib as L
    return L, L.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """A tensor of `shape` / `dtype` inside one byte allocation with GUARD bytes of PATTERN on both sides."""

    def __init__(self, shape, dtype, dev, fill=None, raw_fill=None):
        numel = 1
        for s in shape:
            numel *= s
        self.nbytes = numel * torch.tensor([], dtype=dtype).element_size()
        self.raw = torch.full((2 * GUARD + self.nbytes,), PATTERN, dtype=torch.uint8, device=dev)
        body = self.raw[GUARD:GUARD + self.nbytes]
        if raw_fill is not None:
            body.fill_(raw_fill)
        self.t = body.view(dtype).view(*shape) if self.nbytes else body
        if fill is not None:
            if torch.is_tensor(fill):
                self.t.copy_(fill)
            else:
                self.t.fill_(fill)

    def ptr(self):
        return self.t.data_ptr() if self.nbytes else None

    def check(self, what):
        torch.cuda.synchronize()
        lo = int((self.raw[:GUARD] != PATTERN).sum())
        hi = int((self.raw[GUARD + self.nbytes:] != PATTERN).sum())
        assert lo == 0 and hi == 0, '%s: %d guard bytes before and %d after the %d-byte buffer were written' % (what, lo, hi, self.nbytes)


def workspace(nbytes, dev):
    """NaN-poisoned workspace (every fp32 word 0xFFFFFFFF) inside a guard band"""
    return Guarded((nbytes,), torch.uint8, dev, raw_fill=0xFF)


def check_close(got, ref, A, what, rel=BF16_RNE, start=None):
    """Every element: |got - (start +) ref| <= rel |ref| + C_ACC A (NaN fails).  Returns the worst error / bound."""
    g = got.detach().double().cpu()
    if start is not None:
        g = g - start
    assert float(A.max()) > 0, '%s: empty reference' % what
    bound = rel * ref.abs() + C_ACC * A
    err = (g - ref).abs()
    ok = err <= bound
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError('%s: %d of %d elements outside the bound; first at %s: got %r, ref %r, A %r, bound %.3e'
                             % (what, bad.shape[0], ok.numel(), i, float(g[i]), float(ref[i]), float(A[i]), float(bound[i])))
    return float((err / bound.clamp_min(1e-300)).max())


def check_sentinel(got, keep, what):
    """Outside the listed rectangles (keep == False) the output must still hold SENTINEL, bit for bit."""
    g = got.detach().cpu()
    sent = torch.full_like(g, SENTINEL)
    outside = (~keep).expand_as(g)
    diff = (g.view(torch.int16) != sent.view(torch.int16)) & outside
    n = int(diff.sum())
    assert n == 0, '%s: %d elements outside the listed rectangles changed (first at %s)' % (what, n, tuple(int(v) for v in diff.nonzero()[0]))


def desc(N, H, W, cin, cout, transposed=0, out_act=0, aux_mode=0):
    L, _ = lib()
    return L.ConvDesc(N, H, W, cin, H, W, cout, 3, 3, 1, 1, transposed, 0, out_act, aux_mode)


def cap():
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count


def items_of(N, H, W, cout):
    return N * (H // 16) * (W // 16) * (1 if cout <= 64 else -(-cout // 128))


def rel_cap(items):
    if items is None:
        return '-'
    c = cap()
    d = items - c if items < 2 * c else items - 2 * c
    return '%d = %s%+d' % (items, 'cap' if items < 2 * c else '2*cap', d) if abs(d) < 16 else '%d (cap %d)' % (items, c)


def conv_kernel(d, fused=False):
    """Which kernel the library runs for a plain / data-gradient descriptor, asserted against the switches of this process."""
    L, lb = lib()
    duo = lb.s2e_conv2d_rects_supported(L.S2E_BF16, C.byref(d)) == 1
    if duo:
        return 'duo-bn64' if d.Cout <= 64 else ('duo-mf16' if mf16_on() else 'duo-mf32')
    assert lb.s2e_conv2d_kernel_kind(L.S2E_BF16, C.byref(d)) == KERNEL_PATCH, 'not a patch-resident shape'
    return 'patch'


def expect_kernel(d, want, what):
    k = conv_kernel(d)
    family = 'duo' if k.startswith('duo') else k
    assert family == want, '%s: ran in %s, the case is written for %s' % (what, k, want)
    return k


RESULTS = []


def report(group, name, kernel, items, worst):
    line = '  %-11s %-44s kernel=%-14s items=%-22s worst err/bound %.3f' % (group, name, kernel, rel_cap(items), worst)
    RESULTS.append(line)
    print(line, flush=True)


def rnd(shape, g, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=g) * scale + shift


# ---- forward: every epilogue, and the statistics forms
EPILOGUES = [  # (name, bias, residual, LeakyReLU)
    ('none', False, False, False), ('bias', True, False, False), ('bias+res', True, True, False),
    ('bias+lrelu', True, False, True), ('bias+res+lrelu', True, True, True)]


def run_forward(group, N, H, W, cin, cout, want, dev, seed, epilogues=EPILOGUES, stats=True):
    L, lb = lib()
    from seg2eye_amd import ops
    g = torch.Generator().manual_seed(seed)
    x = rnd((N, H, W, cin), g).to(torch.bfloat16)
    w = rnd((cout, cin, 3, 3), g, (cin * 9) ** -0.5)
    b = rnd((cout,), g, 0.5)
    res = rnd((N, H, W, cout), g, 0.7, 0.2).to(torch.bfloat16)
    wq = w.to(torch.bfloat16).double()
    x64 = x.double()
    conv = conv3x3_64(x64, wq)
    A0 = conv3x3_64(x64.abs(), wq.abs())
    res64, b64 = res.double(), b.double()
    xd, wp, bd, resd = x.to(dev), ops.pack_weight(w.to(dev), torch.bfloat16, cin, False), b.to(dev), res.to(dev)
    shape = '%dx%dx%dx%d->%d' % (N, H, W, cin, cout)
    for name, with_b, with_r, with_l in epilogues:
        d = desc(N, H, W, cin, cout, out_act=L.ACT_LRELU if with_l else L.ACT_NONE)
        k = expect_kernel(d, want, shape)
        ref, A = conv.clone(), A0.clone()
        if with_b:
            ref += b64
            A += b64.abs()
        if with_r:
            ref += res64
            A += res64.abs()
        if with_l:
            ref = lrelu(ref)
        y = Guarded((N, H, W, cout), torch.bfloat16, dev, float('nan'))
        wsb = int(lb.s2e_conv2d_workspace_bytes(L.S2E_BF16, C.byref(d)))
        ws = workspace(wsb, dev)
        L.check(lb.s2e_conv2d(L.S2E_BF16, xd.data_ptr(), wp.data_ptr(), bd.data_ptr() if with_b else None,
                              resd.data_ptr() if with_r else None, None, y.ptr(), C.byref(d), ws.ptr(), wsb, stream()), 's2e_conv2d')
        y.check('%s %s y' % (shape, name))
        ws.check('%s %s workspace' % (shape, name))
        worst = check_close(y.t, ref, A, 'forward %s %s' % (shape, name))
        report(group, 'fwd %s %s' % (shape, name), k + ('+ws' if wsb else ''), items_of(N, H, W, cout), worst)
    if not stats:
        return
    d = desc(N, H, W, cin, cout)
    slots = int(lb.s2e_conv2d_stats_slots(L.S2E_BF16, C.byref(d)))
    if want != 'duo':
        assert slots == 0, '%s: the statistics epilogue is a duo-kernel form' % shape
        return
    assert slots > 0, '%s: no statistics epilogue for a duo shape' % shape
    for with_r in (False, True):
        name = 'stats' + ('+res' if with_r else '')
        k = expect_kernel(d, want, shape)
        ref, A = conv + b64, A0 + b64.abs()
        if with_r:
            ref += res64
            A += res64.abs()
        y = Guarded((N, H, W, cout), torch.bfloat16, dev, float('nan'))
        part = Guarded((N, slots, cout, 2), torch.float32, dev, float('nan'))
        L.check(lb.s2e_conv2d_stats(L.S2E_BF16, xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), resd.data_ptr() if with_r else None, y.ptr(),
                                    C.byref(d), part.ptr(), stream()), 's2e_conv2d_stats')
        y.check('%s %s y' % (shape, name))
        part.check('%s %s partial sums' % (shape, name))
        worst = check_close(y.t, ref, A, 'forward %s %s' % (shape, name))
        ys = y.t.double().cpu().view(N, H * W, cout)
        p = part.t.double().cpu()
        assert bool(torch.isfinite(p).all()), '%s %s: a partial-sum slot was not written' % (shape, name)
        got = p.sum(1)                                                      # (N, cout, 2)
        for j, (r, a) in enumerate(((ys.sum(1), ys.abs().sum(1)), ((ys * ys).sum(1), (ys * ys).sum(1)))):
            worst = max(worst, check_close(got[..., j], r, a, '%s %s partial sums [%s]' % (shape, name, ('sum y', 'sum y^2')[j]), rel=0.0))
        report(group, 'fwd %s %s' % (shape, name), k, items_of(N, H, W, cout), worst)


# ---- data gradient: no mask, ReLU mask, LeakyReLU-gradient mask; and the rectangle-list form
def dgrad_operands(N, H, W, cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    gy = rnd((N, H, W, cout), g).to(torch.bfloat16)
    w = rnd((cout, cin, 3, 3), g, (cout * 9) ** -0.5)
    aux = rnd((N, H, W, cin), g).to(torch.bfloat16)
    wq = w.to(torch.bfloat16).double()
    dx = dgrad3x3_64(gy.double(), wq)
    A = dgrad3x3_64(gy.double().abs(), wq.abs())
    return gy, w, aux, dx, A


def mask_of(aux, mode):
    from seg2eye_amd import _lib as L
    pos = aux.double() > 0
    if mode == L.AUX_RELU_MASK:
        return torch.where(pos, 1.0, 0.0).double()
    if mode == L.AUX_LRELU_GRAD:
        return torch.where(pos, 1.0, 0.2).double()
    return None


def run_dgrad(group, N, H, W, cin, cout, want, dev, seed):
    """the data gradient of the forward conv cin -> cout: gy (N, H, W, cout) -> dx (N, H, W, cin)"""
    L, lb = lib()
    from seg2eye_amd import ops
    gy, w, aux, dx, A = dgrad_operands(N, H, W, cin, cout, seed)
    gyd, auxd, wpt = gy.to(dev), aux.to(dev), ops.pack_weight(w.to(dev), torch.bfloat16, cin, True)
    shape = '%dx%dx%dx%d<-%d' % (N, H, W, cin, cout)
    for mode, mname in ((L.AUX_NONE, 'plain'), (L.AUX_RELU_MASK, 'relu-mask'), (L.AUX_LRELU_GRAD, 'lrelu-grad')):
        d = desc(N, H, W, cout, cin, transposed=1, aux_mode=mode)
        k = expect_kernel(d, want, shape)
        m = mask_of(aux, mode)
        ref = dx * m if m is not None else dx
        y = Guarded((N, H, W, cin), torch.bfloat16, dev, float('nan'))
        wsb = int(lb.s2e_conv2d_workspace_bytes(L.S2E_BF16, C.byref(d)))
        ws = workspace(wsb, dev)
        L.check(lb.s2e_conv2d(L.S2E_BF16, gyd.data_ptr(), wpt.data_ptr(), None, None, auxd.data_ptr() if m is not None else None, y.ptr(),
                              C.byref(d), ws.ptr(), wsb, stream()), 's2e_conv2d (data gradient)')
        y.check('%s %s dx' % (shape, mname))
        ws.check('%s %s workspace' % (shape, mname))
        worst = check_close(y.t, ref, A, 'data gradient %s %s' % (shape, mname))
        report(group, 'dgrad %s %s' % (shape, mname), k + ('+ws' if wsb else ''), items_of(N, H, W, cin), worst)


def rect_lists(R, g):
    """(name, list, device count): a random subset in random order with the count below its length, none, one, all"""
    perm = torch.randperm(R, generator=g).tolist()
    k = max(3, R // 2)
    return [('subset %d of %d listed' % (k - 2, k), perm[:k], k - 2), ('count 0', perm[:3], 0), ('count 1', perm[:4], 1),
            ('all %d' % R, torch.randperm(R, generator=g).tolist(), R)]


def run_rects(group, N, H, W, cin, cout, dev, seed):
    """s2e_conv2d_rects: the data gradient with the ReLU mask over a device-side rectangle list (duo shapes only)"""
    L, lb = lib()
    from seg2eye_amd import ops
    gy, w, aux, dx, A = dgrad_operands(N, H, W, cin, cout, seed)
    gyd, auxd, wpt = gy.to(dev), aux.to(dev), ops.pack_weight(w.to(dev), torch.bfloat16, cin, True)
    d = desc(N, H, W, cout, cin, transposed=1, aux_mode=L.AUX_RELU_MASK)
    k = expect_kernel(d, 'duo', 'rects')
    ref = dx * mask_of(aux, L.AUX_RELU_MASK)
    R = N * (H // 16) * (W // 16)
    shape = '%dx%dx%dx%d<-%d' % (N, H, W, cin, cout)
    for lname, ids, count in rect_lists(R, torch.Generator().manual_seed(seed + 1)):
        lst = torch.tensor(ids, dtype=torch.int32, device=dev)
        cnt = torch.tensor([count, 0], dtype=torch.int32, device=dev)
        y = Guarded((N, H, W, cin), torch.bfloat16, dev, SENTINEL)
        L.check(lb.s2e_conv2d_rects(L.S2E_BF16, gyd.data_ptr(), wpt.data_ptr(), None, None, auxd.data_ptr(), y.ptr(), C.byref(d),
                                    lst.data_ptr(), cnt.data_ptr(), stream()), 's2e_conv2d_rects')
        y.check('rects %s %s' % (shape, lname))
        keep = rect_mask(N, H, W, ids[:count])
        check_sentinel(y.t, keep, 'rects %s %s' % (shape, lname))
        worst = 0.0
        if count:
            worst = check_close(torch.where(keep, y.t.cpu().double(), 0.0), torch.where(keep, ref, 0.0), torch.where(keep, A, 1.0),
                                'rects %s %s' % (shape, lname))
        report(group, 'rects %s %s' % (shape, lname), k, count * (1 if cin <= 64 else -(-cin // 128)), worst)


# ---- fused [gamma | beta] conv + SPADE+Style modulation (nh = 128)
NH = 128


def run_fused(group, N, H, W, C_, lrelu_on, up, banked, with_gamma, with_bias, dev, seed, lists=False):
    L, lb = lib()
    from seg2eye_amd import ops
    flags = L.SPADE_X_HALF if up else 0
    g = torch.Generator().manual_seed(seed)
    actv = torch.relu(rnd((N, H, W, NH), g)).to(torch.bfloat16)
    w = rnd((2 * C_, NH, 3, 3), g, (NH * 9) ** -0.5)
    bias = rnd((2 * C_,), g, 0.2)
    hx, wx = (H // 2, W // 2) if up else (H, W)
    x = rnd((N, hx, wx, C_), g, 1.0, 0.3).to(torch.bfloat16)
    stats = torch.stack([rnd((N, C_), g, 0.3), 0.5 + 1.5 * torch.rand(N, C_, generator=g)], -1).float().contiguous()
    # the style codes: this layer's 2C columns in the MIDDLE of a bank holding three layers' (networks/stylebank.py); ld = S
    col0, S = (128, 128 + 2 * C_ + 256) if banked else (0, 2 * C_)
    bank = rnd((N, S), g, 0.4)
    s0, s1 = bank[:, col0:col0 + C_].double(), bank[:, col0 + C_:col0 + 2 * C_].double()
    x_full = x.double()
    if up:
        x_full = x_full.repeat_interleave(2, 1).repeat_interleave(2, 2)
    out_ref, a_out, gam_ref, a_gam = fused_ref(actv.double(), w.to(torch.bfloat16).double(), bias.double() if with_bias else None,
                                               x_full, stats.double(), s0, s1, lrelu_on)
    tw, th = C.c_int(0), C.c_int(0)
    assert lb.s2e_spade_conv_modulate_supported(L.S2E_BF16, N, H, W, C_, NH, flags)
    assert lb.s2e_spade_conv_modulate_rect(L.S2E_BF16, N, H, W, C_, NH, flags, C.byref(tw), C.byref(th))
    duo = duo_takes_fused(N, H, W, C_, NH, flags, tw.value, th.value)
    want = os.environ.get('S2E_CONV_DUO') != '0'
    assert duo == want, 'fused %dx%dx%dx%d: the duo rule says %s' % (N, H, W, C_, duo)
    k = ('duo-fused-mf16' if mf16_on() else 'duo-fused-mf32') if duo else 'patch-fused'
    ad, wp, bd, xd = actv.to(dev), ops.pack_weight(w.to(dev), torch.bfloat16, NH, False), bias.to(dev), x.to(dev)
    std, bankd = stats.to(dev), bank.to(dev)
    tag = '%dx%dx%dx%d%s%s%s%s%s' % (N, H, W, C_, ' lrelu' if lrelu_on else '', ' x/2' if up else '', ' bank' if banked else ' ld=0',
                                      '' if with_gamma else ' gamma=NULL', '' if with_bias else ' bias=NULL')
    R = N * (H // th.value) * (W // tw.value)

    def call(out, gam, ids=None, count=None):
        args = (L.S2E_BF16, ad.data_ptr(), wp.data_ptr(), bd.data_ptr() if with_bias else None, xd.data_ptr(), std.data_ptr(),
                bankd.data_ptr() + 4 * col0, S if banked else 0, out.ptr(), gam.ptr() if gam is not None else None, N, H, W, C_, NH,
                int(lrelu_on), flags)
        if ids is None:
            L.check(lb.s2e_spade_conv_modulate(*args, stream()), 's2e_spade_conv_modulate')
        else:
            lst = torch.tensor(ids, dtype=torch.int32, device=dev)
            cnt = torch.tensor([count, 0], dtype=torch.int32, device=dev)
            L.check(lb.s2e_spade_conv_modulate_sparse(*args, lst.data_ptr(), cnt.data_ptr(), stream()), 's2e_spade_conv_modulate_sparse')
            torch.cuda.synchronize()

    if not lists:
        out = Guarded((N, H, W, C_), torch.bfloat16, dev, float('nan'))
        gam = Guarded((N, H, W, C_), torch.bfloat16, dev, float('nan')) if with_gamma else None
        call(out, gam)
        out.check('fused %s out' % tag)
        worst = check_close(out.t, out_ref, a_out, 'fused %s out' % tag)
        if gam is not None:
            gam.check('fused %s gamma' % tag)
            worst = max(worst, check_close(gam.t, gam_ref, a_gam, 'fused %s gamma' % tag))
        report(group, 'fused %s' % tag, k, R * (C_ // 64), worst)
        return
    assert tw.value == 16 and th.value == 16
    for lname, ids, count in rect_lists(R, torch.Generator().manual_seed(seed + 1)):
        out = Guarded((N, H, W, C_), torch.bfloat16, dev, SENTINEL)
        gam = Guarded((N, H, W, C_), torch.bfloat16, dev, SENTINEL) if with_gamma else None
        call(out, gam, ids, count)
        keep = rect_mask(N, H, W, ids[:count])
        out.check('fused list %s %s out' % (tag, lname))
        check_sentinel(out.t, keep, 'fused list %s %s out' % (tag, lname))
        worst = 0.0
        if count:
            worst = check_close(torch.where(keep, out.t.cpu().double(), 0.0), torch.where(keep, out_ref, 0.0), torch.where(keep, a_out, 1.0),
                                'fused list %s %s out' % (tag, lname))
        if gam is not None:
            gam.check('fused list %s %s gamma' % (tag, lname))
            check_sentinel(gam.t, keep, 'fused list %s %s gamma' % (tag, lname))
            if count:
                worst = max(worst, check_close(torch.where(keep, gam.t.cpu().double(), 0.0), torch.where(keep, gam_ref, 0.0),
                                               torch.where(keep, a_gam, 1.0), 'fused list %s %s gamma' % (tag, lname)))
        report(group, 'fused list %s %s' % (tag, lname), k, count * (C_ // 64), worst)


# ---- weight gradient (conv_wgrad_patch.hip)
def wgrad_operands(N, H, W, cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = rnd((N, H, W, cin), g).to(torch.bfloat16)
    gy = rnd((N, H, W, cout), g).to(torch.bfloat16)
    return x, gy


def wgrad_call(x, gy, dw, db, d, ws, wsb, ids=None, count=None):
    L, lb = lib()
    dev = x.device
    if ids is None:
        L.check(lb.s2e_conv2d_wgrad(L.S2E_BF16, x.data_ptr(), gy.data_ptr(), dw.ptr(), db.ptr(), C.byref(d), ws.ptr(), wsb, stream()),
                's2e_conv2d_wgrad')
    else:
        lst = torch.tensor(ids, dtype=torch.int32, device=dev)
        cnt = torch.tensor([count, 0], dtype=torch.int32, device=dev)
        L.check(lb.s2e_conv2d_wgrad_rects(L.S2E_BF16, x.data_ptr(), gy.data_ptr(), dw.ptr(), db.ptr(), C.byref(d), lst.data_ptr(),
                                          cnt.data_ptr(), ws.ptr(), wsb, stream()), 's2e_conv2d_wgrad_rects')
    torch.cuda.synchronize()


def wgrad_kernel(d, N, H, W):
    L, lb = lib()
    assert lb.s2e_conv2d_wgrad_kernel_kind(L.S2E_BF16, C.byref(d)) == KERNEL_PATCH, 'the weight gradient left the patch kernel'
    assert lb.s2e_conv2d_wgrad_rects_workspace_bytes(L.S2E_BF16, C.byref(d)) > 0, 'the patch weight gradient takes no list here'
    return 'wgrad-patch-slab%d' % wgrad_slab(H, W)


def run_wgrad(group, N, H, W, cin, cout, dev, seed, modes=('exact', 'short', 'none'), twice=False):
    L, lb = lib()
    x, gy = wgrad_operands(N, H, W, cin, cout, seed)
    x64, g64 = x.double(), gy.double()
    ref, A = wgrad3x3_64(x64, g64), wgrad3x3_64(x64.abs(), g64.abs())
    rb, Ab = g64.sum((0, 1, 2)), g64.abs().sum((0, 1, 2))
    d = desc(N, H, W, cin, cout)
    k = wgrad_kernel(d, N, H, W)
    g = torch.Generator().manual_seed(seed + 7)
    dw0, db0 = rnd((cout, 9 * cin), g), rnd((cout,), g)
    xd, gyd = x.to(dev), gy.to(dev)
    need = int(lb.s2e_conv2d_wgrad_workspace_bytes(L.S2E_BF16, C.byref(d)))
    shape = '%dx%dx%dx%d->%d' % (N, H, W, cin, cout)
    for mode in modes:
        if mode == 'short' and need <= 256:
            continue
        wsb = {'exact': need, 'short': need - 256, 'none': 0}[mode]
        outs = []
        for rep in range(2 if twice else 1):
            dw = Guarded((cout, 9 * cin), torch.float32, dev, dw0)
            db = Guarded((cout,), torch.float32, dev, db0)
            ws = workspace(wsb, dev)
            wgrad_call(xd, gyd, dw, db, d, ws, wsb)
            for b_, nm in ((dw, 'dW'), (db, 'dbias'), (ws, 'workspace')):
                b_.check('wgrad %s %s %s' % (shape, mode, nm))
            outs.append((dw.t.clone(), db.t.clone()))
        worst = check_close(outs[0][0], ref, A + dw0.double().abs(), 'wgrad %s %s dW' % (shape, mode), rel=0.0, start=dw0.double())
        worst = max(worst, check_close(outs[0][1], rb, Ab + db0.double().abs(), 'wgrad %s %s dbias' % (shape, mode), rel=0.0, start=db0.double()))
        if twice:
            assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), \
                'wgrad %s %s: two S2E_DETERMINISTIC calls differ' % (shape, mode)
        report(group, 'wgrad %s %s ws %d B%s' % (shape, mode, wsb, ' x2 bitwise' if twice else ''), k, None, worst)


def run_wgrad_rects(group, N, H, W, cin, cout, dev, seed):
    L, lb = lib()
    x, gy = wgrad_operands(N, H, W, cin, cout, seed)
    x64, g64 = x.double(), gy.double()
    d = desc(N, H, W, cin, cout)
    k = wgrad_kernel(d, N, H, W)
    need = int(lb.s2e_conv2d_wgrad_rects_workspace_bytes(L.S2E_BF16, C.byref(d)))
    g = torch.Generator().manual_seed(seed + 7)
    dw0, db0 = rnd((cout, 9 * cin), g), rnd((cout,), g)
    xd, gyd = x.to(dev), gy.to(dev)
    R = N * (H // 16) * (W // 16)
    perm = torch.randperm(R, generator=g).tolist()
    shape = '%dx%dx%dx%d->%d' % (N, H, W, cin, cout)
    for lname, ids, count in (('count 0', perm[:3], 0), ('count 1', perm[:4], 1), ('count 2 of 5', perm[:5], 2),
                              ('subset %d' % (R // 3), perm[:R // 3 + 2], R // 3), ('all %d' % R, perm, R)):
        m = rect_mask(N, H, W, ids[:count]).double()
        gm = g64 * m
        ref, A = wgrad3x3_64(x64, gm), wgrad3x3_64(x64.abs(), gm.abs())
        dw = Guarded((cout, 9 * cin), torch.float32, dev, dw0)
        db = Guarded((cout,), torch.float32, dev, db0)
        ws = workspace(need, dev)
        wgrad_call(xd, gyd, dw, db, d, ws, need, ids, count)
        for b_, nm in ((dw, 'dW'), (db, 'dbias'), (ws, 'workspace')):
            b_.check('wgrad rects %s %s %s' % (shape, lname, nm))
        worst = check_close(dw.t, ref, A + dw0.double().abs(), 'wgrad rects %s %s dW' % (shape, lname), rel=0.0, start=dw0.double())
        worst = max(worst, check_close(db.t, gm.sum((0, 1, 2)), gm.abs().sum((0, 1, 2)) + db0.double().abs(),
                                       'wgrad rects %s %s dbias' % (shape, lname), rel=0.0, start=db0.double()))
        report(group, 'wgrad-rects %s %s ws %d B' % (shape, lname, need), k, None, worst)


# ---- the groups
FWD_SHAPES = [  # (N, H, W, Cin, Cout): one item (BN = 64); a 3 x 5 rectangle grid; three channel tiles; long K
    (1, 16, 16, 64, 64), (3, 48, 80, 128, 128), (2, 32, 64, 64, 384), (2, 16, 48, 1024, 128)]


def cap_shape(items):
    """(N, 16, 16 * items / N): N the smallest odd factor of `items` up to 9, else 1"""
    n = next((f for f in (3, 5, 7, 9) if items % f == 0), 1)
    return n, 16, 16 * (items // n)


def group_fwd(dev, want, shapes=FWD_SHAPES):
    for i, s in enumerate(shapes):
        run_forward('fwd', *s, want=want, dev=dev, seed=100 + i)


def group_dgrad(dev, want, shapes=FWD_SHAPES):
    for i, s in enumerate(shapes):
        run_dgrad('dgrad', *s, want=want, dev=dev, seed=200 + i)


def group_rects(dev, want):
    assert want == 'duo'
    for i, s in enumerate([(3, 48, 80, 128, 128), (2, 32, 64, 64, 384), (2, 32, 32, 256, 64)]):
        run_rects('rects', *s, dev=dev, seed=300 + i)


FUSED = [  # (N, H, W, C, lrelu, x at half resolution, banked style, gamma_out, bias)
    (1, 16, 16, 64, False, False, True, True, True),
    (3, 48, 80, 128, True, True, True, True, True),
    (3, 48, 80, 128, False, False, True, False, False),
    (2, 32, 32, 192, True, False, True, True, True),
    (2, 32, 32, 192, False, True, False, True, True),
    (2, 16, 16, 512, True, True, True, True, True)]


def group_fused(dev, want, cases=FUSED):
    for i, c in enumerate(cases):
        run_fused('fused', *c, dev=dev, seed=400 + i)


def group_fused_lists(dev, want):
    for i, c in enumerate([(3, 48, 80, 128, True, True, True, True, True), (2, 32, 32, 192, False, False, True, True, True),
                           (2, 16, 32, 512, True, False, True, False, True)]):
        run_fused('fused-list', *c, dev=dev, seed=500 + i, lists=True)


def group_cap(dev, want, which=('cap-1', 'cap+1', '2cap+3')):
    """item counts around the persistent grid of the duo kernel (grid = min(items, cap), cap = 2 x CUs): one item per workgroup,
    one workgroup with a second item, three workgroups with a third"""
    c = cap()
    table = {'cap-1': (c - 1, 64), 'cap+1': (c + 1, 128), '2cap+3': (2 * c + 3, 64)}
    for i, name in enumerate(which):
        items, cout = table[name]
        n, h, w = cap_shape(items)
        assert items_of(n, h, w, cout) == items
        run_forward('cap', n, h, w, 64, cout, want=want, dev=dev, seed=600 + i,
                    epilogues=[e for e in EPILOGUES if e[0] in ('bias+lrelu', 'bias+res')], stats=(name == 'cap+1'))
    n, h, w = cap_shape(c + 1)
    run_dgrad('cap', n, h, w, 64, 64, want=want, dev=dev, seed=650)


def group_bench(dev, want):
    """bench-like shapes with the library's own thresholds (no switches set): 256 and 512 work items"""
    run_forward('bench', 8, 64, 64, 128, 256, want='duo', dev=dev, seed=700, epilogues=[EPILOGUES[2], EPILOGUES[4]])
    run_dgrad('bench', 8, 64, 64, 128, 256, want='patch', dev=dev, seed=701)     # 128 items: below the duo threshold
    run_forward('bench', 2, 256, 256, 64, 128, want='duo', dev=dev, seed=702, epilogues=[EPILOGUES[3]])
    run_dgrad('bench', 2, 256, 256, 64, 128, want='duo', dev=dev, seed=703)
    run_fused('bench', 2, 128, 128, 128, True, True, True, True, True, dev=dev, seed=704)


WGRAD = [  # (N, H, W, Cin, Cout): slab 64 / 32 / 16; Cout 64 (a half-empty co tile), 192, 256; Cin 64 and 512
    (2, 16, 64, 64, 128), (2, 16, 96, 64, 192), (3, 16, 48, 512, 64), (2, 32, 64, 64, 256), (2, 32, 32, 512, 192)]


def group_wgrad(dev, want):
    slabs = set()
    for i, s in enumerate(WGRAD):
        slabs.add(wgrad_slab(s[1], s[2]))
        run_wgrad('wgrad', *s, dev=dev, seed=800 + i)
    assert slabs == {64, 32, 16}, slabs


def group_wgrad_rects(dev, want):
    for i, s in enumerate([(2, 32, 32, 64, 128), (1, 32, 48, 512, 64), (3, 16, 32, 64, 192)]):
        run_wgrad_rects('wgrad-rects', *s, dev=dev, seed=900 + i)


def group_wgrad_det(dev, want):
    assert os.environ.get('S2E_DETERMINISTIC') == '1'
    for i, s in enumerate([WGRAD[0], WGRAD[2], WGRAD[4]]):
        run_wgrad('wgrad-det', *s, dev=dev, seed=950 + i, modes=('exact',), twice=True)


GROUPS = {'fwd': group_fwd, 'dgrad': group_dgrad, 'rects': group_rects, 'fused': group_fused, 'fused_lists': group_fused_lists,
          'cap': group_cap, 'bench': group_bench, 'wgrad': group_wgrad, 'wgrad_rects': group_wgrad_rects, 'wgrad_det': group_wgrad_det}
SUBSETS = {  # --subset: the cases of a group a child under S2E_DUO_MF16=0 repeats
    'fwd': [FWD_SHAPES[1], FWD_SHAPES[2], FWD_SHAPES[3]], 'dgrad': [FWD_SHAPES[1], FWD_SHAPES[3]], 'fused': FUSED[1:5],
    'cap': ('cap+1',)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--groups', required=True)
    ap.add_argument('--subset', action='store_true', help='the reduced case list of the S2E_DUO_MF16=0 child')
    args = ap.parse_args()
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    dev = torch.device('cuda', 0)
    lib()
    want = 'patch' if os.environ.get('S2E_CONV_DUO') == '0' else 'duo'
    for name in args.groups.split(','):
        if args.subset and name in SUBSETS:
            GROUPS[name](dev, want, SUBSETS[name])
        else:
            GROUPS[name](dev, want)
    sw = ' '.join('%s=%s' % (k, os.environ[k]) for k in ('S2E_CONV_DUO', 'S2E_CONV_PATCH', 'S2E_SPADE_FUSED_TILES', 'S2E_DUO_MF16',
                                                        'S2E_WGRAD_PATCH', 'S2E_DETERMINISTIC') if k in os.environ) or 'defaults'
    print('conv3x3 ok: %d checks, groups %s (%s)' % (len(RESULTS), args.groups, sw), flush=True)


if __name__ == '__main__':
    main()
