#!/usr/bin/env python3
"""The label-map and resampling kernels of csrc/label_ops.hip at the C ABI, against tests/_label_ops_ref.py (references, bounds and
their derivation are there): s2e_label_conv3x3, s2e_label_conv3x3_batch (+ s2e_label_conv_block_map), s2e_onehot_nhwc,
s2e_upsample2x_fwd / _bwd, s2e_avgpool3x3s2_fwd / _bwd, s2e_tanh_bwd, s2e_lrelu_bwd, s2e_bilinear_resize_fwd / _bwd.

Run by tests/test_label_ops_fp64_gpu.py, one child per (group set, dtype), because the library reads S2E_LABEL_CONV_CAP once per
process (--cap sets it, after every S2E_* variable has been stripped from the environment):

    python tests/_label_ops_child.py --groups conv_small,conv_wave,conv_batch,onehot,upsample,pool,act,bilinear --dtype bf16|fp32 [--cap 3]
    python tests/_label_ops_child.py --groups wrap_upsample,wrap_pool,wrap_act,wrap_onehot --dtype none

Guards, as tests/_conv3x3_child.py (whose Guarded is used): every output lives inside a byte tensor with pattern bytes on both sides
that must come back unchanged; outputs the call overwrites start as NaN (all bits set), the bilinear backward's gx starts at zero as
its contract says.  Every element of every output is compared: err / bound <= 1, or bit for bit for the pure selections.  Every case
names the walk or kernel it was written for and asserts it from the launcher's own conditions (R.label_conv_plan, R.pool_kernel,
R.onehot_kernel, R.wraps), so that it cannot silently take another path.  Prints one line per case with its largest err / bound
('equal' for selections) and 'label ops ok: ...' last."""
import argparse
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import numpy as np                              # noqa: E402
import torch                                    # noqa: E402

import _label_ops_ref as R                      # noqa: E402
from _conv3x3_child import Guarded, lib, stream      # noqa: E402

S2E_ERR_UNSUPPORTED = -3
NAN_BYTE = 0xFF                                 # bf16 0xFFFF and fp32 0xFFFFFFFF are NaNs
RESULTS = []


def report(group, name, worst):
    line = '  %-13s %-100s %s' % (group, name, 'equal' if worst is None else 'worst err/bound %.3f' % worst)
    RESULTS.append(line)
    print(line, flush=True)


def code_of(dt):
    from seg2eye_amd import _lib as L
    return L.S2E_BF16 if dt == 'bf16' else L.S2E_F32


CAP = [R.LABEL_CONV_CAP]                        # --cap: what main() sets S2E_LABEL_CONV_CAP to


def cap():
    return CAP[0]


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def check_equal(got, want, what):
    """bit for bit (want: fp64 values exact in got's dtype)"""
    g, w = bits(got), bits(want.to(got.dtype))
    n = int((g != w).sum())
    assert n == 0, '%s: %d of %d elements differ bitwise (first at %s)' % (what, n, g.numel(), tuple(int(v) for v in (g != w).nonzero()[0]))


def nan_out(shape, dt, dev):
    return Guarded(tuple(shape), R.TDT[dt], dev, raw_fill=NAN_BYTE)


def walks_text(chunks):
    return '+'.join('%s(%d lanes/px, %d passes)' % (wk, cgb, passes) for wk, cgb, ppb, passes in chunks)


# ---- label conv, single launch
def run_conv(group, name, dt, dev, label, h, w, ncls, Cout, with_bias, relu, seed, want, kinds=None):
    """want: the walk of every 128-channel chunk the case is written for.  kinds: 'both' | 'uniform' | 'none' -- which kinds of pixel
    (3x3 neighbourhood one in-image class, or not) the label map must hold."""
    L, lb = lib()
    N, H, W = label.shape
    assert int(label.max()) < ncls
    npix = N * h * w
    gx, chunks = R.label_conv_plan(dt, npix, Cout, R.FAST_MIN_SINGLE, cap())
    assert [c[0] for c in chunks] == list(want), '%s: written for %s, the launcher takes %s' % (name, want, walks_text(chunks))
    uni = R.uniform_pixels(label, h, w)
    n_uni = int(uni.sum())
    if kinds == 'both':
        assert 0 < n_uni < npix, (name, n_uni)
    elif kinds == 'uniform':
        assert n_uni == max(0, h - 2) * max(0, w - 2) * N, (name, n_uni)
    elif kinds == 'none':
        assert n_uni == 0, (name, n_uni)
    wgt, b = R.label_conv_weights(Cout, ncls, with_bias, seed)
    ref, bound = R.label_conv_ref(label, h, w, wgt, b, relu, dt)
    lab, wd = torch.from_numpy(label).to(dev), wgt.to(dev)
    bd = b.to(dev) if with_bias else None
    out = nan_out((N, h, w, Cout), dt, dev)
    L.check(lb.s2e_label_conv3x3(code_of(dt), lab.data_ptr(), wd.data_ptr(), bd.data_ptr() if with_bias else None, out.ptr(),
                                 N, H, W, h, w, ncls, Cout, int(relu), stream()), 's2e_label_conv3x3')
    tag = '%s %dx%dx%d -> %dx%d ncls=%d Cout=%d%s%s%s, %d blocks x %s, %d uniform of %d px' % (
        name, N, H, W, h, w, ncls, Cout, ' ragged' if Cout % R.VEC[dt] else '', ' bias' if with_bias else ' bias=NULL', ' relu' if relu else '',
        gx, walks_text(chunks), n_uni, npix)
    out.check(tag)
    report(group, tag, R.worst_ratio(out.t, ref, bound, tag))
    return max(c[3] for c in chunks)


def no_uniform(label, ncls):
    """noise with every uniform neighbourhood broken (ncls > 1)"""
    lab = label.copy()
    for _ in range(20):
        uni = R.uniform_pixels(lab, lab.shape[1], lab.shape[2])
        if not uni.any():
            return lab
        lab[uni] = (lab[uni] + 1) % ncls
    raise AssertionError('could not break the uniform neighbourhoods')


def group_conv_small(dev, dt):
    g = 'conv_small'
    T = ('thread',)
    small = R.blocky_labels(2, 12, 12, 4, 101, block=4)
    run_conv(g, 'blocky', dt, dev, R.expand_labels(small, 2, 2, 4), 12, 12, 4, 128, True, 1, 201, T, 'both')
    run_conv(g, 'one class', dt, dev, R.expand_labels(R.one_class_labels(2, 12, 12, 3), 2, 2, 4), 12, 12, 4, 128, True, 1, 202, T, 'uniform')
    noise7 = no_uniform(R.noise_labels(1, 9, 7, 7, 102), 7)
    assert int((noise7 == 6).sum()) > 0
    run_conv(g, 'noise', dt, dev, R.expand_labels(noise7, 1, 2, 7), 9, 7, 7, 20, False, 0, 203, T, 'none')
    blocky7 = R.blocky_labels(1, 9, 7, 7, 103, block=4)
    assert int((blocky7 == 6).sum()) > 0
    run_conv(g, 'blocky', dt, dev, R.expand_labels(blocky7, 1, 2, 7), 9, 7, 7, 22, False, 0, 204, T, 'both')      # ragged in both dtypes
    run_conv(g, 'blocky', dt, dev, R.blocky_labels(3, 5, 6, 3, 104, block=5), 5, 6, 3, 152, True, 1, 205, T * 2, 'both')
    run_conv(g, 'noise', dt, dev, no_uniform(R.noise_labels(3, 5, 6, 3, 105), 3), 5, 6, 3, 152, True, 1, 206, T * 2, 'none')
    run_conv(g, 'one class', dt, dev, R.one_class_labels(1, 4, 4, 1), 4, 4, 2, 260, True, 0, 207, T * 3, 'uniform')
    for H, W in ((1, 1), (1, 37), (37, 1)):
        run_conv(g, 'one class', dt, dev, R.one_class_labels(1, H, W, 0), H, W, 1, 1, True, 0, 208 + H + W, T, 'uniform')


def group_conv_wave(dev, dt):
    g = 'conv_wave'
    Wv, T = ('wave',), ('thread',)
    small = R.blocky_labels(1, 260, 253, 4, 111, block=16)
    passes = 0
    for i, Cout in enumerate((8, 12, 32, 128, 136)):
        want = Wv * (2 if Cout > 128 else 1)
        if dt == 'fp32' and Cout == 12:
            want = T                                     # 3 lanes per pixel: the thread walk at 65780 pixels
        passes = max(passes, run_conv(g, 'blocky', dt, dev, small, 260, 253, 4, Cout, i != 2, i % 2, 301 + i, want, 'both'))
    # a full chunk on the wave walk and a 24-channel chunk (3 or 6 lanes per pixel) on the thread walk, in one launch whose grid is sized
    # from the first
    passes = max(passes, run_conv(g, 'blocky mixed walks', dt, dev, small, 260, 253, 4, 152, True, 1, 309, ('wave', 'thread'), 'both'))
    run_conv(g, 'blocky 65536 px', dt, dev, R.blocky_labels(1, 256, 256, 4, 112, block=16), 256, 256, 4, 8, True, 1, 310, Wv, 'both')
    run_conv(g, 'blocky 65535 px', dt, dev, R.blocky_labels(1, 255, 257, 4, 113, block=16), 255, 257, 4, 8, True, 1, 311, T, 'both')
    run_conv(g, 'blocky sy=2 sx=1', dt, dev, R.expand_labels(small, 2, 1, 4), 260, 253, 4, 32, True, 0, 312, Wv, 'both')
    assert cap() >= 257 or passes >= 86, passes          # under a small cap every block makes many passes


# ---- label conv, batched
BATCH_JOBS = [(48, 44, 128, 1, 'wave'), (24, 22, 64, 1, 'thread'), (48, 44, 20, 0, 'thread'), (16, 11, 128, 1, 'thread'), (48, 44, 8, 1, 'wave')]


def group_conv_batch(dev, dt):
    L, lb = lib()
    N, H, W, ncls = 1, 48, 44, 4
    label = R.blocky_labels(N, H, W, ncls, 121, block=6)
    uni = R.uniform_pixels(label, H, W)
    assert 0 < int(uni.sum()) < uni.size
    esz, gap = (2 if dt == 'bf16' else 4), 272           # a guard gap between the outputs; offsets stay 16-byte aligned
    refs, offs, ops, off, want_blocks, texts = [], [], [], 64, 0, []
    for j, (h, w, cout, relu, want) in enumerate(BATCH_JOBS):
        gx, chunks = R.label_conv_plan(dt, N * h * w, cout, R.FAST_MIN_BATCH, cap())
        assert len(chunks) == 1 and chunks[0][0] == want, 'job %d: written for the %s walk, the launcher takes %s' % (j, want, walks_text(chunks))
        want_blocks += gx
        texts.append('%d blocks x %s' % (gx, walks_text(chunks)))
        wgt, b = R.label_conv_weights(cout, ncls, j != 2, 400 + j)
        refs.append(R.label_conv_ref(label, h, w, wgt, b, relu, dt))
        ops.append((wgt.to(dev), b.to(dev) if b is not None else None))
        offs.append(off)
        off += N * h * w * cout * esz + gap
    buf = Guarded((off,), torch.uint8, dev, raw_fill=NAN_BYTE)
    jobs = (L.LabelConvJob * len(BATCH_JOBS))()
    for j, (h, w, cout, relu, want) in enumerate(BATCH_JOBS):
        jobs[j].weight, jobs[j].bias = ops[j][0].data_ptr(), (ops[j][1].data_ptr() if ops[j][1] is not None else None)
        jobs[j].out_off, jobs[j].h, jobs[j].w, jobs[j].cout, jobs[j].relu = offs[j], h, w, cout, relu
    nb = int(lb.s2e_label_conv_block_map(code_of(dt), C.byref(jobs), len(BATCH_JOBS), N, None))
    assert nb == want_blocks, 'block count %d with a NULL map, the launcher\'s rule gives %d' % (nb, want_blocks)
    bm = (C.c_int * (3 * nb))()
    assert int(lb.s2e_label_conv_block_map(code_of(dt), C.byref(jobs), len(BATCH_JOBS), N, bm)) == nb, 'block count with a map differs from the count without'
    jobs_dev = torch.tensor(list(bytes(jobs)), dtype=torch.uint8).to(dev)
    bm_dev = torch.tensor(list(bm), dtype=torch.int32).to(dev)
    lab = torch.from_numpy(label).to(dev)
    L.check(lb.s2e_label_conv3x3_batch(code_of(dt), lab.data_ptr(), jobs_dev.data_ptr(), bm_dev.data_ptr(), nb, buf.ptr(), N, H, W, ncls, stream()),
            's2e_label_conv3x3_batch')
    buf.check('label conv batch')
    flat = buf.t.cpu()
    gaps = torch.ones(off, dtype=torch.bool)
    for j, (h, w, cout, relu, want) in enumerate(BATCH_JOBS):
        nbytes = N * h * w * cout * esz
        gaps[offs[j]:offs[j] + nbytes] = False
        got = flat[offs[j]:offs[j] + nbytes].clone().view(R.TDT[dt]).view(N, h, w, cout)
        tag = 'job %d of one launch: %dx%dx%d -> %dx%d Cout=%d%s%s%s out_off=%d, %s' % (
            j, N, H, W, h, w, cout, ' ragged' if cout % R.VEC[dt] else '', ' bias' if ops[j][1] is not None else ' bias=NULL', ' relu' if relu else '',
            offs[j], texts[j])
        report('conv_batch', tag, R.worst_ratio(got, refs[j][0], refs[j][1], tag))
    assert bool((flat[gaps] == NAN_BYTE).all()), 'label conv batch: %d bytes between the outputs were written' % int((flat[gaps] != NAN_BYTE).sum())
    report('conv_batch', 'block map: %d blocks with a NULL map and with a map; %d gap bytes untouched' % (nb, int(gaps.sum())), None)


# ---- one-hot
def run_onehot(group, name, dt, dev, label, h, w, ncls, cpad, with_img, misaligned, want, seed=0, img=None, wrap_cap=None):
    L, lb = lib()
    N, H, W = label.shape
    assert int(label.max()) < ncls
    px = N * h * w
    assert R.onehot_kernel(cpad, misaligned, px) == want, '%s: written for %s' % (name, want)
    if wrap_cap is not None:
        assert R.wraps(px * (1 if want == 'onehot_nhwc8' else cpad), wrap_cap), '%s: the grid does not wrap' % name
    if with_img and img is None:
        img = torch.randn(N, h, w, generator=R.gen(seed)).to(R.TDT[dt])
    ref = R.onehot_ref(label, h, w, ncls, cpad, img if with_img else None)
    lab = torch.from_numpy(label).to(dev)
    imd = img.to(dev) if with_img else None
    esz = 2 if dt == 'bf16' else 4
    out = nan_out((px * cpad + 2,), dt, dev)             # one element before and one after stay NaN in the misaligned form
    ptr = out.ptr() + (esz if misaligned else 0)
    L.check(lb.s2e_onehot_nhwc(code_of(dt), lab.data_ptr(), imd.data_ptr() if with_img else None, ptr, N, H, W, h, w, ncls, cpad, stream()),
            's2e_onehot_nhwc')
    tag = '%s %dx%dx%d -> %dx%d ncls=%d cpad=%d%s%s: %s' % (name, N, H, W, h, w, ncls, cpad, ' image' if with_img else ' img=NULL',
                                                         ' out + 1 element' if misaligned else '', want)
    out.check(tag)
    lo = 1 if misaligned else 0
    check_equal(out.t[lo:lo + px * cpad].view(N, h, w, cpad), ref, tag)
    rest = torch.cat([out.t[:lo], out.t[lo + px * cpad:]])
    assert bool((bits(rest) == -1).all()), '%s: an element outside the output was written' % tag
    report(group, tag, None)


def group_onehot(dev, dt):
    g = 'onehot'
    for N, H, W in ((2, 6, 10), (1, 1, 1)):
        for ncls, with_img in ((4, True), (4, False), (7, True), (8, False)):
            run_onehot(g, 'aligned', dt, dev, R.noise_labels(N, H, W, ncls, 500 + ncls), H, W, ncls, 8, with_img, False, 'onehot_nhwc8', 510 + ncls)
        for cpad in (5, 12):
            run_onehot(g, 'generic', dt, dev, R.noise_labels(N, H, W, 4, 520 + cpad), H, W, 4, cpad, True, False, 'onehot_nhwc', 530 + cpad)
        run_onehot(g, 'generic', dt, dev, R.noise_labels(N, H, W, 5, 525), H, W, 5, 5, False, False, 'onehot_nhwc', 535)
        run_onehot(g, 'misaligned', dt, dev, R.noise_labels(N, H, W, 4, 540), H, W, 4, 8, True, True, 'onehot_nhwc', 541)
    small = R.noise_labels(2, 6, 10, 4, 550)
    big = R.expand_labels(small, 2, 4, 4)                # (2, 12, 40): h = H / 2, w = W / 4, the skipped pixels another class
    run_onehot(g, 'strided', dt, dev, big, 6, 10, 4, 8, True, False, 'onehot_nhwc8', 551)
    run_onehot(g, 'strided', dt, dev, big, 6, 10, 4, 12, True, False, 'onehot_nhwc', 552)


# ---- upsample 2x
def run_upsample(group, name, dt, dev, x, gy, wrap=False):
    L, lb = lib()
    N, h, w, C_ = x.shape
    assert C_ % R.VEC[dt] == 0
    if wrap:
        assert R.wraps(N * 4 * h * w * C_ // R.VEC[dt]) if gy is None else R.wraps(N * h * w * C_ // R.VEC[dt]), '%s: the grid does not wrap' % name
    if gy is None:
        y = nan_out((N, 2 * h, 2 * w, C_), dt, dev)
        xd = x.to(dev)
        L.check(lb.s2e_upsample2x_fwd(code_of(dt), xd.data_ptr(), y.ptr(), N, h, w, C_, stream()), 's2e_upsample2x_fwd')
        tag = '%s fwd %dx%dx%dx%d%s' % (name, N, h, w, C_, ': every block a second pass' if wrap else '')
        y.check(tag)
        check_equal(y.t, R.upsample_ref(x).double(), tag)
        report(group, tag, None)
    else:
        ref, bound = R.upsample_bwd_ref(gy, dt)
        gx = nan_out((N, h, w, C_), dt, dev)
        gd = gy.to(dev)
        L.check(lb.s2e_upsample2x_bwd(code_of(dt), gd.data_ptr(), gx.ptr(), N, h, w, C_, stream()), 's2e_upsample2x_bwd')
        tag = '%s bwd %dx%dx%dx%d%s' % (name, N, h, w, C_, ': every block a second pass' if wrap else '')
        gx.check(tag)
        report(group, tag, R.worst_ratio(gx.t, ref, bound, tag))


def group_upsample(dev, dt):
    L, lb = lib()
    V = R.VEC[dt]
    g = R.gen(600)
    for N, h, w, C_ in ((2, 5, 7, 16), (1, 1, 1, V), (3, 2, 9, 3 * V)):
        run_upsample('upsample', 'random', dt, dev, torch.randn(N, h, w, C_, generator=g).to(R.TDT[dt]), None)
        run_upsample('upsample', 'random', dt, dev, torch.empty(N, h, w, C_), (torch.randn(N, 2 * h, 2 * w, C_, generator=g) + 0.25).to(R.TDT[dt]))
    C_ = V + 1                                           # unsupported: the status, and nothing written
    for fwd in (True, False):
        a = torch.randn(2 * 6 * 6 * C_, generator=g).to(R.TDT[dt]).to(dev)
        out = nan_out((2 * 6 * 6 * C_,), dt, dev)
        fn = lb.s2e_upsample2x_fwd if fwd else lb.s2e_upsample2x_bwd
        rc = int(fn(code_of(dt), a.data_ptr(), out.ptr(), 2, 3, 3, C_, stream()))
        assert rc == S2E_ERR_UNSUPPORTED, 'C = VEC + 1: status %d, expected %d' % (rc, S2E_ERR_UNSUPPORTED)
        out.check('upsample C = VEC + 1')
        assert bool((bits(out.t) == -1).all()), 'upsample C = VEC + 1: the output was written'
        report('upsample', '%s C=%d: unsupported status, output untouched' % ('fwd' if fwd else 'bwd', C_), None)


# ---- average pool
POOL_C = ((8, {'bf16': 'vector', 'fp32': 'vector'}), (16, {'bf16': 'vector', 'fp32': 'vector'}), (12, {'bf16': 'scalar', 'fp32': 'vector'}),
          (5, {'bf16': 'scalar', 'fp32': 'scalar'}))
POOL_HW = ((1, 1), (1, 6), (2, 2), (5, 1), (17, 13), (32, 32))


def run_pool(group, name, dt, dev, x, gy, H, W, want, wrap=False):
    L, lb = lib()
    C_ = (x if gy is None else gy).shape[-1]
    N = (x if gy is None else gy).shape[0]
    assert R.pool_kernel(dt, C_) == want, '%s: written for the %s kernel' % (name, want)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    if wrap:
        assert want == 'vector' and R.wraps(N * (Ho * Wo if gy is None else H * W) * C_ // R.VEC[dt]), '%s: the grid does not wrap' % name
    if gy is None:
        ref, bound = R.pool_fwd_ref(x, dt)
        out = nan_out((N, Ho, Wo, C_), dt, dev)
        a = x.to(dev)
        L.check(lb.s2e_avgpool3x3s2_fwd(code_of(dt), a.data_ptr(), out.ptr(), N, H, W, C_, stream()), 's2e_avgpool3x3s2_fwd')
    else:
        ref, bound = R.pool_bwd_ref(gy, H, W, dt)
        out = nan_out((N, H, W, C_), dt, dev)
        a = gy.to(dev)
        L.check(lb.s2e_avgpool3x3s2_bwd(code_of(dt), a.data_ptr(), out.ptr(), N, H, W, C_, stream()), 's2e_avgpool3x3s2_bwd')
    tag = '%s %s %dx%dx%dx%d: %s kernel%s' % (name, 'fwd' if gy is None else 'bwd', N, H, W, C_, want, ', every block a second pass' if wrap else '')
    out.check(tag)
    report(group, tag, R.worst_ratio(out.t, ref, bound, tag))


def group_pool(dev, dt):
    g = R.gen(700)
    for C_, want in POOL_C:
        for H, W in POOL_HW:
            x = (torch.randn(2, H, W, C_, generator=g) + 0.5).to(R.TDT[dt])
            run_pool('pool', 'random', dt, dev, x, None, H, W, want[dt])
            gy = (torch.randn(2, (H + 1) // 2, (W + 1) // 2, C_, generator=g) + 0.5).to(R.TDT[dt])
            run_pool('pool', 'random', dt, dev, None, gy, H, W, want[dt])


# ---- tanh', LeakyReLU'
def run_act(group, name, dt, dev, gy, y, tanh, wrap=False, alias=False):
    L, lb = lib()
    n = gy.numel()
    if wrap:
        assert R.wraps(n if tanh else n // R.VEC[dt]), '%s: the grid does not wrap' % name
    ref, bound = (R.tanh_bwd_ref if tanh else R.lrelu_bwd_ref)(gy, y, dt)
    yd = y.to(dev)
    gd = yd if alias else gy.to(dev)
    gx = nan_out((n,), dt, dev)
    fn = lb.s2e_tanh_bwd if tanh else lb.s2e_lrelu_bwd
    L.check(fn(code_of(dt), gd.data_ptr(), yd.data_ptr(), gx.ptr(), n, stream()), 's2e_tanh_bwd' if tanh else 's2e_lrelu_bwd')
    tail = '' if tanh else ' (%d vectors + %d scalar)' % (n // R.VEC[dt], n % R.VEC[dt])
    tag = '%s %s n=%d%s%s, %d zeros in y' % (name, 'tanh_bwd' if tanh else 'lrelu_bwd', n, tail, ': every block a second pass' if wrap else '',
                                            int((y == 0).sum()))
    gx.check(tag)
    report(group, tag, R.worst_ratio(gx.t, ref, bound, tag))


def group_act(dev, dt):
    V = R.VEC[dt]
    for tanh in (True, False):
        for n in (1, 3, V, V + 1, 4099):
            gy, y = R.activation_inputs(n, dt, 800 + n, tanh)
            assert int((y == 0).sum()) > 0
            run_act('act', 'specials', dt, dev, gy, y, tanh)


# ---- bilinear
def group_bilinear(dev, dt):
    L, lb = lib()
    g = R.gen(900)
    for H, W, Ho, Wo in ((1, 1, 4, 4), (2, 3, 7, 300), (64, 96, 17, 23), (5, 5, 5, 5)):
        N = 2
        x = torch.randn(N, H, W, generator=g) * 2
        ref, bound = R.bilinear_fwd_ref(x, Ho, Wo, dt)
        xd = x.to(dev)
        y = nan_out((N, Ho, Wo), dt, dev)
        L.check(lb.s2e_bilinear_resize_fwd(code_of(dt), xd.data_ptr(), y.ptr(), N, H, W, Ho, Wo, stream()), 's2e_bilinear_resize_fwd')
        tag = 'fwd %dx%dx%d -> %dx%d (%d column blocks)' % (N, H, W, Ho, Wo, R.cdiv(Wo, 256))
        y.check(tag)
        report('bilinear', tag, R.worst_ratio(y.t, ref, bound, tag))
        gy = torch.randn(N, Ho, Wo, generator=g).to(R.TDT[dt])
        ref, bound = R.bilinear_bwd_ref(gy, H, W)
        gd = gy.to(dev)
        gx = Guarded((N, H, W), torch.float32, dev, 0.0)
        L.check(lb.s2e_bilinear_resize_bwd(code_of(dt), gd.data_ptr(), gx.ptr(), N, H, W, Ho, Wo, stream()), 's2e_bilinear_resize_bwd')
        tag = 'bwd %dx%dx%d <- %dx%d, %d input pixels nothing reaches' % (N, H, W, Ho, Wo, int((bound == 0).sum()))
        gx.check(tag)
        report('bilinear', tag, R.worst_ratio(gx.t, ref, bound, tag))


# ---- grid-stride wrap: just over 8192 x 256 threads' worth of work (4096 x 256 for the 8-channel one-hot), in the cheaper dtype
def group_wrap_upsample(dev, dt):
    run_upsample('wrap', 'ramp', 'fp32', dev, R.ramp((1, 363, 362, 16), 'fp32'), None, wrap=True)
    # (the backward reads four vectors per thread: 134 MB of gy for 2^21 threads, whatever the shape)
    run_upsample('wrap', 'ramp', 'fp32', dev, torch.empty(1, 725, 724, 16), R.ramp((1, 1450, 1448, 16), 'fp32'), wrap=True)


def group_wrap_pool(dev, dt):
    # forward: a thread writes 16 bytes and reads the taps of its pixel; 1 x 1 maps keep the input as small as the output
    run_pool('wrap', 'ramp', 'fp32', dev, R.ramp((1050000, 1, 1, 8), 'fp32'), None, 1, 1, 'vector', wrap=True)
    run_pool('wrap', 'ramp', 'fp32', dev, None, R.ramp((2, 182, 181, 32), 'fp32'), 363, 362, 'vector', wrap=True)


def group_wrap_act(dev, dt):
    n = R.GRID_CAP * 256 + 4099
    run_act('wrap', 'ramp', 'bf16', dev, R.ramp((n,), 'bf16', period=241), R.ramp((n,), 'bf16'), True, wrap=True)
    n = 4 * (R.GRID_CAP * 256 + 1000) + 3                # (gy and y are one buffer: three of 33.6 MB would not fit the budget)
    y = R.ramp((n,), 'fp32')
    run_act('wrap', 'ramp gy=y', 'fp32', dev, y, y, False, wrap=True, alias=True)


def group_wrap_onehot(dev, dt):
    N, h, w = 1, 1025, 1024
    label = ((np.arange(N * h * w, dtype=np.int64) % 5) % 4).astype(np.uint8).reshape(N, h, w)
    run_onehot('wrap', 'ramp', 'bf16', dev, label, h, w, 4, 8, True, False, 'onehot_nhwc8', img=R.ramp((N, h, w), 'bf16'), wrap_cap=R.GRID_CAP_ONEHOT8)
    N, h, w = 1, 648, 648
    label = ((np.arange(N * h * w, dtype=np.int64) % 5) % 4).astype(np.uint8).reshape(N, h, w)
    run_onehot('wrap', 'ramp', 'bf16', dev, label, h, w, 4, 5, True, False, 'onehot_nhwc', img=R.ramp((N, h, w), 'bf16'), wrap_cap=R.GRID_CAP)


GROUPS = {'conv_small': group_conv_small, 'conv_wave': group_conv_wave, 'conv_batch': group_conv_batch, 'onehot': group_onehot,
          'upsample': group_upsample, 'pool': group_pool, 'act': group_act, 'bilinear': group_bilinear,
          'wrap_upsample': group_wrap_upsample, 'wrap_pool': group_wrap_pool, 'wrap_act': group_wrap_act, 'wrap_onehot': group_wrap_onehot}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--groups', required=True)
    ap.add_argument('--dtype', default='none', choices=['bf16', 'fp32', 'none'])
    ap.add_argument('--cap', type=int, default=0, help='S2E_LABEL_CONV_CAP for this process (0: the default)')
    args = ap.parse_args()
    for k in [k for k in os.environ if k.startswith('S2E_')]:
        del os.environ[k]                                # the library reads its switches once: only what the cases name
    if args.cap:
        os.environ['S2E_LABEL_CONV_CAP'] = str(args.cap)
        CAP[0] = args.cap
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    dev = torch.device('cuda', 0)
    lib()
    dt = None if args.dtype == 'none' else args.dtype
    for name in args.groups.split(','):
        assert dt is not None or name.startswith('wrap_'), 'group %s needs --dtype' % name
        GROUPS[name](dev, dt)
    print('label ops ok: %d cases, groups %s (%s), S2E_LABEL_CONV_CAP=%d' % (len(RESULTS), args.groups, args.dtype, cap()), flush=True)


if __name__ == '__main__':
    main()
