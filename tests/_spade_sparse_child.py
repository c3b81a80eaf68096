#!/usr/bin/env python3
"""The small kernels of the label-sparse SPADE path at the C ABI, against tests/_spade_sparse_ref.py (references, bounds and their
derivation are there): s2e_label_rect_classify, s2e_spade_class_table, s2e_spade_class_table_batch, s2e_spade_modulate_uniform
(csrc/label_ops.hip), s2e_label_rect_lists_bwd, s2e_spade_uniform_sums, s2e_spade_uniform_grads (csrc/spade_sparse_bwd.hip).

Run by tests/test_spade_sparse_fp64_gpu.py, one child per (group set, dtype):

    python tests/_spade_sparse_child.py --groups classify,lists_bwd,table,modulate,sums,grads,chain --dtype bf16|fp32|none

Guards, as tests/_conv3x3_child.py (whose Guarded is used): every output and scratch buffer lives inside a byte tensor with pattern bytes
on both sides that must come back unchanged; outputs the call overwrites start as NaN (integers: as a poison value), outputs it
accumulates into start non-zero, and whatever a list form must not touch starts as a sentinel that must stay bit-identical.  Every element
of every output is compared.  Prints one line per case with its largest err / bound ('equal' for integer outputs) and
'spade sparse ok: ...' last."""
import argparse
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import numpy as np                              # noqa: E402
import torch                                    # noqa: E402

import _spade_sparse_ref as R                   # noqa: E402
from _conv3x3_child import Guarded, SENTINEL, lib, stream      # noqa: E402

SENT_I = -77                                    # what list entries at and beyond the count must keep
POISON_U8 = 0xEE                                # cls before the call: neither a class nor 255
NCLS = 4
DTYPES = {'bf16': torch.bfloat16, 'fp32': torch.float32}
RESULTS = []


def report(group, name, worst):
    line = '  %-9s %-86s %s' % (group, name, 'equal' if worst is None else 'worst err/bound %.3f' % worst)
    RESULTS.append(line)
    print(line, flush=True)


def code_of(dt):
    from seg2eye_amd import _lib as L
    return L.S2E_BF16 if dt == torch.bfloat16 else L.S2E_F32


def gen(seed):
    return torch.Generator().manual_seed(seed)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def check_bits(got, want, where, what):
    """got must equal want bit for bit wherever `where` (broadcastable bool) holds"""
    diff = (bits(got) != bits(want)) & where
    n = int(diff.sum())
    assert n == 0, '%s: %d elements differ bitwise (first at %s)' % (what, n, tuple(int(v) for v in diff.nonzero()[0]))


def check_list(buf, want, count_got, what):
    """a compacted list: the first len(want) entries equal want (ascending), every later entry still SENT_I"""
    got = buf.t.cpu().numpy()
    assert count_got == len(want), '%s: count %d, reference %d' % (what, count_got, len(want))
    assert np.array_equal(got[:len(want)], want), '%s: list differs from the reference' % what
    assert (got[len(want):] == SENT_I).all(), '%s: entries beyond the count were written' % what


def i32(a, dev):
    return torch.as_tensor(np.asarray(a, dtype=np.int32)).to(dev)


# ---- classify
def run_classify(name, label, h, w, tw, th, dev, expect=()):
    """expect: [(rectangle, class | 255)] the case is written for, asserted on the reference first"""
    L, lb = lib()
    N, H, W = label.shape
    cls_ref, dense_ref, uni_ref = R.classify_ref(label, h, w, tw, th)
    for r, want in expect:
        assert cls_ref[r] == want, '%s: the reference gives rectangle %d class %d, the case is written for %d' % (name, r, cls_ref[r], want)
    total = cls_ref.size
    lab = torch.from_numpy(label).to(dev)
    cls = Guarded((total,), torch.uint8, dev, raw_fill=POISON_U8)
    dl, ul = Guarded((total,), torch.int32, dev, SENT_I), Guarded((total,), torch.int32, dev, SENT_I)
    cnt = Guarded((2,), torch.int32, dev, SENT_I)
    L.check(lb.s2e_label_rect_classify(lab.data_ptr(), N, H, W, h, w, tw, th, cls.ptr(), dl.ptr(), ul.ptr(), cnt.ptr(), stream()),
            's2e_label_rect_classify')
    for b_, nm in ((cls, 'cls'), (dl, 'dense list'), (ul, 'uniform list'), (cnt, 'counts')):
        b_.check('classify %s %s' % (name, nm))
    got = cls.t.cpu().numpy()
    bad = np.nonzero(got != cls_ref)[0]
    assert bad.size == 0, 'classify %s: %d of %d rectangles differ; first %d: got %d, reference %d' % (
        name, bad.size, total, bad[0], got[bad[0]], cls_ref[bad[0]])
    c = cnt.t.cpu().tolist()
    check_list(dl, dense_ref, c[0], 'classify %s dense' % name)
    check_list(ul, uni_ref, c[1], 'classify %s uniform' % name)
    report('classify', '%s: %dx%dx%d -> %dx%d, %dx%d rects, %d dense + %d uniform' % (name, N, H, W, h, w, tw, th, len(dense_ref), len(uni_ref)), None)


RECTS = [(16, 16), (8, 8), (32, 8), (64, 64)]


def group_classify(dev, dt):
    base = R.salt(R.block_labels(2, 96, 96), [(0, 20, 20), (1, 70, 33), (1, 95, 95), (0, 0, 50)])
    for tw, th in RECTS:
        for s in (1, 2, 4):
            run_classify('block H=%dh' % s, R.upsample_salted(base, s), 96, 96, tw, th, dev)
    for shape in ((2, 40, 50), (3, 21, 19)):
        rag = R.salt(np.full(shape, 2, dtype=np.uint8), [(0, 11, 7), (shape[0] - 1, shape[1] - 1, shape[2] - 1)])
        for tw, th in RECTS:
            run_classify('ragged', rag, shape[1], shape[2], tw, th, dev)
        run_classify('ragged H=2h', R.upsample_salted(rag, 2), shape[1], shape[2], 8, 8, dev)
    # one salted pixel around rectangle (ty, tx) = (2, 2) of a one-class 96 x 96 map in 16 x 16 rectangles: pixels 32..47
    one = np.full((2, 96, 96), 1, dtype=np.uint8)
    r22 = 2 * 6 + 2
    for nm, (y, x), want in (('inside the rectangle', (40, 40), R.DENSE), ('halo distance 1', (31, 40), R.DENSE),
                             ('halo distance 2', (40, 49), R.DENSE), ('halo corner (2, 2)', (30, 30), R.DENSE),
                             ('halo corner (2, 2) low right', (49, 49), R.DENSE), ('distance 3', (29, 40), 1),
                             ('diagonal distance 3', (50, 50), 1)):
        run_classify('salt %s' % nm, R.salt(one, [(0, y, x)]), 96, 96, 16, 16, dev, expect=[(r22, want)])
    # the halo clipped at the image edge: what lies beyond it in memory (the end of the row before, the start of the row after)
    run_classify('salt outside the left edge', R.salt(one, [(0, 39, 95), (0, 39, 94)]), 96, 96, 16, 16, dev, expect=[(2 * 6 + 0, 1), (2 * 6 + 5, R.DENSE)])
    run_classify('salt outside the right edge', R.salt(one, [(0, 41, 0), (0, 41, 1)]), 96, 96, 16, 16, dev, expect=[(2 * 6 + 5, 1), (2 * 6 + 0, R.DENSE)])
    run_classify('salt last row of sample 0', R.salt(one, [(0, 95, 40), (0, 94, 40)]), 96, 96, 16, 16, dev, expect=[(36 + 2, 1), (5 * 6 + 2, R.DENSE)])
    run_classify('salt first row of sample 1', R.salt(one, [(1, 0, 40), (1, 1, 40)]), 96, 96, 16, 16, dev, expect=[(5 * 6 + 2, 1), (36 + 2, R.DENSE)])
    run_classify('all uniform', one, 96, 96, 16, 16, dev)
    checker = ((np.arange(48)[:, None] + np.arange(64)[None, :]) % 3).astype(np.uint8)[None].repeat(2, 0)
    run_classify('all dense', checker, 48, 64, 8, 8, dev)
    big = R.salt(R.block_labels(3, 152, 152), [(0, 30, 30), (1, 100, 9), (2, 151, 151), (2, 0, 0)])
    run_classify('1083 rectangles', big, 152, 152, 8, 8, dev)


# ---- lists_bwd
def run_lists_bwd(name, cls_np, N, tiles_y, tiles_x, dev):
    L, lb = lib()
    work_ref, ui_ref = R.lists_bwd_ref(cls_np, N, tiles_y, tiles_x)
    total = cls_np.size
    cls = torch.from_numpy(cls_np).to(dev)
    wl, ul = Guarded((total,), torch.int32, dev, SENT_I), Guarded((total,), torch.int32, dev, SENT_I)
    cnt = Guarded((2,), torch.int32, dev, SENT_I)
    L.check(lb.s2e_label_rect_lists_bwd(cls.data_ptr(), N, tiles_y, tiles_x, wl.ptr(), ul.ptr(), cnt.ptr(), stream()), 's2e_label_rect_lists_bwd')
    for b_, nm in ((wl, 'work list'), (ul, 'uniform-interior list'), (cnt, 'counts')):
        b_.check('lists_bwd %s %s' % (name, nm))
    c = cnt.t.cpu().tolist()
    check_list(wl, work_ref, c[0], 'lists_bwd %s work' % name)
    check_list(ul, ui_ref, c[1], 'lists_bwd %s uniform-interior' % name)
    report('lists_bwd', '%s: %d x %dx%d tiles, %d work + %d uniform-interior' % (name, N, tiles_y, tiles_x, len(work_ref), len(ui_ref)), None)


def group_lists_bwd(dev, dt):
    g = np.random.RandomState(11)
    for nm, N, ty, tx in (('3x3', 2, 3, 3), ('1x7 no interior', 2, 1, 7), ('2x2 no interior', 3, 2, 2), ('1125 rectangles', 5, 15, 15)):
        cls = g.choice(np.array([0, 1, 2, 3, R.DENSE], dtype=np.uint8), size=N * ty * tx, p=[0.2, 0.2, 0.2, 0.15, 0.25])
        run_lists_bwd(nm, cls, N, ty, tx, dev)
    run_lists_bwd('3x3 all uniform', np.full(9, 3, dtype=np.uint8), 1, 3, 3, dev)
    run_lists_bwd('15x15 all dense', np.full(225, R.DENSE, dtype=np.uint8), 1, 15, 15, dev)


# ---- table
def table_operands(nh, ncls, C_, with_bias, dt, dev, seed):
    """-> device operands (w_sh, b_sh, packed [gamma | beta] weight, bias | None) and the fp64 reference with its |.| twin"""
    from seg2eye_amd import ops
    g = gen(seed)
    w_sh, b_sh = R.grid_weights((nh, ncls, 3, 3), g), R.grid_weights((nh,), g)
    w = torch.randn(2 * C_, nh, 3, 3, generator=g) * (9 * nh) ** -0.5
    bias = torch.randn(2 * C_, generator=g) * 0.2
    ref, A = R.table_ref(w_sh, b_sh, w.to(dt).double(), bias.double() if with_bias else None, dt)
    d = (w_sh.float().to(dev), b_sh.float().to(dev), ops.pack_weight(w.to(dev), dt, nh, False), bias.to(dev) if with_bias else None)
    return d, ref, A


def group_table(dev, dt):
    L, lb = lib()
    seed = 1000
    for nh in (128, 64, 40):
        for ncls in (4, 3, 1):
            for C_ in (64, 6, 1):
                for with_bias in (True, False):
                    seed += 1
                    (w_sh, b_sh, wp, bias), ref, A = table_operands(nh, ncls, C_, with_bias, dt, dev, seed)
                    tab = Guarded((ncls, 5, 5, 2 * C_), torch.float32, dev, float('nan'))
                    L.check(lb.s2e_spade_class_table(code_of(dt), w_sh.data_ptr(), b_sh.data_ptr(), wp.data_ptr(), bias.data_ptr() if with_bias else None,
                                                     tab.ptr(), ncls, nh, C_, stream()), 's2e_spade_class_table')
                    name = 'table nh=%d ncls=%d C=%d %s' % (nh, ncls, C_, 'bias' if with_bias else 'bias=NULL')
                    tab.check(name)
                    report('table', name, R.check_close(tab.t.double().cpu(), ref, A, name, rel=0.0))
    # the batch form: three jobs that differ in nh and C, tables at uneven offsets of one buffer whose gaps must stay as they were
    for ncls in (4, 3):
        specs = [(128, 64, True), (64, 6, False), (40, 1, True)]
        ops_, refs, offs, off = [], [], [], 64
        for j, (nh, C_, with_bias) in enumerate(specs):
            d, ref, A = table_operands(nh, ncls, C_, with_bias, dt, dev, 1900 + 10 * ncls + j)
            ops_.append(d)
            refs.append((ref, A))
            offs.append(off)
            off += ncls * 25 * 2 * C_ * 4 + 40
        buf = Guarded((off // 4,), torch.float32, dev, float('nan'))
        start = buf.t.clone()
        jobs = (L.ClassTableJob * len(specs))()
        for j, (nh, C_, with_bias) in enumerate(specs):
            w_sh, b_sh, wp, bias = ops_[j]
            jobs[j].w_sh, jobs[j].b_sh, jobs[j].w_packed = w_sh.data_ptr(), b_sh.data_ptr(), wp.data_ptr()
            jobs[j].bias = bias.data_ptr() if with_bias else None
            jobs[j].table_off, jobs[j].nh, jobs[j].C = offs[j], nh, C_
        nb = int(lb.s2e_class_table_block_map(C.byref(jobs), len(specs), None))
        assert nb == sum(-(-2 * s[1] // 4) for s in specs), nb
        bm = (C.c_int * (2 * nb))()
        assert int(lb.s2e_class_table_block_map(C.byref(jobs), len(specs), bm)) == nb
        jobs_dev = torch.tensor(list(bytes(jobs)), dtype=torch.uint8).to(dev)
        bm_dev = i32(list(bm), dev)
        L.check(lb.s2e_spade_class_table_batch(code_of(dt), jobs_dev.data_ptr(), bm_dev.data_ptr(), nb, buf.ptr(), ncls, stream()),
                's2e_spade_class_table_batch')
        buf.check('table batch ncls=%d' % ncls)
        flat = buf.t.cpu()
        gap = torch.ones(flat.numel(), dtype=torch.bool)
        for j, (nh, C_, with_bias) in enumerate(specs):
            n = ncls * 25 * 2 * C_
            gap[offs[j] // 4:offs[j] // 4 + n] = False
            name = 'table batch ncls=%d job %d nh=%d C=%d %s table_off=%d' % (ncls, j, nh, C_, 'bias' if with_bias else 'bias=NULL', offs[j])
            got = flat[offs[j] // 4:offs[j] // 4 + n].view(ncls, 5, 5, 2 * C_).double()
            report('table', name, R.check_close(got, refs[j][0], refs[j][1], name, rel=0.0))
        check_bits(flat, start, gap, 'table batch ncls=%d: the gaps between the tables' % ncls)


# ---- modulate
def band_labels(N, H, W):
    """the class by horizontal band (boundary at H / 2), rotated by the sample index: uniform rectangles at every rectangle width"""
    lab = np.zeros((N, H, W), dtype=np.uint8)
    lab[:, H // 2:] = 1
    return ((lab + np.arange(N, dtype=np.uint8)[:, None, None]) % NCLS).astype(np.uint8)


def run_modulate(name, dt, label, C_, tw, th, lrelu_on, with_gamma, x_up, banked, short, dev, seed):
    L, lb = lib()
    N, H, W = label.shape
    cls, dense, uni = R.classify_ref(label, H, W, tw, th)
    assert len(uni) > 0, '%s: no uniform rectangle' % name
    count = len(uni) - (-(-len(uni) // 3) if short else 0)
    assert not short or 0 < count < len(uni), '%s: the list is too short to be cut' % name
    keep = torch.from_numpy(R.rect_pixels(uni[:count], N, H, W, tw, th))[..., None]
    cmap = R.rect_class_map(cls, N, H, W, tw, th)
    cmap = np.where(cmap == R.DENSE, 0, cmap)
    g = gen(seed)
    hx, wx = (H // 2, W // 2) if x_up else (H, W)
    x = (torch.randn(N, hx, wx, C_, generator=g) + 0.3).to(dt)
    stats = torch.stack([torch.randn(N, C_, generator=g) * 0.3, 0.5 + 1.5 * torch.rand(N, C_, generator=g)], -1).float().contiguous()
    col0, S = (132, 132 + 2 * C_ + 24) if banked else (0, 2 * C_)        # 16-byte-aligned offset into a wider bank
    bank = torch.randn(N, S, generator=g) * 0.4
    table = torch.randn(NCLS, 5, 5, 2 * C_, generator=g) * 0.5
    x_full = x.double()
    if x_up:
        x_full = x_full.repeat_interleave(2, 1).repeat_interleave(2, 2)
    ref, A, gamma = R.modulate_ref(x_full, stats.double(), bank[:, col0:col0 + C_].double(), bank[:, col0 + C_:col0 + 2 * C_].double(),
                                   table.double(), cmap, lrelu_on)
    xd, std, bankd, tabd = x.to(dev), stats.to(dev), bank.to(dev), table.to(dev)
    clsd, unid = torch.from_numpy(cls).to(dev), i32(uni, dev)
    cnt = i32([len(dense), count], dev)
    out = Guarded((N, H, W, C_), dt, dev, SENTINEL)
    gam = Guarded((N, H, W, C_), dt, dev, SENTINEL) if with_gamma else None
    L.check(lb.s2e_spade_modulate_uniform(code_of(dt), xd.data_ptr(), std.data_ptr(), bankd.data_ptr() + 4 * col0, S if banked else 0, tabd.data_ptr(),
                                          clsd.data_ptr(), unid.data_ptr(), cnt.data_ptr(), out.ptr(), gam.ptr() if gam is not None else None,
                                          N, H, W, C_, tw, th, int(lrelu_on), int(x_up), stream()), 's2e_spade_modulate_uniform')
    tag = '%s %dx%dx%dx%d %dx%d rects%s%s%s%s, %d of %d uniform listed' % (
        name, N, H, W, C_, tw, th, ' lrelu' if lrelu_on else '', ' x/2' if x_up else '', ' style_ld=%d' % S if banked else ' ld=0',
        '' if with_gamma else ' gamma=NULL', count, len(uni))
    out.check(tag + ' out')
    sent = torch.full((1,), SENTINEL, dtype=dt)
    check_bits(out.t, sent.expand(N, H, W, C_), ~keep, tag + ' out outside the listed rectangles')
    worst = R.check_close(torch.where(keep, out.t.double().cpu(), 0.0), torch.where(keep, ref, 0.0), torch.where(keep, A, 1.0), tag + ' out',
                          rel=R.rel_of(dt))
    if gam is not None:
        gam.check(tag + ' gamma')
        check_bits(gam.t, torch.where(keep, gamma.float().to(dt), sent), torch.ones(1, dtype=torch.bool), tag + ' gamma (bit-equal; sentinel outside)')
    report('modulate', tag, worst)


MOD_RECTS = [(16, 16), (32, 8), (8, 8)]


def group_modulate(dev, dt):
    maps = [('5x5', np.full((1, 5, 5), 2, dtype=np.uint8)),
            ('21x19', R.salt(np.full((2, 21, 19), 1, dtype=np.uint8), [(0, 10, 9), (1, 3, 15)])),
            ('48x64', R.salt(band_labels(2, 48, 64), [(0, 5, 5), (1, 40, 60)]))]
    i = 0
    for C_ in ((8, 64, 24) if dt == torch.bfloat16 else (4, 12)):
        for tw, th in MOD_RECTS:
            for mname, label in maps:
                n_uni = len(R.classify_ref(label, label.shape[1], label.shape[2], tw, th)[2])
                run_modulate(mname, dt, label, C_, tw, th, lrelu_on=i % 2 == 0, with_gamma=(i // 2) % 2 == 0, x_up=mname == '48x64' and i % 4 < 2,
                             banked=(i // 3) % 2 == 0, short=n_uni >= 3 and i % 3 != 1, dev=dev, seed=2000 + i)
                i += 1
    if dt == torch.float32:          # 257 channel groups: two trips of a thread over the groups, one pixel at a time
        one = np.full((1, 8, 8), 3, dtype=np.uint8)
        run_modulate('8x8', dt, one, 1028, 8, 8, True, True, True, True, False, dev, 2100)
        run_modulate('8x8', dt, one, 1028, 16, 16, False, True, False, False, False, dev, 2101)
    else:                            # 2178 uniform rectangles against a grid of 2048 blocks
        big = np.stack([np.full((264, 264), 1, dtype=np.uint8), np.full((264, 264), 3, dtype=np.uint8)])
        run_modulate('2178 rectangles', dt, big, 8, 8, 8, True, True, True, True, False, dev, 2200)


# ---- sums
def run_sums(name, dt, label, C2, mode, dev, seed):
    """mode: 'all' | 'subset' (counts[1] below the list) | 'zero' (counts[1] = 0)"""
    L, lb = lib()
    N, H, W = label.shape
    cls, _, _ = R.classify_ref(label, H, W, 16, 16)
    _, ui = R.lists_bwd_ref(cls, N, H // 16, W // 16)
    assert len(ui) > 0
    count = {'all': len(ui), 'subset': (len(ui) * 9 + 15) // 16, 'zero': 0}[mode]
    assert mode != 'subset' or 0 < count < len(ui)
    g = gen(seed)
    dgb = torch.randn(N, H, W, C2, generator=g).to(dt)
    R0 = torch.randn(R.UNI_REPLICAS, NCLS, 9, C2, generator=g) * 4.0
    ref, A = R.sums_ref(dgb.double(), cls, ui[:count], H, W, NCLS)
    near = torch.from_numpy(R.neighbourhood_mask(ui[:count], N, H, W))[..., None]
    dgb_d = torch.where(near, dgb, torch.full((1,), float('nan'), dtype=dt)).to(dev)      # NaN wherever the call has no business
    Rg = Guarded(tuple(R0.shape), torch.float32, dev, R0)
    clsd, uid, cnt = torch.from_numpy(cls).to(dev), i32(ui, dev), i32([N * (H // 16) * (W // 16) - len(ui), count], dev)
    L.check(lb.s2e_spade_uniform_sums(code_of(dt), dgb_d.data_ptr(), N, H, W, C2, NCLS, clsd.data_ptr(), uid.data_ptr(), cnt.data_ptr(), Rg.ptr(),
                                      stream()), 's2e_spade_uniform_sums')
    tag = '%s %dx%dx%dx%d, %d of %d uniform-interior listed (%d blocks)' % (name, N, H, W, C2, count, len(ui), N * (H // 16 - 2) * (W // 16 - 2))
    Rg.check(tag + ' R')
    got = Rg.t.cpu()
    assert bool(torch.isfinite(got).all()), '%s: a NaN from outside the listed neighbourhoods reached R' % tag
    if count == 0:
        check_bits(got, R0, torch.ones(1, dtype=torch.bool), tag + ' R')
        report('sums', tag + ': R bit-unchanged', None)
        return
    worst = R.check_close((got.double() - R0.double()).sum(0), ref, A + R0.double().abs().sum(0), tag + ' R (replicas folded)', rel=0.0)
    report('sums', tag, worst)


def group_sums(dev, dt):
    one = np.full((1, 48, 48), 2, dtype=np.uint8)
    b96, b128 = R.block_labels(1, 96, 96), R.block_labels(2, 128, 128)
    i = 0
    for C2 in (128, 256, 512, 1024):
        run_sums('one class', dt, one, C2, 'all', dev, 3000 + i)
        run_sums('block', dt, b96, C2, 'all' if C2 != 256 else 'subset', dev, 3100 + i)
        i += 1
    run_sums('block', dt, b128, 128, 'all', dev, 3200)
    run_sums('block', dt, b128, 256, 'subset', dev, 3201)
    run_sums('block', dt, b96, 128, 'subset', dev, 3202)
    run_sums('block', dt, b96, 512, 'zero', dev, 3203)
    run_sums('block', dt, b128, 128, 'zero', dev, 3204)


# ---- grads
class Job:
    """one s2e_spade_uni_job: its device operands, guarded targets and fp64 reference.  R_dev: None (random, every replica filled), or
    the device tensor s2e_spade_uniform_sums wrote (then R64 / Rabs64 are the reference's folded sums)."""

    def __init__(self, dev, seed, C2, nh, ncls, cl, act_bf16, gb, dw_sh=True, db_sh=True, R_dev=None, R64=None, Rabs64=None, w=None, w_sh=None, b_sh=None):
        self.C2, self.nh, self.ncls, self.cl, self.act_bf16, self.gb = C2, nh, ncls, cl, act_bf16, gb
        g = gen(seed)
        if R_dev is None:
            Rr = torch.randn(R.UNI_REPLICAS, ncls, 9, C2, generator=g)
            R_dev, R64, Rabs64 = Rr.to(dev), Rr.double().sum(0), Rr.double().abs().sum(0)
        self.R = R_dev
        w = torch.randn(C2, nh, 3, 3, generator=g) * (9 * nh) ** -0.5 if w is None else w
        w_sh = R.grid_weights((nh, ncls, 3, 3), g) if w_sh is None else w_sh
        b_sh = R.grid_weights((nh,), g) if b_sh is None else b_sh
        self.ref = R.grads_ref(R64, Rabs64, w.double(), w_sh, b_sh, torch.bfloat16 if act_bf16 else torch.float32)
        self.w = (w.permute(0, 2, 3, 1).contiguous() if cl else w.contiguous()).to(dev)      # channels-last: memory (co, ky, kx, k)
        self.strides = (9 * nh, 1, nh) if cl else (9 * nh, 9, 1)                              # (co, k, tap), in elements
        self.w_sh, self.b_sh = w_sh.float().to(dev), b_sh.float().to(dev)
        self.A = Guarded((ncls, nh), torch.float32, dev, 0.0)
        self.start, self.out = {}, {}
        shapes = {'dw_sh': (nh, ncls, 3, 3), 'db_sh': (nh,), 'dw_gb': (C2, nh, 3, 3), 'db_gb': (C2,)}
        have = {'dw_sh': dw_sh, 'db_sh': db_sh, 'dw_gb': gb in ('both', 'dw_only'), 'db_gb': gb == 'both'}
        for k, shp in shapes.items():
            if not have[k]:
                continue
            s0 = torch.randn(*shp, generator=g) * 0.5 + 0.25
            mem = s0.permute(0, 2, 3, 1).contiguous() if (k == 'dw_gb' and cl) else s0
            self.start[k], self.out[k] = s0, Guarded(tuple(mem.shape), torch.float32, dev, mem)

    def fill(self, a):
        p = lambda k: self.out[k].ptr() if k in self.out else None
        a.R, a.A, a.w_gb = self.R.data_ptr(), self.A.ptr(), self.w.data_ptr()
        a.w_sc, a.w_sk, a.w_st = self.strides
        a.w_sh, a.b_sh = self.w_sh.data_ptr(), self.b_sh.data_ptr()
        a.dw_sh, a.db_sh, a.dw_gb, a.db_gb = p('dw_sh'), p('db_sh'), p('dw_gb'), p('db_gb')
        a.C2, a.nh, a.ncls, a.act_bf16 = self.C2, self.nh, self.ncls, int(self.act_bf16)

    def tag(self):
        return 'C2=%d nh=%d ncls=%d w_gb %s act_bf16=%d dw_gb=%s db_gb=%s dw_sh=%s db_sh=%s' % (
            self.C2, self.nh, self.ncls, 'channels-last (9nh, 1, nh)' if self.cl else 'torch (9nh, 9, 1)', self.act_bf16,
            *('yes' if k in self.out else 'NULL' for k in ('dw_gb', 'db_gb', 'dw_sh', 'db_sh')))

    def got(self, k):
        t = self.out[k].t.double().cpu()
        return t.permute(0, 3, 1, 2).contiguous() if (k == 'dw_gb' and self.cl) else t

    def check(self, what, refs=None, acc_sh=None, with_A=True):
        """refs: {name: increment} replacing the restated algebra's (the chain case's autograd); the |.| twins stay"""
        acc_sh = R.grads_acc(self.C2) if acc_sh is None else acc_sh
        self.A.check(what + ' A')
        worst = 0.0
        if with_A:
            worst = R.check_close(self.A.t.double().cpu(), self.ref['A'][0], self.ref['A'][1], what + ' A', rel=0.0, acc=acc_sh)
        for k, buf in self.out.items():
            buf.check('%s %s' % (what, k))
            ref = self.ref[k][0] if refs is None else refs[k]
            worst = max(worst, R.check_close(self.got(k), ref, self.ref[k][1], '%s %s' % (what, k), rel=0.0,
                                             acc=acc_sh if k in ('dw_sh', 'db_sh') else R.C_ACC, start=self.start[k].double()))
        return worst


def launch_grads(jobs):
    L, lb = lib()
    arr = (L.SpadeUniJob * len(jobs))()
    for a, j in zip(arr, jobs):
        j.fill(a)
    L.check(lb.s2e_spade_uniform_grads(C.byref(arr), len(jobs), stream()), 's2e_spade_uniform_grads')
    torch.cuda.synchronize()


# (call, [job]): gb = which of dw_gb / db_gb the job carries ('both', 'dw_only': db_gb NULL, None: both NULL)
GRADS_CALLS = [
    ('1 job', [dict(C2=128, nh=128, ncls=4, cl=False, act_bf16=1, gb='both')]),
    ('3 jobs', [dict(C2=12, nh=40, ncls=1, cl=True, act_bf16=0, gb='both'),
                dict(C2=128, nh=64, ncls=3, cl=False, act_bf16=1, gb=None),
                dict(C2=1024, nh=128, ncls=4, cl=True, act_bf16=1, gb='dw_only')]),
    ('3 jobs, no dw_gb', [dict(C2=1024, nh=128, ncls=4, cl=False, act_bf16=0, gb=None),
                          dict(C2=12, nh=64, ncls=4, cl=True, act_bf16=1, gb=None, dw_sh=False),
                          dict(C2=128, nh=40, ncls=3, cl=False, act_bf16=1, gb=None, db_sh=False)]),
    ('16 jobs', [dict(C2=(12, 128, 1024)[j % 3], nh=(128, 64, 40)[(j // 3) % 3], ncls=(4, 3, 1)[(j // 2) % 3], cl=j % 2 == 1, act_bf16=(j // 4) % 2,
                      gb=('both', None, 'dw_only', 'both')[j % 4], dw_sh=j % 5 != 2, db_sh=j % 7 != 3) for j in range(16)])]


def group_grads(dev, dt):
    for ci, (cname, specs) in enumerate(GRADS_CALLS):
        jobs = [Job(dev, 4000 + 100 * ci + j, **s) for j, s in enumerate(specs)]
        launch_grads(jobs)
        for j, job in enumerate(jobs):
            what = 'grads %s #%d %s' % (cname, j, job.tag())
            report('grads', what, job.check(what))


# ---- chain: classify -> lists_bwd -> sums -> grads against autograd
def group_chain(dev, dt):
    assert dt == torch.bfloat16
    L, lb = lib()
    N, H, W, C2, nh = 2, 128, 128, 128, 128
    label = R.salt(R.block_labels(N, H, W), [(0, 24, 24), (1, 31, 90), (1, 100, 47)])
    cls_ref, dense_ref, uni_ref = R.classify_ref(label, H, W, 16, 16)
    work_ref, ui_ref = R.lists_bwd_ref(cls_ref, N, H // 16, W // 16)
    assert len(ui_ref) > R.UNI_REPLICAS, len(ui_ref)
    total = cls_ref.size
    lab = torch.from_numpy(label).to(dev)
    cls = Guarded((total,), torch.uint8, dev, raw_fill=POISON_U8)
    lists = [Guarded((total,), torch.int32, dev, SENT_I) for _ in range(4)]
    cnt, cntb = Guarded((2,), torch.int32, dev, SENT_I), Guarded((2,), torch.int32, dev, SENT_I)
    L.check(lb.s2e_label_rect_classify(lab.data_ptr(), N, H, W, H, W, 16, 16, cls.ptr(), lists[0].ptr(), lists[1].ptr(), cnt.ptr(), stream()),
            's2e_label_rect_classify')
    L.check(lb.s2e_label_rect_lists_bwd(cls.ptr(), N, H // 16, W // 16, lists[2].ptr(), lists[3].ptr(), cntb.ptr(), stream()), 's2e_label_rect_lists_bwd')
    g = gen(5000)
    dgb = torch.randn(N, H, W, C2, generator=g).to(dt)
    dgb_d = dgb.to(dev)
    Rg = Guarded((R.UNI_REPLICAS, NCLS, 9, C2), torch.float32, dev, 0.0)
    L.check(lb.s2e_spade_uniform_sums(code_of(dt), dgb_d.data_ptr(), N, H, W, C2, NCLS, cls.ptr(), lists[3].ptr(), cntb.ptr(), Rg.ptr(), stream()),
            's2e_spade_uniform_sums')
    R64, Rabs64 = R.sums_ref(dgb.double(), cls_ref, ui_ref, H, W, NCLS)
    w = torch.randn(C2, nh, 3, 3, generator=g) * (9 * nh) ** -0.5
    w_sh, b_sh = R.grid_weights((nh, NCLS, 3, 3), g), R.grid_weights((nh,), g)
    job = Job(dev, 5001, C2, nh, NCLS, False, 1, 'both', R_dev=Rg.t, R64=R64, Rabs64=Rabs64, w=w, w_sh=w_sh, b_sh=b_sh)
    launch_grads([job])
    for b_, nm in [(cls, 'cls'), (cnt, 'counts'), (cntb, 'backward counts'), (Rg, 'R')] + [(l, 'list %d' % i) for i, l in enumerate(lists)]:
        b_.check('chain %s' % nm)
    assert np.array_equal(cls.t.cpu().numpy(), cls_ref), 'chain: cls differs from the reference'
    c, cb = cnt.t.cpu().tolist(), cntb.t.cpu().tolist()
    for l, want, n, nm in ((lists[0], dense_ref, c[0], 'dense'), (lists[1], uni_ref, c[1], 'uniform'), (lists[2], work_ref, cb[0], 'work'),
                           (lists[3], ui_ref, cb[1], 'uniform-interior')):
        check_list(l, want, n, 'chain %s' % nm)
    auto = R.branch_autograd(label, w_sh, b_sh, w.double(), dgb.double(), R.rect_pixels(ui_ref, N, H, W, 16, 16), torch.bfloat16)
    what = 'chain 2x128x128 block map + 3 salted pixels, %d uniform-interior, bf16 C2=128 nh=128, against autograd' % len(ui_ref)
    # (A is the kernels' scratch and has no autograd counterpart: dw_sh and db_sh are its masked copies.  The chain of roundings runs
    #  through the sums and the gemv: _spade_sparse_ref.CHAIN['chain_sh'] <= 256, so C_ACC.)
    worst = R.check_close(Rg.t.double().cpu().sum(0), R64, Rabs64, 'chain R (replicas folded)', rel=0.0)
    report('chain', what, max(worst, job.check(what, refs=auto, acc_sh=R.C_ACC, with_A=False)))


GROUPS = {'classify': group_classify, 'lists_bwd': group_lists_bwd, 'table': group_table, 'modulate': group_modulate, 'sums': group_sums,
          'grads': group_grads, 'chain': group_chain}
TYPED = ('table', 'modulate', 'sums', 'chain')          # the groups that need --dtype bf16 | fp32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--groups', required=True)
    ap.add_argument('--dtype', default='none', choices=['bf16', 'fp32', 'none'])
    args = ap.parse_args()
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    dev = torch.device('cuda', 0)
    lib()
    dt = DTYPES.get(args.dtype)
    for name in args.groups.split(','):
        assert dt is not None or name not in TYPED, 'group %s needs --dtype' % name
        GROUPS[name](dev, dt)
    print('spade sparse ok: %d checks, groups %s (%s)' % (len(RESULTS), args.groups, args.dtype), flush=True)


if __name__ == '__main__':
    main()
