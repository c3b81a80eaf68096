"""The segmenter's paired augmentation without a GPU: the restatement (tests/_seg_augment_ref.py) against literal facts and
a line's cover against exact rationals; `AugmentRule`'s one draw, its identities, its tables and its refusals; the order of the trainer's
draws with CPU stand-ins for the ops; every refused call of the C ABI with its code and message; the command line.  Every comparison
is == on bytes, integers or float bit patterns."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _seg_augment_ref as R
import _segment_ref as SR

P = 4096                                                      # a dummy non-null pointer: must never reach a kernel
ARG, UNSUPPORTED = -1, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 65536
IDENT = [Q, 0, 0, 0, Q, 0]
STRONG = dict(rotate=180.0, scale=4.0, translate=1.0, gamma=3.0, contrast=0.9, brightness=0.5, lines=8)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ops():
    from seg2eye_amd.ops import augment
    return augment


# ------------------------------------------------------------------------------------------------ the restatement alone
@pytest.mark.parametrize('shape', [(1, 1), (1, 9), (9, 1), (5, 7), (12, 11)], ids=lambda s: '%dx%d' % s)
def test_restated_warp_literal_facts(shape):
    H, W = shape
    img, lab = (a[0] for a in R.planes((1, H, W), 5))
    # identity
    assert np.array_equal(R.warp_frame(img, IDENT), img) and np.array_equal(R.warp_label(lab, IDENT), lab)
    # mirror along x, and a half turn
    mirror = [-Q, 0, (W - 1) << 16, 0, Q, 0]
    assert np.array_equal(R.warp_frame(img, mirror), np.flip(img, 1)) and np.array_equal(R.warp_label(lab, mirror), np.flip(lab, 1))
    turn = [-Q, 0, (W - 1) << 16, 0, -Q, (H - 1) << 16]
    assert np.array_equal(R.warp_frame(img, turn), np.flip(img, (0, 1))) and np.array_equal(R.warp_label(lab, turn), np.flip(lab, (0, 1)))
    # an integer shift: the plane shifted, its edge replicated
    for sx, sy in ((2, 0), (-3, 1), (0, -2), (100, -100)):
        ys, xs = np.clip(np.arange(H) + sy, 0, H - 1), np.clip(np.arange(W) + sx, 0, W - 1)
        A = [Q, 0, sx * Q, 0, Q, sy * Q]
        assert np.array_equal(R.warp_frame(img, A), img[ys][:, xs]) and np.array_equal(R.warp_label(lab, A), lab[ys][:, xs])
    # half a pixel along x: the rounded mean of two neighbours; the label takes the right one (0.5 rounds up)
    p = img.astype(np.int64)
    right = np.minimum(np.arange(W) + 1, W - 1)
    half = [Q, 0, 0x8000, 0, Q, 0]
    assert np.array_equal(R.warp_frame(img, half), (p + p[:, right] + 1) >> 1) and np.array_equal(R.warp_label(lab, half), lab[:, right])
    # sources far outside the plane stay in bounds: every extreme of int32, for every coefficient
    big = [2 ** 31 - 1, -2 ** 31]
    for A in ([a, b, c, d, e, f] for a in big for b in big for c in big for d in big for e in big for f in big):
        sx, sy = R.source(A, H, W)
        assert sx.min() >= 0 and sx.max() <= (W - 1) << 16 and sy.min() >= 0 and sy.max() <= (H - 1) << 16
        out = R.warp_frame(img, A)
        assert out.min() >= 0 and out.max() <= 255
    assert np.array_equal(R.warp_label(lab, [2 ** 31 - 1] * 6), np.full((H, W), lab[-1, -1]))
    assert np.array_equal(R.warp_frame(img, [-2 ** 31] * 6)[-1, -1:], img[0, :1])


LINES = {'zero_length': (3, 4, 3, 4, 3, 9), 'zero_width': (0, 0, 10, 8, 0, 9), 'horizontal': (2, 5, 11, 5, 3, 200), 'vertical': (6, -3, 6, 40, 2, 1),
         'diagonal': (0, 0, 12, 10, 1, 7), 'wide_diagonal': (12, 0, 0, 10, 4, 255), 'beyond_the_clamp': (-9000, 5, 9000, 5, 300, 256 + 17),
         'negative_width': (0, 0, 5, 5, -2, 3)}


@pytest.mark.parametrize('name', sorted(LINES))
def test_restated_line_cover_is_the_exact_rational_one(name):
    H, W = 11, 13
    line = LINES[name]
    hit, value = R.line_cover(line, H, W)
    want = np.array([[R.covered_exact(line, x, y) for x in range(W)] for y in range(H)])
    assert np.array_equal(hit, want) and value == (line[5] & 255)
    if name in ('zero_length', 'zero_width', 'negative_width'):
        assert not hit.any()
    if name == 'horizontal':                                   # width 3: the row and its two neighbours, between the end points
        assert np.array_equal(np.argwhere(hit), [[y, x] for y in (4, 5, 6) for x in range(2, 12)])
    if name == 'vertical':                                     # width 2: |x - 6| <= 1
        assert np.array_equal(np.argwhere(hit), [[y, x] for y in range(H) for x in (5, 6, 7)])
    if name == 'diagonal':
        assert hit[0, 0] and hit[10, 12] and hit[5, 6] and not hit[0, 2]
    if name == 'beyond_the_clamp':                             # the ends clamp to -4096 and 8191, the width to 255: everything, value & 255
        assert hit.all() and value == 17


def test_restated_pairs_apply_lines_in_order_to_the_frame_only():
    img, lab = R.planes((2, 9, 12), 3)
    p = R.identity(2, lines=2)
    p.lines[0] = [(0, 4, 11, 4, 1, 50), (5, 0, 5, 8, 1, 60)]
    p.lines[1, 1] = (0, 0, 11, 8, 2, 300)
    xf, xb, y = R.augment_pairs(img, lab, p)
    assert np.array_equal(y, lab)
    want = img.copy()
    want[0, 4, :] = 50
    want[0, :, 5] = 60                                         # the later line wins the crossing
    assert np.array_equal(xb[0], want[0]) and xb[0, 4, 5] == 60 and (xb[1] == 44).sum() >= 12 and np.array_equal(_bits(xf), _bits(p.lut_f32[0][xb]))
    assert R.augment_pairs(None, lab, p)[:2] == (None, None) and R.augment_pairs(img, None, p)[2] is None


# ------------------------------------------------------------------------------------------------ AugmentRule
class _CountingRng:
    def __init__(self, seed):
        self.rng, self.calls = np.random.RandomState(seed), []

    def rand(self, *shape):
        self.calls.append(shape)
        return self.rng.rand(*shape)


@pytest.mark.parametrize('kw', [{}, STRONG, dict(prob=0.5, **STRONG), dict(lines=3), dict(rotate=10.0)], ids=['off', 'strong', 'half', 'lines', 'rotate'])
def test_rule_makes_one_rand_call_and_is_the_restated_draw(kw):
    A = _ops()
    for n, h, w in ((1, 8, 8), (5, 320, 200), (16, 64, 40)):
        rng = _CountingRng(n)
        got = A.AugmentRule(**kw).draw(rng, n, h, w)
        assert rng.calls == [(n, 57)]
        want = R.draw(np.random.RandomState(n), n, h, w, **kw)
        assert got.affine.dtype == np.int32 and got.affine.shape == (n, 6) and np.array_equal(got.affine, want.affine)
        assert got.lut_f32.dtype == np.float32 and np.array_equal(_bits(got.lut_f32), _bits(want.lut_f32))
        assert got.lut_u8.dtype == np.uint8 and np.array_equal(got.lut_u8, want.lut_u8)
        if kw.get('lines'):
            assert got.lines.dtype == np.int32 and got.lines.shape == (n, kw['lines'], 6) and np.array_equal(got.lines, want.lines)
        else:
            assert got.lines is None and want.lines is None


def test_turning_one_augmentation_off_does_not_shift_anothers_stream():
    A = _ops()
    full = A.AugmentRule(**STRONG).draw(np.random.RandomState(4), 6, 64, 40)
    geo = A.AugmentRule(rotate=180.0, scale=4.0, translate=1.0).draw(np.random.RandomState(4), 6, 64, 40)
    photo = A.AugmentRule(gamma=3.0, contrast=0.9, brightness=0.5).draw(np.random.RandomState(4), 6, 64, 40)
    occ = A.AugmentRule(lines=8).draw(np.random.RandomState(4), 6, 64, 40)
    assert np.array_equal(full.affine, geo.affine) and np.array_equal(_bits(full.lut_f32), _bits(photo.lut_f32)) and np.array_equal(full.lines, occ.lines)
    assert (geo.affine != IDENT).any() and (photo.lut_u8 != np.arange(256)).any() and (occ.lines[..., 4] > 0).any() and (occ.lines[..., 4] == 0).any()


def test_zero_amplitudes_and_zero_prob_are_exact_identities():
    A = _ops()
    from seg2eye_amd.ops.preprocess import normalize_lut
    norm = _bits(normalize_lut().numpy())
    for rule in (A.AugmentRule(), A.AugmentRule(prob=0.0, **STRONG)):
        p = rule.draw(np.random.RandomState(1), 7, 320, 200)
        assert p.affine.tolist() == [IDENT] * 7
        assert all(np.array_equal(_bits(row), norm) for row in p.lut_f32) and all(np.array_equal(row, np.arange(256)) for row in p.lut_u8)
        assert p.lines is None or not p.lines.any()
        assert rule.is_identity()
    assert not A.AugmentRule(lines=1).is_identity()
    q = A.identity_params(3, lines=2)
    assert q.affine.tolist() == [IDENT] * 3 and q.lines.shape == (3, 2, 6) and not q.lines.any() and np.array_equal(_bits(q.lut_f32[2]), norm)
    # the identity tables are the special case, not the formula: the formula's fp32 rounding differs from normalize_lut() somewhere or nowhere,
    # the bits returned are normalize_lut()'s either way
    f, b = A.photometric_luts(1.0, 1.0, 0.0)
    assert np.array_equal(_bits(f), norm) and np.array_equal(b, np.arange(256))


def test_tables_are_monotone_and_in_range():
    A = _ops()
    p = A.AugmentRule(gamma=4.0, contrast=0.999, brightness=1.0).draw(np.random.RandomState(2), 64, 16, 16)
    assert (np.diff(p.lut_f32.astype(np.float64), axis=1) >= 0).all() and p.lut_f32.min() >= -1.0 and p.lut_f32.max() <= 1.0
    assert (np.diff(p.lut_u8.astype(np.int64), axis=1) >= 0).all()
    assert len({row.tobytes() for row in p.lut_u8}) > 32       # (tables that saturate everywhere coincide; most frames get their own)
    f, b = A.photometric_luts(2.0, 0.5, 0.25)
    c = np.clip(0.5 * (np.arange(256) / 255.0) ** 2.0 + 0.25, 0, 1)
    assert np.array_equal(_bits(f), _bits(((c - 0.5) / 0.5).astype(np.float32))) and np.array_equal(b, np.rint(255 * c).astype(np.uint8))


@pytest.mark.parametrize('kw', [dict(prob=-0.1), dict(prob=1.1), dict(rotate=-1), dict(rotate=180.5), dict(scale=0.9), dict(scale=4.1), dict(translate=-0.1),
                                dict(translate=1.5), dict(gamma=0.5), dict(gamma=5), dict(contrast=1.0), dict(contrast=-0.2), dict(brightness=1.2),
                                dict(brightness=-1), dict(lines=9), dict(lines=-1), dict(lines=1.5), dict(rotate='10'), dict(scale=float('nan')), dict(prob=None)],
                         ids=lambda kw: '%s=%s' % next(iter(kw.items())))
def test_rule_refuses_values_out_of_range_naming_the_flag(kw):
    with pytest.raises(ValueError, match='--aug_%s' % next(iter(kw))):
        _ops().AugmentRule(**kw)


def test_rule_accepts_the_ends_of_every_range():
    A = _ops()
    r = A.AugmentRule(prob=1, rotate=180, scale=4, translate=1, gamma=4, contrast=0.999, brightness=1, lines=8)
    assert (r.rotate, r.scale, r.lines) == (180.0, 4.0, 8) and 'rotate=180.0' in repr(r)
    A.AugmentRule(prob=0, rotate=0, scale=1, translate=0, gamma=1, contrast=0, brightness=0, lines=0)


@pytest.mark.parametrize('hw', [(320, 200), (64, 40), (9, 4096), (1, 1)], ids=lambda s: '%dx%d' % s)
def test_centre_plus_shift_reads_the_centre(hw):
    """The output point centre + shift has the source centre, to within one unit of Q16 (1 / 65536 of a pixel) in either coordinate:
    A2 and A5 are formed from the rounded A0 .. A4."""
    h, w = hw
    u = np.random.RandomState(9).rand(200, 57)
    p = _ops().AugmentRule(rotate=180.0, scale=4.0, translate=1.0).draw(np.random.RandomState(9), 200, h, w)
    s = 2 * u - 1
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    X, Y = cx + s[:, 3] * 1.0 * w, cy + s[:, 4] * 1.0 * h
    A = p.affine.astype(np.float64)
    inside = (np.abs(A[:, 2]) < 2 ** 31 - 1) & (np.abs(A[:, 5]) < 2 ** 31 - 1)          # (not clipped to int32: only at sides near 4096)
    assert inside.mean() > 0.5
    ex, ey = A[:, 0] * X + A[:, 1] * Y + A[:, 2] - cx * Q, A[:, 3] * X + A[:, 4] * Y + A[:, 5] - cy * Q
    assert np.abs(ex[inside]).max() <= 1.0 and np.abs(ey[inside]).max() <= 1.0
    # the linear part is a rotation over the scale: A3 = -A1, A4 = A0, and A0^2 + A1^2 = (65536 / s)^2 to the rounding
    assert np.array_equal(p.affine[:, 3], -p.affine[:, 1]) and np.array_equal(p.affine[:, 4], p.affine[:, 0])
    scale = np.exp(s[:, 2] * np.log(4.0))
    assert np.abs(np.hypot(A[:, 0], A[:, 1]) - Q / scale).max() <= 1.0


# ------------------------------------------------------------------------------------------------ the trainer's draws
class _StubAdam:
    def __init__(self, params, lr, betas):
        self.opt = torch.optim.Adam(params, lr=lr, betas=betas)

    def zero_grad(self):
        self.opt.zero_grad()

    def step(self):
        self.opt.step()


class _SegNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.k = torch.nn.Parameter(torch.tensor(1.0))

    def forward(self, x):                                       # (n, 1, h, w) -> logits (n, h, w, 4)
        grey = torch.tensor(SR.GREY / 255.0 * 2 - 1, dtype=torch.float32)
        return -self.k * (x.permute(0, 2, 3, 1) - grey) ** 2


@pytest.fixture(scope='module')
def store():
    return {'train': SR.learnable_store(H=64, W=40)[0]['train']}


@pytest.fixture()
def recorded(monkeypatch, store):
    """CPU stand-ins for the ops and the optimiser that record, per call, the batch's sample ids, the flip bytes and the parameters."""
    from seg2eye_amd import optim
    from seg2eye_amd.ops import augment, preprocess, segment
    ids = {key: {np.asarray(g[key][i]).tobytes(): (u, i) for u, g in store['train'].items() for i in range(g[key].shape[0])} for key in ('images_ss', 'labels_ss')}
    events = []

    def resize_bicubic_u8(f, Ho, Wo, flip, return_u8=False):
        events.append(('frames', [ids['images_ss'][v.numpy().tobytes()] for v in f], flip.tolist(), (Ho, Wo), return_u8))
        small = f[:, ::8, ::5].contiguous()
        return (small.float() / 127.5 - 1, small) if return_u8 else small.float() / 127.5 - 1

    def resize_nearest_u8(l, Ho, Wo, flip):
        events.append(('labels', [ids['labels_ss'][v.numpy().tobytes()] for v in l], flip.tolist(), (Ho, Wo)))
        return l[:, ::8, ::5].contiguous()

    def augment_pairs(img, lab, params, want_f32=True, want_u8=False):
        assert img.dtype == torch.uint8 and lab.dtype == torch.uint8 and img.shape == lab.shape and want_f32 and not want_u8
        events.append(('augment', tuple(img.shape), [None if a is None else a.tolist() for a in params]))
        xf, _, y = R.augment_pairs(img.numpy(), lab.numpy(), R.Params(*params))
        return torch.from_numpy(xf), None, torch.from_numpy(y)
    monkeypatch.setattr(preprocess, 'resize_bicubic_u8', resize_bicubic_u8)
    monkeypatch.setattr(preprocess, 'resize_nearest_u8', resize_nearest_u8)
    monkeypatch.setattr(augment, 'augment_pairs', augment_pairs)
    monkeypatch.setattr(segment, 'seg_cross_entropy', SR.ce_torch)
    monkeypatch.setattr(optim, 'FlatAdam', _StubAdam)
    return events


@pytest.mark.parametrize('no_flip', [True, False], ids=['no_flip', 'flip'])
def test_trainer_draws_the_permutation_then_the_flip_then_the_rule(recorded, store, no_flip):
    """18 samples in batches of 4 (the last of an epoch holds 2), two epochs: per epoch permutation(18); per batch rand(len(batch)) for
    the flip, only when flips are on, then the rule's rand(len(batch), 57)."""
    from seg2eye_amd import segment
    A = _ops()
    kw = dict(prob=0.7, rotate=20.0, scale=1.3, translate=0.1, gamma=1.5, contrast=0.3, brightness=0.1, lines=3)
    opt = segment.seg_options(seg_hw=(8, 8), batchSize=4, niter=2, seed=11, no_flip=no_flip)
    _, hist = segment.train_segmenter(store, opt, net=_SegNet(), device='cpu', save=False, verbose=False, augment=A.AugmentRule(**kw))
    samples = segment.labelled_samples(store, 'train')
    rng, want = np.random.RandomState(11), []
    for _ in range(2):
        order = rng.permutation(18)
        for b0 in range(0, 18, 4):
            batch = [samples[j] for j in order[b0:b0 + 4]]
            flip = [0] * len(batch) if no_flip else (rng.rand(len(batch)) < 0.5).astype(np.uint8).tolist()
            p = R.draw(rng, len(batch), 8, 8, **kw)
            want += [('frames', batch, flip, (8, 8), True), ('labels', batch, flip, (8, 8)), ('augment', (len(batch), 8, 8), [a.tolist() for a in p])]
    assert recorded == want and len(hist['loss']) == 10 and np.isfinite(hist['loss']).all()


@pytest.mark.parametrize('no_flip', [True, False], ids=['no_flip', 'flip'])
def test_augment_none_is_the_call_without_the_keyword(recorded, store, no_flip):
    from seg2eye_amd import segment
    opt = segment.seg_options(seg_hw=(8, 8), batchSize=4, niter=2, seed=5, no_flip=no_flip, lambda_dice=0.0)
    _, a = segment.train_segmenter(store, opt, net=_SegNet(), device='cpu', save=False, verbose=False)
    first = list(recorded)
    del recorded[:]
    _, b = segment.train_segmenter(store, opt, net=_SegNet(), device='cpu', save=False, verbose=False, augment=None)
    assert recorded == first and a['loss'] == b['loss'] and len(first) == 20
    assert all(e[0] in ('frames', 'labels') for e in first) and all(e[4] is False for e in first if e[0] == 'frames')


# ------------------------------------------------------------------------------------------------ declared, exported, bound, built
def test_new_symbol_is_declared_exported_and_bound():
    from seg2eye_amd import _lib, build, ops
    header = open(os.path.join(ROOT, 'include', 'seg2eye_hip.h')).read()
    assert re.search(r'\bs2e_augment_pairs\(', header)
    assert 's2e_augment_pairs' in _lib.SIGNATURES and hasattr(_lib.lib(), 's2e_augment_pairs')
    assert 'seg_augment.hip' in build.SOURCES and os.path.exists(os.path.join(build.CSRC, 'seg_augment.hip'))
    assert ops.augment_pairs is ops.augment.augment_pairs and ops.AugmentRule is ops.augment.AugmentRule


# ------------------------------------------------------------------------------------------------ refused calls
def _call(img=P, lab=P + 4096, M=2, H=8, W=8, affine=P + 8192, lines=None, L=0, lut_f32=P + 12288, lut_u8=P + 16384, out_f32=P + 20480,
          out_u8=P + 24576, out_lab=P + 28672):
    return (img, lab, M, H, W, affine, lines, L, lut_f32, lut_u8, out_f32, out_u8, out_lab, None)


def _refused(args, code, text):
    from seg2eye_amd import _lib
    L = _lib.lib()
    assert L.s2e_augment_pairs(*args) == code, args
    msg = L.s2e_last_error().decode()
    assert msg.startswith('s2e_augment_pairs: ') and text in msg, msg


def test_refused_calls_of_augment_pairs():
    _refused(_call(affine=None), ARG, 'affine is NULL')
    _refused(_call(out_f32=None, out_u8=None, out_lab=None), ARG, 'no output')
    _refused(_call(img=None), ARG, 'an image output without img')
    _refused(_call(img=None, out_f32=None), ARG, 'an image output without img')
    _refused(_call(lab=None), ARG, 'out_lab without lab')
    for kw in (dict(M=0), dict(M=-3), dict(H=0), dict(W=-1)):
        _refused(_call(**kw), ARG, 'every size must be at least 1')
    _refused(_call(L=1), ARG, 'L=1 lines without the lines array')
    _refused(_call(L=-1, lines=P), ARG, 'L=-1')
    _refused(_call(lut_f32=None), ARG, 'out_f32 without lut_f32')
    _refused(_call(lut_u8=None), ARG, 'out_u8 without lut_u8')
    for kw in (dict(affine=P + 2), dict(lines=P + 1, L=1), dict(lut_f32=P + 3), dict(out_f32=P + 20482)):
        _refused(_call(**kw), ARG, '4-byte aligned')
    for kw in (dict(out_u8=P), dict(out_lab=P + 4096), dict(out_u8=P + 4096), dict(out_lab=P), dict(out_f32=P), dict(out_f32=P + 4096)):
        _refused(_call(**kw), ARG, 'an output is its own input')
    _refused(_call(H=4097), UNSUPPORTED, 'H=4097 W=8 (each at most 4096)')
    _refused(_call(W=4097), UNSUPPORTED, 'H=8 W=4097 (each at most 4096)')
    _refused(_call(L=9, lines=P), UNSUPPORTED, 'L=9 (at most 8 lines per frame)')
    # the order: the pointers, the sizes, the lines, the tables, the alignment, the aliases, then the two limits
    _refused(_call(affine=None, M=0, H=5000), ARG, 'affine is NULL')
    _refused(_call(M=0, H=5000, L=9, lines=P), ARG, 'every size')
    _refused(_call(H=5000, L=9, lines=None), ARG, 'without the lines array')
    _refused(_call(H=5000, lut_f32=None, out_u8=P), ARG, 'out_f32 without lut_f32')
    _refused(_call(H=5000, out_u8=P, affine=P + 2), ARG, '4-byte aligned')
    _refused(_call(H=5000, out_u8=P), ARG, 'its own input')
    _refused(_call(H=5000, L=9, lines=P), UNSUPPORTED, 'each at most')


def test_op_refuses_what_needs_no_device_first_and_cpu_tensors_last():
    from seg2eye_amd import _lib
    A = _ops()
    img, lab = (torch.from_numpy(a) for a in R.planes((2, 5, 7), 1))
    p = A.identity_params(2)
    with pytest.raises(_lib.Seg2EyeHipError, match='GPU only'):
        A.augment_pairs(img, lab, p)
    with pytest.raises(_lib.Seg2EyeHipError, match='GPU only'):
        A.augment_pairs(None, lab, p)
    with pytest.raises(_lib.Seg2EyeHipError, match='GPU only'):
        A.augment_pairs(img, None, A.AugmentRule(**STRONG).draw(np.random.RandomState(0), 2, 5, 7), want_u8=True)
    for bad in (lambda: A.augment_pairs(None, None, p), lambda: A.augment_pairs(img.float(), lab, p), lambda: A.augment_pairs(img[0], lab[0], p),
                lambda: A.augment_pairs(img, lab[:, :4], p), lambda: A.augment_pairs(img, None, p, want_f32=False),
                lambda: A.augment_pairs(img, lab, A.identity_params(3)), lambda: A.augment_pairs(img, lab, p._replace(affine=p.affine.astype(np.int64))),
                lambda: A.augment_pairs(img, lab, p._replace(lut_f32=None)), lambda: A.augment_pairs(img, lab, p._replace(lut_u8=None), want_u8=True),
                lambda: A.augment_pairs(img, lab, p._replace(lines=np.zeros((2, 9, 6), np.int32))),
                lambda: A.augment_pairs(img, lab, p._replace(lines=np.zeros((2, 6), np.int32))),
                lambda: A.augment_pairs(torch.zeros(1, 4097, 2, dtype=torch.uint8), None, A.identity_params(1))):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------ the command line
TRAIN_ARGVS = [[], ['--name', 'x', '--checkpoints_dir', '/tmp/c', '--nsf', '16', '--seg_hw', '64,40', '--label_nc', '3', '--compute_dtype', 'fp32', '--batchSize', '5'],
               ['--niter', '3', '--lr', '0.01', '--class_weights', '1,2,3,4', '--seed', '9', '--no_flip', '--print_freq', '7'],
               ['--lambda_ce', '0.5', '--lambda_dice', '1', '--lambda_surface', '0.25', '--edge_alpha', '2', '--edge_radius', '3']]


@pytest.mark.parametrize('extra', TRAIN_ARGVS, ids=['defaults', 'common', 'train', 'losses'])
def test_train_parses_every_segment_train_argv_to_the_same_values(extra):
    from seg2eye_amd import seg_augment, segment
    argv = ['train', '--dataroot', 'all.h5'] + extra
    theirs = vars(segment.parser().parse_args(argv))
    ours = vars(seg_augment.parser().parse_args(argv))
    assert {k: v for k, v in ours.items() if not k.startswith('aug_')} == theirs
    assert sorted(k for k in ours if k.startswith('aug_')) == sorted(seg_augment.AUG_KEYS) and len(seg_augment.AUG_KEYS) == 8
    rule = seg_augment.rule_of(ours)
    assert rule.is_identity() and repr(rule) == repr(_ops().AugmentRule()) and not any(k.startswith('aug_') for k in ours)
    ours.pop('command'), ours.pop('dataroot')
    segment.seg_options(**ours)                                 # what is left is what seg_options takes


def test_every_flag_of_segment_train_is_a_flag_of_ours_and_the_aug_flags_reach_the_rule():
    from seg2eye_amd import seg_augment, segment

    def flags(ap, command):
        sub = [a for a in ap._actions if isinstance(getattr(a, 'choices', None), dict)][0].choices[command]
        return {s: (a.default, a.type, a.help) for a in sub._actions for s in a.option_strings}
    theirs, ours = flags(segment.parser(), 'train'), flags(seg_augment.parser(), 'train')
    assert {k: v for k, v in ours.items() if not k.startswith('--aug_')} == theirs
    a = vars(seg_augment.parser().parse_args(['train', '--dataroot', 'd', '--aug_prob', '0.5', '--aug_rotate', '10', '--aug_scale', '1.1', '--aug_translate', '0.05',
                                             '--aug_gamma', '1.5', '--aug_contrast', '0.2', '--aug_brightness', '0.1', '--aug_lines', '3']))
    r = seg_augment.rule_of(a)
    assert (r.prob, r.rotate, r.scale, r.translate, r.gamma, r.contrast, r.brightness, r.lines) == (0.5, 10.0, 1.1, 0.05, 1.5, 0.2, 0.1, 3)
    s = vars(seg_augment.parser().parse_args(['show', '--dataroot', 'd', '--out', 'o']))
    assert (s['n'], s['seed'], s['seg_hw'], s['label_nc'], s['dataset_key'], s['out']) == (8, 0, (320, 200), 4, 'train', 'o') and seg_augment.rule_of(s).is_identity()
    with pytest.raises(ValueError, match='--aug_lines'):
        seg_augment.rule_of(vars(seg_augment.parser().parse_args(['show', '--dataroot', 'd', '--out', 'o', '--aug_lines', '9'])))
    for bad in (['train'], ['show', '--dataroot', 'd'], ['eval', '--dataroot', 'd'], []):
        with pytest.raises(SystemExit):
            seg_augment.parser().parse_args(bad)


def test_segment_options_and_parser_have_no_new_key():
    from seg2eye_amd import segment
    assert not any('aug' in k for k in segment.DEFAULTS) and 'aug' not in segment.parser().format_help()
    with pytest.raises(TypeError):
        segment.seg_options(aug_rotate=1.0)


def test_label_grey_is_the_visualisers_scaling():
    from seg2eye_amd import seg_augment
    lab = np.array([[0, 1, 2, 3, 4, 255]], dtype=np.uint8)
    assert seg_augment.label_grey(lab, 4).tolist() == [[0, 85, 170, 255, 255, 255]] == R.label_grey(lab, 4).tolist()
    v = torch.tensor([0.0, 1.0, 2.0, 3.0], dtype=torch.float64) / 3 * 2 - 1                  # postprocessor's normalize, tester's bytes
    assert torch.clamp(torch.trunc((v + 1) * 128), 0, 255).tolist() == [0, 85, 170, 255]
