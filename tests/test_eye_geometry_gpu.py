"""Eye geometry on the GPU: `ops.rim_moments` and `ops.ellipse_paint` against the numpy restatement
(tests/_eye_geometry_ref.py), and the stage end to end.  Every comparison is == on integers or bytes; there is no tolerance anywhere.

A workgroup of the moments kernels takes 4096 pixels (B below) and a lane four consecutive ones; rows of a width that is a multiple of
four on a 4-byte aligned plane go through the word path, everything else through the byte path.  Besides the degenerate shapes, two
shapes span more than one workgroup with ragged rows, one real 640 x 400 batch takes the word path, and a 1024 x 1024 checkerboard
gives the largest sums the int64 bound allows."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _eye_geometry_ref as R
import _mask_clean_ref as MR
import _segment_ref as SR
import _style_rank_ref as K

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 4096                                                      # EG_BLOCK_PIX of seg2eye_amd/csrc/eye_geometry.hip
SHAPES = [(1, 1, 1), (1, 1, 67), (1, 67, 1), (2, 5, 7), (1, 67, 69), (3, 66, 35), (2, 64, 68)]          # (the last: the word path, ragged)
BIG = (2, 640, 400)
PATTERNS = ('constant', 'iid4', 'rings', 'checkerboard', 'iid_ignore', 'all255', 'eyes', 'eyes_specks')
# (ncls, curves): K = 2 (the default), 1 with three `in` classes, 4, and the two ends of ncls
CURVES = [(4, None), (4, (((1, 2, 3), (0,)),)), (4, (((0,), (1,)), ((1,), (0,)), ((3,), (0, 1, 2)), ((2, 3), (1,)))), (2, None), (16, (((2,), (15, 3)), ((0, 1), (2,))))]
CASES = [(s, k) for s in SHAPES for k in PATTERNS] + [(BIG, k) for k in ('eyes', 'iid4', 'occluded')]
assert 67 * 69 > B and 3 * 66 * 35 > B and 64 * 68 > B


def _ops():
    from seg2eye_amd.ops import geometry as G
    return G


@functools.lru_cache(maxsize=None)
def _pattern(kind, shape):
    if kind == 'eyes':
        out = K.eyes(shape[0], shape[1], shape[2], 4, 23)
    elif kind == 'occluded':
        out = np.array(R.occluded(shape[0], shape[1], shape[2])[0])
    else:
        return MR.pattern(kind, shape)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _rim(kind, shape, ci):
    ncls, curves = CURVES[ci]
    out = R.rim_moments(_pattern(kind, shape), ncls, curves)
    out.setflags(write=False)
    return out


def _off_by_one(t):
    """The same planes one byte off their alignment."""
    buf = torch.empty(t.numel() + 1, dtype=torch.uint8, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 2 == 1 and view.is_contiguous()
    return view


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize('shape,kind', CASES, ids=['%s-%s' % ('x'.join(map(str, s)), k) for s, k in CASES])
def test_rim_moments_are_the_restated_ones(shape, kind):
    G = _ops()
    host = _pattern(kind, shape)
    lab = _dev(host)
    odd = _off_by_one(lab)
    for ci, (ncls, curves) in enumerate(CURVES):
        want = _rim(kind, shape, ci)
        rim = G.rim_moments(lab, ncls, curves)
        assert rim.dtype == torch.int64 and tuple(rim.shape) == want.shape
        assert np.array_equal(rim.cpu().numpy(), want), (ncls, curves)
        assert torch.equal(G.rim_moments(lab, ncls, curves), rim) and torch.equal(G.rim_moments(odd, ncls, curves), rim)
    if kind in ('constant', 'all255'):
        assert int(G.rim_moments(lab).abs().sum()) == 0                             # no rim: n = 0, origin 0
    assert torch.equal(lab.cpu(), torch.from_numpy(np.array(host)))                 # the input is read only


def test_largest_sums_of_a_checkerboard():
    G = _ops()
    yy, xx = np.mgrid[0:1024, 0:1024]
    host = ((yy + xx) & 1).astype(np.uint8)[None]
    rim = G.rim_moments(_dev(host), 2, (((1,), (0,)), ((0,), (1,)))).cpu().numpy()
    for k, c in enumerate((1, 0)):
        u, v = np.where(host[0] == c, xx - 512, 0).astype(np.int64), np.where(host[0] == c, yy - 512, 0).astype(np.int64)
        # (the rounded mean of either class is 512, 512: (2 sum x + n) // (2 n) with mean 511.5 exactly)
        want = [1 << 19, 512, 512] + [int(np.where(host[0] == c, u ** i * v ** j, 0).sum()) for i, j in R.IJ]
        assert rim[0, k].tolist() == want, k
    assert rim[0, 0, 13] > 2 ** 52


# ------------------------------------------------------------------------------------------------ the repaint
def _fitted(host, ncls=4, curves=None):
    from seg2eye_amd import eye_geometry as EG
    return EG.ellipse_from_moments(R.rim_moments(host, ncls, curves), 12, 2.0 * max(host.shape[1:]))


def _paint_both(host, fit_arrays, ncls=4, paint=None, keep=(0,), base=1):
    """ops.ellipse_paint on aligned and on shifted planes, twice -> its bytes, checked against the restatement."""
    G = _ops()
    conic, origin, valid = fit_arrays
    lab = _dev(host)
    args = (_dev(conic), _dev(origin), _dev(valid), ncls, paint, keep, base)
    out = G.ellipse_paint(lab, *args)
    assert out.dtype == torch.uint8 and out.shape == lab.shape
    assert torch.equal(G.ellipse_paint(lab, *args), out) and torch.equal(G.ellipse_paint(_off_by_one(lab), *args), out)
    assert torch.equal(lab.cpu(), torch.from_numpy(np.array(host)))
    got = out.cpu().numpy()
    assert np.array_equal(got, R.paint(host, conic, origin, valid, ncls, paint, keep, base))
    return got


@pytest.mark.parametrize('shape,kind', [((2, 5, 7), 'eyes'), ((1, 67, 69), 'eyes'), ((3, 66, 35), 'eyes_specks'), ((2, 64, 68), 'eyes'), ((1, 67, 69), 'iid_ignore'),
                                        (BIG, 'occluded'), (BIG, 'eyes')], ids=lambda v: v if isinstance(v, str) else 'x'.join(map(str, v)))
def test_paint_from_fitted_conics_is_the_restated_one(shape, kind):
    host = _pattern(kind, shape)
    fit = _fitted(host)
    got = _paint_both(host, (fit.conic, fit.origin, fit.valid))
    if kind in ('eyes', 'occluded') and shape[1] >= 64:
        assert fit.valid.all() and (got != host).any()
    # the paint order reversed (the limbus last covers the pupil), no class kept, another base
    _paint_both(host, (fit.conic[:, ::-1], fit.origin[:, ::-1], fit.valid[:, ::-1]), paint=(3, 2))
    _paint_both(host, (fit.conic, fit.origin, fit.valid), keep=(), base=0)
    _paint_both(host, (fit.conic[:, :1], fit.origin[:, :1], fit.valid[:, :1]), paint=(3,), keep=(0, 1), base=2)


def test_paint_of_hand_made_conics():
    rng = np.random.RandomState(3)
    host = rng.randint(1, 4, (3, 17, 19)).astype(np.uint8)
    host[:, 0] = 0
    host[:, :, -1] = 255
    # a circle of radius 5 about (9, 8): Q = 0 exactly on pixel centres such as (14, 8), (12, 12), (13, 11), which are inside
    circle = np.array([0.5, 0.0, 0.5, 0.0, 0.0, -12.5])
    conic = np.tile(circle, (3, 2, 1))
    conic[:, 1] = (0.5, 0.0, 0.5, 0.0, 0.0, -2.0)                                   # ... and of radius 2 inside it
    origin = np.tile(np.array([9, 8], dtype=np.int32), (3, 2, 1))
    valid = np.ones((3, 2), dtype=np.uint8)
    got = _paint_both(host, (conic, origin, valid))
    yy, xx = np.mgrid[0:17, 0:19]
    d2 = (xx - 9) ** 2 + (yy - 8) ** 2
    free = (host[0] != 0) & (host[0] != 255)
    assert np.array_equal(got[0], np.where(free, np.where(d2 <= 4, 3, np.where(d2 <= 25, 2, 1)), host[0]))
    assert got[0, 8, 14] == 2 and got[0, 12, 12] == 2 and got[0, 11, 13] == 2 and got[0, 8, 15] == 1 and got[0, 8, 11] == 3
    # one invalid curve in one image of the batch: only that image is unchanged
    valid[1, 1] = 0
    got = _paint_both(host, (conic, origin, valid))
    assert np.array_equal(got[1], host[1]) and (got[0] != host[0]).any() and (got[2] != host[2]).any()
    # NaN coefficients compare false: the curve paints nothing, the other still does
    conic[2, 0] = np.nan
    got = _paint_both(host, (conic, origin, valid))
    assert set(np.unique(got[2][(host[2] != 0) & (host[2] != 255)])) == {1, 3}
    conic[:] = np.nan
    valid[:] = 1
    got = _paint_both(host, (conic, origin, valid))
    assert (got[:, 1:, :-1] == 1).all()
    # an origin far outside the frame, infinities, 16 classes and four curves
    conic = rng.randn(3, 4, 6)
    conic[0, 0, 0] = np.inf
    conic[1, 2, 5] = -np.inf
    origin = rng.randint(-2 ** 31, 2 ** 31 - 1, (3, 4, 2)).astype(np.int32)
    origin[2] = rng.randint(0, 17, (4, 2))
    _paint_both(rng.randint(0, 16, (3, 17, 19)).astype(np.uint8), (conic, origin, np.ones((3, 4), dtype=np.uint8)), ncls=16, paint=(15, 3, 0, 9), keep=(1, 14), base=7)


# ------------------------------------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def _stores(H=64, W=40):
    return SR.learnable_store(H, W)


def _same_tree(a, b):
    assert sorted(a.keys()) == sorted(b.keys())
    for split in a.keys():
        assert sorted(a[split].keys()) == sorted(b[split].keys())
        for user in a[split].keys():
            assert sorted(a[split][user].keys()) == sorted(b[split][user].keys())
            for name in a[split][user].keys():
                x, y = np.asarray(a[split][user][name]), np.asarray(b[split][user][name])
                assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype.kind == 'f'), (split, user, name)


def _host_shape(EG, monkeypatch, **kw):
    """An EyeShape whose ops are the restatement's (CPU tensors)."""
    R.install(monkeypatch)
    return EG.EyeShape(4, **kw)


def test_fit_on_the_gpu_is_the_restatements_bit_for_bit(monkeypatch):
    from seg2eye_amd import eye_geometry as EG
    _, truth = _stores()
    small = np.concatenate([truth['train'][u]['labels_pred_gen'] for u in truth['train']])
    got = [(EG.EyeShape(4, clean=EG.MaskRule(4)).regularise(_dev(m), return_fit=True), EG.EyeShape(4).fit(_dev(m))) for m in (small, np.array(R.occluded(4)[0]))]
    R.install(monkeypatch)                                                            # from here on the ops are the restatement's
    for ((painted, fit), plain), m in zip(got, (small, np.array(R.occluded(4)[0]))):
        if m.shape[1] <= 64:                                                          # (the cleaner's restatement takes seconds per 640 x 400 mask)
            want_painted, want = EG.EyeShape(4, clean=EG.MaskRule(4)).regularise(torch.from_numpy(m), return_fit=True)
            assert np.array_equal(painted.cpu().numpy(), want_painted.numpy())
            for a, b in zip(fit, want):
                assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')
        want = EG.EyeShape(4).fit(torch.from_numpy(m))
        for a, b in zip(plain, want):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')
        assert plain.valid.any()


def test_apply_and_fit_from_the_shell(tmp_path):
    from seg2eye_amd import eye_geometry as EG, style_rank
    from seg2eye_amd.openeds_store import merge_splits, open_tree
    from seg2eye_amd.prepare_openeds import save_store
    store, truth = _stores()
    paths = [save_store({split: truth[split]}, str(tmp_path / ('masks_%s.h5' % split))) for split in ('train', 'validation')]
    for command, extra in (('apply', ['--batchSize', '5']), ('fit', ['--no_clean', '--min_points', '14'])):
        r = subprocess.run([sys.executable, '-m', 'seg2eye_amd.eye_geometry', command, '--seg_file', ','.join(paths), '--out', str(tmp_path / (command + '.h5'))] + extra,
                           capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        assert ('train: 3 persons, 24 masks' if command == 'apply' else 'train: 24 masks, curve 0 fit rate') in r.stdout and 'validation: ' in r.stdout
        written = [p for p in (str(tmp_path / (command + '.h5')), str(tmp_path / (command + '.h5.npz'))) if os.path.exists(p)]
        assert len(written) == 1 and written[0] in r.stdout
        got = merge_splits(written[0], open_tree)
        if command == 'apply':
            want = EG.regularise_store(truth, EG.EyeShape(4, clean=EG.MaskRule(4)), device=DEV, verbose=False)
            _same_tree(got, want)
            changed = sum(int((want[s][u][n] != truth[s][u][n]).sum()) for s in truth for u in truth[s] for n in truth[s][u])
            assert changed > 0
            applied = written[0]
        else:
            _same_tree(got, EG.fit_store(truth, EG.EyeShape(4, min_points=14), device=DEV, verbose=False))
    # style_rank takes the regularised masks as its --seg_file
    dataroot = save_store(store, str(tmp_path / 'store.h5'))
    style_rank.main(['--dataroot', dataroot, '--dataset_key', 'train', '--seg_file', applied, '--top', '3', '--out', str(tmp_path / 'refs.h5')])
    refs = [p for p in (str(tmp_path / 'refs.h5'), str(tmp_path / 'refs.h5.npz')) if os.path.exists(p)]
    assert len(refs) == 1
    ranked = style_rank.rank_styles(store, 'train', seg_store=merge_splits(applied, open_tree), top=3, device=DEV)
    assert sorted(ranked['train']) == sorted(store['train']) and all(len(v['index']) == 3 for u in ranked['train'].values() for v in u.values())


class _OneHotNet:
    """A stand-in network whose masks are the given ones: one-hot logits of them, batch by batch in the order of the labelled samples."""

    def __init__(self, masks):
        self.masks, self.at = masks, 0

    def __call__(self, x):
        m = torch.from_numpy(self.masks[self.at:self.at + x.shape[0]].astype(np.int64)).to(x.device)
        self.at += x.shape[0]
        return (m[..., None] == torch.arange(4, device=x.device)).float().contiguous()


def test_eval_of_the_true_masks():
    """A network that predicts the truth, at the frames' own 640 x 400: the centres coincide; the repaint changes at most 0.2 % of the
    pixels (the repaint fact), so acc_ellipse >= 0.998, and a class of pixel share s keeps an IoU of at least (s - 0.002) / (s + 0.002)
    -- at most 0.002 of the pixels leave it and at most 0.002 join it."""
    from seg2eye_amd import eye_geometry as EG, segment
    store, _ = _stores(640, 400)
    opt = segment.seg_options(seg_hw=(64, 40), compute_dtype='fp32', batchSize=4)
    truth = np.concatenate([store['validation'][u]['labels_ss'] for u in store['validation']])
    got = EG.evaluate(_OneHotNet(truth), store, 'validation', opt, EG.EyeShape(4, clean=EG.MaskRule(4)), device=DEV, verbose=False)
    keys = {'miou/validation', 'acc/validation'} | {'iou/validation/%d' % c for c in range(4)}
    assert set(got) == keys | {k.replace('/', '_clean/', 1) for k in keys} | {k.replace('/', '_ellipse/', 1) for k in keys} | {
        'centre_px/validation/0', 'centre_px/validation/1', 'fit_rate/validation/0', 'fit_rate/validation/1'}
    assert got['centre_px/validation/0'] == 0.0 == got['centre_px/validation/1'] and got['fit_rate/validation/0'] == 1.0 == got['fit_rate/validation/1']
    assert got['miou/validation'] == 1.0 == got['miou_clean/validation']
    share = np.array([(truth == c).mean() for c in range(4)])
    print({k: v for k, v in got.items() if 'ellipse' in k}, share)
    assert 1.0 > got['acc_ellipse/validation'] >= 1.0 - 0.002
    assert 1.0 > got['miou_ellipse/validation'] >= ((share - 0.002) / (share + 0.002)).mean()
    raw = segment.evaluate(_OneHotNet(truth), store, 'validation', opt, DEV, verbose=False)
    assert all(got[k] == v for k, v in raw.items())                                 # the raw scores are segment eval's
