"""Eye geometry without a GPU: the restatement (tests/_eye_geometry_ref.py) against a literal per-pixel loop and Python
integers; the fit on lattice points that lie exactly on a curve, under translation and transposition, and every cause of valid = 0; the
occluded-pupil fact and the repaint facts, which the restatement must meet before any GPU run; `EyeShape` and the three commands with
the restatement in the ops' place; the parser; the ops' ValueErrors; every refused call of the C ABI with its code and message."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _eye_geometry_ref as R
import _mask_clean_ref as MR
import _segment_ref as SR

P = 4096                                                      # a dummy non-null pointer: must never reach a kernel
BIG = 1 << 40                                                 # a workspace size that is never short
ARG, UNSUPPORTED = -1, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('s2e_rim_moments_workspace_bytes', 's2e_rim_moments', 's2e_ellipse_paint')
SMALL = [(1, 1, 1), (1, 1, 9), (1, 9, 1), (2, 5, 7), (1, 12, 11)]
CURVE_SETS = [(4, None), (4, (((1, 2, 3), (0,)),)), (4, (((0,), (1,)), ((1,), (0,)), ((3,), (0, 1, 2)), ((2, 3), (1,)))), (2, None), (16, (((2,), (15, 3)),))]
CIRCLE = [(x, y) for x in range(-25, 26) for y in range(-25, 26) if x * x + y * y == 625]
OFFSETS = [(0, 0), (25, 25), (500, 300), (37, 911), (998, 30)]


def _eg():
    from seg2eye_amd import eye_geometry as EG
    return EG


# ------------------------------------------------------------------------------------------------ the restatement alone
@pytest.mark.parametrize('shape', SMALL, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('kind', MR.PATTERNS)
def test_restated_rim_is_a_per_pixel_loops(kind, shape):
    lab = MR.pattern(kind, shape)
    for ncls, curves in CURVE_SETS:
        for curve in (curves or R.default_curves(ncls)):
            for n in range(shape[0]):
                assert np.array_equal(R.rim_mask(lab[n], curve, ncls), R.rim_mask_loop(lab[n], curve, ncls)), (ncls, curve, n)


@pytest.mark.parametrize('kind', ['iid4', 'rings', 'checkerboard', 'iid_ignore', 'eyes_specks', 'all255', 'constant'])
def test_restated_moments_are_python_integers(kind):
    lab = MR.pattern(kind, (2, 23, 31))
    for ncls, curves in CURVE_SETS:
        got = R.rim_moments(lab, ncls, curves)
        for n in range(2):
            for k, curve in enumerate(curves or R.default_curves(ncls)):
                ys, xs = np.nonzero(R.rim_mask_loop(lab[n], curve, ncls))
                assert got[n, k].tolist() == R.moments_of_points(xs, ys), (ncls, k)
    assert (R.rim_moments(MR.pattern('constant', (2, 23, 31))) == 0).all() and (R.rim_moments(MR.pattern('all255', (1, 5, 7))) == 0).all()


def test_largest_sums_stay_below_the_headers_bound():
    """A 1024 x 1024 two-class checkerboard: every pixel of the class is a rim pixel; the sums, in Python integers, are below 2^60."""
    xs, ys = np.meshgrid(np.arange(1024), np.arange(1024))
    sel = ((xs + ys) & 1) == 1
    u, v = np.where(sel, xs - 512, 0).astype(np.int64), np.where(sel, ys - 512, 0).astype(np.int64)
    total = lambda i, j: sum(int(t) for t in (np.where(sel, u ** i * v ** j, 0)).sum(axis=1))     # a row's sum is below 2^50; rows added in Python
    assert max(abs(total(i, j)) for i, j in R.IJ) < 2 ** 60 and total(4, 0) > 2 ** 52


# ------------------------------------------------------------------------------------------------ the fit
def _fit_points(xs, ys, **kw):
    return _eg().ellipse_from_moments(np.array(R.moments_of_points(xs, ys), dtype=np.int64), **kw)


@pytest.mark.parametrize('off', OFFSETS, ids=lambda o: '%d_%d' % o)
def test_fit_of_lattice_points_on_a_curve_is_exact_under_translation(off):
    """The 20 integer points of x^2 + y^2 = 25^2, and the same with x doubled: the centre is the offset and the axes 25 / 25 and
    50 / 25 to 1e-9 -- |u| <= 50, fourth powers below 2^23, for which fp64 leaves ten digits."""
    assert len(CIRCLE) == 20
    xs, ys = np.array(CIRCLE).T
    f = _fit_points(xs + off[0], ys + off[1])
    assert f.valid == 1 and f.cause == 0 and tuple(f.origin) == off
    assert np.abs(f.centre - off).max() < 1e-9 and np.abs(f.axes - 25).max() < 1e-9
    assert abs(f.conic[0] + f.conic[2] - 1) < 1e-12 and f.conic[5] < 0
    g = _fit_points(2 * xs + off[0], ys + off[1])
    assert g.valid == 1 and np.abs(g.centre - off).max() < 1e-9 and np.abs(g.axes - (50, 25)).max() < 1e-9 and abs(g.theta) < 1e-9
    h = _fit_points(xs + off[0], 2 * ys + off[1])
    assert h.valid == 1 and np.abs(h.axes - (50, 25)).max() < 1e-9 and abs(h.theta - np.pi / 2) < 1e-9
    p = R.fit_points(2 * xs + off[0], ys + off[1])
    assert np.abs(np.array(p) - (off[0], off[1], 50, 25, 0)).max() < 1e-8


def test_fit_is_the_independent_one_and_is_invariant_under_transposition():
    EG = _eg()
    masks, _, _, _ = R.occluded(6)
    fit = EG.ellipse_from_moments(R.rim_moments(masks), 12, 1280.0)
    swapped = EG.ellipse_from_moments(R.rim_moments(np.ascontiguousarray(masks.transpose(0, 2, 1))), 12, 1280.0)
    assert fit.valid.all() and swapped.valid.all()
    assert np.array_equal(fit.origin, swapped.origin[..., ::-1])
    assert np.abs(fit.centre - swapped.centre[..., ::-1]).max() < 1e-8 and np.abs(fit.axes - swapped.axes).max() < 1e-8
    assert ((fit.theta > -np.pi / 2) & (fit.theta <= np.pi / 2)).all() and (fit.axes[..., 0] >= fit.axes[..., 1]).all()
    long = fit.axes[..., 0] / fit.axes[..., 1] > 1.05
    assert long.any()
    # mirrored in the diagonal: theta' = pi / 2 - theta up to a half turn
    assert np.abs(np.sin(2 * swapped.theta) - np.sin(2 * fit.theta))[long].max() < 1e-6
    assert np.abs(np.cos(2 * swapped.theta) + np.cos(2 * fit.theta))[long].max() < 1e-6
    for n in range(len(masks)):
        for k, curve in enumerate(R.default_curves(4)):
            ys, xs = np.nonzero(R.rim_mask(masks[n], curve, 4))
            want = np.array(R.fit_points(xs, ys))
            got = np.array([*fit.centre[n, k], *fit.axes[n, k], fit.theta[n, k]])
            assert np.abs(got[:4] - want[:4]).max() < 1e-6, (n, k)
            assert not long[n, k] or abs(np.sin(got[4] - want[4])) < 1e-6


def test_every_cause_of_an_invalid_fit():
    EG = _eg()
    xs, ys = np.array(CIRCLE).T
    cases = {
        EG.FEW_POINTS: _fit_points(xs[:11] + 40, ys[:11] + 40),
        EG.SINGULAR_S3: _fit_points(np.arange(30), 2 * np.arange(30) + 1),                       # on a line
        EG.NO_ELLIPSE: _fit_points(np.arange(-30, 31, 2) + 30, np.arange(-30, 31, 2) ** 2 // 4),  # on a parabola
        EG.TOO_LARGE: _fit_points(xs + 40, ys + 40, max_axis=24.0),
    }
    assert _fit_points(xs[:12] + 40, ys[:12] + 40).cause != EG.FEW_POINTS and _fit_points(xs + 40, ys + 40, min_points=21).cause == EG.FEW_POINTS
    assert _fit_points(xs + 40, ys + 40, max_axis=25.1).valid == 1
    row = np.array(R.moments_of_points(xs + 40, ys + 40), dtype=np.float64)
    row[17] = np.inf
    cases[EG.NOT_FINITE] = EG.ellipse_from_moments(row)
    empty = EG.ellipse_from_moments(np.zeros((2, 3, 18), dtype=np.int64))
    assert not empty.valid.any() and (empty.cause == EG.FEW_POINTS).all() and empty.conic.shape == (2, 3, 6) and np.isnan(empty.conic).all()
    for cause, f in cases.items():
        assert f.valid == 0 and f.cause == cause, (cause, f)
        assert np.isnan(f.conic).all() and np.isnan(f.centre).all() and np.isnan(f.axes).all() and np.isnan(f.theta)
    # one bad row among good ones leaves the others as they are
    rows = np.array([R.moments_of_points(xs + 40, ys + 40), [0] * 18, R.moments_of_points(2 * xs + 60, ys + 40)], dtype=np.int64)
    f = EG.ellipse_from_moments(rows)
    assert f.valid.tolist() == [1, 0, 1] and np.abs(f.axes[2] - (50, 25)).max() < 1e-9 and np.abs(f.centre[0] - 40).max() < 1e-9
    assert EG.ellipse_table(f).shape == (3, 6) and EG.ellipse_table(f)[0, 0] == 1 and np.isnan(EG.ellipse_table(f)[1, 1:]).all()


# ------------------------------------------------------------------------------------------------ the facts
def test_rim_fit_finds_an_occluded_pupil_and_the_area_centroid_does_not():
    """200 seeded 640 x 400 masks, the upper lid across 10 ... 100 % of the pupil's upper half: the mean centre error of the rim fit is
    below 0.5 px and below a tenth of the area centroid's (measured: 0.20 px, max 1.31, against 7.59 px, max 19.98)."""
    masks, pupil, iris, cut = R.occluded(200)
    assert masks.shape == (200, 640, 400) and cut.min() < 0.15 and cut.max() > 0.95
    rim = R.rim_moments(masks)
    assert rim[:, 1, 0].min() >= 62                                                 # the smallest rim is no smaller than the issue's
    fit = _eg().ellipse_from_moments(rim, 12, 1280.0)
    assert fit.valid.all()
    err = np.sqrt(((fit.centre[:, 1] - pupil[:, :2]) ** 2).sum(axis=1))
    centroid = np.array([[np.nonzero(m == 3)[1].mean(), np.nonzero(m == 3)[0].mean()] for m in masks])
    cerr = np.sqrt(((centroid - pupil[:, :2]) ** 2).sum(axis=1))
    print('rim fit: mean %.3f max %.3f px; area centroid: mean %.3f max %.3f px' % (err.mean(), err.max(), cerr.mean(), cerr.max()))
    assert err.mean() < 0.5 and err.mean() < cerr.mean() / 10
    short = fit.axes[:, 1] - pupil[:, 2:4]                                          # the inner pixels: short by about half a pixel
    assert -1.0 < short.mean() < -0.2


def test_repaint_keeps_a_true_mask_and_mends_a_frayed_one():
    """At most 0.2 % of the pixels of a true mask change (measured: mean 0.062 %, max 0.089 %); with 35 % of the pixels within 2 of a
    class border flipped, the painted IoU of iris and pupil is above the frayed one on every mask (measured means: iris 0.925 ->
    0.953, pupil 0.897 -> 0.946)."""
    EG = _eg()
    masks = R.occluded(200)[0][:100]
    fit = EG.ellipse_from_moments(R.rim_moments(masks), 12, 1280.0)
    painted = R.paint(masks, fit.conic, fit.origin, fit.valid)
    changed = (painted != masks).reshape(len(masks), -1).mean(axis=1)
    print('changed: mean %.5f max %.5f' % (changed.mean(), changed.max()))
    assert fit.valid.all() and changed.max() <= 0.002
    # the nesting holds by construction: a pupil pixel has no sclera or skin 4-neighbour that the repaint made
    for m in painted[:10]:
        assert R.rim_mask(m, ((3,), (1,)), 4).sum() == 0
    rough = np.stack([R.frayed(m, 100 + i) for i, m in enumerate(masks)])
    assert 0.005 < (rough != masks).mean() < 0.05
    fit = EG.ellipse_from_moments(R.rim_moments(rough), 12, 1280.0)
    mended = R.paint(rough, fit.conic, fit.origin, fit.valid)
    before = np.array([[R.iou(rough[i], masks[i], c) for c in (2, 3)] for i in range(len(masks))])
    after = np.array([[R.iou(mended[i], masks[i], c) for c in (2, 3)] for i in range(len(masks))])
    print('iou iris, pupil: frayed %s painted %s' % (before.mean(axis=0), after.mean(axis=0)))
    assert fit.valid.all() and (after > before).all()


def test_paint_rule_on_hand_made_conics():
    lab = np.array([[[0, 1, 1, 1, 2, 255, 3]]], dtype=np.uint8).repeat(7, axis=1)
    circle = np.array([[[0.5, 0.0, 0.5, 0.0, 0.0, -2.0]]])                         # u^2 + v^2 <= 4 about (3, 3): zero on pixel centres
    origin = np.array([[[3, 3]]], dtype=np.int32)
    one = np.ones((1, 1), dtype=np.uint8)
    out = R.paint(lab, circle, origin, one, 4, (2,), (0,), 1)
    yy, xx = np.mgrid[0:7, 0:7]
    inside = (xx - 3) ** 2 + (yy - 3) ** 2 <= 4
    free = (lab[0] != 0) & (lab[0] != 255)
    assert np.array_equal(out[0], np.where(free, np.where(inside, 2, 1), lab[0])) and out[0, 3, 5] == 255 and out[0, 3, 1] == 2 and out[0, 1, 3] == 2
    assert np.array_equal(R.paint(lab, circle, origin, 0 * one, 4, (2,), (0,), 1), lab)            # an invalid curve: unchanged
    assert (R.paint(lab, circle * np.nan, origin, one, 4, (2,), (0,), 1)[0][free] == 1).all()      # a NaN compares false: the base
    assert (R.paint(lab, circle, origin, one, 4, (2,), (), 3)[0][lab[0] != 255] != 0).all()        # keep empty: the skin is painted too


# ------------------------------------------------------------------------------------------------ the stage
@pytest.fixture
def on_host(monkeypatch):
    from seg2eye_amd import stage
    R.install(monkeypatch)
    monkeypatch.setattr(stage, 'to_device', lambda device, *arrays: [None if a is None else torch.from_numpy(np.ascontiguousarray(a)) for a in arrays])


def test_eye_shape_fits_and_regularises(on_host):
    EG = _eg()
    truth = R.occluded(3, 160, 100)[0]
    y, x = next((y, x) for y in range(2, 150) for x in range(2, 90) if (truth[0, y - 2:y + 4, x - 2:x + 4] == 2).all())
    masks = np.array(truth)
    masks[0, y:y + 2, x:x + 2] = 3                                                  # a speck of pupil in the iris: a false rim
    dirty = torch.from_numpy(masks)
    plain, cleaned = EG.EyeShape(4), EG.EyeShape(4, clean=EG.MaskRule(4))
    f0, f1 = plain.fit(dirty), cleaned.fit(dirty)
    assert isinstance(f0, EG.EllipseFit) and f0.conic.shape == (3, 2, 6) and f1.valid.all()
    truth = MR.clean_batch(masks)[0]                                                # (the speck goes; so does the smaller piece of a split sclera)
    assert (truth != masks)[0, y:y + 2, x:x + 2].all() and truth[0, y, x] == 2
    want = EG.ellipse_from_moments(R.rim_moments(truth), 12, 320.0)
    orig = plain.fit(torch.from_numpy(np.array(R.occluded(3, 160, 100)[0])))
    assert not np.array_equal(f0.conic[0, 1], orig.conic[0, 1]) and np.array_equal(f0.conic[1:], orig.conic[1:]) and np.array_equal(f0.conic[0, 0], orig.conic[0, 0])
    for a, b in zip(f1, want):
        assert np.array_equal(a, b, equal_nan=True)
    out, fit = cleaned.regularise(dirty, return_fit=True)
    assert out.dtype == torch.uint8 and np.array_equal(out.numpy(), R.paint(truth, want.conic, want.origin, want.valid))
    assert np.array_equal(cleaned.regularise(dirty).numpy(), out.numpy())
    few = EG.EyeShape(4, min_points=10 ** 6)
    assert not few.fit(dirty).valid.any() and np.array_equal(few.regularise(dirty).numpy(), masks)
    custom = EG.EyeShape(4, curves=(((3,), (2,)),), paint=(1,), keep=(0, 2), base=1)
    got = custom.regularise(torch.from_numpy(truth)).numpy()
    assert ((got == truth) | (truth == 3) | (truth == 1)).all() and (got[truth == 2] == 2).all() and (got != truth).any()
    assert 'min_points=12' in repr(plain) and 'MaskRule' in repr(cleaned)


def _tree():
    store, truth = SR.learnable_store(64, 40)
    return store, truth


def test_fit_and_apply_commands_keep_the_layout(on_host, tmp_path, capsys):
    EG = _eg()
    from seg2eye_amd.openeds_store import merge_splits, open_tree
    from seg2eye_amd.prepare_openeds import save_store
    _, truth = _tree()
    truth['train']['U101']['note'] = np.arange(3)
    paths = [save_store({split: truth[split]}, str(tmp_path / ('masks_%s.h5' % split))) for split in ('train', 'validation')]
    EG.main(['fit', '--seg_file', ','.join(paths), '--out', str(tmp_path / 'geometry.h5'), '--batchSize', '3', '--no_clean'])
    lines = capsys.readouterr().out.splitlines()
    assert lines[0].startswith('train: 24 masks, curve 0 fit rate ') and ', curve 1 fit rate ' in lines[0] and 'mean axes' in lines[0]
    assert lines[1].startswith('validation: 16 masks') and lines[2].startswith('ellipses of 2 split(s) written to ')
    written = lines[2].split('written to ')[1]
    got = merge_splits(written, open_tree)
    shape = EG.EyeShape(4)
    for split in truth:
        for user in truth[split]:
            assert sorted(got[split][user].keys()) == ['labels_pred_gen_ellipses', 'labels_pred_seq_ellipses']
            for name in ('labels_pred_gen', 'labels_pred_seq'):
                want = EG.ellipse_table(shape.fit(torch.from_numpy(truth[split][user][name])))
                table = np.asarray(got[split][user][name + '_ellipses'])
                assert table.dtype == np.float64 and table.shape == (4, 2, 6) and np.array_equal(table, want, equal_nan=True)
    EG.main(['apply', '--seg_file', ','.join(paths), '--out', str(tmp_path / 'ellipse.h5'), '--batchSize', '5'])
    lines = capsys.readouterr().out.splitlines()
    assert re.match(r'train: 3 persons, 24 masks, \d+\.\d{4}% of the pixels changed, \d+\.\d{4}% of the masks unchanged for want of a valid fit$', lines[0])
    assert lines[1].startswith('validation: 2 persons, 16 masks') and lines[2].startswith('regularised masks of 2 split(s) written to ')
    got = merge_splits(lines[2].split('written to ')[1], open_tree)
    shape = EG.EyeShape(4, clean=EG.MaskRule(4))
    assert np.array_equal(np.asarray(got['train']['U101']['note']), np.arange(3))
    for split in truth:
        for user in truth[split]:
            for name in ('labels_pred_gen', 'labels_pred_seq'):
                want = shape.regularise(torch.from_numpy(truth[split][user][name])).numpy()
                a = np.asarray(got[split][user][name])
                assert a.dtype == np.uint8 and np.array_equal(a, want), (split, user, name)


class _OneHotNet:
    def __init__(self, masks):
        self.masks, self.at = masks, 0

    def __call__(self, x):
        m = torch.from_numpy(self.masks[self.at:self.at + x.shape[0]].astype(np.int64))
        self.at += x.shape[0]
        return (m[..., None] == torch.arange(4)).float().contiguous()


def test_eval_scores_raw_cleaned_and_regularised_masks(on_host, monkeypatch):
    EG = _eg()
    from seg2eye_amd import segment
    from seg2eye_amd.ops import segment as S

    def confusion(pred, truth, ncls, out=None):
        p, t = pred.numpy().astype(np.int64).ravel(), truth.numpy().astype(np.int64).ravel()
        ok = (p < ncls) & (t < ncls)
        out += torch.from_numpy(np.bincount(t[ok] * ncls + p[ok], minlength=ncls * ncls).reshape(ncls, ncls))
        return out
    monkeypatch.setattr(S, 'seg_argmax_u8', lambda logits, Ho=None, Wo=None, ncls=None: logits.argmax(dim=-1).to(torch.uint8))
    monkeypatch.setattr(S, 'seg_confusion', confusion)
    monkeypatch.setattr(segment, '_frames_to_input', lambda frames, hw, flip, device: torch.zeros(len(frames), 1, 8, 8))
    store, _ = _tree()
    opt = segment.seg_options(seg_hw=(64, 40), compute_dtype='fp32', batchSize=5)
    truth = np.concatenate([store['validation'][u]['labels_ss'] for u in store['validation']])
    got = EG.evaluate(_OneHotNet(truth), store, 'validation', opt, EG.EyeShape(4, clean=EG.MaskRule(4)), device='cpu', verbose=False)
    keys = {'miou/validation', 'acc/validation'} | {'iou/validation/%d' % c for c in range(4)}
    want = keys | {k.replace('/', '_clean/', 1) for k in keys} | {k.replace('/', '_ellipse/', 1) for k in keys}
    assert set(got) == want | {'centre_px/validation/0', 'centre_px/validation/1', 'fit_rate/validation/0', 'fit_rate/validation/1'}
    assert got['miou/validation'] == 1.0 == got['miou_clean/validation'] and got['centre_px/validation/0'] == 0.0 == got['centre_px/validation/1']
    assert got['fit_rate/validation/1'] > 0 and 0.8 < got['miou_ellipse/validation'] <= 1.0
    with pytest.raises(ValueError, match='no labelled frames'):
        EG.evaluate(None, {'validation': {}}, 'validation', opt, EG.EyeShape(4), device='cpu')


def test_parser_defaults():
    EG = _eg()
    a = vars(EG.parser().parse_args(['fit', '--seg_file', 'a.h5,b.h5', '--out', 'g.h5']))
    assert (a['command'], a['seg_file'], a['out'], a['no_clean'], a['min_points'], a['label_nc'], a['batchSize']) == ('fit', 'a.h5,b.h5', 'g.h5', False, 12, 4, 64)
    shape = EG.shape_of(a)
    assert (shape.ncls, shape.curves, shape.paint, shape.keep, shape.base, shape.min_points) == (4, None, None, (0,), 1, 12)
    assert isinstance(shape.clean, EG.MaskRule) and shape.clean.ncls == 4
    b = vars(EG.parser().parse_args(['apply', '--seg_file', 'a.h5', '--out', 'c.h5', '--no_clean', '--min_points', '30', '--batchSize', '8']))
    assert (b['command'], b['batchSize'], b['min_points']) == ('apply', 8, 30) and EG.shape_of(b).clean is None and EG.shape_of(b).min_points == 30
    e = vars(EG.parser().parse_args(['eval', '--dataroot', 'all.h5', '--name', 'seg']))
    assert (e['command'], e['dataroot'], e['name'], e['dataset_key'], e['which_epoch'], e['label_nc'], e['batchSize']) == ('eval', 'all.h5', 'seg', 'validation', 'latest', 4, 16)
    assert e['seg_hw'] == (320, 200) and e['nsf'] == 32 and e['compute_dtype'] == 'bf16' and e['checkpoints_dir'] == './checkpoints'
    from seg2eye_amd import mask_clean as MC
    theirs = vars(MC.parser().parse_args(['eval', '--dataroot', 'all.h5', '--name', 'seg']))
    assert set(theirs) - {'conn', 'modes'} <= set(e)                                 # the flags of `mask_clean eval`
    for bad in (['fit', '--out', 'g.h5'], ['apply', '--seg_file', 'a'], ['eval', '--name', 'seg'], ['fit', '--seg_file', 'a', '--out', 'c', '--min_points', 'x'], []):
        with pytest.raises(SystemExit):
            EG.parser().parse_args(bad)


def test_segment_and_refine_command_lines_have_not_moved():
    from seg2eye_amd import refine, segment
    for mod in (segment, refine):
        text = mod.parser().format_help()
        assert 'ellipse' not in text and 'geometry' not in text


# ------------------------------------------------------------------------------------------------ the ops' checks
def test_default_curves():
    from seg2eye_amd.ops import geometry as G
    assert G.default_curves(4) == (((2, 3), (1,)), ((3,), (2,))) == R.default_curves(4) == G.default_curves(16)
    assert G.default_curves(2) == (((1,), (0,)),) == R.default_curves(2) and G.default_curves(3) == (((2,), (1,)),)
    for bad in (0, 1, 17):
        with pytest.raises(ValueError):
            G.default_curves(bad)


def test_op_checks_come_before_the_device():
    from seg2eye_amd import _lib
    from seg2eye_amd.ops import geometry as G
    lab = torch.zeros(2, 5, 7, dtype=torch.uint8)
    conic, origin, valid = torch.zeros(2, 2, 6, dtype=torch.float64), torch.zeros(2, 2, 2, dtype=torch.int32), torch.ones(2, 2, dtype=torch.uint8)
    for bad, kw in ((lab.int(), {}), (lab[0], {}), (torch.zeros(2, 0, 7, dtype=torch.uint8), {}), (torch.zeros(1, 1025, 2, dtype=torch.uint8), {}),
                    (lab, dict(ncls=0)), (lab, dict(ncls=17))):
        with pytest.raises(ValueError):
            G.rim_moments(bad, **kw)
        with pytest.raises(ValueError):
            G.ellipse_paint(bad, conic, origin, valid, **kw)
    for curves in ((), (((3,), (2,)),) * 5, (((3,),),), (((3,), ()),), (((), (2,)),), (((3, 2), (2,)),), (((4,), (2,)),), (((3,), (-1,)),), (((3,), (1.5,)),),
                   (((3,), ('2',)),), ((3, (2,)),)):
        with pytest.raises(ValueError, match='curves'):
            G.rim_moments(lab, 4, curves)
    with pytest.raises(ValueError):
        G.rim_moments(lab, 1)                                                       # one class: no default curve
    for kw in (dict(conic=conic.float()), dict(conic=conic[:1]), dict(conic=conic[..., :5]), dict(conic=torch.zeros(2, 5, 6, dtype=torch.float64)),
               dict(origin=origin.long()), dict(origin=origin[:, :1]), dict(valid=valid.bool()), dict(valid=valid[:, :1]),
               dict(paint=(2,)), dict(paint=(2, 4)), dict(paint=(2, 1.5)), dict(base=4), dict(base=-1), dict(keep=(4,)), dict(keep=3)):
        args = dict(conic=conic, origin=origin, valid=valid)
        args.update(kw)
        with pytest.raises(ValueError):
            G.ellipse_paint(lab, args.pop('conic'), args.pop('origin'), args.pop('valid'), **args)
    with pytest.raises(_lib.Seg2EyeHipError, match='GPU only'):
        G.rim_moments(lab)
    with pytest.raises(_lib.Seg2EyeHipError, match='GPU only'):
        G.rim_moments(lab, 4, (((1, 2, 3), (0,)),))
    with pytest.raises(_lib.Seg2EyeHipError, match='GPU only'):
        G.ellipse_paint(lab, conic, origin, valid, keep=(), paint=(3, 2))


# ------------------------------------------------------------------------------------------------ declared, exported, bound, built
def test_new_symbols_are_declared_exported_and_bound():
    from seg2eye_amd import _lib, build
    header = open(os.path.join(ROOT, 'include', 'seg2eye_hip.h')).read()
    for name in NEW:
        assert re.search(r'\b%s\(' % name, header), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name), name
    assert 'eye_geometry.hip' in build.SOURCES and os.path.exists(os.path.join(build.CSRC, 'eye_geometry.hip'))
    source = open(os.path.join(build.CSRC, 'eye_geometry.hip')).read()
    assert '#pragma clang fp contract(off)' in source and '2^60' in header and 'HOST' in header.split('eye geometry')[1].split('residual refiner')[0]
    from seg2eye_amd import ops
    assert ops.rim_moments is ops.geometry.rim_moments and ops.ellipse_paint is ops.geometry.ellipse_paint


# ------------------------------------------------------------------------------------------------ refused calls
IN = (ctypes.c_uint16 * 4)(0b1100, 0b1000, 0b0001, 0b0010)
OUT = (ctypes.c_uint16 * 4)(0b0010, 0b0100, 0b0010, 0b0001)
PAINT = (ctypes.c_uint8 * 4)(2, 3, 1, 0)


def _sets(*values):
    a = (ctypes.c_uint16 * 4)(*values)
    return a, ctypes.addressof(a)


def _rim(labels=P, N=2, H=8, W=8, ncls=4, K=2, ins=ctypes.addressof(IN), outs=ctypes.addressof(OUT), rim=P, ws=P, wsb=BIG):
    return (labels, N, H, W, ncls, K, ins, outs, rim, ws, wsb, None)


def _paint(labels=P, N=2, H=8, W=8, ncls=4, K=2, conic=P, origin=P, valid=P, paint=ctypes.addressof(PAINT), keep=1, base=1, out=P):
    return (labels, N, H, W, ncls, K, conic, origin, valid, paint, keep, base, out, None)


def _refused(fn, args, code, text):
    from seg2eye_amd import _lib
    L = _lib.lib()
    assert getattr(L, fn)(*args) == code, (fn, args)
    msg = L.s2e_last_error().decode()
    assert msg.startswith(fn + ': ') and text in msg, msg


def test_refused_calls_of_rim_moments():
    from seg2eye_amd import _lib
    L = _lib.lib()
    fn = 's2e_rim_moments'
    for kw in (dict(labels=None), dict(ins=None), dict(outs=None), dict(rim=None), dict(ws=None)):
        _refused(fn, _rim(**kw), ARG, 'bad argument')
    need = L.s2e_rim_moments_workspace_bytes(2, 8, 8, 2)
    assert need > 0 and need % 256 == 0
    _refused(fn, _rim(wsb=need - 1), ARG, 'workspace of %d bytes, needs %d' % (need - 1, need))
    _refused(fn, _rim(ws=P + 4), ARG, '8-byte aligned')
    _refused(fn, _rim(rim=P + 4), ARG, '8-byte aligned')
    for kw in (dict(N=0), dict(H=0), dict(W=-1)):
        _refused(fn, _rim(wsb=0, **kw), ARG, 'every size must be at least 1')         # (a refused shape needs 0 bytes)
    for K in (0, 5):
        _refused(fn, _rim(K=K, wsb=0), UNSUPPORTED, 'K=%d (1 to 4 curves)' % K)
    for ncls in (0, 17):
        _refused(fn, _rim(ncls=ncls), UNSUPPORTED, 'ncls=%d (1 to 16 classes)' % ncls)
    keep = []
    for ins, outs, text in (((0b1100, 0), (0b0010, 0b0100), 'curve 1: in=0x0 out=0x4 (an empty class set)'),
                            ((0b1100, 0b1000), (0, 0b0100), 'curve 0: in=0xc out=0x0 (an empty class set)'),
                            ((0b1100, 0b1100), (0b0010, 0b0100), 'curve 1: in=0xc out=0x4 (the sets overlap)'),
                            ((0b11100, 0b1000), (0b0010, 0b0100), 'curve 0: in=0x1c out=0x2 (a class at or above ncls=4)'),
                            ((0b1100, 0b1000), (0b0010, 0x8004), 'curve 1: in=0x8 out=0x8004 (a class at or above ncls=4)')):
        a, b = _sets(*ins), _sets(*outs)
        keep += [a, b]
        _refused(fn, _rim(ins=a[1], outs=b[1]), ARG, text)
    _refused(fn, _rim(H=1025, wsb=0), UNSUPPORTED, 'H=1025 W=8 (each at most 1024)')
    _refused(fn, _rim(N=65536, H=1, W=1, wsb=0), UNSUPPORTED, 'beyond the launch limits')
    _refused(fn, _rim(N=2048, H=1024, W=1024, wsb=0), UNSUPPORTED, 'beyond the launch limits')
    # the order: null pointers, the workspace, the sizes, K, ncls, the curves, the sides, the batch
    bad = _sets(0, 0)
    _refused(fn, _rim(rim=None, wsb=0), ARG, 'bad argument')
    _refused(fn, _rim(wsb=0, K=2, ncls=99), ARG, 'workspace of 0 bytes')
    _refused(fn, _rim(N=0, K=9, wsb=0), ARG, 'every size')
    _refused(fn, _rim(K=9, ncls=99, wsb=0), UNSUPPORTED, 'K=9')
    _refused(fn, _rim(ncls=99, ins=bad[1]), UNSUPPORTED, 'ncls=99')
    _refused(fn, _rim(ins=bad[1], W=4096, wsb=0), ARG, 'an empty class set')
    _refused(fn, _rim(N=65536, W=4096, wsb=0), UNSUPPORTED, 'each at most')
    # a set behind K is not read
    assert L.s2e_rim_moments(*_rim(ins=_sets(0b1100, 0)[1], K=1, W=4096, wsb=0)) == UNSUPPORTED and b'each at most' in L.s2e_last_error()


def test_refused_calls_of_ellipse_paint():
    from seg2eye_amd import _lib
    L = _lib.lib()
    fn = 's2e_ellipse_paint'
    for kw in (dict(labels=None), dict(conic=None), dict(origin=None), dict(valid=None), dict(paint=None), dict(out=None)):
        _refused(fn, _paint(**kw), ARG, 'bad argument')
    _refused(fn, _paint(conic=P + 4), ARG, '8-byte')
    _refused(fn, _paint(origin=P + 2), ARG, '4-byte aligned')
    for kw in (dict(N=0), dict(H=0), dict(W=-1)):
        _refused(fn, _paint(**kw), ARG, 'every size must be at least 1')
    for K in (0, 5):
        _refused(fn, _paint(K=K), UNSUPPORTED, 'K=%d (1 to 4 curves)' % K)
    for ncls in (0, 17):
        _refused(fn, _paint(ncls=ncls), UNSUPPORTED, 'ncls=%d (1 to 16 classes)' % ncls)
    _refused(fn, _paint(ncls=3), ARG, 'paint[1]=3 (a class below ncls=3)')
    _refused(fn, _paint(base=4), ARG, 'base=4 (a class below ncls=4)')
    _refused(fn, _paint(base=-1), ARG, 'base=-1')
    _refused(fn, _paint(W=1025), UNSUPPORTED, 'H=8 W=1025 (each at most 1024)')
    _refused(fn, _paint(N=65536, H=1, W=1), UNSUPPORTED, 'beyond the launch limits')
    # the order: null pointers, the sizes, K, ncls, the classes, the sides, the batch
    _refused(fn, _paint(out=None, N=0), ARG, 'bad argument')
    _refused(fn, _paint(N=0, K=9), ARG, 'every size')
    _refused(fn, _paint(K=9, ncls=99), UNSUPPORTED, 'K=9')
    _refused(fn, _paint(ncls=99, base=100), UNSUPPORTED, 'ncls=99')
    _refused(fn, _paint(base=4, W=4096), ARG, 'base=4')
    _refused(fn, _paint(N=65536, W=4096), UNSUPPORTED, 'each at most')
    # a paint byte behind K is not read as a class
    assert L.s2e_ellipse_paint(*_paint(ncls=3, K=1, W=4096)) == UNSUPPORTED and b'each at most' in L.s2e_last_error()


def test_workspace_sizes():
    from seg2eye_amd import _lib
    L = _lib.lib()
    al = lambda b: (b + 255) // 256 * 256
    for N, H, W, K in ((1, 1, 1, 1), (2, 5, 7, 2), (16, 640, 400, 2), (3, 1024, 1024, 4), (1, 64, 64, 3), (1, 64, 65, 3)):
        blocks = (H * W + 4095) // 4096
        assert L.s2e_rim_moments_workspace_bytes(N, H, W, K) == al(N * K * blocks * 3 * 8) + al(N * K * blocks * 15 * 8)
    for bad in ((0, 8, 8, 2), (1, 0, 8, 2), (1, 8, 0, 2), (1, 8, 8, 0), (1, 8, 8, 5), (1, 1025, 8, 2), (1, 8, 1025, 2), (65536, 1, 1, 2), (2048, 1024, 1024, 2)):
        assert L.s2e_rim_moments_workspace_bytes(*bad) == 0, bad
