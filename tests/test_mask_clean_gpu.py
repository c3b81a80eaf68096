"""The mask cleaner on the GPU: `ops.mask_components` and `ops.mask_clean` against the numpy restatement
(tests/_mask_clean_ref.py), and the stage end to end.  Every comparison is == on integers; there is no tolerance anywhere.

The kernels label 32 x 32 tiles (T = 32 below): besides the degenerate shapes and one real 640 x 400 batch, two shapes span three tiles
in each direction with ragged edges."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _mask_clean_ref as R
import _segment_ref as SR
import _style_rank_ref as K

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 32                                                        # MC_TILE of seg2eye_amd/csrc/mask_clean.hip
SHAPES = [(1, 1, 1), (1, 1, 67), (1, 67, 1), (2, 5, 7), (1, 2 * T + 3, 2 * T + 5), (3, 2 * T + 2, T + 3)]
BIG = (2, 640, 400)
BIG_PATTERNS = ('eyes_specks', 'spiral', 'iid4')              # the patterns whose restatement runs in a few seconds at this size
VARIANTS = ((4, None), (4, (0,) * 4), (4, (1,) * 4), (4, (2,) * 4), (1, None), (16, None))        # (ncls, modes)
CASES = [(s, k) for s in SHAPES for k in R.PATTERNS] + [(BIG, k) for k in BIG_PATTERNS]


def _ops():
    from seg2eye_amd.ops import mask_clean as M
    return M


def _off_by_one(lab):
    """The same planes one byte off their alignment."""
    buf = torch.empty(lab.numel() + 1, dtype=torch.uint8, device=lab.device)
    view = buf[1:].view(lab.shape)
    view.copy_(lab)
    assert view.data_ptr() % 2 == 1 and view.is_contiguous()
    return view


@pytest.mark.parametrize('conn', [4, 8])
@pytest.mark.parametrize('shape,kind', CASES, ids=['%s-%s' % ('x'.join(map(str, s)), k) for s, k in CASES])
def test_components_and_cleaned_masks_are_the_restated_ones(shape, kind, conn):
    M = _ops()
    host = R.pattern(kind, shape)
    lab = torch.from_numpy(np.array(host)).to(DEV)
    odd = _off_by_one(lab)
    for ncls, modes in VARIANTS:
        want_out, want_stats, want_comp = R.reference(kind, shape, ncls, conn, modes)
        comp = M.mask_components(lab, ncls, conn)
        assert comp.dtype == torch.int32 and np.array_equal(comp.cpu().numpy(), want_comp), (ncls, 'components')
        out, stats = M.mask_clean(lab, ncls, conn, modes, return_stats=True)
        assert out.dtype == torch.uint8 and stats.dtype == torch.int32 and tuple(stats.shape) == (shape[0], ncls, 4)
        assert np.array_equal(out.cpu().numpy(), want_out), (ncls, modes, 'mask')
        assert np.array_equal(stats.cpu().numpy(), want_stats), (ncls, modes, 'stats')
        # two calls give the same bytes; so do planes one byte off their alignment; so does a call without stats
        again, stats2 = M.mask_clean(lab, ncls, conn, modes, return_stats=True)
        assert torch.equal(again, out) and torch.equal(stats2, stats) and torch.equal(M.mask_components(lab, ncls, conn), comp)
        shifted, stats3 = M.mask_clean(odd, ncls, conn, modes, return_stats=True)
        assert torch.equal(shifted, out) and torch.equal(stats3, stats) and torch.equal(M.mask_components(odd, ncls, conn), comp)
        assert torch.equal(M.mask_clean(lab, ncls, conn, modes), out)
    assert torch.equal(lab.cpu(), torch.from_numpy(np.array(host)))                  # the input is read only


def test_mode_names_and_the_default():
    M = _ops()
    lab = torch.from_numpy(np.array(R.pattern('eyes_specks', (2, 67, 69)))).to(DEV)
    want = M.mask_clean(lab)
    assert torch.equal(M.mask_clean(lab, 4, 8, ('border', 'largest', 'largest', 'largest')), want)
    assert torch.equal(M.mask_clean(lab, 4, 8, (2, 1, 1, 1)), want) and torch.equal(M.mask_clean(lab, modes=M.default_modes(4)), want)
    assert not torch.equal(M.mask_clean(lab, modes=('all',) * 4), want)


# ------------------------------------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def _stores():
    store, truth = SR.learnable_store(64, 40)
    return store, truth, R.speckled(truth)


def _same_tree(a, b):
    assert sorted(a.keys()) == sorted(b.keys())
    for split in a.keys():
        assert sorted(a[split].keys()) == sorted(b[split].keys())
        for user in a[split].keys():
            assert sorted(a[split][user].keys()) == sorted(b[split][user].keys())
            for name in a[split][user].keys():
                x, y = np.asarray(a[split][user][name]), np.asarray(b[split][user][name])
                assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), (split, user, name)


def test_clean_store_returns_the_true_masks_and_their_rankings(capsys):
    from seg2eye_amd import mask_clean as MC, style_rank
    store, truth, noisy = _stores()
    for conn in (4, 8):
        cleaned = MC.clean_store(noisy, MC.MaskRule(4, conn), device=DEV, batch=3)
        _same_tree(cleaned, truth)
    lines = capsys.readouterr().out.splitlines()
    assert lines[0].startswith('train: 3 persons, 24 masks, ') and lines[1].startswith('validation: 2 persons, 16 masks, ')
    assert float(lines[0].split('masks, ')[1].split('%')[0]) > 0
    on_truth = style_rank.rank_styles(store, 'train', seg_store=truth, top=3, device=DEV)
    assert not K.same_refs(style_rank.rank_styles(store, 'train', seg_store=cleaned, top=3, device=DEV), on_truth)
    assert K.same_refs(style_rank.rank_styles(store, 'train', seg_store=noisy, top=3, device=DEV), on_truth)      # the specks move a ranking


def _net(nsf, dname, hw):
    from seg2eye_amd.segment import build_network, seg_options
    opt = seg_options(nsf=nsf, compute_dtype=dname, seg_hw=hw, batchSize=3)
    net = build_network(opt, DEV)
    sd = SR.hash_state(net, seed=0, dtype=torch.float64)
    with torch.no_grad():
        for k, v in net.state_dict().items():
            v.copy_(sd[k].float())
    return net, opt


def test_predict_masks_cleans_on_the_device():
    from seg2eye_amd import mask_clean as MC, segment
    M = _ops()
    store, _, _ = _stores()
    net, opt = _net(8, 'fp32', (64, 40))
    rule = MC.MaskRule(4, 8)
    raw = segment.predict_masks(net, store, 'validation', opt, device=DEV)
    assert all(np.array_equal(a, b) for u in raw['validation'] for a, b in
               zip(raw['validation'][u].values(), segment.predict_masks(net, store, 'validation', opt, device=DEV, clean=None)['validation'][u].values()))
    cleaned = segment.predict_masks(net, store, 'validation', opt, device=DEV, clean=rule)
    changed = 0
    for user, g in raw['validation'].items():
        assert sorted(cleaned['validation'][user]) == sorted(g)
        for name, m in g.items():
            want = M.mask_clean(torch.from_numpy(m).to(DEV), 4, 8).cpu().numpy()
            assert np.array_equal(cleaned['validation'][user][name], want), (user, name)
            changed += int((want != m).sum())
    assert changed > 0


class _OneHotNet:
    """A stand-in network whose masks are the given ones: one-hot logits of them, batch by batch in the order of the labelled samples
    (a value that names no class gives all-zero logits, which the argmax reads as class 0)."""

    def __init__(self, masks):
        self.masks, self.at = masks, 0

    def __call__(self, x):
        m = torch.from_numpy(self.masks[self.at:self.at + x.shape[0]].astype(np.int64)).to(x.device)
        self.at += x.shape[0]
        return (m[..., None] == torch.arange(4, device=x.device)).float().contiguous()


def test_eval_scores_raw_and_cleaned_masks():
    from seg2eye_amd import mask_clean as MC, segment
    store, _, _ = _stores()
    opt = segment.seg_options(seg_hw=(64, 40), compute_dtype='fp32', batchSize=4)
    truth = np.concatenate([store['validation'][u]['labels_ss'] for u in store['validation']])
    noisy = np.stack([R.specks(t, R.SEED * 1000 + 500 + i) for i, t in enumerate(truth)])
    assert (noisy != truth).any()
    got = MC.evaluate(_OneHotNet(noisy), store, 'validation', opt, MC.MaskRule(4, 8), device=DEV, verbose=False)
    keys = {'miou/validation', 'acc/validation'} | {'iou/validation/%d' % c for c in range(4)}
    assert set(got) == keys | {k.replace('/', '_clean/', 1) for k in keys}
    assert got['miou_clean/validation'] == 1.0 > got['miou/validation'] and got['acc_clean/validation'] == 1.0 > got['acc/validation']
    assert all(got['iou_clean/validation/%d' % c] == 1.0 for c in range(4))
    raw = segment.evaluate(_OneHotNet(noisy), store, 'validation', opt, DEV, verbose=False)
    assert all(got[k] == v for k, v in raw.items())                                 # the raw scores are segment eval's


def test_apply_from_the_shell(tmp_path):
    from seg2eye_amd import mask_clean as MC
    from seg2eye_amd.openeds_store import merge_splits, open_tree
    from seg2eye_amd.prepare_openeds import save_store
    _, _, noisy = _stores()
    paths = [save_store({split: noisy[split]}, str(tmp_path / ('masks_%s.h5' % split))) for split in ('train', 'validation')]
    r = subprocess.run([sys.executable, '-m', 'seg2eye_amd.mask_clean', 'apply', '--seg_file', ','.join(paths), '--out', str(tmp_path / 'clean.h5'),
                        '--conn', '4', '--modes', 'border,largest,largest,largest', '--batchSize', '5'],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert 'train: 3 persons, 24 masks' in r.stdout and 'validation: 2 persons, 16 masks' in r.stdout
    written = [p for p in (str(tmp_path / 'clean.h5'), str(tmp_path / 'clean.h5.npz')) if os.path.exists(p)]
    assert len(written) == 1 and written[0] in r.stdout
    want = MC.clean_store(noisy, MC.MaskRule(4, 4), device=DEV, verbose=False)
    _same_tree(merge_splits(written[0], open_tree), want)
