"""The mask cleaner without a GPU: the restatement (tests/_mask_clean_ref.py) against a literal breadth-first search and,
where it imports, scipy; the tie rules on hand-made maps; the default modes; the stats identities; the recovery of speckled eye masks;
`clean_store` with a fake op; the parser; the ops' ValueErrors; every refused call of the C ABI with its code and message."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _mask_clean_ref as R
import _segment_ref as SR

P = 4096                                                      # a dummy non-null pointer: must never reach a kernel
BIG = 1 << 40                                                 # a workspace size that is never short
ARG, UNSUPPORTED = -1, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('s2e_mask_clean_workspace_bytes', 's2e_mask_components', 's2e_mask_clean')
SMALL = [(1, 1, 1), (1, 1, 9), (1, 9, 1), (2, 5, 7), (1, 12, 11)]


# ------------------------------------------------------------------------------------------------ the restatement alone
@pytest.mark.parametrize('shape', SMALL, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('kind', R.PATTERNS)
def test_restated_components_are_a_breadth_first_searchs(kind, shape):
    lab = R.pattern(kind, shape)
    for conn in (4, 8):
        for ncls in (1, 4, 16):
            for n in range(shape[0]):
                comp = R.components(lab[n], ncls, conn)
                assert np.array_equal(comp, R.components_bfs(lab[n], ncls, conn)), (conn, ncls, n)
                assert ((comp < 0) == (lab[n] >= ncls)).all()


@pytest.mark.parametrize('kind', R.PATTERNS)
def test_two_pass_fill_is_the_brute_force_one(kind):
    lab = R.pattern(kind, (1, 23, 31))[0]
    for modes in (None, (0,) * 4, (1,) * 4, (2,) * 4):
        a, b = R.clean(lab, 4, 8, modes, brute=True), R.clean(lab, 4, 8, modes, brute=False)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize('conn', [4, 8])
@pytest.mark.parametrize('kind', ['iid4', 'iid2', 'rings', 'iid_ignore', 'eyes_specks', 'spiral'])
def test_restatement_is_scipys(kind, conn):
    """Components through scipy.ndimage.label (their ids renamed to the smallest index), the fill through distance_transform_edt's
    nearest-pixel indices -- another algorithm for the same rule."""
    ndi = pytest.importorskip('scipy.ndimage')
    lab = R.pattern(kind, (1, 40, 33))[0]
    H, W = lab.shape
    st = np.ones((3, 3), int) if conn == 8 else ndi.generate_binary_structure(2, 1)
    comp = -np.ones((H, W), dtype=np.int64)
    for c in range(4):
        cc, n = ndi.label(lab == c, structure=st)
        for i in range(1, n + 1):
            comp[cc == i] = np.flatnonzero(cc == i)[0]
    assert np.array_equal(comp, R.components(lab, 4, conn))
    for modes in (None, (1,) * 4):
        out, _, _ = R.clean(lab, 4, conn, modes)
        kept, _ = R.kept_mask(lab, comp, 4, modes or R.default_modes(4))
        yy, xx = np.mgrid[0:H, 0:W]
        best, cls = np.full((H, W), R.BIG), np.zeros((H, W), np.uint8)
        for c in range(4):
            m = kept & (lab == c)
            if m.any():
                _, (iy, ix) = ndi.distance_transform_edt(~m, return_indices=True)
                d2 = (iy - yy).astype(np.int64) ** 2 + (ix - xx).astype(np.int64) ** 2
                upd = d2 < best
                best[upd], cls[upd] = d2[upd], c
        want = lab.copy()
        want[~kept] = cls[~kept]
        assert np.array_equal(out, want)


def test_tie_rules_on_hand_made_maps():
    # equal areas: of the two 1-pieces of two pixels the one with the smaller id stays; the other takes the nearest kept class
    lab = np.array([[1, 1, 0, 1, 1],
                    [0, 0, 0, 0, 0],
                    [0, 0, 0, 0, 0]], dtype=np.uint8)
    out, stats, comp = R.clean(lab, 2, 4, (R.ALL, R.LARGEST))
    assert comp[0].tolist() == [0, 0, 2, 3, 3] and out[0].tolist() == [1, 1, 0, 0, 0]
    assert stats.tolist() == [[1, 11, 0, 13], [2, 4, 2, 2]]
    # equidistant classes: the ignored pixel in the middle is as far from class 1 as from class 0 and 2 -- the lower class wins
    lab = np.array([[1, 1, 1, 1, 1],
                    [2, 2, 255, 0, 0],
                    [2, 2, 2, 2, 2]], dtype=np.uint8)
    out, stats, _ = R.clean(lab, 3, 4, (R.ALL,) * 3)
    assert out[1, 2] == 0 and (out != lab).sum() == 1
    lab[1, 3:] = 1
    assert R.clean(lab, 3, 4, (R.ALL,) * 3)[0][1, 2] == 1
    # a diagonal pair: two components under 4-connectivity, one under 8
    lab = np.array([[0, 0, 0, 0, 0],
                    [0, 1, 0, 0, 0],
                    [0, 0, 1, 0, 0]], dtype=np.uint8)
    c4, c8 = R.components(lab, 2, 4), R.components(lab, 2, 8)
    assert c4[1, 1] == 6 and c4[2, 2] == 12 and c8[1, 1] == 6 and c8[2, 2] == 6
    out4, s4, _ = R.clean(lab, 2, 4, (R.ALL, R.LARGEST))
    out8, s8, _ = R.clean(lab, 2, 8, (R.ALL, R.LARGEST))
    assert out4[1, 1] == 1 and out4[2, 2] == 0 and s4[1].tolist() == [2, 2, 1, 1]
    assert np.array_equal(out8, lab) and s8[1].tolist() == [1, 2, 0, 2]
    # the 0s around the pair are one piece either way
    assert (c4[lab == 0] == 0).all() and (c8[lab == 0] == 0).all()
    # border: an island of class 0 inside class 1 is a hole, the frame's 0 stays
    lab = np.array([[0, 1, 1, 1, 0],
                    [0, 1, 0, 1, 0],
                    [0, 1, 1, 1, 0]], dtype=np.uint8)
    out, stats, _ = R.clean(lab, 2, 4, (R.BORDER, R.LARGEST))
    assert out[1, 2] == 1 and (out != lab).sum() == 1 and stats.tolist() == [[3, 7, 1, 6], [1, 8, 0, 9]]
    # an image that keeps nothing comes back unchanged
    lab = np.full((3, 5), 255, dtype=np.uint8)
    lab[1, 2] = 0
    out, stats, _ = R.clean(lab, 1, 8, (R.BORDER,))
    assert np.array_equal(out, lab) and stats.tolist() == [[1, 1, 1, 0]]


def test_default_modes():
    from seg2eye_amd.ops import mask_clean as M
    assert M.default_modes(4) == (2, 1, 1, 1) == R.default_modes(4)
    assert M.default_modes(1) == (2,) and M.default_modes(16) == (2,) + (1,) * 15 == R.default_modes(16)
    for bad in (0, 17):
        with pytest.raises(ValueError):
            M.default_modes(bad)


@pytest.mark.parametrize('kind', R.PATTERNS)
def test_stats_identities(kind):
    lab = R.pattern(kind, (2, 23, 31))
    for ncls, modes in ((4, None), (4, (2,) * 4), (1, None), (16, None)):
        out, stats, comp = R.clean_batch(lab, ncls, 8, modes)
        s = stats.astype(np.int64)
        for n in range(len(lab)):
            kept, _ = R.kept_mask(lab[n], comp[n], ncls, modes or R.default_modes(ncls))
            filled = np.array([((out[n] == c) & ~kept).sum() for c in range(ncls)])      # (a removed pixel may be filled into its own class again)
            keeps = kept.any()
            assert keeps == (s[n, :, 1].sum() > s[n, :, 2].sum())
            assert np.array_equal(s[n, :, 1] - s[n, :, 2] + (filled if keeps else 0), s[n, :, 3])      # before - removed + filled-into = after
            assert s[n, :, 3].sum() == ((out[n] < ncls).sum() if keeps else 0) and (not keeps or (out[n] < ncls).all())
            assert np.array_equal(s[n, :, 0], [len(np.unique(comp[n][lab[n] == c])) for c in range(ncls)])


def test_cleaning_recovers_speckled_eye_masks():
    """Specks whose dilated footprint lies inside one true class: with (border, largest, largest, largest) and either connectivity the
    cleaned mask is the truth, exactly."""
    _, truth = SR.learnable_store(64, 40)
    noisy = R.speckled(truth)
    changed = 0
    for split in truth:
        for user in truth[split]:
            for name, t in truth[split][user].items():
                changed += int((noisy[split][user][name] != t).sum())
                for conn in (4, 8):
                    assert np.array_equal(R.clean_batch(noisy[split][user][name], 4, conn)[0], t), (split, user, name, conn)
    assert changed > 1000
    store, _ = SR.learnable_store(64, 40)                         # ... and the labelled frames the eval test corrupts, with its seeds
    labelled = np.concatenate([store['validation'][u]['labels_ss'] for u in store['validation']])
    noisy = np.stack([R.specks(t, R.SEED * 1000 + 500 + i) for i, t in enumerate(labelled)])
    assert (noisy != labelled).any() and np.array_equal(R.clean_batch(np.where(noisy == 255, 0, noisy).astype(np.uint8), 4, 8)[0], labelled)


def test_cleaned_masks_rank_as_the_truth_and_speckled_ones_do_not():
    """The seed of the GPU end-to-end test, checked with the restatements: rankings on the cleaned masks are those on the truth, and
    the speckled masks rank at least one target differently."""
    import _style_rank_ref as K
    store, truth = SR.learnable_store(64, 40)
    noisy = R.speckled(truth)
    want = K.rank_styles(store, 'train', seg_store=truth, top=3)
    assert K.same_refs(K.rank_styles(store, 'train', seg_store=noisy, top=3), want)


# ------------------------------------------------------------------------------------------------ the stage
def test_clean_store_keeps_the_layout(monkeypatch, capsys):
    from seg2eye_amd import mask_clean as MC
    from seg2eye_amd.ops import mask_clean as M
    calls = []

    def fake(labels, ncls=4, conn=8, modes=None, return_stats=False):
        calls.append((tuple(labels.shape), ncls, conn, modes))
        stats = torch.zeros(labels.shape[0], ncls, 4, dtype=torch.int32)
        stats[:, :, 0], stats[:, 1, 2], stats[:, 0, 3] = 2, 3, 3
        return (255 - labels, stats) if return_stats else 255 - labels
    monkeypatch.setattr(M, 'mask_clean', fake)
    rng = np.random.RandomState(0)
    tree = {'train': {'U1': {'labels_pred_gen': rng.randint(0, 4, (5, 6, 4)).astype(np.uint8), 'labels_pred_seq': rng.randint(0, 4, (2, 6, 4)).astype(np.uint8)},
                      'U2': {'labels_pred_gen': rng.randint(0, 4, (1, 6, 4)).astype(np.uint8), 'note': np.arange(3)}},
            'validation': {'U3': {'labels_pred_seq': np.zeros((0, 6, 4), np.uint8)}}}
    out = MC.clean_store(tree, MC.MaskRule(4, 4, ('all', 'largest', 'border', 'all')), device='cpu', batch=2)
    assert sorted(out) == ['train', 'validation'] and sorted(out['train']) == ['U1', 'U2'] and sorted(out['train']['U1']) == ['labels_pred_gen', 'labels_pred_seq']
    for user, g in tree['train'].items():
        for name, a in g.items():
            got = out['train'][user][name]
            assert got.dtype == a.dtype and np.array_equal(got, 255 - a if name.startswith('labels_pred_') else a)
    assert out['validation']['U3']['labels_pred_seq'].shape == (0, 6, 4)
    assert [c[0] for c in calls] == [(2, 6, 4), (2, 6, 4), (1, 6, 4), (2, 6, 4), (1, 6, 4)]
    assert all(c[1:] == (4, 4, ('all', 'largest', 'border', 'all')) for c in calls)
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == 'train: 2 persons, 8 masks, %.4f%% of the pixels changed, 4.00 components beyond one per class and mask' % (100.0 * 8 * 6 / (8 * 24))
    assert lines[1].startswith('validation: 1 persons, 0 masks, 0.0000%')


def test_parser_defaults():
    from seg2eye_amd import mask_clean as MC
    a = vars(MC.parser().parse_args(['apply', '--seg_file', 'a.h5,b.h5', '--out', 'c.h5']))
    assert (a['command'], a['seg_file'], a['out'], a['conn'], a['modes'], a['label_nc'], a['batchSize']) == ('apply', 'a.h5,b.h5', 'c.h5', 8, None, 4, 64)
    rule = MC.rule_of(a)
    assert (rule.ncls, rule.conn, rule.modes) == (4, 8, None)
    e = vars(MC.parser().parse_args(['eval', '--dataroot', 'all.h5', '--name', 'seg', '--modes', 'border,largest,largest,all', '--conn', '4']))
    assert (e['command'], e['dataroot'], e['name'], e['dataset_key'], e['which_epoch'], e['conn'], e['label_nc']) == ('eval', 'all.h5', 'seg', 'validation', 'latest', 4, 4)
    assert e['modes'] == ('border', 'largest', 'largest', 'all') and e['seg_hw'] == (320, 200) and e['nsf'] == 32 and e['batchSize'] == 16
    for bad in (['apply', '--out', 'c.h5'], ['apply', '--seg_file', 'a', '--out', 'c', '--conn', '6'], ['apply', '--seg_file', 'a', '--out', 'c', '--modes', 'biggest'],
                ['eval', '--name', 'seg']):
        with pytest.raises(SystemExit):
            MC.parser().parse_args(bad)


def test_segment_and_refine_command_lines_have_not_moved():
    from seg2eye_amd import segment
    import inspect
    assert inspect.signature(segment.predict_masks).parameters['clean'].default is None
    assert '--clean' not in segment.parser().format_help()


# ------------------------------------------------------------------------------------------------ the ops' checks
def test_op_checks_come_before_the_device():
    from seg2eye_amd import _lib
    from seg2eye_amd.ops import mask_clean as M
    lab = torch.zeros(2, 5, 7, dtype=torch.uint8)
    for fn in (M.mask_components, M.mask_clean):
        for bad, kw in ((lab.int(), {}), (lab[0], {}), (torch.zeros(2, 0, 7, dtype=torch.uint8), {}), (torch.zeros(1, 1025, 2, dtype=torch.uint8), {}),
                        (lab, dict(conn=6)), (lab, dict(ncls=0)), (lab, dict(ncls=17))):
            with pytest.raises(ValueError):
                fn(bad, **kw)
        with pytest.raises(_lib.Seg2EyeHipError, match='GPU only'):
            fn(lab)
    for modes in ((1, 1, 1), (1, 1, 1, 3), (1, 1, 1, -1), ('all', 'largest', 'border', 'biggest'), (0.5, 1, 1, 1)):
        with pytest.raises(ValueError, match='modes'):
            M.mask_clean(lab, modes=modes)
    with pytest.raises(_lib.Seg2EyeHipError, match='GPU only'):
        M.mask_clean(lab, modes=('all', 'largest', 'border', 2))


# ------------------------------------------------------------------------------------------------ declared, exported, bound, built
def test_new_symbols_are_declared_exported_and_bound():
    from seg2eye_amd import _lib, build
    header = open(os.path.join(ROOT, 'include', 'seg2eye_hip.h')).read()
    for name in NEW:
        assert re.search(r'\b%s\(' % name, header), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name), name
    assert 'mask_clean.hip' in build.SOURCES and os.path.exists(os.path.join(build.CSRC, 'mask_clean.hip'))
    assert 'HOST pointer' in header                                    # the modes arrive as a host pointer, and the header says so
    seg_loss = open(os.path.join(build.CSRC, 'seg_loss.hip')).read()
    clean = open(os.path.join(build.CSRC, 'mask_clean.hip')).read()
    assert '#include "seg_dist.h"' in seg_loss and '#include "seg_dist.h"' in clean and 'DIST_NONE16 =' not in seg_loss + clean


# ------------------------------------------------------------------------------------------------ refused calls
MODES = (ctypes.c_uint8 * 16)(2, 1, 1, 1)
MODES_AT = ctypes.addressof(MODES)


def _comp(labels=P, N=2, H=8, W=8, ncls=4, conn=8, comp=P):
    return (labels, N, H, W, ncls, conn, comp, None)


def _clean(labels=P, N=2, H=8, W=8, ncls=4, conn=8, modes=MODES_AT, out=P, stats=P, ws=P, wsb=BIG):
    return (labels, N, H, W, ncls, conn, modes, out, stats, ws, wsb, None)


def _refused(fn, args, code, text):
    from seg2eye_amd import _lib
    L = _lib.lib()
    assert getattr(L, fn)(*args) == code, (fn, args)
    msg = L.s2e_last_error().decode()
    assert msg.startswith(fn + ': ') and text in msg, msg


def test_refused_calls_of_mask_components():
    _refused('s2e_mask_components', _comp(labels=None), ARG, 'bad argument')
    _refused('s2e_mask_components', _comp(comp=None), ARG, 'bad argument')
    for kw in (dict(N=0), dict(H=0), dict(W=-1)):
        _refused('s2e_mask_components', _comp(**kw), ARG, 'every size must be at least 1')
    _refused('s2e_mask_components', _comp(conn=6), ARG, 'conn=6 (4 or 8)')
    for ncls in (0, 17):
        _refused('s2e_mask_components', _comp(ncls=ncls), UNSUPPORTED, 'ncls=%d (1 to 16 classes)' % ncls)
    _refused('s2e_mask_components', _comp(H=1025), UNSUPPORTED, 'each at most 1024')
    _refused('s2e_mask_components', _comp(N=65536, H=1, W=1), UNSUPPORTED, 'beyond the launch limits')
    _refused('s2e_mask_components', _comp(N=2048, H=1024, W=1024), UNSUPPORTED, 'beyond the launch limits')
    # the order: a null pointer before a bad size, conn before ncls, ncls before the sides
    _refused('s2e_mask_components', _comp(labels=None, N=0), ARG, 'bad argument')
    _refused('s2e_mask_components', _comp(conn=5, ncls=99), ARG, 'conn=5')
    _refused('s2e_mask_components', _comp(ncls=99, W=4096), UNSUPPORTED, 'ncls=99')


def test_refused_calls_of_mask_clean():
    from seg2eye_amd import _lib
    L = _lib.lib()
    for kw in (dict(labels=None), dict(out=None), dict(modes=None), dict(ws=None)):
        _refused('s2e_mask_clean', _clean(**kw), ARG, 'bad argument')
    need = L.s2e_mask_clean_workspace_bytes(2, 8, 8, 4)
    assert need > 0 and need % 256 == 0
    _refused('s2e_mask_clean', _clean(wsb=need - 1), ARG, 'workspace of %d bytes, needs %d' % (need - 1, need))
    _refused('s2e_mask_clean', _clean(ws=P + 4), ARG, '8-byte aligned')
    for kw in (dict(N=0), dict(H=0), dict(W=-1)):
        _refused('s2e_mask_clean', _clean(wsb=0, **kw), ARG, 'every size must be at least 1')        # (a refused shape needs 0 bytes)
    _refused('s2e_mask_clean', _clean(conn=0), ARG, 'conn=0 (4 or 8)')
    for ncls in (0, 17):
        _refused('s2e_mask_clean', _clean(ncls=ncls, wsb=0), UNSUPPORTED, 'ncls=%d (1 to 16 classes)' % ncls)
    bad = (ctypes.c_uint8 * 16)(2, 1, 3, 1)
    _refused('s2e_mask_clean', _clean(modes=ctypes.addressof(bad)), ARG, 'modes[2]=3')
    _refused('s2e_mask_clean', _clean(W=1025, wsb=0), UNSUPPORTED, 'H=8 W=1025 (each at most 1024)')
    _refused('s2e_mask_clean', _clean(N=65536, H=1, W=1, wsb=0), UNSUPPORTED, 'beyond the launch limits')
    _refused('s2e_mask_clean', _clean(N=2048, H=1024, W=1024, wsb=0), UNSUPPORTED, 'beyond the launch limits')
    # the order: null pointers, the workspace, the sizes, conn, ncls, the modes, the sides, the batch
    _refused('s2e_mask_clean', _clean(out=None, wsb=0), ARG, 'bad argument')
    _refused('s2e_mask_clean', _clean(wsb=0, conn=5), ARG, 'workspace of 0 bytes')
    _refused('s2e_mask_clean', _clean(N=0, conn=5, wsb=0), ARG, 'every size')
    _refused('s2e_mask_clean', _clean(conn=5, ncls=99, wsb=0), ARG, 'conn=5')
    _refused('s2e_mask_clean', _clean(ncls=99, modes=ctypes.addressof(bad), wsb=0), UNSUPPORTED, 'ncls=99')
    _refused('s2e_mask_clean', _clean(modes=ctypes.addressof(bad), W=4096, wsb=0), ARG, 'modes[2]=3')
    _refused('s2e_mask_clean', _clean(N=65536, W=4096, wsb=0), UNSUPPORTED, 'each at most')
    # a mode byte behind ncls is not read as a mode
    assert L.s2e_mask_clean(*_clean(modes=ctypes.addressof(bad), ncls=2, W=4096, wsb=0)) == UNSUPPORTED
    assert b'each at most' in L.s2e_last_error()


def test_workspace_sizes():
    from seg2eye_amd import _lib
    L = _lib.lib()
    al = lambda b: (b + 255) // 256 * 256
    for N, H, W, ncls in ((1, 1, 1, 1), (2, 5, 7, 4), (16, 640, 400, 4), (3, 1024, 1024, 16)):
        px = N * H * W
        assert L.s2e_mask_clean_workspace_bytes(N, H, W, ncls) == 3 * al(4 * px) + al(N * 16 * 24) + al(N * ncls * 16) + al(2 * px * ncls)
    for bad in ((0, 8, 8, 4), (1, 0, 8, 4), (1, 8, 0, 4), (1, 8, 8, 0), (1, 8, 8, 17), (1, 1025, 8, 4), (1, 8, 1025, 4), (65536, 1, 1, 4), (2048, 1024, 1024, 4)):
        assert L.s2e_mask_clean_workspace_bytes(*bad) == 0, bad
