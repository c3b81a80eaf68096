"""The style reference ranking on the GPU: ops.mask_distances and ops.rank_topk, the raw entry points and the producer
seg2eye_amd.style_rank.rank_styles against the numpy restatement of tests/_style_rank_ref.py (int64 distances, np.lexsort selection).
Everything is integer: every comparison is ==, there is no tolerance in this file.

Targets and candidates are always unrelated maps and M != K wherever the shape allows, so a swapped row / column or a wrong fragment map
of the int8 MFMA cannot pass."""
import functools
import warnings

import numpy as np
import pytest
import torch

import _style_rank_ref as R
from _quality_harness import check_error_table

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
# one pixel; P = 391, odd: the padded path and a tail; exactly one MFMA step; P = 65, one byte past a step, M and K ragged against 16;
# several pixel chunks and two candidate tiles; the real mask: the full split and sums of 10^6
SHAPES = [(1, 1, 1, 1), (3, 5, 17, 23), (16, 16, 8, 8), (17, 33, 5, 13), (20, 70, 64, 100), (4, 6, 640, 400)]
SHAPE_IDS = ['x'.join(map(str, s)) for s in SHAPES]
METRICS = ['l2', 'mismatch']
KINDS = ['iid', 'eyes', 'same', 'extreme']


@functools.lru_cache(maxsize=None)
def _maps(shape, kind, ncls):
    """-> (targets, cands) uint8 numpy, never written to."""
    M, K, H, W = shape
    if kind == 'iid':
        return R.iid(M, H, W, ncls, 11), R.iid(K, H, W, ncls, 12)
    if kind == 'eyes':
        return R.eyes(M, H, W, ncls, 13), R.eyes(K, H, W, ncls, 14)
    if kind == 'same':                                       # every candidate is the target
        one = R.eyes(1, H, W, ncls, 15)
        return np.repeat(one, M, axis=0), np.repeat(one, K, axis=0)
    assert kind == 'extreme'                                 # the largest value there is
    return np.zeros((M, H, W), dtype=np.uint8), np.full((K, H, W), ncls - 1, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _want(shape, kind, ncls, metric):
    t, c = _maps(shape, kind, ncls)
    return R.distances(t, c, metric)


def _dev(a):
    return torch.from_numpy(a).to(DEV)


# ------------------------------------------------------------------------------------------------ distances
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('metric', METRICS)
@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
def test_mask_distances_equal_the_restatement(shape, metric, kind):
    from seg2eye_amd import ops
    t, c = _maps(shape, kind, 4)
    want = _want(shape, kind, 4, metric)
    got = ops.mask_distances(_dev(t), _dev(c), 4, metric)
    assert got.dtype == torch.int32 and tuple(got.shape) == (shape[0], shape[1])
    assert np.array_equal(got.cpu().numpy().astype(np.int64), want)
    P = shape[2] * shape[3]
    if kind == 'same':
        assert not want.any()
    if kind == 'extreme':
        assert (want == (9 * P if metric == 'l2' else P)).all()
        if P == 256000 and metric == 'l2':
            assert int(got[0, 0]) == 2304000


@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
def test_l2_with_seven_classes(shape):
    from seg2eye_amd import ops
    t, c = _maps(shape, 'iid', 7)
    got = ops.mask_distances(_dev(t), _dev(c), 7, 'l2')
    assert np.array_equal(got.cpu().numpy().astype(np.int64), _want(shape, 'iid', 7, 'l2'))


@pytest.mark.parametrize('metric', METRICS)
@pytest.mark.parametrize('shape,pitch', [((17, 33, 5, 13), 96), ((3, 5, 4, 8), 64), ((3, 5, 17, 23), 400)], ids=['P65', 'P32', 'P391'])
def test_padding_bytes_never_count(shape, pitch, metric):
    """The entry point itself with pitch > P: the padding filled with 3s, then with 0s."""
    from seg2eye_amd import _lib
    from seg2eye_amd.ops.core import _p, _stream
    M, K, H, W = shape
    P = H * W
    t, c = _maps(shape, 'iid', 4)
    want = R.distances(t, c, metric)
    got = []
    for fill in (3, 0):
        a = torch.full((M, pitch), fill, dtype=torch.uint8, device=DEV)
        b = torch.full((K, pitch), fill, dtype=torch.uint8, device=DEV)
        a[:, :P] = _dev(t).reshape(M, P)
        b[:, :P] = _dev(c).reshape(K, P)
        dist = torch.full((M, K), 12345, dtype=torch.int32, device=DEV)      # overwritten, not added to
        _lib.call.s2e_mask_dist(_p(a), _p(b), M, K, P, pitch, 4, {'l2': _lib.RANK_L2, 'mismatch': _lib.RANK_MISMATCH}[metric], _p(dist), _stream())
        got.append(dist.cpu())
    assert torch.equal(got[0], got[1])
    assert np.array_equal(got[0].numpy().astype(np.int64), want)


@pytest.mark.parametrize('metric', METRICS)
def test_two_calls_give_the_same_bits(metric):
    from seg2eye_amd import ops
    t, c = (_dev(x) for x in _maps((20, 70, 64, 100), 'eyes', 4))
    assert torch.equal(ops.mask_distances(t, c, 4, metric), ops.mask_distances(t, c, 4, metric))


# ------------------------------------------------------------------------------------------------ selection
@functools.lru_cache(maxsize=None)
def _dist_rows(K):
    """(5, K) int32: many ties; all equal; the whole int32 range; duplicated candidates; distances like the real ones."""
    rng = np.random.RandomState(K)
    half = rng.randint(0, 1000, (K + 1) // 2)
    rows = [rng.randint(0, 20, K), np.full(K, 7), rng.randint(-2 ** 31, 2 ** 31 - 1, K, dtype=np.int64),
            np.concatenate([half, half])[:K], rng.randint(0, 2304001, K)]
    d = np.stack(rows).astype(np.int32)
    if K > 2:
        d[2, K // 2], d[2, K - 1] = 2 ** 31 - 1, -2 ** 31
    return d


def _check_topk(d, k, exclude):
    from seg2eye_amd import ops
    want_idx, want_val = R.topk(d, k, exclude)
    idx, val = ops.rank_topk(_dev(d), k, None if exclude is None else _dev(exclude))
    assert idx.dtype == torch.int32 and val.dtype == torch.int32 and tuple(idx.shape) == tuple(val.shape) == (d.shape[0], k)
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    assert np.array_equal(val.cpu().numpy(), want_val)
    return want_idx


@pytest.mark.parametrize('k', [1, 4, 100])
@pytest.mark.parametrize('K', [1, 5, 64, 65, 1000, 5000])
def test_rank_topk_equals_the_restatement(K, k):
    from seg2eye_amd import ops
    assert 1000 <= ops.rank.max_candidates() < 5000          # K = 5000 takes the two-level path
    d = _dist_rows(K)
    best = _check_topk(d, k, None)
    assert list(best[1][:min(k, K)]) == list(range(min(k, K)))                               # all-equal distances: indices 0 .. k-1
    if k > K:
        assert (best[:, K:] == -1).all()
    # the best candidate of every row excluded (row 1: none; row 3: an index that does not exist)
    ex = best[:, 0].astype(np.int32).copy()
    ex[1], ex[3] = -1, K + 3
    without = _check_topk(d, k, ex)
    for m in (0, 2, 4):
        assert ex[m] not in without[m]
    if K == 1:
        assert (without[[0, 2, 4]] == -1).all()                                              # K' = 0: nothing to return
    _check_topk(d, k, ex.astype(np.int64))


def test_rank_topk_through_more_than_two_levels(monkeypatch):
    """With the per-launch limit lowered to 64 the winners of 5000 candidates are ranked in chunks twice before the last pass."""
    from seg2eye_amd import ops
    monkeypatch.setattr(ops.rank, 'max_candidates', lambda: 64)
    d = _dist_rows(5000)
    best = _check_topk(d, 4, None)
    _check_topk(d, 4, best[:, 0].astype(np.int32))
    _check_topk(d, 4, best[:, 2].astype(np.int32))


# ------------------------------------------------------------------------------------------------ refused calls
def test_entry_points_refuse_bad_calls_before_any_launch():
    """Every pointer is a real device buffer large enough for the sizes of its row, so nothing here could go out of bounds even if a
    row were let through."""
    from seg2eye_amd import _lib
    a = torch.zeros(4 * 64 + 16, dtype=torch.uint8, device=DEV)
    b = torch.zeros(4 * 64 + 16, dtype=torch.uint8, device=DEV)
    dist = torch.zeros(16, dtype=torch.int32, device=DEV)
    A, B, D = a.data_ptr(), b.data_ptr(), dist.data_ptr()
    assert A % 16 == 0 and B % 16 == 0
    L2, MIS = _lib.RANK_L2, _lib.RANK_MISMATCH
    ARG = 's2e_mask_dist: bad argument'
    SIZE = 's2e_mask_dist: M=%d K=%d P=%d (every size must be at least 1)'
    ALIGN = 's2e_mask_dist: a, b and pitch must be multiples of 16 bytes, dist of 4'
    NCLS = 's2e_mask_dist: ncls=%d (1 to %d classes for this metric)'
    #            a  b  M  K  P   pitch ncls metric dist stream
    table = [
        ((None, B, 4, 4, 64, 64, 4, L2, D, None), -1, ARG),
        ((A, None, 4, 4, 64, 64, 4, L2, D, None), -1, ARG),
        ((A, B, 4, 4, 64, 64, 4, L2, None, None), -1, ARG),
        ((A, B, 4, 4, 64, 64, 4, 2, D, None), -1, 's2e_mask_dist: bad metric 2'),
        ((A, B, 4, 4, 64, 64, 4, -1, D, None), -1, 's2e_mask_dist: bad metric -1'),
        ((A, B, 0, 4, 64, 64, 4, L2, D, None), -1, SIZE % (0, 4, 64)),
        ((A, B, 4, 0, 64, 64, 4, MIS, D, None), -1, SIZE % (4, 0, 64)),
        ((A, B, 4, 4, 0, 64, 4, L2, D, None), -1, SIZE % (4, 4, 0)),
        ((A, B, 4, 4, 64, 48, 4, L2, D, None), -1, 's2e_mask_dist: pitch=48 is below P=64'),
        ((A, B, 4, 4, 20, 24, 4, L2, D, None), -1, ALIGN),
        ((A + 1, B, 4, 4, 64, 64, 4, L2, D, None), -1, ALIGN),
        ((A, B + 8, 4, 4, 64, 64, 4, MIS, D, None), -1, ALIGN),
        ((A, B, 4, 4, 64, 64, 4, L2, D + 2, None), -1, ALIGN),
        ((A, B, 4, 4, 64, 64, 0, L2, D, None), -3, NCLS % (0, 128)),
        ((A, B, 4, 4, 64, 64, 129, L2, D, None), -3, NCLS % (129, 128)),
        ((A, B, 4, 4, 64, 64, 0, MIS, D, None), -3, NCLS % (0, 16)),
        ((A, B, 4, 4, 64, 64, 17, MIS, D, None), -3, NCLS % (17, 16)),
        ((A, B, 1, 1, 256000, 256000, 128, L2, D, None), -3, 's2e_mask_dist: (ncls-1)^2 P = 127^2 x 256000 does not fit int32'),
        ((A, B, 1, 1, 9544372, 9544384, 16, MIS, D, None), -3, 's2e_mask_dist: (ncls-1)^2 P = 15^2 x 9544372 does not fit int32'),
    ]
    check_error_table('s2e_mask_dist', table)
    idx = torch.zeros(16, dtype=torch.int32, device=DEV)
    val = torch.zeros(16, dtype=torch.int32, device=DEV)
    I, V = idx.data_ptr(), val.data_ptr()
    limit = _lib.lib().s2e_rank_topk_max_candidates()
    TARG = 's2e_rank_topk: bad argument'
    TSIZE = 's2e_rank_topk: M=%d K=%d k=%d (every size must be at least 1)'
    #            dist M  K  k  exclude idx val stream
    table = [
        ((None, 2, 4, 2, None, I, V, None), -1, TARG),
        ((D, 2, 4, 2, None, None, V, None), -1, TARG),
        ((D, 2, 4, 2, None, I, None, None), -1, TARG),
        ((D, 0, 4, 2, None, I, V, None), -1, TSIZE % (0, 4, 2)),
        ((D, 2, 0, 2, None, I, V, None), -1, TSIZE % (2, 0, 2)),
        ((D, 2, 4, 0, None, I, V, None), -1, TSIZE % (2, 4, 0)),
        ((D, 2, 4, -3, None, I, V, None), -1, TSIZE % (2, 4, -3)),
        ((D, 1, limit + 1, 2, None, I, V, None), -3,
         's2e_rank_topk: K=%d candidates, one launch takes %d (rank chunks, then the winners)' % (limit + 1, limit)),
    ]
    check_error_table('s2e_rank_topk', table)
    torch.cuda.synchronize()
    assert not dist.any() and not idx.any() and not val.any()                                # nothing was launched


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope='module')
def stores():
    """Three persons at 640 x 400; U003 has 101 generative frames in 'train', so that top = 100 is full for it."""
    train, seg_train = R.eye_store(seed=2, n_gen=(5, 6, 101), keys=('train',))
    test, seg_test = R.eye_store(seed=3, keys=('test',))
    return {**train, **test}, {**seg_train, **seg_test}


def _opt(key, method, is_train=True):
    from seg2eye_amd.options import parse
    return parse(['--dataset_mode', 'openeds', '--dataset_key', key, '--crop_size', '64', '--aspect_ratio', '0.8', '--no_flip',
                  '--style_sample_method', method], is_train=is_train)


def _frames(store, key, user, entry, n):
    """The frames the ranking names first, from the store."""
    g = store[key][user]
    images = 'images_ss' if key == 'test' else 'images_gen'
    n_g = g[images].shape[0]
    return np.stack([g['images_seq'][i - n_g] if s == b's' else g[images][i] for i, s in zip(entry['index'][:n], entry['subset'][:n])])


@pytest.mark.filterwarnings('ignore:.*fewer than top')
def test_producer_and_dataset_end_to_end_on_train(stores, tmp_path):
    from seg2eye_amd import style_rank as S
    from seg2eye_amd.openeds_dataset import OpenEDSDataset
    store, seg = stores
    want = R.rank_styles(store, 'train', seg, top=100)
    with pytest.warns(UserWarning, match='fewer than top = 100') as rec:
        refs = S.rank_styles(store, 'train', seg_store=seg, top=100)
    assert len(rec) == 1 and 'U003' not in str(rec[0].message)
    assert not R.same_refs(refs, want)
    assert len(refs['train']['U003']['U003002_ss']['index']) == 100
    assert not R.same_refs(S.rank_styles(store, 'train', seg_store=seg, top=5, metric='mismatch', use_seq=False),
                           R.rank_styles(store, 'train', seg, top=5, metric='mismatch', use_seq=False))
    # ref_first: the frames the restatement names; U001 has 5 generative and 2 sequence frames, so 6 styles hold a sequence frame
    ds = OpenEDSDataset(_opt('train', 'ref_first'), store=store, style_refs=refs)
    entry = want['train']['U001']['U001001_ss']
    assert b's' in list(entry['subset'][:6])
    got, _, sub = ds.get_style_images('U001', 6, None, 'U001001_ss')
    assert [bytes(s) for s in sub] == [bytes(s) for s in entry['subset'][:6]]
    assert np.array_equal(got.numpy(), _frames(store, 'train', 'U001', entry, 6))
    item = ds[1]
    assert item['filename'] == 'U001001_ss' and item['style_image'].shape[0] == ds.opt.input_ns
    # ref_random100 indexes 100 entries: U003 has them
    rnd = OpenEDSDataset(_opt('train', 'ref_random100'), store=store, style_refs=refs, rng=np.random.RandomState(0))
    item = rnd[5 + 2]                                        # U003's target 2
    assert item['user'] == 'U003' and item['style_image'].shape[0] == rnd.opt.input_ns
    # the file
    path = S.save_refs(refs, str(tmp_path / 'style_refs'))
    if path.endswith('.npz'):
        assert not R.same_refs(S.load_refs(path), refs)
    else:
        import h5py
        with h5py.File(path, 'r') as f:
            back = {s: {u: {n: {k: np.asarray(v) for k, v in e.items()} for n, e in fs.items()} for u, fs in us.items()} for s, us in f.items()}
        assert not R.same_refs(back, refs)


def test_producer_and_dataset_end_to_end_on_test(stores):
    from seg2eye_amd import style_rank as S
    from seg2eye_amd.openeds_dataset import OpenEDSDataset
    store, seg = stores
    want = R.rank_styles(store, 'test', None, top=3)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        refs = S.rank_styles(store, 'test', top=3)           # the true labels_ss: no seg_store
    assert not R.same_refs(refs, want)
    assert 2 not in refs['test']['U001']['U001_001_gen']['index']                            # that labelled frame carries the target's name
    ds = OpenEDSDataset(_opt('test', 'ref_first', is_train=False), store=store, style_refs=refs)
    entry = want['test']['U003']['U003_001_gen']
    got, _, _ = ds.get_style_images('U003', 3, None, 'U003_001_gen')
    assert np.array_equal(got.numpy(), _frames(store, 'test', 'U003', entry, 3))
