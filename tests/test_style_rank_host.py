"""The style reference ranking without a GPU: the numpy restatement (tests/_style_rank_ref.py) against a brute-force double
loop, the producer's walk with the restatement in the place of the two ops, the ops' ValueErrors, and the .npz path of --style_ref."""
import warnings

import numpy as np
import pytest
import torch

import _style_rank_ref as R


# ------------------------------------------------------------------------------------------------ the restatement alone
@pytest.mark.parametrize('metric', ['l2', 'mismatch'])
def test_restated_distances_equal_a_double_loop(metric):
    t, c = R.iid(3, 4, 5, 4, 0), R.iid(4, 4, 5, 4, 1)
    want = np.zeros((3, 4), dtype=np.int64)
    for m in range(3):
        for k in range(4):
            for y in range(4):
                for x in range(5):
                    a, b = int(t[m, y, x]), int(c[k, y, x])
                    want[m, k] += (a - b) ** 2 if metric == 'l2' else int(a != b)
    assert np.array_equal(R.distances(t, c, metric), want)


def test_restated_selection_equals_a_double_loop():
    rng = np.random.RandomState(2)
    d = rng.randint(0, 4, (5, 9))                            # many ties
    ex = np.array([-1, 0, 3, 8, -1])
    for k in (1, 4, 12):
        idx, val = R.topk(d, k, ex)
        for m in range(5):
            pairs = sorted((int(d[m, j]), j) for j in range(9) if j != ex[m])[:k]
            assert [int(i) for i in idx[m][:len(pairs)]] == [j for _, j in pairs]
            assert [int(v) for v in val[m][:len(pairs)]] == [v for v, _ in pairs]
            assert (idx[m][len(pairs):] == -1).all() and (val[m][len(pairs):] == -1).all()
    assert np.array_equal(R.topk(np.zeros((2, 6)), 3)[0], [[0, 1, 2], [0, 1, 2]])


def test_eyes_are_nested_and_differ():
    e = R.eyes(3, 64, 40, 4, 7)
    assert e.dtype == np.uint8 and set(np.unique(e)) == {0, 1, 2, 3} and not np.array_equal(e[0], e[1])
    assert R.distances(e[:1], e[:1])[0, 0] == 0 and R.distances(e[:1], e[1:2])[0, 0] > 0


# ------------------------------------------------------------------------------------------------ the producer's walk
@pytest.fixture()
def restated_ops(monkeypatch):
    """seg2eye_amd.ops.rank's two ops replaced by the restatement, on CPU tensors; -> the list of (M, K) of every distance call."""
    from seg2eye_amd.ops import rank
    calls = []

    def mask_distances(t, c, ncls, metric='l2'):
        calls.append((t.shape[0], c.shape[0]))
        return torch.from_numpy(R.distances(t.numpy(), c.numpy(), metric).astype(np.int32))

    def rank_topk(dist, k, exclude=None):
        idx, val = R.topk(dist.numpy(), k, None if exclude is None else exclude.numpy())
        return torch.from_numpy(idx), torch.from_numpy(val)
    monkeypatch.setattr(rank, 'mask_distances', mask_distances)
    monkeypatch.setattr(rank, 'rank_topk', rank_topk)
    return calls


@pytest.fixture(scope='module')
def small_store():
    return R.eye_store(seed=1, H=32, W=20)


@pytest.mark.filterwarnings('ignore:.*fewer than top')
def test_walk_names_offsets_subsets_and_exclusion(restated_ops, small_store):
    from seg2eye_amd import style_rank as S
    store, seg = small_store
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        refs = S.rank_styles(store, 'train', seg_store=seg, top=4, device='cpu')
    assert list(refs) == ['train'] and list(refs['train']) == ['U001', 'U002', 'U003']
    assert sorted(refs['train']['U001']) == ['U001000_ss', 'U001001_ss', 'U001002_ss']          # decoded, the dot removed
    assert not R.same_refs(refs, R.rank_styles(store, 'train', seg, top=4))
    e = refs['train']['U002']['U002001_ss']
    assert e['index'].dtype == np.int64 and e['subset'].dtype == np.dtype('S1') and e['distance'].dtype == np.int32
    # every one of U002's 6 + 3 candidates, in order: the sequence frames sit behind the generative ones
    full = S.rank_styles(store, 'train', seg_store=seg, top=9, device='cpu')['train']['U002']['U002000_ss']
    assert sorted(full['index']) == list(range(9))
    assert all((s == b's') == (i >= 6) for i, s in zip(full['index'], full['subset']))
    d = R.distances(store['train']['U002']['labels_ss'][:1], np.concatenate([seg['train']['U002']['labels_pred_gen'], seg['train']['U002']['labels_pred_seq']]))[0]
    assert np.array_equal(full['distance'], d[full['index']]) and np.array_equal(full['distance'], np.sort(d))
    # U001's generative frame 1 carries the name of target 0: never its style, but every other target's candidate
    u1 = S.rank_styles(store, 'train', seg_store=seg, top=7, device='cpu')['train']['U001']
    assert 1 not in u1['U001000_ss']['index'] and len(u1['U001000_ss']['index']) == 6
    assert 1 in u1['U001001_ss']['index'] and len(u1['U001001_ss']['index']) == 7
    # without the sequence frames: generative indices only
    g = S.rank_styles(store, 'train', seg_store=seg, top=9, use_seq=False, device='cpu')['train']['U002']['U002000_ss']
    assert sorted(g['index']) == list(range(6)) and set(g['subset']) == {b'g'}


def test_walk_of_the_test_split_needs_no_seg_store(restated_ops, small_store):
    from seg2eye_amd import style_rank as S
    store, seg = small_store
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        refs = S.rank_styles(store, 'test', top=3, metric='mismatch', device='cpu')
        with_seq = S.rank_styles(store, 'test', seg_store=seg, top=3, device='cpu')
    assert sorted(refs['test']['U001']) == ['U001_000_gen', 'U001_001_gen', 'U001_002_gen']
    assert not R.same_refs(refs, R.rank_styles(store, 'test', None, top=3, metric='mismatch'))
    assert not R.same_refs(with_seq, R.rank_styles(store, 'test', seg, top=3))
    assert 2 not in refs['test']['U001']['U001_001_gen']['index']                            # labelled frame 2 carries that target's name


def test_candidates_go_up_in_chunks_under_the_byte_budget(restated_ops, small_store, monkeypatch):
    from seg2eye_amd import style_rank as S
    store, seg = small_store
    monkeypatch.setattr(S, 'UPLOAD_BYTES', 2 * 32 * 20)                                     # two masks at a time
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        refs = S.rank_styles(store, 'train', seg_store=seg, top=4, device='cpu')
    assert not R.same_refs(refs, R.rank_styles(store, 'train', seg, top=4))
    assert restated_ops[:5] == [(3, 2), (3, 2), (3, 1), (3, 2)] + [(2, 2)]                   # U001: 5 generative, 2 sequence; then U002


def test_short_person_warns_once_and_missing_seg_store_says_so(restated_ops, small_store):
    from seg2eye_amd import style_rank as S
    store, seg = small_store
    with pytest.warns(UserWarning, match='fewer than top = 8') as rec:
        S.rank_styles(store, 'train', seg_store=seg, top=8, device='cpu')                   # U001 and U003 have 7 candidates, U002 has 9
    assert len(rec) == 1 and 'U001' in str(rec[0].message) and 'U003' in str(rec[0].message) and 'U002' not in str(rec[0].message)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        S.rank_styles(store, 'train', seg_store=seg, top=5, device='cpu')                   # (5 <= 6 = 7 less the excluded one: nobody is short)
    with pytest.raises(ValueError, match='unlabelled -- pass seg_store'):
        S.rank_styles(store, 'train', top=4, device='cpu')


# ------------------------------------------------------------------------------------------------ the ops before the device check
def test_ops_raise_value_errors_before_the_device_check():
    from seg2eye_amd import _lib, ops
    t, c = torch.zeros(2, 4, 4, dtype=torch.uint8), torch.zeros(3, 4, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match='uint8 label maps'):
        ops.mask_distances(t.int(), c, 4)
    with pytest.raises(ValueError, match='uint8 label maps'):
        ops.mask_distances(t, c.float(), 4)
    with pytest.raises(ValueError, match='one H x W'):
        ops.mask_distances(t, torch.zeros(3, 4, 5, dtype=torch.uint8), 4)
    with pytest.raises(ValueError, match=r'\(n, H, W\) expected'):
        ops.mask_distances(t[0], c, 4)
    with pytest.raises(ValueError, match="'l2' or 'mismatch'"):
        ops.mask_distances(t, c, 4, metric='l1')
    with pytest.raises(ValueError, match='int32'):
        ops.rank_topk(torch.zeros(2, 3), 1)
    with pytest.raises(ValueError, match='k >= 1'):
        ops.rank_topk(torch.zeros(2, 3, dtype=torch.int32), 0)
    with pytest.raises(ValueError, match='exclude'):
        ops.rank_topk(torch.zeros(2, 3, dtype=torch.int32), 1, torch.zeros(3, dtype=torch.int32))
    # valid CPU tensors: the device check is what refuses them
    with pytest.raises(_lib.Seg2EyeHipError, match='GPU only'):
        ops.mask_distances(t, c, 4)
    with pytest.raises(_lib.Seg2EyeHipError, match='GPU only'):
        ops.rank_topk(torch.zeros(2, 3, dtype=torch.int32), 1)
    assert ops.rank.max_candidates() == _lib.lib().s2e_rank_topk_max_candidates() >= 1001


# ------------------------------------------------------------------------------------------------ the file
def test_npz_style_ref_is_read_by_the_dataset(restated_ops, small_store, tmp_path):
    from seg2eye_amd import style_rank as S
    from seg2eye_amd.openeds_dataset import OpenEDSDataset
    from seg2eye_amd.options import parse
    store, seg = small_store
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        refs = S.rank_styles(store, 'train', seg_store=seg, top=4, device='cpu')
    flat = {'%s/%s/%s/%s' % (s, u, f, k): v for s, us in refs.items() for u, fs in us.items() for f, e in fs.items() for k, v in e.items()}
    path = str(tmp_path / 'refs.npz')
    np.savez(path, **flat)                                   # the layout save_refs writes without h5py
    assert not R.same_refs(S.load_refs(path), refs)
    written = S.save_refs(refs, str(tmp_path / 'again'))
    if written.endswith('.npz'):
        assert not R.same_refs(S.load_refs(written), refs)
    o = parse(['--dataset_mode', 'openeds', '--dataset_key', 'train', '--crop_size', '16', '--aspect_ratio', '0.625', '--no_flip',
               '--style_sample_method', 'ref_first', '--style_ref', path])
    ds = OpenEDSDataset(o, store=store)
    _, idx, sub = ds.get_style_images('U002', 4, None, 'U002001_ss')
    e = refs['train']['U002']['U002001_ss']
    assert [bytes(s) for s in sub] == [bytes(s) for s in e['subset'][:4]]
    assert idx == [int(i) - (6 if s == b's' else 0) for i, s in zip(e['index'][:4], e['subset'][:4])]
