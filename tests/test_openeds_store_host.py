"""The OpenEDS stages' shared rules without a GPU: the store's layout helpers (seg2eye_amd/openeds_store.py) against the
literal rules -- the writer of the subset byte against its inverse, the keys of a split, the cleaned file names, the .npz key strings --
and what the two side trainers share (seg2eye_amd/stage.py): the order of the draws from the one RandomState, the history's shape, the
progress lines and the command lines' help texts (tests/golden/stage_help.json, captured before the loop was shared)."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import _refine_ref as RR
import _segment_ref as R
import _style_rank_ref as K

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'stage_help.json')


# ------------------------------------------------------------------------------------------------ the layout
def _frames(n, seed):
    return np.random.RandomState(seed).randint(0, 256, (n, 8, 6)).astype(np.uint8)


def _masks(n, seed):
    return np.random.RandomState(seed).randint(0, 4, (n, 8, 6)).astype(np.uint8)


def _two_persons(dataset_key):
    """-> (store, seg): person A has two first-key frames, person B none; both have three sequence frames and two targets."""
    store, seg = {dataset_key: {}}, {dataset_key: {}}
    for p, (user, n_first) in enumerate((('A', 2), ('B', 0))):
        g = {'images_seq': _frames(3, 10 + p)}
        s = {'labels_pred_seq': _masks(3, 20 + p)}
        if dataset_key == 'test':
            g.update(images_ss=_frames(n_first, 30 + p), labels_ss=_masks(n_first, 40 + p), labels_gen=_masks(2, 50 + p),
                     labels_gen_filenames=np.array([b'%s.t0' % user.encode(), b'%s.t1' % user.encode()], dtype='S13'))
        else:
            g.update(images_gen=_frames(n_first, 30 + p), images_ss=_frames(2, 60 + p), labels_ss=_masks(2, 50 + p),
                     images_ss_filenames=np.array([b'%s.t0' % user.encode(), b'%s.t1' % user.encode()], dtype='S13'))
            s['labels_pred_gen'] = _masks(n_first, 40 + p)
        store[dataset_key][user], seg[dataset_key][user] = g, s
    return store, seg


@pytest.mark.parametrize('use_seq', [True, False], ids=['seq', 'no_seq'])
@pytest.mark.parametrize('dataset_key', ['train', 'test'])
def test_candidate_row_undoes_the_order_rank_styles_concatenates_in(dataset_key, use_seq):
    """The subset array as rank_styles builds it (its own _candidates, the empty parts dropped, concatenated) against candidate_row at
    every position -- and against the two readers: refine.pick_reference and OpenEDSDataset.get_style_images."""
    from seg2eye_amd import openeds_store as O, refine, style_rank
    from seg2eye_amd.openeds_dataset import OpenEDSDataset
    from seg2eye_amd.options import parse
    store, seg = _two_persons(dataset_key)
    first_key = 'images_ss' if dataset_key == 'test' else 'images_gen'
    assert O.candidate_parts(dataset_key, use_seq) == [(b'g', first_key)] + ([(b's', 'images_seq')] if use_seq else [])
    checked = 0
    for user, n_first in (('A', 2), ('B', 0)):
        g = store[dataset_key][user]
        parts = [p for p in style_rank._candidates(store, seg, dataset_key, user, use_seq) if p[1].shape[0] > 0]
        if not parts:
            assert n_first == 0 and not use_seq
            continue
        subset = np.concatenate([np.full(p[1].shape[0], p[0], dtype='S1') for p in parts])
        masks = np.concatenate([np.asarray(p[1]) for p in parts])
        assert len(subset) == n_first + (3 if use_seq else 0)
        for i in range(len(subset)):
            want = (first_key, i) if i < n_first else ('images_seq', i - n_first)
            assert O.candidate_row(g, dataset_key, i, subset[i]) == want, (user, i)
            refs = {dataset_key: {user: {'At0': {'index': np.array([i], dtype=np.int64), 'subset': subset[i:i + 1]}}}}
            image_key, row, holder, mask_key = refine.pick_reference(store, seg, refs, dataset_key, user, 'At0')
            assert (image_key, row) == want and np.array_equal(holder[mask_key][row], masks[i])       # the mask the ranking compared
            checked += 1
        if n_first:                                             # (the dataset reads the first key's count of every person it serves)
            refs = {dataset_key: {user: {'%st0' % user: {'index': np.arange(len(subset), dtype=np.int64), 'subset': subset}}}}
            o = parse(['--dataset_mode', 'openeds', '--dataset_key', dataset_key, '--crop_size', '16', '--aspect_ratio', '0.75', '--no_flip',
                       '--style_sample_method', 'ref_first'])
            ds = OpenEDSDataset(o, store=store, style_refs=refs)
            style, idx, _ = ds.get_style_images(user, len(subset), None, '%st0' % user)
            assert [int(i) for i in idx] == list(range(n_first)) + list(range(len(subset) - n_first))
            assert np.array_equal(style.numpy(), np.concatenate([g[first_key]] + ([g['images_seq']] if use_seq else [])))
    assert checked == (8 if use_seq else 2)
    with pytest.raises(ValueError, match='subset'):
        O.candidate_row(store[dataset_key]['A'], dataset_key, 0, b'x')


def test_a_ranking_without_subsets_means_the_first_image_key():
    from seg2eye_amd.openeds_dataset import OpenEDSDataset
    from seg2eye_amd.options import parse
    store, _ = _two_persons('train')
    refs = {'train': {'A': {'At0': {'index': np.array([1, 0], dtype=np.int64)}}}}
    o = parse(['--dataset_mode', 'openeds', '--dataset_key', 'train', '--crop_size', '16', '--aspect_ratio', '0.75', '--no_flip',
               '--style_sample_method', 'ref_first'])
    style, idx, sub = OpenEDSDataset(o, store=store, style_refs=refs).get_style_images('A', 2, None, 'At0')
    assert sub is None and [int(i) for i in idx] == [1, 0] and np.array_equal(style.numpy(), store['train']['A']['images_gen'][[1, 0]])


def test_split_keys_are_the_three_literal_triples():
    from seg2eye_amd import openeds_store as O, refine
    from seg2eye_amd.openeds_dataset import OpenEDSDataset
    from seg2eye_amd.options import parse
    want = {'train': ('images_gen', 'labels_ss', 'images_ss_filenames'), 'validation': ('images_gen', 'labels_ss', 'images_ss_filenames'),
            'test': ('images_ss', 'labels_gen', 'labels_gen_filenames')}
    store = {**_two_persons('train')[0], **_two_persons('test')[0]}
    store['validation'] = store['train']
    for key, triple in want.items():
        k = O.split_keys(key)
        assert tuple(k) == triple and (k.style_images, k.labels, k.filenames) == triple
        assert refine.label_keys(key) == triple[1:]
        ds = OpenEDSDataset(parse(['--dataset_mode', 'openeds', '--dataset_key', key, '--crop_size', '16', '--aspect_ratio', '0.75']), store=store)
        assert (ds.key_style_images, ds.label_key, ds.key_filenames) == triple and len(ds) == 4
    assert O.pred_name('images_gen') == 'labels_pred_gen' and O.pred_name('images_seq') == 'labels_pred_seq'
    g, s = {'labels_ss': 1}, {'labels_pred_seq': 2}
    assert O.mask_source(g, s, 'test', 'images_ss') == (g, 'labels_ss') and O.mask_source(g, s, 'test', 'images_seq') == (s, 'labels_pred_seq')
    assert O.mask_source(g, s, 'train', 'images_gen') == (s, 'labels_pred_gen') and O.mask_source(g, None, 'validation', 'images_seq') == (None, 'labels_pred_seq')


def test_clean_filename_and_the_datasets_item():
    from seg2eye_amd import openeds_store as O, segment, style_rank
    from seg2eye_amd.openeds_dataset import OpenEDSDataset
    from seg2eye_amd.options import parse
    assert O.clean_filename(b'U1.000_ss') == O.clean_filename(np.bytes_(b'U1.000_ss')) == O.clean_filename('U1.000_ss') == 'U1000_ss'
    assert O.clean_filename(b'a.b.c') == O.clean_filename('a.b.c') == 'abc' and O.clean_filename(b'plain') == 'plain'
    assert style_rank.clean_filename is O.clean_filename and segment.pred_name is O.pred_name
    store, _ = _two_persons('train')
    store['train']['A']['images_ss_filenames'] = np.array([b'A.0.t0', b'A..t1'], dtype='S13')
    store['train']['A']['images_gen'] = _frames(4, 5)
    store['train']['B']['images_gen'] = _frames(4, 6)
    for extra in ([], ['--device_preprocess']):
        o = parse(['--dataset_mode', 'openeds', '--dataset_key', 'train', '--crop_size', '16', '--aspect_ratio', '0.75', '--style_sample_method', 'first'] + extra)
        ds = OpenEDSDataset(o, store=store)
        assert [ds[i]['filename'] for i in range(4)] == ['A0t0', 'At1', 'Bt0', 'Bt1']
        assert all(ds[i]['filename'] == O.clean_filename(store['train']['AABB'[i]]['images_ss_filenames'][i % 2]) for i in range(4))


def test_rows_u8_stacks_rows_of_arrays_and_of_one_row_at_a_time_datasets():
    from seg2eye_amd import openeds_store as O

    class OneRow:                                               # an HDF5 dataset as far as the stages use one: integer indexing only
        def __init__(self, a):
            self.a, self.shape = a, a.shape

        def __getitem__(self, i):
            assert type(i) is int
            return self.a[i]
    a, b = _frames(3, 1).astype(np.int64), _frames(2, 2)
    got = O.rows_u8([(a, np.int64(2)), (OneRow(b), 0), (a, 0)])
    assert got.dtype == np.uint8 and got.shape == (3, 8, 6) and np.array_equal(got, np.stack([a[2], b[0], a[0]]))


# ------------------------------------------------------------------------------------------------ the files
def test_trees_round_trip_through_npz_with_the_literal_keys(tmp_path, monkeypatch):
    from seg2eye_amd import openeds_store as O, prepare_openeds, segment, style_rank
    monkeypatch.setitem(sys.modules, 'h5py', None)               # (import h5py is an ImportError, whether it is installed or not)
    store, _ = _two_persons('train')
    store = {'train': {'A': store['train']['A']}, 'test': {'B': {'images_ss': _frames(1, 3)}}}
    path = prepare_openeds.save_store(store, str(tmp_path / 'store.h5'))
    assert path == str(tmp_path / 'store.h5') + '.npz'
    assert sorted(np.load(path).files) == ['test/B/images_ss', 'train/A/images_gen', 'train/A/images_seq', 'train/A/images_ss',
                                           'train/A/images_ss_filenames', 'train/A/labels_ss']
    for back in (prepare_openeds.load_store(path), O.load_tree(path, 3), O.open_tree(path), style_rank._open(path)):
        assert sorted(back) == ['test', 'train'] and sorted(back['train']) == ['A'] and sorted(back['train']['A']) == sorted(store['train']['A'])
        for k, v in store['train']['A'].items():
            assert back['train']['A'][k].dtype == v.dtype and np.array_equal(back['train']['A'][k], v)
    refs = {'train': {'A': {'At0': {'index': np.array([1, 4], dtype=np.int64), 'subset': np.array([b'g', b's'], dtype='S1'),
                                    'distance': np.array([3, 9], dtype=np.int32)}, 'At1': {'index': np.array([], dtype=np.int64)}}, 'B': {}}}
    path = style_rank.save_refs(refs, str(tmp_path / 'refs'))
    assert path == str(tmp_path / 'refs') + '.npz'
    assert sorted(np.load(path).files) == ['train/A/At0/distance', 'train/A/At0/index', 'train/A/At0/subset', 'train/A/At1/index']
    for back in (style_rank.load_refs(path), O.load_tree(path, 4), O.open_tree(path, 4)):
        assert not K.same_refs(back, {'train': {'A': refs['train']['A']}})
    assert O.save_tree(refs, str(tmp_path / 'again'), 4) == str(tmp_path / 'again') + '.npz'
    with pytest.raises(ValueError):
        O.load_tree(path, 3)                                     # a ranking is no store
    merged = O.merge_splits('%s,,%s' % (path, path), style_rank.load_refs)
    assert sorted(merged) == ['train'] and O.merge_splits(None, style_rank.load_refs) == {} == O.merge_splits('', None)


# ------------------------------------------------------------------------------------------------ the trainers' draws
class _StubAdam:
    def __init__(self, params, lr, betas):
        assert betas == (0.9, 0.999)
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
        grey = torch.tensor(R.GREY / 255.0 * 2 - 1, dtype=torch.float32)
        return -self.k * (x.permute(0, 2, 3, 1) - grey) ** 2


class _RefineNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.k = torch.nn.Parameter(torch.tensor(0.1))

    def forward(self, x):                                       # (n, H, W, C) -> residual (n, H, W, 1)
        return self.k * (x[..., 0:1] - x[..., 1:2])


def _ids(store, keys):
    """{bytes of a frame: (user, key, row)} of a split's listed keys; every frame is its own."""
    ids = {np.asarray(g[k][i]).tobytes(): (u, k, i) for u, g in store.items() for k in keys if k in g for i in range(g[k].shape[0])}
    assert len(ids) == sum(g[k].shape[0] for g in store.values() for k in keys if k in g)
    return ids


@pytest.fixture(scope='module')
def stores():
    store, seg = R.learnable_store(H=64, W=40)
    train, seg = {'train': store['train']}, {'train': seg['train']}                     # (no validation split: the scores are not under test)
    return train, seg, K.rank_styles(train, 'train', seg_store=seg, top=4)


@pytest.fixture()
def recorded(monkeypatch, stores):
    """The ops and the optimiser both trainers look up replaced by CPU stand-ins that record, per step, the batch's sample ids, its flip
    bytes and (for the refiner) the reference frames picked."""
    from seg2eye_amd import optim
    from seg2eye_amd.ops import preprocess, refine, segment
    store = stores[0]['train']
    frames, labels, cands = _ids(store, ['images_ss']), _ids(store, ['labels_ss']), _ids(store, ['images_gen', 'images_seq'])
    events = []

    def bits(flip):
        return None if flip is None else [int(v) for v in flip.tolist()]

    def resize_bicubic_u8(f, Ho, Wo, flip, return_u8=False):
        events.append(('frames', [frames[v.numpy().tobytes()][::2] for v in f], bits(flip)))
        return f[:, ::8, ::5].float() / 127.5 - 1

    def resize_nearest_u8(l, Ho, Wo, flip):
        events.append(('labels', [labels[v.numpy().tobytes()][::2] for v in l], bits(flip)))
        return l[:, ::8, ::5].contiguous()

    def seg_loss(logits, label, weights=None, phi=None, band=None, **lam):
        loss = R.ce_torch(logits, label, weights)
        return loss, torch.stack([loss.detach(), loss.detach() * 0, loss.detach() * 0])

    def refine_input(tmask, rimg, rmask, flip=None, ncls=4, channels=8, dtype=None):
        events.append(('targets', [labels[v.numpy().tobytes()][::2] for v in tmask], bits(flip)))
        events.append(('picks', [cands[v.numpy().tobytes()] for v in rimg]))
        return torch.from_numpy(RR.refine_input(tmask.numpy(), rimg.numpy(), rmask.numpy(), None, ncls=ncls, C=channels))

    def refine_loss(res, rimg, truth, flip=None, lambda_eds=1.0, lambda_l1=0.0):
        events.append(('loss flip', bits(flip)))
        loss, per = RR.loss_torch(res, rimg.numpy(), truth.numpy(), lambda_eds, lambda_l1)
        return loss, torch.stack([per.mean(), per.mean() * 0, 1471 * per.mean()]).detach(), None
    monkeypatch.setattr(preprocess, 'resize_bicubic_u8', resize_bicubic_u8)
    monkeypatch.setattr(preprocess, 'resize_nearest_u8', resize_nearest_u8)
    monkeypatch.setattr(segment, 'seg_cross_entropy', R.ce_torch)
    monkeypatch.setattr(segment, 'seg_dist_maps', lambda label, ncls, radius=2: (None, None))
    monkeypatch.setattr(segment, 'seg_loss', seg_loss)
    monkeypatch.setattr(refine, 'refine_input', refine_input)
    monkeypatch.setattr(refine, 'refine_loss', refine_loss)
    monkeypatch.setattr(optim, 'FlatAdam', _StubAdam)
    return events


@pytest.mark.parametrize('no_flip', [True, False], ids=['no_flip', 'flip'])
def test_segmenter_draws_in_the_stated_order(recorded, stores, no_flip):
    """Per epoch permutation(len(samples)); per batch rand(len(batch)) for the flip, only when flips are on.  18 samples in batches of
    4 (the last of an epoch holds 2), two epochs."""
    from seg2eye_amd import segment
    store = stores[0]
    opt = segment.seg_options(seg_hw=(8, 8), batchSize=4, niter=2, seed=11, no_flip=no_flip)
    _, hist = segment.train_segmenter(store, opt, net=_SegNet(), device='cpu', save=False, verbose=False)
    samples = segment.labelled_samples(store, 'train')
    assert samples == [(u, i) for u in store['train'] for i in range(6)]
    rng, want = np.random.RandomState(11), []
    for _ in range(2):
        order = rng.permutation(18)
        for b0 in range(0, 18, 4):
            batch = [samples[j] for j in order[b0:b0 + 4]]
            flip = [0] * len(batch) if no_flip else (rng.rand(len(batch)) < 0.5).astype(np.uint8).tolist()
            want += [('frames', batch, flip), ('labels', batch, flip)]
    assert recorded == want and len(hist['loss']) == 10
    assert no_flip or any(any(e[2]) for e in recorded)


@pytest.mark.parametrize('no_flip', [True, False], ids=['no_flip', 'flip'])
def test_refiner_draws_in_the_stated_order(recorded, stores, no_flip):
    """Per epoch permutation(len(samples)); per batch one randint(0, min(top, n)) per sample in batch order, then rand(len(batch)) for
    the flip, only when flips are on.  Top 3 of the 4 listed candidates."""
    from seg2eye_amd import refine
    store, seg, refs = stores
    opt = refine.refine_options(batchSize=4, niter=2, seed=13, no_flip=no_flip, refine_top=3, compute_dtype='fp32')
    _, hist = refine.train_refiner(store, seg, refs, opt, net=_RefineNet(), device='cpu', save=False, verbose=False)
    samples = refine.targets(store, 'train')
    assert samples == RR.target_list(store, 'train') and len(samples) == 18
    rng, want = np.random.RandomState(13), []
    for _ in range(2):
        order = rng.permutation(18)
        for b0 in range(0, 18, 4):
            batch = [samples[j] for j in order[b0:b0 + 4]]
            picks = []
            for u, _, f in batch:
                e = refs['train'][u][f]
                assert len(e['index']) == 4
                pos = int(rng.randint(0, 3))
                idx = int(e['index'][pos])
                picks.append((u, 'images_gen', idx) if bytes(e['subset'][pos]) == b'g' else (u, 'images_seq', idx - 4))
            flip = None if no_flip else (rng.rand(len(batch)) < 0.5).astype(np.uint8).tolist()
            want += [('targets', [(u, i) for u, i, _ in batch], flip), ('picks', picks), ('loss flip', flip)]
    assert recorded == want and len(hist['loss']) == len(hist['terms']) == 10
    assert len({p for e in recorded if e[0] == 'picks' for p in e[1]}) > 10 and {p[1] for e in recorded if e[0] == 'picks' for p in e[1]} == {'images_gen', 'images_seq'}


# ------------------------------------------------------------------------------------------------ history and progress lines
SEG_LINE = r'epoch 2 step 4 loss \d+\.\d{4}'
SEG_TERMS = r' CE \d+\.\d{4} Dice \d+\.\d{4} Surface -?\d+\.\d{4}'
REFINE_LINE = r'epoch 2 step 4 loss \d+\.\d{5} eds \d+\.\d{5} l1 \d+\.\d{5} score \d+\.\d{3}'


@pytest.mark.parametrize('print_freq', [100, 4])
@pytest.mark.parametrize('stage', ['segment', 'segment_terms', 'refine'])
def test_history_is_whole_and_one_line_is_printed_per_print_freq_steps(recorded, stores, capsys, monkeypatch, stage, print_freq):
    """Six steps (18 samples, batches of 6, two epochs).  print_freq 100: no line, the flush at the end fills the history.  print_freq
    4: one line, after step 4, and the two steps behind it come with the flush.  One device-to-host copy of the losses (and one of the
    terms) per flush, none in between."""
    from seg2eye_amd import refine, segment
    store, seg, refs = stores
    copies = []
    stack = torch.stack
    monkeypatch.setattr(torch, 'stack', lambda tensors, *a, **k: (copies.append(len(tensors)), stack(tensors, *a, **k))[1])
    if stage == 'refine':
        opt = refine.refine_options(batchSize=6, niter=2, seed=2, print_freq=print_freq, refine_top=2, compute_dtype='fp32')
        _, hist = refine.train_refiner(store, seg, refs, opt, net=_RefineNet(), device='cpu', save=False, verbose=True)
        pattern, keys = REFINE_LINE, ['loss', 'scores', 'terms']
    else:
        extra = dict(lambda_dice=1.0) if stage == 'segment_terms' else {}
        opt = segment.seg_options(seg_hw=(8, 8), batchSize=6, niter=2, seed=2, print_freq=print_freq, **extra)
        _, hist = segment.train_segmenter(store, opt, net=_SegNet(), device='cpu', save=False, verbose=True)
        pattern, keys = SEG_LINE + (SEG_TERMS if extra else ''), ['loss', 'scores', 'terms'] if extra else ['loss', 'scores']
    monkeypatch.undo()
    assert sorted(hist) == keys and len(hist['loss']) == 6 and hist['scores'] == [] and np.isfinite(hist['loss']).all()
    assert all(type(v) is float for v in hist['loss'])
    if 'terms' in keys:
        assert len(hist['terms']) == 6 and all(len(t) == 3 for t in hist['terms'])
        assert [t[0] for t in hist['terms']] == pytest.approx(hist['loss'], rel=1e-6)
    lines = [s for s in capsys.readouterr().out.splitlines() if s.startswith('epoch')]
    flushes = [6] if print_freq == 100 else [4, 2]
    assert [n for n in copies if n in (2, 4, 6)] == [n for n in flushes for _ in range(2 if 'terms' in keys else 1)]
    if print_freq == 100:
        assert lines == []
    else:
        assert len(lines) == 1 and re.fullmatch(pattern, lines[0]), lines
        mean = float(np.mean(hist['loss'][:4]))
        assert abs(float(lines[0].split()[5]) - mean) <= 1e-4


# ------------------------------------------------------------------------------------------------ the command lines
def _helps(module, monkeypatch):
    monkeypatch.setenv('COLUMNS', '100')
    ap = module.parser()
    sub = [a for a in ap._actions if hasattr(a, 'choices') and isinstance(a.choices, dict)][0]
    return {'': ap.format_help(), **{name: p.format_help() for name, p in sub.choices.items()}}


def test_help_texts_are_the_recorded_ones(monkeypatch):
    from seg2eye_amd import refine, segment
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == ['refine', 'segment']
    for name, module in (('segment', segment), ('refine', refine)):
        got = _helps(module, monkeypatch)
        assert sorted(got) == ['', 'eval', 'predict', 'train'] == sorted(golden[name])
        for command, text in got.items():
            assert text == golden[name][command], (name, command)
