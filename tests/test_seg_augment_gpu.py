"""The segmenter's paired augmentation on the GPU: `ops.augment_pairs` against the numpy restatement
(tests/_seg_augment_ref.py) at every shape, matrix, line count, subset of the outputs and alignment; the identity against the two resize
ops; a training run whose first batch is the restatement's; the two commands.  Every comparison is == on bytes or float bit patterns."""
import functools
import itertools
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

import _seg_augment_ref as R
import _segment_ref as SR

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 65536
SHAPES = [(1, 1, 1), (1, 1, 67), (1, 67, 1), (2, 5, 7), (3, 66, 35), (2, 64, 68), (2, 320, 200), (1, 640, 400)]
MATRICES = ['identity', 'mirror', 'integer_shift', 'subpixel_shift', 'rule', 'extreme']
STRONG = dict(rotate=180.0, scale=4.0, translate=1.0, gamma=3.0, contrast=0.9, brightness=0.5)
# (frames given, labels given, want_f32, want_u8): every non-empty subset of the three outputs, and the frames given but not wanted
SUBSETS = [(True, True, True, True), (True, True, True, False), (True, True, False, True), (True, True, False, False), (False, True, False, False),
           (True, False, True, True), (True, False, True, False), (True, False, False, True)]
I32 = (-2 ** 31, 2 ** 31 - 1)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _affine(kind, shape, seed):
    n, h, w = shape
    rng = np.random.RandomState(seed)
    if kind == 'identity':
        A = [[Q, 0, 0, 0, Q, 0]] * n
    elif kind == 'mirror':
        A = [[-Q, 0, (w - 1) << 16, 0, Q, 0], [-Q, 0, (w - 1) << 16, 0, -Q, (h - 1) << 16], [Q, 0, 0, 0, -Q, (h - 1) << 16]][:n]
    elif kind == 'integer_shift':
        A = [[Q, 0, int(rng.randint(-w, w + 1)) * Q, 0, Q, int(rng.randint(-h, h + 1)) * Q] for _ in range(n)]
    elif kind == 'subpixel_shift':
        A = [[Q, 0, 0x8000, 0, Q, 0], [Q, 0, 0x1234, 0, Q, -0x4321], [Q, 0, int(rng.randint(-3 * Q, 3 * Q)), 0, Q, int(rng.randint(-3 * Q, 3 * Q))]][:n]
    elif kind == 'rule':
        return R.draw(rng, n, h, w, **STRONG).affine
    else:                                                      # every coefficient one of int32's two ends, or near zero
        A = [[int(rng.choice(I32 + (0, 1, -1))) for _ in range(6)] for _ in range(n)]
        A[0] = [I32[1]] * 6
    return np.array(A, dtype=np.int32)


def _lines(shape, L, seed):
    """L lines per frame: end points in and around the plane, widths 0..4, any value; the last line of frame 0 int32's ends."""
    if not L:
        return None
    n, h, w = shape
    rng = np.random.RandomState(seed)
    lines = np.stack([rng.randint(-w, 2 * w + 1, (n, L)), rng.randint(-h, 2 * h + 1, (n, L)), rng.randint(-w, 2 * w + 1, (n, L)), rng.randint(-h, 2 * h + 1, (n, L)),
                      rng.randint(0, 5, (n, L)), rng.randint(-1000, 1000, (n, L))], axis=-1).astype(np.int32)
    lines[0, -1] = (I32[0], I32[1], I32[1], I32[0], I32[1] if L > 1 else 1, I32[0] + 77)
    return lines


@functools.lru_cache(maxsize=None)
def _case(shape, kind, L):
    """-> (frames, labels, params, the restatement's three outputs); computed once, shared by every subset and alignment."""
    seed = sum(shape) * 7 + MATRICES.index(kind) * 3 + L
    img, lab = R.planes(shape, seed)
    tables = R.draw(np.random.RandomState(seed + 1), shape[0], shape[1], shape[2], gamma=3.0, contrast=0.9, brightness=0.5)
    p = R.Params(_affine(kind, shape, seed + 2), _lines(shape, L, seed + 3), tables.lut_f32, tables.lut_u8)
    return img, lab, p, R.augment_pairs(img, lab, p)


def _check(got, want, given):
    has_img, has_lab, f32, u8 = given
    xf, xb, y = got
    assert (xf is None) == (not (has_img and f32)) and (xb is None) == (not (has_img and u8)) and (y is None) == (not has_lab)
    if xf is not None:
        assert xf.dtype == torch.float32 and np.array_equal(_bits(xf.cpu().numpy()), _bits(want[0]))
    if xb is not None:
        assert xb.dtype == torch.uint8 and np.array_equal(xb.cpu().numpy(), want[1])
    if y is not None:
        assert y.dtype == torch.uint8 and np.array_equal(y.cpu().numpy(), want[2])


def _off_by_one(a, dev, lead=1):
    """A device copy of `a` that starts `lead` elements into its buffer."""
    buf = torch.zeros(a.size + lead, dtype=torch.float32 if a.dtype == np.float32 else torch.uint8, device=dev)
    view = buf[lead:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return view


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_op_is_the_restatement(shape):
    from seg2eye_amd import _lib as L
    from seg2eye_amd.ops import augment as A
    from seg2eye_amd.ops.core import _p, _stream
    n, h, w = shape
    for kind, nl in itertools.product(MATRICES, (0, 1, 8)):
        img, lab, p, want = _case(shape, kind, nl)
        img_d, lab_d = torch.from_numpy(img).to(DEV), torch.from_numpy(lab).to(DEV)
        params = A.AugmentParams(*p)
        for given in SUBSETS:
            got = A.augment_pairs(img_d if given[0] else None, lab_d if given[1] else None, params, want_f32=given[2], want_u8=given[3])
            _check(got, want, given)
        again = A.augment_pairs(img_d, lab_d, params, want_f32=True, want_u8=True)
        _check(again, want, SUBSETS[0])
        assert np.array_equal(img_d.cpu().numpy(), img) and np.array_equal(lab_d.cpu().numpy(), lab)        # the inputs are as they were
        # planes one byte off their alignment (fp32: one element off 16 bytes), inputs and outputs, through the C ABI
        img_o, lab_o = _off_by_one(img, DEV), _off_by_one(lab, DEV)
        xf, xb, y = _off_by_one(np.zeros(shape, np.float32), DEV), _off_by_one(np.zeros(shape, np.uint8), DEV), _off_by_one(np.zeros(shape, np.uint8), DEV, 3)
        assert img_o.data_ptr() % 4 == 1 and xb.data_ptr() % 4 == 1 and y.data_ptr() % 4 == 3 and xf.data_ptr() % 16 == 4
        aff, lut_f, lut_b = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (p.affine, p.lut_f32, p.lut_u8))
        lines = None if p.lines is None else torch.from_numpy(p.lines).to(DEV)
        L.call.s2e_augment_pairs(_p(img_o), _p(lab_o), n, h, w, _p(aff), _p(lines), nl, _p(lut_f), _p(lut_b), _p(xf), _p(xb), _p(y), _stream())
        _check((xf, xb, y), want, SUBSETS[0])


def test_rule_draws_reach_the_kernel_as_drawn():
    """The op's own AugmentRule at full strength, lines and tables included, at the training size."""
    from seg2eye_amd.ops import augment as A
    shape = (4, 320, 200)
    img, lab = R.planes(shape, 77)
    kw = dict(lines=8, **STRONG)
    params = A.AugmentRule(**kw).draw(np.random.RandomState(5), 4, 320, 200)
    want = R.augment_pairs(img, lab, R.draw(np.random.RandomState(5), 4, 320, 200, **kw))
    _check(A.augment_pairs(torch.from_numpy(img).to(DEV), torch.from_numpy(lab).to(DEV), params, want_u8=True), want, SUBSETS[0])
    assert (want[2] != lab).mean() > 0.3 and (want[1] != img).mean() > 0.5


# ------------------------------------------------------------------------------------------------ the unaugmented path
def test_identity_parameters_give_the_resize_ops_outputs():
    """From raw 640 x 400 frames: augment_pairs of the resized bytes with identity parameters is resize_bicubic_u8's fp32 output, bit for
    bit, and resize_nearest_u8's labels -- frames flipped and not."""
    from seg2eye_amd.ops import augment as A, preprocess as P
    lab = SR.eyes(4, 640, 400, 4, 8)
    img = SR.eye_frames(lab, 'aug_identity', 8)
    flip = torch.tensor([0, 1, 1, 0], dtype=torch.uint8, device=DEV)
    for hw in ((320, 200), (64, 40)):
        x, x_u8 = P.resize_bicubic_u8(torch.from_numpy(img).to(DEV), hw[0], hw[1], flip, return_u8=True)
        y = P.resize_nearest_u8(torch.from_numpy(lab).to(DEV), hw[0], hw[1], flip)
        for params in (A.identity_params(4), A.identity_params(4, lines=8), A.AugmentRule().draw(np.random.RandomState(0), 4, *hw),
                       A.AugmentRule(prob=0.0, lines=3, **STRONG).draw(np.random.RandomState(0), 4, *hw)):
            ax, ab, ay = A.augment_pairs(x_u8, y, params, want_u8=True)
            assert np.array_equal(_bits(ax.cpu().numpy()), _bits(x.cpu().numpy())) and torch.equal(ab, x_u8) and torch.equal(ay, y)
    assert not torch.equal(x_u8[1], torch.flip(x_u8[1], (1,)))


# ------------------------------------------------------------------------------------------------ end to end
E2E = dict(nsf=8, seg_hw=(64, 40), compute_dtype='fp32', batchSize=6, niter=2, lr=2e-3, seed=7)
RULE = dict(prob=0.9, rotate=25.0, scale=1.4, translate=0.15, gamma=2.0, contrast=0.5, brightness=0.2, lines=4)


@functools.lru_cache(maxsize=None)
def _store():
    return SR.learnable_store(128, 80)[0]


def _resized(store, key, batch, hw, flip):
    """The restated resize of a batch of labelled samples -> (frames u8, labels u8) at hw, flipped where flip says so."""
    from seg2eye_amd.ops.preprocess import resize_bicubic_u8_reference
    frames = np.stack([resize_bicubic_u8_reference(store[key][u]['images_ss'][i], hw[1], hw[0]) for u, i in batch])
    labels = SR.host_labels(np.stack([store[key][u]['labels_ss'][i] for u, i in batch]), hw)
    for j, f in enumerate(flip):
        if f:
            frames[j], labels[j] = frames[j, :, ::-1], labels[j, :, ::-1]
    return frames, labels


def test_training_run_feeds_the_network_the_restated_batch(monkeypatch):
    from seg2eye_amd import segment
    from seg2eye_amd.ops import augment as A, segment as S
    store = _store()
    opt = segment.seg_options(**E2E)
    net = segment.build_network(opt, DEV)
    seen = {}
    def first_input(module, args):                              # (a pre-hook's result, unless None, replaces the input)
        seen.setdefault('x', args[0].detach().cpu().numpy().copy())
    handle = net.register_forward_pre_hook(first_input)
    ce = S.seg_cross_entropy
    monkeypatch.setattr(S, 'seg_cross_entropy', lambda logits, y, w=None: (seen.setdefault('y', y.cpu().numpy().copy()), ce(logits, y, w))[1])
    _, hist = segment.train_segmenter(store, opt, net=net, device=DEV, save=False, verbose=False, augment=A.AugmentRule(**RULE))
    handle.remove()
    assert len(hist['loss']) == 6 and np.isfinite(hist['loss']).all() and hist['scores'] and len(hist['scores']) == 2
    samples = segment.labelled_samples(store, 'train')
    rng = np.random.RandomState(7)
    batch = [samples[j] for j in rng.permutation(18)[:6]]
    flip = rng.rand(6) < 0.5
    frames, labels = _resized(store, 'train', batch, (64, 40), flip)
    want_x, _, want_y = R.augment_pairs(frames, labels, R.draw(rng, 6, 64, 40, **RULE))
    assert seen['x'].shape == (6, 1, 64, 40) and np.array_equal(_bits(seen['x'][:, 0]), _bits(want_x)) and np.array_equal(seen['y'], want_y)
    assert (want_y != labels).any() and flip.any()


def test_train_command_writes_a_checkpoint_segment_eval_reads(tmp_path, capsys):
    from seg2eye_amd import segment
    from seg2eye_amd.prepare_openeds import save_store
    path = save_store(_store(), str(tmp_path / 'store.h5'))
    common = ['--dataroot', path, '--checkpoints_dir', str(tmp_path), '--name', 'aug', '--nsf', '8', '--seg_hw', '64,40', '--compute_dtype', 'fp32', '--batchSize', '6']
    r = subprocess.run([sys.executable, '-m', 'seg2eye_amd.seg_augment', 'train'] + common
                       + ['--niter', '1', '--print_freq', '1', '--aug_rotate', '25', '--aug_scale', '1.4', '--aug_translate', '0.15', '--aug_gamma', '2', '--aug_contrast', '0.5',
                          '--aug_brightness', '0.2', '--aug_lines', '4', '--aug_prob', '0.9'], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.count('epoch 1 step') == 3 and 'miou/validation' in r.stdout
    assert (tmp_path / 'aug' / 'latest_net_S.pth').exists() and (tmp_path / 'aug' / '1_net_S.pth').exists()
    capsys.readouterr()
    scores = segment.main(['eval'] + common)
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert line.startswith('miou/validation ') and 0.0 <= scores['miou/validation'] <= 1.0 and line == r.stdout.strip().splitlines()[-1]


def _png(path):
    """The 8-bit greyscale PNG visualizer.write_png writes -> a uint8 array."""
    data = open(path, 'rb').read()
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    at, chunks = 8, {}
    while at < len(data):
        size, tag = struct.unpack('>I4s', data[at:at + 8])
        chunks[tag] = data[at + 8:at + 8 + size]
        at += 12 + size
    cols, rows, depth, colour = struct.unpack('>IIBB', chunks[b'IHDR'][:10])
    assert (depth, colour) == (8, 0)
    raw = np.frombuffer(zlib.decompress(chunks[b'IDAT']), dtype=np.uint8).reshape(rows, cols + 1)
    assert not raw[:, 0].any()
    return raw[:, 1:]


def test_show_command_writes_the_restated_panels(tmp_path, capsys):
    from seg2eye_amd import seg_augment, segment
    from seg2eye_amd.prepare_openeds import save_store
    store = _store()
    path = save_store(store, str(tmp_path / 'store.h5'))
    out = tmp_path / 'preview'
    paths = seg_augment.main(['show', '--dataroot', path, '--out', str(out), '--n', '5', '--seed', '3', '--seg_hw', '64,40', '--aug_rotate', '25', '--aug_scale', '1.4',
                              '--aug_translate', '0.15', '--aug_gamma', '2', '--aug_contrast', '0.5', '--aug_brightness', '0.2', '--aug_lines', '4'])
    assert '5 panels written to' in capsys.readouterr().out
    batch = segment.labelled_samples(store, 'train')[:5]
    assert [os.path.basename(p) for p in paths] == ['%s_%03d.png' % s for s in batch] == sorted(os.listdir(out))
    frames, labels = _resized(store, 'train', batch, (64, 40), [0] * 5)
    p = R.draw(np.random.RandomState(3), 5, 64, 40, **dict(RULE, prob=1.0))
    _, ax, ay = R.augment_pairs(frames, labels, p)
    for i, path in enumerate(paths):
        panel = _png(path)
        assert panel.shape == (64, 160)
        for k, want in enumerate((frames[i], R.label_grey(labels[i]), ax[i], R.label_grey(ay[i]))):
            assert np.array_equal(panel[:, 40 * k:40 * k + 40], want), (i, k)
    assert (ax != frames).any() and (ay != labels).any()
