"""The eye segmenter without a GPU: the restatement (tests/_segment_ref.py) against stock torch, the scores read from a
confusion matrix, the refused calls of the four entry points, the ops' ValueErrors, and the mask writer's walk with a stub network and
the restatement in the ops' place -- up to the ranking `style_rank` makes of its result."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _segment_ref as R
import _style_rank_ref as SR
from _quality_harness import check_error_table

F32, BF16, BAD = 0, 1, 7
P = 4096                                                      # a dummy non-null pointer: must never reach a kernel
BIG = 1 << 24                                                 # a workspace size that is never short
ARG, UNSUPPORTED = -1, -3


# ------------------------------------------------------------------------------------------------ the restatement alone
@pytest.mark.parametrize('weights', [None, [0.5, 1.0, 2.0, 4.0], [1.0, 0.0, 1.0, 1.0]])
def test_restated_cross_entropy_is_torchs(weights):
    g = torch.Generator().manual_seed(1)
    z = torch.randn(2, 5, 7, 4, generator=g, dtype=torch.float64).requires_grad_(True)
    lab = torch.randint(0, 4, (2, 5, 7), generator=g, dtype=torch.uint8)
    lab[0, 0, :3] = 255
    lab[1, 2, 4] = 9
    w = torch.ones(4, dtype=torch.float64) if weights is None else torch.tensor(weights, dtype=torch.float64)
    want = F.cross_entropy(z.permute(0, 3, 1, 2), torch.where(lab < 4, lab.long(), torch.full_like(lab.long(), 255)), weight=w,
                           ignore_index=255, reduction='mean')
    dwant, = torch.autograd.grad(want, z)
    loss, grad = R.ce(z.detach().numpy(), lab.numpy(), w.numpy(), 4)
    assert abs(loss - float(want.detach())) < 1e-14 and np.abs(grad - dwant.numpy()).max() < 1e-15
    assert (grad[0, 0, :3] == 0).all() and (grad[1, 2, 4] == 0).all()
    assert abs(float(R.ce_torch(z.detach(), lab, w)) - float(want.detach())) == 0


def test_restated_cross_entropy_pad_channels_and_no_counted_pixel():
    z = np.random.RandomState(2).randn(1, 3, 4, 8)
    z[..., 4:] = np.nan
    lab = np.random.RandomState(3).randint(0, 4, (1, 3, 4)).astype(np.uint8)
    loss, grad = R.ce(z, lab, np.ones(4), 4)
    want, dwant = R.ce(z[..., :4], lab, np.ones(4), 4)
    assert loss == want and np.array_equal(grad[..., :4], dwant) and (grad[..., 4:] == 0).all()
    loss, grad = R.ce(z, np.full((1, 3, 4), 255, np.uint8), np.ones(4), 4)
    assert loss == 0 and (grad == 0).all()
    l32, g32 = R.ce(z, lab, np.ones(4), 4, np.float32)
    assert l32.dtype == np.float32 and g32.dtype == np.float32 and abs(float(l32) - want) < 1e-6


@pytest.mark.parametrize('shape,out', [((2, 7, 5, 4), (13, 11)), ((1, 8, 8, 3), (16, 16)), ((1, 6, 9, 4), (6, 9)), ((1, 9, 6, 4), (4, 5))])
def test_restated_argmax_is_interpolate_then_argmax(shape, out):
    z = torch.randn(*shape, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    up = F.interpolate(z.permute(0, 3, 1, 2), size=out, mode='bilinear', align_corners=False)
    mask, gap = R.argmax_resized(z.numpy(), out[0], out[1], shape[3])
    assert np.abs(R.resized(z.numpy(), out[0], out[1], shape[3]) - up.permute(0, 2, 3, 1).numpy()).max() < 1e-12
    clear = gap > 1e-9
    assert clear.mean() > 0.99 and np.array_equal(mask[clear], up.argmax(1).numpy().astype(np.uint8)[clear])


def test_restated_argmax_ties_go_to_the_lower_class():
    z = np.zeros((1, 2, 2, 4))
    z[0, 0, 0] = [1, 3, 3, 0]
    z[0, 1, 1] = [2, 2, 2, 2]
    mask, gap = R.argmax_resized(z, 2, 2, 4)
    assert mask[0, 0, 0] == 1 and mask[0, 1, 1] == 0 and gap[0, 0, 0] == 0
    assert R.argmax_resized(z, 2, 2, 1)[0].max() == 0


def test_restated_confusion_is_a_bincount():
    rng = np.random.RandomState(5)
    p, t = rng.randint(0, 6, 391).astype(np.uint8), rng.randint(0, 6, 391).astype(np.uint8)
    c = R.confusion(p, t, 4)
    for i in range(4):
        for j in range(4):
            assert c[i, j] == int(((t == i) & (p == j)).sum())
    assert c.sum() == int(((t < 4) & (p < 4)).sum()) and c.dtype == np.int64


# ------------------------------------------------------------------------------------------------ scores
def test_segment_scores_by_hand():
    from seg2eye_amd.ops import segment_scores
    perfect = np.diag([10, 0, 5, 7])                                       # class 1 is in neither mask: left out of the mean
    s = segment_scores(perfect)
    assert s['miou'] == 1.0 and s['acc'] == 1.0 and np.isnan(s['iou'][1]) and list(s['iou'][[0, 2, 3]]) == [1.0, 1.0, 1.0]
    c = np.array([[6, 2, 0], [1, 3, 0], [0, 0, 0]])                         # IoU 6 / 9, 3 / 6; class 2 absent
    s = segment_scores(torch.from_numpy(c))
    assert abs(s['iou'][0] - 6 / 9) < 1e-15 and abs(s['iou'][1] - 0.5) < 1e-15 and np.isnan(s['iou'][2])
    assert abs(s['miou'] - (6 / 9 + 0.5) / 2) < 1e-15 and abs(s['acc'] - 9 / 12) < 1e-15
    c = np.array([[0, 4], [0, 0]])                                          # everything wrong: both classes seen, both 0
    assert segment_scores(c) == {'iou': pytest.approx([0.0, 0.0]), 'miou': 0.0, 'acc': 0.0}
    assert segment_scores(np.zeros((4, 4), np.int64))['miou'] == 0.0
    assert abs(segment_scores(c + 3)['miou'] - R.scores(c + 3)['miou']) < 1e-15
    with pytest.raises(ValueError, match='square'):
        segment_scores(np.zeros((3, 4)))


# ------------------------------------------------------------------------------------------------ refused calls
def _ce_fwd(dtype=F32, x=P, label=P, w=P, N=2, H=8, W=8, C=4, ncls=4, loss=P, denom=P, ws=P, wsb=BIG):
    return (dtype, x, label, w, N, H, W, C, ncls, loss, denom, ws, wsb, None)


def _ce_bwd(dtype=F32, x=P, label=P, w=P, denom=P, g=P, N=2, H=8, W=8, C=4, ncls=4, dx=P):
    return (dtype, x, label, w, denom, g, N, H, W, C, ncls, dx, None)


def _argmax(dtype=BF16, x=P, N=2, h=8, w=8, C=4, ncls=4, Ho=16, Wo=16, mask=P):
    return (dtype, x, N, h, w, C, ncls, Ho, Wo, mask, None)


def _conf(pred=P, truth=P, n=100, ncls=4, conf=P):
    return (pred, truth, n, ncls, conf, None)


def _shared(name, make):
    """The rows every logits entry refuses alike, in the order the header states them."""
    return [
        (make(x=None), ARG, name + ': bad argument'),
        (make(dtype=BAD, N=0), ARG, name + ': bad dtype 7'),                                  # the dtype before the sizes
        (make(N=0, ncls=17), ARG, name + ': N=0 H=8 W=8 (every size must be at least 1)'),    # the sizes before the class count
        (make(H=0), ARG, name + ': N=2 H=0 W=8 (every size must be at least 1)'),
        (make(W=-1), ARG, name + ': N=2 H=8 W=-1 (every size must be at least 1)'),
        (make(ncls=0), UNSUPPORTED, name + ': ncls=0 (1 to 16 classes)'),
        (make(ncls=17, C=16), UNSUPPORTED, name + ': ncls=17 (1 to 16 classes)'),             # the class count before the pitch
        (make(C=3), ARG, name + ': channel pitch C=3 is below ncls=4'),
        (make(N=65536, H=32768, W=1, C=3), ARG, name + ': channel pitch C=3 is below ncls=4'),  # the pitch before the index limit
        (make(N=32768, H=65536, W=1), UNSUPPORTED, name + ': N=32768 H=65536 W=1 is beyond the index limit (N H W <= 2^31 - 1)'),
    ]


FWD = _shared('s2e_seg_ce_fwd', lambda **k: _ce_fwd(**k)) + [
    (_ce_fwd(label=None), ARG, 's2e_seg_ce_fwd: bad argument'),
    (_ce_fwd(w=None), ARG, 's2e_seg_ce_fwd: bad argument'),
    (_ce_fwd(loss=None), ARG, 's2e_seg_ce_fwd: bad argument'),
    (_ce_fwd(denom=None), ARG, 's2e_seg_ce_fwd: bad argument'),
    (_ce_fwd(ws=None), ARG, 's2e_seg_ce_fwd: workspace of 0 bytes, needs 16 (8-byte aligned)'),
    (_ce_fwd(wsb=15), ARG, 's2e_seg_ce_fwd: workspace of 15 bytes, needs 16 (8-byte aligned)'),
    (_ce_fwd(ws=P + 4), ARG, 's2e_seg_ce_fwd: workspace of %d bytes, needs 16 (8-byte aligned)' % BIG),
    (_ce_fwd(N=4, H=320, W=200, wsb=8191), ARG, 's2e_seg_ce_fwd: workspace of 8191 bytes, needs 8192 (8-byte aligned)'),
    (_ce_fwd(ncls=17, ws=None), UNSUPPORTED, 's2e_seg_ce_fwd: ncls=17 (1 to 16 classes)'),   # the workspace last
]
BWD = _shared('s2e_seg_ce_bwd', lambda **k: _ce_bwd(**k)) + [
    (_ce_bwd(**{k: None}), ARG, 's2e_seg_ce_bwd: bad argument') for k in ('label', 'w', 'denom', 'g', 'dx')]


def _argmax_in(**k):
    k = {{'H': 'h', 'W': 'w'}.get(n, n): v for n, v in k.items()}
    return _argmax(**k)


ARGMAX = _shared('s2e_seg_argmax_u8', _argmax_in) + [
    (_argmax(mask=None), ARG, 's2e_seg_argmax_u8: bad argument'),
    (_argmax(Ho=0), ARG, 's2e_seg_argmax_u8: Ho=0 Wo=16 (every size must be at least 1)'),
    (_argmax(Wo=-2), ARG, 's2e_seg_argmax_u8: Ho=16 Wo=-2 (every size must be at least 1)'),
    (_argmax(C=3, Ho=0), ARG, 's2e_seg_argmax_u8: channel pitch C=3 is below ncls=4'),       # the input's checks before the output's
    (_argmax(Ho=65536), UNSUPPORTED,
     's2e_seg_argmax_u8: N=2 Ho=65536 Wo=16 is beyond the launch limits (N, Ho <= 65535, N Ho Wo <= 2^31 - 1)'),
    (_argmax(N=65536, h=1, w=1, Ho=1, Wo=1), UNSUPPORTED,
     's2e_seg_argmax_u8: N=65536 Ho=1 Wo=1 is beyond the launch limits (N, Ho <= 65535, N Ho Wo <= 2^31 - 1)'),
    (_argmax(N=4, Ho=32768, Wo=32768), UNSUPPORTED,
     's2e_seg_argmax_u8: N=4 Ho=32768 Wo=32768 is beyond the launch limits (N, Ho <= 65535, N Ho Wo <= 2^31 - 1)'),
]
CONF = [
    (_conf(pred=None), ARG, 's2e_seg_confusion_u8: bad argument'),
    (_conf(truth=None), ARG, 's2e_seg_confusion_u8: bad argument'),
    (_conf(conf=None), ARG, 's2e_seg_confusion_u8: bad argument'),
    (_conf(conf=P + 4), ARG, 's2e_seg_confusion_u8: bad argument'),
    (_conf(n=0, ncls=0), ARG, 's2e_seg_confusion_u8: P=0 (at least one pixel)'),             # the size before the class count
    (_conf(n=-5), ARG, 's2e_seg_confusion_u8: P=-5 (at least one pixel)'),
    (_conf(ncls=0), UNSUPPORTED, 's2e_seg_confusion_u8: ncls=0 (1 to 16 classes)'),
    (_conf(ncls=17, n=1 << 31), UNSUPPORTED, 's2e_seg_confusion_u8: ncls=17 (1 to 16 classes)'),
    (_conf(n=1 << 31), UNSUPPORTED, 's2e_seg_confusion_u8: P=2147483648 is beyond the index limit (P <= 2^31 - 1 per call)'),
]


def test_segment_entry_points_reject_bad_calls_before_any_launch():
    """Null pointers, a size below 1, C < ncls, an unknown dtype, a missing or short workspace: S2E_ERR_ARG; ncls outside 1..16 and a
    pixel count beyond 2^31 - 1: S2E_ERR_UNSUPPORTED; the message, and which check wins.  Host-only: with a GPU visible the test skips
    itself, so that a dummy pointer can never reach a kernel (as test_region_entry_points_reject_bad_calls_before_any_launch does)."""
    if torch.cuda.is_available():
        pytest.skip('dummy pointers: host-only by construction')
    from seg2eye_amd import _lib
    assert (_lib.S2E_BF16, _lib.S2E_F32) == (BF16, F32)
    for name, table in (('s2e_seg_ce_fwd', FWD), ('s2e_seg_ce_bwd', BWD), ('s2e_seg_argmax_u8', ARGMAX), ('s2e_seg_confusion_u8', CONF)):
        check_error_table(name, table)
    with pytest.raises(_lib.Seg2EyeHipError, match='s2e_seg_ce_fwd failed'):
        _lib.call.s2e_seg_ce_fwd(*FWD[0][0])


def test_workspace_bytes_follows_the_pixel_count():
    """One {numerator, denominator} fp64 pair per workgroup of 256 pixels, at most 512 workgroups; 0 where there is nothing to reduce."""
    from seg2eye_amd import _lib
    q = _lib.lib().s2e_seg_ce_workspace_bytes
    assert [q(1, 1, 1), q(1, 16, 16), q(1, 16, 17), q(4, 320, 200), q(16, 320, 200)] == [16, 16, 32, 8192, 8192]
    assert [q(0, 8, 8), q(2, -1, 8), q(32768, 65536, 1)] == [0, 0, 0]


# ------------------------------------------------------------------------------------------------ the ops before the device check
def test_ops_raise_value_errors_before_the_device_check():
    from seg2eye_amd import _lib, ops
    z, lab = torch.zeros(2, 4, 6, 4), torch.zeros(2, 4, 6, dtype=torch.uint8)
    with pytest.raises(ValueError, match='bf16 or fp32 logits'):
        ops.seg_cross_entropy(z.double(), lab)
    with pytest.raises(ValueError, match='uint8 label map'):
        ops.seg_cross_entropy(z, lab.long())
    with pytest.raises(ValueError, match=r'\(N, H, W, C\) expected'):
        ops.seg_cross_entropy(z[0], lab)
    with pytest.raises(ValueError, match='class weights'):
        ops.seg_cross_entropy(z, lab, torch.ones(4, dtype=torch.float64))
    with pytest.raises(ValueError, match='5 classes in logits of 4 channels'):
        ops.seg_cross_entropy(z, lab, torch.ones(5))
    with pytest.raises(ValueError, match='17 classes'):
        ops.seg_cross_entropy(torch.zeros(1, 2, 2, 17), torch.zeros(1, 2, 2, dtype=torch.uint8))
    with pytest.raises(ValueError, match='one N x H x W'):
        ops.seg_cross_entropy(z, torch.zeros(2, 4, 5, dtype=torch.uint8))
    with pytest.raises(ValueError, match='bf16 or fp32 logits'):
        ops.seg_argmax_u8(z.half())
    with pytest.raises(ValueError, match='at least 1 x 1'):
        ops.seg_argmax_u8(z, 0, 5)
    with pytest.raises(ValueError, match='uint8 masks'):
        ops.seg_confusion(lab, lab.int(), 4)
    with pytest.raises(ValueError, match='1 to 16 classes'):
        ops.seg_confusion(lab, lab, 17)
    with pytest.raises(ValueError, match='one non-empty shape'):
        ops.seg_confusion(lab, lab[:1], 4)
    with pytest.raises(ValueError, match=r'out: int64 \(4, 4\)'):
        ops.seg_confusion(lab, lab, 4, out=torch.zeros(4, 4, dtype=torch.int32))
    # valid CPU tensors: the device check is what refuses them
    with pytest.raises(_lib.Seg2EyeHipError, match='GPU only'):
        ops.seg_cross_entropy(z, lab)
    with pytest.raises(_lib.Seg2EyeHipError, match='GPU only'):
        ops.seg_cross_entropy(z.bfloat16(), lab, torch.ones(3))
    with pytest.raises(_lib.Seg2EyeHipError, match='GPU only'):
        ops.seg_argmax_u8(z, 8, 12)
    with pytest.raises(_lib.Seg2EyeHipError, match='GPU only'):
        ops.seg_confusion(lab, lab, 4)
    with pytest.raises(_lib.Seg2EyeHipError, match='HIP kernels only'):
        from seg2eye_amd.segment import build_network, seg_options
        build_network(seg_options(nsf=8), 'cpu')(torch.zeros(1, 1, 8, 8))


def test_network_keys_are_the_hash_fills():
    from seg2eye_amd.segment import build_network, seg_options
    net = build_network(seg_options(nsf=8, label_nc=4), 'cpu')
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == R.manifest(8)
    sd = R.hash_state(net)
    assert set(sd) == set(net.state_dict()) and sd['out.weight'].shape == (4, 8, 3, 3)
    with pytest.raises(ValueError, match='multiple of 8'):
        build_network(seg_options(nsf=12), 'cpu')
    with pytest.raises(ValueError, match='seg_hw'):
        seg_options(seg_hw=(60, 40))


# ------------------------------------------------------------------------------------------------ the mask writer's walk
@pytest.fixture()
def restated_ops(monkeypatch):
    """The two ops predict_masks calls replaced by the restatement on CPU tensors (seg2eye_amd.segment looks them up when called)."""
    from seg2eye_amd.ops import preprocess, segment

    def resize_bicubic_u8(frames, Ho, Wo, flip, return_u8=False):
        assert frames.dtype == torch.uint8 and not bool(flip.any())
        return R.host_input(frames.numpy(), (Ho, Wo))[:, 0]

    def seg_argmax_u8(logits, Ho=None, Wo=None, ncls=None):
        return torch.from_numpy(R.argmax_resized(logits.float().numpy(), Ho, Wo, logits.shape[3])[0])
    monkeypatch.setattr(preprocess, 'resize_bicubic_u8', resize_bicubic_u8)
    monkeypatch.setattr(segment, 'seg_argmax_u8', seg_argmax_u8)


def _stub(x):
    """Fixed logits from the image alone: the class whose grey level (tests/_segment_ref.py: GREY) is nearest."""
    grey = torch.tensor(R.GREY / 255.0 * 2 - 1, dtype=torch.float32)
    return -(x.permute(0, 2, 3, 1) - grey) ** 2


@pytest.mark.filterwarnings('ignore:.*fewer than top')
def test_predicted_masks_are_what_style_rank_reads(restated_ops, monkeypatch, tmp_path):
    from seg2eye_amd import prepare_openeds, style_rank
    from seg2eye_amd.ops import rank
    from seg2eye_amd.segment import predict_masks, seg_options
    store, _ = SR.eye_store(seed=2, H=64, W=40, keys=('train',))
    del store['train']['U003']['images_seq']                                                 # a person without sequence frames
    opt = seg_options(seg_hw=(32, 24), batchSize=4)
    masks = predict_masks(_stub, store, 'train', opt, device='cpu')
    assert list(masks) == ['train'] and list(masks['train']) == ['U001', 'U002', 'U003']
    assert sorted(masks['train']['U001']) == ['labels_pred_gen', 'labels_pred_seq'] and sorted(masks['train']['U003']) == ['labels_pred_gen']
    for u, g in masks['train'].items():
        for k, m in g.items():
            src = store['train'][u][k.replace('labels_pred_', 'images_')]
            assert m.dtype == np.uint8 and m.shape == src.shape and m.max() < 4
            want = R.argmax_resized(_stub(R.host_input(src, (32, 24))).numpy(), 64, 40, 4)[0]
            assert np.array_equal(m, want)                                                    # row-aligned, batch by batch (5 and 6 rows in fours)
    only = predict_masks(_stub, store, 'train', opt, keys=('images_seq',), device='cpu')
    assert sorted(only['train']['U002']) == ['labels_pred_seq'] and only['train']['U003'] == {}
    # the file: what style_rank --seg_file opens
    path = prepare_openeds.save_store(masks, str(tmp_path / 'masks.h5'))
    back = style_rank._open(path)
    for u, g in masks['train'].items():
        for k, m in g.items():
            got = np.asarray(back['train'][u][k])
            assert got.dtype == np.uint8 and np.array_equal(got, m)
    # and the ranking made of it, with the restatements of tests/_style_rank_ref.py in the ops' place
    monkeypatch.setattr(rank, 'mask_distances', lambda t, c, ncls, metric='l2': torch.from_numpy(SR.distances(t.numpy(), c.numpy(), metric).astype(np.int32)))
    monkeypatch.setattr(rank, 'rank_topk', lambda d, k, ex=None: tuple(torch.from_numpy(a) for a in SR.topk(d.numpy(), k, None if ex is None else ex.numpy())))
    two = {'train': {u: store['train'][u] for u in ('U001', 'U002')}}                          # (style_rank wants both keys of a person)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        refs = style_rank.rank_styles(two, 'train', seg_store=back, top=4, device='cpu')
    assert not SR.same_refs(refs, SR.rank_styles(two, 'train', {'train': {u: masks['train'][u] for u in two['train']}}, top=4))
    assert all(len(e['index']) == 4 for u in refs['train'].values() for e in u.values())


def test_command_line_parses_the_three_commands():
    from seg2eye_amd.segment import parser
    a = parser().parse_args(['train', '--dataroot', 'x.h5', '--seg_hw', '64,40', '--class_weights', '1,2,3,4', '--niter', '3'])
    assert a.command == 'train' and a.seg_hw == (64, 40) and a.class_weights == (1.0, 2.0, 3.0, 4.0) and a.lr == 1e-3 and a.nsf == 32
    a = parser().parse_args(['eval', '--dataroot', 'x.h5'])
    assert a.dataset_key == 'validation' and a.which_epoch == 'latest' and a.seg_hw == (320, 200) and a.label_nc == 4
    a = parser().parse_args(['predict', '--dataroot', 'x.h5', '--out', 'm.h5', '--keys', 'images_gen'])
    assert a.dataset_key == 'train' and a.keys == ('images_gen',) and a.out == 'm.h5' and a.compute_dtype == 'bf16' and a.batchSize == 16
