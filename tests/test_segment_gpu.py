"""The eye segmenter on the GPU: the cross-entropy, argmax and confusion kernels against the fp64 restatement
(tests/_segment_ref.py), the network against stock torch, and the chain train -> eval -> predict -> style_rank on a synthetic store.

Bounds.  Loss and fp32 gradient: the restatement evaluated in fp32 numpy on the same inputs stands at some distance from its fp64 value;
the kernel gets 4x that distance (another summation order, another exp / log), and never less than one fp32 ulp of the value (for a
gradient: of its largest element; the distances are maxima over the elements).  A bf16 gradient is the fp32 value rounded once: at most
one bf16 step from the rounded restatement, per element.  Everything else is ==.  Measured figures: DESIGN 3.21."""
import functools

import numpy as np
import pytest
import torch

import _segment_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DT = {'fp32': torch.float32, 'bf16': torch.bfloat16}


def _ulp32(v):
    return float(np.spacing(np.float32(abs(float(v)))))


def _bf16_steps(a, b):
    """Per element, how many bf16 values lie between two bf16 tensors (0: equal, +0 and -0 included; 1: neighbours)."""
    def ordered(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i >= 0, i, -(i & 0x7fff))
    return (ordered(a) - ordered(b)).abs()


# ------------------------------------------------------------------------------------------------ cross-entropy
def _labels(kind, shape, ncls, seed):
    n, h, w = shape
    rng = np.random.RandomState(seed)
    if kind == 'eyes':
        return R.eyes(n, h, w, ncls, seed)
    if kind == 'iid':
        return rng.randint(0, ncls, shape).astype(np.uint8)
    if kind == 'one':
        return np.full(shape, ncls - 1, dtype=np.uint8)
    if kind == 'all255':
        return np.full(shape, 255, dtype=np.uint8)
    lab = rng.randint(0, ncls, shape).astype(np.uint8)          # 'sprinkled': every fifth pixel or so names no class
    hit = rng.rand(*shape) < 0.2
    lab[hit] = rng.randint(ncls, 255, shape).astype(np.uint8)[hit]
    lab.reshape(-1)[0] = 255
    return lab


def _logits(kind, shape, dtype, ncls, seed):
    """-> a CPU tensor of `dtype` (N, H, W, C); channels ncls.. hold NaN, +inf, -inf and 1e30 in turn."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(*shape, generator=g)
    if kind == 'equal':
        z = torch.full(shape, 0.75)
    elif kind == 'big':                                          # without the maximum subtracted, exp overflows
        mag = 80.0 if dtype == torch.bfloat16 else 1e4
        z = mag * torch.sign(torch.randn(*shape, generator=g)) + z
    for c in range(ncls, shape[3]):
        z[..., c] = (float('nan'), float('inf'), float('-inf'), 1e30)[(c - ncls) % 4]
    return z.to(dtype)


def _weights(kind, ncls):
    if kind == 'uniform':
        return np.ones(ncls, dtype=np.float32)
    w = np.array([(0.5, 1.0, 2.0, 4.0)[c % 4] for c in range(ncls)], dtype=np.float32)
    if kind == 'zero':
        w[min(1, ncls - 1)] = 0.0
    return w


def _run_ce(z, lab, w, scale=None):
    from seg2eye_amd import ops
    zg = z.to(DEV).requires_grad_(True)
    loss = ops.seg_cross_entropy(zg, torch.from_numpy(lab).to(DEV), torch.from_numpy(w).to(DEV))
    (loss if scale is None else loss * scale).backward()
    assert loss.dim() == 0 and loss.dtype == torch.float32 and zg.grad.dtype == z.dtype
    return loss.detach().cpu(), zg.grad.detach().cpu()


def _check_ce(shape, dname, labels='eyes', logits='normal', weights='graded', seed=0):
    n, h, w_, c, ncls = shape
    dtype = DT[dname]
    z = _logits(logits, (n, h, w_, c), dtype, ncls, seed)
    lab = _labels(labels, (n, h, w_), ncls, seed + 1)
    w = _weights(weights, ncls)
    zf = z.float().numpy()
    l64, g64 = R.ce(zf, lab, w, ncls)
    l32, g32 = R.ce(zf, lab, w, ncls, np.float32)
    loss, grad = _run_ce(z, lab, w)
    # the loss
    d_loss = abs(float(l32) - float(l64))
    b_loss = max(4 * d_loss, _ulp32(l64))
    e_loss = abs(float(loss) - float(l64))
    print('ce %s %s %s/%s/%s: loss %.9g  |fp32 restatement - fp64| %.3g  bound %.3g  |kernel - fp64| %.3g'
          % (shape, dname, labels, logits, weights, float(l64), d_loss, b_loss, e_loss))
    assert np.isfinite(float(loss)) and e_loss <= b_loss
    # the gradient
    ignored = torch.from_numpy(lab >= ncls)
    assert not grad[ignored].ne(0).any() and not torch.signbit(grad[ignored]).any()             # +0, every channel
    assert not grad[..., ncls:].ne(0).any() and not torch.signbit(grad[..., ncls:]).any()       # +0 behind ncls
    if dtype == torch.float32:
        d_g = float(np.abs(g32.astype(np.float64) - g64).max())
        b_g = max(4 * d_g, _ulp32(np.abs(g64).max()))
        e_g = float(np.abs(grad.numpy().astype(np.float64) - g64).max())
        print('   gradient: max |fp32 restatement - fp64| %.3g  bound %.3g  max |kernel - fp64| %.3g' % (d_g, b_g, e_g))
        assert e_g <= b_g
    else:
        steps = _bf16_steps(grad[..., :ncls], torch.from_numpy(g64[..., :ncls]).to(torch.bfloat16))
        print('   bf16 gradient: %d of %d elements one step from the rounded restatement, largest distance %d steps'
              % (int((steps == 1).sum()), steps.numel(), int(steps.max())))
        assert int(steps.max()) <= 1
    return z, lab, w, loss, grad


CE_SHAPES = [(1, 1, 1, 4, 4), (2, 5, 7, 4, 4), (1, 16, 24, 8, 4), (3, 33, 65, 4, 3), (2, 64, 40, 16, 16), (4, 320, 200, 4, 4)]


@pytest.mark.parametrize('dname', ['fp32', 'bf16'])
@pytest.mark.parametrize('shape', CE_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_cross_entropy_shapes(shape, dname):
    """Every load form (pitch 4, pitch 8, any), one pixel, ragged sizes, pad channels full of NaN / inf, many partials through the fold."""
    labels = 'iid' if shape[1] == 1 else 'eyes' if shape[4] == 4 else 'sprinkled'               # (the one pixel is a counted one)
    z, lab, w, loss, grad = _check_ce(shape, dname, labels, seed=sum(shape))
    again = _run_ce(z, lab, w)
    assert torch.equal(again[0], loss) and torch.equal(again[1], grad)                          # two calls: the same bits
    clean = z.clone()
    clean[..., shape[4]:] = 0
    planted = _run_ce(clean, lab, w)
    assert torch.equal(planted[0], loss) and torch.equal(planted[1], grad)                      # the pad channels change nothing


@pytest.mark.parametrize('dname', ['fp32', 'bf16'])
@pytest.mark.parametrize('labels,logits,weights', [
    ('iid', 'normal', 'uniform'), ('one', 'normal', 'graded'), ('sprinkled', 'normal', 'zero'), ('iid', 'equal', 'graded'),
    ('eyes', 'big', 'uniform'), ('sprinkled', 'big', 'graded'), ('iid', 'equal', 'uniform'), ('one', 'big', 'zero')])
def test_cross_entropy_labels_logits_weights(labels, logits, weights, dname):
    _check_ce((3, 33, 65, 4, 3) if labels != 'eyes' else (2, 40, 24, 4, 4), dname, labels, logits, weights, seed=11)


@pytest.mark.parametrize('dname', ['fp32', 'bf16'])
def test_cross_entropy_of_nothing_is_zero(dname):
    for weights, labels in (('graded', 'all255'), ('zero', 'one')):                             # no counted pixel; only weight-0 pixels
        ncls = 4 if labels == 'all255' else 2
        z = _logits('normal', (2, 5, 7, 4), DT[dname], ncls, 3)
        loss, grad = _run_ce(z, _labels(labels, (2, 5, 7), ncls, 4), _weights(weights, ncls))
        assert float(loss) == 0.0 and not grad.ne(0).any() and not torch.signbit(grad).any()


@pytest.mark.parametrize('dname', ['fp32', 'bf16'])
def test_cross_entropy_gradient_scales_with_the_upstream_factor(dname):
    """loss * 3 -> gradient * 3.  The factor enters the per-pixel coefficient g w / denom before the product with (softmax - onehot):
    two more roundings than 3 * (the gradient of factor 1), so 4 units of the format's epsilon, relative."""
    z = _logits('normal', (2, 5, 7, 4), DT[dname], 4, 5)
    lab, w = _labels('sprinkled', (2, 5, 7), 4, 6), _weights('graded', 4)
    l1, g1 = _run_ce(z, lab, w)
    l3, g3 = _run_ce(z, lab, w, scale=3.0)
    assert torch.equal(l1, l3)
    eps = 2.0 ** -23 if dname == 'fp32' else 2.0 ** -8
    assert torch.allclose(g3.double(), 3 * g1.double(), rtol=4 * eps, atol=0) and g1.ne(0).any()


def test_cross_entropy_unaligned_logits_take_the_scalar_loads():
    """A bf16 (.., 4) tensor that starts 2 bytes off an 8-byte boundary: the same values through the other load form, the same bits."""
    from seg2eye_amd import ops
    z = _logits('normal', (2, 5, 7, 4), torch.bfloat16, 4, 8)
    lab, w = torch.from_numpy(_labels('iid', (2, 5, 7), 4, 9)).to(DEV), torch.ones(4, device=DEV)
    buf = torch.zeros(z.numel() + 1, dtype=torch.bfloat16, device=DEV)
    off = buf[1:].view(z.shape)
    off.copy_(z)
    assert off.data_ptr() % 8 == 2 and off.is_contiguous()
    assert torch.equal(ops.seg_cross_entropy(off, lab, w), ops.seg_cross_entropy(z.to(DEV), lab, w))


# ------------------------------------------------------------------------------------------------ argmax
def _quarters(shape, ncls, seed):
    """Multiples of 1/4 in [-8, 8] (exact in bf16 and fp32), with ties planted between classes 1 and 2 above everything else and all
    channels equal elsewhere; channels ncls.. hold huge values."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randint(-32, 33, shape, generator=g).float() / 4
    n, h, w, c = shape
    if ncls >= 3:
        z[:, : max(1, h // 3), :, 1] = 8.0
        z[:, : max(1, h // 3), :, 2] = 8.0
    z[:, h - 1, :, :ncls] = -2.5
    for k in range(ncls, c):
        z[..., k] = (1e30, float('inf'), float('nan'), 3e38)[(k - ncls) % 4]
    return z


@pytest.mark.parametrize('dname', ['fp32', 'bf16'])
@pytest.mark.parametrize('shape,ncls', [((2, 8, 8, 4), 4), ((3, 5, 7, 8), 4), ((1, 5, 7, 4), 3), ((2, 8, 8, 16), 16), ((1, 320, 200, 4), 4)],
                         ids=['8x8', '5x7_pitch8', '5x7_3of4', '8x8_16', '320x200'])
def test_argmax_exact_at_twice_the_size_and_at_the_same_size(shape, ncls, dname):
    """Taps of 0.25 / 0.75 on multiples of 1/4: every sum is exact in fp32, so every pixel is ==, ties to the lower class included."""
    from seg2eye_amd import ops
    z = _quarters(shape, ncls, seed=shape[1]).to(DT[dname])
    n, h, w, c = shape
    want, gap = R.argmax_resized(z.float().numpy(), 2 * h, 2 * w, ncls)
    got = ops.seg_argmax_u8(z.to(DEV), 2 * h, 2 * w, ncls=ncls)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (n, 2 * h, 2 * w)
    assert (gap == 0).sum() > 0 and np.array_equal(got.cpu().numpy(), want)
    same = ops.seg_argmax_u8(z.to(DEV), ncls=ncls)
    assert np.array_equal(same.cpu().numpy(), np.nan_to_num(z.float().numpy()[..., :ncls], nan=-np.inf).argmax(-1).astype(np.uint8))
    assert int(got.max()) < ncls and int(same.max()) < ncls


@pytest.mark.parametrize('dname', ['fp32', 'bf16'])
@pytest.mark.parametrize('shape,out', [((2, 7, 5, 4), (13, 11)), ((1, 80, 50, 4), (640, 400)), ((2, 9, 6, 8), (4, 5))], ids=['7x5', '80x50', 'shrink'])
def test_argmax_general_sizes(shape, out, dname):
    """N(0, 1) logits: == wherever the restatement's two largest resized logits are more than 1e-5 apart (fp32 taps and sums are good
    to ~1e-6 here); at most 0.1 % of a case's pixels may be closer -- the restatement alone, for these seeds: 0 of 286, 5 of 256 000 (4 in bf16), 0 of 40."""
    from seg2eye_amd import ops
    z = torch.randn(*shape, generator=torch.Generator().manual_seed(shape[1])).to(DT[dname])
    ncls = 4
    if shape[3] > ncls:
        z[..., ncls:] = 1e30
    want, gap = R.argmax_resized(z.float().numpy(), out[0], out[1], ncls)
    clear = gap > 1e-5
    print('argmax %s -> %s %s: %d of %d pixels left out' % (shape, out, dname, int((~clear).sum()), clear.size))
    assert (~clear).mean() <= 1e-3
    got = ops.seg_argmax_u8(z.to(DEV), out[0], out[1], ncls=ncls).cpu().numpy()
    assert np.array_equal(got[clear], want[clear]) and got.max() < ncls


# ------------------------------------------------------------------------------------------------ confusion
@pytest.mark.parametrize('ncls', [3, 4, 16])
@pytest.mark.parametrize('P', [1, 391, 256000])
def test_confusion_counts(P, ncls):
    from seg2eye_amd import ops
    rng = np.random.RandomState(P + ncls)
    if P == 256000:                                              # masks: runs of equal pairs, as the kernel merges them
        t = R.eyes(1, 640, 400, min(ncls, 4), 1)[0].reshape(-1)
        p = np.roll(t, 3 * 400 + 2)
        noise = rng.rand(P) < 0.05
        p = np.where(noise, rng.randint(0, ncls + 2, P), p).astype(np.uint8)
    else:
        t, p = rng.randint(0, ncls + 2, P).astype(np.uint8), rng.randint(0, ncls + 2, P).astype(np.uint8)
        t[0], p[0] = ncls - 1, ncls - 1
    t[P // 2] = 255
    want = R.confusion(p, t, ncls)
    tp, tt = torch.from_numpy(p).to(DEV), torch.from_numpy(t).to(DEV)
    conf = ops.seg_confusion(tp, tt, ncls)
    assert conf.dtype == torch.int64 and np.array_equal(conf.cpu().numpy(), want) and (P == 1 or want.sum() < P)
    again = ops.seg_confusion(tt, tp, ncls, out=conf)                                           # accumulates: + the transpose
    assert again is conf and np.array_equal(conf.cpu().numpy(), want + want.T)
    if P > 1:                                                    # an unaligned start: one pixel per lane, the same counts
        assert np.array_equal(ops.seg_confusion(tp[1:], tt[1:], ncls).cpu().numpy(), R.confusion(p[1:], t[1:], ncls))


def test_confusion_cells_count_past_two_to_the_31():
    """The matrix is int64 and the atomics are 64-bit: a cell that stands just below 2^31 and one just below 2^32 take a 640 x 400
    'same' pair's counts to exact sums beyond both."""
    from seg2eye_amd import ops
    t = R.eyes(1, 640, 400, 4, 2)
    want = R.confusion(t, t, 4)
    pre = np.zeros((4, 4), dtype=np.int64)
    pre[0, 0], pre[1, 1], pre[2, 3] = (1 << 31) - 5, (1 << 32) - 7, 1 << 40
    conf = torch.from_numpy(pre.copy()).to(DEV)
    m = torch.from_numpy(t).to(DEV)
    for _ in range(3):
        ops.seg_confusion(m, m, 4, out=conf)
    assert want[0, 0] > 5 and want[1, 1] > 7 and np.array_equal(conf.cpu().numpy(), pre + 3 * want)
    assert int(conf[0, 0]) > (1 << 31) and int(conf[1, 1]) > (1 << 32)


# ------------------------------------------------------------------------------------------------ the network
def _net(nsf, dname, hw=(320, 200)):
    from seg2eye_amd.segment import build_network, seg_options
    opt = seg_options(nsf=nsf, compute_dtype=dname, seg_hw=hw)
    net = build_network(opt, DEV)
    sd = R.hash_state(net, seed=0, dtype=torch.float64)
    with torch.no_grad():
        for k, v in net.state_dict().items():
            v.copy_(sd[k].float())
    return net, sd, opt


@pytest.mark.parametrize('hw', [(32, 24), (40, 56)], ids=['32x24', '40x56'])
def test_network_fp32_matches_the_restatement(hw):
    """Hash-filled weights, N = 2, nsf 8: the logits within 1e-3 max-abs (the project's fp32 parity bar, G_TOL of test_networks_gpu.py),
    every weight and bias gradient of the cross-entropy within rtol 2e-3, atol 2e-4 (that file's gradient bounds)."""
    from seg2eye_amd import ops
    from seg2eye_amd.synthetic import hash_uniform
    net, sd, _ = _net(8, 'fp32')
    x = torch.from_numpy(hash_uniform('seg_x', (2, 1) + hw, seed=1))
    lab = torch.from_numpy(R.eyes(2, hw[0], hw[1], 4, 5))
    lab[0, 0, :4] = 255
    logits = net(x.to(DEV))
    assert tuple(logits.shape) == (2,) + hw + (4,) and logits.dtype == torch.float32
    ops.seg_cross_entropy(logits, lab.to(DEV)).backward()
    ref = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    want = R.net_forward(ref, x.double())
    R.ce_torch(want, lab).backward()
    err = float((logits.detach().cpu().double() - want.detach()).abs().max())
    print('segmenter %dx%d fp32: logits max-abs error %.3g' % (hw + (err,)))
    assert err < 1e-3
    for k, p in net.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), ref[k].grad.numpy(), rtol=2e-3, atol=2e-4, err_msg=k)
        assert float(ref[k].grad.abs().max()) > 0


def test_network_bf16_runs():
    net, _, _ = _net(8, 'bf16')
    from seg2eye_amd.synthetic import hash_uniform
    logits = net(torch.from_numpy(hash_uniform('seg_x', (2, 1, 32, 24), seed=1)).to(DEV))
    assert tuple(logits.shape) == (2, 32, 24, 4) and logits.dtype == torch.bfloat16 and bool(torch.isfinite(logits.float()).all())


# ------------------------------------------------------------------------------------------------ end to end
E2E = dict(nsf=8, seg_hw=(64, 40), compute_dtype='fp32', batchSize=6, niter=10, lr=2e-3, seed=7, no_flip=True)


@functools.lru_cache(maxsize=None)
def _store():
    return R.learnable_store()


def test_train_eval_predict_rank_end_to_end(tmp_path):
    """30 steps on 18 labelled frames at 64 x 40, nsf 8, fp32, from the hash-filled weights.  The fp64 restatement of the same run
    (tests/_segment_ref.py: train_restated; figures in DESIGN 3.21) satisfies both conditions with room to spare."""
    from seg2eye_amd import checkpoint, segment, style_rank
    store, _ = _store()
    net, _, _ = _net(8, 'fp32', (64, 40))
    opt = segment.seg_options(checkpoints_dir=str(tmp_path), name='seg', **E2E)
    before = segment.evaluate(net, store, 'validation', opt, DEV, verbose=False)
    net, hist = segment.train_segmenter(store, opt, net=net, device=DEV, verbose=False)
    loss, after = hist['loss'], hist['scores'][-1]
    print('end to end: loss first five %.4f last five %.4f; validation mIoU %.4f -> %.4f'
          % (np.mean(loss[:5]), np.mean(loss[-5:]), before['miou/validation'], after['miou/validation']))
    assert len(loss) == 30 and len(hist['scores']) == 10 and np.isfinite(loss).all()
    assert np.mean(loss[-5:]) < np.mean(loss[:5])
    assert after['miou/validation'] > before['miou/validation']
    assert set(after) == {'miou/validation', 'acc/validation'} | {'iou/validation/%d' % c for c in range(4)}
    # the masks of the unlabelled frames, and the ranking made of them
    masks = segment.predict_masks(net, store, 'train', opt, device=DEV)
    for u, g in store['train'].items():
        assert sorted(masks['train'][u]) == ['labels_pred_gen', 'labels_pred_seq']
        for k in ('gen', 'seq'):
            m = masks['train'][u]['labels_pred_' + k]
            assert m.dtype == np.uint8 and m.shape == g['images_' + k].shape == (4, 640, 400) and m.max() < 4
    refs = style_rank.rank_styles(store, 'train', seg_store=masks, top=4, device=DEV)
    for u, g in store['train'].items():
        assert len(refs['train'][u]) == 6 and all(len(e['index']) == 4 for e in refs['train'][u].values())
    # a checkpoint saved and loaded back predicts the same masks
    other, _, _ = _net(8, 'fp32', (64, 40))
    checkpoint.load_network(other, 'S', 'latest', opt)
    again = segment.predict_masks(other, store, 'train', opt, device=DEV)
    for u in masks['train']:
        for k, m in masks['train'][u].items():
            assert np.array_equal(again['train'][u][k], m)
    assert (tmp_path / 'seg' / '10_net_S.pth').exists()
