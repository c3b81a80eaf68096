"""The residual refiner on the GPU: the four kernels against the restatement (tests/_refine_ref.py), the network against
stock torch, and the tool train -> eval -> predict on a synthetic store.

Bounds.  The network input (fp32, and bf16 against the rounded restatement), the uint8 prediction and the zero channels are ==.  Score,
terms, loss and the fp32 gradient follow the project's rule: the restatement evaluated in fp32 numpy stands at some
distance from its fp64 value; the kernel gets 4x that distance, never less than one fp32 ulp of the value (for a gradient: of its
largest element; the distances are maxima over the elements).  A bf16 gradient is the fp32 value rounded once: at most one bf16 step
from the rounded restatement, per element.  Measured figures: DESIGN 3.23."""
import functools

import numpy as np
import pytest
import torch

import _refine_ref as R
import _segment_ref as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DT = {'fp32': torch.float32, 'bf16': torch.bfloat16}
# one pixel; ragged; a row across a wave; longer than a workgroup in each direction; whole words per row, two images
SHAPES = [(1, 1, 1), (2, 5, 7), (1, 1, 67), (1, 3, 300), (1, 300, 3), (2, 64, 40)]
BIG = (2, 640, 400)
FLIPS = ('none', 'off', 'mixed')
ids = dict(ids=lambda s: 'x'.join(map(str, s)))


def _ulp32(v):
    return float(np.spacing(np.float32(abs(float(v)))))


def _bf16_steps(a, b):
    """Per element, how many bf16 values lie between two bf16 tensors (0: equal, +0 and -0 included; 1: neighbours)."""
    def ordered(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i >= 0, i, -(i & 0x7fff))
    return (ordered(a) - ordered(b)).abs()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _res(res, dname):
    return torch.from_numpy(res).to(DT[dname]).to(DEV)


# ------------------------------------------------------------------------------------------------ the network input
def _check_input(shape, dname, C, flipkind, seed, levels=None, ncls=4):
    from seg2eye_amd import ops
    tmask, rimg, rmask, _ = R.planes(shape, seed, ncls=ncls)
    flip = R.flips(flipkind, shape[0], seed)
    want = R.refine_input(tmask, rimg, rmask, flip, R.LEVELS if levels is None else levels, ncls, C)
    x = ops.refine_input(_dev(tmask), _dev(rimg), _dev(rmask), _dev(flip), levels=levels, ncls=ncls, channels=C, dtype=DT[dname]).cpu()
    assert x.dtype == DT[dname] and tuple(x.shape) == shape + (C,)
    assert torch.equal(x, torch.from_numpy(want) if dname == 'fp32' else R.to_bf16(want)), (shape, dname, C, flipkind)
    assert not torch.signbit(x[..., 3:]).any() and not x[..., 3:].ne(0).any()
    return x


@pytest.mark.parametrize('dname', ['fp32', 'bf16'])
@pytest.mark.parametrize('shape', SHAPES, **ids)
def test_input_is_the_restatement_bit_for_bit(shape, dname):
    for C in (3, 8):
        for flipkind in FLIPS:
            _check_input(shape, dname, C, flipkind, seed=sum(shape) + C)
    _check_input(shape, dname, 5, 'mixed', seed=3, levels=(9, 200, 255), ncls=3)      # other levels, labels 3 and 4 take level 0


def test_input_at_the_frames_size_and_from_unaligned_planes():
    from seg2eye_amd import ops
    _check_input(BIG, 'bf16', 8, 'mixed', seed=1)
    tmask, rimg, rmask, _ = R.planes((2, 64, 40), 2)
    flip = _dev(R.flips('mixed', 2))
    want = ops.refine_input(_dev(tmask), _dev(rimg), _dev(rmask), flip, dtype=torch.float32)

    def off(a):                                                  # the same bytes one byte past a 256-byte boundary: byte loads
        buf = torch.zeros(a.size + 1, dtype=torch.uint8, device=DEV)
        buf[1:].copy_(torch.from_numpy(a).reshape(-1))
        return buf[1:].view(a.shape)
    got = ops.refine_input(off(tmask), off(rimg), off(rmask), flip, dtype=torch.float32)
    assert off(rimg).data_ptr() % 4 == 1 and torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ the loss, its gradient, the bytes
def _run_head(res, rimg, truth, flip, lambdas, g=None):
    from seg2eye_amd import ops
    r = res.detach().requires_grad_(True)                       # (no copy: an unaligned view stays unaligned)
    loss, terms, score = ops.refine_loss(r, rimg, truth, flip, *lambdas)
    (loss if g is None else loss * g).backward()
    assert loss.dim() == 0 and loss.dtype == terms.dtype == score.dtype == torch.float32 and r.grad.dtype == res.dtype
    assert not terms.requires_grad and not score.requires_grad
    return loss.detach().cpu(), terms.cpu(), score.cpu(), r.grad.cpu()


def _within(name, got, v32, v64, what):
    d = abs(float(v32) - float(v64))
    bound = max(4 * d, _ulp32(v64))
    err = abs(float(got) - float(v64))
    print('  %s %s: %.9g  |fp32 restatement - fp64| %.3g  bound %.3g  |kernel - fp64| %.3g' % (what, name, float(v64), d, bound, err))
    assert np.isfinite(float(got)) and err <= bound, (what, name, float(got), float(v64), err, bound)


def _check_head(shape, dname, C, kind='mixed', flipkind='none', lambdas=(1.0, 0.0), g=None, seed=0):
    from seg2eye_amd import ops
    what = '%s %s C%d %s flip %s lambdas %s g %s' % (shape, dname, C, kind, flipkind, lambdas, g)
    _, rimg, _, truth = R.planes(shape, seed)
    res, truth = R.residual(kind, rimg, truth, C, seed + 1, bf16=dname == 'bf16')
    flip = R.flips(flipkind, shape[0], seed)
    h64 = R.head(res, rimg, truth, flip, lambdas[0], lambdas[1], 1.0 if g is None else g)
    h32 = R.head(res, rimg, truth, flip, lambdas[0], lambdas[1], 1.0 if g is None else g, dtype=np.float32)
    args = (_res(res, dname), _dev(rimg), _dev(truth), _dev(flip), lambdas)
    loss, terms, score, grad = _run_head(*args, g=g)
    print('head ' + what)
    _within('loss', loss, h32['loss'], h64['loss'], what)
    for i, name in enumerate(('eds_loss', 'l1', 'score')):
        _within(name, terms[i], h32['terms'][i], h64['terms'][i], what)
    worst = int(np.argmax(np.abs(score.numpy().astype(np.float64) - h64['score'])))
    _within('per_image_score[%d]' % worst, score[worst], h32['score'][worst], h64['score'][worst], what)
    for n in range(shape[0]):
        assert abs(float(score[n]) - h64['score'][n]) <= max(4 * abs(float(h32['score'][n]) - h64['score'][n]), _ulp32(h64['score'][n]))
    assert not grad[..., 1:].ne(0).any() and bool(torch.isfinite(grad).all())                   # the dead channels: 0, whatever res holds there
    g64 = h64['grad'][..., 0]
    if dname == 'fp32':
        d_g = float(np.abs(h32['grad'][..., 0].astype(np.float64) - g64).max())
        b_g = max(4 * d_g, _ulp32(np.abs(g64).max()))
        e_g = float(np.abs(grad[..., 0].numpy().astype(np.float64) - g64).max())
        print('  gradient: max |fp32 restatement - fp64| %.3g  bound %.3g  max |kernel - fp64| %.3g' % (d_g, b_g, e_g))
        assert e_g <= b_g, (what, e_g, b_g)
    else:
        steps = _bf16_steps(grad[..., 0], torch.from_numpy(g64).to(torch.bfloat16))
        print('  bf16 gradient: %d of %d elements one step from the rounded restatement, largest distance %d steps'
              % (int((steps == 1).sum()), steps.numel(), int(steps.max())))
        assert int(steps.max()) <= 1, what
    out = ops.refine_predict_u8(args[0], args[1], args[3])
    assert out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), R.predict_u8(res, rimg, flip)), what
    return args, (loss, terms, score, grad, out.cpu()), h64


@pytest.mark.parametrize('dname', ['fp32', 'bf16'])
@pytest.mark.parametrize('shape', SHAPES, **ids)
def test_head_shapes_channels_and_flips(shape, dname):
    """Every load form (one access per four pixels, strided elements, byte loads), the dead channels full of NaN / inf, flips absent,
    all 0 and mixed; two calls give the same bits."""
    for C in (1, 4, 8):
        for flipkind in FLIPS:
            args, got, _ = _check_head(shape, dname, C, 'mixed', flipkind, (1.0, 0.25), seed=sum(shape) + C)
    again = _run_head(*args)
    assert all(torch.equal(a, b) for a, b in zip(again, got[:4]))


@pytest.mark.parametrize('dname', ['fp32', 'bf16'])
def test_head_at_the_frames_size(dname):
    _check_head(BIG, dname, 1, 'mixed', 'mixed', (1.0, 0.5), seed=11)


@pytest.mark.parametrize('dname', ['fp32', 'bf16'])
@pytest.mark.parametrize('kind,lambdas,g', [('zero', (1.0, 0.0), None), ('zero', (0.0, 1.0), None), ('clampy', (1.0, 0.0), None),
                                            ('clampy', (0.5, 2.0), 1.75), ('mixed', (0.0, 1.0), None), ('mixed', (1.0, 1.0), 0.375),
                                            ('exact', (1.0, 0.0), None), ('exact', (1.0, 0.5), 3.0)])
def test_head_inputs_that_can_go_wrong(kind, lambdas, g, dname):
    """A zero residual on frames holding 0 and 255 (the clamp's ends are inclusive), residuals that clamp most pixels, each lambda alone
    and both, an upstream factor, and an image whose prediction equals its truth."""
    shape = (3, 33, 65)
    args, (loss, terms, score, grad, out), h64 = _check_head(shape, dname, 1, kind, 'mixed', lambdas, g, seed=21)
    rimg = args[1].cpu().numpy()
    s = args[0].float().cpu().numpy()[..., 0] + R.norm(R.flipped(rimg, R.flips('mixed', 3, 21)))
    if kind == 'zero':                                           # every pixel passes its gradient, the ones at exactly -1 and 1 included
        assert (s == 1).any() and (s == -1).any() and int((grad[..., 0] != 0).sum()) == int((h64['grad'][..., 0] != 0).sum())
        at_ends = torch.from_numpy((np.abs(s) == 1) & (h64['grad'][..., 0] != 0))
        assert at_ends.any() and bool((grad[..., 0][at_ends] != 0).all())
    if kind == 'clampy':
        assert (np.abs(s) > 1).mean() > 0.5 and not grad[..., 0][torch.from_numpy(np.abs(s) > 1)].ne(0).any()
    if kind == 'exact':                                          # sumsq == 0: a zero score, a zero gradient, everything finite
        assert float(score[0]) == 0.0 and not grad[0].ne(0).any() and grad[1].ne(0).any()
        assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(terms).all()) and np.isfinite(float(loss))
        assert np.array_equal(out[0].numpy(), R.predict_u8(np.zeros((1,) + shape[1:] + (1,), np.float32), rimg[:1, :, ::-1])[0])   # (image 0 is flipped)


def test_head_unaligned_tensors_take_the_other_loads():
    """The same values one element / one byte off their boundaries: strided and byte loads, the same bits."""
    from seg2eye_amd import ops
    shape = (2, 64, 40)
    _, rimg, _, truth = R.planes(shape, 5)
    res, truth = R.residual('mixed', rimg, truth, 1, 6, bf16=True)
    flip = _dev(R.flips('mixed', 2))

    def off(t):
        buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)
        buf[1:].copy_(t.reshape(-1))
        return buf[1:].view(t.shape)
    for dname in ('fp32', 'bf16'):
        r, ri, tr = _res(res, dname), _dev(rimg), _dev(truth)
        want = _run_head(r, ri, tr, flip, (1.0, 0.5)) + (ops.refine_predict_u8(r, ri, flip).cpu(),)
        r2, ri2, tr2 = off(r), off(ri), off(tr)
        assert r2.data_ptr() % 16 != 0 and ri2.data_ptr() % 4 == 1
        got = _run_head(r2, ri2, tr2, flip, (1.0, 0.5)) + (ops.refine_predict_u8(r2, ri2, flip).cpu(),)
        assert all(torch.equal(a, b) for a, b in zip(got, want)), dname


def test_launches_are_registered_under_the_family_refine():
    from seg2eye_amd import ops
    from seg2eye_amd.ops.core import LaunchProfiler
    shape = (2, 64, 40)
    tmask, rimg, rmask, truth = (_dev(a) for a in R.planes(shape, 7))
    prof = LaunchProfiler()
    LaunchProfiler.install(prof)
    try:
        x = ops.refine_input(tmask, rimg, rmask)
        res = torch.zeros(shape + (1,), dtype=torch.bfloat16, device=DEV, requires_grad=True)
        ops.refine_loss(res, rimg, truth)[0].backward()
        ops.refine_predict_u8(res, rimg)
        torch.cuda.synchronize()
    finally:
        LaunchProfiler.install(None)
    fam = prof.summary()['refine']
    px = 2 * 64 * 40
    assert x.dtype == torch.bfloat16 and fam['launches'] == 4 and fam['bytes'] == px * ((3 + 16) + (2 + 2) + (4 + 2) + (2 + 2)) and fam['ms'] > 0


# ------------------------------------------------------------------------------------------------ the network
def _net(nrf, dname, fill=True):
    from seg2eye_amd.refine import build_network, refine_options
    opt = refine_options(nrf=nrf, compute_dtype=dname)
    net = build_network(opt, DEV)
    sd = S.hash_state(net, seed=0, dtype=torch.float64)
    if fill:
        with torch.no_grad():
            for k, v in net.state_dict().items():
                v.copy_(sd[k].float())
    return net, sd, opt


@pytest.mark.parametrize('hw', [(32, 24), (40, 56)], ids=['32x24', '40x56'])
def test_network_fp32_matches_the_restatement(hw):
    """Hash-filled weights (a non-zero `out`), N = 2, nrf 8: the residual within 1e-3 max-abs, every weight and bias gradient of
    refine_loss within rtol 2e-3, atol 2e-4 -- the bars of test_segment_gpu.py."""
    from seg2eye_amd import ops
    net, sd, _ = _net(8, 'fp32')
    tmask, rimg, rmask, truth = R.planes((2,) + hw, 3)
    x = ops.refine_input(_dev(tmask), _dev(rimg), _dev(rmask), dtype=torch.float32)
    res = net(x)
    assert tuple(res.shape) == (2,) + hw + (1,) and res.dtype == torch.float32
    ops.refine_loss(res, _dev(rimg), _dev(truth), None, 1.0, 0.5)[0].backward()
    ref = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    want = R.net_residual(ref, torch.from_numpy(R.refine_input(tmask, rimg, rmask)).double())
    R.loss_torch(want, rimg, truth, 1.0, 0.5)[0].backward()
    err = float((res.detach().cpu().double() - want.detach()).abs().max())
    print('refiner %dx%d fp32: residual max-abs error %.3g' % (hw + (err,)))
    assert err < 1e-3
    for k, p in net.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), ref[k].grad.numpy(), rtol=2e-3, atol=2e-4, err_msg=k)
        assert float(ref[k].grad.abs().max()) > 0


def test_network_bf16_runs():
    from seg2eye_amd import ops
    net, _, _ = _net(8, 'bf16')
    tmask, rimg, rmask, truth = (_dev(a) for a in R.planes((2, 32, 24), 3))
    res = net(ops.refine_input(tmask, rimg, rmask))
    assert tuple(res.shape) == (2, 32, 24, 1) and res.dtype == torch.bfloat16 and bool(torch.isfinite(res.float()).all())
    loss, terms, score = ops.refine_loss(res, rimg, truth)
    loss.backward()
    assert np.isfinite(float(loss.detach())) and all(bool(torch.isfinite(p.grad).all()) for p in net.parameters())


@pytest.mark.parametrize('dname', ['fp32', 'bf16'])
def test_a_new_refiner_predicts_its_reference_frame(dname):
    """build_network zero-fills `out`: the residual is 0, the bytes are the restated ones -- the frame to within one grey level."""
    from seg2eye_amd import ops
    net, _, _ = _net(8, dname, fill=False)
    tmask, rimg, rmask, _ = R.planes((2, 32, 24), 4)
    rimg[0, 0, :] = np.arange(24) * 11                           # (levels of both kinds of the round trip)
    res = net(ops.refine_input(_dev(tmask), _dev(rimg), _dev(rmask), dtype=DT[dname]))
    assert not res.ne(0).any()
    out = ops.refine_predict_u8(res, _dev(rimg)).cpu().numpy()
    assert np.array_equal(out, R.predict_u8(np.zeros((2, 32, 24, 1), np.float32), rimg))
    off = rimg.astype(np.int64) - out
    assert off.min() == 0 and off.max() == 1


# ------------------------------------------------------------------------------------------------ end to end
E2E = dict(nrf=8, compute_dtype='fp32', batchSize=6, niter=10, lr=2e-3, seed=7, no_flip=True, refine_top=4)


@functools.lru_cache(maxsize=None)
def _store():
    return S.learnable_store(H=64, W=40)


def test_train_eval_predict_end_to_end(tmp_path):
    """30 steps on 18 targets at 64 x 40, nrf 8, fp32, from a new network (kaiming, `out` zero), the references drawn among the four
    nearest of style_rank.  The fp64 restatement of the same run (tests/_refine_ref.py: train_restated, on the host ranking of
    tests/_style_rank_ref.py; figures in DESIGN 3.23) meets both inequalities with room: loss 1.113 -> 0.681, validation 1498 -> 1029.
    Before training the figure is the nearest frame's to within the round trip's one level (1502 against 1498), not equal to it."""
    from seg2eye_amd import checkpoint, refine, style_rank
    store, seg = _store()
    refs = {**style_rank.rank_styles(store, 'train', seg_store=seg, top=4, device=DEV),
            **style_rank.rank_styles(store, 'validation', seg_store=seg, top=4, device=DEV)}
    opt = refine.refine_options(checkpoints_dir=str(tmp_path), name='ref', **E2E)
    net = refine.build_network(opt, DEV)
    before = refine.evaluate(net, store, seg, refs, 'validation', opt, DEV, verbose=False)
    net, hist = refine.train_refiner(store, seg, refs, opt, net=net, device=DEV, verbose=False)
    loss, after = hist['loss'], hist['scores'][-1]
    print('end to end: loss first five %.4f last five %.4f; validation %.2f -> %.2f, nearest frame %.2f (before training: %.2f)'
          % (np.mean(loss[:5]), np.mean(loss[-5:]), before['openeds/validation'], after['openeds/validation'], after['openeds_nn/validation'],
             before['openeds_nn/validation']))
    assert len(loss) == 30 and len(hist['terms']) == 30 and len(hist['scores']) == 10 and np.isfinite(loss).all()
    assert np.mean(loss[-5:]) < np.mean(loss[:5])
    assert after['openeds/validation'] < after['openeds_nn/validation'] == before['openeds_nn/validation']
    assert set(after) == {'openeds/validation', 'openeds_nn/validation'}
    rows = R.target_list(store, 'validation')
    first = [R.expected_reference(store, seg, refs, 'validation', u, f)[0] for u, _, f in rows]
    truth = [store['validation'][u]['images_ss'][i] for u, i, _ in rows]
    assert abs(after['openeds_nn/validation'] - R.openeds_u8(np.stack(first), np.stack(truth))) < 1e-3 * after['openeds_nn/validation']
    # the frames of every target, and the files of a submission
    out = tmp_path / 'submission'
    frames = refine.predict_frames(net, store, seg, refs, 'validation', opt, device=DEV, out=str(out))
    assert sorted(frames) == ['U201', 'U202'] and sum(len(v) for v in frames.values()) == len(rows) == 12
    listed = (out / 'pred_npy_list.txt').read_text().split()
    assert listed == [str(out / ('%s.npy' % f)) for _, _, f in rows]
    for u, _, f in rows:
        assert frames[u][f].dtype == np.uint8 and frames[u][f].shape == (64, 40) and np.array_equal(np.load(out / ('%s.npy' % f)), frames[u][f])
    # a checkpoint saved and loaded back predicts the same bytes
    other = refine.build_network(opt, DEV)
    checkpoint.load_network(other, 'R', 'latest', opt)
    again = refine.predict_frames(other, store, seg, refs, 'validation', opt, device=DEV)
    assert all(np.array_equal(again[u][f], frames[u][f]) for u, _, f in rows)
    assert (tmp_path / 'ref' / '10_net_R.pth').exists()
