"""SSIM on the GPU: ops.ssim / ops.ssim_u8 and the backward against the fp64 restatement of tests/_ssim_ref.py (whose
gradient is autograd's), every element; the generator's --lambda_ssim term, eager and as hipGraph replays; the Tester under --val_ssim.

Bounds come from the restatement, never from the kernel.  Per case, e is the error of the SAME restatement run in fp32 against fp64 on
the same inputs -- for ssim the largest over the images, for the gradient the largest element divided by its image's largest |gradient|.
The kernel must stay within max(4 e, 16 * 2^-24): 4 for another summation order, the floor a few fp32 ulps of a quantity of order 1.
A bf16 gradient element may be off by a further 2^-8 of its own magnitude (the output's rounding).  bf16 inputs are rounded first and
the oracle sees the rounded values.

e as measured (fp32 inputs; `python tests/test_ssim_gpu.py` prints the table, on any machine -- it needs no GPU):

    shape        kind     e(ssim)    e(gradient)
    2x11x11      iid      6.8e-07    1.6e-06
    2x11x11      smooth   9.9e-06    3.1e-05
    2x11x11      bright   3.2e-04    1.5e-03
    2x12x17      iid      5.3e-08    6.9e-07
    2x12x17      smooth   1.5e-05    1.5e-05
    2x12x17      bright   1.9e-04    3.2e-04
    3x43x70      iid      3.2e-08    1.3e-06
    3x43x70      smooth   1.7e-06    1.9e-05
    3x43x70      bright   1.4e-05    4.2e-04
    2x64x64      iid      3.2e-08    1.3e-06
    2x64x64      smooth   1.1e-06    2.5e-05
    2x64x64      bright   1.9e-05    4.5e-04
    2x256x256    iid      1.6e-08    1.5e-06
    2x256x256    smooth   6.3e-07    2.4e-05
    2x256x256    bright   2.9e-06    4.8e-04

The kernels take their moments about each tile's first pixel, so their own error on `ssim` does not grow on the bright-flat inputs (measured on an
MI355X: within 1.4e-7 in every case; the gradient within 1e-6 of the image's largest on iid and smooth inputs, 1.3e-5 on bright-flat ones)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _ssim_ref as R
from _quality_harness import batch as _batch, load_log as _load_log, trainer as _trainer

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SHAPES = [(2, 11, 11), (2, 12, 17), (3, 43, 70), (2, 64, 64), (2, 256, 256)]   # one position; 2 x 7; ragged tiles, halos cross on both axes; ...
SHAPE_IDS = ['x'.join(map(str, s)) for s in SHAPES]
KINDS = ['iid', 'smooth', 'bright']
DTYPES = [torch.float32, torch.bfloat16]
DTYPE_IDS = ['fp32', 'bf16']
FLOOR = 16 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ inputs and references (computed once)
@functools.lru_cache(maxsize=None)
def _inputs(shape, kind, rounded):
    """x, y (fp64 values of fp32 -- or, rounded, bf16 -- numbers) and a random incoming gradient per image; CPU, never written."""
    n, H, W = shape
    gen = torch.Generator().manual_seed(100000 * KINDS.index(kind) + 1000 * n + 31 * H + W)
    if kind == 'iid':
        x, y = torch.rand(n, H, W, generator=gen) * 2 - 1, torch.rand(n, H, W, generator=gen) * 2 - 1
    elif kind == 'smooth':                                    # a 9 x 9 box blur of iid noise; the target is a noisy copy
        x = F.avg_pool2d(torch.rand(n, 1, H + 8, W + 8, generator=gen) * 2 - 1, 9, 1)[:, 0]
        y = (x + 0.1 * torch.randn(n, H, W, generator=gen)).clamp(-1, 1)
    else:                                                     # bright and flat: where E[u^2] - mu^2 cancels in fp32
        x = 0.9 + 0.01 * (torch.rand(n, H, W, generator=gen) * 2 - 1)
        y = 0.88 + 0.01 * (torch.rand(n, H, W, generator=gen) * 2 - 1)
    if rounded:
        x, y = x.bfloat16(), y.bfloat16()
    gs = torch.randn(n, generator=gen)
    return x.double(), y.double(), gs.double()


@functools.lru_cache(maxsize=None)
def _reference(shape, kind, rounded):
    """(ssim64, grad64, image max |grad64|, bound on ssim, bound on gradient / image max) for one case."""
    x, y, gs = _inputs(shape, kind, rounded)
    s64, g64 = R.ssim_and_grad(x, y, gs, torch.float64)
    s32, g32 = R.ssim_and_grad(x, y, gs, torch.float32)
    gmax = g64.abs().amax(dim=(1, 2), keepdim=True)
    e_s = float((s32.double() - s64).abs().max())
    e_g = float(((g32.double() - g64).abs() / gmax).max())
    return s64, g64, gmax, e_s, e_g


def _bound(e):
    return max(4 * e, FLOOR)


def _run(x, y, gs, dtype, grad=True):
    from seg2eye_amd import ops
    n, H, W = x.shape
    xd = x.to(DEV, dtype).view(n, 1, H, W).requires_grad_(grad)
    s = ops.ssim(xd, y.to(DEV, dtype).view(n, 1, H, W))
    if grad:
        s.backward(gs.to(DEV, torch.float32))
    return s.detach(), (xd.grad.view(n, H, W) if grad else None)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ------------------------------------------------------------------------------------------------ the op
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
def test_forward_and_backward_match_the_restatement(shape, kind, dtype):
    rounded = dtype == torch.bfloat16
    x, y, gs = _inputs(shape, kind, rounded)
    s64, g64, gmax, e_s, e_g = _reference(shape, kind, rounded)
    s, dx = _run(x, y, gs, dtype)
    assert s.shape == (shape[0],) and s.dtype == torch.float32 and dx.dtype == dtype and dx.shape == x.shape
    err_s = float((s.double().cpu() - s64).abs().max())
    diff = (dx.double().cpu() - g64).abs()
    allowed = _bound(e_g) * gmax + (2.0 ** -8 * g64.abs() if rounded else 0.0)
    err_g = float((diff / gmax).max())
    print('%s %s %s: ssim error %.3e (e %.3e, bound %.3e); gradient error / image max %.3e (e %.3e, bound %.3e%s)' % (
        shape, kind, 'bf16' if rounded else 'fp32', err_s, e_s, _bound(e_s), err_g, e_g, _bound(e_g), ' + 2^-8 |element|' if rounded else ''))
    assert err_s <= _bound(e_s), (err_s, e_s)
    assert bool((diff <= allowed).all()), (err_g, e_g, int((diff > allowed).sum()))           # every element


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_zero_incoming_gradient_gives_an_all_zero_image(dtype):
    x, y, _ = _inputs((3, 43, 70), 'smooth', dtype == torch.bfloat16)
    _, dx = _run(x, y, torch.tensor([0.0, 1.25, 0.0], dtype=torch.float64), dtype)
    assert bool((dx[0] == 0).all()) and bool((dx[2] == 0).all()) and float(dx[1].float().abs().max()) > 0


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('shape', [(2, 11, 11), (3, 43, 70)], ids=['2x11x11', '3x43x70'])
def test_identical_images_score_one_with_no_gradient(shape, dtype):
    x, _, gs = _inputs(shape, 'iid', dtype == torch.bfloat16)
    s, dx = _run(x, x.clone(), gs, dtype)
    assert float((s - 1).abs().max()) <= 1e-6 and float(dx.float().abs().max()) < 1e-6, (s, float(dx.float().abs().max()))


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('ab', [(0.25, 0.75), (0.9, 0.88)], ids=['0.25-0.75', '0.9-0.88'])
def test_constant_images_match_the_closed_form(ab, dtype):
    """u = a, v = b everywhere: every variance is 0 and S = (2ab + C1) / (a^2 + b^2 + C1) at every position."""
    for shape in ((2, 12, 17), (3, 43, 70)):
        x = torch.full(shape, 2 * ab[0] - 1).to(dtype).double()
        y = torch.full(shape, 2 * ab[1] - 1).to(dtype).double()
        a, b = (x[0, 0, 0] + 1) / 2, (y[0, 0, 0] + 1) / 2
        want = float((2 * a * b + R.C1) / (a * a + b * b + R.C1))
        e = float((R.ssim(x, y, torch.float32).double() - R.ssim(x, y)).abs().max())
        s, _ = _run(x, y, None, dtype, grad=False)
        err = float((s.double().cpu() - want).abs().max())
        print('%s constant %s: error %.3e (e %.3e, bound %.3e)' % (shape, ab, err, e, _bound(e)))
        assert err <= _bound(e), (shape, err, e)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_two_calls_give_the_same_bits(dtype):
    for shape, kind in (((3, 43, 70), 'iid'), ((2, 256, 256), 'smooth')):
        x, y, gs = _inputs(shape, kind, dtype == torch.bfloat16)
        s1, d1 = _run(x, y, gs, dtype)
        s2, d2 = _run(x, y, gs, dtype)
        assert torch.equal(_bits(s1), _bits(s2)) and torch.equal(_bits(d1), _bits(d2)), (shape, kind)


@pytest.mark.parametrize('shape', [(1, 640, 400), (2, 23, 31)], ids=['1x640x400', '2x23x31'])
def test_ssim_u8_matches_the_restatement(shape):
    from seg2eye_amd import ops
    n, H, W = shape
    gen = torch.Generator().manual_seed(7 * H + W)
    a = (F.avg_pool2d(torch.rand(n, 1, H + 4, W + 4, generator=gen), 5, 1)[:, 0] * 255).to(torch.uint8)
    b = (a.float() + 12 * torch.randn(n, H, W, generator=gen)).clamp(0, 255).to(torch.uint8)
    want = R.ssim_u8(a, b)
    e = float((R.ssim_u8(a, b, torch.float32).double() - want).abs().max())
    got = ops.ssim_u8(a.to(DEV).view(n, 1, H, W), b.to(DEV).view(n, 1, H, W))
    assert got.shape == (n,) and got.dtype == torch.float32 and not got.requires_grad
    err = float((got.double().cpu() - want).abs().max())
    print('%s uint8: ssim %s, error %.3e (e %.3e, bound %.3e)' % (shape, want.tolist(), err, e, _bound(e)))
    assert err <= _bound(e), (err, e)
    same = ops.ssim_u8(a.to(DEV), a.to(DEV))
    assert float((same - 1).abs().max()) <= 1e-6


def test_no_maps_are_kept_when_x_needs_no_gradient():
    """The three derivative maps are allocated and saved only for a backward through x: read off the Function's saved tensors."""
    from seg2eye_amd import ops
    x, y, _ = _inputs((2, 64, 64), 'iid', False)
    xd, yd = x.to(DEV, torch.float32), y.to(DEV, torch.float32)
    with_grad = ops.ssim(xd.clone().requires_grad_(True), yd)
    saved = with_grad.grad_fn.saved_tensors
    assert len(saved) == 3 and tuple(saved[2].shape) == (3, 2, 54, 54) and saved[2].dtype == torch.float32
    y_only = ops.ssim(xd, yd.clone().requires_grad_(True))                          # a node exists, but nothing for x to receive
    assert y_only.grad_fn is not None and y_only.grad_fn.saved_tensors == ()
    yg = yd.clone().requires_grad_(True)
    ops.ssim(xd, yg).sum().backward()
    assert yg.grad is None                                                          # no gradient for the target
    plain = ops.ssim(xd, yd)
    assert plain.grad_fn is None and torch.equal(plain, with_grad.detach()) and torch.equal(plain, y_only.detach())


# ------------------------------------------------------------------------------------------------ the generator's loss term
def test_generator_loss_term_matches_the_restatement_and_reaches_netG():
    """ngf = ndf = 8, batch 2, fp32, at 256 x 256 -- the one size the networks exist at (the encoder's FC head is sized for it, as in the
    reference, so a smaller model cannot be built): SSIM/weighted = 3 (1 - mean SSIM(fake, target)) of the fake the step returns, within the
    bound of the op test (times the weight); the backward runs and moves netG's gradient; without the flag the key does not exist."""
    res = {}
    for lam in (3.0, 0.0):
        tr = _trainer(lambda_ssim=lam)
        tr.run_generator_one_step(dict(_batch()))
        torch.cuda.synchronize()
        res[lam] = (tr.get_latest_losses(include_log_losses=True), tr.get_latest_generated().double().cpu(), tr.optimizer_G.flat_g.detach().double().cpu().clone())
    losses, fake, grad = res[3.0]
    assert 'SSIM/weighted' not in res[0.0][0] and 'SSIM/raw' not in res[0.0][0]
    assert set(losses) - set(res[0.0][0]) == {'SSIM/weighted', 'SSIM/raw'}
    assert tuple(losses['SSIM/weighted'].shape) == (1,) and tuple(fake.shape) == (2, 1, 256, 256)
    target = _batch()['target'].double()[:, 0]
    s64 = R.ssim(fake[:, 0], target)
    e = float((R.ssim(fake[:, 0], target, torch.float32).double() - s64).abs().max())
    want = 3.0 * (1.0 - float(s64.mean()))
    got = float(losses['SSIM/weighted'])
    print('SSIM/weighted %.8f, restatement %.8f (e %.3e, bound %.3e); SSIM/raw %.8f' % (got, want, e, 3 * _bound(e), float(losses['SSIM/raw'])))
    assert abs(got - want) <= 3 * _bound(e), (got, want, e)
    assert abs(float(losses['SSIM/raw']) - float(s64.mean())) <= _bound(e)
    assert bool(torch.isfinite(grad).all())
    # the two runs share weights and batch: without the term their gradients differ by float-atomics noise (~1e-6), with it by the term
    moved = float((grad - res[0.0][2]).norm() / res[0.0][2].norm())
    print('netG + netE gradient moved by %.3e of its norm' % moved)
    assert moved > 1e-3, moved


def test_hip_graph_replays_follow_the_eager_ssim_log():
    """Two iterations with hip_graphs on and off from the same state: the SSIM/raw logs agree within test_hip_graph_steps_match_eager's
    bounds (5e-4 on identical weights, 1e-2 once Adam steps have been taken), i.e. the launches capture and every replay scores anew."""
    res = {}
    for graphs in (False, True):
        tr = _trainer(lambda_ssim=2.0, hip_graphs=graphs)
        hist = []
        for it in range(2):
            tr.run_generator_one_step(dict(_batch()))
            tr.run_discriminator_one_step(dict(_batch()))
            hist.append({k: float(v.float().mean()) for k, v in tr.get_latest_losses(include_log_losses=True).items()})
        torch.cuda.synchronize()
        assert tr.use_graphs == graphs and (tr.graph_G is not None) == graphs       # (a failed capture would have fallen back to eager)
        res[graphs] = hist
        del tr
    for it, (a, b) in enumerate(zip(res[False], res[True])):
        assert 'SSIM/raw' in a and 'SSIM/weighted' in a and set(a) == set(b)
        for k in ('SSIM/raw', 'SSIM/weighted'):
            print(it, k, a[k], b[k])
            assert abs(a[k] - b[k]) <= (5e-4 if it == 0 else 1e-2) * max(1.0, abs(a[k])), (it, k, a[k], b[k])
        assert abs(a['SSIM/weighted'] - 2.0 * (1.0 - a['SSIM/raw'])) <= 1e-5
    assert res[True][0]['SSIM/raw'] != res[True][1]['SSIM/raw']                     # the second replay scored the stepped generator


# ------------------------------------------------------------------------------------------------ the Tester
def test_tester_scores_ssim_only_under_the_flag(tmp_path):
    from seg2eye_amd.options import parse
    from seg2eye_amd.pix2pix_model import Pix2PixModel
    from seg2eye_amd.tester import Tester
    argv = ['--name', 'ss', '--checkpoints_dir', str(tmp_path), '--dataset_key', 'validation', '--ngf', '8', '--crop_size', '256',
            '--aspect_ratio', '1.0', '--batchSize', '2', '--synthetic_size', '4', '--compute_dtype', 'fp32']
    opt = parse(argv, is_train=False)
    torch.manual_seed(0)
    Pix2PixModel(parse(argv)).save('latest')
    model = Pix2PixModel(opt)
    model.eval()
    plain = Tester(opt, dataset_key='validation')
    errs_plain, stats_plain = plain.run(model, mode='full', write_error_log=True)
    assert sorted(stats_plain) == ['mse/validation/full/relative'] and len(errs_plain) == 4          # today's key ...
    assert sorted(_load_log(plain)) == ['error', 'filename', 'user'] and plain.all_ssim == []       # ... and today's datasets

    tester = Tester(parse(argv + ['--val_ssim'], is_train=False), dataset_key='validation')
    seen, run_batch = [], tester.run_batch

    def recording(data_i, model):
        out = run_batch(data_i, model)
        assert len(out) == 4
        seen.append((out[2].cpu(), out[3].cpu()))
        return out
    tester.run_batch = recording
    errs, stats = tester.run(model, mode='full', write_error_log=True)
    assert sorted(stats) == ['mse/validation/full/relative', 'ssim/validation/full'] and len(seen) == 2
    np.testing.assert_allclose(np.asarray(errs), np.asarray(errs_plain), rtol=1e-6)
    assert stats['mse/validation/full/relative'] == pytest.approx(stats_plain['mse/validation/full/relative'], rel=1e-6)
    log = _load_log(tester)
    assert sorted(log) == ['error', 'filename', 'ssim', 'user'] and log['ssim'].dtype == np.float64 and log['ssim'].shape == (4,)
    produced, target = torch.cat([p for p, _ in seen])[:, 0], torch.cat([t for _, t in seen])[:, 0]
    assert produced.dtype == torch.uint8 and tuple(produced.shape) == (4, 640, 400) and tuple(target.shape) == (4, 640, 400)
    want = R.ssim_u8(produced, target)
    e = float((R.ssim_u8(produced, target, torch.float32).double() - want).abs().max())
    err = float(np.abs(log['ssim'] - want.numpy()).max())
    print('validation ssim %s; error %.3e (e %.3e, bound %.3e)' % (log['ssim'].tolist(), err, e, _bound(e)))
    assert err <= _bound(e), (err, e)
    assert abs(stats['ssim/validation/full'] - float(want.mean())) <= _bound(e)
    assert np.array_equal(log['ssim'], np.asarray(tester.all_ssim, dtype=np.float64))


# ------------------------------------------------------------------------------------------------ the table of the header
def _table():
    rows = []
    for shape, sid in zip(SHAPES, SHAPE_IDS):
        for kind in KINDS:
            _, _, _, e_s, e_g = _reference(shape, kind, False)
            rows.append('    %-12s %-8s %.1e    %.1e' % (sid, kind, e_s, e_g))
    return '\n'.join(rows)


if __name__ == '__main__':
    print(_table())
