"""MS-SSIM on the GPU: ops.ms_ssim / ops.ms_ssim_u8 and the backward against the fp64 restatement of tests/_msssim_ref.py
(whose gradient is autograd's), every element; the generator's --lambda_msssim term, eager and as hipGraph replays; the Tester under
--val_msssim.

Bounds come from the restatement, never from the kernel.  Per case, e is the error of the SAME restatement run in fp32 against fp64 on
the same inputs -- for the score and the per-level means the largest over the images, for the gradient the largest element divided by
its image's largest |gradient|.  The kernel must stay within max(4 e, 16 * 2^-24): 4 for another summation order, the floor a few fp32
ulps of a quantity of order 1.  A bf16 gradient element may be off by a further 2^-8 of its own magnitude (the output's rounding).  bf16
inputs are rounded first and the oracle sees the rounded values.  Where the oracle's gradient is exactly zero -- a pixel that only
clamped levels reach, an image whose every level is clamped -- the kernel's must be exactly zero too.

No case may sit at the floor's edge, where fp32 and fp64 could land on different sides: every per-level mean of every case is asserted
(from the fp64 restatement) to be >= 0.05 or <= -0.05.

e as measured (fp32 inputs; `python tests/test_msssim_gpu.py` prints the table, on any machine -- it needs no GPU):

    shape        L  kind     means (min .. max)     e(score)   e(gradient)
    2x22x22      2  copy      0.969 ..  0.993       2.5e-06    2.6e-05
    2x22x22      2  smooth    0.381 ..  0.811       1.2e-05    5.6e-05
    2x22x22      2  bright    0.982 ..  0.996       8.2e-05    4.4e-04
    2x22x22      2  split    -0.163 ..  0.965       1.3e-06    4.6e-05
    2x22x22      2  neg      -0.989 .. -0.954       8.6e-10    0.0e+00
    2x45x71      3  copy      0.984 ..  0.988       1.6e-06    3.1e-05
    2x45x71      3  smooth    0.392 ..  0.936       1.9e-05    7.4e-05
    2x45x71      3  bright    0.983 ..  0.999       5.7e-05    2.0e-04
    2x45x71      3  split    -0.204 ..  0.979       2.0e-06    1.0e-04
    2x45x71      3  neg      -0.989 .. -0.729       4.7e-11    0.0e+00
    2x108x172    2  copy      0.984 ..  0.985       4.4e-08    6.4e-06
    2x108x172    2  smooth    0.400 ..  0.765       3.9e-07    2.1e-05
    2x108x172    2  bright    0.982 ..  0.996       7.2e-06    2.7e-04
    2x108x172    2  split    -0.203 ..  0.959       1.2e-08    2.4e-05
    2x108x172    2  neg      -0.989 .. -0.947       8.6e-10    0.0e+00
    2x176x176    5  copy      0.985 ..  0.994       1.2e-05    1.7e-04
    2x176x176    5  smooth    0.399 ..  0.993       1.9e-05    9.7e-05
    2x176x176    5  bright    0.982 ..  1.000       7.3e-05    3.0e-04
    2x176x176    5  split    -0.189 ..  0.996       8.4e-06    1.3e-04
    2x176x176    5  neg      -0.989 ..  0.272       5.7e-08    2.7e-04
    1x177x191    5  copy      0.985 ..  0.995       4.4e-06    1.0e-04
    1x177x191    5  smooth    0.395 ..  0.992       5.5e-06    7.0e-05
    1x177x191    5  bright    0.982 ..  1.000       6.6e-05    2.1e-04
    1x177x191    5  split    -0.193 ..  0.993       1.1e-05    8.7e-05
    1x177x191    5  neg      -0.989 ..  0.208       3.2e-09    4.1e-05
    2x256x256    5  copy      0.985 ..  0.995       4.7e-07    5.4e-05
    2x256x256    5  smooth    0.395 ..  0.994       1.7e-06    3.6e-05
    2x256x256    5  bright    0.982 ..  1.000       4.9e-06    2.5e-04
    2x256x256    5  split    -0.197 ..  0.995       1.4e-06    4.4e-05
    2x256x256    5  neg      -0.989 ..  0.278       3.7e-08    8.0e-05

The kernels take their moments about each tile's first pixel at every level, so their own error does not grow on the bright-flat inputs
(measured on an MI355X in fp32: score within 1.3e-7 and per-level means within 3.7e-7 in every case; the gradient within 5.2e-6 of the
image's largest on copy, smooth, split and neg inputs, 4.3e-5 on bright-flat ones)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _msssim_ref as M
import _ssim_ref as R
from _quality_harness import PARENT_LOSS_KEYS, batch as _batch, load_log as _load_log, trainer as _trainer

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
# one position at the last level; odd sizes dropped at two levels; ragged tiles at both levels, halos crossing; the smallest five-level
# image; odd rows and columns dropped at several levels; the training size
CASES = [((2, 22, 22), 2), ((2, 45, 71), 3), ((2, 108, 172), 2), ((2, 176, 176), 5), ((1, 177, 191), 5), ((2, 256, 256), 5)]
CASE_IDS = ['%s-L%d' % ('x'.join(map(str, s)), L) for s, L in CASES]
KINDS = ['copy', 'smooth', 'bright', 'split', 'neg']
DTYPES = [torch.float32, torch.bfloat16]
DTYPE_IDS = ['fp32', 'bf16']
FLOOR = 16 * 2.0 ** -24
AWAY = 0.05                                                   # no per-level mean of a case within this of 0 (the clamp sits at 1e-3)


def _weights(levels):
    """The published five at five levels; fewer levels take their own (the first `levels` of a fixed list, not renormalised)."""
    return M.WEIGHTS if levels == 5 else (0.25, 0.35, 0.4, 0.3)[:levels]


# ------------------------------------------------------------------------------------------------ inputs and references (computed once)
@functools.lru_cache(maxsize=None)
def _inputs(shape, kind, rounded):
    """x, y (fp64 values of fp32 -- or, rounded, bf16 -- numbers) and a random incoming gradient per image; CPU, never written."""
    n, H, W = shape
    gen = torch.Generator().manual_seed(100000 * KINDS.index(kind) + 1000 * n + 31 * H + W)
    rnd = lambda *s: torch.rand(*s, generator=gen) * 2 - 1
    if kind == 'copy':                                        # iid noise and a noisy copy
        x = rnd(n, H, W)
        y = x + 0.1 * torch.randn(n, H, W, generator=gen)
    elif kind == 'smooth':                                    # a 9 x 9 box blur of iid noise; the target is a noisy copy
        x = F.avg_pool2d(rnd(n, 1, H + 8, W + 8), 9, 1)[:, 0]
        y = (x + 0.1 * torch.randn(n, H, W, generator=gen)).clamp(-1, 1)
    elif kind == 'bright':                                    # bright and flat: where E[u^2] - mu^2 cancels in fp32
        x = 0.9 + 0.01 * rnd(n, H, W)
        y = 0.88 + 0.01 * rnd(n, H, W)
    elif kind == 'split':                                     # fine detail inverted, coarse structure kept with noise: level 0 clamps, the others live
        r = rnd(n, H, W)
        up = lambda t: F.interpolate(t, scale_factor=2)[:, 0, :H, :W]
        lo = up(F.avg_pool2d(r.unsqueeze(1), 2, ceil_mode=True))
        blocky = up(rnd(n, 1, (H + 1) // 2, (W + 1) // 2))
        x = 0.5 * r
        y = 0.5 * (lo + 0.15 * blocky) - 0.25 * (r - lo)
    else:                                                     # 'neg': every covariance negative; only a last level of few pixels stays positive
        x = rnd(n, H, W)
        y = -x
    if rounded:
        x, y = x.bfloat16(), y.bfloat16()
    gs = torch.randn(n, generator=gen)
    return x.double(), y.double(), gs.double()


@functools.lru_cache(maxsize=None)
def _reference(shape, levels, kind, rounded):
    """(score64, terms64, grad64, image max |grad64|, e(score), e(terms), e(gradient / image max)) for one case."""
    x, y, gs = _inputs(shape, kind, rounded)
    w = _weights(levels)
    s64, t64, g64 = M.ms_ssim_and_grad(x, y, gs, w, torch.float64)
    s32, t32, g32 = M.ms_ssim_and_grad(x, y, gs, w, torch.float32)
    assert bool(((t64 >= AWAY) | (t64 <= -AWAY)).all()), ('a level mean at the floor\'s edge', shape, levels, kind, t64)
    gmax = g64.abs().amax(dim=(1, 2), keepdim=True)
    e_s = float((s32.double() - s64).abs().max())
    e_t = float((t32.double() - t64).abs().max())
    e_g = float(((g32.double() - g64).abs() / gmax.clamp(min=1e-300)).max())
    return s64, t64, g64, gmax, e_s, e_t, e_g


def _bound(e):
    return max(4 * e, FLOOR)


def _run(x, y, gs, dtype, weights, grad=True):
    from seg2eye_amd import ops
    n, H, W = x.shape
    xd = x.to(DEV, dtype).view(n, 1, H, W).requires_grad_(grad)
    s, terms = ops.ms_ssim(xd, y.to(DEV, dtype).view(n, 1, H, W), weights, return_terms=True)
    if grad:
        s.backward(gs.to(DEV, torch.float32))
    return s.detach(), terms, (xd.grad.view(n, H, W) if grad else None)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ------------------------------------------------------------------------------------------------ the op
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_forward_and_backward_match_the_restatement(case, kind, dtype):
    shape, levels = case
    rounded = dtype == torch.bfloat16
    x, y, gs = _inputs(shape, kind, rounded)
    s64, t64, g64, gmax, e_s, e_t, e_g = _reference(shape, levels, kind, rounded)
    s, terms, dx = _run(x, y, gs, dtype, _weights(levels))
    assert s.shape == (shape[0],) and s.dtype == torch.float32 and dx.dtype == dtype and dx.shape == x.shape
    assert terms.shape == (shape[0], levels) and terms.dtype == torch.float32 and not terms.requires_grad
    err_s = float((s.double().cpu() - s64).abs().max())
    err_t = float((terms.double().cpu() - t64).abs().max())
    got = dx.double().cpu()
    diff = (got - g64).abs()
    allowed = _bound(e_g) * gmax + (2.0 ** -8 * g64.abs() if rounded else 0.0)
    err_g = float((diff / gmax.clamp(min=1e-300)).max())
    print('%s L%d %s %s: score error %.3e (e %.3e, bound %.3e); means error %.3e (e %.3e, bound %.3e); gradient error / image max %.3e '
          '(e %.3e, bound %.3e%s); means %s' % (shape, levels, kind, 'bf16' if rounded else 'fp32', err_s, e_s, _bound(e_s), err_t, e_t, _bound(e_t),
                                                err_g, e_g, _bound(e_g), ' + 2^-8 |element|' if rounded else '', t64.tolist()))
    assert err_s <= _bound(e_s), (err_s, e_s)
    assert err_t <= _bound(e_t), (err_t, e_t)
    assert bool((diff <= allowed).all()), (err_g, e_g, int((diff > allowed).sum()))           # every element
    assert bool((got[g64 == 0] == 0).all()), int((got[g64 == 0] != 0).sum())                  # a clamped level is exactly absent
    clamped = t64 < M.FLOOR
    if kind == 'neg' and levels <= 3:
        assert bool(clamped.all()) and bool((got == 0).all()) and float(g64.abs().max()) == 0
    if kind == 'neg' and levels == 5:
        assert bool(clamped[:, :4].all()) and not bool(clamped[:, 4].any()) and float(gmax.min()) > 0
    if kind == 'split':
        assert bool(clamped[:, 0].all()) and not bool(clamped[:, 1:].any())
        if shape[1] % 2:                                      # the dropped last row and column belong to level 0 alone: nothing arrives
            assert bool((got[:, -1, :] == 0).all()) and bool((got[:, :, -1] == 0).all()) and float(got.abs().max()) > 0


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_zero_incoming_gradient_gives_an_all_zero_image(dtype):
    x, y, _ = _inputs((2, 176, 176), 'smooth', dtype == torch.bfloat16)
    _, _, dx = _run(x, y, torch.tensor([0.0, 1.25], dtype=torch.float64), dtype, None)
    assert bool((dx[0] == 0).all()) and float(dx[1].float().abs().max()) > 0
    x, y, _ = _inputs((2, 45, 71), 'copy', dtype == torch.bfloat16)
    _, _, dx = _run(x, y, torch.tensor([-0.5, 0.0], dtype=torch.float64), dtype, _weights(3))
    assert bool((dx[1] == 0).all()) and float(dx[0].float().abs().max()) > 0


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_two_calls_give_the_same_bits(dtype):
    for shape, levels, kind in (((2, 45, 71), 3, 'copy'), ((2, 256, 256), 5, 'smooth')):
        x, y, gs = _inputs(shape, kind, dtype == torch.bfloat16)
        s1, t1, d1 = _run(x, y, gs, dtype, _weights(levels))
        s2, t2, d2 = _run(x, y, gs, dtype, _weights(levels))
        assert torch.equal(_bits(s1), _bits(s2)) and torch.equal(_bits(t1), _bits(t2)) and torch.equal(_bits(d1), _bits(d2)), (shape, kind)


def test_identical_images_score_one_with_no_gradient():
    x, _, gs = _inputs((2, 176, 176), 'copy', False)
    s, terms, dx = _run(x, x.clone(), gs, torch.float32, None)
    assert float((s - 1).abs().max()) <= 1e-6 and float((terms - 1).abs().max()) <= 1e-6 and float(dx.abs().max()) < 1e-6


@pytest.mark.parametrize('shape,levels', [((1, 640, 400), 5), ((2, 45, 71), 3)], ids=['1x640x400-L5', '2x45x71-L3'])
def test_ms_ssim_u8_matches_the_restatement(shape, levels):
    from seg2eye_amd import ops
    n, H, W = shape
    w = None if levels == 5 else _weights(levels)
    gen = torch.Generator().manual_seed(7 * H + W)
    a = (F.avg_pool2d(torch.rand(n, 1, H + 4, W + 4, generator=gen), 5, 1)[:, 0] * 255).to(torch.uint8)
    b = (a.float() + 12 * torch.randn(n, H, W, generator=gen)).clamp(0, 255).to(torch.uint8)
    want, t64 = M.ms_ssim_u8(a, b, w, return_terms=True)
    assert bool((t64 >= AWAY).all()), t64
    s32, t32 = M.ms_ssim_u8(a, b, w, torch.float32, return_terms=True)
    e, e_t = float((s32.double() - want).abs().max()), float((t32.double() - t64).abs().max())
    got, terms = ops.ms_ssim_u8(a.to(DEV).view(n, 1, H, W), b.to(DEV).view(n, 1, H, W), w, return_terms=True)
    assert got.shape == (n,) and got.dtype == torch.float32 and not got.requires_grad and terms.shape == (n, levels)
    err, err_t = float((got.double().cpu() - want).abs().max()), float((terms.double().cpu() - t64).abs().max())
    print('%s uint8: msssim %s, error %.3e (e %.3e, bound %.3e); means error %.3e (e %.3e)' % (shape, want.tolist(), err, e, _bound(e), err_t, e_t))
    assert err <= _bound(e) and err_t <= _bound(e_t), (err, e, err_t, e_t)
    same = ops.ms_ssim_u8(a.to(DEV), a.to(DEV), w)
    assert float((same - 1).abs().max()) <= 1e-6


def test_one_level_with_weight_one_agrees_with_ssim():
    from seg2eye_amd import ops
    x, y, gs = _inputs((2, 108, 172), 'copy', False)
    s, terms, dx = _run(x, y, gs, torch.float32, [1.0])
    xd = x.to(DEV, torch.float32).requires_grad_(True)
    s1 = ops.ssim(xd, y.to(DEV, torch.float32))
    s1.backward(gs.to(DEV, torch.float32))
    assert float((s - s1.detach()).abs().max()) <= FLOOR and torch.equal(terms[:, 0], s)
    assert float((dx - xd.grad).abs().max()) <= FLOOR * float(xd.grad.abs().max())


def test_no_maps_or_gradient_buffers_are_kept_when_x_needs_no_gradient():
    """The pyramid, the maps and the coefficients are saved only for a backward through x: read off the Function's saved tensors."""
    from seg2eye_amd import _lib, ops
    x, y, _ = _inputs((2, 176, 176), 'copy', False)
    xd, yd = x.to(DEV, torch.float32), y.to(DEV, torch.float32)
    with_grad = ops.ms_ssim(xd.clone().requires_grad_(True), yd)
    saved = with_grad.grad_fn.saved_tensors
    assert len(saved) == 5
    assert saved[2].numel() * 4 == _lib.lib().s2e_msssim_pyramid_bytes(2, 176, 176, 5) and saved[3].numel() * 4 == _lib.lib().s2e_msssim_maps_bytes(2, 176, 176, 5)
    assert saved[3].dtype == torch.float32 and tuple(saved[4].shape) == (2, 5)
    y_only = ops.ms_ssim(xd, yd.clone().requires_grad_(True))                       # a node exists, but nothing for x to receive
    assert y_only.grad_fn is not None and y_only.grad_fn.saved_tensors == ()
    yg = yd.clone().requires_grad_(True)
    ops.ms_ssim(xd, yg).sum().backward()
    assert yg.grad is None                                                          # no gradient for the target
    plain = ops.ms_ssim(xd, yd)
    assert plain.grad_fn is None and torch.equal(plain, with_grad.detach()) and torch.equal(plain, y_only.detach())
    assert torch.equal(ops.ms_ssim_terms(xd, yd), ops.ms_ssim(xd, yd, return_terms=True)[1])


def test_the_op_refuses_what_the_library_refuses():
    from seg2eye_amd import _lib, ops
    x = torch.zeros(1, 1, 175, 256, device=DEV)
    with pytest.raises(_lib.Seg2EyeHipError, match=r'level 4 is 10 x 16'):
        ops.ms_ssim(x, x)
    with pytest.raises(_lib.Seg2EyeHipError, match=r'weights\[1\]=-1'):
        ops.ms_ssim(x, x, [0.5, -1.0])
    with pytest.raises(ValueError, match='1 to 5 level weights'):
        ops.ms_ssim(x, x, [0.1] * 6)


# ------------------------------------------------------------------------------------------------ the generator's loss term
def test_generator_loss_term_matches_the_restatement_and_reaches_netG():
    """ngf = ndf = 8, batch 2, fp32, at 256 x 256: MSSSIM/weighted = 3 (1 - mean MS-SSIM(fake, target)) of the fake the step returns, within
    the bound of the op test (times the weight); the backward runs and moves netG's gradient; without the flag the keys do not exist and
    the step's losses are the parent commit's."""
    res = {}
    for lam in (3.0, 0.0):
        tr = _trainer(lambda_msssim=lam)
        tr.run_generator_one_step(dict(_batch()))
        torch.cuda.synchronize()
        fake, grad = tr.get_latest_generated().double().cpu(), tr.optimizer_G.flat_g.detach().double().cpu().clone()
        g_losses = dict(tr.get_latest_losses(include_log_losses=True))
        tr.run_discriminator_one_step(dict(_batch()))
        torch.cuda.synchronize()
        res[lam] = (g_losses, fake, grad, set(tr.get_latest_losses(include_log_losses=True)))
    losses, fake, grad, _ = res[3.0]
    # (after the D step: the log entry MSSSIM/raw was read, and so consumed, after the G step)
    assert res[0.0][3] == PARENT_LOSS_KEYS and res[3.0][3] == PARENT_LOSS_KEYS | {'MSSSIM/weighted'}
    assert set(losses) - set(res[0.0][0]) == {'MSSSIM/weighted', 'MSSSIM/raw'}
    assert tuple(losses['MSSSIM/weighted'].shape) == (1,) and tuple(fake.shape) == (2, 1, 256, 256)
    target = _batch()['target'].double()[:, 0]
    s64, t64 = M.ms_ssim(fake[:, 0], target, return_terms=True)
    e = float((M.ms_ssim(fake[:, 0], target, dtype=torch.float32).double() - s64).abs().max())
    want = 3.0 * (1.0 - float(s64.mean()))
    got = float(losses['MSSSIM/weighted'])
    print('MSSSIM/weighted %.8f, restatement %.8f (e %.3e, bound %.3e); MSSSIM/raw %.8f; level means %s' % (
        got, want, e, 3 * _bound(e), float(losses['MSSSIM/raw']), t64.tolist()))
    assert abs(got - want) <= 3 * _bound(e), (got, want, e)
    assert abs(float(losses['MSSSIM/raw']) - float(s64.mean())) <= _bound(e)
    assert bool(torch.isfinite(grad).all())
    # the two runs share weights and batch: without the term their gradients differ by float-atomics noise (~1e-6), with it by the term
    moved = float((grad - res[0.0][2]).norm() / res[0.0][2].norm())
    print('netG + netE gradient moved by %.3e of its norm' % moved)
    assert moved > 1e-3, moved


def test_hip_graph_replays_follow_the_eager_msssim_log():
    """Two iterations with hip_graphs on and off from the same state, --lambda_msssim and --lambda_ssim together: the logs agree within
    test_hip_graph_steps_match_eager's bounds (5e-4 on identical weights, 1e-2 once Adam steps have been taken), i.e. the launches
    capture and every replay scores anew."""
    res = {}
    for graphs in (False, True):
        tr = _trainer(lambda_msssim=2.0, lambda_ssim=1.0, hip_graphs=graphs)
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
        assert set(a) == set(b) == PARENT_LOSS_KEYS | {'MSSSIM/raw', 'MSSSIM/weighted', 'SSIM/raw', 'SSIM/weighted'}
        for k in ('MSSSIM/raw', 'MSSSIM/weighted', 'SSIM/raw'):
            print(it, k, a[k], b[k])
            assert abs(a[k] - b[k]) <= (5e-4 if it == 0 else 1e-2) * max(1.0, abs(a[k])), (it, k, a[k], b[k])
        assert abs(a['MSSSIM/weighted'] - 2.0 * (1.0 - a['MSSSIM/raw'])) <= 1e-5
    assert res[True][0]['MSSSIM/raw'] != res[True][1]['MSSSIM/raw']                 # the second replay scored the stepped generator


# ------------------------------------------------------------------------------------------------ the Tester
def test_tester_scores_msssim_only_under_the_flag(tmp_path):
    from seg2eye_amd.options import parse
    from seg2eye_amd.pix2pix_model import Pix2PixModel
    from seg2eye_amd.tester import Tester
    argv = ['--name', 'ms', '--checkpoints_dir', str(tmp_path), '--dataset_key', 'validation', '--ngf', '8', '--crop_size', '256',
            '--aspect_ratio', '1.0', '--batchSize', '2', '--synthetic_size', '4', '--compute_dtype', 'fp32']
    opt = parse(argv, is_train=False)
    torch.manual_seed(0)
    Pix2PixModel(parse(argv)).save('latest')
    model = Pix2PixModel(opt)
    model.eval()
    plain = Tester(opt, dataset_key='validation')
    errs_plain, stats_plain = plain.run(model, mode='full', write_error_log=True)
    assert sorted(stats_plain) == ['mse/validation/full/relative'] and len(errs_plain) == 4          # the parent commit's key ...
    assert sorted(_load_log(plain)) == ['error', 'filename', 'user'] and plain.all_msssim == []      # ... and its datasets

    tester = Tester(parse(argv + ['--val_msssim', '--val_ssim'], is_train=False), dataset_key='validation')
    seen, run_batch = [], tester.run_batch

    def recording(data_i, model):
        out = run_batch(data_i, model)
        assert len(out) == 4
        seen.append((out[2].cpu(), out[3].cpu()))
        return out
    tester.run_batch = recording
    errs, stats = tester.run(model, mode='full', write_error_log=True)
    assert sorted(stats) == ['mse/validation/full/relative', 'msssim/validation/full', 'ssim/validation/full'] and len(seen) == 2
    np.testing.assert_allclose(np.asarray(errs), np.asarray(errs_plain), rtol=1e-6)
    assert stats['mse/validation/full/relative'] == pytest.approx(stats_plain['mse/validation/full/relative'], rel=1e-6)
    log = _load_log(tester)
    assert sorted(log) == ['error', 'filename', 'msssim', 'ssim', 'user'] and log['msssim'].dtype == np.float64 and log['msssim'].shape == (4,)
    produced, target = torch.cat([p for p, _ in seen])[:, 0], torch.cat([t for _, t in seen])[:, 0]
    assert produced.dtype == torch.uint8 and tuple(produced.shape) == (4, 640, 400) and tuple(target.shape) == (4, 640, 400)
    want = M.ms_ssim_u8(produced, target)
    e = float((M.ms_ssim_u8(produced, target, dtype=torch.float32).double() - want).abs().max())
    err = float(np.abs(log['msssim'] - want.numpy()).max())
    print('validation msssim %s; error %.3e (e %.3e, bound %.3e)' % (log['msssim'].tolist(), err, e, _bound(e)))
    assert err <= _bound(e), (err, e)
    assert abs(stats['msssim/validation/full'] - float(want.mean())) <= _bound(e)
    assert np.array_equal(log['msssim'], np.asarray(tester.all_msssim, dtype=np.float64))
    assert abs(stats['ssim/validation/full'] - float(R.ssim_u8(produced, target).mean())) <= 1e-4


# ------------------------------------------------------------------------------------------------ the table of the header
def _table():
    rows = []
    for (shape, levels), cid in zip(CASES, CASE_IDS):
        for kind in KINDS:
            _, t64, _, _, e_s, _, e_g = _reference(shape, levels, kind, False)
            rows.append('    %-12s %d  %-8s %6.3f .. %6.3f       %.1e    %.1e' % (cid.split('-')[0], levels, kind, float(t64.min()), float(t64.max()), e_s, e_g))
    return '\n'.join(rows)


if __name__ == '__main__':
    print(_table())
