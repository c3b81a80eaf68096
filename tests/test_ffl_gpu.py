"""The focal frequency loss on the GPU: ops.focal_freq_loss / ops.focal_freq_loss_u8 and the backward against the fp64
restatement of tests/_ffl_ref.py (torch.fft.fft2 on the full spectrum, autograd's gradient), every element; the DFT tables; the generator's
--lambda_ffl term, eager and as hipGraph replays; the Tester under --val_ffl.

Bounds come from the restatement, never from the kernel.  Per case, e is the error against fp64 of the SAME rule as two real matrix
products in fp32 with fp32 DFT matrices (the yardstick) on the same inputs -- for the loss the largest over the images of the error relative
to the image's own fp64 loss, for the gradient the largest element divided by its image's largest |gradient|.  The kernel must stay within
max(4 e, 16 * 2^-24): 4 for another summation order, the floor a few fp32 ulps of a quantity of order 1.  A bf16 gradient element may be off
by a further 2^-8 of its own magnitude (the output's rounding).  bf16 inputs are rounded first and the oracle sees the rounded values.

Kinds: `noise` independent images; `copy` iid x, y = x + 0.1 noise; `smooth` a 9 x 9 box blur of noise and a noisy copy; `offset`
y = 0.9 x - 0.3 + 0.01 noise, so the DC bin dominates the maximum; `tone` x - y is one cosine plus 1 % noise, so two bins carry nearly all
the weight.

e as measured (fp32 inputs; `python tests/test_ffl_gpu.py` prints the table, on any machine -- it needs no GPU):

    shape      alpha  kind     ffl (min .. max)         e(loss)    e(gradient)
    2x16x16    0      noise    6.256e-01 .. 6.279e-01   1.4e-07    2.0e-07
    2x16x16    0      copy     8.429e-03 .. 1.156e-02   4.5e-08    1.5e-07
    2x16x16    0      smooth   9.289e-03 .. 9.607e-03   1.2e-07    1.7e-07
    2x16x16    0      offset   9.232e-02 .. 9.579e-02   2.6e-07    4.1e-07
    2x16x16    0      tone     1.248e-01 .. 1.251e-01   9.9e-08    4.0e-07
    2x16x16    1      noise    3.228e-01 .. 3.541e-01   3.0e-08    2.8e-07
    2x16x16    1      copy     4.613e-03 .. 6.717e-03   1.2e-07    2.4e-07
    2x16x16    1      smooth   4.784e-03 .. 5.526e-03   9.3e-08    1.9e-07
    2x16x16    1      offset   8.862e-02 .. 9.221e-02   1.1e-07    4.3e-07
    2x16x16    1      tone     1.247e-01 .. 1.251e-01   1.9e-07    2.3e-07
    2x17x23    0      noise    6.704e-01 .. 6.771e-01   6.1e-08    2.5e-07
    2x17x23    0      copy     1.002e-02 .. 1.060e-02   6.6e-08    2.3e-07
    2x17x23    0      smooth   1.030e-02 .. 1.075e-02   8.1e-08    2.0e-07
    2x17x23    0      offset   9.519e-02 .. 9.525e-02   3.3e-07    5.3e-07
    2x17x23    0      tone     1.249e-01 .. 1.252e-01   5.6e-08    4.0e-07
    2x17x23    1      noise    3.119e-01 .. 3.342e-01   5.1e-08    2.1e-07
    2x17x23    1      copy     5.181e-03 .. 5.705e-03   6.9e-08    2.4e-07
    2x17x23    1      smooth   5.638e-03 .. 6.336e-03   1.6e-07    3.2e-07
    2x17x23    1      offset   9.189e-02 .. 9.200e-02   3.7e-07    6.6e-07
    2x17x23    1      tone     1.249e-01 .. 1.252e-01   6.6e-08    2.7e-07
    1x18x40    0      noise    6.476e-01 .. 6.476e-01   5.2e-08    2.3e-07
    1x18x40    0      copy     1.068e-02 .. 1.068e-02   4.6e-08    2.4e-07
    1x18x40    0      smooth   1.037e-02 .. 1.037e-02   4.1e-08    2.1e-07
    1x18x40    0      offset   9.390e-02 .. 9.390e-02   4.5e-07    6.5e-07
    1x18x40    0      tone     1.249e-01 .. 1.249e-01   1.2e-07    4.9e-07
    1x18x40    1      noise    3.414e-01 .. 3.414e-01   3.8e-08    2.4e-07
    1x18x40    1      copy     5.603e-03 .. 5.603e-03   1.1e-07    2.8e-07
    1x18x40    1      smooth   5.617e-03 .. 5.617e-03   1.8e-07    3.1e-07
    1x18x40    1      offset   9.054e-02 .. 9.054e-02   2.8e-07    7.5e-07
    1x18x40    1      tone     1.249e-01 .. 1.249e-01   1.4e-07    3.7e-07
    2x45x71    0      noise    6.471e-01 .. 6.597e-01   1.2e-07    4.4e-07
    2x45x71    0      copy     1.001e-02 .. 1.012e-02   1.0e-07    2.8e-07
    2x45x71    0      smooth   1.040e-02 .. 1.054e-02   1.0e-07    3.7e-07
    2x45x71    0      offset   9.309e-02 .. 9.455e-02   2.0e-07    1.1e-06
    2x45x71    0      tone     1.250e-01 .. 1.251e-01   6.8e-08    7.9e-07
    2x45x71    1      noise    2.924e-01 .. 3.262e-01   8.1e-08    4.6e-07
    2x45x71    1      copy     4.435e-03 .. 5.316e-03   9.5e-08    4.3e-07
    2x45x71    1      smooth   4.962e-03 .. 5.121e-03   8.0e-08    3.6e-07
    2x45x71    1      offset   8.976e-02 .. 9.115e-02   1.3e-07    1.5e-06
    2x45x71    1      tone     1.250e-01 .. 1.251e-01   7.7e-08    7.0e-07
    1x64x48    0      noise    6.920e-01 .. 6.920e-01   7.1e-10    4.1e-07
    1x64x48    0      copy     9.776e-03 .. 9.776e-03   1.3e-08    1.9e-07
    1x64x48    0      smooth   1.040e-02 .. 1.040e-02   4.2e-08    2.5e-07
    1x64x48    0      offset   9.298e-02 .. 9.298e-02   3.5e-07    8.7e-07
    1x64x48    0      tone     1.250e-01 .. 1.250e-01   7.5e-09    7.7e-07
    1x64x48    1      noise    3.241e-01 .. 3.241e-01   1.7e-07    4.3e-07
    1x64x48    1      copy     4.988e-03 .. 4.988e-03   3.7e-08    2.4e-07
    1x64x48    1      smooth   5.205e-03 .. 5.205e-03   9.3e-08    4.4e-07
    1x64x48    1      offset   8.959e-02 .. 8.959e-02   4.3e-07    1.4e-06
    1x64x48    1      tone     1.249e-01 .. 1.249e-01   4.9e-09    7.5e-07
    2x256x256  0      noise    6.655e-01 .. 6.674e-01   9.1e-08    1.1e-06
    2x256x256  0      copy     9.966e-03 .. 1.006e-02   9.4e-08    6.8e-07
    2x256x256  0      smooth   9.932e-03 .. 1.001e-02   1.2e-07    5.9e-07
    2x256x256  0      offset   9.348e-02 .. 9.353e-02   2.9e-07    3.6e-06
    2x256x256  0      tone     1.250e-01 .. 1.250e-01   4.8e-07    2.1e-06
    2x256x256  1      noise    2.726e-01 .. 2.735e-01   8.8e-08    8.0e-07
    2x256x256  1      copy     3.790e-03 .. 3.819e-03   1.8e-07    6.8e-07
    2x256x256  1      smooth   3.803e-03 .. 4.210e-03   2.6e-07    7.8e-07
    2x256x256  1      offset   9.008e-02 .. 9.010e-02   1.6e-07    4.8e-06
    2x256x256  1      tone     1.250e-01 .. 1.250e-01   4.8e-07    1.3e-06
    2x45x71    2      noise    1.500e-01 .. 1.823e-01   6.1e-08    4.3e-07
    2x45x71    2      copy     2.210e-03 .. 3.192e-03   1.9e-07    4.3e-07
    2x45x71    2      smooth   2.676e-03 .. 2.826e-03   3.6e-08    4.1e-07
    2x45x71    2      offset   8.975e-02 .. 9.114e-02   8.5e-08    1.5e-06
    2x45x71    2      tone     1.250e-01 .. 1.251e-01   1.0e-07    1.5e-07
    2x45x71    1.5    noise    2.066e-01 .. 2.406e-01   4.1e-08    4.8e-07
    2x45x71    1.5    copy     3.086e-03 .. 4.065e-03   7.3e-08    4.4e-07
    2x45x71    1.5    smooth   3.595e-03 .. 3.751e-03   1.3e-07    4.0e-07
    2x45x71    1.5    offset   8.975e-02 .. 9.114e-02   2.5e-07    1.4e-06
    2x45x71    1.5    tone     1.250e-01 .. 1.251e-01   1.1e-07    3.4e-07

The kernels split K over four accumulator sets per wave, so their own error stays at the yardstick's (measured on an MI355X, largest over
the shapes and alpha: loss within 3.1e-7 of the image's loss on fp32 inputs and 3.3e-7 on bf16 ones in every kind; the fp32 gradient within
6.8e-7 (noise), 4.5e-7 (copy), 4.4e-7 (smooth), 2.2e-6 (offset) and 1.4e-6 (tone) of the image's largest)."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _ffl_ref as R
from _quality_harness import PARENT_LOSS_KEYS, batch as _batch, load_log as _load_log, trainer as _trainer

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
# one full tile; both odd (no Nyquist column, ragged tiles); even W (a Nyquist column), H no tile multiple; several ragged tiles;
# portrait, several full tiles; the training size
SHAPES = [(2, 16, 16), (2, 17, 23), (1, 18, 40), (2, 45, 71), (1, 64, 48), (2, 256, 256)]
KINDS = ['noise', 'copy', 'smooth', 'offset', 'tone']
CASES = [(s, a) for s in SHAPES for a in (0.0, 1.0)] + [((2, 45, 71), 2.0), ((2, 45, 71), 1.5)]
CASE_IDS = ['%s-a%g' % ('x'.join(map(str, s)), a) for s, a in CASES]
DTYPES = [torch.float32, torch.bfloat16]
DTYPE_IDS = ['fp32', 'bf16']
FLOOR = 16 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ inputs and references (computed once)
@functools.lru_cache(maxsize=None)
def _inputs(shape, kind, rounded):
    """x, y (fp64 values of fp32 -- or, rounded, bf16 -- numbers) and a random incoming gradient per image; CPU, never written."""
    n, H, W = shape
    gen = torch.Generator().manual_seed(100000 * KINDS.index(kind) + 1000 * n + 31 * H + W)
    rnd = lambda *s: torch.rand(*s, generator=gen) * 2 - 1
    if kind == 'noise':
        x, y = rnd(n, H, W), rnd(n, H, W)
    elif kind == 'copy':
        x = rnd(n, H, W)
        y = x + 0.1 * torch.randn(n, H, W, generator=gen)
    elif kind == 'smooth':
        x = F.avg_pool2d(rnd(n, 1, H + 8, W + 8), 9, 1)[:, 0]
        y = (x + 0.1 * torch.randn(n, H, W, generator=gen)).clamp(-1, 1)
    elif kind == 'offset':
        x = rnd(n, H, W)
        y = 0.9 * x - 0.3 + 0.01 * torch.randn(n, H, W, generator=gen)
    else:                                                     # 'tone': bin (3, 2) and its mirror
        x = rnd(n, H, W)
        r, c = torch.arange(H, dtype=torch.float32)[:, None], torch.arange(W, dtype=torch.float32)[None, :]
        y = x - 0.5 * torch.cos(2 * math.pi * (3 * r / H + 2 * c / W)) - 0.005 * torch.randn(n, H, W, generator=gen)
    if rounded:
        x, y = x.bfloat16(), y.bfloat16()
    gs = torch.randn(n, generator=gen)
    return x.double(), y.double(), gs.double()


@functools.lru_cache(maxsize=None)
def _reference(shape, alpha, kind, rounded):
    """(ffl64, grad64, image max |grad64|, e(loss), e(gradient / image max)) for one case."""
    x, y, gs = _inputs(shape, kind, rounded)
    f64, g64 = R.oracle(x, y, gs, alpha)
    f32, g32 = R.yardstick(x, y, gs, alpha)
    assert float(f64.min()) > 0
    gmax = g64.abs().amax(dim=(1, 2), keepdim=True)
    e_f = float(((f32.double() - f64).abs() / f64).max())
    e_g = float(((g32.double() - g64).abs() / gmax).max())
    return f64, g64, gmax, e_f, e_g


def _bound(e):
    return max(4 * e, FLOOR)


def _run(x, y, gs, dtype, alpha, grad=True):
    from seg2eye_amd import ops
    n, H, W = x.shape
    xd = x.to(DEV, dtype).view(n, 1, H, W).requires_grad_(grad)
    f = ops.focal_freq_loss(xd, y.to(DEV, dtype).view(n, 1, H, W), alpha)
    if grad:
        f.backward(gs.to(DEV, torch.float32))
    return f.detach(), (xd.grad.view(n, H, W) if grad else None)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ------------------------------------------------------------------------------------------------ the tables
@pytest.mark.parametrize('hw', [(16, 16), (17, 23), (18, 40), (45, 71), (256, 256), (640, 400)], ids=lambda s: '%dx%d' % s)
def test_tables_are_the_fp64_values_rounded_to_fp32(hw):
    """Within 1 fp32 ulp of the host's fp64 value rounded to fp32, not always bit-equal: neither side's fp64 cosine is correctly rounded (both are
    within an ulp or two of fp64), so the two fp32 roundings can differ where the value sits within ~1e-16 of a rounding boundary; and at
    the quarter turns the device's sincospi gives an exact 0 where the host's cos(2 pi j / n) of a rounded argument gives ~1e-17 -- the
    absolute allowance 2^-50.  (Measured: every entry of these six sizes within 0.5 ulp of the host's fp64 value, so bit-equal to its rounding
    everywhere but at those zeros.)  The padding is exactly zero, and the transposed W table carries the multiplicities."""
    from seg2eye_amd import ops
    H, W = hw
    up = lambda v, m: (v + m - 1) // m * m
    Hp, Wp, Wh, Whp = up(H, 64), up(W, 64), W // 2 + 1, up(W // 2 + 1, 32)
    t = ops.ffl_tables(H, W, DEV)
    assert t.dtype == torch.float32 and t.numel() == 2 * Hp * Hp + 4 * Wp * Whp and ops.ffl_tables(H, W, DEV) is t      # cached per size
    t = t.cpu()
    ch, sh = t[:Hp * Hp].view(Hp, Hp), t[Hp * Hp:2 * Hp * Hp].view(Hp, Hp)
    tw = t[2 * Hp * Hp:2 * Hp * Hp + 2 * Wp * Whp].view(Wp, 2 * Whp)
    twt = t[2 * Hp * Hp + 2 * Wp * Whp:].view(2 * Whp, Wp)
    c64, s64 = R.dft_matrices(H)
    cw64, sw64 = R.dft_matrices(W)
    m = R.multiplicities(W)
    worst, differ = 0.0, 0
    for got, want in ((ch[:H, :H], c64), (sh[:H, :H], s64), (tw[:W, :Wh], cw64[:, :Wh]), (tw[:W, Whp:Whp + Wh], sw64[:, :Wh]),
                      (twt[:Wh, :W], (cw64[:, :Wh] * m).t()), (twt[Whp:Whp + Wh, :W], (sw64[:, :Wh] * m).t())):
        w32 = want.float()
        ulp = (torch.nextafter(w32.abs(), torch.tensor(float('inf'))) - w32.abs()).double()
        diff = (got.double() - want).abs()
        assert bool((diff <= torch.clamp(ulp, min=2.0 ** -50)).all()), float((diff / ulp).max())
        worst = max(worst, float((diff / torch.clamp(ulp, min=2.0 ** -50)).max()))
        differ += int((got != w32).sum())
    print('%dx%d tables: %d of %d entries differ from the host rounding; worst %.3f ulp' % (H, W, differ, 2 * H * H + 4 * W * Wh, worst))
    for full, live in ((ch, (H, H)), (sh, (H, H))):
        pad = full.clone()
        pad[:live[0], :live[1]] = 0
        assert bool((pad == 0).all())
    pad = tw.clone()
    pad[:W, :Wh] = 0
    pad[:W, Whp:Whp + Wh] = 0
    assert bool((pad == 0).all())
    pad = twt.clone()
    pad[:Wh, :W] = 0
    pad[Whp:Whp + Wh, :W] = 0
    assert bool((pad == 0).all())


# ------------------------------------------------------------------------------------------------ the op
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_forward_and_backward_match_the_restatement(case, kind, dtype):
    shape, alpha = case
    rounded = dtype == torch.bfloat16
    x, y, gs = _inputs(shape, kind, rounded)
    f64, g64, gmax, e_f, e_g = _reference(shape, alpha, kind, rounded)
    f, dx = _run(x, y, gs, dtype, alpha)
    assert f.shape == (shape[0],) and f.dtype == torch.float32 and dx.dtype == dtype and dx.shape == x.shape
    err_f = float(((f.double().cpu() - f64).abs() / f64).max())
    got = dx.double().cpu()
    diff = (got - g64).abs()
    allowed = _bound(e_g) * gmax + (2.0 ** -8 * g64.abs() if rounded else 0.0)
    err_g = float((diff / gmax).max())
    print('%s alpha %g %s %s: loss %s, relative error %.3e (e %.3e, bound %.3e); gradient error / image max %.3e (e %.3e, bound %.3e%s)' % (
        shape, alpha, kind, 'bf16' if rounded else 'fp32', f64.tolist(), err_f, e_f, _bound(e_f), err_g, e_g, _bound(e_g),
        ' + 2^-8 |element|' if rounded else ''))
    assert err_f <= _bound(e_f), (err_f, e_f)
    assert bool((diff <= allowed).all()), (err_g, e_g, int((diff > allowed).sum()))           # every element


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_alpha_zero_is_the_mean_squared_error(shape, dtype):
    """Parseval on the GPU: ffl at alpha = 0 against mean((x - y)^2) in fp64 of the same (rounded) inputs, within the bound of the op test."""
    rounded = dtype == torch.bfloat16
    x, y, gs = _inputs(shape, 'noise', rounded)
    _, _, _, e_f, _ = _reference(shape, 0.0, 'noise', rounded)
    f, _ = _run(x, y, gs, dtype, 0.0, grad=False)
    mse = ((x - y) ** 2).mean(dim=(1, 2))
    err = float(((f.double().cpu() - mse) / mse).abs().max())
    print('%s %s: Parseval relative error %.3e (bound %.3e)' % (shape, 'bf16' if rounded else 'fp32', err, _bound(e_f)))
    assert err <= _bound(e_f), (err, e_f)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_identical_images_give_exact_zeros(dtype):
    for shape, alpha in (((2, 45, 71), 1.0), ((2, 45, 71), 0.0), ((2, 45, 71), 1.5), ((2, 256, 256), 1.0), ((1, 18, 40), 2.0)):
        x, _, gs = _inputs(shape, 'noise', dtype == torch.bfloat16)
        f, dx = _run(x, x.clone(), gs, dtype, alpha)
        assert bool((f == 0).all()) and bool((dx == 0).all()), (shape, alpha)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_zero_incoming_gradient_gives_an_all_zero_image(dtype):
    x, y, _ = _inputs((2, 45, 71), 'smooth', dtype == torch.bfloat16)
    _, dx = _run(x, y, torch.tensor([0.0, 1.25], dtype=torch.float64), dtype, 1.0)
    assert bool((dx[0] == 0).all()) and float(dx[1].float().abs().max()) > 0
    x, y, _ = _inputs((2, 256, 256), 'copy', dtype == torch.bfloat16)
    _, dx = _run(x, y, torch.tensor([-0.5, 0.0], dtype=torch.float64), dtype, 1.5)
    assert bool((dx[1] == 0).all()) and float(dx[0].float().abs().max()) > 0


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_two_calls_give_the_same_bits(dtype):
    for shape, alpha, kind in (((2, 45, 71), 1.5, 'copy'), ((2, 256, 256), 1.0, 'smooth'), ((1, 18, 40), 0.0, 'tone')):
        x, y, gs = _inputs(shape, kind, dtype == torch.bfloat16)
        f1, d1 = _run(x, y, gs, dtype, alpha)
        f2, d2 = _run(x, y, gs, dtype, alpha)
        assert torch.equal(_bits(f1), _bits(f2)) and torch.equal(_bits(d1), _bits(d2)), (shape, kind)


def test_the_loss_is_symmetric_in_its_images():
    """d -> -d negates every product exactly: the same bits."""
    from seg2eye_amd import ops
    x, y, _ = _inputs((2, 45, 71), 'copy', False)
    xd, yd = x.to(DEV, torch.float32), y.to(DEV, torch.float32)
    for alpha in (0.0, 1.0, 1.5):
        assert torch.equal(ops.focal_freq_loss(xd, yd, alpha), ops.focal_freq_loss(yd, xd, alpha)), alpha


@pytest.mark.parametrize('shape', [(1, 640, 400), (2, 45, 71)], ids=['1x640x400', '2x45x71'])
def test_focal_freq_loss_u8_matches_the_restatement(shape):
    from seg2eye_amd import ops
    n, H, W = shape
    gen = torch.Generator().manual_seed(7 * H + W)
    a = (F.avg_pool2d(torch.rand(n, 1, H + 4, W + 4, generator=gen), 5, 1)[:, 0] * 255).to(torch.uint8)
    b = (a.float() + 12 * torch.randn(n, H, W, generator=gen)).clamp(0, 255).to(torch.uint8)
    for alpha in (1.0, 0.0):
        want = R.ffl_u8(a, b, alpha)
        e = float(((R.ffl_u8(a, b, alpha, torch.float32, 'matrix').double() - want).abs() / want).max())
        got = ops.focal_freq_loss_u8(a.to(DEV).view(n, 1, H, W), b.to(DEV).view(n, 1, H, W), alpha)
        assert got.shape == (n,) and got.dtype == torch.float32 and not got.requires_grad
        err = float(((got.double().cpu() - want).abs() / want).max())
        print('%s uint8 alpha %g: ffl %s, relative error %.3e (e %.3e, bound %.3e)' % (shape, alpha, want.tolist(), err, e, _bound(e)))
        assert err <= _bound(e), (err, e)
    assert bool((ops.focal_freq_loss_u8(a.to(DEV), a.to(DEV)) == 0).all())


def test_no_spectrum_is_kept_when_x_needs_no_gradient():
    """The spectrum and the coefficients are saved only for a backward through x: read off the Function's saved tensors."""
    from seg2eye_amd import _lib, ops
    x, y, _ = _inputs((2, 45, 71), 'copy', False)
    xd, yd = x.to(DEV, torch.float32), y.to(DEV, torch.float32)
    with_grad = ops.focal_freq_loss(xd.clone().requires_grad_(True), yd)
    saved = with_grad.grad_fn.saved_tensors
    assert len(saved) == 3 and saved[0].numel() * 4 == _lib.lib().s2e_ffl_spectrum_bytes(2, 45, 71) and tuple(saved[1].shape) == (2,)
    assert saved[2] is ops.ffl_tables(45, 71, DEV) or saved[2].data_ptr() == ops.ffl_tables(45, 71, DEV).data_ptr()
    y_only = ops.focal_freq_loss(xd, yd.clone().requires_grad_(True))               # a node exists, but nothing for x to receive
    assert y_only.grad_fn is not None and y_only.grad_fn.saved_tensors == ()
    yg = yd.clone().requires_grad_(True)
    ops.focal_freq_loss(xd, yg).sum().backward()
    assert yg.grad is None                                                          # no gradient for the target
    plain = ops.focal_freq_loss(xd, yd)
    assert plain.grad_fn is None and torch.equal(plain, with_grad.detach()) and torch.equal(plain, y_only.detach())
    assert torch.equal(ops.focal_freq_loss(xd.view(2, 1, 45, 71), yd), plain)       # (N,1,H,W) and (N,H,W) alike


def test_the_op_refuses_what_the_library_refuses():
    from seg2eye_amd import _lib, ops
    x = torch.zeros(1, 1, 16, 16, device=DEV)
    with pytest.raises(_lib.Seg2EyeHipError, match=r'alpha=-1 \(a finite number in \[0, 4\] expected\)'):
        ops.focal_freq_loss(x, x, -1.0)
    with pytest.raises(_lib.Seg2EyeHipError, match=r'alpha=4\.5'):
        ops.focal_freq_loss_u8(x.to(torch.uint8), x.to(torch.uint8), 4.5)
    with pytest.raises(_lib.Seg2EyeHipError, match=r'alpha=nan'):
        ops.focal_freq_loss(x.clone().requires_grad_(True), x, float('nan'))
    one = torch.zeros(1, 1, 1, 16, device=DEV)
    with pytest.raises(_lib.Seg2EyeHipError, match=r'H=1 W=16 \(2 to 1024 rows and columns expected\)'):
        ops.focal_freq_loss(one, one)
    wide = torch.zeros(1, 2, 1025, device=DEV)
    with pytest.raises(_lib.Seg2EyeHipError, match=r'H=2 W=1025'):
        ops.focal_freq_loss(wide.requires_grad_(True), wide.detach())
    with pytest.raises(ValueError, match='one shape'):
        ops.focal_freq_loss(x, torch.zeros(1, 1, 16, 18, device=DEV))


# ------------------------------------------------------------------------------------------------ the generator's loss term
def test_generator_loss_term_matches_the_restatement_and_reaches_netG():
    """ngf = ndf = 8, batch 2, fp32, at 256 x 256: FFL/weighted = 3 mean ffl(fake, target) of the fake the step returns, within the bound of
    the op test; the backward runs and moves netG's gradient; without the flag the keys do not exist and the step's losses are the parent
    commit's."""
    from seg2eye_amd import ops
    res = {}
    for lam in (3.0, 0.0):
        ops.losses._FFL_TABLES.clear()
        tr = _trainer(lambda_ffl=lam, ffl_alpha=1.0)
        assert (len(ops.losses._FFL_TABLES) == 1) == bool(lam)                      # the model built the tables, and only under the flag
        tr.run_generator_one_step(dict(_batch()))
        torch.cuda.synchronize()
        fake, grad = tr.get_latest_generated().double().cpu(), tr.optimizer_G.flat_g.detach().double().cpu().clone()
        g_losses = dict(tr.get_latest_losses(include_log_losses=True))
        tr.run_discriminator_one_step(dict(_batch()))
        torch.cuda.synchronize()
        res[lam] = (g_losses, fake, grad, set(tr.get_latest_losses(include_log_losses=True)))
    losses, fake, grad, _ = res[3.0]
    assert res[0.0][3] == PARENT_LOSS_KEYS and res[3.0][3] == PARENT_LOSS_KEYS | {'FFL/weighted'}
    assert set(losses) - set(res[0.0][0]) == {'FFL/weighted', 'FFL/raw'}
    assert tuple(losses['FFL/weighted'].shape) == (1,) and tuple(fake.shape) == (2, 1, 256, 256)
    target = _batch()['target'].double()[:, 0]
    f64 = R.ffl(fake[:, 0], target, 1.0)
    e = float(((R.ffl(fake[:, 0], target, 1.0, torch.float32, 'matrix').double() - f64).abs() / f64).max())
    want = float(f64.mean())
    got = float(losses['FFL/weighted'])
    print('FFL/weighted %.8e, restatement %.8e (e %.3e, bound %.3e); FFL/raw %.8e' % (got, 3 * want, e, _bound(e), float(losses['FFL/raw'])))
    assert abs(got - 3 * want) <= 3 * want * (_bound(e) + 2.0 ** -22), (got, want, e)       # (+ the mean and the product, fp32)
    assert abs(float(losses['FFL/raw']) - want) <= want * (_bound(e) + 2.0 ** -22)
    assert bool(torch.isfinite(grad).all())
    # the two runs share weights and batch: without the term their gradients differ by float-atomics noise (~1e-6), with it by the term
    moved = float((grad - res[0.0][2]).norm() / res[0.0][2].norm())
    print('netG + netE gradient moved by %.3e of its norm' % moved)
    assert moved > 1e-3, moved


def test_hip_graph_replays_follow_the_eager_ffl_log():
    """Two iterations with hip_graphs on and off from the same state, --lambda_ffl at alpha 1.5: the logs agree within
    test_hip_graph_steps_match_eager's bounds (5e-4 on identical weights, 1e-2 once Adam steps have been taken), i.e. the launches
    capture and every replay scores anew."""
    res = {}
    for graphs in (False, True):
        tr = _trainer(lambda_ffl=2.0, ffl_alpha=1.5, hip_graphs=graphs)
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
        assert set(a) == set(b) == PARENT_LOSS_KEYS | {'FFL/raw', 'FFL/weighted'}
        for k in ('FFL/raw', 'FFL/weighted'):
            print(it, k, a[k], b[k])
            assert abs(a[k] - b[k]) <= (5e-4 if it == 0 else 1e-2) * abs(a[k]), (it, k, a[k], b[k])
        assert abs(a['FFL/weighted'] - 2.0 * a['FFL/raw']) <= 1e-6 * a['FFL/weighted'] and a['FFL/raw'] > 0
    assert res[True][0]['FFL/raw'] != res[True][1]['FFL/raw']                       # the second replay scored the stepped generator


# ------------------------------------------------------------------------------------------------ the Tester
def test_tester_scores_ffl_only_under_the_flag(tmp_path, capsys):
    from seg2eye_amd.options import parse
    from seg2eye_amd.pix2pix_model import Pix2PixModel
    from seg2eye_amd.tester import Tester
    argv = ['--name', 'ffl', '--checkpoints_dir', str(tmp_path), '--dataset_key', 'validation', '--ngf', '8', '--crop_size', '256',
            '--aspect_ratio', '1.0', '--batchSize', '2', '--synthetic_size', '4', '--compute_dtype', 'fp32']
    opt = parse(argv, is_train=False)
    torch.manual_seed(0)
    Pix2PixModel(parse(argv)).save('latest')
    model = Pix2PixModel(opt)
    model.eval()
    plain = Tester(opt, dataset_key='validation')
    errs_plain, stats_plain = plain.run(model, mode='full', write_error_log=True)
    assert sorted(stats_plain) == ['mse/validation/full/relative'] and len(errs_plain) == 4          # the parent commit's key ...
    assert sorted(_load_log(plain)) == ['error', 'filename', 'user'] and plain.all_ffl == []         # ... and its datasets

    tester = Tester(parse(argv + ['--val_ffl'], is_train=False), dataset_key='validation')
    seen, run_batch = [], tester.run_batch

    def recording(data_i, model):
        out = run_batch(data_i, model)
        assert len(out) == 4
        seen.append((out[2].cpu(), out[3].cpu()))
        return out
    tester.run_batch = recording
    capsys.readouterr()
    errs, stats = tester.run(model, mode='full', write_error_log=True)
    printed = capsys.readouterr().out
    assert sorted(stats) == ['ffl/validation/full', 'mse/validation/full/relative'] and len(seen) == 2
    assert '  ffl/validation/full, %.3e' % stats['ffl/validation/full'] in printed
    np.testing.assert_allclose(np.asarray(errs), np.asarray(errs_plain), rtol=1e-6)
    assert stats['mse/validation/full/relative'] == pytest.approx(stats_plain['mse/validation/full/relative'], rel=1e-6)
    log = _load_log(tester)
    assert sorted(log) == ['error', 'ffl', 'filename', 'user'] and log['ffl'].dtype == np.float64 and log['ffl'].shape == (4,)
    produced, target = torch.cat([p for p, _ in seen])[:, 0], torch.cat([t for _, t in seen])[:, 0]
    assert produced.dtype == torch.uint8 and tuple(produced.shape) == (4, 640, 400) and tuple(target.shape) == (4, 640, 400)
    want = R.ffl_u8(produced, target, 1.0)
    e = float(((R.ffl_u8(produced, target, 1.0, torch.float32, 'matrix').double() - want).abs() / want).max())
    err = float((np.abs(log['ffl'] - want.numpy()) / want.numpy()).max())
    print('validation ffl %s; relative error %.3e (e %.3e, bound %.3e)' % (log['ffl'].tolist(), err, e, _bound(e)))
    assert err <= _bound(e), (err, e)
    assert abs(stats['ffl/validation/full'] - float(want.mean())) <= _bound(e) * float(want.mean())
    assert np.array_equal(log['ffl'], np.asarray(tester.all_ffl, dtype=np.float64))


# ------------------------------------------------------------------------------------------------ the table of the header
def _table():
    rows = ['    shape      alpha  kind     ffl (min .. max)         e(loss)    e(gradient)']
    for (shape, alpha), cid in zip(CASES, CASE_IDS):
        for kind in KINDS:
            f64, _, _, e_f, e_g = _reference(shape, alpha, kind, False)
            rows.append('    %-10s %-5g  %-7s  %.3e .. %.3e   %.1e    %.1e' % (cid.split('-')[0], alpha, kind, float(f64.min()), float(f64.max()), e_f, e_g))
    return '\n'.join(rows)


if __name__ == '__main__':
    print(_table())
