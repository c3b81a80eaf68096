"""The focal frequency loss without a GPU: the torch restatement of the rule (tests/_ffl_ref.py) checked alone -- its three
forms of the spectrum against each other, Parseval, two images by hand, the exact zeros, the swap symmetry -- the flags, the size queries,
and what the entry points answer before any launch.  The DFT tables are filled on the device: tests/test_ffl_gpu.py checks them."""
import ctypes
import math

import pytest
import torch

import _ffl_ref as R
from _quality_harness import check_error_table

F32, BF16, BAD = 0, 1, 7
P = 4096                                                      # a dummy non-null pointer: must never reach a kernel
BIG = 1 << 30                                                 # a buffer size that is never short
ALPHAS = (0.0, 0.5, 1.0, 1.5, 2.0, 4.0)
SHAPES = ((2, 2, 2), (2, 4, 4), (2, 16, 16), (2, 17, 23), (1, 18, 40), (2, 45, 71), (1, 64, 48))


def _iid(n, H, W, seed):
    return torch.rand(n, H, W, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2 - 1


# ------------------------------------------------------------------------------------------------ the restatement
def test_matrix_and_half_spectrum_forms_agree_with_fft2():
    """fp64: the two real matrix products give fft2's spectrum, loss and gradient to rounding, and so does the half spectrum with the
    multiplicities 1, 2, ..., 2 (, 1 when W is even)."""
    for i, (n, H, W) in enumerate(SHAPES):
        x, y, gs = _iid(n, H, W, 10 + i), _iid(n, H, W, 50 + i), torch.tensor([1.0, -0.75][:n], dtype=torch.float64)
        re, im = R.spectrum(x - y, 'fft')
        rm, imm = R.spectrum(x - y, 'matrix')
        rh, ih = R.spectrum(x - y, 'half')
        scale = float((re * re + im * im).max().sqrt())
        assert float((re - rm).abs().max()) <= 1e-13 * scale and float((im - imm).abs().max()) <= 1e-13 * scale, (H, W)
        assert rh.shape == (n, H, W // 2 + 1)                                   # (a narrower product may round differently: no bit equality)
        assert float((rh - rm[..., :W // 2 + 1]).abs().max()) <= 1e-13 * scale and float((ih - imm[..., :W // 2 + 1]).abs().max()) <= 1e-13 * scale
        m = R.multiplicities(W)
        assert float(m.sum()) == W and float(m[0]) == 1 and (float(m[-1]) == 1) == (W % 2 == 0)
        for alpha in ALPHAS:
            f, g = R.ffl_and_grad(x, y, gs, alpha, method='fft')
            for method in ('matrix', 'half'):
                f2, g2 = R.ffl_and_grad(x, y, gs, alpha, method=method)
                assert float(((f2 - f) / f).abs().max()) <= 1e-12, (H, W, alpha, method)
                assert float((g2 - g).abs().max()) <= 1e-12 * float(g.abs().max()), (H, W, alpha, method)


def test_alpha_zero_is_the_mean_squared_error():
    """Parseval: the orthonormal DFT keeps the sum of squares, and at alpha = 0 every weight is 1; the gradient is 2 (x - y) / (H W)."""
    for i, (n, H, W) in enumerate(SHAPES):
        x, y = _iid(n, H, W, 100 + i), _iid(n, H, W, 200 + i)
        mse = ((x - y) ** 2).mean(dim=(1, 2))
        for method in ('fft', 'matrix', 'half'):
            f, g = R.ffl_and_grad(x, y, torch.ones(n, dtype=torch.float64), 0.0, method=method)
            assert float(((f - mse) / mse).abs().max()) <= 1e-13, (H, W, method)
            assert float((g - 2 * (x - y) / (H * W)).abs().max()) <= 1e-13 * float(g.abs().max())


def test_a_2x2_and_a_4x4_image_by_hand():
    # 2 x 2, d = [[1, 2], [3, 4]]: Z = 1/2 [[10, -2], [-4, 0]], dist = [[25, 1], [4, 0]]
    d = torch.tensor([[[1.0, 2.0], [3.0, 4.0]]], dtype=torch.float64)
    zero = torch.zeros_like(d)
    re, im = R.spectrum(d, 'fft')
    assert torch.allclose(re, torch.tensor([[[5.0, -1.0], [-2.0, 0.0]]], dtype=torch.float64), atol=1e-15) and float(im.abs().max()) <= 1e-15
    assert float(R.ffl(d, zero, 0.0)) == pytest.approx(30.0 / 4, rel=1e-15)
    assert float(R.ffl(d, zero, 1.0)) == pytest.approx((25 * 1 + 1 * 0.2 + 4 * 0.4 + 0) / 4, rel=1e-15)          # w = sqrt(dist) / 5
    assert float(R.ffl(d, zero, 2.0)) == pytest.approx((25 * 1 + 1 / 25 + 16 / 25) / 4, rel=1e-15)               # w = dist / 25
    # the gradient at alpha = 2: 2 / (H W) Re IDFT(w Z), w Z = [[5, -1/25], [-8/25, 0]]; IDFT2 (orthonormal) of a real 2 x 2 block B
    # is 1/2 [[a+b+c+e, a-b+c-e], [a+b-c-e, a-b-c+e]] for B = [[a, b], [c, e]]
    _, g = R.ffl_and_grad(d, zero, torch.ones(1, dtype=torch.float64), 2.0)
    a, b, c, e = 5.0, -1 / 25, -8 / 25, 0.0
    want = 0.25 * torch.tensor([[[a + b + c + e, a - b + c - e], [a + b - c - e, a - b - c + e]]], dtype=torch.float64)
    assert torch.allclose(g, want, rtol=0, atol=1e-15)
    # 4 x 4, d = cos(2 pi (r + c) / 4): two bins, (1, 1) and (3, 3), each with Z = 2 (dist 4); every weight that matters is 1 at any alpha
    r = torch.arange(4, dtype=torch.float64)
    d4 = torch.cos(2 * math.pi * (r[:, None] + r[None, :]) / 4).unsqueeze(0)
    re, im = R.spectrum(d4, 'fft')
    want = torch.zeros(1, 4, 4, dtype=torch.float64)
    want[0, 1, 1] = want[0, 3, 3] = 2.0
    assert torch.allclose(re, want, atol=1e-15) and float(im.abs().max()) <= 1e-15
    for alpha in ALPHAS:
        for method in ('fft', 'matrix', 'half'):
            f, g = R.ffl_and_grad(d4, torch.zeros_like(d4), torch.ones(1, dtype=torch.float64), alpha, method=method)
            assert float(f) == pytest.approx(8.0 / 16, rel=1e-14), (alpha, method)                              # = mean(d^2) = 1/2
            assert torch.allclose(g, 2 * d4 / 16, rtol=0, atol=1e-15), (alpha, method)
    # a constant difference: the DC bin alone, Z = c sqrt(H W), ffl = c^2 at every alpha
    for alpha in ALPHAS:
        assert float(R.ffl(torch.full((1, 3, 5), 0.3, dtype=torch.float64), torch.zeros(1, 3, 5, dtype=torch.float64), alpha)) == pytest.approx(0.09, rel=1e-13)


def test_identical_images_give_exact_zeros():
    x = _iid(2, 17, 23, 3)
    for alpha in ALPHAS:
        for dtype, method in ((torch.float64, 'fft'), (torch.float64, 'matrix'), (torch.float64, 'half'), (torch.float32, 'matrix')):
            f, g = R.ffl_and_grad(x, x.clone(), torch.tensor([1.0, -2.0], dtype=torch.float64), alpha, dtype, method)
            assert f.dtype == dtype and bool((f == 0).all()) and bool((g == 0).all()), (alpha, dtype, method)


def test_the_loss_is_symmetric_in_its_images():
    for i, (n, H, W) in enumerate(SHAPES):
        x, y = _iid(n, H, W, 300 + i), _iid(n, H, W, 400 + i)
        for alpha in ALPHAS:
            a, b = R.ffl(x, y, alpha), R.ffl(y, x, alpha)
            assert float(((a - b) / a).abs().max()) <= 1e-13, (H, W, alpha)


def test_the_weight_is_a_constant_of_the_step():
    """No gradient flows through w: the gradient is that of sum(w0 * dist) with w0 frozen, not of the whole expression."""
    x, y = _iid(1, 8, 12, 5), _iid(1, 8, 12, 6)
    _, g = R.ffl_and_grad(x, y, torch.ones(1, dtype=torch.float64), 1.0)
    xx = x.clone().requires_grad_(True)
    z = torch.fft.fft2(xx - y, norm='ortho')
    dist = z.real ** 2 + z.imag ** 2
    w0 = (dist.sqrt() / dist.sqrt().max()).detach()
    (w0 * dist).mean().backward()
    assert float((g - xx.grad).abs().max()) <= 1e-14 * float(g.abs().max())
    xx.grad = None
    z = torch.fft.fft2(xx - y, norm='ortho')
    dist = z.real ** 2 + z.imag ** 2
    ((dist.sqrt() / dist.sqrt().max()) * dist).mean().backward()
    assert float((g - xx.grad).abs().max()) > 1e-3 * float(g.abs().max())


def test_uint8_images_count_in_units_of_255():
    gen = torch.Generator().manual_seed(9)
    a = torch.randint(0, 256, (2, 9, 14), generator=gen, dtype=torch.uint8)
    b = torch.randint(0, 256, (2, 9, 14), generator=gen, dtype=torch.uint8)
    assert torch.allclose(R.ffl_u8(a, b, 0.0), ((a.double() - b.double()) / 255).pow(2).mean(dim=(1, 2)), rtol=1e-13, atol=0)
    assert torch.allclose(R.ffl_u8(a, b, 1.0), R.ffl(a.double() / 255, b.double() / 255, 1.0), rtol=1e-15, atol=0)
    assert bool((R.ffl_u8(a, a, 1.0) == 0).all())


# ------------------------------------------------------------------------------------------------ the flags
def test_flags_parse_and_default_off():
    from seg2eye_amd.options import default_opt, parse
    o = parse([])
    assert (o.lambda_ffl, o.ffl_alpha, o.val_ffl) == (0.0, 1.0, False)
    o = parse(['--lambda_ffl', '2', '--ffl_alpha', '0.5'])
    assert (o.lambda_ffl, o.ffl_alpha, o.val_ffl) == (2.0, 0.5, False)
    t = parse(['--val_ffl'], is_train=False)
    assert t.val_ffl is True and t.lambda_ffl == 0.0 and t.ffl_alpha == 1.0 and parse([], is_train=False).val_ffl is False
    assert parse(['--val_ffl']).val_ffl is True                                     # train.py's periodic validation takes it too
    assert default_opt(lambda_ffl=1.0).lambda_ffl == 1.0 and default_opt().lambda_ffl == 0.0 and default_opt().ffl_alpha == 1.0
    for ok in ('0', '4', '1.5'):
        assert parse(['--ffl_alpha', ok]).ffl_alpha == float(ok)
    for bad in ('-0.5', '4.5', 'nan', 'inf'):
        with pytest.raises(ValueError, match=r'--ffl_alpha must lie in \[0, 4\]'):
            parse(['--lambda_ffl', '1', '--ffl_alpha', bad])
    with pytest.raises(SystemExit):
        parse(['--lambda_ffl', '1'], is_train=False)                                # a training flag only
    with pytest.raises(SystemExit):
        parse(['--ffl_alpha', '1'], is_train=False)


def test_ops_refuse_cpu_tensors():
    from seg2eye_amd import _lib, ops
    x = torch.zeros(2, 1, 16, 16)
    with pytest.raises(_lib.Seg2EyeHipError, match='GPU only'):
        ops.focal_freq_loss(x, x)
    with pytest.raises(_lib.Seg2EyeHipError, match='GPU only'):
        ops.focal_freq_loss(x.requires_grad_(True), x, alpha=0.0)
    with pytest.raises(_lib.Seg2EyeHipError, match='GPU only'):
        ops.focal_freq_loss_u8(x.detach().to(torch.uint8), x.detach().to(torch.uint8))
    with pytest.raises(_lib.Seg2EyeHipError, match='GPU only'):
        ops.ffl_tables(16, 16, 'cpu')
    with pytest.raises(ValueError, match='uint8'):
        ops.focal_freq_loss_u8(x.detach(), x.detach())
    assert ops.focal_freq_loss is ops.losses.focal_freq_loss and ops.focal_freq_loss_u8 is ops.losses.focal_freq_loss_u8
    assert ops.FocalFreqFn is ops.losses.FocalFreqFn


# ------------------------------------------------------------------------------------------------ the entry points, before any launch
NAMES = ('s2e_ffl_tables_bytes', 's2e_ffl_workspace_bytes', 's2e_ffl_spectrum_bytes', 's2e_ffl_tables', 's2e_ffl_fwd', 's2e_ffl_u8', 's2e_ffl_bwd')
TAB, FWD, U8, BWD = NAMES[3:]
SIZE = '%s: H=%d W=%d (2 to 1024 rows and columns expected)'
LIMIT = '%s: N=%d H=%d W=%d is beyond the launch limits (N <= 65535, N H W < 2^31)'
ALPHA = '%s: alpha=%s (a finite number in [0, 4] expected)'


def _up(v, m):
    return (v + m - 1) // m * m


def _sizes(N, H, W):
    """(tables, workspace, spectrum) bytes: rows padded to 64, pixel columns to 64, the W/2 + 1 spectrum columns to 32; the tables are
    C_H, S_H (Hp x Hp), [C_W | S_W] (Wp x 2 Whp) and its transpose with the multiplicities; the workspace holds the row transform
    (N x Hp x 2 Whp fp32) and one fp64 sum and one fp32 maximum per 64 x 32 block of bins, every section on 256 bytes; the spectrum is
    N x 2 Hp x Whp fp32."""
    Hp, Wp, Whp = _up(H, 64), _up(W, 64), _up(W // 2 + 1, 32)
    blocks = N * (Hp // 64) * (Whp // 32)
    return ((2 * Hp * Hp + 4 * Wp * Whp) * 4, _up(N * Hp * 2 * Whp * 4, 256) + _up(blocks * 8, 256) + _up(blocks * 4, 256), N * 2 * Hp * Whp * 4)


T256, WS256, SP256 = 1179648, 656128, 655360                   # (2, 256, 256)


def _tab(H=256, W=256, tables=P, tables_bytes=BIG):
    return (H, W, tables, tables_bytes, None)


def _fwd(dtype=F32, x=P, y=P, N=2, H=256, W=256, alpha=1.0, tables=P, tables_bytes=BIG, out=P, coef=P, spec=P, spec_bytes=BIG, ws=P, ws_bytes=BIG):
    return (dtype, x, y, N, H, W, alpha, tables, tables_bytes, out, coef, spec, spec_bytes, ws, ws_bytes, None)


def _u8(a=P, b=P, N=1, H=640, W=400, alpha=1.0, tables=P, tables_bytes=BIG, out=P, ws=P, ws_bytes=BIG):
    return (a, b, N, H, W, alpha, tables, tables_bytes, out, ws, ws_bytes, None)


def _bwd(dtype=F32, spec=P, coef=P, gout=P, N=2, H=256, W=256, alpha=1.0, tables=P, tables_bytes=BIG, ws=P, ws_bytes=BIG, dx=P):
    return (dtype, spec, coef, gout, N, H, W, alpha, tables, tables_bytes, ws, ws_bytes, dx, None)


def _error_tables():
    inf, nan = float('inf'), float('nan')
    tab = [
        (_tab(tables=None), -1, TAB + ': bad argument'),
        (_tab(H=1), -3, SIZE % (TAB, 1, 256)),
        (_tab(W=1025, tables_bytes=0), -3, SIZE % (TAB, 256, 1025)),                                # the size before the buffer
        (_tab(H=0), -3, SIZE % (TAB, 0, 256)),
        (_tab(tables_bytes=T256 - 4), -1, TAB + ': tables of %d bytes, needs %d' % (T256 - 4, T256)),
    ]
    fwd = [(_fwd(**{k: None}), -1, FWD + ': bad argument') for k in ('x', 'y', 'tables', 'out', 'coef', 'ws')]
    fwd += [
        (_fwd(N=0), -1, FWD + ': bad argument'),
        (_fwd(dtype=BAD, alpha=-1.0, H=1), -1, FWD + ': bad dtype 7'),                              # the dtype before alpha and the size
        (_fwd(alpha=-0.5, H=1), -1, ALPHA % (FWD, '-0.5')),                                         # alpha before the size
        (_fwd(alpha=4.5), -1, ALPHA % (FWD, '4.5')),
        (_fwd(alpha=nan), -1, ALPHA % (FWD, 'nan')),
        (_fwd(alpha=inf), -1, ALPHA % (FWD, 'inf')),
        (_fwd(H=1), -3, SIZE % (FWD, 1, 256)),
        (_fwd(W=1, ws_bytes=0), -3, SIZE % (FWD, 256, 1)),                                          # the size before the buffers
        (_fwd(H=1025), -3, SIZE % (FWD, 1025, 256)),
        (_fwd(W=-3), -3, SIZE % (FWD, 256, -3)),
        (_fwd(N=65536, H=16, W=16), -3, LIMIT % (FWD, 65536, 16, 16)),
        (_fwd(N=2048, H=1024, W=1024), -3, LIMIT % (FWD, 2048, 1024, 1024)),
        (_fwd(tables_bytes=T256 - 4, ws_bytes=0), -1, FWD + ': tables of %d bytes, needs %d' % (T256 - 4, T256)),   # the tables before the workspace
        (_fwd(ws_bytes=WS256 - 1), -1, FWD + ': workspace of %d bytes, needs %d' % (WS256 - 1, WS256)),
        (_fwd(spec_bytes=SP256 - 4), -1, FWD + ': spectrum of %d bytes, needs %d' % (SP256 - 4, SP256)),
        (_fwd(spec=None, spec_bytes=0, ws_bytes=0), -1, FWD + ': workspace of 0 bytes, needs %d' % WS256),            # a forward that keeps nothing is legal
    ]
    u8 = [(_u8(**{k: None}), -1, U8 + ': bad argument') for k in ('a', 'b', 'tables', 'out', 'ws')]
    u8 += [
        (_u8(N=-1), -1, U8 + ': bad argument'),
        (_u8(alpha=5.0), -1, ALPHA % (U8, '5')),
        (_u8(W=1), -3, SIZE % (U8, 640, 1)),
        (_u8(N=65536, H=16, W=16), -3, LIMIT % (U8, 65536, 16, 16)),
        (_u8(ws_bytes=8), -1, U8 + ': workspace of 8 bytes, needs %d' % _sizes(1, 640, 400)[1]),
        (_u8(tables_bytes=8), -1, U8 + ': tables of 8 bytes, needs %d' % _sizes(1, 640, 400)[0]),
    ]
    bwd = [(_bwd(**{k: None}), -1, BWD + ': bad argument') for k in ('spec', 'coef', 'gout', 'tables', 'ws', 'dx')]
    bwd += [
        (_bwd(N=0), -1, BWD + ': bad argument'),
        (_bwd(dtype=BAD, alpha=9.0), -1, BWD + ': bad dtype 7'),
        (_bwd(alpha=-1.0), -1, ALPHA % (BWD, '-1')),
        (_bwd(H=1), -3, SIZE % (BWD, 1, 256)),
        (_bwd(N=32768), -3, LIMIT % (BWD, 32768, 256, 256)),
        (_bwd(ws_bytes=WS256 - 1), -1, BWD + ': workspace of %d bytes, needs %d' % (WS256 - 1, WS256)),
        (_bwd(tables_bytes=0), -1, BWD + ': tables of 0 bytes, needs %d' % T256),
    ]
    return ((TAB, tab), (FWD, fwd), (U8, u8), (BWD, bwd))


def test_entry_points_are_declared_exported_and_bound():
    import os
    import re
    from seg2eye_amd import _lib
    from conftest import ROOT
    header = open(os.path.join(ROOT, 'include', 'seg2eye_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in _lib.SIGNATURES and hasattr(dll, name) and callable(getattr(_lib.call, name)), name
    assert [_lib.SIGNATURES[n][0] for n in NAMES] == [_lib.SIZE] * 3 + [_lib.STATUS] * 4
    # the header comment states the rule in full
    for phrase in ('orthonormal 2-D DFT', 'dist = Re Z^2 + Im Z^2', 'no gradient flows', 'alpha = 0: w = 1 everywhere', '2 / (H W) Re(inverse orthonormal 2-D DFT of w Z)',
                   'multiplicity 1 for kx = 0', 'patch_factor'):
        assert phrase in header, phrase
    from seg2eye_amd import build
    assert 'ffl.hip' in build.SOURCES


def test_ffl_entry_points_reject_bad_calls_before_any_launch():
    """Null pointers (the spectrum of a forward that keeps nothing excepted), N <= 0, a bad dtype, alpha negative, non-finite or above 4, a
    short buffer: S2E_ERR_ARG; H or W outside 2..1024 or a grid beyond the launch limits: S2E_ERR_UNSUPPORTED; the message, and which check
    wins.  Host-only: with a GPU visible the test skips itself, so that a dummy pointer can never reach a kernel (as
    test_msssim_entry_points_reject_bad_calls_before_any_launch does)."""
    if torch.cuda.is_available():
        pytest.skip('dummy pointers: host-only by construction')
    from seg2eye_amd import _lib
    assert (_lib.S2E_BF16, _lib.S2E_F32) == (BF16, F32)
    for name, table in _error_tables():
        check_error_table(name, table)
    with pytest.raises(_lib.Seg2EyeHipError, match='s2e_ffl_fwd failed'):
        _lib.call.s2e_ffl_fwd(*_fwd(x=None))


def test_size_queries_are_exact_monotone_and_zero_where_illegal():
    from seg2eye_amd import _lib
    L = _lib.lib()
    tab, ws, spec = L.s2e_ffl_tables_bytes, L.s2e_ffl_workspace_bytes, L.s2e_ffl_spectrum_bytes
    assert isinstance(tab(16, 16), int) and ctypes.sizeof(ctypes.c_size_t) == 8
    assert (tab(256, 256), ws(2, 256, 256), spec(2, 256, 256)) == (T256, WS256, SP256) == _sizes(2, 256, 256)
    assert (tab(2, 2), ws(1, 2, 2), spec(1, 2, 2)) == ((2 * 64 * 64 + 4 * 64 * 32) * 4, 64 * 64 * 4 + 256 + 256, 2 * 64 * 32 * 4)
    for n, h, w in ((2, 16, 16), (2, 17, 23), (1, 18, 40), (2, 45, 71), (1, 64, 48), (8, 256, 256), (1, 640, 400), (3, 384, 400), (1, 1024, 1024),
                    (65535, 2, 2)):
        assert (tab(h, w), ws(n, h, w), spec(n, h, w)) == _sizes(n, h, w), (n, h, w)
    for bad in ((1, 256), (256, 1), (0, 0), (-4, 64), (1025, 64), (64, 1025)):
        assert tab(*bad) == 0 and ws(2, *bad) == 0 and spec(2, *bad) == 0, bad
    for bad in ((0, 256, 256), (-1, 256, 256), (65536, 16, 16), (2048, 1024, 1024)):
        assert ws(*bad) == 0 and spec(*bad) == 0, bad
    sizes = [2, 16, 17, 64, 65, 256, 384, 400, 640, 1024]
    for n in (1, 2):
        for i, h in enumerate(sizes):
            for j, w in enumerate(sizes):
                for q in (ws, spec):
                    b = q(n, h, w)
                    assert b > 0 and b % 4 == 0 and q(n + 1, h, w) > b, (n, h, w)
                    if i:
                        assert b >= q(n, sizes[i - 1], w), (n, h, w)
                    if j:
                        assert b >= q(n, h, sizes[j - 1]), (n, h, w)
