"""MS-SSIM without a GPU: the torch restatement of the rule (tests/_msssim_ref.py) checked alone, the two flags, the size
queries, and what the three entry points answer before any launch."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _msssim_ref as M
import _ssim_ref as R
from _quality_harness import check_error_table

F32, BF16, BAD = 0, 1, 7
P = 4096                                                      # a dummy non-null pointer: must never reach a kernel
BIG = 1 << 30                                                 # a buffer size that is never short


def _floats(*v):
    return (ctypes.c_float * len(v))(*v)


W5 = _floats(*M.WEIGHTS)
W2 = _floats(0.5, 0.5)


# ------------------------------------------------------------------------------------------------ the restatement
def _iid(n, H, W, seed):
    return torch.rand(n, H, W, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2 - 1


def test_identical_images_score_one_with_no_gradient():
    x = _iid(2, 176, 181, 1)
    s, terms, g = M.ms_ssim_and_grad(x, x.clone(), torch.tensor([1.0, -2.0], dtype=torch.float64))
    assert s.shape == (2,) and terms.shape == (2, 5) and float((terms - 1).abs().max()) <= 1e-12
    assert float((s - 1).abs().max()) <= 1e-12 and g.shape == x.shape and float(g.abs().max()) < 1e-12


def test_constant_images_give_the_closed_form():
    """Every variance is 0: cs = 1 at every level below the last, and the last level is the luminance term alone (0 against 1: 1e-4, below
    the floor, so it counts as F)."""
    for a, b in ((0.25, 0.75), (0.9, 0.88), (0.0, 1.0)):
        x = torch.full((2, 180, 176), 2 * a - 1, dtype=torch.float64)
        y = torch.full((2, 180, 176), 2 * b - 1, dtype=torch.float64)
        lum = (2 * a * b + R.C1) / (a * a + b * b + R.C1)
        want = 1.0
        for j, w in enumerate(M.WEIGHTS):
            want *= (max(lum, M.FLOOR) if j == 4 else 1.0) ** w
        got, terms = M.ms_ssim(x, y, return_terms=True)
        assert float((got - want).abs().max()) <= 1e-9, (a, b)
        assert float((terms[:, :4] - 1).abs().max()) <= 1e-9 and float((terms[:, 4] - lum).abs().max()) <= 1e-9
    a8, b8 = torch.full((1, 22, 22), 63, dtype=torch.uint8), torch.full((1, 22, 22), 191, dtype=torch.uint8)
    ua, ub = 63 / 255, 191 / 255
    assert abs(float(M.ms_ssim_u8(a8, b8, [0.4, 0.6])) - ((2 * ua * ub + R.C1) / (ua * ua + ub * ub + R.C1)) ** 0.6) <= 1e-9


def test_one_level_with_weight_one_is_ssim():
    x, y = _iid(2, 19, 23, 2), _iid(2, 19, 23, 3)
    y = 0.7 * x + 0.3 * y                                     # (positive SSIM: nothing clamps)
    assert float((M.ms_ssim(x, y, [1.0]) - R.ssim(x, y)).abs().max()) <= 1e-15
    _, _, g = M.ms_ssim_and_grad(x, y, torch.ones(2, dtype=torch.float64), [1.0])
    _, g1 = R.ssim_and_grad(x, y, torch.ones(2, dtype=torch.float64))
    assert float((g - g1).abs().max()) <= 1e-15


def _moments(u, v):
    w = torch.outer(R.window(), R.window())
    mu, mv = float((w * u).sum()), float((w * v).sum())
    return mu, mv, float((w * u * u).sum()) - mu * mu, float((w * v * v).sum()) - mv * mv, float((w * u * v).sum()) - mu * mv


def test_two_levels_on_22_by_22_by_hand():
    """Level 0 has 12 x 12 positions, level 1 (11 x 11) exactly one: cs position by position, S of the one window, written out in fp64."""
    x, y = _iid(1, 22, 22, 4), _iid(1, 22, 22, 5)
    y = 0.6 * x + 0.4 * y
    u, v = (x[0] + 1) / 2, (y[0] + 1) / 2
    cs = []
    for r in range(12):
        for c in range(12):
            _, _, su2, sv2, suv = _moments(u[r:r + 11, c:c + 11], v[r:r + 11, c:c + 11])
            cs.append((2 * suv + R.C2) / (su2 + sv2 + R.C2))
    m0 = sum(cs) / 144
    u1 = (u[0::2, 0::2] + u[0::2, 1::2] + u[1::2, 0::2] + u[1::2, 1::2]) / 4
    v1 = (v[0::2, 0::2] + v[0::2, 1::2] + v[1::2, 0::2] + v[1::2, 1::2]) / 4
    mu, mv, su2, sv2, suv = _moments(u1, v1)
    m1 = (2 * mu * mv + R.C1) * (2 * suv + R.C2) / ((mu * mu + mv * mv + R.C1) * (su2 + sv2 + R.C2))
    got, terms = M.ms_ssim(x, y, [0.3, 0.7], return_terms=True)
    assert abs(float(terms[0, 0]) - m0) <= 1e-13 and abs(float(terms[0, 1]) - m1) <= 1e-13
    assert m0 > M.FLOOR and m1 > M.FLOOR and abs(float(got) - m0 ** 0.3 * m1 ** 0.7) <= 1e-13


def test_odd_sizes_drop_the_trailing_row_and_column():
    """45 x 71 at three levels: 22 x 35, then 11 x 17.  The dropped row 44 and column 70 reach level 0 only; columns 68 and 69 (level 1's
    column 34, dropped on the way to level 2) reach levels 0 and 1 only: the levels' means say so, and so does the gradient."""
    x, y = _iid(1, 45, 71, 6), _iid(1, 45, 71, 7)
    y = 0.6 * x + 0.4 * y
    w = [0.2, 0.3, 0.5]
    _, t0 = M.ms_ssim(x, y, w, return_terms=True)
    x1 = x.clone()
    x1[:, 44, :] += 0.3
    x1[:, :, 70] -= 0.3
    _, t1 = M.ms_ssim(x1, y, w, return_terms=True)
    assert t1[0, 0] != t0[0, 0] and torch.equal(t1[0, 1:], t0[0, 1:])
    x2 = x.clone()
    x2[:, :, 68:70] += 0.3                                    # level 1's column 34: dropped on the way to level 2
    _, t2 = M.ms_ssim(x2, y, w, return_terms=True)
    assert t2[0, 0] != t0[0, 0] and t2[0, 1] != t0[0, 1] and torch.equal(t2[0, 2], t0[0, 2])
    lv = M.level_means((x + 1) / 2, (y + 1) / 2, 3)
    u2 = F.avg_pool2d(F.avg_pool2d(((x + 1) / 2)[:, :44, :70].unsqueeze(1), 2)[:, :, :22, :34], 2)[:, 0]
    v2 = F.avg_pool2d(F.avg_pool2d(((y + 1) / 2)[:, :44, :70].unsqueeze(1), 2)[:, :, :22, :34], 2)[:, 0]
    assert tuple(u2.shape) == (1, 11, 17) and abs(float(lv[0, 2]) - float(R.ssim_unit(u2, v2))) <= 1e-14
    # the gradient of the last level alone does not touch what was dropped on the way down: rows 44.., columns 68..
    xx = x.clone().requires_grad_(True)
    M.level_means((xx + 1) / 2, (y + 1) / 2, 3)[0, 2].backward()
    assert float(xx.grad[0, 44:, :].abs().max()) == 0 and float(xx.grad[0, :, 68:].abs().max()) == 0 and float(xx.grad[0, :44, :68].abs().min()) > 0


def test_a_level_clamped_at_the_floor_contributes_the_floor_and_no_gradient():
    """y = -x: the covariance is negative at every fine level, cs < 0, the level counts as F^w and passes nothing back."""
    x = _iid(1, 45, 71, 8)
    y = -x
    w = [0.2, 0.3, 0.5]
    s, terms, g = M.ms_ssim_and_grad(x, y, torch.ones(1, dtype=torch.float64), w)
    assert bool((terms < -0.05).all())
    assert abs(float(s) - M.FLOOR ** 1.0) <= 1e-15 and float(g.abs().max()) == 0
    # one live level: the others contribute F^w_j exactly, and the gradient is that of the live level alone
    xs = 0.5 * x
    lo = F.interpolate(F.avg_pool2d(xs.unsqueeze(1), 2), scale_factor=2)[:, 0]                    # (1, 44, 70)
    ys = xs.clone()
    blocky = F.interpolate(_iid(1, 22, 35, 9).unsqueeze(1), scale_factor=2)[:, 0]
    ys[:, :44, :70] = lo + 0.05 * blocky - (xs[:, :44, :70] - lo)   # fine detail inverted, coarse structure kept with noise: level 0 clamps, level 1 is live
    s, terms, g = M.ms_ssim_and_grad(xs, ys, torch.ones(1, dtype=torch.float64), [0.4, 0.6])
    assert float(terms[0, 0]) < 0 and 0.5 < float(terms[0, 1]) < 0.999
    assert abs(float(s) - M.FLOOR ** 0.4 * float(terms[0, 1]) ** 0.6) <= 1e-15
    xx = xs.clone().requires_grad_(True)
    t = M.level_means((xx + 1) / 2, (ys + 1) / 2, 2)[0, 1]
    (M.FLOOR ** 0.4 * t ** 0.6).backward()
    assert float(g.abs().max()) > 1e-6 and float((g - xx.grad).abs().max()) <= 1e-12 * float(g.abs().max())


# ------------------------------------------------------------------------------------------------ the flags
def test_flags_parse_and_default_off():
    from seg2eye_amd.options import default_opt, parse
    o = parse(['--lambda_msssim', '2'])
    assert o.lambda_msssim == 2.0 and o.val_msssim is False and parse([]).lambda_msssim == 0.0
    t = parse(['--val_msssim'], is_train=False)
    assert t.val_msssim is True and t.lambda_msssim == 0.0 and parse([], is_train=False).val_msssim is False
    assert parse(['--val_msssim']).val_msssim is True                               # train.py's periodic validation takes it too
    assert default_opt(lambda_msssim=1.0).lambda_msssim == 1.0 and default_opt().lambda_msssim == 0.0
    both = parse(['--lambda_msssim', '1', '--lambda_ssim', '0.5', '--val_ssim', '--val_msssim'])
    assert (both.lambda_msssim, both.lambda_ssim, both.val_ssim, both.val_msssim) == (1.0, 0.5, True, True)
    with pytest.raises(SystemExit):
        parse(['--lambda_msssim', '1'], is_train=False)                             # a training flag only


def test_the_model_refuses_images_too_small_for_five_levels():
    from seg2eye_amd.options import default_opt
    from seg2eye_amd.pix2pix_model import Pix2PixModel
    with pytest.raises(ValueError, match=r'--lambda_msssim: images of 128 x 128 are too small for five levels \(H, W >= 176'):
        Pix2PixModel(default_opt(crop_size=128, aspect_ratio=1.0, lambda_msssim=1.0))


def test_ops_refuse_cpu_tensors():
    from seg2eye_amd import _lib, ops
    x = torch.zeros(2, 1, 176, 176)
    with pytest.raises(_lib.Seg2EyeHipError, match='GPU only'):
        ops.ms_ssim(x, x)
    with pytest.raises(_lib.Seg2EyeHipError, match='GPU only'):
        ops.ms_ssim_terms(x, x)
    with pytest.raises(_lib.Seg2EyeHipError, match='GPU only'):
        ops.ms_ssim_u8(x.to(torch.uint8), x.to(torch.uint8))
    with pytest.raises(ValueError, match='uint8'):
        ops.ms_ssim_u8(x, x)
    assert ops.ms_ssim is ops.losses.ms_ssim and ops.MsSsimFn is ops.losses.MsSsimFn
    assert tuple(ops.MSSSIM_WEIGHTS) == M.WEIGHTS and ops.msssim_min_size() == 176 and ops.msssim_min_size(1) == 11


# ------------------------------------------------------------------------------------------------ the entry points, before any launch
SIZE = '%s: H=%d W=%d levels=%d (level %d is %d x %d: smaller than the 11 x 11 window, it has no position)'
LIMIT = '%s: N=%d H=%d W=%d is beyond the launch limits (N <= 65535, N H W < 2^31)'
LEVELS = '%s: levels=%d (1 to 5 levels expected)'
FWD, U8, BWD = 's2e_msssim_fwd', 's2e_msssim_u8', 's2e_msssim_bwd'
WS256, PYR256, MAPS256 = 2 * 171 * 8, 2 * 2 * 21760 * 4, 3 * 2 * (246 ** 2 + 118 ** 2 + 54 ** 2 + 22 ** 2 + 6 ** 2) * 4


def _fwd(dtype=F32, x=P, y=P, N=2, H=256, W=256, levels=5, weights=W5, out=P, terms=P, coef=P, maps=P, maps_bytes=BIG, pyr=P, pyr_bytes=BIG,
         ws=P, ws_bytes=BIG):
    return (dtype, x, y, N, H, W, levels, weights, out, terms, coef, maps, maps_bytes, pyr, pyr_bytes, ws, ws_bytes, None)


def _u8(a=P, b=P, N=1, H=640, W=400, levels=5, weights=W5, out=P, terms=P, pyr=P, pyr_bytes=BIG, ws=P, ws_bytes=BIG):
    return (a, b, N, H, W, levels, weights, out, terms, pyr, pyr_bytes, ws, ws_bytes, None)


def _bwd(dtype=F32, x=P, y=P, pyr=P, maps=P, coef=P, gout=P, N=2, H=256, W=256, levels=5, gbuf=P, gbuf_bytes=BIG, dx=P):
    return (dtype, x, y, pyr, maps, coef, gout, N, H, W, levels, gbuf, gbuf_bytes, dx, None)


def _error_tables():
    inf, nan = float('inf'), float('nan')
    fwd = [(_fwd(**{k: None}), -1, FWD + ': bad argument') for k in ('x', 'y', 'weights', 'out', 'terms', 'coef', 'ws')]
    fwd += [
        (_fwd(N=0), -1, FWD + ': bad argument'),
        (_fwd(dtype=BAD, levels=9, H=10), -1, FWD + ': bad dtype 7'),                               # the dtype before the levels and the size
        (_fwd(levels=0, H=10), -1, LEVELS % (FWD, 0)),                                              # the levels before the size
        (_fwd(levels=6), -1, LEVELS % (FWD, 6)),
        (_fwd(weights=_floats(0.2, 0.0, 0.3, 0.2, 0.1), H=100), -1, FWD + ': weights[1]=0 (every weight must be positive and finite)'),
        (_fwd(weights=_floats(0.2, 0.1, -0.5, 0.2, 0.1)), -1, FWD + ': weights[2]=-0.5 (every weight must be positive and finite)'),
        (_fwd(weights=_floats(0.2, 0.1, 0.5, inf, 0.1)), -1, FWD + ': weights[3]=inf (every weight must be positive and finite)'),
        (_fwd(weights=_floats(nan, 0.1, 0.5, 0.2, 0.1)), -1, FWD + ': weights[0]=nan (every weight must be positive and finite)'),
        (_fwd(levels=2, weights=_floats(0.5, 0.5, -1.0), ws_bytes=0), -1, FWD + ': workspace of 0 bytes, needs %d' % (2 * (128 + 32) * 8)),  # only `levels` weights are read
        (_fwd(H=175), -3, SIZE % (FWD, 175, 256, 5, 4, 10, 16)),
        (_fwd(W=175, ws_bytes=0), -3, SIZE % (FWD, 256, 175, 5, 4, 16, 10)),                        # the size before the buffers
        (_fwd(H=21, W=22, levels=2, weights=W2), -3, SIZE % (FWD, 21, 22, 2, 1, 10, 11)),
        (_fwd(H=0, levels=1), -3, SIZE % (FWD, 0, 256, 1, 0, 0, 256)),
        (_fwd(H=-5, levels=2), -3, SIZE % (FWD, -5, 256, 2, 1, 0, 128)),
        (_fwd(N=65536, H=176, W=176), -3, LIMIT % (FWD, 65536, 176, 176)),
        (_fwd(N=8, H=16384, W=16384), -3, LIMIT % (FWD, 8, 16384, 16384)),
        (_fwd(ws_bytes=WS256 - 1), -1, FWD + ': workspace of %d bytes, needs %d' % (WS256 - 1, WS256)),
        (_fwd(pyr_bytes=PYR256 - 4), -1, FWD + ': pyramid of %d bytes, needs %d' % (PYR256 - 4, PYR256)),
        (_fwd(pyr=None), -1, FWD + ': pyramid of 0 bytes, needs %d' % PYR256),
        (_fwd(maps_bytes=MAPS256 - 4), -1, FWD + ': maps of %d bytes, needs %d' % (MAPS256 - 4, MAPS256)),
        (_fwd(ws_bytes=0, pyr_bytes=0), -1, FWD + ': workspace of 0 bytes, needs %d' % WS256),      # the workspace before the pyramid
    ]
    u8 = [(_u8(**{k: None}), -1, U8 + ': bad argument') for k in ('a', 'b', 'weights', 'out', 'terms', 'ws')]
    u8 += [
        (_u8(N=-1), -1, U8 + ': bad argument'),
        (_u8(levels=6), -1, LEVELS % (U8, 6)),
        (_u8(weights=_floats(0.2, 0.1, 0.5, 0.2, 0.0)), -1, U8 + ': weights[4]=0 (every weight must be positive and finite)'),
        (_u8(W=175), -3, SIZE % (U8, 640, 175, 5, 4, 40, 10)),
        (_u8(N=65536, H=176, W=176), -3, LIMIT % (U8, 65536, 176, 176)),
        (_u8(ws_bytes=8), -1, U8 + ': workspace of 8 bytes, needs %d' % ((40 * 13 + 20 * 6 + 10 * 3 + 5 * 2 + 2 * 1) * 8)),
        (_u8(pyr_bytes=16), -1, U8 + ': pyramid of 16 bytes, needs %d' % (2 * (320 * 200 + 160 * 100 + 80 * 50 + 40 * 25) * 4)),
    ]
    bwd = [(_bwd(**{k: None}), -1, BWD + ': bad argument') for k in ('x', 'y', 'maps', 'coef', 'gout', 'dx', 'pyr')]
    bwd += [
        (_bwd(N=0), -1, BWD + ': bad argument'),
        (_bwd(dtype=BAD, levels=0), -1, BWD + ': bad dtype 7'),
        (_bwd(levels=-1), -1, LEVELS % (BWD, -1)),
        (_bwd(H=175), -3, SIZE % (BWD, 175, 256, 5, 4, 10, 16)),
        (_bwd(N=32768), -3, LIMIT % (BWD, 32768, 256, 256)),
        (_bwd(gbuf_bytes=PYR256 // 2 - 4), -1, BWD + ': gradient buffer of %d bytes, needs %d' % (PYR256 // 2 - 4, PYR256 // 2)),
        (_bwd(gbuf=None), -1, BWD + ': gradient buffer of 0 bytes, needs %d' % (PYR256 // 2)),
    ]
    return ((FWD, fwd), (U8, u8), (BWD, bwd))


def test_msssim_entry_points_reject_bad_calls_before_any_launch():
    """Null pointers, N <= 0, a bad dtype, levels outside 1..5, a weight that is not positive and finite, a short buffer: S2E_ERR_ARG; a
    last level below the window (the message names the level and its size) or a grid beyond the launch limits: S2E_ERR_UNSUPPORTED; the
    message, and which check wins.  Host-only: with a GPU visible the test skips itself, so that a dummy pointer can never reach a kernel
    (as test_ssim_entry_points_reject_bad_calls_before_any_launch does)."""
    if torch.cuda.is_available():
        pytest.skip('dummy pointers: host-only by construction')
    from seg2eye_amd import _lib
    assert (_lib.S2E_BF16, _lib.S2E_F32) == (BF16, F32)
    for name, table in _error_tables():
        check_error_table(name, table)
    with pytest.raises(_lib.Seg2EyeHipError, match='s2e_msssim_fwd failed'):
        _lib.call.s2e_msssim_fwd(*_fwd(x=None))


def test_size_queries_are_exact_monotone_and_zero_where_illegal():
    """workspace: one fp64 partial per 16 x 32 tile of positions, level and image; pyramid: levels 1.. of both images in fp32; maps: three
    fp32 planes of positions per level.  Host-only queries."""
    from seg2eye_amd import _lib
    L = _lib.lib()
    ws, pyr, maps = L.s2e_msssim_workspace_bytes, L.s2e_msssim_pyramid_bytes, L.s2e_msssim_maps_bytes
    assert isinstance(ws(1, 11, 11, 1), int) and ctypes.sizeof(ctypes.c_size_t) == 8
    assert (ws(2, 256, 256, 5), pyr(2, 256, 256, 5), maps(2, 256, 256, 5)) == (WS256, PYR256, MAPS256)
    assert (ws(1, 11, 11, 1), pyr(1, 11, 11, 1), maps(1, 11, 11, 1)) == (8, 0, 12)                   # one level: no pyramid
    assert ws(2, 256, 256, 1) == L.s2e_ssim_workspace_bytes(2, 256, 256) and maps(2, 256, 256, 1) == 3 * 2 * 246 * 246 * 4
    assert (ws(2, 22, 22, 2), pyr(2, 22, 22, 2), maps(2, 22, 22, 2)) == (2 * 2 * 8, 2 * 2 * 121 * 4, 3 * 2 * (144 + 1) * 4)
    assert (ws(1, 45, 71, 3), pyr(1, 45, 71, 3)) == ((3 * 2 + 1 + 1) * 8, 2 * (22 * 35 + 11 * 17) * 4)
    assert ws(1, 640, 400, 5) == (40 * 13 + 20 * 6 + 10 * 3 + 5 * 2 + 2 * 1) * 8
    for q in (ws, pyr, maps):
        for bad in ((0, 256, 256, 5), (-1, 256, 256, 5), (2, 175, 256, 5), (2, 256, 175, 5), (2, 256, 256, 0), (2, 256, 256, 6), (2, 21, 64, 2),
                    (2, 10, 64, 1), (2, -4, 64, 1)):
            assert q(*bad) == 0, (q, bad)
    sizes = [176, 177, 191, 192, 208, 256, 400, 640]
    for n in (1, 2, 3):
        for i, h in enumerate(sizes):
            for j, w in enumerate(sizes):
                for q in (ws, pyr, maps):
                    b = q(n, h, w, 5)
                    assert b > 0 and b % 4 == 0 and q(n + 1, h, w, 5) > b, (n, h, w)
                    assert b > q(n, h, w, 4) or q is ws and b >= q(n, h, w, 4)
                    if i:
                        assert b >= q(n, sizes[i - 1], w, 5), (n, h, w)
                    if j:
                        assert b >= q(n, h, sizes[j - 1], 5), (n, h, w)
