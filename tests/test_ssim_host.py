"""SSIM without a GPU: the torch restatement of the rule (tests/_ssim_ref.py) checked alone, the two flags, and what the
four entry points answer before any launch."""
import ctypes

import pytest
import torch

import _ssim_ref as R
from _quality_harness import check_error_table

F32, BF16, BAD = 0, 1, 7
P = 4096                                                      # a dummy non-null pointer: must never reach a kernel
BIG = 1 << 20                                                 # a workspace size that is never short


# ------------------------------------------------------------------------------------------------ the restatement
def _iid(n, H, W, seed):
    return torch.rand(n, H, W, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2 - 1


def test_window_sums_to_one_and_is_symmetric():
    g = R.window()
    assert g.dtype == torch.float64 and g.shape == (11,) and abs(float(g.sum()) - 1.0) < 1e-15
    assert torch.equal(g, g.flip(0)) and float(g[5]) == float(g.max())
    assert abs(float(g[4] / g[5]) - 0.8007374029168081) < 1e-15                     # exp(-1 / 4.5)


def test_identical_images_score_one_with_no_gradient():
    x = _iid(3, 19, 23, 1)
    s, g = R.ssim_and_grad(x, x.clone(), torch.tensor([1.0, -2.0, 0.5], dtype=torch.float64))
    assert s.shape == (3,) and float((s - 1).abs().max()) <= 1e-12
    assert g.shape == x.shape and float(g.abs().max()) < 1e-12


def test_constant_images_give_the_closed_form():
    for a, b in ((0.25, 0.75), (0.9, 0.88), (0.0, 1.0), (0.5, 0.5)):
        x = torch.full((2, 13, 16), 2 * a - 1, dtype=torch.float64)
        y = torch.full((2, 13, 16), 2 * b - 1, dtype=torch.float64)
        want = (2 * a * b + R.C1) / (a * a + b * b + R.C1)
        assert float((R.ssim(x, y) - want).abs().max()) <= 1e-9, (a, b)
        a8, b8 = torch.full((1, 11, 11), int(a * 255), dtype=torch.uint8), torch.full((1, 11, 11), int(b * 255), dtype=torch.uint8)
        ua, ub = int(a * 255) / 255, int(b * 255) / 255
        assert abs(float(R.ssim_u8(a8, b8)) - (2 * ua * ub + R.C1) / (ua * ua + ub * ub + R.C1)) <= 1e-9


def test_one_position_by_hand():
    """An 11 x 11 image has one window position: S from the weighted moments written out, in fp64."""
    x, y = _iid(1, 11, 11, 2), _iid(1, 11, 11, 3)
    u, v = (x[0] + 1) / 2, (y[0] + 1) / 2
    w = torch.outer(R.window(), R.window())
    mu, mv = float((w * u).sum()), float((w * v).sum())
    su2, sv2, suv = float((w * u * u).sum()) - mu * mu, float((w * v * v).sum()) - mv * mv, float((w * u * v).sum()) - mu * mv
    want = (2 * mu * mv + R.C1) * (2 * suv + R.C2) / ((mu * mu + mv * mv + R.C1) * (su2 + sv2 + R.C2))
    assert abs(float(R.ssim(x, y)) - want) <= 1e-13
    assert R.ssim(_iid(2, 12, 17, 4), _iid(2, 12, 17, 5)).shape == (2,)


# ------------------------------------------------------------------------------------------------ the flags
def test_flags_parse_and_default_off():
    from seg2eye_amd.options import default_opt, parse
    o = parse(['--lambda_ssim', '2'])
    assert o.lambda_ssim == 2.0 and o.val_ssim is False and parse([]).lambda_ssim == 0.0
    t = parse(['--val_ssim'], is_train=False)
    assert t.val_ssim is True and t.lambda_ssim == 0.0 and parse([], is_train=False).val_ssim is False
    assert parse(['--val_ssim']).val_ssim is True                                   # train.py's periodic validation takes it too
    assert default_opt(lambda_ssim=1.0).lambda_ssim == 1.0 and default_opt().lambda_ssim == 0.0
    with pytest.raises(SystemExit):
        parse(['--lambda_ssim', '1'], is_train=False)                               # a training flag only


def test_ops_refuse_cpu_tensors():
    from seg2eye_amd import _lib, ops
    x = torch.zeros(2, 1, 16, 16)
    with pytest.raises(_lib.Seg2EyeHipError, match='GPU only'):
        ops.ssim(x, x)
    with pytest.raises(_lib.Seg2EyeHipError, match='GPU only'):
        ops.ssim_u8(x.to(torch.uint8), x.to(torch.uint8))
    with pytest.raises(ValueError, match='uint8'):
        ops.ssim_u8(x, x)
    assert ops.ssim is ops.losses.ssim and ops.SsimFn is ops.losses.SsimFn


# ------------------------------------------------------------------------------------------------ the entry points, before any launch
SIZE = 's2e_ssim_%s: H=%d W=%d (an image smaller than the 11 x 11 window has no position)'
LIMIT = 's2e_ssim_%s: N=%d H=%d W=%d is beyond the launch limits (N <= 65535, N H W < 2^31)'
#              dtype x  y  N  H   W  ssim maps ws  ws_bytes stream
FWD_ERRORS = [
    ((BF16, None, P, 2, 16, 16, P, P, P, BIG, None), -1, 's2e_ssim_fwd: bad argument'),
    ((BF16, P, None, 2, 16, 16, P, P, P, BIG, None), -1, 's2e_ssim_fwd: bad argument'),
    ((F32, P, P, 2, 16, 16, None, P, P, BIG, None), -1, 's2e_ssim_fwd: bad argument'),
    ((F32, P, P, 2, 16, 16, P, None, None, BIG, None), -1, 's2e_ssim_fwd: bad argument'),
    ((F32, P, P, 0, 16, 16, P, P, P, BIG, None), -1, 's2e_ssim_fwd: bad argument'),
    ((BAD, P, P, 2, 10, 16, P, P, P, BIG, None), -1, 's2e_ssim_fwd: bad dtype 7'),                 # the dtype before the size
    ((BF16, P, P, 2, 10, 16, P, P, P, BIG, None), -3, SIZE % ('fwd', 10, 16)),
    ((BF16, P, P, 2, 16, 10, P, None, P, BIG, None), -3, SIZE % ('fwd', 16, 10)),
    ((BF16, P, P, 2, 0, 16, P, P, P, BIG, None), -3, SIZE % ('fwd', 0, 16)),
    ((F32, P, P, 65536, 16, 16, P, P, P, BIG, None), -3, LIMIT % ('fwd', 65536, 16, 16)),
    ((F32, P, P, 8, 16384, 16384, P, P, P, BIG, None), -3, LIMIT % ('fwd', 8, 16384, 16384)),
    ((F32, P, P, 2, 256, 256, P, P, P, 2 * 16 * 8 * 8 - 1, None), -1, 's2e_ssim_fwd: workspace of 2047 bytes, needs 2048'),
    ((F32, P, P, 2, 10, 256, P, P, P, 0, None), -3, SIZE % ('fwd', 10, 256)),                      # the size before the workspace
]
#             a  b  N  H   W  ssim ws ws_bytes stream
U8_ERRORS = [
    ((None, P, 1, 640, 400, P, P, BIG, None), -1, 's2e_ssim_u8: bad argument'),
    ((P, None, 1, 640, 400, P, P, BIG, None), -1, 's2e_ssim_u8: bad argument'),
    ((P, P, 1, 640, 400, None, P, BIG, None), -1, 's2e_ssim_u8: bad argument'),
    ((P, P, 1, 640, 400, P, None, BIG, None), -1, 's2e_ssim_u8: bad argument'),
    ((P, P, -1, 640, 400, P, P, BIG, None), -1, 's2e_ssim_u8: bad argument'),
    ((P, P, 1, 640, 7, P, P, BIG, None), -3, SIZE % ('u8', 640, 7)),
    ((P, P, 65536, 11, 11, P, P, BIG, None), -3, LIMIT % ('u8', 65536, 11, 11)),
    ((P, P, 1, 640, 400, P, P, 40 * 13 * 8 - 8, None), -1, 's2e_ssim_u8: workspace of 4152 bytes, needs 4160'),
]
#              dtype x  y  maps gssim N  H   W  dx stream
BWD_ERRORS = [
    ((BF16, None, P, P, P, 2, 16, 16, P, None), -1, 's2e_ssim_bwd: bad argument'),
    ((BF16, P, None, P, P, 2, 16, 16, P, None), -1, 's2e_ssim_bwd: bad argument'),
    ((F32, P, P, None, P, 2, 16, 16, P, None), -1, 's2e_ssim_bwd: bad argument'),
    ((F32, P, P, P, None, 2, 16, 16, P, None), -1, 's2e_ssim_bwd: bad argument'),
    ((F32, P, P, P, P, 2, 16, 16, None, None), -1, 's2e_ssim_bwd: bad argument'),
    ((F32, P, P, P, P, 0, 16, 16, P, None), -1, 's2e_ssim_bwd: bad argument'),
    ((BAD, P, P, P, P, 2, 16, 16, P, None), -1, 's2e_ssim_bwd: bad dtype 7'),
    ((BF16, P, P, P, P, 2, 16, 10, P, None), -3, SIZE % ('bwd', 16, 10)),
    ((BF16, P, P, P, P, 2, 10, 16, P, None), -3, SIZE % ('bwd', 10, 16)),
    ((F32, P, P, P, P, 32768, 256, 256, P, None), -3, LIMIT % ('bwd', 32768, 256, 256)),
]


def test_ssim_entry_points_reject_bad_calls_before_any_launch():
    """Null pointers, N <= 0, a bad dtype, a short workspace: S2E_ERR_ARG; an image below the window or a grid beyond the launch limits:
    S2E_ERR_UNSUPPORTED; the message, and which check wins.  Host-only: with a GPU visible the test skips itself, so that a dummy pointer
    can never reach a kernel (as test_dtype_entry_points_reject_bad_calls_before_any_launch does)."""
    if torch.cuda.is_available():
        pytest.skip('dummy pointers: host-only by construction')
    from seg2eye_amd import _lib
    assert (_lib.S2E_BF16, _lib.S2E_F32) == (BF16, F32)
    for name, table in (('s2e_ssim_fwd', FWD_ERRORS), ('s2e_ssim_u8', U8_ERRORS), ('s2e_ssim_bwd', BWD_ERRORS)):
        check_error_table(name, table)
    with pytest.raises(_lib.Seg2EyeHipError, match='s2e_ssim_fwd failed'):
        _lib.call.s2e_ssim_fwd(*FWD_ERRORS[0][0])


def test_workspace_bytes_is_positive_and_monotone():
    """One fp64 partial per 16 x 32 tile of positions and image: positive for every legal size, never smaller for a larger N, H or W,
    0 where there is nothing to score.  A host-only query."""
    from seg2eye_amd import _lib
    ws = _lib.lib().s2e_ssim_workspace_bytes
    assert isinstance(ws(1, 11, 11), int) and ws(1, 11, 11) == 8 and ws(2, 256, 256) == 2 * 16 * 8 * 8 and ws(1, 640, 400) == 40 * 13 * 8
    assert ws(0, 64, 64) == 0 and ws(2, 10, 64) == 0 and ws(2, 64, 10) == 0 and ws(-1, 64, 64) == 0
    sizes = [11, 12, 26, 27, 42, 43, 64, 100, 256, 400, 640]
    for n in (1, 2, 3, 8):
        for i, h in enumerate(sizes):
            for j, w in enumerate(sizes):
                b = ws(n, h, w)
                assert b > 0 and b % 8 == 0 and ws(n + 1, h, w) > b, (n, h, w)
                if i:
                    assert b >= ws(n, sizes[i - 1], w), (n, h, w)
                if j:
                    assert b >= ws(n, h, sizes[j - 1]), (n, h, w)
    assert ws(1, 27, 11) > ws(1, 26, 11) and ws(1, 11, 43) > ws(1, 11, 42)          # a 17th row / 33rd column of positions: one more tile
    assert ctypes.sizeof(ctypes.c_size_t) == 8
