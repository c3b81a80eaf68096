"""The fp64 references and plan mirrors of tests/_conv3x3_child.py, on the CPU: the 3x3 convolution, its data and weight gradients
against torch's own fp64 convolution and autograd, the rectangle masks, the fused SPADE reference against the formula written out,
and the bound's absolute-value twin (it must dominate every intermediate).  No GPU needed."""
import pytest
import torch
import torch.nn.functional as F

import _conv3x3_child as T


def _t(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize('shape', [(2, 5, 7, 3, 4), (1, 16, 16, 8, 16), (3, 4, 9, 16, 5)])
def test_conv_references_match_torch_fp64(shape):
    n, h, w, ci, co = shape
    x, wt, gy = _t((n, h, w, ci), 1), _t((co, ci, 3, 3), 2), _t((n, h, w, co), 3)
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    wr = wt.clone().requires_grad_(True)
    y = F.conv2d(xr, wr, padding=1)
    y.backward(gy.permute(0, 3, 1, 2))
    assert torch.allclose(T.conv3x3_64(x, wt), y.detach().permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    assert torch.allclose(T.dgrad3x3_64(gy, wt), xr.grad.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    # the library's weight-gradient layout: (co, (ky, kx, ci))
    assert torch.allclose(T.wgrad3x3_64(x, gy), wr.grad.permute(0, 2, 3, 1).reshape(co, 9 * ci), rtol=1e-12, atol=1e-12)


def test_conv_reference_chunks_rows():
    """wide maps go through the im2col in row chunks: same result as one piece"""
    x, wt = _t((1, 9, 600, 128), 4), _t((4, 128, 3, 3), 5)
    ref = F.conv2d(x.permute(0, 3, 1, 2), wt, padding=1).permute(0, 2, 3, 1)
    assert (1 << 22) // (600 * 9 * 128) < 9
    assert torch.allclose(T.conv3x3_64(x, wt), ref, rtol=1e-12, atol=1e-12)


def test_rect_mask_numbering():
    m = T.rect_mask(2, 32, 48, [0, 5, 7])                   # 2 x 3 rectangles per sample
    assert m.shape == (2, 32, 48, 1)
    assert bool(m[0, :16, :16].all()) and int(m[0].sum()) == 512
    assert bool(m[0, 16:, 32:].all())                       # 5 = sample 0, row 1, column 2
    assert bool(m[1, :16, 16:32].all()) and int(m[1].sum()) == 256     # 7 = sample 1, row 0, column 1
    assert int(m.sum()) == 3 * 256
    assert int(T.rect_mask(1, 16, 16, []).sum()) == 0


@pytest.mark.parametrize('lrelu', [False, True])
def test_fused_reference_and_its_bound(lrelu):
    n, h, w, c, nh = 2, 4, 5, 3, 8
    actv, wq, b = torch.relu(_t((n, h, w, nh), 6)), _t((2 * c, nh, 3, 3), 7), _t((2 * c,), 8)
    x = _t((n, h, w, c), 9)
    stats = torch.stack([_t((n, c), 10), 0.5 + _t((n, c), 11).abs()], -1)
    s0, s1 = _t((n, c), 12), _t((n, c), 13)
    out, a_out, gamma, a_gamma = T.fused_ref(actv, wq, b, x, stats, s0, s1, lrelu)
    gb = F.conv2d(actv.permute(0, 3, 1, 2), wq, b, padding=1).permute(0, 2, 3, 1)
    ga, be = gb[..., :c], gb[..., c:]
    mu, rs = stats[..., 0][:, None, None], stats[..., 1][:, None, None]
    want = 0.5 * ((x - mu) * rs * (1 + ga) + be + x * (1 + s0[:, None, None]) + s1[:, None, None])
    if lrelu:
        want = F.leaky_relu(want, 0.2)
    assert torch.allclose(out, want, rtol=1e-12, atol=1e-12)
    assert torch.allclose(gamma, ga, rtol=1e-12, atol=1e-12)
    # the absolute-value twin bounds |1 + gamma|, |beta + s1| and the result
    assert bool((a_gamma >= (1 + ga).abs() - 1e-12).all())
    assert bool((a_out >= want.abs() - 1e-12).all())
    # without a bias the twin loses the bias terms
    _, a0, _, ag0 = T.fused_ref(actv, wq, None, x, stats, s0, s1, lrelu)
    assert bool((ag0 <= a_gamma).all()) and bool((a0 <= a_out).all())


def test_check_close_fails_on_nan_and_outliers():
    ref = torch.ones(4, 4, dtype=torch.float64)
    A = torch.full_like(ref, 4.0)
    T.check_close(ref.clone(), ref, A, 'same')
    got = ref.clone()
    got[1, 2] = float('nan')
    with pytest.raises(AssertionError):
        T.check_close(got, ref, A, 'nan')
    got = ref.clone()
    got[3, 0] += 2 * (T.BF16_RNE + 4 * T.C_ACC)
    with pytest.raises(AssertionError):
        T.check_close(got, ref, A, 'outlier')


def test_plan_mirrors(monkeypatch):
    assert [T.wgrad_slab(16, 64), T.wgrad_slab(16, 96), T.wgrad_slab(16, 48), T.wgrad_slab(32, 32)] == [64, 32, 16, 32]
    from seg2eye_amd._lib import SPADE_ANY_TILES
    monkeypatch.setenv('S2E_CONV_DUO', '1')
    assert T.duo_takes_fused(1, 16, 16, 64, 128, 0, 16, 16)
    assert not T.duo_takes_fused(1, 16, 16, 64, 128, SPADE_ANY_TILES, 16, 16)         # routes past the duo kernel
    assert not T.duo_takes_fused(1, 16, 16, 64, 128, 0, 32, 8)
    monkeypatch.setenv('S2E_CONV_DUO', '0')
    assert not T.duo_takes_fused(1, 16, 16, 64, 128, 0, 16, 16)
    monkeypatch.delenv('S2E_CONV_DUO')
    assert T.duo_takes_fused(2, 128, 128, 128, 128, 8, 16, 16)          # 256 items: the default threshold
    assert not T.duo_takes_fused(1, 128, 128, 128, 128, 8, 16, 16)
    for items in (511, 513, 1027):
        n, h, w = T.cap_shape(items)
        assert T.items_of(n, h, w, 64) == items and T.items_of(n, h, w, 128) == items
