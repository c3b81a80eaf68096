"""The MS-SSIM rule of DESIGN 3.17 restated in torch on the pieces of tests/_ssim_ref.py (F.conv2d with the outer-product window,
F.avg_pool2d for the pyramid), for tests/test_msssim_host.py and tests/test_msssim_gpu.py.  `dtype` chooses the arithmetic: torch.float64
is the oracle, torch.float32 the yardstick for what rounding alone costs a straightforward fp32 implementation.  Gradients are autograd's
-- no second hand-written formula."""
import torch
import torch.nn.functional as F

import _ssim_ref as S

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)            # Wang, Simoncelli, Bovik 2003; not renormalised
FLOOR = 1e-3                                                  # a level's mean below it counts as FLOOR and passes no gradient


def level_means(u, v, levels, dtype=torch.float64):
    """u, v (N,H,W) in [0, 1] units -> (N, levels): the mean over level j's valid positions of cs (j < levels - 1) or of S (the last)."""
    u, v = u.to(dtype), v.to(dtype)
    g = S.window(dtype)
    k = torch.outer(g, g).view(1, 1, S.TAPS, S.TAPS)
    m = lambda t: F.conv2d(t.unsqueeze(1), k)[:, 0]
    out = []
    for j in range(levels):
        mu, mv = m(u), m(v)
        su2, sv2, suv = m(u * u) - mu * mu, m(v * v) - mv * mv, m(u * v) - mu * mv
        t = (2 * suv + S.C2) / (su2 + sv2 + S.C2)
        if j == levels - 1:
            t = t * (2 * mu * mv + S.C1) / (mu * mu + mv * mv + S.C1)
        out.append(t.mean(dim=(1, 2)))
        if j < levels - 1:                                    # a trailing odd row or column is dropped
            u, v = F.avg_pool2d(u.unsqueeze(1), 2)[:, 0], F.avg_pool2d(v.unsqueeze(1), 2)[:, 0]
    return torch.stack(out, dim=1)


def combine(terms, weights):
    """(N, levels) means -> msssim (N,) = prod_j max(m_j, FLOOR)^w_j.  torch.clamp passes no gradient below the bound."""
    w = torch.tensor([float(x) for x in weights], dtype=terms.dtype)
    return (terms.clamp(min=FLOOR) ** w).prod(dim=1)


def _weights(weights):
    return WEIGHTS if weights is None else tuple(weights)


def ms_ssim_unit(u, v, weights=None, dtype=torch.float64, return_terms=False):
    w = _weights(weights)
    terms = level_means(u, v, len(w), dtype)
    out = combine(terms, w)
    return (out, terms) if return_terms else out


def ms_ssim(x, y, weights=None, dtype=torch.float64, return_terms=False):
    """x, y (N,H,W) in [-1, 1] (no clamp): u = (x + 1) / 2, v = (y + 1) / 2."""
    return ms_ssim_unit((x.to(dtype) + 1) / 2, (y.to(dtype) + 1) / 2, weights, dtype, return_terms)


def ms_ssim_u8(a, b, weights=None, dtype=torch.float64, return_terms=False):
    """uint8 images 0..255: u = a / 255."""
    return ms_ssim_unit(a.to(dtype) / 255, b.to(dtype) / 255, weights, dtype, return_terms)


def ms_ssim_and_grad(x, y, gout, weights=None, dtype=torch.float64):
    """-> (msssim (N,), terms (N, levels), d sum(gout * msssim) / dx (N,H,W)), in `dtype`, for x, y given as fp64 (or exactly representable) values."""
    xx = x.to(dtype).clone().requires_grad_(True)
    s, terms = ms_ssim(xx, y.to(dtype), weights, dtype, return_terms=True)
    s.backward(gout.to(dtype))
    return s.detach(), terms.detach(), xx.grad.detach()
