"""The SSIM rule of DESIGN 3.15 restated in torch (F.conv2d with the outer-product window), for tests/test_ssim_host.py and
tests/test_ssim_gpu.py.  `dtype` chooses the arithmetic: torch.float64 is the oracle, torch.float32 the yardstick for what rounding alone
costs a straightforward fp32 implementation.  Gradients are autograd's -- no second hand-written formula."""
import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2
TAPS = 11


def window(dtype=torch.float64):
    """11 taps exp(-(i - 5)^2 / (2 * 1.5^2)), normalised to sum 1 in fp64, then cast."""
    i = torch.arange(TAPS, dtype=torch.float64) - TAPS // 2
    g = torch.exp(-i * i / (2 * 1.5 ** 2))
    return (g / g.sum()).to(dtype)


def ssim_unit(u, v, dtype=torch.float64):
    """u, v (N,H,W) already in [0, 1] units -> ssim (N,): the mean of S over the (H-10)(W-10) valid window positions."""
    u, v = u.to(dtype), v.to(dtype)
    g = window(dtype)
    k = torch.outer(g, g).view(1, 1, TAPS, TAPS)
    m = lambda t: F.conv2d(t.unsqueeze(1), k)[:, 0]
    mu, mv = m(u), m(v)
    su2, sv2, suv = m(u * u) - mu * mu, m(v * v) - mv * mv, m(u * v) - mu * mv
    s = (2 * mu * mv + C1) * (2 * suv + C2) / ((mu * mu + mv * mv + C1) * (su2 + sv2 + C2))
    return s.mean(dim=(1, 2))


def ssim(x, y, dtype=torch.float64):
    """x, y (N,H,W) in [-1, 1] (no clamp): u = (x + 1) / 2, v = (y + 1) / 2."""
    return ssim_unit((x.to(dtype) + 1) / 2, (y.to(dtype) + 1) / 2, dtype)


def ssim_u8(a, b, dtype=torch.float64):
    """uint8 images 0..255: u = a / 255."""
    return ssim_unit(a.to(dtype) / 255, b.to(dtype) / 255, dtype)


def ssim_and_grad(x, y, gssim, dtype=torch.float64):
    """-> (ssim (N,), d sum(gssim * ssim) / dx (N,H,W)), both in `dtype`, for x, y given as fp64 (or exactly representable) values."""
    xx = x.to(dtype).clone().requires_grad_(True)
    s = ssim(xx, y.to(dtype), dtype)
    s.backward(gssim.to(dtype))
    return s.detach(), xx.grad.detach()
