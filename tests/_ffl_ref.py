"""The focal frequency loss rule of DESIGN 3.18 restated in torch on the CPU, for tests/test_ffl_host.py and tests/test_ffl_gpu.py.

For one single-channel pair x, y (H, W): d = x - y; Z = the orthonormal 2-D DFT of d; dist = Re Z^2 + Im Z^2;
w = dist^(alpha/2) / max_bins dist^(alpha/2), detached (alpha = 0: w = 1 everywhere; alpha > 0: a bin with dist = 0 has w = 0; an image
whose maximum is 0 has w = 0 everywhere); ffl = mean over the H W bins of w dist.  Gradients are autograd's -- no second hand-written formula.

Three forms of the spectrum:
  'fft'     torch.fft.fft2(norm='ortho') on the full spectrum: the fp64 ORACLE
  'matrix'  the same arithmetic as two real matrix products with the DFT matrices cos, sin (2 pi (k j mod n) / n) / sqrt(n), evaluated in
            fp64 and rounded once to `dtype`: in torch.float32 the YARDSTICK for what rounding alone costs a straightforward fp32 implementation
  'half'    the matrix form on the W/2 + 1 non-redundant columns, with the multiplicities 1 (kx = 0, and kx = W/2 when W is even) and 2"""
import math

import torch


def dft_matrices(n, dtype=torch.float64):
    """(C, S) (n, n): cos and sin of 2 pi (k j mod n) / n, times n^-1/2; the argument reduced in integers, fp64, rounded once to dtype."""
    k = torch.arange(n, dtype=torch.int64)
    ang = ((k[:, None] * k[None, :]) % n).double() * (2.0 * math.pi / n)
    s = 1.0 / math.sqrt(n)
    return (torch.cos(ang) * s).to(dtype), (torch.sin(ang) * s).to(dtype)


def multiplicities(W, dtype=torch.float64):
    """(W/2 + 1,): how many columns of the full spectrum column kx of the half stands for."""
    m = torch.full((W // 2 + 1,), 2.0, dtype=dtype)
    m[0] = 1.0
    if W % 2 == 0:
        m[W // 2] = 1.0
    return m


def spectrum(d, method='fft', dtype=torch.float64):
    """d (N,H,W) of dtype -> (Re Z, Im Z), each (N,H,W) -- or (N,H,W/2+1) for 'half'."""
    H, W = d.shape[-2:]
    if method == 'fft':
        z = torch.fft.fft2(d, norm='ortho')
        return z.real, z.imag
    ch, sh = dft_matrices(H, dtype)
    cw, sw = dft_matrices(W, dtype)
    if method == 'half':
        cw, sw = cw[:, :W // 2 + 1], sw[:, :W // 2 + 1]
    p, q = d @ cw, d @ sw                                     # the row transform: p - i q
    return ch @ p - sh @ q, -(sh @ p + ch @ q)                # (ch - i sh) (p - i q)


def ffl(x, y, alpha=1.0, dtype=torch.float64, method='fft'):
    """x, y (N,H,W) -> ffl (N,), in dtype."""
    d = x.to(dtype) - y.to(dtype)
    H, W = d.shape[-2:]
    re, im = spectrum(d, method, dtype)
    dist = re * re + im * im
    p = torch.ones_like(dist) if alpha == 0 else dist.detach() ** (alpha / 2.0)
    mx = p.amax(dim=(1, 2), keepdim=True)
    w = torch.where(mx > 0, p / torch.where(mx > 0, mx, torch.ones_like(mx)), torch.zeros_like(p)).detach()
    if method == 'half':
        return (w * dist * multiplicities(W, dtype)).sum(dim=(1, 2)) / (H * W)
    return (w * dist).sum(dim=(1, 2)) / (H * W)


def ffl_u8(a, b, alpha=1.0, dtype=torch.float64, method='fft'):
    """uint8 images 0..255: u = a / 255."""
    return ffl(a.to(dtype) / 255, b.to(dtype) / 255, alpha, dtype, method)


def ffl_and_grad(x, y, gout, alpha=1.0, dtype=torch.float64, method='fft'):
    """-> (ffl (N,), d sum(gout * ffl) / dx (N,H,W)), in dtype, for x, y given as fp64 (or exactly representable) values."""
    xx = x.to(dtype).clone().requires_grad_(True)
    f = ffl(xx, y.to(dtype), alpha, dtype, method)
    f.backward(gout.to(dtype))
    return f.detach(), xx.grad.detach()


def oracle(x, y, gout, alpha=1.0):
    return ffl_and_grad(x, y, gout, alpha, torch.float64, 'fft')


def yardstick(x, y, gout, alpha=1.0):
    return ffl_and_grad(x, y, gout, alpha, torch.float32, 'matrix')
