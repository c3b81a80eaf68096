"""The region rule of DESIGN 3.16 restated in torch -- the label lookup by integer index, one mask per class, masked sums, the weighted
mean of the present classes' means -- for tests/test_region_host.py and tests/test_region_gpu.py.  `dtype` is the format of x, y, of the
difference d = x - y formed from them, and of the results (loss, gradient); the sums over pixels and the algebra of the classes are
float64 whatever it is, as the rule asks of every accumulation.  torch.float64 is the oracle; torch.float32 is the yardstick for rounding:
what the number format alone costs (one rounding of d, one of each result).  Gradients are autograd's -- no second hand-written formula."""
import torch


def lookup(label, H, W):
    """label (N,Hl,Wl) integer -> (N,H,W) int64: pixel (r, c) has class label[(r Hl) // H, (c Wl) // W], in integers."""
    label = torch.as_tensor(label)
    _, Hl, Wl = label.shape
    ri = (torch.arange(H, dtype=torch.int64) * Hl) // H
    ci = (torch.arange(W, dtype=torch.int64) * Wl) // W
    return label.long()[:, ri][:, :, ci]


def _masks(label, shape, ncls):
    l = lookup(label, shape[1], shape[2])
    return [(l == c) for c in range(ncls)]                    # a class >= ncls is in no mask


def stats(x, y, label, ncls, dtype=torch.float64):
    """x, y (N,H,W) -> (N, ncls, 3) float64: {count, sum |d|, sum d^2} of d = x - y (formed in `dtype`) over image n's pixels of class c."""
    d = (x.to(dtype) - y.to(dtype)).double()
    rows = []
    for m in _masks(label, d.shape, ncls):
        mf = m.double()
        rows.append(torch.stack([mf.sum(dim=(1, 2)), (d.abs() * mf).sum(dim=(1, 2)), (d * d * mf).sum(dim=(1, 2))], dim=1))
    return torch.stack(rows, dim=1)


def loss(x, y, label, weights, norm='l1', dtype=torch.float64):
    """sum over the present classes of w_c m_c / sum over them of w_c, m_c the mean of f(d) over the BATCH's pixels of class c
    (f = |d| for 'l1', d^2 for 'l2'); 0 when no class of positive weight is present.  -> 0-dim of `dtype`, differentiable in x."""
    d = (x.to(dtype) - y.to(dtype)).double()
    f = d.abs() if norm == 'l1' else d * d
    w = torch.as_tensor(weights, dtype=torch.float64)
    num, den = None, None
    for c, m in enumerate(_masks(label, d.shape, len(w))):
        n_c = int(m.sum())
        if n_c == 0:
            continue
        term = w[c] * (f[m].sum() / n_c)
        num = term if num is None else num + term
        den = w[c] if den is None else den + w[c]
    if den is None or float(den) <= 0:
        return (x.to(dtype) * 0).sum()                        # (0, with a zero gradient)
    return (num / den).to(dtype)


def coef(label, shape, weights):
    """k_c = w_c / (n_c sum_present w) in float64 (0 for an absent class, or when no weighted class is present) -> (ncls,)."""
    w = torch.as_tensor(weights, dtype=torch.float64)
    n = torch.tensor([float(m.sum()) for m in _masks(label, shape, len(w))], dtype=torch.float64)
    sw = float(w[n > 0].sum())
    if sw <= 0:
        return torch.zeros_like(w)
    return torch.where(n > 0, w / (n.clamp(min=1) * sw), torch.zeros_like(w))


def loss_and_grad(x, y, label, weights, norm='l1', g=1.0, dtype=torch.float64):
    """-> (loss, d (g loss) / dx (N,H,W)), both of `dtype`, by autograd."""
    xx = x.to(dtype).clone().requires_grad_(True)
    v = loss(xx, y, label, weights, norm, dtype)
    (v * g).backward()
    return v.detach(), xx.grad.detach()
