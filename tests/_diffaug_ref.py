"""The differentiable augmentation of the discriminator's input restated in fp64 with differentiable torch ops: the
reference of test_diffaug_host.py / test_diffaug_gpu.py.  Its backward is autograd's -- no second hand-written formula."""
import torch

IDENTITY = [0.0, 1.0, 0, 0, 0, 0, 0, 0]


def plain_concat(label, fake, real, ncls=4, cpad=8):
    """cat_batch([cat_ch(one_hot(label), fake); cat_ch(one_hot(label), real)]) as (2N,H,W,cpad) fp64, zero pad channels: what
    ops.d_input builds."""
    n, H, W = label.shape
    out = torch.zeros(2 * n, H, W, cpad, dtype=torch.float64)
    for half, img in ((0, fake), (1, real)):
        o = out[half * n:(half + 1) * n]
        for k in range(ncls):
            o[..., k] = (label == k).double()
        o[..., ncls] = img.double().reshape(n, H, W)
    return out


def visible_mask(row, H, W):
    """(visible (H,W) bool, source rows (H,W) long, source columns (H,W) long -- clamped into the image) of one parameter row."""
    ty, tx, y0, x0, ch, cw = (int(v) for v in row[2:])
    y = torch.arange(H).view(H, 1).expand(H, W)
    x = torch.arange(W).view(1, W).expand(H, W)
    sy, sx = y - ty, x - tx
    inside = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
    cut = (y >= y0) & (y < y0 + ch) & (x >= x0) & (x < x0 + cw)
    return inside & ~cut, sy.clamp(0, H - 1), sx.clamp(0, W - 1)


def d_input_aug_ref(label, fake, real, rows, ncls=4, cpad=8, color=True):
    """label (N,H,W) integer, fake / real (N,H,W) fp64 (fake may require grad), rows (N,8) -> (2N,H,W,cpad) fp64.  Row i serves fake i
    and real i; color=False: b and c are not read."""
    n, H, W = label.shape
    rows = torch.as_tensor(rows, dtype=torch.float64).reshape(n, 8)
    zero = torch.zeros(H, W, dtype=torch.float64)
    halves = []
    for img in (fake.reshape(n, H, W), real.reshape(n, H, W)):
        samples = []
        for i in range(n):
            vis, sy, sx = visible_mask(rows[i].tolist(), H, W)
            b, c = (rows[i, 0], rows[i, 1]) if color else (0.0, 1.0)
            v = img[i].double()
            o = (1.0 - c) * v.mean() + b
            chans = [torch.where(vis & (label[i][sy, sx] == k), 1.0, 0.0).double() for k in range(ncls)]
            chans.append(torch.where(vis, c * v[sy, sx] + o, zero))
            chans += [zero] * (cpad - ncls - 1)
            samples.append(torch.stack(chans, dim=-1))
        halves.append(torch.stack(samples))
    return torch.cat(halves)
