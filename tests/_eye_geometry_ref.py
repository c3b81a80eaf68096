"""The eye-geometry rules (include/seg2eye_hip.h) restated in numpy, for the tests of seg2eye_amd/ops/geometry.py and
seg2eye_amd/eye_geometry.py: the rim by shifted boolean arrays (and by a literal per-pixel loop, for small maps), the moments in
Python integers, the repaint in fp64 numpy in the stated association, a fit from the points themselves that shares nothing with
`ellipse_from_moments` but numpy, stand-ins for the two ops, and the maps the tests fit: occluded eyes and frayed borders.  The integer
results are compared with ==; the independent fit to a tolerance the tests state."""
import functools

import numpy as np
import torch

IJ = [(0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2), (3, 0), (2, 1), (1, 2), (0, 3), (4, 0), (3, 1), (2, 2), (1, 3), (0, 4)]


def default_curves(ncls):
    return (((2, 3), (1,)), ((3,), (2,))) if ncls >= 4 else (((ncls - 1,), (ncls - 2,)),)


# ------------------------------------------------------------------------------------------------ the rim
def _member(lab, classes, ncls):
    return np.isin(lab, [c for c in classes if c < ncls]) & (lab < ncls)


def rim_mask(lab, curve, ncls):
    """lab (H, W) uint8, curve (in classes, out classes) -> bool (H, W): in an `in` class with a 4-neighbour inside the frame in `out`."""
    inside, outside = _member(lab, curve[0], ncls), _member(lab, curve[1], ncls)
    near = np.zeros_like(outside)
    near[1:] |= outside[:-1]
    near[:-1] |= outside[1:]
    near[:, 1:] |= outside[:, :-1]
    near[:, :-1] |= outside[:, 1:]
    return inside & near


def rim_mask_loop(lab, curve, ncls):
    """The same, pixel by pixel."""
    H, W = lab.shape
    out = np.zeros((H, W), dtype=bool)
    for y in range(H):
        for x in range(W):
            l = int(lab[y, x])
            if l >= ncls or l not in curve[0]:
                continue
            for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                yy, xx = y + dy, x + dx
                if 0 <= yy < H and 0 <= xx < W and int(lab[yy, xx]) < ncls and int(lab[yy, xx]) in curve[1]:
                    out[y, x] = True
    return out


def moments_of_points(xs, ys):
    """The row of rim for the points (xs, ys): n, ox, oy and the 15 centred sums, in Python integers."""
    xs, ys = [int(v) for v in xs], [int(v) for v in ys]
    n = len(xs)
    ox, oy = ((2 * sum(xs) + n) // (2 * n), (2 * sum(ys) + n) // (2 * n)) if n else (0, 0)
    row = [n, ox, oy]
    for i, j in IJ:
        row.append(sum((x - ox) ** i * (y - oy) ** j for x, y in zip(xs, ys)))
    return row


def rim_moments(labels, ncls=4, curves=None):
    """labels (N, H, W) uint8 -> int64 (N, K, 18).  The sums are taken in int64 (the header's bound: below 2^60) with numpy for speed;
    moments_of_points is the same in Python integers and the host tests compare the two."""
    curves = default_curves(ncls) if curves is None else curves
    out = np.zeros((len(labels), len(curves), 18), dtype=np.int64)
    for n, lab in enumerate(labels):
        for k, curve in enumerate(curves):
            ys, xs = np.nonzero(rim_mask(lab, curve, ncls))
            cnt = len(xs)
            if not cnt:
                continue
            xs, ys = xs.astype(np.int64), ys.astype(np.int64)
            ox, oy = (2 * int(xs.sum()) + cnt) // (2 * cnt), (2 * int(ys.sum()) + cnt) // (2 * cnt)
            u, v = xs - ox, ys - oy
            out[n, k, :3] = cnt, ox, oy
            out[n, k, 3:] = [int((u ** i * v ** j).sum()) for i, j in IJ]
    return out


# ------------------------------------------------------------------------------------------------ the repaint
def paint(labels, conic, origin, valid, ncls=4, paint=None, keep=(0,), base=1):
    """The rule of s2e_ellipse_paint in fp64 numpy: every product and sum rounded once, in the header's association."""
    K = conic.shape[1]
    paint = tuple(c[0][0] for c in default_curves(ncls)) if paint is None else paint
    out = labels.copy()
    N, H, W = labels.shape
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    for n in range(N):
        if not valid[n].all():
            continue
        free = (labels[n] < ncls) & ~np.isin(labels[n], list(keep))
        cls = np.full((H, W), base, dtype=np.uint8)
        for k in range(K):
            A, B, C, D, E, F = (np.float64(v) for v in conic[n, k])
            u, v = (xx - int(origin[n, k, 0])).astype(np.float64), (yy - int(origin[n, k, 1])).astype(np.float64)
            with np.errstate(all='ignore'):
                Q = (((((A * u) * u + (B * u) * v) + (C * v) * v) + D * u) + E * v) + F
                cls[Q <= 0] = paint[k]
        out[n][free] = cls[free]
    return out


# ------------------------------------------------------------------------------------------------ an independent fit
def fit_points(xs, ys):
    """The direct least-squares ellipse through the points themselves -> (cx, cy, a, b, theta) or None: the design matrix about the
    points' float mean, the constrained eigenproblem per mask through np.linalg.eig, the axes through np.linalg.eigh of the 2 x 2 form."""
    xs, ys = np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)
    mx, my = xs.mean(), ys.mean()
    x, y = xs - mx, ys - my
    D1, D2 = np.stack([x * x, x * y, y * y], axis=1), np.stack([x, y, np.ones_like(x)], axis=1)
    S1, S2, S3 = D1.T @ D1, D1.T @ D2, D2.T @ D2
    T = -np.linalg.solve(S3, S2.T)
    M = np.linalg.solve(np.array([[0, 0, 2.0], [0, -1.0, 0], [2.0, 0, 0]]), S1 + S2 @ T)
    w, vec = np.linalg.eig(M)
    vec = np.real(vec)
    cond = 4 * vec[0] * vec[2] - vec[1] ** 2
    if not (cond > 0).any():
        return None
    a1 = vec[:, np.argmax(cond)]
    A, B, C, D, E, F = np.concatenate([a1, T @ a1])
    Q2 = np.array([[A, B / 2], [B / 2, C]])
    centre = np.linalg.solve(2 * Q2, -np.array([D, E]))
    f0 = F + 0.5 * (D * centre[0] + E * centre[1])
    lam, dirs = np.linalg.eigh(Q2 / -f0)                      # ascending: the major axis first
    d = dirs[:, 0]
    theta = np.arctan2(d[1], d[0])
    theta = theta - np.pi if theta > np.pi / 2 else theta + np.pi if theta <= -np.pi / 2 else theta
    return centre[0] + mx, centre[1] + my, 1 / np.sqrt(lam[0]), 1 / np.sqrt(lam[1]), theta


# ------------------------------------------------------------------------------------------------ stand-ins for the ops
class FakeOps:
    """rim_moments and ellipse_paint of seg2eye_amd.ops.geometry on CPU tensors, through the restatement."""

    @staticmethod
    def rim_moments(labels, ncls=4, curves=None):
        return torch.from_numpy(rim_moments(labels.cpu().numpy(), ncls, curves))

    @staticmethod
    def ellipse_paint(labels, conic, origin, valid, ncls=4, paint_classes=None, keep=(0,), base=1):
        return torch.from_numpy(paint(labels.cpu().numpy(), conic.cpu().numpy(), origin.cpu().numpy(), valid.cpu().numpy(), ncls, paint_classes, keep, base))


def fake_mask_clean(labels, ncls=4, conn=8, modes=None, return_stats=False):
    import _mask_clean_ref as MC
    out, stats, _ = MC.clean_batch(labels.cpu().numpy(), ncls, conn, modes)
    out, stats = torch.from_numpy(out), torch.from_numpy(stats)
    return (out, stats) if return_stats else out


def install(monkeypatch):
    """Put the restatements in the ops' place (ops.geometry's two functions, ops.mask_clean.mask_clean), for stages run without a GPU."""
    from seg2eye_amd.ops import geometry as G, mask_clean as M
    monkeypatch.setattr(G, 'rim_moments', FakeOps.rim_moments)
    monkeypatch.setattr(G, 'ellipse_paint', FakeOps.ellipse_paint)
    monkeypatch.setattr(M, 'mask_clean', fake_mask_clean)


# ------------------------------------------------------------------------------------------------ data
def _ellipse(yy, xx, cx, cy, a, b, t):
    c, s = np.cos(t), np.sin(t)
    u, v = (xx - cx) * c + (yy - cy) * s, -(xx - cx) * s + (yy - cy) * c
    return (u / a) ** 2 + (v / b) ** 2 <= 1.0


OCCLUDED_SEED = 20


@functools.lru_cache(maxsize=None)
def occluded(count, H=640, W=400, seed=OCCLUDED_SEED):
    """-> (masks uint8 (count, H, W), pupil (count, 5), iris (count, 5): cx, cy, a, b, theta, cut (count,)).  A rotated elliptical iris
    and pupil (axis ratio 0.75 ... 1) on sclera, an upper lid that cuts 10 ... 100 % of the pupil's upper half and a lower lid across the
    iris; beyond the lids is skin.  Sizes scale with W / 400."""
    rng = np.random.RandomState(seed)
    s = W / 400.0
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    masks = np.zeros((count, H, W), dtype=np.uint8)
    pupil, iris, cut = np.zeros((count, 5)), np.zeros((count, 5)), np.zeros(count)
    for i in range(count):
        icx, icy = W / 2 + s * rng.uniform(-40, 40), H / 2 + s * rng.uniform(-40, 40)
        ia = s * rng.uniform(90, 130)
        ib, it = ia * rng.uniform(0.75, 1.0), rng.uniform(-np.pi / 2, np.pi / 2)
        pcx, pcy = icx + s * rng.uniform(-5, 5), icy + s * rng.uniform(-5, 5)
        pa = s * rng.uniform(30, 50)
        pb, pt = pa * rng.uniform(0.75, 1.0), rng.uniform(-np.pi / 2, np.pi / 2)
        cut[i] = rng.uniform(0.1, 1.0)
        half = np.sqrt((pa * np.sin(pt)) ** 2 + (pb * np.cos(pt)) ** 2)                 # the pupil's vertical half-extent
        top = pcy - half * (1.0 - cut[i])
        bottom = icy + ib * rng.uniform(0.7, 0.95)
        upper = top + rng.uniform(0.15, 0.45) * (xx - pcx) ** 2 / (W * 1.0)
        lower = bottom - rng.uniform(0.15, 0.45) * (xx - icx) ** 2 / (W * 1.0)
        m = np.zeros((H, W), dtype=np.uint8)
        m[(yy > upper) & (yy < lower)] = 1
        opening = m == 1
        m[opening & _ellipse(yy, xx, icx, icy, ia, ib, it)] = 2
        m[opening & _ellipse(yy, xx, pcx, pcy, pa, pb, pt)] = 3
        masks[i] = m
        pupil[i], iris[i] = (pcx, pcy, pa, pb, pt), (icx, icy, ia, ib, it)
    for a in (masks, pupil, iris, cut):
        a.setflags(write=False)
    return masks, pupil, iris, cut


def frayed(mask, seed, share=0.35, reach=2):
    """mask (H, W) -> a copy in which `share` of the pixels within `reach` of a class border took the class across that border (the
    nearest differing class in the order of the offsets below)."""
    rng = np.random.RandomState(seed)
    H, W = mask.shape
    other = np.full((H, W), 255, dtype=np.uint8)
    offsets = sorted(((dy, dx) for dy in range(-reach, reach + 1) for dx in range(-reach, reach + 1) if (dy, dx) != (0, 0)),
                     key=lambda o: (o[0] ** 2 + o[1] ** 2, o))
    for dy, dx in offsets:
        ya, yb = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
        xa, xb = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
        there = mask[ya, xa]                                           # the pixel at (y + dy, x + dx) of the pixels in [yb, xb]
        take = (other[yb, xb] == 255) & (there != mask[yb, xb])
        other[yb, xb] = np.where(take, there, other[yb, xb])
    flip = (other != 255) & (rng.rand(H, W) < share)
    return np.where(flip, other, mask).astype(np.uint8)


def iou(a, b, c):
    inter, union = ((a == c) & (b == c)).sum(), ((a == c) | (b == c)).sum()
    return inter / union if union else 1.0
