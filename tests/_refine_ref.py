"""The residual refiner restated in numpy / CPU torch, for the tests of seg2eye_amd/ops/refine.py, networks/refiner.py and
seg2eye_amd/refine.py: the four kernels (the network input, the loss terms with the gradient, the submission bytes; the head in fp64, or
in fp32 as the yardstick of the kernels' bound), the sampler's expected picks, the tool's training loop written a second time in fp64 on
stock CPU torch, and the data the tests use.

A frame's value is DATA here, not arithmetic under test: norm(v) = fl(fl(v * fl(2 / 255)) - 1) in fp32 is the rule (the reference's
`image *= 2.0 / 255.0; image -= 1.0` on a float32 array), so both evaluations of the head start from these fp32 values and differ in what
follows -- the sum with the residual, the clamp, the difference, the sums and the coefficients."""
import numpy as np
import torch

import _segment_ref as S

LEVELS = (125, 103, 76, 34)


# ------------------------------------------------------------------------------------------------ the four kernels
def norm(v):
    """uint8 -> fp32 in [-1, 1], two roundings."""
    x = np.asarray(v).astype(np.float32)
    x = x * np.float32(2.0 / 255.0)
    return x - np.float32(1.0)


def flipped(planes, flip):
    """Image n mirrored horizontally where flip[n] != 0 (flip None: nothing is)."""
    planes = np.asarray(planes)
    if flip is None:
        return planes
    return np.where(np.asarray(flip).astype(bool)[:, None, None], planes[:, :, ::-1], planes)


def colourise(mask, levels=LEVELS, ncls=4):
    """A label c < ncls -> levels[c]; a label >= ncls -> 0."""
    lut = np.zeros(256, dtype=np.uint8)
    lut[:ncls] = np.asarray(levels, dtype=np.uint8)[:ncls]
    return lut[np.asarray(mask)]


def refine_input(tmask, rimg, rmask, flip=None, levels=LEVELS, ncls=4, C=8):
    """-> fp32 (N, H, W, C): [norm(levels[tmask]), norm(rimg), norm(levels[rmask]), 0 ...] of the flipped planes."""
    n, h, w = np.asarray(rimg).shape
    x = np.zeros((n, h, w, C), dtype=np.float32)
    x[..., 0] = norm(colourise(flipped(tmask, flip), levels, ncls))
    x[..., 1] = norm(flipped(rimg, flip))
    x[..., 2] = norm(colourise(flipped(rmask, flip), levels, ncls))
    return x


def head(res, rimg, truth, flip=None, lambda_eds=1.0, lambda_l1=0.0, g=1.0, dtype=np.float64):
    """res (N, H, W, C) channel 0 live, rimg / truth uint8 (N, H, W) -> dict(score (N,), sumsq (N,), terms (3,), loss, grad (N, H, W, C)),
    evaluated in `dtype` from the frames' fp32 values.  An image with sumsq == 0 gets 0 for the eds part of its gradient."""
    res = np.asarray(res)
    n, h, w, _ = res.shape
    r = res[..., 0].astype(dtype)
    s = r + norm(flipped(rimg, flip)).astype(dtype)
    d = np.clip(s, dtype(-1), dtype(1)) - norm(flipped(truth, flip)).astype(dtype)
    hw, cnt = dtype(h * w), dtype(n * h * w)
    sumsq = (d * d).reshape(n, -1).sum(axis=1, dtype=dtype)
    root = np.sqrt(sumsq)
    score = dtype(127.5) * root / hw
    eds = score.sum(dtype=dtype) / dtype(n)
    l1 = np.abs(d).sum(dtype=dtype) / cnt
    terms = np.array([eds, l1, dtype(1471) * eds], dtype=dtype)
    loss = dtype(lambda_eds) * eds + dtype(lambda_l1) * l1
    safe = np.where(sumsq > 0, root, dtype(1))
    k_eds = np.where(sumsq > 0, dtype(g) * dtype(lambda_eds) * dtype(127.5) / (cnt * safe), dtype(0))
    k_l1 = dtype(g) * dtype(lambda_l1) / cnt
    passes = (s >= -1) & (s <= 1)
    grad = np.zeros(res.shape, dtype=dtype)
    grad[..., 0] = np.where(passes, k_eds[:, None, None] * d + k_l1 * np.sign(d), dtype(0))
    return dict(score=score, sumsq=sumsq, terms=terms, loss=loss, grad=grad)


def predict_u8(res, rimg, flip=None):
    """-> uint8 (N, H, W): (uint8)(127.5 (clamp(fl(res + norm(rimg)), -1, 1) + 1)) in fp32, truncated."""
    p = np.clip(np.asarray(res)[..., 0].astype(np.float32) + norm(flipped(rimg, flip)), np.float32(-1), np.float32(1))
    return (np.float32(127.5) * (p + np.float32(1.0))).astype(np.uint8)


def openeds_u8(a, b):
    """1471 x the mean over the images of sqrt(sum (a - b)^2) / (H W): the Tester's figure on uint8 images."""
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    per = np.sqrt(((a - b) ** 2).reshape(len(a), -1).sum(axis=1).astype(np.float64)) / float(a.shape[1] * a.shape[2])
    return float(per.mean() * 1471)


def to_bf16(x):
    """fp32 array -> the bf16 tensor of its values rounded to nearest even."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ data of the kernel tests
def planes(shape, seed, ncls=4):
    """-> (tmask, rimg, rmask, truth) uint8: iid labels with some values >= ncls, iid frames that hold the levels 0 and 255."""
    rng = np.random.RandomState(seed)
    tmask, rmask = (rng.randint(0, ncls + 2, shape).astype(np.uint8) for _ in range(2))
    tmask.reshape(-1)[0] = 255
    rimg, truth = (rng.randint(0, 256, shape).astype(np.uint8) for _ in range(2))
    edge = rng.rand(*shape)
    rimg[edge < 0.1] = 0
    rimg[edge > 0.9] = 255
    return tmask, rimg, rmask, truth


def residual(kind, rimg, truth, C, seed, bf16=False):
    """-> (fp32 (N, H, W, C) residuals, truth): channel 0 by `kind`, channels 1.. hold NaN, inf, -inf and 1e30 in turn (never read).
      'mixed'   N(0, 0.6): pixels clamped on both sides; every third residual exactly 0, so that frames at 0 and 255 sit exactly on
                the clamp's ends; where the residual is 0, every other truth pixel equals the frame (d == 0)
      'clampy'  N(0, 4): most pixels clamped
      'zero'    all 0
      'exact'   'mixed', but image 0 has a zero residual and truth == frame: sumsq[0] == 0
    bf16: the residuals are rounded to bf16 values first."""
    rng = np.random.RandomState(seed)
    shape = rimg.shape
    truth = truth.copy()
    r = rng.normal(0.0, 4.0 if kind == 'clampy' else 0.6, shape).astype(np.float32)
    if kind == 'zero':
        r[:] = 0
    if kind in ('mixed', 'exact'):
        zero = rng.rand(*shape) < 1 / 3
        r[zero] = 0
        same = zero & (rng.rand(*shape) < 0.5)
        truth[same] = rimg[same]
    if kind == 'exact':
        r[0] = 0
        truth[0] = rimg[0]
    if bf16:
        r = to_bf16(r).float().numpy()
    res = np.zeros(shape + (C,), dtype=np.float32)
    res[..., 0] = r
    for c in range(1, C):
        res[..., c] = (float('nan'), float('inf'), float('-inf'), 1e30)[(c - 1) % 4]
    return res, truth


def flips(kind, n, seed=0):
    """None ('none'), all 0 ('off') or mixed per image ('mixed': image 0 flipped, then at random)."""
    if kind == 'none':
        return None
    f = np.zeros(n, dtype=np.uint8)
    if kind == 'mixed':
        f[:] = np.random.RandomState(seed).rand(n) < 0.5
        f[0] = 1
        if n > 1:
            f[1] = 0
    return f


# ------------------------------------------------------------------------------------------------ the sampler
def expected_reference(store, seg, refs, key, user, fname, pos=0):
    """-> (frame, mask) of the pos-th listed candidate of a target, from the convention alone: b'g' is the person's generative frames
    with their predicted masks (for 'test': the labelled frames with their true labels), b's' the sequence frames, whose indices were
    appended behind the former."""
    e = refs[key][user][fname]
    idx, sub = int(e['index'][pos]), bytes(e['subset'][pos])
    g = store[key][user]
    first_img, first_mask = (g['images_ss'], g['labels_ss']) if key == 'test' else (g['images_gen'], seg[key][user]['labels_pred_gen'])
    if sub == b'g':
        return np.asarray(first_img[idx]), np.asarray(first_mask[idx])
    k = idx - len(first_img)
    return np.asarray(g['images_seq'][k]), np.asarray(seg[key][user]['labels_pred_seq'][k])


def target_list(store, key):
    from seg2eye_amd.style_rank import clean_filename
    label_key, names_key = ('labels_gen', 'labels_gen_filenames') if key == 'test' else ('labels_ss', 'images_ss_filenames')
    return [(u, i, clean_filename(n)) for u, g in store[key].items() if label_key in g and names_key in g for i, n in enumerate(g[names_key])]


# ------------------------------------------------------------------------------------------------ the network and the tool's loop
def manifest(nrf):
    f = nrf
    convs = [('e0', 3, f), ('e1', f, 2 * f), ('e2', 2 * f, 4 * f), ('e3', 4 * f, 8 * f), ('b', 8 * f, 8 * f), ('d2', 8 * f, 4 * f),
             ('d1', 4 * f, 2 * f), ('d0', 2 * f, f), ('out', f, 1)]
    return [e for n, ci, co in convs for e in ((n + '.weight', (co, ci, 3, 3)), (n + '.bias', (co,)))]


def net_residual(sd, x):
    """x (N, H, W, >= 3) -> the residual (N, H, W, 1) of EyeRefineNet from stock torch calls (the segmenter's body is generic in its
    channel counts), in the dtype of `sd`'s tensors."""
    x = torch.as_tensor(x)
    return S.net_forward(sd, x[..., :3].permute(0, 3, 1, 2))


def loss_torch(res, rimg, truth, lambda_eds=1.0, lambda_l1=0.0):
    """The reference's literal formulas (refinenet/model.py:38-62) on a torch residual (N, H, W, C) of any float dtype:
    clamp, sqrt(sum((255 / 2 d)^2)) / (H W) per image, mean |d|.  -> (loss, per-image score)"""
    dt = res.dtype
    n, h, w, _ = res.shape
    pred = torch.clamp(res[..., 0] + torch.from_numpy(norm(rimg)).to(dt), min=-1.0, max=1.0)
    y = torch.from_numpy(norm(truth)).to(dt)
    l1 = torch.mean(torch.abs(pred - y))
    per = torch.sqrt(torch.sum((255. / 2. * (pred - y)) ** 2, dim=[1, 2])) / float(h * w)
    return lambda_eds * torch.mean(per) + lambda_l1 * l1, per


def _batch(store, seg, refs, key, rows, pos):
    label_key = 'labels_gen' if key == 'test' else 'labels_ss'
    tmask = np.stack([np.asarray(store[key][u][label_key][i]) for u, i, _ in rows])
    ref = [expected_reference(store, seg, refs, key, u, f, p) for (u, _, f), p in zip(rows, pos)]
    rimg, rmask = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])
    truth = np.stack([np.asarray(store[key][u]['images_ss'][i]) for u, i, _ in rows])
    return tmask, rimg, rmask, truth


def evaluate_restated(sd, store, seg, refs, key):
    """-> (openeds, openeds_nn): the refined and the unrefined figure of a split, first listed reference, as seg2eye_amd.refine.evaluate."""
    rows = target_list(store, key)
    tmask, rimg, rmask, truth = _batch(store, seg, refs, key, rows, [0] * len(rows))
    with torch.no_grad():
        res = net_residual(sd, torch.from_numpy(refine_input(tmask, rimg, rmask)).to(sd['e0.weight'].dtype)).float().numpy()
    return openeds_u8(predict_u8(res, rimg), truth), openeds_u8(rimg, truth)


def train_restated(sd0, store, seg, refs, niter, batch, lr, seed, top, lambda_eds=1.0, lambda_l1=0.0):
    """seg2eye_amd.refine.train_refiner (no flip) from the rule alone, in the dtype of sd0: the same shuffled order and the same draws
    among the first `top` candidates, torch.optim.Adam(betas=(0.9, 0.999)).  -> (state dict, [loss per step])"""
    sd = {k: v.clone().requires_grad_(True) for k, v in sd0.items()}
    dt = sd0['e0.weight'].dtype
    opt = torch.optim.Adam(list(sd.values()), lr=lr, betas=(0.9, 0.999), eps=1e-8)
    samples = target_list(store, 'train')
    rng = np.random.RandomState(seed)
    losses = []
    for _ in range(niter):
        order = rng.permutation(len(samples))
        for b0 in range(0, len(order), batch):
            rows = [samples[j] for j in order[b0:b0 + batch]]
            pos = [int(rng.randint(0, min(top, len(refs['train'][u][f]['index'])))) for u, _, f in rows]
            tmask, rimg, rmask, truth = _batch(store, seg, refs, 'train', rows, pos)
            opt.zero_grad()
            loss, _ = loss_torch(net_residual(sd, torch.from_numpy(refine_input(tmask, rimg, rmask)).to(dt)), rimg, truth, lambda_eds, lambda_l1)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
    return {k: v.detach() for k, v in sd.items()}, losses
