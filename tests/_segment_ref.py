"""The eye segmenter restated in numpy / CPU torch, for the tests of seg2eye_amd/ops/segment.py, networks/segmenter.py and
seg2eye_amd/segment.py: the weighted softmax cross-entropy with its gradient (in fp64, or in fp32 as the yardstick of the kernels'
bound), the argmax of bilinearly resized logits with the top-two gap of every pixel, the confusion matrix, the network from stock torch
calls, the tool's training loop written a second time in fp64, and the data the tests use."""
import numpy as np
import torch
import torch.nn.functional as F


# ------------------------------------------------------------------------------------------------ cross-entropy
def ce(logits, label, w, ncls, dtype=np.float64):
    """logits (N, H, W, C) with C >= ncls, label (N, H, W) uint8, w (ncls,) -> (loss, gradient (N, H, W, C)), evaluated in `dtype`:
    sum_p w[l_p] (lse_p - z_{p, l_p}) / sum_p w[l_p] over the pixels whose label is < ncls; 0 when that is no pixel."""
    z = np.asarray(logits)[..., :ncls].astype(dtype)
    label = np.asarray(label)
    w = np.asarray(w, dtype=dtype)
    valid = label < ncls
    l = np.where(valid, label, 0).astype(np.int64)
    wl = np.where(valid, w[l], dtype(0))
    m = z.max(axis=-1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(axis=-1, keepdims=True)
    zl = np.take_along_axis(z, l[..., None], axis=-1)
    per = (np.log(s) - (zl - m))[..., 0]
    den = wl.sum(dtype=dtype)
    grad = np.zeros(np.asarray(logits).shape, dtype=dtype)
    if not den > 0:
        return dtype(0), grad
    loss = (wl * per).sum(dtype=dtype) / den
    onehot = np.arange(ncls)[None, None, None, :] == l[..., None]
    grad[..., :ncls] = (wl / den)[..., None] * (e / s - onehot.astype(dtype))
    return loss, grad


# ------------------------------------------------------------------------------------------------ argmax of resized logits
def _taps(n_out, n_in):
    f = np.maximum((np.arange(n_out, dtype=np.float64) + 0.5) * (n_in / n_out) - 0.5, 0.0)
    i0 = np.minimum(np.floor(f).astype(np.int64), n_in - 1)
    return i0, np.minimum(i0 + 1, n_in - 1), f - i0


def resized(logits, Ho, Wo, ncls):
    """The first ncls channels of (N, h, w, C) logits resized to (N, Ho, Wo, ncls) in fp64: F.interpolate(mode='bilinear',
    align_corners=False), source coordinate (d + 0.5) in / out - 0.5 clamped at 0."""
    z = np.asarray(logits)[..., :ncls].astype(np.float64)
    y0, y1, ly = _taps(Ho, z.shape[1])
    x0, x1, lx = _taps(Wo, z.shape[2])
    ly, lx = ly[None, :, None, None], lx[None, None, :, None]
    top = (1 - lx) * z[:, y0][:, :, x0] + lx * z[:, y0][:, :, x1]
    bot = (1 - lx) * z[:, y1][:, :, x0] + lx * z[:, y1][:, :, x1]
    return (1 - ly) * top + ly * bot


def argmax_resized(logits, Ho, Wo, ncls):
    """-> (mask uint8 (N, Ho, Wo): the lowest class among the largest resized logits, gap (N, Ho, Wo): largest minus second largest)."""
    v = resized(logits, Ho, Wo, ncls)
    mask = v.argmax(axis=-1).astype(np.uint8)                # (np.argmax: the first of equal maxima)
    if ncls == 1:
        return mask, np.full(mask.shape, np.inf)
    s = np.sort(v, axis=-1)
    return mask, s[..., -1] - s[..., -2]


# ------------------------------------------------------------------------------------------------ confusion matrix
def confusion(pred, truth, ncls):
    """-> int64 (ncls, ncls), row = truth, column = pred; a pair with a value >= ncls is skipped."""
    p, t = np.asarray(pred).reshape(-1).astype(np.int64), np.asarray(truth).reshape(-1).astype(np.int64)
    keep = (p < ncls) & (t < ncls)
    return np.bincount(t[keep] * ncls + p[keep], minlength=ncls * ncls).reshape(ncls, ncls).astype(np.int64)


def scores(conf):
    c = np.asarray(conf, dtype=np.float64)
    inter, union = np.diag(c), c.sum(0) + c.sum(1) - np.diag(c)
    seen = union > 0
    return {'miou': float((inter[seen] / union[seen]).mean()) if seen.any() else 0.0, 'acc': float(inter.sum() / max(c.sum(), 1.0))}


# ------------------------------------------------------------------------------------------------ the network
def net_forward(sd, x):
    """EyeSegNet from stock torch calls, in the dtype of `sd`'s tensors: x (N, 1, H, W) -> logits (N, H, W, label_nc)."""
    def block(h, name, stride=1, res=None):
        y = F.conv2d(h, sd[name + '.weight'], sd[name + '.bias'], stride=stride, padding=1)
        if res is not None:
            y = y + res
        return F.leaky_relu(F.instance_norm(y, eps=1e-5), 0.2)

    def up(h):
        return F.interpolate(h, scale_factor=2, mode='nearest')
    x = x.to(sd['e0.weight'].dtype)
    e0 = block(x, 'e0')
    e1 = block(e0, 'e1', 2)
    e2 = block(e1, 'e2', 2)
    e3 = block(e2, 'e3', 2)
    b = block(e3, 'b')
    d2 = block(up(b), 'd2', 1, e2)
    d1 = block(up(d2), 'd1', 1, e1)
    d0 = block(up(d1), 'd0', 1, e0)
    return F.conv2d(d0, sd['out.weight'], sd['out.bias'], padding=1).permute(0, 2, 3, 1)


def ce_torch(logits, label, w=None):
    """F.cross_entropy on NHWC logits (labels >= the channel count are ignored), CPU torch of any float dtype."""
    ncls = logits.shape[-1]
    t = torch.where(label < ncls, label.long(), torch.full_like(label.long(), 255))
    return F.cross_entropy(logits.permute(0, 3, 1, 2), t, weight=w, ignore_index=255, reduction='mean')


def hash_state(net_or_manifest, seed=0, dtype=torch.float64):
    """{key: tensor} of the hash fill (synthetic.fill_state_dict) for a network or a [(key, shape)] manifest."""
    from seg2eye_amd.synthetic import fill_state_dict
    man = net_or_manifest if isinstance(net_or_manifest, list) else [(k, tuple(v.shape)) for k, v in net_or_manifest.state_dict().items()]
    return {k: torch.from_numpy(v).to(dtype) for k, v in fill_state_dict(man, seed).items()}


def manifest(nsf, label_nc=4):
    f = nsf
    convs = [('e0', 1, f), ('e1', f, 2 * f), ('e2', 2 * f, 4 * f), ('e3', 4 * f, 8 * f), ('b', 8 * f, 8 * f), ('d2', 8 * f, 4 * f),
             ('d1', 4 * f, 2 * f), ('d0', 2 * f, f), ('out', f, label_nc)]
    return [e for n, ci, co in convs for e in ((n + '.weight', (co, ci, 3, 3)), (n + '.bias', (co,)))]


# ------------------------------------------------------------------------------------------------ the tool's input path and loop
def host_input(frames, hw):
    """frames (n, H, W) uint8 -> (n, 1, h, w) fp32 in [-1, 1]: Pillow's bicubic resize, then ToTensor + Normalize(0.5, 0.5)."""
    from seg2eye_amd.ops.preprocess import normalize_lut, resize_bicubic_u8_reference
    lut = normalize_lut().numpy()
    return torch.from_numpy(np.stack([lut[resize_bicubic_u8_reference(f, hw[1], hw[0])] for f in np.asarray(frames)]))[:, None]


def host_labels(labels, hw):
    from seg2eye_amd.ops.preprocess import nearest_index
    labels = np.asarray(labels)
    return labels[:, nearest_index(labels.shape[1], hw[0])][:, :, nearest_index(labels.shape[2], hw[1])]


def evaluate_restated(sd, store, key, hw, ncls=4):
    conf = np.zeros((ncls, ncls), dtype=np.int64)
    with torch.no_grad():
        for g in store[key].values():
            logits = net_forward(sd, host_input(g['images_ss'], hw)).numpy()
            truth = np.asarray(g['labels_ss'])
            conf += confusion(argmax_resized(logits, truth.shape[1], truth.shape[2], ncls)[0], truth, ncls)
    return scores(conf)


def train_restated(sd0, store, hw, niter, batch, lr, seed, ncls=4):
    """seg2eye_amd.segment.train_segmenter (no flip, uniform weights) from the rule alone, in the dtype of sd0: the same shuffled order,
    torch.optim.Adam(betas=(0.9, 0.999)).  -> (state dict, [loss per step])."""
    sd = {k: v.clone().requires_grad_(True) for k, v in sd0.items()}
    opt = torch.optim.Adam(list(sd.values()), lr=lr, betas=(0.9, 0.999), eps=1e-8)
    samples = [(u, i) for u, g in store['train'].items() for i in range(len(g['labels_ss']))]
    rng = np.random.RandomState(seed)
    losses = []
    for _ in range(niter):
        order = rng.permutation(len(samples))
        for b0 in range(0, len(order), batch):
            rows = [samples[j] for j in order[b0:b0 + batch]]
            x = host_input(np.stack([store['train'][u]['images_ss'][i] for u, i in rows]), hw)
            y = torch.from_numpy(host_labels(np.stack([store['train'][u]['labels_ss'][i] for u, i in rows]), hw))
            opt.zero_grad()
            loss = ce_torch(net_forward(sd, x), y)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
    return {k: v.detach() for k, v in sd.items()}, losses


# ------------------------------------------------------------------------------------------------ data
def eyes(n, H, W, ncls, seed):
    """Nested ellipses at jittered positions: class c sits inside class c - 1, the background is 0."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((n, H, W), dtype=np.uint8)
    for i in range(n):
        cy, cx = H * (0.5 + 0.15 * rng.uniform(-1, 1)), W * (0.5 + 0.15 * rng.uniform(-1, 1))
        ry, rx = max(0.5, H * (0.32 + 0.1 * rng.uniform(-1, 1))), max(0.5, W * (0.4 + 0.1 * rng.uniform(-1, 1)))
        for c in range(1, ncls):
            s = 1.0 - (c - 1) / float(ncls)
            out[i][((yy - cy) / (ry * s)) ** 2 + ((xx - cx) / (rx * s)) ** 2 <= 1.0] = c
    return out


GREY = np.array([40, 200, 110, 10], dtype=np.float64)          # background skin, sclera, iris, pupil


def eye_frames(labels, name, seed):
    """A learnable image of every label map: a grey level per class plus hash noise of +-24 levels."""
    from seg2eye_amd.synthetic import hash_uniform
    noise = hash_uniform(name, labels.shape, seed, -24.0, 24.0).astype(np.float64)
    return np.clip(GREY[labels] + noise, 0, 255).astype(np.uint8)


def learnable_store(H=640, W=400, seed=3):
    """3 persons in 'train', 2 in 'validation'; 6 labelled and 4 + 4 unlabelled frames each (their true labels are kept aside, under
    the second result), labels from synthetic.ellipse_labels, file names as prepare_openeds writes them."""
    from seg2eye_amd.synthetic import ellipse_labels
    store, truth = {}, {}
    for ki, (key, users) in enumerate((('train', ('U101', 'U102', 'U103')), ('validation', ('U201', 'U202')))):
        store[key], truth[key] = {}, {}
        for ui, u in enumerate(users):
            s = seed * 100 + ki * 10 + ui
            lab = ellipse_labels(14, H, W, seed=s)[:, 0]
            img = eye_frames(lab, '%s/%s' % (key, u), s)
            store[key][u] = {'images_ss': img[:6], 'labels_ss': lab[:6], 'images_gen': img[6:10], 'images_seq': img[10:14],
                             'images_ss_filenames': np.array([('%s.%03d_ss' % (u, i)).encode() for i in range(6)], dtype='S13'),
                             'images_gen_filenames': np.array([('%s_g%03d' % (u, i)).encode() for i in range(4)], dtype='S13')}
            truth[key][u] = {'labels_pred_gen': lab[6:10], 'labels_pred_seq': lab[10:14]}
    return store, truth
