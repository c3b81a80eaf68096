"""Eye geometry: where the pupil and the iris are, as ellipses fitted to the masks, an optional link after mask_clean in
the chain prepare_openeds -> segment -> mask_clean -> (eye_geometry) -> style_rank -> train -> test (and -> refine).

A lid covers part of the pupil in most OpenEDS frames, so the area centroid of the pupil class is not the pupil's centre.  A curve here
is fitted to *rim pixels* only: the pixels of the inner classes that touch the outer class -- pupil against iris, iris or pupil against
sclera -- so the lid's cut contributes no point (include/seg2eye_hip.h states the rule).  The device sums the integer moments of the rim
pixels about their rounded mean (`ops.geometry.rim_moments`); the 3 x 3 algebra per mask is fp64 numpy here (`ellipse_from_moments`, the
direct least-squares fit of Halir and Flusser).  Repainting a mask from its ellipses (`ops.geometry.ellipse_paint`) smooths frayed class
borders and makes pupil inside iris inside sclera hold by construction.

    python -m seg2eye_amd.eye_geometry fit   --seg_file masks_clean.h5 --out geometry.h5
    python -m seg2eye_amd.eye_geometry apply --seg_file masks_clean.h5 --out masks_ellipse.h5
    python -m seg2eye_amd.eye_geometry eval  --dataroot openeds.h5 --name seg --dataset_key validation

`fit` writes per labels_pred_* array `<name>_ellipses`, float64 (n, K, 6): valid, cx, cy, a, b, theta.  `apply` writes the regularised
masks in the layout it read them in, a drop-in --seg_file.  `eval` scores a segmenter's masks of the labelled frames raw, cleaned and
regularised, and the fitted centres against those of the true labels.  All three are plain functions too: `fit_store`,
`regularise_store`, `evaluate`, on an `EyeShape`.  The ops are looked up when called."""
import argparse
import collections

import numpy as np
import torch

from . import stage
from .mask_clean import MaskRule
from .openeds_store import STORE_DEPTH, merge_splits, open_tree, rows_u8, save_tree

SINGULAR = 1e-12            # det S3 <= SINGULAR * S20 S02 S00: the rim pixels lie on a line (or are fewer than three)
# the index of sum u^i v^j in a row of rim (include/seg2eye_hip.h): 3 + m, by degree and then by j
_M = {(0, 0): 3, (1, 0): 4, (0, 1): 5, (2, 0): 6, (1, 1): 7, (0, 2): 8, (3, 0): 9, (2, 1): 10, (1, 2): 11, (0, 3): 12,
      (4, 0): 13, (3, 1): 14, (2, 2): 15, (1, 3): 16, (0, 4): 17}

EllipseFit = collections.namedtuple('EllipseFit', 'valid conic origin centre axes theta cause')
FITTED, FEW_POINTS, SINGULAR_S3, NO_ELLIPSE, NOT_FINITE, TOO_LARGE = range(6)       # EllipseFit.cause: the first test a fit fails


def _block(rim, ij):
    """(..., 18) double -> (..., 3, 3): the sums named by the 3 x 3 table of exponent pairs ij."""
    return np.stack([np.stack([rim[..., _M[e]] for e in row], axis=-1) for row in ij], axis=-2)


def ellipse_from_moments(rim, min_points=12, max_axis=None):
    """rim: int64 (..., 18) as `rim_moments` gives it (n, ox, oy, the 15 centred sums), taken as double -> EllipseFit of
        valid   uint8 (...)        1 where the fit below succeeded
        conic   float64 (..., 6)   (A, B, C, D, E, F) with A + C = 1 in the coordinates u = x - ox, v = y - oy: the inside is Q < 0
        origin  int32 (..., 2)     (ox, oy)
        centre  float64 (..., 2)   (cx, cy) in image coordinates
        axes    float64 (..., 2)   the semi-axes a >= b
        theta   float64 (...)      the major axis against +x with y down, in (-pi/2, pi/2]
        cause   uint8 (...)        0, or why valid is 0: 1 few points, 2 S3 singular, 3 no eigenvector, 4 not finite, 5 too large
    The direct least-squares fit of Halir and Flusser: with the scatter blocks S1 (of u^2, uv, v^2), S2 (those against u, v, 1) and
    S3 (of u, v, 1), T = -S3^-1 S2^T and M = C1^-1 (S1 + S2 T), C1 the constraint 4AC - B^2; of the eigenvectors np.linalg.eig returns
    (unit length) the real one of largest 4AC - B^2 > 0 is (A, B, C), and (D, E, F) = T (A, B, C).
    valid = 0, every parameter NaN (origin kept), where n < min_points; S3 is singular (det S3 <= 1e-12 S20 S02 S00); no eigenvector
    qualifies; anything is not finite (the conic is no real ellipse); or a > max_axis (EyeShape passes 2 max(H, W)).
    The rim pixels are the inner ones of a border, so the axes come out short by about 0.4 px; that bias is left in."""
    rim = np.asarray(rim)
    r = rim.astype(np.float64)
    lead = r.shape[:-1]
    n = r[..., 0]
    S1 = _block(r, (((4, 0), (3, 1), (2, 2)), ((3, 1), (2, 2), (1, 3)), ((2, 2), (1, 3), (0, 4))))
    S2 = _block(r, (((3, 0), (2, 1), (2, 0)), ((2, 1), (1, 2), (1, 1)), ((1, 2), (0, 3), (0, 2))))
    S3 = _block(r, (((2, 0), (1, 1), (1, 0)), ((1, 1), (0, 2), (0, 1)), ((1, 0), (0, 1), (0, 0))))
    with np.errstate(all='ignore'):
        cause = np.zeros(lead, dtype=np.uint8)

        def need(ok, passed, code):
            cause[ok & ~passed] = code
            return ok & passed
        ok = need(np.isfinite(r).all(axis=-1), n >= min_points, FEW_POINTS)
        det = np.linalg.det(np.where(ok[..., None, None], S3, np.eye(3)))
        ok = need(ok, det > SINGULAR * r[..., _M[2, 0]] * r[..., _M[0, 2]] * r[..., _M[0, 0]], SINGULAR_S3)
        S3i = np.linalg.inv(np.where(ok[..., None, None], S3, np.eye(3)))
        T = -np.matmul(S3i, np.swapaxes(S2, -1, -2))
        Mp = S1 + np.matmul(S2, T)
        M = np.stack([Mp[..., 2, :] / 2.0, -Mp[..., 1, :], Mp[..., 0, :] / 2.0], axis=-2)          # C1^-1 (S1 + S2 T)
        ok = need(ok, np.isfinite(M).all(axis=(-1, -2)), NOT_FINITE)
        _, vec = np.linalg.eig(np.where(ok[..., None, None], M, np.eye(3)))
        real = np.abs(np.imag(vec)).max(axis=-2) == 0                                              # per eigenvector (a column)
        vec = np.real(vec)
        cond = 4.0 * vec[..., 0, :] * vec[..., 2, :] - vec[..., 1, :] ** 2
        cond = np.where(real & np.isfinite(cond) & (cond > 0), cond, -np.inf)
        best = np.argmax(cond, axis=-1)
        ok = need(ok, np.take_along_axis(cond, best[..., None], axis=-1)[..., 0] > 0, NO_ELLIPSE)
        a1 = np.take_along_axis(vec, best[..., None, None], axis=-1)[..., 0]                       # (..., 3)
        a2 = np.matmul(T, a1[..., None])[..., 0]
        conic = np.concatenate([a1, a2], axis=-1)
        conic = conic / (conic[..., 0] + conic[..., 2])[..., None]
        A, B, C, D, E, F = (conic[..., i] for i in range(6))
        den = 4.0 * A * C - B * B
        u0, v0 = (B * E - 2.0 * C * D) / den, (B * D - 2.0 * A * E) / den
        F0 = F + (D * u0 + E * v0) / 2.0                                                           # Q at the centre: negative
        root = np.sqrt((A - C) ** 2 + B * B)
        major, minor = np.sqrt(-F0 / ((1.0 - root) / 2.0)), np.sqrt(-F0 / ((1.0 + root) / 2.0))
        theta = 0.5 * np.arctan2(0.0 - B, C - A)
        centre = np.stack([u0 + r[..., 1], v0 + r[..., 2]], axis=-1)
        axes = np.stack([major, minor], axis=-1)
        finite = np.isfinite(conic).all(axis=-1) & np.isfinite(centre).all(axis=-1) & np.isfinite(axes).all(axis=-1) & np.isfinite(theta)
        ok = need(ok, finite & (axes > 0).all(axis=-1), NOT_FINITE)
        if max_axis is not None:
            ok = need(ok, major <= max_axis, TOO_LARGE)
    cause[~np.isfinite(r).all(axis=-1)] = NOT_FINITE
    nan = lambda a: np.where(ok.reshape(lead + (1,) * (a.ndim - len(lead))), a, np.nan)
    origin = np.where(np.isfinite(r[..., 1:3]), rim[..., 1:3], 0).astype(np.int32)
    return EllipseFit(ok.astype(np.uint8), nan(conic), origin, nan(centre), nan(axes), nan(theta), cause)


def ellipse_table(fit):
    """EllipseFit -> float64 (..., 6): valid, cx, cy, a, b, theta -- what `fit` writes."""
    return np.concatenate([fit.valid[..., None].astype(np.float64), fit.centre, fit.axes, fit.theta[..., None]], axis=-1)


class EyeShape:
    """The curves of an eye and what a repaint does with them: ncls classes; curves, K pairs (in classes, out classes), None:
    ops.geometry.default_curves(ncls); paint, the class inside each curve, None: the first `in` class of each; keep, the classes a
    repaint leaves alone; base, the class of every other pixel outside all curves; min_points, the fewest rim pixels a fit takes;
    clean, the MaskRule applied first -- a speck is a false rim -- or None."""

    def __init__(self, ncls=4, curves=None, paint=None, keep=(0,), base=1, min_points=12, clean=None):
        self.ncls, self.base, self.min_points = int(ncls), int(base), int(min_points)
        self.curves = None if curves is None else tuple((tuple(a), tuple(b)) for a, b in curves)
        self.paint = None if paint is None else tuple(paint)
        self.keep = tuple(keep)
        self.clean = clean

    def _painted(self):
        from .ops import geometry as G
        if self.paint is not None:
            return self.paint
        return tuple(pair[0][0] for pair in (self.curves or G.default_curves(self.ncls)))

    def fit(self, masks, return_masks=False):
        """masks (n, H, W) uint8 on the device -> the EllipseFit of every mask and curve, numpy (n, K, ...); with return_masks also the
        masks the rim was taken from (cleaned when `clean` is set)."""
        from .ops import geometry as G
        if self.clean is not None:
            masks = self.clean.apply(masks)
        rim = G.rim_moments(masks, self.ncls, self.curves)
        fit = ellipse_from_moments(rim.cpu().numpy(), self.min_points, 2.0 * max(masks.shape[1:]))
        return (fit, masks) if return_masks else fit

    def regularise(self, masks, return_fit=False):
        """masks (n, H, W) uint8 on the device -> the masks repainted from their fitted ellipses (a mask without a valid fit of every
        curve comes back as cleaned); with return_fit also the EllipseFit."""
        from .ops import geometry as G
        fit, masks = self.fit(masks, return_masks=True)
        dev = masks.device
        out = G.ellipse_paint(masks, torch.from_numpy(np.ascontiguousarray(fit.conic)).to(dev), torch.from_numpy(np.ascontiguousarray(fit.origin)).to(dev),
                              torch.from_numpy(np.ascontiguousarray(fit.valid)).to(dev), self.ncls, self._painted(), self.keep, self.base)
        return (out, fit) if return_fit else out

    def __repr__(self):
        return 'EyeShape(ncls=%d, curves=%s, paint=%s, keep=%s, base=%d, min_points=%d, clean=%r)' % (
            self.ncls, self.curves, self.paint, self.keep, self.base, self.min_points, self.clean)


def _is_masks(name):
    return name.startswith('labels_pred_')


def _batches(dataset, batch, device):
    """The rows of a mask array (numpy or HDF5) as device tensors of at most `batch` masks."""
    n = dataset.shape[0]
    for r0 in range(0, n, int(batch)):
        rows = rows_u8((dataset, r) for r in range(r0, min(r0 + int(batch), n)))
        yield r0, stage.to_device(device, rows)[0]


# ------------------------------------------------------------------------------------------------ fit
def fit_store(seg_tree, shape, device='cuda', batch=64, verbose=True):
    """seg_tree {split: {user: {labels_pred_*: uint8 (n, H, W)}}} -> {split: {user: {<name>_ellipses: float64 (n, K, 6)}}}: valid, cx,
    cy, a, b, theta per mask and curve.  One line per split: masks, the fit rate per curve, the mean semi-axes per curve."""
    out = {}
    for split in seg_tree.keys():
        out[split] = {}
        tables = []
        for user in seg_tree[split].keys():
            g = seg_tree[split][user]
            out[split][user] = {}
            for name in g.keys():
                if not _is_masks(name):
                    continue
                parts = [ellipse_table(shape.fit(rows)) for _, rows in _batches(g[name], batch, device)]
                if parts:
                    table = np.concatenate(parts)
                    tables.append(table)
                    out[split][user][name + '_ellipses'] = table
        if verbose:
            print(_fit_line(split, np.concatenate(tables) if tables else np.zeros((0, 0, 6))))
    return out


def _fit_line(split, table):
    words = ['%s: %d masks' % (split, table.shape[0])]
    for k in range(table.shape[1] if table.shape[0] else 0):
        good = table[:, k, 0] > 0
        words.append('curve %d fit rate %.4f' % (k, good.mean()))
        if good.any():
            words.append('mean axes %.2f %.2f' % (table[good, k, 3].mean(), table[good, k, 4].mean()))
    return ', '.join(words)


# ------------------------------------------------------------------------------------------------ apply
def regularise_store(seg_tree, shape, device='cuda', batch=64, verbose=True):
    """seg_tree as above -> the same tree with every labels_pred_* array repainted from its ellipses by `shape`; any other array of a
    person is passed through.  One line per split: masks, the share of pixels changed, the share of masks left without a valid fit."""
    out = {}
    for split in seg_tree.keys():
        out[split] = {}
        masks = pixels = changed = unfit = 0
        for user in seg_tree[split].keys():
            g = seg_tree[split][user]
            out[split][user] = {}
            for name in g.keys():
                if not _is_masks(name):
                    out[split][user][name] = np.asarray(g[name])
                    continue
                painted = np.zeros(tuple(g[name].shape), dtype=np.uint8)
                for r0, rows in _batches(g[name], batch, device):
                    res, fit = shape.regularise(rows, return_fit=True)
                    painted[r0:r0 + len(rows)] = res.cpu().numpy()
                    changed += int((res != rows).sum())
                    unfit += int((fit.valid.min(axis=1) == 0).sum())
                    masks += len(rows)
                    pixels += rows.numel()
                out[split][user][name] = painted
        if verbose:
            print('%s: %d persons, %d masks, %.4f%% of the pixels changed, %.4f%% of the masks unchanged for want of a valid fit'
                  % (split, len(out[split]), masks, 100.0 * changed / max(pixels, 1), 100.0 * unfit / max(masks, 1)))
    return out


# ------------------------------------------------------------------------------------------------ eval
def evaluate(net, store, dataset_key, opt, shape, device='cuda', verbose=True):
    """mIoU, per-class IoU and pixel accuracy of `net` on the labelled frames of a split for its masks as they are, as shape.clean
    cleans them and as `shape` repaints them -> {'miou<s>/<key>', 'iou<s>/<key>/<c>', 'acc<s>/<key>'} for s in '', '_clean', '_ellipse',
    'centre_px/<key>/<curve>', the mean distance between the centre fitted on the predicted mask and on the true labels over the frames
    where both fits are valid (NaN where there is none), and 'fit_rate/<key>/<curve>' of the predicted masks."""
    from . import segment
    from .ops import segment as S
    ncls = int(opt.label_nc)
    conf = [torch.zeros(ncls, ncls, dtype=torch.int64, device=device) for _ in range(3)]
    samples = segment.labelled_samples(store, dataset_key)
    if not samples:
        raise ValueError("evaluate('%s'): the split has no labelled frames (images_ss / labels_ss)" % dataset_key)
    dist, both, fitted = [], [], []
    with torch.no_grad():
        for b0 in range(0, len(samples), int(opt.batchSize)):
            batch = samples[b0:b0 + int(opt.batchSize)]
            truth = segment._labelled_rows(store, dataset_key, 'labels_ss', batch)
            frames = segment._labelled_rows(store, dataset_key, 'images_ss', batch)
            logits = net(segment._frames_to_input(frames, opt.seg_hw, segment._no_flip(len(batch), device), device))
            pred = S.seg_argmax_u8(logits, truth.shape[1], truth.shape[2])
            t = torch.from_numpy(truth).to(device)
            painted, fit = shape.regularise(pred, return_fit=True)
            S.seg_confusion(pred, t, ncls, out=conf[0])
            S.seg_confusion(pred if shape.clean is None else shape.clean.apply(pred), t, ncls, out=conf[1])
            S.seg_confusion(painted, t, ncls, out=conf[2])
            true_fit = shape.fit(t)
            ok = (fit.valid > 0) & (true_fit.valid > 0)
            d = np.sqrt(((np.where(ok[..., None], fit.centre, 0.0) - np.where(ok[..., None], true_fit.centre, 0.0)) ** 2).sum(axis=-1))
            dist.append(d)
            both.append(ok)
            fitted.append(fit.valid > 0)
    out = {}
    for tag, c in zip(('', '_clean', '_ellipse'), conf):
        scores = S.segment_scores(c)
        out['miou%s/%s' % (tag, dataset_key)] = scores['miou']
        out['acc%s/%s' % (tag, dataset_key)] = scores['acc']
        out.update({'iou%s/%s/%d' % (tag, dataset_key, k): float(v) for k, v in enumerate(scores['iou'])})
    dist, both, fitted = np.concatenate(dist), np.concatenate(both), np.concatenate(fitted)
    for k in range(dist.shape[1]):
        out['centre_px/%s/%d' % (dataset_key, k)] = float(dist[both[:, k], k].mean()) if both[:, k].any() else float('nan')
        out['fit_rate/%s/%d' % (dataset_key, k)] = float(fitted[:, k].mean())
    if verbose:
        print(' '.join('%s %.4f' % (k, v) for k, v in out.items()))
    return out


# ------------------------------------------------------------------------------------------------ the command line
def _csv_int(s):
    return tuple(int(v) for v in s.split(','))


def shape_of(a):
    """The EyeShape of parsed arguments (a mapping with label_nc, min_points, no_clean)."""
    return EyeShape(a['label_nc'], min_points=a['min_points'], clean=None if a['no_clean'] else MaskRule(a['label_nc']))


def parser():
    ap = argparse.ArgumentParser(prog='python -m seg2eye_amd.eye_geometry',
                                 description='Pupil and iris ellipses of predicted eye masks: fit them, repaint the masks from them, score both.')
    common = argparse.ArgumentParser(add_help=False)
    common.add_argument('--no_clean', action='store_true', help='do not run the mask cleaner first (a speck is a false rim)')
    common.add_argument('--min_points', type=int, default=12, help='the fewest rim pixels a fit takes')
    common.add_argument('--label_nc', type=int, default=4)
    sub = ap.add_subparsers(dest='command', required=True)
    f = sub.add_parser('fit', parents=[common], help='write the ellipses of every labels_pred_* array of a mask file')
    f.add_argument('--seg_file', required=True, help='the file(s) `segment predict --out` or `mask_clean apply --out` wrote, comma-separated')
    f.add_argument('--out', required=True, help='<name>_ellipses per person: valid, cx, cy, a, b, theta (HDF5; <out>.npz without h5py)')
    f.add_argument('--batchSize', type=int, default=64)
    a = sub.add_parser('apply', parents=[common], help='repaint every labels_pred_* array of a mask file from its fitted ellipses')
    a.add_argument('--seg_file', required=True, help='the file(s) `segment predict --out` or `mask_clean apply --out` wrote, comma-separated')
    a.add_argument('--out', required=True, help='the regularised masks, a drop-in --seg_file (HDF5; <out>.npz without h5py)')
    a.add_argument('--batchSize', type=int, default=64)
    e = sub.add_parser('eval', parents=[common], help='mIoU of a segmenter checkpoint on the labelled frames, raw, cleaned and regularised; centre errors')
    e.add_argument('--dataroot', required=True, help='the store prepare_openeds wrote (.h5, or .npz without h5py)')
    e.add_argument('--name', default='segmenter', help='the checkpoints live in <checkpoints_dir>/<name>')
    e.add_argument('--checkpoints_dir', default='./checkpoints')
    e.add_argument('--nsf', type=int, default=32, help='# of filters of the first conv layer (a multiple of 8)')
    e.add_argument('--seg_hw', type=_csv_int, default=(320, 200), help='H,W the frames are resized to (multiples of 8)')
    e.add_argument('--compute_dtype', default='bf16', choices=['bf16', 'fp32'])
    e.add_argument('--batchSize', type=int, default=16)
    e.add_argument('--dataset_key', default='validation', choices=['train', 'validation', 'test'])
    e.add_argument('--which_epoch', default='latest')
    return ap


def main(argv=None):
    a = vars(parser().parse_args(argv))
    shape = shape_of(a)
    if a['command'] == 'fit':
        fitted = fit_store(merge_splits(a['seg_file'], open_tree), shape, batch=a['batchSize'])
        print('ellipses of %d split(s) written to %s' % (len(fitted), save_tree(fitted, a['out'], STORE_DEPTH)))
        return None
    if a['command'] == 'apply':
        from .prepare_openeds import save_store
        painted = regularise_store(merge_splits(a['seg_file'], open_tree), shape, batch=a['batchSize'])
        print('regularised masks of %d split(s) written to %s' % (len(painted), save_store(painted, a['out'])))
        return None
    from . import segment
    opt = segment.seg_options(**{k: a[k] for k in ('name', 'checkpoints_dir', 'nsf', 'seg_hw', 'label_nc', 'compute_dtype', 'batchSize')})
    net = stage.load_network(segment.build_network, 'S', opt, a['which_epoch'], 'cuda')
    return evaluate(net, open_tree(a['dataroot']), a['dataset_key'], opt, shape)


if __name__ == '__main__':
    main()
