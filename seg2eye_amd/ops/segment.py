"""The eye segmenter's loss, mask and metric: the weighted softmax cross-entropy of NHWC logits against a uint8 label map
(`seg_cross_entropy`, an autograd Function), the uint8 mask of bilinearly resized logits (`seg_argmax_u8`), the confusion matrix of two
masks accumulated on the device (`seg_confusion`) and, on the host, the scores read from it (`segment_scores`); and its boundary-aware
terms: the signed distance maps and boundary band of a label map (`seg_dist_maps`) and the fused boundary-weighted
cross-entropy + generalised Dice + surface loss (`seg_loss`, an autograd Function)."""
import numpy as np
import torch

from .. import _lib as L
from .core import LaunchProfiler, _dt, _need, _p, _stream

MAX_CLASSES = 16


def _logits(logits, ncls=None):
    """The checks of an NHWC logits tensor that need no device: they come first, as in _image_pair."""
    if logits.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError('bf16 or fp32 logits expected, got %s' % logits.dtype)
    if logits.dim() != 4 or min(logits.shape) < 1:
        raise ValueError('logits: (N, H, W, C) expected, got %s' % (tuple(logits.shape),))
    ncls = logits.shape[3] if ncls is None else int(ncls)
    if not 1 <= ncls <= min(MAX_CLASSES, logits.shape[3]):
        raise ValueError('%d classes in logits of %d channels (1 to %d classes, at most the channels)' % (ncls, logits.shape[3], MAX_CLASSES))
    return ncls


def _ce_args(logits, label, weights):
    ncls = _logits(logits, None if weights is None else weights.numel())
    if label.dtype != torch.uint8:
        raise ValueError('uint8 label map expected, got %s' % label.dtype)
    if weights is not None and (weights.dtype != torch.float32 or weights.dim() != 1):
        raise ValueError('class weights: fp32 (ncls,) expected, got %s %s' % (weights.dtype, tuple(weights.shape)))
    if tuple(label.shape) != tuple(logits.shape[:3]):
        raise ValueError('logits (N, H, W, C) and label (N, H, W) of one N x H x W expected, got %s and %s' % (tuple(logits.shape), tuple(label.shape)))
    return ncls


class SegCrossEntropyFn(torch.autograd.Function):
    """F.cross_entropy(weight=w, ignore_index=every label >= ncls, reduction='mean') of NHWC logits; the gradient goes to the logits."""

    @staticmethod
    def forward(ctx, logits, label, weights, ncls):
        x = logits.detach()
        _need(x, label, weights)
        n, h, w, c = x.shape
        ws = torch.empty(int(L.call.s2e_seg_ce_workspace_bytes(n, h, w)) // 8, dtype=torch.float64, device=x.device)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        denom = torch.empty(1, dtype=torch.float32, device=x.device)    # the sum of the counted pixels' weights, kept for the backward
        LaunchProfiler.run('segment', 0.0, L.call.s2e_seg_ce_fwd,
                           (_dt(x), _p(x), _p(label), _p(weights), n, h, w, c, ncls, _p(loss), _p(denom), _p(ws), ws.numel() * 8, _stream()),
                           nbytes=float(n * h * w * (c * x.element_size() + 1)))     # the logits and the labels, once
        ctx.ncls = ncls
        ctx.save_for_backward(x, label, weights, denom)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        x, label, weights, denom = ctx.saved_tensors
        n, h, w, c = x.shape
        g = gloss.detach().float().contiguous()
        dx = torch.empty_like(x)
        LaunchProfiler.run('segment', 0.0, L.call.s2e_seg_ce_bwd,
                           (_dt(x), _p(x), _p(label), _p(weights), _p(denom), _p(g), n, h, w, c, ctx.ncls, _p(dx), _stream()),
                           nbytes=float(n * h * w * (2 * c * x.element_size() + 1)))  # logits read, gradient written, labels read
        return dx, None, None, None


def seg_cross_entropy(logits, label, weights=None):
    """logits (N, H, W, C) bf16 / fp32, label (N, H, W) uint8, weights None (all 1, C classes) or fp32 (ncls,), ncls <= C -> the 0-dim
    fp32 mean loss over the pixels whose label is < ncls (255 and every other value >= ncls is ignored)."""
    ncls = _ce_args(logits, label, weights)
    if weights is None:
        weights = torch.ones(ncls, dtype=torch.float32, device=logits.device)
    return SegCrossEntropyFn.apply(logits, label, weights, ncls)


MAX_DIST_SIDE = 1024


def seg_dist_maps(label, ncls, radius=2):
    """label (N, H, W) uint8, H, W <= 1024 -> (phi fp32 (N, H, W, ncls), band uint8 (N, H, W)), per image: phi[..., c] = 1 - the
    distance to the nearest pixel outside class c where the label is c, + the distance to the nearest pixel of class c elsewhere, 0 for
    a class that is absent or fills the image; band = 1 where a counted pixel lies within `radius` of a pixel of another class."""
    ncls, radius = int(ncls), int(radius)
    if label.dtype != torch.uint8:
        raise ValueError('uint8 label map expected, got %s' % label.dtype)
    if label.dim() != 3 or min(label.shape) < 1 or max(label.shape[1:]) > MAX_DIST_SIDE:
        raise ValueError('label: (N, H, W) with H, W <= %d expected, got %s' % (MAX_DIST_SIDE, tuple(label.shape)))
    if not 1 <= ncls <= MAX_CLASSES:
        raise ValueError('ncls = %d (1 to %d classes)' % (ncls, MAX_CLASSES))
    if radius < 0:
        raise ValueError('radius = %d (0 or more)' % radius)
    _need(label)
    n, h, w = label.shape
    phi = torch.empty(n, h, w, ncls, dtype=torch.float32, device=label.device)
    band = torch.empty(n, h, w, dtype=torch.uint8, device=label.device)
    ws = torch.empty(int(L.call.s2e_seg_dist_workspace_bytes(n, h, w, ncls)) // 4, dtype=torch.int32, device=label.device)
    LaunchProfiler.run('segment', 0.0, L.call.s2e_seg_dist_maps,
                       (_p(label), n, h, w, ncls, radius, _p(phi), _p(band), _p(ws), ws.numel() * 4, _stream()),
                       nbytes=float(n * h * w * (2 + 4 * ncls)))          # the labels read, phi and the band written, once
    return phi, band


def _loss_args(logits, label, weights, phi, band, lambdas):
    """_ce_args, then the maps in its order -- dtypes, then shapes -- and the scalars last.  -> ncls"""
    ncls = _ce_args(logits, label, weights)
    if phi is not None and phi.dtype != torch.float32:
        raise ValueError('phi: fp32 distance maps expected, got %s' % phi.dtype)
    if band is not None and band.dtype != torch.uint8:
        raise ValueError('band: uint8 expected, got %s' % band.dtype)
    if phi is not None and tuple(phi.shape) != tuple(label.shape) + (ncls,):
        raise ValueError('phi: %s expected, got %s' % (tuple(label.shape) + (ncls,), tuple(phi.shape)))
    if band is not None and tuple(band.shape) != tuple(label.shape):
        raise ValueError('band: %s expected, got %s' % (tuple(label.shape), tuple(band.shape)))
    for name, v in lambdas:
        if not (0.0 <= v < float('inf')):
            raise ValueError('%s = %r (finite and not negative)' % (name, v))
    lam = dict(lambdas)
    if lam['lambda_surface'] != 0.0 and phi is None:
        raise ValueError('lambda_surface = %g needs phi (seg_dist_maps)' % lam['lambda_surface'])
    if lam['edge_alpha'] != 0.0 and band is None:
        raise ValueError('edge_alpha = %g needs band (seg_dist_maps)' % lam['edge_alpha'])
    return ncls


class SegLossFn(torch.autograd.Function):
    """lambda_ce CE + lambda_dice Dice + lambda_surface Surface of NHWC logits (include/seg2eye_hip.h); the gradient goes to the logits."""

    @staticmethod
    def forward(ctx, logits, label, weights, phi, band, ncls, lambda_ce, lambda_dice, lambda_surface, edge_alpha):
        x = logits.detach()
        _need(x, label, weights, phi, band)
        n, h, w, c = x.shape
        ws = torch.empty(int(L.call.s2e_seg_loss_workspace_bytes(n, h, w, ncls)) // 8, dtype=torch.float64, device=x.device)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        terms = torch.empty(3, dtype=torch.float32, device=x.device)
        saved = torch.empty(n * 2 * ncls + 2, dtype=torch.float32, device=x.device)    # the Dice coefficients and the two denominators
        used = (4 * ncls if lambda_surface else 0) + (1 if edge_alpha else 0)          # bytes of phi and band a pixel reads
        LaunchProfiler.run('segment', 0.0, L.call.s2e_seg_loss_fwd,
                           (_dt(x), _p(x), _p(label), _p(weights), _p(phi), _p(band), n, h, w, c, ncls, lambda_ce, lambda_dice, lambda_surface,
                            edge_alpha, _p(loss), _p(terms), _p(saved), _p(ws), ws.numel() * 8, _stream()),
                           nbytes=float(n * h * w * (c * x.element_size() + 1 + used)))
        ctx.args = (ncls, lambda_ce, lambda_surface, edge_alpha, used)
        ctx.save_for_backward(x, label, weights, phi, band, saved)
        ctx.mark_non_differentiable(terms)
        return loss, terms

    @staticmethod
    def backward(ctx, gloss, _gterms):
        x, label, weights, phi, band, saved = ctx.saved_tensors
        ncls, lambda_ce, lambda_surface, edge_alpha, used = ctx.args
        n, h, w, c = x.shape
        g = gloss.detach().float().contiguous()
        dx = torch.empty_like(x)
        LaunchProfiler.run('segment', 0.0, L.call.s2e_seg_loss_bwd,
                           (_dt(x), _p(x), _p(label), _p(weights), _p(phi), _p(band), _p(saved), _p(g), n, h, w, c, ncls, lambda_ce, lambda_surface,
                            edge_alpha, _p(dx), _stream()),
                           nbytes=float(n * h * w * (2 * c * x.element_size() + 1 + used)))
        return (dx,) + (None,) * 9


def seg_loss(logits, label, weights=None, phi=None, band=None, lambda_ce=1., lambda_dice=0., lambda_surface=0., edge_alpha=0.):
    """logits (N, H, W, C) bf16 / fp32, label (N, H, W) uint8, weights None (all 1, C classes) or fp32 (ncls,), phi fp32 (N, H, W, ncls)
    and band uint8 (N, H, W) from seg_dist_maps -> (loss, terms): the 0-dim fp32
        lambda_ce CE + lambda_dice Dice + lambda_surface Surface
    over the pixels whose label is < ncls, and the detached fp32 (3,) terms [CE, Dice, Surface].  CE counts a pixel of the band
    1 + edge_alpha times; Dice is the generalised Dice (classes weighed by inverse squared area, per image); Surface is the mean of
    softmax x phi.  phi is needed when lambda_surface != 0, band when edge_alpha != 0; a term that is off ignores its input."""
    lambdas = [(k, float(v)) for k, v in (('lambda_ce', lambda_ce), ('lambda_dice', lambda_dice), ('lambda_surface', lambda_surface),
                                          ('edge_alpha', edge_alpha))]
    ncls = _loss_args(logits, label, weights, phi, band, lambdas)
    if weights is None:
        weights = torch.ones(ncls, dtype=torch.float32, device=logits.device)
    return SegLossFn.apply(logits, label, weights, phi, band, ncls, *(v for _, v in lambdas))


def seg_argmax_u8(logits, Ho=None, Wo=None, ncls=None):
    """logits (N, h, w, C) -> uint8 (N, Ho, Wo): the argmax of the first ncls (default C) channels resized bilinearly
    (align_corners=False) to Ho x Wo (default h x w: the plain argmax); ties go to the lowest class."""
    ncls = _logits(logits, ncls)
    n, h, w, c = logits.shape
    Ho, Wo = h if Ho is None else int(Ho), w if Wo is None else int(Wo)
    if Ho < 1 or Wo < 1:
        raise ValueError('output size %d x %d (at least 1 x 1)' % (Ho, Wo))
    x = logits.detach()
    _need(x)
    mask = torch.empty(n, Ho, Wo, dtype=torch.uint8, device=x.device)
    LaunchProfiler.run('segment', 0.0, L.call.s2e_seg_argmax_u8, (_dt(x), _p(x), n, h, w, c, ncls, Ho, Wo, _p(mask), _stream()),
                       nbytes=float(x.numel() * x.element_size() + mask.numel()))
    return mask


def seg_confusion(pred, truth, ncls, out=None):
    """pred, truth uint8 of one shape -> int64 (ncls, ncls), row = truth, column = pred: the counts of the pixel pairs ADDED into `out`
    (a new zero matrix when None), pairs with a value >= ncls skipped.  No synchronisation: a validation loop hands the matrix on."""
    ncls = int(ncls)
    if pred.dtype != torch.uint8 or truth.dtype != torch.uint8:
        raise ValueError('uint8 masks expected, got %s and %s' % (pred.dtype, truth.dtype))
    if not 1 <= ncls <= MAX_CLASSES:
        raise ValueError('ncls = %d (1 to %d classes)' % (ncls, MAX_CLASSES))
    if out is not None and (out.dtype != torch.int64 or tuple(out.shape) != (ncls, ncls)):
        raise ValueError('out: int64 (%d, %d) expected, got %s %s' % (ncls, ncls, out.dtype, tuple(out.shape)))
    if pred.shape != truth.shape or pred.numel() < 1:
        raise ValueError('pred and truth of one non-empty shape expected, got %s and %s' % (tuple(pred.shape), tuple(truth.shape)))
    _need(pred, truth, out)
    if out is None:
        out = torch.zeros(ncls, ncls, dtype=torch.int64, device=pred.device)
    LaunchProfiler.run('segment', 0.0, L.call.s2e_seg_confusion_u8, (_p(pred), _p(truth), pred.numel(), ncls, _p(out), _stream()),
                       nbytes=float(2 * pred.numel()))
    return out


def segment_scores(conf):
    """conf (ncls, ncls) counts, row = truth, column = pred (a tensor or an array) -> {'iou': float64 (ncls,), NaN for a class absent
    from truth and pred, 'miou': the mean over the classes whose union is not empty (0 when there is none), 'acc': pixel accuracy}."""
    c = np.asarray(conf.cpu() if torch.is_tensor(conf) else conf).astype(np.float64)
    if c.ndim != 2 or c.shape[0] != c.shape[1]:
        raise ValueError('a square confusion matrix expected, got %s' % (c.shape,))
    inter = np.diag(c)
    union = c.sum(axis=0) + c.sum(axis=1) - inter
    seen = union > 0
    iou = np.where(seen, inter / np.where(seen, union, 1.0), np.nan)
    total = c.sum()
    return {'iou': iou, 'miou': float(iou[seen].mean()) if seen.any() else 0.0, 'acc': float(inter.sum() / total) if total > 0 else 0.0}
