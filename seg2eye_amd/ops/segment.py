"""The eye segmenter's loss, mask and metric: the weighted softmax cross-entropy of NHWC logits against a uint8 label map
(`seg_cross_entropy`, an autograd Function), the uint8 mask of bilinearly resized logits (`seg_argmax_u8`), the confusion matrix of two
masks accumulated on the device (`seg_confusion`) and, on the host, the scores read from it (`segment_scores`)."""
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
