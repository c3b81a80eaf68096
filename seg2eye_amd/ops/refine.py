"""The residual refiner's input, loss and submission bytes: the NHWC network input made of three uint8 planes
(`refine_input`), the loss on the challenge's error of  clamp(reference frame + residual, -1, 1)  against the uint8 truth with its
gradient (`refine_loss`, an autograd Function) and the uint8 prediction (`refine_predict_u8`).  Frames and masks stay uint8 (N, H, W) as
the store holds them; a per-image flip byte mirrors every plane of that image alike."""
import torch

from .. import _lib as L
from .core import LaunchProfiler, _dt, _need, _p, _stream

MAX_CLASSES = 16
CLASS_LEVELS = (125, 103, 76, 34)       # the reference's class means as its uint8 array stores them (refinenet/dataset.py:60-70)


def _planes(named, flip):
    """The checks of the uint8 planes and the flip bytes that need no device.  -> (N, H, W)"""
    shape = None
    for name, t in named:
        if t.dtype != torch.uint8:
            raise ValueError('%s: uint8 expected, got %s' % (name, t.dtype))
        if t.dim() != 3 or min(t.shape) < 1:
            raise ValueError('%s: (N, H, W) expected, got %s' % (name, tuple(t.shape)))
        if shape is not None and tuple(t.shape) != shape:
            raise ValueError('%s: %s as %s expected, got %s' % (name, shape, named[0][0], tuple(t.shape)))
        shape = tuple(t.shape)
    if flip is not None:
        if flip.dtype not in (torch.uint8, torch.bool):
            raise ValueError('flip: uint8 or bool expected, got %s' % flip.dtype)
        if flip.dim() != 1 or flip.numel() != shape[0]:
            raise ValueError('flip: one byte per image (%d,) expected, got %s' % (shape[0], tuple(flip.shape)))
    return shape


def _flip_bytes(flip):
    return flip.view(torch.uint8) if flip is not None and flip.dtype == torch.bool else flip


def _residual(res, shape):
    if res.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError('bf16 or fp32 residual expected, got %s' % res.dtype)
    if res.dim() != 4 or res.shape[3] < 1 or tuple(res.shape[:3]) != shape:
        raise ValueError('res: %s + (C >= 1,) expected, got %s' % (shape, tuple(res.shape)))


def refine_input(tmask, rimg, rmask, flip=None, levels=None, ncls=4, channels=8, dtype=torch.bfloat16):
    """tmask (the target's mask), rimg (the reference frame), rmask (its mask): uint8 (N, H, W) -> x (N, H, W, channels) NHWC of `dtype`
    in [-1, 1]: [the target mask in grey levels, the frame, its mask in grey levels, 0 ...].  levels: ncls grey levels, one per class
    (default: the reference's 125, 103, 76, 34, cut or padded with 0 to ncls); a label >= ncls takes level 0."""
    ncls, channels = int(ncls), int(channels)
    n, h, w = _planes((('tmask', tmask), ('rimg', rimg), ('rmask', rmask)), flip)
    if dtype not in (torch.bfloat16, torch.float32):
        raise ValueError('bf16 or fp32 expected, got %s' % (dtype,))
    if not 1 <= ncls <= MAX_CLASSES:
        raise ValueError('ncls = %d (1 to %d classes)' % (ncls, MAX_CLASSES))
    if channels < 3:
        raise ValueError('channels = %d (at least 3)' % channels)
    if levels is None:
        levels = (CLASS_LEVELS + (0,) * MAX_CLASSES)[:ncls]
    if not torch.is_tensor(levels):
        lv = [int(v) for v in levels]
        if len(lv) != ncls or min(lv) < 0 or max(lv) > 255:
            raise ValueError('levels: %d grey levels 0..255 expected, got %s' % (ncls, lv))
        levels = torch.tensor(lv, dtype=torch.uint8, device=tmask.device)
    elif levels.dtype != torch.uint8 or tuple(levels.shape) != (ncls,):
        raise ValueError('levels: uint8 (%d,) expected, got %s %s' % (ncls, levels.dtype, tuple(levels.shape)))
    flip = _flip_bytes(flip)
    _need(tmask, rimg, rmask, flip, levels)
    x = torch.empty(n, h, w, channels, dtype=dtype, device=tmask.device)
    LaunchProfiler.run('refine', 0.0, L.call.s2e_refine_input,
                       (_dt(dtype), _p(tmask), _p(rimg), _p(rmask), _p(flip), _p(levels), ncls, n, h, w, channels, _p(x), _stream()),
                       nbytes=float(n * h * w * (3 + channels * x.element_size())))      # three planes read, x written
    return x


class RefineLossFn(torch.autograd.Function):
    """lambda_eds eds_loss + lambda_l1 l1 of clamp(frame + res, -1, 1) against the truth (include/seg2eye_hip.h); the gradient goes to res."""

    @staticmethod
    def forward(ctx, res, rimg, truth, flip, lambda_eds, lambda_l1):
        r = res.detach()
        _need(r, rimg, truth, flip)
        n, h, w, c = r.shape
        dev = r.device
        ws = torch.empty(int(L.call.s2e_refine_head_workspace_bytes(n, h, w)) // 8, dtype=torch.float64, device=dev)
        score = torch.empty(n, dtype=torch.float32, device=dev)
        sumsq = torch.empty(n, dtype=torch.float64, device=dev)          # kept for the backward
        terms = torch.empty(3, dtype=torch.float32, device=dev)
        LaunchProfiler.run('refine', 0.0, L.call.s2e_refine_head_fwd,
                           (_dt(r), _p(r), c, _p(rimg), _p(truth), _p(flip), n, h, w, _p(score), _p(sumsq), _p(terms), _p(ws), ws.numel() * 8,
                            _stream()),
                           nbytes=float(n * h * w * (c * r.element_size() + 2)))         # the residual's lines and two planes, once
        loss = lambda_eds * terms[0] if lambda_l1 == 0.0 else lambda_l1 * terms[1] if lambda_eds == 0.0 else lambda_eds * terms[0] + lambda_l1 * terms[1]
        ctx.lambdas = (lambda_eds, lambda_l1)
        ctx.save_for_backward(r, rimg, truth, flip, sumsq)
        ctx.mark_non_differentiable(terms, score)
        return loss, terms, score

    @staticmethod
    def backward(ctx, gloss, _gterms, _gscore):
        r, rimg, truth, flip, sumsq = ctx.saved_tensors
        lambda_eds, lambda_l1 = ctx.lambdas
        n, h, w, c = r.shape
        g = gloss.detach().float().contiguous()
        dres = torch.empty_like(r)
        LaunchProfiler.run('refine', 0.0, L.call.s2e_refine_head_bwd,
                           (_dt(r), _p(r), c, _p(rimg), _p(truth), _p(flip), n, h, w, _p(sumsq), _p(g), lambda_eds, lambda_l1, _p(dres), _stream()),
                           nbytes=float(n * h * w * (2 * c * r.element_size() + 2)))     # residual read, gradient written, two planes
        return dres, None, None, None, None, None


def refine_loss(res, rimg, truth, flip=None, lambda_eds=1.0, lambda_l1=0.0):
    """res (N, H, W, C) bf16 / fp32, channel 0 the residual; rimg, truth uint8 (N, H, W) -> (loss, terms, score): with
    p = clamp(res + frame, -1, 1) and d = p - truth in [-1, 1] units, the 0-dim fp32
        lambda_eds mean_n(127.5 sqrt(sum d^2) / (H W)) + lambda_l1 mean |d|,
    the detached fp32 (3,) terms [eds_loss, l1, 1471 eds_loss] and the detached fp32 (N,) per-image score.  An image whose prediction
    equals its truth gets a zero eds gradient (torch: NaN)."""
    lambda_eds, lambda_l1 = float(lambda_eds), float(lambda_l1)
    shape = _planes((('rimg', rimg), ('truth', truth)), flip)
    _residual(res, shape)
    for name, v in (('lambda_eds', lambda_eds), ('lambda_l1', lambda_l1)):
        if not (0.0 <= v < float('inf')):
            raise ValueError('%s = %r (finite and not negative)' % (name, v))
    return RefineLossFn.apply(res, rimg, truth, _flip_bytes(flip), lambda_eds, lambda_l1)


def refine_predict_u8(res, rimg, flip=None):
    """-> uint8 (N, H, W): (uint8)(127.5 (clamp(res + frame, -1, 1) + 1)), truncated as the reference's submission is; with a zero
    residual that is the frame to within one grey level (47 of the 256 levels come back one lower)."""
    shape = _planes((('rimg', rimg),), flip)
    _residual(res, shape)
    flip = _flip_bytes(flip)
    r = res.detach()
    _need(r, rimg, flip)
    n, h, w, c = r.shape
    out = torch.empty(n, h, w, dtype=torch.uint8, device=r.device)
    LaunchProfiler.run('refine', 0.0, L.call.s2e_refine_predict_u8, (_dt(r), _p(r), c, _p(rimg), _p(flip), n, h, w, _p(out), _stream()),
                       nbytes=float(n * h * w * (c * r.element_size() + 2)))
    return out
