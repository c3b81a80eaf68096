"""Loss reductions (hinge / L1 / feature matching with in-place gradient injection), the flat Adam step, and the OpenEDS validation
metric, SSIM, MS-SSIM, focal-frequency and region-error kernels."""
import torch

from .. import _lib as L
from .._lib import LOSS_L1, LOSS_L1_NANGRAD
from .core import LaunchProfiler, ZeroPool, _dt, _need, _p, _single_channel, _stream
from .conv import _live_tail_buffer


# ------------------------------------------------------------------------------ losses

def _loss_slot(device, pooled):
    """A zeroed fp32 scalar for s2e_loss_reduce to accumulate into.  Pool memory is recycled by the trainer's next step: only
    for terms that are consumed inside the step (see loss_sum)."""
    if pooled and ZeroPool.active() is not None:
        return ZeroPool.take(1, torch.float32, device).view(())
    return torch.zeros((), dtype=torch.float32, device=device)


class LossSumFn(torch.autograd.Function):
    """scale * sum_i f(a_i, b_i) as a 0-dim fp32 tensor (see s2e_loss_reduce for f)."""

    @staticmethod
    def forward(ctx, a, b, mode, scale, pooled=False):
        _need(a, b)
        out = _loss_slot(a.device, pooled)
        L.call.s2e_loss_reduce(_dt(a), mode, _p(a), _p(b), a.numel(), float(scale), _p(out), _stream())
        ctx.cfg = (mode, float(scale))
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    def backward(ctx, gout):
        a, b = ctx.saved_tensors
        mode, scale = ctx.cfg
        gs = gout.detach().float().contiguous()
        da = torch.empty_like(a)
        L.call.s2e_loss_grad(_dt(a), mode, _p(a), _p(b), a.numel(), scale, _p(gs), _p(da), 0, _stream())
        return da, None, None, None, None


class HalfLossFn(torch.autograd.Function):
    """scale * sum_i f(t_i) over ONE half of a [fake | real] batch t (2N, ...), NHWC-contiguous; the other half gets no gradient.
    == loss_sum(t[:N] or t[N:], ...) without the slice: the backward writes the element-wise gradient into the head of a
    zero-tailed buffer (first half, inside a trainer step: _live_tail_buffer -- one launch, and the LivePrefix gate behind it
    recognises the buffer) instead of slice_backward's zero-fill + copy."""

    @staticmethod
    def forward(ctx, t, second, mode, scale, pooled):
        _need(t)
        n = t.shape[0] // 2
        half = t[n:] if second else t[:n]
        out = _loss_slot(t.device, pooled)
        L.call.s2e_loss_reduce(_dt(t), mode, _p(half), None, half.numel(), float(scale), _p(out), _stream())
        ctx.cfg = (bool(second), mode, float(scale), n)
        ctx.save_for_backward(t)
        return out

    @staticmethod
    def backward(ctx, gout):
        t, = ctx.saved_tensors
        second, mode, scale, n = ctx.cfg
        gs = gout.detach().float().contiguous()
        if second:
            gt = torch.empty_like(t)
            gt[:n].zero_()
            dst, src = gt[n:], t[n:]
        else:
            gt = _live_tail_buffer(t, n)
            dst, src = gt[:n], t[:n]
        L.call.s2e_loss_grad(_dt(t), mode, _p(src), None, src.numel(), scale, _p(gs), _p(dst), 0, _stream())
        return gt, None, None, None, None


class PairLossFn(torch.autograd.Function):
    """(scale * sum f_a(t[:N]), scale * sum f_b(t[N:])) for a [fake | real] batch t: the discriminator's two hinge terms from
    the undivided prediction; the backward fills ONE gradient tensor with two launches (no slice_backward, no add)."""

    @staticmethod
    def forward(ctx, t, mode_a, mode_b, scale, pooled):
        _need(t)
        n = t.shape[0] // 2
        outs = []
        for half, mode in ((t[:n], mode_a), (t[n:], mode_b)):
            out = _loss_slot(t.device, pooled)
            L.call.s2e_loss_reduce(_dt(t), mode, _p(half), None, half.numel(), float(scale), _p(out), _stream())
            outs.append(out)
        ctx.cfg = (mode_a, mode_b, float(scale), n)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(t)
        return tuple(outs)

    @staticmethod
    def backward(ctx, ga, gb):
        t, = ctx.saved_tensors
        mode_a, mode_b, scale, n = ctx.cfg
        if ga is None and gb is None:
            return None, None, None, None, None
        gt = torch.empty_like(t)
        for dst, src, mode, g in ((gt[:n], t[:n], mode_a, ga), (gt[n:], t[n:], mode_b, gb)):
            if g is None:
                dst.zero_()
                continue
            gs = g.detach().float().contiguous()
            L.call.s2e_loss_grad(_dt(t), mode, _p(src), None, src.numel(), scale, _p(gs), _p(dst), 0, _stream())
        return gt, None, None, None, None


def half_loss(t, second, mode, scale, pooled=False):
    return HalfLossFn.apply(t, second, mode, scale, pooled)


def pair_loss(t, mode_a, mode_b, scale, pooled=False):
    return PairLossFn.apply(t, mode_a, mode_b, scale, pooled)


def loss_sum(a, b, mode, scale, pooled=False):
    """pooled: the caller only COMBINES the result with other terms inside the step (a sum over scales, a stack) and never
    hands it out: the accumulator may then be a slice of the step's zero pool instead of its own zero-fill launch."""
    return LossSumFn.apply(a, b, mode, scale, pooled)


class FeatTapFn(torch.autograd.Function):
    """Identity on a discriminator feature map h = [fake | real] (2N,H,W,C) that also yields the GAN feature-
    matching term  scale * sum |h[:N] - h[N:].detach()|  (pix2pix_model.py:231-241 of the reference).

    Why not slice-then-loss: the slice's backward materialises a zero (2N,...) tensor, copies the half in and
    autograd then ADDS it to the gradient arriving from the next layer -- three passes over every feature map
    (~0.65 ms per G step).  Here the next layer's gradient arrives first (this node sits on the only path to
    it) and the L1 gradient is accumulated into its fake half in place by s2e_loss_grad(accumulate=1).
    nan_grad: the gradient of a NaN difference is NaN (LOSS_L1_NANGRAD) and not torch's sign(NaN) = 0: for use under the gradient
    guard, which can only skip a step whose non-finite features reached the gradient arena.  Finite inputs give the same bits."""

    @staticmethod
    def forward(ctx, h, scale, pooled=False, nan_grad=False):
        _need(h)
        n = h.shape[0] // 2
        a, b = h[:n], h[n:]
        out = _loss_slot(h.device, pooled)
        L.call.s2e_loss_reduce(_dt(h), LOSS_L1, _p(a), _p(b), a.numel(), float(scale), _p(out), _stream())
        ctx.scale = float(scale)
        ctx.grad_mode = LOSS_L1_NANGRAD if nan_grad else LOSS_L1
        ctx.save_for_backward(h)
        ctx.set_materialize_grads(False)
        return h.view_as(h), out

    @staticmethod
    def backward(ctx, gh, gloss):
        h, = ctx.saved_tensors
        n = h.shape[0] // 2
        if gloss is None:
            return gh, None, None, None
        if gh is None:
            gh = torch.zeros_like(h)
        elif not gh.is_contiguous():
            gh = gh.contiguous()
        a, b, ga = h[:n], h[n:], gh[:n]
        gs = gloss.detach().float().contiguous()
        L.call.s2e_loss_grad(_dt(h), ctx.grad_mode, _p(a), _p(b), a.numel(), ctx.scale, _p(gs), _p(ga), 1, _stream())
        return gh, None, None, None


def feat_tap(h, scale, pooled=False, nan_grad=False):
    """-> (h, term): see FeatTapFn.  pooled: as in loss_sum."""
    return FeatTapFn.apply(h, scale, pooled, nan_grad)


# ------------------------------------------------------------------------------ optimizer

def adam_flat_step(p, g, m, v, hyper, skips_m=False):
    """One torch.optim.Adam step over flat fp32 arenas (pix2pix_model.py:92-110 semantics).
    hyper: 7-float DEVICE tensor {lr, beta1, beta2, eps, completed steps, grad_scale, weight_decay}.
    skips_m: the caller knows beta1 == 0 and weight_decay == 0 (the kernel then leaves m alone): only the profiler's byte count uses it."""
    _need(p, g, m, v, hyper)
    LaunchProfiler.run('adam', 0.0, L.call.s2e_adam_flat, (_p(p), _p(g), _p(m), _p(v), p.numel(), _p(hyper), _stream()),
                       # read p, g, m, v + write p, m, v = 28 B per parameter; without the first moment 20 B
                       nbytes=float((5 if skips_m else 7) * 4 * p.numel()))


def adam_flat_ema_step(p, g, m, v, ema, hyper, ema_hyper, skips_m=False):
    """adam_flat_step with the exponential moving average of p kept in `ema` by the same launch (s2e_adam_flat_ema): p, v, m get
    the bits adam_flat_step gives them.  ema_hyper: 2-float DEVICE tensor {decay, start_step}; the step t = completed steps + 1
    copies p into ema while t <= start_step and averages afterwards, ema = decay * ema + (1 - decay) * p."""
    _need(p, g, m, v, ema, hyper, ema_hyper)
    LaunchProfiler.run('adam', 0.0, L.call.s2e_adam_flat_ema, (_p(p), _p(g), _p(m), _p(v), _p(ema), p.numel(), _p(hyper), _p(ema_hyper), _stream()),
                       # adam_flat_step's bytes + the average's own read and write: 7 floats per parameter without the first moment, 9 with it
                       nbytes=float((7 if skips_m else 9) * 4 * p.numel()))


def grad_guard_workspace(n, device):
    """The workspace s2e_grad_guard needs for an arena of n elements: per-block {fp64 sum, first index} records."""
    return torch.empty(int(L.call.s2e_grad_guard_workspace_bytes(int(n))) // 8, dtype=torch.float64, device=device)


def guard_coefficient(norm, max_norm, has_nonfinite=False, skip_nonfinite=False):
    """The rule s2e_grad_guard applies, restated on the host (the kernel is the implementation, this is its documentation): the
    coefficient the guarded Adam step multiplies the gradient by.  norm: |grad_scale| * sqrt(sum g^2) over the finite elements."""
    if has_nonfinite:
        return 0.0 if skip_nonfinite else float('nan')         # a skipped step / the unguarded behaviour
    if max_norm > 0:
        return min(1.0, float(max_norm) / (float(norm) + 1e-6))  # torch.nn.utils.clip_grad_norm_, norm_type = 2
    return 1.0


def grad_guard(g, hyper, guard, first_bad, workspace):
    """Examine the gradient arena g (flat fp32) and write the guard record: guard (8 fp32, DEVICE) = {max_norm, skip_nonfinite | norm,
    coefficient, skipped, clipped, consecutive skips, 0}, first_bad (1 int32, DEVICE) = index of the first non-finite element or -1
    (seg2eye_hip.h: s2e_grad_guard).  Two launches, no atomics, no synchronisation; hyper[5] (grad_scale) enters the norm."""
    _need(g, hyper, guard, first_bad, workspace)
    LaunchProfiler.run('adam', 0.0, L.call.s2e_grad_guard,
                       (_p(g), g.numel(), _p(hyper), _p(guard), _p(first_bad), _p(workspace), workspace.numel() * workspace.element_size(), _stream()),
                       nbytes=float(4 * g.numel()))                             # the guard reads g once


def adam_flat_guarded_step(p, g, m, v, hyper, guard, skips_m=False):
    """adam_flat_step under the guard record grad_guard wrote: coefficient guard[3] == 0 leaves p, m, v and the step count alone,
    any other multiplies grad_scale (1 gives adam_flat_step's bits)."""
    _need(p, g, m, v, hyper, guard)
    LaunchProfiler.run('adam', 0.0, L.call.s2e_adam_flat_guarded, (_p(p), _p(g), _p(m), _p(v), p.numel(), _p(hyper), _p(guard), _stream()),
                       nbytes=float((5 if skips_m else 7) * 4 * p.numel()))     # (adam_flat_step's; a skipped step moves nothing)


def adam_flat_ema_guarded_step(p, g, m, v, ema, hyper, ema_hyper, guard, skips_m=False):
    """adam_flat_ema_step under the guard record: a skipped step leaves the average alone too."""
    _need(p, g, m, v, ema, hyper, ema_hyper, guard)
    LaunchProfiler.run('adam', 0.0, L.call.s2e_adam_flat_ema_guarded,
                       (_p(p), _p(g), _p(m), _p(v), _p(ema), p.numel(), _p(hyper), _p(ema_hyper), _p(guard), _stream()),
                       nbytes=float((7 if skips_m else 9) * 4 * p.numel()))     # (adam_flat_ema_step's)


def _one_shape(a, b, names):
    if a.shape != b.shape:
        raise ValueError('%s of one shape expected, got %s and %s' % (names, tuple(a.shape), tuple(b.shape)))
    _need(a, b)
    return a, b


def _image_pair(x, y):
    """The two images of a float quality op as contiguous (N,H,W) device tensors of x's dtype, detached (y is cast, as openeds_error
    always did).  The entry points take one (N,H,W) for both pointers, so the shapes are compared here -- before the device check."""
    return _one_shape(_single_channel(x.detach()), _single_channel(y.detach().to(x.dtype)), 'x and y')


def _u8_pair(a, b):
    """The same for the ops on uint8 images that already are 0..255."""
    a, b = _single_channel(a), _single_channel(b)
    if a.dtype != torch.uint8 or b.dtype != torch.uint8:
        raise ValueError('uint8 images expected')
    return _one_shape(a, b, 'a and b')


def openeds_error(produced, target):
    """Per-image OpenEDS error of two batches in [-1, 1] (models/networks/loss.py:135-155 `calculate_mse_for_tensors`):
    both mapped to 0..255 with the reference's int truncation, then sqrt(sum d^2) / (H*W).  -> fp32 (N,), no gradient."""
    a, b = _image_pair(produced, target)
    n, h, w = a.shape
    err = torch.empty(n, dtype=torch.float32, device=a.device)
    L.call.s2e_openeds_error(_dt(a), _p(a), _p(b), n, h, w, _p(err), _stream())
    return err


def openeds_error_u8(produced, target):
    """The same on uint8 images that already are 0..255 (loss.py:116-133 `calculate_mse_for_images`)."""
    a, b = _u8_pair(produced, target)
    n, h, w = a.shape
    err = torch.empty(n, dtype=torch.float32, device=a.device)
    L.call.s2e_openeds_error_u8(_p(a), _p(b), n, h, w, _p(err), _stream())
    return err


def _ssim_workspace(n, h, w, device):
    return torch.empty(int(L.call.s2e_ssim_workspace_bytes(n, h, w)) // 8, dtype=torch.float64, device=device)


def _ssim_cost(n, h, w, planes):
    """(algorithmic FLOPs, bytes) of one SSIM launch pair: `planes` separable 11-tap passes per position; the images once, the maps once."""
    pos = n * (h - 10) * (w - 10)
    return float(2 * 2 * 11 * planes * pos), pos


class SsimFn(torch.autograd.Function):
    """ssim[n] of two (N,H,W) batches in [-1, 1] (s2e_ssim_fwd: two launches); the backward is s2e_ssim_bwd on the saved A, B, C maps
    (one launch), for x only.  When x needs no gradient nothing is saved and no maps are allocated."""

    @staticmethod
    def forward(ctx, x, y):
        a, b = _image_pair(x, y)
        n, h, w = a.shape
        out = torch.empty(n, dtype=torch.float32, device=a.device)
        ws = _ssim_workspace(n, h, w, a.device)
        maps = torch.empty(3, n, h - 10, w - 10, dtype=torch.float32, device=a.device) if ctx.needs_input_grad[0] and h > 10 and w > 10 else None
        flops, pos = _ssim_cost(n, h, w, 5)
        LaunchProfiler.run('ssim_fwd', flops, L.call.s2e_ssim_fwd,
                           (_dt(a), _p(a), _p(b), n, h, w, _p(out), _p(maps), _p(ws), ws.numel() * 8, _stream()),
                           nbytes=float(2 * a.numel() * a.element_size() + (12 * pos if maps is not None else 0)))
        if maps is not None:
            ctx.save_for_backward(a, b, maps)
        ctx.x_shape = x.shape
        return out

    @staticmethod
    def backward(ctx, gout):
        if not ctx.saved_tensors:
            return None, None
        a, b, maps = ctx.saved_tensors
        n, h, w = a.shape
        gs = gout.detach().float().contiguous()
        dx = torch.empty_like(a)
        flops, pos = _ssim_cost(n, h, w, 3)
        LaunchProfiler.run('ssim_bwd', flops, L.call.s2e_ssim_bwd, (_dt(a), _p(a), _p(b), _p(maps), _p(gs), n, h, w, _p(dx), _stream()),
                           nbytes=float(3 * a.numel() * a.element_size() + 12 * pos))
        return dx.view(ctx.x_shape), None


def ssim(x, y):
    """Per-image structural similarity of two single-channel batches in [-1, 1] (11-tap Gaussian window, sigma 1.5, valid
    placement, data range 1, no clamp).  -> fp32 (N,), higher is better, 1 for identical images; differentiable in x only (y is cast
    to x's dtype, as openeds_error does)."""
    return SsimFn.apply(x, y)


def ssim_u8(a, b):
    """The same on uint8 images that already are 0..255 (u = a / 255).  -> fp32 (N,), no gradient."""
    a, b = _u8_pair(a, b)
    n, h, w = a.shape
    out = torch.empty(n, dtype=torch.float32, device=a.device)
    ws = _ssim_workspace(n, h, w, a.device)
    flops, _ = _ssim_cost(n, h, w, 5)
    LaunchProfiler.run('ssim_fwd', flops, L.call.s2e_ssim_u8, (_p(a), _p(b), n, h, w, _p(out), _p(ws), ws.numel() * 8, _stream()),
                       nbytes=float(2 * a.numel()))
    return out


MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)    # Wang, Simoncelli, Bovik 2003, as published (sum 1.0001: not renormalised)


def msssim_min_size(levels=len(MSSSIM_WEIGHTS)):
    """The smallest H (and W) with a window position at the last of `levels` levels: 11 << (levels - 1); 176 at five."""
    return 11 << (int(levels) - 1)


def _msssim_weights(weights):
    """-> (levels, a ctypes array of that many floats: the host array the entry points read).  None: the published five."""
    ws = [float(v) for v in (MSSSIM_WEIGHTS if weights is None else weights)]
    if not 1 <= len(ws) <= 5:
        raise ValueError('1 to 5 level weights expected, got %d' % len(ws))
    return len(ws), (L.C.c_float * len(ws))(*ws)


def _msssim_buffers(n, h, w, levels, device, maps):
    """(workspace, pyramid, maps or None): uninitialised, sized by the library's queries (an illegal size gives empty buffers and the
    entry point then says why)."""
    q = L.call
    ws = torch.empty(max(1, int(q.s2e_msssim_workspace_bytes(n, h, w, levels)) // 8), dtype=torch.float64, device=device)
    pyr = torch.empty(int(q.s2e_msssim_pyramid_bytes(n, h, w, levels)) // 4, dtype=torch.float32, device=device)
    mp = torch.empty(int(q.s2e_msssim_maps_bytes(n, h, w, levels)) // 4, dtype=torch.float32, device=device) if maps else None
    return ws, pyr, mp


def _msssim_cost(n, h, w, levels, planes):
    """(algorithmic FLOPs, positions) over the levels, as _ssim_cost counts one."""
    pos = sum(n * max((h >> j) - 10, 0) * max((w >> j) - 10, 0) for j in range(levels))
    return float(2 * 2 * 11 * planes * pos), pos


class MsSsimFn(torch.autograd.Function):
    """(msssim (N,), terms (N,L)) of two (N,H,W) batches in [-1, 1] (s2e_msssim_fwd: three launches); the backward is s2e_msssim_bwd on the
    saved pyramid, maps and coefficients (two launches), for x only.  When x needs no gradient nothing is saved and no maps are allocated."""

    @staticmethod
    def forward(ctx, x, y, weights):
        a, b = _image_pair(x, y)
        n, h, w = a.shape
        levels, wts = _msssim_weights(weights)
        out = torch.empty(n, dtype=torch.float32, device=a.device)
        terms = torch.empty(n, levels, dtype=torch.float32, device=a.device)
        coef = torch.empty(n, levels, dtype=torch.float32, device=a.device)
        ws, pyr, maps = _msssim_buffers(n, h, w, levels, a.device, ctx.needs_input_grad[0])
        if maps is not None and maps.numel() == 0:
            maps = None                                      # (an illegal size: the entry point refuses it below)
        flops, pos = _msssim_cost(n, h, w, levels, 5)
        LaunchProfiler.run('msssim_fwd', flops, L.call.s2e_msssim_fwd,
                           (_dt(a), _p(a), _p(b), n, h, w, levels, wts, _p(out), _p(terms), _p(coef), _p(maps), maps.numel() * 4 if maps is not None else 0,
                            _p(pyr) if pyr.numel() else None, pyr.numel() * 4, _p(ws), ws.numel() * 8, _stream()),
                           nbytes=float(2 * a.numel() * a.element_size() + 3 * pyr.numel() * 4 + (12 * pos if maps is not None else 0)))
        if maps is not None:
            ctx.save_for_backward(a, b, pyr, maps, coef)
        ctx.cfg = (x.shape, levels)
        ctx.mark_non_differentiable(terms)
        return out, terms

    @staticmethod
    def backward(ctx, gout, _gterms):
        if not ctx.saved_tensors:
            return None, None, None
        a, b, pyr, maps, coef = ctx.saved_tensors
        x_shape, levels = ctx.cfg
        n, h, w = a.shape
        gs = gout.detach().float().contiguous()
        dx = torch.empty_like(a)
        gbuf = torch.empty(pyr.numel() // 2, dtype=torch.float32, device=a.device)     # the coarse levels' gradients, at their own resolution
        flops, pos = _msssim_cost(n, h, w, levels, 3)
        LaunchProfiler.run('msssim_bwd', flops, L.call.s2e_msssim_bwd,
                           (_dt(a), _p(a), _p(b), _p(pyr) if pyr.numel() else None, _p(maps), _p(coef), _p(gs), n, h, w, levels,
                            _p(gbuf) if gbuf.numel() else None, gbuf.numel() * 4, _p(dx), _stream()),
                           nbytes=float(3 * a.numel() * a.element_size() + 12 * pos + 3 * pyr.numel() * 4))
        return dx.view(x_shape), None, None


def ms_ssim(x, y, weights=None, return_terms=False):
    """Per-image multi-scale structural similarity of two single-channel batches in [-1, 1] (ssim's window and constants on a
    2 x 2-mean pyramid; the contrast-structure term on every level but the last, the full SSIM on the last; the product of the levels'
    means, each clamped at 1e-3, to the powers `weights`).  weights: one positive number per level, 1 to 5 of them; None = the published
    five, which need H, W >= 176.  -> fp32 (N,), higher is better, 1 for identical images; differentiable in x only (y is cast to x's
    dtype).  return_terms: -> (msssim, terms (N, levels) fp32: the levels' means before the clamp, detached)."""
    out, terms = MsSsimFn.apply(x, y, weights)
    return (out, terms) if return_terms else out


def ms_ssim_terms(x, y, weights=None):
    """The per-level means m_j of ms_ssim (before the clamp) -> fp32 (N, levels), no gradient."""
    return MsSsimFn.apply(x.detach(), y.detach(), weights)[1]


def ms_ssim_u8(a, b, weights=None, return_terms=False):
    """ms_ssim on uint8 images that already are 0..255 (u = a / 255).  -> fp32 (N,), no gradient."""
    a, b = _u8_pair(a, b)
    n, h, w = a.shape
    levels, wts = _msssim_weights(weights)
    out = torch.empty(n, dtype=torch.float32, device=a.device)
    terms = torch.empty(n, levels, dtype=torch.float32, device=a.device)
    ws, pyr, _ = _msssim_buffers(n, h, w, levels, a.device, False)
    flops, _ = _msssim_cost(n, h, w, levels, 5)
    LaunchProfiler.run('msssim_fwd', flops, L.call.s2e_msssim_u8,
                       (_p(a), _p(b), n, h, w, levels, wts, _p(out), _p(terms), _p(pyr) if pyr.numel() else None, pyr.numel() * 4, _p(ws),
                        ws.numel() * 8, _stream()), nbytes=float(2 * a.numel() + 3 * pyr.numel() * 4))
    return (out, terms) if return_terms else out


_FFL_TABLES = {}     # (device index, H, W) -> the DFT tables of s2e_ffl_tables (fp32, they depend on the size alone)


def ffl_tables(h, w, device):
    """The DFT tables the s2e_ffl_* entries read for H x W images, built on the device by one launch (s2e_ffl_tables) and cached per
    (device, H, W).  A model that uses the term builds them at construction; on a cache miss while a hipGraph is being captured the
    tables are built into a buffer of the capture, as every other buffer of the call is, and not cached (the graph owns that memory).
    An illegal size gives a one-element buffer and the entry point that gets it says why."""
    device = torch.device(device)
    if device.type != 'cuda':
        raise L.Seg2EyeHipError('seg2eye_amd ops run on the GPU only (got a %s device); there is no CPU fallback' % device)
    key = (device.index if device.index is not None else torch.cuda.current_device(), int(h), int(w))
    t = _FFL_TABLES.get(key)
    if t is None:
        nbytes = int(L.call.s2e_ffl_tables_bytes(int(h), int(w)))
        t = torch.empty(max(1, nbytes // 4), dtype=torch.float32, device=device)
        if nbytes:
            L.call.s2e_ffl_tables(int(h), int(w), _p(t), nbytes, _stream())
            if not torch.cuda.is_current_stream_capturing():
                _FFL_TABLES[key] = t
    return t


def _ffl_cost(n, h, w):
    """(algorithmic FLOPs of the two real matrix products of one direction, bytes of the half spectrum): rows H x W x 2 Wh, columns
    2H x 2H x Wh, two FLOPs per multiply-add."""
    wh = w // 2 + 1
    return float(2 * n * (h * w * 2 * wh + 2 * h * 2 * h * wh)), 8 * n * h * wh


class FocalFreqFn(torch.autograd.Function):
    """ffl (N,) of two (N,H,W) batches (s2e_ffl_fwd: three launches); the backward is s2e_ffl_bwd on the saved spectrum and coefficients
    (two launches), for x only.  When x needs no gradient no spectrum is allocated and nothing is saved."""

    @staticmethod
    def forward(ctx, x, y, alpha):
        a, b = _image_pair(x, y)
        n, h, w = a.shape
        alpha = float(alpha)
        tab = ffl_tables(h, w, a.device)
        out = torch.empty(n, dtype=torch.float32, device=a.device)
        coef = torch.empty(n, dtype=torch.float32, device=a.device)
        ws = torch.empty(max(1, int(L.call.s2e_ffl_workspace_bytes(n, h, w)) // 4), dtype=torch.float32, device=a.device)
        spec = None
        if ctx.needs_input_grad[0]:
            spec = torch.empty(int(L.call.s2e_ffl_spectrum_bytes(n, h, w)) // 4, dtype=torch.float32, device=a.device)
            if spec.numel() == 0:
                spec = None                                      # (an illegal size: the entry point refuses it below)
        flops, sbytes = _ffl_cost(n, h, w)
        LaunchProfiler.run('ffl_fwd', flops, L.call.s2e_ffl_fwd,
                           (_dt(a), _p(a), _p(b), n, h, w, alpha, _p(tab), tab.numel() * 4, _p(out), _p(coef), _p(spec),
                            spec.numel() * 4 if spec is not None else 0, _p(ws), ws.numel() * 4, _stream()),
                           nbytes=float(2 * a.numel() * a.element_size() + 2 * sbytes + (sbytes if spec is not None else 0)))
        if spec is not None:
            ctx.save_for_backward(spec, coef, tab)
        ctx.cfg = (x.shape, (n, h, w), a.dtype, alpha)
        return out

    @staticmethod
    def backward(ctx, gout):
        if not ctx.saved_tensors:
            return None, None, None
        spec, coef, tab = ctx.saved_tensors
        x_shape, (n, h, w), dtype, alpha = ctx.cfg
        gs = gout.detach().float().contiguous()
        dx = torch.empty(n, h, w, dtype=dtype, device=spec.device)
        ws = torch.empty(int(L.call.s2e_ffl_workspace_bytes(n, h, w)) // 4, dtype=torch.float32, device=spec.device)
        flops, sbytes = _ffl_cost(n, h, w)
        LaunchProfiler.run('ffl_bwd', flops, L.call.s2e_ffl_bwd,
                           (_dt(dtype), _p(spec), _p(coef), _p(gs), n, h, w, alpha, _p(tab), tab.numel() * 4, _p(ws), ws.numel() * 4, _p(dx), _stream()),
                           nbytes=float(dx.numel() * dx.element_size() + 3 * sbytes))
        return dx.view(x_shape), None, None


def focal_freq_loss(x, y, alpha=1.0):
    """Per-image focal frequency loss (Jiang et al., ICCV 2021) of two single-channel batches, (N,1,H,W) or (N,H,W), fp32 or
    bf16, in the tensors' own units: with Z the orthonormal 2-D DFT of x - y and dist = |Z|^2, ffl[n] = mean over the H W bins of
    w dist, w = dist^(alpha/2) / max_bins dist^(alpha/2) (a constant of the step; alpha in [0, 4]; alpha = 0: w = 1 and ffl is the mean
    squared error).  Whole image, per image, no log.  -> fp32 (N,), lower is better, 0 for identical images; differentiable in x only
    (y is cast to x's dtype)."""
    return FocalFreqFn.apply(x, y, alpha)


def focal_freq_loss_u8(a, b, alpha=1.0):
    """focal_freq_loss on uint8 images that already are 0..255 (u = a / 255).  -> fp32 (N,), no gradient."""
    a, b = _u8_pair(a, b)
    n, h, w = a.shape
    tab = ffl_tables(h, w, a.device)
    out = torch.empty(n, dtype=torch.float32, device=a.device)
    ws = torch.empty(max(1, int(L.call.s2e_ffl_workspace_bytes(n, h, w)) // 4), dtype=torch.float32, device=a.device)
    flops, sbytes = _ffl_cost(n, h, w)
    LaunchProfiler.run('ffl_fwd', flops, L.call.s2e_ffl_u8,
                       (_p(a), _p(b), n, h, w, float(alpha), _p(tab), tab.numel() * 4, _p(out), _p(ws), ws.numel() * 4, _stream()),
                       nbytes=float(2 * a.numel() + 2 * sbytes))
    return out


_REGION_NORMS = {'l1': L.REGION_L1, 'l2': L.REGION_L2}


def _region_workspace(n, h, w, ncls, device):
    return torch.empty(int(L.call.s2e_region_workspace_bytes(n, h, w, ncls)) // 8, dtype=torch.float64, device=device)


def _region_label(label, n):
    """uint8 (N,Hl,Wl), contiguous ((N,1,Hl,Wl) accepted)."""
    if label.dim() == 4 and label.shape[1] == 1:
        label = label[:, 0]
    if label.dim() != 3 or label.shape[0] != n or label.dtype != torch.uint8:
        raise ValueError('label: a uint8 map (N,Hl,Wl) with the images\' N expected, got %s %s' % (label.dtype, tuple(label.shape)))
    return label.contiguous()


def _region_ncls(ncls):
    if not 1 <= int(ncls) <= 8:
        raise ValueError('1 to 8 classes expected, got %d' % ncls)
    return int(ncls)


class RegionLossFn(torch.autograd.Function):
    """(loss, stats) of s2e_region_loss_fwd (two launches); the backward is s2e_region_loss_bwd on the saved images, label and the
    per-class coefficients the fold wrote (one launch), for x only.  When x needs no gradient nothing is saved."""

    @staticmethod
    def forward(ctx, x, y, label, weights, norm):
        a, b = _image_pair(x, y)
        lb = _region_label(label, a.shape[0])
        _need(lb, weights)
        n, h, w = a.shape
        ncls = weights.numel()
        stats = torch.empty(n, ncls, 3, dtype=torch.float64, device=a.device)
        loss = torch.empty((), dtype=torch.float32, device=a.device)
        coef = torch.empty(ncls, dtype=torch.float32, device=a.device)
        ws = _region_workspace(n, h, w, ncls, a.device)
        LaunchProfiler.run('region_fwd', float(4 * a.numel()), L.call.s2e_region_loss_fwd,
                           (_dt(a), _p(a), _p(b), _p(lb), n, h, w, lb.shape[1], lb.shape[2], ncls, norm, _p(weights), _p(stats), _p(loss),
                            _p(coef), _p(ws), ws.numel() * 8, _stream()),
                           nbytes=float(2 * a.numel() * a.element_size() + (lb.numel() if lb.shape[1:] == a.shape[1:] else a.numel())))
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(a, b, lb, coef)
        ctx.cfg = (x.shape, ncls, norm)
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    def backward(ctx, gloss, _gstats):
        if not ctx.saved_tensors:
            return None, None, None, None, None
        a, b, lb, coef = ctx.saved_tensors
        x_shape, ncls, norm = ctx.cfg
        n, h, w = a.shape
        gs = gloss.detach().float().contiguous()
        dx = torch.empty_like(a)
        LaunchProfiler.run('region_bwd', float(3 * a.numel()), L.call.s2e_region_loss_bwd,
                           (_dt(a), _p(a), _p(b), _p(lb), _p(coef), _p(gs), n, h, w, lb.shape[1], lb.shape[2], ncls, norm, _p(dx), _stream()),
                           nbytes=float(3 * a.numel() * a.element_size() + (lb.numel() if lb.shape[1:] == a.shape[1:] else a.numel())))
        return dx.view(x_shape), None, None, None, None


def region_loss(x, y, label, weights, norm='l1'):
    """The class-balanced reconstruction error of two single-channel batches in [-1, 1]: per class c the mean of |x - y|
    ('l1') or (x - y)^2 ('l2') over the batch's pixels of that class, the classes present in the batch averaged by `weights` (fp32,
    one per class, on the device; or a sequence of numbers).  label: uint8 (N,Hl,Wl), looked up at [(r Hl) // H, (c Wl) // W]; a class
    >= len(weights) belongs to no region.  -> (loss: 0-dim fp32, differentiable in x only (y is cast to x's dtype);
    stats: (N, ncls, 3) float64 {count, sum |d|, sum d^2} per image and class, detached)."""
    if norm not in _REGION_NORMS:
        raise ValueError("norm: 'l1' or 'l2' expected, got %r" % (norm,))
    if not torch.is_tensor(weights):
        weights = torch.tensor([float(v) for v in weights], dtype=torch.float32, device=x.device)
    if weights.dtype != torch.float32 or weights.dim() != 1:
        raise ValueError('weights: one fp32 number per class expected')
    _region_ncls(weights.numel())
    return RegionLossFn.apply(x, y, label, weights, _REGION_NORMS[norm])


def region_stats_u8(a, b, label, ncls):
    """{count, sum |a - b|, sum (a - b)^2} per image and class of uint8 images that already are 0..255, by the label lookup of
    region_loss.  -> (N, ncls, 3) float64, every number exact; no gradient."""
    ncls = _region_ncls(ncls)
    a, b = _u8_pair(a, b)
    lb = _region_label(label, a.shape[0])
    _need(lb)
    n, h, w = a.shape
    stats = torch.empty(n, ncls, 3, dtype=torch.float64, device=a.device)
    ws = _region_workspace(n, h, w, ncls, a.device)
    LaunchProfiler.run('region_fwd', float(4 * a.numel()), L.call.s2e_region_stats_u8,
                       (_p(a), _p(b), _p(lb), n, h, w, lb.shape[1], lb.shape[2], ncls, _p(stats), _p(ws), ws.numel() * 8, _stream()),
                       nbytes=float(3 * a.numel()))
    return stats


def resize_to255(x, w=400, h=640):
    """Bilinear resize (cv2.INTER_LINEAR rule) of single-channel [-1, 1] images to (h, w), then 0..255 with int truncation
    (data/postprocessor.py:92-107 `to_255resized_imagebatch`).  -> uint8 (N,1,h,w)."""
    a = _single_channel(x.detach())
    _need(a)
    n, hi, wi = a.shape
    out = torch.empty(n, 1, h, w, dtype=torch.uint8, device=a.device)
    L.call.s2e_resize_to255(_dt(a), _p(a), n, hi, wi, _p(out), h, w, _stream())
    return out
