"""Eye geometry: the integer moments of the rim pixels of uint8 label maps (`rim_moments`), from which the host fits an
ellipse per curve (seg2eye_amd/eye_geometry.py), and the repaint of the maps from fitted conics (`ellipse_paint`).  Everything is per
image and every result an integer or a copy; the rules are stated in include/seg2eye_hip.h.  Two calls give the same bytes."""
import numpy as np
import torch

from .. import _lib as L
from .core import LaunchProfiler, _need, _p, _stream

MAX_CLASSES = 16
MAX_SIDE = 1024
MAX_CURVES = 4
RIM_WIDTH = 18              # n, ox, oy and the 15 centred sums
_WORKSPACES = {}            # (device, N, H, W, K) -> uint8 tensor, as the library sizes it


def _ncls(ncls):
    ncls = int(ncls)
    if not 1 <= ncls <= MAX_CLASSES:
        raise ValueError('ncls = %d (1 to %d classes)' % (ncls, MAX_CLASSES))
    return ncls


def default_curves(ncls):
    """((in classes, out classes), ...) for the OpenEDS classes 0 skin, 1 sclera, 2 iris, 3 pupil: the limbus -- iris or pupil against
    the sclera -- and the pupil's edge against the iris.  Where a lid covers either there is no rim pixel.  With fewer than 4 classes:
    one curve, the highest class against the one below it; with 1 class there is no curve to name."""
    ncls = _ncls(ncls)
    if ncls >= 4:
        return (((2, 3), (1,)), ((3,), (2,)))
    if ncls >= 2:
        return (((ncls - 1,), (ncls - 2,)),)
    raise ValueError('ncls = 1: a curve needs two classes')


def _labels(labels, ncls):
    """The checks that need no device: they come first, as in ops/mask_clean.py."""
    if labels.dtype != torch.uint8:
        raise ValueError('uint8 label maps expected, got %s' % labels.dtype)
    if labels.dim() != 3 or min(labels.shape) < 1 or max(labels.shape[1:]) > MAX_SIDE:
        raise ValueError('labels: (N, H, W) with H, W <= %d expected, got %s' % (MAX_SIDE, tuple(labels.shape)))
    return _ncls(ncls)


def _class_set(what, classes, ncls):
    try:
        classes = tuple(classes)
    except TypeError:
        raise ValueError('%s = %r (a sequence of classes)' % (what, classes))
    bits = 0
    for c in classes:
        if isinstance(c, str) or int(c) != c or not 0 <= int(c) < ncls:
            raise ValueError('%s: class %r (0 to %d)' % (what, c, ncls - 1))
        bits |= 1 << int(c)
    return bits


def _curves(curves, ncls):
    """None, or K pairs (in classes, out classes) -> the two host arrays of K uint16 class sets the library reads."""
    curves = default_curves(ncls) if curves is None else tuple(curves)
    if not 1 <= len(curves) <= MAX_CURVES:
        raise ValueError('curves: %d of them (1 to %d per call)' % (len(curves), MAX_CURVES))
    ins, outs = [], []
    for k, pair in enumerate(curves):
        if len(pair) != 2:
            raise ValueError('curves[%d] = %r (a pair: in classes, out classes)' % (k, pair))
        a, b = _class_set('curves[%d] in' % k, pair[0], ncls), _class_set('curves[%d] out' % k, pair[1], ncls)
        if not a or not b:
            raise ValueError('curves[%d]: an empty class set' % k)
        if a & b:
            raise ValueError('curves[%d]: the sets overlap' % k)
        ins.append(a)
        outs.append(b)
    return np.array(ins, dtype=np.uint16), np.array(outs, dtype=np.uint16)


def _workspace(device, n, h, w, k):
    key = (str(device), n, h, w, k)
    ws = _WORKSPACES.get(key)
    if ws is None:
        if len(_WORKSPACES) >= 8:
            _WORKSPACES.clear()
        ws = _WORKSPACES[key] = torch.empty(int(L.call.s2e_rim_moments_workspace_bytes(n, h, w, k)), dtype=torch.uint8, device=device)
    return ws


def rim_moments(labels, ncls=4, curves=None):
    """labels (N, H, W) uint8 -> int64 (N, K, 18): per image and curve the number of rim pixels, the origin (ox, oy) -- their mean,
    rounded half up -- and the 15 sums of (x - ox)^i (y - oy)^j, i + j <= 4, by degree and then by j.  curves: K <= 4 pairs
    (in classes, out classes), default default_curves(ncls); a rim pixel is one of an `in` class with a 4-neighbour of an `out` class."""
    ncls = _labels(labels, ncls)
    ins, outs = _curves(curves, ncls)
    _need(labels)
    n, h, w = labels.shape
    k = len(ins)
    rim = torch.empty(n, k, RIM_WIDTH, dtype=torch.int64, device=labels.device)
    ws = _workspace(labels.device, n, h, w, k)
    LaunchProfiler.run('geometry', 0.0, L.call.s2e_rim_moments,
                       (_p(labels), n, h, w, ncls, k, ins.ctypes.data, outs.ctypes.data, _p(rim), _p(ws), ws.numel(), _stream()),
                       nbytes=float(2 * n * h * w))                  # the labels once per pass
    return rim


def ellipse_paint(labels, conic, origin, valid, ncls=4, paint=None, keep=(0,), base=1):
    """labels (N, H, W) uint8, conic (N, K, 6) float64, origin (N, K, 2) int32, valid (N, K) uint8 -> uint8 (N, H, W).  An image with
    a valid byte 0 comes back unchanged; otherwise a pixel whose label is >= ncls or in `keep` stays, every other pixel becomes `base`
    and then, for k ascending, paint[k] where the conic Q_k <= 0.  paint: default the classes 2, 3, ... for the default curves."""
    ncls = _labels(labels, ncls)
    if conic.dtype != torch.float64 or conic.dim() != 3 or conic.shape[0] != labels.shape[0] or conic.shape[2] != 6 or not 1 <= conic.shape[1] <= MAX_CURVES:
        raise ValueError('conic: float64 (N, K <= %d, 6) expected, got %s %s' % (MAX_CURVES, conic.dtype, tuple(conic.shape)))
    k = conic.shape[1]
    if origin.dtype != torch.int32 or tuple(origin.shape) != (labels.shape[0], k, 2):
        raise ValueError('origin: int32 (N, K, 2) expected, got %s %s' % (origin.dtype, tuple(origin.shape)))
    if valid.dtype != torch.uint8 or tuple(valid.shape) != (labels.shape[0], k):
        raise ValueError('valid: uint8 (N, K) expected, got %s %s' % (valid.dtype, tuple(valid.shape)))
    if paint is None:
        paint = tuple(pair[0][0] for pair in default_curves(ncls))
    paint = tuple(paint)
    if len(paint) != k:
        raise ValueError('paint: %d entries for %d curves' % (len(paint), k))
    for i, c in enumerate(paint):
        if isinstance(c, str) or int(c) != c or not 0 <= int(c) < ncls:
            raise ValueError('paint[%d] = %r (a class below %d)' % (i, c, ncls))
    if isinstance(base, str) or int(base) != base or not 0 <= int(base) < ncls:
        raise ValueError('base = %r (a class below %d)' % (base, ncls))
    keep_bits = _class_set('keep', keep, ncls)
    paint_bytes = np.array([int(c) for c in paint], dtype=np.uint8)
    _need(labels, conic, origin, valid)
    n, h, w = labels.shape
    out = torch.empty_like(labels)
    LaunchProfiler.run('geometry', 0.0, L.call.s2e_ellipse_paint,
                       (_p(labels), n, h, w, ncls, k, _p(conic), _p(origin), _p(valid), paint_bytes.ctypes.data, keep_bits, int(base), _p(out), _stream()),
                       nbytes=float(2 * n * h * w))                  # the labels in, the mask out
    return out
