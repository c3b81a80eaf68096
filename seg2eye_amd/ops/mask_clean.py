"""The mask cleaner: the connected components of uint8 label maps (`mask_components`) and the maps with, per class, only
the kept components left and every other pixel given the class of the nearest kept pixel (`mask_clean`).  Everything is integer and
per image; the rule is stated in include/seg2eye_hip.h.  Two calls give the same bytes."""
import numpy as np
import torch

from .. import _lib as L
from .core import LaunchProfiler, _need, _p, _stream

MAX_CLASSES = 16
MAX_SIDE = 1024
MODES = {'all': L.MASK_ALL, 'largest': L.MASK_LARGEST, 'border': L.MASK_BORDER}
_WORKSPACES = {}            # (device, N, H, W, ncls) -> uint8 tensor, as the library sizes it


def default_modes(ncls):
    """Class 0 (the skin, which may lie in two pieces above and below the eye) keeps the components that touch the frame, so that an
    island of it inside the eye is a hole; every other class keeps its largest component."""
    ncls = int(ncls)
    if not 1 <= ncls <= MAX_CLASSES:
        raise ValueError('ncls = %d (1 to %d classes)' % (ncls, MAX_CLASSES))
    return (L.MASK_BORDER,) + (L.MASK_LARGEST,) * (ncls - 1)


def _labels(labels, ncls, conn):
    """The checks that need no device: they come first, as in _image_pair.  -> (ncls, conn)"""
    if labels.dtype != torch.uint8:
        raise ValueError('uint8 label maps expected, got %s' % labels.dtype)
    if labels.dim() != 3 or min(labels.shape) < 1 or max(labels.shape[1:]) > MAX_SIDE:
        raise ValueError('labels: (N, H, W) with H, W <= %d expected, got %s' % (MAX_SIDE, tuple(labels.shape)))
    conn, ncls = int(conn), int(ncls)
    if conn not in (4, 8):
        raise ValueError('conn = %d (4 or 8)' % conn)
    if not 1 <= ncls <= MAX_CLASSES:
        raise ValueError('ncls = %d (1 to %d classes)' % (ncls, MAX_CLASSES))
    return ncls, conn


def _modes(modes, ncls):
    """None, or ncls entries of 0 / 1 / 2 or 'all' / 'largest' / 'border' -> the host bytes the library reads."""
    modes = default_modes(ncls) if modes is None else tuple(MODES.get(m, m) if isinstance(m, str) else m for m in modes)
    if len(modes) != ncls:
        raise ValueError('modes: %d entries for %d classes' % (len(modes), ncls))
    for c, m in enumerate(modes):
        if isinstance(m, str) or int(m) != m or not 0 <= int(m) <= 2:
            raise ValueError("modes[%d] = %r (0 'all', 1 'largest' or 2 'border')" % (c, m))
    return np.array([int(m) for m in modes], dtype=np.uint8)


def _workspace(device, n, h, w, ncls):
    key = (str(device), n, h, w, ncls)
    ws = _WORKSPACES.get(key)
    if ws is None:
        if len(_WORKSPACES) >= 8:
            _WORKSPACES.clear()
        ws = _WORKSPACES[key] = torch.empty(int(L.call.s2e_mask_clean_workspace_bytes(n, h, w, ncls)), dtype=torch.uint8, device=device)
    return ws


def mask_components(labels, ncls=4, conn=8):
    """labels (N, H, W) uint8 -> int32 (N, H, W): the id of the pixel's component -- the smallest linear index y W + x among the pixels
    of its label that are conn-adjacent to it, step by step -- and -1 for a label >= ncls."""
    ncls, conn = _labels(labels, ncls, conn)
    _need(labels)
    n, h, w = labels.shape
    comp = torch.empty(n, h, w, dtype=torch.int32, device=labels.device)
    LaunchProfiler.run('mask_clean', 0.0, L.call.s2e_mask_components, (_p(labels), n, h, w, ncls, conn, _p(comp), _stream()),
                       nbytes=float(n * h * w * (1 + 4 + 4)))        # the labels read, the parents written and read once
    return comp


def mask_clean(labels, ncls=4, conn=8, modes=None, return_stats=False):
    """labels (N, H, W) uint8 -> uint8 (N, H, W): per class the kept components (modes, default default_modes(ncls)), every other
    pixel the class of the nearest kept pixel, a tie to the lower class; with return_stats also int32 (N, ncls, 4): components found,
    pixels before, pixels removed, pixels after, per image and class."""
    ncls, conn = _labels(labels, ncls, conn)
    mode_bytes = _modes(modes, ncls)
    _need(labels)
    n, h, w = labels.shape
    out = torch.empty_like(labels)
    stats = torch.empty(n, ncls, 4, dtype=torch.int32, device=labels.device) if return_stats else None
    ws = _workspace(labels.device, n, h, w, ncls)
    LaunchProfiler.run('mask_clean', 0.0, L.call.s2e_mask_clean,
                       (_p(labels), n, h, w, ncls, conn, mode_bytes.ctypes.data, _p(out), _p(stats), _p(ws), ws.numel(), _stream()),
                       nbytes=float(n * h * w * (1 + 1 + 4 + 4)))    # labels in, mask out, the parent array once each way
    return (out, stats) if return_stats else out
