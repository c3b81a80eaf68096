"""Paired augmentation of the segmenter's training data: `augment_pairs` warps a batch of uint8 frames and their label
maps by one affine transform per pair, draws line occluders on the frames and sends the frames through a per-pair table -- one HIP
launch (csrc/seg_augment.hip; the integer rule is stated in include/seg2eye_hip.h) --, and `AugmentRule` draws the parameters of a
batch on the host.

The draw.  `rule.draw(rng, n, h, w)` makes exactly one call u = rng.rand(n, 57) and reads, per frame:
  column 0      the frame is augmented at all iff u < prob; otherwise: the identity matrix, the identity tables, no line
  column 1      angle   theta = (2u - 1) rotate degrees, as radians: theta_deg * (pi / 180)
  column 2      scale   s = exp((2u - 1) ln scale)
  columns 3, 4  shift   tx = (2u - 1) translate w,  ty = (2u - 1) translate h
  column 5      gamma   g = exp((2u - 1) ln gamma)
  column 6      gain    1 + (2u - 1) contrast
  column 7      bias    (2u - 1) brightness
  column 8      number of lines  min(floor(u (lines + 1)), lines)
  columns 9 + 6 j .. 14 + 6 j   line j: floor(u w), floor(u h), floor(u w), floor(u h), width 1 + floor(3 u), value min(floor(256 u), 255)
The column count does not depend on the rule: turning one augmentation on or off never shifts another's stream.

The matrix maps an OUTPUT pixel to its source: the inverse of "rotate by theta and scale by s about the centre (cx, cy) = ((w - 1) / 2,
(h - 1) / 2), then shift by (tx, ty)".  In float64, with a = cos(theta) / s and b = sin(theta) / s:
  A0 = rint(65536 a), A1 = rint(65536 b), A3 = -A1, A4 = A0
  A2 = rint(65536 cx - (A0 (cx + tx) + A1 (cy + ty))),  A5 = rint(65536 cy - (A3 (cx + tx) + A4 (cy + ty)))   (clipped to int32)
A2 and A5 are formed from the ROUNDED A0 .. A4: the output point centre + shift reads the source centre to within half a unit of Q16
whatever the rounding of the other four did, and zero amplitudes give exactly [65536, 0, 0, 0, 65536, 0].

The tables.  For byte b: c = clip(gain (b / 255) ** g + bias, 0, 1) in float64; lut_f32 = (c - 0.5) / 0.5 rounded to fp32, lut_u8 =
rint(255 c).  The identity triple (g = 1, gain = 1, bias = 0) gives `preprocess.normalize_lut()` itself and arange(256)."""
import collections
import math

import numpy as np
import torch

from .. import _lib as L
from .core import LaunchProfiler, _need, _p, _stream
from .preprocess import normalize_lut

MAX_SIDE = 4096
MAX_LINES = 8
DRAW_COLUMNS = 9 + 6 * MAX_LINES
Q16 = 65536
IDENTITY = (Q16, 0, 0, 0, Q16, 0)

AugmentParams = collections.namedtuple('AugmentParams', 'affine lines lut_f32 lut_u8')
AugmentParams.__doc__ = """Host numpy arrays for n pairs: affine (n, 6) int32 Q16; lines (n, L, 6) int32, or None for no line; lut_f32 (n, 256)
float32 and lut_u8 (n, 256) uint8, each None where its output is never asked for."""


def photometric_luts(gamma, gain, bias):
    """-> (float32 [256], uint8 [256]) of one (gamma, gain, bias); the identity triple gives normalize_lut() and arange(256)."""
    if gamma == 1.0 and gain == 1.0 and bias == 0.0:
        return normalize_lut().numpy(), np.arange(256, dtype=np.uint8)
    c = np.clip(gain * (np.arange(256, dtype=np.float64) / 255.0) ** gamma + bias, 0.0, 1.0)
    return ((c - 0.5) / 0.5).astype(np.float32), np.rint(255.0 * c).astype(np.uint8)


def affine_q16(theta_deg, scale, tx, ty, h, w):
    """The six Q16 coefficients (int64, within int32) of one frame: see the module's text."""
    theta = theta_deg * (math.pi / 180.0)
    a, b = np.cos(theta) / scale, np.sin(theta) / scale
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    A0, A1 = np.rint(Q16 * a), np.rint(Q16 * b)
    A3, A4 = -A1, A0
    A2 = np.rint(Q16 * cx - (A0 * (cx + tx) + A1 * (cy + ty)))
    A5 = np.rint(Q16 * cy - (A3 * (cx + tx) + A4 * (cy + ty)))
    return np.clip(np.array([A0, A1, A2, A3, A4, A5], dtype=np.float64), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


def identity_params(n, lines=0):
    """The parameters that change nothing: out_u8 == img, out_lab == lab, out_f32 == normalize_lut()[img]."""
    lut_f, lut_b = photometric_luts(1.0, 1.0, 0.0)
    return AugmentParams(np.tile(np.array(IDENTITY, dtype=np.int32), (n, 1)), np.zeros((n, lines, 6), dtype=np.int32) if lines else None,
                         np.tile(lut_f, (n, 1)), np.tile(lut_b, (n, 1)))


class AugmentRule:
    """What `segment.train_segmenter(..., augment=rule)` draws per batch.  The amplitudes (0 / 1 = off): rotate in degrees [0, 180],
    scale and gamma as factors [1, 4] (drawn log-uniformly in [1 / v, v]), translate and brightness as shares [0, 1] of the side /
    of the grey range, contrast [0, 1), lines [0, 8] occluders at the most, prob [0, 1] the share of the frames augmented at all."""
    RANGES = dict(prob=(0.0, 1.0), rotate=(0.0, 180.0), scale=(1.0, 4.0), translate=(0.0, 1.0), gamma=(1.0, 4.0), contrast=(0.0, 1.0),
                  brightness=(0.0, 1.0), lines=(0, MAX_LINES))

    def __init__(self, prob=1.0, rotate=0.0, scale=1.0, translate=0.0, gamma=1.0, contrast=0.0, brightness=0.0, lines=0):
        given = dict(prob=prob, rotate=rotate, scale=scale, translate=translate, gamma=gamma, contrast=contrast, brightness=brightness, lines=lines)
        for k, v in given.items():
            lo, hi = self.RANGES[k]
            ok = isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and lo <= v <= hi
            if k == 'lines':
                ok = ok and int(v) == v
            if k == 'contrast':
                ok = ok and v < 1.0
            if not ok:
                raise ValueError('--aug_%s: a value in [%s, %s%s expected, got %r' % (k, lo, hi, ')' if k == 'contrast' else ']', v))
            setattr(self, k, int(v) if k == 'lines' else float(v))

    def __repr__(self):
        return 'AugmentRule(%s)' % ', '.join('%s=%r' % (k, getattr(self, k)) for k in self.RANGES)

    def is_identity(self):
        return (self.prob == 0.0 or (self.rotate == 0.0 and self.scale == 1.0 and self.translate == 0.0 and self.gamma == 1.0
                                     and self.contrast == 0.0 and self.brightness == 0.0 and self.lines == 0))

    def draw(self, rng, n, h, w):
        """-> AugmentParams for n frames of h x w from ONE rng.rand(n, 57); lines is None when the rule draws none."""
        u = rng.rand(n, DRAW_COLUMNS)
        on = u[:, 0] < self.prob
        s = 2.0 * u - 1.0
        theta = s[:, 1] * self.rotate
        scale = np.exp(s[:, 2] * math.log(self.scale))
        tx, ty = s[:, 3] * self.translate * w, s[:, 4] * self.translate * h
        gamma = np.exp(s[:, 5] * math.log(self.gamma))
        gain, bias = 1.0 + s[:, 6] * self.contrast, s[:, 7] * self.brightness
        count = np.minimum(np.floor(u[:, 8] * (self.lines + 1)), self.lines).astype(np.int64)
        p = identity_params(n, self.lines)
        for i in np.nonzero(on)[0]:
            p.affine[i] = affine_q16(theta[i], scale[i], tx[i], ty[i], h, w)
            p.lut_f32[i], p.lut_u8[i] = photometric_luts(gamma[i], gain[i], bias[i])
            for j in range(count[i]):
                c = u[i, 9 + 6 * j:15 + 6 * j]
                p.lines[i, j] = (math.floor(c[0] * w), math.floor(c[1] * h), math.floor(c[2] * w), math.floor(c[3] * h),
                                 1 + math.floor(3 * c[4]), min(math.floor(256 * c[5]), 255))
        return p


def _plane(t, what, like=None):
    if t.dtype != torch.uint8 or t.dim() != 3 or min(t.shape) < 1 or max(t.shape[1:]) > MAX_SIDE:
        raise ValueError('%s: uint8 (n, h, w) with h, w <= %d expected, got %s %s' % (what, MAX_SIDE, t.dtype, tuple(t.shape)))
    if like is not None and t.shape != like.shape:
        raise ValueError('%s: %s, the frames are %s' % (what, tuple(t.shape), tuple(like.shape)))


def _table(a, what, dtype, shape):
    a = np.ascontiguousarray(a)
    if a.dtype != dtype or a.shape != shape:
        raise ValueError('params.%s: %s %s expected, got %s %s' % (what, np.dtype(dtype).name, shape, a.dtype, a.shape))
    return a


def augment_pairs(img_u8, lab_u8, params, want_f32=True, want_u8=False):
    """img_u8, lab_u8 (n, h, w) uint8 on the device (either may be None), params an AugmentParams of host arrays -> (x fp32 (n, h, w) or
    None, x_u8 or None, y uint8 or None): the frames warped, occluded and sent through the tables, the label maps warped by the same
    matrices.  The host arrays go up in one small copy; one launch."""
    if img_u8 is None and lab_u8 is None:
        raise ValueError('augment_pairs: frames, label maps or both')
    want_f32, want_u8 = bool(want_f32) and img_u8 is not None, bool(want_u8) and img_u8 is not None
    if img_u8 is not None:
        _plane(img_u8, 'img_u8')
    if lab_u8 is not None:
        _plane(lab_u8, 'lab_u8', img_u8)
    first = img_u8 if img_u8 is not None else lab_u8
    n, h, w = first.shape
    if not (want_f32 or want_u8 or lab_u8 is not None):
        raise ValueError('augment_pairs: no output asked for')
    parts = [_table(params.affine, 'affine', np.int32, (n, 6))]
    nl = 0
    if params.lines is not None and (want_f32 or want_u8):
        nl = np.shape(params.lines)[1] if np.ndim(params.lines) == 3 else -1
        if not 0 <= nl <= MAX_LINES:
            raise ValueError('params.lines: int32 (n, L <= %d, 6) expected, got %s' % (MAX_LINES, np.shape(params.lines)))
        if nl:
            parts.append(_table(params.lines, 'lines', np.int32, (n, nl, 6)))
    for want, what, dtype in ((want_f32, 'lut_f32', np.float32), (want_u8, 'lut_u8', np.uint8)):
        if want:
            if getattr(params, what) is None:
                raise ValueError('params.%s is None and its output is asked for' % what)
            parts.append(_table(getattr(params, what), what, dtype, (n, 256)))
    _need(img_u8, lab_u8)
    dev = first.device
    # one upload: [affine | lines | lut_f32 | lut_u8], every part a multiple of 4 bytes
    blob = torch.from_numpy(np.concatenate([a.reshape(-1).view(np.uint8) for a in parts])).to(dev, non_blocking=True)
    at, ptr = 0, {}
    for a, what in zip(parts, ['affine'] + (['lines'] if nl else []) + (['lut_f32'] if want_f32 else []) + (['lut_u8'] if want_u8 else [])):
        ptr[what] = blob.data_ptr() + at
        at += a.nbytes
    x = torch.empty(n, h, w, dtype=torch.float32, device=dev) if want_f32 else None
    x_u8 = torch.empty(n, h, w, dtype=torch.uint8, device=dev) if want_u8 else None
    y = torch.empty(n, h, w, dtype=torch.uint8, device=dev) if lab_u8 is not None else None
    image = want_f32 or want_u8
    LaunchProfiler.run('augment', 0.0, L.call.s2e_augment_pairs,
                       (_p(img_u8) if image else None, _p(lab_u8), n, h, w, ptr['affine'], ptr.get('lines'), nl, ptr.get('lut_f32'), ptr.get('lut_u8'),
                        _p(x), _p(x_u8), _p(y), _stream()),
                       nbytes=float(n * h * w * ((1 + 4 * want_f32 + want_u8 if image else 0) + 2 * (y is not None))))
    return x, x_u8, y
