"""The segmenter's paired augmentation restated in numpy, for the tests of seg2eye_amd/ops/augment.py,
csrc/seg_augment.hip and seg2eye_amd/seg_augment.py: the warp of a frame and its label map, the line occluders and the tables in int64
arrays (`augment_pairs`), the draw of a batch's parameters (`draw`), a line's cover by exact rational arithmetic (`covered_exact`), and
the data the tests use.  Written from the rule's statement (include/seg2eye_hip.h, ops/augment.py's text), not from the kernel."""
import collections
import fractions
import math

import numpy as np

Params = collections.namedtuple('Params', 'affine lines lut_f32 lut_u8')
COLUMNS = 9 + 6 * 8


# ------------------------------------------------------------------------------------------------ the warp
def source(A, H, W):
    """A: six integers.  -> (sx, sy) int64 (H, W): the clamped Q16 source position of every output pixel."""
    A = [int(v) for v in A]
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    sx = np.clip(A[0] * x + A[1] * y + A[2], 0, (W - 1) << 16)
    sy = np.clip(A[3] * x + A[4] * y + A[5], 0, (H - 1) << 16)
    return sx, sy


def warp_label(lab, A):
    H, W = lab.shape
    sx, sy = source(A, H, W)
    return lab[(sy + 0x8000) >> 16, (sx + 0x8000) >> 16]


def warp_frame(img, A):
    """-> int64 (H, W) in 0..255"""
    H, W = img.shape
    sx, sy = source(A, H, W)
    x0, y0 = sx >> 16, sy >> 16
    fx, fy = (sx & 0xffff) >> 8, (sy & 0xffff) >> 8
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    p = img.astype(np.int64)
    top = p[y0, x0] * (256 - fx) + p[y0, x1] * fx
    bot = p[y1, x0] * (256 - fx) + p[y1, x1] * fx
    return (top * (256 - fy) + bot * fy + 0x8000) >> 16


def line_cover(line, H, W):
    """line: (x0, y0, x1, y1, width, value) integers -> (bool (H, W), value)"""
    x0, y0, x1, y1 = (min(max(int(v), -4096), 8191) for v in line[:4])
    width, value = min(max(int(line[4]), 0), 255), int(line[5]) & 255
    dx, dy = x1 - x0, y1 - y0
    len2 = dx * dx + dy * dy
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    t = (x - x0) * dx + (y - y0) * dy
    c = (x - x0) * dy - (y - y0) * dx
    hit = (t >= 0) & (t <= len2) & (4 * c * c <= width * width * len2)
    return (hit if width >= 1 and len2 > 0 else np.zeros((H, W), dtype=bool)), value


def covered_exact(line, x, y):
    """The same cover for ONE pixel from geometry, in rationals: the foot of the perpendicular from (x, y) lies on the segment and the
    squared distance to the line through the end points is at most (width / 2)^2."""
    x0, y0, x1, y1 = (min(max(int(v), -4096), 8191) for v in line[:4])
    width = min(max(int(line[4]), 0), 255)
    if width < 1 or (x0, y0) == (x1, y1):
        return False
    F = fractions.Fraction
    d = (x1 - x0, y1 - y0)
    len2 = d[0] * d[0] + d[1] * d[1]
    s = F((x - x0) * d[0] + (y - y0) * d[1], len2)               # position of the foot along the segment, 0 .. 1
    foot = (x0 + s * d[0], y0 + s * d[1])
    dist2 = (x - foot[0]) ** 2 + (y - foot[1]) ** 2
    return 0 <= s <= 1 and dist2 <= F(width * width, 4)


def augment_pairs(img, lab, p):
    """img, lab uint8 (n, H, W) or None; p: Params (lines None or (n, L, 6); a table None: its output is None)
    -> (float32 (n, H, W) or None, uint8 or None, uint8 or None)"""
    first = img if img is not None else lab
    n, H, W = first.shape
    xf = np.zeros((n, H, W), dtype=np.float32) if img is not None and p.lut_f32 is not None else None
    xb = np.zeros((n, H, W), dtype=np.uint8) if img is not None and p.lut_u8 is not None else None
    y = np.zeros((n, H, W), dtype=np.uint8) if lab is not None else None
    for m in range(n):
        if y is not None:
            y[m] = warp_label(lab[m], p.affine[m])
        if xf is None and xb is None:
            continue
        v = warp_frame(img[m], p.affine[m])
        for line in ([] if p.lines is None else p.lines[m]):
            hit, value = line_cover(line, H, W)
            v[hit] = value
        if xf is not None:
            xf[m] = np.asarray(p.lut_f32[m])[v]
        if xb is not None:
            xb[m] = np.asarray(p.lut_u8[m])[v]
    return xf, xb, y


# ------------------------------------------------------------------------------------------------ the draw
def identity_luts():
    from seg2eye_amd.ops.preprocess import normalize_lut
    return normalize_lut().numpy(), np.arange(256, dtype=np.uint8)


def luts(gamma, gain, bias):
    if gamma == 1 and gain == 1 and bias == 0:
        return identity_luts()
    c = np.clip(gain * (np.arange(256, dtype=np.float64) / 255.0) ** gamma + bias, 0.0, 1.0)
    return ((c - 0.5) / 0.5).astype(np.float32), np.rint(255.0 * c).astype(np.uint8)


def matrix(theta_deg, scale, tx, ty, h, w):
    theta = theta_deg * (math.pi / 180.0)
    a, b = np.cos(theta) / scale, np.sin(theta) / scale
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    A0, A1 = np.rint(65536 * a), np.rint(65536 * b)
    A3, A4 = -A1, A0
    A2 = np.rint(65536 * cx - (A0 * (cx + tx) + A1 * (cy + ty)))
    A5 = np.rint(65536 * cy - (A3 * (cx + tx) + A4 * (cy + ty)))
    return [int(min(max(v, -2.0 ** 31), 2.0 ** 31 - 1)) for v in (A0, A1, A2, A3, A4, A5)]


def draw(rng, n, h, w, prob=1.0, rotate=0.0, scale=1.0, translate=0.0, gamma=1.0, contrast=0.0, brightness=0.0, lines=0):
    """One rng.rand(n, 57) -> Params, per the table of columns."""
    u = rng.rand(n, COLUMNS)
    affine = np.zeros((n, 6), dtype=np.int32)
    lut_f, lut_b = np.zeros((n, 256), dtype=np.float32), np.zeros((n, 256), dtype=np.uint8)
    occl = np.zeros((n, lines, 6), dtype=np.int32) if lines else None
    for i in range(n):
        r = u[i]
        if not r[0] < prob:
            affine[i] = (65536, 0, 0, 0, 65536, 0)
            lut_f[i], lut_b[i] = identity_luts()
            continue
        s = 2.0 * r - 1.0
        affine[i] = matrix(s[1] * rotate, np.exp(s[2] * math.log(scale)), s[3] * translate * w, s[4] * translate * h, h, w)
        lut_f[i], lut_b[i] = luts(np.exp(s[5] * math.log(gamma)), 1.0 + s[6] * contrast, s[7] * brightness)
        for j in range(min(int(math.floor(r[8] * (lines + 1))), lines)):
            c = r[9 + 6 * j:15 + 6 * j]
            occl[i, j] = (math.floor(c[0] * w), math.floor(c[1] * h), math.floor(c[2] * w), math.floor(c[3] * h), 1 + math.floor(3 * c[4]),
                          min(math.floor(256 * c[5]), 255))
    return Params(affine, occl, lut_f, lut_b)


def identity(n, lines=0):
    f, b = identity_luts()
    return Params(np.tile(np.array([65536, 0, 0, 0, 65536, 0], dtype=np.int32), (n, 1)), np.zeros((n, lines, 6), dtype=np.int32) if lines else None,
                  np.tile(f, (n, 1)), np.tile(b, (n, 1)))


# ------------------------------------------------------------------------------------------------ the data
def planes(shape, seed):
    """-> (frames, labels) uint8 of `shape` = (n, H, W): iid bytes, and iid classes 0..3 with a sprinkle of other bytes (a label map is
    copied, whatever it holds)."""
    rng = np.random.RandomState(seed)
    img = rng.randint(0, 256, shape).astype(np.uint8)
    lab = rng.randint(0, 4, shape).astype(np.uint8)
    odd = rng.rand(*shape) < 0.05
    lab[odd] = rng.randint(4, 256, shape).astype(np.uint8)[odd]
    return img, lab


def label_grey(labels, ncls=4):
    return np.minimum(labels.astype(np.int64) * 256 // (ncls - 1), 255).astype(np.uint8)
