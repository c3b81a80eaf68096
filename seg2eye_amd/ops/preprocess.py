"""Device-side preprocessing of OpenEDS batches (--device_preprocess): what `OpenEDSDataset.__getitem__` does on the
host -- PIL's bicubic resize of five 640 x 400 frames per sample, ToTensor + Normalize, cv2's nearest resize of the label map, the
horizontal flip -- as two HIP launches per batch (csrc/preprocess.hip), bit-identical to the host path.

The rule is Pillow's `ImagingResample` for 8-bit images (src/libImaging/Resample.c), integer arithmetic throughout:

  per axis (in -> out), in double precision:
    scale = in / out, fscale = max(scale, 1), support = 2.0 * fscale (bicubic), ksize = 2 * ceil(support) + 1
    output index i: center = (i + 0.5) * scale
                    xmin = max(int(center - support + 0.5), 0),  xmax = min(int(center + support + 0.5), in) - xmin
                    taps w_x = bicubic((x + xmin - center + 0.5) * (1 / fscale)), a = -0.5, normalised by their sum,
                    then fixed point: int(+-0.5 + w * 2^22), truncating toward zero
  a pass:  clamp((2^21 + sum_x pixel * k_x) >> 22, 0, 255) in 32-bit integers, stored as uint8
  the horizontal pass first, the vertical pass on its uint8 result; a pass whose size does not change is SKIPPED
  flip: of the result (flip(img.resize(...)));  float value: lut[r], lut = ((u8 / 255) - 0.5) / 0.5 computed by torch on the host

`resize_bicubic_u8_reference` applies the same tables with integer numpy: it documents the rule and is what the CPU tests hold
against Pillow.  It is NOT a fallback: the ops below raise on CPU tensors like every other op."""
import math

import numpy as np
import torch

from .. import _lib as L
from .core import _need, _p, _stream

PRECISION_BITS = 22        # 32 - 8 - 2 (Resample.c)
RAW_KEYS = ('label_raw', 'style_raw', 'target_raw')


# ------------------------------------------------------------------------------ the rule (host, numpy float64 / integers)
def _bicubic(t):
    a = -0.5
    t = np.abs(t)
    return np.where(t < 1.0, ((a + 2.0) * t - (a + 3.0)) * t * t + 1, np.where(t < 2.0, (((t - 5) * t + 8) * t - 4) * a, 0.0))


def bicubic_ksize(in_size, out_size):
    return 2 * int(math.ceil(2.0 * max(in_size / out_size, 1.0))) + 1


def bicubic_coeffs(in_size, out_size):
    """-> (int32 [out, ksize] fixed-point taps, int32 [out, 2] bounds (xmin, count)); taps past `count` are zero."""
    scale = in_size / out_size
    fscale = max(scale, 1.0)
    support = 2.0 * fscale
    ksize = bicubic_ksize(in_size, out_size)
    ss = 1.0 / fscale
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    for i in range(out_size):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = _bicubic((np.arange(xmax, dtype=np.float64) + xmin - center + 0.5) * ss)
        ww = 0.0
        for v in w:                                          # (the sum in Pillow's order: left to right)
            ww += v
        if ww != 0.0:
            w = w / ww
        fixed = np.where(w < 0, -0.5 + w * (1 << PRECISION_BITS), 0.5 + w * (1 << PRECISION_BITS))
        kk[i, :xmax] = np.trunc(fixed).astype(np.int32)
        bounds[i] = (xmin, xmax)
    return kk, bounds


def _pass_rows(img, kk, bounds):
    """One pass along the LAST axis of a uint8 array."""
    out = np.empty(img.shape[:-1] + (kk.shape[0],), dtype=np.uint8)
    src = img.astype(np.int32)
    for i in range(kk.shape[0]):
        xmin, n = int(bounds[i, 0]), int(bounds[i, 1])
        acc = (src[..., xmin:xmin + n] * kk[i, :n]).sum(axis=-1, dtype=np.int32) + np.int32(1 << (PRECISION_BITS - 1))
        out[..., i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize_bicubic_u8_reference(img, Wo, Ho):
    """Image.fromarray(img, 'L').resize((Wo, Ho), Image.BICUBIC) as a uint8 array, for a 2-D uint8 array (H, W)."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    H, W = img.shape
    if W != Wo:
        img = _pass_rows(img, *bicubic_coeffs(W, Wo))
    if H != Ho:
        img = np.ascontiguousarray(_pass_rows(np.ascontiguousarray(img.T), *bicubic_coeffs(H, Ho)).T)
    return img


def nearest_index(in_size, out_size):
    """cv2.INTER_NEAREST's source index per output index, as openeds_dataset.resize_nearest computes it."""
    return np.minimum((np.arange(out_size) * (in_size / out_size)).astype(np.int64), in_size - 1).astype(np.int32)


def normalize_lut():
    """fp32 [256]: the very expression of openeds_dataset.get_transform's tf_image, for every uint8 value."""
    u8 = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    return (u8.float().div(255.0) - 0.5) / 0.5


# ------------------------------------------------------------------------------ device tables, cached per (in, out, device)
_TABLES = {}


def _cached(key, make):
    v = _TABLES.get(key)
    if v is None:
        v = _TABLES[key] = make()
    return v


def _bicubic_tables(in_size, out_size, dev):
    """(taps, bounds) on the device; (None, None) when the size does not change (the pass is skipped)."""
    if in_size == out_size:
        return None, None
    return _cached(('bicubic', in_size, out_size, str(dev)),
                   lambda: tuple(torch.from_numpy(a).to(dev) for a in bicubic_coeffs(in_size, out_size)))


def _nearest_table(in_size, out_size, dev):
    return _cached(('nearest', in_size, out_size, str(dev)), lambda: torch.from_numpy(nearest_index(in_size, out_size)).to(dev))


def _lut(dev):
    return _cached(('lut', str(dev)), lambda: normalize_lut().to(dev))


def _frames(frames_u8, flip):
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 3:
        raise L.Seg2EyeHipError('expected uint8 frames (M, H, W), got %s %s' % (frames_u8.dtype, tuple(frames_u8.shape)))
    _need(frames_u8, flip)
    if flip.dtype == torch.bool:
        flip = flip.view(torch.uint8)
    if flip.dtype != torch.uint8 or flip.numel() != frames_u8.shape[0]:
        raise L.Seg2EyeHipError('expected one flip byte per frame')
    return flip


# ------------------------------------------------------------------------------ the two ops (no autograd: the inputs are data)
def resize_bicubic_u8(frames_u8, Ho, Wo, flip, return_u8=False):
    """frames (M, H, W) uint8, flip (M,) bool / uint8 -> fp32 (M, Ho, Wo) in [-1, 1] (and the resized uint8 frames)."""
    flip = _frames(frames_u8, flip)
    M, H, W = frames_u8.shape
    dev = frames_u8.device
    kx, bx = _bicubic_tables(W, Wo, dev)
    ky, by = _bicubic_tables(H, Ho, dev)
    out = torch.empty(M, Ho, Wo, dtype=torch.float32, device=dev)
    out_u8 = torch.empty(M, Ho, Wo, dtype=torch.uint8, device=dev) if return_u8 else None
    L.call.s2e_resize_bicubic_u8(_p(frames_u8), _p(flip), M, H, W, Ho, Wo, _p(kx), _p(bx), _p(ky), _p(by), _p(_lut(dev)),
                                 _p(out), _p(out_u8), _stream())
    return (out, out_u8) if return_u8 else out


def resize_nearest_u8(frames_u8, Ho, Wo, flip):
    """label maps (M, H, W) uint8 -> (M, Ho, Wo) uint8 by cv2's nearest rule, flipped per frame."""
    flip = _frames(frames_u8, flip)
    M, H, W = frames_u8.shape
    dev = frames_u8.device
    out = torch.empty(M, Ho, Wo, dtype=torch.uint8, device=dev)
    L.call.s2e_resize_nearest_u8(_p(frames_u8), _p(flip), M, H, W, Ho, Wo, _p(_nearest_table(H, Ho, dev)),
                                 _p(_nearest_table(W, Wo, dev)), _p(out), _stream())
    return out


# ------------------------------------------------------------------------------ raw batch -> the standard batch contract
def fixed_hw(opt):
    """(H, W) that preprocess_mode 'fixed' resizes to -- openeds_dataset.get_transform's own expression, so that the device path
    yields what the host path yields for every option set (it equals options.image_hw(opt) wherever the generator accepts the
    size; e.g. at crop_size 64, aspect_ratio 0.8 the dataset gives 80 x 64 and the two differ)."""
    return round(opt.crop_size / opt.aspect_ratio), opt.crop_size


def materialize(data, opt, device):
    """A raw batch of OpenEDSDataset (--device_preprocess: `label_raw` (N, 640, 400), `style_raw` (N, ns, 640, 400), `target_raw`
    (N, 640, 400; absent on the test split) uint8 and `flip` (N,) bool) -> the standard contract on `device`: `label` (N, H, W)
    uint8, `style_image` (N, ns, 1, H, W) fp32, `target` (N, 1, H, W) fp32; every other key unchanged.  Idempotent: a batch
    without raw keys comes back untouched.  Two launches: target + style images in one, the labels in the other."""
    if 'label_raw' not in data:
        return data
    device = torch.device(device)
    if device.type != 'cuda':
        raise L.Seg2EyeHipError('materialize runs on the GPU only (got device %s); there is no CPU fallback' % device)
    Ho, Wo = fixed_hw(opt)
    label_raw, style_raw, target_raw = data['label_raw'], data['style_raw'], data.get('target_raw')
    n, ns, H, W = style_raw.shape
    flip = torch.as_tensor(data['flip']).reshape(n).to(torch.bool)
    # frame order: the N targets, then the N * ns style images -- both host tensors land in ONE device buffer as contiguous slices
    nt = n if target_raw is not None else 0
    frames = torch.empty(nt + n * ns, H, W, dtype=torch.uint8, device=device)
    if nt:
        frames[:nt].copy_(target_raw.reshape(n, H, W), non_blocking=True)
    frames[nt:].copy_(style_raw.reshape(n * ns, H, W), non_blocking=True)
    labels = label_raw.reshape(n, H, W).to(device, non_blocking=True)
    # one flip byte per frame of each launch, in one small copy: [labels | targets | style images]
    flips = torch.cat([flip, flip[:nt], flip.repeat_interleave(ns)]).view(torch.uint8).to(device, non_blocking=True)
    images = resize_bicubic_u8(frames, Ho, Wo, flips[n:])
    out = {k: v for k, v in data.items() if k not in RAW_KEYS}
    out['label'] = resize_nearest_u8(labels, Ho, Wo, flips[:n])
    out['style_image'] = images[nt:].view(n, ns, 1, Ho, Wo)
    if nt:
        out['target'] = images[:nt].view(n, 1, Ho, Wo)
    return out
