"""Side-by-side validation panels on the GPU (csrc/visual.hip): the reference's `visualize_sidebyside`
(util/visualizer.py:131-166) for a whole batch as three HIP launches -- [ style | label | target_original | fake | heat ], five
h x w cells of uint8 per sample -- instead of five tensors leaving the device, five cv2.resize calls, the host min / max passes of
`ImageProcessor.normalize` and a torchvision `make_grid` per sample.  The rule is stated in csrc/visual.hip and include/seg2eye_hip.h
and restated on the CPU, operation by operation, by tests/_sidebyside_rule.py (the yardstick of the GPU tests; nothing here imports
it).  There is no CPU path: the ops raise on CPU tensors like every other op."""
import torch

from .. import _lib as L
from .core import _dt, _need, _p, _stream

SIDEBYSIDE_STATUS_NAMES = ('style_image', 'label', 'target_original', 'fake')      # bit i of the status word the launches write


def _sidebyside_planes(t, what):
    """(n, 1, H, W) or (n, H, W) -> contiguous (n, H, W)."""
    if t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 3:
        raise ValueError('%s: expected (n, 1, H, W) or (n, H, W), got %s' % (what, tuple(t.shape)))
    return t.contiguous()


def _sidebyside_launch(label, fake, target_original, style_image, w, h, caption_rows):
    """-> (flat uint8 device buffer, panels view (n, 1, h + caption_rows, 5 w) of it, its last 4 bytes = the status word).  No
    host synchronisation: panels and status live in ONE buffer so that one copy brings both to the host."""
    for t in (label, fake, target_original, style_image):
        if not t.is_cuda:
            raise L.Seg2EyeHipError('seg2eye_amd ops run on the GPU only (got a %s tensor); there is no CPU fallback' % t.device)
    if style_image.dim() != 5 or style_image.shape[2] != 1:
        raise ValueError('style_image: expected (n, ns, 1, H, W), got %s' % (tuple(style_image.shape),))
    if w <= 0 or h <= 0 or caption_rows < 0:
        raise ValueError('w and h must be positive and caption_rows not negative')
    fake = _sidebyside_planes(fake.detach(), 'fake')
    if fake.dtype not in (torch.float32, torch.bfloat16):
        fake = fake.float()
    label = _sidebyside_planes(label, 'label').to(torch.uint8)
    target = _sidebyside_planes(target_original, 'target_original').to(torch.uint8)
    style = style_image.detach()[:, :, 0].float().contiguous()
    n, H, W = fake.shape
    ns = style.shape[1]
    if label.shape != fake.shape or style.shape != (n, ns, H, W) or target.shape[0] != n or ns < 1:
        raise ValueError('shapes disagree: label %s, fake %s, style_image %s, target_original %s'
                         % (tuple(label.shape), tuple(fake.shape), tuple(style_image.shape), tuple(target_original.shape)))
    _need(label, fake, target, style)
    Ht, Wt = target.shape[1:]
    dev = fake.device
    rows, pw = h + caption_rows, 5 * w
    body = n * rows * pw
    flat = torch.empty((body + 3) // 4 * 4 + 4, dtype=torch.uint8, device=dev)
    panels = flat[:body].view(n, 1, rows, pw)
    if caption_rows:
        panels[:, :, h:].zero_()
    ws = torch.empty(L.call.s2e_sidebyside_ws_bytes(n, h, w), dtype=torch.uint8, device=dev)
    L.call.s2e_sidebyside_u8(_dt(fake), _p(fake), _p(style), ns, _p(label), _p(target), n, H, W, Ht, Wt, h, w, pw, rows * pw,
                             _p(ws), flat.data_ptr() + flat.numel() - 4, _p(flat), _stream())
    return flat, panels, flat[-4:]


def sidebyside_check_status(status):
    """The status word (an int) -> ValueError naming every tensor that holds a NaN or fails `ImageProcessor.normalize`'s range check
    (postprocessor.py:75-88: inside [-1 - 1e-6, 1 + 1e-6], or non-negative), where the reference raises its range error."""
    bad = [name for i, name in enumerate(SIDEBYSIDE_STATUS_NAMES) if (status >> i) & 1]
    if bad:
        raise ValueError('Invalid ranges for image: %s (a NaN, or values outside [-1, 1] together with negative ones)' % ', '.join(bad))


def sidebyside_u8(label, fake, target_original, style_image, w=200, h=320, caption_rows=60):
    """label (n,1,H,W) classes 0..3, fake (n,1,H,W) bf16 / fp32 in [-1,1], target_original (n,1,Ht,Wt) 0..255, style_image
    (n,ns,1,H,W) in [-1,1] -> uint8 (n, 1, h + caption_rows, 5 w) on the device: the five cells in rows 0..h-1, the caption rows
    zeroed.  ValueError (after reading the status word: 4 bytes) where the reference raises its range error."""
    _, panels, status = _sidebyside_launch(label, fake, target_original, style_image, w, h, caption_rows)
    sidebyside_check_status(int(status.view(torch.int32).item()))
    return panels


def sidebyside_u8_host(label, fake, target_original, style_image, w=200, h=320, caption_rows=60):
    """The same as a numpy array on the host: panels and status word arrive in one device-to-host copy."""
    flat, panels, _ = _sidebyside_launch(label, fake, target_original, style_image, w, h, caption_rows)
    host = flat.cpu().numpy()
    sidebyside_check_status(int(host[-4:].view('int32')[0]))
    return host[:panels.numel()].reshape(tuple(panels.shape))
