"""The visualiser with the reference's interface (util/visualizer.py:27-166): `loss_log.txt`, and the side-by-side validation panels
-- style images | label map | ground truth | generated image | error heat map -- that every Tester draws per sample.

What differs from the reference: the five cells of a panel are resized, normalised and turned into bytes on the GPU by three HIP
launches per batch (ops.sidebyside_u8; the reference moves five tensors to the host and runs cv2 / torchvision there), a
panel is the uint8 array the reference's error log stores ((v + 1) * 128), and `display_current_results` writes PNG files under
`<checkpoints_dir>/<name>/visuals/` (the reference sends JPEGs to TensorBoard: `--tf_log` stays inert here, as does `--no_html`)."""
import os
import struct
import time
import zlib
from collections import OrderedDict

import numpy as np
import torch

from . import ops

CAPTION_ROWS = 60


def caption_strip(text, width, rows=CAPTION_ROWS):
    """uint8 (rows, width): `text` in white (255) on black (0).  PARITY-UNPINNED: the reference draws it with cv2's Hershey font
    (util/image_annotate.py), which is not restated here; this strip is drawn with Pillow's built-in bitmap font when Pillow imports
    and stays black otherwise.  (The reference also sends its strip through normalize and (v + 1) * 128; here it stays 0 / 255.)"""
    strip = np.zeros((rows, width), dtype=np.uint8)
    try:
        from PIL import Image, ImageDraw, ImageFont
    except ImportError:
        return strip
    img = Image.fromarray(strip, mode='L')
    ImageDraw.Draw(img).text((10, max(0, rows // 2 - 6)), text, fill=255, font=ImageFont.load_default())
    return np.where(np.asarray(img) >= 128, 255, 0).astype(np.uint8)


def visualize_sidebyside(data, limit=-1, key_fake='fake', key_content='label', key_target='target_original', key_style='style_image',
                         log_key='', w=200, h=320, error_list=None):
    """util/visualizer.py:131-166 -> OrderedDict '<log_key>/<i>' -> uint8 (1, h + 60, 5 w): per sample the five cells
    [ style | content | target | fake | heat ] over a 60-row caption '<user> / <filename> (err: <err * 1471>)'.  `limit` > 0 keeps the
    first `limit` entries of every key.  The cells come from the GPU in ONE device-to-host copy per batch; the host only captions.
    ValueError where the reference raises its range error (a NaN, or a tensor outside [-1, 1] that also holds negative values).
    The caption is parity-unpinned (`caption_strip`); the cells follow the reference's rule bit for bit (tests/_sidebyside_rule.py)."""
    if limit > 0:
        data = {k: v[:limit] for k, v in data.items()}
    dev = data[key_fake].device
    on_dev = [torch.as_tensor(data[k]).to(dev, non_blocking=True) for k in (key_content, key_target, key_style)]
    panels = ops.sidebyside_u8_host(on_dev[0], data[key_fake], on_dev[1], on_dev[2], w=w, h=h, caption_rows=CAPTION_ROWS)
    visuals = OrderedDict()
    for i in range(panels.shape[0]):
        text = '%s / %s' % (data['user'][i], data['filename'][i])
        if error_list is not None:
            text += ' (err: %.2f)' % (float(error_list[i]) * 1471)
        panels[i, 0, h:] = caption_strip(text, panels.shape[-1])
        visuals['%s/%d' % (log_key, i)] = panels[i]
    return visuals


def png_bytes(img):
    """An 8-bit greyscale PNG of a 2-D uint8 array: signature, IHDR, one IDAT (filter 0 on every row), IEND."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if img.ndim != 2:
        raise ValueError('a 2-D uint8 array is expected, got shape %s' % (img.shape,))
    rows, cols = img.shape

    def chunk(tag, body):
        return struct.pack('>I', len(body)) + tag + body + struct.pack('>I', zlib.crc32(tag + body) & 0xffffffff)
    raw = np.concatenate([np.zeros((rows, 1), dtype=np.uint8), img], axis=1).tobytes()
    return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', cols, rows, 8, 0, 0, 0, 0))
            + chunk(b'IDAT', zlib.compress(raw, 6)) + chunk(b'IEND', b''))


def write_png(path, img):
    tmp = path + '.part'
    with open(tmp, 'wb') as f:
        f.write(png_bytes(img))
    os.replace(tmp, path)                                    # (a reader never sees half a file)


class Visualizer:
    def __init__(self, opt):
        self.opt = opt
        self.name = opt.name
        self.run_dir = os.path.join(opt.checkpoints_dir, opt.name)
        self.log_name = None
        if opt.isTrain:
            os.makedirs(self.run_dir, exist_ok=True)
            self.log_name = os.path.join(self.run_dir, 'loss_log.txt')
            with open(self.log_name, 'a') as log_file:
                log_file.write('================ Training Loss (%s) ================\n' % time.strftime('%c'))

    def display_current_results(self, visuals, epoch, step):
        """One PNG per entry: <run>/visuals/step<%09d>/<key with '/' -> '_'>.png.  -> the written paths."""
        out_dir = os.path.join(self.run_dir, 'visuals', 'step%09d' % int(step))
        os.makedirs(out_dir, exist_ok=True)
        paths = []
        for key, img in visuals.items():
            img = np.asarray(img)
            paths.append(os.path.join(out_dir, key.strip('/').replace('/', '_') + '.png'))
            write_png(paths[-1], img.reshape(img.shape[-2:]))
        return paths

    def plot_current_errors(self, errors, step):
        """(TensorBoard scalars in the reference; kept for the interface.)"""

    def print_current_errors(self, epoch, i, errors, t):
        """visualizer.py:85-95: the line, printed and appended to loss_log.txt."""
        message = '(epoch: %d, iters: %d, time: %.3f) ' % (epoch, i, t)
        for k, v in errors.items():
            message += '%s: %.3f ' % (k, float(torch.as_tensor(v).float().mean()))
        print(message, flush=True)
        if self.log_name:
            with open(self.log_name, 'a') as log_file:
                log_file.write('%s\n' % message)
