#!/usr/bin/env python3
"""Writes tests/golden/pil_bicubic.npz: what Pillow's `Image.resize(..., BICUBIC)` gives for the cases of
tests/test_preprocess_{host,gpu}.py, so that those tests depend on neither Pillow's presence nor its version.

    python tests/golden/make_pil_bicubic.py

Only the EXPECTED uint8 outputs are stored, one frame per (case, input kind); the inputs are regenerated in the tests from
`np.random.RandomState(seed)` (`case_input` below -- the tests carry a copy), whose legacy stream is stable across numpy versions.
To keep the file small only every `row_step`-th row of the larger outputs is stored (640 x 384: every 8th); the tests hold the
numpy restatement of the rule against these rows, and against live Pillow in full wherever it imports."""
import os

import numpy as np
import PIL
from PIL import Image

# (H, W) -> (Ho, Wo)
CASES = [((640, 400), (80, 64)), ((640, 400), (320, 256)), ((640, 400), (256, 256)), ((640, 400), (640, 384)),
         ((640, 400), (640, 400)), ((37, 23), (64, 48))]
KINDS = ('uniform', 'binary')
ROW_STEP = {'uniform': {(320, 256): 2, (640, 384): 8, (640, 400): 32},
            'binary': {(320, 256): 4, (256, 256): 4, (640, 384): 16, (640, 400): 32}}


def row_step(dst, kind):
    return ROW_STEP[kind].get(dst, 1)


def case_name(src, dst, kind):
    return '%dx%d_to_%dx%d_%s' % (src + dst + (kind,))


def case_input(ci, src, kind):
    """The one stored frame of case number ci: frame 0 of the test's (3, H, W) batch."""
    rng = np.random.RandomState(1000 + 10 * ci + KINDS.index(kind))
    frames = rng.randint(0, 256, (3,) + src) if kind == 'uniform' else rng.randint(0, 2, (3,) + src) * 255
    return frames.astype(np.uint8)


def main():
    out = {'pillow_version': np.array(PIL.__version__)}
    for ci, (src, dst) in enumerate(CASES):
        for kind in KINDS:
            img = case_input(ci, src, kind)[0]
            r = np.asarray(Image.fromarray(img, mode='L').resize((dst[1], dst[0]), Image.BICUBIC), dtype=np.uint8)
            out[case_name(src, dst, kind)] = np.ascontiguousarray(r[::row_step(dst, kind)])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'pil_bicubic.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes; Pillow', PIL.__version__)


if __name__ == '__main__':
    main()
