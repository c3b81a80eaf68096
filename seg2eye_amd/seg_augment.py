"""The eye segmenter trained on augmented data: every step warps the batch's resized frames and label maps together by a
small rotation, scaling and shift, changes the frames' gamma, contrast and brightness and draws dark or bright line occluders (lashes,
the rims of glasses) across them -- `ops.augment_pairs`, one HIP launch, with the parameters `ops.AugmentRule` draws.

    python -m seg2eye_amd.seg_augment train --dataroot openeds.h5 --name seg --aug_rotate 10 --aug_scale 1.1 --aug_translate 0.05 \\
                                            --aug_gamma 1.5 --aug_contrast 0.2 --aug_brightness 0.1 --aug_lines 3
    python -m seg2eye_amd.seg_augment show  --dataroot openeds.h5 --out aug_preview --n 8 --aug_rotate 10 --aug_lines 3

`train` takes every flag of `segment train` and writes the same `*_net_S.pth` files: `segment eval` and `segment predict` read them.
Every --aug_* flag defaults to "off"; with all of them off the rule is the identity (the draws are still made).  `show` writes, per
sample, one PNG [frame | label | augmented frame | augmented label] at --seg_hw: what a setting does, before a training run is spent on it."""
import argparse
import os

import numpy as np

from . import segment, stage
from .openeds_store import open_tree

AUG_FLAGS = [('--aug_prob', dict(type=float, default=1.0, help='share of the frames that are augmented at all')),
             ('--aug_rotate', dict(type=float, default=0.0, help='largest rotation about the centre, in degrees (0: off)')),
             ('--aug_scale', dict(type=float, default=1.0, help='largest scaling factor: drawn log-uniformly in [1/v, v] (1: off)')),
             ('--aug_translate', dict(type=float, default=0.0, help='largest shift, as a share of the width and of the height (0: off)')),
             ('--aug_gamma', dict(type=float, default=1.0, help='largest gamma: drawn log-uniformly in [1/v, v] (1: off)')),
             ('--aug_contrast', dict(type=float, default=0.0, help='the gain is drawn in [1 - v, 1 + v], v < 1 (0: off)')),
             ('--aug_brightness', dict(type=float, default=0.0, help='the bias is drawn in [-v, v] of the grey range (0: off)')),
             ('--aug_lines', dict(type=int, default=0, help='at most this many line occluders per frame, 0 to 8 (0: off)'))]
AUG_KEYS = tuple(flag[2:] for flag, _ in AUG_FLAGS)


def rule_of(a):
    """The `ops.AugmentRule` of parsed arguments (a dict); the --aug_* keys are taken out of it."""
    from .ops.augment import AugmentRule
    return AugmentRule(**{k[4:]: a.pop(k) for k in AUG_KEYS})


def label_grey(labels, ncls):
    """Label maps as the visualiser shows them -- label / max * 2 - 1 stored as trunc((v + 1) * 128), saturating --, with the largest
    class in max's place: min(256 l // (ncls - 1), 255)."""
    return np.minimum(labels.astype(np.int64) * 256 // max(int(ncls) - 1, 1), 255).astype(np.uint8)


def show(store, rule, out_dir, n=8, seed=0, seg_hw=(320, 200), label_nc=4, dataset_key='train', device='cuda'):
    """One PNG per sample of the first n labelled frames of a split -> the written paths.  One draw of the rule from RandomState(seed)."""
    from .ops import augment as A, preprocess as P
    from .visualizer import write_png
    batch = segment.labelled_samples(store, dataset_key)[:int(n)]
    if not batch:
        raise ValueError("show: /%s has no labelled frames (images_ss / labels_ss)" % dataset_key)
    h, w = seg_hw
    frames, labels = stage.to_device(device, segment._labelled_rows(store, dataset_key, 'images_ss', batch), segment._labelled_rows(store, dataset_key, 'labels_ss', batch))
    flip = segment._no_flip(len(batch), device)
    x_u8 = P.resize_bicubic_u8(frames, h, w, flip, return_u8=True)[1]
    y = P.resize_nearest_u8(labels, h, w, flip)
    params = rule.draw(np.random.RandomState(int(seed)), len(batch), h, w)
    _, ax, ay = A.augment_pairs(x_u8, y, params, want_f32=False, want_u8=True)
    x_u8, y, ax, ay = (t.cpu().numpy() for t in (x_u8, y, ax, ay))
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for i, (user, row) in enumerate(batch):
        paths.append(os.path.join(out_dir, '%s_%03d.png' % (user, row)))
        write_png(paths[-1], np.concatenate([x_u8[i], label_grey(y[i], label_nc), ax[i], label_grey(ay[i], label_nc)], axis=1))
    return paths


def parser():
    ap = argparse.ArgumentParser(prog='python -m seg2eye_amd.seg_augment', description='Train the eye segmenter on augmented data, or look at what a setting does.')
    sub = ap.add_subparsers(dest='command', required=True)
    t = sub.add_parser('train', help='segment train, every step on augmented frames and labels')
    stage.add_common_flags(t, segment.DEFAULTS['name'], segment.DEFAULTS['batchSize'], net=segment.NET_FLAGS)
    stage.add_train_flags(t, segment.FLIP_WHAT, segment.TRAIN_FLAGS, segment.TRAIN_LAST_FLAGS)
    stage.add_flags(t, AUG_FLAGS)
    s = sub.add_parser('show', help='write [frame | label | augmented frame | augmented label] PNGs of a few samples')
    s.add_argument('--dataroot', required=True, help='the store prepare_openeds wrote (.h5, or .npz without h5py)')
    s.add_argument('--out', required=True, help='the directory the PNGs go to')
    s.add_argument('--n', type=int, default=8, help='samples: the first n labelled frames of the split')
    s.add_argument('--seed', type=int, default=0)
    s.add_argument('--dataset_key', default='train', choices=['train', 'validation', 'test'])
    stage.add_flags(s, [segment.NET_FLAGS[1]])               # --seg_hw
    s.add_argument('--label_nc', type=int, default=4)
    stage.add_flags(s, AUG_FLAGS)
    return ap


def main(argv=None):
    a = vars(parser().parse_args(argv))
    command, dataroot = a.pop('command'), a.pop('dataroot')
    rule = rule_of(a)
    store = open_tree(dataroot)
    if command == 'train':
        segment.train_segmenter(store, segment.seg_options(**a), augment=rule)
        return None
    paths = show(store, rule, a['out'], a['n'], a['seed'], tuple(int(v) for v in a['seg_hw']), a['label_nc'], a['dataset_key'])
    print('%d panels written to %s (%s)' % (len(paths), a['out'], rule))
    return paths


if __name__ == '__main__':
    main()
