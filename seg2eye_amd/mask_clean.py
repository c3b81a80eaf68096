"""The mask cleaner: the step between `segment predict` and everything that reads its masks, in the chain
prepare_openeds -> segment -> mask_clean -> style_rank -> train -> test (and -> refine).

An eye has one pupil, one iris and one sclera region; a per-pixel argmax gives that plus specks on eyelashes, glints and skin folds, and
pin-holes inside the regions.  Every speck counts in style_rank's mask distance and is painted into the refiner's input.  The rule
(include/seg2eye_hip.h): per class keep all components, the largest one, or those that touch the frame; every other pixel takes the
class of the nearest kept pixel, a tie to the lower class.  By default the skin (class 0) keeps what touches the frame and every other
class its largest component.

    python -m seg2eye_amd.mask_clean apply --seg_file masks.h5 --out masks_clean.h5
    python -m seg2eye_amd.mask_clean eval  --dataroot openeds.h5 --name seg --dataset_key validation

`apply` writes the masks in the layout it read them in, so its output is a drop-in --seg_file.  `eval` scores a segmenter's masks of the
labelled frames before and after cleaning.  Both are plain functions too: `clean_store`, `evaluate`; a `MaskRule` is also what
`segment.predict_masks(..., clean=rule)` takes.  The ops are looked up when called."""
import argparse

import numpy as np
import torch

from . import stage
from .openeds_store import merge_splits, open_tree, rows_u8

MODE_NAMES = ('all', 'largest', 'border')


class MaskRule:
    """What is kept and how pixels join: ncls classes, 4- or 8-connectivity, one mode per class (None: ops.default_modes(ncls))."""

    def __init__(self, ncls=4, conn=8, modes=None):
        self.ncls, self.conn = int(ncls), int(conn)
        self.modes = None if modes is None else tuple(modes)

    def apply(self, masks, return_stats=False):
        """masks (n, H, W) uint8 on the device -> the cleaned masks (and the op's stats)."""
        from .ops import mask_clean as M
        return M.mask_clean(masks, self.ncls, self.conn, self.modes, return_stats)

    __call__ = apply

    def __repr__(self):
        return 'MaskRule(ncls=%d, conn=%d, modes=%s)' % (self.ncls, self.conn, self.modes)


def _is_masks(name):
    return name.startswith('labels_pred_')


# ------------------------------------------------------------------------------------------------ apply
def clean_store(seg_tree, rule, device='cuda', batch=64, verbose=True):
    """seg_tree {split: {user: {labels_pred_*: uint8 (n, H, W)}}} (a mapping or an open file) -> the same tree with every labels_pred_*
    array cleaned by `rule`, in batches of `batch` masks; any other array of a person is passed through.  One line per split: persons,
    masks, the share of pixels that were given another component's class, and the components found beyond one per class, per mask."""
    out = {}
    for split in seg_tree.keys():
        out[split] = {}
        masks = pixels = 0
        filled = extra = None
        for user in seg_tree[split].keys():
            g = seg_tree[split][user]
            out[split][user] = {}
            for name in g.keys():
                if not _is_masks(name):
                    out[split][user][name] = np.asarray(g[name])
                    continue
                n = g[name].shape[0]
                cleaned = np.zeros(tuple(g[name].shape), dtype=np.uint8)
                for r0 in range(0, n, int(batch)):
                    rows = rows_u8((g[name], r) for r in range(r0, min(r0 + int(batch), n)))
                    res, stats = rule.apply(stage.to_device(device, rows)[0], return_stats=True)
                    cleaned[r0:r0 + len(rows)] = res.cpu().numpy()
                    s = stats.to(torch.int64)
                    f = (s[..., 3] - s[..., 1] + s[..., 2]).sum()                      # after - (before - removed): filled in
                    e = (s[..., 0] - 1).clamp(min=0).sum()
                    filled, extra = (f, e) if filled is None else (filled + f, extra + e)
                    masks += len(rows)
                    pixels += rows.size
                out[split][user][name] = cleaned
        if verbose:
            print('%s: %d persons, %d masks, %.4f%% of the pixels changed, %.2f components beyond one per class and mask'
                  % (split, len(out[split]), masks, 100.0 * int(filled if masks else 0) / max(pixels, 1), int(extra if masks else 0) / max(masks, 1)))
    return out


# ------------------------------------------------------------------------------------------------ eval
def evaluate(net, store, dataset_key, opt, rule, device='cuda', verbose=True):
    """mIoU, per-class IoU and pixel accuracy of `net` on the labelled frames of a split, for its masks as they are and as `rule` cleans
    them -> {'miou/<key>', 'iou/<key>/<c>', 'acc/<key>', 'miou_clean/<key>', 'iou_clean/<key>/<c>', 'acc_clean/<key>'}."""
    from . import segment
    from .ops import segment as S
    ncls = int(opt.label_nc)
    conf = [torch.zeros(ncls, ncls, dtype=torch.int64, device=device) for _ in range(2)]
    samples = segment.labelled_samples(store, dataset_key)
    if not samples:
        raise ValueError("evaluate('%s'): the split has no labelled frames (images_ss / labels_ss)" % dataset_key)
    with torch.no_grad():
        for b0 in range(0, len(samples), int(opt.batchSize)):
            batch = samples[b0:b0 + int(opt.batchSize)]
            truth = segment._labelled_rows(store, dataset_key, 'labels_ss', batch)
            frames = segment._labelled_rows(store, dataset_key, 'images_ss', batch)
            logits = net(segment._frames_to_input(frames, opt.seg_hw, segment._no_flip(len(batch), device), device))
            pred = S.seg_argmax_u8(logits, truth.shape[1], truth.shape[2])
            t = torch.from_numpy(truth).to(device)
            S.seg_confusion(pred, t, ncls, out=conf[0])
            S.seg_confusion(rule.apply(pred), t, ncls, out=conf[1])
    out = {}
    for tag, c in zip(('', '_clean'), conf):
        scores = S.segment_scores(c)
        out['miou%s/%s' % (tag, dataset_key)] = scores['miou']
        out['acc%s/%s' % (tag, dataset_key)] = scores['acc']
        out.update({'iou%s/%s/%d' % (tag, dataset_key, k): float(v) for k, v in enumerate(scores['iou'])})
    if verbose:
        print(' '.join('%s %.4f' % (k, v) for k, v in out.items()))
    return out


# ------------------------------------------------------------------------------------------------ the command line
def _modes_arg(s):
    names = tuple(v.strip() for v in s.split(','))
    bad = [v for v in names if v not in MODE_NAMES]
    if bad:
        raise argparse.ArgumentTypeError('modes: %s expected, got %s' % (' / '.join(MODE_NAMES), ', '.join(bad)))
    return names


def _csv_int(s):
    return tuple(int(v) for v in s.split(','))


def rule_of(a):
    """The MaskRule of parsed arguments (a mapping with label_nc, conn, modes)."""
    return MaskRule(a['label_nc'], a['conn'], a['modes'])


def parser():
    ap = argparse.ArgumentParser(prog='python -m seg2eye_amd.mask_clean',
                                 description='Clean predicted eye masks: keep the components the rule names, fill the rest from the nearest kept pixel.')
    rule = argparse.ArgumentParser(add_help=False)
    rule.add_argument('--conn', type=int, default=8, choices=[4, 8], help='which neighbours join two pixels of one class')
    rule.add_argument('--modes', type=_modes_arg, default=None,
                      help='one of all / largest / border per class, e.g. border,largest,largest,largest (the default for 4 classes)')
    rule.add_argument('--label_nc', type=int, default=4)
    sub = ap.add_subparsers(dest='command', required=True)
    a = sub.add_parser('apply', parents=[rule], help='clean every labels_pred_* array of a mask file')
    a.add_argument('--seg_file', required=True, help='the file(s) `segment predict --out` wrote, comma-separated (one split per file)')
    a.add_argument('--out', required=True, help='the cleaned masks, a drop-in --seg_file (HDF5; <out>.npz without h5py)')
    a.add_argument('--batchSize', type=int, default=64)
    e = sub.add_parser('eval', parents=[rule], help='mIoU of a segmenter checkpoint on the labelled frames of a split, raw and cleaned')
    e.add_argument('--dataroot', required=True, help='the store prepare_openeds wrote (.h5, or .npz without h5py)')
    e.add_argument('--name', default='segmenter', help='the checkpoints live in <checkpoints_dir>/<name>')
    e.add_argument('--checkpoints_dir', default='./checkpoints')
    e.add_argument('--nsf', type=int, default=32, help='# of filters of the first conv layer (a multiple of 8)')
    e.add_argument('--seg_hw', type=_csv_int, default=(320, 200), help='H,W the frames are resized to (multiples of 8)')
    e.add_argument('--compute_dtype', default='bf16', choices=['bf16', 'fp32'])
    e.add_argument('--batchSize', type=int, default=16)
    e.add_argument('--dataset_key', default='validation', choices=['train', 'validation', 'test'])
    e.add_argument('--which_epoch', default='latest')
    return ap


def main(argv=None):
    a = vars(parser().parse_args(argv))
    rule = rule_of(a)
    if a['command'] == 'apply':
        from .prepare_openeds import save_store
        cleaned = clean_store(merge_splits(a['seg_file'], open_tree), rule, batch=a['batchSize'])
        print('cleaned masks of %d split(s) written to %s' % (len(cleaned), save_store(cleaned, a['out'])))
        return None
    from . import segment
    opt = segment.seg_options(**{k: a[k] for k in ('name', 'checkpoints_dir', 'nsf', 'seg_hw', 'label_nc', 'compute_dtype', 'batchSize')})
    net = stage.load_network(segment.build_network, 'S', opt, a['which_epoch'], 'cuda')
    return evaluate(net, open_tree(a['dataroot']), a['dataset_key'], opt, rule)


if __name__ == '__main__':
    main()
