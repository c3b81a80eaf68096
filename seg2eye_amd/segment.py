"""The eye segmenter: train it on an OpenEDS store's labelled frames, score it, and write the masks `style_rank --seg_file`
reads -- the step between `prepare_openeds` and `style_rank` of the chain  prepare_openeds -> segment -> mask_clean -> style_rank -> train -> test
(and -> refine, the residual refiner of seg2eye_amd/refine.py, which reads the same masks and rankings).

The generative and sequence frames of the `train` and `validation` splits are unlabelled; `style_rank` compares them through masks it
expects under /{subset}/{user}/{labels_pred_gen, labels_pred_seq} uint8 (n, 640, 400).  The store holds what such masks can be learned
from: every person's labelled frames (`images_ss` / `labels_ss`).

    python -m seg2eye_amd.segment train   --dataroot openeds.h5 --name seg --niter 20
    python -m seg2eye_amd.segment eval    --dataroot openeds.h5 --name seg --dataset_key validation
    python -m seg2eye_amd.segment predict --dataroot openeds.h5 --name seg --dataset_key train --out masks.h5

Frames go to the device as uint8 and are resized there (`ops.resize_bicubic_u8` to --seg_hw, fp32 in [-1, 1]; labels by
`ops.resize_nearest_u8`; the horizontal flip of `train` is those ops' flip byte).  The network (networks/segmenter.py: EyeSegNet) gives
logits at --seg_hw; the loss is `ops.seg_cross_entropy` (or, with --lambda_dice / --lambda_surface / --edge_alpha, `ops.seg_loss`), a mask is `ops.seg_argmax_u8` of the logits resized to the frame's own size,
the score is mIoU (the OpenEDS segmentation metric) from `ops.seg_confusion`, accumulated on the device and read back once.

The three commands are plain functions too: `train_segmenter`, `evaluate`, `predict_masks`.  The ops are looked up when called.
`python -m seg2eye_amd.seg_augment train` is `train` on augmented data (`train_segmenter(..., augment=rule)`)."""
import numpy as np
import torch

from . import stage
from .openeds_store import open_tree, pred_name, rows_u8

PRED_KEYS = ('images_gen', 'images_seq')
DEFAULTS = dict(nsf=32, seg_hw=(320, 200), label_nc=4, compute_dtype='bf16', batchSize=16, checkpoints_dir='./checkpoints', name='segmenter',
                lr=1e-3, niter=20, class_weights=None, seed=0, no_flip=False, print_freq=50,
                lambda_ce=1.0, lambda_dice=0.0, lambda_surface=0.0, edge_alpha=0.0, edge_radius=2)


def seg_options(**kw):
    """The options EyeSegNet, the checkpoint names and the functions below read; keyword arguments override the defaults."""
    o = stage.stage_options(DEFAULTS, kw, 'seg_options')
    o.seg_hw = tuple(int(v) for v in o.seg_hw)
    if len(o.seg_hw) != 2 or o.seg_hw[0] % 8 or o.seg_hw[1] % 8 or min(o.seg_hw) < 8:
        raise ValueError('--seg_hw: H,W, both multiples of 8, expected, got %s' % (o.seg_hw,))
    return o


def build_network(opt, device='cuda'):
    from .networks.segmenter import EyeSegNet
    torch.manual_seed(int(opt.seed))
    net = EyeSegNet(opt)
    net.init_weights('kaiming')
    return net.to(device)


def _frames_to_input(frames, hw, flip, device):
    """frames (n, 640, 400) uint8 host array -> (n, 1, h, w) fp32 in [-1, 1] on `device`."""
    from .ops import preprocess as P
    return P.resize_bicubic_u8(stage.to_device(device, frames)[0], hw[0], hw[1], flip).unsqueeze(1)


def _no_flip(n, device):
    return torch.zeros(n, dtype=torch.uint8, device=device)


def labelled_samples(store, dataset_key):
    """[(user, row)] of every labelled frame of a split, in the store's order."""
    out = []
    for user in store[dataset_key].keys():
        g = store[dataset_key][user]
        if 'images_ss' in g and 'labels_ss' in g:
            out += [(user, i) for i in range(g['labels_ss'].shape[0])]
    return out


def _labelled_rows(store, dataset_key, key, batch):
    """The rows of `key` ('images_ss' or 'labels_ss') of a batch of labelled_samples, stacked."""
    return rows_u8((store[dataset_key][u][key], i) for u, i in batch)


# ------------------------------------------------------------------------------------------------ eval
def evaluate(net, store, dataset_key, opt, device='cuda', verbose=True):
    """mIoU, per-class IoU and pixel accuracy of `net` on the labelled frames of a split, the masks taken at the frames' own size.
    -> {'miou/<key>', 'iou/<key>/<c>', 'acc/<key>'}; the confusion matrix stays on the device until every batch is in."""
    from .ops import segment as S
    ncls = int(opt.label_nc)
    conf = torch.zeros(ncls, ncls, dtype=torch.int64, device=device)
    samples = labelled_samples(store, dataset_key)
    if not samples:
        raise ValueError("evaluate('%s'): the split has no labelled frames (images_ss / labels_ss)" % dataset_key)
    with torch.no_grad():
        for b0 in range(0, len(samples), int(opt.batchSize)):
            batch = samples[b0:b0 + int(opt.batchSize)]
            truth = _labelled_rows(store, dataset_key, 'labels_ss', batch)
            logits = net(_frames_to_input(_labelled_rows(store, dataset_key, 'images_ss', batch), opt.seg_hw, _no_flip(len(batch), device), device))
            pred = S.seg_argmax_u8(logits, truth.shape[1], truth.shape[2])
            S.seg_confusion(pred, torch.from_numpy(truth).to(device), ncls, out=conf)
    scores = S.segment_scores(conf)
    out = {'miou/%s' % dataset_key: scores['miou'], 'acc/%s' % dataset_key: scores['acc']}
    out.update({'iou/%s/%d' % (dataset_key, c): float(v) for c, v in enumerate(scores['iou'])})
    if verbose:
        print(' '.join('%s %.4f' % (k, v) for k, v in out.items()))
    return out


# ------------------------------------------------------------------------------------------------ train
def train_segmenter(store, opt, net=None, device='cuda', save=True, verbose=True, augment=None):
    """Train on every labelled frame of /train, in a shuffled order seeded by opt.seed, for opt.niter epochs; after every epoch score
    /validation (when the store has it) and save `<epoch>_net_S.pth` and `latest_net_S.pth`.  net: a network to go on from (default: a
    new one).  -> (net, {'loss': [one float per step], 'scores': [one dict per epoch]}).

    With --lambda_dice, --lambda_surface or --edge_alpha set (or --lambda_ce off 1) the loss is `ops.seg_loss` on the
    distance maps and boundary band `ops.seg_dist_maps` makes of the resized, flipped labels of the batch; the history then has
    'terms': [[CE, Dice, Surface] per step] too, and the progress line shows their means.

    augment: None, or an `ops.AugmentRule`.  A step then draws, behind the flip, `augment.draw(rng, len(batch),
    *opt.seg_hw)`, and the network and the loss get `ops.augment_pairs` of the resized, flipped uint8 frames and labels."""
    from .ops import augment as A, preprocess as P, segment as S
    if net is None:
        net = build_network(opt, device)
    samples = labelled_samples(store, 'train')
    if not samples:
        raise ValueError('train_segmenter: /train has no labelled frames (images_ss / labels_ss)')
    ncls = int(opt.label_nc)
    cw = [1.0] * ncls if opt.class_weights is None else [float(v) for v in opt.class_weights]
    if len(cw) != ncls:
        raise ValueError('--class_weights: %d values for %d classes' % (len(cw), ncls))
    weights = torch.tensor(cw, dtype=torch.float32, device=device)
    lam = {k: float(getattr(opt, k)) for k in ('lambda_ce', 'lambda_dice', 'lambda_surface', 'edge_alpha')}
    plain = lam == {'lambda_ce': 1.0, 'lambda_dice': 0.0, 'lambda_surface': 0.0, 'edge_alpha': 0.0}

    def step(batch, rng, device):
        flip = _no_flip(len(batch), device) if opt.no_flip else stage.draw_flip(rng, len(batch), device)
        if augment is None:
            x = _frames_to_input(_labelled_rows(store, 'train', 'images_ss', batch), opt.seg_hw, flip, device)
        else:
            params = augment.draw(rng, len(batch), *opt.seg_hw)
            _, x_u8 = P.resize_bicubic_u8(stage.to_device(device, _labelled_rows(store, 'train', 'images_ss', batch))[0], opt.seg_hw[0], opt.seg_hw[1], flip, return_u8=True)
        y = P.resize_nearest_u8(stage.to_device(device, _labelled_rows(store, 'train', 'labels_ss', batch))[0], opt.seg_hw[0], opt.seg_hw[1], flip)
        if augment is not None:
            x, _, y = A.augment_pairs(x_u8, y, params)
            x = x.unsqueeze(1)
        if plain:
            return S.seg_cross_entropy(net(x), y, weights), None
        phi = band = None
        if lam['lambda_surface'] or lam['edge_alpha']:
            phi, band = S.seg_dist_maps(y, ncls, int(opt.edge_radius))
        return S.seg_loss(net(x), y, weights, phi, band, **lam)

    def validate(net):
        if 'validation' in store and labelled_samples(store, 'validation'):
            return evaluate(net, store, 'validation', opt, device, verbose)

    def line(epoch, steps, losses, terms):
        text = 'epoch %d step %d loss %.4f' % (epoch, steps, sum(losses) / len(losses))
        return text if plain else text + ' CE %.4f Dice %.4f Surface %.4f' % tuple(terms.mean(0).tolist())
    return stage.train_epochs(net, samples, opt, 'S', step, validate, line, not plain, device, save, verbose)


# ------------------------------------------------------------------------------------------------ predict
def predict_masks(net, store, dataset_key, opt, keys=PRED_KEYS, device='cuda', clean=None):
    """-> {dataset_key: {user: {'labels_pred_gen': uint8 (n, 640, 400), 'labels_pred_seq': ...}}}: the mask of every row of the listed
    image keys a person has, row-aligned with the images -- what `style_rank.rank_styles(..., seg_store=...)` takes and what
    `prepare_openeds.save_store` writes for `style_rank --seg_file`.  clean: None, or a `mask_clean.MaskRule`: every batch of masks is
    cleaned by it before it leaves the device."""
    from .ops import segment as S
    out = {}
    bs = int(opt.batchSize)
    with torch.no_grad():
        for user in store[dataset_key].keys():
            g = store[dataset_key][user]
            out[user] = {}
            for key in keys:
                if key not in g:
                    continue
                n, H, W = g[key].shape
                masks = np.zeros((n, H, W), dtype=np.uint8)
                for r0 in range(0, n, bs):
                    frames = rows_u8((g[key], r) for r in range(r0, min(r0 + bs, n)))
                    logits = net(_frames_to_input(frames, opt.seg_hw, _no_flip(len(frames), device), device))
                    batch = S.seg_argmax_u8(logits, H, W)
                    masks[r0:r0 + len(frames)] = (batch if clean is None else clean(batch)).cpu().numpy()
                out[user][pred_name(key)] = masks
    return {dataset_key: out}


# ------------------------------------------------------------------------------------------------ the command line
def _csv(kind):
    return lambda s: tuple(kind(v) for v in s.split(','))


# the stage's own flags, where stage.stage_parser lists them (seg_augment's `train` takes the same)
FLIP_WHAT = 'frames'
NET_FLAGS = [('--nsf', dict(type=int, default=32, help='# of filters of the first conv layer (a multiple of 8)')),
             ('--seg_hw', dict(type=_csv(int), default=(320, 200), help='H,W the frames are resized to (multiples of 8)'))]
TRAIN_FLAGS = [('--class_weights', dict(type=_csv(float), default=None, help='one weight per class, e.g. 1,1,1,1'))]
TRAIN_LAST_FLAGS = [('--lambda_ce', dict(type=float, default=1.0, help='weight of the cross-entropy term')),
                    ('--lambda_dice', dict(type=float, default=0.0, help='weight of the generalised Dice term (classes weighed by inverse squared area)')),
                    ('--lambda_surface', dict(type=float, default=0.0, help='weight of the surface (boundary) term on signed distance maps')),
                    ('--edge_alpha', dict(type=float, default=0.0, help='a pixel within --edge_radius of another class counts 1 + edge_alpha times in the cross-entropy')),
                    ('--edge_radius', dict(type=int, default=2, help='width of the boundary band, in pixels of --seg_hw'))]


def parser():
    ap, p = stage.stage_parser(
        'python -m seg2eye_amd.segment', 'Train, score and apply the eye segmenter (the masks of style_rank --seg_file).', DEFAULTS['name'], DEFAULTS['batchSize'],
        ('train on the labelled frames of /train', 'mIoU of a checkpoint on the labelled frames of a split', 'write the masks of the unlabelled frames of a split'),
        FLIP_WHAT, 'train', net=NET_FLAGS, train=TRAIN_FLAGS, train_last=TRAIN_LAST_FLAGS)
    p.add_argument('--out', required=True, help='the file style_rank --seg_file opens (HDF5; <out>.npz without h5py)')
    p.add_argument('--keys', type=_csv(str), default=PRED_KEYS, help='image keys to segment, e.g. images_gen,images_seq')
    return ap


def main(argv=None):
    a = vars(parser().parse_args(argv))
    command, dataroot = a.pop('command'), a.pop('dataroot')
    which_epoch, dataset_key, out, keys = a.pop('which_epoch', None), a.pop('dataset_key', None), a.pop('out', None), a.pop('keys', None)
    opt = seg_options(**a)
    store = open_tree(dataroot)
    if command == 'train':
        train_segmenter(store, opt)
        return None
    net = stage.load_network(build_network, 'S', opt, which_epoch, 'cuda')
    if command == 'eval':
        return evaluate(net, store, dataset_key, opt)
    from .prepare_openeds import save_store
    masks = predict_masks(net, store, dataset_key, opt, keys=keys)
    print('masks of %d persons written to %s' % (len(masks[dataset_key]), save_store(masks, out)))


if __name__ == '__main__':
    main()
