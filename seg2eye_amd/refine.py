"""The residual refiner: the stage the reference's authors won the OpenEDS challenge with (refinenet/README.md) -- take the
top-ranked frame of the same person, predict a residual from [target mask, that frame, that frame's mask], add it to the frame, clamp to
[-1, 1] and train directly on the challenge's error.  The last step of the chain
prepare_openeds -> segment -> style_rank -> refine.

    python -m seg2eye_amd.refine train   --dataroot openeds.h5 --style_ref refs_train.h5,refs_val.h5 --seg_file masks_train.h5,masks_val.h5 --name refiner
    python -m seg2eye_amd.refine eval    --dataroot openeds.h5 --style_ref refs_val.h5 --seg_file masks_val.h5 --name refiner --dataset_key validation
    python -m seg2eye_amd.refine predict --dataroot openeds.h5 --style_ref refs_test.h5 --name refiner --dataset_key test --out submission/

A TARGET is a row of the split's label key, named by its cleaned file name.  Its REFERENCE is an entry (index, subset) of the ranking
`style_rank` wrote for that name: a frame of the same person and that frame's mask.  Which keys a split uses, what the subset byte
means and where a frame's mask lives is stated once, in seg2eye_amd/openeds_store.py (`split_keys`, `candidate_row`, `mask_source`).
Training draws uniformly among the first --refine_top listed candidates; eval and predict take the first (the reference's `pick1`).

Frames and masks go to the device as uint8 and stay uint8: `ops.refine_input` writes the network input, the network (networks/refiner.py:
EyeRefineNet) gives the residual at the frames' own size, `ops.refine_loss` is the loss and `ops.refine_predict_u8` the submission bytes.
The score is the challenge's error of the uint8 predictions (`ops.openeds_error_u8`, x 1471 as the Tester prints it), next to the same
for the unrefined reference frames: the baseline the refiner has to beat.

The three commands are plain functions too: `train_refiner`, `evaluate`, `predict_frames`.  The ops are looked up when called."""
import os

import numpy as np
import torch

from . import openeds_store as O, stage

INPUT_CHANNELS = 8                      # the network input's channel pitch: the three planes and structural zeros (16 bytes of bf16)
SCALE = 1471                            # the Tester's scaling of the mean per-image error
DEFAULTS = dict(nrf=32, label_nc=4, compute_dtype='bf16', batchSize=8, checkpoints_dir='./checkpoints', name='refiner', lr=1e-3, niter=20,
                seed=0, no_flip=False, print_freq=50, lambda_eds=1.0, lambda_l1=0.0, refine_top=100)


def refine_options(**kw):
    """The options EyeRefineNet, the checkpoint names and the functions below read; keyword arguments override the defaults."""
    o = stage.stage_options(DEFAULTS, kw, 'refine_options')
    if int(o.refine_top) < 1:
        raise ValueError('--refine_top: at least 1 expected, got %s' % (o.refine_top,))
    return o


def build_network(opt, device='cuda'):
    """A new EyeRefineNet whose `out` is zero: it predicts its reference frame, and training starts from the nearest-neighbour baseline."""
    from .networks.refiner import EyeRefineNet
    torch.manual_seed(int(opt.seed))
    net = EyeRefineNet(opt)
    net.init_weights('kaiming')
    with torch.no_grad():
        net.out.weight.zero_()
        net.out.bias.zero_()
    return net.to(device)


# ------------------------------------------------------------------------------------------------ the sampler (host only)
def label_keys(dataset_key):
    """-> (the key of the target masks, the key of their file names), as style_rank.rank_styles names its targets."""
    return O.split_keys(dataset_key)[1:]


def targets(store, dataset_key):
    """[(user, row, file name)] of every target mask of a split, in the store's order."""
    label_key, names_key = label_keys(dataset_key)
    out = []
    for user in store[dataset_key].keys():
        g = store[dataset_key][user]
        if label_key in g and names_key in g:
            out += [(user, i, O.clean_filename(n)) for i, n in enumerate(np.asarray(g[names_key]))]
    return out


def pick_reference(store, seg_store, refs, dataset_key, user, fname, top=1, rng=None):
    """The reference of one target -> (image key, row, mask holder, mask key): the frame is store[dataset_key][user][image key][row], its
    mask holder[mask key][row].  The candidate is the first listed one, or with `rng` (a numpy RandomState) one of the first `top`, drawn
    uniformly.  A target without an entry, an index out of range or an unknown subset byte is a ValueError that names the person and
    the file."""
    who = "%s/%s '%s'" % (dataset_key, user, fname)
    try:
        entry = refs[dataset_key][user][fname]
        index, subset = np.asarray(entry['index']), np.asarray(entry['subset'])
    except KeyError:
        raise ValueError('%s: the style ranking has no entry for this target' % who) from None
    if len(index) < 1 or len(subset) != len(index):
        raise ValueError('%s: the style ranking lists no candidate (%d indices, %d subsets)' % (who, len(index), len(subset)))
    pos = 0 if rng is None else int(rng.randint(0, min(int(top), len(index))))
    idx, sub = int(index[pos]), bytes(subset[pos])
    g = store[dataset_key][user]
    try:
        image_key, row = O.candidate_row(g, dataset_key, idx, sub)
    except ValueError:
        raise ValueError('%s: candidate %d comes from an unknown subset %r (b\'g\' or b\'s\')' % (who, pos, sub)) from None
    if image_key not in g or not 0 <= row < g[image_key].shape[0]:
        raise ValueError('%s: candidate %d is index %d of subset %r, row %d of %d %s' % (who, pos, idx, sub, row, g[image_key].shape[0] if image_key in g else 0, image_key))
    try:
        seg_group = seg_store[dataset_key][user]
    except (KeyError, TypeError):
        seg_group = None
    holder, mask_key = O.mask_source(g, seg_group, dataset_key, image_key)
    if holder is None or mask_key not in holder:
        raise ValueError('%s: the masks (--seg_file) hold no %s/%s/%s' % (who, dataset_key, user, mask_key))
    if holder[mask_key].shape[0] != g[image_key].shape[0]:
        raise ValueError('%s: %d masks %s for %d %s' % (who, holder[mask_key].shape[0], mask_key, g[image_key].shape[0], image_key))
    return image_key, row, holder, mask_key


def gather(store, dataset_key, batch, picks):
    """batch [(user, row, file name)], picks [pick_reference's result] -> uint8 host arrays (tmask, rimg, rmask, truth or None)."""
    label_key, _ = label_keys(dataset_key)
    tmask = O.rows_u8((store[dataset_key][u][label_key], i) for u, i, _ in batch)
    rimg = O.rows_u8((store[dataset_key][u][k], r) for (u, _, _), (k, r, _, _) in zip(batch, picks))
    rmask = O.rows_u8((h[mk], r) for _, r, h, mk in picks)
    truth = None if dataset_key == 'test' else O.rows_u8((store[dataset_key][u]['images_ss'], i) for u, i, _ in batch)
    return tmask, rimg, rmask, truth


def _network_input(arrays, flip, opt, device):
    """gather's arrays -> (rimg and truth (or None) on the device as uint8, the network input `ops.refine_input` makes of the planes)."""
    from .networks.base_network import compute_dtype_of
    from .ops import refine as R
    tmask, rimg, rmask, truth = stage.to_device(device, *arrays)
    return rimg, truth, R.refine_input(tmask, rimg, rmask, flip, ncls=int(opt.label_nc), channels=INPUT_CHANNELS, dtype=compute_dtype_of(opt))


def _first_batches(store, seg_store, refs, dataset_key, opt):
    """The split's targets in batches, each with its first listed reference."""
    todo = targets(store, dataset_key)
    if not todo:
        raise ValueError("'%s' has no target masks (%s / %s)" % ((dataset_key,) + label_keys(dataset_key)))
    for b0 in range(0, len(todo), int(opt.batchSize)):
        batch = todo[b0:b0 + int(opt.batchSize)]
        picks = [pick_reference(store, seg_store, refs, dataset_key, u, f) for u, _, f in batch]
        yield batch, gather(store, dataset_key, batch, picks)


# ------------------------------------------------------------------------------------------------ eval
def evaluate(net, store, seg_store, refs, dataset_key, opt, device='cuda', verbose=True):
    """The challenge's error of a split's refined frames and of its unrefined reference frames, both on uint8 images against the uint8
    truth, in the Tester's scaling (1471 x the mean per-image error).  -> {'openeds/<key>', 'openeds_nn/<key>'}; the per-image errors
    stay on the device until every batch is in."""
    from .ops import losses as Q, refine as R
    if dataset_key == 'test':
        raise ValueError("evaluate('test'): the test split has no ground truth")
    refined, nearest = [], []
    with torch.no_grad():
        for _, arrays in _first_batches(store, seg_store, refs, dataset_key, opt):
            rimg, truth, x = _network_input(arrays, None, opt, device)
            refined.append(Q.openeds_error_u8(R.refine_predict_u8(net(x), rimg), truth))
            nearest.append(Q.openeds_error_u8(rimg, truth))
    out = {'openeds/%s' % dataset_key: float(torch.cat(refined).double().mean()) * SCALE,
           'openeds_nn/%s' % dataset_key: float(torch.cat(nearest).double().mean()) * SCALE}
    if verbose:
        print(' '.join('%s %.4f' % (k, v) for k, v in out.items()))
    return out


# ------------------------------------------------------------------------------------------------ train
def train_refiner(store, seg_store, refs, opt, net=None, device='cuda', save=True, verbose=True):
    """Train on every target of /train, in a shuffled order seeded by opt.seed, for opt.niter epochs: each target with one of its first
    opt.refine_top listed references, drawn per step, and (unless --no_flip) a horizontal flip of all its planes.  After every epoch
    score /validation (when the store, the ranking and the masks have it) and save `<epoch>_net_R.pth` and `latest_net_R.pth`.
    net: a network to go on from (default: a new one).  -> (net, {'loss': [one float per step], 'terms': [[eds_loss, l1, 1471
    eds_loss] per step], 'scores': [one dict per epoch]}); the losses stay on the device between two progress lines."""
    from .ops import refine as R
    if net is None:
        net = build_network(opt, device)
    samples = targets(store, 'train')
    if not samples:
        raise ValueError('train_refiner: /train has no target masks (labels_ss / images_ss_filenames)')
    scored = all(s is not None and 'validation' in s for s in (store, refs, seg_store)) and bool(targets(store, 'validation'))

    def step(batch, rng, device):
        picks = [pick_reference(store, seg_store, refs, 'train', u, f, int(opt.refine_top), rng) for u, _, f in batch]
        flip = None if opt.no_flip else stage.draw_flip(rng, len(batch), device)
        rimg, truth, x = _network_input(gather(store, 'train', batch, picks), flip, opt, device)
        loss, terms, _ = R.refine_loss(net(x), rimg, truth, flip, float(opt.lambda_eds), float(opt.lambda_l1))
        return loss, terms

    def validate(net):
        return evaluate(net, store, seg_store, refs, 'validation', opt, device, verbose) if scored else None

    def line(epoch, steps, losses, terms):
        return 'epoch %d step %d loss %.5f eds %.5f l1 %.5f score %.3f' % ((epoch, steps, sum(losses) / len(losses)) + tuple(terms.mean(0).tolist()))
    return stage.train_epochs(net, samples, opt, 'R', step, validate, line, True, device, save, verbose)


# ------------------------------------------------------------------------------------------------ predict
def predict_frames(net, store, seg_store, refs, dataset_key, opt, device='cuda', out=None):
    """-> {user: {file name: uint8 (H, W)}}: the refined frame of every target of the split.  out: a directory that gets one
    `<file name>.npy` per target and `pred_npy_list.txt`, the list of their paths, as the reference's evaluate_refinenet.py writes."""
    from .ops import refine as R
    frames, paths = {}, []
    if out is not None:
        os.makedirs(out, exist_ok=True)
    with torch.no_grad():
        for batch, arrays in _first_batches(store, seg_store, refs, dataset_key, opt):
            rimg, _, x = _network_input(arrays, None, opt, device)
            pred = R.refine_predict_u8(net(x), rimg).cpu().numpy()
            for (user, _, fname), p in zip(batch, pred):
                frames.setdefault(user, {})[fname] = p
                if out is not None:
                    paths.append(os.path.join(out, '%s.npy' % fname))
                    np.save(paths[-1], p)
    if out is not None:
        with open(os.path.join(out, 'pred_npy_list.txt'), 'w') as f:
            f.write(''.join(p + os.linesep for p in paths))
    return frames


# ------------------------------------------------------------------------------------------------ the command line
def parser():
    ap, p = stage.stage_parser(
        'python -m seg2eye_amd.refine', 'Train, score and apply the residual refiner: nearest frame plus a learned correction.', 'refiner', 8,
        ('train on the targets of /train', 'the challenge\'s error of a checkpoint, and of the unrefined reference frames, on a split',
         'write one .npy per target mask of a split'), 'samples', 'test',
        inputs=[('--style_ref', dict(required=True, help='the ranking(s) style_rank wrote, one file per split, comma-separated')),
                ('--seg_file', dict(default=None, help='the masks `segment predict` wrote, one file per split, comma-separated (test needs none for its labelled frames)'))],
        net=[('--nrf', dict(type=int, default=32, help='# of filters of the first conv layer (a multiple of 8)'))],
        train=[('--lambda_eds', dict(type=float, default=1.0, help='weight of the challenge\'s error, the mean per-image 127.5 sqrt(sum d^2) / (H W)')),
               ('--lambda_l1', dict(type=float, default=0.0, help='weight of mean |d|')),
               ('--refine_top', dict(type=int, default=100, help='a training step draws its reference among the first N listed candidates'))])
    p.add_argument('--out', required=True, help='the directory of the .npy files and pred_npy_list.txt')
    return ap


def main(argv=None):
    a = vars(parser().parse_args(argv))
    command, dataroot, style_ref, seg_file = a.pop('command'), a.pop('dataroot'), a.pop('style_ref'), a.pop('seg_file')
    which_epoch, dataset_key, out = a.pop('which_epoch', None), a.pop('dataset_key', None), a.pop('out', None)
    opt = refine_options(**a)
    store, refs = O.open_tree(dataroot), O.merge_splits(style_ref, lambda path: O.open_tree(path, O.REFS_DEPTH))
    seg_store = O.merge_splits(seg_file, O.open_tree)
    if command == 'train':
        train_refiner(store, seg_store, refs, opt)
        return None
    net = stage.load_network(build_network, 'R', opt, which_epoch, 'cuda')
    if command == 'eval':
        return evaluate(net, store, seg_store, refs, dataset_key, opt)
    frames = predict_frames(net, store, seg_store, refs, dataset_key, opt, out=out)
    print('%d frames of %d persons written to %s' % (sum(len(v) for v in frames.values()), len(frames), out))


if __name__ == '__main__':
    main()
