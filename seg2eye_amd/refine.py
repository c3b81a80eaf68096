"""The residual refiner: the stage the reference's authors won the OpenEDS challenge with (refinenet/README.md) -- take the
top-ranked frame of the same person, predict a residual from [target mask, that frame, that frame's mask], add it to the frame, clamp to
[-1, 1] and train directly on the challenge's error.  The last step of the chain
prepare_openeds -> segment -> style_rank -> refine.

    python -m seg2eye_amd.refine train   --dataroot openeds.h5 --style_ref refs_train.h5,refs_val.h5 --seg_file masks_train.h5,masks_val.h5 --name refiner
    python -m seg2eye_amd.refine eval    --dataroot openeds.h5 --style_ref refs_val.h5 --seg_file masks_val.h5 --name refiner --dataset_key validation
    python -m seg2eye_amd.refine predict --dataroot openeds.h5 --style_ref refs_test.h5 --name refiner --dataset_key test --out submission/

A TARGET is a row of the split's label key (`labels_ss`; `labels_gen` for 'test'), named as `style_rank.clean_filename` names it.  Its
REFERENCE is an entry (index, subset) of the ranking `style_rank` wrote for that name, resolved by the convention
`OpenEDSDataset.get_style_images` undoes: b'g' is row `index` of `images_gen` with the mask `labels_pred_gen` of --seg_file (for 'test':
`images_ss` with the store's true `labels_ss`), b's' is row `index - n_gen` of `images_seq` with `labels_pred_seq`.  Training draws
uniformly among the first --refine_top listed candidates; eval and predict take the first (the reference's `pick1`).

Frames and masks go to the device as uint8 and stay uint8: `ops.refine_input` writes the network input, the network (networks/refiner.py:
EyeRefineNet) gives the residual at the frames' own size, `ops.refine_loss` is the loss and `ops.refine_predict_u8` the submission bytes.
The score is the challenge's error of the uint8 predictions (`ops.openeds_error_u8`, x 1471 as the Tester prints it), next to the same
for the unrefined reference frames: the baseline the refiner has to beat.

The three commands are plain functions too: `train_refiner`, `evaluate`, `predict_frames`.  The ops are looked up when called."""
import argparse
import os
import types

import numpy as np
import torch

from .style_rank import clean_filename

INPUT_CHANNELS = 8                      # the network input's channel pitch: the three planes and structural zeros (16 bytes of bf16)
SCALE = 1471                            # the Tester's scaling of the mean per-image error


def refine_options(**kw):
    """The options EyeRefineNet, the checkpoint names and the functions below read; keyword arguments override the defaults."""
    o = dict(nrf=32, label_nc=4, compute_dtype='bf16', batchSize=8, checkpoints_dir='./checkpoints', name='refiner', lr=1e-3, niter=20,
             seed=0, no_flip=False, print_freq=50, lambda_eds=1.0, lambda_l1=0.0, refine_top=100)
    unknown = sorted(set(kw) - set(o))
    if unknown:
        raise TypeError('refine_options: unknown option(s) %s' % ', '.join(unknown))
    o.update(kw)
    if int(o['refine_top']) < 1:
        raise ValueError('--refine_top: at least 1 expected, got %s' % (o['refine_top'],))
    return types.SimpleNamespace(**o)


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
    return ('labels_gen', 'labels_gen_filenames') if dataset_key == 'test' else ('labels_ss', 'images_ss_filenames')


def targets(store, dataset_key):
    """[(user, row, file name)] of every target mask of a split, in the store's order."""
    label_key, names_key = label_keys(dataset_key)
    out = []
    for user in store[dataset_key].keys():
        g = store[dataset_key][user]
        if label_key in g and names_key in g:
            out += [(user, i, clean_filename(n)) for i, n in enumerate(np.asarray(g[names_key]))]
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
    first_key = 'images_ss' if dataset_key == 'test' else 'images_gen'
    if sub == b'g':
        image_key, row = first_key, idx
    elif sub == b's':
        image_key, row = 'images_seq', idx - (g[first_key].shape[0] if first_key in g else 0)
    else:
        raise ValueError('%s: candidate %d comes from an unknown subset %r (b\'g\' or b\'s\')' % (who, pos, sub))
    if image_key not in g or not 0 <= row < g[image_key].shape[0]:
        raise ValueError('%s: candidate %d is index %d of subset %r, row %d of %d %s' % (who, pos, idx, sub, row, g[image_key].shape[0] if image_key in g else 0, image_key))
    if dataset_key == 'test' and sub == b'g':
        holder, mask_key = g, 'labels_ss'
    else:
        mask_key = image_key.replace('images_', 'labels_pred_', 1)
        try:
            holder = seg_store[dataset_key][user]
            holder[mask_key]
        except (KeyError, TypeError):
            raise ValueError('%s: the masks (--seg_file) hold no %s/%s/%s' % (who, dataset_key, user, mask_key)) from None
    if holder[mask_key].shape[0] != g[image_key].shape[0]:
        raise ValueError('%s: %d masks %s for %d %s' % (who, holder[mask_key].shape[0], mask_key, g[image_key].shape[0], image_key))
    return image_key, row, holder, mask_key


def _u8(a):
    return np.asarray(a, dtype=np.uint8)


def gather(store, dataset_key, batch, picks):
    """batch [(user, row, file name)], picks [pick_reference's result] -> uint8 host arrays (tmask, rimg, rmask, truth or None)."""
    label_key, _ = label_keys(dataset_key)
    tmask = np.stack([_u8(store[dataset_key][u][label_key][int(i)]) for u, i, _ in batch])
    rimg = np.stack([_u8(store[dataset_key][u][k][int(r)]) for (u, _, _), (k, r, _, _) in zip(batch, picks)])
    rmask = np.stack([_u8(h[mk][int(r)]) for _, r, h, mk in picks])
    truth = None if dataset_key == 'test' else np.stack([_u8(store[dataset_key][u]['images_ss'][int(i)]) for u, i, _ in batch])
    return tmask, rimg, rmask, truth


def _to(device, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in arrays]


def _cdtype(opt):
    from .networks.base_network import compute_dtype_of
    return compute_dtype_of(opt)


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
            tmask, rimg, rmask, truth = _to(device, *arrays)
            x = R.refine_input(tmask, rimg, rmask, None, ncls=int(opt.label_nc), channels=INPUT_CHANNELS, dtype=_cdtype(opt))
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
    from . import checkpoint
    from .optim import FlatAdam
    from .ops import refine as R
    if net is None:
        net = build_network(opt, device)
    samples = targets(store, 'train')
    if not samples:
        raise ValueError('train_refiner: /train has no target masks (labels_ss / images_ss_filenames)')
    optimizer = FlatAdam(list(net.parameters()), lr=float(opt.lr), betas=(0.9, 0.999))
    rng = np.random.RandomState(int(opt.seed))
    bs, top, dtype = int(opt.batchSize), int(opt.refine_top), _cdtype(opt)
    validate = all(s is not None and 'validation' in s for s in (store, refs, seg_store)) and bool(targets(store, 'validation'))
    losses, terms, history, seen = [], [], {'loss': [], 'terms': [], 'scores': []}, 0
    for epoch in range(1, int(opt.niter) + 1):
        order = rng.permutation(len(samples))
        for b0 in range(0, len(order), bs):
            batch = [samples[j] for j in order[b0:b0 + bs]]
            picks = [pick_reference(store, seg_store, refs, 'train', u, f, top, rng) for u, _, f in batch]
            flip = None if opt.no_flip else torch.from_numpy((rng.rand(len(batch)) < 0.5).astype(np.uint8)).to(device)
            tmask, rimg, rmask, truth = _to(device, *gather(store, 'train', batch, picks))
            x = R.refine_input(tmask, rimg, rmask, flip, ncls=int(opt.label_nc), channels=INPUT_CHANNELS, dtype=dtype)
            optimizer.zero_grad()
            loss, t, _ = R.refine_loss(net(x), rimg, truth, flip, float(opt.lambda_eds), float(opt.lambda_l1))
            loss.backward()
            optimizer.step()
            losses.append(loss.detach())
            terms.append(t)
            if verbose and len(losses) - seen >= int(opt.print_freq):
                recent, recent_t = torch.stack(losses[seen:]).cpu().tolist(), torch.stack(terms[seen:]).cpu()      # (one copy per print_freq steps)
                history['loss'] += recent
                history['terms'] += recent_t.tolist()
                seen = len(losses)
                print('epoch %d step %d loss %.5f eds %.5f l1 %.5f score %.3f' % ((epoch, seen, sum(recent) / len(recent)) + tuple(recent_t.mean(0).tolist())))
        if validate:
            history['scores'].append(evaluate(net, store, seg_store, refs, 'validation', opt, device, verbose))
        if save:
            checkpoint.save_network(net, 'R', epoch, opt)
            checkpoint.save_network(net, 'R', 'latest', opt)
    if len(losses) > seen:
        history['loss'] += torch.stack(losses[seen:]).cpu().tolist()
        history['terms'] += torch.stack(terms[seen:]).cpu().tolist()
    return net, history


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
            tmask, rimg, rmask, _ = _to(device, *arrays)
            x = R.refine_input(tmask, rimg, rmask, None, ncls=int(opt.label_nc), channels=INPUT_CHANNELS, dtype=_cdtype(opt))
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
def _open_store(path):
    if path.endswith('.npz'):
        from .prepare_openeds import load_store
        return load_store(path)
    import h5py
    return h5py.File(path, 'r')


def _open_refs(path):
    if path.endswith('.npz'):
        from .style_rank import load_refs
        return load_refs(path)
    import h5py
    return h5py.File(path, 'r')


def _splits(paths, opener):
    """The files of a comma-separated list as one mapping {split: ...}: style_rank and `segment predict` write one split per file."""
    merged = {}
    for p in (paths or '').split(','):
        if p:
            f = opener(p)
            merged.update({k: f[k] for k in f.keys()})
    return merged


def _load(opt, which_epoch, device):
    from . import checkpoint
    return checkpoint.load_network(build_network(opt, device), 'R', which_epoch, opt)


def parser():
    ap = argparse.ArgumentParser(prog='python -m seg2eye_amd.refine', description='Train, score and apply the residual refiner: nearest frame plus a learned correction.')
    common = argparse.ArgumentParser(add_help=False)
    common.add_argument('--dataroot', required=True, help='the store prepare_openeds wrote (.h5, or .npz without h5py)')
    common.add_argument('--style_ref', required=True, help='the ranking(s) style_rank wrote, one file per split, comma-separated')
    common.add_argument('--seg_file', default=None, help='the masks `segment predict` wrote, one file per split, comma-separated (test needs none for its labelled frames)')
    common.add_argument('--name', default='refiner', help='the checkpoints live in <checkpoints_dir>/<name>')
    common.add_argument('--checkpoints_dir', default='./checkpoints')
    common.add_argument('--nrf', type=int, default=32, help='# of filters of the first conv layer (a multiple of 8)')
    common.add_argument('--label_nc', type=int, default=4)
    common.add_argument('--compute_dtype', default='bf16', choices=['bf16', 'fp32'])
    common.add_argument('--batchSize', type=int, default=8)
    sub = ap.add_subparsers(dest='command', required=True)
    t = sub.add_parser('train', parents=[common], help='train on the targets of /train')
    t.add_argument('--niter', type=int, default=20, help='epochs')
    t.add_argument('--lr', type=float, default=1e-3)
    t.add_argument('--lambda_eds', type=float, default=1.0, help='weight of the challenge\'s error, the mean per-image 127.5 sqrt(sum d^2) / (H W)')
    t.add_argument('--lambda_l1', type=float, default=0.0, help='weight of mean |d|')
    t.add_argument('--refine_top', type=int, default=100, help='a training step draws its reference among the first N listed candidates')
    t.add_argument('--seed', type=int, default=0)
    t.add_argument('--no_flip', action='store_true', help='no horizontal flip of the training samples')
    t.add_argument('--print_freq', type=int, default=50, help='steps between two lines of the running loss')
    e = sub.add_parser('eval', parents=[common], help='the challenge\'s error of a checkpoint, and of the unrefined reference frames, on a split')
    p = sub.add_parser('predict', parents=[common], help='write one .npy per target mask of a split')
    for s in (e, p):
        s.add_argument('--dataset_key', default='validation' if s is e else 'test', choices=['train', 'validation', 'test'])
        s.add_argument('--which_epoch', default='latest')
    p.add_argument('--out', required=True, help='the directory of the .npy files and pred_npy_list.txt')
    return ap


def main(argv=None):
    a = vars(parser().parse_args(argv))
    command, dataroot, style_ref, seg_file = a.pop('command'), a.pop('dataroot'), a.pop('style_ref'), a.pop('seg_file')
    which_epoch, dataset_key, out = a.pop('which_epoch', None), a.pop('dataset_key', None), a.pop('out', None)
    opt = refine_options(**a)
    store, refs, seg_store = _open_store(dataroot), _splits(style_ref, _open_refs), _splits(seg_file, _open_store)
    if command == 'train':
        train_refiner(store, seg_store, refs, opt)
    elif command == 'eval':
        return evaluate(_load(opt, which_epoch, 'cuda'), store, seg_store, refs, dataset_key, opt)
    else:
        frames = predict_frames(_load(opt, which_epoch, 'cuda'), store, seg_store, refs, dataset_key, opt, out=out)
        print('%d frames of %d persons written to %s' % (sum(len(v) for v in frames.values()), len(frames), out))


if __name__ == '__main__':
    main()
