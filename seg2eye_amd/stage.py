"""What the side trainers of the OpenEDS chain share -- the segmenter (segment.py) and the residual refiner (refine.py):
the options builder, the epoch loop, the uint8 upload, the checkpoint loader and the command line's common flags.  A stage states how a
batch becomes a loss, how an epoch is scored and what its progress line looks like.  The optimiser is looked up when the loop is called."""
import argparse
import types

import numpy as np
import torch


def stage_options(defaults, kw, who):
    """`defaults` overridden by the keyword arguments `kw` as a namespace; a key `defaults` does not have is a TypeError naming `who`."""
    unknown = sorted(set(kw) - set(defaults))
    if unknown:
        raise TypeError('%s: unknown option(s) %s' % (who, ', '.join(unknown)))
    return types.SimpleNamespace(**{**defaults, **kw})


def to_device(device, *arrays):
    """Host arrays (or None) -> tensors on `device`, dtype kept: frames and masks go up as uint8."""
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in arrays]


def draw_flip(rng, n, device):
    """One flip byte per sample from `rng`: a single rand(n)."""
    return torch.from_numpy((rng.rand(n) < 0.5).astype(np.uint8)).to(device)


def load_network(build_network, tag, opt, which_epoch, device):
    from . import checkpoint
    return checkpoint.load_network(build_network(opt, device), tag, which_epoch, opt)


def train_epochs(net, samples, opt, tag, step, validate, line, has_terms, device='cuda', save=True, verbose=True):
    """opt.niter epochs over `samples` in a shuffled order seeded by opt.seed, in batches of opt.batchSize, with FlatAdam(opt.lr).
      step(batch, rng, device) -> (loss, terms or None)   the stage's forward; `rng` is the loop's one RandomState: per epoch the loop
                                                           draws permutation(len(samples)), per batch the stage draws what it needs
      validate(net) -> dict or None                        after every epoch; a dict joins history['scores']
      line(epoch, steps, losses, terms) -> str             the progress line of the last opt.print_freq steps (terms: a (n, k) tensor)
    After every epoch `<epoch>_net_<tag>.pth` and `latest_net_<tag>.pth` are saved.  The losses stay on the device between two progress
    lines: one copy per opt.print_freq steps and one at the end.  -> (net, {'loss': [one float per step], 'scores': [...]} and, with
    has_terms, 'terms': [[...] per step])."""
    from . import checkpoint, optim
    optimizer = optim.FlatAdam(list(net.parameters()), lr=float(opt.lr), betas=(0.9, 0.999))
    rng = np.random.RandomState(int(opt.seed))
    bs = int(opt.batchSize)
    losses, terms, seen = [], [], 0
    history = {'loss': [], 'terms': [], 'scores': []} if has_terms else {'loss': [], 'scores': []}

    def flush():
        nonlocal seen
        recent, recent_t = torch.stack(losses[seen:]).cpu().tolist(), None
        history['loss'] += recent
        if has_terms:
            recent_t = torch.stack(terms[seen:]).cpu()
            history['terms'] += recent_t.tolist()
        seen = len(losses)
        return recent, recent_t
    for epoch in range(1, int(opt.niter) + 1):
        order = rng.permutation(len(samples))
        for b0 in range(0, len(order), bs):
            optimizer.zero_grad()
            loss, t = step([samples[j] for j in order[b0:b0 + bs]], rng, device)
            loss.backward()
            optimizer.step()
            losses.append(loss.detach())
            terms.append(t)
            if verbose and len(losses) - seen >= int(opt.print_freq):
                print(line(epoch, len(losses), *flush()))
        scores = validate(net)
        if scores is not None:
            history['scores'].append(scores)
        if save:
            checkpoint.save_network(net, tag, epoch, opt)
            checkpoint.save_network(net, tag, 'latest', opt)
    if len(losses) > seen:
        flush()
    return net, history


# ------------------------------------------------------------------------------------------------ the command line
def add_flags(p, flags):
    """A stage's own flags, [(flag, add_argument's keywords)], onto a parser."""
    for flag, kw in flags:
        p.add_argument(flag, **kw)


def add_common_flags(p, name, batch_size, inputs=(), net=()):
    """The flags every command of a stage takes; `inputs` sit behind --dataroot, `net` behind --checkpoints_dir."""
    p.add_argument('--dataroot', required=True, help='the store prepare_openeds wrote (.h5, or .npz without h5py)')
    add_flags(p, inputs)
    p.add_argument('--name', default=name, help='the checkpoints live in <checkpoints_dir>/<name>')
    p.add_argument('--checkpoints_dir', default='./checkpoints')
    add_flags(p, net)
    p.add_argument('--label_nc', type=int, default=4)
    p.add_argument('--compute_dtype', default='bf16', choices=['bf16', 'fp32'])
    p.add_argument('--batchSize', type=int, default=batch_size)


def add_train_flags(p, flip_what, train=(), train_last=()):
    """The flags of a stage's `train` behind the common ones; `train` sit behind --lr, `train_last` behind --print_freq."""
    p.add_argument('--niter', type=int, default=20, help='epochs')
    p.add_argument('--lr', type=float, default=1e-3)
    add_flags(p, train)
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--no_flip', action='store_true', help='no horizontal flip of the training %s' % flip_what)
    p.add_argument('--print_freq', type=int, default=50, help='steps between two lines of the running loss')
    add_flags(p, train_last)


def stage_parser(prog, description, name, batch_size, helps, flip_what, predict_split, inputs=(), net=(), train=(), train_last=()):
    """The train / eval / predict command line of a stage -> (parser, the predict subparser, for the stage's output flags).  helps: the
    help lines of the three.  The stage's own flags come as [(flag, add_argument's keywords)] and sit where the help has always listed
    them: `inputs` behind --dataroot, `net` behind --checkpoints_dir, `train` behind --lr, `train_last` behind --print_freq."""
    ap = argparse.ArgumentParser(prog=prog, description=description)
    common = argparse.ArgumentParser(add_help=False)
    add_common_flags(common, name, batch_size, inputs, net)
    sub = ap.add_subparsers(dest='command', required=True)
    t = sub.add_parser('train', parents=[common], help=helps[0])
    add_train_flags(t, flip_what, train, train_last)
    e = sub.add_parser('eval', parents=[common], help=helps[1])
    p = sub.add_parser('predict', parents=[common], help=helps[2])
    for s in (e, p):
        s.add_argument('--dataset_key', default='validation' if s is e else predict_split, choices=['train', 'validation', 'test'])
        s.add_argument('--which_epoch', default='latest')
    return ap, p
