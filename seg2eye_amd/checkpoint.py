"""Checkpoint naming and key compatibility of the reference (util/util.py:195-221):
<checkpoints_dir>/<name>/<epoch>_net_<G|D|E>.pth holding net.state_dict() on the CPU; a DataParallel
'module.' prefix on either side is tolerated.  With averaged weights (--ema_decay) two more files, labels `G_ema` / `E_ema`:
the same keys, shapes and dtypes with the AVERAGED parameters and the live buffers, so that renamed over the plain files they
load anywhere the plain ones do."""
import os

import torch


def _path(label, epoch, opt):
    return os.path.join(opt.checkpoints_dir, opt.name, '%s_net_%s.pth' % (epoch, label))


def _save_state(sd, label, epoch, opt):
    path = _path(label, epoch, opt)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    torch.save({k: v.detach().cpu().clone() for k, v in sd.items()}, path)
    return path


def save_network(net, label, epoch, opt):
    return _save_state(net.state_dict(), label, epoch, opt)


def ema_state_dict(net, ema_of):
    """net.state_dict() with every parameter's value replaced by its average; buffers are the live ones.
    ema_of: {id(parameter): tensor of the parameter's shape} (optim.FlatAdam.ema_views)."""
    named = dict(net.named_parameters())
    return {k: (ema_of[id(named[k])] if k in named else v) for k, v in net.state_dict().items()}


def save_network_ema(net, label, epoch, opt, ema_of):
    return _save_state(ema_state_dict(net, ema_of), label + '_ema', epoch, opt)


def ema_files_exist(epoch, opt, labels=('G', 'E')):
    return all(os.path.exists(_path(lab + '_ema', epoch, opt)) for lab in labels)


def load_ema(net, label, epoch, opt, ema_of):
    """The parameters of `<epoch>_net_<label>_ema.pth` into the average's views (the file's buffers are the live network's and
    are not read: `load_network` has put them in place from the plain file)."""
    sd = torch.load(_path(label + '_ema', epoch, opt), map_location='cpu')
    sd = {(k[len('module.'):] if k.startswith('module.') else k): v for k, v in sd.items()}
    with torch.no_grad():
        for k, q in net.named_parameters():
            if k not in sd:
                raise KeyError('averaged checkpoint %s lacks the key %s' % (_path(label + '_ema', epoch, opt), k))
            ema_of[id(q)].copy_(sd[k])


def load_network(net, label, epoch, opt):
    if label.endswith('_ema') and not os.path.exists(_path(label, epoch, opt)):
        raise FileNotFoundError('--use_ema: %s does not exist (written by a training run with --ema_decay)' % _path(label, epoch, opt))
    sd = torch.load(_path(label, epoch, opt), map_location='cpu')
    sd = {(k[len('module.'):] if k.startswith('module.') else k): v for k, v in sd.items()}
    with torch.no_grad():
        own = net.state_dict()
        missing = [k for k in own if k not in sd]
        if missing:
            raise KeyError('checkpoint lacks keys: %s' % missing[:5])
        for k, v in own.items():
            v.copy_(sd[k])          # in place: parameters may alias an optimizer arena
    return net
