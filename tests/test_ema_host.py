"""Averaged generator weights (--ema_decay), the parts that need no GPU: the C ABI of s2e_adam_flat_ema (declared, exported,
argument errors before any launch), the flags, and optim.FlatAdam's fifth arena on CPU tensors -- absent without a decay (the
default path is untouched), a copy of flat_p with parameter-shaped views with one."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT


def test_adam_flat_ema_is_declared_exported_and_checks_its_arguments():
    from seg2eye_amd import _lib
    import __graft_entry__
    __graft_entry__.build()
    text = open(os.path.join(ROOT, 'include', 'seg2eye_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert re.search(r'\bint\s+s2e_adam_flat_ema\s*\(', text)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), 's2e_adam_flat_ema')
    assert _lib.SIGNATURES['s2e_adam_flat_ema'][0] == _lib.STATUS and len(_lib.SIGNATURES['s2e_adam_flat_ema'][1]) == 9
    L = _lib.lib()
    # host buffers: every call below must return S2E_ERR_ARG (-1) from the argument checks, before any launch
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p, g, m, v, e, hy, eh = (base + 16 * i for i in range(7))
    f = L.s2e_adam_flat_ema
    assert f(p, g, m, v, None, 4, hy, eh, None) == -1                       # null ema
    assert b's2e_adam_flat_ema' in L.s2e_last_error()
    assert f(p, g, m, v, e, 4, hy, None, None) == -1                        # null ema_hyper
    assert f(p, g, m, v, e + 4, 4, hy, eh, None) == -1                      # ema arena not 16-byte aligned
    assert b'16-byte' in L.s2e_last_error()
    assert f(p + 8, g, m, v, e, 4, hy, eh, None) == -1                      # p arena not 16-byte aligned
    assert f(p, g, m, v, e, 0, hy, eh, None) == -1                          # n <= 0
    assert f(p, g, m, v, e, -3, hy, eh, None) == -1
    assert f(None, g, m, v, e, 4, hy, eh, None) == -1 and f(p, g, m, v, e, 4, None, eh, None) == -1


def test_ema_flags():
    from seg2eye_amd.options import default_opt, parse
    o = parse([])
    assert o.ema_decay == 0 and o.ema_start == 0
    o = parse(['--ema_decay', '0.999', '--ema_start', '100'])
    assert o.ema_decay == 0.999 and o.ema_start == 100 and isinstance(o.ema_start, int)
    t = parse(['--use_ema'], is_train=False)
    assert t.use_ema is True and t.ema_decay == 0
    assert parse([], is_train=False).use_ema is False
    assert parse([]).use_ema is False                                       # (a field every opt has; the flag is test.py's)
    with pytest.raises(SystemExit):
        parse(['--use_ema'])
    with pytest.raises(ValueError):
        parse(['--ema_decay', '1.0'])
    d = default_opt()
    assert d.ema_decay == 0.0 and d.ema_start == 0 and d.use_ema is False
    assert default_opt(ema_decay=0.9).ema_decay == 0.9


def _params():
    g = torch.Generator().manual_seed(5)
    shapes = [(16, 8, 3, 3), (16,), (5, 3, 3, 3), (7,), (4, 16, 1, 1), (3, 3)]
    return [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in shapes]


def test_flat_adam_without_decay_is_untouched():
    from seg2eye_amd.optim import FlatAdam
    opt = FlatAdam(_params(), lr=1e-3, betas=(0.0, 0.9))
    assert not hasattr(opt, 'flat_ema') and not hasattr(opt, 'ema_hyper') and not opt.has_ema
    assert sorted(opt.state_dict()) == ['layout', 'lr', 'm', 'm_valid', 'step', 'v']
    with pytest.raises(RuntimeError):
        opt.ema_views()


@pytest.mark.parametrize('cl', [False, True])
def test_flat_adam_ema_arena_and_views(cl):
    from seg2eye_amd.optim import FlatAdam
    ps = _params()
    dead = [ps[-1]]
    opt = FlatAdam(ps[:-1], lr=1e-3, betas=(0.0, 0.9), never_updated=dead, channels_last=cl, ema_decay=0.99, ema_start=3)
    assert opt.has_ema and opt.flat_ema.shape == opt.flat_p.shape and opt.flat_ema.dtype == torch.float32
    assert opt.flat_ema.data_ptr() != opt.flat_p.data_ptr() and torch.equal(opt.flat_ema, opt.flat_p)
    assert opt.ema_hyper.tolist() == [pytest.approx(0.99), 3.0]
    views = opt.ema_views()
    assert len(views) == len(opt.params)
    for q, e in zip(opt.params, views):
        assert e.shape == q.shape and e.stride() == q.stride() and torch.equal(e, q)
        assert e.data_ptr() - opt.flat_ema.data_ptr() == q.data_ptr() - opt.flat_p.data_ptr()
    if cl:
        assert any(not q.is_contiguous() for q in opt.params)               # (16, 8, 3, 3) and (4, 16, 1, 1) are channels-last slices
    # the never-updated tail holds its parameters from the first moment on (the launch stops before it)
    assert opt.numel_active < opt.numel and torch.equal(views[-1], dead[0])
    # exchanging the contents twice is the identity; once, the parameters read the average
    with torch.no_grad():
        opt.flat_ema.mul_(0.5)
    before, avg, q0 = opt.flat_p.clone(), opt.flat_ema.clone(), opt.params[0].detach().clone()
    opt.swap_ema()
    assert torch.equal(opt.flat_ema, before) and torch.equal(opt.flat_p, avg) and torch.equal(opt.params[0], q0 * 0.5)
    opt.swap_ema()
    assert torch.equal(opt.flat_p, before)
    # the state carries the average through the same layout conversion as the moments
    sd = opt.state_dict()
    assert sorted(sd) == ['ema', 'layout', 'lr', 'm', 'm_valid', 'step', 'v']
    other = FlatAdam(_params()[:-1], lr=1e-3, betas=(0.0, 0.9), never_updated=[_params()[-1]], channels_last=not cl, ema_decay=0.5)
    other.load_state_dict(sd)
    for a, b in zip(other.ema_views(), views):
        assert torch.equal(a, b)
    with pytest.raises(ValueError):
        FlatAdam(_params(), lr=1e-3, ema_decay=1.0)
