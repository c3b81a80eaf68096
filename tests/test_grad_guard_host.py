"""The gradient guard (--grad_clip_norm / --skip_nonfinite_grads), the parts that need no GPU: the flags, the C ABI of s2e_grad_guard and
the guarded Adam steps (declared, exported, bound, argument errors before any launch), optim.FlatAdam without the settings (untouched)
and its arena-index -> parameter map, and the host restatement of the coefficient rule against torch.nn.utils.clip_grad_norm_."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

NEW = {'s2e_grad_guard_workspace_bytes': 1, 's2e_grad_guard': 8, 's2e_adam_flat_guarded': 8, 's2e_adam_flat_ema_guarded': 10}


# ------------------------------------------------------------------------------------------------ 1. options
def test_guard_flags():
    from seg2eye_amd.options import default_opt, parse
    o = parse([])
    assert o.grad_clip_norm == 0 and o.skip_nonfinite_grads is False and o.max_consecutive_skips == 100
    o = parse(['--grad_clip_norm', '2.5', '--skip_nonfinite_grads', '--max_consecutive_skips', '7'])
    assert o.grad_clip_norm == 2.5 and o.skip_nonfinite_grads is True and o.max_consecutive_skips == 7
    assert isinstance(o.max_consecutive_skips, int)
    assert parse(['--max_consecutive_skips', '0']).max_consecutive_skips == 0       # 0 = never stop
    with pytest.raises(ValueError):
        parse(['--grad_clip_norm', '-1'])
    with pytest.raises(ValueError):
        parse(['--max_consecutive_skips', '-1'])
    d = default_opt()
    assert d.grad_clip_norm == 0.0 and d.skip_nonfinite_grads is False and d.max_consecutive_skips == 100
    d = default_opt(grad_clip_norm=1.0, skip_nonfinite_grads=True, max_consecutive_skips=3)
    assert d.grad_clip_norm == 1.0 and d.skip_nonfinite_grads is True and d.max_consecutive_skips == 3
    t = parse([], is_train=False)                                                   # (fields every opt has; the flags are train.py's)
    assert t.grad_clip_norm == 0.0 and t.skip_nonfinite_grads is False


# ------------------------------------------------------------------------------------------------ 2. ABI
def test_guard_symbols_are_declared_exported_bound_and_check_their_arguments():
    from seg2eye_amd import _lib
    import __graft_entry__
    __graft_entry__.build()
    text = open(os.path.join(ROOT, 'include', 'seg2eye_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in NEW.items():
        assert re.search(r'\b(int|size_t)\s+%s\s*\(' % name, text), name
        assert hasattr(so, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    L = _lib.lib()
    # host buffers: every call below must return S2E_ERR_ARG (-1) from the argument checks, before any launch
    buf = (ctypes.c_float * 96)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p, g, m, v, e, hy, eh, gd, fb, ws = (base + 32 * i for i in range(10))

    need = L.s2e_grad_guard_workspace_bytes
    assert need(0) == 0 and need(-5) == 0
    assert need(3) > 0 and need(3) % 8 == 0 and need(9_000_003) >= need(4 * 257 + 3) >= need(3)
    n, nb = 4, need(4)
    f = L.s2e_grad_guard
    for args in ((None, n, hy, gd, fb, ws, nb), (g, n, None, gd, fb, ws, nb), (g, n, hy, None, fb, ws, nb), (g, n, hy, gd, None, ws, nb),
                 (g, n, hy, gd, fb, None, nb)):                                     # null pointers
        assert f(*args, None) == -1
        assert b's2e_grad_guard' in L.s2e_last_error()
    assert f(g + 4, n, hy, gd, fb, ws, nb, None) == -1                              # arena not 16-byte aligned
    assert b'aligned' in L.s2e_last_error()
    assert f(g, 0, hy, gd, fb, ws, nb, None) == -1 and f(g, -3, hy, gd, fb, ws, nb, None) == -1      # n <= 0
    assert f(g, n, hy, gd, fb, ws, nb - 1, None) == -1                              # workspace one byte short
    assert b'workspace' in L.s2e_last_error()
    assert f(g, 9_000_003, hy, gd, fb, ws, need(9_000_003) - 1, None) == -1

    f = L.s2e_adam_flat_guarded
    assert f(p, g, m, v, n, hy, None, None) == -1                                   # null guard
    assert b's2e_adam_flat_guarded' in L.s2e_last_error()
    assert f(None, g, m, v, n, hy, gd, None) == -1 and f(p, g, m, v, n, None, gd, None) == -1
    assert f(p, g + 8, m, v, n, hy, gd, None) == -1                                 # g arena not 16-byte aligned
    assert b'16-byte' in L.s2e_last_error()
    assert f(p, g, m, v, 0, hy, gd, None) == -1 and f(p, g, m, v, -3, hy, gd, None) == -1

    f = L.s2e_adam_flat_ema_guarded
    assert f(p, g, m, v, e, n, hy, eh, None, None) == -1                            # null guard
    assert b's2e_adam_flat_ema_guarded' in L.s2e_last_error()
    assert f(p, g, m, v, None, n, hy, eh, gd, None) == -1 and f(p, g, m, v, e, n, hy, None, gd, None) == -1
    assert f(p, g, m, v, e + 4, n, hy, eh, gd, None) == -1                          # ema arena not 16-byte aligned
    assert b'16-byte' in L.s2e_last_error()
    assert f(p, g, m, v, e, 0, hy, eh, gd, None) == -1


# ------------------------------------------------------------------------------------------------ 3. FlatAdam
def _params():
    g = torch.Generator().manual_seed(5)
    #          plain 4-D        1-D    conv, Cin % 8 == 0   1-D   never updated
    shapes = [(5, 3, 3, 3), (7,), (16, 8, 3, 3), (6,), (3, 3)]
    return [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in shapes]


def test_flat_adam_without_the_settings_is_untouched():
    from seg2eye_amd.optim import FlatAdam
    for kw in ({}, {'clip_norm': None, 'skip_nonfinite': False}, {'clip_norm': 0.0}):
        opt = FlatAdam(_params(), lr=1e-3, betas=(0.0, 0.9), **kw)
        assert not opt.has_guard
        for name in ('guard', 'first_bad', 'guard_ws', 'clip_norm', 'skip_nonfinite'):
            assert not hasattr(opt, name), name
        assert sorted(opt.state_dict()) == ['layout', 'lr', 'm', 'm_valid', 'step', 'v']
        with pytest.raises(RuntimeError):
            opt.guard_stats()
    with pytest.raises(ValueError):
        FlatAdam(_params(), lr=1e-3, clip_norm=-1.0)


def test_param_at_maps_arena_elements_to_parameters():
    from seg2eye_amd.optim import FlatAdam
    ps = _params()
    opt = FlatAdam(ps[:-1], lr=1e-3, betas=(0.0, 0.9), never_updated=[ps[-1]], channels_last=True)
    assert opt.cl == [False, False, True, False, False]
    # 135 -> 136 elements, 7 -> 8: the channels-last weight would start at 144 and is moved to the next 256-byte boundary, 192
    assert opt.offsets[:3] == [0, 136, 192] and opt.numel_active == opt.offsets[4] < opt.numel
    for i, (q, off) in enumerate(zip(opt.params, opt.offsets)):
        assert opt.param_at(off) == i and opt.param_at(off + q.numel() - 1) == i     # first and last element of every parameter
    assert opt.param_at(135) is None                                                # the 4-element padding after 135 elements
    assert opt.param_at(143) is None                                                # padding of the 7-element vector
    for k in (144, 170, 191):
        assert opt.param_at(k) is None                                              # inside the 64-element alignment gap
    assert opt.params[opt.param_at(opt.numel_active)] is ps[-1]                     # the never-updated tail
    assert opt.numel == opt.offsets[-1] + 12 and opt.param_at(opt.numel - 1) is None    # (3, 3): 9 elements padded to 12
    assert opt.param_at(opt.offsets[-1] + 8) == 4
    for k in (-1, opt.numel):
        with pytest.raises(IndexError):
            opt.param_at(k)


# ------------------------------------------------------------------------------------------------ 4. the rule, restated
@pytest.mark.parametrize('ratio', [0.25, 0.999, 4.0], ids=['clip-4x', 'clip-barely', 'above'])
def test_guard_coefficient_is_clip_grad_norm(ratio):
    """ops.guard_coefficient (the host restatement of what s2e_grad_guard computes) gives the scaling
    torch.nn.utils.clip_grad_norm_ applies, on three fp64 CPU tensors, for max_norm below and above the norm."""
    from seg2eye_amd.ops.losses import guard_coefficient
    gen = torch.Generator().manual_seed(11)
    grads = [torch.randn(*s, generator=gen, dtype=torch.float64) for s in ((16, 8, 3, 3), (7,), (5, 3))]
    norm = float(torch.sqrt(sum((g * g).sum() for g in grads)))
    max_norm = ratio * norm
    ps = [torch.nn.Parameter(torch.zeros_like(g)) for g in grads]
    for q, g in zip(ps, grads):
        q.grad = g.clone()
    total = torch.nn.utils.clip_grad_norm_(ps, max_norm, norm_type=2)
    assert float(total) == pytest.approx(norm, rel=1e-14)
    c = guard_coefficient(norm, max_norm)
    assert (c < 1.0) == (ratio < 1.0) and c <= 1.0
    for q, g in zip(ps, grads):
        torch.testing.assert_close(q.grad, g * c, rtol=1e-14, atol=0.0)
    # the other branches of the rule
    assert guard_coefficient(norm, 0.0) == 1.0 and guard_coefficient(norm, -1.0) == 1.0     # no clipping
    assert guard_coefficient(norm, max_norm, has_nonfinite=True, skip_nonfinite=True) == 0.0
    assert guard_coefficient(norm, max_norm, has_nonfinite=True, skip_nonfinite=False) != \
        guard_coefficient(norm, max_norm, has_nonfinite=True, skip_nonfinite=False)        # NaN: the unguarded behaviour


# ------------------------------------------------------------------------------------------------ train.py's policy, on a stubbed trainer
class _StubTrainer:
    """What TrainingRun.report() and fit() touch: a guard whose record is scripted, and a save() that counts."""
    has_guard = True

    def __init__(self, records):
        self.records, self.saved = list(records), []

    def grad_health(self):
        return self.records.pop(0)

    def get_latest_losses(self, include_log_losses=False):
        return {'GAN': torch.tensor(1.0)}

    def save(self, epoch):
        self.saved.append(epoch)


class _StubCounter:
    total_steps_so_far, time_per_iter, recorded = 4, 0.1, 0

    def __init__(self, epochs):
        self.epochs = epochs

    def training_epochs(self):
        return range(1, self.epochs + 1)

    def record_current_iter(self):
        self.recorded += 1


def _rec(skipped=0, consecutive=0, first_bad=-1, param=None):
    return {'norm': 1.5, 'coef': 0.0 if consecutive else 1.0, 'skipped': skipped, 'clipped': 0, 'consecutive': consecutive,
            'first_bad': first_bad, 'param': param}


def _run(records, epochs, max_consecutive_skips=3):
    """A TrainingRun around the stubs whose epoch is one progress line (the duty under test)."""
    import train as train_mod
    from seg2eye_amd.options import default_opt
    run = object.__new__(train_mod.TrainingRun)
    run.opt, run.rank, run.epoch = default_opt(skip_nonfinite_grads=True, max_consecutive_skips=max_consecutive_skips), 0, 1
    run.trainer, run.counter, run.visualizer, run._skips_seen = _StubTrainer(records), _StubCounter(epochs), None, set()
    run.one_epoch = lambda epoch: run.report()
    return run, train_mod


def test_a_run_of_skips_stops_training_and_keeps_latest(capsys):
    name = 'netG.up_0.conv_1.weight_orig'
    run, train_mod = _run([{'G': _rec(), 'D': _rec()},
                           {'G': _rec(2, 2, 4711, name), 'D': _rec()},
                           {'G': _rec(3, 3, 4711, name), 'D': _rec()}], epochs=5)
    with pytest.raises(train_mod.NonFiniteGradients) as e:
        run.fit()
    assert 'optimizer G skipped 3 steps in a row' in str(e.value) and name in str(e.value) and '4711' in str(e.value)
    assert run.trainer.saved == [] and run.counter.recorded == 0                    # `latest` is as it was
    out = capsys.readouterr().out
    assert 'saving the model before quitting' not in out
    assert out.count('optimizer G skipped 2 step(s) so far: non-finite gradient in %s (arena element 4711)' % name) == 1
    assert 'grad_norm/G: 1.500' in out and 'grad_skipped/G: 2.000' in out and 'grad_skipped/D: 0.000' in out


def test_first_skips_are_announced_per_optimizer_and_without_a_stale_name(capsys):
    # G's skip is seen after clean steps reset first_bad; D's first skip comes later and is announced too; 0 = never stop
    run, _ = _run([{'G': _rec(1), 'D': _rec()},
                   {'G': _rec(1), 'D': _rec(1, 1, 12, 'netD.discriminator_0.model0.0.weight')},
                   {'G': _rec(1), 'D': _rec(9, 8, 12, 'netD.discriminator_0.model0.0.weight')}], epochs=3, max_consecutive_skips=0)
    run.fit()
    out = capsys.readouterr().out
    assert out.count('optimizer G skipped') == 1 and 'optimizer G skipped 1 step(s) so far: non-finite gradient\n' in out
    assert 'None' not in out and 'element -1' not in out
    assert out.count('optimizer D skipped') == 1 and 'in netD.discriminator_0.model0.0.weight (arena element 12)' in out
    assert run.trainer.saved == ['latest'] and run.counter.recorded == 1            # an ordinary end saves as always
