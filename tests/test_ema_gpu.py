"""Averaged generator weights (--ema_decay) on the GPU: s2e_adam_flat_ema against its definition and against s2e_adam_flat, the
average a trainer keeps (eager and hipGraphs, fp32 and bf16), `Pix2PixTrainer.ema_scope()`, and the checkpoint files through
train.py / test.py.

The bound on the average (tests 4 and 5) is derived, not measured: the kernel evaluates decay * ema + (1 - decay) * p in fp32 on
values bounded by max|p|, so every step adds at most about one ulp of max|p| (2^-23 max|p|) to the error it inherits (scaled by
decay < 1); over K steps that is K * 2^-23 max|p|, doubled for margin: K * 2^-22 * max|p|.  The reference value is the same
recurrence in fp64 over the kernel's own fp32 parameter sequence."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _opt(**kw):
    from seg2eye_amd.options import default_opt
    kw.setdefault('gpu_ids', [0])
    return default_opt(**kw)


def _batch(n, h, w, seed):
    from seg2eye_amd import synthetic as syn
    b = syn.make_batch(n, h, w, seed=seed)
    return {'label': torch.from_numpy(b['label']), 'style_image': torch.from_numpy(b['style_image']),
            'target': torch.from_numpy(b['target']), 'filename': b['filename']}


def _ema_bound(steps, pmax):
    return steps * 2.0 ** -22 * pmax


# ------------------------------------------------------------------------------------------------ 4. the kernel
@pytest.mark.parametrize('n', [3, 4 * 257 + 3, 9_000_003], ids=['tail-only', '4k+3', 'grid-stride'])
@pytest.mark.parametrize('betas,wd', [((0.0, 0.9), 0.0), ((0.5, 0.999), 1e-4)], ids=['beta1=0', 'general'])
@pytest.mark.parametrize('decay', [0.9, 0.999])
def test_adam_flat_ema_against_its_definition(n, betas, wd, decay):
    """K = 6 launches, start_step = 2, beside s2e_adam_flat on clones: p, v (m on the general branch) bit-equal after every launch;
    ema == p exactly for steps 1..2, then within K * 2^-22 * max|p| of the fp64 recurrence over the kernel's own p sequence."""
    from seg2eye_amd import ops
    K, start = 6, 2
    gen = torch.Generator(device=DEV).manual_seed(n % 1000 + int(decay * 1000))
    p = torch.randn(n, device=DEV, generator=gen)
    m = torch.randn(n, device=DEV, generator=gen) * 0.01
    v = torch.rand(n, device=DEV, generator=gen) * 0.01
    ema = torch.full((n,), 7.0, device=DEV)                                 # (never read before the first averaging step)
    hyper = torch.tensor([1e-2, betas[0], betas[1], 1e-8, 0.0, 0.5, wd], dtype=torch.float32, device=DEV)
    ema_hyper = torch.tensor([decay, float(start)], dtype=torch.float32, device=DEV)
    p2, m2, v2, hyper2 = p.clone(), m.clone(), v.clone(), hyper.clone()
    m0 = m.clone()
    skips_m = betas[0] == 0.0 and wd == 0.0
    d32 = float(np.float32(decay))
    ref, pmax = None, 0.0
    for t in range(1, K + 1):
        g = torch.randn(n, device=DEV, generator=gen)
        ops.adam_flat_ema_step(p, g, m, v, ema, hyper, ema_hyper, skips_m=skips_m)
        ops.adam_flat_step(p2, g, m2, v2, hyper2, skips_m=skips_m)
        assert torch.equal(p, p2) and torch.equal(v, v2), 'step %d: p / v differ from s2e_adam_flat' % t
        assert torch.equal(m, m2), 'step %d: m differs from s2e_adam_flat' % t
        if skips_m:
            assert torch.equal(m, m0)                                       # (that branch never touches m)
        assert float(hyper[4]) == t == float(hyper2[4])
        pmax = max(pmax, float(p.abs().max()))
        if t <= start:
            assert torch.equal(ema, p), 'step %d <= start_step: the average must be a copy' % t
            ref = p.double()
        else:
            ref = d32 * ref + (1.0 - d32) * p.double()
            err = float((ema.double() - ref).abs().max())
            print('n %d decay %g step %d: |ema - fp64 recurrence| max %.3e (bound %.3e)' % (n, decay, t, err, _ema_bound(K, pmax)))
            assert err <= _ema_bound(K, pmax), (t, err, _ema_bound(K, pmax))
    assert not torch.equal(ema, p)


# ------------------------------------------------------------------------------------------------ 5. the trainer's average
@pytest.mark.parametrize('graphs', [False, True], ids=['eager', 'hip_graphs'])
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_trainer_keeps_the_average(dtype, graphs):
    from seg2eye_amd.pix2pix_trainer import Pix2PixTrainer
    K, decay = 5, 0.9
    tr = Pix2PixTrainer(_opt(ngf=8, ndf=8, crop_size=256, aspect_ratio=1.0, batchSize=2, compute_dtype=dtype, hip_graphs=graphs,
                             ema_decay=decay))
    og = tr.optimizer_G
    assert og.has_ema and not tr.optimizer_D.has_ema                        # only netG + netE are averaged
    assert torch.equal(og.flat_ema, og.flat_p)
    d32 = float(np.float32(decay))
    ref, pmax = og.flat_p.double().clone(), float(og.flat_p.abs().max())
    for i in range(K):
        data = _batch(2, 256, 256, seed=70 + i)
        tr.run_generator_one_step(dict(data))
        p_now = og.flat_p.clone()
        tr.run_discriminator_one_step(dict(data))
        ref = d32 * ref + (1.0 - d32) * p_now.double()
        pmax = max(pmax, float(p_now.abs().max()))
    torch.cuda.synchronize()
    assert tr.use_graphs == graphs                                          # (a failed capture would have fallen back to eager)
    k = og.numel_active
    err = float((og.flat_ema[:k].double() - ref[:k]).abs().max())
    print('%s %s: |flat_ema - fp64 recurrence| max %.3e (bound %.3e)' % (dtype, 'graphs' if graphs else 'eager', err, _ema_bound(K, pmax)))
    assert err <= _ema_bound(K, pmax)
    assert torch.equal(og.flat_ema[k:], og.flat_p[k:])                      # the never-updated tail (netE.fc_var)
    assert not torch.equal(og.flat_ema[:k], og.flat_p[:k])
    for q, e in zip(og.params, og.ema_views()):
        assert e.shape == q.shape and e.stride() == q.stride()


def test_trainer_without_ema_has_no_arena():
    from seg2eye_amd.pix2pix_trainer import Pix2PixTrainer
    tr = Pix2PixTrainer(_opt(ngf=8, ndf=8, crop_size=256, aspect_ratio=1.0, batchSize=2, compute_dtype='fp32', ema_decay=0))
    assert not tr.has_ema and not hasattr(tr.optimizer_G, 'flat_ema') and not hasattr(tr.optimizer_G, 'ema_hyper')
    with pytest.raises(RuntimeError):
        with tr.ema_scope():
            pass


# ------------------------------------------------------------------------------------------------ 6. ema_scope
def _volatile(tr):
    """Everything a pass could move outside the arenas: every bank's u|v arena, every BatchNorm buffer."""
    from seg2eye_amd.spectral import ensure_bank
    m = tr.pix2pix_model
    ts = [b.uv_arena for b in (ensure_bank(net) for net in (m.netG, m.netD, m.netE)) if b is not None]
    ts += [t for net in (m.netG, m.netD, m.netE) for mod in net.modules()
           if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm) and mod.track_running_stats
           for t in (mod.running_mean, mod.running_var, mod.num_batches_tracked)]
    return ts


def _eval_output(model, data):
    model.eval()
    with torch.no_grad():
        return model(dict(data), mode='inference').float().clone()


@pytest.mark.parametrize('norm_G', ['spectralspadeinstance3x3', 'spectralspadebatch3x3'])
def test_ema_scope_exchanges_and_restores(tmp_path, norm_G):
    """Inside the scope the generator computes what a model loaded from the saved `_ema` files computes, bit for bit (the eval
    forward has no float-atomic sums: the same presumption as the graph-versus-eager comparisons); afterwards flat_p, every
    u|v arena and every BatchNorm buffer are what they were -- also after a TRAIN-mode inference pass inside the scope."""
    from seg2eye_amd.pix2pix_model import Pix2PixModel
    from seg2eye_amd.pix2pix_trainer import Pix2PixTrainer
    kw = dict(ngf=8, ndf=8, crop_size=256, aspect_ratio=1.0, batchSize=2, compute_dtype='fp32', norm_G=norm_G,
              checkpoints_dir=str(tmp_path), name='scope')
    tr = Pix2PixTrainer(_opt(ema_decay=0.9, **kw))
    for i in range(3):
        data = _batch(2, 256, 256, seed=80 + i)
        tr.run_generator_one_step(dict(data))
        tr.run_discriminator_one_step(dict(data))
    tr.save('latest')
    fixed = _batch(2, 256, 256, seed=99)
    m, og = tr.pix2pix_model, tr.optimizer_G
    y_live = _eval_output(m, fixed)
    p0, e0 = og.flat_p.clone(), og.flat_ema.clone()
    vol = _volatile(tr)
    if 'batch' in norm_G:
        assert any(t.dtype == torch.long for t in vol)                     # (num_batches_tracked: the BatchNorm buffers are in the list)
    vol0 = [t.clone() for t in vol]
    with tr.ema_scope():
        assert torch.equal(og.flat_p, e0) and torch.equal(og.flat_ema, p0)
        y_ema = _eval_output(m, fixed)
        with pytest.raises(RuntimeError):
            tr.run_generator_one_step(dict(fixed))                          # (would train the averaged weights: refused)
        m.train()
        with torch.no_grad():
            m(dict(fixed), mode='inference')                                # moves u|v and the running statistics
        assert any(not torch.equal(a, b) for a, b in zip(vol, vol0))
    assert torch.equal(og.flat_p, p0) and torch.equal(og.flat_ema, e0)
    for a, b in zip(vol, vol0):
        assert torch.equal(a, b)
    assert torch.equal(_eval_output(m, fixed), y_live)
    assert not torch.equal(y_ema, y_live)
    # a second model, netG / netE loaded from the _ema files by the ordinary load path (test.py --use_ema)
    other = Pix2PixModel(_opt(isTrain=False, use_ema=True, **kw))
    y_plain = _eval_output(other, fixed)
    # No forward kernel sums with float atomics, but sigma's reduction (s2e_sn_power_iteration, csrc/spectral.hip) forms float
    # partial sums along W's MEMORY order, and a model outside an optimizer keeps torch's (Cout, Cin, KH, KW) order where the
    # trainer's arena stores channels-last slices: measured, sigma differs in its last bit (1.9e-9) and the image by 8e-8.  So the
    # bit comparison is made with the loaded weights laid out as the trainer's are -- in a FlatAdam arena, which moves values
    # and changes none --, and the plain layout is held to the README's fp32 parity bound.
    other.create_optimizers(other.opt)
    y_other = _eval_output(other, fixed)
    print('%s: |ema-scope output - output from the _ema files| max %.3e (same layout), %.3e (torch layout); |ema - live| max %.3e'
          % (norm_G, float((y_ema - y_other).abs().max()), float((y_ema - y_plain).abs().max()), float((y_ema - y_live).abs().max())))
    assert torch.equal(y_ema, y_other)
    assert float((y_ema - y_plain).abs().max()) < 1e-3


def test_ema_scope_leaves_no_trace_in_training():
    """S2E_DETERMINISTIC=1 (read when the library loads: one fresh child process, its own time limit): after a scope with an eval
    and a TRAIN-mode pass inside, one more training step gives the same arenas as a twin trainer that never entered it."""
    e = dict(os.environ, S2E_DETERMINISTIC='1')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_ema_child.py')], env=e, capture_output=True, text=True,
                       timeout=420, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0 and 'ema child ok' in r.stdout, (r.stdout[-4000:], r.stderr[-4000:])


# ------------------------------------------------------------------------------------------------ 7. checkpoints through the CLI
def _files(d):
    return {f for f in os.listdir(d) if os.path.isfile(os.path.join(d, f))}


def test_ema_checkpoints_through_the_cli(tmp_path, capsys):
    import train as train_mod
    import test as test_mod
    from seg2eye_amd.options import parse
    from seg2eye_amd.pix2pix_trainer import Pix2PixTrainer
    ckdir = tmp_path / 'ck'
    common = ['--checkpoints_dir', str(ckdir), '--ngf', '8', '--ndf', '8', '--batchSize', '2', '--aspect_ratio', '1.0',
              '--synthetic_size', '4', '--compute_dtype', 'fp32']
    train_args = ['--niter', '1', '--niter_decay', '1', '--lr', '0.001', '--display_freq', '4', '--validation_limit', '2']
    tr = train_mod.main(['--name', 'ema'] + common + train_args + ['--ema_decay', '0.9'])
    out = capsys.readouterr().out
    assert 'validating the averaged weights' in out
    ck = ckdir / 'ema'
    plain = {'%s_net_%s.pth' % (ep, lab) for ep in ('latest', '1', '2') for lab in 'GDE'} | {'iter.txt'}
    extra = {'%s_net_%s_ema.pth' % (ep, lab) for ep in ('latest', '1', '2') for lab in 'GE'}
    assert _files(ck) == plain | extra
    m, og = tr.pix2pix_model, tr.optimizer_G
    ema_of = {id(q): e for q, e in zip(og.params, og.ema_views())}
    saved = {}
    for lab, net in (('G', m.netG), ('E', m.netE)):
        for ep in ('latest', '2'):
            sd, sd_ema = torch.load(ck / ('%s_net_%s.pth' % (ep, lab))), torch.load(ck / ('%s_net_%s_ema.pth' % (ep, lab)))
            assert list(sd) == list(sd_ema)
            for k in sd:
                assert sd[k].shape == sd_ema[k].shape and sd[k].dtype == sd_ema[k].dtype, k
        saved[lab] = sd_ema = torch.load(ck / ('latest_net_%s_ema.pth' % lab))
        named = dict(net.named_parameters())
        live = net.state_dict()
        differs = False
        for k, t in sd_ema.items():
            if k in named:
                assert torch.equal(t, ema_of[id(named[k])].detach().cpu()), k
                differs |= not torch.equal(t, named[k].detach().cpu())
            else:
                assert torch.equal(t, live[k].detach().cpu()), k             # buffers: the live ones
        assert differs
    # --continue_train restores the average from the files ...
    tr2 = Pix2PixTrainer(parse(['--name', 'ema'] + common + ['--continue_train', '--ema_decay', '0.9']))
    m2, og2 = tr2.pix2pix_model, tr2.optimizer_G
    ema2 = {id(q): e for q, e in zip(og2.params, og2.ema_views())}
    for lab, net in (('G', m2.netG), ('E', m2.netE)):
        for k, q in net.named_parameters():
            assert torch.equal(ema2[id(q)].detach().cpu(), saved[lab][k]), k
    assert not torch.equal(og2.flat_ema, og2.flat_p)
    assert 'no averaged checkpoint' not in capsys.readouterr().out
    # ... and, without them, restarts it from the live weights and says so
    gone = ckdir / 'ema_gone'
    shutil.copytree(ck, gone)
    for f in extra:
        os.remove(gone / f)
    tr3 = Pix2PixTrainer(parse(['--name', 'ema_gone'] + common + ['--continue_train', '--ema_decay', '0.9']))
    assert torch.equal(tr3.optimizer_G.flat_ema, tr3.optimizer_G.flat_p)
    assert 'no averaged checkpoint' in capsys.readouterr().out
    # a run without --ema_decay writes exactly the plain file set
    train_mod.main(['--name', 'plain'] + common + train_args)
    assert _files(ckdir / 'plain') == plain
    assert 'averaged' not in capsys.readouterr().out
    # test.py --use_ema == test.py on a directory where the _ema files were renamed over the plain ones; != the live weights
    renamed = ckdir / 'ema_renamed'
    shutil.copytree(ck, renamed)
    for lab in 'GE':
        os.replace(renamed / ('latest_net_%s_ema.pth' % lab), renamed / ('latest_net_%s.pth' % lab))
    targs = common + ['--produce_npy']

    def predictions(name, *more):
        paths = test_mod.main(['--name', name, '--results_dir', 'res' + ''.join(more).replace('--', '_')] + targs + list(more))
        assert len(paths) == 4
        return {os.path.basename(p): np.load(p) for p in paths}
    with_ema, live, from_renamed = predictions('ema', '--use_ema'), predictions('ema'), predictions('ema_renamed')
    assert sorted(with_ema) == sorted(live) == sorted(from_renamed)
    assert all(np.array_equal(with_ema[k], from_renamed[k]) for k in with_ema)
    assert any(not np.array_equal(with_ema[k], live[k]) for k in with_ema)
    with pytest.raises(FileNotFoundError, match='latest_net_G_ema.pth'):
        test_mod.main(['--name', 'plain', '--use_ema'] + targs)
