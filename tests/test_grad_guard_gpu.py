"""The gradient guard on the GPU: s2e_grad_guard against its definition, the guarded Adam launches beside s2e_adam_flat (a coefficient of
1 is free, a clipped step is the unguarded step at grad_scale * c, a skipped step changes nothing), optim.FlatAdam against
clip_grad_norm_ + torch.optim.Adam in fp64, the trainer on a corrupt frame (eager and hipGraphs) and train.py's progress line.

The bound on the norm (tests 5, 6, 8) is derived, not measured: squares and sum are fp64, whose error over n terms is at most
n * 2^-53 relative -- 1e-9 at the largest n here, far below fp32's 2^-24 -- so what remains is the ONE rounding of the result to fp32
(half an ulp) and the reference's own; two fp32 ulps, rtol 2.4e-7, cover both.  The reference is numpy's fp64 sum over the same fp32
values."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [3, 4 * 257 + 3, 9_000_003]                  # tail only, body + tail, a size the grid strides over (test_ema_gpu's three)
SIZE_IDS = ['tail-only', '4k+3', 'grid-stride']
SCALE = 0.5                                          # grad_scale (hyper[5])
RTOL = 2.4e-7                                        # two fp32 ulps
BRANCHES = [((0.0, 0.9), 0.0), ((0.5, 0.999), 1e-4)]
BRANCH_IDS = ['beta1=0', 'general']
INF, NAN = float('inf'), float('nan')


@functools.lru_cache(maxsize=None)
def _arena(n):
    """(g ~ N(0,1) on the device, its norm 0.5 * sqrt(sum g^2) in fp64 by numpy from the same fp32 values): computed once per size,
    shared by the tests and never written."""
    g = torch.randn(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(n % 1000))
    return g, _norm_of(g)


def _norm_of(g):
    return SCALE * float(np.sqrt(np.sum(g.cpu().numpy().astype(np.float64) ** 2)))


def _hyper(betas=(0.0, 0.9), wd=0.0, steps=0.0):
    return torch.tensor([1e-2, betas[0], betas[1], 1e-8, steps, SCALE, wd], dtype=torch.float32, device=DEV)


class _Guard:
    """A guard record, its first_bad word and the workspace for an arena of n elements."""

    def __init__(self, n, max_norm=0.0, skip=0.0):
        from seg2eye_amd import ops
        self.rec = torch.tensor([max_norm, skip, 0, 0, 0, 0, 0, 0], dtype=torch.float32, device=DEV)
        self.first_bad = torch.full((1,), -7, dtype=torch.int32, device=DEV)
        self.ws = ops.grad_guard_workspace(n, DEV)

    def run(self, g, hyper):
        from seg2eye_amd import ops
        ops.grad_guard(g, hyper, self.rec, self.first_bad, self.ws)
        return self.rec.tolist(), int(self.first_bad)

    def bits(self):
        return torch.cat([self.rec.view(torch.int32), self.first_bad]).clone(), self.ws.clone().view(torch.int64)


def _state(n, seed, ema):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    p = torch.randn(n, device=DEV, generator=gen)
    m = torch.randn(n, device=DEV, generator=gen) * 0.01
    v = torch.rand(n, device=DEV, generator=gen) * 0.01
    e = torch.randn(n, device=DEV, generator=gen) if ema else None
    return p, m, v, e


EMA_HYPER = (0.9, 1.0)                               # {decay, start_step}: the second step on averages


def _step(guard, p, g, m, v, e, hyper, skips_m):
    """One Adam launch: guarded when `guard` is a record, s2e_adam_flat / s2e_adam_flat_ema otherwise."""
    from seg2eye_amd import ops
    eh = torch.tensor(EMA_HYPER, dtype=torch.float32, device=DEV)
    if guard is None:
        if e is None:
            ops.adam_flat_step(p, g, m, v, hyper, skips_m=skips_m)
        else:
            ops.adam_flat_ema_step(p, g, m, v, e, hyper, eh, skips_m=skips_m)
    elif e is None:
        ops.adam_flat_guarded_step(p, g, m, v, hyper, guard, skips_m=skips_m)
    else:
        ops.adam_flat_ema_guarded_step(p, g, m, v, e, hyper, eh, guard, skips_m=skips_m)


def _clones(*ts):
    return [None if t is None else t.clone() for t in ts]


def _same(a, b):
    return all(x is None or torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ 5. the reduction
@pytest.mark.parametrize('n', SIZES, ids=SIZE_IDS)
def test_grad_guard_against_its_definition(n):
    g, ref = _arena(n)
    gd = _Guard(n)
    rec, fb = gd.run(g, _hyper())
    print('n %d: norm %.9g, fp64 reference %.9g, relative difference %.3e (bound %.1e)' % (n, rec[2], ref, abs(rec[2] - ref) / ref, RTOL))
    assert abs(rec[2] - ref) <= RTOL * ref
    assert fb == -1 and rec[3] == 1.0 and rec[4:] == [0.0, 0.0, 0.0, 0.0] and rec[:2] == [0.0, 0.0]
    first = gd.bits()
    gd.run(g, _hyper())
    second = gd.bits()
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])    # record and per-block partials: the same bits
    # the sign of grad_scale does not enter the norm
    hy = _hyper()
    hy[5] = -SCALE
    assert gd.run(g, hy)[0][2] == rec[2]


# ------------------------------------------------------------------------------------------------ 6. finite but large
@pytest.mark.parametrize('n', SIZES, ids=SIZE_IDS)
def test_grad_guard_finite_but_large(n):
    """3e19 squared overflows fp32 (9e38 > 3.4e38): the element is finite, the step is not skipped and the norm is exact."""
    g = _arena(n)[0].clone()
    g[n // 2] = 3e19
    assert not torch.isfinite(g[n // 2] * g[n // 2])
    ref = _norm_of(g)
    gd = _Guard(n, max_norm=0.0, skip=1.0)
    rec, fb = gd.run(g, _hyper())
    print('n %d: norm %.9g, fp64 reference %.9g, relative difference %.3e' % (n, rec[2], ref, abs(rec[2] - ref) / ref))
    assert fb == -1 and rec[3] == 1.0 and rec[4] == 0.0 and rec[6] == 0.0
    assert np.isfinite(rec[2]) and abs(rec[2] - ref) <= RTOL * ref


# ------------------------------------------------------------------------------------------------ 7. c == 1 is free
@pytest.mark.parametrize('n', SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize('betas,wd', BRANCHES, ids=BRANCH_IDS)
@pytest.mark.parametrize('ema', [False, True], ids=['plain', 'ema'])
@pytest.mark.parametrize('setting', ['max_norm=4*norm', 'skip-only'])
def test_coefficient_one_is_free(setting, ema, betas, wd, n):
    g, norm = _arena(n)
    gd = _Guard(n, max_norm=4.0 * norm, skip=0.0) if setting == 'max_norm=4*norm' else _Guard(n, max_norm=0.0, skip=1.0)
    skips_m = betas[0] == 0.0 and wd == 0.0
    a = _state(n, 3, ema)
    b = _clones(*a)
    ha, hb = _hyper(betas, wd), _hyper(betas, wd)
    for t in range(1, 4):
        rec, fb = gd.run(g, ha)
        assert rec[3] == 1.0 and fb == -1 and rec[4:7] == [0.0, 0.0, 0.0]
        _step(gd.rec, a[0], g, a[1], a[2], a[3], ha, skips_m)
        _step(None, b[0], g, b[1], b[2], b[3], hb, skips_m)
        assert _same(a, b), 'step %d: p / m / v / ema differ from the unguarded launch' % t
        assert float(ha[4]) == t == float(hb[4])


# ------------------------------------------------------------------------------------------------ 8. clipping
@pytest.mark.parametrize('n', SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize('betas,wd', BRANCHES, ids=BRANCH_IDS)
def test_clipped_step_is_the_unguarded_step_at_the_clipped_scale(betas, wd, n):
    g, norm = _arena(n)
    max_norm = float(np.float32(norm / 4.0))
    gd = _Guard(n, max_norm=max_norm, skip=1.0)
    skips_m = betas[0] == 0.0 and wd == 0.0
    a = _state(n, 4, False)
    b = _clones(*a)
    ha, hb = _hyper(betas, wd), _hyper(betas, wd)
    rec, fb = gd.run(g, ha)
    want = min(1.0, max_norm / (norm + 1e-6))
    print('n %d: c %.9g, fp64 formula %.9g, relative difference %.3e' % (n, rec[3], want, abs(rec[3] - want) / want))
    assert abs(rec[3] - want) <= RTOL * want and rec[3] < 1.0
    assert fb == -1 and rec[4] == 0.0 and rec[5] == 1.0 and rec[6] == 0.0           # counted as clipped, not as skipped
    hb[5:6] = hb[5:6] * gd.rec[3:4]                                                # fl32(0.5 * c), c read back from the record
    _step(gd.rec, a[0], g, a[1], a[2], None, ha, skips_m)
    _step(None, b[0], g, b[1], b[2], None, hb, skips_m)
    assert _same(a, b) and float(ha[4]) == 1.0
    assert float(ha[5]) == SCALE                                                   # (the launch does not write grad_scale)
    p0 = _state(n, 4, False)[0]
    assert not torch.equal(a[0], p0)
    gd.run(g, ha)
    assert gd.rec[5].item() == 2.0


# ------------------------------------------------------------------------------------------------ 9. skipping
N_BIG = SIZES[2]
PLACEMENTS = [(3, {0: INF}), (SIZES[1], {0: INF}), (N_BIG, {0: INF}),
              (3, {2: NAN}), (SIZES[1], {SIZES[1] - 1: NAN}), (N_BIG, {N_BIG - 1: NAN}),          # (the scalar tail)
              (N_BIG, {5_000_001: -INF}),                                                      # a block's second sweep
              (3, {1: NAN, 2: INF}), (SIZES[1], {700: INF, 1030: NAN}), (N_BIG, {5_000_001: -INF, 4_200_000: NAN, N_BIG - 2: INF})]


@pytest.mark.parametrize('n,bad', PLACEMENTS, ids=['%d:%s' % (n, ','.join('%s@%d' % (v, k) for k, v in b.items())) for n, b in PLACEMENTS])
@pytest.mark.parametrize('betas,wd', BRANCHES, ids=BRANCH_IDS)
@pytest.mark.parametrize('ema', [False, True], ids=['plain', 'ema'])
def test_skipped_step_changes_nothing(ema, betas, wd, n, bad):
    g = _arena(n)[0].clone()
    for k, val in bad.items():
        g[k] = val
    gd = _Guard(n, max_norm=1.0, skip=1.0)
    skips_m = betas[0] == 0.0 and wd == 0.0
    a = _state(n, 5, ema)
    before = _clones(*a)
    hy = _hyper(betas, wd, steps=2.0)                                              # (past the average's start_step: it would average)
    rec, fb = gd.run(g, hy)
    assert rec[3] == 0.0 and fb == min(bad) and rec[4] == 1.0 and rec[5] == 0.0 and rec[6] == 1.0
    _step(gd.rec, a[0], g, a[1], a[2], a[3], hy, skips_m)
    assert _same(a, before), 'a skipped step wrote p, m, v or ema'
    assert float(hy[4]) == 2.0
    assert np.isfinite(rec[2])                                                     # the norm of the finite elements


def test_skip_counters_over_a_run():
    """Five steps of one optimizer, steps 2 and 3 carrying a non-finite gradient."""
    from seg2eye_amd.optim import FlatAdam
    n = SIZES[1]
    q = torch.nn.Parameter(torch.randn(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9)))
    opt = FlatAdam([q], lr=1e-3, betas=(0.0, 0.9), skip_nonfinite=True)
    assert opt.has_guard and opt.clip_norm == 0.0
    g = _arena(n)[0]
    seen = []
    for t in range(1, 6):
        opt.zero_grad()
        q.grad.copy_(g)
        if t == 2:
            q.grad[n - 1] = NAN
        if t == 3:
            q.grad[17] = INF
        before = opt.flat_p.clone()
        opt.step(grad_scale=SCALE)
        st = opt.guard_stats()
        seen.append((st['consecutive'], st['skipped'], st['first_bad'], st['coef']))
        assert torch.equal(opt.flat_p, before) == (t in (2, 3))
    assert seen == [(0, 0, -1, 1.0), (1, 1, n - 1, 0.0), (2, 2, 17, 0.0), (0, 2, -1, 1.0), (0, 2, -1, 1.0)]
    assert opt.step_count == 3 and float(opt.hyper[4]) == 3.0                      # the clean steps
    assert opt.state_dict()['step'] == 3


# ------------------------------------------------------------------------------------------------ 10. FlatAdam against torch
@pytest.mark.parametrize('beta1', [0.0, 0.5])
def test_flat_adam_guard_matches_clip_grad_norm_and_torch_adam(beta1):
    """Three parameters (a conv weight stored channels-last behind an alignment gap), clip_norm 17 with gradients on either side of
    it, grad_scale 0.5, five steps, step 3 carrying an inf: against clip_grad_norm_ + torch.optim.Adam in fp64 on the CPU, which skips
    step 3 by hand.  Tolerances: test_adam_flat_matches_torch's."""
    from seg2eye_amd.optim import FlatAdam, _arena_view
    shapes = [(7,), (16, 8, 3, 3), (6, 5)]                                          # 1189 elements: |N(0,1)| * 0.5 has norm ~17.2
    gen = torch.Generator().manual_seed(21)
    init = [torch.randn(*s, generator=gen) for s in shapes]
    ref = [torch.nn.Parameter(t.double().clone()) for t in init]
    ropt = torch.optim.Adam(ref, lr=1e-3, betas=(beta1, 0.9), eps=1e-8)
    mine = [torch.nn.Parameter(t.to(DEV).clone()) for t in init]
    fa = FlatAdam(mine, lr=1e-3, betas=(beta1, 0.9), clip_norm=17.0, skip_nonfinite=True)
    assert fa.cl == [False, True, False] and fa.offsets[1] == 64                    # the gap: elements 8 .. 63
    clipped = 0
    for step, amp in enumerate([0.3, 3.0, 1.0, 0.5, 2.0], start=1):
        gs = [torch.randn(*s, generator=gen) * amp for s in shapes]
        if step == 3:
            gs[1][5, 3, 1, 2] = INF
        fa.zero_grad()
        for q, g in zip(mine, gs):
            q.grad.copy_(g.to(DEV))
        fa.step(grad_scale=SCALE)
        st = fa.guard_stats()
        if step == 3:
            assert st['coef'] == 0.0 and fa.params[fa.param_at(st['first_bad'])] is mine[1]
            sd = fa.state_dict()
            assert sd['m_valid'] is (beta1 != 0.0)                                  # beta1 == 0: m would be formed from a gradient no step consumed
            assert sd['step'] == 2
            continue                                                                # the reference skips by hand
        for r, g in zip(ref, gs):
            r.grad = g.double() * SCALE
        total = float(torch.nn.utils.clip_grad_norm_(ref, 17.0))
        clipped += total > 17.0
        ropt.step()
        assert abs(st['norm'] - total) <= 1e-6 * total and (st['coef'] < 1.0) == (total > 17.0)
    assert clipped == 2 and st['clipped'] == 2 and st['skipped'] == 1 and fa.step_count == 4
    sd = fa.state_dict()
    assert sd['m_valid'] is True and sd['step'] == 4
    for i, (q, r) in enumerate(zip(mine, ref)):
        state = ropt.state[r]
        np.testing.assert_allclose(q.detach().cpu().numpy(), r.detach().numpy(), rtol=1e-5, atol=1e-6)
        v = _arena_view(sd['v'], fa.offsets[i], q, fa.cl[i]).cpu().numpy()
        m = _arena_view(sd['m'], fa.offsets[i], q, fa.cl[i]).cpu().numpy()
        np.testing.assert_allclose(v, state['exp_avg_sq'].numpy(), rtol=1e-5, atol=1e-12)
        np.testing.assert_allclose(m, state['exp_avg'].numpy(), rtol=1e-5, atol=1e-7)


def test_changed_clip_norm_reaches_the_device():
    from seg2eye_amd.optim import FlatAdam
    q = torch.nn.Parameter(torch.ones(8, device=DEV))
    fa = FlatAdam([q], lr=1e-3, betas=(0.0, 0.9), clip_norm=1.0)
    q.grad.fill_(1.0)
    fa.step()
    assert fa.guard_stats()['coef'] < 0.5                                           # norm sqrt(8)
    fa.clip_norm = 100.0
    fa.step()
    st = fa.guard_stats()
    assert st['coef'] == 1.0 and st['clipped'] == 1 and float(fa.guard[0]) == 100.0


# ------------------------------------------------------------------------------------------------ 11. the trainer
def _opt(**kw):
    from seg2eye_amd.options import default_opt
    kw.setdefault('gpu_ids', [0])
    return default_opt(ngf=8, ndf=8, crop_size=256, aspect_ratio=1.0, batchSize=2, compute_dtype='fp32', **kw)


def _batch(seed, corrupt=False):
    from seg2eye_amd import synthetic as syn
    b = syn.make_batch(2, 256, 256, seed=seed)
    data = {'label': torch.from_numpy(b['label']), 'style_image': torch.from_numpy(b['style_image']),
            'target': torch.from_numpy(b['target']).clone(), 'filename': b['filename']}
    if corrupt:
        data['target'][1, 0, 100, 37] = INF                                         # one pixel of a corrupt frame
    return data


def _iteration(tr, data):
    tr.run_generator_one_step(dict(data))
    tr.run_discriminator_one_step(dict(data))
    torch.cuda.synchronize()


def _all_finite(tr):
    return all(bool(torch.isfinite(o.flat_p).all()) for o in (tr.optimizer_G, tr.optimizer_D))


@pytest.mark.parametrize('graphs', [False, True], ids=['eager', 'hip_graphs'])
def test_trainer_survives_a_corrupt_frame(graphs):
    from seg2eye_amd.pix2pix_trainer import Pix2PixTrainer
    tr = Pix2PixTrainer(_opt(hip_graphs=graphs, skip_nonfinite_grads=True, ema_decay=0.9))
    og, od = tr.optimizer_G, tr.optimizer_D
    assert tr.has_guard and og.has_guard and od.has_guard and og.has_ema
    _iteration(tr, _batch(31))
    h = tr.grad_health()
    assert [h[k]['skipped'] for k in 'GD'] == [0, 0] and og.step_count == od.step_count == 1
    arenas = [og.flat_p, og.flat_v, og.flat_ema, od.flat_p, od.flat_v, og.hyper[4:5], od.hyper[4:5]]
    before = [t.clone() for t in arenas]
    _iteration(tr, _batch(32, corrupt=True))
    h = tr.grad_health()
    print('after the corrupt frame:', h)
    m = tr.pix2pix_model
    names = {'%s.%s' % (tag, k) for tag, net in (('netG', m.netG), ('netE', m.netE), ('netD', m.netD)) for k, _ in net.named_parameters()}
    for k in 'GD':
        assert h[k]['skipped'] == 1 and h[k]['consecutive'] == 1 and h[k]['coef'] == 0.0 and h[k]['first_bad'] >= 0, (k, h[k])
        assert h[k]['param'] in names, (k, h[k])
    assert h['G']['param'].startswith(('netG.', 'netE.')) and h['D']['param'].startswith('netD.')
    for t, t0 in zip(arenas, before):
        assert torch.equal(t, t0)
    assert og.step_count == od.step_count == 1
    _iteration(tr, _batch(31))
    h = tr.grad_health()
    assert [h[k]['consecutive'] for k in 'GD'] == [0, 0] and [h[k]['skipped'] for k in 'GD'] == [1, 1]
    assert og.step_count == od.step_count == 2 and float(og.hyper[4]) == float(od.hyper[4]) == 2.0
    assert not torch.equal(og.flat_p, before[0]) and not torch.equal(od.flat_p, before[3])
    assert _all_finite(tr) and bool(torch.isfinite(og.flat_ema).all())
    assert tr.use_graphs == graphs                                                  # (a failed capture would have fallen back to eager)

    # the same sequence without the flag: today's behaviour, and the reason for the feature
    bare = Pix2PixTrainer(_opt(hip_graphs=graphs, ema_decay=0.9))
    assert not bare.has_guard
    with pytest.raises(RuntimeError):
        bare.grad_health()
    for data in (_batch(31), _batch(32, corrupt=True), _batch(31)):
        _iteration(bare, data)
    assert not _all_finite(bare)


# ------------------------------------------------------------------------------------------------ 12. train.py end to end
def test_train_cli_reports_the_guard(tmp_path):
    args = ['--name', 'guard', '--checkpoints_dir', str(tmp_path), '--ngf', '8', '--ndf', '8', '--batchSize', '2', '--aspect_ratio', '1.0',
            '--synthetic_size', '6', '--compute_dtype', 'fp32', '--niter', '1', '--niter_decay', '0', '--lr', '0.001',
            '--grad_clip_norm', '1.0', '--skip_nonfinite_grads', '--print_freq', '2']
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py')] + args, capture_output=True, text=True, timeout=300, cwd=ROOT)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('(epoch:')]
    assert len(lines) == 3                                                          # one per batch
    for ln in lines:
        for key in ('grad_norm/G: ', 'grad_norm/D: ', 'grad_skipped/G: 0.000', 'grad_skipped/D: 0.000'):
            assert key in ln, (key, ln)
    assert 'Training was successfully finished.' in r.stdout
    for lab in 'GDE':
        sd = torch.load(tmp_path / 'guard' / ('latest_net_%s.pth' % lab))
        assert sd and all(bool(torch.isfinite(t.float()).all()) for t in sd.values()), lab


# ------------------------------------------------------------------------------------------------ the loss mode behind test 11's G skip
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('accumulate', [0, 1])
def test_l1_nangrad_is_l1_except_for_a_nan_difference(dtype, accumulate):
    """S2E_LOSS_L1 keeps torch's gradient (sign(a - b), and torch's sign(NaN) is 0); S2E_LOSS_L1_NANGRAD -- what the feature tap uses
    under --skip_nonfinite_grads -- gives NaN exactly where a - b is NaN and S2E_LOSS_L1's bits everywhere else (an infinite
    difference has a sign).  n = 4 * 257 + 3: vector body and scalar tail."""
    from seg2eye_amd import _lib as L
    n = 4 * 257 + 3
    gen = torch.Generator(device=DEV).manual_seed(5)
    a = torch.randn(n, device=DEV, generator=gen).to(dtype)
    b = torch.randn(n, device=DEV, generator=gen).to(dtype)
    b[7] = a[7]                                                                     # a tie: gradient 0 in both modes
    nan_at, inf_at = [3, 600, n - 1], [11, n - 2]                                   # (body and tail)
    b[nan_at] = NAN
    b[inf_at[0]], a[inf_at[1]] = INF, INF
    base = torch.randn(n, device=DEV, generator=gen).to(dtype)
    scale = 0.25
    da = {}
    for mode in (L.LOSS_L1, L.LOSS_L1_NANGRAD):
        out = base.clone()
        L.check(L.lib().s2e_loss_grad(1 if dtype == torch.bfloat16 else 0, mode, a.data_ptr(), b.data_ptr(), n, scale, None, out.data_ptr(),
                                      accumulate, None), 's2e_loss_grad')
        da[mode] = out.float().cpu()
    torch.cuda.synchronize()
    want = scale * torch.sign(a.float() - b.float()).cpu()                          # torch: 0 at a NaN difference
    assert bool((want[nan_at] == 0).all())
    if accumulate:
        want = (want + base.float().cpu()).to(dtype).float()
    assert torch.equal(da[L.LOSS_L1], want)
    keep = torch.ones(n, dtype=torch.bool)
    keep[nan_at] = False
    assert torch.equal(da[L.LOSS_L1_NANGRAD][keep], da[L.LOSS_L1][keep])
    assert bool(torch.isnan(da[L.LOSS_L1_NANGRAD][nan_at]).all()) and bool(torch.isfinite(da[L.LOSS_L1][nan_at]).all())
