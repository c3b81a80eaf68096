"""Differentiable augmentation of the discriminator's input on the GPU: ops.d_input_aug and its backward against the fp64
restatement of tests/_diffaug_ref.py (whose backward is autograd's), element by element, and the trainer under --diffaug.

Bounds (derived, not measured).  Forward: the image channel is ONE rounding to the output dtype of an fp32 multiply-add c * v + o.
bf16: 2^-9 relative for that rounding, doubled to 2^-8 because the fp32 rounding of o may put the sum on the other side of a bf16 tie;
the fp32 arithmetic itself (values bounded by 4.5: a handful of roundings of 2^-24 relative stay under 3e-6) is covered by the absolute
1e-5, which alone is the fp32 bound.  Backward: c * G + k rounded once (2^-8 |ref| as above); k = (1 - c) / (H W) * S with S summed
in fp64, so its error is its one fp32 rounding, below eps32 * max|G| * |1 - c| <= 3e-8 max|G|: 1e-6 max|G| covers it.  Every input is a
bf16 value, so one fp64 reference serves both dtypes.  One-hot, pad and invisible values, a c = 1, b = 0 image channel and anything
under a policy without colour are compared exactly."""
import functools
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT
import _diffaug_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FULL = 'color,translation,cutout'
SHAPES = [(3, 19, 23), (3, 24, 40), (2, 16, 16)]         # odd, non-square, pixel counts that are no multiple of a block, N = 2 and 3
SHAPE_IDS = ['3x19x23', '3x24x40', '2x16x16']
DTYPES = [torch.bfloat16, torch.float32]
DTYPE_IDS = ['bf16', 'fp32']
NCLS, CPAD = 4, 8


def _rows(H, W):
    """The hand-written rows: name -> [b, c, ty, tx, y0, x0, ch, cw]."""
    rh, rw = int(H / 8 + 0.5), int(W / 8 + 0.5)
    ch, cw = H // 2, W // 2
    return {
        'identity': [0, 1, 0, 0, 0, 0, 0, 0],
        'shift++': [0, 1, rh, rw, 0, 0, 0, 0], 'shift--': [0, 1, -rh, -rw, 0, 0, 0, 0],
        'shift+-': [0, 1, rh, -rw, 0, 0, 0, 0], 'shift-+': [0, 1, -rh, rw, 0, 0, 0, 0],
        'cut-top-left': [0, 1, 0, 0, -(ch // 2), -(cw // 2), ch, cw],            # hangs over the top-left corner
        'cut-bottom-right': [0, 1, 0, 0, H - ch // 2, W - cw // 2, ch, cw],      # hangs over the bottom-right edge
        'c=0.5': [0, 0.5, 0, 0, 0, 0, 0, 0], 'c=1.5': [0, 1.5, 0, 0, 0, 0, 0, 0],
        'b=+0.5': [0.5, 1, 0, 0, 0, 0, 0, 0], 'b=-0.5': [-0.5, 1, 0, 0, 0, 0, 0, 0],
        'everything': [0.3125, 0.75, rh, -rw, H - ch - 2, -3, ch, cw],
    }


def _row_sets(n, H, W):
    """Every hand-written row in some batch of n, plus the all-identity batch."""
    rows = list(_rows(H, W).values())
    rows += rows[:(-len(rows)) % n]
    return [[list(map(float, _rows(H, W)['identity']))] * n] + [[list(map(float, r)) for r in rows[i:i + n]] for i in range(0, len(rows), n)]


@functools.lru_cache(maxsize=None)
def _inputs(n, H, W):
    """label, fake, real, upstream gradient: CPU, bf16-representable values in fp64; computed once per shape, never written."""
    gen = torch.Generator().manual_seed(1000 * n + 31 * H + W)
    label = torch.randint(0, NCLS, (n, H, W), generator=gen, dtype=torch.uint8)
    fake = (torch.rand(n, H, W, generator=gen) * 2 - 1).bfloat16().double()
    real = (torch.rand(n, H, W, generator=gen) * 2 - 1).bfloat16().double()
    fake[0, 0, 0], fake[0, 1, 2] = -0.0, 0.0                                        # both zeros: a copy keeps the sign
    G = torch.randn(2 * n, H, W, CPAD, generator=gen).bfloat16().double()
    return label, fake, real, G


@functools.lru_cache(maxsize=None)
def _reference(n, H, W, set_index, color):
    """(out, d fake) of the fp64 restatement for one row set, by autograd; shared by both dtypes."""
    label, fake, real, G = _inputs(n, H, W)
    f = fake.clone().requires_grad_(True)
    out = R.d_input_aug_ref(label.long(), f, real, _row_sets(n, H, W)[set_index], NCLS, CPAD, color=color)
    out.backward(G)
    return out.detach(), f.grad.detach()


def _run(n, H, W, rows, dtype, color, grad=True):
    from seg2eye_amd import ops
    label, fake, real, G = _inputs(n, H, W)
    f = fake.to(DEV, dtype).view(n, 1, H, W).requires_grad_(grad)
    out = ops.d_input_aug(label.to(DEV), f, real.to(DEV, dtype).view(n, 1, H, W), torch.tensor(rows, dtype=torch.float32, device=DEV),
                          NCLS, CPAD, color=color)
    if grad:
        out.backward(G.to(DEV, dtype))
    return out.detach(), (f.grad.view(n, H, W) if grad else None)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ------------------------------------------------------------------------------------------------ the op
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
def test_forward_and_backward_match_the_restatement(shape, dtype):
    n, H, W = shape
    label, fake, real, G = _inputs(n, H, W)
    rel = 2.0 ** -8 if dtype == torch.bfloat16 else 0.0
    gmax = float(G.abs().max())
    worst = [0.0, 0.0]
    for si, rows in enumerate(_row_sets(n, H, W)):
        ref, dref = _reference(n, H, W, si, True)
        out, df = _run(n, H, W, rows, dtype, True)
        got, dgot = out.double().cpu(), df.double().cpu()
        assert got.shape == (2 * n, H, W, CPAD) and out.dtype == dtype and df.dtype == dtype
        # one-hot and pad channels, every element: exactly the reference's 0 / 1
        assert torch.equal(got[..., :NCLS], ref[..., :NCLS]) and bool((got[..., NCLS + 1:] == 0).all()), si
        for i, row in enumerate(rows):
            vis, sy, sx = R.visible_mask(row, H, W)
            for half, img in ((0, fake), (1, real)):
                o = got[half * n + i]
                assert bool((o[~vis] == 0).all()), (si, i, half)                     # invisible: all 8 channels 0
                if row[0] == 0.0 and row[1] == 1.0:                                 # c = 1, b = 0: the source's bits
                    want = torch.where(vis, img[i][sy, sx], torch.zeros(()).double()).to(dtype)
                    assert torch.equal(_bits(out[half * n + i, :, :, NCLS].cpu()[vis]), _bits(want[vis])), (si, i, half)
        err = (got - ref).abs() - rel * ref.abs()
        worst[0] = max(worst[0], float(err.max()))
        assert float(err.max()) <= 1e-5, (si, float(err.max()))
        derr = (dgot - dref).abs() - 2.0 ** -8 * dref.abs()
        worst[1] = max(worst[1], float(derr.max()) / gmax)
        assert float(derr.max()) <= 1e-6 * gmax, (si, float(derr.max()), gmax)
    print('%s %s: forward |got - ref| - rel|ref| at most %.3e (bound 1e-5); backward at most %.3e max|G| (bound 1e-6)'
          % (shape, dtype, worst[0], worst[1]))


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize('color', [True, False], ids=['color', 'no-color'])
def test_identity_rows_give_d_input_bit_for_bit(color, shape, dtype):
    from seg2eye_amd import ops
    n, H, W = shape
    label, fake, real, G = _inputs(n, H, W)
    out, df = _run(n, H, W, _row_sets(n, H, W)[0], dtype, color)
    f = fake.to(DEV, dtype).view(n, 1, H, W).requires_grad_(True)
    plain = ops.d_input(label.to(DEV), f, real.to(DEV, dtype).view(n, 1, H, W), NCLS, CPAD)
    plain.backward(G.to(DEV, dtype))
    assert torch.equal(_bits(out), _bits(plain.detach()))                           # the zeros' signs included
    assert torch.equal(df, f.grad.view(n, H, W))


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
def test_policy_without_colour_is_exact(shape, dtype):
    """color=False: b and c are not read, the image channel is a copy and the gradient a gather -- no arithmetic, so every element
    of both equals the reference (whose values are bf16 numbers)."""
    n, H, W = shape
    for si, rows in enumerate(_row_sets(n, H, W)):
        ref, dref = _reference(n, H, W, si, False)
        out, df = _run(n, H, W, rows, dtype, False)
        assert torch.equal(out.double().cpu(), ref), si
        assert torch.equal(df.double().cpu(), dref), si


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('color', [True, False], ids=['color', 'no-color'])
def test_two_calls_give_the_same_bits(color, dtype):
    n, H, W = SHAPES[1]
    rows = _row_sets(n, H, W)[-1]
    a, b = _run(n, H, W, rows, dtype, color), _run(n, H, W, rows, dtype, color)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))


def test_reductions_span_several_partial_blocks():
    """64 x 80 = 5120 pixels: three 2048-pixel partial sums per image and a grid that strides, against the restatement."""
    from seg2eye_amd import ops
    n, H, W = 2, 64, 80
    gen = torch.Generator().manual_seed(8)
    label = torch.randint(0, NCLS, (n, H, W), generator=gen, dtype=torch.uint8)
    fake = (torch.rand(n, H, W, generator=gen) * 2 - 1).bfloat16().double()
    real = (torch.rand(n, H, W, generator=gen) * 2 - 1).bfloat16().double()
    G = torch.randn(2 * n, H, W, CPAD, generator=gen).bfloat16().double()
    rows = [[0.25, 0.5, 8.0, -10.0, 40.0, -5.0, 32.0, 40.0], [-0.5, 1.5, -8.0, 10.0, -7.0, 60.0, 32.0, 40.0]]
    fr = fake.clone().requires_grad_(True)
    ref = R.d_input_aug_ref(label.long(), fr, real, rows, NCLS, CPAD)
    ref.backward(G)
    f = fake.to(DEV, torch.float32).requires_grad_(True)
    out = ops.d_input_aug(label.to(DEV), f, real.to(DEV, torch.float32), torch.tensor(rows, device=DEV), NCLS, CPAD)
    out.backward(G.to(DEV, torch.float32))
    assert float((out.detach().double().cpu() - ref.detach()).abs().max()) <= 1e-5
    assert float((f.grad.double().cpu() - fr.grad).abs().max()) <= 1e-6 * float(G.abs().max())


def test_d_step_configuration_runs_no_backward():
    n, H, W = SHAPES[0]
    out, _ = _run(n, H, W, _row_sets(n, H, W)[-1], torch.bfloat16, True, grad=False)
    from seg2eye_amd import ops
    label, fake, real, _ = _inputs(n, H, W)
    o = ops.d_input_aug(label.to(DEV), fake.to(DEV, torch.bfloat16), real.to(DEV, torch.bfloat16),
                        torch.tensor(_row_sets(n, H, W)[-1], device=DEV), NCLS, CPAD)
    assert not o.requires_grad and o.grad_fn is None and torch.equal(_bits(o), _bits(out))
    with pytest.raises(ValueError):
        ops.d_input_aug(label.to(DEV), fake.to(DEV, torch.bfloat16), real.to(DEV, torch.bfloat16), torch.zeros(n + 1, 8, device=DEV))


# ------------------------------------------------------------------------------------------------ the trainer
def _opt(**kw):
    from seg2eye_amd.options import default_opt
    kw.setdefault('gpu_ids', [0])
    kw.setdefault('compute_dtype', 'fp32')
    return default_opt(ngf=8, ndf=8, crop_size=256, aspect_ratio=1.0, batchSize=2, **kw)


@functools.lru_cache(maxsize=None)
def _batch(seed=21):
    from seg2eye_amd import synthetic as syn
    b = syn.make_batch(2, 256, 256, seed=seed)
    return {'label': torch.from_numpy(b['label']), 'style_image': torch.from_numpy(b['style_image']), 'target': torch.from_numpy(b['target'])}


def _trainer(**kw):
    """A trainer on the hash-filled weights (the same for every trainer of this file)."""
    from seg2eye_amd import synthetic as syn
    from seg2eye_amd.pix2pix_trainer import Pix2PixTrainer
    tr = Pix2PixTrainer(_opt(**kw))
    m = tr.pix2pix_model
    with torch.no_grad():
        for net in (m.netG, m.netD, m.netE):
            sd = net.state_dict()
            filled = syn.fill_state_dict([(k, tuple(v.shape)) for k, v in sd.items()])
            for k, v in sd.items():
                v.copy_(torch.from_numpy(filled[k]))
    return tr


def _record(monkeypatch):
    """Wrap the sampler: every draw is kept."""
    from seg2eye_amd import diffaug
    drawn, real_sample = [], diffaug.sample

    def sample(policy, n, H, W, generator):
        rows = real_sample(policy, n, H, W, generator)
        drawn.append(rows.clone())
        return rows
    monkeypatch.setattr(diffaug, 'sample', sample)
    return drawn


def _hook_d_input(tr, seen):
    return tr.pix2pix_model.netD.register_forward_pre_hook(lambda mod, args: seen.append(args[0].detach().clone()))


def _losses(tr):
    return {k: v.detach().clone() for k, v in tr.get_latest_losses().items()}


def test_identity_rows_leave_the_step_bit_for_bit():
    """(a) policy set, sampler patched to identity rows: one G and one D step (fp32, eager) against a trainer without the flag -- netD's
    inputs and outputs, the losses and the parameters after both steps, bit for bit.  S2E_DETERMINISTIC=1 (read when the library loads:
    one fresh child process, its own time limit): without it two trainers WITHOUT the flag differ from each other after their first
    optimizer step.  tests/_diffaug_child.py says what was measured, and why GAN_Feat's logged value alone is held to a derived bound."""
    e = dict(os.environ, S2E_DETERMINISTIC='1')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_diffaug_child.py')], env=e, capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0 and 'diffaug child ok' in r.stdout, (r.stdout[-4000:], r.stderr[-4000:])


def test_each_step_sees_its_own_rows_and_both_halves_the_same(monkeypatch):
    """(b) full policy, fixed seed: netD's input in the G step and in the D step against the restatement of that step's rows, applied to
    the label map, that step's generator output (a forward hook on netG) and the target."""
    drawn = _record(monkeypatch)
    tr = _trainer(diffaug=FULL, diffaug_seed=11)
    m = tr.pix2pix_model
    seen, fakes = [], []
    h = [_hook_d_input(tr, seen), m.netG.register_forward_hook(lambda mod, args, out: fakes.append(out.detach().clone()))]
    with torch.no_grad():
        m(dict(_batch()), mode='inference')
    assert seen == [] and drawn == [] and len(fakes) == 1                           # inference neither discriminates nor draws
    tr.run_generator_one_step(dict(_batch()))
    tr.run_discriminator_one_step(dict(_batch()))
    torch.cuda.synchronize()
    for x in h:
        x.remove()
    assert len(seen) == 2 and len(drawn) == 2 and len(fakes) == 3
    assert not torch.equal(drawn[0], drawn[1])                                      # fresh rows before each step
    assert torch.equal(tr.get_latest_generated(), fakes[1])                         # what the trainer hands out is the generator's output
    label = _batch()['label'][:, 0].long()
    real = _batch()['target'].double()[:, 0]
    for step, (x, fake, rows) in enumerate(zip(seen, fakes[1:], drawn)):
        got = x.double().cpu()
        assert got.shape == (4, 256, 256, 8) and tuple(fake.shape) == (2, 1, 256, 256)
        ref = R.d_input_aug_ref(label, fake.double().cpu()[:, 0], real, rows, NCLS, CPAD)
        err = float((got - ref).abs().max())
        print('step %d: |netD input - restatement| at most %.3e (bound 1e-5)' % (step, err))
        assert err <= 1e-5, (step, err)
        assert torch.equal(got[..., :NCLS], ref[..., :NCLS]) and bool((got[..., NCLS + 1:] == 0).all())
        # both halves used the same row per sample: the same pixels are blank, the same one-hot channels
        assert torch.equal(got[:2, :, :, :NCLS], got[2:, :, :, :NCLS]), step
        for i in range(2):
            vis, _, _ = R.visible_mask(rows[i].tolist(), 256, 256)
            assert 0 < int(vis.sum()) < 256 * 256                                   # (the full policy does blank something)
            for half in (0, 1):
                assert bool((got[2 * half + i][~vis] == 0).all()) and bool((got[2 * half + i][vis][:, :NCLS].sum(-1) == 1).all()), (step, i, half)


def test_hip_graph_replays_see_fresh_rows_and_the_eager_sequence(monkeypatch):
    """(c) three iterations with hip_graphs on and off, same seed: the losses follow each other within test_hip_graph_steps_match_eager's
    bounds -- only if every replay reads fresh rows and the capture did not shift the draw sequence."""
    res = {}
    for graphs in (False, True):
        drawn = _record(monkeypatch)
        tr = _trainer(diffaug=FULL, diffaug_seed=5, hip_graphs=graphs)
        hist, inputs = [], []
        for it in range(3):
            tr.run_generator_one_step(dict(_batch()))
            tr.run_discriminator_one_step(dict(_batch()))
            hist.append({k: float(v.float().mean()) for k, v in tr.get_latest_losses().items()})
            inputs.append(tr._aug_rows.clone())
        torch.cuda.synchronize()
        assert tr.use_graphs == graphs and (tr.graph_G is not None) == graphs         # (a failed capture would have fallen back to eager)
        res[graphs] = (hist, [d.clone() for d in drawn], inputs)
        monkeypatch.undo()
        del tr
    assert len(res[False][1]) == len(res[True][1]) == 6                             # capturing drew nothing
    for a, b in zip(res[False][1], res[True][1]):
        assert torch.equal(a, b)
    for graphs in (False, True):                                                    # the device buffer held each iteration's D-step rows
        for it in range(3):
            assert torch.equal(res[graphs][2][it].cpu(), res[graphs][1][2 * it + 1]), (graphs, it)
    for it, (a, b) in enumerate(zip(res[False][0], res[True][0])):
        for k in a:
            print(it, k, a[k], b[k])
            assert abs(a[k] - b[k]) <= (5e-4 if it == 0 else 1e-2) * max(1.0, abs(a[k])), (it, k, a[k], b[k])


def test_replayed_d_input_differs_between_iterations(monkeypatch):
    """(c, second half) under replay netD's captured input buffer holds another augmentation in iteration 2 than in iteration 1: the
    replay read fresh rows.  (A forward pre-hook does not fire during a replay, so the hook keeps the tensor the graph writes.)"""
    tr = _trainer(diffaug=FULL, diffaug_seed=5, hip_graphs=True)
    seen = []
    h = tr.pix2pix_model.netD.register_forward_pre_hook(lambda mod, args: seen.append(args[0].detach()))
    snaps = []
    for it in range(3):
        tr.run_generator_one_step(dict(_batch()))
        tr.run_discriminator_one_step(dict(_batch()))
        torch.cuda.synchronize()
        snaps.append(seen[-1].detach().clone())                                     # the D graph's input tensor, as this replay left it
    h.remove()
    assert tr.use_graphs and tr.graph_D is not None
    assert not torch.equal(snaps[1][2:], snaps[2][2:])                              # the real half: same frames, other rows
    assert not torch.equal(snaps[0][2:], snaps[1][2:])


def test_bf16_steps_stay_finite_and_generated_is_not_augmented():
    """(d) bf16, full policy, three iterations: finite losses, and get_latest_generated() is the generator's own output -- an inference
    pass (train mode, as the step runs) on the weights and buffers as they were before the step -- not what D was shown."""
    tr = _trainer(diffaug=FULL, diffaug_seed=3, compute_dtype='bf16')
    m = tr.pix2pix_model
    for it in range(3):
        buffers = lambda: [b for net in (m.netG, m.netE) for b in net.buffers()]
        snap = [b.clone() for b in buffers()]
        m.train()
        with torch.no_grad():
            want = m(dict(_batch()), mode='inference').float().clone()
            for b, s0 in zip(buffers(), snap):                                      # (the pass advanced spectral norm's u, v: put them back)
                b.copy_(s0)
        tr.run_generator_one_step(dict(_batch()))
        got = tr.get_latest_generated().float()
        tr.run_discriminator_one_step(dict(_batch()))
        losses = {k: float(v.float().mean()) for k, v in tr.get_latest_losses().items()}
        assert all(torch.isfinite(torch.tensor(v)) for v in losses.values()), (it, losses)
        err = float((got - want).abs().max())
        print('iteration %d: generated against inference max-abs-diff %.3e; losses %s' % (it, err, losses))
        assert got.shape == (2, 1, 256, 256) and err < 1e-3, (it, err)               # (G_TOL of test_networks_gpu.py)
