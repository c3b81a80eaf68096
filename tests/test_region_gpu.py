"""The region-aware error on the GPU: ops.region_loss / ops.region_stats_u8 and the backward against the fp64 restatement of
tests/_region_ref.py (whose gradient is autograd's), every element; the generator's --lambda_region term, eager and as hipGraph replays; the
Tester under --val_regions.

Inputs are drawn on the bf16 grid (k / 128, |k| <= 128), so d = x - y and d^2 are exact in fp32 and both dtypes see the same numbers.
Bounds, from the arithmetic and never from the kernel:
    counts                exact
    sum |d|, sum d^2      4 * 2^-24 relative: one rounding of d, at most two more for d^2, same-sign terms, fp64 accumulation
    loss, coef            16 * 2^-24 relative: a handful of fp32 roundings of same-sign terms
    gradient, per element 16 * 2^-24 |want|, plus 2^-8 |want| for a bf16 output; exactly 0 where want is 0
    uint8 statistics      bit-equal: integers below 2^53
The fp32 restatement alone (fp32 x, y, d, loss and gradient around fp64 sums) must stay within 1.6 * 2^-24 of the fp64 one on loss and
gradient, every element, at every case, so the bounds are not met by an accident of the oracle.

Measured on an MI355X (largest over the label plans and norms of a shape; relative, per element for the gradient):

    shape        sum |d|, d^2   loss       coef       gradient fp32   gradient bf16   fp32 restatement: loss, gradient
    1x1x1        0.0e+00        0.0e+00    0.0e+00    0.0e+00         2.9e-03         0.0e+00, 0.0e+00
    2x3x5        0.0e+00        3.9e-08    5.8e-08    1.2e-07         3.7e-03         3.9e-08, 5.3e-08
    2x17x70      0.0e+00        4.0e-08    5.6e-08    1.2e-07         3.8e-03         4.0e-08, 5.9e-08
    3x43x70      0.0e+00        4.6e-08    5.1e-08    1.3e-07         3.8e-03         4.6e-08, 5.7e-08
    2x64x64      0.0e+00        4.5e-08    5.3e-08    1.5e-07         3.9e-03         4.5e-08, 5.9e-08
    2x256x256    0.0e+00        3.4e-08    4.8e-08    1.4e-07         3.7e-03         3.4e-08, 5.9e-08
"""
import functools

import numpy as np
import pytest
import torch

import _region_ref as R
from _quality_harness import batch as _batch, load_log as _load_log, trainer as _trainer

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
# one pixel; less than a wave, odd H W (image 1 starts unaligned); H W no multiple of 8, a ragged last group; one block exactly; many blocks
SHAPES = [(1, 1, 1), (2, 3, 5), (2, 17, 70), (3, 43, 70), (2, 64, 64), (2, 256, 256)]
SHAPE_IDS = ['x'.join(map(str, s)) for s in SHAPES]
KINDS = ['iid', 'absent', 'one_image', 'seven', 'zero_weight']
WEIGHTS = {'iid': (1.0, 1.0, 1.0, 1.0), 'absent': (0.5, 2.0, 1.0, 3.0), 'one_image': (1.0, 1.0, 1.0, 1.0), 'seven': (2.0, 1.0, 0.25, 1.0),
           'zero_weight': (1.0, 0.0, 2.0, 0.5)}
DTYPES = [torch.float32, torch.bfloat16]
DTYPE_IDS = ['fp32', 'bf16']
NORMS = ['l1', 'l2']
NCLS = 4
G = 1.75                                                      # the incoming gradient of the loss
U = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ inputs and references (computed once)
@functools.lru_cache(maxsize=None)
def _inputs(shape, kind):
    """x, y (fp64 values on the bf16 grid, a few x == y pixels planted) and a uint8 label; CPU, never written."""
    n, H, W = shape
    gen = torch.Generator().manual_seed(100000 * KINDS.index(kind) + 1000 * n + 31 * H + W)
    x = torch.randint(-128, 129, shape, generator=gen).double() / 128
    y = torch.randint(-128, 129, shape, generator=gen).double() / 128
    same = torch.rand(shape, generator=gen) < 0.05
    y = torch.where(same, x, y)
    lab = torch.randint(0, NCLS, shape, generator=gen, dtype=torch.uint8)
    if kind == 'absent':                                      # class 3 is nowhere in the batch
        lab = lab.clamp(max=2)
    elif kind == 'one_image':                                 # class 3 in image 0 only
        lab[1:] = lab[1:].clamp(max=2)
        lab[0, 0, 0] = 3
    elif kind == 'seven':                                     # a value that is no class: every fifth pixel, the first included
        lab.view(-1)[::5] = 7
    return x, y, lab


@functools.lru_cache(maxsize=None)
def _reference(shape, kind, norm):
    x, y, lab = _inputs(shape, kind)
    w = WEIGHTS[kind]
    v64, g64 = R.loss_and_grad(x, y, lab, w, norm, G, torch.float64)
    v32, g32 = R.loss_and_grad(x, y, lab, w, norm, G, torch.float32)
    return R.stats(x, y, lab, NCLS), v64, g64, R.coef(lab, shape, w), v32.double(), g32.double()


def _rel(got, want):
    """largest |got - want| / |want| over the elements (0 where both are 0, inf where only want is)"""
    got, want = torch.as_tensor(got, dtype=torch.float64).cpu(), torch.as_tensor(want, dtype=torch.float64)
    diff = (got - want).abs()
    r = torch.where(want != 0, diff / want.abs().clamp(min=1e-300), torch.where(diff == 0, torch.zeros_like(diff), torch.full_like(diff, float('inf'))))
    return float(r.max()) if r.numel() else 0.0


def _run(x, y, lab, w, norm, dtype, grad=True):
    from seg2eye_amd import ops
    n, H, W = x.shape
    xd = x.to(DEV, dtype).view(n, 1, H, W).requires_grad_(grad)
    loss, stats = ops.region_loss(xd, y.to(DEV, dtype).view(n, 1, H, W), lab.to(DEV), torch.tensor(w, dtype=torch.float32, device=DEV), norm)
    coef = None
    if grad:
        coef = loss.grad_fn.saved_tensors[3].clone()
        (loss * G).backward()
    return loss.detach(), stats, coef, (xd.grad.view(n, H, W) if grad else None)


def _bits(t):
    return t.contiguous().view({torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}[t.dtype])


# ------------------------------------------------------------------------------------------------ the op
@pytest.mark.parametrize('norm', NORMS)
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
def test_forward_and_backward_match_the_restatement(shape, kind, dtype, norm):
    x, y, lab = _inputs(shape, kind)
    s64, v64, g64, k64, v32, g32 = _reference(shape, kind, norm)
    bf = dtype == torch.bfloat16
    assert torch.equal(x.to(dtype).double(), x) and torch.equal(y.to(dtype).double(), y)           # on the grid: nothing is lost on the way in
    loss, stats, coef, dx = _run(x, y, lab, WEIGHTS[kind], norm, dtype)
    assert loss.shape == () and loss.dtype == torch.float32 and stats.shape == (shape[0], NCLS, 3) and stats.dtype == torch.float64
    assert not stats.requires_grad and dx.dtype == dtype and dx.shape == x.shape and coef.shape == (NCLS,) and coef.dtype == torch.float32
    stats = stats.cpu()
    e_sum, e_loss, e_coef = _rel(stats[:, :, 1:], s64[:, :, 1:]), _rel(loss, v64), _rel(coef, k64)
    diff = (dx.double().cpu() - g64).abs()
    allowed = (16 * U + (2.0 ** -8 if bf else 0.0)) * g64.abs()
    e_grad = _rel(dx, g64)
    e32_loss, e32_grad = _rel(v32, v64), _rel(g32, g64)
    print('%s %s %s %s: sums %.3e, loss %.3e, coef %.3e, gradient %.3e; the fp32 restatement: loss %.3e, gradient %.3e' % (
        shape, kind, 'bf16' if bf else 'fp32', norm, e_sum, e_loss, e_coef, e_grad, e32_loss, e32_grad))
    assert torch.equal(stats[:, :, 0], s64[:, :, 0])                                                # counts: exactly
    assert e_sum <= 4 * U, e_sum
    assert e_loss <= 16 * U and e_coef <= 16 * U, (e_loss, e_coef)
    assert bool((diff <= allowed).all()), (e_grad, int((diff > allowed).sum()))                     # every element
    l = R.lookup(lab, shape[1], shape[2])
    zero_w = torch.tensor([wc == 0 for wc in WEIGHTS[kind]] + [True] * 252)[l]                     # (a class >= ncls: no weight at all)
    must_be_zero = zero_w | ((x == y) if norm == 'l1' else torch.zeros_like(zero_w))
    assert bool((dx.cpu()[must_be_zero] == 0).all())
    if bool((~must_be_zero & (x != y)).any()):
        assert float(dx.float().abs().max()) > 0
    assert e32_loss <= 1.6 * U and e32_grad <= 1.6 * U, (e32_loss, e32_grad)                        # the yardstick


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_two_calls_give_the_same_bits(dtype):
    for shape, kind in (((3, 43, 70), 'iid'), ((2, 256, 256), 'zero_weight')):
        x, y, lab = _inputs(shape, kind)
        a = _run(x, y, lab, WEIGHTS[kind], 'l2', dtype)
        b = _run(x, y, lab, WEIGHTS[kind], 'l2', dtype)
        for s, t in zip(a, b):
            assert torch.equal(_bits(s), _bits(t)), (shape, kind)


def test_nothing_is_saved_when_x_needs_no_gradient():
    from seg2eye_amd import ops
    x, y, lab = _inputs((2, 64, 64), 'iid')
    xd, yd, ld = x.to(DEV, torch.float32), y.to(DEV, torch.float32), lab.to(DEV)
    w = torch.ones(NCLS, device=DEV)
    with_grad, _ = ops.region_loss(xd.clone().requires_grad_(True), yd, ld, w)
    saved = with_grad.grad_fn.saved_tensors
    assert len(saved) == 4 and tuple(saved[3].shape) == (NCLS,) and saved[2].dtype == torch.uint8
    y_only, _ = ops.region_loss(xd, yd.clone().requires_grad_(True), ld, w)         # a node exists, but nothing for x to receive
    assert y_only.grad_fn is not None and y_only.grad_fn.saved_tensors == ()
    yg = yd.clone().requires_grad_(True)
    ops.region_loss(xd, yg, ld, w)[0].backward()
    assert yg.grad is None                                                          # no gradient for the target
    plain, stats = ops.region_loss(xd, yd, ld, w)
    assert plain.grad_fn is None and stats.grad_fn is None
    assert torch.equal(plain, with_grad.detach()) and torch.equal(plain, y_only.detach())
    listed, _ = ops.region_loss(xd, yd, ld, [1, 1, 1, 1])                           # weights as plain numbers
    assert torch.equal(listed, plain)


@pytest.mark.parametrize('shape,lshape', [((2, 11, 13), (2, 11, 13)), ((2, 640, 400), (2, 256, 256))], ids=['2x11x13', '2x640x400-label256'])
def test_stats_u8_are_bit_equal_to_the_restatement(shape, lshape):
    from seg2eye_amd import ops
    gen = torch.Generator().manual_seed(7 * shape[1] + shape[2])
    a = torch.randint(0, 256, shape, generator=gen, dtype=torch.uint8)
    b = torch.randint(0, 256, shape, generator=gen, dtype=torch.uint8)
    b[0, 0, :5] = a[0, 0, :5]
    lab = torch.randint(0, NCLS + 1, lshape, generator=gen, dtype=torch.uint8)      # (class 4 with ncls = 4: in no region)
    lab[lab == NCLS] = 7
    want = R.stats(a, b, lab, NCLS)
    got = ops.region_stats_u8(a.to(DEV).view(shape[0], 1, *shape[1:]), b.to(DEV), lab.to(DEV), NCLS)
    assert got.shape == (shape[0], NCLS, 3) and got.dtype == torch.float64 and not got.requires_grad
    assert torch.equal(_bits(got.cpu()), _bits(want)), (got.cpu() - want).abs().max()
    assert float(want[:, :, 0].sum()) < shape[0] * shape[1] * shape[2]              # (some pixels really were in no region)
    again = ops.region_stats_u8(a.to(DEV), b.to(DEV), lab.to(DEV), NCLS)
    assert torch.equal(_bits(again), _bits(got))


# ------------------------------------------------------------------------------------------------ the generator's loss term
def test_generator_loss_term_matches_the_restatement_and_reaches_netG():
    """ngf = ndf = 8, batch 2, fp32, 256 x 256: region/weighted = 3 * the restatement's loss on the fake the step returns and the batch's
    label; the two keys exist only under the flag; netG's gradient moves by at least 10 x the run-to-run noise of two runs without the term."""
    lam, w = 3.0, (1.0, 2.0, 4.0, 8.0)
    res = []
    for kw in (dict(lambda_region=lam, region_weights=','.join(map(str, w))), {}, {}):
        tr = _trainer(**kw)
        assert (tr.pix2pix_model.region_w is not None) == bool(kw)                   # nothing is allocated without the flag
        tr.run_generator_one_step(dict(_batch()))
        torch.cuda.synchronize()
        res.append((tr.get_latest_losses(include_log_losses=True), tr.get_latest_generated().double().cpu(), tr.optimizer_G.flat_g.detach().double().cpu().clone()))
        del tr
    (losses, fake, grad), (plain, _, grad0), (_, _, grad1) = res
    assert 'region/weighted' not in plain and 'region/raw' not in plain
    assert set(losses) - set(plain) == {'region/weighted', 'region/raw'} and set(plain) <= set(losses)
    assert tuple(losses['region/weighted'].shape) == (1,) and tuple(fake.shape) == (2, 1, 256, 256)
    label = _batch()['label'][:, 0]
    assert [int((label[i] == c).sum()) for i in range(2) for c in range(4)] == [46049, 17161, 2101, 225, 41223, 19675, 3554, 1084]
    want = float(R.loss(fake[:, 0], _batch()['target'].double()[:, 0], label, w, 'l1'))
    got, raw = float(losses['region/weighted']), float(losses['region/raw'])
    print('region/weighted %.8f, 3 x restatement %.8f (relative %.3e, bound %.3e); region/raw %.8f' % (got, lam * want, abs(got - lam * want) / (lam * want), 16 * U, raw))
    assert abs(got - lam * want) <= lam * 16 * U * want, (got, lam * want)
    assert abs(raw - want) <= 16 * U * want
    assert bool(torch.isfinite(grad).all())
    noise = float((grad1 - grad0).norm() / grad0.norm())
    moved = float((grad - grad0).norm() / grad0.norm())
    print('netG + netE gradient: moved by %.3e of its norm under the term; two runs without it differ by %.3e' % (moved, noise))
    assert moved > 0 and moved >= 10 * noise, (moved, noise)


def test_hip_graph_replays_follow_the_eager_region_log():
    """Two G + D iterations with hip_graphs on and off from the same state: the region logs agree within test_hip_graph_steps_match_eager's
    bounds (5e-4 on identical weights, 1e-2 once Adam steps have been taken), i.e. the launches capture and every replay scores anew."""
    res = {}
    for graphs in (False, True):
        tr = _trainer(lambda_region=2.0, region_norm='l2', hip_graphs=graphs)
        hist = []
        for it in range(2):
            tr.run_generator_one_step(dict(_batch()))
            tr.run_discriminator_one_step(dict(_batch()))
            hist.append({k: float(v.float().mean()) for k, v in tr.get_latest_losses(include_log_losses=True).items()})
        torch.cuda.synchronize()
        assert tr.use_graphs == graphs and (tr.graph_G is not None) == graphs       # (a failed capture would have fallen back to eager)
        res[graphs] = hist
        del tr
    for it, (a, b) in enumerate(zip(res[False], res[True])):
        assert 'region/raw' in a and 'region/weighted' in a and set(a) == set(b)
        for k in ('region/raw', 'region/weighted'):
            print(it, k, a[k], b[k])
            assert abs(a[k] - b[k]) <= (5e-4 if it == 0 else 1e-2) * max(1.0, abs(a[k])), (it, k, a[k], b[k])
        assert abs(a['region/weighted'] - 2.0 * a['region/raw']) <= 1e-6 * abs(a['region/weighted'])
    assert res[True][0]['region/raw'] != res[True][1]['region/raw']                 # the second replay scored the stepped generator


# ------------------------------------------------------------------------------------------------ the Tester
def test_tester_takes_the_error_apart_only_under_the_flag(tmp_path):
    from seg2eye_amd.options import parse
    from seg2eye_amd.pix2pix_model import Pix2PixModel
    from seg2eye_amd.tester import Tester
    argv = ['--name', 'rg', '--checkpoints_dir', str(tmp_path), '--dataset_key', 'validation', '--ngf', '8', '--crop_size', '256',
            '--aspect_ratio', '1.0', '--batchSize', '2', '--synthetic_size', '4', '--compute_dtype', 'fp32']
    opt = parse(argv, is_train=False)
    torch.manual_seed(0)
    Pix2PixModel(parse(argv)).save('latest')
    model = Pix2PixModel(opt)
    model.eval()
    plain = Tester(opt, dataset_key='validation')
    errs_plain, stats_plain = plain.run(model, mode='full', write_error_log=True)
    assert sorted(stats_plain) == ['mse/validation/full/relative'] and len(errs_plain) == 4          # today's key ...
    assert sorted(_load_log(plain)) == ['error', 'filename', 'user'] and plain.all_regions == []    # ... and today's datasets

    tester = Tester(parse(argv + ['--val_regions'], is_train=False), dataset_key='validation')
    seen, labels, run_batch = [], [], tester.run_batch

    def recording(data_i, model):
        out = run_batch(data_i, model)
        assert len(out) == 4
        seen.append((out[2].cpu(), out[3].cpu()))
        labels.append(torch.as_tensor(data_i['label']).cpu())
        return out
    tester.run_batch = recording
    errs, stats = tester.run(model, mode='full', write_error_log=True)
    np.testing.assert_allclose(np.asarray(errs), np.asarray(errs_plain), rtol=1e-6)
    log = _load_log(tester)
    assert sorted(log) == ['error', 'filename', 'region', 'user'] and log['region'].dtype == np.float64 and log['region'].shape == (4, 4, 3)
    produced, target = torch.cat([p for p, _ in seen])[:, 0], torch.cat([t for _, t in seen])[:, 0]
    label = torch.cat(labels)
    label = (label[:, 0] if label.dim() == 4 else label).to(torch.uint8)
    assert produced.dtype == torch.uint8 and tuple(produced.shape) == (4, 640, 400) and tuple(label.shape) == (4, 256, 256)
    want = R.stats(produced, target, label, 4).numpy()
    assert np.array_equal(log['region'], want)                                       # integers below 2^53: exactly
    assert np.array_equal(log['region'], np.asarray(tester.all_regions, dtype=np.float64))
    tot = want.sum(axis=0)
    present = [c for c in range(4) if tot[c, 0] > 0]
    assert present, tot
    keys = ['region_mae/validation/full/%d' % c for c in present] + ['region_rmse/validation/full/%d' % c for c in present]
    assert sorted(stats) == sorted(['mse/validation/full/relative'] + keys)
    assert stats['mse/validation/full/relative'] == pytest.approx(stats_plain['mse/validation/full/relative'], rel=1e-6)
    for c in present:
        assert stats['region_mae/validation/full/%d' % c] == pytest.approx(tot[c, 1] / tot[c, 0], rel=1e-12)
        assert stats['region_rmse/validation/full/%d' % c] == pytest.approx(np.sqrt(tot[c, 2] / tot[c, 0]), rel=1e-12)
    # the synthetic labels are all below 4, so the classes tile the frame: their squared errors add up to the OpenEDS error's
    assert float(want[:, :, 0].sum()) == 4 * 640 * 400
    oe = np.sqrt(want[:, :, 2].sum(axis=1)) / (640 * 400)
    print('per-class statistics %s; OpenEDS error from the records %s, reported %s' % ({k: stats[k] for k in keys}, oe.tolist(), list(map(float, errs))))
    np.testing.assert_allclose(oe, np.asarray(errs, dtype=np.float64), rtol=1e-6)
