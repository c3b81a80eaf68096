"""The loop over quality.TERMS on the GPU, all four terms at once: the generator's loss eager and as hipGraph replays, and the Tester.
No kernel is tested here (tests/test_{ssim,msssim,region,ffl}_gpu.py do that, per element): what is checked is that the loop hands each
op the step's own tensors -- so every logged term is bit-equal to the op called directly, each op's test_two_calls_give_the_same_bits
having established that two calls agree to the bit -- and that the four capture together.  ngf = ndf = 8, batch 2, fp32, 256 x 256:
the harness's shape, and the smallest of the term tests that five-level MS-SSIM admits (H, W >= 176)."""
import numpy as np
import pytest
import torch

from _quality_harness import PARENT_LOSS_KEYS, batch, load_log, recording_tester, trainer

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LAMBDAS = dict(lambda_ssim=1.0, lambda_msssim=2.0, lambda_region=3.0, lambda_ffl=4.0)
RAW = ['SSIM/raw', 'MSSSIM/raw', 'region/raw', 'FFL/raw']
WEIGHTED = ['SSIM/weighted', 'MSSSIM/weighted', 'region/weighted', 'FFL/weighted']
# what the graph-versus-eager bound is relative to, as in each term's own graph test: max(1, |value|) for the three terms of order one,
# the value itself for the focal frequency loss, which is far below one
FLOOR = {k: (lambda v: v) if k.startswith('FFL/') else (lambda v: max(1.0, v)) for k in RAW + WEIGHTED}


def _bits(t):
    return t.detach().float().contiguous().view(torch.int32).cpu()


def test_an_eager_step_logs_what_the_ops_give_on_the_steps_own_tensors():
    from seg2eye_amd import ops
    tr = trainer(ffl_alpha=1.5, region_weights='1,2,4,8', **LAMBDAS)
    tr.run_generator_one_step(dict(batch()))
    torch.cuda.synchronize()
    losses = dict(tr.get_latest_losses(include_log_losses=True))
    fake, grad = tr.get_latest_generated().detach(), tr.optimizer_G.flat_g.detach().clone()
    model = tr.pix2pix_model
    target = batch()['target'].to(DEV)
    label = batch()['label'].to(DEV).to(torch.uint8)
    assert model.region_w is not None and model.region_w.tolist() == [1.0, 2.0, 4.0, 8.0] and model.opt.ffl_alpha == 1.5
    assert tuple(fake.shape) == (2, 1, 256, 256) and fake.dtype == torch.float32
    want = {'SSIM/raw': ops.ssim(fake, target).mean(), 'MSSSIM/raw': ops.ms_ssim(fake, target).mean(),     # (before the D step reuses the step's memory)
            'region/raw': ops.region_loss(fake, target, label, model.region_w, 'l1')[0],
            'FFL/raw': ops.focal_freq_loss(fake, target, model.opt.ffl_alpha).mean()}
    tr.run_discriminator_one_step(dict(batch()))
    torch.cuda.synchronize()
    # (after the D step: the log entries */raw were read, and so consumed, after the G step)
    assert set(tr.get_latest_losses(include_log_losses=True)) == PARENT_LOSS_KEYS | set(WEIGHTED)
    assert set(losses) >= set(RAW) | set(WEIGHTED) and all(tuple(losses[k].shape) == (1,) for k in WEIGHTED)
    for k in RAW:
        print(k, float(losses[k]), float(want[k]))
        assert torch.equal(_bits(losses[k]).view(-1), _bits(want[k]).view(-1)), (k, float(losses[k]), float(want[k]))
    assert bool(torch.isfinite(grad).all())


def test_hip_graph_replays_follow_the_eager_log_of_all_four_terms():
    """Two iterations with hip_graphs off and on from the same state: the logs agree within the bounds of the per-term graph tests
    (5e-4 on identical weights, 1e-2 once an Adam step has been taken), the G step was captured, and every replay scores anew."""
    res = {}
    for graphs in (False, True):
        tr = trainer(hip_graphs=graphs, **LAMBDAS)
        hist = []
        for it in range(2):
            tr.run_generator_one_step(dict(batch()))
            tr.run_discriminator_one_step(dict(batch()))
            hist.append({k: float(v.float().mean()) for k, v in tr.get_latest_losses(include_log_losses=True).items()})
        torch.cuda.synchronize()
        assert tr.use_graphs == graphs and (tr.graph_G is not None) == graphs       # (a failed capture would have fallen back to eager)
        res[graphs] = hist
        del tr
    for it, (a, b) in enumerate(zip(res[False], res[True])):
        assert set(a) == set(b) == PARENT_LOSS_KEYS | set(RAW) | set(WEIGHTED)
        for k in RAW + WEIGHTED:
            print(it, k, a[k], b[k])
            assert abs(a[k] - b[k]) <= (5e-4 if it == 0 else 1e-2) * FLOOR[k](abs(a[k])), (it, k, a[k], b[k])
    for k in RAW:
        assert res[True][0][k] != res[True][1][k], k                                # the second replay scored the stepped generator


def test_the_tester_writes_what_the_u8_ops_give_on_the_pairs_it_scored(tmp_path):
    from seg2eye_amd import ops
    from seg2eye_amd.options import parse
    from seg2eye_amd.pix2pix_model import Pix2PixModel
    argv = ['--name', 'qt', '--checkpoints_dir', str(tmp_path), '--dataset_key', 'validation', '--ngf', '8', '--crop_size', '256',
            '--aspect_ratio', '1.0', '--batchSize', '2', '--synthetic_size', '4', '--compute_dtype', 'fp32']
    torch.manual_seed(0)
    Pix2PixModel(parse(argv)).save('latest')
    model = Pix2PixModel(parse(argv, is_train=False))
    model.eval()
    tester, seen, labels = recording_tester(argv, ['--val_ssim', '--val_msssim', '--val_regions', '--val_ffl'])
    errs, stats = tester.run(model, mode='full', write_error_log=True)
    log = load_log(tester)
    assert len(seen) == 2 and len(errs) == 4
    assert sorted(log) == ['error', 'ffl', 'filename', 'msssim', 'region', 'ssim', 'user']
    want = {k: [] for k in ('ssim', 'msssim', 'region', 'ffl')}
    for (p, t), lab in zip(seen, labels):
        p, t, lab = p.to(DEV), t.to(DEV), lab.to(DEV).to(torch.uint8)
        assert p.dtype == torch.uint8 and tuple(p.shape) == (2, 1, 640, 400) and tuple(t.shape) == (2, 1, 640, 400)
        want['ssim'].append(ops.ssim_u8(p, t))
        want['msssim'].append(ops.ms_ssim_u8(p, t))
        want['region'].append(ops.region_stats_u8(p, t, lab, tester.opt.label_nc))
        want['ffl'].append(ops.focal_freq_loss_u8(p, t, 1.0))
    for k, rows in want.items():
        rows = torch.cat(rows).cpu().numpy().astype(np.float64)
        assert log[k].dtype == np.float64 and log[k].shape == rows.shape and np.array_equal(log[k], rows), k
    for k, attr in (('ssim', 'all_ssim'), ('msssim', 'all_msssim'), ('region', 'all_regions'), ('ffl', 'all_ffl')):
        assert np.array_equal(log[k], np.asarray(getattr(tester, attr), dtype=np.float64)), k
    tot = log['region'].sum(axis=0)
    present = [c for c in range(tot.shape[0]) if tot[c, 0] > 0]
    assert present and sorted(stats) == sorted(
        ['mse/validation/full/relative', 'ssim/validation/full', 'msssim/validation/full', 'ffl/validation/full']
        + ['region_mae/validation/full/%d' % c for c in present] + ['region_rmse/validation/full/%d' % c for c in present])
