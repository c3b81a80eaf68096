"""The table of image-quality terms (seg2eye_amd/quality.py) and its consumers, without a GPU: the records and their flags; the shape
check every quality op makes before it looks at the device; the Tester's walk over the records, with each record's `score_u8` replaced
by the fp64 restatement of tests/_*_ref.py."""
import numpy as np
import pytest
import torch

import _ffl_ref
import _msssim_ref
import _region_ref
import _ssim_ref
from _quality_harness import load_log

NAMES = ['ssim', 'msssim', 'region', 'ffl']


def test_the_table_names_four_terms_in_step_order_and_only_known_flags():
    from seg2eye_amd.options import parse
    from seg2eye_amd.quality import TERMS
    assert [t.name for t in TERMS] == NAMES
    assert [t.train_flag for t in TERMS] == ['lambda_ssim', 'lambda_msssim', 'lambda_region', 'lambda_ffl']
    assert [t.val_flag for t in TERMS] == ['val_ssim', 'val_msssim', 'val_regions', 'val_ffl']
    assert [(t.loss_key, t.log_key) for t in TERMS] == [('SSIM/weighted', 'SSIM/raw'), ('MSSSIM/weighted', 'MSSSIM/raw'),
                                                        ('region/weighted', 'region/raw'), ('FFL/weighted', 'FFL/raw')]
    assert [t.dataset for t in TERMS] == NAMES and [t.fmt for t in TERMS] == ['%.4f', '%.4f', '%.2f', '%.3e']
    assert [t.all_attr for t in TERMS] == ['all_ssim', 'all_msssim', 'all_regions', 'all_ffl']
    for field in ('name', 'train_flag', 'val_flag', 'loss_key', 'log_key', 'dataset'):
        assert len({getattr(t, field) for t in TERMS}) == len(TERMS), field
    for t in TERMS:
        assert getattr(parse(['--' + t.train_flag, '1.5']), t.train_flag) == 1.5
        with pytest.raises(SystemExit):
            parse(['--' + t.train_flag, '1.5'], is_train=False)                       # a training flag only
        assert getattr(parse(['--' + t.val_flag]), t.val_flag) is True
        assert getattr(parse(['--' + t.val_flag], is_train=False), t.val_flag) is True
        assert getattr(parse([]), t.train_flag) == 0.0 and getattr(parse([], is_train=False), t.val_flag) is False


def _ops_on(x, y):
    """The ten quality ops on the float pair (x, y) and on its uint8 form, as thunks."""
    from seg2eye_amd import ops
    a, b = x.to(torch.uint8), y.to(torch.uint8)
    lab = torch.zeros(2, 16, 16, dtype=torch.uint8)
    return {'ssim': lambda: ops.ssim(x, y), 'ssim_u8': lambda: ops.ssim_u8(a, b),
            'ms_ssim': lambda: ops.ms_ssim(x, y), 'ms_ssim_u8': lambda: ops.ms_ssim_u8(a, b),
            'focal_freq_loss': lambda: ops.focal_freq_loss(x, y), 'focal_freq_loss_u8': lambda: ops.focal_freq_loss_u8(a, b),
            'region_loss': lambda: ops.region_loss(x, y, lab, torch.ones(4)), 'region_stats_u8': lambda: ops.region_stats_u8(a, b, lab, 4),
            'openeds_error': lambda: ops.openeds_error(x, y), 'openeds_error_u8': lambda: ops.openeds_error_u8(a, b)}


def test_every_quality_op_compares_the_two_shapes_before_it_looks_at_the_device():
    """The entry points take one (N, H, W) for both images, so a smaller second image would be read past its end: the ops refuse the
    pair, and do so before the device check -- which is why CPU tensors can show it.  With equal shapes the device check is next."""
    from seg2eye_amd import _lib
    x = torch.zeros(2, 1, 16, 16)
    for name, call in _ops_on(x, torch.zeros(2, 1, 16, 18)).items():
        with pytest.raises(ValueError, match='one shape'):
            call()
    for name, call in _ops_on(x.requires_grad_(True), torch.zeros(2, 1, 18, 16)).items():
        with pytest.raises(ValueError, match='one shape'):
            call()
    for name, call in _ops_on(x.detach(), torch.zeros(2, 1, 16, 16)).items():
        with pytest.raises(_lib.Seg2EyeHipError, match='GPU only'):
            call()


# ------------------------------------------------------------------------------------------------ the Tester's walk
class _Model:
    """What run_validation asks of a model once run_batch is replaced."""

    def device(self):
        return torch.device('cpu')


def _label(data_i):
    label = torch.as_tensor(data_i['label'])
    return (label[:, 0] if label.dim() == 4 else label).to(torch.uint8)


_RESTATEMENTS = {
    'ssim': lambda f, t, data_i, opt: _ssim_ref.ssim_u8(f[:, 0], t[:, 0]).numpy(),
    'msssim': lambda f, t, data_i, opt: _msssim_ref.ms_ssim_u8(f[:, 0], t[:, 0]).numpy(),
    'region': lambda f, t, data_i, opt: _region_ref.stats(f[:, 0], t[:, 0], _label(data_i), opt.label_nc).numpy(),
    'ffl': lambda f, t, data_i, opt: _ffl_ref.ffl_u8(f[:, 0], t[:, 0], 1.0).numpy(),
}


def _restated(name, batches):
    """The record `name`'s score_u8 as the fp64 restatement -- after it has seen that the Tester hands it the produced image, the target
    and the batch of the run_batch call just made, in that order (the restatements are symmetric in the pair and could not tell)."""
    def score_u8(f, t, data_i, opt):
        _, produced, target, batch = batches[-1]
        assert f is produced and t is target and data_i is batch, name
        return _RESTATEMENTS[name](f, t, data_i, opt)
    return score_u8


def _walk(tmp_path, monkeypatch, capsys, flags):
    """A validation Tester on the synthetic dataset (2 batches of 2) whose run_batch returns fixed random uint8 pairs and whose records
    score with the restatements -> (tester, errors, statistics, printed text, log, [(errors, produced, target, data_i) per batch])."""
    from seg2eye_amd.options import parse
    from seg2eye_amd.quality import TERMS
    from seg2eye_amd.tester import Tester
    batches = []
    for t in TERMS:
        monkeypatch.setattr(t, 'score_u8', _restated(t.name, batches))
    argv = ['--name', 'qt', '--checkpoints_dir', str(tmp_path), '--dataset_key', 'validation', '--crop_size', '256', '--aspect_ratio', '1.0',
            '--batchSize', '2', '--synthetic_size', '4']
    tester = Tester(parse(argv + flags, is_train=False), dataset_key='validation')
    gen = torch.Generator().manual_seed(5)

    def run_batch(data_i, model):
        produced = torch.randint(0, 256, (2, 1, 640, 400), generator=gen, dtype=torch.uint8)
        target = (produced.float() + 20 * torch.randn(2, 1, 640, 400, generator=gen)).clamp(0, 255).to(torch.uint8)
        errors = np.sqrt(((produced.double() - target.double()) ** 2).sum(dim=(1, 2, 3)).numpy()) / (640 * 400)
        batches.append((errors, produced, target, data_i))
        return errors, None, produced, target
    tester.run_batch = run_batch
    capsys.readouterr()
    errs, stats = tester.run(_Model(), mode='full', write_error_log=True)
    return tester, errs, stats, capsys.readouterr().out, load_log(tester), batches


def test_the_tester_walks_the_records_into_the_log_the_lists_and_the_statistics(tmp_path, monkeypatch, capsys):
    tester, errs, stats, printed, log, batches = _walk(tmp_path, monkeypatch, capsys, ['--val_ssim', '--val_msssim', '--val_regions', '--val_ffl'])
    assert len(batches) == 2 and len(errs) == 4
    assert sorted(log) == ['error', 'ffl', 'filename', 'msssim', 'region', 'ssim', 'user']
    for k in ('error', 'ssim', 'msssim', 'ffl'):
        assert log[k].dtype == np.float64 and log[k].shape == (4,), k
    assert log['region'].dtype == np.float64 and log['region'].shape == (4, tester.opt.label_nc, 3)
    assert log['user'].dtype == np.dtype('S4') and log['filename'].dtype == np.dtype('S13')
    assert np.array_equal(log['error'], np.concatenate([b[0] for b in batches]))
    for name in NAMES:                                                               # bit for bit against the restatement, computed anew
        want = np.concatenate([_RESTATEMENTS[name](p, t, d, tester.opt) for _, p, t, d in batches]).astype(np.float64)
        assert np.array_equal(log[name], want), name
    for name, attr in zip(NAMES, ('all_ssim', 'all_msssim', 'all_regions', 'all_ffl')):
        assert np.array_equal(np.asarray(getattr(tester, attr), dtype=np.float64), log[name]), attr
    assert float(log['region'][:, :, 0].sum()) == 4 * 640 * 400                      # the synthetic labels tile the frame
    tot = log['region'].sum(axis=0)
    present = [c for c in range(tot.shape[0]) if tot[c, 0] > 0]
    want = {'mse/validation/full/relative': '%.2f', 'ssim/validation/full': '%.4f', 'msssim/validation/full': '%.4f', 'ffl/validation/full': '%.3e'}
    for c in present:
        want['region_mae/validation/full/%d' % c] = want['region_rmse/validation/full/%d' % c] = '%.2f'
        assert stats['region_mae/validation/full/%d' % c] == float(tot[c, 1] / tot[c, 0])
        assert stats['region_rmse/validation/full/%d' % c] == float(np.sqrt(tot[c, 2] / tot[c, 0]))
    assert present and sorted(stats) == sorted(want)
    for name in ('ssim', 'msssim', 'ffl'):
        assert stats['%s/validation/full' % name] == float(np.mean(log[name]))
    for k, fmt in want.items():                                                      # every statistic in its own format
        assert ('  %s, ' + fmt) % (k, stats[k]) + '\n' in printed, (k, printed)
    tester.print_results(errs, stats)                                                # ... also when called on its own, as before
    assert capsys.readouterr().out.splitlines()[3:-1] == [('  %s, ' + want[k]) % (k, stats[k]) for k in sorted(want)]
    # a second run starts new lists: the first run's are left as they were
    first = tester.all_ssim
    assert tester.run_validation(_Model(), iter(()), limit=4) == []
    assert tester.all_ssim is not first and len(first) == 4 and tester.all_ssim == [] and tester.scores['ssim'] is tester.all_ssim


def test_without_a_flag_the_tester_writes_the_base_datasets_and_the_one_statistic(tmp_path, monkeypatch, capsys):
    tester, errs, stats, printed, log, batches = _walk(tmp_path, monkeypatch, capsys, [])
    assert sorted(log) == ['error', 'filename', 'user'] and sorted(stats) == ['mse/validation/full/relative'] and len(errs) == 4
    assert tester.all_ssim == [] and tester.all_msssim == [] and tester.all_regions == [] and tester.all_ffl == []
    assert '  mse/validation/full/relative, %.2f\n' % stats['mse/validation/full/relative'] in printed
