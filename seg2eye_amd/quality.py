"""The image-quality terms beyond the reference's own, one record each: what the generator's loss, the Tester and
the tools need to know about SSIM, MS-SSIM, the region-aware error and the focal frequency loss.  `TERMS` is ordered; its order is the
launch order of a training step and of a validation batch.  Adding a term: its kernels and ops, a restatement under tests/, one
record here."""
from dataclasses import dataclass
from typing import Callable

import numpy as np


def _ops():
    from . import ops                                        # (lazily: the library is loaded by the first op that runs, not by an import)
    return ops


@dataclass(eq=False)                                         # (not frozen: a test may substitute a record's score_u8)
class Term:
    name: str
    train_flag: str                                          # the weight of the term in the generator's loss; 0 / absent: the term is off
    val_flag: str                                            # the Tester scores every validation pair with it
    all_attr: str                                            # the Tester attribute that holds the last run_validation's per-sample scores
    loss_key: str                                            # G_losses: lambda * to_loss(raw), shape (1,)
    log_key: str                                             # the loss log: raw, detached, viewed as log_shape
    raw: Callable                                            # (model, fake, target, seg) -> the unweighted term, a 0-dim tensor
    to_loss: Callable                                        # raw -> what lambda multiplies
    score_u8: Callable                                       # (fake_resized, target, data_i, opt) -> numpy, one row per sample
    summarise: Callable                                      # (all_scores, dataset_key, mode) -> {statistics key: float}; the keys begin with name
    fmt: str                                                 # how print_results prints the statistics whose keys begin with name
    prepare: Callable = lambda model, opt: None              # (model, opt): the constructor's part under train_flag, after the networks exist
    check: Callable = lambda opt: None                       # (opt): the constructor's part under train_flag, before the networks are built
    log_shape: tuple = ()
    row_shape: Callable = lambda opt: ()                     # the error-log dataset is (N,) + row_shape(opt)
    dtype = np.float64                                       # ... of this type, for every term so far

    @property
    def dataset(self):
        """The error log's dataset, the key of the Tester's score lists and of `_write_error_log_batch(scores=...)`."""
        return self.name


def _mean(dataset):
    def summarise(all_scores, dataset_key, mode):
        return {'%s/%s/%s' % (dataset, dataset_key, mode): float(np.mean(np.asarray(all_scores, dtype=np.float64)))}
    return summarise


def _similarity(s):
    return 1.0 - s                                           # (the mean similarity itself is logged: higher is better)


def _identity(v):
    return v


def _msssim_check(opt):
    # five levels halve the image four times and the last one must still hold an 11 x 11 window
    from .options import image_hw
    h, w = image_hw(opt)
    if min(h, w) < _ops().msssim_min_size():
        raise ValueError('--lambda_msssim: images of %d x %d are too small for five levels (H, W >= %d: the last level, %d x %d, must '
                         'hold an 11 x 11 window)' % (h, w, _ops().msssim_min_size(), h >> 4, w >> 4))


def _region_prepare(model, opt):
    # the class weights as the fp32 device tensor s2e_region_loss_fwd reads, made once -- a captured step reads the same address at
    # every replay
    import torch
    from .options import parse_region_weights
    model.region_w = torch.tensor(parse_region_weights(getattr(opt, 'region_weights', ''), opt.label_nc), dtype=torch.float32,
                                  device=model.device())


def _region_score_u8(fake_resized, target, data_i, opt):
    import torch
    label = torch.as_tensor(data_i['label']).to(fake_resized.device).to(torch.uint8)
    return _ops().region_stats_u8(fake_resized, target, label.unsqueeze(0) if label.dim() == 2 else label, opt.label_nc).cpu().numpy()


def _region_summarise(all_scores, dataset_key, mode):
    out = {}
    if len(all_scores):
        tot = np.sum(np.asarray(all_scores, dtype=np.float64), axis=0)                             # (label_nc, 3) over the scored samples
        for c in range(tot.shape[0]):
            if tot[c, 0] > 0:
                out['region_mae/%s/%s/%d' % (dataset_key, mode, c)] = float(tot[c, 1] / tot[c, 0])
                out['region_rmse/%s/%s/%d' % (dataset_key, mode, c)] = float(np.sqrt(tot[c, 2] / tot[c, 0]))
    return out


def _ffl_prepare(model, opt):
    # the DFT tables of the image size, built once and outside any graph capture -- a captured step reads the cached tables at every replay
    if model.device().type == 'cuda':
        from .options import image_hw
        _ops().ffl_tables(*image_hw(opt), model.device())


TERMS = (
    # structural similarity of the un-augmented fake and the target: two launches, one in the backward
    Term('ssim', 'lambda_ssim', 'val_ssim', 'all_ssim', 'SSIM/weighted', 'SSIM/raw',
         raw=lambda model, fake, target, seg: _ops().ssim(fake, target).mean(), to_loss=_similarity,
         score_u8=lambda fake_resized, target, data_i, opt: _ops().ssim_u8(fake_resized, target).cpu().numpy(),   # the same uint8 pair the error saw
         summarise=_mean('ssim'), fmt='%.4f'),
    # multi-scale structural similarity of the same pair: three launches, two in the backward
    Term('msssim', 'lambda_msssim', 'val_msssim', 'all_msssim', 'MSSSIM/weighted', 'MSSSIM/raw',
         raw=lambda model, fake, target, seg: _ops().ms_ssim(fake, target).mean(), to_loss=_similarity,
         score_u8=lambda fake_resized, target, data_i, opt: _ops().ms_ssim_u8(fake_resized, target).cpu().numpy(),
         summarise=_mean('msssim'), fmt='%.4f', check=_msssim_check),
    # class-balanced error of the same pair, keyed by the step's own label map: two launches, one in the backward
    Term('region', 'lambda_region', 'val_regions', 'all_regions', 'region/weighted', 'region/raw',
         raw=lambda model, fake, target, seg: _ops().region_loss(fake, target, seg.label, model.region_w,
                                                                 getattr(model.opt, 'region_norm', 'l1'))[0],
         to_loss=_identity, score_u8=_region_score_u8, summarise=_region_summarise, fmt='%.2f', prepare=_region_prepare, log_shape=(1,),
         row_shape=lambda opt: (opt.label_nc, 3)),
    # focal frequency loss of the same pair (lower is better): three launches, two in the backward; validation at alpha = 1
    Term('ffl', 'lambda_ffl', 'val_ffl', 'all_ffl', 'FFL/weighted', 'FFL/raw',
         raw=lambda model, fake, target, seg: _ops().focal_freq_loss(fake, target, getattr(model.opt, 'ffl_alpha', 1.0)).mean(),
         to_loss=_identity,
         score_u8=lambda fake_resized, target, data_i, opt: _ops().focal_freq_loss_u8(fake_resized, target, 1.0).cpu().numpy(),
         summarise=_mean('ffl'), fmt='%.3e', prepare=_ffl_prepare),
)
