#!/usr/bin/env python3
"""Training entry point, flag-compatible with the reference's train.py (train.py:23-116): same option names and defaults
(seg2eye_amd/options.py), same loop -- G step when `i % D_steps_per_G == 0`, then the D step -- same LR schedule,
same checkpoint files (`<checkpoints_dir>/<name>/<epoch>_net_{G,D,E}.pth`, reference state-dict keys; with `--ema_decay d` also
`<epoch>_net_{G,E}_ema.pth`, the averaged generator weights, which the validation passes then score) and `iter.txt`
resume record, same validation passes -- every `--display_freq` samples a quick one (`--validation_limit` samples), every
`--full_val_freq` samples a full one, on the train and validation splits, scored with the OpenEDS metric on the device
(seg2eye_amd/tester.py).  With `--visuals` the reference's Visualizer runs too (seg2eye_amd/visualizer.py): every loss and metric
line also goes to `loss_log.txt`, every quick validation writes side-by-side panels (style images | label map | ground truth |
generated image | error heat map, built on the GPU: DESIGN 3.12) as PNG files under `visuals/step<n>/`, and `--write_error_log`
gains the `visualisation` dataset.  Not carried over (out of scope): TF logging / HTML pages, source-tree copy.
Data: `--dataset_mode synthetic` (default) or `openeds` (an H5 file at `--dataroot`; needs h5py); with `--device_preprocess` the
OpenEDS frames are resized, flipped and normalised on the GPU, bit-identical to the host transform.
`--grad_clip_norm F` clips each optimizer's gradient to the global norm F and `--skip_nonfinite_grads` makes a step whose gradient
holds an inf / NaN change nothing, both inside the Adam step and without a host round trip; the progress line then
carries `grad_norm/{G,D}` and `grad_skipped/{G,D}`, and `--max_consecutive_skips` skipped steps in a row end the run with the
offending parameter's name -- `latest` is left as it was.
`--diffaug color,translation,cutout` (or a subset) augments what the discriminator sees -- fake and real alike, in the G step and in the D
step, fresh parameters before each, drawn from a CPU generator seeded `--diffaug_seed` + rank -- inside the launches that build D's input
(DESIGN 3.14); validation, the other loss terms and the saved images are untouched.

    python train.py --name run1 --batchSize 8 --aspect_ratio 1.0 --niter 1 --niter_decay 0
    python train.py --name run1 --batchSize 8 --aspect_ratio 1.0 --display_freq 1000 --visuals     # + loss_log.txt and PNG panels
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 --master-port 29500 train.py ...
"""
import contextlib
import sys
import traceback

import torch

from seg2eye_amd import distributed as dist
from seg2eye_amd.data import create_dataloader
from seg2eye_amd.iter_counter import IterationCounter
from seg2eye_amd.ops.preprocess import materialize
from seg2eye_amd.options import parse
from seg2eye_amd.pix2pix_trainer import Pix2PixTrainer
from seg2eye_amd.tester import Tester
from seg2eye_amd.visualizer import Visualizer


class NonFiniteGradients(RuntimeError):
    """--max_consecutive_skips steps in a row were skipped for non-finite gradients: the run ends and `latest` stays as it is."""


class TrainingRun:
    """The objects of one run and what is due around every iteration.  `fit()` walks the epochs; the per-iteration
    duties (progress line, quick / full validation, `latest` checkpoint) are a table of (is it due?, do it) pairs
    checked in the reference's order."""

    def __init__(self, opt, rank=0, world=1):
        self.opt, self.rank = opt, rank
        self.dataloader = create_dataloader(opt, rank, world)
        self.trainer = Pix2PixTrainer(opt)
        # samples per epoch AS THIS RANK COUNTS THEM (each rank sees 1/world of an epoch and counts its own samples, so the
        # cadences --print_freq / --save_latest_freq / ... are per-rank sample counts).  The reference passes len(dataloader) --
        # BATCHES -- while its counter advances in samples (train.py:33, util/iter_counter.py:13-31): the same number at its
        # batchSize 1; counting samples throughout keeps `iter.txt` resumes exact at any batch size.
        self.counter = IterationCounter(opt, len(self.dataloader) * opt.batchSize)
        self.world = world
        # validation runs on rank 0 only (it has no collectives); the reference keeps one tester per split
        self.visualizer = Visualizer(opt) if opt.visuals and rank == 0 else None      # (--visuals: one for the run, as in the reference)
        self.testers = [Tester(opt, dataset_key=split, visualizer=self.visualizer) for split in ('train', 'validation')] if rank == 0 else []
        c = self.counter
        self.duties = ((c.needs_printing, self.report), (c.needs_displaying, self.quick_validation),
                       (c.needs_saving, self.save_latest), (c.needs_full_validation, self.full_validation))
        self.epoch = c.current_epoch
        self._skips_seen = set()                                 # optimizers whose first skip has been announced

    # ---- duties
    def grad_health(self):
        """The guard's figures for the progress line -- read at --print_freq cadence only: no step waits for the host -- and the run's
        policy: announce each optimizer's first skip seen (with the parameter's name when the record still holds it), stop at --max_consecutive_skips.  Every rank decides alike (the guard's
        decision is a function of the exchanged gradient)."""
        health = self.trainer.grad_health()
        for tag, st in health.items():
            # (the record names the element only while the LAST step was a bad one: a clean step resets first_bad to -1)
            where = ' in %s (arena element %d)' % (st['param'], st['first_bad']) if st['first_bad'] >= 0 else ''
            if st['skipped'] and tag not in self._skips_seen:
                self._skips_seen.add(tag)
                if not self.rank:
                    print('optimizer %s skipped %d step(s) so far: non-finite gradient%s' % (tag, st['skipped'], where), flush=True)
            if 0 < self.opt.max_consecutive_skips <= st['consecutive']:
                raise NonFiniteGradients('optimizer %s skipped %d steps in a row (--max_consecutive_skips %d): non-finite gradient%s'
                                         % (tag, st['consecutive'], self.opt.max_consecutive_skips, where))
        return {'grad_%s/%s' % (k, tag): torch.tensor(float(health[tag][k])) for k in ('norm', 'skipped') for tag in ('G', 'D')}

    def report(self):
        health = self.grad_health() if self.trainer.has_guard else {}
        if self.rank:
            return
        c = self.counter
        losses = {**self.trainer.get_latest_losses(include_log_losses=True), **health}
        if self.visualizer is not None:
            self.visualizer.print_current_errors(self.epoch, c.total_steps_so_far, losses, c.time_per_iter)
            return self.visualizer.plot_current_errors(losses, c.total_steps_so_far)
        head = '(epoch: %d, iters: %d, time: %.3f) ' % (self.epoch, c.total_steps_so_far, c.time_per_iter)
        print(head + ' '.join('%s: %.3f' % (name, float(v.float().mean())) for name, v in losses.items()), flush=True)

    def _weights(self):
        """The weights a validation pass scores: the averaged ones (--ema_decay; trainer.ema_scope exchanges them in and restores
        the live ones and every buffer the pass moved) or the model as it is."""
        if self.testers and self.trainer.has_ema:            # (rank 0 only: its arenas are exchanged and restored locally)
            print('validating the averaged weights (ema_decay %g)' % self.opt.ema_decay, flush=True)
            return self.trainer.ema_scope()
        return contextlib.nullcontext()

    def quick_validation(self):
        # (the reference validates the model as it is: train mode.  solo: only rank 0 is here -- no per-layer exchange)
        with torch.no_grad(), dist.solo(), self._weights():
            for t in self.testers:
                t.run_partial_modes(model=self.trainer.pix2pix_model, epoch=self.epoch, n_steps=self.counter.total_steps_so_far,
                                    log=True, visualize_images=self.visualizer is not None, limit=self.opt.validation_limit)
        self.trainer.sync_replica_buffers()                      # rank 0's train-mode pass advanced its u, v / BN statistics

    def full_validation(self):
        with torch.no_grad(), dist.solo(), self._weights():
            for t in self.testers:
                t.run(self.trainer.pix2pix_model, mode='full', epoch=self.epoch, n_steps=self.counter.total_steps_so_far,
                      log=True, write_error_log=self.opt.write_error_log)
        self.trainer.sync_replica_buffers()

    def save_latest(self):
        if self.rank:
            return
        print('saving the latest model (epoch %d, total_steps %d)' % (self.epoch, self.counter.total_steps_so_far))
        self.trainer.save('latest')
        self.counter.record_current_iter()

    # ---- the loop
    def one_epoch(self, epoch):
        c, trainer = self.counter, self.trainer
        self.epoch = epoch
        if c.current_epoch != epoch:                             # equal only at the very start and right after a resume
            c.record_epoch_start(epoch)
        sampler = getattr(self.dataloader, 'sampler', None)
        if hasattr(sampler, 'set_epoch'):
            sampler.set_epoch(epoch)                             # (DistributedSampler: a new permutation per epoch)
        for i, batch in enumerate(self.dataloader, start=c.epoch_iter):
            c.record_one_iteration()
            batch = materialize(batch, self.opt, trainer.pix2pix_model.device())     # (--device_preprocess: once, before both steps)
            if i % self.opt.D_steps_per_G == 0:
                trainer.run_generator_one_step(batch)
            trainer.run_discriminator_one_step(batch)
            for due, act in self.duties:
                if due():
                    act()
        trainer.update_learning_rate(epoch)
        c.record_epoch_end(write=self.rank == 0)
        if self.rank == 0 and (epoch % self.opt.save_epoch_freq == 0 or epoch == c.total_epochs):
            print('saving the model at the end of epoch %d, iters %d' % (epoch, c.total_steps_so_far))
            trainer.save('latest')
            trainer.save(epoch)

    def fit(self):
        keep_latest = False
        try:
            for epoch in self.counter.training_epochs():
                self.one_epoch(epoch)
            print('Training was successfully finished.')
        except (KeyboardInterrupt, SystemExit):
            print('KeyboardInterrupt. Shutting down.')
            print(traceback.format_exc())
        except NonFiniteGradients:
            keep_latest = True                                   # the last good checkpoint is worth more than this state
            raise
        finally:
            if self.rank == 0 and not keep_latest:
                print('saving the model before quitting')
                self.trainer.save('latest')
                self.counter.record_current_iter()
        return self.trainer


def main(argv=None):
    opt = parse(argv, is_train=True)
    rank, world, local = dist.init_from_env()
    if torch.cuda.is_available():
        dev = local % max(torch.cuda.device_count(), 1)          # (== local on a full node; a 2-rank gloo run may share one GPU)
        opt.gpu_ids = [dev]
        torch.cuda.set_device(dev)
    return TrainingRun(opt, rank, world).fit()


if __name__ == '__main__':
    main(sys.argv[1:])
