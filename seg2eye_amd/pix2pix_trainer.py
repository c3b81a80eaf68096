"""Pix2PixTrainer (reference trainers/pix2pix_trainer.py:8-88): owns the model and the two optimizers,
runs one G step / one D step, LR decay, save.  Multi-GPU: when torch.distributed is initialised the
flat gradient arenas are sum-all-reduced (RCCL) between backward and the Adam launch."""
import contextlib
import os

from . import diffaug
from .distributed import FlatGradSync, broadcast_buffers, broadcast_flat, exchange_active, world_size
from .ops import ZeroPool
from .pix2pix_model import Pix2PixModel


def _total(losses):
    """sum(losses.values()).mean() (trainers/pix2pix_trainer.py:31,41) without the launches that change nothing: no `0 + l` to
    start the sum, no mean over a single element."""
    vals = list(losses.values())
    t = vals[0]
    for v in vals[1:]:
        t = t + v
    return t.view(()) if t.numel() == 1 else t.mean()


class _StepGraph:
    """One captured step body: a single hipGraph, or a chain of segments cut where a gradient group completes
    (`groups[k]` = the arena group that is final after segment k)."""

    def __init__(self, segments, groups):
        self.segments, self.groups = segments, groups

    def pool(self):
        return self.segments[0].pool()

    def replay(self, launch=None):
        for k, g in enumerate(self.segments):
            g.replay()
            if launch is not None and k < len(self.groups):
                launch(self.groups[k])


class Pix2PixTrainer:
    def __init__(self, opt):
        self.opt = opt
        self.pix2pix_model = Pix2PixModel(opt)
        self.pix2pix_model_on_one_gpu = self.pix2pix_model
        self.generated = None
        self.g_losses, self.d_losses = {}, {}
        self._static, self.graph_G, self.graph_D = None, None, None
        self.pool = ZeroPool(self.pix2pix_model.device())    # this trainer's zero-filled scratch + deferred gradient re-layouts
        self.diffaug = self.pix2pix_model.diffaug            # --diffaug: the enabled parts (empty: off -- nothing below exists)
        if self.diffaug:
            # the sampler's own CPU generator, seeded per replica (each draws its own rows; nothing is exchanged), and the ONE device
            # buffer the rows of every full-size step are copied into -- under hipGraphs a further static input of both graphs
            import torch
            from .distributed import get_rank
            self._aug_gen = torch.Generator().manual_seed(int(getattr(opt, 'diffaug_seed', 0) or 0) + get_rank())
            self._aug_rows = None
        if opt.isTrain:
            self.optimizer_G, self.optimizer_D = self.pix2pix_model_on_one_gpu.create_optimizers(opt)
            self.old_lr = opt.lr
            how = dict(payload=getattr(opt, 'grad_dtype', 'fp32'), algorithm=getattr(opt, 'grad_exchange', 'allreduce'))
            self.sync_G = FlatGradSync(self.optimizer_G.flat_g, groups=self.pix2pix_model.grad_groups_G, **how)
            self.sync_D = FlatGradSync(self.optimizer_D.flat_g, **how)
            self._segments = None                            # while the G step is being captured in segments: (graphs, groups, mode)
            self._quiet_hooks = False                        # capture warm-up passes: hooks flush but exchange nothing
            if exchange_active() and not getattr(opt, 'no_overlap_allreduce', False):
                # Overlap the gradient exchange with the backward pass: the generator reports when a group of
                # blocks has all its gradients (networks/generator.py); we flush that group's queued gradient re-layouts and
                # start the all-reduce of its arena slice.  With --hip_graphs the G step is captured as one graph SEGMENT per
                # group (round 4): a hook that fires during capture ends the current segment and begins the next, and a replayed
                # step is `replay segment k; start group k's all-reduce` -- the collective runs on the backend's stream while the
                # next segment replays.  (Rounds 1-3 had to choose: eager launches + overlap, or graphs + one exposed exchange.)
                self.pix2pix_model.netG.__dict__['grad_ready'] = self._group_ready
            if exchange_active() and 'batch' in str(getattr(opt, 'norm_G', '')) and getattr(opt, 'hip_graphs', False):
                # BatchNorm SPADE under data parallelism exchanges its batch statistics between the replicas INSIDE every forward
                # and backward (normalization.py::spade_stats): a collective cannot be captured into a hipGraph (gloo synchronises
                # the stream on the host; attempting it took the process down), so these runs launch eagerly
                from .distributed import get_rank
                if get_rank() == 0:
                    import sys
                    print('seg2eye_amd: --norm_G %s with %d replicas exchanges batch statistics inside the step: the steps run '
                          'as individual launches (no hipGraphs)' % (opt.norm_G, world_size()), file=sys.stderr)
                self.opt.hip_graphs = False
            if self.optimizer_G.has_ema and opt.continue_train:
                self._load_ema()
            broadcast_flat(self.optimizer_G.flat_p)          # identical replicas at step 0: parameters ...
            broadcast_flat(self.optimizer_D.flat_p)
            if self.optimizer_G.has_ema:
                broadcast_flat(self.optimizer_G.flat_ema)    # ... their average (from here on every replica computes the same one) ...
            self.sync_replica_buffers()                      # ... and spectral-norm u, v / BatchNorm running statistics

    def sync_replica_buffers(self):
        """Every replica takes rank 0's spectral-norm u, v and BatchNorm running buffers (no-op on one process).  Called at
        construction and by train.py after rank 0 alone ran a validation pass: that pass runs in train mode (the reference never
        calls eval()) and so advances rank 0's u, v and running statistics."""
        m = self.pix2pix_model
        broadcast_buffers([m.netG, m.netD, m.netE])

    def _group_ready(self, i):
        """Backward hook (data parallel): parameter group i of the G arena is final.  Only during the G step's backward --
        the D step's no-grad generator forward registers no hooks."""
        pool = ZeroPool.active()
        if pool is not self.pool or pool.key != 'G':
            return
        pool.sink.flush()                                    # the group's queued packed-dW -> arena conversions: now
        if self._segments is not None:
            self._next_segment(i)                            # capturing: the segment ends here, replay launches the exchange
        elif not self._quiet_hooks:
            self.sync_G.launch(i)

    def _next_segment(self, group):
        import torch
        segs, groups, mode = self._segments
        segs[-1].capture_end()
        groups.append(group)
        g = torch.cuda.CUDAGraph()
        g.capture_begin(pool=segs[0].pool(), capture_error_mode=mode)
        segs.append(g)

    def _train_mode(self):
        """model.train() -- when something put it or ANY of its modules into eval mode (a validation pass, a caller freezing one
        SPADE block: spectral norm's power iteration and BatchNorm's running statistics stop there).  Reading the ~260 cached
        flags costs ~15 us; walking `modules()` to see whether the module LIST changed (a module added or replaced
        later must be seen) costs a few hundred us, so that walk runs on the first call and then every 64th --
        `invalidate_modules()` forces it at once."""
        mods = self.__dict__.get('_all_modules')
        tick = self.__dict__['_mode_tick'] = self.__dict__.get('_mode_tick', 0) + 1
        if mods is None or tick % 64 == 1:
            now = list(self.pix2pix_model.modules())
            if mods is None or len(mods) != len(now) or any(a is not b for a, b in zip(mods, now)):
                mods = self.__dict__['_all_modules'] = now
        if not all(x.training for x in mods):
            self.pix2pix_model.train()

    def invalidate_modules(self):
        """Call after adding / replacing a module of the model: the next step re-reads the module list."""
        self.__dict__.pop('_all_modules', None)

    def _one(self):
        """d(total)/d(total) as a persistent device scalar (autograd would launch a ones_like per backward)."""
        t = self.__dict__.get('_one_t')
        if t is None:
            import torch
            t = self.__dict__['_one_t'] = torch.ones((), dtype=torch.float32, device=self.pix2pix_model.device())
        return t

    # ---- step bodies: zero_grad + forward + backward (what a hipGraph captures) -------------------
    def _g_body(self, data):
        self.optimizer_G.zero_grad()
        try:
            with self.pool.scope('G'):                           # all zero-filled scratch of the step: one fill
                g_losses, generated = self.pix2pix_model(data, mode='generator')
                _total(g_losses).backward(self._one())
        except BaseException:
            self.sync_G.reset()                                  # exchanges the backward hooks started for a step that failed
            raise
        # keep detached copies only: a live autograd graph would pin last iteration's AccumulateGrad nodes
        # (and their stream), which breaks hipGraph capture
        self.g_losses = {k: v.detach() for k, v in g_losses.items()}
        self.generated = generated.detach()

    def _d_body(self, data):
        self.optimizer_D.zero_grad()
        with self.pool.scope('D'):
            d_losses = self.pix2pix_model(data, mode='discriminator')
            _total(d_losses).backward(self._one())
        self.d_losses = {k: v.detach() for k, v in d_losses.items()}

    def _hand_rows(self, data):
        """--diffaug: draw this step's rows and hand them to the model (Pix2PixModel.discriminate).  Called BEFORE the inputs are
        staged, with and without hipGraphs: the capture (inside _stage_inputs) and its warm-up passes then read the buffer as it
        stands and draw nothing, so a run draws the same sequence either way.  The rows go into the persistent buffer (what a
        replay reads); a batch of another size -- an epoch's ragged last one, which runs eagerly -- gets rows of its own size."""
        label = data['label']
        n, (H, W) = label.shape[0], label.shape[-2:]
        rows = diffaug.sample(self.diffaug, n, H, W, self._aug_gen)
        if self._aug_rows is None:
            self._aug_rows = rows.to(self.pix2pix_model.device())
        elif self._aug_rows.shape[0] == n:
            self._aug_rows.copy_(rows, non_blocking=True)
        else:
            self.pix2pix_model.diffaug_rows = rows.to(self.pix2pix_model.device())
            return
        self.pix2pix_model.diffaug_rows = self._aug_rows

    def run_generator_one_step(self, data):
        """trainers/pix2pix_trainer.py:26-35.  With opt.hip_graphs the body is one graph replay."""
        if self.__dict__.get('_in_ema_scope'):
            raise RuntimeError('a generator step inside ema_scope() would train the averaged weights')
        self._train_mode()
        data = self._materialized(data)
        if self.diffaug:
            self._hand_rows(data)
        if self.use_graphs and self._stage_inputs(data):     # (captures on first use; turns graphs off if that fails)
            self.graph_G.replay(self.sync_G.launch)          # (segment k, then group k's exchange beside segment k+1)
            for k, v in getattr(self, '_static_log', {}).items():   # the replay refreshed these in place: log this step's values
                self.pix2pix_model.add_to_loss_log(k, v.clone())
        else:
            self._g_body(data)
        if self.diffaug:
            self.pix2pix_model.diffaug_rows = None           # (outside a step nothing augments)
        self.optimizer_G.step(grad_scale=self.sync_G.all_reduce())

    def run_discriminator_one_step(self, data):
        """trainers/pix2pix_trainer.py:37-45."""
        self._train_mode()
        data = self._materialized(data)
        if self.diffaug:
            self._hand_rows(data)
        if self.use_graphs and self._stage_inputs(data):
            self.graph_D.replay()
        else:
            self._d_body(data)
        if self.diffaug:
            self.pix2pix_model.diffaug_rows = None
        self.optimizer_D.step(grad_scale=self.sync_D.all_reduce())

    def _materialized(self, data):
        """--device_preprocess: a raw batch becomes the standard one on the GPU (ops.preprocess.materialize; train.py does this once
        per batch, before both steps); every other batch comes back as it is."""
        from .ops.preprocess import materialize
        return materialize(data, self.opt, self.pix2pix_model.device())

    # ---- hipGraph capture ---------------------------------------------------------------------------
    @property
    def use_graphs(self):
        return bool(getattr(self.opt, 'hip_graphs', False))

    def _stage_inputs(self, data):
        """Copy the batch into the static input buffers the graphs read (capturing on first use).  True: replay.  False: this
        step runs as individual launches -- the capture failed (graphs are off from now on), or this batch has another shape
        than the one the graphs were captured for (they stay for the batches that have it)."""
        if self._static is None:
            try:
                self._capture(data)
            except Exception as e:                           # noqa: BLE001 -- any capture failure: run eager instead
                # Eager runs the same kernels (10 % slower on a slow host: DESIGN 6); a failed capture must not take a multi-GPU
                # job down.  The step that triggered the capture has not run yet.
                import sys
                import torch
                print('seg2eye_amd: hipGraph capture failed (%s: %s) -- continuing without graphs' % (type(e).__name__, e),
                      file=sys.stderr)
                if os.environ.get('S2E_DEBUG_CAPTURE'):
                    import traceback
                    traceback.print_exc()
                torch.cuda.synchronize()
                self.opt.hip_graphs = False
                self._static, self.graph_G, self.graph_D = None, None, None
                self.pool.unfreeze()
                return False
        if any(tuple(data[k].shape) != tuple(buf.shape) for k, buf in self._static.items()):
            return False                                     # (an epoch's ragged last batch: this step runs as individual launches)
        for k, buf in self._static.items():
            src = data[k]
            if src.data_ptr() != buf.data_ptr():
                buf.copy_(src, non_blocking=True)
        return True

    def _capture(self, data):
        import torch
        m = self.pix2pix_model
        dev = m.device()
        self._static = {k: data[k].to(dev).clone() for k in ('label', 'style_image', 'target')}
        # the warm-up passes run the spectral-norm power iterations for real: snapshot every bank's u|v
        # arena and put it back afterwards so capturing does not change the training trajectory (weights
        # are untouched: the bodies contain no optimizer step)
        from .spectral import ensure_bank
        banks = [b for b in (ensure_bank(net) for net in (m.netG, m.netD, m.netE)) if b is not None]
        snap = [b.uv_arena.clone() for b in banks]
        # ... and so do BatchNorm's running statistics (--norm_G spectralspadebatch3x3, the reference's default)
        bn_bufs = [t for net in (m.netG, m.netD, m.netE) for mod in net.modules()
                   if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm) and mod.track_running_stats
                   for t in (mod.running_mean, mod.running_var, mod.num_batches_tracked)]
        bn_snap = [t.clone() for t in bn_bufs]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        self._quiet_hooks = True                             # (the warm-up passes exchange nothing: every rank runs them alike)
        try:
            with torch.cuda.stream(side):
                for _ in range(2):
                    self._g_body(self._static)
                    self._d_body(self._static)
        finally:
            self._quiet_hooks = False
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.pool.freeze()                                   # the graphs hold raw pointers into the pool
        # With a process group up, RCCL's watchdog thread polls events while we capture: only calls made by the
        # capturing threads may invalidate the capture (the collectives themselves stay outside the graphs).
        multi = torch.distributed.is_available() and torch.distributed.is_initialized()
        mode = {'capture_error_mode': 'thread_local'} if multi else {}
        # No CYCLIC garbage collection while capturing: a collection that happens to start inside the captured body may destroy
        # objects of an earlier trainer (hipGraph executables, streams) -- runtime calls a capture does not survive: the full test suite
        # aborted once in "Garbage-collecting" under _g_body.  Reference counting frees everything else as always.
        import gc
        gc.collect()
        gc_was = gc.isenabled()
        gc.disable()
        try:
            if m.netG.__dict__.get('grad_ready') is not None:
                graph_G = self._capture_segmented(self._g_body, mode.get('capture_error_mode', 'global'))
            else:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, **mode):
                    self._g_body(self._static)
                graph_G = _StepGraph([g], [])
            graph_D = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph_D, pool=graph_G.pool(), **mode):
                self._d_body(self._static)
            self.graph_G, self.graph_D = graph_G, graph_D
        finally:
            if gc_was:
                gc.enable()
            with torch.no_grad():
                for b, s0 in zip(banks, snap):
                    b.uv_arena.copy_(s0)
                for t, s0 in zip(bn_bufs, bn_snap):
                    t.copy_(s0)
            # the '*/raw' log entries (pix2pix_model.add_to_loss_log) appended while capturing are the graph's static output
            # tensors: remember them, a replay refreshes their values and run_generator_one_step re-registers them
            self._static_log = {k: v[-1] for k, v in m.loss_log.items() if len(v)}
            m.reset_loss_log()

    def _capture_segmented(self, body, mode):
        """Capture `body` as a chain of hipGraphs that share one memory pool: `_group_ready` -- a backward hook -- closes the
        current segment and opens the next wherever a gradient group completes.  The backward runs on THIS thread while
        capturing (autograd's device thread would end a capture another thread began)."""
        import gc
        import torch
        torch.cuda.synchronize()
        gc.collect()
        torch.cuda.empty_cache()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        segs, groups = [torch.cuda.CUDAGraph()], []
        with torch.cuda.stream(stream), torch.autograd.set_multithreading_enabled(False):
            segs[0].capture_begin(capture_error_mode=mode)
            self._segments = (segs, groups, mode)
            try:
                body(self._static)
            except BaseException:
                self._segments = None
                try:
                    segs[-1].capture_end()                   # (an already invalidated capture raises here: keep the FIRST error)
                except Exception:                            # noqa: BLE001
                    pass
                raise
            self._segments = None
            segs[-1].capture_end()
        torch.cuda.current_stream().wait_stream(stream)
        return _StepGraph(segs, groups)

    def get_latest_losses(self, include_log_losses=False):
        losses = {**self.g_losses, **self.d_losses}
        if include_log_losses:
            losses = {**losses, **self.pix2pix_model_on_one_gpu.get_loss_log()}
            self.pix2pix_model_on_one_gpu.reset_loss_log()
        return losses

    def get_latest_generated(self):
        return self.generated

    def save(self, epoch):
        self.pix2pix_model_on_one_gpu.save(epoch, ema_of=self._ema_of() if self.has_ema else None)

    # ---- the gradient guard (--grad_clip_norm / --skip_nonfinite_grads) -----------------------
    @property
    def has_guard(self):
        return bool(self.opt.isTrain and self.optimizer_G.has_guard)

    def grad_health(self):
        """{'G': optimizer_G.guard_stats(), 'D': optimizer_D.guard_stats()} plus, per optimizer, 'param': the state-dict name of
        the parameter that owns the first non-finite gradient element (e.g. 'netG.up_0.conv_1.weight_orig'; None when the last
        gradient was finite or the element lies in an alignment gap).  Two small device-to-host copies: for the progress line, not
        for every step.  The guard itself sits inside FlatAdam.step(), after the gradient exchange."""
        if not self.has_guard:
            raise RuntimeError('grad_health: this trainer has no gradient guard (--grad_clip_norm 0, no --skip_nonfinite_grads)')
        names = self.__dict__.get('_param_names')
        if names is None:
            m = self.pix2pix_model
            names = self.__dict__['_param_names'] = {id(p): '%s.%s' % (tag, k) for tag, net in (('netG', m.netG), ('netE', m.netE), ('netD', m.netD))
                                                     for k, p in net.named_parameters()}
        out = {}
        for tag, o in (('G', self.optimizer_G), ('D', self.optimizer_D)):
            st = o.guard_stats()
            i = o.param_at(st['first_bad']) if st['first_bad'] >= 0 else None
            st['param'] = names.get(id(o.params[i])) if i is not None else None
            out[tag] = st
        return out

    # ---- averaged generator weights (--ema_decay) ------------------------------------------
    @property
    def has_ema(self):
        return bool(self.opt.isTrain and self.optimizer_G.has_ema)

    def _ema_of(self):
        """{id(parameter): its averaged value} over optimizer G's parameters (netG + netE)."""
        og = self.optimizer_G
        return {id(p): e for p, e in zip(og.params, og.ema_views())}

    def _load_ema(self):
        """--continue_train: `<which_epoch>_net_{G,E}_ema.pth` into the average when both exist; otherwise the average restarts
        from the loaded live weights (flat_ema is a copy of flat_p at construction).  Either way --ema_start counts from the
        resume: it is compared with the optimizer's own step count, which restarts at 0 like the moments."""
        from . import checkpoint
        m, opt = self.pix2pix_model, self.opt
        if checkpoint.ema_files_exist(opt.which_epoch, opt):
            ema_of = self._ema_of()
            checkpoint.load_ema(m.netG, 'G', opt.which_epoch, opt, ema_of)
            checkpoint.load_ema(m.netE, 'E', opt.which_epoch, opt, ema_of)
        else:
            print('seg2eye_amd: no averaged checkpoint (%s_net_{G,E}_ema.pth) to resume from: the average restarts from the '
                  'loaded weights' % opt.which_epoch, flush=True)

    @contextlib.contextmanager
    def ema_scope(self):
        """Inside: netG / netE's parameters hold the averaged values; on exit the live ones again, bit for bit.
        The CONTENTS of flat_p and flat_ema are exchanged (the parameters alias flat_p and captured graphs hold its address).
        Nothing derived from the weights outlives the exchange: sigma and the weight packs are recomputed from the masters at
        the top of every forward (spectral.sn_begin, packing.PackPlan.run), the SPADE prepass and the style bank keep addresses,
        not values.  Buffers outside the arena -- spectral-norm u|v, BatchNorm running statistics -- are shared with the live
        network; since a pass may run in TRAIN mode here (train.py's validation does) and would move them, they are snapshotted
        on entry and put back on exit, as `_capture` does around its warm-up passes: a pass on the averaged weights leaves no
        trace in the live training state.  Not re-entrant; no optimizer step inside."""
        if not self.has_ema:
            raise RuntimeError('ema_scope: this trainer keeps no averaged weights (--ema_decay 0)')
        if self.__dict__.get('_in_ema_scope'):
            raise RuntimeError('ema_scope is not re-entrant')
        import torch
        from .spectral import ensure_bank
        m = self.pix2pix_model
        nets = (m.netG, m.netE)
        bufs = [b.uv_arena for b in (ensure_bank(net) for net in nets) if b is not None]
        bufs += [t for net in nets for mod in net.modules()
                 if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm) and mod.track_running_stats
                 for t in (mod.running_mean, mod.running_var, mod.num_batches_tracked)]
        snap = [t.clone() for t in bufs]
        self.optimizer_G.swap_ema()
        self._in_ema_scope = True
        try:
            yield self
        finally:
            self._in_ema_scope = False
            self.optimizer_G.swap_ema()
            with torch.no_grad():
                for t, s0 in zip(bufs, snap):
                    t.copy_(s0)

    def update_learning_rate(self, epoch):
        """Constant for niter epochs, then linear to 0 over niter_decay, keeping TTUR's 1/2 : 2 ratio
        (pix2pix_trainer.py:68-88)."""
        if epoch > self.opt.niter:
            new_lr = self.old_lr - self.opt.lr / self.opt.niter_decay
        else:
            new_lr = self.old_lr
        if new_lr != self.old_lr:
            new_lr_G, new_lr_D = (new_lr, new_lr) if self.opt.no_TTUR else (new_lr / 2, new_lr * 2)
            for g in self.optimizer_D.param_groups:
                g['lr'] = new_lr_D
            for g in self.optimizer_G.param_groups:
                g['lr'] = new_lr_G
            print('update learning rate: %f -> %f' % (self.old_lr, new_lr))
            self.old_lr = new_lr
