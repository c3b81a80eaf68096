"""The trainer step's queues of deferred weight-side launches (GradSink): what a backward would launch layer by layer -- weight
gradients, spectral norm's chain rule, the re-layout of packed gradients into the arena -- is queued inside a ZeroPool scope and run
as one or two launches per queue at the flush.  One record type per queue; the sink owns what a scope's start, flush and failure do
to them.

core.py and this module need each other (a ZeroPool creates its sink; the sink asks ZeroPool.active() / grad_is_fresh): this module
imports core at its top, ZeroPool.__init__ imports GradSink locally."""
import ctypes as C
from collections import namedtuple

import torch

from .. import _lib as L
from . import switches
from .core import LaunchProfiler, ZeroPool, _cl_rows, _need, _p, _stream, device_job_table, memo


def _overlap(a, b):
    """Do tensors a and b share a byte of the same storage?  (The byte range of a strided tensor: from its first element to its
    last, gaps included -- conservative for interleaved views.)"""
    if a.numel() == 0 or b.numel() == 0:
        return False

    def span(t):
        lo = t.data_ptr()
        n = t.numel() if t.is_contiguous() else sum((k - 1) * s for k, s in zip(t.shape, t.stride())) + 1
        return lo, lo + n * t.element_size()
    alo, ahi = span(a)
    blo, bhi = span(b)
    return alo < bhi and blo < ahi and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()


def _p0(t):
    return 0 if t is None else t.data_ptr()


# ------------------------------------------------------------------------------ one record per queue
# `jobs`: packed dW -> OIHW arena slice; with w_orig / u / v / sigma, through spectral norm's chain rule (push)
RelayoutJob = namedtuple('RelayoutJob', 'dwp dst w_orig u v sigma cout cin taps cin_pad')
# `inplace`: spectral norm's chain rule applied in place to the channels-last gradient slice g (push_inplace)
InplaceJob = namedtuple('InplaceJob', 'g w u v sigma rows cin taps')
# `gwg`: a generic weight gradient (push_gwg); desc: the ConvDesc fields of the forward conv
GwgJob = namedtuple('GwgJob', 'x gy dw dbias desc')
# `c8`: mlp_shared's weight gradient against the 8-channel one-hot map (push_c8)
C8Job = namedtuple('C8Job', 'oh dactv dw db ncls rects')
# `uni`: the uniform rectangles' closed-form gradients of a label-sparse SPADE backward (push_uniform)
UniformJob = namedtuple('UniformJob', 'R A w_gb w_sh b_sh dw_sh db_sh dw_gb db_gb c2 nh ncls act_bf16')


class WgradJob:
    """`wg`: a patch-resident 3x3 weight gradient (push_wgrad).  Not a tuple: `fresh` (store, do not add) is cleared when the same dW
    receives another contribution before the flush."""
    __slots__ = ('x', 'gy', 'dw', 'dbias', 'rects', 'fresh')

    def __init__(self, x, gy, dw, dbias, rects, fresh):
        self.x, self.gy, self.dw, self.dbias, self.rects, self.fresh = x, gy, dw, dbias, rects, fresh


def _wgrad_batch_ok(key):
    n, h, w, cin, cout, sparse = key
    return bool(L.call.s2e_wgrad_batch_supported(L.S2E_BF16, n, h, w, cin, cout)) and (not sparse or (h % 16 == 0 and w % 16 == 0))


def _wgrad_multi_ok(desc_key):
    d = L.ConvDesc(*desc_key)
    return bool(L.call.s2e_conv2d_wgrad_multi_supported(L.S2E_BF16, d))


class GradSink:
    """Inside a ZeroPool scope (a trainer step) the per-layer "packed dW -> OIHW gradient arena" conversions -- plain
    re-layout, or the spectral-norm chain rule dW_orig = (dW - <dW, W_sn> u v^T)/sigma -- are not launched one by one
    (~95 launches of a few microseconds of work each, 1.2 ms per step) but queued and done by TWO launches at scope
    exit (`s2e_weight_grads_batched`); the weight gradients themselves are queued likewise (push_wgrad, push_gwg, push_c8,
    push_uniform, push_inplace).  The packed buffers are ZeroPool slices, alive until the next scope.  The
    device job tables are cached by content: in steady state (and always under a hipGraph) every pointer repeats.
    One sink per pool (= per trainer)."""

    # The queues, in the order a flush must run them (queue attribute, its method).  __init__, flush and abort all walk this table:
    # a queue is a row here, and with that an aborted step drops it.  Every queue `q` has `keep_q`: the jobs of its last flush, whose
    # tensors stay referenced until that queue's next flush (stream order covers the rest).
    ORDER = (
        ('wg', '_flush_wgrad'),         # batched patch-resident 3x3 weight gradients, first: the re-layout / chain-rule / rank-1 jobs below
                                        # read or add to its results (and a `fresh` job STORES its tiles)
        ('gwg', '_flush_gwg'),          # generic multi-job weight gradients: likewise, their dW buffers feed the re-layout / chain-rule jobs
        ('uni', '_flush_uniform'),      # uniform rectangles' rank-1 parts: added to the [gamma | beta] dW that `wg` has written by now
        ('c8', '_flush_c8'),            # 8-channel batch: adds to mlp_shared's gradients, as `uni` did (float sums: the order is kept)
        ('inplace', '_flush_inplace'),  # in-place chain rules: each rewrites an arena slice that must hold the step's finished raw sum
        ('jobs', '_flush_relayout'),    # re-layout / chain-rule table: reads the packed dW buffers, finished by `wg` / `gwg`
    )

    def __init__(self):
        for q, _ in self.ORDER:
            setattr(self, q, [])
            setattr(self, 'keep_' + q, None)
        self.inplace_done = set()  # gradient slices whose chain rule has already RUN in the open scope (see inplace_allowed)
        self.wg_done = set()       # dW slices a wgrad flush of the open scope has already written (a later job must ADD to them)
        self.tables = {}           # (queue, content key) -> device job table: _table
        self.wg_ws = None          # workspace of the batched patch launch (kept: the same ~216 MiB every flush)
        self.gwg_ws = None         # workspace of the multi-job generic launch

    # ------------------------------------------------------------------ the scope's life cycle (ZeroPool calls these)
    def begin_scope(self):
        self.inplace_done = set()
        self.wg_done = set()

    def flush(self):
        """Run everything queued, in ORDER.  At scope exit, and from Pix2PixTrainer._group_ready when a gradient group is complete."""
        for q, run in self.ORDER:
            if getattr(self, q):
                getattr(self, run)()

    def abort(self):
        """The step failed: drop every queued job (and with it the tensors it holds); nothing of this scope runs in a later one."""
        for q, _ in self.ORDER:
            setattr(self, q, [])

    def _table(self, queue, key, build):
        ent = self.tables.get((queue, key))
        if ent is None:
            ent = build()
            if len(self.tables) > 64:                        # (a step flushes once per all-reduce group: up to 2 x 7 tables + the in-place ones;
                self.tables.clear()                          #  a table rebuilt inside a hipGraph capture would be a host-to-device copy there)
            self.tables[(queue, key)] = ent
        return ent

    # ------------------------------------------------------------------ re-layout / chain rule of packed gradients
    @staticmethod
    def push(dwp, dst, cout, cin, taps, cin_pad, w_orig=None, u=None, v=None, sigma=None):
        """True if queued (caller must not touch dst until flush); False: no scope active, do it now."""
        pool = ZeroPool.active()
        if pool is None:
            return False
        pool.sink.jobs.append(RelayoutJob(dwp, dst, w_orig, u, v, sigma, int(cout), int(cin), int(taps), int(cin_pad)))
        return True

    def _flush_relayout(self):
        jobs, self.jobs = self.jobs, []
        dev = jobs[0].dwp.device
        key = tuple((j.dwp.data_ptr(), j.dst.data_ptr(), _p0(j.w_orig), _p0(j.u), _p0(j.v), _p0(j.sigma), j.cout, j.cin, j.taps, j.cin_pad)
                    for j in jobs)

        def build():
            arr = (L.GradJob * len(jobs))()
            nsn = 0
            for a, j in zip(arr, jobs):
                a.gw_packed, a.out = j.dwp.data_ptr(), j.dst.data_ptr()
                a.cout, a.cin, a.taps, a.cin_pad = j.cout, j.cin, j.taps, j.cin_pad
                if j.w_orig is not None:
                    a.w_orig, a.u, a.v, a.sigma, a.dot_index = j.w_orig.data_ptr(), j.u.data_ptr(), j.v.data_ptr(), j.sigma.data_ptr(), nsn
                    nsn += 1
                else:
                    a.dot_index = -1
            return device_job_table(arr, lambda bm: L.call.s2e_grad_block_map(C.byref(arr), len(jobs), bm), 3, dev) \
                + (max(j.taps for j in jobs), nsn)
        jobs_dev, map_dev, nb, max_taps, nsn = self._table('jobs', key, build)
        dots = ZeroPool.take(max(nsn, 1), torch.float32, dev)
        LaunchProfiler.run(
            'weight_grad_relayout', 0.0, L.call.s2e_weight_grads_batched,
            (jobs_dev.data_ptr(), map_dev.data_ptr(), nb, max_taps, int(nsn > 0), dots.data_ptr(), _stream()),
            nbytes=lambda: float(sum(j.dwp.numel() * 4 * (3 if j.w_orig is not None else 2) + (j.dwp.numel() * 4 if j.w_orig is not None else 0)
                                     for j in jobs)))
        self.keep_jobs = jobs

    # ------------------------------------------------------------------ in-place chain rule (channels-last masters)
    @staticmethod
    def inplace_allowed(wdst):
        """May the weight-gradient kernel accumulate a SPECTRAL-NORMED layer's raw gradient straight into `wdst` (its channels-
        last .grad), to be rewritten in place by the chain rule g <- g/sigma - (<g, W>/sigma^2) u v^T at the next flush?  The
        rewrite equals "accumulate the chain-ruled gradient" only if wdst held ZEROS before this step's contributions and the
        rule runs ONCE over their sum (it is linear in g).  So: inside a trainer step (ZeroPool scope) whose gradient arena
        zero_grad cleared right before the scope, and not after this slice's rule has already run in the scope (a second
        backward behind a flush).  Everything else -- stand-alone ops, gradient accumulation over several backwards, plain
        .grad tensors -- takes the packed scratch + accumulate path."""
        pool = ZeroPool.active()
        return pool is not None and ZeroPool.grad_is_fresh(wdst) and wdst.data_ptr() not in pool.sink.inplace_done

    @staticmethod
    def push_inplace(g_rows, weight, u, v, sigma, rows, cin, taps):
        """g_rows (rows, taps*cin): a spectral-normed conv's weight gradient, accumulated by the wgrad kernel straight into the
        parameter's channels-last arena slice; weight: weight_orig (same layout).  Applies dW_orig = g/sigma - (<g, W>/sigma^2) u v^T
        in place at the next flush of the step's sink (all layers: one launch pair).  Callers ask `inplace_allowed` first.  A layer
        used twice before a flush queues ONE job: both raw contributions are in g already and the rule is linear."""
        if cin % 8:
            raise ValueError('GradSink.push_inplace: Cin = %d is not a multiple of 8' % cin)
        pool = ZeroPool.active()
        if pool is None:
            raise RuntimeError('GradSink.push_inplace outside a trainer step: the in-place chain rule needs a gradient known to be fresh')
        if any(j.g.data_ptr() == g_rows.data_ptr() for j in pool.sink.inplace):
            return
        pool.sink.inplace.append(InplaceJob(g_rows, _cl_rows(weight), u, v, sigma, int(rows), int(cin), int(taps)))

    def _flush_inplace(self):
        jobs, self.inplace = self.inplace, []
        self.inplace_done.update(j.g.data_ptr() for j in jobs)
        key = tuple((j.g.data_ptr(), j.w.data_ptr(), j.u.data_ptr(), j.v.data_ptr(), j.sigma.data_ptr(), j.rows, j.cin, j.taps) for j in jobs)

        def build():
            dev = jobs[0].g.device
            arr = (L.SnGradJob * len(jobs))()
            for a, j in zip(arr, jobs):
                a.g, a.w, a.u, a.v, a.sigma = j.g.data_ptr(), j.w.data_ptr(), j.u.data_ptr(), j.v.data_ptr(), j.sigma.data_ptr()
                a.rows, a.cin, a.taps = j.rows, j.cin, j.taps
            table = device_job_table(arr, lambda bm: L.call.s2e_sngrad_block_map(C.byref(arr), len(jobs), bm), 2, dev)
            nscratch = int(L.call.s2e_sngrad_scratch_floats(C.byref(arr), len(jobs)))
            return table + (torch.empty(nscratch, dtype=torch.float32, device=dev),)
        jobs_dev, map_dev, nb, partials = self._table('inplace', key, build)
        LaunchProfiler.run(
            'weight_grad_relayout', 0.0, L.call.s2e_sn_grads_inplace, (jobs_dev.data_ptr(), map_dev.data_ptr(), nb, partials.data_ptr(), _stream()),
            nbytes=lambda: float(sum(j.g.numel() * 16 for j in jobs)))     # g and W read for the dot product, g read and written
        self.keep_inplace = jobs

    # ------------------------------------------------------------------ batched patch-resident 3x3 weight gradients
    @staticmethod
    def push_wgrad(x, gy, dw_rows, dbias, rects=None):
        """Queue the weight (and bias) gradient of a 3x3 stride-1 pad-1 conv -- x (N,H,W,Cin), gy (N,H,W,Cout) bf16 -- to be ACCUMULATED
        into dw_rows (Cout, 9*Cin) fp32 row-major / dbias (Cout) at the next flush: all queued layers as ONE persistent launch
        (s2e_wgrad_batch, csrc/conv_wgrad_batch.hip) instead of a launch + a 75-MB partial-tile round trip per layer.  rects =
        (rect_list, counts): the label-sparse form.  x, gy (and the list) stay referenced until the next flush (gy itself, not a copy:
        see is_pinned).  False: not queued -- no trainer step open, a shape the batch does not take, a dW already queued in this flush
        (single-owner tiles are added without atomics), or S2E_WGRAD_BATCH=0 / S2E_DETERMINISTIC=1."""
        pool = ZeroPool.active()
        if pool is None:
            return False
        # FIRST, whatever the shape: a dW that already has a queued job receives another contribution before the flush -- that job must
        # ADD, not store (the scan used to sit behind the early returns below, so a second use of the weight at a shape the
        # batch does not take left the queued job's `fresh` flag set and the flush overwrote the immediate contribution)
        for j in pool.sink.wg:
            if j.dw.data_ptr() == dw_rows.data_ptr():
                j.fresh = False
                return False

        def declined():
            # the caller now accumulates into dw_rows at once: a job queued for it LATER in this scope must add as well
            pool.sink.wg_done.add(dw_rows.data_ptr())
            return False
        if switches.WGRAD_BATCH_OFF or x.dtype != torch.bfloat16 or gy.dtype != torch.bfloat16:
            return declined()
        n, h, w, cin = x.shape
        key = (n, h, w, cin, gy.shape[-1], rects is not None)
        if not memo('wgrad_batch', key, _wgrad_batch_ok, key):
            return declined()
        _need(x, gy, dw_rows, dbias)
        # a gradient arena that zero_grad cleared right before this step, and nothing queued for it yet: single-owner tiles are stored
        fresh = ZeroPool.grad_is_fresh(dw_rows) and dw_rows.data_ptr() not in pool.sink.wg_done
        pool.sink.wg.append(WgradJob(x, gy, dw_rows, dbias, rects, fresh))
        return True

    def _flush_wgrad(self):
        jobs, self.wg = self.wg, []
        self.wg_done.update(j.dw.data_ptr() for j in jobs)
        dev = jobs[0].x.device
        arr = (L.WgradBatchJob * len(jobs))()
        flops = executed = nbytes = 0.0
        for a, j in zip(arr, jobs):
            a.flags = 1 if j.fresh else 0                    # S2E_WGRAD_BATCH_DW_ZERO
            n, h, w, cin = j.x.shape
            cout = j.gy.shape[-1]
            a.x, a.gy, a.dw, a.dbias = j.x.data_ptr(), j.gy.data_ptr(), j.dw.data_ptr(), _p(j.dbias)
            a.N, a.H, a.W, a.Cin, a.Cout = n, h, w, cin, cout
            f, frac = 2.0 * n * h * w * cin * cout * 9, 1.0
            if j.rects is not None:
                a.rect_list, a.rect_count = j.rects[0].data_ptr(), j.rects[1].data_ptr()
                frac = LaunchProfiler.executed_fraction(j.rects[1], n * (h // 16) * (w // 16))
            flops += f
            executed += f * frac
            nbytes += (j.x.numel() + j.gy.numel()) * 2.0 * frac + j.dw.numel() * 4.0
        ws = self.wg_ws
        wsb = L.call.s2e_wgrad_batch_workspace_bytes()
        if ws is None or ws.device != dev or ws.numel() * 4 < wsb:
            ws = self.wg_ws = torch.empty(wsb // 4, dtype=torch.float32, device=dev)      # (3 slots x 256 workgroups x 288 KB)
        LaunchProfiler.run('conv_wgrad_patch', flops, L.call.s2e_wgrad_batch, (L.S2E_BF16, C.byref(arr), len(jobs), _p(ws), wsb, _stream()),
                           tag=lambda: 'W k3 s1 x%d batched' % len(jobs), nbytes=nbytes, executed=executed)
        self.keep_wg = jobs

    @staticmethod
    def is_pinned(t):
        """Does `t` share memory with the output gradient of a weight-gradient job queued in the open trainer step (not launched yet)?
        Whoever would modify it in place (ModulateFn's relay) must write elsewhere: the queue holds the tensor itself, not a copy.
        A view at another offset, a reshaped alias or any overlapping slice of that tensor's storage counts; a disjoint slice does not.
        Why the tensor itself: a conv with a residual input returns gy as the residual's gradient, and the block's first SPADE then adds
        its own dx to it; the deferred launch must not see that sum.  Rounds 4-5 queued a COPY (135 MB of copies per G step); since
        round 6 the relay asks here and writes its sum to a new tensor instead of in place when the one it was handed is still to be
        read by a queued job."""
        pool = ZeroPool.active()
        if pool is None or t is None:
            return False
        return any(_overlap(t, j.gy) for j in pool.sink.wg) or any(_overlap(t, j.gy) for j in pool.sink.gwg)

    # ------------------------------------------------------------------ generic weight gradients, multi-job
    @staticmethod
    def push_gwg(x, gy, dw, dbias, desc_key):
        """Queue a GENERIC weight gradient (a shape s2e_conv2d_wgrad would run in its implicit-GEMM kernel: the 1x1 shortcuts, netE's
        stride-2 layers, the PatchGAN's 4x4 layers, the 8x8 maps) to be accumulated into dw (Cout, KH*KW*Cin) / dbias at the next
        flush, every queued job in ONE launch (s2e_conv2d_wgrad_multi).  desc_key: the ConvDesc fields of the forward conv.  False:
        not queued (no trainer step open, not bf16, not a generic shape, a dW that already has a queued job, S2E_WGRAD_MULTI=0)."""
        pool = ZeroPool.active()
        if pool is None or switches.WGRAD_MULTI_OFF or x.dtype != torch.bfloat16 or gy.dtype != torch.bfloat16:
            return False
        if (not memo('wgrad_multi', desc_key, _wgrad_multi_ok, desc_key)
                or any(j.dw.data_ptr() == dw.data_ptr() for j in pool.sink.gwg)):      # (the reduction adds without atomics: one job per dW)
            return False
        _need(x, gy, dw, dbias)
        pool.sink.gwg.append(GwgJob(x, gy, dw, dbias, desc_key))
        return True

    def _flush_gwg(self):
        jobs, self.gwg = self.gwg, []
        dev = jobs[0].x.device
        arr = (L.WgradMultiJob * len(jobs))()
        flops = nbytes = 0.0
        for a, j in zip(arr, jobs):
            a.x, a.gy, a.dw, a.dbias = j.x.data_ptr(), j.gy.data_ptr(), j.dw.data_ptr(), _p(j.dbias)
            a.d = L.ConvDesc(*j.desc)
            n, _, _, cin, ho, wo, cout, kh, kw = j.desc[:9]
            flops += 2.0 * n * ho * wo * cin * cout * kh * kw
            nbytes += (j.x.numel() + j.gy.numel()) * 2.0 + j.dw.numel() * 4.0
        wsb = int(L.call.s2e_conv2d_wgrad_multi_workspace_bytes(L.S2E_BF16, C.byref(arr), len(jobs)))
        ws = self.gwg_ws
        if wsb and (ws is None or ws.device != dev or ws.numel() * 4 < wsb):
            pool = ZeroPool.active()
            if pool is not None and pool.frozen:
                ws, wsb = None, 0                            # (a captured graph must not start using new memory: those jobs add with atomics)
            else:
                ws = self.gwg_ws = torch.empty(wsb // 4 + 64, dtype=torch.float32, device=dev)
        LaunchProfiler.run(
            'conv_wgrad', flops, L.call.s2e_conv2d_wgrad_multi, (L.S2E_BF16, C.byref(arr), len(jobs), _p(ws) if wsb else None, wsb, _stream()),
            tag=lambda: 'W generic x%d multi' % len(jobs), nbytes=nbytes)
        self.keep_gwg = jobs

    # ------------------------------------------------------------------ 8-channel weight gradients (mlp_shared)
    @staticmethod
    def c8_takes(dtype, h, w, nh, dw, db, rects):
        """Does push_c8 queue this layer?  A trainer step open, gradient destinations given, bf16, nh = 128 output channels, a map the
        batch kernel takes, and with a rectangle list 16-aligned sides.  Said here alone: push_c8 acts on it, and the SPADE backward's
        plan asks it before it leaves d(actv) undefined outside the rectangle list it passes."""
        return bool(ZeroPool.active() is not None and dw is not None and db is not None and dtype == torch.bfloat16 and nh == 128
                    and memo('wgrad_c8', (h, w), L.call.s2e_wgrad_c8_batch_supported, L.S2E_BF16, h, w, 128) and (rects is None or not ((h | w) & 15)))

    @staticmethod
    def push_c8(oh, dactv, dw, db, ncls, rects=None):
        """Queue the weight / bias gradient of a 3x3 conv on the 8-channel one-hot map `oh` (N,h,w,8) with output gradient
        `dactv` (N,h,w,128), accumulated straight into dw (128,ncls,3,3) / db (128) fp32 at the next flush -- all queued layers
        in one launch per slab shape (s2e_wgrad_c8_batch).  rects = (rect_list, counts): only the pixels of those 16 x 16 rectangles
        contribute (the label-sparse backward: dactv is defined there only).  False: not queued (c8_takes says no)."""
        if not GradSink.c8_takes(oh.dtype, oh.shape[1], oh.shape[2], dactv.shape[-1], dw, db, rects):
            return False
        ZeroPool.active().sink.c8.append(C8Job(oh, dactv, dw, db, int(ncls), rects))
        return True

    def _flush_c8(self):
        c8, self.c8 = self.c8, []
        n = c8[0].oh.shape[0]
        rest = [j for j in c8 if j.oh.shape[0] != n]         # (a launch shares one batch size: other sizes go in a round of their own)
        if rest:
            c8 = [j for j in c8 if j.oh.shape[0] == n]
            self.c8 = rest
        arr = (L.WgradC8Job * len(c8))()
        for a, j in zip(arr, c8):
            a.x, a.gy, a.dw_oihw, a.dbias = j.oh.data_ptr(), j.dactv.data_ptr(), j.dw.data_ptr(), j.db.data_ptr()
            a.H, a.W, a.ncls = j.oh.shape[1], j.oh.shape[2], j.ncls
            if j.rects is not None:
                a.rect_list, a.rect_count = j.rects[0].data_ptr(), j.rects[1].data_ptr()
        wsb = L.call.s2e_wgrad_c8_batch_workspace_bytes(n, C.byref(arr), len(c8))
        ws = torch.empty(wsb // 4, dtype=torch.float32, device=c8[0].oh.device)
        LaunchProfiler.run(
            'conv_wgrad_patch', sum(2.0 * n * j.oh.shape[1] * j.oh.shape[2] * 8 * 128 * 9 for j in c8),
            L.call.s2e_wgrad_c8_batch, (L.S2E_BF16, n, C.byref(arr), len(c8), _p(ws), wsb, _stream()),
            tag=lambda: 'W n%d c8->128 k3 s1 x%d batched' % (n, len(c8)),
            nbytes=lambda: float(sum((j.oh.numel() + j.dactv.numel()) * 2 for j in c8)))
        self.keep_c8 = (c8, ws, self.keep_c8 if rest else None)   # (with the workspace; a round of another batch size chains the one before it)
        if rest:
            self._flush_c8()

    # ------------------------------------------------------------------ uniform rectangles of the label-sparse SPADE backward
    @staticmethod
    def push_uniform(R, A, w_gb, w_sh, b_sh, dw_sh, db_sh, dw_gb, db_gb, c2, nh, ncls, act_bf16):
        """Queue the closed-form part of a label-sparse SPADE backward: on the label-uniform interior rectangles the gradients of
        mlp_shared (dw_sh (nh,ncls,3,3) / db_sh) and of the [gamma | beta] conv (dw_gb / db_gb, its rank-1 update per class; None:
        that conv's gradient ran dense) follow from R, the per-class nine shifted sums of d[gamma | beta] that s2e_spade_uniform_sums
        has launched, and the weights w_gb (C2,nh,3,3), w_sh, b_sh; A (ncls, nh) is zeroed scratch for the per-class activations.
        Added to the targets at the next flush, up to 16 layers per launch pair (s2e_spade_uniform_grads).  Only inside a trainer step:
        R and A are ZeroPool scratch."""
        pool = ZeroPool.active()
        if pool is None:
            raise RuntimeError('GradSink.push_uniform outside a trainer step')
        queue = pool.sink.uni
        queue.append(UniformJob(R, A, w_gb, w_sh, b_sh, dw_sh, db_sh, dw_gb, db_gb, int(c2), int(nh), int(ncls), int(act_bf16)))

    def _flush_uniform(self):
        """All queued SPADE layers' uniform-rectangle gradients (s2e_spade_uniform_grads): two launches per 16 layers."""
        jobs, self.uni = self.uni, []
        # launches of <= 16 jobs; two jobs that add into the SAME parameter gradients (a SPADE module applied twice before a flush)
        # never share one: the apply kernel adds with plain read-modify-writes, one job per blockIdx.y
        chunks, cur, seen = [], [], set()
        for j in jobs:
            keys = {t.data_ptr() for t in (j.dw_sh, j.db_sh, j.dw_gb, j.db_gb) if t is not None}
            if len(cur) == 16 or (keys & seen):
                chunks.append(cur)
                cur, seen = [], set()
            cur.append(j)
            seen |= keys
        if cur:
            chunks.append(cur)
        for chunk in chunks:
            arr = (L.SpadeUniJob * len(chunk))()
            for a, j in zip(arr, chunk):
                a.R, a.A, a.w_gb = j.R.data_ptr(), j.A.data_ptr(), j.w_gb.data_ptr()
                a.w_sc, a.w_sk = j.w_gb.stride(0), j.w_gb.stride(1)
                a.w_st = j.w_gb.stride(3)                        # tap t = 3 ky + kx: stride(2) == 3 * stride(3) in both layouts
                a.w_sh, a.b_sh = j.w_sh.data_ptr(), j.b_sh.data_ptr()
                a.dw_sh, a.db_sh, a.dw_gb, a.db_gb = _p(j.dw_sh), _p(j.db_sh), _p(j.dw_gb), _p(j.db_gb)
                a.C2, a.nh, a.ncls, a.act_bf16 = j.c2, j.nh, j.ncls, j.act_bf16
            LaunchProfiler.run('spade_uniform_bwd', 0.0, L.call.s2e_spade_uniform_grads, (C.byref(arr), len(chunk), _stream()),
                               nbytes=lambda: float(sum(j.w_gb.numel() * 4 for j in chunk)))
        self.keep_uni = jobs
