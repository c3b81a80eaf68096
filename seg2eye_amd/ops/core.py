"""What every op family shares: dtype / pointer / stream helpers, the memo of per-shape library queries, the upload of host-built
job tables, the per-launch profiler, the trainer step's zero-filled scratch (ZeroPool; its queue of deferred weight-side launches is
sink.GradSink) and the views of channels-last parameter memory."""
import numpy as np
import torch

from .. import _lib as L

IN_EPS = 1e-5      # nn.InstanceNorm2d default (models/networks/normalization.py:41,73)


def _dt(t):
    """The library's dtype code of a tensor or a torch.dtype."""
    dtype = t if isinstance(t, torch.dtype) else t.dtype
    if dtype == torch.bfloat16:
        return L.S2E_BF16
    if dtype == torch.float32:
        return L.S2E_F32
    raise TypeError('seg2eye_amd ops take bf16 or fp32 tensors, got %s' % dtype)


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    # the raw handle of torch's current stream, without building a torch.cuda.Stream object per launch (that path resolves
    # the device index through four Python layers: 2.4 ms of host time per eager step of ~1000 launches)
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())


def _need(*ts):
    for t in ts:
        if t is not None:
            if not t.is_cuda:
                raise L.Seg2EyeHipError('seg2eye_amd ops run on the GPU only (got a %s tensor); '
                                        'there is no CPU fallback' % t.device)
            if not t.is_contiguous():
                raise L.Seg2EyeHipError('seg2eye_amd ops need contiguous tensors')


# ------------------------------------------------------------------------------ per-shape library queries, device job tables
_MEMO = {}


def memo(kind, key, fn, *args):
    """fn(*args) -- what the library answers about ONE shape (is this kernel available, how much workspace) -- asked once per
    (kind, key): a step repeats the same ~150 shapes.  One dict for every kind, cleared when it passes 8192 entries."""
    k = (kind, key)
    v = _MEMO.get(k)
    if v is None:
        if len(_MEMO) > 8192:
            _MEMO.clear()
        v = _MEMO[k] = fn(*args)
    return v


def upload_structs(arr, dev):
    """A ctypes structure (array) as a uint8 device tensor."""
    return torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy()).to(dev)


def device_job_table(arr, block_map, ints, dev):
    """-> (jobs on the device, block map on the device, blocks) for a batched launch.  arr: the filled ctypes job array; block_map(None)
    counts the blocks and block_map(host pointer) writes `ints` int32 per block (a planner of the library with its leading arguments
    closed over).  The job bytes are uploaded AFTER the fill call: s2e_sngrad_block_map writes part0 / nparts / vmem0 into the jobs."""
    nb = int(block_map(None))
    bm = np.zeros(ints * nb, dtype=np.int32)
    block_map(bm.ctypes.data)
    return upload_structs(arr, dev), torch.from_numpy(bm).to(dev), nb


# ------------------------------------------------------------------------------ per-launch timing
class LaunchProfiler:
    """Optional HIP-event timing of the kernels, per C-ABI call, on the stream they are launched on (torch's current
    stream).  bench.py / tools create one, install it with `LaunchProfiler.install(p)` and read `p.summary()`; with none
    installed (the default) `run` is a plain call.  Families: the MFMA kernels by `s2e_conv2d_kernel_kind` (conv_patch /
    conv_igemm / conv_small and the weight-gradient ones), the HBM-bound ones by entry point (in_stats, modulate_fwd,
    modulate_bwd, label_conv, adam, ...), each with its ALGORITHMIC FLOPs / bytes."""
    current = None        # the installed profiler (one per process at a time: it times whatever runs on this thread)

    def __init__(self):
        self.records = []     # (family, algorithmic_flops, start_event, end_event, tag, algorithmic_bytes, executed_flops)

    @classmethod
    def install(cls, prof):
        cls.current = prof

    @classmethod
    def active(cls):
        return cls.current is not None

    @classmethod
    def run(cls, family, flops, fn, args, tag='', nbytes=0.0, executed=None):
        """fn(*args) is the launch (L.call.s2e_x and its arguments: nothing is built per launch while no profiler is installed).
        executed: the FLOPs the launch really performs when that is less than its algorithmic count (the label-sparse
        SPADE launch computes only the rectangles that cross a label boundary); default = flops."""
        prof = cls.current
        if prof is None:
            return fn(*args)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        r = fn(*args)
        e.record()
        # (family / tag / nbytes may be callables: evaluated only here, i.e. only while a profiler is installed -- formatting a
        # tag string and summing tensor sizes for each of ~1000 launches cost ~2 ms of host time per eager step)
        prof.records.append((family() if callable(family) else family, flops, s, e, tag() if callable(tag) else tag,
                             nbytes() if callable(nbytes) else nbytes, flops if executed is None else executed))
        return r

    @classmethod
    def executed_fraction(cls, counts, total):
        """The part of its `total` rectangles that a launch over a device-side rectangle list executes, counts[0] / total, for
        `executed` and the byte counts of `run` -- read from the device (a sync) only while a profiler is installed; 1.0 otherwise."""
        return float(int(counts[0])) / max(total, 1) if cls.current is not None else 1.0

    def summary(self):
        """family -> dict(launches, flops, ms, bytes); call after a device synchronize."""
        out = {}
        for fam, fl, s, e, _, nb, ex in self.records:
            d = out.setdefault(fam, dict(launches=0, flops=0.0, ms=0.0, bytes=0.0, executed_flops=0.0))
            d['launches'] += 1
            d['flops'] += fl
            d['executed_flops'] += ex
            d['bytes'] += nb
            d['ms'] += s.elapsed_time(e)
        return out

    def reset(self):
        self.records = []


# ------------------------------------------------------------------------------ zero-filled scratch
class ZeroPool:
    """Zero-initialised scratch for the steps of ONE trainer, filled by ONE launch per step.

    A G or D step needs ~200 small zero-filled buffers (packed weight-gradient accumulators, fp64 reduction scratch of
    the statistics / modulation kernels, the spectral-norm dot products).  Zeroing each with its own 4-5 us launch cost
    ~1 ms of a 35 ms step.  Inside `with pool.scope(key)` they are bump-allocated from the pool's device buffer, whose
    used prefix (the high-water mark of earlier scopes with the same key) is cleared by a single fill at scope entry; a
    take beyond the cleared prefix clears its own slice.  The ops ask `ZeroPool.take(...)`, which serves from the pool
    whose scope is open on this process (scopes do not nest) and is plain torch.zeros when none is -- stand-alone ops,
    inference models and tests behave as before.  Everything taken inside a scope must be dead when the pool's next
    scope starts: true for the scratch listed above, NOT for tensors handed to the caller (losses, parameter
    gradients) -- those never come from a pool.  After `freeze()` (a hipGraph holds raw pointers into the buffer) the
    buffer is never re-allocated; overflow falls back to torch.zeros.

    Each Pix2PixTrainer owns its pool (and with it the queues of deferred weight-side launches, sink.GradSink): two
    trainers -- or a trainer and an inference model -- in one process share nothing."""
    ALIGN = 256
    _active = None     # the pool whose scope is open
    serial = 0         # scopes begun so far, over all pools (lets per-scope state elsewhere notice a new step)
    _zeroed = {}       # gradient arena base pointer -> (bytes, ZeroPool.serial when optim.FlatAdam.zero_grad last cleared it)

    @classmethod
    def arena_zeroed(cls, flat_g):
        """optim.FlatAdam.zero_grad reports here: this gradient arena is all zeros as of now.  Entries of arenas that no longer
        exist -- their memory now (partly) belongs to this one -- are dropped: a lookup by address must find THIS arena's entry, not
        a dead optimizer's (found in round 5 as a test-order-dependent failure: `arena_touched` marked the stale entry, the live
        arena stayed "fresh" and a chain-ruled gradient was rewritten in place)."""
        base, nbytes = flat_g.data_ptr(), flat_g.numel() * flat_g.element_size()
        for b in [b for b, (nb, _) in cls._zeroed.items() if b != base and b < base + nbytes and base < b + nb]:
            del cls._zeroed[b]
        cls._zeroed[base] = (nbytes, cls.serial)

    @classmethod
    def arena_touched(cls, g):
        """A gradient that is NOT the raw sum of this step's contributions was (or is about to be) accumulated into `g`'s arena
        outside the in-place protocol -- e.g. a spectral-normed layer's chain-ruled gradient through the accumulate path: the
        arena no longer counts as fresh until the next zero_grad."""
        ptr = g.data_ptr()
        for base, (nbytes, _) in cls._zeroed.items():
            if base <= ptr < base + nbytes:
                cls._zeroed[base] = (nbytes, -1)
                return

    @classmethod
    def grad_is_fresh(cls, g):
        """Is `g` (a view of a gradient arena) known to have been ZERO when the open scope began -- cleared by zero_grad after
        the previous scope and before this one?  Only then may a kernel sequence that REWRITES the gradient (spectral norm's
        in-place chain rule) stand in for one that accumulates."""
        if cls._active is None:
            return False
        ptr = g.data_ptr()
        for base, (nbytes, serial) in cls._zeroed.items():
            if base <= ptr < base + nbytes:
                return serial == cls.serial - 1
        return False

    def __init__(self, device):
        self.device = torch.device(device)
        self.buf = None
        self.cap = 0            # bytes allocated
        self.bump = 0           # bytes handed out in the current scope
        self.clean = 0          # [bump, clean) is known to be zero
        self.need = 0           # largest total any scope asked for (drives growth)
        self.high = {}          # key -> high-water mark
        self.key = None
        self.frozen = False
        self.step_cache = {}    # per-scope memo of derived read-only tensors (cleared at scope entry and exit)
        self.tails, self.tail_i = {}, 0     # (scope key, i) -> (live, persistent zero-tailed gradient buffer): _live_tail_buffer
        from .sink import GradSink                           # (sink.py imports this module at its top: the one place the cycle is cut)
        self.sink = GradSink()

    def scope(self, key):
        return _ZeroScope(self, key)

    def freeze(self):
        self.frozen = True

    def unfreeze(self):
        self.frozen = False

    @classmethod
    def active(cls):
        """The pool whose scope is open, or None."""
        return cls._active

    def _begin(self, key):
        if ZeroPool._active is not None:
            raise RuntimeError('ZeroPool scopes do not nest')
        if not self.frozen and self.need > self.cap:
            self.cap = (int(self.need * 1.25) + self.ALIGN - 1) // self.ALIGN * self.ALIGN
            self.buf = torch.zeros(self.cap, dtype=torch.uint8, device=self.device)
            self.clean = self.cap
        else:
            hw = min(self.high.get(key, 0), self.cap)
            if hw:
                self.buf[:hw].zero_()
            self.clean = hw
        self.key, self.bump, self.tail_i = key, 0, 0
        self.step_cache = {}
        self.sink.begin_scope()
        ZeroPool._active = self
        ZeroPool.serial += 1

    def _end(self):
        self.high[self.key] = max(self.high.get(self.key, 0), self.bump)
        self.need = max(self.need, self.bump)
        self.key = None
        self.step_cache = {}
        ZeroPool._active = None

    @classmethod
    def take(cls, numel, dtype, device):
        pool = cls._active
        if pool is None:
            return torch.zeros(numel, dtype=dtype, device=device)
        nbytes = numel * torch.empty((), dtype=dtype).element_size()
        off = pool.bump
        end = off + (nbytes + cls.ALIGN - 1) // cls.ALIGN * cls.ALIGN
        pool.bump = end                                  # counts overflow too: that is how the pool learns its size
        if end > pool.cap or pool.buf.device != torch.device(device):
            return torch.zeros(numel, dtype=dtype, device=device)
        if end > pool.clean:
            pool.buf[max(off, pool.clean):end].zero_()
            pool.clean = end
        return pool.buf[off:off + nbytes].view(dtype)


class _ZeroScope:
    def __init__(self, pool, key):
        self.pool, self.key = pool, key

    def __enter__(self):
        self.pool._begin(self.key)

    def __exit__(self, *exc):
        try:
            if exc[0] is None:
                self.pool.sink.flush()                       # every queued weight-side launch of the step
            else:
                self.pool.sink.abort()                       # a failed step: nothing of it runs later
        finally:
            self.pool._end()
        return False


# ------------------------------------------------------------------------------ parameter memory views
def _cl_dense(t):
    """A 4-D tensor whose memory is one dense block in [d0][d2][d3][d1] order: a conv weight stored channels-last
    (optim.FlatAdam), i.e. already in the packed order of the MFMA kernels."""
    return t is not None and t.dim() == 4 and t.permute(0, 2, 3, 1).is_contiguous()


def _cl_rows(t):
    """(Cout, KH*KW*Cin) row-major view of a channels-last conv weight's (or gradient's) memory."""
    co, ci, kh, kw = t.shape
    return t.detach().permute(0, 2, 3, 1).reshape(co, kh * kw * ci)


def _grad_dst(p):
    """The tensor a backward kernel may accumulate this parameter's gradient into directly: its .grad when
    that already exists as a contiguous fp32 tensor (optim.FlatAdam keeps .grad as a view of the gradient
    arena and zeroes it at the start of every step).  None -> return the gradient to autograd instead."""
    if p is None or not p.is_leaf:                       # (a non-leaf's .grad is never an arena view; asking for it warns)
        return None
    g = getattr(p, 'grad', None)
    if g is None or g.dtype != torch.float32 or not (g.is_contiguous() or _cl_dense(g)) or not g.is_cuda:
        return None
    return g


def _adjacent(a, b):
    """b starts exactly where a ends in the same storage (both dense: contiguous, or channels-last conv weights)."""
    return (a is not None and b is not None and (a.is_contiguous() or _cl_dense(a)) and (b.is_contiguous() or _cl_dense(b))
            and a.is_contiguous() == b.is_contiguous()
            and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()
            and b.storage_offset() == a.storage_offset() + a.numel())


def _span2(a, shape):
    """View of `a`'s storage starting at a, with `shape` (covers a and the tensor laid out right after it, which is stacked
    along dimension 0); in a's memory order -- row-major, or channels-last for a conv weight stored that way."""
    if len(shape) == 4 and not a.is_contiguous() and _cl_dense(a):
        co, ci, kh, kw = shape
        return a.detach().as_strided(shape, (kh * kw * ci, 1, kw * ci, ci))
    strides, st = [], 1
    for d in reversed(shape):
        strides.append(st)
        st *= d
    return a.detach().as_strided(shape, tuple(reversed(strides)))


def colsum(g):
    _need(g)
    c = g.shape[-1]
    out = torch.zeros(c, dtype=torch.float32, device=g.device)
    L.call.s2e_colsum(_dt(g), _p(g), g.numel() // c, c, _p(out), _stream())
    return out


# ------------------------------------------------------------------------------ OpenEDS validation metric
def _single_channel(x):
    """(N,1,H,W) / (N,H,W,1) / (N,H,W) -> contiguous (N,H,W) view of the same dtype."""
    if x.dim() == 4 and x.shape[1] == 1:
        x = x[:, 0]
    elif x.dim() == 4 and x.shape[-1] == 1:
        x = x[..., 0]
    if x.dim() != 3:
        raise ValueError('single-channel image batch expected, got shape %s' % (tuple(x.shape),))
    return x.contiguous()
