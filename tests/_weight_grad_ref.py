"""csrc/weight_grad.hip -- packed dW -> OIHW gradient, with or without spectral norm's chain rule -- at the C ABI: the cases, their
inputs, the fp64 reference, the error bound and an fp32 emulation of the kernels' order of operations that checks the bound's two
constants without a GPU (tests/test_weight_grad_host.py).  tests/test_weight_grad_gpu.py runs the library on the same cases.

Reference.  g[co][ci][tap] = gw_packed[co][tap][ci] (exact), D = <g, W_orig> in fp64,
    ref = start + g / sigma - (D / sigma^2) u[co] v[ci * taps + tap]              (start = 0 without `accumulate`)

Bound, per element, with eps = 2^-24 (the relative error of one fp32 rounding):
    |got - ref| <= C_OPS eps (|start| + |g| / sigma + |D| |u| |v| / sigma^2) + E_dot |u| |v| / sigma^2,   E_dot = d eps sum |g_i w_i|
C_OPS = 7 counts the roundings on the longest path to an output element, each relative to a quantity no larger than the bracket:
the divide 1 / sigma (it enters the coefficient dot * inv * inv twice: 2), the two multiplies that form the coefficient (2), the
multiply by u[co] (1), the multiply-subtract (1; its product is not rounded), the accumulate (1).  The g / sigma term sees the divide
once, the scale, the multiply-subtract and the accumulate: 4.
d is the number of roundings the first product added by a lane goes through before it is part of the dot: one per fused
multiply-add of that lane's chain (taps per tile x tiles per workgroup), six butterfly steps, three adds of the four waves' sums,
and one atomic add per workgroup -- any summation order errs by at most (depth) eps sum |g_i w_i| to first order.
Plain re-layouts do no arithmetic (accumulate = 0) or one exact-to-fp32 add (accumulate = 1): they are compared bit for bit."""
import ctypes as C

import numpy as np
import torch

EPS = 2.0 ** -24
C_OPS = 7
SIGMA = 1.7
ROWS, TILES_PER_BLOCK = 4, 8                    # SNG_ROWS, GRAD_TILES_PER_BLOCK of csrc/weight_grad.hip
DOT_GRID_CAP, UNPACK_GRID_CAP = 1024, 2048      # the per-layer entries' grid caps

# (cout, cin, taps, cin_pad): the branch of the tile logic each one reaches
CASES = [
    (4, 64, 9, 64),         # one full tile
    (6, 72, 9, 72),         # a ragged row group and a ragged 8-channel chunk
    (5, 4, 9, 8),           # cin_pad > cin, the one-hot label conv
    (64, 64, 1, 64),        # one tap
    (8, 130, 16, 136),      # 4x4, three chunks
    (36, 64, 9, 64),        # 9 tiles: two block-map entries, 8 + 1
    (8200, 64, 1, 64),      # 2050 tiles: past both per-layer grid caps, so the grid-stride loop runs
    (4, 64, 64, 64),        # the most taps the entries take
]
KHW = {1: (1, 1), 9: (3, 3), 16: (4, 4), 64: (8, 8)}


def case_id(case):
    return 'x'.join(str(x) for x in case)


def n_tiles(case):
    cout, cin = case[:2]
    return -(-cout // ROWS) * -(-cin // 64)


def schedule(case, entry):
    """The tiles of each workgroup that adds into the dot, in its order: entry 'layer' (grid-stride) or 'batch' (block map)."""
    tiles = n_tiles(case)
    if entry == 'layer':
        grid = min(tiles, DOT_GRID_CAP)
        return [list(range(b, tiles, grid)) for b in range(grid)]
    return [list(range(t0, min(t0 + TILES_PER_BLOCK, tiles))) for t0 in range(0, tiles, TILES_PER_BLOCK)]


def dot_depth(case, entry):
    sched = schedule(case, entry)
    return case[2] * max(len(s) for s in sched) + 6 + 3 + len(sched)


_INPUTS = {}


def inputs(case):
    """CPU fp32 tensors of a case, made once: gwp (channels past cin hold junk the kernels must not use), w, u, v (unit norm, as the
    power iteration leaves them), start, and the fp64 quantities of the bound."""
    if case in _INPUTS:
        return _INPUTS[case]
    cout, cin, taps, cin_pad = case
    gen = torch.Generator().manual_seed(1000 + CASES.index(case))
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)
    d = {'gwp': rnd(cout, taps, cin_pad), 'w': rnd(cout, cin, taps), 'start': rnd(cout, cin, taps),
         'sigma': torch.tensor([SIGMA], dtype=torch.float32)}
    d['gwp'][:, :, cin:] = 1e6
    u, v = rnd(cout), rnd(cin * taps)
    d['u'], d['v'] = u / u.norm(), v / v.norm()
    d['g'] = d['gwp'][:, :, :cin].permute(0, 2, 1).contiguous()                       # [co][ci][tap]
    g64, w64, sg = d['g'].double(), d['w'].double(), float(d['sigma'].double())
    d['D'] = float((g64 * w64).sum())
    d['absdot'] = float((g64 * w64).abs().sum())
    d['uv'] = d['u'].double().abs()[:, None, None] * d['v'].double().abs().view(1, cin, taps)
    d['chain'] = g64 / sg - d['D'] / sg ** 2 * d['u'].double()[:, None, None] * d['v'].double().view(1, cin, taps)
    d['mag'] = g64.abs() / sg + abs(d['D']) * d['uv'] / sg ** 2
    _INPUTS[case] = d
    return d


def chain_ratio(got, case, entry, accumulate, what):
    """Assert the chain-rule bound on every element; returns the worst error / bound."""
    d = inputs(case)
    sg = float(d['sigma'].double())
    start = d['start'].double() if accumulate else torch.zeros_like(d['chain'])
    bound = C_OPS * EPS * (start.abs() + d['mag']) + dot_depth(case, entry) * EPS * d['absdot'] * d['uv'] / sg ** 2
    g = got.detach().double().cpu().view_as(start)
    assert bool(torch.isfinite(g).all()), '%s: non-finite output' % what
    ratio = ((g - (start + d['chain'])).abs() / bound).max().item()
    print('%s: worst error / bound %.4f (d = %d)' % (what, ratio, dot_depth(case, entry)))
    assert ratio <= 1.0, '%s: worst error / bound %.4f' % (what, ratio)
    return ratio


# ------------------------------------------------------------------ fp32 emulation in the kernels' order (numpy, no GPU)
def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)      # (the product is exact in fp64)


def emulate(case, entry, accumulate):
    """What the kernels compute, operation by operation: lanes' multiply-add chains over their workgroup's tiles, the xor butterfly
    32 .. 1, ((r0 + r1) + r2) + r3, the workgroups' atomic adds (in index order), then the element-wise combination."""
    cout, cin, taps, _ = case
    d = inputs(case)
    g, w = d['gwp'].numpy(), d['w'].numpy()
    chunks = -(-cin // 64)
    sched = schedule(case, entry)
    T = np.full((len(sched), max(len(s) for s in sched)), -1)
    for b, s in enumerate(sched):
        T[b, :len(s)] = s
    q = np.zeros((len(sched), ROWS, 64), np.float32)
    for s in range(T.shape[1]):
        t = T[:, s]
        co = (t // chunks * ROWS)[:, None, None] + np.arange(ROWS)[None, :, None]
        ci = (t % chunks * 64)[:, None, None] + np.arange(64)[None, None, :]
        valid = (t >= 0)[:, None, None] & (co < cout) & (ci < cin)
        coc, cic = np.clip(co, 0, cout - 1), np.clip(ci, 0, cin - 1)
        for tap in range(taps):
            q = np.where(valid, _fma(g[coc, tap, cic], w[coc, cic, tap], q), q)
    for o in (32, 16, 8, 4, 2, 1):
        q = q + q[..., np.arange(64) ^ o]
    part = ((q[:, 0, 0] + q[:, 1, 0]) + q[:, 2, 0]) + q[:, 3, 0]
    dot = np.float32(0)
    for p in part:
        dot = np.float32(dot + p)
    inv = np.float32(1) / d['sigma'].numpy()[0]
    c = np.float32(np.float32(dot * inv) * inv)
    cu = (c * d['u'].numpy()).astype(np.float32)[:, None, None]
    gg = _fma(-cu, d['v'].numpy().reshape(1, cin, taps), (d['g'].numpy() * inv).astype(np.float32))
    return torch.from_numpy((d['start'].numpy() + gg).astype(np.float32) if accumulate else gg)


# ------------------------------------------------------------------ the library on a device
def grad_jobs(specs):
    """specs: [(case, gwp, out, w, u, v, sigma)] of device tensors, w .. sigma None for a plain job -> (GradJob array, block map
    (numpy int32, n x 3), max taps, number of spectral-norm jobs), dot_index counted over the spectral-norm jobs as ops/sink.py does."""
    from seg2eye_amd import _lib as L
    arr = (L.GradJob * len(specs))()
    nsn = 0
    for a, (case, gwp, out, w, u, v, sigma) in zip(arr, specs):
        a.gw_packed, a.out = gwp.data_ptr(), out.data_ptr()
        a.cout, a.cin, a.taps, a.cin_pad = case
        if w is not None:
            a.w_orig, a.u, a.v, a.sigma, a.dot_index = w.data_ptr(), u.data_ptr(), v.data_ptr(), sigma.data_ptr(), nsn
            nsn += 1
        else:
            a.dot_index = -1
    n = L.call.s2e_grad_block_map(C.byref(arr), len(specs), None)
    bm = np.zeros(3 * n, dtype=np.int32)
    assert L.call.s2e_grad_block_map(C.byref(arr), len(specs), bm.ctypes.data) == n
    return arr, bm.reshape(n, 3), max(s[0][2] for s in specs), nsn


def to_device(arr_or_np, dev):
    raw = bytes(arr_or_np) if not isinstance(arr_or_np, np.ndarray) else arr_or_np.tobytes()
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
