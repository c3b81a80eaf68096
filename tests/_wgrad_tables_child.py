#!/usr/bin/env python3
"""Job tables of the weight-gradient multi-job calls against fp64, with a guard band behind every workspace.

Used in-process by tests/test_wgrad_job_tables_gpu.py and run by it as a child process for the switches the library reads once per
process (S2E_C8W_WGS, S2E_WGRAD_MULTI_WGS, S2E_WGRAD_FLAT_WGS, S2E_WGRAD_PARTIAL):

    python tests/_wgrad_tables_child.py [--tables a,b,...] [--modes exact,short,half,none]

Every table is a list of jobs (n, hi, wi, cin, cout, k, stride, pad, kind, dw, db): `kind` is the kernel s2e_conv2d_wgrad_multi_kind
must report, dw = (buffer, float offset) and db = (buffer, float offset) or None name ranges of the output buffers, which several jobs
may share (overlapping ranges included).  The buffers start non-zero; the expected result is that start plus the fp64 sums of every
job that writes there, from the same bf16 operands.  The workspace is ONE byte tensor of the size passed to the call plus GUARD bytes
of a fixed pattern, which must come back unchanged: a launcher that writes past its workspace fails here instead of corrupting memory
it does not own.  Prints one line 'tables ok: ...' at the end."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch                                   # noqa: E402

GUARD = 1 << 20                                # bytes of pattern behind every workspace
PATTERN = 0xA5
TOL = 2e-4                                     # x max|summed fp64 reference| of the buffer
C8_WGS, C8_MAX_JOBS = 512, 4                   # conv_c8.hip: a chunk's workgroups / partial tiles, jobs per chunk
C8W_TILE_BYTES = (64 * 128 + 64) * 4


def J(n, hi, wi, cin, cout, k, s, p, kind, dw, db=None):
    return (n, hi, wi, cin, cout, k, s, p, kind, dw, db)


def c8(n, hi, wi, dw, db=None):
    return J(n, hi, wi, 8, 64, 4, 2, 2, 6, dw, db)


def out_hw(j):
    n, hi, wi, cin, cout, k, s, p = j[:8]
    return (hi + 2 * p - k) // s + 1, (wi + 2 * p - k) // s + 1


def c8_shares(jobs, total=C8_WGS):
    """Python mirror of conv_c8.hip's share formula BEFORE the clamp: a job's workgroups by its pixels, at least 1, at most its rows."""
    work = 0.0
    for j in jobs:
        ho, wo = out_hw(j)
        work += float(j[0] * ho * wo)
    out = []
    for j in jobs:
        ho, wo = out_hw(j)
        out.append(max(1, min(j[0] * ho, int(float(total) * float(j[0] * ho * wo) / work))))
    return out


# ---- the tables
_BIG = (16, 128, 128)                          # c8: Ho = Wo = 65
_TINY = (1, 2, 2)                              # c8: Ho = Wo = 2
_MIXED = [(2, 33, 47), (1, 1, 40), (3, 17, 9), (1, 64, 64)]     # ragged, odd, a 1-row map, square


def _c8_table(shapes, share=()):
    """c8 jobs with their own dw / db; `share`: pairs (i, j) of jobs writing the same dw and db as job i."""
    t = [c8(*s, dw=('w%d' % i, 0), db=('b%d' % i, 0)) for i, s in enumerate(shapes)]
    for i, k in share:
        t[k] = c8(*shapes[k], dw=t[i][9], db=t[i][10])
    return t


def _tables():
    T = {}
    # defect 1: 511 + 1 + 1 + 1 = 514 workgroups' partial tiles in a workspace of 512
    T['c8_lopsided'] = _c8_table([_BIG, _TINY, _TINY, _TINY])
    # chunk boundaries at C8W_MAX_JOBS = 4: 4 + 1 (the big job alone last), 4 + 3 (the last chunk lopsided: 511 + 1 + 1), 4 + 4 + 1
    T['c8_chunk5'] = _c8_table(_MIXED + [_BIG])
    T['c8_chunk7'] = _c8_table(_MIXED + [_BIG, _TINY, (1, 3, 5)])
    T['c8_chunk9'] = _c8_table([_BIG, _TINY, _TINY, _TINY] + _MIXED + [(2, 20, 20)], share=[(1, 6), (2, 8)])
    # defect 2: four split jobs with partial tiles, one dw and one dbias
    big = (16, 128, 128, 64, 128, 3, 2, 1, 0)
    T['gen_shared'] = [J(*big, dw=('w', 0), db=('b', 0)) for _ in range(4)]
    # sharing of every sort: dw only, dbias only, a partial and an atomic job on one dw, overlapping (offset) ranges, dbias = NULL
    kd = 128 * 9 * 64
    T['gen_mixed'] = [
        J(*big, dw=('wA', 0), db=('bA', 0)), J(*big, dw=('wA', 0), db=('bB', 0)),                         # dw only
        J(4, 32, 32, 256, 128, 1, 1, 0, 0, dw=('wC', 0)),                                                  # dbias NULL
        J(4, 64, 64, 64, 128, 3, 2, 1, 0, dw=('wD', 0), db=('bD', 0)), J(4, 64, 64, 64, 128, 3, 2, 1, 0, dw=('wE', 0), db=('bD', 0)),  # dbias only
        J(2, 8, 8, 128, 256, 3, 1, 1, 0, dw=('wF', 0)),                                                    # dbias NULL
        J(*big, dw=('wG', 0), db=('bG', 0)), J(1, 16, 16, 64, 128, 3, 2, 1, 0, dw=('wG', 0), db=('bG', 0)),  # partial + atomic
        J(*big, dw=('wH', 0), db=('bH', 0)), J(*big, dw=('wH', kd // 2 + 8), db=('bH', 40)),             # overlapping ranges
    ]
    # WGM_MAX_JOBS = 26: 27 and 53 small generic jobs (a few split ones with partial tiles in every chunk), some dw shared
    small = [(2, 16, 16, 64, 64, 1, 1, 0), (2, 16, 16, 32, 64, 3, 2, 1), (2, 8, 8, 64, 128, 3, 1, 1), (3, 9, 11, 64, 72, 3, 2, 1),
             (4, 64, 64, 64, 64, 1, 1, 0), (1, 8, 8, 128, 136, 1, 1, 0), (2, 17, 13, 16, 40, 4, 2, 2)]
    for n_jobs in (27, 53):
        t = []
        for i in range(n_jobs):
            s = small[i % len(small)]
            t.append(J(*s, 0, dw=('w%d' % i, 0), db=('b%d' % i, 0) if i % 3 else None))
        for a, b in ((5, 26), (0, 28), (4, 11), (45, 52)):          # across a chunk boundary, within a chunk, in the last chunk
            if b < n_jobs:
                assert small[a % len(small)] == small[b % len(small)]
                t[b] = t[b][:9] + (t[a][9], t[a][10] if t[a][10] is not None else t[b][10])
        T['gen_chunk%d' % n_jobs] = t
    # WF_MAX_JOBS = 24: 25 flat jobs (4x4 stride 1 / stride 2), one huge among tiny ones, some dw shared (the flat kernel's single-owner bit, 8 of its own flags)
    t = [J(16, 129, 129, 64, 128, 4, 2, 2, 5, dw=('fw0', 0), db=('fb0', 0))]
    for i in range(1, 25):
        t.append(J(1, 9, 9, 64, 128, 4, 2, 2, 5, dw=('fw%d' % i, 0), db=('fb%d' % i, 0)) if i % 2 else
                 J(1, 8, 8, 64, 64, 4, 1, 2, 4, dw=('fw%d' % i, 0), db=None))
    t[3] = t[3][:9] + (t[1][9], t[1][10])                            # two tiny one-split jobs on one dw
    t[24] = t[24][:9] + (t[2][9], None)                              # across the chunk boundary
    t[5] = t[5][:9] + (t[0][9], ('fb5', 0))                          # a tiny job on the huge one's dw
    T['flat25'] = t
    # all three launch families in one call, dw shared across them (a 1x1 generic dw has the layout of a 4x4 or c8 one)
    T['all_kinds'] = [
        J(4, 64, 64, 64, 128, 3, 2, 1, 0, dw=('g0', 0), db=('gb0', 0)),
        c8(*_BIG, dw=('c0', 0), db=('cb0', 0)),
        J(16, 33, 33, 64, 128, 4, 2, 2, 5, dw=('f0', 0), db=('fb0', 0)),
        J(4, 32, 32, 1024, 128, 1, 1, 0, 0, dw=('f0', 0), db=('fb0', 0)),      # generic, on the flat job's dw
        c8(*_TINY, dw=('c1', 0)),
        J(4, 32, 32, 128, 64, 1, 1, 0, 0, dw=('c0', 0), db=('cb0', 0)),        # generic, on the c8 job's dw
        J(2, 9, 9, 64, 64, 4, 1, 2, 4, dw=('f1', 0)),
        c8(*_TINY, dw=('c2', 0), db=('cb2', 0)),
        J(*big, dw=('g0', 0), db=('gb0', 0)),
        c8(*_TINY, dw=('c1', 0)),
        J(2, 16, 16, 32, 64, 3, 2, 1, 0, dw=('g2', 0)),
    ]
    return T


TABLES = _tables()


# ---- running a table
def lib():
    from seg2eye_amd import _lib as L
    return L, L.lib()


def descs(table):
    L, _ = lib()
    out = []
    for j in table:
        n, hi, wi, cin, cout, k, s, p = j[:8]
        ho, wo = out_hw(j)
        out.append(L.ConvDesc(n, hi, wi, cin, ho, wo, cout, k, k, s, p, 0, 0, 0, 0))
    return out


def job_array(table, ops=None):
    L, _ = lib()
    arr = (L.WgradMultiJob * len(table))()
    for a, d in zip(arr, descs(table)):
        a.d = d
    if ops is not None:
        for a, j, (x, gy) in zip(arr, table, ops['xg']):
            a.x, a.gy = x.data_ptr(), gy.data_ptr()
            a.dw = ops['buf'][j[9][0]].data_ptr() + 4 * j[9][1]
            a.dbias = (ops['buf'][j[10][0]].data_ptr() + 4 * j[10][1]) if j[10] is not None else None
    return arr


def workspace_bytes(table):
    L, lb = lib()
    arr = job_array(table)
    return int(lb.s2e_conv2d_wgrad_multi_workspace_bytes(L.S2E_BF16, C.byref(arr), len(table)))


def kinds(table):
    L, lb = lib()
    return [int(lb.s2e_conv2d_wgrad_multi_kind(L.S2E_BF16, C.byref(d))) for d in descs(table)]


def _sizes(table):
    size = {}
    for j in table:
        n, hi, wi, cin, cout, k = j[:6]
        for r, cnt in ((j[9], cout * k * k * cin), (j[10], cout)):
            if r is not None:
                size[r[0]] = max(size.get(r[0], 0), r[1] + cnt)
    return size


def operands(table, seed, dev):
    """bf16 x / gy per job and the fp64 expected sums per output buffer (without the buffers' start values)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    xg, ref = [], {}
    for name, cnt in _sizes(table).items():
        ref[name] = torch.zeros(cnt, dtype=torch.float64, device=dev)
    for j in table:
        n, hi, wi, cin, cout, k, s, p = j[:8]
        ho, wo = out_hw(j)
        x = torch.randn(n, hi, wi, cin, generator=g, device=dev).to(torch.bfloat16)
        gy = torch.randn(n, ho, wo, cout, generator=g, device=dev).to(torch.bfloat16)
        xg.append((x, gy))
        x64, g64 = x.double().permute(0, 3, 1, 2), gy.double().permute(0, 3, 1, 2)
        dw = torch.nn.grad.conv2d_weight(x64, (cout, cin, k, k), g64, stride=s, padding=p)       # (cout, cin, k, k)
        dw = dw.permute(0, 2, 3, 1).reshape(-1)                                                   # (co, (ky, kx, ci)) row-major
        ref[j[9][0]][j[9][1]:j[9][1] + dw.numel()] += dw
        if j[10] is not None:
            ref[j[10][0]][j[10][1]:j[10][1] + cout] += g64.sum((0, 2, 3))
        del x64, g64, dw
    return {'xg': xg, 'ref': ref}


def run(name, mode, dev=None, ops=None, seed=1):
    """One call of s2e_conv2d_wgrad_multi on table `name`; mode 'exact' (the workspace it asks for), 'short' (256 bytes less: the
    partial-workspace fallback), 'half' (half of it, rounded down to 256: the middle of the greedy fallback, some sections served and
    the rest atomics) or 'none' (no workspace: the atomic fallbacks).  Asserts kinds, guard band and sums; returns the worst
    relative error."""
    L, lb = lib()
    dev = dev or torch.device('cuda', 0)
    table = TABLES[name]
    assert kinds(table) == [j[8] for j in table], (name, kinds(table))
    if ops is None:
        ops = operands(table, seed, dev)
    g = torch.Generator(device=dev).manual_seed(seed + 1000)
    start = {b: torch.randn(r.numel(), generator=g, device=dev) for b, r in ops['ref'].items()}
    ops['buf'] = {b: t.clone() for b, t in start.items()}
    wsb = workspace_bytes(table)
    passed = {'exact': wsb, 'short': max(wsb - 256, 0), 'half': wsb // 2 // 256 * 256, 'none': 0}[mode]
    ws = torch.full((passed + GUARD,), PATTERN, dtype=torch.uint8, device=dev)
    arr = job_array(table, ops)
    st = torch.cuda.current_stream(dev).cuda_stream
    L.check(lb.s2e_conv2d_wgrad_multi(L.S2E_BF16, C.byref(arr), len(table), ws.data_ptr() if mode != 'none' else None,
                                      passed if mode != 'none' else 0, st), 's2e_conv2d_wgrad_multi')
    torch.cuda.synchronize(dev)
    guard = ws[passed:]
    bad = int((guard != PATTERN).sum())
    assert bad == 0, '%s/%s: %d guard bytes behind the %d-byte workspace were written (first at +%d)' % (
        name, mode, bad, passed, int((guard != PATTERN).nonzero()[0]))
    worst = 0.0
    for b, r in ops['ref'].items():
        scale = max(float(r.abs().max()), 1e-6)
        err = float((ops['buf'][b].double() - start[b].double() - r).abs().max())
        assert err <= TOL * scale, '%s/%s: buffer %s off by %.3e (max |ref| %.3e, tolerance %.1e x)' % (name, mode, b, err, scale, TOL)
        worst = max(worst, err / scale)
    return worst


# ---- s2e_wgrad_batch / s2e_wgrad_c8_batch
def wgrad_batch_guard(dev=None, seed=7):
    """s2e_wgrad_batch on 36 jobs (ragged Cout, several ci tiles, with and without bias, two launches) into non-zero dW, the workspace
    followed by a guard band; then a table whose last job reuses the first one's dW must be refused with dW untouched."""
    L, lb = lib()
    dev = dev or torch.device('cuda', 0)
    g = torch.Generator(device=dev).manual_seed(seed)
    cases = [(2, 16, 16, 128, 256, True), (1, 32, 32, 64, 64, True), (2, 16, 32, 128, 136, False), (1, 64, 64, 64, 128, True),
             (2, 8, 16, 192, 72, True), (1, 8, 16, 512, 512, True)] + [(1, 8, 16, 64, 64 + 8 * i, bool(i & 1)) for i in range(30)]
    arr = (L.WgradBatchJob * len(cases))()
    keep = []
    for a, (n, h, w, cin, cout, bias) in zip(arr, cases):
        assert lb.s2e_wgrad_batch_supported(L.S2E_BF16, n, h, w, cin, cout)
        x = torch.randn(n, h, w, cin, generator=g, device=dev).to(torch.bfloat16)
        gy = torch.randn(n, h, w, cout, generator=g, device=dev).to(torch.bfloat16)
        dw = torch.randn(cout, 9 * cin, generator=g, device=dev)
        db = torch.randn(cout, generator=g, device=dev) if bias else None
        x64, g64 = x.double().permute(0, 3, 1, 2), gy.double().permute(0, 3, 1, 2)
        rw = torch.nn.grad.conv2d_weight(x64, (cout, cin, 3, 3), g64, padding=1).permute(0, 2, 3, 1).reshape(cout, 9 * cin)
        keep.append((x, gy, dw, db, dw.double() + rw, (db.double() + g64.sum((0, 2, 3))) if bias else None, float(rw.abs().max()),
                     float(g64.sum((0, 2, 3)).abs().max())))
        a.x, a.gy, a.dw, a.dbias = x.data_ptr(), gy.data_ptr(), dw.data_ptr(), db.data_ptr() if bias else None
        a.N, a.H, a.W, a.Cin, a.Cout = n, h, w, cin, cout
    wsb = int(lb.s2e_wgrad_batch_workspace_bytes())
    ws = torch.full((wsb + GUARD,), PATTERN, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    L.check(lb.s2e_wgrad_batch(L.S2E_BF16, C.byref(arr), len(cases), ws.data_ptr(), wsb, st), 's2e_wgrad_batch')
    torch.cuda.synchronize(dev)
    assert int((ws[wsb:] != PATTERN).sum()) == 0, 's2e_wgrad_batch wrote past its workspace'
    worst = 0.0
    for i, (x, gy, dw, db, rw, rb, sw, sb) in enumerate(keep):
        e = float((dw.double() - rw).abs().max()) / max(sw, 1e-6)
        assert e <= TOL, ('s2e_wgrad_batch dW', i, cases[i], e)
        worst = max(worst, e)
        if db is not None:
            e = float((db.double() - rb).abs().max()) / max(sb, 1e-6)
            assert e <= TOL, ('s2e_wgrad_batch dbias', i, cases[i], e)
            worst = max(worst, e)
    # a shared dW is refused before anything runs
    two = (L.WgradBatchJob * 3)()
    for k, src in enumerate((0, 1, 0)):
        C.memmove(C.byref(two[k]), C.byref(arr[src]), C.sizeof(L.WgradBatchJob))
    dw0 = keep[0][2]
    before = dw0.clone()
    rc = lb.s2e_wgrad_batch(L.S2E_BF16, C.byref(two), 3, ws.data_ptr(), wsb, st)
    torch.cuda.synchronize(dev)
    assert rc == -1, rc                                       # S2E_ERR_ARG
    msg = lb.s2e_last_error()
    assert msg and b'same dW' in msg, msg
    assert torch.equal(dw0, before), 'a refused s2e_wgrad_batch call changed dW'
    return worst


def wgrad_c8_batch_guard(dev=None, seed=9):
    """s2e_wgrad_c8_batch with 25 jobs (WC_MAX_JOBS = 24: two rounds) of every slab shape, ncls 1..8, some without bias, into non-zero
    dW / dbias; the workspace followed by a guard band; against fp64."""
    L, lb = lib()
    dev = dev or torch.device('cuda', 0)
    g = torch.Generator(device=dev).manual_seed(seed)
    N = 2
    maps = [(16, 16), (32, 32), (64, 64), (48, 80), (32, 16), (16, 48), (64, 128)]
    arr = (L.WgradC8Job * 25)()
    keep = []
    for i, a in enumerate(arr):
        h, w = maps[i % len(maps)]
        ncls = 1 + i % 8
        assert lb.s2e_wgrad_c8_batch_supported(L.S2E_BF16, h, w, 128)
        lab = torch.randint(0, ncls, (N, h, w), generator=g, device=dev)
        oh = torch.zeros(N, h, w, 8, device=dev)
        oh.scatter_(3, lab[..., None], 1.0)
        oh = oh.to(torch.bfloat16)
        gy = torch.randn(N, h, w, 128, generator=g, device=dev).to(torch.bfloat16)
        dw = torch.randn(128, ncls, 3, 3, generator=g, device=dev)
        db = torch.randn(128, generator=g, device=dev) if i % 4 else None
        rw = torch.nn.functional.conv2d(oh[..., :ncls].double().permute(3, 0, 1, 2), gy.double().permute(3, 0, 1, 2), None, 1, 1).permute(1, 0, 2, 3)
        rb = gy.double().sum((0, 1, 2))
        keep.append((oh, gy, dw, db, dw.double() + rw, (db.double() + rb) if db is not None else None, float(rw.abs().max()), float(rb.abs().max())))
        a.x, a.gy, a.dw_oihw, a.dbias = oh.data_ptr(), gy.data_ptr(), dw.data_ptr(), db.data_ptr() if db is not None else None
        a.H, a.W, a.ncls = h, w, ncls
    wsb = int(lb.s2e_wgrad_c8_batch_workspace_bytes(N, C.byref(arr), 25))
    assert wsb > 0
    ws = torch.full((wsb + GUARD,), PATTERN, dtype=torch.uint8, device=dev)
    L.check(lb.s2e_wgrad_c8_batch(L.S2E_BF16, N, C.byref(arr), 25, ws.data_ptr(), wsb, torch.cuda.current_stream(dev).cuda_stream), 's2e_wgrad_c8_batch')
    torch.cuda.synchronize(dev)
    assert int((ws[wsb:] != PATTERN).sum()) == 0, 's2e_wgrad_c8_batch wrote past its workspace'
    worst = 0.0
    for i, (oh, gy, dw, db, rw, rb, sw, sb) in enumerate(keep):
        e = float((dw.double() - rw).abs().max()) / max(sw, 1e-6)
        assert e <= TOL, ('s2e_wgrad_c8_batch dW', i, e)
        worst = max(worst, e)
        if db is not None:
            e = float((db.double() - rb).abs().max()) / max(sb, 1e-6)
            assert e <= TOL, ('s2e_wgrad_c8_batch dbias', i, e)
            worst = max(worst, e)
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tables', default=','.join(TABLES))
    ap.add_argument('--modes', default='exact,short,half,none')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    calls, worst = 0, 0.0
    for name in args.tables.split(','):
        ops = operands(TABLES[name], 1, dev)
        for mode in args.modes.split(','):
            worst = max(worst, run(name, mode, dev, ops))
            calls += 1
        del ops
    print('tables ok: %d calls, worst relative error %.2e (%s)' % (
        calls, worst, ' '.join('%s=%s' % (k, os.environ[k]) for k in ('S2E_C8W_WGS', 'S2E_WGRAD_MULTI_WGS', 'S2E_WGRAD_FLAT_WGS',
                                                                         'S2E_WGRAD_PARTIAL') if k in os.environ) or 'defaults'), flush=True)


if __name__ == '__main__':
    main()
