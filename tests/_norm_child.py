#!/usr/bin/env python3
"""The kernels of csrc/norm_modulate.hip -- InstanceNorm statistics, plain IN (+ LeakyReLU) forward / backward, the SPADE+Style
modulation forward and every form of its backward, column sums -- against fp64, element by element, at the C ABI.

Run by tests/test_norm_fp64_gpu.py as a child process per (environment, group), because the library reads S2E_IN_SMALL_HW once per
process (0: every map on the row-walking kernels; 100000: every listed map on the one-launch kernels):

    python tests/_norm_child.py --groups small,rowwalk,forms,edge,partials,colsum,zblocks,long,wrap --dtype bf16

tests/_norm_ref.py has the references, the bounds and their derivation, the geometry and the input generators.

Guards (the discipline of tests/_conv3x3_child.py, whose Guarded / workspace are used here): every output and workspace sits between
GUARD bytes of PATTERN that must come back unchanged; workspaces have exactly the size the *_workspace_bytes query reports and start
as NaN; overwritten outputs start as NaN, accumulated ones non-zero; every call goes through seg2eye_amd._lib.call, which raises on a
non-zero status.  Prints, per case, the kernel that ran and the largest err / bound of each output, and 'norm ok: ...' last."""
import argparse
import os

import torch

import _norm_ref as R
from _conv3x3_child import PATTERN, Guarded, stream, workspace

from seg2eye_amd import _lib as L                      # noqa: E402  (_conv3x3_child put the repository root on sys.path)

SMALL_HW = int(os.environ.get('S2E_IN_SMALL_HW', '1280'))
NAN = float('nan')
RESULTS = []


def code(dt):
    return L.S2E_BF16 if dt == 'bf16' else L.S2E_F32


def ptr(t):
    return None if t is None else (t.ptr() if isinstance(t, Guarded) else t.data_ptr())


def check(got, ref, bound, what):
    """every element within its bound (NaN fails); returns the worst err / bound"""
    g = got.detach().double().cpu().reshape(ref.shape)
    err = (g - ref).abs()
    ok = err <= bound
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        i = tuple(int(v) for v in bad[0])
        msg = ('%s: %d of %d elements outside the bound; first at %s: got %r, ref %r, bound %.3e'
               % (what, bad.shape[0], ok.numel(), i, float(g[i]), float(ref[i]), float(bound[i])))
        print('FAILED ' + msg, flush=True)
        raise AssertionError(msg)
    return float((err / bound.clamp_min(1e-300)).max())


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8).cpu(), b.contiguous().view(torch.uint8).cpu())


def report(group, name, kernel, worst):
    line = '  %-8s %-58s kernel=%-22s err/bound %s' % (group, name, kernel, ' '.join('%s=%.3f' % kv for kv in worst.items()))
    RESULTS.append(line)
    print(line, flush=True)


def doubles(ws, n):
    return ws.t[:8 * n].view(torch.float64)


def tag(dt, N, HW, C, *more):
    return ' '.join(['%s %dx%dx%d' % (dt, N, HW, C)] + [m for m in more if m])


# ---- statistics
def check_stats(stats, st, what, worst):
    s = stats.detach().double().cpu()
    worst['mean'] = check(s[..., 0], st['mean'], st['d_mean'], what + ' mean')
    worst['rstd'] = check(s[..., 1], st['rstd'], st['d_rstd'], what + ' rstd')


def check_ws_sums(ws, st, N, C, what, worst):
    w = doubles(ws, N * C * 2).cpu().view(N, C, 2)
    worst['sum'] = check(w[..., 0], st['s'], st['d_s'], what + ' ws sum x')
    worst['sumsq'] = check(w[..., 1], st['q'], st['d_q'], what + ' ws sum x^2')


def run_in_stats(group, dt, N, HW, C, dev, seed):
    x = R.make_case(dt, N, HW, C, seed)['x']
    st = R.stats_ref(x.double())
    wsb = int(L.call.s2e_in_stats_workspace_bytes(code(dt), N, HW, C))
    ws, stats = workspace(wsb, dev), Guarded((N, C, 2), torch.float32, dev, NAN)
    xd = x.to(dev)                                         # (device operands stay referenced until the results are read)
    L.call.s2e_in_stats(code(dt), xd.data_ptr(), N, HW, C, R.EPS, ws.ptr(), stats.ptr(), stream())
    what, worst = tag(dt, N, HW, C, 'in_stats'), {}
    ws.check(what + ' ws')
    stats.check(what + ' stats')
    check_stats(stats.t, st, what, worst)
    check_ws_sums(ws, st, N, C, what, worst)
    report(group, what, 'in_small' if HW <= SMALL_HW else 'in_stats_partial+finalize', worst)


def run_in_fwd(group, dt, N, HW, C, lrelu_on, dev, seed, edge=None):
    x = R.make_case(dt, N, HW, C, seed, edge=edge)['x']
    ref, bound, st = R.instance_norm_fwd_ref(x.double(), lrelu_on, dt)
    wsb = int(L.call.s2e_in_stats_workspace_bytes(code(dt), N, HW, C))
    ws, stats = workspace(wsb, dev), Guarded((N, C, 2), torch.float32, dev, NAN)
    out = Guarded((N, HW, C), R.TDT[dt], dev, NAN)
    xd = x.to(dev)
    L.call.s2e_instance_norm_fwd(code(dt), xd.data_ptr(), out.ptr(), stats.ptr(), ws.ptr(), N, HW, C, R.EPS, int(lrelu_on), stream())
    what, worst = tag(dt, N, HW, C, 'in_fwd', 'lrelu' if lrelu_on else '', edge), {}
    for b in (ws, stats, out):
        b.check(what)
    check_stats(stats.t, st, what, worst)
    worst['out'] = check(out.t, ref, bound, what + ' out')
    report(group, what, 'in_small<apply>' if HW <= SMALL_HW else 'in_stats+modulate_fwd', worst)


def run_in_bwd(group, dt, N, HW, C, lrelu_on, dev, seed, edge=None):
    case = R.make_case(dt, N, HW, C, seed, edge=edge)
    res = R.modulate_bwd_ref(R.widen(case), R.PLAIN, lrelu_on)
    wsb = int(L.call.s2e_modulate_bwd_workspace_bytes(code(dt), N, HW, C))
    ws, dx = workspace(wsb, dev), Guarded((N, HW, C), R.TDT[dt], dev, NAN)
    d = {k: case[k].to(dev) for k in ('g', 'x', 'stats')}
    L.call.s2e_instance_norm_bwd(code(dt), d['g'].data_ptr(), d['x'].data_ptr(), d['stats'].data_ptr(),
                                 dx.ptr(), ws.ptr(), N, HW, C, int(lrelu_on), stream())
    what = tag(dt, N, HW, C, 'in_bwd', 'lrelu' if lrelu_on else '', edge)
    ws.check(what + ' ws')
    dx.check(what + ' dx')
    worst = {'dx': check(dx.t, res['dx'][0], R.dx_bound(res, dt, False), what + ' dx')}
    report(group, what, 'in_small_bwd' if HW <= SMALL_HW else 'reduce+coef+apply', worst)


def run_mod_fwd(group, dt, N, HW, C, mode, lrelu_on, dev, seed, banked=False):
    ld, off = (2 * C + 24, 8) if banked else (0, 0)
    case = R.make_case(dt, N, HW, C, seed, ld=ld, off=off)
    t = R.widen(case)
    ref, A, _, _ = R.modulate_fwd_ref(t['x'], t['gb'], t['stats'], t['s0'], t['s1'], mode, lrelu_on)
    out = Guarded((N, HW, C), R.TDT[dt], dev, NAN)
    d = {k: case[k].to(dev) for k in ('x', 'gb', 'stats', 'style')}
    spade = mode == R.SPADE
    L.call.s2e_modulate_fwd(code(dt), mode, d['x'].data_ptr(), d['gb'].data_ptr() if spade else None,
                            d['stats'].data_ptr(), d['style'].data_ptr() + 4 * off if spade else None, out.ptr(), N, HW, C,
                            int(lrelu_on), ld, stream())
    what = tag(dt, N, HW, C, 'modulate_fwd', 'spade' if spade else 'plain', 'lrelu' if lrelu_on else '', 'ld=2C+24' if banked else '')
    out.check(what + ' out')
    report(group, what, 'modulate_fwd', {'out': check(out.t, ref, R.bound_out(ref, A, dt), what + ' out')})


# ---- the backward's forms
def take(case, sl):
    c = dict(case)
    for k in ('x', 'g', 'gb', 'style', 'stats', 'fout', 'gamma'):
        if k in case:
            c[k] = case[k][sl].contiguous()
    c['N'] = c['g'].shape[0]
    return c


def run_mod_bwd(group, dt, N, HW, C, mode, lrelu_on, dev, seed, gamma_only=False, acc=None, banked=False, staged=False, batch=None,
                up=None, quad=False, edge=None):
    """one form of s2e_modulate_bwd.  acc: None / 'inplace' / 'apart'; batch: None / 'count0' / 'replica'; up = (H, W)"""
    spade = mode == R.SPADE
    ld, off = (2 * C + 24, 8) if banked else (0, 0)
    n_all = 2 * N if batch == 'replica' else N
    case = R.make_case(dt, n_all, HW, C, seed, edge=edge, up=up, ld=ld, off=off, batch=batch is not None)
    if spade and not gamma_only and lrelu_on:
        R.clear_kink_band(case)
        assert int(R.kink_band(case).sum()) == 0
    if gamma_only:
        R.add_gamma_only(case, lrelu_on)
    other, count = None, 0.0
    if batch == 'replica':
        mine, rest = take(case, slice(0, N)), take(case, slice(N, 2 * N))
        rs = R.modulate_bwd_ref(R.gamma_only_operands(rest) if gamma_only else R.widen(rest), mode, lrelu_on, gamma_only=gamma_only, batch=True)
        other = tuple(v.sum(0) for v in (rs['sums'][0][..., 0], rs['sums'][0][..., 1], rs['sums'][1][..., 0], rs['sums'][1][..., 1]))
        case, count = mine, 2.0 * N * HW
    t = R.gamma_only_operands(case) if gamma_only else R.widen(case)
    tdt, gen = R.TDT[dt], case['gen']
    hwd = HW // 4 if quad else HW
    dx_start = torch.randn(N, hwd, C, generator=gen).to(tdt) if acc else None
    res = R.modulate_bwd_ref(t, mode, lrelu_on, gamma_only=gamma_only, batch=batch is not None, batch_count=count, other=other, up=up,
                             quad=quad, dx_start=dx_start.double() if acc else None)
    small = gamma_only and spade and batch is None and not staged and HW <= SMALL_HW
    kernel = 'spade_small_bwd' if small else ('reduce+sums+coef' if (batch or staged) else 'reduce+coef') + ('+apply_quad' if quad else '+apply')
    what = tag(dt, N, HW, C, 'modulate_bwd', ('gamma-only' if gamma_only else 'gb-form') if spade else 'plain', 'lrelu' if lrelu_on else '',
               'acc-' + acc if acc else '', 'ld=2C+24' if banked else '', 'staged' if staged else '', 'batch-' + batch if batch else '',
               'x/2 %dx%d' % up if up else '', 'quad' if quad else '', edge)
    flags = (L.NORM_SPADE_STYLE_BATCH if batch else L.NORM_SPADE_STYLE) if spade else L.NORM_PLAIN_IN
    if acc:
        flags |= L.NORM_ACCUMULATE_DX
    d = {k: case[k].to(dev) for k in ('g', 'x', 'stats')}
    gbd = (case['gamma'] if gamma_only else case['gb']).to(dev) if spade else None
    foutd = case['fout'].to(dev) if gamma_only else None
    styled = case['style'].to(dev) if spade else None
    wsb = int(L.call.s2e_modulate_bwd_workspace_bytes(code(dt), N, HW, C))
    ds0 = torch.randn(case['style'].shape, generator=gen).float()

    def buffers(pattern_dx=False):
        b = {'ws': workspace(wsb, dev)}
        if pattern_dx:
            b['dx'] = Guarded((N, hwd, C), tdt, dev, raw_fill=PATTERN)
        else:
            b['dx'] = Guarded((N, hwd, C), tdt, dev, dx_start if acc == 'inplace' else NAN)
        b['add'] = Guarded((N, hwd, C), tdt, dev, dx_start) if acc == 'apart' else None
        b['dgb'] = Guarded((N, HW, 2 * C), tdt, dev, NAN) if spade else None
        b['dstyle'] = Guarded(tuple(ds0.shape), torch.float32, dev, ds0) if spade else None
        return b

    def call(b, stage, cnt):
        L.call.s2e_modulate_bwd(code(dt), flags, d['g'].data_ptr(), d['x'].data_ptr(), ptr(gbd), ptr(foutd), d['stats'].data_ptr(),
                                styled.data_ptr() + 4 * off if spade else None, b['dx'].ptr(), ptr(b['add']), ptr(b['dgb']),
                                b['dstyle'].ptr() + 4 * off if spade else None, b['ws'].ptr(), N, HW, C, int(lrelu_on), ld, stage, cnt,
                                up[1] if up else 0, int(quad), stream())
        torch.cuda.synchronize()
        for k, v in b.items():
            if v is not None:
                v.check('%s stage %d %s' % (what, stage, k))

    def check_dgb(b, worst):
        if spade:
            ref, A = res['dgb']
            worst['dgb'] = check(b['dgb'].t, ref, R.bound_out(ref, A, dt), what + ' dgb')

    def check_final(b, worst):
        worst['dx'] = check(b['dx'].t, res['dx'][0], R.dx_bound(res, dt, not small), what + ' dx')
        if acc == 'apart':
            assert same_bits(b['add'].t, dx_start), what + ': dx_add was written'
        if spade:
            grad, A = res['dstyle']
            got, start = b['dstyle'].t.cpu(), ds0.double()
            inner = start[:, off:off + 2 * C]
            worst['dstyle'] = check(got[:, off:off + 2 * C], inner + grad, R.bound_sum(inner + grad, A, inner), what + ' dstyle')
            keep = torch.ones(ds0.shape[1], dtype=torch.bool)
            keep[off:off + 2 * C] = False
            assert same_bits(got[:, keep], ds0[:, keep]), what + ': dstyle columns outside [off, off + 2C) changed'

    worst = {}
    if not staged:
        b = buffers()
        call(b, 0, count)
        check_dgb(b, worst)
        check_final(b, worst)
    else:
        b = buffers(pattern_dx=True)
        call(b, 1, count)
        check_dgb(b, worst)
        S, AS = res['sums']
        worst['ws'] = check(doubles(b['ws'], N * C * 4).cpu().view(N, C, 4), S, R.bound_sum(S, AS), what + ' ws sums after stage 1')
        assert bool((b['dx'].t.contiguous().view(torch.uint8) == PATTERN).all()), what + ': stage 1 wrote dx'
        if acc != 'inplace':
            b['dx'].t.fill_(NAN)
        else:
            b['dx'].t.copy_(dx_start)
        if batch == 'replica':                              # the all-reduce of a second replica: its S0, S1 folded into ws[0, :, 0:2]
            w = doubles(b['ws'], N * C * 4).view(N, C, 4)
            w[0, :, 0] += other[0].to(dev)
            w[0, :, 1] += other[1].to(dev)
        call(b, 2, count)
        check_final(b, worst)
        if batch != 'replica':
            b0 = buffers()
            call(b0, 0, count)
            what += ' [stage 0 %s]' % ('bit-identical' if same_bits(b0['dx'].t, b['dx'].t) and same_bits(b0['dstyle'].t, b['dstyle'].t)
                                      else 'differs in bits')
    report(group, what, kernel, worst)


# ---- partial-sum slots and column sums
def run_partials(group, P, C, dev, seed):
    N, HW = 3, 8 * P
    gen = torch.Generator().manual_seed(seed)
    data = torch.randn(N, P, 8, C, generator=gen) * 1.3 + 0.2
    part = torch.stack([data.sum(2), (data * data).sum(2)], -1).float().contiguous()        # (N, P, C, 2)
    p64 = part.double()
    st = R.stats_from_sums(p64[..., 0].sum(1), p64[..., 1].sum(1), p64[..., 0].abs().sum(1), p64[..., 1].abs().sum(1), HW)
    ws, stats = Guarded((N, C, 2), torch.float64, dev, NAN), Guarded((N, C, 2), torch.float32, dev, NAN)
    partd = part.to(dev)
    L.call.s2e_in_stats_from_partials(partd.data_ptr(), N, P, C, HW, R.EPS, ws.ptr(), stats.ptr(), stream())
    what, worst = 'fp32 slots N=3 P=%d C=%d from_partials' % (P, C), {}
    ws.check(what + ' ws')
    stats.check(what + ' stats')
    check_stats(stats.t, st, what, worst)
    w = ws.t.cpu()
    worst['sum'] = check(w[..., 0], st['s'], st['d_s'], what + ' ws sum')
    worst['sumsq'] = check(w[..., 1], st['q'], st['d_q'], what + ' ws sum of squares')
    report(group, what, 'in_stats_from_partials', worst)


def run_colsum(group, dt, M, C, dev, seed):
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(M, C, generator=gen).to(R.TDT[dt])
    start = torch.randn(C, generator=gen).float()
    out = Guarded((C,), torch.float32, dev, start)
    gd = g.to(dev)
    L.call.s2e_colsum(code(dt), gd.data_ptr(), M, C, out.ptr(), stream())
    what = '%s %dx%d colsum' % (dt, M, C)
    out.check(what)
    ref = start.double() + g.double().sum(0)
    worst = {'out': check(out.t, ref, R.bound_sum(ref, g.double().abs().sum(0), start.double()), what)}
    report(group, what, 'colsum' if C % R.VEC[dt] == 0 else 'colsum_scalar', worst)


# ---- the groups
MODES = ((R.PLAIN, False), (R.SPADE, False), (R.SPADE, True))                 # (mode, gamma-only)


def group_small(dev, dt):
    """the one-launch kernels (defaults: every listed map is <= 1280 pixels)"""
    shapes = [(n, hw, c) for hw in R.SMALL_HW for n, c in R.SMALL_NC[dt]] + [R.SMALL_G8[dt]]
    for i, (n, hw, c) in enumerate(shapes):
        assert hw <= SMALL_HW
        run_in_stats('small', dt, n, hw, c, dev, 1000 + i)
        for lr in (False, True):
            run_in_fwd('small', dt, n, hw, c, lr, dev, 1100 + i)
            run_in_bwd('small', dt, n, hw, c, lr, dev, 1200 + i)
            run_mod_bwd('small', dt, n, hw, c, R.SPADE, lr, dev, 1300 + i, gamma_only=True)


def group_long(dev, dt):
    """S2E_IN_SMALL_HW=100000: the one-launch kernels with 16+ trips per thread"""
    n, hw, c = R.LONG_SMALL
    assert hw <= SMALL_HW
    run_in_stats('long', dt, n, hw, c, dev, 1400)
    for lr in (False, True):
        run_in_fwd('long', dt, n, hw, c, lr, dev, 1401)
        run_in_bwd('long', dt, n, hw, c, lr, dev, 1402)
        run_mod_bwd('long', dt, n, hw, c, R.SPADE, lr, dev, 1403, gamma_only=True)


def rowwalk_ops(group, dt, n, hw, c, dev, seed):
    assert hw > SMALL_HW
    run_in_stats(group, dt, n, hw, c, dev, seed)
    for lr in (False, True):
        run_in_fwd(group, dt, n, hw, c, lr, dev, seed + 1)
        run_in_bwd(group, dt, n, hw, c, lr, dev, seed + 2)
        for mode in (R.PLAIN, R.SPADE):
            run_mod_fwd(group, dt, n, hw, c, mode, lr, dev, seed + 3)
        for mode, go in MODES:
            run_mod_bwd(group, dt, n, hw, c, mode, lr, dev, seed + 4, gamma_only=go)


def group_rowwalk(dev, dt):
    """S2E_IN_SMALL_HW=0: every slab tail, power-of-two and other channel-group counts"""
    i = 0
    for c in R.ROWWALK_C[dt]:
        for hw in R.ROWWALK_HW[dt]:
            rowwalk_ops('rowwalk', dt, 2, hw, c, dev, 2000 + 10 * i)
            i += 1


def group_boundary(dev, dt):
    """defaults: 1281 pixels, the first map past the small-map boundary (1280 is in group small)"""
    rowwalk_ops('boundary', dt, 2, 1281, 64, dev, 2500)


def group_zblocks(dev, dt):
    """257 channel groups: two blocks along the channel axis, one row per pass, 81 slots"""
    n, hw, c = R.ZBLOCKS2[dt]
    assert R.row_plan(dt, n, hw, c) == (257, 256, 1, 2, 16, 81)
    rowwalk_ops('zblocks', dt, n, hw, c, dev, 2600)


def forms(group, dt, n, hw, c, dev, seed, gamma_only_only=False, up=None):
    for lr in (False, True):
        for mode, go in MODES:
            if gamma_only_only and not go:
                continue
            spade = mode == R.SPADE
            kw = dict(gamma_only=go)
            run_mod_bwd(group, dt, n, hw, c, mode, lr, dev, seed, **kw)
            run_mod_bwd(group, dt, n, hw, c, mode, lr, dev, seed + 1, acc='inplace', **kw)
            run_mod_bwd(group, dt, n, hw, c, mode, lr, dev, seed + 2, acc='apart', **kw)
            if spade:
                run_mod_bwd(group, dt, n, hw, c, mode, lr, dev, seed + 3, banked=True, **kw)
                if not gamma_only_only:
                    run_mod_bwd(group, dt, n, hw, c, mode, lr, dev, seed + 4, staged=True, **kw)
                    run_mod_bwd(group, dt, n, hw, c, mode, lr, dev, seed + 5, staged=True, banked=True, acc='apart', **kw)
                    run_mod_bwd(group, dt, n, hw, c, mode, lr, dev, seed + 6, batch='count0', **kw)
                    run_mod_bwd(group, dt, n, hw, c, mode, lr, dev, seed + 7, batch='count0', staged=True, **kw)
                    run_mod_bwd(group, dt, n, hw, c, mode, lr, dev, seed + 8, batch='replica', staged=True, **kw)
        if up:
            h, w = up
            run_mod_bwd(group, dt, n, h * w, c, R.SPADE, lr, dev, seed + 9, gamma_only=True, up=up)
            run_mod_bwd(group, dt, n, h * w, c, R.SPADE, lr, dev, seed + 10, gamma_only=True, up=up, quad=True)
            run_mod_bwd(group, dt, n, h * w, c, R.SPADE, lr, dev, seed + 11, gamma_only=True, up=up, quad=True, acc='inplace')
            run_mod_bwd(group, dt, n, h * w, c, R.SPADE, lr, dev, seed + 12, gamma_only=True, up=up, quad=True, acc='apart', banked=True)


def group_forms(dev, dt):
    """S2E_IN_SMALL_HW=0: every form of s2e_modulate_bwd on the row walk"""
    assert SMALL_HW == 0
    for i, (n, hw, c) in enumerate(R.FORM_SHAPES):
        forms('forms', dt, n, hw, c, dev, 3000 + 20 * i, up=R.UP_ROWWALK)
        run_mod_fwd('forms', dt, n, hw, c, R.SPADE, True, dev, 3015 + 20 * i, banked=True)


def group_forms_small(dev, dt):
    """defaults: the gamma-only forms on the one-launch kernel (289 pixels; x at half resolution of a 16 x 18 map)"""
    assert SMALL_HW >= 289
    forms('forms-s', dt, 2, 289, 64, dev, 3100, gamma_only_only=True, up=R.UP_SMALL)
    forms('forms-s', dt, 2, 289, 72, dev, 3120, gamma_only_only=True)


def group_edge(dev, dt):
    """an exactly constant channel (0 and 1.5: LeakyReLU's slope AT zero is 0.2), and a channel with mean / std ~ 6"""
    n, hw, c = (2, 35, 8) if SMALL_HW == 0 else (2, 289, 8)
    for i, edge in enumerate(('const0', 'const1.5', 'shifted')):
        for lr in (False, True):
            run_in_fwd('edge', dt, n, hw, c, lr, dev, 4000 + i, edge=edge)
            run_in_bwd('edge', dt, n, hw, c, lr, dev, 4010 + i, edge=edge)
            for mode, go in MODES:
                run_mod_bwd('edge', dt, n, hw, c, mode, lr, dev, 4020 + i, gamma_only=go, edge=edge)


def group_partials(dev, dt):
    for i, p in enumerate(R.PARTIALS_P):
        for j, c in enumerate(R.PARTIALS_C):
            run_partials('partials', p, c, dev, 5000 + 10 * i + j)


def group_colsum(dev, dt):
    for i, (m, c) in enumerate(R.COLSUM[dt]):
        run_colsum('colsum', dt, m, c, dev, 6000 + i)


def group_wrap(dev, dt):
    """the element-wise kernels' grid capped at 8192 blocks: a thread takes a second vector of its sample"""
    n, hw, c = R.WRAP[dt]
    assert hw > SMALL_HW and n * hw * (c // R.VEC[dt]) > 8192 * 256 and R.row_plan(dt, n, hw, c)[4] == 33
    run_mod_fwd('wrap', dt, n, hw, c, R.SPADE, True, dev, 7000)
    run_mod_bwd('wrap', dt, n, hw, c, R.SPADE, True, dev, 7001)


GROUPS = {'small': group_small, 'long': group_long, 'rowwalk': group_rowwalk, 'boundary': group_boundary, 'zblocks': group_zblocks,
          'forms': group_forms, 'forms_small': group_forms_small, 'edge': group_edge, 'partials': group_partials, 'colsum': group_colsum,
          'wrap': group_wrap}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--groups', required=True)
    ap.add_argument('--dtype', required=True, choices=('bf16', 'fp32'))
    args = ap.parse_args()
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    dev = torch.device('cuda', 0)
    L.lib()
    for name in args.groups.split(','):
        GROUPS[name](dev, args.dtype)
    print('norm ok: %d checks, groups %s, %s (S2E_IN_SMALL_HW=%s)' % (len(RESULTS), args.groups, args.dtype,
                                                                    os.environ.get('S2E_IN_SMALL_HW', 'default')), flush=True)


if __name__ == '__main__':
    main()
