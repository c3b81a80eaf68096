"""The weight-gradient job tables -- s2e_conv2d_wgrad_multi (generic tile kernel, conv_wgrad_flat.hip, conv_c8.hip), s2e_wgrad_batch and
s2e_wgrad_c8_batch -- on tables built where their host planners can go wrong: chunk boundaries (WGM_MAX_JOBS 26, WF_MAX_JOBS 24,
C8W_MAX_JOBS 4, WC_MAX_JOBS 24), lopsided shares of a fixed workgroup budget, jobs sharing dw / dbias (overlapping ranges included),
a workspace that is exact, 256 bytes short, half the size or absent.  Every result is checked against fp64 sums of the same bf16 operands, accumulated
into non-zero outputs, and every workspace is followed by a guard band that must come back unchanged (tests/_wgrad_tables_child.py)."""
import os
import subprocess
import sys

import pytest
import torch

import _wgrad_tables_child as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    return torch.device('cuda:0')


_OPS = {}


def _ops(name):
    """fp64 references of a table, computed once per table and process"""
    if name not in _OPS:
        _OPS[name] = T.operands(T.TABLES[name], 1, _dev())
    return _OPS[name]


def test_c8_lopsided_table_is_over_budget_before_the_clamp():
    """The c8 cases stay meaningful if their shapes are edited: unclamped, one big and three tiny jobs ask for more than a chunk's 512
    partial tiles (and so does the last chunk of the 7-job table and the first of the 9-job one)."""
    c8_jobs = lambda name: [j for j in T.TABLES[name] if j[8] == 6]
    assert sum(T.c8_shares(c8_jobs('c8_lopsided'))) > T.C8_WGS
    assert sum(T.c8_shares(c8_jobs('c8_chunk7')[4:])) > T.C8_WGS
    assert sum(T.c8_shares(c8_jobs('c8_chunk9')[:4])) > T.C8_WGS
    assert sum(T.c8_shares(c8_jobs('all_kinds')[:4])) > T.C8_WGS
    for name in ('c8_lopsided', 'c8_chunk5', 'c8_chunk7', 'c8_chunk9'):
        n = len(c8_jobs(name))
        assert T.workspace_bytes(T.TABLES[name]) == -(-n // T.C8_MAX_JOBS) * T.C8_WGS * T.C8W_TILE_BYTES


def test_generic_shared_jobs_each_use_partial_tiles():
    """gen_shared is the race of conv_wgrad_reduce_multi_kernel only if every job stores partial tiles: each alone needs a workspace."""
    for j in T.TABLES['gen_shared']:
        assert T.workspace_bytes([j]) > 0


_NO_WORKSPACE = ('flat25',)        # (flat jobs use none: no 'short' and no 'half' case)


@pytest.mark.parametrize('name,mode', [(t, m) for t in T.TABLES for m in ('exact', 'short', 'half', 'none')
                                       if not (m in ('short', 'half') and t in _NO_WORKSPACE)])
def test_wgrad_multi_table_against_fp64(name, mode):
    """s2e_conv2d_wgrad_multi on one table: kinds as planned, guard band intact, every output buffer = its start + the fp64 sums of
    the jobs writing there (2e-4 x max |sum|)."""
    assert (T.workspace_bytes(T.TABLES[name]) == 0) == (name in _NO_WORKSPACE)
    T.run(name, mode, _dev(), _ops(name))


# the switches the library reads once per process, in a child each: the tables they bear on
_CHILD = [
    ({'S2E_C8W_WGS': '500'}, 'c8_lopsided,c8_chunk7,c8_chunk9,all_kinds'),
    ({'S2E_C8W_WGS': '37'}, 'c8_lopsided,c8_chunk5,c8_chunk7,c8_chunk9'),
    ({'S2E_WGRAD_MULTI_WGS': '1'}, 'gen_shared,gen_mixed,gen_chunk27,gen_chunk53,all_kinds'),
    ({'S2E_WGRAD_MULTI_WGS': '100000'}, 'gen_shared,gen_mixed,gen_chunk27,gen_chunk53,all_kinds'),
    ({'S2E_WGRAD_FLAT_WGS': '1'}, 'flat25,all_kinds'),
    ({'S2E_WGRAD_PARTIAL': '2'}, 'gen_shared,gen_mixed,gen_chunk27,gen_chunk53,all_kinds'),
]


@pytest.mark.parametrize('env,tables', _CHILD, ids=['%s=%s' % next(iter(e.items())) for e, _ in _CHILD])
def test_wgrad_multi_tables_under_switches(env, tables):
    e = dict(os.environ)
    for k in ('S2E_C8W_WGS', 'S2E_WGRAD_MULTI_WGS', 'S2E_WGRAD_FLAT_WGS', 'S2E_WGRAD_PARTIAL', 'S2E_WGRAD_FLAT', 'S2E_CONV_C8',
              'S2E_DETERMINISTIC', 'S2E_WF_NOEPI'):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_wgrad_tables_child.py'), '--tables', tables], env=e,
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0 and 'tables ok:' in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


def test_wgrad_batch_guard_band_and_shared_dw_rejection():
    """s2e_wgrad_batch: 36 jobs into non-zero dW against fp64 with a guard band behind the workspace; a table with two jobs on one dW
    comes back S2E_ERR_ARG with a message, before anything runs (dW untouched)."""
    T.wgrad_batch_guard(_dev())


def test_wgrad_c8_batch_two_rounds_guard_band():
    """s2e_wgrad_c8_batch: 25 jobs (one more than an argument block holds) against fp64, guard band behind the workspace."""
    T.wgrad_c8_batch_guard(_dev())


# ---- GradSink.is_pinned: a queued gy is pinned through ANY view of its memory
def _queue_one(pool_dev, which):
    """Queue one weight-gradient job whose gy lives in a bigger buffer; returns (buffer, gy)"""
    from seg2eye_amd import ops
    g = torch.Generator().manual_seed(31)
    if which == 'gwg':                                   # generic: 1x1, 64 -> 64 on 16 x 16 (s2e_conv2d_wgrad_multi)
        x = torch.randn(2, 16, 16, 64, generator=g).to(pool_dev).to(torch.bfloat16)
        buf = torch.randn(3 * 2 * 16 * 16 * 64, generator=g).to(pool_dev).to(torch.bfloat16)
        gy = buf[2 * 16 * 16 * 64:2 * 2 * 16 * 16 * 64].view(2, 16, 16, 64)
        dw = torch.zeros(64, 64, device=pool_dev)
        assert ops.GradSink.push_gwg(x, gy, dw, None, (2, 16, 16, 64, 16, 16, 64, 1, 1, 1, 0, 0, 0, 0, 0))
    else:                                                # patch-resident 3x3 (s2e_wgrad_batch)
        x = torch.randn(2, 16, 16, 64, generator=g).to(pool_dev).to(torch.bfloat16)
        buf = torch.randn(3 * 2 * 16 * 16 * 64, generator=g).to(pool_dev).to(torch.bfloat16)
        gy = buf[2 * 16 * 16 * 64:2 * 2 * 16 * 16 * 64].view(2, 16, 16, 64)
        dw = torch.zeros(64, 9 * 64, device=pool_dev)
        assert ops.GradSink.push_wgrad(x, gy, dw, None)
    return buf, gy


@pytest.mark.parametrize('which', ['gwg', 'wgrad'])
def test_is_pinned_sees_every_view_of_a_queued_gy(which):
    from seg2eye_amd import ops
    dev = _dev()
    pool = ops.ZeroPool(dev)
    n = 2 * 16 * 16 * 64
    with pool.scope('t'):
        buf, gy = _queue_one(dev, which)
        assert ops.GradSink.is_pinned(gy)
        assert ops.GradSink.is_pinned(buf[n + 64:2 * n + 64])                    # a view at another offset, overlapping
        assert ops.GradSink.is_pinned(buf[n // 2:n // 2 + n].view(2, 16, 16, 64))  # ... from the other side
        assert ops.GradSink.is_pinned(gy.reshape(-1, 64))                        # a reshaped alias
        assert ops.GradSink.is_pinned(buf[2 * n - 1:2 * n])                      # the last element alone
        assert ops.GradSink.is_pinned(buf)                                       # the whole buffer
        assert not ops.GradSink.is_pinned(buf[:n])                               # disjoint slices of the same storage
        assert not ops.GradSink.is_pinned(buf[2 * n:])
        assert not ops.GradSink.is_pinned(buf.clone()[n:2 * n])                  # another tensor
        assert not ops.GradSink.is_pinned(torch.zeros_like(gy))
    assert not ops.GradSink.is_pinned(gy)                                        # flushed at scope exit


def test_modulate_relay_into_an_offset_view_of_a_queued_gy():
    """ModulateFn's relay handed a gradient that is an offset view of a queued weight-gradient job's gy: it must not add in place (the
    queued job would read the sum at the flush).  dW from the scope (queued, flushed) must equal the eager path's; so must dx."""
    from seg2eye_amd import ops
    from seg2eye_amd.ops import spade as S
    from types import SimpleNamespace
    dev = _dev()
    g = torch.Generator().manual_seed(41)
    n, h, w, c = 2, 16, 16, 64
    m = n * h * w * c
    xw = torch.randn(n, h, w, 64, generator=g).to(dev).to(torch.bfloat16)         # the conv whose weight gradient is queued: 1x1, 64 -> c
    base = torch.randn(m + 4 * c, generator=g).to(dev).to(torch.bfloat16)
    x = (torch.randn(n, h, w, c, generator=g) * 1.3 + 0.2).to(dev).to(torch.bfloat16)
    gb = (torch.randn(n, h, w, 2 * c, generator=g) * 0.5).to(dev).to(torch.bfloat16)
    style = (torch.randn(n, 2 * c, generator=g) * 0.5).to(dev)
    gout = torch.randn(n, h, w, c, generator=g).to(dev).to(torch.bfloat16)
    stats = ops.in_stats(x)
    ctx = SimpleNamespace(lrelu=False, off=None, dbig=None, batch=False, relay=True)

    def step(scoped):
        buf = base.clone()
        gy = buf[:m].view(n, h, w, c)                           # the conv's output gradient
        g_relay = buf[4 * c:4 * c + m].view(n, h, w, c)         # ... and the relayed gradient: the same memory, 4 pixels further
        dw = torch.zeros(c, 64, device=dev)
        pool = ops.ZeroPool(dev)

        def body():
            ops.conv2d_wgrad_raw(xw, gy, 1, 1, 1, 0, ops.ACT_NONE, False, None, dw_out=dw, defer_ok=True)
            if scoped:
                assert len(pool.sink.gwg) == 1                  # queued: it reads gy at the flush
            dx, _, _ = S._modulate_grads(ctx, gout, g_relay, x, gb, None, style, stats)
            return dx
        if scoped:
            with pool.scope('t'):
                dx = body()
        else:
            dx = body()
        torch.cuda.synchronize()
        return dw, dx
    dw_e, dx_e = step(False)
    dw_s, dx_s = step(True)
    assert float(dw_e.abs().max()) > 0
    assert float((dw_s - dw_e).abs().max()) <= 3e-5 * float(dw_e.abs().max()) + 1e-6
    assert float((dx_s.float() - dx_e.float()).abs().max()) <= 1e-2 * float(dx_e.float().abs().max())
