"""The fp64 reference, the bound and the plan mirror of tests/_wgrad_generic_child.py, on the CPU: the weight-gradient reference against
torch's autograd in fp64 and against the sum written out tap by tap, the LeakyReLU operand on hand-picked values, the mirror of
wgrad_params / generic_wgrad_plan / wgrad_use_partial / generic_partial_bytes / wgrad_chunk_plan against the tree's library (a child
process per environment), the depth condition of the bound and the coverage counters over the shipped lists, and the sensitivity of
the bound to the errors it exists to catch.  No GPU needed."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import _wgrad_generic_child as T
import test_wgrad_generic_fp64_gpu as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_GROUPS = 'big,mid,one,det,multi'


def _t(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize('k,s,p', [(1, 1, 0), (3, 1, 1), (3, 2, 1), (3, 1, 0), (4, 2, 2), (4, 1, 2), (1, 2, 0), (4, 2, 1)])
@pytest.mark.parametrize('hw', [(7, 9), (10, 5)])
def test_wgrad_reference_matches_torch_autograd_fp64(k, s, p, hw):
    n, ci, co = 2, 3, 5
    c = T.Case(n, hw[0], hw[1], ci, co, k, s, p)
    ho, wo = T.out_hw(c)
    x, gy = _t((n, hw[0], hw[1], ci), 1), _t((n, ho, wo, co), 3)
    w = _t((co, ci, k, k), 2).requires_grad_(True)
    b = torch.zeros(co, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.permute(0, 3, 1, 2), w, b, stride=s, padding=p).backward(gy.permute(0, 3, 1, 2))
    want = w.grad.permute(0, 2, 3, 1).reshape(co, k * k * ci)                    # k = (ky KW + kx) Cin + ci
    assert torch.allclose(T.wgrad64(x, gy, k, s, p), want, rtol=1e-12, atol=1e-12)
    ref, A, rb, Ab = T.reference(c, x, gy)
    assert torch.equal(ref, T.wgrad64(x, gy, k, s, p)) and torch.allclose(rb, b.grad, rtol=1e-12, atol=1e-12)
    assert bool((A >= ref.abs() - 1e-12).all()) and bool((Ab >= rb.abs() - 1e-12).all())


def test_wgrad_reference_against_the_sum_written_out():
    """elements of a 4x4 stride-2 pad-2 weight gradient, tap by tap: a corner tap (mostly padding), an inner one, the last one"""
    n, h, w, ci, co, k, s, p = 2, 7, 6, 3, 2, 4, 2, 2
    c = T.Case(n, h, w, ci, co, k, s, p)
    ho, wo = T.out_hw(c)
    x, gy = _t((n, h, w, ci), 4), _t((n, ho, wo, co), 6)
    dw = T.wgrad64(x, gy, k, s, p)
    assert tuple(dw.shape) == (co, k * k * ci)
    for o, ky, kx, i in ((0, 0, 0, 0), (1, 2, 1, 2), (0, 3, 3, 1)):
        acc = 0.0
        for b in range(n):
            for oy in range(ho):
                for ox in range(wo):
                    iy, ix = oy * s - p + ky, ox * s - p + kx
                    if 0 <= iy < h and 0 <= ix < w:
                        acc += float(gy[b, oy, ox, o] * x[b, iy, ix, i])
        assert abs(acc - float(dw[o, (ky * k + kx) * ci + i])) < 1e-12


@pytest.mark.parametrize('dt', ['bf16', 'f32'])
def test_lrelu_operand_of_the_reference(dt):
    """the x operand under in_act = LRELU: bf16 -- the RNE rounding of the fp32 product 0.2f * x; fp32 -- that product itself"""
    dtype = torch.bfloat16 if dt == 'bf16' else torch.float32
    x = torch.tensor([1.0, -1.0, -3.0, 0.0, -0.3359375, 2.5]).to(dtype)
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)                           # noqa: E731
    want = [1.0, float((f32(-1.0) * f32(0.2)).to(dtype)), float((f32(-3.0) * f32(0.2)).to(dtype)), 0.0,
            float((f32(-0.3359375) * f32(0.2)).to(dtype)), 2.5]
    assert T.operand64(x, T.ACT_LRELU, dtype).tolist() == want
    if dt == 'bf16':
        assert want[1] == -0.2001953125 and want[2] == -0.6015625                  # bf16 values, not the fp32 products
    else:
        assert want[1] == float(f32(0.2)) * -1.0 and want[2] == float(f32(-3.0) * f32(0.2)) and want[2] != -0.6
    # reference() multiplies that operand
    c = T.Case(1, 1, 6, 1, 1, 1, 1, 0, dt=dt, lrelu=True)
    gy = torch.tensor([1.0, 2.0, -1.0, 5.0, 4.0, 0.5]).to(dtype)
    ref, A, rb, Ab = T.reference(c, x.view(1, 1, 6, 1), gy.view(1, 1, 6, 1))
    assert float(ref) == sum(a * b for a, b in zip(want, gy.tolist())) and float(A) == sum(abs(a * b) for a, b in zip(want, gy.tolist()))
    assert float(rb) == 11.5 and float(Ab) == 13.5


def test_plan_mirror_on_shapes_worked_out_by_hand():
    """(M, k-tiles x co-tiles, splits, pixels per split, pixels of the last split)"""
    want = {
        T.BIG[0]: (9216, 1, 1, 36, 256, 256), T.BIG[1]: (9216, 1, 1, 36, 256, 256), T.BIG[2]: (32768, 1, 1, 128, 256, 256),
        T.BIG[3]: (38000, 1, 1, 119, 320, 240), T.BIG[4]: (9514, 5, 2, 17, 576, 298),
        T.MID[0]: (4225, 8, 1, 8, 576, 193), T.MID[1]: (4225, 1, 1, 14, 320, 65), T.MID[2]: (2303, 2, 1, 8, 320, 63),
        T.MID[3]: (2400, 1, 1, 8, 320, 160), T.MID[4]: (1760, 1, 1, 6, 320, 160), T.MID[6]: (1568, 2, 1, 5, 320, 288),
        T.ONE[0]: (798, 8, 1, 1, 832, 798), T.ONE[1]: (512, 3, 2, 1, 512, 512), T.ONE[2]: (105, 2, 1, 1, 128, 105),
        T.ONE[3]: (33, 1, 1, 1, 64, 33), T.ONE[4]: (1, 1, 1, 1, 64, 1), T.ONE[5]: (30, 9, 1, 1, 64, 30),
    }
    for c, w in want.items():
        pl = T.plan(c)
        assert (pl['M'], pl['tiles_k'], pl['tiles_co'], pl['splits'], pl['m_per_split'], pl['last']) == w, (c, pl)
    # a job's share of a multi-job launch instead of 2048 workgroups, and no filling of the chip by one job alone
    c = T.Case(2, 64, 64, 64, 64, 1, 1, 0)
    assert (T.plan(c)['splits'], T.plan(c, 3000)['splits'], T.plan(c, 5)['splits']) == (32, 8, 5)
    # the thresholds of wgrad_use_partial
    assert [T.use_partial(s, 'default') for s in (1, 2, 15, 16)] == [False, False, False, True]
    assert [T.use_partial(s, 'partial2') for s in (1, 2)] == [False, True]
    assert [T.use_partial(s, 'partial0') for s in (1, 16, 128)] == [False, False, False]
    assert [T.use_partial(s, 'det') for s in (1, 2)] == [True, True]
    assert T.partial_bytes(T.plan(T.BIG[4])) == 10 * 17 * (128 * 128 + 128) * 4


def _every_case():
    for name in ('big', 'mid', 'one'):
        for c in T.GROUPS[name]:
            yield name, c


def test_every_case_is_inside_the_derivation_of_the_bound():
    """depth 2^-24 <= C_ACC for dw and for dbias, every shipped case, every job of the multi-job call with its share's splits"""
    assert T.DEPTH_MAX * 2.0 ** -24 == T.C_ACC
    worst = 0
    for name, c in _every_case():
        pl, dt = T.plan(c), T.dt_of(c)
        assert T.depth(pl, dt) <= T.DEPTH_MAX, (c, T.depth(pl, dt))
        assert T.bias_depth(pl, dt) <= T.DEPTH_MAX, (c, T.bias_depth(pl, dt))
        assert T.split_class(pl['splits']) is not None, (c, pl['splits'])
        assert c.k in (1, 3, 4) and c.s in (1, 2)
        worst = max(worst, T.depth(pl, dt))
    assert T.depth(T.plan(T.BIG[1]), T.S2E_F32) == 128 + 36 + 3                            # the fp32 1x1 case with 36 splits
    assert worst == T.depth(T.plan(T.MID[4]), T.S2E_F32) == 160 + 6 + 3                    # the fp32 3x3 case: 6 splits of 320
    assert all(c in T.BIG + T.MID + T.ONE for c in T.DET)
    plans, _ = T.multi_plan(T.MULTI, 'det')
    by_bias = {}
    for j, pl in zip(T.MULTI, plans):
        assert T.depth(pl, T.S2E_BF16) <= T.DEPTH_MAX, (j, pl)
        by_bias[j.db] = by_bias.get(j.db, 0) + T.bias_depth(pl, T.S2E_BF16)
    assert all(v <= T.DEPTH_MAX for k, v in by_bias.items() if k), by_bias
    # unsplit fp32 cases: M <= 448
    assert T.depth(T.plan(T.Case(1, 16, 28, 4, 4, 1, 1, 0, dt='f32')), T.S2E_F32) <= T.DEPTH_MAX
    assert T.depth(T.plan(T.Case(1, 16, 29, 4, 4, 1, 1, 0, dt='f32')), T.S2E_F32) > T.DEPTH_MAX


def test_coverage_counters_of_the_shipped_lists():
    cov = T.coverage()
    assert sorted(cov) == sorted(T.COUNTERS)
    assert [k for k, v in cov.items() if v == 0] == []
    # the multi-job call: four jobs of conv_wgrad_flat.hip's kinds and one that is none of them, two on one dbias, one without
    kinds = [(j.k, j.s, j.p) for j in T.MULTI]
    assert {(1, 1, 0), (4, 2, 2), (3, 2, 1)} <= set(kinds) and (3, 1, 1) in kinds
    assert all(j.cin % 64 == 0 and j.cout % 8 == 0 for j in T.MULTI if (j.k, j.s, j.p) != (3, 1, 1))
    dbs = [j.db for j in T.MULTI]
    assert None in dbs and max(dbs.count(b) for b in set(dbs) if b) == 2
    plans, total = T.multi_plan(T.MULTI, 'det')
    assert all(p is not None for p in plans) and any(p['splits'] == 1 for p in plans) and any(p['splits'] > 1 for p in plans)
    assert total == sum(p['tiles'] * p['splits'] for p in plans) * (128 * 128 + 128) * 4


def test_lrelu_cases_have_negative_zero_and_positive_inputs():
    n = 0
    for name, c in _every_case():
        if c.lrelu:
            x = T.operands(c, 3000 + 41 * (T.BIG + T.MID + T.ONE).index(c))[0]
            assert int((x == 0).sum()) > 0 and int((x < 0).sum()) > 0 and int((x > 0).sum()) > 0, c
            n += 1
    assert n >= 3


def test_gpu_children_run_every_group_in_the_environment_it_is_written_for():
    ran = {}
    for cid, env, groups in G._CHILDREN:
        assert T.env_name(env) == cid and T.ENVS[cid] == env
        for name in groups.split(','):
            assert name in T.GROUPS or name == 'multi', name
            assert name in T.ENV_GROUPS[cid]
            ran.setdefault(cid, []).append(name)
    assert ran == {'default': ['big', 'mid', 'one'], 'partial2': ['big', 'mid'], 'partial0': ['big'], 'det': ['det', 'multi']}
    assert all(T.plan(c)['splits'] >= 16 for c in T.BIG) and all(2 <= T.plan(c)['splits'] <= 15 for c in T.MID)
    assert all(T.plan(c)['splits'] == 1 for c in T.ONE)
    assert any(T.plan(c)['splits'] == 1 and c.bias and T.plan(c)['tiles_k'] > 1 for c in T.DET)
    for k in T.SWITCHES:
        with pytest.raises(AssertionError):
            T.env_name({k: '3'})


@pytest.fixture(scope='module')
def built():
    import __graft_entry__
    __graft_entry__.build()


@pytest.mark.parametrize('env', list(T.ENVS.values()), ids=list(T.ENVS))
def test_library_routes_and_workspace_match_the_mirror(built, env):
    """s2e_conv2d_wgrad_kernel_kind and s2e_conv2d_wgrad_workspace_bytes of the tree's library for EVERY case in every environment --
    under S2E_WGRAD_PARTIAL=2 every split launch shows its tiles x splits in the size, under S2E_DETERMINISTIC=1 every launch -- and
    s2e_conv2d_wgrad_multi_kind / s2e_conv2d_wgrad_multi_workspace_bytes of the multi-job call with the shares' splits"""
    e = {k: v for k, v in os.environ.items() if k not in T.SWITCHES}
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_wgrad_generic_child.py'), '--plan', '--groups', ALL_GROUPS],
                       env=e, capture_output=True, text=True, timeout=600, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0 and 'wgrad generic plan ok: 36 cases' in r.stdout, (r.stdout[-4000:], r.stderr[-4000:])


# ---- sensitivity of the bound
def _xcol(c, xo):
    """(M, K) fp64: the operand rows of the weight gradient, k = (ky KW + kx) Cin + ci"""
    ho, wo = T.out_hw(c)
    xp = F.pad(xo, (0, 0, c.p, c.p, c.p, c.p))
    cols = [xp[:, ky:ky + c.s * (ho - 1) + 1:c.s, kx:kx + c.s * (wo - 1) + 1:c.s] for ky in range(c.k) for kx in range(c.k)]
    return torch.cat(cols, dim=-1).reshape(-1, c.k * c.k * c.cin)


def _setup(c, seed):
    x, gy, dw0, db0 = T.operands(c, seed)
    ref, A, rb, Ab = T.reference(c, x, gy)
    xo = T.operand64(x, T.ACT_LRELU if c.lrelu else T.ACT_NONE, T.dtype_of(c))
    g = gy.double().reshape(-1, c.cout)
    col = _xcol(c, xo)
    assert torch.allclose(g.t() @ col, ref, rtol=1e-12, atol=1e-9)
    return dict(c=c, pl=T.plan(c), x=x, g=g, col=col, dw0=dw0.double(), db0=db0.double(), ref=ref, A=A, rb=rb, Ab=Ab)


@pytest.fixture(scope='module')
def largest():
    """the largest-M bf16 case of the shipped lists (a lost pixel is hardest to see there), and the largest one with a bias spread
    over several k-tiles"""
    cases = [c for _, c in _every_case() if c.dt == 'bf16']
    big = max(cases, key=lambda c: T.plan(c)['M'])
    spread = max((c for c in cases if c.bias and T.plan(c)['tiles_k'] > 1), key=lambda c: T.plan(c)['M'])
    assert T.plan(big)['M'] == 38000 and T.plan(spread)['M'] == 9514 and T.plan(spread)['tiles_k'] == 5
    return _setup(big, 11), _setup(spread, 12)


def _dw_check(s, summed, what):
    got = (s['dw0'] + summed).float()                              # what a correct fp32 add of the sums into `start` leaves
    return T.check_close(got, s['ref'], s['A'] + s['dw0'].abs(), what, rel=0.0, start=s['dw0'])


def test_bound_passes_the_rounded_reference_and_fails_a_nan(largest):
    for s in largest:
        assert _dw_check(s, s['ref'], 'rounded reference') <= 1.0
    s = largest[0]
    got = (s['dw0'] + s['ref']).float()
    got[3, 5] = float('nan')
    with pytest.raises(AssertionError, match='outside the bound'):
        T.check_close(got, s['ref'], s['A'] + s['dw0'].abs(), 'a NaN from the workspace', rel=0.0, start=s['dw0'])


def test_bound_catches_a_lost_pixel(largest):
    """(a) one pixel of 38000 missing from every element's sum (a row masked by a wrong m_end, an off-by-one pixel advance)"""
    s = largest[0]
    m = 23456
    lost = s['ref'] - torch.outer(s['g'][m], s['col'][m])
    with pytest.raises(AssertionError, match='outside the bound'):
        _dw_check(s, lost, 'one lost pixel')


def test_bound_catches_a_lost_chunk_and_a_split_added_twice(largest):
    """(b) one 32-pixel chunk missing (the last chunk of a split not computed); (c) one split's tile added twice (a reduce that reads a
    slot twice, a workgroup that runs twice)"""
    s = largest[0]
    mps = s['pl']['m_per_split']
    lo = 57 * mps + 3 * 32
    lost = s['ref'] - s['g'][lo:lo + 32].t() @ s['col'][lo:lo + 32]
    with pytest.raises(AssertionError, match='outside the bound'):
        _dw_check(s, lost, 'one lost chunk')
    lo = (s['pl']['splits'] - 1) * mps                              # the short last split: the smallest
    twice = s['ref'] + s['g'][lo:].t() @ s['col'][lo:]
    assert s['g'][lo:].shape[0] == 240
    with pytest.raises(AssertionError, match='outside the bound'):
        _dw_check(s, twice, 'one split twice')


def test_bound_catches_a_bias_that_misses_one_k_tiles_chunks(largest):
    """(d) the bias sum is spread over the k-tile workgroups (chunk ch of a split by the one with tk == ch % tiles_k): the rows of one
    k-tile's chunks missing -- and, smaller, of one k-tile's chunks of ONE split"""
    s = largest[1]
    pl = s['pl']
    m = torch.arange(pl['M'])
    ch = (m % pl['m_per_split']) // 32
    for what, miss in (('one k-tile of every split', ch % pl['tiles_k'] == 2),
                       ('one k-tile of one split', (ch % pl['tiles_k'] == 2) & (m // pl['m_per_split'] == 9))):
        assert int(miss.sum()) >= 96
        got = (s['db0'] + s['g'][~miss].sum(0)).float()
        with pytest.raises(AssertionError, match='outside the bound'):
            T.check_close(got, s['rb'], s['Ab'] + s['db0'].abs(), what, rel=0.0, start=s['db0'])
    good = (s['db0'] + s['rb']).float()
    assert T.check_close(good, s['rb'], s['Ab'] + s['db0'].abs(), 'rounded bias reference', rel=0.0, start=s['db0']) <= 1.0


def test_bound_catches_a_wrong_lrelu_operand():
    """(e) on the bf16 LeakyReLU case: an operand 0.2f * x kept in fp32 instead of rounded back to bf16 is off by up to 2^-9 relative
    on every negative input -- over 2303 pixels that leaves 1976 of the 8640 elements outside the bound (the first by 1.3 bounds), so
    the bound does tell the two roundings apart.  Coarser mistakes on the same case: the activation left out, the slope on the wrong
    side."""
    c = T.MID[2]
    assert c.lrelu and c.dt == 'bf16'
    s = _setup(c, 13)
    assert _dw_check(s, s['ref'], 'rounded reference') <= 1.0
    xf = s['x'].float()
    for what, xo in (('unrounded', torch.where(xf > 0, xf, xf * 0.2).double()), ('no activation', xf.double()),
                     ('slope on the positive side', torch.where(xf < 0, xf, xf * 0.2).double())):
        with pytest.raises(AssertionError, match='outside the bound'):
            _dw_check(s, s['g'].t() @ _xcol(c, xo), what)
