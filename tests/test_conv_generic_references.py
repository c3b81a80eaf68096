"""The fp64 references and plan mirrors of tests/_conv_generic_child.py, on the CPU: the general convolution and its transposed form
against torch's own fp64 convolution and autograd, the absolute-value twin of every epilogue, the stream-K and split-K plan mirrors
against the tree's library (a child process per environment), the coverage counters of the shipped case lists at 256 CUs, and the
sensitivity of the bound to the errors it exists to catch.  No GPU needed."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import _conv_generic_child as T
import test_conv_generic_fp64_gpu as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _t(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize('k,s,p', [(1, 1, 0), (3, 1, 1), (3, 2, 1), (4, 1, 2), (4, 2, 2), (4, 2, 1), (1, 2, 0), (3, 1, 0)])
@pytest.mark.parametrize('hw', [(7, 9), (10, 5)])
def test_conv_references_match_torch_fp64(k, s, p, hw):
    n, ci, co = 2, 3, 5
    g = T.Geo(n, hw[0], hw[1], ci, co, k, s, p, False)
    ho, wo = T.out_hw(g)
    x, w, gy = _t((n, hw[0], hw[1], ci), 1), _t((co, ci, k, k), 2), _t((n, ho, wo, co), 3)
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = F.conv2d(xr, w, stride=s, padding=p)
    y.backward(gy.permute(0, 3, 1, 2))
    assert torch.allclose(T.conv64(x, w, k, s, p, False, (ho, wo)), y.detach().permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    assert torch.allclose(T.conv64(gy, w, k, s, p, True, hw), xr.grad.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)


def test_forward_reference_against_the_sum_written_out():
    """one output element of a 4x4 stride-2 pad-2 conv and one of its data gradient, tap by tap"""
    g = T.Geo(1, 7, 6, 3, 2, 4, 2, 2, False)
    ho, wo = T.out_hw(g)
    x, w, gy = _t((1, 7, 6, 3), 4), _t((2, 3, 4, 4), 5), _t((1, ho, wo, 2), 6)
    y = T.conv64(x, w, 4, 2, 2, False, (ho, wo))
    dx = T.conv64(gy, w, 4, 2, 2, True, (7, 6))
    for oy, ox, c in ((0, 0, 1), (2, 3, 0), (ho - 1, wo - 1, 1)):
        acc = 0.0
        for ky in range(4):
            for kx in range(4):
                iy, ix = oy * 2 - 2 + ky, ox * 2 - 2 + kx
                if 0 <= iy < 7 and 0 <= ix < 6:
                    acc += float((x[0, iy, ix] * w[c, :, ky, kx]).sum())
        assert abs(acc - float(y[0, oy, ox, c])) < 1e-12
    for iy, ix, c in ((0, 0, 0), (3, 2, 2), (6, 5, 1)):
        acc = 0.0
        for ky in range(4):
            for kx in range(4):
                ty, tx = iy + 2 - ky, ix + 2 - kx                     # the kernel's transposed gather
                if ty >= 0 and tx >= 0 and ty % 2 == 0 and tx % 2 == 0 and ty // 2 < ho and tx // 2 < wo:
                    acc += float((gy[0, ty // 2, tx // 2] * w[:, c, ky, kx]).sum())
        assert abs(acc - float(dx[0, iy, ix, c])) < 1e-12


EPILOGUES = [T.Ep(bias=b, res=r, out_act=a, aux=m) for b in (False, True) for r in (False, True)
             for a in (T.ACT_NONE, T.ACT_LRELU, T.ACT_TANH) for m in (T.AUX_NONE, T.AUX_RELU_MASK, T.AUX_LRELU_GRAD)]


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
@pytest.mark.parametrize('g', [T.Geo(2, 7, 9, 8, 5, 3, 2, 1, False), T.Geo(2, 7, 9, 8, 5, 4, 2, 2, True)], ids=['fwd', 'dgrad'])
def test_epilogues_and_the_twin_dominates(g, dtype):
    x, w, bias, res, aux = T.operands(g, dtype, 11)
    assert int((aux == 0).sum()) > 0 and int((aux > 0).sum()) > 0 and int((aux < 0).sum()) > 0
    conv, a0 = T.conv_pair(x, w, g, T.ACT_NONE, dtype)
    wq = w.to(dtype).double()
    hw = (g.H, g.W) if g.dgrad else T.out_hw(g)
    assert torch.equal(conv, T.conv64(x.double(), wq, g.k, g.s, g.p, g.dgrad, hw))
    for ep in EPILOGUES:
        ref, A = T.epilogue64(conv, a0, bias, res, aux, ep)
        v = conv + (bias.double() if ep.bias else 0.0) + (res.double() if ep.res else 0.0)
        v = F.leaky_relu(v, 0.2) if ep.out_act == T.ACT_LRELU else (torch.tanh(v) if ep.out_act == T.ACT_TANH else v)
        if ep.aux != T.AUX_NONE:
            v = v * torch.where(aux.double() > 0, 1.0, 0.0 if ep.aux == T.AUX_RELU_MASK else 0.2)
        assert torch.allclose(ref, v, rtol=1e-13, atol=1e-13), ep
        assert bool((A >= ref.abs() - 1e-12).all()), ep
        assert bool((A >= 0).all()) and bool(torch.isfinite(A).all())
    # the reference() wrapper is the same thing
    ref, A = T.reference(x, w, bias, res, aux, g, EPILOGUES[-1], dtype)
    r2, a2 = T.epilogue64(conv, a0, bias, res, aux, EPILOGUES[-1])
    assert torch.equal(ref, r2) and torch.equal(A, a2)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_input_activation_operand_is_rounded_back(dtype):
    x = torch.tensor([1.0, -1.0, -3.0, 0.0, -0.3359375, 2.5]).to(dtype)
    got = T.operand64(x, T.ACT_LRELU, dtype)
    want = [1.0, float(torch.tensor(-0.2, dtype=torch.float32).to(dtype)),
            float((torch.tensor(-3.0, dtype=torch.float32) * torch.tensor(0.2, dtype=torch.float32)).to(dtype)), 0.0,
            float((torch.tensor(-0.3359375, dtype=torch.float32) * torch.tensor(0.2, dtype=torch.float32)).to(dtype)), 2.5]
    assert got.tolist() == want
    if dtype == torch.bfloat16:
        assert got[1].item() != -0.2 and abs(got[1].item() + 0.2) < 2.0 ** -9 * 0.2 * 2      # a bf16 value, not the fp64 product
    assert torch.equal(T.operand64(x, T.ACT_NONE, dtype), x.double())


def _all_cases():
    for route in ('stream', 'defaults', 'igemm'):
        for name, cases in T.groups_of(route).items():
            dt = T.S2E_F32 if name.endswith('_f32') else T.S2E_BF16
            for g, eps in cases:
                for ep in eps:
                    yield route, name, dt, g, ep


def test_every_case_is_inside_the_bound_derivation_and_its_kernel_takes_it():
    n = 0
    for route, name, dt, g, ep in _all_cases():
        assert T.k_of(g) <= T.K_MAX, (name, g)
        assert g.k in (1, 3, 4) and g.s in (1, 2)
        pl = T.plan_of(route, T.desc_fields(g, ep), dt, 256, True, True)
        assert pl is not None, (route, name, g, ep)
        n += 1
    assert n > 100


def test_coverage_counters_at_256_cus():
    sc, ic = T.coverage(256)
    assert sorted(sc) == sorted(T.STREAM_COUNTERS) and sorted(ic) == sorted(T.IGEMM_COUNTERS)
    assert [k for k, v in sc.items() if v == 0] == []
    assert [k for k, v in ic.items() if v == 0] == []


def test_stream_mirror_on_shapes_worked_out_by_hand():
    ep = T.Ep()
    pl = T.stream_plan(T.desc_fields(T.Geo(1, 8, 8, 64, 40, 3, 1, 1, False), ep), 256)
    assert (pl['units'], pl['G'], pl['rq'], pl['rr'], pl['whole_tiles'], pl['workspace']) == (9, 9, 1, 0, False, 2 * 9 * 128 * 64 * 4)
    c = T.stream_counters(pl)
    assert c['tiles_cut_3plus'] == 1 and c['ranges_inside_one_tile'] == 9 and c['G_eq_units'] == 1 and c['launches_with_fixup'] == 1
    pl = T.stream_plan(T.desc_fields(T.Geo(4, 260, 259, 8, 64, 1, 1, 0, False), ep), 256)
    assert (pl['tiles'], pl['G'], pl['rq'], pl['rr'], pl['whole_tiles'], pl['workspace']) == (2105, 256, 8, 57, True, 0)
    assert T.stream_counters(pl)['tiles_cut_0'] == 2105
    pl = T.stream_plan(T.desc_fields(T.Geo(3, 33, 31, 72, 136, 3, 2, 1, True), ep), 256)
    assert pl['cls_nk'] == [3, 5, 5, 9] and pl['G'] == pl['units']
    pl = T.stream_plan(T.desc_fields(T.Geo(1, 10, 12, 8, 40, 1, 1, 0, False), ep), 256)
    assert (pl['units'], pl['G'], pl['fixup']) == (1, 1, False)
    # three K-steps per tile, ranges of five or six: a range [5, 10) is the tail of tile 1, tile 2 and the head of tile 3
    pl = T.stream_plan(T.desc_fields(T.Geo(2, 161, 179, 16, 40, 3, 1, 1, False), ep), 256)
    assert (pl['units'], pl['rq'], pl['rr']) == (1353, 5, 73) and T.stream_counters(pl)['ranges_head_whole_tail'] > 0
    # what the kernel declines
    assert T.stream_plan(T.desc_fields(T.Geo(1, 8, 8, 64, 32, 3, 1, 1, False), ep), 256) is None
    assert T.stream_plan(T.desc_fields(T.Geo(1, 8, 8, 5, 40, 3, 1, 1, False), ep), 256) is None
    assert T.stream_plan(T.desc_fields(T.Geo(1, 8, 8, 64, 40, 3, 1, 1, False), T.Ep(out_act=T.ACT_TANH)), 256) is None
    assert T.stream_plan(T.desc_fields(T.Geo(1, 8, 8, 64, 40, 3, 1, 1, False), ep), 256, mode=1) is None


def test_igemm_mirror_on_shapes_worked_out_by_hand():
    ep = T.Ep()
    pl = T.igemm_plan(T.desc_fields(T.Geo(2, 16, 16, 264, 136, 3, 1, 1, False), ep), T.S2E_BF16, True, True)
    assert (pl['tiles'], pl['nk'], pl['splits'], pl['kt_per_split']) == (8, 38, 8, 5) and pl['workspace'] == 8 * 512 * 136 * 4
    assert T.igemm_counters(pl)['split_short_last'] == 1
    pl = T.igemm_plan(T.desc_fields(T.Geo(2, 17, 17, 256, 512, 4, 1, 2, False), ep), T.S2E_BF16, True, True)
    assert (pl['splits'], pl['kt_per_split']) == (16, 4) and T.igemm_counters(pl)['split_full_last'] == 1
    f = T.desc_fields(T.Geo(3, 33, 31, 72, 136, 3, 2, 1, True), ep)
    assert T.igemm_plan(f, T.S2E_BF16, True, True)['s2_class'] and T.igemm_plan(f, T.S2E_BF16, True, True)['splits'] == 1
    assert not T.igemm_plan(f, T.S2E_BF16, False, True)['s2_class'] and not T.igemm_plan(f, T.S2E_BF16, True, False)['s2_class']
    assert T.igemm_plan(f, T.S2E_BF16, True, False)['loader'] == 'register'
    assert T.igemm_plan(T.desc_fields(T.Geo(2, 19, 23, 5, 24, 3, 1, 1, False), ep), T.S2E_BF16, True, True)['loader'] == 'gather'
    assert T.igemm_plan(T.desc_fields(T.Geo(2, 16, 16, 264, 136, 3, 1, 1, False), T.Ep(in_act=T.ACT_LRELU)), T.S2E_F32, True, True)['loader'] == 'register'


def _plan_envs():
    """(id, environment, groups): the children of tests/test_conv_generic_fp64_gpu.py, merged into one process per environment"""
    out = []
    for cid, env, groups in G._CHILDREN:
        hit = [o for o in out if o[1] == env]
        if hit:
            hit[0][2].extend(groups.split(','))
        else:
            out.append((' '.join('%s=%s' % kv for kv in sorted(env.items())) or 'defaults', env, groups.split(',')))
    return out


_PLAN_ENVS = _plan_envs()


def test_gpu_children_run_every_group_in_the_environment_it_is_written_for():
    ran = {}
    for _, env, groups in _PLAN_ENVS:
        route = T.route_of_env(env)
        assert env.get('S2E_CONV_PATCH', '0') == '0' and env.get('S2E_CONV_DUO', '0') == '0'
        assert (route == 'defaults') == (env == {})
        for name in groups:
            assert name in T.groups_of(route), (name, route)
            ran.setdefault(route, set()).add(name)
    masked = [g for _, env, g in _PLAN_ENVS if env.get('S2E_IGEMM_S2CLASS') == '0']
    no_dma = [g for _, env, g in _PLAN_ENVS if env.get('S2E_IGEMM_GLDS') == '0']
    assert masked == [['subset', 'subset_f32']] and no_dma == [['subset', 'subset_f32']]
    assert ran == {r: set(T.groups_of(r)) for r in ('stream', 'defaults', 'igemm')}


@pytest.fixture(scope='module')
def built():
    import __graft_entry__
    __graft_entry__.build()


@pytest.mark.parametrize('env,groups', [c[1:] for c in _PLAN_ENVS], ids=[c[0] for c in _PLAN_ENVS])
def test_library_routes_and_workspace_match_the_mirrors(built, env, groups):
    """s2e_conv2d_kernel_kind and s2e_conv2d_workspace_bytes of the tree's library, for every case, in the environment its GPU child
    runs in: GENERIC, and the bytes the mirror of the kernel the case is written for says"""
    e = {k: v for k, v in os.environ.items() if k not in T.SWITCHES}
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_conv_generic_child.py'), '--plan', '--groups', ','.join(groups)],
                       env=e, capture_output=True, text=True, timeout=600, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0 and 'conv generic plan ok:' in r.stdout, (r.stdout[-4000:], r.stderr[-4000:])


@pytest.fixture(scope='module')
def longest():
    """the largest-K bf16 case of the shipped lists, with its reference"""
    route, name, dt, g, ep = max((c for c in _all_cases() if c[2] == T.S2E_BF16), key=lambda c: T.k_of(c[3]))
    assert T.k_of(g) == 4096 and not g.dgrad
    x, w, bias, res, aux = T.operands(g, torch.bfloat16, 5)
    conv, a0 = T.conv_pair(x, w, g, T.ACT_NONE, torch.bfloat16)
    return g, x, w, bias, res, aux, conv, a0


def test_bound_catches_a_lost_k_step(longest):
    """one 128 x 128 tile that lost one 64-wide K-step of K = 4096 -- what a wrong range boundary or a slot read twice does"""
    g, x, w, bias, res, aux, conv, a0 = longest
    ep = T.Ep(bias=True)
    ref, A = T.epilogue64(conv, a0, bias, res, aux, ep)
    good = ref.to(torch.bfloat16)                                         # a correctly rounded result passes
    assert T.check_close(good, ref, A, 'rounded reference') <= 1.0
    kt = 37                                                               # K-step 37: k in [2368, 2432) = tap 9 (ky 2, kx 1), ci 64 .. 127
    tap, ci0 = divmod(kt * 64, g.cin)
    ky, kx = divmod(tap, g.k)
    w1 = torch.zeros_like(w)
    w1[:, ci0:ci0 + 64, ky, kx] = w[:, ci0:ci0 + 64, ky, kx]
    step = T.conv64(x.double(), T.weight64(w1, torch.bfloat16), g.k, g.s, g.p, False, T.out_hw(g))
    lost = ref.clone().view(-1, g.cout)
    lost[128:256, 128:256] -= step.view(-1, g.cout)[128:256, 128:256]     # pixel tile 1, channel tile 1
    lost = lost.view_as(ref)
    assert int((lost != ref).sum()) > 128 * 128 // 2 and int((lost != ref).sum()) <= 128 * 128
    with pytest.raises(AssertionError, match='outside the bound'):
        T.check_close(lost.to(torch.bfloat16), ref, A, 'lost K-step')


def test_bound_catches_the_wrong_mask_constant_and_a_nan(longest):
    g, x, w, bias, res, aux, conv, a0 = longest
    ref, A = T.epilogue64(conv, a0, bias, res, aux, T.Ep(bias=True, aux=T.AUX_RELU_MASK))
    wrong, _ = T.epilogue64(conv, a0, bias, res, aux, T.Ep(bias=True, aux=T.AUX_LRELU_GRAD))
    T.check_close(ref.to(torch.bfloat16), ref, A, 'rounded reference')
    with pytest.raises(AssertionError, match='outside the bound'):
        T.check_close(wrong.to(torch.bfloat16), ref, A, '0.2 where 0 belongs')
    got = ref.to(torch.bfloat16)
    got[1, 3, 5, 77] = float('nan')
    with pytest.raises(AssertionError, match='outside the bound'):
        T.check_close(got, ref, A, 'a NaN from the workspace')
