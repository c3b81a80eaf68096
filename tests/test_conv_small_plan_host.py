"""The plan mirrors of tests/_conv_small_child.py (csrc/conv_small.hip), without a GPU: every coverage counter is non-zero over the
shipped case lists, three cases' band / rectangle / grid / workspace numbers against values worked out by hand, the library's kind and
workspace queries against the mirrors for every shipped case, and the weight gradients' error constant c_w against a numpy fp32
emulation of the kernels' summation order."""
import os
import subprocess
import sys

import pytest

import _conv_small_child as S
from _conv_generic_child import S2E_BF16, S2E_F32, Ep, Geo, desc_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('det', [False, True], ids=['defaults', 'deterministic'])
def test_no_counter_is_zero_over_the_shipped_lists(det):
    tot = S.coverage(det)
    zero = S.zero_counters(tot)
    if det:                                                # one slab always: the slab counters belong to the default environment
        zero = [z for z in zero if z not in ('wgrad.slabs_2_7', 'wgrad.slabs_8', 'wgrad.unrolled_loop_not_entered')
                and not z.startswith('wgrad.nb_')]
    assert not zero, zero


def test_every_case_runs_in_the_kernel_its_group_is_written_for():
    for name, cases in S.FWD_GROUPS.items():
        for g, eps in cases:
            for ep in eps:
                pl = S.fwd_plan(desc_fields(g, ep), S.group_dt(name))
                assert pl is not None and pl['kernel'] in S.GROUP_KERNELS[name], (name, g, ep)
                assert pl['rounded_in_act'] == (pl['kernel'] in ('fwd_cout1_mfma', 'tap_gemm_fwd', 'tap_gemm_dgrad'))
    for name, cases in S.WGRAD_GROUPS.items():
        for g, in_act in cases:
            pl = S.wgrad_plan(S.wgrad_fields(g, in_act), S.group_dt(name), False)
            assert pl is not None and pl['kernel'] in S.GROUP_KERNELS[name], (name, g)
            assert pl['lds'] <= 64 * 1024 and pl['workspace'] <= S.SMALL_WS_CAP


def test_lds_cap_of_the_dot_then_stencil_rectangles():
    """48 KB of [wk][PP][KS*KS | 1] floats: all eight candidates at wk = 1 with 3x3, 16 and below with 4x4; wk = 4 loses 24 and 32
    (and 12, 16 with 4x4)"""
    assert S.cout1_mfma_allowed(3, 1) == (32, 24, 16, 12, 9, 8, 7, 6)
    assert S.cout1_mfma_allowed(4, 1) == (16, 12, 9, 8, 7, 6)
    assert S.cout1_mfma_allowed(3, 4) == (16, 12, 9, 8, 7, 6)
    assert S.cout1_mfma_allowed(4, 4) == (9, 8, 7, 6)
    for ks in (3, 4):
        assert 24 not in S.cout1_mfma_allowed(ks, 4) and 32 not in S.cout1_mfma_allowed(ks, 4)


def test_three_cases_by_hand():
    # 1. bf16 forward 1 -> 8 on 8 x 129 x 12: 1032 rows over 1024 items -> 2 rows a band, 65 bands (the last has 1 row), one 12-column
    #    segment: 8 * 65 = 520 items, one workgroup each; LDS row stride 11 + 3 = 14; patches of 4 x 14 and 3 x 14 elements
    pl = S.fwd_plan(desc_fields(Geo(8, 129, 12, 1, 8, 3, 1, 1, False), Ep()), S2E_BF16)
    bd = pl['band']
    assert pl['kernel'] == 'fwd_cin1' and (pl['G'], pl['ppb']) == (1, 256)
    assert (bd['rows'], bd['bands'], bd['last_rows'], bd['segw'], bd['segs'], bd['items'], bd['pc']) == (2, 65, 1, 12, 1, 520, 14)
    assert pl['grid'] == 520 and S.band_item_shapes(bd) == [(1, 12), (2, 12)]
    assert [S.band_patch_elems(bd, *s) for s in S.band_item_shapes(bd)] == [42, 56]
    # 2. bf16 forward 64 -> 1 3x3 on 16 x 96 x 96: 32 gives 16 * 9 = 144 tiles, 24 gives 16 * 16 = 256 -> rectangle 24, one slab,
    #    4 K-steps a wave, patch 26 x 26 = 676 pixels = 22 row blocks (the last has 4), 676 * 9 * 4 bytes of LDS
    pl = S.fwd_plan(desc_fields(Geo(16, 96, 96, 64, 1, 3, 1, 1, False), Ep(bias=True)), S2E_BF16)
    assert (pl['kernel'], pl['t'], pl['wk'], pl['nkw'], pl['grid'], pl['PP'], pl['lds']) == ('fwd_cout1_mfma', 24, 1, 4, 256, 676, 24336)
    #    and in fp32 the same shape runs in the vector kernel: G = 16 lanes a pixel, 16 pixels a block, 147456 / 16 = 9216 blocks -> 4096
    pl = S.fwd_plan(desc_fields(Geo(16, 96, 96, 64, 1, 3, 1, 1, False), Ep(bias=True)), S2E_F32)
    assert (pl['kernel'], pl['G'], pl['ppb'], pl['grid'], pl['capped']) == ('fwd_cout1', 16, 16, 4096, True)
    # 3. bf16 weight gradient 512 -> 1 4x4 pad 2 on 8 x 225 x 4: 32 KB a partial row -> 256 blocks at most; 1800 rows -> 8 rows a band,
    #    29 bands (the last has 1 row), 232 items = 232 blocks, 232 * 8192 * 4 bytes of workspace, 232 / 32 = 7 slabs (1 when
    #    deterministic); a slot's chain: 32 pixels over 4 slots = 8, D = 8 + 2 + 0 + 3 + ceil(232 / 112) + 3 + 4 + 14 = 37
    f = S.wgrad_fields(Geo(8, 225, 4, 512, 1, 4, 1, 2, False), 0)
    pl = S.wgrad_plan(f, S2E_BF16, False)
    bd = pl['band']
    assert (pl['kernel'], pl['gmax'], pl['ws_capped'], pl['G'], pl['ppb'], pl['nout']) == ('wgrad_cout1', 256, True, 64, 4, 8192)
    assert (bd['rows'], bd['bands'], bd['last_rows'], bd['items'], bd['flip'], bd['org'], bd['pc']) == (8, 29, 1, 232, 1, -1, 7)
    assert (pl['grid'], pl['workspace'], pl['slabs'], pl['depth']) == (232, 232 * 8192 * 4, 7, 37)
    assert S.wgrad_plan(f, S2E_BF16, True)['slabs'] == 1
    #    fp32 1 -> 4 3x3: 36 outputs a row, 1024 blocks at most
    pl = S.wgrad_plan(S.wgrad_fields(Geo(2, 17, 13, 1, 4, 3, 2, 1, False), 1), S2E_F32, False)
    assert (pl['kernel'], pl['nout'], pl['gmax'], pl['grid'], pl['workspace'], pl['slabs']) == ('wgrad_cin1', 36, 1024, 18, 18 * 144, 1)


def test_negative_routes_are_not_small_in_the_mirror():
    for what, query, dt, f in S.NEGATIVE:
        assert (S.small_conv_kind(f, dt) if query == 'fwd' else S.small_wgrad_kind(f, dt)) == S.SMALL_NONE, what


def test_pixel_counts_keep_a_dropped_term_outside_the_bound():
    for name, cases in S.WGRAD_GROUPS.items():
        for g, in_act in cases:
            for det in (False, True):
                pl = S.wgrad_plan(S.wgrad_fields(g, in_act), S.group_dt(name), det)
                ho, wo = S.out_hw(g)
                assert g.N * ho * wo * (2.0 ** -22 + pl['c_w']) <= 0.5, (name, g, det)


@pytest.mark.parametrize('group,index', S.EMULATED)
def test_fp32_emulation_of_the_summation_order_stays_inside_c_w(group, index):
    """the kernels' order of additions redone in numpy fp32 (linear worst-case bound: the ratio is far below 1)"""
    ratio = S.emulated_ratio(group, index)
    print('emulated %s[%d]: worst error / bound %.4f' % (group, index, ratio))
    assert 0 < ratio <= 1


@pytest.mark.parametrize('env', [{}, {'S2E_DETERMINISTIC': '1'}], ids=['defaults', 'deterministic'])
def test_library_queries_agree_with_the_mirrors(env):
    """s2e_conv2d_kernel_kind, s2e_conv2d_wgrad_kernel_kind and the workspace queries for every shipped case and negative route, on
    the library alone (it plans without a device)"""
    import __graft_entry__
    __graft_entry__.build()
    e = dict(os.environ)
    for k in S.SWITCHES:
        e.pop(k, None)
    e.update(env)
    groups = ','.join(list(S.FWD_GROUPS) + list(S.WGRAD_GROUPS))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_conv_small_child.py'), '--groups', groups, '--plan'], env=e,
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0 and 'conv small plan ok:' in r.stdout, (r.stdout[-4000:], r.stderr[-4000:])
