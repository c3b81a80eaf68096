"""The conv dispatch answers every per-shape query as the commit before the one-router refactor did (no GPU).

tests/golden/make_conv_routing.py sweeps ~1.4 M descriptors (two dtypes, three batch sizes, 17 maps, 13 x 13 channel counts,
eight (k, stride, pad), both directions, five activation / mask combinations) through the ten routing queries, in six
environments (defaults, S2E_CONV_DUO=0, S2E_CONV_PATCH=0, S2E_CONV_STREAM=2, S2E_CONV_PLANE=0, S2E_DETERMINISTIC=1), each in a
child process with every other S2E_* variable removed.  tests/golden/conv_routing.json holds, per slice, the digests and column
statistics of that sweep run on a build of the PARENT commit's library; this test runs it on the tree's own library.

The workspace columns depend on the CU count the library plans with.  The fixture is valid for 256 -- what the library assumes
without a device, and what an MI355X has; on anything else those columns are not compared (the rest still is).
"""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN


def _generator():
    spec = importlib.util.spec_from_file_location('make_conv_routing', os.path.join(GOLDEN, 'make_conv_routing.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def sweeps():
    import __graft_entry__
    __graft_entry__.build()
    from seg2eye_amd import build
    return _generator().run_all(build.LIB)


def test_grid_is_as_varied_as_the_fixture_says():
    """The recorded grid itself: every public kernel family in both directions, the five plane modes, 14 slot counts, and at least
    the 1335 forward / 788 weight-gradient workspace sizes of the first trial of this sweep."""
    gen = _generator()
    want = json.load(open(os.path.join(GOLDEN, 'conv_routing.json')))
    assert tuple(want['queries']) == gen.QUERIES and sorted(want['envs']) == sorted(gen.ENVS)
    col = {q: i for i, q in enumerate(gen.QUERIES)}
    d = want['envs']['default']['distinct']
    assert d[col['s2e_conv2d_kernel_kind']] == 3 and d[col['s2e_conv2d_wgrad_kernel_kind']] == 3
    assert d[col['s2e_conv2d_plane_supported']] == 6                               # 0 and the five modes
    assert d[col['s2e_conv2d_stats_slots']] >= 14 and d[col['s2e_conv2d_rects_supported']] == 2
    assert d[col['s2e_conv2d_workspace_bytes']] >= 1335 and d[col['s2e_conv2d_wgrad_workspace_bytes']] >= 788
    assert d[col['s2e_conv2d_wgrad_rects_workspace_bytes']] >= 2 and d[col['s2e_conv2d_wgrad_multi_kind']] >= 5
    assert d[col['s2e_conv2d_wgrad_multi_supported']] == 2
    for env in want['envs'].values():
        assert env['cus'] == 256 and len(env['slices']) == 2 * len(gen.KSP) * 2 and sum(s['n'] for s in env['slices'].values()) > 1300000


@pytest.mark.parametrize('env', ['default', 'duo0', 'patch0', 'stream2', 'plane0', 'deterministic'])
def test_every_query_answers_as_the_parent_did(sweeps, env):
    want = json.load(open(os.path.join(GOLDEN, 'conv_routing.json')))['envs'][env]
    got = sweeps[env]
    # a shape that takes a rectangle list (the duo kernel) needs no forward workspace
    assert got['rects_with_workspace'] == 0
    same_cus = got['cus'] == want['cus']
    if not same_cus:
        print('the library plans with %g CUs, the fixture was recorded with %g: workspace columns not compared' % (got['cus'], want['cus']))
    ws = set(_generator().WS_COLS)
    assert sorted(got['slices']) == sorted(want['slices'])
    for name, w in want['slices'].items():
        g = got['slices'][name]
        keep = [c for c in range(len(w['distinct'])) if same_cus or c not in ws]
        # (the statistics first: they say WHICH column moved, the digest only that one did)
        assert g['n'] == w['n'], name
        assert [g['distinct'][c] for c in keep] == [w['distinct'][c] for c in keep], name
        assert [g['nonzero'][c] for c in keep] == [w['nonzero'][c] for c in keep], name
        assert g['sha'] == w['sha'], name
        if same_cus:
            assert g['sha_ws'] == w['sha_ws'], name
