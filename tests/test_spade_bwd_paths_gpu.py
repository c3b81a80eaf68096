"""The path one SPADE+Style layer's backward takes, case by case, against what the commit before the backward's plan
(ops.spade._plan_spade_bwd) took: tests/golden/make_spade_bwd_paths.py runs each case through the public ops with a LaunchProfiler
installed and counts the launches per family of the forward, of the backward before the flush and of the flush, the lengths of the
sink's queues before the flush and how many of the queued jobs carry a rectangle list; tests/golden/spade_bwd_paths.json holds what
that script gave on the parent commit.  A case the parent refused must be refused with the same exception class.  Gradient values
are not compared here: the label-sparse path adds with float atomics, and test_spade_label_sparse_backward holds them to fp64."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _maker():
    spec = importlib.util.spec_from_file_location('make_spade_bwd_paths', os.path.join(GOLDEN, 'make_spade_bwd_paths.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


M = _maker()
FIXTURE = json.load(open(os.path.join(GOLDEN, 'spade_bwd_paths.json')))


def test_fixture_covers_the_cases_and_every_arm():
    assert list(FIXTURE) == list(M.CASES)
    done = [v for v in FIXTURE.values() if 'raises' not in v]
    # both backwards, a c8 job with and without a rectangle list (lazy d(actv) or zero-filled), the [gamma | beta] weight gradient
    # queued with a list, queued dense, launched at once, and through the re-layout queue (torch-order arena)
    assert any(v['backward'].get('spade_uniform_bwd') for v in done) and any(not v['backward'].get('spade_uniform_bwd') for v in done)
    scoped = [v for v in done if v['queues'] is not None]
    assert any(v['with_rects']['c8'] for v in scoped) and any(v['queues']['uni'] and not v['with_rects']['c8'] for v in scoped)
    assert any(v['with_rects']['wg'] for v in scoped) and any(v['queues']['wg'] and not v['with_rects']['wg'] for v in scoped)
    assert any(v['queues']['uni'] and not v['queues']['wg'] for v in scoped) and any(v['queues']['jobs'] for v in scoped)


@pytest.mark.parametrize('name', list(M.CASES))
def test_backward_takes_the_parents_path(name):
    want, got = FIXTURE[name], M.run_case(name)
    print(name, json.dumps(got, sort_keys=True))
    if 'raises' in want:
        assert got.get('raises') == want['raises'], got
    else:
        assert got == want
