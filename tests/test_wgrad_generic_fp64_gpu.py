"""The generic weight-gradient kernel -- csrc/conv_wgrad.hip: conv_wgrad_kernel in bf16 and fp32, with the vector and the scalar
gather, its fixed-order reduction, the atomic fall-back, and the multi-job forms -- against fp64 references of the same operands,
element by element, through s2e_conv2d_wgrad and s2e_conv2d_wgrad_multi (tests/_wgrad_generic_child.py has the references, the
bound and its derivation, the plan mirror, the case lists and the coverage counters).

One child process per environment, because the library reads its switches once per process: the shipped thresholds (atomics below 16
pixel splits, partial tiles and the reduce from 16 on), S2E_WGRAD_PARTIAL=2 (every split launch reduces), S2E_WGRAD_PARTIAL=0 (atomics
only), S2E_DETERMINISTIC=1 (every launch reduces, the unsplit ones too; and one multi-job call whose jobs all take the generic route).
Each child prints per case the route, the splits, the workspace form and the worst error / bound, and ends with 'wgrad generic ok:'."""
import os
import subprocess
import sys

import pytest

import _wgrad_generic_child as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (id, environment, groups)
_CHILDREN = [(name, T.ENVS[name], ','.join(T.ENV_GROUPS[name])) for name in ('default', 'partial2', 'partial0', 'det')]


@pytest.mark.parametrize('env,groups', [c[1:] for c in _CHILDREN], ids=[c[0] for c in _CHILDREN])
def test_wgrad_generic_against_fp64(env, groups):
    e = dict(os.environ)
    for k in T.SWITCHES:
        e.pop(k, None)
    e.update(env)
    cmd = [sys.executable, os.path.join(ROOT, 'tests', '_wgrad_generic_child.py'), '--groups', groups]
    r = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=600, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0 and 'wgrad generic ok:' in r.stdout, (r.stdout[-4000:], r.stderr[-4000:])
