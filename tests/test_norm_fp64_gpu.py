"""The norm / modulation kernels of csrc/norm_modulate.hip -- s2e_in_stats, s2e_in_stats_from_partials, s2e_instance_norm_fwd / _bwd,
s2e_modulate_fwd, every form of s2e_modulate_bwd, s2e_colsum -- against fp64 references of the same operands, element by element, at the
C ABI (tests/_norm_ref.py has the references, the bounds and their derivation; tests/_norm_child.py the GPU side and the guards;
tests/test_norm_ref_host.py proves on the CPU that the references are autograd's and that the bounds catch a dropped row).

Every case runs in a child process, because the library reads S2E_IN_SMALL_HW once per process: the defaults (one-launch kernels up to
1280 pixels), 0 (every map, however small, on the row-walking kernels) and 100000 (the one-launch kernels with many trips per thread).
Each child prints the kernel every case ran in and its largest err / bound per output; the threshold is 1."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEFAULTS, ROWWALK, ONE_LAUNCH = {}, {'S2E_IN_SMALL_HW': '0'}, {'S2E_IN_SMALL_HW': '100000'}

# (id, environment, groups)
_CHILDREN = [
    ('defaults-small', DEFAULTS, 'small'),
    ('defaults-boundary-zblocks-partials-colsum', DEFAULTS, 'boundary,zblocks,partials,colsum'),
    ('defaults-forms-edge', DEFAULTS, 'forms_small,edge'),
    ('rowwalk', ROWWALK, 'rowwalk'),
    ('rowwalk-forms', ROWWALK, 'forms'),
    ('rowwalk-edge', ROWWALK, 'edge'),
    ('one-launch-4100', ONE_LAUNCH, 'long'),
    ('grid-wrap', DEFAULTS, 'wrap'),
]


@pytest.mark.parametrize('dtype', ['bf16', 'fp32'])
@pytest.mark.parametrize('env,groups', [c[1:] for c in _CHILDREN], ids=[c[0] for c in _CHILDREN])
def test_norm_against_fp64(env, groups, dtype):
    e = {k: v for k, v in os.environ.items() if not k.startswith('S2E_')}
    e.update(env)
    cmd = [sys.executable, os.path.join(ROOT, 'tests', '_norm_child.py'), '--groups', groups, '--dtype', dtype]
    r = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=600, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0 and 'norm ok:' in r.stdout, (r.stdout[-4000:], r.stderr[-4000:])
