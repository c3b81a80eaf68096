"""The degenerate-channel convolutions of csrc/conv_small.hip (Cout == 1 and Cin == 1: forward, data gradient, weight gradient) against
fp64 references of the same operands, element by element and kernel by kernel (tests/_conv_small_child.py has the references, the
bounds with their derivation, the plan mirrors and the case lists).

One child process per environment, because the library reads S2E_DETERMINISTIC once per process: the bf16 groups and the fp32 groups
under the defaults, and the weight-gradient groups again under S2E_DETERMINISTIC=1 (one reduce slab: two launches must then agree bit
for bit).  Each child prints the kernel every case ran in, the worst error / bound per case and what the plan mirrors counted; no
counter over the shipped lists may be zero."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ('S2E_DETERMINISTIC', 'S2E_CONV_C8')
DET = {'S2E_DETERMINISTIC': '1'}

# (id, environment, groups)
_CHILDREN = [
    ('bf16-mfma-big', {}, 'mfma_a'), ('bf16-mfma', {}, 'mfma_b'), ('bf16-cout1-band', {}, 'cout1,band'), ('bf16-tap', {}, 'tap'),
    ('bf16-wgrad', {}, 'wgrad'),
    ('f32-fwd-dgrad', {}, 'cout1_f32,band_f32'), ('f32-wgrad', {}, 'wgrad_f32'),
    ('deterministic-wgrad', DET, 'wgrad,wgrad_f32'),
]


@pytest.mark.parametrize('env,groups', [c[1:] for c in _CHILDREN], ids=[c[0] for c in _CHILDREN])
def test_conv_small_against_fp64(env, groups):
    e = dict(os.environ)
    for k in SWITCHES:
        e.pop(k, None)
    e.update(env)
    cmd = [sys.executable, os.path.join(ROOT, 'tests', '_conv_small_child.py'), '--groups', groups]
    r = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=600, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0 and 'conv small ok:' in r.stdout, (r.stdout[-4000:], r.stderr[-4000:])
