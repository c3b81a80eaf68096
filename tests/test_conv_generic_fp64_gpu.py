"""The two generic convolution kernels -- csrc/conv_stream.hip (persistent stream-K and its fix-up launch) and csrc/conv_igemm.hip
(implicit GEMM, split-K with conv_finish_kernel, the stride-2 parity-class mode) -- against fp64 references of the same operands,
element by element (tests/_conv_generic_child.py has the references, the bound, the plan mirrors and the case lists).

Every group of cases runs in a child process with the switches the library reads once per process: stream-K on every shape it can
run (S2E_CONV_STREAM=2), the implicit GEMM on the same shapes and on the ones only it takes (S2E_CONV_STREAM=0) in bf16 and fp32,
both with the small-tile and patch kernels out of the way (S2E_CONV_PATCH=0, S2E_CONV_DUO=0); the masked all-taps walk of the stride-2
data gradient (S2E_IGEMM_S2CLASS=0) and the register-staged loader (S2E_IGEMM_GLDS=0) on a subset; and the library's own thresholds
on two shapes they send to stream-K.  Each child prints the kernel every case ran in, the worst error / bound per group and what the
plan mirrors counted (cut tiles, range shapes, split forms); on a 256-CU device no counter over the shipped lists may be zero."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ('S2E_CONV_STREAM', 'S2E_CONV_PATCH', 'S2E_CONV_DUO', 'S2E_IGEMM_GLDS', 'S2E_IGEMM_S2CLASS', 'S2E_DETERMINISTIC')

STREAM = {'S2E_CONV_STREAM': '2', 'S2E_CONV_PATCH': '0', 'S2E_CONV_DUO': '0'}
IGEMM = {'S2E_CONV_STREAM': '0', 'S2E_CONV_PATCH': '0', 'S2E_CONV_DUO': '0'}
MASKED = dict(IGEMM, S2E_IGEMM_S2CLASS='0')
NO_GLDS = dict(IGEMM, S2E_IGEMM_GLDS='0')

# (id, environment, groups)
_CHILDREN = [
    ('stream-fwd-small', STREAM, 'fwd_small'), ('stream-fwd-big', STREAM, 'fwd_big'), ('stream-dgrad', STREAM, 'dgrad'),
    ('defaults', {}, 'defaults'),
    ('igemm-fwd-small', IGEMM, 'fwd_small'), ('igemm-fwd-big', IGEMM, 'fwd_big'), ('igemm-dgrad', IGEMM, 'dgrad'),
    ('igemm-extra', IGEMM, 'extra,extra_f32'),
    ('igemm-f32-fwd-small', IGEMM, 'fwd_small_f32'), ('igemm-f32-fwd-big', IGEMM, 'fwd_big_f32'), ('igemm-f32-dgrad', IGEMM, 'dgrad_f32'),
    ('igemm-s2class=0', MASKED, 'subset,subset_f32'), ('igemm-glds=0', NO_GLDS, 'subset,subset_f32'),
]


@pytest.mark.parametrize('env,groups', [c[1:] for c in _CHILDREN], ids=[c[0] for c in _CHILDREN])
def test_conv_generic_against_fp64(env, groups):
    e = dict(os.environ)
    for k in SWITCHES:
        e.pop(k, None)
    e.update(env)
    cmd = [sys.executable, os.path.join(ROOT, 'tests', '_conv_generic_child.py'), '--groups', groups]
    r = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=600, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0 and 'conv generic ok:' in r.stdout, (r.stdout[-4000:], r.stderr[-4000:])
