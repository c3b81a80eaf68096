"""The bf16 3x3 stride-1 convolution family -- csrc/conv_duo.hip, csrc/conv_patch.hip on the same shapes, csrc/conv_wgrad_patch.hip --
against fp64 references of the same bf16 operands, element by element (tests/_conv3x3_child.py has the references and the bound).

Every case runs in a child process with the switches the library reads once per process: the duo kernel on small shapes
(S2E_CONV_DUO=1, S2E_SPADE_FUSED_TILES=1: no S2E_SPADE_ANY_TILES, which would route the fused launch past it), conv_patch.hip on the same shapes
(S2E_CONV_DUO=0, S2E_CONV_PATCH=1), the 32x32x16 duo loop (S2E_DUO_MF16=0), the library's own thresholds at bench-like shapes, and the
patch weight gradient (S2E_WGRAD_PATCH=1, with and without S2E_DETERMINISTIC=1).  Each child prints the kernel every case ran in and its
work items relative to the duo kernel's persistent grid (cap = 2 x CUs)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ('S2E_CONV_DUO', 'S2E_CONV_PATCH', 'S2E_SPADE_FUSED_TILES', 'S2E_DUO_MF16', 'S2E_WGRAD_PATCH', 'S2E_DETERMINISTIC')

DUO = {'S2E_CONV_DUO': '1', 'S2E_SPADE_FUSED_TILES': '1'}
PATCH = {'S2E_CONV_DUO': '0', 'S2E_CONV_PATCH': '1', 'S2E_SPADE_FUSED_TILES': '1'}
MF32 = dict(DUO, S2E_DUO_MF16='0')
WGRAD = {'S2E_WGRAD_PATCH': '1'}
WGRAD_DET = {'S2E_WGRAD_PATCH': '1', 'S2E_DETERMINISTIC': '1'}

# (id, environment, group, --subset)
_CHILDREN = [
    ('duo-fwd', DUO, 'fwd', False), ('duo-dgrad', DUO, 'dgrad', False), ('duo-rects', DUO, 'rects', False),
    ('duo-fused', DUO, 'fused', False), ('duo-fused-lists', DUO, 'fused_lists', False), ('duo-cap', DUO, 'cap', False),
    ('patch-fwd', PATCH, 'fwd', False), ('patch-dgrad', PATCH, 'dgrad', False), ('patch-fused', PATCH, 'fused', False),
    ('patch-fused-lists', PATCH, 'fused_lists', False),
    ('mf16=0-fwd-dgrad', MF32, 'fwd,dgrad', True), ('mf16=0-fused', MF32, 'fused,fused_lists', True), ('mf16=0-cap', MF32, 'cap', True),
    ('defaults-bench', {}, 'bench', False),
    ('wgrad-patch', WGRAD, 'wgrad', False), ('wgrad-patch-rects', WGRAD, 'wgrad_rects', False),
    ('wgrad-patch-deterministic', WGRAD_DET, 'wgrad_det', False),
]


@pytest.mark.parametrize('env,groups,subset', [c[1:] for c in _CHILDREN], ids=[c[0] for c in _CHILDREN])
def test_conv3x3_against_fp64(env, groups, subset):
    e = dict(os.environ)
    for k in SWITCHES:
        e.pop(k, None)
    e.update(env)
    cmd = [sys.executable, os.path.join(ROOT, 'tests', '_conv3x3_child.py'), '--groups', groups] + (['--subset'] if subset else [])
    r = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=600, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0 and 'conv3x3 ok:' in r.stdout, (r.stdout[-4000:], r.stderr[-4000:])
