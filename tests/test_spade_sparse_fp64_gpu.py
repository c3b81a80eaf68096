"""The small kernels of the label-sparse SPADE path -- s2e_label_rect_classify, s2e_spade_class_table[_batch], s2e_spade_modulate_uniform
(csrc/label_ops.hip), s2e_label_rect_lists_bwd, s2e_spade_uniform_sums, s2e_spade_uniform_grads (csrc/spade_sparse_bwd.hip) -- called
directly at the C ABI and compared element by element: the integer outputs for equality with a numpy restatement of the header's rule,
the floating-point ones with fp64 references of the same operands (tests/_spade_sparse_ref.py has the references, the bounds and their
derivation; tests/_spade_sparse_child.py the GPU side and the guards; tests/test_spade_sparse_ref_host.py proves on the CPU that the
references are autograd's and that the bounds catch a skipped halo corner, a wrong table row, a swapped tap, a wrong replica tap).

One child process per (group set, dtype), with every S2E_* switch removed from its environment.  Each child prints one line per case with
its largest err / bound; the threshold is 1."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (id, groups, dtype): 'none' for the groups whose operands have one type only (integers; s2e_spade_uniform_grads is fp32 throughout)
_CHILDREN = [
    ('classify-lists_bwd', 'classify,lists_bwd', 'none'),
    ('table-bf16', 'table', 'bf16'), ('table-fp32', 'table', 'fp32'),
    ('modulate-bf16', 'modulate', 'bf16'), ('modulate-fp32', 'modulate', 'fp32'),
    ('sums-bf16', 'sums', 'bf16'), ('sums-fp32', 'sums', 'fp32'),
    ('grads', 'grads', 'none'),
    ('chain-bf16', 'chain', 'bf16'),
]


@pytest.mark.parametrize('groups,dtype', [c[1:] for c in _CHILDREN], ids=[c[0] for c in _CHILDREN])
def test_spade_sparse_against_fp64(groups, dtype):
    e = {k: v for k, v in os.environ.items() if not k.startswith('S2E_')}
    cmd = [sys.executable, os.path.join(ROOT, 'tests', '_spade_sparse_child.py'), '--groups', groups, '--dtype', dtype]
    r = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=600, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0 and 'spade sparse ok:' in r.stdout, (r.stdout[-4000:], r.stderr[-4000:])
