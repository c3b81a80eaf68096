"""The label-map and resampling kernels of csrc/label_ops.hip -- s2e_label_conv3x3 (single and batched launch, both pixel walks),
s2e_onehot_nhwc, s2e_upsample2x_fwd / _bwd, s2e_avgpool3x3s2_fwd / _bwd, s2e_tanh_bwd, s2e_lrelu_bwd, s2e_bilinear_resize_fwd / _bwd --
against fp64 references of the same operands, element by element, at the C ABI (tests/_label_ops_ref.py has the references, the bounds
and their derivation; tests/_label_ops_child.py the GPU side, the guards and the cases; tests/test_label_ops_ref_host.py proves on the
CPU that the references are autograd's, that honest fp32 arithmetic stays under the bounds and that the named defects exceed them).

Every case runs in a child process, because the library reads S2E_LABEL_CONV_CAP once per process: the default (1024 blocks along
the pixels) and 3, under which every block of either walk makes many passes.  Each child prints the walk or kernel every case ran in
and its largest err / bound; the threshold is 1.  The grid-stride wrap cases run once, each in its cheaper dtype."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (id, S2E_LABEL_CONV_CAP or 0, groups)
_CHILDREN = [
    ('conv-small-batch', 0, 'conv_small,conv_batch'),
    ('conv-wave', 0, 'conv_wave'),
    ('cap3-conv-small-batch', 3, 'conv_small,conv_batch'),
    ('cap3-conv-wave', 3, 'conv_wave'),
    ('onehot-upsample-pool-act-bilinear', 0, 'onehot,upsample,pool,act,bilinear'),
]
_WRAP = ['wrap_upsample', 'wrap_pool,wrap_act,wrap_onehot']


def _run(groups, dtype, cap):
    e = {k: v for k, v in os.environ.items() if not k.startswith('S2E_')}
    cmd = [sys.executable, os.path.join(ROOT, 'tests', '_label_ops_child.py'), '--groups', groups, '--dtype', dtype, '--cap', str(cap)]
    r = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=600, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0 and 'label ops ok:' in r.stdout, (r.stdout[-4000:], r.stderr[-4000:])


@pytest.mark.parametrize('dtype', ['bf16', 'fp32'])
@pytest.mark.parametrize('cap,groups', [c[1:] for c in _CHILDREN], ids=[c[0] for c in _CHILDREN])
def test_label_ops_against_fp64(cap, groups, dtype):
    _run(groups, dtype, cap)


@pytest.mark.parametrize('groups', _WRAP, ids=[g.replace(',', '-') for g in _WRAP])
def test_label_ops_grid_wrap(groups):
    _run(groups, 'none', 0)
