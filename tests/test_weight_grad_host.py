"""The bound tests/test_weight_grad_gpu.py holds csrc/weight_grad.hip to, checked without a GPU: an fp32 emulation of the kernels'
order of operations (tests/_weight_grad_ref.py) stays inside it for every case and both entries, and the schedules the emulation and
the depth count are built on are the ones the library plans."""
import ctypes

import numpy as np
import pytest
import torch

import _weight_grad_ref as R


@pytest.mark.parametrize('entry', ['layer', 'batch'])
@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_fp32_emulation_in_kernel_order_stays_inside_the_bound(case, entry):
    for accumulate in (0, 1):
        ratio = R.chain_ratio(R.emulate(case, entry, accumulate), case, entry, accumulate,
                              'emulated %s %s acc=%d' % (R.case_id(case), entry, accumulate))
        assert ratio > 0.0                                       # (fp32 against fp64: never exact on these inputs)


def test_emulation_sees_a_wrong_index():
    """The bound is tight enough to matter: v read in the packed (tap, ci) order instead of (ci, tap) is far outside it."""
    case = (6, 72, 9, 72)
    d = R.inputs(case)
    sg = float(d['sigma'])
    wrong = d['g'].double() / sg - d['D'] / sg ** 2 * d['u'].double()[:, None, None] * d['v'].double().view(1, 9, 72).permute(0, 2, 1)
    with pytest.raises(AssertionError):
        R.chain_ratio(wrong.float(), case, 'layer', 0, 'transposed v')


def test_batch_schedule_is_the_librarys_block_map():
    from seg2eye_amd import _lib
    L = _lib.lib()
    jobs = (_lib.GradJob * len(R.CASES))()
    for j, case in zip(jobs, R.CASES):
        j.cout, j.cin, j.taps, j.cin_pad = case
    n = L.s2e_grad_block_map(ctypes.byref(jobs), len(jobs), None)
    bm = np.zeros(3 * n, dtype=np.int32)
    assert L.s2e_grad_block_map(ctypes.byref(jobs), len(jobs), bm.ctypes.data) == n
    want = [[j, s[0], len(s)] for j, case in enumerate(R.CASES) for s in R.schedule(case, 'batch')]
    assert bm.reshape(-1, 3).tolist() == want
    assert [R.n_tiles(c) for c in R.CASES] == [1, 4, 2, 16, 6, 9, 2050, 1]
    assert torch.equal(R.inputs(R.CASES[2])['g'][1, 3], R.inputs(R.CASES[2])['gwp'][1, :, 3])
