"""csrc/weight_grad.hip at the C ABI, element by element against fp64: s2e_unpack_weight_grad and s2e_sn_weight_grad per layer
(accumulate 0 and 1) and one s2e_weight_grads_batched call holding every case as a spectral-norm job and as a plain job, interleaved.
Cases, reference and bound: tests/_weight_grad_ref.py (the bound's constants are checked on the CPU by tests/test_weight_grad_host.py).
Every output and dot workspace sits between guard bands that must come back unchanged: a row group past cout writes nothing.
Worst error / bound per case: docs/EXPERIMENTS.md 3.4."""
import pytest
import torch

import _weight_grad_ref as R
from _conv3x3_child import Guarded

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
_DEVICE_INPUTS = {}


def _on_device(case):
    if case not in _DEVICE_INPUTS:
        _DEVICE_INPUTS[case] = {k: v.to(DEV) for k, v in R.inputs(case).items() if k in ('gwp', 'w', 'u', 'v', 'sigma')}
    return _DEVICE_INPUTS[case]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _out(case, accumulate):
    cout, cin, taps, _ = case
    return Guarded((cout, cin, taps), torch.float32, DEV, fill=R.inputs(case)['start'] if accumulate else float('nan'))


def _per_layer(case, accumulate):
    """(plain result, chain-rule result) of the per-layer entries, guards checked"""
    from seg2eye_amd import _lib as L
    cout, cin, taps, cin_pad = case
    kh, kw = R.KHW[taps]
    x = _on_device(case)
    plain, sn, dot = _out(case, accumulate), _out(case, accumulate), Guarded((1,), torch.float32, DEV, fill=0.0)
    L.call.s2e_unpack_weight_grad(x['gwp'].data_ptr(), plain.ptr(), cout, cin, kh, kw, cin_pad, accumulate, _stream())
    L.call.s2e_sn_weight_grad(x['gwp'].data_ptr(), x['w'].data_ptr(), x['u'].data_ptr(), x['v'].data_ptr(), x['sigma'].data_ptr(),
                              dot.ptr(), sn.ptr(), cout, cin, kh, kw, cin_pad, accumulate, _stream())
    for buf, what in ((plain, 'plain'), (sn, 'chain rule'), (dot, 'dot')):
        buf.check('%s %s acc=%d' % (R.case_id(case), what, accumulate))
    return plain.t.cpu(), sn.t.cpu()


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_per_layer_entries_against_fp64(case, accumulate):
    d = R.inputs(case)
    plain, sn = _per_layer(case, accumulate)
    assert torch.equal(plain, d['start'] + d['g'] if accumulate else d['g'])           # bit for bit: a permute, or one fp32 add
    R.chain_ratio(sn, case, 'layer', accumulate, 'per-layer %s acc=%d' % (R.case_id(case), accumulate))


def _batched():
    """One s2e_weight_grads_batched call over all cases, each as a spectral-norm job and as a plain job (sn, plain, sn, plain, ...),
    every output started from the case's `start`; guards checked.  Returns [(case, is_sn, result)]."""
    from seg2eye_amd import _lib as L
    specs, outs = [], []
    for case in R.CASES:
        x = _on_device(case)
        for sn in (True, False):
            outs.append(_out(case, 1))
            specs.append((case, x['gwp'], outs[-1].t) + ((x['w'], x['u'], x['v'], x['sigma']) if sn else (None,) * 4))
    arr, bm, max_taps, nsn = R.grad_jobs(specs)
    assert nsn == len(R.CASES) and [a.dot_index for a in arr] == [i // 2 if i % 2 == 0 else -1 for i in range(len(arr))]
    assert [b for b in bm.tolist() if b[0] == 2 * R.CASES.index((36, 64, 9, 64))] == [[10, 0, 8], [10, 8, 1]]
    dots = Guarded((nsn,), torch.float32, DEV, fill=0.0)
    jobs_dev, bm_dev = R.to_device(arr, DEV), R.to_device(bm, DEV)
    L.call.s2e_weight_grads_batched(jobs_dev.data_ptr(), bm_dev.data_ptr(), len(bm), max_taps, 1, dots.ptr(), _stream())
    dots.check('batched dots')
    for i, out in enumerate(outs):
        out.check('batched job %d' % i)
    return [(spec[0], spec[3] is not None, out.t.cpu()) for spec, out in zip(specs, outs)]


def test_batched_entry_against_fp64_and_the_per_layer_entries():
    """The batch accumulates, so the outputs start non-zero.  Where one workgroup adds into the dot in both entries -- a one-tile
    job -- the per-layer entry, started from the same buffer, gives the same bits."""
    one_tile = 0
    for case, sn, got in _batched():
        what = 'batched %s %s' % (R.case_id(case), 'chain rule' if sn else 'plain')
        d = R.inputs(case)
        if not sn:
            assert torch.equal(got, d['start'] + d['g']), what
            continue
        R.chain_ratio(got, case, 'batch', 1, what)
        if R.n_tiles(case) == 1:
            one_tile += 1
            assert torch.equal(got, _per_layer(case, 1)[1]), what + ': per-layer and batched bits differ'
    assert one_tile == 2
