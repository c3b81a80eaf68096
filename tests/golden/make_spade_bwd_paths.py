#!/usr/bin/env python3
"""Which launches and which GradSink queues one SPADE+Style layer's backward takes, case by case.

    python tests/golden/make_spade_bwd_paths.py --record tests/golden/spade_bwd_paths.json          (on an MI355X)

The fixture tests/golden/spade_bwd_paths.json is recorded on the commit BEFORE a change of the backward's host code (ops/spade.py,
ops/sink.py), through the public ops only, so that this same script runs on both trees; tests/test_spade_bwd_paths_gpu.py runs
`run_case` on the tree under test and compares.  Per case, with a LaunchProfiler installed and nested-ellipse labels: one
ops.spade_style_fused forward and backward, and of it
  forward  : the per-family launch counts of the forward (summary()[family]['launches']),
  backward : those of the backward BEFORE the step's sink flushes,
  queues   : len of pool.sink.wg / c8 / uni / gwg / jobs at that point (None: no trainer-step scope open),
  with_rects : how many of the wg and of the c8 jobs carry a rectangle list (a c8 job with one: d(actv) was left undefined elsewhere),
  flush    : the per-family launch counts of the flush,
or {'raises': <exception class>} when the tree refuses the case.  Gradient VALUES are not recorded (the label-sparse path adds with
float atomics; test_spade_label_sparse_backward holds them to fp64).

CASES are the smallest at which each arm of the backward's plan is reachable, all with nh = 128.  `force`: the fused launch at any
tile count and its label-sparse form at any rectangle count (the maps below 128 x 128 have fewer rectangles than the form's threshold)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

QUEUES = ('wg', 'c8', 'uni', 'gwg', 'jobs')
# name: (N, H, W, C), then what differs from: bf16, ncls 4, channels-last FlatAdam arena, scope open, nothing forced, no switch set
CASES = {
    'n4_128_arena_scope': dict(shape=(4, 128, 128, 64)),                                   # sparse throughout, lazy d(actv)
    'n1_96_min_side': dict(shape=(1, 96, 96, 64), force=True),
    'n1_80_below_min': dict(shape=(1, 80, 80, 64), force=True),                            # sparse forward, dense backward
    'n2_104x96_unaligned': dict(shape=(2, 104, 96, 64), force=True),                       # one side no multiple of 16
    'n1_96_fp32': dict(shape=(1, 96, 96, 64), force=True, dtype='fp32'),
    'n1_96_ncls5': dict(shape=(1, 96, 96, 64), force=True, ncls=5),
    'n1_96_no_scope': dict(shape=(1, 96, 96, 64), force=True, scope=False),
    'n1_96_plain_params': dict(shape=(1, 96, 96, 64), force=True, arena=None),
    'n1_96_torch_order_arena': dict(shape=(1, 96, 96, 64), force=True, arena='torch'),
    'n4_128_sparse_bwd_off': dict(shape=(4, 128, 128, 64), switch='SPARSE_BWD_OFF'),
    'n4_128_c8_sparse_off': dict(shape=(4, 128, 128, 64), switch='C8_SPARSE_OFF'),
    'n4_128_wgrad_batch_off': dict(shape=(4, 128, 128, 64), switch='WGRAD_BATCH_OFF'),
    # the per-call conditions once more at the size whose data-gradient kernel takes a rectangle list (a 96 x 96 map of one sample has
    # too few rectangles for it: there the shape alone already decides for the dense backward)
    'n4_128_fp32': dict(shape=(4, 128, 128, 64), dtype='fp32'),
    'n4_128_ncls5': dict(shape=(4, 128, 128, 64), ncls=5),
    'n4_128_no_scope': dict(shape=(4, 128, 128, 64), scope=False),
    'n4_128_plain_params': dict(shape=(4, 128, 128, 64), arena=None),
    'n4_128_torch_order_arena': dict(shape=(4, 128, 128, 64), arena='torch'),
}


def _rnd(shape, seed, scale=1.0):
    import torch
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _launches(prof):
    import torch
    torch.cuda.synchronize()
    return {fam: d['launches'] for fam, d in sorted(prof.summary().items())}


def _run(shape, force=False, dtype='bf16', ncls=4, scope=True, arena='cl', switch=None):
    import contextlib
    import torch
    from seg2eye_amd import _lib as L, ops
    from seg2eye_amd.optim import FlatAdam
    from seg2eye_amd.synthetic import ellipse_labels
    N, H, W, C = shape
    dev = torch.device('cuda', 0)
    dt = torch.bfloat16 if dtype == 'bf16' else torch.float32
    # (the names of the two bits exist after the change this fixture guards; their values are the header's on both sides)
    flags = (getattr(L, 'SPADE_ANY_TILES', 1) | getattr(L, 'SPADE_ANY_RECTS', 4)) if force else 0
    lab = torch.from_numpy(ellipse_labels(N, H, W, 7)[:, 0]).to(dev)
    w_gb, b_gb = _rnd((2 * C, 128, 3, 3), 56, 0.03), _rnd((2 * C,), 57, 0.1)
    prm = [torch.nn.Parameter(t.to(dev)) for t in (_rnd((128, ncls, 3, 3), 54, 0.3), _rnd((128,), 55, 0.1), w_gb[:C].clone(), b_gb[:C].clone(),
                                                   w_gb[C:].clone(), b_gb[C:].clone())]
    if arena is not None:
        fa = FlatAdam([prm[0], prm[1], prm[2], prm[4], prm[3], prm[5]], lr=1e-3, channels_last=(arena == 'cl'))    # gamma / beta adjacent
        fa.zero_grad()
    x = (_rnd((N, H, W, C), 51) * 1.3 + 0.2).to(dt).to(dev).requires_grad_(True)
    style = _rnd((N, 2 * C), 52, 0.5).to(dev)
    gy = _rnd((N, H, W, C), 53).to(dt).to(dev)
    st = ops.in_stats(x.detach())
    pool = ops.ZeroPool(dev) if scope else None
    prof = ops.LaunchProfiler()
    out = {}
    if switch is not None:
        setattr(ops.switches, switch, True)
    ops.LaunchProfiler.install(prof)
    try:
        with (pool.scope('t') if scope else contextlib.nullcontext()):
            y = ops.spade_style_fused(x, lab, *prm, style, st, True, flags=flags)
            out['forward'] = _launches(prof)
            prof.reset()
            y.backward(gy)
            out['backward'] = _launches(prof)
            out['queues'] = {q: len(getattr(pool.sink, q)) for q in QUEUES} if scope else None
            out['with_rects'] = {q: sum(j.rects is not None for j in getattr(pool.sink, q)) for q in ('wg', 'c8')} if scope else None
            prof.reset()
        out['flush'] = _launches(prof)
    finally:
        ops.LaunchProfiler.install(None)
        if switch is not None:
            setattr(ops.switches, switch, False)
    return out


def run_case(name):
    """What CASES[name] does on this tree (module docstring), or {'raises': <exception class>}."""
    try:
        return _run(**CASES[name])
    except Exception as e:                                       # noqa: BLE001 -- a refusal is an outcome the fixture records
        return {'raises': type(e).__name__, 'message': str(e)[:200]}


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--record')
    a = ap.parse_args()
    res = {name: run_case(name) for name in CASES}
    text = '{\n' + ',\n'.join('"%s":%s' % (name, json.dumps(res[name], sort_keys=True, separators=(',', ':'))) for name in CASES) + '\n}\n'
    if a.record:
        open(a.record, 'w').write(text)
    print(text, end='')
