#!/usr/bin/env python3
"""Cost of the differentiable augmentation of D's input beside the plain ops.d_input, at the bench shape (N = 8, 256 x 256,
bf16 by default).

Legs, alternated round by round (same process, same box), each `--launches` back-to-back calls between two HIP events after a warm-up:
  d_input.fwd          ops.d_input: two s2e_onehot_nhwc launches                      (what every D forward runs with the flag off)
  d_input.bwd          its backward: one strided copy of channel ncls of the first half
  aug.fwd / aug.fwd_nocolor    ops.d_input_aug with / without colour in the policy: 2 / 1 launches
  aug.bwd / aug.bwd_nocolor    s2e_d_input_aug_bwd: 2 / 1 launches
The rows are a fixed draw of the full policy (their values do not change the launches).  The figure of a leg is the median over
`--rounds` rounds of its per-call mean, its spread the min .. max.  Next to them the byte floor from the shapes: forward label + two
images in and 2N * H * W * 16 bytes out (bf16); backward one gradient element in and one out per pixel of the N fake images (the strided
read really moves the whole 16- or 32-byte pixel).  An iteration runs D's input twice (G step: forward + backward; D step: forward), so
added_ms_per_iteration = 2 * (aug.fwd - d_input.fwd) + (aug.bwd - d_input.bwd).  One JSON line; `--out` also writes it to a file."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32'])
    ap.add_argument('--rounds', type=int, default=30)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--out', default=None, help='also write the JSON here (profiles/diffaug.json)')
    a = ap.parse_args()
    from seg2eye_amd import _lib as L, diffaug, ops
    from seg2eye_amd.ops.core import _dt, _p, _stream
    dev = 'cuda:0'
    n, H, W, ncls, cpad = a.batch, a.size, a.size, 4, 8
    dtype = torch.bfloat16 if a.dtype == 'bf16' else torch.float32
    gen = torch.Generator().manual_seed(0)
    label = torch.randint(0, ncls, (n, H, W), generator=gen, dtype=torch.uint8).to(dev)
    fake = (torch.rand(n, 1, H, W, generator=gen) * 2 - 1).to(dev, dtype)
    real = (torch.rand(n, 1, H, W, generator=gen) * 2 - 1).to(dev, dtype)
    rows = diffaug.sample('color,translation,cutout', n, H, W, gen).to(dev)
    g = torch.randn(2 * n, H, W, cpad, generator=gen).to(dev, dtype)
    dfake = torch.empty(n, H, W, dtype=dtype, device=dev)
    ws = torch.empty(int(L.call.s2e_d_input_aug_workspace_bytes(n, H, W)) // 8, dtype=torch.float64, device=dev)

    def aug_bwd(color):
        L.call.s2e_d_input_aug_bwd(_dt(g), _p(g), _p(rows), _p(dfake), _p(ws), n, H, W, ncls, cpad, color, _stream())

    legs = {
        'd_input.fwd': lambda: ops.d_input(label, fake, real, ncls, cpad),
        'd_input.bwd': lambda: g[:n, :, :, ncls].contiguous(),
        'aug.fwd': lambda: ops.d_input_aug(label, fake, real, rows, ncls, cpad, color=True),
        'aug.fwd_nocolor': lambda: ops.d_input_aug(label, fake, real, rows, ncls, cpad, color=False),
        'aug.bwd': lambda: aug_bwd(1),
        'aug.bwd_nocolor': lambda: aug_bwd(0),
    }
    launches = {'d_input.fwd': 2, 'd_input.bwd': 1, 'aug.fwd': 2, 'aug.fwd_nocolor': 1, 'aug.bwd': 2, 'aug.bwd_nocolor': 1}
    for f in legs.values():                                  # warm-up: code objects loaded, allocator blocks cached, clocks up
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, f in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.launches)
    es = fake.element_size()
    px = n * H * W
    floor = {'fwd': px + 2 * px * es + 2 * px * cpad * es, 'bwd': 2 * px * es}
    out = {'device': torch.cuda.get_device_name(0), 'arch': torch.cuda.get_device_properties(0).gcnArchName, 'batch': n, 'size': H,
           'dtype': a.dtype, 'rounds': a.rounds, 'launches_per_round': a.launches, 'floor_bytes': floor}
    for k, xs in ms.items():
        xs = sorted(xs)
        med = xs[len(xs) // 2]
        out[k] = {'ms_median': round(med, 5), 'ms_min': round(xs[0], 5), 'ms_max': round(xs[-1], 5), 'kernel_launches': launches[k],
                  'floor_TBps': round(floor[k.split('.')[1][:3]] / med / 1e9, 3)}
    med = lambda k: out[k]['ms_median']
    out['added_ms_per_iteration'] = round(2 * (med('aug.fwd') - med('d_input.fwd')) + med('aug.bwd') - med('d_input.bwd'), 5)
    out['added_ms_per_iteration_nocolor'] = round(2 * (med('aug.fwd_nocolor') - med('d_input.fwd')) + med('aug.bwd_nocolor') - med('d_input.bwd'), 5)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
