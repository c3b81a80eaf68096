#!/usr/bin/env python3
"""Cost of the SSIM launches beside the stock-torch composition of the same rule, at the bench shape (N = 8, 256 x 256, bf16
by default).

Legs, alternated round by round (same process, same box), each `--launches` back-to-back calls between two HIP events after a warm-up:
  ssim.fwd          ops.ssim with x requiring a gradient: s2e_ssim_fwd writing the three maps, 2 launches
  ssim.fwd_nomaps   ops.ssim on detached inputs (what a validation pass runs): 2 launches, no maps
  ssim.bwd          s2e_ssim_bwd on the saved maps: 1 launch
  ssim_u8.fwd       ops.ssim_u8 on a (N, 640, 400) uint8 pair: 2 launches (the Tester's call under --val_ssim)
  torch.fwd         the rule as tests/_ssim_ref.py states it, in fp32 on the GPU from the same bf16 images (fp32 NCHW copies, five
                    F.conv2d with the 11 x 11 outer-product window, the elementwise tail, the mean), recording for autograd
  torch.bwd         autograd's backward through that (the graph retained, the leaf's .grad cleared before each call)
The figure of a leg is the median over `--rounds` rounds of its per-call mean, its spread the min .. max.  kernel_launches: ours by
construction; the composition's counted by torch.profiler over one call (null where the profiler is not available).  One JSON line;
`--out` also writes it to a file."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _bench_legs import count_kernels, time_legs, write_json  # noqa: E402  (beside this file)


def torch_ssim(x, y):
    """The rule in stock torch, fp32: x, y (N,1,H,W) of any float dtype in [-1, 1] -> (N,)."""
    u, v = (x.float() + 1) / 2, (y.float() + 1) / 2
    i = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-i * i / (2 * 1.5 ** 2))
    k = torch.outer(g / g.sum(), g / g.sum()).float().to(x.device).view(1, 1, 11, 11)
    mu, mv = F.conv2d(u, k), F.conv2d(v, k)
    su2, sv2, suv = F.conv2d(u * u, k) - mu * mu, F.conv2d(v * v, k) - mv * mv, F.conv2d(u * v, k) - mu * mv
    s = (2 * mu * mv + 0.01 ** 2) * (2 * suv + 0.03 ** 2) / ((mu * mu + mv * mv + 0.01 ** 2) * (su2 + sv2 + 0.03 ** 2))
    return s.mean(dim=(1, 2, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32'])
    ap.add_argument('--rounds', type=int, default=30)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--no_count', action='store_true', help='skip the torch.profiler launch count of the composition')
    ap.add_argument('--out', default=None, help='also write the JSON here (profiles/ssim.json)')
    a = ap.parse_args()
    from seg2eye_amd import _lib as L, ops
    from seg2eye_amd.ops.core import _dt, _p, _stream
    dev = 'cuda:0'
    n, H, W = a.batch, a.size, a.size
    dtype = torch.bfloat16 if a.dtype == 'bf16' else torch.float32
    gen = torch.Generator().manual_seed(0)
    x = (torch.rand(n, 1, H, W, generator=gen) * 2 - 1).to(dev, dtype)
    y = (x.float() + 0.1 * torch.randn(n, 1, H, W, generator=gen).to(dev)).clamp(-1, 1).to(dtype)
    gs = torch.randn(n, generator=gen).to(dev)
    a8 = torch.randint(0, 256, (n, 1, 640, 400), generator=gen, dtype=torch.uint8).to(dev)
    b8 = torch.randint(0, 256, (n, 1, 640, 400), generator=gen, dtype=torch.uint8).to(dev)
    xg = x.clone().requires_grad_(True)
    kept = ops.ssim(xg, y)                                   # (alive for the run: its node owns the maps the backward leg reads)
    maps = kept.grad_fn.saved_tensors[2]
    dx = torch.empty(n, H, W, dtype=dtype, device=dev)
    xt = x.clone().requires_grad_(True)
    st = torch_ssim(xt, y)

    def torch_bwd():
        xt.grad = None
        st.backward(gs, retain_graph=True)

    legs = {
        'ssim.fwd': lambda: ops.ssim(xg, y),
        'ssim.fwd_nomaps': lambda: ops.ssim(x, y),
        'ssim.bwd': lambda: L.call.s2e_ssim_bwd(_dt(x), _p(x), _p(y), _p(maps), _p(gs), n, H, W, _p(dx), _stream()),
        'ssim_u8.fwd': lambda: ops.ssim_u8(a8, b8),
        'torch.fwd': lambda: torch_ssim(xt, y),
        'torch.bwd': torch_bwd,
    }
    launches = {'ssim.fwd': 2, 'ssim.fwd_nomaps': 2, 'ssim.bwd': 1, 'ssim_u8.fwd': 2, 'torch.fwd': None, 'torch.bwd': None}
    timed = time_legs(legs, a.rounds, a.launches)
    err = float((ops.ssim(x, y) - torch_ssim(x, y)).abs().max())
    out = {'device': torch.cuda.get_device_name(0), 'arch': torch.cuda.get_device_properties(0).gcnArchName, 'batch': n, 'size': H,
           'dtype': a.dtype, 'rounds': a.rounds, 'launches_per_round': a.launches, 'maps_bytes': maps.numel() * 4,
           'max_abs_diff_ssim_vs_torch_fp32': err}
    for k, t in timed.items():
        out[k] = {**t, 'kernel_launches': launches[k]}
    med = lambda k: out[k]['us_median']
    out['fwd_bwd_us'] = {'ssim': round(med('ssim.fwd') + med('ssim.bwd'), 2), 'torch': round(med('torch.fwd') + med('torch.bwd'), 2)}
    write_json(out, a.out)                                   # the timings are on disk before the profiler is touched
    if not a.no_count:
        for k in ('torch.fwd', 'torch.bwd'):
            out[k]['kernel_launches'] = count_kernels(legs[k])
        write_json(out, a.out)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
