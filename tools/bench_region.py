#!/usr/bin/env python3
"""Cost of the region-aware error launches beside the stock-torch composition of the same rule, at the bench shape (N = 8,
256 x 256, bf16 by default, four classes, the synthetic batch's label map).

Legs, alternated round by round (same process, same box), each `--launches` back-to-back calls between two HIP events after a warm-up:
  region.fwd        ops.region_loss with x requiring a gradient: s2e_region_loss_fwd, 2 launches
  region.bwd        s2e_region_loss_bwd on the saved images, label and coefficients: 1 launch
  region_u8.fwd     ops.region_stats_u8 on a (N, 640, 400) uint8 pair with the (N, 256, 256) label: 2 launches (the Tester's call under
                    --val_regions)
  torch.fwd         the rule as tests/_region_ref.py states it, on the GPU from the same bf16 images: fp32 differences, one mask per class,
                    masked fp64 sums, the weighted mean of the present classes -- written without any host synchronisation (presence as a
                    0 / 1 factor), recording for autograd
  torch.bwd         autograd's backward through that (the graph retained, the leaf's .grad cleared before each call)
  torch_u8.fwd      the statistics of the uint8 pair in stock torch: the label gathered by integer index, masks, masked fp64 sums
The figure of a leg is the median over `--rounds` rounds of its per-call mean, its spread the min .. max.  kernel_launches: ours by
construction; the composition's counted by torch.profiler over one call (null where the profiler is not available).  One JSON line;
`--out` also writes it to a file."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _bench_legs import count_kernels, time_legs, write_json  # noqa: E402  (beside this file)


def torch_region_loss(x, y, label, w, norm):
    """The rule in stock torch with no host synchronisation: x, y (N,1,H,W) float, label (N,H,W) uint8 of the same size, w (ncls,) fp32."""
    d = x.float()[:, 0] - y.float()[:, 0]
    f = (d.abs() if norm == 'l1' else d * d).double()
    num = den = 0.0
    for c in range(w.numel()):
        m = (label == c).double()
        n_c = m.sum()
        present = (n_c > 0).double()
        num = num + present * w[c].double() * (f * m).sum() / n_c.clamp(min=1.0)
        den = den + present * w[c].double()
    return (num / den.clamp(min=1e-300)).float()


def torch_region_stats_u8(a, b, label, ncls):
    """(N, ncls, 3) float64 of two (N,H,W) uint8 images, the label (N,Hl,Wl) looked up at [(r Hl) // H, (c Wl) // W]."""
    H, W = a.shape[1:]
    ri = (torch.arange(H, device=a.device) * label.shape[1]) // H
    ci = (torch.arange(W, device=a.device) * label.shape[2]) // W
    l = label[:, ri][:, :, ci]
    d = a.double() - b.double()
    rows = []
    for c in range(ncls):
        m = (l == c).double()
        rows.append(torch.stack([m.sum(dim=(1, 2)), (d.abs() * m).sum(dim=(1, 2)), (d * d * m).sum(dim=(1, 2))], dim=1))
    return torch.stack(rows, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32'])
    ap.add_argument('--norm', default='l1', choices=['l1', 'l2'])
    ap.add_argument('--rounds', type=int, default=30)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--no_count', action='store_true', help='skip the torch.profiler launch count of the composition')
    ap.add_argument('--out', default=None, help='also write the JSON here (profiles/region.json)')
    a = ap.parse_args()
    from seg2eye_amd import _lib as L, ops, synthetic as syn
    from seg2eye_amd.ops.core import _dt, _p, _stream
    dev = 'cuda:0'
    n, H, W, ncls = a.batch, a.size, a.size, 4
    dtype = torch.bfloat16 if a.dtype == 'bf16' else torch.float32
    norm = L.REGION_L1 if a.norm == 'l1' else L.REGION_L2
    gen = torch.Generator().manual_seed(0)
    x = (torch.rand(n, 1, H, W, generator=gen) * 2 - 1).to(dev, dtype)
    y = (x.float() + 0.1 * torch.randn(n, 1, H, W, generator=gen).to(dev)).clamp(-1, 1).to(dtype)
    label = torch.from_numpy(syn.make_batch(n, H, W, seed=21)['label'])[:, 0].to(dev).contiguous()
    w = torch.ones(ncls, device=dev)
    gs = torch.tensor(1.25, device=dev)
    a8 = torch.randint(0, 256, (n, 640, 400), generator=gen, dtype=torch.uint8).to(dev)
    b8 = torch.randint(0, 256, (n, 640, 400), generator=gen, dtype=torch.uint8).to(dev)
    xg = x.clone().requires_grad_(True)
    kept, _ = ops.region_loss(xg, y, label, w, a.norm)       # (alive for the run: its node owns what the backward leg reads)
    xs, ys, ls, coef = kept.grad_fn.saved_tensors
    dx = torch.empty(n, H, W, dtype=dtype, device=dev)
    xt = x.clone().requires_grad_(True)
    st = torch_region_loss(xt, y, label, w, a.norm)

    def torch_bwd():
        xt.grad = None
        st.backward(gs, retain_graph=True)

    legs = {
        'region.fwd': lambda: ops.region_loss(xg, y, label, w, a.norm),
        'region.bwd': lambda: L.call.s2e_region_loss_bwd(_dt(xs), _p(xs), _p(ys), _p(ls), _p(coef), _p(gs), n, H, W, H, W, ncls, norm, _p(dx), _stream()),
        'region_u8.fwd': lambda: ops.region_stats_u8(a8, b8, label, ncls),
        'torch.fwd': lambda: torch_region_loss(xt, y, label, w, a.norm),
        'torch.bwd': torch_bwd,
        'torch_u8.fwd': lambda: torch_region_stats_u8(a8, b8, label, ncls),
    }
    launches = {'region.fwd': 2, 'region.bwd': 1, 'region_u8.fwd': 2, 'torch.fwd': None, 'torch.bwd': None, 'torch_u8.fwd': None}
    timed = time_legs(legs, a.rounds, a.launches)
    ours, theirs = ops.region_loss(x, y, label, w, a.norm)[0], torch_region_loss(x, y, label, w, a.norm)
    same_u8 = bool(torch.equal(ops.region_stats_u8(a8, b8, label, ncls), torch_region_stats_u8(a8, b8, label, ncls)))
    out = {'device': torch.cuda.get_device_name(0), 'arch': torch.cuda.get_device_properties(0).gcnArchName, 'batch': n, 'size': H,
           'dtype': a.dtype, 'norm': a.norm, 'classes': ncls, 'rounds': a.rounds, 'launches_per_round': a.launches,
           'bytes_moved_fwd': 2 * x.numel() * x.element_size() + label.numel(),
           'rel_diff_loss_vs_torch': float((ours - theirs).abs() / theirs.abs()), 'stats_u8_equal_torch': same_u8}
    for k, t in timed.items():
        out[k] = {**t, 'kernel_launches': launches[k]}
    med = lambda k: out[k]['us_median']
    out['fwd_bwd_us'] = {'region': round(med('region.fwd') + med('region.bwd'), 2), 'torch': round(med('torch.fwd') + med('torch.bwd'), 2)}
    write_json(out, a.out)                                   # the timings are on disk before the profiler is touched
    if not a.no_count:
        for k in ('torch.fwd', 'torch.bwd', 'torch_u8.fwd'):
            out[k]['kernel_launches'] = count_kernels(legs[k])
        write_json(out, a.out)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
