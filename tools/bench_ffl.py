#!/usr/bin/env python3
"""Cost of the focal-frequency-loss launches beside the stock-torch composition of the same rule, at the bench shape
(N = 8, 256 x 256, bf16 and fp32, alpha = 1) and for the uint8 entry at 640 x 400.

Legs, alternated round by round (same process, same box), each `--launches` back-to-back calls between two HIP events after a warm-up;
per dtype:
  ffl.fwd          ops.focal_freq_loss with x requiring a gradient: s2e_ffl_fwd keeping the spectrum, 3 launches
  ffl.fwd_nospec   ops.focal_freq_loss on detached inputs (what a validation pass runs): 3 launches, no spectrum
  ffl.bwd          s2e_ffl_bwd on the saved spectrum and coefficients: 2 launches
  torch.fwd        the rule in stock torch, fp32 on the GPU from the same images: torch.fft.rfft2(norm='ortho') of the difference, the
                   squared magnitude, the weight (pow, amax, div; detached), the multiplicities of the half spectrum, the mean --
                   recording for autograd
  torch.bwd        autograd's backward through that (the graph retained, the leaf's .grad cleared before each call)
and once:
  ffl_u8.fwd       ops.focal_freq_loss_u8 on a (N, 640, 400) uint8 pair: 3 launches (the Tester's call under --val_ffl)
  torch_u8.fwd     the composition on the same pair (a / 255), no autograd
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


def torch_ffl(x, y, alpha=1.0):
    """The rule in stock torch, fp32: x, y (N,1,H,W) of any float dtype -> (N,)."""
    d = (x.float() - y.float())[:, 0]
    H, W = d.shape[-2:]
    z = torch.fft.rfft2(d, norm='ortho')
    dist = z.real ** 2 + z.imag ** 2
    p = torch.ones_like(dist) if alpha == 0 else dist.detach() ** (alpha / 2.0)
    mx = p.amax(dim=(1, 2), keepdim=True)
    w = torch.where(mx > 0, p / mx.clamp(min=1e-38), torch.zeros_like(p))
    m = torch.full((W // 2 + 1,), 2.0, device=d.device)
    m[0] = 1.0
    if W % 2 == 0:
        m[W // 2] = 1.0
    return (w * dist * m).sum(dim=(1, 2)) / (H * W)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--dtypes', default='bf16,fp32')
    ap.add_argument('--alpha', type=float, default=1.0)
    ap.add_argument('--rounds', type=int, default=30)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--no_count', action='store_true', help='skip the torch.profiler launch count of the composition')
    ap.add_argument('--out', default=None, help='also write the JSON here (profiles/ffl.json)')
    a = ap.parse_args()
    from seg2eye_amd import _lib as L, ops
    from seg2eye_amd.ops.core import _dt, _p, _stream
    dev = 'cuda:0'
    n, H, W, alpha = a.batch, a.size, a.size, a.alpha
    gen = torch.Generator().manual_seed(0)
    x32 = torch.rand(n, 1, H, W, generator=gen) * 2 - 1
    y32 = (x32 + 0.1 * torch.randn(n, 1, H, W, generator=gen)).clamp(-1, 1)
    gs = torch.randn(n, generator=gen).to(dev)
    a8 = torch.randint(0, 256, (n, 1, 640, 400), generator=gen, dtype=torch.uint8).to(dev)
    b8 = (a8.float() + 12 * torch.randn(n, 1, 640, 400, generator=gen).to(dev)).clamp(0, 255).to(torch.uint8)
    legs, launches, keep, info = {}, {}, [], {}
    for name in a.dtypes.split(','):
        dtype = {'bf16': torch.bfloat16, 'fp32': torch.float32}[name]
        x, y = x32.to(dev, dtype), y32.to(dev, dtype)
        xg = x.clone().requires_grad_(True)
        kept = ops.focal_freq_loss(xg, y, alpha)             # (alive for the run: its node owns what the backward leg reads)
        spec, coef, tab = kept.grad_fn.saved_tensors
        dx = torch.empty(n, H, W, dtype=dtype, device=dev)
        ws = torch.empty(int(L.call.s2e_ffl_workspace_bytes(n, H, W)) // 4, dtype=torch.float32, device=dev)
        xt = x.clone().requires_grad_(True)
        st = torch_ffl(xt, y, alpha)
        keep.append((kept, st))

        def torch_bwd(xt=xt, st=st):
            xt.grad = None
            st.backward(gs, retain_graph=True)

        legs.update({
            name + '/ffl.fwd': lambda xg=xg, y=y: ops.focal_freq_loss(xg, y, alpha),
            name + '/ffl.fwd_nospec': lambda x=x, y=y: ops.focal_freq_loss(x, y, alpha),
            name + '/ffl.bwd': lambda x=x, spec=spec, coef=coef, tab=tab, ws=ws, dx=dx: L.call.s2e_ffl_bwd(
                _dt(x), _p(spec), _p(coef), _p(gs), n, H, W, alpha, _p(tab), tab.numel() * 4, _p(ws), ws.numel() * 4, _p(dx), _stream()),
            name + '/torch.fwd': lambda xt=xt, y=y: torch_ffl(xt, y, alpha),
            name + '/torch.bwd': torch_bwd,
        })
        launches.update({name + '/ffl.fwd': 3, name + '/ffl.fwd_nospec': 3, name + '/ffl.bwd': 2, name + '/torch.fwd': None, name + '/torch.bwd': None})
        info[name] = {'spectrum_bytes': spec.numel() * 4, 'workspace_bytes': ws.numel() * 4, 'tables_bytes': tab.numel() * 4,
                      'max_rel_diff_ffl_vs_torch_fp32': float(((ops.focal_freq_loss(x, y, alpha) - torch_ffl(x, y, alpha)).abs() / torch_ffl(x, y, alpha)).max())}
    u8f = lambda t: t.float() / 255
    legs['u8/ffl_u8.fwd'] = lambda: ops.focal_freq_loss_u8(a8, b8, alpha)
    legs['u8/torch_u8.fwd'] = lambda: torch_ffl(u8f(a8), u8f(b8), alpha)
    launches.update({'u8/ffl_u8.fwd': 3, 'u8/torch_u8.fwd': None})
    timed = time_legs(legs, a.rounds, a.launches)
    out = {'device': torch.cuda.get_device_name(0), 'arch': torch.cuda.get_device_properties(0).gcnArchName, 'batch': n, 'size': H, 'alpha': alpha,
           'rounds': a.rounds, 'launches_per_round': a.launches, 'u8_shape': [n, 640, 400]}
    for k, t in timed.items():
        grp, leg = k.split('/')
        out.setdefault(grp, dict(info.get(grp, {})))[leg] = {**t, 'kernel_launches': launches[k]}
    for name in info:
        med = lambda leg: out[name][leg]['us_median']
        out[name]['fwd_bwd_us'] = {'ffl': round(med('ffl.fwd') + med('ffl.bwd'), 2), 'torch': round(med('torch.fwd') + med('torch.bwd'), 2)}
    write_json(out, a.out)                                   # the timings are on disk before the profiler is touched
    if not a.no_count:
        for k in legs:
            if launches[k] is None:
                grp, leg = k.split('/')
                out[grp][leg]['kernel_launches'] = count_kernels(legs[k])
        write_json(out, a.out)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
