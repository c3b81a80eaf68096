#!/usr/bin/env python3
"""Per-launch cost of the averaged-weights Adam step on optimizer G's real arena size.

Three legs on the same arenas, alternated round by round (same process, same box):
  adam      s2e_adam_flat                      (the step without an average)
  fused     s2e_adam_flat_ema                  (the average kept by the Adam launch)
  two_pass  s2e_adam_flat, then ema.lerp_(p, 1 - decay)   (the stock-torch way this design replaces)
beta1 = 0 / no weight decay branch (TTUR): 20, 28 and 20 + 12 bytes per parameter.  Every arena (396 MB at the default n) is
larger than the Infinity Cache, and a leg touches 4 or 5 of them per launch, so no leg runs out of cache.  HIP events around
`--launches` back-to-back launches per leg and round; the figure of a leg is the median over the rounds of its per-launch mean,
its spread the min .. max over the rounds.  One JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=98_990_000, help='elements per arena (optimizer G at ngf 64: 98.99 M)')
    ap.add_argument('--rounds', type=int, default=12)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--decay', type=float, default=0.999)
    a = ap.parse_args()
    from seg2eye_amd import ops
    dev = 'cuda:0'
    n = a.n // 4 * 4
    p = torch.randn(n, device=dev) * 0.05
    g = torch.randn(n, device=dev) * 1e-3
    m, v, ema = torch.zeros(n, device=dev), torch.full((n,), 1e-6, device=dev), p.clone()
    hyper = torch.tensor([1e-4, 0.0, 0.9, 1e-8, 0.0, 1.0, 0.0], dtype=torch.float32, device=dev)
    ema_hyper = torch.tensor([a.decay, 0.0], dtype=torch.float32, device=dev)

    def adam():
        ops.adam_flat_step(p, g, m, v, hyper, skips_m=True)

    def fused():
        ops.adam_flat_ema_step(p, g, m, v, ema, hyper, ema_hyper, skips_m=True)

    def two_pass():
        ops.adam_flat_step(p, g, m, v, hyper, skips_m=True)
        ema.lerp_(p, 1.0 - a.decay)

    legs = {'adam': adam, 'fused': fused, 'two_pass': two_pass}
    for f in legs.values():                                  # warm-up: code objects loaded, clocks up
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
    out = {'n': n, 'rounds': a.rounds, 'launches': a.launches, 'device': torch.cuda.get_device_name(0)}
    nbytes = {'adam': 20, 'fused': 28, 'two_pass': 32}
    for k, xs in ms.items():
        xs = sorted(xs)
        med = xs[len(xs) // 2]
        out[k] = {'ms_median': round(med, 4), 'ms_min': round(xs[0], 4), 'ms_max': round(xs[-1], 4),
                  'TBps': round(nbytes[k] * n / med / 1e9, 2)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
