#!/usr/bin/env python3
"""Per-step cost of the gradient guard on the two optimizers' real arena sizes.

Two legs per arena, alternated round by round (same process, same box), beta1 = 0 / no weight decay branch (TTUR):
  plain    s2e_adam_flat                              (what the step launches with the guard off: 20 bytes per parameter)
  guarded  s2e_grad_guard, then s2e_adam_flat_guarded   (the guard's two launches read g once more: 24 bytes per parameter)
and, to tell the read from the fp64 arithmetic, the guard alone (`guard`, 4 bytes per parameter).  The gradient is finite and
max_norm is far above its norm, so the guarded launch does the full step (a skipped step would return at once and flatter the leg).
HIP events around `--launches` back-to-back steps per leg and round; the figure of a leg is the median over `--rounds` rounds of its
per-step mean, its spread the min .. max.  One JSON line; `--out` also writes it to a file."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def bench_arena(n, rounds, launches):
    from seg2eye_amd import ops
    dev = 'cuda:0'
    p = torch.randn(n, device=dev) * 0.05
    g = torch.randn(n, device=dev) * 1e-3
    m, v = torch.zeros(n, device=dev), torch.full((n,), 1e-6, device=dev)
    hyper = torch.tensor([1e-4, 0.0, 0.9, 1e-8, 0.0, 1.0, 0.0], dtype=torch.float32, device=dev)
    guard = torch.tensor([1e9, 1.0, 0, 0, 0, 0, 0, 0], dtype=torch.float32, device=dev)
    first_bad = torch.full((1,), -1, dtype=torch.int32, device=dev)
    ws = ops.grad_guard_workspace(n, dev)

    def plain():
        ops.adam_flat_step(p, g, m, v, hyper, skips_m=True)

    def guard_only():
        ops.grad_guard(g, hyper, guard, first_bad, ws)

    def guarded():
        ops.grad_guard(g, hyper, guard, first_bad, ws)
        ops.adam_flat_guarded_step(p, g, m, v, hyper, guard, skips_m=True)

    legs = {'plain': plain, 'guarded': guarded, 'guard': guard_only}
    for f in legs.values():                                  # warm-up: code objects loaded, clocks up
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, f in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / launches)
    rec = guard.tolist()
    assert rec[3] == 1.0 and rec[4] == 0.0 and int(first_bad) == -1, rec     # every guarded step ran in full
    out = {'n': n}
    nbytes = {'plain': 20, 'guarded': 24, 'guard': 4}
    for k, xs in ms.items():
        xs = sorted(xs)
        med = xs[len(xs) // 2]
        out[k] = {'ms_median': round(med, 4), 'ms_min': round(xs[0], 4), 'ms_max': round(xs[-1], 4),
                  'TBps': round(nbytes[k] * n / med / 1e9, 2)}
    out['added_ms'] = round(out['guarded']['ms_median'] - out['plain']['ms_median'], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n_G', type=int, default=98_990_000, help='elements of optimizer G\'s arena at ngf 64 (98.99 M)')
    ap.add_argument('--n_D', type=int, default=5_530_000, help='elements of optimizer D\'s arena at ndf 64 (5.53 M)')
    ap.add_argument('--rounds', type=int, default=30)
    ap.add_argument('--launches', type=int, default=10)
    ap.add_argument('--out', default=None, help='also write the JSON here (profiles/grad_guard.json)')
    a = ap.parse_args()
    out = {'device': torch.cuda.get_device_name(0), 'arch': torch.cuda.get_device_properties(0).gcnArchName, 'rounds': a.rounds, 'launches': a.launches,
           'G': bench_arena(a.n_G // 4 * 4, a.rounds, a.launches), 'D': bench_arena(a.n_D // 4 * 4, a.rounds, a.launches)}
    out['added_ms_per_iteration'] = round(out['G']['added_ms'] + out['D']['added_ms'], 4)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
