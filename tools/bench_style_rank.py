#!/usr/bin/env python3
"""Cost of the style reference ranking at one person's size: M = 64 targets against K = 640 candidates, 640 x 400 masks, four
classes, nested-ellipse maps at jittered positions -- beside the numpy restatement of the same job on this machine's CPU.

Legs, alternated round by round (same process, same box), each `--launches` back-to-back calls between two HIP events after a warm-up:
  l2.dist, mismatch.dist    ops.mask_distances: the zero fill and the int8 MFMA kernel, 2 launches
  topk                      ops.rank_topk(dist, 100, exclude) on the l2 distances: 1 launch
  l2.job, mismatch.job      the two together: what the producer runs per person (uploads apart)
The figure of a leg is the median over `--rounds` rounds of its per-call mean, its spread the min .. max.  Derived from the shapes and the
median of the .dist legs:
  compulsory_bytes          (M + K) P, every mask read once; its rate as a fraction of 8 TB/s
  mfma_ops                  2 M K P int8 multiply-adds for l2, ncls times that for mismatch (one product per class); their rate as a
                            fraction of the dense int8 peak, 5.0e15 op/s (twice bf16's 2.5e15)
numpy: the restatement (int64 differences, one target against blocks of 16 candidates) timed on `--numpy_targets` of the M targets and
scaled to M -- a figure, not an assertion.  The outputs are compared (==) on those targets first.
One JSON line; `--out` also writes it to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _bench_legs import time_legs, write_json  # noqa: E402  (beside this file)

HBM_BYTES_PER_S = 8.0e12
INT8_OPS_PER_S = 5.0e15


def eyes(n, H, W, ncls, seed):
    """Nested ellipses at jittered positions: class c inside class c - 1, background 0."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((n, H, W), dtype=np.uint8)
    for i in range(n):
        cy, cx = H * (0.5 + 0.15 * rng.uniform(-1, 1)), W * (0.5 + 0.15 * rng.uniform(-1, 1))
        ry, rx = H * (0.32 + 0.1 * rng.uniform(-1, 1)), W * (0.4 + 0.1 * rng.uniform(-1, 1))
        for c in range(1, ncls):
            s = 1.0 - (c - 1) / float(ncls)
            out[i][((yy - cy) / (ry * s)) ** 2 + ((xx - cx) / (rx * s)) ** 2 <= 1.0] = c
    return out


def numpy_job(targets, cands, metric, k, exclude):
    """The restatement: int64 distances, np.lexsort on (index, distance)."""
    t = targets.reshape(len(targets), -1)
    c = cands.reshape(len(cands), -1)
    dist = np.empty((len(t), len(c)), dtype=np.int64)
    for m in range(len(t)):
        for k0 in range(0, len(c), 16):
            d = c[k0:k0 + 16].astype(np.int64) - t[m].astype(np.int64)[None, :]
            dist[m, k0:k0 + 16] = (d * d).sum(axis=1) if metric == 'l2' else (d != 0).sum(axis=1)
    idx = np.full((len(t), k), -1, dtype=np.int32)
    for m in range(len(t)):
        order = np.lexsort((np.arange(len(c)), dist[m]))
        order = order[order != exclude[m]][:k]
        idx[m, :len(order)] = order
    return dist, idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--targets', type=int, default=64)
    ap.add_argument('--cands', type=int, default=640)
    ap.add_argument('--height', type=int, default=640)
    ap.add_argument('--width', type=int, default=400)
    ap.add_argument('--top', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--launches', type=int, default=5)
    ap.add_argument('--numpy_targets', type=int, default=2, help='targets the numpy restatement is timed on (scaled to --targets); 0: skip')
    ap.add_argument('--out', default=None, help='also write the JSON here (profiles/style_rank.json)')
    a = ap.parse_args()
    from seg2eye_amd import ops
    dev = 'cuda:0'
    M, K, H, W, ncls = a.targets, a.cands, a.height, a.width, 4
    P = H * W
    t_np, c_np = eyes(M, H, W, ncls, 1), eyes(K, H, W, ncls, 2)
    ex_np = (np.arange(M) * 7 % K).astype(np.int32)
    t, c, ex = torch.from_numpy(t_np).to(dev), torch.from_numpy(c_np).to(dev), torch.from_numpy(ex_np).to(dev)
    dist = ops.mask_distances(t, c, ncls, 'l2')

    def job(metric):
        return ops.rank_topk(ops.mask_distances(t, c, ncls, metric), a.top, ex)

    legs = {'l2.dist': lambda: ops.mask_distances(t, c, ncls, 'l2'), 'mismatch.dist': lambda: ops.mask_distances(t, c, ncls, 'mismatch'),
            'topk': lambda: ops.rank_topk(dist, a.top, ex), 'l2.job': lambda: job('l2'), 'mismatch.job': lambda: job('mismatch')}
    timed = time_legs(legs, a.rounds, a.launches)
    out = {'device': torch.cuda.get_device_name(0), 'arch': torch.cuda.get_device_properties(0).gcnArchName, 'targets': M, 'cands': K,
           'height': H, 'width': W, 'classes': ncls, 'top': a.top, 'rounds': a.rounds, 'launches_per_round': a.launches,
           'compulsory_bytes': (M + K) * P, 'hbm_bytes_per_s': HBM_BYTES_PER_S, 'int8_ops_per_s': INT8_OPS_PER_S}
    out.update(timed)
    for metric, ops_n in (('l2', 2.0 * M * K * P), ('mismatch', 2.0 * M * K * P * ncls)):
        s = timed[metric + '.dist']['us_median'] * 1e-6
        out[metric + '.dist'].update({'mfma_ops': ops_n, 'hbm_fraction': round((M + K) * P / s / HBM_BYTES_PER_S, 5),
                                      'int8_mfma_fraction': round(ops_n / s / INT8_OPS_PER_S, 5)})
    write_json(out, a.out)                                   # the device timings are on disk before the CPU leg starts
    n = min(a.numpy_targets, M)
    if n > 0:
        out['numpy'] = {'targets_timed': n}
        for metric in ('l2', 'mismatch'):
            t0 = time.perf_counter()
            d_np, i_np = numpy_job(t_np[:n], c_np, metric, a.top, ex_np[:n])
            sec = time.perf_counter() - t0
            got_i, _ = job(metric)
            same = bool(np.array_equal(ops.mask_distances(t, c, ncls, metric)[:n].cpu().numpy().astype(np.int64), d_np)
                        and np.array_equal(got_i[:n].cpu().numpy(), i_np))
            scaled = sec * M / n
            out['numpy'][metric] = {'seconds_timed': round(sec, 3), 'seconds_scaled_to_all_targets': round(scaled, 2), 'equal': same,
                                    'ratio_to_job': round(scaled / (timed[metric + '.job']['us_median'] * 1e-6), 1)}
        write_json(out, a.out)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
