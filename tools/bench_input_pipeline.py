#!/usr/bin/env python3
"""What the OpenEDS input pipeline costs per batch, host path against --device_preprocess.  Not part of bench.py.

An in-memory store of random frames (`--samples` per split), batch 8, at 256 x 256 (aspect ratio 1.0) and 320 x 256 (0.8).  Per size:

  host_w0 / host_w8   samples/s of the host path: `__getitem__` (PIL bicubic x 5, nearest, ToTensor, Normalize) + collate +
                      `.to(device)` of label / style_image / target, with 0 and with `--workers` loader workers
  raw_w0 / raw_w8     the same for raw frames from a pinned-memory loader + `ops.materialize`
  critical_path_ms    what the training process itself waits for with the flag on: the copies of one pinned raw batch and the
                      two launches -- HIP events around `materialize` (device time) and a host clock around it that ends in a
                      synchronise (wall time); medians of `--reps`
  kernels_us          the two launches alone on frames that already are on the device, HIP events, median of `--reps`, beside
                      the time of their algorithmic bytes (raw frames read once, outputs written once) at 8 TB/s

Every loader leg is timed from its second batch on (the first pays for starting the workers) and ends in a synchronise.  One
JSON line on stdout (and in --out).  Run it under a `timeout`; nothing here retries a failing step.

    timeout -k 10 600 python tools/bench_input_pipeline.py --out profiles/input_pipeline.json"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEP_MS_BATCH8 = 15.88          # the benchmarked G+D step at batch 8, 256 x 256 (README, round 6)


def make_store(samples, seed=0):
    rng = np.random.RandomState(seed)
    users = ('U001', 'U002')
    n = samples // len(users)
    return {'train': {u: {'images_ss': rng.randint(0, 256, (n, 640, 400)).astype(np.uint8),
                          'labels_ss': rng.randint(0, 4, (n, 640, 400)).astype(np.uint8),
                          'images_gen': rng.randint(0, 256, (16, 640, 400)).astype(np.uint8),
                          'images_ss_filenames': np.array([('%s.%03d_ss' % (u, i)).encode() for i in range(n)], dtype='S13')}
                      for u in users}}


def loader(opt, store, workers):
    from seg2eye_amd.openeds_dataset import OpenEDSDataset
    ds = OpenEDSDataset(opt, store=store, rng=np.random.RandomState(1))
    return torch.utils.data.DataLoader(ds, batch_size=opt.batchSize, shuffle=False, num_workers=workers, drop_last=True,
                                       pin_memory=bool(opt.device_preprocess))


def samples_per_s(opt, store, workers, dev):
    from seg2eye_amd.ops import materialize
    n, t0 = 0, None
    for b in loader(opt, store, workers):
        if opt.device_preprocess:
            b = materialize(b, opt, dev)
        else:
            b = {k: b[k].to(dev) for k in ('label', 'style_image', 'target')}
        if t0 is None:                                       # the first batch started the workers: the clock starts after it
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        else:
            n += b['label'].shape[0]
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=104)
    ap.add_argument('--workers', type=int, default=8)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    assert a.reps >= 20
    from seg2eye_amd import ops
    from seg2eye_amd.options import parse
    dev = torch.device('cuda:0')
    store = make_store(a.samples)
    out = {'device': torch.cuda.get_device_name(0), 'batch': 8, 'samples': a.samples, 'workers': a.workers, 'reps': a.reps,
           'step_ms_batch8': STEP_MS_BATCH8, 'sizes': {}}
    for name, aspect in (('256x256', '1.0'), ('320x256', '0.8')):
        argv = ['--dataset_mode', 'openeds', '--dataset_key', 'train', '--crop_size', '256', '--aspect_ratio', aspect, '--batchSize', '8']
        host, raw = parse(argv), parse(argv + ['--device_preprocess'])
        Ho, Wo = ops.preprocess.fixed_hw(raw)
        r = {}
        # ---- the two launches alone, and the critical path of one pinned batch (both warmed up first)
        batch = next(iter(loader(raw, store, 0)))
        n, ns = batch['style_raw'].shape[:2]
        frames = torch.cat([batch['target_raw'], batch['style_raw'].reshape(n * ns, 640, 400)]).to(dev)
        labels = batch['label_raw'].to(dev)
        flips = torch.cat([batch['flip'], batch['flip'].repeat_interleave(ns)]).view(torch.uint8).to(dev)
        for _ in range(5):
            ops.resize_bicubic_u8(frames, Ho, Wo, flips)
            ops.resize_nearest_u8(labels, Ho, Wo, flips[:n])
            ops.materialize(batch, raw, dev)
        torch.cuda.synchronize()
        k_us, b_us, dev_ms, wall_ms = [], [], [], []
        for _ in range(a.reps):
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            ops.resize_bicubic_u8(frames, Ho, Wo, flips)
            e1.record()
            ops.resize_nearest_u8(labels, Ho, Wo, flips[:n])
            e2.record()
            e2.synchronize()
            k_us.append(e0.elapsed_time(e2) * 1e3)
            b_us.append(e0.elapsed_time(e1) * 1e3)
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            ops.materialize(batch, raw, dev)
            e1.record()
            torch.cuda.synchronize()
            wall_ms.append((time.perf_counter() - t0) * 1e3)
            dev_ms.append(e0.elapsed_time(e1))
        nbytes = (frames.numel() + labels.numel()) + frames.shape[0] * Ho * Wo * 4 + n * Ho * Wo
        r['kernels_us'] = {'bicubic_median': round(statistics.median(b_us), 2), 'median': round(statistics.median(k_us), 2), 'min': round(min(k_us), 2), 'max': round(max(k_us), 2),
                           'algorithmic_bytes': nbytes, 'us_at_8TBps': round(nbytes / 8e12 * 1e6, 2)}
        r['critical_path_ms'] = {'device_median': round(statistics.median(dev_ms), 4), 'device_max': round(max(dev_ms), 4),
                                 'wall_median': round(statistics.median(wall_ms), 4), 'wall_max': round(max(wall_ms), 4),
                                 'raw_bytes_copied': frames.numel() + labels.numel(),
                                 'below_step_ms': bool(statistics.median(wall_ms) < STEP_MS_BATCH8)}
        # ---- the loaders
        for leg, opt, workers in (('host_w0', host, 0), ('raw_w0', raw, 0), ('host_w%d' % a.workers, host, a.workers),
                                  ('raw_w%d' % a.workers, raw, a.workers)):
            r[leg + '_samples_per_s'] = round(samples_per_s(opt, store, workers, dev), 1)
        out['sizes'][name] = r
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
