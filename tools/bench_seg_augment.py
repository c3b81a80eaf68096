#!/usr/bin/env python3
"""Cost of the segmenter's paired augmentation at the training size: a batch of 16 raw 640 x 400 frames with `eyes` label
maps (tests/_segment_ref.py), resized to 320 x 200.

Legs, alternated round by round (same process, same box), each `--launches` back-to-back calls between two HIP events after a warm-up:
  resize           the step's two resize launches alone: ops.resize_bicubic_u8(return_u8=True) and ops.resize_nearest_u8
  resize_augment   the same two plus ops.augment_pairs with a strong rule (its small upload of the parameters included)
  augment          ops.augment_pairs alone, on resized bytes made once; beside it the rate its compulsory bytes -- the frame and the
                   label map in, fp32 and the label map out: 7 bytes per pixel -- give against the 8 TB/s of the HBM
The figure of a leg is the median over `--rounds` rounds of its per-call mean, its spread the min .. max.
Then the mean step time of `segment.train_segmenter` on a synthetic store of `--frames` labelled frames (defaults of `segment train`:
nsf 32, bf16, batches of 16), with and without the rule, alternated over `--step_rounds` rounds of `--epochs` epochs each, a host clock
around a run that ends in a device synchronise; the draws of the rule on the host are part of the step.  Records only: no threshold.
One JSON line; `--out` also writes it to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from _bench_legs import time_legs, write_json  # noqa: E402  (beside this file)
import _seg_augment_ref as R  # noqa: E402  (the host restatement)
import _segment_ref as SR  # noqa: E402  (the inputs)

HBM_BYTES_PER_S = 8.0e12
STRONG = dict(prob=1.0, rotate=25.0, scale=1.4, translate=0.15, gamma=2.0, contrast=0.5, brightness=0.2, lines=8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--frames', type=int, default=64, help='labelled frames of the synthetic store of the step timing')
    ap.add_argument('--epochs', type=int, default=3)
    ap.add_argument('--step_rounds', type=int, default=5)
    ap.add_argument('--out', default=None, help='also write the JSON here (profiles/seg_augment.json)')
    a = ap.parse_args()
    torch.set_num_threads(1)
    from seg2eye_amd import segment
    from seg2eye_amd.ops import augment as A, preprocess as P
    dev = 'cuda:0'
    N, H, W, h, w = a.batch, 640, 400, 320, 200
    lab = SR.eyes(N, H, W, 4, 1)
    img = SR.eye_frames(lab, 'bench_seg_augment', 1)
    img_d, lab_d = torch.from_numpy(img).to(dev), torch.from_numpy(lab).to(dev)
    flip = torch.from_numpy((np.arange(N) % 2).astype(np.uint8)).to(dev)
    rule = A.AugmentRule(**STRONG)
    params = rule.draw(np.random.RandomState(0), N, h, w)

    def resize():
        return P.resize_bicubic_u8(img_d, h, w, flip, return_u8=True)[1], P.resize_nearest_u8(lab_d, h, w, flip)
    x_u8, y = resize()
    got = A.augment_pairs(x_u8, y, params)
    want = R.augment_pairs(x_u8[:2].cpu().numpy(), y[:2].cpu().numpy(), R.Params(*(None if p is None else p[:2] for p in params)))
    assert np.array_equal(got[0][:2].cpu().numpy().view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[2][:2].cpu().numpy(), want[2])
    legs = {'resize': resize, 'resize_augment': lambda: A.augment_pairs(*resize(), params), 'augment': lambda: A.augment_pairs(x_u8, y, params)}
    timed = time_legs(legs, a.rounds, a.launches)
    nbytes = 7 * N * h * w
    timed['augment'].update({'compulsory_bytes': nbytes, 'floor_us': round(nbytes / HBM_BYTES_PER_S * 1e6, 3),
                             'tb_per_s': round(nbytes / (timed['augment']['us_median'] * 1e-6) / 1e12, 4)})
    res = {'device': torch.cuda.get_device_name(0), 'arch': torch.cuda.get_device_properties(0).gcnArchName, 'batch': N, 'raw': [H, W], 'seg_hw': [h, w],
           'rule': STRONG, 'rounds': a.rounds, 'launches_per_round': a.launches, 'hbm_bytes_per_s': HBM_BYTES_PER_S,
           'pixels_changed_share': {'frames': round(float((got[0] != P.resize_bicubic_u8(img_d, h, w, flip)).float().mean()), 4),
                                    'labels': round(float((got[2] != y).float().mean()), 4)}}
    res.update(timed)
    res['added_us_per_batch'] = round(timed['resize_augment']['us_median'] - timed['resize']['us_median'], 2)

    # the step
    slab = SR.eyes(a.frames, H, W, 4, 2)
    store = {'train': {'U001': {'images_ss': SR.eye_frames(slab, 'bench_seg_augment_step', 2), 'labels_ss': slab}}}
    opt = segment.seg_options(niter=a.epochs, seed=0)
    net = segment.build_network(opt, dev)
    steps = a.epochs * ((a.frames + int(opt.batchSize) - 1) // int(opt.batchSize))

    def run(augment):
        torch.cuda.synchronize()
        t = time.perf_counter()
        segment.train_segmenter(store, opt, net=net, device=dev, save=False, verbose=False, augment=augment)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / steps * 1e3
    for augment in (None, rule):                              # warm-up: code objects, allocator blocks
        run(augment)
    ms = {'plain': [], 'augmented': []}
    for _ in range(a.step_rounds):
        ms['plain'].append(run(None))
        ms['augmented'].append(run(rule))
    step = {k: {'ms_median': round(float(np.median(v)), 3), 'ms_min': round(min(v), 3), 'ms_max': round(max(v), 3)} for k, v in ms.items()}
    step.update({'frames': a.frames, 'epochs': a.epochs, 'steps_per_round': steps, 'rounds': a.step_rounds,
                 'added_ms_per_step': round(step['augmented']['ms_median'] - step['plain']['ms_median'], 3),
                 'added_share_of_step': round((step['augmented']['ms_median'] - step['plain']['ms_median']) / step['plain']['ms_median'], 4)})
    res['train_step'] = step
    write_json(res, a.out)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
