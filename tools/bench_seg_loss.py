#!/usr/bin/env python3
"""Cost of the eye segmenter's boundary-aware terms at N = 16 frames of 320 x 200, four classes, bf16: the distance maps,
the fused loss forward and backward, and one training step with the terms on beside the step with them off.

Legs, alternated round by round (same process, same box), each `--launches` back-to-back calls between two HIP events after a warm-up:
  dist            s2e_seg_dist_maps: the column pass and the row pass, 2 launches      } the entry points themselves, called through the
  loss.fwd        s2e_seg_loss_fwd with all three terms: partials and fold, 2 launches } checked binding into buffers allocated once
  loss.bwd        s2e_seg_loss_bwd with all three terms: 1 launch                      }
  ce.fwd, ce.bwd  s2e_seg_ce_fwd / s2e_seg_ce_bwd on the same logits, for scale
  op.loss         ops.seg_dist_maps + ops.seg_loss forward + backward through autograd: what a training step with the terms on pays
  op.ce           ops.seg_cross_entropy forward + backward: what it pays with them off
  step.on         one training step at --nsf with --edge_alpha 20 --lambda_dice 1 --lambda_surface 0.05
  step.off        the same step with the flags at their defaults
For context only (not a leg: the host alone): scipy.ndimage.distance_transform_edt of one 320 x 200 frame, both signs of four classes,
which is what the public recipes pay per frame in the loader.
The figure of a leg is the median over `--rounds` rounds of its per-call mean, its spread the min .. max.  Every kernel leg carries its
compulsory bytes (each operand once) and the rate they give, TB/s, beside the 8 TB/s of the HBM.  Records only: no threshold.
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
from bench_segment import segment_frames  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
RECIPE = dict(lambda_ce=1.0, lambda_dice=1.0, lambda_surface=0.05, edge_alpha=20.0)


def host_edt_us(label, ncls, repeats=5):
    """Median microseconds scipy takes for the signed maps of one frame (None without scipy)."""
    try:
        from scipy.ndimage import distance_transform_edt as edt
    except ImportError:
        return None
    took = []
    for _ in range(repeats):
        t = time.perf_counter()
        for c in range(ncls):
            pos = label == c
            if pos.any() and (~pos).any():
                edt(~pos) * (~pos) - (edt(pos) - 1) * pos
        took.append((time.perf_counter() - t) * 1e6)
    return round(float(np.median(took)), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--height', type=int, default=320)
    ap.add_argument('--width', type=int, default=200)
    ap.add_argument('--nsf', type=int, default=32)
    ap.add_argument('--compute_dtype', default='bf16', choices=['bf16', 'fp32'])
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--out', default=None, help='also write the JSON here (profiles/seg_loss.json)')
    a = ap.parse_args()
    from seg2eye_amd import _lib as L, ops, segment, synthetic
    from seg2eye_amd.ops.core import _dt, _p, _stream
    from seg2eye_amd.optim import FlatAdam
    dev = 'cuda:0'
    N, h, w, ncls, Ho, Wo, radius = a.batch, a.height, a.width, 4, 640, 400, 2
    dtype = torch.bfloat16 if a.compute_dtype == 'bf16' else torch.float32
    esz = 2 if dtype == torch.bfloat16 else 4
    logits = torch.randn(N, h, w, ncls, generator=torch.Generator().manual_seed(0)).to(dtype).to(dev)
    host_label = synthetic.ellipse_labels(N, h, w, seed=3)[:, 0]
    label = torch.from_numpy(host_label).to(dev)
    truth = torch.from_numpy(synthetic.ellipse_labels(N, Ho, Wo, seed=3)[:, 0]).to(dev)
    weights = torch.ones(ncls, device=dev)
    phi, band = ops.seg_dist_maps(label, ncls, radius)
    # ---- the entry points into buffers allocated once
    one = torch.ones((), device=dev)
    ws_d = torch.empty(int(L.call.s2e_seg_dist_workspace_bytes(N, h, w, ncls)) // 4, dtype=torch.int32, device=dev)
    ws_l = torch.empty(int(L.call.s2e_seg_loss_workspace_bytes(N, h, w, ncls)) // 8, dtype=torch.float64, device=dev)
    ws_c = torch.empty(int(L.call.s2e_seg_ce_workspace_bytes(N, h, w)) // 8, dtype=torch.float64, device=dev)
    phi_b, band_b = torch.empty_like(phi), torch.empty_like(band)
    loss_b, terms_b, saved_b = torch.empty((), device=dev), torch.empty(3, device=dev), torch.empty(N * 2 * ncls + 2, device=dev)
    denom_b, dx_b = torch.empty(1, device=dev), torch.empty_like(logits)
    dt, st = _dt(logits), _stream()
    lam = (RECIPE['lambda_ce'], RECIPE['lambda_dice'], RECIPE['lambda_surface'], RECIPE['edge_alpha'])
    legs = {
        'dist': lambda: L.call.s2e_seg_dist_maps(_p(label), N, h, w, ncls, radius, _p(phi_b), _p(band_b), _p(ws_d), ws_d.numel() * 4, st),
        'loss.fwd': lambda: L.call.s2e_seg_loss_fwd(dt, _p(logits), _p(label), _p(weights), _p(phi), _p(band), N, h, w, ncls, ncls, *lam, _p(loss_b),
                                                     _p(terms_b), _p(saved_b), _p(ws_l), ws_l.numel() * 8, st),
        'loss.bwd': lambda: L.call.s2e_seg_loss_bwd(dt, _p(logits), _p(label), _p(weights), _p(phi), _p(band), _p(saved_b), _p(one), N, h, w, ncls, ncls,
                                                     lam[0], lam[2], lam[3], _p(dx_b), st),
        'ce.fwd': lambda: L.call.s2e_seg_ce_fwd(dt, _p(logits), _p(label), _p(weights), N, h, w, ncls, ncls, _p(loss_b), _p(denom_b), _p(ws_c),
                                                 ws_c.numel() * 8, st),
        'ce.bwd': lambda: L.call.s2e_seg_ce_bwd(dt, _p(logits), _p(label), _p(weights), _p(denom_b), _p(one), N, h, w, ncls, ncls, _p(dx_b), st)}
    legs['loss.fwd']()                                           # (saved_b and denom_b hold real values before a backward leg runs)
    legs['ce.fwd']()
    x_on = logits.clone().requires_grad_(True)
    x_off = logits.clone().requires_grad_(True)

    def op_loss():
        x_on.grad = None
        f, b = ops.seg_dist_maps(label, ncls, radius)
        ops.seg_loss(x_on, label, weights, f, b, **RECIPE)[0].backward()

    def op_ce():
        x_off.grad = None
        ops.seg_cross_entropy(x_off, label, weights).backward()

    # ---- one training step with the terms on and off, at nsf (two networks of the same seed, an optimizer each)
    opt = segment.seg_options(nsf=a.nsf, seg_hw=(h, w), compute_dtype=a.compute_dtype, batchSize=N)
    frames = torch.from_numpy(segment_frames(N, Ho, Wo)).to(dev)
    flip = torch.zeros(N, dtype=torch.uint8, device=dev)

    def make_step(on):
        net = segment.build_network(opt, dev)
        optimizer = FlatAdam(list(net.parameters()), lr=1e-3, betas=(0.9, 0.999))

        def step():
            x = ops.resize_bicubic_u8(frames, h, w, flip).unsqueeze(1)
            y = ops.resize_nearest_u8(truth, h, w, flip)
            optimizer.zero_grad()
            if on:
                f, b = ops.seg_dist_maps(y, ncls, radius)
                ops.seg_loss(net(x), y, weights, f, b, **RECIPE)[0].backward()
            else:
                ops.seg_cross_entropy(net(x), y, weights).backward()
            optimizer.step()
        return step

    legs.update({'op.loss': op_loss, 'op.ce': op_ce, 'step.on': make_step(True), 'step.off': make_step(False)})
    timed = time_legs(legs, a.rounds, a.launches)
    P = N * h * w
    floors = {'dist': P * (1 + 4 * ncls + 1), 'loss.fwd': P * (ncls * esz + 1 + 4 * ncls + 1), 'loss.bwd': P * (2 * ncls * esz + 1 + 4 * ncls + 1),
              'ce.fwd': P * (ncls * esz + 1), 'ce.bwd': P * (2 * ncls * esz + 1)}
    out = {'device': torch.cuda.get_device_name(0), 'arch': torch.cuda.get_device_properties(0).gcnArchName, 'batch': N, 'height': h,
           'width': w, 'classes': ncls, 'compute_dtype': a.compute_dtype, 'nsf': a.nsf, 'edge_radius': radius, 'recipe': RECIPE,
           'rounds': a.rounds, 'launches_per_round': a.launches, 'hbm_bytes_per_s': HBM_BYTES_PER_S,
           'band_share': round(float(band.float().mean()), 4), 'host_scipy_edt_us_per_frame': host_edt_us(host_label[0], ncls)}
    out.update(timed)
    for k, nbytes in floors.items():
        s = timed[k]['us_median'] * 1e-6
        out[k].update({'compulsory_bytes': nbytes, 'floor_us': round(nbytes / HBM_BYTES_PER_S * 1e6, 3), 'tb_per_s': round(nbytes / s / 1e12, 4)})
    out['step.on']['frames_per_s'] = round(N / (timed['step.on']['us_median'] * 1e-6), 1)
    out['step.off']['frames_per_s'] = round(N / (timed['step.off']['us_median'] * 1e-6), 1)
    out['step_on_minus_off_us'] = round(timed['step.on']['us_median'] - timed['step.off']['us_median'], 2)
    write_json(out, a.out)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
