#!/usr/bin/env python3
"""Cost of the eye segmenter's three kernels, one training step and the mask writer at N = 16 frames of 320 x 200, four
classes, bf16 -- beside stock torch doing the same jobs on the same box.

Legs, alternated round by round (same process, same box), each `--launches` back-to-back calls between two HIP events after a warm-up:
  ce.fwd          s2e_seg_ce_fwd: the partials and the fold, 2 launches            } the entry points themselves, called through the
  ce.bwd          s2e_seg_ce_bwd: 1 launch (the scalar's gradient is on the device) } checked binding into buffers allocated once:
  argmax          s2e_seg_argmax_u8 to 640 x 400: 1 launch                         } the kernels' time as far as back-to-back
  confusion       s2e_seg_confusion_u8 of 16 masks of 640 x 400: 1 launch          } launches show it
  op.ce           ops.seg_cross_entropy forward + backward through autograd: what a training step pays
  op.argmax       ops.seg_argmax_u8 (allocates the mask)
  op.confusion    ops.seg_confusion into a kept matrix
  torch.ce        F.cross_entropy(logits.float(), ...) forward + backward to the logits
  torch.argmax    F.interpolate(bilinear, 640 x 400).argmax(1)
  torch.bincount  torch.bincount(truth * ncls + pred, minlength=ncls^2)
  step            one training step at --nsf: resize, forward, loss, backward, FlatAdam
  predict         16 frames through resize, the network and the argmax (no copy back): frames/s
The figure of a leg is the median over `--rounds` rounds of its per-call mean, its spread the min .. max.  Every kernel leg carries its
compulsory bytes (each operand once) and the rate they give, TB/s, beside the 8 TB/s of the HBM.  The outputs of the kernel and torch
legs are compared first (the masks where torch's own fp32 result is not within 1e-5 of a tie).
One JSON line; `--out` also writes it to a file."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _bench_legs import time_legs, write_json  # noqa: E402  (beside this file)

HBM_BYTES_PER_S = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--height', type=int, default=320)
    ap.add_argument('--width', type=int, default=200)
    ap.add_argument('--nsf', type=int, default=32)
    ap.add_argument('--compute_dtype', default='bf16', choices=['bf16', 'fp32'])
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--out', default=None, help='also write the JSON here (profiles/segment.json)')
    a = ap.parse_args()
    from seg2eye_amd import ops, segment, synthetic
    from seg2eye_amd.optim import FlatAdam
    dev = 'cuda:0'
    N, h, w, ncls, Ho, Wo = a.batch, a.height, a.width, 4, 640, 400
    dtype = torch.bfloat16 if a.compute_dtype == 'bf16' else torch.float32
    esz = 2 if dtype == torch.bfloat16 else 4
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(N, h, w, ncls, generator=g).to(dtype).to(dev)
    label = torch.from_numpy(synthetic.ellipse_labels(N, h, w, seed=3)[:, 0]).to(dev)
    truth = torch.from_numpy(synthetic.ellipse_labels(N, Ho, Wo, seed=3)[:, 0]).to(dev)
    weights = torch.ones(ncls, device=dev)
    # ---- the jobs agree
    lg = logits.clone().requires_grad_(True)
    loss = ops.seg_cross_entropy(lg, label, weights)
    loss.backward()
    lt = logits.float().requires_grad_(True)
    loss_t = F.cross_entropy(lt.permute(0, 3, 1, 2), label.long())
    loss_t.backward()
    pred = ops.seg_argmax_u8(logits, Ho, Wo)
    up = F.interpolate(logits.float().permute(0, 3, 1, 2), size=(Ho, Wo), mode='bilinear', align_corners=False)
    top2 = up.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-5
    conf = ops.seg_confusion(pred, truth, ncls)
    conf_t = torch.bincount(truth.long().view(-1) * ncls + pred.long().view(-1), minlength=ncls * ncls).view(ncls, ncls)
    agree = {'loss_abs_diff': abs(float(loss.detach()) - float(loss_t.detach())), 'grad_max_abs_diff': float((lg.grad.float() - lt.grad).abs().max()),
             'masks_equal_away_from_ties': bool(torch.equal(pred[clear], up.argmax(1).to(torch.uint8)[clear])),
             'pixels_near_a_tie': int((~clear).sum()), 'confusion_equal': bool(torch.equal(conf, conf_t))}
    # ---- the kernel legs and torch's
    one = torch.ones((), device=dev)
    x_ce = logits.clone().requires_grad_(True)
    x_t = logits.clone().requires_grad_(True)

    def op_ce():
        x_ce.grad = None
        ops.seg_cross_entropy(x_ce, label, weights).backward()

    from seg2eye_amd import _lib as L
    from seg2eye_amd.ops.core import _dt, _p, _stream
    ws = torch.empty(int(L.call.s2e_seg_ce_workspace_bytes(N, h, w)) // 8, dtype=torch.float64, device=dev)
    loss_b, denom_b, dx_b = torch.empty((), device=dev), torch.empty(1, device=dev), torch.empty_like(logits)
    mask_b = torch.empty(N, Ho, Wo, dtype=torch.uint8, device=dev)
    conf_b = torch.zeros(ncls, ncls, dtype=torch.int64, device=dev)
    dt, st = _dt(logits), _stream()
    raw = {'ce.fwd': lambda: L.call.s2e_seg_ce_fwd(dt, _p(logits), _p(label), _p(weights), N, h, w, ncls, ncls, _p(loss_b), _p(denom_b), _p(ws),
                                                   ws.numel() * 8, st),
           'ce.bwd': lambda: L.call.s2e_seg_ce_bwd(dt, _p(logits), _p(label), _p(weights), _p(denom_b), _p(one), N, h, w, ncls, ncls, _p(dx_b), st),
           'argmax': lambda: L.call.s2e_seg_argmax_u8(dt, _p(logits), N, h, w, ncls, ncls, Ho, Wo, _p(mask_b), st),
           'confusion': lambda: L.call.s2e_seg_confusion_u8(_p(pred), _p(truth), pred.numel(), ncls, _p(conf_b), st)}

    def torch_ce():
        x_t.grad = None
        F.cross_entropy(x_t.float().permute(0, 3, 1, 2), label.long()).backward()

    def torch_argmax():
        return F.interpolate(logits.float().permute(0, 3, 1, 2), size=(Ho, Wo), mode='bilinear', align_corners=False).argmax(1)

    def torch_bincount():
        return torch.bincount(truth.long().view(-1) * ncls + pred.long().view(-1), minlength=ncls * ncls)

    conf_acc = torch.zeros(ncls, ncls, dtype=torch.int64, device=dev)
    # ---- one training step and the mask writer, at nsf
    opt = segment.seg_options(nsf=a.nsf, seg_hw=(h, w), compute_dtype=a.compute_dtype, batchSize=N)
    net = segment.build_network(opt, dev)
    optimizer = FlatAdam(list(net.parameters()), lr=1e-3, betas=(0.9, 0.999))
    frames = torch.from_numpy(segment_frames(N, Ho, Wo)).to(dev)
    flip = torch.zeros(N, dtype=torch.uint8, device=dev)

    def step():
        x = ops.resize_bicubic_u8(frames, h, w, flip).unsqueeze(1)
        y = ops.resize_nearest_u8(truth, h, w, flip)
        optimizer.zero_grad()
        ops.seg_cross_entropy(net(x), y, weights).backward()
        optimizer.step()

    def predict():
        with torch.no_grad():
            return ops.seg_argmax_u8(net(ops.resize_bicubic_u8(frames, h, w, flip).unsqueeze(1)), Ho, Wo)

    legs = dict(raw)
    legs.update({'op.ce': op_ce, 'op.argmax': lambda: ops.seg_argmax_u8(logits, Ho, Wo),
                 'op.confusion': lambda: ops.seg_confusion(pred, truth, ncls, out=conf_acc), 'torch.ce': torch_ce,
                 'torch.argmax': torch_argmax, 'torch.bincount': torch_bincount, 'step': step, 'predict': predict})
    timed = time_legs(legs, a.rounds, a.launches)
    P = N * h * w
    floors = {'ce.fwd': P * (ncls * esz + 1), 'ce.bwd': P * (2 * ncls * esz + 1), 'argmax': P * ncls * esz + N * Ho * Wo,
              'confusion': 2 * N * Ho * Wo}
    out = {'device': torch.cuda.get_device_name(0), 'arch': torch.cuda.get_device_properties(0).gcnArchName, 'batch': N, 'height': h,
           'width': w, 'classes': ncls, 'compute_dtype': a.compute_dtype, 'nsf': a.nsf, 'mask_height': Ho, 'mask_width': Wo,
           'rounds': a.rounds, 'launches_per_round': a.launches, 'hbm_bytes_per_s': HBM_BYTES_PER_S, 'agree': agree}
    out.update(timed)
    for k, nbytes in floors.items():
        s = timed[k]['us_median'] * 1e-6
        out[k].update({'compulsory_bytes': nbytes, 'floor_us': round(nbytes / HBM_BYTES_PER_S * 1e6, 3), 'tb_per_s': round(nbytes / s / 1e12, 4)})
    for ours, theirs in (('op.ce', 'torch.ce'), ('op.argmax', 'torch.argmax'), ('op.confusion', 'torch.bincount')):
        out['ratio.' + theirs] = round(timed[theirs]['us_median'] / timed[ours]['us_median'], 2)
    out['predict']['frames_per_s'] = round(N / (timed['predict']['us_median'] * 1e-6), 1)
    out['step']['frames_per_s'] = round(N / (timed['step']['us_median'] * 1e-6), 1)
    write_json(out, a.out)
    print(json.dumps(out))


def segment_frames(n, H, W):
    """Synthetic eye frames: a grey level per class of synthetic.ellipse_labels plus hash noise."""
    from seg2eye_amd import synthetic
    lab = synthetic.ellipse_labels(n, H, W, seed=3)[:, 0]
    grey = np.array([40, 200, 110, 10], dtype=np.float64)
    return np.clip(grey[lab] + synthetic.hash_uniform('bench_segment', lab.shape, 0, -24.0, 24.0), 0, 255).astype(np.uint8)


if __name__ == '__main__':
    main()
