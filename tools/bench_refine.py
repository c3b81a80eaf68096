#!/usr/bin/env python3
"""Cost of the residual refiner's four launches at N = 8 frames of 640 x 400, bf16 and fp32 -- beside the same arithmetic
written in stock torch ops on the same box, which is what they replace.

Legs, alternated round by round (same process, same box), each `--launches` back-to-back calls between two HIP events after a warm-up:
  input           s2e_refine_input: three uint8 planes -> x (N, H, W, 8)                     } the entry points themselves, called
  head.fwd        s2e_refine_head_fwd on a one-channel residual: partials and fold, 2 launches } through the checked binding into
  head.bwd        s2e_refine_head_bwd: 1 launch                                              } buffers allocated once
  predict         s2e_refine_predict_u8: 1 launch                                            }
  torch.input     the lookup of the grey levels, the two-step normalisation, the stack and the cast
  torch.head.fwd  the normalisation of frame and truth, the sum, the clamp, sqrt(sum d^2) per image, the two means, in fp32
  torch.head.bwd  autograd's backward of the same graph to the residual (forward excluded: timed as fwd+bwd minus fwd)
  torch.predict   the normalisation, the sum, the clamp, 127.5 (p + 1) and the cast to uint8
The figure of a leg is the median over `--rounds` rounds of its per-call mean, its spread the min .. max.  Every kernel leg carries its
compulsory bytes (each operand once) and the rate they give, TB/s, beside the 8 TB/s of the HBM.  The outputs are compared first.
One JSON line; `--out` also writes it to a file."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _bench_legs import time_legs, write_json  # noqa: E402  (beside this file)

HBM_BYTES_PER_S = 8.0e12


def run(dtype, a, dev='cuda:0'):
    from seg2eye_amd import _lib as L, ops, synthetic
    from seg2eye_amd.ops.core import _dt, _p, _stream
    N, H, W, C = a.batch, a.height, a.width, 8
    esz = 2 if dtype == torch.bfloat16 else 4
    lab = synthetic.ellipse_labels(2 * N, H, W, seed=3)[:, 0]
    grey = np.array([40, 200, 110, 10], dtype=np.float64)
    img = np.clip(grey[lab] + synthetic.hash_uniform('bench_refine', lab.shape, 0, -24.0, 24.0), 0, 255).astype(np.uint8)
    tmask, rmask, truth, rimg = (torch.from_numpy(v).to(dev) for v in (lab[:N], lab[N:], img[:N], img[N:]))
    levels = torch.tensor(ops.refine.CLASS_LEVELS, dtype=torch.uint8, device=dev)
    lut = torch.zeros(256, dtype=torch.uint8, device=dev)
    lut[:4] = levels
    res = (0.3 * torch.randn(N, H, W, 1, generator=torch.Generator().manual_seed(0))).to(dtype).to(dev)
    scale = torch.tensor(2.0 / 255.0, dtype=torch.float32, device=dev)

    def norm(u8):
        return u8.float() * scale - 1.0

    def torch_input():
        planes = torch.stack([norm(lut[tmask.long()]), norm(rimg), norm(lut[rmask.long()])], dim=-1)
        return torch.cat([planes, planes.new_zeros(N, H, W, C - 3)], dim=-1).to(dtype)

    def torch_loss(r):
        d = torch.clamp(r[..., 0].float() + norm(rimg), -1.0, 1.0) - norm(truth)
        per = torch.sqrt(torch.sum((127.5 * d) ** 2, dim=[1, 2])) / float(H * W)
        return per.mean() + 0.5 * d.abs().mean()

    def torch_predict():
        return (127.5 * (torch.clamp(res[..., 0].float() + norm(rimg), -1.0, 1.0) + 1.0)).to(torch.uint8)

    # ---- the jobs agree
    x = ops.refine_input(tmask, rimg, rmask, dtype=dtype)
    rg = res.clone().requires_grad_(True)
    loss, terms, score = ops.refine_loss(rg, rimg, truth, None, 1.0, 0.5)
    loss.backward()
    rt = res.clone().requires_grad_(True)
    loss_t = torch_loss(rt)
    loss_t.backward()
    agree = {'input_equal': bool(torch.equal(x, torch_input())), 'loss_abs_diff': abs(float(loss.detach()) - float(loss_t.detach())),
             'grad_max_abs_diff': float((rg.grad.float() - rt.grad.float()).abs().max()), 'grad_max_abs': float(rt.grad.float().abs().max()),
             'bytes_equal': bool(torch.equal(ops.refine_predict_u8(res, rimg), torch_predict()))}
    # ---- the legs
    ws = torch.empty(int(L.call.s2e_refine_head_workspace_bytes(N, H, W)) // 8, dtype=torch.float64, device=dev)
    x_b, dres_b, out_b = torch.empty_like(x), torch.empty_like(res), torch.empty(N, H, W, dtype=torch.uint8, device=dev)
    score_b, sumsq_b, terms_b = torch.empty(N, device=dev), torch.empty(N, dtype=torch.float64, device=dev), torch.empty(3, device=dev)
    one = torch.ones((), device=dev)
    dt, st = _dt(res), _stream()
    x_t = res.clone().requires_grad_(True)

    def torch_fwd_bwd():
        x_t.grad = None
        torch_loss(x_t).backward()

    def torch_fwd():
        with torch.no_grad():
            return torch_loss(res)

    legs = {'input': lambda: L.call.s2e_refine_input(dt, _p(tmask), _p(rimg), _p(rmask), None, _p(levels), 4, N, H, W, C, _p(x_b), st),
            'head.fwd': lambda: L.call.s2e_refine_head_fwd(dt, _p(res), 1, _p(rimg), _p(truth), None, N, H, W, _p(score_b), _p(sumsq_b), _p(terms_b),
                                                           _p(ws), ws.numel() * 8, st),
            'head.bwd': lambda: L.call.s2e_refine_head_bwd(dt, _p(res), 1, _p(rimg), _p(truth), None, N, H, W, _p(sumsq_b), _p(one), 1.0, 0.5,
                                                           _p(dres_b), st),
            'predict': lambda: L.call.s2e_refine_predict_u8(dt, _p(res), 1, _p(rimg), None, N, H, W, _p(out_b), st),
            'torch.input': torch_input, 'torch.head.fwd': torch_fwd, 'torch.head.fwd_bwd': torch_fwd_bwd, 'torch.predict': torch_predict}
    timed = time_legs(legs, a.rounds, a.launches)
    P = N * H * W
    floors = {'input': P * (3 + C * esz), 'head.fwd': P * (esz + 2), 'head.bwd': P * (2 * esz + 2), 'predict': P * (esz + 2)}
    out = {'agree': agree}
    out.update(timed)
    for k, nbytes in floors.items():
        s = timed[k]['us_median'] * 1e-6
        out[k].update({'compulsory_bytes': nbytes, 'floor_us': round(nbytes / HBM_BYTES_PER_S * 1e6, 3), 'tb_per_s': round(nbytes / s / 1e12, 4),
                       'share_of_hbm_peak': round(nbytes / s / HBM_BYTES_PER_S, 4)})
    out['torch.head.bwd'] = {'us_median': round(timed['torch.head.fwd_bwd']['us_median'] - timed['torch.head.fwd']['us_median'], 2)}
    for ours, theirs in (('input', 'torch.input'), ('head.fwd', 'torch.head.fwd'), ('head.bwd', 'torch.head.bwd'), ('predict', 'torch.predict')):
        out['ratio.' + theirs] = round(out[theirs]['us_median'] / timed[ours]['us_median'], 2)
    ours = sum(timed[k]['us_median'] for k in floors)
    theirs = timed['torch.input']['us_median'] + timed['torch.head.fwd_bwd']['us_median'] + timed['torch.predict']['us_median']
    out['four_launches_us'], out['torch_us'], out['ratio.all'] = round(ours, 2), round(theirs, 2), round(theirs / ours, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--height', type=int, default=640)
    ap.add_argument('--width', type=int, default=400)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--out', default=None, help='also write the JSON here (profiles/refine.json)')
    a = ap.parse_args()
    out = {'device': torch.cuda.get_device_name(0), 'arch': torch.cuda.get_device_properties(0).gcnArchName, 'batch': a.batch, 'height': a.height,
           'width': a.width, 'input_channels': 8, 'residual_channels': 1, 'rounds': a.rounds, 'launches_per_round': a.launches,
           'hbm_bytes_per_s': HBM_BYTES_PER_S, 'bf16': run(torch.bfloat16, a), 'fp32': run(torch.float32, a)}
    write_json(out, a.out)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
