#!/usr/bin/env python3
"""Cost of the eye-geometry kernels at N = 16 masks of 640 x 400, four classes, the default curves.

Inputs: `eyes` plus specks (tests/_mask_clean_ref.py: the realistic case) and iid over 4 classes (most pixels are rim pixels of some
curve: the most adds).
Legs, alternated round by round (same process, same box), each `--launches` back-to-back calls between two HIP events after a warm-up,
the entry points themselves called through the checked binding into buffers allocated once:
  moments.<input>   s2e_rim_moments: first moments, centred sums, fold -- 3 launches; compulsory bytes: the labels once per pass
  paint.<input>     s2e_ellipse_paint from the conics the host fitted to that input (every curve marked valid, so that every pixel is
                    evaluated) -- 1 launch; compulsory bytes: the labels in, the mask out
The figure of a leg is the median over `--rounds` rounds of its per-call mean, its spread the min .. max, beside the rate its compulsory
bytes give against the 8 TB/s of the HBM.  For context (not a leg: the host alone, one thread): the same rules for one mask in numpy,
through the restatement of tests/_eye_geometry_ref.py, and the 3 x 3 algebra of the fit for the whole batch.  Records only: no threshold.
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
import _eye_geometry_ref as R  # noqa: E402  (the host restatement)
import _mask_clean_ref as MR  # noqa: E402  (the inputs)

HBM_BYTES_PER_S = 8.0e12
LAUNCHES = {'moments': 3, 'paint': 1}


def host_us(fn, repeats=3):
    took = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        took.append((time.perf_counter() - t) * 1e6)
    return round(float(np.median(took)), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--height', type=int, default=640)
    ap.add_argument('--width', type=int, default=400)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--out', default=None, help='also write the JSON here (profiles/eye_geometry.json)')
    a = ap.parse_args()
    torch.set_num_threads(1)
    from seg2eye_amd import _lib as L, eye_geometry as EG
    from seg2eye_amd.ops import geometry as G
    from seg2eye_amd.ops.core import _p, _stream
    dev = 'cuda:0'
    N, H, W, ncls = a.batch, a.height, a.width, 4
    ins, outs = G._curves(None, ncls)
    K = len(ins)
    paint = np.array([2, 3], dtype=np.uint8)
    inputs = {'eyes_specks': MR.pattern('eyes_specks', (N, H, W)), 'iid4': MR.pattern('iid4', (N, H, W))}
    ws = torch.empty(int(L.call.s2e_rim_moments_workspace_bytes(N, H, W, K)), dtype=torch.uint8, device=dev)
    rim = torch.empty(N, K, G.RIM_WIDTH, dtype=torch.int64, device=dev)
    out = torch.empty(N, H, W, dtype=torch.uint8, device=dev)
    st = _stream()
    legs, info, keep = {}, {}, []
    for name, host in inputs.items():
        lab = torch.from_numpy(np.array(host)).to(dev)
        moments = G.rim_moments(lab, ncls).cpu().numpy()
        assert np.array_equal(moments[:2], R.rim_moments(np.array(host[:2]), ncls))
        fit = EG.ellipse_from_moments(moments, 12, 2.0 * max(H, W))
        conic = np.where(np.isfinite(fit.conic), fit.conic, np.array([0.5, 0.0, 0.5, 0.0, 0.0, -1e4]))     # an unfitted curve: a circle of radius 100
        conic_d, origin_d = torch.from_numpy(conic).to(dev), torch.from_numpy(np.ascontiguousarray(fit.origin)).to(dev)
        valid_d = torch.ones(N, K, dtype=torch.uint8, device=dev)
        keep += [lab, conic_d, origin_d, valid_d]
        legs['moments.' + name] = lambda lab=lab: L.call.s2e_rim_moments(_p(lab), N, H, W, ncls, K, ins.ctypes.data, outs.ctypes.data, _p(rim), _p(ws), ws.numel(), st)
        legs['paint.' + name] = lambda lab=lab, c=conic_d, o=origin_d, v=valid_d: L.call.s2e_ellipse_paint(
            _p(lab), N, H, W, ncls, K, _p(c), _p(o), _p(v), paint.ctypes.data, 1, 1, _p(out), st)
        painted = G.ellipse_paint(lab, conic_d, origin_d, valid_d, ncls)
        one = np.array(host[:1])
        assert np.array_equal(painted[:1].cpu().numpy(), R.paint(one, conic[:1], fit.origin[:1], np.ones((1, K), np.uint8), ncls))
        info[name] = {'rim_pixels_per_mask': [round(float(v), 1) for v in moments[:, :, 0].mean(axis=0)], 'fit_rate': [round(float(v), 4) for v in fit.valid.mean(axis=0)],
                      'pixels_changed_share': round(float((painted != lab).float().mean()), 5),
                      'host_moments_us_per_mask': host_us(lambda: R.rim_moments(one, ncls)),
                      'host_paint_us_per_mask': host_us(lambda: R.paint(one, conic[:1], fit.origin[:1], np.ones((1, K), np.uint8), ncls)),
                      'host_fit_us_per_batch': host_us(lambda: EG.ellipse_from_moments(moments, 12, 2.0 * max(H, W)))}
    timed = time_legs(legs, a.rounds, a.launches)
    P = N * H * W
    res = {'device': torch.cuda.get_device_name(0), 'arch': torch.cuda.get_device_properties(0).gcnArchName, 'batch': N, 'height': H, 'width': W,
           'classes': ncls, 'curves': K, 'rounds': a.rounds, 'launches_per_round': a.launches, 'hbm_bytes_per_s': HBM_BYTES_PER_S, 'inputs': info}
    for k, v in timed.items():
        kind, name = k.split('.')
        nbytes = 2 * P                                        # moments: the labels once per pass; paint: the labels in, the mask out
        host = info[name]['host_moments_us_per_mask' if kind == 'moments' else 'host_paint_us_per_mask']
        v.update({'launches': LAUNCHES[kind], 'compulsory_bytes': nbytes, 'floor_us': round(nbytes / HBM_BYTES_PER_S * 1e6, 3),
                  'tb_per_s': round(nbytes / (v['us_median'] * 1e-6) / 1e12, 4), 'us_per_mask': round(v['us_median'] / N, 2),
                  'host_over_gpu_per_mask': round(host / (v['us_median'] / N), 1)})
        res[k] = v
    write_json(res, a.out)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
