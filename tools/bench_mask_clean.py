#!/usr/bin/env python3
"""Cost of the mask cleaner at N = 16 masks of 640 x 400, four classes, 8-connectivity, the default modes.

Inputs: `eyes` plus specks (tests/_mask_clean_ref.py: the realistic case) and iid over 4 classes (the worst case for the union: a
quarter of a million components per mask).
Legs, alternated round by round (same process, same box), each `--launches` back-to-back calls between two HIP events after a warm-up,
the entry points themselves called through the checked binding into buffers allocated once:
  components.<input>   s2e_mask_components: label, merge, flatten -- 3 launches
  clean.<input>        s2e_mask_clean: those, then best, keep, column, row -- 7 launches
The figure of a leg is the median over `--rounds` rounds of its per-call mean, its spread the min .. max.  Every leg carries its
compulsory bytes (labels in, ids or mask out, the parent array once each way) and the rate they give beside the 8 TB/s of the HBM.
For context (not a leg: the host alone, one thread): the same rule for one mask on the CPU, through scipy.ndimage where it imports,
otherwise through the numpy restatement -- the only way a user has today.  Records only: no threshold.
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
import _mask_clean_ref as R  # noqa: E402  (the inputs and the host restatement)

HBM_BYTES_PER_S = 8.0e12
LAUNCHES = {'components': 3, 'clean': 7}


def scipy_clean(lab, ncls, modes, conn):
    """The rule through scipy.ndimage.label and distance_transform_edt; None without scipy."""
    try:
        from scipy import ndimage as ndi
    except ImportError:
        return None
    H, W = lab.shape
    st = np.ones((3, 3), int) if conn == 8 else ndi.generate_binary_structure(2, 1)
    kept = np.zeros((H, W), bool)
    for c in range(ncls):
        cc, n = ndi.label(lab == c, structure=st)
        if n == 0:
            continue
        if modes[c] == R.ALL:
            kept |= cc > 0
        elif modes[c] == R.LARGEST:
            kept |= cc == 1 + int(np.argmax(np.bincount(cc.ravel())[1:]))
        else:
            ids = np.unique(np.concatenate([cc[0], cc[-1], cc[:, 0], cc[:, -1]]))
            kept |= np.isin(cc, ids[ids > 0])
    out = lab.copy()
    if not kept.any():
        return out
    best, cls = np.full((H, W), np.iinfo(np.int64).max), np.zeros((H, W), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for c in range(ncls):
        m = kept & (lab == c)
        if m.any():
            _, (iy, ix) = ndi.distance_transform_edt(~m, return_indices=True)
            d2 = (iy - yy).astype(np.int64) ** 2 + (ix - xx).astype(np.int64) ** 2
            upd = d2 < best
            best[upd], cls[upd] = d2[upd], c
    out[~kept] = cls[~kept]
    return out


def host_us(lab, ncls, modes, conn, repeats=3):
    """(path, median microseconds) of the rule on the host for one mask; the result is checked against the restatement once."""
    want = R.clean(lab, ncls, conn, modes)[0]
    got = scipy_clean(lab, ncls, modes, conn)
    path, fn = ('scipy', lambda: scipy_clean(lab, ncls, modes, conn)) if got is not None else ('numpy restatement', lambda: R.clean(lab, ncls, conn, modes))
    assert got is None or np.array_equal(got, want)
    took = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        took.append((time.perf_counter() - t) * 1e6)
    return path, round(float(np.median(took)), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--height', type=int, default=640)
    ap.add_argument('--width', type=int, default=400)
    ap.add_argument('--conn', type=int, default=8)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--out', default=None, help='also write the JSON here (profiles/mask_clean.json)')
    a = ap.parse_args()
    from seg2eye_amd import _lib as L
    from seg2eye_amd.ops import mask_clean as M
    from seg2eye_amd.ops.core import _p, _stream
    dev = 'cuda:0'
    N, H, W, ncls, conn = a.batch, a.height, a.width, 4, a.conn
    modes = np.array(M.default_modes(ncls), dtype=np.uint8)
    inputs = {'eyes_specks': R.pattern('eyes_specks', (N, H, W)), 'iid4': R.pattern('iid4', (N, H, W))}
    ws = torch.empty(int(L.call.s2e_mask_clean_workspace_bytes(N, H, W, ncls)), dtype=torch.uint8, device=dev)
    comp = torch.empty(N, H, W, dtype=torch.int32, device=dev)
    out = torch.empty(N, H, W, dtype=torch.uint8, device=dev)
    stats = torch.empty(N, ncls, 4, dtype=torch.int32, device=dev)
    st = _stream()
    legs, info = {}, {}
    for name, host in inputs.items():
        lab = torch.from_numpy(np.array(host)).to(dev)
        legs['components.' + name] = lambda lab=lab: L.call.s2e_mask_components(_p(lab), N, H, W, ncls, conn, _p(comp), st)
        legs['clean.' + name] = lambda lab=lab: L.call.s2e_mask_clean(_p(lab), N, H, W, ncls, conn, modes.ctypes.data, _p(out), _p(stats), _p(ws), ws.numel(), st)
        cleaned, s = M.mask_clean(lab, ncls, conn, return_stats=True)
        s = s.cpu().numpy().astype(np.int64)
        path, us = host_us(np.array(host[0]), ncls, tuple(int(m) for m in modes), conn)
        info[name] = {'components_per_mask': round(float(s[..., 0].sum()) / N, 1), 'pixels_changed_share': round(float((cleaned != lab).float().mean()), 5),
                      'host_path': path, 'host_us_per_mask': us}
    timed = time_legs(legs, a.rounds, a.launches)
    P = N * H * W
    res = {'device': torch.cuda.get_device_name(0), 'arch': torch.cuda.get_device_properties(0).gcnArchName, 'batch': N, 'height': H, 'width': W,
           'classes': ncls, 'conn': conn, 'modes': [int(m) for m in modes], 'rounds': a.rounds, 'launches_per_round': a.launches,
           'hbm_bytes_per_s': HBM_BYTES_PER_S, 'inputs': info}
    for k, v in timed.items():
        kind, name = k.split('.')
        nbytes = P * (1 + 4 + 4 + (4 if kind == 'components' else 1))   # labels in, parents out and in, ids (the parents again) or mask out
        v.update({'launches': LAUNCHES[kind], 'compulsory_bytes': nbytes, 'floor_us': round(nbytes / HBM_BYTES_PER_S * 1e6, 3),
                  'tb_per_s': round(nbytes / (v['us_median'] * 1e-6) / 1e12, 4), 'us_per_mask': round(v['us_median'] / N, 2)})
        if kind == 'clean':
            v['host_over_gpu_per_mask'] = round(info[name]['host_us_per_mask'] / (v['us_median'] / N), 1)
        res[k] = v
    write_json(res, a.out)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
