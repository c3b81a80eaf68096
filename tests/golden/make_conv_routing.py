#!/usr/bin/env python3
"""Sweep a grid of conv descriptors through the library's ten per-shape routing queries and digest the answers.

    python tests/golden/make_conv_routing.py --lib <libseg2eye_hip.so> --record tests/golden/conv_routing.json
    python tests/golden/make_conv_routing.py --lib <libseg2eye_hip.so> --env NAME        (one environment, JSON on stdout)

The fixture tests/golden/conv_routing.json is recorded with --lib pointing at a build of the commit BEFORE a change of the
dispatch (a scratch checkout of it), never at the code under test; tests/test_conv_routing_host.py runs the same sweep on the
tree's own library and compares.  No GPU needed, plain ctypes, no torch.

The library reads its switches once per process, so every environment is a child process of its own (--env), started with
every S2E_* variable removed and the environment's one switch set.

A slice is (environment, dtype, (k, stride, pad), direction).  Per slice: `sha` = SHA-256 of the seven kind / slot / support
columns of every descriptor in sweep order, `sha_ws` = the same of the three workspace columns (they depend on the CU count
the library sees: 256 without a device and on an MI355X; `cus` records what the sweep saw, from a stream-K shape whose
workspace is 2 * CUs * 128 * 128 floats), and per column the number of distinct values and the non-zero share -- an empty or
degenerate grid shows there (`distinct` of an environment: the same over all of its slices).  `rects_with_workspace` counts the
descriptors that take a rectangle list (the duo kernel) and still report forward workspace: DESIGN 3.3's invariant says none.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ENVS = {'default': {}, 'duo0': {'S2E_CONV_DUO': '0'}, 'patch0': {'S2E_CONV_PATCH': '0'}, 'stream2': {'S2E_CONV_STREAM': '2'},
        'plane0': {'S2E_CONV_PLANE': '0'}, 'deterministic': {'S2E_DETERMINISTIC': '1'}}
DTYPES = (0, 1)                                                  # S2E_F32, S2E_BF16
BATCHES = (1, 8, 16)
MAPS = [(s, s) for s in (4, 8, 16, 32, 64, 128, 256, 17, 18, 33, 34, 65, 129)] + [(66, 50), (24, 40), (96, 160), (384, 640)]
CHANNELS = (1, 3, 8, 32, 40, 64, 96, 128, 256, 384, 512, 1024, 2048)  # either side of: % 8, <= 32, > 64, % 64, % 128, == 8
KSP = ((1, 1, 0), (3, 1, 1), (3, 1, 0), (3, 2, 1), (4, 1, 2), (4, 2, 2), (4, 2, 1), (5, 1, 2))
ACTS = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 2, 0), (0, 0, 1))      # (in_act, out_act, aux_mode); no planner tells the two masks apart
QUERIES = ('s2e_conv2d_kernel_kind', 's2e_conv2d_workspace_bytes', 's2e_conv2d_stats_slots', 's2e_conv2d_rects_supported',
           's2e_conv2d_plane_supported', 's2e_conv2d_wgrad_kernel_kind', 's2e_conv2d_wgrad_workspace_bytes',
           's2e_conv2d_wgrad_rects_workspace_bytes', 's2e_conv2d_wgrad_multi_supported', 's2e_conv2d_wgrad_multi_kind')
WS_COLS = [i for i, q in enumerate(QUERIES) if q.endswith('workspace_bytes')]
KIND_COLS = [i for i in range(len(QUERIES)) if i not in WS_COLS]
FIELDS = ('N', 'Hi', 'Wi', 'Cin', 'Ho', 'Wo', 'Cout', 'KH', 'KW', 'stride', 'pad', 'transposed', 'in_act', 'out_act', 'aux_mode')


class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_int) for n in FIELDS]


def descriptors(k, stride, pad, transposed):
    """The slice's descriptors in sweep order.  direction 1 = the data gradient of the forward conv map -> out: x is the gradient."""
    for n in BATCHES:
        for h, w in MAPS:
            ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
            if ho <= 0 or wo <= 0:
                continue
            for ci in CHANNELS:
                for co in CHANNELS:
                    for ia, oa, am in ACTS:
                        if transposed:
                            yield (n, ho, wo, co, h, w, ci, k, k, stride, pad, 1, ia, oa, am)
                        else:
                            yield (n, h, w, ci, ho, wo, co, k, k, stride, pad, 0, ia, oa, am)


def sweep(lib_path):
    lib = C.CDLL(lib_path)
    fns = []
    for q in QUERIES:
        f = getattr(lib, q)
        f.argtypes, f.restype = [C.c_int, C.POINTER(ConvDesc)], (C.c_size_t if q.endswith('workspace_bytes') else C.c_int)
        fns.append(f)
    d = ConvDesc()
    ref = C.byref(d)
    # the CU count the library plans with: bf16 1x1 1024 -> 1024 at 32 x 32, one sample -- 64 tiles of 16 K-steps go to the stream-K
    # kernel (whatever the switches of ENVS say), which asks for two 128 x 128 fp32 partial tiles per CU
    for name, v in zip(FIELDS, (1, 32, 32, 1024, 32, 32, 1024, 1, 1, 1, 0, 0, 0, 0, 0)):
        setattr(d, name, v)
    out = {'cus': fns[1](1, ref) / (2.0 * 128 * 128 * 4), 'slices': {}, 'rects_with_workspace': 0}
    seen = [set() for _ in QUERIES]                              # distinct values per column over the whole sweep
    for dtype in DTYPES:
        for k, stride, pad in KSP:
            for transposed in (0, 1):
                rows = []
                for vals in descriptors(k, stride, pad, transposed):
                    (d.N, d.Hi, d.Wi, d.Cin, d.Ho, d.Wo, d.Cout, d.KH, d.KW, d.stride, d.pad, d.transposed, d.in_act, d.out_act,
                     d.aux_mode) = vals
                    rows.append([f(dtype, ref) for f in fns])
                a = np.asarray(rows, dtype=np.int64)
                for c in range(a.shape[1]):
                    seen[c].update(np.unique(a[:, c]).tolist())
                out['rects_with_workspace'] += int(np.count_nonzero((a[:, 3] == 1) & (a[:, 1] != 0)))
                out['slices']['%s k%d s%d p%d %s' % (('f32', 'bf16')[dtype], k, stride, pad, 'DF'[1 - transposed])] = {
                    'n': int(a.shape[0]),
                    'sha': hashlib.sha256(np.ascontiguousarray(a[:, KIND_COLS]).tobytes()).hexdigest(),
                    'sha_ws': hashlib.sha256(np.ascontiguousarray(a[:, WS_COLS]).tobytes()).hexdigest(),
                    'distinct': [int(np.unique(a[:, c]).size) for c in range(a.shape[1])],
                    'nonzero': [round(float(np.count_nonzero(a[:, c])) / a.shape[0], 6) for c in range(a.shape[1])]}
    out['distinct'] = [len(v) for v in seen]
    return out


def run_all(lib_path):
    """{environment: sweep(lib_path)}, each environment in a child process of its own, side by side."""
    base = {k: v for k, v in os.environ.items() if not k.startswith('S2E_')}
    procs = {name: subprocess.Popen([sys.executable, os.path.abspath(__file__), '--lib', lib_path, '--env', name],
                                    env=dict(base, **extra), stdout=subprocess.PIPE) for name, extra in ENVS.items()}
    out = {}
    for name, p in procs.items():
        text, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError('the sweep of environment %r ended with status %d' % (name, p.returncode))
        out[name] = json.loads(text)
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', required=True)
    ap.add_argument('--env', choices=sorted(ENVS))
    ap.add_argument('--record')
    a = ap.parse_args()
    if a.env:                                                    # (the parent set the environment: see run_all)
        json.dump(sweep(a.lib), sys.stdout)
    else:
        res = run_all(a.lib)
        text = json.dumps({'queries': QUERIES, 'envs': res}, indent=1, sort_keys=True)
        if a.record:
            open(a.record, 'w').write(text + '\n')
        else:
            print(text)
