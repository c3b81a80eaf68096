#!/usr/bin/env python3
"""Run job tables through the library's three weight-gradient size queries and record the answers.

    python tests/golden/make_wgrad_plan.py --lib <libseg2eye_hip.so> --record tests/golden/wgrad_plan.json
    python tests/golden/make_wgrad_plan.py --lib <libseg2eye_hip.so> --env NAME     (one environment: tables on stdin, JSON on stdout)

The fixture tests/golden/wgrad_plan.json is recorded with --lib pointing at a build of the commit BEFORE a change of the planners (a
scratch checkout of it), never at the code under test; tests/test_wgrad_plan_host.py asks the tree's own library the same questions and
compares number by number.  No GPU needed; the children use plain ctypes (the queries never follow a job's pointers).

Queries: s2e_conv2d_wgrad_multi_workspace_bytes on every table of tests/_wgrad_tables_child.py, every prefix of each (prefixes move the
chunk boundaries of all three families) and 200 seeded random tables of 1 to 120 jobs from POOL, some jobs sharing dw;
s2e_wgrad_c8_batch_workspace_bytes on 100 seeded random tables; s2e_wgrad_batch_workspace_bytes (it takes no jobs and depends on the CU
count the library plans with: `cus` records it, 256 without a device and on an MI355X).  `kinds` is s2e_conv2d_wgrad_multi_kind of
every POOL shape.

The library reads its switches once per process, so every environment is a child process (--env) started with every S2E_* variable
removed and the environment's one switch set.  The c8_batch and wgrad_batch answers and `cus` depend on none of these switches: the
fixture holds them once, and fixture() refuses a library whose environments disagree on them.

check() refuses a degenerate grid: per environment at least three distinct kinds and 50 distinct non-zero sizes of the multi query
(the c8_batch tables add some 90 more, the same in every environment).  Two kinds of environment cannot give that much by construction
and are held to what they can: S2E_DETERMINISTIC=1 turns the flat and c8 kernels off, so its kinds are -1 and 0 alone; with
S2E_WGRAD_PARTIAL=0 (or S2E_WGRAD_MULTI_WGS=1, one split per job) no generic job asks for workspace and a call's size is its c8
sections', at most 30 values for 120 jobs -- there the multi query must still give ten.
"""
import argparse
import ctypes as C
import json
import os
import random
import subprocess
import sys

ENVS = {'default': {}, 'partial0': {'S2E_WGRAD_PARTIAL': '0'}, 'partial2': {'S2E_WGRAD_PARTIAL': '2'},
        'multi_wgs1': {'S2E_WGRAD_MULTI_WGS': '1'}, 'multi_wgs100000': {'S2E_WGRAD_MULTI_WGS': '100000'},
        'deterministic': {'S2E_DETERMINISTIC': '1'}, 'flat0': {'S2E_WGRAD_FLAT': '0'}, 'flat_all': {'S2E_WGRAD_FLAT': '62'},
        'c8_0': {'S2E_CONV_C8': '0'}, 'c8w_wgs37': {'S2E_C8W_WGS': '37'}}
S2E_BF16 = 1
# (n, hi, wi, cin, cout, k, stride, pad, in_act).  Kinds with the default switches: 0 generic, 4 / 5 flat, 6 c8, -1 not a job of the call
POOL = [
    (2, 16, 16, 32, 64, 3, 2, 1, 0), (3, 9, 11, 64, 72, 3, 2, 1, 0), (2, 17, 13, 16, 40, 4, 2, 2, 0), (1, 8, 8, 128, 136, 1, 1, 0, 0),    # generic
    (16, 128, 128, 64, 128, 3, 2, 1, 0), (8, 64, 64, 128, 256, 3, 2, 1, 0), (4, 32, 32, 1024, 128, 1, 1, 0, 0), (4, 64, 64, 64, 64, 1, 1, 0, 0),
    (2, 8, 8, 128, 256, 3, 1, 1, 0), (2, 16, 16, 64, 64, 1, 1, 0, 1), (4, 64, 64, 64, 128, 4, 2, 2, 1),                                   # (an input activation: never flat)
    (1, 8, 8, 64, 64, 1, 1, 0, 0), (1, 8, 8, 64, 64, 3, 1, 1, 0), (2, 16, 16, 64, 64, 3, 2, 1, 0),                                        # flat 1 .. 3 (off by default: generic)
    (1, 8, 8, 64, 64, 4, 1, 2, 0), (2, 9, 9, 64, 64, 4, 1, 2, 0), (1, 9, 9, 64, 128, 4, 2, 2, 0), (16, 33, 33, 64, 128, 4, 2, 2, 0),      # flat 4, 5
    (16, 129, 129, 64, 128, 4, 2, 2, 0),
    (16, 128, 128, 8, 64, 4, 2, 2, 0), (1, 2, 2, 8, 64, 4, 2, 2, 0), (2, 33, 47, 8, 64, 4, 2, 2, 0), (1, 1, 40, 8, 64, 4, 2, 2, 0),       # c8
    (3, 17, 9, 8, 64, 4, 2, 2, 0), (1, 64, 64, 8, 64, 4, 2, 2, 0), (2, 20, 20, 8, 64, 4, 2, 2, 0),
    (1, 300, 300, 8, 64, 4, 2, 2, 0),                                                                                                     # (too wide for c8: generic)
    (2, 16, 16, 3, 64, 3, 1, 1, 0), (8, 64, 64, 128, 128, 3, 1, 1, 0),                                                                    # not jobs of the call
]
N_GOOD = len(POOL) - 2
FIELDS = ('N', 'Hi', 'Wi', 'Cin', 'Ho', 'Wo', 'Cout', 'KH', 'KW', 'stride', 'pad', 'transposed', 'in_act', 'out_act', 'aux_mode')
C8_MAPS = [(16, 16), (32, 32), (64, 64), (48, 80), (32, 16), (16, 48), (64, 128), (128, 128), (256, 256), (24, 40), (96, 160), (80, 48),
           (17, 33), (8, 8), (20, 100)]                            # (the last three: slabs less than 80 % inside the map)


class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_int) for n in FIELDS]


class MultiJob(C.Structure):
    _fields_ = [('x', C.c_void_p), ('gy', C.c_void_p), ('dw', C.c_void_p), ('dbias', C.c_void_p), ('d', ConvDesc)]


class C8Job(C.Structure):
    _fields_ = [('x', C.c_void_p), ('gy', C.c_void_p), ('dw_oihw', C.c_void_p), ('dbias', C.c_void_p), ('H', C.c_int), ('W', C.c_int),
                ('ncls', C.c_int), ('rect_list', C.c_void_p), ('rect_count', C.c_void_p)]


def tables():
    """{'names': [...], 'multi': [[(n, hi, wi, cin, cout, k, s, p, in_act, dw id), ...], ...], 'c8_batch': [[N, [(H, W, ncls, rects), ...]], ...]}"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
    import _wgrad_tables_child as T
    names, multi = [], []
    for name, t in T.TABLES.items():
        ids = {}
        jobs = [tuple(j[:8]) + (0, ids.setdefault(j[9], len(ids))) for j in t]
        for n in range(1, len(jobs) + 1):
            names.append(name if n == len(jobs) else '%s[:%d]' % (name, n))
            multi.append(jobs[:n])
    rng = random.Random(20260)
    for i in range(200):
        n = rng.randint(1, 120)
        bad = i % 20 == 19                                       # one table in twenty holds a shape the call refuses: the query says 0
        jobs = [POOL[rng.randrange(len(POOL) if bad else N_GOOD)] + (k,) for k in range(n)]
        for k in range(1, n):                                    # some jobs write the dw of an earlier job of the same shape
            if rng.random() < 0.15:
                same = [m for m in range(k) if jobs[m][:9] == jobs[k][:9]]
                if same:
                    jobs[k] = jobs[k][:9] + (jobs[rng.choice(same)][9],)
        names.append('random%03d' % i)
        multi.append(jobs)
    c8 = []
    for i in range(100):
        maps = C8_MAPS if i % 10 == 9 else C8_MAPS[:-3]          # (one table in ten may hold a map that is none of the kernel's: the query says 0)
        jobs = []
        for _ in range(rng.randint(1, 40)):
            h, w = rng.choice(maps)
            jobs.append((h, w, rng.randint(1, 8), int((h | w) % 16 == 0 and rng.random() < 0.3)))
        c8.append([rng.choice((1, 2, 8, 16)), jobs])
    return {'names': names, 'multi': multi, 'c8_batch': c8}


def answer(lib_path, tabs):
    lib = C.CDLL(lib_path)
    lib.s2e_conv2d_workspace_bytes.argtypes, lib.s2e_conv2d_workspace_bytes.restype = [C.c_int, C.POINTER(ConvDesc)], C.c_size_t
    lib.s2e_conv2d_wgrad_multi_kind.argtypes, lib.s2e_conv2d_wgrad_multi_kind.restype = [C.c_int, C.POINTER(ConvDesc)], C.c_int
    lib.s2e_conv2d_wgrad_multi_workspace_bytes.argtypes = [C.c_int, C.POINTER(MultiJob), C.c_int]
    lib.s2e_conv2d_wgrad_multi_workspace_bytes.restype = C.c_size_t
    lib.s2e_wgrad_c8_batch_workspace_bytes.argtypes, lib.s2e_wgrad_c8_batch_workspace_bytes.restype = [C.c_int, C.POINTER(C8Job), C.c_int], C.c_size_t
    lib.s2e_wgrad_batch_workspace_bytes.argtypes, lib.s2e_wgrad_batch_workspace_bytes.restype = [], C.c_size_t

    def desc(j):
        n, hi, wi, cin, cout, k, s, p, act = j[:9]
        return ConvDesc(n, hi, wi, cin, (hi + 2 * p - k) // s + 1, (wi + 2 * p - k) // s + 1, cout, k, k, s, p, 0, act, 0, 0)
    # the CU count the library plans with (tests/golden/make_conv_routing.py): a stream-K shape asks for two 128 x 128 fp32 tiles per CU
    out = {'cus': lib.s2e_conv2d_workspace_bytes(S2E_BF16, C.byref(ConvDesc(1, 32, 32, 1024, 32, 32, 1024, 1, 1, 1, 0, 0, 0, 0, 0))) / (2.0 * 128 * 128 * 4),
           'kinds': [int(lib.s2e_conv2d_wgrad_multi_kind(S2E_BF16, C.byref(desc(j)))) for j in POOL], 'multi': [], 'c8_batch': []}
    for jobs in tabs['multi']:
        arr = (MultiJob * len(jobs))()
        for a, j in zip(arr, jobs):                              # (addresses nobody reads: a job's dw id picks its range)
            a.x, a.gy, a.dw, a.dbias, a.d = 0x1000, 0x2000, 0x100000 * (1 + j[9]), None, desc(j)
        out['multi'].append(int(lib.s2e_conv2d_wgrad_multi_workspace_bytes(S2E_BF16, arr, len(jobs))))
    for n, jobs in tabs['c8_batch']:
        arr = (C8Job * len(jobs))()
        for a, (h, w, ncls, rects) in zip(arr, jobs):
            a.x, a.gy, a.dw_oihw, a.H, a.W, a.ncls = 0x1000, 0x2000, 0x3000, h, w, ncls
            a.rect_list = a.rect_count = 0x4000 if rects else None
        out['c8_batch'].append(int(lib.s2e_wgrad_c8_batch_workspace_bytes(n, arr, len(jobs))))
    out['wgrad_batch'] = int(lib.s2e_wgrad_batch_workspace_bytes())
    return out


SHARED = ('cus', 'c8_batch', 'wgrad_batch')                     # answers that depend on none of ENVS' switches


def fixture(names, res):
    """what --record writes: the SHARED answers once, per environment its kinds and multi sizes"""
    for r in res.values():
        assert all(r[k] == res['default'][k] for k in SHARED), 'an environment-independent answer differs between environments'
    out = {k: res['default'][k] for k in SHARED}
    out.update(names=names, envs={name: {'kinds': r['kinds'], 'multi': r['multi']} for name, r in res.items()})
    return out


def check(fix):
    """the recorded grid is not degenerate (see the module docstring)"""
    assert 0 in fix['c8_batch'] and len({v for v in fix['c8_batch'] if v}) >= 50
    for name, r in fix['envs'].items():
        kinds = set(r['kinds'])
        multi = {v for v in r['multi'] if v}
        assert (kinds == {-1, 0}) if name == 'deterministic' else len(kinds) >= 3, (name, sorted(kinds))
        assert len(multi) >= (10 if name in ('partial0', 'multi_wgs1') else 50), (name, len(multi))
        assert 0 in r['multi'], name                             # (the refused tables)


def run_all(lib_path):
    """(tables, {environment: answer(lib_path, tables)}), each environment in a child process of its own, side by side."""
    tabs = tables()
    text = json.dumps(tabs).encode()
    base = {k: v for k, v in os.environ.items() if not k.startswith('S2E_')}
    procs = {name: subprocess.Popen([sys.executable, os.path.abspath(__file__), '--lib', lib_path, '--env', name], env=dict(base, **extra),
                                    stdin=subprocess.PIPE, stdout=subprocess.PIPE) for name, extra in ENVS.items()}
    out = {}
    for name, p in procs.items():
        got, _ = p.communicate(text)
        if p.returncode != 0:
            raise RuntimeError('the queries of environment %r ended with status %d' % (name, p.returncode))
        out[name] = json.loads(got)
    return tabs, out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', required=True)
    ap.add_argument('--env', choices=sorted(ENVS))
    ap.add_argument('--record')
    a = ap.parse_args()
    if a.env:                                                    # (the parent set the environment: see run_all)
        json.dump(answer(a.lib, json.load(sys.stdin)), sys.stdout)
    else:
        tabs, res = run_all(a.lib)
        fix = fixture(tabs['names'], res)
        check(fix)
        row = lambda v: json.dumps(v, sort_keys=True, separators=(',', ':'))          # one line per key and per environment
        text = '{\n' + ',\n'.join('"%s":%s' % (k, row(fix[k])) for k in SHARED + ('names',)) + ',\n"envs":{\n' + ',\n'.join(
            '"%s":%s' % (name, row(fix['envs'][name])) for name in sorted(fix['envs'])) + '\n}}'
        if a.record:
            open(a.record, 'w').write(text + '\n')
        else:
            print(text)
