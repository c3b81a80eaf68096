#!/usr/bin/env python3
"""What the validation panels of the visualiser cost.  Not part of bench.py.

n = 8, 320 x 256 sources, 640 x 400 targets, 4 style images, 200 x 320 cells, `fake` in fp32 and in bf16:

  launches_us   the three launches of `s2e_sidebyside_u8` alone, on tensors that already are on the device: HIP events, median of
                `--reps` with min and max
  op_us         `ops.sidebyside_u8` as a caller sees it: the conversions to uint8, the buffer, the zeroed caption rows, the
                launches and the 4-byte status read
  bytes         the algorithmic bytes: every source read once, the panels written once, and their time at 8 TB/s

One JSON line on stdout (and in --out).  Run it under a `timeout`; nothing here retries a failing step.

    timeout -k 10 150 python tools/bench_sidebyside.py --out profiles/sidebyside.json"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def events_us(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return {'median': round(ts[len(ts) // 2], 1), 'min': round(ts[0], 1), 'max': round(ts[-1], 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    from seg2eye_amd import _lib as L, ops
    from seg2eye_amd.ops.core import _p, _stream
    n, H, W, Ht, Wt, h, w, ns = 8, 320, 256, 640, 400, 320, 200, 4
    g = torch.Generator().manual_seed(0)
    label = torch.randint(0, 4, (n, H, W), generator=g, dtype=torch.uint8).cuda()
    target = torch.randint(0, 256, (n, Ht, Wt), generator=g, dtype=torch.uint8).cuda()
    style = (torch.rand(n, ns, H, W, generator=g) * 2 - 1).cuda()
    fake32 = (torch.rand(n, H, W, generator=g) * 2 - 1).cuda()
    lib = L.lib()
    out = torch.zeros(n, 1, h + 60, 5 * w, dtype=torch.uint8, device='cuda')
    status = torch.zeros(1, dtype=torch.int32, device='cuda')
    ws = torch.empty(lib.s2e_sidebyside_ws_bytes(n, h, w), dtype=torch.uint8, device='cuda')
    res = {'shape': dict(n=n, H=H, W=W, Ht=Ht, Wt=Wt, h=h, w=w, ns=ns), 'reps': args.reps}
    for name, fake in (('fp32', fake32), ('bf16', fake32.bfloat16())):
        def launches():
            L.check(lib.s2e_sidebyside_u8(L.S2E_BF16 if name == 'bf16' else L.S2E_F32, _p(fake), _p(style), ns, _p(label), _p(target), n, H, W,
                                          Ht, Wt, h, w, 5 * w, (h + 60) * 5 * w, _p(ws), _p(status), _p(out), _stream()), 's2e_sidebyside_u8')

        def op():
            ops.sidebyside_u8(label, fake, target, style.unsqueeze(2))
        for _ in range(5):
            launches()
            op()
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        read = label.numel() + target.numel() + style.numel() * 4 + fake.numel() * fake.element_size()
        res[name] = {'launches_us': events_us(launches, args.reps), 'op_us': events_us(op, args.reps),
                     'bytes': {'read_once': read, 'written': n * h * 5 * w, 'us_at_8TBps': round((read + n * h * 5 * w) / 8e6, 2)}}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
