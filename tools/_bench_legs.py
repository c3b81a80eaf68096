"""What the tools/bench_{ssim,msssim,region,ffl}.py share: the launch count of a torch composition, the alternating HIP-event timing
loop, and the JSON file."""
import json
import os

import torch


def count_kernels(fn):
    """Device kernels one call of fn launches, by torch.profiler; None when it cannot tell."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA') and 'memcpy' not in e.name.lower()
                and 'memset' not in e.name.lower())
        return n or None
    except Exception:                                        # noqa: BLE001 -- a count, not a measurement: the timings stand without it
        return None


def time_legs(legs, rounds, launches):
    """legs: {name: callable}.  After a warm-up (code objects loaded, allocator blocks cached, clocks up) the legs are alternated round
    by round, each `launches` back-to-back calls between two HIP events.  -> {name: {'us_median', 'us_min', 'us_max'}}: the median over
    the rounds of the per-call mean, and its spread."""
    for f in legs.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, f in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / launches)
    out = {}
    for k, xs in ms.items():
        xs = sorted(xs)
        out[k] = {'us_median': round(1e3 * xs[len(xs) // 2], 2), 'us_min': round(1e3 * xs[0], 2), 'us_max': round(1e3 * xs[-1], 2)}
    return out


def write_json(out, path):
    """`out` as indented JSON to `path` (None: nowhere), its directory made."""
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')
