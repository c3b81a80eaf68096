#!/usr/bin/env python3
"""Digests of everything the norm / modulation kernels (csrc/norm_modulate.hip) compute, for an A/B of two source trees.

    python tools/norm_ab.py --root TREE --out a.json          # once per tree (each its own process)
    python tools/norm_ab.py --compare a.json b.json           # exit status 1 when a digest differs

Drives the public seg2eye_amd.ops functions of TREE with seeded inputs at the partial-slab test shapes and at the train
step's shapes (tools/mod_bwd_bench.py), both dtypes: in_stats with sums, instance_norm forward and backward,
spade_style_modulate, spade_style_fused with and without flags 8 and relay, and _modulate_grads with a pinned relay in the
staged BatchNorm form.  Every output tensor is recorded as a digest of its bytes: the kernels are deterministic, so two
trees that compute the same thing give the same digests.  colsum over more than one row block combines the blocks with
float atomics (order-dependent): there the entry is the error against the fp64 column sum and its bound M * 2^-24 (relative
to the column's sum of magnitudes) instead.
"""
import argparse
import hashlib
import json
import os
import sys
import types


def digest(t):
    """SHA-256 of a small tensor's bytes; of a large one, two 64-bit sums of its 32-bit words formed on the device (the plain
    sum and one weighted by position): exact integer arithmetic, equal for equal bits."""
    import torch
    t = t.detach().contiguous()
    if t.numel() * t.element_size() <= 1 << 22:
        return hashlib.sha256(t.cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:24]
    v = t.view(-1).view(torch.int32)
    a = b = 0
    for i in range(0, v.numel(), 1 << 24):
        c = v[i:i + (1 << 24)].to(torch.int64)
        k = torch.arange(i, i + c.numel(), device=c.device, dtype=torch.int64) % 1000003 + 1
        a += int(c.sum())
        b += int((c * k).sum())
    return '%016x%016x' % (a & (2 ** 64 - 1), b & (2 ** 64 - 1))


def run(root, out_path):
    sys.path.insert(0, os.path.abspath(root))
    import torch
    from seg2eye_amd import ops, _lib as L
    from seg2eye_amd.ops import spade as S
    from seg2eye_amd.ops.sink import GradSink
    from seg2eye_amd import distributed as sdist
    dev = torch.device('cuda', 0)
    gen = torch.Generator(device=dev)
    res = {}

    def rnd(shape, seed, dtype, scale=1.0, shift=0.0):
        gen.manual_seed(seed)
        return (torch.randn(*shape, device=dev, generator=gen) * scale + shift).to(dtype).contiguous()

    def put(key, *tensors):
        for i, t in enumerate(tensors):
            res['%s/%d' % (key, i)] = digest(t)

    test_shapes = [(2, 33, 40, 64), (2, 40, 50, 64), (2, 36, 36, 64), (2, 16, 16, 64)]          # (the last: a small map, one launch)
    step_shapes = [(8, 256, 256, 128), (8, 256, 256, 64), (8, 128, 128, 256), (8, 128, 128, 128), (8, 64, 64, 512)]
    in_shapes = [(16, 129, 129, 128), (16, 65, 65, 256), (32, 128, 128, 64), (32, 64, 64, 128), (3, 40, 50, 2064), (2, 33, 33, 64)]
    for dtype in (torch.bfloat16, torch.float32):
        dn = 'bf16' if dtype == torch.bfloat16 else 'fp32'
        for shape in test_shapes + step_shapes + in_shapes:
            n, h, w, c = shape
            key = '%s/%dx%dx%dx%d' % ((dn,) + shape)
            x = rnd(shape, 1, dtype, 1.5, 0.3)
            gy = rnd(shape, 2, dtype)
            stats, sums = ops.in_stats(x, return_sums=True)
            put(key + '/in_stats', stats, sums)
            for lrelu in (False, True):
                xg = x.clone().requires_grad_(True)
                y = ops.instance_norm(xg, lrelu)
                y.backward(gy)
                put(key + '/instance_norm%d' % lrelu, y, xg.grad)
            m = n * h * w
            cs = ops.colsum(gy)
            if m <= (256 // min(c // (8 if dtype == torch.bfloat16 else 4), 256)) * 64:
                put(key + '/colsum', cs)
            else:
                ref = gy.double().view(m, c)
                err = float(((cs.double() - ref.sum(0)).abs() / ref.abs().sum(0)).max())
                res[key + '/colsum/err_le_bound'] = bool(err <= m * 2.0 ** -24)
            if shape in in_shapes:
                continue
            gb = rnd((n, h, w, 2 * c), 3, dtype, 0.5)
            style = rnd((n, 2 * c), 4, torch.float32, 0.5)
            for lrelu in (False, True):
                for relay in (False, True):
                    xg, gbg, sg = x.clone().requires_grad_(True), gb.clone().requires_grad_(True), style.clone().requires_grad_(True)
                    y = ops.spade_style_modulate(xg, gbg, sg, stats, lrelu, relay=relay)
                    if relay:
                        y, xa = y
                        torch.autograd.backward([y, xa], [gy, rnd(shape, 5, dtype)])
                    else:
                        y.backward(gy)
                    put(key + '/modulate%d%d' % (lrelu, relay), y, xg.grad, gbg.grad, sg.grad)
            # the staged BatchNorm form with a relayed gradient that a queued job still has to read: dx apart from g_relay
            ctx = types.SimpleNamespace(off=None, dbig=None, batch=True, lrelu=True)
            bstats = stats[:1].expand(n, c, 2).contiguous()
            g_relay = rnd(shape, 6, dtype)
            keep = g_relay.clone()
            saved = (GradSink.is_pinned, sdist.sync_world_size, sdist.all_reduce_sum_)
            GradSink.is_pinned = staticmethod(lambda t: True)
            sdist.sync_world_size = lambda: 2
            sdist.all_reduce_sum_ = lambda t: t.mul_(2.0)
            try:
                dx, dgb, dstyle = S._modulate_grads(ctx, gy, g_relay, x, gb, None, style, bstats)
            finally:
                GradSink.is_pinned, sdist.sync_world_size, sdist.all_reduce_sum_ = saved
            assert torch.equal(g_relay, keep) and dx.data_ptr() != g_relay.data_ptr()
            put(key + '/staged_relay', dx, dgb, dstyle)
            # the fused launch (gamma-only backward; flags 8: x at half resolution, the quad dx), where the layer is one it takes
            if c % 64 or not ops.spade_fused_supported(x, 128, flags=L.SPADE_ANY_TILES):
                continue
            gen.manual_seed(7)
            lab = torch.randint(0, 4, (n, h, w), device=dev, generator=gen, dtype=torch.uint8)
            prm = [rnd((128, 4, 3, 3), 8, torch.float32, 0.3), rnd((128,), 9, torch.float32, 0.1), rnd((c, 128, 3, 3), 10, torch.float32, 0.03),
                   rnd((c,), 11, torch.float32, 0.1), rnd((c, 128, 3, 3), 12, torch.float32, 0.03), rnd((c,), 13, torch.float32, 0.1)]
            for fold in (False, True):
                if fold and (h % 2 or w % 2):
                    continue
                xin = rnd((n, h // 2, w // 2, c), 14, dtype, 1.1, -0.1) if fold else x
                st = ops.in_stats(xin)
                for relay in (False, True):
                    xs = xin.clone().requires_grad_(True)
                    p2 = [t.clone().requires_grad_(True) for t in prm]
                    sg = style.clone().requires_grad_(True)
                    y = ops.spade_style_fused(xs, lab, *p2, sg, st, True, relay=relay,
                                              flags=L.SPADE_ANY_TILES | L.SPADE_DENSE | (L.SPADE_X_HALF if fold else 0))
                    if relay:
                        y, xa = y
                        torch.autograd.backward([y, xa], [gy, rnd(tuple(xin.shape), 15, dtype)])
                    else:
                        y.backward(gy)
                    # (the conv weights' gradients are summed with atomics: not part of the comparison)
                    put(key + '/fused%d%d' % (fold, relay), y, xs.grad, sg.grad)
            torch.cuda.synchronize()
    with open(out_path, 'w') as f:
        json.dump(res, f, indent=0, sort_keys=True)
    print('norm_ab: %d entries -> %s' % (len(res), out_path))


def compare(a_path, b_path):
    a, b = json.load(open(a_path)), json.load(open(b_path))
    bad = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k) or a.get(k) is False]
    for k in bad:
        print('DIFFERS %s: %s | %s' % (k, a.get(k), b.get(k)))
    print('norm_ab: %d entries, %d differ' % (len(set(a) | set(b)), len(bad)))
    return 1 if bad else 0


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--out')
    ap.add_argument('--compare', nargs=2, metavar='JSON')
    args = ap.parse_args()
    sys.exit(compare(*args.compare) if args.compare else run(args.root, args.out) or 0)
