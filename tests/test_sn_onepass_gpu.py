"""The one-pass train-mode power iteration (csrc/spectral.hip: sn_onepass_kernel + sn_onepass_finalize_kernel) through SpectralBank,
against an fp64 power iteration in torch on the CPU -- the yardstick of test_fused_spectral_norm_conv_matches_torch.

One bank mixes the shapes at which the kernel takes another path: rows 1, 8, 33, 130 (no multiple of the 32-row sweep), 1024 (the
register strip's limit) and 1032 (one chunk beyond it); cols 9 (scalar loads), 36 and 40 (strip tails), 4608 + 8 (145 strips, the
last one a tail); 1 x 1, 2 x 2, 3 x 3 and 4 x 4 convs (sn_vidx), in both master layouts.

Accuracy: the error of the kernels this form replaced was recorded on the same inputs (tests/golden/sn_onepass_parent_err.npz, made by
running THIS FILE as a script in a checkout of the parent commit: profiles/sn_onepass.json has the command); the new kernels must stay
within 2 x that error plus one fp32 ulp (2^-23: u and v have unit norm, sigma's error is relative)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

if __name__ == '__main__':
    sys.path.insert(0, os.getcwd())

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sn_onepass_parent_err.npz')
SN_EPS = 1e-12
ULP = 2.0 ** -23
# (cin, cout, k): rows = cout, cols = cin * k * k
LAYERS = [(8, 1, 3), (1, 8, 3), (4, 33, 3), (40, 130, 1), (8, 130, 4), (16, 1024, 2), (64, 1032, 1), (4616, 16, 1), (8, 33, 3)]
SCALES = (1e-2, 1.0, 1e2)
ITERATIONS = (1, 2, 3, 8)
LAYOUTS = ('plain', 'channels_last')


def _make_net(scale, zero_layer=None):
    """The bank's convs on the CPU, each W scaled so that its spectral norm is `scale`; the same bits for every caller."""
    torch.manual_seed(11)
    convs = []
    for i, (cin, cout, k) in enumerate(LAYERS):
        c = torch.nn.utils.spectral_norm(torch.nn.Conv2d(cin, cout, k, bias=False))
        with torch.no_grad():
            w = c.weight_orig
            sigma = torch.linalg.matrix_norm(w.double().reshape(cout, -1), 2)
            w.mul_(float(scale / sigma))
            if i == zero_layer:
                w.zero_()
        convs.append(c)
    return torch.nn.Sequential(*convs)


@functools.lru_cache(maxsize=None)
def _reference(scale, iterations):
    """fp64 power iteration per layer: (u, v, sigma) after `iterations` train-mode iterations; computed once, never modified."""
    out = []
    for c in _make_net(scale):
        w = c.weight_orig.detach().double().reshape(c.weight_orig.shape[0], -1)
        u, v = c.weight_u.detach().double(), c.weight_v.detach().double()
        for _ in range(iterations):
            v = torch.nn.functional.normalize(w.t() @ u, dim=0, eps=SN_EPS)
            u = torch.nn.functional.normalize(w @ v, dim=0, eps=SN_EPS)
        out.append((u, v, float(u @ (w @ v))))
    return tuple(out)


def _bank_on_gpu(net, layout):
    from seg2eye_amd import spectral
    net = net.to(torch.device('cuda:0')).train()
    keep = None
    if layout == 'channels_last':
        from seg2eye_amd.optim import FlatAdam
        keep = FlatAdam(list(net.parameters()), lr=1e-3, channels_last=True)
        assert not net[5].weight_orig.is_contiguous() and not net[8].weight_orig.is_contiguous()     # (cin % 8 == 0, k > 1)
    return net, spectral.ensure_bank(net), keep


def _results(bank):
    torch.cuda.synchronize()
    uv, sg = bank.uv_arena.cpu(), bank.sigma.cpu()
    return [(uv[ou:ou + r], uv[ov:ov + c], float(sg[i])) for i, ((ou, ov), r, c) in enumerate(zip(bank.uv_off, bank.rows, bank.cols))]


def _errors(got, ref):
    """per layer: max abs error of u and of v, relative error of sigma"""
    return np.array([[float((u.double() - ur).abs().max()), float((v.double() - vr).abs().max()), abs(s - sr) / abs(sr)]
                     for (u, v, s), (ur, vr, sr) in zip(got, ref)])


def _key(layout, scale, iterations):
    return '%s_sigma%g_it%d' % (layout, scale, iterations)


@pytest.mark.gpu
@pytest.mark.parametrize('iterations', ITERATIONS)
@pytest.mark.parametrize('scale', SCALES)
@pytest.mark.parametrize('layout', LAYOUTS)
def test_one_pass_power_iteration_matches_fp64(layout, scale, iterations):
    net, bank, _keep = _bank_on_gpu(_make_net(scale), layout)
    state0 = bank.uv_arena.clone()
    with torch.no_grad():
        bank.step(True, iterations)
        first = _results(bank)
        assert int((bank.scratch != 0).sum()) == 0, 'the scratch is not zero after the call'
        uv1, sg1 = bank.uv_arena.clone(), bank.sigma.clone()
        bank.uv_arena.copy_(state0)
        bank.step(True, iterations)
        torch.cuda.synchronize()
        assert torch.equal(bank.uv_arena, uv1) and torch.equal(bank.sigma, sg1), 'two calls from identical state differ'
        assert int((bank.scratch != 0).sum()) == 0
    err = _errors(first, _reference(scale, iterations))
    parent = np.load(GOLDEN)[_key(layout, scale, iterations)]
    print('%s: per layer [u, v, sigma] errors\n%s\nparent max %s' % (_key(layout, scale, iterations), err, parent.max(axis=0)))
    assert np.isfinite(err).all()
    bound = 2.0 * parent.max(axis=0) + ULP
    assert (err.max(axis=0) <= bound).all(), (err.max(axis=0), bound)


@pytest.mark.gpu
@pytest.mark.parametrize('iterations', (1, 3))
def test_all_zero_layer_gives_zeros_and_leaves_the_others_alone(iterations):
    zero = 4
    _, bank, _ = _bank_on_gpu(_make_net(1.0), 'plain')
    _, bank_z, _ = _bank_on_gpu(_make_net(1.0, zero_layer=zero), 'plain')
    with torch.no_grad():
        bank.step(True, iterations)
        bank_z.step(True, iterations)
    want, got = _results(bank), _results(bank_z)
    for i, ((u, v, s), (uz, vz, sz)) in enumerate(zip(want, got)):
        assert torch.isfinite(uz).all() and torch.isfinite(vz).all() and np.isfinite(sz)
        if i == zero:
            assert not uz.any() and not vz.any() and sz == 0.0
        else:
            assert torch.equal(u, uz) and torch.equal(v, vz) and s == sz, i
    assert int((bank_z.scratch != 0).sum()) == 0


@pytest.mark.gpu
def test_eval_call_after_train_calls_leaves_u_v_and_gives_sigma():
    net, bank, _ = _bank_on_gpu(_make_net(1.0), 'channels_last')
    with torch.no_grad():
        bank.step(True, 2)
        bank.step(True, 1)
        trained = _results(bank)
        uv = bank.uv_arena.clone()
        net.eval()
        bank.step(False)
        got = _results(bank)
    assert torch.equal(bank.uv_arena, uv) and int((bank.scratch != 0).sum()) == 0
    for c, (u, v, s_train), (_, _, s) in zip(_make_net(1.0), trained, got):
        w = c.weight_orig.detach().double().reshape(u.numel(), -1)
        want = float(u.double() @ (w @ v.double()))
        # sigma = u . W v of the SAME u, v in both modes: fp32 sums of up to 4616 terms against fp64
        assert abs(s - want) <= 1e-5 * abs(want) and abs(s - s_train) <= 1e-5 * abs(want), (s, s_train, want)


if __name__ == '__main__':
    # record the errors of the checkout in the current directory:  python <this file> --record OUT.npz
    assert sys.argv[1] == '--record', sys.argv
    rec = {}
    for layout in LAYOUTS:
        for scale in SCALES:
            for iterations in ITERATIONS:
                _, bank, _keep = _bank_on_gpu(_make_net(scale), layout)
                with torch.no_grad():
                    bank.step(True, iterations)
                rec[_key(layout, scale, iterations)] = _errors(_results(bank), _reference(scale, iterations))
                print(_key(layout, scale, iterations), rec[_key(layout, scale, iterations)].max(axis=0), flush=True)
    np.savez(sys.argv[2], **rec)
