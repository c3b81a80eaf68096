"""The segmenter's boundary-aware terms on the GPU: the distance maps and the band against the integers of the
restatement (tests/_seg_loss_ref.py), the fused loss and its gradient against the fp64 restatement, and the tool's loop with the terms on.

Distance maps.  Every case compares integers with ==: rint(phi^2) outside a class, rint((1 - phi)^2) inside, the band byte; phi itself
within one fp32 ulp of the fp32 value of the definition (zero ulps seen everywhere).

Loss.  The rule of DESIGN 3.21, unchanged: each term, the loss and the fp32 gradient within 4x the distance at which the restatement
evaluated in fp32 numpy stands from its fp64 value, never less than one fp32 ulp of the value (a gradient: of its largest element); a bf16
gradient within one bf16 step of the rounded restatement, per element.  Everything else is ==.  Measured figures: DESIGN 3.22."""
import functools

import numpy as np
import pytest
import torch

import _seg_loss_ref as SL
import _segment_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DT = {'fp32': torch.float32, 'bf16': torch.bfloat16}
KINDS = ['ellipse', 'iid', 'fill', 'absent', 'corner', 'checker', 'sprinkled', 'differ']


def _ulp32(v):
    return float(np.spacing(np.float32(abs(float(v)))))


def _ulps(a, b):
    """Per element, how many fp32 values lie between two fp32 arrays (+0 and -0 count as equal)."""
    def ordered(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i >= 0, i, -(i & 0x7fffffff))
    return np.abs(ordered(a) - ordered(b))


def _bf16_steps(a, b):
    def ordered(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i >= 0, i, -(i & 0x7fff))
    return (ordered(a) - ordered(b)).abs()


# ------------------------------------------------------------------------------------------------ distance maps
def _check_dist(lab, ncls, radius, brute=True):
    from seg2eye_amd import ops
    m = (SL.sq_dists_brute if brute else SL.sq_dists_scipy)(lab, ncls)
    want_phi, want_band = SL.maps_from_sq(m, lab, ncls, radius, np.float32)
    t = torch.from_numpy(lab).to(DEV)
    phi, band = ops.seg_dist_maps(t, ncls, radius)
    assert phi.dtype == torch.float32 and tuple(phi.shape) == lab.shape + (ncls,) and band.dtype == torch.uint8 and tuple(band.shape) == lab.shape
    got = phi.cpu().numpy()
    own = np.arange(ncls)[None, None, None, :] == lab[..., None]
    none = m == SL.NONE
    r = np.where(own, 1.0 - got.astype(np.float64), got.astype(np.float64))
    back = np.where(none, SL.NONE, np.rint(r * r).astype(np.int64))
    assert np.array_equal(back, m)                                                             # the integers
    assert not got[none].any() and not np.signbit(got[none]).any()                              # +0 where the set is empty
    assert not np.signbit(got[got == 0]).any()                                                  # a pixel that touches another class: +0
    ulps = int(_ulps(got, want_phi).max())
    assert np.array_equal(band.cpu().numpy(), want_band)
    again = ops.seg_dist_maps(t, ncls, radius)
    assert torch.equal(again[0], phi) and torch.equal(again[1], band)                           # two calls: the same bits
    print('dist %s ncls %d radius %d: largest m %d, phi at most %d ulp from the definition, band share %.3f'
          % (lab.shape, ncls, radius, int(m.max()), ulps, float(want_band.mean())))
    assert ulps <= 1
    return phi, band


DIST_SHAPES = [(1, 1, 1), (1, 1, 9), (1, 9, 1), (2, 5, 7), (2, 24, 16), (1, 40, 67), (1, 3, 300), (1, 300, 3), (2, 64, 40)]


@pytest.mark.parametrize('kind', ['ellipse', 'iid'])
@pytest.mark.parametrize('shape', DIST_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_distance_maps_shapes(shape, kind):
    """One pixel, one row, one column, a row across a wave (67), a row and a column longer than a workgroup (300), two images."""
    _check_dist(SL.label_maps(kind, shape, 4, seed=sum(shape)), 4, 2)


@pytest.mark.parametrize('shape', [(2, 24, 16), (1, 3, 300), (1, 300, 3)], ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('kind', KINDS)
def test_distance_maps_label_maps(kind, shape):
    """Every pixel a boundary, a class that fills an image, an absent class, one far pixel (the longest reach along both axes), a
    checkerboard, ignored pixels, and two images of a batch that must not see each other."""
    _check_dist(SL.label_maps(kind, shape, 4, seed=5), 4, 2)


@pytest.mark.parametrize('radius', [0, 1, 2, 5])
@pytest.mark.parametrize('ncls', [1, 3, 4, 16])
def test_distance_maps_classes_and_radii(ncls, radius):
    lab = SL.label_maps('iid' if ncls == 16 else 'sprinkled', (2, 24, 16), ncls, seed=ncls + radius)
    if ncls == 16:
        lab[0, :12] = 7                                                                         # a block of one class: distances beyond 1
    phi, band = _check_dist(lab, ncls, radius)
    if radius == 0:
        assert not band.any()


def test_distance_maps_without_a_band_and_through_the_scalar_stores():
    """band = NULL at the C ABI, and a phi of four classes that is not 16-byte aligned: the same bits as the op's."""
    from seg2eye_amd import _lib as L, ops
    lab = torch.from_numpy(SL.label_maps('sprinkled', (2, 24, 16), 4, seed=8)).to(DEV)
    phi, _ = ops.seg_dist_maps(lab, 4, 2)
    ws = torch.empty(int(L.call.s2e_seg_dist_workspace_bytes(2, 24, 16, 4)) // 4, dtype=torch.int32, device=DEV)
    buf = torch.full((phi.numel() + 1,), -7.0, device=DEV)
    off = buf[1:].view(phi.shape)
    assert off.data_ptr() % 16 == 4
    for out in (torch.full_like(phi, -7.0), off):
        L.call.s2e_seg_dist_maps(lab.data_ptr(), 2, 24, 16, 4, 2, out.data_ptr(), None, ws.data_ptr(), ws.numel() * 4, torch.cuda.current_stream().cuda_stream)
        assert torch.equal(out, phi)
    assert float(buf[0]) == -7.0


def test_distance_maps_large_against_scipy():
    _check_dist(SL.label_maps('ellipse', (2, 320, 200), 4, seed=2), 4, 2, brute=False)


# ------------------------------------------------------------------------------------------------ the fused loss
def _labels(kind, shape, ncls, seed):
    n, h, w = shape
    rng = np.random.RandomState(seed)
    if kind == 'eyes':
        return R.eyes(n, h, w, ncls, seed)
    if kind == 'iid':
        return rng.randint(0, ncls, shape).astype(np.uint8)
    if kind == 'all255':
        return np.full(shape, 255, dtype=np.uint8)
    if kind == 'holes':                                          # the last image wholly ignored, the one before lacks the last class
        lab = rng.randint(0, ncls, shape).astype(np.uint8)
        lab[0, 0, :3] = 255
        lab[n - 1] = 255
        lab[n - 2][lab[n - 2] == ncls - 1] = 0
        return lab
    lab = rng.randint(0, ncls, shape).astype(np.uint8)          # 'sprinkled'
    hit = rng.rand(*shape) < 0.2
    lab[hit] = rng.randint(ncls, 255, shape).astype(np.uint8)[hit]
    lab.reshape(-1)[0] = 255
    return lab


def _logits(kind, shape, dtype, ncls, seed, lab=None):
    """-> a CPU tensor of `dtype` (N, H, W, C); channels ncls.. hold NaN, +inf, -inf and 1e30 in turn."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(*shape, generator=g)
    if kind == 'big':                                            # |z| ~ 80: without the maximum subtracted, exp overflows
        z = 80.0 * torch.sign(torch.randn(*shape, generator=g)) + z
    elif kind == 'right':                                        # a near-perfect prediction: the label's logit stands 12 above the others
        z = z + 12.0 * torch.nn.functional.one_hot(torch.from_numpy(np.minimum(lab, ncls - 1)).long(), shape[3]).float()
    for c in range(ncls, shape[3]):
        z[..., c] = (float('nan'), float('inf'), float('-inf'), 1e30)[(c - ncls) % 4]
    return z.to(dtype)


def _weights(kind, ncls):
    if kind == 'uniform':
        return np.ones(ncls, dtype=np.float32)
    return np.array([(0.5, 1.0, 2.0, 4.0)[c % 4] for c in range(ncls)], dtype=np.float32)


FULL = (0.7, 1.3, 0.9, 20.0)                                     # lambda_ce, lambda_dice, lambda_surface, edge_alpha


def _run(z, lab, w, phi, band, lambdas=FULL, scale=None):
    from seg2eye_amd import ops
    zg = z.to(DEV).requires_grad_(True)
    dev = lambda a: None if a is None else torch.from_numpy(a).to(DEV)
    loss, terms = ops.seg_loss(zg, dev(lab), dev(w), dev(phi), dev(band), *lambdas)
    (loss if scale is None else loss * scale).backward()
    assert loss.dim() == 0 and loss.dtype == torch.float32 and tuple(terms.shape) == (3,) and terms.dtype == torch.float32
    assert not terms.requires_grad and zg.grad.dtype == z.dtype
    return loss.detach().cpu(), terms.cpu(), zg.grad.detach().cpu()


def _inputs(shape, dname, labels, logits, weights, seed):
    n, h, w_, c, ncls = shape
    lab = _labels(labels, (n, h, w_), ncls, seed + 1)
    z = _logits(logits, (n, h, w_, c), DT[dname], ncls, seed, lab)
    phi, band = SL.dist_maps(lab, ncls, 2)
    return z, lab, _weights(weights, ncls), phi, band


def _check_loss(shape, dname, labels='eyes', logits='normal', weights='graded', lambdas=FULL, seed=0, report=None):
    ncls = shape[4]
    z, lab, w, phi, band = _inputs(shape, dname, labels, logits, weights, seed)
    zf = z.float().numpy()
    l64, t64, g64 = SL.loss(zf, lab, w, phi, band, *lambdas, ncls)
    l32, t32, g32 = SL.loss(zf, lab, w, phi, band, *lambdas, ncls, np.float32)
    loss, terms, grad = _run(z, lab, w, phi, band, lambdas)
    tag = 'loss %s %s %s/%s/%s' % (shape, dname, labels, logits, weights)
    failed = []
    for name, got, v64, v32 in [('loss', loss, l64, l32)] + [(k, terms[i], t64[i], t32[i]) for i, k in enumerate(('CE', 'Dice', 'Surface'))]:
        d = abs(float(v32) - float(v64))
        bound = max(4 * d, _ulp32(v64))
        err = abs(float(got) - float(v64))
        print('%s: %s %.9g  |fp32 restatement - fp64| %.3g  bound %.3g  |kernel - fp64| %.3g' % (tag, name, float(v64), d, bound, err))
        if report is not None:
            report[name] = (d, bound, err)
        if not (np.isfinite(float(got)) and err <= bound):
            failed.append((name, float(v64), d, bound, err))
    assert abs(float(loss) - sum(l * float(t) for l, t in zip(lambdas[:3], terms))) <= 4 * 2.0 ** -23 * max(abs(float(loss)), sum(l * abs(float(t)) for l, t in zip(lambdas[:3], terms)))
    ignored = torch.from_numpy(lab >= ncls)
    assert not grad[ignored].ne(0).any() and not torch.signbit(grad[ignored]).any()             # +0, every channel
    assert not grad[..., ncls:].ne(0).any() and not torch.signbit(grad[..., ncls:]).any()       # +0 behind ncls
    if dname == 'fp32':
        d_g = float(np.abs(g32.astype(np.float64) - g64).max())
        b_g = max(4 * d_g, _ulp32(np.abs(g64).max()))
        e_g = float(np.abs(grad.numpy().astype(np.float64) - g64).max())
        print('   gradient: max |fp32 restatement - fp64| %.3g  bound %.3g  max |kernel - fp64| %.3g' % (d_g, b_g, e_g))
        if not e_g <= b_g:
            failed.append(('gradient', float(np.abs(g64).max()), d_g, b_g, e_g))
    else:
        steps = _bf16_steps(grad[..., :ncls], torch.from_numpy(g64[..., :ncls]).to(torch.bfloat16))
        print('   bf16 gradient: %d of %d elements one step from the rounded restatement, largest distance %d steps'
              % (int((steps == 1).sum()), steps.numel(), int(steps.max())))
        if int(steps.max()) > 1:
            failed.append(('bf16 gradient', int(steps.max())))
    assert not failed, failed
    return z, lab, w, phi, band, loss, terms, grad


LOSS_SHAPES = [((1, 1, 1, 4, 4), 'fp32'), ((1, 1, 1, 4, 4), 'bf16'), ((2, 5, 7, 4, 4), 'fp32'), ((2, 5, 7, 4, 4), 'bf16'), ((2, 5, 7, 8, 4), 'bf16'),
               ((2, 24, 16, 16, 16), 'fp32'), ((2, 24, 16, 16, 16), 'bf16'), ((2, 64, 40, 4, 4), 'fp32'), ((2, 64, 40, 4, 4), 'bf16'),
               ((3, 6, 5, 4, 4), 'fp32'), ((3, 6, 5, 4, 4), 'bf16')]


@pytest.mark.parametrize('shape,dname', LOSS_SHAPES, ids=lambda v: v if isinstance(v, str) else 'x'.join(map(str, v)))
def test_loss_shapes(shape, dname):
    """Every load form (pitch 4, pitch 8, any), one pixel, several workgroups per image, pad channels full of NaN / inf, sixteen classes,
    an image wholly ignored and one that lacks a class; two calls and planted pad channels give the same bits."""
    labels = 'holes' if shape[0] == 3 else 'iid' if shape[1] == 1 else 'eyes' if shape[4] == 4 else 'sprinkled'
    z, lab, w, phi, band, loss, terms, grad = _check_loss(shape, dname, labels, seed=sum(shape))
    again = _run(z, lab, w, phi, band)
    assert torch.equal(again[0], loss) and torch.equal(again[1], terms) and torch.equal(again[2], grad)
    clean = z.clone()
    clean[..., shape[4]:] = 0
    planted = _run(clean, lab, w, phi, band)
    assert torch.equal(planted[0], loss) and torch.equal(planted[1], terms) and torch.equal(planted[2], grad)
    if labels == 'holes':
        assert not grad[2].ne(0).any()


@pytest.mark.parametrize('dname', ['fp32', 'bf16'])
@pytest.mark.parametrize('lambdas', [(1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0), (1.0, 0.0, 0.0, 20.0), (1.0, 1.0, 0.05, 20.0)],
                         ids=['ce', 'dice', 'surface', 'edge', 'recipe'])
@pytest.mark.parametrize('logits', ['normal', 'big'])
def test_loss_terms_one_by_one(logits, lambdas, dname):
    _check_loss((2, 24, 16, 4, 4), dname, 'sprinkled', logits, 'graded' if lambdas[0] else 'uniform', lambdas, seed=11)


@pytest.mark.parametrize('dname', ['fp32', 'bf16'])
def test_loss_of_a_near_perfect_prediction(dname):
    """The label's logit 12 above the others: Dice = 1 - (a ratio near 1).  The rule holds here because the ratio is formed in fp64 from
    fp64 sums in the kernel, where the fp32 restatement cancels in fp32."""
    _check_loss((2, 24, 16, 4, 4), dname, 'eyes', 'right', 'uniform', (1.0, 1.0, 0.05, 20.0), seed=13)


@pytest.mark.parametrize('dname', ['fp32', 'bf16'])
def test_loss_of_nothing_is_zero(dname):
    z, lab, w, phi, band = _inputs((2, 5, 7, 4, 4), dname, 'all255', 'normal', 'graded', 3)
    loss, terms, grad = _run(z, lab, w, phi, band)
    assert float(loss) == 0.0 and not terms.ne(0).any() and not grad.ne(0).any() and not torch.signbit(grad).any()


@pytest.mark.parametrize('dname', ['fp32', 'bf16'])
def test_loss_gradient_scales_with_the_upstream_factor(dname):
    """loss * 3 -> gradient * 3: the factor multiplies the finished per-element sum, one more rounding; 4 units of the format's epsilon."""
    z, lab, w, phi, band = _inputs((2, 5, 7, 4, 4), dname, 'sprinkled', 'normal', 'graded', 5)
    l1, t1, g1 = _run(z, lab, w, phi, band)
    l3, t3, g3 = _run(z, lab, w, phi, band, scale=3.0)
    assert torch.equal(l1, l3) and torch.equal(t1, t3)
    eps = 2.0 ** -23 if dname == 'fp32' else 2.0 ** -8
    assert torch.allclose(g3.double(), 3 * g1.double(), rtol=4 * eps, atol=0) and g1.ne(0).any()


def test_loss_unaligned_logits_and_phi_take_the_scalar_loads():
    """A bf16 (.., 4) tensor 2 bytes off an 8-byte boundary and a phi 4 bytes off a 16-byte one: the other load forms, the same bits."""
    from seg2eye_amd import ops
    z, lab, w, phi, band = _inputs((2, 5, 7, 4, 4), 'bf16', 'sprinkled', 'normal', 'graded', 8)
    lab, w, band = (torch.from_numpy(a).to(DEV) for a in (lab, w, band))
    zbuf = torch.zeros(z.numel() + 1, dtype=torch.bfloat16, device=DEV)
    zoff = zbuf[1:].view(z.shape)
    zoff.copy_(z)
    pbuf = torch.zeros(phi.size + 1, dtype=torch.float32, device=DEV)
    poff = pbuf[1:].view(phi.shape)
    poff.copy_(torch.from_numpy(phi))
    assert zoff.data_ptr() % 8 == 2 and poff.data_ptr() % 16 == 4
    out = []
    for zz, pp in ((z.to(DEV), torch.from_numpy(phi).to(DEV)), (zoff, poff)):
        zz = zz.detach().requires_grad_(True)
        loss, terms = ops.seg_loss(zz, lab, w, pp, band, *FULL)
        loss.backward()
        out.append((loss.detach(), terms, zz.grad))
    assert all(torch.equal(a, b) for a, b in zip(*out)) and out[0][2].ne(0).any()


@pytest.mark.parametrize('dname', ['fp32', 'bf16'])
def test_loss_terms_that_are_off_read_nothing(dname):
    """phi = None with lambda_surface = 0 and band = None with edge_alpha = 0: the bits of the call that passes them -- also when what
    it passes is full of NaN."""
    z, lab, w, phi, band = _inputs((2, 5, 7, 4, 4), dname, 'sprinkled', 'normal', 'graded', 9)
    for lambdas, drop in (((0.7, 1.3, 0.0, 20.0), 'phi'), ((0.7, 1.3, 0.9, 0.0), 'band'), ((1.0, 1.0, 0.0, 0.0), 'both')):
        full = _run(z, lab, w, phi, band, lambdas)
        none = _run(z, lab, w, None if drop in ('phi', 'both') else phi, None if drop in ('band', 'both') else band, lambdas)
        junk = _run(z, lab, w, np.full_like(phi, np.nan) if drop in ('phi', 'both') else phi, np.full_like(band, 255) if drop in ('band', 'both') else band, lambdas)
        for other in (none, junk):
            assert all(torch.equal(a, b) for a, b in zip(full, other)), (lambdas, drop)
        if drop != 'band':
            assert float(full[1][2]) == 0.0


@pytest.mark.parametrize('dname', ['fp32', 'bf16'])
def test_loss_with_the_terms_off_is_the_cross_entropy(dname):
    """edge_alpha = 0, lambda = (1, 0, 0): within the cross-entropy's rule of _segment_ref's cross-entropy, and of ops.seg_cross_entropy."""
    from seg2eye_amd import ops
    z, lab, w, phi, band = _inputs((2, 24, 16, 4, 4), dname, 'sprinkled', 'normal', 'graded', 10)
    zf = z.float().numpy()
    l64, g64 = R.ce(zf, lab, w, 4)
    l32, _ = R.ce(zf, lab, w, 4, np.float32)
    loss, terms, grad = _run(z, lab, w, None, None, (1.0, 0.0, 0.0, 0.0))
    bound = max(4 * abs(float(l32) - float(l64)), _ulp32(l64))
    print('terms off %s: CE %.9g bound %.3g |kernel - fp64| %.3g' % (dname, float(l64), bound, abs(float(loss) - float(l64))))
    assert abs(float(loss) - float(l64)) <= bound and float(terms[0]) == float(loss)
    ce = ops.seg_cross_entropy(z.to(DEV), torch.from_numpy(lab).to(DEV), torch.from_numpy(w).to(DEV))
    assert abs(float(ce) - float(loss)) <= 2 * _ulp32(l64)


# ------------------------------------------------------------------------------------------------ end to end
E2E = dict(nsf=8, seg_hw=(64, 40), compute_dtype='fp32', batchSize=6, niter=10, lr=2e-3, seed=7, no_flip=True)
RECIPE = dict(lambda_ce=1.0, lambda_dice=1.0, lambda_surface=0.05, edge_alpha=20.0, edge_radius=2)


@functools.lru_cache(maxsize=None)
def _store():
    return R.learnable_store()


def _net():
    from seg2eye_amd.segment import build_network, seg_options
    opt = seg_options(nsf=8, compute_dtype='fp32', seg_hw=(64, 40))
    net = build_network(opt, DEV)
    sd = R.hash_state(net, seed=0, dtype=torch.float64)
    with torch.no_grad():
        for k, v in net.state_dict().items():
            v.copy_(sd[k].float())
    return net, sd


def test_train_with_all_three_terms_end_to_end():
    """30 steps on 18 labelled frames at 64 x 40, nsf 8, fp32, from the hash-filled weights, with --edge_alpha 20 --edge_radius 2
    --lambda_dice 1 --lambda_surface 0.05.  The fp64 restatement of the same run satisfies both conditions with room to spare
    (DESIGN 3.22); its first step, at the same weights, is made here and compared."""
    from seg2eye_amd import segment
    store, _ = _store()
    net, sd = _net()
    opt = segment.seg_options(**E2E, **RECIPE)
    _, _, first = SL.train_restated(sd, store, (64, 40), 1, 6, 2e-3, 7, (1.0, 1.0, 0.05, 20.0), 2, steps=1)
    before = segment.evaluate(net, store, 'validation', opt, DEV, verbose=False)
    net, hist = segment.train_segmenter(store, opt, net=net, device=DEV, save=False, verbose=False)
    loss, terms, after = hist['loss'], np.array(hist['terms']), hist['scores'][-1]
    print('end to end, terms on: loss first five %.4f last five %.4f; CE %.4f -> %.4f, Dice %.4f -> %.4f, Surface %.4f -> %.4f; validation mIoU %.4f -> %.4f'
          % (np.mean(loss[:5]), np.mean(loss[-5:]), terms[:5, 0].mean(), terms[-5:, 0].mean(), terms[:5, 1].mean(), terms[-5:, 1].mean(),
             terms[:5, 2].mean(), terms[-5:, 2].mean(), before['miou/validation'], after['miou/validation']))
    assert len(loss) == 30 and terms.shape == (30, 3) and len(hist['scores']) == 10
    assert np.isfinite(loss).all() and np.isfinite(terms).all()
    assert np.mean(loss[-5:]) < np.mean(loss[:5])
    assert after['miou/validation'] > before['miou/validation']
    print('   first step [CE, Dice, Surface]: %s, the restatement %s' % (terms[0].tolist(), first[0]))
    np.testing.assert_allclose(terms[0], first[0], rtol=2e-3, atol=2e-4)                       # at step 1 both runs hold the same weights
