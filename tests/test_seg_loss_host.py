"""The segmenter's boundary-aware terms without a GPU: the restatement (tests/_seg_loss_ref.py) against scipy and fp64
autograd, the new symbols' declarations, the refused calls of the three entry points, the workspace sizes, the ops' ValueErrors, and the
tool's loop with the new flags on a stub network with the restatements in the ops' place."""
import os
import re

import numpy as np
import pytest
import torch

import _seg_loss_ref as SL
import _segment_ref as R
from _quality_harness import check_error_table

F32, BF16, BAD = 0, 1, 7
P = 4096                                                      # a dummy non-null pointer: must never reach a kernel
BIG = 1 << 33                                                 # a workspace size that is never short
ARG, UNSUPPORTED = -1, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('s2e_seg_dist_workspace_bytes', 's2e_seg_dist_maps', 's2e_seg_loss_workspace_bytes', 's2e_seg_loss_fwd', 's2e_seg_loss_bwd')


# ------------------------------------------------------------------------------------------------ the restatement alone
@pytest.mark.parametrize('shape', [(2, 5, 7), (2, 24, 16), (1, 64, 40)], ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('kind', ['ellipse', 'iid', 'fill', 'absent', 'corner', 'sprinkled', 'differ'])
def test_brute_force_distances_are_scipys(kind, shape):
    """The O((HW)^2) evaluation of the definition == scipy's exact transform: the integers, and phi in fp64 against Kervadec's
    one_hot2dist as the public recipes write it, with a maximum difference of 0."""
    lab = SL.label_maps(kind, shape, 4, seed=3)
    m = SL.sq_dists_brute(lab, 4)
    assert np.array_equal(m, SL.sq_dists_scipy(lab, 4))
    phi, band = SL.maps_from_sq(m, lab, 4, 2, np.float64)
    assert np.array_equal(phi, SL.phi_scipy_form(lab, 4)) and not np.signbit(phi[phi == 0]).any()
    assert band.dtype == np.uint8 and not band[lab >= 4].any()
    assert not SL.maps_from_sq(m, lab, 4, 0)[1].any()                                         # radius 0: nobody is within 0 of another class
    if kind == 'ellipse' and shape == (1, 64, 40):
        assert 0.1 < band.mean() < 0.5                                                         # neither empty nor everything
    if kind == 'fill':
        assert not phi[0].any() and not band[0].any()                                          # one class fills image 0
    if kind == 'differ':
        n, h, w = shape
        assert m[0, h - 1, w - 1, 3] == (h - 1) ** 2 + (w - 1) ** 2 and (n == 1 or m[1, 0, 0, 0] == (h - 1) ** 2 + (w - 1) ** 2)


def test_fp32_square_roots_give_the_integers_back():
    m = np.arange(0, 2 * 1023 * 1023 + 1, dtype=np.int64)
    s = np.sqrt(m.astype(np.float32)).astype(np.float64)
    assert np.array_equal(np.rint(s * s).astype(np.int64), m)
    inside = (1.0 - (np.float32(1) - np.sqrt(m.astype(np.float32))).astype(np.float64))       # 1 - phi of an inside pixel
    assert np.array_equal(np.rint(inside * inside).astype(np.int64), m)


def _case(seed=0):
    """The case of the closed form's derivation: ignored pixels, a wholly ignored image, an image lacking a class."""
    g = torch.Generator().manual_seed(seed)
    N, H, W, C = 3, 6, 5, 4
    z = torch.randn(N, H, W, C, generator=g, dtype=torch.float64)
    lab = torch.randint(0, 4, (N, H, W), generator=g, dtype=torch.uint8)
    lab[0, 0, :3] = 255
    lab[2] = 255
    lab[1][lab[1] == 3] = 0
    w = torch.tensor([1.0, 2.0, 0.5, 3.0], dtype=torch.float64)
    phi, band = SL.dist_maps(lab.numpy(), 4, 2, np.float64, brute=True)
    return z, lab, w, phi, band


@pytest.mark.parametrize('lambdas', [(0.7, 1.3, 0.9, 20.0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (1, 0, 0, 5.0)])
def test_closed_form_gradient_is_autograds(lambdas):
    z, lab, w, phi, band = _case()
    zt = z.clone().requires_grad_(True)
    want, terms = SL.loss_torch(zt, lab, w, torch.from_numpy(phi), torch.from_numpy(band), *lambdas)
    dwant, = torch.autograd.grad(want, zt)
    total, t, grad = SL.loss(z.numpy(), lab.numpy(), w.numpy(), phi, band, *lambdas, 4)
    assert abs(float(total) - float(want.detach())) < 1e-14 and np.abs(t - terms.detach().numpy()).max() < 1e-14
    assert np.abs(grad - dwant.numpy()).max() < 1e-15
    assert not grad[lab.numpy() >= 4].any() and not grad[2].any()
    if lambdas == (1, 0, 0, 0):                                                                 # the existing loss
        l0, g0 = R.ce(z.numpy(), lab.numpy(), w.numpy(), 4)
        assert abs(float(total) - float(l0)) < 1e-15 and np.abs(grad - g0).max() < 1e-16
    t32 = SL.loss(z.numpy(), lab.numpy(), w.numpy(), phi, band, *lambdas, 4, np.float32)
    assert t32[0].dtype == np.float32 and t32[2].dtype == np.float32 and abs(float(t32[0]) - float(total)) < 1e-5


@pytest.mark.parametrize('scale', [1.0, 80.0])
def test_pairwise_gradient_is_the_issues_plain_form(scale):
    """SL.loss writes a_c - sum_k a_k p_k as sum_k p_k (a_c - a_k).  Here the issue's plain form is written out on its own, from `saved`'s
    definitions, and autograd is taken too -- on N(0, 1) logits and on logits near 80 rounded to bf16, where classes tie and the softmax is
    one-hot.  All three agree to the fp64 rounding of the plain form's own cancellation: a few eps of the largest |a| + CE factor."""
    z, lab, w, phi, band = _case(2)
    z = (z * scale).to(torch.bfloat16).to(torch.float64)
    lam_ce, lam_dice, lam_surf, alpha = 0.7, 1.3, 0.9, 20.0
    _, _, grad = SL.loss(z.numpy(), lab.numpy(), w.numpy(), phi, band, lam_ce, lam_dice, lam_surf, alpha, 4)
    zn, l = z.numpy(), lab.numpy()
    cnt = l < 4
    g = (np.arange(4) == np.where(cnt, l, 0)[..., None]) & cnt[..., None]
    p = np.exp(zn - zn.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    pm = p * cnt[..., None]
    I, U, G = (pm * g).sum((1, 2)), (pm + g).sum((1, 2)), g.sum((1, 2)).astype(np.float64)
    v = np.where(G > 0, 1 / np.maximum(G, 1) ** 2, 0.0)
    A, D = (v * I).sum(1), (v * U).sum(1)
    has = cnt.reshape(3, -1).any(1)
    ncnt, D1 = has.sum(), np.where(has, D, 1.0)
    kI = np.where(has[:, None], -(lam_dice / ncnt) * 2 * v / D1[:, None], 0.0)
    kU = np.where(has[:, None], (lam_dice / ncnt) * 2 * A[:, None] * v / D1[:, None] ** 2, 0.0)
    a = kI[:, None, None, :] * g + kU[:, None, None, :] + lam_surf * phi / (cnt.sum() * 4)
    wl = np.where(cnt, w.numpy()[np.where(cnt, l, 0)], 0.0)
    ce = lam_ce * wl * (1 + alpha * band) / wl.sum()
    plain = cnt[..., None] * (p * (a - (a * p).sum(-1, keepdims=True)) + ce[..., None] * (p - g))
    room = 8 * np.finfo(np.float64).eps * (np.abs(a).max() + ce.max())
    assert np.abs(grad - plain).max() <= room
    zt = z.clone().requires_grad_(True)
    want, _ = SL.loss_torch(zt, lab, w, torch.from_numpy(phi), torch.from_numpy(band), lam_ce, lam_dice, lam_surf, alpha)
    # (autograd reaches the same numbers through a chain of a few dozen rounded steps -- logsumexp, the masked sums, 2 A / D -- not one
    # subtraction: eight times the room)
    assert np.abs(grad - torch.autograd.grad(want, zt)[0].numpy()).max() <= 8 * room


def test_restated_loss_pad_channels_and_no_counted_pixel():
    z, lab, w, phi, band = _case(1)
    padded = np.concatenate([z.numpy(), np.full(z.shape, np.nan)], -1)
    a = SL.loss(padded, lab.numpy(), w.numpy(), phi, band, 1, 1, 1, 3, 4)
    b = SL.loss(z.numpy(), lab.numpy(), w.numpy(), phi, band, 1, 1, 1, 3, 4)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2][..., :4], b[2]) and not a[2][..., 4:].any()
    none = SL.loss(z.numpy(), np.full(lab.shape, 255, np.uint8), w.numpy(), phi, band, 1, 1, 1, 3, 4)
    assert none[0] == 0 and not none[1].any() and not none[2].any()


# ------------------------------------------------------------------------------------------------ declared, exported, bound, built
def test_new_symbols_are_declared_exported_and_bound():
    from seg2eye_amd import _lib, build
    header = open(os.path.join(ROOT, 'include', 'seg2eye_hip.h')).read()
    for name in NEW:
        assert re.search(r'\b%s\(' % name, header), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name), name
    assert 'seg_loss.hip' in build.SOURCES and os.path.exists(os.path.join(build.CSRC, 'seg_loss.hip'))
    assert _lib.SIGNATURES['s2e_seg_dist_maps'][0] == _lib.STATUS and _lib.SIGNATURES['s2e_seg_loss_workspace_bytes'][0] == _lib.SIZE


# ------------------------------------------------------------------------------------------------ refused calls
def _dist(label=P, N=2, H=8, W=8, ncls=4, radius=2, phi=P, band=P, ws=P, wsb=BIG):
    return (label, N, H, W, ncls, radius, phi, band, ws, wsb, None)


def _fwd(dtype=F32, x=P, label=P, w=P, phi=P, band=P, N=2, H=8, W=8, C=4, ncls=4, lce=1.0, ldice=1.0, lsurf=1.0, alpha=1.0, loss=P, terms=P,
         saved=P, ws=P, wsb=BIG):
    return (dtype, x, label, w, phi, band, N, H, W, C, ncls, lce, ldice, lsurf, alpha, loss, terms, saved, ws, wsb, None)


def _bwd(dtype=F32, x=P, label=P, w=P, phi=P, band=P, saved=P, g=P, N=2, H=8, W=8, C=4, ncls=4, lce=1.0, lsurf=1.0, alpha=1.0, dx=P):
    return (dtype, x, label, w, phi, band, saved, g, N, H, W, C, ncls, lce, lsurf, alpha, dx, None)


D = 's2e_seg_dist_maps'
DIST = [
    (_dist(label=None), ARG, D + ': bad argument'),
    (_dist(phi=None), ARG, D + ': bad argument'),
    (_dist(ws=None), ARG, D + ': bad argument'),
    (_dist(wsb=2047), ARG, D + ': workspace of 2047 bytes, needs 2048'),
    (_dist(wsb=2047, N=0), ARG, D + ': N=0 H=8 W=8 (every size must be at least 1)'),         # a refused shape needs no bytes
    (_dist(ws=P + 2), ARG, D + ': workspace and phi must be 4-byte aligned'),
    (_dist(phi=P + 1, N=0), ARG, D + ': workspace and phi must be 4-byte aligned'),            # the buffers before the sizes
    (_dist(N=0, ncls=17), ARG, D + ': N=0 H=8 W=8 (every size must be at least 1)'),           # the sizes before the class count
    (_dist(H=-1), ARG, D + ': N=2 H=-1 W=8 (every size must be at least 1)'),
    (_dist(W=0), ARG, D + ': N=2 H=8 W=0 (every size must be at least 1)'),
    (_dist(radius=-1, ncls=0), ARG, D + ': radius=-1 (0 or more)'),
    (_dist(ncls=0), UNSUPPORTED, D + ': ncls=0 (1 to 16 classes)'),
    (_dist(ncls=17, H=2000), UNSUPPORTED, D + ': ncls=17 (1 to 16 classes)'),                  # the class count before the side limit
    (_dist(H=1025), UNSUPPORTED, D + ': H=1025 W=8 (each at most 1024)'),
    (_dist(W=1025, N=65536), UNSUPPORTED, D + ': H=8 W=1025 (each at most 1024)'),             # the side limit before the batch limit
    (_dist(N=65536, H=1, W=1), UNSUPPORTED, D + ': N=65536 H=1 W=1 is beyond the launch limits (N <= 65535, N H W < 2^31)'),
    (_dist(N=2048, H=1024, W=1024), UNSUPPORTED, D + ': N=2048 H=1024 W=1024 is beyond the launch limits (N <= 65535, N H W < 2^31)'),
    (_dist(N=512, H=1024, W=1024), UNSUPPORTED, D + ': N=512 H=1024 W=1024 ncls=4 is beyond the index limit (N H W ncls < 2^31)'),
]


def _shared(name, make):
    """The rows forward and backward refuse alike, in the order the header states them."""
    return [
        (make(x=None), ARG, name + ': bad argument'),
        (make(label=None), ARG, name + ': bad argument'),
        (make(w=None), ARG, name + ': bad argument'),
        (make(saved=None), ARG, name + ': bad argument'),
        (make(dtype=BAD, N=0), ARG, name + ': bad dtype 7'),
        (make(N=0, ncls=17), ARG, name + ': N=0 H=8 W=8 (every size must be at least 1)'),
        (make(W=-1), ARG, name + ': N=2 H=8 W=-1 (every size must be at least 1)'),
        (make(ncls=0), UNSUPPORTED, name + ': ncls=0 (1 to 16 classes)'),
        (make(ncls=17, C=16), UNSUPPORTED, name + ': ncls=17 (1 to 16 classes)'),
        (make(C=3), ARG, name + ': channel pitch C=3 is below ncls=4'),
        (make(N=32768, H=65536, W=1), UNSUPPORTED, name + ': N=32768 H=65536 W=1 is beyond the index limit (N H W <= 2^31 - 1)'),
        (make(N=65536, H=1, W=1, lce=-1.0), UNSUPPORTED, name + ': N=65536 H=1 W=1 is beyond the launch limits (N <= 65535, N H W < 2^31)'),
        (make(lce=-1.0, phi=None), ARG, name + ': lambda_ce=-1 lambda_dice=%s lambda_surf=1 edge_alpha=1 (finite and not negative)'),
        (make(lsurf=float('nan')), ARG, name + ': lambda_ce=1 lambda_dice=%s lambda_surf=nan edge_alpha=1 (finite and not negative)'),
        (make(alpha=float('inf')), ARG, name + ': lambda_ce=1 lambda_dice=%s lambda_surf=1 edge_alpha=inf (finite and not negative)'),
        (make(phi=None, band=None), ARG, name + ': lambda_surf=1 without phi'),                # phi before the band
        (make(band=None), ARG, name + ': edge_alpha=1 without band'),
        (make(phi=None, lsurf=0.0, band=None, alpha=0.5), ARG, name + ': edge_alpha=0.5 without band'),
    ]


def _fill(rows, dice):
    return [(a, c, t % dice if '%s' in t else t) for a, c, t in rows]


FWD = _fill(_shared('s2e_seg_loss_fwd', lambda **k: _fwd(**k)), '1') + [
    (_fwd(loss=None), ARG, 's2e_seg_loss_fwd: bad argument'),
    (_fwd(terms=None), ARG, 's2e_seg_loss_fwd: bad argument'),
    (_fwd(ldice=-0.5), ARG, 's2e_seg_loss_fwd: lambda_ce=1 lambda_dice=-0.5 lambda_surf=1 edge_alpha=1 (finite and not negative)'),
    (_fwd(ws=None), ARG, 's2e_seg_loss_fwd: workspace of 0 bytes, needs 560 (8-byte aligned)'),
    (_fwd(wsb=559), ARG, 's2e_seg_loss_fwd: workspace of 559 bytes, needs 560 (8-byte aligned)'),
    (_fwd(ws=P + 4), ARG, 's2e_seg_loss_fwd: workspace of %d bytes, needs 560 (8-byte aligned)' % BIG),
    (_fwd(band=None, ws=None), ARG, 's2e_seg_loss_fwd: edge_alpha=1 without band'),           # the workspace last
]
BWD = _fill(_shared('s2e_seg_loss_bwd', lambda **k: _bwd(**k)), '0') + [
    (_bwd(g=None), ARG, 's2e_seg_loss_bwd: bad argument'),
    (_bwd(dx=None), ARG, 's2e_seg_loss_bwd: bad argument'),
]


def test_seg_loss_entry_points_reject_bad_calls_before_any_launch():
    """The refusals of include/seg2eye_hip.h with their messages, and which check wins.  Host-only: with a GPU visible the test skips
    itself, so that a dummy pointer can never reach a kernel (as test_segment_entry_points_reject_bad_calls_before_any_launch does)."""
    if torch.cuda.is_available():
        pytest.skip('dummy pointers: host-only by construction')
    from seg2eye_amd import _lib
    for name, table in ((D, DIST), ('s2e_seg_loss_fwd', FWD), ('s2e_seg_loss_bwd', BWD)):
        check_error_table(name, table)
    with pytest.raises(_lib.Seg2EyeHipError, match='s2e_seg_dist_maps failed'):
        _lib.call.s2e_seg_dist_maps(*DIST[0][0])


def test_workspace_sizes():
    """Distance maps: one uint32 per (pixel, class).  Loss: K = 4 + 3 ncls doubles per workgroup -- ceil(H W / 256) per image, at most
    512 / N (at least one) -- and K + 3 per image for the fold.  0 for a shape the entry point refuses."""
    from seg2eye_amd import _lib
    q = _lib.lib().s2e_seg_dist_workspace_bytes
    assert [q(1, 1, 1, 1), q(2, 8, 8, 4), q(16, 320, 200, 4), q(2, 64, 40, 16)] == [4, 2048, 16 * 320 * 200 * 16, 2 * 64 * 40 * 64]
    assert [q(0, 8, 8, 4), q(2, 8, 8, 0), q(2, 8, 8, 17), q(1, 1025, 8, 4), q(1, 8, 1025, 4), q(65536, 1, 1, 1), q(512, 1024, 1024, 4)] == [0] * 7
    q = _lib.lib().s2e_seg_loss_workspace_bytes

    def want(N, HW, ncls):
        K = 4 + 3 * ncls
        blocks = min(-(-HW // 256), max(512 // N, 1))
        return 8 * (N * blocks * K + N * (K + 3))
    for N, H, W, ncls in ((1, 1, 1, 4), (2, 8, 8, 4), (16, 320, 200, 4), (1, 320, 200, 4), (3, 64, 40, 16), (600, 40, 40, 3)):
        assert q(N, H, W, ncls) == want(N, H * W, ncls), (N, H, W, ncls)
    assert q(2, 8, 8, 4) == 560 and q(16, 320, 200, 4) == 8 * (16 * 32 * 16 + 16 * 19)
    assert [q(0, 8, 8, 4), q(2, 8, 8, 0), q(2, 8, 8, 17), q(65536, 1, 1, 1), q(32768, 65536, 1, 4)] == [0] * 5


# ------------------------------------------------------------------------------------------------ the ops before the device check
def test_ops_raise_value_errors_before_the_device_check():
    from seg2eye_amd import _lib, ops
    z, lab = torch.zeros(2, 4, 6, 4), torch.zeros(2, 4, 6, dtype=torch.uint8)
    phi, band = torch.zeros(2, 4, 6, 4), torch.zeros(2, 4, 6, dtype=torch.uint8)
    with pytest.raises(ValueError, match='uint8 label map'):
        ops.seg_dist_maps(lab.long(), 4)
    with pytest.raises(ValueError, match=r'\(N, H, W\) with H, W <= 1024'):
        ops.seg_dist_maps(lab[0], 4)
    with pytest.raises(ValueError, match=r'\(N, H, W\) with H, W <= 1024'):
        ops.seg_dist_maps(torch.zeros(1, 1025, 2, dtype=torch.uint8), 4)
    with pytest.raises(ValueError, match='1 to 16 classes'):
        ops.seg_dist_maps(lab, 17)
    with pytest.raises(ValueError, match='radius = -1'):
        ops.seg_dist_maps(lab, 4, -1)
    with pytest.raises(ValueError, match='bf16 or fp32 logits'):
        ops.seg_loss(z.double(), lab.long())                                                  # the logits' dtype first
    with pytest.raises(ValueError, match='uint8 label map'):
        ops.seg_loss(z, lab.long(), phi=phi[0])                                               # dtypes before shapes
    with pytest.raises(ValueError, match='class weights'):
        ops.seg_loss(z, lab, torch.ones(4, dtype=torch.float64))
    with pytest.raises(ValueError, match='phi: fp32'):
        ops.seg_loss(z, lab, phi=phi.double(), lambda_surface=1.0)
    with pytest.raises(ValueError, match='band: uint8'):
        ops.seg_loss(z, lab, band=band.float(), edge_alpha=1.0)
    with pytest.raises(ValueError, match='one N x H x W'):
        ops.seg_loss(z, lab[:, :3])
    with pytest.raises(ValueError, match=r'phi: \(2, 4, 6, 4\) expected'):
        ops.seg_loss(z, lab, phi=phi[..., :3], lambda_surface=1.0)
    with pytest.raises(ValueError, match=r'phi: \(2, 4, 6, 3\) expected'):
        ops.seg_loss(z, lab, torch.ones(3), phi=phi, lambda_surface=1.0)                      # three classes by the weights
    with pytest.raises(ValueError, match=r'band: \(2, 4, 6\) expected'):
        ops.seg_loss(z, lab, band=band[:1], edge_alpha=1.0)
    with pytest.raises(ValueError, match='lambda_dice = -1.0'):
        ops.seg_loss(z, lab, lambda_dice=-1.0)
    with pytest.raises(ValueError, match='edge_alpha = nan'):
        ops.seg_loss(z, lab, band=band, edge_alpha=float('nan'))
    with pytest.raises(ValueError, match='lambda_surface = 0.5 needs phi'):
        ops.seg_loss(z, lab, band=band, lambda_surface=0.5)
    with pytest.raises(ValueError, match='edge_alpha = 20 needs band'):
        ops.seg_loss(z, lab, phi=phi, edge_alpha=20.0)
    # valid CPU tensors: the device check is what refuses them
    with pytest.raises(_lib.Seg2EyeHipError, match='GPU only'):
        ops.seg_dist_maps(lab, 4)
    with pytest.raises(_lib.Seg2EyeHipError, match='GPU only'):
        ops.seg_loss(z, lab, None, phi, band, 1.0, 1.0, 0.05, 20.0)
    with pytest.raises(_lib.Seg2EyeHipError, match='GPU only'):
        ops.seg_loss(z.bfloat16(), lab, lambda_dice=1.0)                                      # Dice alone needs neither map


# ------------------------------------------------------------------------------------------------ the tool
class _StubNet(torch.nn.Module):
    """Logits from the image alone, one learnable sharpness: the class whose grey level (tests/_segment_ref.py: GREY) is nearest."""

    def __init__(self):
        super().__init__()
        self.k = torch.nn.Parameter(torch.tensor(1.0))

    def forward(self, x):
        grey = torch.tensor(R.GREY / 255.0 * 2 - 1, dtype=torch.float32)
        return -self.k * (x.permute(0, 2, 3, 1) - grey) ** 2


class _StubAdam:
    def __init__(self, params, lr, betas):
        self.opt = torch.optim.Adam(params, lr=lr, betas=betas)

    def zero_grad(self):
        self.opt.zero_grad()

    def step(self):
        self.opt.step()


@pytest.fixture()
def restated_tool(monkeypatch):
    """The ops train_segmenter calls replaced by the restatements on CPU tensors, every call counted."""
    from seg2eye_amd import optim
    from seg2eye_amd.ops import preprocess, segment
    calls = {'seg_cross_entropy': 0, 'seg_dist_maps': 0, 'seg_loss': 0, 'args': []}

    def resize_bicubic_u8(frames, Ho, Wo, flip, return_u8=False):
        return R.host_input(frames.numpy(), (Ho, Wo))[:, 0]

    def resize_nearest_u8(labels, Ho, Wo, flip):
        return torch.from_numpy(np.ascontiguousarray(R.host_labels(labels.numpy(), (Ho, Wo))))

    def seg_cross_entropy(logits, label, weights=None):
        calls['seg_cross_entropy'] += 1
        return R.ce_torch(logits, label, weights)

    def seg_dist_maps(label, ncls, radius=2):
        calls['seg_dist_maps'] += 1
        calls['args'].append((ncls, radius))
        phi, band = SL.dist_maps(label.numpy(), ncls, radius)
        return torch.from_numpy(phi), torch.from_numpy(band)

    def seg_loss(logits, label, weights=None, phi=None, band=None, lambda_ce=1., lambda_dice=0., lambda_surface=0., edge_alpha=0.):
        calls['seg_loss'] += 1
        calls['args'].append((phi is None, band is None, lambda_ce, lambda_dice, lambda_surface, edge_alpha))
        total, terms = SL.loss_torch(logits, label, weights, phi, band, lambda_ce, lambda_dice, lambda_surface, edge_alpha)
        return total, terms.detach()
    monkeypatch.setattr(preprocess, 'resize_bicubic_u8', resize_bicubic_u8)
    monkeypatch.setattr(preprocess, 'resize_nearest_u8', resize_nearest_u8)
    monkeypatch.setattr(segment, 'seg_cross_entropy', seg_cross_entropy)
    monkeypatch.setattr(segment, 'seg_dist_maps', seg_dist_maps)
    monkeypatch.setattr(segment, 'seg_loss', seg_loss)
    monkeypatch.setattr(optim, 'FlatAdam', _StubAdam)
    return calls


def _tiny_store():
    store, _ = R.learnable_store(H=64, W=40)
    return {'train': store['train']}                                                          # (no validation split: evaluate is not under test)


def test_default_flags_train_with_the_cross_entropy_alone(restated_tool):
    from seg2eye_amd.segment import seg_options, train_segmenter
    opt = seg_options(seg_hw=(32, 24), batchSize=6, niter=2, no_flip=True, lr=1e-2)
    assert (opt.lambda_ce, opt.lambda_dice, opt.lambda_surface, opt.edge_alpha, opt.edge_radius) == (1.0, 0.0, 0.0, 0.0, 2)
    _, hist = train_segmenter(_tiny_store(), opt, net=_StubNet(), device='cpu', save=False, verbose=False)
    assert restated_tool['seg_cross_entropy'] == 6 and restated_tool['seg_loss'] == 0 and restated_tool['seg_dist_maps'] == 0
    assert sorted(hist) == ['loss', 'scores'] and len(hist['loss']) == 6


def test_flags_switch_the_loop_to_seg_loss(restated_tool, capsys):
    from seg2eye_amd.segment import seg_options, train_segmenter
    opt = seg_options(seg_hw=(32, 24), batchSize=6, niter=2, no_flip=True, lr=1e-2, print_freq=4, lambda_dice=1.0, lambda_surface=0.05,
                      edge_alpha=20.0, edge_radius=3)
    _, hist = train_segmenter(_tiny_store(), opt, net=_StubNet(), device='cpu', save=False, verbose=True)
    assert restated_tool['seg_cross_entropy'] == 0 and restated_tool['seg_loss'] == 6 and restated_tool['seg_dist_maps'] == 6
    assert (4, 3) in restated_tool['args'] and (False, False, 1.0, 1.0, 0.05, 20.0) in restated_tool['args']
    assert len(hist['loss']) == 6 and len(hist['terms']) == 6 and all(len(t) == 3 and np.isfinite(t).all() for t in hist['terms'])
    for total, t in zip(hist['loss'], hist['terms']):
        assert abs(total - (t[0] + t[1] + 0.05 * t[2])) < 1e-5
    line = [s for s in capsys.readouterr().out.splitlines() if s.startswith('epoch')][0]
    assert re.fullmatch(r'epoch 2 step 4 loss \d+\.\d{4} CE \d+\.\d{4} Dice \d+\.\d{4} Surface -?\d+\.\d{4}', line), line


def test_dice_alone_makes_no_distance_maps(restated_tool):
    from seg2eye_amd.segment import seg_options, train_segmenter
    opt = seg_options(seg_hw=(32, 24), batchSize=9, niter=1, no_flip=True, lambda_ce=0.5, lambda_dice=1.0)
    _, hist = train_segmenter(_tiny_store(), opt, net=_StubNet(), device='cpu', save=False, verbose=False)
    assert restated_tool['seg_loss'] == 2 and restated_tool['seg_dist_maps'] == 0
    assert restated_tool['args'] == [(True, True, 0.5, 1.0, 0.0, 0.0)] * 2 and len(hist['terms']) == 2


def test_parser_defaults_and_new_flags():
    from seg2eye_amd.segment import parser, seg_options
    a = parser().parse_args(['train', '--dataroot', 'x.h5'])
    assert (a.lambda_ce, a.lambda_dice, a.lambda_surface, a.edge_alpha, a.edge_radius) == (1.0, 0.0, 0.0, 0.0, 2)
    a = parser().parse_args(['train', '--dataroot', 'x.h5', '--edge_alpha', '20', '--edge_radius', '3', '--lambda_dice', '1', '--lambda_surface', '0.05',
                             '--lambda_ce', '0.5'])
    assert (a.lambda_ce, a.lambda_dice, a.lambda_surface, a.edge_alpha, a.edge_radius) == (0.5, 1.0, 0.05, 20.0, 3)
    a = vars(a)
    for k in ('command', 'dataroot'):
        a.pop(k)
    assert seg_options(**a).edge_alpha == 20.0
    with pytest.raises(SystemExit):
        parser().parse_args(['eval', '--dataroot', 'x.h5', '--lambda_dice', '1'])             # train only
