"""tests/_label_ops_ref.py on the CPU, per operation: (1) the fp64 reference is torch.nn.functional's fp64 forward and autograd's
backward to 1e-12 relative; (2) the bound is not too tight -- an honest fp32 evaluation of the same operation in ANOTHER summation
order, rounded to the output dtype, stays under it on every element; (3) the bound is not too loose -- the reference (rounded as the
kernel rounds) with one defect planted exceeds it.  Also the launch geometry the GPU cases assert.  No GPU needed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _label_ops_ref as R

DTS = ['bf16', 'fp32']
REV = tuple(reversed(range(9)))


def rnd(t, dt):
    """an fp64 / fp32 result as the kernel stores it"""
    return t.float().to(R.TDT[dt])


def rel_close(a, b, tol=1e-12):
    scale = max(1.0, float(b.abs().max()))
    assert float((a - b).abs().max()) <= tol * scale, float((a - b).abs().max())


# (N, H, W, h, w, ncls, Cout, bias, relu, map)
CONV_CASES = [(2, 24, 24, 12, 12, 4, 128, True, 1, 'blocky'), (1, 9, 14, 9, 7, 7, 20, False, 0, 'noise'), (3, 5, 6, 5, 6, 3, 152, True, 1, 'blocky'),
              (1, 1, 37, 1, 37, 1, 1, True, 0, 'one'), (1, 9, 14, 9, 7, 7, 22, False, 0, 'noise')]


def conv_case(c, seed=7):
    N, H, W, h, w, ncls, Cout, bias, relu, kind = c
    small = {'blocky': lambda: R.blocky_labels(N, h, w, ncls, seed, block=4), 'noise': lambda: R.noise_labels(N, h, w, ncls, seed),
             'one': lambda: R.one_class_labels(N, h, w, ncls - 1)}[kind]()
    label = R.expand_labels(small, H // h, W // w, ncls)
    wgt, b = R.label_conv_weights(Cout, ncls, bias, seed)
    return label, wgt, b


# ---- (1) the references are torch's
@pytest.mark.parametrize('c', CONV_CASES)
def test_label_conv_is_conv2d_of_the_one_hot(c):
    N, H, W, h, w, ncls, Cout, bias, relu, kind = c
    label, wgt, b = conv_case(c)
    ref = R.label_conv_eval(label, h, w, wgt.double(), None if b is None else b.double(), relu)
    lab = torch.from_numpy(label[:, ::H // h, ::W // w].astype(np.int64))
    want = F.conv2d(F.one_hot(lab, ncls).permute(0, 3, 1, 2).double(), wgt.double(), None if b is None else b.double(), padding=1)
    want = (F.relu(want) if relu else want).permute(0, 2, 3, 1)
    rel_close(ref, want)
    if kind == 'blocky':
        uni = R.uniform_pixels(label, h, w)
        assert 0 < int(uni.sum()) < uni.size
        assert not uni[:, 0].any() and not uni[:, :, -1].any()                 # a border pixel has neighbours outside the map
    if ncls == 7:
        assert int((label[:, ::H // h, ::W // w] == 6).sum()) > 0


def test_onehot_is_the_integer_definition():
    label = R.expand_labels(R.noise_labels(2, 3, 5, 4, 3), 2, 2, 4)
    img = torch.randn(2, 3, 5, generator=R.gen(1)).bfloat16()
    ref = R.onehot_ref(label, 3, 5, 4, 8, img)
    want = F.one_hot(torch.from_numpy(label[:, ::2, ::2].astype(np.int64)), 4).double()
    assert torch.equal(ref[..., :4], want) and torch.equal(ref[..., 4], img.double()) and not ref[..., 5:].any()
    assert not R.onehot_ref(label, 3, 5, 4, 5, None)[..., 4:].any()
    assert (R.onehot_kernel(8, False, 10), R.onehot_kernel(8, True, 10), R.onehot_kernel(12, False, 10)) == ('onehot_nhwc8', 'onehot_nhwc', 'onehot_nhwc')


@pytest.mark.parametrize('shape', [(2, 5, 7, 16), (1, 1, 1, 8), (3, 2, 9, 12)])
def test_upsample_is_nearest_and_its_autograd(shape):
    x = torch.randn(*shape, generator=R.gen(2), dtype=torch.float64).requires_grad_()
    y = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode='nearest').permute(0, 2, 3, 1)
    assert torch.equal(R.upsample_ref(x.detach()), y.detach())
    gy = torch.randn(*y.shape, generator=R.gen(3), dtype=torch.float64)
    rel_close(R.upsample_bwd_ref(gy, 'fp32')[0], torch.autograd.grad(y, x, gy)[0])


POOL_HW = [(1, 1), (1, 6), (2, 2), (5, 1), (17, 13), (32, 32)]


@pytest.mark.parametrize('H,W', POOL_HW)
def test_pool_is_avg_pool2d_and_its_autograd(H, W):
    x = torch.randn(2, H, W, 5, generator=R.gen(4), dtype=torch.float64).requires_grad_()
    y = F.avg_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1, count_include_pad=False).permute(0, 2, 3, 1)
    rel_close(R.pool_fwd_eval(x.detach()), y.detach())
    gy = torch.randn(*y.shape, generator=R.gen(5), dtype=torch.float64)
    rel_close(R.pool_bwd_eval(gy, H, W), torch.autograd.grad(y, x, gy)[0])
    cnt = R.pool_counts(H, W)
    assert cnt[0, 0] == min(2, H) * min(2, W) and float(cnt.max()) <= 9


def test_activation_backwards_are_autograd_and_inputs_hold_the_specials():
    for tanh in (True, False):
        for dt in DTS:
            gy, y = R.activation_inputs(4099, dt, 6, tanh)
            assert int((y == 0).sum()) > 3 and int((y.float().abs() == 1e-30 if dt == 'fp32' else (y.float().abs() < 1e-29) & (y != 0)).sum()) > 3
            assert not tanh or (int((y == 1).sum()) > 3 and int((y == -1).sum()) > 3)
    pre = torch.randn(300, generator=R.gen(7), dtype=torch.float64)
    pre[::7] = 0.0
    pre.requires_grad_()
    gy = torch.randn(300, generator=R.gen(8), dtype=torch.float64)
    y = torch.tanh(pre)
    rel_close(R.tanh_bwd_ref(gy, y.detach(), 'fp32')[0], torch.autograd.grad(y, pre, gy)[0])
    y = F.leaky_relu(pre, 0.2)
    rel_close(R.lrelu_bwd_ref(gy, y.detach(), 'fp32')[0], torch.autograd.grad(y, pre, gy)[0])


BIL = [(1, 1, 4, 4), (2, 3, 7, 300), (64, 96, 17, 23), (5, 5, 5, 5)]


@pytest.mark.parametrize('H,W,Ho,Wo', BIL)
def test_bilinear_is_interpolate_and_its_autograd(H, W, Ho, Wo):
    x = torch.randn(2, H, W, generator=R.gen(9), dtype=torch.float64).requires_grad_()
    y = F.interpolate(x[:, None], size=(Ho, Wo), mode='bilinear', align_corners=False)[:, 0]
    rel_close(R.bilinear_fwd_ref(x.detach().float(), Ho, Wo, 'fp32')[0], F.interpolate(x.detach().float().double()[:, None], size=(Ho, Wo), mode='bilinear')[:, 0])
    rel_close(R.bilinear_matrix(H, Ho) @ x.detach() @ R.bilinear_matrix(W, Wo).t(), y.detach())
    gy = torch.randn(2, Ho, Wo, generator=R.gen(10), dtype=torch.float64)
    rel_close(R.bilinear_bwd_ref(gy, H, W)[0], torch.autograd.grad(y, x, gy)[0])


# ---- (2) an honest fp32 evaluation in another order stays under the bound
@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('c', CONV_CASES)
def test_label_conv_fp32_other_order_is_under_the_bound(c, dt):
    N, H, W, h, w, ncls, Cout, bias, relu, kind = c
    label, wgt, b = conv_case(c)
    ref, bound = R.label_conv_ref(label, h, w, wgt, b, relu, dt)
    for order in (REV, (4, 0, 8, 2, 6, 1, 7, 3, 5)):
        assert R.exceeds(rnd(R.label_conv_eval(label, h, w, wgt, b, relu, torch.float32, order), dt), ref, bound) == 0


@pytest.mark.parametrize('dt', DTS)
def test_upsample_pool_fp32_other_order_is_under_the_bound(dt):
    g = R.gen(11)
    gy = torch.randn(3, 4, 18, 12, generator=g).to(R.TDT[dt])
    ref, bound = R.upsample_bwd_ref(gy, dt)
    f = gy.float()
    assert R.exceeds(rnd(((f[:, 1::2, 1::2] + f[:, 1::2, 0::2]) + f[:, 0::2, 1::2]) + f[:, 0::2, 0::2], dt), ref, bound) == 0
    for H, W in POOL_HW:
        x = (torch.randn(2, H, W, 5, generator=g) + 0.5).to(R.TDT[dt])
        ref, bound = R.pool_fwd_ref(x, dt)
        assert R.exceeds(rnd(R.pool_fwd_eval(x, torch.float32, REV), dt), ref, bound) == 0
        gyp = torch.randn(*ref.shape, generator=g).to(R.TDT[dt])
        ref, bound = R.pool_bwd_ref(gyp, H, W, dt)
        assert R.exceeds(rnd(R.pool_bwd_eval(gyp, H, W, torch.float32, REV), dt), ref, bound) == 0


@pytest.mark.parametrize('dt', DTS)
def test_activation_backwards_fp32_are_under_the_bound(dt):
    for n in (1, 3, R.VEC[dt] + 1, 4099):
        gy, y = R.activation_inputs(n, dt, 12 + n, True)
        ref, bound = R.tanh_bwd_ref(gy, y, dt)
        g, v = gy.float(), y.float()
        assert R.exceeds(rnd(g - (g * v) * v, dt), ref, bound) == 0                       # another association than gy (1 - y y)
        assert R.exceeds(rnd(g * (1 - v * v), dt), ref, bound) == 0
        gy, y = R.activation_inputs(n, dt, 13 + n, False)
        ref, bound = R.lrelu_bwd_ref(gy, y, dt)
        assert R.exceeds(rnd(gy.float() * torch.where(y.float() > 0, torch.tensor(1.0), torch.tensor(0.2)), dt), ref, bound) == 0


def _bilinear_fp32(x, Ho, Wo, reverse):
    """the kernel's recipe in fp32 on the CPU (fp32 scale, fp32 coordinate), the four products summed in either order"""
    N, H, W = x.shape

    def taps(n_in, n_out):
        s = torch.tensor(n_in, dtype=torch.float32) / torch.tensor(n_out, dtype=torch.float32)
        f = ((torch.arange(n_out, dtype=torch.float32) + 0.5) * s - 0.5).clamp_min(0)
        i0 = f.long()
        return i0, (i0 + 1).clamp_max(n_in - 1), f - i0.float()
    y0, y1, ly = taps(H, Ho)
    x0, x1, lx = taps(W, Wo)
    ly, lx = ly[None, :, None], lx[None, None, :]
    p = [x[:, y0][:, :, x0] * (1 - ly) * (1 - lx), x[:, y0][:, :, x1] * (1 - ly) * lx, x[:, y1][:, :, x0] * ly * (1 - lx), x[:, y1][:, :, x1] * ly * lx]
    return ((p[3] + p[2]) + p[1]) + p[0] if reverse else ((p[0] + p[1]) + p[2]) + p[3]


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('H,W,Ho,Wo', BIL)
def test_bilinear_fp32_is_under_the_bound(H, W, Ho, Wo, dt):
    x = (torch.randn(2, H, W, generator=R.gen(14)) * 2).requires_grad_()
    ref, bound = R.bilinear_fwd_ref(x.detach(), Ho, Wo, dt)
    y = F.interpolate(x[:, None], size=(Ho, Wo), mode='bilinear', align_corners=False)[:, 0]        # torch's own fp32 kernel
    assert R.exceeds(rnd(y.detach(), dt), ref, bound) == 0
    for reverse in (False, True):
        assert R.exceeds(rnd(_bilinear_fp32(x.detach(), Ho, Wo, reverse), dt), ref, bound) == 0
    gy = torch.randn(2, Ho, Wo, generator=R.gen(15)).to(R.TDT[dt])
    ref, bound = R.bilinear_bwd_ref(gy, H, W)
    assert R.exceeds(torch.autograd.grad(y, x, gy.float())[0], ref, bound) == 0                      # fp32, torch's order
    if (H, W) == (64, 96):
        assert int((bound == 0).sum()) > 0 and not ref[bound == 0].any()                            # pixels nothing reaches


# ---- (3) every named defect exceeds the bound
@pytest.mark.parametrize('dt', DTS)
def test_label_conv_defects_exceed_the_bound(dt):
    c = CONV_CASES[4]                                                                  # 9 x 7, 7 classes, Cout 22 (ragged in both dtypes), no ReLU
    N, H, W, h, w, ncls, Cout, bias, relu, kind = c
    label, wgt, b = conv_case(c)
    ref, bound = R.label_conv_ref(label, h, w, wgt, b, relu, dt)
    good = rnd(ref, dt)
    assert R.exceeds(good, ref, bound) == 0
    # one tap dropped at one pixel: every channel of that pixel moves by a weight of at least 0.05
    got = good.clone()
    got[0, 4, 3] = rnd(R.label_conv_eval(label, h, w, wgt.double(), None, relu, order=(0, 1, 2, 3, 5, 6, 7, 8))[0, 4, 3], dt)
    assert R.exceeds(got, ref, bound) == Cout
    # padding counted as class 0: only the border pixels move
    got = rnd(R.label_conv_eval(label, h, w, wgt.double(), None, relu, pad_cls=0), dt)
    over = ((got.double() - ref).abs() > bound).any(-1)[0]
    assert over[0].all() and over[-1].all() and over[:, 0].all() and over[:, -1].all() and not over[1:-1, 1:-1].any()
    # the channel tail Cout % VEC left unwritten (NaN, as the outputs start)
    got = good.clone()
    tail = Cout % R.VEC[dt]
    assert tail > 0
    got[..., Cout - tail:] = float('nan')
    assert R.exceeds(got, ref, bound) == N * h * w * tail
    # the tail of the last 64-pixel group skipped
    got = good.clone().view(-1, Cout)
    got[(N * h * w) // 64 * 64:] = float('nan')
    assert (N * h * w) % 64 and R.exceeds(got.view_as(ref), ref, bound) == ((N * h * w) % 64) * Cout


@pytest.mark.parametrize('dt', DTS)
def test_resampling_defects_exceed_the_bound(dt):
    g = R.gen(16)
    # the pool divisor 9 at a border pixel
    x = (torch.randn(2, 17, 13, 5, generator=g) + 1.0).to(R.TDT[dt])
    ref, bound = R.pool_fwd_ref(x, dt)
    for px in ((0, 3), (4, 0), (8, 6)):                        # top row, left column, the corner of the odd sizes
        assert R.pool_counts(17, 13)[px] < 9
        assert R.exceeds(rnd(R.pool_fwd_eval(x.double(), div9=(px,)), dt), ref, bound) >= 2 * 5 - 1
    # an upsample backward that adds three of the four
    gy = (torch.randn(2, 4, 6, 16, generator=g) + 0.5).to(R.TDT[dt])
    ref, bound = R.upsample_bwd_ref(gy, dt)
    q = gy.double()
    assert R.exceeds(rnd(q[:, 0::2, 0::2] + q[:, 0::2, 1::2] + q[:, 1::2, 0::2], dt), ref, bound) > 0.95 * ref.numel()
    # LeakyReLU slope 1 at y == 0
    gy, y = R.activation_inputs(4099, dt, 17, False)
    ref, bound = R.lrelu_bwd_ref(gy, y, dt)
    got = rnd(gy.double() * torch.where(y.double() >= 0, 1.0, 0.2), dt)
    assert R.exceeds(got, ref, bound) == int(((y == 0) & (gy != 0)).sum()) > 0
    # a bilinear i1 not clamped at the last row: it reads the row behind the image (here: the next image's first row, or beyond)
    x = torch.randn(2, 2, 3, generator=g)
    ref, bound = R.bilinear_fwd_ref(x, 7, 300, dt)
    ext = torch.cat([x, torch.cat([x[1:, :1], torch.full((1, 1, 3), 7.0)])], 1).double()          # (2, 3, 3): the row an unclamped i1 reads
    f, i0, i1, l = R.bilinear_taps(2, 7)
    Ry = torch.zeros(7, 3, dtype=torch.float64)
    Ry[torch.arange(7), i0] += 1 - l
    Ry[torch.arange(7), i0 + 1] += l
    got = rnd(Ry @ ext @ R.bilinear_matrix(3, 300).t(), dt)
    over = ((got.double() - ref).abs() > bound)
    assert over[:, -1].any() and not over[:, :4].any()


# ---- the launch geometry the GPU cases assert
def test_label_conv_plan():
    P = R.label_conv_plan
    assert P('bf16', 65780, 128, R.FAST_MIN_SINGLE) == (257, [('wave', 16, 256, 1)])
    assert P('fp32', 65780, 12, R.FAST_MIN_SINGLE)[1] == [('thread', 3, 85, 1)] and P('bf16', 65780, 12, R.FAST_MIN_SINGLE)[1][0][:2] == ('wave', 2)
    assert [c[:2] for c in P('bf16', 65780, 136, R.FAST_MIN_SINGLE)[1]] == [('wave', 16), ('wave', 1)]
    assert [c[0] for c in P('bf16', 65535, 8, R.FAST_MIN_SINGLE)[1]] == ['thread'] and [c[0] for c in P('bf16', 65536, 8, R.FAST_MIN_SINGLE)[1]] == ['wave']
    assert [c[:2] for c in P('bf16', 90, 152, R.FAST_MIN_SINGLE)[1]] == [('thread', 16), ('thread', 3)]
    assert [c[:2] for c in P('bf16', 16, 260, R.FAST_MIN_SINGLE)[1]] == [('thread', 16), ('thread', 16), ('thread', 1)]
    assert P('bf16', 2112, 128, R.FAST_MIN_BATCH)[1][0][0] == 'wave' and P('bf16', 528, 64, R.FAST_MIN_BATCH)[1][0][0] == 'thread'
    gx, chunks = P('bf16', 65780, 136, R.FAST_MIN_SINGLE, cap=3)
    assert gx == 3 and all(c[3] == 86 for c in chunks)
    assert R.wraps(8192 * 256 + 1) and not R.wraps(8192 * 256) and R.wraps(4096 * 256 + 1, R.GRID_CAP_ONEHOT8)
    assert (R.pool_kernel('bf16', 12), R.pool_kernel('fp32', 12), R.pool_kernel('bf16', 5), R.pool_kernel('fp32', 16)) == ('scalar', 'vector', 'scalar', 'vector')


def test_ramp_has_no_equal_values_a_grid_apart():
    for dt in DTS:
        r = R.ramp((3 * 8192 * 256 // 8,), dt).float()
        for stride in (8192 * 256 // 8, 4096 * 256 // 8, 256, 1):
            assert not (r[stride:] == r[:-stride]).any()
        assert torch.equal(r.double(), (torch.arange(r.numel()) % 251).double() / 64 - 1)
