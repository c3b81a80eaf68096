"""fp64 references, per-element bounds, launch geometry and input generators for the label-map and resampling kernels of
csrc/label_ops.hip: s2e_label_conv3x3 (+ _batch), s2e_onehot_nhwc, s2e_upsample2x_fwd / _bwd, s2e_avgpool3x3s2_fwd / _bwd,
s2e_tanh_bwd, s2e_lrelu_bwd, s2e_bilinear_resize_fwd / _bwd.  CPU only; imports nothing of the library.  tests/_label_ops_child.py
compares the kernels against these on the GPU, tests/test_label_ops_ref_host.py checks on the CPU that the references are
torch.nn.functional's and autograd's, that an honest fp32 / bf16 evaluation stays under every bound, and that each of eight planted
defects exceeds it.

Reference.  fp64 from exactly the values a kernel is handed (bf16 / fp32 tensors widened), written from the operation's definition:
  label conv   conv3x3(one_hot(label[::sy, ::sx]), weight, pad 1) + bias, optional ReLU: a gather over the nine taps of weight[:, cls, tap]
               with the class of each neighbour, nothing for a neighbour outside the map
  one-hot      out[n, y, x, c] = 1 if label[n, y sy, x sx] == c for c < ncls, the image for c == ncls (when given), 0 beyond
  upsample 2x  y[2i + a, 2j + b] = x[i, j]; backward the sum of the four
  avg pool     3x3 stride 2 pad 1, count_include_pad=False: the mean of the in-image taps; backward its explicit transpose
  tanh' / LeakyReLU'  gy (1 - y^2); gy (1 if y > 0 else 0.2) -- torch.nn.functional.leaky_relu's rule, 0.2 AT zero
  bilinear     align_corners=False: source coordinate f = max((d + 0.5) in / out - 0.5, 0), taps i0 = floor f, i1 = min(i0 + 1, in - 1),
               weights (1 - l, l), l = f - i0, as matrices Ry (Ho x H), Rx (Wo x W): y = Ry x Rx^T, backward gx = Ry^T gy Rx

Bounds, per element; the GPU check is err / bound <= 1 everywhere (a bound of 0 demands equality).  u = 2^-24 is the fp32 unit
roundoff, gamma(k) = k u / (1 - k u) bounds k successive roundings, hu(ref) is half an ulp of the OUTPUT format at the reference
(2^(e - 9) for bf16 and 0 for fp32 -- an fp32 output's own rounding is the last of the k -- with 2^e <= |ref| < 2^(e + 1)), and every
fp32 error e in front of a bf16 store enters as (1 + 2^-7) e, because the stored value is the rounding of ref + e, not of ref.
  sums           gamma(k) A + hu, A the sum of the terms' magnitudes, k the number of terms the operation really adds:
    label conv     k = 10: the bias and nine table rows (fewer at the border).  ReLU is 1-Lipschitz: the same bound after it.
    upsample bwd   k = 4
    pool fwd       k = cnt + 1: cnt <= 9 in-image taps and the (correctly rounded: no fast-math) division; A = sum |x| / cnt
    pool bwd       k = m + 1: m <= 4 outputs reach an input pixel, each term gy / cnt is one division; A = sum |gy| / cnt
  tanh'          gamma(3) |gy| (1 + y^2) + hu: y y, 1 - y y (which cancels near |y| = 1: the error is relative to 1 + y^2, not to 1 - y^2),
                 the product
  LeakyReLU'     gamma(2) |ref| + hu: the fp32 constant 0.2f and the product
  selections     one-hot, upsample forward: bit for bit
  bilinear fwd   the kernel forms f in fp32 from scale = fl(in / out): scale, the product and the subtraction are three roundings
                 of numbers no larger than f + 1, so |f_kernel - f| <= d = COORD_ULPS u (f + 1) with COORD_ULPS = 4.  The interpolant is
                 continuous and piecewise linear in f, so a coordinate off by d moves the value by at most d times the steepest
                 segment nearby: slope_y = max |x[s + 1, c] - x[s, c]| over the segments s in i0y - 1 .. i0y + 1 and the columns c
                 in i0x - 2 .. i0x + 2 (a superset of what either the exact or the rounded coordinate can touch), likewise slope_x.
                 bound = d_y slope_y + d_x slope_x + gamma(8) (Ry |x| Rx^T) + hu: 1 - l, two products and two sums per axis.
  bilinear bwd   per INPUT pixel, over the terms that land on it, whatever the order of the fp32 atomics: K terms land (each of the
                 four taps of an output pixel counts, also with weight 0), each formed with 4 roundings (1 - ly, 1 - lx, two
                 products): gamma(K + 4) (Ry^T |gy| Rx).  The coordinate error changes a term's weight by at most d_y + d_x and, where
                 f crosses an integer, moves d |gy| from one pixel to its neighbour: every input pixel in i0 - 1 .. i0 + 2 (both
                 axes) of an output pixel gets (d_y + d_x) |gy| of it.  An input pixel that nothing reaches has bound 0 and must
                 come back 0.

Launch geometry (closed forms read from the launchers of csrc/label_ops.hip, so that a case can assert the path it was written for
from npix, Cout, VEC and the cap, without asking the library): label_conv_plan(), pool_kernel(), onehot_kernel(), wraps()."""
import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
TDT = {'bf16': torch.bfloat16, 'fp32': torch.float32}
VEC = {'bf16': 8, 'fp32': 4}
COORD_ULPS = 4
SLOPE = 0.2
FAST_MIN_SINGLE, FAST_MIN_BATCH = 65536, 2048          # pixels from which the wave walk runs: a launch alone / inside the batch
LABEL_CONV_CAP = 1024                                  # S2E_LABEL_CONV_CAP's default
GRID_CAP, GRID_CAP_ONEHOT8 = 8192, 4096                # s2e_grid1d's caps, in 256-thread blocks


def cdiv(a, b):
    return -(-a // b)


def gamma(k):
    return k * U32 / (1.0 - k * U32)


def half_ulp(ref, dt):
    """half an ulp of the output format at |ref| (0 for fp32: see the module docstring)"""
    if dt == 'fp32':
        return torch.zeros_like(ref)
    _, e = torch.frexp(ref)                            # |ref| in [2^(e-1), 2^e): bf16 ulp 2^(e-1-7)
    return torch.where(ref == 0, torch.zeros_like(ref), torch.ldexp(torch.ones_like(ref), e - 9))


def bound_of(ref, fp32_err, dt):
    """hu(ref) + the fp32 error in front of the store"""
    return half_ulp(ref, dt) + (1.0 + (2.0 ** -7 if dt == 'bf16' else 0.0)) * fp32_err


def worst_ratio(got, ref, bound, what):
    """max err / bound over every element; asserts it is <= 1 (NaN fails; bound 0 demands equality)"""
    g = got.detach().double().cpu()
    assert g.shape == ref.shape, '%s: shape %s, reference %s' % (what, tuple(g.shape), tuple(ref.shape))
    assert bool(torch.isfinite(g).all()), '%s: %d non-finite elements (unwritten or NaN)' % (what, int((~torch.isfinite(g)).sum()))
    err = (g - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if not worst <= 1.0:
        i = int(ratio.flatten().argmax())
        idx = tuple(int(v) for v in np.unravel_index(i, tuple(ratio.shape)))
        raise AssertionError('%s: err / bound %.3g at %s (got %.9g, reference %.9g, bound %.3g); %d of %d elements over' % (
            what, worst, idx, float(g.flatten()[i]), float(ref.flatten()[i]), float(bound.flatten()[i]), int((ratio > 1).sum()), ratio.numel()))
    return worst


def exceeds(got, ref, bound):
    """number of elements over the bound (the host proof's view of worst_ratio)"""
    err = (got.double() - ref).abs()
    return int(((err > bound) | ~torch.isfinite(got.double())).sum())


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- label maps
def noise_labels(N, H, W, ncls, seed):
    """random classes: (almost) no uniform neighbourhood"""
    return np.random.RandomState(seed).randint(0, ncls, size=(N, H, W)).astype(np.uint8)


def one_class_labels(N, H, W, cls):
    return np.full((N, H, W), cls, dtype=np.uint8)


def blocky_labels(N, H, W, ncls, seed, block=5):
    """constant blocks of block x block pixels (classes at random, the last class forced in) with a few single pixels changed"""
    g = np.random.RandomState(seed)
    coarse = g.randint(0, ncls, size=(N, cdiv(H, block), cdiv(W, block))).astype(np.uint8)
    coarse.flat[0] = ncls - 1
    lab = coarse.repeat(block, 1).repeat(block, 2)[:, :H, :W].copy()
    for _ in range(max(1, N * H * W // 97)):
        n, y, x = g.randint(N), g.randint(H), g.randint(W)
        lab[n, y, x] = (lab[n, y, x] + 1) % ncls
    return lab


def expand_labels(lab, sy, sx, ncls):
    """(N, h, w) -> (N, h sy, w sx) whose [::sy, ::sx] is lab and whose skipped pixels are all ANOTHER class (ncls > 1), so that a
    kernel that reads a skipped pixel is seen"""
    N, h, w = lab.shape
    big = ((lab.astype(np.int64) + 1) % max(ncls, 1)).astype(np.uint8).repeat(sy, 1).repeat(sx, 2)
    big[:, ::sy, ::sx] = lab
    return big


# ---- label conv
def _neighbour_classes(label, h, w, pad_cls):
    """(9, N, h, w) int64: the class of each 3x3 neighbour (tap = ky * 3 + kx) of the nearest-downsampled map, pad_cls outside it"""
    N, H, W = label.shape
    assert H % h == 0 and W % w == 0
    lab = label[:, ::H // h, ::W // w]
    assert lab.shape == (N, h, w)
    p = np.full((N, h + 2, w + 2), pad_cls, dtype=np.int64)
    p[:, 1:-1, 1:-1] = lab
    return np.stack([p[:, ky:ky + h, kx:kx + w] for ky in range(3) for kx in range(3)])


def label_conv_eval(label, h, w, weight, bias, relu, dtype=torch.float64, order=range(9), absolute=False, pad_cls=None):
    """(N, h, w, Cout) in `dtype`, the taps added in `order` onto the bias.  weight (Cout, ncls, 3, 3), bias (Cout,) | None.
    absolute: the sum of the magnitudes instead (the A of the bound; no ReLU).  pad_cls: the class a neighbour outside the map counts
    as (a defect; None: it adds nothing)."""
    Cout, ncls = weight.shape[:2]
    nb = torch.from_numpy(_neighbour_classes(label, h, w, ncls if pad_cls is None else pad_cls))
    wt = torch.cat([weight, torch.zeros(Cout, 1, 3, 3, dtype=weight.dtype)], 1).to(dtype)      # row ncls: outside the map, nothing
    b = torch.zeros(Cout, dtype=dtype) if bias is None else bias.to(dtype)
    if absolute:
        wt, b = wt.abs(), b.abs()
    out = b.expand(*nb.shape[1:], Cout).clone()
    for t in order:
        out += wt[:, :, t // 3, t % 3].t()[nb[t]]
    return out.clamp_min(0) if (relu and not absolute) else out


def label_conv_ref(label, h, w, weight, bias, relu, dt):
    """-> (ref, bound) in fp64"""
    w64 = weight.double()
    b64 = None if bias is None else bias.double()
    ref = label_conv_eval(label, h, w, w64, b64, relu)
    A = label_conv_eval(label, h, w, w64, b64, relu, absolute=True)
    return ref, bound_of(ref, gamma(10) * A, dt)


def uniform_pixels(label, h, w):
    """(N, h, w) bool: the pixel's nine neighbours are all inside the map and of ONE class"""
    nb = _neighbour_classes(label, h, w, -1)
    return (nb == nb[0]).all(0) & (nb[0] >= 0)


def label_conv_weights(Cout, ncls, with_bias, seed):
    g = gen(seed)
    w = torch.randn(Cout, ncls, 3, 3, generator=g) * 0.5
    w += 0.05 * torch.sign(w)                          # no tap so small that dropping it hides under the bound
    b = torch.randn(Cout, generator=g) * 0.3 if with_bias else None
    return w, b


def label_conv_plan(dt, npix, Cout, fast_min, cap=LABEL_CONV_CAP):
    """-> (blocks along the pixels, [(walk, lanes per pixel, pixels per block per pass, passes)] per 128-channel chunk).  The grid is
    sized from the FIRST chunk; every chunk walks with its own lanes-per-pixel."""
    vec = VEC[dt]

    def walk(cw):
        cgb = cdiv(cw, vec)
        return ('wave', cgb, 256) if (64 % cgb == 0 and npix >= fast_min) else ('thread', cgb, 256 // cgb)
    gx = min(cap, cdiv(npix, walk(min(Cout, 128))[2]))
    chunks = []
    for c0 in range(0, Cout, 128):
        wk, cgb, ppb = walk(min(128, Cout - c0))
        chunks.append((wk, cgb, ppb, cdiv(npix, gx * ppb)))
    return gx, chunks


# ---- one-hot
def onehot_ref(label, h, w, ncls, cpad, img):
    """(N, h, w, cpad) fp64; img (N, h, w) of the compute dtype | None"""
    N, H, W = label.shape
    lab = torch.from_numpy(label[:, ::H // h, ::W // w].astype(np.int64))
    out = torch.zeros(N, h, w, cpad, dtype=torch.float64)
    for c in range(ncls):
        out[..., c] = (lab == c).double()
    if img is not None:
        out[..., ncls] = img.double()
    return out


def onehot_kernel(cpad, misaligned, px):
    return 'onehot_nhwc8' if (cpad == 8 and not misaligned and px < 2 ** 31) else 'onehot_nhwc'


# ---- upsample 2x
def upsample_ref(x):
    """x (N, h, w, C) -> (N, 2h, 2w, C), the same values"""
    N, h, w, C_ = x.shape
    y = torch.empty(N, 2 * h, 2 * w, C_, dtype=x.dtype)
    for a in range(2):
        for b in range(2):
            y[:, a::2, b::2] = x
    return y


def upsample_bwd_ref(gy, dt):
    g = gy.double()
    q = [g[:, a::2, b::2] for a in range(2) for b in range(2)]
    ref = q[0] + q[1] + q[2] + q[3]
    A = q[0].abs() + q[1].abs() + q[2].abs() + q[3].abs()
    return ref, bound_of(ref, gamma(4) * A, dt)


# ---- average pool 3x3 s2 p1, count_include_pad=False
def _pool_taps(H, W):
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    return Ho, Wo, [(ky, kx, slice(ky, ky + 2 * Ho, 2), slice(kx, kx + 2 * Wo, 2)) for ky in range(3) for kx in range(3)]


def pool_counts(H, W):
    """(Ho, Wo) fp64: in-image taps of every output pixel"""
    Ho, Wo, taps = _pool_taps(H, W)
    ones = F.pad(torch.ones(H, W, dtype=torch.float64), (1, 1, 1, 1))
    return sum(ones[sy, sx][:Ho, :Wo] for _, _, sy, sx in taps)


def pool_fwd_eval(x, dtype=torch.float64, order=range(9), div9=()):
    """x (N, H, W, C) -> (N, Ho, Wo, C) in dtype.  div9: output pixels (oy, ox) divided by 9 whatever their count (a defect)"""
    N, H, W, C_ = x.shape
    Ho, Wo, taps = _pool_taps(H, W)
    xp = F.pad(x.to(dtype), (0, 0, 1, 1, 1, 1))
    s = torch.zeros(N, Ho, Wo, C_, dtype=dtype)
    for t in order:
        _, _, sy, sx = taps[t]
        s += xp[:, sy, sx][:, :Ho, :Wo]
    cnt = pool_counts(H, W).clone()
    for oy, ox in div9:
        cnt[oy, ox] = 9
    return s / cnt.to(dtype)[None, :, :, None]


def pool_fwd_ref(x, dt):
    N, H, W, C_ = x.shape
    ref = pool_fwd_eval(x.double())
    A = pool_fwd_eval(x.double().abs())
    k = pool_counts(H, W)[None, :, :, None] + 1
    return ref, bound_of(ref, k * U32 / (1 - k * U32) * A, dt)


def pool_bwd_eval(gy, H, W, dtype=torch.float64, order=range(9), count=False):
    """the transpose of pool_fwd_eval: every tap (oy, ox) -> (2 oy - 1 + ky, 2 ox - 1 + kx) carries gy / cnt back.
    count: how many outputs reach each input pixel instead."""
    N, Ho, Wo, C_ = gy.shape
    Ho2, Wo2, taps = _pool_taps(H, W)
    assert (Ho, Wo) == (Ho2, Wo2)
    term = torch.ones(1, Ho, Wo, 1, dtype=dtype) if count else gy.to(dtype) / pool_counts(H, W).to(dtype)[None, :, :, None]
    gp = torch.zeros(term.shape[0], 2 * Ho + 2, 2 * Wo + 2, term.shape[3], dtype=dtype)
    for t in order:
        _, _, sy, sx = taps[t]
        gp[:, sy, sx] += term
    return gp[:, 1:H + 1, 1:W + 1]


def pool_bwd_ref(gy, H, W, dt):
    ref = pool_bwd_eval(gy.double(), H, W)
    A = pool_bwd_eval(gy.double().abs(), H, W)
    k = pool_bwd_eval(gy, H, W, count=True) + 1
    return ref, bound_of(ref, k * U32 / (1 - k * U32) * A, dt)


def pool_kernel(dt, C_):
    return 'vector' if C_ % VEC[dt] == 0 else 'scalar'


# ---- tanh', LeakyReLU'
def tanh_bwd_ref(gy, y, dt):
    g, v = gy.double(), y.double()
    ref = g * (1 - v * v)
    return ref, bound_of(ref, gamma(3) * g.abs() * (1 + v * v), dt)


def lrelu_bwd_ref(gy, y, dt):
    g, v = gy.double(), y.double()
    ref = g * torch.where(v > 0, torch.ones_like(v), torch.full_like(v, SLOPE))
    return ref, bound_of(ref, gamma(2) * ref.abs(), dt)


def activation_inputs(n, dt, seed, tanh):
    """gy, y of n elements in the compute dtype: y with exact zeros, +-tiny values and (tanh) +-1 among ordinary values"""
    g = gen(seed)
    gy = torch.randn(n, generator=g) + 0.1
    y = torch.tanh(torch.randn(n, generator=g)) if tanh else torch.randn(n, generator=g)
    special = [0.0, -0.0, 1e-30, -1e-30, 2.0 ** -126, -2.0 ** -126] + ([1.0, -1.0] if tanh else [])
    pos = torch.arange(n)
    for j, s in enumerate(special):                    # every special value at several places, the first and the last elements included
        y[pos % len(special) == j] = torch.where(torch.rand(int((pos % len(special) == j).sum()), generator=g) < 0.5,
                                                 torch.tensor(s), y[pos % len(special) == j])
    y[0], y[-1] = 0.0, (-1e-30 if n > 1 else 0.0)
    return gy.to(TDT[dt]), y.to(TDT[dt])


# ---- bilinear, align_corners=False
def bilinear_taps(n_in, n_out):
    """-> (f, i0, i1, l) in fp64 / int64 by torch's source-index rule"""
    d = torch.arange(n_out, dtype=torch.float64)
    f = ((d + 0.5) * (n_in / n_out) - 0.5).clamp_min(0)
    i0 = f.floor().long().clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    return f, i0, i1, f - i0


def bilinear_matrix(n_in, n_out):
    """(n_out, n_in) fp64 interpolation matrix"""
    f, i0, i1, l = bilinear_taps(n_in, n_out)
    R = torch.zeros(n_out, n_in, dtype=torch.float64)
    r = torch.arange(n_out)
    R.index_put_((r, i0), 1 - l, accumulate=True)
    R.index_put_((r, i1), l, accumulate=True)
    return R


def _coord_err(n_in, n_out):
    f = bilinear_taps(n_in, n_out)[0]
    return COORD_ULPS * U32 * (f + 1)


def _steepest(x, axis_y, i0y, i0x):
    """(N, Ho, Wo): the largest |difference of neighbouring pixels along the axis| near the taps (see the module docstring)"""
    N, H, W = x.shape
    D = (x[:, 1:] - x[:, :-1]).abs() if axis_y else (x[:, :, 1:] - x[:, :, :-1]).abs()
    if D.numel() == 0:
        return torch.zeros(N, len(i0y), len(i0x), dtype=torch.float64)
    k = (3, 5) if axis_y else (5, 3)
    M = F.max_pool2d(D[:, None], k, 1, (k[0] // 2, k[1] // 2))[:, 0]
    iy = i0y.clamp_max(M.shape[1] - 1)
    ix = i0x.clamp_max(M.shape[2] - 1)
    return M[:, iy][:, :, ix]


def bilinear_fwd_ref(x, Ho, Wo, dt):
    """x (N, H, W) fp32 -> (ref, bound), (N, Ho, Wo)"""
    N, H, W = x.shape
    x64 = x.double()
    Ry, Rx = bilinear_matrix(H, Ho), bilinear_matrix(W, Wo)
    ref = Ry @ x64 @ Rx.t()
    A = Ry @ x64.abs() @ Rx.t()
    i0y, i0x = bilinear_taps(H, Ho)[1], bilinear_taps(W, Wo)[1]
    coord = _coord_err(H, Ho)[None, :, None] * _steepest(x64, True, i0y, i0x) + _coord_err(W, Wo)[None, None, :] * _steepest(x64, False, i0y, i0x)
    return ref, bound_of(ref, coord + gamma(8) * A, dt)


def _tap_count(n_in, n_out, near):
    """(n_out, n_in): near=False -- how many of an output's two taps are this input (0, 1, 2); near=True -- 1 on i0 - 1 .. i0 + 2"""
    _, i0, i1, _ = bilinear_taps(n_in, n_out)
    Cm = torch.zeros(n_out, n_in, dtype=torch.float64)
    r = torch.arange(n_out)
    if near:
        for k in (-1, 0, 1, 2):
            Cm[r, (i0 + k).clamp(0, n_in - 1)] = 1
    else:
        Cm.index_put_((r, i0), torch.ones(n_out, dtype=torch.float64), accumulate=True)
        Cm.index_put_((r, i1), torch.ones(n_out, dtype=torch.float64), accumulate=True)
    return Cm


def bilinear_bwd_ref(gy, H, W):
    """gy (N, Ho, Wo) of the compute dtype -> (ref, bound), (N, H, W); the output is fp32 whatever gy's dtype"""
    N, Ho, Wo = gy.shape
    g = gy.double()
    Ry, Rx = bilinear_matrix(H, Ho), bilinear_matrix(W, Wo)
    ref = Ry.t() @ g @ Rx
    A = Ry.t() @ g.abs() @ Rx
    K = (_tap_count(H, Ho, False).t() @ torch.ones(Ho, Wo, dtype=torch.float64) @ _tap_count(W, Wo, False))[None]
    slack = _tap_count(H, Ho, True).t() @ (g.abs() * (_coord_err(H, Ho)[:, None] + _coord_err(W, Wo)[None, :])) @ _tap_count(W, Wo, True)
    k = K + 4
    return ref, k * U32 / (1 - k * U32) * A + slack


# ---- grid-stride wrap
def wraps(work_items, cap=GRID_CAP):
    """a grid-stride kernel with one item per thread takes a second pass"""
    return work_items > cap * 256


def ramp(shape, dt, period=251, scale=1.0 / 64):
    """index-dependent values, exact in bf16 (multiples of `scale` below 2^8 of them), no two neighbours equal; the period is a prime,
    so a wrong second-pass index (a multiple of the grid size, a power of two) cannot land on an equal value"""
    n = 1
    for s in shape:
        n *= s
    v = (torch.arange(n, dtype=torch.int64) % period).float() * scale - 1.0
    return v.view(*shape).to(TDT[dt])
