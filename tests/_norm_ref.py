"""fp64 references, absolute-value twins, bounds, geometry and input generators for the kernels of csrc/norm_modulate.hip:
InstanceNorm statistics, plain IN (+ LeakyReLU) forward / backward, the SPADE+Style modulation forward / backward in all its forms,
column sums.  CPU only; imports nothing of the library.  tests/_norm_child.py compares the kernels against these on the GPU,
tests/test_norm_ref_host.py checks the references against autograd and that the bounds catch the mutants listed in MUTANTS.

Reference.  fp64, from exactly the values a kernel is handed: bf16 / fp32 tensors widened, fp32 stats and style widened.  The backward
entries take `stats` as an INPUT: the reference uses the supplied values and never recomputes them, so the LeakyReLU mask of plain IN
(x > mean on the given fp32 mean) and of the gamma-only form (sign of the supplied `out`) is exact.

The library's LeakyReLU contract is torch.nn.functional.leaky_relu's: slope 0.2 unless the argument is > 0 (so 0.2 AT zero: an exactly
constant channel, x == mean everywhere, takes 0.2 in every kernel, whatever the map size).

Bound, per element.
  compute-dtype outputs (out, dx, dgb):    |got - ref| <= u |ref| + C_ACC A (+ extra)       u = 2^-8 (bf16) / 2^-23 (fp32)
  fp32 / fp64 reduced outputs (sums, dstyle, colsum): |got - ref| <= 2^-23 |ref| + C_ACC A_sum + 2^-23 |start|
A is the formula on absolute values of every term and of every reduced sum (sum|.| / HW for a mean).  xhat = (x - mean) * rstd of
GIVEN x and mean is one exact-sign subtraction and one product, so its own twin is |xhat|; only where a kernel multiplies the
coefficients out (dx = ... - Q - x S, which cancels in fp32 when |mean| >> std) the twin is (|x| + |mean|) rstd.  C_ACC = 2^-16, DERIVED: a thread's
fp32 accumulator takes one rounded addition per row it owns beyond the first (the first lands on 0.0: exact), then everything is fp64.
chain_roundings() states that count per case -- at most 64 at every shape of this suite (65 rows of the 4100-pixel map on 64 row
lanes, `iters` <= 33 rows on the row walk, 64 rows per thread in colsum) -- and the host test asserts it.  64 roundings of 2^-24 A are
2^-18 A even added linearly, the dozen element-wise fp32 operations after them another 2^-20 A: 2^-16 leaves a factor of ~3.
colsum ends in fp32 atomics (one per block) instead of fp64: its total count of roundings (thread chain + fold + atomics) is at most
128 here, i.e. 2^-17 (A_sum + |start|); the test starts `out` at O(1) values, far below A_sum / 50, so the 2^-23 |start| term holds.
  statistics: mean as a sum / HW; rstd by propagating the variance error  dvar <= C_ACC (E|x^2| + 2 |mean| E|x|),
              drstd / rstd <= dvar / (2 (var + eps)) + 2^-23.
  forwards that compute their own statistics add  rstd dmean + |xhat| drstd / rstd.
  row-walk SPADE backward only: pass 2 reads dbeta back in the compute dtype, so dx gets  + r |0.5 go (1 + s0 + rstd (1 + gamma))|
  (`readback`), r = the relative error of that one rounding: 2^-8 for bf16 (RNE to 8 significant bits: half an ulp is 2^-8 of a value
  just above a power of two -- the same u as an output's; a first version had u / 2 here, which the kernel's arithmetic, emulated
  in fp32 on the CPU, exceeds in 1,272 of 163,968 elements by up to 1.5x), 0 for fp32 (stored exactly).  The one-launch small-map
  kernel recomputes go and gets no such term.
  quad form: the sum of four full-resolution terms, rounded once: A (and readback) summed over the four.

Tail table (S2E_IN_SMALL_HW=0; N = 2): rows per thread in the LAST slab of the row walk, (fewest, most) over the row lanes.
The reduce kernel takes rows in trips of 4, 2, 1, so `most % 4` must cover 0, 1, 2, 3 per dtype -- TAIL_ROWS below is that table,
written out by hand from the closed forms of row_plan() and checked against them by the host test."""
import torch

from _conv3x3_child import BF16_RNE, C_ACC            # the project's constants: not copied

F32_RNE = 2.0 ** -23
U = {'bf16': BF16_RNE, 'fp32': F32_RNE}
TDT = {'bf16': torch.bfloat16, 'fp32': torch.float32}
VEC = {'bf16': 8, 'fp32': 4}
EPS = 1e-5
SPADE, PLAIN = 0, 1                                    # S2E_NORM_SPADE_STYLE, S2E_NORM_PLAIN_IN
KINK_BAND = 2.0 ** -12
MAX_CHAIN = 64
MUTANTS = ('drop_row', 'drop_slot', 'swap_s', 'hw1', 'dgamma_x', 'mask1', 'no_dx_add', 'no_batch_count', 'quad3')


def cdiv(a, b):
    return -(-a // b)


# ---- geometry (closed forms read from csrc/norm_modulate.hip; not queried from the library)
def small_groups(N, C, dt):
    """channel groups per block of the one-launch kernels; their row lanes are 256 / G"""
    return 4 if N * cdiv(C, 8 * VEC[dt]) < 192 else 8


def row_plan(dt, N, HW, C):
    """(cg, cgb, rpp, zblocks, iters, P) of the row-walking kernels"""
    cg = C // VEC[dt]
    cgb = min(cg, 256)
    rpp = 256 // cgb
    zb = cdiv(cg, cgb)
    per_n = max(1, 256 // (N * zb))
    iters = max(16, cdiv(HW, rpp * per_n))
    return cg, cgb, rpp, zb, iters, cdiv(HW, rpp * iters)


def last_slab_rows(dt, N, HW, C):
    """(fewest, most) rows a row lane owns in the last slab of a sample"""
    _, _, rpp, _, iters, P = row_plan(dt, N, HW, C)
    last = HW - (P - 1) * rpp * iters
    return max(0, cdiv(last - (rpp - 1), rpp)), cdiv(last, rpp)


def slot_rows(dt, N, HW, C):
    """first pixel row of the last partial-sum slot of a sample"""
    _, _, rpp, _, iters, P = row_plan(dt, N, HW, C)
    return (P - 1) * rpp * iters


def chain_roundings(kind, dt, N, HW, C):
    """rounded fp32 additions in one thread's accumulator (rows it owns - 1) for a case of `kind` in small / rowwalk / colsum"""
    if kind == 'small':
        rows = cdiv(HW, 256 // small_groups(N, C, dt))
    elif kind == 'rowwalk':
        rows = row_plan(dt, N, HW, C)[4]
    else:                                              # colsum: HW is M; 64 row passes per block, or the scalar fallback's stride
        rows = 64 if C % VEC[dt] == 0 else cdiv(HW, 256 * min(HW // 1024 + 1, 256))
    return max(0, rows - 1)


def colsum_total_roundings(dt, M, C):
    """colsum: thread chain + fold over lanes / waves + one fp32 atomic per block"""
    if C % VEC[dt]:
        blocks = min(M // 1024 + 1, 256)
        return chain_roundings('colsum', dt, 1, M, C) + 6 + 3 + blocks
    cg = C // VEC[dt]
    rpp = 256 // min(cg, 256)
    return 63 + rpp + cdiv(M, rpp * 64)


# (dtype, HW, C) -> (fewest, most) rows per lane in the last slab, N = 2
TAIL_ROWS = {
    ('bf16', 35, 64): (1, 2), ('bf16', 1281, 64): (8, 9), ('bf16', 1283, 64): (8, 9), ('bf16', 1290, 64): (8, 9),
    ('bf16', 35, 72): (1, 2), ('bf16', 1281, 72): (13, 14), ('bf16', 1283, 72): (13, 14), ('bf16', 1290, 72): (14, 15),
    ('fp32', 35, 64): (2, 3), ('fp32', 1281, 64): (0, 1), ('fp32', 1283, 64): (0, 1), ('fp32', 1292, 64): (0, 1),
    ('fp32', 35, 24): (0, 1), ('fp32', 1281, 24): (14, 15), ('fp32', 1283, 24): (14, 15), ('fp32', 1292, 24): (14, 15),
}
ROWWALK_HW = {'bf16': (35, 1281, 1283, 1290), 'fp32': (35, 1281, 1283, 1292)}
ROWWALK_C = {'bf16': (64, 72), 'fp32': (64, 24)}
SMALL_HW = (1, 35, 256, 289, 1280)
SMALL_NC = {'bf16': ((2, 8), (2, 72)), 'fp32': ((2, 4), (2, 72))}
SMALL_G8 = {'bf16': (3, 35, 4096), 'fp32': (3, 35, 2048)}
LONG_SMALL = (2, 4100, 64)                             # S2E_IN_SMALL_HW=100000
ZBLOCKS2 = {'bf16': (1, 1281, 2056), 'fp32': (1, 1281, 1028)}
WRAP = {'bf16': (64, 4100, 64), 'fp32': (64, 4100, 32)}
FORM_SHAPES = ((2, 1281, 64), (2, 35, 72))
UP_ROWWALK, UP_SMALL = (36, 36), (16, 18)
PARTIALS_P, PARTIALS_C = (1, 7, 16, 33, 130), (16, 24, 130)
COLSUM = {'bf16': ((1, 64), (2049, 64), (4097, 72), (300, 2056), (1025, 1), (5000, 3), (70000, 1)),
          'fp32': ((1, 64), (2049, 64), (4097, 72), (300, 1028), (1025, 1), (5000, 3), (70000, 1))}


# ---- helpers
def up2(x, H, W):
    """x (N, H/2 * W/2, C) -> nearest 2x upsampling (N, H * W, C)"""
    n, _, c = x.shape
    return x.view(n, H // 2, W // 2, c).repeat_interleave(2, 1).repeat_interleave(2, 2).reshape(n, H * W, c)


def quad_sum(t, H, W, take=4):
    """(N, H * W, C) -> (N, H/2 * W/2, C): the sum over each 2 x 2 block (take < 4: a mutant that leaves pixels out)"""
    n, _, c = t.shape
    v = t.view(n, H // 2, 2, W // 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(n, H // 2, W // 2, 4, c)
    return v[:, :, :, :take].sum(3).reshape(n, (H // 2) * (W // 2), c)


def lrelu(v):
    return torch.where(v > 0, v, 0.2 * v)


def norm_terms(x, stats):
    mean, rstd = stats[:, None, :, 0], stats[:, None, :, 1]
    return mean, rstd, (x - mean) * rstd, (x.abs() + mean.abs()) * rstd


def bound_out(ref, A, dt, extra=None):
    b = U[dt] * ref.abs() + C_ACC * A
    return b if extra is None else b + extra


def bound_sum(ref, A_sum, start=None):
    b = F32_RNE * ref.abs() + C_ACC * A_sum
    return b if start is None else b + F32_RNE * start.abs()


# ---- statistics
def stats_ref(x, eps=EPS, batch=False):
    """x (N, HW, C) fp64 -> dict: s, q (the sums), their absolute twins As, Aq, mean, var, rstd and the bounds d_*; batch: over N too"""
    dims = (0, 1) if batch else 1
    cnt = x.shape[1] * (x.shape[0] if batch else 1)
    return stats_from_sums(x.sum(dims), (x * x).sum(dims), x.abs().sum(dims), (x * x).sum(dims), cnt, eps)


def stats_from_sums(s, q, As, Aq, cnt, eps=EPS):
    mean = s / cnt
    var = (q / cnt - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    d_mean = F32_RNE * mean.abs() + C_ACC * As / cnt
    d_var = C_ACC * (Aq / cnt + 2 * mean.abs() * As / cnt)
    rel_rstd = d_var / (2 * (var + eps)) + F32_RNE
    return dict(s=s, q=q, As=As, Aq=Aq, mean=mean, var=var, rstd=rstd, d_s=bound_sum(s, As), d_q=bound_sum(q, Aq), d_mean=d_mean,
                rel_rstd=rel_rstd, d_rstd=rstd * rel_rstd)


def instance_norm_fwd_ref(x, lrelu_on, dt, eps=EPS):
    """out = [lrelu]((x - mean) * rstd) with its own statistics: (out, bound, stats dict)"""
    st = stats_ref(x, eps)
    mean, rstd = st['mean'][:, None], st['rstd'][:, None]
    xh = (x - mean) * rstd
    A = xh.abs()
    out = lrelu(xh) if lrelu_on else xh
    extra = rstd * st['d_mean'][:, None] + xh.abs() * st['rel_rstd'][:, None]
    return out, bound_out(out, A, dt, extra), st


# ---- modulation forward (statistics are an input)
def modulate_fwd_ref(x, gb, stats, s0, s1, mode, lrelu_on):
    """(out, A, pre, A_pre): pre = the LeakyReLU's argument"""
    _, _, xh, _ = norm_terms(x, stats)
    xh_a = xh.abs()
    if mode == PLAIN:
        pre, A = xh, xh_a
    else:
        C = x.shape[-1]
        ga, be = gb[..., :C], gb[..., C:]
        pre = 0.5 * (xh * (1 + ga) + be + x * (1 + s0[:, None]) + s1[:, None])
        A = 0.5 * (xh_a * (1 + ga.abs()) + be.abs() + x.abs() * (1 + s0.abs()[:, None]) + s1.abs()[:, None])
    return (lrelu(pre) if lrelu_on else pre), A, pre, A


# ---- modulation backward, every form
def modulate_bwd_ref(t, mode, lrelu_on, gamma_only=False, batch=False, batch_count=0.0, other=None, up=None, quad=False,
                     dx_start=None, mut=None, drop_from=None):
    """t: fp64 g, x, gb ((N, HW, 2C) or gamma alone), fout, stats (N, C, 2), s0, s1 (N, C).
    batch: S0, S1 summed over the samples (+ `other` = (S0, S1, A0, A1) per channel of further replicas), count batch_count or N * HW.
    up = (H, W): x is at half resolution; quad: dx at half resolution too.  dx_start: ACCUMULATE_DX.  mut: one of MUTANTS.
    Returns dict of (ref, A) pairs: dx, dgb (SPADE), sums (N, C, 4), dstyle (N, 2C: the gradient alone), and `readback` (SPADE)."""
    g = t['g']
    N, HW, C = g.shape
    x = t['x'] if up is None else up2(t['x'], *up)
    mean, rstd, xh, xh_a = norm_terms(x, t['stats'])
    spade = mode == SPADE
    if spade:
        ga = t['gb'][..., :C]
        G, Ga = 1 + ga, 1 + ga.abs()
        s0, s1 = (t['s1'], t['s0']) if mut == 'swap_s' else (t['s0'], t['s1'])
        a, aa = 1 + s0[:, None], 1 + s0.abs()[:, None]
        if gamma_only:
            arg = t['fout']
        else:
            arg = 0.5 * (xh * G + t['gb'][..., C:] + x * a + s1[:, None])
    else:
        arg = x - mean                                      # xhat > 0 <=> x > mean, exact on the given fp32 mean
    pos = (arg >= 0) if mut == 'mask1' else (arg > 0)
    go = torch.where(pos, g, 0.2 * g) if lrelu_on else g
    if spade:
        gn, gna = 0.5 * go * G, 0.5 * go.abs() * Ga
    else:
        gn, gna = go, go.abs()
    w = torch.ones(N, HW, 1, dtype=torch.float64)
    if mut == 'drop_row':
        w[0, HW - 1:] = 0
    if mut == 'drop_slot':
        w[0, drop_from:] = 0
    z = torch.zeros(N, C, dtype=torch.float64)
    S = torch.stack([(gn * w).sum(1), (gn * xh * w).sum(1), (go * x * w).sum(1) if spade else z, (go * w).sum(1) if spade else z], -1)
    AS = torch.stack([gna.sum(1), (gna * xh.abs()).sum(1), (go * x).abs().sum(1) if spade else z, go.abs().sum(1) if spade else z], -1)
    S0, S1, A0, A1, cnt = S[..., 0], S[..., 1], AS[..., 0], AS[..., 1], float(HW)
    if batch:
        S0, S1, A0, A1 = (v.sum(0, keepdim=True) for v in (S0, S1, A0, A1))
        if other is not None:
            S0, S1, A0, A1 = S0 + other[0], S1 + other[1], A0 + other[2], A1 + other[3]
        cnt = float(N * HW) if (mut == 'no_batch_count' or not batch_count) else float(batch_count)
    if mut == 'hw1':
        cnt += float(N if batch else 1)
    dx = rstd * (gn - (S0 / cnt)[:, None] - xh * (S1 / cnt)[:, None])
    A = rstd * (gna + (A0 / cnt)[:, None] + xh_a * (A1 / cnt)[:, None])
    res = {'sums': (S, AS)}
    rb = None
    if spade:
        dx = dx + 0.5 * go * a
        A = A + 0.5 * go.abs() * aa
        rb = (0.5 * go * (a + rstd * G)).abs()
        dga = 0.5 * go * (x if mut == 'dgamma_x' else xh)
        res['dgb'] = (torch.cat([dga, 0.5 * go], -1), torch.cat([0.5 * go.abs() * xh.abs(), 0.5 * go.abs()], -1))
        res['dstyle'] = (torch.cat([0.5 * S[..., 2], 0.5 * S[..., 3]], -1), torch.cat([0.5 * AS[..., 2], 0.5 * AS[..., 3]], -1))
    if quad:
        take = 3 if mut == 'quad3' else 4
        dx, A = quad_sum(dx, *up, take=take), quad_sum(A, *up)
        rb = quad_sum(rb, *up)
    if dx_start is not None:
        if mut != 'no_dx_add':
            dx = dx + dx_start
        A = A + dx_start.abs()
    res['dx'] = (dx, A)
    res['readback'] = rb
    return res


def dx_bound(res, dt, rowwalk):
    """the bound of dx: the dbeta read-back term for the row-walk SPADE path only"""
    dx, A = res['dx']
    extra = BF16_RNE * res['readback'] if (rowwalk and dt == 'bf16' and res['readback'] is not None) else None
    return bound_out(dx, A, dt, extra)


# ---- input generators (CPU tensors in the kernel's dtypes)
def make_case(dt, N, HW, C, seed, edge=None, up=None, ld=0, off=0, batch=False, lrelu_on=True):
    """dict: x ((N, HW | HW/4, C)), g, gb (N, HW, 2C), gamma, fout in the compute dtype; style (N, ld or 2C) fp32, stats (N, C, 2) fp32
    computed in fp64 from the full-resolution x and rounded (batch: batch-wide, repeated per sample).
    edge: 'const0' / 'const1.5' (channel 0 exactly constant), 'shifted' (channel 1: x = 3 + 0.5 randn, mean / std ~ 6)."""
    gen = torch.Generator().manual_seed(seed)
    tdt = TDT[dt]
    hwx = HW // 4 if up else HW
    x = torch.randn(N, hwx, C, generator=gen) * 1.3 + 0.2
    if edge == 'const0':
        x[..., 0] = 0.0
    elif edge == 'const1.5':
        x[..., 0] = 1.5
    elif edge == 'shifted':
        x[..., 1 % C] = 3.0 + 0.5 * torch.randn(N, hwx, generator=gen)
    x = x.to(tdt)
    g = (torch.randn(N, HW, C, generator=gen) + 0.5).to(tdt)       # a mean well off zero: the backward's per-channel means matter
    gb = (torch.randn(N, HW, 2 * C, generator=gen) * 0.5).to(tdt)
    width = ld if ld else 2 * C
    style = (torch.randn(N, width, generator=gen) * 0.5).float()
    st = stats_ref(x.double(), EPS, batch)
    stats = torch.stack([st['mean'], st['rstd']], -1)
    if batch:
        stats = stats.unsqueeze(0).expand(N, C, 2)
    case = dict(dt=dt, N=N, HW=HW, C=C, up=up, off=off, x=x, g=g, gb=gb.contiguous(), style=style, stats=stats.float().contiguous(),
                gen=gen, redrawn=0)
    return case


def widen(case):
    """the fp64 view of a case's operands, as modulate_*_ref take them"""
    C, off = case['C'], case['off']
    t = {k: case[k].double() for k in ('x', 'g', 'gb', 'stats')}
    t['s0'], t['s1'] = case['style'][:, off:off + C].double(), case['style'][:, off + C:off + 2 * C].double()
    if 'fout' in case:
        t['fout'] = case['fout'].double()
    return t


def kink_band(case):
    """elements of the gb-form SPADE LeakyReLU argument within KINK_BAND * A_pre of zero"""
    t = widen(case)
    x = t['x'] if case['up'] is None else up2(t['x'], *case['up'])
    _, _, pre, A_pre = modulate_fwd_ref(x, t['gb'], t['stats'], t['s0'], t['s1'], SPADE, False)
    return pre.abs() < KINK_BAND * A_pre


def clear_kink_band(case):
    """re-draw beta by +-0.25 wherever the mask's argument is inside the band (the kernel recomputes it in fp32 there); returns the case"""
    C = case['C']
    for _ in range(16):
        m = kink_band(case)
        n = int(m.sum())
        if not n:
            return case
        case['redrawn'] += n
        beta = case['gb'][..., C:].float()
        sign = torch.where(torch.rand(m.shape, generator=case['gen']) < 0.5, -0.25, 0.25)
        case['gb'][..., C:] = torch.where(m, beta + sign, beta).to(case['gb'].dtype)
    raise AssertionError('the kink band did not clear')


def add_gamma_only(case, lrelu_on=True):
    """the gamma-only form's operands: gamma alone and the forward's output `fout` in the compute dtype, some of it exactly +-0"""
    C = case['C']
    t = widen(case)
    x = t['x'] if case['up'] is None else up2(t['x'], *case['up'])
    out = modulate_fwd_ref(x, t['gb'], t['stats'], t['s0'], t['s1'], SPADE, lrelu_on)[0]
    fout = out.to(case['gb'].dtype).contiguous()
    flat = fout.view(-1)
    flat[::101] = 0.0
    flat[50::101] = -0.0
    case['fout'] = fout
    case['gamma'] = case['gb'][..., :C].contiguous()
    return case


def gamma_only_operands(case):
    """widen() with gb replaced by gamma alone"""
    t = widen(case)
    t['gb'] = case['gamma'].double()
    return t
