"""fp64 references, bounds and label-map builders for the small kernels of the label-sparse SPADE path -- s2e_label_rect_classify,
s2e_spade_class_table[_batch], s2e_spade_modulate_uniform (csrc/label_ops.hip), s2e_label_rect_lists_bwd, s2e_spade_uniform_sums,
s2e_spade_uniform_grads (csrc/spade_sparse_bwd.hip).  CPU only: numpy for the integer rules, torch fp64 for the sums.
tests/_spade_sparse_child.py runs the kernels against these on the GPU; tests/test_spade_sparse_ref_host.py proves on the CPU that the
references are autograd's and that each bound catches the mistake it is there for.

Bounds.  Integer outputs (cls, lists, counts) must be equal; the stored gamma must be bit-equal to the table value rounded to the
output dtype.  A floating-point output must satisfy, per element,

    |got - ref| <= rnd |ref| + C_ACC (A + |start|)

rnd = 2^-8 for a bf16 output (its RNE rounding) and 0 for fp32; A is the same computation on absolute values, so every fp32 partial
result is at most A; |start| is what an accumulated target held before the call.  C_ACC = 2^-16 = 256 fp32 half-ulps is the allowance
tests/_conv3x3_child.py derives for sums of up to 9216 terms.  Here it holds in the strict sense as well: the fp32 error of a sum is at
most sum_i |term_i| d_i 2^-24, d_i the number of roundings term i passes through on its way into the result, so C_ACC covers every
output whose longest chain is at most 256 roundings.  The chains, counted from the kernels (the `chain` constants below):

  table     per lane 9 taps x (2 products, 1 add, 1 add into the position class) = 36, the DPP fold of 64 lanes 6, the bias 1:   43
            (bf16 operands: the products are exact, the chain is shorter)
  modulate  x - mean, * rstd, 1 + gamma, *, + beta, 1 + s0, x *, +, + s1, 0.5 *, 0.2 *:                                         11
  sums      a row of 16 pixels 16, the two slides 4, 16 rows into a window 16, up to 8 row slices folded 8, the atomic adds of
            ceil(n / 16) rectangles per replica (n <= 32 here) 2, the start value 1:                                            47
            -- and what the test adds up itself in fp64 (the 16 replicas) costs nothing
  grads     A[c][k]: the fold of 16 replicas 16, per block 8 channels x 9 taps x (product + add) 144, one atomic add per block of
            8 channels 2C / 8; then + 1 for the += into dw_sh, + ncls <= 4 and 1 for db_sh:                          165 + 2C / 8
            -- at 2C = 1024 that is 293, LONGER than 256, so there A, dw_sh and db_sh get GEMV_ACC = 2^-15 (512 roundings)
            instead: grads_acc(2C)
            dw_gb / db_gb: the fold 16, ncls products and adds 8, the += 1:                                                     25
  chain     sums then grads at 2C = 128 (16 blocks): 47 + 16 + 144 + 16 + 5 = 228 for dw_sh / db_sh, 47 + 25 for dw_gb / db_gb

Exactness.  w_sh and b_sh are drawn on a grid (grid_weights: multiples of 2^-7 below 2 in magnitude), so the ten-term pre-activation
b + sum of nine taps is a multiple of 2^-7 below 20: 12 significant bits, exact in fp32 in any order and equal to the fp64 sum.  The
ReLU mask and the bf16 rounding of the hidden activation (torch's RNE .to(bfloat16)) are therefore the same on both sides, and no
element has to be excused."""
import numpy as np
import torch
import torch.nn.functional as F

C_ACC = 2.0 ** -16                  # fp32 chains of up to 256 roundings, x A
GEMV_ACC = 2.0 ** -15               # s2e_spade_uniform_grads' A at 2C > 728 (see above)
BF16_RNE = 2.0 ** -8
UNI_REPLICAS = 16                   # S2E_UNI_REPLICAS of include/seg2eye_hip.h
DENSE = 255                         # cls of a rectangle that is not label-uniform
CHAIN = {'table': 43, 'modulate': 11, 'sums': 47, 'grads_gb': 25, 'chain_sh': 228, 'chain_gb': 72}
assert all(v <= 256 for v in CHAIN.values())


def grads_chain(C2):
    """the longest chain of fp32 roundings behind A / dw_sh / db_sh of s2e_spade_uniform_grads (see above)"""
    return 16 + 144 + -(-C2 // 8) + 5


def grads_acc(C2):
    n = grads_chain(C2)
    assert n <= 512
    return C_ACC if n <= 256 else GEMV_ACC


def rel_of(dtype):
    return BF16_RNE if dtype == torch.bfloat16 else 0.0


# ---- label maps
def block_labels(N, H, W, ncls=4):
    """(N, H, W) uint8: the class by quadrant (boundaries at H/2, W/2), rotated by the sample index so that samples differ"""
    y = (np.arange(H) >= H // 2).astype(np.int64)[:, None]
    x = (np.arange(W) >= W // 2).astype(np.int64)[None, :]
    q = 2 * y + x
    return np.stack([(q + n) % ncls for n in range(N)]).astype(np.uint8)


def salt(lab, points, ncls=4):
    """a copy of lab with the single pixels `points` = [(n, y, x)] set to another class"""
    out = lab.copy()
    for n, y, x in points:
        out[n, y, x] = (int(lab[n, y, x]) + 1) % max(ncls, 2)
    return out


def upsample_salted(lab, s, ncls=4):
    """lab (N, h, w) -> (N, s h, s w) whose pixel (s y, s x) is lab[y, x] and whose every other pixel is ANOTHER class: what the
    nearest downsampling skips must not matter"""
    if s == 1:
        return lab.copy()
    up = lab.repeat(s, 1).repeat(s, 2)
    other = ((up.astype(np.int64) + 1) % max(ncls, 2)).astype(np.uint8)
    yy = (np.arange(up.shape[1]) % s != 0)[:, None]
    xx = (np.arange(up.shape[2]) % s != 0)[None, :]
    return np.where(yy | xx, other, up)


# ---- the integer rules
def classify_ref(label, h, w, tw, th, skip_corners=False):
    """The rule of include/seg2eye_hip.h: rectangle r = (n tiles_y + ty) tiles_x + tx of the nearest-downsampled map (pixel (y, x) =
    label[y H/h, x W/w]) is uniform when its pixels and the in-image part of its 2-pixel halo carry one class.
    -> cls (uint8: class | 255), dense list, uniform list (ascending).  skip_corners: the MISTAKE of the host test -- the four 2 x 2
    diagonal corners of the halo are not looked at."""
    N, H, W = label.shape
    assert H % h == 0 and W % w == 0
    down = label[:, ::H // h, ::W // w]
    tiles_y, tiles_x = -(-h // th), -(-w // tw)
    cls = np.empty(N * tiles_y * tiles_x, dtype=np.uint8)
    for n in range(N):
        for ty in range(tiles_y):
            for tx in range(tiles_x):
                y0, y1, x0, x1 = ty * th, min(h, ty * th + th), tx * tw, min(w, tx * tw + tw)
                ya, yb, xa, xb = max(0, y0 - 2), min(h, y1 + 2), max(0, x0 - 2), min(w, x1 + 2)
                reg = down[n, ya:yb, xa:xb]
                if skip_corners:
                    keep = np.ones(reg.shape, dtype=bool)
                    yy = np.arange(ya, yb)[:, None]
                    xx = np.arange(xa, xb)[None, :]
                    keep &= ~(((yy < y0) | (yy >= y1)) & ((xx < x0) | (xx >= x1)))
                    vals = reg[keep]
                else:
                    vals = reg.ravel()
                cls[(n * tiles_y + ty) * tiles_x + tx] = vals[0] if (vals == vals[0]).all() else DENSE
    r = np.arange(cls.size, dtype=np.int32)
    return cls, r[cls == DENSE], r[cls != DENSE]


def lists_bwd_ref(cls, N, tiles_y, tiles_x):
    """-> work list (dense, or uniform on the image border), uniform-interior list; ascending"""
    r = np.arange(N * tiles_y * tiles_x, dtype=np.int32)
    rr = r % (tiles_y * tiles_x)
    ty, tx = rr // tiles_x, rr % tiles_x
    ui = (cls != DENSE) & (ty > 0) & (ty < tiles_y - 1) & (tx > 0) & (tx < tiles_x - 1)
    return r[~ui], r[ui]


def rect_pixels(ids, N, H, W, tw, th):
    """(N, H, W) bool: the pixels of the rectangles `ids` of the tw x th tiling"""
    tiles_y, tiles_x = -(-H // th), -(-W // tw)
    m = np.zeros(N * tiles_y * tiles_x, dtype=bool)
    m[np.asarray(ids, dtype=np.int64)] = True
    return m.reshape(N, tiles_y, tiles_x).repeat(th, 1).repeat(tw, 2)[:, :H, :W]


def rect_class_map(cls, N, H, W, tw, th):
    """(N, H, W) int64: the class of each pixel's rectangle (255 in a dense one)"""
    tiles_y, tiles_x = -(-H // th), -(-W // tw)
    return cls.astype(np.int64).reshape(N, tiles_y, tiles_x).repeat(th, 1).repeat(tw, 2)[:, :H, :W]


# ---- operands
def grid_weights(shape, g):
    """multiples of 2^-7 with magnitude below 2 (see Exactness), float64"""
    return torch.randint(-255, 256, shape, generator=g).double() / 128.0


def round_to(v, dtype):
    """v (float64) as the kernels store it in `dtype`: RNE"""
    return v.float().to(dtype).double()


def hidden_act(w_sh, b_sh, act_dtype):
    """a_c[c][k] = ReLU(b_sh[k] + the nine taps of w_sh[k][c]) as the dense path stores it: (ncls, nh) float64"""
    pre = b_sh[None, :] + w_sh.sum((2, 3)).t()
    return round_to(torch.relu(pre), act_dtype)


# ---- s2e_spade_class_table
TABLE_POS = (0, 1, 3, 5, 6)          # pixels of a 7-pixel axis: the two rings at either border and the interior


def table_ref(w_sh, b_sh, wq, bias, act_dtype):
    """The [gamma | beta] branch -- one-hot, conv3x3 (w_sh, b_sh), ReLU, rounded to act_dtype, conv3x3 (wq, bias) -- on a 7 x 7 map of
    one class, read at the five position classes of either axis.  w_sh (nh, ncls, 3, 3), wq (2C, nh, 3, 3) the values the conv
    launches multiply with, bias (2C) or None; all float64.  -> table (ncls, 5, 5, 2C) and its absolute-value twin."""
    nh, ncls = w_sh.shape[:2]
    onehot = torch.zeros(ncls, ncls, 7, 7, dtype=torch.float64)            # batch entry c = the map of class c
    for c in range(ncls):
        onehot[c, c] = 1.0
    act = round_to(torch.relu(F.conv2d(onehot, w_sh, b_sh, padding=1)), act_dtype)
    gb = F.conv2d(act, wq, bias, padding=1)
    ab = F.conv2d(act.abs(), wq.abs(), bias.abs() if bias is not None else None, padding=1)
    pos = torch.tensor(TABLE_POS)
    pick = lambda t: t[:, :, pos][:, :, :, pos].permute(0, 2, 3, 1).contiguous()
    return pick(gb), pick(ab)


# ---- s2e_spade_modulate_uniform
def pos_class(i, n):
    """{0, 1, interior, n-2, n-1} -> 0..4"""
    i = np.asarray(i)
    return np.where(i < 2, i, np.where(i >= n - 2, 4 - (n - 1 - i), 2))


def modulate_ref(x_full, stats, s0, s1, table, cmap, lrelu_on):
    """out = [lrelu] 0.5 ((x - mean) rstd (1 + gamma) + beta + x (1 + s0) + s1) with gamma | beta = table[class][cy][cx] (the formula of
    csrc/label_ops.hip).  x_full (N, H, W, C), stats (N, C, 2) = mean, rstd, s0 / s1 (N, C), table (ncls, 5, 5, 2C), all float64; cmap
    (N, H, W) the class of each pixel's rectangle (dense pixels: any valid class; the caller masks them).
    -> out, its absolute-value twin, gamma (the fp32 table value of each pixel, float64)"""
    N, H, W, C_ = x_full.shape
    cy = torch.as_tensor(pos_class(np.arange(H), H))[None, :, None].expand(N, H, W)
    cx = torch.as_tensor(pos_class(np.arange(W), W))[None, None, :].expand(N, H, W)
    gb = table[torch.as_tensor(cmap), cy, cx]                              # (N, H, W, 2C)
    gamma, beta = gb[..., :C_], gb[..., C_:]
    mean, rstd = stats[:, None, None, :, 0], stats[:, None, None, :, 1]
    s0_, s1_ = s0[:, None, None, :], s1[:, None, None, :]
    out = 0.5 * ((x_full - mean) * rstd * (1 + gamma) + beta + x_full * (1 + s0_) + s1_)
    a_out = 0.5 * ((x_full.abs() + mean.abs()) * rstd.abs() * (1 + gamma.abs()) + beta.abs() + x_full.abs() * (1 + s0_.abs()) + s1_.abs())
    if lrelu_on:
        out = torch.where(out > 0, out, 0.2 * out)
    return out, a_out, gamma


# ---- s2e_spade_uniform_sums
def sums_ref(dgb, cls, ui, H, W, ncls, swap_taps=False, drop_row=None):
    """R[c][t][co] = sum over the uniform-interior 16 x 16 rectangles `ui` of class c, over their pixels q, of dgb[q - t + 1], tap
    t = 3 ky + kx, i.e. the rectangle shifted by (1 - ky, 1 - kx).  dgb (N, H, W, 2C) float64.  -> R (ncls, 9, 2C) and its
    absolute-value twin.  The MISTAKES of the host test: swap_taps stores tap t where 8 - t belongs; drop_row = (i, t, row) leaves
    one row out of window t of the i-th rectangle."""
    tiles_y, tiles_x = H // 16, W // 16
    C2 = dgb.shape[-1]
    R = torch.zeros(ncls, 9, C2, dtype=torch.float64)
    A = torch.zeros(ncls, 9, C2, dtype=torch.float64)
    for i, r in enumerate(int(v) for v in ui):
        n, rr = divmod(r, tiles_y * tiles_x)
        ty, tx = divmod(rr, tiles_x)
        c = int(cls[r])
        for t in range(9):
            ky, kx = divmod(t, 3)
            y0, x0 = ty * 16 + 1 - ky, tx * 16 + 1 - kx
            win = dgb[n, y0:y0 + 16, x0:x0 + 16]
            if drop_row is not None and drop_row[:2] == (i, t):
                win = torch.cat([win[:drop_row[2]], win[drop_row[2] + 1:]])
            slot = 8 - t if swap_taps else t
            R[c, slot] += win.sum((0, 1))
            A[c, slot] += win.abs().sum((0, 1))
    return R, A


def neighbourhood_mask(ui, N, H, W):
    """(N, H, W) bool: the 18 x 18 neighbourhoods of the rectangles `ui` -- all that s2e_spade_uniform_sums may read"""
    tiles_y, tiles_x = H // 16, W // 16
    m = np.zeros((N, H, W), dtype=bool)
    for r in (int(v) for v in ui):
        n, rr = divmod(r, tiles_y * tiles_x)
        ty, tx = divmod(rr, tiles_x)
        m[n, ty * 16 - 1:ty * 16 + 17, tx * 16 - 1:tx * 16 + 17] = True
    return m


# ---- s2e_spade_uniform_grads
def grads_ref(R, R_abs, w_gb, w_sh, b_sh, act_dtype, rank1_tap=4, ignore_mask=False):
    """The formulas of csrc/spade_sparse_bwd.hip from the folded sums R (ncls, 9, 2C): with a_c = hidden_act and m_c = [a_c > 0],
        A[c][k]          = sum_{t, co} w_gb[co][k][t] R[c][t][co]
        dw_sh[k][c][t]  += m_c[k] A[c][k]   (every tap)         db_sh[k]  += sum_c m_c[k] A[c][k]
        dw_gb[co][k][t] += sum_c R[c][4][co] a_c[k]  (every tap) db_gb[co] += sum_c R[c][4][co]
    w_gb (2C, nh, 3, 3), w_sh (nh, ncls, 3, 3), b_sh (nh), float64.  R_abs: the sums of |.| (the replicas' |R| added up).
    -> {name: (increment, absolute-value twin)}.  The MISTAKES of the host test: rank1_tap != 4, ignore_mask."""
    C2, nh = w_gb.shape[:2]
    ncls = w_sh.shape[1]
    a_c = hidden_act(w_sh, b_sh, act_dtype)                                # (ncls, nh)
    wm = w_gb.reshape(C2, nh, 9)
    acc = torch.einsum('okt,cto->ck', wm, R)
    acc_abs = torch.einsum('okt,cto->ck', wm.abs(), R_abs)
    m = torch.ones_like(a_c) if ignore_mask else (a_c > 0).double()
    v = m * acc
    rc, rc_abs = R[:, rank1_tap], R_abs[:, rank1_tap]                      # (ncls, 2C)
    gb = torch.einsum('co,ck->ok', rc, a_c)
    gb_abs = torch.einsum('co,ck->ok', rc_abs, a_c.abs())
    nine = lambda t: t[..., None, None].expand(*t.shape, 3, 3).contiguous()
    return {'A': (acc, acc_abs),
            'dw_sh': (nine(v.t()), nine((m * acc_abs).t())), 'db_sh': (v.sum(0), (m * acc_abs).sum(0)),
            'dw_gb': (nine(gb), nine(gb_abs)), 'db_gb': (rc.sum(0), rc_abs.sum(0))}


def branch_autograd(label, w_sh, b_sh, w_gb, dgb, pix_mask, act_dtype):
    """What autograd gives for the pixels `pix_mask` (N, H, W bool): the plain fp64 branch gb = conv3x3(round(ReLU(conv3x3(one-hot) +
    b_sh)), w_gb) with loss = sum gb . dgb, the gradient at the hidden pre-activation masked to pix_mask by a hook -> dw_sh, db_sh;
    and the weight / bias gradient of the [gamma | beta] conv for dgb masked to the same pixels -> dw_gb, db_gb.
    label (N, H, W) uint8, dgb (N, H, W, 2C) float64.  (The rounding passes the gradient straight through; its ReLU mask is that of
    the pre-activation, which on grid_weights is the mask of the rounded value.)"""
    ncls = w_sh.shape[1]
    lab = torch.as_tensor(label.astype(np.int64))
    onehot = F.one_hot(lab, ncls).permute(0, 3, 1, 2).double()
    g = dgb.permute(0, 3, 1, 2)
    pm = torch.as_tensor(pix_mask)[:, None].double()
    w1, b1 = w_sh.clone().requires_grad_(True), b_sh.clone().requires_grad_(True)
    pre = F.conv2d(onehot, w1, b1, padding=1)
    pre.register_hook(lambda gr: gr * pm)
    act = torch.relu(pre)
    act_q = act + (round_to(act.detach(), act_dtype) - act.detach())
    (F.conv2d(act_q, w_gb, None, padding=1) * g).sum().backward()
    w2 = w_gb.clone().requires_grad_(True)
    b2 = torch.zeros(w_gb.shape[0], dtype=torch.float64, requires_grad=True)
    (F.conv2d(act_q.detach(), w2, b2, padding=1) * (g * pm)).sum().backward()
    return {'dw_sh': w1.grad, 'db_sh': b1.grad, 'dw_gb': w2.grad, 'db_gb': b2.grad}


# ---- the comparison
def check_close(got, ref, A, what, rel, acc=C_ACC, start=None):
    """Every element: |got - (start +) ref| <= rel |ref| + acc (A + |start|); NaN fails.  got / ref / A / start: float64 CPU tensors of
    one shape.  -> the worst err / bound."""
    assert got.shape == ref.shape == A.shape, (what, got.shape, ref.shape, A.shape)
    assert float(A.max()) > 0, '%s: empty reference' % what
    scale = A
    if start is not None:
        got = got - start
        scale = A + start.abs()
    bound = rel * ref.abs() + acc * scale
    err = (got - ref).abs()
    ok = err <= bound
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError('%s: %d of %d elements outside the bound; first at %s: got %r, ref %r, A %r, bound %.3e'
                             % (what, bad.shape[0], ok.numel(), i, float(got[i]), float(ref[i]), float(A[i]), float(bound[i])))
    return float((err / bound.clamp_min(1e-300)).max())
