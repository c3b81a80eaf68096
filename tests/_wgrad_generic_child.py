#!/usr/bin/env python3
"""The generic weight-gradient kernel -- csrc/conv_wgrad.hip: conv_wgrad_kernel (bf16 and fp32, vector and scalar gather), its
fixed-order reduction conv_wgrad_reduce_kernel, and the multi-job forms conv_wgrad_multi_kernel / conv_wgrad_reduce_multi_kernel --
against fp64, element by element, through s2e_conv2d_wgrad and s2e_conv2d_wgrad_multi at the C ABI.

Run by tests/test_wgrad_generic_fp64_gpu.py as a child process per environment, because the library reads its switches once per
process (S2E_WGRAD_PARTIAL, S2E_DETERMINISTIC; S2E_WGRAD_PATCH, S2E_WGRAD_C8 and S2E_WGRAD_MULTI_WGS must be unset):

    python tests/_wgrad_generic_child.py --groups big,mid,one                     (no switch: the shipped thresholds)
    python tests/_wgrad_generic_child.py --groups big,mid                         (S2E_WGRAD_PARTIAL=2: every split launch reduces)
    python tests/_wgrad_generic_child.py --groups big                             (S2E_WGRAD_PARTIAL=0: atomics only)
    python tests/_wgrad_generic_child.py --groups det,multi                       (S2E_DETERMINISTIC=1: every launch reduces)
    python tests/_wgrad_generic_child.py --groups big,mid,one,det,multi --plan    (no GPU: routes and workspace sizes only)

Reference.  The fp64 weight gradient on the CPU of exactly the operands the MFMA multiplies: x and gy as stored (bf16 or fp32) widened
to float64; with in_act = LRELU the x operand is the compute-dtype rounding of the fp32 product 0.2f * x (operand64 of
tests/_conv_generic_child.py: the kernel rounds it back before the MFMA).  ref_b = sum of gy over the pixels.  A and A_b are the same
sums over absolute values.  dw is [Cout][KH KW Cin] with k = (ky KW + kx) Cin + ci.

Bound, per element, none skipped:  |got - (start + ref)| <= C_ACC (A + |start|),  C_ACC = 2^-16 of tests/_conv3x3_child.py, rel = 0.
Linear worst case, on that file's premise that an accumulator update costs one rounding of at most 2^-24 of the running magnitude
(<= A + |start|): a pixel split accumulates ceil(m_per_split / 16) MFMA updates in bf16 (products of bf16 values are exact in fp32)
or ceil(m_per_split / 2) in fp32 (whose product roundings together cost at most one more unit), the splits are combined in at most
`splits` further roundings (atomics; the fixed-order reduce needs fewer), and one more covers the add into `start`:
    depth = ceil(m_per_split / (16 | 2)) + splits + 2 (+ 1 for fp32),        depth <= 256  <=>  depth 2^-24 <= C_ACC.
The bias sum: a thread adds the rows it stages of every tiles_k-th chunk (2 rows a chunk in bf16, 4 in fp32), 16 (8) such threads
are added up through LDS, then the splits x tiles_k partial sums and `start`:
    bias_depth = ceil(ceil(m_per_split / 32) / tiles_k) (2 | 4) + (16 | 8) + splits tiles_k + 1  <=  256.
Both are asserted for every shipped case by tests/test_wgrad_generic_references.py; a case that does not satisfy them is shrunk.

Guards.  dw and dbias accumulate: they start from random non-zero values inside Guarded buffers.  The workspace is NaN-poisoned and
guarded and comes in three forms: `exact` (what s2e_conv2d_wgrad_workspace_bytes reports), `short` (256 bytes fewer: the kernel must
fall back to atomics and still be right) and `none` (NULL, 0).  Every launch is made twice; the results must be bit-identical where the
code promises it: dw and dbias where the reduce ran (exact workspace and the mirror says partial tiles), dw alone where splits == 1.

Route.  plan() mirrors wgrad_params + generic_wgrad_plan, use_partial() wgrad_use_partial, partial_bytes() generic_partial_bytes and
multi_plan() wgrad_chunk_plan with its target_override; every case asserts S2E_KERNEL_GENERIC and that the library's workspace query
equals the mirror's.  The mirror also counts what the shipped lists exercise (coverage()): no counter may be zero.
Prints 'wgrad generic ok: ...' last."""
import argparse
import ctypes as C
import json
import os
import sys
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch                                   # noqa: E402
import torch.nn.functional as F                # noqa: E402

from _conv3x3_child import C_ACC, Guarded, check_close, workspace                  # noqa: E402
from _conv_generic_child import ACT_LRELU, ACT_NONE, KERNEL_GENERIC, S2E_BF16, S2E_F32, ceil_div, operand64   # noqa: E402

SWITCHES = ('S2E_WGRAD_PARTIAL', 'S2E_WGRAD_PATCH', 'S2E_WGRAD_C8', 'S2E_WGRAD_MULTI_WGS', 'S2E_DETERMINISTIC')
DEPTH_MAX = 256                                # depth 2^-24 <= C_ACC
TILE_FLOATS = 128 * 128 + 128                  # one workgroup's partial tile and its 128 bias sums
MULTI_WGS = 6144                               # S2E_WGRAD_MULTI_WGS of wgrad_chunk_plan
MODES = ('exact', 'short', 'none')

# the environments of the GPU children: switches, threshold of wgrad_use_partial, groups
ENVS = {'default': {}, 'partial2': {'S2E_WGRAD_PARTIAL': '2'}, 'partial0': {'S2E_WGRAD_PARTIAL': '0'}, 'det': {'S2E_DETERMINISTIC': '1'}}
ENV_GROUPS = {'default': ('big', 'mid', 'one'), 'partial2': ('big', 'mid'), 'partial0': ('big',), 'det': ('det', 'multi')}
PARTIAL_MIN = {'default': 16, 'partial2': 2, 'partial0': 0, 'det': 16}

# the forward conv: x (N, H, W, cin) -> (N, Ho, Wo, cout); dt 'bf16' | 'f32'; lrelu: in_act = LRELU; bias: dbias given
Case = namedtuple('Case', 'N H W cin cout k s p dt lrelu bias', defaults=('bf16', False, True))
# a job of the multi-job call: own dw; db names the dbias buffer (None: NULL); default_kind: s2e_conv2d_wgrad_multi_kind without S2E_DETERMINISTIC
Job = namedtuple('Job', 'N H W cin cout k s p db default_kind')

BIG = [   # >= 16 pixel splits: partial tiles + the fixed-order reduce at the shipped threshold
    Case(1, 96, 96, 16, 16, 1, 1, 0),                            # 36 splits: the reduce's unrolled loop plus a remainder
    Case(1, 96, 96, 12, 20, 1, 1, 0, dt='f32'),                  # its fp32 twin: the 32x32x2 path at 36 splits (the largest depth)
    Case(2, 128, 128, 8, 8, 1, 1, 0),                            # 128 splits
    Case(1, 200, 190, 8, 8, 1, 1, 0, bias=False),                # 119 splits of 320, the last one 240
    Case(2, 133, 141, 40, 136, 4, 2, 2),                         # 5 x 2 tiles with K and Cout tails, 17 splits, 85 bias partials
]
MID = [   # 2 .. 15 splits: atomics at the shipped threshold
    Case(1, 128, 128, 64, 128, 4, 2, 2),                         # 8 x 1 tiles, 8 splits: 64 workgroups
    Case(1, 128, 128, 8, 64, 4, 2, 2, bias=False),               # 14 splits
    Case(1, 47, 49, 24, 40, 3, 1, 1, lrelu=True),                # 2 tiles, 8 splits, the last one 63 pixels
    Case(1, 95, 99, 5, 12, 3, 2, 1),                             # scalar gather, bf16: a 5-channel input
    Case(1, 40, 44, 6, 10, 3, 1, 1, dt='f32'),                   # scalar gather, fp32
    Case(1, 40, 44, 6, 10, 3, 1, 1, dt='f32', lrelu=True, bias=False),
    Case(2, 30, 30, 16, 16, 3, 1, 0),                            # pad 0
]
ONE = [   # one split
    Case(2, 40, 36, 64, 1, 4, 2, 2),                             # Cout = 1 at stride 2 (scalar gather), 8 k-tiles, 25 chunks
    Case(2, 16, 16, 264, 136, 1, 1, 0),                          # 3 x 2 tiles: 6 workgroups, 16 chunks > 3 k-tiles
    Case(7, 3, 5, 16, 24, 3, 1, 1),                              # Ho Wo = 15: the sample index advances twice per chunk
    Case(1, 3, 11, 8, 16, 3, 1, 1, bias=False),                  # 33 pixels: a second chunk of one row
    Case(1, 1, 1, 8, 8, 1, 1, 0),                                # M = 1
    Case(1, 9, 11, 72, 16, 4, 2, 2),                             # 30 pixels, 9 k-tiles: one chunk, eight k-tiles sum no bias row
    Case(3, 9, 7, 12, 8, 3, 1, 1, dt='f32', lrelu=True),         # fp32 vector path with the fused LeakyReLU, M = 189 <= 448
]
DET = [BIG[0], BIG[1], BIG[4], MID[0], MID[2], MID[4], ONE[0], ONE[1], ONE[2], ONE[5], ONE[6]]
GROUPS = {'big': BIG, 'mid': MID, 'one': ONE, 'det': DET}
# one s2e_conv2d_wgrad_multi call under S2E_DETERMINISTIC=1: shapes of conv_wgrad_flat.hip's kinds (1x1, 4x4 stride 2, 4x4 stride 1,
# 3x3 stride 2; the shipped S2E_WGRAD_FLAT mask takes the 4x4 ones), one that is none of them, jobs 0 and 2 on one dbias
MULTI = [
    Job(2, 64, 64, 64, 64, 1, 1, 0, 'b0', 0),
    Job(2, 66, 62, 64, 128, 4, 2, 2, 'b1', 5),
    Job(1, 64, 64, 64, 64, 4, 1, 2, 'b0', 4),
    Job(2, 65, 63, 64, 72, 3, 2, 1, None, 0),
    Job(3, 20, 24, 24, 40, 3, 1, 1, 'b4', 0),
    Job(2, 48, 48, 128, 136, 1, 1, 0, 'b5', 0),
]


def env_name(environ=None):
    """which of ENVS the switches of `environ` (default: this process) are"""
    e = os.environ if environ is None else environ
    for k in ('S2E_WGRAD_PATCH', 'S2E_WGRAD_C8', 'S2E_WGRAD_MULTI_WGS'):
        assert k not in e, '%s must be unset' % k
    have = {k: e[k] for k in ('S2E_WGRAD_PARTIAL', 'S2E_DETERMINISTIC') if k in e}
    for name, sw in ENVS.items():
        if sw == have:
            return name
    raise AssertionError('no case list is written for %r' % have)


def out_hw(c):
    return (c.H + 2 * c.p - c.k) // c.s + 1, (c.W + 2 * c.p - c.k) // c.s + 1


def dtype_of(c):
    return torch.float32 if getattr(c, 'dt', 'bf16') == 'f32' else torch.bfloat16


def dt_of(c):
    return S2E_F32 if getattr(c, 'dt', 'bf16') == 'f32' else S2E_BF16


def case_name(c):
    return '%s %dx%dx%d %d->%d %dx%d/%d/%d%s%s' % (getattr(c, 'dt', 'bf16'), c.N, c.H, c.W, c.cin, c.cout, c.k, c.k, c.s, c.p,
                                                   ' in-lrelu' if getattr(c, 'lrelu', False) else '',
                                                   ' bias' if getattr(c, 'bias', getattr(c, 'db', None)) else '')


# ---- plan mirrors (csrc/conv_wgrad.hip)
def plan(c, target_override=0):
    """wgrad_params + generic_wgrad_plan: tiles, pixel splits and pixels per split of the forward conv c"""
    ho, wo = out_hw(c)
    ktot, M = c.k * c.k * c.cin, c.N * ho * wo
    tiles_k, tiles_co = ceil_div(ktot, 128), ceil_div(c.cout, 128)
    tiles = tiles_k * tiles_co
    splits = ceil_div(target_override if target_override > 0 else 2048, tiles)
    max_splits = min(512, M // (2048 if tiles >= 64 else 1024))
    if target_override <= 0 and tiles * max_splits < 512:
        max_splits = min(ceil_div(512, tiles), M // (256 if tiles <= 2 else 512))
    splits = max(1, min(splits, max(1, max_splits)))
    mps = ceil_div(ceil_div(M, splits), 64) * 64
    splits = ceil_div(M, mps)
    vec = 4 if dt_of(c) == S2E_F32 else 8
    return dict(ho=ho, wo=wo, Ktot=ktot, M=M, tiles_k=tiles_k, tiles_co=tiles_co, tiles=tiles, splits=splits, m_per_split=mps,
                last=M - (splits - 1) * mps, grid=tiles * splits, vecpath=c.cin % vec == 0 and c.cout % vec == 0)


def use_partial(splits, env):
    """wgrad_use_partial"""
    n = PARTIAL_MIN[env]
    return env == 'det' or (n > 0 and splits >= 2 and splits >= n)


def partial_bytes(pl):
    """generic_partial_bytes"""
    return pl['tiles'] * pl['splits'] * TILE_FLOATS * 4


def workspace_of(pl, env):
    return partial_bytes(pl) if use_partial(pl['splits'], env) else 0


def multi_kinds(jobs, env):
    return [0 if env == 'det' else j.default_kind for j in jobs]


def multi_plan(jobs, env):
    """wgrad_call_plan + wgrad_chunk_plan for one call of at most 26 generic jobs and no 8-channel ones: per job the plan with its
    target_override (None: the job runs in another kernel) and the bytes the call asks for"""
    gen = [i for i, k in enumerate(multi_kinds(jobs, env)) if k == 0]
    assert len(gen) <= 26
    base = {i: plan(jobs[i]) for i in gen}
    work = {i: float(base[i]['tiles']) * float(base[i]['M']) for i in gen}
    work_sum = sum(work[i] for i in gen)
    plans, total = [None] * len(jobs), 0
    for i in gen:
        plans[i] = plan(jobs[i], int(MULTI_WGS * work[i] / work_sum) + 1)
        if use_partial(plans[i]['splits'], env):
            total += ceil_div(partial_bytes(plans[i]), 256) * 256
    return plans, total


def depth(pl, dt):
    """roundings on the way of one dw element (see the head of this file)"""
    return ceil_div(pl['m_per_split'], 2 if dt == S2E_F32 else 16) + pl['splits'] + 2 + (1 if dt == S2E_F32 else 0)


def bias_depth(pl, dt):
    ni, rpt = (4, 8) if dt == S2E_F32 else (2, 16)
    return ceil_div(ceil_div(pl['m_per_split'], 32), pl['tiles_k']) * ni + rpt + pl['splits'] * pl['tiles_k'] + 1


def split_class(splits):
    return 'splits_1' if splits == 1 else 'splits_2_15' if splits <= 15 else 'splits_16_28' if splits <= 28 else 'splits_ge_33' if splits >= 33 else None


def modes_of(need):
    """the workspace forms a case runs: `short` needs something to shorten, `none` differs from `exact` only with a workspace"""
    return [m for m in MODES if m == 'exact' or (m == 'short' and need > 256) or (m == 'none' and need > 0)]


COUNTERS = ('bf16_vecpath', 'bf16_scalar_gather', 'f32_vecpath', 'f32_scalar_gather', 'cout1_stride2', 'cin5', 'k1', 'k3', 'k4', 'stride1',
            'stride2', 'pad0', 'pad1', 'pad2', 'non_square_map', 'tiles_k_gt1_with_K_tail', 'tiles_co_gt1_with_cout_tail',
            'grid_not_multiple_of_8', 'wo_lt_32', 'howo_lt_32_with_n_gt_2', 'm_eq_1', 'short_last_split', 'masked_last_chunk',
            'lrelu_bf16', 'lrelu_f32', 'dbias_null', 'dbias_given', 'bias_spread_over_k_tiles', 'bias_fewer_chunks_than_k_tiles',
            'splits_1', 'splits_2_15', 'splits_16_28', 'splits_ge_33', 'bias_partials_gt_32') + tuple(
                '%s_ws_%s' % (sc, m) for sc in ('splits_1', 'splits_2_15', 'splits_16_28', 'splits_ge_33') for m in MODES)


def case_counters(c, pl):
    """what one case exercises whatever the environment"""
    n = dict.fromkeys(COUNTERS, 0)
    f32 = dt_of(c) == S2E_F32
    n[('f32' if f32 else 'bf16') + ('_vecpath' if pl['vecpath'] else '_scalar_gather')] = 1
    n['cout1_stride2'] = int(c.cout == 1 and c.s == 2)
    n['cin5'] = int(c.cin == 5)
    n['k%d' % c.k] = 1
    n['stride%d' % c.s] = 1
    n['pad%d' % c.p] = 1
    n['non_square_map'] = int(pl['ho'] != pl['wo'])
    n['tiles_k_gt1_with_K_tail'] = int(pl['tiles_k'] > 1 and pl['Ktot'] % 128 != 0)
    n['tiles_co_gt1_with_cout_tail'] = int(pl['tiles_co'] > 1 and c.cout % 128 != 0)
    n['grid_not_multiple_of_8'] = int(pl['grid'] % 8 != 0)
    n['wo_lt_32'] = int(pl['wo'] < 32)
    n['howo_lt_32_with_n_gt_2'] = int(pl['ho'] * pl['wo'] < 32 and c.N > 2)
    n['m_eq_1'] = int(pl['M'] == 1)
    n['short_last_split'] = int(pl['splits'] > 1 and pl['last'] < pl['m_per_split'])
    n['masked_last_chunk'] = int(pl['M'] % 32 != 0)
    n['lrelu_f32' if f32 else 'lrelu_bf16'] = int(c.lrelu)
    n['dbias_given' if c.bias else 'dbias_null'] = 1
    full = ceil_div(min(pl['m_per_split'], pl['M']), 32)            # chunks of the first split, of the last one
    n['bias_spread_over_k_tiles'] = int(c.bias and pl['tiles_k'] > 1 and full > pl['tiles_k'])
    n['bias_fewer_chunks_than_k_tiles'] = int(c.bias and pl['tiles_k'] > 1 and ceil_div(pl['last'], 32) < pl['tiles_k'])
    n[split_class(pl['splits'])] = 1
    return n


def coverage():
    """the counters over the shipped lists: shapes over big + mid + one, the workspace forms and the reduce's bias loop over every
    environment's groups (a form counts where it differs from the others: with a workspace to give, shorten or withhold)"""
    tot = dict.fromkeys(COUNTERS, 0)
    for name in ENV_GROUPS['default']:
        for c in GROUPS[name]:
            for k, v in case_counters(c, plan(c)).items():
                tot[k] += v
    for env, names in ENV_GROUPS.items():
        for name in names:
            for c in GROUPS.get(name, ()):
                pl = plan(c)
                need = workspace_of(pl, env)
                tot['bias_partials_gt_32'] += int(c.bias and need > 0 and pl['splits'] * pl['tiles_k'] > 32)
                if need > 0:
                    for m in modes_of(need):
                        tot['%s_ws_%s' % (split_class(pl['splits']), m)] += 1
    return tot


# ---- fp64 reference (CPU)
def wgrad64(x, gy, k, s, p):
    """Weight gradient of the conv with kernel k, stride s, pad p in the dtype of its arguments, in the library's layout:
    x (N, H, W, Ci), gy (N, Ho, Wo, Co) -> (Co, k k Ci), columns (ky, kx, ci)."""
    ci, co = x.shape[-1], gy.shape[-1]
    ho, wo = gy.shape[1], gy.shape[2]
    xp = F.pad(x, (0, 0, p, p, p, p))
    g = gy.reshape(-1, co).t().contiguous()
    out = torch.empty(co, k * k, ci, dtype=x.dtype)
    for t in range(k * k):
        ky, kx = divmod(t, k)
        out[:, t] = g @ xp[:, ky:ky + s * (ho - 1) + 1:s, kx:kx + s * (wo - 1) + 1:s].reshape(-1, ci)
    return out.reshape(co, k * k * ci)


def operands(c, seed):
    """CPU tensors of a case: x and gy in the storage dtype (x with exact zeros, negative and positive values), the non-zero fp32
    starts of dw and dbias"""
    gen = torch.Generator().manual_seed(seed)
    ho, wo = out_hw(c)
    x = torch.randn(c.N, c.H, c.W, c.cin, generator=gen)
    x = torch.where(x.abs() < 0.1, torch.zeros_like(x), x).to(dtype_of(c))
    gy = torch.randn(c.N, ho, wo, c.cout, generator=gen).to(dtype_of(c))
    dw0 = torch.randn(c.cout, c.k * c.k * c.cin, generator=gen)
    db0 = torch.randn(c.cout, generator=gen)
    return x, gy, dw0, db0


def reference(c, x, gy):
    """(ref, A, ref_b, A_b): the fp64 sums of the operands the MFMA multiplies, and the same over absolute values"""
    xo = operand64(x, ACT_LRELU if getattr(c, 'lrelu', False) else ACT_NONE, dtype_of(c))
    g64 = gy.double()
    return (wgrad64(xo, g64, c.k, c.s, c.p), wgrad64(xo.abs(), g64.abs(), c.k, c.s, c.p), g64.sum((0, 1, 2)), g64.abs().sum((0, 1, 2)))


# ---- the library
def lib():
    from seg2eye_amd import _lib as L
    return L, L.lib()


def make_desc(c):
    L, _ = lib()
    ho, wo = out_hw(c)
    return L.ConvDesc(c.N, c.H, c.W, c.cin, ho, wo, c.cout, c.k, c.k, c.s, c.p, 0, ACT_LRELU if getattr(c, 'lrelu', False) else ACT_NONE, 0, 0)


def check_route(c, env):
    """route and workspace of the library against the mirror; returns (plan, workspace bytes)"""
    _, lb = lib()
    what, d, pl = case_name(c), make_desc(c), plan(c)
    kind = lb.s2e_conv2d_wgrad_kernel_kind(dt_of(c), C.byref(d))
    assert kind == KERNEL_GENERIC, '%s: kernel kind %d, the case is written for the generic kernel' % (what, kind)
    need, want = int(lb.s2e_conv2d_wgrad_workspace_bytes(dt_of(c), C.byref(d))), workspace_of(pl, env)
    assert need == want, '%s: the library asks for %d bytes of workspace, the mirror says %d (%d tiles x %d splits, %s)' % (
        what, need, want, pl['tiles'], pl['splits'], 'partial tiles' if want else 'atomics')
    return pl, need


def multi_descs(jobs):
    return [make_desc(j) for j in jobs]


def check_multi_route(jobs, env):
    """kinds and workspace of the multi-job call against the mirror; returns (plans, workspace bytes)"""
    L, lb = lib()
    ds = multi_descs(jobs)
    for j, d in zip(jobs, ds):
        assert lb.s2e_conv2d_wgrad_kernel_kind(S2E_BF16, C.byref(d)) == KERNEL_GENERIC, '%s: not a generic shape' % case_name(j)
    kinds = [int(lb.s2e_conv2d_wgrad_multi_kind(S2E_BF16, C.byref(d))) for d in ds]
    assert kinds == multi_kinds(jobs, env), 'kinds of the multi-job call: %s, written for %s' % (kinds, multi_kinds(jobs, env))
    arr = (L.WgradMultiJob * len(jobs))()
    for a, d in zip(arr, ds):
        a.d = d
    need = int(lb.s2e_conv2d_wgrad_multi_workspace_bytes(S2E_BF16, C.byref(arr), len(jobs)))
    plans, want = multi_plan(jobs, env)
    assert need == want, 'the multi-job call asks for %d bytes of workspace, the mirror says %d' % (need, want)
    return plans, need


RESULTS = []
WORST = {}


def report(group, what, pl, mode, wsb, path, worst, same):
    WORST[group] = max(WORST.get(group, 0.0), worst)
    line = '  %-6s %-44s route=generic tiles=%dx%d splits=%-3d m/split=%-4d %-7s ws=%-5s %-9d worst err/bound %.4f%s' % (
        group, what, pl['tiles_k'], pl['tiles_co'], pl['splits'], pl['m_per_split'], path, mode, wsb, worst, same)
    RESULTS.append(dict(group=group, case=what, splits=pl['splits'], m_per_split=pl['m_per_split'], path=path, mode=mode,
                        workspace=wsb, worst=round(worst, 5)))
    print(line, flush=True)


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def run_case(group, c, env, dev, seed):
    L, lb = lib()
    what = case_name(c)
    pl, need = check_route(c, env)
    dt = dt_of(c)
    assert depth(pl, dt) <= DEPTH_MAX and bias_depth(pl, dt) <= DEPTH_MAX, '%s: outside the derivation of the bound' % what
    x, gy, dw0, db0 = operands(c, seed)
    if c.lrelu:
        assert int((x == 0).sum()) and int((x < 0).sum()) and int((x > 0).sum())
    ref, A, rb, Ab = reference(c, x, gy)
    xd, gyd = x.to(dev), gy.to(dev)
    d = make_desc(c)
    st = torch.cuda.current_stream().cuda_stream
    for mode in modes_of(need):
        wsb = {'exact': need, 'short': need - 256, 'none': 0}[mode]
        reduced = mode == 'exact' and need > 0
        outs = []
        for rep in range(2):
            dw = Guarded(tuple(dw0.shape), torch.float32, dev, dw0)
            db = Guarded((c.cout,), torch.float32, dev, db0) if c.bias else None
            ws = workspace(wsb, dev)
            L.check(lb.s2e_conv2d_wgrad(dt, xd.data_ptr(), gyd.data_ptr(), dw.ptr(), db.ptr() if c.bias else None, C.byref(d),
                                        ws.ptr() if mode != 'none' else None, wsb, st), 's2e_conv2d_wgrad')
            for b_, nm in ((dw, 'dw'), (db, 'dbias'), (ws, 'workspace')):
                if b_ is not None:
                    b_.check('%s %s %s (launch %d)' % (what, mode, nm, rep))
            outs.append((dw.t.clone(), db.t.clone() if c.bias else None))
        worst = check_close(outs[0][0], ref, A + dw0.double().abs(), '%s %s dw' % (what, mode), rel=0.0, start=dw0.double())
        if c.bias:
            worst = max(worst, check_close(outs[0][1], rb, Ab + db0.double().abs(), '%s %s dbias' % (what, mode), rel=0.0, start=db0.double()))
        same = ''
        if reduced or pl['splits'] == 1:
            assert same_bits(outs[0][0], outs[1][0]), '%s %s: dw of two launches differs' % (what, mode)
            same = ' x2 bitwise dw'
        if reduced and c.bias:
            assert same_bits(outs[0][1], outs[1][1]), '%s %s: dbias of two launches differs' % (what, mode)
            same += '+dbias'
        report(group, what, pl, mode, wsb, 'reduce' if reduced else 'atomics', worst, same)


def run_multi(group, jobs, env, dev, seed):
    """one s2e_conv2d_wgrad_multi call under S2E_DETERMINISTIC=1, launched twice"""
    L, lb = lib()
    assert env == 'det'
    plans, need = check_multi_route(jobs, env)
    ops, shared = [], {}
    for i, j in enumerate(jobs):
        assert depth(plans[i], S2E_BF16) <= DEPTH_MAX
        x, gy, dw0, db0 = operands(j, seed + i)
        ops.append((x, gy, dw0, reference(j, x, gy)))
        if j.db:
            shared.setdefault(j.db, dict(start=db0, jobs=[]))['jobs'].append(i)
    dev_ops = [(x.to(dev), gy.to(dev)) for x, gy, _, _ in ops]
    st = torch.cuda.current_stream().cuda_stream
    outs = []
    for rep in range(2):
        dws = [Guarded(tuple(o[2].shape), torch.float32, dev, o[2]) for o in ops]
        dbs = {b: Guarded(tuple(s['start'].shape), torch.float32, dev, s['start']) for b, s in shared.items()}
        ws = workspace(need, dev)
        arr = (L.WgradMultiJob * len(jobs))()
        for a, j, d, (xd, gyd), dw in zip(arr, jobs, multi_descs(jobs), dev_ops, dws):
            a.d, a.x, a.gy, a.dw, a.dbias = d, xd.data_ptr(), gyd.data_ptr(), dw.ptr(), dbs[j.db].ptr() if j.db else None
        L.check(lb.s2e_conv2d_wgrad_multi(S2E_BF16, C.byref(arr), len(jobs), ws.ptr(), need, st), 's2e_conv2d_wgrad_multi')
        for i, b_ in enumerate(dws):
            b_.check('multi job %d dw (launch %d)' % (i, rep))
        for b, b_ in dbs.items():
            b_.check('multi dbias %s (launch %d)' % (b, rep))
        ws.check('multi workspace (launch %d)' % rep)
        outs.append(([b_.t.clone() for b_ in dws], {b: b_.t.clone() for b, b_ in dbs.items()}))
    for i, j in enumerate(jobs):
        what = 'job %d %s' % (i, case_name(j))
        x, gy, dw0, (ref, A, rb, Ab) = ops[i]
        worst = check_close(outs[0][0][i], ref, A + dw0.double().abs(), 'multi %s dw' % what, rel=0.0, start=dw0.double())
        assert same_bits(outs[0][0][i], outs[1][0][i]), 'multi %s: dw of two launches differs' % what
        same = ' x2 bitwise dw'
        if j.db:
            s = shared[j.db]
            assert sum(bias_depth(plans[k], S2E_BF16) for k in s['jobs']) <= DEPTH_MAX
            rsum, asum = sum(ops[k][3][2] for k in s['jobs']), sum(ops[k][3][3] for k in s['jobs'])
            worst = max(worst, check_close(outs[0][1][j.db], rsum, asum + s['start'].double().abs(), 'multi %s dbias %s' % (what, j.db),
                                           rel=0.0, start=s['start'].double()))
            if len(s['jobs']) == 1:
                assert same_bits(outs[0][1][j.db], outs[1][1][j.db]), 'multi %s: dbias of two launches differs' % what
                same += '+dbias'
        report(group, what, plans[i], 'exact', need, 'reduce', worst, same)


def plan_only(names, env):
    """--plan: every case's route and workspace against the mirror, on the library alone (no GPU)"""
    n = 0
    for name in names:
        if name == 'multi':
            check_multi_route(MULTI, env)
            n += len(MULTI)
            continue
        for c in GROUPS[name]:
            check_route(c, env)
            n += 1
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--groups', required=True)
    ap.add_argument('--plan', action='store_true', help='routes and workspace sizes only, without a GPU')
    ap.add_argument('--json', help='also write the per-case results to this file')
    args = ap.parse_args()
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    names = args.groups.split(',')
    env = env_name()
    lib()
    sw = ' '.join('%s=%s' % (k, os.environ[k]) for k in SWITCHES if k in os.environ) or 'defaults'
    if args.plan:
        n = plan_only(names, env)
        print('wgrad generic plan ok: %d cases, groups %s (%s)' % (n, args.groups, sw), flush=True)
        return
    for name in names:
        assert name in ENV_GROUPS[env], 'group %s is not written for the environment %s' % (name, sw)
    dev = torch.device('cuda', 0)
    for name in names:
        if name == 'multi':
            run_multi(name, MULTI, env, dev, 7000)
        else:
            for c in GROUPS[name]:
                run_case(name, c, env, dev, 3000 + 41 * (BIG + MID + ONE).index(c))
        print('  worst err/bound of group %s: %.4f' % (name, WORST[name]), flush=True)
    cov = coverage()
    print('  counters over the shipped lists: %s' % ', '.join('%s=%d' % kv for kv in cov.items()), flush=True)
    zero = [k for k, v in cov.items() if v == 0]
    assert not zero, 'counters that no shipped case exercises: %s' % zero
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(dict(environment=sw, worst=WORST, cases=RESULTS), f, indent=1)
    print('wgrad generic ok: %d checks, groups %s (%s)' % (len(RESULTS), args.groups, sw), flush=True)


if __name__ == '__main__':
    main()
