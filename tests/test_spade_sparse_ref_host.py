"""tests/_spade_sparse_ref.py on the CPU: the label-map counts the GPU cases rely on, the exactness of the gridded mlp_shared weights,
the references against the plain fp64 branch and its autograd, and the teeth of the bounds -- the fp64 reference with ONE mistake planted
in place of the GPU result exceeds the bound tests/_spade_sparse_child.py uses, while the reference rounded as the kernel rounds passes
it.  No GPU needed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _spade_sparse_ref as R

NCLS = 4


def gen(seed):
    return torch.Generator().manual_seed(seed)


def _ui(label):
    N, H, W = label.shape
    cls, dense, uni = R.classify_ref(label, H, W, 16, 16)
    work, ui = R.lists_bwd_ref(cls, N, H // 16, W // 16)
    return cls, ui


# ---- label maps
def test_block_label_counts():
    cls, ui = _ui(R.block_labels(1, 96, 96))
    assert len(ui) == 4 and sorted(cls[ui].tolist()) == [0, 1, 2, 3]
    cls, ui = _ui(R.block_labels(1, 128, 128))
    assert len(ui) == 16 and np.bincount(cls[ui], minlength=4).tolist() == [4, 4, 4, 4]
    cls, ui = _ui(R.block_labels(2, 128, 128))
    assert len(ui) == 32 > R.UNI_REPLICAS and np.bincount(cls[ui], minlength=4).tolist() == [8, 8, 8, 8]
    cls, ui = _ui(np.full((1, 48, 48), 2, dtype=np.uint8))
    assert ui.tolist() == [4]


def test_salt_and_skipped_pixels():
    lab = R.block_labels(2, 32, 32)
    s = R.salt(lab, [(1, 3, 4)])
    assert int((s != lab).sum()) == 1 and s[1, 3, 4] != lab[1, 3, 4] and s[1, 3, 4] < NCLS
    up = R.upsample_salted(s, 4)
    assert np.array_equal(up[:, ::4, ::4], s)
    assert int((up == s.repeat(4, 1).repeat(4, 2)).sum()) == s.size          # every skipped pixel is another class
    a = R.classify_ref(s, 32, 32, 8, 8)
    b = R.classify_ref(up, 32, 32, 8, 8)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('pt,dense', [((40, 40), True), ((31, 40), True), ((40, 49), True), ((30, 30), True), ((49, 49), True),
                                      ((29, 40), False), ((50, 50), False)])
def test_classify_rule_around_a_rectangle(pt, dense):
    """rectangle (2, 2) of a 96 x 96 one-class map in 16 x 16 rectangles: pixels 32..47, halo 30..49"""
    one = np.full((1, 96, 96), 1, dtype=np.uint8)
    cls, _, _ = R.classify_ref(R.salt(one, [(0,) + pt]), 96, 96, 16, 16)
    assert cls[14] == (R.DENSE if dense else 1)


def test_lists_are_a_partition_in_order():
    cls = np.random.RandomState(3).choice(np.array([0, 1, R.DENSE], dtype=np.uint8), size=2 * 5 * 4)
    work, ui = R.lists_bwd_ref(cls, 2, 5, 4)
    assert sorted(work.tolist() + ui.tolist()) == list(range(40))
    assert (np.diff(work) > 0).all() and (np.diff(ui) > 0).all() and (cls[ui] != R.DENSE).all()
    assert len(R.lists_bwd_ref(np.zeros(7, dtype=np.uint8), 1, 1, 7)[1]) == 0


# ---- exactness of the gridded weights
def test_grid_weights_sum_exactly_in_fp32():
    g = gen(1)
    w_sh, b_sh = R.grid_weights((128, NCLS, 3, 3), g), R.grid_weights((128,), g)
    assert float(w_sh.abs().max()) < 2 and bool((w_sh * 128 == (w_sh * 128).round()).all())
    ref = b_sh[:, None] + w_sh.sum((2, 3))
    terms = torch.cat([b_sh[:, None, None].expand(128, NCLS, 1), w_sh.reshape(128, NCLS, 9)], -1).float()
    for order in (list(range(10)), list(range(9, -1, -1)), [5, 0, 9, 2, 7, 1, 8, 3, 6, 4]):
        acc = torch.zeros(128, NCLS, dtype=torch.float32)
        for i in order:
            acc = acc + terms[..., i]
        assert torch.equal(acc.double(), ref)
    # hence one ReLU mask and one bf16 rounding on both sides
    a = R.hidden_act(w_sh, b_sh, torch.bfloat16)
    assert torch.equal(a, torch.relu(ref.float()).to(torch.bfloat16).double().t())
    assert torch.equal(a > 0, (ref > 0).t()) and 0.2 < float((a > 0).double().mean()) < 0.8


# ---- the references against the plain branch
def _branch(label, w_sh, b_sh, wq, bias, act_dtype):
    onehot = F.one_hot(torch.as_tensor(label.astype(np.int64)), w_sh.shape[1]).permute(0, 3, 1, 2).double()
    act = R.round_to(torch.relu(F.conv2d(onehot, w_sh, b_sh, padding=1)), act_dtype)
    return F.conv2d(act, wq, bias, padding=1).permute(0, 2, 3, 1)


@pytest.mark.parametrize('act_dtype', [torch.bfloat16, torch.float32])
def test_table_and_classifier_against_the_dense_branch(act_dtype):
    """wherever classify_ref calls a rectangle uniform, the dense branch equals the table row of the pixel's position class"""
    g = gen(2)
    nh, C_ = 24, 5
    w_sh, b_sh = R.grid_weights((nh, NCLS, 3, 3), g), R.grid_weights((nh,), g)
    wq, bias = torch.randn(2 * C_, nh, 3, 3, generator=g, dtype=torch.float64), torch.randn(2 * C_, generator=g, dtype=torch.float64)
    table, A = R.table_ref(w_sh, b_sh, wq, bias, act_dtype)
    assert bool((A >= table.abs()).all())
    for label, tw, th in ((R.salt(R.block_labels(2, 48, 64), [(0, 5, 5)]), 8, 8), (np.full((1, 5, 5), 3, dtype=np.uint8), 16, 16),
                          (R.salt(np.full((2, 21, 19), 1, dtype=np.uint8), [(0, 10, 9)]), 8, 8)):
        N, H, W = label.shape
        cls, dense, uni = R.classify_ref(label, H, W, tw, th)
        assert len(uni) > 0
        gb = _branch(label, w_sh, b_sh, wq, bias, act_dtype)
        cmap = R.rect_class_map(cls, N, H, W, tw, th)
        keep = torch.from_numpy(cmap != R.DENSE)
        cy = torch.as_tensor(R.pos_class(np.arange(H), H))[None, :, None].expand(N, H, W)
        cx = torch.as_tensor(R.pos_class(np.arange(W), W))[None, None, :].expand(N, H, W)
        look = table[torch.as_tensor(np.where(cmap == R.DENSE, 0, cmap)), cy, cx]
        assert float((look - gb)[keep].abs().max()) <= 1e-12 * float(gb.abs().max())
        # a rectangle one pixel of halo short of uniform is NOT reproduced by the table: the 2-pixel halo is needed
        assert float((look - gb)[~keep].abs().max()) > 1e-3 if bool((~keep).any()) else True


def test_modulate_ref_is_the_modulation_of_the_table_rows():
    g = gen(3)
    N, H, W, C_ = 2, 9, 7, 3
    x = torch.randn(N, H, W, C_, generator=g, dtype=torch.float64)
    stats = torch.stack([torch.randn(N, C_, generator=g, dtype=torch.float64), 0.5 + torch.rand(N, C_, generator=g, dtype=torch.float64)], -1)
    s0, s1 = torch.randn(N, C_, generator=g, dtype=torch.float64), torch.randn(N, C_, generator=g, dtype=torch.float64)
    table = torch.randn(NCLS, 5, 5, 2 * C_, generator=g, dtype=torch.float64)
    cmap = np.random.RandomState(0).randint(0, NCLS, size=(N, H, W))
    out, A, gamma = R.modulate_ref(x, stats, s0, s1, table, cmap, True)
    assert bool((A >= out.abs()).all())
    for n, y, xx in ((0, 0, 0), (1, 1, 5), (0, 4, 3), (1, 7, 6), (1, 8, 1)):
        row = table[cmap[n, y, xx], int(R.pos_class(y, H)), int(R.pos_class(xx, W))]
        v = 0.5 * ((x[n, y, xx] - stats[n, :, 0]) * stats[n, :, 1] * (1 + row[:C_]) + row[C_:] + x[n, y, xx] * (1 + s0[n]) + s1[n])
        assert torch.allclose(out[n, y, xx], torch.where(v > 0, v, 0.2 * v), rtol=1e-13, atol=0)
        assert torch.equal(gamma[n, y, xx], row[:C_])
    assert R.pos_class(np.arange(5), 5).tolist() == [0, 1, 2, 3, 4] and R.pos_class(np.arange(7), 7).tolist() == [0, 1, 2, 2, 2, 3, 4]


def _sums_case(seed, N, HW, C2, nh, salted=()):
    g = gen(seed)
    label = R.salt(R.block_labels(N, HW, HW), list(salted))
    cls, ui = _ui(label)
    dgb = torch.randn(N, HW, HW, C2, generator=g).to(torch.bfloat16).double()
    w_gb = torch.randn(C2, nh, 3, 3, generator=g, dtype=torch.float64) * (9 * nh) ** -0.5
    w_sh, b_sh = R.grid_weights((nh, NCLS, 3, 3), g), R.grid_weights((nh,), g)
    return label, cls, ui, dgb, w_gb, w_sh, b_sh


@pytest.fixture(scope='module')
def sums_case():
    return _sums_case(4, 2, 96, 6, 8, salted=[(1, 70, 70)])


@pytest.mark.parametrize('act_dtype', [torch.bfloat16, torch.float32])
def test_sums_and_grads_against_autograd(sums_case, act_dtype):
    label, cls, ui, dgb, w_gb, w_sh, b_sh = sums_case
    N, H, W = label.shape
    assert 4 <= len(ui) < 8
    Rr, Ra = R.sums_ref(dgb, cls, ui, H, W, NCLS)
    ref = R.grads_ref(Rr, Ra, w_gb, w_sh, b_sh, act_dtype)
    auto = R.branch_autograd(label, w_sh, b_sh, w_gb, dgb, R.rect_pixels(ui, N, H, W, 16, 16), act_dtype)
    for k in ('dw_sh', 'db_sh', 'dw_gb', 'db_gb'):
        assert float(auto[k].abs().max()) > 0
        assert float((ref[k][0] - auto[k]).abs().max()) <= 1e-11 * float(ref[k][1].max()), k
        assert bool((ref[k][1] >= ref[k][0].abs() - 1e-9).all())


# ---- the teeth of the bounds: one planted mistake each
def _fails(*a, **k):
    with pytest.raises(AssertionError, match='outside the bound'):
        R.check_close(*a, **k)


def test_mutant_classifier_skips_halo_corners():
    one = np.full((1, 96, 96), 1, dtype=np.uint8)
    lab = R.salt(one, [(0, 30, 30)])
    good, bad = R.classify_ref(lab, 96, 96, 16, 16), R.classify_ref(lab, 96, 96, 16, 16, skip_corners=True)
    assert good[0][14] == R.DENSE and bad[0][14] == 1 and not np.array_equal(good[2], bad[2])
    lab = R.salt(one, [(0, 31, 40)])                                   # (the mutant still sees the edges of the halo)
    assert np.array_equal(R.classify_ref(lab, 96, 96, 16, 16)[0], R.classify_ref(lab, 96, 96, 16, 16, skip_corners=True)[0])


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float32])
def test_mutant_table_ring_1_gets_the_interior_row(dt):
    g = gen(5)
    nh, C_ = 128, 6
    w_sh, b_sh = R.grid_weights((nh, NCLS, 3, 3), g), R.grid_weights((nh,), g)
    w = torch.randn(2 * C_, nh, 3, 3, generator=g) * (9 * nh) ** -0.5
    ref, A = R.table_ref(w_sh, b_sh, w.to(dt).double(), None, dt)
    assert R.check_close(ref.float().double(), ref, A, 'table stored as fp32', rel=0.0) < 1
    for ax in (1, 2):
        bad = ref.clone()
        bad.select(ax, 1).copy_(ref.select(ax, 2))
        _fails(bad, ref, A, 'ring 1 = interior', rel=0.0)
    # ... and by far: the median element of ring 1 is hundreds of bounds away from the interior row
    assert float(((ref[:, 1] - ref[:, 2]).abs() / (R.C_ACC * A[:, 1])).median()) > 100


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float32])
def test_mutant_modulate_reads_the_neighbouring_class(dt):
    g = gen(6)
    N, H, W, C_ = 1, 21, 19, 8
    x = (torch.randn(N, H, W, C_, generator=g) + 0.3).to(dt).double()
    stats = torch.stack([torch.randn(N, C_, generator=g) * 0.3, 0.5 + 1.5 * torch.rand(N, C_, generator=g)], -1).double()
    s0, s1 = (torch.randn(N, C_, generator=g) * 0.4).double(), (torch.randn(N, C_, generator=g) * 0.4).double()
    table = (torch.randn(NCLS, 5, 5, 2 * C_, generator=g) * 0.5).double()
    cmap = np.full((N, H, W), 1)
    ref, A, _ = R.modulate_ref(x, stats, s0, s1, table, cmap, True)
    assert R.check_close(R.round_to(ref, dt), ref, A, 'out rounded to the dtype', rel=R.rel_of(dt)) <= 1
    bad, _, _ = R.modulate_ref(x, stats, s0, s1, table, (cmap + 1) % NCLS, True)
    _fails(bad, ref, A, 'class + 1', rel=R.rel_of(dt))
    one_pixel = ref.clone()
    one_pixel[0, 1, 1] = bad[0, 1, 1]                                   # a single ring-1 pixel
    _fails(one_pixel, ref, A, 'class + 1 at one pixel', rel=R.rel_of(dt))


def test_mutant_sums(sums_case):
    label, cls, ui, dgb, w_gb, w_sh, b_sh = sums_case
    H, W = label.shape[1:]
    ref, A = R.sums_ref(dgb, cls, ui, H, W, NCLS)
    assert R.check_close(ref.float().double(), ref, A, 'R stored as fp32', rel=0.0) < 1
    _fails(R.sums_ref(dgb, cls, ui, H, W, NCLS, swap_taps=True)[0], ref, A, 'taps t and 8 - t exchanged', rel=0.0)
    _fails(R.sums_ref(dgb, cls, ui, H, W, NCLS, drop_row=(0, 4, 7))[0], ref, A, 'one row of one window dropped', rel=0.0)
    # the start value's allowance does not hide it either
    start = torch.randn(ref.shape, generator=gen(7), dtype=torch.float64) * 4
    _fails(start + R.sums_ref(dgb, cls, ui, H, W, NCLS, drop_row=(1, 0, 15))[0], ref, A, 'dropped row, non-zero start', rel=0.0, start=start)


@pytest.mark.parametrize('C2', [12, 1024])
def test_mutant_grads(C2):
    g = gen(8)
    nh = 40
    Rr = torch.randn(R.UNI_REPLICAS, NCLS, 9, C2, generator=g).double()
    R64, Ra = Rr.sum(0), Rr.abs().sum(0)
    w_gb = torch.randn(C2, nh, 3, 3, generator=g, dtype=torch.float64) * (9 * nh) ** -0.5
    w_sh, b_sh = R.grid_weights((nh, NCLS, 3, 3), g), R.grid_weights((nh,), g)
    ref = R.grads_ref(R64, Ra, w_gb, w_sh, b_sh, torch.bfloat16)
    acc = R.grads_acc(C2)
    assert acc == (R.C_ACC if C2 == 12 else R.GEMV_ACC)
    for k, (v, a) in ref.items():
        assert R.check_close(v.float().double(), v, a, k + ' stored as fp32', rel=0.0, acc=acc if k in ('A', 'dw_sh', 'db_sh') else R.C_ACC) < 1
    tap = R.grads_ref(R64, Ra, w_gb, w_sh, b_sh, torch.bfloat16, rank1_tap=3)
    _fails(tap['dw_gb'][0], ref['dw_gb'][0], ref['dw_gb'][1], 'rank-1 update from tap 3', rel=0.0)
    _fails(tap['db_gb'][0], ref['db_gb'][0], ref['db_gb'][1], 'bias sums from tap 3', rel=0.0)
    nomask = R.grads_ref(R64, Ra, w_gb, w_sh, b_sh, torch.bfloat16, ignore_mask=True)
    # (the |.| twin of the masked-off elements is 0: there the kernel must add exactly nothing)
    _fails(nomask['dw_sh'][0], ref['dw_sh'][0], ref['dw_sh'][1], 'ReLU mask ignored', rel=0.0, acc=acc)
    _fails(nomask['db_sh'][0], ref['db_sh'][0], ref['db_sh'][1], 'ReLU mask ignored', rel=0.0, acc=acc)
    one_replica = R.grads_ref(R64 - Rr[5], Ra, w_gb, w_sh, b_sh, torch.bfloat16)
    _fails(one_replica['A'][0], ref['A'][0], ref['A'][1], 'a replica left out', rel=0.0, acc=acc)


def test_chain_lengths_fit_the_allowance():
    assert all(v <= 256 for v in R.CHAIN.values())
    assert R.grads_chain(128) <= 256 and R.grads_acc(128) == R.C_ACC and R.grads_acc(12) == R.C_ACC
    assert 256 < R.grads_chain(1024) <= 512 and R.grads_acc(1024) == R.GEMV_ACC


# ---- the cases the GPU children run (enumerated with the runners replaced by recorders)
@pytest.fixture(scope='module')
def child_cases():
    import _spade_sparse_child as CH
    mp, rec = pytest.MonkeyPatch(), {}
    try:
        for name in ('run_classify', 'run_lists_bwd', 'run_modulate', 'run_sums'):
            mp.setattr(CH, name, (lambda nm: lambda *a, **k: rec.setdefault(nm, []).append((a, k)))(name))
        CH.group_classify(None, None)
        CH.group_lists_bwd(None, None)
        for dt in (torch.bfloat16, torch.float32):
            CH.group_modulate(None, dt)
            CH.group_sums(None, dt)
    finally:
        mp.undo()
    return CH, rec


def test_child_cases_cover_every_path(child_cases):
    CH, rec = child_cases
    # classify: (name, label, h, w, tw, th, dev)
    cl = [a for a, k in rec['run_classify']]
    assert {(a[4], a[5]) for a in cl} == {(16, 16), (8, 8), (32, 8), (64, 64)}
    assert {a[1].shape[1] // a[2] for a in cl} == {1, 2, 4}
    assert {(40, 50), (21, 19)} <= {(a[2], a[3]) for a in cl}
    rects = [a[1].shape[0] * -(-a[2] // a[5]) * -(-a[3] // a[4]) for a in cl]
    assert 1083 in rects and 1083 % 4 and max(rects) > 1024                  # a second trip of the one-block compaction
    for word in ('inside', 'distance 1', 'distance 2', 'corner', 'distance 3', 'left edge', 'right edge', 'last row', 'first row', 'all uniform',
                 'all dense'):
        assert any(word in a[0] for a in cl), word
    # lists_bwd: (name, cls, N, tiles_y, tiles_x, dev)
    lb = [a for a, k in rec['run_lists_bwd']]
    assert {(3, 3), (1, 7), (2, 2), (15, 15)} <= {(a[3], a[4]) for a in lb}
    assert any(a[1].size == 1125 for a in lb) and all((a[1] == R.DENSE).any() for a in lb[:4])
    # modulate: (name, dt, label, C, tw, th) + keywords or positionals
    names = ('lrelu_on', 'with_gamma', 'x_up', 'banked', 'short')
    mods = [(a[:6], dict(zip(names, a[6:11])) if len(a) > 6 else k) for a, k in rec['run_modulate']]
    for dt, cs in ((torch.bfloat16, {8, 64, 24}), (torch.float32, {4, 12, 1028})):
        mine = [(a, k) for a, k in mods if a[1] == dt]
        assert {a[3] for a, k in mine} == cs
        assert {(a[4], a[5]) for a, k in mine} == {(16, 16), (32, 8), (8, 8)}
        assert {a[2].shape[1:] for a, k in mine} >= {(5, 5), (21, 19), (48, 64)}
        for flag in names:
            assert {bool(k[flag]) for a, k in mine} == {True, False}, (dt, flag)
        for C_ in cs - {1028}:                                                # every flag both ways at every channel count
            assert {bool(k['with_gamma']) for a, k in mine if a[3] == C_} == {True, False}
    assert any(len(R.classify_ref(a[2], a[2].shape[1], a[2].shape[2], a[4], a[5])[2]) > 2048 for a, k in mods if a[1] == torch.bfloat16)
    assert any(a[3] // 4 > 256 for a, k in mods if a[1] == torch.float32)      # more than 256 channel groups
    assert any((a[3] // 8) not in (1, 2, 4, 8, 16, 32) for a, k in mods if a[1] == torch.bfloat16)      # groups that do not divide 256
    # sums: (name, dt, label, C2, mode, dev, seed)
    su = [a for a, k in rec['run_sums']]
    for dt in (torch.bfloat16, torch.float32):
        mine = [a for a in su if a[1] == dt]
        assert {a[3] for a in mine} == {128, 256, 512, 1024} and {a[4] for a in mine} == {'all', 'subset', 'zero'}
        assert {a[2].shape for a in mine} == {(1, 48, 48), (1, 96, 96), (2, 128, 128)}
        assert any(len(_ui(a[2])[1]) > R.UNI_REPLICAS and a[4] == 'all' for a in mine)
    # grads
    jobs = [j for _, specs in CH.GRADS_CALLS for j in specs]
    assert {len(specs) for _, specs in CH.GRADS_CALLS} == {1, 3, 16}
    assert {j['C2'] for j in jobs} == {12, 128, 1024} and {j['nh'] for j in jobs} == {128, 64, 40} and {j['ncls'] for j in jobs} == {4, 3, 1}
    assert {j['cl'] for j in jobs} == {True, False} and {bool(j['act_bf16']) for j in jobs} == {True, False}
    assert {j['gb'] for j in jobs} == {'both', 'dw_only', None}
    assert any({j['gb'] is None for j in specs} == {True, False} for _, specs in CH.GRADS_CALLS)      # dw_gb on some jobs of a call only
    assert any(all(j['gb'] is None for j in specs) for _, specs in CH.GRADS_CALLS)
    assert any(not j.get('dw_sh', True) for j in jobs) and any(not j.get('db_sh', True) for j in jobs)
    for _, specs in CH.GRADS_CALLS[1:]:
        assert len({j['C2'] for j in specs}) == 3                             # 2C mixed within a call
