"""The region-aware error without a GPU: the torch restatement of the rule (tests/_region_ref.py) checked alone, the flags,
and what the four entry points answer before any launch."""
import ctypes

import pytest
import torch

import _region_ref as R
from _quality_harness import check_error_table

F32, BF16, BAD = 0, 1, 7
L1, L2 = 0, 1
P = 4096                                                      # a dummy non-null pointer: must never reach a kernel
BIG = 1 << 24                                                 # a workspace size that is never short


def _grid(shape, seed):
    """numbers k / 128 in [-1, 1]: on the bf16 grid, so differences and their squares are exact in fp32"""
    return torch.randint(-128, 129, shape, generator=torch.Generator().manual_seed(seed)).double() / 128


# ------------------------------------------------------------------------------------------------ the restatement
def test_one_pixel_by_hand():
    x, y = torch.tensor([[[0.5]]]), torch.tensor([[[-0.25]]])
    lab = torch.tensor([[[2]]], dtype=torch.uint8)
    s = R.stats(x, y, lab, 4)
    assert s.shape == (1, 4, 3) and s.dtype == torch.float64
    assert s[0, 2].tolist() == [1.0, 0.75, 0.5625] and float(s[0, [0, 1, 3]].abs().sum()) == 0
    for norm, want, gwant in (('l1', 0.75, 1.0), ('l2', 0.5625, 1.5)):
        v, g = R.loss_and_grad(x, y, lab, [1, 1, 3, 1], norm)
        assert float(v) == want and float(g) == gwant         # the one present class: its weight cancels
    assert R.coef(lab, (1, 1, 1), [1, 1, 3, 1]).tolist() == [0, 0, 1, 0]


def test_an_absent_class_leaves_the_average():
    """classes 0 and 2 present (3 and 1 pixels), 1 absent: loss = (w0 m0 + w2 m2) / (w0 + w2)"""
    x = torch.tensor([[[0.5, 0.25], [0.0, -1.0]]], dtype=torch.float64)
    y = torch.zeros(1, 2, 2, dtype=torch.float64)
    lab = torch.tensor([[[0, 0], [0, 2]]], dtype=torch.uint8)
    v, g = R.loss_and_grad(x, y, lab, [1.0, 5.0, 3.0], 'l1')
    assert abs(float(v) - (1.0 * 0.25 + 3.0 * 1.0) / 4.0) < 1e-15
    assert torch.allclose(g, torch.tensor([[[1 / 12, 1 / 12], [0.0, -3 / 4]]], dtype=torch.float64), atol=1e-15)   # sign(0) = 0
    assert torch.allclose(R.coef(lab, (1, 2, 2), [1.0, 5.0, 3.0]), torch.tensor([1 / 12, 0.0, 3 / 4], dtype=torch.float64))


def test_a_class_in_one_image_only_is_a_batch_mean():
    x, y = _grid((2, 4, 6), 1), _grid((2, 4, 6), 2)
    lab = torch.zeros(2, 4, 6, dtype=torch.uint8)
    lab[0, :2] = 1                                            # class 1: 12 pixels of image 0, none of image 1
    d = (x - y).abs()
    want = (d[lab == 0].mean() + d[lab == 1].mean()) / 2
    assert abs(float(R.loss(x, y, lab, [1, 1]) - want)) < 1e-15
    s = R.stats(x, y, lab, 2)
    assert s[:, :, 0].tolist() == [[12.0, 12.0], [24.0, 0.0]]
    assert abs(float(s[:, 0, 1].sum() / 36 + s[:, 1, 1].sum() / 12) / 2 - float(want)) < 1e-15


def test_a_zero_weight_class_counts_for_nothing():
    x, y = _grid((2, 5, 7), 3), _grid((2, 5, 7), 4)
    lab = torch.randint(0, 3, (2, 5, 7), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)
    v, g = R.loss_and_grad(x, y, lab, [2.0, 0.0, 1.0], 'l2')
    d2 = (x - y) ** 2
    assert abs(float(v) - float(2 * d2[lab == 0].mean() + d2[lab == 2].mean()) / 3) < 1e-15
    assert float(g[lab == 1].abs().max()) == 0 and float(g[lab == 0].abs().max()) > 0
    assert float(R.coef(lab, (2, 5, 7), [2.0, 0.0, 1.0])[1]) == 0


def test_labels_at_or_above_ncls_are_ignored():
    x, y = _grid((1, 3, 4), 6), _grid((1, 3, 4), 7)
    lab = torch.tensor([[[0, 1, 7, 4], [0, 1, 255, 4], [0, 1, 7, 4]]], dtype=torch.uint8)
    s = R.stats(x, y, lab, 4)
    assert s[0, :, 0].tolist() == [3.0, 3.0, 0.0, 0.0]
    v, g = R.loss_and_grad(x, y, lab, [1, 1, 1, 1])
    d = (x - y).abs()
    assert abs(float(v) - float(d[lab == 0].mean() + d[lab == 1].mean()) / 2) < 1e-15
    assert float(g[lab >= 4].abs().max()) == 0


def test_no_weighted_class_present_is_zero_with_a_zero_gradient():
    x, y = _grid((2, 3, 3), 8), _grid((2, 3, 3), 9)
    for lab, w in ((torch.full((2, 3, 3), 7, dtype=torch.uint8), [1, 1, 1, 1]), (torch.ones(2, 3, 3, dtype=torch.uint8), [1, 0, 1, 1])):
        for norm in ('l1', 'l2'):
            v, g = R.loss_and_grad(x, y, lab, w, norm)
            assert float(v) == 0 and g.shape == x.shape and float(g.abs().max()) == 0
        assert float(R.coef(lab, (2, 3, 3), w).abs().max()) == 0


def test_a_single_class_with_weight_one_is_the_plain_mean():
    x, y = _grid((3, 6, 5), 10), _grid((3, 6, 5), 11)
    lab = torch.zeros(3, 6, 5, dtype=torch.uint8)
    assert abs(float(R.loss(x, y, lab, [1.0])) - float((x - y).abs().mean())) < 1e-15
    assert abs(float(R.loss(x, y, lab, [1.0], 'l2')) - float(((x - y) ** 2).mean())) < 1e-15


def test_lookup_256_to_640x400_against_a_python_loop():
    lab = torch.randint(0, 4, (1, 256, 256), generator=torch.Generator().manual_seed(12), dtype=torch.uint8)
    got = R.lookup(lab, 640, 400)
    assert got.shape == (1, 640, 400) and got.dtype == torch.int64
    rows, cols = [(r * 256) // 640 for r in range(640)], [(c * 256) // 400 for c in range(400)]
    want = torch.tensor([[int(lab[0, rr, cc]) for cc in cols] for rr in rows])
    assert torch.equal(got[0], want)
    assert int(got[0, 25, 25]) == int(lab[0, 10, 16]) and int(got[0, 639, 399]) == int(lab[0, 255, 255])      # (25 * 256) // 640 = 10, // 400 = 16
    assert torch.equal(R.lookup(lab, 256, 256), lab.long())    # same size: the identity


# ------------------------------------------------------------------------------------------------ the flags
def test_flags_parse_and_default_off():
    from seg2eye_amd.options import default_opt, parse, parse_region_weights
    o = parse([])
    assert o.lambda_region == 0.0 and o.region_norm == 'l1' and o.region_weights == '' and o.val_regions is False
    o = parse(['--lambda_region', '2', '--region_norm', 'l2', '--region_weights', '1,0,2.5,4'])
    assert o.lambda_region == 2.0 and o.region_norm == 'l2' and parse_region_weights(o.region_weights, o.label_nc) == [1.0, 0.0, 2.5, 4.0]
    assert parse_region_weights('', 4) == [1.0] * 4 and parse_region_weights('3', 1) == [3.0]
    t = parse(['--val_regions'], is_train=False)
    assert t.val_regions is True and t.lambda_region == 0.0 and parse([], is_train=False).val_regions is False
    assert parse(['--val_regions']).val_regions is True        # train.py's periodic validation takes it too
    d = default_opt()
    assert d.lambda_region == 0.0 and d.region_norm == 'l1' and d.region_weights == ''
    assert default_opt(lambda_region=1.5, region_norm='l2').lambda_region == 1.5
    with pytest.raises(SystemExit):
        parse(['--lambda_region', '1'], is_train=False)        # a training flag only
    with pytest.raises(SystemExit):
        parse(['--region_norm', 'huber'])


@pytest.mark.parametrize('text', ['1,2,3', '1,2,3,4,5', '1,-1,1,1', '0,0,0,0', '1,a,1,1', '1,,1,1', '1,nan,1,1', '1,inf,1,1'],
                         ids=['short', 'long', 'negative', 'all-zero', 'non-numeric', 'empty-field', 'nan', 'inf'])
def test_bad_region_weights_raise_at_parse_time(text):
    from seg2eye_amd.options import parse
    with pytest.raises(ValueError, match='region_weights'):
        parse(['--region_weights', text])


def test_ops_refuse_cpu_tensors():
    from seg2eye_amd import _lib, ops
    x = torch.zeros(2, 1, 16, 16)
    lab = torch.zeros(2, 16, 16, dtype=torch.uint8)
    with pytest.raises(_lib.Seg2EyeHipError, match='GPU only'):
        ops.region_loss(x, x, lab, torch.ones(4))
    with pytest.raises(_lib.Seg2EyeHipError, match='GPU only'):
        ops.region_stats_u8(x.to(torch.uint8), x.to(torch.uint8), lab, 4)
    with pytest.raises(ValueError, match='uint8'):
        ops.region_stats_u8(x, x, lab, 4)
    with pytest.raises(ValueError, match='norm'):
        ops.region_loss(x, x, lab, torch.ones(4), norm='huber')
    with pytest.raises(ValueError, match='classes'):
        ops.region_stats_u8(x.to(torch.uint8), x.to(torch.uint8), lab, 9)
    assert ops.region_loss is ops.losses.region_loss and ops.RegionLossFn is ops.losses.RegionLossFn and ops.region_stats_u8 is ops.losses.region_stats_u8


# ------------------------------------------------------------------------------------------------ the entry points, before any launch
ARG = 's2e_region_%s: bad argument'
NCLS = 's2e_region_%s: ncls=%d (1 to 8 classes)'
SIZE = 's2e_region_%s: H=%d W=%d Hl=%d Wl=%d (every size must be at least 1)'
LIMIT = 's2e_region_%s: N=%d H=%d W=%d is beyond the launch limits (N <= 65535, H W <= 2^24, N H W < 2^31)'
#              dtype x  y  label N  H   W   Hl  Wl ncls norm weights stats loss coef ws ws_bytes stream
FWD_ERRORS = [
    ((BF16, None, P, P, 2, 16, 16, 16, 16, 4, L1, P, P, P, P, P, BIG, None), -1, ARG % 'loss_fwd'),
    ((BF16, P, None, P, 2, 16, 16, 16, 16, 4, L1, P, P, P, P, P, BIG, None), -1, ARG % 'loss_fwd'),
    ((BF16, P, P, None, 2, 16, 16, 16, 16, 4, L1, P, P, P, P, P, BIG, None), -1, ARG % 'loss_fwd'),
    ((F32, P, P, P, 2, 16, 16, 16, 16, 4, L1, None, P, P, P, P, BIG, None), -1, ARG % 'loss_fwd'),
    ((F32, P, P, P, 2, 16, 16, 16, 16, 4, L1, P, None, P, P, P, BIG, None), -1, ARG % 'loss_fwd'),
    ((F32, P, P, P, 2, 16, 16, 16, 16, 4, L1, P, P, None, P, P, BIG, None), -1, ARG % 'loss_fwd'),
    ((F32, P, P, P, 2, 16, 16, 16, 16, 4, L1, P, P, P, None, P, BIG, None), -1, ARG % 'loss_fwd'),
    ((F32, P, P, P, 2, 16, 16, 16, 16, 4, L1, P, P, P, P, None, BIG, None), -1, ARG % 'loss_fwd'),
    ((F32, P, P, P, 0, 16, 16, 16, 16, 4, L1, P, P, P, P, P, BIG, None), -1, ARG % 'loss_fwd'),
    ((BAD, P, P, P, 2, 16, 16, 16, 16, 9, 5, P, P, P, P, P, BIG, None), -1, 's2e_region_loss_fwd: bad dtype 7'),      # the dtype first ...
    ((F32, P, P, P, 2, 16, 16, 16, 16, 9, 5, P, P, P, P, P, BIG, None), -1, 's2e_region_loss_fwd: bad norm 5'),       # ... then the norm ...
    ((F32, P, P, P, 2, 0, 16, 16, 16, 9, L2, P, P, P, P, P, BIG, None), -3, NCLS % ('loss_fwd', 9)),                  # ... the classes ...
    ((F32, P, P, P, 2, 16, 16, 16, 16, 0, L2, P, P, P, P, P, BIG, None), -3, NCLS % ('loss_fwd', 0)),
    ((BF16, P, P, P, 2, 0, 16, 16, 16, 4, L1, P, P, P, P, P, BIG, None), -3, SIZE % ('loss_fwd', 0, 16, 16, 16)),     # ... the sizes ...
    ((BF16, P, P, P, 2, 16, -1, 16, 16, 4, L1, P, P, P, P, P, BIG, None), -3, SIZE % ('loss_fwd', 16, -1, 16, 16)),
    ((BF16, P, P, P, 2, 16, 16, 0, 16, 4, L1, P, P, P, P, P, BIG, None), -3, SIZE % ('loss_fwd', 16, 16, 0, 16)),
    ((BF16, P, P, P, 2, 16, 16, 16, 0, 4, L1, P, P, P, P, P, BIG, None), -3, SIZE % ('loss_fwd', 16, 16, 16, 0)),
    ((F32, P, P, P, 65536, 1, 1, 1, 1, 4, L1, P, P, P, P, P, BIG, None), -3, LIMIT % ('loss_fwd', 65536, 1, 1)),      # ... the limits ...
    ((F32, P, P, P, 1, 4097, 4096, 16, 16, 4, L1, P, P, P, P, P, BIG, None), -3, LIMIT % ('loss_fwd', 1, 4097, 4096)),
    ((F32, P, P, P, 128, 4096, 4096, 16, 16, 4, L1, P, P, P, P, P, 1 << 40, None), -3, LIMIT % ('loss_fwd', 128, 4096, 4096)),
    ((F32, P, P, P, 2, 256, 256, 256, 256, 4, L1, P, P, P, P, P, 3071, None), -1, 's2e_region_loss_fwd: workspace of 3071 bytes, needs 3072'),
    ((F32, P, P, P, 2, 256, 0, 256, 256, 4, L1, P, P, P, P, P, 0, None), -3, SIZE % ('loss_fwd', 256, 0, 256, 256)),  # ... before the workspace
]
#             a  b  label N  H    W    Hl   Wl  ncls stats ws ws_bytes stream
U8_ERRORS = [
    ((None, P, P, 1, 640, 400, 256, 256, 4, P, P, BIG, None), -1, ARG % 'stats_u8'),
    ((P, None, P, 1, 640, 400, 256, 256, 4, P, P, BIG, None), -1, ARG % 'stats_u8'),
    ((P, P, None, 1, 640, 400, 256, 256, 4, P, P, BIG, None), -1, ARG % 'stats_u8'),
    ((P, P, P, 1, 640, 400, 256, 256, 4, None, P, BIG, None), -1, ARG % 'stats_u8'),
    ((P, P, P, 1, 640, 400, 256, 256, 4, P, None, BIG, None), -1, ARG % 'stats_u8'),
    ((P, P, P, -1, 640, 400, 256, 256, 4, P, P, BIG, None), -1, ARG % 'stats_u8'),
    ((P, P, P, 1, 640, 400, 256, 256, 9, P, P, BIG, None), -3, NCLS % ('stats_u8', 9)),
    ((P, P, P, 1, 640, 400, 0, 256, 4, P, P, BIG, None), -3, SIZE % ('stats_u8', 640, 400, 0, 256)),
    ((P, P, P, 65536, 11, 11, 11, 11, 4, P, P, BIG, None), -3, LIMIT % ('stats_u8', 65536, 11, 11)),
    ((P, P, P, 1, 640, 400, 256, 256, 4, P, P, 63 * 4 * 24 - 8, None), -1, 's2e_region_stats_u8: workspace of 6040 bytes, needs 6048'),
]
#              dtype x  y  label coef gloss N  H   W   Hl  Wl ncls norm dx stream
BWD_ERRORS = [
    ((BF16, None, P, P, P, P, 2, 16, 16, 16, 16, 4, L1, P, None), -1, ARG % 'loss_bwd'),
    ((BF16, P, None, P, P, P, 2, 16, 16, 16, 16, 4, L1, P, None), -1, ARG % 'loss_bwd'),
    ((BF16, P, P, None, P, P, 2, 16, 16, 16, 16, 4, L1, P, None), -1, ARG % 'loss_bwd'),
    ((F32, P, P, P, None, P, 2, 16, 16, 16, 16, 4, L1, P, None), -1, ARG % 'loss_bwd'),
    ((F32, P, P, P, P, None, 2, 16, 16, 16, 16, 4, L1, P, None), -1, ARG % 'loss_bwd'),
    ((F32, P, P, P, P, P, 2, 16, 16, 16, 16, 4, L1, None, None), -1, ARG % 'loss_bwd'),
    ((F32, P, P, P, P, P, 0, 16, 16, 16, 16, 4, L1, P, None), -1, ARG % 'loss_bwd'),
    ((BAD, P, P, P, P, P, 2, 16, 16, 16, 16, 4, -1, P, None), -1, 's2e_region_loss_bwd: bad dtype 7'),
    ((BF16, P, P, P, P, P, 2, 16, 16, 16, 16, 12, 2, P, None), -1, 's2e_region_loss_bwd: bad norm 2'),
    ((BF16, P, P, P, P, P, 2, 16, 0, 16, 16, 12, L2, P, None), -3, NCLS % ('loss_bwd', 12)),
    ((BF16, P, P, P, P, P, 2, 16, 0, 16, 16, 4, L2, P, None), -3, SIZE % ('loss_bwd', 16, 0, 16, 16)),
    ((F32, P, P, P, P, P, 32768, 256, 256, 256, 256, 4, L1, P, None), -3, LIMIT % ('loss_bwd', 32768, 256, 256)),
]


def test_region_entry_points_reject_bad_calls_before_any_launch():
    """Null pointers, N <= 0, a bad dtype or norm, a short workspace: S2E_ERR_ARG; ncls outside 1..8, a size below 1 or a grid beyond the
    launch limits: S2E_ERR_UNSUPPORTED; the message, and which check wins.  Host-only: with a GPU visible the test skips itself, so that a
    dummy pointer can never reach a kernel (as test_ssim_entry_points_reject_bad_calls_before_any_launch does)."""
    if torch.cuda.is_available():
        pytest.skip('dummy pointers: host-only by construction')
    from seg2eye_amd import _lib
    assert (_lib.S2E_BF16, _lib.S2E_F32, _lib.REGION_L1, _lib.REGION_L2) == (BF16, F32, L1, L2)
    for name, table in (('s2e_region_loss_fwd', FWD_ERRORS), ('s2e_region_stats_u8', U8_ERRORS), ('s2e_region_loss_bwd', BWD_ERRORS)):
        check_error_table(name, table)
    with pytest.raises(_lib.Seg2EyeHipError, match='s2e_region_loss_fwd failed'):
        _lib.call.s2e_region_loss_fwd(*FWD_ERRORS[0][0])


def test_workspace_bytes_is_positive_and_monotone():
    """One {count, sum |d|, sum d^2} fp64 record per class, 4096-pixel block and image: positive for every legal size, never smaller for a
    larger N, H, W or ncls, 0 where there is nothing to reduce.  A host-only query."""
    from seg2eye_amd import _lib
    ws = _lib.lib().s2e_region_workspace_bytes
    assert isinstance(ws(1, 1, 1, 1), int) and ws(1, 1, 1, 1) == 24 and ws(2, 256, 256, 4) == 2 * 16 * 4 * 24 and ws(1, 640, 400, 4) == 63 * 4 * 24
    assert ws(0, 64, 64, 4) == 0 and ws(-1, 64, 64, 4) == 0 and ws(2, 0, 64, 4) == 0 and ws(2, 64, 0, 4) == 0
    assert ws(2, 64, 64, 0) == 0 and ws(2, 64, 64, 9) == 0
    sizes = [1, 3, 17, 63, 64, 65, 100, 256, 400, 640]
    for ncls in (1, 4, 8):
        for n in (1, 2, 3, 8):
            for i, h in enumerate(sizes):
                for j, w in enumerate(sizes):
                    b = ws(n, h, w, ncls)
                    assert b > 0 and b % 24 == 0 and ws(n + 1, h, w, ncls) > b, (n, h, w, ncls)
                    if i:
                        assert b >= ws(n, sizes[i - 1], w, ncls), (n, h, w, ncls)
                    if j:
                        assert b >= ws(n, h, sizes[j - 1], ncls), (n, h, w, ncls)
                    if ncls > 1:
                        assert b > ws(n, h, w, ncls - 1)
    assert ws(1, 64, 64, 4) == 96 and ws(1, 64, 65, 4) == 192  # the 4097th pixel: one more block
    assert ctypes.sizeof(ctypes.c_size_t) == 8
