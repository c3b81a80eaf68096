"""The residual refiner without a GPU: the restatement the GPU tests compare against (tests/_refine_ref.py) checked
against the reference's literal formulas under torch autograd, the facts of the uint8 round trip, the sampler of seg2eye_amd/refine.py
on a synthetic store, the options, the ops' argument checks that need no device and the library's argument errors."""
import numpy as np
import pytest
import torch

import _refine_ref as R
import _segment_ref as S
import _style_rank_ref as K


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('lambdas', [(1.0, 0.0), (0.0, 1.0), (0.7, 0.3)], ids=['eds', 'l1', 'both'])
@pytest.mark.parametrize('kind', ['mixed', 'clampy', 'zero'])
def test_restatement_agrees_with_the_literal_formulas_under_autograd(kind, lambdas):
    """fp64 on both sides: clamp, sqrt(sum((255 / 2 d)^2)) / (H W), mean |d| (refinenet/model.py:38-62) through torch autograd against
    the closed forms of _refine_ref.head -- with pixels clamped on both sides, pixels exactly at +-1 under a zero residual (torch.clamp
    passes their gradient) and pixels with d == 0 (sign(0) = 0)."""
    _, rimg, _, truth = R.planes((3, 6, 9), seed=4)
    res, truth = R.residual(kind, rimg, truth, 2, seed=5)
    res[..., 1] = 0.25                                           # (a finite dead channel: its gradient is 0 on both sides)
    s = res[..., 0].astype(np.float64) + R.norm(rimg)
    if kind == 'mixed':
        assert (s > 1).any() and (s < -1).any() and (s == 1).any() and (s == -1).any()
        assert ((np.clip(s, -1, 1) - R.norm(truth)) == 0).any()
    want = R.head(res, rimg, truth, None, lambdas[0], lambdas[1], g=1.75)
    t = torch.from_numpy(res.astype(np.float64)).requires_grad_(True)
    loss, per = R.loss_torch(t, rimg, truth, *lambdas)
    (1.75 * loss).backward()
    assert abs(float(loss.detach()) - float(want['loss'])) <= 1e-14 * max(1.0, abs(float(want['loss'])))
    np.testing.assert_allclose(per.detach().numpy(), want['score'], rtol=1e-13, atol=0)
    np.testing.assert_allclose(t.grad.numpy(), want['grad'], rtol=1e-12, atol=1e-18)
    assert want['terms'][2] == 1471 * want['terms'][0] and np.abs(want['grad'][..., 0]).max() > 0
    assert not want['grad'][..., 1:].any()


def test_restatement_of_an_exact_prediction_is_finite_and_zero():
    """sumsq == 0: torch's sqrt gives a NaN gradient, the stated deviation gives 0 for the eds term; the other image keeps its gradient."""
    _, rimg, _, truth = R.planes((2, 4, 6), seed=6)
    res, truth = R.residual('exact', rimg, truth, 1, seed=7)
    h = R.head(res, rimg, truth, None, 1.0, 0.5)
    assert h['sumsq'][0] == 0 and h['score'][0] == 0 and h['sumsq'][1] > 0
    assert np.isfinite(h['grad']).all() and not h['grad'][0].any() and h['grad'][1].any()
    t = torch.from_numpy(res.astype(np.float64)).requires_grad_(True)
    R.loss_torch(t, rimg, truth)[0].backward()
    assert torch.isnan(t.grad[0]).any()


def test_flip_mirrors_every_plane_alike():
    """The loss of (res, flipped planes) equals the loss of (res mirrored, planes) mirrored back: a flip is a change of coordinates."""
    _, rimg, _, truth = R.planes((2, 3, 5), seed=8)
    res, truth = R.residual('mixed', rimg, truth, 1, seed=9)
    flip = np.array([1, 0], dtype=np.uint8)
    a = R.head(res, rimg, truth, flip)
    b = R.head(res, R.flipped(rimg, flip), R.flipped(truth, flip), None)
    assert a['loss'] == b['loss'] and np.array_equal(a['grad'], b['grad'])
    assert np.array_equal(R.predict_u8(res, rimg, flip), R.predict_u8(res, R.flipped(rimg, flip)))
    assert not np.array_equal(R.flipped(rimg, flip)[0], rimg[0]) and np.array_equal(R.flipped(rimg, flip)[1], rimg[1])


def test_the_uint8_round_trip_loses_one_level_for_47_of_256():
    """(uint8)(127.5 (norm(v) + 1)) with the fp32 roundings of the rule and a truncation: v - 1 for 47 levels, v for the others, never
    further off.  So an untrained refiner returns its reference frame only to within one level."""
    v = np.arange(256, dtype=np.uint8).reshape(1, 16, 16)
    q = R.predict_u8(np.zeros((1, 16, 16, 1), dtype=np.float32), v).astype(np.int64)
    off = v.astype(np.int64) - q
    assert int((off == 1).sum()) == 47 and int((off == 0).sum()) == 209
    assert q[0, 0, 0] == 0 and q[0, 15, 15] == 255
    x = R.norm(v)
    assert x.dtype == np.float32 and x.min() == -1.0 and x.max() == 1.0


def test_colour_levels_and_labels_past_the_classes():
    mask = np.array([[[0, 1, 2, 3, 4, 200, 255]]], dtype=np.uint8)
    assert R.colourise(mask).tolist() == [[[125, 103, 76, 34, 0, 0, 0]]]
    assert R.colourise(mask, ncls=2).tolist() == [[[125, 103, 0, 0, 0, 0, 0]]]
    assert R.colourise(mask, levels=(9, 8, 7), ncls=3).tolist() == [[[9, 8, 7, 0, 0, 0, 0]]]
    frame = np.full((1, 1, 7), 255, dtype=np.uint8)
    x = R.refine_input(mask, frame, mask[:, :, ::-1], C=5)
    assert x.shape == (1, 1, 7, 5) and x.dtype == np.float32 and not x[..., 3:].any()
    assert np.array_equal(x[..., 0], R.norm(R.colourise(mask))) and (x[..., 1] == 1).all()
    assert np.array_equal(x[..., 2], R.norm(R.colourise(mask))[:, :, ::-1])
    from seg2eye_amd.ops import refine as ops_refine
    assert ops_refine.CLASS_LEVELS == R.LEVELS == (125, 103, 76, 34)        # int(125.73929), int(103.19314), int(76.50751), int(34.1294)


# ------------------------------------------------------------------------------------------------ the sampler
def _store():
    """learnable_store at 64 x 40 with its kept-aside truth as the masks, the host restatement of style_rank for the ranking, and a
    hand-made 'test' split: two labelled frames, three sequence frames, two target masks."""
    store, seg = S.learnable_store(H=64, W=40)
    refs = {**K.rank_styles(store, 'train', seg_store=seg, top=4), **K.rank_styles(store, 'validation', seg_store=seg, top=4)}
    lab = S.eyes(7, 64, 40, 4, seed=31)
    img = S.eye_frames(lab, 'test/U301', 31)
    store['test'] = {'U301': {'images_ss': img[:2], 'labels_ss': lab[:2], 'images_seq': img[2:5], 'labels_gen': lab[5:7],
                              'labels_gen_filenames': np.array([b'U301.g000', b'U301.g001'], dtype='S13')}}
    seg['test'] = {'U301': {'labels_pred_seq': lab[2:5]}}
    refs['test'] = {'U301': {'U301g000': {'index': np.array([1, 4], dtype=np.int64), 'subset': np.array([b'g', b's'], dtype='S1')},
                             'U301g001': {'index': np.array([2, 0], dtype=np.int64), 'subset': np.array([b's', b'g'], dtype='S1')}}}
    return store, seg, refs


def _resolved(store, pick, key, user):
    image_key, row, holder, mask_key = pick
    return np.asarray(store[key][user][image_key][row]), np.asarray(holder[mask_key][row])


def test_sampler_resolves_both_subsets_and_the_test_split():
    from seg2eye_amd import refine
    store, seg, refs = _store()
    seen = set()
    for key in ('train', 'validation', 'test'):
        todo = refine.targets(store, key)
        assert todo == R.target_list(store, key) and len(todo) == {'train': 18, 'validation': 12, 'test': 2}[key]
        for user, _, fname in todo:
            for pos in range(len(refs[key][user][fname]['index'])):
                class At:                                                   # a "generator" whose draw is `pos`
                    @staticmethod
                    def randint(lo, hi):
                        assert lo == 0 and hi == len(refs[key][user][fname]['index'])
                        return pos
                pick = refine.pick_reference(store, seg, refs, key, user, fname, top=100, rng=At)
                frame, mask = _resolved(store, pick, key, user)
                want = R.expected_reference(store, seg, refs, key, user, fname, pos)
                assert np.array_equal(frame, want[0]) and np.array_equal(mask, want[1])
                seen.add((key, bytes(refs[key][user][fname]['subset'][pos]), pick[0], pick[3]))
    assert seen == {('train', b'g', 'images_gen', 'labels_pred_gen'), ('train', b's', 'images_seq', 'labels_pred_seq'),
                    ('validation', b'g', 'images_gen', 'labels_pred_gen'), ('validation', b's', 'images_seq', 'labels_pred_seq'),
                    ('test', b'g', 'images_ss', 'labels_ss'), ('test', b's', 'images_seq', 'labels_pred_seq')}
    # the test split's b'g' masks are the store's true labels, its sequence indices sit behind the two labelled frames
    assert refine.pick_reference(store, seg, refs, 'test', 'U301', 'U301g000')[2:] == (store['test']['U301'], 'labels_ss')
    assert refine.pick_reference(store, seg, refs, 'test', 'U301', 'U301g001')[:2] == ('images_seq', 0)
    assert refine.pick_reference(store, None, refs, 'test', 'U301', 'U301g000')[:2] == ('images_ss', 1)      # needs no --seg_file


def test_sampler_takes_the_first_candidate_or_a_seeded_draw_among_the_top():
    from seg2eye_amd import refine
    store, seg, refs = _store()
    todo = refine.targets(store, 'train')
    first = [refine.pick_reference(store, seg, refs, 'train', u, f)[:2] for u, _, f in todo]
    want = []
    for u, _, f in todo:                                                    # pick1: entry 0, whatever `top` says
        e = refs['train'][u][f]
        want.append(('images_gen', int(e['index'][0])) if bytes(e['subset'][0]) == b'g' else ('images_seq', int(e['index'][0]) - 4))
    assert first == want == [refine.pick_reference(store, seg, refs, 'train', u, f, top=4)[:2] for u, _, f in todo]

    def draws(seed, top):
        rng = np.random.RandomState(seed)
        return [refine.pick_reference(store, seg, refs, 'train', u, f, top, rng)[:2] for u, _, f in todo]
    assert draws(5, 4) == draws(5, 4) and draws(5, 4) != draws(6, 4) and draws(5, 4) != first
    assert draws(5, 1) == first and draws(5, 100) == draws(5, 4)            # top is cut to the candidates listed
    rng = np.random.RandomState(5)                                          # the restatement's draw: one randint per target
    pos = [int(rng.randint(0, 4)) for _ in todo]
    for (u, _, f), p, got in zip(todo, pos, draws(5, 4)):
        e = refs['train'][u][f]
        assert got == (('images_gen', int(e['index'][p])) if bytes(e['subset'][p]) == b'g' else ('images_seq', int(e['index'][p]) - 4))
    batch = todo[:3]
    picks = [refine.pick_reference(store, seg, refs, 'train', u, f) for u, _, f in batch]
    tmask, rimg, rmask, truth = refine.gather(store, 'train', batch, picks)
    assert all(a.dtype == np.uint8 and a.shape == (3, 64, 40) for a in (tmask, rimg, rmask, truth))
    assert np.array_equal(tmask[1], store['train'][batch[1][0]]['labels_ss'][batch[1][1]])
    assert np.array_equal(truth[2], store['train'][batch[2][0]]['images_ss'][batch[2][1]])
    assert np.array_equal(rimg[0], R.expected_reference(store, seg, refs, 'train', batch[0][0], batch[0][2])[0])
    assert np.array_equal(rmask[0], R.expected_reference(store, seg, refs, 'train', batch[0][0], batch[0][2])[1])
    assert refine.gather(store, 'test', refine.targets(store, 'test')[:1],
                         [refine.pick_reference(store, seg, refs, 'test', 'U301', 'U301g000')])[3] is None


def test_sampler_errors_name_the_person_and_the_file():
    from seg2eye_amd import refine
    store, seg, refs = _store()
    user, _, fname = refine.targets(store, 'train')[0]

    def entry(index, subset):
        return {'train': {user: {fname: {'index': np.array(index, dtype=np.int64), 'subset': np.array(subset, dtype='S1')}}}}
    cases = [({'train': {user: {}}}, seg, 'no entry'), ({'train': {}}, seg, 'no entry'), (entry([], []), seg, 'lists no candidate'),
             (entry([4], [b'g']), seg, 'row 4 of 4 images_gen'), (entry([3], [b's']), seg, 'row -1 of 4 images_seq'),
             (entry([8], [b's']), seg, 'row 4 of 4 images_seq'), (entry([0], [b'x']), seg, 'unknown subset'),
             (entry([0], [b'g']), {'train': {}}, 'hold no train/%s/labels_pred_gen' % user), (entry([0], [b'g']), None, 'labels_pred_gen'),
             (entry([0], [b'g']), {'train': {user: {'labels_pred_gen': seg['train'][user]['labels_pred_gen'][:3]}}}, '3 masks labels_pred_gen for 4 images_gen')]
    for bad_refs, bad_seg, text in cases:
        with pytest.raises(ValueError) as e:
            refine.pick_reference(store, bad_seg, bad_refs, 'train', user, fname)
        assert user in str(e.value) and fname in str(e.value) and text in str(e.value), (text, str(e.value))
    with pytest.raises(ValueError, match='no target masks'):
        list(refine._first_batches({'validation': {}}, seg, refs, 'validation', refine.refine_options()))
    with pytest.raises(ValueError, match='no ground truth'):
        refine.evaluate(None, store, seg, refs, 'test', refine.refine_options())


def test_refine_options_and_the_command_line():
    from seg2eye_amd import refine
    o = refine.refine_options(nrf=8, lr=2e-3, refine_top=4)
    assert (o.nrf, o.lr, o.refine_top, o.lambda_eds, o.lambda_l1, o.compute_dtype, o.no_flip) == (8, 2e-3, 4, 1.0, 0.0, 'bf16', False)
    with pytest.raises(TypeError, match='nsf, seg_hw'):
        refine.refine_options(nsf=8, seg_hw=(64, 40))
    with pytest.raises(ValueError, match='refine_top'):
        refine.refine_options(refine_top=0)
    a = vars(refine.parser().parse_args(['train', '--dataroot', 'd.npz', '--style_ref', 'a.npz,b.npz', '--seg_file', 'm.npz', '--nrf', '16',
                                         '--lambda_l1', '0.5', '--no_flip', '--refine_top', '10']))
    for k in ('command', 'dataroot', 'style_ref', 'seg_file'):
        a.pop(k)
    o = refine.refine_options(**a)                                          # every flag of `train` is an option
    assert (o.nrf, o.lambda_l1, o.no_flip, o.refine_top, o.niter) == (16, 0.5, True, 10, 20)
    p = vars(refine.parser().parse_args(['predict', '--dataroot', 'd.npz', '--style_ref', 'a.npz', '--out', 'sub']))
    assert p['dataset_key'] == 'test' and p['out'] == 'sub' and p['seg_file'] is None
    assert vars(refine.parser().parse_args(['eval', '--dataroot', 'd', '--style_ref', 'a']))['dataset_key'] == 'validation'


def test_network_layer_plan_and_zero_filled_out():
    from seg2eye_amd import refine, segment
    net = refine.build_network(refine.refine_options(nrf=8, compute_dtype='fp32'), 'cpu')
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == R.manifest(8)
    assert not net.out.weight.any() and not net.out.bias.any() and net.e0.weight.any() and net.d0.weight.any()
    seg_net = segment.build_network(segment.seg_options(nsf=8), 'cpu')         # the segmenter keeps its keys and shapes
    assert [(k, tuple(v.shape)) for k, v in seg_net.state_dict().items()] == S.manifest(8)
    with pytest.raises(ValueError, match='nrf'):
        refine.build_network(refine.refine_options(nrf=12), 'cpu')
    from seg2eye_amd import _lib
    with pytest.raises(_lib.Seg2EyeHipError):
        net(torch.zeros(1, 8, 8, 8))


# ------------------------------------------------------------------------------------------------ the ops' argument checks
def test_op_argument_checks_come_before_the_device_check():
    from seg2eye_amd import ops, _lib
    u8 = torch.zeros(2, 8, 8, dtype=torch.uint8)
    res = torch.zeros(2, 8, 8, 1)
    bad = [
        (lambda: ops.refine_input(u8.float(), u8, u8), 'tmask: uint8'),
        (lambda: ops.refine_input(u8, u8[0], u8), r'rimg: \(N, H, W\)'),
        (lambda: ops.refine_input(u8, u8, u8[:, :4]), 'rmask: .* as tmask'),
        (lambda: ops.refine_input(u8, u8, u8, flip=torch.zeros(2)), 'flip: uint8 or bool'),
        (lambda: ops.refine_input(u8, u8, u8, flip=torch.zeros(3, dtype=torch.uint8)), 'flip: one byte per image'),
        (lambda: ops.refine_input(u8, u8, u8, dtype=torch.float16), 'bf16 or fp32'),
        (lambda: ops.refine_input(u8, u8, u8, ncls=0), 'ncls = 0'),
        (lambda: ops.refine_input(u8, u8, u8, ncls=17), 'ncls = 17'),
        (lambda: ops.refine_input(u8, u8, u8, channels=2), 'channels = 2'),
        (lambda: ops.refine_input(u8, u8, u8, levels=(1, 2, 3)), 'levels: 4 grey levels'),
        (lambda: ops.refine_input(u8, u8, u8, levels=(1, 2, 3, 256)), 'levels: 4 grey levels'),
        (lambda: ops.refine_input(u8, u8, u8, levels=torch.zeros(4)), r'levels: uint8 \(4,\)'),
        (lambda: ops.refine_loss(res.double(), u8, u8), 'bf16 or fp32 residual'),
        (lambda: ops.refine_loss(res[..., 0], u8, u8), 'res: '),
        (lambda: ops.refine_loss(res[:1], u8, u8), 'res: '),
        (lambda: ops.refine_loss(res, u8, u8.int()), 'truth: uint8'),
        (lambda: ops.refine_loss(res, u8, u8[:, :, :4]), 'truth: .* as rimg'),
        (lambda: ops.refine_loss(res, u8, u8, lambda_eds=-1.0), 'lambda_eds'),
        (lambda: ops.refine_loss(res, u8, u8, lambda_l1=float('nan')), 'lambda_l1'),
        (lambda: ops.refine_loss(res, u8, u8, flip=torch.zeros(2, 1, dtype=torch.uint8)), 'flip: one byte per image'),
        (lambda: ops.refine_predict_u8(res.half(), u8), 'bf16 or fp32 residual'),
        (lambda: ops.refine_predict_u8(res, u8.float()), 'rimg: uint8'),
        (lambda: ops.refine_predict_u8(torch.zeros(2, 8, 8, 0), u8), 'res: '),
    ]
    for call, text in bad:
        with pytest.raises(ValueError, match=text):
            call()
    for call in (lambda: ops.refine_input(u8, u8, u8), lambda: ops.refine_loss(res, u8, u8, flip=torch.zeros(2, dtype=torch.bool)),
                 lambda: ops.refine_predict_u8(res, u8)):
        with pytest.raises(_lib.Seg2EyeHipError, match='GPU only'):           # valid arguments on the host: no CPU path
            call()


def test_library_refuses_bad_calls_before_any_launch():
    """Every call below fails a check, so no dummy pointer reaches a kernel: codes, messages and which check wins."""
    from seg2eye_amd import _lib
    L = _lib.lib()
    F32, BF16, P = _lib.S2E_F32, _lib.S2E_BF16, 4096            # P: a non-null, 8-byte aligned stand-in for a pointer
    ARG, UNS = -1, -3
    table = [
        ('s2e_refine_input', (F32, None, P, P, None, P, 4, 1, 8, 8, 8, P, None), ARG, 'bad argument'),
        ('s2e_refine_input', (F32, P, P, P, None, None, 4, 1, 8, 8, 8, P, None), ARG, 'bad argument'),
        ('s2e_refine_input', (7, P, P, P, None, P, 4, 1, 8, 8, 8, P, None), ARG, 'bad dtype 7'),
        ('s2e_refine_input', (BF16, P, P, P, None, P, 4, 0, 8, 8, 8, P, None), ARG, 'N=0'),
        ('s2e_refine_input', (BF16, P, P, P, None, P, 4, 1, 8, 0, 8, P, None), ARG, 'W=0'),
        ('s2e_refine_input', (BF16, P, P, P, None, P, 4, 1, 8, 8, 2, P, None), ARG, 'C=2 (at least 3 channels)'),
        ('s2e_refine_input', (BF16, P, P, P, None, P, 4, 70000, 8, 8, 8, P, None), UNS, 'beyond the launch limits'),
        ('s2e_refine_input', (BF16, P, P, P, None, P, 4, 1, 40000, 40000, 8, P, None), UNS, 'H W <= 2^30'),
        ('s2e_refine_input', (BF16, P, P, P, None, P, 0, 1, 8, 8, 8, P, None), UNS, 'ncls=0'),
        ('s2e_refine_input', (BF16, P, P, P, None, P, 17, 1, 8, 8, 8, P, None), UNS, 'ncls=17'),
        ('s2e_refine_head_fwd', (F32, P, 1, P, P, None, 1, 8, 8, P, P, P, None, 1 << 20, None), ARG, 'bad argument'),
        ('s2e_refine_head_fwd', (F32, P, 1, P, P, None, 1, 8, 8, P, P, P, P + 4, 1 << 20, None), ARG, 'bad argument'),
        ('s2e_refine_head_fwd', (F32, P, 1, P, None, None, 1, 8, 8, P, P, P, P, 1 << 20, None), ARG, 'bad argument'),
        ('s2e_refine_head_fwd', (3, P, 1, P, P, None, 1, 8, 8, P, P, P, P, 1 << 20, None), ARG, 'bad dtype 3'),
        ('s2e_refine_head_fwd', (F32, P, 0, P, P, None, 1, 8, 8, P, P, P, P, 1 << 20, None), ARG, 'C=0 (at least 1 channel)'),
        ('s2e_refine_head_fwd', (F32, P, 1, P, P, None, 1, 0, 8, P, P, P, P, 1 << 20, None), ARG, 'H=0'),
        ('s2e_refine_head_fwd', (F32, P, 1, P, P, None, 2, 640, 400, P, P, P, P, 2 * 63 * 16 - 1, None), ARG, 'workspace of 2015 bytes, needs 2016'),
        ('s2e_refine_head_fwd', (F32, P, 1, P, P, None, 65536, 8, 8, P, P, P, P, 1 << 20, None), UNS, 'beyond the launch limits'),
        ('s2e_refine_head_bwd', (F32, P, 1, P, P, None, 1, 8, 8, None, P, 1.0, 0.0, P, None), ARG, 'bad argument'),
        ('s2e_refine_head_bwd', (F32, P, 1, P, P, None, 1, 8, 8, P, None, 1.0, 0.0, P, None), ARG, 'bad argument'),
        ('s2e_refine_head_bwd', (F32, P, 1, P, P, None, 1, 8, 8, P, P, 1.0, 0.0, None, None), ARG, 'bad argument'),
        ('s2e_refine_head_bwd', (9, P, 1, P, P, None, 1, 8, 8, P, P, 1.0, 0.0, P, None), ARG, 'bad dtype 9'),
        ('s2e_refine_head_bwd', (BF16, P, 0, P, P, None, 1, 8, 8, P, P, 1.0, 0.0, P, None), ARG, 'C=0'),
        ('s2e_refine_head_bwd', (BF16, P, 1, P, P, None, 1, 8, -1, P, P, 1.0, 0.0, P, None), ARG, 'W=-1'),
        ('s2e_refine_predict_u8', (F32, None, 1, P, None, 1, 8, 8, P, None), ARG, 'bad argument'),
        ('s2e_refine_predict_u8', (F32, P, 1, P, None, 1, 8, 8, None, None), ARG, 'bad argument'),
        ('s2e_refine_predict_u8', (-1, P, 1, P, None, 1, 8, 8, P, None), ARG, 'bad dtype -1'),
        ('s2e_refine_predict_u8', (F32, P, 0, P, None, 1, 8, 8, P, None), ARG, 'C=0'),
        ('s2e_refine_predict_u8', (F32, P, 1, P, None, 0, 8, 8, P, None), ARG, 'N=0'),
        ('s2e_refine_predict_u8', (F32, P, 1, P, None, 1, 1 << 16, 1 << 16, P, None), UNS, 'H W <= 2^30'),
    ]
    for name, args, code, text in table:
        rc = getattr(L, name)(*args)
        msg = L.s2e_last_error().decode()
        assert rc == code and name in msg and text in msg, (name, args, rc, msg)
    size = L.s2e_refine_head_workspace_bytes
    assert size(2, 640, 400) == 2 * 63 * 16 and size(1, 1, 1) == 16 and size(3, 64, 64) == 3 * 16 and size(1, 64, 65) == 2 * 16
    assert size(0, 8, 8) == 0 and size(1, 0, 8) == 0 and size(65536, 8, 8) == 0 and size(1, 1 << 16, 1 << 16) == 0
    with pytest.raises(_lib.Seg2EyeHipError, match='s2e_refine_predict_u8 failed'):
        _lib.call.s2e_refine_predict_u8(F32, P, 0, P, None, 1, 8, 8, P, None)
