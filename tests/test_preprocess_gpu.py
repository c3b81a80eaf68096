"""--device_preprocess on the GPU: the bicubic kernel against Pillow's committed outputs and the numpy restatement of
its rule, the nearest kernel against `resize_nearest`, `materialize` against the host-mode batch, one G+D step and one training
epoch from raw batches.  EXACT equality throughout: integer arithmetic plus a lookup table leaves no room for differences."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from test_preprocess_host import CASES, CASE_IDS, KINDS, ROW_STEP, case_input, case_name, fake_openeds_store

pytestmark = pytest.mark.gpu
FLIPS = [0, 1, 0]
_REF = {}


def reference(ci, kind):
    """(frames (3, H, W) uint8, expected (3, Ho, Wo) uint8 after the flips) of a case, computed once."""
    from seg2eye_amd.ops.preprocess import resize_bicubic_u8_reference
    if (ci, kind) not in _REF:
        src, dst = CASES[ci]
        frames = case_input(ci, src, kind)
        want = np.stack([resize_bicubic_u8_reference(f, dst[1], dst[0]) for f in frames])
        for m, fl in enumerate(FLIPS):
            if fl:
                want[m] = want[m, :, ::-1]
        frames.setflags(write=False)
        want.setflags(write=False)
        _REF[(ci, kind)] = (frames, want)
    return _REF[(ci, kind)]


@pytest.mark.parametrize('ci', range(len(CASES)), ids=CASE_IDS)
@pytest.mark.parametrize('kind', KINDS)
def test_bicubic_kernel_is_pillow_exact(ci, kind):
    from seg2eye_amd.ops import resize_bicubic_u8
    from seg2eye_amd.ops.preprocess import normalize_lut
    src, dst = CASES[ci]
    frames, want = reference(ci, kind)
    dev = torch.device('cuda:0')
    flip = torch.tensor(FLIPS, dtype=torch.bool, device=dev)
    out, out_u8 = resize_bicubic_u8(torch.from_numpy(frames.copy()).to(dev), dst[0], dst[1], flip, return_u8=True)
    only = resize_bicubic_u8(torch.from_numpy(frames.copy()).to(dev), dst[0], dst[1], flip)           # out_u8 = NULL
    torch.cuda.synchronize()
    got = out_u8.cpu().numpy()
    assert got.shape == (3,) + dst and out.shape == (3,) + dst and out.dtype == torch.float32
    # frame 0 is not flipped: Pillow's own bytes (the rows the fixture keeps)
    z = load_golden('pil_bicubic')
    step = ROW_STEP[kind].get(dst, 1)
    assert int((got[0, ::step] != z[case_name(src, dst, kind)]).sum()) == 0
    bad = int((got != want).sum())
    print('%s %s: %d mismatching of %d; %d saturated' % (CASE_IDS[ci], kind, bad, want.size, int(((want == 0) | (want == 255)).sum())))
    assert bad == 0
    want_f = normalize_lut()[torch.from_numpy(want.copy()).long()]
    assert torch.equal(out.cpu(), want_f) and torch.equal(only.cpu(), want_f)


@pytest.mark.parametrize('ci', range(len(CASES)), ids=CASE_IDS)
def test_nearest_kernel_is_the_host_rule(ci):
    from seg2eye_amd.openeds_dataset import resize_nearest
    from seg2eye_amd.ops import resize_nearest_u8
    src, dst = CASES[ci]
    labels = np.random.RandomState(77 + ci).randint(0, 4, (3,) + src).astype(np.uint8)
    dev = torch.device('cuda:0')
    got = resize_nearest_u8(torch.from_numpy(labels).to(dev), dst[0], dst[1], torch.tensor(FLIPS, dtype=torch.uint8, device=dev)).cpu().numpy()
    for m, fl in enumerate(FLIPS):
        want = resize_nearest(labels[m], dst[1], dst[0])
        assert np.array_equal(got[m], want[:, ::-1] if fl else want), (CASE_IDS[ci], m)


def test_unaligned_frames_and_odd_widths():
    """Frames that start at an odd address inside a larger allocation (the 16-byte loads' lead-in and the byte loads at both ends of
    the tensor), and an output width that is no multiple of 4 (the scalar store path)."""
    from seg2eye_amd.ops import resize_bicubic_u8, resize_nearest_u8
    from seg2eye_amd.openeds_dataset import resize_nearest
    from seg2eye_amd.ops.preprocess import resize_bicubic_u8_reference
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(9)
    for (H, W), (Ho, Wo), off in (((37, 23), (30, 19), 5), ((50, 41), (50, 62), 3), ((33, 40), (21, 40), 1)):
        frames = rng.randint(0, 256, (2, H, W)).astype(np.uint8)
        buf = torch.full((off + frames.size + 64,), 255, dtype=torch.uint8, device=dev)
        view = buf[off:off + frames.size].view(2, H, W)
        view.copy_(torch.from_numpy(frames))
        flip = torch.tensor([1, 0], dtype=torch.uint8, device=dev)
        _, got = resize_bicubic_u8(view, Ho, Wo, flip, return_u8=True)
        near = resize_nearest_u8(view, Ho, Wo, flip).cpu().numpy()
        got = got.cpu().numpy()
        for m in range(2):
            want = resize_bicubic_u8_reference(frames[m], Wo, Ho)
            wn = resize_nearest(frames[m], Wo, Ho)
            assert np.array_equal(got[m], want[:, ::-1] if m == 0 else want), ((H, W), (Ho, Wo), m)
            assert np.array_equal(near[m], wn[:, ::-1] if m == 0 else wn), ((H, W), (Ho, Wo), m)


class _Flips:
    """rng stub over a RandomState: the flip decisions alternate (so a batch of two carries both), everything else is drawn."""

    def __init__(self, seed):
        self.r, self.k = np.random.RandomState(seed), 0

    def random(self):
        self.k += 1
        return 0.9 if self.k % 2 else 0.1

    def choice(self, seq, n):
        return self.r.choice(seq, n)


def _twin_batches(crop, aspect, store, seed=11):
    from seg2eye_amd.openeds_dataset import OpenEDSDataset
    from seg2eye_amd.options import parse
    from torch.utils.data import default_collate
    argv = ['--dataset_mode', 'openeds', '--dataset_key', 'train', '--crop_size', str(crop), '--aspect_ratio', str(aspect),
            '--style_sample_method', 'random', '--batchSize', '2']
    host = OpenEDSDataset(parse(argv), store=store, rng=_Flips(seed))
    opt = parse(argv + ['--device_preprocess'])
    raw = OpenEDSDataset(opt, store=store, rng=_Flips(seed))
    return default_collate([host[1], host[5]]), default_collate([raw[1], raw[5]]), opt


@pytest.fixture(scope='module')
def store():
    return fake_openeds_store(seed=4)


@pytest.mark.parametrize('crop,aspect', [(64, 0.8), (256, 1.0)])
def test_materialize_equals_the_host_batch(store, crop, aspect):
    from seg2eye_amd.ops import materialize
    hb, rb, opt = _twin_batches(crop, aspect, store)
    assert rb['flip'].tolist() == [True, False]
    out = materialize(rb, opt, 'cuda:0')
    h = round(crop / aspect)
    assert out['label'].shape == (2, h, crop) and out['label'].dtype == torch.uint8 and out['label'].is_cuda
    assert out['style_image'].shape == (2, 4, 1, h, crop) and out['target'].shape == (2, 1, h, crop)
    for k in ('label', 'style_image', 'target'):
        assert torch.equal(out[k].cpu(), hb[k]), k
    assert out['filename'] == hb['filename'] and out['user'] == hb['user'] and torch.equal(out['target_original'], hb['target_original'])
    assert 'label_raw' not in out and materialize(out, opt, 'cuda:0') is out            # idempotent


def _filled_trainer(graphs):
    from seg2eye_amd import synthetic as syn
    from seg2eye_amd.options import default_opt
    from seg2eye_amd.pix2pix_trainer import Pix2PixTrainer
    opt = default_opt(ngf=8, ndf=8, crop_size=256, aspect_ratio=1.0, batchSize=2, compute_dtype='fp32', gpu_ids=[0],
                      hip_graphs=graphs, device_preprocess=True)
    tr = Pix2PixTrainer(opt)
    m = tr.pix2pix_model
    with torch.no_grad():
        for net in (m.netG, m.netD, m.netE):
            sd = net.state_dict()
            filled = syn.fill_state_dict([(k, tuple(v.shape)) for k, v in sd.items()])
            for k, v in sd.items():
                v.copy_(torch.from_numpy(filled[k]))
    return tr


@pytest.mark.parametrize('graphs', [True, False], ids=['graphs', 'eager'])
def test_one_step_from_a_raw_batch(store, graphs):
    hb, rb, _ = _twin_batches(256, 1.0, store)
    losses = []
    for batch in (hb, rb):
        tr = _filled_trainer(graphs)
        tr.run_generator_one_step(dict(batch))
        tr.run_discriminator_one_step(dict(batch))
        torch.cuda.synchronize()
        assert bool(tr.opt.hip_graphs) == graphs                 # (a failed capture would have turned them off)
        losses.append({k: float(v.detach().float().mean()) for k, v in tr.get_latest_losses().items()})
    ref, got = losses
    assert set(ref) == set(got) and len(ref) >= 3
    for k, r in ref.items():
        print('%s: host batch %.6f, raw batch %.6f' % (k, r, got[k]))
        assert np.isfinite(r) and np.isfinite(got[k])
        assert abs(got[k] - r) <= 2e-3 * max(1.0, abs(r)), (k, got[k], r)


def test_one_epoch_training_run_with_device_preprocess(tmp_path, monkeypatch, capsys):
    import train as train_mod
    import seg2eye_amd.data as data_mod
    small = fake_openeds_store(seed=6, users=('U001', 'U002'), n_ss=(2, 2), n_gen=4)
    orig = data_mod.create_dataloader
    patched = lambda o, *a, **k: orig(o, *a, store=small, **k)           # noqa: E731
    monkeypatch.setattr(data_mod, 'create_dataloader', patched)
    monkeypatch.setattr(train_mod, 'create_dataloader', patched)
    tr = train_mod.main(['--name', 'dp', '--checkpoints_dir', str(tmp_path), '--dataset_mode', 'openeds', '--device_preprocess',
                         '--ngf', '8', '--ndf', '8', '--batchSize', '2', '--crop_size', '256', '--aspect_ratio', '1.0',
                         '--compute_dtype', 'fp32', '--niter', '1', '--niter_decay', '0', '--print_freq', '2', '--display_freq', '4',
                         '--validation_limit', '2'])
    text = capsys.readouterr().out
    assert 'Training was successfully finished.' in text
    assert text.count('Validation Results') == 2                        # the quick pass on the train and validation splits
    assert 'Error calculated on 2 / 4 samples' in text
    assert (tmp_path / 'dp' / 'latest_net_G.pth').exists()
    assert all(torch.isfinite(v.float()).all() for v in tr.get_latest_losses().values())
