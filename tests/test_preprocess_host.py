"""--device_preprocess without a GPU: the numpy restatement of Pillow's 8-bit bicubic resize against the committed
Pillow outputs (tests/golden/pil_bicubic.npz) and against live Pillow; the raw-frame mode of OpenEDSDataset against its host-mode
twin; the entry points' argument checks; the flag's parse-time errors."""
import numpy as np
import pytest
import torch

from conftest import load_golden

# (H, W) -> (Ho, Wo); the inputs and row steps of tests/golden/make_pil_bicubic.py (a copy: the generator needs Pillow, the tests do not)
CASES = [((640, 400), (80, 64)), ((640, 400), (320, 256)), ((640, 400), (256, 256)), ((640, 400), (640, 384)),
         ((640, 400), (640, 400)), ((37, 23), (64, 48))]
KINDS = ('uniform', 'binary')
ROW_STEP = {'uniform': {(320, 256): 2, (640, 384): 8, (640, 400): 32},
            'binary': {(320, 256): 4, (256, 256): 4, (640, 384): 16, (640, 400): 32}}
CASE_IDS = ['%dx%d_to_%dx%d' % (s + d) for s, d in CASES]


def case_name(src, dst, kind):
    return '%dx%d_to_%dx%d_%s' % (src + dst + (kind,))


def case_input(ci, src, kind):
    rng = np.random.RandomState(1000 + 10 * ci + KINDS.index(kind))
    frames = rng.randint(0, 256, (3,) + src) if kind == 'uniform' else rng.randint(0, 2, (3,) + src) * 255
    return frames.astype(np.uint8)


def fake_openeds_store(seed=0, users=('U001', 'U002', 'U003'), n_ss=(3, 2, 4), n_gen=5):
    """An in-memory stand-in for the OpenEDS H5 file, built the way tests/test_cli.py builds its own."""
    rng = np.random.RandomState(seed)
    store = {}
    for key in ('train', 'validation', 'test'):
        store[key] = {}
        for u, n in zip(users, n_ss):
            store[key][u] = {'images_ss': rng.randint(0, 256, (n, 640, 400)).astype(np.uint8),
                             'labels_ss': rng.randint(0, 4, (n, 640, 400)).astype(np.uint8),
                             'images_gen': rng.randint(0, 256, (n_gen, 640, 400)).astype(np.uint8),
                             'images_seq': rng.randint(0, 256, (2, 640, 400)).astype(np.uint8),
                             'labels_gen': rng.randint(0, 4, (n, 640, 400)).astype(np.uint8),
                             'images_ss_filenames': np.array([('%s.%03d_ss' % (u, i)).encode() for i in range(n)], dtype='S13'),
                             'labels_gen_filenames': np.array([('%s_%03d_gen' % (u, i)).encode() for i in range(n)], dtype='S13')}
    return store


@pytest.mark.parametrize('ci', range(len(CASES)), ids=CASE_IDS)
@pytest.mark.parametrize('kind', KINDS)
def test_reference_equals_the_pillow_fixture(ci, kind):
    from seg2eye_amd.ops.preprocess import resize_bicubic_u8_reference
    src, dst = CASES[ci]
    z = load_golden('pil_bicubic')
    img = case_input(ci, src, kind)[0]
    got = resize_bicubic_u8_reference(img, dst[1], dst[0])
    want = z[case_name(src, dst, kind)]
    assert got.shape == dst and got.dtype == np.uint8
    assert int((got[::ROW_STEP[kind].get(dst, 1)] != want).sum()) == 0, 'Pillow %s' % z['pillow_version']
    if dst == src:
        assert np.array_equal(got, img)                          # both passes skipped


@pytest.mark.parametrize('ci', range(len(CASES)), ids=CASE_IDS)
def test_reference_equals_live_pillow(ci):
    Image = pytest.importorskip('PIL.Image')
    from seg2eye_amd.ops.preprocess import resize_bicubic_u8_reference
    src, dst = CASES[ci]
    for kind in KINDS:
        for img in case_input(ci, src, kind)[:2]:
            want = np.asarray(Image.fromarray(img, mode='L').resize((dst[1], dst[0]), Image.BICUBIC), dtype=np.uint8)
            assert int((resize_bicubic_u8_reference(img, dst[1], dst[0]) != want).sum()) == 0, (dst, kind)


def test_coefficient_tables():
    from seg2eye_amd.ops.preprocess import bicubic_coeffs, bicubic_ksize, nearest_index
    kk, bounds = bicubic_coeffs(640, 80)
    assert kk.shape == (80, 33) and kk.dtype == np.int32 and bounds.shape == (80, 2) and bounds.dtype == np.int32
    assert bicubic_ksize(400, 64) == 27 and bicubic_ksize(23, 48) == 5 and bicubic_ksize(400, 384) == 7
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= 640).all() and (bounds[:, 1] <= 33).all()
    assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(bounds.sum(1)) >= 0).all()     # bands read one contiguous row range
    assert (np.abs(kk.sum(1) - (1 << 22)) <= 33).all()                                     # normalised taps, rounded one by one
    up, ub = bicubic_coeffs(23, 48)
    assert ub[0, 0] == 0 and ub[-1].sum() == 23 and ub[0, 1] < 5 and ub[-1, 1] < 5          # windows clipped at both borders
    assert np.array_equal(nearest_index(640, 80), np.arange(80) * 8)
    assert nearest_index(23, 48).max() == 22


def _twins(argv_extra, seed, store):
    from seg2eye_amd.openeds_dataset import OpenEDSDataset
    from seg2eye_amd.options import parse
    argv = ['--dataset_mode', 'openeds', '--dataset_key', 'train', '--crop_size', '64', '--aspect_ratio', '0.8',
            '--style_sample_method', 'random'] + argv_extra
    host = OpenEDSDataset(parse(argv), store=store, rng=np.random.RandomState(seed))
    raw = OpenEDSDataset(parse(argv + ['--device_preprocess']), store=store, rng=np.random.RandomState(seed))
    return host, raw


def test_raw_dataset_is_the_host_dataset_before_its_transform():
    """Same seeded rng -> same sample: filename, user, flip, style frames; the numpy restatement + the lookup table applied to the
    raw frames reproduce the host-mode tensors exactly."""
    from seg2eye_amd.openeds_dataset import resize_nearest
    from seg2eye_amd.ops.preprocess import normalize_lut, resize_bicubic_u8_reference
    store = fake_openeds_store()
    host, raw = _twins([], 5, store)
    lut = normalize_lut()
    flips = []
    for idx in (0, 4, 8, 2):
        h, r = host[idx], raw[idx]
        assert set(r) == {'label_raw', 'style_raw', 'target_raw', 'flip', 'filename', 'user', 'target_original'}
        assert r['filename'] == h['filename'] and r['user'] == h['user']
        assert r['label_raw'].shape == (640, 400) and r['label_raw'].dtype == torch.uint8
        assert r['style_raw'].shape == (4, 640, 400) and r['style_raw'].dtype == torch.uint8
        assert r['target_raw'].shape == (640, 400) and r['target_raw'].dtype == torch.uint8 and isinstance(r['flip'], bool)
        assert torch.equal(r['target_original'], h['target_original'])
        flips.append(r['flip'])

        def tf(frame):
            u8 = torch.from_numpy(resize_bicubic_u8_reference(frame.numpy(), 64, 80))
            u8 = u8.flip(-1) if r['flip'] else u8
            return lut[u8.long()].unsqueeze(0)
        assert torch.equal(tf(r['target_raw']), h['target'])
        assert torch.equal(torch.stack([tf(f) for f in r['style_raw']]), h['style_image'])
        lab = torch.from_numpy(resize_nearest(r['label_raw'].numpy(), 64, 80))
        assert torch.equal(lab.flip(-1) if r['flip'] else lab, h['label'])
    assert True in flips and False in flips
    # the two generators are in the same state afterwards: the same draws were made
    assert host.rng.randint(1 << 30) == raw.rng.randint(1 << 30)


def test_raw_dataset_test_split_and_loader():
    from seg2eye_amd.data import create_dataloader
    from seg2eye_amd.openeds_dataset import OpenEDSDataset
    from seg2eye_amd.options import parse
    store = fake_openeds_store()
    ot = parse(['--dataset_mode', 'openeds', '--dataset_key', 'test', '--crop_size', '64', '--aspect_ratio', '0.8', '--device_preprocess'],
               is_train=False)
    ds = OpenEDSDataset(ot, store=store)
    t = ds[0]
    assert 'target_raw' not in t and 'target_original' not in t and t['flip'] is False and t['filename'] == 'U001_000_gen'
    assert torch.equal(t['label_raw'], torch.from_numpy(store['test']['U001']['labels_gen'][0]))
    p = ds.get_particular(1)
    assert p['label_raw'].shape == (1, 640, 400) and p['style_raw'].shape == (1, 4, 640, 400) and p['flip'].tolist() == [False]
    o = parse(['--dataset_mode', 'openeds', '--dataset_key', 'validation', '--crop_size', '64', '--aspect_ratio', '0.8', '--batchSize', '2',
               '--serial_batches', '--device_preprocess'])
    dl = create_dataloader(o, store=store)
    assert dl.pin_memory and not create_dataloader(parse(['--dataset_mode', 'openeds', '--dataset_key', 'validation']), store=store).pin_memory
    b = next(iter(dl))
    assert b['label_raw'].shape == (2, 640, 400) and b['style_raw'].shape == (2, 4, 640, 400) and b['target_raw'].shape == (2, 640, 400)
    assert b['flip'].shape == (2,) and b['flip'].dtype == torch.bool and b['target_original'].shape == (2, 1, 640, 400)


def test_materialize_leaves_standard_batches_alone_and_has_no_cpu_path():
    from seg2eye_amd._lib import Seg2EyeHipError
    from seg2eye_amd.ops import materialize, resize_bicubic_u8, resize_nearest_u8
    from seg2eye_amd.options import parse
    o = parse(['--dataset_mode', 'openeds', '--crop_size', '64', '--device_preprocess'])
    std = {'label': torch.zeros(1, 80, 64, dtype=torch.uint8), 'style_image': torch.zeros(1, 4, 1, 80, 64), 'target': torch.zeros(1, 1, 80, 64)}
    assert materialize(std, o, 'cpu') is std
    raw = {'label_raw': torch.zeros(1, 640, 400, dtype=torch.uint8), 'style_raw': torch.zeros(1, 4, 640, 400, dtype=torch.uint8),
           'flip': torch.tensor([False])}
    with pytest.raises(Seg2EyeHipError):
        materialize(raw, o, 'cpu')
    with pytest.raises(Seg2EyeHipError):
        resize_bicubic_u8(raw['label_raw'], 80, 64, raw['flip'])
    with pytest.raises(Seg2EyeHipError):
        resize_nearest_u8(raw['label_raw'], 80, 64, raw['flip'])


def test_entry_points_reject_null_pointers_before_any_launch():
    from seg2eye_amd import _lib as L
    lib = L.lib()
    one = 16                                                 # any non-NULL value: the checks come before any dereference
    assert lib.s2e_resize_bicubic_u8(None, one, 1, 8, 8, 4, 4, one, one, one, one, one, one, None, None) == -1
    assert b's2e_resize_bicubic_u8' in lib.s2e_last_error()
    assert lib.s2e_resize_bicubic_u8(one, None, 1, 8, 8, 4, 4, one, one, one, one, one, one, None, None) == -1
    assert lib.s2e_resize_bicubic_u8(one, one, 1, 8, 8, 4, 4, one, one, one, one, None, one, None, None) == -1       # no table
    assert lib.s2e_resize_bicubic_u8(one, one, 1, 8, 8, 4, 4, one, one, one, one, one, None, None, None) == -1       # no output
    assert lib.s2e_resize_bicubic_u8(one, one, 0, 8, 8, 4, 4, one, one, one, one, one, one, None, None) == -1        # no frames
    assert lib.s2e_resize_bicubic_u8(one, one, 1, 8, 8, 4, 4, None, one, one, one, one, one, None, None) == -1       # W changes: taps needed
    assert lib.s2e_resize_bicubic_u8(one, one, 1, 8, 8, 4, 8, None, None, one, None, one, one, None, None) == -1     # H changes: bounds needed
    # one output row needs 2 * ceil(2 * 40000 / 16) + 1 source rows of 400 + 256 bytes: far beyond 64 KiB of LDS
    assert lib.s2e_resize_bicubic_u8(one, one, 1, 40000, 400, 16, 256, one, one, one, one, one, one, None, None) == -3
    assert b'LDS' in lib.s2e_last_error()
    assert lib.s2e_resize_nearest_u8(None, one, 1, 8, 8, 4, 4, one, one, one, None) == -1
    assert b's2e_resize_nearest_u8' in lib.s2e_last_error()
    for hole in range(4):
        ptrs = [one, one, one, one]
        ptrs[hole] = None
        assert lib.s2e_resize_nearest_u8(one, ptrs[0], 1, 8, 8, 4, 4, ptrs[1], ptrs[2], ptrs[3], None) == -1
    assert lib.s2e_resize_nearest_u8(one, one, 1, 8, 0, 4, 4, one, one, one, None) == -1


def test_flag_is_rejected_where_it_cannot_apply():
    from seg2eye_amd.options import parse
    with pytest.raises(ValueError, match='--device_preprocess'):
        parse(['--device_preprocess'])                                                    # dataset_mode synthetic (the default)
    with pytest.raises(ValueError, match='--device_preprocess'):
        parse(['--device_preprocess', '--dataset_mode', 'synthetic'], is_train=False)
    with pytest.raises(ValueError, match='--device_preprocess'):
        parse(['--device_preprocess', '--dataset_mode', 'openeds', '--preprocess_mode', 'resize_and_crop'])
    assert parse(['--device_preprocess', '--dataset_mode', 'openeds']).device_preprocess is True
    assert parse(['--dataset_mode', 'openeds']).device_preprocess is False and parse([]).device_preprocess is False
