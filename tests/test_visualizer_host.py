"""The visualiser without a GPU: properties of the CPU restatement of the panel rule (tests/_sidebyside_rule.py, the
yardstick of test_visualizer_gpu.py), the entry point's argument errors, the PNG writer, loss_log.txt, the --visuals flag."""
import ctypes
import inspect
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import _sidebyside_rule as R


def _batch(n=2, H=6, W=4, ns=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    return dict(label=torch.randint(0, 4, (n, 1, H, W), generator=g, dtype=torch.uint8),
                fake=torch.rand(n, 1, H, W, generator=g) * 2 - 1,
                target_original=torch.randint(0, 256, (n, 1, 2 * H, 2 * W), generator=g, dtype=torch.uint8),
                style_image=torch.rand(n, ns, 1, H, W, generator=g) * 2 - 1)


# ------------------------------------------------------------------------------------------------ the rule helper
@pytest.mark.parametrize('ns', [1, 2, 3, 4, 5])
def test_style_grid_layout(ns):
    b = _batch(ns=ns)
    s, H, W = b['style_image'], 6, 4
    grid = R.style_grid(s)
    rows, cols = (1, 1) if ns == 1 else (1, 2) if ns == 2 else (2, 2)
    assert grid.shape == (2, 1, rows * H, cols * W) and grid.dtype == torch.float32
    for cell in range(rows * cols):
        got = grid[:, 0, (cell // cols) * H:(cell // cols + 1) * H, (cell % cols) * W:(cell % cols + 1) * W]
        if cell < min(ns, 4):
            a = s[:, cell, 0]
            assert torch.equal(got, ((a + a) + a) / 3)                   # the fp32 channel mean, which is not `a` (below)
        else:
            assert torch.equal(got, torch.zeros_like(got))               # a missing fourth cell is 0 ...
    if ns == 3:                                                          # ... which becomes byte 128 (cells at the grid's own size)
        panel = R.panels_u8(b['label'], b['fake'], b['target_original'], s, w=2 * W, h=2 * H)
        assert torch.equal(panel[:, 0, H:, W:2 * W], torch.full((2, H, W), 128, dtype=torch.uint8))
    if ns == 5:                                                          # a fifth image changes nothing
        assert torch.equal(grid, R.style_grid(s[:, :4]))


def test_channel_mean_is_fp32_arithmetic_and_not_the_identity():
    a = torch.rand(1000000, generator=torch.Generator().manual_seed(1)) * 2 - 1
    mean = torch.mean(torch.stack([a, a, a], 1), 1)
    assert torch.equal(mean, ((a + a) + a) / 3)
    assert 0.10 < float((mean != a).float().mean()) < 0.25


def test_label_batch_of_two_classes_passes_through_unnormalised():
    b = _batch()
    two = b['label'] % 2
    c = R.cells(two, b['fake'], b['target_original'], b['style_image'], w=9, h=13)[..., 9:18]
    assert torch.equal(c, R.O.resize_bilinear(two, 9, 13)) and float(c.max()) == 1.0 and float(c.min()) == 0.0
    c4 = R.cells(b['label'], b['fake'], b['target_original'], b['style_image'], w=9, h=13)[..., 9:18]
    r4 = R.O.resize_bilinear(b['label'], 9, 13)
    assert torch.equal(c4, r4 / r4.max() * 2 - 1) and float(c4.min()) == -1.0


def test_zero_error_gives_an_all_zero_heat_cell():
    b = _batch()
    tgt = (b['label'] % 2)                                                # same size as fake, maximum 1: normalize leaves it alone
    panel = R.panels_u8(b['label'], tgt.float(), tgt, b['style_image'], w=9, h=13)
    assert torch.equal(panel[..., 36:45], torch.zeros_like(panel[..., 36:45]))
    assert torch.equal(panel[..., 18:27], panel[..., 27:36])


def test_bytes_truncate_and_saturate():
    v = torch.tensor([-1.0, -0.999, 0.0, 0.99, 1.0 - 2.0 ** -52, 1.0], dtype=torch.float64)
    assert R.to_bytes(v).tolist() == [0, 0, 128, 254, 255, 255]


def test_range_errors_name_the_tensor():
    b = _batch()
    bad = b['fake'].clone()
    bad[0, 0, 2:4, 1:3] = 1.5
    with pytest.raises(ValueError, match='fake'):
        R.cells(b['label'], bad, b['target_original'], b['style_image'])
    bad = b['fake'].clone()
    bad[1, 0, 0, 0] = float('nan')
    with pytest.raises(ValueError, match='fake'):
        R.cells(b['label'], bad, b['target_original'], b['style_image'])


# ------------------------------------------------------------------------------------------------ the entry point, without a GPU
def test_entry_point_reports_every_bad_argument():
    from seg2eye_amd import _lib
    L = _lib.lib()
    assert L.s2e_sidebyside_ws_bytes(8, 320, 200) > 0 and L.s2e_sidebyside_ws_bytes(8, 320, 200) % 8 == 0
    for bad in ((0, 320, 200), (8, 0, 200), (8, 320, -1)):
        assert L.s2e_sidebyside_ws_bytes(*bad) == -1 and b's2e_sidebyside_ws_bytes' in L.s2e_last_error()
    buf = ctypes.create_string_buffer(64)                                # never dereferenced: every call below fails its checks
    p = ctypes.addressof(buf) // 8 * 8 + 8
    names = ['fake_dtype', 'fake', 'style', 'ns', 'label', 'target_original', 'n', 'H', 'W', 'Ht', 'Wt', 'h', 'w', 'row_stride',
             'panel_stride', 'ws', 'status', 'out', 'stream']
    good = dict(fake_dtype=_lib.S2E_F32, fake=p, style=p, ns=4, label=p, target_original=p, n=2, H=40, W=32, Ht=74, Wt=46, h=21, w=13,
                row_stride=65, panel_stride=65 * 81, ws=p, status=p, out=p, stream=None)
    cases = [(k, None) for k in ('fake', 'style', 'label', 'target_original', 'ws', 'status', 'out')]
    cases += [(k, v) for k in ('n', 'H', 'W', 'Ht', 'Wt', 'h', 'w') for v in (0, -3)]
    cases += [('ns', 0), ('row_stride', 64), ('fake_dtype', 7), ('panel_stride', 65 * 20), ('ws', p + 4), ('status', p + 2)]
    for name, value in cases:
        args = dict(good, **{name: value})
        assert L.s2e_sidebyside_u8(*[args[k] for k in names]) == -1, name                  # S2E_ERR_ARG, before any launch
        msg = L.s2e_last_error()
        assert b's2e_sidebyside_u8' in msg and name.encode() in msg, (name, msg)


def test_op_refuses_cpu_tensors():
    from seg2eye_amd import ops
    from seg2eye_amd._lib import Seg2EyeHipError
    b = _batch()
    with pytest.raises(Seg2EyeHipError, match='GPU only'):
        ops.sidebyside_u8(b['label'], b['fake'], b['target_original'], b['style_image'])


def test_visualize_sidebyside_has_the_reference_signature():
    from seg2eye_amd.visualizer import visualize_sidebyside
    sig = inspect.signature(visualize_sidebyside)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ('data', inspect.Parameter.empty), ('limit', -1), ('key_fake', 'fake'), ('key_content', 'label'), ('key_target', 'target_original'),
        ('key_style', 'style_image'), ('log_key', ''), ('w', 200), ('h', 320), ('error_list', None)]


# ------------------------------------------------------------------------------------------------ PNG, loss log, flag
def _decode_png(data):
    try:
        import io
        from PIL import Image
        return np.asarray(Image.open(io.BytesIO(data)))
    except ImportError:
        assert data[:8] == b'\x89PNG\r\n\x1a\n'
        pos, idat, shape = 8, b'', None
        while pos < len(data):
            n, tag = struct.unpack('>I4s', data[pos:pos + 8])
            body = data[pos + 8:pos + 8 + n]
            assert struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff
            if tag == b'IHDR':
                cols, rows, depth, colour = struct.unpack('>IIBB', body[:10])
                assert (depth, colour) == (8, 0)
                shape = (rows, cols)
            idat += body if tag == b'IDAT' else b''
            pos += 12 + n
        raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(shape[0], shape[1] + 1)
        assert not raw[:, 0].any()                                       # filter type 0 on every row
        return raw[:, 1:]


def test_png_writer_round_trips_a_ragged_array(tmp_path):
    from seg2eye_amd.visualizer import png_bytes, write_png
    img = np.random.RandomState(0).randint(0, 256, (7, 13)).astype(np.uint8)
    got = _decode_png(png_bytes(img))
    assert got.shape == (7, 13) and got.dtype == np.uint8 and np.array_equal(got, img)
    write_png(str(tmp_path / 'a.png'), img[:, ::2])                      # (a non-contiguous view)
    assert np.array_equal(_decode_png((tmp_path / 'a.png').read_bytes()), img[:, ::2]) and os.listdir(tmp_path) == ['a.png']
    with pytest.raises(ValueError):
        png_bytes(img[None])


def test_loss_log_and_png_files(tmp_path, capsys):
    from seg2eye_amd.options import parse
    from seg2eye_amd.visualizer import Visualizer
    opt = parse(['--name', 'run', '--checkpoints_dir', str(tmp_path), '--visuals'])
    assert opt.visuals and not parse([]).visuals and not parse([], is_train=False).visuals
    vis = Visualizer(opt)
    vis.print_current_errors(2, 480, {'GAN': torch.tensor([0.5, 1.5]), 'mse/train/rand/relative': 3.14159}, 0.0421)
    vis.plot_current_errors({'GAN': torch.tensor(1.0)}, 480)
    line = '(epoch: 2, iters: 480, time: 0.042) GAN: 1.000 mse/train/rand/relative: 3.142 '
    assert capsys.readouterr().out == line + '\n'
    Visualizer(opt)                                                      # a resumed run appends a second header
    log = (tmp_path / 'run' / 'loss_log.txt').read_text().split('\n')
    assert len(log) == 4 and log[1] == line and log[3] == ''
    for header in (log[0], log[2]):
        assert header.startswith('================ Training Loss (') and header.endswith(') ================')
    panel = np.arange(380 * 1000, dtype=np.uint32).astype(np.uint8).reshape(1, 380, 1000)
    paths = vis.display_current_results({'train/rand/0': panel, 'train/rand/1': panel[:, ::-1]}, 2, 480)
    assert [os.path.relpath(p, tmp_path / 'run') for p in paths] == [os.path.join('visuals', 'step000000480', 'train_rand_%d.png' % i) for i in (0, 1)]
    assert np.array_equal(_decode_png(open(paths[1], 'rb').read()), panel[0, ::-1])


@pytest.mark.parametrize('mode', ['train', 'test'])
def test_parser_still_matches_the_reference_flag_table(mode):
    from test_cli import test_cli_flags_match_the_reference
    from seg2eye_amd.options import build_parser, default_opt
    test_cli_flags_match_the_reference(mode)
    flags = {a.dest: a for a in build_parser(mode == 'train')._actions}
    assert ('visuals' in flags) == (mode == 'train') and default_opt().visuals is False
    if mode == 'train':
        assert type(flags['visuals']).__name__ == '_StoreTrueAction' and flags['visuals'].default is False
        assert 'tf_log' in flags and 'no_html' in flags               # (accepted, inert)


def test_caption_strip_is_black_and_white():
    from seg2eye_amd.visualizer import caption_strip
    s = caption_strip('U001 / U001000_ss (err: 12.34)', 1000)
    assert s.shape == (60, 1000) and s.dtype == np.uint8 and set(np.unique(s)) <= {0, 255}
