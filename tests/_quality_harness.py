"""What the tests of the image-quality terms (SSIM, MS-SSIM, region error, focal frequency loss; seg2eye_amd/quality.py) share: the
small trainer and its batch, the Tester's error log, and the walk of a raw entry point's table of refused calls."""
import functools
import glob
import os

import numpy as np
import torch

PARENT_LOSS_KEYS = {'GAN', 'GAN_Feat', 'D/Fake', 'D/real'}     # the step's losses with no extension flag set


def opt(**kw):
    """ngf = ndf = 8, batch 2, fp32, at 256 x 256 -- the one size the networks exist at (the encoder's FC head is sized for it)."""
    from seg2eye_amd.options import default_opt
    kw.setdefault('gpu_ids', [0])
    kw.setdefault('compute_dtype', 'fp32')
    return default_opt(ngf=8, ndf=8, crop_size=256, aspect_ratio=1.0, batchSize=2, **kw)


@functools.lru_cache(maxsize=None)
def batch(seed=21):
    from seg2eye_amd import synthetic as syn
    b = syn.make_batch(2, 256, 256, seed=seed)
    return {'label': torch.from_numpy(b['label']), 'style_image': torch.from_numpy(b['style_image']), 'target': torch.from_numpy(b['target'])}


def trainer(**kw):
    """A trainer on the hash-filled weights (the same for every trainer)."""
    from seg2eye_amd import synthetic as syn
    from seg2eye_amd.pix2pix_trainer import Pix2PixTrainer
    tr = Pix2PixTrainer(opt(**kw))
    m = tr.pix2pix_model
    with torch.no_grad():
        for net in (m.netG, m.netD, m.netE):
            sd = net.state_dict()
            filled = syn.fill_state_dict([(k, tuple(v.shape)) for k, v in sd.items()])
            for k, v in sd.items():
                v.copy_(torch.from_numpy(filled[k]))
    return tr


def load_log(tester):
    logs = glob.glob(os.path.join(tester.results_dir, 'error_log_validation.*'))
    assert len(logs) == 1, logs
    if logs[0].endswith('.npz'):
        return dict(np.load(logs[0]))
    import h5py
    with h5py.File(logs[0], 'r') as f:
        return {k: np.asarray(v) for k, v in f.items()}


def recording_tester(argv, flags):
    """-> (a validation Tester of `argv + flags`, seen, labels): every run_batch appends its uint8 (produced, target) pair to `seen` and
    its batch's label map to `labels`, on the CPU."""
    from seg2eye_amd.options import parse
    from seg2eye_amd.tester import Tester
    tester = Tester(parse(list(argv) + list(flags), is_train=False), dataset_key='validation')
    seen, labels, run_batch = [], [], tester.run_batch

    def recording(data_i, model):
        out = run_batch(data_i, model)
        assert len(out) == 4
        seen.append((out[2].cpu(), out[3].cpu()))
        labels.append(torch.as_tensor(data_i['label']).cpu())
        return out
    tester.run_batch = recording
    return tester, seen, labels


def check_error_table(name, table):
    """Call the raw entry point `name` with each row's arguments (dummy pointers: the caller makes sure no GPU is visible) and compare
    (return code, s2e_last_error()) with the row's (code, message); every mismatch is reported, not only the first."""
    from seg2eye_amd import _lib
    L = _lib.lib()
    wrong = []
    for args, code, text in table:
        rc = getattr(L, name)(*args)
        got = (rc, L.s2e_last_error().decode() if rc else '')
        if got != (code, text):
            wrong.append((args, got, (code, text)))
    assert not wrong, wrong
