"""Network-level parity of the HIP path (through define_G/define_D/define_E, Pix2PixModel and
Pix2PixTrainer) against (a) the golden vectors produced by the REAL reference and (b) the CPU oracle
on the same seeded inputs.

Tolerances: the north-star bar for the fp32 generator is max-abs-diff < 1e-3 on trained-scale weights
(output std ~0.5); gradients and parameters are compared through the fixtures' checksums with a
relative bound; bf16 runs are compared against the fp32 result with a bound that reflects bf16's
8 significant bits through ~40 layers."""
import numpy as np
import pytest
import torch

from conftest import load_golden, filled_state, manifest_of, assert_checksum_close

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
G_TOL = 1e-3        # north_star: generator output max-abs-diff vs the CPU reference path, fp32
KINK_TOL = 2e-2     # whole-network gradients (see test_generator_fp32_matches_reference)


def _opt(**kw):
    from seg2eye_amd.options import default_opt
    kw.setdefault('gpu_ids', [0])
    return default_opt(**kw)


def _load(net, z, prefix):
    sd = filled_state(z, prefix)
    net.load_state_dict(sd)
    return net


def _label(z):
    return torch.from_numpy(z['label']).to(DEV)       # (N,1,H,W) uint8


@pytest.mark.parametrize('tag,ngf,crop,ar', [('g_ngf8_64', 8, 64, 1.0), ('g_ngf16_128x64', 16, 64, 0.5)])
def test_generator_fp32_matches_reference(tag, ngf, crop, ar):
    from seg2eye_amd import networks
    z = load_golden(tag)
    opt = _opt(ngf=ngf, crop_size=crop, aspect_ratio=ar, compute_dtype='fp32')
    G = _load(networks.define_G(opt), z, 'G')
    w = torch.from_numpy(z['w']).to(DEV)
    G.eval()
    with torch.no_grad():
        y = G(_label(z), w)
    assert y.shape == z['y_eval'].shape
    err = float((y.float().cpu() - torch.from_numpy(z['y_eval'])).abs().max())
    assert err < G_TOL, 'eval-mode G output differs from the reference by %.3e' % err
    # also accepts the one-hot float tensor of the reference call site
    onehot = torch.zeros(z['label'].shape[0], 4, *z['label'].shape[2:], device=DEV).scatter_(1, _label(z).long(), 1.0)
    with torch.no_grad():
        y2 = G(onehot, w)
    assert float((y - y2).abs().max()) < 1e-5          # sigma is reduced with float atomics: not bit-reproducible
    # backward (eval mode): every parameter gradient vs the reference's checksums
    G.zero_grad()
    wt = w.clone().requires_grad_(True)
    yg = G(_label(z), wt)
    from seg2eye_amd import synthetic as syn
    proj = torch.from_numpy(syn.hash_uniform('g_proj', tuple(yg.shape), seed=7)).to(DEV)
    (yg.float() * proj).sum().backward()
    # Whole-network gradients are compared with a kink-tolerant bound: a LeakyReLU pre-activation that
    # sits within fp32 rounding of 0 may fall on either side in two fp32 implementations, and one
    # flipped mask element moves every upstream gradient by a few 1e-3 (measured: exactly one such
    # element in this fixture; all other intermediate gradients agree to 1e-6).  The tight gradient
    # checks live in test_resblk_matches_oracle_tight / test_modules_fp32_match_reference.
    gw = z['grad_w']
    assert float((wt.grad.cpu() - torch.from_numpy(gw)).abs().max()) < KINK_TOL * np.abs(gw).max()
    for k, p in G.named_parameters():
        assert_checksum_close(p.grad, z['grad_' + k], KINK_TOL, k)
    # one train-mode forward from the pinned u, v: output and post-forward buffers
    G.train()
    with torch.no_grad():
        yt = G(_label(z), w)
    err = float((yt.float().cpu() - torch.from_numpy(z['y_train'])).abs().max())
    assert err < G_TOL, 'train-mode G output differs by %.3e' % err
    sd = G.state_dict()
    for k in [k[3:] for k in z.files if k.startswith('uv_')]:
        np.testing.assert_allclose(sd[k].cpu().numpy(), z['uv_' + k], atol=2e-5, rtol=0)


@pytest.mark.parametrize('dt', ['fp32', 'bf16'])
def test_pack_plan_matches_individual_packs(dt):
    """The first forward/backward of a network packs every weight on its own and teaches the PackPlan;
    later ones take all packs from ONE batched launch.  Same bits either way (eval mode: sigma fixed)."""
    from seg2eye_amd import networks
    z = load_golden('g_ngf16_128x64')
    opt = _opt(ngf=16, crop_size=64, aspect_ratio=0.5, compute_dtype=dt)
    G = _load(networks.define_G(opt), z, 'G').eval()
    w = torch.from_numpy(z['w']).to(DEV)
    runs = []
    for it in range(3):
        G.zero_grad()
        wt = w.clone().requires_grad_(True)
        y = G(_label(z), wt)
        y.float().square().sum().backward()
        runs.append((y.detach().float().clone(), wt.grad.clone(), [p.grad.clone() for p in G.parameters()]))
        plan = G.__dict__['_pack_plan']
        if it == 0:
            assert plan.hits == 0 and len(plan.jobs) > 30          # learned fwd + transposed packs
        if it == 1:
            h1 = plan.hits
            assert h1 >= len(plan.jobs) - 2, (h1, len(plan.jobs))
    assert plan.hits >= 2 * h1
    # the batched launch produced exactly the matrices the individual packs produce (same sigma array)
    from seg2eye_amd import ops
    sigma = G.__dict__['_sn_owned_bank'].sigma
    for j in plan.jobs.values():
        sg = None if j['sigma_index'] < 0 else sigma[j['sigma_index']:j['sigma_index'] + 1]
        ref = ops.pack_weight(j['w'], j['dtype'], j['cin_pad'], j['transposed'], sg)
        assert torch.equal(ref.view(torch.uint8), j['out'].view(torch.uint8)), (tuple(j['w'].shape), j['transposed'])
    # The FORWARD is bit-reproducible since round 2 (spectral norm accumulates with integer atomics, the statistics kernels add
    # per-block partials in a fixed order; round 1: two bf16 forwards differed by ~0.05 through sigma's float-atomic noise).
    # Weight gradients still combine pixel slices with fp32 atomics: equal up to summation order.
    gtol = KINK_TOL                                                # one flipped LeakyReLU mask moves a whole sample's gradient
    for k in (1, 2):
        assert torch.equal(runs[k][0], runs[0][0]), float((runs[k][0] - runs[0][0]).abs().max())
        gt = gtol if dt == 'fp32' else 5 * gtol
        assert float((runs[k][1] - runs[0][1]).abs().max()) <= gt * max(1.0, float(runs[0][1].abs().max()))
        for a, b in zip(runs[k][2], runs[0][2]):
            assert float((a - b).abs().max()) <= gt * max(1.0, float(b.abs().max()))
    tol = 0.0
    with torch.no_grad():                                          # forward-only: transposed packs skipped, still correct
        y3 = G(_label(z), w).float()
    assert float((y3 - runs[0][0]).abs().max()) <= tol


def test_generator_batchnorm_spade_fp32_matches_reference():
    """G3: --norm_G spectralspadebatch3x3 (the reference's default): train-mode forward on batch statistics, parameter
    gradients, the BatchNorm running buffers after the forward, then eval mode on those buffers -- vs the REAL reference."""
    from seg2eye_amd import networks, synthetic as syn
    z = load_golden('g_bn_ngf8_64')
    opt = _opt(ngf=8, crop_size=64, aspect_ratio=1.0, compute_dtype='fp32', norm_G='spectralspadebatch3x3')
    G = _load(networks.define_G(opt), z, 'G')
    assert len(G.state_dict()) == 270
    w = torch.from_numpy(z['w']).to(DEV)
    G.train()
    wt = w.clone().requires_grad_(True)
    y = G(_label(z), wt)
    err = float((y.detach().float().cpu() - torch.from_numpy(z['y_train'])).abs().max())
    assert err < G_TOL, 'train-mode BN-SPADE output differs from the reference by %.3e' % err
    proj = torch.from_numpy(syn.hash_uniform('g_proj', tuple(y.shape), seed=9)).to(DEV)
    (y.float() * proj).sum().backward()
    gw = z['grad_w']
    assert float((wt.grad.cpu() - torch.from_numpy(gw)).abs().max()) < KINK_TOL * np.abs(gw).max()
    for k, p in G.named_parameters():
        assert_checksum_close(p.grad, z['grad_' + k], KINK_TOL, k)
    sd = G.state_dict()
    for k in [k[4:] for k in z.files if k.startswith('buf_')]:
        np.testing.assert_allclose(sd[k].cpu().numpy(), z['buf_' + k], atol=2e-5, rtol=0, err_msg=k)
    G.eval()
    with torch.no_grad():
        ye = G(_label(z), w)
    err = float((ye.float().cpu() - torch.from_numpy(z['y_eval_after'])).abs().max())
    assert err < G_TOL, 'eval-mode BN-SPADE output differs by %.3e' % err
    # bf16 train step with the BatchNorm variant stays finite through Pix2PixTrainer (graphs on)
    from seg2eye_amd.pix2pix_trainer import Pix2PixTrainer
    tr = Pix2PixTrainer(_opt(ngf=8, ndf=8, crop_size=256, aspect_ratio=1.0, batchSize=2, compute_dtype='bf16',
                             norm_G='spectralspadebatch3x3', hip_graphs=True))
    data = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in _batch(2, 256, 256, 3).items()}
    for _ in range(2):
        tr.run_generator_one_step(dict(data))
        tr.run_discriminator_one_step(dict(data))
    assert all(np.isfinite(float(v)) for v in tr.get_latest_losses().values())


def test_generator_bf16_close_to_fp32():
    from seg2eye_amd import networks
    z = load_golden('g_ngf16_128x64')
    outs = {}
    for dt in ('fp32', 'bf16'):
        opt = _opt(ngf=16, crop_size=64, aspect_ratio=0.5, compute_dtype=dt)
        G = _load(networks.define_G(opt), z, 'G').eval()
        with torch.no_grad():
            outs[dt] = G(_label(z), torch.from_numpy(z['w']).to(DEV)).float().cpu()
    assert outs['bf16'].dtype == torch.float32
    d = (outs['bf16'] - outs['fp32']).abs()
    assert float(d.mean()) < 2e-2 and float(d.max()) < 0.25, (float(d.mean()), float(d.max()))


def test_discriminator_and_losses_fp32():
    from seg2eye_amd import networks, ops
    z = load_golden('d_ndf8_32')
    opt = _opt(ndf=8, crop_size=32, compute_dtype='fp32')
    D = _load(networks.define_D(opt), z, 'D').eval()
    lab = _label(z)[:, 0]
    fake = torch.from_numpy(z['fake']).to(DEV).requires_grad_(True)
    real = torch.from_numpy(z['real']).to(DEV)
    imgs = torch.cat([fake[:, 0], real[:, 0]], 0)
    x = ops.seg_image_concat(torch.cat([lab, lab], 0), imgs)
    pred = D(x)
    for i in range(2):
        for j in range(5):
            ref = z['pred_%d_%d' % (i, j)]
            if ref.ndim == 1 and ref.shape[0] == 18:
                assert_checksum_close(pred[i][j].contiguous(), ref, 1e-4, 'pred%d%d' % (i, j))
            else:
                np.testing.assert_allclose(pred[i][j].detach().cpu().numpy(), ref, atol=2e-4, rtol=0)
    # reference API: the NCHW 5-channel tensor gives the same result
    onehot = torch.zeros(2, 4, 32, 32, device=DEV).scatter_(1, lab.long().unsqueeze(1), 1.0)
    xin = torch.cat([torch.cat([onehot, fake.detach()], 1), torch.cat([onehot, real], 1)], 0)
    pred2 = D(xin)
    assert float((pred2[1][4] - pred[1][4].detach()).abs().max()) < 1e-5
    crit = networks.GANLoss('hinge', opt=opt)
    pf = [[t[:2] for t in p] for p in pred]
    pr = [[t[2:] for t in p] for p in pred]
    l_g = crit(pf, True, for_discriminator=False)
    l_df = crit(pf, False, for_discriminator=True)
    l_dr = crit(pr, True, for_discriminator=True)
    feat = networks.feature_matching_loss(pf, pr, 10.0)
    for got, key in ((l_g, 'l_g'), (l_df, 'l_df'), (l_dr, 'l_dr'), (feat, 'l_feat')):
        assert tuple(got.shape) == (1,)
        np.testing.assert_allclose(got.detach().cpu().numpy(), z[key], atol=2e-5, rtol=2e-5)
    params = dict(D.named_parameters())
    grads = torch.autograd.grad((l_g + feat).sum(), [fake] + list(params.values()), retain_graph=True)
    gf = z['grad_fake']
    assert float((grads[0].cpu() - torch.from_numpy(gf)).abs().max()) < KINK_TOL * np.abs(gf).max()
    for k, g in zip(params, grads[1:]):
        assert_checksum_close(g, z['gradG_' + k], KINK_TOL, k)
    grads = torch.autograd.grad((l_df + l_dr).sum(), list(params.values()))
    for k, g in zip(params, grads):
        assert_checksum_close(g, z['gradD_' + k], KINK_TOL, k)


@pytest.mark.parametrize('dt', ['fp32', 'bf16'])
def test_fused_feature_matching_matches_unfused(dt):
    """netD(x, feat_lambda=...) (the G step's path: feature-matching terms and their gradients produced inside
    D's forward/backward by ops.feat_tap) == features + networks.feature_matching_loss afterwards."""
    from seg2eye_amd import networks, ops
    z = load_golden('d_ndf8_32')
    opt = _opt(ndf=8, crop_size=32, compute_dtype=dt)
    D = _load(networks.define_D(opt), z, 'D').eval()
    for p in D.parameters():
        p.requires_grad_(False)
    lab = _label(z)[:, 0]
    real = torch.from_numpy(z['real']).to(DEV)
    crit = networks.GANLoss('hinge', opt=opt)
    res = []
    for fused in (False, True):
        fake = torch.from_numpy(z['fake']).to(DEV).requires_grad_(True)
        x = ops.seg_image_concat(torch.cat([lab, lab], 0), torch.cat([fake[:, 0], real[:, 0]], 0).to(D.cdtype))
        if fused:
            pred, feat = D(x, feat_lambda=10.0)
        else:
            pred = D(x)
        pf = [[t[:2] for t in p] for p in pred]
        pr = [[t[2:] for t in p] for p in pred]
        if not fused:
            feat = networks.feature_matching_loss(pf, pr, 10.0)
        l_g = crit(pf, True, for_discriminator=False)
        g, = torch.autograd.grad((l_g + feat).sum(), [fake])
        res.append((float(feat), float(l_g), g.float().cpu()))
    tol = 1e-5 if dt == 'fp32' else 2e-2
    assert abs(res[0][0] - res[1][0]) <= tol * abs(res[0][0]) and abs(res[0][1] - res[1][1]) <= tol * max(1.0, abs(res[0][1]))
    assert float((res[0][2] - res[1][2]).abs().max()) <= (1e-5 if dt == 'fp32' else 5e-2) * float(res[0][2].abs().max())
    if dt == 'fp32':
        np.testing.assert_allclose(res[1][0], float(z['l_feat']), rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize('mode', ['ls', 'original', 'w'])
def test_non_hinge_gan_modes(mode):
    """--gan_mode ls / original / w (loss.py:58-65, 78-83): the reference's formulas on the multiscale prediction lists,
    and a trainer iteration with each."""
    from seg2eye_amd import networks
    import torch.nn.functional as F
    opt = _opt(ndf=8, crop_size=32, compute_dtype='fp32', gan_mode=mode)
    crit = networks.GANLoss(mode, opt=opt)
    g = torch.Generator().manual_seed(5)
    preds = [[torch.randn(2, 1, 7, 7, generator=g).to(DEV)], [torch.randn(2, 1, 4, 4, generator=g).to(DEV)]]
    for real in (True, False):
        want = 0
        for (p,) in preds:
            t = torch.full_like(p, 1.0 if real else 0.0)
            want = want + {'ls': F.mse_loss(p, t), 'original': F.binary_cross_entropy_with_logits(p, t),
                           'w': (-p.mean() if real else p.mean())}[mode]
        got = crit(preds, real, for_discriminator=True)
        assert abs(float(got) - float(want / 2)) < 1e-6
    from seg2eye_amd.pix2pix_trainer import Pix2PixTrainer
    tr = Pix2PixTrainer(_opt(ngf=8, ndf=8, crop_size=256, aspect_ratio=1.0, batchSize=2, compute_dtype='bf16', gan_mode=mode))
    data = _batch(2, 256, 256, 4)
    tr.run_generator_one_step(dict(data))
    tr.run_discriminator_one_step(dict(data))
    assert all(np.isfinite(float(v)) for v in tr.get_latest_losses().values())


def test_encoder_fp32():
    from seg2eye_amd import networks
    z = load_golden('e_ngf8')
    opt = _opt(ngf=8, crop_size=256, compute_dtype='fp32')
    E = _load(networks.define_E(opt), z, 'E').eval()
    with torch.no_grad():
        mu, logvar, feats = E(torch.from_numpy(z['x']).to(DEV))
    np.testing.assert_allclose(mu.cpu().numpy(), z['mu'], atol=3e-4, rtol=0)
    np.testing.assert_allclose(logvar.cpu().numpy(), z['logvar'], atol=3e-4, rtol=0)
    np.testing.assert_allclose(feats[-1].float().cpu().numpy(), z['feat_last'], atol=3e-4, rtol=0)


def _batch(n, h, w, seed):
    from seg2eye_amd import synthetic as syn
    b = syn.make_batch(n, h, w, seed=seed)
    return {'label': torch.from_numpy(b['label']), 'style_image': torch.from_numpy(b['style_image']),
            'target': torch.from_numpy(b['target']), 'filename': b['filename']}


def test_trainer_two_iterations_fp32_match_reference():
    """T1: G-step, D-step, G-step, D-step through Pix2PixTrainer on the HIP path vs the REAL
    reference's losses and parameter/buffer checksums (TTUR Adam, double power iteration, G
    regeneration in the D step)."""
    from seg2eye_amd.pix2pix_trainer import Pix2PixTrainer
    z = load_golden('trainer_ngf8_256')
    opt = _opt(ngf=8, ndf=8, crop_size=256, aspect_ratio=1.0, batchSize=2, compute_dtype='fp32')
    tr = Pix2PixTrainer(opt)
    m = tr.pix2pix_model
    for tag, net in (('G', m.netG), ('D', m.netD), ('E', m.netE)):
        sd = filled_state(z, tag)
        with torch.no_grad():
            for k, v in net.state_dict().items():
                v.copy_(sd[k])                           # in place: parameters alias the Adam arenas
    data = _batch(2, 256, 256, 21)
    for it in range(2):
        tr.run_generator_one_step(dict(data))
        tr.run_discriminator_one_step(dict(data))
        for k, v in tr.get_latest_losses().items():
            ref = z['it%d_%s' % (it, k.replace('/', '_'))]
            np.testing.assert_allclose(v.detach().cpu().numpy().reshape(ref.shape), ref, rtol=2e-3, atol=2e-4,
                                       err_msg='it%d %s' % (it, k))
        if it == 0:
            sub = tr.get_latest_generated().detach()[:, :, ::8, ::8].float().cpu().numpy()
            assert np.abs(sub - z['it0_fake_sub']).max() < G_TOL
        for tag, net in (('G', m.netG), ('D', m.netD), ('E', m.netE)):
            for k, v in net.state_dict().items():
                lr = opt.lr * 2 if tag == 'D' else opt.lr / 2       # TTUR (pix2pix_model.create_optimizers)
                # one sign flip of a near-zero gradient moves a weight by twice the largest step Adam(beta1=0, beta2=0.9) can
                # take at step t: lr * sqrt((1 - beta2^t) / (1 - beta2)) = 1, 1.38, ... x lr
                steps = sum(((1 - 0.9 ** t) / (1 - 0.9)) ** 0.5 for t in range(1, it + 2))
                flip = 2 * lr * steps if v.dtype.is_floating_point and not k.endswith(('_u', '_v')) else 0.0
                assert_checksum_close(v, z['it%d_ck_%s.%s' % (it, tag, k)], 2e-3, 'it%d %s.%s' % (it, tag, k), flip=flip)


@pytest.mark.parametrize('graphs', [False, True])
def test_trainer_openeds_loss_matches_oracle(graphs):
    """--lambda_openeds (pix2pix_model.py:206-210): the per-image OpenEDS error of the generated batch enters
    the logged G loss (no gradient); one G + D step on the HIP path vs the CPU oracle, eager and as hipGraph replays."""
    from oracle import seg2eye_oracle as O
    from seg2eye_amd.pix2pix_trainer import Pix2PixTrainer
    z = load_golden('trainer_ngf8_256')
    opt = _opt(ngf=8, ndf=8, crop_size=256, aspect_ratio=1.0, batchSize=2, compute_dtype='fp32', hip_graphs=graphs, lambda_openeds=3.0)
    tr = Pix2PixTrainer(opt)
    m = tr.pix2pix_model
    sds = {}
    for tag, net in (('G', m.netG), ('D', m.netD), ('E', m.netE)):
        sds[tag] = filled_state(z, tag)
        with torch.no_grad():
            for k, v in net.state_dict().items():
                v.copy_(sds[tag][k])
    batch = _batch(2, 256, 256, 21)
    data = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}
    tr.run_generator_one_step(dict(data))
    tr.run_discriminator_one_step(dict(data))
    got = tr.get_latest_losses()
    om = O.OracleModel(sds['G'], sds['D'], sds['E'], opt, 8, 8)
    gl, fake = om.run_generator_one_step({**batch, 'label': batch['label'].long()})
    assert 'openeds/weighted' in got and got['openeds/weighted'].shape == (2,)
    # a generated pixel within 1e-5 of an integer boundary may truncate either way: 1 grey level on a few pixels
    np.testing.assert_allclose(got['openeds/weighted'].detach().cpu().numpy(), gl['openeds/weighted'].numpy(), rtol=2e-3)
    np.testing.assert_allclose(float(got['GAN'].mean()), float(gl['GAN'].mean()), rtol=2e-3, atol=2e-4)
    log = m.get_loss_log()
    np.testing.assert_allclose(float(log['openeds/raw']) * 3.0, float(gl['openeds/weighted'].mean()), rtol=2e-3)


STYLE_LAMBDAS = dict(lambda_l2=15.0, lambda_l1=2.0, lambda_style_w=0.5, lambda_style_feat=0.001, lambda_gram=10000.0)


@pytest.mark.parametrize('graphs', [False, True])
def test_trainer_optional_losses_fp32_match_reference(graphs):
    """T2: the reference's own training recipe -- L2/L1 + the style-consistency terms that re-encode the generated
    image (netE runs twice in the G step) -- one G step + one D step on the HIP path vs the REAL reference's losses
    and parameter checksums; eager and as hipGraph replays."""
    from seg2eye_amd.pix2pix_trainer import Pix2PixTrainer
    z = load_golden('trainer_style_ngf8_256')
    opt = _opt(ngf=8, ndf=8, crop_size=256, aspect_ratio=1.0, batchSize=2, compute_dtype='fp32', hip_graphs=graphs, **STYLE_LAMBDAS)
    tr = Pix2PixTrainer(opt)
    m = tr.pix2pix_model
    for tag, net in (('G', m.netG), ('D', m.netD), ('E', m.netE)):
        sd = filled_state(z, tag)
        with torch.no_grad():
            for k, v in net.state_dict().items():
                v.copy_(sd[k])
    data = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in _batch(2, 256, 256, 23).items()}
    tr.run_generator_one_step(dict(data))
    tr.run_discriminator_one_step(dict(data))
    losses = tr.get_latest_losses()
    assert set(losses) == {'GAN', 'L2/weighted', 'L1/weighted', 'style_w/weighted', 'style_feat/weighted', 'gram/weighted',
                           'GAN_Feat', 'D/Fake', 'D/real'}
    for k, v in losses.items():
        ref = z['it0_%s' % k.replace('/', '_')]
        np.testing.assert_allclose(v.detach().cpu().numpy().reshape(ref.shape), ref, rtol=2e-3, atol=2e-4, err_msg=k)
    sub = tr.get_latest_generated().detach()[:, :, ::8, ::8].float().cpu().numpy()
    assert np.abs(sub - z['it0_fake_sub']).max() < G_TOL
    state0 = {tag: {k: v.detach().clone() for k, v in net.state_dict().items()} for tag, net in (('G', m.netG), ('D', m.netD), ('E', m.netE))}
    # the log-only '*/raw' entries (pix2pix_model.py:49-59, 196-229) survive get_latest_losses' reset under graph replay too:
    # every step logs its own values (L2/raw * lambda == L2/weighted of the same step)
    for _ in range(2):
        log = tr.get_latest_losses(include_log_losses=True)
        assert {'L2/raw', 'L1/raw', 'style_w/raw', 'style_feat/raw', 'gram/raw'} <= set(log), sorted(log)
        np.testing.assert_allclose(float(log['L2/raw']) * 15.0, float(log['L2/weighted'].mean()), rtol=1e-4)
        tr.run_generator_one_step(dict(data))
        tr.run_discriminator_one_step(dict(data))
    if not graphs:           # (capture runs warm-up iterations on the weights' spectral-norm state restored afterwards;
        for tag, net in (('G', m.netG), ('D', m.netD), ('E', m.netE)):      # parameters are compared on the eager run)
            for k, v in state0[tag].items():
                lr = opt.lr * 2 if tag == 'D' else opt.lr / 2
                flip = 2 * lr if v.dtype.is_floating_point and not k.endswith(('_u', '_v')) else 0.0
                assert_checksum_close(v, z['it0_ck_%s.%s' % (tag, k)], 2e-3, '%s.%s' % (tag, k), flip=flip)


@pytest.mark.parametrize('graphs', [False, True])
def test_trainer_max_aggregation_fp32_matches_reference(graphs):
    """T4: --style_aggr_method max (pix2pix_model.py:271-278; VERDICT r3: it ran through torch.max with no fixture anywhere): the
    aggregated style codes, one G step + one D step, netE's parameter gradients (only the arg-max style image of a component
    receives one) and every parameter / buffer afterwards on the HIP path vs the REAL reference; eager and as hipGraph replays."""
    from seg2eye_amd.pix2pix_trainer import Pix2PixTrainer
    z = load_golden('trainer_max_ngf8_256')
    opt = _opt(ngf=8, ndf=8, crop_size=256, aspect_ratio=1.0, batchSize=2, compute_dtype='fp32', hip_graphs=graphs, style_aggr_method='max')
    tr = Pix2PixTrainer(opt)
    m = tr.pix2pix_model
    for tag, net in (('G', m.netG), ('D', m.netD), ('E', m.netE)):
        sd = filled_state(z, tag)
        with torch.no_grad():
            for k, v in net.state_dict().items():
                v.copy_(sd[k])
    data = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in _batch(2, 256, 256, 29).items()}
    sdE = {k: v.detach().clone() for k, v in m.netE.state_dict().items()}
    with torch.no_grad():
        w = m(dict(data), 'encode_only')
    np.testing.assert_allclose(w.float().cpu().numpy(), z['w'], atol=5e-5, rtol=1e-3)
    with torch.no_grad():                                   # (the train-mode encode advanced netE's u, v: put them back)
        for k, v in m.netE.state_dict().items():
            v.copy_(sdE[k])
    tr.run_generator_one_step(dict(data))
    if not graphs:
        seen = 0
        for k, q in m.netE.named_parameters():
            key = 'it0_grad_E.' + k
            if key in z.files:
                assert_checksum_close(q.grad, z[key], 2e-3, 'grad E.' + k)
                seen += 1
        assert seen >= 8
    tr.run_discriminator_one_step(dict(data))
    losses = tr.get_latest_losses()
    for k, v in losses.items():
        ref = z['it0_%s' % k.replace('/', '_')]
        np.testing.assert_allclose(v.detach().cpu().numpy().reshape(ref.shape), ref, rtol=2e-3, atol=2e-4, err_msg=k)
    sub = tr.get_latest_generated().detach()[:, :, ::8, ::8].float().cpu().numpy()
    assert np.abs(sub - z['it0_fake_sub']).max() < G_TOL
    if not graphs:
        for tag, net in (('G', m.netG), ('D', m.netD), ('E', m.netE)):
            for k, v in net.state_dict().items():
                lr = opt.lr * 2 if tag == 'D' else opt.lr / 2
                flip = 2 * lr if v.dtype.is_floating_point and not k.endswith(('_u', '_v')) else 0.0
                assert_checksum_close(v, z['it0_ck_%s.%s' % (tag, k)], 2e-3, '%s.%s' % (tag, k), flip=flip)


def test_model_modes_and_bf16_step():
    from seg2eye_amd.pix2pix_trainer import Pix2PixTrainer
    z = load_golden('trainer_ngf8_256')
    opt = _opt(ngf=8, ndf=8, crop_size=256, aspect_ratio=1.0, batchSize=2, compute_dtype='bf16')
    tr = Pix2PixTrainer(opt)
    m = tr.pix2pix_model
    for tag, net in (('G', m.netG), ('D', m.netD), ('E', m.netE)):
        sd = filled_state(z, tag)
        with torch.no_grad():
            for k, v in net.state_dict().items():
                v.copy_(sd[k])
    data = _batch(2, 256, 256, 21)
    w = m(dict(data), 'encode_only')
    assert tuple(w.shape) == (2, 16)
    fake = m(dict(data), 'inference')
    assert tuple(fake.shape) == (2, 1, 256, 256) and float(fake.abs().max()) <= 1.0
    fake2 = m({**data, 'latent_style': w.detach().cpu()}, 'inference')
    assert tuple(fake2.shape) == (2, 1, 256, 256)
    with pytest.raises(ValueError):
        m(dict(data), 'nonsense')
    tr.run_generator_one_step(dict(data))
    tr.run_discriminator_one_step(dict(data))
    losses = {k: float(v) for k, v in tr.get_latest_losses().items()}
    assert set(losses) == {'GAN', 'GAN_Feat', 'D/Fake', 'D/real'}
    ref = {k: float(z['it0_%s' % k.replace('/', '_')]) for k in losses}
    for k in losses:                                     # bf16 step stays close to the fp32 reference
        assert abs(losses[k] - ref[k]) < 0.05 * max(1.0, abs(ref[k])), (k, losses[k], ref[k])


def test_trainer_nonsquare_batch3_runs():
    """cfg5-like geometry (H = 1.667 W, odd batch): two graph-free trainer iterations stay finite, the fake has the
    label's size, and every parameter moved."""
    from seg2eye_amd.pix2pix_trainer import Pix2PixTrainer
    from seg2eye_amd.options import image_hw
    from seg2eye_amd import synthetic as syn
    opt = _opt(ngf=8, ndf=8, crop_size=384, aspect_ratio=0.6, batchSize=3, compute_dtype='bf16')   # crop < 256 breaks E
    h, w = image_hw(opt)
    assert (h, w) == (640, 384)
    tr = Pix2PixTrainer(opt)
    m = tr.pix2pix_model
    for net, seed in ((m.netG, 1), (m.netD, 2), (m.netE, 3)):
        sd = syn.fill_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()], seed)
        with torch.no_grad():
            for k, v in net.state_dict().items():
                v.copy_(torch.from_numpy(sd[k]))
    before = tr.optimizer_G.flat_p.clone()
    data = _batch(3, h, w, 5)
    for _ in range(2):
        tr.run_generator_one_step(dict(data))
        tr.run_discriminator_one_step(dict(data))
    losses = {k: float(v) for k, v in tr.get_latest_losses().items()}
    assert all(np.isfinite(v) for v in losses.values()), losses
    assert tuple(tr.get_latest_generated().shape) == (3, 1, h, w)
    moved = (tr.optimizer_G.flat_p != before).float().mean()
    assert float(moved) > 0.99, float(moved)


def test_full_size_generator_fp32_pin():
    """Config 2 (BASELINE.json): ngf=64, 256x256, N=8, fp32 eval-mode G vs the reference's output
    (every 8th pixel + moments stored in the fixture)."""
    from seg2eye_amd import networks, synthetic as syn
    z = load_golden('g_ngf64_256_pin')
    opt = _opt(ngf=64, crop_size=256, aspect_ratio=1.0, compute_dtype='fp32')
    G = networks.define_G(opt)
    sd = syn.fill_state_dict(manifest_of(z, 'G'))
    G.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    G.eval()
    label = torch.from_numpy(syn.ellipse_labels(8, 256, 256, seed=1234)).to(DEV)
    w = torch.from_numpy(syn.hash_normal('latent_w', (8, 16), seed=1234)).to(DEV)
    with torch.no_grad():
        y = G(label, w).float().cpu()
    err = float((y[:, :, ::8, ::8] - torch.from_numpy(z['y_sub'])).abs().max())
    assert err < G_TOL, 'full-size G differs from the reference by %.3e' % err
    np.testing.assert_allclose([float(y.mean()), float(y.std())], z['stats'][:2], atol=1e-4)


def test_modules_fp32_match_reference():
    """G3: SPADE_STYLE_Block and both ResBlk flavours (fin == fout, fin != fout) vs the reference's
    outputs, input gradients and parameter-gradient checksums."""
    from seg2eye_amd import synthetic as syn
    from seg2eye_amd.networks.architecture import SPADE_STYLE_ResnetBlock
    from seg2eye_amd.networks.normalization import SPADE_STYLE_Block, SegMap
    z = load_golden('modules')
    opt = _opt(ngf=8, crop_size=64, compute_dtype='fp32')
    seg = SegMap.of(_label(z))
    C = 16
    errs = []
    for name, ctor in (('ssb', lambda: SPADE_STYLE_Block(C, opt)),
                       ('res_same', lambda: SPADE_STYLE_ResnetBlock(C, C, opt)),
                       ('res_diff', lambda: SPADE_STYLE_ResnetBlock(C, C // 2, opt))):
        m = ctor().to(DEV)
        m.load_state_dict(filled_state(z, name))
        m.eval()
        x = torch.from_numpy(z['x']).to(DEV).permute(0, 2, 3, 1).contiguous().requires_grad_(True)
        w = torch.from_numpy(z['w']).to(DEV).requires_grad_(True)
        y = m(x, seg, w)
        yr = z[name + '_y']
        e = float((y.permute(0, 3, 1, 2).cpu() - torch.from_numpy(yr)).abs().max())
        errs.append((name + ' y', e, 2e-4 * np.abs(yr).max()))
        proj = torch.from_numpy(syn.hash_uniform('proj_' + name, yr.shape, seed=11)).to(DEV).permute(0, 2, 3, 1)
        (y * proj).sum().backward()
        for key, got in (('_dx', x.grad.permute(0, 3, 1, 2)), ('_dw', w.grad)):
            ref = z[name + key]
            errs.append((name + key, float((got.cpu() - torch.from_numpy(ref)).abs().max()), 1e-3 * np.abs(ref).max()))
        for k, p in m.named_parameters():
            ref = z['%s_grad_%s' % (name, k)]
            from conftest import checksum
            got = checksum(p.grad)
            errs.append(('%s:%s' % (name, k), abs(got[1] - ref[1]) + abs(got[0] - ref[0]), 2e-3 * ref[1]))
    bad = [e for e in errs if not e[1] <= e[2]]
    assert not bad, '\n'.join('%s err %.3e > %.3e' % e for e in bad)


@pytest.mark.parametrize('fin,fout,name', [(16, 8, 'res_diff'), (16, 16, 'res_same')])
@pytest.mark.parametrize('hw', [16, 64])
def test_resblk_matches_oracle_tight(fin, fout, name, hw):
    """One SPADE+Style ResBlk, forward and every gradient, against the CPU oracle at 1e-5 relative."""
    from oracle import seg2eye_oracle as O
    from seg2eye_amd import synthetic as syn
    from seg2eye_amd.networks.architecture import SPADE_STYLE_ResnetBlock
    from seg2eye_amd.networks.normalization import SegMap
    z = load_golden('modules')
    sd = filled_state(z, name)
    opt = _opt(ngf=8, crop_size=64, compute_dtype='fp32')
    lab = torch.from_numpy(syn.ellipse_labels(2, 64, 64, seed=11))
    seg = O.one_hot_labels(lab.long(), 4)
    x = torch.from_numpy(syn.hash_normal('dbg_x', (2, fin, hw, hw), seed=hw))
    w = torch.from_numpy(syn.hash_normal('dbg_w', (2, 16), seed=3))
    leaf = {('p.' + k): (v.clone().requires_grad_(True) if O.OracleModel.is_param(k) else v) for k, v in sd.items()}
    xo, wo = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    yo = O.spade_style_resblk(leaf, 'p', xo, seg, wo, False, None)
    proj = torch.from_numpy(syn.hash_uniform('dbg_p', tuple(yo.shape), seed=5))
    (yo * proj).sum().backward()
    m = SPADE_STYLE_ResnetBlock(fin, fout, opt).to(DEV)
    m.load_state_dict(sd)
    m.eval()
    xg = x.to(DEV).permute(0, 2, 3, 1).contiguous().requires_grad_(True)
    wg = w.to(DEV).requires_grad_(True)
    y = m(xg, SegMap.of(lab.to(DEV)), wg)
    (y * proj.to(DEV).permute(0, 2, 3, 1)).sum().backward()
    rel = lambda a, b: float((a.cpu() - b).abs().max() / (b.abs().max() + 1e-12))
    assert rel(y.permute(0, 3, 1, 2).detach(), yo.detach()) < 1e-5
    assert rel(xg.grad.permute(0, 3, 1, 2), xo.grad) < 1e-5
    assert rel(wg.grad, wo.grad) < 1e-5
    for k, p in m.named_parameters():
        assert rel(p.grad, leaf['p.' + k].grad) < 2e-5, k


def test_hip_graph_capture_failure_falls_back_to_eager(monkeypatch, capsys):
    """A capture that fails (e.g. a runtime thread interfering in a multi-process job) must not take the job down:
    the trainer reports it once and runs the same step bodies eagerly."""
    from seg2eye_amd.pix2pix_trainer import Pix2PixTrainer
    tr = Pix2PixTrainer(_opt(ngf=8, ndf=8, crop_size=256, aspect_ratio=1.0, batchSize=2, compute_dtype='bf16', hip_graphs=True))

    def boom(data):
        raise RuntimeError('capture refused')
    monkeypatch.setattr(tr, '_capture', boom)
    data = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in _batch(2, 256, 256, 5).items()}
    for _ in range(2):
        tr.run_generator_one_step(dict(data))
        tr.run_discriminator_one_step(dict(data))
    assert tr.use_graphs is False and tr.graph_G is None
    assert 'continuing without graphs' in capsys.readouterr().err
    assert all(bool(torch.isfinite(v.float()).all()) for v in tr.get_latest_losses().values())


def test_hip_graph_steps_match_eager():
    """opt.hip_graphs: replaying the captured step bodies must follow the eager trajectory (same losses
    over 3 iterations within float-atomics noise, capture itself leaves weights AND u, v untouched)."""
    from seg2eye_amd.pix2pix_trainer import Pix2PixTrainer
    z = load_golden('trainer_ngf8_256')
    res = {}
    for graphs in (False, True):
        opt = _opt(ngf=8, ndf=8, crop_size=256, aspect_ratio=1.0, batchSize=2, compute_dtype='fp32', hip_graphs=graphs)
        tr = Pix2PixTrainer(opt)
        m = tr.pix2pix_model
        for tag, net in (('G', m.netG), ('D', m.netD), ('E', m.netE)):
            sd = filled_state(z, tag)
            with torch.no_grad():
                for k, v in net.state_dict().items():
                    v.copy_(sd[k])
        data = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in _batch(2, 256, 256, 21).items()}
        hist = []
        for it in range(3):
            tr.run_generator_one_step(dict(data))
            tr.run_discriminator_one_step(dict(data))
            hist.append({k: float(v.float().mean()) for k, v in tr.get_latest_losses().items()})
        res[graphs] = (hist, {k: v.detach().float().cpu().clone() for k, v in m.netG.state_dict().items()})
    # iteration 0 runs on identical weights: tight.  Later iterations have taken beta1 = 0 Adam steps (+-lr per
    # weight, sign flips on near-zero gradients under float-atomic noise), so the trajectories drift a little.
    for it, (a, b) in enumerate(zip(res[False][0], res[True][0])):
        for k in a:
            assert abs(a[k] - b[k]) <= (5e-4 if it == 0 else 1e-2) * max(1.0, abs(a[k])), (it, k, a[k], b[k])
    ref = {k: float(z['it0_%s' % k.replace('/', '_')]) for k in res[True][0][0]}
    for k, v in res[True][0][0].items():                      # and the graphed first iteration matches the real reference
        assert abs(v - ref[k]) <= 2e-3 * max(1.0, abs(ref[k])), (k, v, ref[k])
    # beta1 = 0, beta2 = 0.9: step t moves a weight by at most lr_G * sqrt((1 - beta2^t) / (1 - beta2)) (a gradient much
    # larger than its history: v_hat = (1 - beta2) g^2 / (1 - beta2^t)), i.e. 1, 1.38, 1.65 x lr_G; a near-zero gradient whose
    # sign flips under float-atomic summation noise differs by twice that per step.  3 steps at lr_G = 1e-4
    bound = 2 * 1e-4 * sum(((1 - 0.9 ** t) / (1 - 0.9)) ** 0.5 for t in (1, 2, 3)) + 1e-5
    for k, v in res[False][1].items():
        assert float((v - res[True][1][k]).abs().max()) <= bound, k


def test_full_size_train_step_matches_oracle():
    """The bench configuration's architecture (ngf = ndf = 64, 256x256) at batch 1: one G step + one D step through
    Pix2PixTrainer on the HIP path in fp32 vs the CPU oracle on the same seeded weights and inputs -- the full-size
    shapes exercise what the small fixtures cannot (split-K, 1024-channel tiles, the 1-channel stream kernels, the
    batched pack / gradient re-layout at 100 M parameters) -- then the bf16 step against the fp32 one."""
    from oracle import seg2eye_oracle as O
    from seg2eye_amd import synthetic as syn
    from seg2eye_amd.pix2pix_trainer import Pix2PixTrainer
    b = syn.make_batch(1, 256, 256, seed=33)
    data = {'label': torch.from_numpy(b['label']), 'style_image': torch.from_numpy(b['style_image']),
            'target': torch.from_numpy(b['target'])}
    res, sds = {}, None
    for dt in ('fp32', 'bf16'):
        opt = _opt(ngf=64, ndf=64, crop_size=256, aspect_ratio=1.0, batchSize=1, compute_dtype=dt)
        tr = Pix2PixTrainer(opt)
        m = tr.pix2pix_model
        if sds is None:
            sds = {}
            for tag, net in (('G', m.netG), ('D', m.netD), ('E', m.netE)):
                filled = syn.fill_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()])
                sds[tag] = {k: torch.from_numpy(v) for k, v in filled.items()}
        for tag, net in (('G', m.netG), ('D', m.netD), ('E', m.netE)):
            with torch.no_grad():
                for k, v in net.state_dict().items():
                    v.copy_(sds[tag][k])
        tr.run_generator_one_step(dict(data))
        tr.run_discriminator_one_step(dict(data))
        res[dt] = ({k: float(v.detach().float().mean()) for k, v in tr.get_latest_losses().items()},
                   tr.get_latest_generated().float().cpu())
        del tr, m
        torch.cuda.empty_cache()
    opt = _opt(ngf=64, ndf=64, crop_size=256, aspect_ratio=1.0, batchSize=1, compute_dtype='fp32')
    torch.set_num_threads(min(16, torch.get_num_threads()))
    om = O.OracleModel(sds['G'], sds['D'], sds['E'], opt, 8, 8)
    odata = {**data, 'label': data['label'].long()}
    gl, fake = om.run_generator_one_step(odata)
    dl = om.run_discriminator_one_step(odata)
    err = float((res['fp32'][1] - fake).abs().max())
    assert err < G_TOL, 'full-size fp32 generator output differs from the oracle by %.3e' % err
    for k, v in {**gl, **dl}.items():
        r = float(v.mean())
        assert abs(res['fp32'][0][k] - r) <= 2e-3 * max(1.0, abs(r)), (k, res['fp32'][0][k], r)
        assert abs(res['bf16'][0][k] - r) <= 0.05 * max(1.0, abs(r)), (k, res['bf16'][0][k], r)
    d = (res['bf16'][1] - res['fp32'][1]).abs()
    assert float(d.mean()) < 3e-2 and float(d.max()) < 0.5, (float(d.mean()), float(d.max()))


@pytest.mark.parametrize('exchange', ['after_backward', 'overlap', 'overlap+bf16+direct', 'overlap+debug_sync'])
def test_bench_two_ranks_dry_run(exchange):
    """`python bench.py --gpus 2` with NO launcher: bench.py starts its own two ranks in a child process; here
    they share this box's GPU over gloo (S2E_DIST_BACKEND=gloo: RCCL refuses two ranks on one device; the collective calls
    are the same).  Covers the multi-rank control flow -- barriers, max-over-ranks timing, the eager event pass on EVERY rank
    (a step contains the gradient all-reduce, so rank 0 alone would wait for ever), the final barrier -- and that BOTH
    exchanges run on hipGraph replays: the overlapped one as one graph segment per gradient group."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, S2E_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    # round 5: the bf16 payload through the spelled-out direct exchange (all-to-all + owner sum + all-gather), and the
    # overlapped exchange under S2E_DEBUG_SYNC -- every group's slice must still hold the bits it had when its hook declared it final
    # (i.e. no later graph segment, deferred weight-gradient batch or chain rule writes a group that has been handed to the exchange)
    extra = []
    exchange, _, opts = exchange.partition('+')
    if 'bf16' in opts:
        extra = ['--grad-dtype', 'bf16', '--grad-exchange', 'direct']
    if 'debug_sync' in opts:
        env['S2E_DEBUG_SYNC'] = '1'
    out = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--steps', '2', '--warmup', '1', '--ngf', '16',
                          '--batch', '2', '--exchange', exchange, '--full'] + extra, env=env, capture_output=True, text=True, timeout=600, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]                       # rank 0 prints ONE line
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['config']['global_batch'] == 4 and d['config']['parallelism'] == 'dp2' and d['rccl_ranks'] == 2
    assert d['value'] > 0 and 'roofline' in d and 'cpu_baseline' not in d
    assert d['config']['gradient_exchange'] == exchange and d['hip_graphs'] is True, d['config']
    assert d['config']['graph_segments_G'] == (6 if exchange == 'overlap' else 1), d['config']
    ex = d['config']['exchange']
    assert ex['payload'] == ('bf16' if extra else 'fp32') and ex['algorithm'] == ('direct' if extra else 'allreduce') and ex['groups'] == 6, ex


def test_bench_plain_run_and_dump_outputs(tmp_path):
    """A plain `bench.py` run prints the headline alone (nothing of --full), times exactly --steps steps, and --dump-outputs
    writes the last timed step's outputs as float32 .npy files: the generated batch and the losses of the line.  That step starts
    from the set-up state, so two runs with the same arguments write the same outputs up to the rounding of one step's
    float-atomic sums (without the restore the steps before it carry their rounding into the weights, further every step)."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'S2E_DIST_BACKEND', 'S2E_DETERMINISTIC')}
    runs = []
    for tag in ('a', 'b'):
        dump = tmp_path / tag
        out = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', '6', '--warmup', '2', '--ngf', '16',
                              '--batch', '2', '--dump-outputs', str(dump)], env=env, capture_output=True, text=True, timeout=600, cwd=root)
        assert out.returncode == 0, out.stderr[-3000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
        assert len(lines) == 1, out.stdout[-2000:]
        d = json.loads(lines[0])
        assert d['steps'] == 6 and d['value'] > 0 and d['unit'] == 'images/s' and d['higher_is_better'] is True and d['dtype'] == 'bf16'
        assert abs(d['value'] - 2 / (d['ms_per_step'] / 1e3)) <= 1e-6 * d['value'], d
        for k in ('roofline', 'kernels', 'ms_per_step_median', 'single_batch', 'dense_labels', 'eager', 'secondary', 'cpu_baseline'):
            assert k not in d, k
        files = sorted(os.listdir(dump))
        assert files == sorted(['generated.npy'] + ['loss_%s.npy' % k.replace('/', '_') for k in d['losses']]), files
        arrs = {f: np.load(os.path.join(dump, f)) for f in files}
        for f, a in arrs.items():
            assert a.dtype == np.float32 and np.isfinite(a).all(), f
        assert arrs['generated.npy'].shape == (2, 1, 256, 256)      # (output_nc = 1: grey-level eye images)
        for k, v in d['losses'].items():
            np.testing.assert_allclose(float(arrs['loss_%s.npy' % k.replace('/', '_')].mean()), v, rtol=1e-6)
        runs.append(arrs)
    # the generator's output is tanh in [-1, 1], computed in bf16 (one ulp near 1: 2^-8)
    np.testing.assert_allclose(runs[0]['generated.npy'], runs[1]['generated.npy'], rtol=0, atol=1e-2)
    for f in runs[0]:
        if f.startswith('loss_'):
            np.testing.assert_allclose(runs[0][f], runs[1][f], rtol=1e-3, atol=1e-4, err_msg=f)


def test_bench_refuses_more_ranks_than_gpus():
    """--gpus N beyond the visible devices is refused (exit status 2) before anything is launched -- unless the gloo dry run is asked for."""
    import os, subprocess, sys
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'S2E_DIST_BACKEND')}
    out = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', str(torch.cuda.device_count() + 1)], env=env,
                         capture_output=True, text=True, timeout=300, cwd=root)
    assert out.returncode == 2 and 'GPU(s) visible' in out.stderr, (out.returncode, out.stderr[-500:])


# ------------------------------------------------------------------------------------------ config 3 AS BENCHED
_BLOCKS = ('head_0', 'G_middle_0', 'G_middle_1', 'up_0', 'up_1', 'up_2', 'up_3')


def _bench_shape_kernels(dt):
    """The kernels the library picks for the layers of the benchmarked configuration (N = 8, 256x256, ngf = ndf = 64):
    name -> kind, via the same planner calls the launches use."""
    import ctypes as C
    from seg2eye_amd import _lib as L
    lib = L.lib()
    d = L.S2E_BF16 if dt == 'bf16' else L.S2E_F32

    def conv(n, h, cin, cout, k, s, p, tr=0):
        ho = h if s == 1 and 2 * p == k - 1 else ((h + 2 * p - k) // s + 1)
        desc = L.ConvDesc(n, h, h, cin, ho, ho, cout, k, k, s, p, tr, 0, 0, 0) if not tr else \
            L.ConvDesc(n, ho, ho, cout, h, h, cin, k, k, s, p, 1, 0, 0, 0)
        return lib.s2e_conv2d_kernel_kind(d, C.byref(desc)), lib.s2e_conv2d_workspace_bytes(d, C.byref(desc))

    def wgrad(n, h, cin, cout, k):
        desc = L.ConvDesc(n, h, h, cin, h, h, cout, k, k, 1, k // 2, 0, 0, 0, 0)
        return lib.s2e_conv2d_wgrad_kernel_kind(d, C.byref(desc))
    return {
        'up_3 conv_0 fwd': conv(8, 256, 128, 64, 3, 1, 1), 'up_2 conv_0 fwd': conv(8, 128, 256, 128, 3, 1, 1),
        'mid conv split fwd': conv(8, 16, 1024, 1024, 3, 1, 1), 'gb dgrad 32^2': conv(8, 32, 128, 2048, 3, 1, 1, 1),
        'D m3 4x4 s1': conv(16, 33, 256, 512, 4, 1, 2),
        'gb wgrad 256^2': wgrad(8, 256, 128, 256, 3), 'up_1 wgrad': wgrad(8, 64, 512, 256, 3),
        'fused 256^2 C=128': lib.s2e_spade_conv_modulate_supported(d, 8, 256, 256, 128, 128, 0),
        'fused 16^2 C=1024': lib.s2e_spade_conv_modulate_supported(d, 8, 16, 16, 1024, 128, 0),
    }


def _cfg3_run(dt, graphs, z, steps=1, hooks=True, crop=256, aspect=1.0, n=8, hw=(256, 256), seed=1234):
    """One (or more) G+D iterations of Pix2PixTrainer at the benchmarked configuration (or, with the keywords, config 5's per-GPU
    workload) on the fixture's weights and batch.
    -> dict(losses, fake, acts {block: NCHW fp32 cpu}, grads {name: fp32 gpu clone}, trainer)"""
    from seg2eye_amd.pix2pix_trainer import Pix2PixTrainer
    opt = _opt(ngf=64, ndf=64, crop_size=crop, aspect_ratio=aspect, batchSize=n, compute_dtype=dt, hip_graphs=graphs)
    tr = Pix2PixTrainer(opt)
    m = tr.pix2pix_model
    for tag, net in (('G', m.netG), ('D', m.netD), ('E', m.netE)):
        sd = filled_state(z, tag)
        with torch.no_grad():
            for k, v in net.state_dict().items():
                v.copy_(sd[k])
    data = _batch(n, hw[0], hw[1], seed)
    acts, hs = {}, []
    if hooks:
        for name in _BLOCKS:
            def hook(mod, inp, out, name=name):
                acts.setdefault(name, out.detach().permute(0, 3, 1, 2).float().contiguous().cpu())   # first call = the G step's forward
            hs.append(getattr(m.netG, name).register_forward_hook(hook))
    out = {'acts': acts, 'tr': tr}
    for it in range(steps):
        tr.run_generator_one_step(dict(data))
        if it == 0:
            for h in hs:
                h.remove()
            torch.cuda.synchronize()
            out['grads_G'] = {('G.' + k): p.grad.detach().clone() for k, p in m.netG.named_parameters() if p.grad is not None}
            out['grads_G'].update({('E.' + k): p.grad.detach().clone() for k, p in m.netE.named_parameters() if p.grad is not None})
            out['fake'] = tr.get_latest_generated().detach().float().cpu()
        tr.run_discriminator_one_step(dict(data))
        if it == 0:
            torch.cuda.synchronize()
            out['grads_D'] = {('D.' + k): p.grad.detach().clone() for k, p in m.netD.named_parameters() if p.grad is not None}
            out['losses'] = {k: float(v.detach().float().mean()) for k, v in tr.get_latest_losses().items()}
    return out


def _relrms(a, b):
    a, b = a.double(), b.double()
    return float(((a - b) ** 2).mean().sqrt() / b.pow(2).mean().sqrt().clamp_min(1e-30))


def _check_fp32_step_against_reference(a, z):
    """`a` = _cfg3_run('fp32', False, z, ...): losses 2e-3, generated image < 1e-3, every ResBlk output, every G / E / D parameter
    gradient and every parameter / buffer after the iteration against the reference trainer's fixture `z`, by checksum."""
    errs = []
    for k, v in a['losses'].items():
        ref = float(z['it0_%s' % k.replace('/', '_')].reshape(-1)[0])
        errs.append(('loss ' + k, abs(v - ref), 2e-3 * max(1.0, abs(ref))))
    errs.append(('fake', float(np.abs(a['fake'][:, :, ::8, ::8].numpy() - z['it0_fake_sub']).max()), G_TOL))
    from conftest import checksum
    for name in _BLOCKS:
        ref, got = z['it0_act_' + name], checksum(a['acts'][name])
        scale = ref[1] / a['acts'][name].numel()                                       # mean |activation|
        errs.append(('act ' + name + ' sums', abs(got[0] - ref[0]) + abs(got[1] - ref[1]), 1e-4 * ref[1]))
        errs.append(('act ' + name + ' samples', float(np.abs(got[2:] - ref[2:]).max()), 2e-3 * scale))
    ngrad = 0
    # D's gradients belong to the D step, i.e. they sit behind netG's Adam update: with beta1 = 0 the first update is
    # -lr * sign(g), so gradients within summation noise of zero move their weight by +lr here and -lr there and the
    # regenerated image -- D's input -- differs by ~1e-4: their sums wobble at the 2e-3 level run to run (measured)
    for grads, rt in ((a['grads_G'], 2e-3), (a['grads_D'], 6e-3)):
        for k, g in grads.items():
            key = 'it0_grad_' + k
            if key not in z.files:
                continue
            ref, got = z[key], checksum(g)
            ngrad += 1
            # (a one-element gradient -- conv_img's bias -- is a signed sum over N*H*W pixels that cancels to ~1e-3: its error is
            # fp32 summation noise relative to the L1 mass of the summands, not to the sum; measured 3e-5)
            errs.append(('grad ' + k + ' sums', abs(got[0] - ref[0]) + abs(got[1] - ref[1]), rt * ref[1] + (1e-4 if g.numel() == 1 else 1e-9)))
            # 16 sampled elements: each is a signed sum over all pixels (the one-hot input channels of D's first layer cancel
            # to a few % of the mean magnitude): bound relative to the mean |g| of the tensor; worst measured 0.053
            errs.append(('grad ' + k + ' samples', float(np.abs(got[2:] - ref[2:]).max()), 0.1 * ref[1] / g.numel() + 1e-9))
    assert ngrad >= 200, ngrad
    bad = [e for e in errs if not e[1] <= e[2]]
    assert not bad, '\n'.join('%s err %.3e > %.3e' % e for e in bad)
    m = a['tr'].pix2pix_model
    for tag, net in (('G', m.netG), ('D', m.netD), ('E', m.netE)):
        lr = 2e-4 * 2 if tag == 'D' else 2e-4 / 2
        for k, v in net.state_dict().items():
            flip = 2 * lr if v.dtype.is_floating_point and not k.endswith(('_u', '_v')) else 0.0
            assert_checksum_close(v, z['it0_ck_%s.%s' % (tag, k)], 2e-3, 'after it0 %s.%s' % (tag, k), flip=flip)


def test_cfg3_as_benched_matches_reference():
    """BASELINE.json configs[2] exactly as bench.py runs it -- ngf = ndf = 64, 256x256, batch 8, the bench's seed-1234 batch --
    against ONE G step + ONE D step of the real reference's Pix2PixTrainer (trainers/pix2pix_trainer.py:26-45; fixture
    trainer_ngf64_256_n8.npz, `make_golden.py --only full-train`):
      (a) fp32 eager: losses 2e-3, generated image < 1e-3, every ResBlk output, every G / E / D parameter gradient and every
          parameter / buffer after the iteration, by checksum;
      (b) bf16 eager against the fp32 run: every ResBlk output, losses, the weight gradients of the five largest layers;
      (c) bf16 with hipGraphs ON (what the bench times): the replayed step against (b) and against the reference's losses.
    The shapes take the patch-resident / split / fused kernels at batch 8 (they take the generic one at batch 1): asserted."""
    z = load_golden('trainer_ngf64_256_n8')
    from seg2eye_amd import _lib as L
    for dt in ('fp32', 'bf16'):
        kinds = _bench_shape_kernels(dt)
        for name in ('up_3 conv_0 fwd', 'up_2 conv_0 fwd', 'mid conv split fwd', 'gb dgrad 32^2', 'D m3 4x4 s1'):
            assert kinds[name][0] == 2, (dt, name, kinds[name])                       # S2E_KERNEL_PATCH
        assert kinds['mid conv split fwd'][1] > 0, kinds['mid conv split fwd']          # ... split over channel chunks
        assert kinds['fused 256^2 C=128'] == 1 and kinds['fused 16^2 C=1024'] == 1, kinds
        if dt == 'bf16':
            assert kinds['gb wgrad 256^2'] == 2 and kinds['up_1 wgrad'] == 2, kinds     # patch-resident weight gradient
    # ---- (a) fp32 eager vs the reference
    a = _cfg3_run('fp32', False, z)
    _check_fp32_step_against_reference(a, z)
    fp32 = {k: a[k] for k in ('losses', 'fake', 'acts', 'grads_G', 'grads_D')}
    del a
    torch.cuda.empty_cache()
    # ---- (b) bf16 eager vs fp32
    b = _cfg3_run('bf16', False, z)
    rep = {name: _relrms(b['acts'][name], fp32['acts'][name]) for name in _BLOCKS}
    big = sorted(fp32['grads_G'], key=lambda k: -fp32['grads_G'][k].numel())[:5]
    grep = {k: _relrms(b['grads_G'][k], fp32['grads_G'][k]) for k in big}
    drep = {k: _relrms(b['grads_D'][k], fp32['grads_D'][k]) for k in sorted(fp32['grads_D'], key=lambda k: -fp32['grads_D'][k].numel())[:3]}
    print('cfg3 bf16 vs fp32: ResBlk rel-RMS', {k: round(v, 4) for k, v in rep.items()})
    print('cfg3 bf16 vs fp32: wgrad rel-RMS', {k: round(v, 4) for k, v in {**grep, **drep}.items()})
    print('cfg3 losses fp32 %s | bf16 %s' % (fp32['losses'], b['losses']))
    assert max(rep.values()) < 2e-2, rep
    # measured: ResBlk outputs 0.4 % (head_0) ... 1.3 % (up_3); weight gradients 3.6 - 5.6 % (they sit behind the whole bf16
    # backward through D and G)
    assert max(grep.values()) < 8e-2 and max(drep.values()) < 8e-2, (grep, drep)
    for k, v in b['losses'].items():
        assert abs(v - fp32['losses'][k]) <= 2e-2 * max(1.0, abs(fp32['losses'][k])), (k, v, fp32['losses'][k])
    dimg = (b['fake'] - fp32['fake']).abs()
    print('cfg3 bf16 image vs fp32: mean %.4f max %.4f rel-RMS %.4f' % (float(dimg.mean()), float(dimg.max()), _relrms(b['fake'], fp32['fake'])))
    assert _relrms(b['fake'], fp32['fake']) < 3e-2 and float(dimg.mean()) < 1e-2
    bf = {k: b[k] for k in ('losses', 'fake', 'grads_G')}
    del b
    torch.cuda.empty_cache()
    # ---- (c) bf16 + hipGraphs: the replayed step (what bench.py times)
    c = _cfg3_run('bf16', True, z, steps=1, hooks=False)
    assert c['tr'].use_graphs and c['tr'].graph_G is not None, 'the step did not run as a hipGraph replay'
    for k, v in c['losses'].items():
        ref = float(z['it0_%s' % k.replace('/', '_')].reshape(-1)[0])
        assert abs(v - bf['losses'][k]) <= 1e-2 * max(1.0, abs(bf['losses'][k])), ('graph vs eager', k, v, bf['losses'][k])
        assert abs(v - ref) <= 2e-2 * max(1.0, abs(ref)), ('graph vs reference', k, v, ref)
    assert _relrms(c['fake'], fp32['fake']) < 3e-2
    g5 = {k: _relrms(c['grads_G'][k], fp32['grads_G'][k]) for k in big}
    print('cfg3 bf16 hipGraph vs fp32: wgrad rel-RMS', {k: round(v, 4) for k, v in g5.items()})
    assert max(g5.values()) < 8e-2, g5


def _trajectory(dt, graphs, z, iters, seeds):
    """`iters` G+D iterations of Pix2PixTrainer at the benchmarked configuration from the fixture's weights, batch `seeds[it % len]`
    at iteration it.  -> per-iteration losses, the last generated image, the G / D parameter arenas before and after."""
    from seg2eye_amd.pix2pix_trainer import Pix2PixTrainer
    opt = _opt(ngf=64, ndf=64, crop_size=256, aspect_ratio=1.0, batchSize=8, compute_dtype=dt, hip_graphs=graphs)
    tr = Pix2PixTrainer(opt)
    m = tr.pix2pix_model
    for tag, net in (('G', m.netG), ('D', m.netD), ('E', m.netE)):
        sd = filled_state(z, tag)
        with torch.no_grad():
            for k, v in net.state_dict().items():
                v.copy_(sd[k])
    batches = [_batch(8, 256, 256, sd) for sd in seeds]
    p0 = (tr.optimizer_G.flat_p.clone(), tr.optimizer_D.flat_p.clone())
    losses = []
    for it in range(iters):
        data = batches[it % len(batches)]
        tr.run_generator_one_step(dict(data))
        tr.run_discriminator_one_step(dict(data))
        losses.append({k: float(v.detach().float().mean()) for k, v in tr.get_latest_losses().items()})
    torch.cuda.synchronize()
    out = {'losses': losses, 'fake': tr.get_latest_generated().detach().float().cpu(), 'p0': p0,
           'p': (tr.optimizer_G.flat_p.clone(), tr.optimizer_D.flat_p.clone()), 'graphs': tr.use_graphs and tr.graph_G is not None}
    del tr
    torch.cuda.empty_cache()
    return out


def test_bf16_trajectory_tracks_fp32_over_20_iterations():
    """the benchmarked dtype beyond ONE step.  20 G+D iterations of trainers/pix2pix_trainer.py:26-45 at the bench's
    size (ngf = ndf = 64, 256x256, batch 8; four batches in rotation) from the same weights:
      A, A' -- fp32, eager, twice: their difference is the trajectory's OWN run-to-run spread (weight-gradient partial sums are
               combined with float atomics, and Adam with beta1 = 0 turns a 1e-7 difference of a near-zero gradient into a +-lr step);
      B     -- bf16 with hipGraphs on (what bench.py times).
    What can be asked of B is set by A': this GAN is chaotic at the fixture's weights -- measured (round 5), A' itself leaves A within
    ~6 iterations: by iteration 20 its losses differ from A's by 0.06-0.40 (of max(1, |loss|)), its last generated image by rel-RMS
    1.6 (decorrelated), its parameters by 0.83 (G) / 0.46 (D) of the distance training moved them.  So: (1) while the trajectories
    still coincide -- the first 3 iterations -- B's losses are within 5 % of A's (measured 0.8-1.3 %), and within 25 % over the first 8
    (measured 6 %; bf16's 2e-3 start grows ~1.4x an iteration); (2) over all 20 iterations B stays as close to A as another fp32 run
    does, up to a stated factor OR the distance two decorrelated runs of this model sit apart -- A' 's own spread varies 2.5x from run
    to run (ten runs), so a pure ratio against it failed one run in four: parameter distance <= max(1.5 x A' 's, the distance training
    moved them) + 0.05 (G 0.84-0.96 vs 0.83-0.97, D 0.52-0.64 vs 0.41-0.53), worst loss deviation <= max(5 x A' 's, 2.0) + 0.05
    (0.54-1.40 vs 0.26-0.69: hinge losses of order 1 that have decorrelated), and the last generated image -- decorrelated from A's in
    BOTH, rel-RMS 1.27-2.05 vs 0.89-1.90 -- of the same energy and not further than max(2 x A' 's, 2.5) + 0.5.  Divergence, NaNs or a
    collapsed generator are one to several orders outside every one of these."""
    z = load_golden('trainer_ngf64_256_n8')
    iters, seeds = 20, (1234, 77, 2024, 5)
    a = _trajectory('fp32', False, z, iters, seeds)
    a2 = _trajectory('fp32', False, z, iters, seeds)
    b = _trajectory('bf16', True, z, iters, seeds)
    assert b['graphs'], 'the bf16 run did not replay hipGraphs'
    # per loss: the largest deviation from A over the 20 iterations, in units of max(1, |loss|) -- for B and for A's own rerun
    worst, spread = {}, {}
    for it in range(iters):
        for k, v in a['losses'][it].items():
            worst[k] = max(worst.get(k, 0.0), abs(b['losses'][it][k] - v) / max(1.0, abs(v)))
            spread[k] = max(spread.get(k, 0.0), abs(a2['losses'][it][k] - v) / max(1.0, abs(v)))
    early = max(abs(b['losses'][it][k] - v) / max(1.0, abs(v)) for it in range(3) for k, v in a['losses'][it].items())
    per_it = lambda r: [round(max(abs(r['losses'][it][k] - v) / max(1.0, abs(v)) for k, v in a['losses'][it].items()), 3) for it in range(iters)]
    print('trajectory losses: worst deviation bf16 %s | fp32 rerun %s | bf16, first 3 iterations %.4f'
          % ({k: round(v, 4) for k, v in worst.items()}, {k: round(v, 4) for k, v in spread.items()}, early))
    print('trajectory losses, max deviation per iteration: bf16 %s | fp32 rerun %s' % (per_it(b), per_it(a2)))
    img_b, img_a2 = _relrms(b['fake'], a['fake']), _relrms(a2['fake'], a['fake'])
    rep = {}
    for i, tag in enumerate(('G', 'D')):
        moved = (a['p'][i] - a['p0'][i]).double().norm()                       # how far 20 iterations moved the parameters
        rep[tag] = (float((b['p'][i] - a['p'][i]).double().norm() / moved), float((a2['p'][i] - a['p'][i]).double().norm() / moved))
    print('trajectory (20 it): worst loss deviation %s | image rel-RMS bf16 %.4f, fp32 rerun %.4f | parameter distance / movement: %s'
          % ({k: round(v, 4) for k, v in worst.items()}, img_b, img_a2, {k: (round(x, 4), round(y, 4)) for k, (x, y) in rep.items()}))
    assert early < 5e-2, early
    assert max(per_it(b)[:8]) < 0.25, per_it(b)
    for k in worst:
        assert np.isfinite(worst[k]) and worst[k] < max(5.0 * spread[k], 2.0) + 5e-2, (k, worst[k], spread[k])
    # (two decorrelated images of equal energy are rel-RMS sqrt(2) apart; over ten runs A' sat at 0.89 ... 1.90 from A, B at 1.27 ... 2.05)
    assert img_b < max(2.0 * img_a2, 2.5) + 0.5, (img_b, img_a2)
    energy = float(b['fake'].double().pow(2).mean().sqrt() / a['fake'].double().pow(2).mean().sqrt())
    assert 0.5 < energy < 2.0, energy
    for tag, (db, da) in rep.items():
        assert db < max(1.5 * da, 1.0) + 5e-2, (tag, db, da)    # as far from A as another fp32 run, or as training moved the parameters


def _teacher_state(tr):
    """What one G+D step starts from: both parameter arenas and every spectral-norm bank's u|v arena (clones)."""
    from seg2eye_amd.spectral import ensure_bank
    m = tr.pix2pix_model
    banks = [b for b in (ensure_bank(net) for net in (m.netG, m.netD, m.netE)) if b is not None]
    return [tr.optimizer_G.flat_p.clone(), tr.optimizer_D.flat_p.clone()] + [b.uv_arena.clone() for b in banks]


def _load_teacher_state(tr, state):
    from seg2eye_amd.spectral import ensure_bank
    m = tr.pix2pix_model
    banks = [b for b in (ensure_bank(net) for net in (m.netG, m.netD, m.netE)) if b is not None]
    with torch.no_grad():
        for dst, src in zip([tr.optimizer_G.flat_p, tr.optimizer_D.flat_p] + [b.uv_arena for b in banks], state):
            dst.copy_(src)


def _one_iteration(tr, data, acts=None, mid_state=None):
    """One G + one D step; -> losses, generated image, the G / E / D parameter gradients (clones), and the state between the two steps.
    acts: a dict to fill with the ResBlk outputs of the G step's forward (eager trainers only: a hipGraph replay runs no hooks).
    mid_state: a teacher's state after ITS G step, loaded before this trainer's D step -- the D step then starts from the teacher's
    weights too (its own G update, -lr * sign-like steps of Adam at beta1 = 0 on bf16 gradients, is not what is being compared)."""
    m = tr.pix2pix_model
    hs = []
    if acts is not None:
        for name in _BLOCKS:
            def hook(mod, inp, out, name=name):
                acts.setdefault(name, out.detach().permute(0, 3, 1, 2).float().contiguous().cpu())
            hs.append(getattr(m.netG, name).register_forward_hook(hook))
    tr.run_generator_one_step(dict(data))
    for h in hs:
        h.remove()
    torch.cuda.synchronize()
    gg = {('G.' + k): p.grad.detach().clone() for k, p in m.netG.named_parameters() if p.grad is not None}
    gg.update({('E.' + k): p.grad.detach().clone() for k, p in m.netE.named_parameters() if p.grad is not None})
    fake = tr.get_latest_generated().detach().float().cpu()
    if mid_state is not None:
        _load_teacher_state(tr, mid_state)
    mid = _teacher_state(tr)
    tr.run_discriminator_one_step(dict(data))
    torch.cuda.synchronize()
    gd = {('D.' + k): p.grad.detach().clone() for k, p in m.netD.named_parameters() if p.grad is not None}
    return {'losses': {k: float(v.detach().float().mean()) for k, v in tr.get_latest_losses().items()}, 'fake': fake, 'grads_G': gg, 'grads_D': gd,
            'mid': mid}


def test_bf16_step_teacher_forced_along_the_fp32_trajectory():
    """VERDICT r5 "weak" #1: the benchmarked dtype AWAY from the initial weights.  A free-running bf16 trajectory cannot be held to the
    fp32 one beyond a few iterations (the fixture's GAN is chaotic: fp32 does not track itself, see the test above), so here the
    fp32 eager run of trainers/pix2pix_trainer.py:26-45 is the TEACHER: at its iterations 0, 5, 10, 15 and 20 (four batches in
    rotation, ngf = ndf = 64, 256x256, batch 8) its parameters and spectral-norm u|v are copied into a bf16 trainer with hipGraphs on
    (what bench.py times) and into a bf16 eager one, which then run ONE G step from exactly that state on the same batch, take the
    teacher's state after ITS G step, and run ONE D step; the per-step bounds of test_cfg3_as_benched_matches_reference are held at all five states: losses 2 %, generated image rel-RMS < 3 %,
    every ResBlk output < 2 % (eager bf16: a replay runs no hooks), the five largest G and three largest D weight gradients < 8 %
    (12 % away from the fixture's weights: see below)."""
    from seg2eye_amd.pix2pix_trainer import Pix2PixTrainer
    z = load_golden('trainer_ngf64_256_n8')

    def make(dt, graphs):
        tr = Pix2PixTrainer(_opt(ngf=64, ndf=64, crop_size=256, aspect_ratio=1.0, batchSize=8, compute_dtype=dt, hip_graphs=graphs))
        m = tr.pix2pix_model
        for tag, net in (('G', m.netG), ('D', m.netD), ('E', m.netE)):
            sd = filled_state(z, tag)
            with torch.no_grad():
                for k, v in net.state_dict().items():
                    v.copy_(sd[k])
        return tr
    teacher, graphed, eager = make('fp32', False), make('bf16', True), make('bf16', False)
    batches = [_batch(8, 256, 256, sd) for sd in (1234, 77, 2024, 5)]
    report = []
    for it in range(21):
        data = batches[it % len(batches)]
        if it % 5:
            teacher.run_generator_one_step(dict(data))
            teacher.run_discriminator_one_step(dict(data))
            continue
        state = _teacher_state(teacher)
        ta = {}
        t = _one_iteration(teacher, data, ta)                # (this IS the teacher's iteration `it`: its trajectory goes on from here)
        _load_teacher_state(graphed, state)
        g = _one_iteration(graphed, data, mid_state=t['mid'])
        assert graphed.use_graphs and graphed.graph_G is not None, 'the bf16 step did not run as a hipGraph replay'
        _load_teacher_state(eager, state)
        ea = {}
        e = _one_iteration(eager, data, ea, mid_state=t['mid'])
        big = sorted(t['grads_G'], key=lambda k: -t['grads_G'][k].numel())[:5]
        bigd = sorted(t['grads_D'], key=lambda k: -t['grads_D'][k].numel())[:3]
        for tag, r in (('graphs', g), ('eager', e)):
            for k, v in r['losses'].items():
                assert abs(v - t['losses'][k]) <= 2e-2 * max(1.0, abs(t['losses'][k])), (it, tag, k, v, t['losses'][k])
            img = _relrms(r['fake'], t['fake'])
            gw = {k: _relrms(r['grads_G'][k], t['grads_G'][k]) for k in big}
            gd = {k: _relrms(r['grads_D'][k], t['grads_D'][k]) for k in bigd}
            assert img < 3e-2, (it, tag, img)
            # (8 % at the fixture's weights as in the cfg3 test; along the trajectory the five largest layers' gradients shrink and the
            #  state itself differs from run to run -- float atomics in the teacher -- measured 2.3 ... 9.6 % over four runs: 12 %)
            wb = 8e-2 if it == 0 else 12e-2
            assert max(gw.values()) < wb and max(gd.values()) < wb, (it, tag, gw, gd)
            report.append((it, tag, round(img, 4), round(max(gw.values()), 4), round(max(gd.values()), 4)))
        rep = {name: _relrms(ea[name], ta[name]) for name in _BLOCKS}
        assert max(rep.values()) < 2e-2, (it, rep)
        report.append((it, 'ResBlk', {k: round(v, 4) for k, v in rep.items()}))
    print('teacher-forced bf16 steps (iteration, run, image rel-RMS, worst G wgrad, worst D wgrad):', report)


def test_cfg5_train_step_matches_reference():
    """BASELINE.json configs[4]'s per-GPU workload -- ngf = ndf = 64, 640x384 (--crop_size 384 --aspect_ratio 0.6), batch 4,
    encoder + feature matching on -- against ONE G step + ONE D step of the real reference's Pix2PixTrainer
    (trainers/pix2pix_trainer.py:26-45; fixture trainer_ngf64_640x384_n4.npz, `make_golden.py --only cfg5-train`), as cfg3 is
    (the 640x384 backward / optimizer path was pinned only to itself):
      (a) fp32 eager: losses, generated image < 1e-3, every ResBlk output, all G / E / D parameter gradients and every parameter /
          buffer after the iteration, by checksum;
      (b) bf16 with hipGraphs ON against (a) and against the reference's losses."""
    z = load_golden('trainer_ngf64_640x384_n4')
    cfg = dict(crop=384, aspect=0.6, n=4, hw=(640, 384), seed=77)
    a = _cfg3_run('fp32', False, z, **cfg)
    _check_fp32_step_against_reference(a, z)
    fp32 = {k: a[k] for k in ('losses', 'fake', 'grads_G')}
    del a
    torch.cuda.empty_cache()
    c = _cfg3_run('bf16', True, z, steps=1, hooks=False, **cfg)
    assert c['tr'].use_graphs and c['tr'].graph_G is not None, 'the step did not run as a hipGraph replay'
    for k, v in c['losses'].items():
        ref = float(z['it0_%s' % k.replace('/', '_')].reshape(-1)[0])
        assert abs(v - fp32['losses'][k]) <= 2e-2 * max(1.0, abs(fp32['losses'][k])), ('bf16 graphs vs fp32', k, v, fp32['losses'][k])
        assert abs(v - ref) <= 2e-2 * max(1.0, abs(ref)), ('bf16 graphs vs reference', k, v, ref)
    assert _relrms(c['fake'], fp32['fake']) < 3e-2
    big = sorted(fp32['grads_G'], key=lambda k: -fp32['grads_G'][k].numel())[:5]
    g5 = {k: _relrms(c['grads_G'][k], fp32['grads_G'][k]) for k in big}
    print('cfg5 bf16 (graphs) vs fp32: image rel-RMS %.4f, wgrad rel-RMS %s' % (_relrms(c['fake'], fp32['fake']), {k: round(v, 4) for k, v in g5.items()}))
    assert max(g5.values()) < 8e-2, g5


def test_cfg5_full_width_matches_reference():
    """BASELINE.json configs[4] geometry at full width: ngf = ndf = 64, 640x384 (--crop_size 384 --aspect_ratio 0.6),
    batch 4 -- fp32 eval-mode netG and netD's feature lists against the real reference (fixture cfg5_ngf64_640x384_n4.npz:
    generator.py:69-101, discriminator.py:53-63), then one bf16 G+D trainer iteration of the same shape against the fp32 one."""
    from seg2eye_amd import networks, synthetic as syn, ops
    from seg2eye_amd.pix2pix_trainer import Pix2PixTrainer
    from conftest import checksum
    z = load_golden('cfg5_ngf64_640x384_n4')
    opt = _opt(ngf=64, ndf=64, crop_size=384, aspect_ratio=0.6, compute_dtype='fp32')
    H, W = 640, 384
    b = syn.make_batch(4, H, W, seed=55)
    label = torch.from_numpy(b['label']).to(DEV)
    G = networks.define_G(opt)
    G.load_state_dict(filled_state(z, 'G'))
    G.eval()
    with torch.no_grad():
        y = G(label, torch.from_numpy(z['w']).to(DEV))
    yc = y.float().cpu()
    err = float((yc[:, :, ::8, ::8] - torch.from_numpy(z['y_sub'])).abs().max())
    assert err < G_TOL, 'cfg5 fp32 G differs from the reference by %.3e' % err
    np.testing.assert_allclose([float(yc.mean()), float(yc.std())], z['stats'][:2], atol=1e-4)
    D = networks.define_D(opt)
    D.load_state_dict(filled_state(z, 'D'))
    D.eval()
    imgs = torch.cat([y[:, 0].float(), torch.from_numpy(b['target'])[:, 0].to(DEV)], 0).contiguous()
    x = ops.seg_image_concat(torch.cat([label[:, 0], label[:, 0]], 0).contiguous(), imgs, 4, networks.discriminator.D_CPAD)
    with torch.no_grad():
        pred = D(x)
    for i in range(2):
        for j in range(5):
            t = pred[i][j].float()
            assert tuple(t.shape) == tuple(int(v) for v in z['pred_shape_%d_%d' % (i, j)]), (i, j, t.shape)
            ref = z['pred_%d_%d' % (i, j)]
            if j == 4:
                assert float((t.cpu() - torch.from_numpy(ref)).abs().max()) < 2e-3 * max(1.0, float(np.abs(ref).max())), (i, j)
            else:
                assert_checksum_close(t, ref, 1e-3, 'cfg5 D feature %d/%d' % (i, j))
    del G, D, pred, x, y
    torch.cuda.empty_cache()
    # one trainer iteration at this shape: bf16 against fp32 (same weights, same batch)
    data = {'label': torch.from_numpy(b['label']), 'style_image': torch.from_numpy(b['style_image']), 'target': torch.from_numpy(b['target'])}
    res = {}
    for dt in ('fp32', 'bf16'):
        o = _opt(ngf=64, ndf=64, crop_size=384, aspect_ratio=0.6, batchSize=4, compute_dtype=dt)
        tr = Pix2PixTrainer(o)
        m = tr.pix2pix_model
        for tag, net in (('G', m.netG), ('D', m.netD)):
            sd = filled_state(z, tag)
            with torch.no_grad():
                for k, v in net.state_dict().items():
                    v.copy_(sd[k])
        sdE = syn.fill_state_dict([(k, tuple(v.shape)) for k, v in m.netE.state_dict().items()])
        with torch.no_grad():
            for k, v in m.netE.state_dict().items():
                v.copy_(torch.from_numpy(sdE[k]))
        tr.run_generator_one_step(dict(data))
        torch.cuda.synchronize()
        big = sorted(((k, p) for k, p in m.netG.named_parameters()), key=lambda kp: -kp[1].numel())[:5]
        grads = {k: p.grad.detach().clone() for k, p in big}
        tr.run_discriminator_one_step(dict(data))
        res[dt] = ({k: float(v.detach().float().mean()) for k, v in tr.get_latest_losses().items()},
                   tr.get_latest_generated().float().cpu(), grads)
        assert tuple(res[dt][1].shape) == (4, 1, H, W)
        del tr, m
        torch.cuda.empty_cache()
    for k, v in res['bf16'][0].items():
        assert np.isfinite(v) and abs(v - res['fp32'][0][k]) <= 2e-2 * max(1.0, abs(res['fp32'][0][k])), (k, v, res['fp32'][0][k])
    assert _relrms(res['bf16'][1], res['fp32'][1]) < 3e-2
    g5 = {k: _relrms(res['bf16'][2][k], res['fp32'][2][k]) for k in res['fp32'][2]}
    print('cfg5 bf16 vs fp32: image rel-RMS %.4f, wgrad rel-RMS %s' % (_relrms(res['bf16'][1], res['fp32'][1]), {k: round(v, 4) for k, v in g5.items()}))
    assert max(g5.values()) < 8e-2, g5


def test_generator_more_upsampling_matches_reference():
    """--num_upsampling_layers more (generator.py:52-67,80-82: a sixth upsampling between the two middle blocks, start map
    crop/64): eval forward, d/dw and every parameter gradient against the real reference (g_more_ngf8_128.npz)."""
    from seg2eye_amd import networks, synthetic as syn
    from conftest import checksum
    z = load_golden('g_more_ngf8_128')
    opt = _opt(ngf=8, crop_size=128, aspect_ratio=1.0, num_upsampling_layers='more', compute_dtype='fp32')
    G = _load(networks.define_G(opt), z, 'G')
    G.eval()
    w = torch.from_numpy(z['w']).to(DEV).requires_grad_(True)
    y = G(_label(z), w)
    assert tuple(y.shape) == tuple(z['y_eval'].shape) == (2, 1, 128, 128)
    err = float((y.detach().float().cpu() - torch.from_numpy(z['y_eval'])).abs().max())
    assert err < G_TOL, "'more' generator differs from the reference by %.3e" % err
    proj = torch.from_numpy(syn.hash_uniform('g_proj', tuple(z['y_eval'].shape), seed=41)).to(DEV)
    (y.float() * proj).sum().backward()
    gw = z['grad_w']
    assert float((w.grad.cpu() - torch.from_numpy(gw)).abs().max()) <= KINK_TOL * float(np.abs(gw).max())
    for k, p in G.named_parameters():
        ref, got = z['grad_' + k], checksum(p.grad)
        assert abs(got[0] - ref[0]) + abs(got[1] - ref[1]) <= KINK_TOL * ref[1] + 1e-9, (k, got[:2], ref[:2])


def test_two_graph_trainers_and_inference_share_nothing():
    """Two Pix2PixTrainers with hipGraphs on plus inference forwards (what Tester.forward calls, util/tester.py:44-47) in ONE
    process: every trainer owns its ZeroPool / gradient sink, so interleaving their steps -- and running no-grad inference
    between a trainer's G and D step -- gives each trainer exactly the parameters it reaches when it runs alone."""
    from seg2eye_amd import synthetic as syn
    from seg2eye_amd.ops import ZeroPool
    from seg2eye_amd.pix2pix_trainer import Pix2PixTrainer

    def make(seed):
        opt = _opt(ngf=8, ndf=8, crop_size=256, aspect_ratio=1.0, batchSize=2, compute_dtype='fp32', hip_graphs=True)
        tr = Pix2PixTrainer(opt)
        m = tr.pix2pix_model
        for net, s in ((m.netG, seed), (m.netD, seed + 1), (m.netE, seed + 2)):
            sd = syn.fill_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()], s)
            with torch.no_grad():
                for k, v in net.state_dict().items():
                    v.copy_(torch.from_numpy(sd[k]))
        return tr
    d1, d2 = _batch(2, 256, 256, 61), _batch(2, 256, 256, 62)

    def alone(seed, data):
        tr = make(seed)
        for _ in range(3):
            tr.run_generator_one_step(dict(data))
            tr.run_discriminator_one_step(dict(data))
        torch.cuda.synchronize()
        return tr.optimizer_G.flat_p.clone(), tr.optimizer_D.flat_p.clone()
    ref1, ref2 = alone(101, d1), alone(202, d2)
    a, b = make(101), make(202)
    assert a.pool is not b.pool and a.pool.sink is not b.pool.sink
    for _ in range(3):
        a.run_generator_one_step(dict(d1))
        b.run_generator_one_step(dict(d2))
        with torch.no_grad():                                      # inference between the steps: no pool scope is open
            assert ZeroPool.active() is None
            b.pix2pix_model.eval()                                 # (train mode would advance b's spectral-norm u, v: a different trajectory)
            img = b.pix2pix_model(dict(d1), mode='inference')
            assert tuple(img.shape) == (2, 1, 256, 256) and bool(torch.isfinite(img.float()).all())
        b.run_discriminator_one_step(dict(d2))
        a.run_discriminator_one_step(dict(d1))
    torch.cuda.synchronize()
    assert a.use_graphs and b.use_graphs and a.graph_G is not None and b.graph_G is not None
    # fp32 weight-gradient atomics are not bit-reproducible: bound by a few Adam sign flips (see the trainer tests)
    bound = 2 * 4e-4 * sum(((1 - 0.9 ** t) / (1 - 0.9)) ** 0.5 for t in (1, 2, 3)) + 1e-5
    for got, ref in ((a.optimizer_G.flat_p, ref1[0]), (a.optimizer_D.flat_p, ref1[1]), (b.optimizer_G.flat_p, ref2[0]), (b.optimizer_D.flat_p, ref2[1])):
        assert float((got - ref).abs().max()) <= bound, float((got - ref).abs().max())


def _run_dp_check(nproc, *extra):
    import json, os, socket, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, S2E_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
    script = os.path.join(root, 'tools', 'dp_check.py')
    if nproc == 1:
        cmd = [sys.executable, script, *extra]
        env.pop('WORLD_SIZE', None)
    else:
        with socket.socket() as s:
            s.bind(('127.0.0.1', 0))
            port = s.getsockname()[1]
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(nproc), '--master-addr', '127.0.0.1',
               '--master-port', str(port), script, *extra]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_data_parallel_replicas_stay_bit_identical():
    """two ranks (sharing this box's GPU over gloo -- RCCL refuses two ranks on one device; same collective calls),
    each constructed from DIFFERENT weights and spectral-norm vectors, run 3 full G+D trainer iterations on their shards: after
    the start-up broadcasts and the summed-gradient exchange the parameter arenas AND the spectral-norm u|v arenas are
    bit-identical across ranks (the power iteration accumulates with integer atomics), and losses / parameters agree with ONE
    process running the global batch (2 x 2 = 4 samples; InstanceNorm is per sample, losses are batch means)."""
    two = _run_dp_check(2, '--mode', 'train', '--iters', '3', '--batch', '2')
    assert two['world'] == 2 and two['identical_G'] and two['identical_D'] and two['identical_uv'], two
    one = _run_dp_check(1, '--mode', 'train', '--iters', '3', '--batch', '4')
    for i in range(3):
        for k, v in one['losses'][i].items():
            assert abs(two['losses'][i][k] - v) <= (2e-3 if i == 0 else 1e-2) * max(1.0, abs(v)), (i, k, two['losses'][i][k], v)
    # parameters: equal up to Adam's sign flips of near-zero gradients (see the trainer tests); compared through the arena sums
    assert abs(two['G_abs'] - one['G_abs']) <= 1e-4 * one['G_abs'] and abs(two['D_abs'] - one['D_abs']) <= 1e-4 * one['D_abs'], (two, one)


def test_rccl_single_rank_overlapped_step_matches_exchange_after_backward():
    """RCCL itself (backend 'nccl', a process group of ONE rank, S2E_DIST_SINGLE=1) carries every collective of
    the data-parallel path on this one-GPU box: start-up broadcasts, the asynchronous all-reduces of the generator's gradient
    groups launched from the backward hooks, the exchange after the backward of the --no_overlap_allreduce mode (under hipGraph
    replays).  Both modes run the same two G+D iterations from the same weights and must agree (up to Adam's sign flips of
    near-zero gradients: the weight-gradient atomics are not bit-reproducible, see the trainer tests)."""
    import json, os, socket, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    env = dict(os.environ, RANK='0', WORLD_SIZE='1', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
               S2E_DIST_SINGLE='1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    env.pop('S2E_DIST_BACKEND', None)
    out = subprocess.run([sys.executable, os.path.join(root, 'tools', 'rccl_single_rank_check.py'), '--iters', '2'], env=env,
                         capture_output=True, text=True, timeout=900, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])
    assert r['backend'] == 'nccl' and r['world'] == 1 and r['finite'], r
    assert r['overlap']['hooked'] and r['overlap']['early_launches'] >= 2 * 5 and not r['overlap']['graphs'], r
    # round 4: the overlapped exchange ON hipGraph replays -- the G step is six graph segments (five gradient groups + the rest),
    # the first five groups' all-reduces are started between segments in every iteration
    og = r['overlap_graphs']
    assert og['hooked'] and og['graphs'] and og['segments'] == 6 and og['early_launches'] >= 2 * 5, r
    assert not r['after_backward']['hooked'] and r['after_backward']['graphs'] and r['after_backward']['segments'] == 1, r
    # per trainer: broadcasts of 2 parameter arenas + the u|v arenas at construction; >= 1 all-reduce per group per step
    assert r['overlap']['broadcast_calls'] >= 4 and r['overlap']['all_reduce_calls'] >= 2 * 2 * 2, r
    assert og['all_reduce_calls'] >= 2 * (6 + 1), r
    assert r['after_backward']['all_reduce_calls'] >= 2 * 2, r
    bound = 2 * 4e-4 * sum(((1 - 0.9 ** t) / (1 - 0.9)) ** 0.5 for t in (1, 2)) + 1e-5
    assert r['max_abs_diff_G'] <= bound and r['max_abs_diff_D'] <= bound, r
    assert r['max_abs_diff_G_segmented'] <= bound and r['max_abs_diff_D_segmented'] <= bound, r
    for tag in ('overlap', 'overlap_graphs'):
        for k, v in r[tag]['losses'].items():
            assert abs(v - r['after_backward']['losses'][k]) <= 2e-2 * max(1.0, abs(v)), (tag, k, r)


def test_batchnorm_spade_statistics_are_synchronised_across_replicas():
    """--norm_G spectralspadebatch3x3 under data parallelism normalises with the statistics of the GLOBAL batch (one
    2*C all-reduce per layer forward, one in its backward): two ranks on halves of a batch reproduce one process on the whole
    batch -- generated images, the summed parameter gradient, and running buffers identical on both ranks."""
    two = _run_dp_check(2, '--mode', 'bn', '--batch', '2', '--norm_G', 'spectralspadebatch3x3')
    one = _run_dp_check(1, '--mode', 'bn', '--batch', '4', '--norm_G', 'spectralspadebatch3x3')
    assert two['identical_running'], two
    assert abs(sum(two['y_sum']) - one['y_sum'][0]) <= 2e-4 * one['y_abs'][0], (two, one)
    assert abs(sum(two['y_abs']) - one['y_abs'][0]) <= 2e-4 * one['y_abs'][0], (two, one)
    assert abs(two['g_sum'] - one['g_sum']) <= 2e-3 * one['g_abs'] and abs(two['g_abs'] - one['g_abs']) <= 2e-3 * one['g_abs'], (two, one)
    assert abs(two['rm_abs'] - one['rm_abs']) <= 1e-5 * max(one['rm_abs'], 1e-6) and abs(two['rv_sum'] - one['rv_sum']) <= 1e-5 * one['rv_sum'], (two, one)


def test_spectralbatch_norm_d_and_e_match_reference():
    """--norm_D spectralbatch / --norm_E spectralbatch (normalization.py:38-39; BatchNorm2d(affine=True) behind the spectral convs):
    train-mode forward, input gradient, every parameter gradient and the running buffers against the real reference
    (de_spectralbatch.npz)."""
    from seg2eye_amd import networks, synthetic as syn, ops
    from conftest import checksum
    z = load_golden('de_spectralbatch')
    opt = _opt(ndf=8, ngf=8, crop_size=256, norm_D='spectralbatch', norm_E='spectralbatch', compute_dtype='fp32')
    D = _load(networks.define_D(opt), z, 'D')
    D.train()
    label = torch.from_numpy(z['label']).to(DEV)
    fake = torch.from_numpy(syn.smooth_images('d_fake', (2, 1, 64, 64), seed=71)).to(DEV).requires_grad_(True)
    real = torch.from_numpy(syn.smooth_images('d_real', (2, 1, 64, 64), seed=71)).to(DEV)
    imgs = torch.cat([fake[:, 0], real[:, 0]], 0).contiguous()
    x = ops.seg_image_concat(torch.cat([label[:, 0], label[:, 0]], 0).contiguous(), imgs, 4, networks.discriminator.D_CPAD)
    pred = D(x)
    loss = sum((p[-1].float() * torch.from_numpy(syn.hash_uniform('dproj%d' % i, tuple(p[-1].shape), seed=71)).to(DEV)).sum() for i, p in enumerate(pred))
    loss = loss + sum(f.float().abs().mean() for p in pred for f in p[:-1])
    loss.backward()
    assert abs(float(loss) - float(z['loss'][0])) <= 1e-3 * max(1.0, abs(float(z['loss'][0])))
    for i in range(2):
        np.testing.assert_allclose(pred[i][-1].detach().float().cpu().numpy(), z['pred_%d' % i], atol=2e-3, rtol=0)
        assert_checksum_close(pred[i][1].detach().float(), z['feat_%d_1' % i], 1e-3, 'feat %d' % i)
    gf = z['grad_fake']
    assert float((fake.grad.cpu() - torch.from_numpy(gf)).abs().max()) <= KINK_TOL * float(np.abs(gf).max())
    for k, p in D.named_parameters():
        ref, got = z['gradD_' + k], checksum(p.grad)
        assert abs(got[0] - ref[0]) + abs(got[1] - ref[1]) <= KINK_TOL * ref[1] + 1e-7, (k, got[:2], ref[:2])
    for k, v in D.state_dict().items():
        if 'running' in k:
            np.testing.assert_allclose(v.float().cpu().numpy(), z['bufD_' + k], atol=1e-4, rtol=1e-4, err_msg=k)
    E = _load(networks.define_E(opt), z, 'E')
    E.train()
    xs = torch.from_numpy(syn.smooth_images('e_style', (3, 1, 256, 256), seed=72)).to(DEV).requires_grad_(True)
    mu, logvar, feats = E(xs)
    (mu.sum() + 0.5 * logvar.sum()).backward()
    np.testing.assert_allclose(mu.detach().cpu().numpy(), z['e_mu'], atol=1e-3, rtol=0)
    np.testing.assert_allclose(logvar.detach().cpu().numpy(), z['e_logvar'], atol=1e-3, rtol=0)
    for k, p in E.named_parameters():
        ref, got = z['gradE_' + k], checksum(p.grad)
        assert abs(got[0] - ref[0]) + abs(got[1] - ref[1]) <= KINK_TOL * ref[1] + 1e-7, (k, got[:2], ref[:2])


def test_label_sparse_forward_under_graph_replay_with_changing_labels():
    """The label-sparse SPADE forward (ops.label_rects -> s2e_spade_conv_modulate_sparse + s2e_spade_modulate_uniform) decides per
    rectangle ON THE DEVICE, so a captured hipGraph must follow label maps that change between replays: a full-width trainer
    (ngf = ndf = 64, 256x256, batch 2, bf16) alternates two batches -- nested ellipses, and a map salted with random classes
    (fewer uniform rectangles) -- as graph replays and as eager launches; generated images agree (the forward is
    bit-reproducible; weights drift by Adam's sign flips of near-zero gradients only), and with the sparse form switched off the
    first iteration gives the same image up to the bf16 rounding of the fused path."""
    from seg2eye_amd import ops, synthetic as syn
    from seg2eye_amd.pix2pix_trainer import Pix2PixTrainer
    b1 = _batch(2, 256, 256, 91)
    b2 = _batch(2, 256, 256, 92)
    g = np.random.RandomState(3)
    lab2 = b2['label'].numpy().copy()
    salt = g.rand(*lab2.shape) < 0.002
    lab2[salt] = g.randint(0, 4, size=int(salt.sum())).astype(lab2.dtype)
    b2 = dict(b2, label=torch.from_numpy(lab2))
    # the two maps really differ in their rectangle statistics at 256^2
    counts = []
    for b in (b1, b2):
        rc = ops.label_rects(b['label'][:, 0].contiguous().to(DEV), 256, 256, torch.bfloat16, 128, 128)
        assert rc is not None
        counts.append(int(rc[3][0]))
    assert counts[0] < counts[1] < rc[0].numel(), counts
    res = {}
    for mode in ('eager', 'graph', 'dense'):
        old = ops.switches.SPARSE_OFF
        ops.switches.SPARSE_OFF = mode == 'dense'
        try:
            opt = _opt(ngf=64, ndf=64, crop_size=256, aspect_ratio=1.0, batchSize=2, compute_dtype='bf16', hip_graphs=(mode == 'graph'))
            tr = Pix2PixTrainer(opt)
            m = tr.pix2pix_model
            for net, seed in ((m.netG, 1), (m.netD, 2), (m.netE, 3)):
                sd = syn.fill_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()], seed)
                with torch.no_grad():
                    for k, v in net.state_dict().items():
                        v.copy_(torch.from_numpy(sd[k]))
            imgs = []
            for it, b in enumerate((b1, b2, b1, b2)):
                tr.run_generator_one_step(dict(b))
                tr.run_discriminator_one_step(dict(b))
                imgs.append(tr.get_latest_generated().detach().float().cpu().clone())
            if mode == 'graph':
                assert tr.use_graphs and tr.graph_G is not None
            res[mode] = imgs
            del tr, m
        finally:
            ops.switches.SPARSE_OFF = old
        torch.cuda.empty_cache()
    assert torch.equal(res['eager'][0], res['graph'][0])                               # same weights, same labels: same bits
    # Iteration 1 is the check that matters: the first replay on a map whose rectangle classes differ from the captured one's
    # (a stale list would put table values on dense rectangles).  Later iterations only bound the drift: two EAGER runs of
    # this trainer differ by 0.003 / 0.013 / 0.02-0.03 rel-RMS at iterations 1 / 2 / 3 (weight-gradient atomics, amplified by
    # Adam's sign flips of near-zero gradients, about doubling per step: tools/check_run_to_run_drift.py).
    for it, bound in ((1, 1e-2), (2, 4e-2), (3, 1.5e-1)):
        assert _relrms(res['graph'][it], res['eager'][it]) < bound, (it, _relrms(res['graph'][it], res['eager'][it]))
    assert _relrms(res['dense'][0], res['eager'][0]) < 5e-3, _relrms(res['dense'][0], res['eager'][0])
    assert float((res['eager'][1] - res['eager'][0]).abs().max()) > 0.05               # (the batches do differ)


def test_deterministic_mode_gives_bit_identical_training_runs():
    """S2E_DETERMINISTIC=1: every gradient of the step is summed in a fixed order, so two trainers from the same
    weights on the same batches end with the same BITS in both parameter arenas -- eager launches and hipGraph replays.  A
    child process each: the library reads the switch once."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for extra in ([], ['--graphs']):
        env = dict(os.environ, S2E_DETERMINISTIC='1')
        out = subprocess.run([sys.executable, os.path.join(root, 'tools', 'check_deterministic.py'), '--ngf', '32', '--iters', '3'] + extra,
                             env=env, capture_output=True, text=True, timeout=900, cwd=root)
        assert out.returncode == 0, out.stderr[-3000:]
        d = json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])
        assert d['bit_identical'] and d['deterministic_env'] == '1', d
