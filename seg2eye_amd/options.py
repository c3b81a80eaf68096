"""Option namespace for the Seg2Eye hot path.

Mirrors the flag names and defaults the reference parses in
``options/base_options.py:21-64``, ``options/train_options.py:13-51``,
``models/networks/generator.py:15-20`` and
``models/networks/discriminator.py:16-28,69-72`` -- only the flags that shape
the G+D train step.  One deliberate difference: ``norm_G`` defaults to the
InstanceNorm variant (``spectralspadeinstance3x3``) because that is what the
hot path (BASELINE.json north_star) is defined on; the BatchNorm
SPADE variant is not built and asking for it raises.
"""
import argparse

_DEFAULTS = dict(
    name='seg2eye_amd', gpu_ids=[0], checkpoints_dir='./checkpoints', model='pix2pix',
    norm_G='spectralspadeinstance3x3', norm_D='spectralinstance', norm_E='spectralinstance',
    netG='spadestyle', netD='multiscale', netE='conv',
    batchSize=1, preprocess_mode='fixed', load_size=256, crop_size=256, aspect_ratio=1.0,
    label_nc=4, input_nc=1, output_nc=1, input_ns=4, semantic_nc=4,
    style_aggr_method='mean', style_sample_method='random',
    ngf=64, ndf=64, nef=16, w_dim=16, init_type='xavier', init_variance=0.02,
    isTrain=True, continue_train=False, which_epoch='latest',
    niter=14, niter_decay=7, optimizer='adam', beta1=0.5, beta2=0.999, lr=2e-4,
    D_steps_per_G=1, weight_decay=0.0,
    lambda_feat=10.0, lambda_vgg=10.0, lambda_l2=0.0, lambda_l1=0.0, lambda_openeds=0.0,
    lambda_kld=0.05, lambda_style_w=0.0, lambda_style_feat=0.0, lambda_gram=0.0,
    no_ganFeat_loss=False, no_vgg_loss=True, gan_mode='hinge', no_TTUR=False,
    num_upsampling_layers='normal', netD_subarch='n_layer', num_D=2, n_layers_D=4,
    # build-only knobs (no reference counterpart)
    compute_dtype='bf16',      # 'bf16' | 'fp32': storage + MFMA input type of the HIP path
    hip_graphs=False,          # capture zero_grad+forward+backward of each step into a hipGraph (fixed shapes)
    no_overlap_allreduce=False,  # data parallel: exchange all gradients after the backward instead of group by group during it
    grad_dtype='fp32',         # data parallel: what travels in the gradient exchange ('fp32' | 'bf16': half the bytes, distributed.FlatGradSync)
    grad_exchange='allreduce',  # 'allreduce' (the backend's all-reduce) | 'direct' (all-to-all + owner sum + all-gather over the xGMI mesh)
    ema_decay=0.0,             # > 0: exponential moving average of netG + netE's weights, kept by the Adam launch (optim.FlatAdam); 0 = off
    ema_start=0,               # optimizer steps during which the average just copies the weights (counted from a resume, like the moments)
    use_ema=False,             # test.py: load <epoch>_net_{G,E}_ema.pth instead of the live weights
    device_preprocess=False,   # openeds: the dataset hands out raw frames; resize / flip / normalise run on the GPU (ops.preprocess)
    visuals=False,             # train.py: loss_log.txt + side-by-side validation panels (seg2eye_amd/visualizer.py)
    grad_clip_norm=0.0,        # > 0: each optimizer's gradient is clipped to this global norm inside the Adam step (optim.FlatAdam); 0 = off
    skip_nonfinite_grads=False,  # a step whose gradient holds an inf / NaN changes nothing: parameters, moments, average, step count
    max_consecutive_skips=100,  # train.py stops after this many skipped steps in a row (0 = never); a policy default, not a measurement
    diffaug='',                # differentiable augmentation of D's input: parts of 'color,translation,cutout' (seg2eye_amd/diffaug.py); '' = off
    diffaug_seed=0,            # the sampler's CPU generator is seeded diffaug_seed + rank
    lambda_ssim=0.0,           # > 0: lambda_ssim * (1 - mean SSIM(fake, target)) joins the generator's loss (ops.ssim); 0 = off
    lambda_msssim=0.0,         # > 0: lambda_msssim * (1 - mean MS-SSIM(fake, target)) joins the generator's loss (ops.ms_ssim); 0 = off
    lambda_region=0.0,         # > 0: lambda_region * the class-balanced reconstruction error joins the generator's loss (ops.region_loss); 0 = off
    region_norm='l1',          # 'l1' | 'l2': the per-pixel error of that term
    region_weights='',         # 'w0,w1,...': one non-negative weight per label class (parse_region_weights); '' = all ones
    lambda_ffl=0.0,            # > 0: lambda_ffl * mean focal frequency loss(fake, target) joins the generator's loss (ops.focal_freq_loss); 0 = off
    ffl_alpha=1.0,             # the focal exponent of that term, in [0, 4]: a bin's weight is its spectral distance to the power alpha / 2, over the image's largest
)


def default_opt(**overrides):
    """Return an ``argparse.Namespace`` with the reference's field list
     and the given overrides."""
    d = dict(_DEFAULTS)
    unknown = set(overrides) - set(d)
    if unknown:
        raise KeyError('unknown option(s): %s' % sorted(unknown))
    d.update(overrides)
    d['semantic_nc'] = d['label_nc']          # options/base_options.py:150
    if isinstance(d['gpu_ids'], str):         # options/base_options.py:153-158
        d['gpu_ids'] = [int(s) for s in d['gpu_ids'].split(',') if int(s) >= 0]
    return argparse.Namespace(**d)


def parse_region_weights(text, label_nc):
    """--region_weights: exactly label_nc non-negative finite numbers separated by commas, at least one positive; '' = all ones.
    -> list of floats; anything else is a ValueError."""
    if text is None or str(text).strip() == '':
        return [1.0] * int(label_nc)
    try:
        ws = [float(t) for t in str(text).split(',')]
    except ValueError:
        raise ValueError("--region_weights '%s': numbers separated by commas expected" % text) from None
    if len(ws) != int(label_nc):
        raise ValueError("--region_weights '%s': %d weights for %d label classes" % (text, len(ws), label_nc))
    if not all(w >= 0.0 and w != float('inf') for w in ws):          # (a NaN fails w >= 0)
        raise ValueError("--region_weights '%s': every weight must be finite and not negative" % text)
    if not any(w > 0.0 for w in ws):
        raise ValueError("--region_weights '%s': at least one weight must be positive" % text)
    return ws


def latent_size(opt):
    """(sw, sh) of the generator's starting feature map,
    models/networks/generator.py:52-67 (python ``round`` = banker's)."""
    if opt.num_upsampling_layers == 'normal':
        n_up = 5
    elif opt.num_upsampling_layers == 'more':
        n_up = 6
    else:
        # 'most' is broken in the reference (generator.py:44-46)
        raise ValueError('opt.num_upsampling_layers [%s] not supported' % opt.num_upsampling_layers)
    sw = opt.crop_size // (2 ** n_up)
    sh = round(sw / opt.aspect_ratio)
    return sw, sh


def image_hw(opt):
    """Legal (H, W) of labels/images for this opt."""
    sw, sh = latent_size(opt)
    f = 32 if opt.num_upsampling_layers == 'normal' else 64
    return sh * f, sw * f


# ----------------------------------------------------------------------------------------- command line
# Every flag of the reference's TrainOptions / TestOptions parsers (options/base_options.py:21-64,
# options/train_options.py:13-51, options/test_options.py) with the reference's type and default -- checked against
# tests/golden/reference_option_defaults.json, which make_golden.py dumped from the real parsers -- plus the four
# model-specific flags added by modify_commandline_options and this build's own knobs.  One deliberate difference:
#   dataset_mode  default 'synthetic' (reference: 'openeds', the H5 dataset of SURVEY 8 f4, not built)
# (norm_G defaults to the reference's BatchNorm SPADE here; default_opt() -- the Python helper the benchmark and the
# parity tests use -- keeps the InstanceNorm variant the hot path is defined on)
_F, _I, _S = float, int, str
_CLI = [  # (name, type or 'flag', default, choices)
    ('name', _S, '', None), ('gpu_ids', _S, '0', None), ('checkpoints_dir', _S, './checkpoints', None), ('model', _S, 'pix2pix', None),
    ('norm_G', _S, 'spectralspadebatch3x3', None), ('norm_D', _S, 'spectralinstance', None), ('norm_E', _S, 'spectralinstance', None),
    ('batchSize', _I, 1, None),
    ('preprocess_mode', _S, 'fixed', ['resize_and_crop', 'crop', 'scale_width', 'scale_width_and_crop', 'scale_shortside',
                                       'scale_shortside_and_crop', 'fixed', 'none']),
    ('load_size', _I, 256, None), ('crop_size', _I, 256, None), ('aspect_ratio', _F, 0.8, None),
    ('label_nc', _I, 4, None), ('input_nc', _I, 1, None), ('output_nc', _I, 1, None), ('input_ns', _I, 4, None),
    ('dataroot', _S, None, None), ('dataset_mode', _S, 'synthetic', None), ('dataset_key', _S, 'train', None),
    ('serial_batches', 'flag', False, None), ('no_flip', 'flag', False, None), ('nThreads', _I, 0, None),
    ('load_from_opt_file', 'flag', False, None), ('seg_file', _S, '', None),
    ('style_ref', _S, 'datasets/0910_deeplab_top_image_indices_for_marcel.h5', None),
    ('style_aggr_method', _S, 'mean', ['mean', 'max']),
    ('style_sample_method', _S, 'random', ['random', 'first', 'ref_first', 'ref_random100']),
    ('netG', _S, 'spadestyle', None), ('netD', _S, 'multiscale', None), ('netE', _S, 'conv', None),
    ('ngf', _I, 64, None), ('ndf', _I, 64, None), ('nef', _I, 16, None), ('w_dim', _I, 16, None),
    ('init_type', _S, 'xavier', None), ('init_variance', _F, 0.02, None),
    ('validation_limit', _I, 250, None), ('write_error_log', 'flag', False, None),
    # model-specific (generator.py:15-20, discriminator.py:16-28,69-72)
    ('num_upsampling_layers', _S, 'normal', ['normal', 'more', 'most']), ('netD_subarch', _S, 'n_layer', None),
    ('num_D', _I, 2, None), ('n_layers_D', _I, 4, None),
    # build-only
    ('compute_dtype', _S, 'bf16', ['bf16', 'fp32']), ('hip_graphs', 'flag', False, None), ('no_hip_graphs', 'flag', False, None),
    ('no_overlap_allreduce', 'flag', False, None),
    ('grad_dtype', _S, 'fp32', ['fp32', 'bf16']), ('grad_exchange', _S, 'allreduce', ['allreduce', 'direct']),
    ('synthetic_size', _I, 64, None),        # samples per epoch of the synthetic dataset
    # the dataset's resize / flip / normalise as HIP launches on raw frames, bit-identical to the host path; off = host
    ('device_preprocess', 'flag', False, None),
    # validation also scores SSIM on the 640 x 400 uint8 pair the OpenEDS error sees (ops.ssim_u8): 'ssim/<key>/<mode>' in
    # the statistics (higher is better), `ssim` in the error log; off = validation as it was
    ('val_ssim', 'flag', False, None),
    # validation also scores five-level MS-SSIM on the same uint8 pair (ops.ms_ssim_u8): 'msssim/<key>/<mode>' in the statistics
    # (higher is better), `msssim` in the error log; off = validation as it was
    ('val_msssim', 'flag', False, None),
    # validation also takes the error apart by label class (ops.region_stats_u8 on the same uint8 pair):
    # 'region_mae/<key>/<mode>/<c>' and 'region_rmse/<key>/<mode>/<c>' in the statistics (grey levels), `region` in the error log
    ('val_regions', 'flag', False, None),
    # validation also scores the focal frequency loss, alpha = 1, on the same uint8 pair (ops.focal_freq_loss_u8): 'ffl/<key>/<mode>'
    # in the statistics (lower is better), `ffl` in the error log; off = validation as it was
    ('val_ffl', 'flag', False, None),
]
_CLI_TRAIN_BUILD = [
    ('ema_decay', _F, 0.0, None), ('ema_start', _I, 0, None),        # averaged generator weights; 0 = off
    # the visualiser: loss_log.txt, PNG panels at every quick validation, `visualisation` in the error log; off = none of it
    ('visuals', 'flag', False, None),
    # the gradient guard: clip by global norm, skip steps with non-finite gradients; off = the Adam step as it was
    ('grad_clip_norm', _F, 0.0, None), ('skip_nonfinite_grads', 'flag', False, None), ('max_consecutive_skips', _I, 100, None),
    # differentiable augmentation of the discriminator's input: 'color,translation,cutout' or a subset; '' = off
    ('diffaug', _S, '', None), ('diffaug_seed', _I, 0, None),
    # structural-similarity term of the generator's loss: lambda_ssim * (1 - mean SSIM(fake, target)); 'SSIM/raw' in the
    # loss log is the mean SSIM itself, so HIGHER is better (1 = identical); 0 = off, nothing is launched
    ('lambda_ssim', _F, 0.0, None),
    # multi-scale structural-similarity term of the generator's loss: lambda_msssim * (1 - mean MS-SSIM(fake, target)), five
    # levels with the published weights; 'MSSSIM/raw' in the loss log is the mean MS-SSIM itself, so HIGHER is better; 0 = off, nothing is launched
    ('lambda_msssim', _F, 0.0, None),
    # class-balanced reconstruction term of the generator's loss: every label class counts by its weight, not by its area;
    # 'region/raw' in the loss log is the term before lambda_region; 0 = off, nothing is launched
    ('lambda_region', _F, 0.0, None), ('region_norm', _S, 'l1', ['l1', 'l2']), ('region_weights', _S, '', None),
    # focal frequency term of the generator's loss: lambda_ffl * mean_n ffl[n](fake, target), the spectrum's squared distance with
    # every frequency weighted by how badly it is missed; 'FFL/raw' in the loss log is the mean before lambda, so LOWER is better; 0 = off,
    # nothing is launched
    ('lambda_ffl', _F, 0.0, None), ('ffl_alpha', _F, 1.0, None),
]
_CLI_TEST_BUILD = [
    ('use_ema', 'flag', False, None),                                 # score / generate with the averaged weights' checkpoint files
]
_CLI_TRAIN = [
    ('display_freq', _I, 5000, None), ('print_freq', _I, 500, None), ('save_latest_freq', _I, 5000, None),
    ('save_epoch_freq', _I, 1, None), ('full_val_freq', _I, 50000, None), ('no_html', 'flag', False, None), ('tf_log', 'flag', False, None),
    ('continue_train', 'flag', False, None), ('which_epoch', _S, 'latest', None),
    ('niter', _I, 14, None), ('niter_decay', _I, 7, None), ('optimizer', _S, 'adam', None),
    ('beta1', _F, 0.5, None), ('beta2', _F, 0.999, None), ('lr', _F, 0.0002, None), ('D_steps_per_G', _I, 1, None),
    ('weight_decay', _F, 0.0, None),
    ('lambda_feat', _F, 10.0, None), ('lambda_vgg', _F, 10.0, None), ('lambda_l2', _F, 0, None), ('lambda_l1', _F, 0, None),
    ('lambda_openeds', _F, 0, None), ('lambda_kld', _F, 0.05, None), ('lambda_style_w', _F, 0.0, None),
    ('lambda_style_feat', _F, 0.0, None), ('lambda_gram', _F, 0.0, None),
    ('no_ganFeat_loss', 'flag', False, None), ('no_vgg_loss', 'flag', True, None), ('gan_mode', _S, 'hinge', None), ('no_TTUR', 'flag', False, None),
]
_CLI_TEST = [
    ('results_dir', _S, 'results/', None), ('which_epoch', _S, 'latest', None), ('how_many', _I, float('inf'), None),
    ('produce_npy', 'flag', False, None),
]


def build_parser(is_train=True):
    ap = argparse.ArgumentParser(description='seg2eye_amd %s options (flag-compatible with the reference)' % ('train' if is_train else 'test'))
    for name, typ, default, choices in _CLI + (_CLI_TRAIN + _CLI_TRAIN_BUILD if is_train else _CLI_TEST + _CLI_TEST_BUILD):
        if not is_train and name in ('serial_batches', 'no_flip'):
            default = True                                 # options/test_options.py: parser.set_defaults(serial_batches=True, no_flip=True)
        if typ == 'flag':
            ap.add_argument('--' + name, action='store_true', default=default)
        else:
            ap.add_argument('--' + name, type=typ, default=default, choices=choices)
    return ap


def parse(argv=None, is_train=True):
    """argv -> option Namespace with the reference's post-processing (options/base_options.py:139-160)."""
    opt = build_parser(is_train).parse_args(argv)
    opt.isTrain = is_train
    opt.semantic_nc = opt.label_nc
    opt.gpu_ids = [int(s) for s in str(opt.gpu_ids).split(',') if s.strip() and int(s) >= 0]
    for k, v in _DEFAULTS.items():                      # fields the model reads that have no flag in this mode
        if not hasattr(opt, k):
            setattr(opt, k, v)
    if not is_train:
        opt.continue_train = False
    if opt.device_preprocess and (opt.dataset_mode != 'openeds' or opt.preprocess_mode != 'fixed'):
        raise ValueError("--device_preprocess needs --dataset_mode openeds and --preprocess_mode fixed (got '%s', '%s'): it restates "
                         "that dataset's host transform on the GPU" % (opt.dataset_mode, opt.preprocess_mode))
    if not 0.0 <= opt.ema_decay < 1.0 or opt.ema_start < 0:
        raise ValueError('--ema_decay must lie in [0, 1) (0 = off) and --ema_start must not be negative')
    if not opt.grad_clip_norm >= 0.0 or opt.max_consecutive_skips < 0:
        raise ValueError('--grad_clip_norm (0 = off) and --max_consecutive_skips (0 = never stop) must not be negative')
    if not 0.0 <= opt.ffl_alpha <= 4.0:                     # (a NaN fails both comparisons)
        raise ValueError('--ffl_alpha must lie in [0, 4] (got %r)' % (opt.ffl_alpha,))
    parse_region_weights(opt.region_weights, opt.label_nc)   # (a malformed list raises ValueError here, not at the first step)
    if opt.diffaug:
        from .diffaug import parse_policy
        parse_policy(opt.diffaug)                          # (an unknown part raises ValueError)
    # train.py replays each step as hipGraphs BY DEFAULT (round 4: the replayed step is 15 % faster than ~900 individual launches
    # on a slow host, and the overlapped gradient exchange replays graph segments); --no_hip_graphs launches eagerly.  A failed
    # capture falls back to eager launches by itself, a batch of another shape runs eagerly for that step.  (--hip_graphs is
    # accepted for command lines written before it became the default.)
    opt.hip_graphs = bool(is_train and not opt.no_hip_graphs)
    return opt
