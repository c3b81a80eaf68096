"""PyTorch-ROCm custom ops over the C-ABI kernels (include/seg2eye_hip.h).

torch is plumbing here: it owns device memory (caching allocator), the stream and
the autograd tape; every forward/backward body below is one or more HIP kernel
launches through ctypes on torch's current stream.  Internal activations are
NHWC-contiguous 4-D tensors (N, H, W, C) in the compute dtype (bf16 or fp32).

There is no CPU path: calling an op with a non-CUDA tensor raises.

One module per family (round 5; `ops.<name>` keeps resolving for every name, private helpers included):
  core      helpers, the memo of per-shape library queries, device job tables, LaunchProfiler, ZeroPool (the trainer step's scratch)
  sink      GradSink: the step's queues of deferred weight-side launches, one record type per queue
  conv      packs, conv2d / wgrad launchers, Conv2dFn, the encoder's FC head
  spade     statistics, label convs, the SPADE+Style block (fused, label-sparse), InstanceNorm
  resample  upsampling, resize, pooling, the discriminator's input plumbing
  losses    loss reductions, feature matching, Adam, the OpenEDS metric, SSIM and MS-SSIM, the region-aware error, the focal frequency loss
  preprocess  --device_preprocess: Pillow's bicubic resize and cv2's nearest resize of raw OpenEDS frames, `materialize`
  visual    the validation panels of the visualiser: five resized, normalised cells per sample as uint8 (`sidebyside_u8`)
  rank      style reference rankings: mask distances on the int8 matrix cores (`mask_distances`) and the k nearest per row (`rank_topk`)
  segment   the eye segmenter: softmax cross-entropy on NHWC logits, the uint8 mask of resized logits, the confusion matrix and its scores
  refine    the residual refiner: the network input of three uint8 planes, the loss on the challenge's error, the uint8 prediction
  mask_clean  the mask cleaner: connected components of label maps and the nearest-class fill (`ops.mask_clean` is the module)
  geometry  eye geometry: the integer moments of a mask's rim pixels (`rim_moments`) and the repaint from fitted conics (`ellipse_paint`)
  augment   the segmenter's paired augmentation: frames and label maps warped by one transform per pair (`augment_pairs`), `AugmentRule`
  switches  the experiment switches (environment)"""
from . import switches                                   # noqa: F401
from . import core, sink, conv, spade, resample, losses, preprocess, visual, rank, segment, refine, mask_clean, geometry, augment  # noqa: F401
from .._lib import (NORM_SPADE_STYLE_BATCH, NORM_ACCUMULATE_DX, ConvDesc, ACT_NONE, ACT_LRELU, ACT_TANH, AUX_NONE, AUX_RELU_MASK,      # noqa: F401
                    AUX_LRELU_GRAD, NORM_SPADE_STYLE, NORM_PLAIN_IN, LOSS_NEG_MEAN, LOSS_HINGE_REAL, LOSS_HINGE_FAKE, LOSS_L1)
from .. import _lib as L                                 # noqa: F401

for _m in (core, sink, conv, spade, resample, losses, preprocess, visual, rank, segment, refine, mask_clean, geometry, augment):
    for _k, _v in vars(_m).items():
        if not _k.startswith('__') and _k not in ('switches', 'core', 'sink', 'conv', 'spade', 'resample', 'losses', 'preprocess', 'visual', 'rank', 'segment', 'refine', 'mask_clean', 'geometry', 'augment'):
            globals().setdefault(_k, _v)
del _m, _k, _v
