"""EyeSegNet: the small encoder-decoder that predicts the masks `style_rank --seg_file` reads.  Not in the reference,
whose authors took those masks from a DeepLab outside the scope contract (refinenet/); built from this library's existing
ops only -- 3x3 convs with bias (pad 1), InstanceNorm + LeakyReLU(0.2), nearest 2x upsampling, skip connections as the convs' fused
residual -- with F = --nsf:

    e0 = IN.LReLU(conv(x, 1 -> F))                                                  H x W
    e1 = IN.LReLU(conv s2(e0, F -> 2F))    e2 = ...(2F -> 4F)    e3 = ...(4F -> 8F)       H/8 x W/8
    b  = IN.LReLU(conv(e3, 8F -> 8F))
    d2 = IN.LReLU(conv(up2x(b), 8F -> 4F) + e2)    d1 = ...(4F -> 2F) + e1    d0 = ...(2F -> F) + e0
    logits = conv(d0, F -> label_nc)                                                (N, H, W, label_nc), compute dtype"""
import torch.nn as nn

from .. import ops
from .. import packing
from .base_network import BaseNetwork, compute_dtype_of


class EyeSegNet(BaseNetwork):
    FILTERS_OPTION = 'nsf'

    @staticmethod
    def modify_commandline_options(parser, is_train):
        parser.add_argument('--nsf', type=int, default=32, help='# of filters of the segmenter\'s first conv layer (a multiple of 8)')
        return parser

    def __init__(self, opt, in_nc=1, out_nc=None, filters=None):
        """in_nc / out_nc / filters: the channels of the first conv's weight, of `out` and of e0 (default: 1, --label_nc, --nsf) -- what
        EyeRefineNet (networks/refiner.py) builds the same body with."""
        super().__init__()
        self.opt = opt
        self.cdtype = compute_dtype_of(opt)
        f = int(getattr(opt, 'nsf', 32) if filters is None else filters)
        if f < 8 or f % 8:
            raise ValueError('--%s must be a positive multiple of 8, got %d' % (self.FILTERS_OPTION, f))
        self.label_nc = int(getattr(opt, 'label_nc', 4))
        self.in_nc, self.out_nc = int(in_nc), int(self.label_nc if out_nc is None else out_nc)

        def conv(cin, cout):
            return nn.Conv2d(cin, cout, 3, padding=1)
        self.e0, self.e1, self.e2, self.e3 = conv(self.in_nc, f), conv(f, 2 * f), conv(2 * f, 4 * f), conv(4 * f, 8 * f)
        self.b = conv(8 * f, 8 * f)
        self.d2, self.d1, self.d0 = conv(8 * f, 4 * f), conv(4 * f, 2 * f), conv(2 * f, f)
        self.out = conv(f, self.out_nc)

    def forward(self, x):
        """x: (N, 1, H, W) fp32 in [-1, 1], H and W multiples of 8 -> logits (N, H, W, label_nc) NHWC in the compute dtype."""
        self.require_gpu(x)
        if x.dim() != 4 or x.shape[1] != 1 or x.shape[2] % 8 or x.shape[3] % 8:
            raise ValueError('EyeSegNet takes (N, 1, H, W) with H and W multiples of 8, got %s' % (tuple(x.shape),))
        return self.body(x.permute(0, 2, 3, 1).contiguous().to(self.cdtype))      # (N, H, W, 1): same memory order as NCHW

    def body(self, h):
        """h: (N, H, W, >= in_nc) NHWC in the compute dtype, H and W multiples of 8 -> (N, H, W, out_nc)."""
        def block(h, conv, stride=1, residual=None):
            return ops.instance_norm(ops.conv2d(h, conv.weight, conv.bias, residual, stride, 1), lrelu=True)
        with packing.network_scope(self, None):              # all weight packs of this forward: one launch
            e0 = block(h, self.e0)
            e1 = block(e0, self.e1, 2)
            e2 = block(e1, self.e2, 2)
            e3 = block(e2, self.e3, 2)
            b = block(e3, self.b)
            d2 = block(ops.upsample2x(b), self.d2, 1, e2)
            d1 = block(ops.upsample2x(d2), self.d1, 1, e1)
            d0 = block(ops.upsample2x(d1), self.d0, 1, e0)
            return ops.conv2d(d0, self.out.weight, self.out.bias, None, 1, 1)
