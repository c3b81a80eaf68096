"""EyeRefineNet: the network of the residual refiner.  The reference predicts its residual with a DeepLab
(refinenet/model.py), which is outside the scope contract; this is the body of EyeSegNet (networks/segmenter.py: e0..e3, b, d2..d0,
out; InstanceNorm + LeakyReLU, skips as the convs' fused residual) with F = --nrf, 3 input channels -- [the target mask in grey levels,
the reference frame, its mask in grey levels], what `ops.refine_input` writes -- and 1 output channel, the residual:

    x (N, H, W, >= 3) NHWC in the compute dtype, H and W multiples of 8 -> residual (N, H, W, 1)

It runs at the frames' own size (640 x 400): nothing is resized in this stage."""
from .segmenter import EyeSegNet


class EyeRefineNet(EyeSegNet):
    FILTERS_OPTION = 'nrf'

    @staticmethod
    def modify_commandline_options(parser, is_train):
        parser.add_argument('--nrf', type=int, default=32, help='# of filters of the refiner\'s first conv layer (a multiple of 8)')
        return parser

    def __init__(self, opt):
        super().__init__(opt, in_nc=3, out_nc=1, filters=getattr(opt, 'nrf', 32))

    def forward(self, x):
        self.require_gpu(x)
        if x.dim() != 4 or x.shape[3] < 3 or x.shape[1] % 8 or x.shape[2] % 8 or x.dtype != self.cdtype:
            raise ValueError('EyeRefineNet takes %s (N, H, W, >= 3) with H and W multiples of 8, got %s %s' % (self.cdtype, x.dtype, tuple(x.shape)))
        return self.body(x)
