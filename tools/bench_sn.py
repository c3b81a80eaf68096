#!/usr/bin/env python3
"""Train-mode power iteration of the three banks, us per call and per iteration: the style encoder's (6 layers, 25 MB of fp32
weights) and the discriminator's at 1 and 16 iterations per call (the benchmark step runs the encoder's 8 at a time, one per style
image, pix2pix_model.py:280-290), the generator's (267 MB) at 1."""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from seg2eye_amd import networks, spectral
from seg2eye_amd.options import default_opt
dev = torch.device('cuda:0')
opt = default_opt(gpu_ids=[0], compute_dtype='bf16')
for name, net, its in (('E', networks.define_E(opt), (1, 16)), ('D', networks.define_D(opt), (1, 16)), ('G', networks.define_G(opt), (1,))):
    net = net.to(dev).train()
    bank = spectral.ensure_bank(net)
    for it in its:
        for _ in range(3): bank.step(True, it)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(20): bank.step(True, it)
        e.record(); torch.cuda.synchronize()
        mb = 4e-6 * sum(r * c for r, c in zip(bank.rows, bank.cols))
        print('%s bank (%d layers, %.1f MB), %2d iterations: %.1f us per call, %.1f us per iteration' % (
            name, bank.n, mb, it, s.elapsed_time(e) / 20 * 1e3, s.elapsed_time(e) / 20 / it * 1e3), flush=True)
