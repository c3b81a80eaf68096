"""Child of tests/test_ema_gpu.py::test_ema_scope_leaves_no_trace_in_training; run with S2E_DETERMINISTIC=1 (read when the
library loads).  Two trainers with identical state, one after the other, take two G+D steps; one of them then scores its averaged
weights -- an eval pass and a TRAIN-mode pass inside `ema_scope()` --; after one more G+D step the two must hold the same bits
in the parameter arenas of both optimizers, in the average and in every buffer.  argv: [compute dtype [norm_G]].
The second-moment arenas are compared too but only reported: two such runs differ there in the last bit of a few elements
(measured: 1 of 4.5 M) WITHOUT any scope (after the first two steps, fp32 and bf16: some gradient sum is not in a fixed order even under
S2E_DETERMINISTIC=1), which the parameters do not show -- at beta1 = 0 the update g / sqrt(v) barely depends on |g|.  Prints 'ema child ok' on success."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECOND_MOMENTS = ('G.flat_v', 'D.flat_v')
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    assert os.environ.get('S2E_DETERMINISTIC') == '1'
    from seg2eye_amd import synthetic as syn
    from seg2eye_amd.options import default_opt
    from seg2eye_amd.pix2pix_trainer import Pix2PixTrainer

    def batch(seed):
        b = syn.make_batch(2, 256, 256, seed=seed)
        return {'label': torch.from_numpy(b['label']), 'style_image': torch.from_numpy(b['style_image']),
                'target': torch.from_numpy(b['target'])}

    dtype = sys.argv[1] if len(sys.argv) > 1 else 'fp32'
    norm_G = sys.argv[2] if len(sys.argv) > 2 else 'spectralspadeinstance3x3'

    def nets(tr):
        m = tr.pix2pix_model
        return (m.netG, m.netD, m.netE)

    def trainer():
        tr = Pix2PixTrainer(default_opt(ngf=8, ndf=8, crop_size=256, aspect_ratio=1.0, batchSize=2, compute_dtype=dtype,
                                        norm_G=norm_G, gpu_ids=[0], ema_decay=0.9))
        with torch.no_grad():                                   # the same hash-filled parameters and buffers in both twins
            for net in nets(tr):
                sd = net.state_dict()
                filled = syn.fill_state_dict([(k, tuple(v.shape)) for k, v in sd.items()])
                for k, v in sd.items():
                    v.copy_(torch.from_numpy(filled[k]))
            tr.optimizer_G.flat_ema.copy_(tr.optimizer_G.flat_p)
        return tr

    def state(tr):
        """Clones of every arena and of every parameter and buffer."""
        og, od = tr.optimizer_G, tr.optimizer_D
        out = {'G.flat_p': og.flat_p, 'G.flat_v': og.flat_v, 'G.flat_ema': og.flat_ema, 'D.flat_p': od.flat_p, 'D.flat_v': od.flat_v}
        for tag, net in zip('GDE', nets(tr)):
            out.update({'%s.%s' % (tag, k): v for k, v in net.state_dict().items()})
        torch.cuda.synchronize()
        return {k: v.detach().clone() for k, v in out.items()}

    def step(tr, seed):
        tr.run_generator_one_step(batch(seed))
        tr.run_discriminator_one_step(batch(seed))

    def run(with_scope):
        """Three G+D steps; with_scope: the averaged weights are scored -- an eval and a TRAIN-mode pass -- after the second."""
        tr = trainer()
        states = [state(tr)]
        for s in (1, 2):
            step(tr, s)
        states.append(state(tr))
        if with_scope:
            m = tr.pix2pix_model
            with tr.ema_scope(), torch.no_grad():
                m.eval()
                m(batch(9), mode='inference')
                m.train()
                m(batch(9), mode='inference')
            states.append(state(tr))
        else:
            states.append(states[-1])
        step(tr, 3)
        states.append(state(tr))
        assert not torch.equal(tr.optimizer_G.flat_ema, tr.optimizer_G.flat_p)
        return states

    # one trainer after the other, as tools/check_deterministic.py runs its pair
    twin, scoped = run(False), run(True)
    for what, sa, sb in zip(('start', 'two steps (the runs must be reproducible for the comparison below to mean anything)',
                             'after the scope', 'one step after the scope'), twin, scoped):
        assert sorted(sa) == sorted(sb)
        for k in SECOND_MOMENTS:                                # (reported, not asserted: see the module docstring)
            n_diff = int((sa[k] != sb[k]).sum())
            if n_diff:
                print('%s: %s differs between the twins in %d of %d elements, max %.3e' % (what, k, n_diff, sa[k].numel(),
                                                                                         float((sa[k] - sb[k]).abs().max())))
        bad = [k for k in sa if k not in SECOND_MOMENTS and not torch.equal(sa[k], sb[k])]
        assert not bad, (what, bad[:8])
    print('ema child ok (%s, %s): three G+D steps' % (dtype, norm_G) + ', a scope with an eval and a train-mode pass after the second')


if __name__ == '__main__':
    main()
