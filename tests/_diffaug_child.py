"""Child process of test_diffaug_gpu.test_identity_rows_leave_the_step_bit_for_bit, run with S2E_DETERMINISTIC=1 (the library reads the
switch once, when it loads).  Two trainers on the same filled weights and batch, fp32, eager: one without --diffaug, one with the full
policy whose sampler is patched to identity rows.  One G step and one D step each; compared bit for bit: netD's input and every tensor
netD returns (predictions and features) in both steps, the losses, both parameter arenas after both steps.

Why a child, and the one value that is not compared by its bits.  Without the switch the PARENT's weight gradients are summed with
float atomics: two trainers WITHOUT the flag already differ after their first Adam step (measured on an MI355X: 1 695 of 4.47 M
generator parameters, hence 127 002 of 131 072 pixels of the D step's fake, by up to 7.6e-6), so only the deterministic mode can show
that identity rows change nothing.  Even there the logged VALUE of GAN_Feat ends in one float atomic per block (loss_reduce_kernel:
up to 256 blocks in each of the 8 feature launches), in an order that varies from run to run: five trainers without the flag gave two
values one ulp apart in 3 of 15 bodies.  Its inputs -- every feature map, compared here by their bits -- and its gradient are
reproducible; the value itself is held to the reordering bound: at most 2 048 additions, each rounding by at most 2^-24 of the
(non-negative) running sum, for either order: |a - b| <= 2 * 2048 * 2^-24 * |a|."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
import test_diffaug_gpu as T                      # noqa: E402


def flat(x):
    if torch.is_tensor(x):
        return [x.detach().clone()] if x.numel() > 1 else []                        # (the G step also returns GAN_Feat's value: see above)
    if isinstance(x, (list, tuple)):
        return [t for y in x for t in flat(y)]
    return []


def run(flag):
    tr = T._trainer(diffaug=flag)
    m = tr.pix2pix_model
    ins, outs = [], []
    hooks = [T._hook_d_input(tr, ins), m.netD.register_forward_hook(lambda mod, args, out: outs.append(flat(out)))]
    tr.run_generator_one_step(dict(T._batch()))
    losses = T._losses(tr)
    tr.run_discriminator_one_step(dict(T._batch()))
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    assert m.diffaug_rows is None                                                   # nothing is handed over outside a step
    return {**losses, **T._losses(tr)}, ins, outs, (tr.optimizer_G.flat_p.clone(), tr.optimizer_D.flat_p.clone())


def main():
    assert os.environ.get('S2E_DETERMINISTIC') == '1'
    from seg2eye_amd import diffaug
    draws = []

    def identity_rows(policy, n, H, W, generator):
        draws.append(n)
        return diffaug.identity(n)
    diffaug.sample = identity_rows
    plain, aug = run(''), run(T.FULL)
    assert draws == [2, 2], draws                                                   # the flagged trainer drew once per step
    assert len(plain[1]) == len(aug[1]) == 2 and len(plain[2]) == len(aug[2]) == 2
    for step in (0, 1):
        assert torch.equal(T._bits(plain[1][step]), T._bits(aug[1][step])), 'netD input, step %d' % step
        assert len(plain[2][step]) == len(aug[2][step]) >= 8
        for i, (a, b) in enumerate(zip(plain[2][step], aug[2][step])):
            assert torch.equal(a, b), 'netD output %d, step %d' % (i, step)
    assert sorted(plain[0]) == sorted(aug[0]) == ['D/Fake', 'D/real', 'GAN', 'GAN_Feat']
    for k, a in plain[0].items():
        b = aug[0][k]
        print('%s: %.9g without the flag, %.9g with identity rows, bits %s' % (k, float(a), float(b), 'equal' if torch.equal(a, b) else 'DIFFERENT'))
        if k == 'GAN_Feat':
            assert abs(float(a) - float(b)) <= 2 * 2048 * 2.0 ** -24 * abs(float(a)), k
        else:
            assert torch.equal(a, b), k
    for tag, a, b in zip('GD', plain[3], aug[3]):
        assert torch.equal(a, b), 'parameters of optimizer %s after both steps' % tag
    print('diffaug child ok')


if __name__ == '__main__':
    main()
