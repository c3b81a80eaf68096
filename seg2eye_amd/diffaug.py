"""Differentiable augmentation of the discriminator's input (--diffaug): the policy and the sampler of the parameter rows.

The transform itself is ops.d_input_aug (csrc/d_augment.hip); this module only draws its rows, on the host, from a CPU generator.
A row is 8 floats [b, c, ty, tx, y0, x0, ch, cw] (the last six integers, stored exactly) and serves one sample: its fake AND its real
image.  After DiffAugment (Zhao et al. 2020), for one-channel images:
  color        brightness b = u - 0.5 and contrast c = u' + 0.5, u, u' uniform in [0, 1): out = c * (v - mean(v)) + mean(v) + b.
               DiffAugment's saturation scales the distance from the channel mean; with ONE channel that distance is zero, so it
               is left out.
  translation  ty uniform integer in [-r_h, r_h], r_h = int(H / 8 + 0.5); tx likewise with W; pixels shifted in from outside are 0.
  cutout       a ch x cw = H // 2 x W // 2 rectangle of zeros whose centre (cy, cx) is uniform over the image's pixels:
               y0 = cy - ch // 2, x0 = cx - cw // 2 (the rectangle may stick out of the image).
A part that is off contributes its identity values (b = 0, c = 1, ty = tx = 0, an empty rectangle) and draws nothing.

Draw order (fixed: a seed reproduces a run): the enabled parts in the order color, translation, cutout; within a part one vector of
n draws per quantity, in the order b, c / ty, tx / cy, cx."""
import torch

PARTS = ('color', 'translation', 'cutout')
IDENTITY_ROW = (0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)


def parse_policy(text):
    """'color,translation,cutout' -> frozenset of the enabled parts ('' or None: empty = off).  An unknown name raises ValueError."""
    if isinstance(text, (set, frozenset)):
        names = list(text)
    else:
        names = [s.strip() for s in (text or '').split(',') if s.strip()]
    bad = [s for s in names if s not in PARTS]
    if bad:
        raise ValueError('--diffaug: unknown part(s) %s (known: %s)' % (sorted(bad), ', '.join(PARTS)))
    return frozenset(names)


def translation_range(size):
    return int(size / 8 + 0.5)


def identity(n):
    """(n, 8) fp32 rows that change nothing: ops.d_input_aug gives ops.d_input's bits."""
    return torch.tensor(IDENTITY_ROW, dtype=torch.float32).repeat(n, 1)


def sample(policy, n, H, W, generator):
    """(n, 8) fp32 CPU rows for one D forward of n samples of H x W, drawn from `generator` (a CPU torch.Generator)."""
    policy = parse_policy(policy)
    rows = identity(n)

    def ints(lo, hi):                                        # n uniform integers in [lo, hi]
        return torch.randint(lo, hi + 1, (n,), generator=generator).to(torch.float32)
    if 'color' in policy:
        rows[:, 0] = torch.rand(n, generator=generator) - 0.5
        rows[:, 1] = torch.rand(n, generator=generator) + 0.5
    if 'translation' in policy:
        rh, rw = translation_range(H), translation_range(W)
        rows[:, 2] = ints(-rh, rh)
        rows[:, 3] = ints(-rw, rw)
    if 'cutout' in policy:
        ch, cw = H // 2, W // 2
        cy, cx = ints(0, H - 1), ints(0, W - 1)
        rows[:, 4], rows[:, 5] = cy - ch // 2, cx - cw // 2
        rows[:, 6], rows[:, 7] = float(ch), float(cw)
    return rows
