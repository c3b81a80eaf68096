"""The mask cleaner's rule (include/seg2eye_hip.h) restated in numpy, for the tests of seg2eye_amd/ops/mask_clean.py and
seg2eye_amd/mask_clean.py: components by minimum propagation over equal-label neighbours with pointer jumping until nothing changes, the
keep rules literally, the fill by brute force over the kept pixels at small sizes and by a column pass then a row pass in int64 at
large ones; and the label maps the tests clean.  Everything is integer, so every comparison against it is ==."""
import functools

import numpy as np

ALL, LARGEST, BORDER = 0, 1, 2
BRUTE_PIXELS = 1200                     # maps up to this many pixels are filled by brute force
BIG = np.iinfo(np.int64).max // 4


def default_modes(ncls):
    return (BORDER,) + (LARGEST,) * (ncls - 1)


def _offsets(conn):
    return [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if conn == 8 else [])


# ------------------------------------------------------------------------------------------------ components
def components(lab, ncls, conn):
    """lab (H, W) uint8 -> int64 (H, W): the smallest linear index of the pixel's component, -1 for a label >= ncls."""
    H, W = lab.shape
    valid = lab < ncls
    cur = np.where(valid, np.arange(H * W, dtype=np.int64).reshape(H, W), -1)
    while True:
        new = cur.copy()
        for dy, dx in _offsets(conn):                         # each pair of neighbours, both ways
            ya, yb = slice(0, H - dy), slice(dy, H)
            xa, xb = (slice(0, W - dx), slice(dx, W)) if dx >= 0 else (slice(-dx, W), slice(0, W + dx))
            same = valid[ya, xa] & valid[yb, xb] & (lab[ya, xa] == lab[yb, xb])
            m = np.minimum(new[ya, xa], new[yb, xb])
            new[ya, xa] = np.where(same, np.minimum(m, new[ya, xa]), new[ya, xa])     # (the two views overlap: only ever lower a value)
            new[yb, xb] = np.where(same, np.minimum(m, new[yb, xb]), new[yb, xb])
        flat = new.reshape(-1)
        named = cur.reshape(-1)[valid.reshape(-1)]             # the pixel a pixel named so far takes what the pixel has found: whole
        np.minimum.at(flat, named, flat[valid.reshape(-1)])    # pieces move at once, not one step of a winding chain per round
        while True:                                           # pointer jumping: a pixel takes the value of the pixel it names
            nxt = np.where(flat >= 0, flat[np.maximum(flat, 0)], -1)
            if np.array_equal(nxt, flat):
                break
            flat = nxt
        new = flat.reshape(H, W)
        if np.array_equal(new, cur):
            return cur
        cur = new


def components_bfs(lab, ncls, conn):
    """The same by a literal breadth-first search, for small maps."""
    H, W = lab.shape
    comp = -np.ones((H, W), dtype=np.int64)
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if conn == 8 else [])
    for y0 in range(H):
        for x0 in range(W):
            if lab[y0, x0] >= ncls or comp[y0, x0] >= 0:
                continue
            comp[y0, x0] = y0 * W + x0
            queue = [(y0, x0)]
            while queue:
                y, x = queue.pop()
                for dy, dx in steps:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < H and 0 <= xx < W and lab[yy, xx] == lab[y, x] and comp[yy, xx] < 0:
                        comp[yy, xx] = y0 * W + x0
                        queue.append((yy, xx))
    return comp


# ------------------------------------------------------------------------------------------------ what is kept
def kept_mask(lab, comp, ncls, modes):
    """-> (kept bool (H, W), found int64 (ncls,)): the keep rules, literally."""
    H, W = lab.shape
    kept = np.zeros((H, W), dtype=bool)
    found = np.zeros(ncls, dtype=np.int64)
    frame = np.zeros((H, W), dtype=bool)
    frame[0] = frame[-1] = True
    frame[:, 0] = frame[:, -1] = True
    for c in range(ncls):
        of_c = lab == c
        ids, areas = np.unique(comp[of_c], return_counts=True)          # ids ascending
        found[c] = len(ids)
        if not len(ids):
            continue
        if modes[c] == ALL:
            kept |= of_c
        elif modes[c] == LARGEST:
            kept |= of_c & (comp == ids[np.argmax(areas)])              # argmax: the first of equal areas, the smallest id
        elif modes[c] == BORDER:
            kept |= of_c & np.isin(comp, np.unique(comp[of_c & frame]))
        else:
            raise ValueError('mode %r' % (modes[c],))
    return kept, found


# ------------------------------------------------------------------------------------------------ the fill
def _fill_brute(lab, kept, ncls):
    H, W = lab.shape
    yy, xx = np.mgrid[0:H, 0:W]
    py, px = yy[~kept].astype(np.int64), xx[~kept].astype(np.int64)
    best = np.full(len(py), BIG, dtype=np.int64)
    cls = np.full(len(py), -1, dtype=np.int64)
    for c in range(ncls):
        m = kept & (lab == c)
        if not m.any():
            continue
        d2 = ((py[:, None] - yy[m][None, :]) ** 2 + (px[:, None] - xx[m][None, :]) ** 2).min(axis=1)
        upd = d2 < best                                                 # strictly: a tie stays with the lower class
        best[upd], cls[upd] = d2[upd], c
    return cls


def _fill_two_pass(lab, kept, ncls):
    H, W = lab.shape
    need_rows = np.nonzero((~kept).any(axis=1))[0]
    best = np.full((H, W), BIG, dtype=np.int64)
    cls = np.full((H, W), -1, dtype=np.int64)
    xs = np.arange(W, dtype=np.int64)
    dx2 = (xs[:, None] - xs[None, :]) ** 2
    for c in range(ncls):
        m = kept & (lab == c)
        if not m.any():
            continue
        g = np.full((H, W), BIG, dtype=np.int64)                        # column pass: the vertical distance to the class, down then up
        last = np.full(W, -1, dtype=np.int64)
        for y in range(H):
            last = np.where(m[y], y, last)
            g[y] = np.where(last >= 0, y - last, BIG)
        last = np.full(W, -1, dtype=np.int64)
        for y in range(H - 1, -1, -1):
            last = np.where(m[y], y, last)
            g[y] = np.minimum(g[y], np.where(last >= 0, last - y, BIG))
        g2 = np.where(g >= BIG, BIG, g * g)
        cols = np.nonzero(m.any(axis=0))[0]                             # (a column without the class holds BIG in every row)
        for r0 in range(0, len(need_rows), 16):                         # row pass: min over x' of (x - x')^2 + g(x')^2
            rows = need_rows[r0:r0 + 16]
            d2 = (dx2[None, :, cols] + g2[rows][:, None, cols]).min(axis=2)
            upd = d2 < best[rows]
            best[rows] = np.where(upd, d2, best[rows])
            cls[rows] = np.where(upd, c, cls[rows])
    return cls[~kept]


def clean(lab, ncls=4, conn=8, modes=None, brute=None):
    """lab (H, W) uint8 -> (out uint8 (H, W), stats int64 (ncls, 4), comp int64 (H, W))."""
    modes = default_modes(ncls) if modes is None else modes
    comp = components(lab, ncls, conn)
    kept, found = kept_mask(lab, comp, ncls, modes)
    out = lab.copy()
    stats = np.zeros((ncls, 4), dtype=np.int64)
    stats[:, 0] = found
    for c in range(ncls):
        stats[c, 1] = (lab == c).sum()
        stats[c, 2] = ((lab == c) & ~kept).sum()
    if kept.any() and not kept.all():
        brute = lab.size <= BRUTE_PIXELS if brute is None else brute
        cls = (_fill_brute if brute else _fill_two_pass)(lab, kept, ncls)
        out[~kept] = cls.astype(np.uint8)
    if kept.any():
        for c in range(ncls):
            stats[c, 3] = (out == c).sum()
    return out, stats, comp


def clean_batch(labels, ncls=4, conn=8, modes=None):
    """labels (N, H, W) -> (out uint8 (N, H, W), stats int32 (N, ncls, 4), comp int32 (N, H, W)), image by image."""
    res = [clean(l, ncls, conn, modes) for l in labels]
    return (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]).astype(np.int32), np.stack([r[2] for r in res]).astype(np.int32))


# ------------------------------------------------------------------------------------------------ data
def spiral(H, W):
    """A one-pixel-wide spiral of 1 on 0 from the top-left corner inwards: one component that winds through every tile."""
    a = np.zeros((H, W), dtype=np.uint8)
    y = x = d = turns = 0
    a[0, 0] = 1
    step = ((0, 1), (1, 0), (0, -1), (-1, 0))
    inside = lambda yy, xx: 0 <= yy < H and 0 <= xx < W
    while turns < 2:
        dy, dx = step[d]
        ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if inside(ny, nx) and not a[ny, nx] and (not inside(ay, ax) or not a[ay, ax]):
            y, x, turns = ny, nx, 0
            a[y, x] = 1
        else:
            d, turns = (d + 1) % 4, turns + 1
    return a


def serpentine(H, W):
    """Every second row full, joined alternately at the right and the left end: one component, the longest chain across tile borders."""
    a = np.zeros((H, W), dtype=np.uint8)
    a[0::2] = 1
    for y in range(1, H, 2):
        a[y, W - 1 if (y // 2) % 2 == 0 else 0] = 1
    return a


def rings(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return (np.minimum(np.minimum(yy, H - 1 - yy), np.minimum(xx, W - 1 - xx)) % 3).astype(np.uint8)


def specks(truth, seed, count=12):
    """truth (H, W) -> a copy with up to `count` square specks of another class or of 255.  Each speck's one-pixel-dilated footprint
    lies inside one true class and does not touch an earlier speck."""
    rng = np.random.RandomState(seed)
    H, W = truth.shape
    noisy = truth.copy()
    placed = tries = 0
    while placed < count and tries < 5000 and H >= 4 and W >= 4:
        tries += 1
        k = rng.randint(1, max(2, H // 16))
        if H - k - 1 <= 1 or W - k - 1 <= 1:
            continue
        y, x = rng.randint(1, H - k - 1), rng.randint(1, W - k - 1)
        reg = truth[y - 1:y + k + 1, x - 1:x + k + 1]
        if reg.min() != reg.max() or (noisy[y - 1:y + k + 1, x - 1:x + k + 1] != reg).any():
            continue
        noisy[y:y + k, x:x + k] = rng.choice([v for v in range(4) if v != int(reg[0, 0])] + [255])
        placed += 1
    return noisy


SEED = 5                                # the specks of the end-to-end tests: test_mask_clean_host.py checks them on the CPU


def speckled(truth, seed=None):
    """The truth tree of learnable_store with the specks of the issue's recovery fact, image by image."""
    seed = SEED if seed is None else seed
    out, k = {}, 0
    for split in truth:
        out[split] = {}
        for user in truth[split]:
            out[split][user] = {}
            for name, t in truth[split][user].items():
                out[split][user][name] = np.stack([specks(t[i], seed * 1000 + k + i) for i in range(len(t))])
                k += len(t)
    return out


PATTERNS = ('constant', 'iid4', 'iid2', 'spiral', 'serpentine', 'checkerboard', 'rings', 'all255', 'iid_ignore', 'eyes_specks')


@functools.lru_cache(maxsize=None)
def pattern(kind, shape, seed=0):
    """(N, H, W) uint8 of one of PATTERNS; the images of a batch differ where the pattern has a seed or an orientation."""
    from _style_rank_ref import eyes
    N, H, W = shape
    rng = np.random.RandomState(seed + 7919 * H + W)
    if kind == 'constant':
        out = np.stack([np.full((H, W), n % 4, dtype=np.uint8) for n in range(N)])
    elif kind == 'iid4':
        out = rng.randint(0, 4, shape).astype(np.uint8)
    elif kind == 'iid2':
        out = (rng.rand(*shape) < 0.59).astype(np.uint8)
    elif kind == 'spiral':
        out = np.stack([spiral(H, W) if n % 2 == 0 else spiral(H, W)[::-1, ::-1] for n in range(N)])
    elif kind == 'serpentine':
        out = np.stack([serpentine(H, W) if n % 2 == 0 else 1 - serpentine(H, W) for n in range(N)])
    elif kind == 'checkerboard':
        yy, xx = np.mgrid[0:H, 0:W]
        out = np.stack([((yy + xx + n) & 1).astype(np.uint8) for n in range(N)])
    elif kind == 'rings':
        out = np.stack([(rings(H, W) + n) % 3 for n in range(N)]).astype(np.uint8)
    elif kind == 'all255':
        out = np.full(shape, 255, dtype=np.uint8)
    elif kind == 'iid_ignore':
        out = rng.randint(0, 4, shape).astype(np.uint8)
        hole = rng.rand(*shape) < 0.25                           # a quarter of the pixels name no class: 16 ... 255
        out = np.where(hole, rng.randint(16, 256, shape), out).astype(np.uint8)
    elif kind == 'eyes_specks':
        truth = eyes(N, H, W, 4, seed + 11)
        out = np.stack([specks(truth[n], seed + n) for n in range(N)])
    else:
        raise ValueError(kind)
    out = np.ascontiguousarray(out)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(kind, shape, ncls, conn, modes=None, seed=0):
    """clean_batch of pattern(kind, shape, seed), computed once and shared (read-only)."""
    res = clean_batch(pattern(kind, shape, seed), ncls, conn, modes)
    for a in res:
        a.setflags(write=False)
    return res
