"""The style reference ranking restated in numpy, for the tests of seg2eye_amd/ops/rank.py and seg2eye_amd/style_rank.py:
int64 distances, np.lexsort on (index, distance) for the selection, the producer's walk written a second time, and the label maps and
the store the tests rank.  Everything is integer, so every comparison against it is ==."""
import re

import numpy as np


def distances(targets, cands, metric='l2'):
    """(M, H, W), (K, H, W) uint8 -> int64 (M, K)."""
    t = np.asarray(targets).reshape(len(targets), -1)
    c = np.asarray(cands).reshape(len(cands), -1)
    out = np.empty((len(t), len(c)), dtype=np.int64)
    for m in range(len(t)):
        for k0 in range(0, len(c), 16):                      # (blocks of candidates: the int64 differences of a block, not of all)
            d = c[k0:k0 + 16].astype(np.int64) - t[m].astype(np.int64)[None, :]
            out[m, k0:k0 + 16] = (d * d).sum(axis=1) if metric == 'l2' else (d != 0).sum(axis=1)
    return out


def topk(dist, k, exclude=None):
    """dist (M, K) -> (idx, val) int32 (M, k): smallest (distance, index) first, the excluded candidate of a row left out, -1 tails."""
    dist = np.asarray(dist)
    M, K = dist.shape
    idx = np.full((M, k), -1, dtype=np.int32)
    val = np.full((M, k), -1, dtype=np.int32)
    for m in range(M):
        order = np.lexsort((np.arange(K), dist[m]))          # the last key is the primary one
        if exclude is not None and 0 <= int(exclude[m]) < K:
            order = order[order != int(exclude[m])]
        order = order[:k]
        idx[m, :len(order)] = order
        val[m, :len(order)] = dist[m][order]
    return idx, val


def clean(name):
    return re.sub(r'\.', '', name.decode('utf-8') if isinstance(name, bytes) else str(name))


def rank_styles(store, dataset_key, seg_store=None, top=100, metric='l2', use_seq=True):
    """The mapping seg2eye_amd.style_rank.rank_styles returns, from the rule alone."""
    out = {}
    for user, g in store[dataset_key].items():
        if dataset_key == 'test':
            names = [clean(n) for n in g['labels_gen_filenames']]
            targets = g['labels_gen']
            groups = [(b'g', g['labels_ss'], g.get('images_ss_filenames'))]
            if use_seq and seg_store is not None:
                groups.append((b's', seg_store['test'][user]['labels_pred_seq'], g.get('images_seq_filenames')))
        else:
            names = [clean(n) for n in g['images_ss_filenames']]
            targets = g['labels_ss']
            groups = [(b'g', seg_store[dataset_key][user]['labels_pred_gen'], g.get('images_gen_filenames'))]
            if use_seq:
                groups.append((b's', seg_store[dataset_key][user]['labels_pred_seq'], g.get('images_seq_filenames')))
        masks = np.concatenate([np.asarray(m) for _, m, _ in groups])
        subset = np.concatenate([np.full(len(m), s, dtype='S1') for s, m, _ in groups])
        cnames = [clean(n) if f is not None else None for _, m, f in groups for n in (f if f is not None else [None] * len(m))]
        d = distances(targets, masks, metric)
        ex = np.array([cnames.index(n) if n in cnames else -1 for n in names])
        idx, val = topk(d, top, ex)
        out[user] = {}
        for m, n in enumerate(names):
            sel = idx[m][idx[m] >= 0].astype(np.int64)
            out[user][n] = {'index': sel, 'subset': subset[sel], 'distance': val[m][idx[m] >= 0].astype(np.int32)}
    return {dataset_key: out}


def same_refs(a, b):
    """Two ranking mappings, compared key by key, value by value and dtype by dtype; -> the list of differences."""
    wrong = []
    if sorted(a) != sorted(b):
        return [('splits', sorted(a), sorted(b))]
    for s in a:
        if sorted(a[s]) != sorted(b[s]):
            wrong.append((s, 'users', sorted(a[s]), sorted(b[s])))
            continue
        for u in a[s]:
            if sorted(a[s][u]) != sorted(b[s][u]):
                wrong.append((s, u, 'files', sorted(a[s][u]), sorted(b[s][u])))
                continue
            for f in a[s][u]:
                x, y = a[s][u][f], b[s][u][f]
                if sorted(x.keys()) != sorted(y.keys()):
                    wrong.append((s, u, f, 'keys', sorted(x.keys()), sorted(y.keys())))
                    continue
                for k in x.keys():
                    p, q = np.asarray(x[k]), np.asarray(y[k])
                    if p.dtype != q.dtype or p.shape != q.shape or not np.array_equal(p, q):
                        wrong.append((s, u, f, k, p, q))
    return wrong


# ------------------------------------------------------------------------------------------------ data
def iid(n, H, W, ncls, seed):
    return np.random.RandomState(seed).randint(0, ncls, (n, H, W)).astype(np.uint8)


def eyes(n, H, W, ncls, seed):
    """Nested ellipses at jittered positions: class c sits inside class c - 1, the background is 0."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((n, H, W), dtype=np.uint8)
    for i in range(n):
        cy, cx = H * (0.5 + 0.15 * rng.uniform(-1, 1)), W * (0.5 + 0.15 * rng.uniform(-1, 1))
        ry, rx = max(0.5, H * (0.32 + 0.1 * rng.uniform(-1, 1))), max(0.5, W * (0.4 + 0.1 * rng.uniform(-1, 1)))
        for c in range(1, ncls):
            s = 1.0 - (c - 1) / float(ncls)
            out[i][((yy - cy) / (ry * s)) ** 2 + ((xx - cx) / (rx * s)) ** 2 <= 1.0] = c
    return out


def eye_store(seed=0, users=('U001', 'U002', 'U003'), n_ss=(3, 2, 4), n_gen=(5, 6, 5), n_seq=(2, 3, 2), H=640, W=400, keys=('train', 'test')):
    """-> (store, seg_store) in the layout of tests/test_cli.py's _fake_openeds_store, for 'train' and 'test', with blob masks: images are
    random bytes, every mask an `eyes` map.  images_gen_filenames names the generative frames; U001's generative frame 1 carries the
    name of U001's target 0, and in 'test' U001's labelled frame 2 the name of its target 1, so the file-name exclusion has work to do."""
    rng = np.random.RandomState(seed)
    store, seg = {}, {}
    for key in keys:
        store[key], seg[key] = {}, {}
        for ui, (u, n, ng, ns) in enumerate(zip(users, n_ss, n_gen, n_seq)):
            s = seed * 1000 + ui * 10 + (0 if key == 'train' else 5)
            ss_names = [('%s.%03d_ss' % (u, i)).encode() for i in range(n)]
            lg_names = [('%s_%03d_gen' % (u, i)).encode() for i in range(n)]
            gen_names = [('%s_g%03d' % (u, i)).encode() for i in range(ng)]
            if ui == 0:
                gen_names[1] = ss_names[0]
                if key == 'test':
                    ss_names[2] = lg_names[1]
            store[key][u] = {'images_ss': rng.randint(0, 256, (n, H, W)).astype(np.uint8),
                             'labels_ss': eyes(n, H, W, 4, s),
                             'images_gen': rng.randint(0, 256, (ng, H, W)).astype(np.uint8),
                             'images_seq': rng.randint(0, 256, (ns, H, W)).astype(np.uint8),
                             'labels_gen': eyes(n, H, W, 4, s + 1),
                             'images_ss_filenames': np.array(ss_names, dtype='S13'),
                             'labels_gen_filenames': np.array(lg_names, dtype='S13'),
                             'images_gen_filenames': np.array(gen_names, dtype='S13')}
            seg[key][u] = {'labels_pred_gen': eyes(ng, H, W, 4, s + 2), 'labels_pred_seq': eyes(ns, H, W, 4, s + 3)}
    return store, seg
