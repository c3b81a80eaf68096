"""The producer of `--style_ref`: "a pre-created similarity ranking of style images" (DESIGN 3.20).

The reference trains and tests with `--style_sample_method ref_first` / `ref_random100`, which read such a file, states its rule
("rank these images by their L2 distance to the target segmentation mask", refinenet/README.md) and ships neither the file nor a program
that writes one.  `rank_styles` writes the mapping `OpenEDSDataset(opt, style_refs=...)` reads:

    {dataset_key: {user: {filename: {'index': int64 (n,), 'subset': S1 (n,), 'distance': int32 (n,)}}}}

Per person: the TARGETS are the rows of the dataset's own label key (`labels_ss`; `labels_gen` for 'test'), named as the dataset names
them (decoded, dots removed).  The CANDIDATES are the person's style images (`images_gen`; `images_ss` for 'test'), subset b'g', followed
when `use_seq` by `images_seq`, subset b's', whose indices are offset by the number of the former: the order of
`openeds_store.candidate_parts`, which `openeds_store.candidate_row` undoes for the dataset and the refiner.  A candidate is compared
through its segmentation mask (`openeds_store.mask_source`):
  'test'                the style images are the labelled frames: their masks are the store's true `labels_ss`; the sequence frames join
                        only where `seg_store` holds their masks
  'train', 'validation' the generative and sequence frames are unlabelled (as they were for the reference's authors): their masks come
                        from `seg_store`: /{subset}/{user}/{labels_pred_gen, labels_pred_seq} uint8 (n, 640, 400), row-aligned with
                        the images -- what `python -m seg2eye_amd.segment predict` writes
A candidate whose file name equals the target's is excluded (where the store names the candidates: `<images key>_filenames`), so a
target is never its own style.  The distances (`ops.mask_distances`) and the selection (`ops.rank_topk`) run on the GPU; a person's
candidates are uploaded in chunks of at most UPLOAD_BYTES.

    python -m seg2eye_amd.segment predict --dataroot openeds.h5 --name seg --dataset_key train --out masks.h5
    python -m seg2eye_amd.style_rank --dataroot openeds.h5 --dataset_key train --seg_file masks.h5 --out style_refs.h5

`save_refs` / `load_refs` are openeds_store.save_tree / load_tree at the ranking's depth: HDF5 when h5py is installed, else `.npz` with
'/'-joined keys; the dataset reads a `--style_ref` that ends in `.npz` through `load_refs`."""
import argparse
import warnings

import numpy as np
import torch

from .openeds_store import REFS_DEPTH, candidate_parts, clean_filename, load_tree, mask_source, open_tree as _open, save_tree, split_keys

UPLOAD_BYTES = 1 << 30                  # candidate masks on the device at a time


def _names(group, key):
    return [clean_filename(n) for n in np.asarray(group[key])] if key in group else None


def _candidates(store, seg_store, dataset_key, user, use_seq):
    """-> [(subset byte, masks (n, H, W) array-like, cleaned names or None)] in the order of openeds_store.candidate_parts.  The test
    split's sequence frames join only where seg_store holds their masks; in the other splits every part needs its predicted masks."""
    g, test = store[dataset_key][user], dataset_key == 'test'
    if test and 'labels_ss' not in g:
        raise ValueError("rank_styles('test'): %s has no labels_ss -- the masks of its style images (images_ss)" % user)
    if not test and seg_store is None:
        raise ValueError("rank_styles('%s'): the generative and sequence frames of this split are unlabelled -- pass seg_store, the "
                         "masks a segmentation network predicts for them: /%s/<user>/{labels_pred_gen, labels_pred_seq} uint8 "
                         "(n, 640, 400), row-aligned with images_gen / images_seq" % (dataset_key, dataset_key))
    seg = None if seg_store is None else seg_store[dataset_key][user]
    parts = []
    for subset, image_key in candidate_parts(dataset_key, use_seq):
        holder, mask_key = mask_source(g, seg, dataset_key, image_key)
        if not test or (holder is not None and mask_key in holder):
            parts.append((subset, holder[mask_key], _names(g, image_key + '_filenames')))
    for (_, masks, _), (_, key) in zip(parts, candidate_parts(dataset_key, use_seq)):
        if not test and masks.shape[0] != g[key].shape[0]:
            raise ValueError('%s/%s: %d predicted masks for %d %s' % (dataset_key, user, masks.shape[0], g[key].shape[0], key))
    return parts


def _distances(targets, parts, ncls, metric, device):
    """(M, K) int32 on `device`: the candidates of `parts` go up in chunks of at most UPLOAD_BYTES."""
    from .ops import rank as R
    t = torch.from_numpy(np.ascontiguousarray(targets, dtype=np.uint8)).to(device)
    per = max(1, UPLOAD_BYTES // max(1, int(np.prod(t.shape[1:]))))
    cols = []
    for _, masks, _ in parts:
        for c0 in range(0, masks.shape[0], per):
            c = torch.from_numpy(np.ascontiguousarray(masks[c0:c0 + per], dtype=np.uint8)).to(device)
            cols.append(R.mask_distances(t, c, ncls, metric))
    return torch.cat(cols, dim=1)


def rank_styles(store, dataset_key, seg_store=None, top=100, metric='l2', use_seq=True, ncls=4, device='cuda'):
    from .ops import rank as R
    _, label_key, key_filenames = split_keys(dataset_key)
    out, short = {}, []
    for user in store[dataset_key].keys():
        g = store[dataset_key][user]
        out[user] = {}
        if key_filenames not in g:                           # (the dataset counts no samples for such a person)
            continue
        names = _names(g, key_filenames)
        parts = [p for p in _candidates(store, seg_store, dataset_key, user, use_seq) if p[1].shape[0] > 0]
        if not names or not parts:
            continue
        subset = np.concatenate([np.full(p[1].shape[0], p[0], dtype='S1') for p in parts])
        cand_names = [n for p in parts for n in (p[2] if p[2] is not None else [None] * p[1].shape[0])]
        where = {}
        for i, n in enumerate(cand_names):
            if n is not None:
                where.setdefault(n, i)
        exclude = np.array([where.get(n, -1) for n in names], dtype=np.int32)
        dist = _distances(g[label_key], parts, ncls, metric, device)
        idx, val = R.rank_topk(dist, top, torch.from_numpy(exclude).to(device))
        idx, val = idx.cpu().numpy(), val.cpu().numpy()
        for m, n in enumerate(names):
            keep = idx[m] >= 0
            sel = idx[m][keep].astype(np.int64)
            out[user][n] = {'index': sel, 'subset': subset[sel], 'distance': val[m][keep].astype(np.int32)}
        if min((len(e['index']) for e in out[user].values()), default=top) < top:
            short.append(user)
    if short:
        warnings.warn('%d person(s) have fewer than top = %d style candidates (%s%s): --style_sample_method ref_random%d indexes %d entries'
                      % (len(short), top, ', '.join(short[:5]), ', ...' if len(short) > 5 else '', top, top))
    return {dataset_key: out}


# ------------------------------------------------------------------------------------------------ the file
def save_refs(refs, path):
    """HDF5 at `path` when h5py is installed, else `path + '.npz'` with '/'-joined keys (as prepare_openeds.save_store).  -> the path written."""
    return save_tree(refs, path, REFS_DEPTH)


def load_refs(path):
    """The nested mapping OpenEDSDataset(opt, style_refs=...) takes, from the .npz save_refs wrote."""
    return load_tree(path, REFS_DEPTH)


def main(argv=None):
    ap = argparse.ArgumentParser(description='Write the --style_ref ranking of an OpenEDS store.')
    ap.add_argument('--dataroot', required=True, help='the store prepare_openeds wrote (.h5, or .npz without h5py)')
    ap.add_argument('--dataset_key', default='train', choices=['train', 'validation', 'test'])
    ap.add_argument('--seg_file', default=None, help='predicted masks of the unlabelled frames, /{subset}/{user}/{labels_pred_gen, labels_pred_seq}: the file '
                                                     '`python -m seg2eye_amd.segment predict --out` writes')
    ap.add_argument('--top', type=int, default=100, help='entries kept per target (ref_randomN needs N)')
    ap.add_argument('--rank_metric', default='l2', choices=['l2', 'mismatch'])
    ap.add_argument('--no_seq', action='store_true', help='rank the generative frames only')
    ap.add_argument('--out', required=True)
    a = ap.parse_args(argv)
    refs = rank_styles(_open(a.dataroot), a.dataset_key, seg_store=_open(a.seg_file) if a.seg_file else None, top=a.top,
                       metric=a.rank_metric, use_seq=not a.no_seq)
    print('style ranking of %d persons written to %s' % (len(refs[a.dataset_key]), save_refs(refs, a.out)))


if __name__ == '__main__':
    main()
