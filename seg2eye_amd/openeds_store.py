"""The OpenEDS store's layout and its files: the one place that knows the tree /{split}/{user}/{key} of prepare_openeds,
the masks /{split}/{user}/{labels_pred_gen, labels_pred_seq} of `segment predict` and the ranking /{split}/{user}/{file name}/{index,
subset, distance} of style_rank -- which keys a split uses, how a file name is cleaned, what a subset byte means, where a frame's mask
lives, how such a tree is saved and opened.  The dataset and the stages take it from here.  Host only: numpy, h5py where installed."""
import collections
import re

import numpy as np

STORE_DEPTH, REFS_DEPTH = 3, 4          # split/user/key and split/user/file name/key
SplitKeys = collections.namedtuple('SplitKeys', 'style_images labels filenames')


# ------------------------------------------------------------------------------------------------ the layout
def split_keys(dataset_key):
    """The keys of a split's style images, target masks and target file names: the test split's targets are the masks of the images
    to generate and its style images the labelled frames (reference data/openeds_dataset.py:44-52)."""
    if dataset_key == 'test':
        return SplitKeys('images_ss', 'labels_gen', 'labels_gen_filenames')
    return SplitKeys('images_gen', 'labels_ss', 'images_ss_filenames')


def clean_filename(name):
    """A stored file name as the dataset and the ranking name a target: decoded, dots removed (some names carry an additional dot)."""
    name = name.decode('utf-8') if isinstance(name, (bytes, np.bytes_)) else str(name)
    return re.sub(r'\.', '', name)


def pred_name(image_key):
    """'images_gen' -> 'labels_pred_gen': the name `segment predict` writes the masks of an image key under."""
    return image_key.replace('images_', 'labels_pred_', 1)


def candidate_parts(dataset_key, use_seq=True):
    """[(subset byte, image key)] in the order style_rank concatenates a person's candidates: a ranking's `index` counts through them."""
    return [(b'g', split_keys(dataset_key).style_images)] + ([(b's', 'images_seq')] if use_seq else [])


def candidate_row(group, dataset_key, index, subset):
    """The inverse of candidate_parts for one entry of a ranking -> (image key, row): b'g' is row `index` of the first part, b's' row
    `index` less the first part's length of `images_seq`.  group: the person's group of the store.  The row is not range-checked."""
    (g, first_key), (s, seq_key) = candidate_parts(dataset_key)
    if bytes(subset) == g:
        return first_key, index
    if bytes(subset) == s:
        return seq_key, index - (group[first_key].shape[0] if first_key in group else 0)
    raise ValueError('unknown subset %r of a style ranking (%r or %r)' % (bytes(subset), g, s))


def mask_source(store_group, seg_group, dataset_key, image_key):
    """Where the masks of a person's frames live -> (holder, mask key): the test split's labelled frames have their true `labels_ss` in the
    store, every other frame a predicted mask in the person's group of --seg_file (which may be None or lack the key: the caller's error)."""
    if dataset_key == 'test' and image_key == 'images_ss':
        return store_group, 'labels_ss'
    return seg_group, pred_name(image_key)


def rows_u8(rows):
    """[(dataset, row)] -> one stacked uint8 array; a dataset is a numpy array or an HDF5 dataset, which gives one row at a time."""
    return np.stack([np.asarray(d[int(i)], dtype=np.uint8) for d, i in rows])


# ------------------------------------------------------------------------------------------------ the files
def _holders(tree, depth, keys=()):
    """(keys, {name: array}) of every innermost mapping of a tree `depth` levels deep."""
    if depth == 1:
        yield keys, tree
    else:
        for k, v in tree.items():
            yield from _holders(v, depth - 1, keys + (k,))


def save_tree(tree, path, depth, chunk_images=False):
    """HDF5 at `path` when h5py is installed, else `path + '.npz'` with '/'-joined keys.  -> the path written.  chunk_images: the
    store's form -- one chunk per image for the 3-D arrays like the reference, and a group for a split without persons too."""
    try:
        import h5py
    except ImportError:
        np.savez(path + '.npz', **{'/'.join(keys + (k,)): v for keys, d in _holders(tree, depth) for k, v in d.items()})
        return path + '.npz'
    with h5py.File(path, 'w') as f:
        for split in tree if chunk_images else ():
            f.require_group(split)
        for keys, d in _holders(tree, depth):
            g = f.require_group('/'.join(keys))
            for k, v in d.items():
                g.create_dataset(k, data=v, chunks=((1,) + v.shape[1:] if v.ndim == 3 else True) if chunk_images else None)
    return path


def load_tree(path, depth):
    """The nested mapping of the .npz save_tree wrote; a key that is not `depth` levels deep is a ValueError."""
    z = np.load(path)
    tree = {}
    for key in z.files:
        *groups, name = key.split('/')
        if len(groups) != depth - 1:
            raise ValueError("%s: '%s' is not a key %d levels deep" % (path, key, depth))
        node = tree
        for g in groups:
            node = node.setdefault(g, {})
        node[name] = z[key]
    return tree


def open_tree(path, depth=STORE_DEPTH):
    """A store or a mask file (or with depth=REFS_DEPTH a ranking) for reading: the mapping of a `.npz`, otherwise the HDF5 file."""
    if path.endswith('.npz'):
        return load_tree(path, depth)
    import h5py
    return h5py.File(path, 'r')


def merge_splits(paths, opener):
    """The files of a comma-separated list as one mapping {split: ...}: style_rank and `segment predict` write one split per file."""
    merged = {}
    for p in (paths or '').split(','):
        if p:
            f = opener(p)
            merged.update({k: f[k] for k in f.keys()})
    return merged
