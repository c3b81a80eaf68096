"""Style reference rankings: the distances between target and candidate label maps (`mask_distances`, a byte GEMM on the
int8 matrix cores) and the k nearest candidates of every target (`rank_topk`).  Everything is integer: the results are exact."""
import torch

from .. import _lib as L
from .core import _need, _p, _stream

METRICS = {'l2': L.RANK_L2, 'mismatch': L.RANK_MISMATCH}


def _label_maps(targets, cands, metric):
    """The checks that need no device: they come first, as in _image_pair."""
    if metric not in METRICS:
        raise ValueError("metric 'l2' or 'mismatch' expected, got %r" % (metric,))
    for name, t in (('targets', targets), ('cands', cands)):
        if t.dtype != torch.uint8:
            raise ValueError('uint8 label maps expected, %s is %s' % (name, t.dtype))
        if t.dim() != 3:
            raise ValueError('%s: (n, H, W) expected, got %s' % (name, tuple(t.shape)))
    if targets.shape[1:] != cands.shape[1:]:
        raise ValueError('targets and cands of one H x W expected, got %s and %s' % (tuple(targets.shape[1:]), tuple(cands.shape[1:])))
    if targets.shape[0] < 1 or cands.shape[0] < 1 or targets[0].numel() < 1:
        raise ValueError('empty label maps: %s and %s' % (tuple(targets.shape), tuple(cands.shape)))


def _rows(t, P, pitch):
    """(n, H, W) -> the (n, pitch) rows the entry point reads.  With P a multiple of 16 (a real 640 x 400 mask is) that is the tensor
    itself; else the maps are copied into padded rows, whose padding stays uninitialised (the kernel never lets it count)."""
    if pitch == P:
        return t if t.data_ptr() % 16 == 0 else t.clone()
    rows = torch.empty((t.shape[0], pitch), dtype=torch.uint8, device=t.device)
    rows[:, :P] = t.reshape(t.shape[0], P)
    return rows


def mask_distances(targets, cands, ncls, metric='l2'):
    """targets (M, H, W), cands (K, H, W) uint8 label maps with values < ncls -> int32 (M, K):  'l2' sum_p (a - b)^2 (the reference's
    rule), 'mismatch' the number of pixels whose labels differ.  Exact; the same bits on every run."""
    _label_maps(targets, cands, metric)
    _need(targets, cands)
    M, K, P = targets.shape[0], cands.shape[0], targets.shape[1] * targets.shape[2]
    pitch = (P + 15) // 16 * 16
    a, b = _rows(targets, P, pitch), _rows(cands, P, pitch)
    dist = torch.empty((M, K), dtype=torch.int32, device=targets.device)
    L.call.s2e_mask_dist(_p(a), _p(b), M, K, P, pitch, int(ncls), METRICS[metric], _p(dist), _stream())
    return dist


def max_candidates():
    """Candidates one s2e_rank_topk launch takes (what fits a workgroup's LDS)."""
    return L.lib().s2e_rank_topk_max_candidates()


def _topk_launch(dist, k, exclude):
    M, K = dist.shape
    idx = torch.empty((M, k), dtype=torch.int32, device=dist.device)
    val = torch.empty((M, k), dtype=torch.int32, device=dist.device)
    L.call.s2e_rank_topk(_p(dist), M, K, k, _p(exclude), _p(idx), _p(val), _stream())
    return idx, val


def rank_topk(dist, k, exclude=None):
    """dist (M, K) int32 -> (idx, val), both (M, k) int32: per row the min(k, K') candidates of smallest (distance, index), distance
    ascending and ties to the lower index; unused slots hold -1.  exclude: None or (M,) integers, one candidate per row that is not
    returned (-1: none); K' counts the rest.
    Above the per-launch limit the row is ranked in chunks and the winners are ranked again, carrying their original indices.  A chunk's
    winners are in (distance, index) order and the chunks are in index order, so among equal distances a winner's POSITION orders like
    its index: ranking the winners by (distance, position) is ranking them by (distance, index).  The excluded candidate is taken out in
    the last pass only (the earlier ones keep one winner more), so every earlier slot is a real candidate."""
    if dist.dtype != torch.int32 or dist.dim() != 2 or dist.shape[0] < 1 or dist.shape[1] < 1:
        raise ValueError('int32 (M, K) distances expected, got %s %s' % (dist.dtype, tuple(dist.shape)))
    k = int(k)
    if k < 1:
        raise ValueError('k >= 1 expected, got %d' % k)
    if exclude is not None:
        if exclude.dtype not in (torch.int32, torch.int64) or tuple(exclude.shape) != (dist.shape[0],):
            raise ValueError('exclude: (M,) int32 or int64 expected, got %s %s' % (exclude.dtype, tuple(exclude.shape)))
    _need(dist, exclude)
    ex = None if exclude is None else exclude.to(torch.int32)
    limit = max_candidates()
    if dist.shape[1] <= limit:
        return _topk_launch(dist, k, ex)
    keep = k + (ex is not None)
    if 2 * keep > limit:
        raise ValueError('k = %d of %d candidates: above %d candidates k must stay below %d' % (k, dist.shape[1], limit, limit // 2))
    vals, orig = dist, None
    while vals.shape[1] > limit:
        vs, os_ = [], []
        for c0 in range(0, vals.shape[1], limit):
            chunk = vals[:, c0:c0 + limit].contiguous()
            i, v = _topk_launch(chunk, min(keep, chunk.shape[1]), None)
            i = i.long() + c0
            vs.append(v)
            os_.append(i if orig is None else orig.gather(1, i))
        vals, orig = torch.cat(vs, dim=1), torch.cat(os_, dim=1)
    pos_ex = None
    if ex is not None:
        hit = orig == ex[:, None].long()
        pos_ex = torch.where(hit.any(dim=1), hit.int().argmax(dim=1), torch.full_like(ex, -1, dtype=torch.int64)).to(torch.int32)
    pos, val = _topk_launch(vals, k, pos_ex)
    idx = torch.where(pos >= 0, orig.gather(1, pos.clamp(min=0).long()), torch.full_like(pos, -1, dtype=torch.int64)).to(torch.int32)
    return idx, val
