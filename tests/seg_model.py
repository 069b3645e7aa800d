"""numpy model of the pre-pass's per-lane decisions (tile_skip_kernel with
seg_skip), on top of tests/mask_model.py and in its integer units: the live
mask L of every (query, tile) — bit s set iff the masked integer sum of
sub-block s exceeds MARGIN_INT, the compare whose maximum decides the cut —
and the drop rule: in a tile that is not cut, term lane t is dropped iff
(mk[t] & L) == 0.  Shared by tests/test_seg_skip_model.py (CPU) and
tests/test_gpu_seg_skip.py."""
import numpy as np

import mask_model as mm

TILE, SUB, LANES = mm.TILE, mm.SUB, mm.LANES


def live_model(bmax, tmask, row, theta, use_mask=True, seg=True):
    """(cut bool [nt], L u32 [nt], drop bool [LANES, nt]) of one query row
    under the threshold score theta.  cut is mask_model.skip_model's decision
    (asserted); L is 0 where the tile is cut by the whole-tile bound or there
    are no masks; drop is all False without masks, without seg, or without a
    positive theta — and in cut tiles (their byte is 0xFF: no lane runs)."""
    V, nt = bmax.shape
    theta = np.float32(theta)
    whole, cut = mm.skip_model(bmax, tmask, row, theta, use_mask=use_mask)
    L = np.zeros(nt, np.uint32)
    drop = np.zeros((LANES, nt), bool)
    if not theta > 0 or not use_mask:
        return cut, L, drop
    ub = np.zeros((LANES, nt), np.float32)
    mk = np.zeros((LANES, nt), np.uint32)
    for i, t in enumerate(row[:LANES]):
        if 0 <= t < V:
            ub[i] = mm._upper(bmax[t])
            mk[i] = tmask[t]
    with np.errstate(over="ignore", invalid="ignore"):
        K = np.float32(1048576.0) / theta
        scaled = np.fmin(ub * K, np.float32(2097152.0))
        c = np.where(mk != 0, np.ceil(scaled).astype(np.uint32) + np.uint32(1), np.uint32(0))
    for sb in range(32):
        acc = (((mk >> np.uint32(sb)) & np.uint32(1)) * c).sum(axis=0, dtype=np.uint32)
        L |= (acc > mm.MARGIN_INT).astype(np.uint32) << np.uint32(sb)
    L[whole] = 0
    assert np.array_equal(cut, whole | (L == 0))  # the cut is L == 0: the kernel's, the model's
    if seg:
        drop = ((mk & L[None, :]) == 0) & ~cut[None, :]
    return cut, L, drop


def segment_postings(indptr, indices, row, nt):
    """int64 [LANES, nt]: postings of each term lane's segment in each tile
    (0 for padding and unknown ids; a repeated term on each of its lanes)."""
    V = len(indptr) - 1
    n = np.zeros((LANES, nt), np.int64)
    for i, t in enumerate(row[:LANES]):
        if 0 <= t < V:
            tiles = np.asarray(indices[indptr[t]:indptr[t + 1]], np.int64) // TILE
            n[i] = np.bincount(tiles, minlength=nt)
    return n


def counts(indptr, indices, bmax, tmask, queries, k, pooled, tile_mask=True, seg=True,
           theta_of=None):
    """What the count_skips build reports for a search under the tile-bound
    threshold: (cut pairs, their postings, dropped non-empty segments of the
    scored tiles, their postings) and, last, the non-empty segments of the
    scored tiles (the share's denominator)."""
    nt = bmax.shape[1]
    pairs = posts = dsegs = dposts = segs = 0
    for row in queries:
        theta = theta_of(row) if theta_of else mm.theta_bound(bmax, row, k, pooled)
        cut, _, drop = live_model(bmax, tmask, row, theta, use_mask=bool(tile_mask), seg=bool(seg))
        n = segment_postings(indptr, indices, row, nt)
        pairs += int(cut.sum())
        posts += int(n[:, cut].sum())
        dsegs += int((drop & (n > 0)).sum())
        dposts += int(n[drop].sum())
        segs += int((n[:, ~cut] > 0).sum())
    return pairs, posts, dsegs, dposts, segs
