"""numpy model of row_skip: the index's row presence masks (build_rowmask_
kernel and the heavy-slot table beside it) and the u16 word the pre-pass
writes per (query, tile, term lane), on top of tests/mask_model.py and
tests/seg_model.py.  Shared by tests/test_row_skip_model.py (CPU) and
tests/test_gpu_row_skip.py.

Rows are REST's double rows: for a segment [b, b + l) of absolute posting
indices, row r holds the postings p with (b & ~1) + 128 r <= p < (b & ~1) +
128 (r + 1); it has ((b & 1) + l + 127) >> 7 rows.  A term is heavy when one
of its segments has two or more rows; heavy terms take table slots in the
order of their document frequency (largest first, the lower id on a tie) while
the table's budget lasts.  A segment of more than ROWS rows stores all ones in
its ROWS entries, so its lane's word is 0xFFFF: every row runs."""
import numpy as np

import mask_model as mm
import seg_model as sm

TILE, SUB, LANES = mm.TILE, mm.SUB, mm.LANES
ROWS = 16                 # row entries of a (heavy term, tile)
ROW = 128                 # postings of a double row
ALL = 0xFFFF


def seg_rows(b, l):
    """Double rows of the segment [b, b + l)."""
    return 0 if l == 0 else ((b & 1) + l + ROW - 1) // ROW


def row_postings(b, l, r):
    """Postings of row r of the segment [b, b + l)."""
    lo = (b & 1) if r == 0 else 0
    hi = min(ROW, (b & 1) + l - ROW * r)
    return max(hi - lo, 0)


def segments(indptr, indices, t, nt):
    """(b int64 [nt], l int64 [nt]): term t's segment of every tile."""
    lo, hi = int(indptr[t]), int(indptr[t + 1])
    tiles = np.asarray(indices[lo:hi], np.int64) // TILE
    l = np.bincount(tiles, minlength=nt).astype(np.int64)
    b = lo + np.concatenate([[0], np.cumsum(l)[:-1]])
    return b, l


def row_tables(indptr, indices, n_docs, budget_bytes=256 << 20):
    """(hslot int32 [V], rowmask u32 [H, nt, ROWS])."""
    V = len(indptr) - 1
    nt = (n_docs + TILE - 1) // TILE
    heavy = []
    for t in range(V):
        b, l = segments(indptr, indices, t, nt)
        if any(seg_rows(int(bb), int(ll)) >= 2 for bb, ll in zip(b, l)):
            heavy.append(t)
    heavy.sort(key=lambda t: (-(int(indptr[t + 1]) - int(indptr[t])), t))
    heavy = heavy[:max(0, budget_bytes // (nt * ROWS * 4))] if nt else []
    hslot = np.full(V, -1, np.int32)
    rowmask = np.zeros((len(heavy), nt, ROWS), np.uint32)
    for h, t in enumerate(heavy):
        hslot[t] = h
        b, l = segments(indptr, indices, t, nt)
        for j in range(nt):
            bb, ll = int(b[j]), int(l[j])
            if seg_rows(bb, ll) > ROWS:
                rowmask[h, j] = 0xFFFFFFFF
                continue
            p = np.arange(bb, bb + ll)
            r = (p - (bb & ~1)) // ROW
            bit = np.uint32(1) << ((np.asarray(indices[bb:bb + ll], np.int64) % TILE) // SUB).astype(np.uint32)
            np.bitwise_or.at(rowmask[h, j], r, bit)
    return hslot, rowmask


def lane_words(bmax, tmask, hslot, rowmask, row, theta, use_mask=True, seg=True, rows=True):
    """u16 [LANES, nt] of one query row: 0 = the lane's segment is dropped
    (all eight: the tile is cut), 0xFFFF = every row runs, else bit r = row r
    runs."""
    V, nt = bmax.shape
    cut, L, drop = sm.live_model(bmax, tmask, row, theta, use_mask=use_mask, seg=seg)
    w = np.where(cut[None, :] | drop, 0, ALL).astype(np.uint16)
    if not (rows and seg and use_mask and np.float32(theta) > 0) or hslot is None:
        return w
    for i, t in enumerate(row[:LANES]):
        if 0 <= t < V and hslot[t] >= 0:
            live = (rowmask[hslot[t]] & L[:, None]) != 0                    # [nt, ROWS]
            bits = (live.astype(np.uint32) << np.arange(ROWS, dtype=np.uint32)).sum(axis=1)
            keep = w[i] != 0
            w[i, keep] = bits[keep].astype(np.uint16)
    return w


def kept_rows(w, b, l):
    """bool [rows of the segment]: the rows of [b, b + l) that run under the
    lane word w."""
    n = seg_rows(b, l)
    if w == ALL:
        return np.ones(n, bool)
    return np.array([(w >> r) & 1 == 1 for r in range(n)], bool)


def row_counts(indptr, indices, bmax, tmask, hslot, rowmask, queries, k, pooled,
               tile_mask=True, seg=True, rows=True, theta_of=None):
    """(rows dropped in kept segments, their postings, rows of the kept
    segments) of a search under the tile-bound threshold."""
    V, nt = bmax.shape
    drows = dposts = total = 0
    for row in queries:
        theta = theta_of(row) if theta_of else mm.theta_bound(bmax, row, k, pooled)
        w = lane_words(bmax, tmask, hslot, rowmask, row, theta, bool(tile_mask), bool(seg), bool(rows))
        for i, t in enumerate(row[:LANES]):
            if not 0 <= t < V:
                continue
            b, l = segments(indptr, indices, t, nt)
            for j in np.flatnonzero((w[i] != 0) & (l > 0)):
                bb, ll, ww = int(b[j]), int(l[j]), int(w[i, j])
                keep = kept_rows(ww, bb, ll)
                total += len(keep)
                for r in np.flatnonzero(~keep):
                    drows += 1
                    dposts += row_postings(bb, ll, int(r))
    return drows, dposts, total
