"""The segment-drop rule of the pre-pass (tests/seg_model.py) against a
brute-force check of every document: a document whose full fp32 score reaches
theta lies in a live sub-block of a tile that is not cut, every term lane
with a posting on a document of a live sub-block is kept, and so the scores
REST forms without the dropped segments are the full ones wherever they can
matter and never larger elsewhere."""
import numpy as np

import mask_model as mm
import seg_model as sm

TILE, SUB = mm.TILE, mm.SUB
N = 3 * TILE + 500            # a partial last tile
V = 48


def _index(rng):
    """Terms clustered in a few sub-blocks each (so sub-blocks do die), a few
    spread over every tile, one empty; f32 scores in (0.25, 4)."""
    cols = []
    for t in range(V):
        if t == 7:
            cols.append(np.zeros(0, np.int64))
            continue
        if t % 6 == 0:
            d = rng.choice(N, int(rng.integers(200, 900)), replace=False)
        else:
            blocks = rng.choice((N + SUB - 1) // SUB, int(rng.integers(1, 6)), replace=False)
            d = np.concatenate([b * SUB + rng.choice(SUB, int(rng.integers(1, 40)), replace=False)
                                for b in blocks])
            d = d[d < N]
        cols.append(np.unique(d))
    ip = np.zeros(V + 1, np.int64)
    ip[1:] = np.cumsum([len(d) for d in cols])
    ix = np.concatenate(cols).astype(np.int32)
    dt = rng.uniform(0.25, 4.0, len(ix)).astype(np.float32)
    return ip, ix, dt


def _scores(ip, ix, dt, row, keep=None):
    """fp32 sums in query order; keep bool [LANES, nt]: lane i adds only in
    the tiles where keep[i] holds."""
    acc = np.zeros(N, np.float32)
    for i, t in enumerate(row):
        if 0 <= t < V:
            d = ix[ip[t]:ip[t + 1]].astype(np.int64)
            v = dt[ip[t]:ip[t + 1]]
            if keep is not None:
                m = keep[i, d // TILE]
                d, v = d[m], v[m]
            np.add.at(acc, d, v)
    return acc


def test_drop_rule_against_every_document():
    rng = np.random.default_rng(5)
    ip, ix, dt = _index(rng)
    bmax, tmask = mm.tables(ip, ix, dt, N)
    nt = bmax.shape[1]
    dropped = total = 0
    for qi in range(24):
        row = rng.integers(0, V, 8).astype(np.int32)
        if qi % 4 == 1:
            row[3] = row[0]                      # a repeated term
        if qi % 4 == 2:
            row[[1, 5]] = [-1, V + 3]            # padding and an unknown id between terms
        if qi % 4 == 3:
            row[4:] = -1
        full = _scores(ip, ix, dt, row)
        top = np.sort(full)[::-1]
        for theta in (top[0], top[9], top[99], np.float32(top[0] * 0.5)):
            if not theta > 0:
                continue
            cut, L, drop = sm.live_model(bmax, tmask, row, theta)
            assert not drop[:, cut].any()
            docs = np.arange(N)
            tile, sb = docs // TILE, (docs % TILE) // SUB
            live = ~cut[tile] & (((L[tile] >> sb.astype(np.uint32)) & 1) == 1)
            # a document that reaches theta is in a live sub-block
            assert live[full >= theta].all(), (qi, theta)
            # every term with a posting on a document of a live sub-block is kept
            for i, t in enumerate(row):
                if 0 <= t < V:
                    d = ix[ip[t]:ip[t + 1]].astype(np.int64)
                    assert not drop[i, d[live[d]] // TILE].any(), (qi, i, theta)
            # ... so REST's sums are the full ones there, and never larger elsewhere
            kept = _scores(ip, ix, dt, row, keep=~drop & ~cut[None, :])
            assert np.array_equal(kept[live].view(np.uint32), full[live].view(np.uint32))
            assert (kept <= full).all() and (kept[~live] < theta).all()
            # a tile that is not cut keeps a non-empty segment
            n = sm.segment_postings(ip, ix, row, nt)
            assert ((n > 0) & ~drop)[:, ~cut].any(axis=0).all()
            # a repeated term: both lanes or neither
            if qi % 4 == 1:
                assert np.array_equal(drop[0], drop[3])
            dropped += int((drop & (n > 0)).sum())
            total += int((n[:, ~cut] > 0).sum())
    assert dropped * 10 > total, (dropped, total)   # the rule does drop segments here


def test_no_masks_no_theta_no_seg():
    rng = np.random.default_rng(6)
    ip, ix, dt = _index(rng)
    bmax, tmask = mm.tables(ip, ix, dt, N)
    row = np.array([0, 1, 2, 3, 6, 12, -1, -1], np.int32)
    theta = np.sort(_scores(ip, ix, dt, row))[::-1][3]
    for kw in (dict(use_mask=False), dict(seg=False)):
        cut, L, drop = sm.live_model(bmax, tmask, row, theta, **kw)
        assert not drop.any()
        assert np.array_equal(cut, mm.skip_model(bmax, tmask, row, theta, kw.get("use_mask", True))[1])
    cut, L, drop = sm.live_model(bmax, tmask, row, np.float32(0))
    assert not cut.any() and not L.any() and not drop.any()
