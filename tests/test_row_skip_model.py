"""The row rule of the pre-pass (tests/row_model.py) against a brute-force
check of every document: a document whose full fp32 score reaches theta lies
in a kept row of a kept lane for every term it holds, so the sums REST forms
from the kept rows alone are the full ones wherever they can matter, bit for
bit, and never larger elsewhere."""
import numpy as np

import mask_model as mm
import row_model as rm
import seg_model as sm

TILE, SUB, LANES = mm.TILE, mm.SUB, mm.LANES
N = 3 * TILE + 500            # a partial last tile
V = 24


def _index(rng):
    """Heavy terms in runs of consecutive documents (several rows per tile,
    most of them far from the light terms), light terms clustered in a few
    sub-blocks, one empty; f32 scores in (0.25, 4)."""
    cols = []
    for t in range(V):
        if t == 7:
            d = np.zeros(0, np.int64)
        elif t % 4 == 0:
            runs = [np.arange(s, min(N, s + int(rng.integers(150, 1900))))
                    for s in rng.choice(N, int(rng.integers(1, 4)), replace=False)]
            d = np.concatenate(runs)
        else:
            blocks = rng.choice((N + SUB - 1) // SUB, int(rng.integers(1, 6)), replace=False)
            d = np.concatenate([b * SUB + rng.choice(SUB, int(rng.integers(1, 40)), replace=False)
                                for b in blocks])
        cols.append(np.unique(d[d < N]))
    ip = np.zeros(V + 1, np.int64)
    ip[1:] = np.cumsum([len(d) for d in cols])
    ix = np.concatenate(cols).astype(np.int32)
    dt = rng.uniform(0.25, 4.0, len(ix)).astype(np.float32)
    return ip, ix, dt


def _kept_postings(ip, ix, t, w_lane, nt):
    """bool [df]: the postings of term t that lie in rows its lane's words keep."""
    b, l = rm.segments(ip, ix, t, nt)
    keep = np.zeros(int(ip[t + 1] - ip[t]), bool)
    for j in range(nt):
        bb, ll, ww = int(b[j]), int(l[j]), int(w_lane[j])
        if ll == 0 or ww == 0:
            continue
        rows = rm.kept_rows(ww, bb, ll)
        p = np.arange(bb, bb + ll)
        keep[p - int(ip[t])] = rows[(p - (bb & ~1)) // rm.ROW]
    return keep


def _scores(ip, ix, dt, row, words=None, nt=0):
    """fp32 sums in query order; words u16 [LANES, nt]: lane i adds only the
    postings of the rows its words keep."""
    acc = np.zeros(N, np.float32)
    for i, t in enumerate(row):
        if 0 <= t < V:
            d = ix[ip[t]:ip[t + 1]].astype(np.int64)
            v = dt[ip[t]:ip[t + 1]]
            if words is not None:
                m = _kept_postings(ip, ix, t, words[i], nt)
                d, v = d[m], v[m]
            np.add.at(acc, d, v)
    return acc


def test_row_rule_against_every_document():
    rng = np.random.default_rng(11)
    ip, ix, dt = _index(rng)
    bmax, tmask = mm.tables(ip, ix, dt, N)
    nt = bmax.shape[1]
    hslot, rowmask = rm.row_tables(ip, ix, N)
    assert (hslot[::4] >= 0).all() and rowmask.shape == (int((hslot >= 0).sum()), nt, rm.ROWS)
    # a term's row masks add up to its tile mask
    for t in np.flatnonzero(hslot >= 0):
        b, l = rm.segments(ip, ix, t, nt)
        small = np.array([rm.seg_rows(int(x), int(y)) <= rm.ROWS for x, y in zip(b, l)])
        assert np.array_equal(np.bitwise_or.reduce(rowmask[hslot[t]], axis=1)[small], tmask[t][small])
    drows = total = 0
    for qi in range(24):
        row = rng.integers(0, V, 8).astype(np.int32)
        row[0] = 4 * int(rng.integers(0, V // 4))        # a heavy term on lane 0
        if qi % 4 == 1:
            row[3] = row[0]                              # ... twice
        if qi % 4 == 2:
            row[[1, 5]] = [-1, V + 3]                    # padding and an unknown id between terms
        if qi % 4 == 3:
            row[4:] = -1
        full = _scores(ip, ix, dt, row)
        top = np.sort(full)[::-1]
        for theta in (top[0], top[9], top[99], np.float32(top[0] * 0.5)):
            if not theta > 0:
                continue
            cut, L, drop = sm.live_model(bmax, tmask, row, theta)
            w = rm.lane_words(bmax, tmask, hslot, rowmask, row, theta)
            assert np.array_equal(w == 0, drop | cut[None, :])      # rows never drop a lane
            docs = np.arange(N)
            tile, sb = docs // TILE, (docs % TILE) // SUB
            live = ~cut[tile] & (((L[tile] >> sb.astype(np.uint32)) & 1) == 1)
            assert live[full >= theta].all()
            # every posting on a document of a live sub-block is in a kept row
            for i, t in enumerate(row):
                if 0 <= t < V:
                    d = ix[ip[t]:ip[t + 1]].astype(np.int64)
                    assert _kept_postings(ip, ix, t, w[i], nt)[live[d]].all(), (qi, i, theta)
            # ... so REST's sums are the full ones there, bit for bit, and never larger elsewhere
            kept = _scores(ip, ix, dt, row, words=w, nt=nt)
            assert np.array_equal(kept[live].view(np.uint32), full[live].view(np.uint32))
            assert (kept <= full).all() and (kept[~live] < theta).all()
            hit = full >= theta
            assert np.array_equal(kept[hit].view(np.uint32), full[hit].view(np.uint32))
            # a tile that is not cut keeps a row
            n = sm.segment_postings(ip, ix, row, nt)
            assert ((n > 0) & (w != 0))[:, ~cut].any(axis=0).all()
            if qi % 4 == 1:
                assert np.array_equal(w[0], w[3])
            # without the option, the masks or the segment bits: only 0 and 0xFFFF
            for kw in (dict(rows=False), dict(seg=False), dict(use_mask=False)):
                w0 = rm.lane_words(bmax, tmask, hslot, rowmask, row, theta, **kw)
                assert np.isin(w0, (0, rm.ALL)).all()
        c = rm.row_counts(ip, ix, bmax, tmask, hslot, rowmask, row[None, :], 10, False,
                          theta_of=lambda r: top[9])
        drows += c[0]
        total += c[2]
    assert drows * 10 > total, (drows, total)            # the rule does drop rows here
    w = rm.lane_words(bmax, tmask, hslot, rowmask, row, np.float32(0))
    assert (w == rm.ALL).all()                           # no positive theta: every row runs


def test_hand_made_rows():
    """Row numbering: an odd start shifts the rows by one posting and a full
    tile then takes 17 rows; entries past a segment's rows stay zero."""
    assert [rm.seg_rows(b, l) for b, l in ((0, 0), (0, 1), (0, 128), (1, 128), (0, 2048), (1, 2048))] == \
        [0, 1, 1, 2, 16, 17]
    assert rm.row_postings(1, 128, 0) == 127 and rm.row_postings(1, 128, 1) == 1
    assert sum(rm.row_postings(3, 1000, r) for r in range(rm.seg_rows(3, 1000))) == 1000
    # term 0: one posting (so term 1 starts odd); term 1: a whole tile; term 2: 130 postings
    cols = [np.array([5]), np.arange(TILE), np.r_[np.arange(64, 64 + 129), 1999]]
    ip = np.zeros(4, np.int64)
    ip[1:] = np.cumsum([len(c) for c in cols])
    ix = np.concatenate(cols).astype(np.int32)
    hslot, rowmask = rm.row_tables(ip, ix, TILE)
    assert list(hslot) == [-1, 0, 1]
    assert (rowmask[0, 0] == 0xFFFFFFFF).all()           # 17 rows: all ones
    # term 2 starts at posting 2049 (odd): row 0 holds 127 postings (docs 64..190: sub-blocks
    # 1, 2), row 1 the last three (docs 191, 192: sub-blocks 2, 3; doc 1999: sub-block 31)
    assert list(rowmask[1, 0][:3]) == [0b110, (1 << 2) | (1 << 3) | (1 << 31), 0]
    # the budget: one slot goes to the larger term
    hslot, rowmask = rm.row_tables(ip, ix, TILE, budget_bytes=64)
    assert list(hslot) == [-1, 0, -1] and len(rowmask) == 1
    assert rm.kept_rows(0b101, 0, 300).tolist() == [True, False, True]
    assert rm.kept_rows(rm.ALL, 1, 2048).all() and len(rm.kept_rows(rm.ALL, 1, 2048)) == 17
