"""Dead rows of multi-row term segments (option row_skip): the index keeps a
presence mask per double row of its heavy terms, the pre-pass writes one u16
per (query, tile, term lane), and REST runs only the rows of a kept segment
that have a posting in a live sub-block.  On constructed indexes of f16-valued
scores: results are the oracle's bit for bit with row_skip on and off, the two
new counters of the count_skips build are the numpy model's (tests/
row_model.py), and the four older ones stay tests/seg_model.py's."""
import os

import numpy as np
import pytest

import mask_model as mm
import row_model as rm
import seg_model as sm
from oracle import oracle
from test_gpu_edges import _csc
from test_gpu_parity import _exact, _idx, _world_bounds_search
from test_gpu_seg_skip import _device_search, _set

pytestmark = pytest.mark.gpu

TILE, SUB = mm.TILE, mm.SUB
H, H2, A, B, C, F = range(6)          # H, H2: heavy terms (H the heavier); F: empty
V_FIX = 6
K = 4
ANCHORS = (10, 20, 30, 40)
PEAKS = (12, 22, 32, 42)
FULL = list(range(TILE))


def _fixture(nt):
    """nt tiles (a partial last one).  K anchor tiles hold one document with
    A = 8.0: theta = 8.0 for every query with A.  In the case tiles (two
    8-tile items from `base`, a third tile after them) a sub-block is live
    iff it holds a document with B = C = 5.0; H and H2 score 1.0 there.
    Returns (csc, n_docs, base, want): want[tile] = H's expected row word
    under theta = 8.0."""
    base = (nt - 24) // 8 * 8
    assert base > max(ANCHORS) + 1 and base + 17 <= nt
    n_docs = (nt - 1) * TILE + 993
    # H peaks at 2.0 on one document of four tiles of its own: theta = 2.0 for H alone
    h = [t * TILE + 7 for t in PEAKS]
    bc, want = [], {}

    def case(tile, offs, live, word):
        assert len(h) % 2 == 0 or word is None     # H is term 0: b is even up to the filler
        h.extend(tile * TILE + o for o in offs)
        bc.extend(tile * TILE + o for o in live)
        want[tile] = word

    # ---- item 1: 71 rows of H before dropping, 8 after
    case(base + 0, range(100), [70], 0x0001)                               # one row
    case(base + 1, range(200), [250], 0x0002)                              # only the last of two
    case(base + 2, range(200), [5], 0x0001)                                # only the first of two
    case(base + 3, FULL, [7 * SUB + 3], 1 << 3)                            # 16 rows, a middle one
    case(base + 4, FULL, [1], 1 << 0)                                      # ... the first
    case(base + 5, FULL, [31 * SUB + 60], 1 << 15)                         # ... the last
    case(base + 6, FULL, [16 * SUB], 1 << 8)
    # sub-block 10 touched only by the last posting of row 0 (position 127 = doc 640)
    case(base + 7, list(range(127)) + [640] + list(range(704, 804)), [650], 0x0001)
    # ---- item 2: 72 rows left after dropping (two chunks)
    # ... only by the first posting of row 1 (position 128 = doc 640)
    case(base + 8, list(range(128)) + [640] + list(range(704, 803)), [650], 0x0002)
    for i in range(5):                                                     # every other row lives
        case(base + 9 + i, FULL, [s * SUB + 9 for s in range(0, 32, 4)], 0x5555)
    h.append((base + 14) * TILE + 2047)                                    # filler: b is odd from here
    want[base + 14] = 0                                                    # (H alone: the tile is cut)
    case(base + 15, FULL, [5 * SUB], None)                                 # 17 rows: every row runs
    want[base + 15] = rm.ALL
    # ---- a third item: H2 (three rows, the last one lives) beside H
    case(base + 16, range(200), [260], None)
    del want[base + 16]
    h2 = [(base + 16) * TILE + o for o in range(300)]
    a = [t * TILE + 100 for t in ANCHORS]
    hv = np.full(len(h), 1.0, np.float32)
    hv[:len(PEAKS)] = 2.0
    cols = [(np.array(h, np.int32), hv),
            (np.array(h2, np.int32), np.full(len(h2), 1.0, np.float32)),
            (np.array(a, np.int32), np.full(len(a), 8.0, np.float32)),
            (np.array(bc, np.int32), np.full(len(bc), 5.0, np.float32)),
            (np.array(bc, np.int32), np.full(len(bc), 5.0, np.float32)),
            (np.zeros(0, np.int32), np.zeros(0, np.float32))]
    assert all(np.all(np.diff(d) > 0) for d, _ in cols)
    return _csc(cols, np.float32), n_docs, base, want


def _queries8():
    q = np.full((6, 8), -1, np.int32)
    q[0, :4] = [H, A, B, C]                      # the heavy term on lane 0 (the tile-start bit)
    q[1, :3], q[1, 7] = [A, B, C], H             # ... on lane 7
    q[2, :5] = [H, A, B, H, C]                   # ... twice
    q[3, :7] = [B, -1, H, 99, C, F, A]           # ... beside padding, an unknown id, an empty term
    q[4, :5] = [H2, A, B, C, H]                  # two heavy terms
    q[5, :3] = [A, B, C]                         # none
    return q


def _stats(index, run, ref):
    index.set_option("count_skips", 1)
    _exact(run(), ref)
    st = index.search_stats()
    index.set_option("count_skips", 0)
    old = (st["bound_skipped_tiles"], st["bound_skipped_postings"],
           st["bound_dropped_segments"], st["bound_dropped_postings"])
    return old, (st["bound_dropped_rows"], st["bound_dropped_row_postings"])


def _index(csc, n_docs, budget_kb=None):
    old = os.environ.get("BM25_ROW_MASK_KB")
    if budget_kb is not None:
        os.environ["BM25_ROW_MASK_KB"] = str(budget_kb)
    try:
        return _idx(*csc, n_docs, segments="dense")
    finally:
        if budget_kb is not None:
            if old is None:
                os.environ.pop("BM25_ROW_MASK_KB")
            else:
                os.environ["BM25_ROW_MASK_KB"] = old


def _check(index, csc, n_docs, q, tables, rows_tab, combos, flat_bws=(8, 0)):
    """Every option combination: exact, the dispatch bits, old and new counters."""
    ip, ix, dt = csc
    bmax, tmask = tables
    hslot, rowmask = rows_tab
    ref = oracle.search_c(n_docs, ip, ix, dt, np.where(q >= V_FIX, -1, q), K)
    run = lambda: _device_search(index, q, K)
    seen = {}
    for flat_bw in flat_bws:
        for row, seg, tile_mask in combos:
            _set(index, flat_bw=flat_bw, row_skip=row, seg_skip=seg, tile_mask=tile_mask)
            _exact(run(), ref)
            d = index.last_dispatch()
            assert d["sample_p"] == 0 and d["tile_skip"] and "flat_rest" in d["kernels"], d
            assert d["seg_skip"] == bool(seg and tile_mask), d
            assert d["row_skip"] == bool(row and seg and tile_mask and hslot is not None), d
            old, new = _stats(index, run, ref)
            pooled = "bound_pool" in index.last_dispatch()["kernels"]
            want_old = sm.counts(ip, ix, bmax, tmask, q, K, pooled, tile_mask, seg)[:4]
            want_new = rm.row_counts(ip, ix, bmax, tmask, hslot, rowmask, q, K, pooled,
                                     tile_mask, seg, row)[:2]
            print(f"  flat_bw={flat_bw} row={row} seg={seg} mask={tile_mask}: old {old} model {want_old}; "
                  f"rows {new} model {want_new}")
            assert old == want_old
            assert new == want_new
            if not (row and seg and tile_mask):
                assert new == (0, 0)             # only words 0 and 0xFFFF
            seen[row, seg, tile_mask] = new
    _set(index, flat_bw=0, row_skip=1, seg_skip=1, tile_mask=1)
    return seen


ALL_COMBOS = ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0))


def test_constructed_rows(gpu):
    csc, n_docs, base, want = _fixture(80)
    ip, ix, dt = csc
    tables = mm.tables(ip, ix, dt, n_docs)
    hslot, rowmask = rm.row_tables(ip, ix, n_docs)
    assert hslot[H] == 0 and hslot[H2] == 1 and (hslot[[A, B, C, F]] == -1).all()
    q = _queries8()
    # the cases are what the model sees: H's row word in every case tile, on every lane it takes
    for row in q:
        w = rm.lane_words(*tables, hslot, rowmask, row, np.float32(8.0))
        for lane in np.flatnonzero(row == H):
            for tile, word in want.items():
                assert w[lane, tile] == word, (row, lane, tile - base, hex(w[lane, tile]), hex(word))
    w = rm.lane_words(*tables, hslot, rowmask, q[4], np.float32(8.0))
    assert w[0, base + 16] == 0x0004             # H2: the last of three rows
    # an item of more than 64 rows before dropping and fewer after; one of more than 64 after
    b, l = rm.segments(ip, ix, H, 80)
    full = [rm.seg_rows(int(b[t]), int(l[t])) for t in range(80)]
    kept = [int(rm.kept_rows(want[t], int(b[t]), int(l[t])).sum()) if want.get(t) else 0 for t in range(80)]
    assert sum(full[base:base + 8]) > 64 > sum(kept[base:base + 8]) + 16
    assert sum(kept[base + 8:base + 16]) + 14 > 64 and full[base + 15] == 17   # (+ B's and C's rows)
    index = _index(csc, n_docs)
    seen = _check(index, csc, n_docs, q, tables, (hslot, rowmask), ALL_COMBOS)
    assert seen[1, 1, 1][0] > 5 * 60             # five lanes of H drop 63 of item 1's rows each
    # narrower batches
    for qn in (np.array([[H, B, C], [H2, B, C], [B, H, -1]], np.int32), np.array([[H], [A], [B]], np.int32)):
        _check(index, csc, n_docs, qn, tables, (hslot, rowmask), ((1, 1, 1), (0, 1, 1)), flat_bws=(0,))
    # 16 term lanes: the old path, no pre-pass
    q16 = np.concatenate([q, q[::-1]], axis=1)
    ref16 = oracle.search_c(n_docs, ip, ix, dt, np.where(q16 >= V_FIX, -1, q16), K)
    _exact(_device_search(index, q16, K), ref16)
    d = index.last_dispatch()
    assert not d["tile_skip"] and not d["seg_skip"] and not d["row_skip"] and d["term_lanes"] == 16, d
    # a fork shares the table
    fork = index.fork()
    ref = oracle.search_c(n_docs, ip, ix, dt, np.where(q >= V_FIX, -1, q), K)
    _exact(_device_search(fork, q, K), ref)
    assert fork.last_dispatch()["row_skip"]
    fork.close()
    index.close()


def test_budget_leaves_the_lighter_heavy_term_whole(gpu):
    csc, n_docs, base, want = _fixture(80)
    ip, ix, dt = csc
    tables = mm.tables(ip, ix, dt, n_docs)
    kb = (80 * rm.ROWS * 4 + 1023) // 1024        # one slot
    hslot, rowmask = rm.row_tables(ip, ix, n_docs, budget_bytes=kb * 1024)
    assert hslot[H] == 0 and hslot[H2] == -1 and len(rowmask) == 1
    q = _queries8()
    w = rm.lane_words(*tables, hslot, rowmask, q[4], np.float32(8.0))
    assert w[0, base + 16] == rm.ALL and w[4, base + 3] == 1 << 3
    index = _index(csc, n_docs, budget_kb=kb)
    _check(index, csc, n_docs, q, tables, (hslot, rowmask), ((1, 1, 1),), flat_bws=(8,))
    index.close()
    # no budget: no table, every row runs
    index = _index(csc, n_docs, budget_kb=0)
    _check(index, csc, n_docs, q, tables, (None, None), ((1, 1, 1),), flat_bws=(8,))
    index.close()


@pytest.mark.parametrize("nt", [508, 523, 1020, 1030])
def test_two_and_four_tiles_per_thread(gpu, nt):
    """The pre-pass takes two tiles per thread from 512 tiles (rounded up to
    fours) and four from 1024: both sides of each step."""
    csc, n_docs, base, want = _fixture(nt)
    ip, ix, dt = csc
    tables = mm.tables(ip, ix, dt, n_docs)
    rows_tab = rm.row_tables(ip, ix, n_docs)
    index = _index(csc, n_docs)
    seen = _check(index, csc, n_docs, _queries8(), tables, rows_tab, ((1, 1, 1), (0, 1, 1)), flat_bws=(0,))
    assert seen[1, 1, 1][0] > 5 * 60
    index.close()


def test_doc_shards_under_world_bounds(gpu):
    import scipy.sparse as sp
    import torch
    csc, n_docs, base, want = _fixture(80)
    ip, ix, dt = csc
    q = _queries8()
    q[3, 3] = -1                                 # (the shard search validates ids)
    ref = oracle.search_c(n_docs, ip, ix, dt, q, K)
    m = sp.csc_matrix((dt, ix, ip), shape=(n_docs, V_FIX))
    cut = 37 * TILE
    shards = []
    for lo, hi in ((0, cut), (cut, n_docs)):
        s = m[lo:hi].tocsc()
        s.sort_indices()
        shards.append(_idx(s.indptr.astype(np.int64), s.indices.astype(np.int32),
                           s.data.astype(np.float32), hi - lo, doc_offset=lo, segments="dense"))
    dq = torch.from_numpy(q).cuda()
    for row in (1, 0):
        for s in shards:
            s.set_option("row_skip", row)
        _exact(_world_bounds_search(shards, dq, K), ref)
        d = shards[1].last_dispatch()
        assert d["sample_p"] == 0 and d["tile_skip"] and d["seg_skip"] and d["row_skip"] == bool(row), d
        assert not shards[0].last_dispatch()["row_skip"]      # no heavy term in the first shard
    for s in shards:
        s.close()
