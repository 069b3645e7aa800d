"""CPU model of the masked tile bound (no GPU; DESIGN.md §4 "Tile bounds").

tests/mask_model.py restates tile_skip_kernel: the whole-tile bound (the sum
of the query terms' f16 upper bounds) and its refinement by the 32-bit
sub-block presence masks (max over the 64-document sub-blocks of the sum of
the terms present there).  On a small synthetic index (bm25mi.synth, the
bench's generator at 100k documents with config 3's vocabulary and postings
per document) and 200 of its queries, plus hand-made
rows with duplicates, padding and out-of-vocabulary ids, under several
thresholds:
  * every (query, tile) pair the model skips holds no document at or above
    the threshold — the oracle's dense fp32 scores decide;
  * the masked bound never exceeds the whole-tile bound, so it skips every
    pair the whole-tile bound skips (and, on this data, more)."""
import numpy as np
import pytest

import mask_model as mm
from oracle import oracle

N, V = 100_000, 200_000


@pytest.fixture(scope="module")
def case():
    from bm25mi import synth
    cfg = synth.Config("mask model", N, V, 6_400_000, 200, 8, 10)
    ip, ix, dt = synth.make_index(cfg, threads=4)
    q = synth.make_queries(cfg)
    hand = np.full((6, 8), -1, np.int32)
    hand[0, :3] = q[0, :3]                       # padded tail
    hand[1, :] = q[1, 0]                         # one term eight times
    hand[2, [0, 3, 5]] = q[2, 0], q[2, 0], q[2, 1]  # duplicates between padding
    hand[3, :4] = [V, q[3, 0], V + 7, 2**31 - 1]  # out-of-vocabulary ids
    hand[4, 0] = int(np.argmax(np.diff(ip)))     # the most common term alone
    # hand[5]: all padding
    bmax, tmask = mm.tables(ip, ix, dt, N)
    return ip, ix, dt, np.concatenate([q, hand]), bmax, tmask


def test_masked_bound_is_sound_and_tighter(case):
    ip, ix, dt, q, bmax, tmask = case
    nt = bmax.shape[1]
    more = pairs = 0
    for row in q:
        terms = row[(row >= 0) & (row < V)]
        dense = oracle.scores_dense_c(N, ip, ix, dt, terms)
        best = np.pad(dense, (0, nt * mm.TILE - N)).reshape(nt, mm.TILE).max(axis=1)
        top = np.sort(dense)[::-1]
        masked_ub, whole_ub = mm.real_masked_bound(bmax, tmask, row)
        assert (masked_ub <= whole_ub).all()
        assert (best <= masked_ub).all()         # an upper bound of every fp32 sum in the tile
        for theta in (mm.theta_bound(bmax, row, 3, False), mm.theta_bound(bmax, row, 3, True),
                      top[9], top[99], top[999]):
            whole, skipped = mm.skip_model(bmax, tmask, row, theta)
            assert (best[skipped] < theta).all(), (row, theta)
            assert not (whole & ~skipped).any()
            _, plain = mm.skip_model(bmax, tmask, row, theta, use_mask=False)
            assert np.array_equal(plain, whole)
            if theta > 0:
                more += int((skipped & ~whole).sum())
                pairs += nt
            else:
                assert not skipped.any()
    print(f"  masks cut {more} of {pairs} pairs that the whole-tile sum keeps")
    assert more > 0, pairs                       # the masks do cut pairs the sum does not


def test_model_tables_and_edges():
    """Sub-block bits at the block edges, the duplicate counted twice, and a
    term past f16's range never cut."""
    docs = np.array([0, 63, 64, 1983, 2047, 2048 + 64], np.int32)
    ip = np.array([0, 6, 6, 8], np.int64)
    ix = np.concatenate([docs, [5, 2048 + 5]]).astype(np.int32)
    dt = np.array([5, 5, 5, 5, 5, 5, 70000.0, 5], np.float32)
    bmax, tmask = mm.tables(ip, ix, dt, 2 * mm.TILE)
    assert tmask[0].tolist() == [1 | 2 | 1 << 30 | 1 << 31, 2] and tmask[1].tolist() == [0, 0]
    assert bmax[2, 0] == 0x7BFF and bmax[1].tolist() == [0, 0]
    # tile 1: term 0 in sub-block 1, term 2 in sub-block 0 — 5 + 5 reaches 8 only together
    whole, skipped = mm.skip_model(bmax, tmask, np.array([0, 2], np.int32), 8.0)
    assert whole.tolist() == [False, False] and skipped.tolist() == [False, True]
    # the duplicate counts twice: 2 x 5 >= 8 in tile 1; once would be cut
    _, skipped = mm.skip_model(bmax, tmask, np.array([0, 0], np.int32), 8.0)
    assert skipped.tolist() == [False, False]
    _, skipped = mm.skip_model(bmax, tmask, np.array([0, -1], np.int32), 8.0)
    assert skipped.tolist() == [True, True]
    # theta not positive: nothing is skipped
    _, skipped = mm.skip_model(bmax, tmask, np.array([1, -1], np.int32), 0.0)
    assert not skipped.any()
