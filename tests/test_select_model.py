"""CPU checks of tests/select_cases.py (no GPU): every case's numpy model of
the candidate list — tile maxima rounded down to f16, the k-th largest, the
documents at or above it — holds exactly the intended number of documents,
from the per-tile and from the pooled bounds alike, and the cases' routes
through the selection stage (the mirror of merge_fast_kernel's dispatch)
cover every route of the kernel."""
import numpy as np
import pytest

import select_cases as sc


@pytest.fixture(scope="module")
def cases():
    return sc.grid()


def test_list_count_is_the_intended_length(cases):
    assert len({c.term for c in cases}) == len(cases)
    for c in cases:
        assert np.all(np.diff(c.docs.astype(np.int64)) > 0)
        assert c.docs.max(initial=0) < sc.N_DOCS
        # f16 values: the tile bounds are exact
        assert np.array_equal(c.vals.astype(np.float16).astype(np.float32), c.vals)
        for pool in (False, True):
            m = sc.row_model(c.docs, c.vals, c.k, pool=pool)
            assert m["cnt"] == c.cnt, (c, pool, m)
            assert sc.list_count((c.docs, c.vals), c.k, pool=pool) == c.cnt
            assert m["zero_fill"] == (c.pattern == "zf"), (c, m)
            if c.pattern != "zf":
                assert m["v_k"] == float(sc.f16_bits(sc.BASE)), (c, m)
        if c.pattern == "d":
            assert m["above_kth"] == c.k - 1
            assert m["above_kth"] + m["ties_at_kth"] == (c.cnt if c.ge is None else c.ge)
        if c.pattern == "a":
            assert m["ties_at_kth"] == c.cnt


def test_noise_sits_one_f16_step_below_the_threshold(cases):
    for c in cases:
        if c.pattern == "zf":
            continue
        below = c.vals[c.vals < sc.f16_bits(sc.BASE)]
        assert len(below) >= 40 and np.all(below == sc.f16_bits(sc.BASE - 1)), c
        # ... in tiles of their own and inside anchor tiles
        lt = np.unique(c.docs[c.vals >= sc.f16_bits(sc.BASE)] // sc.TILE)
        nt = c.docs[c.vals < sc.f16_bits(sc.BASE)] // sc.TILE
        assert np.isin(nt, lt).any() and (~np.isin(nt, lt)).any(), c
        if c.k > 1:  # exactly k anchor tiles, in distinct groups of 4
            assert len(lt) == c.k and len(np.unique(lt // sc.POOL)) == c.k, c


def test_route_mirror_edges():
    r = sc.route
    C = sc.LIST_CAP
    assert [r(n, 64, 1, False, C) for n in (256, 257, 512, 513)] == \
        ["fast4", "fast8_provisional", "fast8_provisional", "block_long"]
    assert [r(n, 64, 1, True, C) for n in (512, 513, 1024, 1025)] == \
        ["shard8", "shard16", "shard16", "block_long"]
    assert [r(n, 128, 1, False, C) for n in (8192, 8193, C, C + 1)] == \
        ["block_long", "tail_merge_first", "tail_merge_first", "fallback"]
    assert [r(n, 129, 1, False, C) for n in (256, 257, 512, 513, 1024, 1025, 2048)] == \
        ["fast4", "fast8_regs4", "fast8_regs4", "fast16_regs4", "fast16_regs4", "fast32_regs4",
         "fast32_regs4"]
    assert [r(n, 300, 1, False, C) for n in (300, 512, 513, 2048, 2049)] == \
        ["fast8_lds", "fast8_lds", "fast16_lds", "fast32_lds", "long_sampled"]
    assert [r(3000, 1024, t, False, C) for t in (1, 2)] == ["long_digits", "long_giveup"]
    assert r(3000, 300, 3000, False, C) == "long_sampled"  # (the sample decides first)
    assert [r(n, 1025, 1, False, C) for n in (8192, 8193)] == ["merge_first", "merge_first_chunked"]
    assert r(3, 64, 0, False, C, zero_fill=True) == "zero_fill"
    assert r(69, 64, 1, False, C, zero_fill=True) == "fast4"
    assert r(600, 64, 1, False, C, zero_fill=True) == "fast16_regs2"
    with pytest.raises(ValueError):
        r(2049, 500, 1, False, C)  # ~1000 keys reach the sampled threshold: either way


def test_grid_covers_every_route(cases):
    """The single-index grid, the two doc shards of its k = 100 and k = 300
    batches and the overflow rows between them take every route of the
    selection stage."""
    seen = {}
    for c in cases:
        m = sc.row_model(c.docs, c.vals, c.k)
        seen.setdefault(sc.model_route(m, c.k), []).append((c.k, c.cnt, c.pattern))
    for c in cases:
        if c.k in (100, 300):
            for m in sc.shard_models(c.docs, c.vals, c.k, [sc.SHARD_CUT_TILE]):
                seen.setdefault(sc.model_route(m, c.k, unsorted=True), []).append(
                    (c.k, m["cnt"], c.pattern))
    seen.setdefault(sc.route(1025, 100, 1, False, 1024), []).append((100, 1025, "overflow"))
    for name in sc.ROUTES:
        print(f"{name:20s} {len(seen.get(name, [])):4d} cases, e.g. {seen.get(name, ['-'])[0]}")
    assert set(seen) >= set(sc.ROUTES), set(sc.ROUTES) - set(seen)
    assert set(seen) <= set(sc.ROUTES), set(seen) - set(sc.ROUTES)


def test_shards_split_the_lists(cases):
    """The doc-shard cut splits the anchor tiles unevenly, and the two
    shards' lists add up to the single index's list or less (ties at v_k past
    the k-th tile's last document are cut by the global theta)."""
    for c in cases:
        if c.k not in (100, 300) or c.pattern == "zf":
            continue
        a, b = sc.shard_models(c.docs, c.vals, c.k, [sc.SHARD_CUT_TILE])
        assert c.k <= a["cnt"] + b["cnt"] <= c.cnt, (c, a, b)
        assert a["cnt"] > 0 and b["cnt"] > 0, (c, a, b)
        lt = np.unique(c.docs[c.vals >= sc.f16_bits(sc.BASE)] // sc.TILE)
        lo = int((lt < sc.SHARD_CUT_TILE).sum())
        assert 0 < lo < c.k - lo, (c, lo)
