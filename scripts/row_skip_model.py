"""Model of REST's double rows under the tile cut, seg_skip and row_skip (dev
analysis, CPU only; DESIGN.md §4 "Dead rows of multi-row segments").

scripts/mask_bound_model.py's setting — a config's bench queries, the
per-tile unpooled tile-bound threshold, 64-doc presence masks — on a seeded
random sample of the batch (its first queries are not representative: they
cut 8 % of the pairs where the whole batch cuts 23.6 %).  Counts REST's double
rows — a (term, tile) segment [b, b + l) of absolute posting indices has
((b & 1) + l + 127) >> 7 of them — that run

  all      without any bound
  cut      in the tiles the masked bound does not cut
  seg      ... of the segments with a posting in a live sub-block (seg_skip)
  row      ... that themselves hold a posting in a live sub-block (row_skip;
           segments of more than 16 rows keep all of them)

and prints their shares of `all`, the rows row_skip drops relative to seg, the
share of the seg rows owned by terms with a multi-row segment, and the rows
and postings in segments of 128 or more postings.

  python scripts/row_skip_model.py [--config c3] [--queries 40] [--seed 1]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "mojo-bm25_amd"), REPO]

TD, SUB, ROW, ROWS = 2048, 64, 128, 16


def term_tables(ip, ix, dt, t, nt):
    """Per tile: maximum, sub-block mask, segment start and length; per
    posting: its tile, row of its segment and sub-block bit."""
    a, e = int(ip[t]), int(ip[t + 1])
    d = ix[a:e].astype(np.int64)
    tile = d // TD
    m = np.zeros(nt, np.float32)
    np.maximum.at(m, tile, dt[a:e])
    bit = np.uint32(1) << ((d % TD) // SUB).astype(np.uint32)
    mask = np.zeros(nt, np.uint32)
    np.bitwise_or.at(mask, tile, bit)
    l = np.bincount(tile, minlength=nt).astype(np.int64)
    b = a + np.concatenate([[0], np.cumsum(l)[:-1]])
    row = (np.arange(a, e) - (b[tile] & ~1)) // ROW
    nrows = np.where(l > 0, ((b & 1) + l + ROW - 1) // ROW, 0)
    return m, mask, l, nrows, tile, row, bit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--queries", type=int, default=40)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    from bm25mi import synth
    cfg = synth.CONFIGS[args.config]
    t0 = time.time()
    ip, ix, dt = synth.make_index(cfg, threads=8)
    N = cfg.n_docs
    print(f"index {time.time() - t0:.1f}s", file=sys.stderr)
    qa = synth.make_queries(cfg)
    q = qa[np.sort(np.random.default_rng(args.seed).choice(len(qa), args.queries, replace=False))]
    k, nt = cfg.k, (N + TD - 1) // TD
    tab = {int(t): term_tables(ip, ix, dt, int(t), nt) for t in np.unique(q[q >= 0])}
    rows = dict.fromkeys(("all", "cut", "seg", "row"), 0)
    heavy_rows = big_rows = big_posts = all_posts = 0
    for qrow in q:
        terms = [int(t) for t in qrow if t >= 0]
        lb = np.zeros(nt, np.float32)
        for t in terms:
            lb = np.maximum(lb, tab[t][0])
        theta = np.sort(lb)[::-1][k - 1]
        # live mask of every tile: bit s = the masked sum of sub-block s reaches theta
        L = np.zeros(nt, np.uint32)
        for s in range(32):
            acc = np.zeros(nt, np.float32)
            for t in terms:
                acc += ((tab[t][1] >> np.uint32(s)) & 1) * tab[t][0]
            L |= (acc * np.float32(1.0001) >= theta).astype(np.uint32) << np.uint32(s)
        for t in terms:
            m, mask, l, nrows, tile, row, bit = tab[t]
            keep_seg = (mask & L) != 0
            rows["all"] += int(nrows.sum())
            rows["cut"] += int(nrows[L != 0].sum())
            rows["seg"] += int(nrows[keep_seg].sum())
            live_post = (bit & L[tile]) != 0
            wide = keep_seg & (nrows > ROWS)          # (17 rows: all of them run)
            lp = live_post & ~wide[tile]
            rows["row"] += len(np.unique(tile[lp] * 64 + row[lp])) + int(nrows[wide].sum())
            if (nrows >= 2).any():
                heavy_rows += int(nrows[keep_seg].sum())
            big_rows += int(nrows[l >= 128].sum())
            big_posts += int(l[l >= 128].sum())
            all_posts += int(l.sum())
    a = max(rows["all"], 1)
    print(json.dumps({"config": args.config, "queries": len(q), "seed": args.seed, "k": k,
                      **{f"rows_{n}": round(rows[n] / a, 4) for n in ("cut", "seg", "row")},
                      "row_vs_seg": round(1 - rows["row"] / max(rows["seg"], 1), 4),
                      "seg_rows_of_heavy_terms": round(heavy_rows / max(rows["seg"], 1), 4),
                      "rows_in_segments_ge_128": round(big_rows / a, 4),
                      "postings_in_segments_ge_128": round(big_posts / max(all_posts, 1), 4)}))


if __name__ == "__main__":
    main()
