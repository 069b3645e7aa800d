"""Model of the REST pass's tile bound refined by sub-block presence masks
(dev analysis, CPU only; DESIGN.md §4 "Tile bounds").

scripts/bound_model.py's setting — a sample of a config's bench queries, the
per-tile unpooled tile-bound threshold (k-th best over tiles of the tile's
largest single-term maximum) — and, beside the whole-tile bound (the sum of
the query terms' tile maxima), the masked bound at sub-blocks of 128, 64 and
32 documents: max over the sub-blocks of the sum of the terms with a posting
in the sub-block; for comparison the bound from per-sub-block maxima at 64
documents (a table 32 times bmax's: not an option).  Prints the share of
(query, tile) pairs and of postings each bound skips.

  python scripts/mask_bound_model.py [--config c3] [--queries 32] [--terms 8]
"""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "mojo-bm25_amd"), REPO]

TD = 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--queries", type=int, default=32)
    ap.add_argument("--terms", type=int, default=0)
    ap.add_argument("--shard", type=int, default=0, help="c5: rank of the 8-way shard")
    args = ap.parse_args()
    from bm25mi import synth
    cfg = synth.CONFIGS[args.config]
    if args.terms:
        cfg = dataclasses.replace(cfg, terms_per_query=args.terms)
    lo, hi = (synth.shard_bounds(cfg.n_docs, 8, args.shard) if args.config == "c5"
              else (0, cfg.n_docs))
    t0 = time.time()
    ip, ix, dt = synth.make_index(cfg, lo, hi, threads=8)
    N = hi - lo
    print(f"index {time.time() - t0:.1f}s", file=sys.stderr)
    q = synth.make_queries(cfg)[:args.queries]
    k = cfg.k
    nt = (N + TD - 1) // TD
    # per-(term, tile) maxima, posting counts, and per-(term, 32-doc block) maxima
    tmax, tcnt, bmax32 = {}, {}, {}
    for t in np.unique(q[q >= 0]):
        a, b = ip[t], ip[t + 1]
        d = ix[a:b].astype(np.int64)
        m = np.zeros(nt, np.float32)
        np.maximum.at(m, d // TD, dt[a:b])
        tmax[t] = m
        tcnt[t] = np.bincount(d // TD, minlength=nt)
        m32 = np.zeros(nt * 64, np.float32)
        np.maximum.at(m32, d // 32, dt[a:b])
        bmax32[t] = m32.reshape(nt, 64)
    names = ("tile", "mask128", "mask64", "mask32", "max64")
    pairs = dict.fromkeys(names, 0)
    posts = dict.fromkeys(names, 0)
    all_pairs = all_posts = 0
    for row in q:
        terms = row[row >= 0]
        lb = np.zeros(nt, np.float32)
        cnt = np.zeros(nt, np.int64)
        for t in terms:
            lb = np.maximum(lb, tmax[t])
            cnt += tcnt[t]
        theta = np.sort(lb)[::-1][k - 1]
        ub = {"tile": sum(tmax[t] for t in terms)}
        for docs in (128, 64, 32):
            g = docs // 32
            s = np.zeros((nt, 64 // g), np.float32)
            for t in terms:
                present = bmax32[t].reshape(nt, 64 // g, g).max(axis=2) > 0
                s += present * tmax[t][:, None]
            ub[f"mask{docs}"] = s.max(axis=1)
        ub["max64"] = sum(bmax32[t].reshape(nt, 32, 2).max(axis=2) for t in terms).max(axis=1)
        all_pairs += nt
        all_posts += int(cnt.sum())
        for name in names:
            cut = ub[name] * 1.0001 < theta
            pairs[name] += int(cut.sum())
            posts[name] += int(cnt[cut].sum())
    print(json.dumps({"config": args.config, "terms": int(cfg.terms_per_query), "queries": len(q),
                      "k": k, **{f"skip_pairs_{n}": round(pairs[n] / all_pairs, 4) for n in names},
                      **{f"skip_post_{n}": round(posts[n] / max(all_posts, 1), 4) for n in names}}))


if __name__ == "__main__":
    main()
