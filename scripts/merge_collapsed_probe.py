"""Time the doc-shard merge of collapsed lists on config 3 (GPU box) beside the
plain W-way merge and the per-shard collapsed search.

  python scripts/merge_collapsed_probe.py [--out FILE] [--steps N] [--repeats N]

Config 3 (bm25mi.synth) as eight doc shards on one GPU, batch 1024, k = 100,
per_group 1, the uniform layout of scripts/search_collapsed_time.py (groups of
about 16 documents, drawn over the whole collection).  Every shard runs
search_collapsed_device with d_groups_out into its slice of the packed
[8][docs|scores|groups][Q][k] buffer — what bm25mi.dist.sharded_search_collapsed
all-gathers — and between HIP events (--warmup warm-ups, then --steps calls,
the median of them one repeat's figure; --repeats repeats, interleaved) the
script times

  * bm25_merge_collapsed_device on that buffer,
  * bm25_merge_sorted_device on the same docs and scores (existing code: the
    yardstick; it does not collapse, so its rows differ),
  * one shard's search_collapsed_device (shard 0): a rank's own work in a
    sharded collapsed batch, of which the merge is a share.

Nothing here is a threshold.  The merged rows are checked for what can be
checked without a reference: no group twice in a row, no padding, order.
Writes one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _time(fn, st, warmup, steps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(steps)]
    for e0, e1 in ev:
        e0.record(st)
        fn()
        e1.record(st)
    torch.cuda.synchronize()
    return round(statistics.median(e0.elapsed_time(e1) for e0, e1 in ev), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--shards", type=int, default=8)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16, help="host threads for index generation")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "merge_collapse", "c3.jsonl"))
    args = ap.parse_args()
    for p in (os.path.join(REPO, "mojo-bm25_amd"), REPO):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    from bm25mi import synth
    from bm25mi.index import GpuIndex, merge_collapsed_device, merge_sorted_device
    if not torch.cuda.is_available():
        sys.exit("no GPU: this script measures, it has no CPU path")
    cfg = synth.CONFIGS[args.config]
    W, k, N = args.shards, args.k, cfg.n_docs
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    q = synth.make_queries(cfg)
    Q = q.shape[0]
    dq = torch.from_numpy(q).to(dev)
    groups = np.random.default_rng(5).integers(0, N // 16, N).astype(np.int32)
    shards, dgroups = [], []
    t0 = time.time()
    for r in range(W):
        lo, hi = synth.shard_bounds(N, W, r)
        ip, ix, dt = synth.make_index(cfg, lo, hi, threads=args.threads)
        shards.append(GpuIndex(ip, ix, dt, hi - lo, doc_offset=lo))
        dgroups.append(torch.from_numpy(groups[lo:hi]).to(dev))
        del ip, ix, dt
    print(f"# {W} shards generated in {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
    g = torch.empty((W, 3, Q, k), dtype=torch.int32, device=dev)

    def search(r):
        shards[r].search_collapsed_device(dq, k, dgroups[r], 1, None, None, None, g[r, 0],
                                          g[r, 1].view(torch.float32), g[r, 2], st)

    rounds = []
    for r in range(W):
        search(r)
        rounds.append(shards[r].collapse_stats()["rounds"])
    torch.cuda.synchronize()
    od = torch.empty((Q, k), dtype=torch.int32, device=dev)
    os_ = torch.empty((Q, k), dtype=torch.float32, device=dev)
    og = torch.empty((Q, k), dtype=torch.int32, device=dev)
    pd = torch.empty((Q, k), dtype=torch.int32, device=dev)
    ps = torch.empty((Q, k), dtype=torch.float32, device=dev)
    gs = g[:, 1].view(torch.float32)
    calls = {
        "merge_collapsed": lambda: merge_collapsed_device(0, g, gs, g[:, 2], W, Q, k, 3 * Q * k, 1,
                                                          od, os_, og, st),
        "merge_sorted": lambda: merge_sorted_device(0, g, gs, W, Q, k, 3 * Q * k, pd, ps, st),
        "shard_search": lambda: search(0),
    }
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    srt = torch.sort(og, dim=1).values
    assert not bool(((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] >= 0)).any()), "a group twice"
    assert bool((od >= 0).all()), "a padded row on config 3"
    assert bool((os_[:, 1:] <= os_[:, :-1]).all()), "a row out of order"
    dropped = int((od != pd).any(dim=1).sum())  # rows the second collapse changed
    ms = {name: [] for name in calls}
    for _ in range(args.repeats):
        for name, fn in calls.items():
            ms[name].append(_time(fn, st, args.warmup, args.steps))
    rec = {"config": args.config, "shards": W, "Q": Q, "k": k, "per_group": 1, "n_docs": N,
           "layout": "uniform", "groups": int(len(np.unique(groups))), "steps": args.steps,
           "warmup": args.warmup, "repeats": args.repeats, "shard_rounds": rounds,
           "rows_changed_by_second_collapse": dropped}
    for name, v in ms.items():
        rec[name + "_ms"] = {"ms": v, "median": round(statistics.median(v), 4), "min": min(v),
                             "max": max(v)}
    mc, mso, ss = (rec[n + "_ms"]["median"] for n in ("merge_collapsed", "merge_sorted",
                                                      "shard_search"))
    rec["collapsed_over_sorted"] = round(mc / mso, 3)
    rec["merge_share_of_rank_batch"] = round(mc / (mc + ss), 4)
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    for s in shards:
        s.close()


if __name__ == "__main__":
    main()
