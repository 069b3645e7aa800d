"""Time the cursor search against the calls it leaves alone and the calls it
replaces, on config 3 (GPU box).

  python scripts/search_after_time.py [--pkg DIR] [--out FILE] [--label NAME]

Builds config 3 (bm25mi.synth), batch 1024, k = 100, and times between HIP
events (3 warm-ups, then --steps calls; the median is one repeat's figure;
--repeats repeats of each call, interleaved, so their spread is the spread of
the session):

  * the calls without a cursor, which launch the same kernel instantiations
    before and after the cursor search exists: search_filtered_device with
    every query_mask entry -1, search_weighted_device with all-1.0 weights;
  * the way pages 2 and 51 are served without a cursor: search_device at
    k = 200 and k = 5100;
  * (a build with the cursor search) search_after_device at k = 100 with each
    row's cursor at its rank-100 and at its rank-5000 key — checked bit for
    bit against columns 100..199 / 5000..5099 of those searches.

--pkg DIR imports another built checkout's mojo-bm25_amd directory (the parent
commit's) in place of the tree's; what it lacks is not measured.  Writes one
JSON line.
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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16, help="host threads for index generation")
    ap.add_argument("--pkg", default=None,
                    help="another built checkout's mojo-bm25_amd directory to measure")
    ap.add_argument("--label", default="tree", help="name of the measured build")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "search_after", "c3.jsonl"))
    args = ap.parse_args()
    for p in (os.path.abspath(args.pkg) if args.pkg else os.path.join(REPO, "mojo-bm25_amd"),
              REPO):
        sys.path.insert(0, p)
    import torch
    from bm25mi import synth
    from bm25mi.index import GpuIndex
    if not torch.cuda.is_available():
        sys.exit("no GPU: this script measures, it has no CPU path")
    has_after = hasattr(GpuIndex, "search_after_device")
    cfg = synth.CONFIGS[args.config]
    t0 = time.time()
    ip, ix, dt = synth.make_index(cfg, threads=args.threads)
    print(f"# index generated in {time.time() - t0:.1f}s nnz={int(ip[-1])}", file=sys.stderr,
          flush=True)
    index = GpuIndex(ip, ix, dt, cfg.n_docs)
    del ix, dt
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    q = synth.make_queries(cfg)
    Q, T, k, N = q.shape[0], q.shape[1], cfg.k, cfg.n_docs
    W = (N + 31) // 32
    dq = torch.from_numpy(q).to(dev)
    none = torch.full((Q,), -1, dtype=torch.int32, device=dev)
    no_masks = torch.zeros((0, W), dtype=torch.int32, device=dev)
    w_ones = torch.ones((Q, T), dtype=torch.float32, device=dev)
    out = lambda n: (torch.empty((Q, n), dtype=torch.int32, device=dev),
                     torch.empty((Q, n), dtype=torch.float32, device=dev))
    fd, fs = out(k)
    wd, ws = out(k)
    d200, s200 = out(2 * k)
    d5100, s5100 = out(51 * k)
    ad, as_ = out(k)
    calls = {
        "filtered_no_filter": lambda: index.search_filtered_device(dq, k, no_masks, none, fd, fs,
                                                                   st),
        "weighted_ones": lambda: index.search_weighted_device(dq, w_ones, k, None, None, wd, ws,
                                                              st),
        "search_k200": lambda: index.search_device(dq, 2 * k, d200, s200, st),
        "search_k5100": lambda: index.search_device(dq, 51 * k, d5100, s5100, st),
    }
    rec = {"config": args.config, "label": args.label, "Q": Q, "T": T, "k": k, "n_docs": N,
           "n_tiles": index.info()["n_tiles"], "steps": args.steps, "warmup": args.warmup,
           "repeats": args.repeats, "has_search_after": bool(has_after)}
    if has_after:
        calls["search_k5100"]()
        calls["search_k200"]()
        torch.cuda.synchronize()
        cur = {100: (s200[:, k - 1].contiguous(), d200[:, k - 1].contiguous()),
               5000: (s5100[:, 50 * k - 1].contiguous(), d5100[:, 50 * k - 1].contiguous())}
        for rank, want in ((100, (d200[:, k:], s200[:, k:])),
                           (5000, (d5100[:, 50 * k:], s5100[:, 50 * k:]))):
            index.search_after_device(dq, k, cur[rank], None, None, None, ad, as_, st)
            torch.cuda.synchronize()
            same = bool(torch.equal(ad, want[0])) and bool(
                torch.equal(as_.view(torch.int32), want[1].contiguous().view(torch.int32)))
            assert same, f"the page after rank {rank} differs from search_device's columns"
            dense, skipped, rescored = index.filtered_stats()
            rec[f"after_rank{rank}_stats"] = {"dense_queries": dense, "rescored_pairs": rescored}
        rec["pages_bit_equal_to_search"] = True
        calls["after_rank100"] = lambda: index.search_after_device(dq, k, cur[100], None, None,
                                                                   None, ad, as_, st)
        calls["after_rank5000"] = lambda: index.search_after_device(dq, k, cur[5000], None, None,
                                                                    None, ad, as_, st)
    ms = {name: [] for name in calls}
    for _ in range(args.repeats):
        for name, fn in calls.items():
            ms[name].append(_time(fn, st, args.warmup, args.steps))
    for name, v in ms.items():
        rec[name] = {"ms": v, "median": round(statistics.median(v), 4), "min": min(v),
                     "max": max(v)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)
    index.close()


if __name__ == "__main__":
    main()
