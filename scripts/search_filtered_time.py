"""Time bm25_search_filtered_device on config 3 (GPU box).

  python scripts/search_filtered_time.py [--out profiles/search_filtered/c3.jsonl] [--commit ID]

Builds config 3 (bm25mi.synth), batch 1024, k = 100, and times between HIP
events (3 warm-ups, then --steps calls; the median is reported):

  * the tile passes with four masks: all ones, random 50 %, random 1 % and a
    contiguous 1 % range of the documents;
  * the dense path (filter_tiles = 0) on a --dense-queries subset with the
    50 % mask, scaled to the whole batch;
  * as yardsticks, code paths this feature does not touch: search_device as
    it is, and search_device with flat = 0, sample_p = 1 — the exact pass over
    every tile through the same add_item helper the filter's pass A uses.

The all-ones result must equal search_device's bit for bit.  Writes one JSON
line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "mojo-bm25_amd"), REPO):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402


def _commit():
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], check=True,
                              capture_output=True, text=True).stdout.strip()
    except Exception:
        return "unknown"


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
    ms = [e0.elapsed_time(e1) for e0, e1 in ev]
    return {"ms": round(statistics.median(ms), 4), "min": round(min(ms), 4),
            "max": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dense-queries", type=int, default=32)
    ap.add_argument("--threads", type=int, default=16, help="host threads for index generation")
    ap.add_argument("--only", default=None,
                    help="run the tile passes with this mask alone (ones, half, one_pct, "
                         "range_one_pct) and write nothing: the run to put under a profiler")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "search_filtered", "c3.jsonl"))
    ap.add_argument("--commit", default=None, help="label of the measured code (default: git HEAD)")
    args = ap.parse_args()
    import torch
    import bm25mi
    from bm25mi import synth
    from bm25mi.index import GpuIndex
    if not torch.cuda.is_available():
        sys.exit("no GPU: this script measures, it has no CPU path")
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
    dq = torch.from_numpy(q).to(dev)
    dd = torch.empty((Q, k), dtype=torch.int32, device=dev)
    ds = torch.empty((Q, k), dtype=torch.float32, device=dev)
    fd = torch.empty((Q, k), dtype=torch.int32, device=dev)
    fs = torch.empty((Q, k), dtype=torch.float32, device=dev)

    rng = np.random.default_rng(0)
    lo = N // 3
    rng_mask = np.zeros(N, bool)
    rng_mask[lo:lo + N // 100] = True
    allow = {"ones": np.ones(N, bool), "half": rng.random(N) < 0.5,
             "one_pct": rng.random(N) < 0.01, "range_one_pct": rng_mask}
    names = list(allow)
    dm = torch.from_numpy(bm25mi.pack_mask(np.stack([allow[n] for n in names])).view(np.int32)).to(dev)
    rec = {"config": args.config, "commit": args.commit or _commit(), "Q": Q, "T": T, "k": k,
           "n_docs": N, "n_tiles": index.info()["n_tiles"], "steps": args.steps,
           "warmup": args.warmup, "segments_sparse": index.info()["sparse"]}

    if args.only:
        dqm = torch.full((Q,), names.index(args.only), dtype=torch.int32, device=dev)
        print(json.dumps(_time(lambda: index.search_filtered_device(dq, k, dm, dqm, fd, fs, st),
                               st, args.warmup, args.steps)), flush=True)
        index.close()
        return

    # yardsticks: the unfiltered search as it is, and its exact pass over every tile
    rec["search_device"] = _time(lambda: index.search_device(dq, k, dd, ds, st), st, args.warmup,
                                 args.steps)
    old = {n: index.get_option(n) for n in ("flat", "sample_p")}
    index.set_option("flat", 0)
    index.set_option("sample_p", 1)
    rec["search_device_flat0_p1"] = _time(lambda: index.search_device(dq, k, dd, ds, st), st,
                                          args.warmup, args.steps)
    for n, v in old.items():
        index.set_option(n, v)
    index.search_device(dq, k, dd, ds, st)
    torch.cuda.synchronize()

    for m, name in enumerate(names):
        dqm = torch.full((Q,), m, dtype=torch.int32, device=dev)
        r = _time(lambda: index.search_filtered_device(dq, k, dm, dqm, fd, fs, st), st,
                  args.warmup, args.steps)
        dense, skipped, rescored = index.filtered_stats()
        r.update({"dense_queries": dense, "skipped_pairs": skipped, "rescored_pairs": rescored})
        rec["tiles_" + name] = r
        if name == "ones":
            torch.cuda.synchronize()
            same = bool(torch.equal(fd, dd)) and bool(torch.equal(fs.view(torch.int32),
                                                                  ds.view(torch.int32)))
            assert same, "the all-ones filtered result differs from search_device"
            rec["ones_bit_equal_to_search"] = True

    # the dense path on a subset, scaled to the batch
    n = min(args.dense_queries, Q)
    index.set_option("filter_tiles", 0)
    dqm = torch.full((n,), names.index("half"), dtype=torch.int32, device=dev)
    r = _time(lambda: index.search_filtered_device(dq[:n], k, dm, dqm, fd[:n], fs[:n], st), st,
              args.warmup, args.steps)
    index.set_option("filter_tiles", 1)
    r.update({"queries": n, "ms_scaled_to_batch": round(r["ms"] * Q / n, 3)})
    rec["dense_half"] = r

    rec["ratio_ones_over_flat0_p1"] = round(rec["tiles_ones"]["ms"] /
                                            rec["search_device_flat0_p1"]["ms"], 3)
    rec["ratio_range_over_ones"] = round(rec["tiles_range_one_pct"]["ms"] /
                                         rec["tiles_ones"]["ms"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)
    index.close()


if __name__ == "__main__":
    main()
