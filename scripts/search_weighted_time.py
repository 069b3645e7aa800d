"""Time bm25_search_weighted_device on config 3 (GPU box).

  python scripts/search_weighted_time.py [--out profiles/search_weighted/c3.jsonl] [--commit ID]

Builds config 3 (bm25mi.synth), batch 1024, k = 100, and times between HIP
events (3 warm-ups, then --steps calls; the median is reported), all without a
filter:

  * the yardstick, code from before the weighted search: search_filtered_device
    with every query_mask entry -1;
  * search_weighted_device with all-1.0 weights (its result must equal the
    yardstick's bit for bit);
  * search_weighted_device with random weights in [0.5, 2).

Writes one JSON line with the two ratios over the yardstick.  --only
{filtered,ones,random} runs that call alone and writes nothing: the run to put
under a profiler.  On a build without the weighted search only the yardstick
is measured (--yardstick-only).
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
    ap.add_argument("--threads", type=int, default=16, help="host threads for index generation")
    ap.add_argument("--only", default=None, choices=("filtered", "ones", "random"),
                    help="run this call alone and write nothing: the run to put under a profiler")
    ap.add_argument("--yardstick-only", action="store_true",
                    help="measure search_filtered_device alone (a build without the weighted search)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "search_weighted", "c3.jsonl"))
    ap.add_argument("--commit", default=None, help="label of the measured code (default: git HEAD)")
    args = ap.parse_args()
    import torch
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
    W = (N + 31) // 32
    dq = torch.from_numpy(q).to(dev)
    none = torch.full((Q,), -1, dtype=torch.int32, device=dev)
    no_masks = torch.zeros((0, W), dtype=torch.int32, device=dev)
    rng = np.random.default_rng(0)
    w_ones = torch.ones((Q, T), dtype=torch.float32, device=dev)
    w_rand = torch.from_numpy(rng.uniform(0.5, 2.0, (Q, T)).astype(np.float32)).to(dev)
    fd = torch.empty((Q, k), dtype=torch.int32, device=dev)
    fs = torch.empty((Q, k), dtype=torch.float32, device=dev)
    wd = torch.empty((Q, k), dtype=torch.int32, device=dev)
    ws = torch.empty((Q, k), dtype=torch.float32, device=dev)
    calls = {
        "filtered": lambda: index.search_filtered_device(dq, k, no_masks, none, fd, fs, st),
        "ones": lambda: index.search_weighted_device(dq, w_ones, k, None, None, wd, ws, st),
        "random": lambda: index.search_weighted_device(dq, w_rand, k, None, None, wd, ws, st),
    }
    rec = {"config": args.config, "commit": args.commit or _commit(), "Q": Q, "T": T, "k": k,
           "n_docs": N, "n_tiles": index.info()["n_tiles"], "steps": args.steps,
           "warmup": args.warmup, "segments_sparse": index.info()["sparse"]}

    if args.only:
        print(json.dumps(_time(calls[args.only], st, args.warmup, args.steps)), flush=True)
        index.close()
        return

    def run(name):
        r = _time(calls[name], st, args.warmup, args.steps)
        dense, skipped, rescored = index.filtered_stats()
        r.update({"dense_queries": dense, "rescored_pairs": rescored})
        return r

    rec["filtered_no_filter"] = run("filtered")
    if not args.yardstick_only:
        rec["weighted_ones"] = run("ones")
        torch.cuda.synchronize()
        same = bool(torch.equal(fd, wd)) and bool(torch.equal(fs.view(torch.int32),
                                                              ws.view(torch.int32)))
        assert same, "the all-1.0 weighted result differs from search_filtered_device"
        rec["ones_bit_equal_to_filtered"] = True
        rec["weighted_random"] = run("random")
        # the yardstick once more, after the weighted calls (drift of the session)
        rec["filtered_no_filter_again"] = run("filtered")
        base = rec["filtered_no_filter"]["ms"]
        rec["ratio_ones_over_filtered"] = round(rec["weighted_ones"]["ms"] / base, 3)
        rec["ratio_random_over_filtered"] = round(rec["weighted_random"]["ms"] / base, 3)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)
    index.close()


if __name__ == "__main__":
    main()
