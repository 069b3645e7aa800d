"""Time the collapsed search on config 3 (GPU box) beside the cursor-search
page it is built on.

  python scripts/search_collapsed_time.py [--out FILE] [--steps N] [--repeats N]

Builds config 3 (bm25mi.synth), batch 1024, per_group 1, k = 10 and 100, and
times between HIP events (--warmup warm-ups, then --steps calls; the median is
one repeat's figure; --repeats repeats of each call, interleaved):

  * search_collapsed_device under a uniform layout (groups of about 16
    documents) at collapse_page p in {k, 2k, 4k, 8k} (capped at 4096), and at
    the automatic page under the uniform and a skewed layout (a document's
    group drawn with the synth's own term-frequency skew: probability
    proportional to a term's document frequency);
  * from the same run, one search_after_device page of the same p without a
    cursor — the floor a one-round collapsed search cannot beat.  The
    difference of the two is what the walk adds (its kernel, the state's
    memsets and the round's read-back); rounds past the first show in
    "rounds" and in the time.

Nothing here is a threshold.  Every collapsed result is checked for the
property that can be checked without a reference: no group twice in a row.
Writes one JSON line per (layout, k, p).
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
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16, help="host threads for index generation")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "collapse", "c3.jsonl"))
    args = ap.parse_args()
    for p in (os.path.join(REPO, "mojo-bm25_amd"), REPO):
        sys.path.insert(0, p)
    import numpy as np
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
    Q, T, N = q.shape[0], q.shape[1], cfg.n_docs
    dq = torch.from_numpy(q).to(dev)
    rng = np.random.default_rng(5)
    df = np.diff(np.asarray(ip, np.int64)).astype(np.float64)
    cdf = np.cumsum(df / df.sum())
    layouts = {
        "uniform": rng.integers(0, N // 16, N).astype(np.int32),
        "skewed": np.minimum(np.searchsorted(cdf, rng.random(N)), len(df) - 1).astype(np.int32),
    }
    sizes = {name: np.bincount(g) for name, g in layouts.items()}
    dgroups = {name: torch.from_numpy(g).to(dev) for name, g in layouts.items()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    lines = []
    for k in (10, 100):
        cd = torch.empty((Q, k), dtype=torch.int32, device=dev)
        cs = torch.empty((Q, k), dtype=torch.float32, device=dev)
        cg = torch.empty((Q, k), dtype=torch.int32, device=dev)
        cases = [("uniform", p) for p in sorted({min(4096, m * k) for m in (1, 2, 4, 8)})]
        cases += [("uniform", 0), ("skewed", 0)]
        calls, recs = {}, {}
        for name, p in cases:
            index.set_option("collapse_page", p)
            index.search_collapsed_device(dq, k, dgroups[name], 1, None, None, None, cd, cs, cg, st)
            torch.cuda.synchronize()
            stats = index.collapse_stats()
            srt = torch.sort(cg, dim=1).values
            twice = bool(((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] >= 0)).any())
            assert not twice, f"a group twice in a row ({name}, k={k}, p={p})"
            assert bool((cd >= 0).all()), "a padded row on config 3"
            page = p if p else min(4096, 2 * k)   # (the automatic page: 2 k)
            recs[(name, p)] = {"config": args.config, "layout": name, "Q": Q, "T": T, "k": k,
                               "per_group": 1, "collapse_page": p, "page": page, "n_docs": N,
                               "groups": int((sizes[name] > 0).sum()),
                               "largest_group": int(sizes[name].max()), "steps": args.steps,
                               "warmup": args.warmup, "repeats": args.repeats, **stats}

            def collapsed(name=name, p=p):
                index.set_option("collapse_page", p)
                index.search_collapsed_device(dq, k, dgroups[name], 1, None, None, None, cd, cs,
                                              cg, st)
            calls[("collapsed", name, p)] = collapsed
            if name == "uniform":
                pd = torch.empty((Q, page), dtype=torch.int32, device=dev)
                ps = torch.empty((Q, page), dtype=torch.float32, device=dev)
                calls[("page", name, p)] = (lambda page=page, pd=pd, ps=ps:
                                            index.search_after_device(dq, page, None, None, None,
                                                                      None, pd, ps, st))
        ms = {key: [] for key in calls}
        for _ in range(args.repeats):
            for key, fn in calls.items():
                # (a layout that takes many rounds: fewer, longer steps)
                many = key[0] == "collapsed" and recs[key[1:]]["rounds"] > 4
                ms[key].append(_time(fn, st, 1 if many else args.warmup,
                                     3 if many else args.steps))
        for (name, p), rec in recs.items():
            v = ms[("collapsed", name, p)]
            rec["collapsed_ms"] = {"ms": v, "median": round(statistics.median(v), 4),
                                   "min": min(v), "max": max(v)}
            pv = ms.get(("page", name, p))
            if pv:
                rec["page_ms"] = {"ms": pv, "median": round(statistics.median(pv), 4),
                                  "min": min(pv), "max": max(pv)}
                rec["walk_share"] = round(
                    1.0 - rec["page_ms"]["median"] / rec["collapsed_ms"]["median"], 4)
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    index.set_option("collapse_page", 0)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    index.close()


if __name__ == "__main__":
    main()
