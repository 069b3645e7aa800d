"""Time bm25_score_docs_device against the dense-row alternative (GPU box).

  python scripts/score_docs_time.py [--out profiles/score_docs/c3.jsonl] [--commit ID]

Builds config 3 (bm25mi.synth), runs one search at the config's k = 100 and
scores that search's own [1024, 100] result again with score_docs_device:
3 warm-ups, then --steps calls each between two HIP events.  The scores must
come back bit-equal to the search's.  For comparison, the only path without
the lookup: bm25_scores_dense (host call: the 40 MB row comes back) for
--dense-queries of those queries, each followed by a host gather of its 100
candidates, timed with a host clock (every call ends in a device
synchronise) and scaled to one query.  Writes one JSON line.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dense-queries", type=int, default=16)
    ap.add_argument("--threads", type=int, default=16, help="host threads for index generation")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "score_docs", "c3.jsonl"))
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
    Q, T, k = q.shape[0], q.shape[1], cfg.k
    dq = torch.from_numpy(q).to(dev)
    dd = torch.empty((Q, k), dtype=torch.int32, device=dev)
    ds = torch.empty((Q, k), dtype=torch.float32, device=dev)
    index.search_device(dq, k, dd, ds, st)
    torch.cuda.synchronize()
    docs, scores = dd.cpu().numpy(), ds.cpu().numpy()

    out = torch.zeros((Q, k), dtype=torch.float32, device=dev)
    for _ in range(args.warmup):
        index.score_docs_device(dq, dd, out, st)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(args.steps)]
    for e0, e1 in ev:
        e0.record(st)
        index.score_docs_device(dq, dd, out, st)
        e1.record(st)
    torch.cuda.synchronize()
    ms = [e0.elapsed_time(e1) for e0, e1 in ev]
    b0, b1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    b0.record(st)  # the same calls back to back between one pair of events
    for _ in range(args.steps):
        index.score_docs_device(dq, dd, out, st)
    b1.record(st)
    torch.cuda.synchronize()
    back_to_back_ms = b0.elapsed_time(b1) / args.steps
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), scores.view(np.uint32)), \
        "score_docs_device differs from the search's scores"

    # the alternative: one dense row per query, gathered on the host
    n = min(args.dense_queries, Q)
    index.scores_dense(q[0])  # warm-up
    gathered = np.zeros((n, k), np.float32)
    t0 = time.perf_counter()
    for i in range(n):
        gathered[i] = index.scores_dense(q[i])[docs[i]]
    dense_ms = 1000.0 * (time.perf_counter() - t0) / n
    assert np.array_equal(gathered.view(np.uint32), scores[:n].view(np.uint32)), \
        "dense rows differ from the search's scores"

    call_ms = statistics.median(ms)
    lookup_ms = call_ms / Q
    rec = {"config": args.config, "commit": args.commit or _commit(), "Q": Q, "T": T, "C": k,
           "steps": args.steps, "warmup": args.warmup,
           "score_docs_ms_per_call": round(call_ms, 5),
           "score_docs_ms_per_call_min": round(min(ms), 5),
           "score_docs_ms_per_call_max": round(max(ms), 5),
           "score_docs_ms_per_call_back_to_back": round(back_to_back_ms, 5),
           "pairs_per_s": round(Q * k / (call_ms * 1e-3), 1),
           "score_docs_ms_per_query": round(lookup_ms, 7),
           "dense_queries": n, "dense_gather_ms_per_query": round(dense_ms, 4),
           "ratio_dense_over_score_docs": round(dense_ms / lookup_ms, 1),
           "bit_equal_to_search": True, "segments_sparse": index.info()["sparse"]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)
    index.close()


if __name__ == "__main__":
    main()
