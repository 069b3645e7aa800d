"""Time bm25_term_masks_device, and the filtered search it feeds, on config 3
(GPU box).

  python scripts/term_masks_time.py [--out profiles/term_masks/c3.jsonl] [--commit ID]

Builds config 3 (bm25mi.synth: 10M documents), takes the batch of 1024
synthetic queries and gives every query a clause row drawn from its own
tokens: its first two valid ids as ``must``, its third as ``must_not``.  Times
between HIP events, alternating the two calls in one process (--warmup rounds,
then --steps rounds; medians are reported):

  * term_masks_device: 1024 masks of W = ceil(n_docs / 32) words;
  * search_filtered_device, k = 100, on the masks it produced (query q under
    mask q) — existing code, the comparison point.

Beside the times: the bytes written (M * W * 4), the ldoc bytes of the clause
terms' posting lists (2 B per posting; an upper bound of the ldoc bytes read,
since tiles whose must terms have an empty segment read no posting), the
GB/s both give over the mask build, and the masks' allowed documents.  The
masks of the first --check rows are compared with a numpy build from the CSC
arrays.  Writes one JSON line.
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


def _stats(ms):
    return {"ms": round(statistics.median(ms), 4), "min": round(min(ms), 4),
            "max": round(max(ms), 4)}


def clause_rows(q):
    """must [Q, 2], must_not [Q, 1] from each query's first three valid ids."""
    Q = q.shape[0]
    must = np.full((Q, 2), -1, np.int32)
    must_not = np.full((Q, 1), -1, np.int32)
    for r in range(Q):
        ids = q[r][q[r] >= 0][:3]
        must[r, :min(2, len(ids))] = ids[:2]
        if len(ids) > 2:
            must_not[r, 0] = ids[2]
    return must, must_not


def numpy_mask(ip, ix, n_docs, must, must_not):
    import bm25mi
    ok = np.ones(n_docs, bool)
    for t in must[must >= 0]:
        has = np.zeros(n_docs, bool)
        has[ix[ip[t]:ip[t + 1]]] = True
        ok &= has
    for t in must_not[must_not >= 0]:
        ok[ix[ip[t]:ip[t + 1]]] = False
    return bm25mi.pack_mask(ok)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", type=int, default=4, help="mask rows compared with numpy")
    ap.add_argument("--threads", type=int, default=16, help="host threads for index generation")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "term_masks", "c3.jsonl"))
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
    del dt
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    q = synth.make_queries(cfg)
    Q, T, k, N = q.shape[0], q.shape[1], cfg.k, cfg.n_docs
    W = (N + 31) // 32
    must, must_not = clause_rows(q)
    df = np.diff(ip)
    ldoc_bytes = int(2 * (df[must[must >= 0]].sum() + df[must_not[must_not >= 0]].sum()))
    dq = torch.from_numpy(q).to(dev)
    dmu = torch.from_numpy(must).to(dev)
    dmn = torch.from_numpy(must_not).to(dev)
    dm = torch.empty((Q, W), dtype=torch.int32, device=dev)
    fd = torch.empty((Q, k), dtype=torch.int32, device=dev)
    fs = torch.empty((Q, k), dtype=torch.float32, device=dev)
    dqm = torch.arange(Q, dtype=torch.int32, device=dev)

    build = lambda: index.term_masks_device(dmu, None, dmn, None, dm, st)
    search = lambda: index.search_filtered_device(dq, k, dm, dqm, fd, fs, st)
    for _ in range(args.warmup):
        build()
        search()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.steps)]
    for e in ev:  # alternating, one process
        e[0].record(st)
        build()
        e[1].record(st)
        search()
        e[2].record(st)
    torch.cuda.synchronize()
    t_build = _stats([e[0].elapsed_time(e[1]) for e in ev])
    t_search = _stats([e[1].elapsed_time(e[2]) for e in ev])
    dense, skipped, rescored = index.filtered_stats()

    masks = dm.cpu().numpy().view(np.uint32)
    for r in range(min(args.check, Q)):
        assert np.array_equal(masks[r], numpy_mask(ip, ix, N, must[r], must_not[r])), r
    allowed = np.unpackbits(masks[:64].view(np.uint8), axis=1).sum(axis=1)
    out_bytes = Q * W * 4
    s = t_build["ms"] * 1e-3
    rec = {"config": args.config, "commit": args.commit or _commit(), "M": Q, "T": T, "k": k,
           "n_docs": N, "W": W, "n_tiles": index.info()["n_tiles"],
           "segments_sparse": index.info()["sparse"], "steps": args.steps, "warmup": args.warmup,
           "term_masks_device": t_build, "search_filtered_device": t_search,
           "search_dense_queries": dense, "search_skipped_pairs": skipped,
           "search_rescored_pairs": rescored,
           "bytes_written": out_bytes, "ldoc_bytes_upper_bound": ldoc_bytes,
           "write_GBps": round(out_bytes / s / 1e9, 1),
           "write_plus_ldoc_GBps": round((out_bytes + ldoc_bytes) / s / 1e9, 1),
           "build_over_search": round(t_build["ms"] / t_search["ms"], 3),
           "allowed_docs_first_64_masks": {"min": int(allowed.min()),
                                           "median": int(np.median(allowed)),
                                           "max": int(allowed.max())},
           "checked_rows": min(args.check, Q)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)
    index.close()


if __name__ == "__main__":
    main()
