"""Time the counting any clause (bm25_term_masks_min_match_device) and the hit
count (bm25_mask_count_device) on config 3 (GPU box).

  python scripts/min_match_time.py [--out profiles/min_match/c3.jsonl] [--commit ID]

Builds config 3 (bm25mi.synth: 10M documents), takes the batch of 1024
synthetic queries and gives every query one clause row: ``any`` = the query's
valid ids (padding kept as padding).  Times between HIP events, the five calls
in turn in one process (--warmup rounds, then --steps rounds; medians are
reported):

  (a) term_masks_device, no min_match: the existing kernel, the comparison point;
  (b) term_masks_device, d_min_match all 1: the counting instantiation on its
      shared-bitmap branch;
  (c) d_min_match all 2;
  (d) d_min_match = "75%" of each row's terms (bm25mi.min_match_rows);
  (e) mask_count_device on the masks of (c).

Beside the times: the bytes written (M * W * 4), the ldoc bytes of the clause
terms' posting lists (2 B per posting; an upper bound of the ldoc bytes read:
a tile where fewer than min_match terms have a segment reads no posting), the
need per row, and the allowed documents of the first 64 masks of each build.
The masks of the first --check rows of (b), (c) and (d), and their counts, are
compared with a numpy build from the CSC arrays; (b) must equal (a) word for
word.  Writes one JSON line.
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


def numpy_mask(ip, ix, n_docs, any_row, need):
    import bm25mi
    ids = any_row[any_row >= 0]
    if len(ids) == 0 or need <= 0:
        return bm25mi.pack_mask(np.ones(n_docs, bool))[0]
    count = np.zeros(n_docs, np.int32)
    for t in ids:
        count[ix[ip[t]:ip[t + 1]]] += 1
    return bm25mi.pack_mask(count >= need)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", type=int, default=4, help="mask rows compared with numpy")
    ap.add_argument("--threads", type=int, default=16, help="host threads for index generation")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "min_match", "c3.jsonl"))
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
    del dt
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    q = synth.make_queries(cfg)
    Q, T, N = q.shape[0], q.shape[1], cfg.n_docs
    W = (N + 31) // 32
    any_rows = np.ascontiguousarray(q, dtype=np.int32)
    any_rows[any_rows >= len(ip) - 1] = -1
    needs = {"min_match_1": np.ones(Q, np.int32), "min_match_2": np.full(Q, 2, np.int32),
             "min_match_75pct": bm25mi.min_match_rows(any_rows, "75%")}
    df = np.diff(ip)
    ldoc_bytes = int(2 * df[any_rows[any_rows >= 0]].sum())
    dan = torch.from_numpy(any_rows).to(dev)
    dmm = {n: torch.from_numpy(v).to(dev) for n, v in needs.items()}
    dm = torch.empty((Q, W), dtype=torch.int32, device=dev)
    dm2 = torch.empty((Q, W), dtype=torch.int32, device=dev)   # the masks of (c), kept for (e)
    dc = torch.empty(Q, dtype=torch.int64, device=dev)

    calls = [("term_masks_device", lambda: index.term_masks_device(None, dan, None, None, dm, st))]
    for n in needs:
        out = dm2 if n == "min_match_2" else dm
        calls.append((n, lambda n=n, out=out: index.term_masks_device(
            None, dan, None, None, out, st, d_min_match=dmm[n])))
    calls.append(("mask_count_device", lambda: index.mask_count_device(dm2, dc, st)))
    for _ in range(args.warmup):
        for _, f in calls:
            f()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(calls) + 1)]
          for _ in range(args.steps)]
    for e in ev:  # the calls in turn, one process
        e[0].record(st)
        for i, (_, f) in enumerate(calls):
            f()
            e[i + 1].record(st)
    torch.cuda.synchronize()
    times = {n: _stats([e[i].elapsed_time(e[i + 1]) for e in ev]) for i, (n, _) in enumerate(calls)}

    # checks, and the allowed documents of each build
    allowed = {}
    calls[0][1]()
    torch.cuda.synchronize()
    old = dm.cpu().numpy().view(np.uint32).copy()
    nchk = min(args.check, Q)
    for n, need in needs.items():
        out = dm2 if n == "min_match_2" else dm
        index.term_masks_device(None, dan, None, None, out, st, d_min_match=dmm[n])
        index.mask_count_device(out, dc, st)
        torch.cuda.synchronize()
        masks = out.cpu().numpy().view(np.uint32)
        counts = dc.cpu().numpy()
        if n == "min_match_1":
            assert np.array_equal(masks, old), "min_match 1 differs from bm25_term_masks_device"
        for r in range(nchk):
            want = numpy_mask(ip, ix, N, any_rows[r], int(need[r]))
            assert np.array_equal(masks[r], want), (n, r)
            bits = int(np.unpackbits(want.view(np.uint8)).sum())
            assert int(counts[r]) == bits, (n, r, int(counts[r]), bits)
        a = counts[:64]
        allowed[n] = {"min": int(a.min()), "median": int(np.median(a)), "max": int(a.max())}
    out_bytes = Q * W * 4
    n_any = (any_rows >= 0).sum(axis=1)
    rec = {"config": args.config, "commit": args.commit or _commit(), "M": Q, "T": T,
           "n_docs": N, "W": W, "n_tiles": index.info()["n_tiles"],
           "segments_sparse": index.info()["sparse"], "steps": args.steps, "warmup": args.warmup,
           **times,
           "n_any": {"min": int(n_any.min()), "median": int(np.median(n_any)),
                     "max": int(n_any.max())},
           "need_75pct": {"min": int(needs["min_match_75pct"].min()),
                          "median": int(np.median(needs["min_match_75pct"])),
                          "max": int(needs["min_match_75pct"].max())},
           "bytes_written": out_bytes, "ldoc_bytes_upper_bound": ldoc_bytes,
           "write_plus_ldoc_GBps": {n: round((out_bytes + ldoc_bytes) / (times[n]["ms"] * 1e-3) / 1e9, 1)
                                    for n in ["term_masks_device"] + list(needs)},
           "mask_count_read_GBps": round(out_bytes / (times["mask_count_device"]["ms"] * 1e-3) / 1e9, 1),
           "allowed_docs_first_64_masks": allowed, "checked_rows": nchk}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)
    index.close()


if __name__ == "__main__":
    main()
