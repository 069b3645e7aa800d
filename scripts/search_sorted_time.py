"""Time the sort-by-field search (bm25_sort_ranks_device,
bm25_search_sorted_device, bm25_search_boolean_sorted) at config 3's size (GPU
box).

  python scripts/search_sorted_time.py [--out profiles/sorted/c3.jsonl] [--commit ID]
                                       [--full-index]

A handle over config 3's 10M documents (bm25mi.synth), a random int32 column
(a timestamp: about 1000 documents per value), --rows mask rows (1024) and k =
100.  Records, one JSON line each:

  rank_build     bm25_sort_ranks_device per kind and direction, by a host clock
                 (the call synchronises its stream); the int32 descending order
                 is compared with np.lexsort
  search_sorted  bm25_search_sorted_device between HIP events (--warmup rounds,
                 then --steps rounds; the median), on masks of density 100 %,
                 10 % and 0.1 % and on a contiguous-rank mask (a range filter on
                 the sorted field: a tenth of the ranks, another tenth per row);
                 row 0 is compared with numpy
  boolean_sorted the one-call search_boolean(sort=...) from host arrays, by a
                 host clock: no clause (every document), and with --full-index
                 each query's first term as its must clause

Beside each search_sorted time, yardsticks that are not the code under test:

  bytes    the selection streams levels + 1 passes of the mask words (M * W * 4
           each) and, per pass and block of 32 rows, the ranks (n_docs * 4);
           GBps_masks is the mask words alone over the time, GBps the two
  torch    what a caller can do today on the same box: unpack a device mask row
           and torch.where(mask, rank, INT_MAX).topk(k, largest=False), row by
           row (--torch-rows of them; torch_ms_all_rows scales to all rows)
  filtered bm25_search_filtered_device on the same masks with config 3's
           queries, which scores as well (--full-index only: it needs the
           postings)
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

ROWS, BINS, WMAX = 32, 256, 2048   # kSortedRows, kSortedBins, kSortedWmax (bm25mi_internal.h)


def _commit():
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], check=True,
                              capture_output=True, text=True).stdout.strip()
    except Exception:
        return "unknown"


def _timed(torch, st, f, warmup, steps):
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(steps)]
    for a, b in ev:
        a.record(st)
        f()
        b.record(st)
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    return {"ms": round(statistics.median(ms), 4), "min": round(min(ms), 4),
            "max": round(max(ms), 4)}


def _host_timed(torch, f, warmup, steps):
    for _ in range(warmup):
        f()
    ms = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ms.append(1000.0 * (time.perf_counter() - t0))
    return {"ms": round(statistics.median(ms), 3), "min": round(min(ms), 3),
            "max": round(max(ms), 3)}


def levels_of(n, bins=BINS):
    """Histogram levels of the selection at n documents (launch_search_sorted)."""
    levels, width = 0, n
    while width > WMAX:
        shift = 0
        while (bins << shift) < width:
            shift += 1
        width = 1 << shift
        levels += 1
    return levels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--density", type=float, nargs="*", default=[1.0, 0.1, 0.001])
    ap.add_argument("--torch-rows", type=int, default=16, help="rows the torch yardstick runs")
    ap.add_argument("--full-index", action="store_true")
    ap.add_argument("--threads", type=int, default=16, help="host threads for index generation")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sorted", "c3.jsonl"))
    ap.add_argument("--commit", default=None, help="label of the measured code (default: git HEAD)")
    args = ap.parse_args()
    import torch
    from bm25mi import synth
    from bm25mi.index import GpuIndex
    if not torch.cuda.is_available():
        sys.exit("no GPU: this script measures, it has no CPU path")
    cfg = synth.CONFIGS[args.config]
    N, M, k = cfg.n_docs, args.rows, args.k
    if args.full_index:
        ip, ix, dt = synth.make_index(cfg, threads=args.threads)
        index = GpuIndex(ip, ix, dt, N)
        del ip, ix, dt
    else:
        index = GpuIndex(np.array([0, 1], np.int64), np.zeros(1, np.int32),
                         np.ones(1, np.float32), N)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    W = (N + 31) // 32
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    shifts = torch.arange(32, dtype=torch.int32, device=dev)
    commit = args.commit or _commit()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")
    common = {"config": args.config, "commit": commit, "n_docs": N, "W": W,
              "full_index": args.full_index, "steps": args.steps, "warmup": args.warmup}

    def emit(rec):
        rec = dict(common, **rec)
        out.write(json.dumps(rec) + "\n")
        out.flush()
        print(json.dumps(rec), flush=True)

    # ---- the rank build
    stamp = torch.randint(0, max(2, N // 1000), (N,), dtype=torch.int32, device=dev, generator=gen)
    dr = torch.empty(N, dtype=torch.int32, device=dev)
    dp = torch.empty(N, dtype=torch.int32, device=dev)
    for name, col in (("int32", stamp), ("float32", stamp.to(torch.float32) / 7),
                      ("int64", stamp.to(torch.int64) << 20)):
        for desc in (False, True):
            t = _host_timed(torch, lambda: index.sort_ranks_device(col, dr, dp, desc, st), 1, 3)
            emit({"what": "rank_build", "kind": name, "descending": desc, "sort_ranks_device": t,
                  "scratch_bytes_per_doc": 24})
    index.sort_ranks_device(stamp, dr, dp, True, st)   # newest first: the order of what follows
    ranks, perm = dr.cpu().numpy(), dp.cpu().numpy()
    v = stamp.cpu().numpy()
    want_perm = np.lexsort((np.arange(N), -v.astype(np.int64)))
    assert np.array_equal(perm, want_perm) and np.array_equal(ranks[perm], np.arange(N))

    # ---- the masks
    def pack(bits):                 # bool [n, N] on the device -> int32 [n, W]
        pad = torch.zeros((bits.shape[0], W * 32), dtype=torch.int32, device=dev)
        pad[:, :N] = bits
        return (pad.view(-1, W, 32) << shifts).sum(dim=2, dtype=torch.int32)

    def make_masks(what):
        if what == 1.0:
            return torch.full((M, W), -1, dtype=torch.int32, device=dev)
        dm = torch.empty((M, W), dtype=torch.int32, device=dev)
        for m0 in range(0, M, 8):     # (8 rows of 10M bits at a time)
            n = min(8, M - m0)
            if what == "contiguous":   # ranks [a, a + N / 10), a by the row
                a = (torch.arange(m0, m0 + n, device=dev) * 7919 % 9) * (N // 10)
                bits = (dr[None, :] >= a[:, None]) & (dr[None, :] < a[:, None] + N // 10)
            else:
                bits = torch.rand((n, N), device=dev, generator=gen) < what
            dm[m0:m0 + n] = pack(bits)
        return dm

    levels = levels_of(N)
    blocks = (M + ROWS - 1) // ROWS
    need = index.sorted_scratch_bytes(M, k)
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    dd = torch.empty((M, k), dtype=torch.int32, device=dev)
    do = torch.empty((M, k), dtype=torch.int32, device=dev)
    if args.full_index:
        dq = torch.from_numpy(synth.make_queries(cfg, n_queries=M)).to(dev)
        dqm = torch.arange(M, dtype=torch.int32, device=dev)
        ds = torch.empty((M, k), dtype=torch.float32, device=dev)
    big = torch.iinfo(torch.int32).max
    for what in list(args.density) + ["contiguous"]:
        dm = make_masks(what)
        t = _timed(torch, st, lambda: index.search_sorted_device(dm, dr, dp, k, None, dd, do,
                                                                 scratch, st),
                   args.warmup, args.steps)
        row0 = dm[0].cpu().numpy().view(np.uint32)
        bits0 = np.unpackbits(row0.view(np.uint8), bitorder="little")[:N].astype(bool)
        r0 = np.sort(ranks[bits0])[:k]
        got_d, got_r = dd[0].cpu().numpy(), do[0].cpu().numpy()
        assert np.array_equal(got_r[:r0.size], r0) and (got_r[r0.size:] == -1).all(), what
        assert np.array_equal(got_d[:r0.size], perm[r0]), what
        mask_bytes = (levels + 1) * M * W * 4
        rank_bytes = (levels + 1) * blocks * N * 4
        rec = {"what": "search_sorted", "mask": what, "M": M, "k": k, "levels": levels,
               "passes": levels + 1, "scratch_bytes": need, "search_sorted_device": t,
               "mask_bytes": mask_bytes, "rank_bytes": rank_bytes,
               "GBps_masks": round(mask_bytes / (t["ms"] * 1e-3) / 1e9, 1),
               "GBps": round((mask_bytes + rank_bytes) / (t["ms"] * 1e-3) / 1e9, 1)}
        rows = min(args.torch_rows, M)

        def by_torch():
            for m in range(rows):
                allowed = ((dm[m][:, None] >> shifts) & 1).reshape(-1)[:N].bool()
                val, _ = torch.where(allowed, dr, big).topk(k, largest=False)
                do[m] = val
        rec["torch_where_topk"] = dict(_timed(torch, st, by_torch, 1, min(args.steps, 3)),
                                       rows=rows)
        tr = np.sort(do[0].cpu().numpy())
        assert np.array_equal(tr[:r0.size], r0), ("torch", what)
        rec["torch_ms_all_rows"] = round(rec["torch_where_topk"]["ms"] * M / rows, 2)
        rec["speedup_vs_torch"] = round(rec["torch_ms_all_rows"] / t["ms"], 1)
        if args.full_index:
            rec["search_filtered_device"] = _timed(
                torch, st, lambda: index.search_filtered_device(dq, k, dm, dqm, dd, ds, st),
                args.warmup, args.steps)
        emit(rec)
        del dm
    del scratch

    # ---- the one-call search from host arrays
    q = synth.make_queries(cfg, n_queries=M) if args.full_index else np.zeros((M, 1), np.int32)
    cases = [("no clause", None)]
    if args.full_index:
        cases.append(("must = first query term", [[int(t)] for t in q[:, 0]]))
    for name, must in cases:
        t = _host_timed(torch, lambda: index.search_boolean(q, k, must, sort=(ranks, perm)), 1, 3)
        t0 = _host_timed(torch, lambda: index.search_boolean(q, k, must), 1, 3)
        emit({"what": "boolean_sorted", "clauses": name, "Q": M, "k": k,
              "search_boolean_sort": t, "search_boolean_by_score": t0,
              "order_upload_bytes": 8 * N})
    out.close()
    index.close()


if __name__ == "__main__":
    main()
