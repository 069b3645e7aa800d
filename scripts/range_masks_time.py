"""Time the numeric range filters (bm25_range_masks_device) at config 3's size (GPU box).

  python scripts/range_masks_time.py [--out profiles/range_masks/c3.jsonl] [--commit ID]

A handle over config 3's 10M documents (bm25mi.synth) on a one-posting index
(the range calls read the caller's buffers only), C columns of uniform random
values in [0, 10^6); for M in {1, 64, 1024} rows, C in {1, 2} clauses a row
(each on a column of its own), int32 and int64 columns and a selectivity of
1 %, 50 % and 100 % (each clause lets selectivity^(1/C) through; the rows'
ranges start at different values) the call is timed between HIP events
(--warmup rounds, then --steps rounds; the median is reported).  No base.

Beside each time, two yardsticks that are not the code under test:

  bytes   what the call must move: the C columns once per row block
          (ceil(M / 64) * C * n_docs * 4 or 8) and the output (M * W * 4), and
          the GB/s that gives;
  torch   what a user of the previous commit would do on the same box:
          (v >= lo) & (v <= hi) per clause on the device with torch, packed to
          32-bit words, row by row (for M <= --torch-rows); and, for one row,
          the host route: the numpy compare, bm25mi.pack_mask and the upload
          of the packed row (wall clock).

Row 0 of every case is compared with numpy.  Writes one JSON line per case.
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

ROWS = 64          # kRangeRows (bm25mi_internal.h)
SPAN = 1_000_000   # the values lie in [0, SPAN)


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


def _wall(torch, f, warmup, steps):
    ms = []
    for i in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms": round(statistics.median(ms), 4), "min": round(min(ms), 4),
            "max": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, nargs="*", default=[1, 64, 1024])
    ap.add_argument("--clauses", type=int, nargs="*", default=[1, 2])
    ap.add_argument("--kinds", nargs="*", default=["int32", "int64"])
    ap.add_argument("--selectivity", type=float, nargs="*", default=[0.01, 0.5, 1.0])
    ap.add_argument("--torch-rows", type=int, default=64, help="largest M the torch yardstick runs")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "range_masks", "c3.jsonl"))
    ap.add_argument("--commit", default=None, help="label of the measured code (default: git HEAD)")
    args = ap.parse_args()
    import torch
    import bm25mi
    from bm25mi import synth
    from bm25mi.index import GpuIndex
    if not torch.cuda.is_available():
        sys.exit("no GPU: this script measures, it has no CPU path")
    N = synth.CONFIGS[args.config].n_docs
    index = GpuIndex(np.array([0, 1], np.int64), np.zeros(1, np.int32), np.ones(1, np.float32), N)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    W = (N + 31) // 32
    Mmax, Cmax = max(args.rows), max(args.clauses)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    shifts = torch.arange(32, dtype=torch.int32, device=dev)
    commit = args.commit or _commit()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")
    d_out = torch.empty((Mmax, W), dtype=torch.int32, device=dev)
    pad = torch.zeros(W * 32, dtype=torch.bool, device=dev)

    def torch_row(dv, lo, hi, m, C):
        ok = (dv[0] >= lo[m, 0]) & (dv[0] <= hi[m, 0])
        for c in range(1, C):
            ok &= (dv[c] >= lo[m, c]) & (dv[c] <= hi[m, c])
        pad[:N] = ok
        return (pad.view(W, 32).to(torch.int32) << shifts).sum(dim=1, dtype=torch.int32)

    for kind in args.kinds:
        tdt = {"int32": torch.int32, "int64": torch.int64}[kind]
        dv = torch.randint(0, SPAN, (Cmax, N), dtype=tdt, device=dev, generator=gen)
        hv = dv.cpu().numpy()
        for C in args.clauses:
            for p in args.selectivity:
                width = max(1, round(SPAN * p ** (1.0 / C)))
                start = (np.arange(Mmax)[:, None] * 7919 + np.arange(C)[None, :] * 104729) % (
                    SPAN - width + 1)
                lo = torch.from_numpy(start.astype(hv.dtype)).to(dev)
                hi = torch.from_numpy((start + width - 1).astype(hv.dtype)).to(dev)
                fields = torch.arange(C, dtype=torch.int32, device=dev).repeat(Mmax, 1).contiguous()
                ok0 = np.ones(N, bool)
                for c in range(C):
                    ok0 &= (hv[c] >= start[0, c]) & (hv[c] <= start[0, c] + width - 1)
                want0 = bm25mi.pack_mask(ok0)[0]
                for M in args.rows:
                    call = lambda: index.range_masks_device(  # noqa: E731
                        dv[:C], fields[:M], lo[:M].contiguous(), hi[:M].contiguous(), d_out[:M],
                        None, st)
                    t = _timed(torch, st, call, args.warmup, args.steps)
                    got0 = d_out[0].cpu().numpy().view(np.uint32)
                    assert np.array_equal(got0, want0), (kind, C, p, M)
                    blocks = (M + ROWS - 1) // ROWS
                    nbytes = blocks * C * N * hv.dtype.itemsize + M * W * 4
                    rec = {"config": args.config, "commit": commit, "n_docs": N, "W": W, "M": M,
                           "C": C, "kind": kind, "selectivity": p,
                           "hits_row0": int(ok0.sum()), "row_blocks": blocks, "steps": args.steps,
                           "warmup": args.warmup, "range_masks_device": t, "bytes": nbytes,
                           "GBps": round(nbytes / (t["ms"] * 1e-3) / 1e9, 1)}
                    if M <= args.torch_rows:
                        def by_torch():
                            for m in range(M):
                                d_out[m] = torch_row(dv, lo, hi, m, C)
                        rec["torch_compare_pack"] = _timed(torch, st, by_torch, 1,
                                                           min(args.steps, 3))
                        got0 = d_out[0].cpu().numpy().view(np.uint32)
                        assert np.array_equal(got0, want0), ("torch", kind, C, p, M)
                        rec["speedup_vs_torch"] = round(
                            rec["torch_compare_pack"]["ms"] / t["ms"], 1)
                    if M == 1:
                        def by_host():
                            ok = (hv[0] >= start[0, 0]) & (hv[0] <= start[0, 0] + width - 1)
                            for c in range(1, C):
                                ok &= (hv[c] >= start[0, c]) & (hv[c] <= start[0, c] + width - 1)
                            d_out[0] = torch.from_numpy(
                                bm25mi.pack_mask(ok)[0].view(np.int32)).to(dev)
                        rec["numpy_pack_upload"] = _wall(torch, by_host, 1, min(args.steps, 3))
                        rec["speedup_vs_host"] = round(rec["numpy_pack_upload"]["ms"] / t["ms"], 1)
                    out.write(json.dumps(rec) + "\n")
                    out.flush()
                    print(json.dumps(rec), flush=True)
        del dv
    out.close()
    index.close()


if __name__ == "__main__":
    main()
