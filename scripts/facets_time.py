"""Time the facet counts (bm25_mask_facets_device) at config 3's size (GPU box).

  python scripts/facets_time.py [--out profiles/facets/c3.jsonl] [--commit ID] [--full-index]

A handle over config 3's 10M documents (bm25mi.synth), random group ids (no
negative ones) and random masks of density 1 %, 50 % and 100 %; for M in
{1, 64, 1024} rows and G in {16, 256, 8192 (the last LDS shape), 65536 (the
global-atomic route)} the call is timed between HIP events (--warmup rounds,
then --steps rounds; the median is reported).  The facet calls read the
caller's masks and groups only, so by default the handle holds config 3's
document count over a one-posting index; --full-index builds the real one.

Beside each time, two yardsticks that are not the code under test:

  bytes   what the call must move: the groups once per row block
          (ceil(M / R) * n_docs * 4), the masks (M * W * 4) and the output
          (M * G * 8), and the GB/s that gives;
  torch   what a user of the previous commit would do on the same box: unpack
          a device mask row with torch and torch.bincount the allowed
          documents' groups, row by row (for M <= --torch-rows).

Row 0 of every (G, density) is compared with numpy.  Writes one JSON line per
case.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "mojo-bm25_amd"), REPO):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

BINS, MAXROWS = 8192, 64   # kFacetBins, kFacetMaxRows (bm25mi_internal.h)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, nargs="*", default=[1, 64, 1024])
    ap.add_argument("--groups", type=int, nargs="*", default=[16, 256, BINS, 65536])
    ap.add_argument("--density", type=float, nargs="*", default=[0.01, 0.5, 1.0])
    ap.add_argument("--torch-rows", type=int, default=64, help="largest M the torch yardstick runs")
    ap.add_argument("--full-index", action="store_true")
    ap.add_argument("--threads", type=int, default=16, help="host threads for index generation")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "facets", "c3.jsonl"))
    ap.add_argument("--commit", default=None, help="label of the measured code (default: git HEAD)")
    args = ap.parse_args()
    import torch
    from bm25mi import synth
    from bm25mi.index import GpuIndex
    if not torch.cuda.is_available():
        sys.exit("no GPU: this script measures, it has no CPU path")
    cfg = synth.CONFIGS[args.config]
    N = cfg.n_docs
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
    Mmax = max(args.rows)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    shifts = torch.arange(32, dtype=torch.int32, device=dev)
    commit = args.commit or _commit()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")

    def make_masks(p):
        """[Mmax, W] packed words, each bit set with probability p."""
        if p >= 1.0:
            return torch.full((Mmax, W), -1, dtype=torch.int32, device=dev)
        dm = torch.zeros((Mmax, W), dtype=torch.int32, device=dev)
        for m0 in range(0, Mmax, 8):      # (8 rows of 10M random bits at a time)
            n = min(8, Mmax - m0)
            bits = (torch.rand((n, W, 32), device=dev, generator=gen) < p).to(torch.int32)
            dm[m0:m0 + n] = (bits << shifts).sum(dim=2, dtype=torch.int32)
        return dm

    def torch_row(words, dg, G):
        allowed = ((words[:, None] >> shifts) & 1).reshape(-1)[:N].bool()
        return torch.bincount(dg[allowed], minlength=G)

    for p in args.density:
        dm = make_masks(p)
        for G in args.groups:
            dg = torch.randint(0, G, (N,), dtype=torch.int32, device=dev, generator=gen)
            row0 = dm[0].cpu().numpy().view(np.uint32)
            bits = np.unpackbits(row0.view(np.uint8), bitorder="little")[:N].astype(bool)
            want0 = np.bincount(dg.cpu().numpy()[bits], minlength=G)
            for M in args.rows:
                dc = torch.empty((M, G), dtype=torch.int64, device=dev)
                t = _timed(torch, st, lambda: index.facets_device(dm[:M], dg, G, dc, st),
                           args.warmup, args.steps)
                assert np.array_equal(dc[0].cpu().numpy(), want0), (p, G, M)
                R = 1 if G > BINS else min(MAXROWS, BINS // G)
                blocks = (M + R - 1) // R
                nbytes = blocks * N * 4 + M * W * 4 + M * G * 8
                rec = {"config": args.config, "commit": commit, "n_docs": N, "W": W,
                       "full_index": args.full_index, "M": M, "G": G, "density": p,
                       "route": "global" if G > BINS else "lds", "R": R, "row_blocks": blocks,
                       "steps": args.steps, "warmup": args.warmup, "facets_device": t,
                       "bytes": nbytes, "GBps": round(nbytes / (t["ms"] * 1e-3) / 1e9, 1)}
                if M <= args.torch_rows:
                    def by_torch():
                        for m in range(M):
                            dc[m] = torch_row(dm[m], dg, G)
                    rec["torch_unpack_bincount"] = _timed(torch, st, by_torch, 1,
                                                          min(args.steps, 3))
                    assert np.array_equal(dc[0].cpu().numpy(), want0), ("torch", p, G, M)
                    rec["speedup_vs_torch"] = round(
                        rec["torch_unpack_bincount"]["ms"] / t["ms"], 1)
                out.write(json.dumps(rec) + "\n")
                out.flush()
                print(json.dumps(rec), flush=True)
                del dc
            del dg
        del dm
    out.close()
    index.close()


if __name__ == "__main__":
    main()
