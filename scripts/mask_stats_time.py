"""Time the field statistics (bm25_mask_stats_device) at config 3's size (GPU box).

  python scripts/mask_stats_time.py [--out profiles/stats/c3.jsonl] [--commit ID]

A handle over config 3's 10M documents (a one-posting index: the stats calls
read the caller's buffers only), random masks of density 50 % and 1 %, a
float32 column (log-normal "prices" of both signs) and an int64 column
("timestamps").  For M in {1, 64} rows and each density: float32 and int64
ungrouped, float32 at G = 16 (the LDS route) and at G = 100 000 (the
global-atomic route).  The call — scratch clear, accumulate pass, finalise
pass, all four outputs — is timed between HIP events (--warmup rounds, then
--steps rounds; the median is reported).  The same call over all-zero masks
(no column read, no update: the scratch clear, the mask words and the finalise
pass) is timed beside it, to show where the time goes.

Beside each time, two figures for the same shape that are not the code under
test:

  facets  bm25_mask_facets_device on the same masks and G (ungrouped: G = 1
          over groups of zeros): the nearest existing kernel;
  floor   the bytes the call cannot avoid — the column, the groups and the
          M * W mask words — over 6.29 TB/s, the streaming copy rate of the
          device (MI355X_MICROARCH.md).

Row 0 of every case is compared with numpy (count, min, max, integer sum) and,
ungrouped float32, with math.fsum bit for bit.  Writes one JSON line per case.
"""
import argparse
import json
import math
import os
import struct
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "mojo-bm25_amd"), REPO, os.path.join(REPO, "scripts")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

from facets_time import _commit, _timed  # noqa: E402

COPY_RATE = 6.29e12   # bytes per second of a streaming copy (MI355X_MICROARCH.md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, nargs="*", default=[1, 64])
    ap.add_argument("--density", type=float, nargs="*", default=[0.5, 0.01])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "stats", "c3.jsonl"))
    ap.add_argument("--commit", default=None, help="label of the measured code (default: git HEAD)")
    args = ap.parse_args()
    import torch
    from bm25mi import synth
    from bm25mi.index import GpuIndex
    if not torch.cuda.is_available():
        sys.exit("no GPU: this script measures, it has no CPU path")
    N = synth.CONFIGS[args.config].n_docs
    index = GpuIndex(np.array([0, 1], np.int64), np.zeros(1, np.int32), np.ones(1, np.float32), N)
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

    sign = torch.where(torch.rand(N, device=dev, generator=gen) < 0.1, -1.0, 1.0)
    f32 = (torch.exp(3.0 + 1.5 * torch.randn(N, device=dev, generator=gen)) * sign).float()
    i64 = torch.randint(1_500_000_000_000, 1_800_000_000_000, (N,), dtype=torch.int64,
                        device=dev, generator=gen)
    zeros = torch.zeros(N, dtype=torch.int32, device=dev)
    no_docs = torch.zeros((Mmax, W), dtype=torch.int32, device=dev)   # all-zero masks
    cases = [("float32", f32, 0), ("int64", i64, 0), ("float32", f32, 16), ("float32", f32, 100_000)]

    for p in args.density:
        dm = torch.zeros((Mmax, W), dtype=torch.int32, device=dev)
        for m0 in range(0, Mmax, 8):      # (8 rows of 10M random bits at a time)
            n = min(8, Mmax - m0)
            bits = (torch.rand((n, W, 32), device=dev, generator=gen) < p).to(torch.int32)
            dm[m0:m0 + n] = (bits << shifts).sum(dim=2, dtype=torch.int32)
        row0 = dm[0].cpu().numpy().view(np.uint32)
        allowed0 = np.unpackbits(row0.view(np.uint8), bitorder="little")[:N].astype(bool)
        for name, dv, G in cases:
            B = G or 1
            dg = (torch.randint(0, G, (N,), dtype=torch.int32, device=dev, generator=gen)
                  if G else None)
            v0 = dv.cpu().numpy()[allowed0]
            g0 = dg.cpu().numpy()[allowed0] if G else None
            for M in args.rows:
                sum_dt = torch.float64 if dv.dtype == torch.float32 else torch.int64
                dc = torch.empty((M, B), dtype=torch.int64, device=dev)
                dlo = torch.empty((M, B), dtype=dv.dtype, device=dev)
                dhi = torch.empty((M, B), dtype=dv.dtype, device=dev)
                dsum = torch.empty((M, B), dtype=sum_dt, device=dev)
                nscr = index.stats_scratch_bytes(v0.dtype, M, G)
                scr = torch.empty(nscr, dtype=torch.uint8, device=dev)
                t = _timed(torch, st, lambda: index.stats_device(dm[:M], dv, dc, dlo, dhi, dsum,
                                                                 dg, G, scr, st),
                           args.warmup, args.steps)
                # row 0 against numpy
                cnt = dc[0].cpu().numpy()
                if G:
                    assert np.array_equal(cnt, np.bincount(g0, minlength=G)), (name, G, M, p)
                else:
                    assert cnt[0] == v0.size, (name, M, p)
                    assert dlo[0, 0].item() == v0.min() and dhi[0, 0].item() == v0.max()
                    if name == "int64":
                        assert dsum[0, 0].item() == int(v0.sum(dtype=np.int64))
                    else:
                        want = math.fsum(v0.astype(np.float64).tolist())
                        assert struct.pack("<d", dsum[0, 0].item()) == struct.pack("<d", want)
                # the same call over all-zero masks: the scratch clear, the mask
                # words and the finalise pass, with no column read and no update
                te = _timed(torch, st, lambda: index.stats_device(no_docs[:M], dv, dc, dlo, dhi,
                                                                  dsum, dg, G, scr, st),
                            args.warmup, args.steps)
                assert int(dc.sum().item()) == 0
                fg = dg if G else zeros
                fc = torch.empty((M, B), dtype=torch.int64, device=dev)
                tf = _timed(torch, st, lambda: index.facets_device(dm[:M], fg, B, fc, st),
                            args.warmup, args.steps)
                assert np.array_equal(fc[0].cpu().numpy(),
                                      np.bincount(g0, minlength=G) if G else [allowed0.sum()])
                floor_bytes = N * dv.element_size() + (N * 4 if G else 0) + M * W * 4
                floor_ms = floor_bytes / COPY_RATE * 1e3
                rec = {"config": args.config, "commit": commit, "n_docs": N, "W": W, "M": M,
                       "G": G, "dtype": name, "density": p,
                       "route": "global" if B > (128 if name == "float32" else 1152) else "lds",
                       "scratch_bytes": nscr, "steps": args.steps, "warmup": args.warmup,
                       "stats_device": t, "stats_device_empty_masks": te, "facets_device": tf,
                       "stats_over_facets": round(t["ms"] / tf["ms"], 2),
                       "floor_bytes": floor_bytes, "floor_ms": round(floor_ms, 4),
                       "stats_over_floor": round(t["ms"] / floor_ms, 1)}
                out.write(json.dumps(rec) + "\n")
                out.flush()
                print(json.dumps(rec), flush=True)
                del dc, dlo, dhi, dsum, scr, fc
            del dg
        del dm
    out.close()
    index.close()


if __name__ == "__main__":
    main()
