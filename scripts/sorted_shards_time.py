"""Time the sort-by-field search over doc shards (bm25_merge_sort_keys_device,
bm25_sort_keys_device, bm25_sort_cursor_device) at config 3's size (GPU box).

  python scripts/sorted_shards_time.py [--out profiles/sorted_shards/c3.jsonl] [--commit ID]

Config 3's 10M documents cut --world (8) ways (bm25mi.shard.shard_bounds), a
random int32 column (a timestamp: about 1000 documents per value), a handle per
shard with the ranks of its own slice.  Every shard's lists come from
bm25_search_sorted_device without masks from a random rank cursor per row (so
the --rows (1024) rows differ), keyed by bm25_sort_keys_device and packed as
the all-gather of bm25mi.dist.sharded_search_sorted would leave them: int32
[W, 3, Q, k].  Records, one JSON line per k (100 and 4096), times between HIP
events (--warmup rounds, then --steps rounds; the median):

  merge_sort_keys  bm25_merge_sort_keys_device on the packed buffer; row 0 is
                   compared with numpy
  merge_sorted     the yardstick, bm25_merge_sorted_device at the same W, Q and k
                   on the same lists with the score -value (best-first, ties by
                   doc id): 8-byte keys against 12 bytes an entry here
  sort_keys        bm25_sort_keys_device over one shard's [Q, k] page
  sort_cursor      bm25_sort_cursor_device for Q collection cursors (the merged
                   page's last column) on one shard
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
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--k", type=int, nargs="*", default=[100, 4096])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sorted_shards", "c3.jsonl"))
    ap.add_argument("--commit", default=None, help="label of the measured code (default: git HEAD)")
    args = ap.parse_args()
    import torch
    import bm25mi
    from bm25mi import synth
    from bm25mi.index import GpuIndex, merge_sorted_device
    from bm25mi.shard import shard_bounds
    if not torch.cuda.is_available():
        sys.exit("no GPU: this script measures, it has no CPU path")
    N, Q, W = synth.CONFIGS[args.config].n_docs, args.rows, args.world
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    stamp = torch.randint(0, max(2, N // 1000), (N,), dtype=torch.int32, device=dev, generator=gen)
    shards = []
    for w in range(W):
        lo, hi = shard_bounds(N, W, w)
        h = GpuIndex(np.array([0, 1], np.int64), np.zeros(1, np.int32), np.ones(1, np.float32),
                     hi - lo, doc_offset=lo)
        col = stamp[lo:hi].contiguous()
        dr = torch.empty(hi - lo, dtype=torch.int32, device=dev)
        dp = torch.empty(hi - lo, dtype=torch.int32, device=dev)
        h.sort_ranks_device(col, dr, dp, False, st)
        shards.append((h, col, dr, dp, lo, hi))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")
    common = {"config": args.config, "commit": args.commit or _commit(), "n_docs": N, "W": W,
              "Q": Q, "steps": args.steps, "warmup": args.warmup}
    for k in args.k:
        g = torch.empty((W, 3, Q, k), dtype=torch.int32, device=dev)
        tmp = torch.empty((Q, k), dtype=torch.int32, device=dev)
        for w, (h, col, dr, dp, lo, hi) in enumerate(shards):
            after = torch.randint(0, hi - lo - k, (Q,), dtype=torch.int32, device=dev,
                                  generator=gen)
            h.search_sorted_device(None, dr, dp, k, after, g[w, 0], tmp, None, st)
            h.sort_keys_device(col, g[w, 0], g[w, 1], g[w, 2], False, st)
        res = torch.empty((3, Q, k), dtype=torch.int32, device=dev)
        merge = lambda: bm25mi.merge_sort_keys_device(0, g, g[:, 1], g[:, 2], W, Q, k, 3 * Q * k,
                                                      res[0], res[1], res[2], st)
        t_merge = _timed(torch, st, merge, args.warmup, args.steps)
        gh = g.cpu().numpy()
        d0 = gh[:, 0, 0].reshape(-1).astype(np.int64)
        k0 = (gh[:, 1, 0].reshape(-1).view(np.uint32).astype(np.uint64) << np.uint64(32)) \
            | gh[:, 2, 0].reshape(-1).view(np.uint32).astype(np.uint64)
        o = np.lexsort((d0, k0))[:k]
        got = res.cpu().numpy()
        assert np.array_equal(got[0, 0], d0[o]), "merged row 0 differs from numpy"
        assert np.array_equal(got[2, 0].view(np.uint32), (k0[o] & np.uint64(0xFFFFFFFF)))
        # the yardstick: the same lists as best-first (score, doc) lists
        y = torch.empty((W, 2, Q, k), dtype=torch.int32, device=dev)
        y[:, 0] = g[:, 0]
        # (the int32 key's low word is value + 2^31: the score is -value, exact below 2^24)
        y[:, 1] = (-(g[:, 2].to(torch.int64) + 2 ** 31 & 0xFFFFFFFF).to(torch.float32)) \
            .view(torch.int32)
        yd = torch.empty((Q, k), dtype=torch.int32, device=dev)
        ys = torch.empty((Q, k), dtype=torch.float32, device=dev)
        yard = lambda: merge_sorted_device(0, y, y[:, 1].view(torch.float32), W, Q, k, 2 * Q * k,
                                           yd, ys, st)
        t_yard = _timed(torch, st, yard, args.warmup, args.steps)
        assert np.array_equal(yd[0].cpu().numpy(), d0[o]), "the yardstick's row 0 differs"
        h, col, dr, dp, lo, hi = shards[0]
        page = g[0, 0].contiguous()
        khi, klo = torch.empty_like(page), torch.empty_like(page)
        t_keys = _timed(torch, st, lambda: h.sort_keys_device(col, page, khi, klo, False, st),
                        args.warmup, args.steps)
        ad, ah, al = (res[i][:, -1].contiguous() for i in (0, 1, 2))
        ar = torch.empty(Q, dtype=torch.int32, device=dev)
        t_cur = _timed(torch, st, lambda: h.sort_cursor_device(col, dp, ah, al, ad, ar, False, st),
                       args.warmup, args.steps)
        rec = dict(common, what="sorted_shards", k=k, merge_sort_keys=t_merge,
                   merge_sorted=t_yard, ratio=round(t_merge["ms"] / t_yard["ms"], 2),
                   sort_keys=t_keys, sort_cursor=t_cur, shard_docs=hi - lo,
                   gathered_bytes=W * 12 * Q * k)
        out.write(json.dumps(rec) + "\n")
        out.flush()
        print(json.dumps(rec), flush=True)
    out.close()
    for s in shards:
        s[0].close()


if __name__ == "__main__":
    main()
