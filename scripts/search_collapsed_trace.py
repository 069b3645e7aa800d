"""The kernels of a collapsed search, with and without a second round (GPU box).

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \
      python scripts/search_collapsed_trace.py

Config 3, batch 1024, k = 100, per_group 1, the uniform layout of
scripts/search_collapsed_time.py: 8 searches at collapse_page = 100 (11 rows
take a second round: the compaction, gather and exclusion kernels run) and 8
at the automatic page (one round).  The kernel statistics of the run give each
kernel's calls and time; profiles/collapse/kernels_c3.json keeps the rows of
the collapse kernels and of the filter passes beside them.
"""
import os
import sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "mojo-bm25_amd"), REPO):
    sys.path.insert(0, p)
import numpy as np
import torch
from bm25mi import synth
from bm25mi.index import GpuIndex
cfg = synth.CONFIGS["c3"]
ip, ix, dt = synth.make_index(cfg, threads=16)
index = GpuIndex(ip, ix, dt, cfg.n_docs)
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream(dev)
q = synth.make_queries(cfg)
Q, N, k = q.shape[0], cfg.n_docs, 100
dq = torch.from_numpy(q).to(dev)
g = torch.from_numpy(np.random.default_rng(5).integers(0, N // 16, N).astype(np.int32)).to(dev)
cd = torch.empty((Q, k), dtype=torch.int32, device=dev)
cs = torch.empty((Q, k), dtype=torch.float32, device=dev)
cg = torch.empty((Q, k), dtype=torch.int32, device=dev)
for page in (100, 0):
    index.set_option("collapse_page", page)
    for _ in range(8):
        index.search_collapsed_device(dq, k, g, 1, None, None, None, cd, cs, cg, st)
    torch.cuda.synchronize()
    print(page, index.collapse_stats(), flush=True)
index.close()
