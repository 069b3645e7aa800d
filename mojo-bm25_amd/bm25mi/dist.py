"""Doc-sharded search across ranks.

One process per GPU.  Rank r owns the contiguous document range
``shard_bounds(N, W, r)`` (bm25mi.shard) as an independent index whose ``doc_offset``
is the global id of its first document, and searches the whole (replicated)
query batch on it.  The path has two exchanges, both all-gathers (RCCL over
xGMI with the ``nccl`` backend): every rank's sample keys (global doc ids),
from which each rank takes the same global threshold, and every rank's
[Q, k] list of keys above it (global doc ids + scores), merged by the same
(score desc, doc asc) rule — so the result is exactly the single-index top-k.

The reference has no multi-device path (``DEVICE_ID = 0`` at
main.py:205); this module is the build's only collective.
"""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import torch
import torch.distributed as dist

from .shard import shard_bounds  # noqa: F401  (the one definition; re-exported here)

# merge(g_docs [W,Q,k] int32, g_scores [W,Q,k] f32) -> (docs [Q,k], scores [Q,k])
MergeFn = Callable[[torch.Tensor, torch.Tensor], Tuple[torch.Tensor, torch.Tensor]]


def _all_gather(x: torch.Tensor, group: Optional[dist.ProcessGroup] = None) -> torch.Tensor:
    """[...] on every rank -> [W, ...] (rank-major).  RCCL (backend "nccl")
    gathers device tensors in place over xGMI; gloo (CPU tests, several ranks
    sharing one GPU) has no into-tensor form and no device all_gather, so
    device tensors are staged through host memory there."""
    world = dist.get_world_size(group)
    x = x.contiguous()
    if dist.get_backend(group) != "gloo":
        out = torch.empty((world,) + tuple(x.shape), dtype=x.dtype, device=x.device)
        dist.all_gather_into_tensor(out, x, group=group)
        return out
    h = x.cpu()
    out = torch.empty((world,) + tuple(h.shape), dtype=h.dtype)
    dist.all_gather(list(out.unbind(0)), h, group=group)
    return out.to(x.device)


def all_gather_lists(docs: torch.Tensor, scores: torch.Tensor,
                     group: Optional[dist.ProcessGroup] = None
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
    """All ranks' [Q, k] lists -> [W, Q, k] (rank-major), on every rank."""
    return _all_gather(docs, group), _all_gather(scores, group)


def sharded_topk(docs: torch.Tensor, scores: torch.Tensor, merge: MergeFn,
                 group: Optional[dist.ProcessGroup] = None
                 ) -> Tuple[torch.Tensor, torch.Tensor]:
    """This rank's [Q, k] list (global doc ids) -> the global [Q, k] top-k."""
    if dist.get_world_size(group) == 1:
        return docs, scores
    g_docs, g_scores = all_gather_lists(docs, scores, group)
    return merge(g_docs, g_scores)


def gpu_merge(device: int, stream=None) -> MergeFn:
    """The HIP merge (bm25_merge_topk_device) as a MergeFn, on ``stream``."""
    from .index import merge_topk_device

    def merge(g_docs: torch.Tensor, g_scores: torch.Tensor):
        W, Q, k = g_docs.shape
        out_d = torch.empty((Q, k), dtype=torch.int32, device=g_docs.device)
        out_s = torch.empty((Q, k), dtype=torch.float32, device=g_docs.device)
        merge_topk_device(device, g_docs, g_scores, W, Q, k, out_d, out_s, stream)
        return out_d, out_s

    return merge


def _group_key(group):
    return dist.group.WORLD if group is None else group


def _global_docs(index, device, group=None) -> int:
    """Documents of the whole collection: the sum of every rank's shard,
    all-reduced once per process group and cached on the index object."""
    cache = index.__dict__.setdefault("_bm25_global_docs", {})
    n = cache.get(_group_key(group))
    if n is None:
        if dist.get_world_size(group) == 1:
            n = int(index.n_docs)
        else:
            backend = dist.get_backend(group)
            t = torch.tensor([int(index.n_docs)], dtype=torch.int64,
                             device="cpu" if backend == "gloo" else device)
            dist.all_reduce(t, group=group)
            n = int(t.item())
        cache[_group_key(group)] = n
    return n


def _agree_width(index, S: int, k: int, device, group=None) -> None:
    """Every rank must sample the same width S (the key all-gather has one
    shape): it depends on k, the world and the handle's ``sample_p`` and
    ``theta_bound`` options (and on the shard having tile bounds), which each
    rank sets on its own.  Checked once per (group, k) by one
    all-reduce of (S, -S) with MAX; every rank raises the same ValueError when
    they differ.  GpuIndex.set_option drops the cache, so a changed option
    is re-checked on the next search — every rank must change it together."""
    seen = index.__dict__.setdefault("_bm25_width_ok", set())
    key = (_group_key(group), int(k))
    if key in seen:
        return
    backend = dist.get_backend(group)
    t = torch.tensor([S, -S], dtype=torch.int64, device="cpu" if backend == "gloo" else device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
    lo, hi = -int(t[1].item()), int(t[0].item())
    if lo != hi:
        raise ValueError(f"ranks disagree on the sample width at k={k} (min {lo}, max {hi}): "
                         "set the same sample_p and theta_bound options on every rank's index "
                         "(theta_bound needs every shard's tile bounds: dense, non-negative)")
    seen.add(key)


BOUND_MAX_TILES = 30720  # tiles one block selects a threshold over (kBoundMaxTiles)


def setup_world_bounds(index, group: Optional[dist.ProcessGroup] = None, stream=None,
                       device=None) -> bool:
    """The one-collective protocol's setup (include/bm25mi.h,
    bm25_search_shard_device): every rank exports its shard's tile bounds, the
    ranks all-gather them once, and each rank's handle keeps the world's
    [W, n_terms, stride] table, so a search takes the whole collection's
    tile-bound threshold without the per-batch key exchange.  Collective:
    every rank calls it; False (on every rank) when a shard keeps no tile
    bounds or the collection has more tiles than one block selects over
    (config 5: the two-exchange protocol stays).  ~2 GB per rank at config 3."""
    world = dist.get_world_size(group)
    info = index.info()
    dev = torch.device(device) if device is not None else torch.device("cuda", index.device)
    backend = dist.get_backend(group)
    tdev = "cpu" if backend == "gloo" else dev
    # (no bounds anywhere -> 1, widest stride) by one MAX all-reduce; tiles by a SUM
    t = torch.tensor([0 if info["tile_bounds"] else 1, index.bounds_stride()], dtype=torch.int64,
                     device=tdev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
    n = torch.tensor([int(info["n_tiles"])], dtype=torch.int64, device=tdev)
    dist.all_reduce(n, group=group)
    missing, stride, tiles = int(t[0].item()), int(t[1].item()), int(n.item())
    if missing or world * stride > BOUND_MAX_TILES + 4 * world or tiles < 1:
        return False
    local = torch.empty((index.n_terms, stride), dtype=torch.int16, device=dev)
    st = (stream if stream is not None else torch.cuda.current_stream(dev)) if dev.type == "cuda" \
        else None
    index.bounds_export(local, stride, st)
    with _stream_ctx(st):  # (as int32 pairs: RCCL and gloo move no int16)
        g = _all_gather(local.view(torch.int32), group).view(torch.int16)  # [W, n_terms, stride]
    if st is not None:
        st.synchronize()
    index.set_world_bounds(g, world, stride, tiles)
    return True


def gather_keys(keys: torch.Tensor, group: Optional[dist.ProcessGroup] = None) -> torch.Tensor:
    """All ranks' [Q, S] sample keys -> [W, Q, S] (rank-major), on every rank."""
    return _all_gather(keys, group)


def _forks(index, parts: int):
    """The index and parts - 1 forks of it (bm25_index_fork: shared device
    arrays, own workspaces), created once and cached on the index.  Options
    are copied at fork time; set_option on the index drops the cache."""
    forks = index.__dict__.setdefault("_bm25_forks", [])
    while len(forks) < parts - 1:
        forks.append(index.fork())
    return [index] + forks[:parts - 1]


def _part_streams(index, parts: int, device):
    """One torch stream per part (cached on the index), or None on the CPU."""
    if device.type != "cuda":
        return [None] * parts
    st = index.__dict__.setdefault("_bm25_part_streams", [])
    while len(st) < parts:
        st.append(torch.cuda.Stream(device=device))
    return st[:parts]


def _stream_ctx(s):
    import contextlib
    return torch.cuda.stream(s) if s is not None else contextlib.nullcontext()


def _search_parts(index, d_queries, k, shard_docs_max, d_docs, d_scores, stream, group, world,
                  S, parts):
    """sharded_search over `parts` contiguous row ranges of the batch, each
    on its own fork of the index and its own stream, issued phase by phase
    (every part's sample half, every part's key all-gather, every finish
    half, every list all-gather, every W-way merge).  The device then runs one
    part's collectives and its latency-bound kernels (threshold, merges: one
    wavefront per query) beside another part's score pass — the per-batch
    fixed costs of a doc shard overlap instead of adding up.
    Collectives keep one issue order on every rank.  The result is the
    unsplit search's, row for row."""
    from .index import merge_sorted_device
    Q = d_queries.shape[0]
    cuts = [Q * i // parts for i in range(parts + 1)]
    rows = [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
    ctxs = _forks(index, len(rows))
    dev = d_queries.device
    streams = _part_streams(index, len(rows), dev)
    if streams[0] is not None:  # the parts start after the caller's stream
        ev = torch.cuda.Event()
        ev.record(stream)
        for s in streams:
            s.wait_event(ev)
    qs = [d_queries[a:b] for a, b in rows]
    keys, all_keys, packed, gathered = [], [], [], []
    for i, (a, b) in enumerate(rows):
        with _stream_ctx(streams[i]):
            kk = (torch.empty if S > 0 else torch.zeros)((b - a, max(S, 1)), dtype=torch.int64,
                                                        device=dev)
            if S > 0:
                ctxs[i].search_sample_device(qs[i], k, world, shard_docs_max, kk, streams[i])
            keys.append(kk)
    for i in range(len(rows)):
        with _stream_ctx(streams[i]):
            all_keys.append(gather_keys(keys[i], group) if world > 1 and S > 0
                            else keys[i].unsqueeze(0))
    for i, (a, b) in enumerate(rows):
        with _stream_ctx(streams[i]):
            pk = torch.empty((2, b - a, k), dtype=torch.int32, device=dev)
            ctxs[i].search_finish_device(qs[i], k, world, shard_docs_max, all_keys[i], pk[0],
                                         pk[1].view(torch.float32), streams[i])
            packed.append(pk)
    for i in range(len(rows)):
        with _stream_ctx(streams[i]):
            gathered.append(_all_gather(packed[i], group) if world > 1 else packed[i].unsqueeze(0))
    for i, (a, b) in enumerate(rows):
        with _stream_ctx(streams[i]):
            g = gathered[i]
            merge_sorted_device(dev.index, g, g[:, 1].view(torch.float32), world, b - a, k,
                                2 * (b - a) * k, d_docs[a:b], d_scores[a:b], streams[i])
    if streams[0] is not None:  # the caller's stream continues after every part
        for s in streams:
            ev = torch.cuda.Event()
            ev.record(s)
            stream.wait_event(ev)
    return d_docs, d_scores


def sharded_search(index, d_queries: torch.Tensor, k: int, shard_docs_max: int,
                   d_docs: torch.Tensor, d_scores: torch.Tensor,
                   merge: Optional[MergeFn] = None, stream=None,
                   group: Optional[dist.ProcessGroup] = None,
                   exchange: Optional[Callable[[torch.Tensor], torch.Tensor]] = None,
                   n_docs_total: Optional[int] = None, parts: int = 1
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """One rank's doc-sharded search with a GLOBAL threshold (bm25_search_
    sample/finish_device): this shard's sample keys are all-gathered, theta =
    the k-th best key of the whole sample, the shard lists its keys >= theta,
    and the lists are all-gathered and merged.  Two collectives per batch:
    W*Q*S*8 B of sample keys (S ~ 2k/W: ~200 KB per rank at config 3) and the
    [Q, k] lists — docs and scores in one packed [2, Q, k] buffer, merged by
    the W-way merge of best-first lists (bm25_merge_sorted_device) unless a
    ``merge`` of the two gathered arrays is given.  ``exchange`` replaces the
    key all-gather (tests).

    Everything — kernels and collectives — is enqueued on ``stream`` (default:
    the current stream; a torch.cuda.Stream or a raw hipStream_t handle): the
    collectives order against torch's current stream, so the body runs with
    ``stream`` made current.

    ``k`` is checked against the whole collection's document count, as the
    single-index search checks it (numpy's argpartition error,
    bm25_native.py:205): ``n_docs_total``, or one all-reduce of the shards'
    counts on the first search (cached on ``index``).

    ``parts`` > 1 (packed lists, no ``merge`` / ``exchange``): the batch's
    rows are searched as that many parts pipelined over forks of the index
    on their own streams (``_search_parts``) — the same result."""
    world = int(exchange.world) if exchange is not None else dist.get_world_size(group)
    total = n_docs_total if n_docs_total is not None else (
        _global_docs(index, d_queries.device, group) if exchange is None else None)
    if total is not None and k > total:
        raise ValueError(f"kth(={total - k}) out of bounds ({total})")
    # (k > 4096: S = 0, every shard's exact top-k — bm25mi_large.hip)
    S = index.sample_width(k, world, shard_docs_max)
    if exchange is None and world > 1:
        _agree_width(index, S, k, d_queries.device, group)
    cuda = d_queries.device.type == "cuda"
    if not cuda:
        stream = None
    elif stream is None:
        stream = torch.cuda.current_stream(d_queries.device)
    elif not isinstance(stream, torch.cuda.Stream):
        stream = torch.cuda.ExternalStream(int(stream), device=d_queries.device)
    if (merge is None and exchange is None and parts <= 1
            and index.__dict__.get("_bm25_world_bounds") is not None):
        # one collective: the shard's keys >= the collection's threshold (its
        # own from the world bounds), all-gathered and merged
        with _stream_ctx(stream):
            Q = d_queries.shape[0]
            pk = torch.empty((2, Q, k), dtype=torch.int32, device=d_queries.device)
            index.search_shard_device(d_queries, k, pk[0], pk[1].view(torch.float32), stream)
            g = _all_gather(pk, group) if world > 1 else pk.unsqueeze(0)
            from .index import merge_sorted_device
            merge_sorted_device(d_queries.device.index, g, g[:, 1].view(torch.float32), world, Q,
                                k, 2 * Q * k, d_docs, d_scores, stream)
            return d_docs, d_scores
    if parts > 1 and merge is None and exchange is None:
        return _search_parts(index, d_queries, k, shard_docs_max, d_docs, d_scores, stream,
                             group, world, S, parts)
    if not cuda:
        raise ValueError("sharded_search runs on the GPU (parts > 1 for CPU protocol tests)")
    with torch.cuda.stream(stream):
        Q = d_queries.shape[0]
        # S > 0: the sample pass writes every key of its own width
        keys = (torch.empty if S > 0 else torch.zeros)((Q, max(S, 1)), dtype=torch.int64,
                                                       device=d_queries.device)
        if S > 0:
            index.search_sample_device(d_queries, k, world, shard_docs_max, keys, stream)
        if exchange is not None:
            all_keys = exchange(keys)
        elif world > 1 and S > 0:
            all_keys = gather_keys(keys, group)
        else:
            all_keys = keys.unsqueeze(0)
        packed = merge is None and exchange is None and world > 1
        if not packed:
            index.search_finish_device(d_queries, k, world, shard_docs_max, all_keys, d_docs,
                                       d_scores, stream)
            if exchange is not None or world == 1:
                return d_docs, d_scores
            return sharded_topk(d_docs, d_scores, merge, group)
        pk = torch.empty((2, Q, k), dtype=torch.int32, device=d_queries.device)
        index.search_finish_device(d_queries, k, world, shard_docs_max, all_keys, pk[0],
                                   pk[1].view(torch.float32), stream)
        g = _all_gather(pk, group)  # [W, 2, Q, k]: one collective for docs and scores
        # the merge reads rank w's docs at w * 2Qk and its scores Qk later
        assert tuple(g.shape) == (world, 2, Q, k) and g.is_contiguous(), tuple(g.shape)
        from .index import merge_sorted_device
        merge_sorted_device(d_queries.device.index, g, g[:, 1].view(torch.float32), world, Q, k,
                            2 * Q * k, d_docs, d_scores, stream)
        return d_docs, d_scores


def sharded_search_collapsed(index, d_queries: torch.Tensor, k: int, d_groups: torch.Tensor,
                             per_group: int = 1, d_weights: Optional[torch.Tensor] = None,
                             d_masks: Optional[torch.Tensor] = None,
                             d_query_mask: Optional[torch.Tensor] = None,
                             d_docs: Optional[torch.Tensor] = None,
                             d_scores: Optional[torch.Tensor] = None,
                             d_groups_out: Optional[torch.Tensor] = None, stream=None,
                             group: Optional[dist.ProcessGroup] = None
                             ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """One rank's collapsed search over doc shards (field collapsing: at most
    ``per_group`` hits of a group in a row's top-k): exactly the single-index
    GpuIndex.search_collapsed over the whole collection, on every rank.

    Every rank runs search_collapsed_device on its shard — ``d_groups``,
    ``d_masks`` and ``d_weights`` are by the rank's own documents, as that call
    documents them — into one packed int32 [3, Q, k] buffer (docs | score bits
    | groups).  One all-gather moves it (12 Q k bytes per rank), and
    bm25_merge_collapsed_device merges the world's lists in key order while it
    collapses them once more: a document of the collection's collapsed top-k
    is inside its shard's collapsed top-k, and a merged entry that the
    collection drops finds its per_group better group-mates in the merged input
    (DESIGN.md §4).  A plain merge would not do: two shards can each return a
    hit of one group.

    A shard of fewer than k documents searches at min(k, n_docs) and pads its
    slice.  World size 1 is the plain call, no collective.  Everything is
    enqueued on ``stream`` (default: the current stream), the merge after the
    all-gather as in sharded_search; the shard's search synchronises the
    stream once per round.  Returns (docs, scores, groups), each [Q, k]."""
    if d_queries.dim() != 2:
        raise ValueError("d_queries must be a 2-D [Q, T] tensor")
    k, per_group = int(k), int(per_group)
    if k < 0:
        raise ValueError(f"k={k} must be >= 0")
    world = dist.get_world_size(group)
    dev = d_queries.device
    Q = d_queries.shape[0]
    if d_docs is None:
        d_docs = torch.empty((Q, k), dtype=torch.int32, device=dev)
    if d_scores is None:
        d_scores = torch.empty((Q, k), dtype=torch.float32, device=dev)
    if d_groups_out is None:
        d_groups_out = torch.empty((Q, k), dtype=torch.int32, device=dev)
    for name, t in (("d_docs", d_docs), ("d_scores", d_scores), ("d_groups_out", d_groups_out)):
        if t.numel() != Q * k or t.element_size() != 4 or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous 32-bit [{Q}, {k}] tensor")
    if dev.type != "cuda":
        stream = None
    elif stream is None:
        stream = torch.cuda.current_stream(dev)
    elif not isinstance(stream, torch.cuda.Stream):
        stream = torch.cuda.ExternalStream(int(stream), device=dev)
    if world == 1:
        index.search_collapsed_device(d_queries, k, d_groups, per_group, d_weights, d_masks,
                                      d_query_mask, d_docs, d_scores, d_groups_out, stream)
        return d_docs, d_scores, d_groups_out
    from .index import merge_collapsed_device
    with _stream_ctx(stream):
        pk = torch.empty((3, Q, k), dtype=torch.int32, device=dev)
        ks = min(k, int(index.n_docs))  # (the C call rejects k > n_docs)
        if ks == k:
            part = pk
        else:  # a short shard: its [Q, ks] lists, then padding up to k
            part = torch.empty((3, Q, ks), dtype=torch.int32, device=dev)
            pk[0].fill_(-1)
            pk[1].fill_(-1)  # (score bits 0xFFFFFFFF)
            pk[2].fill_(-1)
        index.search_collapsed_device(d_queries, ks, d_groups, per_group, d_weights, d_masks,
                                      d_query_mask, part[0], part[1].view(torch.float32), part[2],
                                      stream)
        if ks != k:
            pk[:, :, :ks].copy_(part)
        g = _all_gather(pk, group)  # [W, 3, Q, k]: one collective for docs, scores and groups
        assert tuple(g.shape) == (world, 3, Q, k) and g.is_contiguous(), tuple(g.shape)
        # the merge reads rank w's docs at w * 3Qk, its scores Qk and its groups 2Qk later
        merge_collapsed_device(dev.index, g, g[:, 1].view(torch.float32), g[:, 2], world, Q, k,
                               3 * Q * k, per_group, d_docs, d_scores, d_groups_out, stream)
    return d_docs, d_scores, d_groups_out


def sharded_search_sorted(index, d_masks: Optional[torch.Tensor], d_values: torch.Tensor, order,
                          k: int, descending: bool = False, after=None,
                          d_queries: Optional[torch.Tensor] = None, rows: Optional[int] = None,
                          stream=None, group: Optional[dist.ProcessGroup] = None):
    """One rank's sort-by-field search over doc shards: exactly the
    single-index GpuIndex.search_sorted_device over the whole collection, on
    every rank, with the hits' order keys in place of their ranks (a rank is a
    position in one handle's permutation and means nothing on another shard;
    include/bm25mi.h, "Sort-by-field search over doc shards").

    ``d_masks`` ([M, W] packed words, or None: every document), ``d_values``
    (the column's slice) and ``order`` = (d_ranks, d_perm), prebuilt by
    sort_ranks_device for that slice and ``descending``, are by the rank's own
    documents.  Every rank must pass the same kind (dtype of the column) and
    the same direction: keys of different kinds or directions do not compare.
    ``after`` is an optional collection cursor (d_after_docs int32 [M],
    d_after_keys int32 [2, M]): the last column of the docs and of the keys a
    previous page returned (a doc of -1 gives an all-padding row, a doc < -1 is
    no cursor).  M comes from d_masks, else the cursor, else d_queries, else
    ``rows``.

    Steps, all enqueued on ``stream`` (default: the current stream):
    sort_cursor_device turns the cursor into this shard's rank cursors;
    search_sorted_device runs at min(k, n_docs) into a packed int32 [3, M, k]
    buffer (docs | key_hi | key_lo; a short shard's slice pre-filled with -1);
    sort_keys_device fills the key planes; one all-gather moves the buffer
    (12 M k bytes per rank); bm25_merge_sort_keys_device merges the world's
    lists on (key, doc).  World size 1 skips the collective and the merge and
    still returns keys, so paging code is the same at every world size.

    Returns (docs [M, k] int32, keys [2, M, k] int32: key_hi and key_lo;
    padding is doc -1 with keys 0xFFFFFFFF).  With ``d_queries`` ([M, T] token
    ids) it returns (docs, keys, scores): score_docs_device runs on the merged
    docs on every rank (a document of another shard scores +0.0f), one more
    all-gather and a sum over the ranks give every hit's score — exact, as at
    most one addend per slot is non-zero and none is -0.0f — and the score bits
    are 0xFFFFFFFF where the doc is -1: the bits search_boolean(sort=...)
    returns beside its hits on a single index."""
    if not isinstance(order, (tuple, list)) or len(order) != 2:
        raise ValueError("order must be a pair (d_ranks, d_perm), as sort_ranks_device fills them")
    d_ranks, d_perm = order
    k = int(k)
    if k < 0:
        raise ValueError(f"k={k} must be >= 0")
    d_after_docs = d_after_keys = None
    if after is not None:
        if not isinstance(after, (tuple, list)) or len(after) != 2:
            raise ValueError("after must be a pair (d_after_docs [M], d_after_keys [2, M])")
        d_after_docs, d_after_keys = after
    if d_masks is not None:
        M = int(d_masks.shape[0])
    elif d_after_docs is not None:
        M = int(d_after_docs.shape[0])
    elif d_queries is not None:
        M = int(d_queries.shape[0])
    elif rows is not None:
        M = int(rows)
    else:
        raise ValueError("without d_masks, a cursor or d_queries, pass rows")
    if d_after_docs is not None and (
            d_after_docs.dtype != torch.int32 or tuple(d_after_docs.shape) != (M,)
            or d_after_keys.dtype != torch.int32 or tuple(d_after_keys.shape) != (2, M)):
        raise ValueError(f"after must be int32 tensors (d_after_docs [{M}], d_after_keys [2, {M}])")
    if d_queries is not None and (d_queries.dim() != 2 or d_queries.shape[0] != M):
        raise ValueError(f"d_queries must be a 2-D [{M}, T] tensor (one query per row)")
    world = dist.get_world_size(group)
    dev = d_values.device
    if dev.type != "cuda":
        stream = None
    elif stream is None:
        stream = torch.cuda.current_stream(dev)
    elif not isinstance(stream, torch.cuda.Stream):
        stream = torch.cuda.ExternalStream(int(stream), device=dev)
    from . import index as _index
    with _stream_ctx(stream):
        d_after = None
        if d_after_docs is not None:
            d_after = torch.empty((M,), dtype=torch.int32, device=dev)
            keys_in = d_after_keys.contiguous()
            index.sort_cursor_device(d_values, d_perm, keys_in[0], keys_in[1],
                                     d_after_docs.contiguous(), d_after, descending, stream)
        pk = torch.empty((3, M, k), dtype=torch.int32, device=dev)
        ks = min(k, int(index.n_docs))  # (the C call rejects k > n_docs)
        scratch = None
        if d_masks is not None and M and ks:
            scratch = torch.empty((index.sorted_scratch_bytes(M, ks),), dtype=torch.uint8,
                                  device=dev)
        if ks == k:
            index.search_sorted_device(d_masks, d_ranks, d_perm, ks, d_after, pk[0],
                                       torch.empty((M, ks), dtype=torch.int32, device=dev),
                                       scratch, stream)
        else:  # a short shard: its [M, ks] lists, then padding up to k
            pk[0].fill_(-1)
            part = torch.empty((2, M, ks), dtype=torch.int32, device=dev)
            index.search_sorted_device(d_masks, d_ranks, d_perm, ks, d_after, part[0], part[1],
                                       scratch, stream)
            pk[0, :, :ks].copy_(part[0])
        # (docs of -1 get the padding key: every slot of the planes is written)
        index.sort_keys_device(d_values, pk[0], pk[1], pk[2], descending, stream)
        if world == 1:
            docs, keys = pk[0], pk[1:]
        else:
            g = _all_gather(pk, group)  # [W, 3, M, k]: one collective for docs and keys
            assert tuple(g.shape) == (world, 3, M, k) and g.is_contiguous(), tuple(g.shape)
            out = torch.empty((3, M, k), dtype=torch.int32, device=dev)
            # the merge reads rank w's docs at w * 3Mk, its key_hi Mk and its key_lo 2Mk later
            _index.merge_sort_keys_device(dev.index, g, g[:, 1], g[:, 2], world, M, k, 3 * M * k,
                                          out[0], out[1], out[2], stream)
            docs, keys = out[0], out[1:]
        if d_queries is None:
            return docs, keys
        scores = torch.empty((M, k), dtype=torch.float32, device=dev)
        if M and k:
            index.score_docs_device(d_queries, docs, scores, stream)
            if world > 1:
                scores = _all_gather(scores, group).sum(dim=0)
            scores.view(torch.int32).masked_fill_(docs < 0, -1)  # (score bits 0xFFFFFFFF)
    return docs, keys, scores
