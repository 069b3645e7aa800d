"""numpy model of the REST pass's tile bounds (tile_skip_kernel and the tables
it reads), shared by tests/test_mask_bound_model.py (CPU) and
tests/test_gpu_tile_mask.py.  It restates the device arithmetic step by step
— f16 tables, the fp32 tree sum of the whole-tile bound, the integer masked
bound in units of theta / 2^20 — so that its decisions are the kernel's, and
the tile-bound threshold (bound_keys_kernel: the k-th best of the tiles'
largest single-term bounds, per tile or per group of 4 tiles)."""
import numpy as np

TILE = 2048
SUB = TILE // 32          # documents of a sub-block
LANES = 8                 # term lanes of the flat kernel with tile bounds
MARGIN_INT = 1048471      # best * 1.0001 < 2^20


def bounds_stride(ntiles: int) -> int:
    return (ntiles + 3) // 4 * 4


def tables(indptr, indices, data, n_docs: int):
    """(bmax u16 [V, ntiles], tmask u32 [V, ntiles]): build_bmax_kernel's f16
    bits rounded down (65504 past f16's range, 0: no posting) and
    build_tmask_kernel's presence bits."""
    V = len(indptr) - 1
    nt = (n_docs + TILE - 1) // TILE
    nnz = int(indptr[-1])
    term = np.repeat(np.arange(V), np.diff(indptr))
    idx = np.asarray(indices[:nnz], np.int64)
    tile = idx // TILE
    m = np.zeros((V, nt), np.float32)
    tm = np.zeros((V, nt), np.uint32)
    if nnz:
        # a canonical CSC is sorted by (term, doc): each (term, tile) is one run
        key = term * nt + tile
        start = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
        m.reshape(-1)[key[start]] = np.maximum.reduceat(np.asarray(data[:nnz], np.float32), start)
        bit = np.uint32(1) << ((idx % TILE) // SUB).astype(np.uint32)
        tm.reshape(-1)[key[start]] = np.bitwise_or.reduceat(bit, start)
    with np.errstate(over="ignore"):
        h = m.astype(np.float16)
    up = h.astype(np.float32) > m
    h[up] = np.nextafter(h[up], np.float16(-np.inf))
    return h.view(np.uint16), tm


def _upper(bits):
    """One f16 step above the stored maximum, as fp32."""
    return (bits + np.uint16(1)).astype(np.uint16).view(np.float16).astype(np.float32)


def theta_bound(bmax, row, k: int, pool: bool) -> np.float32:
    """The tile-bound threshold's score: the k-th best, over tiles (pool:
    groups of 4 tiles), of the largest stored bound of the row's terms; the
    smallest normal float where fewer than k are positive."""
    V, nt = bmax.shape
    terms = [int(t) for t in row if 0 <= t < V]
    lb = np.zeros(nt, np.float32)
    for t in terms:
        lb = np.maximum(lb, bmax[t].view(np.float16).astype(np.float32))
    if pool:
        ng = (nt + 3) // 4
        lb = np.pad(lb, (0, ng * 4 - nt)).reshape(ng, 4).max(axis=1)
    kth = np.sort(lb)[::-1][k - 1] if k <= lb.size else np.float32(0)
    # fewer than k positive bounds: the zero-fill threshold (kZeroFillTheta), every positive sum
    return kth if kth > 0 else np.float32(1.17549435e-38)


def skip_model(bmax, tmask, row, theta, use_mask=True):
    """(whole, skipped) bool [ntiles] of one query row under the threshold
    score theta: the tiles the whole-tile bound cuts, and the tiles
    tile_skip_kernel marks (whole, or the masked bound where use_mask)."""
    V, nt = bmax.shape
    theta = np.float32(theta)
    if not theta > 0:
        z = np.zeros(nt, bool)
        return z, z.copy()
    ub = np.zeros((LANES, nt), np.float32)
    mk = np.zeros((LANES, nt), np.uint32)
    for i, t in enumerate(row[:LANES]):
        if 0 <= t < V:
            ub[i] = _upper(bmax[t])
            mk[i] = tmask[t]
    with np.errstate(over="ignore", invalid="ignore"):
        s = ((ub[0] + ub[1]) + (ub[2] + ub[3])) + ((ub[4] + ub[5]) + (ub[6] + ub[7]))
        whole = s * np.float32(1.0001) < theta
        K = np.float32(1048576.0) / theta
        scaled = np.fmin(ub * K, np.float32(2097152.0))   # (fminf: NaN -> the cap)
        c = np.where(mk != 0, np.ceil(scaled).astype(np.uint32) + np.uint32(1), np.uint32(0))
    best = np.zeros(nt, np.uint32)
    for sb in range(32):
        acc = (((mk >> np.uint32(sb)) & np.uint32(1)) * c).sum(axis=0, dtype=np.uint32)
        best = np.maximum(best, acc)
    masked = best <= MARGIN_INT
    return whole, (whole | masked) if use_mask else whole.copy()


def real_masked_bound(bmax, tmask, row):
    """The masked bound itself in float64 (no scaling): max over sub-blocks
    of the sum of the present terms' upper bounds, and the whole-tile sum."""
    V, nt = bmax.shape
    ub = np.zeros((LANES, nt), np.float64)
    mk = np.zeros((LANES, nt), np.uint32)
    for i, t in enumerate(row[:LANES]):
        if 0 <= t < V:
            ub[i] = _upper(bmax[t]).astype(np.float64)
            mk[i] = tmask[t]
    per = np.stack([(((mk >> np.uint32(sb)) & np.uint32(1)) * ub).sum(axis=0) for sb in range(32)])
    return per.max(axis=0), ub.sum(axis=0)


def skipped_postings(indptr, indices, row, skipped):
    """Postings of the row's term lanes (duplicates twice) in the skipped tiles."""
    V = len(indptr) - 1
    n = 0
    for t in row[:LANES]:
        if 0 <= t < V:
            tiles = np.asarray(indices[indptr[t]:indptr[t + 1]], np.int64) // TILE
            n += int(skipped[tiles].sum())
    return n
