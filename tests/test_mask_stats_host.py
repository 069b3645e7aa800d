"""CPU tests of the field statistics (bm25_mask_stats_scratch, bm25_mask_stats,
bm25_mask_stats_device): the symbols are exported, bound and documented, a NULL
handle is rejected without a GPU and leaves the outputs untouched, the Python
layers reject malformed arguments before any C call, and the model the GPU
tests compare against (tests/stats_model.py) is right: its float sum — 32
integer bins, a carry loop, one rounding — is bit-equal to math.fsum, its
integer sums equal a plain Python loop.  The finalise function of the kernels
(bm25mi_stats_sum.h, host-callable) is run against the model by a stand-alone
program under AddressSanitizer and UBSan."""
import ctypes
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import stats_model as sm
from test_term_masks_host import _bare_index

SYMS = {"bm25_mask_stats_scratch": 5, "bm25_mask_stats": 11, "bm25_mask_stats_device": 14}
FLT_MAX = np.float32(3.4028234663852886e38)


def test_symbols_exported_bound_and_documented():
    from bm25mi import _capi
    syms = _capi.header_symbols()
    text = open(_capi.HEADER).read()
    for s, n in SYMS.items():
        assert s in syms, s
        f = getattr(_capi.lib, s)
        assert f.argtypes is not None and f.restype is ctypes.c_int, s
        assert s in _capi._SIGS
        assert len(f.argtypes) == n, s
        decl = text[text.rindex(f"int {s}("):]
        decl = decl[:decl.index(");")]
        assert decl.count(",") + 1 == n, s  # the declaration of include/bm25mi.h
    doc = text[text.index("Field statistics:"):text.index("int bm25_mask_stats_scratch(")]
    flat = " ".join(" ".join(line.strip().lstrip("*") for line in doc.splitlines()).split())
    for phrase in ("masks [M, W] uint32, W = ceil(n_docs / 32), the layout of bm25_search_filtered",
                   "Bits at or past n_docs are ignored even when set",
                   "No word at index >= W of a row is read",
                   "No entry at index >= n_docs is read",
                   "groups == NULL and G == 0 together mean one bucket per row that holds every "
                   "allowed document",
                   "A document with a negative group, or in the device call a group >= G, is in "
                   "no bucket",
                   "Exactly one of (groups == NULL, G == 0) is BM25_EINVAL",
                   "its value is a number", "NaN is \"no value\"", "+-inf are numbers",
                   "Every entry is written and the caller need not clear them",
                   "Nothing past M * B entries is touched",
                   "int64 never goes through a float", "-0.0f == +0.0f",
                   "a zero result is written as +0.0f",
                   "the sum modulo 2^64",
                   "the exact real sum of the finite contributing values rounded to "
                   "nearest-even once",
                   "+0.0 when that sum is zero or nothing contributes",
                   "both contributing gives NaN",
                   "fewer than 2^32 addends below 2^128",
                   "Where out_count is 0, min, max and sum are written as 0 of their type",
                   "out_min, out_max and out_sum may each be NULL",
                   "+-(sig << (E & 7)), a magnitude below 2^31, to int64 bin E >> 3",
                   "A bin of weight 2^(8 b - 150) cannot overflow int64 below 2^32 addends",
                   "there are no float atomics", "does not depend on scheduling",
                   "ungrouped out_count == bm25_mask_count",
                   "grouped out_count == bm25_mask_facets",
                   "== the ungrouped sum, in wrapping int64",
                   "their float64 sum is not bit-equal to the collection's",
                   "they leave bm25_search_dispatch, bm25_search_counters and "
                   "bm25_search_filtered_stats alone",
                   "at most 288 bytes per bucket plus a constant",
                   "the message names d and the value",
                   "On any error the outputs are untouched",
                   "M == 0 returns BM25_OK without device work", "n_docs == 0 writes zeros",
                   "never synchronises", "retains nothing",
                   "not ordered against the handle's searches", "M may pass 65535",
                   "Out of scope", "percentiles, variance and histograms",
                   "several columns per call"):
        assert phrase in flat, phrase
    assert _capi.abi_version() == 1  # additive: the ABI version stays
    import bm25mi
    assert bm25mi.STATS_KEYS == ("count", "min", "max", "sum", "mean")
    for name in ("stats", "stats_scratch_bytes", "stats_device"):
        assert callable(getattr(bm25mi.GpuIndex, name))


def test_null_handle_is_einval_and_outputs_untouched():
    from bm25mi._capi import BM25_EINVAL, lib
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    masks = np.full((2, 3), 0xFFFFFFFF, np.uint32)
    vals = np.ones(70, np.float32)
    groups = np.zeros(70, np.int32)
    cnt = np.full((2, 4), -7, np.int64)
    lo, hi = np.full((2, 4), -7, np.float32), np.full((2, 4), -7, np.float32)
    tot = np.full((2, 4), -7, np.float64)
    nbytes = ctypes.c_int64(-7)
    calls = (
        lambda: lib.bm25_mask_stats_scratch(None, 1, 2, 4, ctypes.byref(nbytes)),
        lambda: lib.bm25_mask_stats(None, p(masks), 2, p(vals), 1, p(groups), 4, p(cnt), p(lo),
                                    p(hi), p(tot)),
        lambda: lib.bm25_mask_stats_device(None, p(masks), 2, p(vals), 1, p(groups), 4, p(cnt),
                                           p(lo), p(hi), p(tot), p(tot), 1 << 20, None),
    )
    for call in calls:
        assert call() == BM25_EINVAL
        assert b"NULL index" in lib.bm25_last_error()
    assert nbytes.value == -7 and (cnt == -7).all() and (lo == -7).all() and (hi == -7).all()
    assert (tot == -7).all()


def test_python_layers_reject_stats_before_c():
    g = _bare_index(70)  # no handle: reaching the C call would fail on it
    masks = np.ones((2, 70), bool)
    vals = np.zeros(70, np.float32)
    groups = np.zeros(70, np.int64)
    with pytest.raises(ValueError, match="values have dtype float64"):
        g.stats(masks, vals.astype(np.float64))
    with pytest.raises(ValueError, match="values have dtype int16"):
        g.stats(masks, vals.astype(np.int16))
    with pytest.raises(ValueError, match=r"values has shape \(69,\), expected \(70,\)"):
        g.stats(masks, vals[:69])
    with pytest.raises(ValueError, match=r"values has shape \(1, 70\)"):
        g.stats(masks, vals[None, :])
    with pytest.raises(ValueError, match=r"70 \(n_docs\) columns"):
        g.stats(np.ones((2, 69), bool), vals)
    with pytest.raises(ValueError, match="3 .* words per row"):
        g.stats(np.zeros((1, 4), np.uint32), vals)
    with pytest.raises(ValueError, match=r"groups has shape \(69,\), expected \(70,\)"):
        g.stats(masks, vals, groups[:69], 4)
    with pytest.raises(ValueError, match="groups must be an integer array"):
        g.stats(masks, vals, groups.astype(np.float32), 4)
    with pytest.raises(ValueError, match="n_groups = -1 is negative"):
        g.stats(masks, vals, groups, -1)
    with pytest.raises(ValueError, match="n_groups must be an int"):
        g.stats(masks, vals, groups, 4.0)
    with pytest.raises(ValueError, match="n_groups must fit int32"):
        g.stats(masks, vals, groups, 2**31)
    with pytest.raises(ValueError, match="n_groups = 0 with groups"):
        g.stats(masks, vals, groups, 0)
    with pytest.raises(ValueError, match="n_groups = 4 without groups"):
        g.stats(masks, vals, None, 4)
    with pytest.raises(ValueError, match="dtype float64: int32, int64 or float32"):
        g.stats_scratch_bytes(np.float64, 2, 0)


def test_device_wrapper_rejects_shapes_before_c():
    import torch
    g = _bare_index(70)
    dm = torch.zeros((2, 3), dtype=torch.int32)
    dv = torch.zeros(70, dtype=torch.float32)
    dg = torch.zeros(70, dtype=torch.int32)
    dc = torch.zeros((2, 4), dtype=torch.int64)
    dlo = torch.zeros((2, 4), dtype=torch.float32)
    dsum = torch.zeros((2, 4), dtype=torch.float64)
    scr = torch.zeros(2 * 4 * 36, dtype=torch.int64)
    ok = dict(d_groups=dg, n_groups=4, d_scratch=scr)
    with pytest.raises(ValueError, match=r"d_masks must be a packed \[M, 3\]"):
        g.stats_device(dm[:, :2], dv, dc, **ok)
    with pytest.raises(ValueError, match="d_masks must be contiguous"):
        g.stats_device(torch.zeros((3, 2), dtype=torch.int32).t(), dv, dc, **ok)
    with pytest.raises(ValueError, match="d_values has dtype torch.float64"):
        g.stats_device(dm, dv.double(), dc, **ok)
    for bad in (torch.zeros(69), torch.zeros((1, 70)), torch.zeros(140)[::2]):
        with pytest.raises(ValueError, match=r"d_values must be a contiguous \[70\] tensor"):
            g.stats_device(dm, bad, dc, **ok)
    for bad in (torch.zeros(69, dtype=torch.int32), torch.zeros(70, dtype=torch.int64),
                torch.zeros(140, dtype=torch.int32)[::2]):
        with pytest.raises(ValueError, match=r"d_groups must be an int32 \[70\] tensor"):
            g.stats_device(dm, dv, dc, d_groups=bad, n_groups=4, d_scratch=scr)
    with pytest.raises(ValueError, match="d_groups and n_groups come together"):
        g.stats_device(dm, dv, dc, d_groups=dg, n_groups=0, d_scratch=scr)
    with pytest.raises(ValueError, match="d_groups and n_groups come together"):
        g.stats_device(dm, dv, dc, n_groups=4, d_scratch=scr)
    with pytest.raises(ValueError, match="n_groups = -1 must be in"):
        g.stats_device(dm, dv, dc, d_groups=dg, n_groups=-1, d_scratch=scr)
    with pytest.raises(ValueError, match="n_groups must be an int"):
        g.stats_device(dm, dv, dc, d_groups=dg, n_groups=4.0, d_scratch=scr)
    for bad in (torch.zeros((2, 5), dtype=torch.int64), torch.zeros((2, 4), dtype=torch.int32),
                torch.zeros((4, 2), dtype=torch.int64).t(), None):
        with pytest.raises(ValueError, match=r"d_count must be a contiguous torch.int64 \[2, 4\]"):
            g.stats_device(dm, dv, bad, **ok)
    with pytest.raises(ValueError, match=r"d_min must be a contiguous torch.float32 \[2, 4\]"):
        g.stats_device(dm, dv, dc, d_min=dsum, **ok)
    with pytest.raises(ValueError, match=r"d_max must be a contiguous torch.float32 \[2, 4\]"):
        g.stats_device(dm, dv, dc, d_max=dlo[:1], **ok)
    with pytest.raises(ValueError, match=r"d_sum must be a contiguous torch.float64 \[2, 4\]"):
        g.stats_device(dm, dv, dc, d_sum=dlo, **ok)
    with pytest.raises(ValueError, match=r"d_sum must be a contiguous torch.int64 \[2, 4\]"):
        g.stats_device(dm, dv.int(), dc, d_sum=dsum, **ok)
    with pytest.raises(ValueError, match="d_scratch must be a contiguous, 8-byte aligned tensor "
                                         "of at least 2304 bytes"):
        g.stats_device(dm, dv, dc, d_groups=dg, n_groups=4, d_scratch=scr[:-1])
    with pytest.raises(ValueError, match="at least 256 bytes"):
        g.stats_device(dm, dv.int(), dc, d_groups=dg, n_groups=4, d_scratch=scr[:31])


# ------------------------------------------------------------- the float model
def _float_cases():
    """Finite float32 arrays whose exact sum is not zero."""
    rng = np.random.default_rng(17)
    cases = []
    for n in (1, 2, 7, 300, 5000):
        mag = 10.0 ** rng.uniform(-30, 30, n)
        cases.append((mag * rng.choice([-1.0, 1.0], n)).astype(np.float32))
    for n in (1, 3, 64, 4000):  # random bit patterns, the non-finite ones made finite
        u = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
        u = np.where((u & 0x7F800000) == 0x7F800000, u & np.uint32(0xBFFFFFFF), u)
        cases.append(u.view(np.float32))
    for n in (5, 400):  # +-x cancellation with subnormal remainders
        x = (10.0 ** rng.uniform(-10, 30, n)).astype(np.float32)
        tiny = (rng.integers(1, 2**20, n).astype(np.uint32)).view(np.float32)
        cases.append(rng.permutation(np.concatenate([x, -x, tiny])))
    cases.append(np.array([2.0**24, 1, 1, -2.0**24], np.float32))
    cases.append(np.array([1e30, -1e30, 1e-40, 1e30, -1e30, 1e-40], np.float32))
    cases.append(np.full(70_000, FLT_MAX, np.float32))
    cases.append(np.full(70_000, -FLT_MAX, np.float32))
    cases.append(np.array([1.0, 2.0**-53], np.float32))           # a tie: to even (down)
    cases.append(np.array([1.0, 2.0**-52, 2.0**-53], np.float32))  # a tie: to even (up)
    cases.append(np.array([1.0, 2.0**-53, 2.0**-149], np.float32))  # above the tie: up
    cases.append(np.array([-1.0, -2.0**-53, -2.0**-149], np.float32))
    cases.append(np.array([2.0**-149], np.float32))
    cases.append(np.array([-2.0**-149, -2.0**-149], np.float32))
    for c in cases:
        assert np.isfinite(c).all() and math.fsum(c.astype(np.float64).tolist()) != 0.0
    return cases


def test_float_model_is_fsum_on_finite_nonzero_sums():
    for c in _float_cases():
        want = math.fsum(c.astype(np.float64).tolist())   # (float32 -> float64 is exact)
        got = sm.float_sum(c)
        assert sm.bits64(got) == sm.bits64(want), (c[:8], got, want)
    # the intermediate bins are visible: 1.0 is 2^23 * 2^(127 - 150), bin 15, shift 7
    assert sm.few_bins(np.array([1.0, 1.0, -1.0], np.float32), [14, 15, 16]) == [0, 1 << 30, 0]
    assert sm.few_bins(np.array([2.0**-149] * 3, np.float32), [0, 1]) == [3 << 1, 0]
    assert sm.few_bins(np.full(5, FLT_MAX, np.float32), [30, 31]) == [0, 5 * (0xFFFFFF << 6)]
    digits, carry = sm.carry_digits([-1] + [0] * 31)
    assert digits == [255] * 32 and carry == -1


def test_float_model_zero_sums_and_inf_rules():
    z = lambda a: sm.bits64(sm.float_sum(np.array(a, np.float32)))
    assert z([]) == 0 and z([0.0, -0.0]) == 0 and z([-0.0]) == 0
    assert z([1e30, -1e30]) == 0 and z([1e-40, 5.0, -1e-40, -5.0]) == 0
    assert z([np.nan, np.nan]) == 0
    inf = np.inf
    assert sm.float_sum(np.array([1.0, inf, inf, np.nan], np.float32)) == inf
    assert sm.float_sum(np.array([-inf, 3e38, 3e38], np.float32)) == -inf
    assert math.isnan(sm.float_sum(np.array([inf, -inf, 1.0], np.float32)))
    assert sm.float_sum(np.array([np.nan, 2.5], np.float32)) == 2.5


def test_model_against_a_plain_loop():
    """70 documents, 3 masks, G = 5 and ungrouped: negative groups, groups >= G,
    garbage bits past n_docs, NaN and -0.0 in the float column, int64 values
    whose sum wraps."""
    import bm25mi
    rng = np.random.default_rng(11)
    n, G = 70, 5
    allow = rng.random((3, n)) < 0.6
    allow[1] = True
    groups = rng.integers(0, G, n).astype(np.int32)
    groups[rng.random(n) < 0.2] = -1
    groups[[7, 69]] = G
    packed = bm25mi.pack_mask(allow)
    packed[:, -1] |= np.uint32(0xFFFFFFFF << (n % 32) & 0xFFFFFFFF)   # garbage tail bits
    i64 = rng.integers(-2**62, 2**62, n).astype(np.int64)
    i64[:4] = [2**63 - 1, 2**63 - 1, -2**63, 5]
    i32 = rng.integers(-2**31, 2**31, n).astype(np.int32)
    f32 = (rng.standard_normal(n) * 1e3).astype(np.float32)
    f32[[2, 30]] = np.nan
    f32[5] = -0.0
    for vals in (i64, i32, f32):
        for gr, B in ((None, 1), (groups, G)):
            got = sm.stats_want(packed, vals, gr, G if gr is not None else 0)
            for m in range(3):
                for b in range(B):
                    sel = [d for d in range(n) if (int(packed[m, d >> 5]) >> (d & 31)) & 1
                           and (gr is None or gr[d] == b) and vals[d] == vals[d]]
                    assert got["count"][m, b] == len(sel)
                    if not sel:
                        assert got["min"][m, b] == 0 and got["sum"][m, b] == 0
                        continue
                    assert got["min"][m, b] == min(vals[d] for d in sel)
                    assert got["max"][m, b] == max(vals[d] for d in sel)
                    if vals.dtype.kind == "i":
                        s = sum(int(vals[d]) for d in sel)
                        s = (s + 2**63) % 2**64 - 2**63
                        assert int(got["sum"][m, b]) == s
                    else:
                        want = math.fsum(float(vals[d]) for d in sel)
                        assert sm.bits64(got["sum"][m, b]) == sm.bits64(want + 0.0)
    assert sm.stats_want(packed[:0], f32)["count"].shape == (0, 1)


# ----------------------------------------------- the kernels' finalise function
def test_finalise_header_against_the_model_under_sanitizers(tmp_path):
    """bm25mi_stats_sum.h through tests/asan/stats_sum_check.cpp (its own main,
    the host compiler, -fsanitize=address,undefined): sum bits and bins 0, 15,
    31 equal the model's on every case above and on zero, inf and NaN cases."""
    from bm25mi.build import build_host_program
    exe = build_host_program("stats_sum_check")
    inf = np.inf
    cases = _float_cases() + [np.array(a, np.float32) for a in (
        [], [0.0, -0.0], [1e30, -1e30], [np.nan], [inf, 1.0], [-inf, -inf], [inf, -inf],
        [np.nan, 2.5, -0.0])]
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        for c in cases:
            f.write(struct.pack("<I", c.size))
            f.write(np.ascontiguousarray(c, dtype=np.float32).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(cases)
    for c, line in zip(cases, lines):
        bits, b0, b15, b31 = line.split()
        assert int(bits, 16) == sm.bits64(sm.float_sum(c)), (c[:8], line)
        assert [int(b0), int(b15), int(b31)] == sm.few_bins(c, [0, 15, 31]), (c[:8], line)
