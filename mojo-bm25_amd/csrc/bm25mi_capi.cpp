// bm25mi_capi.cpp — the extern "C" boundary of libbm25mi.so (include/bm25mi.h).
//
// Host side of the drop-in: validation with the reference's error behaviour
// (bm25_native.py:105-127), index upload + device layout build, workspace
// management and the search pipeline (score_tiles -> merge -> rescore ->
// merge_final), all on one HIP stream per handle.
#include "../../include/bm25mi.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "bm25mi_host.h"
#include "bm25mi_internal.h"

using namespace bm25mi;

namespace {
thread_local std::string g_err;
}  // namespace

int bm25mi::fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

int bm25mi::hip_fail(hipError_t e, const char* what) {
  return fail(e == hipErrorOutOfMemory ? BM25_ENOMEM : BM25_EHIP, "%s: %s (%s)", what,
              hipGetErrorString(e), hipGetErrorName(e));
}

namespace {

#define HIP_TRY(expr, what)                 \
  do {                                      \
    hipError_t e_ = (expr);                 \
    if (e_ != hipSuccess) return hip_fail(e_, what); \
  } while (0)

int env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return (v && *v) ? atoi(v) : dflt;
}

struct EventPair {
  hipEvent_t a = nullptr, b = nullptr, c = nullptr;  // start, after score pass, end
  bool with_c = false;                                 // c recorded (profiling level 2)
};

// The device arrays of one built index, shared by the handle that built it
// and its forks (bm25_index_fork): freed when the last of them is destroyed.
struct IndexArrays {
  int device = 0;
  std::vector<void*> p;
  ~IndexArrays() {
    hipSetDevice(device);
    for (void* x : p) hipFree(x);
  }
};

}  // namespace

struct bm25_index {
  DevIndex ix;
  std::shared_ptr<IndexArrays> arrays;  // owner of ix's device arrays (null while building)
  hipStream_t stream = nullptr;
  Workspace ws;
  // host-call staging buffers (device)
  int32_t* d_q = nullptr;
  int32_t* d_docs = nullptr;
  float* d_scores = nullptr;
  int64_t cap_q_elems = 0, cap_out_elems = 0;
  std::mutex mu;
  // profiling
  int prof = 0;  // 1: score pass events (a, b) per search; 2: also the search's end (c)
  std::vector<EventPair> ev_pool;
  size_t ev_used = 0;
  double score_ms = 0.0, total_ms = 0.0;
  int64_t score_launches = 0, searches = 0, rescored = 0;
  int64_t device_bytes = 0;
  EventPair* split_ev = nullptr;  // events of a sample/finish search in flight
  hipEvent_t ws_done = nullptr;    // recorded on ws_stream when a search moves to another stream
  hipEvent_t ev_split[2] = {nullptr, nullptr};  // theta -> REST, REST -> select (three streams)
  hipStream_t ws_stream = nullptr; // the stream of the last search that used the workspace
  int32_t* d_maxtok = nullptr;     // bm25_max_token_device result
  bool sampled = false;            // a sample half ran since the last finish half
  // the threshold source (choose_theta_source): host-mapped report of the
  // searches' overflow, the search sequence, the last tile-bound search
  int32_t* report_host = nullptr;
  int32_t* report_dev = nullptr;
  int32_t seq = 0, last_bound_seq = -1, seen_seq = -1, weak_until = 0, backoff = 64;
  int64_t last_bound_q = 0;
  int64_t large_fallback = 0;  // queries of the last large-k list search taken by dense rows
                               // (-1: the dense path served the whole search)
  LargeArena arena;            // the large-k paths' scratch (grown to what they last asked for)
  int64_t filtered_dense = 0;  // queries of the last filtered search the dense path served
  // the collapsed search's state of its rows (run_collapsed), kept for the next
  // one like the large-k scratch, and the last one's bm25_search_collapsed_stats
  char* cstate = nullptr;
  size_t cstate_bytes = 0;
  int64_t cstats[4] = {0, 0, 0, 0};
};

static const OptDesc* find_opt(const char* name) {
  for (const OptDesc& d : kOpts)
    if (!strcmp(d.name, name)) return &d;
  for (const OptDesc& d : kOptsMore)
    if (!strcmp(d.name, name)) return &d;
  fail(BM25_EINVAL, "unknown option '%s'", name);
  return nullptr;
}

int bm25mi::set_opt(SearchOpts& o, const char* name, int64_t v) {
  if (!name) return fail(BM25_EINVAL, "NULL option name");
  const OptDesc* d = find_opt(name);
  if (!d) return BM25_EINVAL;
  if (v < d->lo || v > d->hi || (d->kind == kOptPow2 && (v & (v - 1)) != 0)) {
    if (d->msg) return fail(BM25_EINVAL, "%s", d->msg);
    if (d->kind == kOptBool) return fail(BM25_EINVAL, "%s must be 0 or 1", name);
    return fail(BM25_EINVAL, d->kind == kOptPow2 ? "%s must be a power of two in %d..%d"
                                                  : "%s must be in %d..%d", name, d->lo, d->hi);
  }
  o.*d->field = (int)v;
  return BM25_OK;
}

int bm25mi::get_opt(const SearchOpts& o, const char* name, int64_t* v) {
  if (!name || !v) return fail(BM25_EINVAL, "NULL argument");
  const OptDesc* d = find_opt(name);
  if (!d) return BM25_EINVAL;
  *v = o.*d->field;
  return BM25_OK;
}

namespace {

void free_ws(Workspace& ws) {
  hipFree(ws.cand);
  hipFree(ws.theta);
  hipFree(ws.list);
  hipFree(ws.list_cnt);
  hipFree(ws.fb);
  hipFree(ws.cand2);
  hipFree(ws.flag_tiles);
  hipFree(ws.nflag);
  hipFree(ws.queue);
  hipFree(ws.counters);
  hipFree(ws.slow);
  hipFree(ws.wctr);
  hipFree(ws.seg);
  hipFree(ws.qw);
  hipFree(ws.sub);
  hipFree(ws.sub_ipb);
  hipFree(ws.sub_done);
  hipFree(ws.tskip);
  ws = Workspace{};
}

// Candidate-list capacity per query: the keys above theta of the non-sample
// tiles number about (P-1)*k; a list that overflows sends its query to the
// exact fallback stage (the list_cap option overrides, for tests).
int32_t list_cap_for(const SearchOpts& o, int64_t k) {
  if (o.list_cap > 0) return o.list_cap;
  return (int32_t)std::min<int64_t>(65536, std::max<int64_t>(2048, 64 * k));
}

// Options of a new handle: the BM25_* environment (include/bm25mi.h).
SearchOpts env_opts() {
  SearchOpts o;
  auto read = [&o](const OptDesc& d) {
    int v = env_int(d.env, o.*d.field);
    if (d.kind == kOptBool) v = v != 0;
    if (d.env_clamp >= 1) v = std::max(d.lo, v);
    if (d.env_clamp >= 2) v = std::min(d.hi, v);
    o.*d.field = v;
  };
  for (const OptDesc& d : kOpts) read(d);
  for (const OptDesc& d : kOptsMore) read(d);
  return o;
}

// The workspace for a search of Q queries of T terms at k, enqueued on st.
// A (re)allocated workspace's counters are zeroed on st itself, so they are
// ordered before the search's first kernel on any stream, blocking or not
// (they were zeroed on the null stream once, which a non-blocking stream does
// not wait for: a fork's first search on a part stream read a half-zeroed
// claim counter and skipped items).
int ensure_ws(bm25_index* h, int64_t Q, int64_t T, int k, hipStream_t st) {
  Workspace& ws = h->ws;
  const int64_t need_seg = seg_entries(h->ix, std::max(Q, ws.cap_q), T);
  if (Q <= ws.cap_q && k <= ws.cap_k) {
    if (need_seg <= ws.cap_seg) return BM25_OK;
    // a wider query batch on a sparse index: only the segment table grows
    hipFree(ws.seg);
    ws.seg = nullptr;
    ws.cap_seg = 0;
    HIP_TRY(hipMalloc(&ws.seg, sizeof(uint64_t) * need_seg), "hipMalloc(seg)");
    ws.cap_seg = need_seg;
    return BM25_OK;
  }
  const int64_t q = std::max(Q, ws.cap_q);
  const int64_t kk = std::max<int64_t>(k, ws.cap_k);
  free_ws(ws);
  const int64_t nt = h->ix.ntiles;
  const int64_t mf = maxflag_for((int)kk, nt);
  const int32_t C = list_cap_for(h->ix.opt, kk);
  HIP_TRY(hipMalloc(&ws.cand, sizeof(uint64_t) * q * nt * kTileM), "hipMalloc(cand)");
  HIP_TRY(hipMalloc(&ws.theta, sizeof(uint64_t) * q), "hipMalloc(theta)");
  HIP_TRY(hipMalloc(&ws.list, sizeof(uint64_t) * q * C), "hipMalloc(list)");
  HIP_TRY(hipMalloc(&ws.list_cnt, sizeof(int32_t) * q), "hipMalloc(list_cnt)");
  HIP_TRY(hipMalloc(&ws.fb, sizeof(int32_t) * q), "hipMalloc(fb)");
  HIP_TRY(hipMalloc(&ws.cand2, sizeof(uint64_t) * q * mf * kk), "hipMalloc(cand2)");
  HIP_TRY(hipMalloc(&ws.flag_tiles, sizeof(int32_t) * q * mf), "hipMalloc(flag_tiles)");
  HIP_TRY(hipMalloc(&ws.nflag, sizeof(int32_t) * q), "hipMalloc(nflag)");
  HIP_TRY(hipMalloc(&ws.queue, sizeof(int32_t) * q * mf), "hipMalloc(queue)");
  HIP_TRY(hipMalloc(&ws.counters, sizeof(int32_t) * kCounters), "hipMalloc(counters)");
  HIP_TRY(hipMemsetAsync(ws.counters, 0, sizeof(int32_t) * kCounters, st), "hipMemsetAsync(counters)");
  HIP_TRY(hipMalloc(&ws.slow, sizeof(int32_t) * q), "hipMalloc(slow)");
  HIP_TRY(hipMalloc(&ws.wctr, sizeof(int32_t) * kWctrRegions * kWctrInts), "hipMalloc(wctr)");
  // claim counters start at 0; each flat launch's last wave re-zeroes its region
  HIP_TRY(hipMemsetAsync(ws.wctr, 0, sizeof(int32_t) * kWctrRegions * kWctrInts, st),
          "hipMemsetAsync(wctr)");
  // the split-item table of the REST pass (bound_keys_kernel builds it; its
  // finished-block count resets itself)
  HIP_TRY(hipMalloc(&ws.qw, sizeof(uint32_t) * q), "hipMalloc(qw)");
  HIP_TRY(hipMalloc(&ws.sub, sizeof(uint32_t) * q * 8), "hipMalloc(sub)");
  HIP_TRY(hipMalloc(&ws.sub_ipb, sizeof(int32_t)), "hipMalloc(sub_ipb)");
  HIP_TRY(hipMalloc(&ws.sub_done, sizeof(int32_t)), "hipMalloc(sub_done)");
  HIP_TRY(hipMemsetAsync(ws.sub_done, 0, sizeof(int32_t), st), "hipMemsetAsync(sub_done)");
  // the REST pass's tile-skip words (tile_skip_kernel writes them per search)
  if (h->ix.bmax)
    HIP_TRY(hipMalloc(&ws.tskip, sizeof(uint16_t) * 8 * (size_t)std::max<int64_t>(q * tskip_stride(nt), 1)),
            "hipMalloc(tskip)");
  ws.cap_seg = need_seg;
  if (ws.cap_seg > 0) HIP_TRY(hipMalloc(&ws.seg, sizeof(uint64_t) * ws.cap_seg), "hipMalloc(seg)");
  ws.list_cap = C;
  ws.cap_q = q;
  ws.cap_k = kk;
  return BM25_OK;
}

// The handle's persistent staging buffers of the host searches.  A capacity
// is 0 while its buffer is gone: a failed regrow leaves nothing that the
// next, smaller call would take for a buffer.
int ensure_io(bm25_index* h, int64_t q_elems, int64_t out_elems) {
  if (q_elems > h->cap_q_elems) {
    hipFree(h->d_q);
    h->d_q = nullptr;
    h->cap_q_elems = 0;
    HIP_TRY(hipMalloc(&h->d_q, sizeof(int32_t) * std::max<int64_t>(q_elems, 1)), "hipMalloc(queries)");
    h->cap_q_elems = q_elems;
  }
  if (out_elems > h->cap_out_elems) {
    hipFree(h->d_docs);
    hipFree(h->d_scores);
    h->d_docs = nullptr;
    h->d_scores = nullptr;
    h->cap_out_elems = 0;
    HIP_TRY(hipMalloc(&h->d_docs, sizeof(int32_t) * std::max<int64_t>(out_elems, 1)), "hipMalloc(docs)");
    HIP_TRY(hipMalloc(&h->d_scores, sizeof(float) * std::max<int64_t>(out_elems, 1)), "hipMalloc(scores)");
    h->cap_out_elems = out_elems;
  }
  return BM25_OK;
}

void harvest_events(bm25_index* h) {
  if (h->ev_used == 0) return;
  for (size_t i = 0; i < h->ev_used; ++i) {
    float ms1 = 0.f, ms2 = 0.f;
    const bool tot = h->ev_pool[i].with_c;
    hipEventSynchronize(tot ? h->ev_pool[i].c : h->ev_pool[i].b);  // (maybe a caller's stream)
    hipEventElapsedTime(&ms1, h->ev_pool[i].a, h->ev_pool[i].b);
    if (tot) hipEventElapsedTime(&ms2, h->ev_pool[i].a, h->ev_pool[i].c);
    h->score_ms += ms1;
    h->total_ms += tot ? ms2 : ms1;
  }
  h->ev_used = 0;
}

EventPair* next_events(bm25_index* h) {
  if (!h->prof) return nullptr;
  if (h->ev_used == h->ev_pool.size()) {
    if (h->ev_pool.size() < 512) {
      EventPair p;
      hipEventCreate(&p.a);
      hipEventCreate(&p.b);
      hipEventCreate(&p.c);
      h->ev_pool.push_back(p);
    } else {
      harvest_events(h);
    }
  }
  EventPair* e = &h->ev_pool[h->ev_used++];
  e->with_c = h->prof >= 2;
  return e;
}

// Records the search's end event of a profiled search (level 2 only: every
// event record is a marker packet the device spends ~4 us on).
hipError_t record_end(bm25_index* h, EventPair* ev, hipStream_t st) {
  return (ev && ev->with_c) ? hipEventRecord(ev->c, st) : hipSuccess;
}

// The workspace is shared by every search on the handle: a search enqueued
// on another stream than the previous one first waits for everything
// enqueued on that stream so far (ws_done, recorded there now).  Searches
// that stay on one stream record nothing: an event record costs the device
// a marker packet (~4 us, measured: scripts/dev/latency_bench.hip), a
// cross-stream wait more.  The previous search's stream must still exist
// (torch's pooled streams do).
hipError_t order_ws(bm25_index* h, hipStream_t st) {
  if (h->ws_stream == nullptr || st == h->ws_stream) {
    h->ws_stream = st;
    return hipSuccess;
  }
  if (!h->ws_done) {
    const hipError_t e = hipEventCreateWithFlags(&h->ws_done, hipEventDisableTiming);
    if (e != hipSuccess) return e;
  }
  hipError_t e = hipEventRecord(h->ws_done, h->ws_stream);
  if (e == hipSuccess) e = hipStreamWaitEvent(st, h->ws_done, 0);
  h->ws_stream = st;
  return e;
}

// The host waits for the workspace's last search (its stream).
void ws_wait_host(bm25_index* h) {
  if (h->ws_stream) hipStreamSynchronize(h->ws_stream);
}

// The threshold source of the handle's next search (DevIndex::bound_weak).
// A search that took the tile-bound threshold and sent more than 1/16 of its
// queries to the exact fallback stage — their candidate lists overflowed:
// the single-term tile maxima sit far below the best sums, as on an index
// whose terms all weigh alike — turns that threshold off for the next
// `backoff` searches (64, doubling while it keeps failing, at most 4096),
// which take the sampled threshold instead.  The overflow comes from the
// host-mapped report merge_tail_kernel writes at the end of a search: no
// wait — a report not written yet leaves the choice as it is.  Every choice
// is exact; only the cost differs.  Caller holds h->mu.
void choose_theta_source(bm25_index* h) {
  ++h->seq;
  if (h->report_host && h->last_bound_seq >= 0 && h->seen_seq != h->last_bound_seq) {
    const int32_t r = __atomic_load_n(h->report_host + 1, __ATOMIC_ACQUIRE);
    if (r == h->last_bound_seq) {
      h->seen_seq = r;
      const int64_t nf = __atomic_load_n(h->report_host, __ATOMIC_RELAXED);
      if (nf * 16 > h->last_bound_q) {
        h->weak_until = h->seq + h->backoff;
        h->backoff = std::min(2 * h->backoff, 4096);
      } else {
        h->backoff = 64;
      }
    }
  }
  h->ix.bound_weak = h->seq < h->weak_until;
}

// The search's report slot and sequence number in the workspace (after
// ensure_ws, which may rebuild it); P = 0: it took the tile-bound threshold.
void arm_report(bm25_index* h, int P, int64_t Q) {
  h->ws.report = h->report_dev;
  h->ws.seq = h->seq;
  if (h->ix.bound_weak) h->ix.disp.kernels |= kKBoundOff;
  if (P == 0) {
    h->last_bound_seq = h->seq;
    h->last_bound_q = Q;
  }
}

void alloc_report(bm25_index* h) {
  if (hipHostMalloc((void**)&h->report_host, 2 * sizeof(int32_t), hipHostMallocMapped) !=
      hipSuccess) {
    (void)hipGetLastError();
    h->report_host = nullptr;
    return;
  }
  h->report_host[0] = 0;
  h->report_host[1] = -1;
  if (hipHostGetDevicePointer((void**)&h->report_dev, h->report_host, 0) != hipSuccess) {
    (void)hipGetLastError();
    hipHostFree(h->report_host);
    h->report_host = h->report_dev = nullptr;
  }
}

// Grows a device buffer the handle keeps for its next searches (the large-k
// scratch, the collapsed search's state) to `need` bytes.  Earlier searches
// may still be using the old one: the host waits for their stream first.  A
// size is 0 while its buffer is gone, as ensure_io's.
int grow_kept(bm25_index* h, char*& p, size_t& bytes, size_t need, const char* what) {
  if (need <= bytes) return BM25_OK;
  if (h->ws_stream) HIP_TRY(hipStreamSynchronize(h->ws_stream), "hipStreamSynchronize");
  hipFree(p);
  p = nullptr;
  bytes = 0;
  HIP_TRY(hipMalloc((void**)&p, need), what);
  bytes = need;
  return BM25_OK;
}

// One search in the profile's counts.
void count_search(bm25_index* h) {
  if (h->prof) {
    h->score_launches += 1;
    h->searches += 1;
  }
}

// Device pipeline on stream st; caller holds h->mu and has set the device.
// shard: bm25_search_shard_device — the collection's threshold from the
// world bounds and this shard's keys >= it, unsorted, for the W-way merge.
int run_search(bm25_index* h, const int32_t* d_queries, int64_t Q, int64_t T, int k,
               int32_t* d_docs, float* d_scores, hipStream_t st, bool shard = false) {
  if (Q == 0 || k == 0) return BM25_OK;
  if (k > kMaxK) {  // any k up to n_docs: the large-k path (bm25mi_large.hip)
    // the list path when it applies (no dense score rows), else dense rows
    const bool lists = h->ix.opt.large_lists && k <= kLargeListMaxK && k <= h->ix.n_docs &&
                       large_list_supported(h->ix, T, Q) && large_geom(h->ix, k).P > 0;
    if (lists) {
      const int rc = ensure_ws(h, Q, T, 1, st);  // claim counters, counters, segment table
      if (rc) return rc;
    }
    // the scratch the large-k paths last asked for, allocated once for the
    // next ones (the device is done with the old arena: its last search is)
    const int rcg =
        grow_kept(h, h->arena.base, h->arena.bytes, h->arena.need, "hipMalloc(large-k scratch)");
    if (rcg) return rcg;
    h->arena.used = 0;
    h->ws.arena = &h->arena;
    HIP_TRY(order_ws(h, st), "workspace order");
    // this search selects without the counters: the stats read as zero, not
    // as the previous search's
    if (h->ws.counters)
      HIP_TRY(hipMemsetAsync(h->ws.counters, 0, sizeof(int32_t) * kCounters, st), "hipMemsetAsync");
    h->ix.disp = Dispatch{};
    h->ix.disp.sample_p = 1;
    EventPair* ev = next_events(h);
    if (ev) HIP_TRY(hipEventRecord(ev->a, st), "hipEventRecord");
    if (lists) {
      int64_t nfb = 0;
      HIP_TRY(launch_search_large_lists(h->ix, d_queries, Q, T, k, h->ws, d_docs, d_scores, &nfb, st),
              "large-k list search");
      h->large_fallback = nfb;
    } else {
      h->large_fallback = -1;
      HIP_TRY(launch_search_large(h->ix, d_queries, Q, T, k, d_docs, d_scores, st, &h->arena),
              "large-k search launch");
    }
    if (ev) {
      HIP_TRY(hipEventRecord(ev->b, st), "hipEventRecord");
      HIP_TRY(record_end(h, ev, st), "hipEventRecord");
    }
    count_search(h);
    return BM25_OK;
  }
  int rc = ensure_ws(h, Q, T, k, st);
  if (rc) return rc;
  HIP_TRY(order_ws(h, st), "workspace order");
  h->large_fallback = 0;  // (counter [5] belongs to the last search: no large-k rows here)
  choose_theta_source(h);
  const int P = shard_geom_world(h->ix, k, T, shard).P;
  h->ix.disp = Dispatch{};
  h->ix.disp.sample_p = P;
  arm_report(h, P, Q);
  EventPair* ev = next_events(h);
  if (ev) HIP_TRY(hipEventRecord(ev->a, st), "hipEventRecord");
  HIP_TRY(launch_score(h->ix, d_queries, Q, T, k, h->ws, st, shard), "score launch");
  if (ev) HIP_TRY(hipEventRecord(ev->b, st), "hipEventRecord");
  HIP_TRY(launch_select(h->ix, d_queries, Q, T, k, P, h->ws, d_docs, d_scores, st, shard),
          "select launch");
  HIP_TRY(record_end(h, ev, st), "hipEventRecord");
  count_search(h);
  return BM25_OK;
}

// The device arrays of a ranked search (RankedArgs' on the device).  A null
// d_weights: plain sums.  after: the call is bm25_search_after's (the dispatch
// flag kKAfter), with the cursor arrays d_after_scores / d_after_docs (both
// null: no cursor).
struct RankedDev {
  const int32_t* d_queries = nullptr;
  const float* d_weights = nullptr;
  const uint32_t* d_masks = nullptr;
  int64_t M = 0;
  const int32_t* d_query_mask = nullptr;
  bool after = false;
  const float* d_after_scores = nullptr;
  const int32_t* d_after_docs = nullptr;
};

// Bump offsets of 256-byte aligned parts of one allocation of `bytes` bytes.
struct Carve {
  size_t bytes = 0;
  size_t part(int64_t n) {
    const size_t at = bytes;
    bytes += ((size_t)n + 255) & ~(size_t)255;
    return at;
  }
};

// The filtered search's device pipeline on stream st (bm25mi_filter.hip);
// caller holds h->mu and has set the device.  A search of the handle: the
// workspace, its stream ordering and the large-k scratch as run_search's.
int run_filtered(bm25_index* h, int64_t Q, int64_t T, int k, const RankedDev& d, int32_t* d_docs,
                 float* d_scores, hipStream_t st) {
  if (Q == 0 || k == 0) return BM25_OK;
  int rc = ensure_ws(h, Q, T, std::min<int>(k, kMaxK), st);
  if (rc) return rc;
  rc = grow_kept(h, h->arena.base, h->arena.bytes, h->arena.need, "hipMalloc(filtered scratch)");
  if (rc) return rc;
  h->arena.used = 0;
  h->ws.arena = &h->arena;
  HIP_TRY(order_ws(h, st), "workspace order");
  h->large_fallback = 0;
  h->ix.disp = Dispatch{};
  h->ix.disp.sample_p = 1;
  h->ws.report = nullptr;
  EventPair* ev = next_events(h);
  if (ev) HIP_TRY(hipEventRecord(ev->a, st), "hipEventRecord");
  int64_t nd = 0;
  if (d.after) h->ix.disp.kernels |= kKAfter;
  HIP_TRY(launch_search_filtered(h->ix, d.d_queries, Q, T, k, d.d_masks, d.M, d.d_query_mask,
                                 h->ws, d_docs, d_scores, &nd, st, d.d_weights, d.d_after_scores,
                                 d.d_after_docs),
          d.after ? "cursor search" : d.d_weights ? "weighted search" : "filtered search");
  h->filtered_dense = nd;
  if (ev) {
    HIP_TRY(hipEventRecord(ev->b, st), "hipEventRecord");
    HIP_TRY(record_end(h, ev, st), "hipEventRecord");
  }
  count_search(h);
  return BM25_OK;
}

// The automatic page of a collapsed search at k (option collapse_page = 0):
// twice k — a row of small groups drops few of its first results, so one round
// serves it, and a page costs the cursor search little more than k results do
// (DESIGN.md §4 has the sweep).
int collapse_auto_page(int k) { return (int)std::min<int64_t>(kMaxK, 2 * (int64_t)k); }

// A device buffer of one call's own.
struct OwnBuffer {
  char* p = nullptr;
  ~OwnBuffer() { hipFree(p); }
};

// The collapsed search's loop on stream st (kernels: bm25mi_collapse.hip);
// caller holds h->mu and has set the device.  Round 1 pages the whole batch
// (run_filtered as the cursor search, no cursor) and walks the pages into the
// rows; the rows left unfinished go on in compact sub-batches, each round a
// page after the row's cursor under the row's mask minus its saturated groups.
// A round kept at least one new hit of every row it left unfinished (the first
// entry of such a page is of an open group), so a row takes at most k + 1
// rounds; a round that left a row unfinished dropped an entry of it, that is,
// saturated a new group.  The host waits for the stream once per round, for
// the number of unfinished rows (beside the filtered search's own wait for
// its overflowed lists).  d_groups_out may be null: the rows' groups are then
// kept in the state.
int run_collapsed(bm25_index* h, int64_t Q, int64_t T, int k, const RankedDev& d,
                  const int32_t* d_groups, int per_group, int32_t* d_docs, float* d_scores,
                  int32_t* d_groups_out, hipStream_t st) {
  if (Q == 0 || k == 0) return BM25_OK;
  const int64_t n_docs = h->ix.n_docs, W = (n_docs + 31) >> 5;
  const SearchOpts& o = h->ix.opt;
  const int p = (int)std::max<int64_t>(
      1, std::min<int64_t>(o.collapse_page > 0 ? o.collapse_page : collapse_auto_page(k),
                           std::min<int64_t>(n_docs, kMaxK)));
  // the state of the rows: not the arena's, which run_filtered resets per call
  Carve cs;
  const size_t o_pd = cs.part(4 * Q * p), o_ps = cs.part(4 * Q * p), o_cs = cs.part(4 * Q),
               o_cd = cs.part(4 * Q), o_cnt = cs.part(4 * Q), o_rows = cs.part(4 * Q),
               o_ctr = cs.part(16), o_og = d_groups_out ? 0 : cs.part(4 * Q * k);
  int rc = grow_kept(h, h->cstate, h->cstate_bytes, cs.bytes, "hipMalloc(collapse state)");
  if (rc) return rc;
  HIP_TRY(order_ws(h, st), "workspace order");
  char* const b = h->cstate;
  int32_t* pd = (int32_t*)(b + o_pd);
  float* ps = (float*)(b + o_ps);
  float* cur_s = (float*)(b + o_cs);
  int32_t* cur_d = (int32_t*)(b + o_cd);
  int32_t* cnt = (int32_t*)(b + o_cnt);
  int32_t* rows = (int32_t*)(b + o_rows);
  unsigned long long* ctr = (unsigned long long*)(b + o_ctr);
  int32_t* og = d_groups_out ? d_groups_out : (int32_t*)(b + o_og);
  HIP_TRY(hipMemsetAsync(cur_d, 0xFE, 4 * Q, st), "hipMemsetAsync");  // (< -1: no cursor yet)
  HIP_TRY(hipMemsetAsync(cnt, 0, 4 * Q, st), "hipMemsetAsync");
  HIP_TRY(hipMemsetAsync(ctr, 0, 16, st), "hipMemsetAsync");
  unsigned long long got[2] = {0, 0};
  auto walk = [&](const int32_t* row_map, int64_t R) -> int {
    HIP_TRY(launch_collapse_page(pd, ps, p, row_map, R, d_groups, n_docs, h->ix.doc_offset,
                                 per_group, k, cnt, d_docs, d_scores, og, cur_s, cur_d, ctr, st),
            "collapse walk");
    HIP_TRY(hipMemcpyAsync(got, ctr, sizeof got, hipMemcpyDeviceToHost, st), "D2H unfinished");
    HIP_TRY(hipStreamSynchronize(st), "collapse round sync");
    return BM25_OK;
  };
  RankedDev page = d;  // the cursor search, no cursor yet
  page.after = true;
  rc = run_filtered(h, Q, T, p, page, pd, ps, st);
  if (rc) return rc;
  rc = walk(nullptr, Q);
  if (rc) return rc;
  const int64_t U = (int64_t)got[0];
  int64_t rounds = 1, served = 0;
  if (U > 0) {
    HIP_TRY(launch_collapse_compact(cur_d, Q, rows, st), "collapse compact");
    // rows per sub-batch: their exclusion masks stay within 1 GiB (automatic)
    int64_t chunk = o.collapse_chunk > 0 ? o.collapse_chunk
                                         : std::max<int64_t>(1, ((int64_t)1 << 28) / W);
    chunk = std::min(chunk, U);
    OwnBuffer own;
    Carve cc;
    const size_t c_q = cc.part(4 * chunk * T), c_w = cc.part(d.d_weights ? 4 * chunk * T : 0),
                 c_as = cc.part(4 * chunk), c_ad = cc.part(4 * chunk), c_id = cc.part(4 * chunk),
                 c_ex = cc.part(4 * chunk * W);
    HIP_TRY(hipMalloc((void**)&own.p, std::max<size_t>(cc.bytes, 256)),
            "hipMalloc(collapse masks)");
    int32_t* cq = (int32_t*)(own.p + c_q);
    float* cw = d.d_weights ? (float*)(own.p + c_w) : nullptr;
    float* as = (float*)(own.p + c_as);
    int32_t* ad = (int32_t*)(own.p + c_ad);
    int32_t* ids = (int32_t*)(own.p + c_id);
    uint32_t* excl = (uint32_t*)(own.p + c_ex);
    // a sub-batch: its rows' queries under their own exclusion masks and cursors
    page.d_queries = cq;
    page.d_weights = cw;
    page.d_masks = excl;
    page.d_query_mask = ids;
    page.d_after_scores = as;
    page.d_after_docs = ad;
    for (int64_t u0 = 0; u0 < U; u0 += chunk) {
      const int64_t n = std::min(chunk, U - u0);
      int64_t live = n, sub = 0;
      while (live > 0) {
        if (++sub > (int64_t)k + 1) {
          hipStreamSynchronize(st);
          return fail(BM25_EHIP, "collapsed search: a row took more than k + 1 = %d rounds", k + 1);
        }
        served += live;
        HIP_TRY(launch_collapse_gather(rows + u0, n, d.d_queries, d.d_weights, T, cur_s, cur_d, cq,
                                       cw, as, ad, ids, st),
                "collapse gather");
        HIP_TRY(launch_collapse_exclude(rows + u0, n, d.d_masks, d.M, d.d_query_mask, d_groups,
                                        n_docs, per_group, k, cnt, og, cur_d, excl, st),
                "collapse exclusion masks");
        HIP_TRY(hipMemsetAsync(ctr, 0, 8, st), "hipMemsetAsync");
        page.M = n;
        rc = run_filtered(h, n, T, p, page, pd, ps, st);
        if (rc) {
          hipStreamSynchronize(st);
          return rc;
        }
        rc = walk(rows + u0, n);
        if (rc) return rc;
        live = (int64_t)got[0];
      }
      rounds = std::max(rounds, 1 + sub);
    }
  }
  h->ix.disp.kernels |= kKCollapsed;
  h->cstats[0] = rounds;
  h->cstats[1] = U;
  h->cstats[2] = (int64_t)got[1];
  h->cstats[3] = served;
  return BM25_OK;
}

// Counters of the last search (caller holds h->mu); the search may run on a
// caller's stream: wait for that stream, not for the device.
void read_counters(bm25_index* h, int32_t (&cnt)[kCounters]) {
  if (!h->ws.counters) return;
  ws_wait_host(h);
  hipMemcpyAsync(cnt, h->ws.counters, sizeof cnt, hipMemcpyDeviceToHost, h->stream);
  hipStreamSynchronize(h->stream);
}

// A call's hold on its handle: the handle's mutex, and its device current
// (rc: hipSetDevice's failure).
struct Enter {
  std::lock_guard<std::mutex> lk;
  int rc;
  explicit Enter(bm25_index* h) : lk(h->mu), rc(BM25_OK) {
    const hipError_t e = hipSetDevice(h->ix.device);
    if (e != hipSuccess) rc = hip_fail(e, "hipSetDevice");
  }
};

// A stream of the call's own, destroyed after the HostCall declared below it.
struct OwnStream {
  hipStream_t s = nullptr;
  ~OwnStream() {
    if (s) hipStreamDestroy(s);
  }
};

}  // namespace

extern "C" {

int bm25_abi_version(void) { return BM25MI_ABI_VERSION; }

const char* bm25_last_error(void) { return g_err.c_str(); }

int bm25_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

static int build_index(bm25_index* h, const std::vector<int64_t>& ip, const int32_t* indices,
                       const float* data);

int bm25_index_create(int device, int64_t n_docs, int64_t n_terms, int64_t nnz,
                      const void* indptr, int indptr_is_i64, const int32_t* indices,
                      const float* data, int64_t doc_offset, bm25_index** out) {
  if (!out) return fail(BM25_EINVAL, "out is NULL");
  *out = nullptr;
  if (n_docs < 0 || n_terms < 0 || nnz < 0)
    return fail(BM25_EINVAL, "negative size (n_docs=%lld n_terms=%lld nnz=%lld)",
                (long long)n_docs, (long long)n_terms, (long long)nnz);
  if (n_docs > INT32_MAX) return fail(BM25_EINVAL, "n_docs=%lld exceeds int32 doc ids", (long long)n_docs);
  if (doc_offset < 0 || doc_offset + n_docs > (int64_t)INT32_MAX + 1)
    return fail(BM25_EINVAL, "doc_offset=%lld out of int32 range", (long long)doc_offset);
  if (!indptr || (nnz > 0 && (!indices || !data)))
    return fail(BM25_EINVAL, "NULL CSC array");
  // indptr on the host: int64, validated O(V)
  std::vector<int64_t> ip(n_terms + 1);
  for (int64_t t = 0; t <= n_terms; ++t)
    ip[t] = indptr_is_i64 ? ((const int64_t*)indptr)[t] : (int64_t)((const int32_t*)indptr)[t];
  if (ip[0] != 0 || ip[n_terms] != nnz)
    return fail(BM25_EINVAL, "indptr must start at 0 and end at nnz (got %lld..%lld, nnz=%lld)",
                (long long)ip[0], (long long)ip[n_terms], (long long)nnz);
  for (int64_t t = 0; t < n_terms; ++t) {
    if (ip[t + 1] < ip[t]) return fail(BM25_EINVAL, "indptr decreases at column %lld", (long long)t);
    if (ip[t + 1] - ip[t] > n_docs)
      return fail(BM25_EINVAL, "column %lld has more entries than n_docs", (long long)t);
  }
  const int shift = build_tile_shift();
  const int64_t ntiles = (n_docs + (1LL << shift) - 1) >> shift;
  if (ntiles > 65536) return fail(BM25_EINVAL, "n_docs=%lld needs %lld tiles (> 65536)", (long long)n_docs, (long long)ntiles);

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(BM25_EHIP, "no HIP device available");
  if (device < 0 || device >= ndev) return fail(BM25_EINVAL, "device %d out of range (%d visible)", device, ndev);
  HIP_TRY(hipSetDevice(device), "hipSetDevice");

  bm25_index* h = new bm25_index();
  DevIndex& ix = h->ix;
  ix.opt = env_opts();
  ix.device = device;
  ix.n_docs = n_docs;
  ix.n_terms = n_terms;
  ix.nnz = nnz;
  ix.doc_offset = doc_offset;
  ix.tile_shift = shift;
  ix.ntiles = ntiles;
  const int rc = build_index(h, ip, indices, data);
  if (rc == BM25_OK) {
    h->arrays = std::make_shared<IndexArrays>();
    h->arrays->device = device;
    h->arrays->p = {ix.indptr, ix.rel, ix.tl_ptr, ix.tl_tile, ix.tl_start, ix.ldoc, ix.val, ix.bmax,
                    ix.bpool, ix.tmask, ix.hslot, ix.rowmask};
    *out = h;
  } else {
    bm25_index_destroy(h);
  }
  return rc;
}

// The row presence masks of the heavy terms (row_skip; DevIndex::rowmask),
// beside tmask: the device marks the heavy terms, the host gives them table
// slots in the order of their document frequency (largest first, the lower id
// on a tie) while the budget lasts (row_mask_kb KiB; a slot is ntiles x 64 B),
// the device fills the slots.  Optional like tmask: without the memory, or
// without a heavy term, the handle stays without the table.
static void build_row_masks(bm25_index* h, HostCall& c, const std::vector<int64_t>& ip) {
  DevIndex& ix = h->ix;
  const int64_t V = ix.n_terms;
  const int64_t slot_bytes = (int64_t)sizeof(uint32_t) * kRowEntries * ix.ntiles;
  const int64_t max_slots = ((int64_t)ix.opt.row_mask_kb << 10) / slot_bytes;
  if (max_slots <= 0) return;
  int32_t* d_heavy = c.alloc<int32_t>(V, "hipMalloc(heavy)");
  std::vector<int32_t> heavy(V, 0);
  if (c.ok()) c.run(launch_heavy_terms(ix, d_heavy, h->stream), "heavy_terms launch");
  c.download(heavy.data(), d_heavy, V, "D2H heavy");
  if (c.ok()) c.run(hipStreamSynchronize(h->stream), "heavy_terms");
  if (!c.ok()) return;
  std::vector<int32_t> hterm;
  for (int64_t t = 0; t < V; ++t)
    if (heavy[t]) hterm.push_back((int32_t)t);
  std::stable_sort(hterm.begin(), hterm.end(), [&ip](int32_t x, int32_t y) {
    return ip[x + 1] - ip[x] > ip[y + 1] - ip[y];
  });
  if ((int64_t)hterm.size() > max_slots) hterm.resize((size_t)max_slots);
  if (hterm.empty()) return;
  std::vector<int32_t> hslot(V, -1);
  for (size_t i = 0; i < hterm.size(); ++i) hslot[hterm[i]] = (int32_t)i;
  const int64_t H = (int64_t)hterm.size();
  if (hipMalloc(&ix.hslot, sizeof(int32_t) * V) != hipSuccess ||
      hipMalloc(&ix.rowmask, (size_t)(slot_bytes * H)) != hipSuccess) {
    (void)hipGetLastError();
    hipFree(ix.hslot);
    ix.hslot = nullptr;
    ix.rowmask = nullptr;
    return;
  }
  ix.n_heavy = H;
  int32_t* d_hterm = c.alloc<int32_t>(H, "hipMalloc(hterm)");
  c.upload_to(ix.hslot, hslot.data(), V, "H2D hslot");
  c.upload_to(d_hterm, hterm.data(), H, "H2D hterm");
  if (c.ok()) c.run(launch_build_rowmask(ix, d_hterm, h->stream), "build_rowmask launch");
  // the staged host vectors must outlive the copies, whatever failed since
  const hipError_t es = hipStreamSynchronize(h->stream);
  if (c.ok()) c.run(es, "build_rowmask");
  if (c.ok()) h->device_bytes += (int64_t)sizeof(int32_t) * V + slot_bytes * H;
}

// The device layout of a new handle from the caller's CSC (ip: its indptr
// as int64), on the handle's new stream.  The arrays it leaves in h->ix are
// the handle's (bm25_index_destroy frees them after a failure too); the
// staging buffers are the HostCall's.
static int build_index(bm25_index* h, const std::vector<int64_t>& ip, const int32_t* indices,
                       const float* data) {
  DevIndex& ix = h->ix;
  const int64_t n_terms = ix.n_terms, nnz = ix.nnz, ntiles = ix.ntiles;
  HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking), "hipStreamCreate");
  std::vector<int64_t> cnt;  // (sparse: the tile counts, copied from and to the device)
  HostCall c(h->stream);
  // an array of the index's own
  auto own = [&c](auto** p, int64_t bytes, const char* what) {
    if (c.ok()) c.run(hipMalloc(p, (size_t)bytes), what);
  };
  alloc_report(h);
  // segment table form (DevIndex): BM25_SEGMENTS=dense|sparse; by default the
  // dense V x (ntiles+1) table (O(1) lookups, no per-search table: config 5's
  // 24 GB per rank ran 6 % faster than the tile lists) unless it would
  // outgrow both twice the posting arrays (6 B per posting) and 1/8 of the
  // device's memory — then the O(pairs) tile lists
  const int64_t rel_elems = n_terms * (ntiles + 1);
  {
    const char* m = getenv("BM25_SEGMENTS");
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) total_b = 0;
    const int64_t rel_bytes = rel_elems * 4;
    if (m && !strcmp(m, "sparse")) ix.sparse = true;
    else if (m && !strcmp(m, "dense")) ix.sparse = false;
    else ix.sparse = rel_bytes > 2 * 6 * std::max<int64_t>(nnz, 1) &&
                     rel_bytes > (int64_t)(total_b / 8);
  }
  own(&ix.indptr, sizeof(int64_t) * (n_terms + 1), "hipMalloc(indptr)");
  if (!ix.sparse) own(&ix.rel, sizeof(uint32_t) * std::max<int64_t>(rel_elems, 1), "hipMalloc(rel)");
  own(&ix.ldoc, sizeof(uint16_t) * (nnz + kPostingPad), "hipMalloc(ldoc)");
  own(&ix.val, sizeof(float) * (nnz + kPostingPad), "hipMalloc(val)");
  if (c.ok()) c.run(hipMemsetAsync(ix.ldoc + nnz, 0, sizeof(uint16_t) * kPostingPad, h->stream), "hipMemset");
  if (c.ok()) c.run(hipMemsetAsync(ix.val + nnz, 0, sizeof(float) * kPostingPad, h->stream), "hipMemset");
  int32_t* d_indices = c.alloc<int32_t>(nnz, "hipMalloc(indices)");
  int32_t* d_err = c.alloc<int32_t>(1, "hipMalloc(err)");
  h->device_bytes = (int64_t)(sizeof(int64_t) * (n_terms + 1) +
                              (ix.sparse ? 0 : sizeof(uint32_t) * rel_elems) +
                              (sizeof(uint16_t) + sizeof(float)) * nnz);
  if (c.ok()) c.run(hipMemsetAsync(d_err, 0, sizeof(int32_t), h->stream), "hipMemset");
  c.upload_to(ix.indptr, ip.data(), n_terms + 1, "H2D indptr");
  c.upload_to(d_indices, indices, nnz, "H2D indices");
  c.upload_to(ix.val, data, nnz, "H2D data");
  if (!ix.sparse) {
    if (c.ok()) c.run(launch_build_tables(ix, d_indices, d_err, h->stream), "build_tables launch");
  } else {  // tile lists: count per term, scan on the host, fill
    int64_t* d_cnt = c.alloc<int64_t>(n_terms, "hipMalloc(cnt)");
    cnt.assign(n_terms + 1, 0);
    if (c.ok()) c.run(launch_count_tiles(ix, d_indices, d_cnt, d_err, h->stream), "count_tiles");
    c.download(cnt.data() + 1, d_cnt, n_terms, "count_tiles");
    if (c.ok()) c.run(hipStreamSynchronize(h->stream), "count_tiles");
    for (int64_t t = 0; t < n_terms; ++t) cnt[t + 1] += cnt[t];
    ix.n_pairs = cnt[n_terms];
    own(&ix.tl_ptr, sizeof(int64_t) * (n_terms + 1), "hipMalloc(tl_ptr)");
    own(&ix.tl_tile, sizeof(uint16_t) * std::max<int64_t>(ix.n_pairs, 1), "hipMalloc(tl_tile)");
    own(&ix.tl_start, sizeof(uint32_t) * std::max<int64_t>(ix.n_pairs, 1), "hipMalloc(tl_start)");
    c.upload_to(ix.tl_ptr, cnt.data(), n_terms + 1, "H2D tl_ptr");
    if (c.ok()) c.run(launch_fill_tiles(ix, d_indices, h->stream), "fill_tiles launch");
    if (c.ok()) c.run(hipStreamSynchronize(h->stream), "fill_tiles");
    h->device_bytes += (int64_t)(sizeof(int64_t) * (n_terms + 1) +
                                 (sizeof(uint16_t) + sizeof(uint32_t)) * ix.n_pairs);
  }
  // values 0 or normal positive (no NaN, no denormal): every doc's running
  // sum only grows and is 0 or >= FLT_MIN, which lets the REST pass flag
  // candidates while adding and complete rare queries with zero-score docs
  // (bm25mi_kernels.hip)
  ix.nonneg = true;
  for (int64_t p = 0; p < nnz && ix.nonneg; ++p)
    ix.nonneg = data[p] == 0.0f || data[p] >= 1.17549435e-38f;
  // tile bounds of the REST pass (dense table, non-negative index); without
  // the memory the search simply runs without them
  if (c.ok() && !ix.sparse && ix.nonneg && n_terms > 0 && ntiles > 0) {
    if (hipMalloc(&ix.bmax, sizeof(uint16_t) * n_terms * bmax_stride(ntiles)) == hipSuccess) {
      c.run(launch_build_bmax(ix, h->stream), "build_bmax launch");
      h->device_bytes += (int64_t)(sizeof(uint16_t) * n_terms * bmax_stride(ntiles));
      // the pooled copy of the threshold kernel (a quarter of the bytes; optional)
      const int64_t ps = bmax_stride((ntiles + kPool - 1) / kPool);
      if (c.ok() && hipMalloc(&ix.bpool, sizeof(uint16_t) * n_terms * ps) == hipSuccess) {
        ix.pstride = ps;
        c.run(launch_pool_bounds(ix.bmax, n_terms, bmax_stride(ntiles), ix.bpool, ps, h->stream),
              "pool_bounds launch");
        h->device_bytes += (int64_t)(sizeof(uint16_t) * n_terms * ps);
      } else {
        (void)hipGetLastError();
        ix.bpool = nullptr;
      }
      // the sub-block presence masks that refine the tile bound (optional too)
      if (c.ok() && ix.opt.tile_mask &&
          hipMalloc(&ix.tmask, sizeof(uint32_t) * n_terms * bmax_stride(ntiles)) == hipSuccess) {
        c.run(launch_build_tmask(ix, h->stream), "build_tmask launch");
        h->device_bytes += (int64_t)(sizeof(uint32_t) * n_terms * bmax_stride(ntiles));
        if (c.ok()) build_row_masks(h, c, ip);
      } else {
        (void)hipGetLastError();
        ix.tmask = nullptr;
      }
    } else {
      (void)hipGetLastError();
      ix.bmax = nullptr;
    }
  }
  int32_t herr = 0;
  c.download(&herr, d_err, 1, "D2H err");
  const int rc = c.finish("build sync");
  if (rc) return rc;
  if (herr)
    return fail(BM25_EINVAL,
                "indices must be sorted, unique and in [0, n_docs) within every column "
                "(canonical CSC)");
  return BM25_OK;
}

int bm25_index_destroy(bm25_index* h) {
  if (!h) return BM25_OK;
  hipSetDevice(h->ix.device);
  if (h->stream) hipStreamSynchronize(h->stream);
  // a search on a caller's stream (which the caller may have destroyed since:
  // the device, not the stream)
  if (h->ws_stream) hipDeviceSynchronize();
  for (auto& p : h->ev_pool) {
    hipEventDestroy(p.a);
    hipEventDestroy(p.b);
    hipEventDestroy(p.c);
  }
  if (h->ws_done) hipEventDestroy(h->ws_done);
  for (hipEvent_t e : h->ev_split)
    if (e) hipEventDestroy(e);
  free_ws(h->ws);
  hipFree(h->arena.base);
  hipFree(h->cstate);
  hipFree(h->d_q);
  hipFree(h->d_docs);
  hipFree(h->d_scores);
  hipFree(h->d_maxtok);
  if (h->report_host) hipHostFree(h->report_host);
  if (h->arrays) {
    h->arrays.reset();  // the index arrays go with the last handle sharing them
  } else {              // a create that failed part-way
    for (void* x : {(void*)h->ix.indptr, (void*)h->ix.rel, (void*)h->ix.tl_ptr,
                    (void*)h->ix.tl_tile, (void*)h->ix.tl_start, (void*)h->ix.ldoc,
                    (void*)h->ix.val, (void*)h->ix.bmax, (void*)h->ix.bpool,
                    (void*)h->ix.tmask, (void*)h->ix.hslot, (void*)h->ix.rowmask})
      hipFree(x);
  }
  hipFree(h->ix.wbpool);  // (the handle's own pooled world bounds)
  if (h->stream) hipStreamDestroy(h->stream);
  delete h;
  return BM25_OK;
}

static int pool_world(bm25_index* h);

int bm25_index_fork(bm25_index* base, bm25_index** out) {
  if (!out) return fail(BM25_EINVAL, "out is NULL");
  *out = nullptr;
  if (!base || !base->arrays) return fail(BM25_EINVAL, "NULL or unbuilt index");
  std::lock_guard<std::mutex> lk(base->mu);
  HIP_TRY(hipSetDevice(base->ix.device), "hipSetDevice");
  bm25_index* h = new bm25_index();
  h->ix = base->ix;  // the same device arrays and options; its own dispatch report
  h->ix.disp = Dispatch{};
  h->ix.wbpool = nullptr;  // (the base's own; the fork pools the world table itself, below)
  h->arrays = base->arrays;
  h->device_bytes = base->device_bytes;
  const hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    bm25_index_destroy(h);
    return hip_fail(e, "hipStreamCreate");
  }
  alloc_report(h);
  if (h->ix.wbmax) {
    const int rc = pool_world(h);
    if (rc) {
      bm25_index_destroy(h);
      return rc;
    }
  }
  *out = h;
  return BM25_OK;
}

int bm25_index_info(const bm25_index* h, int64_t* n_docs, int64_t* n_terms, int64_t* nnz,
                    int32_t* tile_docs, int64_t* n_tiles, int64_t* device_bytes) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  if (n_docs) *n_docs = h->ix.n_docs;
  if (n_terms) *n_terms = h->ix.n_terms;
  if (nnz) *nnz = h->ix.nnz;
  if (tile_docs) *tile_docs = 1 << h->ix.tile_shift;
  if (n_tiles) *n_tiles = h->ix.ntiles;
  if (device_bytes) *device_bytes = h->device_bytes;
  return BM25_OK;
}

int bm25_index_segments(const bm25_index* h, int32_t* sparse, int64_t* n_pairs) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  if (sparse) *sparse = h->ix.sparse ? 1 : 0;
  if (n_pairs) *n_pairs = h->ix.n_pairs;
  return BM25_OK;
}

int bm25_index_bounds(const bm25_index* h, int32_t* has_bounds, int64_t* bytes) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  const bool on = h->ix.bmax != nullptr;
  if (has_bounds) *has_bounds = on ? 1 : 0;
  if (bytes) *bytes = on ? (int64_t)sizeof(uint16_t) * h->ix.n_terms * bmax_stride(h->ix.ntiles) : 0;
  return BM25_OK;
}

int bm25_search(bm25_index* h, const int32_t* queries, int64_t Q, int64_t T, int32_t k,
                int32_t* out_docs, float* out_scores) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  if (Q < 0 || T < 0) return fail(BM25_EINVAL, "negative query shape");
  int rc = check_k(h->ix.n_docs, k);
  if (rc) return rc;
  if (Q == 0 || k == 0) return BM25_OK;
  if (T > 0 && !queries) return fail(BM25_EINVAL, "NULL queries");
  if (!out_docs || !out_scores) return fail(BM25_EINVAL, "NULL output");
  rc = check_token_ids(h->ix.n_terms, 0, queries, Q * T);
  if (rc) return rc;
  Enter in(h);
  if (in.rc) return in.rc;
  rc = ensure_io(h, Q * T, Q * (int64_t)k);
  if (rc) return rc;
  HostCall c(h->stream);
  c.upload_to(h->d_q, queries, Q * T, "H2D queries");
  if (c.ok()) c.hold(run_search(h, h->d_q, Q, T, k, h->d_docs, h->d_scores, h->stream));
  c.download(out_docs, h->d_docs, Q * k, "D2H docs");
  c.download(out_scores, h->d_scores, Q * k, "D2H scores");
  return c.finish("search sync");
}

int bm25_search_device(bm25_index* h, const int32_t* d_queries, int64_t Q, int64_t T, int32_t k,
                       int32_t* d_docs, float* d_scores, void* stream) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  if (Q < 0 || T < 0) return fail(BM25_EINVAL, "negative query shape");
  int rc = check_k(h->ix.n_docs, k);
  if (rc) return rc;
  if (Q == 0 || k == 0) return BM25_OK;
  Enter in(h);
  if (in.rc) return in.rc;
  return run_search(h, d_queries, Q, T, k, d_docs, d_scores, (hipStream_t)stream);
}

// The arguments of a ranked host call on the device: the weights (with `rules`
// kRankedWeights even where T == 0: the weighted path wants a pointer), masks,
// mask ids and cursors in staging buffers of the call's own, the queries in
// the handle's d_q (after ensure_io).
static RankedDev stage_ranked(bm25_index* h, HostCall& c, const RankedArgs& a, unsigned rules) {
  const int64_t W = (h->ix.n_docs + 31) >> 5;
  RankedDev d;
  if (a.weights || (rules & kRankedWeights)) {
    float* d_w = c.alloc<float>(a.Q * a.T);
    c.upload_to(d_w, a.weights, a.Q * a.T);
    d.d_weights = d_w;
  }
  d.d_masks = c.upload(a.masks, a.M * W);
  d.M = a.M;
  d.d_query_mask = c.upload(a.query_mask, a.query_mask ? a.Q : 0);
  d.d_after_scores = c.upload(a.after_scores, a.after_docs ? a.Q : 0);
  d.d_after_docs = c.upload(a.after_docs, a.after_docs ? a.Q : 0);
  c.upload_to(h->d_q, a.queries, a.Q * a.T);
  d.d_queries = h->d_q;
  d.after = (rules & kRankedCursor) != 0;
  return d;
}

// A ranked host call but the collapsed one: validate, stage, run_filtered into
// the handle's output buffers, download.  what: the call's label in a HIP
// error's text ("<what> staging" for a failed upload).
static int ranked_host_call(bm25_index* h, const RankedArgs& a, unsigned rules,
                            const char* what_staging, const char* what) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  int rc = check_ranked_shape(h->ix.n_docs, a, rules);
  if (rc) return rc;
  if (a.Q == 0 || a.k == 0) return BM25_OK;
  rc = check_ranked_content(h->ix.n_terms, a, rules);
  if (rc) return rc;
  Enter in(h);
  if (in.rc) return in.rc;
  rc = ensure_io(h, a.Q * a.T, a.Q * (int64_t)a.k);
  if (rc) return rc;
  HostCall c(h->stream);
  const RankedDev d = stage_ranked(h, c, a, rules);
  if (!c.ok()) return c.finish(what_staging);
  c.hold(run_filtered(h, a.Q, a.T, a.k, d, h->d_docs, h->d_scores, h->stream));
  c.download(a.out_docs, h->d_docs, a.Q * a.k);
  c.download(a.out_scores, h->d_scores, a.Q * a.k);
  return c.finish(what);
}

int bm25_search_filtered(bm25_index* h, const int32_t* queries, int64_t Q, int64_t T, int32_t k,
                         const uint32_t* masks, int64_t M, const int32_t* query_mask,
                         int32_t* out_docs, float* out_scores) {
  RankedArgs a;
  a.queries = queries, a.Q = Q, a.T = T, a.k = k;
  a.masks = masks, a.M = M, a.query_mask = query_mask;
  a.out_docs = out_docs, a.out_scores = out_scores;
  return ranked_host_call(h, a, kRankedNeedsMask, "filtered search staging", "filtered search");
}

int bm25_search_filtered_device(bm25_index* h, const int32_t* d_queries, int64_t Q, int64_t T,
                                int32_t k, const uint32_t* d_masks, int64_t M,
                                const int32_t* d_query_mask, int32_t* d_docs, float* d_scores,
                                void* stream) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  RankedArgs a;
  a.Q = Q, a.T = T, a.k = k, a.M = M;
  const int rc = check_ranked_shape(h->ix.n_docs, a, 0);
  if (rc) return rc;
  if (Q == 0 || k == 0) return BM25_OK;
  Enter in(h);
  if (in.rc) return in.rc;
  RankedDev d;
  d.d_queries = d_queries;
  d.d_masks = d_masks, d.M = M, d.d_query_mask = d_query_mask;
  return run_filtered(h, Q, T, k, d, d_docs, d_scores, (hipStream_t)stream);
}

int bm25_search_weighted(bm25_index* h, const int32_t* queries, const float* weights, int64_t Q,
                         int64_t T, int32_t k, const uint32_t* masks, int64_t M,
                         const int32_t* query_mask, int32_t* out_docs, float* out_scores) {
  RankedArgs a;
  a.queries = queries, a.weights = weights, a.Q = Q, a.T = T, a.k = k;
  a.masks = masks, a.M = M, a.query_mask = query_mask;
  a.out_docs = out_docs, a.out_scores = out_scores;
  return ranked_host_call(h, a, kRankedWeights, "weighted search staging", "weighted search");
}

int bm25_search_weighted_device(bm25_index* h, const int32_t* d_queries, const float* d_weights,
                                int64_t Q, int64_t T, int32_t k, const uint32_t* d_masks,
                                int64_t M, const int32_t* d_query_mask, int32_t* d_docs,
                                float* d_scores, void* stream) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  RankedArgs a;
  a.Q = Q, a.T = T, a.k = k, a.M = M;
  const int rc = check_ranked_shape(h->ix.n_docs, a, kRankedWeights);
  if (rc) return rc;
  if (Q == 0 || k == 0) return BM25_OK;
  if (T > 0 && (!d_queries || !d_weights)) return fail(BM25_EINVAL, "NULL queries or weights");
  if (M > 0 && !d_masks) return fail(BM25_EINVAL, "NULL masks");
  if (!d_docs || !d_scores) return fail(BM25_EINVAL, "NULL output");
  Enter in(h);
  if (in.rc) return in.rc;
  // T == 0: no weight is read, but the weighted path still wants a pointer
  static const float none = 0.f;
  RankedDev d;
  d.d_queries = d_queries, d.d_weights = d_weights ? d_weights : &none;
  d.d_masks = d_masks, d.M = M, d.d_query_mask = d_query_mask;
  return run_filtered(h, Q, T, k, d, d_docs, d_scores, (hipStream_t)stream);
}

int bm25_search_after(bm25_index* h, const int32_t* queries, const float* weights, int64_t Q,
                      int64_t T, int32_t k, const uint32_t* masks, int64_t M,
                      const int32_t* query_mask, const float* after_scores,
                      const int32_t* after_docs, int32_t* out_docs, float* out_scores) {
  RankedArgs a;
  a.queries = queries, a.weights = weights, a.Q = Q, a.T = T, a.k = k;
  a.masks = masks, a.M = M, a.query_mask = query_mask;
  a.after_scores = after_scores, a.after_docs = after_docs;
  a.out_docs = out_docs, a.out_scores = out_scores;
  return ranked_host_call(h, a, kRankedCursor, "cursor search staging", "cursor search");
}

int bm25_search_after_device(bm25_index* h, const int32_t* d_queries, const float* d_weights,
                             int64_t Q, int64_t T, int32_t k, const uint32_t* d_masks, int64_t M,
                             const int32_t* d_query_mask, const float* d_after_scores,
                             const int32_t* d_after_docs, int32_t* d_docs, float* d_scores,
                             void* stream) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  RankedArgs a;  // (device pointers: looked at, never read)
  a.queries = d_queries, a.Q = Q, a.T = T, a.k = k, a.masks = d_masks, a.M = M;
  a.after_scores = d_after_scores, a.after_docs = d_after_docs;
  a.out_docs = d_docs, a.out_scores = d_scores;
  int rc = check_ranked_shape(h->ix.n_docs, a, kRankedCursor);
  if (rc) return rc;
  if (Q == 0 || k == 0) return BM25_OK;
  rc = check_ranked_pointers(a, kRankedCursor);
  if (rc) return rc;
  Enter in(h);
  if (in.rc) return in.rc;
  RankedDev d;
  d.d_queries = d_queries, d.d_weights = d_weights;
  d.d_masks = d_masks, d.M = M, d.d_query_mask = d_query_mask;
  d.after = true, d.d_after_scores = d_after_scores, d.d_after_docs = d_after_docs;
  return run_filtered(h, Q, T, k, d, d_docs, d_scores, (hipStream_t)stream);
}

int bm25_search_collapsed(bm25_index* h, const int32_t* queries, const float* weights, int64_t Q,
                          int64_t T, int32_t k, const uint32_t* masks, int64_t M,
                          const int32_t* query_mask, const int32_t* groups, int32_t per_group,
                          int32_t* out_docs, float* out_scores, int32_t* out_groups) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  RankedArgs a;
  a.queries = queries, a.weights = weights, a.Q = Q, a.T = T, a.k = k;
  a.masks = masks, a.M = M, a.query_mask = query_mask;
  a.groups = groups, a.per_group = per_group;
  a.out_docs = out_docs, a.out_scores = out_scores;
  int rc = check_ranked_shape(h->ix.n_docs, a, kRankedCollapse);
  if (rc) return rc;
  if (Q == 0 || k == 0) return BM25_OK;
  rc = check_ranked_content(h->ix.n_terms, a, kRankedCollapse);
  if (rc) return rc;
  Enter in(h);
  if (in.rc) return in.rc;
  rc = ensure_io(h, Q * T, Q * (int64_t)k);
  if (rc) return rc;
  // beside the ranked arguments, the groups and the rows' groups: staging
  // buffers of this call's own
  HostCall c(h->stream);
  const RankedDev d = stage_ranked(h, c, a, kRankedCollapse);
  const int32_t* d_groups = c.upload(groups, h->ix.n_docs);
  int32_t* d_og = c.alloc<int32_t>(Q * (int64_t)k);
  if (!c.ok()) return c.finish("collapsed search staging");
  c.hold(run_collapsed(h, Q, T, k, d, d_groups, per_group, h->d_docs, h->d_scores, d_og,
                       h->stream));
  c.download(out_docs, h->d_docs, Q * k);
  c.download(out_scores, h->d_scores, Q * k);
  if (out_groups) c.download(out_groups, d_og, Q * k);
  return c.finish("collapsed search");
}

int bm25_search_collapsed_device(bm25_index* h, const int32_t* d_queries, const float* d_weights,
                                 int64_t Q, int64_t T, int32_t k, const uint32_t* d_masks,
                                 int64_t M, const int32_t* d_query_mask, const int32_t* d_groups,
                                 int32_t per_group, int32_t* d_docs, float* d_scores,
                                 int32_t* d_groups_out, void* stream) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  RankedArgs a;  // (device pointers: looked at, never read)
  a.queries = d_queries, a.Q = Q, a.T = T, a.k = k, a.masks = d_masks, a.M = M;
  a.groups = d_groups, a.per_group = per_group;
  a.out_docs = d_docs, a.out_scores = d_scores;
  int rc = check_ranked_shape(h->ix.n_docs, a, kRankedCollapse);
  if (rc) return rc;
  if (Q == 0 || k == 0) return BM25_OK;
  rc = check_ranked_pointers(a, kRankedCollapse);
  if (rc) return rc;
  Enter in(h);
  if (in.rc) return in.rc;
  RankedDev d;
  d.d_queries = d_queries, d.d_weights = d_weights;
  d.d_masks = d_masks, d.M = M, d.d_query_mask = d_query_mask;
  return run_collapsed(h, Q, T, k, d, d_groups, per_group, d_docs, d_scores, d_groups_out,
                       (hipStream_t)stream);
}

int bm25_search_collapsed_stats(bm25_index* h, int64_t* out, int32_t n) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  if (!out) return fail(BM25_EINVAL, "NULL argument");
  if (n < 1 || n > 4) return fail(BM25_EINVAL, "n=%d must be in 1..4", n);
  std::lock_guard<std::mutex> lk(h->mu);
  for (int i = 0; i < n; ++i) out[i] = h->cstats[i];
  return BM25_OK;
}

int bm25_search_filtered_stats(bm25_index* h, int64_t* out, int32_t n) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  if (!out) return fail(BM25_EINVAL, "NULL argument");
  if (n < 1 || n > 3) return fail(BM25_EINVAL, "n=%d must be in 1..3", n);
  Enter in(h);
  if (in.rc) return in.rc;
  int32_t cnt[kCounters] = {};
  read_counters(h, cnt);
  // (counters [5] and [3]: pass A's skipped pairs, pass B's re-scored pairs)
  const bool tiles = (h->ix.disp.kernels & kKFiltered) != 0;
  const int64_t v[3] = {h->filtered_dense, tiles ? cnt[5] : 0, tiles ? cnt[3] : 0};
  for (int i = 0; i < n; ++i) out[i] = v[i];
  return BM25_OK;
}

}  // extern "C"

namespace {

// The clause arguments of the term-mask calls: shapes and pointers.
int check_clauses(const void* must, int64_t A, const void* any, int64_t B, const void* must_not,
                  int64_t N, int64_t M, const void* base, int64_t Mb) {
  if (A < 0 || B < 0 || N < 0 || M < 0 || Mb < 0)
    return fail(BM25_EINVAL, "negative clause or mask shape");
  if (Mb != 0 && Mb != 1 && Mb != M)
    return fail(BM25_EINVAL, "base masks: Mb = %lld must be 0, 1 or M = %lld", (long long)Mb,
                (long long)M);
  if (M == 0) return BM25_OK;
  if (A > 0 && !must) return fail(BM25_EINVAL, "NULL must");
  if (B > 0 && !any) return fail(BM25_EINVAL, "NULL any");
  if (N > 0 && !must_not) return fail(BM25_EINVAL, "NULL must_not");
  if (Mb > 0 && !base) return fail(BM25_EINVAL, "NULL base");
  return BM25_OK;
}

// check_token_ids over the clause ids: max(initial = mx) >= n_terms -> ValueError
int check_clause_ids(const bm25_index* h, int64_t mx, const int32_t* must, int64_t A,
                     const int32_t* any, int64_t B, const int32_t* must_not, int64_t N, int64_t M) {
  mx = max_token(max_token(mx, must, M * A), any, M * B);
  return check_token_ids(h->ix.n_terms, mx, must_not, M * N);
}

// min_match of the min-match calls (NULL: every row needs one term): the
// clause width the counter holds — a shape, so the device call checks it too
// — and, of host values, their sign.
int check_min_match(const int32_t* min_match, int64_t B, int64_t M, bool host) {
  if (!min_match) return BM25_OK;
  if (B > 65535)
    return fail(BM25_EINVAL, "min_match: the any clause holds B = %lld slots, at most 65535",
                (long long)B);
  for (int64_t m = 0; host && m < M; ++m)
    if (min_match[m] < 0)
      return fail(BM25_EINVAL, "min_match[%lld] = %d is negative", (long long)m, min_match[m]);
  return BM25_OK;
}

// The facet arguments' shape, G in [0, 2^31 - 1]: a group id is an int32.
int check_facet_shape(int64_t M, int64_t G) {
  if (M < 0 || G < 0) return fail(BM25_EINVAL, "negative facet shape");
  if (G > 0x7FFFFFFFll)
    return fail(BM25_EINVAL, "G = %lld groups: at most 2^31 - 1", (long long)G);
  return BM25_OK;
}

// Host group ids: an id >= G names no group (a negative one: no group at all).
int check_groups(const int32_t* groups, int64_t n_docs, int64_t G) {
  for (int64_t d = 0; d < n_docs; ++d)
    if (groups[d] >= G)
      return fail(BM25_EINVAL, "groups[%lld] = %d is not below G = %lld", (long long)d, groups[d],
                  (long long)G);
  return BM25_OK;
}

// The range arguments' shapes and pointers (host and device calls alike).
int check_range_shape(int32_t kind, int64_t F, const void* fields, const void* lo, const void* hi,
                      int64_t C, int64_t M, const void* base, int64_t Mb) {
  if (kind != BM25_FIELD_I32 && kind != BM25_FIELD_F32 && kind != BM25_FIELD_I64)
    return fail(BM25_EINVAL, "kind = %d: BM25_FIELD_I32 (0), BM25_FIELD_F32 (1) or BM25_FIELD_I64 (2)",
                (int)kind);
  if (F < 0 || C < 0 || M < 0 || Mb < 0) return fail(BM25_EINVAL, "negative range or mask shape");
  if (Mb != 0 && Mb != 1 && Mb != M)
    return fail(BM25_EINVAL, "base masks: Mb = %lld must be 0, 1 or M = %lld", (long long)Mb,
                (long long)M);
  if (M == 0) return BM25_OK;
  if (C > 0 && !fields) return fail(BM25_EINVAL, "NULL fields");
  if (C > 0 && (!lo || !hi)) return fail(BM25_EINVAL, "NULL bounds");
  if (Mb > 0 && !base) return fail(BM25_EINVAL, "NULL base");
  return BM25_OK;
}

size_t field_bytes(int32_t kind) { return kind == BM25_FIELD_I64 ? 8 : 4; }

int check_kind(int32_t kind) {
  if (kind != BM25_FIELD_I32 && kind != BM25_FIELD_F32 && kind != BM25_FIELD_I64)
    return fail(BM25_EINVAL, "kind = %d: BM25_FIELD_I32 (0), BM25_FIELD_F32 (1) or BM25_FIELD_I64 (2)",
                (int)kind);
  return BM25_OK;
}

// The shape of a sorted search: M rows, 0 <= k <= min(n_docs, kMaxK).
int check_sorted_shape(const bm25_index* h, int64_t M, int32_t k) {
  if (M < 0) return fail(BM25_EINVAL, "negative mask shape");
  if (k < 0) return fail(BM25_EINVAL, "negative dimensions are not allowed");
  if (k > kMaxK)
    return fail(BM25_EINVAL, "k = %d: a sorted search returns at most %d hits a row", (int)k,
                (int)kMaxK);
  if (k > h->ix.n_docs)
    return fail(BM25_EINVAL, "k = %d is above the index's %lld documents", (int)k,
                (long long)h->ix.n_docs);
  return BM25_OK;
}

// Host range clauses: a field id >= F names no field (a negative one is
// padding), and a float32 NaN bound would silently match nothing.
int check_ranges(int32_t kind, int64_t F, const int32_t* fields, const void* lo, const void* hi,
                 int64_t C, int64_t M) {
  const float* flo = kind == BM25_FIELD_F32 ? (const float*)lo : nullptr;
  const float* fhi = kind == BM25_FIELD_F32 ? (const float*)hi : nullptr;
  for (int64_t m = 0; m < M; ++m)
    for (int64_t c = 0; c < C; ++c) {
      const int64_t i = m * C + c;
      if (fields[i] < 0) continue;
      if (fields[i] >= F)
        return fail(BM25_EINVAL, "fields[%lld][%lld] = %d is not below F = %lld", (long long)m,
                    (long long)c, fields[i], (long long)F);
      if (flo && (flo[i] != flo[i] || fhi[i] != fhi[i]))
        return fail(BM25_EINVAL, "%s[%lld][%lld] is NaN", flo[i] != flo[i] ? "lo" : "hi",
                    (long long)m, (long long)c);
    }
  return BM25_OK;
}

}  // namespace

extern "C" {

int bm25_range_masks(bm25_index* h, const void* values, int32_t kind, int64_t F,
                     const int32_t* fields, const void* lo, const void* hi, int64_t C, int64_t M,
                     const uint32_t* base, int64_t Mb, uint32_t* out_masks) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  int rc = check_range_shape(kind, F, fields, lo, hi, C, M, base, Mb);
  if (rc) return rc;
  const int64_t n_docs = h->ix.n_docs, W = (n_docs + 31) >> 5;
  if (M == 0 || W == 0) return BM25_OK;
  if (!out_masks) return fail(BM25_EINVAL, "NULL output");
  if (F > 0 && !values) return fail(BM25_EINVAL, "NULL values");
  rc = check_ranges(kind, F, fields, lo, hi, C, M);
  if (rc) return rc;
  Enter in(h);
  if (in.rc) return in.rc;
  const int64_t es = (int64_t)field_bytes(kind);
  HostCall c(h->stream);
  const char* d_values = c.upload((const char*)values, F * n_docs * es);
  const int32_t* d_fields = c.upload(fields, M * C);
  const char* d_lo = c.upload((const char*)lo, M * C * es);
  const char* d_hi = c.upload((const char*)hi, M * C * es);
  const uint32_t* d_base = c.upload(base, Mb * W);
  uint32_t* d_out = c.alloc<uint32_t>(M * W);
  if (c.ok())
    c.run(launch_range_masks(h->ix, d_values, kind, F, d_fields, d_lo, d_hi, C, M, d_base, Mb,
                             d_out, h->stream));
  c.download(out_masks, d_out, M * W);
  return c.finish("range_masks");
}

int bm25_range_masks_device(bm25_index* h, const void* d_values, int32_t kind, int64_t F,
                            const int32_t* d_fields, const void* d_lo, const void* d_hi, int64_t C,
                            int64_t M, const uint32_t* d_base, int64_t Mb, uint32_t* d_out_masks,
                            void* stream) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  const int rc = check_range_shape(kind, F, d_fields, d_lo, d_hi, C, M, d_base, Mb);
  if (rc) return rc;
  if (M == 0 || h->ix.n_docs == 0) return BM25_OK;
  if (!d_out_masks) return fail(BM25_EINVAL, "NULL output");
  if (F > 0 && !d_values) return fail(BM25_EINVAL, "NULL values");
  // reads the caller's buffers only (as bm25_mask_facets_device: no workspace,
  // no index array, no ordering against the handle's searches)
  Enter in(h);
  if (in.rc) return in.rc;
  HIP_TRY(launch_range_masks(h->ix, d_values, kind, F, d_fields, d_lo, d_hi, C, M, d_base, Mb,
                             d_out_masks, (hipStream_t)stream),
          "range_masks launch");
  return BM25_OK;
}

int bm25_sort_ranks(bm25_index* h, const void* values, int32_t kind, int32_t descending,
                    int32_t* out_ranks, int32_t* out_perm) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  const int rc = check_kind(kind);
  if (rc) return rc;
  const int64_t n = h->ix.n_docs;
  if (n == 0) return BM25_OK;
  if (!values) return fail(BM25_EINVAL, "NULL values");
  if (!out_ranks || !out_perm) return fail(BM25_EINVAL, "NULL output");
  Enter in(h);
  if (in.rc) return in.rc;
  HostCall c(h->stream);
  const char* d_values = c.upload((const char*)values, n * (int64_t)field_bytes(kind));
  int32_t* d_ranks = c.alloc<int32_t>(n);
  int32_t* d_perm = c.alloc<int32_t>(n);
  if (c.ok())
    c.run(launch_sort_ranks(h->ix, d_values, kind, descending != 0, d_ranks, d_perm, h->stream));
  c.download(out_ranks, d_ranks, n);
  c.download(out_perm, d_perm, n);
  return c.finish("sort_ranks");
}

int bm25_sort_ranks_device(bm25_index* h, const void* d_values, int32_t kind, int32_t descending,
                           int32_t* d_ranks, int32_t* d_perm, void* stream) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  const int rc = check_kind(kind);
  if (rc) return rc;
  if (h->ix.n_docs == 0) return BM25_OK;
  if (!d_values) return fail(BM25_EINVAL, "NULL values");
  if (!d_ranks || !d_perm) return fail(BM25_EINVAL, "NULL output");
  // a setup call: reads the caller's column only, takes and frees the sort's
  // buffers and waits for `stream` before they go
  Enter in(h);
  if (in.rc) return in.rc;
  HIP_TRY(launch_sort_ranks(h->ix, d_values, kind, descending != 0, d_ranks, d_perm,
                            (hipStream_t)stream),
          "sort_ranks");
  return BM25_OK;
}

int bm25_search_sorted_scratch(const bm25_index* h, int64_t M, int32_t k, int64_t* bytes) {
  if (!h || !bytes) return fail(BM25_EINVAL, h ? "NULL output" : "NULL index");
  const int rc = check_sorted_shape(h, M, k);
  if (rc) return rc;
  *bytes = sorted_scratch_bytes(h->ix.n_docs, M, k);
  return BM25_OK;
}

int bm25_search_sorted(bm25_index* h, const uint32_t* masks, int64_t M, const int32_t* ranks,
                       const int32_t* perm, int32_t k, const int32_t* after_ranks,
                       int32_t* out_docs, int32_t* out_ranks) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  int rc = check_sorted_shape(h, M, k);
  if (rc) return rc;
  if (M == 0 || k == 0) return BM25_OK;
  if (!ranks || !perm) return fail(BM25_EINVAL, "NULL ranks or perm");
  if (!out_docs || !out_ranks) return fail(BM25_EINVAL, "NULL output");
  const int64_t n = h->ix.n_docs, W = (n + 31) >> 5;
  rc = check_sort_order(ranks, perm, n);
  if (rc) return rc;
  rc = check_after_ranks(after_ranks, M);
  if (rc) return rc;
  Enter in(h);
  if (in.rc) return in.rc;
  // staging buffers of this call's own (as bm25_mask_facets)
  HostCall c(h->stream);
  const uint32_t* d_masks = c.upload(masks, masks ? M * W : 0);
  const int32_t* d_ranks = c.upload(ranks, n);
  const int32_t* d_perm = c.upload(perm, n);
  const int32_t* d_after = c.upload(after_ranks, after_ranks ? M : 0);
  int32_t* d_docs = c.alloc<int32_t>(M * k);
  int32_t* d_or = c.alloc<int32_t>(M * k);
  char* d_scratch = c.alloc<char>(sorted_scratch_bytes(n, M, k));
  if (c.ok())
    c.run(launch_search_sorted(h->ix, d_masks, M, d_ranks, d_perm, k, d_after, d_docs, d_or,
                               d_scratch, h->ix.opt.sorted_bins, h->stream));
  c.download(out_docs, d_docs, M * k);
  c.download(out_ranks, d_or, M * k);
  return c.finish("search_sorted");
}

int bm25_search_sorted_device(bm25_index* h, const uint32_t* d_masks, int64_t M,
                              const int32_t* d_ranks, const int32_t* d_perm, int32_t k,
                              const int32_t* d_after_ranks, int32_t* d_docs, int32_t* d_out_ranks,
                              void* d_scratch, int64_t scratch_bytes, void* stream) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  const int rc = check_sorted_shape(h, M, k);
  if (rc) return rc;
  if (M == 0 || k == 0) return BM25_OK;
  if (!d_ranks || !d_perm) return fail(BM25_EINVAL, "NULL ranks or perm");
  if (!d_docs || !d_out_ranks) return fail(BM25_EINVAL, "NULL output");
  const int64_t need = sorted_scratch_bytes(h->ix.n_docs, M, k);
  if (d_masks && (!d_scratch || scratch_bytes < need))
    return fail(BM25_EINVAL, "scratch of %lld bytes: bm25_search_sorted_scratch asks for %lld",
                (long long)(d_scratch ? scratch_bytes : 0), (long long)need);
  if (((uintptr_t)d_scratch & 3u) != 0) return fail(BM25_EINVAL, "scratch must be 4-byte aligned");
  // reads the caller's buffers only (as bm25_mask_facets_device: no workspace,
  // no index array, no ordering against the handle's searches)
  Enter in(h);
  if (in.rc) return in.rc;
  HIP_TRY(launch_search_sorted(h->ix, d_masks, M, d_ranks, d_perm, k, d_after_ranks, d_docs,
                               d_out_ranks, d_scratch, h->ix.opt.sorted_bins, (hipStream_t)stream),
          "search_sorted launch");
  return BM25_OK;
}

int bm25_term_masks(bm25_index* h, const int32_t* must, int64_t A, const int32_t* any, int64_t B,
                    const int32_t* must_not, int64_t N, int64_t M, const uint32_t* base, int64_t Mb,
                    uint32_t* out_masks) {
  return bm25_term_masks_min_match(h, must, A, any, B, must_not, N, nullptr, M, base, Mb, out_masks);
}

int bm25_term_masks_min_match(bm25_index* h, const int32_t* must, int64_t A, const int32_t* any,
                              int64_t B, const int32_t* must_not, int64_t N,
                              const int32_t* min_match, int64_t M, const uint32_t* base, int64_t Mb,
                              uint32_t* out_masks) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  int rc = check_clauses(must, A, any, B, must_not, N, M, base, Mb);
  if (rc) return rc;
  rc = check_min_match(min_match, B, M, true);
  if (rc) return rc;
  const int64_t W = (h->ix.n_docs + 31) >> 5;
  if (M == 0 || W == 0) return BM25_OK;
  if (!out_masks) return fail(BM25_EINVAL, "NULL output");
  rc = check_clause_ids(h, 0, must, A, any, B, must_not, N, M);
  if (rc) return rc;
  Enter in(h);
  if (in.rc) return in.rc;
  // staging buffers of this call's own (as bm25_score_docs)
  HostCall c(h->stream);
  const int32_t* d_must = c.upload(must, M * A);
  const int32_t* d_any = c.upload(any, M * B);
  const int32_t* d_not = c.upload(must_not, M * N);
  const uint32_t* d_base = c.upload(base, Mb * W);
  const int32_t* d_mm = c.upload(min_match, min_match ? M : 0);
  uint32_t* d_out = c.alloc<uint32_t>(M * W);
  if (c.ok())
    c.run(launch_term_masks(h->ix, d_must, A, d_any, B, d_not, N, M, d_base, Mb, d_out, h->stream,
                            d_mm));
  c.download(out_masks, d_out, M * W);
  return c.finish("term_masks");
}

int bm25_term_masks_device(bm25_index* h, const int32_t* d_must, int64_t A, const int32_t* d_any,
                           int64_t B, const int32_t* d_must_not, int64_t N, int64_t M,
                           const uint32_t* d_base, int64_t Mb, uint32_t* d_out_masks, void* stream) {
  return bm25_term_masks_min_match_device(h, d_must, A, d_any, B, d_must_not, N, nullptr, M, d_base,
                                          Mb, d_out_masks, stream);
}

int bm25_term_masks_min_match_device(bm25_index* h, const int32_t* d_must, int64_t A,
                                     const int32_t* d_any, int64_t B, const int32_t* d_must_not,
                                     int64_t N, const int32_t* d_min_match, int64_t M,
                                     const uint32_t* d_base, int64_t Mb, uint32_t* d_out_masks,
                                     void* stream) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  int rc = check_clauses(d_must, A, d_any, B, d_must_not, N, M, d_base, Mb);
  if (rc) return rc;
  rc = check_min_match(d_min_match, B, M, false);
  if (rc) return rc;
  if (M == 0 || h->ix.n_docs == 0) return BM25_OK;
  if (!d_out_masks) return fail(BM25_EINVAL, "NULL output");
  // reads the immutable index arrays only: no workspace, no ordering against
  // the handle's searches (ws_stream)
  Enter in(h);
  if (in.rc) return in.rc;
  HIP_TRY(launch_term_masks(h->ix, d_must, A, d_any, B, d_must_not, N, M, d_base, Mb, d_out_masks,
                            (hipStream_t)stream, d_min_match),
          "term_masks launch");
  return BM25_OK;
}

int bm25_mask_count(bm25_index* h, const uint32_t* masks, int64_t M, int64_t* out_counts) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  if (M < 0) return fail(BM25_EINVAL, "negative mask shape");
  if (M == 0) return BM25_OK;
  if (!out_counts) return fail(BM25_EINVAL, "NULL output");
  const int64_t W = (h->ix.n_docs + 31) >> 5;
  if (W > 0 && !masks) return fail(BM25_EINVAL, "NULL masks");
  Enter in(h);
  if (in.rc) return in.rc;
  HostCall c(h->stream);
  const uint32_t* d_masks = c.upload(masks, M * W);
  int64_t* d_counts = c.alloc<int64_t>(M);
  if (c.ok()) c.run(launch_mask_count(h->ix, d_masks, M, d_counts, h->stream));
  c.download(out_counts, d_counts, M);
  return c.finish("mask_count");
}

int bm25_mask_count_device(bm25_index* h, const uint32_t* d_masks, int64_t M, int64_t* d_counts,
                           void* stream) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  if (M < 0) return fail(BM25_EINVAL, "negative mask shape");
  if (M == 0) return BM25_OK;
  if (!d_counts) return fail(BM25_EINVAL, "NULL output");
  if (h->ix.n_docs > 0 && !d_masks) return fail(BM25_EINVAL, "NULL masks");
  // reads the caller's masks only (as bm25_term_masks_device: no workspace)
  Enter in(h);
  if (in.rc) return in.rc;
  HIP_TRY(launch_mask_count(h->ix, d_masks, M, d_counts, (hipStream_t)stream), "mask_count launch");
  return BM25_OK;
}

int bm25_mask_facets(bm25_index* h, const uint32_t* masks, int64_t M, const int32_t* groups,
                     int64_t G, int64_t* out_counts) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  int rc = check_facet_shape(M, G);
  if (rc) return rc;
  if (M == 0 || G == 0) return BM25_OK;
  if (!out_counts) return fail(BM25_EINVAL, "NULL output");
  const int64_t n_docs = h->ix.n_docs, W = (n_docs + 31) >> 5;
  if (W > 0 && !masks) return fail(BM25_EINVAL, "NULL masks");
  if (n_docs > 0 && !groups) return fail(BM25_EINVAL, "NULL groups");
  rc = check_groups(groups, n_docs, G);
  if (rc) return rc;
  Enter in(h);
  if (in.rc) return in.rc;
  HostCall c(h->stream);
  const uint32_t* d_masks = c.upload(masks, M * W);
  const int32_t* d_groups = c.upload(groups, n_docs);
  int64_t* d_counts = c.alloc<int64_t>(M * G);
  if (c.ok()) c.run(launch_mask_facets(h->ix, d_masks, M, d_groups, G, d_counts, h->stream));
  c.download(out_counts, d_counts, M * G);
  return c.finish("mask_facets");
}

int bm25_mask_facets_device(bm25_index* h, const uint32_t* d_masks, int64_t M,
                            const int32_t* d_groups, int64_t G, int64_t* d_counts, void* stream) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  const int rc = check_facet_shape(M, G);
  if (rc) return rc;
  if (M == 0 || G == 0) return BM25_OK;
  if (!d_counts) return fail(BM25_EINVAL, "NULL output");
  if (h->ix.n_docs > 0 && !d_masks) return fail(BM25_EINVAL, "NULL masks");
  if (h->ix.n_docs > 0 && !d_groups) return fail(BM25_EINVAL, "NULL groups");
  // reads the caller's masks and groups only (as bm25_mask_count_device: no workspace)
  Enter in(h);
  if (in.rc) return in.rc;
  HIP_TRY(launch_mask_facets(h->ix, d_masks, M, d_groups, G, d_counts, (hipStream_t)stream),
          "mask_facets launch");
  return BM25_OK;
}

int bm25_mask_stats_scratch(const bm25_index* h, int32_t kind, int64_t M, int64_t G,
                            int64_t* bytes) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  int rc = check_kind(kind);
  if (!rc) rc = check_facet_shape(M, G);
  if (rc) return rc;
  if (!bytes) return fail(BM25_EINVAL, "NULL output");
  const int64_t b = stats_scratch_bytes(kind, M, G);
  if (b < 0)
    return fail(BM25_EINVAL, "M = %lld rows of %lld buckets: the scratch does not fit int64 bytes",
                (long long)M, (long long)(G > 0 ? G : 1));
  *bytes = b;
  return BM25_OK;
}

int bm25_mask_stats(bm25_index* h, const uint32_t* masks, int64_t M, const void* values,
                    int32_t kind, const int32_t* groups, int64_t G, int64_t* out_count,
                    void* out_min, void* out_max, void* out_sum) {
  int64_t bytes = 0;
  int rc = bm25_mask_stats_scratch(h, kind, M, G, &bytes);
  if (rc) return rc;
  if ((groups == nullptr) != (G == 0))
    return fail(BM25_EINVAL, "stats: groups and G come together (groups NULL with G = 0: one "
                             "bucket per row)");
  if (M == 0) return BM25_OK;
  if (!out_count) return fail(BM25_EINVAL, "NULL output");
  const int64_t n_docs = h->ix.n_docs, W = (n_docs + 31) >> 5, B = G > 0 ? G : 1;
  if (W > 0 && !masks) return fail(BM25_EINVAL, "NULL masks");
  if (n_docs > 0 && !values) return fail(BM25_EINVAL, "NULL values");
  if (groups) {
    rc = check_groups(groups, n_docs, G);
    if (rc) return rc;
  }
  Enter in(h);
  if (in.rc) return in.rc;
  const int64_t es = (int64_t)field_bytes(kind);
  HostCall c(h->stream);
  const uint32_t* d_masks = c.upload(masks, M * W);
  const char* d_values = c.upload((const char*)values, n_docs * es);
  const int32_t* d_groups = groups ? c.upload(groups, n_docs) : nullptr;
  // (with no document the groups are not read: any non-null pointer says "grouped")
  if (groups && !d_groups) d_groups = c.alloc<int32_t>(1);
  int64_t* d_count = c.alloc<int64_t>(M * B);
  char* d_min = out_min ? c.alloc<char>(M * B * es) : nullptr;
  char* d_max = out_max ? c.alloc<char>(M * B * es) : nullptr;
  int64_t* d_sum = out_sum ? c.alloc<int64_t>(M * B) : nullptr;
  char* d_scratch = c.alloc<char>(bytes);
  if (c.ok())
    c.run(launch_mask_stats(h->ix, d_masks, M, d_values, kind, d_groups, G, d_count, d_min, d_max,
                            d_sum, d_scratch, h->stream));
  c.download(out_count, d_count, M * B);
  if (out_min) c.download((char*)out_min, d_min, M * B * es);
  if (out_max) c.download((char*)out_max, d_max, M * B * es);
  if (out_sum) c.download((int64_t*)out_sum, d_sum, M * B);  // (int64 or float64: 8 bytes)
  return c.finish("mask_stats");
}

int bm25_mask_stats_device(bm25_index* h, const uint32_t* d_masks, int64_t M, const void* d_values,
                           int32_t kind, const int32_t* d_groups, int64_t G, int64_t* d_count,
                           void* d_min, void* d_max, void* d_sum, void* d_scratch,
                           int64_t scratch_bytes, void* stream) {
  int64_t bytes = 0;
  const int rc = bm25_mask_stats_scratch(h, kind, M, G, &bytes);
  if (rc) return rc;
  if ((d_groups == nullptr) != (G == 0))
    return fail(BM25_EINVAL, "stats: groups and G come together (groups NULL with G = 0: one "
                             "bucket per row)");
  if (M == 0) return BM25_OK;
  if (!d_count) return fail(BM25_EINVAL, "NULL output");
  if (h->ix.n_docs > 0 && !d_masks) return fail(BM25_EINVAL, "NULL masks");
  if (h->ix.n_docs > 0 && !d_values) return fail(BM25_EINVAL, "NULL values");
  if (!d_scratch) return fail(BM25_EINVAL, "NULL scratch");
  if (scratch_bytes < bytes)
    return fail(BM25_EINVAL, "scratch_bytes = %lld: bm25_mask_stats_scratch asks for %lld",
                (long long)scratch_bytes, (long long)bytes);
  if ((uintptr_t)d_scratch % 8)
    return fail(BM25_EINVAL, "the scratch must be 8-byte aligned");
  // reads the caller's buffers only (as bm25_mask_facets_device: no workspace,
  // no index array, no ordering against the handle's searches)
  Enter in(h);
  if (in.rc) return in.rc;
  HIP_TRY(launch_mask_stats(h->ix, d_masks, M, d_values, kind, d_groups, G, d_count, d_min, d_max,
                            d_sum, d_scratch, (hipStream_t)stream),
          "mask_stats launch");
  return BM25_OK;
}

int bm25_search_boolean(bm25_index* h, const int32_t* queries, int64_t Q, int64_t T, int32_t k,
                        const int32_t* must, int64_t A, const int32_t* any, int64_t B,
                        const int32_t* must_not, int64_t N, const uint32_t* base, int64_t Mb,
                        int32_t* out_docs, float* out_scores) {
  return bm25_search_boolean_min_match(h, queries, Q, T, k, must, A, any, B, must_not, N, nullptr,
                                       base, Mb, out_docs, out_scores, nullptr);
}

int bm25_search_boolean_min_match(bm25_index* h, const int32_t* queries, int64_t Q, int64_t T,
                                  int32_t k, const int32_t* must, int64_t A, const int32_t* any,
                                  int64_t B, const int32_t* must_not, int64_t N,
                                  const int32_t* min_match, const uint32_t* base, int64_t Mb,
                                  int32_t* out_docs, float* out_scores, int64_t* out_total_hits) {
  return bm25_search_boolean_facets(h, queries, Q, T, k, must, A, any, B, must_not, N, min_match,
                                    base, Mb, nullptr, 0, out_docs, out_scores, out_total_hits,
                                    nullptr);
}

int bm25_search_boolean_facets(bm25_index* h, const int32_t* queries, int64_t Q, int64_t T,
                               int32_t k, const int32_t* must, int64_t A, const int32_t* any,
                               int64_t B, const int32_t* must_not, int64_t N,
                               const int32_t* min_match, const uint32_t* base, int64_t Mb,
                               const int32_t* groups, int64_t G, int32_t* out_docs,
                               float* out_scores, int64_t* out_total_hits, int64_t* out_facets) {
  return bm25_search_boolean_ranges(h, queries, Q, T, k, must, A, any, B, must_not, N, min_match,
                                    base, Mb, groups, G, nullptr, BM25_FIELD_I32, 0, nullptr,
                                    nullptr, nullptr, 0, out_docs, out_scores, out_total_hits,
                                    out_facets);
}

int bm25_search_boolean_ranges(bm25_index* h, const int32_t* queries, int64_t Q, int64_t T,
                               int32_t k, const int32_t* must, int64_t A, const int32_t* any,
                               int64_t B, const int32_t* must_not, int64_t N,
                               const int32_t* min_match, const uint32_t* base, int64_t Mb,
                               const int32_t* groups, int64_t G, const void* values, int32_t kind,
                               int64_t F, const int32_t* fields, const void* lo, const void* hi,
                               int64_t C, int32_t* out_docs, float* out_scores,
                               int64_t* out_total_hits, int64_t* out_facets) {
  return bm25_search_boolean_sorted(h, queries, Q, T, k, must, A, any, B, must_not, N, min_match,
                                    base, Mb, groups, G, values, kind, F, fields, lo, hi, C,
                                    out_docs, out_scores, out_total_hits, out_facets, nullptr,
                                    nullptr, nullptr, nullptr);
}

int bm25_search_boolean_sorted(bm25_index* h, const int32_t* queries, int64_t Q, int64_t T,
                               int32_t k, const int32_t* must, int64_t A, const int32_t* any,
                               int64_t B, const int32_t* must_not, int64_t N,
                               const int32_t* min_match, const uint32_t* base, int64_t Mb,
                               const int32_t* groups, int64_t G, const void* values, int32_t kind,
                               int64_t F, const int32_t* fields, const void* lo, const void* hi,
                               int64_t C, int32_t* out_docs, float* out_scores,
                               int64_t* out_total_hits, int64_t* out_facets, const int32_t* ranks,
                               const int32_t* perm, const int32_t* after_ranks,
                               int32_t* out_ranks) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  // (ranks == NULL: bm25_search_boolean_ranges, the order by score)
  const bool sorted = ranks != nullptr;
  if (Q < 0 || T < 0) return fail(BM25_EINVAL, "negative query shape");
  int rc = check_clauses(must, A, any, B, must_not, N, Q, base, Mb);
  if (rc) return rc;
  rc = check_min_match(min_match, B, Q, true);
  if (rc) return rc;
  rc = check_facet_shape(Q, G);
  if (rc) return rc;
  if (F < 0 || C < 0) return fail(BM25_EINVAL, "negative range or mask shape");
  // (F == 0, C == 0 or no values: no range clause, today's path unchanged)
  const bool ranged = values && F > 0 && C > 0;
  if (ranged) {
    rc = check_range_shape(kind, F, fields, lo, hi, C, Q, nullptr, 0);
    if (rc) return rc;
  }
  if (G > 0 && (groups == nullptr) != (out_facets == nullptr))
    return fail(BM25_EINVAL, "facets: groups and out_facets come together (one of them is NULL)");
  if (G == 0 || !groups) out_facets = nullptr;  // (no group: no facet row to write)
  rc = check_k(h->ix.n_docs, k);
  if (rc) return rc;
  if (sorted && k > kMaxK)
    return fail(BM25_EINVAL, "k = %d: a sorted search returns at most %d hits a row", (int)k,
                (int)kMaxK);
  // (k == 0 with out_total_hits or out_facets: "how many match" alone — the
  // masks are still built and counted)
  if (Q == 0 || (k == 0 && !out_total_hits && !out_facets)) return BM25_OK;
  if (k > 0 && T > 0 && !queries) return fail(BM25_EINVAL, "NULL queries");
  if (k > 0 && (!out_docs || !out_scores)) return fail(BM25_EINVAL, "NULL output");
  if (sorted && k > 0) {
    if (!perm) return fail(BM25_EINVAL, "NULL perm");
    if (!out_ranks) return fail(BM25_EINVAL, "NULL output");
    rc = check_sort_order(ranks, perm, h->ix.n_docs);
    if (rc) return rc;
    rc = check_after_ranks(after_ranks, Q);
    if (rc) return rc;
  }
  rc = check_clause_ids(h, max_token(0, queries, k > 0 ? Q * T : 0), must, A, any, B, must_not, N,
                        Q);
  if (rc) return rc;
  if (out_facets) {
    rc = check_groups(groups, h->ix.n_docs, G);
    if (rc) return rc;
  }
  if (ranged) {
    rc = check_ranges(kind, F, fields, lo, hi, C, Q);
    if (rc) return rc;
  }
  Enter in(h);
  if (in.rc) return in.rc;
  rc = ensure_io(h, k > 0 ? Q * T : 0, Q * (int64_t)k);
  if (rc) return rc;
  // queries per chunk: the masks of one chunk stay on the device, in a buffer
  // of this call's own of at most 1 GiB (automatic) and at least one query
  const int64_t W = (h->ix.n_docs + 31) >> 5;
  if (W == 0) {  // (k == 0: an index without documents matches none)
    if (out_total_hits) std::fill(out_total_hits, out_total_hits + Q, (int64_t)0);
    if (out_facets) std::fill(out_facets, out_facets + Q * G, (int64_t)0);
    return BM25_OK;
  }
  // (with ranges a chunk holds two buffers: the automatic chunk halves)
  int64_t chunk = h->ix.opt.bool_chunk > 0
                      ? h->ix.opt.bool_chunk
                      : std::max<int64_t>(1, ((int64_t)1 << (ranged ? 27 : 28)) / W);
  chunk = std::min(chunk, Q);
  std::vector<int32_t> ids((size_t)chunk);
  for (int64_t i = 0; i < chunk; ++i) ids[(size_t)i] = (int32_t)i;
  HostCall c(h->stream);
  const int32_t* d_must = c.upload(must, Q * A);
  const int32_t* d_any = c.upload(any, Q * B);
  const int32_t* d_not = c.upload(must_not, Q * N);
  const uint32_t* d_base = c.upload(base, Mb * W);
  const int32_t* d_mm = c.upload(min_match, min_match ? Q : 0);
  int64_t* d_hits = out_total_hits ? c.alloc<int64_t>(Q) : nullptr;
  // the groups go up once per call; every chunk's facet rows land in one [Q, G] buffer
  const int32_t* d_groups = out_facets ? c.upload(groups, h->ix.n_docs) : nullptr;
  int64_t* d_facets = out_facets ? c.alloc<int64_t>(Q * G) : nullptr;
  uint32_t* d_masks = c.alloc<uint32_t>(chunk * W);
  // the columns go up once per call; every chunk's range masks land in a second
  // buffer, the chunk's per-row base of the term masks (whose base and out are
  // __restrict__: never one buffer)
  const int64_t es = (int64_t)field_bytes(kind);
  const char* d_values = ranged ? c.upload((const char*)values, F * h->ix.n_docs * es) : nullptr;
  const int32_t* d_fields = ranged ? c.upload(fields, Q * C) : nullptr;
  const char* d_lo = ranged ? c.upload((const char*)lo, Q * C * es) : nullptr;
  const char* d_hi = ranged ? c.upload((const char*)hi, Q * C * es) : nullptr;
  uint32_t* d_rmasks = ranged ? c.alloc<uint32_t>(chunk * W) : nullptr;
  int32_t* d_qm = c.alloc<int32_t>(chunk);
  c.upload_to(d_qm, ids.data(), chunk);
  if (k > 0) c.upload_to(h->d_q, queries, Q * T);
  // the order goes up once per call; a chunk's rows are selected by rank into
  // the staging rows, in scratch of this call's own
  const bool by_rank = sorted && k > 0;
  const int32_t* d_ranks = by_rank ? c.upload(ranks, h->ix.n_docs) : nullptr;
  const int32_t* d_perm = by_rank ? c.upload(perm, h->ix.n_docs) : nullptr;
  const int32_t* d_after = by_rank && after_ranks ? c.upload(after_ranks, Q) : nullptr;
  int32_t* d_oranks = by_rank ? c.alloc<int32_t>(Q * k) : nullptr;
  char* d_sscratch =
      by_rank ? c.alloc<char>(sorted_scratch_bytes(h->ix.n_docs, chunk, k)) : nullptr;
  int64_t n_dense = 0;
  for (int64_t q0 = 0; c.ok() && q0 < Q; q0 += chunk) {
    const int64_t n = std::min(chunk, Q - q0);
    const uint32_t* cbase = Mb == Q && Q > 1 ? d_base + q0 * W : d_base;
    int64_t cMb = Mb == 0 ? 0 : (Mb == 1 ? 1 : n);
    if (ranged) {
      c.run(launch_range_masks(h->ix, d_values, kind, F, d_fields + q0 * C, d_lo + q0 * C * es,
                               d_hi + q0 * C * es, C, n, cbase, cMb, d_rmasks, h->stream));
      if (!c.ok()) break;
      cbase = d_rmasks;
      cMb = n;
    }
    c.run(launch_term_masks(h->ix, d_must + q0 * A, A, d_any + q0 * B, B, d_not + q0 * N, N, n,
                            cbase, cMb, d_masks, h->stream, d_mm ? d_mm + q0 : nullptr));
    // the chunk's counts, before its mask buffer is reused
    if (d_hits && c.ok()) c.run(launch_mask_count(h->ix, d_masks, n, d_hits + q0, h->stream));
    if (d_facets && c.ok())
      c.run(launch_mask_facets(h->ix, d_masks, n, d_groups, G, d_facets + q0 * G, h->stream));
    if (!c.ok()) break;
    if (k == 0) continue;  // (the counts alone: no search ran, the handle's counters stay)
    if (by_rank) {
      // the rows by rank, their scores by the point lookup (a padding slot
      // scores +0.0f there), then the tails' score bits
      c.run(launch_search_sorted(h->ix, d_masks, n, d_ranks, d_perm, k,
                                 d_after ? d_after + q0 : nullptr, h->d_docs + q0 * k,
                                 d_oranks + q0 * k, d_sscratch, h->ix.opt.sorted_bins, h->stream));
      if (c.ok())
        c.run(launch_score_docs(h->ix, h->d_q + q0 * T, n, T, h->d_docs + q0 * k, k,
                                h->d_scores + q0 * k, h->stream));
      if (c.ok())
        c.run(launch_sorted_pad_scores(h->d_docs + q0 * k, h->d_scores + q0 * k, n * k, h->stream));
      continue;
    }
    RankedDev rows;  // the chunk's queries, each under its own mask
    rows.d_queries = h->d_q + q0 * T;
    rows.d_masks = d_masks, rows.M = n, rows.d_query_mask = d_qm;
    c.hold(run_filtered(h, n, T, k, rows, h->d_docs + q0 * k, h->d_scores + q0 * k, h->stream));
    n_dense += h->filtered_dense;
  }
  if (k > 0 && !by_rank) h->filtered_dense = n_dense;
  c.download(out_docs, h->d_docs, Q * k);
  c.download(out_scores, h->d_scores, Q * k);
  if (by_rank) c.download(out_ranks, d_oranks, Q * k);
  if (d_hits) c.download(out_total_hits, d_hits, Q);
  if (d_facets) c.download(out_facets, d_facets, Q * G);
  return c.finish("boolean search");
}

int bm25_index_bounds_export(bm25_index* h, uint16_t* d_out, int64_t stride, void* stream) {
  if (!h || !d_out) return fail(BM25_EINVAL, "NULL argument");
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->ix.bmax)
    return fail(BM25_EINVAL, "the index keeps no tile bounds (a dense, non-negative index does)");
  const int64_t bs = bmax_stride(h->ix.ntiles);
  if (stride < bs || stride % 4 != 0)
    return fail(BM25_EINVAL, "stride %lld: a multiple of 4, >= %lld", (long long)stride, (long long)bs);
  HIP_TRY(hipSetDevice(h->ix.device), "hipSetDevice");
  const hipStream_t st = (hipStream_t)stream;
  const int64_t V = h->ix.n_terms;
  if (V == 0) return BM25_OK;
  if (stride > bs) HIP_TRY(hipMemsetAsync(d_out, 0, sizeof(uint16_t) * V * stride, st), "hipMemsetAsync");
  if (bs > 0)
    HIP_TRY(hipMemcpy2DAsync(d_out, sizeof(uint16_t) * stride, h->ix.bmax, sizeof(uint16_t) * bs,
                             sizeof(uint16_t) * bs, V, hipMemcpyDeviceToDevice, st),
            "hipMemcpy2DAsync");
  return BM25_OK;
}

int bm25_index_masks_export(bm25_index* h, uint32_t* d_out, int64_t stride, void* stream) {
  if (!h || !d_out) return fail(BM25_EINVAL, "NULL argument");
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->ix.tmask)
    return fail(BM25_EINVAL, "the index keeps no sub-block masks (tile bounds and BM25_TILE_MASK != 0 "
                             "at create)");
  const int64_t bs = bmax_stride(h->ix.ntiles);
  if (stride < bs || stride % 4 != 0)
    return fail(BM25_EINVAL, "stride %lld: a multiple of 4, >= %lld", (long long)stride, (long long)bs);
  HIP_TRY(hipSetDevice(h->ix.device), "hipSetDevice");
  const hipStream_t st = (hipStream_t)stream;
  const int64_t V = h->ix.n_terms;
  if (V == 0) return BM25_OK;
  if (stride > bs) HIP_TRY(hipMemsetAsync(d_out, 0, sizeof(uint32_t) * V * stride, st), "hipMemsetAsync");
  if (bs > 0)
    HIP_TRY(hipMemcpy2DAsync(d_out, sizeof(uint32_t) * stride, h->ix.tmask, sizeof(uint32_t) * bs,
                             sizeof(uint32_t) * bs, V, hipMemcpyDeviceToDevice, st),
            "hipMemcpy2DAsync");
  return BM25_OK;
}

// The pooled world table (DevIndex::wbpool) of a handle with world bounds,
// built on the handle's stream once the device is idle (the caller's table
// finished on whatever stream wrote it) and owned by the handle; without the
// memory, none (the per-tile table serves).
static int pool_world(bm25_index* h) {
  DevIndex& ix = h->ix;
  const int64_t ps = bmax_stride(ix.wstride / kPool);
  const int64_t rows = (int64_t)ix.wW * ix.n_terms;
  if (rows > 0 && hipMalloc(&ix.wbpool, sizeof(uint16_t) * rows * ps) == hipSuccess) {
    // the caller's table may still be in flight on any of its streams (the
    // exports, the all-gather): the whole device first — a setup call
    HIP_TRY(hipDeviceSynchronize(), "hipDeviceSynchronize");
    HIP_TRY(launch_pool_bounds(ix.wbmax, rows, ix.wstride, ix.wbpool, ps, h->stream), "pool_bounds launch");
    HIP_TRY(hipStreamSynchronize(h->stream), "pool_bounds");
    ix.wpstride = ps;
    // (a lower estimate of the collection's groups: each shard has ceil(its
    // tiles / kPool) of them)
    ix.wgroups = std::min<int64_t>((ix.wtiles + kPool - 1) / kPool, (int64_t)ix.wW * ps);
  } else {
    (void)hipGetLastError();
    ix.wbpool = nullptr;
    ix.wpstride = ix.wgroups = 0;
  }
  return BM25_OK;
}

int bm25_index_set_world_bounds(bm25_index* h, const uint16_t* d_world, int32_t world,
                                int64_t stride, int64_t world_tiles) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  std::lock_guard<std::mutex> lk(h->mu);
  auto clear = [&]() {
    if (h->ix.wbpool) {  // (searches still reading it: on the handle's last stream)
      if (h->ws_stream) hipStreamSynchronize(h->ws_stream);
      hipStreamSynchronize(h->stream);
      hipFree(h->ix.wbpool);
    }
    h->ix.wbmax = nullptr;
    h->ix.wbpool = nullptr;
    h->ix.wW = 0;
    h->ix.wstride = h->ix.wtiles = h->ix.wpstride = h->ix.wgroups = 0;
  };
  if (!d_world) {
    HIP_TRY(hipSetDevice(h->ix.device), "hipSetDevice");
    clear();
    return BM25_OK;
  }
  if (!h->ix.bmax)
    return fail(BM25_EINVAL, "the index keeps no tile bounds (a dense, non-negative index does)");
  if (world < 1 || stride % 4 != 0 || stride < bmax_stride(h->ix.ntiles) || world_tiles < 1 ||
      world_tiles > (int64_t)world * stride)
    return fail(BM25_EINVAL, "bad world bounds (world %d, stride %lld, tiles %lld)", world,
                (long long)stride, (long long)world_tiles);
  if ((int64_t)world * stride > kBoundMaxTiles + 4 * (int64_t)world)
    return fail(BM25_EINVAL, "world bounds of %lld tiles exceed the %lld one block selects over",
                (long long)((int64_t)world * stride), (long long)kBoundMaxTiles);
  HIP_TRY(hipSetDevice(h->ix.device), "hipSetDevice");
  clear();
  h->ix.wbmax = d_world;
  h->ix.wW = world;
  h->ix.wstride = stride;
  h->ix.wtiles = world_tiles;
  return pool_world(h);
}

int bm25_search_shard_device(bm25_index* h, const int32_t* d_queries, int64_t Q, int64_t T,
                             int32_t k, int32_t* d_docs, float* d_scores, void* stream) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  if (Q < 0 || T < 0) return fail(BM25_EINVAL, "negative query shape");
  int rc = check_k(h->ix.n_docs, k, true);
  if (rc) return rc;
  if (Q == 0 || k == 0) return BM25_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->ix.wbmax) return fail(BM25_EINVAL, "no world bounds: bm25_index_set_world_bounds first");
  HIP_TRY(hipSetDevice(h->ix.device), "hipSetDevice");
  h->sampled = false;
  // k > 4096: this shard's exact top-k (padded past its documents)
  return run_search(h, d_queries, Q, T, k, d_docs, d_scores, (hipStream_t)stream, k <= kMaxK);
}

int bm25_max_token_device(bm25_index* h, const int32_t* d_queries, int64_t Q, int64_t T,
                          int32_t* max_token, void* stream) {
  if (!h || !max_token) return fail(BM25_EINVAL, "NULL argument");
  if (Q < 0 || T < 0) return fail(BM25_EINVAL, "negative query shape");
  Enter in(h);
  if (in.rc) return in.rc;
  if (!h->d_maxtok) HIP_TRY(hipMalloc(&h->d_maxtok, sizeof(int32_t)), "hipMalloc");
  const hipStream_t st = (hipStream_t)stream;
  HIP_TRY(launch_max_token(d_queries, Q * T, h->d_maxtok, st), "max_token_kernel");
  HIP_TRY(hipMemcpyAsync(max_token, h->d_maxtok, sizeof(int32_t), hipMemcpyDeviceToHost, st),
          "hipMemcpyAsync");
  HIP_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
  return BM25_OK;
}

// Two-phase search of W doc shards with a global threshold (bm25mi.h).
// (T = 0: the width alone — the same for every T, search_geom)
static SampleGeom shard_geom(const bm25_index* h, int64_t shard_docs_max, int32_t world, int k,
                             int64_t T = 0) {
  const int64_t D = 1ll << h->ix.tile_shift;
  const int64_t nt = std::max<int64_t>((std::max<int64_t>(shard_docs_max, h->ix.n_docs) + D - 1) / D, 1);
  return search_geom(h->ix, nt, k, std::max(world, 1), T);
}

int bm25_sample_width(const bm25_index* h, int64_t shard_docs_max, int32_t world, int32_t k,
                      int64_t* width) {
  if (!h || !width) return fail(BM25_EINVAL, "NULL argument");
  if (world < 1 || k < 0) return fail(BM25_EINVAL, "bad world=%d or k=%d", world, k);
  // k > kMaxK: no sample (each shard's exact top-k, bm25mi_large.hip)
  *width = (k == 0 || k > kMaxK) ? 0 : shard_geom(h, shard_docs_max, world, k).S;
  return BM25_OK;
}

int bm25_search_sample_device(bm25_index* h, const int32_t* d_queries, int64_t Q, int64_t T,
                              int32_t k, int32_t world, int64_t shard_docs_max, uint64_t* d_keys,
                              void* stream) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  if (Q < 0 || T < 0 || world < 1) return fail(BM25_EINVAL, "bad shape");
  int rc = check_k(h->ix.n_docs, k, true);
  if (rc) return rc;
  if (Q == 0 || k == 0 || k > kMaxK) return BM25_OK;  // k > kMaxK: no sample half
  Enter in(h);
  if (in.rc) return in.rc;
  const hipStream_t st = (hipStream_t)stream;
  rc = ensure_ws(h, Q, T, k, st);
  if (rc) return rc;
  HIP_TRY(order_ws(h, st), "workspace order");
  h->large_fallback = 0;
  h->split_ev = next_events(h);
  if (h->split_ev) HIP_TRY(hipEventRecord(h->split_ev->a, st), "hipEventRecord");
  choose_theta_source(h);  // (the finish half keeps this choice)
  const SampleGeom g = shard_geom(h, shard_docs_max, world, k, T);
  h->ix.disp = Dispatch{};
  h->ix.disp.sample_p = g.P;
  arm_report(h, g.P, Q);
  h->sampled = true;
  HIP_TRY(launch_sample(h->ix, d_queries, Q, T, g, d_keys, h->ws, st), "sample launch");
  return BM25_OK;
}

// The finish half on up to three streams: theta on st_theta, the REST pass
// on st_rest (after theta: an event), the merges on st_sel (after REST).  One
// stream for all three is bm25_search_finish_device.
static int finish_impl(bm25_index* h, const int32_t* d_queries, int64_t Q, int64_t T, int32_t k,
                       int32_t world, int64_t shard_docs_max, const uint64_t* d_all_keys,
                       int32_t* d_docs, float* d_scores, hipStream_t st, hipStream_t st_rest,
                       hipStream_t st_sel) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  if (Q < 0 || T < 0 || world < 1) return fail(BM25_EINVAL, "bad shape");
  int rc = check_k(h->ix.n_docs, k, true);
  if (rc) return rc;
  if (Q == 0 || k == 0) return BM25_OK;
  Enter in(h);
  if (in.rc) return in.rc;
  for (hipEvent_t& e : h->ev_split)
    if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
  // st_sel continues after everything enqueued on st (an event; none if equal)
  auto join = [&](hipStream_t from, hipStream_t to, hipEvent_t e) -> hipError_t {
    if (from == to) return hipSuccess;
    hipError_t x = hipEventRecord(e, from);
    return x != hipSuccess ? x : hipStreamWaitEvent(to, e, 0);
  };
  if (k > kMaxK) {  // this shard's exact top-k (padded past its documents)
    h->sampled = false;
    rc = run_search(h, d_queries, Q, T, k, d_docs, d_scores, st);
    if (rc) return rc;
    HIP_TRY(join(st, st_sel, h->ev_split[1]), "stream join");
    if (st_sel != st) h->ws_stream = st_sel;  // (after the join: st_sel waits for st)
    return BM25_OK;
  }
  rc = ensure_ws(h, Q, T, k, st);
  if (rc) return rc;
  HIP_TRY(order_ws(h, st), "workspace order");
  h->large_fallback = 0;
  if (!h->sampled) choose_theta_source(h);  // no sample half ran for this search (S = 0)
  const SampleGeom g = shard_geom(h, shard_docs_max, world, k, T);
  if (!h->sampled) {
    h->ix.disp = Dispatch{};
    h->ix.disp.sample_p = g.P;
    arm_report(h, g.P, Q);
  } else {
    h->ws.report = h->report_dev;  // (ensure_ws may have rebuilt the workspace)
    h->ws.seq = h->seq;
  }
  h->sampled = false;
  EventPair* ev = h->split_ev;
  h->split_ev = nullptr;
  // on three streams the score pass is timed on its own stream, from the
  // REST pass's start (the sample half and theta ran on another stream)
  HIP_TRY(launch_finish(h->ix, d_queries, Q, T, k, g, world, d_all_keys, h->ws, st, st_rest,
                        h->ev_split[0], (ev && st_rest != st) ? ev->a : nullptr),
          "finish launch");
  if (ev) HIP_TRY(hipEventRecord(ev->b, st_rest), "hipEventRecord");
  HIP_TRY(join(st_rest, st_sel, h->ev_split[1]), "stream join");
  // world > 1: this shard's list goes to the W-way merge, which sorts (no
  // sorted list needed here); world = 1 is a plain search: sorted
  HIP_TRY(launch_select(h->ix, d_queries, Q, T, k, g.P, h->ws, d_docs, d_scores, st_sel,
                        world > 1),
          "select launch");
  HIP_TRY(record_end(h, ev, st_sel), "hipEventRecord");
  h->ws_stream = st_sel;  // (the next search on another stream waits for this one)
  count_search(h);
  return BM25_OK;
}

int bm25_search_finish_device(bm25_index* h, const int32_t* d_queries, int64_t Q, int64_t T,
                              int32_t k, int32_t world, int64_t shard_docs_max,
                              const uint64_t* d_all_keys, int32_t* d_docs, float* d_scores,
                              void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  return finish_impl(h, d_queries, Q, T, k, world, shard_docs_max, d_all_keys, d_docs, d_scores,
                     st, st, st);
}

int bm25_search_finish_streams_device(bm25_index* h, const int32_t* d_queries, int64_t Q,
                                      int64_t T, int32_t k, int32_t world,
                                      int64_t shard_docs_max, const uint64_t* d_all_keys,
                                      int32_t* d_docs, float* d_scores, void* stream_theta,
                                      void* stream_rest, void* stream_select) {
  return finish_impl(h, d_queries, Q, T, k, world, shard_docs_max, d_all_keys, d_docs, d_scores,
                     (hipStream_t)stream_theta, (hipStream_t)stream_rest,
                     (hipStream_t)stream_select);
}

int bm25_build_scores(int device, int64_t n_docs, int64_t n_terms, int64_t n_triples,
                      const int32_t* docs, const int32_t* terms, const float* tfs,
                      const int32_t* doc_len, double avgdl, double k1, double b, int method,
                      const float* idf, int64_t* out_indptr, int32_t* out_indices,
                      float* out_data, double* out_data64) {
  if (n_docs < 0 || n_terms < 0 || n_triples < 0)
    return fail(BM25_EINVAL, "negative size (n_docs=%lld n_terms=%lld n=%lld)", (long long)n_docs,
                (long long)n_terms, (long long)n_triples);
  if (n_docs > INT32_MAX || n_terms > INT32_MAX || n_triples > INT32_MAX)
    return fail(BM25_EINVAL, "sizes above int32 are built per shard");
  if (method != kLucene && method != kBm25Py) return fail(BM25_EINVAL, "unknown method %d", method);
  if (!out_indptr || (n_triples > 0 && (!docs || !terms || !tfs || !doc_len || !out_indices ||
                                         !out_data)))
    return fail(BM25_EINVAL, "NULL argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(BM25_EHIP, "no HIP device available");
  if (device < 0 || device >= ndev) return fail(BM25_EINVAL, "device %d out of range (%d visible)", device, ndev);
  HIP_TRY(hipSetDevice(device), "hipSetDevice");
  const int64_t n = n_triples;
  OwnStream own;
  HIP_TRY(hipStreamCreateWithFlags(&own.s, hipStreamNonBlocking), "hipStreamCreate");
  const hipStream_t st = own.s;
  HostCall c(st);
  int32_t* d_docs = c.alloc<int32_t>(n, "hipMalloc(docs)");
  int32_t* d_terms = c.alloc<int32_t>(n, "hipMalloc(terms)");
  float* d_tf = c.alloc<float>(n, "hipMalloc(tf)");
  int32_t* d_dl = c.alloc<int32_t>(n_docs, "hipMalloc(doc_len)");
  int32_t* d_ix = c.alloc<int32_t>(n, "hipMalloc(indices)");
  float* d_dt = c.alloc<float>(n, "hipMalloc(data)");
  int64_t* d_ip = c.alloc<int64_t>(n_terms + 1, "hipMalloc(indptr)");
  int32_t* d_err = c.alloc<int32_t>(1, "hipMalloc(err)");
  double* d_dt64 = out_data64 ? c.alloc<double>(n, "hipMalloc(data64)") : nullptr;
  float* d_idf = idf ? c.alloc<float>(n_terms, "hipMalloc(idf)") : nullptr;
  if (idf) c.upload_to(d_idf, idf, n_terms, "H2D idf");
  if (c.ok()) c.run(hipMemsetAsync(d_err, 0, sizeof(int32_t), st), "hipMemset");
  c.upload_to(d_docs, docs, n, "H2D docs");
  c.upload_to(d_terms, terms, n, "H2D terms");
  c.upload_to(d_tf, tfs, n, "H2D tf");
  if (n > 0) c.upload_to(d_dl, doc_len, n_docs, "H2D doc_len");
  if (c.ok())
    c.run(build_scores(n_docs, n_terms, n_triples, d_docs, d_terms, d_tf, d_dl, avgdl, k1, b,
                       method, d_idf, d_ip, d_ix, d_dt, d_dt64, d_err, st), "build_scores");
  int32_t herr = 0;
  c.download(&herr, d_err, 1, "D2H err");
  if (c.ok()) c.run(hipStreamSynchronize(st), "build sync");
  if (!c.ok()) herr = 0;  // (not read back)
  if (herr & 1) c.hold(fail(BM25_EINVAL, "doc or term id out of range"));
  else if (herr & 2) c.hold(fail(BM25_EINVAL, "term frequencies must be positive and finite"));
  else if (herr & 4) c.hold(fail(BM25_EINVAL, "duplicate (doc, term) triple"));
  c.download(out_indptr, d_ip, n_terms + 1, "D2H indptr");
  c.download(out_indices, d_ix, n, "D2H indices");
  c.download(out_data, d_dt, n, "D2H data");
  if (out_data64) c.download(out_data64, d_dt64, n, "D2H data64");
  return c.finish("build sync");
}

int bm25_scores_dense(bm25_index* h, const int32_t* query, int64_t T, float* out_scores) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  if (T < 0) return fail(BM25_EINVAL, "negative query length");
  if (!out_scores) return fail(BM25_EINVAL, "NULL output");
  if (T > 0 && !query) return fail(BM25_EINVAL, "NULL query");
  const int rc = check_token_ids(h->ix.n_terms, 0, query, T);
  if (rc) return rc;
  if (h->ix.n_docs == 0) return BM25_OK;
  Enter in(h);
  if (in.rc) return in.rc;
  HostCall c(h->stream);
  float* d_out = c.alloc<float>(h->ix.n_docs, "hipMalloc(dense)");
  int32_t* d_qq = c.alloc<int32_t>(T);
  c.upload_to(d_qq, query, T);
  if (c.ok()) c.run(launch_scores_dense(h->ix, d_qq, T, d_out, h->stream));
  c.download(out_scores, d_out, h->ix.n_docs);
  return c.finish("scores_dense");
}

int bm25_score_docs(bm25_index* h, const int32_t* queries, int64_t Q, int64_t T,
                    const int32_t* docs, int64_t C, float* out_scores) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  if (Q < 0 || T < 0 || C < 0) return fail(BM25_EINVAL, "negative query or candidate shape");
  if (Q == 0 || C == 0) return BM25_OK;
  if (T > 0 && !queries) return fail(BM25_EINVAL, "NULL queries");
  if (!docs) return fail(BM25_EINVAL, "NULL docs");
  if (!out_scores) return fail(BM25_EINVAL, "NULL output");
  const int rc = check_token_ids(h->ix.n_terms, 0, queries, Q * T);
  if (rc) return rc;
  const int64_t lo = h->ix.doc_offset, hi = h->ix.doc_offset + h->ix.n_docs;
  for (int64_t i = 0; i < Q * C; ++i)
    if (docs[i] >= 0 && (docs[i] < lo || docs[i] >= hi))
      return fail(BM25_EINVAL, "doc id %lld (row %lld) is outside the index's documents [%lld, %lld)",
                  (long long)docs[i], (long long)(i / C), (long long)lo, (long long)hi);
  Enter in(h);
  if (in.rc) return in.rc;
  // staging buffers of this call's own (as bm25_scores_dense): the search
  // workspace and the search staging buffers stay untouched
  HostCall c(h->stream);
  int32_t* d_qq = c.alloc<int32_t>(Q * T);
  int32_t* d_dd = c.alloc<int32_t>(Q * C);
  float* d_out = c.alloc<float>(Q * C);
  c.upload_to(d_qq, queries, Q * T);
  c.upload_to(d_dd, docs, Q * C);
  if (c.ok()) c.run(launch_score_docs(h->ix, d_qq, Q, T, d_dd, C, d_out, h->stream));
  c.download(out_scores, d_out, Q * C);
  return c.finish("score_docs");
}

int bm25_score_docs_device(bm25_index* h, const int32_t* d_queries, int64_t Q, int64_t T,
                           const int32_t* d_docs, int64_t C, float* d_scores, void* stream) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  if (Q < 0 || T < 0 || C < 0) return fail(BM25_EINVAL, "negative query or candidate shape");
  if (Q == 0 || C == 0) return BM25_OK;
  // reads the immutable index arrays only: no workspace, no ordering against
  // the handle's searches (ws_stream)
  Enter in(h);
  if (in.rc) return in.rc;
  HIP_TRY(launch_score_docs(h->ix, d_queries, Q, T, d_docs, C, d_scores, (hipStream_t)stream),
          "score_docs launch");
  return BM25_OK;
}

int bm25_score_docs_weighted(bm25_index* h, const int32_t* queries, const float* weights,
                             int64_t Q, int64_t T, const int32_t* docs, int64_t C,
                             float* out_scores) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  if (Q < 0 || T < 0 || C < 0) return fail(BM25_EINVAL, "negative query or candidate shape");
  if (Q == 0 || C == 0) return BM25_OK;
  if (T > 0 && !queries) return fail(BM25_EINVAL, "NULL queries");
  if (T > 0 && !weights) return fail(BM25_EINVAL, "NULL weights");
  if (!docs) return fail(BM25_EINVAL, "NULL docs");
  if (!out_scores) return fail(BM25_EINVAL, "NULL output");
  int rc = check_token_ids(h->ix.n_terms, 0, queries, Q * T);
  if (rc) return rc;
  rc = check_weights(queries, weights, Q, T);
  if (rc) return rc;
  const int64_t lo = h->ix.doc_offset, hi = h->ix.doc_offset + h->ix.n_docs;
  for (int64_t i = 0; i < Q * C; ++i)
    if (docs[i] >= 0 && (docs[i] < lo || docs[i] >= hi))
      return fail(BM25_EINVAL, "doc id %lld (row %lld) is outside the index's documents [%lld, %lld)",
                  (long long)docs[i], (long long)(i / C), (long long)lo, (long long)hi);
  Enter in(h);
  if (in.rc) return in.rc;
  // staging buffers of this call's own (as bm25_score_docs)
  HostCall c(h->stream);
  int32_t* d_qq = c.alloc<int32_t>(Q * T);
  float* d_ww = c.alloc<float>(Q * T);
  int32_t* d_dd = c.alloc<int32_t>(Q * C);
  float* d_out = c.alloc<float>(Q * C);
  c.upload_to(d_qq, queries, Q * T);
  c.upload_to(d_ww, weights, Q * T);
  c.upload_to(d_dd, docs, Q * C);
  if (c.ok()) c.run(launch_score_docs(h->ix, d_qq, Q, T, d_dd, C, d_out, h->stream, d_ww));
  c.download(out_scores, d_out, Q * C);
  return c.finish("score_docs_weighted");
}

int bm25_score_docs_weighted_device(bm25_index* h, const int32_t* d_queries,
                                    const float* d_weights, int64_t Q, int64_t T,
                                    const int32_t* d_docs, int64_t C, float* d_scores,
                                    void* stream) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  if (Q < 0 || T < 0 || C < 0) return fail(BM25_EINVAL, "negative query or candidate shape");
  if (Q == 0 || C == 0) return BM25_OK;
  if (T > 0 && (!d_queries || !d_weights)) return fail(BM25_EINVAL, "NULL queries or weights");
  if (!d_docs || !d_scores) return fail(BM25_EINVAL, "NULL docs or output");
  // (as bm25_score_docs_device: the index arrays only, no ordering, no wait)
  Enter in(h);
  if (in.rc) return in.rc;
  // T == 0: every score is +0.0f either way (no weight is read)
  HIP_TRY(launch_score_docs(h->ix, d_queries, Q, T, d_docs, C, d_scores, (hipStream_t)stream,
                            T > 0 ? d_weights : nullptr),
          "score_docs_weighted launch");
  return BM25_OK;
}

int bm25_index_set_values_f64(bm25_index* h, const double* data64) {
  if (!h || (h->ix.nnz > 0 && !data64)) return fail(BM25_EINVAL, "NULL argument");
  if (!h->arrays) return fail(BM25_EINVAL, "unbuilt index");
  Enter in(h);
  if (in.rc) return in.rc;
  if (!h->ix.val64) {
    HIP_TRY(hipMalloc(&h->ix.val64, sizeof(double) * std::max<int64_t>(h->ix.nnz, 1)),
            "hipMalloc(val64)");
    h->arrays->p.push_back(h->ix.val64);  // freed with the index arrays
  }
  HostCall c(h->stream);
  c.upload_to(h->ix.val64, data64, h->ix.nnz, "H2D val64");
  return c.finish("val64 sync");
}

// The f64 dense sums of one query, staged and enqueued through c (caller
// holds h->mu and has set the device): the device row, owned by c.  A bad
// query is c's held return code.
static double* dense_f64_query(bm25_index* h, HostCall& c, const int32_t* query, int64_t T) {
  if (T < 0) c.hold(fail(BM25_EINVAL, "negative query length"));
  else if (T > 0 && !query) c.hold(fail(BM25_EINVAL, "NULL query"));
  else if (!h->ix.val64)
    c.hold(fail(BM25_EINVAL, "no float64 values: bm25_index_set_values_f64 first"));
  else c.hold(check_token_ids(h->ix.n_terms, 0, query, T));
  int32_t* d_q = c.alloc<int32_t>(T, "hipMalloc(query)");
  double* d_out = c.alloc<double>(h->ix.n_docs, "hipMalloc(dense)");
  c.upload_to(d_q, query, T, "H2D query");
  if (c.ok())
    c.run(launch_dense_f64(h->ix, h->ix.val64, d_q, T, d_out, h->stream), "dense f64 launch");
  return d_out;
}

int bm25_scores_dense_f64(bm25_index* h, const int32_t* query, int64_t T, double* out_scores) {
  if (!h || !out_scores) return fail(BM25_EINVAL, "NULL argument");
  Enter in(h);
  if (in.rc) return in.rc;
  HostCall c(h->stream);
  const double* d_out = dense_f64_query(h, c, query, T);
  c.download(out_scores, d_out, h->ix.n_docs);
  return c.finish("scores_dense_f64");
}

int bm25_topn_f64(bm25_index* h, const int32_t* query, int64_t T, int64_t n, int32_t* out_docs,
                  double* out_scores) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  if (n < 0 || n > h->ix.n_docs)
    return fail(BM25_EINVAL, "n=%lld must be in 0..n_docs (%lld)", (long long)n,
                (long long)h->ix.n_docs);
  if (n > 0 && (!out_docs || !out_scores)) return fail(BM25_EINVAL, "NULL output");
  if (n == 0) return BM25_OK;
  Enter in(h);
  if (in.rc) return in.rc;
  HostCall c(h->stream);
  const double* d_out = dense_f64_query(h, c, query, T);
  void* scratch = c.alloc<char>((int64_t)topn_f64_scratch_bytes(h->ix.n_docs));
  int32_t* d_docs = c.alloc<int32_t>(n);
  double* d_sc = c.alloc<double>(n);
  if (c.ok()) c.run(launch_topn_f64(d_out, h->ix.n_docs, n, scratch, d_docs, d_sc, h->stream));
  c.download(out_docs, d_docs, n);
  c.download(out_scores, d_sc, n);
  return c.finish("topn_f64");
}

int bm25_merge_topk_device(int device, const int32_t* d_docs, const float* d_scores, int64_t W,
                           int64_t Q, int32_t k, int32_t* d_out_docs, float* d_out_scores,
                           void* stream) {
  if (W < 1 || Q < 0 || k < 0) return fail(BM25_EINVAL, "bad merge shape W=%lld Q=%lld k=%d", (long long)W, (long long)Q, k);
  HIP_TRY(hipSetDevice(device), "hipSetDevice");
  HIP_TRY(launch_merge_lists(d_docs, d_scores, W, Q, k, Q * (int64_t)k, false, d_out_docs, d_out_scores, (hipStream_t)stream), "merge_lists launch");
  return BM25_OK;
}

int bm25_merge_sorted_device(int device, const int32_t* d_docs, const float* d_scores, int64_t W,
                             int64_t Q, int32_t k, int64_t rank_stride, int32_t* d_out_docs,
                             float* d_out_scores, void* stream) {
  if (W < 1 || Q < 0 || k < 0 || rank_stride < Q * (int64_t)k)
    return fail(BM25_EINVAL, "bad merge shape W=%lld Q=%lld k=%d stride=%lld", (long long)W,
                (long long)Q, k, (long long)rank_stride);
  HIP_TRY(hipSetDevice(device), "hipSetDevice");
  HIP_TRY(launch_merge_lists(d_docs, d_scores, W, Q, k, rank_stride, true, d_out_docs,
                             d_out_scores, (hipStream_t)stream),
          "merge_sorted launch");
  return BM25_OK;
}

// Every check precedes hipSetDevice: a bad call touches no device.
int bm25_merge_collapsed_device(int device, const int32_t* d_docs, const float* d_scores,
                                const int32_t* d_groups, int64_t W, int64_t Q, int32_t k,
                                int64_t rank_stride, int32_t per_group, int32_t* d_out_docs,
                                float* d_out_scores, int32_t* d_out_groups, void* stream) {
  if (W < 1 || W > 64)
    return fail(BM25_EINVAL, "merge_collapsed: W=%lld must be in 1..64 (W > 64: merge in stages)",
                (long long)W);
  if (Q < 0) return fail(BM25_EINVAL, "merge_collapsed: Q=%lld must be >= 0", (long long)Q);
  if (k < 0) return fail(BM25_EINVAL, "merge_collapsed: k=%d must be >= 0", k);
  if (k > kMaxK)
    return fail(BM25_EINVAL,
                "merge_collapsed: k=%d: collapse is limited to k <= %d (the group table lives in LDS)",
                k, kMaxK);
  if (per_group < 1)
    return fail(BM25_EINVAL, "merge_collapsed: per_group=%d must be >= 1", per_group);
  if (Q > 0x7FFFFFFF)
    return fail(BM25_EINVAL, "merge_collapsed: Q=%lld must be < 2^31", (long long)Q);
  if (rank_stride < Q * (int64_t)k)
    return fail(BM25_EINVAL, "merge_collapsed: rank_stride=%lld must be >= Q * k (%lld)",
                (long long)rank_stride, (long long)(Q * (int64_t)k));
  if (Q == 0 || k == 0) return BM25_OK;
  if (!d_docs || !d_scores || !d_groups) return fail(BM25_EINVAL, "merge_collapsed: NULL input");
  if (!d_out_docs || !d_out_scores) return fail(BM25_EINVAL, "merge_collapsed: NULL output");
  HIP_TRY(hipSetDevice(device), "hipSetDevice");
  HIP_TRY(launch_merge_collapsed(d_docs, d_scores, d_groups, W, Q, k, rank_stride, per_group,
                                 d_out_docs, d_out_scores, d_out_groups, (hipStream_t)stream),
          "merge_collapsed launch");
  return BM25_OK;
}

// Sort-by-field search over doc shards.  Every check precedes the first device
// call (Enter's hipSetDevice included): a bad call touches no device.
int bm25_sort_keys_device(bm25_index* h, const void* d_values, int32_t kind, int32_t descending,
                          const int32_t* d_docs, int64_t n, uint32_t* d_key_hi,
                          uint32_t* d_key_lo, void* stream) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  const int rc = check_kind(kind);
  if (rc) return rc;
  if (n < 0) return fail(BM25_EINVAL, "sort_keys: n=%lld must be >= 0", (long long)n);
  if (n == 0) return BM25_OK;
  if (!d_docs) return fail(BM25_EINVAL, "sort_keys: NULL docs");
  if (!d_key_hi || !d_key_lo) return fail(BM25_EINVAL, "sort_keys: NULL output");
  if (h->ix.n_docs > 0 && !d_values) return fail(BM25_EINVAL, "sort_keys: NULL values");
  // reads the caller's buffers only (as bm25_search_sorted_device: no workspace,
  // no index array, no ordering against the handle's searches)
  Enter in(h);
  if (in.rc) return in.rc;
  HIP_TRY(launch_sort_keys(h->ix, d_values, kind, descending != 0, d_docs, n, d_key_hi, d_key_lo,
                           (hipStream_t)stream),
          "sort_keys launch");
  return BM25_OK;
}

int bm25_sort_cursor_device(bm25_index* h, const void* d_values, int32_t kind, int32_t descending,
                            const int32_t* d_perm, const uint32_t* d_after_key_hi,
                            const uint32_t* d_after_key_lo, const int32_t* d_after_docs, int64_t M,
                            int32_t* d_after_ranks, void* stream) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  const int rc = check_kind(kind);
  if (rc) return rc;
  if (M < 0) return fail(BM25_EINVAL, "sort_cursor: M=%lld must be >= 0", (long long)M);
  if (M == 0) return BM25_OK;
  if (!d_after_key_hi || !d_after_key_lo || !d_after_docs)
    return fail(BM25_EINVAL, "sort_cursor: NULL cursor");
  if (!d_after_ranks) return fail(BM25_EINVAL, "sort_cursor: NULL output");
  if (h->ix.n_docs > 0 && (!d_values || !d_perm))
    return fail(BM25_EINVAL, "sort_cursor: NULL values or perm");
  Enter in(h);  // (as bm25_sort_keys_device: the caller's buffers only)
  if (in.rc) return in.rc;
  HIP_TRY(launch_sort_cursor(h->ix, d_values, kind, descending != 0, d_perm, d_after_key_hi,
                             d_after_key_lo, d_after_docs, M, d_after_ranks, (hipStream_t)stream),
          "sort_cursor launch");
  return BM25_OK;
}

int bm25_merge_sort_keys_device(int device, const int32_t* d_docs, const uint32_t* d_key_hi,
                                const uint32_t* d_key_lo, int64_t W, int64_t Q, int32_t k,
                                int64_t rank_stride, int32_t* d_out_docs, uint32_t* d_out_key_hi,
                                uint32_t* d_out_key_lo, void* stream) {
  if (W < 1 || W > 64)
    return fail(BM25_EINVAL, "merge_sort_keys: W=%lld must be in 1..64 (W > 64: merge in stages)",
                (long long)W);
  if (Q < 0) return fail(BM25_EINVAL, "merge_sort_keys: Q=%lld must be >= 0", (long long)Q);
  if (k < 0) return fail(BM25_EINVAL, "merge_sort_keys: k=%d must be >= 0", k);
  if (k > kMaxK)
    return fail(BM25_EINVAL,
                "merge_sort_keys: k=%d: a sorted search returns at most %d (the row is merged in LDS)",
                k, kMaxK);
  if (Q > 0x7FFFFFFF)
    return fail(BM25_EINVAL, "merge_sort_keys: Q=%lld must be < 2^31", (long long)Q);
  if (rank_stride < Q * (int64_t)k)
    return fail(BM25_EINVAL, "merge_sort_keys: rank_stride=%lld must be >= Q * k (%lld)",
                (long long)rank_stride, (long long)(Q * (int64_t)k));
  if (Q == 0 || k == 0) return BM25_OK;
  if (!d_docs || !d_key_hi || !d_key_lo) return fail(BM25_EINVAL, "merge_sort_keys: NULL input");
  if (!d_out_docs || !d_out_key_hi || !d_out_key_lo)
    return fail(BM25_EINVAL, "merge_sort_keys: NULL output");
  HIP_TRY(hipSetDevice(device), "hipSetDevice");
  HIP_TRY(launch_merge_sort_keys(d_docs, d_key_hi, d_key_lo, W, Q, k, rank_stride, d_out_docs,
                                 d_out_key_hi, d_out_key_lo, (hipStream_t)stream),
          "merge_sort_keys launch");
  return BM25_OK;
}

int bm25_profile_enable(bm25_index* h, int on) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  std::lock_guard<std::mutex> lk(h->mu);
  hipSetDevice(h->ix.device);
  harvest_events(h);
  h->prof = on < 0 ? 0 : (on > 2 ? 2 : on);
  h->score_ms = h->total_ms = 0.0;
  h->score_launches = h->searches = h->rescored = 0;
  return BM25_OK;
}

int bm25_profile_read(bm25_index* h, double* score_ms_total, int64_t* score_launches,
                      double* total_ms, int64_t* searches, int64_t* rescored_tiles) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  std::lock_guard<std::mutex> lk(h->mu);
  hipSetDevice(h->ix.device);
  harvest_events(h);
  int32_t cnt[kCounters] = {};
  read_counters(h, cnt);
  if (score_ms_total) *score_ms_total = h->score_ms;
  if (score_launches) *score_launches = h->score_launches;
  if (total_ms) *total_ms = h->total_ms;
  if (searches) *searches = h->searches;
  if (rescored_tiles) *rescored_tiles = cnt[3];  // tiles re-scored by the last search
  return BM25_OK;
}

int bm25_search_stats(bm25_index* h, int64_t* rescored_tiles, int64_t* fallback_queries) {
  return bm25_search_stats_ex(h, rescored_tiles, fallback_queries, nullptr);
}

int bm25_search_stats_ex(bm25_index* h, int64_t* rescored_tiles, int64_t* fallback_queries,
                         int64_t* bound_skipped) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  Enter in(h);
  if (in.rc) return in.rc;
  int32_t cnt[kCounters] = {};
  read_counters(h, cnt);
  if (rescored_tiles) *rescored_tiles = cnt[3];
  if (fallback_queries) *fallback_queries = cnt[2];
  if (bound_skipped) *bound_skipped = (h->ix.disp.kernels & kKCountSkips) ? cnt[5] : -1;
  return BM25_OK;
}

int bm25_search_counters(bm25_index* h, int64_t* out, int32_t n) {
  if (!h || !out) return fail(BM25_EINVAL, "NULL argument");
  if (n < 1 || n > 10) return fail(BM25_EINVAL, "n=%d must be in 1..10", n);
  Enter in(h);
  if (in.rc) return in.rc;
  int32_t cnt[kCounters] = {};
  read_counters(h, cnt);
  uint64_t post = 0;
  std::memcpy(&post, cnt + 6, sizeof post);  // counters[6..7]: a u64 (score_flat_kernel)
  // (the skipped pairs and postings: counted by the count_skips build only, else -1)
  const bool counted = (h->ix.disp.kernels & kKCountSkips) != 0;
  uint64_t dpost = 0;
  std::memcpy(&dpost, cnt + 10, sizeof dpost);  // counters[10..11]: the dropped segments' postings
  uint64_t rpost = 0;
  std::memcpy(&rpost, cnt + 12, sizeof rpost);  // counters[12..13]: the dropped rows' postings
  const int64_t v[10] = {cnt[3], cnt[2], counted ? cnt[5] : -1, counted ? (int64_t)post : -1,
                         cnt[4], h->large_fallback, counted ? cnt[8] : -1,
                         counted ? (int64_t)dpost : -1, counted ? cnt[9] : -1,
                         counted ? (int64_t)rpost : -1};
  for (int i = 0; i < n; ++i) out[i] = v[i];
  return BM25_OK;
}

int bm25_index_set_option(bm25_index* h, const char* name, int64_t value) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  std::lock_guard<std::mutex> lk(h->mu);
  const int old_cap = h->ix.opt.list_cap;
  const int rc = set_opt(h->ix.opt, name, value);
  if (rc) return rc;
  if (h->ix.opt.list_cap != old_cap && h->ws.cap_q > 0) {  // the list capacity is sized in
    hipSetDevice(h->ix.device);                            // the workspace: rebuild it
    ws_wait_host(h);
    free_ws(h->ws);
  }
  return BM25_OK;
}

int bm25_index_get_option(const bm25_index* h, const char* name, int64_t* value) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  bm25_index* m = const_cast<bm25_index*>(h);  // the mutex only: set_option writes under it
  std::lock_guard<std::mutex> lk(m->mu);
  return get_opt(h->ix.opt, name, value);
}

int bm25_search_dispatch(bm25_index* h, uint32_t* kernels, int32_t* term_lanes,
                         int32_t* band_tiles, int32_t* sample_p) {
  if (!h) return fail(BM25_EINVAL, "NULL index");
  std::lock_guard<std::mutex> lk(h->mu);
  const Dispatch& d = h->ix.disp;
  if (kernels) *kernels = d.kernels;
  if (term_lanes) *term_lanes = d.term_lanes;
  if (band_tiles)
    for (int i = 0; i < 3; ++i) band_tiles[i] = d.band_tiles[i];
  if (sample_p) *sample_p = d.sample_p;
  return BM25_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Doc-sharded index over several devices of one process:
// shard s owns the tile-aligned doc range [lo_s, hi_s) as an ordinary index
// (doc_offset = lo_s) on devices[s].  A search is the global-threshold
// protocol of the multi-process path (bm25mi.dist.sharded_search) with peer
// copies over xGMI in place of the collectives:
//   1. every shard samples on its own stream -> keys_s [Q][S];
//   2. every shard's keys are copied into every shard's all_keys [W][Q][S]
//      (peer copies on the destination's stream, after the source's event);
//   3. every shard: theta = the k-th best key of the whole sample, then its
//      keys >= theta as a padded [Q, k] list (global doc ids);
//   4. the lists are copied to shard 0's device and merged there with the
//      same (score desc, doc asc) rule, so the result equals a single-index
//      search.
// One process owns every device here, so no RCCL communicator is involved
// (the multi-process path runs its all-gathers over RCCL).
// ---------------------------------------------------------------------------
struct bm25_sharded {
  std::vector<bm25_index*> shards;
  std::vector<int64_t> lo, hi;
  std::vector<hipEvent_t> sampled;  // per shard: its sample keys are written
  std::vector<hipEvent_t> keyed;    // per shard: its all_keys copies landed
  std::vector<hipEvent_t> done;     // per shard: its [Q, k] list is written
  std::vector<uint64_t*> keys;      // per shard (own device): [Q][S]
  std::vector<uint64_t*> all_keys;  // per shard (own device): [W][Q][S]
  int64_t cap_keys = 0;
  int64_t n_docs = 0, n_terms = 0, shard_docs_max = 0;
  int32_t* g_docs = nullptr;     // [W][Q][k] on shard 0's device
  float* g_scores = nullptr;
  int32_t* m_docs = nullptr;     // [Q][k]
  float* m_scores = nullptr;
  int64_t cap_g = 0, cap_m = 0;
  std::mutex mu;
};

namespace {

int sharded_free(bm25_sharded* s) {
  if (!s) return BM25_OK;
  if (!s->shards.empty() && s->shards[0]) {
    hipSetDevice(s->shards[0]->ix.device);
    hipFree(s->g_docs);
    hipFree(s->g_scores);
    hipFree(s->m_docs);
    hipFree(s->m_scores);
  }
  for (size_t i = 0; i < s->shards.size(); ++i) {
    if (!s->shards[i]) continue;
    hipSetDevice(s->shards[i]->ix.device);
    hipStreamSynchronize(s->shards[i]->stream);
    for (auto* v : {&s->sampled, &s->keyed, &s->done})
      if (i < v->size() && (*v)[i]) hipEventDestroy((*v)[i]);
    if (i < s->keys.size()) hipFree(s->keys[i]);
    if (i < s->all_keys.size()) hipFree(s->all_keys[i]);
    bm25_index_destroy(s->shards[i]);
  }
  delete s;
  return BM25_OK;
}

// Waits for every shard's stream when a sharded search fails part-way (s =
// nullptr: it ended, drained).
struct DrainShards {
  bm25_sharded* s;
  ~DrainShards() {
    for (size_t r = 0; s && r < s->shards.size(); ++r) {
      hipSetDevice(s->shards[r]->ix.device);
      hipStreamSynchronize(s->shards[r]->stream);
    }
  }
};

}  // namespace

extern "C" {

int bm25_sharded_create(int n_dev, const int* devices, int64_t n_docs, int64_t n_terms,
                        int64_t nnz, const void* indptr, int indptr_is_i64,
                        const int32_t* indices, const float* data, bm25_sharded** out) {
  if (!out) return fail(BM25_EINVAL, "out is NULL");
  *out = nullptr;
  if (n_dev < 1 || !devices) return fail(BM25_EINVAL, "need at least one device");
  if (n_docs < 0 || n_terms < 0 || nnz < 0) return fail(BM25_EINVAL, "negative size");
  if (!indptr || (nnz > 0 && (!indices || !data))) return fail(BM25_EINVAL, "NULL CSC array");
  std::vector<int64_t> ip(n_terms + 1);
  for (int64_t t = 0; t <= n_terms; ++t)
    ip[t] = indptr_is_i64 ? ((const int64_t*)indptr)[t] : (int64_t)((const int32_t*)indptr)[t];
  if (ip[0] != 0 || ip[n_terms] != nnz)
    return fail(BM25_EINVAL, "indptr must start at 0 and end at nnz");
  for (int64_t t = 0; t < n_terms; ++t)
    if (ip[t + 1] < ip[t]) return fail(BM25_EINVAL, "indptr decreases at column %lld", (long long)t);
  bm25_sharded* s = new bm25_sharded();
  s->n_docs = n_docs;
  s->n_terms = n_terms;
  const int64_t align = 2048;
  auto bound = [&](int64_t r) -> int64_t {
    if (r >= n_dev) return n_docs;
    const int64_t x = n_docs * r / n_dev;
    return std::min(n_docs, (x + align / 2) / align * align);
  };
  std::vector<int64_t> sip(n_terms + 1);
  std::vector<int32_t> six;
  std::vector<float> sdt;
  for (int r = 0; r < n_dev; ++r) {
    const int64_t lo = bound(r), hi = bound(r + 1);
    // the shard's CSC: per column, the entries with lo <= doc < hi (columns are
    // sorted; unsorted input is rejected by the shard's own build check)
    sip[0] = 0;
    for (int64_t t = 0; t < n_terms; ++t) {
      const int32_t* b = indices + ip[t];
      const int32_t* e = indices + ip[t + 1];
      const int32_t* p0 = std::lower_bound(b, e, (int32_t)std::min<int64_t>(lo, INT32_MAX));
      const int32_t* p1 = std::lower_bound(p0, e, (int32_t)std::min<int64_t>(hi, INT32_MAX));
      sip[t + 1] = sip[t] + (p1 - p0);
    }
    six.resize(std::max<int64_t>(sip[n_terms], 1));
    sdt.resize(std::max<int64_t>(sip[n_terms], 1));
    for (int64_t t = 0; t < n_terms; ++t) {
      const int32_t* b = indices + ip[t];
      const int32_t* e = indices + ip[t + 1];
      const int32_t* p0 = std::lower_bound(b, e, (int32_t)std::min<int64_t>(lo, INT32_MAX));
      for (int64_t i = 0; i < sip[t + 1] - sip[t]; ++i) {
        six[sip[t] + i] = p0[i] - (int32_t)lo;
        sdt[sip[t] + i] = data[(p0 - indices) + i];
      }
    }
    bm25_index* h = nullptr;
    const int rc = bm25_index_create(devices[r], hi - lo, n_terms, sip[n_terms], sip.data(), 1,
                                     six.data(), sdt.data(), lo, &h);
    if (rc) {
      const std::string msg = g_err;
      sharded_free(s);
      return fail(rc, "shard %d (device %d): %s", r, devices[r], msg.c_str());
    }
    s->shards.push_back(h);
    s->lo.push_back(lo);
    s->hi.push_back(hi);
    s->keys.push_back(nullptr);
    s->all_keys.push_back(nullptr);
    s->shard_docs_max = std::max(s->shard_docs_max, hi - lo);
    hipSetDevice(devices[r]);
    for (auto* v : {&s->sampled, &s->keyed, &s->done}) {
      hipEvent_t ev = nullptr;
      if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
        sharded_free(s);
        return fail(BM25_EHIP, "hipEventCreate");
      }
      v->push_back(ev);
    }
  }
  *out = s;
  return BM25_OK;
}

int bm25_sharded_destroy(bm25_sharded* s) { return sharded_free(s); }

int bm25_sharded_search(bm25_sharded* s, const int32_t* queries, int64_t Q, int64_t T,
                        int32_t k, int32_t* out_docs, float* out_scores) {
  if (!s) return fail(BM25_EINVAL, "NULL index");
  if (Q < 0 || T < 0) return fail(BM25_EINVAL, "negative query shape");
  if (k < 0) return fail(BM25_EINVAL, "negative dimensions are not allowed (top_k=%d)", k);
  if (k > s->n_docs)
    return fail(BM25_EINVAL, "kth(=%lld) out of bounds (%lld)", (long long)(s->n_docs - k),
                (long long)s->n_docs);
  if (Q == 0 || k == 0) return BM25_OK;
  if (T > 0 && !queries) return fail(BM25_EINVAL, "NULL queries");
  if (!out_docs || !out_scores) return fail(BM25_EINVAL, "NULL output");
  int rc = check_token_ids(s->n_terms, 0, queries, Q * T);
  if (rc) return rc;
  const int64_t W = (int64_t)s->shards.size();
  std::lock_guard<std::mutex> lk(s->mu);
  bm25_index* h0 = s->shards[0];
  const int64_t out = Q * (int64_t)k;
  HIP_TRY(hipSetDevice(h0->ix.device), "hipSetDevice");
  if (W * out > s->cap_g) {
    hipFree(s->g_docs);
    hipFree(s->g_scores);
    s->g_docs = nullptr;
    s->g_scores = nullptr;
    s->cap_g = 0;
    HIP_TRY(hipMalloc(&s->g_docs, sizeof(int32_t) * W * out), "hipMalloc(shard lists)");
    HIP_TRY(hipMalloc(&s->g_scores, sizeof(float) * W * out), "hipMalloc(shard lists)");
    s->cap_g = W * out;
  }
  if (out > s->cap_m) {
    hipFree(s->m_docs);
    hipFree(s->m_scores);
    s->m_docs = nullptr;
    s->m_scores = nullptr;
    s->cap_m = 0;
    HIP_TRY(hipMalloc(&s->m_docs, sizeof(int32_t) * out), "hipMalloc(merged)");
    HIP_TRY(hipMalloc(&s->m_scores, sizeof(float) * out), "hipMalloc(merged)");
    s->cap_m = out;
  }
  // sample width: the same on every shard (bm25_sample_width's rule)
  int64_t S = 0;
  rc = bm25_sample_width(h0, s->shard_docs_max, (int32_t)W, k, &S);
  if (rc) return rc;
  if (Q * S > s->cap_keys) {
    s->cap_keys = 0;
    for (int64_t r = 0; r < W; ++r) {
      HIP_TRY(hipSetDevice(s->shards[r]->ix.device), "hipSetDevice");
      hipStreamSynchronize(s->shards[r]->stream);
      hipFree(s->keys[r]);
      hipFree(s->all_keys[r]);
      s->keys[r] = s->all_keys[r] = nullptr;
      HIP_TRY(hipMalloc(&s->keys[r], sizeof(uint64_t) * Q * S), "hipMalloc(sample keys)");
      HIP_TRY(hipMalloc(&s->all_keys[r], sizeof(uint64_t) * W * Q * S), "hipMalloc(all keys)");
    }
    s->cap_keys = Q * S;
  }
  // from here on the shards' streams read and write the caller's arrays:
  // no return before they have drained
  DrainShards drain{s};
  // 1. every shard: H2D queries + its sample keys, on its own stream
  for (int64_t r = 0; r < W; ++r) {
    bm25_index* h = s->shards[r];
    HIP_TRY(hipSetDevice(h->ix.device), "hipSetDevice");
    {
      std::lock_guard<std::mutex> lh(h->mu);
      rc = ensure_io(h, Q * T, out);
      if (rc) return rc;
      if (Q * T > 0)
        HIP_TRY(hipMemcpyAsync(h->d_q, queries, sizeof(int32_t) * Q * T, hipMemcpyHostToDevice,
                               h->stream), "H2D queries");
    }
    if (S > 0) {
      rc = bm25_search_sample_device(h, h->d_q, Q, T, k, (int32_t)W, s->shard_docs_max,
                                     s->keys[r], h->stream);
      if (rc) return rc;
    }
    HIP_TRY(hipEventRecord(s->sampled[r], h->stream), "hipEventRecord");
  }
  // 2. every shard's keys into every shard's all_keys (destination stream)
  if (S > 0) {
    for (int64_t d = 0; d < W; ++d) {
      bm25_index* hd = s->shards[d];
      HIP_TRY(hipSetDevice(hd->ix.device), "hipSetDevice");
      for (int64_t r = 0; r < W; ++r) {
        bm25_index* hr = s->shards[r];
        HIP_TRY(hipStreamWaitEvent(hd->stream, s->sampled[r], 0), "hipStreamWaitEvent");
        HIP_TRY(hipMemcpyPeerAsync(s->all_keys[d] + r * Q * S, hd->ix.device, s->keys[r],
                                   hr->ix.device, sizeof(uint64_t) * Q * S, hd->stream),
                "peer copy (sample keys)");
      }
      HIP_TRY(hipEventRecord(s->keyed[d], hd->stream), "hipEventRecord");
    }
  }
  // 3. every shard: global theta, REST, its padded [Q, k] list (a shard's
  // keys buffer is rewritten only by the next search, and this one waits for
  // every keyed[*] event before it returns)
  for (int64_t r = 0; r < W; ++r) {
    bm25_index* h = s->shards[r];
    HIP_TRY(hipSetDevice(h->ix.device), "hipSetDevice");
    rc = bm25_search_finish_device(h, h->d_q, Q, T, k, (int32_t)W, s->shard_docs_max,
                                   S > 0 ? s->all_keys[r] : nullptr, h->d_docs, h->d_scores,
                                   h->stream);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(s->done[r], h->stream), "hipEventRecord");
  }
  // gather on shard 0's stream (peer copies after each shard's event), merge, D2H
  HIP_TRY(hipSetDevice(h0->ix.device), "hipSetDevice");
  for (int64_t r = 0; r < W; ++r) {
    bm25_index* h = s->shards[r];
    HIP_TRY(hipStreamWaitEvent(h0->stream, s->done[r], 0), "hipStreamWaitEvent");
    HIP_TRY(hipMemcpyPeerAsync(s->g_docs + r * out, h0->ix.device, h->d_docs, h->ix.device,
                               sizeof(int32_t) * out, h0->stream), "peer copy");
    HIP_TRY(hipMemcpyPeerAsync(s->g_scores + r * out, h0->ix.device, h->d_scores, h->ix.device,
                               sizeof(float) * out, h0->stream), "peer copy");
  }
  HIP_TRY(launch_merge_lists(s->g_docs, s->g_scores, W, Q, k, Q * (int64_t)k, true, s->m_docs, s->m_scores, h0->stream),
          "merge_lists launch");
  HIP_TRY(hipMemcpyAsync(out_docs, s->m_docs, sizeof(int32_t) * out, hipMemcpyDeviceToHost,
                         h0->stream), "D2H docs");
  HIP_TRY(hipMemcpyAsync(out_scores, s->m_scores, sizeof(float) * out, hipMemcpyDeviceToHost,
                         h0->stream), "D2H scores");
  HIP_TRY(hipStreamSynchronize(h0->stream), "sharded search sync");
  // every shard's stream has drained its copies of the others' keys
  for (int64_t r = 0; r < W; ++r) {
    HIP_TRY(hipSetDevice(s->shards[r]->ix.device), "hipSetDevice");
    HIP_TRY(hipEventSynchronize(s->keyed[r]), "hipEventSynchronize");
  }
  drain.s = nullptr;  // (they have)
  return BM25_OK;
}

int bm25_sharded_info(const bm25_sharded* s, int64_t* n_shards, int64_t* shard_lo,
                      int64_t* shard_hi) {
  if (!s) return fail(BM25_EINVAL, "NULL index");
  if (n_shards) *n_shards = (int64_t)s->shards.size();
  for (size_t i = 0; i < s->shards.size(); ++i) {
    if (shard_lo) shard_lo[i] = s->lo[i];
    if (shard_hi) shard_hi[i] = s->hi[i];
  }
  return BM25_OK;
}

}  // extern "C"
