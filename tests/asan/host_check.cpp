// Host-side check of libbm25mi's C-ABI under AddressSanitizer (SURVEY.md:235;
// VERDICT r4 item 8).  Built by tests/test_host.py::test_capi_host_asan with
// every source compiled for the host only (--cuda-host-only) and
// -fsanitize=address, and run where no GPU is visible: the argument checks,
// error messages and early-exit paths of the boundary that need no handle run
// (the ranked searches' rules sit behind one: tests/asan/ranked_check.cpp
// drives those), the device calls fail with EHIP, and ASan reports any
// out-of-bounds or use-after-free on the way (the process exits non-zero).
// The boundary's two internal pieces
// (csrc/bm25mi_host.h) are driven directly: the HostCall staging helper with
// every HIP call failing, and the option table behind set_option / get_option.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <fstream>
#include <iterator>
#include <unistd.h>

#include "../../include/bm25mi.h"
#include "../../mojo-bm25_amd/csrc/bm25mi_host.h"

static int failures = 0;

static void expect(int rc, int want, const char* what, const char* msg_part = nullptr) {
  const std::string msg = bm25_last_error();
  const bool ok = rc == want && (!msg_part || msg.find(msg_part) != std::string::npos);
  if (!ok) {
    std::printf("FAIL %s: rc=%d want=%d msg='%s'\n", what, rc, want, msg.c_str());
    ++failures;
  }
}

static void expect_true(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAIL %s\n", what);
    ++failures;
  }
}

// The exact message of the last failure.
static void expect_msg(int rc, int want, const char* what, const std::string& msg) {
  expect(rc, want, what);
  if (msg != bm25_last_error()) {
    std::printf("FAIL %s: msg='%s' want='%s'\n", what, bm25_last_error(), msg.c_str());
    ++failures;
  }
}

// HostCall where every HIP call fails (no device visible): the first failure
// is held, later steps make no HIP call and return null, finish reports it
// under its label, a held return code wins, and the destructors run clean.
static void check_host_call_no_device() {
  using bm25mi::HostCall;
  const int32_t src[3] = {1, 2, 3};
  int32_t dst[3] = {7, 7, 7};
  {
    HostCall c(nullptr);
    int32_t* d = c.upload(src, 3);
    expect_true(d == nullptr && !c.ok(), "HostCall upload fails without a device");
    float* a = c.alloc<float>(5);
    expect_true(a == nullptr, "HostCall alloc after a failure is null");
    expect_true(c.upload(src, 3) == nullptr, "HostCall upload after a failure is null");
    expect_true(c.upload(src, 0) == nullptr, "HostCall upload of nothing is null");
    c.download(dst, d, 3);
    c.run(hipSuccess);
    expect(c.finish("probe"), BM25_EHIP, "HostCall finish", "probe: ");
    expect_true(std::string(bm25_last_error()).rfind("probe: ", 0) == 0, "HostCall message start");
    expect_true(dst[0] == 7 && dst[2] == 7, "HostCall download after a failure copies nothing");
  }
  {  // a step's own label, kept in place of finish's
    HostCall c(nullptr);
    c.alloc<int32_t>(4, "hipMalloc(first)");
    c.alloc<int32_t>(4, "hipMalloc(second)");
    expect(c.finish("probe"), BM25_EHIP, "HostCall label", "hipMalloc(first): ");
  }
  {  // a pipeline's return code wins over the HIP error
    HostCall c(nullptr);
    c.alloc<int32_t>(4);
    c.hold(bm25mi::fail(BM25_EINVAL, "held"));
    c.hold(BM25_ENOMEM);
    expect_msg(c.finish("probe"), BM25_EINVAL, "HostCall held code", "held");
  }
  {  // never finished: the destructor alone
    HostCall c(nullptr);
    c.alloc<double>(2);
  }
}

// BM25_* names in the environment paragraph of include/bm25mi.h (the file
// lies three directories above this program, or two above this source).
static int header_env_names() {
  std::string text;
  char exe[4096];
  const ssize_t n = readlink("/proc/self/exe", exe, sizeof exe - 1);
  std::vector<std::string> paths;
  if (n > 0) {
    std::string p(exe, (size_t)n);
    for (int up = 0; up < 4 && p.rfind('/') != std::string::npos; ++up) p.erase(p.rfind('/'));
    paths.push_back(p + "/include/bm25mi.h");
  }
  std::string src = __FILE__;
  for (int up = 0; up < 3 && src.rfind('/') != std::string::npos; ++up) src.erase(src.rfind('/'));
  paths.push_back(src + "/include/bm25mi.h");
  for (const std::string& p : paths) {
    std::ifstream f(p);
    if (!f) continue;
    text.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    break;
  }
  const size_t a = text.find("environment (BM25_");
  const size_t b = a == std::string::npos ? a : text.find(')', a);
  if (b == std::string::npos) return -1;
  int names = 0;
  for (size_t p = text.find("BM25_", a); p != std::string::npos && p < b; p = text.find("BM25_", p + 1))
    ++names;
  return names;
}

// The option table on a default SearchOpts: every name reads its default,
// takes an accepted value and reads it back, and rejects a value outside
// with the message bm25_index_set_option always gave.
static void check_option_table() {
  using bm25mi::SearchOpts;
  struct Case {
    const char* name;
    int SearchOpts::*field;
    int64_t good, bad;
    const char* msg;
  };
  const Case cases[] = {
      {"flat", &SearchOpts::flat, 0, 2, "flat must be 0 or 1"},
      {"flat_bw", &SearchOpts::flat_bw, 8, 3, "flat_bw must be 0, 1, 2, 4 or 8"},
      {"items_per_wave", &SearchOpts::items_per_wave, 1024, 0, "items_per_wave must be in 1..1024"},
      {"sample_p", &SearchOpts::sample_p, 64, 0, "sample_p must be a power of two in 1..64"},
      {"list_cap", &SearchOpts::list_cap, 1 << 20, (1 << 20) + 1, "list_cap must be in 0..2^20"},
      {"claim_ch", &SearchOpts::claim_ch, 64, 65, "claim_ch must be in 1..64"},
      {"claim_m", &SearchOpts::claim_m, 8, 9, "claim_m must be in 1..8"},
      {"tile_bound", &SearchOpts::tile_bound, 0, -1, "tile_bound must be 0 or 1"},
      {"theta_bound", &SearchOpts::theta_bound, 0, 2, "theta_bound must be 0 or 1"},
      {"large_lists", &SearchOpts::large_lists, 0, 2, "large_lists must be 0 or 1"},
      {"rest_split", &SearchOpts::rest_split, 1, 2, "rest_split must be 0 or 1"},
      {"bound_pool", &SearchOpts::bound_pool, 0, 2, "bound_pool must be 0 or 1"},
      {"filter_tiles", &SearchOpts::filter_tiles, 0, 2, "filter_tiles must be 0 or 1"},
      {"bool_chunk", &SearchOpts::bool_chunk, 1 << 30, (1ll << 30) + 1,
       "bool_chunk must be in 0..2^30"},
      {"count_skips", &SearchOpts::count_skips, 1, 2, "count_skips must be 0 or 1"},
      {"grid_pct", &SearchOpts::grid_pct, 1, 101, "grid_pct must be in 1..100"},
  };
  const SearchOpts dflt;
  int n_cases = 0;
  for (const Case& t : cases) {
    ++n_cases;
    SearchOpts o;
    int64_t v = -99;
    expect(bm25mi::get_opt(o, t.name, &v), BM25_OK, t.name);
    expect_true(v == dflt.*t.field, t.name);
    expect_msg(bm25mi::set_opt(o, t.name, t.bad), BM25_EINVAL, t.name, t.msg);
    expect_true(o.*t.field == dflt.*t.field, t.name);  // a rejected value changes nothing
    expect(bm25mi::set_opt(o, t.name, t.good), BM25_OK, t.name);
    expect(bm25mi::get_opt(o, t.name, &v), BM25_OK, t.name);
    expect_true(v == t.good && o.*t.field == t.good, t.name);
  }
  // further edges of the two shapes that are no plain range
  SearchOpts o;
  int64_t v = 0;
  for (int64_t bw : {0, 1, 2, 4, 8}) expect(bm25mi::set_opt(o, "flat_bw", bw), BM25_OK, "flat_bw");
  for (int64_t bw : {-1, 5, 6, 16})
    expect_msg(bm25mi::set_opt(o, "flat_bw", bw), BM25_EINVAL, "flat_bw", "flat_bw must be 0, 1, 2, 4 or 8");
  for (int64_t p : {-8, 3, 128})
    expect_msg(bm25mi::set_opt(o, "sample_p", p), BM25_EINVAL, "sample_p",
               "sample_p must be a power of two in 1..64");
  expect_msg(bm25mi::set_opt(o, "x", 1), BM25_EINVAL, "unknown set", "unknown option 'x'");
  expect_msg(bm25mi::get_opt(o, "x", &v), BM25_EINVAL, "unknown get", "unknown option 'x'");
  expect_msg(bm25mi::set_opt(o, nullptr, 1), BM25_EINVAL, "NULL name", "NULL option name");
  expect_msg(bm25mi::get_opt(o, "flat", nullptr), BM25_EINVAL, "NULL value", "NULL argument");
  const int n_table = (int)(sizeof bm25mi::kOpts / sizeof bm25mi::kOpts[0]);
  expect_true(n_cases == 16 && n_table == 16, "16 options");
  const int n_header = header_env_names();
  if (n_header != n_table) {
    std::printf("FAIL include/bm25mi.h names %d BM25_* variables, the table %d\n", n_header, n_table);
    ++failures;
  }
}

int main() {
  if (bm25_abi_version() != BM25MI_ABI_VERSION) ++failures;
  const int ndev = bm25_device_count();
  // a small valid CSC: 3 terms over 5 documents
  std::vector<int64_t> ip = {0, 2, 2, 5};
  std::vector<int32_t> ix = {0, 3, 1, 2, 4};
  std::vector<float> dt = {1.f, 2.f, 0.5f, 0.25f, 3.f};
  bm25_index* h = nullptr;
  expect(bm25_index_create(0, 5, 3, 5, ip.data(), 1, ix.data(), dt.data(), 0, nullptr),
         BM25_EINVAL, "out NULL");
  expect(bm25_index_create(0, -1, 3, 5, ip.data(), 1, ix.data(), dt.data(), 0, &h), BM25_EINVAL,
         "negative", "negative size");
  expect(bm25_index_create(0, 5, 3, 5, nullptr, 1, ix.data(), dt.data(), 0, &h), BM25_EINVAL,
         "NULL indptr", "NULL CSC");
  std::vector<int64_t> bad = {0, 3, 2, 5};
  expect(bm25_index_create(0, 5, 3, 5, bad.data(), 1, ix.data(), dt.data(), 0, &h), BM25_EINVAL,
         "decreasing", "decreases");
  std::vector<int64_t> end = {0, 2, 2, 4};
  expect(bm25_index_create(0, 5, 3, 5, end.data(), 1, ix.data(), dt.data(), 0, &h), BM25_EINVAL,
         "end", "end at nnz");
  std::vector<int32_t> ip32 = {0, 6, 6, 6};
  std::vector<int32_t> ix6(6, 0);
  std::vector<float> dt6(6, 1.f);
  expect(bm25_index_create(0, 5, 3, 6, ip32.data(), 0, ix6.data(), dt6.data(), 0, &h),
         BM25_EINVAL, "column longer than n_docs", "more entries");
  expect(bm25_index_create(0, 5, 3, 5, ip.data(), 1, ix.data(), dt.data(), -4, &h), BM25_EINVAL,
         "doc_offset", "doc_offset");
  expect(bm25_index_create(0, (int64_t)1 << 40, 3, 5, ip.data(), 1, ix.data(), dt.data(), 0, &h),
         BM25_EINVAL, "n_docs range");
  // a wide vocabulary: the host copy of indptr is O(V)
  const int64_t V = 200000;
  std::vector<int64_t> wide(V + 1, 0);
  for (int64_t t = 0; t <= V; ++t) wide[t] = t < 5 ? t : 5;
  if (ndev == 0) {
    expect(bm25_index_create(0, 5, 3, 5, ip.data(), 1, ix.data(), dt.data(), 0, &h), BM25_EHIP,
           "no GPU", "no HIP device");
    std::vector<int32_t> wix = {0, 1, 2, 3, 4};
    expect(bm25_index_create(0, 5, V, 5, wide.data(), 1, wix.data(), dt.data(), 0, &h), BM25_EHIP,
           "no GPU, wide", "no HIP device");
    int devs[2] = {0, 0};
    bm25_sharded* s = nullptr;
    expect(bm25_sharded_create(2, devs, 5, 3, 5, ip.data(), 1, ix.data(), dt.data(), &s),
           BM25_EHIP, "sharded, no GPU", "no HIP device");
    std::vector<int32_t> docs = {0, 1, 1}, terms = {0, 0, 2}, dl = {3, 4};
    std::vector<float> tf = {1.f, 2.f, 1.f};
    std::vector<int64_t> oip(4);
    std::vector<int32_t> oix(3);
    std::vector<float> odt(3);
    expect(bm25_build_scores(0, 2, 3, 3, docs.data(), terms.data(), tf.data(), dl.data(), 3.5, 1.5,
                             0.75, 0, nullptr, oip.data(), oix.data(), odt.data(), nullptr),
           BM25_EHIP, "build, no GPU", "no HIP device");
    check_host_call_no_device();
  }
  check_option_table();
  int devs[1] = {0};
  bm25_sharded* s = nullptr;
  expect(bm25_sharded_create(0, devs, 5, 3, 5, ip.data(), 1, ix.data(), dt.data(), &s), BM25_EINVAL,
         "sharded n_dev", "at least one device");
  expect(bm25_sharded_create(1, devs, 5, 3, 5, bad.data(), 1, ix.data(), dt.data(), &s),
         BM25_EINVAL, "sharded decreasing", "decreases");
  std::vector<int32_t> docs = {0, 1}, terms = {0, 7};
  std::vector<float> tf = {1.f, 1.f};
  std::vector<int32_t> dl = {1, 1};
  std::vector<int64_t> oip(4);
  std::vector<int32_t> oix(2);
  std::vector<float> odt(2);
  expect(bm25_build_scores(0, -2, 3, 2, docs.data(), terms.data(), tf.data(), dl.data(), 1.0, 1.5,
                           0.75, 0, nullptr, oip.data(), oix.data(), odt.data(), nullptr),
         BM25_EINVAL, "build negative", "negative size");
  expect(bm25_build_scores(0, 2, 3, 2, docs.data(), terms.data(), tf.data(), dl.data(), 1.0, 1.5,
                           0.75, 9, nullptr, oip.data(), oix.data(), odt.data(), nullptr),
         BM25_EINVAL, "build method", "unknown method");
  expect(bm25_build_scores(0, 2, 3, 2, nullptr, terms.data(), tf.data(), dl.data(), 1.0, 1.5, 0.75,
                           0, nullptr, oip.data(), oix.data(), odt.data(), nullptr),
         BM25_EINVAL, "build NULL", "NULL argument");
  // every entry point that takes a handle rejects NULL
  int32_t q[2] = {0, 1}, od[2];
  float os[2];
  double od64[2];
  int64_t v64 = 0, cnt[5];
  int32_t i32 = 0;
  uint32_t u32 = 0;
  expect(bm25_search(nullptr, q, 1, 2, 1, od, os), BM25_EINVAL, "search NULL");
  expect(bm25_search_device(nullptr, q, 1, 2, 1, od, os, nullptr), BM25_EINVAL, "device NULL");
  expect(bm25_scores_dense(nullptr, q, 2, os), BM25_EINVAL, "dense NULL");
  expect(bm25_scores_dense_f64(nullptr, q, 2, od64), BM25_EINVAL, "dense64 NULL");
  expect(bm25_topn_f64(nullptr, q, 2, 1, od, od64), BM25_EINVAL, "topn64 NULL");
  expect(bm25_index_set_values_f64(nullptr, od64), BM25_EINVAL, "values64 NULL");
  expect(bm25_index_fork(nullptr, nullptr), BM25_EINVAL, "fork NULL");
  bm25_index* f = nullptr;
  expect(bm25_index_fork(nullptr, &f), BM25_EINVAL, "fork NULL base", "unbuilt");
  expect(bm25_index_info(nullptr, &v64, &v64, &v64, &i32, &v64, &v64), BM25_EINVAL, "info NULL");
  expect(bm25_index_segments(nullptr, &i32, &v64), BM25_EINVAL, "segments NULL");
  expect(bm25_index_bounds(nullptr, &i32, &v64), BM25_EINVAL, "bounds NULL");
  expect(bm25_index_set_option(nullptr, "flat", 1), BM25_EINVAL, "set_option NULL");
  expect(bm25_index_get_option(nullptr, "flat", &v64), BM25_EINVAL, "get_option NULL");
  expect(bm25_search_dispatch(nullptr, &u32, &i32, &i32, &i32), BM25_EINVAL, "dispatch NULL");
  expect(bm25_search_stats(nullptr, &v64, &v64), BM25_EINVAL, "stats NULL");
  expect(bm25_search_stats_ex(nullptr, &v64, &v64, &v64), BM25_EINVAL, "stats_ex NULL");
  expect(bm25_search_counters(nullptr, cnt, 5), BM25_EINVAL, "counters NULL");
  expect(bm25_profile_enable(nullptr, 1), BM25_EINVAL, "profile NULL");
  expect(bm25_sample_width(nullptr, 10, 1, 10, &v64), BM25_EINVAL, "width NULL");
  expect(bm25_search_sample_device(nullptr, q, 1, 2, 1, 1, 10, nullptr, nullptr), BM25_EINVAL,
         "sample NULL");
  expect(bm25_search_finish_device(nullptr, q, 1, 2, 1, 1, 10, nullptr, od, os, nullptr),
         BM25_EINVAL, "finish NULL");
  expect(bm25_sharded_search(nullptr, q, 1, 2, 1, od, os), BM25_EINVAL, "sharded search NULL");
  expect(bm25_merge_topk_device(0, nullptr, nullptr, 0, 1, 1, od, os, nullptr), BM25_EINVAL,
         "merge W", "bad merge shape");
  expect(bm25_merge_sorted_device(0, nullptr, nullptr, 2, 4, 3, 5, od, os, nullptr), BM25_EINVAL,
         "merge stride", "bad merge shape");
  expect(bm25_index_destroy(nullptr), BM25_OK, "destroy NULL");
  expect(bm25_sharded_destroy(nullptr), BM25_OK, "sharded destroy NULL");
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("asan host check ok (%d devices)\n", ndev);
  return 0;
}
