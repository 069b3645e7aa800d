// ranked_check — the argument rules of the ranked searches
// (bm25_search_filtered, _weighted, _after, _collapsed) under AddressSanitizer
// and UBSan, without a device: check_ranked_shape and check_ranked_content
// (bm25mi_host.h) with the rule set of each call, on heap arrays of exactly
// the size a rule may read (Q*T, Q, M*W, n_docs), so an over-read is a
// sanitizer failure.  The expected texts are the calls' own, written out here.
// Built and run by tests/test_ranked_args_host.py with the host compiler
// alone (no HIP call is made, none is linked); fail() is this program's own.
#include <cstdarg>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../mojo-bm25_amd/csrc/bm25mi_host.h"

static std::string g_err;
int bm25mi::fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

using namespace bm25mi;

static const int64_t kDocs = 40, kTerms = 6, kW = (kDocs + 31) / 32;
static const char* g_set = "";

#define EXPECT(cond)                                                                    \
  do {                                                                                  \
    if (!(cond)) {                                                                      \
      fprintf(stderr, "ranked_check.cpp:%d: [%s] %s (last error: %s)\n", __LINE__, g_set, #cond, \
              g_err.c_str());                                                           \
      return 1;                                                                         \
    }                                                                                   \
  } while (0)

// One call's arguments in vectors of their own; args() points into them.
struct Case {
  int64_t Q = 3, T = 2, M = 2;
  int32_t k = 2, per_group = 1;
  std::vector<int32_t> queries{0, 5, 3, -1, 2, 4}, query_mask{0, 1, -1}, after_docs{7, -1, -2},
      groups = std::vector<int32_t>((size_t)kDocs, 1), out_docs = std::vector<int32_t>(6, 7);
  std::vector<float> weights{1.f, 2.f, 0.5f, 9.f, -1.f, 0.f}, after_scores{1.5f, 0.f, 0.f},
      out_scores = std::vector<float>(6, 7.f);
  std::vector<uint32_t> masks = std::vector<uint32_t>((size_t)(2 * kW), 0xFFu);
  bool no_queries = false, no_weights = false, no_masks = false, no_query_mask = false,
       no_after_scores = false, no_after_docs = false, no_groups = false, no_docs = false,
       no_scores = false;
  unsigned rules = 0;

  RankedArgs args() {
    RankedArgs a;
    a.Q = Q, a.T = T, a.M = M, a.k = k;
    a.queries = no_queries ? nullptr : queries.data();
    a.masks = no_masks ? nullptr : masks.data();
    a.query_mask = no_query_mask ? nullptr : query_mask.data();
    a.out_docs = no_docs ? nullptr : out_docs.data();
    a.out_scores = no_scores ? nullptr : out_scores.data();
    if (!(rules & kRankedNeedsMask))  // (the filtered call takes no weights)
      a.weights = no_weights ? nullptr : weights.data();
    if (rules & kRankedCursor) {
      a.after_scores = no_after_scores ? nullptr : after_scores.data();
      a.after_docs = no_after_docs ? nullptr : after_docs.data();
    }
    if (rules & kRankedCollapse) {
      a.groups = no_groups ? nullptr : groups.data();
      a.per_group = per_group;
    }
    return a;
  }
  // The call as an entry point makes it: shape, the early return, content.
  int run() {
    g_err.clear();
    const RankedArgs a = args();
    int rc = check_ranked_shape(kDocs, a, rules);
    if (rc || a.Q == 0 || a.k == 0) return rc;
    return check_ranked_content(kTerms, a, rules);
  }
  // No array but the token ids.
  void all_null() {
    no_queries = no_weights = no_masks = no_query_mask = no_after_scores = no_after_docs =
        no_groups = no_docs = no_scores = true;
  }
};

static const char* const kNegK = "negative dimensions are not allowed (top_k=-1)";
static const char* const kBigK = "kth(=-1) out of bounds (40)";
static const char* const kNegShape = "negative query or mask shape";
static const char* const kToken =
    "The maximum token ID in the query (6) is higher than the number of tokens in the index.";
static const char* const kNoMasks = "no masks: query_mask must name -1 (no filter) for every query";
static const char* const kOneSided =
    "after_scores and after_docs must both be given or both be NULL";
static const char* const kGroups = "NULL groups (one int32 per document; < 0: no group)";
static const char* const kLds =
    "k=4097: a collapsed search is limited to k <= 4096 (the per-row group table lives in LDS)";

static bool is(int rc, const char* text) { return rc == BM25_EINVAL && g_err == text; }

static int check_rule_set(unsigned rules) {
  const bool weighted = rules & kRankedWeights, filtered = rules & kRankedNeedsMask,
             cursor = rules & kRankedCursor, collapse = rules & kRankedCollapse;
  const bool takes_weights = !filtered;
  auto fresh = [rules] {
    Case c;
    c.rules = rules;
    return c;
  };
  const float nan = std::numeric_limits<float>::quiet_NaN();
  const float inf = std::numeric_limits<float>::infinity();
  Case c = fresh();
  EXPECT(c.run() == BM25_OK);
  // the early return: no pointer is looked at
  c = fresh(), c.all_null(), c.k = 0;
  EXPECT(c.run() == BM25_OK);
  c = fresh(), c.all_null(), c.Q = 0;
  EXPECT(c.run() == BM25_OK);
  // shapes
  c = fresh(), c.k = -1;
  EXPECT(is(c.run(), kNegK));
  c = fresh(), c.k = 41;
  EXPECT(is(c.run(), kBigK));
  c = fresh(), c.M = -1;
  EXPECT(is(c.run(), kNegShape));
  c = fresh(), c.Q = -1;
  EXPECT(is(c.run(), kNegShape));
  c = fresh(), c.T = -1;
  EXPECT(is(c.run(), kNegShape));
  // one fault at a time
  c = fresh(), c.no_queries = true;
  EXPECT(is(c.run(), "NULL queries"));
  c = fresh(), c.no_masks = true;
  EXPECT(is(c.run(), "NULL masks"));
  c = fresh(), c.no_docs = true;
  EXPECT(is(c.run(), "NULL output"));
  c = fresh(), c.no_scores = true;
  EXPECT(is(c.run(), "NULL output"));
  c = fresh(), c.queries[3] = 6;
  EXPECT(is(c.run(), kToken));
  c = fresh(), c.query_mask[1] = -2;
  EXPECT(is(c.run(), "query_mask[1] = -2 is outside [-1, 2)"));
  c = fresh(), c.query_mask[1] = 2;
  EXPECT(is(c.run(), "query_mask[1] = 2 is outside [-1, 2)"));
  // no terms: neither the queries nor the weights are needed
  c = fresh(), c.T = 0, c.no_queries = c.no_weights = true, c.queries.clear(), c.weights.clear();
  EXPECT(c.run() == BM25_OK);
  // no mask ids: every query takes mask 0
  c = fresh(), c.no_query_mask = true, c.query_mask.clear();
  EXPECT(c.run() == BM25_OK);
  // the weights
  c = fresh(), c.no_weights = true, c.weights.clear();
  if (weighted) EXPECT(is(c.run(), "NULL weights"));
  else EXPECT(c.run() == BM25_OK);
  c = fresh(), c.weights[2] = nan;
  if (takes_weights) EXPECT(is(c.run(), "weights[1][0] = nan is not finite"));
  else EXPECT(c.run() == BM25_OK);
  c = fresh(), c.weights[2] = inf;
  if (takes_weights) EXPECT(is(c.run(), "weights[1][0] = inf is not finite"));
  c = fresh(), c.weights[2] = -inf;
  if (takes_weights) EXPECT(is(c.run(), "weights[1][0] = -inf is not finite"));
  c = fresh(), c.weights[3] = nan;  // (a padding slot: its weight is ignored)
  EXPECT(c.run() == BM25_OK);
  // no masks: the filtered call alone wants mask ids then
  c = fresh(), c.M = 0, c.no_masks = c.no_query_mask = true, c.masks.clear(), c.query_mask.clear();
  if (filtered) EXPECT(is(c.run(), kNoMasks));
  else EXPECT(c.run() == BM25_OK);
  c = fresh(), c.M = 0, c.no_masks = true, c.masks.clear(), c.query_mask = {-1, -1, -1};
  EXPECT(c.run() == BM25_OK);
  c.query_mask[2] = 0;
  EXPECT(is(c.run(), "query_mask[2] = 0 is outside [-1, 0)"));
  // the cursor
  if (cursor) {
    c = fresh(), c.no_after_scores = true;
    EXPECT(is(c.run(), kOneSided));
    c = fresh(), c.no_after_docs = true;
    EXPECT(is(c.run(), kOneSided));
    c = fresh(), c.all_null(), c.no_after_docs = false, c.k = 0;  // (before the early return)
    EXPECT(is(c.run(), kOneSided));
    c = fresh(), c.k = 41, c.no_after_docs = true;  // (after k)
    EXPECT(is(c.run(), kBigK));
    c = fresh(), c.no_after_scores = c.no_after_docs = true;
    EXPECT(c.run() == BM25_OK);
    c = fresh(), c.after_docs[1] = -3;
    EXPECT(is(c.run(), "after_docs[1] = -3 is below BM25_AFTER_NONE (-2): a cursor names a doc id "
                       ">= 0, -1 (exhausted) or BM25_AFTER_NONE"));
    c = fresh(), c.after_docs[2] = 5, c.after_scores[2] = nan;
    EXPECT(is(c.run(), "after_scores[2] = nan is not a score (the cursor of doc 5)"));
    c = fresh(), c.after_scores[1] = c.after_scores[2] = nan;  // (docs -1 and -2: not read)
    EXPECT(c.run() == BM25_OK);
    c = fresh(), c.after_scores[0] = inf, c.after_docs[0] = std::numeric_limits<int32_t>::max();
    EXPECT(c.run() == BM25_OK);
  }
  // the collapse
  if (collapse) {
    c = fresh(), c.k = 4097;  // (before k > n_docs)
    EXPECT(is(c.run(), kLds));
    c = fresh(), c.per_group = 0;
    EXPECT(is(c.run(), "per_group=0 must be >= 1"));
    c = fresh(), c.per_group = 0, c.k = 41;
    EXPECT(is(c.run(), "per_group=0 must be >= 1"));
    c = fresh(), c.per_group = 0, c.k = 0, c.all_null();
    EXPECT(is(c.run(), "per_group=0 must be >= 1"));
    c = fresh(), c.no_groups = true;
    EXPECT(is(c.run(), kGroups));
    c = fresh(), c.no_groups = c.no_docs = true;
    EXPECT(is(c.run(), kGroups));
    c = fresh(), c.no_groups = c.no_masks = true;
    EXPECT(is(c.run(), "NULL masks"));
  } else {
    c = fresh(), c.k = 4097;
    EXPECT(is(c.run(), "kth(=-4057) out of bounds (40)"));
  }
  // two faults in one call: the first named wins
  c = fresh(), c.k = -1, c.no_queries = true;
  EXPECT(is(c.run(), kNegK));
  c = fresh(), c.M = -1, c.k = -1;
  EXPECT(is(c.run(), kNegShape));
  c = fresh(), c.no_queries = c.no_masks = true;
  EXPECT(is(c.run(), "NULL queries"));
  c = fresh(), c.no_masks = c.no_docs = true;
  EXPECT(is(c.run(), "NULL masks"));
  c = fresh(), c.no_docs = true, c.queries[0] = 6;
  EXPECT(is(c.run(), "NULL output"));
  c = fresh(), c.queries[3] = 6, c.weights[2] = nan;
  EXPECT(is(c.run(), kToken));
  c = fresh(), c.queries[3] = 6, c.query_mask[0] = 2;
  EXPECT(is(c.run(), kToken));
  if (weighted) {
    c = fresh(), c.no_queries = c.no_weights = true;
    EXPECT(is(c.run(), "NULL queries"));
    c = fresh(), c.no_weights = c.no_masks = true;
    EXPECT(is(c.run(), "NULL weights"));
  }
  if (takes_weights) {
    c = fresh(), c.weights[2] = nan, c.query_mask[0] = 2;
    EXPECT(is(c.run(), "weights[1][0] = nan is not finite"));
  }
  if (filtered) {
    c = fresh(), c.M = 0, c.no_masks = c.no_query_mask = c.no_docs = true;
    EXPECT(is(c.run(), kNoMasks));
  }
  if (cursor) {
    c = fresh(), c.query_mask[2] = 2, c.after_docs[0] = -3;
    EXPECT(is(c.run(), "query_mask[2] = 2 is outside [-1, 2)"));
  }
  return 0;
}

int main() {
  const struct {
    const char* name;
    unsigned rules;
  } sets[] = {{"filtered", kRankedNeedsMask},
              {"weighted", kRankedWeights},
              {"cursor", kRankedCursor},
              {"collapsed", kRankedCollapse}};
  for (const auto& s : sets) {
    g_set = s.name;
    if (check_rule_set(s.rules)) return 1;
  }
  // the helpers the other calls share
  g_set = "helpers";
  EXPECT(check_k(40, 41, true) == BM25_OK && check_k(40, 40) == BM25_OK);
  EXPECT(check_k(40, -1, true) == BM25_EINVAL && g_err == kNegK);
  std::vector<int32_t> ids{-1, 5, 2};
  EXPECT(max_token(0, ids.data(), 3) == 5 && max_token(7, ids.data(), 3) == 7);
  EXPECT(max_token(0, nullptr, 0) == 0);
  EXPECT(check_token_ids(6, 0, ids.data(), 3) == BM25_OK);
  EXPECT(check_token_ids(5, 0, ids.data(), 3) == BM25_EINVAL);
  EXPECT(check_token_ids(0, 0, nullptr, 0) == BM25_EINVAL);  // (max(initial = 0) >= n_terms)
  printf("ranked_check ok\n");
  return 0;
}
