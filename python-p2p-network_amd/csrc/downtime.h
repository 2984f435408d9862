// Peer downtime (p2pg_set_downtime): the host's side of the per-peer offline
// intervals.  Peer v is offline in the half-open interval of rounds [from[v], until[v]):
// from[v] = -1 never, otherwise 0 <= from[v] < until[v]; until[v] = INT32_MAX never returns (a
// crash), from[v] = 0 joins late.  Here: the one definition of "offline in round r" (the kernels
// evaluate the same function), the validation of the two arrays, the check that no origination
// falls into its origin's interval, and a sorted-endpoint sweep that answers "how many peers are
// offline in round r" in O(log V).
//
// Plain C++: included by engine.cpp, by the kernels (the predicate only) and by host programs
// (tests/test_downtime_host.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DOWNTIME_HD __host__ __device__ inline
#else
#define DOWNTIME_HD inline
#endif

namespace downtime {

constexpr int32_t FOREVER = 0x7FFFFFFF;

// Is a peer with the interval [from, until) offline in round r?
DOWNTIME_HD bool offline(int32_t r, int32_t from, int32_t until) { return from >= 0 && from <= r && r < until; }

// What is wrong with an interval (0: nothing).
enum Bad { OK = 0, BAD_FROM = 1, BAD_UNTIL = 2 };
inline Bad check(int32_t from, int32_t until) {
  if (from < -1) return BAD_FROM;
  if (from >= 0 && until <= from) return BAD_UNTIL;
  return OK;
}

// The first peer with a bad interval (what = its kind), or -1.
inline int64_t first_bad(int64_t V, const int32_t* from, const int32_t* until, Bad* what) {
  for (int64_t v = 0; v < V; ++v) {
    const Bad b = check(from[v], until[v]);
    if (b != OK) {
      if (what) *what = b;
      return v;
    }
  }
  return -1;
}

// Does any peer carry an interval?  (None: the engine without the call.)
inline bool any(int64_t V, const int32_t* from) {
  for (int64_t v = 0; from && v < V; ++v)
    if (from[v] >= 0) return true;
  return false;
}

// The first of n originations (src[i] in round start[i]; start < 0 = unscheduled, skipped) whose
// origin is offline in its start round, or -1: originations at an offline peer are refused.
inline int64_t first_refused(int64_t n, const int32_t* src, const int32_t* start, const int32_t* from,
                             const int32_t* until) {
  for (int64_t i = 0; i < n; ++i) {
    const int32_t s = start ? start[i] : 0;
    if (s < 0 || src[i] < 0) continue;
    if (offline(s, from[src[i]], until[src[i]])) return i;
  }
  return -1;
}

// The sorted endpoints of every interval.  #(from <= r) - #(until <= r) peers are offline in round
// r (from < until: a peer counted by the second term is counted by the first).
struct Sweep {
  std::vector<int32_t> froms, untils;  // ascending, the peers with an interval only

  void build(int64_t V, const int32_t* from, const int32_t* until) {
    froms.clear();
    untils.clear();
    for (int64_t v = 0; from && v < V; ++v)
      if (from[v] >= 0) {
        froms.push_back(from[v]);
        untils.push_back(until[v]);
      }
    std::sort(froms.begin(), froms.end());
    std::sort(untils.begin(), untils.end());
  }
  bool empty() const { return froms.empty(); }
  int32_t min_from() const { return froms.empty() ? -1 : froms.front(); }
  int32_t max_until() const { return untils.empty() ? -1 : untils.back(); }
  // peers offline in round r
  int64_t count(int32_t r) const {
    const int64_t a = std::upper_bound(froms.begin(), froms.end(), r) - froms.begin();
    const int64_t b = std::upper_bound(untils.begin(), untils.end(), r) - untils.begin();
    return a - b;
  }
  // Is round r an offline round (somebody is offline in it)?
  bool offline_round(int32_t r) const { return count(r) > 0; }
  // Does an offline round lie at or after round r?  (The round max_until - 1 is one: the peer
  // with the largest until is offline in it.)
  bool offline_ahead(int32_t r) const { return !empty() && r < max_until(); }
  // min(from) <= r < max(until): the rounds whose arrivals a downtime may have cut
  bool in_span(int32_t r) const { return !empty() && min_from() <= r && r < max_until(); }
};

}  // namespace downtime
