// Host check of csrc/downtime.h (tests/test_downtime_host.py): the header the engine and the
// kernels include, walked by a stand-alone program -- validation of every bad-interval kind, the
// refusal of originations at an offline peer in both call orders, the sorted-endpoint sweep against
// a brute-force count over random intervals, and the cases V = 1, all -1 and until = INT32_MAX.
// Prints "ok <cases>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "downtime.h"

static long cases = 0;
#define CHECK(x)                                                     \
  do {                                                               \
    ++cases;                                                         \
    if (!(x)) {                                                      \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x);  \
      std::exit(1);                                                  \
    }                                                                \
  } while (0)

using downtime::FOREVER;

static int64_t brute(const std::vector<int32_t>& f, const std::vector<int32_t>& u, int32_t r) {
  int64_t n = 0;
  for (size_t v = 0; v < f.size(); ++v) n += f[v] >= 0 && f[v] <= r && r < u[v];
  return n;
}

int main() {
  // the predicate at the edges of the interval
  CHECK(!downtime::offline(2, 3, 5) && downtime::offline(3, 3, 5) && downtime::offline(4, 3, 5) &&
        !downtime::offline(5, 3, 5));
  CHECK(!downtime::offline(0, -1, FOREVER) && !downtime::offline(FOREVER - 1, -1, FOREVER));
  CHECK(downtime::offline(0, 0, 1) && !downtime::offline(1, 0, 1));
  CHECK(downtime::offline(FOREVER - 1, 7, FOREVER) && !downtime::offline(6, 7, FOREVER));

  // validation: every bad-interval kind, and the first bad peer is the one reported
  CHECK(downtime::check(-1, 0) == downtime::OK);        // never offline: until is not read
  CHECK(downtime::check(-1, -5) == downtime::OK);
  CHECK(downtime::check(0, 1) == downtime::OK);
  CHECK(downtime::check(4, FOREVER) == downtime::OK);
  CHECK(downtime::check(-2, 3) == downtime::BAD_FROM);
  CHECK(downtime::check(INT32_MIN, 3) == downtime::BAD_FROM);
  CHECK(downtime::check(3, 3) == downtime::BAD_UNTIL);  // empty
  CHECK(downtime::check(3, 2) == downtime::BAD_UNTIL);  // reversed
  CHECK(downtime::check(0, 0) == downtime::BAD_UNTIL);
  CHECK(downtime::check(0, -1) == downtime::BAD_UNTIL);
  CHECK(downtime::check(FOREVER, FOREVER) == downtime::BAD_UNTIL);
  {
    std::vector<int32_t> f = {-1, 2, 5, -3, 4}, u = {0, 4, 5, 9, 1};
    downtime::Bad what = downtime::OK;
    CHECK(downtime::first_bad(5, f.data(), u.data(), &what) == 2 && what == downtime::BAD_UNTIL);
    f[2] = -1;
    CHECK(downtime::first_bad(5, f.data(), u.data(), &what) == 3 && what == downtime::BAD_FROM);
    f[3] = -1;
    CHECK(downtime::first_bad(5, f.data(), u.data(), &what) == 4 && what == downtime::BAD_UNTIL);
    f[4] = 0;
    CHECK(downtime::first_bad(5, f.data(), u.data(), nullptr) == -1);
    CHECK(downtime::any(5, f.data()));
  }

  // originations at an offline peer, in both call orders: the schedule first and the downtime
  // checked against it (p2pg_set_downtime), or the downtime first and a new schedule / a single
  // origination checked against it (p2pg_set_sources[_at], p2pg_originate)
  {
    std::vector<int32_t> f = {-1, 2, 0, 6}, u = {FOREVER, 4, 3, FOREVER};
    std::vector<int32_t> src = {0, 1, 1, 2, 3, -1}, start = {0, 1, 4, 3, 5, -1};
    CHECK(downtime::first_refused(6, src.data(), start.data(), f.data(), u.data()) == -1);
    CHECK(downtime::first_refused(6, src.data(), nullptr, f.data(), u.data()) == 3);  // all in round 0: peer 2 joins late
    start[2] = 3;  // peer 1 offline in [2, 4)
    CHECK(downtime::first_refused(6, src.data(), start.data(), f.data(), u.data()) == 2);
    start[2] = 2;
    CHECK(downtime::first_refused(6, src.data(), start.data(), f.data(), u.data()) == 2);
    start[2] = 4;
    start[4] = 6;  // the crash round itself
    CHECK(downtime::first_refused(6, src.data(), start.data(), f.data(), u.data()) == 4);
    start[4] = 1 << 30;
    CHECK(downtime::first_refused(6, src.data(), start.data(), f.data(), u.data()) == 4);
    // the other order: the same schedule against a downtime that is set later
    start[4] = 5;
    std::vector<int32_t> f2 = {0, -1, -1, -1}, u2 = {1, FOREVER, FOREVER, FOREVER};
    CHECK(downtime::first_refused(6, src.data(), start.data(), f2.data(), u2.data()) == 0);
    f2[0] = 1;
    u2[0] = 2;
    CHECK(downtime::first_refused(6, src.data(), start.data(), f2.data(), u2.data()) == -1);
    // one origination (p2pg_originate): peer 3 in rounds 5 and 6
    const int32_t peer = 3;
    int32_t round = 5;
    CHECK(downtime::first_refused(1, &peer, &round, f.data(), u.data()) == -1);
    round = 6;
    CHECK(downtime::first_refused(1, &peer, &round, f.data(), u.data()) == 0);
    // an unscheduled message (start -1, source -1) is skipped
    const int32_t none = -1;
    CHECK(downtime::first_refused(1, &none, &none, f.data(), u.data()) == -1);
  }

  // V = 1
  {
    int32_t f = 2, u = 3;
    downtime::Sweep s;
    s.build(1, &f, &u);
    CHECK(!s.empty() && s.min_from() == 2 && s.max_until() == 3);
    CHECK(s.count(1) == 0 && s.count(2) == 1 && s.count(3) == 0);
    CHECK(!s.offline_round(1) && s.offline_round(2) && !s.offline_round(3));
    CHECK(s.offline_ahead(0) && s.offline_ahead(2) && !s.offline_ahead(3));
    CHECK(!s.in_span(1) && s.in_span(2) && !s.in_span(3));
    f = -1;
    s.build(1, &f, &u);
    CHECK(s.empty() && !s.offline_round(2) && !s.offline_ahead(0) && !s.in_span(2) && s.count(2) == 0);
    CHECK(!downtime::any(1, &f));
  }
  // all -1, a null pointer, and an empty build after a full one
  {
    std::vector<int32_t> f(100, -1), u(100, FOREVER);
    downtime::Sweep s;
    s.build(100, f.data(), u.data());
    CHECK(s.empty() && s.min_from() == -1 && s.max_until() == -1 && !s.offline_ahead(0));
    CHECK(!downtime::any(100, f.data()) && !downtime::any(100, nullptr));
    f[7] = 1;
    s.build(100, f.data(), u.data());
    CHECK(!s.empty());
    s.build(0, nullptr, nullptr);
    CHECK(s.empty() && s.count(5) == 0);
  }
  // until = INT32_MAX: every round from the crash on is an offline round, and one lies ahead of any
  {
    std::vector<int32_t> f = {-1, 5, 9}, u = {FOREVER, FOREVER, 11};
    downtime::Sweep s;
    s.build(3, f.data(), u.data());
    CHECK(s.min_from() == 5 && s.max_until() == FOREVER);
    CHECK(s.count(4) == 0 && s.count(5) == 1 && s.count(9) == 2 && s.count(10) == 2 && s.count(11) == 1);
    CHECK(s.count(FOREVER - 1) == 1 && s.offline_round(1 << 30) && s.offline_ahead(FOREVER - 1));
    CHECK(s.offline_ahead(0) && !s.offline_round(0) && !s.in_span(4) && s.in_span(5) && s.in_span(FOREVER - 1));
  }

  // the sweep against a brute-force count over random intervals
  std::mt19937 rng(12345);
  for (int trial = 0; trial < 300; ++trial) {
    const int V = 1 + (int)(rng() % 400);
    const int span = 1 + (int)(rng() % 60);
    std::vector<int32_t> f(V), u(V);
    for (int v = 0; v < V; ++v) {
      const unsigned kind = rng() % 10;
      if (kind < 4) {
        f[v] = -1;
        u[v] = (rng() & 1) ? FOREVER : (int32_t)(rng() % 7);  // (never read)
      } else if (kind == 4) {
        f[v] = (int32_t)(rng() % span);
        u[v] = FOREVER;
      } else if (kind == 5) {
        f[v] = 0;
        u[v] = 1 + (int32_t)(rng() % span);
      } else {
        f[v] = (int32_t)(rng() % span);
        u[v] = f[v] + 1 + (int32_t)(rng() % 4);
      }
    }
    CHECK(downtime::first_bad(V, f.data(), u.data(), nullptr) == -1);
    downtime::Sweep s;
    s.build(V, f.data(), u.data());
    int32_t lo = FOREVER, hi = -1;
    for (int v = 0; v < V; ++v)
      if (f[v] >= 0) {
        lo = f[v] < lo ? f[v] : lo;
        hi = u[v] > hi ? u[v] : hi;
      }
    CHECK(s.empty() == (hi < 0));
    if (!s.empty()) CHECK(s.min_from() == lo && s.max_until() == hi);
    bool later = false;  // is some round >= r an offline round?  (walked downwards)
    const int32_t top = span + 8;
    if (hi == FOREVER) later = true;
    for (int32_t r = top; r >= 0; --r) {
      const int64_t n = brute(f, u, r);
      CHECK(s.count(r) == n);
      CHECK(s.offline_round(r) == (n > 0));
      later = later || n > 0;
      CHECK(s.offline_ahead(r) == later);
      CHECK(s.in_span(r) == (!s.empty() && lo <= r && r < hi));
    }
    CHECK(s.count(FOREVER - 1) == brute(f, u, FOREVER - 1));
  }
  std::printf("ok %ld\n", cases);
  return 0;
}
