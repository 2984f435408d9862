// Host check of csrc/anti_entropy.h and of the arrival round's plan (csrc/round_plan.h); built and
// run by tests/test_anti_entropy_host.py.  Prints "ok <cases>" and exits 0, or the first failure.
//
//  * every (first, last, period) with 0 <= first <= 6, first <= last <= 14, 1 <= period <= 5 against
//    a brute-force list of its request rounds: request / reply / arrival round for -3 <= r <= 22,
//    "a request round at or ahead", "an arrival round at or ahead", the last request round;
//  * the edges: period 0 is off whatever first and last say, last = INT32_MAX does not overflow,
//    argument validation of every bad kind and its precedence;
//  * plan_round: in a dense gossip history (the round would be fused) an arrival round is unfused
//    with whole rows, not blind, not held, and its counters are read before its push; the same
//    facts without `pull` -- the rounds around it -- keep the fused form; a flood arrival round
//    keeps the flood pull; a decay tail is not batched while an arrival round lies ahead.
#include <cstdio>
#include <cstdlib>
#include <set>

#include "anti_entropy.h"
#include "round_plan.h"

namespace ae = anti_entropy;
namespace rp = round_plan;

static long cases = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    ++cases;                                              \
    if (!(cond)) {                                        \
      std::printf("FAIL %s:%d %s -- ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                           \
      std::printf("\n");                                  \
      std::exit(1);                                       \
    }                                                     \
  } while (0)

static void brute(int32_t first, int32_t last, int32_t period) {
  CHECK(ae::check(first, last, period) == ae::OK, "%d %d %d", first, last, period);
  ae::Setting s;
  s.first = first;
  s.last = last;
  s.period = period;
  std::set<int> req;
  for (int r = first; r <= last; ++r)
    if ((r - first) % period == 0) req.insert(r);
  CHECK(s.on(), "on");
  CHECK(!req.empty() && s.last_request() == *req.rbegin(), "last request %d %d %d", first, last, period);
  for (int r = -3; r <= 22; ++r) {
    CHECK(s.request_round(r) == (req.count(r) > 0), "request %d in %d %d %d", r, first, last, period);
    CHECK(s.reply_round(r) == (req.count(r - 1) > 0), "reply %d in %d %d %d", r, first, last, period);
    CHECK(s.arrival_round(r) == (req.count(r - 2) > 0), "arrival %d in %d %d %d", r, first, last, period);
    bool req_ahead = false, arr_ahead = false;
    for (int q : req) {
      req_ahead |= q >= r;
      arr_ahead |= q + 2 >= r;
    }
    CHECK(s.request_ahead(r) == req_ahead, "request ahead %d in %d %d %d", r, first, last, period);
    CHECK(s.arrival_ahead(r) == arr_ahead, "arrival ahead %d in %d %d %d", r, first, last, period);
    // an exchange in flight keeps the run going: a reply or arrival round implies "ahead"
    if (s.reply_round(r) || s.arrival_round(r)) CHECK(s.arrival_ahead(r), "in flight %d", r);
  }
}

static void edges() {
  ae::Setting off;
  for (int r = -3; r <= 10; ++r) {
    CHECK(!off.request_round(r) && !off.reply_round(r) && !off.arrival_round(r), "off %d", r);
    CHECK(!off.request_ahead(r) && !off.arrival_ahead(r), "off ahead %d", r);
  }
  off.first = 2;
  off.last = 9;  // (period 0: first and last are not looked at)
  CHECK(!off.on() && !off.request_round(2) && !off.arrival_ahead(0), "period 0");
  CHECK(ae::check(-5, -9, 0) == ae::OK, "period 0 removes, whatever the rest");
  CHECK(ae::check(0, 0, -1) == ae::BAD_PERIOD, "period");
  CHECK(ae::check(-1, -2, -1) == ae::BAD_PERIOD, "period first");
  CHECK(ae::check(-1, 5, 1) == ae::BAD_FIRST, "first");
  CHECK(ae::check(-1, -2, 1) == ae::BAD_FIRST, "first before last");
  CHECK(ae::check(3, 2, 1) == ae::BAD_LAST, "last");
  CHECK(ae::check(3, 3, 1) == ae::OK, "one round");
  CHECK(ae::check(0, 0x7FFFFFFF, 0x7FFFFFFF) == ae::OK, "max");
  ae::Setting big;
  big.first = 0x7FFFFFFF - 1;
  big.last = 0x7FFFFFFF;
  big.period = 1;
  CHECK(big.last_request() == 0x7FFFFFFFll, "last request at INT32_MAX");
  CHECK(big.request_round(0x7FFFFFFFll) && big.arrival_round(0x7FFFFFFFll + 2), "no overflow");
  CHECK(big.arrival_ahead(0x7FFFFFFFll + 2) && !big.arrival_ahead(0x7FFFFFFFll + 3), "ahead past INT32_MAX");
  big.first = 0;
  big.period = 0x7FFFFFFF;
  CHECK(big.last_request() == 0x7FFFFFFFll && big.request_round(0) && !big.request_round(1), "one long period");
}

static void plans() {
  // a dense gossip history: the last round pushed into E and the frontier is still dense
  rp::RoundRules rules;
  rules.W = 64;
  rules.v_conn = 1000;
  rp::RoundHistory dense;
  dense.prev_aw = 40000;
  dense.prev_av = 900;
  dense.prev2_aw = 30000;
  dense.prev2_av = 800;
  dense.last_new = 500000;
  dense.prev2_new = 300000;
  dense.prev_sw = 100000;
  dense.saw_dense = dense.last_push_e = true;
  rp::RoundCaps caps;
  caps.gossip = caps.e_planes = caps.fused = caps.update_push = caps.sparse_scatter = caps.partial_rows = true;
  for (int skip = 0; skip < 2; ++skip) {
    rp::RoundFacts f;
    f.round = 9;
    f.skip_frontier = skip != 0;
    const rp::RoundPlan around = rp::plan_round(dense, rules, caps, f);
    CHECK(around.receive == rp::Receive::Fused && around.push == rp::Push::Made, "the rounds around stay fused");
    f.pull = true;
    const rp::RoundPlan a = rp::plan_round(dense, rules, caps, f);
    CHECK(a.receive == rp::Receive::GossipPull, "an arrival round is unfused");
    CHECK(a.store_f == 1, "whole rows");
    CHECK(!a.held, "not held");
    CHECK(a.push == rp::Push::ByCounters && a.mid_read, "its own counters choose the push");
    CHECK(a.list != rp::PushList::PrevSw, "never blind");
  }
  // a sparse tail: a plain round pushes blind, an arrival round never does
  rp::RoundHistory tail;
  tail.prev_aw = 30;
  tail.prev_av = 20;
  tail.prev2_aw = 90;
  tail.prev2_av = 60;
  tail.last_new = 40;
  tail.prev2_new = 120;
  tail.prev_sw = 50;
  tail.saw_dense = true;
  {
    rp::RoundFacts f;
    f.round = 30;
    f.skip_frontier = true;
    const rp::RoundPlan plain = rp::plan_round(tail, rules, caps, f);
    CHECK(plain.receive == rp::Receive::Update && plain.list == rp::PushList::PrevSw && plain.store_f == 2,
          "a plain tail round is blind with partial rows");
    f.pull = true;
    const rp::RoundPlan a = rp::plan_round(tail, rules, caps, f);
    CHECK(a.receive == rp::Receive::Update && a.store_f == 1 && a.list == rp::PushList::Counters && a.mid_read && !a.held,
          "an arrival round in the tail");
    rp::DecayFacts d;
    d.round = 30;
    d.V = 1000;
    CHECK(rp::decay_batchable(tail, rules, caps, d), "the tail is batchable");
    d.pull_ahead = true;
    CHECK(!rp::decay_batchable(tail, rules, caps, d), "not across an arrival round");
  }
  {  // flood
    rp::RoundCaps fc;
    rp::RoundFacts f;
    f.round = 5;
    f.pull = true;
    const rp::RoundPlan a = rp::plan_round(rp::RoundHistory{}, rules, fc, f);
    CHECK(a.receive == rp::Receive::FloodPull && a.store_f == 1 && !a.held, "flood arrival round");
  }
}

int main() {
  for (int first = 0; first <= 6; ++first)
    for (int last = first; last <= 14; ++last)
      for (int period = 1; period <= 5; ++period) brute(first, last, period);
  edges();
  plans();
  std::printf("ok %ld\n", cases);
  return 0;
}
