// Host check of csrc/netsplit.h and of the netsplit's part of csrc/round_plan.h
// (tests/test_netsplit_host.py): the headers the engine and the kernels include, walked by a
// stand-alone program -- the cut predicate at the window's edges, validation, the window's questions
// (cut round, cut sends, cut ahead) and the crossing count against brute force over random graphs and
// sides, and the plan of every round a netsplit acts on.  Prints "ok <cases>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "netsplit.h"
#include "round_plan.h"

static long cases = 0;
#define CHECK(x)                                                     \
  do {                                                               \
    ++cases;                                                         \
    if (!(x)) {                                                      \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x);  \
      std::exit(1);                                                  \
    }                                                                \
  } while (0)

namespace rp = round_plan;

static void plans() {
  rp::RoundRules r;
  r.W = 64;
  r.v_conn = 1000;
  rp::RoundHistory dense;  // the previous round pushed a dense frontier into E
  dense.prev_aw = dense.prev2_aw = 50000;
  dense.prev_av = dense.prev2_av = 900;
  dense.last_new = 40000;
  dense.prev2_new = 30000;
  dense.prev_sw = 60000;
  dense.saw_dense = dense.last_push_e = true;
  rp::RoundHistory sparse;  // a rising sparse run that predict_dense calls dense
  sparse.prev_aw = 40000;
  sparse.prev2_aw = 8000;
  sparse.prev_av = 700;
  sparse.prev2_av = 300;
  sparse.last_new = 40000;
  sparse.prev2_new = 8000;
  sparse.prev_sw = 60000;
  rp::RoundCaps g;
  g.gossip = g.e_planes = g.fused = g.update_push = g.sparse_scatter = g.partial_rows = true;
  rp::RoundFacts f;
  f.round = 7;
  f.skip_frontier = true;
  // without the cut these two are the fused and the update+push round
  CHECK(rp::plan_round(dense, r, g, f).receive == rp::Receive::Fused);
  CHECK(rp::plan_round(sparse, r, g, f).receive == rp::Receive::UpdatePush);
  f.cut = true;
  for (int withf = 0; withf < 16; ++withf) {
    rp::RoundFacts q = f;
    q.origination = withf & 1;
    q.offline = withf & 2;
    q.pull = withf & 4;
    q.skip_frontier = withf & 8;
    for (const rp::RoundHistory* h : {&dense, &sparse}) {
      const rp::RoundPlan p = rp::plan_round(*h, r, g, q);
      CHECK(p.receive == (h == &dense ? rp::Receive::GossipPull : rp::Receive::Update));
      CHECK(p.push == rp::Push::AtomicCut && !p.held && p.store_f == 1);
      CHECK(p.list == rp::PushList::None && !p.mid_read);
      CHECK(rp::resolve_push(p, r, 1u << 30, 1000) == rp::Push::AtomicCut);
    }
  }
  // round 0 of a gossip run whose round 1 is a cut round: seeded, then the cut push
  {
    rp::RoundFacts q;
    q.cut = true;
    const rp::RoundPlan p = rp::plan_round(rp::RoundHistory{}, r, g, q);
    CHECK(p.receive == rp::Receive::Seed && p.push == rp::Push::AtomicCut && !p.mid_read);
  }
  // forced push modes do not override it
  for (int mode = 0; mode < 3; ++mode) {
    rp::RoundRules r2 = r;
    r2.push_mode = mode;
    CHECK(rp::plan_round(dense, r2, g, f).push == rp::Push::AtomicCut);
    CHECK(rp::plan_round(dense, r2, g, f).receive == rp::Receive::GossipPull);
  }
  // flood: the cut pull in a cut round, the flood pull in every other round
  rp::RoundCaps fl;
  rp::RoundFacts q;
  q.round = 3;
  CHECK(rp::plan_round(sparse, r, fl, q).receive == rp::Receive::FloodPull);
  q.cut = true;
  CHECK(rp::plan_round(sparse, r, fl, q).receive == rp::Receive::FloodPullCut);
  CHECK(rp::plan_round(sparse, r, fl, q).push == rp::Push::None);
  q.round = 0;
  CHECK(rp::plan_round(sparse, r, fl, q).receive == rp::Receive::Seed);

  // no batch while a round the cut acts on lies at or ahead
  rp::RoundHistory tail;
  tail.saw_dense = true;
  tail.last_new = 10;
  tail.prev2_new = 40;
  tail.prev_sw = 30;
  rp::DecayFacts d;
  d.round = 30;
  d.V = 1000;
  CHECK(rp::decay_batchable(tail, r, g, d));
  d.cut_ahead = true;
  CHECK(!rp::decay_batchable(tail, r, g, d));
}

int main() {
  // the predicate at the edges of the window
  CHECK(!netsplit::link_cut(2, 0, 1, 3, 5) && netsplit::link_cut(3, 0, 1, 3, 5) && netsplit::link_cut(4, 0, 1, 3, 5) &&
        !netsplit::link_cut(5, 0, 1, 3, 5));
  CHECK(!netsplit::link_cut(3, 1, 1, 3, 5) && !netsplit::link_cut(4, 7, 7, 0, 100));
  CHECK(netsplit::link_cut(0, 2, 0, 0, 1) && !netsplit::link_cut(1, 2, 0, 0, 1));
  CHECK(!netsplit::link_cut(3, 0, 1, 5, 3) && !netsplit::link_cut(4, 0, 1, 4, 4));  // empty windows
  CHECK(netsplit::link_cut(0x7FFFFFFE, 0, 1, 0, 0x7FFFFFFF));
  // validation
  CHECK(netsplit::check_window(0, 0) == netsplit::OK && netsplit::check_window(5, 2) == netsplit::OK);
  CHECK(netsplit::check_window(-1, 3) == netsplit::BAD_FROM && netsplit::check_window(INT32_MIN, 3) == netsplit::BAD_FROM);
  CHECK(netsplit::check_window(0, -1) == netsplit::BAD_UNTIL);
  {
    std::vector<int32_t> s = {0, 3, 3, -1, 2, -7};
    CHECK(netsplit::first_bad_side(6, s.data()) == 3);
    s[3] = 0;
    CHECK(netsplit::first_bad_side(6, s.data()) == 5);
    s[5] = 0x7FFFFFFF;
    CHECK(netsplit::first_bad_side(6, s.data()) == -1 && netsplit::first_bad_side(6, nullptr) == -1);
  }
  // the window's questions
  {
    netsplit::Window w;
    CHECK(!w.on() && !w.cut_round(0) && !w.cut_sends(0) && !w.cut_ahead(0));
    w.from = 4;
    w.until = 4;
    CHECK(!w.on() && !w.cut_round(4) && !w.cut_ahead(0));
    w.from = 6;
    w.until = 2;
    CHECK(!w.on() && !w.cut_round(3) && !w.cut_sends(3) && !w.cut_ahead(0));
  }
  for (int32_t from = 0; from < 8; ++from)
    for (int32_t until = 0; until < 10; ++until) {
      netsplit::Window w;
      w.from = from;
      w.until = until;
      bool ahead = false;  // does a cut round, or a round whose sends arrive in one, lie at or after r?
      for (int32_t r = 12; r >= 0; --r) {
        const bool cut = from <= r && r < until;
        const bool sends = from <= r + 1 && r + 1 < until;
        CHECK(w.cut_round(r) == cut);
        CHECK(w.cut_sends(r) == sends);
        CHECK(w.cut_round(r) == netsplit::link_cut(r, 0, 1, from, until));
        ahead = ahead || cut || sends;
        CHECK(w.cut_ahead(r) == ahead);
      }
    }
  // the crossing count against brute force over random graphs and sides
  std::mt19937 rng(2024);
  for (int trial = 0; trial < 200; ++trial) {
    const int V = 1 + (int)(rng() % 60);
    std::set<std::pair<int, int>> E;
    const int ne = (int)(rng() % (3 * V));
    for (int i = 0; i < ne; ++i) {
      const int a = (int)(rng() % V), b = (int)(rng() % V);
      if (a != b) E.insert({a < b ? a : b, a < b ? b : a});
    }
    std::vector<std::vector<int32_t>> adj(V);
    for (auto& e : E) {
      adj[e.first].push_back(e.second);
      adj[e.second].push_back(e.first);
    }
    std::vector<int64_t> rowptr(V + 1, 0);
    std::vector<int32_t> colidx;
    for (int v = 0; v < V; ++v) {
      for (int32_t u : adj[v]) colidx.push_back(u);
      rowptr[v + 1] = (int64_t)colidx.size();
    }
    const int nsides = 1 + (int)(rng() % 4);
    std::vector<int32_t> side(V);
    for (int v = 0; v < V; ++v) side[v] = (int32_t)(rng() % nsides) * 5;
    int64_t want = 0;
    for (auto& e : E) want += side[e.first] != side[e.second];
    CHECK(netsplit::crossing(V, rowptr.data(), colidx.data(), side.data()) == want);
    CHECK(netsplit::crossing(V, rowptr.data(), colidx.data(), nullptr) == 0);
    CHECK(netsplit::any(V, rowptr.data(), colidx.data(), side.data(), 2, 5) == (want > 0));
    CHECK(!netsplit::any(V, rowptr.data(), colidx.data(), side.data(), 5, 5));
    CHECK(!netsplit::any(V, rowptr.data(), colidx.data(), side.data(), 5, 2));
    CHECK(!netsplit::any(V, rowptr.data(), colidx.data(), nullptr, 2, 5));
    std::vector<int32_t> same(V, 9);
    CHECK(!netsplit::any(V, rowptr.data(), colidx.data(), same.data(), 0, 100));
  }
  plans();
  std::printf("ok %ld\n", cases);
  return 0;
}
