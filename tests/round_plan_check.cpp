// Host check of the round schedule (csrc/round_plan.h); built and run by tests/test_round_plan.py.
//
//   round_plan_check TRACE...    prints "replay <rounds> mid_reads <n>" per trace, then "ok <cases>"
//
// A trace file is "W v_conn e_thresh v_thresh update_push_cap n" and n rows of "round new_deliveries
// active_vertices active_words scatter_words push_form" (p2pg_round_stats of a recorded run).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "round_plan.h"

using namespace round_plan;

#define CHECK(x)                                                        \
  do {                                                                  \
    if (!(x)) {                                                         \
      std::fprintf(stderr, "%s:%d: %s\n%s [%d %d %d %d]\n", __FILE__, __LINE__, #x, ctx, at[0], at[1], at[2], at[3]); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

static char ctx[512] = "";
static int at[4] = {0, 0, 0, 0};  // grid position: history, rules, caps, facts
static long cases = 0;

// p2pg_round_stats.push_form (include/p2pgpu.h)
enum { FORM_NONE = 0, FORM_ATOMIC = 1, FORM_EDGE = 2, FORM_FUSED = 3, FORM_UPDATE_EDGE = 4 };

// Replay: every recorded round's counters through plan_round, resolve_push and advance, as
// p2pg_step does; the planned forms must be the recorded ones.
static void replay(const char* path) {
  std::FILE* f = std::fopen(path, "r");
  std::snprintf(ctx, sizeof(ctx), "trace %s", path);
  CHECK(f != nullptr);
  RoundRules r;
  RoundCaps c;
  int up_cap = 0, n = 0;
  CHECK(std::fscanf(f, "%" SCNd32 " %" SCNd64 " %lf %lf %d %d", &r.W, &r.v_conn, &r.e_thresh, &r.v_thresh,
                    &up_cap, &n) == 6);
  c.gossip = c.e_planes = c.fused = c.sparse_scatter = true;
  c.update_push = up_cap != 0;
  RoundHistory h;
  int mid_reads = 0;
  for (int i = 0; i < n; ++i) {
    int round = 0, form = 0;
    RoundCounters k;
    CHECK(std::fscanf(f, "%d %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %d", &round, &k.fresh, &k.av,
                      &k.aw, &k.sw, &form) == 6);
    std::snprintf(ctx, sizeof(ctx), "trace %s round %d", path, round);
    CHECK(round == i);
    RoundFacts facts;
    facts.round = round;
    const RoundPlan p = plan_round(h, r, c, facts);
    CHECK(!p.held && p.store_f == 1);
    CHECK((p.receive == Receive::Seed) == (round == 0));
    const Push push = resolve_push(p, r, k.aw, k.av);
    const int planned = p.receive == Receive::Fused        ? FORM_FUSED
                        : p.receive == Receive::UpdatePush ? FORM_UPDATE_EDGE
                        : push == Push::Edge               ? FORM_EDGE
                                                           : FORM_ATOMIC;
    CHECK(push == Push::Made || push == Push::Edge || push == Push::Atomic);
    CHECK(planned == form);
    // a push sized by the last round's pushed masks holds this round's nonzero words
    if (p.list == PushList::PrevSw) CHECK(k.aw <= h.prev_sw);
    mid_reads += p.mid_read;
    const RoundHistory before = h;
    advance(h, k, planned != FORM_ATOMIC);
    CHECK(h.prev2_aw == before.prev_aw && h.prev2_av == before.prev_av && h.prev2_new == before.last_new);
    CHECK(h.prev_aw == k.aw && h.prev_av == k.av && h.last_new == k.fresh && h.prev_sw == k.sw);
    CHECK(h.last_push_e == (planned != FORM_ATOMIC) && h.saw_dense == (before.saw_dense || h.last_push_e));
    ++cases;
  }
  std::fclose(f);
  std::printf("replay %d mid_reads %d\n", n, mid_reads);
}

static bool is_e(Push p) { return p == Push::Made || p == Push::Edge; }

// Properties of one plan (W = 64, 10 M connected peers, default thresholds).
static void check_plan(const RoundHistory& h, const RoundRules& r, const RoundCaps& c, const RoundFacts& f) {
  const RoundPlan p = plan_round(h, r, c, f);
  const bool special = f.origination || f.expiry || f.policy;
  const bool made = p.receive == Receive::Fused || p.receive == Receive::UpdatePush;
  CHECK((p.receive == Receive::Seed) == (f.round == 0));
  CHECK(made == (p.push == Push::Made));
  CHECK(c.gossip || (p.push == Push::None && p.store_f == 1 && !p.mid_read));
  CHECK(p.store_f == 1 || (made ? p.store_f == 0 : p.store_f == 2));
  if (p.store_f != 1) CHECK(f.skip_frontier && (made ? !c.records : c.partial_rows));
  // a round with an origination, an expiry or a policy: unfused, whole rows
  if (special) CHECK(!made && p.store_f == 1);
  // ... and a gossip round with an expiry or a policy holds its push (nothing read for it)
  CHECK(p.held == (f.expiry || f.policy));
  if (p.held) CHECK(!made && !p.mid_read && p.list == PushList::None);
  // its form once the counters are known, sparse and dense
  const Push sparse = resolve_push(p, r, 1, 1), dense = resolve_push(p, r, 640000000ull, 10000000ull);
  CHECK(sparse == dense || (p.push == Push::ByCounters && sparse == Push::Atomic && dense == Push::Edge));
  if (c.gossip) {
    CHECK(dense != Push::None && dense != Push::ByCounters);
    // the overrides: always row atomics / always edge stores (a partitioned rank only if it can
    // take the dense rounds; an expiry round's held push keeps the row atomics)
    if (r.push_mode == 1) CHECK(sparse == Push::Atomic && dense == Push::Atomic);
    if (r.push_mode == 2 && c.e_planes && (!c.partitioned || c.part_dense) && !f.expiry)
      CHECK(is_e(sparse) && is_e(dense));
    if (!c.e_planes || (c.partitioned && !c.part_dense)) CHECK(made || dense == Push::Atomic);
  }
  if (f.round == 0) CHECK(!p.mid_read);
  if (p.list == PushList::PrevSw) CHECK(h.prev_sw > 0 && !p.mid_read && !special && !c.partitioned);
  if (p.list == PushList::Counters) CHECK(p.mid_read == (f.round > 0));
  if (p.list != PushList::None) CHECK(c.sparse_scatter && p.push != Push::Edge && !made);
  if (p.push == Push::ByCounters && !p.held) CHECK(p.mid_read == (f.round > 0));
  ++cases;
}

// The batched decay tail: what it implies, and that p2pg_step would plan the same round.
static void check_decay(const RoundHistory& h, const RoundRules& r, const RoundCaps& c, const DecayFacts& d) {
  ++cases;
  if (!decay_batchable(h, r, c, d)) return;
  CHECK(h.saw_dense && !h.last_push_e && d.round > 0);
  CHECK(push_dedup(h, r) == (r.push_dedup != 0));  // (what the batch computed on its own before)
  if (r.update_push == 1) return;  // (forced update+push rounds: p2pg_step only)
  RoundFacts f;
  f.round = d.round;
  const RoundPlan p = plan_round(h, r, c, f);
  CHECK(p.receive == Receive::Update && p.push == Push::Atomic && p.list == PushList::PrevSw && !p.mid_read);
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) replay(argv[i]);
  // histories: empty, rising, dense, decaying (config 4's rounds 0, 8, 18 and 30 at W = 64)
  RoundHistory hs[4];
  hs[1] = {7800000, 3300000, 2600000, 1500000, 7900000, 2650000, 23000000, false, false};
  hs[2] = {520000000, 9990000, 470000000, 9980000, 1900000000ull, 1700000000ull, 620000000, true, true};
  hs[3] = {150000, 140000, 420000, 380000, 150000, 420000, 450000, true, false};
  const int modes[3] = {0, 1, 2}, tri[3] = {-1, 0, 1};
  for (int hi = 0; hi < 4; ++hi)
    for (int le = 0; le < 2; ++le) {  // (each history with and without E pushes in its last round)
      RoundHistory h = hs[hi];
      h.last_push_e = le != 0;
      h.saw_dense = h.saw_dense || h.last_push_e;
      for (int ri = 0; ri < 54; ++ri) {
        RoundRules r;
        r.W = 64;
        r.v_conn = 10000000;
        r.push_mode = modes[ri % 3];
        r.update_push = tri[ri / 3 % 3];
        r.push_dedup = tri[ri / 9 % 3];
        r.decay_pred = ri / 27 != 0;
        std::snprintf(ctx, sizeof(ctx), "grid");
        at[0] = 2 * hi + le;
        at[1] = ri;
        at[2] = at[3] = -1;
        // the density rule, one definition: still_dense is it on a history without decay
        if (!(h.last_new < h.prev2_new))
          CHECK(still_dense(h, r) == dense_frontier(r, (double)h.prev_aw, (double)h.prev_av));
        CHECK(!dense_frontier(r, 1.0, 0.0) && dense_frontier(r, 0.07 * 64 * 3.1e6, 3.1e6) &&
              !dense_frontier(r, 0.07 * 64 * 3.1e6, 3.1e6, 1.2) && !dense_frontier(r, 64 * 2.9e6, 2.9e6));
        for (int ci = 0; ci < 512; ++ci) {
          RoundCaps c;
          c.gossip = ci & 1;
          c.e_planes = ci & 2;
          c.partitioned = ci & 4;
          c.part_dense = ci & 8;
          c.fused = ci & 16;
          c.update_push = ci & 32;
          c.sparse_scatter = ci & 64;
          c.partial_rows = ci & 128;
          c.records = ci & 256;
          if (c.part_dense && !c.partitioned) continue;  // (part_dense is a partitioned rank's)
          for (int fi = 0; fi < 128; ++fi) {
            RoundFacts f;
            f.round = fi & 1 ? 3 : 0;
            f.consume_next = fi & 2;
            f.split = fi & 4;
            f.origination = fi & 8;
            f.expiry = fi & 16;
            f.policy = fi & 32;
            f.skip_frontier = fi & 64;
            if (f.policy && f.round == 0) continue;  // (a policy acts on rounds > 0)
            at[2] = ci;
            at[3] = fi;
            check_plan(h, r, c, f);
          }
          for (int di = 0; di < 256; ++di) {
            DecayFacts d;
            d.round = di & 1 ? 30 : 0;
            d.V = 10000000;
            d.consume_next = di & 2;
            d.late_starts = di & 4;
            d.expiry_ahead = di & 8;
            d.frontier_needed = di & 16;
            d.autostop = !(di & 32);
            d.auto_buf = di & 64;
            d.arr_pending = di & 128;
            at[2] = ci;
            at[3] = 1000 + di;
            check_decay(h, r, c, d);
          }
        }
      }
    }
  std::printf("ok %ld\n", cases);
  return 0;
}
