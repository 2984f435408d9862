// The host's round schedule: what a round is, decided before anything is launched.
//
// The engine gathers a round's facts, asks plan_round for its receive pass, its frontier rows and
// its push, and launches what the plan names (p2pg_step); the counters of every finished round
// pass through advance, the one place that rolls the history the next plan reads.  Every rule
// here only picks a launch form or spares a host synchronisation, never a result.
//
// Plain C++: included by engine.cpp and by host programs (tests/test_round_plan.py).
#pragma once
#include <algorithm>
#include <cstdint>

namespace round_plan {

// The counters of finished rounds that the rules read.
struct RoundHistory {
  uint64_t prev_aw = 0, prev_av = 0;  // active words / rows of the previous round
  uint64_t prev2_aw = 0, prev2_av = 0;  // the same, one round earlier
  uint64_t last_new = 0, prev2_new = 0;  // first receipts of the last round run, and the one before
  uint64_t prev_sw = 0;        // distinct masks pushed in the last round (>= the next frontier's
                               // nonzero words: each of them received at least one)
  bool saw_dense = false;      // a round of this run pushed into E (the dense phase has begun)
  bool last_push_e = false;    // gossip: pushes of the previous round went to E (dense)
};

// A finished round's counters (p2pg_round_stats: new_deliveries, active_vertices, active_words,
// scatter_words).
struct RoundCounters {
  uint64_t fresh = 0, av = 0, aw = 0, sw = 0;
};

// The one roll of the history: a round ended with counters c; pushed_e = its pushes went to E.
inline void advance(RoundHistory& h, const RoundCounters& c, bool pushed_e) {
  h.prev2_aw = h.prev_aw;
  h.prev2_av = h.prev_av;
  h.prev2_new = h.last_new;
  h.prev_aw = c.aw;
  h.prev_av = c.av;
  h.last_new = c.fresh;
  h.prev_sw = c.sw;
  h.last_push_e = pushed_e;
  if (pushed_e) h.saw_dense = true;
}

struct RoundRules {
  int32_t W = 0;               // 64-bit words per row
  int64_t v_conn = 0;          // peers with >= 1 connection: the ones a round can make active
                               // (isolated peers do not keep a run sparse)
  double e_thresh = 0.06;      // dense when active words >= e_thresh * active rows * W ...
  double v_thresh = 0.3;       // ... and active rows >= v_thresh * v_conn: a dense round visits every
                               // unsaturated peer, a sparse one only the pushed-to rows (narrow
                               // rows: word density alone is high whenever anything is active)
  int push_mode = 0;           // 0 auto, 1 always row atomics, 2 always edge stores (P2PG_GOSSIP_PUSH)
  int update_push = -1;        // the first dense round after a sparse one: its update and its E
                               // pushes in one pass -- -1 when the round is predicted dense
                               // (predict_dense), 0 never, 1 whenever the rows allow it
                               // (P2PG_UPDATE_PUSH)
  int push_dedup = -1;         // sparse pushes drop seen bits: -1 in the decay phase, 0 never,
                               // 1 always (P2PG_PUSH_DEDUP)
  bool decay_pred = true;      // still_dense shrinks the counters in the decay phase
                               // (P2PG_DECAY_PRED=0: the last round's counters as they are)
};

// What the engine's state and kernels allow, evaluated by the engine once per round.
struct RoundCaps {
  bool gossip = false;         // else flood
  bool e_planes = false;       // edge-mask planes E are allocated
  bool partitioned = false;    // a vertex-partitioned rank (global ids set) ...
  bool part_dense = false;     // ... that can take the dense rounds in their PART form
  bool fused = false;          // gossip_fused_supported
  bool update_push = false;    // gossip_update_push_supported and hub pushes by atomics
  bool sparse_scatter = false;  // row-atomic pushes run lane-parallel (a (peer, word) list)
  bool partial_rows = false;   // updates / the last dense pull may write nonzero words only
  bool records = false;        // hop / parent planes (P2PG_FLAG_RECORD)
};

struct RoundFacts {
  int32_t round = 0;
  bool consume_next = false;   // the round consumes materialized rows
  bool split = false;          // its receive pass runs in two phases (interior, border)
  bool origination = false;    // messages start in it
  bool expiry = false;         // hop limits run out in it
  bool policy = false;         // a relay policy acts on it (every round > 0 of a policy engine)
  bool offline = false;        // somebody is offline in it (p2pg_set_downtime): the receipts its
                               // receive pass made at the offline peers are undone before its push
  bool pull = false;           // the replies of an anti-entropy exchange arrive in it
                               // (p2pg_set_anti_entropy): what they carried joins its first receipts
                               // between the receive pass and the push
  bool cut = false;            // a netsplit acts on it (p2pg_set_netsplit): a flood round > 0 inside
                               // the window receives over cut connections; a gossip round's sends
                               // arrive in a round of the window
  bool skip_frontier = false;  // nobody observes its frontier rows (inside p2pg_run)
};

// FloodPullCut: the flood pull of a cut round (relay_netsplit.hip).
enum class Receive { Seed, Consume, FloodPull, GossipPull, Fused, UpdatePush, Update, FloodPullCut };
// Made: by the receive pass (Fused, UpdatePush).  ByCounters: edge stores or row atomics by the
// density of the round's own frontier (resolve_push).
// AtomicCut: row atomics by the push that leaves out the picks over cut connections.
enum class Push { None, Made, Edge, Atomic, ByCounters, AtomicCut };
// The (peer, word) list of a lane-parallel row-atomic push: sized by the last round's pushed masks
// or by the round's own active words (Counters: they are read first).
enum class PushList { None, PrevSw, Counters };

struct RoundPlan {
  Receive receive = Receive::Update;
  int store_f = 1;             // RoundParams::store_f: 0 no frontier rows, 1 whole, 2 nonzero words
  Push push = Push::None;
  bool held = false;           // the round's sends (a gossip round's push) wait until the boundary
                               // makes them final (finalize_expiry)
  PushList list = PushList::None;
  bool mid_read = false;       // the round's counters are read from the device before its push
};

// The density rule: a frontier of aw nonzero words in av active rows is dense -- pushed by
// whole-row edge-mask stores (and pulled next round) rather than by row atomics.
inline bool dense_frontier(const RoundRules& r, double aw, double av, double margin = 1.0) {
  return av > 0.0 && aw >= margin * r.e_thresh * av * (double)r.W && av >= r.v_thresh * (double)r.v_conn;
}

// Will the pushes of the next round (a round after a sparse one, before its update ran) be dense?
// Rising phase only: active words grow by the last round's factor and inactive peers shrink by
// it, with a 15 % margin on the word test.  On config 4's recorded rounds at 512 / 1024 / 2048 /
// 4096 broadcasts this names exactly the first dense round at W = 32 / 64 and none at W <= 16 (no
// false positive).
inline bool predict_dense(const RoundHistory& h, const RoundRules& r) {
  if (h.prev2_aw == 0 || h.prev2_av == 0 || h.last_new <= h.prev2_new) return false;
  const double V = (double)r.v_conn;
  const double in1 = V - (double)h.prev_av, in2 = V - (double)h.prev2_av;
  if (in2 <= 0.0) return false;
  const double est_av = V - in1 * (in1 / in2);
  const double est_aw = (double)h.prev_aw * ((double)h.prev_aw / (double)h.prev2_aw);
  return dense_frontier(r, est_aw, est_av, 1.15);
}

// Will this round's pushes go by row atomics whatever its counters say?  Then the push is
// launched without reading them first (one host synchronisation per round instead of two): in
// the decay phase (after the dense rounds, receipts shrinking) and while the rising frontier is
// far below the dense-round thresholds (active peers, grown twice by the last growth factor, under
// half of v_thresh * v_conn).
inline bool clearly_sparse(const RoundHistory& h, const RoundRules& r, int32_t round) {
  if (round == 0) return false;  // (origination: the counters are the host's)
  // a bound, not a guess: every active peer of this round received at least one of the masks
  // pushed in the last one (prev_sw), and a dense round needs v_thresh * v_conn active peers
  // (c4: rounds 5 and 6, whose frontiers grow too fast for the guess below)
  if (h.prev_sw > 0 && (double)h.prev_sw < r.v_thresh * (double)r.v_conn) return true;
  if (h.saw_dense) return h.last_new < h.prev2_new;
  if (h.prev_av == 0) return true;  // nothing arrives: an empty round
  const double grow = h.prev2_av ? std::max(1.0, (double)h.prev_av / (double)h.prev2_av) : 64.0;
  return (double)h.prev_av * grow * grow < 0.5 * r.v_thresh * (double)r.v_conn;
}

// A dense round follows a dense round if the frontier it will push is still dense.  The counters
// are those of the round before; in the decay phase (receipts shrinking) they are first shrunk by
// their last factor, so the last dense round is not one round late (c4: round 24's 3.0e7 active
// words are below 0.06 x 8.2e6 peers x 64, while round 23's were above).
inline bool still_dense(const RoundHistory& h, const RoundRules& r) {
  double aw = (double)h.prev_aw, av = (double)h.prev_av;
  if (r.decay_pred && h.saw_dense && h.last_new < h.prev2_new && h.prev2_aw && h.prev2_av) {
    aw *= aw / (double)h.prev2_aw;
    av *= av / (double)h.prev2_av;
  }
  return dense_frontier(r, aw, av);
}

// Does a sparse push drop seen bits before its atomics (RoundParams::dedup_push)?  In the decay
// phase most pushes are duplicates.  The phase is "after the dense rounds" (saw_dense), a fact
// every schedule agrees on -- a batched decay round, a blind push and a round that read its
// counters first must filter alike, because the filter decides which fully-seen masks are still
// pushed, i.e. the touched-words counter of the next round.
inline bool push_dedup(const RoundHistory& h, const RoundRules& r) {
  return r.push_dedup == 1 || (r.push_dedup < 0 && h.saw_dense);
}

// The plan of round f.round.
//
// A round with an origination, an expiry or a policy is special: its frontier rows are read and
// rewritten after the receive pass (k_originate ORs into them; the expire / policy passes and the
// boundary's clearing read and write them), so it takes the unfused schedule with whole rows, and
// it never pushes blind (the last round's pushed masks do not bound words nobody pushed).  A
// gossip round with an expiry or a policy also holds its push back until its sends are final: an
// expiry round's then leaves by row atomics, a pure policy round's in the form its own density
// chose.  An offline round (peer downtime) is special in the same way -- its rows are rewritten
// between the receive pass and the push (relay_offline.hip) -- but not held: the undo is done
// before the push, which leaves in the round, in the form the density rule gives.  The arrival
// round of an anti-entropy exchange is planned like an offline round: k_pull_apply (relay_pull.hip)
// ORs the pulled receipts into the rows before the push, so whole rows, unfused, never blind, not
// held; request and reply rounds launch nothing and are no special rounds.  A round a netsplit acts
// on is special as well.  In a flood it is a cut round, whose receive pass is the cut pull.  In gossip
// it is a round whose sends arrive in a cut round: the loss is decided where the send is made, so it
// receives and pushes in separate passes (never Fused / UpdatePush, no edge stores), keeps whole
// frontier rows and pushes by the cut push (row atomics) at once, without reading its counters: not
// held, no list.  The rounds around a special round keep every form they have.
inline RoundPlan plan_round(const RoundHistory& h, const RoundRules& r, const RoundCaps& c,
                            const RoundFacts& f) {
  RoundPlan p;
  const bool special = f.origination || f.expiry || f.policy || f.offline || f.pull || f.cut;
  // the update / pull-only pass of this round (fused and update+push rounds set their own): a
  // frontier nobody observes is written by its nonzero words only
  if (c.gossip && !special && f.skip_frontier && c.partial_rows) p.store_f = 2;
  // ... and a pass that also pushes does not store it at all
  const int made_store_f = f.skip_frontier && !c.records ? 0 : 1;
  const bool e_ok = c.e_planes && (!c.partitioned || c.part_dense);
  if (f.round == 0) {
    p.receive = Receive::Seed;
  } else if (f.consume_next) {
    p.receive = Receive::Consume;
  } else if (!c.gossip) {
    p.receive = f.cut ? Receive::FloodPullCut : Receive::FloodPull;
  } else if (h.last_push_e) {
    // the previous round stored per-edge masks: gather them (pull, no atomics); if this round is
    // predicted dense as well, the same pass also pushes its receipts
    const bool dense = r.push_mode == 2 || (r.push_mode == 0 && still_dense(h, r));
    const bool fused = !special && (!c.partitioned || c.part_dense) && dense && c.fused;
    p.receive = fused ? Receive::Fused : Receive::GossipPull;
  } else if (!special && r.update_push != 0 && r.push_mode == 0 && !c.partitioned && !f.split &&
             c.e_planes && c.update_push && (r.update_push == 1 || predict_dense(h, r))) {
    p.receive = Receive::UpdatePush;
  } else {
    p.receive = Receive::Update;
  }
  p.held = f.expiry || f.policy;
  if (!c.gossip) return p;
  if (p.receive == Receive::Fused || p.receive == Receive::UpdatePush) {
    p.store_f = made_store_f;
    p.push = Push::Made;
    return p;
  }
  // The counters of this round are needed before its push only to choose the form (unless that
  // choice is clear already) and to size the sparse push's list (else bounded by the last round's
  // pushed masks).  Not on a vertex-partitioned rank: rows other ranks pushed arrive by the
  // exchange, so this rank's own pushed masks bound nothing.
  if (f.cut) {
    p.push = Push::AtomicCut;
    p.held = false;
    return p;
  }
  const bool blind = f.round > 0 && r.push_mode != 2 && !c.partitioned && !special &&
                     clearly_sparse(h, r, f.round) && h.prev_sw > 0;
  if (f.expiry || !e_ok || r.push_mode == 1 || blind)
    p.push = Push::Atomic;
  else
    p.push = r.push_mode == 2 ? Push::Edge : Push::ByCounters;
  if (p.held) return p;  // (a held push is sized when it leaves: finalize_expiry)
  if (p.push != Push::Edge && c.sparse_scatter) p.list = blind ? PushList::PrevSw : PushList::Counters;
  // round 0's counters are the host's (seed_stats): no read-back
  p.mid_read = f.round > 0 && (p.push == Push::ByCounters || p.list == PushList::Counters);
  return p;
}

// The form of a planned push once the round's counters (aw active words in av rows) are known:
// Edge or Atomic.  A dense round by row atomics only would run at the atomic units' rate.
inline Push resolve_push(const RoundPlan& p, const RoundRules& r, uint64_t aw, uint64_t av) {
  if (p.push != Push::ByCounters) return p.push;
  return dense_frontier(r, (double)aw, (double)av) ? Push::Edge : Push::Atomic;
}

// p2pg_run's decay phase: after the dense rounds, while receipts shrink, every round is an update
// of the row pushes and a row-atomic push whose form, list bound (the last round's pushed masks,
// shrinking too) and dedup setting need none of its own counters, so several are enqueued at once.
struct DecayFacts {
  int32_t round = 0;
  int64_t V = 0;
  bool consume_next = false;
  bool late_starts = false;      // some start round is not 0: a batch's list is sized for one wave's
                                 // decay; a younger wave may still be growing under the older ones'
                                 // and outgrow it mid-batch, and an origination round reads its own
                                 // counters before its push
  bool expiry_ahead = false;     // a hop limit expires from here on: its round runs its own schedule
  bool offline_ahead = false;    // somebody is offline in a round from here on (p2pg_set_downtime):
                                 // that round runs its own schedule
  bool pull_ahead = false;       // the replies of an anti-entropy exchange arrive in a round from here
                                 // on (p2pg_set_anti_entropy): that round runs its own schedule
  bool cut_ahead = false;        // a netsplit acts on a round from here on (p2pg_set_netsplit): that
                                 // round runs its own schedule
  bool frontier_needed = false;  // every round's frontier rows are read whole (lost count, tallies,
                                 // relay policy)
  bool autostop = true;
  bool auto_buf = false;         // every round packs its boundary rows (p2pg_set_exchange_buffer)
  bool arr_pending = false;      // arrivals still travel on a graph a topology update replaced
};

inline bool decay_batchable(const RoundHistory& h, const RoundRules& r, const RoundCaps& c,
                            const DecayFacts& f) {
  return f.round > 0 && !f.frontier_needed && c.gossip && h.saw_dense && !h.last_push_e &&
         h.last_new < h.prev2_new && h.prev_sw > 0 && !f.consume_next && !f.arr_pending &&
         !f.late_starts && !f.expiry_ahead && !f.offline_ahead && !f.pull_ahead && !f.cut_ahead && !c.partitioned && f.autostop && r.push_mode != 2 &&
         !f.auto_buf && c.sparse_scatter &&
         h.last_new * 16 < (uint64_t)f.V;  // the tail: small rounds, where the syncs dominate
}

}  // namespace round_plan
