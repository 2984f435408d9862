// Host side of the relay engine: the C-ABI declared in include/p2pgpu.h.
//
// One engine = one GPU = one simulated peer graph resident in HBM.  Per round it launches a
// handful of HIP kernels (relay_kernels.hip) on one stream and copies back 8 shards x 8
// counters; nothing else crosses PCIe inside a run.
//
// Round schedule (r = round index; pushes made in round r arrive in round r+1):
//   r = 0          seed: F[0], seen, A[0] <- source bits    (Node.send_to_nodes at the origin,
//                                                            p2pnetwork/node.py:106-112)
//   flood  r >= 1  pull:   F[r&1], A[r&1], seen <- OR of active neighbours' F[(r-1)&1]
//   gossip r >= 1  update: F[r&1], A[r&1], seen <- next[r&1] & ~seen  (T[r&1] = touched rows)
//   gossip r >= 0  scatter: next[(r+1)&1], T[(r+1)&1] |= k Philox picks of every F[r&1] bit
//                  (sparse rounds), or E[r&1] per-connection masks (dense rounds; the next
//                  round pulls them; a dense round after a dense round runs pull + scatter
//                  as one fused pass, k_gossip_fused)
//   r >= 1         originate: F[r&1], seen, A[r&1] |= the bits of the messages whose start round
//                  is r, after the receive pass (relay_originate.hip); such a gossip round is
//                  never fused: update / pull, originate, then the separate scatter
//   record         hop/parent planes for the bits of F[r&1]   (P2PG_FLAG_RECORD only)
//   expire         a round in which hop limits run out (p2pg_set_ttl; relay_expire.hip) runs the
//                  unfused schedule too; after record and the tally count the relays of its
//                  expired first receipts leave its counters, and when its sends become final (the
//                  next round's start or a boundary call) their frontier bits are cleared -- then,
//                  gossip, its held-back push leaves by row atomics
//   policy         with a relay policy (p2pg_set_relay_policy; relay_policy.hip) every round > 0 is
//                  scheduled like an expiry round: the muted first receipts' relays leave its
//                  counters, their frontier bits are cleared when its sends become final, and the
//                  held-back gossip push then takes the form the round's own density chose
//   downtime       with peer downtime (p2pg_set_downtime; relay_offline.hip, downtime.h) a round in
//                  which somebody is offline takes the unfused schedule: the receipts its receive
//                  pass made at the offline peers are undone right after that pass, and its push
//                  leaves in the round.  Sends to a peer that is offline in the next round are lost
//   anti-entropy   with periodic pull repair (p2pg_set_anti_entropy; relay_pull.hip, anti_entropy.h)
//                  the round in which an exchange's replies arrive takes the unfused schedule too:
//                  the reply plane is gathered before its receive pass, and what the replies carried
//                  and no relay copy delivered joins its first receipts after that pass.  Request
//                  and reply rounds launch nothing
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/p2pgpu.h"
#include "anti_entropy.h"
#include "downtime.h"
#include "netsplit.h"
#include "internal.h"
#include "latency.h"
#include "philox.h"
#include "round_plan.h"

using namespace p2pg;
namespace rp = round_plan;

// round 0's counters (seed_stats)
struct SeedStats {
  bool ok = false;
  uint64_t nw = 0, relays = 0, av = 0, aw = 0, wedge = 0, degact = 0;
};

struct p2pg_engine {
  p2pg_config cfg{};
  std::string err;
  int64_t V = 0, nnz = 0;
  int32_t M = 0, W = 0;
  std::vector<int64_t> h_rowptr;
  std::vector<int32_t> h_colidx;  // host copy of the adjacency (topology updates, snapshots)
  std::vector<int32_t> h_src;
  // device
  int64_t* d_rowptr = nullptr;
  int32_t* d_colidx = nullptr;
  int64_t* d_hub = nullptr;
  int64_t n_hub = 0;
  int64_t* d_hub_big = nullptr;  // the chunk items of sources with deg > HUB_T (fused rounds)
  int64_t n_hub_big = 0;
  int32_t* d_wide_big = nullptr;  // sources with deg > HUB_T (fused rounds' hub pushes)
  int64_t n_wide_big = 0;
  uint32_t* d_rev = nullptr;   // gossip: reverse edge slots
  // pull hub split (deg > HUB_T)
  uint32_t* d_H = nullptr;
  int64_t* d_hub_items = nullptr;
  int32_t* d_hubs = nullptr;
  int64_t* d_hub_begin = nullptr;
  uint64_t* d_partial = nullptr;
  HubPlan hp{};
  // vertex-partitioned runs
  int32_t* d_gid = nullptr;
  std::vector<int32_t> h_gid;
  int32_t* d_gdeg = nullptr;          // ghost senders' global degrees (p2pg_set_ghost_senders)
  int32_t* d_gpos = nullptr;          // per local slot: position in the ghost neighbour's row
  int32_t* d_send = nullptr;
  int32_t* d_recv = nullptr;
  int64_t n_send = 0, n_recv = 0;
  uint32_t* d_border = nullptr;       // owned peers with a ghost neighbour (phase 1 of a round)
  std::vector<int64_t> send_seg, recv_seg;  // list offsets per rank (p2pg_set_exchange_segments)
  int64_t* d_send_seg = nullptr;
  int64_t* d_recv_seg = nullptr;
  unsigned long long* d_seg_cnt = nullptr;  // live rows per destination (pack_live)
  unsigned long long* h_seg_cnt = nullptr;  // pinned
  // p2pg_set_exchange_buffer: every round packs its live rows of this plane into this buffer
  // right after its kernels, and the counts come back with the round counters (one host
  // synchronisation per round); pack_live then only hands them over
  void* auto_buf = nullptr;
  int32_t auto_plane = -1;
  int32_t auto_round = -1;           // the round whose records auto_buf / auto_cnt hold
  int64_t auto_cnt[P2PG_MAX_RANKS] = {0};  // their counts per destination (h_seg_cnt is reused
                                           // by explicit packs of the other plane)
  bool begun = false;                 // p2pg_step_begin ran this round's phase 0
  // the round schedule (round_plan.h): the rolling counters of the finished rounds and the rules
  // (row width and thresholds: alloc_state; v_conn: p2pg_load_csr; the switches: p2pg_create)
  rp::RoundHistory hist;
  rp::RoundRules rules;
  double e_thresh_env = -1.0;  // P2PG_E_THRESH (>= 0) or by the current row width (alloc_state)
                               // (c4 A/B, interleaved runs: 0.04 320.4 ms vs 0.1 324.3 ms, round 1;
                               // with the lane-parallel sparse push (round 2) W = 64: 0.04 / 0.06 /
                               // 0.08 -> 278.4 / 275.5 / 275.2 ms, W = 8: 89.1 / 89.4 / 89.5 ms)
  double v_thresh_env = -1.0;  // P2PG_V_THRESH, likewise
  bool fused = true;           // dense rounds after dense rounds: one pull+scatter pass
  bool wide_atomic = true;     // fused rounds: hub pushes by atomics (P2PG_WIDE_ATOMIC=0: one
                               // wave per 16-connection chunk item)
  bool sparse_lp = true;       // sparse rounds: lane-parallel scatter (relay_sparse.hip) when
                               // the rows allow it; P2PG_SPARSE_LP=0 keeps the per-source one
  bool skip_frontier = false;  // p2pg_run, not its last two allowed rounds: fused rounds may skip F
  bool partial_f = true;       // ... and updates / the last dense pull write its nonzero words
                               // only (P2PG_PARTIAL_F=0: whole rows, A/B)
  bool frontier_kept = true;   // F[(round-1)&1] holds the last round's first receipts
  bool frontier_kept_prev = true;  // ... and F[round&1] the round before (delivery parents)
  int32_t* d_src = nullptr;
  DevState st{};
  size_t plane_bytes = 0, bm_bytes = 0;
  unsigned long long* h_stats = nullptr;  // pinned
  // The round counters accumulate on the device across rounds (no per-round clearing launch): a
  // round's counters are the difference to stats_base, the copy read at the end of the round
  // before.  stats_clear: the device counters must be zeroed first (new state, reset, restore, or
  // an out-of-round launch that counted: a topology update's re-push, a snapshot's materialize)
  unsigned long long stats_base[STAT_N * STAT_SHARDS] = {0};
  bool stats_clear = true;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  hipEvent_t ev_sync = nullptr;  // round_sync's marker (no timing)
  bool spin = false;             // round_sync polls the marker instead of blocking (P2PG_SPIN)
  // per-launch timing events: recorded around each launch, resolved after the round's stream
  // sync (no extra host synchronisation inside a round)
  std::vector<hipEvent_t> ev_pool;
  std::vector<int> ev_cls;  // class of pending pair i (events 2i, 2i+1)
  uint32_t timed_mask = (1u << P2PG_KCLASS_N) - 1u;  // classes whose launches get events
  double kms[P2PG_KCLASS_N] = {0};
  int64_t klaunch[P2PG_KCLASS_N] = {0};
  int32_t round = 0;
  bool done = false;
  bool have_state = false;
  std::string failed;           // non-empty: the device state is inconsistent (a batched round's
                                // push list overflowed); every step / run refuses until a reset
  // after a topology update: the graph the in-flight messages were sent on and its removed
  // slots, kept for the parents (record / deliveries) of the round that receives them
  int64_t* d_rowptr_arr = nullptr;
  int32_t* d_colidx_arr = nullptr;
  uint8_t* d_gone = nullptr;
  int32_t arr_round = -1;       // the round whose arrivals travelled on that graph
  bool consume_next = false;    // the next round consumes materialized rows (update kernel)
  uint64_t total_relays = 0;    // relays since the last reset (= sum of message_count_send)
  // sparse-round scatter (relay_sparse.hip): the (peer, word) list of a frontier; its fill
  // count lives in the stats buffer, slot STAT_COUNT
  uint64_t* d_wlist = nullptr;
  int64_t wlist_cap = 0;
  uint8_t* d_touched = nullptr;  // one byte per peer (V rounded up to 32), zero between launches
  uint32_t* d_chunk_cnt = nullptr;  // per list chunk: pairs, and their offsets
  uint64_t* d_chunk_off = nullptr;
  bool wlist_check = false;     // a sparse scatter ran this round: check its count after it
  // p2pg_run's decay-phase batches: round counters of up to BATCH_MAX rounds (one slot each)
  unsigned long long* d_bstats = nullptr;
  unsigned long long* h_bstats = nullptr;  // pinned
  int batch_rounds = -1;        // P2PG_RUN_BATCH (rounds per host synchronisation in the decay
                                // phase; 1 = none), -1 = the default
  // Double-buffered seen plane: a reset swaps in the spare (zeroed earlier) and zeroes the plane
  // it replaces on a side stream, behind the work already queued -- the zeroing overlaps the next
  // run's first rounds (latency-bound sparse rounds) instead of leading it.  P2PG_SEEN_SPARE=0,
  // a plane above 1/16 of the device or a failed allocation: the reset zeroes seen in stream
  // order (spare_ready).
  bool seen_spare_on = true;    // P2PG_SEEN_SPARE (for good)
  bool seen_spare_off = false;  // the current plane size / free memory ruled it out (re-examined
                                // when the state is allocated again, alloc_state)
  uint64_t* seen_spare = nullptr;
  bool spare_pending = false;   // a zeroing of seen_spare is queued on `side` (ev_spare marks it)
  hipStream_t side = nullptr;
  hipEvent_t ev_spare = nullptr, ev_main = nullptr;
  SeedStats seed;               // round 0's counters (seed_stats), valid for these sources / rows
  // the arrivals of the next round (p2pg_round_stats.received): the last round's sends
  // (send_to_node calls, less the relays p2pg_drop_relays withdrew) and how many of them are
  // lost -- to churn (counted after every round of a churn run: cnt_lost) or to a connection a
  // topology update removed (counted by p2pg_update_edges)
  uint64_t sent_last = 0, lost_last = 0;
  unsigned long long* d_cnt2 = nullptr;  // k_sends counters [2] (device) / pinned copy
  unsigned long long* h_cnt2 = nullptr;
  // run tallies (P2PG_FLAG_TALLY; relay_tally.hip): per message reach / hop_sum [M] and last_hop
  // [M], per peer sent / received [V], and the column count's shard scratch
  unsigned long long* d_treach = nullptr;
  unsigned long long* d_thop = nullptr;
  int32_t* d_tlast = nullptr;
  unsigned long long* d_tsent = nullptr;
  unsigned long long* d_trecv = nullptr;
  unsigned long long* d_tscratch = nullptr;
  // per-message cost (P2PG_FLAG_MSG_COST; k_msg_cost): sent / received [M] and its shard scratch
  unsigned long long* d_csent = nullptr;
  unsigned long long* d_crecv = nullptr;
  unsigned long long* d_cscratch = nullptr;
  // delivery latency (P2PG_FLAG_LATENCY; relay_latency.hip): per message the histogram of relative
  // hops [M][lat_bins], per peer hop sum / receipts / largest hop [V]; the device copy of h_start
  // [M] and its bit-sliced planes [lat_B][W] (latency.h), kept equal to h_start wherever it changes
  // (upload_latency).  The frontier count's shards are d_tscratch, shared with the tallies.
  int32_t lat_bins = latency::BINS_DEFAULT;
  unsigned long long* d_lhist = nullptr;
  PeerLat* d_lpeer = nullptr;
  int32_t* d_lstart = nullptr;
  uint64_t* d_lplanes = nullptr;
  int32_t lat_B = 0;            // planes in use (0: every start is 0)
  int64_t lat_planes_cap = 0;   // words allocated at d_lplanes
  int32_t tally_pending = -1;   // the round whose sends the peer / cost counters do not hold yet: they
                                // are final (drops, removed connections) only at the next round's
                                // start, in p2pg_update_edges or when the counters are read
  int32_t tally_read_at = -1;   // e->round when p2pg_peer_counters / p2pg_message_cost took the
                                // pending round in
  // Start rounds (p2pg_set_sources_at / p2pg_originate): h_start[m] = the round message m
  // originates in at h_src[m] (0: round 0's seed; -1 with h_src[m] = -1: unscheduled).  The
  // messages that start after round 0 are kept on the device sorted by (round, peer, msg) and cut
  // into groups of one (round, peer) each (k_originate: one wave per group); sched_rounds holds
  // the group range of every round that has any.  Uploaded when the schedule changes, not per round.
  struct SchedRound {
    int32_t round;
    int64_t g_lo, g_hi;  // its groups
  };
  std::vector<int32_t> h_start;
  std::vector<SchedRound> sched_rounds;  // ascending rounds
  int32_t last_start = 0;        // the latest scheduled start round (0: nothing starts late)
  bool late = false;             // some start is not 0 (a late or an unscheduled message)
  int32_t* d_sched_peer = nullptr;
  int32_t* d_sched_msg = nullptr;
  int64_t* d_sched_grp = nullptr;
  // Hop limits (p2pg_set_ttl): h_ttl[m] >= 0, or -1 = unlimited (empty: none set).  A scheduled
  // message expires in round start[m] + ttl[m]; exp_rounds holds those rounds, ascending, and d_exp
  // two W-word masks per round i (relay_expire.hip): X at (2 i) W, Z at (2 i + 1) W.  Uploaded
  // when the limits or the schedule change, not per round.
  std::vector<int32_t> h_ttl;
  bool ttl_on = false;           // some hop limit is finite
  std::vector<int32_t> exp_rounds;
  uint64_t* d_exp = nullptr;
  int32_t exp_pending = -1;      // the expiry round whose sends are not final yet: its expired
                                 // frontier bits still stand (they serve its delivery stream) and
                                 // its gossip push is held back (finalize_expiry)
  int32_t exp_final = -1;        // the last expiry or policy round whose frontier bits were cleared
  // Relay policy (p2pg_set_relay_policy): h_thr[v] = peer v's mute threshold (empty: no policy),
  // d_thr its device copy, uploaded once.  The policy belongs to the peers: it lives and dies with
  // the graph (p2pg_load_csr), not with the sources.  pex_rounds holds the rounds > 0 with an
  // origination or an expiry, ascending, and d_pex one W-word mask per such round of the messages
  // the policy leaves alone in it (relay_policy.hip); uploaded when the schedule, the hop limits
  // or the policy change, not per round.
  std::vector<uint32_t> h_thr;
  uint32_t* d_thr = nullptr;
  uint64_t pol_seed = 0;
  bool pol_on = false;
  std::vector<int32_t> pex_rounds;
  uint64_t* d_pex = nullptr;
  int32_t pol_pending = -1;      // the policy round whose sends are not final yet (finalize_expiry)
  bool held_push_e = false;      // the pending round's held-back gossip push leaves by edge stores
                                 // (rp::resolve_push at its end), not by row atomics
  // Peer downtime (p2pg_set_downtime): peer v is offline in the rounds [h_down_from[v],
  // h_down_until[v]) (empty: no downtime), d_down_from / d_down_until the device copies, uploaded
  // once by the call.  Like the policy it belongs to the peers and lives and dies with the graph.
  // down_sweep answers which rounds are offline rounds (downtime.h).
  std::vector<int32_t> h_down_from, h_down_until;
  int32_t* d_down_from = nullptr;
  int32_t* d_down_until = nullptr;
  bool down_on = false;
  downtime::Sweep down_sweep;
  // Network partition (p2pg_set_netsplit): peer v is on side d_side[v] (uploaded once by the call);
  // the connections between sides are cut in the rounds of ns_win (empty: no netsplit).
  int32_t* d_side = nullptr;
  netsplit::Window ns_win;
  // Anti-entropy (p2pg_set_anti_entropy; anti_entropy.h, relay_pull.hip): the request rounds and
  // the partner draw's key.  The reply plane, its bitmap and the exchange's counter shards exist
  // only while it is set (with a state: they are sized by W).  pull_round = the arrival round the
  // plane belongs to (-1: none yet); pull_log = the exchanges completed in this run.
  anti_entropy::Setting ae;
  uint64_t ae_seed = 0;
  uint64_t* d_pull_R = nullptr;
  uint32_t* d_pull_PB = nullptr;
  unsigned long long* d_pull_cnt = nullptr;
  unsigned long long* h_pull_cnt = nullptr;  // pinned, [STAT_SHARDS][PULL_N]
  int32_t pull_round = -1;
  std::vector<p2pg_pull_stats> pull_log;
};

namespace {

// stats buffer: STAT_N x STAT_SHARDS round counters, then the sparse scatter's list count
constexpr int STAT_COUNT = STAT_N * STAT_SHARDS;
constexpr size_t STAT_BYTES = sizeof(unsigned long long) * (STAT_COUNT + 1);

int fail(p2pg_engine* e, int code, const std::string& msg) {
  if (e) e->err = msg;
  set_global_error(msg);
  return code;
}

#define HIPCHK(e, x)                                                                     \
  do {                                                                                   \
    hipError_t _r = (x);                                                                 \
    if (_r != hipSuccess)                                                                \
      return fail(e, P2PG_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(_r));      \
  } while (0)

template <class T>
void dfree(T*& p) {
  if (p) (void)hipFree(p);
  p = nullptr;
}

// Anti-entropy: the reply plane, its bitmap and the counter shards (allocated at the first arrival
// round: ensure_pull), and what the run recorded.
void free_pull(p2pg_engine* e) {
  dfree(e->d_pull_R);
  dfree(e->d_pull_PB);
  dfree(e->d_pull_cnt);
  if (e->h_pull_cnt) (void)hipHostFree(e->h_pull_cnt);
  e->h_pull_cnt = nullptr;
  e->pull_round = -1;
  e->pull_log.clear();
}

void free_state(p2pg_engine* e) {
  dfree(e->d_cnt2);
  if (e->h_cnt2) (void)hipHostFree(e->h_cnt2);
  e->h_cnt2 = nullptr;
  dfree(e->d_treach);
  dfree(e->d_thop);
  dfree(e->d_tlast);
  dfree(e->d_tsent);
  dfree(e->d_trecv);
  dfree(e->d_tscratch);
  dfree(e->d_csent);
  dfree(e->d_crecv);
  dfree(e->d_cscratch);
  dfree(e->d_lhist);
  dfree(e->d_lpeer);
  dfree(e->d_lstart);
  dfree(e->d_lplanes);
  e->lat_planes_cap = 0;
  e->lat_B = 0;
  DevState& s = e->st;
  dfree(s.seen);
  if (e->seen_spare) {
    if (e->spare_pending) (void)hipStreamSynchronize(e->side);
    dfree(e->seen_spare);
  }
  e->spare_pending = false;
  for (int i = 0; i < 2; ++i) {
    dfree(s.F[i]);
    dfree(s.next[i]);
    dfree(s.A[i]);
    dfree(s.T[i]);
  }
  dfree(s.S);
  dfree(s.hop);
  dfree(s.parent);
  if (s.E[1] == s.E[0]) s.E[1] = nullptr;
  for (int i = 0; i < 2; ++i) dfree(s.E[i]);
  for (int i = 0; i < 2; ++i) dfree(s.AW[i]);
  dfree(s.stats);
  dfree(e->d_wlist);
  e->wlist_cap = 0;
  dfree(e->d_touched);
  dfree(e->d_chunk_cnt);
  dfree(e->d_chunk_off);
#ifdef P2PG_PROF
  if (s.prof) {
    unsigned long long h[16];
    if (hipMemcpy(h, s.prof, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess) {
      fprintf(stderr, "P2PG_PROF");
      for (int i = 0; i < 16; ++i) fprintf(stderr, " %llu", h[i]);
      fprintf(stderr, "\n");
    }
  }
  dfree(s.prof);
#endif
  dfree(e->d_src);
  dfree(e->d_sched_peer);
  dfree(e->d_sched_msg);
  dfree(e->d_sched_grp);
  e->sched_rounds.clear();
  e->late = false;
  e->last_start = 0;
  dfree(e->d_exp);
  e->exp_rounds.clear();
  e->h_ttl.clear();
  e->ttl_on = false;
  e->exp_pending = e->exp_final = -1;
  dfree(e->d_pex);  // (the policy itself stays with the graph: free_graph)
  e->pex_rounds.clear();
  e->pol_pending = -1;
  free_pull(e);  // (sized by W; the setting itself stays with the graph: free_graph)
  e->have_state = false;
}

void free_arr(p2pg_engine* e) {
  dfree(e->d_rowptr_arr);
  dfree(e->d_colidx_arr);
  dfree(e->d_gone);
  e->arr_round = -1;
}

// the topology arrays only (rows, reverse slots, hub lists / plans)
void free_topology(p2pg_engine* e) {
  dfree(e->d_rowptr);
  dfree(e->d_colidx);
  dfree(e->d_hub);
  dfree(e->d_hub_big);
  dfree(e->d_wide_big);
  dfree(e->d_rev);
  dfree(e->d_H);
  dfree(e->d_hub_items);
  dfree(e->d_hubs);
  dfree(e->d_hub_begin);
  dfree(e->d_partial);
  e->hp = HubPlan{};
  e->n_hub = 0;
  e->n_hub_big = 0;
  e->n_wide_big = 0;
}

void free_graph(p2pg_engine* e) {
  free_arr(e);
  dfree(e->d_rowptr);
  dfree(e->d_colidx);
  dfree(e->d_hub);
  dfree(e->d_hub_big);
  dfree(e->d_wide_big);
  dfree(e->d_rev);
  dfree(e->d_H);
  dfree(e->d_hub_items);
  dfree(e->d_hubs);
  dfree(e->d_hub_begin);
  dfree(e->d_partial);
  dfree(e->d_gid);
  dfree(e->d_gdeg);
  dfree(e->d_gpos);
  dfree(e->d_send);
  dfree(e->d_recv);
  dfree(e->d_border);
  dfree(e->d_send_seg);
  dfree(e->d_recv_seg);
  dfree(e->d_seg_cnt);
  dfree(e->d_thr);
  e->h_thr.clear();
  e->pol_on = false;
  dfree(e->d_down_from);
  dfree(e->d_down_until);
  e->h_down_from.clear();
  e->h_down_until.clear();
  e->down_sweep.build(0, nullptr, nullptr);
  e->down_on = false;
  dfree(e->d_side);
  e->ns_win = netsplit::Window{};
  free_pull(e);
  e->ae = anti_entropy::Setting{};
  e->ae_seed = 0;
  if (e->h_seg_cnt) (void)hipHostFree(e->h_seg_cnt);
  e->h_seg_cnt = nullptr;
  e->auto_buf = nullptr;
  e->auto_plane = e->auto_round = -1;
  e->send_seg.clear();
  e->recv_seg.clear();
  e->h_gid.clear();
  e->n_send = e->n_recv = 0;
  e->hp = HubPlan{};
  e->n_hub = 0;
  e->n_hub_big = 0;
  e->n_wide_big = 0;
}

RoundParams params(const p2pg_engine* e) {
  RoundParams p{};
  p.round = e->round;
  p.mode = e->cfg.mode;
  p.fanout = e->cfg.fanout;
  p.msg_base = e->cfg.msg_id_base;
  p.gseed_lo = (uint32_t)e->cfg.gossip_seed;
  p.gseed_hi = (uint32_t)(e->cfg.gossip_seed >> 32);
  p.churn_thr = e->cfg.churn_threshold;
  p.cseed_lo = (uint32_t)e->cfg.churn_seed;
  p.cseed_hi = (uint32_t)(e->cfg.churn_seed >> 32);
  p.border = nullptr;
  p.phase = -1;
  p.store_f = 1;
  p.dedup_push = 0;
  return p;
}

DevGraph graph(const p2pg_engine* e) {
  return DevGraph{e->d_rowptr, e->d_colidx, e->d_rev, e->d_H, e->d_gid, nullptr, e->V,
                  e->d_gdeg, e->d_gpos};
}

// The graph round r's arrivals travelled on: the pre-update graph (with its removed slots) for
// the round right after a topology update, else the current one.
DevGraph graph_for_arrivals(const p2pg_engine* e, int32_t r) {
  if (r == e->arr_round && e->d_rowptr_arr)
    return DevGraph{e->d_rowptr_arr, e->d_colidx_arr, nullptr, nullptr, e->d_gid, e->d_gone, e->V,
                    nullptr, nullptr};
  return graph(e);
}

// The host's wait for a round's counters (everything enqueued on the engine's stream so far):
// a blocking stream synchronisation, or -- P2PG_SPIN -- a marker event polled in a loop, which
// trades a spinning host thread for the wake-up latency of a blocking wait (the GPU idles
// between a round's counter copy and the next round's first launch for as long as the host takes
// to notice).
hipError_t round_sync(p2pg_engine* e) {
  if (!e->spin) return hipStreamSynchronize(e->stream);
  hipError_t r = hipEventRecord(e->ev_sync, e->stream);
  if (r != hipSuccess) return r;
  while ((r = hipEventQuery(e->ev_sync)) == hipErrorNotReady) {
  }
  return r;
}

// Timed launch: kernel class cls in [0, P2PG_KCLASS_N) (see include/p2pgpu.h).
template <class F>
int timed(p2pg_engine* e, int cls, F&& launch) {
  const bool timing = (e->cfg.flags & P2PG_FLAG_TIMING) != 0 && ((e->timed_mask >> cls) & 1u);
  size_t slot = 0;
  if (timing) {
    slot = e->ev_cls.size();
    while (e->ev_pool.size() < 2 * (slot + 1)) {
      hipEvent_t ev;
      HIPCHK(e, hipEventCreate(&ev));
      e->ev_pool.push_back(ev);
    }
    HIPCHK(e, hipEventRecord(e->ev_pool[2 * slot], e->stream));
  }
  hipError_t r = launch();
  if (r != hipSuccess) return fail(e, P2PG_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(r));
  if (timing) {
    HIPCHK(e, hipEventRecord(e->ev_pool[2 * slot + 1], e->stream));
    e->ev_cls.push_back(cls);
  }
  e->klaunch[cls] += 1;
  return P2PG_OK;
}

// After a stream sync: fold the pending launch timings into the per-class sums.
int resolve_timings(p2pg_engine* e) {
  for (size_t i = 0; i < e->ev_cls.size(); ++i) {
    float ms = 0.f;
    HIPCHK(e, hipEventElapsedTime(&ms, e->ev_pool[2 * i], e->ev_pool[2 * i + 1]));
    e->kms[e->ev_cls[i]] += ms;
  }
  e->ev_cls.clear();
  return P2PG_OK;
}

// Can round p's row-atomic push run lane-parallel (relay_sparse.hip)?
bool sparse_scatter_on(const p2pg_engine* e) {
  return e->sparse_lp && gossip_scatter_sparse_supported(e->st);
}

// Buffers of the lane-parallel pushes, grown on demand: a (peer, word) list of >= need entries,
// its chunk counts / offsets, the touched bytes.  Its fill count goes to the stats slot
// STAT_COUNT and is checked after the round (check_scatter_list).
hipError_t sparse_bufs(p2pg_engine* e, int64_t need, SparseBufs& b) {
  need = need > 0 ? need : 1;
  if (need > e->wlist_cap) {
    dfree(e->d_wlist);
    e->wlist_cap = 0;
    const int64_t cap = need + need / 4 + 4096;  // grows by steps, not per round
    hipError_t r = hipMalloc((void**)&e->d_wlist, sizeof(uint64_t) * (size_t)cap);
    if (r != hipSuccess) return r;
    e->wlist_cap = cap;
  }
  if (!e->d_touched) {
    const size_t tb = (size_t)((e->V + 31) >> 5) << 5;
    const size_t nc = ((size_t)sparse_chunks(e->V) + 8) & ~(size_t)7;  // 16 B loads
    hipError_t r = hipMalloc((void**)&e->d_touched, tb ? tb : 32);
    if (r == hipSuccess) r = hipMemsetAsync(e->d_touched, 0, tb ? tb : 32, e->stream);
    if (r == hipSuccess) r = hipMalloc((void**)&e->d_chunk_cnt, sizeof(uint32_t) * nc);
    if (r == hipSuccess) r = hipMalloc((void**)&e->d_chunk_off, sizeof(uint64_t) * nc);
    if (r != hipSuccess) return r;
  }
  e->wlist_check = true;
  b = SparseBufs{e->d_wlist, e->wlist_cap, e->st.stats + STAT_COUNT, e->d_chunk_cnt,
                 e->d_chunk_off, e->d_touched};
  return hipSuccess;
}

// Row-atomic push of the frontier of round p.round over g: lane-parallel when the rows allow it
// (n_words = that frontier's nonzero words, which sizes the (peer, word) list), else per source.
hipError_t launch_scatter_atomic(p2pg_engine* e, const DevGraph& g, const RoundParams& p,
                                 uint64_t n_words) {
  DevState& s = e->st;
  if (!sparse_scatter_on(e))
    return launch_gossip_scatter(g, s, p, e->d_hub, e->n_hub, false, e->stream);
  SparseBufs b;
  hipError_t r = sparse_bufs(e, (int64_t)n_words, b);
  if (r != hipSuccess) return r;
  return launch_gossip_scatter_sparse(g, s, p, (int64_t)n_words, b, e->stream);
}

// Can the fused rounds' hub pushes run by atomics (launch_wide_push_e)?
bool wide_atomic_on(const p2pg_engine* e) {
  return e->wide_atomic && e->W <= 64 && (e->W <= PACK_W_MAX_PLAIN || e->st.AW[0]);
}

// May a round inside p2pg_run (not its last two allowed rounds) write only the nonzero words of its
// frontier rows in its update / last dense pull (RoundParams::store_f == 2)?  No hop/parent records,
// packed rows only (16 < W <= 64: AW planes, one peer per wave), not on a partitioned rank.  A
// whole 512 B row write per active peer was ~40 % of the sparse update's bytes; the words are
// read back only through the AW mask (sparse push list, push-only pass, per-source scatter).
bool partial_rows(const p2pg_engine* e) {
  return !e->st.hop && e->st.AW[0] && e->W > GROUPED_W_MAX && e->W <= 64 && !e->d_gid && e->partial_f;
}

// A fused dense round (pull of E[(r-1)&1] + pushes into E[r&1]) and its hub pushes.
hipError_t launch_fused_round(p2pg_engine* e, const DevGraph& g, const RoundParams& p) {
  DevState& s = e->st;
  if (e->d_gid) {  // the exchanged row pushes it ORed in are cleared after the pass
    hipError_t r = launch_gossip_fused(g, s, p, e->hp, nullptr, 0, true, e->stream);
    return r != hipSuccess ? r : launch_clear_arrivals(s, p.round, e->V, e->stream);
  }
  const bool wa = wide_atomic_on(e);
  hipError_t r = launch_gossip_fused(g, s, p, e->hp, e->d_hub_big, e->n_hub_big, wa, e->stream);
  if (r != hipSuccess || !wa) return r;
  return launch_wide_push_e(g, s, p, e->d_hub_big, e->n_hub_big, e->d_wide_big, e->n_wide_big,
                            e->stream);
}

// Can this vertex-partitioned rank (global ids set) take the dense rounds (E pushes, fused and
// pull-only passes in their PART form, relay_kernels.hip)?  Packed rows over 16 < W <= 64 and
// two E planes; otherwise its gossip pushes go by row atomics only.
bool part_dense(const p2pg_engine* e) {
  const DevState& s = e->st;
  return e->d_gid && e->d_rev && s.E[0] && s.E[1] && s.E[0] != s.E[1] && s.AW[0] &&
         e->W > GROUPED_W_MAX && e->W <= 64;
}

// What this engine's state and kernels allow a round (round_plan.h), evaluated once per round.
rp::RoundCaps round_caps(const p2pg_engine* e) {
  rp::RoundCaps c;
  c.gossip = e->cfg.mode == P2PG_MODE_GOSSIP;
  c.e_planes = e->st.E[0] != nullptr;
  c.partitioned = e->d_gid != nullptr;
  c.part_dense = part_dense(e);
  c.fused = gossip_fused_supported(e->st);
  c.update_push = gossip_update_push_supported(e->st) && wide_atomic_on(e);
  c.sparse_scatter = sparse_scatter_on(e);
  c.partial_rows = partial_rows(e);
  c.records = e->st.hop != nullptr;
  return c;
}

// After the stream synced on a round whose push ran lane-parallel: the list must have held
// every (peer, word) pair (n_words is the frontier's own count, so a shortfall is a bug).
int check_scatter_list(p2pg_engine* e, unsigned long long listed) {
  if (!e->wlist_check) return P2PG_OK;
  e->wlist_check = false;
  if ((int64_t)listed > e->wlist_cap)
    return fail(e, P2PG_ERR_STATE, "sparse scatter: " + std::to_string(listed) +
                                          " frontier words listed, room for " +
                                          std::to_string(e->wlist_cap));
  return P2PG_OK;
}

// Arrivals (p2pg_round_stats.received): a churn or downtime run with P2PG_FLAG_RECEIVED counts the
// lost sends of every round.
bool count_lost_on(const p2pg_engine* e) {
  return (e->cfg.churn_threshold != 0 || e->down_on || e->ns_win.on()) && (e->cfg.flags & P2PG_FLAG_RECEIVED);
}
// Is the `received` counter of round r exact?  No churn, or the losses counted; with a downtime
// whose losses are not counted, every round outside min(from) <= r < max(until); with a netsplit
// whose losses are not counted, every round that is no cut round.
bool received_exact(const p2pg_engine* e, int32_t r) {
  if (count_lost_on(e)) return true;
  return e->cfg.churn_threshold == 0 && !(e->down_on && e->down_sweep.in_span(r)) && !e->ns_win.cut_round(r);
}
// The device's view of the downtime (null pointers without one: send_lost, device_util.h).
Downtime down(const p2pg_engine* e) { return Downtime{e->d_down_from, e->d_down_until}; }
// The device's view of the netsplit (a null side without one).
Netsplit cut(const p2pg_engine* e) { return Netsplit{e->d_side, e->ns_win.from, e->ns_win.until}; }
// The device's view of the anti-entropy exchange whose replies arrived in round r: the reply plane
// while it still belongs to that round (until the next gather), else null pointers -- find_parent
// and the sender walks of k_sends / k_peer_tally then do what they do without the setting.
Pull pull_of(const p2pg_engine* e, int32_t r) {
  if (!e->ae.on() || !e->d_pull_R || r < 0 || e->pull_round != r) return Pull{nullptr, nullptr, nullptr, 0u, 0u};
  return Pull{e->d_pull_R, e->d_pull_PB, e->d_pull_cnt, (uint32_t)e->ae_seed, (uint32_t)(e->ae_seed >> 32)};
}

constexpr size_t PULL_BYTES = sizeof(unsigned long long) * STAT_SHARDS * PULL_N;
// The reply plane, its bitmap and the counter shards, allocated at the first arrival round of a
// state (they are sized by its W) and freed with it.
int ensure_pull(p2pg_engine* e) {
  if (e->d_pull_R) return P2PG_OK;
  hipError_t x = hipMalloc((void**)&e->d_pull_R, e->plane_bytes ? e->plane_bytes : 8);
  if (x == hipSuccess) x = hipMalloc((void**)&e->d_pull_PB, e->bm_bytes ? e->bm_bytes : 8);
  if (x == hipSuccess) x = hipMalloc((void**)&e->d_pull_cnt, PULL_BYTES);
  if (x == hipSuccess) x = hipHostMalloc((void**)&e->h_pull_cnt, PULL_BYTES);
  if (x == hipSuccess) return P2PG_OK;
  dfree(e->d_pull_R);
  dfree(e->d_pull_PB);
  dfree(e->d_pull_cnt);
  return fail(e, x == hipErrorOutOfMemory ? P2PG_ERR_NOMEM : P2PG_ERR_HIP,
              std::string("step (anti-entropy planes): ") + hipGetErrorString(x));
}

// Run tallies (P2PG_FLAG_TALLY): every round keeps its whole frontier rows, which the column
// count (at the round's end) and the peer pass (before the next round) read.
bool tally_on(const p2pg_engine* e) { return (e->cfg.flags & P2PG_FLAG_TALLY) != 0; }
// Per-message cost (P2PG_FLAG_MSG_COST): the pass over a round's final sends binned by message.
bool cost_on(const p2pg_engine* e) { return (e->cfg.flags & P2PG_FLAG_MSG_COST) != 0; }
// Is some pass deferred to the point where a round's sends are final (flush_peer_tally)?  Such an
// engine keeps whole frontier rows and the pending-round bookkeeping.
bool deferred_on(const p2pg_engine* e) { return tally_on(e) || cost_on(e); }
// Does a round of this engine need its frontier rows whole (no skipped / partial rows, no
// batched decay rounds)?
// (a relay policy reads and rewrites the rows of every round: relay_policy.hip)
// Delivery latency (P2PG_FLAG_LATENCY): every round keeps its whole frontier rows, which the two
// latency passes read at the round's end.  Nothing is deferred: receipts are final then.
bool latency_on(const p2pg_engine* e) { return (e->cfg.flags & P2PG_FLAG_LATENCY) != 0; }
bool frontier_needed(const p2pg_engine* e) {
  return count_lost_on(e) || deferred_on(e) || latency_on(e) || e->pol_on;
}

// The device copy of the start rounds and their bit-sliced planes from h_start (the caller has
// synchronised the stream: upload_schedule).  The planes grow when a later start needs more bits.
int upload_latency(p2pg_engine* e) {
  const int32_t M = e->M, W = e->W;
  const int B = latency::plane_bits(latency::max_start(M, e->h_start.data()));
  HIPCHK(e, hipMemcpy(e->d_lstart, e->h_start.data(), sizeof(int32_t) * (size_t)M, hipMemcpyHostToDevice));
  e->lat_B = B;
  if (!B) return P2PG_OK;
  const int64_t words = (int64_t)B * W;
  if (words > e->lat_planes_cap) {
    dfree(e->d_lplanes);
    e->lat_planes_cap = 0;
    HIPCHK(e, hipMalloc((void**)&e->d_lplanes, sizeof(uint64_t) * (size_t)words));
    e->lat_planes_cap = words;
  }
  std::vector<uint64_t> planes((size_t)words);
  latency::build_start_planes(M, W, e->h_start.data(), B, planes.data());
  HIPCHK(e, hipMemcpy(e->d_lplanes, planes.data(), sizeof(uint64_t) * (size_t)words, hipMemcpyHostToDevice));
  return P2PG_OK;
}

// The histogram plane [M][lat_bins], zeroed (alloc_state, p2pg_set_latency_bins).
int alloc_latency_hist(p2pg_engine* e) {
  dfree(e->d_lhist);
  const size_t hb = sizeof(unsigned long long) * (size_t)e->M * (size_t)e->lat_bins;
  const hipError_t r = hipMalloc((void**)&e->d_lhist, hb ? hb : 8);
  if (r != hipSuccess)
    return fail(e, r == hipErrorOutOfMemory ? P2PG_ERR_NOMEM : P2PG_ERR_HIP,
                std::string("hipMalloc (latency histograms): ") + hipGetErrorString(r));
  HIPCHK(e, hipMemsetAsync(e->d_lhist, 0, hb, e->stream));
  return P2PG_OK;
}

// Enqueue the peer counters and / or the per-message cost of the pending round (its sends are
// final now): the sends leave on
// gs (gone slots = connections removed while they were in flight), the round's own arrivals
// travelled on graph_for_arrivals.  Stream order only, no host synchronisation.
hipError_t flush_peer_tally(p2pg_engine* e, const DevGraph& gs) {
  if (!deferred_on(e) || e->tally_pending < 0) return hipSuccess;
  const int32_t r = e->tally_pending;
  e->tally_pending = -1;
  RoundParams p = params(e);
  p.round = r;
  hipError_t x = hipSuccess;
  if (tally_on(e))
    x = launch_peer_tally(gs, graph_for_arrivals(e, r), e->st, p, down(e), cut(e), pull_of(e, r), e->d_tsent, e->d_trecv, e->stream);
  if (x == hipSuccess && cost_on(e))
    x = launch_msg_cost(gs, graph_for_arrivals(e, r), e->st, p, down(e), cut(e), pull_of(e, r), e->d_cscratch, e->d_csent,
                        e->d_crecv, e->stream);
  return x;
}

// Enqueue the count of round r's lost sends (k_sends, count mode) over gs (the graph the sends
// leave on; gone slots = removed connections) and gp (the graph round r's arrivals travelled
// on: the senders' own first receipts); the count lands in h_cnt2[1] at the next stream sync.
hipError_t enqueue_lost_count(p2pg_engine* e, const DevGraph& gs, const DevGraph& gp, int32_t r) {
  hipError_t x = hipMemsetAsync(e->d_cnt2, 0, 2 * sizeof(unsigned long long), e->stream);
  RoundParams p = params(e);
  p.round = r;
  if (x == hipSuccess)
    x = launch_sends(gs, gp, e->st, p, down(e), cut(e), pull_of(e, r), false, 0, nullptr, nullptr, nullptr, nullptr, e->d_cnt2, e->stream);
  if (x == hipSuccess)
    x = hipMemcpyAsync(e->h_cnt2, e->d_cnt2, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream);
  return x;
}

// Dense-round edge-mask planes E, sized by the current nnz: one, or two for fused rounds
// (round r pulls E[(r-1)&1], pushes E[r&1]); only if they fit with headroom -- else gossip
// pushes by row atomics only.  Replaces any previous planes (their contents are dropped).
int alloc_edge_planes(p2pg_engine* e) {
  DevState& s = e->st;
  if (s.E[1] == s.E[0]) s.E[1] = nullptr;
  dfree(s.E[0]);
  dfree(s.E[1]);
  if (e->cfg.mode != P2PG_MODE_GOSSIP || !e->d_rev || e->rules.push_mode == 1) return P2PG_OK;
  // a rank-local graph's ghost slots are usable by the PART kernels only (part_dense)
  if ((e->cfg.flags & P2PG_FLAG_LOCAL_GRAPH) &&
      !(e->fused && e->W > GROUPED_W_MAX && e->W <= 64 && s.AW[0]))
    return P2PG_OK;
  const size_t eb = (size_t)e->nnz * e->W * sizeof(uint64_t);
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || eb + ((size_t)4 << 30) >= free_b)
    return P2PG_OK;
  HIPCHK(e, hipMalloc((void**)&s.E[0], eb ? eb : 8));
  s.E[1] = s.E[0];
  if (e->W <= 64 && e->fused && hipMemGetInfo(&free_b, &total_b) == hipSuccess &&
      eb + ((size_t)4 << 30) < free_b)
    HIPCHK(e, hipMalloc((void**)&s.E[1], eb ? eb : 8));
  return P2PG_OK;
}

int alloc_state(p2pg_engine* e) {
  free_state(e);
  DevState& s = e->st;
  s.W = e->rules.W = e->W;
  e->rules.e_thresh = e->e_thresh_env >= 0.0 ? e->e_thresh_env : (e->W > GROUPED_W_MAX ? 0.06 : 0.04);
  // a dense round costs a visit of every unsaturated peer whatever the width, a sparse one an
  // atomic per pushed mask: narrow rows (a message split's shares) stay sparse until nearly every
  // peer is active (c4 interleaved sweeps, profiles/r03/ab_v_thresh.txt: W = 8 0.3 / 0.6 / 0.9 /
  // 0.95 / 0.98 -> 85.6 / 81.3 / 79.9 / 79.2 / 83.6 ms; W = 16 -> 144.5 / 138.9 / 130.4 / 128.7 /
  // 127.6 ms; W = 32 0.3 / 0.7 / 0.9 / 0.95 -> 218.4 / 211.7 / 208.4 / 203.7 ms; W = 64: 0.3 ...
  // 0.9 equal, 0.95 within 1 %, so the round-2 value stays)
  e->rules.v_thresh = e->v_thresh_env >= 0.0 ? e->v_thresh_env : e->W <= 32 ? 0.95 : 0.3;
  s.M = e->M;
  e->plane_bytes = (size_t)e->V * e->W * sizeof(uint64_t);
  e->seen_spare_off = false;  // a new plane size: the spare's size / memory check runs again
  e->bm_bytes = (size_t)((e->V + 31) / 32) * sizeof(uint32_t);
  const bool gossip = e->cfg.mode == P2PG_MODE_GOSSIP;
  const bool rec = (e->cfg.flags & P2PG_FLAG_RECORD) != 0;
  auto A = [&](void** p, size_t n) -> int {
    hipError_t r = hipMalloc(p, n ? n : 8);
    if (r != hipSuccess) {
      free_state(e);
      return fail(e, r == hipErrorOutOfMemory ? P2PG_ERR_NOMEM : P2PG_ERR_HIP,
                  std::string("hipMalloc: ") + hipGetErrorString(r));
    }
    return P2PG_OK;
  };
  int rc;
  if ((rc = A((void**)&s.seen, e->plane_bytes))) return rc;
  for (int i = 0; i < 2; ++i) {
    if ((rc = A((void**)&s.F[i], e->plane_bytes))) return rc;
    if ((rc = A((void**)&s.A[i], e->bm_bytes))) return rc;
    if (gossip) {
      if ((rc = A((void**)&s.next[i], e->plane_bytes))) return rc;
      if ((rc = A((void**)&s.T[i], e->bm_bytes))) return rc;
      HIPCHK(e, hipMemsetAsync(s.next[i], 0, e->plane_bytes, e->stream));
      HIPCHK(e, hipMemsetAsync(s.T[i], 0, e->bm_bytes, e->stream));
    }
  }
  if ((rc = A((void**)&s.S, e->bm_bytes))) return rc;
  if (gossip && e->W > PACK_W_MAX_PLAIN && e->W <= 64)  // packed E rows (see DevState::AW)
    for (int i = 0; i < 2; ++i)
      if ((rc = A((void**)&s.AW[i], sizeof(uint64_t) * (size_t)e->V))) return rc;
  if ((rc = alloc_edge_planes(e))) {
    free_state(e);
    return rc;
  }
  if (rec) {
    const size_t hb = (size_t)e->V * e->M * sizeof(int32_t);
    if ((rc = A((void**)&s.hop, hb))) return rc;
    if ((rc = A((void**)&s.parent, hb))) return rc;
  }
  if ((rc = A((void**)&s.stats, STAT_BYTES))) return rc;
  if ((rc = A((void**)&e->d_cnt2, 2 * sizeof(unsigned long long)))) return rc;
  HIPCHK(e, hipHostMalloc((void**)&e->h_cnt2, 2 * sizeof(unsigned long long)));
  if (tally_on(e)) {  // 2 * V * 8 + M * 20 bytes, and the column count's shards (p2pg_reset zeroes)
    const size_t sb = sizeof(unsigned long long) * (size_t)tally_scratch_words(e->W);
    if ((rc = A((void**)&e->d_treach, sizeof(unsigned long long) * (size_t)e->M))) return rc;
    if ((rc = A((void**)&e->d_thop, sizeof(unsigned long long) * (size_t)e->M))) return rc;
    if ((rc = A((void**)&e->d_tlast, sizeof(int32_t) * (size_t)e->M))) return rc;
    if ((rc = A((void**)&e->d_tsent, sizeof(unsigned long long) * (size_t)e->V))) return rc;
    if ((rc = A((void**)&e->d_trecv, sizeof(unsigned long long) * (size_t)e->V))) return rc;
    if ((rc = A((void**)&e->d_tscratch, sb))) return rc;
    const hipError_t zr = hipMemsetAsync(e->d_tscratch, 0, sb, e->stream);
    if (zr != hipSuccess) {
      free_state(e);
      return fail(e, P2PG_ERR_HIP, std::string("alloc_state (tallies): ") + hipGetErrorString(zr));
    }
  }
  if (cost_on(e)) {  // M * 16 bytes and the cost pass's shards (p2pg_reset zeroes the counters)
    const size_t sb = sizeof(unsigned long long) * (size_t)cost_scratch_words(e->W);
    if ((rc = A((void**)&e->d_csent, sizeof(unsigned long long) * (size_t)e->M))) return rc;
    if ((rc = A((void**)&e->d_crecv, sizeof(unsigned long long) * (size_t)e->M))) return rc;
    if ((rc = A((void**)&e->d_cscratch, sb))) return rc;
    const hipError_t zr = hipMemsetAsync(e->d_cscratch, 0, sb, e->stream);
    if (zr != hipSuccess) {
      free_state(e);
      return fail(e, P2PG_ERR_HIP, std::string("alloc_state (message cost): ") + hipGetErrorString(zr));
    }
  }
  if (latency_on(e)) {  // M * (bins * 8 + 4) + V * 16 bytes; the planes follow the schedule (upload_latency)
    if ((rc = alloc_latency_hist(e))) {
      free_state(e);
      return rc;
    }
    if ((rc = A((void**)&e->d_lstart, sizeof(int32_t) * (size_t)e->M))) return rc;
    if ((rc = A((void**)&e->d_lpeer, sizeof(PeerLat) * (size_t)e->V))) return rc;
    if (!e->d_tscratch) {  // (with P2PG_FLAG_TALLY the two folds share the tally's shards)
      const size_t sb = sizeof(unsigned long long) * (size_t)tally_scratch_words(e->W);
      if ((rc = A((void**)&e->d_tscratch, sb))) return rc;
      const hipError_t zr = hipMemsetAsync(e->d_tscratch, 0, sb, e->stream);
      if (zr != hipSuccess) {
        free_state(e);
        return fail(e, P2PG_ERR_HIP, std::string("alloc_state (latency): ") + hipGetErrorString(zr));
      }
    }
  }
#ifdef P2PG_PROF
  if ((rc = A((void**)&s.prof, sizeof(unsigned long long) * 16))) return rc;
  HIPCHK(e, hipMemset(s.prof, 0, sizeof(unsigned long long) * 16));
#endif
  if ((rc = A((void**)&e->d_src, sizeof(int32_t) * (e->M ? e->M : 1)))) return rc;
  e->have_state = true;
  e->stats_clear = true;
  return P2PG_OK;
}

}  // namespace

extern "C" {

int p2pg_create(const p2pg_config* cfg, p2pg_engine** out) {
  if (!cfg || !out) return fail(nullptr, P2PG_ERR_ARG, "create: null argument");
  *out = nullptr;
  if (cfg->mode != P2PG_MODE_FLOOD && cfg->mode != P2PG_MODE_GOSSIP)
    return fail(nullptr, P2PG_ERR_ARG, "create: unknown mode");
  if (cfg->mode == P2PG_MODE_GOSSIP && (cfg->fanout < 1 || cfg->fanout > 16))
    return fail(nullptr, P2PG_ERR_ARG, "create: gossip fanout must be in [1, 16]");
  if ((cfg->flags & P2PG_FLAG_TALLY) && (cfg->flags & P2PG_FLAG_LOCAL_GRAPH))
    return fail(nullptr, P2PG_ERR_ARG, "create: P2PG_FLAG_TALLY is not available on a vertex-partitioned rank "
                                       "(P2PG_FLAG_LOCAL_GRAPH): ghost rows would be counted on two ranks");
  if ((cfg->flags & P2PG_FLAG_MSG_COST) && (cfg->flags & P2PG_FLAG_LOCAL_GRAPH))
    return fail(nullptr, P2PG_ERR_ARG, "create: P2PG_FLAG_MSG_COST is not available on a vertex-partitioned rank "
                                       "(P2PG_FLAG_LOCAL_GRAPH): ghost rows would be counted on two ranks");
  if ((cfg->flags & P2PG_FLAG_LATENCY) && (cfg->flags & P2PG_FLAG_LOCAL_GRAPH))
    return fail(nullptr, P2PG_ERR_ARG, "create: P2PG_FLAG_LATENCY is not available on a vertex-partitioned rank "
                                       "(P2PG_FLAG_LOCAL_GRAPH): ghost rows would be counted on two ranks");
  int ndev = 0;
  hipError_t r = hipGetDeviceCount(&ndev);
  if (r != hipSuccess || ndev == 0)
    return fail(nullptr, P2PG_ERR_HIP, "create: no HIP device visible");
  if (cfg->device < 0 || cfg->device >= ndev)
    return fail(nullptr, P2PG_ERR_ARG, "create: device ordinal out of range");
  p2pg_engine* e = new p2pg_engine;
  e->cfg = *cfg;
  if (const char* t = std::getenv("P2PG_E_THRESH")) e->e_thresh_env = std::atof(t);
  if (const char* t = std::getenv("P2PG_V_THRESH")) e->v_thresh_env = std::atof(t);
  if (const char* f = std::getenv("P2PG_FUSED")) e->fused = std::strcmp(f, "0") != 0;
  if (const char* f = std::getenv("P2PG_SPARSE_LP")) e->sparse_lp = std::strcmp(f, "0") != 0;
  if (const char* f = std::getenv("P2PG_PUSH_DEDUP")) e->rules.push_dedup = std::atoi(f);
  if (const char* f = std::getenv("P2PG_WIDE_ATOMIC")) e->wide_atomic = std::strcmp(f, "0") != 0;
  if (const char* f = std::getenv("P2PG_UPDATE_PUSH")) e->rules.update_push = std::atoi(f);
  if (const char* f = std::getenv("P2PG_RUN_BATCH")) e->batch_rounds = std::atoi(f);
  if (const char* f = std::getenv("P2PG_DECAY_PRED")) e->rules.decay_pred = std::strcmp(f, "0") != 0;
  if (const char* f = std::getenv("P2PG_PARTIAL_F")) e->partial_f = std::strcmp(f, "0") != 0;
  if (const char* f = std::getenv("P2PG_SEEN_SPARE")) e->seen_spare_on = std::strcmp(f, "0") != 0;
  if (const char* m = std::getenv("P2PG_GOSSIP_PUSH"))
    e->rules.push_mode = !std::strcmp(m, "atomic") ? 1 : (!std::strcmp(m, "store") ? 2 : 0);
  HIPCHK(e, hipSetDevice(cfg->device));
  HIPCHK(e, hipStreamCreateWithFlags(&e->own_stream, hipStreamNonBlocking));
  e->stream = e->own_stream;
  HIPCHK(e, hipEventCreate(&e->ev[0]));
  HIPCHK(e, hipEventCreate(&e->ev[1]));
  HIPCHK(e, hipEventCreateWithFlags(&e->ev_sync, hipEventDisableTiming));
  if (const char* f = std::getenv("P2PG_SPIN")) e->spin = std::strcmp(f, "0") != 0;
  HIPCHK(e, hipHostMalloc((void**)&e->h_stats, STAT_BYTES));
  *out = e;
  return P2PG_OK;
}

int p2pg_set_stream(p2pg_engine* e, void* hip_stream) {
  if (!e) return P2PG_ERR_ARG;
  hipStream_t s = hip_stream ? (hipStream_t)hip_stream : e->own_stream;
  if (s != e->stream && e->stream) {  // work queued on the old stream finishes first
    HIPCHK(e, hipSetDevice(e->cfg.device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
  }
  e->stream = s;
  return P2PG_OK;
}

}  // extern "C"

namespace {

// Checks the CSR invariants the kernels rely on and builds the gossip reverse slots.
int check_csr(p2pg_engine* e, int64_t V, const int64_t* rowptr, const int32_t* colidx,
              std::vector<uint32_t>& rev) {
  if (V <= 0 || V > 0x7FFFFFFFll || !rowptr) return fail(e, P2PG_ERR_ARG, "load_csr: bad arguments");
  const int64_t nnz = rowptr[V];
  if (rowptr[0] != 0 || nnz < 0 || (nnz > 0 && !colidx))
    return fail(e, P2PG_ERR_GRAPH, "load_csr: rowptr[0] must be 0 and rowptr[V] >= 0");
  // validate: monotone rows, ids in range, strictly ascending (sorted, no multi-edges),
  // no self loops -- the invariants the kernels' lowest-id parent order relies on
  for (int64_t v = 0; v < V; ++v) {
    if (rowptr[v + 1] < rowptr[v]) return fail(e, P2PG_ERR_GRAPH, "load_csr: rowptr not monotone");
    for (int64_t j = rowptr[v]; j < rowptr[v + 1]; ++j) {
      const int32_t u = colidx[j];
      if (u < 0 || u >= V) return fail(e, P2PG_ERR_GRAPH, "load_csr: neighbour id out of range");
      if (u == v) return fail(e, P2PG_ERR_GRAPH, "load_csr: self loop");
      if (j > rowptr[v] && colidx[j - 1] >= u)
        return fail(e, P2PG_ERR_GRAPH, "load_csr: row not strictly ascending");
    }
  }
  // symmetry (every connection relays both ways, node.py:75-78) and reverse slots
  const bool local = (e->cfg.flags & P2PG_FLAG_LOCAL_GRAPH) != 0;
  // reverse slots for gossip's dense rounds; on a rank-local graph a ghost neighbour's slot is
  // marked instead (REV_GHOST | its local id), and slot ids must stay below that bit
  rev.assign(e->cfg.mode == P2PG_MODE_GOSSIP && nnz < (local ? (int64_t)REV_GHOST : 0xFFFFFFFFll) ? nnz : 0,
             0u);
  int64_t asym = -1;
#pragma omp parallel for schedule(dynamic, 4096)
  for (int64_t u = 0; u < V; ++u) {
    for (int64_t j = rowptr[u]; j < rowptr[u + 1]; ++j) {
      const int64_t v = colidx[j];
      const int32_t* b = colidx + rowptr[v];
      const int32_t* en = colidx + rowptr[v + 1];
      if (local && b == en) {  // ghost peer: its row lives on its owner rank
        if (!rev.empty()) rev[j] = REV_GHOST | (uint32_t)v;
        continue;
      }
      const int32_t* it = std::lower_bound(b, en, (int32_t)u);
      if (it == en || *it != u) {
#pragma omp critical
        asym = u;
      } else if (!rev.empty()) {
        rev[j] = (uint32_t)(rowptr[v] + (it - b));
      }
    }
  }
  if (asym >= 0) return fail(e, P2PG_ERR_GRAPH, "load_csr: adjacency not symmetric");
  return P2PG_OK;
}

// Device copies of a checked CSR (rows, reverse slots, gossip chunk items, pull hub plan);
// replaces the engine's topology arrays, leaves the run state alone.
int upload_graph(p2pg_engine* e, int64_t V, const int64_t* rowptr, const int32_t* colidx,
                 const std::vector<uint32_t>& rev) {
  const int64_t nnz = rowptr[V];
  free_topology(e);
  e->V = V;
  e->nnz = nnz;
  e->rules.v_conn = 0;
  for (int64_t v = 0; v < V; ++v) e->rules.v_conn += rowptr[v + 1] > rowptr[v];
  if (!rev.empty()) {
    HIPCHK(e, hipMalloc((void**)&e->d_rev, sizeof(uint32_t) * rev.size()));
    HIPCHK(e, hipMemcpy(e->d_rev, rev.data(), sizeof(uint32_t) * rev.size(), hipMemcpyHostToDevice));
  }
  e->h_rowptr.assign(rowptr, rowptr + V + 1);
  e->seed.ok = false;
  e->h_colidx.assign(colidx, colidx + nnz);
  HIPCHK(e, hipMalloc((void**)&e->d_rowptr, sizeof(int64_t) * (V + 1)));
  HIPCHK(e, hipMalloc((void**)&e->d_colidx, sizeof(int32_t) * (nnz ? nnz : 1)));
  HIPCHK(e, hipMemcpy(e->d_rowptr, rowptr, sizeof(int64_t) * (V + 1), hipMemcpyHostToDevice));
  if (nnz) HIPCHK(e, hipMemcpy(e->d_colidx, colidx, sizeof(int32_t) * nnz, hipMemcpyHostToDevice));
  // gossip: (source, neighbour-chunk) items for sources wider than one chunk
  std::vector<int64_t> hub, hub_big;
  std::vector<int32_t> wide_big;
  for (int64_t v = 0; v < V; ++v) {
    const int64_t d = rowptr[v + 1] - rowptr[v];
    if (d > GCHUNK) {
      if (d > HUB_T) wide_big.push_back((int32_t)v);
      for (int64_t c = 0; c * GCHUNK < d; ++c) {
        hub.push_back((v << 32) | c);
        if (d > HUB_T) hub_big.push_back((v << 32) | c);
      }
    }
  }
  e->n_wide_big = (int64_t)wide_big.size();
  if (!wide_big.empty()) {
    HIPCHK(e, hipMalloc((void**)&e->d_wide_big, sizeof(int32_t) * wide_big.size()));
    HIPCHK(e, hipMemcpy(e->d_wide_big, wide_big.data(), sizeof(int32_t) * wide_big.size(), hipMemcpyHostToDevice));
  }
  e->n_hub = (int64_t)hub.size();
  e->n_hub_big = (int64_t)hub_big.size();
  {  // pull-side hub plan
    std::vector<int32_t> hubs;
    std::vector<int64_t> items, begin{0};
    std::vector<uint32_t> H((V + 31) / 32, 0u);
    for (int64_t v = 0; v < V; ++v) {
      const int64_t d = rowptr[v + 1] - rowptr[v];
      if (d <= HUB_T) continue;
      hubs.push_back((int32_t)v);
      H[v >> 5] |= 1u << (v & 31);
      for (int64_t c = 0; c * HUB_CHUNK < d; ++c) items.push_back((v << 32) | c);
      begin.push_back((int64_t)items.size());
    }
    HIPCHK(e, hipMalloc((void**)&e->d_H, sizeof(uint32_t) * H.size()));
    HIPCHK(e, hipMemcpy(e->d_H, H.data(), sizeof(uint32_t) * H.size(), hipMemcpyHostToDevice));
    if (!hubs.empty()) {
      HIPCHK(e, hipMalloc((void**)&e->d_hubs, sizeof(int32_t) * hubs.size()));
      HIPCHK(e, hipMalloc((void**)&e->d_hub_items, sizeof(int64_t) * items.size()));
      HIPCHK(e, hipMalloc((void**)&e->d_hub_begin, sizeof(int64_t) * begin.size()));
      HIPCHK(e, hipMalloc((void**)&e->d_partial, sizeof(uint64_t) * 64 * items.size()));
      HIPCHK(e, hipMemcpy(e->d_hubs, hubs.data(), sizeof(int32_t) * hubs.size(), hipMemcpyHostToDevice));
      HIPCHK(e, hipMemcpy(e->d_hub_items, items.data(), sizeof(int64_t) * items.size(), hipMemcpyHostToDevice));
      HIPCHK(e, hipMemcpy(e->d_hub_begin, begin.data(), sizeof(int64_t) * begin.size(), hipMemcpyHostToDevice));
    }
    e->hp = HubPlan{e->d_hub_items, (int64_t)items.size(), e->d_hubs, e->d_hub_begin,
                    (int64_t)hubs.size(), e->d_partial};
    // the fused kernels' push modes skip the H peers and push them through wide_big
    // (launch_wide_push_e): the two sets must be the same peers
    if (hubs.size() != wide_big.size() || !std::equal(hubs.begin(), hubs.end(), wide_big.begin()))
      return fail(e, P2PG_ERR_STATE, "load_csr: pull hubs and wide push sources differ");
  }
  HIPCHK(e, hipMalloc((void**)&e->d_hub, sizeof(int64_t) * (hub.empty() ? 1 : hub.size())));
  if (!hub.empty())
    HIPCHK(e, hipMemcpy(e->d_hub, hub.data(), sizeof(int64_t) * hub.size(), hipMemcpyHostToDevice));
  HIPCHK(e, hipMalloc((void**)&e->d_hub_big, sizeof(int64_t) * (hub_big.empty() ? 1 : hub_big.size())));
  if (!hub_big.empty())
    HIPCHK(e, hipMemcpy(e->d_hub_big, hub_big.data(), sizeof(int64_t) * hub_big.size(), hipMemcpyHostToDevice));
  return P2PG_OK;
}

}  // namespace

extern "C" {

int p2pg_load_csr(p2pg_engine* e, int64_t V, const int64_t* rowptr, const int32_t* colidx) {
  if (!e) return fail(e, P2PG_ERR_ARG, "load_csr: bad arguments");
  std::vector<uint32_t> rev;
  int rc = check_csr(e, V, rowptr, colidx, rev);
  if (rc) return rc;
  HIPCHK(e, hipSetDevice(e->cfg.device));
  free_graph(e);
  free_state(e);
  if ((rc = upload_graph(e, V, rowptr, colidx, rev))) return rc;
  e->M = 0;
  e->W = 0;
  e->round = 0;
  e->done = true;
  return P2PG_OK;
}

}  // extern "C"

namespace {

// The device schedule from h_src / h_start: the messages with start > 0 sorted by (round, peer,
// msg), their (round, peer) groups, the group range of every round; d_src = round 0's seeds
// (-1 for every other message).  Runs when the schedule changes (set_sources[_at], originate).
int upload_schedule(p2pg_engine* e) {
  const int32_t M = e->M;
  std::vector<int32_t> seed0(M), order;
  e->late = false;
  e->last_start = 0;
  for (int32_t m = 0; m < M; ++m) {
    seed0[m] = e->h_start[m] == 0 ? e->h_src[m] : -1;
    if (e->h_start[m] != 0) e->late = true;
    if (e->h_start[m] > 0) {
      order.push_back(m);
      e->last_start = std::max(e->last_start, e->h_start[m]);
    }
  }
  std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
    if (e->h_start[a] != e->h_start[b]) return e->h_start[a] < e->h_start[b];
    return e->h_src[a] != e->h_src[b] ? e->h_src[a] < e->h_src[b] : a < b;
  });
  const size_t n = order.size();
  std::vector<int32_t> peer(n), msg(n);
  std::vector<int64_t> grp;
  e->sched_rounds.clear();
  for (size_t i = 0; i < n; ++i) {
    const int32_t m = order[i];
    peer[i] = e->h_src[m];
    msg[i] = m;
    const bool new_round = i == 0 || e->h_start[m] != e->h_start[order[i - 1]];
    if (new_round || peer[i] != peer[i - 1]) {
      if (new_round) {
        if (!e->sched_rounds.empty()) e->sched_rounds.back().g_hi = (int64_t)grp.size();
        e->sched_rounds.push_back({e->h_start[m], (int64_t)grp.size(), 0});
      }
      grp.push_back((int64_t)i);
    }
  }
  if (!e->sched_rounds.empty()) e->sched_rounds.back().g_hi = (int64_t)grp.size();
  grp.push_back((int64_t)n);
  HIPCHK(e, hipSetDevice(e->cfg.device));
  // (the stream may still run a round that reads the old arrays)
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipMemcpy(e->d_src, seed0.data(), sizeof(int32_t) * M, hipMemcpyHostToDevice));
  dfree(e->d_sched_peer);
  dfree(e->d_sched_msg);
  dfree(e->d_sched_grp);
  if (n) {
    HIPCHK(e, hipMalloc((void**)&e->d_sched_peer, sizeof(int32_t) * n));
    HIPCHK(e, hipMalloc((void**)&e->d_sched_msg, sizeof(int32_t) * n));
    HIPCHK(e, hipMalloc((void**)&e->d_sched_grp, sizeof(int64_t) * grp.size()));
    HIPCHK(e, hipMemcpy(e->d_sched_peer, peer.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(e->d_sched_msg, msg.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(e->d_sched_grp, grp.data(), sizeof(int64_t) * grp.size(), hipMemcpyHostToDevice));
  }
  return latency_on(e) ? upload_latency(e) : P2PG_OK;
}

// The originations of round r > 0, or nullptr.
const p2pg_engine::SchedRound* sched_round(const p2pg_engine* e, int32_t r) {
  if (r <= 0 || r > e->last_start) return nullptr;
  auto it = std::lower_bound(e->sched_rounds.begin(), e->sched_rounds.end(), r,
                             [](const p2pg_engine::SchedRound& a, int32_t x) { return a.round < x; });
  return it != e->sched_rounds.end() && it->round == r ? &*it : nullptr;
}

// Does a scheduled start lie at or after round r?  (Unscheduled messages keep no run alive.)
bool start_ahead(const p2pg_engine* e, int32_t r) { return e->last_start >= r && e->last_start > 0; }

// Is this engine a rank of a vertex partition?
bool partitioned(const p2pg_engine* e) { return e->d_gid || (e->cfg.flags & P2PG_FLAG_LOCAL_GRAPH); }

// The device expiry schedule from h_ttl / h_start: the rounds in which a scheduled message with a
// finite hop limit expires and their X / Z masks.  Runs when the limits or the schedule change
// (set_ttl, originate); an unscheduled message has no expiry round until p2pg_originate gives it
// a start.
int upload_expiry(p2pg_engine* e) {
  const int32_t M = e->M, W = e->W;
  std::vector<std::pair<int64_t, int32_t>> xs;  // (expiry round, message)
  e->ttl_on = false;
  for (int32_t m = 0; m < M && !e->h_ttl.empty(); ++m) {
    if (e->h_ttl[m] < 0) continue;
    e->ttl_on = true;
    const int64_t x = (int64_t)e->h_start[m] + e->h_ttl[m];
    if (e->h_start[m] >= 0 && x <= 0x7FFFFFFFll) xs.emplace_back(x, m);
  }
  std::sort(xs.begin(), xs.end());
  e->exp_rounds.clear();
  std::vector<uint64_t> masks;
  for (const auto& xm : xs) {
    if (e->exp_rounds.empty() || e->exp_rounds.back() != (int32_t)xm.first) {
      e->exp_rounds.push_back((int32_t)xm.first);
      masks.resize(masks.size() + 2 * (size_t)W, 0ull);
    }
    uint64_t* const X = masks.data() + masks.size() - 2 * (size_t)W;
    const int32_t m = xm.second;
    X[m >> 6] |= 1ull << (m & 63);
    if (e->h_ttl[m] == 0) X[W + (m >> 6)] |= 1ull << (m & 63);
  }
  HIPCHK(e, hipSetDevice(e->cfg.device));
  // (the stream may still run a pass that reads the old masks)
  HIPCHK(e, hipStreamSynchronize(e->stream));
  dfree(e->d_exp);
  if (!masks.empty()) {
    HIPCHK(e, hipMalloc((void**)&e->d_exp, sizeof(uint64_t) * masks.size()));
    HIPCHK(e, hipMemcpy(e->d_exp, masks.data(), sizeof(uint64_t) * masks.size(), hipMemcpyHostToDevice));
  }
  e->seed.ok = false;  // (round 0's relays leave out the ttl-0 originations)
  return P2PG_OK;
}

// Index into exp_rounds of round r's expiries, or -1.
int64_t expiry_index(const p2pg_engine* e, int32_t r) {
  if (e->exp_rounds.empty() || r > e->exp_rounds.back()) return -1;
  auto it = std::lower_bound(e->exp_rounds.begin(), e->exp_rounds.end(), r);
  return it != e->exp_rounds.end() && *it == r ? (int64_t)(it - e->exp_rounds.begin()) : -1;
}

// Does an expiry lie at or after round r?
bool expiry_ahead(const p2pg_engine* e, int32_t r) {
  return !e->exp_rounds.empty() && e->exp_rounds.back() >= r;
}

// Does message m expire in round r?
bool expires_in(const p2pg_engine* e, int32_t m, int32_t r) {
  return !e->h_ttl.empty() && e->h_ttl[m] >= 0 && e->h_start[m] >= 0 &&
         (int64_t)e->h_start[m] + e->h_ttl[m] == (int64_t)r;
}

// Relay policy: the per-round masks of the messages the policy leaves alone -- the originations of
// a round (the app's own send_to_nodes, not a relay) and the messages whose hop limit runs out in
// it (k_expire cancels those, once).  One W-word mask per round > 0 that has either; round 0 is
// never a policy round.  Runs when the schedule, the hop limits or the policy change.
int upload_exempt(p2pg_engine* e) {
  if (!e->have_state) return P2PG_OK;
  const int32_t M = e->M, W = e->W;
  std::vector<std::pair<int64_t, int32_t>> xs;  // (round, message)
  for (int32_t m = 0; m < M && e->pol_on; ++m) {
    if (e->h_start[m] < 0) continue;
    if (e->h_start[m] > 0) xs.emplace_back(e->h_start[m], m);
    if (!e->h_ttl.empty() && e->h_ttl[m] > 0) {  // (ttl 0 expires in the start round itself)
      const int64_t x = (int64_t)e->h_start[m] + e->h_ttl[m];
      if (x <= 0x7FFFFFFFll) xs.emplace_back(x, m);
    }
  }
  std::sort(xs.begin(), xs.end());
  e->pex_rounds.clear();
  std::vector<uint64_t> masks;
  for (const auto& xm : xs) {
    if (e->pex_rounds.empty() || e->pex_rounds.back() != (int32_t)xm.first) {
      e->pex_rounds.push_back((int32_t)xm.first);
      masks.resize(masks.size() + (size_t)W, 0ull);
    }
    masks[masks.size() - (size_t)W + (xm.second >> 6)] |= 1ull << (xm.second & 63);
  }
  HIPCHK(e, hipSetDevice(e->cfg.device));
  // (the stream may still run a pass that reads the old masks)
  HIPCHK(e, hipStreamSynchronize(e->stream));
  dfree(e->d_pex);
  if (!masks.empty()) {
    HIPCHK(e, hipMalloc((void**)&e->d_pex, sizeof(uint64_t) * masks.size()));
    HIPCHK(e, hipMemcpy(e->d_pex, masks.data(), sizeof(uint64_t) * masks.size(), hipMemcpyHostToDevice));
  }
  return P2PG_OK;
}

// The policy's exempt mask of round r, or nullptr (no origination, no expiry in it).
const uint64_t* exempt_mask(const p2pg_engine* e, int32_t r) {
  if (e->pex_rounds.empty() || r > e->pex_rounds.back()) return nullptr;
  auto it = std::lower_bound(e->pex_rounds.begin(), e->pex_rounds.end(), r);
  if (it == e->pex_rounds.end() || *it != r) return nullptr;
  return e->d_pex + (size_t)(it - e->pex_rounds.begin()) * e->W;
}

// Is the first receipt of message m at peer v in round r muted by the relay policy?
bool policy_muted(const p2pg_engine* e, int64_t v, int32_t m, int32_t r) {
  if (!e->pol_on || r <= 0 || e->h_start[m] == r) return false;
  return relay_muted((uint32_t)r, (uint32_t)v, e->cfg.msg_id_base + (uint32_t)m, e->h_thr[v],
                     (uint32_t)e->pol_seed, (uint32_t)(e->pol_seed >> 32));
}

// The sends of the pending expiry or policy round become final: its expired and its muted frontier
// bits are cleared (relay_expire.hip, relay_policy.hip; a round may have both; from here on
// p2pg_get_new_deliveries refuses that round), then -- push -- a gossip round's held-back push
// leaves in the form its plan resolved to at the round's end (held_push_e): row atomics into the
// planes the next round's update consumes (an expiry round's always), or edge-mask stores into E
// that the next round pulls.  No push is made twice, no plane zeroed.  A churn run with
// P2PG_FLAG_RECEIVED then counts the round's lost sends, which it could not before the clearing.
// Called at the top of the next round, before the peer counters take the round in, and by the
// boundary calls that read or change the round's sends; drop_relays and update_edges redo the
// gossip pushes themselves (push = false).
// Returns a P2PG code.  The passes are timed with their classes: k_expire and k_policy with the
// origination class 0 (like k_originate, a pass over the schedule's messages), the push with
// class 6 or 2.
int finalize_expiry(p2pg_engine* e, bool push) {
  if (e->exp_pending < 0 && e->pol_pending < 0) return P2PG_OK;
  const int32_t r = std::max(e->exp_pending, e->pol_pending);  // (both are the last round)
  const int64_t xi = e->exp_pending >= 0 ? expiry_index(e, r) : -1;
  const bool pol = e->pol_pending >= 0 && e->pol_on;
  if (xi < 0 && !pol) {
    e->exp_pending = e->pol_pending = -1;
    return P2PG_OK;
  }
  RoundParams p = params(e);
  p.round = r;
  const DevGraph g = graph(e);
  int rc;
  if (xi >= 0) {
    const uint64_t* X = e->d_exp + 2 * (size_t)xi * e->W;
    if ((rc = timed(e, 0, [&] { return launch_expire(g, e->st, p, X, X + e->W, true, e->stream); }))) return rc;
  }
  if (pol &&
      (rc = timed(e, 0, [&] {
         return launch_policy(g, e->st, p, e->d_thr, e->pol_seed, exempt_mask(e, r), true, e->stream);
       })))
    return rc;
  // the bits are gone (stream order): the round is final whatever happens below
  e->exp_pending = e->pol_pending = -1;
  e->exp_final = r;
  if (push && e->cfg.mode == P2PG_MODE_GOSSIP && e->hist.last_new > 0) {
    if (e->held_push_e) {
      // a policy round that chose the dense form from its own counters: edge-mask stores into
      // E[r&1], which the next round pulls (last_push_e stands since the round's end)
      rc = timed(e, 6, [&] {
        return launch_gossip_scatter(g, e->st, p, e->d_hub, e->n_hub, true, e->stream, e->d_hub_big,
                                     e->n_hub_big, e->d_wide_big, e->n_wide_big);
      });
    } else {
      // The list is sized by the round's nonzero frontier words before the clearing (prev_aw), which
      // bounds the words left after it: this push cannot outgrow its list, so its count is not read
      // back (check_scatter_list would cost the boundary a host synchronisation).
      rc = timed(e, 2, [&] { return launch_scatter_atomic(e, g, p, std::max<uint64_t>(e->hist.prev_aw, 1)); });
      e->wlist_check = false;
    }
    e->stats_clear = true;  // the push counted into the round counters
    if (rc) return rc;
  }
  if (count_lost_on(e)) {
    hipError_t x = enqueue_lost_count(e, g, graph_for_arrivals(e, r), r);
    if (x == hipSuccess) x = hipStreamSynchronize(e->stream);
    if (x != hipSuccess) return fail(e, P2PG_ERR_HIP, std::string("hop limits (lost sends): ") + hipGetErrorString(x));
    e->lost_last = (uint64_t)e->h_cnt2[1];
  }
  return P2PG_OK;
}

// p2pg_set_sources (start == nullptr: every message starts in round 0) / p2pg_set_sources_at
int set_sources(p2pg_engine* e, const char* what, int32_t M, const int32_t* src, const int32_t* start) {
  const std::string w(what);
  if (!e || M <= 0 || !src) return fail(e, P2PG_ERR_ARG, w + ": need M > 0 and src");
  if (!e->d_rowptr) return fail(e, P2PG_ERR_STATE, w + ": load a graph first");
  if (start && e->begun) return fail(e, P2PG_ERR_STATE, w + ": a round has begun (step_begin)");
  bool late = false;
  for (int32_t m = 0; m < M; ++m) {
    const int32_t s = start ? start[m] : 0;
    if (s < -1) return fail(e, P2PG_ERR_ARG, w + ": start round below -1");
    if (s == -1 ? src[m] != -1 : (src[m] < 0 || src[m] >= e->V))
      return fail(e, P2PG_ERR_ARG, s == -1 ? w + ": an unscheduled message (start -1) takes source -1"
                                           : w + ": source out of range");
    late |= s != 0;
  }
  if (late && partitioned(e))
    return fail(e, P2PG_ERR_STATE, w + ": start rounds other than 0 are not available on a vertex-partitioned rank");
  if (e->down_on) {  // originations at an offline peer are refused (p2pg_set_downtime)
    const int64_t m = downtime::first_refused(M, src, start, e->h_down_from.data(), e->h_down_until.data());
    if (m >= 0)
      return fail(e, P2PG_ERR_ARG, w + ": the origin of message " + std::to_string(m) +
                                       " is offline in its start round (p2pg_set_downtime)");
  }
  HIPCHK(e, hipSetDevice(e->cfg.device));
  const int32_t W = (M + 63) / 64;
  e->h_src.assign(src, src + M);
  if (start)
    e->h_start.assign(start, start + M);
  else
    e->h_start.assign(M, 0);
  e->seed.ok = false;
  if (!e->have_state || W != e->W || M != e->M) {
    e->M = M;
    e->W = W;
    int rc = alloc_state(e);
    if (rc) return rc;
  }
  int rc = upload_schedule(e);
  if (rc) return rc;
  if (!e->h_ttl.empty()) {  // new sources carry no hop limits
    e->h_ttl.clear();
    if ((rc = upload_expiry(e))) return rc;
  }
  // (a relay policy belongs to the peers and stays: its exempt masks follow the new schedule)
  if ((e->pol_on || e->d_pex) && (rc = upload_exempt(e))) return rc;
  return p2pg_reset(e);
}

}  // namespace

extern "C" {

int p2pg_set_sources(p2pg_engine* e, int32_t M, const int32_t* src) {
  return set_sources(e, "set_sources", M, src, nullptr);
}

int p2pg_set_sources_at(p2pg_engine* e, int32_t M, const int32_t* src, const int32_t* start) {
  if (e && !start) return fail(e, P2PG_ERR_ARG, "set_sources_at: need M > 0, src and start");
  return set_sources(e, "set_sources_at", M, src, start);
}

int p2pg_originate(p2pg_engine* e, int64_t n, const int32_t* msg, const int32_t* peer, int32_t round) {
  if (!e || n < 0 || (n > 0 && (!msg || !peer))) return fail(e, P2PG_ERR_ARG, "originate: bad arguments");
  if (!e->have_state) return fail(e, P2PG_ERR_STATE, "originate: no sources set");
  if (e->begun) return fail(e, P2PG_ERR_STATE, "originate: a round has begun (step_begin)");
  if (partitioned(e)) return fail(e, P2PG_ERR_STATE, "originate: not on a vertex-partitioned rank");
  if (!e->failed.empty()) return fail(e, P2PG_ERR_STATE, "originate: " + e->failed);
  if (round < std::max<int32_t>(1, e->round))
    return fail(e, P2PG_ERR_ARG, "originate: round " + std::to_string(round) + " is not ahead (the next round to run is " +
                                     std::to_string(e->round) + ", and round 0 belongs to p2pg_set_sources_at)");
  std::vector<int32_t> ms(msg, msg + n);
  for (int64_t i = 0; i < n; ++i) {
    if (msg[i] < 0 || msg[i] >= e->M) return fail(e, P2PG_ERR_ARG, "originate: message out of range");
    if (peer[i] < 0 || peer[i] >= e->V) return fail(e, P2PG_ERR_ARG, "originate: peer out of range");
    if (e->h_start[msg[i]] != -1)
      return fail(e, P2PG_ERR_ARG, "originate: message " + std::to_string(msg[i]) + " is scheduled already (round " +
                                       std::to_string(e->h_start[msg[i]]) + ")");
  }
  std::sort(ms.begin(), ms.end());
  if (std::adjacent_find(ms.begin(), ms.end()) != ms.end())
    return fail(e, P2PG_ERR_ARG, "originate: a message is listed twice");
  for (int64_t i = 0; e->down_on && i < n; ++i)
    if (downtime::offline(round, e->h_down_from[peer[i]], e->h_down_until[peer[i]]))
      return fail(e, P2PG_ERR_ARG, "originate: peer " + std::to_string(peer[i]) + " is offline in round " +
                                       std::to_string(round) + " (p2pg_set_downtime)");
  if (n == 0) return P2PG_OK;
  for (int64_t i = 0; i < n; ++i) {
    e->h_src[msg[i]] = peer[i];
    e->h_start[msg[i]] = round;
  }
  int rc = upload_schedule(e);
  if (rc) return rc;
  if (e->ttl_on && (rc = upload_expiry(e))) return rc;  // (the new starts fix their expiry rounds)
  if (e->pol_on && (rc = upload_exempt(e))) return rc;  // (and the policy's exempt rounds)
  e->done = false;  // (an engine that had gone quiet runs on: a start lies ahead)
  return P2PG_OK;
}

int p2pg_set_ttl(p2pg_engine* e, int32_t M, const int32_t* ttl) {
  if (!e) return fail(e, P2PG_ERR_ARG, "set_ttl: no engine");
  if (!e->have_state) return fail(e, P2PG_ERR_STATE, "set_ttl: no sources set");
  if (M != e->M) return fail(e, P2PG_ERR_ARG, "set_ttl: M differs from the engine's message count");
  bool finite = false;
  for (int32_t m = 0; ttl && m < M; ++m) {
    if (ttl[m] < -1 || ttl[m] > (1 << 30))
      return fail(e, P2PG_ERR_ARG, "set_ttl: a hop limit must lie in [-1, 2^30]");
    finite |= ttl[m] >= 0;
  }
  if (partitioned(e))
    return fail(e, P2PG_ERR_STATE, "set_ttl: hop limits are not available on a vertex-partitioned rank");
  if (e->begun) return fail(e, P2PG_ERR_STATE, "set_ttl: a round has begun (step_begin)");
  if (e->round > 0) return fail(e, P2PG_ERR_STATE, "set_ttl: a round has run (set the hop limits before round 0, or after p2pg_reset)");
  if (!e->failed.empty()) return fail(e, P2PG_ERR_STATE, "set_ttl: " + e->failed);
  if (finite && e->ae.on())
    return fail(e, P2PG_ERR_STATE, "set_ttl: hop limits are not available together with anti-entropy "
                                   "(p2pg_set_anti_entropy): a pulled message's remaining budget is no function of the round");
  if (finite && e->ns_win.on())
    return fail(e, P2PG_ERR_STATE, "set_ttl: hop limits are not available together with a netsplit "
                                   "(p2pg_set_netsplit): their held-back pushes would need the cut as well");
  if (!finite && e->h_ttl.empty()) return P2PG_OK;  // nothing set, nothing to remove
  if (finite)
    e->h_ttl.assign(ttl, ttl + M);
  else
    e->h_ttl.clear();  // all -1 (or NULL): the engine without this call
  const int rc = upload_expiry(e);
  return rc || !e->pol_on ? rc : upload_exempt(e);
}

int p2pg_set_relay_policy(p2pg_engine* e, int64_t V, const uint32_t* thr, uint64_t seed) {
  if (!e) return fail(e, P2PG_ERR_ARG, "set_relay_policy: no engine");
  if (!e->d_rowptr) return fail(e, P2PG_ERR_STATE, "set_relay_policy: load a graph first");
  if (V != e->V) return fail(e, P2PG_ERR_ARG, "set_relay_policy: V differs from the engine's peer count");
  if (partitioned(e))
    return fail(e, P2PG_ERR_STATE, "set_relay_policy: a relay policy is not available on a vertex-partitioned rank");
  if (e->begun) return fail(e, P2PG_ERR_STATE, "set_relay_policy: a round has begun (step_begin)");
  if (e->have_state && e->round > 0)
    return fail(e, P2PG_ERR_STATE, "set_relay_policy: a round has run (set the policy before round 0, or after p2pg_reset)");
  if (!e->failed.empty()) return fail(e, P2PG_ERR_STATE, "set_relay_policy: " + e->failed);
  bool any = false;
  for (int64_t v = 0; thr && v < V; ++v) any |= thr[v] != 0u;
  if (any && e->ae.on())
    return fail(e, P2PG_ERR_STATE, "set_relay_policy: a relay policy is not available together with anti-entropy "
                                   "(p2pg_set_anti_entropy)");
  if (any && e->ns_win.on())
    return fail(e, P2PG_ERR_STATE, "set_relay_policy: a relay policy is not available together with a netsplit "
                                   "(p2pg_set_netsplit): its held-back pushes would need the cut as well");
  if (!any && !e->pol_on) return P2PG_OK;  // nothing set, nothing to remove
  HIPCHK(e, hipSetDevice(e->cfg.device));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (any) {
    uint32_t* d = nullptr;
    HIPCHK(e, hipMalloc((void**)&d, sizeof(uint32_t) * (size_t)V));
    const hipError_t x = hipMemcpy(d, thr, sizeof(uint32_t) * (size_t)V, hipMemcpyHostToDevice);
    if (x != hipSuccess) {
      (void)hipFree(d);
      return fail(e, P2PG_ERR_HIP, std::string("set_relay_policy: ") + hipGetErrorString(x));
    }
    dfree(e->d_thr);
    e->d_thr = d;
    e->h_thr.assign(thr, thr + V);
    e->pol_seed = seed;
    e->pol_on = true;
  } else {  // all zero (or NULL): the engine without this call
    dfree(e->d_thr);
    e->h_thr.clear();
    e->pol_seed = 0;
    e->pol_on = false;
  }
  e->pol_pending = -1;
  return upload_exempt(e);
}

int p2pg_set_downtime(p2pg_engine* e, int64_t V, const int32_t* from, const int32_t* until) {
  if (!e) return fail(e, P2PG_ERR_ARG, "set_downtime: no engine");
  if (!e->d_rowptr) return fail(e, P2PG_ERR_STATE, "set_downtime: load a graph first");
  if (V != e->V) return fail(e, P2PG_ERR_ARG, "set_downtime: V differs from the engine's peer count");
  const bool any = downtime::any(V, from);
  if (any) {
    if (!until) return fail(e, P2PG_ERR_ARG, "set_downtime: need until with from");
    downtime::Bad what = downtime::OK;
    const int64_t v = downtime::first_bad(V, from, until, &what);
    if (v >= 0)
      return fail(e, P2PG_ERR_ARG, "set_downtime: peer " + std::to_string(v) +
                                       (what == downtime::BAD_FROM ? ": from below -1" : ": until is not above from"));
  } else {
    for (int64_t v = 0; from && v < V; ++v)
      if (from[v] < -1) return fail(e, P2PG_ERR_ARG, "set_downtime: peer " + std::to_string(v) + ": from below -1");
  }
  if (partitioned(e))
    return fail(e, P2PG_ERR_STATE, "set_downtime: peer downtime is not available on a vertex-partitioned rank");
  if (e->begun) return fail(e, P2PG_ERR_STATE, "set_downtime: a round has begun (step_begin)");
  if (e->have_state && e->round > 0)
    return fail(e, P2PG_ERR_STATE, "set_downtime: a round has run (set the downtime before round 0, or after p2pg_reset)");
  if (!e->failed.empty()) return fail(e, P2PG_ERR_STATE, "set_downtime: " + e->failed);
  if (any && e->have_state) {  // originations at an offline peer are refused
    const int64_t m = downtime::first_refused(e->M, e->h_src.data(), e->h_start.data(), from, until);
    if (m >= 0)
      return fail(e, P2PG_ERR_ARG, "set_downtime: the origin of message " + std::to_string(m) +
                                       " would be offline in its start round");
  }
  if (!any && !e->down_on) return P2PG_OK;  // nothing set, nothing to remove
  HIPCHK(e, hipSetDevice(e->cfg.device));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (any) {
    int32_t *df = nullptr, *du = nullptr;
    const size_t nb = sizeof(int32_t) * (size_t)V;
    hipError_t x = hipMalloc((void**)&df, nb);
    if (x == hipSuccess) x = hipMalloc((void**)&du, nb);
    if (x == hipSuccess) x = hipMemcpy(df, from, nb, hipMemcpyHostToDevice);
    if (x == hipSuccess) x = hipMemcpy(du, until, nb, hipMemcpyHostToDevice);
    if (x != hipSuccess) {
      if (df) (void)hipFree(df);
      if (du) (void)hipFree(du);
      return fail(e, P2PG_ERR_HIP, std::string("set_downtime: ") + hipGetErrorString(x));
    }
    dfree(e->d_down_from);
    dfree(e->d_down_until);
    e->d_down_from = df;
    e->d_down_until = du;
    e->h_down_from.assign(from, from + V);
    e->h_down_until.assign(until, until + V);
    e->down_sweep.build(V, from, until);
    e->down_on = true;
  } else {  // all -1 (or NULL): the engine without this call
    dfree(e->d_down_from);
    dfree(e->d_down_until);
    e->h_down_from.clear();
    e->h_down_until.clear();
    e->down_sweep.build(0, nullptr, nullptr);
    e->down_on = false;
  }
  return P2PG_OK;
}

int p2pg_peer_offline(int32_t round, int32_t from, int32_t until) {
  return downtime::offline(round, from, until) ? 1 : 0;
}

int p2pg_set_netsplit(p2pg_engine* e, int64_t V, const int32_t* side, int32_t cut_from, int32_t cut_until) {
  if (!e) return fail(e, P2PG_ERR_ARG, "set_netsplit: no engine");
  if (!e->d_rowptr) return fail(e, P2PG_ERR_STATE, "set_netsplit: load a graph first");
  if (V != e->V) return fail(e, P2PG_ERR_ARG, "set_netsplit: V differs from the engine's peer count");
  if (side) {  // (side = NULL removes the setting whatever the window)
    const netsplit::Bad w = netsplit::check_window(cut_from, cut_until);
    if (w != netsplit::OK)
      return fail(e, P2PG_ERR_ARG, w == netsplit::BAD_FROM ? "set_netsplit: cut_from below 0" : "set_netsplit: cut_until below 0");
    const int64_t v = netsplit::first_bad_side(V, side);
    if (v >= 0) return fail(e, P2PG_ERR_ARG, "set_netsplit: peer " + std::to_string(v) + ": a negative side");
  }
  if (partitioned(e))
    return fail(e, P2PG_ERR_STATE, "set_netsplit: a netsplit is not available on a vertex-partitioned rank");
  if (e->begun) return fail(e, P2PG_ERR_STATE, "set_netsplit: a round has begun (step_begin)");
  if (e->have_state && e->round > 0)
    return fail(e, P2PG_ERR_STATE, "set_netsplit: a round has run (set the netsplit before round 0, or after p2pg_reset)");
  if (!e->failed.empty()) return fail(e, P2PG_ERR_STATE, "set_netsplit: " + e->failed);
  const bool any = netsplit::any(V, e->h_rowptr.data(), e->h_colidx.data(), side, cut_from, cut_until);
  if (any && !e->h_ttl.empty())
    return fail(e, P2PG_ERR_STATE, "set_netsplit: not available together with hop limits (p2pg_set_ttl)");
  if (any && e->pol_on)
    return fail(e, P2PG_ERR_STATE, "set_netsplit: not available together with a relay policy (p2pg_set_relay_policy)");
  if (any && e->arr_round >= 0)
    return fail(e, P2PG_ERR_STATE, "set_netsplit: not available after a topology update (p2pg_update_edges)");
  if (!any && !e->ns_win.on()) return P2PG_OK;  // nothing set, nothing to remove
  HIPCHK(e, hipSetDevice(e->cfg.device));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (any) {
    int32_t* ds = nullptr;
    const size_t nb = sizeof(int32_t) * (size_t)V;
    hipError_t x = hipMalloc((void**)&ds, nb);
    if (x == hipSuccess) x = hipMemcpy(ds, side, nb, hipMemcpyHostToDevice);
    if (x != hipSuccess) {
      if (ds) (void)hipFree(ds);
      return fail(e, P2PG_ERR_HIP, std::string("set_netsplit: ") + hipGetErrorString(x));
    }
    dfree(e->d_side);
    e->d_side = ds;
    e->ns_win.from = cut_from;
    e->ns_win.until = cut_until;
  } else {  // no sides, an empty window or no crossing connection: the engine without this call
    dfree(e->d_side);
    e->ns_win = netsplit::Window{};
  }
  return P2PG_OK;
}

int p2pg_link_cut(int32_t round, int32_t side_a, int32_t side_b, int32_t cut_from, int32_t cut_until) {
  return netsplit::link_cut(round, side_a, side_b, cut_from, cut_until) ? 1 : 0;
}

int p2pg_set_anti_entropy(p2pg_engine* e, int32_t first, int32_t last, int32_t period, uint64_t seed) {
  if (!e) return fail(e, P2PG_ERR_ARG, "set_anti_entropy: no engine");
  if (!e->d_rowptr) return fail(e, P2PG_ERR_STATE, "set_anti_entropy: load a graph first");
  switch (anti_entropy::check(first, last, period)) {
    case anti_entropy::BAD_PERIOD: return fail(e, P2PG_ERR_ARG, "set_anti_entropy: period below 0");
    case anti_entropy::BAD_FIRST: return fail(e, P2PG_ERR_ARG, "set_anti_entropy: first below 0");
    case anti_entropy::BAD_LAST: return fail(e, P2PG_ERR_ARG, "set_anti_entropy: last below first");
    case anti_entropy::OK: break;
  }
  if (partitioned(e))
    return fail(e, P2PG_ERR_STATE, "set_anti_entropy: anti-entropy is not available on a vertex-partitioned rank");
  if (e->begun) return fail(e, P2PG_ERR_STATE, "set_anti_entropy: a round has begun (step_begin)");
  if (e->have_state && e->round > 0)
    return fail(e, P2PG_ERR_STATE, "set_anti_entropy: a round has run (set it before round 0, or after p2pg_reset)");
  if (!e->failed.empty()) return fail(e, P2PG_ERR_STATE, "set_anti_entropy: " + e->failed);
  if (period > 0 && !e->h_ttl.empty())
    return fail(e, P2PG_ERR_STATE, "set_anti_entropy: not available together with hop limits (p2pg_set_ttl): a pulled "
                                   "message's remaining budget is no function of the round");
  if (period > 0 && e->pol_on)
    return fail(e, P2PG_ERR_STATE, "set_anti_entropy: not available together with a relay policy (p2pg_set_relay_policy)");
  if (period == 0) {  // the engine without this call
    if (!e->ae.on()) return P2PG_OK;
    HIPCHK(e, hipSetDevice(e->cfg.device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    free_pull(e);
    e->ae = anti_entropy::Setting{};
    e->ae_seed = 0;
    return P2PG_OK;
  }
  e->ae.first = first;
  e->ae.last = last;
  e->ae.period = period;
  e->ae_seed = seed;
  e->pull_round = -1;
  e->pull_log.clear();
  return P2PG_OK;
}

int32_t p2pg_pull_partner_slot(uint32_t round, uint32_t peer, uint32_t deg, uint64_t seed) {
  if (deg == 0u) return -1;
  return (int32_t)pull_partner_slot(round, peer, deg, (uint32_t)seed, (uint32_t)(seed >> 32));
}

int p2pg_get_pull_stats(p2pg_engine* e, int64_t cap, p2pg_pull_stats* out, int64_t* n_out) {
  if (!e || cap < 0 || !n_out || (cap > 0 && !out)) return fail(e, P2PG_ERR_ARG, "get_pull_stats: bad arguments");
  const int64_t n = (int64_t)e->pull_log.size();
  for (int64_t i = 0; i < n && i < cap; ++i) out[i] = e->pull_log[i];
  *n_out = n;
  return P2PG_OK;
}

}  // extern "C"

namespace {

// Round 0's counters: the originations, from the host copies of the sources and the rows (the
// seed kernel counts nothing).  They depend on the sources and the graph only, so they are
// computed once per p2pg_set_sources / p2pg_load_csr rather than per run: a run's round 0 used to
// sort the sources on the host while the GPU waited (~0.25 ms per c4 step).
const SeedStats& seed_stats(p2pg_engine* e) {
  SeedStats& ss = e->seed;
  if (ss.ok) return ss;
  ss = SeedStats{};
  const bool gossip = e->cfg.mode == P2PG_MODE_GOSSIP;
  std::vector<int64_t> vs, vw;  // round 0's origins: the messages with start 0
  vs.reserve(e->M);
  vw.reserve(e->M);
  for (int32_t m = 0; m < e->M; ++m) {
    if (e->h_start[m] != 0) continue;
    const int64_t v = e->h_src[m];
    const int64_t d = e->h_rowptr[v + 1] - e->h_rowptr[v];
    if (!expires_in(e, m, 0))  // (ttl 0: the origin marks the message seen and sends nothing)
      ss.relays += gossip ? (uint64_t)std::min<int64_t>(d, e->cfg.fanout) : (uint64_t)d;
    vs.push_back(v);
    vw.push_back(v * e->W + (m >> 6));
  }
  ss.nw = (uint64_t)vs.size();
  std::sort(vs.begin(), vs.end());
  vs.erase(std::unique(vs.begin(), vs.end()), vs.end());
  std::sort(vw.begin(), vw.end());
  vw.erase(std::unique(vw.begin(), vw.end()), vw.end());
  ss.av = vs.size();
  ss.aw = vw.size();
  for (int64_t v : vs) ss.degact += (uint64_t)(e->h_rowptr[v + 1] - e->h_rowptr[v]);
  for (int64_t x : vw) {
    const int64_t v = x / e->W;
    ss.wedge += (uint64_t)(e->h_rowptr[v + 1] - e->h_rowptr[v]);
  }
  ss.ok = true;
  return ss;
}

// p2pg_reset's spare seen plane (p2pg_engine::seen_spare): allocated on first use; false when
// disabled or when the device has no room for it (then it stays disabled)
bool spare_ready(p2pg_engine* e) {
  if (!e->seen_spare_on || e->seen_spare_off) return false;
  if (e->seen_spare) return true;
  // only where it is cheap: a plane of at most 1/16 of the device (config 4: 5.1 GB of 288) with
  // room to spare, so that the copy never takes the memory a larger run (config 5's 51 GB planes,
  // several engines of one process) needs
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || e->plane_bytes > total_b / 16 ||
      free_b < 4 * e->plane_bytes) {
    (void)hipGetLastError();
    e->seen_spare_off = true;
    return false;
  }
  if (!e->side) {
    if (hipStreamCreateWithFlags(&e->side, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_spare, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_main, hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError();
      e->seen_spare_off = true;
      return false;
    }
  }
  if (hipMalloc((void**)&e->seen_spare, e->plane_bytes) != hipSuccess) {
    (void)hipGetLastError();
    e->seen_spare = nullptr;
    e->seen_spare_off = true;
    return false;
  }
  e->spare_pending = false;
  return true;
}

}  // namespace

extern "C" {

int p2pg_reset(p2pg_engine* e) {
  if (!e || !e->have_state) return fail(e, P2PG_ERR_STATE, "reset: no sources set");
  HIPCHK(e, hipSetDevice(e->cfg.device));
  DevState& s = e->st;
  if (!spare_ready(e)) {
    HIPCHK(e, hipMemsetAsync(s.seen, 0, e->plane_bytes, e->stream));
  } else {
    if (e->spare_pending) {  // the spare is zero once the side stream's zeroing has run
      HIPCHK(e, hipStreamWaitEvent(e->stream, e->ev_spare, 0));
      std::swap(s.seen, e->seen_spare);
    } else {  // (first reset with a spare: zero the plane in use here, the spare below)
      HIPCHK(e, hipMemsetAsync(s.seen, 0, e->plane_bytes, e->stream));
    }
    // the replaced plane: zeroed on the side stream after everything queued so far has read it
    HIPCHK(e, hipEventRecord(e->ev_main, e->stream));
    HIPCHK(e, hipStreamWaitEvent(e->side, e->ev_main, 0));
    HIPCHK(e, hipMemsetAsync(e->seen_spare, 0, e->plane_bytes, e->side));
    HIPCHK(e, hipEventRecord(e->ev_spare, e->side));
    e->spare_pending = true;
  }
  HIPCHK(e, hipMemsetAsync(s.S, 0, e->bm_bytes, e->stream));
  for (int i = 0; i < 2; ++i) HIPCHK(e, hipMemsetAsync(s.A[i], 0, e->bm_bytes, e->stream));
  if (s.next[0] && ((!e->done && e->round > 0) || e->consume_next)) {
    // an interrupted run may leave pushes / materialized arrivals in flight: clear them
    for (int i = 0; i < 2; ++i) {
      HIPCHK(e, hipMemsetAsync(s.next[i], 0, e->plane_bytes, e->stream));
      HIPCHK(e, hipMemsetAsync(s.T[i], 0, e->bm_bytes, e->stream));
    }
  }
  if (s.hop) {
    HIPCHK(e, hipMemsetAsync(s.hop, 0xFF, (size_t)e->V * e->M * sizeof(int32_t), e->stream));
    HIPCHK(e, hipMemsetAsync(s.parent, 0xFF, (size_t)e->V * e->M * sizeof(int32_t), e->stream));
  }
  if (tally_on(e)) {
    HIPCHK(e, hipMemsetAsync(e->d_treach, 0, sizeof(unsigned long long) * (size_t)e->M, e->stream));
    HIPCHK(e, hipMemsetAsync(e->d_thop, 0, sizeof(unsigned long long) * (size_t)e->M, e->stream));
    HIPCHK(e, hipMemsetAsync(e->d_tlast, 0xFF, sizeof(int32_t) * (size_t)e->M, e->stream));
    HIPCHK(e, hipMemsetAsync(e->d_tsent, 0, sizeof(unsigned long long) * (size_t)e->V, e->stream));
    HIPCHK(e, hipMemsetAsync(e->d_trecv, 0, sizeof(unsigned long long) * (size_t)e->V, e->stream));
  }
  if (cost_on(e)) {
    HIPCHK(e, hipMemsetAsync(e->d_csent, 0, sizeof(unsigned long long) * (size_t)e->M, e->stream));
    HIPCHK(e, hipMemsetAsync(e->d_crecv, 0, sizeof(unsigned long long) * (size_t)e->M, e->stream));
  }
  if (latency_on(e)) {
    HIPCHK(e, hipMemsetAsync(e->d_lhist, 0, sizeof(unsigned long long) * (size_t)e->M * (size_t)e->lat_bins, e->stream));
    HIPCHK(e, hipMemsetAsync(e->d_lpeer, 0, sizeof(PeerLat) * (size_t)e->V, e->stream));
  }
  e->tally_pending = -1;
  e->tally_read_at = -1;
  e->exp_pending = e->exp_final = -1;  // (the hop limits themselves stay and are replayed)
  e->pol_pending = -1;                 // (and so does the relay policy)
  e->pull_round = -1;                  // (and the anti-entropy setting; the run's records go)
  e->pull_log.clear();
  e->round = 0;
  e->done = false;
  e->failed.clear();
  e->stats_clear = true;
  e->begun = false;
  e->auto_round = -1;
  e->frontier_kept = true;
  e->frontier_kept_prev = true;
  e->hist = rp::RoundHistory{};
  e->consume_next = false;
  e->total_relays = 0;
  e->sent_last = e->lost_last = 0;
  free_arr(e);
  // (a previous run's unresolved launch timings belong to it, not to the next one)
  e->ev_cls.clear();
  for (int i = 0; i < P2PG_KCLASS_N; ++i) {
    e->kms[i] = 0;
    e->klaunch[i] = 0;
  }
  return P2PG_OK;
}

}  // extern "C"

namespace {

// Can this round's pull / update run in two phases (interior peers, then border peers)?
// Vertex-partitioned ranks with ghosts, rounds r >= 1 of the flood pull or the gossip update.
bool split_round(const p2pg_engine* e) {
  return e->d_border && e->round > 0 && !e->consume_next &&
         (e->cfg.mode == P2PG_MODE_FLOOD || !e->hist.last_push_e);
}

// The end of round e->round with counters tot (p2pg_step, and every reported round of a decay
// batch): fills out, rolls the schedule's history, takes the round's sends and frontier state in.
// pushed_e: its gossip pushes went (or, held back, will go) to E; rows_whole: its frontier rows
// were stored whole; lost: its counted lost sends.  Returns whether the run goes on: receipts in
// flight, or a scheduled start at or after the next round.
bool close_round(p2pg_engine* e, const uint64_t* tot, int32_t push_form, bool pushed_e, bool rows_whole,
                 uint64_t lost, p2pg_round_stats* out) {
  // (anti-entropy: a request round at or ahead, or an exchange in flight, keeps the run going)
  const bool active = tot[ST_NEW] != 0 || start_ahead(e, e->round + 1) || e->ae.arrival_ahead((int64_t)e->round + 1);
  if (out) {
    out->round = e->round;
    out->active = active ? 1 : 0;
    out->new_deliveries = tot[ST_NEW];
    out->relays = tot[ST_RELAYS];
    out->active_vertices = tot[ST_ACTIVE_V];
    out->active_words = tot[ST_ACTIVE_W];
    out->wedges = tot[ST_WEDGES];
    out->deg_active = tot[ST_DEG_ACT];
    out->scatter_words = tot[ST_SCATTER];
    out->touched_words = tot[ST_AUX];
    out->push_form = push_form;
    out->received_exact = received_exact(e, e->round) ? 1 : 0;
    out->received = e->round == 0 ? 0 : e->sent_last - e->lost_last;
  }
  rp::advance(e->hist, {tot[ST_NEW], tot[ST_ACTIVE_V], tot[ST_ACTIVE_W], tot[ST_SCATTER]}, pushed_e);
  e->sent_last = tot[ST_RELAYS];
  e->lost_last = lost;
  e->total_relays += tot[ST_RELAYS];
  e->frontier_kept_prev = e->frontier_kept;
  e->frontier_kept = rows_whole || tot[ST_NEW] == 0;
  e->round += 1;
  if (!active && !(e->cfg.flags & P2PG_FLAG_NO_AUTOSTOP)) e->done = true;
  return active;
}

}  // namespace

extern "C" {

int p2pg_step_begin(p2pg_engine* e) {
  if (!e || !e->have_state) return fail(e, P2PG_ERR_STATE, "step_begin: no sources set");
  if (!e->failed.empty()) return fail(e, P2PG_ERR_STATE, "step_begin: " + e->failed);
  if (e->begun) return fail(e, P2PG_ERR_STATE, "step_begin: the round has begun already");
  // a rank-local graph marks its ghost slots REV_GHOST | id, which only the PART kernels (global
  // ids set) know: the one-GPU kernels would index E with them
  if ((e->cfg.flags & P2PG_FLAG_LOCAL_GRAPH) && !e->d_gid)
    return fail(e, P2PG_ERR_STATE, "step_begin: a local-graph engine needs p2pg_set_global_ids first");
  if (e->done) return P2PG_OK;
  HIPCHK(e, hipSetDevice(e->cfg.device));
  DevState& s = e->st;
  {  // hop limits: the last round's expired receipts send nothing (before anything reads its sends)
    const int xrc = finalize_expiry(e, true);
    if (xrc) return xrc;
  }
  {  // tallies: the last round's sends are final; its frontiers are overwritten from here on
    const hipError_t x = flush_peer_tally(e, graph(e));
    if (x != hipSuccess) return fail(e, P2PG_ERR_HIP, std::string("step (peer counters): ") + hipGetErrorString(x));
  }
  if (e->stats_clear) {
    HIPCHK(e, hipMemsetAsync(s.stats, 0, STAT_BYTES, e->stream));
    std::memset(e->stats_base, 0, sizeof(e->stats_base));
    e->stats_clear = false;
  }
  e->begun = true;
  if (!split_round(e)) return P2PG_OK;
  // phase 0: peers without a ghost neighbour, which need none of the rows still in transit
  const DevGraph g = graph(e);
  RoundParams p = params(e);
  p.border = e->d_border;
  p.phase = 0;
  if (e->cfg.mode == P2PG_MODE_FLOOD)
    return timed(e, 1, [&] { return launch_flood_pull(g, s, p, e->hp, e->stream); });
  return timed(e, 4, [&] { return launch_gossip_update(g, s, p, e->stream); });
}

int p2pg_step(p2pg_engine* e, p2pg_round_stats* out) {
  if (!e || !e->have_state) return fail(e, P2PG_ERR_STATE, "step: no sources set");
  if (!e->failed.empty()) return fail(e, P2PG_ERR_STATE, "step: " + e->failed);
  if (e->done) {
    e->begun = false;
    if (out) {
      std::memset(out, 0, sizeof(*out));
      out->round = e->round;
    }
    return 0;
  }
  int rc;
  if (!e->begun && (rc = p2pg_step_begin(e))) return rc;
  HIPCHK(e, hipSetDevice(e->cfg.device));
  DevState& s = e->st;
  if (e->arr_round >= 0 && e->round > e->arr_round) {
    if (deferred_on(e)) HIPCHK(e, hipStreamSynchronize(e->stream));  // (the passes queued above read it)
    free_arr(e);
  }
  const DevGraph g = graph(e);
  RoundParams p = params(e);
  if (split_round(e)) {  // phase 0 ran in step_begin: the border peers now
    p.border = e->d_border;
    p.phase = 1;
  }
  e->begun = false;
  const bool gossip = e->cfg.mode == P2PG_MODE_GOSSIP;
  // What this round is (round_plan.h).  Its originations (start rounds > 0) are injected into the
  // frontier rows after the receive pass and before the pushes.  Hop limits that expire in it
  // (p2pg_set_ttl) and a relay policy (p2pg_set_relay_policy: every round after round 0, any of its
  // first receipts may be muted) correct its counters below, and its sends -- a gossip round's
  // push -- wait until they are final (finalize_expiry).
  const p2pg_engine::SchedRound* const orig = sched_round(e, e->round);
  const int64_t xi = expiry_index(e, e->round);
  const bool pol = e->pol_on && e->round > 0;
  const rp::RoundCaps caps = round_caps(e);
  rp::RoundFacts facts;
  facts.round = e->round;
  facts.consume_next = e->consume_next;
  facts.split = p.phase >= 0;
  facts.origination = orig != nullptr;
  facts.expiry = xi >= 0;
  facts.policy = pol;
  // Peer downtime: somebody is offline in this round (round 0 has no receive pass, and an
  // origination at an offline peer is refused, so it has nothing to undo).
  facts.offline = e->down_on && e->round > 0 && e->down_sweep.offline_round(e->round);
  // Anti-entropy: the replies of request round e->round - 2 arrive in this round.
  const bool pull = e->ae.on() && e->ae.arrival_round(e->round);
  facts.pull = pull;
  // Netsplit: the cut acts on this round -- a flood round receives over cut connections (a cut
  // round > 0), a gossip round's sends arrive in a cut round.
  facts.cut = gossip ? e->ns_win.cut_sends(e->round) : e->round > 0 && e->ns_win.cut_round(e->round);
  facts.skip_frontier = e->skip_frontier;
  const rp::RoundPlan plan = rp::plan_round(e->hist, e->rules, caps, facts);
  p.store_f = plan.store_f;
  if (pull) {
    // before the receive pass, while seen is the state at the end of the last round: the partner
    // draws, the losses, and what each reply carries (relay_pull.hip)
    if ((rc = ensure_pull(e))) return rc;
    HIPCHK(e, hipMemsetAsync(e->d_pull_cnt, 0, PULL_BYTES, e->stream));
    e->pull_round = e->round;
    if ((rc = timed(e, 0, [&] { return launch_pull_gather(g, s, p, down(e), cut(e), pull_of(e, e->round), e->stream); })))
      return rc;
  }
  uint64_t tot[STAT_N] = {0};
  // round 0's counters are the host's: origination stats from the host copy of the sources
  // (computed once per sources and graph)
  auto host_stats = [&] {
    const SeedStats& ss = seed_stats(e);
    tot[ST_NEW] = ss.nw;
    tot[ST_RELAYS] = ss.relays;
    tot[ST_ACTIVE_V] = ss.av;
    tot[ST_ACTIVE_W] = ss.aw;
    tot[ST_WEDGES] = ss.wedge;
    tot[ST_DEG_ACT] = ss.degact;
  };
  switch (plan.receive) {
    case rp::Receive::Seed:
      if ((rc = timed(e, 0, [&] { return launch_zero_rows(s.F[0], e->W, e->d_src, e->M, e->stream); }))) return rc;
      if (s.AW[0])
        if ((rc = timed(e, 0, [&] { return launch_zero_rows(s.AW[0], 1, e->d_src, e->M, e->stream); }))) return rc;
      if ((rc = timed(e, 0, [&] { return launch_seed(s, e->d_src, e->M, e->stream); }))) return rc;
      host_stats();
      break;
    case rp::Receive::Consume:  // arrivals materialized into row pushes (topology update / snapshot)
    case rp::Receive::Update:
      if ((rc = timed(e, 4, [&] { return launch_gossip_update(g, s, p, e->stream); }))) return rc;
      e->consume_next = false;
      break;
    case rp::Receive::FloodPull:
      if ((rc = timed(e, 1, [&] { return launch_flood_pull(g, s, p, e->hp, e->stream); }))) return rc;
      break;
    case rp::Receive::FloodPullCut:  // the copies over cut connections do not arrive (relay_netsplit.hip)
      if ((rc = timed(e, 1, [&] { return launch_pull_cut(g, s, p, cut(e), e->hp, e->stream); }))) return rc;
      break;
    case rp::Receive::GossipPull:  // (a partitioned rank gets here only if part_dense)
      if ((rc = timed(e, 5, [&] {
             hipError_t r = launch_gossip_pull(g, s, p, e->hp, e->stream);
             return r != hipSuccess || !e->d_gid ? r : launch_clear_arrivals(s, p.round, e->V, e->stream);
           })))
        return rc;
      break;
    case rp::Receive::Fused:
      if ((rc = timed(e, 7, [&] { return launch_fused_round(e, g, p); }))) return rc;
      break;
    case rp::Receive::UpdatePush:  // (timed with the store pushes)
      if ((rc = timed(e, 6, [&] {
             return launch_gossip_update_push(g, s, p, e->d_hub_big, e->n_hub_big, e->d_wide_big,
                                              e->n_wide_big, e->stream);
           })))
        return rc;
      break;
  }
  if (facts.offline)  // the receipts the pass made at offline peers did not happen (relay_offline.hip)
    if ((rc = timed(e, 0, [&] { return launch_offline(g, s, p, down(e), e->stream); }))) return rc;
  if (pull)  // what the replies carried and no relay copy delivered: first receipts of this round
    if ((rc = timed(e, 0, [&] { return launch_pull_apply(g, s, p, pull_of(e, e->round), e->stream); }))) return rc;
  if (orig)  // Node.send_to_nodes at the origins of this round (node.py:106-112)
    if ((rc = timed(e, 0, [&] {
           return launch_originate(g, s, p, e->d_sched_peer, e->d_sched_msg, e->d_sched_grp, orig->g_lo,
                                   orig->g_hi - orig->g_lo, e->stream);
         })))
      return rc;
  if (s.hop)
    if ((rc = timed(e, 3, [&] {
           return launch_record(graph_for_arrivals(e, e->round), s, p, pull_of(e, e->round), cut(e), e->stream);
         })))
      return rc;
  auto read_stats = [&]() -> int {
    HIPCHK(e, hipMemcpyAsync(e->h_stats, s.stats, STAT_BYTES, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, round_sync(e));
    int r2 = resolve_timings(e);
    if (r2) return r2;
    for (int i = 0; i < STAT_N; ++i) tot[i] = 0;
    for (int sh = 0; sh < STAT_SHARDS; ++sh)
      for (int i = 0; i < STAT_N; ++i)
        tot[i] += e->h_stats[sh * STAT_N + i] - e->stats_base[sh * STAT_N + i];
    if (e->round == 0) host_stats();
    return P2PG_OK;
  };
  // did this round's pushes go to E?  The fused and update+push launches pushed every source
  bool pushed_e = plan.push == rp::Push::Made;
  if (gossip && plan.push == rp::Push::AtomicCut) {
    // the sends arrive in a cut round: row atomics, the picks over cut connections left out
    p.dedup_push = rp::push_dedup(e->hist, e->rules);
    if ((rc = timed(e, 2, [&] { return launch_push_cut(g, s, p, cut(e), e->stream); }))) return rc;
  } else if (gossip && !pushed_e && !plan.held) {
    // the push the plan names, after the round's own counters where it asks for them
    if (plan.mid_read && (rc = read_stats())) return rc;
    const bool use_e =
        rp::resolve_push(plan, e->rules, tot[ST_ACTIVE_W], tot[ST_ACTIVE_V]) == rp::Push::Edge;
    if (!use_e && caps.sparse_scatter) p.dedup_push = rp::push_dedup(e->hist, e->rules);
    const uint64_t list_words = plan.list == rp::PushList::Counters ? tot[ST_ACTIVE_W] : e->hist.prev_sw;
    if ((rc = timed(e, use_e ? 6 : 2, [&] {
           return use_e ? launch_gossip_scatter(g, s, p, e->d_hub, e->n_hub, true, e->stream,
                                                e->d_hub_big, e->n_hub_big, e->d_wide_big,
                                                e->n_wide_big)
                        : launch_scatter_atomic(e, g, p, list_words);
         })))
      return rc;
    pushed_e = use_e;
  }
  if (e->auto_buf && e->d_seg_cnt) {
    // partitioned ranks: pack this round's live boundary rows now, so the one synchronisation
    // below (the round counters) also covers the pack and its counts -- no second drain of the
    // stream before the records leave (p2pg_set_exchange_buffer)
    const bool fwd = e->auto_plane == 0;
    const int nseg = (int)e->send_seg.size() - 1;
    HIPCHK(e, hipMemsetAsync(e->d_seg_cnt, 0, sizeof(unsigned long long) * P2PG_MAX_RANKS, e->stream));
    hipError_t r = launch_pack_live(s, e->auto_plane, e->round, fwd ? e->d_send : e->d_recv,
                                    fwd ? e->n_send : e->n_recv, fwd ? e->d_send_seg : e->d_recv_seg,
                                    nseg, e->d_seg_cnt, (int64_t*)e->auto_buf, e->stream);
    if (r == hipSuccess)
      r = hipMemcpyAsync(e->h_seg_cnt, e->d_seg_cnt, sizeof(unsigned long long) * nseg,
                         hipMemcpyDeviceToHost, e->stream);
    if (r != hipSuccess) return fail(e, P2PG_ERR_HIP, std::string("step (exchange pack): ") + hipGetErrorString(r));
    e->auto_round = e->round;
  }
  if (latency_on(e)) {
    // this round's first receipts by relative hop: one column count of its frontier rows, whose
    // shards the latency fold bins per message -- and, on a tally engine, the tally's fold reads
    // next and leaves zero -- then the per-peer pass over the same rows.  Stream order only.
    hipError_t x = launch_frontier_count(s.F[e->round & 1], s.A[e->round & 1], e->V, e->W, e->d_tscratch, e->stream);
    if (x == hipSuccess)
      x = launch_latency_fold(e->d_tscratch, e->W, e->M, e->round, e->d_lstart, e->lat_bins, e->d_lhist, !tally_on(e),
                              e->stream);
    if (x == hipSuccess && tally_on(e))
      x = launch_tally_fold(e->d_tscratch, e->W, e->M, e->round, nullptr, e->d_treach, e->d_thop, e->d_tlast,
                            e->stream);
    if (x == hipSuccess)
      x = launch_peer_latency(s, e->V, e->round, e->lat_B ? e->d_lplanes : nullptr, e->lat_B, e->d_lpeer, e->stream);
    if (x != hipSuccess) return fail(e, P2PG_ERR_HIP, std::string("step (delivery latency): ") + hipGetErrorString(x));
  } else if (tally_on(e)) {
    // this round's first receipts per message: column counts of its frontier rows (whole on a
    // tally engine); its sends wait for the next boundary (flush_peer_tally)
    const hipError_t x = launch_column_count(s.F[e->round & 1], s.A[e->round & 1], e->V, e->W, e->M, e->round,
                                             e->d_tscratch, nullptr, e->d_treach, e->d_thop, e->d_tlast,
                                             e->stream);
    if (x != hipSuccess) return fail(e, P2PG_ERR_HIP, std::string("step (message tallies): ") + hipGetErrorString(x));
  }
  if (deferred_on(e)) e->tally_pending = e->round;
  if (xi >= 0) {
    // hop limits: the receive pass and k_originate counted every first receipt's relays; the
    // expired ones leave this round's total (round 0's are the host's: seed_stats).  Their frontier
    // bits stand until the round's sends are final -- they are the round's deliveries
    if (e->round > 0) {
      const uint64_t* X = e->d_exp + 2 * (size_t)xi * e->W;
      if ((rc = timed(e, 0, [&] { return launch_expire(g, s, p, X, X + e->W, false, e->stream); }))) return rc;
    }
    e->exp_pending = e->round;
  }
  if (pol) {
    // relay policy: the muted first receipts' relays leave this round's total as well (never an
    // origination's, never twice for a receipt a hop limit cancelled: the round's exempt mask)
    if ((rc = timed(e, 0, [&] {
           return launch_policy(g, s, p, e->d_thr, e->pol_seed, exempt_mask(e, e->round), false, e->stream);
         })))
      return rc;
    e->pol_pending = e->round;
  }
  // (an expiry or policy round's lost sends are counted once its bits are cleared: finalize_expiry)
  const bool cnt_lost = count_lost_on(e) && !plan.held;
  if (cnt_lost) {  // this round's lost sends: the next round's arrivals are its sends minus them
    hipError_t x = enqueue_lost_count(e, g, graph_for_arrivals(e, e->round), e->round);
    if (x != hipSuccess) return fail(e, P2PG_ERR_HIP, std::string("step (lost sends): ") + hipGetErrorString(x));
  }
  if (pull)
    HIPCHK(e, hipMemcpyAsync(e->h_pull_cnt, e->d_pull_cnt, PULL_BYTES, hipMemcpyDeviceToHost, e->stream));
  if ((rc = read_stats())) return rc;
  std::memcpy(e->stats_base, e->h_stats, sizeof(e->stats_base));  // the next round counts from here
  if (pull) {  // the exchange is complete: its record (p2pg_get_pull_stats)
    uint64_t c[PULL_N] = {0};
    for (int sh = 0; sh < STAT_SHARDS; ++sh)
      for (int i = 0; i < PULL_N; ++i) c[i] += e->h_pull_cnt[sh * PULL_N + i];
    p2pg_pull_stats rec;
    rec.request_round = e->round - 2;
    rec.reserved = 0;
    rec.requests = c[PL_REQUESTS];
    rec.requests_lost = c[PL_REQUESTS_LOST];
    rec.replies = c[PL_REPLIES];
    rec.replies_lost = c[PL_REPLIES_LOST];
    rec.repaired = c[PL_REPAIRED];
    e->pull_log.push_back(rec);
  }
  if ((rc = check_scatter_list(e, e->h_stats[STAT_COUNT]))) return rc;
  if (plan.held) {
    // the form of the held-back push, by the rule of the rounds that push at once (the density of
    // the round's own frontier, before the muting); the next round pulls E, push_form reports it
    e->held_push_e = rp::resolve_push(plan, e->rules, tot[ST_ACTIVE_W], tot[ST_ACTIVE_V]) == rp::Push::Edge;
    pushed_e = e->held_push_e;
  }
  if (e->auto_round == e->round)  // the round's own pack landed with its counters
    for (int q = 0; q + 1 < (int)e->send_seg.size(); ++q) e->auto_cnt[q] = (int64_t)e->h_seg_cnt[q];
#ifdef P2PG_PROF
  if (plan.receive == rp::Receive::Fused && s.prof && std::getenv("P2PG_PROF_ROUNDS")) {
    // development builds: per-round fused-kernel segment clocks (then reset)
    unsigned long long h[9];
    HIPCHK(e, hipMemcpy(h, s.prof, sizeof(h), hipMemcpyDeviceToHost));
    HIPCHK(e, hipMemset(s.prof, 0, sizeof(h)));
    fprintf(stderr, "P2PG_PROF_ROUND %d", e->round);
    for (int i = 0; i < 9; ++i) fprintf(stderr, " %llu", h[i]);
    fprintf(stderr, "\n");
  }
#endif
  const int32_t form = !gossip ? P2PG_PUSH_NONE
                       : plan.receive == rp::Receive::Fused ? P2PG_PUSH_FUSED
                       : plan.receive == rp::Receive::UpdatePush ? P2PG_PUSH_UPDATE_EDGE
                       : pushed_e ? P2PG_PUSH_EDGE : P2PG_PUSH_ATOMIC;
  return close_round(e, tot, form, pushed_e, p.store_f == 1, cnt_lost ? (uint64_t)e->h_cnt2[1] : 0, out) ? 1 : 0;
}

int p2pg_step_end(p2pg_engine* e, p2pg_round_stats* out) { return p2pg_step(e, out); }

// p2pg_run's decay phase: after the dense rounds, while receipts shrink, every round is an update
// of the row pushes and a row-atomic push whose form, list bound (the last round's pushed masks,
// shrinking too) and dedup setting need none of its own counters -- so BATCH_MAX of them are
// enqueued at once, each writing its counters to its own slot, and read with ONE host
// synchronisation (c4: ~20 tail rounds of 0.05-0.2 ms kernels each paid a full host round trip).
// Rounds enqueued after the run went quiet see an empty frontier and change nothing; they are
// not reported and the engine stands where p2pg_step would have left it.  The list is sized by
// a bound that holds for the batch's first round (its frontier words <= the masks pushed into it,
// prev_sw) with room to spare for the others (decay: each round's frontier is ~2.5x smaller); a
// later round whose frontier still outgrew it had its push truncated, so the call reports the
// rounds before that one, fails (P2PG_ERR_STATE) and leaves the engine refusing every further
// round until a reset (the device state past that round is not the run's).
constexpr int BATCH_MAX = 8;

static bool decay_batchable(const p2pg_engine* e) {
  const int br = e->batch_rounds < 0 ? BATCH_MAX : e->batch_rounds;
  if (br <= 1 || !e->have_state || e->done || e->begun) return false;
  rp::DecayFacts f;
  f.round = e->round;
  f.V = e->V;
  f.consume_next = e->consume_next;
  f.late_starts = e->last_start != 0;
  f.expiry_ahead = expiry_ahead(e, e->round);
  f.offline_ahead = e->down_on && e->down_sweep.offline_ahead(e->round);
  f.pull_ahead = e->ae.arrival_ahead(e->round);
  f.cut_ahead = e->ns_win.cut_ahead(e->round);
  f.frontier_needed = frontier_needed(e);
  f.autostop = !(e->cfg.flags & P2PG_FLAG_NO_AUTOSTOP);
  f.auto_buf = e->auto_buf != nullptr;
  f.arr_pending = e->arr_round >= 0;
  return rp::decay_batchable(e->hist, e->rules, round_caps(e), f);
}

// n_left: rounds the p2pg_run call may still run (its last two keep their frontier rows whole).
static int run_decay_batch(p2pg_engine* e, int32_t R, p2pg_round_stats* out, int32_t* ran,
                           int32_t n_left) {
  constexpr size_t SLOT = STAT_COUNT + 1;  // counters + the sparse list's fill count
  DevState& s = e->st;
  HIPCHK(e, hipSetDevice(e->cfg.device));
  if (!e->d_bstats) {
    HIPCHK(e, hipMalloc((void**)&e->d_bstats, sizeof(unsigned long long) * SLOT * BATCH_MAX));
    HIPCHK(e, hipHostMalloc((void**)&e->h_bstats, sizeof(unsigned long long) * SLOT * BATCH_MAX));
  }
  HIPCHK(e, hipMemsetAsync(e->d_bstats, 0, sizeof(unsigned long long) * SLOT * R, e->stream));
  // the list, sized once for the batch: the first round's bound, doubled for the others
  SparseBufs b;
  hipError_t lr = sparse_bufs(e, 2 * (int64_t)e->hist.prev_sw, b);
  if (lr != hipSuccess) return fail(e, P2PG_ERR_HIP, std::string("run (batch list): ") + hipGetErrorString(lr));
  const uint64_t words = (uint64_t)e->wlist_cap;  // no round of the batch grows the list
  unsigned long long* const stats0 = s.stats;
  const DevGraph g = graph(e);
  int rc = P2PG_OK;
  bool partial[BATCH_MAX] = {false};
  for (int32_t i = 0; i < R && rc == P2PG_OK; ++i) {
    s.stats = e->d_bstats + SLOT * i;
    RoundParams p = params(e);
    p.round = e->round + i;
    if (i + 2 < n_left && partial_rows(e)) p.store_f = 2;
    partial[i] = p.store_f == 2;
    rc = timed(e, 4, [&] { return launch_gossip_update(g, s, p, e->stream); });
    if (rc == P2PG_OK && s.hop) rc = timed(e, 3, [&] { return launch_record(g, s, p, pull_of(e, -1), cut(e), e->stream); });
    p.dedup_push = rp::push_dedup(e->hist, e->rules);
    if (rc == P2PG_OK)
      rc = timed(e, 2, [&] {
        return launch_scatter_atomic(e, g, p, std::min<uint64_t>(e->hist.prev_sw, words));
      });
  }
  s.stats = stats0;
  e->wlist_check = false;
  if (rc) return rc;
  HIPCHK(e, hipMemcpyAsync(e->h_bstats, e->d_bstats, sizeof(unsigned long long) * SLOT * R,
                           hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, round_sync(e));
  if ((rc = resolve_timings(e))) return rc;
  *ran = 0;
  for (int32_t i = 0; i < R; ++i) {
    const unsigned long long* h = e->h_bstats + SLOT * i;
    if ((int64_t)h[STAT_COUNT] > e->wlist_cap) {
      // round e->round's push was truncated: the rounds before it stand (reported), nothing after
      e->failed = "round " + std::to_string(e->round) + " of a batched decay run outgrew its sparse push list (" +
                  std::to_string(h[STAT_COUNT]) + " words listed, room for " + std::to_string(e->wlist_cap) +
                  "); reset to run again";
      e->done = true;
      return fail(e, P2PG_ERR_STATE, "run: " + e->failed);
    }
    uint64_t tot[STAT_N] = {0};
    for (int sh = 0; sh < STAT_SHARDS; ++sh)
      for (int q = 0; q < STAT_N; ++q) tot[q] += h[sh * STAT_N + q];
    // (no churn in a batched run: no lost sends)
    const bool active = close_round(e, tot, P2PG_PUSH_ATOMIC, false, !partial[i], 0, &out[i]);
    *ran = i + 1;
    if (!active) break;  // the run is done (rounds enqueued after this one saw an empty frontier)
  }
  return P2PG_OK;
}

int p2pg_run(p2pg_engine* e, int32_t max_rounds, p2pg_round_stats* per_round,
             int32_t* n_rounds) {
  if (!e) return P2PG_ERR_ARG;
  int32_t n = 0;
  int rc = 1;
  while (n < max_rounds) {
    p2pg_round_stats tmp;
    if (decay_batchable(e) && max_rounds - n >= 2) {
      const int br = e->batch_rounds < 0 ? BATCH_MAX : std::min(e->batch_rounds, BATCH_MAX);
      const int32_t R = std::min<int32_t>(br, max_rounds - n);
      p2pg_round_stats buf[BATCH_MAX];
      int32_t ran = 0;
      rc = run_decay_batch(e, R, buf, &ran, max_rounds - n);
      if (per_round) std::memcpy(per_round + n, buf, sizeof(p2pg_round_stats) * ran);
      n += ran;
      if (rc < 0) {  // (the rounds that stand are reported)
        if (n_rounds) *n_rounds = n;
        return rc;
      }
      rc = e->done ? 0 : 1;
      if (rc == 0) break;
      continue;
    }
    // only the last two rounds a call may run can leave frontiers behind for the caller (the
    // deliveries of the last round and their parents in the round before; snapshots); a
    // quiescent round has none
    e->skip_frontier = n + 2 < max_rounds && !frontier_needed(e);  // (the lost count / tallies read F)
    rc = p2pg_step(e, per_round ? &per_round[n] : &tmp);
    e->skip_frontier = false;
    if (rc < 0) return rc;
    ++n;
    if (rc == 0) break;
  }
  if (n_rounds) *n_rounds = n;
  return rc;
}

int p2pg_get_new_deliveries(p2pg_engine* e, int64_t cap, int32_t* peer, int32_t* msg,
                            int32_t* hop, int32_t* parent, int64_t* n_out) {
  if (!e || cap < 0 || !n_out || (cap > 0 && (!peer || !msg || !hop || !parent)))
    return fail(e, P2PG_ERR_ARG, "get_new_deliveries: bad arguments");
  if (!e->have_state || e->round == 0)
    return fail(e, P2PG_ERR_STATE, "get_new_deliveries: no round has run");
  if (e->hist.last_new == 0) {  // a round without receipts has no deliveries (and needs no parents)
    *n_out = 0;
    return P2PG_OK;
  }
  if (!e->frontier_kept)
    return fail(e, P2PG_ERR_STATE, "get_new_deliveries: the last round's frontier was not kept");
  if (e->exp_final == e->round - 1)
    return fail(e, P2PG_ERR_STATE, "get_new_deliveries: hop limits expired or a relay policy acted in the last round and its sends were "
                                   "made final (get_sends, peer_counters, update_edges, drop_relays or "
                                   "step_begin): read the round's deliveries first");
  if (!e->frontier_kept_prev)
    return fail(e, P2PG_ERR_STATE, "get_new_deliveries: the parents need the frontier of the round "
                                   "before, which was not kept (a fused round inside p2pg_run, or "
                                   "the round a snapshot was restored at)");
  HIPCHK(e, hipSetDevice(e->cfg.device));
  // the most recent round is e->round - 1; its frontier is F[(round-1)&1]
  RoundParams p = params(e);
  p.round = e->round - 1;
  const DevGraph g = graph_for_arrivals(e, p.round);
  int32_t *dpeer = nullptr, *dmsg = nullptr, *dpar = nullptr;
  unsigned long long* dcnt = nullptr;
  const int64_t c = cap > 0 ? cap : 1;
  HIPCHK(e, hipMalloc((void**)&dpeer, sizeof(int32_t) * c));
  HIPCHK(e, hipMalloc((void**)&dmsg, sizeof(int32_t) * c));
  HIPCHK(e, hipMalloc((void**)&dpar, sizeof(int32_t) * c));
  HIPCHK(e, hipMalloc((void**)&dcnt, sizeof(unsigned long long)));
  HIPCHK(e, hipMemsetAsync(dcnt, 0, sizeof(unsigned long long), e->stream));
  hipError_t lr = launch_deliveries(g, e->st, p, pull_of(e, p.round), cut(e), cap, dpeer, dmsg, dpar, dcnt, e->stream);
  unsigned long long cnt = 0;
  if (lr == hipSuccess) lr = hipMemcpyAsync(&cnt, dcnt, sizeof(cnt), hipMemcpyDeviceToHost, e->stream);
  if (lr == hipSuccess) lr = hipStreamSynchronize(e->stream);
  const int64_t n = std::min<int64_t>((int64_t)cnt, cap);
  std::vector<int32_t> hp(n), hm(n), hpar(n);
  if (lr == hipSuccess && n > 0) {
    lr = hipMemcpy(hp.data(), dpeer, sizeof(int32_t) * n, hipMemcpyDeviceToHost);
    if (lr == hipSuccess) lr = hipMemcpy(hm.data(), dmsg, sizeof(int32_t) * n, hipMemcpyDeviceToHost);
    if (lr == hipSuccess) lr = hipMemcpy(hpar.data(), dpar, sizeof(int32_t) * n, hipMemcpyDeviceToHost);
  }
  (void)hipFree(dpeer);
  (void)hipFree(dmsg);
  (void)hipFree(dpar);
  (void)hipFree(dcnt);
  if (lr != hipSuccess) return fail(e, P2PG_ERR_HIP, std::string("get_new_deliveries: ") + hipGetErrorString(lr));
  // deterministic order: ascending (peer, msg)  (the compat layer replays hooks in it)
  std::vector<int64_t> idx(n);
  std::iota(idx.begin(), idx.end(), 0);
  std::sort(idx.begin(), idx.end(), [&](int64_t a, int64_t b) {
    return hp[a] != hp[b] ? hp[a] < hp[b] : hm[a] < hm[b];
  });
  const bool map = !e->h_gid.empty();
  for (int64_t i = 0; i < n; ++i) {
    const int32_t pr = hpar[idx[i]];
    peer[i] = map ? e->h_gid[hp[idx[i]]] : hp[idx[i]];
    msg[i] = hm[idx[i]];
    hop[i] = p.round;
    parent[i] = (map && pr >= 0) ? e->h_gid[pr] : pr;
  }
  *n_out = (int64_t)cnt;
  return P2PG_OK;
}

// Shared preconditions of the sends stream / relay withdrawal: a round ran, its frontier (and,
// flood, the one before it: the senders' parents) is in F, and no topology update or half
// round stands between that round and now.
static int sends_state(p2pg_engine* e, const char* what) {
  const std::string w(what);
  if (!e->have_state || e->round == 0) return fail(e, P2PG_ERR_STATE, w + ": no round has run");
  if (e->begun) return fail(e, P2PG_ERR_STATE, w + ": a round has begun (step_begin)");
  if (e->arr_round >= 0 && e->arr_round == e->round)
    return fail(e, P2PG_ERR_STATE, w + ": the connections changed since the round (call it before p2pg_update_edges)");
  if (e->hist.last_new == 0) return P2PG_OK;
  if (!e->frontier_kept) return fail(e, P2PG_ERR_STATE, w + ": the last round's frontier was not kept");
  if (e->cfg.mode == P2PG_MODE_FLOOD && e->round > 1 && !e->frontier_kept_prev)
    return fail(e, P2PG_ERR_STATE, w + ": the senders' parents need the frontier of the round before, "
                                       "which was not kept");
  return P2PG_OK;
}

int p2pg_get_sends(p2pg_engine* e, int64_t cap, int32_t* sender, int32_t* receiver, int32_t* msg,
                   uint8_t* lost, int64_t* n_out) {
  if (!e || cap < 0 || !n_out || (cap > 0 && (!sender || !receiver || !msg || !lost)))
    return fail(e, P2PG_ERR_ARG, "get_sends: bad arguments");
  int rc = sends_state(e, "get_sends");
  if (rc) return rc;
  if (e->hist.last_new == 0) {
    *n_out = 0;
    return P2PG_OK;
  }
  HIPCHK(e, hipSetDevice(e->cfg.device));
  {  // hop limits: the expired receipts' sends do not exist
    const int xrc = finalize_expiry(e, true);
    if (xrc) return xrc;
  }
  const int32_t r = e->round - 1;
  RoundParams p = params(e);
  p.round = r;
  const int64_t c = cap > 0 ? cap : 1;
  int32_t *ds = nullptr, *dr = nullptr, *dm = nullptr;
  uint8_t* dl = nullptr;
  // (one chain: whatever fails, every buffer allocated so far is freed below)
  hipError_t lr = hipMalloc((void**)&ds, sizeof(int32_t) * c);
  if (lr == hipSuccess) lr = hipMalloc((void**)&dr, sizeof(int32_t) * c);
  if (lr == hipSuccess) lr = hipMalloc((void**)&dm, sizeof(int32_t) * c);
  if (lr == hipSuccess) lr = hipMalloc((void**)&dl, c);
  if (lr == hipSuccess) lr = hipMemsetAsync(e->d_cnt2, 0, 2 * sizeof(unsigned long long), e->stream);
  if (lr == hipSuccess)
    lr = launch_sends(graph(e), graph_for_arrivals(e, r), e->st, p, down(e), cut(e), pull_of(e, r), true, cap, ds, dr, dm, dl, e->d_cnt2, e->stream);
  unsigned long long cnt = 0;
  if (lr == hipSuccess) lr = hipMemcpyAsync(&cnt, e->d_cnt2, sizeof(cnt), hipMemcpyDeviceToHost, e->stream);
  if (lr == hipSuccess) lr = hipStreamSynchronize(e->stream);
  const int64_t n = std::min<int64_t>((int64_t)cnt, cap);
  std::vector<int32_t> hs(n), hr(n), hm(n);
  std::vector<uint8_t> hl(n);
  if (lr == hipSuccess && n > 0) {
    lr = hipMemcpy(hs.data(), ds, sizeof(int32_t) * n, hipMemcpyDeviceToHost);
    if (lr == hipSuccess) lr = hipMemcpy(hr.data(), dr, sizeof(int32_t) * n, hipMemcpyDeviceToHost);
    if (lr == hipSuccess) lr = hipMemcpy(hm.data(), dm, sizeof(int32_t) * n, hipMemcpyDeviceToHost);
    if (lr == hipSuccess) lr = hipMemcpy(hl.data(), dl, n, hipMemcpyDeviceToHost);
  }
  (void)hipFree(ds);
  (void)hipFree(dr);
  (void)hipFree(dm);
  (void)hipFree(dl);
  if (lr != hipSuccess) return fail(e, P2PG_ERR_HIP, std::string("get_sends: ") + hipGetErrorString(lr));
  // deterministic order: ascending (receiver, sender, msg) -- the harness's delivery order up to the
  // order of one sender's packets on one connection, which the caller knows (its relay order)
  std::vector<int64_t> idx(n);
  std::iota(idx.begin(), idx.end(), 0);
  std::sort(idx.begin(), idx.end(), [&](int64_t a, int64_t b) {
    if (hr[a] != hr[b]) return hr[a] < hr[b];
    return hs[a] != hs[b] ? hs[a] < hs[b] : hm[a] < hm[b];
  });
  const bool map = !e->h_gid.empty();
  for (int64_t i = 0; i < n; ++i) {
    const int64_t k = idx[i];
    sender[i] = map ? e->h_gid[hs[k]] : hs[k];
    receiver[i] = map ? e->h_gid[hr[k]] : hr[k];
    msg[i] = hm[k];
    lost[i] = hl[k];
  }
  *n_out = (int64_t)cnt;
  return P2PG_OK;
}

int p2pg_drop_relays(p2pg_engine* e, int64_t n, const int32_t* peer, const int32_t* msg) {
  if (!e || n < 0 || (n > 0 && (!peer || !msg))) return fail(e, P2PG_ERR_ARG, "drop_relays: bad arguments");
  if (e && e->ae.on())
    return fail(e, P2PG_ERR_STATE, "drop_relays: not available while anti-entropy is set (p2pg_set_anti_entropy)");
  if (e && e->ns_win.on())
    return fail(e, P2PG_ERR_STATE, "drop_relays: not available while a netsplit is set (p2pg_set_netsplit)");
  int rc = sends_state(e, "drop_relays");
  if (rc) return rc;
  if (deferred_on(e) && e->tally_read_at == e->round)
    return fail(e, P2PG_ERR_STATE, "drop_relays: p2pg_peer_counters / p2pg_message_cost has counted this round's sends already; "
                                   "read the counters after the changes of a round boundary");
  if (n == 0) return P2PG_OK;
  if (e->d_gid || (e->cfg.flags & P2PG_FLAG_LOCAL_GRAPH))
    return fail(e, P2PG_ERR_STATE, "drop_relays: not on a vertex-partitioned rank");
  const bool gossip = e->cfg.mode == P2PG_MODE_GOSSIP;
  if (!gossip && e->consume_next)
    return fail(e, P2PG_ERR_STATE, "drop_relays: the last round's sends were materialized (restored snapshot)");
  std::vector<uint64_t> list(n);
  for (int64_t i = 0; i < n; ++i) {
    if (peer[i] < 0 || peer[i] >= e->V || msg[i] < 0 || msg[i] >= e->M)
      return fail(e, P2PG_ERR_ARG, "drop_relays: peer or message out of range");
    list[i] = ((uint64_t)(uint32_t)peer[i] << 32) | (uint32_t)msg[i];
  }
  std::sort(list.begin(), list.end());
  if (std::adjacent_find(list.begin(), list.end()) != list.end())
    return fail(e, P2PG_ERR_ARG, "drop_relays: a first receipt is listed twice");
  HIPCHK(e, hipSetDevice(e->cfg.device));
  const int32_t r = e->round - 1;
  // Hop limits: a receipt of a message that expired in this round relays nothing, so dropping it
  // is legal and cancels nothing.  Once the round's sends are final its frontier bits are gone and
  // such an entry can no longer be checked against them: it is then taken as listed.
  if (e->exp_final == r)
    list.erase(std::remove_if(list.begin(), list.end(),
                              [&](uint64_t x) {
                                // (a receipt the relay policy muted went the same way)
                                return expires_in(e, (int32_t)(uint32_t)x, r) ||
                                       policy_muted(e, (int64_t)(x >> 32), (int32_t)(uint32_t)x, r);
                              }),
               list.end());
  n = (int64_t)list.size();
  uint64_t* dl = nullptr;
  HIPCHK(e, hipMalloc((void**)&dl, sizeof(uint64_t) * (n ? n : 1)));
  hipError_t lr = hipMemcpyAsync(dl, list.data(), sizeof(uint64_t) * n, hipMemcpyHostToDevice, e->stream);
  if (lr == hipSuccess) lr = hipMemsetAsync(e->d_cnt2, 0, 2 * sizeof(unsigned long long), e->stream);
  if (lr == hipSuccess) lr = launch_drop(e->st, r, dl, n, true, e->d_cnt2, e->stream);
  if (lr == hipSuccess)
    lr = hipMemcpyAsync(e->h_cnt2, e->d_cnt2, sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream);
  if (lr == hipSuccess) lr = hipStreamSynchronize(e->stream);
  if (lr == hipSuccess && (int64_t)e->h_cnt2[0] != n) {
    (void)hipFree(dl);
    return fail(e, P2PG_ERR_ARG, "drop_relays: " + std::to_string(n - (int64_t)e->h_cnt2[0]) +
                                     " listed (peer, msg) are not first receipts of the last round");
  }
  // (the listed receipts stand: now the round's expired bits go, then the listed ones)
  if (lr == hipSuccess) {
    const int xrc = finalize_expiry(e, false);
    if (xrc) {
      (void)hipFree(dl);
      return xrc;
    }
  }
  if (lr == hipSuccess) lr = launch_drop(e->st, r, dl, n, false, nullptr, e->stream);
  if (lr == hipSuccess) lr = launch_rebuild_aw(e->st, r, e->V, e->stream);
  // the relays these receipts would have made (node.py:106-116): flood every connection but
  // the sender (all of them at the origin), gossip min(k, deg)
  uint64_t cancelled = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t v = (int64_t)(list[i] >> 32);
    const uint64_t deg = (uint64_t)(e->h_rowptr[v + 1] - e->h_rowptr[v]);
    const bool origin = e->h_start[(uint32_t)list[i]] == r;  // the message's own origination
    if (expires_in(e, (int32_t)(uint32_t)list[i], r)) continue;  // (it made no relays to cancel)
    if (policy_muted(e, v, (int32_t)(uint32_t)list[i], r)) continue;  // (nor did a muted receipt)
    cancelled += gossip ? std::min<uint64_t>(deg, (uint64_t)e->cfg.fanout) : (origin ? deg : (deg ? deg - 1 : 0));
  }
  if (lr == hipSuccess && gossip) {
    // this round's pushes left inside the round: push the remaining receipts again, as row
    // atomics, into the cleared row-push planes the next round consumes (the Philox picks are a
    // pure function of round, peer and message, so the others go where they went)
    DevState& s = e->st;
    const int nx = e->round & 1;
    lr = hipMemsetAsync(s.next[nx], 0, e->plane_bytes, e->stream);
    if (lr == hipSuccess) lr = hipMemsetAsync(s.T[nx], 0, e->bm_bytes, e->stream);
    RoundParams p = params(e);
    p.round = r;
    if (lr == hipSuccess) lr = launch_scatter_atomic(e, graph(e), p, std::max<uint64_t>(e->hist.prev_aw, 1));
  }
  if (lr == hipSuccess && count_lost_on(e))
    lr = enqueue_lost_count(e, graph(e), graph_for_arrivals(e, r), r);
  if (lr == hipSuccess) lr = hipStreamSynchronize(e->stream);
  unsigned long long listed = 0;
  if (lr == hipSuccess && gossip && e->wlist_check)
    lr = hipMemcpy(&listed, e->st.stats + STAT_COUNT, sizeof(listed), hipMemcpyDeviceToHost);
  (void)hipFree(dl);  // the one exit of the chain above: every path past the allocation frees it
  if (lr != hipSuccess) return fail(e, P2PG_ERR_HIP, std::string("drop_relays: ") + hipGetErrorString(lr));
  if (gossip) {
    if (e->wlist_check && (rc = check_scatter_list(e, listed))) return rc;
    e->consume_next = true;
    e->hist.last_push_e = false;
    e->stats_clear = true;  // the re-push counted into the round counters
  }
  if (count_lost_on(e)) e->lost_last = (uint64_t)e->h_cnt2[1];
  e->sent_last -= std::min(cancelled, e->sent_last);
  e->total_relays -= std::min(cancelled, e->total_relays);
  return P2PG_OK;
}

int p2pg_read_planes(p2pg_engine* e, uint64_t* seen, int32_t* hop, int32_t* parent) {
  if (!e || !e->have_state) return fail(e, P2PG_ERR_STATE, "read_planes: no state");
  if ((hop || parent) && !e->st.hop)
    return fail(e, P2PG_ERR_STATE, "read_planes: hop/parent need P2PG_FLAG_RECORD");
  HIPCHK(e, hipSetDevice(e->cfg.device));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (seen) HIPCHK(e, hipMemcpy(seen, e->st.seen, e->plane_bytes, hipMemcpyDeviceToHost));
  const size_t hb = (size_t)e->V * e->M * sizeof(int32_t);
  if (hop) HIPCHK(e, hipMemcpy(hop, e->st.hop, hb, hipMemcpyDeviceToHost));
  if (parent) {
    HIPCHK(e, hipMemcpy(parent, e->st.parent, hb, hipMemcpyDeviceToHost));
    if (!e->h_gid.empty())  // local -> global sender ids
      for (size_t i = 0; i < (size_t)e->V * e->M; ++i)
        if (parent[i] >= 0) parent[i] = e->h_gid[parent[i]];
  }
  return P2PG_OK;
}

int p2pg_read_seen_word(p2pg_engine* e, int32_t w, uint64_t* out) {
  if (!e || !e->have_state) return fail(e, P2PG_ERR_STATE, "read_seen_word: no state");
  if (w < 0 || w >= e->W || !out) return fail(e, P2PG_ERR_ARG, "read_seen_word: word out of range");
  HIPCHK(e, hipSetDevice(e->cfg.device));
  // column w of the [V][W] plane gathered into a contiguous device buffer, then one copy
  uint64_t* col = nullptr;
  HIPCHK(e, hipMalloc((void**)&col, sizeof(uint64_t) * (size_t)e->V));
  hipError_t r = launch_column(e->st.seen, e->W, w, e->V, col, e->stream);
  if (r == hipSuccess) r = hipStreamSynchronize(e->stream);
  if (r == hipSuccess) r = hipMemcpy(out, col, sizeof(uint64_t) * (size_t)e->V, hipMemcpyDeviceToHost);
  (void)hipFree(col);
  if (r != hipSuccess) return fail(e, P2PG_ERR_HIP, std::string("read_seen_word: ") + hipGetErrorString(r));
  return P2PG_OK;
}

// Shared preconditions of the tally reads: sources set, between rounds.
static int tally_state(p2pg_engine* e, const char* what, bool need_flag) {
  const std::string w(what);
  if (!e) return fail(e, P2PG_ERR_ARG, w + ": no engine");
  if (!e->have_state) return fail(e, P2PG_ERR_STATE, w + ": no sources set");
  if (e->begun) return fail(e, P2PG_ERR_STATE, w + ": a round has begun (step_begin)");
  if (need_flag && !tally_on(e)) return fail(e, P2PG_ERR_STATE, w + ": needs P2PG_FLAG_TALLY");
  return P2PG_OK;
}

// The pending round's sends count as they stand (p2pg_peer_counters, p2pg_message_cost): a later
// drop or topology update at this boundary would change sends already counted, so those calls
// refuse from here on.
static int take_pending_round(p2pg_engine* e, const char* what) {
  if (e->tally_pending < 0) return P2PG_OK;
  {  // hop limits: the expired receipts' sends do not exist
    const int xrc = finalize_expiry(e, true);
    if (xrc) return xrc;
  }
  const hipError_t x = flush_peer_tally(e, graph(e));
  if (x != hipSuccess) return fail(e, P2PG_ERR_HIP, std::string(what) + ": " + hipGetErrorString(x));
  e->tally_read_at = e->round;
  return P2PG_OK;
}

int p2pg_message_reach(p2pg_engine* e, uint64_t* reach) {
  int rc = tally_state(e, "message_reach", false);
  if (rc) return rc;
  if (!reach) return fail(e, P2PG_ERR_ARG, "message_reach: no output array");
  if (e->d_gid || (e->cfg.flags & P2PG_FLAG_LOCAL_GRAPH))
    return fail(e, P2PG_ERR_STATE, "message_reach: not on a vertex-partitioned rank (ghost rows are "
                                   "another rank's peers)");
  HIPCHK(e, hipSetDevice(e->cfg.device));
  // the shard scratch and the counts: the engine's own scratch with the flag, else for this call
  const size_t sb = sizeof(unsigned long long) * (size_t)tally_scratch_words(e->W);
  unsigned long long *scratch = e->d_tscratch, *out = nullptr;
  hipError_t r = hipMalloc((void**)&out, sizeof(unsigned long long) * (size_t)e->M);
  if (r == hipSuccess && !scratch) {
    r = hipMalloc((void**)&scratch, sb);
    if (r == hipSuccess) r = hipMemsetAsync(scratch, 0, sb, e->stream);
  }
  if (r == hipSuccess)
    r = launch_column_count(e->st.seen, nullptr, e->V, e->W, e->M, 0, scratch, out, nullptr, nullptr, nullptr,
                            e->stream);
  if (r == hipSuccess) r = hipStreamSynchronize(e->stream);
  if (r == hipSuccess) r = hipMemcpy(reach, out, sizeof(unsigned long long) * (size_t)e->M, hipMemcpyDeviceToHost);
  if (scratch && scratch != e->d_tscratch) (void)hipFree(scratch);
  if (out) (void)hipFree(out);
  if (r != hipSuccess) return fail(e, P2PG_ERR_HIP, std::string("message_reach: ") + hipGetErrorString(r));
  return P2PG_OK;
}

int p2pg_message_tally(p2pg_engine* e, uint64_t* reach, uint64_t* hop_sum, int32_t* last_hop) {
  int rc = tally_state(e, "message_tally", true);
  if (rc) return rc;
  HIPCHK(e, hipSetDevice(e->cfg.device));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  const size_t n = (size_t)e->M;
  if (reach) HIPCHK(e, hipMemcpy(reach, e->d_treach, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost));
  if (hop_sum) HIPCHK(e, hipMemcpy(hop_sum, e->d_thop, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost));
  if (last_hop) HIPCHK(e, hipMemcpy(last_hop, e->d_tlast, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  return P2PG_OK;
}

int p2pg_peer_counters(p2pg_engine* e, uint64_t* sent, uint64_t* received) {
  int rc = tally_state(e, "peer_counters", true);
  if (rc) return rc;
  HIPCHK(e, hipSetDevice(e->cfg.device));
  if ((rc = take_pending_round(e, "peer_counters"))) return rc;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  const size_t n = (size_t)e->V;
  if (sent) HIPCHK(e, hipMemcpy(sent, e->d_tsent, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost));
  if (received) HIPCHK(e, hipMemcpy(received, e->d_trecv, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost));
  return P2PG_OK;
}

int p2pg_message_cost(p2pg_engine* e, uint64_t* sent, uint64_t* received) {
  int rc = tally_state(e, "message_cost", false);
  if (rc) return rc;
  if (!cost_on(e)) return fail(e, P2PG_ERR_STATE, "message_cost: needs P2PG_FLAG_MSG_COST");
  if (e->d_gid || (e->cfg.flags & P2PG_FLAG_LOCAL_GRAPH))
    return fail(e, P2PG_ERR_STATE, "message_cost: not on a vertex-partitioned rank");
  HIPCHK(e, hipSetDevice(e->cfg.device));
  if ((rc = take_pending_round(e, "message_cost"))) return rc;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  const size_t n = (size_t)e->M;
  if (sent) HIPCHK(e, hipMemcpy(sent, e->d_csent, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost));
  if (received) HIPCHK(e, hipMemcpy(received, e->d_crecv, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost));
  return P2PG_OK;
}

// Shared preconditions of the latency calls: the flag, sources set, between rounds, one rank.
static int latency_state(p2pg_engine* e, const char* what) {
  const std::string w(what);
  if (!e) return fail(e, P2PG_ERR_ARG, w + ": no engine");
  if (!latency_on(e)) return fail(e, P2PG_ERR_STATE, w + ": needs P2PG_FLAG_LATENCY");
  if (!e->have_state) return fail(e, P2PG_ERR_STATE, w + ": no sources set");
  if (e->begun) return fail(e, P2PG_ERR_STATE, w + ": a round has begun (step_begin)");
  if (e->d_gid || (e->cfg.flags & P2PG_FLAG_LOCAL_GRAPH))
    return fail(e, P2PG_ERR_STATE, w + ": not on a vertex-partitioned rank");
  return P2PG_OK;
}

int p2pg_set_latency_bins(p2pg_engine* e, int32_t bins) {
  int rc = latency_state(e, "set_latency_bins");
  if (rc) return rc;
  if (bins < latency::BINS_MIN || bins > latency::BINS_MAX)
    return fail(e, P2PG_ERR_ARG, "set_latency_bins: bins must lie in [2, 1024]");
  if (e->round > 0)
    return fail(e, P2PG_ERR_STATE, "set_latency_bins: a round has run (set the bins before round 0, or after p2pg_reset)");
  if (bins == e->lat_bins) return P2PG_OK;
  HIPCHK(e, hipSetDevice(e->cfg.device));
  HIPCHK(e, hipStreamSynchronize(e->stream));  // (a reset's zeroing of the old plane may be queued)
  const int32_t old = e->lat_bins;
  e->lat_bins = bins;
  if ((rc = alloc_latency_hist(e))) {
    e->lat_bins = old;
    const int rc2 = alloc_latency_hist(e);
    return rc2 ? rc2 : rc;
  }
  return P2PG_OK;
}

int p2pg_message_latency(p2pg_engine* e, int32_t bins, uint64_t* hist) {
  int rc = latency_state(e, "message_latency");
  if (rc) return rc;
  if (!hist) return fail(e, P2PG_ERR_ARG, "message_latency: no output array");
  if (bins != e->lat_bins)
    return fail(e, P2PG_ERR_ARG, "message_latency: bins differs from the engine's (" + std::to_string(e->lat_bins) + ")");
  HIPCHK(e, hipSetDevice(e->cfg.device));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipMemcpy(hist, e->d_lhist, sizeof(unsigned long long) * (size_t)e->M * (size_t)bins, hipMemcpyDeviceToHost));
  return P2PG_OK;
}

int p2pg_peer_latency(p2pg_engine* e, uint64_t* hop_sum, uint32_t* receipts, int32_t* max_hop) {
  int rc = latency_state(e, "peer_latency");
  if (rc) return rc;
  HIPCHK(e, hipSetDevice(e->cfg.device));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (!hop_sum && !receipts && !max_hop) return P2PG_OK;
  std::vector<PeerLat> h((size_t)e->V);
  HIPCHK(e, hipMemcpy(h.data(), e->d_lpeer, sizeof(PeerLat) * (size_t)e->V, hipMemcpyDeviceToHost));
  for (int64_t v = 0; v < e->V; ++v) {
    if (hop_sum) hop_sum[v] = h[v].hop_sum;
    if (receipts) receipts[v] = h[v].receipts;
    if (max_hop) max_hop[v] = (int32_t)h[v].max1 - 1;
  }
  return P2PG_OK;
}

int p2pg_set_global_ids(p2pg_engine* e, const int32_t* gid) {
  if (!e || !e->d_rowptr) return fail(e, P2PG_ERR_STATE, "set_global_ids: load a graph first");
  if (latency_on(e))
    return fail(e, P2PG_ERR_STATE, "set_global_ids: a P2PG_FLAG_LATENCY engine cannot be a vertex-partitioned "
                                   "rank (ghost rows would be counted on two ranks)");
  if (tally_on(e))
    return fail(e, P2PG_ERR_STATE, "set_global_ids: a P2PG_FLAG_TALLY engine cannot be a vertex-partitioned "
                                   "rank (ghost rows would be counted on two ranks)");
  if (cost_on(e))
    return fail(e, P2PG_ERR_STATE, "set_global_ids: a P2PG_FLAG_MSG_COST engine cannot be a vertex-partitioned "
                                   "rank (ghost rows would be counted on two ranks)");
  if (gid && e->have_state && e->late)
    return fail(e, P2PG_ERR_STATE, "set_global_ids: start rounds other than 0 are not available on a "
                                   "vertex-partitioned rank");
  if (gid && e->have_state && e->ttl_on)
    return fail(e, P2PG_ERR_STATE, "set_global_ids: hop limits (p2pg_set_ttl) are not available on a "
                                   "vertex-partitioned rank");
  if (gid && e->pol_on)
    return fail(e, P2PG_ERR_STATE, "set_global_ids: a relay policy (p2pg_set_relay_policy) is not available on a "
                                   "vertex-partitioned rank");
  if (gid && e->ns_win.on())
    return fail(e, P2PG_ERR_STATE, "set_global_ids: a netsplit (p2pg_set_netsplit) is not available on a "
                                   "vertex-partitioned rank");
  if (gid && e->down_on)
    return fail(e, P2PG_ERR_STATE, "set_global_ids: peer downtime (p2pg_set_downtime) is not available on a "
                                   "vertex-partitioned rank");
  if (gid && e->ae.on())
    return fail(e, P2PG_ERR_STATE, "set_global_ids: anti-entropy (p2pg_set_anti_entropy) is not available on a "
                                   "vertex-partitioned rank");
  HIPCHK(e, hipSetDevice(e->cfg.device));
  dfree(e->d_gid);
  e->h_gid.clear();
  if (!gid) return P2PG_OK;
  for (int64_t v = 1; v < e->V; ++v)
    if (gid[v] <= gid[v - 1])
      return fail(e, P2PG_ERR_ARG, "set_global_ids: ids must be strictly ascending (global order)");
  e->h_gid.assign(gid, gid + e->V);
  HIPCHK(e, hipMalloc((void**)&e->d_gid, sizeof(int32_t) * e->V));
  HIPCHK(e, hipMemcpy(e->d_gid, gid, sizeof(int32_t) * e->V, hipMemcpyHostToDevice));
  return P2PG_OK;
}

int p2pg_set_ghost_senders(p2pg_engine* e, const int32_t* ghost_deg, const int32_t* slot_pos) {
  if (!e || !e->d_rowptr) return fail(e, P2PG_ERR_STATE, "set_ghost_senders: load a graph first");
  HIPCHK(e, hipSetDevice(e->cfg.device));
  dfree(e->d_gdeg);
  dfree(e->d_gpos);
  if (!ghost_deg && !slot_pos) return P2PG_OK;
  if (!ghost_deg || !slot_pos) return fail(e, P2PG_ERR_ARG, "set_ghost_senders: need both arrays");
  for (int64_t v = 0; v < e->V; ++v)
    for (int64_t j = e->h_rowptr[v]; j < e->h_rowptr[v + 1]; ++j) {
      const int32_t u = e->h_colidx[j];
      if (slot_pos[j] < -1 || (slot_pos[j] >= 0 && slot_pos[j] >= ghost_deg[u]))
        return fail(e, P2PG_ERR_ARG, "set_ghost_senders: slot position outside the ghost's row");
    }
  HIPCHK(e, hipMalloc((void**)&e->d_gdeg, sizeof(int32_t) * (size_t)e->V));
  HIPCHK(e, hipMalloc((void**)&e->d_gpos, sizeof(int32_t) * (size_t)(e->nnz ? e->nnz : 1)));
  HIPCHK(e, hipMemcpy(e->d_gdeg, ghost_deg, sizeof(int32_t) * (size_t)e->V, hipMemcpyHostToDevice));
  if (e->nnz)
    HIPCHK(e, hipMemcpy(e->d_gpos, slot_pos, sizeof(int32_t) * (size_t)e->nnz, hipMemcpyHostToDevice));
  return P2PG_OK;
}

int p2pg_set_exchange(p2pg_engine* e, int64_t n_send, const int32_t* send_local, int64_t n_recv,
                      const int32_t* recv_local) {
  if (!e || !e->d_rowptr || n_send < 0 || n_recv < 0 || (n_send && !send_local) ||
      (n_recv && !recv_local))
    return fail(e, P2PG_ERR_ARG, "set_exchange: bad arguments");
  if (e->begun) return fail(e, P2PG_ERR_STATE, "set_exchange: a round has begun (step_begin)");
  for (int64_t i = 0; i < n_send; ++i)
    if (send_local[i] < 0 || send_local[i] >= e->V) return fail(e, P2PG_ERR_ARG, "set_exchange: send id out of range");
  for (int64_t i = 0; i < n_recv; ++i)
    if (recv_local[i] < 0 || recv_local[i] >= e->V) return fail(e, P2PG_ERR_ARG, "set_exchange: recv id out of range");
  HIPCHK(e, hipSetDevice(e->cfg.device));
  dfree(e->d_send);
  dfree(e->d_recv);
  e->n_send = n_send;
  e->n_recv = n_recv;
  HIPCHK(e, hipMalloc((void**)&e->d_send, sizeof(int32_t) * (n_send ? n_send : 1)));
  HIPCHK(e, hipMalloc((void**)&e->d_recv, sizeof(int32_t) * (n_recv ? n_recv : 1)));
  if (n_send) HIPCHK(e, hipMemcpy(e->d_send, send_local, sizeof(int32_t) * n_send, hipMemcpyHostToDevice));
  if (n_recv) HIPCHK(e, hipMemcpy(e->d_recv, recv_local, sizeof(int32_t) * n_recv, hipMemcpyHostToDevice));
  // border peers: a ghost (recv list) among the neighbours -- their pull / update waits for the
  // exchanged rows (phase 1); every other peer can run while the exchange is in flight
  dfree(e->d_border);
  if (n_recv) {
    std::vector<uint8_t> ghost((size_t)e->V, 0);
    for (int64_t i = 0; i < n_recv; ++i) ghost[recv_local[i]] = 1;
    std::vector<uint32_t> border((size_t)((e->V + 31) / 32), 0u);
    for (int64_t v = 0; v < e->V; ++v)
      for (int64_t j = e->h_rowptr[v]; j < e->h_rowptr[v + 1]; ++j)
        if (ghost[e->h_colidx[j]]) {
          border[v >> 5] |= 1u << (v & 31);
          break;
        }
    HIPCHK(e, hipMalloc((void**)&e->d_border, sizeof(uint32_t) * border.size()));
    HIPCHK(e, hipMemcpy(e->d_border, border.data(), sizeof(uint32_t) * border.size(), hipMemcpyHostToDevice));
  }
  return P2PG_OK;
}

int p2pg_set_exchange_segments(p2pg_engine* e, int32_t nseg, const int64_t* send_counts,
                               const int64_t* recv_counts) {
  if (!e || !e->d_send || nseg < 1 || nseg > P2PG_MAX_RANKS || !send_counts || !recv_counts)
    return fail(e, P2PG_ERR_ARG, "set_exchange_segments: bad arguments (set_exchange first; 1..16 ranks)");
  std::vector<int64_t> so(nseg + 1, 0), ro(nseg + 1, 0);
  for (int q = 0; q < nseg; ++q) {
    if (send_counts[q] < 0 || recv_counts[q] < 0) return fail(e, P2PG_ERR_ARG, "set_exchange_segments: negative count");
    so[q + 1] = so[q] + send_counts[q];
    ro[q + 1] = ro[q] + recv_counts[q];
  }
  if (so[nseg] != e->n_send || ro[nseg] != e->n_recv)
    return fail(e, P2PG_ERR_ARG, "set_exchange_segments: counts do not add up to the exchange lists");
  HIPCHK(e, hipSetDevice(e->cfg.device));
  dfree(e->d_send_seg);
  dfree(e->d_recv_seg);
  dfree(e->d_seg_cnt);
  if (e->h_seg_cnt) (void)hipHostFree(e->h_seg_cnt);
  e->h_seg_cnt = nullptr;
  e->send_seg = so;
  e->recv_seg = ro;
  HIPCHK(e, hipMalloc((void**)&e->d_send_seg, sizeof(int64_t) * so.size()));
  HIPCHK(e, hipMalloc((void**)&e->d_recv_seg, sizeof(int64_t) * ro.size()));
  HIPCHK(e, hipMemcpy(e->d_send_seg, so.data(), sizeof(int64_t) * so.size(), hipMemcpyHostToDevice));
  HIPCHK(e, hipMemcpy(e->d_recv_seg, ro.data(), sizeof(int64_t) * ro.size(), hipMemcpyHostToDevice));
  HIPCHK(e, hipMalloc((void**)&e->d_seg_cnt, sizeof(unsigned long long) * P2PG_MAX_RANKS));
  HIPCHK(e, hipHostMalloc((void**)&e->h_seg_cnt, sizeof(unsigned long long) * P2PG_MAX_RANKS));
  return P2PG_OK;
}

int p2pg_set_exchange_buffer(p2pg_engine* e, int32_t plane, void* dev_buf) {
  if (!e) return P2PG_ERR_ARG;
  if (!dev_buf) {
    e->auto_buf = nullptr;
    e->auto_plane = -1;
    e->auto_round = -1;
    return P2PG_OK;
  }
  if (plane != 0 && plane != 1) return fail(e, P2PG_ERR_ARG, "set_exchange_buffer: plane 0 or 1");
  if (!e->d_seg_cnt) return fail(e, P2PG_ERR_STATE, "set_exchange_buffer: set_exchange_segments first");
  if (plane == 1 && e->cfg.mode != P2PG_MODE_GOSSIP)
    return fail(e, P2PG_ERR_ARG, "set_exchange_buffer: plane 1 is for gossip pushes");
  if (e->begun) return fail(e, P2PG_ERR_STATE, "set_exchange_buffer: a round has begun (step_begin)");
  e->auto_buf = dev_buf;
  e->auto_plane = plane;
  e->auto_round = -1;
  return P2PG_OK;
}

int p2pg_exchange_pack_live(p2pg_engine* e, int32_t plane, void* dev_buf, int64_t* counts) {
  if (!e || !e->have_state || e->round == 0 || (plane != 0 && plane != 1) || !dev_buf || !counts)
    return fail(e, P2PG_ERR_STATE, "exchange_pack_live: need a completed round, plane 0 or 1, buffers");
  if (!e->d_seg_cnt) return fail(e, P2PG_ERR_STATE, "exchange_pack_live: set_exchange_segments first");
  if (e->begun) return fail(e, P2PG_ERR_STATE, "exchange_pack_live: the next round has begun");
  if (plane == 1 && e->cfg.mode != P2PG_MODE_GOSSIP)
    return fail(e, P2PG_ERR_ARG, "exchange_pack_live: plane 1 is for gossip pushes");
  const int nseg = (int)e->send_seg.size() - 1;
  if (dev_buf == e->auto_buf && plane == e->auto_plane && e->auto_round == e->round - 1) {
    // packed by the round itself (p2pg_set_exchange_buffer), counts read with its counters
    for (int q = 0; q < nseg; ++q) counts[q] = e->auto_cnt[q];
    e->auto_round = -1;  // handed over once
    return P2PG_OK;
  }
  HIPCHK(e, hipSetDevice(e->cfg.device));
  // plane 0 moves frontier rows owner -> ghost (send list); plane 1 pushes ghost -> owner
  const bool fwd = plane == 0;
  const int32_t* ids = fwd ? e->d_send : e->d_recv;
  const int64_t n = fwd ? e->n_send : e->n_recv;
  const int64_t* seg = fwd ? e->d_send_seg : e->d_recv_seg;
  HIPCHK(e, hipMemsetAsync(e->d_seg_cnt, 0, sizeof(unsigned long long) * P2PG_MAX_RANKS, e->stream));
  hipError_t r = launch_pack_live(e->st, plane, e->round - 1, ids, n, seg, nseg, e->d_seg_cnt,
                                  (int64_t*)dev_buf, e->stream);
  if (r == hipSuccess)
    r = hipMemcpyAsync(e->h_seg_cnt, e->d_seg_cnt, sizeof(unsigned long long) * nseg, hipMemcpyDeviceToHost,
                       e->stream);
  if (r == hipSuccess) r = hipStreamSynchronize(e->stream);
  if (r != hipSuccess) return fail(e, P2PG_ERR_HIP, std::string("exchange_pack_live: ") + hipGetErrorString(r));
  for (int q = 0; q < nseg; ++q) counts[q] = (int64_t)e->h_seg_cnt[q];
  return P2PG_OK;
}

int p2pg_exchange_unpack_live(p2pg_engine* e, int32_t plane, const void* dev_buf, const int64_t* counts) {
  if (!e || !e->have_state || e->round == 0 || (plane != 0 && plane != 1) || !counts)
    return fail(e, P2PG_ERR_STATE, "exchange_unpack_live: need a completed round, plane 0 or 1, counts");
  if (!e->d_seg_cnt) return fail(e, P2PG_ERR_STATE, "exchange_unpack_live: set_exchange_segments first");
  HIPCHK(e, hipSetDevice(e->cfg.device));
  const int nseg = (int)e->send_seg.size() - 1;
  const bool fwd = plane == 0;  // plane 0 lands in the recv list (ghosts), plane 1 in the send list
  const int32_t* ids = fwd ? e->d_recv : e->d_send;
  const std::vector<int64_t>& lst = fwd ? e->recv_seg : e->send_seg;
  const int64_t* lseg = fwd ? e->d_recv_seg : e->d_send_seg;
  int64_t ro[P2PG_MAX_RANKS + 1] = {0};
  for (int q = 0; q < nseg; ++q) {
    if (counts[q] < 0 || counts[q] > lst[q + 1] - lst[q])
      return fail(e, P2PG_ERR_ARG, "exchange_unpack_live: more records than the list segment holds");
    ro[q + 1] = ro[q] + counts[q];
  }
  if (ro[nseg] > 0 && !dev_buf) return fail(e, P2PG_ERR_ARG, "exchange_unpack_live: no buffer");
  // asynchronous on the engine stream: the next step orders after it
  hipError_t r = launch_unpack_live(e->st, plane, e->round - 1, ids, lseg, nseg, ro, (const int64_t*)dev_buf,
                                    e->stream);
  if (r != hipSuccess) return fail(e, P2PG_ERR_HIP, std::string("exchange_unpack_live: ") + hipGetErrorString(r));
  return P2PG_OK;
}

static int exchange(p2pg_engine* e, int32_t plane, bool pack, void* buf) {
  if (!e || !e->have_state || e->round == 0 || (plane != 0 && plane != 1))
    return fail(e, P2PG_ERR_STATE, "exchange: need a completed round and plane 0 or 1");
  if (e->begun) return fail(e, P2PG_ERR_STATE, "exchange: the next round has begun");
  if (plane == 1 && e->cfg.mode != P2PG_MODE_GOSSIP)
    return fail(e, P2PG_ERR_ARG, "exchange: plane 1 is for gossip pushes");
  HIPCHK(e, hipSetDevice(e->cfg.device));
  const int r = e->round - 1;  // the round step() completed
  // plane 0 moves frontier rows owner -> ghost; plane 1 moves pushed rows ghost -> owner
  const bool use_send_list = (plane == 0) == pack;
  const int32_t* ids = use_send_list ? e->d_send : e->d_recv;
  const int64_t n = use_send_list ? e->n_send : e->n_recv;
  hipError_t rr = pack ? launch_pack(e->st, plane, r, ids, n, (uint64_t*)buf, e->stream)
                       : launch_unpack(e->st, plane, r, ids, n, (const uint64_t*)buf, e->stream);
  if (rr == hipSuccess) rr = hipStreamSynchronize(e->stream);
  if (rr != hipSuccess) return fail(e, P2PG_ERR_HIP, std::string("exchange: ") + hipGetErrorString(rr));
  return P2PG_OK;
}

int p2pg_exchange_pack(p2pg_engine* e, int32_t plane, void* dev_buf) {
  return exchange(e, plane, true, dev_buf);
}

int p2pg_exchange_unpack(p2pg_engine* e, int32_t plane, const void* dev_buf) {
  return exchange(e, plane, false, const_cast<void*>(dev_buf));
}

int p2pg_update_edges(p2pg_engine* e, int64_t n_add, const int32_t* add, int64_t n_del,
                      const int32_t* del) {
  if (!e || !e->d_rowptr || n_add < 0 || n_del < 0 || (n_add && !add) || (n_del && !del))
    return fail(e, P2PG_ERR_ARG, "update_edges: bad arguments");
  if (e->d_gid || (e->cfg.flags & P2PG_FLAG_LOCAL_GRAPH))
    return fail(e, P2PG_ERR_STATE, "update_edges: not supported on a vertex-partitioned rank");
  if (e->ae.on())
    return fail(e, P2PG_ERR_STATE, "update_edges: not available while anti-entropy is set (p2pg_set_anti_entropy)");
  if (e->ns_win.on())
    return fail(e, P2PG_ERR_STATE, "update_edges: not available while a netsplit is set (p2pg_set_netsplit)");
  if (e->arr_round >= 0 && e->arr_round == e->round)
    return fail(e, P2PG_ERR_STATE, "update_edges: one update per round boundary");
  if (e->begun) return fail(e, P2PG_ERR_STATE, "update_edges: a round has begun (step_begin)");
  if (deferred_on(e) && e->have_state && e->tally_read_at == e->round)
    return fail(e, P2PG_ERR_STATE, "update_edges: p2pg_peer_counters / p2pg_message_cost has counted this round's sends already; "
                                   "read the counters after the changes of a round boundary");
  const int64_t V = e->V;
  const std::vector<int64_t>& rp = e->h_rowptr;
  const std::vector<int32_t>& ci = e->h_colidx;
  auto slot_of = [&](int32_t a, int32_t b) -> int64_t {  // slot of b in a's row, or -1
    const int32_t* beg = ci.data() + rp[a];
    const int32_t* end = ci.data() + rp[a + 1];
    const int32_t* it = std::lower_bound(beg, end, b);
    return (it != end && *it == b) ? (int64_t)(it - ci.data()) : -1;
  };
  // both directions of every change, sorted by (row, neighbour)
  std::vector<std::pair<int32_t, int32_t>> adds, dels;
  auto collect = [&](int64_t n, const int32_t* pr, bool is_add,
                     std::vector<std::pair<int32_t, int32_t>>& out) -> int {
    for (int64_t i = 0; i < n; ++i) {
      const int32_t a = pr[2 * i], b = pr[2 * i + 1];
      if (a < 0 || b < 0 || a >= V || b >= V)
        return fail(e, P2PG_ERR_ARG, "update_edges: peer id out of range");
      if (a == b)  // node.py:131-133 refuses self connections
        return fail(e, P2PG_ERR_ARG, "update_edges: self connection");
      const bool exists = slot_of(a, b) >= 0;
      if (is_add && exists)  // node.py:136-139: already connected
        return fail(e, P2PG_ERR_ARG, "update_edges: connection already exists");
      if (!is_add && !exists)  // node.py:178-189: not connected
        return fail(e, P2PG_ERR_ARG, "update_edges: no such connection");
      out.emplace_back(a, b);
      out.emplace_back(b, a);
    }
    std::sort(out.begin(), out.end());
    if (std::adjacent_find(out.begin(), out.end()) != out.end())
      return fail(e, P2PG_ERR_ARG, "update_edges: a connection is listed twice");
    return P2PG_OK;
  };
  int rc;
  if ((rc = collect(n_add, add, true, adds))) return rc;
  if ((rc = collect(n_del, del, false, dels))) return rc;
  HIPCHK(e, hipSetDevice(e->cfg.device));
  // new adjacency: each row = old row - removed + added, ascending
  std::vector<int64_t> nrp(V + 1, 0);
  std::vector<int32_t> nci;
  nci.reserve(ci.size() + adds.size());
  {
    size_t ia = 0, id = 0;
    for (int64_t v = 0; v < V; ++v) {
      std::vector<int32_t> plus;
      while (ia < adds.size() && adds[ia].first == v) plus.push_back(adds[ia++].second);
      size_t k = 0;
      for (int64_t j = rp[v]; j < rp[v + 1]; ++j) {
        const int32_t u = ci[j];
        if (id < dels.size() && dels[id].first == v && dels[id].second == u) {
          ++id;
          continue;
        }
        while (k < plus.size() && plus[k] < u) nci.push_back(plus[k++]);
        nci.push_back(u);
      }
      while (k < plus.size()) nci.push_back(plus[k++]);
      nrp[v + 1] = (int64_t)nci.size();
    }
  }
  const bool running = e->have_state && e->round > 0 && !e->done;
  if (running) {
    // Messages sent in the last round are in flight on the OLD connections: the ones on removed
    // connections are lost (a stopped NodeConnection drops its unread buffer,
    // nodeconnection.py:192-228), the rest arrive next round.  Materialize them as row pushes
    // next[round&1] over the old graph minus the removed slots, before the graph changes.
    DevState& s = e->st;
    const bool gossip = e->cfg.mode == P2PG_MODE_GOSSIP;
    {  // hop limits: the last round's expired receipts have nothing in flight (the gossip pushes
       // are redone below)
      const int xrc = finalize_expiry(e, false);
      if (xrc) return xrc;
    }
    std::vector<uint8_t> gone(ci.size(), 0);
    for (const auto& d : dels) gone[slot_of(d.first, d.second)] = 1;
    uint8_t* d_gone = nullptr;
    HIPCHK(e, hipMalloc((void**)&d_gone, gone.empty() ? 1 : gone.size()));
    hipError_t gr = gone.empty() ? hipSuccess : hipMemcpy(d_gone, gone.data(), gone.size(), hipMemcpyHostToDevice);
    if (gr == hipSuccess) {
      // tallies: the last round's sends are final now -- the ones on removed connections are lost
      DevGraph gs = graph(e);
      gs.gone = d_gone;
      gr = flush_peer_tally(e, gs);
      // (it reads the arrival graph freed below)
      if (gr == hipSuccess && deferred_on(e)) gr = hipStreamSynchronize(e->stream);
    }
    if (gr != hipSuccess) {
      (void)hipFree(d_gone);
      return fail(e, P2PG_ERR_HIP, std::string("update_edges: ") + hipGetErrorString(gr));
    }
    if (!dels.empty()) {
      // the arrivals of the next round lose the sends in flight on the removed connections: count
      // the last round's lost sends again with those slots gone (churn losses included), while the
      // graph its own arrivals travelled on (the senders' first receipts) is still at hand
      DevGraph gs = graph(e);
      gs.gone = d_gone;
      hipError_t x = enqueue_lost_count(e, gs, graph_for_arrivals(e, e->round - 1), e->round - 1);
      if (x == hipSuccess) x = hipStreamSynchronize(e->stream);
      if (x != hipSuccess) {
        (void)hipFree(d_gone);
        return fail(e, P2PG_ERR_HIP, std::string("update_edges (lost sends): ") + hipGetErrorString(x));
      }
      e->lost_last = (uint64_t)e->h_cnt2[1];
    }
    free_arr(e);
    e->d_gone = d_gone;
    if (!s.next[0]) {  // flood: row-push planes on first use
      for (int i = 0; i < 2; ++i) {
        HIPCHK(e, hipMalloc((void**)&s.next[i], e->plane_bytes ? e->plane_bytes : 8));
        HIPCHK(e, hipMalloc((void**)&s.T[i], e->bm_bytes ? e->bm_bytes : 8));
        HIPCHK(e, hipMemsetAsync(s.next[i], 0, e->plane_bytes, e->stream));
        HIPCHK(e, hipMemsetAsync(s.T[i], 0, e->bm_bytes, e->stream));
      }
    }
    DevGraph gold = graph(e);
    gold.gone = e->d_gone;
    RoundParams p = params(e);
    const int nx = e->round & 1;
    hipError_t lr;
    if (!gossip) {
      if (!e->consume_next) {
        lr = launch_materialize(gold, s, p, true, e->stream);
        if (lr != hipSuccess) return fail(e, P2PG_ERR_HIP, std::string("update_edges: ") + hipGetErrorString(lr));
      }
    } else {
      // the pushes of the last round, recomputed (Philox picks are a pure function of the
      // round, peer and message) as row atomics over the old graph without the removed slots
      HIPCHK(e, hipMemsetAsync(s.next[nx], 0, e->plane_bytes, e->stream));
      HIPCHK(e, hipMemsetAsync(s.T[nx], 0, e->bm_bytes, e->stream));
      p.round = e->round - 1;
      lr = launch_scatter_atomic(e, gold, p, e->hist.prev_aw);
      if (lr != hipSuccess) return fail(e, P2PG_ERR_HIP, std::string("update_edges: ") + hipGetErrorString(lr));
    }
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (e->wlist_check) {
      unsigned long long listed = 0;
      HIPCHK(e, hipMemcpy(&listed, s.stats + STAT_COUNT, sizeof(listed), hipMemcpyDeviceToHost));
      if (int rc2 = check_scatter_list(e, listed)) return rc2;
    }
    e->consume_next = true;
    e->hist.last_push_e = false;
    e->stats_clear = true;  // the re-push above counted into the round counters
    // keep the old rows for the parents of the receiving round (record / deliveries)
    e->d_rowptr_arr = e->d_rowptr;
    e->d_colidx_arr = e->d_colidx;
    e->d_rowptr = nullptr;
    e->d_colidx = nullptr;
    e->arr_round = e->round;
  } else if (deferred_on(e) && e->tally_pending >= 0) {
    // a finished run: its last round's sends (none pass a quiet round) over the graph they left on
    hipError_t x = flush_peer_tally(e, graph(e));
    if (x == hipSuccess) x = hipStreamSynchronize(e->stream);
    if (x != hipSuccess) return fail(e, P2PG_ERR_HIP, std::string("update_edges (peer counters): ") + hipGetErrorString(x));
  }
  std::vector<uint32_t> rev;
  if ((rc = check_csr(e, V, nrp.data(), nci.data(), rev))) return rc;
  if ((rc = upload_graph(e, V, nrp.data(), nci.data(), rev))) return rc;
  if (e->have_state && (rc = alloc_edge_planes(e))) return rc;
  return P2PG_OK;
}

}  // extern "C"

namespace {

constexpr uint64_t SNAP_MAGIC = 0x50414E5347503250ull;  // "P2PGSNAP"
constexpr uint32_t SNAP_VERSION = 3;  // 2: + last_new; 3: + sent_last / lost_last

struct SnapHeader {
  uint64_t magic;
  uint32_t version, mode;
  int64_t V, nnz;
  int32_t M, W, fanout, round;
  uint32_t flags, churn_threshold, msg_id_base, done;
  uint32_t consume_next, has_next;
  uint64_t gossip_seed, churn_seed, graph_hash, src_hash, total_relays, prev_aw, prev_av;
  uint64_t last_new;  // first receipts of the last round (deliveries, decay-phase push dedup)
  uint64_t sent_last, lost_last;  // the next round's arrivals (p2pg_round_stats.received)
};

uint64_t fnv1a(uint64_t h, const void* data, size_t n) {
  const unsigned char* p = (const unsigned char*)data;
  for (size_t i = 0; i < n; ++i) {
    h ^= p[i];
    h *= 0x100000001B3ull;
  }
  return h;
}

uint64_t graph_hash(const p2pg_engine* e) {
  uint64_t h = fnv1a(0xCBF29CE484222325ull, e->h_rowptr.data(), e->h_rowptr.size() * sizeof(int64_t));
  return fnv1a(h, e->h_colidx.data(), e->h_colidx.size() * sizeof(int32_t));
}

int64_t snapshot_bytes(const p2pg_engine* e, bool with_next, bool with_record) {
  int64_t n = (int64_t)sizeof(SnapHeader) + 2 * (int64_t)e->plane_bytes + 2 * (int64_t)e->bm_bytes;
  if (with_next) n += (int64_t)e->plane_bytes + (int64_t)e->bm_bytes;
  if (with_record) n += 2 * (int64_t)e->V * e->M * (int64_t)sizeof(int32_t);
  return n;
}

int64_t snapshot_bytes(const p2pg_engine* e) {
  return snapshot_bytes(e, e->st.next[0] != nullptr, e->st.hop != nullptr);
}

// The planes of a snapshot, in order: seen, saturated bits, the last round's activity bits and
// frontier (its first receipts), [pending row pushes + their bits], [hop, parent].
template <class F>
int for_planes(p2pg_engine* e, bool with_next, F&& f) {
  DevState& s = e->st;
  const int last = (e->round + 1) & 1;  // (round - 1) & 1
  const int nx = e->round & 1;
  int rc;
  if ((rc = f((void*)s.seen, e->plane_bytes))) return rc;
  if ((rc = f((void*)s.S, e->bm_bytes))) return rc;
  if ((rc = f((void*)s.A[last], e->bm_bytes))) return rc;
  if ((rc = f((void*)s.F[last], e->plane_bytes))) return rc;
  if (with_next) {
    if ((rc = f((void*)s.next[nx], e->plane_bytes))) return rc;
    if ((rc = f((void*)s.T[nx], e->bm_bytes))) return rc;
  }
  if (s.hop) {
    const size_t hb = (size_t)e->V * e->M * sizeof(int32_t);
    if ((rc = f((void*)s.hop, hb))) return rc;
    if ((rc = f((void*)s.parent, hb))) return rc;
  }
  return P2PG_OK;
}

}  // namespace

extern "C" {

int p2pg_snapshot_size(p2pg_engine* e, int64_t* bytes) {
  if (!e || !bytes) return fail(e, P2PG_ERR_ARG, "snapshot_size: bad arguments");
  if (!e->have_state) return fail(e, P2PG_ERR_STATE, "snapshot_size: no sources set");
  *bytes = snapshot_bytes(e);
  return P2PG_OK;
}

int p2pg_snapshot(p2pg_engine* e, void* buf, int64_t cap) {
  if (!e || !buf) return fail(e, P2PG_ERR_ARG, "snapshot: bad arguments");
  if (!e->have_state) return fail(e, P2PG_ERR_STATE, "snapshot: no sources set");
  if (tally_on(e))
    return fail(e, P2PG_ERR_STATE, "snapshot: snapshots do not hold run tallies (P2PG_FLAG_TALLY)");
  if (cost_on(e))
    return fail(e, P2PG_ERR_STATE, "snapshot: snapshots do not hold the per-message cost (P2PG_FLAG_MSG_COST)");
  if (latency_on(e))
    return fail(e, P2PG_ERR_STATE, "snapshot: snapshots do not hold the delivery latency (P2PG_FLAG_LATENCY)");
  if (e->late)
    return fail(e, P2PG_ERR_STATE, "snapshot: snapshots do not hold start rounds other than 0 "
                                   "(p2pg_set_sources_at / p2pg_originate)");
  if (e->ttl_on)
    return fail(e, P2PG_ERR_STATE, "snapshot: snapshots do not hold hop limits (p2pg_set_ttl)");
  if (e->pol_on)
    return fail(e, P2PG_ERR_STATE, "snapshot: snapshots do not hold a relay policy (p2pg_set_relay_policy)");
  if (e->down_on)
    return fail(e, P2PG_ERR_STATE, "snapshot: snapshots do not hold peer downtime (p2pg_set_downtime)");
  if (e->ns_win.on())
    return fail(e, P2PG_ERR_STATE, "snapshot: snapshots do not hold a netsplit (p2pg_set_netsplit)");
  if (e->ae.on())
    return fail(e, P2PG_ERR_STATE, "snapshot: snapshots do not hold anti-entropy exchanges (p2pg_set_anti_entropy)");
  if (e->begun) return fail(e, P2PG_ERR_STATE, "snapshot: a round has begun (step_begin)");
  if (e->arr_round >= 0 && e->arr_round == e->round)
    return fail(e, P2PG_ERR_STATE, "snapshot: take it before a topology update or after the next round");
  if (!e->frontier_kept)
    return fail(e, P2PG_ERR_STATE, "snapshot: the last round's frontier was not kept");
  if (e->d_gid && e->cfg.mode == P2PG_MODE_GOSSIP && e->hist.last_push_e && e->round > 0 && !e->done)
    return fail(e, P2PG_ERR_STATE,
                "snapshot: a partitioned rank holds this round's pushes per connection; take it "
                "after a sparse round");
  HIPCHK(e, hipSetDevice(e->cfg.device));
  DevState& s = e->st;
  if (e->cfg.mode == P2PG_MODE_GOSSIP && e->hist.last_push_e && e->round > 0 && !e->done) {
    // pushes held per connection (E) -> row pushes, so the state does not depend on slots
    RoundParams p = params(e);
    hipError_t lr = launch_materialize(graph(e), s, p, false, e->stream);
    if (lr != hipSuccess) return fail(e, P2PG_ERR_HIP, std::string("snapshot: ") + hipGetErrorString(lr));
    e->hist.last_push_e = false;
    e->stats_clear = true;
  }
  HIPCHK(e, hipStreamSynchronize(e->stream));
  const int64_t need = snapshot_bytes(e);
  if (cap < need) return fail(e, P2PG_ERR_ARG, "snapshot: buffer smaller than p2pg_snapshot_size");
  SnapHeader h{};
  h.magic = SNAP_MAGIC;
  h.version = SNAP_VERSION;
  h.mode = (uint32_t)e->cfg.mode;
  h.V = e->V;
  h.nnz = e->nnz;
  h.M = e->M;
  h.W = e->W;
  h.fanout = e->cfg.fanout;
  h.round = e->round;
  h.flags = e->cfg.flags & P2PG_FLAG_RECORD;
  h.churn_threshold = e->cfg.churn_threshold;
  h.msg_id_base = e->cfg.msg_id_base;
  h.done = e->done ? 1u : 0u;
  h.consume_next = e->consume_next ? 1u : 0u;
  h.has_next = s.next[0] ? 1u : 0u;
  h.gossip_seed = e->cfg.gossip_seed;
  h.churn_seed = e->cfg.churn_seed;
  h.graph_hash = graph_hash(e);
  h.src_hash = fnv1a(0xCBF29CE484222325ull, e->h_src.data(), e->h_src.size() * sizeof(int32_t));
  h.total_relays = e->total_relays;
  h.prev_aw = e->hist.prev_aw;
  h.prev_av = e->hist.prev_av;
  h.last_new = e->hist.last_new;
  h.sent_last = e->sent_last;
  h.lost_last = e->lost_last;
  char* out = (char*)buf;
  std::memcpy(out, &h, sizeof(h));
  size_t off = sizeof(h);
  return for_planes(e, s.next[0] != nullptr, [&](void* dev, size_t n) -> int {
    if (n) HIPCHK(e, hipMemcpy(out + off, dev, n, hipMemcpyDeviceToHost));
    off += n;
    return P2PG_OK;
  });
}

int p2pg_restore(p2pg_engine* e, const void* buf, int64_t size) {
  if (!e || !buf || size < (int64_t)sizeof(SnapHeader)) return fail(e, P2PG_ERR_ARG, "restore: bad arguments");
  if (!e->have_state) return fail(e, P2PG_ERR_STATE, "restore: set the same sources first");
  if (tally_on(e))
    return fail(e, P2PG_ERR_STATE, "restore: snapshots do not hold run tallies (P2PG_FLAG_TALLY)");
  if (cost_on(e))
    return fail(e, P2PG_ERR_STATE, "restore: snapshots do not hold the per-message cost (P2PG_FLAG_MSG_COST)");
  if (latency_on(e))
    return fail(e, P2PG_ERR_STATE, "restore: snapshots do not hold the delivery latency (P2PG_FLAG_LATENCY)");
  if (e->late)
    return fail(e, P2PG_ERR_STATE, "restore: snapshots do not hold start rounds other than 0 "
                                   "(p2pg_set_sources_at / p2pg_originate)");
  if (e->ttl_on)
    return fail(e, P2PG_ERR_STATE, "restore: snapshots do not hold hop limits (p2pg_set_ttl)");
  if (e->pol_on)
    return fail(e, P2PG_ERR_STATE, "restore: snapshots do not hold a relay policy (p2pg_set_relay_policy)");
  if (e->down_on)
    return fail(e, P2PG_ERR_STATE, "restore: snapshots do not hold peer downtime (p2pg_set_downtime)");
  if (e->ns_win.on())
    return fail(e, P2PG_ERR_STATE, "restore: snapshots do not hold a netsplit (p2pg_set_netsplit)");
  if (e->ae.on())
    return fail(e, P2PG_ERR_STATE, "restore: snapshots do not hold anti-entropy exchanges (p2pg_set_anti_entropy)");
  if (e->begun) return fail(e, P2PG_ERR_STATE, "restore: a round has begun (step_begin)");
  SnapHeader h;
  std::memcpy(&h, buf, sizeof(h));
  if (h.magic != SNAP_MAGIC || h.version != SNAP_VERSION)
    return fail(e, P2PG_ERR_ARG, "restore: not a relay-engine snapshot");
  if (h.mode != (uint32_t)e->cfg.mode || h.fanout != e->cfg.fanout ||
      h.gossip_seed != e->cfg.gossip_seed || h.churn_seed != e->cfg.churn_seed ||
      h.churn_threshold != e->cfg.churn_threshold || h.msg_id_base != e->cfg.msg_id_base ||
      h.flags != (e->cfg.flags & P2PG_FLAG_RECORD))
    return fail(e, P2PG_ERR_STATE, "restore: engine configuration differs from the snapshot's");
  if (h.V != e->V || h.nnz != e->nnz || h.graph_hash != graph_hash(e))
    return fail(e, P2PG_ERR_STATE, "restore: graph differs from the snapshot's");
  if (h.M != e->M || h.src_hash != fnv1a(0xCBF29CE484222325ull, e->h_src.data(), e->h_src.size() * sizeof(int32_t)))
    return fail(e, P2PG_ERR_STATE, "restore: broadcast sources differ from the snapshot's");
  // validate everything before the engine is touched: a rejected snapshot leaves it as it was
  if (h.round < 0 || h.has_next > 1 || h.done > 1 || h.consume_next > 1 ||
      (h.consume_next && !h.has_next))
    return fail(e, P2PG_ERR_ARG, "restore: corrupt snapshot header");
  const bool with_next = h.has_next != 0;
  if (size < snapshot_bytes(e, with_next, (h.flags & P2PG_FLAG_RECORD) != 0))
    return fail(e, P2PG_ERR_ARG, "restore: snapshot truncated");
  HIPCHK(e, hipSetDevice(e->cfg.device));
  DevState& s = e->st;
  if (with_next && !s.next[0]) {  // flood run that had a topology update
    for (int i = 0; i < 2; ++i) {
      HIPCHK(e, hipMalloc((void**)&s.next[i], e->plane_bytes ? e->plane_bytes : 8));
      HIPCHK(e, hipMalloc((void**)&s.T[i], e->bm_bytes ? e->bm_bytes : 8));
    }
  }
  int rc = p2pg_reset(e);
  if (rc) return rc;
  if (s.next[0]) {  // pending pushes: from the snapshot, or none (a flood snapshot without them)
    for (int i = 0; i < 2; ++i) {
      HIPCHK(e, hipMemsetAsync(s.next[i], 0, e->plane_bytes, e->stream));
      HIPCHK(e, hipMemsetAsync(s.T[i], 0, e->bm_bytes, e->stream));
    }
  }
  HIPCHK(e, hipStreamSynchronize(e->stream));
  e->round = h.round;
  e->done = h.done != 0;
  e->consume_next = h.consume_next != 0;
  e->total_relays = h.total_relays;
  e->hist.prev_aw = h.prev_aw;
  e->hist.prev_av = h.prev_av;
  e->hist.last_new = h.last_new;
  e->sent_last = h.sent_last;
  e->lost_last = h.lost_last;
  // the snapshot holds the last round's frontier, not the one before it, so that round's
  // delivery parents cannot be found (round 0's are -1): deliveries refuse it, as documented
  e->frontier_kept = true;
  e->frontier_kept_prev = h.round <= 1;
  // (the reset above left no growth history: no update+push prediction, no dense phase seen)
  const char* in = (const char*)buf;
  size_t off = sizeof(h);
  rc = for_planes(e, with_next, [&](void* dev, size_t n) -> int {
    if (n) HIPCHK(e, hipMemcpy(dev, in + off, n, hipMemcpyHostToDevice));
    off += n;
    return P2PG_OK;
  });
  if (rc) return rc;
  HIPCHK(e, hipMemsetAsync(s.A[e->round & 1], 0, e->bm_bytes, e->stream));
  // the last round's active-word masks are not in the snapshot: rebuilt from its frontier rows
  // (a re-push after a topology update, and the next sparse push, list words by them)
  if (e->round > 0) {
    hipError_t x = launch_rebuild_aw(s, e->round - 1, e->V, e->stream);
    if (x == hipSuccess) x = hipStreamSynchronize(e->stream);
    if (x != hipSuccess) return fail(e, P2PG_ERR_HIP, std::string("restore: ") + hipGetErrorString(x));
  }
  return P2PG_OK;
}

int p2pg_kernel_times(p2pg_engine* e, double ms[P2PG_KCLASS_N], int64_t launches[P2PG_KCLASS_N]) {
  if (!e) return P2PG_ERR_ARG;
  if (!e->ev_cls.empty()) {
    // launches still unresolved: a run whose last rounds went without a counter read-back (a
    // batched flood or decay tail) -- wait for them, so the sums cover every launch counted
    HIPCHK(e, hipSetDevice(e->cfg.device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    const int r = resolve_timings(e);
    if (r) return r;
  }
  for (int i = 0; i < P2PG_KCLASS_N; ++i) {
    if (ms) ms[i] = e->kms[i];
    if (launches) launches[i] = e->klaunch[i];
  }
  return P2PG_OK;
}

int p2pg_set_timed_classes(p2pg_engine* e, uint32_t mask) {
  if (!e) return P2PG_ERR_ARG;
  if (mask >> P2PG_KCLASS_N) return fail(e, P2PG_ERR_ARG, "set_timed_classes: unknown class bit");
  e->timed_mask = mask;
  return P2PG_OK;
}

int p2pg_device_philox(p2pg_engine* e, int32_t n, const uint32_t* ctr, const uint32_t key[2],
                       uint32_t* out) {
  if (!e || n < 0 || (n > 0 && (!ctr || !key || !out))) return fail(e, P2PG_ERR_ARG, "device_philox: bad arguments");
  if (n == 0) return P2PG_OK;
  HIPCHK(e, hipSetDevice(e->cfg.device));
  uint32_t *dc = nullptr, *dout = nullptr;
  HIPCHK(e, hipMalloc((void**)&dc, sizeof(uint32_t) * 4 * n));
  HIPCHK(e, hipMalloc((void**)&dout, sizeof(uint32_t) * 4 * n));
  hipError_t r = hipMemcpy(dc, ctr, sizeof(uint32_t) * 4 * n, hipMemcpyHostToDevice);
  if (r == hipSuccess) r = launch_philox(n, dc, key[0], key[1], dout, e->stream);
  if (r == hipSuccess) r = hipStreamSynchronize(e->stream);
  if (r == hipSuccess) r = hipMemcpy(out, dout, sizeof(uint32_t) * 4 * n, hipMemcpyDeviceToHost);
  (void)hipFree(dc);
  (void)hipFree(dout);
  if (r != hipSuccess) return fail(e, P2PG_ERR_HIP, std::string("device_philox: ") + hipGetErrorString(r));
  return P2PG_OK;
}

const char* p2pg_last_error(const p2pg_engine* e) { return e ? e->err.c_str() : p2pg_global_error(); }

void p2pg_destroy(p2pg_engine* e) {
  if (!e) return;
  (void)hipSetDevice(e->cfg.device);
  (void)hipStreamSynchronize(e->stream);
  free_state(e);
  free_graph(e);
  if (e->h_stats) (void)hipHostFree(e->h_stats);
  if (e->h_bstats) (void)hipHostFree(e->h_bstats);
  if (e->d_bstats) (void)hipFree(e->d_bstats);
  for (int i = 0; i < 2; ++i)
    if (e->ev[i]) (void)hipEventDestroy(e->ev[i]);
  for (hipEvent_t ev : e->ev_pool) (void)hipEventDestroy(ev);
  if (e->ev_sync) (void)hipEventDestroy(e->ev_sync);
  if (e->ev_spare) (void)hipEventDestroy(e->ev_spare);
  if (e->ev_main) (void)hipEventDestroy(e->ev_main);
  if (e->side) (void)hipStreamDestroy(e->side);
  if (e->own_stream) (void)hipStreamDestroy(e->own_stream);
  delete e;
}

}  // extern "C"
