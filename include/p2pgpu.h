/*
 * p2pgpu.h -- C-ABI of the MI355X broadcast/relay engine (libp2pgpu.so).
 *
 * The engine replaces, for ONE hot path, what a p2pnetwork application does with
 * Node.send_to_nodes + node_message + a message-id "seen" set (the dedup/no-echo contract of
 * /root/reference/README.md:20): it runs that flood relay, and a push-gossip variant, over a
 * whole simulated peer graph at once, 64 concurrent broadcasts per uint64 bitset word.
 *
 * Reference interface each entry point replaces (file:line in pj8912/python-p2p-network):
 *   p2pg_load_csr / p2pg_graph_*  <- the topology built by Node.connect_with_node
 *                                    (p2pnetwork/node.py:122-176); a peer's neighbour list is
 *                                    Node.all_nodes = nodes_inbound + nodes_outbound (node.py:75-78)
 *   p2pg_set_sources              <- the originating Node.send_to_nodes(data) call per broadcast
 *                                    (node.py:106-112)
 *   p2pg_set_sources_at /         <- the same call made later in the run: an app says something
 *   p2pg_originate                   whenever it has something to say (node.py:106-112), so each
 *                                    broadcast has its own start round
 *   p2pg_set_ttl                  <- a hop budget in the payload, forwarded as ttl - 1 while
 *                                    ttl > 0 (README.md:20; the sends are node.py:106-116)
 *   p2pg_step / p2pg_run          <- one / all rounds of: NodeConnection.run receive loop
 *                                    (nodeconnection.py:186-218) -> Node.node_message
 *                                    (node.py:334-338) -> app dedup -> send_to_nodes(data,
 *                                    exclude=[sender]) (node.py:106-112) -> send_to_node
 *                                    (node.py:114-120, message_count_send += 1 at :116)
 *   p2pg_round_stats.relays       <- sum over peers of Node.message_count_send (node.py:65,116)
 *   p2pg_get_new_deliveries       <- the node_message(node, data) events of one round, as
 *                                    (peer, msg, hop, parent) records (node.py:334-338)
 *   p2pg_get_sends                <- every Node.send_to_node call of one round (node.py:114-120),
 *                                    i.e. every packet NodeConnection.run hands to node_message
 *                                    the next round (nodeconnection.py:211-216), duplicates
 *                                    included, with the ones churn loses (nodeconnection.py:123-126)
 *   p2pg_drop_relays              <- an app whose node_message did not call send_to_nodes for a
 *                                    first receipt (README.md:20: the app decides)
 *   p2pg_round_stats.received     <- sum over peers of message_count_recv (nodeconnection.py:215)
 *   p2pg_read_planes              <- each app's "seen" set + first-receipt (hop, sender)
 *   p2pg_message_reach / _tally   <- per broadcast: how many apps' "seen" sets hold it, and the
 *                                    hops of the node_message events that put it there
 *   p2pg_peer_counters            <- per peer: Node.message_count_send / message_count_recv
 *                                    (node.py:65-67, :116; nodeconnection.py:215)
 *   p2pg_message_cost             <- per payload id: the send_to_node calls that carried it
 *                                    (node.py:116) and the packets of it that a receive loop
 *                                    handed on (nodeconnection.py:215)
 *   p2pg_message_latency /        <- the node_message events that pass the app's dedup
 *   p2pg_peer_latency                (node.py:334-338, README.md:20), by how many rounds after the
 *                                    broadcast's own start they happened: per broadcast a
 *                                    histogram, per peer their sum / number / largest
 *   p2pg_last_error             <- (reference swallows errors via debug_print, node.py:80-83)
 *
 * Conventions: plain C types only; 0 = OK, negative = error (message via p2pg_last_error);
 * no exceptions cross the ABI; the engine owns all device memory; caller keeps ownership of
 * every host array it passes; one engine per host thread (not re-entrant).
 */
#ifndef P2PGPU_H
#define P2PGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define P2PG_OK 0
#define P2PG_ERR_ARG (-1)
#define P2PG_ERR_STATE (-2)
#define P2PG_ERR_HIP (-3)
#define P2PG_ERR_NOMEM (-4)
#define P2PG_ERR_GRAPH (-5)

#define P2PG_MODE_FLOOD 0  /* forward to all connections except the sender (node.py:106-112) */
#define P2PG_MODE_GOSSIP 1 /* push-gossip: k Philox-chosen connections      */

#define P2PG_PUSH_NONE 0   /* flood, or nothing pushed                                   */
#define P2PG_PUSH_ATOMIC 1 /* gossip sparse round: row atomicOr into the targets' rows    */
#define P2PG_PUSH_EDGE 2   /* gossip dense round: per-connection mask stores (E plane)    */
#define P2PG_PUSH_FUSED 3  /* as EDGE, in one pass with this round's pull of E            */
#define P2PG_PUSH_UPDATE_EDGE 4 /* as EDGE, in one pass with this round's update (the    */
                                /* row pushes of a sparse round before it)                */

#define P2PG_FLAG_RECORD 1u /* keep hop/parent planes [V][M] (validation scale)            */
#define P2PG_FLAG_TIMING 2u /* per-kernel HIP-event timing (p2pg_kernel_times)              */
#define P2PG_FLAG_NO_AUTOSTOP 4u /* partitioned runs: keep stepping after a locally quiet
                                    round (the caller decides global quiescence)          */
#define P2PG_FLAG_LOCAL_GRAPH 8u /* rank-local graph of a vertex partition: ghost peers have
                                    empty rows, so symmetry is checked between non-empty
                                    rows only; a ghost's reverse slot is marked, so at
                                    16 < W <= 64 gossip takes the dense rounds (per-
                                    connection pushes for local connections, row pushes for
                                    ghost ones, exchanged); narrower rows: row atomics only */

#define P2PG_FLAG_RECEIVED 16u /* churn runs: count every round's lost sends, so that
                                    p2pg_round_stats.received is exact (a counting pass over the
                                    round's frontier after each round: config 5 +100 %); without
                                    it a churn run reports the sends of the round before there
                                    (an upper bound, received_exact = 0)                     */

#define P2PG_FLAG_TALLY 32u /* run tallies on the device: per broadcast reach / hop sum / last
                                    hop (p2pg_message_tally), per peer Node.message_count_send /
                                    message_count_recv (p2pg_peer_counters).  2 V 8 + M 20 bytes of
                                    device memory (config 4: 160 MB); every round keeps its whole
                                    frontier rows, a column count follows each round and a per-peer
                                    pass precedes the next (the price: DESIGN.md 4g).  Not on a
                                    vertex-partitioned rank, not with snapshots                  */

#define P2PG_FLAG_MSG_COST 64u /* per-broadcast cost on the device: the send_to_node calls that
                                    carried message m and those of them that arrived
                                    (p2pg_message_cost).  Independent of P2PG_FLAG_TALLY (either,
                                    both or neither).  M 16 bytes of device memory and 512 KB of
                                    shard scratch per 4096 messages; every round keeps its whole frontier
                                    rows and a per-message pass over its sends precedes the next
                                    round (the price: DESIGN.md 4g).  Not on a vertex-partitioned
                                    rank, not with snapshots                                     */

#define P2PG_FLAG_LATENCY 128u /* delivery latency on the device: per broadcast a histogram of the
                                    relative hops (round - start round) of its first receipts
                                    (p2pg_message_latency), per peer their sum, number and largest
                                    (p2pg_peer_latency).  Independent of P2PG_FLAG_TALLY and
                                    P2PG_FLAG_MSG_COST (any combination).  M (bins 8 + 4) + V 16
                                    bytes of device memory (config 4: 160 MB per-peer, 2 MB of
                                    histograms at 64 bins), the start rounds as bit planes and,
                                    without P2PG_FLAG_TALLY, 256 KB of shard scratch per 4096
                                    messages; every round keeps its whole frontier rows, a column
                                    count and a per-peer pass follow each round (the price:
                                    DESIGN.md 4g).  Not on a vertex-partitioned rank, not with
                                    snapshots                                                    */

typedef struct p2pg_engine p2pg_engine;
typedef struct p2pg_graph p2pg_graph;

typedef struct p2pg_config {
  int32_t mode;              /* P2PG_MODE_*                                              */
  int32_t fanout;            /* gossip k (1..16); ignored for flood                       */
  uint64_t gossip_seed;      /* Philox key for gossip picks                               */
  uint64_t churn_seed;       /* Philox key for the per-round edge-drop mask               */
  uint32_t churn_threshold;  /* send lost iff philox(...).x < threshold; 0 = no churn    */
  uint32_t msg_id_base;      /* global id of local message 0 (message-axis sharding)      */
  uint32_t flags;            /* P2PG_FLAG_*                                               */
  int32_t device;            /* HIP device ordinal                                        */
} p2pg_config;

typedef struct p2pg_round_stats {
  int32_t round;             /* round index r (0 = origination)                           */
  int32_t active;            /* 1 if messages are still in flight after this round, or a
                                broadcast is scheduled to start in a later one            */
  uint64_t new_deliveries;   /* (peer,msg) first receipts in round r (= node_message events
                                that pass dedup)                                          */
  uint64_t relays;           /* send_to_node calls made in round r (message_count_send)   */
  uint64_t active_vertices;  /* |A_r|: peers with >= 1 first receipt in round r           */
  uint64_t active_words;     /* N_aw: nonzero (peer, word) of the round-r frontier        */
  uint64_t wedges;           /* sum over nonzero frontier words of deg(peer)              */
  uint64_t deg_active;       /* sum over A_r of deg(peer)                                 */
  uint64_t scatter_words;    /* gossip: nonzero (sender, target, word) masks pushed       */
  uint64_t touched_words;    /* gossip: nonzero pushed-to words consumed in round r       */
  int32_t push_form;         /* gossip: how round r's pushes left (P2PG_PUSH_*); flood 0    */
  int32_t received_exact;    /* 1: `received` is exact; 0: a churn run without
                                P2PG_FLAG_RECEIVED, `received` = the sends of round r-1     */
  uint64_t received;         /* packets that arrived in round r: the sends of round r-1 less
                                those lost to churn or to a connection removed in between
                                (sum over peers of message_count_recv += 1,
                                nodeconnection.py:215; duplicates included, 0 at round 0)  */
} p2pg_round_stats;

/* One anti-entropy exchange (p2pg_set_anti_entropy, p2pg_get_pull_stats): the requests of round
 * request_round, their replies of the round after, and what the replies repaired in the round
 * after that.  Pull packets are counted here only, never in the relay counters.              */
typedef struct p2pg_pull_stats {
  int32_t request_round;
  int32_t reserved;
  uint64_t requests;       /* request packets sent (one per online peer with a connection)      */
  uint64_t requests_lost;  /* ... lost: churn, or the partner offline in request_round + 1       */
  uint64_t replies;        /* reply packets sent = requests that arrived (empty replies too)     */
  uint64_t replies_lost;   /* ... lost: churn, or the requester offline in request_round + 2     */
  uint64_t repaired;       /* first receipts of request_round + 2 that no relay copy delivered   */
} p2pg_pull_stats;

/* ---- graphs (host side; no GPU needed) ---------------------------------------------- */
/* kind: 0 random d-regular (a = d), 1 G(n,p) with p = a / (V-1) (a = mean degree),
 *       2 Barabasi-Albert (a = m, initial (m+1)-clique), 3 Watts-Strogatz (a = k, b = beta),
 *       4 ring + chords (config 1: a = chord stride, 0 = none)                           */
int p2pg_graph_generate(int32_t kind, int64_t V, double a, double b, uint64_t seed,
                        p2pg_graph** out);
/* Build from an undirected edge list (any order, duplicates/self-loops dropped). */
int p2pg_graph_from_edges(int64_t V, int64_t n_edges, const int32_t* src, const int32_t* dst,
                          p2pg_graph** out);
int p2pg_graph_info(const p2pg_graph* g, int64_t* V, int64_t* nnz);
/* Borrowed pointers, valid until p2pg_graph_free. */
int p2pg_graph_arrays(const p2pg_graph* g, const int64_t** rowptr, const int32_t** colidx);
void p2pg_graph_free(p2pg_graph* g);
/* src[m] = lemire32(philox(key=(seed_lo, seed_hi ^ 'SRC'), ctr=(msg_id_base+m,0,0,0)).x, V) */
int p2pg_make_sources(int64_t V, int32_t M, uint64_t seed, uint32_t msg_id_base, int32_t* src);
/* Host Philox4x32-10 (KAT hook). */
void p2pg_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
/* Host evaluation of the engine's random draws (the wire bridge replays the sends of a run):
 * the connections (indices into the peer's ascending adjacency) a gossip first receipt of
 * message msg (global id) at peer in round `round` is pushed to, in draw order -- what
 * Node.send_to_node is called on (node.py:114-120); returns their number min(k, deg).     */
int p2pg_gossip_targets(uint32_t round, uint32_t peer, uint32_t msg, uint32_t deg, int32_t k,
                        uint64_t seed, uint32_t* out);
/* 1 iff a send over {a, b} made in round `round` is lost to churn.       */
int p2pg_churn_lost(uint32_t round, uint32_t a, uint32_t b, uint32_t threshold, uint64_t seed);
/* 1 iff the relay policy mutes the first receipt of message msg (global id) at peer in round
 * `round` under the peer's threshold thr (p2pg_set_relay_policy; the exemption of originations is
 * the caller's).                                                                            */
int p2pg_relay_muted(uint32_t round, uint32_t peer, uint32_t msg, uint32_t thr, uint64_t seed);
/* 1 iff a peer with the downtime interval [from, until) is offline in round `round`
 * (p2pg_set_downtime; from = -1: never).                                                    */
int p2pg_peer_offline(int32_t round, int32_t from, int32_t until);
/* 1 iff a connection between a peer of side_a and a peer of side_b is cut in round `round` under
 * the window [cut_from, cut_until) (p2pg_set_netsplit): side_a != side_b and cut_from <= round <
 * cut_until.                                                                                 */
int p2pg_link_cut(int32_t round, int32_t side_a, int32_t side_b, int32_t cut_from, int32_t cut_until);
/* The slot, in its ascending connection list of length deg >= 1, of the connection `peer` sends its
 * anti-entropy request of round `round` to under the key `seed` (p2pg_set_anti_entropy):
 * lemire32(philox4x32_10((round, peer, 0, 'AEP'), seed).x, deg).  -1 for deg = 0.            */
int32_t p2pg_pull_partner_slot(uint32_t round, uint32_t peer, uint32_t deg, uint64_t seed);

/* ---- engine ------------------------------------------------------------------------- */
int p2pg_create(const p2pg_config* cfg, p2pg_engine** out);
int p2pg_load_csr(p2pg_engine* e, int64_t V, const int64_t* rowptr, const int32_t* colidx);
int p2pg_set_sources(p2pg_engine* e, int32_t M, const int32_t* src);
/* Broadcasts that enter the network over time (Node.send_to_nodes(data) called at the origin
 * whenever the app has something to say, node.py:106-112): like p2pg_set_sources, and message m
 * originates at src[m] in round start[m] >= 0 instead of round 0; start[m] = -1 with src[m] = -1
 * declares an unscheduled message (it owns its bit column and does nothing until
 * p2pg_originate schedules it).  In round r the arrivals are received first, then every m with
 * start[m] == r originates: a first receipt of round r at the origin (hop r, parent -1) that
 * sends to all deg connections (flood) or to the min(k, deg) Philox picks of (r, origin,
 * msg_id_base + m) (gossip); those sends arrive in round r + 1 under round r's churn draw.
 * Hops stay absolute round indices everywhere.  p2pg_round_stats.active stays 1 while a
 * scheduled start lies ahead, so p2pg_run crosses idle gaps and stops after the last wave;
 * unscheduled messages keep no run alive.  p2pg_reset keeps the schedule and replays it.
 * start all zero is exactly p2pg_set_sources.  A gossip round with originations runs its
 * receive pass and its pushes as separate passes (never P2PG_PUSH_FUSED / _UPDATE_EDGE).
 * Not on a vertex-partitioned rank (P2PG_ERR_STATE); an engine whose schedule holds a start
 * other than 0 refuses p2pg_snapshot / p2pg_restore (P2PG_ERR_STATE).                       */
int p2pg_set_sources_at(p2pg_engine* e, int32_t M, const int32_t* src, const int32_t* start);
/* Between rounds: schedule the unscheduled messages msg[i] to originate at peer[i] in `round`
 * -- the send_to_nodes(data) an app decides on while it runs (node.py:106-112), e.g. a reply
 * made in a batched node_message hook.  round >= max(1, the next round to run); every msg[i]
 * in range, unscheduled and listed once; every peer[i] in range (P2PG_ERR_ARG otherwise,
 * nothing changed).  Wakes an engine that had gone quiet.  P2PG_ERR_STATE between
 * p2pg_step_begin / p2pg_step_end and on a vertex-partitioned rank.                        */
int p2pg_originate(p2pg_engine* e, int64_t n, const int32_t* msg, const int32_t* peer, int32_t round);
/* Hop limits: the hop budget an app puts into its payload and forwards as ttl - 1 while
 * ttl > 0 (README.md:20: the app decides whether its node_message calls send_to_nodes,
 * node.py:106-116).  ttl[m] >= 0 bounds message m, -1 leaves it unlimited.  A first receipt of m
 * in round r has relative hop h = r - start[m] (the origination is the receipt with h = 0).  It
 * happens exactly as without a limit -- seen bit, hop r, parent, new_deliveries and the other
 * receipt counters, the delivery stream, reach / hop_sum / last_hop -- and makes its sends iff
 * ttl[m] < 0 or h < ttl[m].  A receipt with h == ttl[m] makes none: they are in no round's
 * `relays`, no next round's `received` (with or without P2PG_FLAG_RECEIVED), not in
 * p2pg_get_sends, p2pg_peer_counters or the lost-send count; ttl 0 = the origin marks the message
 * seen and sends nothing.  So m has nothing in flight after its expiry round start[m] + ttl[m],
 * and a run with hop limits is the unlimited run cut off at relative hop ttl[m], message by
 * message, under churn and in gossip as well.  Hops stay absolute; `active` keeps its rule.
 * Call it after p2pg_set_sources / p2pg_set_sources_at and before round 0 runs, or after a
 * p2pg_reset: M = the engine's message count, every ttl[m] in [-1, 2^30] (P2PG_ERR_ARG
 * otherwise).  An unscheduled message keeps its limit for the round p2pg_originate gives it.
 * All -1, or ttl = NULL, removes the limits: the engine is then exactly the engine without this
 * call.  p2pg_reset keeps them and replays them; p2pg_set_sources[_at] clears them.
 * P2PG_ERR_STATE on a vertex-partitioned rank, between p2pg_step_begin / p2pg_step_end and once a
 * round has run; while a finite limit is set p2pg_snapshot / p2pg_restore return P2PG_ERR_STATE.
 * A rejected call changes nothing.
 * An expiry round's sends become final at the start of the next round or inside p2pg_get_sends,
 * p2pg_peer_counters, p2pg_message_cost, p2pg_update_edges or p2pg_drop_relays, whichever comes
 * first: read the
 * round's deliveries before those (as for p2pg_drop_relays) -- they hold all its receipts, the
 * expired messages' last ones included; afterwards p2pg_get_new_deliveries for that round returns
 * P2PG_ERR_STATE, never a shortened list.  p2pg_drop_relays of an expired receipt is legal and
 * cancels nothing.  A gossip expiry round runs the unfused schedule and its pushes leave by row
 * atomics when its sends become final: its scatter_words is 0 and its push_form
 * P2PG_PUSH_ATOMIC, and the next round's touched_words counts what that push touched (DESIGN.md
 * 4j).  Rounds without an expiry keep every form they have.                                    */
int p2pg_set_ttl(p2pg_engine* e, int32_t M, const int32_t* ttl);
/* Relay policy: the per-peer decision whether node_message forwards a first receipt
 * (README.md:20, node.py:106-116) -- silent peers (free riders, light clients, faulty nodes) and
 * probabilistic relay.  thr[v] = 0: peer v relays every first receipt; 0xFFFFFFFF: none; otherwise
 * its first receipt of message m in round r is muted iff
 *   philox4x32_10(ctr = (r, v, msg_id_base + m, 'RLY' = 0x00524C59), key = seed).x < thr[v]
 * (p2pg_relay_muted evaluates it on the host; `seed` is the policy's own, independent of the
 * gossip and churn seeds).  A muted first receipt behaves exactly like a receipt at its hop limit
 * (p2pg_set_ttl): it happens as usual -- seen bit, hop, parent, every receipt counter, the delivery
 * stream, the tallies -- and makes no sends: none in `relays`, the next round's `received`,
 * p2pg_get_sends, p2pg_peer_counters or the lost-send count.  Originations (round 0's, a start
 * round's, p2pg_originate's) are the app's own send_to_nodes and never muted; round 0 is never a
 * policy round.  With hop limits a receipt sends iff it is neither expired nor muted.
 * thr = NULL or all zero removes the policy: the engine then launches exactly what it launched
 * before.  V = the engine's peer count (P2PG_ERR_ARG otherwise).  p2pg_reset keeps and replays the
 * policy, p2pg_set_sources[_at] keep it (it belongs to the peers), p2pg_load_csr clears it.
 * P2PG_ERR_STATE on a vertex-partitioned rank, between p2pg_step_begin / p2pg_step_end and once a
 * round has run; while a policy is set p2pg_snapshot / p2pg_restore return P2PG_ERR_STATE.  A
 * rejected call changes nothing.
 * With a policy every round after round 0 is scheduled like an expiry round: the unfused
 * schedule, and its sends become final at the points named for p2pg_set_ttl (p2pg_message_cost among
 * them; read the round's deliveries first; p2pg_drop_relays of a muted receipt is legal and cancels nothing).  Its
 * scatter_words is 0, the following round's touched_words counts what the held-back push
 * touched, and push_form reports the form chosen for that push from the round's own density
 * (P2PG_PUSH_ATOMIC or P2PG_PUSH_EDGE; P2PG_PUSH_ATOMIC in a round that is an expiry round too). */
int p2pg_set_relay_policy(p2pg_engine* e, int64_t V, const uint32_t* thr, uint64_t seed);
/* Peer downtime: per-peer, deterministic churn -- offline windows, crashes and late joiners.
 * Each peer has one half-open interval of rounds [from[v], until[v]): from[v] = -1 never offline,
 * otherwise 0 <= from[v] < until[v]; until[v] = INT32_MAX never returns (a crash); from[v] = 0
 * joins late.  Peer v is offline in round r iff from[v] <= r < until[v] (p2pg_peer_offline).
 * An offline peer keeps its connections: its neighbours have no failure detector and go on
 * sending to it, and those sends are counted and lost like a send that churn drops (node.py:116
 * counts before sending).
 *  1. A send made in round r and addressed to u is lost iff it was lost before (churn, or a
 *     connection removed at the boundary) or u is offline in round r + 1.  Its sender still
 *     counts it (round r's relays, sent[v], p2pg_get_sends with lost = 1); it is no arrival
 *     (round r + 1's received, received[u]) and sets no seen bit at u.  u may still get the
 *     message later from another copy: an ordinary first receipt of that later round, with the
 *     later hop and that round's lowest-id sender as parent.
 *  2. An offline peer has no first receipts, so it sends nothing.  Its seen bits from before
 *     stand; a receipt it made in round from[v] - 1 sends normally in that round.
 *  3. Originations at an offline peer are refused, not dropped: P2PG_ERR_ARG from this call when
 *     a scheduled message (start >= 0) has its source offline in its start round, and from
 *     p2pg_set_sources, p2pg_set_sources_at and p2pg_originate when a downtime is set and an
 *     origination falls into its origin's interval.
 *  4. It composes with flood and gossip, churn, start rounds, hop limits, a relay policy,
 *     p2pg_update_edges, p2pg_drop_relays, the tallies, the delivery stream and the records: a
 *     receipt that did not happen is neither expired nor muted.  `active` keeps its rule: a run may
 *     end while peers are offline, and they do not catch up (unless p2pg_set_anti_entropy is set).
 *  5. Every receipt counter follows from the receipts that happened.  `received` is exact iff
 *     P2PG_FLAG_RECEIVED is set (as under churn); without it a round r with min(from) <= r <
 *     max(until) reports the sends of round r - 1 (an upper bound) and received_exact = 0.
 *     p2pg_peer_counters is exact either way.  scatter_words counts the masks pushed towards
 *     peers that are offline in the next round too (the push happens, the receiver discards it);
 *     touched_words, and push_form of a round in which somebody is offline, are the engine's.
 *  6. The downtime belongs to the peers: p2pg_reset and p2pg_set_sources[_at] keep it (subject
 *     to 3), p2pg_load_csr clears it.  from = NULL or all -1 removes it: the engine then launches
 *     exactly what it launched before.  V = the engine's peer count.  P2PG_ERR_ARG: another V,
 *     from[v] < -1, until[v] <= from[v] where from[v] >= 0.  P2PG_ERR_STATE: on a
 *     vertex-partitioned rank (and p2pg_set_global_ids once a downtime is set), between
 *     p2pg_step_begin / p2pg_step_end, once a round has run (allowed again after p2pg_reset), and
 *     p2pg_snapshot / p2pg_restore while one is set.  A rejected call changes nothing.
 * A round in which somebody is offline takes the unfused schedule (receive pass, the undo of the
 * offline peers' receipts, push); every other round is planned exactly as without the call. */
int p2pg_set_downtime(p2pg_engine* e, int64_t V, const int32_t* from, const int32_t* until);
/* Network partition: a netsplit window that heals.  Every peer has a side, side[v] >= 0, and there
 * is one window of rounds [cut_from, cut_until).  Connection {a, b} is cut in round t iff side[a] !=
 * side[b] and cut_from <= t < cut_until (p2pg_link_cut).  Peers keep their connections and have no
 * failure detector: they go on sending over a cut connection, gossip picks are unchanged and a pick
 * may be wasted on a cut connection.  On the reference harness this is one more term in
 * dropped(a, b): `or (side[a] != side[b] and cut_from <= round + 1 < cut_until)`.
 *  1. A send made in round r from v to u is lost iff it was lost before (churn, or a receiver that
 *     is offline in r + 1) or {v, u} is cut in round r + 1, the round it would arrive in.  Its sender
 *     still counts it (round r's relays, sent[v], p2pg_message_cost sent, p2pg_get_sends with lost =
 *     1); it is no arrival (round r + 1's received, received[u], p2pg_message_cost received) and
 *     sets no seen bit.  u may still get the message later from another copy: an ordinary first
 *     receipt of that later round, with that round's hop and that round's lowest-id sender whose
 *     copy arrived as parent.
 *  2. Originations are not sends: a message may start on any side in any round.
 *  3. Anti-entropy packets are sends: a request of round r is lost as well if {u, p} is cut in
 *     r + 1, a reply of round r + 1 if the connection is cut in r + 2 (requests_lost /
 *     replies_lost of p2pg_pull_stats).  A flood that saturated its side before the heal never
 *     crosses afterwards -- a peer sends only on a first receipt -- so only the pull repair carries
 *     its messages across.
 *  4. Every receipt counter follows from the receipts that happened.  `received` is exact iff
 *     P2PG_FLAG_RECEIVED is set; without it a round r with cut_from <= r < cut_until reports the
 *     sends of round r - 1 and received_exact = 0.  p2pg_peer_counters and p2pg_message_cost are
 *     exact either way.  A flood cut round receives by the cut pull (touched_words 0, push_form
 *     P2PG_PUSH_NONE as in every flood round).  A gossip round whose sends arrive in a cut round
 *     (cut_from - 1 <= r <= cut_until - 2) receives and pushes in separate passes with whole
 *     frontier rows and pushes by row atomics: push_form P2PG_PUSH_ATOMIC, scatter_words = its
 *     sends that were not lost to churn or the cut (one per (sender, message, pick), or per (sender,
 *     word, connection) for a sender with deg <= k: an upper bound of the distinct masks other
 *     rounds report), and the next round's touched_words counts what that push touched.
 *  5. It composes with flood and gossip, churn, start rounds and p2pg_originate, peer downtime,
 *     anti-entropy, the three tallies, the records, the delivery stream and p2pg_get_sends, under
 *     p2pg_step and p2pg_run (which batches no round at or before the last cut round).  p2pg_reset
 *     and p2pg_set_sources[_at] keep the setting, p2pg_load_csr clears it.  side = NULL, no
 *     connection between two sides (all sides equal), or cut_until <= cut_from (both >= 0) removes
 *     it: the engine then launches exactly what it launched before.
 *  6. P2PG_ERR_STATE, in either call order, a rejected call changing nothing: together with a
 *     finite hop limit, a relay policy, p2pg_drop_relays or p2pg_update_edges (their held-back pushes
 *     and rebuilt rows would each need the cut as well), p2pg_snapshot / p2pg_restore, on a
 *     vertex-partitioned rank (and p2pg_set_global_ids once a netsplit is set), between
 *     p2pg_step_begin / p2pg_step_end, and once a round has run (allowed again after p2pg_reset).
 *     P2PG_ERR_ARG: another V, a negative side, cut_from < 0 or cut_until < 0.
 * Rounds outside the window are planned exactly as without the call; the fused rounds come back
 * after the heal. */
int p2pg_set_netsplit(p2pg_engine* e, int64_t V, const int32_t* side, int32_t cut_from, int32_t cut_until);
/* Anti-entropy: periodic pull repair, the other half of epidemic broadcast.  An exchange happens in
 * every request round r with first <= r <= last and (r - first) % period == 0 and takes three
 * rounds (the reference app: a request queue on the dedup relay's Node, the harness's round being
 * arrivals, originations, replies, requests):
 *  1. Round r, after its arrivals and originations: every peer u that is online in r and has a
 *     connection sends one request to the connection in slot p2pg_pull_partner_slot(r, u, deg(u),
 *     seed) of its ascending list, carrying its seen set of that moment.  There is no failure
 *     detector: u may pick an offline neighbour.  The request is a send of round r: lost by the
 *     churn draw of (r, {u, p}) or because p is offline in r + 1.
 *  2. Round r + 1, at the partner p, after that round's arrivals and originations: one reply per
 *     request that arrived, listing every message p has seen by then that the digest lacks -- sent
 *     even if that list is empty, so replies = requests that arrived.  A send of round r + 1: lost
 *     by the churn draw of (r + 1, {p, u}) or because u is offline in r + 2.
 *  3. Round r + 2, at u: the reply is one more arriving packet from sender p, processed in
 *     ascending sender order after p's relay packets.  Every listed message u has not seen is an
 *     ordinary first receipt of round r + 2: hop r + 2, parent = the lowest-id sender whose copy
 *     arrived (min of the lowest relay sender and p), relayed like any other (flood: every
 *     connection but that sender; gossip: its k picks of round r + 2).  What p itself receives in
 *     round r + 2 is not visible to u in that round.
 *  4. relays, received, the per-peer counters and p2pg_get_sends stay what they are -- relay
 *     packets only, those of pulled first receipts included.  Pull packets are recorded per
 *     exchange (p2pg_get_pull_stats).  new_deliveries and the other receipt counters of round r + 2
 *     include the pulled receipts.
 *  5. `active` (and so p2pg_run) stays 1 while a request round lies at or ahead or an exchange is
 *     in flight, besides packets and starts ahead; `last` is mandatory, so a run ends.
 *  6. It composes with flood and gossip, churn, start rounds, p2pg_originate, peer downtime, the
 *     tallies, the records, the delivery stream and p2pg_get_sends.  The setting belongs to the
 *     peers: p2pg_reset and p2pg_set_sources[_at] keep it, p2pg_load_csr clears it.  period = 0
 *     removes it (first, last and seed are then ignored): the engine launches exactly what it
 *     launched before.
 * P2PG_ERR_ARG: first < 0, last < first, period < 0.  P2PG_ERR_STATE: once a round has run (allowed
 * again after p2pg_reset), between p2pg_step_begin / p2pg_step_end, and on a vertex-partitioned
 * rank (p2pg_set_global_ids while it is set likewise).  While it is set, p2pg_snapshot /
 * p2pg_restore, p2pg_update_edges and p2pg_drop_relays return P2PG_ERR_STATE.  Not together with a
 * finite hop limit, in either call order (P2PG_ERR_STATE from the second call): under the
 * reference's ttl - 1 app a pulled message carries the budget its holder had left, which is not a
 * function of the round, so the engine's round-based expiry would be wrong.  Not together with a
 * relay policy either (P2PG_ERR_STATE, either order): whether a muted peer answers requests is a
 * policy question of its own and out of scope here.  A rejected call changes nothing.
 * Only the arrival rounds r + 2 launch anything (two passes around the receive pass, unfused
 * schedule); request and reply rounds are planned exactly as without the call.              */
int p2pg_set_anti_entropy(p2pg_engine* e, int32_t first, int32_t last, int32_t period, uint64_t seed);
/* The records of the exchanges completed in this run (since p2pg_reset / the sources), in order of
 * request round: up to cap of them into out, *n_out = their number.                            */
int p2pg_get_pull_stats(p2pg_engine* e, int64_t cap, p2pg_pull_stats* out, int64_t* n_out);
/* Back to round 0 with the same graph, sources and start rounds (clears seen/frontier state). */
int p2pg_reset(p2pg_engine* e);
/* One round. Returns 1 while messages are in flight, 0 when quiescent, < 0 on error. */
int p2pg_step(p2pg_engine* e, p2pg_round_stats* out);
/* Rounds until quiescence or max_rounds; per_round may be NULL (else >= max_rounds slots).
 * Inside a call, fused dense gossip rounds other than the last two it may run do not store
 * their frontier rows (no later round reads them), so the delivery stream is available for
 * the last round a call ran, as after p2pg_step.                                          */
int p2pg_run(p2pg_engine* e, int32_t max_rounds, p2pg_round_stats* per_round,
             int32_t* n_rounds);
/* The first receipts of the most recent round, sorted by (peer, msg); parent = -1 at the
 * source.  Writes min(cap, count) records; *n_out = count (may exceed cap).
 * A round without first receipts has none (*n_out = 0).  P2PG_ERR_STATE if that round's
 * (or, for the parents, the previous round's) frontier was not kept -- not reachable through
 * p2pg_step / p2pg_run as specified above -- and for the round a snapshot was restored at
 * (p2pg_restore: the snapshot holds that round's frontier, not the one before it; the rounds
 * the restored engine runs report their deliveries as usual).                              */
int p2pg_get_new_deliveries(p2pg_engine* e, int64_t cap, int32_t* peer, int32_t* msg,
                            int32_t* hop, int32_t* parent, int64_t* n_out);
/* Every send of the most recent round -- the send_to_node calls its first receipts made
 * (node.py:114-120): flood, each connection but the one the receipt came from (all of them at
 * the origin, node.py:106-112); gossip, the k Philox picks -- as (sender, receiver, msg) records
 * sorted by (receiver, sender, msg), lost[i] = 1 if the send never arrives (churn drops it,
 * nodeconnection.py:123-126).  These are exactly the packets the next round's receivers hand to
 * node_message (nodeconnection.py:211-216), duplicates included; a p2pg_update_edges after this
 * call loses the ones on removed connections as well.  Reflects p2pg_drop_relays.  Writes
 * min(cap, count) records, *n_out = count.  P2PG_ERR_STATE after a p2pg_update_edges at this
 * round boundary or when the frontier (flood: and the one before it) was not kept.          */
int p2pg_get_sends(p2pg_engine* e, int64_t cap, int32_t* sender, int32_t* receiver, int32_t* msg,
                   uint8_t* lost, int64_t* n_out);
/* The app did not relay these first receipts of the most recent round (its node_message made no
 * send_to_nodes / send_to_node call for them, README.md:20): withdraw their sends before the
 * next round -- flood, their frontier bits; gossip, the round's pushes are redone without them.
 * Relay counters and the next round's `received` drop accordingly.  Each (peer[i], msg[i]) must
 * be a first receipt of that round, listed once (P2PG_ERR_ARG otherwise, nothing changed).
 * Read the round's deliveries first (they are its frontier bits).  Not on a vertex-partitioned
 * rank, not after a p2pg_update_edges at this boundary.                                      */
int p2pg_drop_relays(p2pg_engine* e, int64_t n, const int32_t* peer, const int32_t* msg);
/* Validation copies: seen [V][W] uint64 (W = ceil(M/64)); hop/parent [V][M] int32 need
 * P2PG_FLAG_RECORD (-1 = not delivered).  Any pointer may be NULL.                      */
int p2pg_read_planes(p2pg_engine* e, uint64_t* seen, int32_t* hop, int32_t* parent);
/* Word w of every peer's seen row (messages 64w .. 64w+63): out[V].  Full-size validation
 * without copying a whole plane (config 5: 51 GB at 100M peers x 4096 broadcasts).       */
int p2pg_read_seen_word(p2pg_engine* e, int32_t w, uint64_t* out);
/* ---- run tallies: what a p2pnetwork user reads off a finished run, computed on the device ----
 * Per broadcast, the size of every peer's dedup "seen" set membership (README.md:20); per peer,
 * the reference's only counters, Node.message_count_send / message_count_recv (node.py:65-67).
 * All three: P2PG_ERR_STATE before p2pg_set_sources and between p2pg_step_begin / p2pg_step_end.
 *
 * Peers that hold message m now (column popcount of the seen plane), reach[M].  No flag
 * needed, no cost to the rounds; valid between rounds on any engine with sources set,
 * including after a p2pg_run that skipped frontier rows.  Not on a vertex-partitioned rank. */
int p2pg_message_reach(p2pg_engine* e, uint64_t* reach);
/* With P2PG_FLAG_TALLY, accumulated round by round from each round's first receipts -- the
 * node_message events that pass dedup (node.py:334-338) -- (any pointer may be NULL):
 *   reach[m]    first receipts of m so far, origin included (== p2pg_message_reach)
 *   hop_sum[m]  sum over those receipts of their hop (round index); mean hop = hop_sum/reach
 *   last_hop[m] round of m's latest first receipt (-1 before round 0 ran)
 * Counted when the receipts happen: a later p2pg_drop_relays withdraws relays, not receipts. */
int p2pg_message_tally(p2pg_engine* e, uint64_t* reach, uint64_t* hop_sum, int32_t* last_hop);
/* With P2PG_FLAG_TALLY: sent[V], received[V] (either may be NULL).
 *   sent[v]     send_to_node calls peer v made in the rounds run so far, lost ones included
 *               (node.py:116 counts before sending), less relays withdrawn by
 *               p2pg_drop_relays: Node.message_count_send.
 *   received[v] those sends, from any peer, that are addressed to v and are not lost to
 *               churn or to a connection p2pg_update_edges removed while they were in
 *               flight: v's message_count_recv (nodeconnection.py:215) once the next round
 *               has handed them over.  Exact under churn with or without P2PG_FLAG_RECEIVED.
 * A round's sends are counted once they are final: when the next round starts, inside
 * p2pg_update_edges, or by this call -- after which a p2pg_drop_relays or p2pg_update_edges at
 * the same round boundary is refused (P2PG_ERR_STATE): read the counters after the changes of
 * a boundary.  p2pg_reset and p2pg_set_sources zero all tallies. */
int p2pg_peer_counters(p2pg_engine* e, uint64_t* sent, uint64_t* received);
/* With P2PG_FLAG_MSG_COST: what each broadcast cost, sent[M], received[M] (either may be NULL).
 *   sent[m]     send_to_node calls that carried message m in the rounds run so far -- its first
 *               receipts' relays and its originations -- lost ones included (node.py:116 counts
 *               before sending), less relays withdrawn by p2pg_drop_relays.
 *   received[m] those of them that are not lost: to churn, to a connection p2pg_update_edges
 *               removed while the packet was in flight, or to a receiver that is offline in the
 *               arrival round (nodeconnection.py:215 per payload id).
 * These are the records of p2pg_get_sends binned by msg.  Pull packets of anti-entropy are not
 * counted; the relays of pulled first receipts are.  On every run sum_m sent[m] = the sum of
 * round_stats.relays, and with P2PG_FLAG_TALLY as well sum_m sent[m] = sum_v of
 * p2pg_peer_counters' sent[v], likewise received.  sent[m] / (reach[m] - 1) - 1 is the relative
 * message redundancy of broadcast m.
 * The lifecycle is that of p2pg_peer_counters: a round's sends are counted once they are final --
 * when the next round starts, inside p2pg_update_edges, or by this call, which first makes a
 * held-back expiry / policy round final as p2pg_peer_counters does -- after which a
 * p2pg_drop_relays or p2pg_update_edges at the same round boundary is refused (P2PG_ERR_STATE):
 * read the counters after the changes of a boundary.  p2pg_reset and p2pg_set_sources[_at] zero
 * the counters.  P2PG_ERR_STATE without the flag, before sources are set, between
 * p2pg_step_begin and p2pg_step_end, and on a vertex-partitioned rank.                       */
int p2pg_message_cost(p2pg_engine* e, uint64_t* sent, uint64_t* received);
/* ---- delivery latency (P2PG_FLAG_LATENCY): how long delivery took, computed on the device ----
 * The relative hop of a first receipt of message m in round r -- a node_message event that passes
 * the app's dedup (node.py:334-338, README.md:20) -- is h = r - start[m]; the origination is the
 * receipt with h = 0 at the origin and is counted, as in reach.  A receipt is counted at the end
 * of the round in which it happens, from the round's final frontier: an offline peer's undone
 * receipt is not counted, a receipt an anti-entropy reply made is counted with the hop of its
 * arrival round, an expired or muted receipt is counted (it happened), and a later
 * p2pg_drop_relays or p2pg_update_edges changes nothing (they withdraw relays, not receipts).
 * Reading needs no final sends and refuses nothing afterwards.
 * All three: P2PG_ERR_STATE without the flag, before p2pg_set_sources, between p2pg_step_begin /
 * p2pg_step_end and on a vertex-partitioned rank.  p2pg_reset and p2pg_set_sources[_at] zero the
 * counters and keep the number of bins.
 *
 * The histograms' number of bins, 2..1024 (P2PG_ERR_ARG outside; default 64): the last bin
 * collects every hop >= bins - 1.  P2PG_ERR_STATE once a round has run (allowed again after
 * p2pg_reset).                                                                                 */
int p2pg_set_latency_bins(p2pg_engine* e, int32_t bins);
/* hist[M][bins], row-major: hist[m][b] = the first receipts of m so far with min(h, bins - 1) == b;
 * sum_b hist[m][b] == p2pg_message_reach[m].  bins must be the engine's (P2PG_ERR_ARG).       */
int p2pg_message_latency(p2pg_engine* e, int32_t bins, uint64_t* hist);
/* Per peer, exact and independent of bins ([V]; any pointer may be NULL):
 *   hop_sum[v]   sum of h over v's first receipts so far
 *   receipts[v]  their number; sum_v receipts[v] == sum_m reach[m]
 *   max_hop[v]   the largest h, -1 with no receipt                                          */
int p2pg_peer_latency(p2pg_engine* e, uint64_t* hop_sum, uint32_t* receipts, int32_t* max_hop);
/* Summed device time per kernel class since the last reset (needs P2PG_FLAG_TIMING):
 * 0 seed (origination, in round 0 and later; the hop-limit passes of expiry rounds; the relay-policy
 * and downtime passes; the two anti-entropy passes of arrival rounds, k_pull_gather and
 * k_pull_apply -- an anti-entropy run's repair time shows up in this class), 1 flood pull, 2 gossip scatter by row atomics (sparse rounds),
 * 3 record (validation), 4 gossip update (consume row atomics), 5 gossip pull (consume edge
 * stores), 6 gossip scatter by edge stores (dense rounds), 7 gossip fused pull + scatter
 * (a dense round after a dense round).                                                  */
#define P2PG_KCLASS_N 8
int p2pg_kernel_times(p2pg_engine* e, double ms[P2PG_KCLASS_N], int64_t launches[P2PG_KCLASS_N]);
/* With P2PG_FLAG_TIMING: only launches of the classes in mask (bit i = class i; default all)
 * are bracketed by HIP events -- two event records per launch cost ~2.7 us of stream time each
 * (0.8 ms per config-4 broadcast), so a measurement can time its dominant kernel alone.
 * (Instrumentation; the reference has none -- its only counters are node.py:65-67.)       */
int p2pg_set_timed_classes(p2pg_engine* e, uint32_t mask);
/* ---- vertex-partitioned runs (one engine per GPU) ---------------------
 * The caller loads the rank's LOCAL graph: owned peers plus ghost peers (remote neighbours),
 * all numbered in ascending GLOBAL id order (so lowest-id tie-breaks are unchanged); ghosts
 * have empty rows.  gid[local] = global id (Philox keys, reported ids).  send_local = owned
 * boundary peers in the order the peers' ghost blocks expect them; recv_local = ghost peers
 * in the order the owners send them.  After each p2pg_step the caller moves rows between
 * ranks (e.g. RCCL all-to-all): plane 0 = frontier rows (pack from send_local, unpack into
 * recv_local, before the next flood step); plane 1 = gossip pushes addressed to ghosts (pack
 * from recv_local -- cleared locally --, unpack ORed into send_local).  Buffers are device
 * memory of n x W uint64 words.  Replaces the cross-host TCP fan-out of
 * NodeConnection.send (nodeconnection.py:107-160).                                      */
int p2pg_set_global_ids(p2pg_engine* e, const int32_t* gid);
/* Partitioned gossip, for hop / parent records and the delivery stream: a first receipt's
 * parent is the lowest-id neighbour whose Philox picks chose the receiver (node.py:334-338's
 * sender), and a GHOST neighbour's picks depend on its global degree and the
 * receiver's place in its global adjacency, which the rank-local graph does not hold:
 * ghost_deg[local] = global degree of each ghost (any value for owned peers), slot_pos[j] for
 * every local slot j = position of the slot's row owner in the neighbour's global ascending
 * adjacency when the neighbour is a ghost, else -1.  The ghosts' frontier rows must then also
 * travel each round (plane 0).  NULL, NULL removes them.                                   */
int p2pg_set_ghost_senders(p2pg_engine* e, const int32_t* ghost_deg, const int32_t* slot_pos);
int p2pg_set_exchange(p2pg_engine* e, int64_t n_send, const int32_t* send_local, int64_t n_recv,
                      const int32_t* recv_local);
int p2pg_exchange_pack(p2pg_engine* e, int32_t plane, void* dev_buf);
int p2pg_exchange_unpack(p2pg_engine* e, int32_t plane, const void* dev_buf);
/* Compacted exchange: only rows that carry something travel (plane 0: boundary peers with first
 * receipts this round; plane 1: ghosts that were pushed to), as records of 1 + W int64: the row's
 * index within the destination's list segment, then its W words.  The lists are cut into one
 * segment per rank (p2pg_set_exchange_segments: send / recv rows per rank, summing to the
 * set_exchange lists).  pack_live writes segment q's records from record send_off[q] of dev_buf
 * (capacity: the list length x (1 + W) int64) and returns the record count per destination in
 * counts[nseg] (host); unpack_live takes the records of all sources packed in source order and
 * their counts, and is asynchronous on the engine's stream.                               */
int p2pg_set_exchange_segments(p2pg_engine* e, int32_t nseg, const int64_t* send_counts,
                               const int64_t* recv_counts);
int p2pg_exchange_pack_live(p2pg_engine* e, int32_t plane, void* dev_buf, int64_t* counts);
/* Pack inside the round: from now on every p2pg_step / p2pg_step_end packs the live rows of
 * `plane` into dev_buf (same layout and capacity as pack_live) right after the round's kernels,
 * and the record counts come back together with the round counters -- one host
 * synchronisation per round instead of a second drain of the stream for the pack.  A following
 * p2pg_exchange_pack_live(e, plane, dev_buf, counts) then only returns those counts.  NULL turns
 * it off.  (Replaces, like pack_live, the cross-host fan-out of NodeConnection.send,
 * nodeconnection.py:107-160.)                                                              */
int p2pg_set_exchange_buffer(p2pg_engine* e, int32_t plane, void* dev_buf);
int p2pg_exchange_unpack_live(p2pg_engine* e, int32_t plane, const void* dev_buf, const int64_t* counts);
/* A round in two calls, so a vertex-partitioned rank overlaps the exchange of the last round's
 * rows with work: step_begin launches the pull / update of the peers with no ghost neighbour
 * (they need none of the exchanged rows) and returns at once; step_end runs the rest of the
 * round once the rows are unpacked (= p2pg_step).  p2pg_step alone does both.  Between the
 * two, snapshot / restore / update_edges / set_exchange / exchange packing are refused
 * (P2PG_ERR_STATE): the round is half done.                                                */
int p2pg_step_begin(p2pg_engine* e);
int p2pg_step_end(p2pg_engine* e, p2pg_round_stats* out);
/* ---- dynamic topology --------------------------------------------
 * Connection changes between rounds: n_add pairs to connect (Node.connect_with_node,
 * node.py:122-176) and n_del pairs to disconnect (Node.disconnect_with_node, node.py:178-189,
 * then node_disconnected on both ends, node.py:307-319), as 2*n peer ids (a0, b0, a1, b1..).
 * Connecting an existing pair, disconnecting a missing one, self connections and pairs listed
 * twice are errors (P2PG_ERR_ARG; the reference refuses them with a debug print).  Messages
 * sent in the last round and still in flight on a removed connection are lost (a stopped
 * NodeConnection drops its unread buffer, nodeconnection.py:192-228); the others arrive next
 * round; every send from the next round on uses the new connections.  One update per round
 * boundary; not on a vertex-partitioned rank.                                              */
int p2pg_update_edges(p2pg_engine* e, int64_t n_add, const int32_t* add, int64_t n_del,
                      const int32_t* del);
/* ---- snapshot / resume (the reference has no checkpointing) --------
 * Between rounds, the run state (round, seen sets, saturation, the last round's first
 * receipts, messages in flight, hop/parent planes in record mode) is written to a caller
 * buffer of p2pg_snapshot_size bytes, and read back by p2pg_restore into an engine with the
 * same configuration, graph and sources (checked: P2PG_ERR_STATE otherwise), which then
 * continues bit-identically.  Not between a topology update and the next round.           */
int p2pg_snapshot_size(p2pg_engine* e, int64_t* bytes);
int p2pg_snapshot(p2pg_engine* e, void* buf, int64_t cap);
int p2pg_restore(p2pg_engine* e, const void* buf, int64_t size);
/* Launch on this hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL =
 * the engine's own stream.                                                              */
int p2pg_set_stream(p2pg_engine* e, void* hip_stream);
/* Device-side Philox KAT: evaluates philox4x32_10 on n counters with one key.          */
int p2pg_device_philox(p2pg_engine* e, int32_t n, const uint32_t* ctr, const uint32_t key[2],
                       uint32_t* out);
const char* p2pg_last_error(const p2pg_engine* e);
const char* p2pg_global_error(void);
void p2pg_destroy(p2pg_engine* e);

#ifdef __cplusplus
}
#endif
#endif /* P2PGPU_H */
