"""GraphNetwork: a whole population of relaying p2pnetwork peers on one MI355X.

What an application builds on p2pnetwork for a broadcast is (pj8912/python-p2p-network):

    class MyNode(Node):                                   # p2pnetwork/node.py:13
        def node_message(self, node, data):               # node.py:334-338
            if data["id"] in self.seen: return            # dedup, README.md:20
            self.seen.add(data["id"])
            self.send_to_nodes(data, exclude=[node])      # node.py:106-112 -> send_to_node
                                                          #   (message_count_send += 1, :116)

GraphNetwork runs that relay for every peer of a ``PeerGraph`` at once, for up to thousands of
concurrent broadcasts (64 per uint64 word), round-synchronously, through the HIP engine behind
the C-ABI of include/p2pgpu.h.  The hook surface is kept in batched form: per round,
``node_message_batch(deliveries)`` receives the first receipts of that round as arrays
(peer, msg, hop, parent) -- the node_message events that pass dedup -- and a
``callback(event, network, connected_node, data)`` with the reference signature
(node.py:25-29) is invoked with event "node_message_batch".  Per-callback replay for Node
subclasses is in ``p2pnetwork.gpu.compat``.
"""
import ctypes
from collections import namedtuple
from dataclasses import dataclass

import numpy as np

from . import _lib
from .graph import PeerGraph

# p2pg_round_stats.push_form (include/p2pgpu.h P2PG_PUSH_*)
PUSH_FORMS = ("none", "atomic", "edge", "fused", "update_edge")

STAT_FIELDS = ("round", "active", "new_deliveries", "relays", "active_vertices", "active_words",
               "wedges", "deg_active", "scatter_words", "touched_words", "received")


@dataclass(slots=True)
class RoundStats:
    round: int
    active: int
    new_deliveries: int
    relays: int
    active_vertices: int
    active_words: int
    wedges: int
    deg_active: int
    scatter_words: int
    touched_words: int
    received: int = 0   # packets that arrived this round (sum of message_count_recv += 1,
                        # nodeconnection.py:215): last round's sends less the lost ones
    push_form: int = 0  # gossip: how this round's pushes left (PUSH_FORMS); not a result
    received_exact: int = 1  # 0: a churn run without count_received -- `received` is then the
                             # sends of the round before (an upper bound)

    @classmethod
    def from_c(cls, s):
        return cls(*(int(getattr(s, f)) for f in STAT_FIELDS), push_form=int(s.push_form),
                   received_exact=int(s.received_exact))

    @classmethod
    def from_c_array(cls, buf, n):
        """The first n entries of a RoundStatsC array (one numpy view instead of 11 ctypes field
        reads per round: p2pg_run's results are converted while the GPU waits for the next call)."""
        if n <= 0:
            return []
        rows = np.frombuffer(buf, dtype=_ROUND_DTYPE, count=n)[_ROUND_COLS].tolist()
        return [cls(*r) for r in rows]

    def as_dict(self):
        return {f: getattr(self, f) for f in STAT_FIELDS}


@dataclass
class Sends:
    """Every send of one round (Node.send_to_node calls, node.py:114-120), sorted by (receiver,
    sender, msg); lost = churn dropped it (nodeconnection.py:123-126).  The ones not lost are the
    next round's arrivals, each a node_message call (nodeconnection.py:211-216)."""
    sender: np.ndarray
    receiver: np.ndarray
    msg: np.ndarray
    lost: np.ndarray

    def __len__(self):
        return len(self.sender)


@dataclass
class Deliveries:
    """First receipts of one round, sorted by (peer, msg); parent = -1 at the origin."""
    peer: np.ndarray
    msg: np.ndarray
    hop: np.ndarray
    parent: np.ndarray

    def __len__(self):
        return len(self.peer)


# Run tallies (GraphNetwork(tally=True)): per broadcast, uint64 [M] reach (peers that received
# it, origin included) and hop_sum (sum of their hops; mean hop = hop_sum / reach), int32 [M]
# last_hop (round of the latest first receipt, -1 = none yet) -- p2pg_message_tally
MessageTally = namedtuple("MessageTally", "reach hop_sum last_hop")
# ... and per peer, uint64 [V]: Node.message_count_send (node.py:65, :116) and
# message_count_recv (nodeconnection.py:215) -- p2pg_peer_counters
PeerCounters = namedtuple("PeerCounters", "sent received")
# Per-broadcast cost (GraphNetwork(cost=True)), uint64 [M]: the send_to_node calls that carried
# each broadcast (node.py:116) and those of them that arrived (nodeconnection.py:215) --
# p2pg_message_cost
MessageCost = namedtuple("MessageCost", "sent received")


class PeerLatency(namedtuple("PeerLatency", "hop_sum receipts max_hop")):
    """Delivery latency per peer (GraphNetwork(latency=True)), [V]: uint64 hop_sum (sum over the
    peer's first receipts of their relative hop, round - start round of the broadcast), uint32
    receipts (their number), int32 max_hop (the largest, -1 = no receipt) -- p2pg_peer_latency"""
    __slots__ = ()

    def mean(self):
        """float64 [V]: hop_sum / receipts, NaN for a peer without a receipt."""
        out = np.full(len(self.receipts), np.nan)
        ok = self.receipts > 0
        out[ok] = self.hop_sum[ok].astype(np.float64) / self.receipts[ok].astype(np.float64)
        return out

# index of SnapHeader.total_relays in the snapshot header viewed as uint64 words (engine.cpp:
# magic 0, version/mode 1, V 2, nnz 3, M/W 4, fanout/round 5, flags/thr 6, base/done 7,
# consume/has_next 8, gossip_seed 9, churn_seed 10, graph_hash 11, src_hash 12, total_relays 13)
_SNAP_TOTAL_RELAYS_WORD = 13

# p2pg_set_downtime: until = INT32_MAX, a peer that never returns
_FOREVER = 0x7FFFFFFF

# one anti-entropy exchange (p2pg_pull_stats)
PULL_STATS_DTYPE = np.dtype([("request_round", np.int32), ("reserved", np.int32), ("requests", np.uint64),
                             ("requests_lost", np.uint64), ("replies", np.uint64), ("replies_lost", np.uint64),
                             ("repaired", np.uint64)])


def churn_threshold(p_drop):
    """floor(p_drop * 2^32), the integer threshold of the per-round edge-drop mask."""
    if not 0.0 <= p_drop < 1.0:
        raise ValueError("churn probability must be in [0, 1)")
    return int(np.floor(p_drop * 4294967296.0))


_ROUND_DTYPE = np.dtype([(n, {ctypes.c_int32: "<i4", ctypes.c_uint64: "<u8"}[t])
                         for n, t in _lib.RoundStatsC._fields_])
assert _ROUND_DTYPE.itemsize == ctypes.sizeof(_lib.RoundStatsC)
_ROUND_COLS = list(STAT_FIELDS) + ["push_form", "received_exact"]


class GraphNetwork:
    """A peer graph resident in HBM plus the relay engine that floods/gossips over it."""

    def __init__(self, graph, mode="flood", fanout=3, gossip_seed=0x5EED, churn=0.0,
                 churn_threshold_value=None, churn_seed=0xC0FFEE, record=False, timing=False,
                 device=0, msg_id_base=0, callback=None, autostop=True, local_graph=False,
                 count_received=False, tally=False, cost=False, latency=False, latency_bins=64):
        if not isinstance(graph, PeerGraph):
            raise TypeError("graph must be a PeerGraph")
        if mode not in ("flood", "gossip"):
            raise ValueError("mode must be 'flood' or 'gossip'")
        self.graph = graph
        self.mode = mode
        self.fanout = int(fanout)
        self.record = bool(record)
        self.callback = callback
        self.latency = bool(latency)
        self.latency_bins = int(latency_bins)
        if self.latency and not 2 <= self.latency_bins <= 1024:
            raise ValueError("latency_bins must lie in [2, 1024]")
        self._engine_bins = 64       # the engine's number of histogram bins (its default)
        cfg = _lib.Config()
        cfg.mode = _lib.MODE_FLOOD if mode == "flood" else _lib.MODE_GOSSIP
        cfg.fanout = self.fanout
        cfg.gossip_seed = int(gossip_seed)
        cfg.churn_seed = int(churn_seed)
        cfg.churn_threshold = int(churn_threshold_value if churn_threshold_value is not None
                                  else churn_threshold(churn))
        cfg.msg_id_base = int(msg_id_base)
        cfg.flags = ((_lib.FLAG_RECORD if record else 0) | (_lib.FLAG_TIMING if timing else 0)
                     | (0 if autostop else _lib.FLAG_NO_AUTOSTOP)
                     | (_lib.FLAG_LOCAL_GRAPH if local_graph else 0)
                     | (_lib.FLAG_RECEIVED if count_received else 0)
                     | (_lib.FLAG_TALLY if tally else 0)
                     | (_lib.FLAG_MSG_COST if cost else 0)
                     | (_lib.FLAG_LATENCY if latency else 0))
        cfg.device = int(device)
        self.config = cfg
        L = _lib.lib()
        h = ctypes.c_void_p()
        _lib.check(L.p2pg_create(ctypes.byref(cfg), ctypes.byref(h)))
        self._h = h
        self._check(L.p2pg_load_csr(h, graph.V, _lib.ptr(graph.rowptr), _lib.ptr(graph.colidx)))
        self.sources = None
        self.start_rounds = None     # int32 [M]: the round each broadcast originates in (-1 = unscheduled)
        self.ttl = None              # int32 [M]: each broadcast's hop limit (-1 = unlimited)
        self.relay_thr = None        # uint32 [V]: the relay policy's mute thresholds (None = no policy)
        self.relay_seed = 0
        self.offline_from = None     # int32 [V]: the peers' downtime intervals [from, until)
        self.offline_until = None    # (None = no downtime; until 0x7FFFFFFF = forever)
        self.anti_entropy = None     # (period, first_round, last_round, seed), None = not set
        self.netsplit = None         # (side int32 [V], cut_from, cut_until), None = not set
        self._autostop = bool(autostop)
        self._next_round = 0         # the next round the engine runs
        self._quiet = False          # the engine went quiet (further steps run no round)
        self.rounds = []
        self.message_count_send = 0  # sum of Node.message_count_send (node.py:65, :116)
        self._run_buf = None

    # -- plumbing -------------------------------------------------------------------------
    def _check(self, rc):
        return _lib.check(rc, self._h)

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().p2pg_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def M(self):
        return 0 if self.sources is None else len(self.sources)

    @property
    def W(self):
        return (self.M + 63) // 64

    def set_stream(self, hip_stream):
        """Launch on an external hipStream_t handle (int), e.g. torch's current stream."""
        self._check(_lib.lib().p2pg_set_stream(self._h, ctypes.c_void_p(hip_stream or None)))

    # -- broadcasts -----------------------------------------------------------------------
    def broadcast(self, sources, start_rounds=None, ttl=None):
        """Originate one broadcast per entry (origin peer ids); message m = position m.
        Equivalent of calling Node.send_to_nodes(data) at each origin (node.py:106).

        ``ttl[m]`` is message m's hop limit (default: none), see ``set_ttl``.

        ``start_rounds[m]`` is the round message m originates in (default: all in round 0): in
        that round, after its arrivals, the origin makes a first receipt (hop = the round,
        parent -1) and sends to all its connections (flood) or its ``fanout`` picks (gossip).
        -1 in both arrays declares an unscheduled message, to be started by ``originate``.
        ``run`` crosses the idle rounds before a scheduled start; hops stay absolute round
        indices (``hop_parent(relative=True)`` subtracts the start rounds)."""
        src = np.array(sources, dtype=np.int32, ndmin=1)
        if src.ndim != 1 or len(src) == 0:
            raise ValueError("sources must be a non-empty 1-D array of peer ids")
        if start_rounds is None:
            self._check(_lib.lib().p2pg_set_sources(self._h, len(src), _lib.ptr(src)))
            start = np.zeros(len(src), dtype=np.int32)
        else:
            start = np.array(start_rounds, dtype=np.int32, ndmin=1)
            if start.shape != src.shape:
                raise ValueError("start_rounds must have one entry per source")
            self._check(_lib.lib().p2pg_set_sources_at(self._h, len(src), _lib.ptr(src), _lib.ptr(start)))
        self.sources = src
        self.start_rounds = start
        if self.latency and self.latency_bins != self._engine_bins:  # (the engine keeps it from here on)
            self.set_latency_bins(self.latency_bins)
        self.ttl = np.full(len(src), -1, dtype=np.int32)  # (new sources carry no hop limits)
        self.rounds = []
        self.message_count_send = 0
        self._next_round, self._quiet = 0, False
        if ttl is not None:
            self.set_ttl(ttl)

    def set_ttl(self, ttl):
        """Hop limits, before round 0 runs (or after ``reset``): ``ttl[m] >= 0`` bounds broadcast
        m, -1 leaves it unlimited; ``None`` removes them all.  A first receipt of m at relative hop
        ``h = round - start_rounds[m]`` (the origination has h = 0) is recorded as always and
        relays iff ``ttl[m] < 0 or h < ttl[m]`` -- the app that forwards ``ttl - 1`` while
        ``ttl > 0`` (README.md:20); ``ttl = 0`` marks the message seen at its origin and sends
        nothing.  ``reset`` keeps the limits, ``broadcast`` clears them (p2pg_set_ttl).  Read an
        expiry round's ``deliveries()`` before its ``sends()`` / ``peer_counters()`` /
        ``update_edges()`` / ``drop_relays()``."""
        if self.sources is None:
            raise RuntimeError("set_ttl: call broadcast(sources) first")
        if ttl is None:
            t = np.full(self.M, -1, dtype=np.int32)
        else:
            t = np.array(ttl, dtype=np.int64, ndmin=1)
            if t.ndim != 1 or ((t < -(1 << 31)) | (t >= (1 << 31))).any():
                raise ValueError("ttl must be a 1-D array of int32 hop limits")
            t = np.ascontiguousarray(t, dtype=np.int32)
        self._check(_lib.lib().p2pg_set_ttl(self._h, len(t), _lib.ptr(t) if ttl is not None else None))
        self.ttl = t

    @staticmethod
    def relay_thresholds(relay_prob, V):
        """uint32 [V] mute thresholds of relay probabilities q in [0, 1] (scalar or [V]):
        1 -> 0 (relays all, no draw), 0 -> 0xFFFFFFFF (relays none, no draw), otherwise
        floor((1 - q) * 2^32) clipped to [1, 0xFFFFFFFE]."""
        q = np.asarray(relay_prob, dtype=np.float64)
        if q.ndim > 1 or (q.ndim == 1 and len(q) != V):
            raise ValueError("relay_prob must be a scalar or one probability per peer")
        q = np.broadcast_to(q, (V,))
        if not ((q >= 0.0) & (q <= 1.0)).all():
            raise ValueError("relay probabilities must lie in [0, 1]")
        t = np.clip(np.floor((1.0 - q) * 4294967296.0), 1.0, float(0xFFFFFFFE))
        t = np.where(q == 1.0, 0.0, np.where(q == 0.0, float(0xFFFFFFFF), t))
        return np.ascontiguousarray(t, dtype=np.uint32)

    @staticmethod
    def relay_muted(round, peer, msg, threshold, seed=0):
        """Does the relay policy mute the first receipt of message ``msg`` (global id) at ``peer``
        in ``round`` under the peer's ``threshold``?  (p2pg_relay_muted; originations are exempt,
        which is the caller's to apply.)"""
        return bool(_lib.lib().p2pg_relay_muted(int(round), int(peer), int(msg), int(threshold), int(seed)))

    def set_relay_policy(self, relay_prob=None, *, thresholds=None, seed=0):
        """Per-peer relay policy, before round 0 runs (or after ``reset``): peer v forwards a first
        receipt with probability ``relay_prob[v]`` (scalar or [V]; 0 = a silent peer that receives
        and never forwards, 1 = always).  A muted receipt is recorded as always and sends nothing,
        like a receipt at its hop limit; originations are never muted.  ``thresholds`` gives the
        uint32 [V] thresholds directly (see ``relay_thresholds``); ``seed`` is the policy's own
        Philox key.  ``None`` (or probability 1 everywhere) removes the policy.  ``reset`` and
        ``broadcast`` keep it (p2pg_set_relay_policy).  Read a round's ``deliveries()`` before its
        ``sends()`` / ``peer_counters()`` / ``update_edges()`` / ``drop_relays()``."""
        V = self.graph.V
        if relay_prob is not None and thresholds is not None:
            raise ValueError("give relay_prob or thresholds, not both")
        if thresholds is not None:
            t = np.array(thresholds, dtype=np.int64, ndmin=1)
            if t.shape != (V,) or ((t < 0) | (t > 0xFFFFFFFF)).any():
                raise ValueError("thresholds must be one uint32 per peer")
            t = np.ascontiguousarray(t, dtype=np.uint32)
        elif relay_prob is not None:
            t = self.relay_thresholds(relay_prob, V)
        else:
            t = None
        self._check(_lib.lib().p2pg_set_relay_policy(self._h, V, _lib.ptr(t) if t is not None else None,
                                                     ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)))
        self.relay_thr = t if t is not None and t.any() else None
        self.relay_seed = int(seed) & 0xFFFFFFFFFFFFFFFF if self.relay_thr is not None else 0

    @staticmethod
    def peer_offline(round, offline_from, offline_until):
        """Is a peer with the downtime interval [``offline_from``, ``offline_until``) offline in
        ``round``?  (p2pg_peer_offline; ``offline_from`` -1 = never, ``offline_until`` None or -1 =
        forever.)"""
        until = _FOREVER if offline_until is None or int(offline_until) == -1 else int(offline_until)
        return bool(_lib.lib().p2pg_peer_offline(int(round), int(offline_from), until))

    def set_downtime(self, offline_from, offline_until=None):
        """Per-peer downtime, before round 0 runs (or after ``reset``): peer v is offline in the
        rounds ``offline_from[v] <= r < offline_until[v]`` (``offline_from[v]`` = -1: never; 0: it
        joins late; ``offline_until`` None, or -1 entries: forever, a crash).  An offline peer keeps
        its connections: its neighbours go on sending to it, and those sends are counted by their
        senders and lost.  It has no first receipts and sends nothing; after its return it may
        still get a message from a later copy.  Originations at an offline peer are refused.
        ``set_downtime(None)`` (or all -1) removes it.  ``reset`` and ``broadcast`` keep it
        (p2pg_set_downtime)."""
        V = self.graph.V
        if offline_from is None:
            self._check(_lib.lib().p2pg_set_downtime(self._h, V, None, None))
            self.offline_from = self.offline_until = None
            return
        f = np.array(offline_from, dtype=np.int64, ndmin=1)
        u = np.full(V, -1, dtype=np.int64) if offline_until is None else np.array(offline_until, dtype=np.int64, ndmin=1)
        if f.shape != (V,) or u.shape != (V,):
            raise ValueError("offline_from / offline_until must hold one round per peer")
        u = np.where(u == -1, _FOREVER, u)
        if ((f < -(1 << 31)) | (f > _FOREVER) | (u < -(1 << 31)) | (u > _FOREVER)).any():
            raise ValueError("offline_from / offline_until must be int32 rounds")
        f = np.ascontiguousarray(f, dtype=np.int32)
        u = np.ascontiguousarray(u, dtype=np.int32)
        self._check(_lib.lib().p2pg_set_downtime(self._h, V, _lib.ptr(f), _lib.ptr(u)))
        on = bool((f >= 0).any())
        self.offline_from = f if on else None
        self.offline_until = u if on else None

    @staticmethod
    def link_cut(round, side_a, side_b, cut_from, cut_until):
        """Is a connection between a peer of ``side_a`` and a peer of ``side_b`` cut in ``round``
        under the window [``cut_from``, ``cut_until``)?  (p2pg_link_cut)"""
        return bool(_lib.lib().p2pg_link_cut(int(round), int(side_a), int(side_b), int(cut_from), int(cut_until)))

    def set_netsplit(self, side, cut_from=0, cut_until=0):
        """A network partition that heals, before round 0 runs (or after ``reset``): peer v is on
        side ``side[v]`` (>= 0) and every connection between two sides is cut in the rounds
        ``cut_from <= r < cut_until``.  Peers keep their connections and go on sending over a cut
        connection; a send that would arrive in a cut round is counted by its sender and lost,
        anti-entropy requests and replies included.  ``set_netsplit(None)``, equal sides or an empty
        window remove it.  Not together with hop limits, a relay policy, ``drop_relays``,
        ``update_edges`` or snapshots.  ``reset`` and ``broadcast`` keep it (p2pg_set_netsplit)."""
        V = self.graph.V
        if side is None:
            self._check(_lib.lib().p2pg_set_netsplit(self._h, V, None, 0, 0))
            self.netsplit = None
            return
        s = np.array(side, dtype=np.int64, ndmin=1)
        if s.shape != (V,):
            raise ValueError("side must hold one side per peer")
        for x in (cut_from, cut_until):
            if not -(1 << 31) <= int(x) <= _FOREVER:
                raise ValueError("cut_from and cut_until must be int32 rounds")
        if ((s < -(1 << 31)) | (s > _FOREVER)).any():
            raise ValueError("sides must be int32")
        s = np.ascontiguousarray(s, dtype=np.int32)
        self._check(_lib.lib().p2pg_set_netsplit(self._h, V, _lib.ptr(s), int(cut_from), int(cut_until)))
        g = self.graph
        crossing = bool((s[np.repeat(np.arange(V), np.diff(g.rowptr))] != s[g.colidx]).any())
        on = crossing and int(cut_from) < int(cut_until)
        self.netsplit = (s, int(cut_from), int(cut_until)) if on else None

    def set_anti_entropy(self, period, first_round=0, last_round=None, seed=0):
        """Periodic pull repair, before round 0 runs (or after ``reset``): in every round r with
        ``first_round <= r <= last_round`` and ``(r - first_round) % period == 0`` each online peer
        with a connection asks one drawn connection (``pull_partner``) for the messages it is
        missing; the partner answers in round r + 1 and what the reply lists is first-received in
        round r + 2 and relayed like any other receipt.  Requests and replies are lost like any
        send of their round (churn, an offline receiver) and are counted per exchange
        (``pull_stats``), never in the relay counters.  ``last_round`` is mandatory: the run goes on
        until the last exchange is complete.  Not together with hop limits or a relay policy.
        ``set_anti_entropy(None)`` removes it.  ``reset`` and ``broadcast`` keep it
        (p2pg_set_anti_entropy)."""
        if period is None or int(period) == 0:
            self._check(_lib.lib().p2pg_set_anti_entropy(self._h, 0, 0, 0, 0))
            self.anti_entropy = None
            return
        if last_round is None:
            raise ValueError("set_anti_entropy needs last_round (the run ends after the last exchange)")
        for x in (period, first_round, last_round):
            if not -(1 << 31) <= int(x) <= _FOREVER:
                raise ValueError("period, first_round and last_round must be int32")
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._check(_lib.lib().p2pg_set_anti_entropy(self._h, int(first_round), int(last_round), int(period), seed))
        self.anti_entropy = (int(period), int(first_round), int(last_round), seed)
        self._quiet = False

    def pull_partner(self, round, peer):
        """The connection ``peer`` sends its anti-entropy request of ``round`` to (whether or not
        ``round`` is a request round), or -1 for a peer without connections
        (p2pg_pull_partner_slot)."""
        if self.anti_entropy is None:
            raise ValueError("no anti-entropy is set")
        nb = self.graph.neighbours(int(peer))
        j = _lib.lib().p2pg_pull_partner_slot(int(round), int(peer), len(nb), self.anti_entropy[3])
        return -1 if j < 0 else int(nb[j])

    def pull_stats(self):
        """The anti-entropy exchanges completed in this run, one record each (PULL_STATS_DTYPE:
        request_round, requests, requests_lost, replies, replies_lost, repaired), in order of
        request round (p2pg_get_pull_stats)."""
        n = ctypes.c_int64()
        self._check(_lib.lib().p2pg_get_pull_stats(self._h, 0, None, ctypes.byref(n)))
        out = np.zeros(n.value, dtype=PULL_STATS_DTYPE)
        if n.value:
            self._check(_lib.lib().p2pg_get_pull_stats(self._h, n.value, _lib.ptr(out), ctypes.byref(n)))
        return out

    def originate(self, msgs, peers, round=None):
        """Between rounds: start the unscheduled broadcasts ``msgs`` at ``peers`` in ``round``
        (default: the next round to run) -- the send_to_nodes(data) an app decides on while it
        runs, e.g. a reply made in ``node_message_batch`` (p2pg_originate).  Wakes a network
        that had gone quiet: ``run`` / ``step`` continue."""
        m = np.array(msgs, dtype=np.int32, ndmin=1)
        p = np.array(peers, dtype=np.int32, ndmin=1)
        if m.ndim != 1 or m.shape != p.shape:
            raise ValueError("msgs and peers must be 1-D arrays of the same length")
        if round is None:
            round = max(1, self._next_round)
        self._check(_lib.lib().p2pg_originate(self._h, len(m), _lib.ptr(m) if len(m) else None,
                                              _lib.ptr(p) if len(p) else None, int(round)))
        self.sources[m] = p
        self.start_rounds[m] = int(round)
        if len(m):
            self._quiet = False

    def reset(self):
        """Back to round 0 with the same sources and start rounds (``originate`` included)."""
        self._check(_lib.lib().p2pg_reset(self._h))
        self.rounds = []
        self.message_count_send = 0
        self._next_round, self._quiet = 0, False

    def _ran(self, st):
        """Book-keeping of the next round to run (``originate``'s default) after round stats st."""
        if not self._quiet:
            self._next_round = st.round + 1
            self._quiet = self._autostop and not st.active

    def step_begin(self):
        """Start the next round asynchronously: on a vertex-partitioned rank, the peers with no
        ghost neighbour (p2pg_step_begin); ``step`` / ``step_end`` finishes the round."""
        self._check(_lib.lib().p2pg_step_begin(self._h))

    def step_end(self):
        return self.step()

    def step(self):
        """Run one round; returns its RoundStats (``active`` = messages still in flight)."""
        s = _lib.RoundStatsC()
        self._check(_lib.lib().p2pg_step(self._h, ctypes.byref(s)))
        st = RoundStats.from_c(s)
        self.rounds.append(st)
        self.message_count_send += st.relays
        self._ran(st)
        if st.new_deliveries and self._wants_deliveries():
            self.node_message_batch(self.deliveries())
        return st

    def run(self, max_rounds=1 << 20):
        """Rounds until quiescence; returns the list of RoundStats (last one has no receipts)."""
        if not self._wants_deliveries():
            buf = self._run_buf
            if buf is None:  # (kept: a fresh 4096-entry array per call costs ~20 us of host time)
                buf = self._run_buf = (_lib.RoundStatsC * 4096)()
            out = []
            while len(out) < max_rounds:
                n = ctypes.c_int32()
                chunk = min(max_rounds - len(out), len(buf))
                rc = _lib.lib().p2pg_run(self._h, chunk, buf, ctypes.byref(n))
                got = RoundStats.from_c_array(buf, n.value)  # rounds that stand are kept even
                out.extend(got)                              # if the call failed
                self.rounds.extend(got)
                self.message_count_send += sum(st.relays for st in got)
                if got:
                    self._ran(got[-1])
                rc = self._check(rc)
                if rc == 0 or n.value == 0:
                    break
            return out
        out = []
        while len(out) < max_rounds:
            st = self.step()
            out.append(st)
            if not st.active:
                break
        return out

    # -- topology changes between rounds ------------------------------
    def update_edges(self, add=(), remove=()):
        """Connect the (a, b) pairs in ``add`` (Node.connect_with_node, node.py:122-176) and
        disconnect those in ``remove`` (Node.disconnect_with_node, node.py:178-189) between
        rounds.  Messages in flight on a removed connection are lost; every send from the next
        round on uses the new connections (include/p2pgpu.h p2pg_update_edges)."""
        a = np.ascontiguousarray(np.asarray(add, dtype=np.int32).reshape(-1, 2))
        r = np.ascontiguousarray(np.asarray(remove, dtype=np.int32).reshape(-1, 2))
        self._check(_lib.lib().p2pg_update_edges(self._h, len(a), _lib.ptr(a) if len(a) else None,
                                                 len(r), _lib.ptr(r) if len(r) else None))
        self.graph = self.graph.with_changes(a, r)

    def connect(self, pairs):
        self.update_edges(add=pairs)

    def disconnect(self, pairs):
        self.update_edges(remove=pairs)

    # -- snapshot / resume ------------------------------------------
    def snapshot(self):
        """The run state between rounds as a uint8 array (p2pg_snapshot)."""
        n = ctypes.c_int64()
        self._check(_lib.lib().p2pg_snapshot_size(self._h, ctypes.byref(n)))
        buf = np.empty(max(n.value, 1), dtype=np.uint8)
        self._check(_lib.lib().p2pg_snapshot(self._h, _lib.ptr(buf), n.value))
        return buf[:n.value]

    def restore(self, buf):
        """Continue from a snapshot of an engine with the same configuration, graph and
        sources (call broadcast(sources) first)."""
        b = np.ascontiguousarray(buf, dtype=np.uint8)
        self._check(_lib.lib().p2pg_restore(self._h, _lib.ptr(b), len(b)))
        self.rounds = []
        head = np.frombuffer(b[:128].tobytes(), dtype=np.uint64)
        self.message_count_send = int(head[_SNAP_TOTAL_RELAYS_WORD])
        self._next_round = int(head[5] >> np.uint64(32))        # SnapHeader.round
        self._quiet = self._autostop and bool(head[7] >> np.uint64(32))  # SnapHeader.done

    def save_snapshot(self, path):
        np.save(path, self.snapshot(), allow_pickle=False)

    def load_snapshot(self, path):
        self.restore(np.load(path, allow_pickle=False))

    # -- the batched hook (override like Node.node_message, node.py:334-338) --------------
    def node_message_batch(self, deliveries):
        if self.callback is not None:
            self.callback("node_message_batch", self, None, deliveries)

    def _wants_deliveries(self):
        return (self.callback is not None
                or type(self).node_message_batch is not GraphNetwork.node_message_batch)

    def deliveries_count(self):
        """Number of first-receipt records the last round's delivery stream holds."""
        n = ctypes.c_int64()
        z = np.zeros(1, dtype=np.int32)
        self._check(_lib.lib().p2pg_get_new_deliveries(self._h, 0, _lib.ptr(z), _lib.ptr(z), _lib.ptr(z),
                                                        _lib.ptr(z), ctypes.byref(n)))
        return int(n.value)

    def deliveries(self, cap=None):
        """First receipts of the most recent round as (peer, msg, hop, parent) arrays."""
        if cap is None:
            cap = self.rounds[-1].new_deliveries if self.rounds else 0
        cap = int(cap)
        peer = np.zeros(max(cap, 1), dtype=np.int32)
        msg = np.zeros_like(peer)
        hop = np.zeros_like(peer)
        parent = np.zeros_like(peer)
        n = ctypes.c_int64()
        self._check(_lib.lib().p2pg_get_new_deliveries(
            self._h, cap, _lib.ptr(peer), _lib.ptr(msg), _lib.ptr(hop), _lib.ptr(parent), ctypes.byref(n)))
        k = min(n.value, cap)
        return Deliveries(peer[:k], msg[:k], hop[:k], parent[:k])

    def sends(self):
        """Every send of the most recent round (p2pg_get_sends): the packets its first receipts
        put on the wire, duplicates included, after any drop_relays."""
        n = ctypes.c_int64()
        z = np.zeros(1, dtype=np.int32)
        z8 = np.zeros(1, dtype=np.uint8)
        L = _lib.lib()
        self._check(L.p2pg_get_sends(self._h, 0, _lib.ptr(z), _lib.ptr(z), _lib.ptr(z), _lib.ptr(z8),
                                     ctypes.byref(n)))
        cap = int(n.value)
        snd = np.zeros(max(cap, 1), dtype=np.int32)
        rcv = np.zeros_like(snd)
        msg = np.zeros_like(snd)
        lost = np.zeros(max(cap, 1), dtype=np.uint8)
        self._check(L.p2pg_get_sends(self._h, cap, _lib.ptr(snd), _lib.ptr(rcv), _lib.ptr(msg), _lib.ptr(lost),
                                     ctypes.byref(n)))
        k = min(int(n.value), cap)
        return Sends(snd[:k], rcv[:k], msg[:k], lost[:k].astype(bool))

    def drop_relays(self, peer, msg):
        """Withdraw the relays of these first receipts of the most recent round: the app did not
        forward them (p2pg_drop_relays)."""
        p = np.ascontiguousarray(peer, dtype=np.int32)
        m = np.ascontiguousarray(msg, dtype=np.int32)
        if len(p) != len(m):
            raise ValueError("peer and msg must have the same length")
        self._check(_lib.lib().p2pg_drop_relays(self._h, len(p), _lib.ptr(p) if len(p) else None,
                                                _lib.ptr(m) if len(m) else None))
        last = self.rounds[-1].round if self.rounds else -1
        origin = (self.start_rounds[m] == last).tolist()  # a message's own origination: all deg
        # (a receipt of a message whose hop limit ran out in that round made no relays)
        spent = ((self.ttl[m] >= 0) & (self.start_rounds[m].astype(np.int64) + self.ttl[m] == last)).tolist()
        if self.relay_thr is not None and last > 0:  # (nor did one the relay policy muted)
            base = int(self.config.msg_id_base)
            spent = [x or (not o and self.relay_muted(last, v, base + k, int(self.relay_thr[v]), self.relay_seed))
                     for x, o, v, k in zip(spent, origin, p.tolist(), m.tolist())]
        drop = sum(0 if x else min(self.fanout, d) if self.mode == "gossip" else (d if o else max(d - 1, 0))
                   for d, o, x in zip(self.graph.degree()[p].tolist(), origin, spent))
        self.message_count_send -= drop

    # -- validation planes ----------------------------------------------------------------
    def seen_plane(self):
        out = np.zeros((self.graph.V, self.W), dtype=np.uint64)
        self._check(_lib.lib().p2pg_read_planes(self._h, _lib.ptr(out), None, None))
        return out

    def seen_word(self, w):
        """uint64 [V]: word w of every peer's seen row (messages 64w .. 64w+63), without
        copying the whole plane (p2pg_read_seen_word)."""
        out = np.zeros(self.graph.V, dtype=np.uint64)
        self._check(_lib.lib().p2pg_read_seen_word(self._h, int(w), _lib.ptr(out)))
        return out

    def delivered(self):
        """bool [V, M]: peer v has received broadcast m (its dedup 'seen' set)."""
        s = self.seen_plane()
        bits = np.unpackbits(s.view(np.uint8).reshape(self.graph.V, -1), axis=1, bitorder="little")
        return bits[:, :self.M].astype(bool)

    # -- run tallies, computed on the device -------------------------------------------------
    def message_reach(self):
        """uint64 [M]: peers that hold each broadcast now -- the column counts of the seen plane,
        without copying it (p2pg_message_reach; needs no flag)."""
        out = np.zeros(self.M, dtype=np.uint64)
        self._check(_lib.lib().p2pg_message_reach(self._h, _lib.ptr(out)))
        return out

    def message_tally(self):
        """MessageTally(reach, hop_sum, last_hop) per broadcast, accumulated from every round's
        first receipts; needs tally=True (p2pg_message_tally).  Hops are absolute round indices:
        for a broadcast that started late, the mean hop counted from its own start is
        ``hop_sum / reach - start_rounds`` and its last hop ``last_hop - start_rounds``
        (``message_latency()`` with latency=True gives the whole distribution from the start)."""
        reach = np.zeros(self.M, dtype=np.uint64)
        hop_sum = np.zeros(self.M, dtype=np.uint64)
        last_hop = np.zeros(self.M, dtype=np.int32)
        self._check(_lib.lib().p2pg_message_tally(self._h, _lib.ptr(reach), _lib.ptr(hop_sum),
                                                  _lib.ptr(last_hop)))
        return MessageTally(reach, hop_sum, last_hop)

    def peer_counters(self):
        """PeerCounters(sent, received) per peer: Node.message_count_send / message_count_recv of
        the rounds run so far; needs tally=True.  Read them after a round boundary's drop_relays /
        update_edges: those calls refuse once the boundary's sends are counted
        (p2pg_peer_counters)."""
        sent = np.zeros(self.graph.V, dtype=np.uint64)
        received = np.zeros(self.graph.V, dtype=np.uint64)
        self._check(_lib.lib().p2pg_peer_counters(self._h, _lib.ptr(sent), _lib.ptr(received)))
        return PeerCounters(sent, received)

    def message_cost(self):
        """MessageCost(sent, received) per broadcast: the send_to_node calls that carried it in
        the rounds run so far (lost ones included, withdrawn relays not) and those of them that
        arrived; needs cost=True.  The records of ``sends()`` binned by message.  Read it after a
        round boundary's drop_relays / update_edges, as ``peer_counters()`` (p2pg_message_cost)."""
        sent = np.zeros(self.M, dtype=np.uint64)
        received = np.zeros(self.M, dtype=np.uint64)
        self._check(_lib.lib().p2pg_message_cost(self._h, _lib.ptr(sent), _lib.ptr(received)))
        return MessageCost(sent, received)

    # -- delivery latency, computed on the device ---------------------------------------------
    def set_latency_bins(self, bins):
        """The histograms' number of bins, 2..1024, before round 0 runs or after ``reset``
        (p2pg_set_latency_bins); needs latency=True and sources."""
        self._check(_lib.lib().p2pg_set_latency_bins(self._h, int(bins)))
        self.latency_bins = self._engine_bins = int(bins)

    def message_latency(self):
        """uint64 [M, bins]: per broadcast the histogram of its first receipts by relative hop
        (round - start round; the origination is hop 0), the last bin collecting every hop >=
        bins - 1; needs latency=True (p2pg_message_latency).  Rows sum to ``message_reach()``."""
        bins = self._engine_bins
        out = np.zeros((self.M, bins), dtype=np.uint64)
        self._check(_lib.lib().p2pg_message_latency(self._h, bins, _lib.ptr(out)))
        return out

    def peer_latency(self):
        """PeerLatency(hop_sum, receipts, max_hop) per peer, exact whatever the number of bins;
        needs latency=True (p2pg_peer_latency).  ``.mean()`` is the peer's mean relative hop."""
        hop_sum = np.zeros(self.graph.V, dtype=np.uint64)
        receipts = np.zeros(self.graph.V, dtype=np.uint32)
        max_hop = np.zeros(self.graph.V, dtype=np.int32)
        self._check(_lib.lib().p2pg_peer_latency(self._h, _lib.ptr(hop_sum), _lib.ptr(receipts),
                                                 _lib.ptr(max_hop)))
        return PeerLatency(hop_sum, receipts, max_hop)

    def coverage_curve(self, of="reach"):
        """float64 [M, bins]: the share delivered within b rounds of the broadcast's start --
        ``cumsum(message_latency(), axis=1)`` over the broadcast's final reach (``of="reach"``) or
        over the number of peers (``of="peers"``).  NaN for a broadcast with reach 0 (an
        unscheduled one).  The last column includes the clamped receipts.  Host arithmetic."""
        if of not in ("reach", "peers"):
            raise ValueError("of must be 'reach' or 'peers'")
        cum = np.cumsum(self.message_latency(), axis=1, dtype=np.uint64)
        reach = cum[:, -1].astype(np.float64)
        den = reach if of == "reach" else np.full(self.M, float(self.graph.V))
        out = np.full(cum.shape, np.nan)
        ok = reach > 0
        out[ok] = cum[ok].astype(np.float64) / den[ok, None]
        return out

    def latency_percentile(self, q):
        """int32 [M]: the smallest relative hop b by which at least ceil(q * reach) of the
        broadcast's first receipts had happened, 0 < q <= 1 (q = 0.5: the median rounds to
        delivery); -1 for a broadcast with reach 0.  A result of ``bins - 1`` is a lower bound:
        that bin holds every later receipt as well.  Host arithmetic on ``message_latency()``."""
        if not 0.0 < q <= 1.0:
            raise ValueError("q must lie in (0, 1]")
        cum = np.cumsum(self.message_latency(), axis=1, dtype=np.uint64)
        reach = cum[:, -1]
        need = np.ceil(q * reach.astype(np.float64)).astype(np.uint64)
        out = (cum < need[:, None]).sum(axis=1).astype(np.int32)
        out[reach == 0] = -1
        return out

    def message_redundancy(self):
        """float64 [M]: the relative message redundancy of each broadcast, sent / (reach - 1) - 1
        (0 = every peer reached got exactly one copy, as over a spanning tree); NaN where the
        broadcast reached nobody but its origin.  Host arithmetic on ``message_cost()`` and
        ``message_reach()``; needs cost=True."""
        sent = self.message_cost().sent.astype(np.float64)
        reach = self.message_reach().astype(np.float64)
        out = np.full(self.M, np.nan)
        ok = reach > 1
        out[ok] = sent[ok] / (reach[ok] - 1.0) - 1.0
        return out

    def hop_parent(self, relative=False):
        """(hop, parent) int32 [V, M]; needs record=True.  -1 = not delivered / origin.  Hops are
        absolute round indices; ``relative=True`` subtracts each broadcast's start round from its
        delivered hops (-1 stays -1)."""
        if not self.record:
            raise RuntimeError("hop/parent planes need GraphNetwork(record=True)")
        hop = np.zeros((self.graph.V, self.M), dtype=np.int32)
        par = np.zeros_like(hop)
        self._check(_lib.lib().p2pg_read_planes(self._h, None, _lib.ptr(hop), _lib.ptr(par)))
        if relative:
            hop = np.where(hop >= 0, hop - self.start_rounds[None, :], -1).astype(np.int32)
        return hop, par

    KERNEL_CLASSES = ("seed", "flood_pull", "gossip_scatter_atomic", "record", "gossip_update",
                      "gossip_pull", "gossip_scatter_store", "gossip_fused")

    def kernel_times(self):
        """Summed device ms and launch counts per kernel class since the last reset (needs
        timing=True); classes as in include/p2pgpu.h (P2PG_KCLASS_N)."""
        n = len(self.KERNEL_CLASSES)
        ms = np.zeros(n, dtype=np.float64)
        cnt = np.zeros(n, dtype=np.int64)
        self._check(_lib.lib().p2pg_kernel_times(self._h, _lib.ptr(ms), _lib.ptr(cnt)))
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(self.KERNEL_CLASSES)}

    def set_timed_classes(self, classes=None):
        """Time only these kernel classes with HIP events (None = all; p2pg_set_timed_classes):
        events cost stream time, so a measurement can bracket its dominant kernel alone."""
        names = self.KERNEL_CLASSES if classes is None else classes
        mask = 0
        for k in names:
            mask |= 1 << self.KERNEL_CLASSES.index(k)
        self._check(_lib.lib().p2pg_set_timed_classes(self._h, mask))

    # -- vertex-partitioned runs (p2pnetwork.gpu.partition) --------------------------------
    def set_global_ids(self, gid):
        self._gid = np.ascontiguousarray(gid, dtype=np.int32)
        self._check(_lib.lib().p2pg_set_global_ids(self._h, _lib.ptr(self._gid)))

    def set_ghost_senders(self, ghost_deg, slot_pos):
        """Partitioned gossip records / deliveries: the ghosts' global degrees and, per local
        slot, the row owner's position in its ghost neighbour's global adjacency (-1 = local
        neighbour) -- p2pg_set_ghost_senders."""
        self._gdeg = np.ascontiguousarray(ghost_deg, dtype=np.int32)
        self._gpos = np.ascontiguousarray(slot_pos, dtype=np.int32)
        self._check(_lib.lib().p2pg_set_ghost_senders(self._h, _lib.ptr(self._gdeg), _lib.ptr(self._gpos)))

    def set_exchange(self, send_local, recv_local):
        s = np.ascontiguousarray(send_local, dtype=np.int32)
        r = np.ascontiguousarray(recv_local, dtype=np.int32)
        self._check(_lib.lib().p2pg_set_exchange(self._h, len(s), _lib.ptr(s), len(r), _lib.ptr(r)))

    def set_exchange_segments(self, send_counts, recv_counts):
        """Rows per rank of the send / recv lists (p2pg_set_exchange_segments)."""
        sc = np.ascontiguousarray(send_counts, dtype=np.int64)
        rc = np.ascontiguousarray(recv_counts, dtype=np.int64)
        self._nseg = len(sc)
        self._check(_lib.lib().p2pg_set_exchange_segments(self._h, len(sc), _lib.ptr(sc), _lib.ptr(rc)))

    def exchange_pack_live(self, plane, buf):
        """Pack the live rows of the last round as records into device buffer ``buf``; returns
        the record count per destination rank (p2pg_exchange_pack_live)."""
        counts = np.zeros(self._nseg, dtype=np.int64)
        self._check(_lib.lib().p2pg_exchange_pack_live(self._h, int(plane), ctypes.c_void_p(buf.data_ptr()),
                                                       _lib.ptr(counts)))
        return counts

    def set_exchange_buffer(self, plane, buf):
        """Pack the live rows of ``plane`` into device buffer ``buf`` inside every round, their
        counts read back with the round counters (p2pg_set_exchange_buffer); ``None`` = off."""
        self._check(_lib.lib().p2pg_set_exchange_buffer(
            self._h, int(plane), ctypes.c_void_p(buf.data_ptr()) if buf is not None else None))

    def exchange_unpack_live(self, plane, buf, counts):
        c = np.ascontiguousarray(counts, dtype=np.int64)
        self._check(_lib.lib().p2pg_exchange_unpack_live(self._h, int(plane), ctypes.c_void_p(buf.data_ptr()),
                                                         _lib.ptr(c)))

    def alloc_exchange(self, n_words):
        """Device buffer for exchange rows (a torch tensor on this engine's GPU)."""
        import torch
        return torch.empty(max(int(n_words), 1), dtype=torch.int64, device=f"cuda:{self.config.device}")

    def exchange_pack(self, plane, buf):
        self._check(_lib.lib().p2pg_exchange_pack(self._h, int(plane), ctypes.c_void_p(buf.data_ptr())))

    def exchange_unpack(self, plane, buf):
        self._check(_lib.lib().p2pg_exchange_unpack(self._h, int(plane), ctypes.c_void_p(buf.data_ptr())))

    def device_philox(self, ctr, key):
        """Evaluate Philox4x32-10 on the GPU for counters [n, 4] (KAT hook)."""
        c = np.ascontiguousarray(ctr, dtype=np.uint32).reshape(-1, 4)
        k = np.ascontiguousarray(key, dtype=np.uint32)
        out = np.zeros_like(c)
        self._check(_lib.lib().p2pg_device_philox(self._h, len(c), _lib.ptr(c), _lib.ptr(k), _lib.ptr(out)))
        return out
