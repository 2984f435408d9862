"""Numpy restatement of the relay with anti-entropy, periodic pull repair (test infrastructure only).

tests/down_ref.py's loop plus the rule of p2pg_set_anti_entropy.  An exchange happens in every
request round r with ``first <= r <= last`` and ``(r - first) % period == 0``; a round is arrivals,
originations, replies, requests:

  round r      after the arrivals and originations every peer u that is online in r and has a
               connection sends one request to ``colidx[rowptr[u] + j]``, ``j = lemire32(philox((r, u,
               0, 'AEP'), seed).x, deg(u))``, carrying its seen set of that moment (the digest).  Lost
               like any send of round r: the churn draw of (r, {u, p}), or p offline in r + 1.
  round r + 1  p, after its arrivals and originations, answers every request that arrived with the
               messages it has seen by then and the digest lacks -- also when that list is empty.
               A send of round r + 1: lost by churn (r + 1, {p, u}) or because u is offline in r + 2.
  round r + 2  the reply arrives at u as one more packet from sender p, after p's relay packets:
               every listed message u has not seen is a first receipt of round r + 2 with parent
               min(lowest relay sender, p), relayed like any other.

This file keeps the digest and the reply list literally (the engine uses the consequence
``seen_p[end of r + 1] & ~seen_u[before the arrivals of r + 2]``; the tests pin the two to each
other).  Pull packets are counted per exchange and per peer (pull_sent / pull_recv), never in the
relay counters.  The run goes on while a request round lies at or ahead or an exchange is in
flight.  ``late_gather=True`` is the WRONG variant the two-pass split of the engine exists to
avoid -- the reply read when it arrives, after the partner's own arrivals of round r + 2 -- kept so
that the tests can show they tell the two apart.

Draws go through oracle.philox.  down_ref and its yardsticks stay untouched; tests/test_pull.py
pins this loop to down_ref (no exchange) and to the reference's own Node objects
(tests/golden/pull/*.npz).
"""
from dataclasses import dataclass, field

import numpy as np

from down_ref import FOREVER, no_downtime, offline  # noqa: F401  (re-exported for the tests)
from drop_ref import DropResult, _sends
from late_ref import COUNTERS, pad_equal  # noqa: F401
from oracle import philox
from oracle.relay_oracle import _round_stats

TAG_AEP = 0x00414550  # 'AEP'
RECORD = ("request_round", "requests", "requests_lost", "replies", "replies_lost", "repaired")


@dataclass
class PullResult(DropResult):
    # one dict per completed exchange (RECORD), in order of request round
    exchanges: list = field(default_factory=list)
    pull_sent: np.ndarray = None  # int64 [V]: request and reply packets sent (lost ones included)
    pull_recv: np.ndarray = None  # int64 [V]: request and reply packets that arrived
    # bool [V, M] per round: the first receipts no relay copy delivered in that round
    pulled: list = field(default_factory=list)
    # per round: bool [V, M] the unseen messages an arrived reply carried (pulled is the part of it
    # no relay copy delivered), bool [V, M] the first receipts the relay packets made, and int64 [V]
    # the partner whose reply arrived (-1: none)
    fresh: list = field(default_factory=list)
    relay_new: list = field(default_factory=list)
    partner: list = field(default_factory=list)

    def records(self):
        """The exchange records as an int64 [n, 6] array (RECORD's columns)."""
        return np.array([[x[k] for k in RECORD] for x in self.exchanges], dtype=np.int64).reshape(-1, len(RECORD))


def request_round(r, setting):
    """setting = (period, first, last) or None."""
    if not setting or setting[0] <= 0:
        return False
    period, first, last = setting
    return first <= r <= last and (r - first) % period == 0


def arrival_ahead(r, setting):
    """Does an arrival round lie at or ahead of round r?"""
    if not setting or setting[0] <= 0:
        return False
    period, first, last = setting
    return r <= first + (last - first) // period * period + 2


def partner_slot(r, peer, deg, seed):
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    x, _, _, _ = philox.philox4x32_10(r, peer, 0, TAG_AEP, k0, k1)
    return philox.lemire32(x, deg).astype(np.int64)


def partners(r, rowptr, colidx, seed):
    """int64 [V]: the connection every peer would send its request of round r to (-1: deg 0)."""
    deg = np.diff(rowptr)
    V = len(deg)
    out = np.full(V, -1, dtype=np.int64)
    has = deg > 0
    u = np.nonzero(has)[0]
    out[u] = colidx[rowptr[u] + partner_slot(r, u, deg[u], seed)]
    return out


def run(rowptr, colidx, src, start, down_from=None, down_until=None, anti_entropy=None, pull_seed=0, mode="flood",
        fanout=3, gossip_seed=0, msg_id_base=0, churn_threshold=0, churn_seed=0, late_gather=False,
        planes=True, max_rounds=1 << 20):
    """anti_entropy: (period, first, last) or None.  planes=False: the per-round bool planes (pulled,
    fresh, relay_new, dropped) and send lists are not kept (large cases)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colidx = np.asarray(colidx, dtype=np.int64)
    src = np.asarray(src, dtype=np.int64)
    start = np.asarray(start, dtype=np.int64)
    V, M = len(rowptr) - 1, len(src)
    if down_from is None:
        down_from, down_until = no_downtime(V)
    W = (M + 63) // 64
    k = int(fanout)
    gossip = mode == "gossip"
    deg = np.diff(rowptr)
    hop = np.full((V, M), -1, dtype=np.int32)
    parent = np.full((V, M), -1, dtype=np.int32)
    seen = np.zeros((V, M), dtype=bool)
    res = PullResult(hop, parent, np.zeros(V, dtype=np.int64), np.zeros(V, dtype=np.int64))
    res.pull_sent = np.zeros(V, dtype=np.int64)
    res.pull_recv = np.zeros(V, dtype=np.int64)
    last = int(start.max()) if M else -1
    snd = tgt = msg = np.zeros(0, dtype=np.int64)  # the relay sends in flight (not lost)
    none = np.zeros(0, dtype=np.int64)
    req_u, req_p, req_digest = none, none, np.zeros((0, M), dtype=bool)  # the requests in flight
    rep_u, rep_p, rep_list = none, none, np.zeros((0, M), dtype=bool)    # the replies in flight
    rep_list_digest = np.zeros((0, M), dtype=bool)                       # (their requests' digests)
    open_rec = {}  # request round -> its record so far

    def churned(r, a, b):
        c = philox.churn_dropped(r, a, b, churn_threshold, churn_seed)
        return np.broadcast_to(np.asarray(c, dtype=bool), np.shape(a)).copy()

    r = 0
    while r < max_rounds:
        # arrivals of round r (none at an offline peer: those sends were lost)
        new = np.zeros((V, M), dtype=bool)
        best = np.full((V, M), np.iinfo(np.int32).max, dtype=np.int64)
        if len(tgt):
            assert not offline(r, down_from, down_until)[tgt].any()
            new[tgt, msg] = True
            new &= ~seen
            np.minimum.at(best, (tgt, msg), snd)
            np.add.at(res.peer_recv, tgt, 1)
        received = len(tgt)
        # ... and the replies, processed after the relay packets of their sender: what they list and
        # no relay copy delivered is pulled; the parent is the lowest-id sender whose copy arrived
        pulled = np.zeros((V, M), dtype=bool)
        fresh = np.zeros((V, M), dtype=bool)
        if planes:
            res.relay_new.append(new.copy())
        res.partner.append(np.full(V, -1, dtype=np.int64))
        if len(rep_u):
            assert not offline(r, down_from, down_until)[rep_u].any()
            lists = rep_list
            if late_gather:  # (the wrong variant: the partner's row as it stands after its arrivals of round r)
                lists = (seen[rep_p] | new[rep_p]) & ~rep_list_digest
            carried = np.zeros((V, M), dtype=bool)
            carried[rep_u] = lists  # (one request per peer and exchange: rep_u is unique)
            fresh = carried & ~seen
            pulled = fresh & ~new
            pp = np.full(V, np.iinfo(np.int32).max, dtype=np.int64)
            pp[rep_u] = rep_p
            best = np.where(fresh, np.minimum(best, pp[:, None]), best)
            new |= fresh
            np.add.at(res.pull_recv, rep_u, 1)
            rec = open_rec.pop(r - 2)
            rec["repaired"] = int(pulled.sum())
            res.exchanges.append(rec)
            res.partner[-1][rep_u] = rep_p
        elif (r - 2) in open_rec:  # every reply was lost
            rec = open_rec.pop(r - 2)
            rec["repaired"] = 0
            res.exchanges.append(rec)
        parent[new] = best[new]
        origin = np.zeros((V, M), dtype=bool)
        due = np.nonzero(start == r)[0]
        origin[src[due], due] = True
        assert not (origin & seen).any() and not (origin & new).any()
        assert not offline(r, down_from, down_until)[src[due]].any(), "an origination at an offline peer"
        new |= origin
        seen |= new
        hop[new] = r
        if planes:
            res.pulled.append(pulled)
            res.fresh.append(fresh)
        per = np.minimum(deg, k) if gossip else np.maximum(deg - 1, 0)
        st = _round_stats(r, new, deg, per)
        if not gossip:  # an origin has no sender to exclude
            st["relays"] += int(origin.sum(axis=1) @ (deg - np.maximum(deg - 1, 0)))
        st["received"] = received
        res.relays_offered.append(int(st["relays"]))
        if planes:
            res.dropped.append(np.zeros((V, M), dtype=bool))
        # the relay sends of round r
        snd, tgt, msg = _sends(rowptr, colidx, r, new, parent, gossip, k, gossip_seed, msg_id_base)
        assert len(snd) == st["relays"], (r, len(snd), st["relays"])
        np.add.at(res.peer_sent, snd, 1)
        ch = churned(r, snd, tgt)
        lost = ch | offline(r + 1, down_from, down_until)[tgt]
        order = np.lexsort((msg, snd, tgt))
        if planes:
            res.sends.append((snd[order], tgt[order], msg[order], lost[order].copy()))
        if gossip and (~ch).any():  # (the masks towards offline receivers are pushed too)
            st["scatter_words"] = int(len(np.unique((snd[~ch] * V + tgt[~ch]) * W + msg[~ch] // 64)))
        keep = ~lost
        snd, tgt, msg = snd[keep], tgt[keep], msg[keep]
        res.rounds.append(st)
        # the replies of round r: one per request that arrived, after the arrivals and originations
        rep_u, rep_p, rep_list = none, none, np.zeros((0, M), dtype=bool)
        rep_list_digest = np.zeros((0, M), dtype=bool)
        if len(req_u):
            assert not offline(r, down_from, down_until)[req_p].any()
            np.add.at(res.pull_recv, req_p, 1)
            np.add.at(res.pull_sent, req_p, 1)
            lists = seen[req_p] & ~req_digest
            lost = churned(r, req_p, req_u) | offline(r + 1, down_from, down_until)[req_u]
            rec = open_rec[r - 1]
            rec["replies"] = int(len(req_u))
            rec["replies_lost"] = int(lost.sum())
            rep_u, rep_p, rep_list = req_u[~lost], req_p[~lost], lists[~lost]
            rep_list_digest = req_digest[~lost]
        # the requests of round r
        req_u, req_p, req_digest = none, none, np.zeros((0, M), dtype=bool)
        if request_round(r, anti_entropy):
            u = np.nonzero((deg > 0) & ~offline(r, down_from, down_until))[0]
            p = colidx[rowptr[u] + partner_slot(r, u, deg[u], pull_seed)] if len(u) else none
            np.add.at(res.pull_sent, u, 1)
            lost = churned(r, u, p) | offline(r + 1, down_from, down_until)[p]
            open_rec[r] = dict(request_round=r, requests=int(len(u)), requests_lost=int(lost.sum()), replies=0,
                               replies_lost=0, repaired=0)
            req_u, req_p, req_digest = u[~lost], p[~lost], seen[u[~lost]].copy()
        if not new.any() and last <= r and not arrival_ahead(r + 1, anti_entropy):
            break
        r += 1
    assert not open_rec
    return res


# What every anti-entropy fixture must hold, so none passes vacuously (tests/golden/
# make_pull_golden.py asserts it when it writes them, tests/test_pull.py from the data).  Parent
# outcomes: a (peer, message) the same case without anti-entropy never delivers and a reply now
# does; a pulled receipt whose parent is the partner; one whose relay sender has the lower id.
# Lost packets (the churn items only under churn): a request and a reply lost to churn, a request to
# an offline partner, a reply to a peer that went offline.  Relays: a pulled receipt relayed on by
# a flood peer of degree >= 3 / a gossip peer with deg > k.  Race and row state: a peer that is
# somebody's partner and itself gains a bit by pull in the arrival round in which its requester,
# who lacks that bit, does not get it; a pull into a row without a relayed receipt in that round and
# one into a row with some; a row that becomes full by pull.
CENSUS = ("repaired_never", "parent_partner", "parent_relay", "request_churned", "reply_churned",
          "request_offline", "reply_offline", "relayed_on", "race", "row_inactive", "row_active", "row_full")


# The one exemption, by fixture name.  The downtime schedule of pull_rrg200_flood is the down
# fixture's and is not redrawn.  In a flood without churn a peer lacks a message for good only if
# every neighbour sent it while the peer was offline; under this schedule ten peers do (four of them
# crashed), no two of them are neighbours, and none of them returns after the last broadcasts (start
# rounds 30 .. 45) have passed.  So no requester and its partner ever lack the same message (race),
# and a pull never delivers the last message a row lacks (row_full).  Every setting with period 1,
# first 1 .. 3, last = the last return + 3 or + 5 and seeds 0 .. 399 (2400 runs) gives neither.  The
# other three fixtures hold both; the wrong variant (late_gather) is told apart on them and on the
# hand case.
EXEMPT = {"pull_rrg200_flood": ("race", "row_full")}


def census_items(gossip, churn):
    skip = () if churn else ("request_churned", "reply_churned")
    return tuple(x for x in CENSUS if x not in skip)


def census(z, res, nopull):
    """The census of one fixture: res = pull_ref on its inputs, nopull = the same case without
    anti-entropy.  Returns {item: found}."""
    rowptr, colidx = np.asarray(z["rowptr"], dtype=np.int64), np.asarray(z["colidx"], dtype=np.int64)
    f, u_ = z["down_from"], z["down_until"]
    deg = np.diff(rowptr)
    gossip, k = str(z["mode"]) == "gossip", int(z["fanout"])
    period, first, last = (int(x) for x in z["anti_entropy"])
    seed, cthr, cseed = int(z["pull_seed"]), int(z["churn_threshold"]), int(z["churn_seed"])
    hop, parent = res.hop, res.parent
    V, M = hop.shape
    got = dict.fromkeys(CENSUS, False)

    def churned(r, a, b):
        c = philox.churn_dropped(r, a, b, cthr, cseed)
        return np.broadcast_to(np.asarray(c, dtype=bool), np.shape(a))

    for r in range(len(res.rounds)):
        if request_round(r, (period, first, last)):
            u = np.nonzero((deg > 0) & ~offline(r, f, u_))[0]
            p = colidx[rowptr[u] + partner_slot(r, u, deg[u], seed)]
            c1 = churned(r, u, p)
            o1 = offline(r + 1, f, u_)[p]
            got["request_churned"] |= bool(c1.any())
            got["request_offline"] |= bool((o1 & ~c1).any())
            ok = ~(c1 | o1)
            c2 = churned(r + 1, p[ok], u[ok])
            o2 = offline(r + 2, f, u_)[u[ok]]
            got["reply_churned"] |= bool(c2.any())
            got["reply_offline"] |= bool((o2 & ~c2).any())
        pulled, fresh, pp, rnew = res.pulled[r], res.fresh[r], res.partner[r], res.relay_new[r]
        if not fresh.any():
            continue
        got["repaired_never"] |= bool((pulled & (nopull.hop < 0)).any())
        got["parent_partner"] |= bool((pulled & (parent == pp[:, None])).any())
        got["parent_relay"] |= bool((fresh & (parent < pp[:, None]) & (parent >= 0)).any())
        rows = pulled.any(axis=1)
        got["relayed_on"] |= bool((rows & (deg > k if gossip else deg >= 3)).any())
        got["row_inactive"] |= bool((rows & ~rnew.any(axis=1)).any())
        got["row_active"] |= bool((rows & rnew.any(axis=1)).any())
        before = (hop >= 0) & (hop < r)
        got["row_full"] |= bool((rows & ~before.all(axis=1) & ((hop >= 0) & (hop <= r)).all(axis=1)).any())
        # the race: u's partner p gains m by pull in round r, u lacks m and does not get it in round r
        us = np.nonzero(pp >= 0)[0]
        gain = pulled[pp[us]]  # [n, M]: what each requester's partner pulls in this round
        lacks = ~((hop[us] >= 0) & (hop[us] <= r))
        got["race"] |= bool((gain & lacks).any())
    return got
