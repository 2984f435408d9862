"""Numpy restatement of the relay with peer downtime (test infrastructure only).

tests/drop_ref.py's loop with one more way to lose a send.  Peer v is offline in the rounds
``down_from[v] <= r < down_until[v]`` (``down_from[v]`` = -1: never; ``down_until[v]`` = FOREVER:
it never returns).  An offline peer keeps its connections and its neighbours go on sending to it:
a send of round r addressed to u is lost iff it was lost before (churn, a connection removed at the
boundary) or u is offline in round r + 1.  A lost send is counted by its sender (the round's
relays, peer_sent, the send list with lost = 1) and is no arrival: not in the next round's
``received``, not in peer_recv, no seen bit.  So an offline peer has no first receipts and sends
nothing, and a message it missed may still reach it later from another copy.  An origination at an
offline peer is an error (the engine refuses it).

Conventions of the counters the engine leaves open: ``scatter_words`` of a round counts the masks
pushed towards peers that are offline in the next round too (the push happens, the receiver
discards it) -- the sends churn did not drop, as in drop_ref.

late_ref, ttl_ref, drop_ref and policy_ref stay untouched as yardsticks; tests/test_down.py pins
this loop to them (no interval = drop_ref = late_ref) and to the reference's own Node objects
(tests/golden/down/*.npz).  Draws go through oracle.philox.
"""
import numpy as np

from drop_ref import DropResult, _sends, no_drop
from late_ref import COUNTERS, pad_equal  # noqa: F401  (re-exported for the tests)
from oracle import philox
from oracle.relay_oracle import _apply_changes, _round_stats

FOREVER = 0x7FFFFFFF


def offline(r, down_from, down_until):
    """bool [V]: the peers that are offline in round r."""
    f = np.asarray(down_from, dtype=np.int64)
    u = np.asarray(down_until, dtype=np.int64)
    return (f >= 0) & (f <= r) & (r < u)


def no_downtime(V):
    return np.full(V, -1, dtype=np.int32), np.full(V, FOREVER, dtype=np.int32)


def run(rowptr, colidx, src, start, down_from=None, down_until=None, drop=no_drop, mode="flood", fanout=3,
        gossip_seed=0, msg_id_base=0, churn_threshold=0, churn_seed=0, updates=None, max_rounds=1 << 20):
    """updates: {r: (add_pairs, remove_pairs)} -- connection changes after round r.
    drop: drop_ref's callback (the receipts whose relays are withdrawn: hop limits, a relay policy,
    p2pg_drop_relays); it is shown only receipts that happened."""
    updates = updates or {}
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
    res = DropResult(hop, parent, np.zeros(V, dtype=np.int64), np.zeros(V, dtype=np.int64))
    last = int(start.max()) if M else -1
    snd = tgt = msg = np.zeros(0, dtype=np.int64)  # the sends in flight (not lost)
    r = 0
    while r < max_rounds:
        # arrivals of round r (none at an offline peer: those sends were lost)
        new = np.zeros((V, M), dtype=bool)
        if len(tgt):
            assert not offline(r, down_from, down_until)[tgt].any()
            new[tgt, msg] = True
            new &= ~seen
            best = np.full((V, M), np.iinfo(np.int32).max, dtype=np.int64)
            np.minimum.at(best, (tgt, msg), snd)
            parent[new] = best[new]
            np.add.at(res.peer_recv, tgt, 1)
        received = len(tgt)
        origin = np.zeros((V, M), dtype=bool)
        due = np.nonzero(start == r)[0]
        origin[src[due], due] = True
        assert not (origin & seen).any()
        assert not offline(r, down_from, down_until)[src[due]].any(), "an origination at an offline peer"
        new |= origin
        seen |= new
        hop[new] = r
        gone = np.asarray(drop(r, new.copy()), dtype=bool)
        assert gone.shape == (V, M) and not (gone & ~new).any(), "only a first receipt can be dropped"
        live = new & ~gone
        per = np.minimum(deg, k) if gossip else np.maximum(deg - 1, 0)
        st = _round_stats(r, new, deg, per)
        offered = st["relays"]
        if not gossip:  # an origin has no sender to exclude
            offered += int(origin.sum(axis=1) @ (deg - np.maximum(deg - 1, 0)))
        st["relays"] = int((live.sum(axis=1) * per).sum())
        if not gossip:
            st["relays"] += int((origin & live).sum(axis=1) @ (deg - np.maximum(deg - 1, 0)))
        st["received"] = received
        res.relays_offered.append(int(offered))
        res.dropped.append(gone)
        # the sends of round r
        snd, tgt, msg = _sends(rowptr, colidx, r, live, parent, gossip, k, gossip_seed, msg_id_base)
        assert len(snd) == st["relays"], (r, len(snd), st["relays"])
        np.add.at(res.peer_sent, snd, 1)
        churned = philox.churn_dropped(r, snd, tgt, churn_threshold, churn_seed)
        churned = np.broadcast_to(np.asarray(churned, dtype=bool), snd.shape)
        lost = churned | offline(r + 1, down_from, down_until)[tgt]
        order = np.lexsort((msg, snd, tgt))
        res.sends.append((snd[order], tgt[order], msg[order], lost[order].copy()))
        if gossip and (~churned).any():  # (the masks towards offline receivers are pushed too)
            st["scatter_words"] = int(len(np.unique((snd[~churned] * V + tgt[~churned]) * W + msg[~churned] // 64)))
        keep = ~lost
        snd, tgt, msg = snd[keep], tgt[keep], msg[keep]
        res.rounds.append(st)
        if not new.any() and last <= r:
            break
        upd = updates.get(r)
        if upd is not None:  # sends on removed connections are lost; later sends use the new ones
            rm = np.asarray(upd[1], dtype=np.int64).reshape(-1, 2)
            cut = set(map(tuple, rm.tolist())) | set(map(tuple, rm[:, ::-1].tolist()))
            if len(tgt) and cut:
                keep = np.array([(int(a), int(b)) not in cut for a, b in zip(snd, tgt)], dtype=bool)
                snd, tgt, msg = snd[keep], tgt[keep], msg[keep]
            rowptr, colidx = _apply_changes(rowptr, colidx, upd[0], upd[1])
            deg = np.diff(rowptr)
        r += 1
    return res


# What every downtime fixture must hold, so none passes vacuously (tests/golden/make_down_golden.py
# asserts it when it writes them, tests/test_down.py from the data): a crash, a late joiner, a
# one-round and a multi-round outage, a (peer, message) lost while the peer was offline and received
# after its return from another sender at a later hop, one never received because of the downtime,
# an offline peer of degree >= 2 that two neighbours send to in one round, a gossip pick that hits
# an offline peer from a sender with deg > k, a peer whose row would have become full in a round it
# was offline in, and a message all of whose sends of one round are lost.
CENSUS = ("crash", "late_joiner", "one_round", "multi_round", "late_receipt", "never_received", "two_senders",
          "gossip_deg", "row_full", "all_lost")


def lost_to_downtime(z, res, r):
    """Of round r's send list: the sends churn let through and an offline receiver lost."""
    snd, tgt, msg, lost = res.sends[r]
    churned = philox.churn_dropped(r, snd, tgt, int(z["churn_threshold"]), int(z["churn_seed"]))
    churned = np.broadcast_to(np.asarray(churned, dtype=bool), snd.shape)
    return lost & ~churned


def census(z, res, full):
    """The census of one fixture: res = down_ref on its inputs, full = the same case without a
    downtime.  Returns {item: found}."""
    rowptr = z["rowptr"]
    hop, parent = res.hop, res.parent
    f, u = z["down_from"].astype(np.int64), z["down_until"].astype(np.int64)
    V, M = hop.shape
    deg = np.diff(rowptr)
    k = int(z["fanout"])
    got = dict.fromkeys(CENSUS, False)
    got["crash"] = bool(((f > 0) & (u == FOREVER)).any())
    got["late_joiner"] = bool(((f == 0) & (u < FOREVER)).any())
    got["one_round"] = bool(((f > 0) & (u - f == 1)).any())
    got["multi_round"] = bool(((f > 0) & (u - f >= 2) & (u < FOREVER)).any())
    for r in range(len(res.sends)):
        snd, tgt, msg, lost = res.sends[r]
        down = lost_to_downtime(z, res, r)
        if down.any():
            s, t, m = snd[down], tgt[down], msg[down]
            h = hop[t, m]
            got["late_receipt"] |= bool(((h > r + 1) & (h >= u[t]) & (parent[t, m] != s)).any())
            got["never_received"] |= bool(((h < 0) & (full.hop[t, m] >= 0)).any())
            got["gossip_deg"] |= bool((deg[s] > k).any())
            pairs = np.unique(np.stack([t, s], axis=1), axis=0)
            tt, cnt = np.unique(pairs[:, 0], return_counts=True)
            got["two_senders"] |= bool(((cnt >= 2) & (deg[tt] >= 2)).any())
            # a row that would have filled: everything seen before, plus what the peer missed now
            miss = np.zeros((V, M), dtype=bool)
            miss[t, m] = True
            before = (hop >= 0) & (hop <= r)
            got["row_full"] |= bool((miss.any(axis=1) & (before | miss).all(axis=1)).any())
        for mm in np.unique(msg):
            got["all_lost"] |= bool(lost[msg == mm].all())
    return got
