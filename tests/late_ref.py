"""Numpy restatement of the relay with per-message start rounds (test infrastructure only).

Message m originates at src[m] in round start[m] (-1: never).  Round r: the sends of round r-1
that were not lost arrive first (dedup, lowest-id sender = parent), then every m with
start[m] == r originates at src[m] -- a first receipt of round r with parent -1 -- and every
first receipt of the round sends: flood to all connections but the parent (all of them at an
origin), gossip to the min(k, deg) Philox picks of (r, peer, msg_id_base + m).  A send of round
r is lost iff churn_dropped(r, sender, receiver), or its connection is removed by an update at
the r / r+1 boundary.  The run ends with the first round that has no first receipt while no
start lies ahead (the engine's last round).

Pinned to the reference's own Node objects by tests/golden/late/*.npz (tests/test_late.py);
draws through oracle.philox.
"""
from dataclasses import dataclass, field

import numpy as np

from oracle import philox
from oracle.relay_oracle import _apply_changes, _round_stats

COUNTERS = ("new_deliveries", "relays", "active_vertices", "active_words", "wedges", "deg_active",
            "scatter_words", "received")


@dataclass
class LateResult:
    hop: np.ndarray
    parent: np.ndarray
    peer_sent: np.ndarray
    peer_recv: np.ndarray
    rounds: list = field(default_factory=list)

    def column(self, key):
        return np.array([r[key] for r in self.rounds], dtype=np.int64)


def run(rowptr, colidx, src, start, mode="flood", fanout=3, gossip_seed=0, msg_id_base=0,
        churn_threshold=0, churn_seed=0, updates=None, max_rounds=1 << 20):
    """updates: {r: (add_pairs, remove_pairs)} -- connection changes after round r."""
    updates = updates or {}
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colidx = np.asarray(colidx, dtype=np.int64)
    src = np.asarray(src, dtype=np.int64)
    start = np.asarray(start, dtype=np.int64)
    V, M = len(rowptr) - 1, len(src)
    W = (M + 63) // 64
    k = int(fanout)
    gossip = mode == "gossip"
    deg = np.diff(rowptr)
    hop = np.full((V, M), -1, dtype=np.int32)
    parent = np.full((V, M), -1, dtype=np.int32)
    seen = np.zeros((V, M), dtype=bool)
    res = LateResult(hop, parent, np.zeros(V, dtype=np.int64), np.zeros(V, dtype=np.int64))
    last = int(start.max()) if M else -1
    snd = tgt = msg = np.zeros(0, dtype=np.int64)  # the sends in flight (not lost)
    r = 0
    while r < max_rounds:
        # arrivals of round r
        new = np.zeros((V, M), dtype=bool)
        if len(tgt):
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
        new |= origin
        seen |= new
        hop[new] = r
        per = np.minimum(deg, k) if gossip else np.maximum(deg - 1, 0)
        st = _round_stats(r, new, deg, per)
        if not gossip:  # an origin has no sender to exclude
            st["relays"] += int(origin.sum(axis=1) @ (deg - np.maximum(deg - 1, 0)))
        st["received"] = received
        # the sends of round r
        vs, ms = np.nonzero(new)
        d = deg[vs]
        if gossip:
            small = d <= k
            rep = np.repeat(np.nonzero(small)[0], d[small])  # every connection
            off = np.arange(len(rep)) - np.repeat(np.cumsum(d[small]) - d[small], d[small])
            s_l, t_l, m_l = [vs[rep]], [colidx[rowptr[vs[rep]] + off]], [ms[rep]]
            big = ~small
            if big.any():
                pk = philox.gossip_picks(r, vs[big], ms[big] + msg_id_base, d[big], k, gossip_seed)
                t_l.append(colidx[rowptr[vs[big]][:, None] + pk].ravel())
                s_l.append(np.repeat(vs[big], k))
                m_l.append(np.repeat(ms[big], k))
            snd, tgt, msg = (np.concatenate(x).astype(np.int64) for x in (s_l, t_l, m_l))
        else:
            rep = np.repeat(np.arange(len(vs)), d)
            off = np.arange(len(rep)) - np.repeat(np.cumsum(d) - d, d)
            snd, msg = vs[rep], ms[rep]
            tgt = colidx[rowptr[snd] + off]
            keep = tgt != parent[snd, msg]
            snd, tgt, msg = snd[keep], tgt[keep], msg[keep]
        assert len(snd) == st["relays"], (r, len(snd), st["relays"])
        np.add.at(res.peer_sent, snd, 1)
        keep = ~philox.churn_dropped(r, snd, tgt, churn_threshold, churn_seed)
        snd, tgt, msg = snd[keep], tgt[keep], msg[keep]
        if gossip and len(tgt):
            st["scatter_words"] = int(len(np.unique((snd * V + tgt) * W + msg // 64)))
        res.rounds.append(st)
        if not new.any() and last <= r:
            break
        upd = updates.get(r)
        if upd is not None:  # sends on removed connections are lost; later sends use the new ones
            rm = np.asarray(upd[1], dtype=np.int64).reshape(-1, 2)
            gone = set(map(tuple, rm.tolist())) | set(map(tuple, rm[:, ::-1].tolist()))
            if len(tgt) and gone:
                keep = np.array([(int(a), int(b)) not in gone for a, b in zip(snd, tgt)], dtype=bool)
                snd, tgt, msg = snd[keep], tgt[keep], msg[keep]
            rowptr, colidx = _apply_changes(rowptr, colidx, upd[0], upd[1])
            deg = np.diff(rowptr)
        r += 1
    return res


def pad_equal(a, b):
    """Two per-round columns are equal up to trailing zeros."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    n = max(len(a), len(b))
    return np.array_equal(np.pad(a, (0, n - len(a))), np.pad(b, (0, n - len(b))))
