"""Numpy restatement of the relay with per-message hop limits (test infrastructure only).

tests/late_ref.py plus one rule: message m carries ttl[m] >= 0, or -1 for unlimited.  A first
receipt of m in round r has relative hop h = r - start[m] (the origination is the receipt with
h = 0); it happens exactly as in late_ref -- seen, hop, parent, the receipt counters -- and makes
its sends iff ttl[m] < 0 or h < ttl[m].  A receipt with h == ttl[m] sends nothing: those sends are
in no counter, no peer's sent / received, no send list.  The run ends, as in late_ref, with the
first round that has no first receipt while no start lies ahead.

Pinned to the reference's own Node objects (a dedup app that forwards ``ttl - 1`` while
``ttl > 0``, node.py:106-116, README.md:20) by tests/golden/ttl/*.npz (tests/test_ttl.py); draws
through oracle.philox.  With every ttl -1 it is late_ref.run, round for round.

Why run() is a second loop and not a call of late_ref.run: the rule acts in the middle of a round
(between the receipts and their sends), late_ref.run has no hook there and is a yardstick that
stays as it is.  The loop below is late_ref's with the `alive` mask and the send lists added; its
result type, helpers and draws are late_ref's own, and test_ttl_ref_without_limits_is_late_ref
pins the two loops to each other.
"""
from dataclasses import dataclass, field

import numpy as np

from late_ref import COUNTERS, LateResult, pad_equal  # noqa: F401  (re-exported for the tests)
from oracle import philox
from oracle.relay_oracle import _apply_changes, _round_stats


@dataclass
class TtlResult(LateResult):
    # sends[r] = (sender, receiver, msg, lost) int64 / bool arrays of round r, sorted by
    # (receiver, sender, msg) -- p2pg_get_sends' order; lost = churn only
    sends: list = field(default_factory=list)


def run(rowptr, colidx, src, start, ttl, mode="flood", fanout=3, gossip_seed=0, msg_id_base=0,
        churn_threshold=0, churn_seed=0, updates=None, max_rounds=1 << 20):
    """updates: {r: (add_pairs, remove_pairs)} -- connection changes after round r."""
    updates = updates or {}
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colidx = np.asarray(colidx, dtype=np.int64)
    src = np.asarray(src, dtype=np.int64)
    start = np.asarray(start, dtype=np.int64)
    ttl = np.asarray(ttl, dtype=np.int64)
    V, M = len(rowptr) - 1, len(src)
    assert ttl.shape == (M,) and (ttl >= -1).all()
    W = (M + 63) // 64
    k = int(fanout)
    gossip = mode == "gossip"
    deg = np.diff(rowptr)
    hop = np.full((V, M), -1, dtype=np.int32)
    parent = np.full((V, M), -1, dtype=np.int32)
    seen = np.zeros((V, M), dtype=bool)
    res = TtlResult(hop, parent, np.zeros(V, dtype=np.int64), np.zeros(V, dtype=np.int64))
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
        # the receipts that still send: relative hop below the message's hop limit
        alive = (ttl < 0) | (r - start < ttl)
        live = new & alive[None, :]
        per = np.minimum(deg, k) if gossip else np.maximum(deg - 1, 0)
        st = _round_stats(r, new, deg, per)
        st["relays"] = int((live.sum(axis=1) * per).sum())
        if not gossip:  # an origin has no sender to exclude
            st["relays"] += int((origin & live).sum(axis=1) @ (deg - np.maximum(deg - 1, 0)))
        st["received"] = received
        # the sends of round r
        vs, ms = np.nonzero(live)
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
        lost = philox.churn_dropped(r, snd, tgt, churn_threshold, churn_seed)
        lost = np.broadcast_to(np.asarray(lost, dtype=bool), snd.shape)
        order = np.lexsort((msg, snd, tgt))
        res.sends.append((snd[order], tgt[order], msg[order], lost[order].copy()))
        keep = ~lost
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


def cut_at_ttl(hop, parent, start, ttl):
    """The prefix property: the planes of an unlimited run with every receipt of relative hop above
    ttl[m] blanked are the planes of the run with those hop limits."""
    start = np.asarray(start, dtype=np.int64)[None, :]
    ttl = np.asarray(ttl, dtype=np.int64)[None, :]
    keep = (hop >= 0) & ((ttl < 0) | (hop - start <= ttl))
    return np.where(keep, hop, -1).astype(np.int32), np.where(keep, parent, -1).astype(np.int32)
