"""Numpy restatement of the relay with withdrawn relays (test infrastructure only).

tests/ttl_ref.py with its one rule generalised: instead of a message-wide hop limit, a callback
``drop(r, new) -> bool [V, M]`` is shown the first receipts of round r (originations included) and
returns the ones whose relays are withdrawn -- an app whose node_message did not forward them
(p2pg_drop_relays).  A dropped receipt still happens: seen, hop, parent and the receipt counters
are as without the drop; it makes no sends, exactly like a receipt at its hop limit in ttl_ref --
those sends are in no counter, no peer's sent / received, no send list.  The run ends, as in
late_ref, with the first round that has no first receipt while no start lies ahead.

late_ref and ttl_ref stay untouched as yardsticks; the loop below is ttl_ref's with the `alive`
mask replaced by the per-receipt one, and tests/test_drop_ref.py pins it to both (no drops =
late_ref; drops at relative hop ttl[m] = ttl_ref) and to the per-bit stand-in of
tests/partition_mock.py.  Draws go through oracle.philox.
"""
from dataclasses import dataclass, field

import numpy as np

from late_ref import COUNTERS, pad_equal  # noqa: F401  (re-exported for the tests)
from oracle import philox
from oracle.relay_oracle import _apply_changes, _round_stats
from ttl_ref import TtlResult


@dataclass
class DropResult(TtlResult):
    # per round: the relays before the drop (what the engine's step() reports; rounds[r]["relays"]
    # and sends[r] are the ones after it) and the bool [V, M] mask of the dropped receipts
    relays_offered: list = field(default_factory=list)
    dropped: list = field(default_factory=list)


def no_drop(r, new):
    return np.zeros_like(new)


def ttl_rule(start, ttl):
    """The drop rule that restates hop limits: the receipts at relative hop ttl[m]."""
    start, ttl = np.asarray(start, dtype=np.int64), np.asarray(ttl, dtype=np.int64)
    return lambda r, new: new & (r - start == ttl)[None, :]


def _sends(rowptr, colidx, r, live, parent, gossip, k, gossip_seed, msg_id_base):
    """(sender, receiver, msg) of every send the receipts `live` of round r make (ttl_ref's)."""
    deg = np.diff(rowptr)
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
        return tuple(np.concatenate(x).astype(np.int64) for x in (s_l, t_l, m_l))
    rep = np.repeat(np.arange(len(vs)), d)
    off = np.arange(len(rep)) - np.repeat(np.cumsum(d) - d, d)
    snd, msg = vs[rep], ms[rep]
    tgt = colidx[rowptr[snd] + off]
    keep = tgt != parent[snd, msg]  # not back to the sender (an origin has none: parent -1)
    return snd[keep], tgt[keep], msg[keep]


def round_sends(rowptr, colidx, r, live, parent, mode="flood", fanout=3, gossip_seed=0, msg_id_base=0,
                churn_threshold=0, churn_seed=0):
    """The send list (sender, receiver, msg, lost), in p2pg_get_sends' order, that the first
    receipts `live` of round r make over the given connections -- with a run's receipts of round r
    (hop == r) and its parent plane: that round's sends before any drop."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colidx = np.asarray(colidx, dtype=np.int64)
    snd, tgt, msg = _sends(rowptr, colidx, r, live, parent, mode == "gossip", int(fanout), gossip_seed,
                           msg_id_base)
    lost = philox.churn_dropped(r, snd, tgt, churn_threshold, churn_seed)
    lost = np.broadcast_to(np.asarray(lost, dtype=bool), snd.shape)
    order = np.lexsort((msg, snd, tgt))
    return snd[order], tgt[order], msg[order], lost[order].copy()


def run(rowptr, colidx, src, start, drop=no_drop, mode="flood", fanout=3, gossip_seed=0, msg_id_base=0,
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
    res = DropResult(hop, parent, np.zeros(V, dtype=np.int64), np.zeros(V, dtype=np.int64))
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
        # the receipts that still send: the ones the callback does not withdraw
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
            cut = set(map(tuple, rm.tolist())) | set(map(tuple, rm[:, ::-1].tolist()))
            if len(tgt) and cut:
                keep = np.array([(int(a), int(b)) not in cut for a, b in zip(snd, tgt)], dtype=bool)
                snd, tgt, msg = snd[keep], tgt[keep], msg[keep]
            rowptr, colidx = _apply_changes(rowptr, colidx, upd[0], upd[1])
            deg = np.diff(rowptr)
        r += 1
    return res


def issue_rule(rowptr, M, drop_rounds, thin=3, extras=True):
    """The deterministic rule of the GPU tests: in the rounds `drop_rounds`, (v, m) is dropped iff
    (7 v + 13 m + r) % thin == 0; with `extras`, round 3 also drops every message of the last word
    (W = 1: the upper half of the only word) and every receipt of the max-degree peer, round 4
    every receipt of the peers with v % 5 == 0."""
    deg = np.diff(np.asarray(rowptr, dtype=np.int64))
    V = len(deg)
    W = (M + 63) // 64
    v = np.arange(V, dtype=np.int64)[:, None]
    m = np.arange(M, dtype=np.int64)[None, :]
    hub = int(np.argmax(deg))
    drop_rounds = frozenset(int(x) for x in drop_rounds)

    def rule(r, new):
        if r not in drop_rounds:
            return np.zeros_like(new)
        gone = (7 * v + 13 * m + r) % thin == 0
        if extras and r == 3:
            gone = gone | (m >= max(64 * (W - 1), 32)) | (v == hub)
        if extras and r == 4:
            gone = gone | (v % 5 == 0)
        return new & gone
    return rule
