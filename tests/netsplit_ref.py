"""Numpy restatement of the relay with a network partition that heals (test infrastructure only).

The rule of p2pg_set_netsplit: every peer has a side, ``side[v] >= 0``, and there is one window of
rounds ``[cut_from, cut_until)``.  Connection {a, b} is cut in round t iff ``side[a] != side[b]`` and
``cut_from <= t < cut_until``.  Peers keep their connections and go on sending over a cut one; a
send made in round r from a to b -- a relay packet, an anti-entropy request or a reply -- is lost iff
it was lost before (churn, a receiver that is offline in r + 1) or {a, b} is cut in round r + 1, the
round it would arrive in.  A lost send is counted by its sender and is no arrival.

tests/pull_ref.py is the loop (arrivals, originations, replies, requests; downtime; anti-entropy) and
stays untouched.  Every send it makes passes one test, its churn draw ``(r, a, b)``, and "cut in
r + 1" is a function of exactly those three; so this file runs that loop with the draw replaced by
``churn draw or cut in r + 1`` -- nothing else differs -- and adds what the tallies report: the
per-message cost (cost_ref, from the send lists) and the latency histograms (latency_ref, from the hop
plane).  ``scatter_words`` of a gossip round whose sends arrive in a cut round is the engine's own
and not restated.  tests/test_netsplit.py pins this file to pull_ref / down_ref (equal sides) and to
the reference's own Node objects (tests/golden/netsplit/*.npz).
"""
import contextlib

import numpy as np

import cost_ref
import latency_ref
import pull_ref
from oracle import philox
from pull_ref import FOREVER, RECORD, no_downtime, offline, pad_equal  # noqa: F401  (re-exported for the tests)


def link_cut(t, side_a, side_b, cut_from, cut_until):
    """Is a connection between peers of side_a and side_b cut in round t?  (Arrays broadcast.)"""
    t = np.asarray(t, dtype=np.int64)
    return (np.asarray(side_a) != np.asarray(side_b)) & (cut_from <= t) & (t < cut_until)


def cut_round(t, cut_from, cut_until):
    return cut_from <= t < cut_until


class _CutDraw:
    """oracle.philox with churn_dropped = the churn draw or "cut in the arrival round"."""

    def __init__(self, side, cut_from, cut_until):
        self.side, self.cut_from, self.cut_until = np.asarray(side, dtype=np.int64), int(cut_from), int(cut_until)
        self.calls = 0  # (run() checks that the loop still draws through this object)

    def __getattr__(self, name):
        return getattr(philox, name)

    def churn_dropped(self, r, a, b, threshold, seed):
        self.calls += 1
        ch = np.asarray(philox.churn_dropped(r, a, b, threshold, seed), dtype=bool)
        a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
        cut = link_cut(np.asarray(r, dtype=np.int64) + 1, self.side[a], self.side[b], self.cut_from, self.cut_until)
        return ch | cut


@contextlib.contextmanager
def _draw(obj):
    keep = pull_ref.philox
    pull_ref.philox = obj
    try:
        yield
    finally:
        pull_ref.philox = keep


def run(rowptr, colidx, src, start, side=None, cut_from=0, cut_until=0, bins=64, **kw):
    """pull_ref.run's arguments plus the netsplit; returns its PullResult with, in addition,
    msg_sent / msg_recv (uint64 [M], when the send lists are kept) and latency
    (latency_ref.Latency).  side = None, equal sides or an empty window: pull_ref.run itself."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colidx = np.asarray(colidx, dtype=np.int64)
    V = len(rowptr) - 1
    on = side is not None and cut_from < cut_until
    if on:
        side = np.asarray(side, dtype=np.int64)
        assert side.shape == (V,) and (side >= 0).all() and cut_from >= 0
        on = bool((side[np.repeat(np.arange(V), np.diff(rowptr))] != side[colidx]).any())
    if on:
        draw = _CutDraw(side, cut_from, cut_until)
        with _draw(draw):
            res = pull_ref.run(rowptr, colidx, src, start, **kw)
        # one draw per round's relay sends at least: a pull_ref that stopped drawing through its
        # module-level philox would run without the cut, and must not do so silently
        assert draw.calls >= len(res.rounds), (draw.calls, len(res.rounds))
    else:
        res = pull_ref.run(rowptr, colidx, src, start, **kw)
    M = len(np.asarray(src))
    if kw.get("planes", True):
        res.msg_sent, res.msg_recv = cost_ref.message_cost(res.sends, M)
    res.latency = latency_ref.latency(res.hop, np.asarray(start, dtype=np.int64), bins)
    res.received_total = int(sum(r["received"] for r in res.rounds))
    return res


def lost_to_cut(res, r, side, cut_from, cut_until, churn_threshold=0, churn_seed=0, down_from=None, down_until=None):
    """Of round r's send list: the sends lost to the cut alone -- churn let them through and their
    receiver is online in r + 1."""
    snd, tgt, msg, lost = res.sends[r]
    ch = np.broadcast_to(np.asarray(philox.churn_dropped(r, snd, tgt, churn_threshold, churn_seed), dtype=bool), snd.shape)
    off = np.zeros(len(snd), dtype=bool) if down_from is None else offline(r + 1, down_from, down_until)[tgt]
    cut = link_cut(r + 1, np.asarray(side)[snd], np.asarray(side)[tgt], cut_from, cut_until)
    assert not (cut & ~lost).any()
    return cut & ~ch & ~off


# What the netsplit fixtures must hold between them, so none passes vacuously
# (tests/golden/make_netsplit_golden.py asserts it when it writes them, tests/test_netsplit.py from the
# data): a send lost to the cut alone; a message that never reaches another side without
# anti-entropy; one that crosses after the heal by an ordinary relay (a first receipt or a start at
# r >= cut_until - 1 at a border peer); a first receipt whose parent is a same-side sender while a
# lower-id other-side sender's copy was cut in that round; a request and a reply lost to the cut; a
# receipt repaired across the healed cut; a gossip pick wasted on a cut connection by a hub with
# degree > 64.
CENSUS = ("cut_alone", "never_crosses", "crosses_by_relay", "parent_same_side", "request_cut", "reply_cut",
          "repaired_across", "hub_pick_wasted")


def census(z, res, nopull):
    """The census of one fixture: res = run() on its inputs, nopull = the same case without
    anti-entropy.  Returns {item: found}."""
    rowptr, colidx = np.asarray(z["rowptr"], dtype=np.int64), np.asarray(z["colidx"], dtype=np.int64)
    side = np.asarray(z["side"], dtype=np.int64)
    cf, cu = int(z["cut_from"]), int(z["cut_until"])
    f, u_ = z["down_from"], z["down_until"]
    cthr, cseed = int(z["churn_threshold"]), int(z["churn_seed"])
    gossip, k = str(z["mode"]) == "gossip", int(z["fanout"])
    setting = tuple(int(x) for x in z["anti_entropy"])
    deg = np.diff(rowptr)
    V, M = res.hop.shape
    got = dict.fromkeys(CENSUS, False)
    src = np.asarray(z["src"], dtype=np.int64)
    # sides a message reaches without anti-entropy
    reach = nopull.hop >= 0
    for m in range(M):
        sides = set(side[reach[:, m]].tolist())
        got["never_crosses"] |= len(sides) < len(set(side.tolist())) and bool(reach[:, m].any())
    for r in range(len(res.rounds)):
        alone = lost_to_cut(res, r, side, cf, cu, cthr, cseed, f, u_)
        got["cut_alone"] |= bool(alone.any())
        snd, tgt, msg, lost = res.sends[r]
        if gossip and alone.any():
            got["hub_pick_wasted"] |= bool((deg[snd[alone]] > np.maximum(64, k)).any())
        # a send that crosses sides and arrives in a round after the heal
        cross = (side[snd] != side[tgt]) & ~lost & (r + 1 >= cu)
        if cross.any():
            first = (res.hop[tgt[cross], msg[cross]] == r + 1) & (res.parent[tgt[cross], msg[cross]] == snd[cross])
            got["crosses_by_relay"] |= bool(first.any())
        # a cut copy from a lower-id sender, and the receipt made in that round from a same-side one
        cut = link_cut(r + 1, side[snd], side[tgt], cf, cu)
        if cut.any():
            t, m, s = tgt[cut], msg[cut], snd[cut]
            par = res.parent[t, m].astype(np.int64)
            hit = (res.hop[t, m] == r + 1) & (par >= 0) & (par > s)
            hit &= side[np.maximum(par, 0)] == side[t]
            got["parent_same_side"] |= bool(hit.any())
        if pull_ref.request_round(r, setting):
            uu = np.nonzero((deg > 0) & ~offline(r, f, u_))[0]
            p = colidx[rowptr[uu] + pull_ref.partner_slot(r, uu, deg[uu], int(z["pull_seed"]))]
            ch1 = np.broadcast_to(np.asarray(philox.churn_dropped(r, uu, p, cthr, cseed), dtype=bool), uu.shape)
            off1 = offline(r + 1, f, u_)[p]
            c1 = link_cut(r + 1, side[uu], side[p], cf, cu)
            got["request_cut"] |= bool((c1 & ~ch1 & ~off1).any())
            ok = ~(ch1 | off1 | c1)
            ch2 = np.broadcast_to(np.asarray(philox.churn_dropped(r + 1, p[ok], uu[ok], cthr, cseed), dtype=bool),
                                  uu[ok].shape)
            off2 = offline(r + 2, f, u_)[uu[ok]]
            c2 = link_cut(r + 2, side[p[ok]], side[uu[ok]], cf, cu)
            got["reply_cut"] |= bool((c2 & ~ch2 & ~off2).any())
        pulled, pp = res.pulled[r], res.partner[r]
        if pulled.any() and r >= cu:
            us, ms = np.nonzero(pulled)
            got["repaired_across"] |= bool((side[pp[us]] != side[us]).any())
    return got


def flood_packed(rowptr, colidx, src, start, side=None, cut_from=0, cut_until=0, churn_threshold=0, churn_seed=0,
                 max_rounds=1 << 20):
    """The flood under a netsplit on packed rows, for cases too large for run()'s per-send arrays
    (no downtime, no anti-entropy): a copy v -> u of round r - 1 arrives in round r iff churn did not
    drop (r - 1, {v, u}) and {v, u} is not cut in r, so the arrivals of a round are one OR over the
    connections that let their copy through.  Returns (hop int32 [V][M], rounds: the list of
    per-round dicts with new_deliveries, relays, active_vertices, active_words, wedges, deg_active).
    tests/test_netsplit.py pins it to run()."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colidx = np.asarray(colidx, dtype=np.int64)
    src = np.asarray(src, dtype=np.int64)
    start = np.asarray(start, dtype=np.int64)
    V, M = len(rowptr) - 1, len(src)
    W = (M + 63) // 64
    deg = np.diff(rowptr)
    rcv = np.repeat(np.arange(V), deg)
    snd = colidx
    if side is None:
        side = np.zeros(V, dtype=np.int64)
    side = np.asarray(side, dtype=np.int64)
    crossing = side[rcv] != side[snd]
    hop = np.full((V, M), -1, dtype=np.int32)
    seen = np.zeros((V, W), dtype=np.uint64)
    prev = np.zeros((V, W), dtype=np.uint64)
    rounds = []
    last = int(start.max()) if M else -1
    r = 0
    while r < max_rounds:
        arr = np.zeros((V, W), dtype=np.uint64)
        if r > 0 and prev.any():
            keep = prev[snd].any(axis=1)
            keep &= ~(crossing & cut_round(r, cut_from, cut_until))
            ch = np.asarray(philox.churn_dropped(r - 1, snd, rcv, churn_threshold, churn_seed), dtype=bool)
            keep &= ~np.broadcast_to(ch, snd.shape)
            np.bitwise_or.at(arr, rcv[keep], prev[snd[keep]])
        new = arr & ~seen
        origin = np.zeros((V, W), dtype=np.uint64)
        due = np.nonzero(start == r)[0]
        np.bitwise_or.at(origin, (src[due], due // 64), np.uint64(1) << (due % 64).astype(np.uint64))
        assert not (origin & (seen | new)).any()
        new |= origin
        seen |= new
        bits = np.unpackbits(new.view(np.uint8).reshape(V, W * 8), axis=1, bitorder="little")[:, :M].astype(bool)
        hop[bits] = r
        per_row = bits.sum(axis=1)
        words = new != 0
        obits = np.unpackbits(origin.view(np.uint8).reshape(V, W * 8), axis=1, bitorder="little")[:, :M].sum(axis=1)
        rounds.append(dict(
            new_deliveries=int(per_row.sum()),
            relays=int((per_row * np.maximum(deg - 1, 0)).sum() + (obits * (deg - np.maximum(deg - 1, 0))).sum()),
            active_vertices=int((per_row > 0).sum()), active_words=int(words.sum()),
            wedges=int((words.sum(axis=1) * deg).sum()), deg_active=int(deg[per_row > 0].sum())))
        prev = new
        if not new.any() and last <= r:
            break
        r += 1
    return hop, rounds
