"""Relay withdrawal (p2pg_drop_relays) and the sends stream (p2pg_get_sends) on the GPU, at every
row width and after every push form, against tests/drop_ref.py (pinned on the CPU to late_ref,
ttl_ref and the per-bit stand-in, tests/test_drop_ref.py), bit for bit.

One driver steps a record / count_received / tally engine and, every round, reads the deliveries,
withdraws the relays of the receipts an arithmetic rule names (listed in descending order: the host
sorts) and reads the sends again: every counter of every round, every round's send list after the
drop (on a few rounds also before it), the deliveries, message_count_send, and at the end the
planes, the tallies and the per-peer counters.  Not compared, because the engine defines them for
itself: touched_words, the push_form of the rounds after a drop, the scatter_words of drop rounds.

The rule, in the drop rounds D: (v, m) iff (7 v + 13 m + r) % 3 == 0; round 3 also every message
of the last word (W = 1: the upper half of the only word) and every receipt of the max-degree peer;
round 4 also every receipt of the peers with v % 5 == 0 (drop_ref.issue_rule).  The conditions that
keep a case from passing vacuously are asserted on the reference (assert_not_vacuous)."""
import functools

import numpy as np
import pytest

import drop_ref
import ttl_ref
from test_gpu_late import assert_planes, dense_case, gpu_net
from test_gpu_ttl import assert_tallies

pytestmark = pytest.mark.gpu

CHURN = 430_000_000
GSEED, CSEED = 11, 5
KEYS = ("new_deliveries", "active_vertices", "active_words", "wedges", "deg_active", "received")


# ---- cases and their references ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_of(kind, n):
    """("dense", W): test_gpu_late's dense_case; ("hub", M): a 700-leaf star at peer 0 joined at
    peer 701 to the 30-peer ring 701..730 -- the hub's row (701 connections) is wider than the
    per-wave connection table; the hub, a leaf and a ring peer originate too."""
    from p2pnetwork.gpu import PeerGraph, make_sources
    if kind == "dense":
        g, M, src = dense_case(n)
        return g, M, np.asarray(src, dtype=np.int32)
    ring = list(range(701, 731))
    edges = [(0, i) for i in range(1, 702)] + list(zip(ring, ring[1:] + ring[:1]))
    g = PeerGraph.from_edges(731, np.array(edges, dtype=np.int32))
    assert int(g.degree().max()) == 701 and int(np.argmax(g.degree())) == 0
    src = make_sources(g.V, n, seed=6).astype(np.int32)
    src[:3] = (0, 5, 715)
    return g, n, src


@functools.lru_cache(maxsize=2)  # the push forms of one case run back to back
def reference(kind, n, mode, k, thr, D, thin=3, extras=True):
    """drop_ref on a case (computed once, shared, never written to) and its rule."""
    g, M, src = case_of(kind, n)
    rule = drop_ref.issue_rule(g.rowptr, M, D, thin, extras)
    ref = drop_ref.run(g.rowptr, g.colidx, src, np.zeros(M, dtype=np.int32), rule, mode, k, GSEED, 0, thr,
                       CSEED)
    for a in (ref.hop, ref.parent, ref.peer_sent, ref.peer_recv):
        a.setflags(write=False)
    return ref, rule


def words_of(b):
    """bool [V, M] -> bool [V, W]: the nonzero 64-message words of every row"""
    V, M = b.shape
    W = (M + 63) // 64
    pad = np.zeros((V, W * 64), dtype=bool)
    pad[:, :M] = b
    return pad.reshape(V, W, 64).any(axis=2)


def drop_facts(ref, r):
    """(some receipts dropped and some kept, a peer loses its whole row -- A bit set, F row zero --,
    a peer loses a whole word while keeping others -- its AW mask changes) of drop round r"""
    new, gone = ref.hop == r, ref.dropped[r]
    kept = new & ~gone
    nw, kw = words_of(new), words_of(kept)
    return (bool(gone.any() and kept.any()),
            bool((new.any(axis=1) & ~kept.any(axis=1)).any()),
            bool(((nw & ~kw).any(axis=1) & kw.any(axis=1)).any()))


def assert_not_vacuous(ref, D, W, mode, fixed=True, words=True):
    """Gossip: in every drop round (with D = {2, 3, 4, 6} no row is emptied in round 6 from W = 8
    up: every peer takes too many receipts there); flood: the row in round 4, the word in round 3.
    And the run goes on after the last drop.  fixed=False (drop rounds that follow the push forms
    or the graph, not the table's): a row is emptied in one of them at least -- the rounds of the
    dense forms are the ones in which every peer keeps some receipt."""
    facts = {r: drop_facts(ref, r) for r in sorted(D)}
    for r, (mixed, row, word) in facts.items():
        assert mixed, (r, "some receipts dropped and some kept")
        if not fixed:
            assert word or not words or W == 1, (r, "a peer loses a whole word while keeping others")
            continue
        if mode == "gossip":
            if not (r == 6 and W >= 8):
                assert row, (r, "a peer loses its whole row")
            if W > 1:
                assert word, (r, "a peer loses a whole word while keeping others")
        else:
            if r == 4:
                assert row, (r, "a peer loses its whole row")
            if r == 3 and W > 1:
                assert word, (r, "a peer loses a whole word while keeping others")
    if not fixed:
        assert any(row for _, row, _ in facts.values()), (facts, "a peer loses its whole row")
    after = sum(1 for x in ref.rounds[max(D) + 1:] if x["new_deliveries"])
    assert after >= (3 if mode == "gossip" else 2), after


# ---- the driver ------------------------------------------------------------------------------------
def assert_sends(s, want):
    snd, rcv, msg, lost = want
    np.testing.assert_array_equal(s.sender, snd)
    np.testing.assert_array_equal(s.receiver, rcv)
    np.testing.assert_array_equal(s.msg, msg)
    np.testing.assert_array_equal(s.lost, lost)


def drive(net, g, ref, rule, mode, k, thr, pre=(), before_drop=None, after_drop=None):
    """Step `net` (sources set) until it is quiet; every round against `ref`.  pre: the rounds whose
    sends are also read before the drop; before_drop / after_drop(net, r): a case's own calls."""
    rounds, sent = [], 0
    while True:
        st = net.step()
        r = st.round
        assert r == len(rounds) and r < len(ref.rounds), (r, len(ref.rounds))
        rounds.append(st)
        want = ref.rounds[r]
        for key in KEYS:
            assert getattr(st, key) == want[key], (r, key, getattr(st, key), want[key])
        assert st.relays == ref.relays_offered[r], (r, st.relays, ref.relays_offered[r])
        assert st.received_exact == 1
        new, gone = ref.hop == r, ref.dropped[r]
        if mode == "gossip" and not gone.any():
            assert st.scatter_words == want["scatter_words"], (r, st.scatter_words, want["scatter_words"])
        ahead = any(x["new_deliveries"] for x in ref.rounds[r + 1:])
        assert st.active == (1 if want["new_deliveries"] or ahead else 0), (r, st.active)
        d = net.deliveries()
        vs, ms = np.nonzero(new)  # ascending (peer, msg)
        np.testing.assert_array_equal(d.peer, vs)
        np.testing.assert_array_equal(d.msg, ms)
        assert (d.hop == r).all()
        np.testing.assert_array_equal(d.parent, ref.parent[vs, ms])
        if r in pre:  # the round's sends as they stand before the drop
            assert_sends(net.sends(), drop_ref.round_sends(g.rowptr, g.colidx, r, new, ref.parent, mode, k,
                                                           GSEED, 0, thr, CSEED))
        got = np.zeros_like(new)
        got[d.peer, d.msg] = True
        np.testing.assert_array_equal(rule(r, got), gone)  # the rule on the engine's own deliveries
        if before_drop is not None:
            before_drop(net, r)
        if gone.any():
            pv, pm = np.nonzero(gone)
            net.drop_relays(pv[::-1], pm[::-1])  # descending (peer, msg)
        if after_drop is not None:
            after_drop(net, r)
        assert_sends(net.sends(), ref.sends[r])
        sent += want["relays"]
        assert net.message_count_send == sent, (r, net.message_count_send, sent)
        if not st.active:
            break
    assert len(rounds) == len(ref.rounds), (len(rounds), len(ref.rounds))
    return rounds


def assert_end(net, ref):
    assert_planes(net, ref)   # hop_parent(), delivered()
    assert_tallies(net, ref)  # message_tally(), peer_counters(), message_reach()


def forms_of(rounds):
    from p2pnetwork.gpu.network import PUSH_FORMS
    return [PUSH_FORMS[x.push_form] for x in rounds]


def set_push(monkeypatch, push):
    if push != "auto":
        monkeypatch.setenv("P2PG_GOSSIP_PUSH", push)
    else:  # the thresholds at which a 600-peer graph reaches the dense forms (test_gpu_late)
        monkeypatch.setenv("P2PG_E_THRESH", "0.05")
        monkeypatch.setenv("P2PG_V_THRESH", "0.3")
        monkeypatch.setenv("P2PG_UPDATE_PUSH", "1")


def stepped(g, src, mode, k, thr, each=None):
    """The same engine stepped without drops: its rounds (and planes)."""
    with gpu_net(g, mode, k, GSEED, thr, CSEED, tally=True) as net:
        net.broadcast(src)
        rounds = []
        while True:
            rounds.append(net.step())
            if each is not None:
                each(net)
            if not rounds[-1].active:
                break
        return rounds, net.hop_parent(), net.seen_plane()


def auto_drop_rounds(forms):
    """The first round of each form present (atomic after round 0, edge / update_edge, fused), plus
    the round after the first of them."""
    firsts = set()
    for names in (("atomic",), ("edge", "update_edge"), ("fused",)):
        at = [i for i, f in enumerate(forms) if f in names and i > 0]
        if at:
            firsts.add(at[0])
    return tuple(sorted(firsts | {min(firsts) + 1}))


# ---- 1. gossip, dense: every width class x every push form ------------------------------------------
GOSSIP_SHAPES = [(W, 3) for W in (1, 3, 8, 9, 16, 17, 32, 64, 65)] + [(17, 2), (17, 5)]


@pytest.mark.parametrize("push", ["store", "atomic", "auto"])  # (varies fastest)
@pytest.mark.parametrize("W,k", GOSSIP_SHAPES)
def test_gossip_drops_match_drop_ref(W, k, push, monkeypatch):
    """Whole-row E (W <= 8), packed E with AW masks (8 < W <= 64), the 64-lane edge, two slices;
    fanout 2 and 5 at W = 17: the re-push's compile-time fanout instances and the generic one."""
    set_push(monkeypatch, push)
    g, M, src = case_of("dense", W)
    thr = CHURN if W % 2 else 0
    if push == "auto":
        base = forms_of(stepped(g, src, "gossip", k, thr)[0])
        D = auto_drop_rounds(base)
    else:
        D = (2, 3, 4, 6)
    ref, rule = reference("dense", W, "gossip", k, thr, D)
    assert_not_vacuous(ref, D, W, "gossip", fixed=push != "auto")
    with gpu_net(g, "gossip", k, GSEED, thr, CSEED, tally=True) as net:
        net.broadcast(src)
        rounds = drive(net, g, ref, rule, "gossip", k, thr, pre=(D[0], D[-1], D[-1] + 1))
        assert_end(net, ref)
    forms = forms_of(rounds)
    print(push, "W", W, "k", k, "churn", thr, "D", D, "push forms", forms,
          "dropped after", [forms[r] for r in D])
    live = [f for f, x in zip(forms, rounds) if x.new_deliveries]
    if push == "store":
        # rounds 2 and 6 are dropped after a fused round (W > 64: the unpacked fallback); 3 and 4
        # follow a drop, whose re-push by row atomics the next round takes in before it pushes
        # per connection again
        want = "fused" if W <= 64 else "edge"
        assert forms[0] == "edge" and forms[2] == want and forms[6] == want, forms
    elif push == "atomic":
        assert set(live) == {"atomic"}, forms
    else:  # the run is the base run up to its first drop
        assert forms[:D[0] + 1] == base[:D[0] + 1], (forms, base)
        assert {base[r] for r in D} >= set(base[1:]) - {"none"}, (D, base)  # every form is dropped after


# ---- 2. flood, dense ---------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [0, CHURN])
@pytest.mark.parametrize("W", [1, 9, 40, 65])
def test_flood_drops_match_drop_ref(W, thr):
    g, M, src = case_of("dense", W)
    D = (2, 3, 4)
    ref, rule = reference("dense", W, "flood", 3, thr, D)
    assert_not_vacuous(ref, D, W, "flood")
    with gpu_net(g, "flood", 3, GSEED, thr, CSEED, tally=True) as net:
        net.broadcast(src)
        drive(net, g, ref, rule, "flood", 3, thr, pre=(2, 4, 5))
        assert_end(net, ref)


# ---- 3. a row of 701 connections ----------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["flood", "gossip"])
@pytest.mark.parametrize("M", [70, 600])
def test_hub_row_above_512_drops_match_drop_ref(M, mode):
    """k_sends over a row wider than 512 connections, with lost flags, and the count-only pass
    behind `received`; the arithmetic rule alone, so the hub keeps relaying part of its receipts."""
    g, _, src = case_of("hub", M)
    D = (1, 2, 3)
    ref, rule = reference("hub", M, mode, 3, CHURN, D, 3, False)
    assert_not_vacuous(ref, D, (M + 63) // 64, mode, fixed=False, words=False)
    hub = [(int(ref.dropped[r][0].sum()), int(((ref.hop[0] == r) & ~ref.dropped[r][0]).sum())) for r in D]
    assert any(a and b for a, b in hub), hub  # the hub has dropped and kept receipts in one round
    assert any(lost[snd == 0].any() and not lost[snd == 0].all() for snd, _, _, lost in ref.sends)
    with gpu_net(g, mode, 3, GSEED, CHURN, CSEED, tally=True) as net:
        net.broadcast(src)
        rounds = drive(net, g, ref, rule, mode, 3, CHURN, pre=(0, 1, 2))
        assert_end(net, ref)
    print("hub M", M, mode, "hub receipts (dropped, kept) in", D, hub, "push forms", forms_of(rounds))


# ---- 4. an empty list changes nothing -----------------------------------------------------------------
def test_empty_drop_is_a_no_op(monkeypatch):
    set_push(monkeypatch, "store")
    g, M, src = case_of("dense", 17)
    base, planes, seen = stepped(g, src, "gossip", 3, CHURN)
    again, planes2, seen2 = stepped(g, src, "gossip", 3, CHURN, each=lambda net: net.drop_relays([], []))
    forms = forms_of(base)
    assert forms[0] == "edge" and set(forms[1:-1]) == {"fused"}, forms  # (it would force row pushes)
    assert again == base  # every field of every round: touched_words and push_form included
    for a, b in zip(planes + (seen,), planes2 + (seen2,)):
        np.testing.assert_array_equal(a, b)
    ref, rule = reference("dense", 17, "gossip", 3, CHURN, ())
    assert not any(x.any() for x in ref.dropped)
    with gpu_net(g, "gossip", 3, GSEED, CHURN, CSEED, tally=True) as net:
        net.broadcast(src)
        rounds = drive(net, g, ref, rule, "gossip", 3, CHURN, pre=(3,),
                       after_drop=lambda n, r: n.drop_relays([], []))
        assert_end(net, ref)
    assert forms_of(rounds) == forms


# ---- 5. refused lists change nothing --------------------------------------------------------------------
def test_refused_drops_after_a_fused_round_change_nothing(monkeypatch):
    from p2pnetwork.gpu import P2PGError
    set_push(monkeypatch, "store")
    W, D = 17, (2, 3, 4, 6)
    g, M, src = case_of("dense", W)
    ref, rule = reference("dense", W, "gossip", 3, CHURN, D)
    tried = []

    def refusals(net, r):
        if r not in (2, 6):
            return
        pv, pm = np.nonzero(ref.dropped[r])
        sent = net.message_count_send
        # a receipt of the round before (seen, no first receipt now) and a pair not delivered at all
        for bad in (np.argwhere(ref.hop == r - 1)[0], np.argwhere((ref.hop < 0) | (ref.hop > r))[-1]):
            with pytest.raises(P2PGError, match="bad argument"):
                net.drop_relays(np.append(pv, bad[0]), np.append(pm, bad[1]))
        with pytest.raises(P2PGError, match="bad argument"):  # a receipt listed twice
            net.drop_relays(np.append(pv, pv[3]), np.append(pm, pm[3]))
        assert net.message_count_send == sent
        tried.append(r)

    with gpu_net(g, "gossip", 3, GSEED, CHURN, CSEED, tally=True) as net:
        net.broadcast(src)
        rounds = drive(net, g, ref, rule, "gossip", 3, CHURN, pre=(2,), before_drop=refusals)
        assert_end(net, ref)
    forms = forms_of(rounds)
    assert tried == [2, 6] and forms[2] == "fused" and forms[6] == "fused", forms


# ---- 6. the per-peer counters between a drop and the next round ------------------------------------------
def test_peer_counters_right_after_a_drop(monkeypatch):
    from p2pnetwork.gpu import P2PGError
    set_push(monkeypatch, "store")
    W, D = 9, (2, 3, 4, 6)
    g, M, src = case_of("dense", W)
    ref, rule = reference("dense", W, "gossip", 3, CHURN, D)
    read = []

    def counters(net, r):
        if r != 3:
            return
        c = net.peer_counters()
        sent = sum(np.bincount(s[0], minlength=g.V) for s in ref.sends[:4])
        recv = sum(np.bincount(s[1][~s[3]], minlength=g.V) for s in ref.sends[:4])
        np.testing.assert_array_equal(c.sent, sent)
        np.testing.assert_array_equal(c.received, recv)
        kept = np.argwhere((ref.hop == 3) & ~ref.dropped[3])[0]
        with pytest.raises(P2PGError, match="bad state"):  # the round's sends are counted
            net.drop_relays([kept[0]], [kept[1]])
        read.append(r)

    with gpu_net(g, "gossip", 3, GSEED, CHURN, CSEED, tally=True) as net:
        net.broadcast(src)
        drive(net, g, ref, rule, "gossip", 3, CHURN, after_drop=counters)
        assert_end(net, ref)
    assert read == [3]


# ---- 7. the hop-limit rule by two device paths -------------------------------------------------------------
@pytest.mark.parametrize("W", [3, 17])
@pytest.mark.parametrize("mode", ["gossip", "flood"])
def test_ttl_by_set_ttl_and_by_drops(mode, W, monkeypatch):
    """k_expire / finalize_expiry (A: p2pg_set_ttl) and k_drop plus the re-push (B: no limits, the
    receipts at relative hop ttl[m] dropped every round) against ttl_ref and each other; the
    schedule of test_ttl_run_is_the_unlimited_run_cut_off."""
    set_push(monkeypatch, "store")
    g, M, src = case_of("dense", W)
    rng = np.random.default_rng(W)
    start = np.zeros(M, dtype=np.int32)
    start[rng.integers(0, M, max(M // 8, 1))] = 2
    ttl = np.array([3, 4, 6, -1, -1], dtype=np.int32)[rng.integers(0, 5, M)]
    lastw = np.arange(M) >= max(64 * (W - 1), 32)
    ttl[lastw] = 4 - start[lastw]
    cfg = (mode, 3, GSEED, 0, 0, CSEED)
    want = ttl_ref.run(g.rowptr, g.colidx, src, start, ttl, *cfg)
    rule = drop_ref.ttl_rule(start, ttl)
    ref = drop_ref.run(g.rowptr, g.colidx, src, start, rule, *cfg)
    assert ref.rounds == want.rounds and len(ref.sends) == len(want.sends)  # (as pinned on the CPU)
    np.testing.assert_array_equal(ref.hop, want.hop)
    assert sum(int(x.any()) for x in ref.dropped) >= 3
    total = int(want.column("relays").sum())
    # A: the limits on the device
    with gpu_net(g, mode, 3, GSEED, 0, CSEED, tally=True) as a:
        a.broadcast(src, start, ttl)
        lists = []
        while True:
            st = a.step()
            r = st.round
            assert st.new_deliveries == want.rounds[r]["new_deliveries"], r
            assert st.received == want.rounds[r]["received"], r
            assert len(a.deliveries()) == st.new_deliveries
            lists.append(a.sends())
            assert_sends(lists[-1], want.sends[r])
            if not st.active:
                break
        assert len(lists) == len(want.rounds) and a.message_count_send == total
        assert_end(a, want)
        planes_a, tally_a, count_a = a.hop_parent(), a.message_tally(), a.peer_counters()
    # B: the same rule as per-round drops
    with gpu_net(g, mode, 3, GSEED, 0, CSEED, tally=True) as b:
        b.broadcast(src, start)
        rounds = drive(b, g, ref, rule, mode, 3, 0, pre=(3, 4))
        assert b.message_count_send == total
        assert_end(b, want)
        for x, y in zip(planes_a + tuple(tally_a) + tuple(count_a),
                        b.hop_parent() + tuple(b.message_tally()) + tuple(b.peer_counters())):
            np.testing.assert_array_equal(x, y)
    print("ttl by drops", mode, "W", W, "push forms", forms_of(rounds))
