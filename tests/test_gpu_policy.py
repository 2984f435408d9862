"""The relay policy (p2pg_set_relay_policy) on the GPU: the engine, through the C-ABI, against the
policy/ fixtures of the reference's own Node objects, against tests/policy_ref.py as a drop_ref
rule (pinned to those fixtures on the CPU, tests/test_policy.py) and against the host route (a
second engine stepped with deliveries() and drop_relays() of exactly the muted receipts) --
bit-exact hop, parent, delivered set, send lists, tallies and every per-round counter but the three
a policy round defines for itself (its scatter_words and push_form, the next round's
touched_words)."""
import functools
import zlib

import numpy as np
import pytest

import drop_ref
import policy_ref
from test_gpu_late import assert_planes, gpu_net
from test_gpu_ttl import assert_rounds, assert_tallies
from test_policy import POLICY_CASES, load_policy, ref_of

pytestmark = pytest.mark.gpu

SILENT = 0xFFFFFFFF
THRS = np.array([0, SILENT, 1, 1 << 31, 0xFFFFFFFE], dtype=np.uint64)
CHURN = 430_000_000
ATOMIC, EDGE, FUSED = 1, 2, 3  # p2pg_round_stats.push_form


def mixed_thr(V, seed, weights=(0.4, 0.1, 0.1, 0.3, 0.1)):
    """Thresholds over all five kinds; peers 0 .. 4 carry one each whatever the draw."""
    thr = THRS[np.random.default_rng(seed).choice(len(THRS), V, p=weights)]
    thr[:5] = THRS
    return thr.astype(np.uint32)


def ref_run(g, src, start, thr, pseed, mode, k, gseed, cthr=0, cseed=0, ttl=None, updates=None, extra=None):
    rule = policy_ref.policy_rule(thr, pseed, start)
    if ttl is not None:
        rule = policy_ref.with_ttl(rule, start, ttl)
    if extra is not None:  # (round, peer, msg) receipts an app withdrew on top (drop_relays)
        inner = rule

        def rule(r, new):
            gone = inner(r, new)
            for rr, v, m in extra:
                if rr == r:
                    gone[v, m] = True
            return gone
    return drop_ref.run(g.rowptr, g.colidx, src, start, rule, mode, k, gseed, 0, cthr, cseed, updates=updates)


def policy_rounds(ref):
    """The rounds whose scatter_words the contract leaves to the engine: all but round 0."""
    return set(range(1, len(ref.rounds)))


def assert_sends(net, ref, r):
    s = net.sends()
    snd, rcv, msg, lost = ref.sends[r]
    np.testing.assert_array_equal(s.sender, snd)
    np.testing.assert_array_equal(s.receiver, rcv)
    np.testing.assert_array_equal(s.msg, msg)
    np.testing.assert_array_equal(s.lost, lost)


# ---- 1. the four fixtures of the reference's own Node objects -----------------------------------
@pytest.mark.parametrize("name", POLICY_CASES)
def test_policy_fixture_through_the_c_abi(name):
    z = load_policy(name)
    mode = str(z["mode"])
    cfg = (mode, int(z["fanout"]), int(z["gossip_seed"]), int(z["churn_threshold"]), int(z["churn_seed"]))
    ref = ref_of(name)
    with gpu_net(z, *cfg, record=True, tally=True) as net:
        net.broadcast(z["src"], z["start"], ttl=z["ttl"])
        net.set_relay_policy(thresholds=z["thr"], seed=int(z["policy_seed"]))
        rounds = net.run()
        hop, parent = net.hop_parent()
        np.testing.assert_array_equal(hop, z["hop"])
        np.testing.assert_array_equal(parent, z["parent"])
        np.testing.assert_array_equal(net.delivered(), z["hop"] >= 0)
        assert drop_ref.pad_equal([r.relays for r in rounds], z["round_relays"])
        assert net.message_count_send == int(z["round_relays"].sum())
        assert sum(r.received for r in rounds) == int(z["total_recv"])
        assert_rounds(rounds, ref, mode, policy_rounds(ref))
        assert_planes(net, ref)
        assert_tallies(net, ref)
        c = net.peer_counters()
        np.testing.assert_array_equal(c.sent, z["peer_sent"])
        np.testing.assert_array_equal(c.received, z["peer_recv"])
        # the send lists of every round, stepping the replay
        net.reset()
        for r in range(len(ref.rounds)):
            st = net.step()
            assert st.relays == ref.rounds[r]["relays"]
            assert_sends(net, ref, r)
        assert not st.active


# ---- 2. flood sweep against policy_ref ------------------------------------------------------------
FLOOD_CASES = [(V, M, thr) for V in (33, 200) for M in (1, 63, 64, 65, 130) for thr in (0, CHURN)]
FLOOD_CASES += [(40, 4160, 0), (40, 4160, CHURN)]


@pytest.mark.parametrize("V,M,cthr", FLOOD_CASES)
def test_policy_flood_matches_policy_ref(V, M, cthr):
    from p2pnetwork.gpu import PeerGraph, make_sources
    seed = zlib.crc32(repr((V, M, cthr)).encode()) & 0xFFFF
    g = PeerGraph.random_regular(V, 4, seed) if (V + M) % 2 else PeerGraph.gnp(V, 5.0, seed)
    rng = np.random.default_rng(seed)
    src = make_sources(g.V, M, seed=seed).astype(np.int32)
    start = rng.integers(0, 4, M).astype(np.int32)
    start[0] = 0 if M > 1 else 1
    thr = mixed_thr(g.V, seed)
    ref = ref_run(g, src, start, thr, seed + 3, "flood", 3, seed + 1, cthr, seed + 2)
    with gpu_net(g, "flood", 3, seed + 1, cthr, seed + 2, tally=True) as net:
        net.broadcast(src, start)
        net.set_relay_policy(thresholds=thr, seed=seed + 3)
        rounds = net.run()
        assert_rounds(rounds, ref, "flood", policy_rounds(ref))
        assert_planes(net, ref)
        assert_tallies(net, ref)
    assert any(x.any() for x in ref.dropped), "nothing was muted"


# ---- 3. gossip sweep: row widths x push forms -------------------------------------------------------
def gossip_case(W):
    """Every message from one of 20 origins (test_gpu_late.dense_case with fewer peers for the wide
    rows): a sparse start, then rounds in which every peer takes first receipts in most words."""
    from p2pnetwork.gpu import PeerGraph, make_sources
    g = PeerGraph.barabasi_albert(600 if W <= 17 else 160, 4, seed=40 + W)
    M = 64 * W - 5
    src = (make_sources(20, M, seed=W) * 7 + 3).astype(np.int32)
    start = np.zeros(M, dtype=np.int32)
    start[np.random.default_rng(W).integers(0, M, max(M // 8, 1))] = 2
    # mostly relaying peers, so the dense rounds are reached; every kind of threshold present
    thr = mixed_thr(g.V, W, (0.62, 0.05, 0.1, 0.18, 0.05))
    return g, src, start, thr


@functools.lru_cache(maxsize=None)
def gossip_ref(W):
    g, src, start, thr = gossip_case(W)
    return ref_run(g, src, start, thr, 77, "gossip", 3, 11, 0, 5)


@pytest.mark.parametrize("W", [1, 8, 9, 16, 17, 64, 65])
@pytest.mark.parametrize("push", ["atomic", "store", "auto"])
def test_policy_gossip_push_forms(W, push, monkeypatch):
    """Whole-row E (W <= 8), packed E with AW masks (8 < W <= 64), the 64-lane edge, two slices;
    the held-back push in both forms."""
    if push != "auto":
        monkeypatch.setenv("P2PG_GOSSIP_PUSH", push)
    else:  # the thresholds test_late_gossip_push_forms sets: small graphs enter dense rounds
        monkeypatch.setenv("P2PG_E_THRESH", "0.05")
        monkeypatch.setenv("P2PG_V_THRESH", "0.3")
        monkeypatch.setenv("P2PG_UPDATE_PUSH", "1")
    g, src, start, thr = gossip_case(W)
    ref = gossip_ref(W)
    with gpu_net(g, "gossip", 3, 11, 0, 5, tally=True) as net:
        net.broadcast(src, start)
        net.set_relay_policy(thresholds=thr, seed=77)
        rounds = net.run()
        assert_rounds(rounds, ref, "gossip", policy_rounds(ref))
        assert_planes(net, ref)
        assert_tallies(net, ref)
    forms = {r.push_form for r in rounds[1:] if r.new_deliveries}
    assert all(r.scatter_words == 0 for r in rounds[1:])
    assert forms <= {ATOMIC, EDGE}, forms  # never fused: every round after round 0 is a policy round
    if push == "atomic":
        assert forms == {ATOMIC}
    elif push == "store":
        assert forms == {EDGE}
    else:
        assert forms == {ATOMIC, EDGE}, [r.push_form for r in rounds]
    # without records, tallies or the lost count: the same receipts and relays
    with gpu_net(g, "gossip", 3, 11, 0, 5, record=False, count_received=False) as net:
        net.broadcast(src, start)
        net.set_relay_policy(thresholds=thr, seed=77)
        lean = net.run()
        np.testing.assert_array_equal(net.delivered(), ref.hop >= 0)
    assert [(x.new_deliveries, x.relays) for x in lean] == [(x.new_deliveries, x.relays) for x in rounds]


@pytest.mark.parametrize("push", ["atomic", "store"])
def test_policy_gossip_hub_row_under_churn(push, monkeypatch):
    """One row of 701 connections (above the hub threshold of the pull and push passes): a ring of
    702 peers with peer 0 connected to everyone."""
    from p2pnetwork.gpu import PeerGraph, make_sources
    monkeypatch.setenv("P2PG_GOSSIP_PUSH", push)
    V = 702
    g = PeerGraph.from_edges(V, [(i, (i + 1) % V) for i in range(V)] + [(0, j) for j in range(2, V - 1)])
    assert int(g.degree()[0]) == 701
    M = 70
    src = make_sources(V, M, seed=9).astype(np.int32)
    src[:3] = 0
    start = np.random.default_rng(9).integers(0, 3, M).astype(np.int32)
    for hub_thr in (1 << 31, SILENT):
        thr = mixed_thr(V, 9)
        thr[0] = hub_thr
        ref = ref_run(g, src, start, thr, 5, "gossip", 3, 11, CHURN, 6)
        with gpu_net(g, "gossip", 3, 11, CHURN, 6, tally=True) as net:
            net.broadcast(src, start)
            net.set_relay_policy(thresholds=thr, seed=5)
            rounds = net.run()
            assert_rounds(rounds, ref, "gossip", policy_rounds(ref))
            assert_planes(net, ref)
            assert_tallies(net, ref)
        assert any(x[0].any() for x in ref.dropped[1:]), "the hub muted nothing"


# ---- 4. self-consistency with the host route ------------------------------------------------------
@pytest.mark.parametrize("mode,cthr,M", [("flood", 0, 130), ("flood", CHURN, 70), ("gossip", 0, 130),
                                         ("gossip", CHURN, 1100)])
def test_policy_equals_the_host_route(mode, cthr, M):
    from p2pnetwork.gpu import PeerGraph, make_sources
    g = PeerGraph.barabasi_albert(300, 3, seed=31)
    src = make_sources(g.V, M, seed=31).astype(np.int32)
    start = np.random.default_rng(31).integers(0, 3, M).astype(np.int32)
    thr = mixed_thr(g.V, 31)
    with gpu_net(g, mode, 2, 13, cthr, 14) as net:
        net.broadcast(src, start)
        net.set_relay_policy(thresholds=thr, seed=99)
        dev = net.run()
        dev_seen = net.seen_plane()
        dev_hop, dev_parent = net.hop_parent()
    host_relays = []
    with gpu_net(g, mode, 2, 13, cthr, 14) as net:
        net.broadcast(src, start)
        while True:
            before = net.message_count_send
            st = net.step()
            if st.round > 0 and st.new_deliveries:
                d = net.deliveries()
                gone = policy_ref.muted(st.round, d.peer, d.msg, thr[d.peer], 99) & (start[d.msg] != st.round)
                net.drop_relays(d.peer[gone], d.msg[gone])
            host_relays.append(net.message_count_send - before)
            if not st.active:
                break
        np.testing.assert_array_equal(net.seen_plane(), dev_seen)
        hop, parent = net.hop_parent()
        np.testing.assert_array_equal(hop, dev_hop)
        np.testing.assert_array_equal(parent, dev_parent)
    assert [r.relays for r in dev] == host_relays


# ---- 5. interplay ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,cthr", [("flood", 0), ("flood", CHURN), ("gossip", 0), ("gossip", CHURN)])
def test_policy_run_equals_stepping_and_reset_replays(mode, cthr):
    from p2pnetwork.gpu import P2PGError, PeerGraph, make_sources
    g = PeerGraph.barabasi_albert(400, 3, seed=12)
    M = 130
    src = make_sources(g.V, M, seed=12).astype(np.int32)
    start = np.random.default_rng(12).integers(0, 4, M).astype(np.int32)
    thr = mixed_thr(g.V, 12)
    ref = ref_run(g, src, start, thr, 8, mode, 2, 31, cthr, 7)
    xs = policy_rounds(ref)
    with gpu_net(g, mode, 2, 31, cthr, 7) as net:
        net.broadcast(src, start)
        net.set_relay_policy(thresholds=thr, seed=8)
        assert_rounds(net.run(), ref, mode, xs)
        assert_planes(net, ref)
        for _ in range(2):  # reset keeps the policy and replays it
            net.reset()
            assert_rounds(net.run(), ref, mode, xs)
            assert_planes(net, ref)
        net.broadcast(src, start)  # new sources keep it too: it belongs to the peers
        assert_rounds(net.run(), ref, mode, xs)
        net.reset()
        stepped = []
        hop = np.full((g.V, M), -1, dtype=np.int32)
        parent = np.full((g.V, M), -1, dtype=np.int32)
        while True:
            st = net.step()
            stepped.append(st)
            d = net.deliveries()  # before finalisation: all the round's receipts, the muted included
            assert len(d) == st.new_deliveries and (d.hop == st.round).all()
            assert (hop[d.peer, d.msg] == -1).all()
            hop[d.peer, d.msg] = d.hop
            parent[d.peer, d.msg] = d.parent
            if st.round % 2 == 1:
                assert_sends(net, ref, st.round)
                if st.new_deliveries:
                    with pytest.raises(P2PGError, match="bad state"):  # after it: never a shortened list
                        net.deliveries()
            if not st.active:
                break
        assert_rounds(stepped, ref, mode, xs)
        np.testing.assert_array_equal(hop, ref.hop)
        np.testing.assert_array_equal(parent, ref.parent)
        assert_planes(net, ref)


@pytest.mark.parametrize("mode", ["flood", "gossip"])
def test_policy_update_edges_at_a_boundary(mode):
    from p2pnetwork.gpu import PeerGraph, make_sources
    g = PeerGraph.random_regular(300, 4, seed=14)
    M = 70
    src = make_sources(g.V, M, seed=14).astype(np.int32)
    start = np.random.default_rng(14).integers(0, 3, M).astype(np.int32)
    thr = mixed_thr(g.V, 14)
    probe = ref_run(g, src, start, thr, 4, mode, 2, 41)
    # after round 2: a peer that holds muted receipts of that round loses a connection and gains one
    a = int(np.nonzero(probe.dropped[2].any(axis=1))[0][0])
    b = int(g.neighbours(a)[0])
    c = next(x for x in range(g.V) if x != a and x not in set(g.neighbours(a).tolist()))
    rem = [(int(g.neighbours(v)[1]), v) for v in (10, 50) if a not in (v, int(g.neighbours(v)[1]))]
    updates = {2: (np.array([(a, c)], np.int32), np.array([(a, b)] + rem, np.int32))}
    ref = ref_run(g, src, start, thr, 4, mode, 2, 41, updates=updates)
    with gpu_net(g, mode, 2, 41, tally=True) as net:
        net.broadcast(src, start)
        net.set_relay_policy(thresholds=thr, seed=4)
        rounds = [net.step() for _ in range(3)]
        net.update_edges(add=updates[2][0], remove=updates[2][1])
        while rounds[-1].active:
            rounds.append(net.step())
        assert_rounds(rounds, ref, mode, policy_rounds(ref))
        assert_planes(net, ref)
        cnt = net.peer_counters()
        np.testing.assert_array_equal(cnt.sent, ref.peer_sent)
        np.testing.assert_array_equal(cnt.received, ref.peer_recv)


@pytest.mark.parametrize("mode", ["flood", "gossip"])
@pytest.mark.parametrize("final_first", [False, True])
def test_policy_drop_relays_at_a_boundary(mode, final_first):
    from p2pnetwork.gpu import PeerGraph, make_sources
    g = PeerGraph.random_regular(200, 5, seed=15)
    M = 66
    src = make_sources(g.V, M, seed=15).astype(np.int32)
    start = np.zeros(M, dtype=np.int32)
    thr = mixed_thr(g.V, 15)
    probe = ref_run(g, src, start, thr, 6, mode, 3, 51)
    new = probe.hop == 2
    dv, dm = (int(x[0]) for x in np.nonzero(probe.dropped[2]))   # a muted receipt of round 2
    lv, lm = (int(x[0]) for x in np.nonzero(new & ~probe.dropped[2]))  # one that relays
    ref = ref_run(g, src, start, thr, 6, mode, 3, 51, extra=[(2, lv, lm)])
    per = 4 if mode == "flood" else 3  # relays of one (non-origin) first receipt
    with gpu_net(g, mode, 3, 51) as net:
        net.broadcast(src, start)
        net.set_relay_policy(thresholds=thr, seed=6)
        rounds = [net.step() for _ in range(3)]
        assert rounds[2].relays == probe.rounds[2]["relays"]
        if final_first:
            net.sends()  # the round's sends are final: the muted bits are gone
        sent = net.message_count_send
        net.drop_relays([dv], [dm])
        assert net.message_count_send == sent  # legal, cancels nothing
        net.drop_relays([lv, dv], [lm, dm])
        assert sent - net.message_count_send == per
        assert_sends(net, ref, 2)
        st = net.step()
        assert st.received == ref.rounds[3]["received"]
        while st.active:
            st = net.step()
        assert_planes(net, ref)
        assert net.message_count_send == sum(x["relays"] for x in ref.rounds)


@pytest.mark.parametrize("mode", ["flood", "gossip"])
def test_policy_originate_wakes_a_quiet_engine(mode):
    from p2pnetwork.gpu import PeerGraph, make_sources
    g = PeerGraph.barabasi_albert(400, 3, seed=21)
    M = 70
    src = make_sources(g.V, M, seed=21).astype(np.int32)
    start = np.zeros(M, dtype=np.int32)
    src[[66, 67, 68]] = -1
    start[[66, 67, 68]] = -1
    thr = mixed_thr(g.V, 21)
    thr[5] = SILENT  # a silent origin still sends its own message
    with gpu_net(g, mode, 2, 31, tally=True) as net:
        net.set_relay_policy(thresholds=thr, seed=3)  # before the sources: it belongs to the peers
        net.broadcast(src, start)
        first = net.run()
        assert not first[-1].active
        quiet = len(first)
        net.originate([66, 67], [5, 9], round=quiet + 3)
        net.originate([68], [17])
        more = net.run()
        ref = ref_run(g, net.sources, net.start_rounds, thr, 3, mode, 2, 31)
        assert_rounds(first + more, ref, mode, policy_rounds(ref), check_active=False)
        assert_planes(net, ref)
        assert_tallies(net, ref)
        assert (ref.hop[:, 66] >= 0).sum() > 1
        net.reset()  # the schedule and the policy are replayed
        assert_rounds(net.run(), ref, mode, policy_rounds(ref))
        assert_planes(net, ref)


# ---- 6. no policy means no change ---------------------------------------------------------------------
def test_all_zero_thresholds_are_no_policy():
    from p2pnetwork.gpu import PeerGraph, make_sources
    g = PeerGraph.barabasi_albert(2000, 4, seed=3)
    src = make_sources(g.V, 4096, seed=3)
    out = []
    for how in ("never", "zeros", "ones", "removed"):
        with gpu_net(g, "gossip", 3, 0x5EED, record=False, count_received=False) as net:
            net.broadcast(src)
            if how == "zeros":
                net.set_relay_policy(thresholds=np.zeros(g.V, dtype=np.uint32), seed=5)
            elif how == "ones":
                net.set_relay_policy(1.0)
            elif how == "removed":
                net.set_relay_policy(0.5, seed=5)
                net.set_relay_policy(None)
            assert net.relay_thr is None
            rounds = net.run()
            assert len(net.snapshot()) > 0  # no policy: snapshots work
            out.append((rounds, net.seen_plane()))
    for rounds, seen in out[1:]:
        assert rounds == out[0][0]  # every field of every round, push_form included
        np.testing.assert_array_equal(seen, out[0][1])
    assert {r.push_form for r in out[0][0]} >= {ATOMIC, FUSED}  # fused rounds ran


@pytest.mark.parametrize("mode", ["flood", "gossip"])
def test_a_ttl_only_run_is_unchanged(mode):
    from p2pnetwork.gpu import PeerGraph, make_sources
    g = PeerGraph.barabasi_albert(600, 4, seed=4)
    M = 1100
    src = make_sources(g.V, M, seed=4)
    start = np.random.default_rng(4).integers(0, 3, M).astype(np.int32)
    ttl = np.array([2, 3, 5, -1], dtype=np.int32)[np.random.default_rng(5).integers(0, 4, M)]
    out = []
    for zeros in (False, True):
        with gpu_net(g, mode, 3, 0x5EED, CHURN, 9) as net:
            net.broadcast(src, start, ttl=ttl)
            if zeros:
                net.set_relay_policy(thresholds=np.zeros(g.V, dtype=np.uint32), seed=1)
            out.append((net.run(), net.seen_plane(), net.hop_parent()))
    assert out[0][0] == out[1][0]  # every field of every round
    np.testing.assert_array_equal(out[0][1], out[1][1])
    np.testing.assert_array_equal(out[0][2][1], out[1][2][1])


# ---- 7. refusals ---------------------------------------------------------------------------------------
def test_policy_refusals_leave_the_engine_unchanged():
    from p2pnetwork.gpu import P2PGError, PeerGraph, _lib
    g = PeerGraph.random_regular(200, 4, seed=16)
    src = np.array([1, 2, 7, 30], dtype=np.int32)
    start = np.array([0, 1, 0, 2], dtype=np.int32)
    thr = mixed_thr(g.V, 16)
    ref = ref_run(g, src, start, thr, 2, "flood", 3, 0)
    xs = policy_rounds(ref)
    L = _lib.lib()
    with gpu_net(g, "flood") as net:
        net.broadcast(src, start)
        net.set_relay_policy(thresholds=thr, seed=2)
        for bad in (thr[:-1], np.append(thr, 0)):  # a wrong V
            with pytest.raises(ValueError):
                net.set_relay_policy(thresholds=bad)
            b = np.ascontiguousarray(bad, dtype=np.uint32)
            assert L.p2pg_set_relay_policy(net._h, len(b), _lib.ptr(b), 0) == -1
        np.testing.assert_array_equal(net.relay_thr, thr)
        net.step_begin()
        with pytest.raises(P2PGError, match="bad state"):  # between step_begin / step_end
            net.set_relay_policy(0.5)
        r0 = net.step_end()
        assert r0.round == 0
        with pytest.raises(P2PGError, match="bad state"):  # once a round has run
            net.set_relay_policy(0.5)
        with pytest.raises(P2PGError, match="bad state"):
            net.set_relay_policy(None)
        with pytest.raises(P2PGError, match="bad state"):  # snapshots do not hold a policy
            net.snapshot()
        with pytest.raises(P2PGError, match="bad state"):
            net.restore(np.zeros(256, dtype=np.uint8))
        np.testing.assert_array_equal(net.relay_thr, thr)
        rounds = net.rounds[:]
        while rounds[-1].active:
            rounds.append(net.step())
        assert_rounds(rounds, ref, "flood", xs)
        assert_planes(net, ref)
        # after a reset the policy may change
        net.reset()
        net.set_relay_policy(0.0)
        net.set_relay_policy(thresholds=thr, seed=2)
        assert_rounds(net.run(), ref, "flood", xs)
        net.reset()
        net.set_relay_policy(None)
        assert net.relay_thr is None
        free = ref_run(g, src, start, np.zeros_like(thr), 2, "flood", 3, 0)
        assert_rounds(net.run(), free, "flood", set())
    # a vertex-partitioned rank
    with gpu_net(g, "flood", local_graph=True, count_received=False) as net:
        net.broadcast([1, 2])
        with pytest.raises(P2PGError, match="bad state"):
            net.set_relay_policy(0.5)
        assert net.relay_thr is None
    with gpu_net(g, "flood", count_received=False) as net:
        net.set_global_ids(np.arange(g.V, dtype=np.int32))
        net.broadcast([1, 2])
        with pytest.raises(P2PGError, match="bad state"):
            net.set_relay_policy(0.5)
    with gpu_net(g, "flood", count_received=False) as net:
        net.set_relay_policy(0.5)
        with pytest.raises(P2PGError, match="bad state"):  # ... and a rank cannot be made of it
            net.set_global_ids(np.arange(g.V, dtype=np.int32))
