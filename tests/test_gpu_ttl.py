"""Hop limits (p2pg_set_ttl) on the GPU: the engine, through the C-ABI, against the ttl/ fixtures of
the reference's own Node objects, against tests/ttl_ref.py (pinned to those fixtures on the CPU,
tests/test_ttl.py) and against itself (the prefix property: a run with hop limits is the unlimited
run cut off at relative hop ttl[m]) -- bit-exact hop, parent, delivered set, send lists, tallies
and every per-round counter but the three an expiry round defines for itself (its scatter_words
and push_form, the next round's touched_words)."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import ttl_ref
from test_gpu_late import FLOOD_KEYS, assert_planes, dense_case, gpu_net
from test_ttl import TTL, TTL_CASES, load_ttl, ref_of

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TTLS = np.array([0, 1, 2, 3, 4, 6, -1], dtype=np.int32)


def expiry_rounds(start, ttl):
    start, ttl = np.asarray(start, dtype=np.int64), np.asarray(ttl, dtype=np.int64)
    return set((start + ttl)[(ttl >= 0) & (start >= 0)].tolist())


def assert_rounds(rounds, ref, mode, expiries, check_active=True, exact=True):
    """Every counter of every round (the engine may not stop earlier or later than the reference);
    scatter_words outside the expiry rounds.  exact=False: a churn run without count_received
    reports the sends of the round before as `received`."""
    assert len(rounds) == len(ref.rounds), (len(rounds), len(ref.rounds))
    for i, (a, b) in enumerate(zip(rounds, ref.rounds)):
        assert a.round == i and a.received_exact == (1 if exact else 0)
        for k in FLOOD_KEYS:
            want = b[k] if exact or k != "received" else (ref.rounds[i - 1]["relays"] if i else 0)
            assert getattr(a, k) == want, (i, k, getattr(a, k), want)
        if mode == "gossip" and i not in expiries:
            assert a.scatter_words == b["scatter_words"], (i, a.scatter_words, b["scatter_words"])
        ahead = any(r["new_deliveries"] for r in ref.rounds[i + 1:])
        if check_active:
            assert a.active == (1 if b["new_deliveries"] or ahead else 0), (i, a.active)


def assert_tallies(net, ref):
    got = ref.hop >= 0
    t = net.message_tally()
    np.testing.assert_array_equal(t.reach, got.sum(axis=0))
    np.testing.assert_array_equal(t.hop_sum, np.where(got, ref.hop, 0).sum(axis=0))
    np.testing.assert_array_equal(t.last_hop, ref.hop.max(axis=0))
    c = net.peer_counters()
    np.testing.assert_array_equal(c.sent, ref.peer_sent)
    np.testing.assert_array_equal(c.received, ref.peer_recv)
    np.testing.assert_array_equal(net.message_reach(), got.sum(axis=0))


# ---- 1. the four fixtures of the reference's own Node objects -----------------------------------
@pytest.mark.parametrize("name", TTL_CASES)
def test_ttl_fixture_through_the_c_abi(name):
    z = load_ttl(name)
    mode = str(z["mode"])
    cfg = (mode, int(z["fanout"]), int(z["gossip_seed"]), int(z["churn_threshold"]), int(z["churn_seed"]))
    ref = ref_of(name)
    xs = expiry_rounds(z["start"], z["ttl"])
    with gpu_net(z, *cfg, record=True, tally=True) as net:
        net.broadcast(z["src"], z["start"], ttl=z["ttl"])
        np.testing.assert_array_equal(net.ttl, z["ttl"])
        rounds = net.run()
        hop, parent = net.hop_parent()
        np.testing.assert_array_equal(hop, z["hop"])
        np.testing.assert_array_equal(parent, z["parent"])
        np.testing.assert_array_equal(net.delivered(), z["hop"] >= 0)
        assert ttl_ref.pad_equal([r.relays for r in rounds], z["round_relays"])
        assert net.message_count_send == int(z["round_relays"].sum())
        assert sum(r.received for r in rounds) == int(z["total_recv"])
        assert_rounds(rounds, ref, mode, xs)
        t = net.message_tally()
        got = z["hop"] >= 0
        np.testing.assert_array_equal(t.reach, got.sum(axis=0))
        np.testing.assert_array_equal(t.hop_sum, np.where(got, z["hop"], 0).sum(axis=0))
        np.testing.assert_array_equal(t.last_hop, z["hop"].max(axis=0))
        c = net.peer_counters()
        np.testing.assert_array_equal(c.sent, z["peer_sent"])
        np.testing.assert_array_equal(c.received, z["peer_recv"])
        np.testing.assert_array_equal(net.message_reach(), got.sum(axis=0))


# ---- 2. randomised against ttl_ref ---------------------------------------------------------------
def make_graph(kind, seed):
    from p2pnetwork.gpu import PeerGraph
    if kind == "rrg":
        return PeerGraph.random_regular(300, 4, seed)
    if kind == "ws":
        return PeerGraph.watts_strogatz(400, 6, 0.1, seed)
    if kind == "gnp":  # mean degree 2.5: isolated peers and several components
        return PeerGraph.gnp(400, 2.5, seed)
    if kind == "hub":  # ring of 600, peer 0 connected to 520 others (deg > HUB_T = 512)
        V = 600
        return PeerGraph.from_edges(V, [(i, (i + 1) % V) for i in range(V)] + [(0, j) for j in range(2, 521)])
    return PeerGraph.barabasi_albert(500, 3, seed)


def make_schedule(g, M, seed):
    """Mixed starts 0..4 and hop limits from TTLS; where M allows: a ttl-0 message, an unlimited
    one, two messages of one word and one origin with different limits, a hub origin with ttl 1
    and a leaf origin with ttl 2, an isolated origin."""
    from p2pnetwork.gpu import make_sources
    rng = np.random.default_rng(seed)
    src = make_sources(g.V, M, seed=seed).astype(np.int32)
    start = rng.integers(0, 5, M).astype(np.int32)
    ttl = TTLS[rng.integers(0, len(TTLS), M)]
    if M == 1:
        return src, np.array([1], np.int32), np.array([2], np.int32)
    ttl[0], ttl[1], start[0] = 0, -1, 0
    deg = g.degree()
    if M >= 8:
        src[2] = src[3]
        start[2] = start[3] = 1
        ttl[2], ttl[3] = 1, 3
        src[4], ttl[4], start[4] = int(np.argmax(deg)), 1, 2  # a hub
        src[5], ttl[5], start[5] = int(np.argmin(np.where(deg > 0, deg, 1 << 30))), 2, 0  # a leaf
        iso = np.nonzero(deg == 0)[0]
        if len(iso):
            src[6], ttl[6], start[6] = iso[0], 3, 1
        ttl[7], start[7] = 0, 3  # a ttl-0 origination after round 0
    return src, start, ttl


RANDOM_CASES = [
    # kind, mode, k, churn threshold, M, count_received
    ("rrg", "flood", 3, 0, 1, True),
    ("rrg", "gossip", 2, 0, 1, True),
    ("rrg", "flood", 3, 430_000_000, 70, True),
    ("rrg", "flood", 3, 0, 1100, False),
    ("ba", "flood", 3, 0, 200, True),
    ("ba", "gossip", 3, 0, 70, True),
    ("ba", "gossip", 2, 430_000_000, 200, True),
    ("ba", "gossip", 3, 430_000_000, 70, False),
    ("ba", "gossip", 3, 0, 1100, True),
    ("ws", "flood", 3, 430_000_000, 200, False),
    ("ws", "gossip", 1, 0, 200, True),
    ("gnp", "flood", 3, 0, 70, True),
    ("gnp", "gossip", 3, 430_000_000, 200, True),
    ("hub", "flood", 3, 0, 70, True),
    ("hub", "gossip", 3, 0, 70, True),
]


@pytest.mark.parametrize("kind,mode,k,thr,M,count", RANDOM_CASES)
def test_ttl_random_matches_ttl_ref(kind, mode, k, thr, M, count):
    seed = zlib.crc32(repr((kind, mode, k, thr, M)).encode()) & 0xFFFF
    g = make_graph(kind, seed)
    src, start, ttl = make_schedule(g, M, seed)
    ref = ttl_ref.run(g.rowptr, g.colidx, src, start, ttl, mode, k, seed + 1, 0, thr, seed + 2)
    with gpu_net(g, mode, k, seed + 1, thr, seed + 2, count_received=count, tally=True) as net:
        net.broadcast(src, start, ttl)
        rounds = net.run()
        assert_rounds(rounds, ref, mode, expiry_rounds(start, ttl), exact=count or thr == 0)
        assert_planes(net, ref)
        assert_tallies(net, ref)


# ---- 3. the prefix property against the engine itself, gossip push forms ---------------------------
def run_gossip(g, src, start, ttl, k=3, gseed=11):
    with gpu_net(g, "gossip", k, gseed, 0, 5) as net:
        net.broadcast(src, start, ttl)
        rounds = net.run()
        hop, parent = net.hop_parent()
    return rounds, hop, parent


@pytest.mark.parametrize("W", [1, 3, 16, 17, 64, 65])
@pytest.mark.parametrize("push", ["store", "auto", "atomic"])
def test_ttl_run_is_the_unlimited_run_cut_off(W, push, monkeypatch):
    """Whole-row E (W <= 8), packed E with AW masks (8 < W <= 64), the 64-lane edge, two slices;
    dense rounds reached on a 600-peer graph by the thresholds test_late_gossip_push_forms sets."""
    if push != "auto":
        monkeypatch.setenv("P2PG_GOSSIP_PUSH", push)
    else:
        monkeypatch.setenv("P2PG_E_THRESH", "0.05")
        monkeypatch.setenv("P2PG_V_THRESH", "0.3")
        monkeypatch.setenv("P2PG_UPDATE_PUSH", "1")
    g, M, src = dense_case(W)
    rng = np.random.default_rng(W)
    start = np.zeros(M, dtype=np.int32)
    start[rng.integers(0, M, max(M // 8, 1))] = 2
    # limits 3, 4, 6 and unlimited: the first expiry is round 3, in the dense phase; several words
    # lose some of their messages in one round, the last word all of them in round 4
    ttl = np.array([3, 4, 6, -1, -1], dtype=np.int32)[rng.integers(0, 5, M)]
    lastw = np.arange(M) >= max(64 * (W - 1), 32)  # (W = 1: the upper half of the only word)
    ttl[lastw] = 4 - start[lastw]
    base, hop0, par0 = run_gossip(g, src, start, None)
    rounds, hop, parent = run_gossip(g, src, start, ttl)
    want_hop, want_par = ttl_ref.cut_at_ttl(hop0, par0, start, ttl)
    np.testing.assert_array_equal(hop, want_hop)
    np.testing.assert_array_equal(parent, want_par)
    assert (hop != hop0).any(), "no limit cut anything"
    first = min(expiry_rounds(start, ttl))
    assert first == 3
    for key in FLOOD_KEYS + ("scatter_words", "touched_words", "push_form"):
        assert [getattr(x, key) for x in rounds[:first]] == [getattr(x, key) for x in base[:first]], key
    # new_deliveries of every round: the unlimited run's receipts within the limits
    for r, x in enumerate(rounds):
        assert x.new_deliveries == int((want_hop == r).sum()), r
    if push == "store" and W in (3, 16, 17, 64):
        assert 3 in {x.push_form for x in base}, [x.push_form for x in base]  # fused rounds ran
    # without records, tallies or the lost count p2pg_run may skip frontier rows and batch rounds
    # wherever no expiry stands in the way: the same receipts and relays
    with gpu_net(g, "gossip", 3, 11, 0, 5, record=False, count_received=False) as net:
        net.broadcast(src, start, ttl)
        lean = net.run()
        np.testing.assert_array_equal(net.delivered(), want_hop >= 0)
    assert [(x.new_deliveries, x.relays) for x in lean] == [(x.new_deliveries, x.relays) for x in rounds]


# ---- 4. run() vs stepping, reset, deliveries and sends of expiry rounds -------------------------------
@pytest.mark.parametrize("mode,thr", [("flood", 0), ("flood", 430_000_000), ("gossip", 0), ("gossip", 430_000_000)])
def test_ttl_run_equals_stepping_and_reset_replays(mode, thr):
    from p2pnetwork.gpu import P2PGError, PeerGraph
    g = PeerGraph.barabasi_albert(400, 3, seed=12)
    M = 130
    src, start, ttl = make_schedule(g, M, 12)
    ref = ttl_ref.run(g.rowptr, g.colidx, src, start, ttl, mode, 2, 31, 0, thr, 7)
    xs = expiry_rounds(start, ttl)
    with gpu_net(g, mode, 2, 31, thr, 7) as net:
        net.broadcast(src, start, ttl)
        ran = net.run()
        assert_rounds(ran, ref, mode, xs)
        assert_planes(net, ref)
        for _ in range(2):  # reset keeps the limits and replays them
            net.reset()
            assert_rounds(net.run(), ref, mode, xs)
            assert_planes(net, ref)
        net.reset()
        stepped = []
        hop = np.full((g.V, M), -1, dtype=np.int32)
        parent = np.full((g.V, M), -1, dtype=np.int32)
        while True:
            st = net.step()
            stepped.append(st)
            d = net.deliveries()  # first: an expiry round's deliveries hold its expired receipts
            assert len(d) == st.new_deliveries and (d.hop == st.round).all()
            assert (hop[d.peer, d.msg] == -1).all()
            hop[d.peer, d.msg] = d.hop
            parent[d.peer, d.msg] = d.parent
            if st.round in xs or st.round % 3 == 0:
                s = net.sends()
                snd, rcv, msg, lost = ref.sends[st.round]
                np.testing.assert_array_equal(s.sender, snd)
                np.testing.assert_array_equal(s.receiver, rcv)
                np.testing.assert_array_equal(s.msg, msg)
                np.testing.assert_array_equal(s.lost, lost)
                if st.round in xs and st.new_deliveries:
                    with pytest.raises(P2PGError, match="bad state"):  # never a shortened list
                        net.deliveries()
            if not st.active:
                break
        assert_rounds(stepped, ref, mode, xs)
        np.testing.assert_array_equal(hop, ref.hop)  # nothing is missing in an expiry round
        np.testing.assert_array_equal(parent, ref.parent)
        assert_planes(net, ref)


# ---- 5. all -1 is no hop limit ----------------------------------------------------------------------
def test_all_minus_one_is_no_ttl():
    from p2pnetwork.gpu import PeerGraph, make_sources
    g = PeerGraph.barabasi_albert(2000, 4, seed=3)
    src = make_sources(g.V, 4096, seed=3)
    out = []
    for ttl in (None, np.full(4096, -1, dtype=np.int32), "removed"):
        with gpu_net(g, "gossip", 3, 0x5EED, record=False, count_received=False) as net:
            if isinstance(ttl, str):
                net.broadcast(src, ttl=np.full(4096, 2, dtype=np.int32))
                net.set_ttl(None)
            else:
                net.broadcast(src, ttl=ttl)
            rounds = net.run()
            assert len(net.snapshot()) > 0  # no finite limit: snapshots work
            out.append((rounds, net.seen_plane()))
    for rounds, seen in out[1:]:
        assert rounds == out[0][0]  # every field of every round, push_form included
        np.testing.assert_array_equal(seen, out[0][1])
    assert {r.push_form for r in out[0][0]} >= {1, 3}  # fused rounds ran


# ---- 6. across round boundaries -----------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["flood", "gossip"])
def test_ttl_update_edges_after_an_expiry_round(mode):
    from p2pnetwork.gpu import PeerGraph, make_sources
    g = PeerGraph.random_regular(300, 4, seed=14)
    M = 70
    src = make_sources(g.V, M, seed=14).astype(np.int32)
    start = np.random.default_rng(14).integers(0, 3, M).astype(np.int32)
    ttl = TTLS[np.random.default_rng(15).integers(0, len(TTLS), M)]
    start[:6] = 0
    ttl[:3] = 2  # expire in round 2, right before the update
    ttl[3:6] = -1
    # after round 2: a peer that holds expired receipts of message 0 loses a connection and gains one
    probe = ttl_ref.run(g.rowptr, g.colidx, src, start, ttl, mode, 2, 41)
    a = int(np.nonzero(probe.hop[:, 0] == 2)[0][0])
    b = int(g.neighbours(a)[0])
    c = next(x for x in range(g.V) if x != a and x not in set(g.neighbours(a).tolist()))
    rem = [(int(g.neighbours(v)[1]), v) for v in (10, 50) if a not in (v, int(g.neighbours(v)[1]))]
    updates = {2: (np.array([(a, c)], np.int32), np.array([(a, b)] + rem, np.int32))}
    ref = ttl_ref.run(g.rowptr, g.colidx, src, start, ttl, mode, 2, 41, updates=updates)
    with gpu_net(g, mode, 2, 41, tally=True) as net:
        net.broadcast(src, start, ttl)
        rounds = [net.step() for _ in range(3)]
        net.update_edges(add=updates[2][0], remove=updates[2][1])
        while rounds[-1].active:
            rounds.append(net.step())
        assert_rounds(rounds, ref, mode, expiry_rounds(start, ttl))
        assert_planes(net, ref)
        c = net.peer_counters()
        np.testing.assert_array_equal(c.sent, ref.peer_sent)
        np.testing.assert_array_equal(c.received, ref.peer_recv)


@pytest.mark.parametrize("mode", ["flood", "gossip"])
def test_drop_relays_in_an_expiry_round(mode):
    from p2pnetwork.gpu import PeerGraph
    g = PeerGraph.random_regular(200, 5, seed=15)
    src = np.array([3, 9, 40], dtype=np.int32)
    start = np.array([0, 0, 1], dtype=np.int32)
    ttl = np.array([2, -1, 1], dtype=np.int32)  # 0 and 2 expire in round 2
    ref = ttl_ref.run(g.rowptr, g.colidx, src, start, ttl, mode, 3, 51)
    per = 4 if mode == "flood" else 3  # relays of one (non-origin) first receipt
    with gpu_net(g, mode, 3, 51) as net:
        net.broadcast(src, start, ttl)
        rounds = [net.step() for _ in range(3)]
        assert rounds[2].relays == ref.rounds[2]["relays"]
        d = net.deliveries()
        dead = np.nonzero(d.msg == 0)[0][0]   # an expired receipt
        live = np.nonzero(d.msg == 1)[0][0]   # a live one
        sent = net.message_count_send
        net.drop_relays([d.peer[dead]], [0])
        assert net.message_count_send == sent  # legal, cancels nothing
        net.drop_relays([d.peer[live], d.peer[dead]], [1, 0])  # ... also once the sends are final
        assert sent - net.message_count_send == per
        nxt = net.step()
        assert nxt.received == rounds[2].relays - per
        while nxt.active:
            nxt = net.step()
        got = net.delivered()
        np.testing.assert_array_equal(got[:, [0, 2]], ref.hop[:, [0, 2]] >= 0)  # cut at their limits
        # (the live message goes on without the withdrawn relays; a gossip may then take other ways)
        assert got[:, 1].sum() > 1 and (mode == "gossip" or got[:, 1].sum() <= (ref.hop[:, 1] >= 0).sum())


# ---- 7. an unscheduled message with a hop limit ------------------------------------------------------
@pytest.mark.parametrize("mode", ["flood", "gossip"])
def test_ttl_of_an_unscheduled_message_started_after_the_run_went_quiet(mode):
    from p2pnetwork.gpu import PeerGraph, make_sources
    g = PeerGraph.barabasi_albert(400, 3, seed=21)
    M = 70
    src = make_sources(g.V, M, seed=21).astype(np.int32)
    start = np.zeros(M, dtype=np.int32)
    ttl = np.full(M, 3, dtype=np.int32)
    ttl[::7] = -1
    src[[66, 67, 68]] = -1
    start[[66, 67, 68]] = -1
    ttl[[66, 67, 68]] = [2, 0, -1]
    with gpu_net(g, mode, 2, 31, tally=True) as net:
        net.broadcast(src, start, ttl)
        first = net.run()
        assert not first[-1].active
        quiet = len(first)
        net.originate([66, 67], [5, 9], round=quiet + 3)
        net.originate([68], [17])
        more = net.run()
        ref = ttl_ref.run(g.rowptr, g.colidx, net.sources, net.start_rounds, ttl, mode, 2, 31)
        xs = expiry_rounds(net.start_rounds, ttl)
        assert quiet + 5 in xs and quiet + 3 in xs
        assert_rounds(first + more, ref, mode, xs, check_active=False)
        assert_planes(net, ref)
        assert_tallies(net, ref)
        assert (ref.hop[:, 67] >= 0).sum() == 1 and (ref.hop[:, 66] - (quiet + 3)).max() == 2
        net.reset()  # the schedule and the limits are replayed
        assert_rounds(net.run(), ref, mode, xs)
        assert_planes(net, ref)


# ---- 8. one-block grids: k_expire's grid-stride loop -------------------------------------------------
CHILD = r"""
import os, sys
sys.path[:0] = [%r, %r]
import numpy as np
from p2pnetwork.gpu import GraphNetwork, PeerGraph
for name in %r:
    with np.load(os.path.join(%r, name + ".npz"), allow_pickle=False) as f:
        z = {k: f[k] for k in f.files}
    with GraphNetwork(PeerGraph(z["rowptr"], z["colidx"]), mode=str(z["mode"]), fanout=int(z["fanout"]),
                      gossip_seed=int(z["gossip_seed"]), churn_threshold_value=int(z["churn_threshold"]),
                      churn_seed=int(z["churn_seed"]), record=True, count_received=True, tally=True) as net:
        net.broadcast(z["src"], z["start"], ttl=z["ttl"])
        rounds = net.run()
        hop, parent = net.hop_parent()
        c = net.peer_counters()
    assert np.array_equal(hop, z["hop"]) and np.array_equal(parent, z["parent"]), name
    assert [r.relays for r in rounds if r.relays] == [int(x) for x in z["round_relays"] if x], name
    assert sum(r.received for r in rounds) == int(z["total_recv"]), name
    assert np.array_equal(c.sent, z["peer_sent"]) and np.array_equal(c.received, z["peer_recv"]), name
print("ok")
"""


def test_ttl_single_block_grid():
    """P2PG_GRID_MAX is read once per process, so a child: one block = 4 waves over the 7-10
    32-peer tasks of the fixtures' graphs."""
    env = dict(os.environ, P2PG_GRID_MAX="1")
    code = CHILD % (REPO, os.path.join(REPO, "python-p2p-network_amd"), TTL_CASES, TTL)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.strip().endswith("ok")


# ---- 9. refusals ------------------------------------------------------------------------------------
def test_ttl_refusals_leave_the_engine_unchanged():
    from p2pnetwork.gpu import P2PGError, PeerGraph, _lib
    g = PeerGraph.random_regular(200, 4, seed=16)
    src = np.array([1, 2, 7, 30], dtype=np.int32)
    start = np.array([0, 1, 0, 2], dtype=np.int32)
    ttl = np.array([2, 3, -1, 0], dtype=np.int32)
    ref = ttl_ref.run(g.rowptr, g.colidx, src, start, ttl, "flood")
    xs = expiry_rounds(start, ttl)
    L = _lib.lib()
    with gpu_net(g, "flood") as net:
        with pytest.raises(RuntimeError):
            net.set_ttl(ttl)  # no sources yet
        assert L.p2pg_set_ttl(net._h, 4, _lib.ptr(ttl)) == -2
        net.broadcast(src, start, ttl)
        for bad in ([2, 3, -2, 0], [2, 3, -1, (1 << 30) + 1]):
            with pytest.raises(P2PGError, match="bad argument"):
                net.set_ttl(bad)
        for bad in ([2, 3, -1], [2, 3, -1, 0, 0]):  # wrong M
            with pytest.raises(P2PGError, match="bad argument"):
                net.set_ttl(bad)
        np.testing.assert_array_equal(net.ttl, ttl)
        net.step_begin()
        with pytest.raises(P2PGError, match="bad state"):  # between step_begin / step_end
            net.set_ttl([1, 1, 1, 1])
        r0 = net.step_end()
        assert r0.round == 0
        with pytest.raises(P2PGError, match="bad state"):  # once a round has run
            net.set_ttl([1, 1, 1, 1])
        with pytest.raises(P2PGError, match="bad state"):  # snapshots do not hold hop limits
            net.snapshot()
        with pytest.raises(P2PGError, match="bad state"):
            net.restore(np.zeros(256, dtype=np.uint8))
        rounds = net.rounds[:]
        while rounds[-1].active:
            rounds.append(net.step())
        assert_rounds(rounds, ref, "flood", xs)
        assert_planes(net, ref)
        # after a reset the limits may change; new sources clear them
        net.reset()
        net.set_ttl([-1, -1, -1, 1 << 30])
        net.set_ttl(ttl)
        assert_rounds(net.run(), ref, "flood", xs)
        net.broadcast(src, start)
        assert (net.ttl == -1).all()
        full = ttl_ref.run(g.rowptr, g.colidx, src, start, np.full(4, -1), "flood")
        assert_rounds(net.run(), full, "flood", set())
    # a vertex-partitioned rank
    with gpu_net(g, "flood", local_graph=True, count_received=False) as net:
        net.broadcast([1, 2])
        with pytest.raises(P2PGError, match="bad state"):
            net.set_ttl([1, -1])
        assert (net.ttl == -1).all()
    with gpu_net(g, "flood", count_received=False) as net:
        net.set_global_ids(np.arange(g.V, dtype=np.int32))
        net.broadcast([1, 2])
        with pytest.raises(P2PGError, match="bad state"):
            net.set_ttl([1, -1])
