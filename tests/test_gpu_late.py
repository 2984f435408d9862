"""Broadcasts that start mid-run (p2pg_set_sources_at / p2pg_originate) on the GPU: the engine,
through the C-ABI, against the late/ fixtures of the reference's own Node objects and against
tests/late_ref.py (pinned to those fixtures on the CPU, tests/test_late.py) -- bit-exact hop,
parent, delivered set and every per-round counter."""
import zlib

import numpy as np
import pytest

import late_ref
from test_late import LATE_CASES, load_late, ref_of

pytestmark = pytest.mark.gpu

FLOOD_KEYS = ("new_deliveries", "relays", "active_vertices", "active_words", "wedges", "deg_active",
              "received")
GOSSIP_KEYS = FLOOD_KEYS + ("scatter_words",)


def gpu_net(g, mode="flood", fanout=3, gseed=0, thr=0, cseed=0, record=True, **kw):
    from p2pnetwork.gpu import GraphNetwork, PeerGraph
    if not isinstance(g, PeerGraph):
        g = PeerGraph(g["rowptr"], g["colidx"])
    kw.setdefault("count_received", True)
    return GraphNetwork(g, mode=mode, fanout=fanout, gossip_seed=gseed, churn_threshold_value=thr,
                        churn_seed=cseed, record=record, **kw)


def assert_rounds(rounds, ref, mode, check_active=True):
    """Every counter of every round (the engine may not stop earlier or later than the reference).
    check_active=False: a schedule that grew while the run stood (originate after a quiet round)."""
    assert len(rounds) == len(ref.rounds), (len(rounds), len(ref.rounds))
    for i, (a, b) in enumerate(zip(rounds, ref.rounds)):
        assert a.round == i and a.received_exact == 1
        for k in (GOSSIP_KEYS if mode == "gossip" else FLOOD_KEYS):
            assert getattr(a, k) == b[k], (i, k, getattr(a, k), b[k])
        ahead = any(r["new_deliveries"] for r in ref.rounds[i + 1:])
        if check_active:
            assert a.active == (1 if b["new_deliveries"] or ahead else 0), (i, a.active)


def assert_planes(net, ref):
    hop, parent = net.hop_parent()
    np.testing.assert_array_equal(hop, ref.hop)
    np.testing.assert_array_equal(parent, ref.parent)
    np.testing.assert_array_equal(net.delivered(), ref.hop >= 0)


# ---- 1. the four fixtures of the reference's own Node objects -----------------------------------
@pytest.mark.parametrize("name", LATE_CASES)
def test_late_fixture_through_the_c_abi(name):
    z = load_late(name)
    mode = str(z["mode"])
    cfg = (mode, int(z["fanout"]), int(z["gossip_seed"]), int(z["churn_threshold"]), int(z["churn_seed"]))
    with gpu_net(z, *cfg) as net:
        net.broadcast(z["src"], z["start"])
        rounds = net.run()
        hop, parent = net.hop_parent()
        np.testing.assert_array_equal(hop, z["hop"])
        np.testing.assert_array_equal(parent, z["parent"])
        np.testing.assert_array_equal(net.delivered(), z["hop"] >= 0)
        assert late_ref.pad_equal([r.relays for r in rounds], z["round_relays"])
        assert net.message_count_send == int(z["round_relays"].sum())
        assert sum(r.received for r in rounds) == int(z["total_recv"])
        rel, _ = net.hop_parent(relative=True)
        np.testing.assert_array_equal(rel, np.where(z["hop"] >= 0, z["hop"] - z["start"][None, :], -1))
        assert_rounds(rounds, ref_of(z), mode)
    with gpu_net(z, *cfg, record=False, tally=True) as net:
        net.broadcast(z["src"], z["start"])
        rounds2 = net.run()
        assert [r.relays for r in rounds2] == [r.relays for r in rounds]
        t = net.message_tally()
        got = z["hop"] >= 0
        np.testing.assert_array_equal(t.reach, got.sum(axis=0))
        np.testing.assert_array_equal(t.hop_sum, np.where(got, z["hop"], 0).sum(axis=0))
        np.testing.assert_array_equal(t.last_hop, z["hop"].max(axis=0))
        c = net.peer_counters()
        np.testing.assert_array_equal(c.sent, z["peer_sent"])
        np.testing.assert_array_equal(c.received, z["peer_recv"])
        np.testing.assert_array_equal(net.message_reach(), got.sum(axis=0))


# ---- 2. randomised against late_ref ------------------------------------------------------------
def make_graph(kind, seed):
    from p2pnetwork.gpu import PeerGraph
    if kind == "rrg":
        return PeerGraph.random_regular(300, 4, seed)
    if kind == "rrg64":
        return PeerGraph.random_regular(64, 4, seed)
    if kind == "gnp":  # mean degree 2.5: isolated peers and several components
        return PeerGraph.gnp(400, 2.5, seed)
    return PeerGraph.barabasi_albert(500, 3, seed)


def make_schedule(g, M, seed, pattern, run_kw):
    """src / start: `late` = every start in 1..5; `mixed` = starts 0..4 and, where M allows: two
    messages of one word and two of different words at one peer in one round, an origin that is
    already active in its start round, an isolated origin."""
    from p2pnetwork.gpu import make_sources
    rng = np.random.default_rng(seed)
    src = make_sources(g.V, M, seed=seed).astype(np.int32)
    if pattern == "late":
        return src, rng.integers(1, 6, M).astype(np.int32)
    start = rng.integers(0, 5, M).astype(np.int32)
    start[0] = 0
    if M >= 4:  # one word, one peer, one round
        src[2] = src[3]
        start[2] = start[3] = 2
    if M >= 66:  # two words, one peer, one round
        src[65] = src[1]
        start[65] = start[1] = 3
    iso = np.nonzero(g.degree() == 0)[0]
    if len(iso) and M >= 6:
        src[5] = iso[0]
        start[5] = 1
    if M >= 8:  # a peer that takes a first receipt of message 0 in round 2 originates 6 and 7 there
        ref = late_ref.run(g.rowptr, g.colidx, src[:1], start[:1], **run_kw)
        busy = np.nonzero(ref.hop[:, 0] == 2)[0]
        assert len(busy)
        src[6] = src[7] = busy[0]
        start[6] = start[7] = 2
    return src, start


RANDOM_CASES = [
    ("rrg", "flood", 3, 0, 1, "late"),
    ("rrg", "flood", 3, 430_000_000, 63, "mixed"),
    ("gnp", "flood", 3, 0, 65, "mixed"),
    ("gnp", "gossip", 1, 0, 64, "mixed"),
    ("gnp", "gossip", 3, 430_000_000, 130, "mixed"),
    ("ba", "flood", 3, 430_000_000, 130, "late"),
    ("ba", "gossip", 3, 0, 65, "mixed"),
    ("ba", "gossip", 1, 430_000_000, 63, "late"),
    ("ba", "gossip", 3, 0, 1, "late"),
    ("rrg64", "flood", 3, 0, 4160, "mixed"),
    ("rrg64", "gossip", 3, 0, 4160, "mixed"),
    ("rrg64", "gossip", 1, 430_000_000, 4160, "late"),
]


@pytest.mark.parametrize("kind,mode,k,thr,M,pattern", RANDOM_CASES)
def test_late_random_matches_late_ref(kind, mode, k, thr, M, pattern):
    seed = zlib.crc32(repr((kind, mode, k, thr, M, pattern)).encode()) & 0xFFFF
    g = make_graph(kind, seed)
    run_kw = dict(mode=mode, fanout=k, gossip_seed=seed + 1, churn_threshold=thr, churn_seed=seed + 2)
    src, start = make_schedule(g, M, seed, pattern, run_kw)
    ref = late_ref.run(g.rowptr, g.colidx, src, start, **run_kw)
    with gpu_net(g, mode, k, seed + 1, thr, seed + 2) as net:
        net.broadcast(src, start)
        rounds = net.run()
        assert_rounds(rounds, ref, mode)
        assert_planes(net, ref)
        np.testing.assert_array_equal(net.start_rounds, start)


# ---- 3. gossip push forms ----------------------------------------------------------------------
def dense_case(W):
    """Every message from one of 20 origins: a sparse start, then rounds in which every peer takes
    first receipts in most words."""
    from p2pnetwork.gpu import PeerGraph, make_sources
    g = PeerGraph.barabasi_albert(600, 4, seed=40 + W)
    M = 64 * W - 5
    src = (make_sources(20, M, seed=W) * 29 + 7).astype(np.int32)
    return g, M, src


def late_at(g, M, src, r):
    """Messages 1, 2 (one word), M - 1 (the last word) and 7 start in round r: 1 and 2 at one peer,
    M - 1 at a hub of the BA graph, 7 where it was; every other message starts in round 0."""
    src, start = src.copy(), np.zeros(M, dtype=np.int32)
    late = [1, 2, 7, M - 1]
    start[late] = r
    src[2] = src[1]
    src[M - 1] = int(np.argmax(g.degree()))
    return src, start, late


def run_forms(g, src, start, k=3, gseed=11, thr=0):
    with gpu_net(g, "gossip", k, gseed, thr, 5) as net:
        net.broadcast(src, start)
        rounds = net.run()
        hop, parent = net.hop_parent()
    return rounds, hop, parent


@pytest.mark.parametrize("W", [3, 16, 17])
@pytest.mark.parametrize("push", ["store", "auto", "atomic"])
def test_late_gossip_push_forms(W, push, monkeypatch):
    """An origination round runs update / pull, k_originate and the separate push, whatever form
    the round would have had: after an E round (fused otherwise), in the first dense round after a
    sparse one (update + push in one pass otherwise, W > 16), in a sparse round.  The rounds before
    it keep the forms (and counters) they have without it."""
    from p2pnetwork.gpu.network import PUSH_FORMS
    if push != "auto":
        monkeypatch.setenv("P2PG_GOSSIP_PUSH", push)
    else:
        monkeypatch.setenv("P2PG_E_THRESH", "0.05")
        monkeypatch.setenv("P2PG_V_THRESH", "0.3")
        monkeypatch.setenv("P2PG_UPDATE_PUSH", "1")
    g, M, src = dense_case(W)
    # the same run with the late messages declared but never started: its rounds show where the
    # forms fall
    s0, st0, late = late_at(g, M, src, 1)
    s0[late] = -1
    st0[late] = -1
    base, _, _ = run_forms(g, s0, st0)
    forms = [PUSH_FORMS[r.push_form] for r in base]
    if push == "store":
        assert forms[0] == "edge" and set(forms[1:]) == {"fused"}, forms
        targets = [2]
    elif push == "atomic":
        assert set(forms) == {"atomic"}, forms
        targets = [3]
    else:
        dense = [i for i, f in enumerate(forms) if f != "atomic"]
        assert forms[0] == "atomic" and dense, forms
        # the first round after a sparse one that pushes per connection: update + push in one pass
        # where the rows allow it (W > 16)
        assert forms[dense[0]] == ("update_edge" if W > 16 else "edge"), forms
        assert "fused" in forms, forms
        sparse = [i for i, f in enumerate(forms) if f == "atomic" and i > 0]
        targets = sorted({dense[0], forms.index("fused")} | set(sparse[:1]))
    for r in targets:
        s, st, _ = late_at(g, M, src, r)
        rounds, hop, parent = run_forms(g, s, st)
        ref = late_ref.run(g.rowptr, g.colidx, s, st, "gossip", 3, 11, 0, 0, 5)
        assert_rounds(rounds, ref, "gossip")
        np.testing.assert_array_equal(hop, ref.hop)
        np.testing.assert_array_equal(parent, ref.parent)
        got = [PUSH_FORMS[x.push_form] for x in rounds]
        assert got[:r] == forms[:r], (r, got, forms)
        for k in GOSSIP_KEYS:
            assert [getattr(x, k) for x in rounds[:r]] == [getattr(x, k) for x in base[:r]], k
        assert got[r] in ("edge", "atomic"), (r, got)
        if push == "store":
            assert got[r] == "edge" and set(got[1:r] + got[r + 1:]) == {"fused"}, got


# ---- 4. hub origin -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["flood", "gossip"])
def test_late_hub_and_leaf_origins(mode):
    """Ring of 600 with peer 0 connected to 520 others (deg > HUB_T = 512: the pull hub split);
    originations at the hub (two words) and at a leaf in round 2."""
    from p2pnetwork.gpu import PeerGraph, make_sources
    V = 600
    edges = [(i, (i + 1) % V) for i in range(V)] + [(0, j) for j in range(2, 521)]
    g = PeerGraph.from_edges(V, edges)
    assert g.degree()[0] == 521 and g.degree()[550] == 2
    M = 70
    src = make_sources(V, M, seed=8).astype(np.int32)
    start = np.zeros(M, dtype=np.int32)
    src[[1, 65]] = 0
    src[3] = 550
    start[[1, 65, 3]] = 2
    ref = late_ref.run(g.rowptr, g.colidx, src, start, mode, 3, 21)
    with gpu_net(g, mode, 3, 21) as net:
        net.broadcast(src, start)
        rounds = net.run()
        assert_rounds(rounds, ref, mode)
        assert_planes(net, ref)
    assert rounds[2].relays >= (2 * 521 if mode == "flood" else 6)


# ---- 5. identity when nothing is late ----------------------------------------------------------
@pytest.mark.parametrize("record", [False, True])
def test_all_zero_starts_are_set_sources(record):
    from p2pnetwork.gpu import PeerGraph, make_sources
    g = PeerGraph.barabasi_albert(2000, 4, seed=3)
    src = make_sources(g.V, 4096, seed=3)
    out = []
    for start in (None, np.zeros(4096, dtype=np.int32)):
        with gpu_net(g, "gossip", 3, 0x5EED, record=record, count_received=False) as net:
            net.broadcast(src, start)
            rounds = net.run()
            planes = net.hop_parent() if record else ()
            out.append((rounds, net.seen_plane(), planes))
    (ra, sa, pa), (rb, sb, pb) = out
    assert ra == rb  # every field of every round, push_form included
    assert {r.push_form for r in ra} >= {1, 3}
    np.testing.assert_array_equal(sa, sb)
    for x, y in zip(pa, pb):
        np.testing.assert_array_equal(x, y)


# ---- 6. run() vs stepping, reset, wake-up, idle gap --------------------------------------------
@pytest.mark.parametrize("mode", ["flood", "gossip"])
def test_late_run_equals_stepping_and_reset_replays(mode):
    from p2pnetwork.gpu import PeerGraph, make_sources
    g = PeerGraph.barabasi_albert(400, 3, seed=12)
    M = 130
    src = make_sources(g.V, M, seed=12).astype(np.int32)
    start = np.random.default_rng(12).integers(0, 4, M).astype(np.int32)
    src[[127, 128, 129]] = -1  # declared, started below
    start[[127, 128, 129]] = -1
    ref = late_ref.run(g.rowptr, g.colidx, src[:127], start[:127], mode, 2, 31)
    quiet = len(ref.rounds)  # rounds 0 .. quiet - 1 ran; the next round to run is `quiet`
    gap = quiet + 10
    with gpu_net(g, mode, 2, 31) as net:
        net.broadcast(src, start)
        first = net.run()
        assert len(first) == quiet and not first[-1].active
        assert net.step().new_deliveries == 0  # a quiet engine stays quiet
        # a reply decided after the run went quiet wakes it; an idle gap of 10 rounds is crossed
        net.originate([127, 128], [5, 5], round=gap)
        net.originate([129], [17])  # default: the next round to run
        assert net.start_rounds[129] == quiet and net.sources[128] == 5
        more = net.run()
        full_src, full_start = net.sources.copy(), net.start_rounds.copy()
        ref2 = late_ref.run(g.rowptr, g.colidx, full_src, full_start, mode, 2, 31)
        assert more[0].round == quiet and not more[-1].active and more[-1].round > gap
        assert_rounds(first + more, ref2, mode, check_active=False)
        assert_planes(net, ref2)
        assert all(r.active for r in more if r.round < gap)
        # reset keeps the schedule (originate included) and replays it: twice the same
        for _ in range(2):
            net.reset()
            again = net.run()
            assert_rounds(again, ref2, mode)
            assert_planes(net, ref2)
        # stepping gives what run() gave
        net.reset()
        stepped = []
        while True:
            stepped.append(net.step())
            if not stepped[-1].active:
                break
        assert_rounds(stepped, ref2, mode)
        assert_planes(net, ref2)


# ---- 7. across round boundaries ----------------------------------------------------------------
@pytest.mark.parametrize("mode", ["flood", "gossip"])
def test_late_after_update_edges_matches_late_ref(mode):
    from p2pnetwork.gpu import PeerGraph, make_sources
    g = PeerGraph.random_regular(300, 4, seed=14)
    M = 70
    src = make_sources(g.V, M, seed=14).astype(np.int32)
    start = np.random.default_rng(14).integers(0, 5, M).astype(np.int32)
    start[:3] = 0
    start[3:8] = 3
    # after round 2, right before the origination round 3: the origin of message 3 loses a
    # connection (its sends of round 3 use the new ones) and gains one
    a = int(src[3])
    b = int(g.neighbours(a)[0])
    c = next(x for x in range(g.V) if x != a and x not in set(g.neighbours(a).tolist()))
    rem = [(int(g.neighbours(v)[1]), v) for v in (10, 50) if a not in (v, int(g.neighbours(v)[1]))]
    updates = {2: (np.array([(a, c)], np.int32), np.array([(a, b)] + rem, np.int32))}
    ref = late_ref.run(g.rowptr, g.colidx, src, start, mode, 2, 41, updates=updates)
    with gpu_net(g, mode, 2, 41) as net:
        net.broadcast(src, start)
        rounds = [net.step() for _ in range(3)]
        net.update_edges(add=updates[2][0], remove=updates[2][1])
        while rounds[-1].active:
            rounds.append(net.step())
        assert_rounds(rounds, ref, mode)
        assert_planes(net, ref)


@pytest.mark.parametrize("mode", ["flood", "gossip"])
def test_drop_relays_of_a_late_origination(mode):
    from p2pnetwork.gpu import PeerGraph
    g = PeerGraph.random_regular(200, 5, seed=15)
    src = np.array([3, 9, 9], dtype=np.int32)
    start = np.array([0, 2, 2], dtype=np.int32)
    with gpu_net(g, mode, 3, 51) as net:
        net.broadcast(src, start)
        rounds = [net.step() for _ in range(3)]
        d = net.deliveries()
        mine = (d.peer == 9) & (d.msg == 1)
        assert mine.sum() == 1 and d.parent[mine][0] == -1 and d.hop[mine][0] == 2
        sent = net.message_count_send
        net.drop_relays([9], [1])
        # an origination's relays: all deg connections (flood), min(k, deg) (gossip)
        assert sent - net.message_count_send == (5 if mode == "flood" else 3)
        nxt = net.step()
        assert nxt.received == rounds[2].relays - (5 if mode == "flood" else 3)
        while nxt.active:
            nxt = net.step()
        got = net.delivered()
        assert got[:, 1].sum() == 1 and got[9, 1]       # the withdrawn message never spreads
        assert got[:, 2].sum() == g.V or mode == "gossip"  # its sibling at the same origin does
        assert got[:, 2].sum() > 1


# ---- 8. refusals -------------------------------------------------------------------------------
def test_late_refusals_leave_the_engine_unchanged():
    from p2pnetwork.gpu import P2PGError, PeerGraph, _lib
    g = PeerGraph.random_regular(200, 4, seed=16)
    src = np.array([1, 2, -1, -1, 7], dtype=np.int32)
    start = np.array([0, 4, -1, -1, 6], dtype=np.int32)
    L = _lib.lib()
    with gpu_net(g, "flood") as net:
        one = np.array([5], dtype=np.int32)
        for bad_src, bad_start in (([1, 2], [0, -2]), ([1, -1], [0, 0]), ([1, 5], [0, -1]), ([1, 200], [0, 3])):
            with pytest.raises(P2PGError, match="bad argument"):
                net.broadcast(bad_src, bad_start)
        with pytest.raises(P2PGError, match="bad state"):
            net.originate([0], [1], round=1)  # no sources yet
        net.broadcast(src, start)
        with pytest.raises(P2PGError, match="bad argument"):
            net.broadcast([1, -1])  # p2pg_set_sources still rejects negative sources
        net.broadcast(src, start)
        for _ in range(3):
            net.step()
        ref = late_ref.run(g.rowptr, g.colidx, [1, 2, 9, 0, 7], [0, 4, 5, -1, 6], "flood")

        def refused(kind, msgs, peers, rnd):
            with pytest.raises(P2PGError, match=kind):
                net.originate(msgs, peers, round=rnd)
        refused("bad argument", [2], [9], 2)        # a round that has run
        refused("bad argument", [2], [9], 0)        # round 0 belongs to set_sources_at
        refused("bad argument", [1], [9], 5)        # scheduled already
        refused("bad argument", [0], [9], 5)        # ... and originated already
        refused("bad argument", [5], [9], 5)        # message out of range
        refused("bad argument", [-1], [9], 5)
        refused("bad argument", [2], [200], 5)      # peer out of range
        refused("bad argument", [2, 3, 2], [9, 9, 9], 5)  # listed twice
        refused("bad argument", [2, 1], [9, 9], 5)  # one bad entry rejects the whole call
        assert L.p2pg_originate(net._h, 1, None, _lib.ptr(one), 5) == -1
        np.testing.assert_array_equal(net.start_rounds, start)
        # snapshots do not hold a late schedule
        with pytest.raises(P2PGError, match="bad state"):
            net.snapshot()
        with pytest.raises(P2PGError, match="bad state"):
            net.restore(np.zeros(256, dtype=np.uint8))
        # between step_begin and step_end
        net.step_begin()
        refused("bad state", [2], [9], 5)
        with pytest.raises(P2PGError, match="bad state"):
            net.broadcast(src, start)
        r3 = net.step_end()
        assert r3.round == 3
        net.originate([2], [9], round=5)            # the valid call, after all of them
        rounds = net.rounds[:]
        while rounds[-1].active:
            rounds.append(net.step())
        assert_rounds(rounds, ref, "flood")
        assert_planes(net, ref)
    # a vertex-partitioned rank
    with gpu_net(g, "flood", local_graph=True, count_received=False) as net:
        with pytest.raises(P2PGError, match="bad state"):
            net.broadcast([1, 2], [0, 3])
        net.broadcast([1, 2], [0, 0])               # all zero is p2pg_set_sources
        net.broadcast([1, 2])
        z = np.zeros(1, dtype=np.int32)
        assert L.p2pg_originate(net._h, 1, _lib.ptr(z), _lib.ptr(z), 3) == -2
    with gpu_net(g, "flood", count_received=False) as net:
        net.set_global_ids(np.arange(g.V, dtype=np.int32))
        with pytest.raises(P2PGError, match="bad state"):
            net.broadcast([1, 2], [0, 3])
        net.broadcast([1, 2])
        z = np.zeros(1, dtype=np.int32)
        assert L.p2pg_originate(net._h, 1, _lib.ptr(z), _lib.ptr(z), 3) == -2
    # with all starts 0 snapshots work as before
    with gpu_net(g, "flood", count_received=False) as net:
        net.broadcast([1, 2], [0, 0])
        net.step()
        assert len(net.snapshot()) > 0
