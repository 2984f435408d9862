"""Network partitions (p2pg_set_netsplit) on the GPU: the engine, through the C-ABI, against
tests/netsplit_ref.py (pinned on the CPU by tests/test_netsplit.py) -- the seen plane, hop and parent,
every per-round counter the rule fixes, the send lists of a cut round and of the round before the
window, the three tallies and the exchange records.  scatter_words and touched_words of a gossip
round whose sends arrive in a cut round are the engine's own."""
import functools
import os

import numpy as np
import pytest

import netsplit_ref
from test_gpu_cost import assert_cost
from test_gpu_late import FLOOD_KEYS, assert_planes, gpu_net
from test_gpu_latency import assert_latency
from test_gpu_pull import assert_records

pytestmark = pytest.mark.gpu

CHURN = 430_000_000  # 10 %
ATOMIC, EDGE, FUSED, UPDATE_EDGE = 1, 2, 3, 4  # p2pg_round_stats.push_form
WIDTHS = [1, 3, 8, 9, 16, 17, 32, 64, 65]


def sides_of(V, how):
    v = np.arange(V)
    return {"range2": (v >= V // 2), "range3": v * 3 // V, "parity2": v % 2, "parity3": v % 3}[how].astype(np.int32)


def push_cut_rounds(cf, cu, n):
    """The gossip rounds whose sends arrive in a cut round."""
    return {r for r in range(n) if cf <= r + 1 < cu}


def assert_rounds(rounds, ref_rounds, mode, cf, cu, counted=True, setting=None, last_start=0, keys=FLOOD_KEYS):
    """Every counter the rule fixes.  counted = P2PG_FLAG_RECEIVED: `received` exact everywhere; else a
    cut round reports the sends of the round before and received_exact = 0."""
    assert len(rounds) == len(ref_rounds), (len(rounds), len(ref_rounds))
    own = push_cut_rounds(cf, cu, len(rounds)) if mode == "gossip" else set()
    for i, (a, b) in enumerate(zip(rounds, ref_rounds)):
        inexact = not counted and cf <= i < cu
        assert a.round == i and a.received_exact == (0 if inexact else 1), (i, a.received_exact)
        for k in keys:
            want = b[k] if k != "received" or not inexact else (ref_rounds[i - 1]["relays"] if i else 0)
            assert getattr(a, k) == want, (i, k, getattr(a, k), want)
        if mode == "gossip":
            if i in own:
                assert a.push_form == ATOMIC, (i, a.push_form)
            elif "scatter_words" in b:
                assert a.scatter_words == b["scatter_words"], (i, a.scatter_words, b["scatter_words"])
        ahead = any(r["new_deliveries"] for r in ref_rounds[i + 1:]) or last_start > i
        if setting is not None:
            ahead = ahead or netsplit_ref.pull_ref.arrival_ahead(i + 1, setting)
        assert a.active == (1 if b["new_deliveries"] or ahead else 0), (i, a.active)


def assert_sends(net, ref, r):
    s = net.sends()
    snd, rcv, msg, lost = ref.sends[r]
    np.testing.assert_array_equal(s.sender, snd)
    np.testing.assert_array_equal(s.receiver, rcv)
    np.testing.assert_array_equal(s.msg, msg)
    np.testing.assert_array_equal(s.lost, lost)


def assert_all_tallies(net, ref, start):
    got = ref.hop >= 0
    t = net.message_tally()
    np.testing.assert_array_equal(t.reach, got.sum(axis=0))
    np.testing.assert_array_equal(t.hop_sum, np.where(got, ref.hop, 0).sum(axis=0))
    np.testing.assert_array_equal(t.last_hop, ref.hop.max(axis=0))
    c = net.peer_counters()
    np.testing.assert_array_equal(c.sent, ref.peer_sent)
    np.testing.assert_array_equal(c.received, ref.peer_recv)
    assert_cost(net.message_cost(), (ref.msg_sent, ref.msg_recv))
    assert_latency(net, ref.hop, start)
    assert int(ref.msg_sent.sum()) == sum(r["relays"] for r in ref.rounds)


def full_compare(g, mode, k, gseed, cthr, cseed, src, start, side, cf, cu, ref, down=None, ae=None, sends_at=()):
    """One engine with records and the three tallies: run() against ref, then the stepped replay
    with the send lists of the rounds `sends_at`."""
    with gpu_net(g, mode, k, gseed, cthr, cseed, record=True, tally=True, cost=True, latency=True) as net:
        net.broadcast(src, start)
        if down is not None:
            net.set_downtime(*down)
        if ae is not None:
            net.set_anti_entropy(ae[0], ae[1], ae[2], seed=ae[3])
        net.set_netsplit(side, cf, cu)
        assert net.netsplit is not None
        rounds = net.run()
        assert_rounds(rounds, ref.rounds, mode, cf, cu, setting=ae[:3] if ae else None, last_start=int(np.max(start)))
        assert_planes(net, ref)
        bits = np.unpackbits(net.seen_plane().view(np.uint8).reshape(g.V, -1), axis=1, bitorder="little")
        np.testing.assert_array_equal(bits[:, :len(src)].astype(bool), ref.hop >= 0)
        assert_all_tallies(net, ref, start)
        assert_records(net, ref)
        net.reset()  # the setting stays, the run replays
        stepped = []
        for r in range(len(ref.rounds)):
            stepped.append(net.step())
            if r in sends_at:
                assert_sends(net, ref, r)
        assert stepped == rounds
        assert_planes(net, ref)
        assert_records(net, ref)
    return rounds


# ---- 1. the four fixtures of the reference's own Node objects -----------------------------------
def test_netsplit_fixtures_through_the_c_abi():
    from test_netsplit import NETSPLIT_CASES, cfg_of, load_netsplit, ref_of
    for name in NETSPLIT_CASES:
        z = load_netsplit(name)
        c = cfg_of(z)
        ref = ref_of(name)
        cf, cu = int(z["cut_from"]), int(z["cut_until"])
        ae = tuple(int(x) for x in z["anti_entropy"]) + (int(z["pull_seed"]),)
        down = (z["down_from"], z["down_until"]) if (z["down_from"] >= 0).any() else None
        from p2pnetwork.gpu import PeerGraph
        g = PeerGraph(z["rowptr"], z["colidx"])
        rounds = full_compare(g, c["mode"], c["fanout"], c["gossip_seed"], c["churn_threshold"], c["churn_seed"],
                              z["src"], z["start"], z["side"], cf, cu, ref, down=down, ae=ae if ae[0] > 0 else None,
                              sends_at={max(cf - 2, 0), cf, cu - 1})
        assert netsplit_ref.pad_equal([r.relays for r in rounds], z["round_relays"])
        assert sum(r.received for r in rounds) == int(z["total_recv"])


# ---- 2. flood: k_pull_cut at every row width --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ba2000():
    from p2pnetwork.gpu import PeerGraph
    g = PeerGraph.barabasi_albert(2000, 4, seed=3)
    assert int(g.degree().max()) > 64
    return g


@functools.lru_cache(maxsize=None)
def flood_case(W, cthr, how):
    from p2pnetwork.gpu import make_sources
    g = ba2000()
    M = 64 * W - 5
    src = make_sources(g.V, M, seed=W).astype(np.int32)
    start = np.zeros(M, dtype=np.int32)
    start[np.random.default_rng(W).integers(0, M, max(M // 8, 1))] = 2
    side = sides_of(g.V, how)
    hop, rounds = netsplit_ref.flood_packed(g.rowptr, g.colidx, src, start, side, 1, 4, cthr, 7)
    return g, src, start, side, hop, rounds


@pytest.mark.parametrize("how", ["range2", "range3", "parity2", "parity3"])
@pytest.mark.parametrize("cthr", [0, CHURN])
@pytest.mark.parametrize("W", WIDTHS)
def test_flood_pull_cut_row_widths(W, cthr, how):
    """Cut rounds 1 .. 3 (round 2 is an origination round too), the heal in round 4; hubs of degree
    > 64 on every side.  The id-parity split cuts almost every connection: a peer's arrivals come
    from a strict subset of its row."""
    g, src, start, side, hop, ref_rounds = flood_case(W, cthr, how)
    keys = tuple(k for k in FLOOD_KEYS if k != "received")
    with gpu_net(g, "flood", 3, 0, cthr, 7, record=False, latency=True) as net:
        net.broadcast(src, start)
        net.set_netsplit(side, 1, 4)
        rounds = net.run()
        assert_rounds(rounds, ref_rounds, "flood", 1, 4, keys=keys, last_start=2)
        bits = np.unpackbits(net.seen_plane().view(np.uint8).reshape(g.V, -1), axis=1, bitorder="little")
        np.testing.assert_array_equal(bits[:, :len(src)].astype(bool), hop >= 0)
        assert_latency(net, hop, start)
    # the cut held: nothing crossed in rounds 1 .. 3 but by origination
    for r in (1, 2, 3):
        vs, ms = np.nonzero(hop == r)
        assert (side[vs] == side[src[ms]]).all()


@pytest.mark.parametrize("how", ["range3", "parity2"])
@pytest.mark.parametrize("cthr", [0, CHURN])
@pytest.mark.parametrize("W", [1, 3])
def test_flood_pull_cut_everything_compared(W, cthr, how):
    """The same graph at narrow rows against netsplit_ref.run: parents, send lists, the three
    tallies, `received`, with anti-entropy after the heal."""
    g, src, start, side, hop, _ = flood_case(W, cthr, how)
    ae = (2, 3, 9, 77)
    ref = netsplit_ref.run(g.rowptr, g.colidx, src, start, side, 1, 4, mode="flood", churn_threshold=cthr,
                           churn_seed=7, anti_entropy=ae[:3], pull_seed=ae[3])
    full_compare(g, "flood", 3, 0, cthr, 7, src, start, side, 1, 4, ref, ae=ae, sends_at={0, 2, 3})


@pytest.mark.parametrize("cthr", [0, CHURN])
@pytest.mark.parametrize("W", [8, 17, 65])
def test_flood_pull_cut_wide_rows_everything_compared(W, cthr):
    """Wide rows and the slice loop against netsplit_ref.run on a small graph: parents, `received`,
    send lists and the three tallies (the flood branches of the passes that carry the cut term)."""
    from p2pnetwork.gpu import PeerGraph, make_sources
    g = PeerGraph.barabasi_albert(300 if W <= 17 else 120, 4, seed=60 + W)
    M = 64 * W - 5
    src = make_sources(g.V, M, seed=W).astype(np.int32)
    start = np.zeros(M, dtype=np.int32)
    start[np.random.default_rng(W).integers(0, M, max(M // 8, 1))] = 2
    side = sides_of(g.V, "parity2" if W != 17 else "range3")
    ref = netsplit_ref.run(g.rowptr, g.colidx, src, start, side, 1, 4, mode="flood", churn_threshold=cthr, churn_seed=7)
    assert sum(netsplit_ref.lost_to_cut(ref, r, side, 1, 4, cthr, 7).sum() for r in range(3)) > 0
    full_compare(g, "flood", 3, 0, cthr, 7, src, start, side, 1, 4, ref, sends_at={0, 2, 3})


# ---- 2b. flood: a pull hub with neighbours on both sides (k_pull_cut_hub) --------------------------------
@functools.lru_cache(maxsize=None)
def split_hub_graph():
    """Peer 0 with 1300 connections (above the pull hubs' threshold of 512 and the 1024 connections
    of one LDS stage); its neighbours 1 .. 1300 form a random 3-regular graph among themselves, so
    the flood moves among them without the hub.  Sides by id range: the hub with 1 .. 650, the other
    half of its row on the other side."""
    from p2pnetwork.gpu import PeerGraph
    n = 1300
    r = PeerGraph.random_regular(n, 3, seed=13)
    a = np.repeat(np.arange(n), np.diff(r.rowptr))
    among = [(int(x) + 1, int(y) + 1) for x, y in zip(a, r.colidx) if x < y]
    edges = [(0, i) for i in range(1, n + 1)] + among
    g = PeerGraph.from_edges(n + 1, np.array(edges, dtype=np.int32))
    assert int(g.degree()[0]) == n > 1024
    side = (np.arange(n + 1) > n // 2).astype(np.int32)
    return g, side


def split_hub_case(W):
    from p2pnetwork.gpu import make_sources
    g, side = split_hub_graph()
    M = 64 * W - 5
    src = (1 + make_sources(g.V - 1, M, seed=W)).astype(np.int32)  # every origin a neighbour of the hub
    start = np.random.default_rng(W).integers(0, 3, M).astype(np.int32)
    return g, side, src, start


@pytest.mark.parametrize("cthr", [0, CHURN])
@pytest.mark.parametrize("W", [1, 2, 64])
def test_flood_pull_hub_with_neighbours_on_both_sides(W, cthr):
    """The hub first-receives in the cut rounds 1 .. 3 from its own side only -- single copies (an
    origin's own send) and many at once (its neighbours' relays) -- and from the other side after the
    heal.  W = 1, 2: everything against netsplit_ref.run; W = 64: planes and counters against the
    packed flood."""
    g, side, src, start = split_hub_case(W)
    if W <= 2:
        ref = netsplit_ref.run(g.rowptr, g.colidx, src, start, side, 1, 4, mode="flood", churn_threshold=cthr,
                               churn_seed=9)
        hop = ref.hop
    else:
        hop, ref_rounds = netsplit_ref.flood_packed(g.rowptr, g.colidx, src, start, side, 1, 4, cthr, 9)
    # the hub's receipts: some in every cut round, each from a same-side origin or relay; some after
    # the heal of messages that started on the other side
    for r in (1, 2, 3):
        assert (hop[0] == r).any()
    other = side[src] != side[0]
    assert not ((hop[0][other] >= 0) & (hop[0][other] < 4)).any() and (hop[0][other] >= 4).any()
    assert ((hop[0][~other] >= 1) & (hop[0][~other] < 4)).any()
    if W <= 2:
        full_compare(g, "flood", 3, 0, cthr, 9, src, start, side, 1, 4, ref, sends_at={0, 1, 3, 4})
        return
    keys = tuple(k for k in FLOOD_KEYS if k != "received")
    with gpu_net(g, "flood", 3, 0, cthr, 9, record=False, latency=True) as net:
        net.broadcast(src, start)
        net.set_netsplit(side, 1, 4)
        rounds = net.run()
        assert_rounds(rounds, ref_rounds, "flood", 1, 4, keys=keys, last_start=2)
        bits = np.unpackbits(net.seen_plane().view(np.uint8).reshape(g.V, -1), axis=1, bitorder="little")
        np.testing.assert_array_equal(bits[:, :len(src)].astype(bool), hop >= 0)
        assert_latency(net, hop, start)


# ---- 3. gossip: k_push_cut at every row width ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gossip_graph(W):
    from p2pnetwork.gpu import PeerGraph
    return PeerGraph.barabasi_albert(600 if W <= 17 else 160, 4, seed=40 + W)


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("W", WIDTHS)
def test_gossip_push_cut_row_widths(W, k, monkeypatch):
    """A window that starts in the sparse phase (rounds 2 .. 5), under churn, with the thresholds
    that let small graphs enter the dense rounds after the heal."""
    from p2pnetwork.gpu import make_sources
    monkeypatch.setenv("P2PG_E_THRESH", "0.05")
    monkeypatch.setenv("P2PG_V_THRESH", "0.3")
    monkeypatch.setenv("P2PG_UPDATE_PUSH", "1")
    g = gossip_graph(W)
    M = 64 * W - 5
    src = (make_sources(20, M, seed=W) * 7 + 3).astype(np.int32)
    start = np.zeros(M, dtype=np.int32)
    start[np.random.default_rng(W).integers(0, M, max(M // 8, 1))] = 3
    side = sides_of(g.V, "parity2" if W % 2 else "range3")
    cthr = CHURN if k == 3 else 0
    ref = netsplit_ref.run(g.rowptr, g.colidx, src, start, side, 2, 6, mode="gossip", fanout=k, gossip_seed=11,
                           churn_threshold=cthr, churn_seed=5)
    wasted = [netsplit_ref.lost_to_cut(ref, r, side, 2, 6, cthr, 5).sum() for r in range(len(ref.rounds))]
    assert sum(wasted) > 0 and all(wasted[r] == 0 for r in range(len(wasted)) if not 2 <= r + 1 < 6)
    full_compare(g, "gossip", k, 11, cthr, 5, src, start, side, 2, 6, ref, sends_at={0, 1, 4})


@functools.lru_cache(maxsize=None)
def dense_graph():
    from p2pnetwork.gpu import PeerGraph, make_sources
    g = PeerGraph.barabasi_albert(2000, 4, seed=3)
    return g, make_sources(g.V, 4096, seed=3)


def dense_run(side=None, cf=0, cu=0, call=True, timing=False):
    g, src = dense_graph()
    with gpu_net(g, "gossip", 3, 0x5EED, record=False, count_received=False, timing=timing) as net:
        net.broadcast(src)
        if call:
            net.set_netsplit(side, cf, cu)
        rounds = net.run()
        return rounds, net.seen_plane(), ({k: v[1] for k, v in net.kernel_times().items()} if timing else None)


@functools.lru_cache(maxsize=None)
def dense_base():
    return dense_run(call=False, timing=True)


def test_netsplit_window_inside_the_fused_rounds():
    g, src = dense_graph()
    base, _, _ = dense_base()
    fused = [r.round for r in base if r.push_form == FUSED]
    assert len(fused) >= 5, [r.push_form for r in base]
    w0 = fused[2]  # cut rounds w0, w0 + 1: the pushes of rounds w0 - 1 and w0 take the cut
    assert w0 - 2 in fused and w0 + 2 in fused
    side = sides_of(g.V, "range2")
    rounds, seen, _ = dense_run(side, w0, w0 + 2)
    assert rounds[:w0 - 1] == base[:w0 - 1]  # every field of every round before, push_form included
    assert rounds[w0 - 2].push_form == FUSED  # the round before the window's first cut push
    assert [rounds[r].push_form for r in (w0 - 1, w0)] == [ATOMIC, ATOMIC], [x.push_form for x in rounds]
    # after the heal: round w0 + 1 consumes the last cut push (an update) and stores its dense frontier
    # into E, and round w0 + 2, the first that can be fused again, is -- as in the plain run
    assert base[w0 + 2].push_form == FUSED
    assert rounds[w0 + 1].push_form in (EDGE, UPDATE_EDGE), [x.push_form for x in rounds]
    assert rounds[w0 + 2].push_form == FUSED, [x.push_form for x in rounds]
    ref = netsplit_ref.run(g.rowptr, g.colidx, src, np.zeros(len(src), dtype=np.int32), side, w0, w0 + 2,
                           mode="gossip", fanout=3, gossip_seed=0x5EED, planes=False)
    assert_rounds(rounds, ref.rounds, "gossip", w0, w0 + 2, counted=False)
    bits = np.unpackbits(seen.view(np.uint8).reshape(g.V, -1), axis=1, bitorder="little")[:, :len(src)]
    np.testing.assert_array_equal(bits.astype(bool), ref.hop >= 0)


# ---- 4. a hub on the border -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["flood", "gossip"])
def test_hub_on_the_border_under_churn(mode):
    """test_gpu_drop's hub graph: peer 0 with 701 connections, alone on its side -- every neighbour
    is on the other side; the window opens in round 1 and heals in round 4."""
    from test_gpu_drop import case_of
    g, M, src = case_of("hub", 70)
    start = np.random.default_rng(9).integers(0, 3, M).astype(np.int32)
    start[src == 0] = 0
    side = np.zeros(g.V, dtype=np.int32)
    side[0] = 5
    ref = netsplit_ref.run(g.rowptr, g.colidx, src, start, side, 1, 4, mode=mode, fanout=3, gossip_seed=11,
                           churn_threshold=CHURN, churn_seed=6)
    lost0 = netsplit_ref.lost_to_cut(ref, 0, side, 1, 4, CHURN, 6)
    assert lost0.any() and (ref.sends[0][0][lost0] == 0).any()  # the hub's own sends, wasted on the cut
    assert not ((ref.hop[0] >= 1) & (ref.hop[0] < 4)).any() and (ref.hop[0] >= 4).any()
    full_compare(g, mode, 3, 11, CHURN, 6, src, start, side, 1, 4, ref, sends_at={0, 1, 3})


# ---- 5. heal and repair -------------------------------------------------------------------------------
def test_flood_saturates_both_sides_and_only_the_repair_crosses():
    from p2pnetwork.gpu import PeerGraph, make_sources
    g = PeerGraph.random_regular(300, 4, seed=31)
    M = 70
    src = make_sources(g.V, M, seed=31).astype(np.int32)
    start = np.zeros(M, dtype=np.int32)
    side = sides_of(g.V, "range2")
    cf, cu = 0, 40  # the flood is over long before the heal
    ae = (3, cu, cu + 30, 5)
    none = netsplit_ref.run(g.rowptr, g.colidx, src, start, side, cf, cu, mode="flood")
    assert len(none.rounds) < cu - 2
    vs, ms = np.nonzero(none.hop >= 0)
    assert (side[vs] == side[src[ms]]).all() and not (none.hop >= 0).all()
    ref = netsplit_ref.run(g.rowptr, g.colidx, src, start, side, cf, cu, mode="flood", anti_entropy=ae[:3],
                           pull_seed=ae[3])
    assert (ref.hop >= 0).all()  # full reach with the repair
    with gpu_net(g, "flood", record=False, count_received=False) as net:
        net.broadcast(src, start)
        net.set_netsplit(side, cf, cu)
        rounds = net.run()
        assert len(rounds) == len(none.rounds)
        np.testing.assert_array_equal(net.delivered(), none.hop >= 0)
    rounds = full_compare(g, "flood", 3, 0, 0, 0, src, start, side, cf, cu, ref, ae=ae, sends_at={cu - 1, cu + 2})
    assert sum(r.new_deliveries for r in rounds) == g.V * M
    # message_latency (compared in full_compare) puts the repaired receipts at their arrival rounds
    crossed = side[:, None] != side[src][None, :]
    # (with them, the few same-side peers the cut had isolated from their own side's flood)
    late = ref.hop >= cu + 2
    assert late[crossed].all() and not (none.hop >= 0)[late].any()
    assert ref.latency.hist[:, cu + 2:].sum() == late.sum() >= crossed.sum() > 0


# ---- 6. a removed setting ----------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["none", "equal_sides", "empty_window"])
def test_removed_netsplit_is_an_engine_that_never_saw_the_call(how):
    g, src = dense_graph()
    base, seen0, launches0 = dense_base()
    side = sides_of(g.V, "range2")
    with gpu_net(g, "gossip", 3, 0x5EED, record=False, count_received=False, timing=True) as net:
        net.broadcast(src)
        net.set_netsplit(side, 3, 6)
        assert net.netsplit is not None
        if how == "none":
            net.set_netsplit(None)
        elif how == "equal_sides":
            net.set_netsplit(np.full(g.V, 4, dtype=np.int32), 3, 6)
        else:
            net.set_netsplit(side, 6, 3)
        assert net.netsplit is None
        rounds = net.run()
        assert rounds == base  # every field of every round, push_form included
        np.testing.assert_array_equal(net.seen_plane(), seen0)
        assert {k: v[1] for k, v in net.kernel_times().items()} == launches0
        assert len(net.snapshot()) > 0  # (and snapshots work again)


def test_engine_without_the_call_equals_the_recorded_rounds():
    """The comparison run of the tests above is the run the tree made before the call existed:
    tests/golden/netsplit/dense2000_parent_rounds.npz holds the rounds the parent commit's library reported
    for the same graph and sources -- every field, push_form included -- and its launch counts."""
    base, _, launches = dense_base()
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "netsplit",
                              "dense2000_parent_rounds.npz"),
                 allow_pickle=False) as z:
        fields = [str(x) for x in z["fields"]]
        table = z["rounds"]
        classes = [str(x) for x in z["classes"]]
        counts = z["launches"]
    assert len(base) == len(table)
    for r, row in zip(base, table):
        assert [int(getattr(r, f)) for f in fields] == [int(x) for x in row], (r.round, fields)
    assert {k: int(c) for k, c in zip(classes, counts)} == launches


# ---- 7. run equals stepping, reset replays; 8. received_exact -------------------------------------------
@pytest.mark.parametrize("mode", ["flood", "gossip"])
def test_received_exact_is_zero_exactly_in_the_window_without_the_flag(mode):
    from p2pnetwork.gpu import PeerGraph, make_sources
    g = PeerGraph.random_regular(200, 4, seed=21) if mode == "flood" else PeerGraph.barabasi_albert(400, 3, 21)
    src = make_sources(g.V, 70, seed=21).astype(np.int32)
    start = np.zeros(70, dtype=np.int32)
    side = sides_of(g.V, "parity2")
    ref = netsplit_ref.run(g.rowptr, g.colidx, src, start, side, 2, 5, mode=mode, fanout=3, gossip_seed=71)
    assert len(ref.rounds) > 7
    with gpu_net(g, mode, 3, 71, record=True, count_received=False) as net:
        net.broadcast(src, start)
        net.set_netsplit(side, 2, 5)
        rounds = net.run()
        assert [r.received_exact for r in rounds] == [0 if 2 <= r.round < 5 else 1 for r in rounds]
        assert_rounds(rounds, ref.rounds, mode, 2, 5, counted=False)
        assert rounds[2].received > ref.rounds[2]["received"]  # an upper bound, and not the exact count
        assert_planes(net, ref)
        net.reset()
        stepped = [net.step() for _ in rounds]
        assert stepped == rounds
    with gpu_net(g, mode, 3, 71, record=True, count_received=True) as net:  # exact with the flag, churn or not
        net.broadcast(src, start)
        net.set_netsplit(side, 2, 5)
        assert_rounds(net.run(), ref.rounds, mode, 2, 5)


# ---- 9. refusals ---------------------------------------------------------------------------------------
def test_netsplit_refusals_leave_the_engine_unchanged():
    from p2pnetwork.gpu import CompatNetwork, P2PGError, PeerGraph, _lib
    L = _lib.lib()
    g = PeerGraph.random_regular(200, 4, seed=22)
    V = g.V
    src = np.array([1, 2, 7], dtype=np.int32)
    start = np.array([0, 4, 6], dtype=np.int32)
    side = sides_of(V, "range2")
    ref = netsplit_ref.run(g.rowptr, g.colidx, src, start, side, 1, 7, mode="flood")
    assert not hasattr(CompatNetwork, "set_netsplit")

    def ptr(a):
        return _lib.ptr(np.ascontiguousarray(a, dtype=np.int32))

    with gpu_net(g, "flood", tally=True) as net:
        net.set_netsplit(side, 1, 7)  # before any sources: the sides belong to the peers
        net.broadcast(src, start)
        assert net.netsplit is not None
        # argument errors
        bad = side.copy()
        bad[20] = -1
        with pytest.raises(P2PGError, match="bad argument"):
            net.set_netsplit(bad, 1, 7)
        with pytest.raises(P2PGError, match="bad argument"):
            net.set_netsplit(side, -1, 7)
        assert L.p2pg_set_netsplit(net._h, V - 1, ptr(side[:-1]), 1, 7) == -1
        assert L.p2pg_set_netsplit(net._h, V + 1, ptr(np.append(side, 0)), 1, 7) == -1
        with pytest.raises(ValueError):
            net.set_netsplit(side[:-1], 1, 7)
        # hop limits, a relay policy, snapshots
        with pytest.raises(P2PGError, match="bad state"):
            net.set_ttl(np.array([3, -1, -1], dtype=np.int32))
        with pytest.raises(P2PGError, match="bad state"):
            net.set_relay_policy(thresholds=np.full(V, 1 << 31, dtype=np.uint32), seed=1)
        with pytest.raises(P2PGError, match="bad state"):
            net.snapshot()
        with pytest.raises(P2PGError, match="bad state"):
            net.restore(np.zeros(256, dtype=np.uint8))
        # between step_begin and step_end, and once a round has run
        net.step_begin()
        with pytest.raises(P2PGError, match="bad state"):
            net.set_netsplit(side, 1, 7)
        with pytest.raises(P2PGError, match="bad state"):
            net.set_netsplit(None)
        assert net.step_end().round == 0
        with pytest.raises(P2PGError, match="bad state"):
            net.set_netsplit(side, 2, 7)
        with pytest.raises(P2PGError, match="bad state"):
            net.set_netsplit(None)
        net.step()
        with pytest.raises(P2PGError, match="bad state"):
            net.update_edges(add=np.array([(0, 199)], np.int32), remove=np.zeros((0, 2), np.int32))
        with pytest.raises(P2PGError, match="bad state"):
            net.drop_relays(np.array([1], np.int32), np.array([0], np.int32))
        rounds = net.rounds[:]
        while rounds[-1].active:
            rounds.append(net.step())
        assert_rounds(rounds, ref.rounds, "flood", 1, 7, last_start=6)
        assert_planes(net, ref)
        net.reset()  # allowed again after a reset; the run replays
        net.set_netsplit(side, 1, 7)
        assert_rounds(net.run(), ref.rounds, "flood", 1, 7, last_start=6)
    # the other call order: hop limits or a policy first
    with gpu_net(g, "flood", count_received=False) as net:
        net.broadcast(src, start, ttl=np.array([3, -1, -1], dtype=np.int32))
        with pytest.raises(P2PGError, match="bad state"):
            net.set_netsplit(side, 1, 7)
        assert net.netsplit is None
    with gpu_net(g, "flood", count_received=False) as net:
        net.broadcast(src, start)
        net.set_relay_policy(thresholds=np.full(V, 1 << 31, dtype=np.uint32), seed=1)
        with pytest.raises(P2PGError, match="bad state"):
            net.set_netsplit(side, 1, 7)
    # a vertex-partitioned rank
    with gpu_net(g, "flood", local_graph=True, count_received=False) as net:
        with pytest.raises(P2PGError, match="bad state"):
            net.set_netsplit(side, 1, 7)
    with gpu_net(g, "flood", count_received=False) as net:
        net.set_global_ids(np.arange(V, dtype=np.int32))
        with pytest.raises(P2PGError, match="bad state"):
            net.set_netsplit(side, 1, 7)
    with gpu_net(g, "flood", count_received=False) as net:
        net.set_netsplit(side, 1, 7)
        with pytest.raises(P2PGError, match="bad state"):
            net.set_global_ids(np.arange(V, dtype=np.int32))
        net.set_netsplit(None)
        net.set_global_ids(np.arange(V, dtype=np.int32))
    # a new graph clears it (p2pg_load_csr)
    with gpu_net(g, "flood", count_received=False) as net:
        net.set_netsplit(side, 0, 9)
        net._check(L.p2pg_load_csr(net._h, g.V, _lib.ptr(g.rowptr), _lib.ptr(g.colidx)))
        net.broadcast([10])
        assert net.step().received_exact == 1 and len(net.snapshot()) > 0
