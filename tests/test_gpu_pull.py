"""Anti-entropy (p2pg_set_anti_entropy) on the GPU: the engine, through the C-ABI, against the pull/
fixtures of the reference's own Node objects and against tests/pull_ref.py (pinned to those
fixtures on the CPU, tests/test_pull.py) -- bit-exact hop, parent, delivered set, the exchange
records, send lists (the excluded connection of a pulled flood receipt is the partner), delivery
streams, tallies and every per-round counter the contract defines (touched_words and the push form
of an arrival round are the engine's)."""
import functools
import zlib

import numpy as np
import pytest

import pull_ref
from test_gpu_late import FLOOD_KEYS, assert_planes, gpu_net
from test_pull import PULL_CASES, cfg_of, load_pull, ref_of, setting_of, star_with_chains

pytestmark = pytest.mark.gpu

CHURN = 430_000_000
FOREVER = pull_ref.FOREVER
ATOMIC, EDGE, FUSED, UPDATE_EDGE = 1, 2, 3, 4  # p2pg_round_stats.push_form


def assert_rounds(rounds, ref, mode, setting, last_start=0):
    """Every counter of every round; the run goes on while receipts, starts, a request round or an
    exchange in flight lie ahead, and stops then."""
    assert len(rounds) == len(ref.rounds), (len(rounds), len(ref.rounds))
    for i, (a, b) in enumerate(zip(rounds, ref.rounds)):
        assert a.round == i and a.received_exact == 1, (i, a.received_exact)
        for k in FLOOD_KEYS:
            assert getattr(a, k) == b[k], (i, k, getattr(a, k), b[k])
        if mode == "gossip":
            assert a.scatter_words == b["scatter_words"], (i, a.scatter_words, b["scatter_words"])
        want = b["new_deliveries"] or last_start > i or pull_ref.arrival_ahead(i + 1, setting)
        assert a.active == (1 if want else 0), (i, a.active)


def assert_records(net, ref):
    ps = net.pull_stats()
    got = np.array([[int(x[k]) for k in pull_ref.RECORD] for x in ps], dtype=np.int64).reshape(-1, 6)
    np.testing.assert_array_equal(got, ref.records())


def assert_tallies(net, ref):
    got = ref.hop >= 0
    t = net.message_tally()
    np.testing.assert_array_equal(t.reach, got.sum(axis=0))
    np.testing.assert_array_equal(t.hop_sum, np.where(got, ref.hop, 0).sum(axis=0))
    np.testing.assert_array_equal(t.last_hop, ref.hop.max(axis=0))
    c = net.peer_counters()
    np.testing.assert_array_equal(c.sent, ref.peer_sent)
    np.testing.assert_array_equal(c.received, ref.peer_recv)


def assert_step(net, ref, r):
    """After stepping round r: its send list with the lost flags and its delivery stream."""
    s = net.sends()
    snd, rcv, msg, lost = ref.sends[r]
    np.testing.assert_array_equal(s.sender, snd)
    np.testing.assert_array_equal(s.receiver, rcv)
    np.testing.assert_array_equal(s.msg, msg)
    np.testing.assert_array_equal(s.lost, lost)
    d = net.deliveries()
    peers, msgs = np.nonzero(ref.hop == r)
    np.testing.assert_array_equal(d.peer, peers)
    np.testing.assert_array_equal(d.msg, msgs)
    np.testing.assert_array_equal(d.parent, ref.parent[peers, msgs])


def pulled_excludes_partner(ref, rowptr):
    """Some pulled flood receipt whose parent is the partner is relayed on: its send list holds every
    connection of the peer but the partner."""
    for r, pulled in enumerate(ref.pulled):
        us, ms = np.nonzero(pulled & (ref.parent == ref.partner[r][:, None]))
        for u, m in zip(us.tolist(), ms.tolist()):
            if rowptr[u + 1] - rowptr[u] >= 2:
                snd, rcv, msg, _ = ref.sends[r]
                to = rcv[(snd == u) & (msg == m)]
                assert ref.partner[r][u] not in to and len(to) == rowptr[u + 1] - rowptr[u] - 1
                return True
    return False


# ---- 1. the four fixtures of the reference's own Node objects -----------------------------------
@pytest.mark.parametrize("name", PULL_CASES)
def test_pull_fixture_through_the_c_abi(name):
    z = load_pull(name)
    c = cfg_of(z)
    mode = c["mode"]
    period, first, last = setting_of(z)
    ref = ref_of(name)
    with gpu_net(z, mode, c["fanout"], c["gossip_seed"], c["churn_threshold"], c["churn_seed"], record=True,
                 tally=True) as net:
        net.broadcast(z["src"], z["start"])
        net.set_downtime(z["down_from"], z["down_until"])
        net.set_anti_entropy(period, first, last, seed=int(z["pull_seed"]))
        assert net.anti_entropy == (period, first, last, int(z["pull_seed"]))
        for r, v in ((first, 0), (first + period, 17), (last, 101)):
            assert net.pull_partner(r, v) == int(pull_ref.partners(r, z["rowptr"], z["colidx"], int(z["pull_seed"]))[v])
        rounds = net.run()
        hop, parent = net.hop_parent()
        np.testing.assert_array_equal(hop, z["hop"])
        np.testing.assert_array_equal(parent, z["parent"])
        np.testing.assert_array_equal(net.delivered(), z["hop"] >= 0)
        assert pull_ref.pad_equal([r.relays for r in rounds], z["round_relays"])
        assert net.message_count_send == int(z["round_relays"].sum())
        assert sum(r.received for r in rounds) == int(z["total_recv"])
        ps = net.pull_stats()
        np.testing.assert_array_equal(
            np.array([[int(x[k]) for k in pull_ref.RECORD] for x in ps], dtype=np.int64).reshape(-1, 6), z["exchanges"])
        assert_rounds(rounds, ref, mode, (period, first, last), int(z["start"].max()))
        assert_planes(net, ref)
        assert_tallies(net, ref)
        cnt = net.peer_counters()
        np.testing.assert_array_equal(cnt.sent, z["peer_sent"])
        np.testing.assert_array_equal(cnt.received, z["peer_recv"])
        # the send lists and delivery streams of every round, stepping the replay
        net.reset()
        assert len(net.pull_stats()) == 0
        for r in range(len(ref.rounds)):
            st = net.step()
            assert st.relays == ref.rounds[r]["relays"]
            if st.new_deliveries:
                assert_step(net, ref, r)
        assert not st.active
        assert_records(net, ref)
    if mode == "flood":
        assert pulled_excludes_partner(ref, z["rowptr"])


# ---- 2. flood sweep against pull_ref ----------------------------------------------------------------
FLOOD_CASES = [(V, M, thr) for V in (33, 200) for M in (1, 63, 64, 65, 130, 200) for thr in (0, CHURN)]
FLOOD_CASES += [(40, 2100, CHURN), (40, 4160, 0), (40, 4160, CHURN)]


def graph_of(V, seed, kind=None):
    """Regular, small-world, scale-free with a hub, and a sparse G(n, p) with isolated peers."""
    from p2pnetwork.gpu import PeerGraph
    kind = seed % 4 if kind is None else kind
    if kind == 0:
        return PeerGraph.random_regular(V, 4, seed)
    if kind == 1:
        return PeerGraph.watts_strogatz(V, 4, 0.2, seed)
    if kind == 2:
        return PeerGraph.barabasi_albert(V, 2, seed)
    return PeerGraph.gnp(V, 2.5, seed)


def outages(V, seed, src, start, last=9):
    """A quarter of the peers: late joiners, crashes and outages of one to three rounds, none
    holding one of the peer's own originations."""
    rng = np.random.default_rng(seed)
    f = np.full(V, -1, dtype=np.int32)
    u = np.full(V, FOREVER, dtype=np.int32)
    own = {}
    for p, s in zip(np.asarray(src).tolist(), np.asarray(start).tolist()):
        own.setdefault(p, []).append(s)
    for v in rng.permutation(V)[:max(V // 4, 4)].tolist():
        kind = int(rng.integers(0, 8))
        a = 0 if kind == 0 else int(rng.integers(1, last))
        b = FOREVER if kind == 1 else a + int(rng.integers(1, 4))
        if not any(a <= s < b for s in own.get(v, [])):
            f[v], u[v] = a, b
    return f, u


@pytest.mark.parametrize("V,M,cthr", FLOOD_CASES)
def test_pull_flood_matches_pull_ref(V, M, cthr):
    from p2pnetwork.gpu import make_sources
    seed = zlib.crc32(repr((V, M, cthr)).encode()) & 0xFFFF
    g = graph_of(V, seed)
    rng = np.random.default_rng(seed)
    src = make_sources(g.V, M, seed=seed).astype(np.int32)
    src[g.degree()[src] == 0] = int(np.argmax(g.degree()))  # (an isolated origin floods nothing)
    start = rng.integers(0, 4, M).astype(np.int32)
    start[0] = 0 if M > 1 else 1
    f, u = outages(g.V, seed, src, start)
    setting = ((1, 4)[(seed >> 2) % 2], 1 + (seed >> 3) % 3, 14)  # (drawn apart from the graph kind, seed % 4)
    kw = dict(mode="flood", fanout=3, gossip_seed=seed + 1, churn_threshold=cthr, churn_seed=seed + 2)
    ref = pull_ref.run(g.rowptr, g.colidx, src, start, f, u, anti_entropy=setting, pull_seed=seed + 3, **kw)
    # (a flood without churn may lose nothing that a pull could repair; under churn every case does)
    assert ref.records()[:, 5].sum() > 0 or not cthr, "nothing repaired: the case is vacuous"
    with gpu_net(g, "flood", 3, seed + 1, cthr, seed + 2, tally=True) as net:
        net.broadcast(src, start)
        net.set_downtime(f, u)
        net.set_anti_entropy(*setting, seed=seed + 3)
        rounds = net.run()
        assert_rounds(rounds, ref, "flood", setting, int(start.max()))
        assert_planes(net, ref)
        assert_tallies(net, ref)
        assert_records(net, ref)


# ---- 3. gossip sweep: row widths x push forms -------------------------------------------------------
# W -> M: the widths the issue names through their message counts (1 .. 4160), and the grouped
# kernels' widths through 64 * W
GOSSIP_M = {1: 63, 2: 65, 3: 192, 4: 200, 8: 512, 9: 576, 16: 1024, 17: 1088, 32: 2048, 33: 2100, 65: 4160}


def gossip_case(W):
    """Every message from one of 20 origins, an eighth of them in round 2; a quarter of the peers
    with downtime; 8 % churn at the odd widths; anti-entropy of period 1 (even widths) or 4."""
    from p2pnetwork.gpu import PeerGraph, make_sources
    g = PeerGraph.barabasi_albert(300 if W <= 17 else 120, 3, seed=50 + W)
    M = GOSSIP_M[W]
    src = (make_sources(20, M, seed=W) * 5 + 2).astype(np.int32)
    start = np.zeros(M, dtype=np.int32)
    start[np.random.default_rng(W).integers(0, M, max(M // 8, 1))] = 2
    f, u = outages(g.V, 200 + W, src, start, last=7)
    setting = (1 if W % 2 == 0 else 4, 1 + W % 3, 12)
    return g, src, start, f, u, setting, (CHURN if W % 2 else 0)


@functools.lru_cache(maxsize=2)  # the push forms of one width run back to back
def gossip_ref(W):
    g, src, start, f, u, setting, cthr = gossip_case(W)
    return pull_ref.run(g.rowptr, g.colidx, src, start, f, u, anti_entropy=setting, pull_seed=77 + W, mode="gossip",
                        fanout=3, gossip_seed=11, churn_threshold=cthr, churn_seed=5)


@pytest.mark.parametrize("W", sorted(GOSSIP_M))
@pytest.mark.parametrize("push", ["atomic", "store", "auto"])
def test_pull_gossip_push_forms(W, push, monkeypatch):
    """Whole-row E (W <= 8), packed E with AW masks (8 < W <= 64), the narrow gather's groupings
    (1, 2, 4, 8, 16, 32 lanes per peer), the 64-lane edge, two slices."""
    if push != "auto":
        monkeypatch.setenv("P2PG_GOSSIP_PUSH", push)
    else:  # the thresholds test_late_gossip_push_forms sets: small graphs enter dense rounds
        monkeypatch.setenv("P2PG_E_THRESH", "0.05")
        monkeypatch.setenv("P2PG_V_THRESH", "0.3")
        monkeypatch.setenv("P2PG_UPDATE_PUSH", "1")
    g, src, start, f, u, setting, cthr = gossip_case(W)
    assert (len(src) + 63) // 64 == W
    ref = gossip_ref(W)
    assert ref.records()[:, 5].sum() > 0
    with gpu_net(g, "gossip", 3, 11, cthr, 5, tally=True) as net:
        net.broadcast(src, start)
        net.set_downtime(f, u)
        net.set_anti_entropy(*setting, seed=77 + W)
        rounds = net.run()
        assert_rounds(rounds, ref, "gossip", setting, 2)
        assert_planes(net, ref)
        assert_tallies(net, ref)
        assert_records(net, ref)
    arrivals = {r + 2 for r in range(setting[1], setting[2] + 1, setting[0])}
    forms = [x.push_form for x in rounds]
    assert all(forms[r] in (ATOMIC, EDGE) for r in arrivals if r < len(forms)), forms
    if push == "atomic":
        assert set(forms) == {ATOMIC}
    # without records, tallies or the lost count: the same receipts and relays
    with gpu_net(g, "gossip", 3, 11, cthr, 5, record=False, count_received=False) as net:
        net.broadcast(src, start)
        net.set_downtime(f, u)
        net.set_anti_entropy(*setting, seed=77 + W)
        lean = net.run()
        np.testing.assert_array_equal(net.delivered(), ref.hop >= 0)
        assert_records(net, ref)
    assert [(x.new_deliveries, x.relays) for x in lean] == [(x.new_deliveries, x.relays) for x in rounds]


# ---- 3b. gossip on every graph kind, at the message counts the width sweep leaves out -----------------
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("M", [1, 64, 130])
def test_pull_gossip_graph_kinds(kind, M):
    """Regular, small-world, scale-free and G(n, p) with isolated peers; k = 2, so the 4-regular and
    small-world peers pick among their connections too; churn at the odd kinds; periods 1 and 4."""
    from p2pnetwork.gpu import make_sources
    seed = zlib.crc32(repr(("gossip", kind, M)).encode()) & 0xFFFF
    g = graph_of(200, seed, kind)
    if kind == 3:
        assert (g.degree() == 0).any()
    rng = np.random.default_rng(seed)
    src = make_sources(g.V, M, seed=seed).astype(np.int32)
    src[g.degree()[src] == 0] = int(np.argmax(g.degree()))
    start = rng.integers(0, 4, M).astype(np.int32)
    start[0] = 0 if M > 1 else 1
    f, u = outages(g.V, seed, src, start)
    setting = ((1, 4)[(seed >> 2) % 2], 1 + (seed >> 3) % 3, 14)
    cthr = CHURN if kind % 2 else 0
    ref = pull_ref.run(g.rowptr, g.colidx, src, start, f, u, anti_entropy=setting, pull_seed=seed + 3, mode="gossip",
                       fanout=2, gossip_seed=seed + 1, churn_threshold=cthr, churn_seed=seed + 2)
    # (one message on the sparse G(n, p) may die out before anybody misses it)
    assert ref.records()[:, 5].sum() > 0 or M == 1, "nothing repaired: the case is vacuous"
    with gpu_net(g, "gossip", 2, seed + 1, cthr, seed + 2, tally=True) as net:
        net.broadcast(src, start)
        net.set_downtime(f, u)
        net.set_anti_entropy(*setting, seed=seed + 3)
        rounds = net.run()
        assert_rounds(rounds, ref, "gossip", setting, int(start.max()))
        assert_planes(net, ref)
        assert_tallies(net, ref)
        assert_records(net, ref)


# ---- 4. the dense phase, run == stepping, reset, removal ------------------------------------------
@functools.lru_cache(maxsize=None)
def dense_graph():
    from p2pnetwork.gpu import PeerGraph, make_sources
    g = PeerGraph.barabasi_albert(2000, 4, seed=3)
    return g, make_sources(g.V, 4096, seed=3)


def dense_run(setting=None, down=None, stepping=False, twice=False):
    g, src = dense_graph()
    with gpu_net(g, "gossip", 3, 0x5EED, record=False, count_received=False) as net:
        net.broadcast(src)
        if down is not None:
            net.set_downtime(*down)
        if setting:
            net.set_anti_entropy(*setting, seed=9)
        if twice:
            net.run()
            net.reset()
        if stepping:
            rounds = []
            while True:
                rounds.append(net.step())
                if not rounds[-1].active:
                    break
        else:
            rounds = net.run()
        stats = net.pull_stats() if setting else None
        return rounds, net.seen_plane(), stats


@functools.lru_cache(maxsize=None)
def dense_base():
    return dense_run()


def test_pull_arrival_round_inside_the_fused_rounds():
    g, src = dense_graph()
    f = np.full(g.V, -1, dtype=np.int32)
    u = np.full(g.V, FOREVER, dtype=np.int32)
    late = np.random.default_rng(4).permutation(g.V)[:g.V // 10]
    late = late[~np.isin(late, src)]
    f[late], u[late] = 0, 4  # late joiners: back long before the dense rounds, with holes to repair
    no_pull, _, _ = dense_run(down=(f, u))
    forms = [r.push_form for r in no_pull]
    inside = [r for r in range(7, len(forms) - 1) if forms[r - 1] == forms[r] == forms[r + 1] == FUSED]
    assert inside, forms
    a = inside[0]  # one arrival round inside the fused rounds, fused rounds on both sides
    setting = (4, a - 2, a - 2)  # one exchange: requests in a - 2, arrival in a
    rounds, seen, stats = dense_run(setting, down=(f, u))
    # every field of every round before the arrival round, push_form included: request and reply
    # rounds launch nothing and are planned as without the call
    assert rounds[:a] == no_pull[:a]
    assert rounds[a].push_form in (ATOMIC, EDGE) and no_pull[a].push_form == FUSED, [x.push_form for x in rounds]
    assert any(x.push_form == FUSED for x in rounds[a + 1:]), [x.push_form for x in rounds]
    ref = pull_ref.run(g.rowptr, g.colidx, src, np.zeros(len(src), dtype=np.int32), f, u, anti_entropy=setting,
                       pull_seed=9, mode="gossip", fanout=3, gossip_seed=0x5EED, planes=False)
    assert len(rounds) == len(ref.rounds)
    for i, (x, y) in enumerate(zip(rounds, ref.rounds)):
        for k in ("new_deliveries", "relays", "active_vertices", "active_words", "wedges", "deg_active"):
            assert getattr(x, k) == y[k], (i, k)
    bits = np.unpackbits(seen.view(np.uint8).reshape(g.V, -1), axis=1, bitorder="little")[:, :len(src)]
    np.testing.assert_array_equal(bits.astype(bool), ref.hop >= 0)
    got = np.array([[int(x[k]) for k in pull_ref.RECORD] for x in stats], dtype=np.int64).reshape(-1, 6)
    np.testing.assert_array_equal(got, ref.records())
    assert got[0, 5] > 0
    # run() == stepping, and a second run after reset is the first
    stepped, seen2, stats2 = dense_run(setting, down=(f, u), stepping=True)
    assert [(x.new_deliveries, x.relays, x.active) for x in stepped] == [(x.new_deliveries, x.relays, x.active) for x in rounds]
    np.testing.assert_array_equal(seen2, seen)
    np.testing.assert_array_equal(stats2, stats)
    again, seen3, stats3 = dense_run(setting, down=(f, u), twice=True)
    assert again == rounds
    np.testing.assert_array_equal(seen3, seen)
    np.testing.assert_array_equal(stats3, stats)


def test_removed_anti_entropy_is_an_engine_that_never_saw_the_call():
    g, src = dense_graph()
    base, seen0, _ = dense_base()
    with gpu_net(g, "gossip", 3, 0x5EED, record=False, count_received=False) as net:
        net.broadcast(src)
        net.set_anti_entropy(1, 2, 9, seed=3)
        net.set_anti_entropy(None)
        assert net.anti_entropy is None
        rounds = net.run()
        assert rounds == base  # every field of every round, push_form included
        np.testing.assert_array_equal(net.seen_plane(), seen0)
        assert len(net.pull_stats()) == 0
        assert len(net.snapshot()) > 0  # (and snapshots work again)


# ---- 5. the hand case ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["flood", "gossip"])
def test_the_hand_case_of_the_two_pass_split_on_the_engine(mode):
    """tests/test_pull.py::star_with_chains: leaf 4's partner 2 gets the message by relay in the very
    round in which 4's (empty) reply arrives; 4 gets it one round later.  (Gossip with k = 3 >= every
    degree sends to every connection: the same receipts, parents and hops.)"""
    from p2pnetwork.gpu import PeerGraph
    rowptr, colidx, src, start, setting = star_with_chains()
    g = PeerGraph(rowptr, colidx)
    for seed in (0, 1, 2, 3):
        with gpu_net(g, mode, 3, 1, 0, 0, tally=True) as net:
            net.broadcast(src, start)
            net.set_anti_entropy(*setting, seed=seed)
            rounds = net.run()
            hop, parent = net.hop_parent()
            assert hop[:, 0].tolist() == [2, 1, 3, 0, 4]
            assert parent[:, 0].tolist() == [1, 3, 0, -1, 2]
            assert len(rounds) == 6 and [r.active for r in rounds] == [1, 1, 1, 1, 1, 0]
            ps = net.pull_stats()
            assert [[int(x[k]) for k in pull_ref.RECORD] for x in ps] == [[1, 5, 0, 5, 0, 0], [2, 5, 0, 5, 0, 0],
                                                                         [3, 5, 0, 5, 0, 0]]


# ---- 6. refusals --------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_unchanged():
    from p2pnetwork.gpu import P2PGError, PeerGraph, make_sources
    g = PeerGraph.random_regular(64, 4, 5)
    src = make_sources(g.V, 70, seed=5).astype(np.int32)
    ref = pull_ref.run(g.rowptr, g.colidx, src, np.zeros(70, dtype=np.int32), anti_entropy=(1, 1, 5), pull_seed=4,
                       mode="flood")
    # the other call order of the partitioned rank: global ids first, then the setting
    with gpu_net(g, "flood", 3, 1, 0, 0) as net:
        net.broadcast(src)
        net.set_global_ids(np.arange(g.V, dtype=np.int32))
        with pytest.raises(P2PGError, match="vertex-partitioned"):
            net.set_anti_entropy(1, 1, 5, seed=4)
        assert net.anti_entropy is None and len(net.pull_stats()) == 0
    with gpu_net(g, "flood", 3, 1, 0, 0) as net:
        net.broadcast(src)
        for bad in ((1, -1, 5), (1, 3, 2), (-1, 0, 5)):
            with pytest.raises(P2PGError):
                net.set_anti_entropy(*bad)
            assert net.anti_entropy is None
        # hop limits first: anti-entropy is refused; anti-entropy first: finite hop limits are
        net.set_ttl(np.full(70, 3, dtype=np.int32))
        with pytest.raises(P2PGError, match="hop limits"):
            net.set_anti_entropy(1, 1, 5, seed=4)
        net.set_ttl(None)
        net.set_relay_policy(thresholds=np.full(g.V, 1 << 31, dtype=np.uint32), seed=1)
        with pytest.raises(P2PGError, match="relay policy"):
            net.set_anti_entropy(1, 1, 5, seed=4)
        net.set_relay_policy(None)
        net.set_anti_entropy(1, 1, 5, seed=4)
        with pytest.raises(P2PGError, match="anti-entropy"):
            net.set_ttl(np.full(70, 3, dtype=np.int32))
        net.set_ttl(np.full(70, -1, dtype=np.int32))  # (no finite limit: nothing to refuse)
        with pytest.raises(P2PGError, match="anti-entropy"):
            net.set_relay_policy(thresholds=np.full(g.V, 1 << 31, dtype=np.uint32), seed=1)
        with pytest.raises(P2PGError, match="anti-entropy"):
            net.snapshot()
        with pytest.raises(P2PGError, match="anti-entropy"):  # (refused before the buffer is looked at)
            net.restore(np.zeros(4096, dtype=np.uint8))
        with pytest.raises(P2PGError, match="anti-entropy"):
            net.set_global_ids(np.arange(g.V, dtype=np.int32))
        net.step_begin()
        with pytest.raises(P2PGError, match="begun"):
            net.set_anti_entropy(1, 2, 5, seed=4)
        net.step_end()
        with pytest.raises(P2PGError, match="a round has run"):
            net.set_anti_entropy(1, 2, 5, seed=4)
        with pytest.raises(P2PGError, match="anti-entropy"):
            net.update_edges(add=[(0, 63)] if 63 not in g.neighbours(0) else [(0, 62)])
        with pytest.raises(P2PGError, match="anti-entropy"):
            net.drop_relays([0], [0])
        assert net.anti_entropy == (1, 1, 5, 4)
        # every refusal left the engine as it was: the run is the reference's
        net.reset()
        rounds = net.run()
        assert_rounds(rounds, ref, "flood", (1, 1, 5))
        assert_planes(net, ref)
        assert_records(net, ref)
