"""GPU: the delivery latency computed on the device (p2pg_message_latency: per broadcast the
histogram of its first receipts by relative hop; p2pg_peer_latency: per peer their sum, number and
largest) against the host reference tests/latency_ref.py (pinned by tests/test_latency.py) of the
hop planes the reference's own Node objects produced (the fixtures' z["hop"] / z["start"]) and,
for shapes without a fixture, of a record=True twin engine's hop plane.  Every comparison is
integer-exact."""
import numpy as np
import pytest

import latency_ref
from conftest import golden_cases, load_golden, updates_of
from p2pnetwork.gpu import _lib
from p2pnetwork.gpu._lib import P2PGError
from test_cost import FEATURE_CASES, load_feature
from test_gpu_cost import assert_cost, feature_net
from test_gpu_tally import net_of, results, run_steps

pytestmark = pytest.mark.gpu


def assert_latency(net, hop, start, bins=64, upto=None):
    want = latency_ref.latency(hop, start, bins, upto)
    hist, p = net.message_latency(), net.peer_latency()
    assert hist.dtype == np.uint64 and hist.shape == (hop.shape[1], bins)
    assert p.hop_sum.dtype == np.uint64 and p.receipts.dtype == np.uint32 and p.max_hop.dtype == np.int32
    np.testing.assert_array_equal(hist, want.hist)
    np.testing.assert_array_equal(p.receipts, want.receipts)
    np.testing.assert_array_equal(p.hop_sum, want.hop_sum)
    np.testing.assert_array_equal(p.max_hop, want.max_hop)
    np.testing.assert_array_equal(p.mean(), latency_ref.mean(want))
    return hist, p


# 1 -- every static fixture, by run() and by step(); the flag changes no result of the run
@pytest.mark.parametrize("how", ["run", "step"])
@pytest.mark.parametrize("name", golden_cases())
def test_latency_matches_reference(name, how):
    z = load_golden(name)
    with net_of(z) as plain:
        plain.broadcast(z["src"])
        want_rounds = results(plain.run())
        want_seen = plain.seen_plane()
    with net_of(z, latency=True) as net:
        net.broadcast(z["src"])
        rounds = net.run() if how == "run" else run_steps(net)
        hist, p = assert_latency(net, z["hop"], latency_ref.start_of(z))
        reach = net.message_reach()
        np.testing.assert_array_equal(hist.sum(axis=1), reach)
        assert int(p.receipts.sum()) == int(reach.sum())
        assert int(p.hop_sum.sum()) == int((hist.astype(np.int64) * np.arange(64)[None, :]).sum())
        assert results(rounds) == want_rounds
        np.testing.assert_array_equal(net.seen_plane(), want_seen)
        np.testing.assert_array_equal(net.coverage_curve(), latency_ref.coverage_curve(hist))
        np.testing.assert_array_equal(net.coverage_curve(of="peers"), latency_ref.coverage_curve(hist, hop_V(z)))
        for q in (0.5, 0.9, 0.99, 1.0):
            np.testing.assert_array_equal(net.latency_percentile(q), latency_ref.percentile(hist, q))


def hop_V(z):
    return z["hop"].shape[0]


@pytest.mark.parametrize("name", golden_cases(dynamic=True))
def test_latency_with_topology_updates(name):
    z = load_golden(name)
    upd = updates_of(z)
    with net_of(z, latency=True) as net:
        net.broadcast(z["src"])
        while True:
            st = net.step()
            if st.round in upd:
                net.update_edges(*upd[st.round])
            if not st.active:
                break
        assert_latency(net, z["hop"], latency_ref.start_of(z))


# 2 -- start rounds, hop limits, the relay policy, downtime, anti-entropy: the reference's planes
NARROW = [c for c in FEATURE_CASES if c[1].endswith(("rrg200_flood", "ba300_gossip_k2_churn10"))]


@pytest.mark.parametrize("kind,name,bins", [c + (64,) for c in FEATURE_CASES] + [c + (8,) for c in NARROW])
def test_latency_composes_with_the_per_message_features(kind, name, bins):
    z = load_feature(kind, name)
    with feature_net(z, latency=True, latency_bins=bins) as net:
        rounds = net.run()
        hist, p = assert_latency(net, z["hop"], z["start"], bins)
        np.testing.assert_array_equal(hist.sum(axis=1), net.message_reach())
        # a step-by-step replay read at three boundaries: the receipts of the rounds so far
        net.reset()
        for i in range(len(rounds)):
            st = net.step()
            if i in (1, 3, len(rounds) - 1):
                assert_latency(net, z["hop"], z["start"], bins, upto=st.round)
        assert st.round == rounds[-1].round


# 3 -- row widths: lanes past the row, a tail word, 16 and 4 rows per load, a whole slice, a second
# slice of one word; V = 3001 is no multiple of the 32-peer task.  Staggered starts and one message
# per word far behind: 7 planes, the sum and the minimum differ per word.
@pytest.fixture(scope="module")
def ba3001():
    from p2pnetwork.gpu import PeerGraph
    return PeerGraph.barabasi_albert(3001, 4, seed=9)


def twin_latency(g, src, start, mode, k=3, gseed=11, bins=64):
    from p2pnetwork.gpu import GraphNetwork
    kw = dict(mode=mode, fanout=k, gossip_seed=gseed)
    with GraphNetwork(g, latency=True, latency_bins=bins, **kw) as net, GraphNetwork(g, record=True, **kw) as rec:
        net.broadcast(src, start)
        rec.broadcast(src, start)
        rounds = net.run()
        assert results(rec.run()) == results(rounds)
        hop, _ = rec.hop_parent()
        st = np.zeros(len(src), dtype=np.int64) if start is None else np.asarray(start)
        hist, p = assert_latency(net, hop, st, bins)
        np.testing.assert_array_equal(hist.sum(axis=1), net.message_reach())
    return hist, p


def staggered(M):
    start = (np.arange(M) % 5).astype(np.int32)
    start[::64] = 70
    return start


@pytest.mark.parametrize("M,mode", [(1, "gossip"), (63, "gossip"), (64, "gossip"), (65, "gossip"), (200, "gossip"),
                                    (1000, "gossip"), (4096, "gossip"), (4100, "flood")])
def test_row_widths(ba3001, M, mode):
    from p2pnetwork.gpu import make_sources
    hist, p = twin_latency(ba3001, make_sources(ba3001.V, M, seed=3), staggered(M), mode)
    assert (hist[:, 0] == 1).all() and int(p.max_hop.max()) > 0  # (the originations are receipts of hop 0)


@pytest.mark.parametrize("M", [65, 4096])
def test_all_starts_zero_needs_no_planes(ba3001, M):
    from p2pnetwork.gpu import make_sources
    twin_latency(ba3001, make_sources(ba3001.V, M, seed=3), None, "gossip")


# 4 -- small populations
def test_single_peer():
    from p2pnetwork.gpu import PeerGraph
    g = PeerGraph(np.zeros(2, dtype=np.int64), np.zeros(0, dtype=np.int32))
    hist, p = twin_latency(g, np.zeros(3, dtype=np.int32), np.array([0, 2, 1], dtype=np.int32), "flood")
    np.testing.assert_array_equal(p.receipts, [3])
    np.testing.assert_array_equal(p.max_hop, [0])


def test_ring_of_33_second_activity_word():
    from p2pnetwork.gpu import PeerGraph
    ring = np.arange(33)
    g = PeerGraph.from_edges(33, np.stack([ring, (ring + 1) % 33], axis=1).astype(np.int32))
    src = np.array([32, 0, 16, 32], dtype=np.int32)
    hist, p = twin_latency(g, src, np.array([0, 1, 0, 3], dtype=np.int32), "flood")
    assert int(p.max_hop[32]) == 16 and int(p.receipts[32]) == 4


def test_star_of_40_one_hub_row():
    from p2pnetwork.gpu import PeerGraph
    g = PeerGraph.from_edges(40, np.array([(0, i) for i in range(1, 40)], dtype=np.int32))
    src = np.array([0, 0, 7] + [0] * 67, dtype=np.int32)
    hist, p = twin_latency(g, src, np.array([0, 2, 1] + [0] * 67, dtype=np.int32), "flood")
    np.testing.assert_array_equal(hist[0, :3], [1, 39, 0])
    np.testing.assert_array_equal(hist[2, :3], [1, 1, 38])


# 5 -- p2pg_originate: the schedule grows mid-run, and with it the number of planes
def test_originate_raises_the_plane_count_mid_run():
    from p2pnetwork.gpu import GraphNetwork, PeerGraph, make_sources
    g = PeerGraph.barabasi_albert(400, 3, seed=12)
    M = 130
    src = make_sources(g.V, M, seed=12).astype(np.int32)
    start = np.random.default_rng(12).integers(0, 2, M).astype(np.int32)  # (1 plane)
    late = np.arange(1, M, 2)
    peers = src[late].copy()
    src[late] = -1
    start[late] = -1
    kw = dict(mode="gossip", fanout=2, gossip_seed=31)
    with GraphNetwork(g, latency=True, **kw) as net, GraphNetwork(g, record=True, **kw) as rec:
        net.broadcast(src, start)
        for _ in range(3):
            net.step()
        assert not net.message_latency()[late].any()
        net.originate(late[:30], peers[:30], round=3)  # 2 planes
        first = net.run()
        assert not first[-1].active
        net.originate(late[30:], peers[30:], round=max(first[-1].round + 5, 64))  # 7 planes
        more = net.run()
        assert more[-1].round > 64 and int(net.start_rounds.max()).bit_length() == 7
        rec.broadcast(net.sources, net.start_rounds)
        rec.run()
        hop, _ = rec.hop_parent()
        hist, p = assert_latency(net, hop, net.start_rounds)
        assert (hist[late].sum(axis=1) > 1).all()
        net.reset()  # keeps the schedule (originate included) and replays it
        assert not net.message_latency().any() and not net.peer_latency().receipts.any()
        net.run()
        assert_latency(net, hop, net.start_rounds)


# 6 -- all three flags: one column count serves both folds, every result is what its flag gives alone
@pytest.mark.parametrize("name", ["c2_rrg1000_flood", "ba1000_gossip_k3"])
def test_all_three_flags_together(name):
    z = load_golden(name)
    alone = {}
    for flag in ("tally", "cost", "latency"):
        with net_of(z, **{flag: True}) as one:
            one.broadcast(z["src"])
            one.run()
            if flag == "tally":
                alone[flag] = (one.message_tally(), one.peer_counters())
            elif flag == "cost":
                alone[flag] = one.message_cost()
            else:
                alone[flag] = (one.message_latency(), one.peer_latency())
    with net_of(z, tally=True, cost=True, latency=True) as net:
        net.broadcast(z["src"])
        for rep in range(2):  # (and again after a reset: the shared shards were left zero)
            net.run()
            hist, p = assert_latency(net, z["hop"], latency_ref.start_of(z))
            t, pc, c = net.message_tally(), net.peer_counters(), net.message_cost()
            for a, b in zip(t + pc, alone["tally"][0] + alone["tally"][1]):
                np.testing.assert_array_equal(a, b)
            assert_cost(c, alone["cost"])
            np.testing.assert_array_equal(hist, alone["latency"][0])
            for a, b in zip(p, alone["latency"][1]):
                np.testing.assert_array_equal(a, b)
            # the cross-identities (every start is 0)
            b = np.arange(64, dtype=np.uint64)
            np.testing.assert_array_equal(hist.sum(axis=1), t.reach)
            np.testing.assert_array_equal((hist * b[None, :]).sum(axis=1), t.hop_sum)
            np.testing.assert_array_equal([np.nonzero(row)[0][-1] for row in hist], t.last_hop)
            assert int(p.hop_sum.sum()) == int(t.hop_sum.sum())
            net.reset()


def test_tally_identities_with_late_starts():
    z = load_feature("late", "late_ba300_gossip_k2_churn10")
    with feature_net(z, tally=True, latency=True) as net:
        net.run()
        hist, p = assert_latency(net, z["hop"], z["start"])
        t = net.message_tally()
    start = z["start"].astype(np.int64)
    b = np.arange(64, dtype=np.int64)
    np.testing.assert_array_equal((hist.astype(np.int64) * b[None, :]).sum(axis=1),
                                  t.hop_sum.astype(np.int64) - start * t.reach.astype(np.int64))
    np.testing.assert_array_equal([np.nonzero(row)[0][-1] for row in hist], t.last_hop - start)


# 7 -- lifecycle and refusals
def test_reset_and_new_sources_zero_the_counters_and_keep_the_bins():
    z = load_golden("ba1000_gossip_k3")
    with net_of(z, latency=True, latency_bins=16) as net:
        net.broadcast(z["src"])
        net.run()
        h1, p1 = assert_latency(net, z["hop"], latency_ref.start_of(z), 16)
        h2, p2 = net.message_latency(), net.peer_latency()  # reading twice: the same values
        np.testing.assert_array_equal(h1, h2)
        for a, b in zip(p1, p2):
            np.testing.assert_array_equal(a, b)
        net.reset()
        assert net.message_latency().shape == (len(z["src"]), 16) and not net.message_latency().any()
        p0 = net.peer_latency()
        assert not p0.hop_sum.any() and not p0.receipts.any() and (p0.max_hop == -1).all()
        assert np.isnan(p0.mean()).all() and np.isnan(net.coverage_curve()).all()
        assert (net.latency_percentile(0.5) == -1).all()
        net.run()
        np.testing.assert_array_equal(net.message_latency(), h1)
        net.broadcast(z["src"][::-1].copy())
        assert net.message_latency().shape == (len(z["src"]), 16) and not net.message_latency().any()
        assert not net.peer_latency().receipts.any()
        net.step()  # round 0: the originations, hop 0 at the origins
        h = net.message_latency()
        assert (h[:, 0] == 1).all() and not h[:, 1:].any()
        np.testing.assert_array_equal(net.peer_latency().receipts,
                                      np.bincount(z["src"], minlength=len(z["rowptr"]) - 1))


def test_reading_refuses_nothing_afterwards():
    from p2pnetwork.gpu import GraphNetwork, PeerGraph, make_sources
    g = PeerGraph.random_regular(300, 6, seed=8)
    src = make_sources(g.V, 100, seed=9)
    with GraphNetwork(g, mode="flood", latency=True) as net, GraphNetwork(g, mode="flood", record=True) as rec:
        net.broadcast(src)
        rec.broadcast(src)
        while True:
            st, _ = net.step(), rec.step()
            net.message_latency()
            net.peer_latency()
            if st.new_deliveries and st.round >= 2:  # the receipts stay counted, their relays go
                for n in (net, rec):
                    d = n.deliveries()
                    n.drop_relays(d.peer, d.msg)
            if not st.active:
                break
        hop, _ = rec.hop_parent()
        assert (hop.max(axis=0) <= 2).all()
        assert_latency(net, hop, np.zeros(100, dtype=np.int64))


def test_refusals():
    from p2pnetwork.gpu import GraphNetwork, PeerGraph, make_sources
    g = PeerGraph.random_regular(200, 4, seed=3)
    src = make_sources(g.V, 10, seed=1)
    L = _lib.lib()
    STATE, ARG = -2, -1
    with pytest.raises(P2PGError, match="partitioned"):
        GraphNetwork(g, latency=True, local_graph=True)
    with pytest.raises(ValueError):
        GraphNetwork(g, latency=True, latency_bins=1)
    buf = np.zeros(10 * 64, dtype=np.uint64)
    with GraphNetwork(g, latency=True) as net:
        for call in (net.message_latency, net.peer_latency, lambda: net.set_latency_bins(8)):
            with pytest.raises(P2PGError, match="no sources"):
                call()
        assert L.p2pg_set_latency_bins(net._h, 8) == STATE
        with pytest.raises(P2PGError, match="partitioned"):
            net.set_global_ids(np.arange(g.V, dtype=np.int32))
        assert L.p2pg_set_global_ids(net._h, _lib.ptr(np.arange(g.V, dtype=np.int32))) == STATE
        net.broadcast(src)
        for bad in (1, 0, -3, 1025):
            with pytest.raises(P2PGError, match="bins must lie"):
                net.set_latency_bins(bad)
            assert L.p2pg_set_latency_bins(net._h, bad) == ARG
        assert net.message_latency().shape == (10, 64)  # a rejected call changes nothing
        assert L.p2pg_message_latency(net._h, 32, _lib.ptr(buf)) == ARG
        assert L.p2pg_message_latency(net._h, 64, None) == ARG
        assert L.p2pg_peer_latency(net._h, None, None, None) == 0
        net.set_latency_bins(2)
        net.set_latency_bins(1024)
        assert net.message_latency().shape == (10, 1024)
        net.set_latency_bins(64)
        net.step()
        with pytest.raises(P2PGError, match="a round has run"):
            net.set_latency_bins(8)
        assert L.p2pg_set_latency_bins(net._h, 8) == STATE
        assert net.latency_bins == 64 and net.message_latency().shape == (10, 64)
        with pytest.raises(P2PGError, match="P2PG_FLAG_LATENCY"):
            net.snapshot()
        with pytest.raises(P2PGError, match="P2PG_FLAG_LATENCY"):
            net.restore(np.zeros(4096, dtype=np.uint8))
        with pytest.raises(P2PGError, match="P2PG_FLAG_TALLY"):  # the other flags' reads stay their own
            net.peer_counters()
        with pytest.raises(P2PGError, match="P2PG_FLAG_MSG_COST"):
            net.message_cost()
        net.step_begin()
        for call in (net.message_latency, net.peer_latency):
            with pytest.raises(P2PGError, match="begun"):  # half a round
                call()
        assert L.p2pg_message_latency(net._h, 64, _lib.ptr(buf)) == STATE
        st = net.step_end()
        assert st.round == 1
        h = net.message_latency()
        assert (h[:, 0] == 1).all() and (h[:, 1] == 4).all() and not h[:, 2:].any()
        net.reset()
        net.set_latency_bins(8)  # allowed again after a reset
        net.run()
        assert net.message_latency().shape == (10, 8)
        assert (net.message_latency().sum(axis=1) == g.V).all()
    for kw in ({}, {"tally": True, "cost": True}):
        with GraphNetwork(g, **kw) as net:
            net.broadcast(src)
            net.run()
            for call in (net.message_latency, net.peer_latency, net.coverage_curve,
                         lambda: net.latency_percentile(0.5), lambda: net.set_latency_bins(8)):
                with pytest.raises(P2PGError, match="P2PG_FLAG_LATENCY"):
                    call()
            assert L.p2pg_peer_latency(net._h, None, None, None) == STATE
