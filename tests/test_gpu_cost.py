"""GPU: the per-broadcast cost computed on the device (p2pg_message_cost: the send_to_node calls
that carried each message and those of them that arrived) against the host reference
tests/cost_ref.py (pinned by tests/test_cost.py), the down_ref / pull_ref send streams of the
feature fixtures, and the engine's own pinned send stream (p2pg_get_sends).  Every comparison of
sent and received is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cost_ref
from conftest import REPO, golden_cases, load_golden, updates_of
from p2pnetwork.gpu._lib import P2PGError
from test_cost import FEATURE_CASES, feature_ref, load_feature
from test_gpu_tally import net_of, results, run_steps

pytestmark = pytest.mark.gpu


def assert_cost(c, want):
    assert c.sent.dtype == c.received.dtype == np.uint64
    np.testing.assert_array_equal(c.sent, want[0])
    np.testing.assert_array_equal(c.received, want[1])


# 1 -- every static fixture, by run() and by step(); the flag changes no result of the run
@pytest.mark.parametrize("how", ["run", "step"])
@pytest.mark.parametrize("name", golden_cases())
def test_cost_matches_reference(name, how):
    z = load_golden(name)
    with net_of(z) as plain:
        plain.broadcast(z["src"])
        want_rounds = results(plain.run())
        want_seen = plain.seen_plane()
    with net_of(z, cost=True) as net:
        net.broadcast(z["src"])
        rounds = net.run() if how == "run" else run_steps(net)
        c = net.message_cost()
        assert_cost(c, cost_ref.of_fixture(z))
        assert int(c.sent.sum()) == sum(r.relays for r in rounds) == int(z["round_relays"].sum())
        assert int(c.received.sum()) == int(z["total_recv"])
        assert results(rounds) == want_rounds
        np.testing.assert_array_equal(net.seen_plane(), want_seen)


# 2 -- start rounds, hop limits, the relay policy, downtime, anti-entropy: the fixtures' streams
def feature_net(z, **kw):
    from p2pnetwork.gpu import GraphNetwork, PeerGraph
    net = GraphNetwork(PeerGraph(z["rowptr"], z["colidx"]), mode=str(z["mode"]), fanout=int(z["fanout"]),
                       gossip_seed=int(z["gossip_seed"]), churn_threshold_value=int(z["churn_threshold"]),
                       churn_seed=int(z["churn_seed"]), **kw)
    net.broadcast(z["src"], z["start"], ttl=z["ttl"] if "ttl" in z else None)
    if "thr" in z and z["thr"].any():
        net.set_relay_policy(thresholds=z["thr"], seed=int(z["policy_seed"]))
    if "down_from" in z:
        net.set_downtime(z["down_from"], z["down_until"])
    if "anti_entropy" in z:
        period, first, last = (int(x) for x in z["anti_entropy"])
        net.set_anti_entropy(period, first, last, seed=int(z["pull_seed"]))
    return net


COMPOSED = [c for c in FEATURE_CASES if c[0] == "pull" or c[1].endswith(("rrg200_flood", "ba300_gossip_k2_churn10"))]


@pytest.mark.parametrize("kind,name", COMPOSED)
def test_cost_composes_with_the_per_message_features(kind, name):
    z = load_feature(kind, name)
    ref = feature_ref(kind, name)
    M = len(z["src"])
    with feature_net(z, cost=True) as net:
        rounds = net.run()
        c = net.message_cost()
        assert_cost(c, cost_ref.message_cost(ref.sends, M))
        assert int(c.sent.sum()) == sum(r.relays for r in rounds) == int(z["round_relays"].sum())
        assert int(c.received.sum()) == int(z["total_recv"])
        np.testing.assert_array_equal(net.message_reach(), (z["hop"] >= 0).sum(axis=0))
        # the counters of a step-by-step replay read at every boundary: the stream's prefix sums
        net.reset()
        for r in range(len(ref.rounds)):
            net.step()
            if r in (1, 3, len(ref.rounds) - 1):
                assert_cost(net.message_cost(), cost_ref.message_cost(ref.sends[:r + 1], M))


# 3 -- row widths: lanes past the row, a tail word, whole slices, a second (one-word) slice;
# V = 3001 is no multiple of the 32-peer task
def twin_cost(g, src, mode, k, gseed, thr=0, cseed=0):
    """the cost of a cost engine against cost_ref's from a record twin's hop / parent."""
    from p2pnetwork.gpu import GraphNetwork
    kw = dict(mode=mode, fanout=k, gossip_seed=gseed, churn_threshold_value=thr, churn_seed=cseed)
    with GraphNetwork(g, cost=True, **kw) as net:
        net.broadcast(src)
        rounds = net.run()
        c = net.message_cost()
        reach = net.message_reach()
        red = net.message_redundancy()
    with GraphNetwork(g, record=True, **kw) as rec:
        rec.broadcast(src)
        assert results(rec.run()) == results(rounds)
        hop, parent = rec.hop_parent()
    assert_cost(c, cost_ref.plane_cost(hop, parent, g.rowptr, g.colidx, mode, k, gseed, thr, cseed))
    assert int(c.sent.sum()) == sum(r.relays for r in rounds)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = np.where(reach > 1, c.sent.astype(np.float64) / (reach.astype(np.float64) - 1.0) - 1.0, np.nan)
    np.testing.assert_array_equal(red, want)
    return rounds


@pytest.fixture(scope="module")
def ba3001():
    from p2pnetwork.gpu import PeerGraph
    return PeerGraph.barabasi_albert(3001, 4, seed=9)


@pytest.fixture(scope="module")
def ba600():
    from p2pnetwork.gpu import PeerGraph
    return PeerGraph.barabasi_albert(600, 4, seed=2)


@pytest.mark.parametrize("M", [1, 63, 64, 65, 1000])
def test_row_widths(ba3001, M):
    from p2pnetwork.gpu import make_sources
    twin_cost(ba3001, make_sources(ba3001.V, M, seed=3), "gossip", 3, 11)


def test_row_width_64_words_dense_rounds(ba600):
    from p2pnetwork.gpu import make_sources
    rounds = twin_cost(ba600, make_sources(ba600.V, 4096, seed=4), "gossip", 3, 0x5EED)
    assert {r.push_form for r in rounds} & {2, 3, 4}, "no dense round ran"


def test_row_width_second_slice(ba600):
    from p2pnetwork.gpu import make_sources
    twin_cost(ba600, make_sources(ba600.V, 4100, seed=4), "flood", 3, 0)


# 4 -- a hub wider than any per-wave table and than the vertical counters hold
@pytest.mark.parametrize("mode,thr", [("flood", 0), ("gossip", 0), ("gossip", 1 << 29)])
def test_hub_above_512(mode, thr):
    from p2pnetwork.gpu import PeerGraph, make_sources
    ring = list(range(701, 800))
    edges = [(0, i) for i in range(1, 702)] + list(zip(ring, ring[1:] + ring[:1]))
    g = PeerGraph.from_edges(800, np.array(edges, dtype=np.int32))
    assert int(g.degree().max()) == 701
    src = make_sources(g.V, 70, seed=6)
    src[:3] = (0, 5, 750)  # the hub, a leaf and a ring peer originate too
    twin_cost(g, src, mode, 3, 77, thr, 5)


# 5 -- counter capacity.  P2PG_GRID_MAX is read once per process, so a child: one block = 4 waves
# takes every peer of every round.  The vertical counters hold 255 per bit, a flood receipt on the
# 4-regular graph adds 4: a wave absorbs 63 peers per flush period, the block 252, and the middle
# rounds have nearly all 2048 peers active.  A flood on a connected graph sends every message over
# every connection in both directions, less once to each peer's sender: 2 E - (V - 1).
CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np
from p2pnetwork.gpu import GraphNetwork, PeerGraph, make_sources
g = PeerGraph.random_regular(2048, 4, seed=5)
src = make_sources(g.V, 4096, seed=2)
with GraphNetwork(g, mode="flood", cost=True) as net:
    net.broadcast(src)
    rounds = net.run()
    c = net.message_cost()
    reach = net.message_reach()
    red = net.message_redundancy()
assert (reach == g.V).all(), reach
assert max(r.active_vertices for r in rounds) > 4 * (255 // 4), "no round went past one flush period"
want = 2 * (len(g.colidx) // 2) - (g.V - 1)
assert want == 6145
assert c.sent.shape == (4096,) and (c.sent == want).all(), c.sent
assert (c.received == want).all(), c.received
assert (red == 6145 / 2047 - 1).all(), red
print("ok")
"""


# (P2PG_COST_DRAIN: the weight a wave adds before it takes the block's 32-bit LDS counts out to
# the shards, 2^29 by default -- lowered so that the run reaches that path at this size)
@pytest.mark.parametrize("drain", [None, "1000"])
def test_counter_capacity_single_block(drain):
    env = dict(os.environ, P2PG_GRID_MAX="1")
    if drain:
        env["P2PG_COST_DRAIN"] = drain
    code = CHILD % (REPO, os.path.join(REPO, "python-p2p-network_amd"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.strip().endswith("ok")


# An addend above 1/32 of that weight bypasses the LDS counts (one 64-bit atomic per set bit into the
# shards): by default a peer with more than 2^24 connections; with the weight lowered to 2048, the
# 701-connection hub of case 4, whose neighbours still go through the vertical counters.
HUB_CHILD = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import numpy as np
import cost_ref
from p2pnetwork.gpu import GraphNetwork, PeerGraph, make_sources
ring = list(range(701, 800))
edges = [(0, i) for i in range(1, 702)] + list(zip(ring, ring[1:] + ring[:1]))
g = PeerGraph.from_edges(800, np.array(edges, dtype=np.int32))
src = make_sources(g.V, 70, seed=6)
src[:3] = (0, 5, 750)
for thr in (0, 1 << 29):
    kw = dict(mode="flood", churn_threshold_value=thr, churn_seed=5)
    with GraphNetwork(g, cost=True, **kw) as net:
        net.broadcast(src)
        net.run()
        c = net.message_cost()
    with GraphNetwork(g, record=True, **kw) as rec:
        rec.broadcast(src)
        rec.run()
        hop, parent = rec.hop_parent()
    sent, received = cost_ref.plane_cost(hop, parent, g.rowptr, g.colidx, "flood", 3, 0, thr, 5)
    assert sent.max() > 701 and (c.sent == sent).all() and (c.received == received).all(), (c, sent, received)
print("ok")
"""


def test_hub_addends_straight_to_the_shards():
    env = dict(os.environ, P2PG_COST_DRAIN="2048")
    code = HUB_CHILD % (REPO, os.path.join(REPO, "python-p2p-network_amd"), os.path.join(REPO, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.strip().endswith("ok")


# 6 -- drops and topology changes: the engine's own pinned send stream is the reference
def test_cost_after_drop_relays():
    from p2pnetwork.gpu import GraphNetwork, PeerGraph, make_sources
    g = PeerGraph.random_regular(300, 6, seed=8)
    src = make_sources(g.V, 100, seed=9)
    stream = []
    with GraphNetwork(g, mode="flood", cost=True) as net:
        net.broadcast(src)
        while True:
            st = net.step()
            if st.new_deliveries and st.round >= 2:  # TTL 2: later first receipts are not relayed
                d = net.deliveries()
                net.drop_relays(d.peer, d.msg)
            stream.append(net.sends())
            if not st.active:
                break
        c = net.message_cost()
    want = cost_ref.message_cost(stream, 100)
    assert want[0].sum() > 0 and not len(stream[2].sender)
    assert_cost(c, want)


@pytest.mark.parametrize("name", golden_cases(dynamic=True))
def test_cost_with_topology_updates(name):
    z = load_golden(name)
    upd = updates_of(z)
    stream, removed = [], {}
    with net_of(z, cost=True) as net:
        net.broadcast(z["src"])
        while True:
            st = net.step()
            stream.append(net.sends())
            if st.round in upd:
                add, rem = upd[st.round]
                removed[st.round] = np.asarray(rem, dtype=np.int64).reshape(-1, 2)
                net.update_edges(add, rem)
            if not st.active:
                break
        c = net.message_cost()
    assert_cost(c, cost_ref.message_cost(stream, len(z["src"]), removed))
    assert int(c.sent.sum()) == int(z["round_relays"].sum())
    assert int(c.received.sum()) == int(z["total_recv"])


# 7 -- both flags: the per-peer and the per-message pass count the same sends
@pytest.mark.parametrize("name", golden_cases())
def test_both_flags_agree(name):
    z = load_golden(name)
    with net_of(z, tally=True) as one:
        one.broadcast(z["src"])
        one.run()
        want_t = one.message_tally()
    with net_of(z, tally=True, cost=True) as net:
        net.broadcast(z["src"])
        rounds = net.run()
        c, p, t = net.message_cost(), net.peer_counters(), net.message_tally()
    assert int(c.sent.sum()) == int(p.sent.sum()) == sum(r.relays for r in rounds)
    assert int(c.received.sum()) == int(p.received.sum()) == int(z["total_recv"])
    assert_cost(c, cost_ref.of_fixture(z))
    for a, b in zip(t, want_t):
        np.testing.assert_array_equal(a, b)


# 8 -- lifecycle
def test_reset_and_new_sources_zero_the_cost():
    z = load_golden("ba1000_gossip_k3")
    with net_of(z, cost=True) as net:
        net.broadcast(z["src"])
        net.run()
        c1 = net.message_cost()
        assert int(c1.sent.sum()) == int(z["round_relays"].sum())
        net.reset()
        c0 = net.message_cost()
        assert not c0.sent.any() and not c0.received.any()
        net.run()
        assert_cost(net.message_cost(), c1)
        net.broadcast(z["src"][::-1].copy())
        c0 = net.message_cost()
        assert not c0.sent.any() and not c0.received.any()
        assert np.isnan(net.message_redundancy()).all()
        net.step()
        deg = np.diff(z["rowptr"])[z["src"][::-1]]
        np.testing.assert_array_equal(net.message_cost().sent, np.minimum(deg, int(z["fanout"])))


# 9 -- refusals
def test_refusals():
    from p2pnetwork.gpu import GraphNetwork, PeerGraph, make_sources
    g = PeerGraph.random_regular(200, 4, seed=3)
    src = make_sources(g.V, 10, seed=1)
    with pytest.raises(P2PGError, match="partitioned"):
        GraphNetwork(g, cost=True, local_graph=True)
    with GraphNetwork(g, cost=True) as net:
        with pytest.raises(P2PGError, match="no sources"):
            net.message_cost()
        with pytest.raises(P2PGError, match="partitioned"):
            net.set_global_ids(np.arange(g.V, dtype=np.int32))
        net.broadcast(src)
        net.step()
        with pytest.raises(P2PGError, match="P2PG_FLAG_MSG_COST"):
            net.snapshot()
        with pytest.raises(P2PGError, match="P2PG_FLAG_MSG_COST"):
            net.restore(np.zeros(4096, dtype=np.uint8))
        with pytest.raises(P2PGError, match="P2PG_FLAG_TALLY"):  # the other flag's reads stay its own
            net.peer_counters()
        net.step_begin()
        with pytest.raises(P2PGError, match="begun"):  # half a round
            net.message_cost()
        st = net.step_end()
        # the counters of a boundary are read after its changes
        d = net.deliveries()
        net.message_cost()
        with pytest.raises(P2PGError, match="read the counters after"):
            net.drop_relays(d.peer[:1], d.msg[:1])
        with pytest.raises(P2PGError, match="read the counters after"):
            net.update_edges(remove=[(0, int(g.neighbours(0)[0]))])
        assert st.round == 1
        net.step()  # the next boundary is open again
        d = net.deliveries()
        net.drop_relays(d.peer[:1], d.msg[:1])
        net.message_cost()
    for kw in ({}, {"tally": True}):
        with GraphNetwork(g, **kw) as net:
            net.broadcast(src)
            net.run()
            with pytest.raises(P2PGError, match="P2PG_FLAG_MSG_COST"):
                net.message_cost()
            with pytest.raises(P2PGError, match="P2PG_FLAG_MSG_COST"):
                net.message_redundancy()
    with GraphNetwork(g, local_graph=True) as net:
        net.broadcast(src)
        with pytest.raises(P2PGError):
            net.message_cost()
