"""GPU: run tallies computed on the device -- per-broadcast reach / hop sum / last hop
(p2pg_message_reach, p2pg_message_tally) and per-peer Node.message_count_send /
message_count_recv (p2pg_peer_counters) -- against the reference-harness fixtures, the host
reference tests/tally_ref.py (pinned by tests/test_tally.py), the C oracle and the engine's own
pinned streams (seen plane, hop plane of a record engine, p2pg_get_sends)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import tally_ref
from conftest import REPO, golden_cases, load_golden, updates_of
from p2pnetwork.gpu._lib import P2PGError

pytestmark = pytest.mark.gpu

# every RoundStats field but the ones that describe the kernel form a round took
RESULT_FIELDS = ("round", "active", "new_deliveries", "relays", "active_vertices", "active_words", "wedges",
                 "deg_active", "scatter_words", "received", "received_exact")
PEER_FIXTURES = ("c2_rrg1000_flood", "ws1000_flood_churn05", "ba1000_gossip_k3", "ba500_gossip_k2_churn10")


def net_of(z, graph=None, **kw):
    from p2pnetwork.gpu import GraphNetwork, PeerGraph
    g = graph if graph is not None else PeerGraph(z["rowptr"], z["colidx"])
    return GraphNetwork(g, mode=str(z["mode"]), fanout=int(z["fanout"]), gossip_seed=int(z["gossip_seed"]),
                        churn_threshold_value=int(z["churn_threshold"]), churn_seed=int(z["churn_seed"]), **kw)


def column_counts(seen, M):
    """numpy column popcounts of a seen plane [V][W] for messages 0..M-1."""
    V = seen.shape[0]
    out = np.zeros(M, dtype=np.uint64)
    for w in range(seen.shape[1]):  # (word by word: no [V][M] byte plane at M = 4096)
        bits = np.unpackbits(np.ascontiguousarray(seen[:, w]).view(np.uint8).reshape(V, 8), axis=1,
                             bitorder="little")
        n = min(64, M - 64 * w)
        out[64 * w:64 * w + n] = bits[:, :n].sum(0, dtype=np.uint64)
    return out


def results(rounds):
    return [tuple(getattr(r, f) for f in RESULT_FIELDS) for r in rounds]


def assert_tally(t, hop):
    reach, hop_sum, last_hop = tally_ref.message_tally(hop)
    np.testing.assert_array_equal(t.reach, reach)
    np.testing.assert_array_equal(t.hop_sum, hop_sum)
    np.testing.assert_array_equal(t.last_hop, last_hop)


def run_steps(net):
    out = []
    while True:
        out.append(net.step())
        if not out[-1].active:
            return out


# 1 -- reach needs no flag and no frontier rows: p2pg_run's skipped / partial / batched rounds
@pytest.mark.parametrize("name", golden_cases())
def test_message_reach_without_the_flag(name):
    z = load_golden(name)
    with net_of(z) as net:
        net.broadcast(z["src"])
        net.run()
        reach = net.message_reach()
    assert reach.dtype == np.uint64
    np.testing.assert_array_equal(reach, (z["hop"] >= 0).sum(0).astype(np.uint64))


# 2 -- message tallies with the flag, and the flag changes no result of the run
@pytest.mark.parametrize("how", ["run", "step"])
@pytest.mark.parametrize("name", golden_cases())
def test_message_tally_matches_reference(name, how):
    z = load_golden(name)
    with net_of(z) as plain:
        plain.broadcast(z["src"])
        want_rounds = results(plain.run())
        want_seen = plain.seen_plane()
    with net_of(z, tally=True) as net:
        net.broadcast(z["src"])
        rounds = net.run() if how == "run" else run_steps(net)
        t = net.message_tally()
        assert_tally(t, z["hop"])
        np.testing.assert_array_equal(t.reach, net.message_reach())
        assert results(rounds) == want_rounds
        np.testing.assert_array_equal(net.seen_plane(), want_seen)


# 3 -- row widths: 64 / W rows per load, a tail word, whole slices, a second (partial) slice;
# V = 3001 is no multiple of the 32-peer task
@pytest.fixture(scope="module")
def ba3001():
    from p2pnetwork.gpu import PeerGraph
    return PeerGraph.barabasi_albert(3001, 4, seed=9)


@pytest.mark.parametrize("M,mode", [(1, "gossip"), (63, "gossip"), (64, "gossip"), (65, "gossip"),
                                    (512, "gossip"), (1000, "gossip"), (2048, "gossip"), (4096, "gossip"),
                                    (4100, "flood")])
def test_row_widths(ba3001, M, mode):
    from p2pnetwork.gpu import GraphNetwork, make_sources
    g = ba3001
    src = make_sources(g.V, M, seed=3)
    with GraphNetwork(g, mode=mode, fanout=3, gossip_seed=11, tally=True) as net:
        net.broadcast(src)
        net.run()
        seen = net.seen_plane()
        t = net.message_tally()
        reach = net.message_reach()
    with GraphNetwork(g, mode=mode, fanout=3, gossip_seed=11, record=True) as rec:
        rec.broadcast(src)
        rec.run()
        hop, _ = rec.hop_parent()
        np.testing.assert_array_equal(rec.seen_plane(), seen)
        np.testing.assert_array_equal(rec.message_reach(), reach)
    want = column_counts(seen, M)
    np.testing.assert_array_equal(reach, want)
    np.testing.assert_array_equal(t.reach, want)
    assert_tally(t, hop)


# 4 -- the fused dense rounds of the flagship shape keep their frontier rows with the flag on
def test_dense_fused_rounds_with_tally():
    from oracle import coracle
    from p2pnetwork.gpu import GraphNetwork, PeerGraph, make_sources
    g = PeerGraph.barabasi_albert(20000, 4, seed=1)
    src = make_sources(g.V, 4096, seed=1)
    with GraphNetwork(g, mode="gossip", fanout=3, gossip_seed=0x5EED) as plain:
        plain.broadcast(src)
        plain.run()
        want = column_counts(plain.seen_plane(), 4096)
    with GraphNetwork(g, mode="gossip", fanout=3, gossip_seed=0x5EED, tally=True) as net:
        net.broadcast(src)
        rounds = net.run()
        t = net.message_tally()
        reach = net.message_reach()
    assert 3 in {r.push_form for r in rounds}, "no fused dense round ran"
    np.testing.assert_array_equal(t.reach, want)
    np.testing.assert_array_equal(reach, want)
    assert int(t.hop_sum.sum()) == sum(r.round * r.new_deliveries for r in rounds)
    for w in (0, 63):
        ora = coracle.run(g.rowptr, g.colidx, src[64 * w:64 * (w + 1)], "gossip", 3, 0x5EED,
                          msg_id_base=64 * w, record=True)
        _, hop_sum, last_hop = tally_ref.message_tally(ora.hop)
        np.testing.assert_array_equal(t.hop_sum[64 * w:64 * (w + 1)], hop_sum)
        np.testing.assert_array_equal(t.last_hop[64 * w:64 * (w + 1)], last_hop)


# 5 -- the vertical counters' flush period.  P2PG_GRID_MAX is read once per process, so a child:
# one block = 4 waves; W = 64, so a wave load is one row and a wave task 256 rows (whole plane) or
# the active rows of 32 peers (frontier).  The bit-sliced counters hold 2^6 - 1 = 63 rows and are
# flushed every 60 (rows are absorbed 4 at a time).  V = 2048: 8 whole-plane tasks, 2 per wave =
# 512 rows >= 8 periods; in the flood's middle rounds nearly every peer has first receipts, so a
# wave's 16 frontier tasks hold up to 512 rows as well.
CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np
from p2pnetwork.gpu import GraphNetwork, PeerGraph, make_sources
g = PeerGraph.random_regular(2048, 4, seed=5)
src = make_sources(g.V, 4096, seed=2)
with GraphNetwork(g, mode="flood", tally=True) as net:
    net.broadcast(src)
    rounds = net.run()
    t = net.message_tally()
    reach = net.message_reach()
assert max(r.active_vertices for r in rounds) > 4 * 2 * 63, "no round filled two periods per wave"
assert reach.shape == (4096,) and (reach == g.V).all(), reach
assert (t.reach == g.V).all(), t.reach
assert int(t.hop_sum.sum()) == sum(r.round * r.new_deliveries for r in rounds)
print("ok")
"""


def test_counter_period_single_block():
    env = dict(os.environ, P2PG_GRID_MAX="1")
    code = CHILD % (REPO, os.path.join(REPO, "python-p2p-network_amd"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.strip().endswith("ok")


# 6 -- peer counters
@pytest.mark.parametrize("name", PEER_FIXTURES)
def test_peer_counters_match_reference(name):
    z = load_golden(name)
    with net_of(z, tally=True) as net:
        net.broadcast(z["src"])
        net.run()
        c = net.peer_counters()
    sent, received = tally_ref.of_fixture(z)
    np.testing.assert_array_equal(c.sent, sent)
    np.testing.assert_array_equal(c.received, received)


@pytest.mark.parametrize("name", golden_cases())
def test_peer_counter_sums_match_reference_totals(name):
    z = load_golden(name)
    with net_of(z, tally=True) as net:
        net.broadcast(z["src"])
        rounds = net.run()
        c = net.peer_counters()
    assert int(c.sent.sum()) == sum(r.relays for r in rounds) == int(z["round_relays"].sum())
    assert int(c.received.sum()) == int(z["total_recv"])


def twin_counters(g, src, mode, k, gseed, thr=0, cseed=0):
    """peer counters of a tally engine and tally_ref's from a record twin's hop / parent."""
    from p2pnetwork.gpu import GraphNetwork
    kw = dict(mode=mode, fanout=k, gossip_seed=gseed, churn_threshold_value=thr, churn_seed=cseed)
    with GraphNetwork(g, tally=True, **kw) as net:
        net.broadcast(src)
        rounds = net.run()
        c = net.peer_counters()
    with GraphNetwork(g, record=True, **kw) as rec:
        rec.broadcast(src)
        rec.run()
        hop, parent = rec.hop_parent()
    sent, received = tally_ref.peer_counters(hop, parent, g.rowptr, g.colidx, mode, k, gseed, thr, cseed)
    np.testing.assert_array_equal(c.sent, sent)
    np.testing.assert_array_equal(c.received, received)
    return rounds


def test_peer_counters_dense_rounds_w64():
    from p2pnetwork.gpu import PeerGraph, make_sources
    g = PeerGraph.barabasi_albert(600, 4, seed=2)
    rounds = twin_counters(g, make_sources(g.V, 4096, seed=4), "gossip", 3, 0x5EED)
    assert {r.push_form for r in rounds} & {2, 3, 4}, "no dense round ran"


@pytest.mark.parametrize("mode,thr", [("flood", 0), ("gossip", 0), ("gossip", 1 << 29)])
def test_peer_counters_hub_above_512(mode, thr):
    from p2pnetwork.gpu import PeerGraph, make_sources
    # a 700-leaf star (hub 0) joined to a 99-peer ring at peer 701: the hub's row is wider than
    # the per-wave connection table
    ring = list(range(701, 800))
    edges = [(0, i) for i in range(1, 702)] + list(zip(ring, ring[1:] + ring[:1]))
    g = PeerGraph.from_edges(800, np.array(edges, dtype=np.int32))
    assert int(g.degree().max()) == 701
    src = make_sources(g.V, 70, seed=6)
    src[:3] = (0, 5, 750)  # the hub, a leaf and a ring peer originate too
    twin_counters(g, src, mode, 3, 77, thr, 5)


# 7 -- drops and topology changes: the engine's own pinned send stream is the reference
def test_peer_counters_after_drop_relays():
    from p2pnetwork.gpu import GraphNetwork, PeerGraph, make_sources
    g = PeerGraph.random_regular(300, 6, seed=8)
    src = make_sources(g.V, 100, seed=9)
    sent = np.zeros(g.V, dtype=np.uint64)
    received = np.zeros(g.V, dtype=np.uint64)
    hop = np.full((g.V, 100), -1, dtype=np.int32)
    with GraphNetwork(g, mode="flood", tally=True) as net:
        net.broadcast(src)
        while True:
            st = net.step()
            if st.new_deliveries:
                d = net.deliveries()
                hop[d.peer, d.msg] = st.round
                if st.round >= 2:  # TTL 2: later first receipts are not relayed
                    net.drop_relays(d.peer, d.msg)
            s = net.sends()
            sent += np.bincount(s.sender, minlength=g.V).astype(np.uint64)
            received += np.bincount(s.receiver[~s.lost], minlength=g.V).astype(np.uint64)
            if not st.active:
                break
        c = net.peer_counters()
        t = net.message_tally()
        np.testing.assert_array_equal(t.reach, net.message_reach())
    assert hop.max() == 2 and sent.sum() > 0
    np.testing.assert_array_equal(c.sent, sent)
    np.testing.assert_array_equal(c.received, received)
    assert_tally(t, hop)  # the receipts happened; only their relays were withdrawn


@pytest.mark.parametrize("name", golden_cases(dynamic=True))
def test_peer_counters_with_topology_updates(name):
    z = load_golden(name)
    upd = updates_of(z)
    V = len(z["rowptr"]) - 1
    sent = np.zeros(V, dtype=np.uint64)
    received = np.zeros(V, dtype=np.uint64)
    with net_of(z, tally=True) as net:
        net.broadcast(z["src"])
        while True:
            st = net.step()
            s = net.sends()
            lost = s.lost.copy()
            if st.round in upd:
                add, rem = upd[st.round]
                rem = np.asarray(rem, dtype=np.int64).reshape(-1, 2)
                gone = set(map(tuple, rem.tolist())) | set(map(tuple, rem[:, ::-1].tolist()))
                lost |= np.array([(a, b) in gone for a, b in zip(s.sender.tolist(), s.receiver.tolist())],
                                 dtype=bool).reshape(len(lost))
                net.update_edges(add, rem)
            sent += np.bincount(s.sender, minlength=V).astype(np.uint64)
            received += np.bincount(s.receiver[~lost], minlength=V).astype(np.uint64)
            if not st.active:
                break
        c = net.peer_counters()
        t = net.message_tally()
    np.testing.assert_array_equal(c.sent, sent)
    np.testing.assert_array_equal(c.received, received)
    assert int(c.received.sum()) == int(z["total_recv"])
    assert int(c.sent.sum()) == int(z["round_relays"].sum())
    assert_tally(t, z["hop"])


# 8 -- lifecycle and refusals
def test_reset_and_new_sources_zero_the_tallies():
    z = load_golden("ba1000_gossip_k3")
    with net_of(z, tally=True) as net:
        net.broadcast(z["src"])
        net.run()
        t1, c1 = net.message_tally(), net.peer_counters()
        net.reset()
        net.run()
        t2, c2 = net.message_tally(), net.peer_counters()
        for a, b in zip(t1 + c1, t2 + c2):
            np.testing.assert_array_equal(a, b)
        assert int(c1.sent.sum()) == int(z["round_relays"].sum())
        net.broadcast(z["src"][::-1].copy())
        t0, c0 = net.message_tally(), net.peer_counters()
        assert not t0.reach.any() and not t0.hop_sum.any() and (t0.last_hop == -1).all()
        assert not c0.sent.any() and not c0.received.any()
        assert not net.message_reach().any()
        net.step()
        assert (net.message_tally().reach == 1).all() and (net.message_tally().last_hop == 0).all()


def test_refusals():
    from p2pnetwork.gpu import GraphNetwork, PeerGraph, make_sources
    g = PeerGraph.random_regular(200, 4, seed=3)
    src = make_sources(g.V, 10, seed=1)
    with pytest.raises(P2PGError, match="partitioned"):
        GraphNetwork(g, tally=True, local_graph=True)
    with GraphNetwork(g, tally=True) as net:
        for read in (net.message_reach, net.message_tally, net.peer_counters):
            with pytest.raises(P2PGError, match="no sources"):  # before the sources are set
                read()
        with pytest.raises(P2PGError, match="partitioned"):
            net.set_global_ids(np.arange(g.V, dtype=np.int32))
        net.broadcast(src)
        net.step()
        with pytest.raises(P2PGError, match="tallies"):
            net.snapshot()
        with pytest.raises(P2PGError, match="tallies"):
            net.restore(np.zeros(4096, dtype=np.uint8))
        net.step_begin()
        for read in (net.message_reach, net.message_tally, net.peer_counters):
            with pytest.raises(P2PGError, match="begun"):  # half a round
                read()
        st = net.step_end()
        # the counters of a boundary are read after its changes
        d = net.deliveries()
        net.peer_counters()
        with pytest.raises(P2PGError, match="read the counters after"):
            net.drop_relays(d.peer[:1], d.msg[:1])
        with pytest.raises(P2PGError, match="read the counters after"):
            net.update_edges(remove=[(0, int(g.neighbours(0)[0]))])
        assert st.round == 1
        net.step()  # the next boundary is open again
        d = net.deliveries()
        net.drop_relays(d.peer[:1], d.msg[:1])
        net.peer_counters()
    with GraphNetwork(g) as net:
        net.broadcast(src)
        net.run()
        for read in (net.message_tally, net.peer_counters):
            with pytest.raises(P2PGError, match="P2PG_FLAG_TALLY"):
                read()
        assert (net.message_reach() == g.V).all()
    with GraphNetwork(g, local_graph=True) as net:
        net.broadcast(src)
        with pytest.raises(P2PGError, match="partitioned"):
            net.message_reach()
