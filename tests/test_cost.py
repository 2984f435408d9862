"""CPU: the per-broadcast cost interface (include/p2pgpu.h P2PG_FLAG_MSG_COST, p2pg_message_cost)
is declared, and the host reference the GPU tests compare against (tests/cost_ref.py) agrees with
references that do not depend on the engine: the object-level relay's send_to_node / node_message
calls counted per payload id, and the reference-made totals of every fixture."""
import functools
import os
import re

import numpy as np
import pytest

import cost_ref
import down_ref
import policy_ref
import pull_ref
from conftest import GOLDEN, REPO, golden_cases, load_golden
from oracle import object_relay
from p2pnetwork.gpu import PeerGraph, _lib, make_sources
from p2pnetwork.gpu.network import churn_threshold
from test_tally import SMALL


def test_header_declares_the_cost_interface():
    text = open(os.path.join(REPO, "include", "p2pgpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define\s+P2PG_FLAG_MSG_COST\s+64u", code)
    assert re.search(r"\bint\s+p2pg_message_cost\s*\(", code)
    assert "p2pg_message_cost" in _lib.SIGNATURES
    assert _lib.FLAG_MSG_COST == 64


@pytest.mark.parametrize("mode,make,M,k,churn", SMALL, ids=["rrg60_flood", "ws80_flood_churn", "ba100_gossip_k2_churn"])
def test_reference_matches_object_relay_calls_per_payload(monkeypatch, mode, make, M, k, churn):
    g = make()
    src = make_sources(g.V, M, seed=7)
    thr, gseed, cseed = churn_threshold(churn), 0x5EED, 0xC0FFEE
    want_s = np.zeros(M, dtype=np.uint64)
    want_r = np.zeros(M, dtype=np.uint64)
    send_to_node, node_message = object_relay._Peer.send_to_node, object_relay._Peer.node_message

    def counting_send(self, conn, data):  # node.py:116, per payload id
        want_s[data["mid"]] += 1
        return send_to_node(self, conn, data)

    def counting_message(self, conn, data):  # nodeconnection.py:215 hands every packet over
        want_r[data["mid"]] += 1
        return node_message(self, conn, data)

    monkeypatch.setattr(object_relay._Peer, "send_to_node", counting_send)
    monkeypatch.setattr(object_relay._Peer, "node_message", counting_message)
    sim = object_relay.ObjectRelay(g.rowptr, g.colidx, mode, k, gseed, thr, cseed)
    per_round = sim.run(src)
    hop, parent = sim.planes(g.V, M)
    sent, received = cost_ref.plane_cost(hop, parent, g.rowptr, g.colidx, mode, k, gseed, thr, cseed)
    np.testing.assert_array_equal(sent, want_s)
    np.testing.assert_array_equal(received, want_r)
    assert int(sent.sum()) == sum(per_round) == sum(p.count_send for p in sim.peers.values())
    assert int(received.sum()) == sum(p.count_recv for p in sim.peers.values())
    assert churn == 0.0 or int(received.sum()) < int(sent.sum())


@pytest.mark.parametrize("name", golden_cases())
def test_reference_sums_match_reference_made_totals(name):
    z = load_golden(name)
    sent, received = cost_ref.of_fixture(z)
    assert sent.dtype == received.dtype == np.uint64 and sent.shape == received.shape == (len(z["src"]),)
    assert int(sent.sum()) == int(z["round_relays"].sum())
    assert int(received.sum()) == int(z["total_recv"])


# The feature fixtures (late / ttl / policy / down / pull): their runs through down_ref / pull_ref,
# computed once and shared with tests/test_gpu_cost.py.
FEATURE_CASES = [(kind, "%s_%s" % (kind, case)) for kind in ("late", "ttl", "policy", "down", "pull")
                 for case in ("ba300_gossip_k2", "ba300_gossip_k2_churn10", "rrg200_flood", "ws300_flood_churn10")]


def load_feature(kind, name):
    with np.load(os.path.join(GOLDEN, kind, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def cfg_of(z):
    return dict(mode=str(z["mode"]), fanout=int(z["fanout"]), gossip_seed=int(z["gossip_seed"]),
                churn_threshold=int(z["churn_threshold"]), churn_seed=int(z["churn_seed"]))


def rule_of(z):
    """The drop= rule the fixture generators use: the fixture's relay policy and hop limits (a
    fixture without either drops nothing)."""
    V, M = z["hop"].shape
    thr = z["thr"] if "thr" in z else np.zeros(V, dtype=np.uint32)
    ttl = z["ttl"] if "ttl" in z else np.full(M, -1, dtype=np.int32)
    return policy_ref.with_ttl(policy_ref.policy_rule(thr, int(z["policy_seed"]) if "policy_seed" in z else 0,
                                                      z["start"]), z["start"], ttl)


@functools.lru_cache(maxsize=None)
def feature_ref(kind, name):
    """The fixture's run through down_ref (pull/: pull_ref); shared, never written to."""
    z = load_feature(kind, name)
    f, u = (z["down_from"], z["down_until"]) if "down_from" in z else (None, None)
    if kind == "pull":
        return pull_ref.run(z["rowptr"], z["colidx"], z["src"], z["start"], f, u,
                            anti_entropy=tuple(int(x) for x in z["anti_entropy"]), pull_seed=int(z["pull_seed"]),
                            **cfg_of(z))
    return down_ref.run(z["rowptr"], z["colidx"], z["src"], z["start"], f, u, drop=rule_of(z), **cfg_of(z))


@pytest.mark.parametrize("kind,name", [c for c in FEATURE_CASES if c[0] != "late"])
def test_stream_cost_sums_match_reference_made_totals(kind, name):
    z = load_feature(kind, name)
    ref = feature_ref(kind, name)
    np.testing.assert_array_equal(ref.hop, z["hop"])
    sent, received = cost_ref.message_cost(ref.sends, len(z["src"]))
    assert int(sent.sum()) == int(z["round_relays"].sum())
    assert int(received.sum()) == int(z["total_recv"])
    assert (received <= sent).all()


def test_stream_and_plane_routes_agree_and_removed_pairs_are_lost():
    z = load_feature("late", "late_ws300_flood_churn10")
    z0 = dict(z, start=np.zeros_like(z["start"]))
    ref = down_ref.run(z0["rowptr"], z0["colidx"], z0["src"], z0["start"], **cfg_of(z0))
    a = cost_ref.message_cost(ref.sends, len(z0["src"]))
    c0 = cfg_of(z0)
    b = cost_ref.plane_cost(ref.hop, ref.parent, z0["rowptr"], z0["colidx"], c0["mode"], c0["fanout"],
                            c0["gossip_seed"], c0["churn_threshold"], c0["churn_seed"])
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    snd, rcv, msg, lost = ref.sends[1]
    i = int(np.nonzero(~lost)[0][0])
    c = cost_ref.message_cost(ref.sends, len(z0["src"]), removed={1: [(int(rcv[i]), int(snd[i]))]})
    hit = ~lost & (((snd == snd[i]) & (rcv == rcv[i])) | ((snd == rcv[i]) & (rcv == snd[i])))
    np.testing.assert_array_equal(c[0], a[0])
    np.testing.assert_array_equal(a[1] - c[1], np.bincount(msg[hit], minlength=len(z0["src"])).astype(np.uint64))


def test_partitioned_network_refuses_the_cost():
    from p2pnetwork.gpu import PartitionedNetwork
    g = PeerGraph.random_regular(60, 4, seed=2)
    with pytest.raises(ValueError, match="cost"):
        PartitionedNetwork(g, 2, 0, transport=None, cost=True)
