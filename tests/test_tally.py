"""CPU: the run-tally interface (include/p2pgpu.h P2PG_FLAG_TALLY, p2pg_message_reach /
p2pg_message_tally / p2pg_peer_counters) is declared, and the host reference the GPU tests compare
against (tests/tally_ref.py) agrees with references that do not depend on the engine: the
object-level relay's per-peer counters and the reference-made fixture totals."""
import os
import re

import numpy as np
import pytest

import tally_ref
from conftest import REPO, golden_cases, load_golden
from oracle.object_relay import ObjectRelay
from p2pnetwork.gpu import PeerGraph, _lib, make_sources
from p2pnetwork.gpu.network import churn_threshold


def test_header_declares_the_tally_interface():
    text = open(os.path.join(REPO, "include", "p2pgpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define\s+P2PG_FLAG_TALLY\s+32u", code)
    for fn in ("p2pg_message_reach", "p2pg_message_tally", "p2pg_peer_counters"):
        assert re.search(r"\bint\s+%s\s*\(" % fn, code), fn
        assert fn in _lib.SIGNATURES
    assert _lib.FLAG_TALLY == 32


SMALL = [
    ("flood", lambda: PeerGraph.random_regular(60, 4, seed=2), 10, 3, 0.0),
    ("flood", lambda: PeerGraph.watts_strogatz(80, 4, 0.2, seed=3), 12, 3, 0.1),
    ("gossip", lambda: PeerGraph.barabasi_albert(100, 3, seed=4), 16, 2, 0.1),
]


@pytest.mark.parametrize("mode,make,M,k,churn", SMALL, ids=["rrg60_flood", "ws80_flood_churn", "ba100_gossip_k2_churn"])
def test_reference_matches_object_relay_counters(mode, make, M, k, churn):
    g = make()
    src = make_sources(g.V, M, seed=7)
    thr, gseed, cseed = churn_threshold(churn), 0x5EED, 0xC0FFEE
    sim = ObjectRelay(g.rowptr, g.colidx, mode, k, gseed, thr, cseed)
    per_round = sim.run(src)
    hop, parent = sim.planes(g.V, M)
    sent, received = tally_ref.peer_counters(hop, parent, g.rowptr, g.colidx, mode, k, gseed, thr, cseed)
    want_s = np.zeros(g.V, dtype=np.uint64)
    want_r = np.zeros(g.V, dtype=np.uint64)
    for v, p in sim.peers.items():
        want_s[v], want_r[v] = p.count_send, p.count_recv
    np.testing.assert_array_equal(sent, want_s)
    np.testing.assert_array_equal(received, want_r)
    assert int(sent.sum()) == sum(per_round) and (churn == 0.0 or int(received.sum()) < int(sent.sum()))
    reach, hop_sum, last_hop = tally_ref.message_tally(hop)
    for m in range(M):
        hops = [r for p in sim.peers.values() for mm, (r, _) in p.seen.items() if mm == m]
        assert (int(reach[m]), int(hop_sum[m]), int(last_hop[m])) == (len(hops), sum(hops), max(hops))


@pytest.mark.parametrize("name", golden_cases())
def test_reference_sums_match_reference_made_totals(name):
    z = load_golden(name)
    sent, received = tally_ref.of_fixture(z)
    assert int(sent.sum()) == int(z["round_relays"].sum())
    assert int(received.sum()) == int(z["total_recv"])


def test_partitioned_network_refuses_tallies():
    from p2pnetwork.gpu import PartitionedNetwork
    g = PeerGraph.random_regular(60, 4, seed=2)
    with pytest.raises(ValueError, match="tallies"):
        PartitionedNetwork(g, 2, 0, transport=None, tally=True)
