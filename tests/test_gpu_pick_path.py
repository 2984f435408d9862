"""The entry list and the pick batches of the fused gossip round against the oracle, bit for bit.

A small graph on which every shape of a peer's entry list occurs: 600 peers on a ring with steps
1 and 7 (deg >= 4), peer 1 with 36 extra leaves (peers 100..135: deg 40, a wide sender), and all
M broadcasts originating at peer 0 (deg 4).  So round 1 hands three quarters of all messages to
each of peer 0's four neighbours -- several list windows at a narrow peer and at peer 1 -- and the
later rounds thin out to lists of every length down to one entry.

Each case runs under the forced store form (one unfused round, then fused rounds) and under the
automatic form with the update+push pass (P2PG_V_THRESH = 0 there: the automatic form otherwise
keeps the rounds with few active peers sparse, round 1 with its long lists among them); seen / hop / parent planes and every per-round counter
equal the oracle's.  So that no list shape can go missing unnoticed, each run asserts from its
push forms and the oracle's hop plane that the rounds of the form under test hold peer visits
(first receipts of one peer in one round: the list that peer pushes from) with more than 1023
entries at a narrow peer and at peer 1, a multiple of 64, 64 k + 1, and fewer than 64.
"""
import functools

import numpy as np
import pytest

from test_gpu_parity import assert_rounds_equal, gpu_net, oracle_for

pytestmark = pytest.mark.gpu

V = 600
WIDE = 1
LEAVES = range(100, 136)
FANOUT = 3


@functools.lru_cache(maxsize=None)
def pick_graph():
    from p2pnetwork.gpu import PeerGraph
    ring = np.arange(V, dtype=np.int64)
    edges = [np.stack([ring, (ring + s) % V], axis=1) for s in (1, 7)]
    leaves = np.array(LEAVES, dtype=np.int64)
    edges.append(np.stack([np.full(len(leaves), WIDE, dtype=np.int64), leaves], axis=1))
    g = PeerGraph.from_edges(V, np.concatenate(edges))
    deg = np.diff(g.rowptr)
    assert deg[WIDE] == 40 and deg[0] == 4 and deg.min() >= 4
    assert deg[np.arange(V) != WIDE].max() <= 16  # every other peer is a narrow sender
    return g


# (M, gossip seed, churn threshold): W = 64; a ragged last word; churn (list_bits and pick_batch
# are shared with the churn instances)
CASES = [(4096, 1234, 0), (4000, 77, 0), (4096, 1234, 300_000_000)]


@functools.lru_cache(maxsize=1)  # the forms of one case run back to back
def reference(M, gseed, thr):
    g = pick_graph()
    src = np.zeros(M, dtype=np.int32)
    ora = oracle_for(g.rowptr, g.colidx, src, "gossip", FANOUT, gseed, thr, 5 + M)
    for a in (ora.hop, ora.parent):
        a.setflags(write=False)
    return src, ora


def visit_shapes(hop, rounds_under_test):
    """The list shapes among the peer visits of the given rounds (hop: [peer][message])."""
    got = set()
    for r in rounds_under_test:
        n = (hop == r).sum(axis=1)
        narrow = np.delete(n, WIDE)
        if (narrow > 1023).any():
            got.add("narrow > 1023")
        if n[WIDE] > 1023:
            got.add("wide > 1023")
        if ((n >= 64) & (n % 64 == 0)).any():
            got.add("64 k")
        if ((n > 64) & (n % 64 == 1)).any():
            got.add("64 k + 1")
        if ((n > 0) & (n < 64)).any():
            got.add("< 64")
    return got


SHAPES = {"narrow > 1023", "wide > 1023", "64 k", "64 k + 1", "< 64"}


@pytest.mark.parametrize("form", ["store", "auto_update"])  # (varies fastest)
@pytest.mark.parametrize("M,gseed,thr", CASES)
def test_pick_path_matches_oracle(M, gseed, thr, form, monkeypatch):
    monkeypatch.setenv("P2PG_GOSSIP_PUSH", form.split("_")[0])
    monkeypatch.setenv("P2PG_FUSED", "1")
    monkeypatch.setenv("P2PG_UPDATE_PUSH", "1" if form == "auto_update" else "0")
    if form == "auto_update":
        # no floor on the active peers of a dense round: round 1 -- four active peers, the long
        # lists -- then already runs in the dense forms (update+push, then fused)
        monkeypatch.setenv("P2PG_V_THRESH", "0")
    g = pick_graph()
    src, ora = reference(M, gseed, thr)
    with gpu_net(g, "gossip", FANOUT, gseed, thr, 5 + M) as net:
        net.broadcast(src)
        rounds = net.run()
        hop, parent = net.hop_parent()
        seen = net.delivered()
    forms = [r.push_form for r in rounds]
    print(form, "push forms", forms)
    delivering = [f for f, r in zip(forms, rounds) if r.new_deliveries]
    if form == "store":
        assert delivering[0] == 2 and delivering[1:] and all(f == 3 for f in delivering[1:]), forms
        under_test = {3}
    else:
        assert 4 in delivering, forms
        under_test = {3, 4}
    # not vacuous: a visit of round r is a push of round r, in that round's form
    got = visit_shapes(ora.hop, [r for r, f in enumerate(forms) if r >= 1 and f in under_test])
    print(form, "list shapes", sorted(got))
    assert got == SHAPES, (sorted(SHAPES - got), forms)
    np.testing.assert_array_equal(seen, ora.hop >= 0)
    np.testing.assert_array_equal(hop, ora.hop)
    np.testing.assert_array_equal(parent, ora.parent)
    assert_rounds_equal(rounds, ora.rounds)
