"""The fused gossip round's trimmed scalar state against the oracle, bit for bit.

One small graph packs in the places where a peer / task / slot scalar, a kernel argument held in
a register or a lane mask that is no longer tested can go wrong (DESIGN.md 4a,
profiles/fused_scalars):

* V = 32 * 40 + 1 peers: the last task is ragged (one peer, V - 1);
* task 1 (peers 32..63) is a tight cluster hanging off the origin, peer 0 (deg 3): a cycle with
  its 16 diameters, so every degree in it is <= 3 = the fanout and its pushes go to every
  connection.  All M broadcasts cross it in 9 rounds and it is saturated rounds before the rest,
  so later rounds meet a task with nothing to do and one that finishes in mid-run.  (A clique of
  wider peers never saturates: a push reaches 3 of 31 connections, and some of 4096 broadcasts
  miss some peer.)
* task 20 (peers 640..671) is a chain spliced into the ring: every peer of it has degree <= 3
  (the push that copies the row instead of drawing picks);
* peer MED has 16 < deg <= 64 and peer WIDE 64 < deg <= 512 connections, WIDE's spread over the
  whole ring (which also keeps the run short);
* the rest is the ring of tests/test_gpu_pick_path.py (steps 1 and 7), all M broadcasts from peer 0.

Each case runs under the forced store form (one unfused round, then fused rounds) and under the
automatic form with the update+push pass; seen / hop / parent planes and every per-round counter
equal the oracle's.  From the oracle's hop plane each run asserts that the rounds of the form
under test hold a task whose peers are all saturated while others are not, a visit of the last
peer, and a visit of WIDE with more than 64 active slots -- a missing shape fails the test.
"""
import functools

import numpy as np
import pytest

from test_gpu_parity import assert_rounds_equal, gpu_net, oracle_for

pytestmark = pytest.mark.gpu

V = 32 * 40 + 1
CLUSTER = range(32, 64)
CHAIN = range(640, 672)
WIDE, WIDE_EXTRA = 300, 100
MED, MED_EXTRA = 900, 30
FANOUT = 3


@functools.lru_cache(maxsize=None)
def scalar_graph():
    from p2pnetwork.gpu import PeerGraph
    off_ring = {0} | set(CLUSTER) | set(CHAIN)
    ring = np.array([v for v in range(V) if v not in off_ring], dtype=np.int64)
    n = len(ring)
    edges = [np.stack([ring, ring[(np.arange(n) + s) % n]], axis=1) for s in (1, 7)]
    cl = np.array(CLUSTER, dtype=np.int64)
    edges.append(np.stack([cl, np.roll(cl, -1)], axis=1))  # the cycle ...
    edges.append(np.stack([cl[1:16], cl[17:]], axis=1))    # ... its diameters (but the entry's)
    edges.append(np.array([[0, CLUSTER[0]], [0, 1], [0, 2]], dtype=np.int64))  # the origin
    ch = np.array(CHAIN, dtype=np.int64)
    edges.append(np.stack([ch[:-1], ch[1:]], axis=1))
    edges.append(np.array([[CHAIN[0] - 1, CHAIN[0]], [CHAIN[-1], CHAIN[-1] + 1]], dtype=np.int64))

    def extra(hub, count, first, step):  # `count` ring peers from ring position `first` on
        pos = int(np.searchsorted(ring, hub))
        far = [(first + step * i) % n for i in range(count)]
        assert all((f - pos) % n not in (0, 1, 7, n - 1, n - 7) for f in far)  # new connections
        return np.stack([np.full(count, hub, dtype=np.int64), ring[far]], axis=1)

    edges.append(extra(WIDE, WIDE_EXTRA, 5, 12))
    edges.append(extra(MED, MED_EXTRA, 500, 2))
    g = PeerGraph.from_edges(V, np.concatenate(edges))
    deg = np.diff(g.rowptr)
    assert V % 32 == 1 and g.V == V
    assert deg[list(CHAIN)].max() <= FANOUT and deg[list(CHAIN)].min() >= 2
    assert 16 < deg[MED] <= 64 and 64 < deg[WIDE] <= 512
    assert deg[list(CLUSTER)].max() <= FANOUT and deg[0] == 3 and deg[V - 1] == 4
    return g


# (M, gossip seed, churn threshold, msg_id_base): the full width; W = 63 with a ragged last word;
# W = 33, the narrowest row of the one-slot-per-load instances; churn; global message ids
CASES = [(4096, 1234, 0, 0), (4000, 77, 0, 0), (2112, 5, 0, 0), (4096, 1234, 300_000_000, 0),
         (4096, 99, 0, 8192)]


@functools.lru_cache(maxsize=1)  # the forms of one case run back to back
def reference(M, gseed, thr, base):
    g = scalar_graph()
    src = np.zeros(M, dtype=np.int32)
    if base:
        from oracle import relay_oracle
        ora = relay_oracle.gossip(g.rowptr, g.colidx, src, FANOUT, gseed, base, thr, 5 + M)
    else:
        ora = oracle_for(g.rowptr, g.colidx, src, "gossip", FANOUT, gseed, thr, 5 + M)
    for a in (ora.hop, ora.parent):
        a.setflags(write=False)
    return src, ora


def visit_shapes(g, hop, rounds_under_test):
    """The shapes among the peer visits of the given rounds (hop: [peer][message]; a peer is
    visited in round r while it still misses a message, and a connection slot is active in round r
    when its neighbour had a first receipt in round r - 1)."""
    got = set()
    done = np.where((hop >= 0).all(axis=1), hop.max(axis=1), np.iinfo(np.int32).max)  # saturated after
    pad = np.full(41 * 32, -1, dtype=np.int64)  # (the ragged task's missing peers: saturated)
    pad[:V] = done
    task_done = pad.reshape(41, 32).max(axis=1)
    wide_nbrs = g.colidx[g.rowptr[WIDE]:g.rowptr[WIDE + 1]]
    for r in rounds_under_test:
        if (task_done < r).any() and (task_done >= r).any():
            got.add("saturated task")
        if (hop[V - 1] == r).any():
            got.add("last peer")
        if done[WIDE] >= r and (hop[wide_nbrs] == r - 1).any(axis=1).sum() > 64:
            got.add("wide > 64 active")
    return got


SHAPES = {"saturated task", "last peer", "wide > 64 active"}


@pytest.mark.parametrize("form", ["store", "auto_update"])  # (varies fastest)
@pytest.mark.parametrize("M,gseed,thr,base", CASES)
def test_fused_scalars_match_oracle(M, gseed, thr, base, form, monkeypatch):
    monkeypatch.setenv("P2PG_GOSSIP_PUSH", form.split("_")[0])
    monkeypatch.setenv("P2PG_FUSED", "1")
    monkeypatch.setenv("P2PG_UPDATE_PUSH", "1" if form == "auto_update" else "0")
    if form == "auto_update":
        monkeypatch.setenv("P2PG_V_THRESH", "0")  # (no floor on a dense round's active peers)
    g = scalar_graph()
    src, ora = reference(M, gseed, thr, base)
    kw = {"msg_id_base": base} if base else {}
    with gpu_net(g, "gossip", FANOUT, gseed, thr, 5 + M, **kw) as net:
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
    # not vacuous: the pull of round r runs in the form of round r
    got = visit_shapes(g, ora.hop, [r for r, f in enumerate(forms) if r >= 1 and f in under_test])
    print(form, "visit shapes", sorted(got))
    assert got == SHAPES, (sorted(SHAPES - got), forms)
    np.testing.assert_array_equal(seen, ora.hop >= 0)
    np.testing.assert_array_equal(hop, ora.hop)
    np.testing.assert_array_equal(parent, ora.parent)
    assert_rounds_equal(rounds, ora.rounds)
