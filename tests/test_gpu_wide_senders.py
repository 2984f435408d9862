"""Wide senders of the fused gossip round (16 < deg <= 512) against the oracle, bit for bit.

One graph of 4,000 peers holds a centre of every degree at which the fused push changes its path:
16 (the last narrow sender), 17 / 32 / 33 / 48 / 64 (one connection group; 2 or 4 word passes
when every word is active), 65 / 128 / 129 / 300 / 512 (2..8 groups, ragged last group), and 513
(a hub: the hub kernels).  Each centre has its own leaves; the leaves and the other peers form a
ring with two chords per peer, so every peer has deg >= 4 and the graph is connected.

Each case runs under the store form (one unfused round, then fused rounds), the automatic form
with the update+push pass, and the unfused store form; seen / hop / parent planes and every
per-round counter equal the oracle's.  So that the wide path cannot be skipped unnoticed, each run
asserts from its push forms and the oracle's hop plane that every centre of degree 17..512 made
first receipts -- and therefore pushed -- in a round of the form under test.
"""
import functools

import numpy as np
import pytest

from test_gpu_parity import assert_rounds_equal, gpu_net, oracle_for

pytestmark = pytest.mark.gpu

V = 4000
CENTRES = (16, 17, 32, 33, 48, 64, 65, 128, 129, 300, 512, 513)
CHORDS = (61, 617)


def wide_edges():
    """Centres 0..11; ring peers 12..V-1 (ring + chords); centre c's leaves are a slice of a
    seeded permutation of the ring peers."""
    n0 = len(CENTRES)
    ring = np.arange(n0, V, dtype=np.int64)
    n = len(ring)
    edges = [np.stack([ring, ring[(np.arange(n) + s) % n]], axis=1) for s in (1,) + CHORDS]
    perm = np.random.default_rng(20).permutation(ring)
    at = 0
    for c, d in enumerate(CENTRES):
        edges.append(np.stack([np.full(d, c, dtype=np.int64), perm[at:at + d]], axis=1))
        at += d
    return np.concatenate(edges)


@functools.lru_cache(maxsize=None)
def wide_graph():
    from p2pnetwork.gpu import PeerGraph
    g = PeerGraph.from_edges(V, wide_edges())
    deg = np.diff(g.rowptr)
    assert tuple(deg[:len(CENTRES)]) == CENTRES and deg.min() >= 4
    return g


# (M, fanout, churn threshold): W = 64; 47 with a ragged last word; 33; 32 (the HALF instance);
# 18; generic fanout (chunked pushes); churn (chunked pushes)
CASES = [(4096, 3, 0), (3000, 3, 0), (2100, 3, 0), (2048, 3, 0), (1100, 3, 0), (4096, 5, 0),
         (3000, 3, 300_000_000)]


@functools.lru_cache(maxsize=1)  # the forms of one case run back to back
def reference(M, fanout, thr):
    from p2pnetwork.gpu import make_sources
    g = wide_graph()
    src = make_sources(g.V, M, seed=7 + M)
    ora = oracle_for(g.rowptr, g.colidx, src, "gossip", fanout, 99 + M, thr, 5 + M)
    for a in (ora.hop, ora.parent):
        a.setflags(write=False)
    return src, ora


def centre_receipt_rounds(hop):
    """Per centre of degree 17..512: the rounds >= 1 in which it made first receipts."""
    return {d: set(np.unique(hop[c][hop[c] >= 1]).tolist())
            for c, d in enumerate(CENTRES) if 16 < d <= 512}


@pytest.mark.parametrize("form", ["store", "auto_update", "store_unfused"])  # (varies fastest)
@pytest.mark.parametrize("M,fanout,thr", CASES)
def test_wide_senders_match_oracle(M, fanout, thr, form, monkeypatch):
    monkeypatch.setenv("P2PG_GOSSIP_PUSH", form.split("_")[0])
    monkeypatch.setenv("P2PG_FUSED", "0" if form == "store_unfused" else "1")
    monkeypatch.setenv("P2PG_UPDATE_PUSH", "1" if form == "auto_update" else "0")
    g = wide_graph()
    src, ora = reference(M, fanout, thr)
    with gpu_net(g, "gossip", fanout, 99 + M, thr, 5 + M) as net:
        net.broadcast(src)
        rounds = net.run()
        hop, parent = net.hop_parent()
        seen = net.delivered()
    forms = [r.push_form for r in rounds]
    print(form, "push forms", forms)
    # not vacuous: rounds of the form under test delivered, and every wide centre pushed in one
    delivering = [f for f, r in zip(forms, rounds) if r.new_deliveries]
    if form == "store":
        assert delivering[0] == 2 and delivering[1:] and all(f == 3 for f in delivering[1:]), forms
        under_test = {3}
    elif form == "auto_update":
        assert 4 in delivering, forms
        under_test = {3, 4}
    else:
        assert all(f == 2 for f in delivering), forms
        under_test = {2}
    for d, rs in centre_receipt_rounds(ora.hop).items():
        hit = sorted(r for r in rs if forms[r] in under_test)
        assert hit, (d, sorted(rs), forms)
    np.testing.assert_array_equal(seen, ora.hop >= 0)
    np.testing.assert_array_equal(hop, ora.hop)
    np.testing.assert_array_equal(parent, ora.parent)
    assert_rounds_equal(rounds, ora.rounds)
