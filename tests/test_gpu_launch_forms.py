"""Every branch of the kernel launch layer against the oracle, bit for bit.

The launchers pick a kernel instance by row width (W = words of 64 broadcasts), fanout (1..4 are
compile-time instances, any other one takes the generic one) and churn (on / off).  One graph with
narrow, chunked (deg > 16, > 64) and hub (deg > 512) senders runs one message count per width
class the launchers distinguish, each with a (fanout, churn) pair such that between them every
fanout case and both churn values occur, under the two push forms that between them reach the
dense launchers: edge stores (one unfused round, then fused rounds; the last dense pull) and the
automatic switch with the update+push pass (sparse pushes, updates, the first dense round).
"""
import functools

import numpy as np
import pytest

from test_gpu_parity import assert_rounds_equal, gpu_net, make_graph, oracle_for

pytestmark = pytest.mark.gpu

# (M, fanout, churn threshold)
CASES = [
    (64, 1, 0),                # W = 1
    (128, 2, 300_000_000),     # W = 2
    (256, 3, 0),               # W = 4
    (512, 4, 300_000_000),     # W = 8: plain rows, grouped
    (1024, 5, 0),              # W = 16: packed, grouped
    (2048, 3, 300_000_000),    # W = 32: half-width fused, paired update
    (4096, 2, 0),              # W = 64: fused, dual update
    (4160, 1, 300_000_000),    # W = 65: the unpacked fallbacks
]


@functools.lru_cache(maxsize=None)
def graph():
    return make_graph("hub", dict(V=1500, m=3, star=300), 0x1A7)


@functools.lru_cache(maxsize=1)  # the forms of one case run back to back
def reference(M, fanout, thr):
    from p2pnetwork.gpu import make_sources
    g = graph()
    src = make_sources(g.V, M, seed=3 + M)
    ora = oracle_for(g.rowptr, g.colidx, src, "gossip", fanout, 99 + M, thr, 5 + M)
    for a in (ora.hop, ora.parent):
        a.setflags(write=False)
    return src, ora


@pytest.mark.parametrize("form", ["store", "auto_update"])  # (varies fastest)
@pytest.mark.parametrize("M,fanout,thr", CASES)
def test_launch_forms_match_oracle(M, fanout, thr, form, monkeypatch):
    monkeypatch.setenv("P2PG_GOSSIP_PUSH", form.split("_")[0])
    if form == "auto_update":
        monkeypatch.setenv("P2PG_UPDATE_PUSH", "1")
    src, ora = reference(M, fanout, thr)
    with gpu_net(graph(), "gossip", fanout, 99 + M, thr, 5 + M) as net:
        net.broadcast(src)
        rounds = net.run()
        hop, parent = net.hop_parent()
    forms = [r.push_form for r in rounds if r.new_deliveries]
    print(form, "M", M, "push forms", forms)
    # not vacuous: the dense launchers ran where the row width admits them
    if form == "auto_update":
        assert (4 in forms) == (1024 < M <= 4096), forms
    elif M <= 4096:
        assert forms[0] == 2 and forms[1:] and all(f == 3 for f in forms[1:]), forms
    else:
        assert all(f == 2 for f in forms), forms
    np.testing.assert_array_equal(hop, ora.hop)
    np.testing.assert_array_equal(parent, ora.parent)
    assert_rounds_equal(rounds, ora.rounds)
