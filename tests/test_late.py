"""Start rounds on the CPU: tests/late_ref.py (the numpy restatement the GPU tests compare the
engine with) is pinned bit for bit to the late/ fixtures, which were produced by the reference's
own Node objects (tests/golden/make_late_golden.py); and the library exports the two entry points
and rejects the calls that need no device."""
import ctypes
import os

import numpy as np
import pytest

import late_ref
from conftest import GOLDEN, golden_cases

LATE = os.path.join(GOLDEN, "late")
LATE_CASES = ("late_ba300_gossip_k2", "late_ba300_gossip_k2_churn10", "late_rrg200_flood",
              "late_ws300_flood_churn10")


def load_late(name):
    with np.load(os.path.join(LATE, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def ref_of(z, **kw):
    return late_ref.run(z["rowptr"], z["colidx"], z["src"], z["start"], str(z["mode"]), int(z["fanout"]),
                        int(z["gossip_seed"]), 0, int(z["churn_threshold"]), int(z["churn_seed"]), **kw)


def test_the_four_late_fixtures_are_there_and_apart():
    assert tuple(sorted(f[:-4] for f in os.listdir(LATE) if f.endswith(".npz"))) == LATE_CASES
    # the parametrised tests over tests/golden/*.npz must not pick them up
    assert not [c for c in golden_cases() + golden_cases(dynamic=True) if c.startswith("late")]
    for name in LATE_CASES:
        z = load_late(name)
        assert os.path.getsize(os.path.join(LATE, name + ".npz")) < 100_000
        start, src = z["start"], z["src"]
        assert start.min() == 0 and (start > 0).sum() > len(start) // 2
        quiet = np.nonzero(z["round_relays"] == 0)[0]
        assert len(quiet) and start.max() > quiet[0], "a start well after the first quiet round"
        pairs = list(zip(src.tolist(), start.tolist()))
        assert len(set(pairs)) < len(pairs), "several messages share one origin and round"


@pytest.mark.parametrize("name", LATE_CASES)
def test_late_ref_equals_the_reference_nodes(name):
    z = load_late(name)
    res = ref_of(z)
    np.testing.assert_array_equal(res.hop, z["hop"])
    np.testing.assert_array_equal(res.parent, z["parent"])
    assert late_ref.pad_equal(res.column("relays"), z["round_relays"])
    assert int(res.column("received").sum()) == int(z["total_recv"])
    np.testing.assert_array_equal(res.peer_sent, z["peer_sent"])
    np.testing.assert_array_equal(res.peer_recv, z["peer_recv"])
    # an origination is a first receipt of its start round at its origin, parent -1
    m = np.arange(len(z["src"]))
    np.testing.assert_array_equal(z["hop"][z["src"], m], z["start"])
    assert (z["parent"][z["src"], m] == -1).all()
    assert (z["hop"][z["hop"] >= 0] >= np.broadcast_to(z["start"], z["hop"].shape)[z["hop"] >= 0]).all()
    # the run crosses its idle gaps: a round per index up to the last start and beyond
    assert len(res.rounds) > int(z["start"].max())
    assert res.rounds[-1]["new_deliveries"] == 0 and res.rounds[0]["received"] == 0


def test_late_ref_with_all_starts_zero_is_the_oracle():
    from oracle import relay_oracle
    from p2pnetwork.gpu import PeerGraph, make_sources
    g = PeerGraph.barabasi_albert(200, 3, seed=5)
    src = make_sources(g.V, 70, seed=5)
    for mode, thr in (("flood", 0), ("gossip", 0), ("gossip", 400_000_000), ("flood", 400_000_000)):
        res = late_ref.run(g.rowptr, g.colidx, src, np.zeros(70, np.int32), mode, 2, 9, 0, thr, 4)
        ora = (relay_oracle.flood(g.rowptr, g.colidx, src, thr, 4) if mode == "flood" else
               relay_oracle.gossip(g.rowptr, g.colidx, src, 2, 9, 0, thr, 4))
        np.testing.assert_array_equal(res.hop, ora.hop)
        np.testing.assert_array_equal(res.parent, ora.parent)
        assert len(res.rounds) == len(ora.rounds)
        for a, b in zip(res.rounds, ora.rounds):
            assert {k: a[k] for k in b} == b


def test_library_exports_the_start_round_entry_points():
    from p2pnetwork.gpu import _lib
    L = _lib.lib()
    for name in ("p2pg_set_sources_at", "p2pg_originate"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    one = np.zeros(1, dtype=np.int32)
    # no engine: rejected before any device is touched
    assert L.p2pg_set_sources_at(None, 1, _lib.ptr(one), _lib.ptr(one)) == -1
    assert L.p2pg_originate(None, 1, _lib.ptr(one), _lib.ptr(one), 1) == -1
    assert b"originate" in L.p2pg_global_error()
    assert L.p2pg_originate.argtypes[-1] is ctypes.c_int32


def test_graphnetwork_has_the_start_round_interface():
    import inspect
    from p2pnetwork.gpu import GraphNetwork
    assert "start_rounds" in inspect.signature(GraphNetwork.broadcast).parameters
    assert list(inspect.signature(GraphNetwork.originate).parameters)[1:] == ["msgs", "peers", "round"]
    assert inspect.signature(GraphNetwork.hop_parent).parameters["relative"].default is False
    assert "start_rounds" in GraphNetwork.message_tally.__doc__
