"""Hop limits on the CPU: tests/ttl_ref.py (the numpy restatement the GPU tests compare the engine
with) is pinned bit for bit to the ttl/ fixtures, which were produced by the reference's own Node
objects under a dedup app that forwards ``ttl - 1`` while ``ttl > 0``
(tests/golden/make_ttl_golden.py); without limits it is late_ref; it has the prefix property; and
the library exports p2pg_set_ttl and rejects the calls that need no device."""
import ctypes
import functools
import os

import numpy as np
import pytest

import late_ref
import ttl_ref
from conftest import GOLDEN, golden_cases

TTL = os.path.join(GOLDEN, "ttl")
TTL_CASES = ("ttl_ba300_gossip_k2", "ttl_ba300_gossip_k2_churn10", "ttl_rrg200_flood",
             "ttl_ws300_flood_churn10")
TTLS = {0, 1, 2, 3, 4, 6, -1}


def load_ttl(name):
    with np.load(os.path.join(TTL, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def cfg_of(z):
    return (str(z["mode"]), int(z["fanout"]), int(z["gossip_seed"]), 0, int(z["churn_threshold"]),
            int(z["churn_seed"]))


@functools.lru_cache(maxsize=None)
def ref_of(name):
    """ttl_ref on a fixture's inputs (computed once, shared, never written to)."""
    z = load_ttl(name)
    return ttl_ref.run(z["rowptr"], z["colidx"], z["src"], z["start"], z["ttl"], *cfg_of(z))


@functools.lru_cache(maxsize=None)
def unlimited_of(name):
    z = load_ttl(name)
    return late_ref.run(z["rowptr"], z["colidx"], z["src"], z["start"], *cfg_of(z))


def test_the_four_ttl_fixtures_are_there_and_hold_what_the_generator_asserts():
    assert tuple(sorted(f[:-4] for f in os.listdir(TTL) if f.endswith(".npz"))) == TTL_CASES
    # the parametrised tests over tests/golden/*.npz must not pick them up
    assert not [c for c in golden_cases() + golden_cases(dynamic=True) if c.startswith("ttl")]
    for name in TTL_CASES:
        z = load_ttl(name)
        assert os.path.getsize(os.path.join(TTL, name + ".npz")) < 100_000
        late = load_late_twin(name)
        np.testing.assert_array_equal(z["rowptr"], late["rowptr"])  # the late fixtures' graphs
        np.testing.assert_array_equal(z["colidx"], late["colidx"])
        start, ttl, hop = z["start"].astype(np.int64), z["ttl"].astype(np.int64), z["hop"]
        M = len(ttl)
        assert ttl.dtype == np.int64 and z["ttl"].dtype == np.int32 and set(ttl.tolist()) <= TTLS
        fin = ttl >= 0
        rel = np.where(hop >= 0, hop - start[None, :], -1)
        assert (rel[:, fin] <= ttl[fin][None, :]).all(), "no receipt past the hop limit"
        full = unlimited_of(name).hop
        same = ((hop >= 0) == (full >= 0)).all(axis=0)
        assert same[~fin].all()
        assert (fin & ~same).any(), "a message is cut short"
        assert (fin & same & (ttl > 0)).any(), "a finite-ttl message finishes inside its limit"
        assert (ttl == 0).sum() >= 1 and (ttl == -1).sum() >= 1
        xs = np.where(fin, start + ttl, -1)
        assert len(set(xs[fin].tolist())) >= 3, "3 distinct expiry rounds"
        assert set(xs[fin].tolist()) & set(start[start > 0].tolist()), "an expiry round that originates"
        words = np.arange(M) // 64
        ws = sorted(set(words.tolist()))
        assert any(len(set(xs[(words == w) & fin].tolist())) >= 2 for w in ws), \
            "two messages of one word expire in different rounds"
        if M > 64:
            assert any(any((xs[words == w] == r).all() for w in ws) and
                       any(not (xs[words == w] == r).any() for w in ws)
                       for r in set(xs[fin].tolist())), "a word expires whole beside an untouched one"


def load_late_twin(name):
    with np.load(os.path.join(GOLDEN, "late", name.replace("ttl_", "late_", 1) + ".npz"),
                 allow_pickle=False) as z:
        return {k: z[k] for k in ("rowptr", "colidx")}


@pytest.mark.parametrize("name", TTL_CASES)
def test_ttl_ref_equals_the_reference_nodes(name):
    z = load_ttl(name)
    res = ref_of(name)
    np.testing.assert_array_equal(res.hop, z["hop"])
    np.testing.assert_array_equal(res.parent, z["parent"])
    assert late_ref.pad_equal(res.column("relays"), z["round_relays"])
    assert int(res.column("received").sum()) == int(z["total_recv"])
    np.testing.assert_array_equal(res.peer_sent, z["peer_sent"])
    np.testing.assert_array_equal(res.peer_recv, z["peer_recv"])
    # the sends it lists are the sends it counts, and the arrivals are the ones not lost
    for r, (snd, rcv, msg, lost) in enumerate(res.sends):
        assert len(snd) == res.rounds[r]["relays"]
        if r + 1 < len(res.rounds):
            assert int((~lost).sum()) == res.rounds[r + 1]["received"]
    # ttl 0: seen at the origin only, nothing sent
    for m in np.nonzero(z["ttl"] == 0)[0]:
        assert (z["hop"][:, m] >= 0).sum() == 1 and z["hop"][z["src"][m], m] == z["start"][m]
        assert not any((s[2] == m).any() for s in res.sends)


@pytest.mark.parametrize("name", TTL_CASES)
def test_ttl_ref_has_the_prefix_property(name):
    z = load_ttl(name)
    res, full = ref_of(name), unlimited_of(name)
    hop, parent = ttl_ref.cut_at_ttl(full.hop, full.parent, z["start"], z["ttl"])
    np.testing.assert_array_equal(res.hop, hop)
    np.testing.assert_array_equal(res.parent, parent)
    # nothing of message m is sent in or after its expiry round
    x = np.where(z["ttl"] >= 0, z["start"].astype(np.int64) + z["ttl"], np.iinfo(np.int64).max)
    for r, (_, _, msg, _) in enumerate(res.sends):
        assert (x[msg] > r).all()


@pytest.mark.parametrize("name", TTL_CASES)
def test_ttl_ref_without_limits_is_late_ref(name):
    z = load_ttl(name)
    res = ttl_ref.run(z["rowptr"], z["colidx"], z["src"], z["start"], np.full(len(z["src"]), -1),
                      *cfg_of(z))
    full = unlimited_of(name)
    np.testing.assert_array_equal(res.hop, full.hop)
    np.testing.assert_array_equal(res.parent, full.parent)
    np.testing.assert_array_equal(res.peer_sent, full.peer_sent)
    np.testing.assert_array_equal(res.peer_recv, full.peer_recv)
    assert res.rounds == full.rounds


def test_library_exports_the_hop_limit_entry_point():
    from p2pnetwork.gpu import _lib
    L = _lib.lib()
    assert hasattr(L, "p2pg_set_ttl") and "p2pg_set_ttl" in _lib.SIGNATURES
    one = np.zeros(1, dtype=np.int32)
    # no engine: rejected before any device is touched
    assert L.p2pg_set_ttl(None, 1, _lib.ptr(one)) == -1
    assert b"set_ttl" in L.p2pg_global_error()
    assert L.p2pg_set_ttl(None, 1, None) == -1
    assert L.p2pg_set_ttl.argtypes[1] is ctypes.c_int32


def test_graphnetwork_has_the_hop_limit_interface():
    import inspect
    from p2pnetwork.gpu import GraphNetwork
    assert list(inspect.signature(GraphNetwork.broadcast).parameters)[1:] == ["sources", "start_rounds", "ttl"]
    assert inspect.signature(GraphNetwork.broadcast).parameters["ttl"].default is None
    assert list(inspect.signature(GraphNetwork.set_ttl).parameters)[1:] == ["ttl"]
    assert list(inspect.signature(GraphNetwork.originate).parameters)[1:] == ["msgs", "peers", "round"]
