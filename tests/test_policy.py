"""The relay policy on the CPU: tests/policy_ref.py (the numpy draw and the drop_ref rule the GPU
tests compare the engine with) is pinned bit for bit to the policy/ fixtures, which were produced
by the reference's own Node objects under a dedup app that forwards a first receipt iff its policy
draw says so (tests/golden/make_policy_golden.py); with all-zero thresholds it is late_ref; the
library's host draw p2pg_relay_muted is the numpy draw; and all-silent peers end every broadcast at
its origin's connections."""
import ctypes
import functools
import os

import numpy as np
import pytest

import drop_ref
import late_ref
import policy_ref
from conftest import GOLDEN, golden_cases

POLICY = os.path.join(GOLDEN, "policy")
POLICY_CASES = ("policy_ba300_gossip_k2", "policy_ba300_gossip_k2_churn10", "policy_rrg200_flood",
                "policy_ws300_flood_churn10")
SILENT = 0xFFFFFFFF
THRS = {0, SILENT, 1, 1 << 31, 0xFFFFFFFE}


def load_policy(name):
    with np.load(os.path.join(POLICY, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def cfg_of(z):
    return (str(z["mode"]), int(z["fanout"]), int(z["gossip_seed"]), 0, int(z["churn_threshold"]),
            int(z["churn_seed"]))


def rule_of(z):
    return policy_ref.with_ttl(policy_ref.policy_rule(z["thr"], int(z["policy_seed"]), z["start"]),
                               z["start"], z["ttl"])


@functools.lru_cache(maxsize=None)
def ref_of(name):
    """drop_ref under the policy rule on a fixture's inputs (computed once, shared, never written to)."""
    z = load_policy(name)
    return drop_ref.run(z["rowptr"], z["colidx"], z["src"], z["start"], rule_of(z), *cfg_of(z))


@functools.lru_cache(maxsize=None)
def unmuted_of(name):
    z = load_policy(name)
    return late_ref.run(z["rowptr"], z["colidx"], z["src"], z["start"], *cfg_of(z))


def test_the_four_policy_fixtures_are_there_and_hold_what_the_generator_asserts():
    assert tuple(sorted(f[:-4] for f in os.listdir(POLICY) if f.endswith(".npz"))) == POLICY_CASES
    # the parametrised tests over tests/golden/*.npz must not pick them up
    assert not [c for c in golden_cases() + golden_cases(dynamic=True) if c.startswith("policy")]
    with_ttl = 0
    for name in POLICY_CASES:
        z = load_policy(name)
        assert os.path.getsize(os.path.join(POLICY, name + ".npz")) < 100_000
        with np.load(os.path.join(GOLDEN, "late", name.replace("policy_", "late_", 1) + ".npz"),
                     allow_pickle=False) as late:  # the late fixtures' graphs and schedules
            for key in ("rowptr", "colidx", "src", "start"):
                np.testing.assert_array_equal(z[key], late[key])
        assert z["thr"].dtype == np.uint32 and set(z["thr"].tolist()) == THRS
        res = ref_of(name)
        thr, hop, parent = z["thr"].astype(np.int64), z["hop"], z["parent"]
        start, ttl, src = z["start"].astype(np.int64), z["ttl"].astype(np.int64), z["src"]
        V, M = hop.shape
        deg = np.diff(z["rowptr"])
        gossip, k = str(z["mode"]) == "gossip", int(z["fanout"])
        drawn, silent = (thr != 0) & (thr != SILENT), thr == SILENT
        got = dict.fromkeys(("mixed_word", "silent_receipt", "silent_origin", "busy_origin", "gossip_deg",
                             "expired_and_muted"), False)
        for r, gone in enumerate(res.dropped):
            new = hop == r
            relayed = new & ~gone & (parent >= 0)
            pol = gone & policy_ref.muted_plane(r, thr, M, int(z["policy_seed"]))
            for w in range((M + 63) // 64):
                sl = slice(64 * w, 64 * w + 64)
                got["mixed_word"] |= bool((drawn & pol[:, sl].any(axis=1) & relayed[:, sl].any(axis=1)).any())
            got["silent_receipt"] |= bool((silent & (deg >= 2) & (new & (parent >= 0)).any(axis=1)).any())
            got["gossip_deg"] |= bool((pol.any(axis=1) & (deg > k)).any())
            got["expired_and_muted"] |= bool((pol & (r - start == ttl)[None, :] & (start != r)[None, :]).any())
            for m in np.nonzero(start == r)[0] if r else ():
                s = int(src[m])
                sent = bool(((res.sends[r][0] == s) & (res.sends[r][2] == m)).any())
                got["silent_origin"] |= bool(silent[s]) and sent
                got["busy_origin"] |= bool((new[s] & (parent[s] >= 0)).any())
        need = ["mixed_word", "silent_receipt", "silent_origin", "busy_origin"]
        need += ["gossip_deg"] if gossip else []
        if (ttl >= 0).any():
            with_ttl += 1
            need.append("expired_and_muted")
        assert all(got[key] for key in need), (name, got)
        wide = ((hop >= 0).sum(axis=0) * 2 >= V).sum()
        full = unmuted_of(name).hop
        wide_full = ((full >= 0).sum(axis=0) * 2 >= V).sum()
        if wide_full * 2 >= M:
            assert wide * 2 >= M, (name, wide)
        else:  # (the k = 2 gossip under churn: see the generator)
            assert wide * 2 >= wide_full and (hop >= 0).sum() * 10 >= (full >= 0).sum() * 9, (name, wide, wide_full)
    assert with_ttl >= 1, "one fixture carries hop limits"


@pytest.mark.parametrize("name", POLICY_CASES)
def test_policy_ref_equals_the_reference_nodes(name):
    z = load_policy(name)
    res = ref_of(name)
    np.testing.assert_array_equal(res.hop, z["hop"])
    np.testing.assert_array_equal(res.parent, z["parent"])
    assert late_ref.pad_equal(res.column("relays"), z["round_relays"])
    assert int(res.column("received").sum()) == int(z["total_recv"])
    np.testing.assert_array_equal(res.peer_sent, z["peer_sent"])
    np.testing.assert_array_equal(res.peer_recv, z["peer_recv"])
    # the sends it lists are the sends it counts; no muted receipt and no silent peer's relay is in them
    thr = z["thr"].astype(np.int64)
    for r, (snd, rcv, msg, lost) in enumerate(res.sends):
        assert len(snd) == res.rounds[r]["relays"]
        assert not res.dropped[r][snd, msg].any()
        assert (z["start"][msg[thr[snd] == SILENT]] == r).all()  # a silent peer sends its own only
        if r + 1 < len(res.rounds):
            assert int((~lost).sum()) == res.rounds[r + 1]["received"]


@pytest.mark.parametrize("name", POLICY_CASES)
def test_all_zero_thresholds_are_late_ref(name):
    z = load_policy(name)
    res = drop_ref.run(z["rowptr"], z["colidx"], z["src"], z["start"],
                       policy_ref.policy_rule(np.zeros_like(z["thr"]), int(z["policy_seed"]), z["start"]),
                       *cfg_of(z))
    full = unmuted_of(name)
    np.testing.assert_array_equal(res.hop, full.hop)
    np.testing.assert_array_equal(res.parent, full.parent)
    np.testing.assert_array_equal(res.peer_sent, full.peer_sent)
    np.testing.assert_array_equal(res.peer_recv, full.peer_recv)
    assert res.rounds == full.rounds


def test_host_draw_equals_the_numpy_draw():
    from p2pnetwork.gpu import GraphNetwork, _lib
    L = _lib.lib()
    assert "p2pg_relay_muted" in _lib.SIGNATURES
    rng = np.random.default_rng(5)
    n = 4000
    rnd = rng.integers(0, 1 << 31, n)
    peer = rng.integers(0, 1 << 31, n)
    msg = rng.integers(0, 1 << 32, n)
    thr = rng.integers(0, 1 << 32, n)
    edge = np.array([0, 1, 2, 1 << 31, 0xFFFFFFFE, SILENT])
    thr[:600] = np.repeat(edge, 100)
    rnd[:20], peer[20:40], msg[40:60] = 0, 0, 0xFFFFFFFF
    for seed in (0, 0xA11CE, 0xFEDCBA9876543210):
        want = policy_ref.muted(rnd, peer, msg, thr, seed)
        got = [L.p2pg_relay_muted(int(a), int(b), int(c), int(d), seed) for a, b, c, d in zip(rnd, peer, msg, thr)]
        np.testing.assert_array_equal(np.array(got, dtype=bool), want)
        assert GraphNetwork.relay_muted(int(rnd[700]), int(peer[700]), int(msg[700]), int(thr[700]), seed) == want[700]
    assert not want[:100].any() and want[500:600].all()       # 0 never mutes, 0xFFFFFFFF always
    assert not want[100:200].any() and want[400:500].all()    # 1 and 0xFFFFFFFE: all but never / always
    assert 0.4 < want[300:400].mean() < 0.6                   # 2^31: half


def test_probabilities_map_to_thresholds():
    from p2pnetwork.gpu import GraphNetwork
    t = GraphNetwork.relay_thresholds([1.0, 0.0, 0.5, 0.75, 1e-12, 1.0 - 1e-12], 6)
    assert t.dtype == np.uint32
    assert t.tolist() == [0, SILENT, 1 << 31, 1 << 30, 0xFFFFFFFE, 1]
    np.testing.assert_array_equal(t, policy_ref.thresholds([1.0, 0.0, 0.5, 0.75, 1e-12, 1.0 - 1e-12], 6))
    assert GraphNetwork.relay_thresholds(0.5, 3).tolist() == [1 << 31] * 3
    for bad in (-0.1, 1.1, [0.5, 0.5]):
        with pytest.raises(ValueError):
            GraphNetwork.relay_thresholds(bad, 3)


@pytest.mark.parametrize("name", POLICY_CASES)
def test_all_silent_peers_end_every_broadcast_at_its_origins_connections(name):
    z = load_policy(name)
    V, M = z["hop"].shape
    thr = np.full(V, SILENT, dtype=np.uint32)
    res = drop_ref.run(z["rowptr"], z["colidx"], z["src"], z["start"],
                       policy_ref.policy_rule(thr, 7, z["start"]), *cfg_of(z))
    full = unmuted_of(name)
    start = z["start"].astype(np.int64)
    rel = np.where(res.hop >= 0, res.hop - start[None, :], -1)
    assert rel.max() == 1  # the origin and what it sent to, nothing further
    # exactly the origin and the connections its own sends reached
    for m in range(M):
        got = res.hop[:, m] >= 0
        assert got[z["src"][m]] and res.hop[z["src"][m], m] == start[m]
        nb = z["colidx"][z["rowptr"][z["src"][m]]:z["rowptr"][z["src"][m] + 1]]
        assert set(np.nonzero(got)[0].tolist()) <= set(nb.tolist()) | {int(z["src"][m])}
        if str(z["mode"]) == "flood" and int(z["churn_threshold"]) == 0:
            assert set(np.nonzero(got)[0].tolist()) == set(nb.tolist()) | {int(z["src"][m])}
    # the run ends: the last origination's sends arrive one round later, and nothing follows them
    assert len(res.rounds) <= int(start.max()) + 3 and res.rounds[-1]["new_deliveries"] == 0
    assert sum(x["relays"] for x in res.rounds) < sum(x["relays"] for x in full.rounds)


def test_library_exports_the_relay_policy_entry_points():
    from p2pnetwork.gpu import _lib
    L = _lib.lib()
    assert hasattr(L, "p2pg_set_relay_policy") and "p2pg_set_relay_policy" in _lib.SIGNATURES
    one = np.zeros(1, dtype=np.uint32)
    # no engine: rejected before any device is touched
    assert L.p2pg_set_relay_policy(None, 1, _lib.ptr(one), 0) == -1
    assert b"set_relay_policy" in L.p2pg_global_error()
    assert L.p2pg_set_relay_policy.argtypes[1] is ctypes.c_int64
    assert L.p2pg_set_relay_policy.argtypes[3] is ctypes.c_uint64


def test_graphnetwork_has_the_relay_policy_interface():
    import inspect
    from p2pnetwork.gpu import GraphNetwork
    sig = inspect.signature(GraphNetwork.set_relay_policy)
    assert list(sig.parameters)[1:] == ["relay_prob", "thresholds", "seed"]
    assert sig.parameters["relay_prob"].default is None
    assert sig.parameters["thresholds"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["seed"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["seed"].default == 0
