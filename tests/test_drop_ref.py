"""Withdrawn relays on the CPU: tests/drop_ref.py (the numpy restatement tests/test_gpu_drop.py
compares the engine with) is pinned to the two yardsticks it generalises -- without drops it is
late_ref, with the receipts at relative hop ttl[m] dropped it is ttl_ref, round for round -- and to
the per-bit stand-in of tests/partition_mock.py driven through step / deliveries / drop_relays /
sends with the GPU tests' drop rule."""
import numpy as np
import pytest

import drop_ref
import late_ref
import ttl_ref
from test_ttl import TTL_CASES, cfg_of, load_ttl, ref_of, unlimited_of

CHURN = 430_000_000


def assert_same_run(res, want, sends=True):
    np.testing.assert_array_equal(res.hop, want.hop)
    np.testing.assert_array_equal(res.parent, want.parent)
    np.testing.assert_array_equal(res.peer_sent, want.peer_sent)
    np.testing.assert_array_equal(res.peer_recv, want.peer_recv)
    assert res.rounds == want.rounds  # every counter of every round, and the number of rounds
    if sends:
        assert len(res.sends) == len(want.sends)
        for a, b in zip(res.sends, want.sends):
            for x, y in zip(a, b):
                np.testing.assert_array_equal(x, y)


def random_schedule(mode):
    from p2pnetwork.gpu import PeerGraph, make_sources
    seed = 23 if mode == "flood" else 29
    g = PeerGraph.barabasi_albert(300, 3, seed=seed)
    M = 130
    rng = np.random.default_rng(seed)
    src = make_sources(g.V, M, seed=seed).astype(np.int32)
    start = rng.integers(0, 5, M).astype(np.int32)
    ttl = np.array([0, 1, 2, 3, 4, 6, -1], dtype=np.int32)[rng.integers(0, 7, M)]
    ttl[0], ttl[1], start[0] = 0, -1, 0
    return g, src, start, ttl, (mode, 2, seed + 1, 0, CHURN, seed + 2)


# ---- 1. no drops: late_ref -----------------------------------------------------------------------
@pytest.mark.parametrize("name", TTL_CASES)
def test_drop_ref_without_drops_is_late_ref(name):
    z = load_ttl(name)
    res = drop_ref.run(z["rowptr"], z["colidx"], z["src"], z["start"], drop_ref.no_drop, *cfg_of(z))
    assert_same_run(res, unlimited_of(name), sends=False)
    assert res.relays_offered == [r["relays"] for r in res.rounds]
    assert not any(d.any() for d in res.dropped)
    # round_sends (the GPU tests' list of a round's sends before its drop) on a finished run's planes
    for r in (0, 2, len(res.rounds) - 2):
        got = drop_ref.round_sends(z["rowptr"], z["colidx"], r, res.hop == r, res.parent, *cfg_of(z))
        for x, y in zip(got, res.sends[r]):
            np.testing.assert_array_equal(x, y)


# ---- 2. the receipts at relative hop ttl[m] dropped: ttl_ref -----------------------------------------
def check_against_ttl_ref(res, want, full):
    assert_same_run(res, want)
    # up to the first drop the offered relays are the unlimited run's
    first = next(r for r, d in enumerate(res.dropped) if d.any())
    assert res.relays_offered[:first + 1] == full.column("relays")[:first + 1].tolist()
    cut = sum(int(d.sum()) for d in res.dropped)
    assert cut > 0 and any(o > r["relays"] for o, r in zip(res.relays_offered, res.rounds))
    for r, d in enumerate(res.dropped):  # a dropped receipt happened in that round
        assert (res.hop[d] == r).all()


@pytest.mark.parametrize("name", TTL_CASES)
def test_drop_ref_with_the_ttl_rule_is_ttl_ref_on_the_fixtures(name):
    z = load_ttl(name)
    res = drop_ref.run(z["rowptr"], z["colidx"], z["src"], z["start"],
                       drop_ref.ttl_rule(z["start"], z["ttl"]), *cfg_of(z))
    check_against_ttl_ref(res, ref_of(name), unlimited_of(name))
    np.testing.assert_array_equal(res.hop, z["hop"])  # ... which are the reference's own Node objects
    np.testing.assert_array_equal(res.parent, z["parent"])


@pytest.mark.parametrize("mode", ["flood", "gossip"])
def test_drop_ref_with_the_ttl_rule_is_ttl_ref_on_random_schedules_with_churn(mode):
    g, src, start, ttl, cfg = random_schedule(mode)
    want = ttl_ref.run(g.rowptr, g.colidx, src, start, ttl, *cfg)
    full = late_ref.run(g.rowptr, g.colidx, src, start, *cfg)
    res = drop_ref.run(g.rowptr, g.colidx, src, start, drop_ref.ttl_rule(start, ttl), *cfg)
    check_against_ttl_ref(res, want, full)
    assert any(lost.any() for _, _, _, lost in res.sends), "no churn"


# ---- 3. the per-bit stand-in, driven as the GPU tests drive the engine ----------------------------------
MOCK_CASES = [
    # V, M, mode, fanout, churn threshold
    (120, 70, "flood", 3, 0),
    (110, 70, "flood", 3, CHURN),
    (120, 70, "gossip", 3, 0),
    (100, 33, "gossip", 2, CHURN),
]


@pytest.mark.parametrize("V,M,mode,k,thr", MOCK_CASES)
def test_drop_ref_equals_the_mock_engine(V, M, mode, k, thr):
    from partition_mock import MockEngine
    from p2pnetwork.gpu import PeerGraph, make_sources
    g = PeerGraph.barabasi_albert(V, 3, seed=V + M)
    src = make_sources(g.V, M, seed=M).astype(np.int32)
    drops = {1, 2, 3, 4}
    rule = drop_ref.issue_rule(g.rowptr, M, drops)
    ref = drop_ref.run(g.rowptr, g.colidx, src, np.zeros(M, np.int32), rule, mode, k, 17, 0, thr, 3)
    eng = MockEngine(g, mode, k, 17, thr, 3)
    eng.broadcast(src)
    r = 0
    while True:
        st = eng.step()
        assert st.round == r and st.new_deliveries == ref.rounds[r]["new_deliveries"]
        if mode == "gossip" or r > 0:  # (the stand-in does not count a flood origin's extra send)
            assert st.relays == ref.relays_offered[r]
        d = eng.deliveries()
        new = np.zeros((g.V, M), dtype=bool)
        new[d.peer, d.msg] = True
        np.testing.assert_array_equal(new, ref.hop == r)
        vs, ms = np.nonzero(rule(r, new))
        np.testing.assert_array_equal(rule(r, new), ref.dropped[r])
        if len(vs):
            eng.drop_relays(vs[::-1], ms[::-1])
        s = eng.sends()
        snd, rcv, msg, lost = ref.sends[r]
        np.testing.assert_array_equal(s.sender, snd)
        np.testing.assert_array_equal(s.receiver, rcv)
        np.testing.assert_array_equal(s.msg, msg)
        np.testing.assert_array_equal(s.lost, lost)
        if not st.new_deliveries:
            break
        r += 1
    assert r + 1 == len(ref.rounds)
    hop, par = eng.hop_parent()
    np.testing.assert_array_equal(hop, ref.hop)
    np.testing.assert_array_equal(par, ref.parent)
    np.testing.assert_array_equal(eng.seen, ref.hop >= 0)
    # not vacuous: every drop round dropped some receipts and kept some, and the run went on
    for x in sorted(drops):
        kept = (ref.hop == x) & ~ref.dropped[x]
        assert ref.dropped[x].any() and kept.any(), x
    assert sum(rr["new_deliveries"] > 0 for rr in ref.rounds[max(drops) + 1:]) >= 1
    if thr:
        assert any(lo.any() for _, _, _, lo in ref.sends)


def test_issue_rule_is_what_the_gpu_tests_say_it_is():
    rowptr = np.array([0, 1, 4, 5, 6, 6, 6, 6, 6, 6, 6, 6])  # peer 1 has the most connections
    V, M = 11, 70
    new = np.ones((V, M), dtype=bool)
    rule = drop_ref.issue_rule(rowptr, M, {2, 3, 4})
    assert not rule(1, new).any() and not rule(5, new).any()
    v, m = np.arange(V)[:, None], np.arange(M)[None, :]
    np.testing.assert_array_equal(rule(2, new), (7 * v + 13 * m + 2) % 3 == 0)
    np.testing.assert_array_equal(rule(3, new), ((7 * v + 13 * m + 3) % 3 == 0) | (m >= 64) | (v == 1))
    np.testing.assert_array_equal(rule(4, new), ((7 * v + 13 * m + 4) % 3 == 0) | (v % 5 == 0))
    one = drop_ref.issue_rule(rowptr, 60, {3})(3, np.ones((V, 60), dtype=bool))
    assert one[:, 32:].all() and not one[0, :32].all()  # W = 1: the upper half of the only word
    assert not rule(3, np.zeros((V, M), dtype=bool)).any()  # only first receipts
    plain = drop_ref.issue_rule(rowptr, M, {3}, extras=False)
    np.testing.assert_array_equal(plain(3, new), (7 * v + 13 * m + 3) % 3 == 0)
