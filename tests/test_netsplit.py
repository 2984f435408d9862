"""Network partitions on the CPU: tests/netsplit_ref.py (the numpy restatement the GPU tests compare
the engine with) is pinned bit for bit to the netsplit/ fixtures, which were produced by the
reference's own Node objects with one more term in the harness's dropped(a, b)
(tests/golden/make_netsplit_golden.py); with equal sides it is pull_ref / down_ref; the census holds
from the data; the packed flood agrees with the loop; and the laws of the rule hold."""
import functools
import os

import numpy as np
import pytest

import down_ref
import netsplit_ref
import pull_ref
from conftest import GOLDEN, golden_cases

NETSPLIT = os.path.join(GOLDEN, "netsplit")
NETSPLIT_CASES = ("ba300_gossip_k2", "ba300_gossip_k2_churn10", "rrg200_flood", "ws300_flood_churn10")


def load_netsplit(name):
    with np.load(os.path.join(NETSPLIT, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def cfg_of(z):
    return dict(mode=str(z["mode"]), fanout=int(z["fanout"]), gossip_seed=int(z["gossip_seed"]),
                churn_threshold=int(z["churn_threshold"]), churn_seed=int(z["churn_seed"]))


def setting_of(z):
    s = tuple(int(x) for x in z["anti_entropy"])
    return s if s[0] > 0 else None


@functools.lru_cache(maxsize=None)
def ref_of(name, pull=True):
    """netsplit_ref on a fixture's inputs (computed once, shared, never written to)."""
    z = load_netsplit(name)
    return netsplit_ref.run(z["rowptr"], z["colidx"], z["src"], z["start"], z["side"], int(z["cut_from"]),
                            int(z["cut_until"]), down_from=z["down_from"], down_until=z["down_until"],
                            anti_entropy=setting_of(z) if pull else None, pull_seed=int(z["pull_seed"]), **cfg_of(z))


def test_the_four_netsplit_fixtures_are_there_and_stand_on_the_pull_fixtures():
    # (dense2000_parent_rounds holds no run of the rule: the rounds of an engine without the call)
    assert tuple(sorted(f[:-4] for f in os.listdir(NETSPLIT) if f.endswith(".npz"))) == tuple(
        sorted(NETSPLIT_CASES + ("dense2000_parent_rounds",)))
    assert not [c for c in golden_cases() + golden_cases(dynamic=True) if c in NETSPLIT_CASES]
    asked, pulls, downs, sides = set(), 0, 0, set()
    for name in NETSPLIT_CASES:
        z = load_netsplit(name)
        assert os.path.getsize(os.path.join(NETSPLIT, name + ".npz")) < 100_000
        with np.load(os.path.join(GOLDEN, "pull", "pull_" + name + ".npz"), allow_pickle=False) as d:
            for key in ("rowptr", "colidx", "src", "start", "mode", "fanout", "gossip_seed", "churn_threshold", "churn_seed"):
                np.testing.assert_array_equal(z[key], d[key])
        cf, cu = int(z["cut_from"]), int(z["cut_until"])
        assert 0 <= cf < cu and (z["side"] >= 0).all() and z["side"].dtype == np.int32
        s = setting_of(z)
        if s:  # request rounds inside the window and after the heal
            pulls += 1
            rr = [r for r in range(s[1], s[2] + 1) if pull_ref.request_round(r, s)]
            assert any(cf <= r < cu for r in rr) and any(r >= cu for r in rr)
        downs += bool((z["down_from"] >= 0).any())
        sides.add(len(np.unique(z["side"])))
        asked |= set(str(x) for x in z["census"])
        assert set(str(x) for x in z["census"]) | set(str(x) for x in z["census_impossible"]) == set(netsplit_ref.CENSUS)
    assert pulls >= 2 and downs >= 1 and 3 in sides
    # every item holds in some fixture, but the one no fixture graph can have: a gossip sender of
    # degree > 64 (the widest peer of the 300-peer graph has 52 connections)
    assert set(netsplit_ref.CENSUS) - asked == {"hub_pick_wasted"}
    for name in NETSPLIT_CASES:
        assert int(np.diff(load_netsplit(name)["rowptr"]).max()) <= 64


@pytest.mark.parametrize("name", NETSPLIT_CASES)
def test_netsplit_ref_equals_the_reference_nodes_bit_for_bit(name):
    z, res = load_netsplit(name), ref_of(name)
    np.testing.assert_array_equal(res.hop, z["hop"])
    np.testing.assert_array_equal(res.parent, z["parent"])
    assert netsplit_ref.pad_equal(res.column("relays"), z["round_relays"])
    assert int(res.column("relays").sum()) == int(z["round_relays"].sum()) == int(z["peer_sent"].sum())
    assert res.received_total == int(res.peer_recv.sum()) == int(z["total_recv"])
    np.testing.assert_array_equal(res.peer_sent, z["peer_sent"])
    np.testing.assert_array_equal(res.peer_recv, z["peer_recv"])
    np.testing.assert_array_equal(res.records(), z["exchanges"])
    np.testing.assert_array_equal(res.pull_sent, z["pull_sent"])
    np.testing.assert_array_equal(res.pull_recv, z["pull_recv"])
    np.testing.assert_array_equal(res.msg_sent, z["msg_sent"])
    np.testing.assert_array_equal(res.msg_recv, z["msg_recv"])
    # the laws: the sum over m of sent is the sum of relays; received = sent - lost, per round
    assert int(res.msg_sent.sum()) == int(res.column("relays").sum())
    for r, (snd, tgt, msg, lost) in enumerate(res.sends):
        assert len(snd) == res.rounds[r]["relays"]
        if r + 1 < len(res.rounds):
            assert res.rounds[r + 1]["received"] == int((~lost).sum())
    # the histograms sum to the reach
    np.testing.assert_array_equal(res.latency.hist.sum(axis=1), (res.hop >= 0).sum(axis=0))


@pytest.mark.parametrize("name", NETSPLIT_CASES)
def test_census_holds_from_the_data(name):
    z, res = load_netsplit(name), ref_of(name)
    got = netsplit_ref.census(z, res, ref_of(name, pull=False))
    for item in z["census"]:
        assert got[str(item)], (name, str(item))
    for item in z["census_impossible"]:
        assert not got[str(item)], (name, str(item))
    # the cut holds: no first receipt of a cut round has a parent on another side
    side, cf, cu = z["side"], int(z["cut_from"]), int(z["cut_until"])
    vs, ms = np.nonzero((res.hop >= cf) & (res.hop < cu) & (res.parent >= 0))
    assert (side[vs] == side[res.parent[vs, ms]]).all()


@pytest.mark.parametrize("name", NETSPLIT_CASES)
def test_equal_sides_are_pull_ref_and_down_ref(name):
    z = load_netsplit(name)
    V = len(z["rowptr"]) - 1
    args = (z["rowptr"], z["colidx"], z["src"], z["start"])
    kw = dict(down_from=z["down_from"], down_until=z["down_until"], **cfg_of(z))
    for side, cf, cu in ((np.full(V, 3), 2, 9), (z["side"], 9, 9), (z["side"], 9, 2), (None, 2, 9)):
        a = netsplit_ref.run(*args, side, cf, cu, anti_entropy=setting_of(z), pull_seed=int(z["pull_seed"]), **kw)
        b = pull_ref.run(*args, anti_entropy=setting_of(z), pull_seed=int(z["pull_seed"]), **kw)
        np.testing.assert_array_equal(a.hop, b.hop)
        np.testing.assert_array_equal(a.parent, b.parent)
        assert a.rounds == b.rounds and a.exchanges == b.exchanges
    a = netsplit_ref.run(*args, np.full(V, 3), 2, 9, **kw)
    d = down_ref.run(*args, z["down_from"], z["down_until"], **cfg_of(z))
    np.testing.assert_array_equal(a.hop, d.hop)
    np.testing.assert_array_equal(a.parent, d.parent)
    assert a.rounds == d.rounds
    np.testing.assert_array_equal(a.peer_sent, d.peer_sent)
    np.testing.assert_array_equal(a.peer_recv, d.peer_recv)


@pytest.mark.parametrize("cthr", [0, 430_000_000])
def test_packed_flood_equals_the_loop(cthr):
    z = load_netsplit("ws300_flood_churn10")
    V = len(z["rowptr"]) - 1
    for side, cf, cu in ((z["side"], int(z["cut_from"]), int(z["cut_until"])), (np.arange(V) % 2, 1, 4), (None, 0, 0)):
        res = netsplit_ref.run(z["rowptr"], z["colidx"], z["src"], z["start"], side, cf, cu, mode="flood",
                               churn_threshold=cthr, churn_seed=7)
        hop, rounds = netsplit_ref.flood_packed(z["rowptr"], z["colidx"], z["src"], z["start"], side, cf, cu, cthr, 7)
        np.testing.assert_array_equal(hop, res.hop)
        assert len(rounds) == len(res.rounds)
        for a, b in zip(rounds, res.rounds):
            assert all(a[k] == b[k] for k in a), (a, b)


def test_link_cut_rule():
    assert not netsplit_ref.link_cut(2, 0, 1, 3, 5) and netsplit_ref.link_cut(3, 0, 1, 3, 5)
    assert netsplit_ref.link_cut(4, 0, 1, 3, 5) and not netsplit_ref.link_cut(5, 0, 1, 3, 5)
    assert not netsplit_ref.link_cut(4, 2, 2, 3, 5) and not netsplit_ref.link_cut(4, 0, 1, 5, 3)
