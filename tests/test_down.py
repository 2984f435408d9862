"""Peer downtime on the CPU: tests/down_ref.py (the numpy restatement the GPU tests compare the
engine with) is pinned bit for bit to the down/ fixtures, which were produced by the reference's
own Node objects under the dedup app with one more term in the harness's ``dropped(a, b)`` -- the
receiver is offline in the round the packet would arrive in (tests/golden/make_down_golden.py);
without an interval it is late_ref / drop_ref; the rounds before the first interval are the run
without a downtime; and the library exports the two entry points."""
import ctypes
import functools
import os

import numpy as np
import pytest

import down_ref
import drop_ref
import late_ref
import policy_ref
from conftest import GOLDEN, golden_cases

DOWN = os.path.join(GOLDEN, "down")
DOWN_CASES = ("down_ba300_gossip_k2", "down_ba300_gossip_k2_churn10", "down_rrg200_flood",
              "down_ws300_flood_churn10")
FOREVER = 0x7FFFFFFF


def load_down(name):
    with np.load(os.path.join(DOWN, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def cfg_of(z):
    return dict(mode=str(z["mode"]), fanout=int(z["fanout"]), gossip_seed=int(z["gossip_seed"]),
                churn_threshold=int(z["churn_threshold"]), churn_seed=int(z["churn_seed"]))


def rule_of(z):
    """The fixture's hop limits and relay policy as a drop_ref callback (none: nothing dropped)."""
    return policy_ref.with_ttl(policy_ref.policy_rule(z["thr"], int(z["policy_seed"]), z["start"]),
                               z["start"], z["ttl"])


@functools.lru_cache(maxsize=None)
def ref_of(name):
    """down_ref on a fixture's inputs (computed once, shared, never written to)."""
    z = load_down(name)
    return down_ref.run(z["rowptr"], z["colidx"], z["src"], z["start"], z["down_from"], z["down_until"],
                        drop=rule_of(z), **cfg_of(z))


@functools.lru_cache(maxsize=None)
def full_of(name):
    """The same case without a downtime, through drop_ref (the yardstick loop)."""
    z = load_down(name)
    c = cfg_of(z)
    return drop_ref.run(z["rowptr"], z["colidx"], z["src"], z["start"], rule_of(z), c["mode"], c["fanout"],
                        c["gossip_seed"], 0, c["churn_threshold"], c["churn_seed"])


def test_the_four_downtime_fixtures_are_there_and_hold_the_census():
    assert tuple(sorted(f[:-4] for f in os.listdir(DOWN) if f.endswith(".npz"))) == DOWN_CASES
    # the parametrised tests over tests/golden/*.npz must not pick them up
    assert not [c for c in golden_cases() + golden_cases(dynamic=True) if c.startswith("down")]
    with_policy = row_full = 0
    for name in DOWN_CASES:
        z = load_down(name)
        assert os.path.getsize(os.path.join(DOWN, name + ".npz")) < 100_000
        with np.load(os.path.join(GOLDEN, "late", name.replace("down_", "late_", 1) + ".npz"),
                     allow_pickle=False) as late:  # the late fixtures' graphs and schedules, nothing moved
            for key in ("rowptr", "colidx", "src", "start"):
                np.testing.assert_array_equal(z[key], late[key])
        f, u = z["down_from"], z["down_until"]
        V, M = z["hop"].shape
        assert f.dtype == np.int32 and u.dtype == np.int32 and f.shape == u.shape == (V,)
        assert ((f == -1) | ((f >= 0) & (u > f))).all()
        # a fifth of the peers, less the few whose own originations stand in the way, plus the placed outages
        assert V // 5 - 8 <= (f >= 0).sum() <= V // 5 + 8
        # no origination at an offline peer
        assert not any(down_ref.offline(int(s), f, u)[int(p)] for p, s in zip(z["src"], z["start"]))
        res, full = ref_of(name), full_of(name)
        got = down_ref.census(z, res, full)
        gossip = str(z["mode"]) == "gossip"
        fills = bool((full.hop >= 0).all(axis=1).any())  # does any row fill without the downtime?
        need = [x for x in down_ref.CENSUS if (x != "gossip_deg" or gossip) and (x != "row_full" or fills)]
        assert all(got[x] for x in need), (name, got)
        assert sorted(z["census"].tolist()) == sorted(need)
        row_full += got["row_full"]
        with_policy += bool((z["ttl"] >= 0).any() and z["thr"].any())
        # not degenerate: against the same case without a downtime
        assert (z["hop"] >= 0).sum() * 10 >= (full.hop >= 0).sum() * 9
        wide = ((z["hop"] >= 0).sum(axis=0) * 2 >= V).sum()
        wide_full = ((full.hop >= 0).sum(axis=0) * 2 >= V).sum()
        assert wide * 2 >= wide_full, (name, wide, wide_full)
        assert ((res.hop > full.hop) & (full.hop >= 0)).sum() >= 100  # receipts made later ...
        assert ((res.hop < 0) & (full.hop >= 0)).sum() >= 100         # ... and never
    assert with_policy == 1, "the flood on the 4-regular graph carries hop limits and a relay policy"
    assert row_full >= 2, "a flood and a gossip fixture hold a row that would have filled while offline"


@pytest.mark.parametrize("name", DOWN_CASES)
def test_down_ref_equals_the_reference_nodes(name):
    z = load_down(name)
    res = ref_of(name)
    np.testing.assert_array_equal(res.hop, z["hop"])
    np.testing.assert_array_equal(res.parent, z["parent"])
    assert late_ref.pad_equal(res.column("relays"), z["round_relays"])
    assert int(res.column("received").sum()) == int(z["total_recv"])
    np.testing.assert_array_equal(res.peer_sent, z["peer_sent"])
    np.testing.assert_array_equal(res.peer_recv, z["peer_recv"])
    f, u = z["down_from"], z["down_until"]
    for r, (snd, rcv, msg, lost) in enumerate(res.sends):
        assert len(snd) == res.rounds[r]["relays"]
        off_now, off_next = down_ref.offline(r, f, u), down_ref.offline(r + 1, f, u)
        assert not off_now[snd].any()          # an offline peer sends nothing
        assert lost[off_next[rcv]].all()       # what is addressed to an offline peer is lost
        assert not (z["hop"][off_now] == r).any()  # ... and it has no first receipt
        if r + 1 < len(res.rounds):
            assert int((~lost).sum()) == res.rounds[r + 1]["received"]


@pytest.mark.parametrize("name", DOWN_CASES)
def test_without_an_interval_down_ref_is_late_ref_and_drop_ref(name):
    z = load_down(name)
    c = cfg_of(z)
    V = len(z["rowptr"]) - 1
    args = (c["mode"], c["fanout"], c["gossip_seed"], 0, c["churn_threshold"], c["churn_seed"])
    for down in ((None, None), down_ref.no_downtime(V)):
        res = down_ref.run(z["rowptr"], z["colidx"], z["src"], z["start"], *down, **c)
        late = late_ref.run(z["rowptr"], z["colidx"], z["src"], z["start"], *args)
        np.testing.assert_array_equal(res.hop, late.hop)
        np.testing.assert_array_equal(res.parent, late.parent)
        np.testing.assert_array_equal(res.peer_sent, late.peer_sent)
        np.testing.assert_array_equal(res.peer_recv, late.peer_recv)
        assert res.rounds == late.rounds
    # ... and with the fixture's hop limits and policy, drop_ref, send lists included
    res = down_ref.run(z["rowptr"], z["colidx"], z["src"], z["start"], drop=rule_of(z), **c)
    full = full_of(name)
    np.testing.assert_array_equal(res.hop, full.hop)
    np.testing.assert_array_equal(res.parent, full.parent)
    assert res.rounds == full.rounds and res.relays_offered == full.relays_offered
    for a, b in zip(res.sends, full.sends):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("name", DOWN_CASES)
def test_rounds_before_the_first_interval_are_the_run_without_downtime(name):
    z = load_down(name)
    f, u = z["down_from"].copy(), z["down_until"].copy()
    # the fixtures hold late joiners (from 0): shift the whole schedule by three rounds where no
    # origination stands in the way, so that there is a prefix to compare
    shift = 3
    f = np.where(f >= 0, f + shift, f)
    u = np.where((z["down_from"] >= 0) & (u < FOREVER), u + shift, u)
    for m, (p, s) in enumerate(zip(z["src"], z["start"])):
        if down_ref.offline(int(s), f, u)[int(p)]:
            f[int(p)], u[int(p)] = -1, FOREVER
    first = int(f[f >= 0].min())
    assert first == shift
    res = down_ref.run(z["rowptr"], z["colidx"], z["src"], z["start"], f, u, drop=rule_of(z), **cfg_of(z))
    full = full_of(name)
    # a send of round first - 1 may already be lost (its receiver is offline in round first):
    # every field of every round before min(from) stands, the lost flags of the rounds before that
    assert res.rounds[:first] == full.rounds[:first]
    pre_r, pre_f = (res.hop >= 0) & (res.hop < first), (full.hop >= 0) & (full.hop < first)
    np.testing.assert_array_equal(pre_r, pre_f)
    np.testing.assert_array_equal(np.where(pre_r, res.hop, -1), np.where(pre_f, full.hop, -1))
    np.testing.assert_array_equal(np.where(pre_r, res.parent, -1), np.where(pre_f, full.parent, -1))
    for r in range(first - 1):
        for x, y in zip(res.sends[r], full.sends[r]):
            np.testing.assert_array_equal(x, y)
    for x, y in zip(res.sends[first - 1][:3], full.sends[first - 1][:3]):
        np.testing.assert_array_equal(x, y)
    assert res.rounds[first:] != full.rounds[first:]


def test_library_exports_the_downtime_entry_points():
    from p2pnetwork.gpu import _lib
    L = _lib.lib()
    for name in ("p2pg_set_downtime", "p2pg_peer_offline"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    assert L.p2pg_set_downtime.argtypes[1] is ctypes.c_int64
    assert L.p2pg_set_downtime.restype is ctypes.c_int
    assert list(L.p2pg_peer_offline.argtypes) == [ctypes.c_int32] * 3
    one = np.zeros(1, dtype=np.int32)
    # no engine: rejected before any device is touched
    assert L.p2pg_set_downtime(None, 1, _lib.ptr(one), _lib.ptr(one)) == -1
    assert b"set_downtime" in L.p2pg_global_error()


def test_peer_offline_at_the_edges_of_the_interval():
    from p2pnetwork.gpu import GraphNetwork, _lib
    L = _lib.lib()
    # [3, 5): offline in 3 and 4 only
    assert [L.p2pg_peer_offline(r, 3, 5) for r in (0, 2, 3, 4, 5, 6)] == [0, 0, 1, 1, 0, 0]
    # never
    assert not any(L.p2pg_peer_offline(r, -1, FOREVER) for r in (0, 1, FOREVER - 1))
    # a crash: from its round on, for good
    assert [L.p2pg_peer_offline(r, 7, FOREVER) for r in (6, 7, 1 << 30, FOREVER - 1)] == [0, 1, 1, 1]
    # a late joiner
    assert [L.p2pg_peer_offline(r, 0, 2) for r in (0, 1, 2)] == [1, 1, 0]
    # a one-round outage
    assert [L.p2pg_peer_offline(r, 9, 10) for r in (8, 9, 10)] == [0, 1, 0]
    rng = np.random.default_rng(3)
    f = rng.integers(-1, 20, 500)
    u = np.where(rng.random(500) < 0.2, FOREVER, f + rng.integers(1, 5, 500))
    for r in (0, 1, 5, 19, 23):
        got = [L.p2pg_peer_offline(r, int(a), int(b)) for a, b in zip(f, u)]
        np.testing.assert_array_equal(np.array(got, dtype=bool), down_ref.offline(r, f, u))
    assert GraphNetwork.peer_offline(4, 3, 5) and not GraphNetwork.peer_offline(5, 3, 5)
    assert GraphNetwork.peer_offline(1 << 30, 3, None) and GraphNetwork.peer_offline(1 << 30, 3, -1)
    assert not GraphNetwork.peer_offline(1 << 30, -1, None)


def test_graphnetwork_has_the_downtime_interface():
    import inspect
    from p2pnetwork.gpu import GraphNetwork
    sig = inspect.signature(GraphNetwork.set_downtime)
    assert list(sig.parameters)[1:] == ["offline_from", "offline_until"]
    assert sig.parameters["offline_until"].default is None
    assert isinstance(inspect.getattr_static(GraphNetwork, "peer_offline"), staticmethod)
    assert list(inspect.signature(GraphNetwork.peer_offline).parameters) == ["round", "offline_from", "offline_until"]
