"""Anti-entropy on the CPU: tests/pull_ref.py (the numpy restatement the GPU tests compare the
engine with) is pinned bit for bit to the pull/ fixtures, which were produced by the reference's
own Node objects under the dedup app with a request queue (tests/golden/make_pull_golden.py);
without an exchange it is down_ref; the census holds from the data; a flood without churn only
gains by it; the wrong variant (the reply read after the partner's arrivals of the arrival round)
is told apart by the race item and by the hand case; and the library exports the entry points."""
import ctypes
import functools
import os

import numpy as np
import pytest

import down_ref
import pull_ref
from conftest import GOLDEN, golden_cases

PULL = os.path.join(GOLDEN, "pull")
PULL_CASES = ("pull_ba300_gossip_k2", "pull_ba300_gossip_k2_churn10", "pull_rrg200_flood", "pull_ws300_flood_churn10")


def load_pull(name):
    with np.load(os.path.join(PULL, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def cfg_of(z):
    return dict(mode=str(z["mode"]), fanout=int(z["fanout"]), gossip_seed=int(z["gossip_seed"]),
                churn_threshold=int(z["churn_threshold"]), churn_seed=int(z["churn_seed"]))


def setting_of(z):
    return tuple(int(x) for x in z["anti_entropy"])


@functools.lru_cache(maxsize=None)
def ref_of(name, late_gather=False):
    """pull_ref on a fixture's inputs (computed once, shared, never written to)."""
    z = load_pull(name)
    return pull_ref.run(z["rowptr"], z["colidx"], z["src"], z["start"], z["down_from"], z["down_until"],
                        anti_entropy=setting_of(z), pull_seed=int(z["pull_seed"]), late_gather=late_gather, **cfg_of(z))


@functools.lru_cache(maxsize=None)
def nopull_of(name):
    """The same case without anti-entropy, through down_ref (the yardstick loop)."""
    z = load_pull(name)
    return down_ref.run(z["rowptr"], z["colidx"], z["src"], z["start"], z["down_from"], z["down_until"], **cfg_of(z))


def test_the_four_pull_fixtures_are_there_and_stand_on_the_down_fixtures():
    assert tuple(sorted(f[:-4] for f in os.listdir(PULL) if f.endswith(".npz"))) == PULL_CASES
    # the parametrised tests over tests/golden/*.npz must not pick them up
    assert not [c for c in golden_cases() + golden_cases(dynamic=True) if c.startswith("pull")]
    asked = set()
    for name in PULL_CASES:
        z = load_pull(name)
        assert os.path.getsize(os.path.join(PULL, name + ".npz")) < 100_000
        with np.load(os.path.join(GOLDEN, "down", name.replace("pull_", "down_", 1) + ".npz"), allow_pickle=False) as d:
            for key in ("rowptr", "colidx", "src", "start", "down_from", "down_until", "mode", "fanout", "gossip_seed",
                        "churn_threshold", "churn_seed"):
                np.testing.assert_array_equal(z[key], d[key])
        period, first, last = setting_of(z)
        f, u = z["down_from"], z["down_until"]
        assert period in (1, 3, 4) and 1 <= first <= 3
        assert last == int(u[(f >= 0) & (u < pull_ref.FOREVER)].max()) + 3  # a few rounds after the last return
        assert z["exchanges"].shape == (len(range(first, last + 1, period)), 6)
        asked |= set(str(x) for x in z["census"])
    assert asked == set(pull_ref.CENSUS)


@pytest.mark.parametrize("name", PULL_CASES)
def test_pull_ref_equals_the_reference_nodes_bit_for_bit(name):
    z, res = load_pull(name), ref_of(name)
    np.testing.assert_array_equal(res.hop, z["hop"])
    np.testing.assert_array_equal(res.parent, z["parent"])
    assert pull_ref.pad_equal(res.column("relays"), z["round_relays"])
    assert int(res.column("relays").sum()) == int(z["round_relays"].sum()) == int(z["peer_sent"].sum())
    assert int(res.peer_recv.sum()) == int(z["total_recv"])
    np.testing.assert_array_equal(res.peer_sent, z["peer_sent"])
    np.testing.assert_array_equal(res.peer_recv, z["peer_recv"])
    np.testing.assert_array_equal(res.records(), z["exchanges"])
    np.testing.assert_array_equal(res.pull_sent, z["pull_sent"])
    np.testing.assert_array_equal(res.pull_recv, z["pull_recv"])
    # the records are consistent with themselves and with the per-peer pull counters
    x = z["exchanges"]
    assert (x[:, 3] == x[:, 1] - x[:, 2]).all(), "replies = requests that arrived"
    assert int(z["pull_sent"].sum()) == int(x[:, 1].sum() + x[:, 3].sum())
    assert int(z["pull_recv"].sum()) == int(x[:, 3].sum() + (x[:, 3] - x[:, 4]).sum())
    assert int(x[:, 5].sum()) == int(sum(p.sum() for p in res.pulled))


@pytest.mark.parametrize("name", PULL_CASES)
def test_the_engine_s_consequence_equals_the_literal_reply_list(name):
    """The engine never keeps a digest: it takes seen_p[end of r + 1] & ~seen_u[before the arrivals
    of r + 2].  pull_ref keeps the digest and the list; what a reply's unseen messages are must
    not depend on it: recomputed here from the hop plane alone."""
    z, res = load_pull(name), ref_of(name)
    hop = res.hop
    for a in range(2, len(res.rounds)):
        pp = res.partner[a]
        us = np.nonzero(pp >= 0)[0]
        if not len(us):
            assert not res.fresh[a].any()
            continue
        seen_p = (hop[pp[us]] >= 0) & (hop[pp[us]] <= a - 1)
        seen_u = (hop[us] >= 0) & (hop[us] <= a - 1)
        want = np.zeros_like(res.fresh[a])
        want[us] = seen_p & ~seen_u
        np.testing.assert_array_equal(res.fresh[a], want)


@pytest.mark.parametrize("name", PULL_CASES)
def test_without_an_exchange_it_is_down_ref(name):
    z = load_pull(name)
    for setting in (None, (0, 0, 0)):
        a = pull_ref.run(z["rowptr"], z["colidx"], z["src"], z["start"], z["down_from"], z["down_until"],
                         anti_entropy=setting, **cfg_of(z))
        b = nopull_of(name)
        np.testing.assert_array_equal(a.hop, b.hop)
        np.testing.assert_array_equal(a.parent, b.parent)
        assert a.rounds == b.rounds
        np.testing.assert_array_equal(a.peer_sent, b.peer_sent)
        np.testing.assert_array_equal(a.peer_recv, b.peer_recv)
        assert all(np.array_equal(x, y) for s, t in zip(a.sends, b.sends) for x, y in zip(s, t))
        assert a.exchanges == [] and not a.pull_sent.any() and not a.pull_recv.any()


@pytest.mark.parametrize("name", PULL_CASES)
def test_the_census_holds(name):
    z, res = load_pull(name), ref_of(name)
    churn = int(z["churn_threshold"]) != 0
    got = pull_ref.census(z, res, nopull_of(name))
    asked = [str(x) for x in z["census"]]
    assert set(asked) <= set(pull_ref.census_items(str(z["mode"]) == "gossip", churn))
    # every fixture is asked the whole census of its case; the one exemption is named (pull_ref.EXEMPT)
    assert set(pull_ref.EXEMPT) == {"pull_rrg200_flood"}
    missing = set(pull_ref.census_items(str(z["mode"]) == "gossip", churn)) - set(asked)
    assert missing == set(pull_ref.EXEMPT.get(name, ()))
    for item in asked:
        assert got[item], f"{name}: census item {item} is missing"


@pytest.mark.parametrize("name", [n for n in PULL_CASES if "race" not in pull_ref.EXEMPT.get(n, ())])
def test_the_race_item_tells_the_late_gather_apart(name):
    """With the reply read after the partner's own arrivals of the arrival round (the gather moved
    behind the receive pass, or the two passes merged) a requester gets bits a round early: the
    fixtures that hold the race item must differ."""
    good, bad = ref_of(name), ref_of(name, True)
    assert not np.array_equal(good.hop, bad.hop)
    assert int((bad.hop != good.hop).sum()) > 0


def test_in_a_flood_without_churn_anti_entropy_only_gains():
    z, res, no = load_pull("pull_rrg200_flood"), ref_of("pull_rrg200_flood"), nopull_of("pull_rrg200_flood")
    assert int(z["churn_threshold"]) == 0
    assert not ((no.hop >= 0) & (res.hop < 0)).any(), "the delivered set is a superset"
    both = no.hop >= 0
    assert (res.hop[both] <= no.hop[both]).all(), "and no hop is later"
    assert ((res.hop >= 0) & (no.hop < 0)).sum() > 0


def star_with_chains():
    """The hand case of the two-pass split (tests/test_gpu_pull.py runs it on the engine).

        3 - 1 - 0 - 2 - 4          peer 0 is the hub; 3 and 4 are leaves (deg 1: their partner is
                                   forced, whatever the seed), 1 and 2 have deg 2

    Message 0 starts at peer 3 in round 0 and floods: 1 has it in round 1, 0 in round 2, 2 in round
    3, 4 in round 4 -- each from its one neighbour towards 3.  Anti-entropy of period 1 in rounds
    1 .. 3.  Leaf 4 asks 2 in round 1; 2 answers in round 2, when it does not have the message, so
    the reply that arrives at 4 in round 3 is empty.  In that same round 3 the partner 2 gets the
    message by relay from 0.  4 must NOT get it in round 3: it gets it in round 4, from 2 (by 2's
    relay and by the reply to its request of round 2, both from sender 2).  A gather behind the
    receive pass, or one pass that reads 2's row while it is being written, hands 4 the message in
    round 3.  Nothing is repaired in any exchange: every pulled bit arrives by relay as well.
    Requests: 5 per exchange (every peer has a connection), none lost.
    """
    edges = [(0, 1), (0, 2), (1, 3), (2, 4)]
    V = 5
    adj = [[] for _ in range(V)]
    for a, b in edges:
        adj[a].append(b)
        adj[b].append(a)
    rowptr = np.cumsum([0] + [len(x) for x in adj]).astype(np.int64)
    colidx = np.array([y for x in adj for y in sorted(x)], dtype=np.int32)
    src = np.array([3], dtype=np.int32)
    start = np.array([0], dtype=np.int32)
    return rowptr, colidx, src, start, (1, 1, 3)


def test_the_hand_case_of_the_two_pass_split():
    """The hand case on the reference side only: pull_ref gives the hand-computed run and its wrong
    variant differs, so the case has teeth.  It runs none of the engine (the engine-side guard of the
    two-pass split is tests/test_gpu_pull.py's run of the same case)."""
    rowptr, colidx, src, start, setting = star_with_chains()
    for seed in (0, 1, 2, 3):  # (the leaves' partners are forced; the others' draws do not matter)
        assert pull_ref.partners(1, rowptr, colidx, seed)[4] == 2 and pull_ref.partners(2, rowptr, colidx, seed)[3] == 1
        res = pull_ref.run(rowptr, colidx, src, start, anti_entropy=setting, pull_seed=seed)
        assert res.hop[:, 0].tolist() == [2, 1, 3, 0, 4]
        assert res.parent[:, 0].tolist() == [1, 3, 0, -1, 2]
        assert res.records().tolist() == [[1, 5, 0, 5, 0, 0], [2, 5, 0, 5, 0, 0], [3, 5, 0, 5, 0, 0]]
        assert len(res.rounds) == 6  # the exchange of round 3 completes in round 5
        # the wrong variant hands the message to 4 in round 3 already
        bad = pull_ref.run(rowptr, colidx, src, start, anti_entropy=setting, pull_seed=seed, late_gather=True)
        assert bad.hop[2, 0] == 3 and bad.hop[4, 0] == 3


def test_library_exports_the_anti_entropy_entry_points():
    from p2pnetwork.gpu import _lib
    L = _lib.lib()
    for name in ("p2pg_set_anti_entropy", "p2pg_pull_partner_slot", "p2pg_get_pull_stats"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    assert list(L.p2pg_set_anti_entropy.argtypes[1:]) == [ctypes.c_int32] * 3 + [ctypes.c_uint64]
    assert ctypes.sizeof(_lib.PullStatsC) == 48
    # no engine: rejected before any device is touched
    assert L.p2pg_set_anti_entropy(None, 0, 4, 1, 0) == -1
    assert b"set_anti_entropy" in L.p2pg_global_error()
    # the host export of the draw is pull_ref's
    for seed in (0, 0xBEEF, 0x123456789ABCDEF):
        for r, peer, deg in ((0, 0, 1), (3, 17, 4), (100, 299, 77), (2, 5, 1000), (7, 123456, 3)):
            assert L.p2pg_pull_partner_slot(r, peer, deg, seed) == int(pull_ref.partner_slot(r, peer, deg, seed))
    assert L.p2pg_pull_partner_slot(1, 1, 0, 0) == -1
