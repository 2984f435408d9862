"""Peer downtime (p2pg_set_downtime) on the GPU: the engine, through the C-ABI, against the down/
fixtures of the reference's own Node objects and against tests/down_ref.py (pinned to those
fixtures on the CPU, tests/test_down.py) -- bit-exact hop, parent, delivered set, send lists with
their lost flags, tallies and every per-round counter the contract defines (touched_words and the
push form of an offline round are the engine's)."""
import functools
import zlib

import numpy as np
import pytest

import down_ref
import policy_ref
from test_down import DOWN_CASES, cfg_of, load_down, ref_of, rule_of
from test_gpu_late import FLOOD_KEYS, assert_planes, gpu_net

pytestmark = pytest.mark.gpu

CHURN = 430_000_000
FOREVER = down_ref.FOREVER
ATOMIC, EDGE, FUSED, UPDATE_EDGE = 1, 2, 3, 4  # p2pg_round_stats.push_form


def assert_rounds(rounds, ref, mode, no_scatter=(), inexact=(), check_active=True):
    """Every counter of every round (the engine may not stop earlier or later than the reference).
    no_scatter: rounds whose scatter_words another feature leaves to the engine (a held-back push);
    inexact: the rounds a downtime engine without count_received reports with received_exact = 0
    and the sends of the round before as `received`."""
    assert len(rounds) == len(ref.rounds), (len(rounds), len(ref.rounds))
    for i, (a, b) in enumerate(zip(rounds, ref.rounds)):
        assert a.round == i and a.received_exact == (0 if i in inexact else 1), (i, a.received_exact)
        for k in FLOOD_KEYS:
            want = b[k] if k != "received" or i not in inexact else (ref.rounds[i - 1]["relays"] if i else 0)
            assert getattr(a, k) == want, (i, k, getattr(a, k), want)
        if mode == "gossip" and i not in no_scatter:
            assert a.scatter_words == b["scatter_words"], (i, a.scatter_words, b["scatter_words"])
        ahead = any(r["new_deliveries"] for r in ref.rounds[i + 1:])
        if check_active:
            assert a.active == (1 if b["new_deliveries"] or ahead else 0), (i, a.active)


def assert_tallies(net, ref):
    got = ref.hop >= 0
    t = net.message_tally()
    np.testing.assert_array_equal(t.reach, got.sum(axis=0))
    np.testing.assert_array_equal(t.hop_sum, np.where(got, ref.hop, 0).sum(axis=0))
    np.testing.assert_array_equal(t.last_hop, ref.hop.max(axis=0))
    c = net.peer_counters()
    np.testing.assert_array_equal(c.sent, ref.peer_sent)
    np.testing.assert_array_equal(c.received, ref.peer_recv)
    np.testing.assert_array_equal(net.message_reach(), got.sum(axis=0))


def assert_sends(net, ref, r):
    s = net.sends()
    snd, rcv, msg, lost = ref.sends[r]
    np.testing.assert_array_equal(s.sender, snd)
    np.testing.assert_array_equal(s.receiver, rcv)
    np.testing.assert_array_equal(s.msg, msg)
    np.testing.assert_array_equal(s.lost, lost)


def offline_rounds(f, u, n):
    return {r for r in range(n) if down_ref.offline(r, f, u).any()}


def intervals(V, seed, src, start, last=8):
    """A fifth of the peers with an interval of every kind -- a crash, a late joiner, a one-round
    and a multi-round outage first, then drawn -- none holding one of the peer's own originations."""
    rng = np.random.default_rng(seed)
    f = np.full(V, -1, dtype=np.int32)
    u = np.full(V, FOREVER, dtype=np.int32)
    own = {}
    for p, s in zip(np.asarray(src).tolist(), np.asarray(start).tolist()):
        own.setdefault(p, []).append(s)
    kinds = [(2, FOREVER), (0, 2), (1, 2), (2, 5)]
    for i, v in enumerate(rng.permutation(V)[:max(V // 5, 5)].tolist()):
        for _ in range(32):
            if i < len(kinds):
                a, b = kinds[i]
            else:
                kind = rng.integers(0, 10)
                a = 0 if kind == 0 else int(rng.integers(1, last))
                b = FOREVER if kind == 1 else a + int(rng.integers(1, 4))
            if not any(a <= s < b for s in own.get(v, [])):
                f[v], u[v] = a, b
                break
            i = len(kinds)  # (a fixed kind that does not fit this peer: draw instead)
    return f, u


def windows(V, seed, src, start, spans):
    """A fifth of the peers, dealt over the intervals `spans` in turn (none holding one of the
    peer's own originations): offline rounds with rounds in between in which nobody is offline."""
    f = np.full(V, -1, dtype=np.int32)
    u = np.full(V, FOREVER, dtype=np.int32)
    own = {}
    for p, s in zip(np.asarray(src).tolist(), np.asarray(start).tolist()):
        own.setdefault(p, []).append(s)
    for i, v in enumerate(np.random.default_rng(seed).permutation(V)[:V // 5].tolist()):
        a, b = spans[i % len(spans)]
        if not any(a <= s < b for s in own.get(v, [])):
            f[v], u[v] = a, b
    return f, u


def not_vacuous(ref, f, u):
    """Somebody's receipt was lost to the downtime and made later, and somebody was sent to while
    offline."""
    hit = later = False
    for r, (snd, rcv, msg, lost) in enumerate(ref.sends):
        off = down_ref.offline(r + 1, f, u)[rcv]
        hit |= bool(off.any())
        later |= bool((ref.hop[rcv[off], msg[off]] > r + 1).any())
    return hit and later


# ---- 1. the four fixtures of the reference's own Node objects -----------------------------------
@pytest.mark.parametrize("name", DOWN_CASES)
def test_down_fixture_through_the_c_abi(name):
    z = load_down(name)
    mode = str(z["mode"])
    cfg = (mode, int(z["fanout"]), int(z["gossip_seed"]), int(z["churn_threshold"]), int(z["churn_seed"]))
    ref = ref_of(name)
    policy = bool(z["thr"].any())
    with gpu_net(z, *cfg, record=True, tally=True) as net:
        net.broadcast(z["src"], z["start"], ttl=z["ttl"])
        if policy:
            net.set_relay_policy(thresholds=z["thr"], seed=int(z["policy_seed"]))
        net.set_downtime(z["down_from"], z["down_until"])
        np.testing.assert_array_equal(net.offline_from, z["down_from"])
        rounds = net.run()
        hop, parent = net.hop_parent()
        np.testing.assert_array_equal(hop, z["hop"])
        np.testing.assert_array_equal(parent, z["parent"])
        np.testing.assert_array_equal(net.delivered(), z["hop"] >= 0)
        assert down_ref.pad_equal([r.relays for r in rounds], z["round_relays"])
        assert net.message_count_send == int(z["round_relays"].sum())
        assert sum(r.received for r in rounds) == int(z["total_recv"])
        # (with a policy every round after round 0 holds its push back: scatter_words is the engine's)
        assert_rounds(rounds, ref, mode, no_scatter=set(range(1, len(rounds))) if policy else ())
        assert_planes(net, ref)
        assert_tallies(net, ref)
        c = net.peer_counters()
        np.testing.assert_array_equal(c.sent, z["peer_sent"])
        np.testing.assert_array_equal(c.received, z["peer_recv"])
        # the send lists of every round with their lost flags, stepping the replay
        net.reset()
        for r in range(len(ref.rounds)):
            st = net.step()
            assert st.relays == ref.rounds[r]["relays"]
            assert_sends(net, ref, r)
        assert not st.active


# ---- 2. flood sweep against down_ref --------------------------------------------------------------
FLOOD_CASES = [(V, M, thr) for V in (33, 200) for M in (1, 63, 64, 65, 130) for thr in (0, CHURN)]
FLOOD_CASES += [(40, 4160, 0), (40, 4160, CHURN)]


def place_row_fill(g, src, start, f, u, kw):
    """A peer without an interval goes offline in exactly the round its row would fill, and ends
    with the receipt it makes later: the first candidate for which that holds (f, u are updated)."""
    base = down_ref.run(g.rowptr, g.colidx, src, start, f, u, **kw)
    full = np.nonzero((base.hop >= 0).all(axis=1) & (f < 0))[0]
    for v in full.tolist():
        r = int(base.hop[v].max())
        if r == 0 or ((np.asarray(src) == v) & (np.asarray(start) == r)).any():
            continue
        f2, u2 = f.copy(), u.copy()
        f2[v], u2[v] = r, r + 1
        ref = down_ref.run(g.rowptr, g.colidx, src, start, f2, u2, **kw)
        if (ref.hop[v] >= 0).all() and ref.hop[v].max() > r:
            f[:], u[:] = f2, u2
            return ref, v, r
    return None


@pytest.mark.parametrize("V,M,cthr", FLOOD_CASES)
def test_down_flood_matches_down_ref(V, M, cthr):
    from p2pnetwork.gpu import PeerGraph, make_sources
    seed = zlib.crc32(repr((V, M, cthr)).encode()) & 0xFFFF
    # (the saturation cases on the connected graph: a row fills only where every message arrives)
    regular = (V + M) % 2 == 1 or M in (1, 64)
    g = PeerGraph.random_regular(V, 4, seed) if regular else PeerGraph.gnp(V, 5.0, seed)
    rng = np.random.default_rng(seed)
    src = make_sources(g.V, M, seed=seed).astype(np.int32)
    start = rng.integers(0, 4, M).astype(np.int32)
    start[0] = 0 if M > 1 else 1
    f, u = intervals(g.V, seed, src, start)
    kw = dict(mode="flood", fanout=3, gossip_seed=seed + 1, churn_threshold=cthr, churn_seed=seed + 2)
    if M in (1, 64):  # saturation: the row fills (S bit) in a round the peer is offline in
        # (a flood sends a message once per connection: the late receipt needs a neighbour that
        # gets it later still, which not every schedule has -- the first of a few that does)
        for j in range(16):
            f, u = intervals(g.V, seed + j, src, start)
            placed = place_row_fill(g, src, start, f, u, kw)
            if placed:
                break
        ref, v, r = placed
        assert f[v] == r and u[v] == r + 1 and (ref.hop[v] >= 0).all() and ref.hop[v].max() > r
    else:
        ref = down_ref.run(g.rowptr, g.colidx, src, start, f, u, **kw)
    assert not_vacuous(ref, f, u)
    with gpu_net(g, "flood", 3, seed + 1, cthr, seed + 2, tally=True) as net:
        net.broadcast(src, start)
        net.set_downtime(f, u)
        rounds = net.run()
        assert_rounds(rounds, ref, "flood")
        assert_planes(net, ref)
        assert_tallies(net, ref)
    for r in offline_rounds(f, u, len(rounds)):
        assert not (ref.hop[down_ref.offline(r, f, u)] == r).any()


# ---- 3. gossip sweep: row widths x push forms -------------------------------------------------------
def gossip_case(W):
    """Every message from one of 20 origins (test_gpu_policy.gossip_case): a sparse start, then
    rounds in which every peer takes first receipts in most words; a fifth of the peers join late
    or have a one-round or a three-round outage, with rounds in between in which nobody is offline
    (round 2, an origination round, and rounds 4 and 5)."""
    from p2pnetwork.gpu import PeerGraph, make_sources
    g = PeerGraph.barabasi_albert(600 if W <= 17 else 160, 4, seed=40 + W)
    M = 64 * W - 5
    src = (make_sources(20, M, seed=W) * 7 + 3).astype(np.int32)
    start = np.zeros(M, dtype=np.int32)
    start[np.random.default_rng(W).integers(0, M, max(M // 8, 1))] = 2
    f, u = windows(g.V, 100 + W, src, start, [(0, 2), (3, 4), (6, 9)])
    return g, src, start, f, u


@functools.lru_cache(maxsize=None)
def gossip_ref(W):
    g, src, start, f, u = gossip_case(W)
    return down_ref.run(g.rowptr, g.colidx, src, start, f, u, mode="gossip", fanout=3, gossip_seed=11,
                        churn_threshold=0, churn_seed=5)


@pytest.mark.parametrize("W", [1, 3, 8, 9, 16, 17, 32, 64, 65])
@pytest.mark.parametrize("push", ["atomic", "store", "auto"])
def test_down_gossip_push_forms(W, push, monkeypatch):
    """Whole-row E (W <= 8), packed E with AW masks (8 < W <= 64), the grouped kernels' widths, the
    64-lane edge, two slices; offline rounds after an E round, after a sparse round and in the
    first dense round."""
    if push != "auto":
        monkeypatch.setenv("P2PG_GOSSIP_PUSH", push)
    else:  # the thresholds test_late_gossip_push_forms sets: small graphs enter dense rounds
        monkeypatch.setenv("P2PG_E_THRESH", "0.05")
        monkeypatch.setenv("P2PG_V_THRESH", "0.3")
        monkeypatch.setenv("P2PG_UPDATE_PUSH", "1")
    g, src, start, f, u = gossip_case(W)
    ref = gossip_ref(W)
    assert not_vacuous(ref, f, u)
    with gpu_net(g, "gossip", 3, 11, 0, 5, tally=True) as net:
        net.broadcast(src, start)
        net.set_downtime(f, u)
        rounds = net.run()
        assert_rounds(rounds, ref, "gossip")
        assert_planes(net, ref)
        assert_tallies(net, ref)
    off = offline_rounds(f, u, len(rounds))
    forms = [x.push_form for x in rounds]
    assert off == {0, 1, 3, 6, 7, 8} and len(rounds) > 11, (sorted(off), len(rounds))
    assert all(forms[r] in (ATOMIC, EDGE) for r in off), forms
    if push == "atomic":
        assert set(forms) == {ATOMIC}
    elif push == "store":  # fused wherever nobody is offline and nothing originates
        assert all(forms[r] == EDGE for r in off | {0, 2}), forms
        if W <= 64:  # (two-slice rows have no fused round)
            assert all(forms[r] == FUSED for r in range(1, len(rounds)) if r not in off | {2}), forms
    # without records, tallies or the lost count: the same receipts and relays
    with gpu_net(g, "gossip", 3, 11, 0, 5, record=False, count_received=False) as net:
        net.broadcast(src, start)
        net.set_downtime(f, u)
        lean = net.run()
        np.testing.assert_array_equal(net.delivered(), ref.hop >= 0)
    assert [(x.new_deliveries, x.relays) for x in lean] == [(x.new_deliveries, x.relays) for x in rounds]


# ---- 4. the dense phase -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense_graph():
    from p2pnetwork.gpu import PeerGraph, make_sources
    g = PeerGraph.barabasi_albert(2000, 4, seed=3)
    return g, make_sources(g.V, 4096, seed=3)


def dense_run(f=None, u=None, call=True):
    g, src = dense_graph()
    with gpu_net(g, "gossip", 3, 0x5EED, record=False, count_received=False) as net:
        net.broadcast(src)
        if call:
            net.set_downtime(f, u)
        rounds = net.run()
        return rounds, net.seen_plane()


@functools.lru_cache(maxsize=None)
def dense_base():
    return dense_run(call=False)


def test_down_window_inside_the_fused_rounds():
    g, src = dense_graph()
    base, _ = dense_base()
    fused = [r.round for r in base if r.push_form == FUSED]
    assert len(fused) >= 4, [r.push_form for r in base]
    w0 = fused[1]  # a two-round window inside the fused rounds, fused rounds on both sides
    assert w0 + 1 in fused and w0 + 2 in fused
    f = np.full(g.V, -1, dtype=np.int32)
    u = np.full(g.V, FOREVER, dtype=np.int32)
    # (every broadcast starts in round 0 and the window lies after it: any peer may be in it)
    down = np.random.default_rng(4).permutation(g.V)[:g.V // 10]
    f[down], u[down] = w0, w0 + 2
    rounds, seen = dense_run(f, u)
    # every field of every round before the window, push_form included
    assert rounds[:w0] == base[:w0]
    assert all(rounds[r].push_form in (ATOMIC, EDGE) for r in (w0, w0 + 1)), [x.push_form for x in rounds]
    assert any(x.push_form == FUSED for x in rounds[w0 + 2:]), [x.push_form for x in rounds]
    ref = down_ref.run(g.rowptr, g.colidx, src, np.zeros(len(src), dtype=np.int32), f, u, mode="gossip", fanout=3,
                       gossip_seed=0x5EED)
    assert_rounds(rounds, ref, "gossip", inexact={w0, w0 + 1})
    bits = np.unpackbits(seen.view(np.uint8).reshape(g.V, -1), axis=1, bitorder="little")[:, :len(src)]
    np.testing.assert_array_equal(bits.astype(bool), ref.hop >= 0)
    assert ((ref.hop > w0 + 1) & down_ref.offline(w0, f, u)[:, None]).any()  # caught up after the window


# ---- 7. removal -------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["none", "all_minus_one"])
def test_removed_downtime_is_an_engine_that_never_saw_the_call(how):
    g, src = dense_graph()
    base, seen0 = dense_base()
    f = np.full(g.V, -1, dtype=np.int32)
    u = np.full(g.V, FOREVER, dtype=np.int32)
    f[5], u[5] = 3, 6
    with gpu_net(g, "gossip", 3, 0x5EED, record=False, count_received=False) as net:
        net.broadcast(src)
        net.set_downtime(f, u)
        if how == "none":
            net.set_downtime(None)
        else:
            net.set_downtime(np.full(g.V, -1, dtype=np.int32), np.zeros(g.V, dtype=np.int32))
        assert net.offline_from is None
        rounds = net.run()
        assert rounds == base  # every field of every round, push_form included
        np.testing.assert_array_equal(net.seen_plane(), seen0)
        assert len(net.snapshot()) > 0  # (and snapshots work again)


# ---- 5. a hub row -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["flood", "gossip"])
@pytest.mark.parametrize("who", ["hub", "neighbours"])
def test_down_hub_row_under_churn(mode, who):
    """test_gpu_drop's hub graph (peer 0 with 701 connections, above the hub threshold of the pull
    and push passes): the hub offline for a window, and its neighbours offline while it relays."""
    from test_gpu_drop import case_of
    g, M, src = case_of("hub", 70)
    start = np.random.default_rng(9).integers(0, 3, M).astype(np.int32)
    start[src == 0] = 0
    f = np.full(g.V, -1, dtype=np.int32)
    u = np.full(g.V, FOREVER, dtype=np.int32)
    if who == "hub":
        f[0], u[0] = 1, 4
    else:
        nb = np.arange(1, 702)
        nb = nb[~np.isin(nb, src)]
        f[nb[::2]], u[nb[::2]] = 1, 3
        f[nb[1::7]], u[nb[1::7]] = 2, FOREVER
    ref = down_ref.run(g.rowptr, g.colidx, src, start, f, u, mode=mode, fanout=3, gossip_seed=11,
                       churn_threshold=CHURN, churn_seed=6)
    if who == "hub":  # sends to the hub are lost while it is away, and it catches up afterwards
        assert all(((rcv == 0) & lost).any() for _, rcv, _, lost in ref.sends[0:3])
        assert (ref.hop[0] >= 4).any() and not ((ref.hop[0] >= 1) & (ref.hop[0] < 4)).any()
    else:
        assert any((snd == 0).any() and lost[snd == 0].any() for snd, _, _, lost in ref.sends[:3])
    with gpu_net(g, mode, 3, 11, CHURN, 6, tally=True) as net:
        net.broadcast(src, start)
        net.set_downtime(f, u)
        rounds = []
        for r in range(len(ref.rounds)):
            rounds.append(net.step())
            if r < 5:
                assert_sends(net, ref, r)
        assert_rounds(rounds, ref, mode)
        assert_planes(net, ref)
        assert_tallies(net, ref)


# ---- 6. across other calls ----------------------------------------------------------------------------
def small_case(mode, seed, M=130):
    from p2pnetwork.gpu import PeerGraph, make_sources
    g = PeerGraph.random_regular(300, 4, seed) if mode == "flood" else PeerGraph.barabasi_albert(400, 3, seed)
    src = make_sources(g.V, M, seed=seed).astype(np.int32)
    start = np.random.default_rng(seed).integers(0, 4, M).astype(np.int32)
    f, u = intervals(g.V, seed, src, start)
    return g, src, start, f, u


@pytest.mark.parametrize("mode", ["flood", "gossip"])
def test_down_update_edges_at_a_boundary_inside_a_window(mode):
    g, src, start, f, u = small_case(mode, 14)
    # after round 2 (peers are offline in rounds 2 and 3): a connection of an offline peer and one
    # between online peers are removed, an offline peer gains one
    off = np.nonzero(down_ref.offline(2, f, u) & down_ref.offline(3, f, u))[0]
    on = np.nonzero(f < 0)[0]
    a = int(off[0])
    b = int(g.neighbours(a)[0])
    c = next(int(x) for x in on if x != a and x not in set(g.neighbours(a).tolist()))
    d = int(on[10])
    updates = {2: (np.array([(a, c)], np.int32), np.array([(a, b), (d, int(g.neighbours(d)[1]))], np.int32))}
    ref = down_ref.run(g.rowptr, g.colidx, src, start, f, u, mode=mode, fanout=2, gossip_seed=41,
                       churn_threshold=CHURN, churn_seed=3, updates=updates)
    with gpu_net(g, mode, 2, 41, CHURN, 3, tally=True) as net:
        net.broadcast(src, start)
        net.set_downtime(f, u)
        rounds = [net.step() for _ in range(3)]
        net.update_edges(add=updates[2][0], remove=updates[2][1])
        while rounds[-1].active:
            rounds.append(net.step())
        assert_rounds(rounds, ref, mode)
        assert_planes(net, ref)
        assert_tallies(net, ref)


@pytest.mark.parametrize("mode", ["flood", "gossip"])
def test_down_drop_relays_in_an_offline_round(mode):
    g, src, start, f, u = small_case(mode, 15)
    kw = dict(mode=mode, fanout=3, gossip_seed=51, churn_threshold=0, churn_seed=0)
    plain = down_ref.run(g.rowptr, g.colidx, src, start, f, u, **kw)
    R = 3
    assert down_ref.offline(R, f, u).any()
    vs, ms = np.nonzero(plain.hop == R)
    pick = slice(0, len(vs), 3)  # a third of round 3's first receipts do not forward

    def rule(r, new):
        gone = np.zeros_like(new)
        if r == R:
            gone[vs[pick], ms[pick]] = True
        return gone
    ref = down_ref.run(g.rowptr, g.colidx, src, start, f, u, drop=rule, **kw)
    with gpu_net(g, mode, 3, 51, tally=True) as net:
        net.broadcast(src, start)
        net.set_downtime(f, u)
        rounds = [net.step() for _ in range(R + 1)]
        assert rounds[R].relays == ref.relays_offered[R]
        d = net.deliveries()
        assert not down_ref.offline(R, f, u)[d.peer].any()  # no delivery at an offline peer
        np.testing.assert_array_equal(np.stack([d.peer, d.msg]), np.stack([vs, ms]))
        net.drop_relays(vs[pick], ms[pick])
        assert net.message_count_send == sum(x["relays"] for x in ref.rounds[:R + 1])
        assert_sends(net, ref, R)
        while rounds[-1].active:
            rounds.append(net.step())
        for a, b in zip(rounds[R + 1:], ref.rounds[R + 1:]):
            for k in FLOOD_KEYS:
                assert getattr(a, k) == b[k], (a.round, k)
        assert_planes(net, ref)
        assert_tallies(net, ref)


@pytest.mark.parametrize("mode", ["flood", "gossip"])
def test_down_originate_mid_run(mode):
    from p2pnetwork.gpu import P2PGError
    g, src, start, f, u = small_case(mode, 16)
    src[[127, 128, 129]] = -1
    start[[127, 128, 129]] = -1
    off4 = np.nonzero(down_ref.offline(4, f, u) & (u < FOREVER))[0]  # offline in 4, and back later
    on4 = np.nonzero(~down_ref.offline(4, f, u) & (f >= 0) & (f > 4))[0]  # online in 4, offline later
    assert len(off4) and len(on4)
    with gpu_net(g, mode, 2, 31, CHURN, 8, tally=True) as net:
        net.broadcast(src, start)
        net.set_downtime(f, u)
        rounds = [net.step() for _ in range(3)]
        before = (net.sources.copy(), net.start_rounds.copy())
        with pytest.raises(P2PGError, match="bad argument"):
            net.originate([127, 128], [int(on4[0]), int(off4[0])], round=4)  # one offline origin rejects the call
        np.testing.assert_array_equal(net.sources, before[0])
        np.testing.assert_array_equal(net.start_rounds, before[1])
        net.originate([127, 128], [int(on4[0]), int(on4[0])], round=4)
        net.originate([129], [int(off4[0])], round=int(u[off4[0]]))  # ... in the round it returns
        ref = down_ref.run(g.rowptr, g.colidx, net.sources, net.start_rounds, f, u, mode=mode, fanout=2,
                           gossip_seed=31, churn_threshold=CHURN, churn_seed=8)
        while rounds[-1].active:
            rounds.append(net.step())
        assert_rounds(rounds, ref, mode, check_active=False)
        assert_planes(net, ref)
        assert_tallies(net, ref)


@pytest.mark.parametrize("mode", ["flood", "gossip"])
def test_down_with_hop_limits_and_a_relay_policy_run_stepping_and_reset(mode):
    g, src, start, f, u = small_case(mode, 17)
    M = len(src)
    ttl = np.array([2, 3, 5, -1, -1], dtype=np.int32)[np.random.default_rng(18).integers(0, 5, M)]
    thr = np.array([0, 0xFFFFFFFF, 1 << 31, 0], dtype=np.uint32)[np.random.default_rng(19).integers(0, 4, g.V)]
    rule = policy_ref.with_ttl(policy_ref.policy_rule(thr, 77, start), start, ttl)
    ref = down_ref.run(g.rowptr, g.colidx, src, start, f, u, drop=rule, mode=mode, fanout=3, gossip_seed=61,
                       churn_threshold=CHURN, churn_seed=9)
    assert not_vacuous(ref, f, u) and any(x.any() for x in ref.dropped)
    held = set(range(1, len(ref.rounds)))  # (a policy holds every round's push back)
    with gpu_net(g, mode, 3, 61, CHURN, 9, tally=True) as net:
        net.broadcast(src, start, ttl=ttl)
        net.set_relay_policy(thresholds=thr, seed=77)
        net.set_downtime(f, u)
        rounds = net.run()
        assert_rounds(rounds, ref, mode, no_scatter=held)
        assert_planes(net, ref)
        assert_tallies(net, ref)
        for _ in range(2):  # reset keeps the downtime and replays bit-identically
            net.reset()
            again = net.run()
            assert again == rounds
            assert_planes(net, ref)
        net.reset()
        stepped = []
        while True:
            stepped.append(net.step())
            if not stepped[-1].active:
                break
        assert_rounds(stepped, ref, mode, no_scatter=held)
        assert [(x.new_deliveries, x.relays, x.received) for x in stepped] == \
               [(x.new_deliveries, x.relays, x.received) for x in rounds]
        assert_planes(net, ref)
        assert_tallies(net, ref)


@pytest.mark.parametrize("mode", ["flood", "gossip"])
def test_down_run_equals_stepping_without_the_lost_count(mode):
    g, src, start, f, u = small_case(mode, 20)
    ref = down_ref.run(g.rowptr, g.colidx, src, start, f, u, mode=mode, fanout=3, gossip_seed=71)
    span = set(range(int(f[f >= 0].min()), min(int(u[f >= 0].max()), 1 << 20)))
    with gpu_net(g, mode, 3, 71, record=True, count_received=False) as net:
        net.broadcast(src, start)
        net.set_downtime(f, u)
        rounds = net.run()
        assert_rounds(rounds, ref, mode, inexact=span)
        assert_planes(net, ref)
        net.reset()
        stepped = [net.step() for _ in rounds]
        assert stepped == rounds


# ---- 8. refusals and received_exact -------------------------------------------------------------------
def test_received_exact_is_zero_exactly_in_the_span_of_the_intervals():
    from p2pnetwork.gpu import PeerGraph, make_sources
    g = PeerGraph.random_regular(200, 4, seed=21)
    src = make_sources(g.V, 70, seed=21).astype(np.int32)
    start = np.zeros(70, dtype=np.int32)
    f = np.full(g.V, -1, dtype=np.int32)
    u = np.full(g.V, FOREVER, dtype=np.int32)
    quiet = [v for v in range(g.V) if v not in set(src.tolist())]
    f[quiet[:10]], u[quiet[:10]] = 2, 3     # min(from) = 2
    f[quiet[10:20]], u[quiet[10:20]] = 5, 7  # max(until) = 7; nobody is offline in rounds 3 and 4
    ref = down_ref.run(g.rowptr, g.colidx, src, start, f, u, mode="flood")
    assert len(ref.rounds) > 8
    with gpu_net(g, "flood", count_received=False) as net:
        net.broadcast(src, start)
        net.set_downtime(f, u)
        rounds = net.run()
        assert [r.received_exact for r in rounds] == [0 if 2 <= r.round < 7 else 1 for r in rounds]
        assert_rounds(rounds, ref, "flood", inexact={2, 3, 4, 5, 6})
        assert rounds[2].received > ref.rounds[2]["received"]  # an upper bound, and not the exact count
    with gpu_net(g, "flood", count_received=True) as net:  # ... exact with the flag, churn or not
        net.broadcast(src, start)
        net.set_downtime(f, u)
        assert_rounds(net.run(), ref, "flood")


def test_down_refusals_leave_the_engine_unchanged():
    from p2pnetwork.gpu import P2PGError, PeerGraph, _lib
    L = _lib.lib()
    g = PeerGraph.random_regular(200, 4, seed=22)
    V = g.V
    src = np.array([1, 2, 7, -1], dtype=np.int32)
    start = np.array([0, 4, 6, -1], dtype=np.int32)
    f = np.full(V, -1, dtype=np.int32)
    u = np.full(V, FOREVER, dtype=np.int32)
    f[[10, 11, 12, 13]] = (0, 2, 3, 5)
    u[[10, 11, 12, 13]] = (3, 3, 6, FOREVER)
    ref = down_ref.run(g.rowptr, g.colidx, src, start, f, u, mode="flood")

    def ptr(a):
        return _lib.ptr(np.ascontiguousarray(a, dtype=np.int32))

    with gpu_net(g, "flood", tally=True) as net:
        net.set_downtime(f, u)  # before any sources: the downtime belongs to the peers
        # rule 3, this order: the sources are checked against the downtime
        for bad_src, bad_start in (([10], [0]), ([1, 12], [0, 5]), ([13, 1], [1 << 20, 0])):
            with pytest.raises(P2PGError, match="bad argument"):
                net.broadcast(bad_src, bad_start)
        with pytest.raises(P2PGError, match="bad argument"):
            net.broadcast([10])  # p2pg_set_sources: round 0, peer 10 joins late
        net.broadcast([10, 12, 13], [3, 2, 4])  # the edges of the intervals are online
        net.broadcast(src, start)
        # argument errors
        bad = f.copy()
        bad[20] = -2
        with pytest.raises(P2PGError, match="bad argument"):
            net.set_downtime(bad, u)
        for a, b in ((4, 4), (4, 3), (0, 0)):
            bad, bu = f.copy(), u.copy()
            bad[20], bu[20] = a, b
            with pytest.raises(P2PGError, match="bad argument"):
                net.set_downtime(bad, bu)
        assert L.p2pg_set_downtime(net._h, V - 1, ptr(f[:-1]), ptr(u[:-1])) == -1
        assert L.p2pg_set_downtime(net._h, V + 1, ptr(np.append(f, -1)), ptr(np.append(u, 0))) == -1
        assert L.p2pg_set_downtime(net._h, V, ptr(f), None) == -1
        with pytest.raises(ValueError):
            net.set_downtime(f[:-1], u[:-1])
        # rule 3, the other order: the downtime is checked against the schedule
        bad, bu = f.copy(), u.copy()
        bad[2], bu[2] = 4, 5  # message 1 starts at peer 2 in round 4
        with pytest.raises(P2PGError, match="bad argument"):
            net.set_downtime(bad, bu)
        bad[2], bu[2] = 5, 6
        net.set_downtime(bad, bu)  # the round after is fine
        net.set_downtime(f, u)
        # snapshots do not hold a downtime
        with pytest.raises(P2PGError, match="bad state"):
            net.snapshot()
        with pytest.raises(P2PGError, match="bad state"):
            net.restore(np.zeros(256, dtype=np.uint8))
        # between step_begin and step_end, and once a round has run
        net.step_begin()
        with pytest.raises(P2PGError, match="bad state"):
            net.set_downtime(f, u)
        with pytest.raises(P2PGError, match="bad state"):
            net.set_downtime(None)
        r0 = net.step_end()
        assert r0.round == 0
        with pytest.raises(P2PGError, match="bad state"):
            net.set_downtime(f, u)
        with pytest.raises(P2PGError, match="bad state"):
            net.set_downtime(None)
        net.step()
        # p2pg_originate at an offline peer
        with pytest.raises(P2PGError, match="bad argument"):
            net.originate([3], [13], round=5)
        with pytest.raises(P2PGError, match="bad argument"):
            net.originate([3], [12], round=3)
        np.testing.assert_array_equal(net.start_rounds, start)
        rounds = net.rounds[:]
        while rounds[-1].active:
            rounds.append(net.step())
        assert_rounds(rounds, ref, "flood")
        assert_planes(net, ref)
        # allowed again after a reset; the run replays
        net.reset()
        net.set_downtime(f, u)
        again = net.run()
        assert_rounds(again, ref, "flood")
    # a vertex-partitioned rank
    with gpu_net(g, "flood", local_graph=True, count_received=False) as net:
        with pytest.raises(P2PGError, match="bad state"):
            net.set_downtime(f, u)
    with gpu_net(g, "flood", count_received=False) as net:
        net.set_global_ids(np.arange(V, dtype=np.int32))
        with pytest.raises(P2PGError, match="bad state"):
            net.set_downtime(f, u)
    with gpu_net(g, "flood", count_received=False) as net:
        net.set_downtime(f, u)
        with pytest.raises(P2PGError, match="bad state"):
            net.set_global_ids(np.arange(V, dtype=np.int32))
        net.set_downtime(None)
        net.set_global_ids(np.arange(V, dtype=np.int32))
    # with all starts 0: snapshots are refused because of the downtime, and work without it
    with gpu_net(g, "flood", count_received=False) as net:
        net.broadcast([1, 2])
        net.set_downtime(f, u)
        with pytest.raises(P2PGError, match="bad state"):
            net.snapshot()
        net.set_downtime(None)
        net.step()
        assert len(net.snapshot()) > 0
    # a new graph clears it (p2pg_load_csr)
    with gpu_net(g, "flood", count_received=False) as net:
        net.set_downtime(f, u)
        net._check(L.p2pg_load_csr(net._h, g.V, _lib.ptr(g.rowptr), _lib.ptr(g.colidx)))
        net.broadcast([10])  # peer 10 joined late under the old downtime
        assert net.step().received_exact == 1 and len(net.snapshot()) > 0
