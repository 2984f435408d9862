"""The narrow sender's push of the fused gossip round -- its entry scan, its pick batches, and the
table pass and deferred flush over the mask table's 64-bit cells -- against the oracle, bit for bit
(profiles/narrow_push).

One graph of 1285 peers (the last 32-peer task is ragged) and message origins chosen so that round
1, the first round of the forms under test, holds every shape at which one of the parts can go
wrong.  Peers 0..19 are origins with one connection each (one, SHARED, has two): all their
broadcasts reach that neighbour in round 1 and nothing else does, so the list a peer pushes from in
round 1 is exactly what its origin was given:

* P[n], n = 1, 63, 64, 65, 1023, 1024 (deg 4): a list of exactly n entries -- one entry, one short
  of a batch, a whole batch, one more, one short of a list window and the second window.  P[63]'s
  bits all lie in word 0, P[1]'s in the last word.  (At M = 2112 the six counts exceed M: there
  1023 of P[1024]'s messages come from SHARED, whose other connection is P[1023].)
* task 2 (peers 64..95) is visited in this order: A (4 active words), Q, B (4), C (20), D (4),
  E (deg 3 = the fanout: the row copy, no table), F (4), G (nothing arrives), H (4), MED
  (16 < deg <= 64: the wide pass, whose tables lie in the same LDS), J (4).  A peer's flush runs
  one visit later, right before that visit's own table pass or wide pass; what stays live in
  between is the table.  The table pass clears and the flush reads the cells of the active words
  only, in segments of 16 or 32 lanes or row by row: a cell cleared or read at the wrong place
  shows where the segment width changes, after a peer without a table and after one without
  news, in the wide pass and in the next narrow push.  (The shapes were chosen when the flush
  also took its rank -> word map from the table pass; that part was measured and removed.)
  Q receives every broadcast that is not named here, all from peer 0: a full row, every word
  active, bits 31 and 32 of a word, words 0 and 32.
* the last peer, V - 1, has an origin too: the flush after the loop.

Each case runs under the forced store form (one unfused round, then fused rounds) and under the
automatic form with the update+push pass; seen / hop / parent planes and every per-round counter
equal the oracle's.  Every shape is asserted present from the oracle's hop plane and the run's push
forms, so a missing shape fails the test.  The churn seeds are ones under which no origin's
connection is down in round 0 (the shapes would go missing; found with the oracle alone).
"""
import functools

import numpy as np
import pytest

from test_gpu_parity import assert_rounds_equal, gpu_net

pytestmark = pytest.mark.gpu

V = 32 * 40 + 5
FANOUT = 3
NS = (1, 63, 64, 65, 1023, 1024)
P = {n: 160 + i for i, n in enumerate(NS)}  # the peers with a list of exactly n entries
A, Q, B, C, D, E, F, G, H, MED, J = range(64, 75)
LAST = V - 1
MED_EXTRA = 24
# origin -> its one connection (SHARED: P[1023] and P[1024])
RECEIVERS = [Q, A, B, C, D, E, F, H, MED, J, LAST] + [P[n] for n in NS]
ORIGIN = {u: o for o, u in enumerate(RECEIVERS)}  # peer 0 is Q's
SHARED = len(RECEIVERS)
N_ORIGINS = SHARED + 1
assert N_ORIGINS <= 20


@functools.lru_cache(maxsize=None)
def push_graph():
    from p2pnetwork.gpu import PeerGraph
    off_ring = set(range(N_ORIGINS)) | {E}
    ring = np.array([v for v in range(V) if v not in off_ring], dtype=np.int64)
    n = len(ring)
    # (the long step keeps the runs short: a ring of steps 1 and 7 alone takes ~200 rounds)
    edges = [np.stack([ring, ring[(np.arange(n) + s) % n]], axis=1) for s in (1, 7, 89)]
    edges.append(np.array([[o, u] for u, o in ORIGIN.items()], dtype=np.int64))
    edges.append(np.array([[SHARED, P[1023]], [SHARED, P[1024]], [E, 400], [E, 900]], dtype=np.int64))
    pos = int(np.searchsorted(ring, MED))
    far = [(pos + 100 + 9 * i) % n for i in range(MED_EXTRA)]
    edges.append(np.stack([np.full(MED_EXTRA, MED, dtype=np.int64), ring[far]], axis=1))
    g = PeerGraph.from_edges(V, np.concatenate(edges))
    deg = np.diff(g.rowptr)
    assert g.V == V and V % 32 == 5
    assert (deg[:SHARED] == 1).all() and deg[SHARED] == 2 and deg[E] == FANOUT
    assert 16 < deg[MED] <= 64
    narrow = [A, Q, B, C, D, F, G, H, J, LAST] + list(P.values())
    assert (deg[narrow] > FANOUT).all() and (deg[narrow] <= 16).all()
    return g


def plan(M):
    """src[m] for every broadcast m, and the words x bits layout behind it (module docstring)."""
    W = (M + 63) // 64
    src = np.zeros(M, dtype=np.int32)  # what is not handed out below: peer 0 -> Q
    free = np.ones(M, dtype=bool)

    def give(origin, ids):
        ids = np.asarray(ids, dtype=np.int64)
        assert ids.size and ids.max() < M and free[ids].all()
        free[ids] = False
        src[ids] = origin

    def column(bit, words):  # one bit of each of the words
        return [64 * w + bit for w in words]

    def pool(count, first_word):  # word-major from bits 12..47 of the words from first_word on
        ids = [64 * w + b for w in range(first_word, W) for b in range(12, 48)
               if 64 * w + b < M and free[64 * w + b]]
        assert len(ids) >= count
        return ids[:count]

    give(ORIGIN[P[63]], range(0, 63))                      # word 0 (its bit 63 stays with Q)
    give(ORIGIN[P[1]], [64 * (W - 1)])                     # the last word
    big = pool(1024, 1)
    if M >= 1024 + 1023 + 1200:
        give(ORIGIN[P[1024]], big)
        give(ORIGIN[P[1023]], pool(1023, 1))
    else:  # SHARED hands its 1023 to both, P[1024]'s own origin adds one
        give(SHARED, big[:1023])
        give(ORIGIN[P[1024]], big[1023:])
    give(ORIGIN[P[64]], [64 * w + b for w in range(1, 5) for b in range(48, 64)])
    give(ORIGIN[P[65]], [64 * w + b for w in range(5, 9) for b in range(48, 64)] + [64 * 9 + 48])
    give(ORIGIN[A], column(1, range(1, 5)))
    give(ORIGIN[B], column(2, range(1, 5)))
    give(ORIGIN[C], column(3, range(1, 21)))
    give(ORIGIN[D], column(4, range(5, 9)))
    give(ORIGIN[E], column(5, range(1, 4)))
    give(ORIGIN[F], column(6, range(1, 5)))
    give(ORIGIN[H], column(7, range(1, 5)))
    give(ORIGIN[MED], column(8, range(1, 7)))
    give(ORIGIN[J], column(9, range(1, 5)))
    give(ORIGIN[LAST], column(10, range(1, 5)))
    return src


# (M, gossip seed, churn threshold, churn seed, msg_id_base): the full width; W = 63 with a ragged
# last word; W = 33; churn (the row-by-row flush over the same table); global message ids
CASES = [(4096, 1234, 0, 0, 0), (4000, 77, 0, 0, 0), (2112, 5, 0, 0, 0),
         (4096, 1234, 300_000_000, 4106, 0), (4096, 99, 0, 0, 8192)]


@functools.lru_cache(maxsize=1)  # the forms of one case run back to back
def reference(M, gseed, thr, cseed, base):
    from oracle import relay_oracle
    g = push_graph()
    src = plan(M)
    ora = relay_oracle.gossip(g.rowptr, g.colidx, src, FANOUT, gseed, base, thr, cseed)
    for a in (src, ora.hop, ora.parent):
        a.setflags(write=False)
    return src, ora


def round1_shapes(g, hop, M):
    """The shapes among the pushes of round 1 (hop: [peer][message]; a peer pushes in round r what
    it first received in round r)."""
    W = (M + 63) // 64
    new = hop == 1
    cnt = new.sum(axis=1)
    pad = np.zeros((V, W * 64), dtype=bool)
    pad[:, :M] = new
    words = pad.reshape(V, W, 64).any(axis=2)  # [peer][word]: active in its round-1 push
    nf = words.sum(axis=1)
    deg = np.diff(g.rowptr)
    got = set()
    for n in NS:
        if cnt[P[n]] == n:
            got.add(f"list of {n}")
    if cnt[P[63]] and nf[P[63]] == 1 and words[P[63], 0]:
        got.add("all in word 0")
    if cnt[P[1]] and nf[P[1]] == 1 and words[P[1], W - 1]:
        got.add("all in the last word")
    qb = pad[Q].reshape(W, 64)
    if nf[Q] == W and words[Q, 0] and words[Q, 32] and (qb[:, 31] & qb[:, 32]).any():
        got.add("full row")

    def narrow(u):
        return FANOUT < deg[u] <= 16

    def few(u):
        return narrow(u) and 1 <= nf[u] <= 16

    if few(A) and narrow(Q) and nf[Q] > 32:
        got.add("<= 16 then > 32")
    if narrow(Q) and nf[Q] > 32 and few(B):
        got.add("> 32 then <= 16")
    if narrow(C) and 17 <= nf[C] <= 32 and few(D):
        got.add("17..32 then <= 16")
    if few(D) and deg[E] <= FANOUT and nf[E] and few(F):
        got.add("row copy between tables")
    if few(F) and cnt[G] == 0 and few(H):
        got.add("no news after a pending flush")
    if few(H) and 16 < deg[MED] <= 64 and nf[MED] and few(J):
        got.add("wide pass between narrow")
    if narrow(LAST) and nf[LAST]:
        got.add("last peer")
    return got


SHAPES = ({f"list of {n}" for n in NS} |
          {"all in word 0", "all in the last word", "full row", "<= 16 then > 32", "> 32 then <= 16",
           "17..32 then <= 16", "row copy between tables", "no news after a pending flush",
           "wide pass between narrow", "last peer"})


def test_layout():
    """(no GPU work) the plan hands every P[n] its n broadcasts at every M of the cases."""
    for M in sorted({c[0] for c in CASES}):
        src = plan(M)
        for n in NS:
            mine = (src == ORIGIN[P[n]]).sum() + (src == SHARED).sum() * (n >= 1023)
            assert mine == n, (M, n, mine)
        assert ((src == SHARED).sum() > 0) == (M == 2112)


@pytest.mark.parametrize("form", ["store", "auto_update"])  # (varies fastest)
@pytest.mark.parametrize("M,gseed,thr,cseed,base", CASES)
def test_narrow_push_matches_oracle(M, gseed, thr, cseed, base, form, monkeypatch):
    monkeypatch.setenv("P2PG_GOSSIP_PUSH", form.split("_")[0])
    monkeypatch.setenv("P2PG_FUSED", "1")
    monkeypatch.setenv("P2PG_UPDATE_PUSH", "1" if form == "auto_update" else "0")
    if form == "auto_update":
        # no floor on the active peers of a dense round: round 1 then already runs in the dense
        # forms (update+push, whose pushes are the same code, then fused)
        monkeypatch.setenv("P2PG_V_THRESH", "0")
    g = push_graph()
    src, ora = reference(M, gseed, thr, cseed, base)
    kw = {"msg_id_base": base} if base else {}
    with gpu_net(g, "gossip", FANOUT, gseed, thr, cseed, **kw) as net:
        net.broadcast(src)
        rounds = net.run()
        hop, parent = net.hop_parent()
        seen = net.delivered()
    forms = [r.push_form for r in rounds]
    print(form, "push forms", forms)
    delivering = [f for f, r in zip(forms, rounds) if r.new_deliveries]
    if form == "store":
        assert delivering[0] == 2 and delivering[1:] and all(f == 3 for f in delivering[1:]), forms
        under_test = {3}
    else:
        assert 4 in delivering, forms
        under_test = {3, 4}
    # not vacuous: the pushes of round 1 run in the form of round 1
    assert forms[1] in under_test, forms
    got = round1_shapes(g, ora.hop, M)
    if forms[1] == 4:
        # (the update+push pass visits the peers something arrived at: G is not among them there)
        assert (ora.hop[G] != 1).all()
        got.add("no news after a pending flush")
    print(form, "shapes", sorted(got))
    assert got == SHAPES, (sorted(SHAPES - got), forms)
    np.testing.assert_array_equal(seen, ora.hop >= 0)
    np.testing.assert_array_equal(hop, ora.hop)
    np.testing.assert_array_equal(parent, ora.parent)
    assert_rounds_equal(rounds, ora.rounds)
