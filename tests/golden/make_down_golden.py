"""Generate the peer-downtime fixtures (tests/golden/down/*.npz) by driving the REFERENCE's own
Node / NodeConnection, like make_policy_golden.py (whose harness and app this one reuses).

Runs only in the build container (needs the reference checkout make_golden.py names); writes plain
.npz data files (inputs + expected outputs, loaded with allow_pickle=False).

Peer v is offline in the rounds ``down_from[v] <= r < down_until[v]`` (-1: never; 0x7FFFFFFF: it
never returns).  An offline peer keeps its connections; its neighbours have no failure detector and
go on sending to it.  ``Node.send_to_node`` counts before it sends (node.py:116) and the harness's
``FakeSock.sendall`` returns silently on a broken link, so the whole rule is one more term in
``Harness.dropped(a, b)``: churn, or ``b`` offline in ``self.round + 1`` -- the round the packet
would arrive in.  The app is make_golden's dedup relay, unchanged.

The four fixtures stand on the late fixtures' graphs, sources and start rounds; no origin or start
had to move (the schedules are drawn so that no origin is offline in its start round).  The flood
on the 4-regular graph also carries the policy fixture's hop limits and relay policy.  The
schedule: a fifth of the peers carry an interval -- a tenth of those crash in rounds 1-7, a tenth
join late (offline from round 0 until a round in 2-9), the rest have an outage of 1-3 rounds
anywhere in the run -- plus, where some peer's row fills at all, one peer that is offline in
exactly the round its row would have filled, and, where chance does not give it (a flood), a
one-round outage of the few receivers of one message's sends of one round, so that all of them are
lost.  The seed of each schedule is searched until the census (down_ref.census) holds.

Per fixture: the fields of the policy fixtures (CSR, src, start, ttl, thr, policy_seed, hop, parent,
round_relays, total_recv, peer_sent, peer_recv, the mode fields) plus down_from / down_until
(int32 [V]).

Usage:  python tests/golden/make_down_golden.py
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))  # tests/: down_ref, policy_ref
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the repository: oracle
import make_golden as mg  # noqa: E402
import down_ref  # noqa: E402
import policy_ref  # noqa: E402
from make_golden import PeerGraph, make_sources  # noqa: E402
from make_late_golden import spread_starts  # noqa: E402
from make_policy_golden import PolicyHarness, draw_thresholds  # noqa: E402
from oracle import philox  # noqa: E402

OUT = os.path.join(HERE, "down")
FOREVER = down_ref.FOREVER
ITEMS = down_ref.CENSUS
census = down_ref.census


class DownHarness(PolicyHarness):
    def run(self, src, start, ttl, thr, pseed, down_from, down_until):
        self.down_from = [int(x) for x in down_from]
        self.down_until = [int(x) for x in down_until]
        return super().run(src, start, ttl, thr, pseed)

    def dropped(self, a, b):
        # a packet sent in this round would arrive in the next one
        return super().dropped(a, b) or self.down_from[b] >= 0 and self.down_from[b] <= self.round + 1 < self.down_until[b]


def draw_schedule(V, seed, run_rounds, src, start):
    """A fifth of the peers: a tenth of them crash in rounds 1-7, a tenth join in rounds 2-9, the
    rest have an outage of 1-3 rounds anywhere in the run.  An interval that would hold one of the
    peer's own originations is redrawn."""
    rng = np.random.default_rng(seed)
    down_from = np.full(V, -1, dtype=np.int32)
    down_until = np.full(V, FOREVER, dtype=np.int32)
    peers = rng.permutation(V)[:V // 5]
    n10 = max(1, len(peers) // 10)
    own = {}
    for m, s in enumerate(src):
        own.setdefault(int(s), []).append(int(start[m]))
    for i, v in enumerate(peers):
        for _ in range(64):
            if i < n10:
                f, u = int(rng.integers(1, 8)), FOREVER
            elif i < 2 * n10:
                f, u = 0, int(rng.integers(2, 10))
            else:
                f = int(rng.integers(1, run_rounds))
                u = f + int(rng.integers(1, 4))
            if not any(f <= s < u for s in own.get(int(v), [])):
                down_from[v], down_until[v] = f, u
                break
    return down_from, down_until


def fills_somewhere(full):
    return bool((full.hop >= 0).all(axis=1).any())


def lose_one_round(res, f, u, src, start):
    """A flood with six connections per peer does not lose every send of a message in one round by
    chance.  Take the (message, round) whose sends go to the fewest receivers that are still
    reachable, none of which carries an interval or originates in the next round, and give those
    receivers a one-round outage in the round the sends would arrive in (the rounds up to that one
    are unchanged by it).  Returns whether one was found."""
    src, start = np.asarray(src), np.asarray(start)
    best = None
    for r in range(1, len(res.sends) - 1):
        snd, tgt, msg, lost = res.sends[r]
        for m in np.unique(msg):
            open_t = np.unique(tgt[(msg == m) & ~lost])
            if len(open_t) == 0 or (f[open_t] >= 0).any() or ((start == r + 1) & np.isin(src, open_t)).any():
                continue
            if best is None or len(open_t) < len(best[1]) or (len(open_t) == len(best[1]) and r > best[0]):
                best = (r, open_t)
    if best is None:
        return False
    f[best[1]], u[best[1]] = best[0] + 1, best[0] + 2
    return True


def search_schedule(name, case, kw, rule, need, seed0, tries=400):
    """The first seed from seed0 whose schedule holds every census item of `need` and keeps the
    fixture from going degenerate."""
    g, src, start = case
    V, M = g.V, len(src)
    full = down_ref.run(g.rowptr, g.colidx, src, start, drop=rule, **kw)
    feasible = fills_somewhere(full)
    need = [x for x in need if x != "row_full" or feasible]
    zk = dict(rowptr=g.rowptr, fanout=np.int64(kw.get("fanout", 3)), churn_threshold=np.uint64(kw.get("churn_threshold", 0)),
              churn_seed=np.uint64(kw.get("churn_seed", 0)))
    for seed in range(seed0, seed0 + tries):
        f, u = draw_schedule(V, seed, len(full.rounds), src, start)
        if feasible:
            # one peer (without an interval, no origin of that round) is offline in exactly the
            # round its row fills in the run so far
            res = down_ref.run(g.rowptr, g.colidx, src, start, f, u, drop=rule, **kw)
            rows = np.nonzero((res.hop >= 0).all(axis=1) & (f < 0))[0]
            rows = [v for v in rows if res.hop[v].max() > 0 and
                    not ((np.asarray(src) == v) & (np.asarray(start) == res.hop[v].max())).any()]
            if not rows:
                continue
            v = rows[seed % len(rows)]
            f[v], u[v] = int(res.hop[v].max()), int(res.hop[v].max()) + 1
        res = down_ref.run(g.rowptr, g.colidx, src, start, f, u, drop=rule, **kw)
        got = census(dict(zk, down_from=f, down_until=u), res, full)
        if "all_lost" in need and not got["all_lost"] and lose_one_round(res, f, u, src, start):
            res = down_ref.run(g.rowptr, g.colidx, src, start, f, u, drop=rule, **kw)
            got = census(dict(zk, down_from=f, down_until=u), res, full)
        kept = (res.hop >= 0).sum() / max(1, (full.hop >= 0).sum())
        wide = int(((res.hop >= 0).sum(axis=0) * 2 >= V).sum())
        wide_full = int(((full.hop >= 0).sum(axis=0) * 2 >= V).sum())
        if all(got[x] for x in need) and kept >= 0.9 and wide * 2 >= wide_full:
            later = int(((res.hop > full.hop) & (full.hop >= 0)).sum())
            never = int(((res.hop < 0) & (full.hop >= 0)).sum())
            print(f"{name}: schedule seed {seed}: {int((f >= 0).sum())} peers with an interval; census "
                  f"{', '.join(x for x in ITEMS if got[x])}" + ("" if feasible else " (no row fills without a downtime either: row_full not asked)") +
                  f"; first receipts kept {100 * kept:.1f} %, messages reaching half {wide} / {wide_full}, "
                  f"receipts later {later}, never {never}")
            return f, u, res, need
    raise AssertionError(f"{name}: no schedule in {tries} seeds holds the census")


def down_case(name, graph, src, start, seed0, need, ttl=None, thr=None, pseed=0, mode="flood", k=3, gseed=0,
              churn=0.0, cseed=0):
    cthr = int(np.floor(churn * 4294967296.0)) if churn else 0
    src = np.asarray(src, dtype=np.int32)
    start = np.asarray(start, dtype=np.int32)
    ttl = np.full(len(src), -1, dtype=np.int32) if ttl is None else np.asarray(ttl, dtype=np.int32)
    thr = np.zeros(graph.V, dtype=np.uint32) if thr is None else np.asarray(thr, dtype=np.uint32)
    kw = dict(mode=mode, fanout=k, gossip_seed=gseed, churn_threshold=cthr, churn_seed=cseed)
    rule = policy_ref.with_ttl(policy_ref.policy_rule(thr, pseed, start), start, ttl)
    f, u, res, need = search_schedule(name, (graph, src, start), kw, rule, need, seed0)
    t = time.time()
    hop, parent, relays, sent, recv = DownHarness(graph, mode, k, gseed, cthr, cseed).run(src, start, ttl, thr, pseed, f, u)
    dt = time.time() - t
    assert np.array_equal(res.hop, hop) and np.array_equal(res.parent, parent), f"{name}: down_ref differs"
    assert down_ref.pad_equal(res.column("relays"), relays), f"{name}: relays per round differ"
    assert np.array_equal(res.peer_sent, sent) and np.array_equal(res.peer_recv, recv), f"{name}: peer counters differ"
    z = dict(rowptr=graph.rowptr, colidx=graph.colidx, src=src, start=start, ttl=ttl, thr=thr,
             policy_seed=np.uint64(pseed), down_from=f, down_until=u, hop=hop, parent=parent, round_relays=relays,
             total_recv=np.int64(recv.sum()), peer_sent=sent, peer_recv=recv, mode=np.array(mode),
             fanout=np.int64(k), gossip_seed=np.uint64(gseed), churn_threshold=np.uint64(cthr),
             churn_seed=np.uint64(cseed), census=np.array(need))
    os.makedirs(OUT, exist_ok=True)
    out = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(out, **z)
    assert os.path.getsize(out) < 100 * 1024, name
    print(f"{name}: V={graph.V} M={len(src)} mode={mode} rounds={len(relays)} relays={relays.sum()} "
          f"delivered={(hop >= 0).sum()} ({dt:.1f}s) -> {os.path.getsize(out)} B")


def main():
    mg.Node, mg.NodeConnection = mg._load_reference()
    flood = [x for x in ITEMS if x != "gossip_deg"]
    # the late fixtures' graphs, sources and start rounds
    g = PeerGraph.random_regular(200, 4, seed=61)
    src = make_sources(g.V, 70, seed=61)
    start = spread_starts(70, 61, 6, [30, 30, 31, 45, 45])
    src[4] = src[5] = src[3]
    start[4] = start[5] = start[3] = 2
    src[66] = src[65]
    start[66] = start[65]
    src[68] = src[69]
    # ... with the policy fixture's hop limits and relay policy
    thr = draw_thresholds(g.V, 81, (0.55, 0.08, 0.12, 0.17, 0.08), silent_at=[src[3]])
    ttl = np.array([3, 4, 6, -1, -1], dtype=np.int32)[np.random.default_rng(82).integers(0, 5, 70)]
    down_case("down_rrg200_flood", g, src, start, 100, flood, ttl=ttl, thr=thr, pseed=0xA11CE)
    g = PeerGraph.watts_strogatz(300, 6, 0.1, seed=62)
    src = make_sources(g.V, 40, seed=62)
    start = spread_starts(40, 62, 5, [25, 26, 26])
    down_case("down_ws300_flood_churn10", g, src, start, 200, flood, churn=0.10, cseed=17)
    g = PeerGraph.barabasi_albert(300, 3, seed=63)
    src = make_sources(g.V, 130, seed=63)
    start = spread_starts(130, 63, 7, [40, 40, 41, 100])
    src[10] = src[11] = src[100]  # one origin, one round, two words
    start[10] = start[11] = start[100] = 3
    src[129] = 0  # a hub of the BA graph, long after quiescence
    down_case("down_ba300_gossip_k2", g, src, start, 300, ITEMS, mode="gossip", k=2, gseed=23)
    down_case("down_ba300_gossip_k2_churn10", g, src, start, 400, ITEMS, mode="gossip", k=2, gseed=23, churn=0.10,
              cseed=29)


if __name__ == "__main__":
    main()
