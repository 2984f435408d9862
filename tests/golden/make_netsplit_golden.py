"""Generate the netsplit fixtures (tests/golden/netsplit/*.npz) by driving the REFERENCE's own Node /
NodeConnection through make_pull_golden.py's PullHarness, which routes relay packets, requests and
replies through ``dropped(a, b)``.  This file overrides only that method: a packet sent in this round
over {a, b} is dropped as well if ``side[a] != side[b]`` and the round it would arrive in lies in
``[cut_from, cut_until)``.

Runs only in the build container (needs the reference checkout make_golden.py names); writes plain
.npz data files (inputs + expected outputs, loaded with allow_pickle=False).

The four fixtures stand on the pull fixtures' graphs, sources, start rounds, churn and gossip seeds
(read from tests/golden/pull/*.npz).  Three have anti-entropy on (their request rounds run from
inside the window to well after the heal), one of them keeps the pull fixture's downtime as well, one
uses three sides; ba300_gossip_k2 runs without anti-entropy and without a downtime.  The sides, the
window (8 to 19 rounds from round 2 .. 6 on), the request rounds (from two rounds before the window
to 6 .. 11 rounds after the heal) and the pull seed are drawn from a seed that is searched until
the fixture's part of the census (netsplit_ref.CENSUS) holds and no receipt is later than relative
hop 43, the largest of the fixture inventory tests/test_latency.py pins.  One item cannot hold on these graphs at all and is listed as
such for every fixture: `hub_pick_wasted` asks for a gossip sender of degree > 64, and the widest
peer of the 300-peer Barabasi-Albert graph has 52 connections (the GPU suite covers that case on a
graph with a 701-connection hub: tests/test_gpu_netsplit.py).

Per fixture: the pull fixtures' fields plus side (int32 [V]), cut_from, cut_until, msg_sent / msg_recv
(uint64 [M], netsplit_ref's, equal to the harness's totals) and census / census_impossible (the items
asked of it and the items it cannot have).

Usage:  python tests/golden/make_netsplit_golden.py
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))  # tests/: netsplit_ref, pull_ref
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the repository: oracle
import latency_ref  # noqa: E402
import make_golden as mg  # noqa: E402
import netsplit_ref  # noqa: E402
from make_golden import PeerGraph  # noqa: E402
from make_pull_golden import PullHarness  # noqa: E402

OUT = os.path.join(HERE, "netsplit")
PULL = os.path.join(HERE, "pull")
REPORT = os.path.join(os.path.dirname(os.path.dirname(HERE)), "profiles", "netsplit", "make_netsplit_golden.txt")
FLOOD_IMPOSSIBLE = ("hub_pick_wasted",)  # a flood has no picks
NO_HUB = ("hub_pick_wasted",)            # no peer of degree > 64 on the fixtures' graphs
NO_PULL = ("request_cut", "reply_cut", "repaired_across")  # a fixture without anti-entropy


class NetsplitHarness(PullHarness):
    def dropped(self, a, b):
        # a packet sent in this round would arrive in the next one
        return super().dropped(a, b) or (self.side[a] != self.side[b] and self.cut_from <= self.round + 1 < self.cut_until)


def case(name, pull_name, seed0, log, nsides=2, pull=True, downtime=False, tries=300):
    with np.load(os.path.join(PULL, pull_name + ".npz"), allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    graph = PeerGraph(d["rowptr"], d["colidx"])
    V = graph.V
    src, start = d["src"], d["start"]
    f, u = (d["down_from"], d["down_until"]) if downtime else netsplit_ref.no_downtime(V)
    mode, k = str(d["mode"]), int(d["fanout"])
    gseed, cthr, cseed = int(d["gossip_seed"]), int(d["churn_threshold"]), int(d["churn_seed"])
    kw = dict(down_from=f, down_until=u, mode=mode, fanout=k, gossip_seed=gseed, churn_threshold=cthr, churn_seed=cseed)
    impossible = tuple(dict.fromkeys((FLOOD_IMPOSSIBLE if mode == "flood" else NO_HUB) + (() if pull else NO_PULL)))
    assert int(np.diff(graph.rowptr).max()) <= 64
    need = tuple(x for x in netsplit_ref.CENSUS if x not in impossible)
    last_start = int(start.max())

    def attempt(seed):
        rng = np.random.default_rng(seed)
        if rng.integers(0, 2):
            side = (np.arange(V) * nsides // V).astype(np.int32)  # by id range
        else:
            side = rng.integers(0, nsides, V).astype(np.int32)
        cf = int(rng.integers(2, 7))
        cu = cf + int(rng.integers(8, 20))
        # request rounds from two rounds before the window (the request of round cut_from - 2 arrives,
        # its reply is cut) through the window to some rounds after the heal
        setting = (int(rng.choice([1, 2, 3])), cf - 2, cu + int(rng.integers(6, 12))) if pull else None
        zk = dict(rowptr=graph.rowptr, colidx=graph.colidx, src=src, side=side, cut_from=cf, cut_until=cu, down_from=f,
                  down_until=u, mode=np.array(mode), fanout=k, churn_threshold=cthr, churn_seed=cseed,
                  anti_entropy=np.array(setting if pull else (0, 0, 0)), pull_seed=seed)
        nopull = netsplit_ref.run(graph.rowptr, graph.colidx, src, start, side, cf, cu, **kw)
        res = netsplit_ref.run(graph.rowptr, graph.colidx, src, start, side, cf, cu, anti_entropy=setting,
                               pull_seed=seed, **kw) if pull else nopull
        return side, cf, cu, setting, res, netsplit_ref.census(zk, res, nopull)

    for seed in range(seed0, seed0 + tries):
        side, cf, cu, setting, res, got = attempt(seed)
        # (tests/test_latency.py walks every hop plane under tests/golden and pins the largest
        # relative hop of the inventory, 43: these fixtures stay below it)
        if all(got[x] for x in need) and int(latency_ref.relative(res.hop, start).max()) <= 43:
            break
    else:
        raise AssertionError(f"{name}: no seed in {seed0} .. {seed0 + tries - 1} holds the census")
    t = time.time()
    h = NetsplitHarness(graph, mode, k, gseed, cthr, cseed)
    h.side, h.cut_from, h.cut_until = [int(x) for x in side], cf, cu
    hop, parent, relays, sent, recv, hrecs, psent, precv = h.run(src, start, f, u, setting, seed)
    dt = time.time() - t
    assert np.array_equal(res.hop, hop) and np.array_equal(res.parent, parent), f"{name}: netsplit_ref differs"
    assert netsplit_ref.pad_equal(res.column("relays"), relays), f"{name}: relays per round differ"
    assert np.array_equal(res.peer_sent, sent) and np.array_equal(res.peer_recv, recv), f"{name}: peer counters differ"
    assert np.array_equal(res.records(), hrecs), f"{name}: exchange records differ"
    assert np.array_equal(res.pull_sent, psent) and np.array_equal(res.pull_recv, precv), f"{name}: pull counters differ"
    assert int(res.msg_sent.sum()) == int(sent.sum()) and int(res.msg_recv.sum()) == int(recv.sum())
    out = dict(rowptr=graph.rowptr, colidx=graph.colidx, src=src, start=start, down_from=f, down_until=u, hop=hop,
               parent=parent, round_relays=relays, total_recv=np.int64(recv.sum()), peer_sent=sent, peer_recv=recv,
               mode=np.array(mode), fanout=np.int64(k), gossip_seed=np.uint64(gseed), churn_threshold=np.uint64(cthr),
               churn_seed=np.uint64(cseed), anti_entropy=np.array(setting if pull else (0, 0, 0), dtype=np.int32),
               pull_seed=np.uint64(seed), exchanges=hrecs, pull_sent=psent, pull_recv=precv, side=side,
               cut_from=np.int32(cf), cut_until=np.int32(cu), msg_sent=res.msg_sent, msg_recv=res.msg_recv,
               census=np.array(need), census_impossible=np.array(impossible))
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 100 * 1024, name
    recs = res.records()
    log(f"{name}: seed {seed}: {nsides} sides ({np.bincount(side).tolist()}), window [{cf}, {cu}), anti-entropy "
        f"{setting}, downtime {'yes' if downtime else 'no'}; census {', '.join(need)}; cannot hold: "
        f"{', '.join(impossible)}; {len(recs)} exchanges, requests lost {recs[:, 2].sum() if len(recs) else 0}, replies "
        f"lost {recs[:, 4].sum() if len(recs) else 0}, repaired {recs[:, 5].sum() if len(recs) else 0}; V={V} "
        f"M={len(src)} mode={mode} rounds={len(relays)} relays={relays.sum()} delivered={(hop >= 0).sum()} "
        f"({dt:.1f}s) -> {os.path.getsize(path)} B")
    return set(need)


def main():
    mg.Node, mg.NodeConnection = mg._load_reference()
    lines = []

    def log(s):
        print(s)
        lines.append(s)

    asked = case("rrg200_flood", "pull_rrg200_flood", 100, log, nsides=2, downtime=True)
    asked |= case("ws300_flood_churn10", "pull_ws300_flood_churn10", 200, log, nsides=3)
    asked |= case("ba300_gossip_k2", "pull_ba300_gossip_k2", 300, log, nsides=2, pull=False)
    asked |= case("ba300_gossip_k2_churn10", "pull_ba300_gossip_k2_churn10", 400, log, nsides=2)
    missing = set(netsplit_ref.CENSUS) - asked
    log(f"census items no fixture can hold: {', '.join(sorted(missing)) or 'none'} (no peer of degree > 64 on the "
        f"pull fixtures' graphs; covered on the GPU by the 701-connection hub of tests/test_gpu_netsplit.py)")
    assert missing <= {"hub_pick_wasted"}, missing
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
