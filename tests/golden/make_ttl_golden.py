"""Generate the hop-limit fixtures (tests/golden/ttl/*.npz) by driving the REFERENCE's own Node /
NodeConnection, like make_late_golden.py (whose harness this one extends).

Runs only in the build container (needs the reference checkout make_golden.py names); writes plain
.npz data files (inputs + expected outputs, loaded with allow_pickle=False).

A p2pnetwork application bounds a broadcast with a hop budget in its payload: the dedup app here
takes every first receipt as make_golden's RelayNode does, and forwards ``{"mid": m, "ttl": t - 1}``
while ``t > 0`` (README.md:20: the app decides; the sends are the reference's own
Node.send_to_nodes / send_to_node, node.py:106-116).  A payload without a ``ttl`` field is
unlimited.  The origin handles its own message the same way: ``ttl = 0`` marks it seen and sends
nothing.

Per fixture: the fields of the late fixtures (CSR, src, start, hop, parent, round_relays,
total_recv, peer_sent, peer_recv, the mode fields) plus ttl (int32 [M], -1 = unlimited).

Usage:  python tests/golden/make_ttl_golden.py
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))  # tests/: late_ref, the restatement without hop limits
import make_golden as mg  # noqa: E402
import late_ref  # noqa: E402
from make_golden import PeerGraph, make_sources  # noqa: E402
from make_late_golden import LateHarness, spread_starts  # noqa: E402

OUT = os.path.join(HERE, "ttl")
TTLS = (0, 1, 2, 3, 4, 6, -1)

_relay_node_class = mg.make_node_class


def make_ttl_node_class(NodeBase):
    Relay = _relay_node_class(NodeBase)

    class TtlNode(Relay):
        """The dedup relay app with a hop budget in the payload."""

        def node_message(self, node, data):
            mid = data["mid"]
            if mid in self.seen:  # dedup: drop echoes (README.md:20)
                return
            self.first_receipt(mid, int(node.id))
            self.forward(data, exclude=node)

        def forward(self, data, exclude=None):
            if "ttl" not in data:  # unlimited
                super().relay(data, exclude=exclude)
            elif data["ttl"] > 0:
                super().relay({"mid": data["mid"], "ttl": data["ttl"] - 1}, exclude=exclude)

        def relay(self, data, exclude=None):
            """LateHarness.run originates with ``relay({"mid": m})`` at the origin: the app's own
            send_to_nodes call, which puts the message's budget into the payload."""
            t = self.harness.ttl[data["mid"]]
            self.forward({"mid": data["mid"], "ttl": t} if t >= 0 else data, exclude=exclude)

    return TtlNode


class TtlHarness(LateHarness):
    def __init__(self, *a, **kw):
        mg.make_node_class = make_ttl_node_class  # Harness.__init__ builds its nodes from it
        try:
            super().__init__(*a, **kw)
        finally:
            mg.make_node_class = _relay_node_class

    def run(self, src, start, ttl):
        self.ttl = [int(t) for t in ttl]
        return super().run(src, start)


def census(name, z, full_hop):
    """What every fixture must hold (re-checked from the data by tests/test_ttl.py); full_hop = the
    hop plane of the same run without hop limits (tests/late_ref.py)."""
    start, ttl, hop = z["start"].astype(np.int64), z["ttl"].astype(np.int64), z["hop"]
    M = len(ttl)
    fin = ttl >= 0
    rel = np.where(hop >= 0, hop - start[None, :], -1)
    assert set(ttl.tolist()) <= set(TTLS), name
    assert (rel[:, fin] <= ttl[fin][None, :]).all(), "no receipt past the hop limit"
    same = ((hop >= 0) == (full_hop >= 0)).all(axis=0)  # the limit took no receipt away
    assert same[~fin].all(), name
    assert (fin & ~same).any(), f"{name}: no message is cut short"
    assert (fin & same & (ttl > 0)).any(), f"{name}: no finite-ttl message finishes inside its limit"
    assert (ttl == 0).sum() >= 1 and (ttl == -1).sum() >= 1, name
    xs = np.where(fin, start + ttl, -1)
    assert len(set(xs[fin].tolist())) >= 3, f"{name}: fewer than 3 expiry rounds"
    assert set(xs[fin].tolist()) & set(start[start > 0].tolist()), f"{name}: no expiry round is an origination round"
    words = np.arange(M) // 64
    assert any(len(set(xs[(words == w) & fin].tolist())) >= 2 for w in set(words.tolist())), name
    if M > 64:
        assert any(any((xs[words == w] == r).all() for w in set(words.tolist())) and
                   any(not (xs[words == w] == r).any() for w in set(words.tolist()))
                   for r in set(xs[fin].tolist())), f"{name}: no word expires whole beside an untouched one"


def ttl_case(name, graph, src, start, ttl, mode="flood", k=3, gseed=0, churn=0.0, cseed=0):
    thr = int(np.floor(churn * 4294967296.0)) if churn else 0
    src = np.asarray(src, dtype=np.int32)
    start = np.asarray(start, dtype=np.int32)
    ttl = np.asarray(ttl, dtype=np.int32)
    t = time.time()
    hop, parent, relays, sent, recv = TtlHarness(graph, mode, k, gseed, thr, cseed).run(src, start, ttl)
    dt = time.time() - t
    z = dict(rowptr=graph.rowptr, colidx=graph.colidx, src=src, start=start, ttl=ttl, hop=hop,
             parent=parent, round_relays=relays, total_recv=np.int64(recv.sum()),
             peer_sent=sent, peer_recv=recv, mode=np.array(mode), fanout=np.int64(k),
             gossip_seed=np.uint64(gseed), churn_threshold=np.uint64(thr),
             churn_seed=np.uint64(cseed))
    full = late_ref.run(graph.rowptr, graph.colidx, src, start, mode, k, gseed, 0, thr, cseed)
    census(name, z, full.hop)
    os.makedirs(OUT, exist_ok=True)
    out = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(out, **z)
    print(f"{name}: V={graph.V} M={len(src)} mode={mode} rounds={len(relays)} relays={relays.sum()} "
          f"delivered={(hop >= 0).sum()} ({dt:.1f}s) -> {os.path.getsize(out)} B")


def draw_ttls(M, seed):
    rng = np.random.default_rng(seed)
    ttl = np.array(TTLS, dtype=np.int32)[rng.integers(0, len(TTLS), M)]
    ttl[0], ttl[1] = 0, -1
    return ttl


def main():
    mg.Node, mg.NodeConnection = mg._load_reference()
    # the late fixtures' graphs, sources and start rounds
    g = PeerGraph.random_regular(200, 4, seed=61)
    src = make_sources(g.V, 70, seed=61)
    start = spread_starts(70, 61, 6, [30, 30, 31, 45, 45])
    src[4] = src[5] = src[3]
    start[4] = start[5] = start[3] = 2
    src[66] = src[65]
    start[66] = start[65]
    src[68] = src[69]
    ttl = draw_ttls(70, 71)
    ttl[64:] = [4, 0, 0, 1, 6, 2]  # the second word expires whole in round 30 ...
    start[64:] = 30 - ttl[64:]
    ttl[:64] = np.where(start[:64] + ttl[:64] == 30, -1, ttl[:64])  # ... the first not at all
    ttl[0] = 0
    ttl[3], ttl[4] = 1, 3  # one origin, one round, one word: different expiry rounds
    ttl[2] = 6  # a flood of depth 6-7: may finish inside its budget
    ttl[6] = 2
    start[7], ttl[7] = start[6] + 2, 4  # starts in the round message 6 expires
    ttl_case("ttl_rrg200_flood", g, src, start, ttl)
    g = PeerGraph.watts_strogatz(300, 6, 0.1, seed=62)
    src = make_sources(g.V, 40, seed=62)
    start = spread_starts(40, 62, 5, [25, 26, 26])
    ttl = draw_ttls(40, 72)
    ttl[2], start[3] = 2, start[2] + 2
    # floods on this graph under this churn are 6-9 hops deep; from peer 173 one started in round
    # 2 is 6 deep (found by search over the origins): it finishes inside ttl 6
    src[5], start[5], ttl[5] = 173, 2, 6
    ttl_case("ttl_ws300_flood_churn10", g, src, start, ttl, churn=0.10, cseed=17)
    g = PeerGraph.barabasi_albert(300, 3, seed=63)
    src = make_sources(g.V, 130, seed=63)
    start = spread_starts(130, 63, 7, [40, 40, 41, 100])
    src[10] = src[11] = src[100]  # one origin, one round, two words
    start[10] = start[11] = start[100] = 3
    src[129] = 0  # a hub of the BA graph, long after quiescence
    ttl = draw_ttls(130, 73)
    ttl[64:128] = 4  # the second word expires whole in round 9, the first and third not at all
    start[64:128] = 5
    ttl[:64] = np.where(start[:64] + ttl[:64] == 9, -1, ttl[:64])
    ttl[128:] = np.where(start[128:] + ttl[128:] == 9, -1, ttl[128:])
    ttl[0] = 0
    ttl[20], start[21] = 3, start[20] + 3  # message 21 starts in the round message 20 expires
    # gossip runs on this graph are 12-43 hops deep, so every limit drawn above cuts its message;
    # these two die out on their own after one hop (their receivers pick peers that hold them),
    # message 16 without churn and message 2 under it (found by search over the origins)
    src[16], start[16], ttl[16] = 67, 2, 4
    src[2], start[2], ttl[2] = 17, 1, 4
    ttl_case("ttl_ba300_gossip_k2", g, src, start, ttl, mode="gossip", k=2, gseed=23)
    ttl_case("ttl_ba300_gossip_k2_churn10", g, src, start, ttl, mode="gossip", k=2, gseed=23, churn=0.10,
             cseed=29)


if __name__ == "__main__":
    main()
