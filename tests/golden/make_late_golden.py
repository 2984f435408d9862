"""Generate the late-origination fixtures (tests/golden/late/*.npz) by driving the REFERENCE's own
Node / NodeConnection, like make_golden.py (whose harness this one extends).

Runs only in the build container (needs the reference checkout make_golden.py names); writes plain
.npz data files (inputs + expected outputs, loaded with allow_pickle=False).

A p2pnetwork app calls ``Node.send_to_nodes(data)`` (node.py:106-112) whenever it has something to
say, not only before the network starts.  Here message m is originated at ``src[m]`` in round
``start[m]``: after that round's arrivals have been handed to ``node_message``, the origin's
``RelayNode`` takes the first receipt (hop = the round, parent -1) and relays -- flood to all its
connections, gossip to the k Philox picks of (round, origin, m) -- on the reference's own Node.
Those packets arrive in the next round under this round's churn draw.  The loop runs while packets
are in flight or a start lies ahead, so idle gaps are crossed.

Per fixture: CSR, src, start, hop, parent (absolute round indices), round_relays, total_recv,
peer_sent / peer_recv (every node's own message_count_send / message_count_recv) and the mode
fields of the other fixtures.

Usage:  python tests/golden/make_late_golden.py
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from make_golden import Harness, PeerGraph, make_sources  # noqa: E402

OUT = os.path.join(HERE, "late")


class LateHarness(Harness):
    def run(self, src, start):
        V, M = self.g.V, len(src)
        start = [int(s) for s in start]
        sends = lambda: sum(n.message_count_send for n in self.nodes)  # noqa: E731
        last = max(start)
        rounds = []
        eot = (0x04).to_bytes(1, "big")
        self.round = -1
        while self.outbox or last > self.round:
            self.round += 1
            batch = sorted(self.outbox)  # (receiver, sender, seq)
            self.outbox = []
            before = sends()
            i = 0
            while i < len(batch):  # this round's arrivals first (NodeConnection.run's framing)
                rcv, snd = batch[i][0], batch[i][1]
                buf = b""
                while i < len(batch) and batch[i][0] == rcv and batch[i][1] == snd:
                    buf += batch[i][3]
                    i += 1
                conn = self.conn[(rcv, snd)]
                node = self.nodes[rcv]
                pos = buf.find(eot)
                while pos > 0:  # nodeconnection.py:209-218
                    packet, buf = buf[:pos], buf[pos + 1:]
                    node.message_count_recv += 1
                    node.node_message(conn, conn.parse_packet(packet))
                    pos = buf.find(eot)
            for m in range(M):  # then the messages due: Node.send_to_nodes / send_to_node at the origin
                if start[m] == self.round:
                    node = self.nodes[int(src[m])]
                    node.first_receipt(m, -1)
                    node.relay({"mid": m})
            rounds.append(sends() - before)
        hop = np.full((V, M), -1, dtype=np.int32)
        parent = np.full((V, M), -1, dtype=np.int32)
        for v, n in enumerate(self.nodes):
            for mid, (r, p) in n.seen.items():
                hop[v, mid] = r
                parent[v, mid] = p
        sent = np.array([n.message_count_send for n in self.nodes], dtype=np.int64)
        recv = np.array([n.message_count_recv for n in self.nodes], dtype=np.int64)
        return hop, parent, np.array(rounds, dtype=np.int64), sent, recv


def late_case(name, graph, src, start, mode="flood", k=3, gseed=0, churn=0.0, cseed=0):
    thr = int(np.floor(churn * 4294967296.0)) if churn else 0
    src = np.asarray(src, dtype=np.int32)
    start = np.asarray(start, dtype=np.int32)
    t = time.time()
    hop, parent, relays, sent, recv = LateHarness(graph, mode, k, gseed, thr, cseed).run(src, start)
    dt = time.time() - t
    os.makedirs(OUT, exist_ok=True)
    out = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(out, rowptr=graph.rowptr, colidx=graph.colidx, src=src, start=start, hop=hop,
                        parent=parent, round_relays=relays, total_recv=np.int64(recv.sum()),
                        peer_sent=sent, peer_recv=recv, mode=np.array(mode), fanout=np.int64(k),
                        gossip_seed=np.uint64(gseed), churn_threshold=np.uint64(thr),
                        churn_seed=np.uint64(cseed))
    print(f"{name}: V={graph.V} M={len(src)} mode={mode} rounds={len(relays)} relays={relays.sum()} "
          f"delivered={(hop >= 0).sum()} ({dt:.1f}s) -> {os.path.getsize(out)} B")


def spread_starts(M, seed, hi, tail):
    """Starts spread over rounds 0 .. hi, the last len(tail) messages at the rounds of `tail`."""
    rng = np.random.default_rng(seed)
    start = rng.integers(0, hi + 1, M).astype(np.int32)
    start[M - len(tail):] = tail
    return start


def main():
    mg.Node, mg.NodeConnection = mg._load_reference()
    # flood, 200-peer 4-regular: starts over rounds 0-6, five well after quiescence; messages
    # 3/4/5 share one origin and round, 66/67 (the second word) share the origin of a late one
    g = PeerGraph.random_regular(200, 4, seed=61)
    src = make_sources(g.V, 70, seed=61)
    start = spread_starts(70, 61, 6, [30, 30, 31, 45, 45])
    src[4] = src[5] = src[3]
    start[4] = start[5] = start[3] = 2
    src[66] = src[65]
    start[66] = start[65]
    src[68] = src[69]
    late_case("late_rrg200_flood", g, src, start)
    g = PeerGraph.watts_strogatz(300, 6, 0.1, seed=62)
    src = make_sources(g.V, 40, seed=62)
    start = spread_starts(40, 62, 5, [25, 26, 26])
    late_case("late_ws300_flood_churn10", g, src, start, churn=0.10, cseed=17)
    g = PeerGraph.barabasi_albert(300, 3, seed=63)
    src = make_sources(g.V, 130, seed=63)
    start = spread_starts(130, 63, 7, [40, 40, 41, 100])
    src[10] = src[11] = src[100]  # one origin, one round, two words
    start[10] = start[11] = start[100] = 3
    src[129] = 0  # a hub of the BA graph, long after quiescence
    late_case("late_ba300_gossip_k2", g, src, start, mode="gossip", k=2, gseed=23)
    late_case("late_ba300_gossip_k2_churn10", g, src, start, mode="gossip", k=2, gseed=23, churn=0.10,
              cseed=29)


if __name__ == "__main__":
    main()
