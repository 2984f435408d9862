"""Generate the anti-entropy fixtures (tests/golden/pull/*.npz) by driving the REFERENCE's own
Node / NodeConnection, like make_down_golden.py (whose harness and loss rule this one reuses).

Runs only in the build container (needs the reference checkout make_golden.py names); writes plain
.npz data files (inputs + expected outputs, loaded with allow_pickle=False).

The app is make_golden's dedup relay plus Demers-style pull repair, an ordinary p2pnetwork app: in a
request round every online node with a connection sends ``{"pull": "req", "digest": [...]}`` to one
connection (``lemire32(philox((round, id, 0, 'AEP'), seed).x, deg)`` into its ascending list); a node
queues the requests that arrive and, after the round's arrivals and originations, answers each with
``{"pull": "rep", "mids": [...]}`` -- what it has seen and the digest lacks, an empty list
included; a reply's unseen messages are first receipts of the round it arrives in, from that
connection, and are relayed like any other.  The harness's round is arrivals, originations,
replies, requests; ``dropped`` is DownHarness's (churn, or the receiver offline in the next round),
so requests and replies are lost like any send of their round.  ``Node.send_to_node`` counts before
it sends (node.py:116); pull packets are tagged, so their counts go to pull_sent / pull_recv and
the relay counters stay relay packets only.

The four fixtures stand on the down fixtures' graphs, sources, start rounds and downtime
schedules (read from tests/golden/down/*.npz), without hop limits or a relay policy.  The period is
drawn from {1, 3, 4}, the first request round from 1 .. 3, ``last`` is three rounds after the last
return; the seed is searched until the census (pull_ref.census) holds, and the generator fails if
none does.  One fixture has a named exemption (pull_ref.EXEMPT): the no-churn flood on the 4-regular
graph cannot hold `race` and `row_full` under the down fixture's schedule, whatever the setting.

Per fixture: the down fixtures' fields (CSR, src, start, down_from / down_until, hop, parent,
round_relays, total_recv, peer_sent, peer_recv, the mode fields), anti_entropy = (period, first,
last), pull_seed, exchanges (int64 [n, 6]: request_round, requests, requests_lost, replies,
replies_lost, repaired), pull_sent / pull_recv (int64 [V]) and census (the items asked).

Usage:  python tests/golden/make_pull_golden.py
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))  # tests/: pull_ref, down_ref
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the repository: oracle
import make_golden as mg  # noqa: E402
import pull_ref  # noqa: E402
from make_golden import PeerGraph  # noqa: E402
from make_down_golden import DownHarness  # noqa: E402

OUT = os.path.join(HERE, "pull")
DOWN = os.path.join(HERE, "down")
FOREVER = pull_ref.FOREVER

_relay_node_class = mg.make_node_class


def make_pull_node_class(NodeBase):
    Relay = _relay_node_class(NodeBase)

    class PullNode(Relay):
        """The dedup relay app with pull repair: a request queue, answered once per round."""

        def __init__(self, i, harness):
            super().__init__(i, harness)
            self.requests = []      # (connection, digest) that arrived in this round
            self.pull_sent = 0      # request and reply packets (send_to_node calls)
            self.pull_recv = 0
            self.by_relay = set()   # mids a relay packet carried to this node in this round
            self.by_reply = set()   # mids first received from a reply in this round

        def node_message(self, node, data):
            kind = data.get("pull")
            if kind == "req":
                self.requests.append((node, set(data["digest"])))
            elif kind == "rep":
                for mid in data["mids"]:
                    if mid not in self.seen:
                        self.by_reply.add(mid)
                        self.first_receipt(mid, int(node.id))
                        self.relay({"mid": mid}, exclude=node)
            else:
                self.by_relay.add(data["mid"])
                super().node_message(node, data)

        def pull_send(self, conn, data):
            before = self.message_count_send
            self.send_to_node(conn, data)  # counts, then sends (node.py:116)
            self.pull_sent += self.message_count_send - before
            self.message_count_send = before  # (tagged: the relay counter stays relay packets only)

        def answer(self):
            h = self.harness
            for conn, digest in self.requests:
                rec = h.records[h.round - 1]
                rec["replies"] += 1
                rec["replies_lost"] += int(h.dropped(int(self.id), int(conn.id)))
                self.pull_send(conn, {"pull": "rep", "mids": sorted(m for m in self.seen if m not in digest)})
            self.requests = []

        def ask(self):
            h = self.harness
            n = len(self.by_peer)
            if n == 0:
                return
            conn = self.by_peer[int(pull_ref.partner_slot(h.round, int(self.id), n, h.pull_seed))]
            rec = h.records[h.round]
            rec["requests"] += 1
            rec["requests_lost"] += int(h.dropped(int(self.id), int(conn.id)))
            self.pull_send(conn, {"pull": "req", "digest": sorted(self.seen)})

    return PullNode


class PullHarness(DownHarness):
    def __init__(self, *a, **kw):
        mg.make_node_class = make_pull_node_class  # Harness.__init__ builds its nodes from it
        try:
            mg.Harness.__init__(self, *a, **kw)
        finally:
            mg.make_node_class = _relay_node_class

    def online(self, v):
        return not (self.down_from[v] >= 0 and self.down_from[v] <= self.round < self.down_until[v])

    def run(self, src, start, down_from, down_until, setting, pull_seed):
        """A round is arrivals, originations, replies, requests."""
        V, M = self.g.V, len(src)
        self.down_from = [int(x) for x in down_from]
        self.down_until = [int(x) for x in down_until]
        self.pull_seed = int(pull_seed)
        start = [int(s) for s in start]
        sends = lambda: sum(n.message_count_send for n in self.nodes)  # noqa: E731
        last = max(start)
        rounds = []
        self.records = {}
        eot = (0x04).to_bytes(1, "big")
        self.round = -1
        while self.outbox or last > self.round or pull_ref.arrival_ahead(self.round + 1, setting):
            self.round += 1
            batch = sorted(self.outbox)  # (receiver, sender, seq): a reply follows its sender's relay packets
            self.outbox = []
            before = sends()
            for n in self.nodes:
                n.by_relay, n.by_reply = set(), set()
            i = 0
            while i < len(batch):
                rcv, snd = batch[i][0], batch[i][1]
                buf = b""
                while i < len(batch) and batch[i][0] == rcv and batch[i][1] == snd:
                    buf += batch[i][3]
                    i += 1
                conn = self.conn[(rcv, snd)]
                node = self.nodes[rcv]
                assert self.online(rcv)
                pos = buf.find(eot)
                while pos > 0:  # nodeconnection.py:209-218
                    packet, buf = buf[:pos], buf[pos + 1:]
                    data = conn.parse_packet(packet)
                    if "pull" in data:
                        node.pull_recv += 1
                    else:
                        node.message_count_recv += 1
                    node.node_message(conn, data)
                    pos = buf.find(eot)
            if self.round - 2 in self.records:  # the exchange is complete
                self.records[self.round - 2]["repaired"] = sum(len(n.by_reply - n.by_relay) for n in self.nodes)
            for m in range(M):
                if start[m] == self.round:
                    assert self.online(int(src[m]))
                    node = self.nodes[int(src[m])]
                    node.first_receipt(m, -1)
                    node.relay({"mid": m})
            for n in self.nodes:
                n.answer()
            if pull_ref.request_round(self.round, setting):
                self.records[self.round] = dict(request_round=self.round, requests=0, requests_lost=0, replies=0,
                                                replies_lost=0, repaired=0)
                for v, n in enumerate(self.nodes):
                    if self.online(v):
                        n.ask()
            rounds.append(sends() - before)
        hop = np.full((V, M), -1, dtype=np.int32)
        parent = np.full((V, M), -1, dtype=np.int32)
        for v, n in enumerate(self.nodes):
            for mid, (r, p) in n.seen.items():
                hop[v, mid] = r
                parent[v, mid] = p
        sent = np.array([n.message_count_send for n in self.nodes], dtype=np.int64)
        recv = np.array([n.message_count_recv for n in self.nodes], dtype=np.int64)
        psent = np.array([n.pull_sent for n in self.nodes], dtype=np.int64)
        precv = np.array([n.pull_recv for n in self.nodes], dtype=np.int64)
        recs = np.array([[self.records[r][k] for k in pull_ref.RECORD] for r in sorted(self.records)],
                        dtype=np.int64).reshape(-1, len(pull_ref.RECORD))
        return hop, parent, np.array(rounds, dtype=np.int64), sent, recv, recs, psent, precv


def pull_case(name, down_name, seed0, tries=200):
    with np.load(os.path.join(DOWN, down_name + ".npz"), allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    graph = PeerGraph(d["rowptr"], d["colidx"])
    src, start, f, u = d["src"], d["start"], d["down_from"], d["down_until"]
    mode, k = str(d["mode"]), int(d["fanout"])
    gseed, cthr, cseed = int(d["gossip_seed"]), int(d["churn_threshold"]), int(d["churn_seed"])
    kw = dict(mode=mode, fanout=k, gossip_seed=gseed, churn_threshold=cthr, churn_seed=cseed)
    last = int(u[(f >= 0) & (u < FOREVER)].max()) + 3  # three rounds after the last return
    nopull = pull_ref.run(graph.rowptr, graph.colidx, src, start, f, u, **kw)
    # the whole census of the case, less the items pull_ref.EXEMPT names for this one fixture
    need = tuple(x for x in pull_ref.census_items(mode == "gossip", cthr != 0) if x not in pull_ref.EXEMPT.get(name, ()))
    zk = dict(rowptr=graph.rowptr, colidx=graph.colidx, down_from=f, down_until=u, mode=np.array(mode),
              fanout=np.int64(k), churn_threshold=np.uint64(cthr), churn_seed=np.uint64(cseed))
    def attempt(seed):
        rng = np.random.default_rng(seed)
        setting = (int(rng.choice([1, 3, 4])), int(rng.integers(1, 4)), last)
        res = pull_ref.run(graph.rowptr, graph.colidx, src, start, f, u, anti_entropy=setting, pull_seed=seed, **kw)
        return setting, res, pull_ref.census(dict(zk, anti_entropy=np.array(setting), pull_seed=np.uint64(seed)), res, nopull)

    for seed in range(seed0, seed0 + tries):
        setting, res, got = attempt(seed)
        if all(got[x] for x in need):
            break
    else:
        raise AssertionError(f"{name}: no seed in {seed0} .. {seed0 + tries - 1} holds the census")
    if name in pull_ref.EXEMPT:
        print(f"{name}: {', '.join(pull_ref.EXEMPT[name])} cannot occur under the down fixture's schedule "
              f"(pull_ref.EXEMPT) and are not asked of this fixture")
    recs = res.records()
    print(f"{name}: seed {seed}: period {setting[0]}, first {setting[1]}, last {setting[2]}; census "
          f"{', '.join(x for x in pull_ref.CENSUS if got[x])}; {len(recs)} exchanges, requests {recs[:, 1].sum()} "
          f"(lost {recs[:, 2].sum()}), replies {recs[:, 3].sum()} (lost {recs[:, 4].sum()}), repaired {recs[:, 5].sum()}; "
          f"delivered {(res.hop >= 0).sum()} against {(nopull.hop >= 0).sum()} without, "
          f"{((res.hop >= 0) & (nopull.hop < 0)).sum()} never delivered without")
    t = time.time()
    hop, parent, relays, sent, recv, hrecs, psent, precv = PullHarness(graph, mode, k, gseed, cthr, cseed).run(
        src, start, f, u, setting, seed)
    dt = time.time() - t
    assert np.array_equal(res.hop, hop) and np.array_equal(res.parent, parent), f"{name}: pull_ref differs"
    assert pull_ref.pad_equal(res.column("relays"), relays), f"{name}: relays per round differ"
    assert np.array_equal(res.peer_sent, sent) and np.array_equal(res.peer_recv, recv), f"{name}: peer counters differ"
    assert np.array_equal(recs, hrecs), f"{name}: exchange records differ"
    assert np.array_equal(res.pull_sent, psent) and np.array_equal(res.pull_recv, precv), f"{name}: pull counters differ"
    out = dict(rowptr=graph.rowptr, colidx=graph.colidx, src=src, start=start, down_from=f, down_until=u, hop=hop,
               parent=parent, round_relays=relays, total_recv=np.int64(recv.sum()), peer_sent=sent, peer_recv=recv,
               mode=np.array(mode), fanout=np.int64(k), gossip_seed=np.uint64(gseed), churn_threshold=np.uint64(cthr),
               churn_seed=np.uint64(cseed), anti_entropy=np.array(setting, dtype=np.int32), pull_seed=np.uint64(seed),
               exchanges=hrecs, pull_sent=psent, pull_recv=precv, census=np.array(need))
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 100 * 1024, name
    print(f"{name}: V={graph.V} M={len(src)} mode={mode} rounds={len(relays)} relays={relays.sum()} "
          f"delivered={(hop >= 0).sum()} ({dt:.1f}s) -> {os.path.getsize(path)} B")
    return set(need)


def main():
    mg.Node, mg.NodeConnection = mg._load_reference()
    asked = pull_case("pull_rrg200_flood", "down_rrg200_flood", 100)
    asked |= pull_case("pull_ws300_flood_churn10", "down_ws300_flood_churn10", 200)
    asked |= pull_case("pull_ba300_gossip_k2_churn10", "down_ba300_gossip_k2_churn10", 300)
    asked |= pull_case("pull_ba300_gossip_k2", "down_ba300_gossip_k2", 400)
    assert asked == set(pull_ref.CENSUS), set(pull_ref.CENSUS) - asked


if __name__ == "__main__":
    main()
