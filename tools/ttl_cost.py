#!/usr/bin/env python
"""What hop limits cost: JSON lines for

  * config 3's flood (1M-peer G(n,p), mean degree 16, 4096 broadcasts) and a 1M-peer
    Barabasi-Albert (m = 4) push-gossip with 4096 broadcasts and fanout 3 (tools/late_cost.py's
    shapes),
  * each run three times: without limits, with ttl = 4 for every broadcast (all start in round 0:
    one expiry round), and as a stream -- 64 new broadcasts per round over rounds 0 .. 63 with
    limits mixed over 1 .. 8 (nearly every round is an expiry round),

with host wall ms per reset + run, rounds, relays, first receipts and the push forms of the rounds.

Device time of k_expire (two launches per expiry round: the relay correction inside the round,
the clearing at the boundary) comes from running this tool under
`rocprofv3 --kernel-trace --stats -- python tools/ttl_cost.py ...`; the line's `expiry_rounds` and
`active_rows_in_expiry_rounds` (x W x 8 bytes: what the two passes read, and at most write) set it
against the bytes it moves.

    python tools/ttl_cost.py [--peers 1000000] [--msgs 4096] [--per-round 64] [--steps 3]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "python-p2p-network_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--peers", type=int, default=1_000_000)
    ap.add_argument("--msgs", type=int, default=4096)
    ap.add_argument("--per-round", type=int, default=64)
    ap.add_argument("--steps", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    from p2pnetwork.gpu import GraphNetwork, PeerGraph, make_sources
    from p2pnetwork.gpu.network import PUSH_FORMS
    M = args.msgs
    stream = (np.arange(M) // args.per_round).astype(np.int32)
    mixed = (1 + np.random.default_rng(1).integers(0, 8, M)).astype(np.int32)
    scheds = (("unlimited", None, None), ("ttl4", None, np.full(M, 4, dtype=np.int32)),
              ("stream_ttl1to8", stream, mixed))
    cases = (("c3_flood", lambda: PeerGraph.gnp(args.peers, 16, seed=1), dict(mode="flood")),
             ("ba_gossip", lambda: PeerGraph.barabasi_albert(args.peers, 4, seed=1),
              dict(mode="gossip", fanout=3, gossip_seed=0x5EED)))
    for name, graph, kw in cases:
        g = graph()
        src = make_sources(g.V, M, seed=1)
        for sched, start, ttl in scheds:
            with GraphNetwork(g, **kw) as net:
                net.broadcast(src, start, ttl)
                net.run()  # warm-up (first launches, the spare seen plane)
                ms = []
                for _ in range(args.steps):
                    t0 = time.perf_counter()
                    net.reset()
                    rounds = net.run()
                    ms.append((time.perf_counter() - t0) * 1e3)
                relays = sum(r.relays for r in rounds)
                forms = {}
                for r in rounds:
                    forms[PUSH_FORMS[r.push_form]] = forms.get(PUSH_FORMS[r.push_form], 0) + 1
                xs = set()
                if ttl is not None:
                    xs = set(((0 if start is None else start.astype(np.int64)) + ttl).tolist())
                med = float(np.median(ms))
                print(json.dumps({"what": name, "schedule": sched, "peers": g.V, "msgs": M, "W": (M + 63) // 64,
                                  "rounds": len(rounds), "relays": relays,
                                  "delivered": int(sum(r.new_deliveries for r in rounds)),
                                  "expiry_rounds": len([r for r in rounds if r.round in xs]),
                                  "active_rows_in_expiry_rounds":
                                      int(sum(r.active_vertices for r in rounds if r.round in xs)),
                                  "ms_per_run": [round(x, 3) for x in ms], "ms_median": round(med, 3),
                                  "gteps": round(relays / (med * 1e-3) / 1e9, 2), "push_forms": forms}),
                      flush=True)


if __name__ == "__main__":
    main()
