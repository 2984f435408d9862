#!/usr/bin/env python
"""What a stream of broadcasts costs: JSON lines for

  * config 3's flood (1M-peer G(n,p), mean degree 16, 4096 broadcasts) and a 1M-peer
    Barabasi-Albert (m = 4) push-gossip with 4096 broadcasts and fanout 3,
  * each run once with every start in round 0 (p2pg_set_sources) and once as a stream: 64 new
    broadcasts per round over rounds 0 .. 63 (p2pg_set_sources_at),

with host wall ms per reset + run, rounds, relays, GTEPS (relays / s / 1e9) and the push forms of
the rounds.  A stream's gossip rounds 1 .. 63 all originate, so none of them is fused: the table
says what those unfused rounds cost against the all-at-0 run.

Device time of k_originate (and of k_seed / k_zero_rows, the round-0 yardstick: one launch that
seeds as many messages as the schedule holds) comes from running this tool under
`rocprofv3 --kernel-trace --stats -- python tools/late_cost.py ...`: the all-at-0 runs launch
k_seed for 4096 messages, the streams k_seed for 64 and k_originate 63 times for 64 each.

    python tools/late_cost.py [--peers 1000000] [--msgs 4096] [--per-round 64] [--steps 3]
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
    cases = (("c3_flood", lambda: PeerGraph.gnp(args.peers, 16, seed=1), dict(mode="flood")),
             ("ba_gossip", lambda: PeerGraph.barabasi_albert(args.peers, 4, seed=1),
              dict(mode="gossip", fanout=3, gossip_seed=0x5EED)))
    for name, graph, kw in cases:
        g = graph()
        src = make_sources(g.V, M, seed=1)
        for sched, start in (("all_at_0", None), ("stream", stream)):
            with GraphNetwork(g, **kw) as net:
                net.broadcast(src, start)
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
                med = float(np.median(ms))
                print(json.dumps({"what": name, "schedule": sched, "peers": g.V, "msgs": M,
                                  "starts_per_round": 0 if start is None else args.per_round,
                                  "last_start": 0 if start is None else int(stream.max()),
                                  "rounds": len(rounds), "relays": relays,
                                  "ms_per_run": [round(x, 3) for x in ms], "ms_median": round(med, 3),
                                  "gteps": round(relays / (med * 1e-3) / 1e9, 2), "push_forms": forms,
                                  "delivered": int(sum(r.new_deliveries for r in rounds))}), flush=True)


if __name__ == "__main__":
    main()
