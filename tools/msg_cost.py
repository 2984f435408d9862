#!/usr/bin/env python
"""What the per-message cost costs: JSON lines for config 4 with engines in four
settings alternating on one box -- no flags, cost=True, tally=True, both -- host wall ms per
reset + run step (the read of the counters included, which takes the last round's pass in).

Device time per kernel (k_msg_cost / k_cost_fold next to k_peer_tally / k_colcount) comes from
running this tool under `rocprofv3 --kernel-trace --stats -- python tools/msg_cost.py ...`: the
deferred passes are not kernel classes of p2pg_kernel_times (P2PG_KCLASS_N is part of the C-ABI).

    python tools/msg_cost.py [--peers 10000000] [--msgs 4096] [--steps 3] [--reps 2] [--churn 0.0]
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

SETTINGS = (("none", False, False), ("cost", False, True), ("tally", True, False), ("both", True, True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--peers", type=int, default=10_000_000)
    ap.add_argument("--msgs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--churn", type=float, default=0.0,
                    help="per-round connection loss: with it the pass re-draws the picks")
    ap.add_argument("--settings", default="none,cost,tally,both")
    args = ap.parse_args()
    import numpy as np
    from p2pnetwork.gpu import GraphNetwork, PeerGraph, make_sources
    g = PeerGraph.barabasi_albert(args.peers, 4, seed=1)
    src = make_sources(g.V, args.msgs, seed=1)
    want = set(args.settings.split(","))
    for rep in range(args.reps):
        for name, tally, cost in SETTINGS:
            if name not in want:
                continue
            with GraphNetwork(g, mode="gossip", fanout=3, gossip_seed=0x5EED, churn=args.churn, tally=tally,
                              cost=cost) as net:
                net.broadcast(src)
                net.run()  # warm-up (first launches, the spare seen plane)
                ms = []
                for _ in range(args.steps):
                    t0 = time.perf_counter()
                    net.reset()
                    rounds = net.run()
                    if tally:
                        net.peer_counters()  # the last round's passes and the read-back
                    if cost:
                        c = net.message_cost()
                    ms.append((time.perf_counter() - t0) * 1e3)
                line = {"what": "step", "rep": rep, "setting": name, "peers": g.V, "msgs": args.msgs,
                        "churn": args.churn, "rounds": len(rounds), "ms_per_step": [round(x, 3) for x in ms],
                        "ms_median": round(float(np.median(ms)), 3)}
                if cost:
                    line["sent_equals_relays"] = int(c.sent.sum()) == sum(r.relays for r in rounds)
                    red = net.message_redundancy()
                    line["redundancy_mean"] = round(float(np.nanmean(red)), 4)
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
