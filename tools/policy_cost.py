#!/usr/bin/env python
"""What a relay policy costs: JSON lines for

  * config 3's flood (1M-peer G(n,p), mean degree 16, 4096 broadcasts) and a 1M-peer
    Barabasi-Albert (m = 4) push-gossip with 4096 broadcasts and fanout 3 (tools/ttl_cost.py's
    shapes),
  * each run three times: without a policy, with 1 % silent peers (no draws: the rows of the
    silent peers are taken whole), and with relay probability 0.5 at every peer (a draw for every
    first receipt of every round),

with host wall ms per reset + run, rounds, relays, first receipts and the push forms of the rounds.
With a policy every round after round 0 runs the unfused schedule, so the gossip lines also show
what that schedule costs next to the fused one of the no-policy run.

Device time of k_policy (two launches per round after round 0: the relay correction inside the
round, the clearing at the boundary) comes from running this tool under
`rocprofv3 --kernel-trace --stats -- python tools/policy_cost.py ...`; the line's `policy_rounds`,
`active_rows` (x W x 8 bytes: what each pass reads, and at most writes) and `draws` (first receipts
at drawing peers: the receipts each pass decides; a lane evaluates Philox once per nonzero word,
`active_words`, whatever the number of set bits) set it against the bytes it moves and the draws
it makes.

    python tools/policy_cost.py [--peers 1000000] [--msgs 4096] [--steps 3]
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
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--only", default="", help="c3_flood or ba_gossip (default: both)")
    args = ap.parse_args()
    import numpy as np
    from p2pnetwork.gpu import GraphNetwork, PeerGraph, make_sources
    from p2pnetwork.gpu.network import PUSH_FORMS
    M = args.msgs
    cases = (("c3_flood", lambda: PeerGraph.gnp(args.peers, 16, seed=1), dict(mode="flood")),
             ("ba_gossip", lambda: PeerGraph.barabasi_albert(args.peers, 4, seed=1),
              dict(mode="gossip", fanout=3, gossip_seed=0x5EED)))
    for name, graph, kw in cases:
        if args.only and args.only != name:
            continue
        g = graph()
        src = make_sources(g.V, M, seed=1)
        silent = np.ones(g.V)
        silent[np.random.default_rng(1).choice(g.V, g.V // 100, replace=False)] = 0.0
        arms = (("none", None), ("silent_1pct", silent), ("q_0.5", 0.5))
        for arm, prob in arms:
            with GraphNetwork(g, **kw) as net:
                net.broadcast(src)
                net.set_relay_policy(prob, seed=0xA11CE)
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
                line = {"what": name, "arm": arm, "peers": g.V, "msgs": M, "W": (M + 63) // 64,
                        "rounds": len(rounds), "relays": relays,
                        "delivered": int(sum(r.new_deliveries for r in rounds))}
                if prob is not None:
                    pr = [r for r in rounds if r.round > 0]
                    line["policy_rounds"] = len(pr)
                    line["active_rows"] = int(sum(r.active_vertices for r in pr))
                    line["active_words"] = int(sum(r.active_words for r in pr))
                    thr = net.relay_thr
                    drawing = (thr != 0) & (thr != 0xFFFFFFFF)
                    line["drawing_peers"] = int(drawing.sum())
                    # every peer draws: one draw per first receipt that is no origination, per pass
                    line["draws"] = line["delivered"] - M if drawing.all() else 0 if not drawing.any() else None
                med = float(np.median(ms))
                line.update({"ms_per_run": [round(x, 3) for x in ms], "ms_median": round(med, 3),
                             "gteps": round(relays / (med * 1e-3) / 1e9, 2), "push_forms": forms})
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
