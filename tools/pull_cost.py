#!/usr/bin/env python
"""What anti-entropy costs and buys: JSON lines for

  * config 3's flood (1M-peer G(n,p), mean degree 16, 4096 broadcasts) and a 1M-peer
    Barabasi-Albert (m = 4) push-gossip with 4096 broadcasts and fanout 3 (tools/downtime_cost.py's
    shapes),
  * each run three times: without a downtime, with 10 % of the peers in a two-round outage
    (rounds 5 and 6), and that plus anti-entropy of period 4 from the return (round 7) until 8
    rounds after it,

with host wall ms per reset + run, rounds, relays, first receipts, what the exchanges repaired and
the push forms of the rounds, each against the no-downtime arm of the same session.  No origin
carries an interval.

Device time of k_pull_gather / k_pull_apply (one launch each per arrival round) comes from running
this tool under `rocprofv3 --kernel-trace --stats -- python tools/pull_cost.py ...`; the gather
reads two rows per peer and writes at most one, so its bytes per launch are at most 3 * V * W * 8.

    python tools/pull_cost.py [--peers 1000000] [--msgs 4096] [--steps 3]
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
        free = np.setdiff1d(np.arange(g.V), src)  # (originations at an offline peer are refused)
        pick = np.random.default_rng(1).permutation(free)[:g.V // 10]
        f = np.full(g.V, -1, dtype=np.int32)
        u = np.full(g.V, 0x7FFFFFFF, dtype=np.int32)
        f[pick], u[pick] = 5, 7
        setting = (4, 7, 7 + 8)  # period, first, last
        arms = (("none", None, None), ("outage_10pct_rounds5_6", (f, u), None),
                ("outage_and_anti_entropy_p4", (f, u), setting))
        base = None
        for arm, down, ae in arms:
            with GraphNetwork(g, **kw) as net:
                net.broadcast(src)
                if down is not None:
                    net.set_downtime(*down)
                if ae is not None:
                    net.set_anti_entropy(*ae, seed=1)
                net.run()  # warm-up (first launches, the spare seen plane, the reply plane)
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
                line = {"what": name, "arm": arm, "peers": g.V, "msgs": M, "W": (M + 63) // 64,
                        "rounds": len(rounds), "relays": relays,
                        "delivered": int(sum(r.new_deliveries for r in rounds)),
                        "ms_per_run": [round(x, 3) for x in ms], "ms_median": round(med, 3),
                        "push_forms": forms,
                        "push_form_per_round": "".join(PUSH_FORMS[r.push_form][0] for r in rounds)}
                if ae is not None:
                    ps = net.pull_stats()
                    line["anti_entropy"] = {"period": ae[0], "first": ae[1], "last": ae[2]}
                    line["exchanges"] = [{k: int(x[k]) for k in ("request_round", "requests", "requests_lost", "replies",
                                                                 "replies_lost", "repaired")} for x in ps]
                    line["repaired"] = int(ps["repaired"].sum())
                    line["gather_bytes_bound_per_launch"] = 3 * g.V * ((M + 63) // 64) * 8
                if base is None:
                    base = line
                else:
                    line["ms_vs_none"] = round(med / base["ms_median"], 3)
                    line["delivered_vs_none"] = round(line["delivered"] / base["delivered"], 6)
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
