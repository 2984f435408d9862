#!/usr/bin/env python
"""What a netsplit costs: JSON lines for

  * config 3's flood (1M-peer G(n,p), mean degree 16, 4096 broadcasts) and a 1M-peer
    Barabasi-Albert (m = 4) push-gossip with 4096 broadcasts and fanout 3 (tools/downtime_cost.py's
    shapes),
  * each run three times: without a netsplit, with a two-side window (the peers split by id
    parity: about half of the connections cross) in the sparse phase (rounds 1 .. 3), and with one
    in the dense phase (three rounds from the round with the most first receipts of the plain run),

with host wall ms per reset + run, rounds, relays, first receipts and the push forms of the rounds,
each against the no-netsplit arm of the same session.  Then one stepped run per arm under
P2PG_FLAG_TIMING: the device ms of every kernel class per round, from which the lines
`kernel_ratio` compare, on the same rounds, the cut pull with the flood pull of the plain arm
(class flood_pull), and the cut push (class gossip_scatter_atomic) with what the plain arm spent on
that round's push (its atomic, store or fused class) and with the plain arm's median sparse push.

    python tools/netsplit_cost.py [--peers 1000000] [--msgs 4096] [--steps 3]
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
        gossip = kw["mode"] == "gossip"
        src = make_sources(g.V, M, seed=1)
        side = (np.arange(g.V) % 2).astype(np.int32)

        def timed_rounds(window):
            """Per round: {class: device ms} of a stepped run."""
            with GraphNetwork(g, timing=True, **kw) as net:
                net.broadcast(src)
                if window:
                    net.set_netsplit(side, *window)
                net.run()
                net.reset()
                out, before = [], {k: v[0] for k, v in net.kernel_times().items()}
                while True:
                    st = net.step()
                    now = {k: v[0] for k, v in net.kernel_times().items()}
                    out.append({k: now[k] - before[k] for k in now})
                    before = now
                    if not st.active:
                        return out

        base = base_rounds = base_ms = None
        arms = [("none", None), ("sparse_rounds_1_3", (1, 4)), ("dense", None)]
        for arm, window in arms:
            if arm == "dense":
                peak = int(np.argmax([r.new_deliveries for r in base_rounds]))
                window = (peak, peak + 3)
            with GraphNetwork(g, **kw) as net:
                net.broadcast(src)
                if window:
                    net.set_netsplit(side, *window)
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
            line = {"what": name, "arm": arm, "peers": g.V, "msgs": M, "W": (M + 63) // 64, "window": window,
                    "rounds": len(rounds), "relays": relays,
                    "delivered": int(sum(r.new_deliveries for r in rounds)),
                    "ms_per_run": [round(x, 3) for x in ms], "ms_median": round(med, 3),
                    "push_forms": forms, "push_form_per_round": "".join(PUSH_FORMS[r.push_form][0] for r in rounds)}
            per_round = timed_rounds(window)
            if window is None:
                base, base_rounds, base_ms = line, rounds, per_round
            else:
                line["ms_vs_none"] = round(med / base["ms_median"], 3)
                line["delivered_vs_none"] = round(line["delivered"] / base["delivered"], 4)
            print(json.dumps(line), flush=True)
            if window is None:
                continue
            cf, cu = window
            if gossip:
                acted = [r for r in range(len(per_round)) if cf <= r + 1 < cu]
                cls = "gossip_scatter_atomic"
                sparse = [x[cls] for x in base_ms if x[cls] > 0 and x["gossip_fused"] == 0 and x["gossip_scatter_store"] == 0]
                plain = [base_ms[r][cls] + base_ms[r]["gossip_scatter_store"] + base_ms[r]["gossip_fused"]
                         for r in acted if r < len(base_ms)]
            else:
                acted = [r for r in range(len(per_round)) if max(cf, 1) <= r < cu]
                cls = "flood_pull"
                sparse = []
                plain = [base_ms[r][cls] for r in acted if r < len(base_ms)]
            cut = [per_round[r][cls] for r in acted]
            ratio = {"what": name, "arm": arm, "line": "kernel_ratio", "class": cls, "rounds": acted,
                     "cut_ms": [round(x, 3) for x in cut], "plain_ms_same_rounds": [round(x, 3) for x in plain],
                     "ratio_same_rounds": [round(a / b, 2) if b > 0 else None for a, b in zip(cut, plain)]}
            if sparse:
                ratio["plain_sparse_push_ms_median"] = round(float(np.median(sparse)), 3)
            print(json.dumps(ratio), flush=True)


if __name__ == "__main__":
    main()
