#!/usr/bin/env python
"""What the run tallies cost: JSON lines for

  * config 4 with tally=False against tally=True, engines alternating on one box: host wall ms
    per reset + run step (the opt-in price of P2PG_FLAG_TALLY);
  * p2pg_message_reach on the finished run's seen plane (host wall of the call, which includes its
    two small allocations, a synchronisation and the copy of M counts) next to a plain streaming
    read of as many bytes (torch sum over an int64 tensor, HIP events).

Device time per kernel (k_colcount / k_tally_fold / k_peer_tally, the split of the price into
the column pass and the peer pass) comes from running this tool under
`rocprofv3 --kernel-trace --stats -- python tools/tally_cost.py ...`: the tally passes are not
kernel classes of p2pg_kernel_times (P2PG_KCLASS_N is part of the C-ABI).

    python tools/tally_cost.py [--peers 10000000] [--msgs 4096] [--steps 3] [--reps 2]
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
    ap.add_argument("--peers", type=int, default=10_000_000)
    ap.add_argument("--msgs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--no-stream-read", action="store_true")
    args = ap.parse_args()
    import numpy as np
    from p2pnetwork.gpu import GraphNetwork, PeerGraph, make_sources
    g = PeerGraph.barabasi_albert(args.peers, 4, seed=1)
    src = make_sources(g.V, args.msgs, seed=1)
    plane_bytes = g.V * ((args.msgs + 63) // 64) * 8
    for rep in range(args.reps):
        for tally in (False, True):
            with GraphNetwork(g, mode="gossip", fanout=3, gossip_seed=0x5EED, tally=tally) as net:
                net.broadcast(src)
                net.run()  # warm-up (first launches, the spare seen plane)
                ms = []
                for _ in range(args.steps):
                    t0 = time.perf_counter()
                    net.reset()
                    rounds = net.run()
                    if tally:
                        net.peer_counters()  # the last round's peer pass and the read-back
                    ms.append((time.perf_counter() - t0) * 1e3)
                line = {"what": "step", "rep": rep, "tally": tally, "peers": g.V, "msgs": args.msgs,
                        "rounds": len(rounds), "ms_per_step": [round(x, 3) for x in ms],
                        "ms_median": round(float(np.median(ms)), 3)}
                print(json.dumps(line), flush=True)
                rt = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    reach = net.message_reach()
                    rt.append((time.perf_counter() - t0) * 1e3)
                line = {"what": "message_reach", "rep": rep, "tally": tally, "plane_bytes": plane_bytes,
                        "host_ms": [round(x, 3) for x in rt],
                        "gbps_host_best": round(plane_bytes / (min(rt) * 1e-3) / 1e9, 1),
                        "reach_min": int(reach.min()), "reach_max": int(reach.max())}
                if tally:
                    line["equals_tally"] = bool((net.message_tally().reach == reach).all())
                print(json.dumps(line), flush=True)
    if not args.no_stream_read:
        import torch
        x = torch.ones(plane_bytes // 8, dtype=torch.int64, device="cuda")
        ts = []
        for _ in range(4):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            s = x.sum()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        assert int(s.item()) == plane_bytes // 8
        print(json.dumps({"what": "stream_read_torch_sum", "bytes": plane_bytes,
                          "device_ms": [round(t, 3) for t in ts],
                          "gbps_best": round(plane_bytes / (min(ts[1:]) * 1e-3) / 1e9, 1)}), flush=True)


if __name__ == "__main__":
    main()
