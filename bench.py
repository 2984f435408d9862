#!/usr/bin/env python3
"""Benchmark of the MI355X relay engine on BASELINE.json's headline workload.

Metric (BASELINE.json): msg-edge relays/s (GTEPS) at 10M peers x 4096 msgs, 1-8 GPU, and % of
the HBM roofline.  One relay = one Node.send_to_node call (p2pnetwork/node.py:114-116).

Workload (default "c4" = BASELINE.json configs[3], the metric's own configuration): 10M-peer
Barabasi-Albert (m=4) graph, 4096 concurrent push-gossip broadcasts with fanout 3 (Philox
picks), synthetic graph and origins (no datasets).  A "step" = one complete broadcast: reset
of the per-run state + every round until quiescence, graph resident in HBM.

Multi-GPU (python -m torch.distributed.run --nproc-per-node N bench.py --gpus N): the SAME
4096 broadcasts are split across the ranks by message word (rank r runs messages
r*4096/N .. (r+1)*4096/N - 1, global message ids, so origins and Philox streams are those of the
1-GPU run) on a replica of the graph -- strong scaling (fixed total work), no data-path
collective, because broadcasts are independent bit lanes; value = relays of all ranks /
max-over-ranks time.  Config 5 (--workload c5) is vertex-partitioned instead (RCCL all-to-all of
boundary rows), and runs unpartitioned at N = 1.  --split vertex / message overrides the
workload's form (config 4 vertex-partitioned: every rank holds ~5M ghosts of the 10M BA graph at
N = 8, so the message split stays its default).

Prints ONE JSON line (rank 0) with the driver's fields plus "roofline" (dominant kernel:
SURVEY.md 8(d)'s algorithmic bytes B_r of the rounds it consumes / its HIP-event time; the
engine's own per-kernel byte model beside it as frac_engine_model).

A plain run does only what that line's headline needs: graph, warmup, the timed steps, the
outputs of --dump-outputs, the line.  --full adds what takes runs of its own: one more step with
every kernel class bracketed by HIP events ("kernel_ms_per_step", "kernel_time_frac_of_step"), one
broadcast stepped round by round ("dominant_ms_by_round", "dominant_round_fracs",
"roofline.survey_rounds_over_peak") and "cpu_baseline" (two CPU legs on the host cores: the
C/OpenMP oracle and the 1-core object-level relay simulator; --no-cpu-baseline leaves it out).

--dump-outputs DIR writes what the last timed step returned to its caller (rank 0's view):
DIR/rounds.npy (float64 [rounds, len(ROUND_FIELDS)]: the per-round counters of run(), all below
2^53) and, where the engine is a GraphNetwork, a fixed seeded sample of the seen plane it leaves
behind: DIR/seen_peers.npy and DIR/seen_words.npy (float64: the sampled peer ids and word indices)
and DIR/seen_sample.npy (float64 [words, peers, 2]: the low and high 32 bits of each sampled
uint64 word).  Graph, origins and Philox seeds are fixed, so two builds given the same arguments
can be compared file for file.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "python-p2p-network_amd"))

HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md, chip-level parameters)

WORKLOADS = {
    "c4": dict(graph="ba", V=10_000_000, a=4, M=4096, mode="gossip", fanout=3,
               name="config4: 10M-peer Barabasi-Albert m=4, 4096 push-gossip broadcasts, fanout 3"),
    "c3": dict(graph="gnp", V=1_000_000, a=16, M=4096, mode="flood", fanout=3,
               name="config3: 1M-peer Erdos-Renyi mean degree 16, 4096 flood broadcasts"),
    "c2": dict(graph="rrg", V=1000, a=8, M=64, mode="flood", fanout=3,
               name="config2: 1k-peer random 8-regular, 64 flood broadcasts"),
    "c5": dict(graph="ws", V=100_000_000, a=8, beta=0.1, M=4096, mode="flood", fanout=3, churn=0.05,
               partition=True,
               name="config5: 100M-peer Watts-Strogatz k=8 beta=0.1, 4096 flood broadcasts, "
                    "per-round edge-drop churn p=0.05, vertex-partitioned"),
}
GOSSIP_SEED, CHURN_SEED = 0x5EED, 0xC0FFEE
# --dump-outputs: the counters of a RoundStats that are results (push_form is how the engine
# scheduled the round, not one), and the seen-plane sample (2 * 8 B per sampled word: 32 MB)
ROUND_FIELDS = ("round", "active", "new_deliveries", "relays", "active_vertices", "active_words",
                "wedges", "deg_active", "scatter_words", "touched_words", "received", "received_exact")
DUMP_SEED, DUMP_PEERS, DUMP_WORDS = 0xD0C5, 500_000, 4

KCLASS = ("seed", "flood_pull", "gossip_scatter_atomic", "record", "gossip_update", "gossip_pull",
          "gossip_scatter_store", "gossip_fused")
ATOMIC, EDGE, FUSED, UPDATE_EDGE = 1, 2, 3, 4  # p2pg_round_stats.push_form (P2PG_PUSH_*)
E_FORMS = (EDGE, FUSED, UPDATE_EDGE)  # pushes into the E plane: the next round pulls them


def push_forms(rounds):
    """Each gossip round's push form; from the engine (push_form) when it reports one, else
    read off the next round (touched_words > 0 <=> the pushes went by row atomics)."""
    n = len(rounds)
    out = []
    for i, r in enumerate(rounds):
        f = getattr(r, "push_form", 0)
        if not f:
            f = EDGE if (i + 1 < n and rounds[i + 1].touched_words == 0 and r.active_vertices > 0) \
                else ATOMIC
        out.append(f)
    return out


def model_bytes(rounds, mode, W, packed=None, per_round=False):
    """Algorithmic HBM bytes per kernel class for one run.

    flood pull, round r:  8*wedges[r-1] + 8*words[r-1] + 4*degact[r-1]
                                        + 8*peers[r-1] + 24*words[r]
    gossip, pushes of round r:          atomic: 8*words[r] + 8*peers[r] + 4*degact[r]
                                                + 16*scatter[r] (read-modify-write of each
                                                pushed word by a row atomicOr)
                                        edge:   8*words[r] + 8*peers[r] + 4*degact[r]
                                                + 8*wedges[r] (packed E rows, W <= 64: each
                                                connection of an active sender gets the
                                                sender's active words only; 8*W*degact[r]
                                                unpacked)
    gossip, arrivals of round r >= 1:   after atomic pushes (update): 24*touched[r] + 16*words[r]
                                        after edge pushes (pull):     8*wedges[r-1] (packed;
                                                unpacked 8*W*degact[r-1]) + 24*words[r]
    fused round r (pull + pushes in one pass, gossip_fused):
                                        8*wedges[r-1] + 24*words[r] + 4*degact[r] + 8*wedges[r]
                                        (the frontier row is not re-read: no 8*words[r])
    update + edge pushes in one pass (UPDATE_EDGE, timed with gossip_scatter_store): the update's
                                        and the edge pushes' bytes, both in that class
    """
    rows = [{k: 0 for k in KCLASS} for _ in rounds]  # bytes charged to each round's kernels
    if packed is None:
        packed = W <= 64
    forms = push_forms(rounds) if mode == "gossip" else []

    def e_bytes(r):
        return 8 * (r.wedges if packed else W * r.deg_active)

    for i, r in enumerate(rounds):
        b = rows[i]
        if mode == "flood":
            if i >= 1:
                p = rounds[i - 1]
                b["flood_pull"] += (8 * p.wedges + 8 * p.active_words + 4 * p.deg_active
                                    + 8 * p.active_vertices + 24 * r.active_words)
            continue
        if forms[i] == FUSED:
            b["gossip_fused"] += (e_bytes(rounds[i - 1]) + 24 * r.active_words + 4 * r.deg_active
                                  + e_bytes(r))
            continue
        if i >= 1:
            if forms[i - 1] in E_FORMS:
                b["gossip_pull"] += e_bytes(rounds[i - 1]) + 24 * r.active_words
            else:
                upd = "gossip_scatter_store" if forms[i] == UPDATE_EDGE else "gossip_update"
                b[upd] += 24 * r.touched_words + 16 * r.active_words
        common = 8 * r.active_words + 8 * r.active_vertices + 4 * r.deg_active
        if forms[i] in (EDGE, UPDATE_EDGE):
            b["gossip_scatter_store"] += common + e_bytes(r)
        else:
            b["gossip_scatter_atomic"] += common + 16 * r.scatter_words
    if per_round:
        return rows
    return {k: sum(x[k] for x in rows) for k in KCLASS}


def survey_bytes(rounds, mode):
    """SURVEY.md 8d reference model for the whole run (gossip: 8 B per bit relay)."""
    tot = 0
    for i, r in enumerate(rounds):
        if i == 0:
            continue
        p = rounds[i - 1]
        move = 8 * (p.wedges if mode == "flood" else p.relays)
        tot += move + 8 * p.active_words + 4 * p.deg_active + 8 * p.active_vertices + 24 * r.active_words
    return tot


def survey_bytes_kernel(rounds, mode, kclass, per_round=False):
    """SURVEY.md 8d bytes of the rounds whose arrivals kernel class `kclass` consumes (the
    fused kernel pulls round r's arrivals: B_r with round r-1's relays)."""
    if mode == "flood":
        if kclass != "flood_pull":
            return [0] * len(rounds) if per_round else 0
        out = [0] + [survey_bytes(rounds[i - 1:i + 1], mode) for i in range(1, len(rounds))]
        return out if per_round else sum(out)
    forms = push_forms(rounds)
    tot = 0
    out = [0] * len(rounds)
    for i in range(1, len(rounds)):
        consumer = ("gossip_fused" if forms[i] == FUSED else
                    "gossip_pull" if forms[i - 1] in E_FORMS else
                    "gossip_scatter_store" if forms[i] == UPDATE_EDGE else "gossip_update")
        if consumer != kclass:
            continue
        p, r = rounds[i - 1], rounds[i]
        out[i] = 8 * p.relays + 8 * p.active_words + 4 * p.deg_active + 8 * p.active_vertices + 24 * r.active_words
        tot += out[i]
    return out if per_round else tot


def build_graph(w):
    from p2pnetwork.gpu import PeerGraph
    if w["graph"] == "ba":
        return PeerGraph.barabasi_albert(w["V"], int(w["a"]), seed=1)
    if w["graph"] == "gnp":
        return PeerGraph.gnp(w["V"], w["a"], seed=1)
    if w["graph"] == "rrg":
        return PeerGraph.random_regular(w["V"], int(w["a"]), seed=1)
    if w["graph"] == "ws":
        return PeerGraph.watts_strogatz(w["V"], int(w["a"]), w["beta"], seed=1)
    raise ValueError(w["graph"])


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(g, w, src, sample_msgs, thr, object_seconds=10.0):
    """Two CPU legs on a bounded sample of the same workload (reported, not a target):
    (ii) the C oracle (oracle/relay_oracle.c, OpenMP, every core of the job's affinity set) on the same graph with
    the first `sample_msgs` broadcasts -- the headline cpu_baseline value; (i) the 1-core,
    object-level Python relay (oracle/object_relay.py: Node / NodeConnection-shaped objects, JSON
    + EOT framing per send, the reference's per-relay work) on broadcast 0 until ~object_seconds
    of relays have been made (a partial broadcast: the rate per relay is what is sampled)."""
    from oracle import coracle
    from oracle.object_relay import ObjectRelay
    threads = int(os.environ.get("OMP_NUM_THREADS", "0")) or len(os.sched_getaffinity(0))
    os.environ["OMP_NUM_THREADS"] = str(threads)
    s = src[:sample_msgs]
    t0 = time.perf_counter()
    res = coracle.run(g.rowptr, g.colidx, s, w["mode"], w["fanout"], GOSSIP_SEED, 0, thr, CHURN_SEED,
                      record=False)
    dt = time.perf_counter() - t0
    relays = sum(r["relays"] for r in res.rounds)
    c_leg = {"value": relays / dt / 1e9, "unit": "GTEPS", "cores": threads, "kind": "port",
             "sample": f"{sample_msgs} of {w['M']} broadcasts on the full {w['V']}-peer graph: "
                       f"{relays} relays in {dt:.2f} s (oracle/relay_oracle.c, {threads} OpenMP threads)"}
    # object leg: calibrate the relay budget on a short run, then time ~object_seconds
    sim = ObjectRelay(g.rowptr, g.colidx, w["mode"], w["fanout"], GOSSIP_SEED, thr, CHURN_SEED)
    t0 = time.perf_counter()
    probe = sum(sim.run(src[:1], max_relays=20000))
    rate = probe / max(time.perf_counter() - t0, 1e-6)
    sim = ObjectRelay(g.rowptr, g.colidx, w["mode"], w["fanout"], GOSSIP_SEED, thr, CHURN_SEED)
    t0 = time.perf_counter()
    per_round = sim.run(src[:1], max_relays=int(rate * object_seconds))
    odt = time.perf_counter() - t0
    orel = sum(per_round)
    o_leg = {"value": orel / odt / 1e9, "unit": "GTEPS", "cores": 1, "kind": "port",
             "sample": f"broadcast 0 of {w['M']} on the full {w['V']}-peer graph, its first "
                       f"{orel} relays ({len(per_round)} rounds) in {odt:.2f} s (oracle/object_relay.py, "
                       f"1 Python thread, {len(sim.peers)} peer objects)"}
    out = dict(c_leg)
    out["cpu_model"] = cpu_model()
    # the job's CPU share: a GPU box pins a one-GPU job to its slice of the host
    out["affinity_cores"] = len(os.sched_getaffinity(0))
    out["host_cpus"] = os.cpu_count()
    out["legs"] = {"c_openmp": c_leg, "python_objects_1core": o_leg}
    return out


def load_traffic(workload, kernel):
    """HBM traffic per launch of the dominant kernel from the committed rocprofv3 PMC pass
    (profiles/traffic_<workload>.json, written by tools/pmc_traffic.py), if present."""
    p = os.path.join(REPO, "profiles", f"traffic_{workload}.json")
    if not os.path.exists(p):
        return None
    with open(p) as f:
        d = json.load(f)
    return d.get("kernels", {}).get(kernel, {}).get("bytes_per_launch")


def dump_outputs(path, net, rounds):
    """The last timed step's results as float64 .npy files under `path` (module docstring)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    tab = np.array([[getattr(r, f) for f in ROUND_FIELDS] for r in rounds], dtype=np.float64)
    np.save(os.path.join(path, "rounds.npy"), tab.reshape(len(rounds), len(ROUND_FIELDS)))
    if not hasattr(net, "seen_word"):
        return  # a vertex-partitioned rank holds its own peers' rows only: the counters stand for it
    rng = np.random.default_rng(DUMP_SEED)
    V, W = net.graph.V, net.W
    peers = np.sort(rng.choice(V, size=min(V, DUMP_PEERS), replace=False))
    # the first and the last word, and seeded ones between them
    words = np.unique(np.concatenate([[0, W - 1], rng.choice(W, size=min(W, DUMP_WORDS - 2), replace=False)]))
    sample = np.empty((len(words), len(peers), 2), dtype=np.float64)
    for i, w in enumerate(words):
        col = net.seen_word(int(w))[peers]
        sample[i, :, 0] = (col & np.uint64(0xFFFFFFFF)).astype(np.float64)
        sample[i, :, 1] = (col >> np.uint64(32)).astype(np.float64)
    np.save(os.path.join(path, "seen_peers.npy"), peers.astype(np.float64))
    np.save(os.path.join(path, "seen_words.npy"), words.astype(np.float64))
    np.save(os.path.join(path, "seen_sample.npy"), sample)


def launch_ranks(n, argv):
    """`bench.py --gpus N` started without a launcher (WORLD_SIZE unset, N > 1): run the N ranks
    as children of this process under torch.distributed.run (127.0.0.1 rendezvous) and return
    their exit code.  Nothing here touches torch or the GPU -- the children initialise it, one
    process per GPU (LOCAL_RANK = device) -- and this process only waits (no exec)."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr=127.0.0.1", f"--master-port={port}", os.path.abspath(__file__), *argv]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on this host driver
    return subprocess.run(cmd, env=env).returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="c4", choices=sorted(WORKLOADS))
    ap.add_argument("--cpu-sample-msgs", type=int, default=64)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="also what takes runs of its own: every kernel class's device time, the "
                         "dominant kernel round by round, the CPU baseline (module docstring)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's results as DIR/<name>.npy (module docstring)")
    ap.add_argument("--peers", type=int, default=0, help="override the workload's peer count "
                    "(rehearsals only; the reported workload names the size actually run)")
    ap.add_argument("--msgs", type=int, default=0, help="override the workload's broadcast count "
                    "(rehearsals only, e.g. one rank's share of a split; the reported workload names it)")
    ap.add_argument("--split", default="auto", choices=["auto", "message", "vertex"],
                    help="multi-GPU form: the workload's own (auto: c5 vertex, else message), the "
                         "message-axis split, or the 1-D vertex partition")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="gloo stages the exchange through host memory (rehearsal with several "
                         "ranks on one GPU); nccl = RCCL over xGMI")
    args = ap.parse_args()
    if args.gpus < 1:
        raise SystemExit(f"--gpus {args.gpus}: need at least one rank")
    if args.steps < 1:
        raise SystemExit(f"--steps {args.steps}: need at least one timed step")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        # a mislaunched job must not report an N = 1 (or partial) number as an N-GPU one
        raise SystemExit(f"bench.py: WORLD_SIZE={world} but --gpus {args.gpus}; launch with "
                         f"--nproc-per-node {args.gpus} or without a launcher")
    dist = None
    if world > 1:
        import torch
        import torch.distributed as dist
        ndev = torch.cuda.device_count()  # counts devices without initialising them
        if args.dist_backend == "nccl" and world > ndev:
            raise SystemExit(f"--gpus {world} with RCCL needs {world} GPUs, {ndev} visible "
                             f"(--dist-backend gloo rehearses several ranks on one GPU)")
        local = local % max(ndev, 1)  # gloo rehearsal: ranks may share a GPU
        torch.cuda.set_device(local)
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group("gloo")

    from p2pnetwork.gpu import GraphNetwork, make_sources
    from p2pnetwork.gpu.network import churn_threshold
    w = dict(WORKLOADS[args.workload])
    if args.peers:
        w["V"] = args.peers
        w["name"] += f" [REDUCED: {args.peers} peers]"
    if args.msgs:
        w["M"] = args.msgs
        w["name"] += f" [REDUCED: {args.msgs} broadcasts]"
    thr = churn_threshold(w.get("churn", 0.0))
    part_form = bool(w.get("partition")) if args.split == "auto" else args.split == "vertex"
    partitioned = part_form and world > 1
    t_gen = time.perf_counter()
    g = build_graph(w)
    t_gen = time.perf_counter() - t_gen
    M = w["M"]
    # per-launch HIP events on the engine's stream (the roofline's kernel time); P2PG_BENCH_TIMING=0
    # turns them off to measure what they cost (A/B only: the line then has no kernel times)
    timing = os.environ.get("P2PG_BENCH_TIMING", "1") != "0"
    common = dict(mode=w["mode"], fanout=w["fanout"], gossip_seed=GOSSIP_SEED, churn_threshold_value=thr,
                  churn_seed=CHURN_SEED, timing=timing, device=local)
    if partitioned:
        # one graph, vertex ranges per rank, boundary rows exchanged per round (RCCL all-to-all)
        from p2pnetwork.gpu import PartitionedNetwork, TorchTransport
        from p2pnetwork.gpu.partition import host_group_for
        src = make_sources(g.V, M, seed=1)
        # every rank makes the (collective) gloo group for the count all-gather here
        hg = host_group_for(None) if args.dist_backend == "nccl" else None
        net = PartitionedNetwork(g, world, rank,
                                 TorchTransport(device=torch.device("cuda", local), host_group=hg), **common)
    else:
        # message axis, fixed total work: rank r runs broadcasts [lo, hi) of the M (global ids,
        # so origins and Philox streams are the 1-GPU run's) on its own graph copy.  4096 split
        # into whole 64-bit words for N | 64; any other split is still exact (a rank's bit
        # positions are local, its message ids global), only the rows are ragged
        if M < world:
            raise SystemExit(f"--gpus {world}: only {M} broadcasts to split")
        lo, hi = rank * M // world, (rank + 1) * M // world
        src = make_sources(g.V, M, seed=1)[lo:hi]
        net = GraphNetwork(g, msg_id_base=lo, **common)
    net.broadcast(src)
    # (>= 2 with timing: the last one names the dominant kernel, and the first run of a process
    # carries the one-time first-launch cost -- config 3's 6.6 ms "seed" against its 5.9 ms pull)
    for _ in range(max(args.warmup, 2 if timing else 0)):
        net.reset()
        net.run()
    # the timed region brackets only the dominant kernel class with HIP events (on the engine's
    # stream): two event records per launch cost ~2.7 us of stream time each, ~0.8 ms per c4
    # step over ~300 launches; with --full the other classes are timed in an untimed step afterwards
    kt_w = net.kernel_times()
    dominant = max(KCLASS, key=lambda k: kt_w[k][0])
    if timing:
        net.set_timed_classes([dominant])

    def barrier():
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    barrier()
    net.reset()  # zero the kernel timers; state re-zeroed again per step below
    kt0 = net.kernel_times()
    t0 = time.perf_counter()
    relays = 0
    all_rounds = []
    for _ in range(args.steps):
        net.reset()
        rounds = net.run()
        relays += sum(r.relays for r in rounds)
        all_rounds.append(rounds)
    barrier()
    elapsed = time.perf_counter() - t0
    kt = net.kernel_times()  # reset() zeroes the timers: this is the LAST step's kernels
    if dist is not None:
        import torch
        red = f"cuda:{local}" if args.dist_backend == "nccl" else "cpu"
        t = torch.tensor([elapsed], dtype=torch.float64, device=red)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        if not partitioned:  # message split: sum the ranks' relays (partitioned counters are global)
            r = torch.tensor([relays], dtype=torch.float64, device=red)
            dist.all_reduce(r, op=dist.ReduceOp.SUM)
            relays = int(r.item())
    del kt0

    last = all_rounds[-1]
    local_last = net.local_rounds if partitioned else last  # this rank's kernels' work
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, net, last)  # before anything below runs the engine again
    W_local = (len(src) + 63) // 64 if not partitioned else (M + 63) // 64
    mb = model_bytes(local_last, w["mode"], W_local)
    dom_ms, dom_n = kt[dominant]  # the last timed step's dominant launches (live HIP events)
    kt_all = None
    if args.full:
        # every class's device time: one more (untimed) step with all classes bracketed
        net.set_timed_classes(None)
        net.reset()
        net.run()
        kt_all = net.kernel_times()
        if dist is not None:
            dist.barrier()
    traffic = load_traffic(args.workload, dominant)
    sb_step = survey_bytes(local_last, w["mode"])
    sb_dom = survey_bytes_kernel(local_last, w["mode"], dominant)
    # achieved = SURVEY.md 8(d)'s algorithmic bytes (B_r; gossip: 8 B per bit relay) of the rounds
    # whose arrivals the dominant kernel consumes, over its HIP-event time; the engine's own
    # per-kernel byte model is reported beside it
    achieved = sb_dom / (dom_ms * 1e-3) / 1e9 if dom_ms > 0 else 0.0
    achieved_engine = mb[dominant] / (dom_ms * 1e-3) / 1e9 if dom_ms > 0 else 0.0
    kernel_ms_total = sum(v[0] for v in kt_all.values()) if kt_all is not None else None
    # per-round honesty: the SURVEY model charges 8 B per BIT relay, which in the peak gossip
    # rounds implies more than the HBM peak -- those rounds are listed, not averaged away; the
    # engine model (8 B per packed E word) and the PMC counter bytes stay physically bounded
    sb_rounds = survey_bytes_kernel(local_last, w["mode"], dominant, per_round=True)
    mb_rounds = [x[dominant] for x in model_bytes(local_last, w["mode"], W_local, per_round=True)]
    by_round = None
    if args.full and w["mode"] == "gossip" and world == 1:
        # untimed: one more broadcast stepped round by round, the dominant kernel's device time
        # per round (a change of the dense-round schedule cannot pass for kernel speed); stepping
        # stores every round's frontier, which p2pg_run skips where nobody reads it
        net.reset()
        by_round = []
        while True:
            k0 = net.kernel_times()[dominant][0]
            st = net.step()
            by_round.append(round(net.kernel_times()[dominant][0] - k0, 3))
            if not st.active:
                break
    round_fracs = None
    if by_round is not None:
        round_fracs = []
        for i, ms in enumerate(by_round):
            if ms <= 0 or i >= len(sb_rounds):
                continue
            fs = sb_rounds[i] / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS
            fe = mb_rounds[i] / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS
            round_fracs.append({"round": i, "ms": ms, "survey_GB": round(sb_rounds[i] / 1e9, 2),
                                "engine_GB": round(mb_rounds[i] / 1e9, 2), "frac_survey": round(fs, 3),
                                "frac_engine": round(fe, 3), "survey_exceeds_peak": fs > 1.0})
    out = {
        "metric": "msg-edge relays/sec (GTEPS) at 10M peers x 4096 msgs; % HBM roofline",
        "value": relays / elapsed / 1e9,
        "unit": "GTEPS",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "u64",
        "data": "synthetic (generated graph + Philox origins)",
        "config": {"workload": w["name"], "peers": g.V, "edges": g.n_edges,
                   "broadcasts": M,
                   "mode": w["mode"], "fanout": w["fanout"], "churn": w.get("churn", 0.0),
                   "rounds": len(last),
                   "parallelism": (f"vertex partition x{world} (RCCL all-to-all of boundary rows)"
                                   if partitioned else
                                   f"message-axis split x{world} ({M // world} broadcasts per rank)"
                                   if world > 1 else "single GPU")},
        "roofline": {
            "bound": "hbm",
            "kernel": dominant,
            "achieved": achieved,
            "peak": HBM_PEAK_GBPS,
            "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBPS,
            "traffic": traffic,
            "algorithmic_bytes_per_launch": sb_dom / max(dom_n, 1),
            "model": "SURVEY.md 8(d) B_r",
            "avg_launch_ms": dom_ms / max(dom_n, 1),
            "launches_per_step": dom_n,
            # the engine's per-kernel model (8 B per packed E word stored / gathered)
            "frac_engine_model": achieved_engine / HBM_PEAK_GBPS,
            "engine_model_bytes_per_launch": mb[dominant] / max(dom_n, 1),
            # the PMC byte counters of the committed profile (profiles/traffic_<workload>.json)
            # over this launch time: what the memory system actually moved
            "frac_counter": (traffic / (dom_ms / max(dom_n, 1) * 1e-3) / 1e9 / HBM_PEAK_GBPS
                             if traffic and dom_ms > 0 else None),
            # rounds whose SURVEY bytes imply more than the HBM peak (the model overcounts there)
            "survey_rounds_over_peak": ([x["round"] for x in round_fracs if x["survey_exceeds_peak"]]
                                        if round_fracs is not None else None),
        },
        "timing_mode": ("HIP events around the dominant kernel class only inside the timed region "
                        "(p2pg_set_timed_classes); kernel_ms_per_step (--full) from one untimed step with "
                        "every class bracketed (round 5 on; earlier rounds bracketed every class)"),
        "dominant_round_fracs": round_fracs,
        # (--full: an untimed step after the timed region, every class bracketed by events)
        "kernel_ms_per_step": {k: v[0] for k, v in kt_all.items()} if kt_all is not None else None,
        "dominant_ms_by_round": by_round,
        "model_bytes_per_step": mb,
        "whole_step_model_GBps": sum(mb.values()) / (elapsed / args.steps) / 1e9,
        "survey_model_bytes_per_step": sb_step,
        "whole_step_frac_survey_model": sb_step / (elapsed / args.steps) / 1e9 / HBM_PEAK_GBPS,
        "kernel_time_frac_of_step": (kernel_ms_total / (elapsed / args.steps * 1e3)
                                     if kernel_ms_total is not None else None),
        "relays_per_step": relays // args.steps,
        # arrivals (sum of message_count_recv, nodeconnection.py:215): relays less churn losses;
        # a churn run counts its losses only with count_received (a counting pass per round,
        # not part of the relay): there the sends of each round before, as an upper bound
        "received_per_step": sum(r.received for r in last),
        "received_exact": all(r.received_exact for r in last),
        "relays_per_step_per_gpu": relays / args.steps / world,
        "exchange_ms_per_step": (net.exchange_s * 1e3) if partitioned else 0.0,
        # compacted exchange: fraction of the boundary rows that had a non-zero word and travelled
        "exchange_live_row_frac": (net.transport.rows_sent / max(net.transport.rows_total, 1))
        if partitioned else None,
        "graph_gen_s": t_gen,
    }
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(g, w, src, args.cpu_sample_msgs, thr)
    net.close()
    if rank == 0:
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
