"""Host reference of the run tallies (include/p2pgpu.h p2pg_message_tally / p2pg_peer_counters),
from the hop / parent planes of a finished run.  NumPy and the oracle's Philox only; it restates
the send set of tests/partition_mock.py MockEngine.sends() for every first receipt of a run at
once, and is itself pinned against oracle.object_relay and the reference-made fixture counters
by tests/test_tally.py."""
import numpy as np

from oracle import philox


def message_tally(hop):
    """(reach, hop_sum, last_hop) per message from a hop plane [V][M] (-1 = not delivered)."""
    got = hop >= 0
    reach = got.sum(0).astype(np.uint64)
    hop_sum = np.where(got, hop, 0).astype(np.int64).sum(0).astype(np.uint64)
    last_hop = hop.max(0).astype(np.int32) if hop.shape[0] else np.full(hop.shape[1], -1, np.int32)
    return reach, hop_sum, last_hop


def round_sends(hop, parent, rowptr, colidx, mode, k=3, gossip_seed=0, churn_threshold=0, churn_seed=0,
                msg_id_base=0):
    """Every send of the run as arrays (round, sender, receiver, lost): per first receipt (v, m)
    at hop r -- flood: every connection but the parent (all of them at the origin); gossip: all
    connections when deg <= k, else philox.gossip_picks; lost per philox.churn_dropped."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colidx = np.asarray(colidx, dtype=np.int64)
    deg = np.diff(rowptr)
    vs, ms = np.nonzero(hop >= 0)
    r = hop[vs, ms].astype(np.int64)
    par = parent[vs, ms].astype(np.int64)
    d = deg[vs]
    if mode == "flood":
        alln = np.ones(len(vs), dtype=bool)
    else:
        alln = d <= k
    # receipts sent over every connection (flood: less the parent's)
    i = np.nonzero(alln & (d > 0))[0]
    rep = np.repeat(i, d[i])
    off = np.arange(len(rep)) - np.repeat(np.cumsum(d[i]) - d[i], d[i])
    u = colidx[rowptr[vs[rep]] + off]
    keep = np.ones(len(rep), dtype=bool)
    if mode == "flood":
        keep = (r[rep] == 0) | (u != par[rep])
    rnd, snd, rcv = [r[rep][keep]], [vs[rep][keep]], [u[keep]]
    # gossip receipts with more connections than the fanout: the Philox picks
    j = np.nonzero(~alln)[0]
    if len(j):
        pk = philox.gossip_picks(r[j], vs[j], ms[j] + msg_id_base, d[j], k, gossip_seed)
        rnd.append(np.repeat(r[j], k))
        snd.append(np.repeat(vs[j], k))
        rcv.append(colidx[(rowptr[vs[j]][:, None] + pk).ravel()])
    rnd, snd, rcv = np.concatenate(rnd), np.concatenate(snd), np.concatenate(rcv)
    lost = np.asarray(philox.churn_dropped(rnd, snd, rcv, int(churn_threshold), int(churn_seed)), dtype=bool)
    return rnd, snd, rcv, lost


def peer_counters(hop, parent, rowptr, colidx, mode, k=3, gossip_seed=0, churn_threshold=0, churn_seed=0,
                  msg_id_base=0):
    """(sent, received) uint64 [V]: Node.message_count_send / message_count_recv of the run."""
    V = len(rowptr) - 1
    _, snd, rcv, lost = round_sends(hop, parent, rowptr, colidx, mode, k, gossip_seed, churn_threshold,
                                    churn_seed, msg_id_base)
    sent = np.bincount(snd, minlength=V).astype(np.uint64)
    received = np.bincount(rcv[~lost], minlength=V).astype(np.uint64)
    return sent, received


def of_fixture(z):
    """peer_counters of a static golden fixture."""
    return peer_counters(z["hop"], z["parent"], z["rowptr"], z["colidx"], str(z["mode"]), int(z["fanout"]),
                         int(z["gossip_seed"]), int(z["churn_threshold"]), int(z["churn_seed"]))
