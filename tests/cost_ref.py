"""Host reference of the per-broadcast cost (include/p2pgpu.h p2pg_message_cost): sent[m] = the
send_to_node calls that carried message m, received[m] = those of them that were not lost.  NumPy
and the oracle's Philox only.  Two routes: message_cost bins per-round send lists (down_ref /
pull_ref runs, GraphNetwork.sends()); plane_cost restates tally_ref.round_sends with the message
kept, for plain runs known by their hop / parent planes.  Pinned against oracle.object_relay and
the reference-made fixture totals by tests/test_cost.py."""
import numpy as np

from oracle import philox

BLOCK = 64  # messages per pass of plane_cost (M = 4096 then needs no [receipts x connections] giant)


def message_cost(sends, M, removed=None):
    """(sent, received) uint64 [M] of a run given as its per-round send lists: sends[r] = (sender,
    receiver, msg, lost) arrays, the shape down_ref.run(...).sends and pull_ref.run(...).sends
    have, or what GraphNetwork.sends() returned after each step.  removed: {r: pairs} -- connections removed
    after round r while its sends were in flight; a send of round r over one of them, in either
    direction, is lost as well."""
    removed = removed or {}
    sent = np.zeros(M, dtype=np.uint64)
    received = np.zeros(M, dtype=np.uint64)
    for r, rec in enumerate(sends):
        if hasattr(rec, "sender"):  # GraphNetwork.sends()
            rec = (rec.sender, rec.receiver, rec.msg, rec.lost)
        snd, rcv, msg, lost = (np.asarray(x) for x in rec)
        lost = lost.astype(bool).copy()
        cut = np.asarray(removed.get(r, ()), dtype=np.int64).reshape(-1, 2)
        if len(cut) and len(snd):
            gone = set(map(tuple, cut.tolist())) | set(map(tuple, cut[:, ::-1].tolist()))
            lost |= np.array([(a, b) in gone for a, b in zip(snd.tolist(), rcv.tolist())], dtype=bool)
        sent += np.bincount(msg, minlength=M).astype(np.uint64)
        received += np.bincount(msg[~lost], minlength=M).astype(np.uint64)
    return sent, received


def _block_sends(hop, parent, m0, rowptr, colidx, deg, mode, k, gossip_seed, msg_id_base):
    """(round, sender, receiver, msg) of every send of the messages m0 .. m0 + hop.shape[1] - 1:
    per first receipt (v, m) at hop r -- flood: every connection but the parent (all of them at the
    origin); gossip: all connections when deg <= k, else philox.gossip_picks."""
    vs, ms = np.nonzero(hop >= 0)
    r = hop[vs, ms].astype(np.int64)
    par = parent[vs, ms].astype(np.int64)
    ms = ms.astype(np.int64) + m0
    d = deg[vs]
    alln = np.ones(len(vs), dtype=bool) if mode == "flood" else d <= k
    i = np.nonzero(alln & (d > 0))[0]
    rep = np.repeat(i, d[i])
    off = np.arange(len(rep)) - np.repeat(np.cumsum(d[i]) - d[i], d[i])
    u = colidx[rowptr[vs[rep]] + off]
    keep = np.ones(len(rep), dtype=bool)
    if mode == "flood":
        keep = (r[rep] == 0) | (u != par[rep])
    rnd, snd, rcv, msg = [r[rep][keep]], [vs[rep][keep]], [u[keep]], [ms[rep][keep]]
    j = np.nonzero(~alln)[0]
    if len(j):
        pk = philox.gossip_picks(r[j], vs[j], ms[j] + msg_id_base, d[j], k, gossip_seed)
        rnd.append(np.repeat(r[j], k))
        snd.append(np.repeat(vs[j], k))
        rcv.append(colidx[(rowptr[vs[j]][:, None] + pk).ravel()])
        msg.append(np.repeat(ms[j], k))
    return np.concatenate(rnd), np.concatenate(snd), np.concatenate(rcv), np.concatenate(msg)


def plane_cost(hop, parent, rowptr, colidx, mode, k=3, gossip_seed=0, churn_threshold=0, churn_seed=0,
               msg_id_base=0):
    """(sent, received) uint64 [M] of a plain run (round-0 starts, no hop limit, policy, downtime,
    anti-entropy or topology change) from its hop / parent planes [V][M]; lost per
    philox.churn_dropped."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colidx = np.asarray(colidx, dtype=np.int64)
    deg = np.diff(rowptr)
    M = hop.shape[1]
    sent = np.zeros(M, dtype=np.uint64)
    received = np.zeros(M, dtype=np.uint64)
    for m0 in range(0, M, BLOCK):
        rnd, snd, rcv, msg = _block_sends(hop[:, m0:m0 + BLOCK], parent[:, m0:m0 + BLOCK], m0, rowptr, colidx, deg,
                                          mode, int(k), int(gossip_seed), int(msg_id_base))
        lost = np.asarray(philox.churn_dropped(rnd, snd, rcv, int(churn_threshold), int(churn_seed)), dtype=bool)
        lost = np.broadcast_to(lost, rnd.shape)
        sent += np.bincount(msg, minlength=M).astype(np.uint64)
        received += np.bincount(msg[~lost], minlength=M).astype(np.uint64)
    return sent, received


def of_fixture(z):
    """plane_cost of a static golden fixture."""
    return plane_cost(z["hop"], z["parent"], z["rowptr"], z["colidx"], str(z["mode"]), int(z["fanout"]),
                      int(z["gossip_seed"]), int(z["churn_threshold"]), int(z["churn_seed"]))
