"""Numpy restatement of the relay policy (test infrastructure only).

Peer v carries a uint32 threshold thr[v]: 0 relays every first receipt, 0xFFFFFFFF none (neither
draws), and otherwise the first receipt of message m at v in round r is muted iff

    philox4x32_10(ctr = (r, v, msg_id_base + m, 'RLY'), key = (seed_lo, seed_hi)).x < thr[v].

A muted receipt happens and sends nothing -- tests/drop_ref.py's rule for a dropped receipt, so the
policy is a drop callback for drop_ref.run: ``new & ~(start == r)[None, :] & muted(r, v, m)``
(originations are the app's own send_to_nodes and exempt; round 0 holds nothing else).  Pinned to
the reference's own Node objects by tests/golden/policy/*.npz (tests/test_policy.py); draws through
oracle.philox.
"""
import numpy as np

from oracle import philox

TAG_RLY = 0x00524C59  # 'RLY'
SILENT = 0xFFFFFFFF


def muted(rnd, peer, msg, thr, seed):
    """The draw, vectorised: rnd, peer, msg (global id) and thr broadcast; returns bool."""
    rnd, peer, msg, thr = np.broadcast_arrays(np.asarray(rnd, dtype=np.int64), np.asarray(peer, dtype=np.int64),
                                              np.asarray(msg, dtype=np.int64), np.asarray(thr, dtype=np.uint64))
    seed = int(seed)
    x, _, _, _ = philox.philox4x32_10(rnd, peer, msg, TAG_RLY, np.uint64(seed & 0xFFFFFFFF),
                                      np.uint64((seed >> 32) & 0xFFFFFFFF))
    return np.where(thr == 0, False, np.where(thr == SILENT, True, x < thr))


def muted_plane(r, thr, M, seed, msg_id_base=0):
    """bool [V, M]: would a first receipt of (v, m) in round r be muted?"""
    thr = np.asarray(thr, dtype=np.uint64)
    v = np.arange(len(thr), dtype=np.int64)[:, None]
    m = np.arange(M, dtype=np.int64)[None, :] + int(msg_id_base)
    return muted(r, v, m, thr[:, None], seed)


def policy_rule(thr, seed, start, msg_id_base=0):
    """The relay policy as a drop_ref callback."""
    thr = np.asarray(thr, dtype=np.uint64)
    start = np.asarray(start, dtype=np.int64)

    def rule(r, new):
        # (the draws of the first receipts only: muted_plane, evaluated where it is asked)
        gone = np.zeros_like(new)
        v, m = np.nonzero(new & ~(start == r)[None, :] & (thr != 0)[:, None])
        gone[v, m] = muted(r, v, m + int(msg_id_base), thr[v], seed)
        return gone
    return rule


def with_ttl(rule, start, ttl):
    """The policy and hop limits together: a receipt sends iff it is neither expired nor muted."""
    start, ttl = np.asarray(start, dtype=np.int64), np.asarray(ttl, dtype=np.int64)
    return lambda r, new: rule(r, new) | (new & (r - start == ttl)[None, :])


def thresholds(relay_prob, V):
    """GraphNetwork.relay_thresholds, restated."""
    q = np.broadcast_to(np.asarray(relay_prob, dtype=np.float64), (V,))
    t = np.clip(np.floor((1.0 - q) * 4294967296.0), 1.0, float(0xFFFFFFFE))
    t = np.where(q == 1.0, 0.0, np.where(q == 0.0, float(SILENT), t))
    return t.astype(np.uint32)
