"""Host reference of the delivery latency (include/p2pgpu.h P2PG_FLAG_LATENCY), numpy only: from a
hop plane [V][M] (absolute round of every first receipt, -1 = not delivered) and the broadcasts'
start rounds, the per-message histograms of relative hops, the per-peer sums, and the curve and
percentile the Python layer derives from the histograms.  Pinned by tests/test_latency.py."""
from collections import namedtuple

import numpy as np

Latency = namedtuple("Latency", "hist hop_sum receipts max_hop")


def start_of(z):
    """The start rounds of a fixture (the static ones start everything in round 0)."""
    M = z["hop"].shape[1]
    return z["start"].astype(np.int64) if "start" in z else np.zeros(M, dtype=np.int64)


def relative(hop, start):
    """int64 [V][M]: hop - start where delivered, -1 elsewhere."""
    hop = np.asarray(hop, dtype=np.int64)
    rel = hop - np.asarray(start, dtype=np.int64)[None, :]
    assert (rel[hop >= 0] >= 0).all(), "a receipt before its broadcast's start"
    return np.where(hop >= 0, rel, -1)


def latency(hop, start, bins=64, upto=None):
    """Latency(hist uint64 [M][bins], hop_sum uint64 [V], receipts uint32 [V], max_hop int32 [V]);
    upto = r: only the receipts of the rounds <= r (a run read after round r)."""
    hop = np.asarray(hop, dtype=np.int64)
    if upto is not None:
        hop = np.where(hop <= upto, hop, -1)
    rel = relative(hop, start)
    got = rel >= 0
    V, M = rel.shape
    vs, ms = np.nonzero(got)
    hist = np.bincount(ms * bins + np.minimum(rel[vs, ms], bins - 1), minlength=M * bins)
    hist = hist.astype(np.uint64).reshape(M, bins)
    hop_sum = np.where(got, rel, 0).sum(axis=1).astype(np.uint64)
    receipts = got.sum(axis=1).astype(np.uint32)
    max_hop = rel.max(axis=1, initial=-1).astype(np.int32)
    return Latency(hist, hop_sum, receipts, max_hop)


def mean(lat):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(lat.receipts > 0, lat.hop_sum.astype(np.float64) / lat.receipts.astype(np.float64), np.nan)


def coverage_curve(hist, V=None):
    """float64 [M][bins]: cumsum over the final reach (V given: over the number of peers)."""
    cum = np.cumsum(hist, axis=1, dtype=np.uint64).astype(np.float64)
    reach = cum[:, -1]
    out = np.full(cum.shape, np.nan)
    for m in range(len(hist)):
        if reach[m] > 0:
            out[m] = cum[m] / (reach[m] if V is None else float(V))
    return out


def percentile(hist, q):
    """int32 [M]: the smallest b with cumsum(hist)[m][b] >= ceil(q * reach[m]); -1 for reach 0."""
    out = np.full(len(hist), -1, dtype=np.int32)
    for m, row in enumerate(hist):
        cum = np.cumsum(row.astype(np.int64))
        if cum[-1] == 0:
            continue
        need = int(np.ceil(q * float(cum[-1])))
        out[m] = int(np.nonzero(cum >= need)[0][0])
    return out
