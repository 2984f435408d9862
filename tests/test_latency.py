"""CPU: the delivery-latency interface (include/p2pgpu.h P2PG_FLAG_LATENCY, p2pg_message_latency /
p2pg_peer_latency) is declared, and the host reference the GPU tests compare against
(tests/latency_ref.py) keeps its identities on the hop planes the reference's own Node objects
produced -- every fixture under tests/golden/ with a 2-D hop plane, static and feature fixtures
alike -- against tests/tally_ref.py, plus the Python layer's curve / percentile arithmetic."""
import os
import re

import numpy as np
import pytest

import latency_ref
import tally_ref
from conftest import GOLDEN, REPO
from p2pnetwork.gpu import GraphNetwork, PeerLatency, _lib


def _hop_fixtures():
    out = []
    for root, _, files in os.walk(GOLDEN):
        for f in sorted(files):
            if not f.endswith(".npz"):
                continue
            path = os.path.join(root, f)
            with np.load(path, allow_pickle=False) as z:
                if "hop" in z.files and z["hop"].ndim == 2:
                    out.append(os.path.relpath(path, GOLDEN)[:-4])
    return sorted(out)


HOP_FIXTURES = _hop_fixtures()


def load(rel):
    with np.load(os.path.join(GOLDEN, rel + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def test_header_declares_the_latency_interface():
    text = open(os.path.join(REPO, "include", "p2pgpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define\s+P2PG_FLAG_LATENCY\s+128u", code)
    assert re.search(r"\bint\s+p2pg_set_latency_bins\s*\(\s*p2pg_engine\s*\*\s*e\s*,\s*int32_t\s+bins\s*\)", code)
    assert re.search(r"\bint\s+p2pg_message_latency\s*\(\s*p2pg_engine\s*\*\s*e\s*,\s*int32_t\s+bins\s*,"
                     r"\s*uint64_t\s*\*\s*hist\s*\)", code)
    assert re.search(r"\bint\s+p2pg_peer_latency\s*\(\s*p2pg_engine\s*\*\s*e\s*,\s*uint64_t\s*\*\s*hop_sum\s*,"
                     r"\s*uint32_t\s*\*\s*receipts\s*,\s*int32_t\s*\*\s*max_hop\s*\)", code)
    for name in ("p2pg_set_latency_bins", "p2pg_message_latency", "p2pg_peer_latency"):
        assert name in _lib.SIGNATURES
    assert _lib.FLAG_LATENCY == 128
    for anchor in ("node.py:334-338", "README.md:20"):
        assert anchor in text[text.index("delivery latency (P2PG_FLAG_LATENCY)"):text.index("int p2pg_set_latency_bins")]


def test_fixture_inventory():
    kinds = {os.path.dirname(f) for f in HOP_FIXTURES}
    assert {"", "late", "ttl", "policy", "down", "pull"} <= kinds
    assert len(HOP_FIXTURES) >= 30
    largest, starts = 0, 0
    for rel in HOP_FIXTURES:
        z = load(rel)
        r = latency_ref.relative(z["hop"], latency_ref.start_of(z))
        largest = max(largest, int(r.max()))
        starts = max(starts, int(latency_ref.start_of(z).max()))
    # at bins = 64 no fixture reaches the last bin; the start planes of the feature fixtures: 7
    assert largest == 43
    assert starts == 100 and starts.bit_length() == 7


@pytest.mark.parametrize("rel", HOP_FIXTURES)
def test_identities_on_reference_made_hop_planes(rel):
    z = load(rel)
    hop, start = z["hop"], latency_ref.start_of(z)
    V, M = hop.shape
    lat = latency_ref.latency(hop, start)
    reach, hop_sum, last_hop = tally_ref.message_tally(hop)
    assert lat.hist.shape == (M, 64) and lat.hist.dtype == np.uint64
    assert lat.hop_sum.dtype == np.uint64 and lat.receipts.dtype == np.uint32 and lat.max_hop.dtype == np.int32
    b = np.arange(64, dtype=np.int64)
    np.testing.assert_array_equal(lat.hist.sum(axis=1), reach)
    assert int(lat.receipts.sum()) == int(reach.sum())
    assert not lat.hist[:, -1].any()  # (largest relative hop 43: nothing is clamped)
    weighted = (lat.hist.astype(np.int64) * b[None, :]).sum(axis=1)
    assert int(lat.hop_sum.sum()) == int(weighted.sum())
    np.testing.assert_array_equal(weighted, hop_sum.astype(np.int64) - start * reach.astype(np.int64))
    top = np.array([np.nonzero(row)[0][-1] if row.any() else -1 for row in lat.hist])
    np.testing.assert_array_equal(top, np.where(reach > 0, last_hop - start, -1))
    np.testing.assert_array_equal(lat.max_hop >= 0, lat.receipts > 0)
    assert int(lat.max_hop.max()) == int(top.max())
    # the curve ends at 1, the percentiles are monotone and end at the highest bin
    cov = latency_ref.coverage_curve(lat.hist)
    assert np.isnan(cov[reach == 0]).all() and (cov[reach > 0, -1] == 1.0).all()
    p50, p100 = latency_ref.percentile(lat.hist, 0.5), latency_ref.percentile(lat.hist, 1.0)
    np.testing.assert_array_equal(p100, top)
    assert (p50 <= p100).all() and (p50[reach == 0] == -1).all()


def test_path_graph_flooded_from_peer_0_with_start_2():
    hop = np.array([[2], [3], [4], [5]], dtype=np.int32)  # 0-1-2-3, origin 0, start 2
    lat = latency_ref.latency(hop, [2], bins=64)
    want = np.zeros((1, 64), dtype=np.uint64)
    want[0, :4] = 1
    np.testing.assert_array_equal(lat.hist, want)
    np.testing.assert_array_equal(lat.hop_sum, [0, 1, 2, 3])
    np.testing.assert_array_equal(lat.receipts, [1, 1, 1, 1])
    np.testing.assert_array_equal(lat.max_hop, [0, 1, 2, 3])
    np.testing.assert_array_equal(latency_ref.percentile(lat.hist, 0.5), [1])
    np.testing.assert_array_equal(latency_ref.percentile(lat.hist, 0.51), [2])
    np.testing.assert_array_equal(latency_ref.coverage_curve(lat.hist)[0, :5], [0.25, 0.5, 0.75, 1.0, 1.0])
    np.testing.assert_array_equal(latency_ref.coverage_curve(lat.hist, V=8)[0, :5], [0.125, 0.25, 0.375, 0.5, 0.5])
    # read after round 3: peers 0 and 1 only; an unreached peer has no receipt
    part = latency_ref.latency(hop, [2], upto=3)
    np.testing.assert_array_equal(part.receipts, [1, 1, 0, 0])
    np.testing.assert_array_equal(part.max_hop, [0, 1, -1, -1])
    np.testing.assert_array_equal(latency_ref.mean(part)[:2], [0.0, 1.0])
    assert np.isnan(latency_ref.mean(part)[2:]).all()


def test_last_bin_hit_without_clamping():
    z = load("late/late_rrg200_flood")
    rel = latency_ref.relative(z["hop"], z["start"])
    assert int(rel.max()) == 7
    lat8, lat64 = latency_ref.latency(z["hop"], z["start"], bins=8), latency_ref.latency(z["hop"], z["start"])
    assert lat8.hist[:, 7].any()
    np.testing.assert_array_equal(lat8.hist, lat64.hist[:, :8])
    for a, b in zip(lat8[1:], lat64[1:]):
        np.testing.assert_array_equal(a, b)


def test_last_bin_collects_the_overflow():
    z = load("late/late_ba300_gossip_k2_churn10")
    rel = latency_ref.relative(z["hop"], z["start"])
    assert int(rel.max()) == 43
    lat8, lat64 = latency_ref.latency(z["hop"], z["start"], bins=8), latency_ref.latency(z["hop"], z["start"])
    np.testing.assert_array_equal(lat8.hist[:, :7], lat64.hist[:, :7])
    np.testing.assert_array_equal(lat8.hist[:, 7], lat64.hist[:, 7:].sum(axis=1))
    assert (lat8.hist[:, 7] > lat64.hist[:, 7]).any()
    for a, b in zip(lat8[1:], lat64[1:]):  # the per-peer arrays do not depend on bins
        np.testing.assert_array_equal(a, b)
    # a percentile that lands in the last bin is a lower bound of the exact one
    p8, p64 = latency_ref.percentile(lat8.hist, 0.99), latency_ref.percentile(lat64.hist, 0.99)
    np.testing.assert_array_equal(p8, np.minimum(p64, 7))
    assert (p64 > 7).any()


class _HostOnly(GraphNetwork):
    """The Python layer's host arithmetic over a given histogram plane (no engine)."""

    def __init__(self, hist, V):
        self._hist = hist
        self.graph = type("G", (), {"V": V})()
        self.sources = np.zeros(len(hist), dtype=np.int32)
        self._h = None

    def message_latency(self):
        return self._hist


@pytest.mark.parametrize("rel,bins", [("late/late_ba300_gossip_k2_churn10", 8), ("pull/pull_rrg200_flood", 64)])
def test_python_curve_and_percentile_are_the_references(rel, bins):
    z = load(rel)
    start = z["start"].copy()
    hop = z["hop"].copy()
    hop[:, 1] = -1  # a broadcast that reached nobody: an unscheduled one
    lat = latency_ref.latency(hop, start, bins=bins)
    net = _HostOnly(lat.hist, hop.shape[0])
    for of, V in (("reach", None), ("peers", hop.shape[0])):
        got, want = net.coverage_curve(of=of), latency_ref.coverage_curve(lat.hist, V)
        assert got.dtype == np.float64 and got.shape == (hop.shape[1], bins)
        np.testing.assert_array_equal(got, want)
        assert np.isnan(got[1]).all()
    for q in (0.01, 0.5, 0.9, 0.99, 1.0):
        got = net.latency_percentile(q)
        assert got.dtype == np.int32 and got[1] == -1
        np.testing.assert_array_equal(got, latency_ref.percentile(lat.hist, q))
    for bad in (0.0, 1.5):
        with pytest.raises(ValueError):
            net.latency_percentile(bad)
    with pytest.raises(ValueError):
        net.coverage_curve(of="all")
    p = PeerLatency(lat.hop_sum, lat.receipts, lat.max_hop)
    np.testing.assert_array_equal(p.mean(), latency_ref.mean(lat))
