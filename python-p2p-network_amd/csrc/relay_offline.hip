// Peer downtime (p2pg_set_downtime): peer v is offline in the rounds
// [from[v], until[v]).  Its neighbours have no failure detector and go on sending to it; a send
// addressed to a peer that is offline in the round it would arrive in is counted by its sender and
// lost, like a send over a broken link (node.py:116 counts before sending).  So an offline peer
// has no first receipts, and therefore sends nothing.
//
// The receive passes know nothing of this.  In a round r in which somebody is offline the engine
// runs the receive pass the plan chose (flood pull, gossip update or gossip pull), then this
// kernel, then everything else (originations, records, tallies, hop limits, relay policy, the
// push): k_offline undoes the first receipts the pass made at the offline peers, so the passes
// after it see only receipts that happened.  Per offline active peer v and word w, with
// f = F[r&1][v][w] (= arrivals & ~seen before the round, so the undo is exact):
//   seen[v][w] &= ~f, F[r&1][v][w] = 0, v leaves A[r&1] and S (a row that filled in this round is
//   no longer full); AW is valid under the A bit only and needs nothing;
//   the round's counters lose what the receive pass counted for v.
// The peer may still get the message later from another copy: an ordinary first receipt of that
// later round.  An engine without a downtime never launches this.  Internal; not part of the
// C-ABI.
#include "device_util.h"

namespace p2pg {
namespace {

// One wave per 32-peer task of A[r&1], lane = word of a 64-word slice of the active peer's row
// (a slice loop covers W > 64).  The task's A and S words are plain stores by the wave that owns
// the task, as in k_policy.  No LDS, no scratch, no global atomics but the counter adds.
__global__ __launch_bounds__(256) void k_offline(DevGraph g, DevState st, RoundParams p, Downtime d) {
  const int lane = threadIdx.x & 63;
  const int cur = p.round & 1;
  const int W = st.W;
  const int nslices = (W + 63) >> 6;
  const int64_t ntasks = (g.V + 31) >> 5;
  // this lane's share of what leaves the round's counters
  uint64_t c_new = 0, c_relays = 0, c_av = 0, c_aw = 0, c_wedges = 0, c_deg = 0;
  for (int64_t task = (int64_t)blockIdx.x * WPB + wave_in_block(); task < ntasks;
       task += (int64_t)gridDim.x * WPB) {
    const uint32_t aw0 = st.A[cur][task];
    uint32_t aw = aw0, undone = 0;
    while (aw) {
      const int b = __builtin_ctz(aw);
      aw &= aw - 1u;
      const int64_t v = (task << 5) + b;
      if (v >= g.V) break;
      const int32_t from = ldc(d.from + v);
      if (from < 0) continue;  // never offline
      if (!downtime::offline(p.round, from, ldc(d.until + v))) continue;
      const uint64_t deg = (uint64_t)(g.rowptr[v + 1] - g.rowptr[v]);
      // relays per first receipt, as the receive passes counted them (never an origination's deg:
      // there is none at an offline peer)
      const uint64_t per = p.mode == 0 ? (deg > 0 ? deg - 1 : 0)
                                       : (deg < (uint64_t)p.fanout ? deg : (uint64_t)p.fanout);
      for (int sl = 0; sl < nslices; ++sl) {
        const int w = sl * 64 + lane;
        if (w >= W) continue;
        const int64_t i = v * W + w;
        const uint64_t f = st.F[cur][i];
        if (!f) continue;
        st.seen[i] &= ~f;
        st.F[cur][i] = 0ull;
        const uint64_t bits = (uint64_t)__popcll(f);
        c_new += bits;
        c_relays += bits * per;
        c_aw += 1;
        c_wedges += deg;
      }
      undone |= 1u << b;
      if (lane == 0) {
        c_av += 1;
        c_deg += deg;
      }
    }
    if (undone && lane == 0) {
      st.A[cur][task] = aw0 & ~undone;
      st.S[task] &= ~undone;
    }
  }
  // the counters are read as differences modulo 2^64 (engine.cpp, read_stats): adding -t takes t
  // out of this round's total
  unsigned long long* const shard = st.stats + (blockIdx.x & (STAT_SHARDS - 1)) * STAT_N;
  auto take = [&](int idx, uint64_t x) {
    const uint64_t t = wave_sum(x);
    if (lane == 0 && t) atomicAdd(shard + idx, 0ull - (unsigned long long)t);
  };
  take(ST_NEW, c_new);
  take(ST_RELAYS, c_relays);
  take(ST_ACTIVE_V, c_av);
  take(ST_ACTIVE_W, c_aw);
  take(ST_WEDGES, c_wedges);
  take(ST_DEG_ACT, c_deg);
}

}  // namespace

hipError_t launch_offline(const DevGraph& g, const DevState& st, const RoundParams& p, const Downtime& d,
                          hipStream_t s) {
  hipLaunchKernelGGL(k_offline, dim3(grid_tasks((g.V + 31) >> 5)), dim3(256), 0, s, g, st, p, d);
  return hipGetLastError();
}

}  // namespace p2pg
