// Originations after round 0: the Node.send_to_nodes(data) call an app makes at its own peer
// whenever it has something to say (p2pnetwork/node.py:106-112), for the messages whose start
// round is the round being run.  Runs after the round's receive pass (pull / update), before
// k_record and the gossip pushes, so an origination is a first receipt of round r at its origin
// like any other: the frontier bit sends it on (flood: the next pull reads F[r&1]; gossip: this
// round's push), k_record / k_deliveries find no sender for it (parent -1), k_sends / k_peer_tally
// give it all deg connections.  Internal; not part of the C-ABI.
#include "device_util.h"

namespace p2pg {
namespace {

// One wave per distinct origin peer of the round (group gi: schedule entries grp_off[gi] ..
// grp_off[gi + 1], all of one peer, sorted by message), lane = word of a 64-word slice.  The wave
// owns the peer's row -- no other kernel runs beside it on the engine's stream -- so the row is
// read and written plainly; only the activity bit shares its bitmap word with other waves.
//   A[r&1] bit clear: the row holds stale data (a frontier row is valid only under its A bit):
//                     the whole row is stored, zeros included, AW = the word mask, A bit set.
//   A[r&1] bit set:   the masks are ORed into the row (and AW).
// Counters as the receive passes count first receipts (the byte model's): relays per origination
// are deg (flood: no sender to exclude) or min(k, deg) (gossip).
__global__ __launch_bounds__(256) void k_originate(DevGraph g, DevState st, RoundParams p,
                                                   const int32_t* __restrict__ peer,
                                                   const int32_t* __restrict__ msg,
                                                   const int64_t* __restrict__ grp_off, int64_t g_lo,
                                                   int64_t n_groups) {
  const int lane = threadIdx.x & 63;
  const int64_t gi = (int64_t)blockIdx.x * WPB + wave_in_block();
  if (gi >= n_groups) return;
  const int64_t e0 = grp_off[g_lo + gi], e1 = grp_off[g_lo + gi + 1];
  if (e1 <= e0) return;
  const int64_t v = peer[e0];
  if (v < 0 || v >= g.V) return;
  const int W = st.W;
  const int cur = p.round & 1;
  const int nslices = (W + 63) >> 6;
  const uint64_t deg = (uint64_t)(g.rowptr[v + 1] - g.rowptr[v]);
  const uint64_t per = p.mode == 0 ? deg : (deg < (uint64_t)p.fanout ? deg : (uint64_t)p.fanout);
  const bool was = bit_test(st.A[cur], v);
  uint64_t c[STAT_N] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int sl = 0; sl < nslices; ++sl) {
    const int w = sl * 64 + lane;
    const bool valid = w < W;
    uint64_t mask = 0;
    for (int64_t i = e0; i < e1; ++i) {
      const int32_t m = msg[i];
      if (m >= 0 && m < st.M && (m >> 6) == w) mask |= 1ull << (m & 63);
    }
    uint64_t* const fw = &st.F[cur][v * W + w];
    const uint64_t old = (valid && was) ? *fw : 0ull;
    if (valid && (!was || mask)) *fw = old | mask;
    if (valid && mask) st.seen[v * W + w] |= mask;
    if (mask && !old) {
      c[ST_ACTIVE_W] += 1;
      c[ST_WEDGES] += deg;
    }
    if (st.AW[cur] && nslices == 1) {  // (AW planes exist for single-slice rows only)
      const uint64_t wm = __ballot(mask != 0ull);
      if (lane == 0) st.AW[cur][v] = was ? (st.AW[cur][v] | wm) : wm;
    }
  }
  if (lane == 0) {
    const uint64_t n = (uint64_t)(e1 - e0);
    c[ST_NEW] += n;
    c[ST_RELAYS] += n * per;
    if (!was) {
      atomicOr(&st.A[cur][v >> 5], 1u << (v & 31));
      c[ST_ACTIVE_V] += 1;
      c[ST_DEG_ACT] += deg;
    }
  }
  flush_stats(st.stats, c, lane);
}

}  // namespace

hipError_t launch_originate(const DevGraph& g, const DevState& st, const RoundParams& p,
                            const int32_t* peer, const int32_t* msg, const int64_t* grp_off,
                            int64_t g_lo, int64_t n_groups, hipStream_t s) {
  if (n_groups <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_originate, dim3((unsigned)((n_groups + WPB - 1) / WPB)), dim3(256), 0, s, g, st, p,
                     peer, msg, grp_off, g_lo, n_groups);
  return hipGetLastError();
}

}  // namespace p2pg
