// Hop limits (p2pg_set_ttl): the app's "forward ttl - 1 while ttl > 0" rule (README.md:20) on top
// of the dedup relay (node.py:106-116).  Message m expires in round x[m] = start[m] + ttl[m]: its
// first receipts of that round happen like any other, but make none of their sends.  The engine
// keeps, per round that has an expiry, a W-word mask X of the messages expiring in it and a mask
// Z <= X of those with ttl 0 (their only receipt is the origination itself, which has no sender
// to exclude), and runs two passes over the round's active rows:
//   count  inside the round, after its receive pass, k_originate, k_record and the tally column
//          count: the relays the expired receipts were counted with leave the round's ST_RELAYS
//          (the receive passes count every first receipt);
//   clear  when the round's sends become final (the next round's start, or a boundary call that
//          reads or changes them): F[r&1][v][w] &= ~X[w], so no later pass -- the next flood
//          pull, the held-back gossip push, k_sends, k_peer_tally, k_materialize -- sees a send of
//          them.  Until then the whole frontier serves the round's delivery stream.
// An engine without finite hop limits launches neither.  Internal; not part of the C-ABI.
#include "device_util.h"

namespace p2pg {
namespace {

// One wave per active peer v of round r (A[r&1]), lane = word of a 64-word slice; grid-stride
// over 32-peer tasks like k_rebuild_aw.  A row that becomes all zero keeps its A bit (legal: k_drop
// leaves such rows too); single-slice rows with AW planes get their word mask rewritten.
template <bool CLEAR>
__global__ __launch_bounds__(256) void k_expire(DevGraph g, DevState st, RoundParams p,
                                                const uint64_t* __restrict__ X,
                                                const uint64_t* __restrict__ Z) {
  const int lane = threadIdx.x & 63;
  const int cur = p.round & 1;
  const int W = st.W;
  const int nslices = (W + 63) >> 6;
  const int64_t ntasks = (g.V + 31) >> 5;
  const bool packed = st.AW[cur] && nslices == 1;  // (AW planes exist for single-slice rows only)
  uint64_t cancelled = 0;  // this lane's share of the relays to take back
  for (int64_t task = (int64_t)blockIdx.x * WPB + wave_in_block(); task < ntasks;
       task += (int64_t)gridDim.x * WPB) {
    uint32_t aw = st.A[cur][task];
    while (aw) {
      const int b = __builtin_ctz(aw);
      aw &= aw - 1u;
      const int64_t v = (task << 5) + b;
      if (v >= g.V) break;
      const uint64_t deg = (uint64_t)(g.rowptr[v + 1] - g.rowptr[v]);
      // relays per expired receipt, as the receive passes and k_originate counted them
      const uint64_t per = p.mode == 0 ? (deg > 0 ? deg - 1 : 0)
                                       : (deg < (uint64_t)p.fanout ? deg : (uint64_t)p.fanout);
      const uint64_t per_origin = p.mode == 0 ? deg : per;
      for (int sl = 0; sl < nslices; ++sl) {
        const int w = sl * 64 + lane;
        const bool valid = w < W;
        const uint64_t x = valid ? X[w] : 0ull;
        uint64_t* const fw = &st.F[cur][v * W + w];
        // (the word mask needs every word of the row, the rest only the words X touches)
        const uint64_t f = (valid && (x || (CLEAR && packed))) ? *fw : 0ull;
        const uint64_t hit = f & x;
        if (CLEAR) {
          if (hit) *fw = f & ~x;
          if (packed) {
            const uint64_t wm = __ballot((f & ~x) != 0ull);
            if (lane == 0) st.AW[cur][v] = wm;
          }
        } else if (hit) {
          const uint64_t no = (uint64_t)__popcll(hit & Z[w]);
          cancelled += ((uint64_t)__popcll(hit) - no) * per + no * per_origin;
        }
      }
    }
  }
  if (!CLEAR) {
    const uint64_t t = wave_sum(cancelled);
    // the counters are read as differences modulo 2^64 (engine.cpp, read_stats): adding -t takes
    // t relays out of this round's total
    if (lane == 0 && t)
      atomicAdd(st.stats + (blockIdx.x & (STAT_SHARDS - 1)) * STAT_N + ST_RELAYS, 0ull - (unsigned long long)t);
  }
}

}  // namespace

hipError_t launch_expire(const DevGraph& g, const DevState& st, const RoundParams& p, const uint64_t* X,
                         const uint64_t* Z, bool clear, hipStream_t s) {
  const int grid = grid_tasks((g.V + 31) >> 5);
  if (clear)
    hipLaunchKernelGGL(k_expire<true>, dim3(grid), dim3(256), 0, s, g, st, p, X, Z);
  else
    hipLaunchKernelGGL(k_expire<false>, dim3(grid), dim3(256), 0, s, g, st, p, X, Z);
  return hipGetLastError();
}

}  // namespace p2pg
