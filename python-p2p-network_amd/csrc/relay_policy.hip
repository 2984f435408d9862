// Relay policy (p2pg_set_relay_policy): the app's per-peer decision whether node_message forwards
// a first receipt (README.md:20, node.py:106-116) -- silent peers and probabilistic relay.  Peer v
// carries a threshold thr[v]: 0 relays everything, 0xFFFFFFFF nothing, and otherwise the first
// receipt of message m at v in round r is muted iff
//   philox4x32_10((r, v, msg_base + m, TAG_RLY), policy seed).x < thr[v].
// A muted receipt happens like any other and makes none of its sends, exactly like a receipt at
// its hop limit (relay_expire.hip).  Originations are the app's own send_to_nodes and exempt, and
// the messages a hop limit cancels in the round are left to k_expire: both come as one W-word
// mask `exempt` per round (null when the round has neither).  Two passes over the round's active
// rows, at the places of k_expire's:
//   count  inside the round: popcount(muted) x relays per receipt leaves the round's ST_RELAYS;
//   clear  when the round's sends become final: F[r&1][v] &= ~muted, AW rewritten, and a row that
//          becomes empty leaves the activity bitmap (it sends nothing: no later pass visits it).
// Both redraw; no [V][W] plane of decisions is kept.  An engine without a policy launches
// neither.  Internal; not part of the C-ABI.
#include "device_util.h"
#include "philox.h"

namespace p2pg {
namespace {

// One wave per 32-peer task, lane = word of a 64-word slice of the active peer's row.  The draws
// map lanes to receipts: a wave-uniform loop over the slice's nonzero candidate words (from a
// ballot), lane = bit of the word, one Philox per lane, the word's muted mask by ballot -- a row
// costs each lane one draw per nonzero word, not per bit.
template <bool CLEAR>
__global__ __launch_bounds__(256) void k_policy(DevGraph g, DevState st, RoundParams p,
                                                const uint32_t* __restrict__ thr, uint32_t seed_lo,
                                                uint32_t seed_hi, const uint64_t* __restrict__ exempt) {
  const int lane = threadIdx.x & 63;
  const int cur = p.round & 1;
  const int W = st.W;
  const int nslices = (W + 63) >> 6;
  const int64_t ntasks = (g.V + 31) >> 5;
  const bool packed = st.AW[cur] && nslices == 1;  // (AW planes exist for single-slice rows only)
  uint64_t cancelled = 0;  // this lane's share of the relays to take back
  for (int64_t task = (int64_t)blockIdx.x * WPB + wave_in_block(); task < ntasks;
       task += (int64_t)gridDim.x * WPB) {
    const uint32_t aw0 = st.A[cur][task];
    uint32_t aw = aw0, emptied = 0;
    while (aw) {
      const int b = __builtin_ctz(aw);
      aw &= aw - 1u;
      const int64_t v = (task << 5) + b;
      if (v >= g.V) break;
      const uint32_t t = ldc(thr + v);
      if (t == 0u) continue;  // relays every first receipt: no draw, nothing to change
      const uint64_t deg = (uint64_t)(g.rowptr[v + 1] - g.rowptr[v]);
      // relays per muted receipt, as the receive passes counted them (never an origination)
      const uint64_t per = p.mode == 0 ? (deg > 0 ? deg - 1 : 0)
                                       : (deg < (uint64_t)p.fanout ? deg : (uint64_t)p.fanout);
      bool left = false;  // does a word of the row stay nonzero?
      for (int sl = 0; sl < nslices; ++sl) {
        const int w = sl * 64 + lane;
        const bool valid = w < W;
        uint64_t* const fw = &st.F[cur][v * W + w];
        const uint64_t f = valid ? *fw : 0ull;
        const uint64_t cand = exempt ? f & ~(valid ? exempt[w] : 0ull) : f;
        uint64_t muted = cand;  // thr = 0xFFFFFFFF: the whole row, no draw
        if (t != 0xFFFFFFFFu) {
          muted = 0ull;
          uint64_t nz = __ballot(cand != 0ull);
          while (nz) {
            const int j = __builtin_amdgcn_readfirstlane(__builtin_ctzll(nz));
            nz &= nz - 1ull;
            const uint64_t word = (uint64_t)readlane64((int64_t)cand, j);
            bool m = false;
            if ((word >> lane) & 1ull) {
              const u32x4 c = {(uint32_t)p.round, (uint32_t)v,
                               p.msg_base + (uint32_t)((sl * 64 + j) * 64 + lane), TAG_RLY};
              m = philox4x32_10(c, seed_lo, seed_hi).x < t;
            }
            const uint64_t mb = __ballot(m);
            if (lane == j) muted = mb;
          }
        }
        if (CLEAR) {
          if (muted) *fw = f & ~muted;
          const uint64_t wm = __ballot((f & ~muted) != 0ull);
          left |= wm != 0ull;
          if (packed && lane == 0) st.AW[cur][v] = wm;
        } else {
          cancelled += (uint64_t)__popcll(muted) * per;
        }
      }
      if (CLEAR && !left) emptied |= 1u << b;
    }
    if (CLEAR && emptied && lane == 0) st.A[cur][task] = aw0 & ~emptied;
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

hipError_t launch_policy(const DevGraph& g, const DevState& st, const RoundParams& p, const uint32_t* thr,
                         uint64_t seed, const uint64_t* exempt, bool clear, hipStream_t s) {
  const int grid = grid_tasks((g.V + 31) >> 5);
  const uint32_t lo = (uint32_t)seed, hi = (uint32_t)(seed >> 32);
  if (clear)
    hipLaunchKernelGGL(k_policy<true>, dim3(grid), dim3(256), 0, s, g, st, p, thr, lo, hi, exempt);
  else
    hipLaunchKernelGGL(k_policy<false>, dim3(grid), dim3(256), 0, s, g, st, p, thr, lo, hi, exempt);
  return hipGetLastError();
}

}  // namespace p2pg
