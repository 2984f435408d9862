// Anti-entropy (p2pg_set_anti_entropy): periodic pull repair.  In a request round r
// every online peer u with a connection sends one request, carrying its seen set, to one drawn
// connection p (pull_partner_slot, philox.h).  p answers in round r + 1, after that round's
// arrivals and originations, with every message it has seen and the digest lacks; the reply
// arrives in round r + 2 as one more packet from sender p.  Request and reply are sends of their
// rounds: lost by the churn draw of (round, {u, p}), because their receiver is offline in the round
// they would arrive in, or because the connection is cut in that round (p2pg_set_netsplit).  Nothing but the arrivals is state, so request and reply rounds
// launch nothing; both kernels here run in the arrival round a = r + 2, around the receive pass
// the plan chose (flood pull, gossip update or gossip pull):
//
//   k_pull_gather   before the receive pass.  seen is then exactly the state at the end of round
//                   a - 1, and what u first-receives by the reply is seen[p] & ~seen[u] of that
//                   state: the digest only shortens the reply's list, since what u saw in r + 1
//                   it does not receive again.  The kernel makes the draw and the four loss tests
//                   per peer, counts the exchange's packets, and writes R[u] = seen[p] & ~seen[u]
//                   and u's PB bit ("a reply with something in it arrived").
//   k_pull_apply    after the receive pass (and k_offline), before k_originate.  The reply is
//                   processed after the relay packets of the round, so add = R[u] & ~seen[u] is what
//                   no relay copy delivered in this round: ordinary first receipts of round a, ORed
//                   into seen and F[a&1] as k_originate does, with the receive passes' counters.
//
// They are two because p's own receipts of round a -- relayed or pulled -- are not visible to u in
// round a: a single pass that read seen[p] while p's wave ORs its new bits in would hand them on a
// round early.  R is left as gathered, so find_parent (relay_kernels.hip) and the sender walks of
// k_sends / k_peer_tally can ask "did the reply carry m" until the next gather.
// An engine without the setting never launches these.  Internal; not part of the C-ABI.
#include "device_util.h"

namespace p2pg {
namespace {

__device__ __forceinline__ void flush_pull(unsigned long long* cnt, int idx, uint64_t x, int lane) {
  const uint64_t t = wave_sum(x);
  if (lane == 0 && t) atomicAdd(cnt + (blockIdx.x & (STAT_SHARDS - 1)) * PULL_N + idx, (unsigned long long)t);
}

// One wave per 32-peer task; the wave stores the task's PB word whole, so no bitmap atomics.
// Stage 1, lane = peer of the task: the partner draw, the loss terms and the packet counts, once
// per peer.  Stage 2, the row gather:
//   NARROW (W <= 32): P = pow2ceil(W) lanes per peer, 64 / P peers per step, lane = (peer, word)
//                     -- a one-peer wave on an 8-word row would leave 7/8 of every gather idle;
//   else:             wave = peer, lane = word of a 64-word slice, a slice loop for W > 64.
// A peer whose row is full (S bit) or whose exchange failed writes nothing but its counts; its R
// row is stale and its PB bit clear.  No LDS, no global atomics but the counter shards.
template <bool NARROW>
__global__ __launch_bounds__(256) void k_pull_gather(DevGraph g, DevState st, RoundParams p, Downtime d, Netsplit ns, Pull pl) {
  const int lane = threadIdx.x & 63;
  const int W = st.W;
  const int32_t rq = p.round - 2;  // the request round
  const int64_t ntasks = (g.V + 31) >> 5;
  int P = 64;  // lanes per peer
  if (NARROW) {
    P = 1;
    while (P < W) P <<= 1;
  }
  const int G = P == 1 ? 32 : 64 / P;  // peers per step (a task has 32)
  const int sub = NARROW ? lane / P : 0;
  const int word = NARROW ? lane & (P - 1) : lane;
  const uint64_t gm = P == 64 ? ~0ull : (1ull << P) - 1ull;
  const int nslices = (W + 63) >> 6;
  uint64_t c_req = 0, c_reql = 0, c_rep = 0, c_repl = 0;
  for (int64_t task = (int64_t)blockIdx.x * WPB + wave_in_block(); task < ntasks;
       task += (int64_t)gridDim.x * WPB) {
    const uint32_t sat = st.S[task];
    // stage 1: lane b < 32 is peer (task << 5) + b
    const int64_t v = (task << 5) + (lane & 31);
    bool ok = false;
    int32_t pp = 0;
    if (lane < 32 && v < g.V) {
      const int64_t beg = g.rowptr[v];
      const uint32_t deg = (uint32_t)(g.rowptr[v + 1] - beg);
      const bool down_v = d.from && downtime::offline(rq, d.from[v], d.until[v]);
      if (deg >= 1u && !down_v) {  // (a peer without a connection and an offline peer send no request)
        pp = g.colidx[beg + pull_partner_slot((uint32_t)rq, gidx(g, v), deg, pl.seed_lo, pl.seed_hi)];
        // the request is a send of round rq to pp, the reply a send of round rq + 1 to v
        const bool req_lost =
            churn_dropped((uint32_t)rq, gidx(g, v), gidx(g, pp), p.churn_thr, p.cseed_lo, p.cseed_hi) ||
            (d.from && downtime::offline(rq + 1, d.from[pp], d.until[pp])) || link_cut(ns, rq + 1, v, pp);
        const bool rep_lost =
            !req_lost &&
            (churn_dropped((uint32_t)(rq + 1), gidx(g, pp), gidx(g, v), p.churn_thr, p.cseed_lo, p.cseed_hi) ||
             (d.from && downtime::offline(rq + 2, d.from[v], d.until[v])) || link_cut(ns, rq + 2, pp, v));
        c_req += 1;
        c_reql += req_lost ? 1 : 0;
        c_rep += req_lost ? 0 : 1;  // (sent even if it lists nothing)
        c_repl += rep_lost ? 1 : 0;
        ok = !req_lost && !rep_lost && !((sat >> (lane & 31)) & 1u);
      }
    }
    const uint32_t okm = (uint32_t)__ballot(ok);
    uint32_t pb = 0;
    if (NARROW) {
      for (int b0 = 0; b0 < 32 && (okm >> b0); b0 += G) {
        const int b = (b0 + sub) & 31;
        const int32_t ppb = (int32_t)bperm(b, (uint32_t)pp);
        const bool mine = sub < G && ((okm >> b) & 1u) && word < W;
        uint64_t x = 0;
        if (mine) {
          const int64_t u = (task << 5) + b;
          x = st.seen[(int64_t)ppb * W + word] & ~st.seen[u * W + word];
          pl.R[u * W + word] = x;
        }
        const uint64_t bal = __ballot(x != 0ull);
        for (int q = 0; q < G; ++q)
          if ((bal >> (q * P)) & gm) pb |= 1u << (b0 + q);
      }
    } else {
      uint32_t todo = okm;
      while (todo) {
        const int b = __builtin_ctz(todo);
        todo &= todo - 1u;
        const int64_t u = (task << 5) + b;
        const int64_t ppb = __builtin_amdgcn_readlane(pp, b);
        bool any = false;
        for (int sl = 0; sl < nslices; ++sl) {
          const int w = sl * 64 + word;
          if (w < W) {
            const uint64_t x = st.seen[ppb * W + w] & ~st.seen[u * W + w];
            pl.R[u * W + w] = x;
            any |= x != 0ull;
          }
        }
        if (__ballot(any)) pb |= 1u << b;
      }
    }
    if (lane == 0) pl.PB[task] = pb;
  }
  flush_pull(pl.cnt, PL_REQUESTS, c_req, lane);
  flush_pull(pl.cnt, PL_REQUESTS_LOST, c_reql, lane);
  flush_pull(pl.cnt, PL_REPLIES, c_rep, lane);
  flush_pull(pl.cnt, PL_REPLIES_LOST, c_repl, lane);
}

// One wave per 32-peer task, then per PB peer u of it, lane = word of a 64-word slice.  The wave
// owns the rows and the task's A word (no other kernel runs beside it on the engine's stream):
//   add = R[u] & ~seen[u]: the reply's bits no relay copy delivered in this round.  Nothing: the
//         peer is left alone.  Else seen |= add and, as k_originate does it,
//   A[a&1] bit clear: the frontier row holds stale data: the whole row is stored, zeros included,
//                     AW = the word mask, the A bit set;
//   A[a&1] bit set:   add is ORed into the row (and AW).
// Counters as the receive passes count first receipts: relays per receipt are deg - 1 (flood: the
// sender is excluded; a peer with a partner has deg >= 1) or min(k, deg) (gossip).
__global__ __launch_bounds__(256) void k_pull_apply(DevGraph g, DevState st, RoundParams p, Pull pl) {
  const int lane = threadIdx.x & 63;
  const int W = st.W;
  const int cur = p.round & 1;
  const int nslices = (W + 63) >> 6;
  const int64_t ntasks = (g.V + 31) >> 5;
  uint64_t c[STAT_N] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t repaired = 0;
  for (int64_t task = (int64_t)blockIdx.x * WPB + wave_in_block(); task < ntasks;
       task += (int64_t)gridDim.x * WPB) {
    uint32_t pb = pl.PB[task];
    if (!pb) continue;
    const uint32_t aw0 = st.A[cur][task];
    uint32_t woken = 0;
    while (pb) {
      const int b = __builtin_ctz(pb);
      pb &= pb - 1u;
      const int64_t u = (task << 5) + b;
      if (u >= g.V) break;
      bool gain = false;
      for (int sl = 0; sl < nslices; ++sl) {
        const int w = sl * 64 + lane;
        if (w < W) gain |= (pl.R[u * W + w] & ~st.seen[u * W + w]) != 0ull;
      }
      if (!__ballot(gain)) continue;  // a relay copy of every listed message arrived in this round
      const bool was = (aw0 >> b) & 1u;
      const uint64_t deg = (uint64_t)(g.rowptr[u + 1] - g.rowptr[u]);
      const uint64_t per = p.mode == 0 ? (deg > 0 ? deg - 1 : 0)
                                       : (deg < (uint64_t)p.fanout ? deg : (uint64_t)p.fanout);
      for (int sl = 0; sl < nslices; ++sl) {
        const int w = sl * 64 + lane;
        const bool valid = w < W;
        const int64_t i = u * W + w;
        const uint64_t s = valid ? st.seen[i] : 0ull;
        const uint64_t add = valid ? pl.R[i] & ~s : 0ull;
        const uint64_t old = (valid && was) ? st.F[cur][i] : 0ull;
        if (valid && (!was || add)) st.F[cur][i] = old | add;
        if (add) st.seen[i] = s | add;
        const uint64_t n = (uint64_t)__popcll(add);
        c[ST_NEW] += n;
        c[ST_RELAYS] += n * per;
        repaired += n;
        if (add && !old) {
          c[ST_ACTIVE_W] += 1;
          c[ST_WEDGES] += deg;
        }
        if (st.AW[cur] && nslices == 1) {  // (AW planes exist for single-slice rows only)
          const uint64_t wm = __ballot(add != 0ull);
          if (lane == 0) st.AW[cur][u] = was ? (st.AW[cur][u] | wm) : wm;
        }
      }
      if (!was) {
        woken |= 1u << b;
        if (lane == 0) {
          c[ST_ACTIVE_V] += 1;
          c[ST_DEG_ACT] += deg;
        }
      }
    }
    if (woken && lane == 0) st.A[cur][task] = aw0 | woken;
  }
  flush_stats(st.stats, c, lane);
  flush_pull(pl.cnt, PL_REPAIRED, repaired, lane);
}

}  // namespace

hipError_t launch_pull_gather(const DevGraph& g, const DevState& st, const RoundParams& p, const Downtime& d,
                              const Netsplit& ns, const Pull& pl, hipStream_t s) {
  const dim3 grid(grid_tasks((g.V + 31) >> 5));
  if (st.W <= 32)
    hipLaunchKernelGGL(k_pull_gather<true>, grid, dim3(256), 0, s, g, st, p, d, ns, pl);
  else
    hipLaunchKernelGGL(k_pull_gather<false>, grid, dim3(256), 0, s, g, st, p, d, ns, pl);
  return hipGetLastError();
}

hipError_t launch_pull_apply(const DevGraph& g, const DevState& st, const RoundParams& p, const Pull& pl,
                             hipStream_t s) {
  hipLaunchKernelGGL(k_pull_apply, dim3(grid_tasks((g.V + 31) >> 5)), dim3(256), 0, s, g, st, p, pl);
  return hipGetLastError();
}

}  // namespace p2pg
