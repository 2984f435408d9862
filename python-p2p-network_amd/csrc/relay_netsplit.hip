// Network partition (p2pg_set_netsplit): the two passes of the rounds a netsplit acts
// on.  A connection whose ends are on different sides is cut in the rounds [from, until); a send over
// it that would arrive in one of them is lost.  The loss is per connection -- a receipt may stand
// because another copy arrived -- so it is decided where the copy is consumed (flood) or where the
// send is made (gossip); every other round launches the kernels it always launched.
//
//   k_pull_cut      flood, the receive pass of a cut round t > 0: the flood pull (k_pull / k_pull1,
//                   relay_kernels.hip, are its specification) over the neighbours whose copy arrived
//                   -- active in t - 1, on the peer's own side, not dropped by the churn draw of
//                   (t - 1, {u, v}).  One more 4-byte gather per neighbour, side[v], beside colidx.
//   k_pull_cut_hub  the same for the pull hubs (deg > HUB_T, W <= 64), one block per hub: the row is
//                   staged through LDS, 1024 connections at a time, and the arrived copies' rows are
//                   gathered by the four waves (k_pull_hub_lds + k_pull_hub_finalize in one).
//   k_push_cut      gossip, the push of a round r whose sends arrive in a cut round: the k Philox
//                   picks of every first receipt, each pushed by a row atomic into next[(r+1)&1]
//                   (the plane k_sparse_push fills, consumed by the update kernels unchanged) unless
//                   its connection is cut in r + 1 or the churn draw of (r, {v, u}) dropped it.
//
// An engine without a netsplit never launches these.  Internal; not part of the C-ABI.
#include "device_util.h"

namespace p2pg {
namespace {

// Wave = G peers of a 32-peer task, P = pow2ceil(min(W, 64)) lanes each, lane = (peer, word): at
// W <= 8 eight or more peers share a wave, at W >= 33 the wave is one peer (side[u] scalar) and rows
// of W > 64 words take a slice loop.  A peer's row is walked in chunks of P connections: lane `word`
// of the group takes slot `word` of the chunk -- its neighbour id, activity bit, side and churn
// draw, once per connection as in k_pull -- and then every lane gathers its own word of the frontier
// rows whose copy arrived, the neighbour ids read across the group's lanes, four rows in flight.  The wave stores the task's A and S words whole;
// no atomics but the counter shards.  Hubs (g.H) are left to k_pull_cut_hub.
template <bool CHURN>
__global__ __launch_bounds__(256) void k_pull_cut(DevGraph g, DevState st, RoundParams p, Netsplit ns) {
  const int lane = threadIdx.x & 63;
  const int wib = wave_in_block();
  const int64_t V = g.V;
  const int W = st.W;
  const int cur = p.round & 1, prv = cur ^ 1;
  const uint64_t* __restrict__ Fp = st.F[prv];
  uint64_t* __restrict__ Fc = st.F[cur];
  const uint32_t* __restrict__ Ap = st.A[prv];
  const int64_t ntasks = (V + 31) >> 5;
  const int nslices = (W + 63) >> 6;
  int P = 64;  // lanes per peer
  if (W < 64) {
    P = 1;
    while (P < W) P <<= 1;
  }
  const int G = P == 1 ? 32 : 64 / P;  // peers per step (a task has 32)
  const int sub = lane / P;
  const int word = lane & (P - 1);
  const bool in_group = sub < G;
  const int gshift = in_group ? sub * P : 0;  // the group's first lane
  const uint64_t gm = (P == 64 ? ~0ull : (1ull << P) - 1ull) << gshift;
  const uint32_t step_mask = G == 32 ? ~0u : (1u << G) - 1u;
  uint64_t c[STAT_N] = {0, 0, 0, 0, 0, 0, 0, 0};

  for (int64_t task = (int64_t)blockIdx.x * WPB + wib; task < ntasks; task += (int64_t)gridDim.x * WPB) {
    const int64_t u0 = task << 5;
    const uint32_t sat0 = st.S[task];
    uint32_t todo = ~sat0;
    if (g.H) todo &= ~g.H[task];
    if (V - u0 < 32) todo &= (1u << (V - u0)) - 1u;
    uint32_t aw = 0, sat = sat0;
    for (int b0 = 0; b0 < 32 && todo; b0 += G) {
      if (!((todo >> b0) & step_mask)) continue;
      const int b = (b0 + sub) & 31;
      const bool on = in_group && ((todo >> b) & 1u);
      const int64_t u = u0 + b;
      int64_t beg = 0, end = 0;
      int32_t su = 0;
      uint32_t gu = 0;
      if (on) {
        beg = g.rowptr[u];
        end = g.rowptr[u + 1];
        su = ns.side[u];
        gu = gidx(g, u);
      }
      const uint64_t deg = (uint64_t)(end - beg);
      bool row_new = false, row_full = true;
      for (int sl = 0; sl < nslices; ++sl) {
        const int w = sl * 64 + word;
        const bool valid = on && w < W;
        const uint64_t fm = valid ? full_mask(w, W, st.M) : 0ull;
        const uint64_t s = valid ? st.seen[u * W + w] : 0ull;
        const uint64_t need = fm & ~s;
        uint64_t acc = 0;
        // The row in chunks of P connections, lane `word` of the group = slot: every neighbour's id,
        // activity, side and churn draw are evaluated once per group, not once per lane.  The trip
        // count is the wave's largest, so the whole wave is active for the lane reads below.
        const bool needg = (__ballot(need != 0ull) & gm) != 0ull;
        const uint32_t chunks = needg ? (uint32_t)((deg + (uint64_t)P - 1) / (uint64_t)P) : 0u;
        const uint32_t trips = wave_reduce_u32<true>(chunks);
        for (uint32_t ci = 0; ci < trips; ++ci) {
          const int64_t j = beg + (int64_t)ci * P + word;
          int32_t v = 0;
          bool a = false;
          if (ci < chunks && j < end) {
            v = g.colidx[j];
            a = bit_test(Ap, v) && !netsplit::link_cut(p.round, su, ns.side[v], ns.from, ns.until);
            if (CHURN && a)
              a = !churn_dropped((uint32_t)(p.round - 1), gu, gidx(g, v), p.churn_thr, p.cseed_lo, p.cseed_hi);
          }
          const uint64_t act = __ballot(a);
          if (!act) continue;
          const uint64_t gact = act >> gshift;  // bit q: slot q of this group's chunk arrived
          for (int q0 = 0; q0 < P; q0 += 4) {
            uint64_t x[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              x[t] = 0ull;
              if (q0 + t < P) {  // (wave-uniform: the lane read runs with every lane active)
                const uint32_t vq = bperm(gshift + q0 + t, (uint32_t)v);
                if (((gact >> (q0 + t)) & 1ull) && need) x[t] = Fp[(int64_t)vq * W + w];
              }
            }
            acc |= (x[0] | x[1]) | (x[2] | x[3]);
          }
        }
        const uint64_t nw = acc & need;
        const bool any = (__ballot(nw != 0ull) & gm) != 0ull;
        row_new |= any;
        if (__ballot(valid && (s | nw) != fm) & gm) row_full = false;
        if (nw) st_row(&st.seen[u * W + w], s | nw);
        // single-slice rows are written only when active; multi-slice rows always (a row must be
        // whole whenever its A bit is set)
        if (valid && (any || nslices > 1)) st_row(&Fc[u * W + w], nw);
        if (nw) {
          const uint64_t pc = (uint64_t)__popcll(nw);
          c[ST_NEW] += pc;
          c[ST_RELAYS] += pc * (deg - 1);
          c[ST_ACTIVE_W] += 1;
          c[ST_WEDGES] += deg;
        }
      }
      const bool lead = on && word == 0;
      if (lead && row_new) {
        c[ST_ACTIVE_V] += 1;
        c[ST_DEG_ACT] += deg;
      }
      const uint64_t newm = __ballot(lead && row_new), fullm = __ballot(lead && row_full);
      for (int q = 0; q < G && b0 + q < 32; ++q) {
        aw |= (uint32_t)((newm >> (q * P)) & 1ull) << (b0 + q);
        sat |= (uint32_t)((fullm >> (q * P)) & 1ull) << (b0 + q);
      }
    }
    if (lane == 0) {
      // (a task's hubs: their bits are ORed in by k_pull_cut_hub, which runs after this kernel)
      st.A[cur][task] = aw;
      if (sat != sat0) st.S[task] = sat;
    }
  }
  flush_stats(st.stats, c, lane);
}

// One block per pull hub (deg > HUB_T), W <= 64.  Per 1024 connections of the row: all 256 threads
// load the neighbour ids, activity, sides (and the churn draw) at once and compact the neighbours
// whose copy arrived into an LDS list; the four waves gather the listed frontier rows (lane = word, 8
// in flight).  The waves' ORs are folded through LDS and wave 0 finalises the hub as
// k_pull_hub_finalize does: its A / S bits by atomicOr, since k_pull_cut stored those words whole.
constexpr int CUT_STAGE = 1024;
template <bool CHURN>
__global__ __launch_bounds__(256) void k_pull_cut_hub(DevGraph g, DevState st, RoundParams p, Netsplit ns,
                                                      const int32_t* __restrict__ hubs, int64_t n_hubs) {
  static_assert(CUT_STAGE % 256 == 0, "whole slots per thread");
  __shared__ uint32_t s_row[CUT_STAGE];
  __shared__ uint64_t s_acc[WPB][64];
  __shared__ uint32_t s_n;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wib = wave_in_block();
  const int W = st.W;
  const int cur = p.round & 1, prv = cur ^ 1;
  const uint64_t* __restrict__ Fp = st.F[prv];
  const uint32_t* __restrict__ Ap = st.A[prv];
  const bool valid = lane < W;
  const uint64_t fm = valid ? full_mask(lane, W, st.M) : 0ull;
  uint64_t c[STAT_N] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int64_t h = blockIdx.x; h < n_hubs; h += gridDim.x) {
    const int64_t u = hubs[h];
    if (bit_test(st.S, u)) continue;  // (the same for every wave: only this block writes u's bit)
    const int64_t beg = g.rowptr[u], end = g.rowptr[u + 1];
    const uint64_t s = valid ? at_row(st.seen, u, W)[lane] : 0ull;
    const uint64_t need = fm & ~s;
    const int32_t su = ns.side[u];
    const uint32_t gu = gidx(g, u);
    uint64_t acc = 0;
    for (int64_t c0 = beg; c0 < end; c0 += CUT_STAGE) {
      if (tid == 0) s_n = 0u;
      __syncthreads();
#pragma unroll
      for (int k0 = 0; k0 < CUT_STAGE; k0 += 256) {
        const int64_t j = c0 + k0 + tid;
        if (j < end) {
          const int32_t v = g.colidx[j];
          bool a = bit_test(Ap, v) && !netsplit::link_cut(p.round, su, ns.side[v], ns.from, ns.until);
          if (CHURN && a)
            a = !churn_dropped((uint32_t)(p.round - 1), gu, gidx(g, v), p.churn_thr, p.cseed_lo, p.cseed_hi);
          if (a) s_row[atomicAdd(&s_n, 1u)] = (uint32_t)v;  // (at most CUT_STAGE candidates per stage)
        }
      }
      __syncthreads();
      const uint32_t n = s_n;
      for (uint32_t i0 = (uint32_t)wib * 8u; i0 < n; i0 += WPB * 8u) {
        uint64_t x[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const uint32_t i = i0 + (uint32_t)k;
          x[k] = (i < n && need) ? at_row(Fp, s_row[i], W)[lane] : 0ull;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) acc |= x[k];
      }
      __syncthreads();  // s_n / s_row are rewritten by the next stage
    }
    s_acc[wib][lane] = acc;
    __syncthreads();
    if (wib == 0) {
      uint64_t r = 0;
#pragma unroll
      for (int q = 0; q < WPB; ++q) r |= s_acc[q][lane];
      const uint64_t nw = r & need;
      const uint64_t deg = (uint64_t)(end - beg);
      if (nw) {
        st_row(at_row(st.seen, u, W) + lane, s | nw);
        const uint64_t pc = (uint64_t)__popcll(nw);
        c[ST_NEW] += pc;
        c[ST_RELAYS] += pc * (deg - 1);
        c[ST_ACTIVE_W] += 1;
        c[ST_WEDGES] += deg;
      }
      if (__ballot(nw != 0ull)) {
        if (valid) st_row(at_row(st.F[cur], u, W) + lane, nw);
        if (lane == 0) {
          atomicOr(&st.A[cur][u >> 5], 1u << (u & 31));
          c[ST_ACTIVE_V] += 1;
          c[ST_DEG_ACT] += deg;
        }
      }
      if (!__ballot(valid && (s | nw) != fm) && lane == 0) atomicOr(&st.S[u >> 5], 1u << (u & 31));
    }
    __syncthreads();  // s_acc is rewritten by the next hub
  }
  flush_stats(st.stats, c, lane);
}

// One wave per active peer v of round r = p.round, lane = word of a 64-word slice (a slice loop for
// W > 64); the frontier rows of such a round are whole.  Per lane: a peer with deg <= k sends the
// word to every connection; else every set bit draws its k Philox picks (gossip_picks, any degree:
// a wide sender needs nothing more).  Per send: lost if the connection was removed, is cut in r + 1
// or the churn draw of (r, {v, u}) dropped it; else one atomicOr into next[(r+1)&1][u][w] and u's T
// bit (a receiver that is offline in r + 1 stays the job of k_offline).  ST_SCATTER counts the sends
// that were not lost -- one per (sender, message, pick), or per (sender, word, connection) at
// deg <= k: at least the distinct masks the sparse push would count, which is all the schedule asks
// of it (a bound on the next frontier's words).
template <bool CHURN>
__global__ __launch_bounds__(256) void k_push_cut(DevGraph g, DevState st, RoundParams p, Netsplit ns) {
  const int lane = threadIdx.x & 63;
  const int wib = wave_in_block();
  const int W = st.W;
  const int cur = p.round & 1, nxt = cur ^ 1;
  const uint64_t* __restrict__ Fc = st.F[cur];
  uint64_t* __restrict__ nx = st.next[nxt];
  uint32_t* __restrict__ Tn = st.T[nxt];
  const int nslices = (W + 63) >> 6;
  const int64_t ntasks = (g.V + 31) >> 5;
  const uint32_t k = (uint32_t)p.fanout;
  uint64_t pushed = 0;
  for (int64_t task = (int64_t)blockIdx.x * WPB + wib; task < ntasks; task += (int64_t)gridDim.x * WPB) {
    uint32_t aw = st.A[cur][task];
    while (aw) {
      const int b = __builtin_ctz(aw);
      aw &= aw - 1u;
      const int64_t v = (task << 5) + b;
      const int64_t rb = g.rowptr[v];
      const uint32_t deg = (uint32_t)(g.rowptr[v + 1] - rb);
      if (deg == 0u) continue;
      const int32_t sv = ns.side[v];
      const uint32_t gv = gidx(g, v);
      for (int sl = 0; sl < nslices; ++sl) {
        const int w = sl * 64 + lane;
        const uint64_t f = w < W ? Fc[v * W + w] : 0ull;
        auto push = [&](int64_t slot, uint64_t mask) {
          if (g.gone && g.gone[slot]) return;
          const int32_t u = g.colidx[slot];
          if (netsplit::link_cut(p.round + 1, sv, ns.side[u], ns.from, ns.until)) return;
          if (CHURN && churn_dropped((uint32_t)p.round, gv, gidx(g, u), p.churn_thr, p.cseed_lo, p.cseed_hi)) return;
          pushed += 1;
          if (p.dedup_push) {
            mask &= ~st.seen[(int64_t)u * W + w];
            if (!mask) return;  // a duplicate in its entirety: nothing to deliver
          }
          atomicOr((unsigned long long*)&nx[(int64_t)u * W + w], (unsigned long long)mask);
          const uint32_t tb = 1u << (u & 31);
          if (!(Tn[u >> 5] & tb)) atomicOr(&Tn[u >> 5], tb);
        };
        if (!f) continue;
        if (deg <= k) {
          for (uint32_t q = 0; q < deg; ++q) push(rb + (int64_t)q, f);
        } else {
          uint64_t o = f;
          while (o) {
            const int bit = __builtin_ctzll(o);
            o &= o - 1ull;
            uint32_t pk[16];
            gossip_picks((uint32_t)p.round, gv, p.msg_base + (uint32_t)(w * 64 + bit), deg, (int)k, p.gseed_lo,
                         p.gseed_hi, pk);
            for (uint32_t q = 0; q < k; ++q) push(rb + (int64_t)pk[q], 1ull << bit);
          }
        }
      }
    }
  }
  uint64_t c[STAT_N] = {0, 0, 0, 0, 0, 0, 0, 0};
  c[ST_SCATTER] = pushed;
  flush_stats(st.stats, c, lane);
}

}  // namespace

hipError_t launch_pull_cut(const DevGraph& g, const DevState& st, const RoundParams& p, const Netsplit& ns,
                           const HubPlan& hp, hipStream_t s) {
  if (!ns.side || p.round < 1) return hipErrorInvalidValue;
  DevGraph g2 = g;
  const bool hubs = st.W <= 64 && g.H && hp.n_hubs > 0;
  if (!hubs) g2.H = nullptr;  // multi-slice rows: no hub split (as the flood pull)
  const int grid = grid_tasks((g.V + 31) >> 5);
  const unsigned hgrid = (unsigned)std::min<int64_t>(hp.n_hubs, 65535);
  if (p.churn_thr) {
    hipLaunchKernelGGL(k_pull_cut<true>, dim3(grid), dim3(256), 0, s, g2, st, p, ns);
    if (hubs) hipLaunchKernelGGL(k_pull_cut_hub<true>, dim3(hgrid), dim3(256), 0, s, g2, st, p, ns, hp.hubs, hp.n_hubs);
  } else {
    hipLaunchKernelGGL(k_pull_cut<false>, dim3(grid), dim3(256), 0, s, g2, st, p, ns);
    if (hubs) hipLaunchKernelGGL(k_pull_cut_hub<false>, dim3(hgrid), dim3(256), 0, s, g2, st, p, ns, hp.hubs, hp.n_hubs);
  }
  return hipGetLastError();
}

hipError_t launch_push_cut(const DevGraph& g, const DevState& st, const RoundParams& p, const Netsplit& ns,
                           hipStream_t s) {
  if (!ns.side || p.fanout < 1 || p.fanout > 16) return hipErrorInvalidValue;
  const int grid = grid_tasks((g.V + 31) >> 5);
  if (p.churn_thr)
    hipLaunchKernelGGL(k_push_cut<true>, dim3(grid), dim3(256), 0, s, g, st, p, ns);
  else
    hipLaunchKernelGGL(k_push_cut<false>, dim3(grid), dim3(256), 0, s, g, st, p, ns);
  return hipGetLastError();
}

}  // namespace p2pg
