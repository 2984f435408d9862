// Run tallies computed on the device (p2pg_message_reach / p2pg_message_tally /
// p2pg_peer_counters):
//   * k_colcount: per-message (bit-column) counts of a [V][W] bitset plane -- every row (the seen
//     plane: how many peers hold message m) or the rows under an activity bitmap (a round's
//     frontier: its first receipts, from which reach / hop_sum / last_hop accumulate);
//   * k_peer_tally: Node.message_count_send (node.py:65, :116) and message_count_recv
//     (nodeconnection.py:215) per peer, from the same send set relay_sends.hip's k_sends
//     enumerates, accumulated instead of emitted;
//   * k_msg_cost (p2pg_message_cost): the same send set accumulated per message -- the
//     send_to_node calls that carried payload id m (node.py:116) and those of them that arrived
//     (nodeconnection.py:215).
// Opt-in passes outside the rounds' own kernels.  Internal; not part of the C-ABI.
#include "device_util.h"

namespace p2pg {
namespace {

// Vertical (bit-sliced) counters: plane i of a lane holds bit i of 64 independent counters, one
// per bit of the lane's word, so absorbing a row is a ripple-carry add of a 1-bit number:
// 2 logic ops per plane instead of ~2 per BIT.  They hold 2^PLANES - 1 rows, then are flushed
// (~2 ops per plane and bit, once per period) into the block's 64 x 64 counts in LDS.
constexpr int TALLY_PLANES = 7;
constexpr int TALLY_PERIOD = (1 << TALLY_PLANES) - 1;
constexpr int TALLY_UNROLL = 4;     // rows in flight per lane
constexpr int TALLY_ROWS = 256;     // whole-plane form: rows per wave task

struct VCount {
  uint64_t c[TALLY_PLANES];
  int absorbed;  // rows in c since its last flush (wave-uniform)
};

__device__ __forceinline__ void vc_reset(VCount& k) {
#pragma unroll
  for (int i = 0; i < TALLY_PLANES; ++i) k.c[i] = 0ull;
  k.absorbed = 0;
}

__device__ __forceinline__ void vc_absorb(VCount& k, uint64_t x) {
  uint64_t carry = x;
#pragma unroll
  for (int i = 0; i < TALLY_PLANES; ++i) {
    const uint64_t t = k.c[i] & carry;
    k.c[i] ^= carry;
    carry = t;
  }
}

// The lane's 64 counts go to row wl of lds[64][64], rotated by wl so that the 64 lanes of one
// LDS instruction spread over the banks (unrotated they would all hit bank b & 31).
__device__ __forceinline__ void vc_flush(VCount& k, uint32_t* lds, int wl, bool lane_on) {
  if (lane_on) {
#pragma unroll
    for (int b = 0; b < 64; ++b) {
      uint32_t v = 0u;
#pragma unroll
      for (int i = 0; i < TALLY_PLANES; ++i) v |= ((uint32_t)(k.c[i] >> b) & 1u) << i;
      if (v) atomicAdd(&lds[wl * 64 + ((b + wl) & 63)], v);
    }
  }
  vc_reset(k);
}

// Bit-column counts of plane [V][W].  lane <-> word of a row: at W >= 64 a wave's load is one
// 64-word slice of one row, at W < 64 it is 64 / W whole rows (contiguous either way).  A block
// works on one slice at a time (block items are slice-major), each wave on its own task: TALLY_ROWS
// consecutive rows (whole plane), or the active rows of one 32-peer word of A (FRONTIER: a tail
// round costs a bitmap scan).  The waves' vertical counters meet in the block's LDS counts; when
// the block's slice changes and at its end only the nonzero counts go out, one atomic per (block,
// message), into shard blockIdx & (shards - 1) of scratch[shards][nsl * 4096] -- few lines, so
// spread like the round counters (STAT_SHARDS).  LDS counts are 32 bits: a block absorbs at most
// V < 2^31 rows of a slice.
template <bool FRONTIER>
__global__ __launch_bounds__(256) void k_colcount(const uint64_t* __restrict__ plane,
                                                  const uint32_t* __restrict__ A, int64_t V, int W,
                                                  unsigned long long* __restrict__ scratch, int shards) {
  __shared__ uint32_t lds[64 * 64];
  const int lane = threadIdx.x & 63;
  const int wib = wave_in_block();
  const int SW = W < 64 ? W : 64;  // words of a row a wave load covers
  const int R = 64 / SW;           // rows per wave load
  const int wl = lane % SW, ro = lane / SW;
  const bool lane_on = ro < R;
  const int nsl = (W + 63) >> 6;
  const int64_t ntasks = FRONTIER ? (V + 31) >> 5 : (V + TALLY_ROWS - 1) / TALLY_ROWS;
  const int64_t nbt = (ntasks + WPB - 1) / WPB;  // block tasks: WPB wave tasks each
  const int64_t nitems = nbt * nsl;
  VCount k;
  vc_reset(k);
  for (int i = threadIdx.x; i < 64 * 64; i += 256) lds[i] = 0u;
  __syncthreads();
  auto block_flush = [&](int sl) {  // block-uniform calls only; leaves the LDS counts zero
    vc_flush(k, lds, wl, lane_on);
    __syncthreads();
    unsigned long long* out = scratch + (size_t)(blockIdx.x & (shards - 1)) * ((size_t)nsl * 4096);
    for (int i = threadIdx.x; i < SW * 64; i += 256) {
      const int word = i >> 6;
      const int b = ((i & 63) - word) & 63;
      const uint32_t v = lds[i];
      const int gw = sl * 64 + word;
      if (v) {
        lds[i] = 0u;
        if (gw < W) atomicAdd(out + (size_t)gw * 64 + b, (unsigned long long)v);
      }
    }
    __syncthreads();
  };
  int cur_sl = -1;
  for (int64_t bi = blockIdx.x; bi < nitems; bi += gridDim.x) {
    const int sl = (int)(bi / nbt);
    if (sl != cur_sl) {
      if (cur_sl >= 0) block_flush(cur_sl);
      cur_sl = sl;
    }
    const int64_t task = (bi - (int64_t)sl * nbt) * WPB + wib;
    if (task >= ntasks) continue;
    const int w = sl * 64 + wl;
    const bool w_on = lane_on && w < W;
    uint32_t rest = 0u;  // FRONTIER: the task's active peers not yet taken
    int64_t row0;
    int n;               // rows of this task
    if (FRONTIER) {
      rest = A[task];
      row0 = task << 5;
      n = __popc(rest);
    } else {
      row0 = task * TALLY_ROWS;
      n = (int)(V - row0 < TALLY_ROWS ? V - row0 : TALLY_ROWS);
    }
    for (int i0 = 0; i0 < n; i0 += R * TALLY_UNROLL) {
      if (k.absorbed + TALLY_UNROLL > TALLY_PERIOD) vc_flush(k, lds, wl, lane_on);
      uint64_t x[TALLY_UNROLL];
#pragma unroll
      for (int u = 0; u < TALLY_UNROLL; ++u) {
        int64_t row = -1;
        if (FRONTIER) {
          // this load takes the R lowest peers still in `rest`; the lane's is the ro-th of them
          const int np = __popc(rest);
          if (ro < np) row = row0 + (R == 1 ? (uint32_t)__builtin_ctz(rest) : select_bit32(rest, (uint32_t)ro));
          for (int q = 0; q < R && rest; ++q) rest &= rest - 1u;
        } else {
          const int i = i0 + u * R + ro;
          if (i < n) row = row0 + i;
        }
        x[u] = (w_on && row >= 0 && row < V) ? plane[row * W + w] : 0ull;
      }
#pragma unroll
      for (int u = 0; u < TALLY_UNROLL; ++u) vc_absorb(k, x[u]);
      k.absorbed += TALLY_UNROLL;
    }
  }
  if (cur_sl >= 0) block_flush(cur_sl);
}

// Sum the shards of scratch (n = nsl * 4096 entries each; entry m = message m) and leave them
// zero for the next count.  reach_out: the counts themselves (p2pg_message_reach); else the
// frontier of round `round`: reach += c, hop_sum += round * c, last_hop = round where c > 0.
// Entries at or above M (the last word's tail bits) are dropped.
__global__ __launch_bounds__(256) void k_tally_fold(unsigned long long* __restrict__ scratch, int shards,
                                                    int64_t n, int32_t M, int32_t round,
                                                    unsigned long long* __restrict__ reach_out,
                                                    unsigned long long* __restrict__ reach,
                                                    unsigned long long* __restrict__ hop_sum,
                                                    int32_t* __restrict__ last_hop) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned long long c = 0;
  for (int s = 0; s < shards; ++s) {
    c += scratch[(size_t)s * n + i];
    scratch[(size_t)s * n + i] = 0ull;
  }
  if (i >= M) return;
  if (reach_out) {
    reach_out[i] = c;
  } else if (c) {
    reach[i] += c;
    hop_sum[i] += c * (unsigned long long)round;
    last_hop[i] = round;
  }
}

// ---- per-peer counters ---------------------------------------------------------------------

// k_sends' helpers (relay_sends.hip), same tests.
__device__ __forceinline__ uint64_t prev_sends(const DevGraph& gp, const DevState& st, const RoundParams& p,
                                               const Netsplit& ns, int64_t v, int32_t y, int64_t slot, int w) {
  const int prv = (p.round & 1) ^ 1;
  if (gp.gone && gp.gone[slot]) return 0ull;
  if (!bit_test(st.A[prv], y)) return 0ull;
  if (link_cut(ns, p.round, v, y)) return 0ull;
  if (p.churn_thr && churn_dropped((uint32_t)(p.round - 1), gidx(gp, v), gidx(gp, y), p.churn_thr,
                                   p.cseed_lo, p.cseed_hi))
    return 0ull;
  return w < st.W ? st.F[prv][(int64_t)y * st.W + w] : 0ull;
}

// Slot of y in v's ascending gs row, or -1 (wave-uniform arguments).
__device__ __forceinline__ int64_t find_slot(const DevGraph& gs, int64_t beg, int64_t end, int32_t y) {
  int64_t lo = beg, hi = end;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (gs.colidx[mid] < y) lo = mid + 1; else hi = mid;
  }
  return (lo < end && gs.colidx[lo] == y) ? lo : -1;
}

// sent[v] += the send_to_node calls of v's round-r first receipts, received[u] += those of them
// addressed to u that are not lost (send_lost, device_util.h).  One wave per active peer v
// of round r = p.round, lane = word of a 64-word slice, the send set of k_sends:
// Flood: all n bits of a slice go to every connection (lane-parallel over the connections: one
//   add of n per connection), less, for r > 0, each bit's sender -- the lowest-id neighbour over
//   gp whose round-(r-1) send reached v (k_sends' walk: `rem` = bits whose sender is not found
//   yet).  Only a neighbour that IS some bit's sender costs a second wave sum and takes its bits
//   back off its own count (an add of -c: the counters are sums modulo 2^64, exact once the
//   pass is done).  In an arrival round of an anti-entropy exchange the partner whose reply arrived
//   at v is a sender of the bits the reply carried (pl).
// Gossip: deg <= k sends every bit to every connection (as flood, nobody excluded); else the
//   Philox picks are re-drawn, lane-balanced over a list of the slice's receipts, and aggregated
//   per connection in the wave's LDS table (rows of at most HUB_T connections), so the global
//   atomics are one per connection that was picked; wider rows add per pick.
__global__ __launch_bounds__(256) void k_peer_tally(DevGraph gs, DevGraph gp, DevState st, RoundParams p,
                                                    Downtime d, Netsplit ns, Pull pl,
                                                    unsigned long long* __restrict__ sent,
                                                    unsigned long long* __restrict__ received) {
  __shared__ uint32_t tab_all[WPB][HUB_T];
  __shared__ uint16_t lst_all[WPB][4096];  // a slice's set bits, as message indices within it
  const int lane = threadIdx.x & 63;
  const int wib = wave_in_block();
  uint32_t* tab = tab_all[wib];
  uint16_t* lst = lst_all[wib];
  const int cur = p.round & 1;
  const int W = st.W;
  const int nslices = (W + 63) >> 6;
  const int64_t ntasks = (gs.V + 31) >> 5;
  const bool same = gs.rowptr == gp.rowptr && gs.colidx == gp.colidx;
  for (int64_t task = (int64_t)blockIdx.x * WPB + wib; task < ntasks; task += (int64_t)gridDim.x * WPB) {
    uint32_t aw = st.A[cur][task];
    while (aw) {
      const int b = __builtin_ctz(aw);
      aw &= aw - 1u;
      const int64_t v = (task << 5) + b;
      const int64_t beg = gs.rowptr[v], end = gs.rowptr[v + 1];
      if (beg == end) continue;
      const uint32_t deg = (uint32_t)(end - beg);
      const bool picks = p.mode != 0 && (int)deg > p.fanout;
      const bool use_tab = picks && deg <= (uint32_t)HUB_T;
      unsigned long long v_sent = 0;  // wave-uniform
      // anti-entropy: the partner whose reply arrived at v in this round is a sender too (k_sends)
      const int32_t partner = pl.R && p.mode == 0 && bit_test(pl.PB, v) ? pull_partner(gp, pl, p.round - 2, v) : -1;
      if (use_tab) {
        for (uint32_t i = lane; i < deg; i += 64) tab[i] = 0u;
        wave_lds_sync();
      }
      for (int sl = 0; sl < nslices; ++sl) {
        const int w = sl * 64 + lane;
        const uint64_t f = w < W ? st.F[cur][v * W + w] : 0ull;
        const uint32_t n = wave_reduce_u32<false>((uint32_t)__popcll(f));
        if (!n) continue;
        if (!picks) {
          // every bit to every connection
          for (int64_t j0 = beg; j0 < end; j0 += 64) {
            const int64_t j = j0 + lane;
            if (j < end) {
              const int32_t u = gs.colidx[j];
              if (!send_lost(gs, p, d, ns, v, u, j)) atomicAdd(received + u, (unsigned long long)n);
            }
          }
          v_sent += (unsigned long long)n * deg;
          if (p.mode == 0 && p.round > 0) {
            // ... but a bit's sender
            uint64_t rem = f;
            const uint64_t pw = partner >= 0 ? pull_word(st, pl, v, w) : 0ull;
            const int64_t ep = gp.rowptr[v + 1];
            for (int64_t jp = gp.rowptr[v]; jp < ep && __ballot(rem != 0ull); ++jp) {
              const int32_t y = gp.colidx[jp];
              const uint64_t sy = prev_sends(gp, st, p, ns, v, y, jp, w) | (y == partner ? pw : 0ull);
              const uint64_t pu = rem & sy;
              rem &= ~sy;
              if (!__ballot(pu != 0ull)) continue;
              const uint32_t c = wave_reduce_u32<false>((uint32_t)__popcll(pu));
              const int64_t j = same ? jp : find_slot(gs, beg, end, y);
              if (j < 0) continue;  // no longer a connection: nothing was sent to it
              v_sent -= c;
              if (lane == 0 && !send_lost(gs, p, d, ns, v, y, j)) atomicAdd(received + y, 0ull - (unsigned long long)c);
            }
          }
        } else {
          // the slice's receipts as a list of message indices in LDS, so that every lane draws
          // for the same number of them (bits per word are uneven: a lane-per-word loop would run
          // as long as the fullest word)
          const uint32_t pc = (uint32_t)__popcll(f);
          uint32_t pos = wave_scan_u32(pc) - pc;
          uint64_t o = f;
          while (o) {
            lst[pos++] = (uint16_t)(lane * 64 + __builtin_ctzll(o));
            o &= o - 1ull;
          }
          wave_lds_sync();
          auto send = [&](uint32_t pick) {
            if (use_tab) {
              atomicAdd(&tab[pick], 1u);
            } else {
              const int64_t j = beg + (int64_t)pick;
              const int32_t u = gs.colidx[j];
              if (!send_lost(gs, p, d, ns, v, u, j)) atomicAdd(received + u, 1ull);
            }
          };
          auto draw = [&](auto kc) {  // fanout <= 4: one Philox block per receipt, picks in registers
            constexpr int K = decltype(kc)::value;
            const PickKey key = pick_key((uint32_t)p.round, gidx(gs, v), p.gseed_lo, p.gseed_hi);
            for (uint32_t i = lane; i < n; i += 64) {
              uint32_t pk[K];
              gossip_picks_k<K>(key, p.msg_base + (uint32_t)(sl * 4096) + lst[i], deg, pk);
#pragma unroll
              for (int q = 0; q < K; ++q) send(pk[q]);
            }
          };
          switch (p.fanout) {
            case 1: draw(std::integral_constant<int, 1>{}); break;
            case 2: draw(std::integral_constant<int, 2>{}); break;
            case 3: draw(std::integral_constant<int, 3>{}); break;
            case 4: draw(std::integral_constant<int, 4>{}); break;
            default:
              for (uint32_t i = lane; i < n; i += 64) {
                uint32_t pk[16];
                gossip_picks((uint32_t)p.round, gidx(gs, v), p.msg_base + (uint32_t)(sl * 4096) + lst[i], deg,
                             p.fanout, p.gseed_lo, p.gseed_hi, pk);
                for (int q = 0; q < p.fanout; ++q) send(pk[q]);
              }
          }
          wave_lds_sync();  // (the next slice rewrites the list)
          v_sent += (unsigned long long)n * (unsigned)p.fanout;
        }
      }
      if (use_tab) {
        wave_lds_sync();
        for (uint32_t i = lane; i < deg; i += 64) {
          const uint32_t c = tab[i];
          if (c) {
            const int64_t j = beg + i;
            const int32_t u = gs.colidx[j];
            if (!send_lost(gs, p, d, ns, v, u, j)) atomicAdd(received + u, (unsigned long long)c);
          }
        }
        wave_lds_sync();
      }
      if (lane == 0 && v_sent) atomicAdd(sent + v, v_sent);
    }
  }
}

// ---- per-message cost ----------------------------------------------------------------------

// Vertical counters that take a multi-bit addend: COST_PLANES planes hold up to COST_CAP per bit
// of the lane's word.  The addend is wave-uniform (a peer's degree, its connections that are not
// lost, the fanout), so each plane's operand is the mask or nothing: one full-adder step per plane,
// whatever the number of set bits.  A flood receipt's sender takes 1 back off (a ripple borrow).
constexpr int COST_PLANES = 8;
constexpr uint32_t COST_CAP = (1u << COST_PLANES) - 1u;
constexpr int COST_LIST = 2048;            // receipts listed per pass of the pick redraw
// A wave takes the block's LDS counts (32 bits) out to the shards before the weight it has added
// since it last did so passes this: 4 waves x 2^29 stay below 2^32 per count.
constexpr uint32_t COST_DRAIN = 1u << 29;
constexpr int COST_LDS_SHIFT = 5;           // one addend above COST_DRAIN >> 5 goes to the shards directly

struct WCount {
  uint64_t c[COST_PLANES];
};

__device__ __forceinline__ void wc_add(WCount& k, uint32_t wgt, uint64_t m) {
  uint64_t carry = 0ull;
#pragma unroll
  for (int i = 0; i < COST_PLANES; ++i) {
    const uint64_t a = k.c[i];
    const uint64_t b = ((wgt >> i) & 1u) ? m : 0ull;
    const uint64_t x = a ^ b;
    k.c[i] = x ^ carry;
    carry = (a & b) | (carry & x);
  }
}

__device__ __forceinline__ void wc_sub1(WCount& k, uint64_t m) {
  uint64_t borrow = m;
#pragma unroll
  for (int i = 0; i < COST_PLANES; ++i) {
    const uint64_t a = k.c[i];
    k.c[i] = a ^ borrow;
    borrow &= ~a;
  }
}

// LDS count of bit b of word `word` of the block's slice (k_colcount's rotation: the 64 lanes of
// one instruction spread over the banks).
__device__ __forceinline__ int cost_idx(int word, int b) { return word * 64 + ((b + word) & 63); }

// The lane's nonzero counts to its row of lds[64][64]; only the bits that hold something are
// visited (a tail round has one or two per word).
__device__ __forceinline__ void wc_flush(WCount& k, uint32_t* lds, int lane) {
  uint64_t any = 0ull;
#pragma unroll
  for (int i = 0; i < COST_PLANES; ++i) any |= k.c[i];
  while (any) {
    const int b = __builtin_ctzll(any);
    any &= any - 1ull;
    uint32_t v = 0u;
#pragma unroll
    for (int i = 0; i < COST_PLANES; ++i) v |= ((uint32_t)(k.c[i] >> b) & 1u) << i;
    atomicAdd(&lds[cost_idx(lane, b)], v);
  }
#pragma unroll
  for (int i = 0; i < COST_PLANES; ++i) k.c[i] = 0ull;
}

// sent[m] / received[m] of round r = p.round, per message instead of per peer: k_peer_tally's send
// set (same send_lost, gone slots, find_slot when gs != gp, anti-entropy partner), summed over the
// bit columns of the frontier rows.  Block items are slice-major as in k_colcount (one 64-word
// slice at a time, the block's LDS counts leave when its slice changes); a wave's task is the
// active peers of one 32-peer word of A, lane = word of the slice.  Per peer v and word f:
// Flood, and gossip with deg <= k: every bit adds deg to sent and nl(v) -- v's connections whose
//   send is not lost, counted once per peer -- to received; in flood rounds r > 0 a bit whose sender
//   (k_peer_tally's walk) is still a connection takes 1 back off sent, and off received if the send
//   towards that sender would not have been lost.
// Gossip, deg > k: every bit adds k to sent.  If none of v's connections loses its send (always so
//   without churn, removed slots and downtime) it adds k to received as well and no pick is drawn;
//   else the picks are re-drawn over a lane-balanced list of the slice's receipts and each receipt
//   adds its picks that are not lost (looked up in the peer's bitmap of lost connections; rows
//   above HUB_T connections test per pick), one LDS atomic per receipt.
// Addends above COST_CAP (hubs) skip the vertical counters: one LDS atomic per set bit and counter,
// or, above drain_at >> COST_LDS_SHIFT (2^24 connections), one 64-bit atomic into the shard.
// drain_at: COST_DRAIN (a launch argument so that a test can reach the drain and that last path).
__global__ __launch_bounds__(256) void k_msg_cost(DevGraph gs, DevGraph gp, DevState st, RoundParams p,
                                                  Downtime d, Netsplit ns, Pull pl, unsigned long long* __restrict__ scratch,
                                                  int shards, uint32_t drain_at) {
  __shared__ uint32_t lds_s[64 * 64];
  __shared__ uint32_t lds_r[64 * 64];
  __shared__ uint16_t lst_all[WPB][COST_LIST];
  __shared__ uint32_t lostmap_all[WPB][HUB_T / 32];
  const int lane = threadIdx.x & 63;
  const int wib = wave_in_block();
  uint16_t* lst = lst_all[wib];
  uint32_t* lostmap = lostmap_all[wib];
  const int cur = p.round & 1;
  const int W = st.W;
  const int nsl = (W + 63) >> 6;
  const size_t nmsg = (size_t)nsl * 4096;
  const int64_t ntasks = (gs.V + 31) >> 5;
  const int64_t nbt = (ntasks + WPB - 1) / WPB;
  const int64_t nitems = nbt * nsl;
  const bool same = gs.rowptr == gp.rowptr && gs.colidx == gp.colidx;
  const bool lossless = !gs.gone && !p.churn_thr && !d.from && !ns.side;
  const uint32_t lds_max = drain_at >> COST_LDS_SHIFT;
  unsigned long long* out_s = scratch + (size_t)(blockIdx.x & (shards - 1)) * (2 * nmsg);
  unsigned long long* out_r = out_s + nmsg;
  WCount ks, kr;
#pragma unroll
  for (int i = 0; i < COST_PLANES; ++i) ks.c[i] = kr.c[i] = 0ull;
  uint32_t held = 0u;   // upper bound of any count in ks / kr (wave-uniform)
  uint32_t added = 0u;  // upper bound of what this wave added to any LDS count since its last drain
  for (int i = threadIdx.x; i < 64 * 64; i += 256) lds_s[i] = lds_r[i] = 0u;
  __syncthreads();
  // LDS index i of slice sl -> entry of a shard (word-major, unrotated)
  auto shard_at = [&](int sl, int i) -> int64_t {
    const int word = i >> 6;
    const int gw = sl * 64 + word;
    return gw < W ? (int64_t)gw * 64 + (((i & 63) - word) & 63) : -1;
  };
  // Takes whatever the LDS counts hold out to the shards.  Exchanges, so any wave may do it while
  // the others keep adding: an add lands before the exchange or after it.
  auto drain = [&](int sl, int first, int step) {
    for (int i = first; i < 64 * 64; i += step) {
      const int64_t at = shard_at(sl, i);
      const uint32_t vs = lds_s[i] ? atomicExch(&lds_s[i], 0u) : 0u;
      const uint32_t vr = lds_r[i] ? atomicExch(&lds_r[i], 0u) : 0u;
      if (vs && at >= 0) atomicAdd(out_s + at, (unsigned long long)vs);
      if (vr && at >= 0) atomicAdd(out_r + at, (unsigned long long)vr);
    }
  };
  auto block_flush = [&](int sl) {  // block-uniform calls only; leaves the LDS counts zero
    wc_flush(ks, lds_s, lane);
    wc_flush(kr, lds_r, lane);
    held = 0u;
    __syncthreads();
    drain(sl, threadIdx.x, 256);
    added = 0u;
    __syncthreads();
  };
  // before an addend of wgt per bit: room in the vertical counters and in the LDS counts
  auto make_room = [&](int sl, uint32_t wgt) {
    if (wgt > lds_max) return;  // (add_wide: straight to the shards)
    if (wgt <= COST_CAP && held + wgt > COST_CAP) {
      wc_flush(ks, lds_s, lane);
      wc_flush(kr, lds_r, lane);
      held = 0u;
    }
    if (added + wgt > drain_at) {
      wc_flush(ks, lds_s, lane);
      wc_flush(kr, lds_r, lane);
      held = 0u;
      wave_lds_sync();
      drain(sl, lane, 64);
      added = 0u;
    }
    added += wgt;
    if (wgt <= COST_CAP) held += wgt;
  };
  // a peer whose degree is above COST_CAP: wgt, or wgt - 1 under less1, per set bit of f
  auto add_wide = [&](int sl, uint32_t* lds, unsigned long long* out, uint64_t f, uint32_t wgt, uint64_t less1,
                      bool to_lds) {
    while (f) {
      const int b = __builtin_ctzll(f);
      f &= f - 1ull;
      const uint32_t v = wgt - (uint32_t)((less1 >> b) & 1ull);
      if (!v) continue;
      if (to_lds) {
        atomicAdd(&lds[cost_idx(lane, b)], v);
      } else {
        const int gw = sl * 64 + lane;
        atomicAdd(out + (int64_t)gw * 64 + b, (unsigned long long)v);  // (f != 0: gw < W)
      }
    }
  };
  int cur_sl = -1;
  for (int64_t bi = blockIdx.x; bi < nitems; bi += gridDim.x) {
    const int sl = (int)(bi / nbt);
    if (sl != cur_sl) {
      if (cur_sl >= 0) block_flush(cur_sl);
      cur_sl = sl;
    }
    const int64_t task = (bi - (int64_t)sl * nbt) * WPB + wib;
    if (task >= ntasks) continue;
    const int w = sl * 64 + lane;
    uint32_t aw = st.A[cur][task];
    while (aw) {
      const int b = __builtin_ctz(aw);
      aw &= aw - 1u;
      const int64_t v = (task << 5) + b;
      const int64_t beg = gs.rowptr[v], end = gs.rowptr[v + 1];
      if (beg == end) continue;
      const uint64_t f = w < W ? st.F[cur][v * W + w] : 0ull;
      if (!__ballot(f != 0ull)) continue;
      const uint32_t deg = (uint32_t)(end - beg);
      const bool picks = p.mode != 0 && (int)deg > p.fanout;
      // v's connections whose send is lost, tested once per connection: their number, and for a
      // peer that draws picks (rows of at most HUB_T connections) their bitmap in LDS
      const bool use_map = picks && deg <= (uint32_t)HUB_T;
      uint32_t nlost = 0u;
      if (!lossless) {
        for (int64_t j0 = beg; j0 < end; j0 += 64) {
          const int64_t j = j0 + lane;
          const uint64_t bal = __ballot(j < end && send_lost(gs, p, d, ns, v, gs.colidx[j], j));
          nlost += (uint32_t)__popcll(bal);
          if (use_map && lane < 2) lostmap[((j0 - beg) >> 5) + lane] = (uint32_t)(bal >> (32 * lane));
        }
        if (use_map) wave_lds_sync();
      }
      if (!picks) {
        const uint32_t nl = deg - nlost;  // connections whose send is not lost
        uint64_t ex_s = 0ull, ex_r = 0ull;  // bits whose sender gets no copy / would have got one
        if (p.mode == 0 && p.round > 0) {
          const int32_t partner = pl.R && bit_test(pl.PB, v) ? pull_partner(gp, pl, p.round - 2, v) : -1;
          uint64_t rem = f;
          const uint64_t pw = partner >= 0 ? pull_word(st, pl, v, w) : 0ull;
          const int64_t ep = gp.rowptr[v + 1];
          for (int64_t jp = gp.rowptr[v]; jp < ep && __ballot(rem != 0ull); ++jp) {
            const int32_t y = gp.colidx[jp];
            const uint64_t sy = prev_sends(gp, st, p, ns, v, y, jp, w) | (y == partner ? pw : 0ull);
            const uint64_t pu = rem & sy;
            rem &= ~sy;
            if (!__ballot(pu != 0ull)) continue;
            const int64_t j = same ? jp : find_slot(gs, beg, end, y);
            if (j < 0) continue;  // no longer a connection: nothing was sent to it
            ex_s |= pu;
            if (!send_lost(gs, p, d, ns, v, y, j)) ex_r |= pu;
          }
        }
        make_room(sl, deg);
        if (deg <= COST_CAP && deg <= lds_max) {
          wc_add(ks, deg, f);
          wc_sub1(ks, ex_s);
          wc_add(kr, nl, f);
          wc_sub1(kr, ex_r);  // (a sender whose copy is not lost is one of the nl)
        } else {
          add_wide(sl, lds_s, out_s, f, deg, ex_s, deg <= lds_max);
          add_wide(sl, lds_r, out_r, f, nl, ex_r, deg <= lds_max);
        }
      } else {
        const uint32_t k = (uint32_t)p.fanout;  // <= 16
        make_room(sl, k);
        wc_add(ks, k, f);
        if (!nlost) {  // every pick arrives, whichever it is
          wc_add(kr, k, f);
          continue;
        }
        // the slice's receipts as a list of message indices in LDS (k_peer_tally), COST_LIST per pass
        const uint32_t pc = (uint32_t)__popcll(f);
        const uint32_t pos0 = wave_scan_u32(pc) - pc;
        const uint32_t n = (uint32_t)__builtin_amdgcn_readlane((int)(pos0 + pc), 63);
        auto count = [&](uint32_t m, const uint32_t* pk, int K) {
          uint32_t c = 0u;
          for (int q = 0; q < K; ++q) {
            if (use_map) {
              c += 1u - ((lostmap[pk[q] >> 5] >> (pk[q] & 31u)) & 1u);
            } else {
              const int64_t j = beg + (int64_t)pk[q];
              if (!send_lost(gs, p, d, ns, v, gs.colidx[j], j)) ++c;
            }
          }
          if (c) atomicAdd(&lds_r[cost_idx((int)(m >> 6), (int)(m & 63u))], c);
        };
        for (uint32_t base = 0; base < n; base += COST_LIST) {
          uint32_t pos = pos0 - base;  // (wraps below the window: never < COST_LIST then)
          uint64_t o = f;
          while (o) {
            if (pos < (uint32_t)COST_LIST) lst[pos] = (uint16_t)(lane * 64 + __builtin_ctzll(o));
            ++pos;
            o &= o - 1ull;
          }
          wave_lds_sync();
          const uint32_t cnt = n - base < (uint32_t)COST_LIST ? n - base : (uint32_t)COST_LIST;
          auto draw = [&](auto kc) {  // fanout <= 4: one Philox block per receipt
            constexpr int K = decltype(kc)::value;
            const PickKey key = pick_key((uint32_t)p.round, gidx(gs, v), p.gseed_lo, p.gseed_hi);
            for (uint32_t i = lane; i < cnt; i += 64) {
              uint32_t pk[K];
              const uint32_t m = lst[i];
              gossip_picks_k<K>(key, p.msg_base + (uint32_t)(sl * 4096) + m, deg, pk);
              count(m, pk, K);
            }
          };
          switch (p.fanout) {
            case 1: draw(std::integral_constant<int, 1>{}); break;
            case 2: draw(std::integral_constant<int, 2>{}); break;
            case 3: draw(std::integral_constant<int, 3>{}); break;
            case 4: draw(std::integral_constant<int, 4>{}); break;
            default:
              for (uint32_t i = lane; i < cnt; i += 64) {
                uint32_t pk[16];
                const uint32_t m = lst[i];
                gossip_picks((uint32_t)p.round, gidx(gs, v), p.msg_base + (uint32_t)(sl * 4096) + m, deg, p.fanout,
                             p.gseed_lo, p.gseed_hi, pk);
                count(m, pk, p.fanout);
              }
          }
          wave_lds_sync();  // (the next pass rewrites the list)
        }
      }
    }
  }
  if (cur_sl >= 0) block_flush(cur_sl);
}

// sent[m] += / received[m] += the shards' sums (n entries per counter and shard; entry m = message
// m), which are left zero for the next round.  Entries at or above M hold nothing.
__global__ __launch_bounds__(256) void k_cost_fold(unsigned long long* __restrict__ scratch, int shards, int64_t n,
                                                   int32_t M, unsigned long long* __restrict__ sent,
                                                   unsigned long long* __restrict__ received) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned long long cs = 0, cr = 0;
  for (int s = 0; s < shards; ++s) {
    unsigned long long* sh = scratch + (size_t)s * (2 * (size_t)n);
    cs += sh[i];
    cr += sh[n + i];
    sh[i] = 0ull;
    sh[n + i] = 0ull;
  }
  if (i >= M) return;
  if (cs) sent[i] += cs;
  if (cr) received[i] += cr;
}

}  // namespace

int64_t cost_scratch_words(int32_t W) { return (int64_t)TALLY_SHARDS * 2 * ((W + 63) / 64) * 4096; }

hipError_t launch_msg_cost(const DevGraph& gs, const DevGraph& gp, const DevState& st, const RoundParams& p,
                           const Downtime& d, const Netsplit& ns, const Pull& pl, unsigned long long* scratch,
                           unsigned long long* sent, unsigned long long* received, hipStream_t s) {
  if (gs.V <= 0 || st.W <= 0) return hipSuccess;
  static const uint32_t drain_at = [] {  // P2PG_COST_DRAIN: the tests' way to the LDS drain
    const char* e = std::getenv("P2PG_COST_DRAIN");
    const long v = e ? std::atol(e) : 0;
    // (at least 16 << COST_LDS_SHIFT: the fanout always goes through the vertical counters)
    return v >= (16l << COST_LDS_SHIFT) && v < (long)COST_DRAIN ? (uint32_t)v : COST_DRAIN;
  }();
  const int nsl = (st.W + 63) / 64;
  const int64_t n = (int64_t)nsl * 4096;
  const int64_t nbt = (((gs.V + 31) >> 5) + WPB - 1) / WPB;
  hipLaunchKernelGGL(k_msg_cost, dim3(grid_tasks(nbt * nsl * WPB)), dim3(256), 0, s, gs, gp, st, p, d, ns, pl, scratch,
                     TALLY_SHARDS, drain_at);
  hipError_t r = hipGetLastError();
  if (r != hipSuccess) return r;
  hipLaunchKernelGGL(k_cost_fold, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, scratch, TALLY_SHARDS, n,
                     st.M, sent, received);
  return hipGetLastError();
}

int64_t tally_scratch_words(int32_t W) { return (int64_t)TALLY_SHARDS * ((W + 63) / 64) * 4096; }

hipError_t launch_frontier_count(const uint64_t* plane, const uint32_t* A, int64_t V, int32_t W,
                                 unsigned long long* scratch, hipStream_t s) {
  if (V <= 0 || W <= 0) return hipSuccess;
  const int nsl = (W + 63) / 64;
  const int64_t nbt = (((V + 31) >> 5) + WPB - 1) / WPB;
  hipLaunchKernelGGL(k_colcount<true>, dim3(grid_tasks(nbt * nsl * WPB)), dim3(256), 0, s, plane, A, V, W,
                     scratch, TALLY_SHARDS);
  return hipGetLastError();
}

hipError_t launch_tally_fold(unsigned long long* scratch, int32_t W, int32_t M, int32_t round,
                             unsigned long long* reach_out, unsigned long long* reach,
                             unsigned long long* hop_sum, int32_t* last_hop, hipStream_t s) {
  if (W <= 0) return hipSuccess;
  const int64_t n = (int64_t)((W + 63) / 64) * 4096;
  hipLaunchKernelGGL(k_tally_fold, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, scratch, TALLY_SHARDS, n,
                     M, round, reach_out, reach, hop_sum, last_hop);
  return hipGetLastError();
}

hipError_t launch_column_count(const uint64_t* plane, const uint32_t* A, int64_t V, int32_t W, int32_t M,
                               int32_t round, unsigned long long* scratch, unsigned long long* reach_out,
                               unsigned long long* reach, unsigned long long* hop_sum, int32_t* last_hop,
                               hipStream_t s) {
  if (V <= 0 || W <= 0) return hipSuccess;
  hipError_t r;
  if (A) {
    r = launch_frontier_count(plane, A, V, W, scratch, s);
  } else {
    const int nsl = (W + 63) / 64;
    const int64_t nbt = ((V + TALLY_ROWS - 1) / TALLY_ROWS + WPB - 1) / WPB;
    hipLaunchKernelGGL(k_colcount<false>, dim3(grid_tasks(nbt * nsl * WPB)), dim3(256), 0, s, plane, A, V, W,
                       scratch, TALLY_SHARDS);
    r = hipGetLastError();
  }
  if (r != hipSuccess) return r;
  return launch_tally_fold(scratch, W, M, round, reach_out, reach, hop_sum, last_hop, s);
}

hipError_t launch_peer_tally(const DevGraph& gs, const DevGraph& gp, const DevState& st, const RoundParams& p,
                             const Downtime& d, const Netsplit& ns, const Pull& pl, unsigned long long* sent,
                             unsigned long long* received, hipStream_t s) {
  hipLaunchKernelGGL(k_peer_tally, dim3(grid_tasks((gs.V + 31) >> 5)), dim3(256), 0, s, gs, gp, st, p, d, ns, pl, sent,
                     received);
  return hipGetLastError();
}

}  // namespace p2pg
