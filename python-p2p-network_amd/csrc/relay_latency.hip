// Delivery latency computed on the device (P2PG_FLAG_LATENCY: p2pg_message_latency /
// p2pg_peer_latency).  A first receipt of message m in round r has the relative hop
// h = r - start[m]; both passes read the round's final frontier rows F[r&1] under A[r&1], at the
// point of the tally's column count:
//   * k_latency_fold: the per-message counts of the round's frontier (k_colcount<true>'s shard
//     scratch, relay_tally.hip) binned by min(h, bins - 1) into hist[M][bins];
//   * k_peer_latency: per peer the sum, the number and the largest of the relative hops of its
//     first receipts, from the bit-sliced start planes of latency.h -- no per-bit loop.
// Opt-in passes outside the rounds' own kernels.  Internal; not part of the C-ABI.
#include "device_util.h"
#include "latency.h"

namespace p2pg {
namespace {

constexpr int LAT_UNROLL = 4;  // row loads in flight per lane (k_colcount's TALLY_UNROLL)

// hist[m * bins + min(round - start[m], bins - 1)] += the shards' sum of entry m (n = nsl * 4096
// entries per shard; entry m = message m).  zero: leave the shards zero for the next count (an
// engine without P2PG_FLAG_TALLY); else k_tally_fold, which runs next on the same scratch, does.
__global__ __launch_bounds__(256) void k_latency_fold(unsigned long long* __restrict__ scratch, int shards,
                                                      int64_t n, int32_t M, int32_t round,
                                                      const int32_t* __restrict__ start, int32_t bins,
                                                      unsigned long long* __restrict__ hist, bool zero) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned long long c = 0;
  for (int s = 0; s < shards; ++s) {
    c += scratch[(size_t)s * n + i];
    if (zero) scratch[(size_t)s * n + i] = 0ull;
  }
  if (i >= M || !c) return;
  const int32_t st = start[i] > 0 ? start[i] : 0;
  hist[(size_t)i * bins + latency::bin_of(round - st, bins)] += c;
}

// Inclusive scan over the W-lane segment of a row (wl = the lane's position in it): afterwards the
// segment's last lane holds its total.  Every lane of the wave takes part in the shuffles.
template <class T, class Op>
__device__ __forceinline__ T seg_scan(T x, int wl, int SW, Op op) {
  for (int d = 1; d < SW; d <<= 1) {
    const T y = __shfl_up(x, d);
    if (wl >= d) x = op(x, y);
  }
  return x;
}

__device__ __forceinline__ void peer_add(PeerLat* __restrict__ out, int64_t v, unsigned long long hop_sum,
                                         uint32_t receipts, uint32_t max1) {
  PeerLat p = out[v];
  p.hop_sum += hop_sum;
  p.receipts += receipts;
  p.max1 = p.max1 > max1 ? p.max1 : max1;
  out[v] = p;
}

// out[v] takes in v's first receipts of round `round`: their number, the sum of their relative
// hops and the largest of them (as max1 = hop + 1; 0 = no receipt yet).  One pass over the frontier
// rows under A; a wave's task is the active peers of one 32-peer word of A, lane <-> word of a row
// as in k_colcount:
//   WIDE (W >= 64): a wave load is one 64-word slice of one row, LAT_UNROLL rows in flight; a row's
//     slices all go to the same wave (the lanes accumulate over them), then one whole-wave
//     reduction per row;
//   else: 64 / W whole rows per load (select_bit32 on the A word), LAT_UNROLL loads in flight, and
//     a segmented scan over the W lanes of a row; the lanes past (64 / W) * W take no row.
// Exactly one wave owns a peer within a launch, and a peer has at most one frontier row per round:
// the counters are updated by plain vector read-modify-write, no atomics.
// B = 0 (every start is 0): a word's relative-hop sum is round * popcount and the largest hop is
// the round -- the planes S are not read.
template <bool WIDE>
__global__ __launch_bounds__(256) void k_peer_latency(const uint64_t* __restrict__ F,
                                                      const uint32_t* __restrict__ A, int64_t V, int W,
                                                      int32_t round, const uint64_t* __restrict__ S, int B,
                                                      PeerLat* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wib = wave_in_block();
  const int64_t ntasks = (V + 31) >> 5;
  const uint32_t r1 = (uint32_t)round + 1u;
  auto umax = [](uint32_t a, uint32_t b) { return a > b ? a : b; };
  if (WIDE) {
    const int nsl = (W + 63) >> 6;
    for (int64_t task = (int64_t)blockIdx.x * WPB + wib; task < ntasks; task += (int64_t)gridDim.x * WPB) {
      uint32_t rest = (uint32_t)__builtin_amdgcn_readfirstlane((int)A[task]);
      while (rest) {
        int64_t row[LAT_UNROLL];  // wave-uniform
#pragma unroll
        for (int u = 0; u < LAT_UNROLL; ++u) {
          row[u] = -1;
          if (rest) {
            const int64_t v = (task << 5) + __builtin_ctz(rest);
            rest &= rest - 1u;
            if (v < V) row[u] = v;
          }
        }
        uint32_t cnt[LAT_UNROLL], mx[LAT_UNROLL];
        uint64_t ssum[LAT_UNROLL];
#pragma unroll
        for (int u = 0; u < LAT_UNROLL; ++u) {
          cnt[u] = mx[u] = 0u;
          ssum[u] = 0ull;
        }
        for (int sl = 0; sl < nsl; ++sl) {
          const int w = sl * 64 + lane;
          uint64_t x[LAT_UNROLL];
#pragma unroll
          for (int u = 0; u < LAT_UNROLL; ++u) x[u] = (w < W && row[u] >= 0) ? F[row[u] * W + w] : 0ull;
#pragma unroll
          for (int u = 0; u < LAT_UNROLL; ++u) {
            cnt[u] += (uint32_t)__popcll(x[u]);
            if (B && x[u]) {  // (x != 0: w < W)
              ssum[u] += latency::start_sum(x[u], S + w, W, B);
              mx[u] = umax(mx[u], r1 - latency::start_min(x[u], S + w, W, B));
            }
          }
        }
        // lane u takes row u's totals to its counters
        int64_t my_row = -1;
        uint32_t my_c = 0u, my_m = 0u;
        unsigned long long my_h = 0ull;
#pragma unroll
        for (int u = 0; u < LAT_UNROLL; ++u) {
          if (row[u] < 0) continue;  // (wave-uniform)
          const uint32_t c = wave_reduce_u32<false>(cnt[u]);
          unsigned long long h = (unsigned long long)(uint32_t)round * c;
          uint32_t m = r1;
          if (B) {
            h -= wave_sum(ssum[u]);
            m = wave_reduce_u32<true>(mx[u]);
          }
          if (lane == u) {
            my_row = row[u];
            my_c = c;
            my_h = h;
            my_m = m;
          }
        }
        if (my_row >= 0 && my_c) peer_add(out, my_row, my_h, my_c, my_m);
      }
    }
  } else {
    const int R = 64 / W;  // rows per wave load
    const int wl = lane % W, ro = lane / W;
    const bool lane_on = ro < R;
    for (int64_t task = (int64_t)blockIdx.x * WPB + wib; task < ntasks; task += (int64_t)gridDim.x * WPB) {
      uint32_t rest = (uint32_t)__builtin_amdgcn_readfirstlane((int)A[task]);
      while (rest) {
        int64_t row[LAT_UNROLL];
        uint64_t x[LAT_UNROLL];
#pragma unroll
        for (int u = 0; u < LAT_UNROLL; ++u) {
          // this load takes the R lowest peers still in `rest`; the lane's is the ro-th of them
          const int np = __popc(rest);
          row[u] = -1;
          if (lane_on && ro < np) {
            const int64_t v = (task << 5) + (R == 1 ? (uint32_t)__builtin_ctz(rest) : select_bit32(rest, (uint32_t)ro));
            if (v < V) row[u] = v;
          }
          for (int q = 0; q < R && rest; ++q) rest &= rest - 1u;
          x[u] = row[u] >= 0 ? F[row[u] * W + wl] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < LAT_UNROLL; ++u) {
          if (!__ballot(row[u] >= 0)) continue;  // (wave-uniform: the shuffles below see every lane)
          const uint32_t c =
              seg_scan((uint32_t)__popcll(x[u]), wl, W, [](uint32_t a, uint32_t b) { return a + b; });
          unsigned long long h = (unsigned long long)(uint32_t)round * c;
          uint32_t m = r1;
          if (B) {
            const uint64_t s1 = x[u] ? latency::start_sum(x[u], S + wl, W, B) : 0ull;
            const uint32_t m1 = x[u] ? r1 - latency::start_min(x[u], S + wl, W, B) : 0u;
            h -= seg_scan(s1, wl, W, [](uint64_t a, uint64_t b) { return a + b; });
            m = seg_scan(m1, wl, W, umax);
          }
          if (row[u] >= 0 && wl == W - 1 && c) peer_add(out, row[u], h, c, m);
        }
      }
    }
  }
}

}  // namespace

hipError_t launch_latency_fold(unsigned long long* scratch, int32_t W, int32_t M, int32_t round,
                               const int32_t* start, int32_t bins, unsigned long long* hist, bool zero,
                               hipStream_t s) {
  if (W <= 0) return hipSuccess;
  const int64_t n = (int64_t)((W + 63) / 64) * 4096;
  hipLaunchKernelGGL(k_latency_fold, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, scratch, TALLY_SHARDS, n, M,
                     round, start, bins, hist, zero);
  return hipGetLastError();
}

hipError_t launch_peer_latency(const DevState& st, int64_t V, int32_t round, const uint64_t* S, int32_t B,
                               PeerLat* out, hipStream_t s) {
  if (V <= 0 || st.W <= 0) return hipSuccess;
  const dim3 grid(grid_tasks((V + 31) >> 5));
  const uint64_t* F = st.F[round & 1];
  const uint32_t* A = st.A[round & 1];
  if (st.W >= 64)
    hipLaunchKernelGGL(k_peer_latency<true>, grid, dim3(256), 0, s, F, A, V, st.W, round, S, B, out);
  else
    hipLaunchKernelGGL(k_peer_latency<false>, grid, dim3(256), 0, s, F, A, V, st.W, round, S, B, out);
  return hipGetLastError();
}

}  // namespace p2pg
