// Delivery latency (P2PG_FLAG_LATENCY): the start rounds of the messages as
// bit-sliced planes, so that a pass over a frontier row needs no per-bit loop.  Plane b holds, per
// 64-message word w, the mask S[b][w] of the messages of that word whose start round has bit b
// set; B = the number of bits of the largest scheduled start (0: every start is 0, no planes).
// Unscheduled messages (start -1) count as 0: they never have a frontier bit.  For a frontier
// word f of word w:
//   sum of the starts under f     = sum_b popcount(f & S[b][w]) << b
//   smallest start under f        = the bit-sliced minimum: from the top plane down, the
//                                   candidates whose bit b is clear stay if there are any
// from which the word's relative hops follow: sum = round * popcount(f) - sum of starts, largest
// = round - smallest start.
//
// Plain C++: included by engine.cpp (the planes are built on the host), by relay_latency.hip (the
// per-word functions) and by host programs (tests/test_latency_host.py).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LATENCY_HD __host__ __device__ inline
#else
#define LATENCY_HD inline
#endif

namespace latency {

constexpr int32_t BINS_DEFAULT = 64;
constexpr int32_t BINS_MIN = 2;
constexpr int32_t BINS_MAX = 1024;

LATENCY_HD int popcount64(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(x);
#else
  return __builtin_popcountll(x);
#endif
}

// Planes needed for starts up to max_start: its number of bits (0 for max_start <= 0).
LATENCY_HD int plane_bits(int32_t max_start) {
  int b = 0;
  if (max_start <= 0) return 0;
  while (b < 31 && (max_start >> b) != 0) ++b;
  return b;
}

// The largest start of a schedule (0 for an empty one or one without a positive start).
inline int32_t max_start(int32_t M, const int32_t* start) {
  int32_t mx = 0;
  for (int32_t m = 0; m < M; ++m)
    if (start[m] > mx) mx = start[m];
  return mx;
}

// out[b * W + w], b < B: the planes of start[0 .. M-1] (B >= plane_bits of their maximum; bits at
// or above M stay clear).  Writes B * W words.
inline void build_start_planes(int32_t M, int32_t W, const int32_t* start, int B, uint64_t* out) {
  for (size_t i = 0; i < (size_t)B * (size_t)W; ++i) out[i] = 0ull;
  for (int32_t m = 0; m < M; ++m) {
    const int32_t s = start[m];
    if (s <= 0) continue;
    for (int b = 0; b < B; ++b)
      if ((s >> b) & 1) out[(size_t)b * W + (m >> 6)] |= 1ull << (m & 63);
  }
}

// The bin of a relative hop h >= 0: the last bin collects the overflow.
LATENCY_HD int32_t bin_of(int32_t h, int32_t bins) { return h < bins - 1 ? (h < 0 ? 0 : h) : bins - 1; }

// Sw = the planes at the word's column (&S[0][w]), stride W between planes.
// Sum of the starts of the messages under f.
LATENCY_HD uint64_t start_sum(uint64_t f, const uint64_t* Sw, int32_t W, int B) {
  uint64_t s = 0ull;
  for (int b = 0; b < B; ++b) s += (uint64_t)popcount64(f & Sw[(size_t)b * W]) << b;
  return s;
}

// The smallest start among the messages under f; f != 0.
LATENCY_HD uint32_t start_min(uint64_t f, const uint64_t* Sw, int32_t W, int B) {
  uint64_t cand = f;
  uint32_t mn = 0u;
  for (int b = B - 1; b >= 0; --b) {
    const uint64_t t = cand & ~Sw[(size_t)b * W];
    if (t)
      cand = t;  // somebody has bit b clear: only they can be the minimum
    else
      mn |= 1u << b;
  }
  return mn;
}

}  // namespace latency
