// Pass plan of a wide sender's push in the fused gossip round (k_gossip_fused).
//
// A sender of 16 < deg <= 512 connections pushes through one wave's LDS mask table of
// PLAN_CELLS u32 cells = PLAN_MASKS (connection, word) masks of two halves each.  Its
// connections are cut into groups of at most PLAN_GROUP; inside a group its ACTIVE words (the
// set bits of the row's active-word mask, counted by rank = position in the packed E row) are
// cut into passes, so that every pass -- conns x seg masks, seg = the pass's words rounded up to
// a flush segment -- fits the table.  Every (peer, message) pick is then evaluated once per
// group, not once per 16-connection chunk.
//
// Plain C++: included by the kernel and by host programs (tests/test_pass_plan.py).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PASS_PLAN_HD __host__ __device__ inline
#else
#define PASS_PLAN_HD inline
#endif

constexpr int PLAN_CELLS = 2048;             // u32 cells of the table (GCHUNK * 128)
constexpr int PLAN_MASKS = PLAN_CELLS / 2;   // (connection, word) masks of one pass
constexpr int PLAN_GROUP = 64;               // connections per group (one 64-slot rev[] load)

// connection groups of a sender: group g covers connections [plan_group_begin, + plan_group_conns)
PASS_PLAN_HD int plan_groups(int deg) { return (deg + PLAN_GROUP - 1) / PLAN_GROUP; }
PASS_PLAN_HD int plan_group_begin(int g) { return g * PLAN_GROUP; }
PASS_PLAN_HD int plan_group_conns(int deg, int g) {
  const int c = deg - g * PLAN_GROUP;
  return c < PLAN_GROUP ? c : PLAN_GROUP;
}

// active words one pass of a group of `conns` connections may hold: a power of two (a flush
// segment), conns * words <= PLAN_MASKS
PASS_PLAN_HD int plan_pass_words(int conns) { return conns <= 16 ? 64 : conns <= 32 ? 32 : 16; }

// passes of a group over a row of `nactive` active words; pass p covers the ranks
// [plan_pass_rank0, + plan_pass_ranks)
PASS_PLAN_HD int plan_passes(int conns, int nactive) {
  const int wp = plan_pass_words(conns);
  return (nactive + wp - 1) / wp;
}
PASS_PLAN_HD int plan_pass_rank0(int conns, int p) { return p * plan_pass_words(conns); }
PASS_PLAN_HD int plan_pass_ranks(int conns, int nactive, int p) {
  const int wp = plan_pass_words(conns);
  const int r = nactive - p * wp;
  return r < wp ? r : wp;
}

// flush segment of a pass of `ranks` words: lane l serves rank l % seg of connection l / seg, one
// store instruction covers 64 / seg connections; the pass's table is conns * seg masks
PASS_PLAN_HD int plan_seg(int ranks) { return ranks <= 16 ? 16 : ranks <= 32 ? 32 : 64; }
PASS_PLAN_HD int plan_pass_cells(int conns, int ranks) { return conns * plan_seg(ranks) * 2; }
// store instructions of a pass's flush
PASS_PLAN_HD int plan_flush_count(int conns, int ranks) {
  const int per = 64 / plan_seg(ranks);
  return (conns + per - 1) / per;
}

// the words (a sub-mask of the active-word mask `fam`) whose ranks are [rank0, rank0 + ranks)
PASS_PLAN_HD uint64_t plan_rank_words(uint64_t fam, int rank0, int ranks) {
  uint64_t out = 0;
  int r = 0;
  for (uint64_t m = fam; m; m &= m - 1, ++r)
    if (r >= rank0 && r < rank0 + ranks) out |= m & (~m + 1);
  return out;
}
