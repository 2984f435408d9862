// Network partition (p2pg_set_netsplit): the host's side of the netsplit.  Every peer
// has a side, side[v] >= 0, and there is one window of rounds [cut_from, cut_until).  Connection
// {a, b} is cut in round t iff side[a] != side[b] and cut_from <= t < cut_until; a send of round r
// over a connection that is cut in round r + 1, the round it would arrive in, is lost.  Here: the
// one definition of "cut in round t" (the kernels evaluate the same function), the validation of
// the call's arguments, the two questions the schedule asks about the window, and the count of the
// connections that cross sides (none: the setting is no setting).
//
// Plain C++: included by engine.cpp, by the kernels (the predicate only) and by host programs
// (tests/netsplit_check.cpp).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NETSPLIT_HD __host__ __device__ inline
#else
#define NETSPLIT_HD inline
#endif

namespace netsplit {

// Is round t inside the window?
NETSPLIT_HD bool in_window(int32_t t, int32_t cut_from, int32_t cut_until) { return cut_from <= t && t < cut_until; }

// Is a connection between a peer of side_a and a peer of side_b cut in round t?
NETSPLIT_HD bool link_cut(int32_t t, int32_t side_a, int32_t side_b, int32_t cut_from, int32_t cut_until) {
  return side_a != side_b && in_window(t, cut_from, cut_until);
}

// What is wrong with the arguments (0: nothing).
enum Bad { OK = 0, BAD_FROM = 1, BAD_UNTIL = 2, BAD_SIDE = 3 };

// The window alone.  cut_until <= cut_from (both >= 0) is an empty window: valid, and no setting.
inline Bad check_window(int32_t cut_from, int32_t cut_until) {
  if (cut_from < 0) return BAD_FROM;
  if (cut_until < 0) return BAD_UNTIL;
  return OK;
}

// The first peer with a negative side, or -1.
inline int64_t first_bad_side(int64_t V, const int32_t* side) {
  for (int64_t v = 0; side && v < V; ++v)
    if (side[v] < 0) return v;
  return -1;
}

// Connections {a, b}, a < b, whose ends are on different sides (CSR with both directions).
inline int64_t crossing(int64_t V, const int64_t* rowptr, const int32_t* colidx, const int32_t* side) {
  int64_t n = 0;
  for (int64_t v = 0; side && v < V; ++v)
    for (int64_t j = rowptr[v]; j < rowptr[v + 1]; ++j)
      if (colidx[j] > v && side[colidx[j]] != side[v]) ++n;
  return n;
}

// Does the call set anything?  No sides, an empty window or no crossing connection: the engine
// without the call.
inline bool any(int64_t V, const int64_t* rowptr, const int32_t* colidx, const int32_t* side, int32_t cut_from,
                int32_t cut_until) {
  return side && cut_from < cut_until && crossing(V, rowptr, colidx, side) > 0;
}

// The window as the schedule sees it (empty: never set).
struct Window {
  int32_t from = 0, until = 0;
  bool on() const { return from < until; }
  // Is round t a cut round (its arrivals cross no cut connection)?
  bool cut_round(int32_t t) const { return on() && in_window(t, from, until); }
  // Do the sends of round r arrive in a cut round?  (from - 1 <= r <= until - 2)
  bool cut_sends(int32_t r) const { return cut_round(r + 1); }
  // Does a round whose receive pass or whose sends the cut acts on lie at or ahead of round r?
  // (The last one is until - 1, a cut round whose sends arrive after the heal.)
  bool cut_ahead(int32_t r) const { return on() && r < until; }
};

}  // namespace netsplit
