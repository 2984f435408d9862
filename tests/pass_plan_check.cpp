// Host check of csrc/pass_plan.h (built and run by tests/test_pass_plan.py): for every wide
// sender degree 17..512 and every active-word count 1..64 (the low words) plus random masks,
//   - every pass fits the 2048-cell table;
//   - the connection groups partition [0, deg), each <= 64 connections, one group when deg <= 64;
//   - the word ranges of a group cover every active word exactly once and no other word;
//   - the flush's store instructions do not exceed the chunked push's (16 connections at a time,
//     segments of 16 / 32 / 64 words by the whole row's active count) by more than the rounding
//     of the extra passes of a group (less than one store each), and not at all when deg is a
//     multiple of 4 (nothing to round).
// Prints "ok <cases>" and exits 0, or the first failing case and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "pass_plan.h"

static int popc(uint64_t x) { return __builtin_popcountll(x); }

// store instructions of the chunked push of one sender (scatter_row: compact flush when the row
// has <= 32 active words, else one store per connection)
static int chunked_stores(int deg, int nf) {
  const int seg = nf <= 16 ? 16 : nf <= 32 ? 32 : 64;
  const int per = 64 / seg;
  int n = 0;
  for (int nb = 0; nb < deg; nb += 16) {
    const int nn = deg - nb < 16 ? deg - nb : 16;
    n += (nn + per - 1) / per;
  }
  return n;
}

#define FAIL(...)                                                   \
  do {                                                              \
    std::printf("FAIL deg %d fam %016llx: ", deg, (unsigned long long)fam); \
    std::printf(__VA_ARGS__);                                       \
    std::printf("\n");                                              \
    return false;                                                   \
  } while (0)

static bool check(int deg, uint64_t fam) {
  const int nf = popc(fam);
  const int ng = plan_groups(deg);
  if (deg <= 64 && ng != 1) FAIL("%d groups", ng);
  int next = 0, stores = 0, passes = 0;
  for (int g = 0; g < ng; ++g) {
    const int c0 = plan_group_begin(g), C = plan_group_conns(deg, g);
    if (c0 != next) FAIL("group %d begins at %d, expected %d", g, c0, next);
    if (C < 1 || C > 64) FAIL("group %d has %d connections", g, C);
    next = c0 + C;
    uint64_t seen = 0;
    int nextr = 0;
    const int np = plan_passes(C, nf);
    for (int p = 0; p < np; ++p) {
      const int r0 = plan_pass_rank0(C, p), nr = plan_pass_ranks(C, nf, p);
      if (r0 != nextr || nr < 1) FAIL("group %d pass %d ranks [%d, +%d), expected from %d", g, p, r0, nr, nextr);
      nextr = r0 + nr;
      if (nr > plan_pass_words(C)) FAIL("group %d pass %d: %d words", g, p, nr);
      const int seg = plan_seg(nr);
      if (seg < nr || 64 % seg) FAIL("segment %d for %d words", seg, nr);
      if (plan_pass_cells(C, nr) > PLAN_CELLS) FAIL("group %d pass %d: %d cells", g, p, plan_pass_cells(C, nr));
      const uint64_t wm = plan_rank_words(fam, r0, nr);
      if (popc(wm) != nr) FAIL("group %d pass %d: %d words for %d ranks", g, p, popc(wm), nr);
      if (wm & seen) FAIL("group %d pass %d: a word twice", g, p);
      if (wm & ~fam) FAIL("group %d pass %d: an inactive word", g, p);
      seen |= wm;
      stores += plan_flush_count(C, nr);
      ++passes;
    }
    if (nextr != nf || seen != fam) FAIL("group %d covers %016llx", g, (unsigned long long)seen);
  }
  if (next != deg) FAIL("groups end at %d", next);
  // A pass of C connections and seg-word segments needs ceil(C * seg / 64) stores, the chunked
  // push ceil(16 * seg' / 64) per chunk with seg' >= seg: the plan can exceed it only by the
  // rounding of its passes, less than one store each.
  const int was = chunked_stores(deg, nf);
  if (stores > was + passes - ng) FAIL("%d stores in %d passes, chunked %d", stores, passes, was);
  if (deg % 4 == 0 && stores > was) FAIL("%d stores, chunked %d", stores, was);
  return true;
}

int main() {
  long cases = 0;
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() {  // xorshift64*
    s ^= s >> 12;
    s ^= s << 25;
    s ^= s >> 27;
    return s * 0x2545F4914F6CDD1Dull;
  };
  for (int deg = 17; deg <= 512; ++deg) {
    for (int nf = 1; nf <= 64; ++nf, ++cases)
      if (!check(deg, nf == 64 ? ~0ull : (1ull << nf) - 1ull)) return 1;
    for (int i = 0; i < 300; ++i, ++cases) {
      uint64_t m = rnd();
      if (i % 3 == 1) m &= rnd() & rnd();  // sparse rows (light rounds)
      if (i % 3 == 2) m |= rnd() | rnd();  // nearly full rows (peak rounds)
      if (!m) m = 1ull << (i & 63);
      if (!check(deg, m)) return 1;
    }
  }
  std::printf("ok %ld\n", cases);
  return 0;
}
