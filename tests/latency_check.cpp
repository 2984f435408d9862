// Host check of csrc/latency.h (tests/test_latency_host.py): the bit-sliced start planes and the
// per-word functions the latency kernel runs -- sum of the starts and smallest start under a
// frontier word -- against a per-bit brute force over random schedules and words.  Prints
// "ok <cases>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "latency.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}

static long cases = 0;
#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);      \
      std::exit(1);                                                   \
    }                                                                 \
    ++cases;                                                          \
  } while (0)

// one schedule: the planes, then every word under a set of masks against the per-bit loop
static void check_schedule(const std::vector<int32_t>& start) {
  const int32_t M = (int32_t)start.size();
  const int32_t W = (M + 63) / 64;
  const int32_t mx = latency::max_start(M, start.data());
  const int B = latency::plane_bits(mx);
  CHECK(B >= 0 && B <= 31);
  CHECK(mx <= 0 ? B == 0 : ((mx >> (B - 1)) == 1));
  // (one word more than B * W: the builder must not write past its planes)
  std::vector<uint64_t> S((size_t)B * W + 1, 0xA5A5A5A5A5A5A5A5ull);
  latency::build_start_planes(M, W, start.data(), B, S.data());
  CHECK(S[(size_t)B * W] == 0xA5A5A5A5A5A5A5A5ull);
  for (int b = 0; b < B; ++b)
    for (int32_t w = 0; w < W; ++w)
      for (int i = 0; i < 64; ++i) {
        const int32_t m = w * 64 + i;
        const bool want = m < M && start[m] > 0 && ((start[m] >> b) & 1);  // (tail bits, -1 and 0: clear)
        if ((((S[(size_t)b * W + w]) >> i) & 1ull) != (want ? 1ull : 0ull)) CHECK(false);
      }
  ++cases;
  for (int32_t w = 0; w < W; ++w) {
    const int nbits = M - w * 64 < 64 ? M - w * 64 : 64;
    const uint64_t valid = nbits == 64 ? ~0ull : (1ull << nbits) - 1ull;
    uint64_t masks[8] = {0ull, valid, 1ull, 1ull << (nbits - 1), 1ull << (rnd() % nbits), rnd() & valid,
                         rnd() & rnd() & valid, (rnd() | rnd()) & valid};
    for (uint64_t f : masks) {
      uint64_t sum = 0;
      uint32_t mn = 0xFFFFFFFFu;
      int cnt = 0;
      for (int i = 0; i < 64; ++i)
        if ((f >> i) & 1ull) {
          const int32_t s = start[w * 64 + i] > 0 ? start[w * 64 + i] : 0;  // (-1 counts as 0)
          sum += (uint64_t)s;
          if ((uint32_t)s < mn) mn = (uint32_t)s;
          ++cnt;
        }
      CHECK(latency::popcount64(f) == cnt);
      CHECK(latency::start_sum(f, S.data() + w, W, B) == sum);
      if (f) CHECK(latency::start_min(f, S.data() + w, W, B) == mn);
      // the word's relative hops in a round at or after every start under f
      const int32_t round = mx > 0 ? mx + (int32_t)(rnd() % 5) : (int32_t)(rnd() % 9);
      if (f && round >= 0) {
        uint64_t hops = 0;
        int32_t top = -1;
        for (int i = 0; i < 64; ++i)
          if ((f >> i) & 1ull) {
            const int32_t s = start[w * 64 + i] > 0 ? start[w * 64 + i] : 0;
            hops += (uint64_t)(round - s);
            if (round - s > top) top = round - s;
          }
        CHECK((uint64_t)round * (uint64_t)cnt - latency::start_sum(f, S.data() + w, W, B) == hops);
        CHECK((int32_t)((uint32_t)round - latency::start_min(f, S.data() + w, W, B)) == top);
      }
    }
  }
}

int main() {
  // plane_bits and bin_of at their edges
  CHECK(latency::plane_bits(-1) == 0 && latency::plane_bits(0) == 0 && latency::plane_bits(1) == 1);
  CHECK(latency::plane_bits(2) == 2 && latency::plane_bits(3) == 2 && latency::plane_bits(4) == 3);
  CHECK(latency::plane_bits(100) == 7 && latency::plane_bits(127) == 7 && latency::plane_bits(128) == 8);
  CHECK(latency::plane_bits(1 << 30) == 31 && latency::plane_bits(0x7FFFFFFF) == 31);
  CHECK(latency::bin_of(0, 2) == 0 && latency::bin_of(1, 2) == 1 && latency::bin_of(2, 2) == 1);
  CHECK(latency::bin_of(62, 64) == 62 && latency::bin_of(63, 64) == 63 && latency::bin_of(64, 64) == 63);
  CHECK(latency::bin_of(0x7FFFFFFF, 1024) == 1023 && latency::bin_of(7, 8) == 7 && latency::bin_of(43, 8) == 7);

  const int32_t sizes[] = {1, 2, 63, 64, 65, 70, 128, 200, 1000, 4100};
  for (int32_t M : sizes) {
    check_schedule(std::vector<int32_t>((size_t)M, 0));   // every start 0: B = 0
    check_schedule(std::vector<int32_t>((size_t)M, -1));  // nothing scheduled
    std::vector<int32_t> st((size_t)M);
    for (int32_t m = 0; m < M; ++m) st[m] = m % 5;
    for (int32_t m = 0; m < M; m += 64) st[m] = 70;  // one message per word far behind
    check_schedule(st);
    for (int32_t m = 0; m < M; ++m) st[m] = (m % 3 == 0) ? -1 : (int32_t)(rnd() % 101);
    check_schedule(st);
    for (int32_t m = 0; m < M; ++m) st[m] = (int32_t)(rnd() % 3) - 1;
    st[(size_t)(rnd() % (uint64_t)M)] = 1 << 30;  // the largest start p2pg_set_ttl's range knows
    check_schedule(st);
    st.assign((size_t)M, 1 << 30);
    check_schedule(st);
  }
  for (int it = 0; it < 300; ++it) {
    const int32_t M = 1 + (int32_t)(rnd() % 300);
    const int32_t top = 1 + (int32_t)(rnd() % (it % 3 == 0 ? 0x7FFFFFFFull : 200ull));
    std::vector<int32_t> st((size_t)M);
    for (int32_t m = 0; m < M; ++m) st[m] = rnd() % 7 == 0 ? -1 : (int32_t)(rnd() % (uint64_t)top);
    check_schedule(st);
  }
  std::printf("ok %ld\n", cases);
  return 0;
}
