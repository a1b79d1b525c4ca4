// The chunk pool's layout rule (pool_layout, numamma_amd/csrc/nmg_pool_layout.h)
// on the CPU, no HIP involved: where route_pool puts the workgroups' private
// chunk ranges in a pool of 2^K-chunk pieces.  Built by
// tests/test_pool_layout_host.py with the address and undefined-behaviour
// sanitizers.
#include <cstdio>
#include <random>
#include <vector>

#include "nmg_pool_layout.h"

using namespace nmg;

static int g_failed = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      g_failed++;                                                       \
    }                                                                   \
  } while (0)

static const uint64_t kLimit = 1ull << 25;  // kChunkIdBits

// every property of one accepted layout; the number of ids skipped
static uint64_t check_layout(const std::vector<uint64_t>& cap, uint32_t K, const std::vector<uint32_t>& c0,
                             uint32_t pieces) {
  const uint32_t n = (uint32_t)cap.size();
  uint64_t asked = 0;
  CHECK(c0[0] == 0);
  for (uint32_t w = 0; w < n; w++) {
    CHECK(c0[w] <= c0[w + 1]);                      // ascending, so disjoint
    CHECK((uint64_t)c0[w + 1] - c0[w] >= cap[w]);   // at least its capacity
    if (c0[w + 1] > c0[w])                          // one piece: its first and last id
      CHECK((c0[w] >> K) == ((c0[w + 1] - 1) >> K));
    if (cap[w])  // the ids it asked for, whatever the next range's start adds
      CHECK((c0[w] >> K) == ((c0[w] + cap[w] - 1) >> K));
    asked += cap[w];
  }
  const uint64_t tot = c0[n];
  CHECK(tot < kLimit);
  CHECK(pieces == (tot + (1ull << K) - 1) >> K);
  CHECK(tot >= asked && tot - asked < asked + 1);  // fewer ids skipped than asked for (route_eligible's bound)
  return tot - asked;
}

static bool layout(const std::vector<uint64_t>& cap, uint32_t K, uint64_t* skipped = nullptr) {
  std::vector<uint32_t> c0(cap.size() + 1, 0xdeadbeefu);
  uint32_t pieces = ~0u;
  if (!pool_layout(cap.data(), (uint32_t)cap.size(), K, kLimit, c0.data(), &pieces)) return false;
  const uint64_t s = check_layout(cap, K, c0, pieces);
  if (skipped) *skipped = s;
  return true;
}

int main() {
  CHECK(pool_min_log2(0) == 0 && pool_min_log2(1) == 0 && pool_min_log2(2) == 1 && pool_min_log2(3) == 2);
  CHECK(pool_min_log2(64) == 6 && pool_min_log2(65) == 7 && pool_min_log2(1ull << 20) == 20);

  // by hand, pieces of 8: [0,3) [3,8) (4 asked for, and the id skipped before the next) [8,16) [16,23) [23,24) [24,24)
  {
    const std::vector<uint64_t> cap = {3, 4, 8, 7, 1, 0};
    std::vector<uint32_t> c0(cap.size() + 1);
    uint32_t pieces = 0;
    CHECK(pool_layout(cap.data(), (uint32_t)cap.size(), 3, kLimit, c0.data(), &pieces));
    const std::vector<uint32_t> want = {0, 3, 8, 16, 23, 24, 24};
    CHECK(c0 == want);
    CHECK(pieces == 3);
    check_layout(cap, 3, c0, pieces);
  }
  // nothing asked for: no ids, no pieces
  {
    uint32_t c0[1] = {7}, pieces = 7;
    CHECK(pool_layout(nullptr, 0, 16, kLimit, c0, &pieces) && c0[0] == 0 && pieces == 0);
  }
  // a capacity larger than a piece, and K out of range: refused
  CHECK(!layout({9}, 3));
  CHECK(layout({8}, 3));
  CHECK(!layout({1}, 32));
  // the id limit: 2^25 - 1 ids pass, 2^25 do not, with and without skipped ids
  CHECK(layout({kLimit - 1}, 25));
  CHECK(!layout({kLimit}, 25));
  CHECK(layout(std::vector<uint64_t>(511, 1u << 16), 16));
  CHECK(!layout(std::vector<uint64_t>(512, 1u << 16), 16));
  CHECK(layout(std::vector<uint64_t>(512, 40000), 16));   // one range per piece: the last starts at 511 * 2^16
  CHECK(!layout(std::vector<uint64_t>(513, 40000), 16));  // (20.5M ids asked for: the skipped ones reach the limit)

  // random capacities: several K, capacities up to a piece, among them whole
  // pieces and one chunk below
  std::mt19937_64 rng(12345);
  uint64_t skipped_any = 0, accepted = 0, refused = 0;
  for (uint32_t K : {1u, 3u, 6u, 10u, 16u, 20u}) {
    const uint64_t piece = 1ull << K;
    for (int round = 0; round < 200; round++) {
      const uint32_t n = 1 + (uint32_t)(rng() % 300);
      const uint64_t top = 1 + rng() % piece;  // this round's largest capacity
      std::vector<uint64_t> cap(n);
      for (uint64_t& c : cap) {
        const uint64_t pick = rng() % 16;
        c = pick == 0 ? piece : pick == 1 ? piece - 1 : pick == 2 ? 0 : 1 + rng() % top;
      }
      uint64_t skipped = 0;
      if (layout(cap, K, &skipped)) {
        accepted++;
        skipped_any += skipped;
      } else {  // only the id limit can refuse these: twice the capacities reach it
        uint64_t asked = 0;
        for (uint64_t c : cap) asked += c;
        CHECK(2 * asked >= kLimit);
        refused++;
      }
    }
  }
  CHECK(accepted > 600 && refused > 0 && skipped_any > 0);

  if (g_failed) return 1;
  printf("nmg_pool_layout_host: ok\n");
  return 0;
}
