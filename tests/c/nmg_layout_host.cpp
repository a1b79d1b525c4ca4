// The counter arrays' layout (numamma_amd/csrc/nmg_internal.h) on the CPU, no
// HIP involved.  Prints every constant and helper value as "name value" lines
// for tests/test_layout_host.py to compare with the Python mirror
// (numamma_amd/results.py), and checks here that the index helpers tile each
// array: every word of sum64 / min64 / max64 belongs to exactly one region,
// and the regions' total is the word-count helper.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nmg_internal.h"

using namespace nmg;

static int g_failed = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      g_failed++;                                                       \
    }                                                                   \
  } while (0)

// marks word i of an array of n words; false if it is outside or taken
static bool take(std::vector<int>& words, uint64_t i) { return i < words.size() && words[i]++ == 0; }
static bool all_taken(const std::vector<int>& words) {
  for (int w : words)
    if (w != 1) return false;
  return true;
}

static void check_tiling(uint64_t E, bool levels) {
  std::vector<int> sum(sum64_words(E, levels), 0);
  for (uint32_t a = 0; a < 2; a++)
    for (uint32_t i = 0; i < kGlobalSums; i++) CHECK(take(sum, gsum_index(a, i)));
  for (uint64_t e = 0; e < E; e++)
    for (uint32_t a = 0; a < 2; a++)
      for (uint32_t w = 0; w < 2; w++) CHECK(take(sum, objcw_index(e, a, w, E)));
  for (uint64_t e = 0; levels && e < E; e++)
    for (uint32_t a = 0; a < 2; a++)
      for (uint32_t k = 0; k < kLevelWords; k++) CHECK(take(sum, levels_index(e, a, E) + k));
  CHECK(all_taken(sum));
  // the regions in order: globals, rows, levels
  CHECK(gsum_index(1, kGlobalSums - 1) + 1 == kCwBase);
  CHECK(objcw_index(0, 0, 0, E) == kCwBase);
  CHECK(kCwBase + kCwRows * E == levels_base(E));
  CHECK(levels_index(0, 0, E) == levels_base(E));
  CHECK(sum64_words(E, false) == levels_base(E));

  std::vector<int> mn(min64_words(E), 0), mx(max64_words(), 0);
  for (uint32_t a = 0; a < 2; a++)
    for (uint32_t b = 0; b < kBuckets; b++) {
      CHECK(take(mn, gminmax_index(a, b)));
      CHECK(take(mx, gminmax_index(a, b)));
    }
  for (uint64_t e = 0; e < E; e++) CHECK(take(mn, first_index(e)));
  CHECK(take(mn, error_index(E)));
  CHECK(all_taken(mn));
  CHECK(all_taken(mx));
  CHECK(first_index(0) == kFirstBase && kFirstBase == kGlobalMinMax);
  CHECK(error_index(E) + 1 == min64_words(E));
}

int main() {
  printf("NB_BUCKETS %u\n", kBuckets);
  printf("GLOBAL_SUMS %u\n", kGlobalSums);
  printf("LEVEL_WORDS %u\n", kLevelWords);
  printf("GLOBAL_SUM_WORDS %u\n", kCwBase);
  printf("CW_ROWS %u\n", kCwRows);
  printf("GLOBAL_MIN_WORDS %u\n", kGlobalMinMax);
  printf("COUNTER_WORDS %zu\n", sizeof(nmg_mem_counters) / 8);
  printf("max64_words %llu\n", (unsigned long long)max64_words());
  const uint64_t sizes[] = {0, 1, 5};
  for (uint64_t E : sizes) {
    printf("min64_words:%llu %llu\n", (unsigned long long)E, (unsigned long long)min64_words(E));
    for (int levels = 0; levels < 2; levels++) {
      printf("sum64_words:%llu:%d %llu\n", (unsigned long long)E, levels, (unsigned long long)sum64_words(E, levels));
      check_tiling(E, levels);
    }
  }
  if (g_failed) return 1;
  printf("nmg_layout_host: ok\n");
  return 0;
}
