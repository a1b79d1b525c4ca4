// The timeline sparse table on the host (numamma_amd/csrc/nmg_internal.h:
// tl_sparse_key and its decoders, tl_sparse_hash, tl_merge_rows) on the CPU,
// no HIP involved: the key round trip at every field's limits, the all-ones
// word never produced, key order = (ordinal, bin, thread, row) order, and the
// merge of the sorted sparse words into the dense rows -- sparse entries
// before, between and after the dense ones, an empty side each way, the dense
// rows apart from the output and in its own tail (the engine's fill).  Every
// merge is compared with a sort of the decoded rows.  Built by
// tests/test_timeline_all_host.py with the address and undefined-behaviour
// sanitizers.
#include <algorithm>
#include <array>
#include <cstdio>
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

typedef std::array<uint32_t, 5> Row;

static void check_keys() {
  const uint32_t ords[] = {0, 1, 511, 1021, kTlMaxSparse - 1};
  const uint32_t bins[] = {0, 1, 2048, 4095};
  const uint32_t ths[] = {0, 1, 512, 1023};
  const uint32_t rows[] = {0, 1, 0x7fffffffu, 0x80000000u, 0xffffffffu};
  uint64_t prev = 0;
  bool first = true;
  for (uint32_t o : ords)
    for (uint32_t b : bins)
      for (uint32_t t : ths)
        for (uint32_t r : rows) {
          const uint64_t k = tl_sparse_key(o, b, t, r);
          CHECK(tl_sparse_key_ord(k) == o && tl_sparse_key_bin(k) == b && tl_sparse_key_thread(k) == t &&
                tl_sparse_key_row(k) == r);
          CHECK(k != ~0ull);
          if (!first) CHECK(prev < k);  // the loops run in (ordinal, bin, thread, row) order
          prev = k;
          first = false;
        }
  static_assert(kTlMaxSparse == 1023, "ordinals 0..1022");
  // the largest key there is, and the only way to the empty marker: the ordinal no entry gets
  CHECK(tl_sparse_key(kTlMaxSparse - 1, 4095, 1023, 0xffffffffu) == 0xffbfffffffffffffull);
  CHECK(tl_sparse_key(kTlMaxSparse, 4095, 1023, 0xffffffffu) == ~0ull);
  // the fields do not overlap: each alone, at its limit
  CHECK(tl_sparse_key(0, 0, 0, 0xffffffffu) == 0xffffffffull);
  CHECK(tl_sparse_key(0, 0, 1023, 0) == 0x3ffull << 32);
  CHECK(tl_sparse_key(0, 4095, 0, 0) == 0xfffull << 42);
  CHECK(tl_sparse_key(1022, 0, 0, 0) == 1022ull << 54);
  // the hash sees the high fields: keys that differ in ordinal or bin alone start at different slots of a
  // 2^10-slot table more often than not (sparse_slot's hash would give them one)
  uint32_t differ = 0;
  for (uint32_t o = 0; o < 64; o++)
    differ += (tl_sparse_hash(tl_sparse_key(o, 3, 2, 77)) & 1023) != (tl_sparse_hash(tl_sparse_key(o + 1, 3, 2, 77)) & 1023);
  for (uint32_t b = 0; b < 64; b++)
    differ += (tl_sparse_hash(tl_sparse_key(5, b, 2, 77)) & 1023) != (tl_sparse_hash(tl_sparse_key(5, b + 1, 2, 77)) & 1023);
  CHECK(differ > 120);
  CHECK(tl_sparse_hash(0) == 0 && tl_sparse_hash(1) == 0xb456bcfc34c2cb2cull);  // murmur3's fmix64
}

// dense: rows of dense entries; sparse: rows of the entries sp_ids, any order
static void check_merge(std::vector<Row> dense, const std::vector<Row>& sparse, const std::vector<uint32_t>& sp_ids) {
  std::sort(dense.begin(), dense.end());
  std::vector<uint64_t> kv;
  for (const Row& r : sparse) {
    const size_t ord = std::find(sp_ids.begin(), sp_ids.end(), r[0]) - sp_ids.begin();
    CHECK(ord < sp_ids.size());
    kv.push_back(tl_sparse_key((uint32_t)ord, r[1], r[2], r[3]));
    kv.push_back(r[4]);
  }
  sparse_words_sort(kv);
  std::vector<Row> want = dense;
  want.insert(want.end(), sparse.begin(), sparse.end());
  std::sort(want.begin(), want.end());
  const size_t nd = dense.size(), ns = sparse.size();
  std::vector<uint32_t> flat;
  for (const Row& r : dense) flat.insert(flat.end(), r.begin(), r.end());
  // apart: exactly sized blocks, so that the sanitizer sees a step past either
  std::vector<uint32_t> out((nd + ns) * 5);
  tl_merge_rows(flat.data(), nd, kv.data(), ns, sp_ids, out.data());
  // in the output's own tail, as timeline_fill has them
  std::vector<uint32_t> tail((nd + ns) * 5, 0xdeadbeefu);
  std::copy(flat.begin(), flat.end(), tail.begin() + ns * 5);
  tl_merge_rows(tail.data() + ns * 5, nd, kv.data(), ns, sp_ids, tail.data());
  CHECK(out == tail);
  CHECK(out.size() == want.size() * 5);
  for (size_t i = 0; i < want.size() && i * 5 < out.size(); i++)
    for (int k = 0; k < 5; k++) CHECK(out[5 * i + k] == want[i][k]);
}

int main() {
  check_keys();
  const std::vector<Row> d = {{3, 0, 0, 0, 7}, {3, 0, 1, 2, 1}, {3, 11, 0, 0, 2}, {8, 4, 7, 9, 5}, {9, 0, 0, 1, 1}};
  // sparse entries before (1), between (5, 6), and after (12, 40) the dense ones; 20 selected but without a cell
  const std::vector<uint32_t> ids = {1, 5, 6, 12, 20, 40};
  const std::vector<Row> s = {{40, 0, 0, 0xffffffffu, 20}, {1, 4095, 1023, 0, 3}, {1, 0, 0, 5, 1},  {5, 2, 1, 1, 9},
                              {6, 2, 1, 1, 4},             {5, 2, 0, 7, 1},       {12, 0, 3, 0, 0xffffffffu}, {5, 1, 9, 9, 2}};
  check_merge(d, s, ids);
  check_merge(d, {}, ids);   // an empty side each way
  check_merge({}, s, ids);
  check_merge({}, {}, {});
  check_merge(d, {}, {});
  check_merge(d, {{1, 0, 0, 0, 1}}, {1});           // before only
  check_merge(d, {{5, 0, 0, 0, 1}, {5, 0, 0, 1, 1}}, {5});  // between only
  check_merge(d, {{10, 0, 0, 0, 1}}, {10});         // after only
  check_merge({{0, 0, 0, 0, 1}}, {{1022, 4095, 1023, 0xffffffffu, 1}}, std::vector<uint32_t>{1022});
  {  // 1023 sparse entries, one row each, around one dense entry: every ordinal decodes to its entry
    std::vector<uint32_t> many;
    std::vector<Row> rows;
    for (uint32_t k = 0; k < kTlMaxSparse; k++) {
      many.push_back(2 * k + (k >= 500));  // (entry 1000 is the dense one)
      rows.push_back({many.back(), k & 4095, k & 1023, k * 4099u, k + 1});
    }
    check_merge({{1000, 0, 0, 0, 1}, {1000, 1, 0, 0, 1}}, rows, many);
  }
  if (g_failed) {
    fprintf(stderr, "nmg_tl_sparse_host: %d checks failed\n", g_failed);
    return 1;
  }
  printf("nmg_tl_sparse_host: ok\n");
  return 0;
}
