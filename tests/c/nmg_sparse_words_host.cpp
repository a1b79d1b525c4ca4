// The sparse page table's words on the host (numamma_amd/csrc/nmg_internal.h:
// sparse_words_sort, place_sparse_rows) on the CPU, no HIP involved: the
// interleaved (key, value) words sorted by key, equal keys merged with a u32
// sum, and the words placed as (entry, thread, page, value) rows.  Every result
// is compared with a direct restatement below.  Built by
// tests/test_sparse_words_host.py with the address and undefined-behaviour
// sanitizers.
#include <cstdio>
#include <cstring>
#include <map>
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

typedef std::vector<uint64_t> Words;

// the merge restated: a map from key to the u32 sum of its values, read in key order
static Words merged(const Words& kv) {
  std::map<uint64_t, uint32_t> m;
  for (size_t i = 0; i < kv.size(); i += 2) m[kv[i]] += (uint32_t)kv[i + 1];
  Words out;
  for (const auto& e : m) {
    out.push_back(e.first);
    out.push_back(e.second);
  }
  return out;
}

static void check_sort(const Words& kv) {
  Words s = kv;
  sparse_words_sort(s);
  CHECK(s.size() == kv.size());
  for (size_t i = 2; i < s.size(); i += 2) CHECK(s[i - 2] <= s[i]);
  // the same (key, value) pairs: each input pair crossed off once
  Words left = s;
  for (size_t i = 0; i < kv.size(); i += 2) {
    bool found = false;
    for (size_t j = 0; j < left.size() && !found; j += 2)
      if (left[j] == kv[i] && left[j + 1] == kv[i + 1]) {
        left.erase(left.begin() + j, left.begin() + j + 2);
        found = true;
      }
    CHECK(found);
  }
  CHECK(left.empty());
  Words m = kv;
  sparse_words_sort(m, true);
  CHECK(m == merged(kv));
  for (size_t i = 2; i < m.size(); i += 2) CHECK(m[i - 2] < m[i]);  // ascending and unique
}

// place_sparse_rows over rows pre-filled with 0xA5, against the restatement:
// for each sparse index in turn, its kept words in (thread, page) order from
// row soff[s] on; every other word of the array untouched
template <class W>
static void check_place(const Words& kv, const std::vector<uint32_t>& sent_entry, const std::vector<uint64_t>& soff,
                        size_t nrows) {
  std::vector<W> rows(nrows * 4), want(nrows * 4);
  memset(rows.data(), 0xA5, rows.size() * sizeof(W));
  memset(want.data(), 0xA5, want.size() * sizeof(W));
  for (uint32_t s = 0; s < sent_entry.size(); s++) {
    std::map<std::pair<uint32_t, uint32_t>, W> cells;  // (thread, page) -> value
    for (size_t i = 0; i < kv.size(); i += 2) {
      const uint64_t k = kv[i];
      if (k == ~0ull || !(W)kv[i + 1] || sent_entry[s] == ~0u || (k >> 42) != s) continue;
      cells[{(uint32_t)((k >> 32) & 0x3ff), (uint32_t)k}] = (W)kv[i + 1];
    }
    size_t r = soff[s];
    for (const auto& c : cells) {
      CHECK(r < nrows);
      if (r >= nrows) break;
      want[4 * r] = sent_entry[s];
      want[4 * r + 1] = c.first.first;
      want[4 * r + 2] = c.first.second;
      want[4 * r + 3] = c.second;
      r++;
    }
  }
  place_sparse_rows(kv.data(), kv.size() / 2, sent_entry, soff.data(), rows.data());
  CHECK(rows == want);
}

template <class W>
static void place_cases() {
  const uint64_t big = sizeof(W) == 8 ? (1ull << 40) : 0;  // a cost above 2^32 where the rows are u64
  // no words, and no sparse entry
  check_place<W>({}, {}, {}, 2);
  check_place<W>({}, {7, 9}, {0, 1}, 2);
  // one word
  check_place<W>({sparse_key(0, 1, 5), 3}, {4}, {1}, 3);
  // two sparse entries (rows 1.. and 6..), their words interleaved, threads and pages out of order
  const Words two = {sparse_key(1, 1, 2), 11,       sparse_key(0, 1, 0), 12, sparse_key(1, 0, 9), 13 + big,
                     sparse_key(0, 0, 70000), 14,   sparse_key(1, 1, 1), 15, sparse_key(0, 0, 3), 16,
                     sparse_key(1, 0, 0xffffffffu), 17, sparse_key(0, 1023, 1), 18};
  check_place<W>(two, {5, 2}, {1, 6}, 11);
  // words to skip: an empty slot's key, a zero value, an index past the sparse entries, an entry no longer sparse
  const Words skip = {~0ull, 5,      sparse_key(0, 0, 1), 0, sparse_key(3, 0, 0), 6, sparse_key(1, 0, 4), 7,
                      sparse_key(2, 1, 1), 8, sparse_key(0, 0, 2), 9, sparse_key(2, 0, 8), 10 + big};
  check_place<W>(skip, {6, ~0u, 1}, {4, 0, 1}, 7);
  check_place<W>(skip, {~0u, ~0u, ~0u}, {0, 0, 0}, 2);  // nothing placed at all
}

int main() {
  // sort and merge: no words, one word
  check_sort({});
  check_sort({sparse_key(2, 1, 7), 4});
  {  // (and on the values themselves)
    Words one = {sparse_key(2, 1, 7), 4};
    sparse_words_sort(one, true);
    CHECK((one == Words{sparse_key(2, 1, 7), 4}));
  }
  // three workers' words concatenated: key a in all three, b in two, c once, d in two with a u32 sum that wraps
  const uint64_t a = sparse_key(1, 0, 5), b = sparse_key(0, 3, 9), c = sparse_key(4, 1, 0), d = sparse_key(0, 3, 8);
  const Words parts = {b, 2, a, 1, d, 0xfffffff0u, /* | */ a, 10, d, 0x20, /* | */ c, 7, b, 40, a, 100};
  check_sort(parts);
  {
    Words m = parts;
    sparse_words_sort(m, true);
    CHECK((m == Words{d, 0x10, b, 42, a, 111, c, 7}));
  }
  place_cases<uint32_t>();
  place_cases<uint64_t>();

  if (g_failed) return 1;
  printf("nmg_sparse_words_host: ok\n");
  return 0;
}
