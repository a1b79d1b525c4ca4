// The report's walk order (numamma_amd/csrc/nmg_walk_order.h) on the CPU, no
// HIP involved: the per-entry arrays permuted to walk positions, a row array's
// entry column rewritten, and nmg_report's stable regrouping of the page rows.
// Every result is compared with a direct restatement below.  Built by
// tests/test_walk_order_host.py with the address and undefined-behaviour
// sanitizers.
#include <cstdio>
#include <numeric>
#include <random>
#include <vector>

#include "nmg_walk_order.h"

using namespace nmg;

static int g_failed = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      g_failed++;                                                       \
    }                                                                   \
  } while (0)

// per-id inputs that tell every id and word apart
struct Inputs {
  std::vector<uint64_t> size, first, cw;
  explicit Inputs(uint32_t E) : size(E), first(E), cw((size_t)E * 4) {
    for (uint32_t id = 0; id < E; id++) {
      size[id] = 1000 + id;
      first[id] = 2000 + id;
      for (int q = 0; q < 4; q++) cw[(size_t)id * 4 + q] = 3000 + 10 * id + q;
    }
  }
};

// walk_permute over `order`, checked word for word: position k holds what id order[k] had
static WalkCounters check_permute(const std::vector<uint32_t>& order) {
  const uint32_t E = (uint32_t)order.size();
  const Inputs in(E);
  const uint64_t *size = in.size.data(), *first = in.first.data(), *cw = in.cw.data();
  WalkCounters w;
  walk_permute(order.data(), E, &size, &first, &cw, w);
  CHECK(w.pos.size() == E && w.size.size() == E && w.first.size() == E && w.cw.size() == (size_t)E * 4);
  CHECK(size == w.size.data() && first == w.first.data() && cw == w.cw.data());
  for (uint32_t k = 0; k < E; k++) {
    const uint32_t id = order[k];
    CHECK(w.pos[id] == k);
    CHECK(size[k] == 1000 + id && first[k] == 2000 + id);
    for (int q = 0; q < 4; q++) CHECK(cw[(size_t)k * 4 + q] == 3000 + 10 * id + (uint64_t)q);
  }
  return w;
}

// rows of `width` words whose entries (column 0) repeat and are not sorted; the other columns number the row
template <class W>
static std::vector<W> make_rows(const std::vector<uint32_t>& entries, uint32_t width) {
  std::vector<W> rows(entries.size() * width);
  for (size_t i = 0; i < entries.size(); i++) {
    rows[i * width] = (W)entries[i];
    for (uint32_t c = 1; c < width; c++) rows[i * width + c] = (W)(100 * i + c);
  }
  return rows;
}

template <class W>
static void check_rewrite(const std::vector<uint32_t>& entries, uint32_t width, const std::vector<uint32_t>& pos) {
  std::vector<W> rows = make_rows<W>(entries, width);
  const std::vector<W> before = rows;
  walk_rewrite_entries(rows.data(), (int64_t)entries.size(), width, pos);
  for (size_t i = 0; i < entries.size(); i++) {
    CHECK(rows[i * width] == (W)(pos.empty() ? entries[i] : pos[entries[i]]));
    for (uint32_t c = 1; c < width; c++) CHECK(rows[i * width + c] == before[i * width + c]);
  }
}

// the regrouping restated: for each position in turn, the rows of its id in their first order
static void check_regroup(const std::vector<uint32_t>& entries, const std::vector<uint32_t>& order,
                          const std::vector<uint32_t>& pos) {
  const std::vector<uint32_t> rows = make_rows<uint32_t>(entries, 4);
  const std::vector<uint32_t> got = walk_regroup_rows(rows.data(), (int64_t)entries.size(), pos);
  std::vector<uint32_t> want;
  for (uint32_t k = 0; k < (uint32_t)order.size(); k++)
    for (size_t i = 0; i < entries.size(); i++)
      if (entries[i] == order[k]) {
        want.push_back(k);
        for (uint32_t c = 1; c < 4; c++) want.push_back(rows[i * 4 + c]);
      }
  CHECK(got == want);
}

int main() {
  // an empty order: the id order -- nothing allocated, the pointers untouched, rows as they were
  {
    const uint64_t a[1] = {1}, b[1] = {2}, c[4] = {3, 4, 5, 6};
    const uint64_t *size = a, *first = b, *cw = c;
    WalkCounters w;
    walk_permute(nullptr, 0, &size, &first, &cw, w);
    CHECK(size == a && first == b && cw == c);
    CHECK(w.pos.empty() && w.size.empty() && w.first.empty() && w.cw.empty());
    check_rewrite<uint32_t>({2, 0, 2, 1}, 5, w.pos);
    check_rewrite<uint64_t>({2, 0, 2, 1}, 4, w.pos);
    uint32_t* none = nullptr;
    walk_rewrite_entries(none, 0, 5, w.pos);
  }
  // one entry
  {
    const WalkCounters w = check_permute({0});
    check_rewrite<uint32_t>({0, 0, 0}, 5, w.pos);
    check_rewrite<uint64_t>({0}, 4, w.pos);
    check_regroup({0, 0}, {0}, w.pos);
  }
  // five entries reversed, and at random; rows with repeated entries, widths 4 and 5, and no row
  const std::vector<uint32_t> entries = {3, 3, 0, 4, 1, 1, 1, 4, 2, 0, 3};
  std::vector<uint32_t> random(5);
  std::iota(random.begin(), random.end(), 0u);
  std::mt19937 rng(2024);
  do std::shuffle(random.begin(), random.end(), rng);
  while (std::is_sorted(random.begin(), random.end()) || std::is_sorted(random.rbegin(), random.rend()));
  for (const std::vector<uint32_t>& order : {std::vector<uint32_t>{4, 3, 2, 1, 0}, random}) {
    const WalkCounters w = check_permute(order);
    check_rewrite<uint32_t>(entries, 5, w.pos);  // timeline rows
    check_rewrite<uint64_t>(entries, 4, w.pos);  // cost rows
    check_rewrite<uint32_t>(entries, 4, w.pos);
    check_rewrite<uint64_t>(entries, 5, w.pos);
    check_rewrite<uint32_t>({}, 5, w.pos);
    check_rewrite<uint64_t>({}, 4, w.pos);
    uint64_t* none = nullptr;
    walk_rewrite_entries(none, 0, 4, w.pos);
    check_regroup(entries, order, w.pos);
    check_regroup({}, order, w.pos);
    CHECK(walk_regroup_rows(nullptr, 0, w.pos).empty());
  }

  if (g_failed) return 1;
  printf("nmg_walk_order_host: ok\n");
  return 0;
}
