// nmg_walk_order.h -- the report's walk order over plain arrays.  Plain C++,
// no HIP and no engine: the engine and tests/c/nmg_walk_order_host.cpp include it.
//
// The engine keeps everything by entry id.  A report of a live online table
// walks the entries in the order of the latest table that listed them all
// (order[position] = id) and its metadata follows that order, so what the
// registry reads per entry is permuted and rows name entries by position.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace nmg {

// walk_counters' arrays (empty while the walk order is the id order)
struct WalkCounters {
  std::vector<uint64_t> size, first, cw;  // by position: buffer size, first ordinal, [4] counts / weights
  std::vector<uint32_t> pos;              // by id: the walk position
};

// The per-entry arrays the registry reads, by walk position, and w.pos: the
// pointers then point into w.  An empty order (E == 0) is the id order: w stays
// empty and the pointers are what they were.  order: a permutation of 0 .. E - 1.
inline void walk_permute(const uint32_t* order, uint32_t E, const uint64_t** size, const uint64_t** first,
                         const uint64_t** cw, WalkCounters& w) {
  if (!E) return;
  w.pos.resize(E);
  w.size.resize(E);
  w.first.resize(E);
  w.cw.resize((size_t)E * 4);
  for (uint32_t k = 0; k < E; k++) {
    const uint32_t id = order[k];
    w.pos[id] = k;
    w.size[k] = (*size)[id];
    w.first[k] = (*first)[id];
    for (int q = 0; q < 4; q++) w.cw[(size_t)k * 4 + q] = (*cw)[(size_t)id * 4 + q];
  }
  *size = w.size.data();
  *first = w.first.data();
  *cw = w.cw.data();
}

// rows[n][width]: column 0 from entry id to walk position (pos empty: the id
// order).  The rows keep their places: for writers that take them in any order.
template <class W>
inline void walk_rewrite_entries(W* rows, int64_t n, uint32_t width, const std::vector<uint32_t>& pos) {
  if (pos.empty()) return;
  for (int64_t i = 0; i < n; i++) rows[(size_t)i * width] = (W)pos[rows[(size_t)i * width]];
}

// Page rows (entry, thread, page, count) grouped by walk position, each entry's
// rows in the order they had, column 0 rewritten: what nmg_report's writer walks.
inline std::vector<uint32_t> walk_regroup_rows(const uint32_t* rows, int64_t n, const std::vector<uint32_t>& pos) {
  std::vector<uint32_t> idx((size_t)n);
  for (uint32_t i = 0; i < (uint32_t)n; i++) idx[i] = i;
  std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return pos[rows[4 * (size_t)a]] < pos[rows[4 * (size_t)b]]; });
  std::vector<uint32_t> out((size_t)n * 4);
  for (size_t i = 0; i < idx.size(); i++) {
    std::copy_n(rows + 4 * (size_t)idx[i], 4, &out[4 * i]);
    out[4 * i] = pos[out[4 * i]];
  }
  return out;
}

}  // namespace nmg
