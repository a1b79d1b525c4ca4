// nmg_placement_huge_host.cpp -- the host statement of the placement rule
// (placement_blocks_host, nmg_report.cpp) over groups with a sparse member,
// stand-alone: built with nmg_report.cpp by tests/test_placement_huge_host.py
// (under the address and undefined-behaviour sanitizers where the compiler has
// them) and run as a child process.
//
//  1. a [stack]-sized group: 10^8 pages, a handful of cells.  A [page][node]
//     array over it would be 10^8 * nodes sums; the walk over the cells ends
//     at once.
//  2. a call-site group of one dense and one sparse member, pages past the
//     site's rows dropped for both, a page that qualifies only through both.
//  3. without the flag the same tables give the dense entries' rows alone.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nmg_internal.h"

using namespace nmg;

#define CHECK(c)                                            \
  do {                                                      \
    if (!(c)) {                                             \
      printf("%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
      exit(1);                                              \
    }                                                       \
  } while (0)

typedef std::vector<uint64_t> Rows;

static bool row_is(const Rows& r, size_t i, uint64_t g, uint64_t node, uint64_t s, uint64_t e, uint64_t c) {
  return r.size() >= 5 * (i + 1) && r[5 * i] == g && r[5 * i + 1] == node && r[5 * i + 2] == s && r[5 * i + 3] == e &&
         r[5 * i + 4] == c;
}

int main() {
  const uint32_t T = 4;
  nmg_placement_options po = {2, 8, nullptr, NMG_PLACE_PAGE_COUNTS | NMG_PLACE_HUGE};
  PlaceMap map;
  CHECK(placement_map(&po, T, map) == NMG_OK);  // threads 0, 1 -> node 0; 2, 3 -> node 1
  po.source = NMG_PLACE_PAGE_COST | NMG_PLACE_HUGE;
  CHECK(placement_map(&po, T, map) == NMG_ERR_INVALID);
  po.source = NMG_PLACE_HUGE | 1;
  CHECK(placement_map(&po, T, map) == NMG_ERR_INVALID);
  po.source = NMG_PLACE_HUGE;
  CHECK(placement_map(&po, T, map) == NMG_OK);

  // entries: 0 a dense object of 4 pages; 1 [stack], 10^8 pages; 2 a sparse heap
  // object of 2^23 pages; 3 a dense object of 3 pages
  const uint64_t kStack = 100000000ull, kBig = 1ull << 23;
  const uint64_t npages[4] = {4, kStack, kBig, 3};
  uint8_t dense[4];
  for (int e = 0; e < 4; e++) dense[e] = npages[e] * T <= kMaxEntryCells;
  CHECK(dense[0] && !dense[1] && !dense[2] && dense[3]);
  // (entry, thread, page, count), sorted by entry
  const uint32_t cells[][4] = {
      {0, 0, 1, 9},                                  // e0 page 1: node 0
      {0, 2, 2, 5},                                  // e0 page 2: 5 alone; with e2's 5 the site's page 2 qualifies
      {1, 0, 0, 20},        {1, 1, 99999999, 20},    // [stack]: its first and its last page, node 0
      {1, 2, 70000000, 9},  {1, 3, 70000000, 9},     //   a page above 2^26: node 1 through two threads (18)
      {1, 0, 70000001, 8},                           //   exactly the threshold: out
      {1, 0, 70000002, 12}, {1, 2, 70000002, 12},    //   a tie: node 0
      {2, 3, 2, 5},                                  // e2 page 2 (see e0)
      {2, 0, 3, 30},                                 // e2 page 3: the site's last row
      {2, 0, 4, 30},        {2, 1, 8388607, 30},     // e2 pages past the site's 4 rows; its own last page
      {3, 3, 0, 50},
  };
  const int64_t nc = (int64_t)(sizeof(cells) / sizeof(cells[0]));

  // 1. and 3.: every entry its own group
  {
    PlaceGroups g;
    placement_object_groups(4, npages, dense, g, true);
    CHECK(g.gid.size() == 4 && g.huge[0] == 0 && g.huge[1] == 1 && g.huge[2] == 1 && g.huge[3] == 0);
    CHECK(g.rows[1] == kStack && g.any_huge());
    Rows r;
    placement_blocks_host(g, map, &cells[0][0], nc, 4, r);
    CHECK(r.size() == 5 * 6);
    CHECK(row_is(r, 0, 0, 0, 1, 1, 9));
    CHECK(row_is(r, 1, 1, 0, 0, 0, 20));
    CHECK(row_is(r, 2, 1, 1, 70000000, 70000000, 18));
    CHECK(row_is(r, 3, 1, 0, 70000002, 99999999, 32));  // the tie's lower node, extended to the last page
    CHECK(row_is(r, 4, 2, 0, 3, 8388607, 90));
    CHECK(row_is(r, 5, 3, 1, 0, 0, 50));
    PlaceGroups g0;
    placement_object_groups(4, npages, dense, g0);
    CHECK(g0.gid.size() == 2 && !g0.any_huge());
    Rows r0;
    placement_blocks_host(g0, map, &cells[0][0], nc, 4, r0);
    CHECK(r0.size() == 5 * 2 && row_is(r0, 0, 0, 0, 1, 1, 9) && row_is(r0, 1, 3, 1, 0, 0, 50));
  }
  // 2. a site of the dense entry 0 (which created it: 4 rows) and the sparse entry 2
  {
    const std::vector<uint32_t> members = {0, 2};
    PlaceGroups g;
    g.add(7, 4, members, npages, dense, true);
    CHECK(g.gid.size() == 1 && g.huge[0] == 1 && g.rows[0] == 4 && g.m_np[0] == 4 && g.m_np[1] == 4);
    CHECK(g.m_dense[0] == 1 && g.m_dense[1] == 0);
    Rows r;
    placement_blocks_host(g, map, &cells[0][0], nc, 4, r);
    CHECK(r.size() == 5 * 3);
    CHECK(row_is(r, 0, 7, 0, 1, 1, 9));
    CHECK(row_is(r, 1, 7, 1, 2, 2, 10));  // 5 + 5 from the two members
    CHECK(row_is(r, 2, 7, 0, 3, 3, 30));  // page 4 and the last page: past the site's rows
    PlaceGroups g0;
    g0.add(7, 4, members, npages, dense);
    CHECK(g0.gid.size() == 1 && g0.huge[0] == 0 && g0.m_entry.size() == 1);
    Rows r0;
    placement_blocks_host(g0, map, &cells[0][0], nc, 4, r0);
    CHECK(r0.size() == 5 && row_is(r0, 0, 7, 0, 1, 1, 9));
  }
  printf("nmg_placement_huge_host: ok\n");
  return 0;
}
