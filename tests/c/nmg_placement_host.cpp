// Page-cell placement (CellCursor, numamma_amd/csrc/nmg_internal.h) on the
// CPU, no HIP involved: where nmg_set_objects and nmg_update_objects put an
// entry's cells.  Small budgets, so nothing large is allocated; built with
// the address and undefined-behaviour sanitizers by tests/test_layout_host.py.
#include <cstdio>

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

static const uint64_t kNoBase = ~0ull - 1;
static const uint32_t kNoIdx = ~0u - 1;

// a cursor for T threads whose budget is `per_thread` cells each, as the
// engine sets it up from hist_budget_bytes = per_thread * T * 4
static CellCursor cursor(uint64_t T, uint64_t per_thread) {
  CellCursor c;
  c.threads = T;
  c.budget_cells = per_thread * T * 4 / 4;
  return c;
}

struct Got {
  Placement how;
  uint64_t base;
  uint32_t sidx;
};
static Got place(CellCursor& c, uint64_t np, bool must_be_dense = false) {
  Got g{kPlaceDense, kNoBase, kNoIdx};
  g.how = c.place(np, must_be_dense, &g.base, &g.sidx);
  return g;
}
static bool same(const CellCursor& a, const CellCursor& b) {
  return a.threads == b.threads && a.budget_cells == b.budget_cells && a.cells == b.cells && a.nsparse == b.nsparse;
}

int main() {
  {  // dense: consecutive blocks, nothing else touched
    CellCursor c = cursor(2, 64);
    Got g = place(c, 3);
    CHECK(g.how == kPlaceDense && g.base == 0 && g.sidx == kNoIdx);
    g = place(c, 5);
    CHECK(g.how == kPlaceDense && g.base == 3 && g.sidx == kNoIdx);
    CHECK(c.cells == 8 && c.nsparse == 0);
  }
  {  // the per-entry cap: np * T at 2^24 is dense, one page more is not
    CellCursor c = cursor(2, 1ull << 40);
    const uint64_t np = kMaxEntryCells / 2;
    Got g = place(c, np);
    CHECK(g.how == kPlaceDense && g.base == 0 && c.cells == np);
    const CellCursor before = c;
    g = place(c, np + 1, true);  // an entry that must stay dense: refused, nothing changed
    CHECK(g.how == kPlaceOverBudget && g.base == kNoBase && g.sidx == kNoIdx && same(c, before));
    g = place(c, np + 1);
    CHECK(g.how == kPlaceSparse && g.sidx == 0 && g.base == kNoBase);
    CHECK(c.cells == np && c.nsparse == 1);
  }
  {  // the budget: the last cells fit exactly, one more does not
    CellCursor c = cursor(3, 64);
    CHECK(place(c, 60).how == kPlaceDense);
    const CellCursor at60 = c;
    Got g = place(c, 5);
    CHECK(g.how == kPlaceSparse && g.sidx == 0 && c.cells == 60);
    c = at60;
    CHECK(place(c, 5, true).how == kPlaceOverBudget && same(c, at60));
    g = place(c, 4);
    CHECK(g.how == kPlaceDense && g.base == 60 && c.cells == 64);
    CHECK(place(c, 1).how == kPlaceSparse);
  }
  {  // no budget at all (hist_budget_bytes = 4): every entry sparse, indices in order
    CellCursor c = cursor(1, 0);
    c.budget_cells = 1;
    CHECK(place(c, 1).how == kPlaceDense);  // (a single one-page entry of one thread still fits)
    c = cursor(2, 0);
    c.budget_cells = 1;
    Got g = place(c, 1);
    CHECK(g.how == kPlaceSparse && g.sidx == 0);
    g = place(c, 1);
    CHECK(g.how == kPlaceSparse && g.sidx == 1 && c.cells == 0 && c.nsparse == 2);
  }
  {  // the 32-bit cell index: cells stay below 2^32 - 1
    CellCursor c = cursor(1, 1ull << 40);
    c.cells = kMaxCellIndex - 10;
    Got g = place(c, 9);
    CHECK(g.how == kPlaceDense && g.base == kMaxCellIndex - 10 && c.cells == kMaxCellIndex - 1);
    const CellCursor before = c;
    CHECK(place(c, 1, true).how == kPlaceOverBudget && same(c, before));
    g = place(c, 1);
    CHECK(g.how == kPlaceSparse && c.cells == kMaxCellIndex - 1);
  }
  {  // the sparse-entry limit
    CellCursor c = cursor(1, 0);
    c.nsparse = kMaxSparse - 1;
    Got g = place(c, 7);
    CHECK(g.how == kPlaceSparse && g.sidx == kMaxSparse - 1 && c.nsparse == kMaxSparse);
    const CellCursor before = c;
    g = place(c, 7);
    CHECK(g.how == kPlaceSparseFull && g.sidx == kNoIdx && g.base == kNoBase && same(c, before));
    // the index still fits sparse_key's 22-bit field
    CHECK(sparse_key_idx(sparse_key(kMaxSparse - 1, 0x3ff, ~0u)) == kMaxSparse - 1);
  }
  {  // the arena is padded to a multiple of 4 cells per thread; the cursor itself is not moved
    CellCursor c = cursor(2, 64);
    const uint64_t in[] = {0, 1, 3, 4, 5, 8, 61}, out[] = {0, 4, 4, 4, 8, 8, 64};
    for (int i = 0; i < 7; i++) {
      c.cells = in[i];
      CHECK(c.padded_cells() == out[i] && c.cells == in[i]);
    }
  }
  if (g_failed) return 1;
  printf("nmg_placement_host: ok\n");
  return 0;
}
