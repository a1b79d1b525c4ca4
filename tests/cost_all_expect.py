"""Expected page cost cells with NMG_COST_SCOPE_ALL, derived from the oracle's
files only (shared by test_gpu_page_cost_all.py and test_page_cost_all_host.py;
not a test module).

With the scope every entry has cost cells, so:

- non-stack entries, sparse or not: cost_expect.Dump with its `dense` mask all
  true -- the lines of the oracle's -D dump of every entry;
- [stack], which the dump omits, is pinned two ways from the oracle's raw dump:
  per bucket (a one-bucket mask over cost_expect.redraw_levels' records: an
  entry's rows summed are the oracle's per-object level count or weight sum,
  the stack entry's included) and per cell (records redrawn from SELECTED, the
  levels whose selection mask is non-zero: with every bucket selected and the
  count metric the cost rows of every entry are the oracle's page cells).

check_dump_covers asserts, on the oracle's files alone, that the dump's lines
plus the stack's page cells are the raw dump's page cells: nothing else is
left out of the dump."""
import numpy as np

import cost_expect as cx
import placement_expect as px
import placement_huge_expect as hx

SCOPE_DENSE, SCOPE_ALL = 0, 1

_GROUP_BITS = [cx.LVL_L1, cx.LVL_L2, cx.LVL_L3, cx.LVL_LFB, cx.LVL_LOC_RAM, cx.LVL_REM_RAM1 | cx.LVL_REM_RAM2,
               cx.LVL_REM_CCE1 | cx.LVL_REM_CCE2, cx.LVL_IO, cx.LVL_UNC]  # struct mem_counters' bucket order


def sel(lvl):
    """The 19-bit selection mask of a mem_lvl field (the rule of include/numamma_gpu.h)."""
    m = cx.NA if lvl & cx.LVL_NA else 0
    shift = 0 if lvl & cx.LVL_HIT else 9 if lvl & cx.LVL_MISS else None
    if shift is not None:
        for g, bits in enumerate(_GROUP_BITS):
            if lvl & bits:
                m |= 1 << (g + shift)
    return m


def selected_levels():
    """The levels of cost_expect.ALL_LEVELS that EVERYTHING selects: a HIT or
    MISS with a level bit, or NA.  The property is asserted from sel()."""
    L = [l for l in cx.ALL_LEVELS if sel(l) != 0]
    level_bits = 0x3FF8
    for l in cx.ALL_LEVELS:
        want = bool(l & cx.LVL_NA) or bool((l & (cx.LVL_HIT | cx.LVL_MISS)) and (l & level_bits))
        assert (sel(l) != 0) == want and (sel(l) & cx.ALL) == sel(l), hex(l)
    assert 0 < len(L) < len(cx.ALL_LEVELS) and all(sel(l) & cx.EVERYTHING.bucket_mask for l in L)
    return L


SELECTED = selected_levels()


class DumpAll(cx.Dump):
    """cost_expect.Dump over every entry: the `dense` mask all true."""

    def __init__(self, odir, table, nb_threads):
        super().__init__(odir, table, nb_threads)
        self.table_dense = self.dense  # (of the default budget's per-entry cap; kept for the dense-scope rows)
        self.dense = np.ones_like(self.dense)

    def dense_rows(self, o):
        """The scope-dense rows (cost_expect.Dump.rows as it is)."""
        all_true, self.dense = self.dense, self.table_dense
        try:
            return self.rows(o)[0]
        finally:
            self.dense = all_true

    def line_cells(self):
        """(entry, thread, page, lines) u64 rows over every line, selected or not."""
        keys = np.stack([self.ent, self.thread, self.page], axis=1)
        return cx._sum(keys, np.ones(keys.shape[0], dtype=np.uint64))


def stack_entry(table):
    from numamma_amd.replay import MEM_STACK
    st = np.flatnonzero(table.entries["mem_type"] == MEM_STACK)
    assert st.shape[0] == 1
    return int(st[0])


def check_dump_covers(dump, raw, table):
    """The all-true dump's lines plus [stack]'s page cells are raw.cells (oracle files only)."""
    st = stack_entry(table)
    cells = raw.cells.astype(np.uint64)
    lines = dump.line_cells()
    assert not (lines[:, 0] == st).any()
    both = np.concatenate([lines, cells[cells[:, 0] == st]])
    both = both[np.lexsort((both[:, 2], both[:, 1], both[:, 0]))]
    assert both.shape == cells.shape and np.array_equal(both, cells)
    return int((cells[:, 0] == st).sum())


def with_times(rows, times):
    out = rows.copy()
    out[:, 3] *= np.uint64(times)
    return out


def bucket_sums(raw, bucket, metric, access_mask):
    """Per entry the oracle's level count (COUNT) or weight sum (WEIGHT) of one bucket (18: N/A, count only)."""
    lv = cx.oracle_levels(raw)
    word = 0 if bucket == 18 else 1 + 2 * bucket + metric
    want = np.zeros(lv.shape[0], dtype=np.uint64)
    for a in (0, 1):
        if access_mask & (1 << a):
            want += lv[:, a, word]
    return want


def object_blocks_all(rows, table, nb_threads, po: px.Opts):
    """nmg_get_object_blocks' rows from cost rows of every entry: placement_huge_expect.blocks_of_cells
    per entry over its (thread, page, value) rows, with the entry's page limit."""
    npg = table.entries["buffer_size"].astype(np.uint64) // np.uint64(px.PAGE) + np.uint64(1)
    out = []
    for e in np.unique(rows[:, 0]).tolist():
        c = rows[rows[:, 0] == e][:, 1:]
        b = hx.blocks_of_cells(c, po, nb_threads, min(int(npg[int(e)]), 0xFFFFFFFF))
        out.append(np.concatenate([np.full((b.shape[0], 1), e, dtype=np.uint64), b], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 5), dtype=np.uint64)
