"""Expected access-timeline rows with NMG_TL_SCOPE_ALL, derived from the
oracle's files only (shared by test_gpu_timeline_all.py and
test_timeline_all_host.py; not a test module).

With the scope an entry is selected by its size alone, so:

- non-stack entries, sparse or not: the lines of the oracle's -D dump
  (all_memory_accesses.dat lists the matched samples of sparse non-stack
  entries too), binned as timeline_expect does;
- [stack], which the dump omits, matches only ts = 0 samples (quirk Q4): its
  bin is 0 whatever t0 is, so its rows are the oracle's page cells of the stack
  entry in bin 0, grouped by row.

check_covers asserts, on the oracle's files alone, that the rows summed over
the bins are the oracle's page cells of every selected entry grouped by row:
nothing is left out.  The key layout of the timeline sparse table
(numamma_amd/csrc/nmg_internal.h: tl_sparse_key) is mirrored here."""
import os

import numpy as np

import placement_huge_expect as hx
import timeline_expect as tx
from numamma_amd.replay import MEM_STACK, RECORD_DTYPE

SCOPE_DENSE, SCOPE_ALL = 0, 1
MAX_SPARSE = 1023  # selected sparse entries (ordinals 0..1022)
SLOT_BYTES = 12    # a u64 key and a u32 count


# ---- the key: row:32 | thread:10 << 32 | bin:12 << 42 | ordinal:10 << 54

def tl_key(ordinal, b, thread, row):
    u = np.uint64
    return (np.asarray(ordinal, dtype=u) << u(54)) | (np.asarray(b, dtype=u) << u(42)) | \
           (np.asarray(thread, dtype=u) << u(32)) | np.asarray(row, dtype=u)


def tl_key_fields(k):
    k = np.asarray(k, dtype=np.uint64)
    u = np.uint64
    return k >> u(54), (k >> u(42)) & u(0xFFF), (k >> u(32)) & u(0x3FF), k & u(0xFFFFFFFF)


# ---- selection and rows

def selected_all(table, o: tx.TlOpts):
    """The scope's selection: the size rule alone."""
    return table.entries["buffer_size"].astype(np.uint64) >= np.uint64(o.min_object_bytes)


def stack_entry(table):
    st = np.flatnonzero(table.entries["mem_type"] == MEM_STACK)
    assert st.shape[0] <= 1
    return int(st[0]) if st.shape[0] else None


def _entry_of_lines(a, table):
    ids = table.entries["id"].astype(np.int64)
    pos = np.full(int(ids.max()) + 2, -1, dtype=np.int64)
    pos[ids] = np.arange(ids.shape[0])
    ent = pos[a[:, 2].astype(np.int64)]
    assert (ent >= 0).all()
    return ent


def expected_rows_all(odir, raw, table, o: tx.TlOpts):
    """(entry, bin, thread, row, count) u32 rows sorted by (entry, bin, thread, row)."""
    a = tx._columns(os.path.join(odir, "all_memory_accesses.dat"), 4)  # thread ts object_id offset
    ent = _entry_of_lines(a, table)
    st = stack_entry(table)
    assert st is None or not (ent == st).any()  # the dump omits [stack]
    keep = selected_all(table, o)[ent]
    a, ent = a[keep], ent[keep]
    row = (a[:, 3] >> np.uint64(12)) >> np.uint64(o.row_shift)
    rows = tx._count(np.stack([ent.astype(np.uint64), tx.bins_of(a[:, 1], o), a[:, 0], row], axis=1))
    if st is not None and selected_all(table, o)[st]:
        c = raw.cells[raw.cells[:, 0] == st].astype(np.uint64)  # (entry, thread, page, count)
        if c.shape[0]:
            s = tx.sum_over_bins(np.stack([c[:, 0], np.zeros(c.shape[0], dtype=np.uint64), c[:, 1],
                                           c[:, 2] >> np.uint64(o.row_shift), c[:, 3]], axis=1))  # (entry, thread, row, count)
            srows = np.stack([s[:, 0], np.zeros(s.shape[0], dtype=np.uint64), s[:, 1], s[:, 2], s[:, 3]], axis=1)
            rows = np.concatenate([rows, srows])
            rows = rows[np.lexsort((rows[:, 3], rows[:, 2], rows[:, 1], rows[:, 0]))]
    assert int(rows[:, 4].max(initial=0)) < 1 << 32
    return rows.astype(np.uint32)


def check_covers(rows, raw, table, o: tx.TlOpts):
    """The rows summed over the bins are the oracle's page cells of every selected entry, grouped by row."""
    sel = selected_all(table, o)
    want = tx.page_cells_by_row(raw.cells.astype(np.uint32), sel, o.row_shift)
    assert np.array_equal(tx.sum_over_bins(rows), want)
    return want


def sparse_ordinals(table, dense, o: tx.TlOpts):
    """{entry: ordinal} of the selected sparse entries, in id order (dense: the engine's dense entries)."""
    ids = np.flatnonzero(selected_all(table, o) & ~dense)
    return {int(e): k for k, e in enumerate(ids.tolist())}


def sparse_keys(rows, table, dense, o: tx.TlOpts):
    """The timeline sparse table's keys of the expected rows, ascending: the rows of sparse entries, in order."""
    ordn = sparse_ordinals(table, dense, o)
    r = rows[~dense[rows[:, 0]]]
    k = tl_key([ordn[int(e)] for e in r[:, 0]], r[:, 1], r[:, 2], r[:, 3])
    assert np.all(k[1:] > k[:-1]) and not (k == np.uint64(0xFFFFFFFFFFFFFFFF)).any()
    return k


# ---- the huge replay, its planted records spread over the bins

def restamp(rp, role, o: tx.TlOpts, roles=("H", "M")):
    """The records inside the entries `roles` re-stamped, in turn, with: the
    entry's alloc_date (below t0: bin 0), three timestamps inside bins 3, 6 and
    the last one, and its free_date (past the last bin's end: the clamp).  All
    inside [alloc_date, free_date]."""
    ent = rp.table.entries
    for r in roles:
        e = role[r]
        lo, size = int(ent["buffer_addr"][e]), int(ent["buffer_size"][e])
        al, fr = int(ent["alloc_date"][e]), int(ent["free_date"][e])
        stamps = np.array([al, o.t0 + (3 << o.bin_shift) + 17, o.t0 + (6 << o.bin_shift) + 1,
                           o.t0 + ((o.nb_bins - 1) << o.bin_shift), fr], dtype=np.uint64)
        assert al < o.t0 and fr >= o.t0 + (o.nb_bins << o.bin_shift) and all(al <= int(s) <= fr for s in stamps)
        for b in rp.buffers:
            rec = b.ring.view(RECORD_DTYPE)
            hit = np.flatnonzero((rec["addr"] >= np.uint64(lo)) & (rec["addr"] < np.uint64(lo + size)))
            rec["timestamp"][hit] = stamps[np.arange(hit.shape[0]) % stamps.shape[0]]
    return rp


def huge_replay_tl(o: tx.TlOpts, plan=None):
    """placement_huge_expect.huge_replay (H and M past the per-entry cap, a [stack] cell) with restamp."""
    stack = plan is None
    rp, role = hx.huge_replay(stack=stack, plan=plan)
    return restamp(rp, role, o), role
