"""Expected NUMA-placement blocks with NMG_PLACE_HUGE, and the replay with a
truly huge heap object (shared by test_placement_huge_host.py and
test_gpu_placement_huge.py; not a test module).

With the flag every entry contributes, so the rule of include/numamma_gpu.h is
restated here over the (entry, thread, page, count) cells of the oracle's raw
dump alone: no [pages][threads] matrix is built ([stack] has 10^8 pages).  For
call sites placement_expect.expected_file already is the flagged expectation:
the oracle's callsite_counters_<id>.dat sums all of a site's members."""
import numpy as np

import placement_expect as px
from numamma_amd.replay import HORIZON, MEM_DYNAMIC, MEM_STACK, RECORD_DTYPE, T0, SynthConfig, generate

PAGE = px.PAGE
D = 8
T = 8
PRIMARY = px.Opts(4, (0, 0, 1, 1, 3, 3, 3, 3), D)
SOURCE_HUGE = 4  # NMG_PLACE_PAGE_COUNTS | NMG_PLACE_HUGE


def page_table(cells, o: px.Opts, nb_threads, limit=None, times=1):
    """(pages, dom, cnt) of the touched pages of one group, pages ascending:
    cells are (thread, page, count) rows (any order, any number of members)."""
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    if limit is not None:
        cells = cells[cells[:, 1] < limit]
    if cells.shape[0] == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z.astype(np.uint64)
    node = o.node_of(nb_threads)[cells[:, 0]]
    key, inv = np.unique(cells[:, 1] * 64 + node, return_inverse=True)
    s = np.zeros(key.shape[0], dtype=np.uint64)
    np.add.at(s, inv.reshape(-1), cells[:, 2].astype(np.uint64) * np.uint64(times))
    page, nd = key >> 6, key & 63
    # per page the largest sum, the lowest node on a tie: (page, -sum, node) order, the first of each page
    order = np.lexsort((nd, -s.astype(np.int64), page))
    page, nd, s = page[order], nd[order], s[order]
    first = np.flatnonzero(np.concatenate([[True], page[1:] != page[:-1]]))
    return page[first], nd[first], s[first]


def blocks_of_cells(cells, o: px.Opts, nb_threads, limit=None, times=1):
    """The blocks of one group as (node, start, end, count) u64 rows."""
    page, dom, cnt = page_table(cells, o, nb_threads, limit, times)
    q = cnt > np.uint64(o.density_threshold)
    page, dom, cnt = page[q], dom[q], cnt[q]
    if page.shape[0] == 0:
        return np.zeros((0, 4), dtype=np.uint64)
    first = np.flatnonzero(np.concatenate([[True], dom[1:] != dom[:-1]]))
    last = np.concatenate([first[1:], [page.shape[0]]]) - 1
    return np.stack([dom[first].astype(np.uint64), page[first].astype(np.uint64), page[last].astype(np.uint64),
                     np.add.reduceat(cnt, first).astype(np.uint64)], axis=1)


def entry_cells(raw):
    """{entry: (thread, page, count) rows} of the raw dump's cells."""
    cells = raw.cells
    if cells.shape[0] == 0:
        return {}
    b = np.flatnonzero(np.concatenate([[True], cells[1:, 0] != cells[:-1, 0], [True]]))
    return {int(cells[a0, 0]): cells[a0:a1, 1:] for a0, a1 in zip(b[:-1], b[1:])}


def object_rows_all(raw, table, o: px.Opts, times=1):
    """(entry, node, start, end, count) rows sorted by (entry, start), over every entry's cells."""
    npg = table.entries["buffer_size"].astype(np.uint64) // np.uint64(PAGE) + np.uint64(1)
    rows = []
    for e, c in sorted(entry_cells(raw).items()):
        b = blocks_of_cells(c, o, raw.nb_threads, min(int(npg[e]), 0xFFFFFFFF), times)
        rows.append(np.concatenate([np.full((b.shape[0], 1), e, dtype=np.uint64), b], axis=1))
    return np.concatenate(rows) if rows else np.zeros((0, 5), dtype=np.uint64)


def blocks(rows, e):
    return [tuple(r) for r in rows[rows[:, 0] == e][:, 1:].tolist()]


def file_blocks(text, sid):
    """The (node, start, end, count) lines of site sid in a blocks.dat text, or None."""
    lines = text.split("\n")
    for i, line in enumerate(lines):
        if line.startswith(f"#site {sid} "):
            n = int(lines[i + 2].split()[-1])
            return [tuple(int(x) for x in l.split()) for l in lines[i + 3:i + 3 + n]]
    return None


# ---- the replay with a truly huge heap object

HUGE_CFG = SynthConfig(nb_samples=30_000, nb_intervals=400, nb_threads=T, heap_clusters=2, seed=212)
H_PAGES = (1 << 21) + 3  # * 8 threads > 2^24 cells: sparse whatever the budget
M_PAGES = (1 << 21) + 1
STACK_PAGE = (1 << 26) + 5
T_A, T_B, T_N1, T_N3 = 0, 1, 2, 4  # two threads of node 0, one of node 1, one of node 3 under PRIMARY


def huge_plan(stack):
    """(role, page, thread, count) of the crafted records; H's situations by name."""
    last = H_PAGES - 1
    plan = [
        ("H", 0, T_A, 20), ("H", last, T_N1, 20),              # page 0 and the last page
        ("H", 1000, T_A, 20), ("H", 1001, T_A, 20),            # two adjacent pages of one node
        ("H", 2000, T_A, 20), ("H", 2001, T_N3, 20),           # two adjacent pages of different nodes
        ("H", 3000, T_A, 15), ("H", 3000, T_N1, 15),           # a tie: the lower node
        ("H", 4000, T_N3, D), ("H", 4002, T_N3, D + 1),        # exactly D (out), D + 1 (in)
        ("H", 5000, T_N1, 20), ("H", 5001, T_N1, 3), ("H", 5002, T_N1, 20),  # a touched page that does not qualify between
        ("H", 6000, T_A, 5), ("H", 6000, T_B, 5),              # two threads of one node: only their sum passes D
        ("M", 7, T_N3, 20), ("M", M_PAGES - 1, T_N1, 20),
    ]
    if stack:
        plan.append(("stack", STACK_PAGE, T_A, 20))
    return plan


def huge_replay(stack=False, plan=None):
    """(replay, {role: entry}): H, the last dynamic entry below [stack], grown to
    H_PAGES pages (address space only), M, the last entry of the first heap
    cluster, grown to M_PAGES -- each with a size of its own, so its own call
    site -- and the plan's records written over the first records of four
    buffers.  stack: also a [stack] cell (ts = 0) on a page >= 2^26.  plan:
    other (role, page, thread, count) records than huge_plan's."""
    rp = generate(HUGE_CFG)
    t = rp.table
    ent = t.entries
    eo = t.entry_off.astype(np.int64)
    key_of = np.repeat(np.arange(t.nb_keys), np.diff(eo))
    single = np.diff(eo)[key_of] == 1
    clean = (ent["mem_type"] == MEM_DYNAMIC) & single & (ent["buffer_size"] == ent["initial_buffer_size"])
    dyn = np.flatnonzero(ent["mem_type"] == MEM_DYNAMIC)
    H = int(dyn[-1])
    gaps = ent["buffer_addr"][dyn[1:]].astype(np.int64) - ent["buffer_addr"][dyn[:-1]].astype(np.int64)
    M = int(dyn[int(np.argmax(gaps))])  # the entry before the gap between the clusters
    role = {"H": H, "M": M, "stack": int(np.flatnonzero(ent["mem_type"] == MEM_STACK)[0])}
    assert clean[H] and clean[M] and H != M and M < H - 50 and H == role["stack"] - 1
    lo = np.sort(np.array([int(ent["buffer_addr"][e]) for e in (H, M)], dtype=np.uint64))
    for e, pages, odd in ((H, H_PAGES, 8), (M, M_PAGES, 16)):
        ent["buffer_size"][e] = ent["initial_buffer_size"][e] = (pages - 1) * PAGE + odd
        nxt = int(t.keys[int(key_of[e]) + 1])
        assert int(ent["buffer_addr"][e]) + int(ent["buffer_size"][e]) < nxt  # room: address space only
        assert int((ent["initial_buffer_size"] == ent["initial_buffer_size"][e]).sum()) == 1
    # the generator's own records inside the two grown ranges aimed at no object
    new_hi = {int(ent["buffer_addr"][e]): int(ent["buffer_addr"][e]) + int(ent["buffer_size"][e]) for e in (H, M)}
    hi = np.array([new_hi[int(a)] for a in lo], dtype=np.uint64)
    for b in rp.buffers:
        rec = b.ring.view(RECORD_DTYPE)
        k = np.searchsorted(lo, rec["addr"], side="right") - 1
        hit = (k >= 0) & (rec["addr"] < hi[np.maximum(k, 0)])
        rec["addr"][hit] = 8
    plan = huge_plan(stack) if plan is None else plan
    for b, th in zip(rp.buffers, (T_A, T_B, T_N1, T_N3)):
        rec = b.ring.view(RECORD_DTYPE)
        mine = [(role[r], p, c) for r, p, t_, c in plan if t_ == th]
        n = sum(c for _, _, c in mine)
        assert b.data_tail == 0 and n < rec.shape[0]
        b.thread_rank = th
        if not mine:
            continue
        rec["addr"][:n] = np.concatenate([np.full(c, int(ent["buffer_addr"][e]) + p * PAGE, dtype=np.uint64)
                                          for e, p, c in mine])
        rec["timestamp"][:n] = np.concatenate([np.full(c, 0 if e == role["stack"] else T0 + HORIZON // 2, dtype=np.uint64)
                                               for e, p, c in mine])
        b.thread_rank = th
    return rp, role


def check_huge_expectation(raw, table, role, stack=False):
    """Assert, on the oracle's cells alone, that H's pages hold every situation; the flagged rows."""
    o = PRIMARY
    rows = object_rows_all(raw, table, o)
    H, M = role["H"], role["M"]
    page, dom, cnt = page_table(entry_cells(raw)[H], o, raw.nb_threads)
    at = {int(p): (int(n), int(c)) for p, n, c in zip(page, dom, cnt)}
    last = H_PAGES - 1
    assert int(table.entries["buffer_size"][H]) // PAGE + 1 == H_PAGES and not px.dense(table, T)[H]
    assert at[0] == (0, 20) and at[last] == (1, 20)
    assert at[1000] == at[1001] == (0, 20)
    assert at[2000] == (0, 20) and at[2001] == (3, 20)
    assert at[3000] == (0, 15)  # 15 : 15 between nodes 0 and 1
    assert at[4000] == (3, D) and at[4002] == (3, D + 1)
    assert at[5000] == at[5002] == (1, 20) and at[5001] == (1, 3)
    assert at[6000] == (0, 10)  # 5 + 5 from two threads of node 0
    assert blocks(rows, H) == [(0, 0, 2000, 80), (3, 2001, 2001, 20), (0, 3000, 3000, 15), (3, 4002, 4002, D + 1),
                               (1, 5000, 5002, 40), (0, 6000, 6000, 10), (1, last, last, 20)]
    assert blocks(rows, M) == [(3, 7, 7, 20), (1, M_PAGES - 1, M_PAGES - 1, 20)]
    if stack:
        assert blocks(rows, role["stack"]) == [(0, STACK_PAGE, STACK_PAGE, 20)]
    ids = rows[:, 0]
    assert ids[ids < M].shape[0] > 20 and ids[(ids > M) & (ids < H)].shape[0] > 20  # dense objects on both sides of M
    return rows
