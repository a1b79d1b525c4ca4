"""Expected NUMA-placement blocks, derived from the oracle's files only (shared
by test_placement_host.py and test_gpu_placement.py; not a test module).

A numpy restatement of the rule in include/numamma_gpu.h.  Per call site it
reads the oracle's callsite_counters_<id>.dat (rows = pages, columns =
threads) and call_sites.log (id, caller, size); a site's memory type comes
from the replay table's entries with that caller and initial size.  Per object
it takes the page cells of the oracle's raw dump."""
import dataclasses
import os
import re

import numpy as np

import pyoracle
from numamma_amd.replay import MEM_DYNAMIC, MEM_GLOBAL
from numamma_amd.results import RawResults

PAGE = 4096
MAX_ENTRY_CELLS = 1 << 24  # a dense entry's pages * threads (CellCursor::place)


@dataclasses.dataclass(frozen=True)
class Opts:
    nb_nodes: int
    thread_node: tuple = None  # None: rank // (T // nb_nodes)
    density_threshold: int = 8

    def kw(self):
        return dict(nb_nodes=self.nb_nodes, density_threshold=self.density_threshold,
                    thread_node=None if self.thread_node is None else np.array(self.thread_node, dtype=np.uint32))

    def node_of(self, T):
        if self.thread_node is not None:
            return np.array(self.thread_node, dtype=np.int64)
        assert T % self.nb_nodes == 0
        return np.arange(T, dtype=np.int64) // (T // self.nb_nodes)


def run_oracle(rp, d, **kw):
    """The oracle over rp; (raw results, its output dir)."""
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, "replay.bin")
    rp.write(path)
    odir = os.path.join(d, "oracle")
    pyoracle.run(path, odir, os.path.join(d, "o.txt"), os.path.join(d, "o_raw.bin"), **kw)
    os.remove(path)
    return RawResults.read(os.path.join(d, "o_raw.bin")), odir


def page_dom(mat, o: Opts):
    """mat[page][thread] -> (dom, cnt) per page: the lowest node with the
    largest count, and that count."""
    T = mat.shape[1]
    node_of = o.node_of(T)
    c = np.zeros((mat.shape[0], o.nb_nodes), dtype=np.uint64)
    for n in range(o.nb_nodes):
        c[:, n] = mat[:, node_of == n].sum(axis=1, dtype=np.uint64)
    dom = np.argmax(c, axis=1)  # (the first maximum)
    return dom, c[np.arange(c.shape[0]), dom]


def blocks_of(mat, o: Opts):
    """The blocks of one group as (node, start, end, count) u64 rows."""
    dom, cnt = page_dom(mat, o)
    pages = np.flatnonzero(cnt > np.uint64(o.density_threshold))
    if pages.shape[0] == 0:
        return np.zeros((0, 4), dtype=np.uint64)
    nodes = dom[pages]
    first = np.flatnonzero(np.concatenate([[True], nodes[1:] != nodes[:-1]]))
    last = np.concatenate([first[1:], [pages.shape[0]]]) - 1
    count = np.add.reduceat(cnt[pages], first)
    return np.stack([nodes[first].astype(np.uint64), pages[first].astype(np.uint64), pages[last].astype(np.uint64),
                     count.astype(np.uint64)], axis=1)


# ---- objects

def dense(table, nb_threads):
    pages = table.entries["buffer_size"].astype(np.uint64) // np.uint64(PAGE) + np.uint64(1)
    return pages * np.uint64(nb_threads) <= np.uint64(MAX_ENTRY_CELLS)


def object_matrices(raw, table, times=1):
    """{entry: mat[page][thread]} of every dense entry with a page cell."""
    T = raw.nb_threads
    ok = dense(table, T)
    npg = table.entries["buffer_size"].astype(np.int64) // PAGE + 1
    cells = raw.cells
    out = {}
    bounds = np.flatnonzero(np.concatenate([[True], cells[1:, 0] != cells[:-1, 0], [True]])) if cells.shape[0] else []
    for a, b in zip(bounds[:-1], bounds[1:]):
        e = int(cells[a, 0])
        if not ok[e]:
            continue
        m = np.zeros((int(npg[e]), T), dtype=np.uint64)
        m[cells[a:b, 2], cells[a:b, 1]] = cells[a:b, 3].astype(np.uint64) * np.uint64(times)
        out[e] = m
    return out


def object_rows(raw, table, o: Opts, times=1):
    """(entry, node, start, end, count) rows sorted by (entry, start)."""
    rows = []
    for e, m in sorted(object_matrices(raw, table, times).items()):
        b = blocks_of(m, o)
        rows.append(np.concatenate([np.full((b.shape[0], 1), e, dtype=np.uint64), b], axis=1))
    return np.concatenate(rows) if rows else np.zeros((0, 5), dtype=np.uint64)


# ---- call sites

_SITE = re.compile(r"^(\d+)\t(.*) \(size=(\d+)\) - ")


def read_sites(odir):
    """[(id, caller, size)] of call_sites.log."""
    out = []
    with open(os.path.join(odir, "call_sites.log")) as f:
        for line in f:
            m = _SITE.match(line)
            assert m, line
            out.append((int(m.group(1)), m.group(2), int(m.group(3))))
    return out


def site_matrix(odir, sid, times=1):
    """callsite_counters_<id>.dat as mat[page][thread] (the file prints u32 cells with %d)."""
    m = np.loadtxt(os.path.join(odir, f"callsite_counters_{sid}.dat"), dtype=np.int64, ndmin=2)
    return (m & 0xFFFFFFFF).astype(np.uint64) * np.uint64(times)


def site_types(table):
    """{(caller, initial size): mem_type} of the table's entries."""
    ent = table.entries
    out = {}
    for e in range(table.nb_entries):
        out.setdefault((table.caller(e), int(ent["initial_buffer_size"][e])), int(ent["mem_type"][e]))
    return out


def identifier(caller, mem_type):
    """What blocks.dat names the site by, or None when it is skipped."""
    if mem_type == MEM_DYNAMIC:
        return "malloc"
    if mem_type == MEM_GLOBAL and caller and not re.search(r"[\s\[/]", caller):
        return caller
    return None


def site_blocks(odir, table, o: Opts, times=1):
    """[(id, caller, identifier, size, blocks)] in ascending id of the sites blocks.dat lists."""
    types = site_types(table)
    out = []
    for sid, caller, size in sorted(read_sites(odir)):
        ident = identifier(caller, types[(caller, size)])
        if ident is None or not os.path.exists(os.path.join(odir, f"callsite_counters_{sid}.dat")):
            continue
        b = blocks_of(site_matrix(odir, sid, times), o)
        if b.shape[0]:
            out.append((sid, caller, ident, size, b))
    return out


def blocks_text(sites):
    lines = []
    for sid, caller, ident, size, b in sites:
        lines.append(f"#site {sid} {caller}\nbegin_block\n{ident} {size} {b.shape[0]}\n")
        lines += [f"{n} {s} {e} {c}\n" for n, s, e, c in b.tolist()]
        lines.append("end_block\n")
    return "".join(lines)


def expected_file(odir, table, o: Opts, times=1):
    return blocks_text(site_blocks(odir, table, o, times))
