"""Expected access-timeline rows, derived from the oracle's dump files only
(shared by test_gpu_timeline.py and test_timeline_host.py; not a test module).

The oracle's -D dump lists every matched non-stack sample
(all_memory_accesses.dat: thread ts object_id offset ...), its -d dump the
same per call site (callsite_dump_<id>.dat: thread ts offset ...).  Binning
those lines in numpy with the rule of include/numamma_gpu.h gives what the
engine's cells must hold."""
import dataclasses
import os

import numpy as np

import pyoracle
from numamma_amd.replay import T0
from numamma_amd.results import RawResults

PAGE = 4096
MAX_ENTRY_CELLS = 1 << 24  # a dense entry's pages * threads (CellCursor::place)


@dataclasses.dataclass(frozen=True)
class TlOpts:
    t0: int = T0 + (1 << 31)
    bin_shift: int = 29
    nb_bins: int = 12
    row_shift: int = 0
    min_object_bytes: int = 4096

    def kw(self):
        return dataclasses.asdict(self)


def run_oracle(rp, d, **kw):
    """The oracle over rp with both dump modes; (raw results, its output dir)."""
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, "replay.bin")
    rp.write(path)
    odir = os.path.join(d, "oracle")
    pyoracle.run(path, odir, os.path.join(d, "o.txt"), os.path.join(d, "o_raw.bin"), dump=True, dump_all=True, **kw)
    os.remove(path)
    return RawResults.read(os.path.join(d, "o_raw.bin")), odir


def _columns(path, ncol):
    """The first ncol (integer) columns of a dump file's lines."""
    out = []
    with open(path) as f:
        for line in f:
            if line.startswith("#"):
                continue
            out.append([int(x) for x in line.split(None, ncol)[:ncol]])
    return np.array(out, dtype=np.uint64).reshape(-1, ncol)


def bins_of(ts, o: TlOpts):
    ts = ts.astype(np.uint64)
    rel = np.where(ts < np.uint64(o.t0), np.uint64(0), ts - np.uint64(o.t0)) >> np.uint64(o.bin_shift)
    return np.minimum(rel, np.uint64(o.nb_bins - 1))


def selected(table, nb_threads, o: TlOpts):
    """Entries that get a timeline: dense page cells and at least min_object_bytes."""
    size = table.entries["buffer_size"].astype(np.uint64)
    pages = size // np.uint64(PAGE) + np.uint64(1)
    return (pages * np.uint64(nb_threads) <= np.uint64(MAX_ENTRY_CELLS)) & (size >= np.uint64(o.min_object_bytes))


def _count(cols):
    """Rows of equal columns counted: sorted unique rows with their counts appended."""
    if cols.shape[0] == 0:
        return np.zeros((0, cols.shape[1] + 1), dtype=np.uint64)
    u, c = np.unique(cols, axis=0, return_counts=True)
    return np.concatenate([u, c[:, None].astype(np.uint64)], axis=1)


def expected_rows(odir, table, nb_threads, o: TlOpts):
    """(entry, bin, thread, row, count) rows sorted by (entry, bin, thread, row),
    and the number of matched lines read."""
    a = _columns(os.path.join(odir, "all_memory_accesses.dat"), 4)  # thread ts object_id offset
    ids = table.entries["id"].astype(np.int64)
    pos = np.full(int(ids.max()) + 2, -1, dtype=np.int64)
    pos[ids] = np.arange(ids.shape[0])
    ent = pos[a[:, 2].astype(np.int64)]
    assert (ent >= 0).all()
    keep = selected(table, nb_threads, o)[ent]
    a, ent = a[keep], ent[keep]
    row = (a[:, 3] >> np.uint64(12)) >> np.uint64(o.row_shift)
    cols = np.stack([ent.astype(np.uint64), bins_of(a[:, 1], o), a[:, 0], row], axis=1)
    return _count(cols).astype(np.uint32), int(keep.shape[0])


def expected_site_files(odir, o: TlOpts):
    """{file name: text} of callsite_timeline_<id>.dat from the oracle's callsite_dump_<id>.dat."""
    out = {}
    for name in os.listdir(odir):
        if not name.startswith("callsite_dump_"):
            continue
        a = _columns(os.path.join(odir, name), 3)  # thread ts offset
        row = (a[:, 2] >> np.uint64(12)) >> np.uint64(o.row_shift)
        r = _count(np.stack([bins_of(a[:, 1], o), a[:, 0], row], axis=1))  # (bin, thread, row) order
        lines = ["#thread_rank timestamp offset count\n"]
        for b, th, rw, c in r.tolist():
            lines.append(f"{th} {o.t0 + (b << o.bin_shift)} {rw << (12 + o.row_shift)} {c}\n")
        out[name.replace("callsite_dump_", "callsite_timeline_")] = "".join(lines)
    return out


def read_dir(d, prefix):
    return {n: open(os.path.join(d, n)).read() for n in os.listdir(d) if n.startswith(prefix)}


def sum_over_bins(rows):
    """Timeline rows with the bins summed out: (entry, thread, row, count)."""
    if rows.shape[0] == 0:
        return np.zeros((0, 4), dtype=np.uint64)
    key = rows[:, [0, 2, 3]].astype(np.uint64)
    u, inv = np.unique(key, axis=0, return_inverse=True)
    c = np.bincount(inv.reshape(-1), weights=rows[:, 4].astype(np.float64), minlength=u.shape[0])
    return np.concatenate([u, c[:, None].astype(np.uint64)], axis=1)


def page_cells_by_row(cells, sel, row_shift):
    """eng.page_cells() rows of the selected entries grouped by page >> row_shift:
    (entry, thread, row, count), sorted like sum_over_bins."""
    c = cells[sel[cells[:, 0]]]
    rows = np.stack([c[:, 0], np.zeros(c.shape[0], dtype=np.uint32), c[:, 1], c[:, 2] >> row_shift, c[:, 3]], axis=1)
    return sum_over_bins(rows)
