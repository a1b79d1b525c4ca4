"""Expected page cost cells, derived from the oracle's dump files only (shared
by test_gpu_page_cost.py and test_page_cost_host.py; not a test module).

The oracle's -D dump lists every matched non-stack sample
(all_memory_accesses.dat: thread ts object_id offset mem_level weight
access_type), its -d dump the same per call site (callsite_dump_<id>.dat
without the object id).  Selecting those lines by level string and access and
binning them in numpy, with the rule of include/numamma_gpu.h, gives what the
engine's cells must hold.  The level string names the first level bit of the
record, so the string -> bucket map is exact for records with one level bit,
which is what the generator emits; records with several are checked against
the oracle's per-object level counters instead (redraw_levels)."""
import dataclasses
import os

import numpy as np

import placement_expect as px
from numamma_amd.replay import RECORD_DTYPE
from timeline_expect import MAX_ENTRY_CELLS, PAGE, read_dir, run_oracle  # noqa: F401 (re-exported)

COUNT, WEIGHT = 0, 1
NA = 0x40000
REMOTE = (1 << 5) | (1 << 6)
MEMORY = (1 << 4) | REMOTE
ALL = (1 << 18) - 1 | NA  # every bucket and the N/A bit

_GROUP = {"L1": 0, "L2": 1, "L3": 2, "LFB": 3, "Local_RAM": 4, "Remote_RAM_1_hop": 5, "Remote_RAM_2_hops": 5,
          "Remote_Cache_1_hop": 6, "Remote_Cache_2_hops": 6, "IO_Memory": 7, "Uncached_Memory": 8}


def sel_of(level):
    """The 19-bit selection mask of a dump line's level string."""
    if level == "Unknown":
        return 0
    for suffix, shift in (("_Hit", 0), ("_Miss", 9)):
        if level.endswith(suffix):
            base = level[:-len(suffix)]
            return NA if base == "NA" else 1 << (_GROUP[base] + shift)
    if level == "NA":
        return NA
    assert level in _GROUP, level  # a level bit without HIT or MISS: no bucket
    return 0


@dataclasses.dataclass(frozen=True)
class CostOpts:
    bucket_mask: int = MEMORY
    access_mask: int = 3
    metric: int = WEIGHT

    def kw(self):
        return dataclasses.asdict(self)


MEMORY_WEIGHT = CostOpts()
REMOTE_READS = CostOpts(REMOTE, 1, COUNT)
EVERYTHING = CostOpts(ALL, 3, COUNT)
OPTION_SETS = [MEMORY_WEIGHT, REMOTE_READS, EVERYTHING]
OPTION_IDS = ["memory-weight", "remote-reads-count", "all-count"]


def _lines(path, with_object):
    """(integer columns [thread, (object,) offset], sel mask, weight, access) of a dump file's lines."""
    cols, sel, w, acc = [], [], [], []
    k = 1 if with_object else 0
    with open(path) as f:
        for line in f:
            if line.startswith("#"):
                continue
            p = line.split()
            cols.append([int(p[0])] + ([int(p[2])] if with_object else []) + [int(p[2 + k])])
            sel.append(sel_of(p[3 + k]))
            w.append(int(p[4 + k]))
            acc.append({"r": 0, "w": 1}[p[5 + k]])
    return (np.array(cols, dtype=np.int64).reshape(-1, 2 + k), np.array(sel, dtype=np.int64),
            np.array(w, dtype=np.uint64), np.array(acc, dtype=np.int64))


def _sum(keys, vals):
    """Rows of equal keys summed: sorted unique keys with the sum appended, zero sums dropped."""
    if keys.shape[0] == 0:
        return np.zeros((0, keys.shape[1] + 1), dtype=np.uint64)
    u, inv = np.unique(keys, axis=0, return_inverse=True)
    s = np.zeros(u.shape[0], dtype=np.uint64)
    np.add.at(s, inv.reshape(-1), vals)
    out = np.concatenate([u.astype(np.uint64), s[:, None]], axis=1)
    return out[s != 0]


def _picked(sel, w, acc, o: CostOpts):
    keep = ((sel & o.bucket_mask) != 0) & (((1 << acc) & o.access_mask) != 0)
    return keep, (w if o.metric == WEIGHT else np.ones_like(w))


def dense(table, nb_threads):
    return px.dense(table, nb_threads)


class Dump:
    """all_memory_accesses.dat read once: the matched non-stack lines with their
    entry (table position), for any number of option sets."""

    def __init__(self, odir, table, nb_threads):
        a, self.sel, self.w, self.acc = _lines(os.path.join(odir, "all_memory_accesses.dat"), True)
        ids = table.entries["id"].astype(np.int64)
        pos = np.full(int(ids.max()) + 2, -1, dtype=np.int64)
        pos[ids] = np.arange(ids.shape[0])
        self.ent = pos[a[:, 1]]
        assert (self.ent >= 0).all()
        self.thread, self.page = a[:, 0], a[:, 2] >> 12
        self.dense = dense(table, nb_threads)[self.ent]
        self.nlines = int(a.shape[0])
        self.unknown = int((self.sel == 0).sum())

    def rows(self, o: CostOpts):
        """(entry, thread, page, value) u64 rows sorted by (entry, thread, page), and the lines selected."""
        keep, val = _picked(self.sel, self.w, self.acc, o)
        keep &= self.dense
        keys = np.stack([self.ent, self.thread, self.page], axis=1)[keep]
        return _sum(keys, val[keep]), int(keep.sum())


def object_matrices(rows, table, nb_threads):
    """{entry: mat[page][thread]} of every entry with a row."""
    npg = table.entries["buffer_size"].astype(np.int64) // PAGE + 1
    out = {}
    for e in np.unique(rows[:, 0]).tolist():
        r = rows[rows[:, 0] == e]
        m = np.zeros((int(npg[e]), nb_threads), dtype=np.uint64)
        m[r[:, 2].astype(np.int64), r[:, 1].astype(np.int64)] = r[:, 3]
        out[int(e)] = m
    return out


def object_blocks(rows, table, nb_threads, po: px.Opts):
    """nmg_get_object_blocks' rows from the cost rows: placement_expect.blocks_of per entry."""
    out = []
    for e, m in sorted(object_matrices(rows, table, nb_threads).items()):
        b = px.blocks_of(m, po)
        out.append(np.concatenate([np.full((b.shape[0], 1), e, dtype=np.uint64), b], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 5), dtype=np.uint64)


def site_matrices(odir, nb_threads, o: CostOpts):
    """{site id: mat[page][thread]} from callsite_dump_<id>.dat, the rows taken
    from the line count of the oracle's callsite_counters_<id>.dat; sites
    without a non-zero cell inside their rows left out."""
    out = {}
    for name in os.listdir(odir):
        if not name.startswith("callsite_dump_"):
            continue
        sid = int(name[len("callsite_dump_"):-len(".dat")])
        with open(os.path.join(odir, f"callsite_counters_{sid}.dat")) as f:
            nrows = sum(1 for _ in f)
        a, sel, w, acc = _lines(os.path.join(odir, name), False)
        keep, val = _picked(sel, w, acc, o)
        page = a[:, 1] >> 12
        keep &= page < nrows
        m = np.zeros((nrows, nb_threads), dtype=np.uint64)
        np.add.at(m, (page[keep], a[keep, 0]), val[keep])
        if m.any():
            out[sid] = m
    return out


def site_files(mats):
    """{file name: text} of callsite_cost_<id>.dat."""
    return {f"callsite_cost_{sid}.dat": "".join("".join(f"\t{v}" for v in row) + "\n" for row in m.tolist())
            for sid, m in mats.items()}


def site_blocks_text(odir, table, mats, po: px.Opts):
    """blocks.dat from the per-site cost matrices (placement_expect's site list and text)."""
    types = px.site_types(table)
    sites = []
    for sid, caller, size in sorted(px.read_sites(odir)):
        ident = px.identifier(caller, types[(caller, size)])
        if ident is None or sid not in mats:
            continue
        b = px.blocks_of(mats[sid], po)
        if b.shape[0]:
            sites.append((sid, caller, ident, size, b))
    return px.blocks_text(sites)


# ---- records with several level bits (test_gpu_route_levels.py's draw, restated)

LVL_NA, LVL_HIT, LVL_MISS = 0x01, 0x02, 0x04
LVL_L1, LVL_LFB, LVL_L2, LVL_L3, LVL_LOC_RAM = 0x08, 0x10, 0x20, 0x40, 0x80
LVL_REM_RAM1, LVL_REM_RAM2, LVL_REM_CCE1, LVL_REM_CCE2, LVL_IO, LVL_UNC = 0x100, 0x200, 0x400, 0x800, 0x1000, 0x2000
_BITS = [LVL_L1, LVL_LFB, LVL_L2, LVL_L3, LVL_LOC_RAM, LVL_REM_RAM1, LVL_REM_RAM2, LVL_REM_CCE1, LVL_REM_CCE2,
         LVL_IO, LVL_UNC]
ALL_LEVELS = ([LVL_HIT | b for b in _BITS] + [LVL_MISS | b for b in _BITS]
              + [LVL_HIT | LVL_MISS | b for b in _BITS]  # HIT beats MISS (quirk Q12)
              + [LVL_NA, LVL_NA | LVL_HIT | LVL_L3, LVL_NA | LVL_MISS | LVL_LOC_RAM, LVL_NA | LVL_L1]
              + [LVL_HIT | LVL_REM_RAM1 | LVL_REM_RAM2, LVL_MISS | LVL_REM_RAM1 | LVL_REM_RAM2,
                 LVL_HIT | LVL_REM_CCE1 | LVL_REM_CCE2, LVL_MISS | LVL_REM_CCE1 | LVL_REM_CCE2]
              + [LVL_HIT | LVL_L1 | LVL_L2 | LVL_IO, LVL_MISS | LVL_L3 | LVL_UNC | LVL_LFB]  # several groups at once
              + [LVL_L2, LVL_IO | LVL_UNC]  # a level without HIT or MISS: no bucket
              + [0])


def samples(rp):
    return [b.ring.view(RECORD_DTYPE) for b in rp.buffers]


def redraw_levels(rp, seed, levels=ALL_LEVELS):
    """Overwrite data_src.mem_lvl of every record with a draw from `levels`."""
    rng = np.random.default_rng(seed)
    lv = np.array(levels, dtype=np.uint64)
    keep = ~np.uint64(0x3FFF << 5)
    for rec in samples(rp):
        pick = lv[rng.integers(0, lv.shape[0], rec.shape[0])]
        rec["data_src"] = (rec["data_src"] & keep) | (pick << np.uint64(5))


def oracle_levels(raw):
    """The oracle's per-entry level counters as [E][2][37]: na_miss, then 18 x (count, weight sum)."""
    ent = raw.entries
    return np.stack([ent[:, 3:40], ent[:, 42:79]], axis=1).astype(np.uint64)


def entry_sums(rows, nb_entries):
    """The rows' values summed per entry."""
    s = np.zeros(nb_entries, dtype=np.uint64)
    np.add.at(s, rows[:, 0].astype(np.int64), rows[:, 3])
    return s
