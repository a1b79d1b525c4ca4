"""Canonical raw-results dump ("NMGRES01") and the host-only report.

Both the engine (nmg_run_replay(..., raw_path)) and the test oracle write
this format, so parity checks compare every counter bit for bit:

    "NMGRES01", u32 nb_entries, u32 nb_buffers, u32 nb_threads, u32 0
    u64 global[2][COUNTER_WORDS]  struct mem_counters x {read, write}
    u64 nb_samples_total, u64 nb_found_total
    u32 buf_samples[B], u32 buf_found[B]
    u64 entry[E][ENTRY_WORDS]  first-match ordinal, then per access GLOBAL_SUMS words:
                               count, weight, na_miss_count, NB_BUCKETS x (count, sum)
    u64 n, u32 cells[n][4]     (entry, thread, page, read+write count),
                               (entry, thread, page) order, non-zero only
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

# The engine's flat counter arrays (nmg_export_array), in u64 words: the Python
# mirror of the layout in numamma_amd/csrc/nmg_internal.h, which describes it.
# tests/test_layout_host.py compares every name here with the C++ one.
NB_BUCKETS = 18                       # NMG_NB_BUCKETS / kBuckets: 9 hit + 9 miss levels
GLOBAL_SUMS = 3 + 2 * NB_BUCKETS      # kGlobalSums: total_count, total_weight, na, NB_BUCKETS x (count, sum)
LEVEL_WORDS = 1 + 2 * NB_BUCKETS      # kLevelWords, per entry and access: na, NB_BUCKETS x (count, sum)
GLOBAL_SUM_WORDS = 2 * GLOBAL_SUMS    # kCwBase: sum64's head, [2 access][GLOBAL_SUMS]
CW_ROWS = 4                           # kCwRows: then [2 access][2][E] count / weight rows
GLOBAL_MIN_WORDS = 2 * NB_BUCKETS     # kGlobalMinMax: min64's head and all of max64, [2 access][NB_BUCKETS]
COUNTER_WORDS = 3 + 4 * NB_BUCKETS    # struct mem_counters: ... NB_BUCKETS x (count, min, max, sum)
ENTRY_WORDS = 1 + 2 * GLOBAL_SUMS     # the raw dump's record of one entry


def sum64_words(nb_entries: int, levels: bool) -> int:
    """sum64: the global sums, the rows, then [E][2][LEVEL_WORDS] with NMG_F_OBJECT_LEVELS."""
    return GLOBAL_SUM_WORDS + nb_entries * (CW_ROWS + (2 * LEVEL_WORDS if levels else 0))


def min64_words(nb_entries: int) -> int:
    """min64: the global minima, [E] first-match ordinals, the error word."""
    return GLOBAL_MIN_WORDS + nb_entries + 1


def max64_words() -> int:
    return GLOBAL_MIN_WORDS


@dataclass
class RawResults:
    nb_entries: int
    nb_buffers: int
    nb_threads: int
    global_counters: np.ndarray  # u64[2][COUNTER_WORDS]
    nb_samples: int
    nb_found: int
    buf_samples: np.ndarray
    buf_found: np.ndarray
    entries: np.ndarray  # u64[E][ENTRY_WORDS]
    cells: np.ndarray  # u32[n][4]

    @staticmethod
    def read(path: str) -> "RawResults":
        raw = open(path, "rb").read()
        if raw[:8] != b"NMGRES01":
            raise ValueError("not a raw-results dump")
        E, B, T, _ = np.frombuffer(raw, "<u4", 4, 8)
        off = 24
        g = np.frombuffer(raw, "<u8", 2 * COUNTER_WORDS, off).reshape(2, COUNTER_WORDS).copy()
        off += 8 * 2 * COUNTER_WORDS
        ns, nf = np.frombuffer(raw, "<u8", 2, off)
        off += 16
        bs = np.frombuffer(raw, "<u4", B, off).copy()
        off += 4 * B
        bf = np.frombuffer(raw, "<u4", B, off).copy()
        off += 4 * B
        ent = np.frombuffer(raw, "<u8", E * ENTRY_WORDS, off).reshape(E, ENTRY_WORDS).copy()
        off += 8 * ENTRY_WORDS * E
        (n,) = np.frombuffer(raw, "<u8", 1, off)
        off += 8
        cells = np.frombuffer(raw, "<u4", 4 * int(n), off).reshape(int(n), 4).copy()
        return RawResults(int(E), int(B), int(T), g, int(ns), int(nf), bs, bf, ent, cells)

    @property
    def first_ordinal(self) -> np.ndarray:
        return self.entries[:, 0]

    @property
    def count_weight(self) -> np.ndarray:
        cw = np.zeros((self.nb_entries, 2, 2), dtype=np.uint64)
        cw[:, 0, 0] = self.entries[:, 1]
        cw[:, 0, 1] = self.entries[:, 2]
        cw[:, 1, 0] = self.entries[:, 1 + GLOBAL_SUMS]
        cw[:, 1, 1] = self.entries[:, 2 + GLOBAL_SUMS]
        return cw


def report_host(res: RawResults, table, buf_bytes: np.ndarray, output_dir: str,
                stdout_path: Optional[str], match_samples: bool = True, dump_single_items: int = 1,
                dump_flags: int = 0, modules=None, online: bool = False) -> None:
    """nmg_report_host(): the report from host arrays (no GPU involved).
    dump_flags: NMG_DUMP_ALL writes all_memory_objects.dat (the sample dumps
    need the engine's per-sample matches: nmg_report)."""
    from . import _lib
    from .engine import build_meta

    hr, keep = _host_results(res, table, buf_bytes, match_samples)
    meta, kmeta = build_meta(table)
    marr, nmods = _lib.module_array(modules)
    ro = _lib.nmg_report_options(output_dir.encode(), dump_single_items, dump_flags, None, None, marr, nmods,
                                 int(online))
    _lib.check(_lib.lib.nmg_report_host(C.byref(hr), meta, C.byref(ro),
                                        stdout_path.encode() if stdout_path else None))
    del keep, kmeta


def report_timeline_host(res: RawResults, table, output_dir: str, rows: np.ndarray, online: bool = False,
                         **timeline) -> None:
    """nmg_report_timeline_host(): callsite_timeline_<id>.dat files from host
    arrays (no GPU involved).  rows: (entry, bin, thread, row, count) as
    Engine.timeline_cells() returns them; timeline: the nmg_timeline_options
    fields the rows were counted with (t0, bin_shift, nb_bins, row_shift, ...)."""
    from . import _lib
    from .engine import build_meta

    hr, keep = _host_results(res, table, np.zeros(res.nb_buffers, dtype=np.uint64), True)
    meta, kmeta = build_meta(table)
    ro = _lib.nmg_report_options(output_dir.encode(), 1, 0, None, None, None, 0, int(online))
    tl = _lib.nmg_timeline_options(timeline.get("t0", 0), timeline.get("bin_shift", 0), timeline.get("nb_bins", 1),
                                   timeline.get("row_shift", 0), timeline.get("reserved", 0),
                                   timeline.get("min_object_bytes", 0), timeline.get("budget_bytes", 0))
    rows = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1, 5)
    _lib.check(_lib.lib.nmg_report_timeline_host(C.byref(hr), meta, C.byref(ro), C.byref(tl),
                                                 rows.ctypes.data_as(C.POINTER(C.c_uint32)), rows.shape[0]))
    del keep, kmeta


def report_page_cost_host(res: RawResults, table, output_dir: str, rows: np.ndarray, online: bool = False) -> None:
    """nmg_report_page_cost_host(): callsite_cost_<id>.dat files from host
    arrays (no GPU involved).  rows: u64 (entry, thread, page, value) as
    Engine.cost_cells() returns them."""
    from . import _lib
    from .engine import build_meta

    hr, keep = _host_results(res, table, np.zeros(res.nb_buffers, dtype=np.uint64), True)
    meta, kmeta = build_meta(table)
    ro = _lib.nmg_report_options(output_dir.encode(), 1, 0, None, None, None, 0, int(online))
    rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, 4)
    _lib.check(_lib.lib.nmg_report_page_cost_host(C.byref(hr), meta, C.byref(ro),
                                                  rows.ctypes.data_as(C.POINTER(C.c_uint64)), rows.shape[0]))
    del keep, kmeta


def report_placement_host(res: RawResults, table, output_dir: str, nb_nodes: int, thread_node=None,
                          density_threshold: int = 8, online: bool = False, source: int = 0) -> None:
    """nmg_report_placement_host(): <output_dir>/blocks.dat from host arrays (no
    GPU involved), the options as Engine.report_placement takes them (source:
    NMG_PLACE_PAGE_COUNTS, or with NMG_PLACE_HUGE)."""
    from . import _lib
    from .engine import build_meta

    hr, keep = _host_results(res, table, np.zeros(res.nb_buffers, dtype=np.uint64), True)
    meta, kmeta = build_meta(table)
    ro = _lib.nmg_report_options(output_dir.encode(), 1, 0, None, None, None, 0, int(online))
    po, kmap = _lib.placement_options(res.nb_threads, nb_nodes, thread_node, density_threshold, source=source)
    _lib.check(_lib.lib.nmg_report_placement_host(C.byref(hr), meta, C.byref(ro), C.byref(po)))
    del keep, kmeta, kmap


def object_blocks_host(res: RawResults, table, nb_nodes: int, thread_node=None,
                       density_threshold: int = 8, source: int = 0) -> np.ndarray:
    """Engine.object_blocks' rows computed on the host from res.cells (internal:
    the library's host statement of the rule; tools/placement_timing.py)."""
    from . import _lib

    hr, keep = _host_results(res, table, np.zeros(res.nb_buffers, dtype=np.uint64), True)
    po, kmap = _lib.placement_options(res.nb_threads, nb_nodes, thread_node, density_threshold, source=source)
    n = _lib.check(_lib.lib.nmg_debug_object_blocks_host(C.byref(hr), C.byref(po), None, 0))
    rows = np.empty((n, 5), dtype=np.uint64)
    _lib.check(_lib.lib.nmg_debug_object_blocks_host(C.byref(hr), C.byref(po),
                                                     rows.ctypes.data_as(C.POINTER(C.c_uint64)), n))
    del keep, kmap
    return rows


def _host_results(res: RawResults, table, buf_bytes: np.ndarray, match_samples: bool):
    """struct nmg_host_results over res's arrays, and what keeps them alive."""
    from . import _lib
    from .engine import table_objects

    hr = _lib.nmg_host_results()
    gbytes = np.ascontiguousarray(res.global_counters, dtype="<u8").tobytes()
    C.memmove(C.addressof(hr.global_), gbytes, len(gbytes))
    keep = []

    def p(a, dt, ct):
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a.ctypes.data_as(C.POINTER(ct))

    hr.nb_buffers = res.nb_buffers
    hr.nb_entries = res.nb_entries
    hr.buf_samples = p(res.buf_samples, np.uint32, C.c_uint32)
    hr.buf_found = p(res.buf_found, np.uint32, C.c_uint32)
    hr.buf_bytes = p(buf_bytes, np.uint64, C.c_uint64)
    hr.buffer_size = p(table.entries["buffer_size"], np.uint64, C.c_uint64)
    hr.first_ordinal = p(res.first_ordinal, np.uint64, C.c_uint64)
    hr.count_weight = p(res.count_weight, np.uint64, C.c_uint64)
    hr.cells = p(res.cells, np.uint32, C.c_uint32)
    hr.nb_cells = res.cells.shape[0]
    hr.nb_threads = res.nb_threads
    hr.match_samples = int(match_samples)
    objs = table_objects(table)
    keep.append(objs)
    hr.objects = objs.ctypes.data_as(C.POINTER(_lib.nmg_object))
    return hr, keep
