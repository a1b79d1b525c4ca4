#!/usr/bin/env python3
"""What the device placement path saves: bench.py's workload (default: the
configs[3] per-GPU shard, 125M records against 1M intervals), device-resident,
analysed once; then, with 8 nodes, the NULL thread map and threshold 8,
  (a) nmg_count_object_blocks + nmg_get_object_blocks: fold, blocks, scan and
      emit on the device, only the block rows cross PCIe;
  (b) what a caller does without it for the same rows: nmg_count_page_cells +
      nmg_get_page_cells (every non-zero cell crosses PCIe), then the rule on
      the host (nmg_report_placement_host's computation over the objects).
Both are cached per results epoch, so before every run the epoch is bumped by
importing the engine's own sum64 array unchanged (a device copy, not timed).
One warm-up and 5 timed runs each; a run that exceeds --limit seconds ends the
process (exit status 124).  The timed work reads nothing but the engine.
--huge also times (c), (a) with NMG_PLACE_HUGE: every entry contributes, the
sparse ones through the sparse table; --hist-budget-bytes / --sparse-capacity
give the engine a page-histogram budget that leaves a share of the entries
sparse (the default budget leaves [stack] alone).  --sets N repeats (a)'s
warm-up and runs N times: the spread between sets of unchanged code.
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c4")
    ap.add_argument("--nodes", type=int, default=8)
    ap.add_argument("--threshold", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds a single run may take")
    ap.add_argument("--huge", action="store_true", help="also time the object blocks with NMG_PLACE_HUGE")
    ap.add_argument("--hist-budget-bytes", type=int, default=0, help="nmg_options.hist_budget_bytes (0: the default)")
    ap.add_argument("--sparse-capacity", type=int, default=0, help="nmg_options.sparse_capacity (0: the default)")
    ap.add_argument("--sets", type=int, default=1, help="how often (a) is measured (warm-up + runs each)")
    ap.add_argument("--skip-host", action="store_true", help="leave out (b)")
    args = ap.parse_args()

    import numpy as np
    import torch

    import bench  # (the generator and the device-resident engine setup: bench.Workload)
    from numamma_amd import _lib
    import numamma_amd.engine as engine_mod

    if args.hist_budget_bytes or args.sparse_capacity:  # (bench.Workload builds its engine with the defaults)
        class BudgetedEngine(engine_mod.Engine):
            def __init__(self, *a, **kw):
                kw.setdefault("hist_budget_bytes", args.hist_budget_bytes)
                kw.setdefault("sparse_capacity", args.sparse_capacity)
                super().__init__(*a, **kw)

        engine_mod.Engine = BudgetedEngine

    w = bench.Workload(args.workload, 0, torch.device("cuda", 0), False)
    eng, rp = w.eng, w.rp
    eng.reset()
    eng.analyze()
    eng.synchronize()
    scratch = torch.empty(eng.array_size(_lib.NMG_ARR_SUM64), dtype=torch.int64, device="cuda")

    def bump():  # a new results epoch over the same counters
        eng.export_array(_lib.NMG_ARR_SUM64, scratch.data_ptr())
        eng.import_array(_lib.NMG_ARR_SUM64, scratch.data_ptr())
        eng.synchronize()

    def limited(fn):
        guard = threading.Timer(args.limit, lambda: os._exit(124))
        guard.daemon = True
        guard.start()
        try:
            t0 = time.perf_counter()
            out = fn()
            return (time.perf_counter() - t0) * 1e3, out
        finally:
            guard.cancel()

    def timed(fn):
        ms = []
        for i in range(args.runs + 1):  # (the first is the warm-up)
            bump()
            t, out = limited(fn)
            ms.append(t)
        return {"warmup_ms": ms[0], "ms": ms[1:], "median_ms": statistics.median(ms[1:])}, out

    T = rp.nb_threads
    po, keep = _lib.placement_options(T, args.nodes, None, args.threshold)

    def device_path():
        return eng.object_blocks(args.nodes, None, args.threshold)

    def device_path_huge():
        return eng.object_blocks(args.nodes, None, args.threshold, source=_lib.NMG_PLACE_HUGE)

    sizes = np.ascontiguousarray(rp.table.entries["buffer_size"], dtype=np.uint64)
    cap = [0]

    def host_path():
        cells = eng.page_cells()
        hr = _lib.nmg_host_results()
        hr.nb_entries = rp.table.nb_entries
        hr.buffer_size = sizes.ctypes.data_as(C.POINTER(C.c_uint64))
        hr.cells = cells.ctypes.data_as(C.POINTER(C.c_uint32))
        hr.nb_cells = cells.shape[0]
        hr.nb_threads = T
        rows = np.empty((cap[0], 5), dtype=np.uint64)
        n = _lib.check(_lib.lib.nmg_debug_object_blocks_host(C.byref(hr), C.byref(po),
                                                             rows.ctypes.data_as(C.POINTER(C.c_uint64)), cap[0]))
        assert n <= cap[0]
        return rows[:n], cells.shape[0]

    sets = []
    for _ in range(max(1, args.sets)):
        a, rows_a = timed(device_path)
        sets.append(a["median_ms"])
    huge = None
    if args.huge:
        c, rows_c = timed(device_path_huge)
        nsparse = int(eng.sparse_export()[0].shape[0])
        po, keep = _lib.placement_options(T, args.nodes, None, args.threshold, source=_lib.NMG_PLACE_HUGE)
        cap[0] = rows_c.shape[0] + 1
        _, (rows_h, ncells) = limited(host_path)  # (the host rule with the flag: the rows to compare with)
        huge = dict(c, rows=int(rows_c.shape[0]), bytes_d2h=int(rows_c.nbytes), sparse_cells=nsparse, cells=int(ncells),
                    rows_equal_host=bool(rows_c.shape == rows_h.shape and np.array_equal(rows_c, rows_h)))
        po, keep = _lib.placement_options(T, args.nodes, None, args.threshold)
    cap[0] = rows_a.shape[0] + 1
    if args.skip_host:
        b, rows_b, ncells = {}, rows_a, 0
    else:
        b, (rows_b, ncells) = timed(host_path)
    ent = rp.table.entries
    pages = ent["buffer_size"].astype(np.uint64) // np.uint64(4096) + np.uint64(1)
    dense = pages * np.uint64(T) <= np.uint64(1 << 24)
    out = {
        "tool": "placement_timing", "workload": args.workload, "records": w.samples,
        "box": {"gpu": getattr(torch.cuda.get_device_properties(0), "gcnArchName", torch.cuda.get_device_name(0)).split(":")[0], "date": time.strftime("%Y-%m-%d")},
        "nb_nodes": args.nodes, "density_threshold": args.threshold, "nb_threads": T,
        "entries": int(rp.table.nb_entries), "dense_entries": int(dense.sum()), "group_pages": int(pages[dense].sum()),
        "largest_object_pages": int(pages[dense].max()),
        "nb_found": int(eng.global_counters()[2]),
        "a_object_blocks": dict(a, rows=int(rows_a.shape[0]), bytes_d2h=int(rows_a.nbytes),
                                bytes_h2d_per_call=4 * (T + args.nodes + 1),
                                bytes_h2d_once_per_table=int(dense.sum()) * 28 + 12),
        "b_page_cells_then_host_rule": dict(b, rows=int(rows_b.shape[0]), cells=int(ncells), bytes_d2h=int(ncells) * 16),
        "rows_equal": bool(rows_a.shape == rows_b.shape and np.array_equal(rows_a, rows_b)),
        "a_set_medians_ms": sets,
        "hist_budget_bytes": args.hist_budget_bytes, "sparse_capacity": args.sparse_capacity,
    }
    if huge is not None:
        out["c_object_blocks_huge"] = huge
        # the entries the budget leaves dense (CellCursor::place in id order)
        budget_cells = (args.hist_budget_bytes or 4 << 30) // 4
        used, nd = 0, 0
        for n, ok in zip(pages.tolist(), dense.tolist()):
            if ok and (used + n) * T <= budget_cells:
                used += n
                nd += 1
        huge["dense_entries_in_budget"] = nd
        huge["sparse_entries"] = int(rp.table.nb_entries) - nd
    del keep
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
