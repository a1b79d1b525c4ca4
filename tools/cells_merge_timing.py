#!/usr/bin/env python3
"""What the packed merge of the page cost cells and the timeline cells costs
on one engine: bench.py's workload (default: the configs[3] per-GPU shard),
device-resident, analysed once with the cost cells of tools/cost_timing.py
(NMG_COST_MEMORY, both accesses, NMG_COST_WEIGHT) and the timeline of
tools/timeline_timing.py (64 bins of 2^28 ns, objects >= 4 KiB).  Per array
(NMG_ARR_COST64, NMG_ARR_TL32), warmed, the median of --runs calls of

  pack     nmg_cells_pack into a list buffer that holds the whole list
  unpack   nmg_cells_unpack_add of that list (the cells grow by themselves:
           the time does not depend on the values)
  dense    nmg_export_array then nmg_import_array of the same array

each between two device events and under a host clock; every call ends in
the engine's own stream synchronise, so both see the whole call.  At the end
the list is checked to rebuild the array on its own: reset, unpack, and the
export must equal the one taken before (round_trip_equal).  Prints one JSON
line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c4")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch

    import bench  # (the generator and the device-resident engine setup: bench.Workload)
    from numamma_amd import _lib
    from numamma_amd.replay import T0

    if not torch.cuda.is_available():
        sys.exit("cells_merge_timing: no GPU")
    dev = torch.device("cuda", 0)
    w = bench.Workload(args.workload, 0, dev, False)
    eng = w.eng
    eng.set_page_cost(bucket_mask=_lib.NMG_COST_MEMORY, access_mask=3, metric=_lib.NMG_COST_WEIGHT)
    eng.set_timeline(t0=T0, bin_shift=28, nb_bins=64, row_shift=0, min_object_bytes=4096, budget_bytes=16 << 30)
    eng.reset()
    eng.analyze()
    eng.synchronize()

    def timed(fn):
        ev, host = [], []
        for i in range(args.warmup + args.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            t1 = time.perf_counter()
            if i >= args.warmup:
                ev.append(e0.elapsed_time(e1))
                host.append((t1 - t0) * 1e3)
        return {"event_ms": {"median": statistics.median(ev), "min": min(ev), "max": max(ev)},
                "host_ms": {"median": statistics.median(host), "min": min(host), "max": max(host)}}

    out = {"workload": args.workload, "records": w.samples, "runs": args.runs, "warmup": args.warmup, "arrays": {}}
    for name, which, dt, width in (("NMG_ARR_COST64", _lib.NMG_ARR_COST64, torch.int64, 8),
                                   ("NMG_ARR_TL32", _lib.NMG_ARR_TL32, torch.int32, 4)):
        cells = eng.array_size(which)
        n = eng.cells_pack(which, 0, 0)
        lst = torch.empty(2 * max(n, 1), dtype=torch.int64, device=dev)
        dense = torch.empty(cells, dtype=dt, device=dev)
        torch.cuda.synchronize(dev)
        r = {"cells": cells, "dense_bytes": cells * width, "nonzero": n, "list_bytes": 16 * n}
        r["pack"] = timed(lambda: eng.cells_pack(which, lst.data_ptr(), n))
        r["dense_export_import"] = timed(lambda: (eng.export_array(which, dense.data_ptr()),
                                                  eng.import_array(which, dense.data_ptr())))
        r["unpack_add"] = timed(lambda: eng.cells_unpack_add(which, lst.data_ptr(), n))
        # the list still describes the analysis' cells: after a reset it alone rebuilds them
        eng.reset()
        eng.cells_unpack_add(which, lst.data_ptr(), n)
        after = torch.empty(cells, dtype=dt, device=dev)
        eng.export_array(which, after.data_ptr())
        r["round_trip_equal"] = bool(torch.equal(after, dense))
        out["arrays"][name] = r
        del lst, dense, after
        eng.reset()
        eng.analyze()
        eng.synchronize()
    print(json.dumps(out))
    if not all(a["round_trip_equal"] for a in out["arrays"].values()):
        sys.exit("cells_merge_timing: a packed list did not rebuild its array")


if __name__ == "__main__":
    main()
