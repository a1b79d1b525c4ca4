#!/usr/bin/env python3
"""What the page cost cells (nmg_set_page_cost) cost on a large table:
bench.py's workload (default: the configs[3] per-GPU shard, 125M records
against 1M intervals), device-resident, analysed in warmed-up
`reset(); analyze()` steps; the times are the engine's own launch events
(nmg_get_kernel_times, and the first-kernel / rest split of
nmg_debug_phase_times) plus the host's wall time per step, which also holds
the reset (with cost cells: the memset of the u64 array).  Prints one JSON
line.

One process and one generated batch serve every variant, so they are timed on
one box by construction:
  plain       NMG_F_DEFAULT, no cost cells (the benchmark's step)
  memw_r<N>   (NMG_COST_MEMORY, both accesses, NMG_COST_WEIGHT), cost_add
              merging for at most N rounds (NMG_COST_ROUNDS; 0: one atomic per
              selected record)
  allc_r<N>   (every bucket | NMG_COST_NA, both accesses, NMG_COST_COUNT): every
              record with a non-zero level adds
--scopes 0,1 times each of them with nmg_set_page_cost (scope 0,
NMG_COST_SCOPE_DENSE) and with nmg_set_page_cost_ex(NMG_COST_SCOPE_ALL) (scope
1: the sparse entries, [stack] among them, get cost cells too; the variant's
name then ends in _all).
A checksum of the rows must be equal across the round settings of a variant
(the tool fails otherwise).  Then one line in placement_timing.py's style:
nmg_get_object_blocks from the cost cells against from the counts, median of
--runs calls, each on a fresh results epoch."""
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", default="0,1,4,64", help="merge-round bounds to time")
    ap.add_argument("--scopes", default="0", help="cost scopes to time: 0 dense, 1 all (comma-separated)")
    ap.add_argument("--nodes", type=int, default=8)
    ap.add_argument("--threshold", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    if not 1 <= args.steps <= 64:
        ap.error("--steps: 1 to 64 (the engine keeps the events of its last 64 launches)")

    import numpy as np
    import torch

    import bench  # (the generator and the device-resident engine setup: bench.Workload)
    from numamma_amd import _lib
    from numamma_amd.engine import Engine

    w = bench.Workload(args.workload, 0, torch.device("cuda", 0), False)
    rp = w.rp
    _, offs, lens, ranks, acc = rp.packed()

    def stats(v):
        return {"median": statistics.median(v), "min": min(v), "max": max(v)}

    def timed(eng):
        for _ in range(args.warmup):
            eng.reset()
            eng.analyze()
        eng.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            eng.reset()
            eng.analyze()
        eng.synchronize()
        wall = (time.perf_counter() - t0) * 1e3 / args.steps
        attr, total = eng.kernel_times(args.steps)
        first, rest = eng.phase_times(args.steps)
        return {"step_ms": stats(total), "first_kernel_ms": stats(first), "rest_ms": stats(rest),
                "wall_ms_per_step": wall, "route_launches": eng.route_count(),
                "nb_found": int(eng.global_counters()[2])}

    def engine(flags):
        eng = Engine(device=0, flags=flags, nb_threads=rp.nb_threads)
        eng.set_objects(rp.table)
        eng.set_device_buffers(w.d_arena.data_ptr(), offs, lens, ranks, acc)
        return eng

    out = {"tool": "cost_timing", "workload": args.workload, "records": w.samples, "steps": args.steps,
           "warmup": args.warmup, "library": os.path.relpath(_lib.LIB_PATH, ROOT),
           "box": {"gpu": getattr(torch.cuda.get_device_properties(0), "gcnArchName",
                                  torch.cuda.get_device_name(0)).split(":")[0], "date": time.strftime("%Y-%m-%d")},
           "variants": {}}
    out["variants"]["plain"] = timed(w.eng)
    w.eng.close()
    costs = {"memw": dict(bucket_mask=_lib.NMG_COST_MEMORY, access_mask=3, metric=_lib.NMG_COST_WEIGHT),
             "allc": dict(bucket_mask=((1 << 18) - 1) | _lib.NMG_COST_NA, access_mask=3, metric=_lib.NMG_COST_COUNT)}
    out["costs"] = costs
    mul = np.array([3, 5, 7, 11], dtype="uint64")
    for name, opt, scope in [(n + ("_all" if int(sc) else ""), o, int(sc)) for sc in args.scopes.split(",")
                             for n, o in costs.items()]:
        sums = set()
        for r in [int(x) for x in args.rounds.split(",")]:
            os.environ["NMG_COST_ROUNDS"] = str(r)  # (read when the cells are set)
            eng = engine(_lib.NMG_F_DEFAULT)
            eng.set_page_cost(**opt, scope=scope)
            res = timed(eng)
            if scope:
                res["sparse_cells"] = int(eng.sparse_export()[0].shape[0])
            rows = eng.cost_cells()
            res.update(rows=int(rows.shape[0]), value_sum=int(rows[:, 3].sum(dtype="uint64")),
                       max_cell=int(rows[:, 3].max()) if rows.shape[0] else 0,
                       checksum=int((rows * mul).sum(dtype="uint64")))
            sums.add(res["checksum"])
            out["variants"][f"{name}_r{r}"] = res
            eng.close()
        if len(sums) != 1:
            print(json.dumps(out), flush=True)
            sys.exit(f"{name}: the rows differ between the merge-round settings")
    os.environ.pop("NMG_COST_ROUNDS", None)

    # object blocks from the cost cells against from the counts
    eng = engine(_lib.NMG_F_DEFAULT)
    eng.set_page_cost(**costs["memw"])
    eng.reset()
    eng.analyze()
    eng.synchronize()
    scratch = torch.empty(eng.array_size(_lib.NMG_ARR_SUM64), dtype=torch.int64, device="cuda")

    def bump():  # a new results epoch over the same counters
        eng.export_array(_lib.NMG_ARR_SUM64, scratch.data_ptr())
        eng.import_array(_lib.NMG_ARR_SUM64, scratch.data_ptr())
        eng.synchronize()

    place = {}
    for name, source in (("counts", _lib.NMG_PLACE_PAGE_COUNTS), ("cost", _lib.NMG_PLACE_PAGE_COST)):
        ms = []
        for _ in range(args.runs + 1):  # (the first is the warm-up)
            bump()
            t0 = time.perf_counter()
            rows = eng.object_blocks(args.nodes, None, args.threshold, source=source)
            ms.append((time.perf_counter() - t0) * 1e3)
        place[name] = {"warmup_ms": ms[0], "ms": ms[1:], "median_ms": statistics.median(ms[1:]),
                       "rows": int(rows.shape[0]), "count_sum": int(rows[:, 4].sum(dtype="uint64"))}
    out["placement"] = dict(place, nb_nodes=args.nodes, density_threshold=args.threshold, cost_options="memw")
    eng.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
