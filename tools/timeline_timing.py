#!/usr/bin/env python3
"""What the access timeline (nmg_set_timeline) costs on a large table:
bench.py's workload (default: the configs[3] per-GPU shard, 125M records
against 1M intervals), device-resident, analysed in warmed-up
`reset(); analyze()` steps; the times are the engine's own launch events
(nmg_get_kernel_times, and the first-kernel / rest split of
nmg_debug_phase_times) plus the host's wall time per step, which also holds
the reset (with a timeline: the memset of its cells).  Prints one JSON line.

One process and one generated batch serve every variant, so they are timed on
one box by construction:
  plain      NMG_F_DEFAULT, no timeline (the benchmark's step)
  levels     NMG_F_DEFAULT | NMG_F_OBJECT_LEVELS, no timeline (DESIGN 7.0r7's 31 ms)
  tl_r<N>    NMG_F_DEFAULT with the timeline, timeline_add merging for at most
             N rounds (NMG_TL_ROUNDS; 0: one atomic per record)
  one_r<N>   (--one-cell) the same with one bin and one row per object: every
             record of a hot object and thread on one word
The timeline: min_object_bytes 4096, row_shift 0, 64 bins of 2^28 ns from the
generator's first timestamp on (its 10 s horizon ends in bin 37).
--scope all sets it with NMG_TL_SCOPE_ALL (nmg_set_timeline_ex): at the
configs[3] shard no record matches a sparse entry, so the difference to the
dense scope is the price of the kernels' checks alone.
NMG_LIB_PATH picks another build of the library (with NMG_LIB_AB=1 an older
one); one that predates the timeline runs `plain` and `levels` only
(--no-timeline), one that predates the scope the dense scope only."""
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
    ap.add_argument("--rounds", default="0,4,16", help="merge-round bounds to time")
    ap.add_argument("--one-cell", action="store_true",
                    help="also time a timeline of one bin and one row per object (the hottest cells the data can give)")
    ap.add_argument("--no-timeline", action="store_true", help="the yardsticks only (a library without the timeline)")
    ap.add_argument("--scope", choices=["dense", "all"], default="dense",
                    help="all: NMG_TL_SCOPE_ALL (nmg_set_timeline_ex) -- the sparse entries selected too, their cells in "
                         "the timeline sparse table; needs a library that has it")
    args = ap.parse_args()
    if not 1 <= args.steps <= 64:
        ap.error("--steps: 1 to 64 (the engine keeps the events of its last 64 launches)")

    import numpy as np
    import torch

    import bench  # (the generator and the device-resident engine setup: bench.Workload)
    from numamma_amd import _lib
    from numamma_amd.engine import Engine
    from numamma_amd.replay import T0

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

    out = {"tool": "timeline_timing", "workload": args.workload, "records": w.samples, "steps": args.steps,
           "warmup": args.warmup, "scope": args.scope, "library": os.path.relpath(_lib.LIB_PATH, ROOT), "variants": {}}
    out["variants"]["plain"] = timed(w.eng)
    w.eng.close()
    eng = engine(_lib.NMG_F_DEFAULT | _lib.NMG_F_OBJECT_LEVELS)
    out["variants"]["levels"] = timed(eng)
    eng.close()
    if not args.no_timeline:
        tls = {"tl": dict(t0=T0, bin_shift=28, nb_bins=64, row_shift=0, min_object_bytes=4096, budget_bytes=16 << 30)}
        if args.one_cell:  # one cell per object and thread: every record of a hot object on one word
            tls["one"] = dict(t0=T0, bin_shift=63, nb_bins=1, row_shift=20, min_object_bytes=4096)
        out["timelines"] = tls
        for name, tl in tls.items():
            for r in [int(x) for x in args.rounds.split(",")]:
                os.environ["NMG_TL_ROUNDS"] = str(r)  # (read when the timeline is set)
                eng = engine(_lib.NMG_F_DEFAULT)
                if args.scope == "all":
                    eng.set_timeline(**tl, scope=_lib.NMG_TL_SCOPE_ALL)
                else:
                    eng.set_timeline(**tl)
                res = timed(eng)
                rows = eng.timeline_cells()
                mul = np.array([3, 5, 7, 11, 13], dtype="uint64")
                res.update(rows=int(rows.shape[0]), count_sum=int(rows[:, 4].sum(dtype="uint64")),
                           max_cell=int(rows[:, 4].max()) if rows.shape[0] else 0,
                           checksum=int((rows.astype("uint64") * mul).sum(dtype="uint64")))
                out["variants"][f"{name}_r{r}"] = res
                eng.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
