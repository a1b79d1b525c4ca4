#!/usr/bin/env python3
"""What per-object level counters (NMG_F_OBJECT_LEVELS) cost on a large table:
bench.py's workload (default: the configs[3] per-GPU shard, 125M records
against 1M intervals), device-resident, analysed with NMG_F_DEFAULT |
NMG_F_OBJECT_LEVELS in warmed-up `reset(); analyze()` steps; the times are the
engine's own launch events (nmg_get_kernel_times, and the first-kernel / rest
split of nmg_debug_phase_times).  Prints one JSON line.

The script uses nothing a tree without levels on the partition-first path
lacks, so the same file times both sides of that change (NMG_LIB_PATH picks
another build of the library): `route_launches` tells which path ran, and
`levels_checksum` that both computed the same rows.  --single-pass forces
attribute_kernel (NMG_F_SINGLE_PASS) inside one build."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c4")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--single-pass", action="store_true")
    ap.add_argument("--no-levels", action="store_true", help="NMG_F_DEFAULT alone (the benchmark's flags)")
    args = ap.parse_args()
    if not 1 <= args.steps <= 64:
        ap.error("--steps: 1 to 64 (the engine keeps the events of its last 64 launches)")

    import torch

    import bench  # (the generator and the device-resident engine setup: bench.Workload)
    from numamma_amd import _lib

    flags = (0 if args.no_levels else _lib.NMG_F_OBJECT_LEVELS) | (_lib.NMG_F_SINGLE_PASS if args.single_pass else 0)
    # bench.Workload ORs these bits into NMG_F_DEFAULT
    os.environ["NMG_BENCH_DEBUG_FLAGS"] = hex(flags)
    w = bench.Workload(args.workload, 0, torch.device("cuda", 0), False)
    eng = w.eng
    for _ in range(args.warmup):
        w.step()
    eng.synchronize()
    for _ in range(args.steps):
        w.step()
    eng.synchronize()
    attr, total = eng.kernel_times(args.steps)
    first, rest = eng.phase_times(args.steps)

    def stats(v):
        return {"median": statistics.median(v), "min": min(v), "max": max(v)}

    out = {
        "tool": "levels_timing", "workload": args.workload, "records": w.samples, "flags": hex(_lib.NMG_F_DEFAULT | flags),
        "steps": args.steps, "warmup": args.warmup, "library": os.path.relpath(_lib.LIB_PATH, ROOT),
        "route_launches": eng.route_count(),  # 0: every step ran attribute_kernel
        "step_ms": stats(total),              # first to last event of a step's analysis
        "attribution_ms": stats(attr),
        "first_kernel_ms": stats(first),      # route2_kernel, or attribute_kernel
        "rest_ms": stats(rest),               # overflow, count, plan, scatter, local_kernel (0: single pass)
        "nb_found": int(eng.global_counters()[2]),
    }
    if not args.no_levels:
        out["levels_checksum"] = int(eng.object_levels().sum(dtype="uint64"))
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
