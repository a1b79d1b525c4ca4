#!/usr/bin/env python3
"""Host time of the calls that build and upload an object table's lookup
structures (numamma_amd/csrc/nmg_table_build.h): Engine.set_objects of the
benchmark's 1M-interval table (bench.py's default workload, table only), and
Engine.update_objects of the same table with ids in creation order, as
tools/online_timing.py builds it, on an engine that holds the empty table.
Each call ends with the table uploaded (the engine synchronises its stream),
timed with the host clock.

Prints one JSON line with every raw timing (the first round is the warm-up and
is listed apart).  For an A/B of two builds of the library run it once per
build and round, alternated, with NMG_LIB_PATH (tools/ab_build.sh)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--intervals", type=int, default=1_000_000)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()

    from numamma_amd import _lib
    from numamma_amd.engine import Engine, table_objects
    from numamma_amd.replay import ObjectTable, SynthConfig, make_table

    cfg = SynthConfig(seed=1, nb_samples=0, nb_intervals=a.intervals, size_max=64 * 1024)
    t = make_table(cfg, np.random.default_rng(cfg.seed))
    objs = table_objects(t)
    order = np.lexsort((np.arange(t.nb_entries), t.entries["alloc_date"]))
    cid = np.empty(t.nb_entries, dtype=np.uint32)
    cid[order] = np.arange(t.nb_entries, dtype=np.uint32)
    ms = {"set_objects": [], "update_objects": []}
    eng = Engine(nb_threads=cfg.nb_threads)
    for _ in range(a.rounds + 1):
        t0 = time.perf_counter()
        eng.set_objects(t)
        ms["set_objects"].append((time.perf_counter() - t0) * 1e3)
        eng.set_objects(ObjectTable.empty())
        t0 = time.perf_counter()
        eng.update_objects(t.keys, t.entry_off, cid, objs)
        ms["update_objects"].append((time.perf_counter() - t0) * 1e3)
    eng.close()
    print(json.dumps({"tool": "table_timing", "tag": a.tag, "library": os.path.relpath(_lib.LIB_PATH, ROOT),
                      "keys": t.nb_keys, "entries": t.nb_entries, "rounds": a.rounds,
                      "warmup_ms": {c: v[0] for c, v in ms.items()}, "ms": {c: v[1:] for c, v in ms.items()}}),
          flush=True)


if __name__ == "__main__":
    main()
