#!/usr/bin/env python3
"""Host time of the synchronous calls that read the sparse page table:
page_cells(), sparse_export() and, with set_page_cost(scope = all), cost_cells()
-- each a count and a get that end in a wait or a blocking copy, timed with the
host clock on a fresh results epoch (reset, analyze, synchronize before each
round).  Three replays:

  k60k        tests/test_gpu_results.py's k60k with the default budget: every
              entry fits the budget, so all rows are dense and the sparse
              table stays untouched (sparse_nonempty's short cut)
  k60k_mixed  the same with hist_budget_bytes = 64 MiB: dense and sparse rows
  all_sparse  tests/test_gpu_parity.py::test_sparse_histogram_path's replay
              with hist_budget_bytes = 4: every row a sparse one

Prints one JSON line with every raw timing (the first round of each replay is
the warm-up and is listed apart).  For an A/B of two builds of the library run
it once per build and round, alternated, with NMG_LIB_PATH (tools/ab_build.sh)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()

    from numamma_amd import _lib
    from numamma_amd.engine import Engine
    from numamma_amd.replay import SynthConfig, generate

    cases = {
        "k60k": (dict(nb_samples=300_000, nb_intervals=60_000, size_max=4 << 20, seed=22), {}),
        "k60k_mixed": (dict(nb_samples=300_000, nb_intervals=60_000, size_max=4 << 20, seed=22),
                       dict(hist_budget_bytes=64 << 20)),
        "all_sparse": (dict(nb_samples=100_000, nb_intervals=400, seed=9),
                       dict(hist_budget_bytes=4, sparse_capacity=1 << 16)),
    }
    out = {"tool": "sparse_words_timing", "tag": a.tag, "library": os.path.relpath(_lib.LIB_PATH, ROOT),
           "rounds": a.rounds, "replays": {}}
    for name, (cfg, kw) in cases.items():
        rp = generate(SynthConfig(**cfg))
        eng = Engine(nb_threads=rp.nb_threads, **kw)
        eng.set_objects(rp.table)
        eng.set_page_cost(budget_bytes=64 << 30, scope=_lib.NMG_COST_SCOPE_ALL)
        eng.submit_replay(rp)
        calls = {"page_cells": eng.page_cells, "sparse_export": lambda: eng.sparse_export()[0],
                 "cost_cells": eng.cost_cells}
        ms = {c: [] for c in calls}
        rows = {}
        for _ in range(a.rounds + 1):
            eng.reset()
            eng.analyze()
            eng.synchronize()
            for c, f in calls.items():
                t0 = time.perf_counter()
                r = f()
                ms[c].append((time.perf_counter() - t0) * 1e3)
                rows[c] = int(r.shape[0])
        out["replays"][name] = {"rows": rows, "warmup_ms": {c: v[0] for c, v in ms.items()},
                                "ms": {c: v[1:] for c, v in ms.items()}}
        eng.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
