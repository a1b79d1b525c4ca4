"""The table builders on the CPU.

numamma_amd/csrc/nmg_table_build.h holds the formats of everything the kernels
read of an object table -- the small table's Eytzinger tree, the fences and
bucket directory of a large one, the route pass's segments, and the
partition-first path's partitions, node records, PartDir slots, older-entry
lists, dead bits and packed cell maps -- and the builders that make them; it
needs no HIP and no engine.  tests/c/nmg_table_build_host.cpp checks every
array against a direct restatement of that header's format comments, and every
built lookup against a host restatement of the device's read sequence
(lower_key, route_partition_l, the local pass's slot read), which must return
upper_bound - 1 for every key, key +- 1, 0, ~0 and the midpoint of every gap:

  trees       K = 0, 1, 2, 1022, 1023 (elevels, the ~0 padding carrying the
              last node);
  fences      K = 1024, 4095 (one key per fence, no directory); 4096, 8190
              (fence_log2 1, two slots per key); 8191, where two keys per
              fence would need 4096 fences, one more than kMaxFences, so
              fence_log2 is 2; 20000 (fence_log2 3); no_dir; a bucket whose
              span needs a shift above 32 (kShiftSearch).  Buckets more than
              2^16 keys wide need 2.7e8 keys and stay unexercised;
  segments    P = 1; P = 2 across 2^45; twelve clusters whose largest seven
              gaps cut; a slot that saturates; starts up to ~0 - 1;
  the cut     1023 + 1 keys; kPartEntries (768 keys of two entries; a key of
              1536 entries alone, of 1537: no path); 2^39 from the first key
              (and 8 bytes less); kPartCells with T = 2, and one key alone past
              it; 2047 and 2048 partitions; ids as the identity, as a
              permutation (cmap / lrel, a sparse entry), 2^31 dense cells;
  records     an object above 4 GiB, an entry freed before tbase, saturated
              dates, a three-entry key's older list, a key whose older entries
              would end past kOldLds, dead partitions, tbase with and without
              an allocation date.

The program is also given, in a file, the three tables tests/local_lane_cases.py
crafts its record streams for; the second test requires the partitions and
every PartDir slot it prints for them to equal that module's restatement
(partitions, dshift_of, dir_slot), which the GPU tests rely on.

Compiled once for both tests, with g++ as tests/test_layout_host.py compiles
its programs: under the address and undefined-behaviour sanitizers where the
compiler has them, linked statically.
"""
import os

import numpy as np
import pytest

import local_lane_cases as lc
from test_layout_host import SAN, _build_and_run

NAME = "nmg_table_build_host"


def _tables():
    rp = lc.base(lc.DENSE_CFG)
    return [rp.table, lc.base(lc.WIDE_CFG).table, lc.lone_key_table(rp.table)]


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    """The program compiled and run once, on its own cases and on the tables of local_lane_cases."""
    d = str(tmp_path_factory.mktemp("table_build"))
    path = os.path.join(d, "tables.bin")
    with open(path, "wb") as f:
        tables = _tables()
        f.write(np.uint32(len(tables)).tobytes())
        for t in tables:
            ent = t.entries
            f.write(np.array([t.nb_keys, t.nb_entries], dtype=np.uint32).tobytes())
            f.write(t.keys.astype(np.uint64).tobytes())
            f.write(t.entry_off.astype(np.uint32).tobytes())
            f.write(np.stack([ent[n].astype(np.uint64) for n in ("buffer_addr", "buffer_size", "alloc_date", "free_date")],
                             axis=1).tobytes())
    out, err = _build_and_run(NAME, d, SAN, [path])
    if out is None:  # a compiler without the sanitizer runtimes: the same checks, plain
        out, err = _build_and_run(NAME, d, args=[path])
    assert out is not None, err
    return out


def test_table_build(output):
    assert NAME + ": ok" in output


def test_partitions_match_python_restatement(output):
    tables = _tables()
    got_parts = [[] for _ in tables]
    got_slots = [{} for _ in tables]
    for line in output.splitlines():
        w = line.split()
        if w[0] == "part":
            ti, q, k0, nk, dshift = map(int, w[1:])
            assert q == len(got_parts[ti])
            got_parts[ti].append((k0, nk, dshift))
        elif w[0] == "slot":
            ti, q, j, lo, n, inl = map(int, w[1:])
            got_slots[ti][q, j] = (lo, n, bool(inl))
    for ti, t in enumerate(tables):
        parts = lc.partitions(t, 2)
        assert got_parts[ti] == [(k0, nk, lc.dshift_of(t, (k0, nk))) for k0, nk in parts]
        assert len(got_slots[ti]) == len(parts) * lc.PART_DIR
        for q, part in enumerate(parts):
            for j in range(lc.PART_DIR):
                assert got_slots[ti][q, j] == lc.dir_slot(t, part, j), (ti, q, j)
