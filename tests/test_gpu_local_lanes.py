"""local_kernel's paired common path against the oracle, on the replays of
local_lane_cases.py (their shapes: test_local_lanes_host.py).

local_kernel reads LDS for both chunks of a pair with in-range indices before
it decides either -- the list word, the directory slot, the keys of the
search, the node and info records, the first-match word -- so a lane without
a record reads element 0 and must add nothing:

* stale slots: a second, shorter analysis on one engine, whose partly filled
  chunks lie over the first one's records;
* fills and list ends: partitions of 1, 63, 64, 65, 127, 128, 129 records (a
  one-chunk item, an odd chunk count, a pair whose second chunk is past the
  list);
* directory shapes: a partition of one key, a slot with more than six keys
  next to slots without a search, a slot that is not inline;
* rare records (escaped, older entries, no match) in one chunk of a pair only;
* the same on the EXTRA instance (NMG_F_OBJECT_LEVELS) and on an online
  table (the PACKED instance).

Every run asserts route_count() > 0, that the engine's partition starts
(route_parts) are those of local_lane_cases.partitions, and equals the
oracle's raw dump."""
import os

import numpy as np
import pytest

import cost_expect as cx
import local_lane_cases as lc
import pyoracle
from numamma_amd import _lib
from numamma_amd.replay import ObjectTable
from numamma_amd.results import RawResults

pytestmark = pytest.mark.gpu

DEFAULT = _lib.NMG_F_DEFAULT
LEVELS = _lib.NMG_F_DEFAULT | _lib.NMG_F_OBJECT_LEVELS


@pytest.fixture(scope="module")
def oracle_of(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("lanes"))
    seen = {}

    def get(tag, rp):
        if tag not in seen:
            path = os.path.join(d, f"{tag}.bin")
            rp.write(path)
            pyoracle.run(path, os.path.join(d, f"{tag}_o"), os.path.join(d, f"{tag}.txt"),
                         os.path.join(d, f"{tag}_raw.bin"))
            os.remove(path)
            seen[tag] = RawResults.read(os.path.join(d, f"{tag}_raw.bin"))
        return seen[tag]
    return get


def _check(eng, raw, levels, idmap=None):
    g, ns, nf = eng.global_counters()
    assert np.array_equal(g, raw.global_counters) and (ns, nf) == (raw.nb_samples, raw.nb_found)
    s, f = eng.buffer_counts()
    assert np.array_equal(s, raw.buf_samples) and np.array_equal(f, raw.buf_found)
    first, cw = eng.object_counters()
    lv = eng.object_levels() if levels else None
    cells = eng.page_cells().copy()
    if idmap is not None:  # (an online table: the engine's entry id of each table position)
        first, cw = first[idmap], cw[idmap]
        lv = lv[idmap] if levels else None
        pos = np.empty_like(idmap)
        pos[idmap] = np.arange(idmap.shape[0], dtype=np.uint32)
        cells[:, 0] = pos[cells[:, 0]]
        cells = cells[np.lexsort((cells[:, 2], cells[:, 1], cells[:, 0]))]
    assert np.array_equal(first, raw.first_ordinal)
    assert np.array_equal(cw, raw.count_weight)
    if levels:
        assert np.array_equal(lv, cx.oracle_levels(raw))
    assert np.array_equal(cells, raw.cells)


def _creation_ids(table):
    ent = table.entries
    order = np.lexsort((np.arange(table.nb_entries), ent["alloc_date"]))
    cid = np.empty(table.nb_entries, dtype=np.uint32)
    cid[order] = np.arange(table.nb_entries, dtype=np.uint32)
    assert not np.array_equal(cid, np.arange(table.nb_entries))
    return cid


class Runner:
    """One engine over one table: 'default' and 'levels' set the table once
    (nmg_set_objects); 'online' starts empty and brings the table with ids in
    creation order at the start of every streamed analysis (nmg_update_objects)."""

    def __init__(self, table, T, mode):
        from numamma_amd.engine import Engine

        self.mode, self.table = mode, table
        self.levels = mode != "default"
        self.eng = Engine(flags=LEVELS if self.levels else DEFAULT, nb_threads=T)
        self.cid = _creation_ids(table) if mode == "online" else None
        self.eng.set_objects(ObjectTable.empty() if mode == "online" else table)
        self.routes = 0

    def run(self, rp, raw):
        from numamma_amd.engine import table_objects

        eng = self.eng
        if self.mode == "online":
            eng.stream_begin(chunk_bytes=64 << 20, copy_threads=2)
            eng.update_objects(self.table.keys, self.table.entry_off, self.cid, table_objects(self.table))
            eng.submit_replay(rp)
            eng.analyze()
            eng.stream_end()
        else:
            eng.submit_replay(rp)
            eng.analyze()
        eng.synchronize()
        assert eng.route_count() > self.routes
        # the engine cut the table where local_lane_cases.partitions says: the replays' shapes are the claimed ones
        want = [int(self.table.keys[k0]) for k0, _ in lc.partitions(self.table, rp.nb_threads)]
        assert eng.route_parts().tolist() == want
        self.routes = eng.route_count()
        _check(eng, raw, self.levels, self.cid)

    def again(self):
        self.eng.reset()
        self.eng.clear_buffers()

    def close(self):
        self.eng.close()


MODES = ["default", "levels", "online"]


@pytest.mark.parametrize("mode", MODES)
def test_stale_slots(oracle_of, mode):
    """B's partly filled chunks lie over A's records: B's result is the oracle's on B alone."""
    a, b = lc.stale_pair()
    r = Runner(a.table, a.nb_threads, mode)
    r.run(a, oracle_of("stale_a", a))
    r.again()
    r.run(b, oracle_of("stale_b", b))
    r.close()


@pytest.mark.parametrize("mode", MODES)
def test_fills_and_list_ends(oracle_of, mode):
    """1, 63, 64 / 65, 127, 128 / 129, 64, 63 and 1 (the lone key) records per partition, on one engine."""
    cases = [lc.fills_case(w)[0] for w in (0, 1, 2)]
    r = Runner(cases[0].table, cases[0].nb_threads, mode)
    for w, rp in enumerate(cases):
        r.run(rp, oracle_of(f"fills{w}", rp))
        r.again()
    r.close()


@pytest.mark.parametrize("kind", ["inline", "wide", "lone"])
def test_directory_shapes(oracle_of, kind):
    rp = lc.directory_case(kind)[0]
    r = Runner(rp.table, rp.nb_threads, "default")
    r.run(rp, oracle_of("dir_" + kind, rp))
    r.close()


@pytest.mark.parametrize("mode", ["default", "levels"])
@pytest.mark.parametrize("first", [True, False], ids=["first_chunk", "second_chunk"])
def test_one_sided_rare_paths(oracle_of, first, mode):
    rp = lc.rare_case(first)[0]
    r = Runner(rp.table, rp.nb_threads, mode)
    r.run(rp, oracle_of(f"rare{int(first)}", rp))
    r.close()
