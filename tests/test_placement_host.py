"""nmg_report_placement_host on the CPU: from the oracle's raw results it must
write a blocks.dat byte-identical to the text placement_expect.py derives from
the oracle's call_sites.log and callsite_counters_<id>.dat files -- the rule
of include/numamma_gpu.h restated in numpy.  Also the library's host object
blocks against the same helper, the rejected arguments, and one hand-written
case whose file is spelled out here."""
import os

import numpy as np
import pytest

import placement_expect as px
from numamma_amd import _lib
from numamma_amd.replay import ENTRY_DTYPE, MEM_DYNAMIC, MEM_GLOBAL, MEM_STACK, ObjectTable, SynthConfig, generate
from numamma_amd.engine import build_meta
from numamma_amd.results import RawResults, _host_results, object_blocks_host, report_placement_host

T = 4
INTERLEAVED = {n: tuple(t % n for t in range(T)) for n in (1, 2, 4)}


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    rp = generate(SynthConfig(nb_samples=20_000, nb_intervals=300, nb_threads=T, seed=101))
    raw, odir = px.run_oracle(rp, str(tmp_path_factory.mktemp("plhost")))
    return rp, raw, odir


def _product(tmp_path, raw, table, o, **kw):
    d = str(tmp_path / "product")
    report_placement_host(raw, table, d, **o.kw(), **kw)
    assert os.listdir(d) == ["blocks.dat"]  # (nothing else is written)
    return open(os.path.join(d, "blocks.dat")).read()


@pytest.mark.parametrize("D", [0, 8])
@pytest.mark.parametrize("interleaved", [False, True], ids=["null_map", "interleaved"])
@pytest.mark.parametrize("N", [1, 2, 4])
def test_file_matches_oracle_counters(tmp_path, case, N, interleaved, D):
    rp, raw, odir = case
    o = px.Opts(N, INTERLEAVED[N] if interleaved else None, D)
    sites = px.site_blocks(odir, rp.table, o)
    # not degenerate: most of the 31 sites, sites of many blocks (one node: one block at most), every node,
    # a global-symbol site, and [stack] left out
    assert len(sites) >= 26
    assert max(s[4].shape[0] for s in sites) >= (12 if N > 1 else 1)
    assert set(np.concatenate([s[4][:, 0] for s in sites]).tolist()) == set(range(N))
    assert any(s[2].startswith("global_var_") for s in sites) and all(s[1] != "[stack]" for s in sites)
    assert _product(tmp_path, raw, rp.table, o) == px.blocks_text(sites)


@pytest.mark.parametrize("N,D", [(1, 8), (2, 0), (4, 8)])
def test_host_object_blocks(case, N, D):
    rp, raw, odir = case
    for o in (px.Opts(N, None, D), px.Opts(N, INTERLEAVED[N], D)):
        want = px.object_rows(raw, rp.table, o)
        assert want.shape[0] > 20
        got = object_blocks_host(raw, rp.table, **o.kw())
        assert got.shape == want.shape and np.array_equal(got, want)


def test_rejections(tmp_path, case):
    rp, raw, odir = case

    def code(**kw):
        with pytest.raises(_lib.NmgError) as ei:
            report_placement_host(raw, rp.table, "/nonexistent/dir", **kw)
        return ei.value.code

    assert _lib.lib.nmg_report_placement_host(None, None, None, None) == -1
    assert code(nb_nodes=0) == -1
    assert code(nb_nodes=65) == -1
    assert code(nb_nodes=3) == -1  # NULL map: 4 threads over 3 nodes
    assert code(nb_nodes=2, thread_node=[0, 1, 2, 0]) == -1  # a node >= nb_nodes
    hr, keep = _host_results(raw, rp.table, np.zeros(raw.nb_buffers, dtype=np.uint64), True)
    meta, kmeta = build_meta(rp.table)
    ro = _lib.nmg_report_options(str(tmp_path / "never").encode(), 1, 0, None, None, None, 0, 0)
    res1, _ = _lib.placement_options(T, 2, reserved=1)  # non-zero reserved
    assert _lib.lib.nmg_report_placement_host(hr, meta, ro, res1) == -1
    assert not os.path.exists(str(tmp_path / "never"))
    with pytest.raises(ValueError):  # the binding: one node per thread rank
        report_placement_host(raw, rp.table, str(tmp_path / "never"), nb_nodes=2, thread_node=[0, 1])
    assert code(nb_nodes=2) == -10  # NMG_ERR_IO: the directory cannot be made
    # the limits themselves: 64 nodes with an explicit map, 3 nodes with one
    for i, kw in enumerate((dict(nb_nodes=64, thread_node=[63, 0, 5, 63]), dict(nb_nodes=3, thread_node=[0, 1, 2, 2]))):
        report_placement_host(raw, rp.table, str(tmp_path / f"ok{i}"), **kw)
        assert os.path.getsize(str(tmp_path / f"ok{i}" / "blocks.dat")) > 0


# ---- a hand-written case: three sites, every line of the file spelled out

def _hand_table():
    """Entries 0, 1: two mallocs of 3 pages from one call site; entry 2: a global
    of 2 pages; entry 3: [stack]; entry 4: a malloc whose caller holds a '/'
    (listed: mallocs are named "malloc"); entry 5: a global whose name holds '['
    (skipped)."""
    names = [b"app.c:7(work)", b"app.c:7(work)", b"table", b"[stack]", b"/lib/x.so(f)", b"arr[4]"]
    pool, offs = b"", []
    for n in names:
        offs.append(len(pool))
        pool += n + b"\0"
    ent = np.zeros(6, dtype=ENTRY_DTYPE)
    ent["buffer_addr"] = [0x10000, 0x20000, 0x30000, 0x7FA000000000, 0x40000, 0x50000]
    ent["buffer_size"] = [8192 + 100, 8192 + 100, 4096, 0x5FFFFFFFFFF, 100, 4096]
    ent["initial_buffer_size"] = ent["buffer_size"]
    ent["alloc_date"] = [10, 10, 0, 0, 10, 0]
    ent["free_date"] = [99, 99, 99, 0, 99, 99]
    ent["caller_rip"] = [0x401000, 0x401000, 0, 0, 0x402000, 0x403000]
    ent["mem_type"] = [MEM_DYNAMIC, MEM_DYNAMIC, MEM_GLOBAL, MEM_STACK, MEM_DYNAMIC, MEM_GLOBAL]
    ent["id"] = np.arange(1, 7)
    ent["caller_off"] = offs
    ent["callstack_size"] = 0
    keys = np.sort(ent["buffer_addr"])
    order = np.argsort(ent["buffer_addr"])
    return ObjectTable(keys, np.arange(7, dtype=np.uint32), ent[order], np.zeros(0, dtype=np.uint64), pool), order


def test_hand_written_case(tmp_path):
    table, order = _hand_table()
    pos = np.argsort(order)  # the entry's position in the table
    E = 6
    # (entry, thread, page, count): threads 0, 1 -> node 0 and 2, 3 -> node 1 under the NULL map
    cells = [
        (0, 0, 0, 5), (1, 1, 0, 4),    # site 1 page 0: node 0 has 9 only through both objects
        (0, 2, 1, 9), (0, 0, 1, 9),    # page 1: a tie 9 : 9, node 0 wins -> the block goes on
        (1, 3, 2, 30), (1, 0, 2, 1),   # page 2: node 1
        (2, 3, 0, 8),                  # site 2 page 0: exactly the threshold, out
        (2, 2, 1, 9),                  # page 1: one more, in
        (3, 0, 5, 100),                # [stack]: skipped
        (4, 0, 0, 50),                 # site 4: malloc
        (5, 0, 0, 50),                 # site 5: a global whose name holds '[': skipped
    ]
    c = np.array(sorted((int(pos[e]), t, p, n) for e, t, p, n in cells), dtype=np.uint32)
    entries = np.zeros((E, 1 + 2 * 39), dtype=np.uint64)
    entries[:, 0] = np.uint64(0xFFFFFFFFFFFFFFFF)
    for k, e in enumerate([0, 1, 2, 3, 4, 5]):  # first-match order = site ids 1 (entries 0, 1), 2, 3, 4, 5
        entries[pos[e], 0] = k
        entries[pos[e], 1] = 1  # one read
    raw = RawResults(E, 0, 4, np.zeros((2, 75), dtype=np.uint64), 0, 0, np.zeros(0, np.uint32), np.zeros(0, np.uint32),
                     entries, c)
    d = str(tmp_path / "out")
    report_placement_host(raw, table, d, nb_nodes=2, density_threshold=8)
    assert open(os.path.join(d, "blocks.dat")).read() == (
        "#site 1 app.c:7(work)\n"
        "begin_block\n"
        "malloc 8292 2\n"
        "0 0 1 18\n"
        "1 2 2 30\n"
        "end_block\n"
        "#site 2 table\n"
        "begin_block\n"
        "table 4096 1\n"
        "1 1 1 9\n"
        "end_block\n"
        "#site 4 /lib/x.so(f)\n"
        "begin_block\n"
        "malloc 100 1\n"
        "0 0 0 50\n"
        "end_block\n")
    # the objects on their own: entry 0's page 0 (5) and entry 1's (4) stay below the threshold
    got = object_blocks_host(raw, table, nb_nodes=2, density_threshold=8)
    want = {0: [(0, 1, 1, 9)], 1: [(1, 2, 2, 30)], 2: [(1, 1, 1, 9)], 4: [(0, 0, 0, 50)], 5: [(0, 0, 0, 50)]}
    exp = sorted((int(pos[e]),) + b for e, bl in want.items() for b in bl)
    assert [tuple(r) for r in got.tolist()] == exp
