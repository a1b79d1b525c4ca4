"""The page cost cells and the access timeline through the one-process-per-GPU
merge: two ranks (gloo, both on GPU 0 of the test box, spawned as
test_gpu_distributed.py spawns them) each analyse a byte-balanced shard of
LARGE_CFG at the mid histogram budget -- dense and sparse entries -- with cost
cells (MEMORY, weight, scope ALL) and a timeline (scope ALL) set, then
distributed.merge_engine merges the counters and the two products into rank 0.
Rank 0's cost rows, timeline rows, callsite_cost_<id>.dat,
callsite_timeline_<id>.dat and blocks.dat (NMG_PLACE_PAGE_COST) must equal the
oracle's single unsharded run (cost_expect / timeline_expect /
timeline_all_expect: its dump files binned on the CPU).  A rank that set no
cost cells must make every rank raise, not hang."""
import os
import socket
import sys
import tempfile

import numpy as np
import pytest

import cost_expect as cx
import placement_expect as px
import timeline_all_expect as tax
import timeline_expect as tx
from numamma_amd.replay import generate
from test_gpu_page_cost_all import LARGE_CFG
from test_gpu_page_cost_all import Case as CostCase
from test_gpu_placement_huge import CAP, _mid_budget, dense_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

COST_OPTS = cx.MEMORY_WEIGHT
TL_OPTS = tx.TlOpts(min_object_bytes=0)  # every entry: what the oracle's per-site dumps cover
PLACE = px.Opts(4, density_threshold=0)
FALLBACK_PAIRS = 16  # a CellPacker list buffer no rank's list fits: the dense reduce


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, workdir, mid, mode, ret):
    """mode: dense / packed / fallback (packed with FALLBACK_PAIRS list buffers) / forgot (rank 1 sets no cost cells)."""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
    try:
        import torch
        import torch.distributed as dist

        from numamma_amd import _lib
        from numamma_amd.distributed import CellPacker, merge_engine, shard_ranges
        from numamma_amd.engine import Engine

        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
        dev = torch.device("cuda", 0)
        rp = generate(LARGE_CFG)
        arena, offs, lens, ranks, acc = rp.packed()
        lo, hi = shard_ranges(lens, world)[rank]
        base, end = int(offs[lo]), int(offs[hi - 1] + lens[hi - 1])
        d_arena = torch.from_numpy(arena[base:end].copy()).to(dev)
        eng = Engine(device=0, nb_threads=rp.nb_threads, hist_budget_bytes=mid, sparse_capacity=CAP)
        eng.set_objects(rp.table)
        if not (mode == "forgot" and rank == 1):
            eng.set_page_cost(**COST_OPTS.kw(), scope=_lib.NMG_COST_SCOPE_ALL)
        eng.set_timeline(**TL_OPTS.kw(), scope=_lib.NMG_TL_SCOPE_ALL)
        eng.set_device_buffers(d_arena.data_ptr(), offs[lo:hi] - base, lens[lo:hi], ranks[lo:hi], acc[lo:hi], seq_base=lo)
        eng.analyze()
        eng.synchronize()
        arrays = (_lib.NMG_ARR_COST64, _lib.NMG_ARR_TL32)
        if mode == "fallback":
            eng._cell_packers = {w: CellPacker(eng, dev, w, cap=FALLBACK_PAIRS) for w in arrays}
        try:
            nbytes = merge_engine(eng, dst=0, device=dev, packed_hist=mode in ("packed", "fallback"))
        except RuntimeError as e:
            if mode != "forgot" or "the ranks differ" not in str(e):
                raise
            eng.close()
            dist.destroy_process_group()
            ret.put((rank, "raised: " + str(e)))
            return
        if rank == 0:
            eng.report_page_cost(os.path.join(workdir, "cost"))
            eng.report_timeline(os.path.join(workdir, "tl"))
            eng.report_placement(os.path.join(workdir, "place"), **PLACE.kw(), source=_lib.NMG_PLACE_PAGE_COST)
            # (packed list bytes, dense array bytes) of this rank per merged array
            sizes = np.array([eng._cell_packers[w].last if mode != "dense" else
                              (0, eng.array_size(w) * (8 if w == _lib.NMG_ARR_COST64 else 4)) for w in arrays], dtype=np.int64)
            np.savez(os.path.join(workdir, "merged.npz"), cost=eng.cost_cells(), tl=eng.timeline_cells(),
                     cells=eng.page_cells(), nbytes=nbytes, sizes=sizes,
                     fell_back=np.array([eng._cell_packers[w].dense is not None for w in arrays]))
        eng.close()
        dist.barrier()
        dist.destroy_process_group()
        ret.put((rank, "ok"))
    except Exception:  # surfaced by the parent
        import traceback

        ret.put((rank, traceback.format_exc()))
        raise


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """LARGE_CFG, the oracle's run and every expectation, on the CPU before a rank starts."""
    c = CostCase(generate(LARGE_CFG), str(tmp_path_factory.mktemp("dist_cells")))
    table, T = c.rp.table, c.rp.nb_threads
    assert table.keys.shape[0] > 1023
    c.mid = _mid_budget(table)
    dm = dense_model(table, T, c.mid)
    r = c.rows(COST_OPTS)[:, 0].astype(np.int64)
    assert dm[r].sum() > 300 and (~dm[r]).sum() > 300  # expected cost rows of both kinds at the mid budget
    c.tl = tax.expected_rows_all(c.odir, c.raw, table, TL_OPTS)
    tax.check_covers(c.tl, c.raw, table, TL_OPTS)
    assert dm[c.tl[:, 0]].sum() > 300 and (~dm[c.tl[:, 0]]).sum() > 300
    assert int((tax.selected_all(table, TL_OPTS) & ~dm).sum()) <= tax.MAX_SPARSE
    c.mats = cx.site_matrices(c.odir, T, COST_OPTS)
    c.cost_files = cx.site_files(c.mats)
    c.tl_files = tx.expected_site_files(c.odir, TL_OPTS)
    c.blocks = cx.site_blocks_text(c.odir, table, c.mats, PLACE)
    assert len(c.cost_files) > 50 and len(c.tl_files) > 50 and c.blocks.count("begin_block") > 5
    return c


def _spawn(mid, mode, d):
    import multiprocessing as mp

    ctx = mp.get_context("spawn")
    ret = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, d, mid, mode, ret)) for r in range(2)]
    for p in procs:
        p.start()
    msgs = sorted(ret.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert not any(p.is_alive() for p in procs)
    return msgs, [p.exitcode for p in procs]


@pytest.mark.parametrize("mode", ["dense", "packed", "fallback"])
def test_two_rank_cells_merge_matches_oracle(case, mode):
    c = case
    with tempfile.TemporaryDirectory() as d:
        msgs, codes = _spawn(c.mid, mode, d)
        for rank, msg in msgs:
            assert msg == "ok", f"rank {rank}:\n{msg}"
        assert codes == [0, 0]
        m = np.load(os.path.join(d, "merged.npz"))
        assert np.array_equal(m["cells"], c.raw.cells)
        c.check(m["cost"], COST_OPTS)
        assert m["tl"].dtype == np.uint32 and np.array_equal(m["tl"], c.tl)
        assert cx.read_dir(os.path.join(d, "cost"), "") == c.cost_files
        assert tx.read_dir(os.path.join(d, "tl"), "callsite_timeline_") == c.tl_files
        assert open(os.path.join(d, "place", "blocks.dat")).read() == c.blocks
        sizes = m["sizes"]
        for name, (packed, dense) in zip(("NMG_ARR_COST64", "NMG_ARR_TL32"), sizes.tolist()):
            print(f"{mode}: {name} rank 0 packed list {packed} bytes, dense array {dense} bytes")
        assert (sizes[:, 1] > 0).all() and int(m["nbytes"]) > 0
        if mode == "packed":  # the lists travelled, not the arrays
            assert (sizes[:, 0] > 16 * FALLBACK_PAIRS).all() and not m["fell_back"].any()
        else:  # the arrays themselves
            assert m["fell_back"].all() and int(m["nbytes"]) > int(sizes[:, 1].sum())


def test_a_rank_without_cost_cells_raises_on_every_rank(case):
    with tempfile.TemporaryDirectory() as d:
        msgs, codes = _spawn(case.mid, "forgot", d)
        for rank, msg in msgs:
            assert msg.startswith("raised: ") and "page cost cells" in msg and "product options" in msg, f"rank {rank}:\n{msg}"
        assert codes == [0, 0] and not os.path.exists(os.path.join(d, "merged.npz"))
