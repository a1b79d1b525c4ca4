"""bench.py --dump-outputs: the files hold what the engine's getters return
after the last analysis (themselves bit-exact against the oracle in the parity
tests), as float64, the page-histogram rows sorted and, above the cap, the
same seeded sample of them in every run."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from numamma_amd.replay import SynthConfig, generate  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = {"global_counters", "nb_samples_found", "buffer_samples", "buffer_found", "object_first",
         "object_count_weight", "page_cells", "page_cells_total"}


@pytest.fixture(scope="module")
def analysed():
    """One engine after reset + analyze over a partition-first workload with
    sparse page cells (large objects, the [stack])."""
    import torch
    from numamma_amd.engine import Engine

    rp = generate(SynthConfig(nb_samples=200_000, nb_intervals=30_000, size_max=4 << 20, seed=23))
    arena, offs, lens, ranks, acc = rp.packed()
    d = torch.from_numpy(arena).cuda()
    eng = Engine(nb_threads=rp.nb_threads)
    eng.set_objects(rp.table)
    eng.set_device_buffers(d.data_ptr(), offs, lens, ranks, acc)
    eng.reset()
    eng.analyze()
    eng.synchronize()
    yield eng, rp
    eng.close()


@pytest.mark.parametrize("cap", [None, 1000])
def test_dump_outputs_equal_getters(analysed, tmp_path, monkeypatch, cap):
    import bench

    eng, rp = analysed
    if cap:
        monkeypatch.setattr(bench, "DUMP_MAX_CELLS", cap)
    for d in ("a", "b"):  # twice: the same files
        bench.dump_outputs(eng, str(tmp_path / d))
    assert {f[:-4] for f in os.listdir(tmp_path / "a")} == NAMES
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in NAMES}
    for n in NAMES:
        assert got[n].dtype == np.float64
        assert np.array_equal(got[n], np.load(tmp_path / "b" / (n + ".npy"))), n
    g, ns, nf = eng.global_counters()
    bs, bf = eng.buffer_counts()
    first, cw = eng.object_counters()
    cells = eng.page_cells()
    assert ns == 200_000 and 0 < nf < ns
    for n, want in (("global_counters", g), ("nb_samples_found", [ns, nf]), ("buffer_samples", bs),
                    ("buffer_found", bf), ("object_first", first), ("object_count_weight", cw)):
        want = np.asarray(want)
        assert got[n].shape == want.shape, n
        assert np.array_equal(got[n], want.astype(np.float64)), n
    total = cells.shape[0]
    assert got["page_cells_total"][0] == total > 1000
    rows = got["page_cells"]
    assert rows.shape == (min(total, cap or bench.DUMP_MAX_CELLS), 4)
    # sorted rows of the histogram, each one of the engine's
    key = lambda a: [tuple(r) for r in a.astype(np.int64)]  # noqa: E731
    assert key(rows) == sorted(key(rows))
    assert set(key(rows)) <= set(key(cells))
    if not cap:
        assert len(set(key(rows))) == total
