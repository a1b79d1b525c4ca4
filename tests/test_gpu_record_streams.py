"""Both record-stream parsers -- route2_kernel's per-wave cursor and
attribute_kernel's window cursor -- on irregular perf record streams
(stream_grammar.py): bit-exact against the oracle, whose reading of these
streams test_record_streams_host.py establishes on the CPU.

Parity: the raw dump, stdout and the report directory, as test_gpu_parity.py
compares them, for the grammar replay (every pattern: alternating LOST
records, 40 B non-SAMPLE records, long and short SAMPLEs, 64 KiB jumps,
header-only runs, irregular records around the 64- and 1024-slot window edges,
an overshooting last record, buffers without samples, an empty ring, dense
mixes, a wrapped ring) and for the tiny replay (tens of thousands of buffers
of 1-5 records), on attribute_kernel (309 keys; 3009 keys with the internal
legacy switches) and on every variant of the partition-first path; streamed
in chunks, device-resident, over two workers and analysed twice (buffers read
in place from registered host memory are not covered here); and with the outputs of the local pass that
re-read the raw record at its byte offset (levels, dump files, timeline, page
cost cells).

Errors: the expected (code, buffer, byte offset) comes from the byte cursor
walk() over the non-empty buffers in submission order -- kind x position x
path, two malformed buffers at once (the smallest (buffer, offset) wins), and
an engine reused after an error."""
import os

import numpy as np
import pytest

import cost_expect as cx
import pyoracle
import stream_grammar as sg
import timeline_expect as tx
from numamma_amd import _lib
from numamma_amd.replay import Replay, SynthConfig, generate
from numamma_amd.results import RawResults

pytestmark = pytest.mark.gpu

NO_ROUTE = 0x10000
TINY_POOL = 0x20000
TINY_OVF = 0x80000
NO_LINES = 0x20000000
LAP_NOWAIT = 0x100000
TINY_LOG = 0x2000  # (internal, legacy only) attribute_kernel's hashed long-tail log with sub-logs of 2 records
LEGACY = (NO_ROUTE, TINY_LOG, _lib.NMG_F_SINGLE_PASS)
DUMPS = _lib.NMG_F_DEFAULT | _lib.NMG_F_OBJECT_LEVELS | _lib.NMG_F_SAMPLE_MATCHES
DUMP_ALL = _lib.NMG_DUMP_CALLSITES | _lib.NMG_DUMP_ALL | _lib.NMG_DUMP_UNMATCHED
MAPS = ("00400000-00452000 r-xp 00000000 08:02 173521 /usr/bin/app\n"
        "555500000000-555600000000 rw-p 00000000 00:00 0 [heap]\n"
        "7ffd0000-7ffd1000 rw-p 00000000 00:00 0 [stack]\n")
MODULES = [(0x400000, 0x480000, 0x400000, "/usr/bin/app"), (0x480000, 0x4F0000, 0x470000, "/usr/lib/libfoo.so.1")]


def _same(a, b):
    assert open(a, "rb").read() == open(b, "rb").read(), (a, b)


def _same_dirs(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert fa == fb
    for f in fa:
        _same(os.path.join(a, f), os.path.join(b, f))


class Case:
    """A replay, its file and the oracle's raw dump, stdout and report directory."""

    def __init__(self, rp, d):
        self.rp, self.d = rp, d
        self.path = os.path.join(d, "replay.bin")
        rp.write(self.path)
        self.odir = os.path.join(d, "oracle")
        self.ostdout = os.path.join(d, "oracle_stdout.txt")
        self.oraw = os.path.join(d, "oracle_raw.bin")
        pyoracle.run(self.path, self.odir, self.ostdout, self.oraw)
        self.raw = RawResults.read(self.oraw)
        assert self.raw.nb_found > 0

    def check_replay(self, tmp_path, flags):
        """nmg_run_replay over the file: raw dump, stdout, report directory."""
        from numamma_amd.engine import run_replay

        d = str(tmp_path)
        edir, eraw, eout = os.path.join(d, "engine"), os.path.join(d, "engine_raw.bin"), os.path.join(d, "engine.txt")
        run_replay(self.path, edir, eout, eraw, flags=flags)
        got = RawResults.read(eraw)
        assert np.array_equal(got.buf_samples, self.raw.buf_samples) and np.array_equal(got.buf_found, self.raw.buf_found)
        assert np.array_equal(got.global_counters, self.raw.global_counters)
        assert np.array_equal(got.entries, self.raw.entries) and np.array_equal(got.cells, self.raw.cells)
        _same(self.oraw, eraw)
        _same(self.ostdout, eout)
        _same_dirs(self.odir, edir)

    def check_engine(self, eng, tmp_path=None, times=1):
        """The engine's counters against the oracle's raw dump (`times` analyses
        accumulated: counts and weights scale, first ordinals do not); with
        tmp_path, its report too."""
        raw, k = self.raw, np.uint64(times)
        g, ns, nf = eng.global_counters()
        assert (ns, nf) == (times * raw.nb_samples, times * raw.nb_found)
        if times == 1:
            assert np.array_equal(g, raw.global_counters)
        s, f = eng.buffer_counts()
        assert np.array_equal(s, times * raw.buf_samples) and np.array_equal(f, times * raw.buf_found)
        first, cw = eng.object_counters()
        assert np.array_equal(first, raw.first_ordinal)
        assert np.array_equal(cw, raw.count_weight * k)
        cells = eng.page_cells()
        assert np.array_equal(cells[:, :3], raw.cells[:, :3]) and np.array_equal(cells[:, 3], times * raw.cells[:, 3])
        if tmp_path is not None:
            edir, eout = os.path.join(str(tmp_path), "engine"), os.path.join(str(tmp_path), "engine.txt")
            eng.report(edir, eout)
            _same(self.ostdout, eout)
            _same_dirs(self.odir, edir)


@pytest.fixture(scope="module")
def g300(tmp_path_factory):
    return Case(sg.grammar_replay(300), str(tmp_path_factory.mktemp("g300")))


@pytest.fixture(scope="module")
def g3000(tmp_path_factory):
    return Case(sg.grammar_replay(3000), str(tmp_path_factory.mktemp("g3000")))


@pytest.fixture(scope="module")
def t300(tmp_path_factory):
    return Case(sg.tiny_replay(300), str(tmp_path_factory.mktemp("t300")))


@pytest.fixture(scope="module")
def t3000(tmp_path_factory):
    return Case(sg.tiny_replay(3000), str(tmp_path_factory.mktemp("t3000")))


def _engine(rp, flags=_lib.NMG_F_DEFAULT, **kw):
    from numamma_amd.engine import Engine

    eng = Engine(flags=flags, nb_threads=rp.nb_threads, **kw)
    eng.set_objects(rp.table)
    return eng


def _routes(eng, extra):
    n = eng.route_count()
    return n == 0 if (extra & (NO_ROUTE | TINY_LOG | _lib.NMG_F_SINGLE_PASS)) else n > 0


# ---- 1. parity on every path

@pytest.mark.parametrize("extra", [0, _lib.NMG_F_SINGLE_PASS], ids=["default", "single"])
def test_grammar_small_table(tmp_path, g300, extra):
    g300.check_replay(tmp_path, _lib.NMG_F_DEFAULT | extra)
    eng = _engine(g300.rp, _lib.NMG_F_DEFAULT | extra)
    eng.submit_replay(g300.rp)
    eng.analyze()
    eng.synchronize()
    assert eng.route_count() == 0  # 309 keys: attribute_kernel
    g300.check_engine(eng)
    eng.close()


LARGE = [0, TINY_POOL, TINY_POOL | TINY_OVF, NO_LINES, LAP_NOWAIT, NO_ROUTE, TINY_LOG]
LARGE_IDS = ["route", "tinypool", "tinyovf", "nolines", "lapnowait", "noroute", "tinylog"]


@pytest.mark.parametrize("extra", LARGE, ids=LARGE_IDS)
def test_grammar_large_table(tmp_path, g3000, extra):
    g3000.check_replay(tmp_path, _lib.NMG_F_DEFAULT | extra)


@pytest.mark.parametrize("extra", LARGE, ids=LARGE_IDS)
def test_grammar_large_table_engine(g3000, extra):
    """The same through Engine, which tells which kernels ran."""
    eng = _engine(g3000.rp, _lib.NMG_F_DEFAULT | extra)
    eng.submit_replay(g3000.rp)
    eng.analyze()
    eng.synchronize()
    assert _routes(eng, extra)
    g3000.check_engine(eng)
    eng.close()


def test_tiny_small_table(tmp_path, t300):
    t300.check_replay(tmp_path, _lib.NMG_F_DEFAULT)


@pytest.mark.parametrize("extra", [0, NO_ROUTE, TINY_POOL], ids=["route", "noroute", "tinypool"])
def test_tiny_large_table(tmp_path, t3000, extra):
    assert len(t3000.rp.buffers) >= 16_384
    t3000.check_replay(tmp_path, _lib.NMG_F_DEFAULT | extra)
    eng = _engine(t3000.rp, _lib.NMG_F_DEFAULT | extra)
    eng.submit_replay(t3000.rp)
    eng.analyze()
    eng.synchronize()
    assert _routes(eng, extra)
    eng.close()


# ---- 2. other ways of submitting the buffers

def test_streamed_chunks(tmp_path, monkeypatch, g3000):
    """64 KiB chunks: the jump buffers (about 400 KiB each) are larger than a chunk."""
    monkeypatch.setenv("NMG_REPLAY_STREAM", "65536:2:3")
    g3000.check_replay(tmp_path, _lib.NMG_F_DEFAULT)


def test_device_resident(tmp_path, g3000):
    import torch

    rp = g3000.rp
    arena, offs, lens, ranks, acc = rp.packed()
    dev = torch.from_numpy(arena).cuda()
    eng = _engine(rp)
    eng.set_device_buffers(dev.data_ptr(), offs, lens, ranks, acc)
    eng.analyze()
    eng.synchronize()
    assert eng.route_count() > 0
    g3000.check_engine(eng, tmp_path)
    eng.close()


def test_two_workers(tmp_path, g3000):
    eng = _engine(g3000.rp, devices=[0, 0])
    eng.submit_replay(g3000.rp)
    eng.analyze()
    eng.synchronize()
    assert eng.route_count() >= 2
    g3000.check_engine(eng, tmp_path)
    eng.close()


@pytest.mark.parametrize("extra", [0, NO_ROUTE], ids=["route", "noroute"])
def test_analysed_twice_without_reset(g3000, extra):
    eng = _engine(g3000.rp, _lib.NMG_F_DEFAULT | extra)
    eng.submit_replay(g3000.rp)
    eng.analyze()
    eng.analyze()
    eng.synchronize()
    g3000.check_engine(eng, times=2)
    eng.close()


# ---- 3. the outputs that re-read the raw record at its byte offset

@pytest.fixture(scope="module")
def levels_case(tmp_path_factory):
    """The grammar replay with every sample's level redrawn over ALL_LEVELS
    (multi-bit levels on short and long SAMPLEs too), the oracle run with every
    dump mode."""
    d = str(tmp_path_factory.mktemp("g3000_levels"))
    rp = sg.grammar_replay(3000, prepare_pool=lambda p: cx.redraw_levels(p, 92))
    raw, odir = tx.run_oracle(rp, d, dump_unmatched=True, maps_path="/proc/4242/maps", maps_text=MAPS, modules=MODULES)
    lv = cx.oracle_levels(raw)
    assert lv[:, 0].sum(axis=0).all()  # reads: N/A and every bucket's count and weight sum
    return rp, raw, odir, os.path.join(d, "o.txt")


@pytest.mark.parametrize("extra", [0, _lib.NMG_F_SINGLE_PASS], ids=["route", "single"])
def test_levels_dumps_and_timeline(tmp_path, levels_case, extra):
    rp, raw, odir, ostdout = levels_case
    o = tx.TlOpts()
    eng = _engine(rp, DUMPS | extra)
    eng.set_timeline(**o.kw())
    eng.submit_replay(rp)
    eng.analyze()
    eng.synchronize()
    assert _routes(eng, extra)
    assert np.array_equal(eng.object_levels(), cx.oracle_levels(raw))
    assert np.array_equal(eng.object_counters()[1], raw.count_weight)
    want, nlines = tx.expected_rows(odir, rp.table, rp.nb_threads, o)
    assert nlines > 5_000 and want.shape[0] > 1_000
    assert np.array_equal(eng.timeline_cells(), want)
    edir, eout = os.path.join(str(tmp_path), "engine"), os.path.join(str(tmp_path), "e.txt")
    eng.report(edir, eout, dump_flags=DUMP_ALL, maps_path="/proc/4242/maps", maps_text=MAPS, modules=MODULES)
    eng.close()
    _same(ostdout, eout)
    assert {"all_memory_accesses.dat", "all_memory_objects.dat", "unmatched_samples.log"} <= set(os.listdir(odir))
    _same_dirs(odir, edir)


@pytest.fixture(scope="module")
def cost_case(tmp_path_factory, g3000):
    """The grammar replay's dump lines (generator levels: one bit or none, so
    the level strings select exactly; see stream_grammar.pat_short)."""
    rp = g3000.rp
    raw, odir = tx.run_oracle(rp, str(tmp_path_factory.mktemp("g3000_cost")))
    return rp, cx.Dump(odir, rp.table, rp.nb_threads)


@pytest.mark.parametrize("o", [cx.MEMORY_WEIGHT, cx.EVERYTHING], ids=["memory-weight", "all-count"])
@pytest.mark.parametrize("extra", [0, _lib.NMG_F_SINGLE_PASS], ids=["route", "single"])
def test_page_cost_cells(cost_case, extra, o):
    rp, dump = cost_case
    want, nsel = dump.rows(o)
    assert nsel > 500
    eng = _engine(rp, _lib.NMG_F_DEFAULT | extra)
    eng.set_page_cost(**o.kw())
    eng.submit_replay(rp)
    eng.analyze()
    eng.synchronize()
    assert _routes(eng, extra)
    rows = eng.cost_cells()
    eng.close()
    assert rows.dtype == np.uint64 and rows.shape == want.shape and np.array_equal(rows, want)


# ---- 4. malformed streams

CODES = {"zero_size": -4, "truncated": -5, "unaligned": -9}
ORACLE_SAYS = {"zero_size": "size 0", "truncated": "truncated"}
PATHS = [(300, 0), (3000, 0), (3000, NO_ROUTE)]
PATH_IDS = ["attribute", "route", "noroute"]
KINDS = ["zero_size", "size44", "size4", "cut_sample", "cut_long_sample", "cut_header"]
POSITIONS = [7, 64, 200, 299]


_SRC = {}


def _pool(nkeys):
    """Sample payloads over grammar_replay(nkeys)'s table (same seed: the table is drawn first)."""
    if nkeys not in _SRC:
        _SRC[nkeys] = generate(SynthConfig(nb_samples=20_000, nb_intervals=nkeys, seed=211))
    return _SRC[nkeys], sg.Pool(_SRC[nkeys])


def _set_size(rec, size):
    return rec[:6] + int(size).to_bytes(2, "little") + rec[8:]


def malformed(pool, rng, T, kind, pos, nrec=300):
    """A buffer of nrec records whose record `pos` is malformed.  pos 64 comes
    right after a full run of 64 regular records (a whole route window, a
    whole ballot step of both slow paths); pos 200 has irregular records
    before it; the cut kinds end the buffer inside record pos."""
    parts = sg.regular(pool, nrec)
    if pos == 200:
        for i in (3, 70, 131, 199):
            parts[i] = (sg.lost24(rng), sg.header(sg.LOST, 8), sg.sample(pool.take(), 56, rng), sg.other(3, 40, rng))[i % 4]
    if kind == "zero_size":
        parts[pos] = _set_size(parts[pos], 0)
    elif kind == "size44":
        parts[pos] = _set_size(parts[pos], 44)
    elif kind == "size4":
        parts[pos] = _set_size(parts[pos], 4)
    elif kind == "cut_sample":  # the last record cut to 24 B
        parts = parts[:pos] + [parts[pos][:24]]
    elif kind == "cut_long_sample":  # a SAMPLE of size 48 cut at 40 B
        parts = parts[:pos] + [sg.sample(pool.take(), 48, rng)[:40]]
    elif kind == "cut_header":  # 4 B of a header
        parts = parts[:pos] + [parts[pos][:4]]
    else:
        raise ValueError(kind)
    return sg.buffer_of(parts, rng, T)


def expected_error(rp):
    """(code, buffer, offset, kind) of the first malformed record in analysis order, from walk()."""
    for seq, (_, _, lin) in enumerate(rp.linear_buffers()):
        _, err = sg.walk(lin)
        if err is not None:
            return CODES[err[0]], seq, err[1], err[0]
    return None


def _expect_error(eng, want, run=None):
    """The analysis reports `want` -- at nmg_synchronize; a stream (run given:
    submissions, flush and end) may report it at any call after the chunk."""
    if run is None:
        eng.analyze()
        run = eng.synchronize
    with pytest.raises(_lib.NmgError) as ei:
        run()
    code, seq, off, _ = want
    assert ei.value.code == code, str(ei.value)
    assert f"buffer {seq} (analysis order), byte offset {off}:" in str(ei.value)


def _oracle_agrees(rp, tmp_path, kind):
    if kind not in ORACLE_SAYS:
        return  # (the reference has no alignment rule: walk() is the only reference)
    path = os.path.join(str(tmp_path), "bad.bin")
    rp.write(path)
    with pytest.raises(RuntimeError, match=ORACLE_SAYS[kind]):
        pyoracle.run(path, os.path.join(str(tmp_path), "o"), os.path.join(str(tmp_path), "o.txt"))


@pytest.mark.parametrize("path", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("pos", POSITIONS)
@pytest.mark.parametrize("kind", KINDS)
def test_error_matrix(tmp_path, kind, pos, path):
    nkeys, extra = path
    src, pool = _pool(nkeys)
    rng = np.random.default_rng(1000 * pos + KINDS.index(kind))
    T = src.nb_threads
    bufs = [sg.buffer_of(sg.regular(pool, 300), rng, T), malformed(pool, rng, T, kind, pos),
            sg.buffer_of(sg.regular(pool, 300), rng, T)]
    rp = Replay(T, src.table, bufs)
    want = expected_error(rp)
    assert want is not None and want[1] == 1
    assert want[3] == {"zero_size": "zero_size", "size44": "unaligned", "size4": "unaligned"}.get(kind, "truncated")
    if pos != 200:
        assert want[2] == 40 * pos
    _oracle_agrees(rp, tmp_path, want[3])
    eng = _engine(rp, _lib.NMG_F_DEFAULT | extra)
    eng.submit_replay(rp)  # (a length of 40 k + 4 is accepted: the kernels report it)
    _expect_error(eng, want)
    assert eng.route_count() == (1 if (nkeys, extra) == (3000, 0) else 0)
    eng.close()


@pytest.mark.parametrize("streamed", [False, True], ids=["batch", "streamed"])
@pytest.mark.parametrize("path", PATHS, ids=PATH_IDS)
def test_first_error_in_analysis_order(path, streamed):
    """Forty clean buffers and two malformed ones, at 31 and at 9.  Buffer 31's
    error has the smaller offset and the smaller code; buffer 9 holds two
    errors.  The one reported is the first the reference's loop would meet:
    buffer 9's first."""
    nkeys, extra = path
    src, pool = _pool(nkeys)
    rng = np.random.default_rng(77)
    T = src.nb_threads
    bufs = [sg.buffer_of(sg.regular(pool, 300), rng, T) for _ in range(42)]
    bufs[31] = malformed(pool, rng, T, "zero_size", 3)
    two = sg.regular(pool, 300)
    two[50] = _set_size(two[50], 44)
    two[120] = _set_size(two[120], 0)
    bufs[9] = sg.buffer_of(two, rng, T)
    rp = Replay(T, src.table, bufs)
    want = expected_error(rp)
    assert want[:3] == (-9, 9, 2000)
    eng = _engine(rp, _lib.NMG_F_DEFAULT | extra)
    def submit():
        for r, a, data in rp.linear_buffers():
            eng.submit_buffer(data, r, a)

    def stream():
        eng.stream_begin(chunk_bytes=64 << 10, copy_threads=2)  # 12 KB buffers: the two errors in different chunks
        submit()
        eng.analyze()
        eng.stream_end()
        eng.synchronize()

    if streamed:
        _expect_error(eng, want, stream)
    else:
        submit()
        _expect_error(eng, want)
    eng.close()


@pytest.mark.parametrize("path", PATHS, ids=PATH_IDS)
def test_reuse_after_error(tmp_path, g300, g3000, path):
    """nmg_reset_counters clears a reported stream error with the counters:
    after reset() and clear_buffers() the engine analyses other buffers as a
    new one would."""
    nkeys, extra = path
    case = g300 if nkeys == 300 else g3000
    src, pool = _pool(nkeys)
    assert np.array_equal(src.table.keys, case.rp.table.keys) and np.array_equal(src.table.entries, case.rp.table.entries)
    rng = np.random.default_rng(78)
    T = src.nb_threads
    bad = Replay(T, src.table, [sg.buffer_of(sg.regular(pool, 300), rng, T), malformed(pool, rng, T, "zero_size", 64)])
    eng = _engine(case.rp, _lib.NMG_F_DEFAULT | extra)
    eng.submit_replay(bad)
    _expect_error(eng, expected_error(bad))
    with pytest.raises(_lib.NmgError):  # the error stays until the counters are reset
        eng.synchronize()
    eng.reset()
    eng.clear_buffers()
    eng.submit_replay(case.rp)
    eng.analyze()
    eng.synchronize()
    case.check_engine(eng, tmp_path)
    eng.close()
