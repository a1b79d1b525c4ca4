"""TEST INFRASTRUCTURE ONLY -- ctypes access to the CPU oracle (liboracle.so),
to the reference's own AVL index (oracle/_ref/libref_hash.so) and to its own
sample loop (oracle/_ref/libref_loop.so).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may use
this module, and only as the checker / CPU baseline.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
# (NMG_ORACLE_DIR: the sanitizer build of the oracle libraries, tools/sanitize.sh)
SO_DIR = os.environ.get("NMG_ORACLE_DIR") or HERE
ORACLE_SO = os.path.join(SO_DIR, "liboracle.so")
REF_SO = os.path.join(HERE, "_ref", "libref_hash.so")
REF_HASH_TEST = os.path.join(HERE, "_ref", "hash_test")


def build(quiet: bool = True) -> None:
    """make -C oracle (the reference pieces only build where /root/reference exists)."""
    subprocess.run(["make", "-C", HERE], check=True, stdout=subprocess.DEVNULL if quiet else None)


class _Module(C.Structure):
    _fields_ = [("lo", C.c_uint64), ("hi", C.c_uint64), ("fbase", C.c_uint64), ("fname", C.c_char_p)]


class _Alarm(C.Structure):
    _fields_ = [("buf_end", C.c_uint32), ("nb_keys", C.c_uint32), ("keys", C.c_void_p), ("entry_off", C.c_void_p),
                ("entry_ids", C.c_void_p), ("ent4", C.c_void_p)]


class _Settings(C.Structure):
    _fields_ = [("match_samples", C.c_int), ("dump_single_items", C.c_int), ("dump", C.c_int),
                ("dump_all", C.c_int), ("dump_unmatched", C.c_int), ("reserved", C.c_int),
                ("maps_path", C.c_char_p), ("maps_text", C.c_char_p),
                ("modules", C.POINTER(_Module)), ("nb_modules", C.c_uint32), ("reserved2", C.c_uint32),
                ("alarms", C.POINTER(_Alarm)), ("nb_alarms", C.c_uint32), ("reserved3", C.c_uint32)]


class _Timing(C.Structure):
    _fields_ = [("analysis_s", C.c_double), ("total_s", C.c_double), ("nb_samples", C.c_uint64)]


_oracle = None


def oracle():
    global _oracle
    if _oracle is None:
        if not os.path.exists(ORACLE_SO):
            build()
        lib = C.CDLL(ORACLE_SO)
        lib.nmo_run.restype = C.c_int
        lib.nmo_run.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(_Settings), C.POINTER(_Timing)]
        lib.nmo_strerror.restype = C.c_char_p
        lib.nmo_strerror.argtypes = [C.c_int]
        lib.nmo_lookup.restype = C.c_int64
        lib.nmo_lookup.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64]
        _oracle = lib
    return _oracle


def run(replay_path: str, outdir: str, stdout_path: str, raw_path: str | None = None,
        match_samples: bool = True, dump_single_items: bool = True, dump: bool = False,
        dump_all: bool = False, dump_unmatched: bool = False, maps_path: str | None = None,
        maps_text: str | None = None, modules=None, alarms=None) -> dict:
    """Dump modes (-d / -D / -u) write callsite_dump_<id>.dat, callsite_summary_<id>.dat,
    all_memory_accesses.dat, all_memory_objects.dat and unmatched_samples.log into
    outdir like the reference.  modules = [(lo, hi, fbase, fname)]: dladdr()'s view
    of the traced process, for all_memory_objects.dat.  alarms = [(buf_end, keys,
    entry_off, entry_ids, ent4)]: --online-analysis, each alarm's buffers against
    the table at that alarm (replay.table_at)."""
    import numpy as np

    lib = oracle()
    mods = list(modules or [])
    marr = (_Module * max(1, len(mods)))(*[_Module(lo, hi, fb, fn.encode()) for lo, hi, fb, fn in mods])
    keep = []
    al = list(alarms or [])
    aarr = (_Alarm * max(1, len(al)))()
    for i, (buf_end, keys, off, ids, ent4) in enumerate(al):
        arrs = [np.ascontiguousarray(keys, dtype=np.uint64), np.ascontiguousarray(off, dtype=np.uint32),
                np.ascontiguousarray(ids, dtype=np.uint32), np.ascontiguousarray(ent4, dtype=np.uint64)]
        keep += arrs
        aarr[i] = _Alarm(buf_end, arrs[0].shape[0], *[a.ctypes.data for a in arrs])
    s = _Settings(int(match_samples), int(dump_single_items), int(dump), int(dump_all), int(dump_unmatched), 0,
                  maps_path.encode() if maps_path else None, maps_text.encode() if maps_text else None,
                  marr, len(mods), 0, aarr, len(al), 0)
    t = _Timing()
    rc = lib.nmo_run(replay_path.encode(), outdir.encode(), stdout_path.encode(),
                     raw_path.encode() if raw_path else None, C.byref(s), C.byref(t))
    if rc:
        raise RuntimeError(f"oracle failed: {lib.nmo_strerror(rc).decode()} ({rc})")
    return {"analysis_s": t.analysis_s, "total_s": t.total_s, "nb_samples": t.nb_samples}


def lookup(keys, entry_off, ent4, addr: int, ts: int) -> int:
    import numpy as np

    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    entry_off = np.ascontiguousarray(entry_off, dtype=np.uint32)
    ent4 = np.ascontiguousarray(ent4, dtype=np.uint64)
    return oracle().nmo_lookup(keys.ctypes.data, entry_off.ctypes.data, keys.shape[0], ent4.ctypes.data, addr, ts)


_ref = None


def ref_available() -> bool:
    return os.path.exists(REF_SO)


def ref():
    """The reference's tools/hash.c (unchanged) behind oracle/ref_hash_shim.c."""
    global _ref
    if _ref is None:
        lib = C.CDLL(REF_SO)
        lib.ref_reset.restype = None
        lib.ref_insert.argtypes = [C.c_uint64, C.c_uint64]
        lib.ref_insert.restype = None
        lib.ref_lower_key.argtypes = [C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int]
        lib.ref_lower_key.restype = C.c_int
        lib.ref_foreach.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int64]
        lib.ref_foreach.restype = C.c_int64
        lib.ref_size.restype = C.c_int
        _ref = lib
    return _ref


# ---- the reference's own sample loop (oracle/ref_loop_shim.c -> oracle/_ref/libref_loop.so)
REF_LOOP_SO = os.path.join(HERE, "_ref", "libref_loop.so")
RL_OK, RL_ABORT, RL_ASSERT = 0, 1, 2  # ref_loop_shim.c: how a call into the reference ended
COUNTERS_BYTES = 600  # struct mem_counters (tests/test_abi.py)

_ref_loop = None


def ref_loop_available() -> bool:
    return os.path.exists(REF_LOOP_SO)


def ref_loop():
    """The reference's src/mem_sampling.c + src/mem_analyzer.c (unchanged)
    behind oracle/ref_loop_shim.c."""
    global _ref_loop
    if _ref_loop is None:
        lib = C.CDLL(REF_LOOP_SO)
        u64p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
        lib.rl_reset.argtypes = [C.c_int]
        lib.rl_add.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64]
        lib.rl_move.argtypes = [C.c_int, C.c_uint64]
        lib.rl_free.argtypes = [C.c_int, C.c_uint64, C.c_uint64]
        lib.rl_object.argtypes = [C.c_int, u64p]
        lib.rl_find.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rl_feed.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint, C.c_int, i32p]
        lib.rl_globals.argtypes = [C.c_void_p, u64p]
        lib.rl_blocks.argtypes = [C.c_int, C.c_void_p, C.c_int64]
        lib.rl_blocks.restype = C.c_int64
        lib.rl_update_counters.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        assert lib.rl_counters_bytes() == COUNTERS_BYTES
        _ref_loop = lib
    return _ref_loop


def _counter_pairs(fn, data_src, weight, access: int, fresh: bool):
    import numpy as np

    ds = np.ascontiguousarray(data_src, dtype=np.uint64)
    w = np.ascontiguousarray(weight, dtype=np.uint64)
    assert ds.shape == w.shape
    out = np.zeros((ds.shape[0] if fresh else 1, 2 * COUNTERS_BYTES), dtype=np.uint8)
    rc = fn(ds.shape[0], ds.ctypes.data, w.ctypes.data, access, int(fresh), out.ctypes.data)
    if rc:
        raise RuntimeError(f"update_counters failed ({rc})")
    return out


def ref_update_counters(data_src, weight, access: int, fresh: bool = True):
    """The reference's update_counters on (data_src, weight) samples: the
    bytes of struct mem_counters[2], per sample on fresh counters (fresh) or
    once after all of them."""
    return _counter_pairs(ref_loop().rl_update_counters, data_src, weight, access, fresh)


def update_counters(data_src, weight, access: int, fresh: bool = True):
    """The oracle's o_update_counters, as ref_update_counters."""
    lib = oracle()
    lib.nmo_update_counters.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return _counter_pairs(lib.nmo_update_counters, data_src, weight, access, fresh)


class RefLoop:
    """One run of the reference's loop: objects in, buffers through
    __copy_buffer + __analyze_buffer, counters out.  The library holds one
    state: a new RefLoop resets it."""

    def __init__(self, match_samples: bool = True):
        self.lib = ref_loop()
        self._ok(self.lib.rl_reset(int(match_samples)))
        self.buf_samples, self.buf_found, self.status = [], [], []

    @staticmethod
    def _ok(rc):
        if rc:
            raise RuntimeError(f"the reference stopped ({'abort' if rc == RL_ABORT else 'assert' if rc == RL_ASSERT else rc})")

    def add(self, kind: int, addr: int, size: int, alloc_date: int, free_date: int) -> int:
        idx = self.lib.rl_add(kind, addr, size, alloc_date, free_date)
        if idx < 0:
            self._ok(-1 - idx)
        return idx

    def move(self, idx: int, new_addr: int):
        self._ok(self.lib.rl_move(idx, new_addr))

    def free(self, idx: int, size: int, free_date: int):
        self._ok(self.lib.rl_free(idx, size, free_date))

    def object(self, idx: int):
        out = (C.c_uint64 * 6)()
        self._ok(self.lib.rl_object(idx, out))
        return list(out)

    def add_table(self, table):
        """The objects of a flattened table (numamma_amd.replay.ObjectTable),
        each key's entries oldest first (the AVL node's list is newest-first),
        through the calls the traced process would have made: malloc at the
        key, realloc to buffer_addr where it differs, free with the final
        size; globals and the [stack] by their own paths.  Returns
        obj_of_entry (the shim's number per entry)."""
        import numpy as np

        ent, off = table.entries, table.entry_off.astype(np.int64)
        obj = np.full(ent.shape[0], -1, dtype=np.int64)
        for k in range(table.nb_keys):
            key = int(table.keys[k])
            for e in range(int(off[k + 1]) - 1, int(off[k]) - 1, -1):
                x = ent[e]
                mt, addr, size = int(x["mem_type"]), int(x["buffer_addr"]), int(x["buffer_size"])
                al, fr = int(x["alloc_date"]), int(x["free_date"])
                if mt == 2:  # [stack]: the reference's fixed range
                    i = self.add(2, 0, 0, al, fr)
                    assert self.object(i)[:2] == [addr, size] and key == addr
                elif mt == 3:  # dynamic_allocation
                    i = self.add(0, key, int(x["initial_buffer_size"]), al, 0)
                    if addr != key:
                        self.move(i, addr)
                    self.free(i, size, fr)
                else:  # global_symbol / lib
                    assert key == addr
                    i = self.add(1, addr, size, al, fr)
                obj[e] = i
        return obj

    def find(self, addr, ts):
        """ma_find_mem_info_from_sample per (addr, timestamp): the shim's object number, -1 for none."""
        import numpy as np

        a = np.ascontiguousarray(addr, dtype=np.uint64)
        t = np.ascontiguousarray(ts, dtype=np.uint64)
        out = np.zeros(a.shape[0], dtype=np.int32)
        self._ok(self.lib.rl_find(a.shape[0], a.ctypes.data, t.ctypes.data, out.ctypes.data))
        return out

    def feed(self, ring, data_tail: int, data_head: int, thread_rank: int, access: int):
        """One ring through __copy_buffer and __analyze_buffer.  Returns
        (status, samples, found); an empty ring (head == tail) is not recorded
        as a buffer, as it gets no analysis index."""
        import numpy as np

        ring = np.ascontiguousarray(ring, dtype=np.uint8)
        if data_head >= ring.shape[0]:
            # a replay's buffer is a struct sample_list, whose data_head may equal the ring's size; the
            # mmap page's data_head is reduced modulo data_size (mem_sampling.c:936) and would read as 0:
            # describe the same bytes as a ring with one unread slot after them
            ring = np.concatenate([ring, np.zeros(data_head + 8 - ring.shape[0], dtype=np.uint8)])
        cnt = (C.c_int32 * 2)()
        st = self.lib.rl_feed(ring.ctypes.data, ring.shape[0], data_tail, data_head, thread_rank, access, cnt)
        if data_head % ring.shape[0] != data_tail:
            self.buf_samples.append(cnt[0])
            self.buf_found.append(cnt[1])
            self.status.append(st)
        return st, cnt[0], cnt[1]

    def global_counters(self):
        """(raw bytes of global_counters[2], samples, found)"""
        import numpy as np

        out = np.zeros(2 * COUNTERS_BYTES, dtype=np.uint8)
        tot = (C.c_uint64 * 2)()
        assert self.lib.rl_globals(out.ctypes.data, tot) == 2 * COUNTERS_BYTES
        return out, tot[0], tot[1]

    def blocks(self, idx: int):
        """u64 rows (thread, block id, counters[READ] 75 words, counters[WRITE]
        75 words) of an object's page blocks with a count; None if it never matched."""
        import numpy as np

        width = 2 + 2 * COUNTERS_BYTES // 8
        n = self.lib.rl_blocks(idx, None, 0)
        if n == -1:
            return None
        assert n >= 0
        out = np.zeros((n, width), dtype=np.uint64)
        assert self.lib.rl_blocks(idx, out.ctypes.data, n) == n
        return out


# ---- the multi-threaded restatement (oracle/nmg_cpu_mt.cpp)
class _MtTiming(C.Structure):
    _fields_ = [("load_s", C.c_double), ("analysis_s", C.c_double), ("merge_s", C.c_double),
                ("nb_samples", C.c_uint64), ("threads", C.c_int)]


_mt = None


def run_mt(replay_path: str, raw_path: str | None = None, threads: int = 16, levels: bool = True) -> dict:
    """Analyse a replay with `threads` host threads (bit-exact with run());
    returns the timings: load, parallel analysis, merge."""
    global _mt
    if _mt is None:
        so = os.path.join(SO_DIR, "liboracle_mt.so")
        if not os.path.exists(so):
            build()
        _mt = C.CDLL(so)
        _mt.nmo_mt_run.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(_MtTiming)]
        _mt.nmo_mt_run.restype = C.c_int
    t = _MtTiming()
    rc = _mt.nmo_mt_run(replay_path.encode(), raw_path.encode() if raw_path else None, threads, int(levels),
                        C.byref(t))
    if rc:
        raise RuntimeError(f"multi-threaded restatement failed ({rc})")
    return {"load_s": t.load_s, "analysis_s": t.analysis_s, "merge_s": t.merge_s, "nb_samples": t.nb_samples,
            "threads": t.threads}
