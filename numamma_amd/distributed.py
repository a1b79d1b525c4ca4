"""Multi-GPU analysis: one process per GPU, buffers sharded, counters merged
with RCCL (torch.distributed "nccl") over xGMI.

The reference analyses the `samples` list on one thread
(src/mem_sampling.c:324-342); each buffer is independent given the read-only
object table (__analyze_buffer only reads samples->thread_rank/access_type and
the table), so the analysis-ordered buffer list is split into contiguous,
byte-balanced ranges, one per rank.  Every rank carries its range's global
analysis index (seq_base) so first-match ordinals stay globally comparable.
The only exchange step is the merge of the counters:

* u64 sums (global counts/weights, per-object counts/weights/levels)  -> SUM
* u64 mins (global bucket min_weight, first-match ordinals, error word) -> MIN
* u64 maxes (global bucket max_weight)                                 -> MAX
* u32 page histogram                                                   -> SUM
  (packed, merge_hist_packed: bytes of the cells <= 255 / world summed as
  u8, the larger cells gathered as (cell, count) lists -- 98 -> ~26 MB per
  rank at 1M intervals)
* u64 page cost cells, u32 timeline cells (when set)                    -> SUM
  (packed, CellPacker: both arrays are almost all zeros, so each rank's
  non-zero cells travel as (cell, value) pairs and the root adds them)
* sparse page cells, per-buffer counts: variable length -> gathered to the root
* sparse cost cells, the timeline sparse table (when set): (key, value) pairs
  gathered, summed by key and imported after the sparse page cells

RCCL reduces int64, not uint64: sums are bit-identical under two's
complement; MIN/MAX use the order-preserving map x ^ 2^63.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from .results import CW_ROWS, GLOBAL_SUM_WORDS, min64_words, sum64_words  # the counter arrays' layout

INT64_MIN = -(1 << 63)


def shard_ranges(lengths: Sequence[int], world: int) -> List[Tuple[int, int]]:
    """Contiguous [lo, hi) buffer ranges with balanced byte counts."""
    lengths = np.asarray(lengths, dtype=np.int64)
    n = lengths.shape[0]
    if world <= 1 or n == 0:
        return [(0, n)] + [(n, n)] * max(0, world - 1)
    csum = np.concatenate([[0], np.cumsum(lengths)])
    total = csum[-1]
    cuts = [0]
    for r in range(1, world):
        target = total * r / world
        c = int(np.searchsorted(csum, target, side="left"))
        cuts.append(min(max(c, cuts[-1]), n))
    cuts.append(n)
    return [(cuts[r], cuts[r + 1]) for r in range(world)]


def _collective(t, rop, dst, group):
    """reduce / all_reduce; a device tensor goes through host memory when the
    backend is not RCCL (gloo test runs)."""
    import torch.distributed as dist

    staged = t.is_cuda and dist.get_backend(group) != "nccl"
    x = t.cpu() if staged else t
    if dst is None:
        dist.all_reduce(x, op=rop, group=group)
    else:
        dist.reduce(x, dst=dst, op=rop, group=group)
    if staged:
        t.copy_(x)
    return t


def reduce_u64(t, op: str, dst: Optional[int] = 0, group=None):
    """Reduce a tensor of u64 bit patterns stored as int64.  dst=None -> all-reduce."""
    import torch
    import torch.distributed as dist

    assert t.dtype == torch.int64
    flip = op in ("min", "max")
    if flip:
        t.bitwise_xor_(INT64_MIN)
    rop = {"sum": dist.ReduceOp.SUM, "min": dist.ReduceOp.MIN, "max": dist.ReduceOp.MAX}[op]
    _collective(t, rop, dst, group)
    if flip:
        t.bitwise_xor_(INT64_MIN)
    return t


def reduce_u32_sum(t, dst: Optional[int] = 0, group=None):
    import torch
    import torch.distributed as dist

    assert t.dtype == torch.int32
    return _collective(t, dist.ReduceOp.SUM, dst, group)


class HistPacker:
    """Buffers of the packed page-histogram merge of one engine (allocated
    once; the overflow list holds up to `ovf_frac` of the cells)."""

    def __init__(self, eng, device, ovf_frac: float = 0.125):
        import torch

        from . import _lib

        self.eng = eng
        self.cells = eng.array_size(_lib.NMG_ARR_HIST32)
        self.cap = max(1024, int(self.cells * ovf_frac))
        self.u8 = torch.empty(max(self.cells, 4), dtype=torch.uint8, device=device)
        # (empty, not zeros: a fill on torch's stream is not ordered with
        # nmg_hist_pack, which writes entries [0, n) on the engine's own
        # non-blocking stream; merge() zeroes the padding [n, nmax) itself)
        self.ovf = torch.empty(self.cap, dtype=torch.int64, device=device)
        self.n = torch.zeros(1, dtype=torch.int64, device=device)
        self.dense = None  # fallback: the u32 histogram (a list longer than cap)

    def merge(self, dst: int = 0, group=None) -> int:
        """Merge every rank's histogram into rank dst's engine; returns the
        bytes this rank contributed to the collectives."""
        import torch
        import torch.distributed as dist

        from . import _lib

        if not self.cells:
            return 0
        world = dist.get_world_size(group)
        rank = dist.get_rank(group)
        thr = 255 // world
        n = self.eng.hist_pack(thr, self.u8.data_ptr(), self.ovf.data_ptr(), self.cap)
        self.n.fill_(n)
        _collective(self.n, dist.ReduceOp.MAX, None, group)  # every rank: the longest list
        nmax = int(self.n.item())
        if nmax > self.cap:  # some list does not fit: the plain u32 reduce
            if self.dense is None:
                self.dense = torch.empty(self.cells, dtype=torch.int32, device=self.u8.device)
            self.eng.export_array(_lib.NMG_ARR_HIST32, self.dense.data_ptr())
            reduce_u32_sum(self.dense, dst=dst, group=group)
            if rank == dst:
                torch.cuda.synchronize(self.u8.device)
                self.eng.import_array(_lib.NMG_ARR_HIST32, self.dense.data_ptr())
            return self.cells * 4
        if n < nmax:
            self.ovf[n:nmax].zero_()  # (padding: count 0)
        _collective(self.u8[:self.cells], dist.ReduceOp.SUM, dst, group)
        part = self.ovf[:nmax]
        if dist.get_backend(group) == "nccl":
            out = [torch.empty_like(part) for _ in range(world)] if rank == dst else None
            dist.gather(part, out, dst=dst, group=group)
        else:  # (gloo test runs: host staging)
            cpu = part.cpu()
            out = [torch.empty_like(cpu) for _ in range(world)] if rank == dst else None
            dist.gather(cpu, out, dst=dst, group=group)
        if rank == dst:
            allovf = torch.cat([o.to(self.u8.device) for o in out]) if nmax else self.ovf[:0]
            torch.cuda.synchronize(self.u8.device)
            self.eng.hist_unpack(self.u8.data_ptr(), allovf.data_ptr() if nmax else 0, allovf.numel())
        return self.cells + nmax * 8


class ObjPacker:
    """Buffers of the packed per-object counter merge of one engine
    (nmg_objcw_pack / nmg_objcw_unpack): sum64's four count / weight rows as
    u32 words -- a value below 2^32 / world, so that the sum over the ranks
    fits -- plus a list of the larger values as (row word, value) pairs
    (allocated once; the list holds up to `ovf_frac` of the words)."""

    def __init__(self, eng, device, ovf_frac: float = 1 / 64):
        import torch

        from . import _lib

        self.eng = eng
        n = eng.array_size(_lib.NMG_ARR_SUM64)
        levels = bool(eng.flags & _lib.NMG_F_OBJECT_LEVELS)
        # the entry count from min64's size, checked against sum64's: a layout
        # change in nmg_internal.h that results.py misses fails here, not silently
        self.E = eng.array_size(_lib.NMG_ARR_MIN64) - min64_words(0) if n else 0
        if n and sum64_words(self.E, levels) != n:
            raise RuntimeError(f"ObjPacker: sum64 holds {n} words, not the {sum64_words(self.E, levels)} of "
                               f"{self.E} entries")
        self.n_sum64 = n  # the engine's sum64 size this packer was built for
        self.levels = levels
        self.rows = CW_ROWS * self.E
        self.cap = max(1024, int(self.rows * ovf_frac))
        self.u32 = torch.empty(max(self.rows, 1), dtype=torch.int32, device=device)
        self.ovf = torch.empty(2 * self.cap, dtype=torch.int64, device=device)
        self.n = torch.zeros(1, dtype=torch.int64, device=device)

    def merge(self, t, dst: int = 0, group=None):
        """The rows of the sum64 image t (every rank's) summed into rank dst's
        t; returns the bytes this rank contributed, or None when some rank's
        list outgrew its buffer (the caller reduces the rows as u64)."""
        import torch
        import torch.distributed as dist

        world = dist.get_world_size(group)
        rank = dist.get_rank(group)
        thr = (1 << 32) // world
        n = self.eng.objcw_pack(t.data_ptr(), thr, self.u32.data_ptr(), self.ovf.data_ptr(), self.cap)
        self.n.fill_(n)
        _collective(self.n, dist.ReduceOp.MAX, None, group)
        nmax = int(self.n.item())
        if nmax > self.cap:
            return None
        if n < nmax:
            self.ovf[2 * n:2 * nmax].zero_()  # (padding: row word 0 += 0)
        _collective(self.u32[:self.rows], dist.ReduceOp.SUM, dst, group)  # (u32 sums as int32: the same bits)
        part = self.ovf[:2 * nmax]
        if dist.get_backend(group) == "nccl":
            out = [torch.empty_like(part) for _ in range(world)] if rank == dst else None
            dist.gather(part, out, dst=dst, group=group)
        else:  # (gloo test runs: host staging)
            cpu = part.cpu()
            out = [torch.empty_like(cpu) for _ in range(world)] if rank == dst else None
            dist.gather(cpu, out, dst=dst, group=group)
        if rank == dst:
            allovf = torch.cat([o.to(self.u32.device) for o in out]) if nmax else self.ovf[:0]
            torch.cuda.synchronize(self.u32.device)
            self.eng.objcw_unpack(t.data_ptr(), self.u32.data_ptr(), allovf.data_ptr() if nmax else 0,
                                  allovf.numel() // 2)
        return self.rows * 4 + nmax * 16


def gather_arrays(a: np.ndarray, dst: int = 0, group=None):
    """Variable-length gather of a numpy array; returns the list on dst."""
    import torch.distributed as dist

    world = dist.get_world_size(group)
    out = [None] * world if dist.get_rank(group) == dst else None
    dist.gather_object(a, out, dst=dst, group=group)
    return out


def merge_sparse(parts) -> Tuple[np.ndarray, np.ndarray]:
    keys = np.concatenate([p[0] for p in parts]) if parts else np.zeros(0, np.uint64)
    vals = np.concatenate([p[1] for p in parts]) if parts else np.zeros(0, np.uint32)
    if keys.shape[0] == 0:
        return keys.astype(np.uint64), vals.astype(np.uint32)
    u, inv = np.unique(keys, return_inverse=True)
    s = np.zeros(u.shape[0], dtype=np.uint64)
    np.add.at(s, inv, vals.astype(np.uint64))
    return u, (s & 0xFFFFFFFF).astype(np.uint32)


def merge_sparse_u64(parts) -> Tuple[np.ndarray, np.ndarray]:
    """merge_sparse with the sums kept as u64 (cost sums pass 2^32): (keys,
    values) summed by key, keys ascending and unique."""
    keys = np.concatenate([np.asarray(p[0], dtype=np.uint64) for p in parts]) if parts else np.zeros(0, np.uint64)
    vals = np.concatenate([np.asarray(p[1], dtype=np.uint64) for p in parts]) if parts else np.zeros(0, np.uint64)
    if keys.shape[0] == 0:
        return keys, vals
    u, inv = np.unique(keys, return_inverse=True)
    s = np.zeros(u.shape[0], dtype=np.uint64)
    np.add.at(s, inv.reshape(-1), vals)
    return u, s


_TIMELINE_FIELDS = ("t0", "bin_shift", "nb_bins", "row_shift", "min_object_bytes", "budget_bytes", "scope")
_PAGE_COST_FIELDS = ("bucket_mask", "access_mask", "metric", "budget_bytes", "scope")


def options_digest(timeline_opts: Optional[dict], page_cost_opts: Optional[dict]) -> int:
    """A 62-bit digest of the product options an engine remembers
    (Engine.timeline_opts, Engine.page_cost_opts; None: not set): equal options
    give equal digests on every rank, a difference in any field, the scope
    included, another one.  Non-negative, so it travels as int64."""
    import hashlib

    def words(o, fields):
        return (0,) if o is None else (1,) + tuple(int(o[f]) for f in fields)

    text = repr((words(timeline_opts, _TIMELINE_FIELDS), words(page_cost_opts, _PAGE_COST_FIELDS)))
    return int.from_bytes(hashlib.blake2b(text.encode(), digest_size=8).digest(), "little") >> 2


def check_products(eng, group=None, device=None) -> Tuple[int, int]:
    """Every rank's page cost and timeline arrays must have one size and one
    set of options before they meet in a collective: (NMG_ARR_COST64 size,
    NMG_ARR_TL32 size), or RuntimeError on every rank when some rank differs (a
    rank that forgot set_page_cost would otherwise hang the job in a reduce the
    others never enter, or add cells counted by another rule)."""
    import torch
    import torch.distributed as dist

    from . import _lib

    mine = [eng.array_size(_lib.NMG_ARR_COST64), eng.array_size(_lib.NMG_ARR_TL32),
            options_digest(getattr(eng, "timeline_opts", None), getattr(eng, "page_cost_opts", None))]
    on_dev = dist.get_backend(group) == "nccl"
    lo = torch.tensor(mine, dtype=torch.int64, device=device if on_dev else "cpu")
    hi = lo.clone()
    dist.all_reduce(lo, op=dist.ReduceOp.MIN, group=group)
    dist.all_reduce(hi, op=dist.ReduceOp.MAX, group=group)
    if not torch.equal(lo, hi):
        what = [name for name, a, b in zip(("page cost cells", "timeline cells", "product options"), lo.tolist(),
                                           hi.tolist()) if a != b]
        raise RuntimeError(f"merge_engine: the ranks differ in {', '.join(what)} (this rank: {mine[0]} cost cells, "
                           f"{mine[1]} timeline cells): give every rank the same table, nb_threads, "
                           "hist_budget_bytes, set_timeline and set_page_cost")
    return mine[0], mine[1]


class CellPacker:
    """Buffers of the packed merge of one engine's page cost cells
    (NMG_ARR_COST64) or timeline cells (NMG_ARR_TL32): the non-zero cells as
    (cell index, value) pairs (nmg_cells_pack), gathered and added on the root
    (nmg_cells_unpack_add).  Allocated once; the list holds up to `frac` of
    the cells, or `cap` pairs -- a buffer size only: a longer list falls back
    to the dense reduce."""

    def __init__(self, eng, device, which: int, frac: float = 0.125, cap: Optional[int] = None):
        import torch

        from . import _lib

        assert which in (_lib.NMG_ARR_COST64, _lib.NMG_ARR_TL32)
        self.eng = eng
        self.which = which
        self.cells = eng.array_size(which)
        self.cap = int(cap) if cap is not None else max(1024, int(self.cells * frac))
        # (empty: nmg_cells_pack writes pairs [0, n) on the engine's stream; merge() zeroes the padding)
        self.list = torch.empty(2 * max(self.cap, 1), dtype=torch.int64, device=device)
        self.n = torch.zeros(1, dtype=torch.int64, device=device)
        self.dense = None  # fallback: the array itself (a list longer than cap)
        self.last = (0, 0)  # (packed list bytes, dense array bytes) of the last merge

    def merge_dense(self, dst: int = 0, group=None) -> int:
        """The array itself reduced into rank dst's engine; returns its bytes."""
        import torch
        import torch.distributed as dist

        from . import _lib

        if not self.cells:
            return 0
        u64 = self.which == _lib.NMG_ARR_COST64
        if self.dense is None:
            self.dense = torch.empty(self.cells, dtype=torch.int64 if u64 else torch.int32, device=self.list.device)
        self.eng.export_array(self.which, self.dense.data_ptr())
        if u64:
            reduce_u64(self.dense, "sum", dst=dst, group=group)
        else:
            reduce_u32_sum(self.dense, dst=dst, group=group)
        if dist.get_rank(group) == dst:
            torch.cuda.synchronize(self.list.device)
            self.eng.import_array(self.which, self.dense.data_ptr())
        return self.cells * (8 if u64 else 4)

    def merge(self, dst: int = 0, group=None) -> int:
        """Merge every rank's cells into rank dst's engine; returns the bytes
        this rank contributed to the collectives."""
        import torch
        import torch.distributed as dist

        from . import _lib

        if not self.cells:
            return 0
        world = dist.get_world_size(group)
        rank = dist.get_rank(group)
        dense_bytes = self.cells * (8 if self.which == _lib.NMG_ARR_COST64 else 4)
        n = self.eng.cells_pack(self.which, self.list.data_ptr(), self.cap)
        self.n.fill_(n)
        _collective(self.n, dist.ReduceOp.MAX, None, group)  # every rank: the longest list
        nmax = int(self.n.item())
        self.last = (n * 16, dense_bytes)
        if nmax > self.cap:  # some list does not fit: the array itself
            return self.merge_dense(dst=dst, group=group)
        if n < nmax:
            self.list[2 * n:2 * nmax].zero_()  # (padding: value 0)
        part = self.list[:2 * nmax]
        if dist.get_backend(group) == "nccl":
            out = [torch.empty_like(part) for _ in range(world)] if rank == dst else None
            dist.gather(part, out, dst=dst, group=group)
        else:  # (gloo test runs: host staging)
            cpu = part.cpu()
            out = [torch.empty_like(cpu) for _ in range(world)] if rank == dst else None
            dist.gather(cpu, out, dst=dst, group=group)
        if rank == dst and nmax and world > 1:
            # the other ranks' lists: this rank's cells are in place already
            others = torch.cat([o.to(self.list.device) for r, o in enumerate(out) if r != dst])
            torch.cuda.synchronize(self.list.device)
            self.eng.cells_unpack_add(self.which, others.data_ptr(), others.numel() // 2)
        return nmax * 16


def merge_engine(eng, dst: int = 0, group=None, device=None, packed_hist: bool = False) -> int:
    """Merge every rank's partial counters into rank dst's engine (RCCL reduce
    of the dense arrays over xGMI; gathers of the small variable-length ones).
    packed_hist: the page histogram through HistPacker (bytes + overflow),
    the per-object counters through ObjPacker (u32 words + overflow), and the
    page cost and timeline cells through CellPacker (their non-zero cells).
    The page cost cells and the timeline, dense and sparse, are merged when
    set -- on every rank with the same options, or RuntimeError on every rank
    (check_products).  Returns the bytes this rank contributed to the dense
    collectives and to the gathers of the cost and timeline cells."""
    import torch
    import torch.distributed as dist

    from . import _lib

    rank = dist.get_rank(group)
    dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    n_cost, n_tl = check_products(eng, group=group, device=dev)  # (before anything is merged)
    nbytes = 0
    for which, op in ((_lib.NMG_ARR_SUM64, "sum"), (_lib.NMG_ARR_MIN64, "min"), (_lib.NMG_ARR_MAX64, "max")):
        n = eng.array_size(which)
        if n == 0:
            continue
        t = torch.empty(n, dtype=torch.int64, device=dev)
        eng.export_array(which, t.data_ptr())
        got = None
        if packed_hist and which == _lib.NMG_ARR_SUM64:  # the per-object rows as u32 + a list
            op_ = getattr(eng, "_obj_packer", None)  # rebuilt whenever the table's size changed
            if op_ is None or op_.n_sum64 != n or op_.levels != bool(eng.flags & _lib.NMG_F_OBJECT_LEVELS):
                op_ = eng._obj_packer = ObjPacker(eng, dev)
            got = op_.merge(t, dst=dst, group=group)
            if got is not None:
                nbytes += got
                rest = [t[:GLOBAL_SUM_WORDS]] + ([t[GLOBAL_SUM_WORDS + op_.rows:]] if n > GLOBAL_SUM_WORDS + op_.rows else [])
                for part in rest:  # the global sums (and per-object levels) as u64
                    nbytes += 8 * part.numel()
                    reduce_u64(part, "sum", dst=dst, group=group)
        if got is None:
            nbytes += 8 * n
            reduce_u64(t, op, dst=dst, group=group)
        if rank == dst:
            torch.cuda.synchronize(dev)
            eng.import_array(which, t.data_ptr())
    n = eng.array_size(_lib.NMG_ARR_HIST32)
    if n and packed_hist:
        hp = getattr(eng, "_hist_packer", None)  # one packer per engine, reused across merges
        if hp is None or hp.cells != n:
            hp = eng._hist_packer = HistPacker(eng, dev)
        nbytes += hp.merge(dst=dst, group=group)
    elif n:
        nbytes += 4 * n
        t = torch.empty(n, dtype=torch.int32, device=dev)
        eng.export_array(_lib.NMG_ARR_HIST32, t.data_ptr())
        reduce_u32_sum(t, dst=dst, group=group)
        if rank == dst:
            torch.cuda.synchronize(dev)
            eng.import_array(_lib.NMG_ARR_HIST32, t.data_ptr())
    # the page cost cells and the timeline cells: mostly zeros, so their non-zero cells (packed_hist) or the arrays
    packers = eng.__dict__.setdefault("_cell_packers", {})  # one per array and engine, reused across merges
    for which, n in ((_lib.NMG_ARR_COST64, n_cost), (_lib.NMG_ARR_TL32, n_tl)):
        if not n:
            continue
        cp = packers.get(which)
        if cp is None or cp.cells != n:
            cp = packers[which] = CellPacker(eng, dev, which)
        nbytes += cp.merge(dst=dst, group=group) if packed_hist else cp.merge_dense(dst=dst, group=group)
    kinds = [k for k, on in ((_lib.NMG_SPARSE_PAGE_COST, eng.page_cost_opts is not None),
                             (_lib.NMG_SPARSE_TIMELINE, eng.timeline_opts is not None)) if on]
    nbytes += merge_host_side(eng, dst=dst, group=group, kinds=kinds)
    return nbytes


def merge_host_side(eng, dst: int = 0, group=None, kinds: Sequence[int] = ()) -> int:
    """Sparse page cells and per-buffer counts (variable length): gathered.
    kinds: the further sparse kinds to merge (NMG_SPARSE_PAGE_COST,
    NMG_SPARSE_TIMELINE; the same on every rank), exported before the root's
    page table is rebuilt and imported after it; returns their bytes."""
    import torch.distributed as dist

    rank = dist.get_rank(group)
    k, v = eng.sparse_export()
    extra = [np.stack(eng.sparse_export_ex(kind)) for kind in kinds]
    parts = gather_arrays(np.stack([k, v.astype(np.uint64)]) if k.shape[0] else np.zeros((2, 0), np.uint64),
                          dst=dst, group=group)
    s, f = eng.buffer_counts()
    nbytes = np.asarray(eng.buffer_bytes, dtype=np.uint64)
    counts = gather_arrays(np.stack([s.astype(np.uint64), f.astype(np.uint64), nbytes]), dst=dst, group=group)
    extras = gather_arrays(extra, dst=dst, group=group) if kinds else None
    if rank == dst:
        keys, vals = merge_sparse([(p[0], p[1].astype(np.uint32)) for p in parts])
        eng.sparse_import(keys, vals)  # (zeroes the sparse cost cells: the cost import follows)
        allc = np.concatenate(counts, axis=1)
        eng.set_buffer_counts(allc[0].astype(np.uint32), allc[1].astype(np.uint32), allc[2])
        for i, kind in enumerate(kinds):
            eng.sparse_import_ex(kind, *merge_sparse_u64([(p[i][0], p[i][1]) for p in extras]))
    return sum(16 * int(e.shape[1]) for e in extra)
