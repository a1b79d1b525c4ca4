"""The host pieces of the cost / timeline merge (no GPU): merge_sparse_u64,
the digest of the product options the ranks compare, the C-ABI's new names."""
import numpy as np

from numamma_amd import _lib
from numamma_amd.distributed import merge_sparse, merge_sparse_u64, options_digest

U = np.uint64


def test_abi_names():
    declared = _lib.declared_symbols()
    for name in ("nmg_cells_pack", "nmg_cells_unpack_add", "nmg_sparse_count_ex", "nmg_sparse_export_ex",
                 "nmg_sparse_import_ex"):
        assert name in declared and hasattr(_lib.lib, name)
    assert (_lib.NMG_ARR_COST64, _lib.NMG_ARR_TL32) == (4, 5)
    assert (_lib.NMG_SPARSE_PAGE_COUNTS, _lib.NMG_SPARSE_PAGE_COST, _lib.NMG_SPARSE_TIMELINE) == (0, 1, 2)
    header = open(_lib.HEADER_PATH).read()
    for line in ("#define NMG_ARR_COST64 4", "#define NMG_ARR_TL32 5", "#define NMG_SPARSE_PAGE_COUNTS 0",
                 "#define NMG_SPARSE_PAGE_COST 1", "#define NMG_SPARSE_TIMELINE 2"):
        assert line in header
    # a null handle is refused by every new entry point
    n = _lib.C.c_uint64(7)
    assert _lib.lib.nmg_cells_pack(None, _lib.NMG_ARR_COST64, None, 0, _lib.C.byref(n)) == -1
    assert _lib.lib.nmg_cells_unpack_add(None, _lib.NMG_ARR_TL32, None, 0) == -1
    assert _lib.lib.nmg_sparse_count_ex(None, 0) == -1
    assert _lib.lib.nmg_sparse_export_ex(None, 1, None, None, 0) == -1
    assert _lib.lib.nmg_sparse_import_ex(None, 2, None, None, 0) == -1
    assert _lib.lib.nmg_array_size(None, _lib.NMG_ARR_COST64) == 0


def test_merge_sparse_u64_keeps_sums_above_32_bits():
    big = (U(1) << U(32)) - U(1)
    a = (np.array([7, 3, 1 << 60], dtype=U), np.array([big, 5, 1 << 40], dtype=U))
    b = (np.array([3, 7, 9], dtype=U), np.array([6, big, 2], dtype=U))
    k, v = merge_sparse_u64([a, b])
    assert k.dtype == U and v.dtype == U
    assert k.tolist() == [3, 7, 9, 1 << 60]  # unique, ascending
    assert v.tolist() == [11, 2 * int(big), 2, 1 << 40]
    # merge_sparse stays as it is: its sums wrap to 32 bits
    k32, v32 = merge_sparse([(a[0][:2], a[1][:2].astype(np.uint32)), (b[0], b[1].astype(np.uint32))])
    assert k32.tolist() == [3, 7, 9] and v32.dtype == np.uint32 and v32.tolist() == [11, (2 * int(big)) & 0xFFFFFFFF, 2]


def test_merge_sparse_u64_empty_parts():
    e = (np.zeros(0, dtype=U), np.zeros(0, dtype=U))
    for parts in ([], [e], [e, e]):
        k, v = merge_sparse_u64(parts)
        assert k.dtype == U and v.dtype == U and k.shape == v.shape == (0,)
    a = (np.array([4, 2], dtype=U), np.array([1, 1 << 50], dtype=U))
    k, v = merge_sparse_u64([e, a, e])
    assert k.tolist() == [2, 4] and v.tolist() == [1 << 50, 1]
    k, v = merge_sparse_u64([a, (a[0].astype(np.int64), a[1].astype(np.uint32))])  # (other integer types are widened)
    assert k.dtype == U and v.tolist() == [1 << 50, 2]


TL = dict(t0=1 << 40, bin_shift=29, nb_bins=12, row_shift=0, min_object_bytes=4096, budget_bytes=0, scope=1)
COST = dict(bucket_mask=0x70, access_mask=3, metric=1, budget_bytes=0, scope=1)


def test_options_digest():
    d = options_digest(TL, COST)
    assert isinstance(d, int) and 0 <= d < 1 << 62  # travels as a non-negative int64
    assert d == options_digest(dict(TL), dict(reversed(list(COST.items()))))  # equal options, whatever the dict order
    seen = {d}
    for base, other in ((TL, COST), (COST, TL)):
        for field in base:  # every field, the scope included
            changed = dict(base)
            changed[field] = base[field] + 1
            dd = options_digest(changed, other) if base is TL else options_digest(other, changed)
            assert dd not in seen, field
            seen.add(dd)
    for tl, cost in ((None, COST), (TL, None), (None, None)):  # a product that is not set
        dd = options_digest(tl, cost)
        assert dd not in seen
        seen.add(dd)
    # the two products do not stand in for each other
    assert options_digest(None, None) != options_digest(dict.fromkeys(TL, 0), None) != options_digest(None, dict.fromkeys(COST, 0))


def test_engine_remembers_the_options():
    """Engine keeps what set_timeline / set_page_cost were last given (None when dropped); no GPU: the
    attributes exist on the class's instances before any call."""
    import inspect

    from numamma_amd.engine import Engine

    src = inspect.getsource(Engine.__init__)
    assert "timeline_opts" in src and "page_cost_opts" in src
    for name in ("cells_pack", "cells_unpack_add", "sparse_export_ex", "sparse_import_ex"):
        assert callable(getattr(Engine, name))
