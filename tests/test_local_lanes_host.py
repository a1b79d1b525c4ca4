"""The replays of local_lane_cases.py have the shapes they claim (CPU only).

test_gpu_local_lanes.py runs them through local_kernel, whose common path
reads LDS for both chunks of a pair before it decides either.  What makes a
replay a test of that is its shape: how many records each partition gets
(chunk fills, odd chunk counts, a pair past the list), which directory slot a
record falls in (search depths that differ between the chunks of a pair), and
which chunk of a pair holds the rare records.  All of it follows from the
table and the records; the partition cut is local_lane_cases.partitions, the
oracle's lookup says what every record matches."""
import numpy as np
import pytest

import local_lane_cases as lc
import route_layout_cases as rc


def _lookup(rp):
    rows = lc.rows_of(rp)
    return rc.lookup_all(rp.table, rows[:, 0], rows[:, 1]), rows


def test_tables_and_partitions():
    for cfg in (lc.DENSE_CFG, lc.WIDE_CFG):
        rp = lc.base(cfg)
        assert 1100 <= cfg.nb_intervals <= 3000 and rp.nb_records() <= 60_000
        parts = lc.partitions(rp.table, rp.nb_threads)
        assert len(parts) >= 3 and sum(nk for _, nk in parts) == rp.table.nb_keys
        assert all(nk <= lc.PART_KEYS for _, nk in parts)
    t = lc.lone_key_table(lc.base(lc.DENSE_CFG).table)
    parts = lc.partitions(t, 2)
    assert parts[-1][1] == 1 and int(t.keys[-1]) - int(t.keys[-2]) >= 1 << (lc.ADDR_BITS - 1)


def test_stale_pair_shape():
    a, b = lc.stale_pair()
    na, parts = lc.counts_per_partition(a)
    nb, _ = lc.counts_per_partition(b)
    assert b.nb_records() == 5000 and len(b.buffers) == 1
    # B needs fewer chunks than A left behind in every partition, and ends at least one of them partly filled
    assert (nb < na).all() and (nb > 0).all() and (nb % lc.CHUNK != 0).any()
    ra, rb = lc.rows_of(a), lc.rows_of(b)
    # other addresses and dates: no record of B is a record of A, no date of B occurs in A, and most of B's
    # addresses do not (hot objects are sampled by both streams)
    both = set(map(tuple, ra[:, :2].tolist()))
    assert not any(tuple(r) in both for r in rb[:, :2].tolist())
    assert not np.isin(rb[:, 1], ra[:, 1]).any()
    assert np.isin(rb[:, 0], ra[:, 0]).mean() < 0.5
    m, _ = _lookup(b)
    assert (m >= 0).sum() > 2000 and (m < 0).sum() > 100


@pytest.mark.parametrize("which", [0, 1, 2])
def test_fills_shape(which):
    rp, want = lc.fills_case(which)
    n, parts = lc.counts_per_partition(rp)
    assert tuple(n) == want and len(rp.buffers) == 1
    m, _ = _lookup(rp)
    assert (m >= 0).all()
    chunks = [-(-c // lc.CHUNK) for c in want if c]
    if which == 0:
        assert chunks == [1, 1, 1]            # one-chunk items: the pair's second chunk is past the list
    elif which == 1:
        assert chunks == [2, 2, 2]            # 65 and 127: a second chunk with 1 and 63 records
    else:
        assert chunks == [3, 1, 1, 1]         # an odd chunk count; the lone key's partition gets one record


def test_all_fills_covered():
    got = set()
    for which in (0, 1, 2):
        got |= set(lc.fills_case(which)[1])
    assert got >= set(lc.FILLS)


@pytest.mark.parametrize("kind", ["inline", "wide"])
def test_directory_depths(kind):
    rp, part, (j, lo, n) = lc.directory_case(kind)
    t = rp.table
    chunks, parts = lc.chunks_of(rp)
    q = parts.index(part)
    assert list(chunks) == [q] and [c.shape[0] for c in chunks[q]] == [64, 64]
    deep = [lc.search_depth(t, part, a) for a in chunks[q][0][:, 0]]
    shallow = [lc.search_depth(t, part, a) for a in chunks[q][1][:, 0]]
    assert n > lc.DIR_INLINE and min(deep) >= 1 and max(shallow) == 0
    _, _, inl = lc.dir_slot(t, part, j)
    if kind == "inline":
        assert inl and lc.dshift_of(t, part) <= 16
        assert all(lc.slot_of(t, part, a) == j for a in chunks[q][0][:, 0][:8])
    else:
        # offsets inside the slot need more than 16 bits: the slot is not inline, all n keys are searched
        assert not inl and lc.dshift_of(t, part) > 16 and min(deep) == n
    m, _ = _lookup(rp)
    assert (m >= 0).all()


def test_lone_key_partition():
    rp, part, _ = lc.directory_case("lone")
    n, parts = lc.counts_per_partition(rp)
    assert part == parts[-1] and part[1] == 1 and n[-1] == 128 and n[-2] == 5
    assert lc.dshift_of(rp.table, part) == 0
    m, _ = _lookup(rp)
    assert (m >= 0).all()


@pytest.mark.parametrize("first", [True, False])
def test_rare_kinds_one_sided(first):
    rp, parts = lc.rare_case(first)
    t = rp.table
    chunks, allparts = lc.chunks_of(rp)
    assert sorted(chunks) == [0, 1, 2]
    off = t.entry_off.astype(np.int64)
    for q in range(3):
        assert [c.shape[0] for c in chunks[q]] == [64, 64]
        rare, plain = (chunks[q][0], chunks[q][1]) if first else (chunks[q][1], chunks[q][0])
        mr = rc.lookup_all(t, rare[:, 0], rare[:, 1])
        mp = rc.lookup_all(t, plain[:, 0], plain[:, 1])
        k = lc.part_keys_of(t, plain[:, 0])
        assert (mp == off[k]).all() and (plain[:, 2] < lc.WESC).all()   # plain: the key's newest entry, no escape
        if q == 0:
            assert (rare[:, 2] >= lc.WESC).all() and (mr >= 0).all()
        elif q == 1:
            kr = lc.part_keys_of(t, rare[:, 0])
            assert (mr > off[kr]).all() and (mr < off[kr + 1]).all()        # an older entry of the key
        else:
            assert (mr < 0).all() and (rare[:, 2] < lc.WESC).all()
