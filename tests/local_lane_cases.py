"""Replays for the local pass's paired common path (nmg_route.hip,
local_kernel::process; shared by test_local_lanes_host.py and
test_gpu_local_lanes.py; not a test module).

local_kernel works on two consecutive chunks of a partition's list at a time
and reads LDS for both before it decides either: a lane without a record (a
partly filled chunk, a pair whose second chunk is past the list) reads slot 0
and must count nothing.  The builders here craft small record streams whose
chunks have the shapes where that can go wrong.  Every replay is one buffer
(one route workgroup: a partition's records fill its chunks in buffer order)
over a table of 1,100 to 3,000 intervals.

Nothing here calls the engine.  The partition cut and the per-partition
directory are restated from cut_partitions and build_part_dir
(numamma_amd/csrc/nmg_table_build.h), for tables whose page cells can never
cut a partition (asserted by `partitions`); test_table_build_host.py holds the
restatement against what those builders make."""
import copy
import dataclasses

import numpy as np

from numamma_amd.replay import RECORD_DTYPE, T0, Buffer, Replay, SynthConfig, generate

CHUNK = 64            # kChunk
PART_KEYS = 1023      # kPartKeys
PART_ENTRIES = 1536   # kPartEntries
PART_CELLS = 28672    # kPartCells
PART_DIR = 1024       # kPartDir
DIR_INLINE = 6        # kDirInline
ADDR_BITS = 40        # kAddrBits
PAGE = 4096
WESC = 65535          # wbits 16: the escape mark of these replays' compact records
FILLS = (1, 63, 64, 65, 127, 128, 129)

# heap keys back to back: a partition's keys span ~12 MiB, directory slots of 16 KiB, inline offsets
DENSE_CFG = SynthConfig(nb_samples=40_000, nb_intervals=3_000, nb_threads=2, size_max=16384, reuse_frac=0.1,
                        with_stack=False, seed=211)
# the same heap in six runs 256 MiB apart: a partition spans two gaps, slots of 512 KiB hold tens of keys at
# offsets past 2^16 (not inline: the whole slot is searched)
WIDE_CFG = dataclasses.replace(DENSE_CFG, nb_intervals=2_400, heap_clusters=6, cluster_gap=1 << 28, seed=212)
LONE_LIFT = 1 << 40   # the last key moved this far up: a partition of one key

_BASE = {}


def base(cfg):
    key = dataclasses.astuple(cfg)
    if key not in _BASE:
        _BASE[key] = generate(cfg)
    return _BASE[key]


def lone_key_table(table):
    """A copy of `table` whose last key (and its entries) lies LONE_LIFT higher:
    more than 2^(kAddrBits - 1) above every other key, so it is a partition of its own."""
    t = copy.deepcopy(table)
    k = t.nb_keys - 1
    e0, e1 = int(t.entry_off[k]), int(t.entry_off[k + 1])
    t.keys[k] += np.uint64(LONE_LIFT)
    t.entries["buffer_addr"][e0:e1] += np.uint64(LONE_LIFT)
    t.validate()
    return t


def partitions(table, T):
    """[(k0, nk)] as build_partitions cuts an offline table: at most PART_KEYS
    keys and PART_ENTRIES entries, a key span below 2^(ADDR_BITS - 1).  The
    fourth rule (dense page cells x threads <= PART_CELLS) is shown not to
    apply: no run of keys the other rules allow can own that many pages."""
    keys, off = table.keys.astype(np.uint64), table.entry_off.astype(np.int64)
    size = table.entries["buffer_size"].astype(np.int64)
    out, k, K = [], 0, keys.shape[0]
    while k < K:
        k0 = k
        while k < K and k - k0 < PART_KEYS:
            if k > k0 and int(keys[k]) - int(keys[k0]) >= 1 << (ADDR_BITS - 1):
                break
            if off[k + 1] - off[k0] > PART_ENTRIES:
                assert k > k0
                break
            k += 1
        pages = int(((size[off[k0]:off[k]] + PAGE - 1) // PAGE + 1).sum())  # (+ 1: an object across a page edge)
        assert pages * T <= PART_CELLS, "the page-cell rule could cut this partition"
        out.append((k0, k - k0))
    return out


def part_of(table, parts, addr):
    """Partition of each address: the last one starting at or before it."""
    starts = np.array([int(table.keys[k0]) for k0, _ in parts], dtype=np.uint64)
    return np.searchsorted(starts, np.asarray(addr, dtype=np.uint64), side="right") - 1


def dshift_of(table, part):
    k0, nk = part
    span, sh = int(table.keys[k0 + nk - 1]) - int(table.keys[k0]), 0
    while sh < 63 and (span >> sh) >= PART_DIR:
        sh += 1
    return sh


def dir_slot(table, part, j):
    """(lo, n, inline) of directory slot j of a partition (PartDir)."""
    k0, nk = part
    sh = dshift_of(table, part)
    rel = (table.keys[k0:k0 + nk] - table.keys[k0]).astype(np.uint64)
    s0 = j << sh
    lo = max(int(np.searchsorted(rel, s0, side="right")) - 1, 0)
    hi = nk if j == PART_DIR - 1 else int(np.searchsorted(rel, s0 + (1 << sh), side="left"))
    n = max(hi - (lo + 1), 0)
    inline = n > 0 and all(int(rel[lo + 1 + i]) - s0 < 1 << 16 for i in range(min(n, DIR_INLINE)))
    return lo, n, inline


def slot_of(table, part, addr):
    return min((int(addr) - int(table.keys[part[0]])) >> dshift_of(table, part), PART_DIR - 1)


def search_depth(table, part, addr):
    """Keys local_kernel's lookup has left to search for addr after its directory slot (0: none read)."""
    j = slot_of(table, part, addr)
    lo, n, inline = dir_slot(table, part, j)
    if not inline:
        return n
    rel = int(addr) - int(table.keys[part[0]]) - (j << dshift_of(table, part))
    c = sum(1 for i in range(min(n, DIR_INLINE)) if int(table.keys[part[0] + lo + 1 + i]) - int(table.keys[part[0]])
            - (j << dshift_of(table, part)) <= rel)
    return n - DIR_INLINE if c == DIR_INLINE and n > DIR_INLINE else 0


# ---- records

def _proto(rp):
    return rp.buffers[0].linear().view(RECORD_DTYPE)[0].copy()


def hits(table, e, n, rng, weight=None):
    """n (addr, ts, weight) rows inside entry e, its dates more than two quanta from either bound."""
    ent = table.entries[e]
    a, s, al, fr = (int(ent[f]) for f in ("buffer_addr", "buffer_size", "alloc_date", "free_date"))
    al = max(al, T0)  # (a global's alloc_date is 0: stay inside the compact record's time field)
    assert s >= 1 and fr - al > 4096
    addr = a + rng.integers(0, s, n)
    ts = rng.integers(al + 1024, fr - 1024, n)
    w = rng.integers(1, 200, n) if weight is None else np.full(n, weight)
    return np.stack([addr, ts, w], axis=1).astype(np.uint64)


def newest(table, k):
    return int(table.entry_off[k])


def plain_keys(table, part):
    """The partition's keys whose newest entry starts at the key and ends before the next key (no realloc'd
    object reaching into its neighbour), heap objects only."""
    k0, nk = part
    ks = np.arange(k0, k0 + nk)
    e = table.entry_off[ks].astype(np.int64)
    ent = table.entries
    nxt = np.append(table.keys[1:], np.uint64(1 << 63))[ks]
    ok = (ent["buffer_addr"][e] == table.keys[ks]) & (ent["buffer_addr"][e] + ent["buffer_size"][e] <= nxt) \
        & (ent["alloc_date"][e] >= T0)
    return ks[ok]


def one_buffer(rp, table, rows):
    """A replay of one buffer (thread 1, reads) holding the rows as SAMPLE records."""
    rows = np.asarray(rows, dtype=np.uint64)
    rec = np.zeros(rows.shape[0], dtype=RECORD_DTYPE)
    rec[:] = _proto(rp)
    rec["addr"], rec["timestamp"], rec["weight"] = rows[:, 0], rows[:, 1], rows[:, 2]
    raw = rec.view(np.uint8).copy()
    return Replay(rp.nb_threads, table, [Buffer(1, 0, raw, 0, raw.shape[0])], dict(rp.meta))


def rows_of(rp):
    rec = np.concatenate([b.linear() for b in rp.buffers]).view(RECORD_DTYPE)
    return np.stack([rec["addr"], rec["timestamp"], rec["weight"]], axis=1).astype(np.uint64)


def counts_per_partition(rp, T=None):
    parts = partitions(rp.table, rp.nb_threads if T is None else T)
    q = part_of(rp.table, parts, rows_of(rp)[:, 0])
    assert (q >= 0).all()
    return np.bincount(q, minlength=len(parts)), parts


# ---- the cases

def stale_pair():
    """(A, B): A is DENSE_CFG's own replay; B is 5,000 records of another sample
    stream over the same table, in one buffer."""
    a = base(DENSE_CFG)
    other = base(dataclasses.replace(DENSE_CFG, sample_seed=977))
    assert np.array_equal(other.table.entries, a.table.entries)
    b = one_buffer(a, a.table, rows_of(other)[:5000])
    return a, b


def fills_case(which):
    """Partitions of the lone-key table receiving FILLS[3 * which ...] records
    from one buffer, hits on keys spread over each partition (the last case's
    third partition is the lone key: one record)."""
    rp = base(DENSE_CFG)
    t = lone_key_table(rp.table)
    parts = partitions(t, rp.nb_threads)
    assert len(parts) == 4 and parts[-1][1] == 1
    want = {0: (1, 63, 64, 0), 1: (65, 127, 128, 0), 2: (129, 64, 63, 1)}[which]
    rng = np.random.default_rng(500 + which)
    blocks = []
    for (k0, nk), n in zip(parts, want):
        if n:
            ks = rng.choice(plain_keys(t, (k0, nk)), n)
            blocks.append(np.concatenate([hits(t, newest(t, int(k)), 1, rng) for k in ks]))
    rows = np.concatenate(blocks)
    return one_buffer(rp, t, rows[rng.permutation(rows.shape[0])]), want


def _deep_slot(table, part, inline):
    """A directory slot with more than DIR_INLINE keys: (slot, lo, n)."""
    for j in range(PART_DIR):
        lo, n, inl = dir_slot(table, part, j)
        if n > DIR_INLINE and inl == inline:
            return j, lo, n
    raise AssertionError("no such slot")


def directory_case(kind):
    """128 records for one partition, in buffer order 64 then 64:
    'inline': the first 64 in a slot with more than DIR_INLINE inline keys, past the sixth (the key search
              runs), the other 64 on keys whose slot lists them (no search);
    'wide':   WIDE_CFG's table, the first 64 in a slot whose offsets do not fit 16 bits (the whole slot is
              searched), the other 64 on a slot's first keys;
    'lone':   the lone key's partition: 64 + 64 hits on its only key, and 5 on the partition before it."""
    rng = np.random.default_rng({"inline": 1, "wide": 2, "lone": 3}[kind])
    if kind == "lone":
        rp = base(DENSE_CFG)
        t = lone_key_table(rp.table)
        parts = partitions(t, rp.nb_threads)
        k = parts[-1][0]
        rows = np.concatenate([hits(t, newest(t, k), 128, rng), hits(t, newest(t, parts[-2][0] + 7), 5, rng)])
        return one_buffer(rp, t, rows), parts[-1], None
    rp = base(DENSE_CFG if kind == "inline" else WIDE_CFG)
    t = rp.table
    parts = partitions(t, rp.nb_threads)
    part = parts[1]
    j, lo, n = _deep_slot(t, part, inline=(kind == "inline"))
    deep_keys = [part[0] + lo + 1 + i for i in range(DIR_INLINE, n)]   # past the listed ones
    deep = np.concatenate([hits(t, newest(t, deep_keys[i % len(deep_keys)]), 1, rng) for i in range(64)])
    shallow_keys = [k for k in range(part[0], part[0] + part[1])
                    if search_depth(t, part, int(t.entries["buffer_addr"][newest(t, k)])) == 0
                    and t.entries["buffer_addr"][newest(t, k)] == t.keys[k]][:40]
    shallow = []
    while len(shallow) < 64:   # (addresses anywhere in the object may fall in a deeper slot: keep the shallow ones)
        k = shallow_keys[len(shallow) % len(shallow_keys)]
        r = hits(t, newest(t, k), 1, rng)
        r[0, 0] = t.keys[k]
        shallow.append(r)
    return one_buffer(rp, t, np.concatenate([deep] + shallow)), part, (j, lo, n)


def rare_case(first):
    """Three partitions, 128 records each, in buffer order 64 then 64: one half
    plain hits, the other half (the first 64 when `first`) of one rare kind --
    partition 0: escaped records (weight >= WESC); partition 1: matches of an
    older entry of a reused key; partition 2: records in the gap past an
    object's end (no match)."""
    rp = base(DENSE_CFG)
    t = rp.table
    parts = partitions(t, rp.nb_threads)[:3]
    rng = np.random.default_rng(700 + int(first))
    ent, off = t.entries, t.entry_off.astype(np.int64)
    blocks = []
    for q, (k0, nk) in enumerate(parts):
        ks = plain_keys(t, (k0, nk))
        plain = np.concatenate([hits(t, newest(t, int(k)), 1, rng) for k in rng.choice(ks, 64)])
        if q == 0:
            rare = np.concatenate([hits(t, newest(t, int(k)), 1, rng, weight=WESC + int(i % 3) * 5000)
                                   for i, k in enumerate(rng.choice(ks, 64))])
        elif q == 1:
            reused = ks[(off[ks + 1] - off[ks]) > 1]
            assert reused.shape[0] >= 8
            rare = np.concatenate([hits(t, newest(t, int(k)) + 1, 1, rng) for k in rng.choice(reused, 64)])
        else:
            gaps = [k for k in ks[:-1] if off[k + 1] - off[k] == 1
                    and int(ent["buffer_addr"][off[k]]) + int(ent["buffer_size"][off[k]]) + 8 < int(t.keys[k + 1])]
            assert len(gaps) >= 8
            rare = np.concatenate([hits(t, newest(t, int(k)), 1, rng) for k in rng.choice(gaps, 64)])
            e = np.array([newest(t, int(k)) for k in part_keys_of(t, rare[:, 0])])
            rare[:, 0] = ent["buffer_addr"][e] + ent["buffer_size"][e] + np.uint64(4)  # past the end, before the next key
        blocks.append(np.concatenate([rare, plain] if first else [plain, rare]))
    return one_buffer(rp, t, np.concatenate(blocks)), parts


def part_keys_of(table, addr):
    """Key index of the largest key <= each address."""
    return np.searchsorted(table.keys, np.asarray(addr, dtype=np.uint64), side="right") - 1


def chunks_of(rp):
    """Per partition, the rows of each chunk its records fill from this one-buffer replay, in list order."""
    rows = rows_of(rp)
    parts = partitions(rp.table, rp.nb_threads)
    q = part_of(rp.table, parts, rows[:, 0])
    out = {}
    for p in np.unique(q):
        r = rows[q == p]
        out[int(p)] = [r[i:i + CHUNK] for i in range(0, r.shape[0], CHUNK)]
    return out, parts
