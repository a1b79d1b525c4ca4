"""Replays that move the compact record's fields (nmg_route.h XLayout) and a
profile's dates across the 40-bit time field (shared by
test_route_layouts_host.py and test_gpu_route_layouts.py; not a test module).

The partition-first path packs a sample into 16 bytes whose field widths
follow the workload: gbits from the buffer count, obits from the longest
buffer, tbits from the thread count, and the weight gets what is left.  The
builders here re-cut one fixed set of 60,000 records into the buffer counts,
buffer lengths and thread counts that give each width, plant weights on both
sides of the escape mark, and stretch a profile's dates so that most of it
lies more than 2^40 ns after the table's first allocation, where the packed
node records' quantised dates saturate.  Nothing here calls the engine."""
import copy
import dataclasses

import numpy as np

from numamma_amd.replay import (PERF_RECORD_SAMPLE, RECORD_BYTES, RECORD_DTYPE, T0, Buffer, Replay, SynthConfig,
                                generate)

LAYOUT_CFG = SynthConfig(nb_samples=60_000, nb_intervals=3_000, size_max=16384, seed=131)
STRETCH_CFG = SynthConfig(nb_samples=60_000, nb_intervals=3_000, reuse_frac=0.3, reuse_depth=3, seed=9)
# the long run at 1024 threads: objects of at most five pages, as LAYOUT_CFG's
# (a partition's page cells are threads x pages)
STRETCH_NARROW_CFG = dataclasses.replace(STRETCH_CFG, size_max=16384)
FACTOR = 256
TS_BITS = 40        # kTsBits: a compact record's timestamp field, relative to tbase
Q_SHIFT = 8         # kPnQShift: the packed node records' date quantum
MIN_WEIGHT_BITS = 11  # kMinWeightBits
BIG = 1 << 20       # the long buffer: 26,214 records, 1,048,560 bytes, obits 17

# (T, nbuf, big_bytes) -> (gbits, obits, tbits, loc, wbits); wbits None: the single-pass kernel
LAYOUT_TABLE = {
    (1024, 4, 1 << 20): (2, 17, 10, 30, 16),
    (1024, 9, 1 << 20): (4, 17, 10, 32, 16),    # no slack: the thread field touches the location
    (1024, 17, 1 << 20): (5, 17, 10, 33, 15),
    (1024, 33, 1 << 20): (6, 17, 10, 34, 14),
    (1024, 65, 1 << 20): (7, 17, 10, 35, 13),
    (1024, 129, 1 << 20): (8, 17, 10, 36, 12),
    (1024, 257, 1 << 20): (9, 17, 10, 37, 11),
    (1024, 512, 1 << 20): (9, 17, 10, 37, 11),
    (1024, 513, 1 << 20): (10, 17, 10, 38, None),
    (65, 2048, 1 << 19): (11, 16, 7, 35, 13),
    (3, 5, 1 << 20): (3, 17, 2, 23, 16),
    (1, 5, 1 << 20): (3, 17, 0, 21, 16),
}


def records(rp):
    """Every buffer's records (pure 40-byte SAMPLE streams) as views."""
    return [b.ring.view(RECORD_DTYPE) for b in rp.buffers]


def tbase_of(table):
    """XLayout::tbase: the table's smallest non-zero alloc_date."""
    a = table.entries["alloc_date"]
    return int(a[a != 0].min())


def _sizes(n, parts, limit, rng):
    """n records in `parts` non-empty runs at random cut points, each shorter than limit."""
    for _ in range(1000):
        cuts = np.sort(rng.choice(np.arange(1, n), parts - 1, replace=False)) if parts > 1 else np.zeros(0, np.int64)
        sizes = np.diff(np.concatenate([[0], cuts, [n]]))
        if sizes.max() < limit:
            return sizes.tolist()
    raise AssertionError("no cut with every run shorter than the long buffer")


def recut(rp, T, nbuf, big_bytes=BIG, seed=0, split=0):
    """rp's records, in their order, as nbuf buffers of T threads' ranks: one of
    big_bytes // 40 records at a random place, the others cut at random points
    and all shorter.  Ranks cycle through {0, 1, T/2, T-2, T-1}, accesses
    through read and write.  split = k: the cut for nbuf - k buffers, then its
    k longest short buffers halved, both halves with the buffer's rank and
    access -- every record keeps its thread, so the page cells are those of
    the nbuf - k cut."""
    rec = np.concatenate([b.linear() for b in rp.buffers]).view(RECORD_DTYPE)
    assert (rec["type"] == PERF_RECORD_SAMPLE).all() and (rec["size"] == RECORD_BYTES).all()
    rng = np.random.default_rng(seed)
    nbig = big_bytes // RECORD_BYTES
    base = nbuf - split
    sizes = _sizes(rec.shape[0] - nbig, base - 1, nbig, rng)
    sizes.insert(int(rng.integers(0, base)), nbig)
    cycle = list(dict.fromkeys(min(max(r, 0), T - 1) for r in (T - 1, 0, T // 2, 1, T - 2)))  # (T - 1 first: every tbit set)
    cut = [(cycle[i % len(cycle)], i % 2, n) for i, n in enumerate(sizes)]
    for _ in range(split):
        i = max((j for j in range(len(cut)) if cut[j][2] < nbig), key=lambda j: cut[j][2])
        r, a, n = cut[i]
        cut[i:i + 1] = [(r, a, n // 2), (r, a, n - n // 2)]
    bufs, at = [], 0
    for r, a, n in cut:
        raw = rec[at:at + n].copy().view(np.uint8)
        bufs.append(Buffer(r, a, raw, 0, raw.shape[0]))
        at += n
    assert at == rec.shape[0] and len(bufs) == nbuf and max(b.ring.shape[0] for b in bufs) == nbig * RECORD_BYTES
    return Replay(T, copy.deepcopy(rp.table), bufs, dict(rp.meta))


def expected_layout(rp):
    """gbits, obits, tbits, loc, wbits, wesc, tbase as the XLayout comment of
    nmg_route.h states them; wbits and wesc None past the route limit."""
    lens = [b.linear().shape[0] for b in rp.buffers]
    lens = [n for n in lens if n]
    gbits = (len(lens) - 1).bit_length()
    obits = ((max(lens) - 1) // 8).bit_length()
    tbits = (rp.nb_threads - 1).bit_length()
    loc = gbits + obits + tbits + 1  # (the access bit)
    wbits = min(48 - loc, 16) if 48 - loc >= MIN_WEIGHT_BITS else None
    return {"gbits": gbits, "obits": obits, "tbits": tbits, "loc": loc, "wbits": wbits,
            "wesc": (1 << wbits) - 1 if wbits else None, "tbase": tbase_of(rp.table)}


def planted_values(wesc):
    """The last weight the field holds, the escape mark itself, the first past
    it, and both sides of the 16-bit edge."""
    return [wesc - 1, wesc, wesc + 1, 65535, 65536]


def plant_weights(rp, wesc, seed):
    """Five disjoint random 1 % shares of the records get the planted_values
    as their weight; returns [(value, record indices over the buffers in order)]."""
    recs = records(rp)
    n = sum(r.shape[0] for r in recs)
    share = n // 100
    perm = np.random.default_rng(seed).permutation(n)
    w = np.concatenate([r["weight"] for r in recs])
    out = []
    for i, v in enumerate(planted_values(wesc)):
        idx = np.sort(perm[i * share:(i + 1) * share])
        w[idx] = v
        out.append((v, idx))
    at = 0
    for r in recs:
        r["weight"] = w[at:at + r.shape[0]]
        at += r.shape[0]
    return out


def _map_dates(d, factor):
    d = d.astype(np.uint64)
    assert ((d == 0) | (d >= T0)).all()
    return np.where(d >= T0, np.uint64(T0) + (d - np.uint64(T0)) * np.uint64(factor), d)


def stretch(rp, factor=FACTOR):
    """A copy of rp with every date d >= T0 of the table and of the samples at
    T0 + (d - T0) * factor (no non-zero date lies below T0): the order of all
    dates is kept, so every sample matches what it matched."""
    out = Replay(rp.nb_threads, copy.deepcopy(rp.table),
                 [Buffer(b.thread_rank, b.access_type, b.linear().copy(), 0, b.linear().shape[0]) for b in rp.buffers],
                 dict(rp.meta))
    ent = out.table.entries
    ent["alloc_date"] = _map_dates(ent["alloc_date"], factor)
    ent["free_date"] = _map_dates(ent["free_date"], factor)
    for r in records(out):
        r["timestamp"] = _map_dates(r["timestamp"], factor)
    return out


def edge_probes(rp):
    """A stretched replay with twelve entries' dates on the saturation edge E =
    tbase + 2^40 and one more buffer of samples around it.

    Eight entries lie on keys with a single entry; they start at their key,
    end before the next key and live across E with 2^20 ns to spare on either
    side.  Four get free_date E - 256, E - 1, E, E + 255, four alloc_date
    E - 256, E - 1, E, E + 256 (tbase is not among them).  Four more are the
    middle entry of a reused key's chain of three (an older entry: the local
    pass's LDS list, then the chain in global memory), with free_date E - 256
    or E + 255, or alloc_date E - 256 or E + 256.  The probe buffer (thread
    0, reads) samples each one's first, middle and last byte at
    E + {-257, -256, -1, 0, 1, 255, 256} and at its rewritten date and the
    nanosecond on either side.  Returns (replay, E, [(entry, field, date)],
    probe entry of every probe record)."""
    out = Replay(rp.nb_threads, copy.deepcopy(rp.table),
                 [Buffer(b.thread_rank, b.access_type, b.linear().copy(), 0, b.linear().shape[0]) for b in rp.buffers],
                 dict(rp.meta))
    t = out.table
    ent = t.entries
    tb = tbase_of(t)
    E = tb + (1 << TS_BITS)
    eo = t.entry_off.astype(np.int64)
    single = np.flatnonzero(np.diff(eo) == 1)
    single = single[single + 1 < t.nb_keys]
    e = eo[single]
    margin = 1 << 20
    ok = ((ent["buffer_addr"][e] == t.keys[single]) & (ent["buffer_size"][e] >= 3)
          & (ent["buffer_addr"][e] + ent["buffer_size"][e] <= t.keys[single + 1])
          & (ent["alloc_date"][e] > tb) & (ent["alloc_date"][e] < E - margin) & (ent["free_date"][e] > E + margin))
    picks = e[ok]
    assert picks.shape[0] >= 8
    picks = picks[np.linspace(0, picks.shape[0] - 1, 8).astype(np.int64)]  # spread over the address space
    edits = [("free_date", E - 256), ("free_date", E - 1), ("free_date", E), ("free_date", E + 255),
             ("alloc_date", E - 256), ("alloc_date", E - 1), ("alloc_date", E), ("alloc_date", E + 256)]
    # reused keys: chains of three whose middle entry lives across E (the
    # lifetimes of a chain are disjoint and stay so)
    triple = np.flatnonzero(np.diff(eo) == 3)
    triple = triple[triple + 1 < t.nb_keys]
    m = eo[triple] + 1
    okc = ((ent["buffer_addr"][m] == t.keys[triple]) & (ent["buffer_size"][m] >= 3)
           & (ent["buffer_addr"][m] + ent["buffer_size"][m] <= t.keys[triple + 1])
           & (ent["alloc_date"][m] < E - margin) & (ent["free_date"][m] > E + margin)
           & (ent["free_date"][m + 1] < ent["alloc_date"][m]) & (ent["alloc_date"][m - 1] > ent["free_date"][m]))
    chain = m[okc]
    if chain.shape[0] >= 4:  # (a replay without reuse has none: the single entries alone)
        picks = np.concatenate([picks, chain[np.linspace(0, chain.shape[0] - 1, 4).astype(np.int64)]])
        edits += [("free_date", E - 256), ("free_date", E + 255), ("alloc_date", E - 256), ("alloc_date", E + 256)]
    rows, who = [], []
    for i, (pe, (field, date)) in enumerate(zip(picks.tolist(), edits)):
        ent[field][pe] = date
        assert ent["alloc_date"][pe] <= ent["free_date"][pe]
        a, s = int(ent["buffer_addr"][pe]), int(ent["buffer_size"][pe])
        stamps = sorted({E + k for k in (-257, -256, -1, 0, 1, 255, 256)} | {date - 1, date, date + 1})
        for addr in (a, a + s // 2, a + s - 1):
            for ts in stamps:
                rows.append((addr, ts))
                who.append(i)
    proto = records(rp)[0][0]
    rec = np.zeros(len(rows), dtype=RECORD_DTYPE)
    rec[:] = proto
    rec["addr"] = [r[0] for r in rows]
    rec["timestamp"] = [r[1] for r in rows]
    rec["weight"] = 1 + np.arange(len(rows)) % 7
    raw = rec.view(np.uint8)
    out.buffers.append(Buffer(0, 0, raw, 0, raw.shape[0]))
    return out, E, [(pe, f, d) for pe, (f, d) in zip(picks.tolist(), edits)], np.array(who)


def lookup_all(table, addr, ts):
    """The oracle's lookup (nmo_lookup) of each (addr, ts): the matched table position, or -1."""
    import pyoracle

    ent = table.entries
    ent4 = np.stack([ent["buffer_addr"], ent["buffer_size"], ent["alloc_date"], ent["free_date"]], axis=1).astype(np.uint64)
    ent4 = np.ascontiguousarray(ent4)
    keys = np.ascontiguousarray(table.keys, dtype=np.uint64)
    off = np.ascontiguousarray(table.entry_off, dtype=np.uint32)
    return np.array([pyoracle.lookup(keys, off, ent4, int(a), int(t)) for a, t in zip(addr, ts)], dtype=np.int64)


_BASE = {}


def base_replay(cfg=LAYOUT_CFG):
    """generate(cfg), once per process (the builders copy what they change)."""
    key = dataclasses.astuple(cfg)
    if key not in _BASE:
        _BASE[key] = generate(cfg)
    return _BASE[key]


def layout_case(T, nbuf, big_bytes=BIG, split=0):
    """The re-cut replay of a LAYOUT_TABLE row with the weights planted for
    its own wesc; (replay, expected layout, planted).  split = k: the case of
    nbuf - k buffers, cut, seeds, planted weights and all, with k buffers
    halved (recut)."""
    rp = recut(base_replay(), T, nbuf, big_bytes, seed=1000 + nbuf - split, split=split)
    lay = expected_layout(rp)
    wesc = lay["wesc"] if not split else (1 << LAYOUT_TABLE[(T, nbuf - split, big_bytes)][4]) - 1
    return rp, lay, plant_weights(rp, wesc, seed=nbuf - split)


def narrow_long_run():
    """The long run through the narrowest record: STRETCH_NARROW_CFG re-cut
    into 256 buffers of 1024 threads' ranks, stretched, with the edge probes
    as the 257th buffer and the weights planted for wbits 11."""
    rp = stretch(recut(base_replay(STRETCH_NARROW_CFG), 1024, 256, BIG, seed=1256))
    rp = edge_probes(rp)[0]
    plant_weights(rp, (1 << MIN_WEIGHT_BITS) - 1, seed=257)
    return rp
