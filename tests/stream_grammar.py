"""Irregular perf record streams for the two record-stream parsers
(route2_kernel's per-wave cursor, attribute_kernel's window cursor): a plain
byte cursor, pattern builders and two seeded replays (shared by
test_record_streams_host.py and test_gpu_record_streams.py; not a test module).

walk() is written from the reference's __analyze_buffer loop
(mem_sampling.c:836-926) alone: the cursor starts at 0, reads the 8 B
perf_event_header under it, takes a PERF_RECORD_SAMPLE's 32 B struct
mem_sample right after the header whatever the header's size says, and moves
on by the header's size.  It shares no code with the oracle, the
multi-threaded restatement or the kernels, so it can referee between them.

Every pattern draws its sample payloads (timestamp, address, weight,
data_src) from the records of a generate(SynthConfig(...)) replay, so that
the samples hit the replay's object table like the generator's own."""
import dataclasses
import struct

import numpy as np

from numamma_amd.replay import RECORD_DTYPE, Buffer, Replay, SynthConfig, generate

SAMPLE, LOST = 9, 2
# non-SAMPLE record types that come with 40 B bodies on a real ring: MMAP,
# COMM, THROTTLE, UNTHROTTLE, FORK, SWITCH
OTHER_TYPES = (1, 3, 5, 6, 7, 14)
JUMP_BYTES = 65_528  # the largest 8-byte multiple a u16 header size holds
EDGE_KS = (63, 64, 65, 127, 128, 129, 959, 960, 961, 1023, 1024, 1025)


# ---------------------------------------------------------------------------
# the byte cursor

def walk(raw):
    """(samples, error) of one linearised buffer.  samples: (offset, ts, addr,
    weight, data_src) per PERF_RECORD_SAMPLE; error: None, or (kind, offset)
    of the first record the cursor cannot take -- in this order at the record
    under the cursor: fewer than 8 B left -> truncated; size 0 -> zero_size
    (:857-860); size not a multiple of 8 -> unaligned (the engine's rule,
    NMG_ERR_UNALIGNED: the reference has none); a SAMPLE whose 40 B or whose
    size run past the end -> truncated (:865-879 would read out of bounds)."""
    data = bytes(memoryview(np.ascontiguousarray(raw, dtype=np.uint8)))
    n, cur, samples = len(data), 0, []
    while cur < n:
        if n - cur < 8:
            return samples, ("truncated", cur)
        type_, _, size = struct.unpack_from("<IHH", data, cur)
        if size == 0:
            return samples, ("zero_size", cur)
        if size & 7:
            return samples, ("unaligned", cur)
        if type_ == SAMPLE:
            if cur + 40 > n or cur + size > n:
                return samples, ("truncated", cur)
            samples.append((cur,) + struct.unpack_from("<QQQQ", data, cur + 8))
        cur += size
    return samples, None


def normalised(rp):
    """rp with every buffer rebuilt from walk() as pure 40 B SAMPLE records:
    the same samples in the same buffers and order.  A buffer left without
    samples keeps one 8 B header-only record, so that it is not dropped as an
    empty ring and the buffer indices stay aligned; empty rings stay empty."""
    out = []
    for b in rp.buffers:
        lin = b.linear()
        if lin.shape[0] == 0:
            out.append(b)
            continue
        samples, err = walk(lin)
        assert err is None, err
        if samples:
            rec = np.zeros(len(samples), dtype=RECORD_DTYPE)
            rec["type"], rec["misc"], rec["size"] = SAMPLE, 2, 40
            s = np.array([x[1:] for x in samples], dtype=np.uint64)
            rec["timestamp"], rec["addr"], rec["weight"], rec["data_src"] = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
            raw = rec.view(np.uint8).copy()
        else:
            raw = np.frombuffer(header(LOST, 8), dtype=np.uint8).copy()
        out.append(Buffer(b.thread_rank, b.access_type, raw, 0, raw.shape[0]))
    return dataclasses.replace(rp, buffers=out)


# ---------------------------------------------------------------------------
# records

def header(type_, size, misc=0):
    return struct.pack("<IHH", type_, misc, size)


def sample(payload, size=40, rng=None):
    """A SAMPLE record of `size` bytes: the header, as much of the 32 B payload
    as fits, random trailing bytes past 40."""
    body = payload[:max(0, min(32, size - 8))]
    extra = size - 8 - len(body)
    return header(SAMPLE, size, 2) + body + (rng.bytes(extra) if extra > 0 else b"")


def other(type_, size, rng, stored=None):
    """A non-SAMPLE record: the header and random bytes; stored < size leaves
    the record cut short (a header whose size runs past the buffer's end)."""
    return header(type_, size) + rng.bytes((size if stored is None else stored) - 8)


def lost24(rng):
    return header(LOST, 24) + struct.pack("<QQ", int(rng.integers(1, 1 << 20)), int(rng.integers(1, 100)))


class Pool:
    """The 32 B sample payloads of a generated replay's records, handed out in order."""

    def __init__(self, rp):
        rec = np.concatenate([b.ring.view(RECORD_DTYPE) for b in rp.buffers])
        self.payload = np.ascontiguousarray(rec).view(np.uint8).reshape(-1, 40)[:, 8:]
        self.next = 0

    def take(self):
        p = self.payload[self.next % self.payload.shape[0]].tobytes()
        self.next += 1
        return p


def buffer_of(parts, rng, nb_threads, rank=None, access=None):
    raw = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    return Buffer(int(rng.integers(0, nb_threads)) if rank is None else rank,
                  int(rng.integers(0, 2)) if access is None else access, raw, 0, raw.shape[0])


def regular(pool, n):
    return [sample(pool.take()) for _ in range(n)]


# ---------------------------------------------------------------------------
# patterns: (pool, rng, nb_threads) -> [Buffer]

def pat_alternate(pool, rng, T):
    parts = []
    for _ in range(1000):
        parts += [sample(pool.take()), lost24(rng)]
    return [buffer_of(parts, rng, T)]


def pat_type40(pool, rng, T):
    parts = [other(int(rng.choice(OTHER_TYPES)), 40, rng) if rng.random() < 0.3 else sample(pool.take())
             for _ in range(1500)]
    return [buffer_of(parts, rng, T)]


def pat_long(pool, rng, T):
    parts = [sample(pool.take(), int(rng.choice((40, 48, 56, 64, 104))), rng) for _ in range(1000)]
    return [buffer_of(parts, rng, T)]


def pat_jump(pool, rng, T):
    """Runs of 1-200 SAMPLEs between 65,528 B records that jump over whole
    windows; one buffer ends on a run, the other on a jump."""
    out = []
    for ends_on_jump in (False, True):
        parts = []
        for _ in range(6):
            parts += regular(pool, int(rng.integers(1, 201)))
            parts.append(other(int(rng.choice(OTHER_TYPES)), JUMP_BYTES, rng))
        if not ends_on_jump:
            parts += regular(pool, int(rng.integers(1, 201)))
        out.append(buffer_of(parts, rng, T))
    return out


def pat_hdr8(pool, rng, T):
    parts = []
    for _ in range(400):
        parts.append(sample(pool.take()))
        parts += [header(int(rng.choice(OTHER_TYPES)), 8) for _ in range(int(rng.integers(1, 9)))]
    return [buffer_of(parts, rng, T)]


def edge_buffer(pool, rng, T, k):
    return buffer_of(regular(pool, k) + [lost24(rng)] + regular(pool, k), rng, T)


def pat_edge(pool, rng, T):
    """k regular SAMPLEs, one LOST24, k regular SAMPLEs: the irregular record
    at, one before and one after the 64-slot route window, its double,
    attribute_kernel's list cap (960 = 1024 - 64) and its 1024-slot window."""
    return [edge_buffer(pool, rng, T, k) for k in EDGE_KS]


def pat_overshoot(pool, rng, T):
    return [buffer_of(regular(pool, 70) + [other(int(rng.choice(OTHER_TYPES)), 4096, rng, stored=24)], rng, T)]


def pat_nosample(pool, rng, T):
    return [buffer_of([lost24(rng) for _ in range(200)], rng, T), buffer_of([header(LOST, 8)], rng, T)]


def pat_empty(pool, rng, T):
    """A ring with data_head == data_tail between two others."""
    ring = np.frombuffer(rng.bytes(64), dtype=np.uint8).copy()
    return [buffer_of(regular(pool, 50), rng, T), Buffer(int(rng.integers(0, T)), int(rng.integers(0, 2)), ring, 24, 24),
            buffer_of(regular(pool, 50), rng, T)]


def pat_short(pool, rng, T):
    """SAMPLEs of 16/24/32 B among 40 B ones: a short one's struct mem_sample
    runs into the records after it.  A 16 B one reads the next header as its
    address (no match), a 32 B one as its data_src (level 0).  A 24 B one is
    followed by a 16 B non-SAMPLE record whose body is a pool record's
    data_src: its weight is that record's header (about 2^52: past every
    packed counter), its level one the generator (or a redraw) made, so the
    level strings of the oracle's dump lines stay exact (cost_expect.py).
    Two 40 B records close the buffer: 40 readable bytes after every start."""
    parts = []
    for _ in range(600):
        size = int(rng.choice((16, 24, 32))) if rng.random() < 0.4 else 40
        parts.append(sample(pool.take(), size))
        if size == 24:
            parts.append(header(int(rng.choice(OTHER_TYPES)), 16) + pool.take()[24:32])
    return [buffer_of(parts + regular(pool, 2), rng, T)]


def dense_parts(pool, rng, draws=2000):
    parts = []
    for u in rng.random(draws):
        if u < 0.5:
            parts.append(sample(pool.take()))
        elif u < 0.6:
            parts.append(sample(pool.take(), int(rng.choice((48, 56))), rng))
        else:
            parts.append(other(int(rng.choice(OTHER_TYPES + (LOST,))), int(rng.choice((8, 16, 24, 32, 40, 48, 72, 4096))), rng))
    return parts


def pat_dense(pool, rng, T):
    return [buffer_of(dense_parts(pool, rng), rng, T) for _ in range(2)]


def pat_wrapped(pool, rng, T):
    """A dense buffer stored as a wrapped ring (data_head < data_tail), cut 16 B
    into a SAMPLE record; 64 stale bytes between head and tail are never read."""
    b = buffer_of(dense_parts(pool, rng), rng, T)
    samples, err = walk(b.ring)
    assert err is None and len(samples) > 10
    cut = samples[len(samples) // 2][0] + 16
    first, second = b.ring[:cut], b.ring[cut:]
    ring = np.concatenate([second, np.full(64, 0xAB, dtype=np.uint8), first])
    return [Buffer(b.thread_rank, b.access_type, ring, second.shape[0] + 64, second.shape[0])]


PATTERNS = {"alternate": pat_alternate, "type40": pat_type40, "long": pat_long, "jump": pat_jump, "hdr8": pat_hdr8,
            "edge": pat_edge, "overshoot": pat_overshoot, "nosample": pat_nosample, "empty": pat_empty,
            "short": pat_short, "dense": pat_dense, "wrapped": pat_wrapped}


def tiny_buffer_count():
    """At least 5 buffers per route wave (CU count x 12 waves), and no fewer than 16,384."""
    n = 16_384
    try:
        import torch

        if torch.cuda.is_available():
            n = max(n, 5 * torch.cuda.get_device_properties(0).multi_processor_count * 12)
    except ImportError:
        pass
    return n


def pat_tiny(pool, rng, T, nb_buffers):
    """Buffers of 1-5 records; a quarter hold one irregular record or are a
    single 8 B record.  Thread and access change every few buffers, so that
    neighbours share an attribute_kernel window (same stream) and a route
    wave's slow-path windows are followed by a buffer change."""
    out = []
    rank, access = int(rng.integers(0, T)), int(rng.integers(0, 2))
    for _ in range(nb_buffers):
        if rng.random() < 0.25:
            rank, access = int(rng.integers(0, T)), int(rng.integers(0, 2))
        n = int(rng.integers(1, 6))
        parts = regular(pool, n)
        if rng.random() < 0.25:
            kind = int(rng.integers(0, 5))
            if kind == 0:
                parts = [header(LOST, 8)]
            else:
                irr = (lost24(rng), sample(pool.take(), 48, rng), header(int(rng.choice(OTHER_TYPES)), 8),
                       other(int(rng.choice(OTHER_TYPES)), 40, rng))[kind - 1]
                parts[int(rng.integers(0, n))] = irr
        out.append(buffer_of(parts, rng, T, rank, access))
    return out


# ---------------------------------------------------------------------------
# the two replays

def _pool_replay(nkeys, seed, prepare_pool):
    rp = generate(SynthConfig(nb_samples=60_000, nb_intervals=nkeys, seed=seed))
    if prepare_pool is not None:
        prepare_pool(rp)  # e.g. cost_expect.redraw_levels on the pure 40 B records
    return rp


def grammar_replay(nkeys, prepare_pool=None, seed=211):
    """Every pattern except tiny over a table of nkeys heap intervals: about
    3 MB of records, about 22k samples.  meta["patterns"] = {name: (first
    buffer, count)} indexes rp.buffers."""
    src = _pool_replay(nkeys, seed, prepare_pool)
    pool, rng = Pool(src), np.random.default_rng(seed)
    bufs, where = [], {}
    for name, fn in PATTERNS.items():
        b = fn(pool, rng, src.nb_threads)
        where[name] = (len(bufs), len(b))
        bufs += b
    return Replay(src.nb_threads, src.table, bufs, {"patterns": where})


def tiny_replay(nkeys, nb_buffers=None, prepare_pool=None, seed=223):
    src = _pool_replay(nkeys, seed, prepare_pool)
    rng = np.random.default_rng(seed)
    n = tiny_buffer_count() if nb_buffers is None else nb_buffers
    return Replay(src.nb_threads, src.table, pat_tiny(Pool(src), rng, src.nb_threads, n), {"patterns": {"tiny": (0, n)}})


def kept_index(rp):
    """Index of each buffer among the non-empty ones (the oracle's and the
    engine's buffer numbering), -1 for an empty ring."""
    out, k = [], 0
    for b in rp.buffers:
        if b.linear().shape[0]:
            out.append(k)
            k += 1
        else:
            out.append(-1)
    return out
