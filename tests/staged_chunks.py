"""Batches, chunk sizes and models for the staged pipeline's tests (HipEngine::run_staged: the cut into chunks, the
ring of two slots, one plan per chunk), shared by the GPU tier (tests/test_gpu_staged_chunks.py), which runs them,
and the CPU tier (tests/test_staged_chunks.py), which proves what they claim: that the cut is the rule's, that the
cases reach the chunk counts, start phases, result placements and kernels they are named for, and that their
expected rows tell a stale slot, a misplaced result block or a wrong bit phase from a right run. Plain data, numpy
and the CPU engine: no GPU.

The rule (csrc/include/moc/tile_plan.hpp staged_chunk_end): a chunk is the longest run of records rb..re with
re - rb <= chunk_records and offsets[re] - offsets[rb] <= chunk_bytes, and at least one record."""
import math

import numpy as np

from mpi_openmp_cuda_amd import Problem, Semantics, _lib, search_cpu
from mpi_openmp_cuda_amd.models.problem import pack5
from mpi_openmp_cuda_amd.ops.align import as_triples, kernel_bounds
from mpi_openmp_cuda_amd.utils.synthetic import seq_no_equal_neighbours

POISON = 0x5A            # every byte of a result array before a solve, and of its guard rows always
GUARD = 5                # poisoned rows in front of and behind every result slice
BASE = 12345             # offsets[0] of every batch: a slice of a larger CSR array
DEFAULT_R, DEFAULT_B = 1 << 21, 64 << 20  # EngineOptions' chunk_records and chunk_bytes
INT_MIN = -2 ** 31
FORMAT_BYTES = {"r12": 12, "r8": 8, "r4": 4, "r2": 2}
W6 = (4, 3, 2, 10)       # input6's weights
W = (10, 2, 3, 4)


def model_chunks(offsets, chunk_records=0, chunk_bytes=0):
    """The rule by a plain loop over Python ints: the bounds [0, b1, ..., n]."""
    off = [int(x) for x in offsets]
    n = len(off) - 1
    R = int(chunk_records) or DEFAULT_R
    B = int(chunk_bytes) or DEFAULT_B
    bounds, rb = [0], 0
    while rb < n:
        re = rb + 1  # at least one record
        while re < n and (re + 1) - rb <= R and off[re + 1] - off[rb] <= B:
            re += 1
        bounds.append(re)
        rb = re
    return bounds


# ---- batches ------------------------------------------------------------------------------------------------
class Batch:
    """Records as a slice of a larger CSR array: ``codes`` holds BASE neighbour letters, the records and a tail of
    neighbour letters, ``offsets`` the absolute offsets (offsets[0] = BASE); ``prob`` is the same records alone
    (offsets from 0), what the CPU engine is asked. Everything read-only."""

    def __init__(self, name, weights, seq1, records, seed=0):
        rng = np.random.default_rng(seed + 99)
        lengths = np.array([len(r) for r in records], np.int64)
        assert lengths.min() >= 1  # no zero-length records
        offsets = np.zeros(len(records) + 1, np.int64)
        np.cumsum(lengths, out=offsets[1:])
        letters = np.concatenate(records).astype(np.uint8)
        self.name = name
        self.prob = Problem(weights, np.asarray(seq1, np.uint8), letters, offsets)
        self.codes = np.concatenate([rng.integers(1, 27, BASE).astype(np.uint8), letters,
                                     rng.integers(1, 27, 64).astype(np.uint8)])
        self.offsets = offsets + BASE
        self.lengths = lengths
        self.n = len(records)
        self._rows, self._p5 = {}, None
        for a in (self.prob.codes, self.prob.offsets, self.prob.seq1, self.codes, self.offsets, self.lengths):
            a.setflags(write=False)

    def rows(self, sem=Semantics.REFERENCE):
        """The CPU engine's (score, n, k) rows, computed once per semantics."""
        if sem not in self._rows:
            r = as_triples(search_cpu(self.prob, sem)).copy()
            r.setflags(write=False)
            self._rows[sem] = r
        return self._rows[sem]

    def packed5(self):
        """``codes`` as one 5-bit stream (letter j at bits [5 j, 5 j + 5)): a chunk starts at any bit phase."""
        if self._p5 is None:
            self._p5 = pack5(self.codes)
            self._p5.setflags(write=False)
        return self._p5

    def bounds(self, R=0, B=0):
        return model_chunks(self.offsets, R, B)


def _letters(rng, n):
    return rng.integers(1, 27, int(n)).astype(np.uint8)


def _random_batch(name, weights, L1, lengths, seed):
    rng = np.random.default_rng(seed)
    return Batch(name, weights, _letters(rng, L1), [_letters(rng, l) for l in lengths], seed)


def _swipe6():
    # input6's shape: Seq1 of 26 letters, records of 5..11 (every chunk takes the swipe kernel); the first, the
    # middle and the last record have 11 letters, which chunk_bytes = 10 does not hold
    rng = np.random.default_rng(61)
    lengths = rng.integers(5, 12, 150)
    lengths[[0, 75, 149]] = 11
    return _random_batch("swipe6", W6, 26, lengths, 61)


def _mixed300():
    # Seq1 of 300 letters, records of 1..320: short-kernel and tile16 records in most chunks, records longer than
    # Seq1 (no candidate); 320 letters first, in the middle and last
    rng = np.random.default_rng(300)
    lengths = rng.integers(1, 321, 120)
    lengths[[0, 60, 119]] = 320
    return _random_batch("mixed300", W, 300, lengths, 300)


RING_COUNTS = (1, 2, 3, 4, 5, 8, 9)
RING_N = 360  # a multiple of every count


def _ring():
    rng = np.random.default_rng(360)
    return _random_batch("ring", W6, 26, rng.integers(5, 12, RING_N), 360)


def ring_records(count):
    """chunk_records that cuts the ring batch into exactly ``count`` chunks."""
    return RING_N // count


GROWTH_R = 64
GROWTH_LENGTHS = tuple(math.ceil(64 * 1.3 ** c) for c in range(8))  # 64 .. 402 letters, chunk by chunk
# ensure() (csrc/src/hip_engine.cpp) allocates max(1.25 * bytes, 4096) for the bytes asked, and run_staged asks
# for a chunk's letters + 32: from 4096 letters up, a chunk with more than 1.25 times the letters (and 8 more) of
# the chunk two before it finds its slot too small
GROWTH_FLOOR, GROWTH_FACTOR, GROWTH_PAD = 4096, 1.25, 8


def _growth(reverse=False):
    rng = np.random.default_rng(500)
    seq1 = _letters(rng, 500)
    recs = [_letters(rng, l) for l in GROWTH_LENGTHS for _ in range(GROWTH_R)]
    return Batch("growth_reversed" if reverse else "growth", W, seq1, recs[::-1] if reverse else recs, 500)


PHASE_R, PHASE_CHUNKS = 3, 48
PHASE_SWIPE_LENGTHS = (5, 5, 7)                                  # 17 letters per chunk
PHASE_TILE16_LENGTHS = ((40, 57, 84), (45, 90, 46), (60, 61, 60))  # 181 letters per chunk, chunks in turn


def _phase(name, weights, L1, triples, seed):
    # the first record of every chunk is a copy of Seq1 (without equal neighbours) from an offset that moves with
    # the chunk: its row is (W1 * L2, p, 0), and any other first letter gives another row
    rng = np.random.default_rng(seed)
    seq1 = seq_no_equal_neighbours(rng, L1)
    recs = []
    for c in range(PHASE_CHUNKS):
        t = triples[c % len(triples)]
        p = (7 * c) % (L1 - t[0])  # 0 .. L1 - L2 - 1: an offset both semantics try
        recs += [seq1[p:p + t[0]].copy(), _letters(rng, t[1]), _letters(rng, t[2])]
    return Batch(name, weights, seq1, recs, seed)


def phase_position(batch, c):
    """The offset the first record of chunk c of a phase batch was copied from."""
    L2 = int(batch.lengths[PHASE_R * c])
    return (7 * c) % (batch.prob.L1 - L2)


PLACEMENT_R = 35   # 35 * fb mod 16 = 6, 12, 8, 4 for fb = 2, 4, 8, 12
PLACEMENT_N = 4100  # R2 results of three pages: a half that is page-locked ends inside the array


def _placement():
    rng = np.random.default_rng(35)
    return _random_batch("placement", W6, 26, rng.integers(6, 12, PLACEMENT_N), 35)


# ---- a kernel per chunk: segments of 40 records on a Seq1 of 150 letters -------------------------------------
KERNEL_L1, SEGMENT = 150, 40
W_I16 = (300, 2, 3, 4)    # |Dt| past the byte pairs, within the int16 profile; 2 * 300 * 128 past the swipe keys
W_LUT = (300, 300, 1, 1)  # |Dt| past the int16 profile: the LUT tile kernel
KERNEL_WEIGHTS = {"w10": W, "w300": W_I16, "lut": W_LUT}


def _segment_lengths(name, rng):
    if name == "swipe":
        return rng.integers(90, 129, SEGMENT)
    if name == "short":  # a few records longer than Seq1: unsearchable
        l = rng.integers(130, 151, SEGMENT)
        l[[3, 17, 31, 39]] = rng.integers(151, 201, 4)
        return l
    if name == "tile16":
        return rng.integers(5, 81, SEGMENT)
    if name == "short_tile16":
        return np.array([100, 20] * (SEGMENT // 2))
    if name == "unsearchable":
        return rng.integers(151, 201, SEGMENT)
    if name in ("long20k", "long60k"):  # one very long record among short-kernel records
        l = rng.integers(130, 151, SEGMENT)
        l[17] = 20_000 if name == "long20k" else 60_000
        return l
    raise KeyError(name)


SEGMENTS = ("swipe", "short", "tile16", "short_tile16", "unsearchable", "long20k", "long60k")


def _kernel_batch(name):
    """``kernels_<weights>_<segment>``: one segment alone; ``kernels_<weights>_all``: the segments in order."""
    _, wname, seg = name.split("_", 2)
    rng = np.random.default_rng(150)
    seq1 = _letters(rng, KERNEL_L1)
    recs = {s: [_letters(rng, l) for l in _segment_lengths(s, rng)] for s in SEGMENTS}  # the same under every name
    records = sum((recs[s] for s in SEGMENTS), []) if seg == "all" else recs[seg]
    return Batch(name, KERNEL_WEIGHTS[wname], seq1, records, 150)


# what every segment alone takes: tests/test_staged_chunks.py derives it from the rules (classify), and
# tests/test_gpu_staged_chunks.py asserts that stats() says the same
STATED = {
    "w10": {"swipe": ["swipe"], "short": ["short"], "tile16": ["tile16"], "short_tile16": ["short", "tile16"],
            "unsearchable": ["short"], "long20k": ["short"], "long60k": ["tile16"]},
    "w300": {"swipe": ["short"], "short": ["short"], "tile16": ["tile16"], "short_tile16": ["short", "tile16"],
             "unsearchable": ["short"], "long20k": ["short"], "long60k": ["tile16"]},
    "lut": {"swipe": ["short"], "short": ["short"], "tile16": ["tiles"], "short_tile16": ["short", "tiles"],
            "unsearchable": ["short"], "long20k": ["short"], "long60k": ["tiles"]},
}


def _short_lds_fits(L1, max_l2, fb):
    """configure_short's budget (csrc/src/hip/short_kernels.hip) at its smallest tile of one record: the profile or
    the LUT and Seq1, the tile's offsets, its letters and its results within 60 KiB."""
    def a16(x):
        return (x + 15) & ~15
    row = (L1 + 64 + 3) & ~3
    table = a16(27 * row * 4) if 27 * row * 4 <= 24 * 1024 else 1024 * 4 + a16(L1 + 64 + 4)
    cap = max(max_l2, 1) + 48
    return cap <= 60 * 1024 and table + a16(2 * 4 + 64) + a16(cap) + a16(fb) <= 60 * 1024


def classify(weights, L1, lengths, fb=12):
    """The kernels a chunk of these record lengths takes, as ``stats()["kernels"]`` lists them, from the length
    rules of plan::plan_chunk and HipEngine::plan_batch: records of at least L1 - 63 letters need at most 64 lanes
    (the short set, records longer than Seq1 among them), the others go to the tile kernel; a chunk of short
    records only takes the swipe kernel when its integer bounds hold the chunk (kernel_bounds: at most 64 offsets,
    at most 128 letters, keys that cannot wrap), else the short kernel, and when that kernel's LDS cannot hold the
    longest record every record goes to the tile kernel; the tile kernel is tile16 when a profile holds the
    table, else the LUT tiles."""
    lengths = [int(l) for l in lengths]
    short = [l for l in lengths if l >= max(L1 - 63, 0)]
    tiles = len(short) < len(lengths)
    out = []
    if short:
        kb = kernel_bounds(weights, L1, min(short), max(lengths))
        if not tiles and kb["swipe"] is not None:
            out.append("swipe")
        elif _short_lds_fits(L1, max(lengths), fb):
            out.append("short")
        else:
            tiles = True
    if tiles:
        kb = kernel_bounds(weights, L1, min(lengths), max(lengths))
        out.append("tile16" if kb["profile16"] or kb["profile16_i16"] else "tiles")
    return out


def union_kernels(lists):
    order = ("swipe", "short", "tiles", "tile16")
    return [k for k in order if any(k in l for l in lists)]


def chunk_kernels(b, bounds, fb=12):
    """The kernels of a whole solve of batch ``b`` cut at ``bounds``: every chunk's, together."""
    return union_kernels([classify(b.prob.weights.as_list(), b.prob.L1, b.lengths[a:e], fb)
                          for a, e in zip(bounds, bounds[1:])])


_BUILDERS = {"swipe6": _swipe6, "mixed300": _mixed300, "ring": _ring, "growth": _growth,
             "growth_reversed": lambda: _growth(True), "placement": _placement,
             "phase_swipe": lambda: _phase("phase_swipe", W6, 26, (PHASE_SWIPE_LENGTHS,), 26),
             "phase_tile16": lambda: _phase("phase_tile16", W, 300, PHASE_TILE16_LENGTHS, 301)}
_batches = {}


def batch(name) -> Batch:
    """A batch by name, built once."""
    if name not in _batches:
        _batches[name] = _kernel_batch(name) if name.startswith("kernels_") else _BUILDERS[name]()
    return _batches[name]


# ---- chunk sizes --------------------------------------------------------------------------------------------
CUT_BATCHES = ("swipe6", "mixed300")


def cut_cases(lengths):
    """(tag, chunk_records, chunk_bytes) at the rule's edges for a batch of these lengths; 0: the engine's default.
    j = n // 3 records hold S letters: chunk_bytes of S, S - 1 and S + 1; chunk_bytes one less than the longest
    record (a record longer than chunk_bytes, wherever the batch has its longest records) and 1 (every record);
    chunk_records of 1, n - 1, n and n + 1 (the last two: one chunk, copied on the compute stream); both limits
    at work in one batch."""
    lengths = [int(l) for l in lengths]
    n = len(lengths)
    j = n // 3
    S = sum(lengths[:j])
    return [("bytes_exact", n + 1, S), ("bytes_one_less", n + 1, S - 1), ("bytes_one_more", n + 1, S + 1),
            ("record_over_bytes", n + 1, max(lengths) - 1), ("bytes_1", n + 1, 1),
            ("records_1", 1, 0), ("records_n_minus_1", n - 1, 0), ("records_n", n, 0), ("records_n_plus_1", n + 1, 0),
            ("both_limits", 7, 7 * sum(lengths) // n)]  # seven records of the mean length


# name, lengths, offsets[0], chunk_records, chunk_bytes, the bounds
HAND = [
    ("bytes_exact", [10] * 12, 0, 100, 40, [0, 4, 8, 12]),
    ("bytes_one_less", [10] * 12, 0, 100, 39, [0, 3, 6, 9, 12]),
    ("bytes_one_more", [10] * 12, 0, 100, 41, [0, 4, 8, 12]),
    ("bytes_1", [10] * 12, 0, 100, 1, list(range(13))),
    ("records_1", [10] * 12, 0, 1, 1 << 20, list(range(13))),
    ("records_n_minus_1", [10] * 12, 0, 11, 1 << 20, [0, 11, 12]),
    ("records_n", [10] * 12, 0, 12, 1 << 20, [0, 12]),
    ("records_n_plus_1", [10] * 12, 0, 13, 1 << 20, [0, 12]),
    ("defaults", [10] * 12, 0, 0, 0, [0, 12]),
    ("records_first", [10] * 12, 0, 3, 45, [0, 3, 6, 9, 12]),
    ("bytes_first", [10] * 12, 0, 5, 25, [0, 2, 4, 6, 8, 10, 12]),
    ("long_first", [50, 10, 10, 10, 10], 0, 100, 20, [0, 1, 3, 5]),
    ("long_middle", [10, 10, 50, 10, 10], 0, 100, 20, [0, 2, 3, 5]),
    ("long_before_last", [10, 10, 10, 50, 10], 0, 100, 20, [0, 2, 3, 4, 5]),
    ("long_last", [10, 10, 10, 10, 50], 0, 100, 20, [0, 2, 4, 5]),
    ("long_alone", [3000], 0, 100, 20, [0, 1]),
    ("longer_than_seq1", [2000, 3001, 5, 3500, 3500], 0, 2, 6000, [0, 2, 4, 5]),  # Seq1 has at most 3000 letters
    ("slice", [10] * 12, 12345, 100, 39, [0, 3, 6, 9, 12]),
    ("slice_long_first", [50, 10, 10, 10, 10], 12345, 100, 20, [0, 1, 3, 5]),
    ("slice_past_2_33", [10] * 12, (1 << 33) + 7, 5, 25, [0, 2, 4, 6, 8, 10, 12]),
    ("huge_limits", [10] * 12, 12345, 2 ** 63 - 1, 2 ** 63 - 1, [0, 12]),
]


def hand_offsets(lengths, base):
    return np.concatenate([[base], base + np.cumsum(lengths)]).astype(np.int64)


# ---- models of what the engine does with a chunk's results and bits --------------------------------------------
def r2_stand_in(rows):
    """(smin, kw, j) that hold these rows in R2 codes below 0xFFFF (the engine derives its own from the problem's
    bounds; any parameters that hold the rows decode the same way)."""
    ok = rows[rows[:, 0] != INT_MIN]
    smin, kw = int(ok[:, 0].min()), int(ok[:, 2].max()) + 1
    j = (int(ok[:, 1].max()) + 1) * kw
    assert (int(ok[:, 0].max()) - smin) * j + j - 1 < 0xFFFF
    return smin, kw, j


def encode_rows(rows, fmt, r2=None):
    """int32 [n, 3] rows -> the bytes of result format ``fmt`` (csrc/include/moc/device.hpp ResultFormat)."""
    rows = np.asarray(rows, np.int32)
    none = rows[:, 0] == INT_MIN
    if fmt == "r12":
        return np.ascontiguousarray(rows).view(np.uint8).reshape(-1).copy()
    if fmt == "r2":
        smin, kw, j = r2
        c = (rows[:, 0].astype(np.int64) - smin) * j + rows[:, 1] * kw + rows[:, 2]
        c[none] = 0xFFFF
        return c.astype("<u2").view(np.uint8).copy()
    out = np.zeros(rows.shape[0], _lib.FORMAT_DTYPES[_lib.FORMAT_NAMES.index(fmt)])
    out["score"] = np.where(none & (fmt == "r4"), -2 ** 15, rows[:, 0])
    out["n"], out["k"] = rows[:, 1], rows[:, 2]
    return out.view(np.uint8).copy()


def place_blocks(rows, bounds, fmt, r2=None, row_shift=0, place_fb=None):
    """The result array after a run that copies chunk c's block to byte (b[c] + row_shift) * place_fb of it
    (right: shift 0 and the format's own bytes per row), from poison, guard rows included -> (decoded rows, guard
    bytes intact)."""
    fb = FORMAT_BYTES[fmt]
    place_fb = place_fb or fb
    n = len(rows)
    big = np.full((n + 2 * GUARD) * fb, POISON, np.uint8)
    data = encode_rows(rows, fmt, r2)
    for c in range(len(bounds) - 1):
        at = GUARD * fb + (bounds[c] + row_shift) * place_fb
        blk = data[bounds[c] * fb:bounds[c + 1] * fb]
        big[at:at + len(blk)] = blk[:max(0, len(big) - at)]
    body = big[GUARD * fb:(GUARD + n) * fb]
    intact = bool((big[:GUARD * fb] == POISON).all() and (big[(GUARD + n) * fb:] == POISON).all())
    return as_triples(body.view(_lib.FORMAT_DTYPES[_lib.FORMAT_NAMES.index(fmt)]), r2=r2), intact


def unpack5_at(packed, bit0, n):
    """n letters of a 5-bit stream from bit ``bit0``, by Python ints."""
    stream = int.from_bytes(bytes(packed), "little")
    return np.array([(stream >> (bit0 + 5 * i)) & 31 for i in range(n)], np.uint8)
