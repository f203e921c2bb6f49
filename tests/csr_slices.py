"""Inputs of the slice-contract tests (tests/test_gpu_csr_slices.py, tests/test_csr_slices_fixture.py): a batch as
a slice of a larger CSR array. Plain numpy, no GPU.

``slice_case`` lays a family's records somewhere inside a larger letter array: ``c0`` neighbour letters, the
slice's letters, a tail of neighbour letters; the batch's offsets are absolute (``c0 + sub.offsets``). The
neighbours are valid letters (1..26) in two fills, so a kernel that reads one letter too many or too few, or
rebases an offset wrongly, changes a score and never indexes a table out of range:

* ``"A"``: every neighbour letter is 1;
* ``"continue"``: the letters behind the slice (and behind every record whose successor could be chosen that
  way) are the Seq1 letters that extend the record's planted alignment, the letters before the slice the Seq1
  letters that precede the first record's — an over-read or under-read raises the score.

Most records are pieces of Seq1 (exact, with one letter left out — a winner with k > 0 —, or with a few letters
replaced), the rest random letters: a read that starts one letter off moves the winning offset.

The second half of the module lays the same slices at far placements, offsets past 2^31 and 2^32, into an arena
instead of a storage of their own (tests/test_far_offsets_fixture.py, tests/test_gpu_far_offsets.py).
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from mpi_openmp_cuda_amd import Problem
from mpi_openmp_cuda_amd.utils.synthetic import seq_no_equal_neighbours

FILLS = ("A", "continue")
TAIL = 48  # neighbour letters behind the slice: three 16-byte granules
HEAD = 64  # neighbour letters an arena placement writes in front of the slice: four granules


def _record(rng, seq1, L2, want):
    """One record of L2 letters -> (letters, the Seq1 position it was cut at or -1, the Seq1 position whose letter
    would extend its alignment or -1). ``want``: the letter the record should start with (the previous record's continuation), or 0."""
    L1 = seq1.shape[0]
    kind = int(rng.integers(0, 4))  # 0 exact piece, 1 one letter left out, 2 letters replaced, 3 random
    room = L1 - L2 - (1 if kind == 1 else 0)
    if L2 > L1 or kind == 3 or room < 0 or (kind == 1 and L2 < 2):
        r = rng.integers(1, 27, size=L2, dtype=np.uint8)
        if want and L2:
            r[0] = want
        return r, -1, -1
    starts = np.arange(room + 1)
    if want:
        hit = starts[seq1[:room + 1] == want]
        starts = hit if hit.size else starts
    p = int(starts[rng.integers(0, starts.shape[0])])
    if kind == 1:
        j = int(rng.integers(1, L2))
        r = np.concatenate([seq1[p:p + j], seq1[p + j + 1:p + L2 + 1]])
        nxt = p + L2 + 1
    else:
        r = seq1[p:p + L2].copy()
        nxt = p + L2
        if kind == 2 and L2 >= 4:
            at = rng.integers(1, L2, size=max(1, L2 // 8))  # never the first letter: it continues the record before
            r[at] = rng.integers(1, 27, size=at.shape[0], dtype=np.uint8)
    return r.astype(np.uint8), p, (nxt if nxt < L1 else -1)


@dataclass(frozen=True)
class SliceCase:
    sub: Problem          # the slice's records with offsets from 0: the CPU engine on it is the oracle
    c0: int               # neighbour letters in front of the slice
    offsets: np.ndarray   # int64 [n + 1] absolute offsets into the storage: c0 + sub.offsets
    first_at: int         # Seq1 position of the first record's first letter (-1: not a piece of Seq1)
    next_at: int          # Seq1 position that would extend the last record (-1: none)

    def _laid(self, fill: str, head: int, tail: bool) -> np.ndarray:
        """uint8 [head + letters (+ TAIL)]: ``head`` neighbours in front, the slice's letters, the neighbours behind."""
        seq1, L1 = self.sub.seq1, self.sub.L1
        total = int(self.sub.offsets[-1])
        out = np.ones(head + total + (TAIL if tail else 0), np.uint8)
        out[head:head + total] = self.sub.codes
        if fill == "continue":
            first = self.first_at if self.first_at >= 0 else 0
            out[:head] = seq1[(first - head + np.arange(head)) % L1]  # ..., Seq1[first - 1] | the slice
            if tail:
                nxt = self.next_at if self.next_at >= 0 else 0
                out[head + total:] = seq1[(nxt + np.arange(TAIL)) % L1]
        elif fill != "A":
            raise ValueError(f"fill: one of {FILLS}")
        assert out.min() >= 1 and out.max() <= 26  # never letter 0: its table row is all zero and would hide a leak
        return out

    def storage(self, fill: str = "A", tail: bool = True) -> np.ndarray:
        """uint8 [c0 + letters (+ TAIL)]: the neighbours in front, the slice's letters, the neighbours behind;
        ``tail=False`` ends at the slice's last letter."""
        return self._laid(fill, self.c0, tail)

    def patch(self, fill: str = "A"):
        """The slice for an arena of letter 1 -> ``(at, letters)``: ``letters`` go to ``view[at:at + len(letters)]``.
        They are ``storage(fill)`` from ``HEAD`` letters in front of the slice to ``TAIL`` behind it."""
        assert self.c0 >= HEAD
        return self.c0 - HEAD, self._laid(fill, HEAD, True)


def slice_case(weights, seq1, lens, c0: int = 32, seed: int = 0) -> SliceCase:
    """The slice of a family: records of the lengths ``lens`` against ``seq1`` under ``weights``, placed behind
    ``c0`` neighbour letters. The records depend on ``seed`` alone, not on ``c0``."""
    rng = np.random.default_rng(seed)
    seq1 = np.ascontiguousarray(seq1, dtype=np.uint8)
    recs, want, first_at, nxt = [], 0, -1, -1
    for i, L2 in enumerate(lens):
        r, p, nxt = _record(rng, seq1, int(L2), want)
        if i == 0:
            first_at = p
        want = int(seq1[nxt]) if nxt >= 0 else 0
        recs.append(r)
    lengths = np.array([r.shape[0] for r in recs], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    codes = np.concatenate(recs) if recs else np.zeros(0, np.uint8)
    sub = Problem(list(weights), seq1, codes, offsets)
    return SliceCase(sub, int(c0), offsets + int(c0), first_at, nxt)


# ---- the families: name -> (weights, L1, record lengths); the shapes that select each kernel in tests/test_gpu.py
def _range(lo, hi, n, seed):
    """n lengths in lo..hi with both ends present: the kernels' arithmetic forms follow the batch's extremes."""
    return [lo, hi] + np.random.default_rng(seed).integers(lo, hi + 1, size=n - 2).tolist()


def _input4_lens(n, seed):  # input4's record lengths (5..82)
    return _range(5, 82, n, seed)


TILE_L1 = 140  # tests/test_gpu_topk.py: the wave-tile edges of the profile kernel
TILE_LENS = [TILE_L1 - d for d in (1, 2, 62, 63, 64, 125, 126, 127)] + [TILE_L1, TILE_L1 + 1, 1, 2]
TARGET_LENS = (60, 80)  # the catalog of the targets forms: two targets, TILE_L1 letters together


def _mixed_lens():
    """Short-kernel records (130..150 letters: at most 21 offsets) and tile16 records (5..60: more than 64
    offsets) interleaved."""
    a, b = _range(130, 150, 40, 31), _range(5, 60, 40, 32)
    return [x for pair in zip(a, b) for x in pair]


FAMILIES = {
    # lane-per-record swipe kernels: 4, 16 and 32 record words; 1 100 records = two 512-record tiles and a tail
    "swipe_w4": ((5, 2, 3, 4), 40, lambda: _range(6, 16, 1100, 1)),
    "swipe_w16": ((3, 1, 2, 1), 70, lambda: _range(40, 64, 1100, 2)),
    "swipe_w32": ((100, 3, 2, 7), 190, lambda: _range(127, 128, 1100, 3)),
    "swipe_w4_full": ((5, 2, 3, 4), 40, lambda: [16] * 1100),      # every record at max_l2: 16-byte-multiple tiles
    "swipe_w16_full": ((3, 1, 2, 1), 70, lambda: [64] * 1100),
    "swipe_w32_full": ((100, 3, 2, 7), 190, lambda: [128] * 1100),
    "swipe_r2": ((4, 3, 2, 10), 26, lambda: _range(6, 11, 1100, 4)),  # input6's shape: the R2 format holds it
    "swipe_w4_host": ((5, 2, 3, 4), 40, lambda: _range(6, 16, 2500, 5)),  # host tiles hold 2048 records
    "swipe_w16_host_full": ((3, 1, 2, 1), 70, lambda: [64] * 2500),
    # lane-per-offset short kernel, its three arithmetic forms
    "short_pk": ((109, 0, 0, 109), 150, lambda: _range(130, 150, 300, 6)),
    "short_key32": ((110, 0, 0, 110), 150, lambda: _range(130, 150, 300, 7)),
    "short_key64": ((22076, 0, 0, 22076), 200, lambda: _range(150, 190, 300, 8)),
    "short_full": ((109, 0, 0, 109), 150, lambda: [150] * 300),
    # tile kernels
    "tile16": ((63, 0, 0, 64), 600, lambda: _range(150, 400, 20, 9)),
    "tile16_i16": ((255, 0, 0, 256), 600, lambda: _range(150, 400, 20, 10)),
    "tiles_key64": ((5243, 0, 0, 5243), 600, lambda: _range(150, 400, 20, 11)),
    "tile16_window": ((10, 2, 3, 4), 5000, lambda: _input4_lens(20, 12)),
    # 32 records: the sliding-window plan takes groups of 16 that are at least 0.8 full
    "tile16_slide": ((10, 2, 3, 4), 2000, lambda: _range(400, 900, 32, 13)),
    "mfma": ((2, 2, 1, 10), 1489, lambda: _range(56, 1152, 6, 14)),  # input3's shape
    "mixed": ((10, 2, 3, 4), 150, _mixed_lens),
    # feature kernels (profile, top-K, hits, summary, targets, report): test_gpu_topk.py's tile-edge batch
    "profile": ((10, 2, 3, 4), TILE_L1, lambda: TILE_LENS * 3),
    # host forms: a few hundred short records, so an engine of 100-record chunks takes several
    "host": ((10, 2, 3, 4), 90, lambda: _range(1, 80, 350, 15)),
}


@lru_cache(maxsize=None)
def family_case(name: str, c0: int = 32) -> SliceCase:
    weights, L1, lens = FAMILIES[name]
    seed = sorted(FAMILIES).index(name)
    seq1 = seq_no_equal_neighbours(np.random.default_rng(1000 + seed), L1)
    return slice_case(weights, seq1, lens(), c0, seed)


# ---- far placements: the slice inside an arena, its offsets past 2^31 and 2^32 ---------------------------------------
# An arena is one buffer of letter 1: FRONT guard bytes, then the view that is passed as ``codes`` (16-byte aligned).
# Offsets are relative to the view. A reader that truncates an offset to 32 bits still reads inside the arena — valid
# letters, so wrong rows and never an access outside the allocation:
#   * uint32:  2^32 + r -> r, in the view's first WINDOW bytes;
#   * int32:   2^31 + r -> r - 2^31, in the guard's first WINDOW bytes; 2^32 - x -> -x, in the guard's last WINDOW bytes
#     (the records below the boundary of ``across32`` / ``inside32``); 2^32 + r -> r as above.
# Every r and x is below R_MAX, so with HEAD, TAIL and the slice itself everything lands in LANDING. A host mapping
# (zero pages) writes letter 1 to LANDING and the patch only; a device arena is filled with 1 as a whole.
FRONT = 1 << 31
VIEW = (1 << 32) + (1 << 24)
ARENA = FRONT + VIEW
R_MAX = 2 << 20
WINDOW = 4 << 20
LANDING = ((0, WINDOW), (FRONT - WINDOW, 2 * WINDOW))  # (start, bytes) in the arena: guard head | guard end + view head
PLACEMENTS = ("bit31", "hi1", "across31", "across32", "inside32")
FEW = (0, 1, 3, 13, 15)  # first-letter residues for the kernels that stage letters in granules


def far_c0(sub: Problem, placement: str, s: int = 0, j=None) -> int:
    """The first offset (relative to the view) of a named placement. ``s``: a residue for ``bit31`` / ``hi1``; ``j``:
    the record at the boundary (default: the middle one) for the others."""
    o = sub.offsets
    j = sub.n // 2 if j is None else int(j)
    if placement in ("bit31", "hi1"):
        c0 = (1 << (31 if placement == "bit31" else 32)) + 32 + s
    elif placement in ("across31", "across32"):  # records below and above the boundary, which lies between two
        assert 0 < j < sub.n and s == 0
        c0 = (1 << int(placement[-2:])) - int(o[j])
    elif placement == "inside32":  # the boundary inside record j (by default the middle record, or the next of 2 letters)
        while o[j + 1] - o[j] < 2:
            j += 1
        L = int(o[j + 1] - o[j])
        assert L >= 2 and s == 0
        c0 = (1 << 32) - int(o[j]) - L // 2
    else:
        raise ValueError(f"placement: one of {PLACEMENTS}")
    assert int(o[-1]) + HEAD + TAIL + 64 < R_MAX  # every r and x stays below R_MAX
    return c0


def far_case(name: str, placement: str, s: int = 0, j=None) -> SliceCase:
    """The family's slice at a far placement: the same records as ``family_case(name)``, absolute offsets."""
    return family_case(name, far_c0(family_case(name).sub, placement, s, j))


def host_arena():
    """An anonymous mapping of the arena's layout as a uint8 array, LANDING holding letter 1 -> (arena, view). The
    mapping is untouched elsewhere (zero pages, which cost no memory)."""
    import mmap

    arena = np.frombuffer(mmap.mmap(-1, ARENA), np.uint8)
    for lo, nb in LANDING:
        arena[lo:lo + nb] = 1
    view = arena[FRONT:]
    assert view.ctypes.data % 16 == 0
    return arena, view


def lay(view, case: SliceCase, fill: str):
    """Writes the case's patch into the view -> (at, bytes) for ``unlay``."""
    at, letters = case.patch(fill)
    view[at:at + letters.shape[0]] = letters
    return at, letters.shape[0]


def unlay(view, at: int, nbytes: int):
    view[at:at + nbytes] = 1


# numpy models of a wrong reader of 64-bit offsets. The truncating ones keep a record's length (end - start wraps back
# to it in 32-bit arithmetic); the others change the end or the whole offset.
WRONG_READERS = ("uint32", "int32", "end_takes_start_high", "words_swapped")


def wrong_reader_spans(offsets, model: str):
    """[(start, length)] per record as the wrong reader sees them, in Python ints."""
    o = [int(x) for x in offsets]
    m32 = (1 << 32) - 1
    spans = []
    for a, b in zip(o[:-1], o[1:]):
        if model == "uint32":
            spans.append((a & m32, b - a))
        elif model == "int32":
            t = a & m32
            spans.append((t - (1 << 32) if t >> 31 else t, b - a))
        elif model == "end_takes_start_high":
            spans.append((a, max(0, ((a >> 32 << 32) | (b & m32)) - a)))
        elif model == "words_swapped":
            a2, b2 = ((a & m32) << 32) | (a >> 32), ((b & m32) << 32) | (b >> 32)
            spans.append((a2, max(0, min(b2 - a2, b - a))))
        else:
            raise ValueError(f"model: one of {WRONG_READERS}")
    return spans


def wrong_reader_problem(arena, case: SliceCase, model: str):
    """The records the wrong reader takes out of the arena, as a Problem from offset 0 -> (problem, changed): None
    when a read leaves the arena (such a reader cannot return the rows at all); ``changed``: whether the model reads
    any record elsewhere or at another length than the right reader."""
    spans = wrong_reader_spans(case.offsets, model)
    right = list(zip((int(x) for x in case.offsets[:-1]), (int(x) for x in np.diff(case.offsets))))
    changed = spans != right
    if any(FRONT + a < 0 or FRONT + a + n > arena.shape[0] for a, n in spans):
        return None, changed
    recs = [arena[FRONT + a:FRONT + a + n] for a, n in spans]
    offsets = np.concatenate([[0], np.cumsum([r.shape[0] for r in recs])]).astype(np.int64)
    codes = np.concatenate(recs) if recs else np.zeros(0, np.uint8)
    return Problem(case.sub.weights, case.sub.seq1, codes, offsets), changed


# ---- packed letters at far positions ---------------------------------------------------------------------------------
def place_bits(buf, bit_pos: int, value: int, nbits: int):
    """Writes the ``nbits`` low bits of ``value`` at bit ``bit_pos`` of the little-endian bit stream ``buf``
    (anything with byte slices: a numpy array, or an adapter over a device tensor). The two edge bytes are read,
    modified and written back: the neighbours' bits stay what they were. -> (first byte, bytes) written."""
    b0, sh, b1 = bit_pos >> 3, bit_pos & 7, (bit_pos + nbits + 7) >> 3
    old = int.from_bytes(bytes(np.asarray(buf[b0:b1])), "little")
    mask = ((1 << nbits) - 1) << sh
    new = (old & ~mask) | ((int(value) << sh) & mask)
    buf[b0:b1] = np.frombuffer(new.to_bytes(b1 - b0, "little"), np.uint8)
    return b0, b1 - b0


def pack33_int(letters) -> tuple:
    """Letters (a multiple of 7) as P33 fields in one Python int -> (value, bits): field f holds
    sum (letter[7f + i] - 1) 26^i at bits [33f, 33f + 33)."""
    v = [int(x) for x in letters]
    assert len(v) % 7 == 0 and all(1 <= x <= 26 for x in v)
    value = 0
    for f in range(len(v) // 7):
        value |= sum((v[7 * f + i] - 1) * 26 ** i for i in range(7)) << (33 * f)
    return value, 33 * (len(v) // 7)


def pack5_int(letters) -> tuple:
    """Letters as a 5-bit stream in one Python int -> (value, bits): letter j at bits [5j, 5j + 5)."""
    value = 0
    for j, x in enumerate(letters):
        value |= int(x) << (5 * j)
    return value, 5 * len(letters)


def unpack33_int(stream: int, first_bit: int, c0: int, n: int) -> np.ndarray:
    """Letters c0 .. c0 + n of a P33 stream held as a Python int whose bit 0 is the stream's bit ``first_bit``."""
    out = np.empty(n, np.uint8)
    for i in range(n):
        f, d = divmod(c0 + i, 7)
        out[i] = ((stream >> (33 * f - first_bit)) & ((1 << 33) - 1)) // 26 ** d % 26 + 1
    return out


def _ceil_div(a, b):
    return -(-a // b)


def packed_placements(letters: str):
    """[(name, c0)]: first letter indices at which the packed stream's bit position, its byte position and the letter
    index itself lie just past 2^31 and 2^32, each at several phases of the first letter inside its field (P33: c0 mod
    7 in 0, 3, 6) or byte group (5-bit: every c0 mod 8)."""
    out = []
    for what in ("bit", "byte", "letter"):
        for k in (31, 32):
            if letters == "p33":
                f0 = {"bit": (1 << k) // 33 + 1, "byte": _ceil_div(1 << (k + 3), 33), "letter": _ceil_div(1 << k, 7)}[what]
                out += [(f"{what}{k}_ph{ph}", 7 * f0 + ph) for ph in (0, 3, 6)]
            elif letters == "p5":
                lo = {"bit": (1 << k) // 5 + 1, "byte": _ceil_div(1 << (k + 3), 5), "letter": 1 << k}[what]
                out += [(f"{what}{k}_ph{ph}", lo + (ph - lo) % 8) for ph in range(8)]
            else:
                raise ValueError("letters: p33 or p5")
    return out


def packed_position(letters: str, c0: int) -> dict:
    """Bit, byte and letter position of letter c0's field (P33) or of the letter itself (5-bit)."""
    bit = 33 * (c0 // 7) if letters == "p33" else 5 * c0
    return {"bit": bit, "byte": bit >> 3, "letter": c0}


@dataclass(frozen=True)
class PackedCase:
    case: SliceCase   # the slice with absolute letter offsets c0 + sub.offsets
    letters: str      # "p33" or "p5"

    def run(self, fill: str):
        """(bit position, value, bits) of the packed run: the pad letters that share the first field (or byte group),
        the slice's letters and neighbours behind them, from the project's Python-int packing."""
        c0 = self.case.c0
        if self.letters == "p33":
            ph = c0 % 7
            laid = self.case._laid(fill, ph, True)
            laid = laid[:7 * ((ph + int(self.case.sub.offsets[-1]) + 6) // 7 + 1)]  # whole fields, one of neighbours
            value, bits = pack33_int(laid)
            return 33 * (c0 // 7), value, bits
        ph = c0 % 8
        value, bits = pack5_int(self.case._laid(fill, ph, True))
        return 5 * (c0 - ph), value, bits

    def lay(self, view, fill: str):
        """Writes the run into the view -> (first byte, bytes) for ``unlay``."""
        return place_bits(view, *self.run(fill))


def packed_case(name: str, letters: str, c0: int) -> PackedCase:
    return PackedCase(family_case(name, c0), letters)
