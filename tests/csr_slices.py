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
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from mpi_openmp_cuda_amd import Problem
from mpi_openmp_cuda_amd.utils.synthetic import seq_no_equal_neighbours

FILLS = ("A", "continue")
TAIL = 48  # neighbour letters behind the slice: three 16-byte granules


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

    def storage(self, fill: str = "A", tail: bool = True) -> np.ndarray:
        """uint8 [c0 + letters (+ TAIL)]: the neighbours in front, the slice's letters, the neighbours behind;
        ``tail=False`` ends at the slice's last letter."""
        seq1, L1 = self.sub.seq1, self.sub.L1
        total = int(self.sub.offsets[-1])
        out = np.ones(self.c0 + total + (TAIL if tail else 0), np.uint8)
        out[self.c0:self.c0 + total] = self.sub.codes
        if fill == "continue":
            first = self.first_at if self.first_at >= 0 else 0
            out[:self.c0] = seq1[(first - self.c0 + np.arange(self.c0)) % L1]  # ..., Seq1[first - 1] | the slice
            if tail:
                nxt = self.next_at if self.next_at >= 0 else 0
                out[self.c0 + total:] = seq1[(nxt + np.arange(TAIL)) % L1]
        elif fill != "A":
            raise ValueError(f"fill: one of {FILLS}")
        assert out.min() >= 1 and out.max() <= 26  # never letter 0: its table row is all zero and would hide a leak
        return out


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
