"""Synthetic problems shaped like the reference fixtures (no datasets are available offline).

The benchmark metric (BASELINE.json) is quoted "on input6.txt array ... on synthetic/random-init arrays
of the input6.txt shape": input6 has W = 4 3 2 10, |Seq1| = 26 and Seq2 lengths 6..11
(/root/reference/input6.txt). ``make_synthetic("input6", n)`` draws n records of that shape.
Other shapes mirror input3 (long Seq2, L2 > 1024 present), input4 (longest Seq1, tiny Seq2) and the
PDF limits (|Seq1| = 3000, |Seq2| <= 2000).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ..models.problem import Problem
from ..models.scoring import Weights


@dataclass(frozen=True)
class Shape:
    weights: tuple
    L1: int
    l2_min: int
    l2_max: int


SHAPES = {
    "input6": Shape((4, 3, 2, 10), 26, 6, 11),
    "input1": Shape((100, 2, 3, 4), 51, 32, 41),
    "input3": Shape((2, 2, 1, 10), 1489, 56, 1152),
    "input4": Shape((10, 2, 3, 4), 2976, 5, 82),
    "limits": Shape((10, 2, 3, 4), 3000, 1, 2000),
    # between the reference shapes: records too long for the swipe kernel (> 64 letters) whose offset range
    # still fits a wave (<= 64 lanes): the lane-per-offset short kernel's regime
    "mid": Shape((10, 2, 3, 4), 130, 67, 85),
    # input6's lengths under a heavy weight (W1 = 300): no room for k in the int16 keys, the RK swipe form
    "heavy6": Shape((300, 3, 2, 10), 26, 6, 11),
    # long records under weights past the int8 difference profile (W1 + max(W2, W3, W4) > 127)
    "heavy3": Shape((200, 10, 10, 10), 1489, 56, 1152),
    "heavy4": Shape((120, 20, 1, 1), 2976, 5, 82),
    "heavylim": Shape((200, 10, 10, 10), 3000, 1, 2000),  # limits' lengths, int16 profile (sliding windows)
    "mid3k": Shape((10, 2, 3, 4), 2000, 400, 900),  # L1 past the widened image, records past a widened window
}


def make_synthetic(shape: str = "input6", n_records: int = 1000, seed: int = 0) -> Problem:
    return make_shape(SHAPES[shape], n_records, seed)


def make_shape(s: Shape, n_records: int = 1000, seed: int = 0) -> Problem:
    """Random Seq1 of s.L1 letters and n_records records of s.l2_min..s.l2_max random letters."""
    rng = np.random.default_rng(seed)
    seq1 = rng.integers(1, 27, size=s.L1, dtype=np.uint8)
    lengths = rng.integers(s.l2_min, s.l2_max + 1, size=n_records, dtype=np.int64)
    offsets = np.zeros(n_records + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    codes = rng.integers(1, 27, size=int(offsets[-1]), dtype=np.uint8)
    return Problem(Weights.of(s.weights), seq1, codes, offsets)


def fill_codes(out: np.ndarray, seed: int, chunk: int = 1 << 26):
    """Fills a (possibly huge / shared) uint8 array with random letter codes, chunk by chunk."""
    rng = np.random.default_rng(seed)
    for b in range(0, out.shape[0], chunk):
        e = min(out.shape[0], b + chunk)
        out[b:e] = rng.integers(1, 27, size=e - b, dtype=np.uint8)


def seq_no_equal_neighbours(rng, L: int, alphabet: int = 26) -> np.ndarray:
    """L random letter codes (1..alphabet) with s[i] != s[i-1] for every i. In such a Seq1 an exact copy of
    Seq1[p : p + L2] has no full-score rival through the neighbouring offset: with Seq1[p-1] == Seq1[p] the
    candidate (p-1, k = 1) would tie the copy at p and come first in the reference order."""
    if alphabet < 2:
        raise ValueError("no two neighbours can differ in an alphabet of one letter")
    s = np.empty(L, dtype=np.uint8)
    if L:
        s[0] = rng.integers(1, alphabet + 1)
        # 1..alphabet-1 steps round the alphabet: never back onto the previous letter
        steps = rng.integers(1, alphabet, size=L - 1)
        s[1:] = (int(s[0]) - 1 + np.cumsum(steps)) % alphabet + 1
    return s


def _no_equal_neighbours(s: np.ndarray) -> bool:
    return bool((s[1:] != s[:-1]).all())


def _records(weights, seq1: np.ndarray, recs) -> Problem:
    lengths = np.array([len(r) for r in recs], dtype=np.int64)
    offsets = np.zeros(len(recs) + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    codes = np.concatenate(recs).astype(np.uint8) if len(recs) else np.zeros(0, np.uint8)
    return Problem(Weights.of(weights), seq1, codes, offsets)


def make_planted(L1: int, L2: int, weights, positions=None, seed: int = 0):
    """A problem whose record i is Seq1[p_i : p_i + L2] for every p_i in ``positions`` (default: every offset
    0 .. L1 - L2), on a Seq1 without equal neighbours: a chosen offset is the winner. Returns (problem,
    positions). With W1 > 0 the expected result of record i is (W1 * L2, p_i, 0) under either semantics for
    p_i <= L1 - L2 - 1; for p_i = L1 - L2 under the spec semantics only (the reference semantics never try
    that offset: an oracle decides the record)."""
    if not 0 < L2 <= L1:
        raise ValueError("need 0 < L2 <= L1")
    rng = np.random.default_rng(seed)
    seq1 = seq_no_equal_neighbours(rng, L1)
    pos = np.arange(L1 - L2 + 1, dtype=np.int64) if positions is None else np.asarray(positions, dtype=np.int64)
    if pos.size and (pos.min() < 0 or pos.max() > L1 - L2):
        raise ValueError("positions must lie in 0 .. L1 - L2")
    n = pos.shape[0]
    codes = seq1[(pos[:, None] + np.arange(L2)[None, :]).reshape(-1)] if n else np.zeros(0, np.uint8)
    offsets = np.arange(n + 1, dtype=np.int64) * L2
    return Problem(Weights.of(weights), seq1, np.ascontiguousarray(codes, dtype=np.uint8), offsets), pos


def planted_expected(problem: Problem, positions, semantics) -> np.ndarray:
    """The (score, n, k) rows make_planted's construction implies: (W1 * L2, p, 0) for every record, except
    that under the reference semantics a record planted at the final offset L1 - L2 (which those semantics
    never try) gets the pure-Python prefix oracle's answer."""
    from ..models.reference import prefix_oracle
    from ..models.scoring import Semantics, score_table

    pos = np.asarray(positions, dtype=np.int64)
    L2 = int(problem.offsets[1] - problem.offsets[0]) if problem.n else 0
    out = np.stack([np.full(pos.shape[0], problem.weights.as_list()[0] * L2, np.int64), pos,
                    np.zeros(pos.shape[0], np.int64)], axis=1).astype(np.int32)
    if Semantics.parse(semantics) == Semantics.REFERENCE and L2 < problem.L1:
        table = score_table(problem.weights)
        for i in np.nonzero(pos == problem.L1 - L2)[0]:
            out[i] = prefix_oracle(table, problem.seq1, problem.codes[problem.offsets[i]:problem.offsets[i + 1]],
                                   semantics)
    return out


def differing(got, want, positions) -> str:
    """Failure message for result rows that differ on a planted problem ("" when none do): how many, the first
    few planted positions with their values mod 128 (the tile kernels' sub-tile width), and the rows."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"shapes differ: got {got.shape} want {want.shape}"
    bad = np.nonzero((got != want).any(axis=1))[0]
    if bad.size == 0:
        return ""
    p = np.asarray(positions)[bad[:8]]
    return (f"{bad.size} of {len(positions)} records differ; first p = {p.tolist()} (mod 128: {(p % 128).tolist()}) "
            f"got {got[bad[:8]].tolist()} want {want[bad[:8]].tolist()}")


def make_planted_ties(L1: int, L2: int, weights, pairs, seed: int = 0):
    """A problem with one record per (a, b) in ``pairs`` (a + L2 <= b, b + L2 <= L1): Seq1[a : a + L2] is
    copied to b and is the record, so two offsets reach the full score W1 * L2 and the smaller one must win:
    the expected result is (W1 * L2, a, 0). Segments of different pairs must not overlap. The letter after
    every copy is re-drawn so that Seq1 keeps no equal neighbours (it lies in no segment, or the pair set is
    refused). Returns (problem, pairs as an int64 [n, 2] array)."""
    rng = np.random.default_rng(seed)
    seq1 = seq_no_equal_neighbours(rng, L1)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    owned = np.zeros(L1, dtype=bool)
    for a, b in pairs:
        if not (0 <= a and a + L2 <= b and b + L2 <= L1):
            raise ValueError(f"pair ({a}, {b}): need 0 <= a, a + L2 <= b and b + L2 <= L1")
        if owned[a:a + L2].any() or owned[b:b + L2].any():
            raise ValueError(f"pair ({a}, {b}) overlaps another pair's segment")
        owned[a:a + L2] = True
        owned[b:b + L2] = True
    for a, b in pairs:
        # a copy that follows its source directly meets the source's last letter with the source's first one:
        # the last letter is re-drawn before it is copied (L2 >= 2: it differs from its own left neighbour too)
        if b == a + L2 and L2 >= 2 and seq1[b - 1] == seq1[a]:
            seq1[b - 1] = next(c for c in rng.permutation(26) + 1 if c != seq1[b - 2] and c != seq1[a])
        seq1[b:b + L2] = seq1[a:a + L2]
    # the copy's first letter may now equal the one before it, its last the one after: both neighbours lie
    # outside the copy, and are re-drawn where no segment owns them
    for a, b in pairs:
        for q in (b - 1, b + L2):
            if not 0 <= q < L1:
                continue
            left = seq1[q - 1] if q > 0 else 0
            right = seq1[q + 1] if q + 1 < L1 else 0
            if seq1[q] != left and seq1[q] != right:
                continue
            if owned[q]:
                raise ValueError(f"pair ({a}, {b}): the splice at {q} meets another segment with equal letters")
            seq1[q] = next(c for c in rng.permutation(26) + 1 if c != left and c != right)
    assert _no_equal_neighbours(seq1), "planted ties: equal neighbours left in Seq1"
    recs = [seq1[a:a + L2].copy() for a, _ in pairs]
    for (a, b), r in zip(pairs, recs):
        assert np.array_equal(seq1[b:b + L2], r)
    return _records(weights, seq1, recs), pairs


A, Z = 1, 26  # letter codes of 'A' and 'Z': in no group together, so a pair is '$' or ' '


def make_extreme(L1: int, l2_min: int, l2_max: int, weights, copies: int = 1, seed: int = 0) -> Problem:
    """Adversarial records for the kernels' integer bounds (csrc/include/moc/kernel_bounds.hpp): Seq1 =
    "AZAZ...", and records that are pieces of Seq1 at even offsets (with W1 = W4 every step adds the largest
    difference Dt = W1 + W4, so |D| reaches 2 W L2) and at odd ones (-(W1 + W4)), constant 'A' / 'Z' records,
    A/Z noise and random letters, at the extreme lengths of [l2_min, l2_max]. The periodic Seq1 makes most
    offsets tie, so the reference's tie-break (smallest offset, then k = 0) decides. ``copies`` repeats the
    list (shuffled) so the GPU kernels see every record length mixed in their waves."""
    rng = np.random.default_rng(seed)
    s1 = np.where(np.arange(L1) % 2 == 0, A, Z).astype(np.uint8)
    recs = []
    for L2 in sorted({l2_min, l2_max, (l2_min + l2_max) // 2, max(l2_min, l2_max - 1)}):
        for at in (0, 1, L1 - L2, L1 - L2 - 1):
            if 0 <= at and at + L2 <= L1:
                recs.append(s1[at:at + L2].copy())
        recs.append(np.full(L2, A, np.uint8))
        recs.append(np.full(L2, Z, np.uint8))
        recs.append(np.where(rng.integers(0, 2, L2) == 0, A, Z).astype(np.uint8))
        recs.append(rng.integers(1, 27, size=L2, dtype=np.uint8))
    order = np.concatenate([rng.permutation(len(recs)) for _ in range(copies)])
    lengths = np.array([len(recs[i]) for i in order], dtype=np.int64)
    offsets = np.zeros(len(order) + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    codes = np.concatenate([recs[i] for i in order]) if len(order) else np.zeros(0, np.uint8)
    return Problem(Weights.of(weights), s1, codes, offsets)
