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
    that offset: an oracle decides the record). The winner's k is always 0 here: make_planted_k,
    make_planted_k_ties and make_extreme_mutants plant a mutation point."""
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


# ---- planted mutation points ---------------------------------------------------------------------------
# B J O U X Z: in no conservation group (models/scoring.py), so against any other letter they score -W4
NEUTRAL = tuple(ord(c) - 64 for c in "BJOUXZ")
K_FAMILIES = ("k", "inside", "own", "shadow", "extreme")


def _skipped(seq1: np.ndarray, p: int, L2: int, k: int) -> np.ndarray:
    """Seq1[p : p + k] ++ Seq1[p + k + 1 : p + L2 + 1]: L2 letters of Seq1 from p with the letter at p + k skipped."""
    return np.concatenate([seq1[p:p + k], seq1[p + k + 1:p + L2 + 1]]).astype(np.uint8)


def _neutral(rng, seq1: np.ndarray, q: int) -> int:
    """A neutral letter that differs from Seq1[q] and Seq1[q + 1], the two letters a record letter meets on the
    diagonals p and p + 1: it scores -W4 on both, so its step adds 0 to the diagonal difference D."""
    right = int(seq1[q + 1]) if q + 1 < seq1.shape[0] else 0
    free = [c for c in NEUTRAL if c != int(seq1[q]) and c != right]
    return int(free[int(rng.integers(0, len(free)))])


def _check_k_case(L1: int, p: int, L2: int, k: int):
    if not (L2 >= 2 and 1 <= k <= L2 - 1 and 0 <= p and p + L2 + 1 <= L1):
        raise ValueError(f"case (p={p}, L2={L2}, k={k}) on L1={L1}: need L2 >= 2, 1 <= k <= L2 - 1, p + L2 + 1 <= L1")


def make_planted_k(L1: int, cases, weights, seed: int = 0):
    """A problem with one record per (p, L2, k) in ``cases`` (1 <= k <= L2 - 1, p + L2 + 1 <= L1; lengths may
    differ) on a Seq1 without equal neighbours: the record is Seq1[p : p + L2 + 1] with the letter at p + k
    skipped, so its letters before k match on diagonal p and the rest on diagonal p + 1, and the mutant k at offset
    p is the only candidate with the full score. The expected row is (W1 * L2, p, k) under either semantics
    (planted_k_expected). Returns (problem, cases as an int64 [n, 3] array)."""
    rng = np.random.default_rng(seed)
    seq1 = seq_no_equal_neighbours(rng, L1)
    cases = np.asarray(cases, dtype=np.int64).reshape(-1, 3)
    for p, L2, k in cases:
        _check_k_case(L1, int(p), int(L2), int(k))
    return _records(weights, seq1, [_skipped(seq1, int(p), int(L2), int(k)) for p, L2, k in cases]), cases


def make_planted_k_ties(L1: int, family: str, cases, weights, seed: int = 0):
    """Ties that the mutation point's tie-break decides (first k with the largest diagonal difference D; k = 0
    wins a tie with D(L2); the smaller offset wins). One record per case; returns (problem, cases as int64 rows).

    ``inside``: (p, L2, j, k), 1 <= j < k: make_planted_k's record with its letters j .. k - 1 replaced by neutral
      ones (_neutral), so every k' in j .. k reaches the same score: the row is
      (W1 (L2 - (k - j)) - W4 (k - j), p, j).
    ``own``: (p, L2, k): Seq1[p : p + k] and then L2 - k neutral letters: D(k') = D(L2) for every k' >= k, the
      un-mutated candidate wins: (W1 k - W4 (L2 - k), p, 0) — while the prefix is long enough to beat chance
      elsewhere, so k >= max(5, L2 / 2) is required.
    ``shadow``: (p, L2), p >= 1: Seq1[p - 1] is set to Seq1[p] (the only equal neighbours; the case is refused if
      Seq1[p - 2] or Seq1[p + 1] equals them) and the record is Seq1[p : p + L2]: (p - 1, k = 1) and (p, 0) both
      score W1 L2 and the smaller offset wins: (W1 L2, p - 1, 1). p = L1 - L2 is allowed: the reference semantics
      never try that offset, but they try its shadow."""
    if family not in ("inside", "own", "shadow"):
        raise ValueError(f"unknown tie family {family!r}")
    rng = np.random.default_rng(seed)
    seq1 = seq_no_equal_neighbours(rng, L1)
    width = {"inside": 4, "own": 3, "shadow": 2}[family]
    cases = np.asarray(cases, dtype=np.int64).reshape(-1, width)
    recs = []
    if family == "inside":
        for p, L2, j, k in (tuple(int(v) for v in c) for c in cases):
            _check_k_case(L1, p, L2, k)
            if not 1 <= j < k:
                raise ValueError(f"case (p={p}, L2={L2}, j={j}, k={k}): need 1 <= j < k")
            r = _skipped(seq1, p, L2, k)
            for i in range(j, k):
                r[i] = _neutral(rng, seq1, p + i)
            recs.append(r)
    elif family == "own":
        for p, L2, k in (tuple(int(v) for v in c) for c in cases):
            _check_k_case(L1, p, L2, k)
            if k < max(5, (L2 + 1) // 2):
                raise ValueError(f"case (p={p}, L2={L2}, k={k}): the matching prefix needs k >= max(5, L2 / 2)")
            r = seq1[p:p + L2].copy()
            for i in range(k, L2):
                r[i] = _neutral(rng, seq1, p + i)
            recs.append(r)
    else:
        for p, L2 in (tuple(int(v) for v in c) for c in cases):
            if not (L2 >= 2 and 1 <= p and p + L2 <= L1):
                raise ValueError(f"case (p={p}, L2={L2}) on L1={L1}: need L2 >= 2, p >= 1 and p + L2 <= L1")
            seq1[p - 1] = seq1[p]
        for p, L2 in (tuple(int(v) for v in c) for c in cases):
            if seq1[p - 1] != seq1[p] or (p >= 2 and seq1[p - 2] == seq1[p]) or seq1[p + 1] == seq1[p]:
                raise ValueError(f"case (p={p}, L2={L2}): a third equal letter next to Seq1[{p - 1}] == Seq1[{p}]")
            recs.append(seq1[p:p + L2].copy())
        equal = np.nonzero(seq1[1:] == seq1[:-1])[0] + 1
        assert sorted(equal.tolist()) == sorted({int(p) for p, _ in cases}), "shadow ties: stray equal neighbours"
    return _records(weights, seq1, recs), cases


def make_extreme_mutants(L1: int, l2_min: int, l2_max: int, weights, copies: int = 1, seed: int = 0):
    """make_extreme's Seq1 "AZAZ..." with records that are pieces of it with one letter skipped (make_planted_k's
    construction) at p in {0, 1, 5} and k in {1, 2, L2 / 2, L2 - 2, L2 - 1}, for the lengths make_extreme uses,
    shuffled ``copies`` times. Every letter matches on the mutant's path and, Seq1 having period 2, at offset
    p mod 2 already: the row is (W1 L2, p mod 2, k). With W1 = W4 = W the winner's D(k) = 2 W k: at k = L2 - 1 one
    step under the 2 W L2 the kernels' bounds are set by, in a key whose k field holds its smallest value. A length
    no skipped piece fits (L2 + 1 > L1) gets the exact piece at 0 (k = 0), so that the batch keeps make_extreme's
    length range and with it the kernel form. Returns (problem, cases as int64 rows (p, L2, k) in record order)."""
    rng = np.random.default_rng(seed)
    s1 = np.where(np.arange(L1) % 2 == 0, A, Z).astype(np.uint8)
    recs, rows = [], []
    for L2 in sorted({l2_min, l2_max, (l2_min + l2_max) // 2, max(l2_min, l2_max - 1)}):
        ks = sorted({k for k in (1, 2, L2 // 2, L2 - 2, L2 - 1) if 1 <= k <= L2 - 1})
        fits = [(p, k) for p in (0, 1, 5) for k in ks if p + L2 + 1 <= L1]
        for p, k in fits:
            recs.append(_skipped(s1, p, L2, k))
            rows.append((p, L2, k))
        if not fits:
            if not 0 < L2 <= L1:
                raise ValueError(f"records of {L2} letters do not fit a Seq1 of {L1}")
            recs.append(s1[:L2].copy())
            rows.append((0, L2, 0))
    order = np.concatenate([rng.permutation(len(recs)) for _ in range(copies)])
    return _records(weights, s1, [recs[i] for i in order]), np.array([rows[i] for i in order], dtype=np.int64)


def planted_k_expected(problem: Problem, cases, family: str = "k") -> np.ndarray:
    """The int32 (score, n, k) rows the constructions above claim, under either semantics: ``family`` is "k"
    (make_planted_k), "inside" / "own" / "shadow" (make_planted_k_ties) or "extreme" (make_extreme_mutants)."""
    if family not in K_FAMILIES:
        raise ValueError(f"unknown family {family!r}")
    w1, _, _, w4 = problem.weights.as_list()
    c = np.asarray(cases, dtype=np.int64)
    c = c.reshape(-1, {"inside": 4, "shadow": 2}.get(family, 3))
    if c.shape[0] != problem.n:
        raise ValueError("one case per record")
    p, L2 = c[:, 0], c[:, 1]
    if family == "k":
        rows = (w1 * L2, p, c[:, 2])
    elif family == "inside":
        span = c[:, 3] - c[:, 2]
        rows = (w1 * (L2 - span) - w4 * span, p, c[:, 2])
    elif family == "own":
        rows = (w1 * c[:, 2] - w4 * (L2 - c[:, 2]), p, np.zeros_like(p))
    elif family == "shadow":
        rows = (w1 * L2, p - 1, np.ones_like(p))
    else:
        rows = (w1 * L2, p % 2, c[:, 2])
    return np.stack(rows, axis=1).astype(np.int32)
