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


# ---- wire-decoder cases ---------------------------------------------------------------------------------
# Inputs for the decoders of the wire formats (docs/WIRE_FORMATS.md): P33 fields on every digit carry and at every
# bit phase, every base-6 octet, every narrow length field, as problems whose result rows read the decoded letters
# and lengths back (tests/decoder_cases.py holds the case lists, tests/test_decoder_cases.py proves the claims).
P33_P = 26 ** 4          # a P33 field x = A * 26^4 + B: the device decoders split it there
P33_TOP = 26 ** 7 - 1    # the largest field: seven letters 'Z'
OCTETS = 6 ** 8          # base-6 octet values
OCTET_SLICE = 6 ** 7     # octets that share a top digit


def p33_boundary_fields() -> np.ndarray:
    """The uint64 P33 field values on a digit carry, 41 230 of them: q P - 1 and q P for q = 1 .. 26^3 - 1 (every
    carry into digits 4..6); A P + 676 m - 1 and A P + 676 m for m = 1..675 and A in {0, 8788, 26^3 - 1} (every carry
    into digits 2..3, at the smallest, a middle and the largest upper half); v, 676 v and P v for v = 0..675 (every
    digit pair at each of the three pair positions); 0 and 26^7 - 1."""
    q = np.arange(1, 26 ** 3, dtype=np.uint64) * np.uint64(P33_P)
    parts = [np.stack([q - np.uint64(1), q], axis=1).reshape(-1)]
    m = np.arange(1, 676, dtype=np.uint64) * np.uint64(676)
    for a in (0, 8788, 26 ** 3 - 1):
        at = np.uint64(a * P33_P) + m
        parts.append(np.stack([at - np.uint64(1), at], axis=1).reshape(-1))
    v = np.arange(676, dtype=np.uint64)
    parts.append(np.stack([v, v * np.uint64(676), v * np.uint64(P33_P)], axis=1).reshape(-1))
    parts.append(np.array([0, P33_TOP], dtype=np.uint64))
    return np.concatenate(parts)


def p33_phase_fields() -> np.ndarray:
    """2 x 32 runs of 64 consecutive uint64 fields (4096 fields): 26^7 - 1 at field f of its run and 0 everywhere else,
    for f = 0..31, then the inverse, 0 at field f and 26^7 - 1 everywhere else. A run is 64 fields, so field f of a
    run lies at bit phase 33 f mod 32 = f: the largest and the smallest field at each of the 32 phases beside the
    opposite fill, where a mask or shift that leaks shows."""
    runs = np.zeros((2, 32, 64), dtype=np.uint64)
    runs[1] = P33_TOP
    f = np.arange(32)
    runs[0, f, f] = P33_TOP
    runs[1, f, f] = 0
    return runs.reshape(-1)


def p33_field_letters(fields) -> np.ndarray:
    """The uint8 letter codes of P33 fields, seven per field: digit j of the field's value in base 26, plus 1, digit 0
    first."""
    x = np.asarray(fields, dtype=np.uint64)
    if x.size and int(x.max()) > P33_TOP:
        raise ValueError("a P33 field is below 26^7")
    digits = (x[:, None] // (np.uint64(26) ** np.arange(7, dtype=np.uint64))[None, :]) % np.uint64(26)
    return (digits + np.uint64(1)).astype(np.uint8).reshape(-1)


READOUT_WEIGHTS = (1, 0, 0, 0)


def make_letter_readout(letters):
    """One-letter records that read a decoded letter stream back: Seq1 = "AB...ZA" (27 letters: the second 'A' gives
    the reference semantics, which never try the last offset, an offset for 'Z'), weights (1, 0, 0, 0), record i the
    single letter ``letters[i]``. Its only matching offset below 26 is letters[i] - 1 ('A' also matches at 26, the
    smaller offset wins) and a record of one letter has no mutant, so the row is (1, letters[i] - 1, 0) under either
    semantics. All lengths are 1: base 6 above base 1. Returns (problem, rows)."""
    letters = np.ascontiguousarray(letters, dtype=np.uint8)
    if letters.size and (letters.min() < 1 or letters.max() > 26):
        raise ValueError("letter codes are 1..26")
    seq1 = np.concatenate([np.arange(1, 27), [1]]).astype(np.uint8)
    n = letters.shape[0]
    prob = Problem(Weights.of(READOUT_WEIGHTS), seq1, letters, np.arange(n + 1, dtype=np.int64))
    rows = np.stack([np.ones(n, np.int64), letters.astype(np.int64) - 1, np.zeros(n, np.int64)], axis=1)
    return prob, rows.astype(np.int32)


def octet_digits(values) -> np.ndarray:
    """The 8 base-6 digits of every octet value, digit 0 first: int64 [n, 8]."""
    v = np.asarray(values, dtype=np.int64)
    return (v[:, None] // (6 ** np.arange(8, dtype=np.int64))[None, :]) % 6


def _copies(weights, seq1: np.ndarray, lengths: np.ndarray, starts: np.ndarray) -> Problem:
    """Record i = ``lengths[i]`` letters of Seq1 (read cyclically) from ``starts[i]``."""
    lengths = np.asarray(lengths, dtype=np.int64)
    offsets = np.zeros(lengths.shape[0] + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    within = np.arange(int(offsets[-1]), dtype=np.int64) - np.repeat(offsets[:-1], lengths)
    at = np.repeat(np.asarray(starts, dtype=np.int64), lengths) + within
    return Problem(Weights.of(weights), seq1, seq1[at % seq1.shape[0]], offsets)


OCTET_WEIGHTS = (3, 1, 2, 4)


def make_length_copies(lengths, seed=0):
    """One record per entry of ``lengths`` (each at most 25) that reads its own length back: Seq1 is the 26 distinct
    letters "AB...Z", record i a copy of Seq1[p_i : p_i + L_i] with a seeded p_i <= 25 - L_i, weights (3, 1, 2, 4). No
    other offset and no mutant matches every letter, and p_i + L_i < 26 is an offset both semantics try, so the row is
    (3 L_i, p_i, 0) — a wrong length breaks the score, and every later start of its tile with it. Returns (problem,
    rows)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    if lengths.size and (lengths.min() < 1 or lengths.max() > 25):
        raise ValueError("lengths of 1..25")
    p = np.random.default_rng(seed).integers(0, 26 - lengths)  # 0 .. 25 - L
    prob = _copies(OCTET_WEIGHTS, np.arange(1, 27, dtype=np.uint8), lengths, p)
    rows = np.stack([OCTET_WEIGHTS[0] * lengths, p, np.zeros_like(p)], axis=1).astype(np.int32)
    return prob, rows


def make_octet_copies(top: int, rot: int = 0, base: int = 1, seed: int = 0):
    """Every base-6 octet with top digit ``top`` as record lengths: ``base`` + digit j, j = 0..7, of every value in
    [top 6^7, (top + 1) 6^7), after 8 ``rot`` records of ``base`` letters (``rot`` whole zero octets: with three
    octets to an 8-byte word, rot = 0, 1, 2 put every value at each of the three positions of a word), as
    make_length_copies' records: the row is (3 L_i, p_i, 0). 2 239 488 + 8 rot records. Returns (problem, rows)."""
    if not (0 <= top <= 5 and rot >= 0 and 1 <= base and base + 5 <= 25):
        raise ValueError("need 0 <= top <= 5, rot >= 0 and 1 <= base <= 20")
    values = np.arange(top * OCTET_SLICE, (top + 1) * OCTET_SLICE, dtype=np.int64)
    lengths = np.concatenate([np.full(8 * rot, base, np.int64), base + octet_digits(values).reshape(-1)])
    return make_length_copies(lengths, [seed, top, rot, base])


def make_octet_tail(values, tail: int, base: int = 1, seed: int = 0):
    """A batch that ends inside an octet: ``base`` + digit of every octet of ``values`` but only the first ``tail``
    (1..7) digits of the last one, as make_length_copies' records. The kernels that take four lengths per load decode
    the records after the last whole four one at a time. Returns (problem, rows)."""
    if not 1 <= tail <= 7:
        raise ValueError("tail: 1..7 records of the last octet")
    lengths = base + octet_digits(values).reshape(-1)
    return make_length_copies(lengths[:lengths.shape[0] - 8 + tail], [seed, tail, base])


NARROW_PERIOD = {3: 8, 4: 2, 8: 4}  # records per byte pattern (3-bit), per byte (4-bit), per 4-record load (8-bit)


def narrow_exhaustive_lengths(bits: int, base: int, top: int = None) -> np.ndarray:
    """Record lengths holding every value of a ``bits``-bit length field (3-bit: 0..7, 4-bit: 0..15 above ``base``;
    8-bit: the lengths 1 .. ``top``, default 128, ``base`` ignored) at every index residue that places the field
    differently (index mod 8 for 3-bit fields, mod 2 for nibbles, mod 4 for the bytes a thread loads four at a time),
    once between neighbours of the smallest value and once between neighbours of the largest: one group of
    ``NARROW_PERIOD[bits]`` records per (fill, value, residue), all of the fill but the record at the residue."""
    if bits not in NARROW_PERIOD:
        raise ValueError("bits: 3, 4 or 8")
    period = NARROW_PERIOD[bits]
    values = np.arange(1, (128 if top is None else int(top)) + 1) if bits == 8 else int(base) + np.arange(1 << bits)
    groups = []
    for fill in (values[0], values[-1]):
        g = np.full((values.shape[0], period, period), fill, dtype=np.int64)  # [value, residue, record of the group]
        r = np.arange(period)
        g[:, r, r] = values[:, None]
        groups.append(g.reshape(-1))
    return np.concatenate(groups)


def make_narrow_exhaustive(bits: int, L1: int, base: int = 5, top: int = None, weights=(3, 1, 2, 4), seed: int = 0):
    """narrow_exhaustive_lengths as a problem: Seq1 of ``L1`` random letters without equal neighbours, record i a copy
    of the window of Seq1 from a seeded start (read cyclically where the record is longer than what follows it). The
    reference is the CPU engine. Returns the problem."""
    lengths = narrow_exhaustive_lengths(bits, base, top)
    rng = np.random.default_rng([seed, bits, L1])
    seq1 = seq_no_equal_neighbours(rng, L1)
    return _copies(weights, seq1, lengths, rng.integers(0, L1, lengths.shape[0]))


def short_octets() -> np.ndarray:
    """The octet values whose upper or lower half (v = 1296 h + l) is at an end of its range: h in {0, 1295} with
    every l, l in {0, 1295} with every h — 5 180 values, where the quotient by 6^4 that splits an octet is 0 or
    largest, or steps with the smallest or largest remainder."""
    ends, every = np.array([0, 1295], dtype=np.int64), np.arange(1296, dtype=np.int64)
    v = np.concatenate([(ends[:, None] * 1296 + every[None, :]).reshape(-1),
                        (every[:, None] * 1296 + ends[None, :]).reshape(-1)])
    return np.unique(v)


def make_short_octets(L1: int = 200, base: int = 150, weights=(3, 2, 1, 4), seed: int = 0) -> Problem:
    """short_octets as record lengths ``base`` + digit (150..155) of random letters against a random Seq1 of ``L1``
    (200): the lane-per-offset short kernel's regime with base-6 lengths. The reference is the CPU engine."""
    lengths = base + octet_digits(short_octets()).reshape(-1)
    rng = np.random.default_rng([seed, L1, base])
    seq1 = rng.integers(1, 27, size=L1, dtype=np.uint8)
    offsets = np.zeros(lengths.shape[0] + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    return Problem(Weights.of(weights), seq1, rng.integers(1, 27, size=int(offsets[-1]), dtype=np.uint8), offsets)
