"""Pure-Python oracles of the search, independent of the native code.

* ``brute_force`` replays the reference kernel's loops literally (cudaFunctions.cu:74-172, race-free
  reading): every (offset, mutant) candidate is re-scored from scratch, O(L1*L2^2).
* ``prefix_oracle`` is the O(L1*L2) closed form the engines implement, vectorised
  with numpy cumulative sums.
Both return (score, n, k) and follow the reference tie-break (first maximum in offset-major,
mutant-minor order, mutant 0 = no hyphen first).
"""
from __future__ import annotations

import numpy as np

from .scoring import Semantics, score_table

INT_MIN = -(2**31)


def brute_force(table: np.ndarray, s1: np.ndarray, s2: np.ndarray, semantics=Semantics.REFERENCE):
    L1, L2 = len(s1), len(s2)
    if L2 > L1:
        return (INT_MIN, 0, 0)
    if L2 == L1:
        return (int(sum(table[s2[i], s1[i]] for i in range(L2))), 0, 0)
    best = None
    for o in range(L1 - L2):
        for m in range(L2):
            s = 0
            for i in range(L2):
                j = i + o if (i < m or m == 0) else i + o + 1
                s += int(table[s2[i], s1[j]])
            if best is None or best[0] < s:
                best = (s, o, m)
    if Semantics.parse(semantics) == Semantics.SPEC:
        o = L1 - L2
        s = int(sum(table[s2[i], s1[i + o]] for i in range(L2)))
        if best is None or best[0] < s:
            best = (s, o, 0)
    return best


def brute_force_profile(table: np.ndarray, s1: np.ndarray, s2: np.ndarray, semantics=Semantics.REFERENCE):
    """Per-offset score profile by literal letter-by-letter replay: a list of (score, k), one per candidate
    offset — L1-L2 offsets under reference semantics, one more (k = 0 only) under spec, the single (0, 0)
    candidate when L2 == L1, none when L2 > L1 or L2 == 0. Each offset's best candidate, ties to the smallest
    k with k = 0 (no hyphen) first. O(L1*L2^2); the anchor oracle of the native profile code."""
    L1, L2 = len(s1), len(s2)
    if L2 > L1 or L2 <= 0:
        return []
    if L2 == L1:
        return [(int(sum(int(table[s2[i], s1[i]]) for i in range(L2))), 0)]
    prof = []
    for o in range(L1 - L2):
        best = None
        for m in range(L2):
            s = 0
            for i in range(L2):
                j = i + o if (i < m or m == 0) else i + o + 1
                s += int(table[s2[i], s1[j]])
            if best is None or best[0] < s:
                best = (s, m)
        prof.append(best)
    if Semantics.parse(semantics) == Semantics.SPEC:
        o = L1 - L2
        prof.append((int(sum(int(table[s2[i], s1[i + o]]) for i in range(L2))), 0))
    return prof


def brute_force_peaks(table: np.ndarray, s1: np.ndarray, s2: np.ndarray, radius: int, semantics=Semantics.REFERENCE,
                      profile=None):
    """The peaks of radius ``radius`` of :func:`brute_force_profile` (or of ``profile``, a list of (score, k), when
    given): a list of rows (score, n, k) in ascending n. Entry o is a peak iff no entry o' with 0 < |o - o'| <=
    radius and 0 <= o' < C is better than it — a higher score, or an equal score and a smaller offset. Written from
    that sentence with a plain double loop, O(C * radius): the anchor oracle of the native peak filters."""
    prof = brute_force_profile(table, s1, s2, semantics) if profile is None else list(profile)
    C = len(prof)
    rows = []
    for o in range(C):
        peak = True
        for o2 in range(max(0, o - radius), min(C - 1, o + radius) + 1):
            if o2 == o:
                continue
            if prof[o2][0] > prof[o][0] or (prof[o2][0] == prof[o][0] and o2 < o):
                peak = False
                break
        if peak:
            rows.append((int(prof[o][0]), o, int(prof[o][1])))
    return rows


def prefix_oracle(table: np.ndarray, s1: np.ndarray, s2: np.ndarray, semantics=Semantics.REFERENCE):
    L1, L2 = len(s1), len(s2)
    if L2 > L1:
        return (INT_MIN, 0, 0)
    s1 = np.asarray(s1, dtype=np.int64)
    s2 = np.asarray(s2, dtype=np.int64)
    if L2 == L1:
        return (int(table[s2, s1].sum()), 0, 0)
    nd = L1 - L2 + 1  # diagonals 0..L1-L2
    idx = np.arange(L2)[None, :] + np.arange(nd)[:, None]  # [nd, L2]
    cell = table[s2[None, :], s1[idx]].astype(np.int64)
    P = np.concatenate([np.zeros((nd, 1), np.int64), np.cumsum(cell, axis=1)], axis=1)  # P[d, k]
    tot = P[:, L2]
    n_off = L1 - L2
    # candidates per offset o < n_off: k = 0 -> tot[o]; k >= 1 -> P[o,k] - P[o+1,k] + tot[o+1]
    scores = np.empty((n_off, L2), np.int64)
    scores[:, 0] = tot[:n_off]
    if L2 > 1:
        scores[:, 1:] = P[:n_off, 1:L2] - P[1:n_off + 1, 1:L2] + tot[1:n_off + 1, None]
    flat = scores.reshape(-1)
    best_i = int(np.argmax(flat))  # first maximum = reference order
    best = (int(flat[best_i]), best_i // L2, best_i % L2)
    if Semantics.parse(semantics) == Semantics.SPEC and int(tot[n_off]) > best[0]:
        best = (int(tot[n_off]), n_off, 0)
    return best


def solve_problem(problem, semantics=Semantics.REFERENCE, oracle=prefix_oracle):
    """Runs an oracle over every record of a Problem; returns an (n, 3) int64 array."""
    t = score_table(problem.weights)
    out = np.zeros((problem.n, 3), np.int64)
    for i in range(problem.n):
        s2 = problem.codes[problem.offsets[i]:problem.offsets[i + 1]]
        out[i] = oracle(t, problem.seq1, s2, semantics)
    return out
