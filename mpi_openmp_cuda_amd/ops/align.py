"""Search ops: CPU (OpenMP) and GPU (gfx950 HIP kernels) engines behind one API.

Reference: send_divided_Seq2_To_Cuda + calc_result (cudaFunctions.cu:178-242, 63-176) — one kernel
launch and device sync per record. Here a whole batch is one pipeline call (HipSearchEngine.solve) or,
for device-resident data, one launch sequence on the caller's stream (HipSearchEngine.solve_device /
align_search_device, which take torch tensors on ``cuda:N``).
"""
from __future__ import annotations

import ctypes
import json
from typing import Optional

import numpy as np

from .. import _lib
from ..models.problem import Problem
from ..models.scoring import Semantics, Weights

RESULT_DTYPE = _lib.RESULT_DTYPE
PROFILE_DTYPE = _lib.PROFILE_DTYPE


def empty_results(n: int) -> np.ndarray:
    return np.zeros(n, dtype=RESULT_DTYPE)


def as_triples(results: np.ndarray, r2=None) -> np.ndarray:
    """Results in any wire format (R12/R8/R4 structured, R2 codes with their (smin, kw, j) parameters, or
    (n,3) ints) -> (n, 3) int32 [score, n, k]."""
    r = np.asarray(results)
    if r.dtype == _lib.R2_DTYPE:
        if r2 is None:
            raise ValueError("R2 results need their (smin, kw, j) parameters")
        smin, kw, j = (int(v) for v in r2)
        c = r.astype(np.int64)
        idx = c % j
        out = np.stack([c // j + smin, idx // kw, idx % kw], axis=1).astype(np.int32)
        out[c == 0xFFFF] = (np.iinfo(np.int32).min, 0, 0)
        return out
    if r.dtype == RESULT_DTYPE:
        return r.view(np.int32).reshape(-1, 3)
    if r.dtype.names:
        score = r["score"].astype(np.int32)
        if r.dtype == _lib.R4_DTYPE:
            score[r["score"] == np.iinfo(np.int16).min] = np.iinfo(np.int32).min
        return np.stack([score, r["n"].astype(np.int32), r["k"].astype(np.int32)], axis=1)
    return np.asarray(r, dtype=np.int32).reshape(-1, 3)


# ---------------------------------------------------------------------------------------------- CPU
def search_cpu(problem: Problem, semantics=Semantics.REFERENCE, threads: int = 0) -> np.ndarray:
    """O(L1*L2) OpenMP engine (csrc/src/cpu_engine.cpp). Returns structured results (score, n, k)."""
    out = empty_results(problem.n)
    _lib.check(_lib.lib().moc_cpu_solve(
        _lib.weights_arg(problem.weights.as_list()), _lib.ptr(problem.seq1), problem.L1,
        _lib.ptr(problem.codes), _lib.ptr(problem.offsets), problem.n, int(Semantics.parse(semantics)),
        int(threads), _lib.ptr(out)))
    return out


def search_keys_cpu(problem: Problem, part: int, parts: int, semantics=Semantics.REFERENCE,
                    threads: int = 0) -> np.ndarray:
    """Context-parallel partial search: part ``part`` of ``parts`` of every record's offset
    range -> packed uint64 pass-1 keys (0 = no candidate in this part). ``np.maximum`` over all parts, then
    :func:`decode_keys`, equals :func:`search_cpu`."""
    keys = np.zeros(problem.n, np.uint64)
    _lib.check(_lib.lib().moc_cpu_solve_keys(
        _lib.weights_arg(problem.weights.as_list()), _lib.ptr(problem.seq1), problem.L1,
        _lib.ptr(problem.codes), _lib.ptr(problem.offsets), problem.n, int(Semantics.parse(semantics)),
        int(part), int(parts), int(threads), _lib.ptr(keys)))
    return keys


def decode_keys(keys: np.ndarray, problem: Problem) -> np.ndarray:
    """MAX-combined pass-1 keys ((score^2^31)<<32 | ~(2n + mutated)) -> structured (score, n, k) results; the k
    of a mutated winner is the smallest one on its diagonal with that score, so the problem's records are
    needed (no n*L2 + k index: any L1 * L2)."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    out = empty_results(keys.shape[0])
    _lib.check(_lib.lib().moc_resolve_keys(
        _lib.weights_arg(problem.weights.as_list()), _lib.ptr(problem.seq1), problem.L1, _lib.ptr(problem.codes),
        _lib.ptr(problem.offsets), keys.shape[0], _lib.ptr(keys), _lib.ptr(out)))
    return out


def keys_to_ordered_int64(keys: np.ndarray) -> np.ndarray:
    """uint64 keys -> int64 with the same order (flip the top bit), for signed MAX all-reduces."""
    return (np.ascontiguousarray(keys, dtype=np.uint64) ^ np.uint64(1 << 63)).view(np.int64)


def ordered_int64_to_keys(v: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(v, dtype=np.int64).view(np.uint64) ^ np.uint64(1 << 63)


MAX_TOP_K = 64


def _check_k(K) -> int:
    K = int(K)
    if not 1 <= K <= MAX_TOP_K:
        raise ValueError(f"top-K: K must be in 1..{MAX_TOP_K}, got {K}")
    return K


MAX_PEAK_RADIUS = 2048  # csrc/include/moc/kernel_bounds.hpp kPeaksMaxRadius (tests compare it with the native value)


def _check_radius(radius) -> int:
    """The radius of the distinct forms of top-K and hits: 0 (the plain results) .. MAX_PEAK_RADIUS. Entry o of a
    record's profile is a peak of radius R iff no entry o' with 0 < |o - o'| <= R inside the profile has a higher
    score, or an equal score and a smaller offset; the distinct forms keep the peaks only."""
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)):
        raise ValueError(f"distinct: radius must be an integer in 0..{MAX_PEAK_RADIUS}, got {radius!r}")
    if not 0 <= int(radius) <= MAX_PEAK_RADIUS:
        raise ValueError(f"distinct: radius must be in 0..{MAX_PEAK_RADIUS}, got {int(radius)}")
    return int(radius)


def peaks_geometry() -> tuple:
    """(largest radius, most profile entries of a record that the GPU's wave-per-record peak kernel takes, entries
    per tile of its tile kernel) — csrc/include/moc/kernel_bounds.hpp; no GPU needed."""
    g = np.zeros(3, np.int32)
    _lib.check(_lib.lib().moc_peaks_geometry(_lib.ptr(g)))
    return int(g[0]), int(g[1]), int(g[2])


def profile_offsets(L1: int, lengths, semantics=Semantics.REFERENCE) -> np.ndarray:
    """int64 [n + 1] index of a batch's flat per-offset profile: record i owns entries
    [poffsets[i], poffsets[i + 1]), one per candidate offset — 0 if L2 > L1 or L2 <= 0, 1 if L2 == L1,
    L1 - L2 under reference semantics and L1 - L2 + 1 under spec."""
    L2 = np.asarray(lengths, dtype=np.int64).reshape(-1)
    spec = 1 if Semantics.parse(semantics) == Semantics.SPEC else 0
    c = np.where((L2 > L1) | (L2 <= 0), 0, np.where(L2 == L1, 1, L1 - L2 + spec))
    out = np.zeros(L2.shape[0] + 1, np.int64)
    np.cumsum(c, out=out[1:])
    return out


def search_profile_cpu(problem: Problem, semantics=Semantics.REFERENCE, threads: int = 0):
    """Per-offset score profile on the CPU engine: ``(prof, poffsets)`` — ``prof`` a flat PROFILE_DTYPE array
    (score, k), entry ``poffsets[i] + o`` = the best candidate of record i at offset o (ties: k = 0, then the
    smallest k). The maximum over a record's entries (higher score, then smaller offset) is search_cpu's row."""
    sem = Semantics.parse(semantics)
    poffsets = profile_offsets(problem.L1, problem.lengths, sem)
    prof = np.zeros(int(poffsets[-1]), dtype=PROFILE_DTYPE)
    _lib.check(_lib.lib().moc_cpu_profile(
        _lib.weights_arg(problem.weights.as_list()), _lib.ptr(problem.seq1), problem.L1, _lib.ptr(problem.codes),
        _lib.ptr(problem.offsets), problem.n, int(sem), int(threads), _lib.ptr(poffsets), _lib.ptr(prof)))
    return prof, poffsets


def search_topk_cpu(problem: Problem, K: int, semantics=Semantics.REFERENCE, threads: int = 0,
                    radius: int = 0) -> np.ndarray:
    """The K best offsets of every record on the CPU engine: int32 [n, K, 3] rows (score, n, k) in the order
    higher score, then smaller n, each with that offset's profile k; records with fewer than K candidate
    offsets are padded with (INT32_MIN, 0, 0). Row 0 is search_cpu's result. ``radius`` > 0: distinct placements —
    only the peaks of that radius (:func:`_check_radius`) are ranked, min(K, #peaks) rows and then padding; row 0
    is unchanged, the best offset always being a peak."""
    K = _check_k(K)
    radius = _check_radius(radius)
    out = np.zeros((problem.n, K, 3), np.int32)
    head = (_lib.weights_arg(problem.weights.as_list()), _lib.ptr(problem.seq1), problem.L1, _lib.ptr(problem.codes),
            _lib.ptr(problem.offsets), problem.n, int(Semantics.parse(semantics)), int(threads), K)
    if radius:
        _lib.check(_lib.lib().moc_cpu_topk_distinct(*head, radius, _lib.ptr(out)))
    else:
        _lib.check(_lib.lib().moc_cpu_topk(*head, _lib.ptr(out)))
    return out


# ---- threshold hits: every offset that scores at least a threshold (csrc/include/moc/cpu_engine.hpp)
_I32 = np.iinfo(np.int32)


def hits_geometry() -> tuple:
    """(records per scan block, block sums per pass of the single scanning block) of the GPU's prefix sum over hit
    counts (csrc/include/moc/kernel_bounds.hpp); no GPU needed."""
    g = np.zeros(2, np.int32)
    _lib.check(_lib.lib().moc_hits_geometry(_lib.ptr(g)))
    return int(g[0]), int(g[1])


def within_thresholds(best_scores, within) -> np.ndarray:
    """int32 thresholds "within D of the record's best": best − D, subtracted in int64 and clipped to int32."""
    d = int(within)
    if d < 0:
        raise ValueError(f"hits: within must be >= 0, got {d}")
    t = np.asarray(best_scores).astype(np.int64).reshape(-1) - d
    return np.clip(t, _I32.min, _I32.max).astype(np.int32)


def _hits_thresholds(n: int, min_score, thresholds, within, best_scores):
    """Checks that exactly one of the three is given -> (scalar int, int32 [n] array or None). ``best_scores``:
    a call returning the records' best scores (``within`` only)."""
    given = [x is not None for x in (min_score, thresholds, within)]
    if sum(given) != 1:
        raise ValueError("hits: give exactly one of min_score, thresholds, within")
    if min_score is not None:
        m = int(min_score)
        if not _I32.min <= m <= _I32.max:
            raise ValueError(f"hits: min_score {m} is not an int32")
        return m, None
    if thresholds is not None:
        t = np.asarray(thresholds)
        if t.ndim != 1 or t.shape[0] != n or not np.issubdtype(t.dtype, np.integer):
            raise ValueError(f"hits: thresholds must be {n} integers (one per record), got shape {t.shape}")
        if t.size and (t.min() < _I32.min or t.max() > _I32.max):
            raise ValueError("hits: thresholds must fit int32")
        return 0, np.ascontiguousarray(t, dtype=np.int32)
    if int(within) < 0:
        raise ValueError(f"hits: within must be >= 0, got {int(within)}")
    return 0, within_thresholds(best_scores(), within)


def search_hits_cpu(problem: Problem, min_score=None, thresholds=None, within=None, semantics=Semantics.REFERENCE,
                    threads: int = 0, radius: int = 0):
    """Threshold hits on the CPU engine: ``(rows, hoffsets)``. Record i's hits are the offsets o whose profile score
    (:func:`search_profile_cpu`) is >= its threshold (inclusive), ascending in o, as int32 rows (score, n = o, k of
    that profile entry) at ``rows[hoffsets[i]:hoffsets[i + 1]]``; ``hoffsets`` is int64 [n + 1] and
    ``hoffsets[-1]`` the total H. Exactly one of ``min_score`` (one int32 for the batch; INT32_MIN selects the whole
    profile), ``thresholds`` (int32 [n]) and ``within`` (D >= 0: every offset within D of the record's best score,
    from a search on the same engine) must be given. ``radius`` > 0: distinct placements — only the hits that are
    peaks of that radius (:func:`_check_radius`); a threshold does not interact with the suppression, whatever
    suppresses an entry scores at least as much."""
    sem = Semantics.parse(semantics)
    radius = _check_radius(radius)
    m, t = _hits_thresholds(problem.n, min_score, thresholds, within,
                            lambda: search_cpu(problem, sem, threads)["score"])
    hoffsets = np.zeros(problem.n + 1, np.int64)

    def call(rows, cap):
        head = (_lib.weights_arg(problem.weights.as_list()), _lib.ptr(problem.seq1), problem.L1,
                _lib.ptr(problem.codes), _lib.ptr(problem.offsets), problem.n, int(sem), int(threads), m, _lib.ptr(t))
        if radius:
            _lib.check(_lib.lib().moc_cpu_hits_distinct(*head, radius, _lib.ptr(hoffsets), _lib.ptr(rows), cap))
        else:
            _lib.check(_lib.lib().moc_cpu_hits(*head, _lib.ptr(hoffsets), _lib.ptr(rows), cap))

    call(None, 0)  # counts
    total = int(hoffsets[-1])
    rows = np.zeros((total, 3), np.int32)
    if total:
        call(rows, total)
    return rows, hoffsets


# ---- profile summary: per-record moments, extremes and histogram of the profile (csrc/include/moc/cpu_engine.hpp)
SUMMARY_COLS = ("count", "sum", "sumsq", "min", "max", "n", "k")
SUMMARY_MAX_BINS = 256  # csrc/include/moc/kernel_bounds.hpp kSummaryMaxBins (tests compare it with the native value)
_COUNT, _SUM, _SUMSQ, _MIN, _MAX = 0, 1, 2, 3, 4


def summary_geometry() -> tuple:
    """(records per workgroup of the GPU's summary kernels — one wave each —, threads per workgroup, largest
    ``bins``) — csrc/include/moc/kernel_bounds.hpp; no GPU needed."""
    g = np.zeros(3, np.int32)
    _lib.check(_lib.lib().moc_summary_geometry(_lib.ptr(g)))
    return int(g[0]), int(g[1]), int(g[2])


def summary_bound(max_abs_weight: int, max_l2: int) -> int:
    """The exactness bound of a summary: the most candidate offsets C a record may have so that the int64 sum of
    squares cannot overflow, floor((2^63 - 1) / M^2) with M = min(2^31, max |W| * the call's longest record). A call
    with a longer profile is refused before anything runs. No GPU needed."""
    return int(_lib.lib().moc_summary_bound(int(max_abs_weight), int(max_l2)))


def _summary_args(bins, lo, width) -> tuple:
    bins, lo, width = int(bins), int(lo), int(width)
    if not 0 <= bins <= SUMMARY_MAX_BINS:
        raise ValueError(f"summary: bins must be in 0..{SUMMARY_MAX_BINS}, got {bins}")
    if not 1 <= width <= _I32.max:
        raise ValueError(f"summary: width must be an int32 of at least 1, got {width}")
    if not _I32.min <= lo <= _I32.max:
        raise ValueError(f"summary: lo {lo} is not an int32")
    return bins, lo, width


def _summary_check(rc):
    """A native summary call's status: its argument and exactness-bound errors (messages that start with
    "summary:") are ValueErrors, anything else a NativeError."""
    if rc != 0:
        msg = _lib.lib().moc_last_error().decode(errors="replace")
        if msg.startswith("summary:"):
            raise ValueError(msg)
        raise _lib.NativeError(msg)


def search_summary_cpu(problem: Problem, bins: int = 0, lo: int = 0, width: int = 1, semantics=Semantics.REFERENCE,
                       threads: int = 0):
    """Profile summary on the CPU engine: ``(summary, hist)``. ``summary`` is int64 [n, 7] with the columns
    :data:`SUMMARY_COLS` — ``count`` the record's candidate offsets C, ``sum`` and ``sumsq`` of its profile scores
    (:func:`search_profile_cpu`; exact), ``min`` and ``max`` over them, and ``(max, n, k)`` search_cpu's row; a
    record without candidate offsets gives (0, 0, 0, INT32_MAX, INT32_MIN, 0, 0). ``hist`` is None with
    ``bins = 0``, else int32 [n, bins]: a score s counts in bin clamp(floor((s - lo) / width), 0, bins - 1), so scores
    below ``lo`` land in bin 0 and scores at or past ``lo + bins * width`` in the last; every row sums to ``count``.
    ``bins`` in 0..256, ``width`` >= 1; raises ValueError for those and when the exactness bound
    (:func:`summary_bound`) does not hold for the call."""
    bins, lo, width = _summary_args(bins, lo, width)
    sem = Semantics.parse(semantics)
    summary = np.zeros((problem.n, len(SUMMARY_COLS)), np.int64)
    hist = np.zeros((problem.n, bins), np.int32) if bins else None
    _summary_check(_lib.lib().moc_cpu_summary(
        _lib.weights_arg(problem.weights.as_list()), _lib.ptr(problem.seq1), problem.L1, _lib.ptr(problem.codes),
        _lib.ptr(problem.offsets), problem.n, int(sem), int(threads), bins, lo, width, _lib.ptr(summary),
        _lib.ptr(hist)))
    return summary, hist


def summary_zscore(summary) -> np.ndarray:
    """float64 [n]: how far each record's best score lies above its OTHER C - 1 profile entries, in their population
    standard deviations — with mean' = (sum - max) / (C - 1) and var' = (sumsq - max^2) / (C - 1) - mean'^2,
    z = (max - mean') / sqrt(var'). NaN when C < 3 or var' <= 0 (an all-equal rest). Reads nothing but the summary.
    Both numerators, (C - 1) max - (sum - max) and (C - 1)(sumsq - max^2) - (sum - max)^2, are formed in exact
    Python integers; only the square root and the final division are float64."""
    import math

    s = np.asarray(summary, dtype=np.int64).reshape(-1, len(SUMMARY_COLS))
    out = np.full(s.shape[0], np.nan, np.float64)
    for i, row in enumerate(s.tolist()):
        c, tot, sq, mx = row[_COUNT], row[_SUM], row[_SUMSQ], row[_MAX]
        if c < 3:
            continue
        rest = tot - mx
        num = (c - 1) * (sq - mx * mx) - rest * rest  # (C - 1)^2 var'
        if num > 0:
            out[i] = ((c - 1) * mx - rest) / math.sqrt(num)
    return out


def summary_thresholds(summary, z):
    """int32 [n] thresholds "z standard deviations above the rest": ceil(mean' + z * sd') with mean' and sd' of
    :func:`summary_zscore`, clipped to int32, and INT32_MAX (no hit) where that z-score is NaN (C < 3 or
    var' <= 0) — ready as ``thresholds`` of the hits calls. ``summary``: a numpy array, or a torch tensor — then the
    result is a tensor on its device, computed there with float64 ops and no synchronisation, so summary ->
    thresholds -> ``solve_hits_device`` runs on one stream. Both paths run the same float64 operations: sum - max
    and sumsq - max^2 are exact int64, the rest rounds (var' = E'[s^2] - mean'^2 loses about mean'^2 / var' ulps)."""
    z = float(z)
    if isinstance(summary, np.ndarray) or not hasattr(summary, "device"):
        s = np.asarray(summary, dtype=np.int64).reshape(-1, len(SUMMARY_COLS))
        c, mx = s[:, _COUNT], s[:, _MAX]
        c1 = np.maximum(c - 1, 1).astype(np.float64)
        mean = (s[:, _SUM] - mx).astype(np.float64) / c1
        var = (s[:, _SUMSQ] - mx * mx).astype(np.float64) / c1 - mean * mean
        ok = (c >= 3) & (var > 0)
        sd = np.sqrt(np.where(ok, var, 0.0))
        t = np.ceil(mean + z * sd)
        t = np.where(ok, np.clip(t, float(_I32.min), float(_I32.max)), float(_I32.max))
        return t.astype(np.int64).astype(np.int32)
    import torch

    s = summary.reshape(-1, len(SUMMARY_COLS))
    assert s.dtype == torch.int64
    c, mx = s[:, _COUNT], s[:, _MAX]
    c1 = torch.clamp(c - 1, min=1).to(torch.float64)
    mean = (s[:, _SUM] - mx).to(torch.float64) / c1
    var = (s[:, _SUMSQ] - mx * mx).to(torch.float64) / c1 - mean * mean
    ok = (c >= 3) & (var > 0)
    sd = torch.sqrt(torch.where(ok, var, torch.zeros_like(var)))
    t = torch.ceil(mean + z * sd)
    t = torch.where(ok, torch.clamp(t, float(_I32.min), float(_I32.max)), torch.full_like(t, float(_I32.max)))
    return t.to(torch.int64).to(torch.int32).contiguous()


# ---- multi-target search: every record's best alignment against each of T targets (csrc/include/moc/cpu_engine.hpp)
TARGETS_MAX = 4096  # csrc/include/moc/kernel_bounds.hpp kTargetsMax (tests compare it with the native value)


def targets_geometry() -> tuple:
    """(largest T, threads per workgroup of the GPU's targets kernel, longest slice a 4-lane group takes, longest
    slice a 16-lane group takes) — csrc/include/moc/kernel_bounds.hpp; no GPU needed."""
    g = np.zeros(4, np.int32)
    _lib.check(_lib.lib().moc_targets_geometry(_lib.ptr(g)))
    return tuple(int(x) for x in g)


def _targets_check(rc):
    """A native targets call's status: its target-set errors (messages that start with "targets:") are
    ValueErrors, anything else a NativeError."""
    if rc != 0:
        msg = _lib.lib().moc_last_error().decode(errors="replace")
        if msg.startswith("targets:"):
            raise ValueError(msg)
        raise _lib.NativeError(msg)


def check_targets(starts, L1: int) -> np.ndarray:
    """``starts`` as a contiguous int64 [T + 1] array, checked: 1 <= T <= 4096 and strictly rising from 0 to ``L1``
    (every target holds at least one letter), else a ValueError whose message starts with ``targets:``."""
    s = np.ascontiguousarray(starts, dtype=np.int64).reshape(-1)
    _targets_check(_lib.lib().moc_check_targets(_lib.ptr(s) if s.size else None, int(s.size) - 1, int(L1)))
    return s


class TargetSet:
    """T target sequences stored as their plain concatenation, the catalog (``seq1``: uint8 codes, no separator
    letters), with ``starts`` (int64 [T + 1]): target t is ``seq1[starts[t]:starts[t + 1]]``. The catalog is the
    engines' Seq1: ``Problem(weights, ts.seq1, codes, offsets)`` / ``set_problem(weights, ts.seq1)``."""

    def __init__(self, seq1, starts):
        self.seq1 = np.ascontiguousarray(seq1, dtype=np.uint8)
        self.starts = check_targets(starts, self.seq1.shape[0])

    @classmethod
    def from_sequences(cls, seqs) -> "TargetSet":
        """From T arrays of letter codes (each at least one letter)."""
        seqs = [np.ascontiguousarray(s, dtype=np.uint8).reshape(-1) for s in seqs]
        starts = np.zeros(len(seqs) + 1, np.int64)
        if seqs:
            np.cumsum([s.shape[0] for s in seqs], out=starts[1:])
        return cls(np.concatenate(seqs) if seqs else np.zeros(0, np.uint8), starts)

    @classmethod
    def from_strings(cls, strings) -> "TargetSet":
        """From T strings of letters A-Z (case-insensitive, as Seq1)."""
        from ..models.scoring import encode

        return cls.from_sequences([encode(s) for s in strings])

    @property
    def T(self) -> int:
        return int(self.starts.shape[0] - 1)

    @property
    def lengths(self) -> np.ndarray:
        return np.diff(self.starts)

    def target(self, t: int) -> np.ndarray:
        return self.seq1[self.starts[t]:self.starts[t + 1]]


def _starts_of(targets, L1: int) -> np.ndarray:
    """``targets`` (a :class:`TargetSet` or a starts array) -> checked int64 starts over a catalog of L1 letters."""
    starts = targets.starts if isinstance(targets, TargetSet) else targets
    if L1 is None:  # an engine without a problem: the native call says so
        L1 = int(np.asarray(starts).reshape(-1)[-1]) if np.size(starts) else 0
    return check_targets(starts, L1)


def search_targets_cpu(problem: Problem, targets, semantics=Semantics.REFERENCE, threads: int = 0) -> np.ndarray:
    """Multi-target search on the CPU engine. ``problem.seq1`` is the catalog and ``targets`` its
    :class:`TargetSet` (or just the starts). Returns int32 [n, T, 3]: row [i, t] = (score, n, k) is exactly
    search_cpu's row for record i against target t alone, n relative to the target's start; (INT32_MIN, 0, 0) where
    the record is longer than the target. No placement straddles two targets: a target's rows come from the
    catalog profile's entries that read inside it, plus its own un-mutated final diagonal summed from the letters.
    With T = 1 the [n, 1, 3] result equals search_cpu row for row. ValueError for an invalid target set."""
    starts = _starts_of(targets, problem.L1)
    T = starts.shape[0] - 1
    out = np.zeros((problem.n, T, 3), np.int32)
    _targets_check(_lib.lib().moc_cpu_targets(
        _lib.weights_arg(problem.weights.as_list()), _lib.ptr(problem.seq1), problem.L1, _lib.ptr(problem.codes),
        _lib.ptr(problem.offsets), problem.n, _lib.ptr(starts), T, int(Semantics.parse(semantics)), int(threads),
        _lib.ptr(out)))
    return out


def _targets_best_z(rows, z):
    """targets_best's ranking by z-score; see there."""
    if isinstance(rows, np.ndarray) or not hasattr(rows, "device"):
        r = np.asarray(rows, dtype=np.int32)
        zz = np.asarray(z, dtype=np.float64)
        if r.ndim != 3 or r.shape[2] != 3 or r.shape[1] < 1:
            raise ValueError(f"targets_best needs [n, T, 3] rows, got {r.shape}")
        if zz.shape != r.shape[:2]:
            raise ValueError(f"targets_best needs z of the rows' shape [n, T] = {r.shape[:2]}, got {zz.shape}")
        score = r[:, :, 0].astype(np.int64)
        fit = score != _I32.min
        zk = np.where(fit & ~np.isnan(zz), zz, -np.inf)  # a NaN ranks below every defined z
        cand = fit & (zk == zk.max(axis=1, keepdims=True))
        sk = np.where(cand, score, np.iinfo(np.int64).min)
        cand &= sk == sk.max(axis=1, keepdims=True)  # ties: the higher score
        t = np.argmax(cand, axis=1)                  # then the smallest target index
        none = ~fit.any(axis=1)
        row = np.ascontiguousarray(r[np.arange(r.shape[0]), t])
        row[none] = (_I32.min, 0, 0)
        return np.where(none, -1, t).astype(np.int32), row
    import torch

    assert rows.dtype == torch.int32 and rows.dim() == 3 and rows.shape[2] == 3 and rows.shape[1] >= 1
    assert z.dtype == torch.float64 and tuple(z.shape) == tuple(rows.shape[:2]) and z.device == rows.device
    T = rows.shape[1]
    score = rows[:, :, 0].to(torch.int64)
    fit = score != _I32.min
    zk = torch.where(fit & ~torch.isnan(z), z, torch.full_like(z, float("-inf")))
    cand = fit & (zk == zk.max(dim=1, keepdim=True).values)
    sk = torch.where(cand, score, torch.full_like(score, int(np.iinfo(np.int64).min)))
    cand = cand & (sk == sk.max(dim=1, keepdim=True).values)
    idx = torch.arange(T, device=rows.device).expand_as(score)
    t = torch.where(cand, idx, torch.full_like(idx, T)).min(dim=1).values
    none = ~fit.any(dim=1)
    t = torch.where(none, torch.zeros_like(t), t)
    row = rows.gather(1, t.view(-1, 1, 1).expand(-1, 1, 3)).squeeze(1)
    empty = torch.tensor([_I32.min, 0, 0], dtype=torch.int32, device=rows.device)
    row = torch.where(none.unsqueeze(1), empty.expand_as(row), row).contiguous()
    return torch.where(none, torch.full_like(t, -1), t).to(torch.int32), row


def targets_best(rows, z=None):
    """The best target per record of multi-target rows [n, T, 3]: ``(target int32 [n], row int32 [n, 3])`` — the
    highest score, then the smallest target index; -1 and (INT32_MIN, 0, 0) where no target fits the record.
    ``rows``: a numpy array, or a torch tensor — then both results are tensors on its device, computed there
    without a synchronisation.
    With ``z`` (float64 [n, T] from :func:`targets_zscore`, numpy or torch like ``rows``) the ranking is by z-score
    among the targets that fit: the highest z wins, a NaN ranks below every defined z, ties go to the higher score
    and then to the smaller target index; -1 and the empty row only where no target fits."""
    if z is not None:
        return _targets_best_z(rows, z)
    if isinstance(rows, np.ndarray) or not hasattr(rows, "device"):
        r = np.asarray(rows, dtype=np.int32)
        if r.ndim != 3 or r.shape[2] != 3 or r.shape[1] < 1:
            raise ValueError(f"targets_best needs [n, T, 3] rows, got {r.shape}")
        t = np.argmax(r[:, :, 0], axis=1)  # the first maximum: the smallest target index
        row = np.ascontiguousarray(r[np.arange(r.shape[0]), t])
        none = row[:, 0] == _I32.min
        row[none] = (_I32.min, 0, 0)
        return np.where(none, -1, t).astype(np.int32), row
    import torch

    assert rows.dtype == torch.int32 and rows.dim() == 3 and rows.shape[2] == 3 and rows.shape[1] >= 1
    score = rows[:, :, 0]
    mx = score.max(dim=1, keepdim=True).values
    idx = torch.arange(rows.shape[1], device=rows.device).expand_as(score)
    t = torch.where(score == mx, idx, torch.full_like(idx, rows.shape[1])).min(dim=1).values  # first maximum
    row = rows.gather(1, t.view(-1, 1, 1).expand(-1, 1, 3)).squeeze(1)
    none = mx.squeeze(1) == _I32.min
    empty = torch.tensor([_I32.min, 0, 0], dtype=torch.int32, device=rows.device)
    row = torch.where(none.unsqueeze(1), empty.expand_as(row), row).contiguous()
    return torch.where(none, torch.full_like(t, -1), t).to(torch.int32), row


def targets_catalog_rows(rows, targets):
    """Multi-target rows [n, T, 3], or per-target top-K rows [n, T, K, 3], with their offsets moved from the targets
    to the catalog: n + starts[t]; empty rows (score INT32_MIN) stay untouched. The result has the shape of ``rows``;
    a [n, T, 3] block — or a top-K one reshaped to [n, T * K, 3] — is what the report calls take as it is
    (``search_report_cpu`` / ``report`` / ``report_device`` work on the catalog; at most 64 rows per record there).
    ``rows``: a numpy array, or a torch tensor — then the result is a tensor on its device, computed there without
    a synchronisation (the starts go up with a non-blocking copy)."""
    starts = np.ascontiguousarray(targets.starts if isinstance(targets, TargetSet) else targets, dtype=np.int64)
    T = starts.shape[0] - 1
    if isinstance(rows, np.ndarray) or not hasattr(rows, "device"):
        r = np.array(rows, dtype=np.int32)
        if r.ndim not in (3, 4) or r.shape[-1] != 3 or r.shape[1] != T:
            raise ValueError(f"targets_catalog_rows needs [n, T, 3] or [n, T, K, 3] rows for the T = {T} targets")
        b = starts[:-1].reshape((1, T) + (1,) * (r.ndim - 3))  # one start per target, broadcast over K
        r[..., 1] = (r[..., 1] + np.where(r[..., 0] == _I32.min, 0, b)).astype(np.int32)
        return r
    import torch

    assert rows.dtype == torch.int32 and rows.dim() in (3, 4) and rows.shape[-1] == 3
    assert rows.shape[1] == T
    b = torch.from_numpy(starts[:-1].astype(np.int32)).to(rows.device, non_blocking=True)
    b = b.reshape((1, T) + (1,) * (rows.dim() - 3)).expand(rows.shape[:-1])
    out = rows.clone()
    out[..., 1] += torch.where(rows[..., 0] == _I32.min, torch.zeros_like(b), b)
    return out.contiguous()


# ---- target ranking: each record's M best targets, without the n x T pair rows
RANK_COLS = ("target", "score", "n", "k")


def _check_rank_m(M) -> int:
    M = int(M)
    if not 1 <= M <= MAX_TOP_K:
        raise ValueError(f"rank: M must be in 1..{MAX_TOP_K}, got {M}")
    return M


def _targets_rank_check(rc):
    """A native rank call's status: target-set errors ("targets:") and an M out of range ("rank:") are ValueErrors,
    anything else a NativeError."""
    if rc != 0:
        msg = _lib.lib().moc_last_error().decode(errors="replace")
        if msg.startswith(("targets:", "rank:")):
            raise ValueError(msg)
        raise _lib.NativeError(msg)


def targets_rank_geometry() -> tuple:
    """(bytes of profile scratch a chunk of the engine's rank call needs per (record, target) pair, the most targets a
    4-lane group of the rank kernel takes, the most a 16-lane group takes) — csrc/include/moc/kernel_bounds.hpp; no
    GPU needed."""
    g = np.zeros(3, np.int32)
    _lib.check(_lib.lib().moc_targets_rank_geometry(_lib.ptr(g)))
    return tuple(int(x) for x in g)


def search_targets_rank_cpu(problem: Problem, targets, M: int, semantics=Semantics.REFERENCE,
                            threads: int = 0) -> np.ndarray:
    """Target ranking on the CPU engine. ``problem.seq1`` is the catalog and ``targets`` its :class:`TargetSet` (or
    just the starts). Returns int32 [n, M, 4] with the columns :data:`RANK_COLS`: ``out[i, j]`` = (t, score, n, k) is
    record i's j-th best target among the F_i that fit it (record length <= target length) — higher score first, then
    smaller target index — with (score, n, k) exactly :func:`search_targets_cpu`'s row [i, t], n relative to the
    target's start; the rows past F_i are (-1, INT32_MIN, 0, 0). So ``out[:, 0]`` is :func:`targets_best`, the whole
    result is search_targets_cpu's rows stably sorted by (-score, t) with the pairs that do not fit dropped, and
    T = 1 is :func:`search_cpu` with a leading 0. The n x T pair rows never exist as a whole. ValueError for an
    invalid target set ("targets: ...", first), then for M outside 1..64 ("rank: ...")."""
    starts = _starts_of(targets, problem.L1)
    M = _check_rank_m(M)
    T = starts.shape[0] - 1
    out = np.zeros((problem.n, M, 4), np.int32)
    _targets_rank_check(_lib.lib().moc_cpu_targets_rank(
        _lib.weights_arg(problem.weights.as_list()), _lib.ptr(problem.seq1), problem.L1, _lib.ptr(problem.codes),
        _lib.ptr(problem.offsets), problem.n, _lib.ptr(starts), T, int(Semantics.parse(semantics)), int(threads), M,
        _lib.ptr(out)))
    return out


def targets_rank_catalog_rows(rank, targets):
    """Rank rows [n, M, 4] (columns :data:`RANK_COLS`) as int32 [n, M, 3] rows (score, n, k) on the catalog: n +
    starts[t]; padding rows (target -1) become (INT32_MIN, 0, 0). What the report calls take as it is
    (``search_report_cpu`` / ``report`` / ``report_device`` work on the catalog). ``rank``: a numpy array, or a torch
    tensor — then the result is a tensor on its device, computed there without a synchronisation (the starts go up
    with a non-blocking copy)."""
    starts = np.ascontiguousarray(targets.starts if isinstance(targets, TargetSet) else targets, dtype=np.int64)
    T = starts.shape[0] - 1
    if isinstance(rank, np.ndarray) or not hasattr(rank, "device"):
        r = np.asarray(rank, dtype=np.int32)
        if r.ndim != 3 or r.shape[2] != 4:
            raise ValueError(f"targets_rank_catalog_rows needs [n, M, 4] rank rows, got {r.shape}")
        t = r[:, :, 0].astype(np.int64)
        if t.size and (t.min() < -1 or t.max() >= T):
            raise ValueError(f"targets_rank_catalog_rows: a target index outside -1..{T - 1}")
        pad = t < 0
        out = np.ascontiguousarray(r[:, :, 1:])
        out[:, :, 1] = (out[:, :, 1] + starts[np.where(pad, 0, t)]).astype(np.int32)
        out[pad] = (_I32.min, 0, 0)
        return out
    import torch

    assert rank.dtype == torch.int32 and rank.dim() == 3 and rank.shape[2] == 4
    b = torch.from_numpy(starts[:-1].astype(np.int32)).to(rank.device, non_blocking=True)
    t = rank[:, :, 0].to(torch.int64)
    pad = t < 0
    score, n, k = rank[:, :, 1], rank[:, :, 2] + b[t.clamp(0, T - 1)], rank[:, :, 3]
    zero = torch.zeros_like(score)  # the padding row's values are filled on the device: no host tensor, no copy
    return torch.stack([torch.where(pad, torch.full_like(score, _I32.min), score), torch.where(pad, zero, n),
                        torch.where(pad, zero, k)], dim=2).contiguous()


def targets_rank_chunks(L1: int, offsets, T: int, scratch_bytes: int, semantics=Semantics.REFERENCE) -> np.ndarray:
    """The chunks :meth:`HipSearchEngine.solve_targets_rank` cuts a batch into after
    ``set_profile_scratch(scratch_bytes)`` against a catalog of ``L1`` letters and ``T`` targets
    (csrc/include/moc/tile_plan.hpp plan_profile), no GPU needed: int64 bounds ``0 = b0 < b1 < ... = n``. A chunk takes
    records while ``8 * entries + 12 * T * records <= scratch_bytes`` — its profile entries and its pair rows — and at
    least one record. ``T = 0`` has no per-record bytes: the cut of top-K and hits, records while their entries number
    at most ``max(1, scratch_bytes // 8)``. ``offsets`` as :meth:`HipSearchEngine.solve` takes them."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n = offsets.shape[0] - 1
    if n < 0:
        raise ValueError("offsets needs at least one entry")
    bounds = np.zeros(n + 1, np.int64)
    chunks = int(_lib.lib().moc_targets_rank_chunks(int(L1), _lib.ptr(offsets), n, int(T), int(scratch_bytes),
                                                    int(Semantics.parse(semantics)), _lib.ptr(bounds)))
    if chunks < 0:
        raise _lib.NativeError(_lib.lib().moc_last_error().decode(errors="replace"))
    return bounds[:chunks + 1].copy()


# ---- per-target profile summary: one summary row and histogram per (record, target) pair
def targets_summary_geometry() -> tuple:
    """(threads per workgroup of the GPU's per-target summary kernels, largest ``bins``, the most bins a 4-lane group
    takes in the histogram kernel — past it a 4-lane choice becomes 16 lanes —, the LDS bytes a workgroup's counters
    stay within) — csrc/include/moc/kernel_bounds.hpp; no GPU needed."""
    g = np.zeros(4, np.int32)
    _lib.check(_lib.lib().moc_targets_summary_geometry(_lib.ptr(g)))
    return tuple(int(x) for x in g)


def _targets_summary_check(rc):
    """A native per-target summary call's status: target-set errors ("targets:") and argument or exactness-bound
    errors ("summary:") are ValueErrors, anything else a NativeError."""
    if rc != 0:
        msg = _lib.lib().moc_last_error().decode(errors="replace")
        if msg.startswith("targets:") or msg.startswith("summary:"):
            raise ValueError(msg)
        raise _lib.NativeError(msg)


def search_targets_summary_cpu(problem: Problem, targets, bins: int = 0, lo: int = 0, width: int = 1,
                               semantics=Semantics.REFERENCE, threads: int = 0):
    """Per-target profile summary on the CPU engine: ``(summary, hist)``. ``problem.seq1`` is the catalog and
    ``targets`` its :class:`TargetSet` (or just the starts). ``summary`` is int64 [n, T, 7] with the columns
    :data:`SUMMARY_COLS`: row [i, t] is exactly :func:`search_summary_cpu`'s row of record i against target t alone
    — ``(max, n, k)`` is :func:`search_targets_cpu`'s row, n relative to the target's start — and
    (0, 0, 0, INT32_MAX, INT32_MIN, 0, 0) where the record is longer than the target. ``hist`` is None with
    ``bins = 0``, else int32 [n, T, bins] with search_summary_cpu's bin rule; every row sums to its pair's ``count``.
    No entry straddles two targets. ValueError for an invalid target set ("targets: ..."), for ``bins`` / ``width``
    out of range and when the exactness bound (:func:`summary_bound`) does not hold for the largest target profile
    of the call ("summary: ...") — the catalog's own profile may be past it."""
    bins, lo, width = _summary_args(bins, lo, width)
    starts = _starts_of(targets, problem.L1)
    T = starts.shape[0] - 1
    summary = np.zeros((problem.n, T, len(SUMMARY_COLS)), np.int64)
    hist = np.zeros((problem.n, T, bins), np.int32) if bins else None
    _targets_summary_check(_lib.lib().moc_cpu_targets_summary(
        _lib.weights_arg(problem.weights.as_list()), _lib.ptr(problem.seq1), problem.L1, _lib.ptr(problem.codes),
        _lib.ptr(problem.offsets), problem.n, _lib.ptr(starts), T, int(Semantics.parse(semantics)), int(threads), bins,
        lo, width, _lib.ptr(summary), _lib.ptr(hist)))
    return summary, hist


def targets_zscore(summary):
    """float64 [n, T]: :func:`summary_zscore` of every (record, target) pair of a per-target summary [n, T, 7] — how
    far the pair's best score lies above the other entries of its target profile; NaN where summary_zscore is (fewer
    than 3 entries, a pair that does not fit, or an all-equal rest). ``summary``: a numpy array — exact-integer
    numerators, as summary_zscore — or a torch tensor — then the result is a tensor on its device, computed there
    with float64 operations and no synchronisation, as :func:`summary_thresholds` does (sum - max and sumsq - max^2
    are exact int64, the rest rounds)."""
    if isinstance(summary, np.ndarray) or not hasattr(summary, "device"):
        s = np.asarray(summary, dtype=np.int64)
        if s.ndim != 3 or s.shape[2] != len(SUMMARY_COLS):
            raise ValueError(f"targets_zscore needs a [n, T, 7] summary, got {s.shape}")
        return summary_zscore(s).reshape(s.shape[0], s.shape[1])
    import torch

    assert summary.dtype == torch.int64 and summary.dim() == 3 and summary.shape[2] == len(SUMMARY_COLS)
    c, mx = summary[:, :, _COUNT], summary[:, :, _MAX]
    c1 = torch.clamp(c - 1, min=1).to(torch.float64)
    mean = (summary[:, :, _SUM] - mx).to(torch.float64) / c1
    var = (summary[:, :, _SUMSQ] - mx * mx).to(torch.float64) / c1 - mean * mean
    ok = (c >= 3) & (var > 0)
    sd = torch.sqrt(torch.where(ok, var, torch.ones_like(var)))
    return torch.where(ok, (mx.to(torch.float64) - mean) / sd, torch.full_like(mean, float("nan"))).contiguous()


# ---- per-target top-K and threshold hits: the rows of every (record, target) pair's target profile
def _targets_rows_check(rc):
    """A native per-target top-K / hits call's status: target-set errors ("targets:"), a K out of range ("top-K:")
    buffer errors ("hits:") and a radius out of range ("distinct:") are ValueErrors, anything else a NativeError."""
    if rc != 0:
        msg = _lib.lib().moc_last_error().decode(errors="replace")
        if msg.startswith(("targets:", "top-K:", "hits:", "distinct:")):
            raise ValueError(msg)
        raise _lib.NativeError(msg)


def _targets_hits_thresholds(n: int, T: int, min_score, thresholds, within, best_rows):
    """:func:`_hits_thresholds` over pairs: exactly one of the three -> (scalar int, int32 [n * T] pair-major array or
    None). ``thresholds``: [n, T], or [n] broadcast over the targets. ``best_rows``: a call returning the
    multi-target rows [n, T, 3] (``within`` only); a pair's threshold is its own best score minus D."""
    if sum(x is not None for x in (min_score, thresholds, within)) != 1:
        raise ValueError("hits: give exactly one of min_score, thresholds, within")
    if min_score is not None:
        m = int(min_score)
        if not _I32.min <= m <= _I32.max:
            raise ValueError(f"hits: min_score {m} is not an int32")
        return m, None
    if thresholds is not None:
        t = np.asarray(thresholds)
        if t.shape not in ((n, T), (n,)) or not np.issubdtype(t.dtype, np.integer):
            raise ValueError(f"hits: thresholds must be {n} x {T} integers (one per pair) or {n} (one per record), "
                             f"got shape {t.shape}")
        if t.size and (t.min() < _I32.min or t.max() > _I32.max):
            raise ValueError("hits: thresholds must fit int32")
        if t.ndim == 1:
            t = np.broadcast_to(t[:, None], (n, T))
        return 0, np.ascontiguousarray(t, dtype=np.int32).reshape(-1)
    if int(within) < 0:
        raise ValueError(f"hits: within must be >= 0, got {int(within)}")
    return 0, within_thresholds(np.asarray(best_rows())[:, :, 0], within)


def _targets_hits_args(n: int, T: int, min_score, thresholds, within, radius, best_rows):
    """:func:`_targets_hits_thresholds`, then :func:`_check_radius` — the order of the per-target hits errors — with
    the radius checked before ``best_rows`` runs anything: (scalar, thresholds or None, radius)."""
    def best():
        _check_radius(radius)
        return best_rows()

    m, t = _targets_hits_thresholds(n, T, min_score, thresholds, within, best)
    return m, t, _check_radius(radius)


def search_targets_topk_cpu(problem: Problem, targets, K: int, semantics=Semantics.REFERENCE,
                            threads: int = 0, radius: int = 0) -> np.ndarray:
    """Per-target top-K on the CPU engine. ``problem.seq1`` is the catalog and ``targets`` its :class:`TargetSet` (or
    just the starts). Returns int32 [n, T, K, 3]: ``out[i, t]`` is exactly :func:`search_topk_cpu`'s [K, 3] block of
    record i against target t alone — the pair's best placements in the order higher score, then smaller n, n
    relative to the target's start, padded with (INT32_MIN, 0, 0) — so no row straddles two targets. ``K = 1`` is
    :func:`search_targets_cpu`. ``radius`` > 0 keeps the distinct placements only: the peaks of radius ``radius`` of
    every pair's OWN profile (its windows clipped to the pair's entries, the boundary entry among them), so
    ``out[i, t]`` is :func:`search_topk_cpu` with that radius on target t alone; row 0 is the same at every radius.
    ValueError for an invalid target set ("targets: ...", first), for K outside 1..64, then for the radius
    ("distinct: ...")."""
    starts = _starts_of(targets, problem.L1)
    K = _check_k(K)
    radius = _check_radius(radius)
    T = starts.shape[0] - 1
    out = np.zeros((problem.n, T, K, 3), np.int32)
    _targets_rows_check(_lib.lib().moc_cpu_targets_topk_distinct(
        _lib.weights_arg(problem.weights.as_list()), _lib.ptr(problem.seq1), problem.L1, _lib.ptr(problem.codes),
        _lib.ptr(problem.offsets), problem.n, _lib.ptr(starts), T, int(Semantics.parse(semantics)), int(threads), K,
        radius, _lib.ptr(out)))
    return out


def search_targets_hits_cpu(problem: Problem, targets, min_score=None, thresholds=None, within=None,
                            semantics=Semantics.REFERENCE, threads: int = 0, radius: int = 0):
    """Per-target threshold hits on the CPU engine: ``(rows, toffsets)``. Pair p = i * T + t's hits are exactly
    :func:`search_hits_cpu`'s of record i against target t alone under the pair's threshold — int32 rows (score, n
    relative to the target's start, k), ascending in n, at ``rows[toffsets[p]:toffsets[p + 1]]``; ``toffsets`` is
    int64 [n * T + 1]. Exactly one of ``min_score`` (one int32 for the call; INT32_MIN selects every pair's whole
    target profile), ``thresholds`` (int32 [n, T], or [n] broadcast over the targets) and ``within`` (D >= 0: every
    placement within D of the pair's own best score, from :func:`search_targets_cpu`). A record longer than a target
    has no hits there. ``radius`` > 0 keeps the distinct placements only, the peaks of every pair's own profile as
    :func:`search_targets_topk_cpu` defines them: :func:`search_hits_cpu` with that radius on target t alone (a pair's
    best entry is always a peak, so ``within`` is relative to the same score). ValueError for an invalid target set
    ("targets: ...", first), for malformed thresholds, then for the radius ("distinct: ...")."""
    sem = Semantics.parse(semantics)
    starts = _starts_of(targets, problem.L1)
    T = starts.shape[0] - 1
    m, t, radius = _targets_hits_args(problem.n, T, min_score, thresholds, within, radius,
                                      lambda: search_targets_cpu(problem, starts, sem, threads))
    toffsets = np.zeros(problem.n * T + 1, np.int64)

    def call(rows, cap):
        _targets_rows_check(_lib.lib().moc_cpu_targets_hits_distinct(
            _lib.weights_arg(problem.weights.as_list()), _lib.ptr(problem.seq1), problem.L1, _lib.ptr(problem.codes),
            _lib.ptr(problem.offsets), problem.n, _lib.ptr(starts), T, int(sem), int(threads), m, _lib.ptr(t), radius,
            _lib.ptr(toffsets), _lib.ptr(rows), cap))

    call(None, 0)  # counts
    total = int(toffsets[-1])
    rows = np.zeros((total, 3), np.int32)
    if total:
        call(rows, total)
    return rows, toffsets


# ---- alignment report: sign counts and marker bytes of result rows (csrc/include/moc/cpu_engine.hpp)
REPORT_EMPTY = int(np.iinfo(np.int64).min)        # report_scores of an empty row (score INT32_MIN, top-K padding)
REPORT_INVALID = int(np.iinfo(np.int64).min) + 1  # ... of a row whose (n, k) does not place the record in Seq1


def _report_rows(rows, n: int):
    """``rows`` as [n, 3] / [n, K, 3] integers or RESULT_DTYPE [n] / [n, K] -> (int32 [n, K, 3], K, was_flat)."""
    r = np.asarray(rows)
    if r.dtype == RESULT_DTYPE:
        r = np.ascontiguousarray(r)
        r = r.view(np.int32).reshape(r.shape + (3,))
    flat = r.ndim == 2
    if flat:
        r = r[:, None, :]
    if r.ndim != 3 or r.shape[0] != n or r.shape[2] != 3:
        raise ValueError(f"report: rows must be [n, 3] or [n, K, 3] for the batch's n = {n}, got {np.shape(rows)}")
    return np.ascontiguousarray(r, dtype=np.int32), _check_k(r.shape[1]), flat


def search_report_cpu(problem: Problem, rows, marks: bool = False, threads: int = 0):
    """Sign counts of result rows on the CPU engine. ``rows``: [n, 3] or [n, K, 3] (score, n, k), e.g. from
    search_cpu / search_topk_cpu. Returns int32 counts [n, 4] or [n, K, 4] in PairClass order ($, %, #, space):
    zeros for an empty row (score INT32_MIN), -1 for a row whose n / k do not place the record inside Seq1, else
    the classes of the record's letter pairs (they sum to its length; :func:`report_scores` gives the score they
    stand for — the row's own score is not checked). With ``marks`` also a flat uint8 array of K * total
    marker bytes ('$', '%', '#', ' '; 0 for empty and invalid rows): row j of record i is the L2_i bytes at
    ``K * offsets[i] + j * L2_i``. No semantics: the spec-only final offset is a valid row."""
    r, K, flat = _report_rows(rows, problem.n)
    counts = np.zeros((problem.n, K, 4), np.int32)
    m = np.zeros(max(K * problem.total_chars, 1), np.uint8) if marks else None
    _lib.check(_lib.lib().moc_cpu_report(
        _lib.weights_arg(problem.weights.as_list()), _lib.ptr(problem.seq1), problem.L1, _lib.ptr(problem.codes),
        _lib.ptr(problem.offsets), problem.n, int(threads), K, _lib.ptr(r), _lib.ptr(counts), _lib.ptr(m)))
    counts = counts[:, 0] if flat else counts
    return (counts, m[:K * problem.total_chars]) if marks else counts


def report_scores(counts, weights) -> np.ndarray:
    """int64 W1*c[0] - W2*c[1] - W3*c[2] - W4*c[3] of report counts [..., 4]: the score a valid row's alignment
    really has. Empty rows give REPORT_EMPTY and invalid rows REPORT_INVALID (both outside the int32 range)."""
    c = np.asarray(counts, dtype=np.int64)
    w = Weights.of(weights)
    s = w.w1 * c[..., 0] - w.w2 * c[..., 1] - w.w3 * c[..., 2] - w.w4 * c[..., 3]
    s = np.where(c.sum(axis=-1) == 0, REPORT_EMPTY, s)
    return np.where(c[..., 0] < 0, REPORT_INVALID, s)


# ---- wire-format batches (csrc/include/moc/wire.hpp; parallel.wire.WireSlice holds one)
_LETTER_CODES = {"bytes": 0, "p5": 1, "p33": 3}


def _addr(a):
    return None if a is None else int(a.ctypes.data)


def wire_batch_of(ws, shift: int = 0):
    """A :class:`~..parallel.wire.WireSlice` as the native ``moc_wire_batch`` -> ``(batch, arrays)``; keep
    ``arrays`` alive while ``batch`` is in use. ``shift`` > 0: the slice's sparse offsets, one per 2^shift records
    (``WireSlice.wire_offsets``), which need its narrow lengths."""
    shift = int(shift)
    if shift and ws.lengths is None:
        raise ValueError("sparse offsets need narrow lengths (this slice's lengths are too wide for them)")
    offsets = ws.wire_offsets(shift)
    arrays = (ws.codes, offsets, ws.lengths)
    for a in arrays:
        assert a is None or a.flags["C_CONTIGUOUS"]
    b = _lib.WireBatch(letters=_addr(ws.codes), offsets=_addr(offsets), lengths=_addr(ws.lengths), n=int(ws.n),
                       len_base=int(ws.len_base), packed=_LETTER_CODES[ws.letter_format], off_shift=shift,
                       len_bits=int(ws.len_bits or 8), device=0)
    return b, arrays


def decode_wire_cpu(ws, shift: int = 0):
    """Host reference decode of a wire batch (``moc::decode_wire_cpu``): ``(codes, offsets)`` — one byte per letter
    (P33 letters read back as 1..26) and the int64 [n + 1] dense offsets, ``offsets[0]`` the batch's first letter.
    ``ws``: a WireSlice (``shift`` > 0: through its sparse offsets) or a ``_lib.WireBatch`` of host pointers. A batch
    whose form or lengths are inconsistent raises :class:`~.._lib.NativeError`."""
    b, keep = (ws, None) if isinstance(ws, _lib.WireBatch) else wire_batch_of(ws, shift)
    sizes = np.zeros(2, np.int64)
    _lib.check(_lib.lib().moc_cpu_decode_wire(ctypes.byref(b), None, None, _lib.ptr(sizes)))
    codes = np.empty(int(sizes[0]), np.uint8)
    offsets = np.empty(int(sizes[1]) // 8, np.int64)
    _lib.check(_lib.lib().moc_cpu_decode_wire(ctypes.byref(b), _lib.ptr(codes), _lib.ptr(offsets), None))
    del keep
    return codes, offsets


class _DeviceMemory:
    """Device memory of the native engine as an object torch.as_tensor takes (the CUDA array interface)."""

    def __init__(self, address: int, count: int, typestr: str):
        self.__cuda_array_interface__ = {"shape": (int(count),), "typestr": typestr, "data": (int(address), False),
                                         "version": 2, "strides": None}


def brute_force_native(problem: Problem, semantics=Semantics.REFERENCE) -> np.ndarray:
    """Literal O(L1*L2^2) replay of the reference loops, in C++ (test oracle)."""
    out = empty_results(problem.n)
    _lib.check(_lib.lib().moc_brute_force(
        _lib.weights_arg(problem.weights.as_list()), _lib.ptr(problem.seq1), problem.L1,
        _lib.ptr(problem.codes), _lib.ptr(problem.offsets), problem.n, int(Semantics.parse(semantics)),
        _lib.ptr(out)))
    return out


def native_score_table(weights) -> np.ndarray:
    lut = np.zeros((32, 32), np.int32)
    _lib.check(_lib.lib().moc_score_table(_lib.weights_arg(Weights.of(weights).as_list()), _lib.ptr(lut), None))
    return lut


# ---------------------------------------------------------------------------------------------- GPU
def device_count() -> int:
    return int(_lib.lib().moc_device_count())


def device_info(device: int = 0) -> dict:
    buf = ctypes.create_string_buffer(1024)
    _lib.check(_lib.lib().moc_device_info_json(device, buf, 1024))
    return json.loads(buf.value.decode())


def _format_id(fmt) -> int:
    if isinstance(fmt, (int, np.integer)):
        return int(fmt)
    return _lib.FORMAT_NAMES.index(str(fmt).lower())


class HipSearchEngine:
    """Per-rank gfx950 engine: problem upload, planning, and host<->device data movement.

    ``solve`` picks the zero-copy streaming path automatically when every host buffer is pinned
    (``pin`` / ``_lib.Pinned`` / hipHostMalloc) and all records fit the short kernel; otherwise it runs
    the staged double-buffered chunk pipeline (csrc/src/hip_engine.cpp)."""

    def __init__(self, device: Optional[int] = None, chunk_records: int = 0, chunk_bytes: int = 0,
                 allow_direct: bool = True):
        L = _lib.lib()
        if L.moc_device_count() <= 0:
            raise _lib.NativeError("HipSearchEngine needs a visible HIP device (none found)")
        self._h = L.moc_engine_create(-1 if device is None else int(device), int(chunk_records), int(chunk_bytes),
                                      1 if allow_direct else 0)
        if not self._h:
            raise _lib.NativeError(L.moc_last_error().decode())
        self.problem_L1 = None
        self._problem_key = None  # (weights, seq1, semantics) bytes of the problem in the engine
        self._stats_buf = (ctypes.c_double * 14)()

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().moc_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_problem(self, weights, seq1: np.ndarray, semantics=Semantics.REFERENCE):
        seq1 = np.ascontiguousarray(seq1, dtype=np.uint8)
        if isinstance(weights, np.ndarray) and semantics is Semantics.REFERENCE:
            # a job loop re-sending the same problem (the engine keeps an unchanged image anyway): no
            # conversion or native call at all
            key = (weights.tobytes(), seq1.tobytes())
            if key == self._problem_key:
                return
        else:
            key = None
        self._problem_key = None  # not current until the native call succeeds
        _lib.check(_lib.lib().moc_engine_set_problem(
            self._h, _lib.weights_arg(Weights.of(weights).as_list()), _lib.ptr(seq1), seq1.shape[0],
            int(Semantics.parse(semantics))))
        self.problem_L1 = int(seq1.shape[0])
        self._problem_key = key

    def pin(self, *arrays):
        """Page-locks host arrays for the engine's lifetime (enables the zero-copy path)."""
        for a in arrays:
            if a is not None and a.nbytes:
                _lib.check(_lib.lib().moc_engine_pin(self._h, ctypes.c_void_p(a.ctypes.data), a.nbytes))

    def auto_format(self, max_l2: int, min_l2: int = 0) -> str:
        """Smallest result format for records of lengths [min_l2, max_l2] (min_l2 = 0: unknown -> no R2)."""
        return _lib.FORMAT_NAMES[_lib.lib().moc_engine_auto_format(self._h, int(max_l2), int(min_l2))]

    def r2_params(self, min_l2: int, max_l2: int) -> tuple:
        """(smin, kw, j) of the R2 format for records of lengths [min_l2, max_l2]."""
        v = np.zeros(3, np.int32)
        _lib.check(_lib.lib().moc_engine_r2_params(self._h, int(min_l2), int(max_l2), _lib.ptr(v)))
        return tuple(int(x) for x in v)

    def solve(self, codes: np.ndarray, offsets: np.ndarray, out: Optional[np.ndarray] = None,
              lengths: Optional[np.ndarray] = None, fmt="r12", l2_range=None, packed5: bool = False,
              lengths_bits: int = 8, lengths_base: int = 0,
              packed33: bool = False) -> np.ndarray:
        """Host CSR -> host results. ``codes[offsets[i]:offsets[i+1]]`` is record i (``offsets`` may be a
        slice of a larger absolute offset array). ``fmt``: r12 | r8 | r4 | r2 | auto (smallest that fits);
        ``lengths``: optional narrow record lengths, uint8 (``lengths_bits`` 8) or two per byte
        (``lengths_bits`` 4, low nibble first, length = ``lengths_base`` + nibble; see pack_lengths4) or
        3-bit fields (``lengths_bits`` 3, see pack_lengths3);
        ``l2_range``: optional known (min, max) length (R2 results are encoded for it: decode with
        ``r2_params(*l2_range)`` or ``stats()["r2"]``); ``packed5``: ``codes`` is a 5-bit packed stream
        (models.problem.pack5) instead of bytes; ``packed33``: 33-bit fields of 7 letters
        (models.problem.pack33)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = offsets.shape[0] - 1
        if l2_range is None and (fmt == "auto"):
            L2 = np.diff(offsets) if n else np.zeros(1, np.int64)
            l2_range = (int(L2.min()) if n else 0, int(L2.max()) if n else 0)
        if fmt == "auto":
            fmt = self.auto_format(l2_range[1], l2_range[0])
        fid = _format_id(fmt)
        if out is None:
            out = np.empty(n, dtype=_lib.FORMAT_DTYPES[fid])
        assert out.dtype.itemsize == _lib.FORMAT_DTYPES[fid].itemsize and out.size >= n
        if lengths is not None:
            need = (n if lengths_bits == 8 else (n + 1) // 2 if lengths_bits == 4
                    else 8 * ((n + 23) // 24) if lengths_bits == 6 else (3 * n + 7) // 8 + 1)
            assert lengths.dtype == np.uint8 and lengths.shape[0] >= need
        lo, hi = l2_range if l2_range is not None else (-1, -1)
        _lib.check(_lib.lib().moc_engine_solve_ex(self._h, _lib.ptr(codes), _lib.ptr(offsets), _lib.ptr(lengths),
                                                  int(lengths_bits), int(lengths_base), n, _lib.ptr(out), fid, int(lo),
                                                  int(hi), 3 if packed33 else 1 if packed5 else 0))
        return out

    def solve_device(self, codes_t, offsets_t, h_offsets: np.ndarray, out_t, stream=None):
        """Device-resident batch (torch tensors on this engine's device). ``codes_t`` is the base so that
        record i starts at codes_t[offsets[i]] (absolute offsets: the batch may be a slice of a larger CSR array,
        any first offset, any byte alignment); ``out_t`` is int32 [n, 3], possibly a row slice of a larger tensor.
        Queued on ``stream`` (torch.cuda.Stream, default: the current stream); returns immediately. In every device
        form torch's default stream (handle 0) stands for the engine's own compute stream, which torch's operations
        on the default stream are not ordered with: synchronise, or pass a stream of your own, before torch reads
        the results."""
        import torch

        h_offsets = np.ascontiguousarray(h_offsets, dtype=np.int64)
        n = h_offsets.shape[0] - 1
        assert codes_t.dtype == torch.uint8 and offsets_t.dtype == torch.int64 and out_t.dtype == torch.int32
        assert offsets_t.numel() == n + 1 and out_t.shape == (n, 3)
        if stream is None:
            stream = torch.cuda.current_stream(codes_t.device)
        _lib.check(_lib.lib().moc_engine_solve_device(
            self._h, ctypes.c_void_p(codes_t.data_ptr()), ctypes.c_void_p(offsets_t.data_ptr()), _lib.ptr(h_offsets),
            n, ctypes.c_void_p(out_t.data_ptr()), ctypes.c_void_p(stream.cuda_stream)))
        return out_t

    def solve_wire_device(self, letters_t, offsets_t, lengths_t, n: int, out_t, fmt: str, l2_range,
                          lengths_bits: int = 8, lengths_base: int = 0, packed33: bool = True, off_shift: int = 0):
        """Device-resident batch in the wire formats (torch tensors on this engine's GPU, as the rccl transport
        holds them): ``letters_t`` P33 fields (``packed33``) or bytes, ``offsets_t`` int64 [n + 1] letter
        offsets, ``lengths_t`` narrow lengths (as ``solve``'s) or None, results into ``out_t`` (a uint8
        tensor of n * itemsize bytes of ``fmt``, decoded on the host as ``solve``'s). ``off_shift`` > 0:
        ``offsets_t`` is sparse, one entry per 2^off_shift records and the batch end (``sparse_offsets``),
        and ``lengths_t`` is required; the sparse form trusts ``l2_range`` (the lengths are narrow fields in device
        memory: the check below needs dense offsets). Synchronous; ``stats()["kernel_ms"]`` is the kernel's time."""
        import torch

        fid = _format_id(fmt)
        entries = n + 1 if not off_shift else ((n + (1 << off_shift) - 1) >> off_shift) + 1
        assert letters_t.dtype == torch.uint8 and offsets_t.dtype == torch.int64 and offsets_t.numel() == entries
        assert out_t.dtype == torch.uint8 and out_t.numel() >= n * _lib.FORMAT_DTYPES[fid].itemsize
        assert not off_shift or lengths_t is not None, "sparse offsets need narrow lengths"
        if n > 0 and not off_shift:
            # the kernel sizes its LDS and per-lane record words from l2_range and cannot re-scan device
            # lengths: a range narrower than the batch would give wrong results, so it is checked here (dense
            # offsets only: sparse ones do not hold the lengths, and the caller's range is taken as stated)
            d = offsets_t[1:] - offsets_t[:-1]
            lo, hi = int(d.min()), int(d.max())
            if lo < int(l2_range[0]) or hi > int(l2_range[1]):
                raise ValueError(f"l2_range {tuple(l2_range)} does not hold the batch's lengths [{lo}, {hi}]")
        lp = ctypes.c_void_p(lengths_t.data_ptr()) if lengths_t is not None else None
        tail = (lp, int(lengths_bits), int(lengths_base), int(n), ctypes.c_void_p(out_t.data_ptr()), fid,
                int(l2_range[0]), int(l2_range[1]), 3 if packed33 else 0)
        head = (self._h, ctypes.c_void_p(letters_t.data_ptr()), ctypes.c_void_p(offsets_t.data_ptr()))
        if off_shift:
            _lib.check(_lib.lib().moc_engine_solve_wire_device_sparse(*head, int(off_shift), *tail))
        else:
            _lib.check(_lib.lib().moc_engine_solve_wire_device(*head, *tail))
        return out_t

    def device_kernel_ms(self) -> float:
        """Device time (ms) of the last solve_device's kernels, from events around its launches (after the
        host's per-call planning); waits for them."""
        ms = ctypes.c_double(0.0)
        _lib.check(_lib.lib().moc_engine_device_kernel_ms(self._h, ctypes.addressof(ms)))
        return float(ms.value)

    def search_keys(self, codes: np.ndarray, offsets: np.ndarray, part: int, parts: int) -> np.ndarray:
        """Context-parallel partial search on the GPU: this engine's share (part of parts) of the batch's
        offset tiles -> packed uint64 keys per record (see :func:`search_keys_cpu`)."""
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = offsets.shape[0] - 1
        keys = np.zeros(n, np.uint64)
        _lib.check(_lib.lib().moc_engine_search_keys(self._h, _lib.ptr(codes), _lib.ptr(offsets), n, int(part),
                                                     int(parts), _lib.ptr(keys)))
        return keys

    def search_keys_device(self, codes_t, offsets_t, h_offsets: np.ndarray, part: int, parts: int, keys_t,
                           stream=None):
        """Device-resident form: keys_t is an int64 tensor [n] receiving the uint64 key bits."""
        import torch

        h_offsets = np.ascontiguousarray(h_offsets, dtype=np.int64)
        n = h_offsets.shape[0] - 1
        assert keys_t.dtype == torch.int64 and keys_t.numel() == n
        if stream is None:
            stream = torch.cuda.current_stream(codes_t.device)
        _lib.check(_lib.lib().moc_engine_search_keys_device(
            self._h, ctypes.c_void_p(codes_t.data_ptr()), ctypes.c_void_p(offsets_t.data_ptr()), _lib.ptr(h_offsets),
            n, int(part), int(parts), ctypes.c_void_p(keys_t.data_ptr()), ctypes.c_void_p(stream.cuda_stream)))
        return keys_t

    def finalize_keys_device(self, codes_t, offsets_t, h_offsets: np.ndarray, keys_t, out_t, stream=None):
        """MAX-combined device keys -> int32 [n, 3] results (score, n, k); k is resolved on each record's
        winning diagonal, so the batch (codes_t, offsets_t from 0, host copy h_offsets) is needed."""
        import torch

        n = keys_t.numel()
        assert out_t.dtype == torch.int32 and out_t.shape == (n, 3)
        h_offsets = np.ascontiguousarray(h_offsets, dtype=np.int64)
        if stream is None:
            stream = torch.cuda.current_stream(keys_t.device)
        _lib.check(_lib.lib().moc_engine_finalize_keys_device(
            self._h, ctypes.c_void_p(codes_t.data_ptr()), ctypes.c_void_p(offsets_t.data_ptr()), _lib.ptr(h_offsets),
            n, ctypes.c_void_p(keys_t.data_ptr()), ctypes.c_void_p(out_t.data_ptr()), 0,
            ctypes.c_void_p(stream.cuda_stream)))
        return out_t

    # ---- per-offset score profile and top-K alignments (byte letters, dense offsets)
    def profile_offsets(self, offsets: np.ndarray) -> np.ndarray:
        """int64 [n + 1] profile index of a batch for the engine's problem (see :func:`profile_offsets`)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = offsets.shape[0] - 1
        poffsets = np.zeros(n + 1, np.int64)
        _lib.check(_lib.lib().moc_engine_solve_profile(self._h, None, _lib.ptr(offsets), n, _lib.ptr(poffsets), None))
        return poffsets

    def solve_profile(self, codes: np.ndarray, offsets: np.ndarray):
        """Host CSR -> ``(prof, poffsets)`` as :func:`search_profile_cpu` returns them, computed by the profile
        kernel (csrc/src/hip/profile_kernels.hip). Synchronous."""
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = offsets.shape[0] - 1
        poffsets = self.profile_offsets(offsets)
        prof = np.zeros(max(int(poffsets[-1]), 1), dtype=PROFILE_DTYPE)  # never a NULL pointer: NULL asks for poffsets
        _lib.check(_lib.lib().moc_engine_solve_profile(self._h, _lib.ptr(codes), _lib.ptr(offsets), n,
                                                       _lib.ptr(poffsets), _lib.ptr(prof)))
        return prof[:int(poffsets[-1])], poffsets

    def solve_topk(self, codes: np.ndarray, offsets: np.ndarray, K: int, radius: int = 0) -> np.ndarray:
        """Host CSR -> int32 [n, K, 3] top-K rows as :func:`search_topk_cpu` returns them. The batch's profile
        is never materialised: records run in chunks whose profile scratch stays under the bound of
        :meth:`set_profile_scratch` (default 256 MiB). Synchronous. ``radius`` > 0 (here and in every top-K and
        hits call of the engine): distinct placements, as :func:`search_topk_cpu` — the peak kernels
        (csrc/src/hip/peaks_kernels.hip) run between each chunk's profile and its select, ``stats()["kernels"]``
        names ``peaks``; ``radius=0`` is the plain call, launch for launch."""
        K = _check_k(K)
        radius = _check_radius(radius)
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = offsets.shape[0] - 1
        out = np.zeros((n, K, 3), np.int32)
        if radius:
            _lib.check(_lib.lib().moc_engine_solve_topk_distinct(self._h, _lib.ptr(codes), _lib.ptr(offsets), n, K,
                                                                 radius, _lib.ptr(out)))
        else:
            _lib.check(_lib.lib().moc_engine_solve_topk(self._h, _lib.ptr(codes), _lib.ptr(offsets), n, K,
                                                        _lib.ptr(out)))
        return out

    def solve_profile_device(self, codes_t, offsets_t, h_offsets: np.ndarray, prof_t=None, stream=None):
        """Device-resident batch (as :meth:`solve_device`) -> ``(prof_t, poffsets)``: ``prof_t`` an int32
        [total, 2] tensor of (score, k) entries on the codes' device (allocated when None), ``poffsets`` the host
        index. Queued on ``stream`` (default: the current stream); returns immediately."""
        import torch

        h_offsets = np.ascontiguousarray(h_offsets, dtype=np.int64)
        n = h_offsets.shape[0] - 1
        poffsets = self.profile_offsets(h_offsets)
        total = int(poffsets[-1])
        if prof_t is None:
            prof_t = torch.empty((total, 2), dtype=torch.int32, device=codes_t.device)
        assert codes_t.dtype == torch.uint8 and offsets_t.dtype == torch.int64 and offsets_t.numel() == n + 1
        assert prof_t.dtype == torch.int32 and prof_t.shape == (total, 2) and prof_t.is_contiguous()
        if stream is None:
            stream = torch.cuda.current_stream(codes_t.device)
        _lib.check(_lib.lib().moc_engine_solve_profile_device(
            self._h, ctypes.c_void_p(codes_t.data_ptr()), ctypes.c_void_p(offsets_t.data_ptr()), _lib.ptr(h_offsets),
            n, ctypes.c_void_p(prof_t.data_ptr()), ctypes.c_void_p(stream.cuda_stream)))
        return prof_t, poffsets

    def solve_topk_device(self, codes_t, offsets_t, h_offsets: np.ndarray, K: int, out_t, stream=None,
                          radius: int = 0):
        """Device-resident batch -> ``out_t``, an int32 [n, K, 3] tensor of top-K rows. Queued on ``stream``
        (default: the current stream); returns immediately. ``radius``: as :meth:`solve_topk`."""
        import torch

        K = _check_k(K)
        radius = _check_radius(radius)
        h_offsets = np.ascontiguousarray(h_offsets, dtype=np.int64)
        n = h_offsets.shape[0] - 1
        assert codes_t.dtype == torch.uint8 and offsets_t.dtype == torch.int64 and offsets_t.numel() == n + 1
        assert out_t.dtype == torch.int32 and out_t.shape == (n, K, 3) and out_t.is_contiguous()
        if stream is None:
            stream = torch.cuda.current_stream(codes_t.device)
        head = (self._h, ctypes.c_void_p(codes_t.data_ptr()), ctypes.c_void_p(offsets_t.data_ptr()),
                _lib.ptr(h_offsets), n, K)
        tail = (ctypes.c_void_p(out_t.data_ptr()), ctypes.c_void_p(stream.cuda_stream))
        if radius:
            _lib.check(_lib.lib().moc_engine_solve_topk_device_distinct(*head, radius, *tail))
        else:
            _lib.check(_lib.lib().moc_engine_solve_topk_device(*head, *tail))
        return out_t

    def set_profile_scratch(self, nbytes: int):
        """Bound (bytes) of the profile scratch a top-K call may hold; a record whose profile is larger still
        runs, alone in its chunk. ``stats()["chunks"]`` reports the chunks of the last call."""
        _lib.check(_lib.lib().moc_engine_set_profile_scratch(self._h, int(nbytes)))

    def topk_select_ms(self) -> float:
        """Device time (ms) of the select launches of the last top-K call; 0 unless the engine was created with
        MOC_PROFILE_TIMING=1 in the environment. Waits for them."""
        ms = ctypes.c_double(0.0)
        _lib.check(_lib.lib().moc_engine_topk_select_ms(self._h, ctypes.addressof(ms)))
        return float(ms.value)

    # ---- threshold hits (byte letters, dense offsets; csrc/src/hip/hits_kernels.hip)
    def solve_hits(self, codes: np.ndarray, offsets: np.ndarray, min_score=None, thresholds=None, within=None,
                   max_rows: Optional[int] = None, radius: int = 0):
        """Host CSR -> ``(rows, hoffsets)`` as :func:`search_hits_cpu` returns them (exactly one of ``min_score``,
        ``thresholds``, ``within``), through the chunks of :meth:`solve_topk` with count, prefix sum and compaction
        kernels behind each chunk's profile. Optimistic: one pass with room for ``max_rows`` rows (default 4 n) and
        exactly one more when more offsets qualify (:meth:`hits_passes`). Synchronous. ``radius`` > 0: only the hits
        that are peaks of that radius, as :func:`search_hits_cpu` (see :meth:`solve_topk`)."""
        radius = _check_radius(radius)
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = offsets.shape[0] - 1
        m, t = _hits_thresholds(n, min_score, thresholds, within, lambda: self.solve(codes, offsets)["score"])
        hoffsets = np.zeros(n + 1, np.int64)
        head = (self._h, _lib.ptr(codes), _lib.ptr(offsets), n, m, _lib.ptr(t))
        tail = (-1 if max_rows is None else int(max_rows), _lib.ptr(hoffsets), None, 0)
        if radius:
            _lib.check(_lib.lib().moc_engine_solve_hits_distinct(*head, radius, *tail))
        else:
            _lib.check(_lib.lib().moc_engine_solve_hits(*head, *tail))
        total = int(hoffsets[-1])
        rows = np.zeros((total, 3), np.int32)
        _lib.check(_lib.lib().moc_engine_hits_rows(_lib.ptr(rows) if total else None, total))
        return rows, hoffsets

    def hits_passes(self) -> int:
        """Passes the last :meth:`solve_hits` took: 1, or 2 when its first capacity was too small."""
        return int(_lib.lib().moc_engine_hits_passes(self._h))

    def hits_select_ms(self) -> float:
        """Device time (ms) of the count, scan and compact launches of the last hits call; 0 unless the engine was
        created with MOC_PROFILE_TIMING=1 in the environment. Waits for them."""
        ms = ctypes.c_double(0.0)
        _lib.check(_lib.lib().moc_engine_hits_select_ms(self._h, ctypes.addressof(ms)))
        return float(ms.value)

    def solve_hits_device(self, codes_t, offsets_t, h_offsets: np.ndarray, min_score=None, thresholds_t=None,
                          within=None, cap: Optional[int] = None, rows_t=None, hoffsets_t=None, stream=None,
                          radius: int = 0):
        """Device-resident batch (as :meth:`solve_device`) -> ``(rows_t, hoffsets_t)``: ``hoffsets_t`` an int64
        [n + 1] tensor, always complete and exact; ``rows_t`` an int32 [cap, 3] tensor (``cap`` default 4 n) of
        which the rows with a flat index < cap are written and nothing else is touched — compare
        ``hoffsets_t[-1]`` with ``cap`` after a sync. ``cap = 0`` counts only. Exactly one of ``min_score``,
        ``thresholds_t`` (an int32 [n] tensor on the same device, e.g. built from a search's scores) and ``within``
        (a search queued on the same stream first). Both tensors are allocated when None. Queued on ``stream``
        (default: the current stream); returns immediately — except ``within`` on torch's default stream, which
        stands for the engine's own compute stream: that call waits for its search on the host, since torch's
        operations on the default stream are not ordered with that stream. ``radius``: as :meth:`solve_hits`."""
        import torch

        radius = _check_radius(radius)
        h_offsets = np.ascontiguousarray(h_offsets, dtype=np.int64)
        n = h_offsets.shape[0] - 1
        if sum(x is not None for x in (min_score, thresholds_t, within)) != 1:
            raise ValueError("hits: give exactly one of min_score, thresholds, within")
        assert codes_t.dtype == torch.uint8 and offsets_t.dtype == torch.int64 and offsets_t.numel() == n + 1
        if stream is None:
            stream = torch.cuda.current_stream(codes_t.device)
        if within is not None:
            d = int(within)
            if d < 0:
                raise ValueError(f"hits: within must be >= 0, got {d}")
            best = torch.empty((n, 3), dtype=torch.int32, device=codes_t.device)
            self.solve_device(codes_t, offsets_t, h_offsets, best, stream)
            # torch's default stream (handle 0) stands for the engine's own compute stream, which torch's operations
            # are not ordered with: there the search is waited for before the thresholds are formed, and the
            # thresholds before the hits kernels are queued. Any other stream orders the three by itself.
            own = not stream.cuda_stream
            if own and n > 0:
                self.device_kernel_ms()
            with torch.cuda.stream(stream):
                thresholds_t = (best[:, 0].to(torch.int64) - d).clamp(_I32.min, _I32.max).to(torch.int32).contiguous()
            if own:
                stream.synchronize()
        m = 0
        if min_score is not None:
            m = int(min_score)
            if not _I32.min <= m <= _I32.max:
                raise ValueError(f"hits: min_score {m} is not an int32")
        if thresholds_t is not None:
            if thresholds_t.dtype != torch.int32 or tuple(thresholds_t.shape) != (n,):
                raise ValueError(f"hits: thresholds must be an int32 tensor of {n} entries (one per record)")
            assert thresholds_t.is_contiguous() and thresholds_t.device == codes_t.device
        if cap is None:
            cap = max(4 * n, 1) if rows_t is None else rows_t.shape[0]
        cap = int(cap)
        if cap < 0:
            raise ValueError("hits: cap must be >= 0")
        if rows_t is None:
            rows_t = torch.empty((cap, 3), dtype=torch.int32, device=codes_t.device)
        if hoffsets_t is None:
            hoffsets_t = torch.empty(n + 1, dtype=torch.int64, device=codes_t.device)
        assert rows_t.dtype == torch.int32 and rows_t.is_contiguous() and rows_t.dim() == 2 and rows_t.shape[1] == 3
        assert rows_t.shape[0] >= cap
        assert hoffsets_t.dtype == torch.int64 and hoffsets_t.is_contiguous() and hoffsets_t.numel() == n + 1
        head = (self._h, ctypes.c_void_p(codes_t.data_ptr()), ctypes.c_void_p(offsets_t.data_ptr()),
                _lib.ptr(h_offsets), n, m,
                ctypes.c_void_p(thresholds_t.data_ptr()) if thresholds_t is not None else None)
        tail = (ctypes.c_void_p(hoffsets_t.data_ptr()), ctypes.c_void_p(rows_t.data_ptr()) if cap else None, cap,
                ctypes.c_void_p(stream.cuda_stream))
        if radius:
            _lib.check(_lib.lib().moc_engine_solve_hits_device_distinct(*head, radius, *tail))
        else:
            _lib.check(_lib.lib().moc_engine_solve_hits_device(*head, *tail))
        return rows_t, hoffsets_t

    # ---- profile summary (byte letters, dense offsets; csrc/src/hip/summary_kernels.hip)
    def solve_summary(self, codes: np.ndarray, offsets: np.ndarray, bins: int = 0, lo: int = 0, width: int = 1):
        """Host CSR -> ``(summary, hist)`` as :func:`search_summary_cpu` returns them, through the chunks of
        :meth:`solve_hits` with the summary kernel (and, with ``bins`` > 0, the histogram kernel) behind each chunk's
        profile: 56 + 4 ``bins`` bytes come back per record, never the profile. Synchronous;
        ``stats()["kernels"]`` names ``summary``. ValueError as :func:`search_summary_cpu`, raised before anything is
        launched and without a change to ``stats()``."""
        bins, lo, width = _summary_args(bins, lo, width)
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = offsets.shape[0] - 1
        summary = np.zeros((n, len(SUMMARY_COLS)), np.int64)
        hist = np.zeros((n, bins), np.int32) if bins else None
        _summary_check(_lib.lib().moc_engine_solve_summary(self._h, _lib.ptr(codes), _lib.ptr(offsets), n, bins, lo,
                                                           width, _lib.ptr(summary), _lib.ptr(hist)))
        return summary, hist

    def summary_ms(self) -> float:
        """Device time (ms) of the summary and histogram launches of the last summary call; 0 unless the engine was
        created with MOC_PROFILE_TIMING=1 in the environment. Waits for them."""
        ms = ctypes.c_double(0.0)
        _lib.check(_lib.lib().moc_engine_summary_ms(self._h, ctypes.addressof(ms)))
        return float(ms.value)

    def solve_summary_device(self, codes_t, offsets_t, h_offsets: np.ndarray, bins: int = 0, lo: int = 0,
                             width: int = 1, summary_t=None, hist_t=None, stream=None):
        """Device-resident batch (as :meth:`solve_device`) -> ``(summary_t, hist_t)``: an int64 [n, 7] tensor and,
        with ``bins`` > 0, an int32 [n, bins] tensor on the codes' device (allocated when None; every element of
        both is written). With ``bins = 0`` no histogram work is launched, ``hist_t`` is returned as given (None
        unless passed) and not touched. Queued on ``stream`` (default: the current stream); returns immediately —
        :func:`summary_thresholds` of ``summary_t`` and :meth:`solve_hits_device` can follow on the same stream.
        ValueError as :meth:`solve_summary`."""
        import torch

        bins, lo, width = _summary_args(bins, lo, width)
        h_offsets = np.ascontiguousarray(h_offsets, dtype=np.int64)
        n = h_offsets.shape[0] - 1
        assert codes_t.dtype == torch.uint8 and offsets_t.dtype == torch.int64 and offsets_t.numel() == n + 1
        if stream is None:
            stream = torch.cuda.current_stream(codes_t.device)
        if summary_t is None:
            summary_t = torch.empty((n, len(SUMMARY_COLS)), dtype=torch.int64, device=codes_t.device)
        if hist_t is None and bins:
            hist_t = torch.empty((n, bins), dtype=torch.int32, device=codes_t.device)
        assert summary_t.dtype == torch.int64 and summary_t.is_contiguous()
        assert tuple(summary_t.shape) == (n, len(SUMMARY_COLS))
        if bins:
            assert hist_t.dtype == torch.int32 and hist_t.is_contiguous() and tuple(hist_t.shape) == (n, bins)
        _summary_check(_lib.lib().moc_engine_solve_summary_device(
            self._h, ctypes.c_void_p(codes_t.data_ptr()), ctypes.c_void_p(offsets_t.data_ptr()), _lib.ptr(h_offsets),
            n, bins, lo, width, ctypes.c_void_p(summary_t.data_ptr()),
            ctypes.c_void_p(hist_t.data_ptr()) if bins else None, ctypes.c_void_p(stream.cuda_stream)))
        return summary_t, hist_t

    def solve_summary_wire(self, ws, bins: int = 0, lo: int = 0, width: int = 1, shift: int = 0):
        """Host wire batch -> ``(summary, hist)``, as :meth:`solve_summary` on the decoded records. See
        :meth:`solve_profile_wire`."""
        bins, lo, width = _summary_args(bins, lo, width)
        b, keep = wire_batch_of(ws, shift)
        n = ws.n
        summary = np.zeros((n, len(SUMMARY_COLS)), np.int64)
        hist = np.zeros((n, bins), np.int32) if bins else None
        _summary_check(_lib.lib().moc_engine_solve_summary_wire(self._h, ctypes.byref(b), bins, lo, width,
                                                                _lib.ptr(summary), _lib.ptr(hist)))
        del keep
        return summary, hist

    # ---- multi-target search (byte letters, dense offsets; csrc/src/hip/targets_kernels.hip)
    def solve_targets(self, codes: np.ndarray, offsets: np.ndarray, targets) -> np.ndarray:
        """Host CSR -> int32 [n, T, 3] rows as :func:`search_targets_cpu` returns them, against the engine's Seq1
        as the catalog of ``targets`` (a :class:`TargetSet` or its starts; ``set_problem(weights, ts.seq1)``
        first). One pass: the chunks of :meth:`solve_hits` with the targets select kernel behind each chunk's
        catalog profile — 12 T bytes come back per record, never the profile. Synchronous;
        ``stats()["kernels"]`` names ``targets``. ValueError for an invalid target set, raised before anything is
        launched and without a change to ``stats()``."""
        starts = _starts_of(targets, self.problem_L1)
        T = starts.shape[0] - 1
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = offsets.shape[0] - 1
        out = np.zeros((n, T, 3), np.int32)
        _targets_check(_lib.lib().moc_engine_solve_targets(self._h, _lib.ptr(codes), _lib.ptr(offsets), n,
                                                           _lib.ptr(starts), T, _lib.ptr(out)))
        return out

    def targets_ms(self) -> float:
        """Device time (ms) of the targets select launches of the last targets call; 0 unless the engine was
        created with MOC_PROFILE_TIMING=1 in the environment. Waits for them."""
        ms = ctypes.c_double(0.0)
        _lib.check(_lib.lib().moc_engine_targets_ms(self._h, ctypes.addressof(ms)))
        return float(ms.value)

    def solve_targets_device(self, codes_t, offsets_t, h_offsets: np.ndarray, targets, out_t=None, starts_t=None,
                             stream=None):
        """Device-resident batch (as :meth:`solve_device`) -> ``out_t``, an int32 [n, T, 3] tensor of multi-target
        rows on the codes' device (allocated when None; every row is written). ``starts_t``: an int64 [T + 1]
        device copy of the starts, or None — then the engine uploads them with its plan. Queued on ``stream``
        (default: the current stream); returns immediately — :func:`targets_catalog_rows` and
        :meth:`report_device` can follow on the same stream. ValueError as :meth:`solve_targets`."""
        import torch

        starts = _starts_of(targets, self.problem_L1)
        T = starts.shape[0] - 1
        h_offsets = np.ascontiguousarray(h_offsets, dtype=np.int64)
        n = h_offsets.shape[0] - 1
        assert codes_t.dtype == torch.uint8 and offsets_t.dtype == torch.int64 and offsets_t.numel() == n + 1
        if stream is None:
            stream = torch.cuda.current_stream(codes_t.device)
        if out_t is None:
            out_t = torch.empty((n, T, 3), dtype=torch.int32, device=codes_t.device)
        assert out_t.dtype == torch.int32 and out_t.is_contiguous() and tuple(out_t.shape) == (n, T, 3)
        if starts_t is not None:
            assert starts_t.dtype == torch.int64 and starts_t.is_contiguous() and starts_t.numel() == T + 1
        _targets_check(_lib.lib().moc_engine_solve_targets_device(
            self._h, ctypes.c_void_p(codes_t.data_ptr()), ctypes.c_void_p(offsets_t.data_ptr()), _lib.ptr(h_offsets),
            n, ctypes.c_void_p(starts_t.data_ptr()) if starts_t is not None else None, _lib.ptr(starts), T,
            ctypes.c_void_p(out_t.data_ptr()), ctypes.c_void_p(stream.cuda_stream)))
        return out_t

    def solve_targets_wire(self, ws, targets, shift: int = 0) -> np.ndarray:
        """Host wire batch -> int32 [n, T, 3] multi-target rows, as :meth:`solve_targets` on the decoded records.
        See :meth:`solve_profile_wire`."""
        starts = _starts_of(targets, self.problem_L1)
        T = starts.shape[0] - 1
        b, keep = wire_batch_of(ws, shift)
        out = np.zeros((ws.n, T, 3), np.int32)
        _targets_check(_lib.lib().moc_engine_solve_targets_wire(self._h, ctypes.byref(b), _lib.ptr(starts), T,
                                                                _lib.ptr(out)))
        del keep
        return out

    # ---- target ranking (byte letters, dense offsets; csrc/src/hip/targets_rank_kernels.hip)
    def solve_targets_rank(self, codes: np.ndarray, offsets: np.ndarray, targets, M: int) -> np.ndarray:
        """Host CSR -> int32 [n, M, 4] rank rows (columns :data:`RANK_COLS`) as :func:`search_targets_rank_cpu`
        returns them, against the engine's Seq1 as the catalog of ``targets``. One pass: per chunk the catalog
        profile, the targets select kernel — its pair rows stay in the profile scratch behind the chunk's entries —
        and the rank kernel; a chunk takes records while 8 * entries + 12 * T * records fit
        :meth:`set_profile_scratch` (:func:`targets_rank_chunks`). 16 M bytes come back per record, never the n x T
        rows. Synchronous; ``stats()["kernels"]`` names ``profile``, ``targets`` and ``targets_rank``. ValueError for
        an invalid target set (first), then for M outside 1..64, raised before anything is launched and without a
        change to ``stats()``."""
        starts = _starts_of(targets, self.problem_L1)
        M = _check_rank_m(M)
        T = starts.shape[0] - 1
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = offsets.shape[0] - 1
        out = np.zeros((n, M, 4), np.int32)
        _targets_rank_check(_lib.lib().moc_engine_solve_targets_rank(self._h, _lib.ptr(codes), _lib.ptr(offsets), n,
                                                                     _lib.ptr(starts), T, M, _lib.ptr(out)))
        return out

    def solve_targets_rank_device(self, codes_t, offsets_t, h_offsets: np.ndarray, targets, M: int, out_t=None,
                                  starts_t=None, stream=None):
        """Device-resident batch (as :meth:`solve_device`) -> ``out_t``, an int32 [n, M, 4] tensor of rank rows on
        the codes' device (allocated when None; every row is written). ``starts_t`` as :meth:`solve_targets_device`.
        Queued on ``stream`` (default: the current stream); returns immediately — :func:`targets_rank_catalog_rows`
        and :meth:`report_device` can follow on the same stream. ValueError as :meth:`solve_targets_rank`."""
        import torch

        starts = _starts_of(targets, self.problem_L1)
        M = _check_rank_m(M)
        T = starts.shape[0] - 1
        h_offsets = np.ascontiguousarray(h_offsets, dtype=np.int64)
        n = h_offsets.shape[0] - 1
        assert codes_t.dtype == torch.uint8 and offsets_t.dtype == torch.int64 and offsets_t.numel() == n + 1
        if stream is None:
            stream = torch.cuda.current_stream(codes_t.device)
        if out_t is None:
            out_t = torch.empty((n, M, 4), dtype=torch.int32, device=codes_t.device)
        assert out_t.dtype == torch.int32 and out_t.is_contiguous() and tuple(out_t.shape) == (n, M, 4)
        if starts_t is not None:
            assert starts_t.dtype == torch.int64 and starts_t.is_contiguous() and starts_t.numel() == T + 1
        _targets_rank_check(_lib.lib().moc_engine_solve_targets_rank_device(
            self._h, ctypes.c_void_p(codes_t.data_ptr()), ctypes.c_void_p(offsets_t.data_ptr()), _lib.ptr(h_offsets),
            n, ctypes.c_void_p(starts_t.data_ptr()) if starts_t is not None else None, _lib.ptr(starts), T, M,
            ctypes.c_void_p(out_t.data_ptr()), ctypes.c_void_p(stream.cuda_stream)))
        return out_t

    def solve_targets_rank_wire(self, ws, targets, M: int, shift: int = 0) -> np.ndarray:
        """Host wire batch -> int32 [n, M, 4] rank rows, as :meth:`solve_targets_rank` on the decoded records.
        See :meth:`solve_profile_wire`."""
        starts = _starts_of(targets, self.problem_L1)
        M = _check_rank_m(M)
        T = starts.shape[0] - 1
        b, keep = wire_batch_of(ws, shift)
        out = np.zeros((ws.n, M, 4), np.int32)
        _targets_rank_check(_lib.lib().moc_engine_solve_targets_rank_wire(self._h, ctypes.byref(b), _lib.ptr(starts), T,
                                                                          M, _lib.ptr(out)))
        del keep
        return out

    # ---- per-target top-K and threshold hits (byte letters, dense offsets; csrc/src/hip/targets_rows_kernels.hip)
    def solve_targets_topk(self, codes: np.ndarray, offsets: np.ndarray, targets, K: int, radius: int = 0) -> np.ndarray:
        """Host CSR -> int32 [n, T, K, 3] rows as :func:`search_targets_topk_cpu` returns them, against the engine's
        Seq1 as the catalog of ``targets``. One pass: the chunks of :meth:`solve_targets` with the per-target top-K
        kernel behind each chunk's catalog profile — 12 T K bytes come back per record, never the profile.
        Synchronous; ``stats()["kernels"]`` names ``targets_topk``. ValueError for an invalid target set (first) and
        for K outside 1..64, then for the radius, raised before anything is launched and without a change to
        ``stats()``. ``radius`` > 0: the distinct placements per target (search_targets_topk_cpu's) — the segmented
        peak pass over every pair's own profile (csrc/src/hip/targets_peaks_kernels.hip) runs between each chunk's
        profile and masked per-target kernels, and ``stats()["kernels"]`` also names ``peaks`` and ``targets_peaks``;
        ``radius = 0`` is launch for launch the call without it."""
        starts = _starts_of(targets, self.problem_L1)
        K = _check_k(K)
        radius = _check_radius(radius)
        T = starts.shape[0] - 1
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = offsets.shape[0] - 1
        out = np.zeros((n, T, K, 3), np.int32)
        _targets_rows_check(_lib.lib().moc_engine_solve_targets_topk_distinct(
            self._h, _lib.ptr(codes), _lib.ptr(offsets), n, _lib.ptr(starts), T, K, radius, _lib.ptr(out)))
        return out

    def solve_targets_hits(self, codes: np.ndarray, offsets: np.ndarray, targets, min_score=None, thresholds=None,
                           within=None, max_rows: Optional[int] = None, radius: int = 0):
        """Host CSR -> ``(rows, toffsets)`` as :func:`search_targets_hits_cpu` returns them (exactly one of
        ``min_score``, ``thresholds`` — [n, T], or [n] broadcast over the targets — and ``within``, each pair's own
        best score from :meth:`solve_targets` on this engine minus D). One pass over the chunks of
        :meth:`solve_targets` with count, prefix sum over the pairs and compaction behind each chunk's catalog
        profile. Optimistic: room for ``max_rows`` rows (default n T) and exactly one more pass when more entries
        qualify (:meth:`hits_passes`). Synchronous; ``stats()["kernels"]`` names ``targets_hits``. ValueError as
        search_targets_hits_cpu, before anything is launched. ``radius`` > 0: the distinct placements per target, as
        :meth:`solve_targets_topk` (``stats()["kernels"]`` also names ``peaks`` and ``targets_peaks``)."""
        starts = _starts_of(targets, self.problem_L1)
        T = starts.shape[0] - 1
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = offsets.shape[0] - 1
        m, t, radius = _targets_hits_args(n, T, min_score, thresholds, within, radius,
                                          lambda: self.solve_targets(codes, offsets, starts))
        toffsets = np.zeros(n * T + 1, np.int64)
        _targets_rows_check(_lib.lib().moc_engine_solve_targets_hits_distinct(
            self._h, _lib.ptr(codes), _lib.ptr(offsets), n, _lib.ptr(starts), T, m, _lib.ptr(t),
            -1 if max_rows is None else int(max_rows), radius, _lib.ptr(toffsets), None, 0))
        total = int(toffsets[-1])
        rows = np.zeros((total, 3), np.int32)
        _lib.check(_lib.lib().moc_engine_hits_rows(_lib.ptr(rows) if total else None, total))
        return rows, toffsets

    def solve_targets_topk_device(self, codes_t, offsets_t, h_offsets: np.ndarray, targets, K: int, out_t=None,
                                  starts_t=None, stream=None, radius: int = 0):
        """Device-resident batch (as :meth:`solve_device`) -> ``out_t``, an int32 [n, T, K, 3] tensor of per-target
        top-K rows on the codes' device (allocated when None; every row is written). ``starts_t`` as
        :meth:`solve_targets_device`. Queued on ``stream`` (default: the current stream); returns immediately.
        ``radius`` and ValueError as :meth:`solve_targets_topk`."""
        import torch

        starts = _starts_of(targets, self.problem_L1)
        K = _check_k(K)
        radius = _check_radius(radius)
        T = starts.shape[0] - 1
        h_offsets = np.ascontiguousarray(h_offsets, dtype=np.int64)
        n = h_offsets.shape[0] - 1
        assert codes_t.dtype == torch.uint8 and offsets_t.dtype == torch.int64 and offsets_t.numel() == n + 1
        if stream is None:
            stream = torch.cuda.current_stream(codes_t.device)
        if out_t is None:
            out_t = torch.empty((n, T, K, 3), dtype=torch.int32, device=codes_t.device)
        assert out_t.dtype == torch.int32 and out_t.is_contiguous() and tuple(out_t.shape) == (n, T, K, 3)
        if starts_t is not None:
            assert starts_t.dtype == torch.int64 and starts_t.is_contiguous() and starts_t.numel() == T + 1
        _targets_rows_check(_lib.lib().moc_engine_solve_targets_topk_device_distinct(
            self._h, ctypes.c_void_p(codes_t.data_ptr()), ctypes.c_void_p(offsets_t.data_ptr()), _lib.ptr(h_offsets),
            n, ctypes.c_void_p(starts_t.data_ptr()) if starts_t is not None else None, _lib.ptr(starts), T, K, radius,
            ctypes.c_void_p(out_t.data_ptr()), ctypes.c_void_p(stream.cuda_stream)))
        return out_t

    def solve_targets_hits_device(self, codes_t, offsets_t, h_offsets: np.ndarray, targets, min_score=None,
                                  thresholds_t=None, cap: Optional[int] = None, rows_t=None, toffsets_t=None,
                                  starts_t=None, stream=None, radius: int = 0):
        """Device-resident batch (as :meth:`solve_device`) -> ``(rows_t, toffsets_t)``: ``toffsets_t`` an int64
        [n T + 1] tensor, always complete and exact; ``rows_t`` an int32 [cap, 3] tensor (``cap`` default n T) of
        which the rows with a flat index < cap are written and nothing else is touched — compare
        ``toffsets_t[-1]`` with ``cap`` after a sync. ``cap = 0`` counts only. Exactly one of ``min_score`` and
        ``thresholds_t``, an int32 [n, T] tensor on the same device — ``solve_targets_device(...)[..., 0] - D``
        (in int64, clamped to int32) queued on the same stream gives "within D of each pair's best" without a sync.
        Both result tensors are allocated when None. Queued on ``stream`` (default: the current stream); returns
        immediately. ``radius`` and ValueError as :meth:`solve_targets_hits`."""
        import torch

        starts = _starts_of(targets, self.problem_L1)
        T = starts.shape[0] - 1
        h_offsets = np.ascontiguousarray(h_offsets, dtype=np.int64)
        n = h_offsets.shape[0] - 1
        if (min_score is None) == (thresholds_t is None):
            raise ValueError("hits: give exactly one of min_score, thresholds")
        assert codes_t.dtype == torch.uint8 and offsets_t.dtype == torch.int64 and offsets_t.numel() == n + 1
        if stream is None:
            stream = torch.cuda.current_stream(codes_t.device)
        m = 0
        if min_score is not None:
            m = int(min_score)
            if not _I32.min <= m <= _I32.max:
                raise ValueError(f"hits: min_score {m} is not an int32")
        if thresholds_t is not None:
            if thresholds_t.dtype != torch.int32 or tuple(thresholds_t.shape) != (n, T):
                raise ValueError(f"hits: thresholds must be an int32 tensor of {n} x {T} entries (one per pair)")
            assert thresholds_t.is_contiguous() and thresholds_t.device == codes_t.device
        if cap is None:
            cap = max(n * T, 1) if rows_t is None else rows_t.shape[0]
        cap = int(cap)
        if cap < 0:
            raise ValueError("hits: cap must be >= 0")
        radius = _check_radius(radius)
        if rows_t is None:
            rows_t = torch.empty((cap, 3), dtype=torch.int32, device=codes_t.device)
        if toffsets_t is None:
            toffsets_t = torch.empty(n * T + 1, dtype=torch.int64, device=codes_t.device)
        assert rows_t.dtype == torch.int32 and rows_t.is_contiguous() and rows_t.dim() == 2 and rows_t.shape[1] == 3
        assert rows_t.shape[0] >= cap
        assert toffsets_t.dtype == torch.int64 and toffsets_t.is_contiguous() and toffsets_t.numel() == n * T + 1
        if starts_t is not None:
            assert starts_t.dtype == torch.int64 and starts_t.is_contiguous() and starts_t.numel() == T + 1
        _targets_rows_check(_lib.lib().moc_engine_solve_targets_hits_device_distinct(
            self._h, ctypes.c_void_p(codes_t.data_ptr()), ctypes.c_void_p(offsets_t.data_ptr()), _lib.ptr(h_offsets),
            n, ctypes.c_void_p(starts_t.data_ptr()) if starts_t is not None else None, _lib.ptr(starts), T, m,
            ctypes.c_void_p(thresholds_t.data_ptr()) if thresholds_t is not None else None, radius,
            ctypes.c_void_p(toffsets_t.data_ptr()), ctypes.c_void_p(rows_t.data_ptr()) if cap else None, cap,
            ctypes.c_void_p(stream.cuda_stream)))
        return rows_t, toffsets_t

    def solve_targets_topk_wire(self, ws, targets, K: int, shift: int = 0, radius: int = 0) -> np.ndarray:
        """Host wire batch -> int32 [n, T, K, 3] per-target top-K rows, as :meth:`solve_targets_topk` on the decoded
        records (``radius`` included). See :meth:`solve_profile_wire`."""
        starts = _starts_of(targets, self.problem_L1)
        K = _check_k(K)
        radius = _check_radius(radius)
        T = starts.shape[0] - 1
        b, keep = wire_batch_of(ws, shift)
        out = np.zeros((ws.n, T, K, 3), np.int32)
        _targets_rows_check(_lib.lib().moc_engine_solve_targets_topk_wire_distinct(
            self._h, ctypes.byref(b), _lib.ptr(starts), T, K, radius, _lib.ptr(out)))
        del keep
        return out

    def solve_targets_hits_wire(self, ws, targets, min_score=None, thresholds=None, within=None,
                                max_rows: Optional[int] = None, shift: int = 0, radius: int = 0):
        """Host wire batch -> ``(rows, toffsets)``, as :meth:`solve_targets_hits` on the decoded records (``within``
        runs :meth:`solve_targets_wire` first; ``radius`` included). See :meth:`solve_profile_wire`."""
        starts = _starts_of(targets, self.problem_L1)
        T = starts.shape[0] - 1
        n = ws.n
        m, t, radius = _targets_hits_args(n, T, min_score, thresholds, within, radius,
                                          lambda: self.solve_targets_wire(ws, starts, shift))
        b, keep = wire_batch_of(ws, shift)
        toffsets = np.zeros(n * T + 1, np.int64)
        _targets_rows_check(_lib.lib().moc_engine_solve_targets_hits_wire_distinct(
            self._h, ctypes.byref(b), _lib.ptr(starts), T, m, _lib.ptr(t), -1 if max_rows is None else int(max_rows),
            radius, _lib.ptr(toffsets), None, 0))
        del keep
        total = int(toffsets[-1])
        rows = np.zeros((total, 3), np.int32)
        _lib.check(_lib.lib().moc_engine_hits_rows(_lib.ptr(rows) if total else None, total))
        return rows, toffsets

    # ---- per-target profile summary (byte letters, dense offsets; csrc/src/hip/targets_summary_kernels.hip)
    def solve_targets_summary(self, codes: np.ndarray, offsets: np.ndarray, targets, bins: int = 0, lo: int = 0,
                              width: int = 1):
        """Host CSR -> ``(summary, hist)`` as :func:`search_targets_summary_cpu` returns them, against the engine's
        Seq1 as the catalog of ``targets``. One pass: the chunks of :meth:`solve_targets` with the per-target summary
        kernel (and, with ``bins`` > 0, the histogram kernel) behind each chunk's catalog profile — (56 + 4 ``bins``)
        T bytes come back per record, never the profile. Synchronous; ``stats()["kernels"]`` names
        ``targets_summary``. ValueError as search_targets_summary_cpu, raised before anything is launched and
        without a change to ``stats()``."""
        bins, lo, width = _summary_args(bins, lo, width)
        starts = _starts_of(targets, self.problem_L1)
        T = starts.shape[0] - 1
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = offsets.shape[0] - 1
        summary = np.zeros((n, T, len(SUMMARY_COLS)), np.int64)
        hist = np.zeros((n, T, bins), np.int32) if bins else None
        _targets_summary_check(_lib.lib().moc_engine_solve_targets_summary(
            self._h, _lib.ptr(codes), _lib.ptr(offsets), n, _lib.ptr(starts), T, bins, lo, width, _lib.ptr(summary),
            _lib.ptr(hist)))
        return summary, hist

    def targets_summary_ms(self) -> float:
        """Device time (ms) of the per-target summary and histogram launches of the last such call; 0 unless the
        engine was created with MOC_PROFILE_TIMING=1 in the environment. Waits for them."""
        ms = ctypes.c_double(0.0)
        _lib.check(_lib.lib().moc_engine_targets_summary_ms(self._h, ctypes.addressof(ms)))
        return float(ms.value)

    def solve_targets_summary_device(self, codes_t, offsets_t, h_offsets: np.ndarray, targets, bins: int = 0,
                                     lo: int = 0, width: int = 1, summary_t=None, hist_t=None, starts_t=None,
                                     stream=None):
        """Device-resident batch (as :meth:`solve_device`) -> ``(summary_t, hist_t)``: an int64 [n, T, 7] tensor and,
        with ``bins`` > 0, an int32 [n, T, bins] tensor on the codes' device (allocated when None; every element of
        both is written). With ``bins = 0`` no histogram work is launched, ``hist_t`` is returned as given and not
        touched. ``starts_t`` as :meth:`solve_targets_device`. Queued on ``stream`` (default: the current stream);
        returns immediately — :func:`targets_zscore` and :func:`targets_best` can follow on the same stream.
        ValueError as :meth:`solve_targets_summary`."""
        import torch

        bins, lo, width = _summary_args(bins, lo, width)
        starts = _starts_of(targets, self.problem_L1)
        T = starts.shape[0] - 1
        h_offsets = np.ascontiguousarray(h_offsets, dtype=np.int64)
        n = h_offsets.shape[0] - 1
        assert codes_t.dtype == torch.uint8 and offsets_t.dtype == torch.int64 and offsets_t.numel() == n + 1
        if stream is None:
            stream = torch.cuda.current_stream(codes_t.device)
        if summary_t is None:
            summary_t = torch.empty((n, T, len(SUMMARY_COLS)), dtype=torch.int64, device=codes_t.device)
        if hist_t is None and bins:
            hist_t = torch.empty((n, T, bins), dtype=torch.int32, device=codes_t.device)
        assert summary_t.dtype == torch.int64 and summary_t.is_contiguous()
        assert tuple(summary_t.shape) == (n, T, len(SUMMARY_COLS))
        if bins:
            assert hist_t.dtype == torch.int32 and hist_t.is_contiguous() and tuple(hist_t.shape) == (n, T, bins)
        if starts_t is not None:
            assert starts_t.dtype == torch.int64 and starts_t.is_contiguous() and starts_t.numel() == T + 1
        _targets_summary_check(_lib.lib().moc_engine_solve_targets_summary_device(
            self._h, ctypes.c_void_p(codes_t.data_ptr()), ctypes.c_void_p(offsets_t.data_ptr()), _lib.ptr(h_offsets),
            n, ctypes.c_void_p(starts_t.data_ptr()) if starts_t is not None else None, _lib.ptr(starts), T, bins, lo,
            width, ctypes.c_void_p(summary_t.data_ptr()), ctypes.c_void_p(hist_t.data_ptr()) if bins else None,
            ctypes.c_void_p(stream.cuda_stream)))
        return summary_t, hist_t

    def solve_targets_summary_wire(self, ws, targets, bins: int = 0, lo: int = 0, width: int = 1, shift: int = 0):
        """Host wire batch -> ``(summary, hist)``, as :meth:`solve_targets_summary` on the decoded records. See
        :meth:`solve_profile_wire`."""
        bins, lo, width = _summary_args(bins, lo, width)
        starts = _starts_of(targets, self.problem_L1)
        T = starts.shape[0] - 1
        b, keep = wire_batch_of(ws, shift)
        n = ws.n
        summary = np.zeros((n, T, len(SUMMARY_COLS)), np.int64)
        hist = np.zeros((n, T, bins), np.int32) if bins else None
        _targets_summary_check(_lib.lib().moc_engine_solve_targets_summary_wire(
            self._h, ctypes.byref(b), _lib.ptr(starts), T, bins, lo, width, _lib.ptr(summary), _lib.ptr(hist)))
        del keep
        return summary, hist

    # ---- alignment report (byte letters, dense offsets; csrc/src/hip/report_kernels.hip)
    def report(self,codes: np.ndarray, offsets: np.ndarray, rows, marks: bool = False):
        """Host CSR + result rows ([n, 3] or [n, K, 3]) -> the counts (and marker bytes) :func:`search_report_cpu`
        returns, computed by the report kernels against the engine's Seq1. Synchronous; fills ``stats()``."""
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = offsets.shape[0] - 1
        r, K, flat = _report_rows(rows, n)
        total = int(offsets[-1] - offsets[0])
        counts = np.zeros((n, K, 4), np.int32)
        m = np.zeros(max(K * total, 1), np.uint8) if marks else None
        _lib.check(_lib.lib().moc_engine_report(self._h, _lib.ptr(codes), _lib.ptr(offsets), n, K, _lib.ptr(r),
                                                _lib.ptr(counts), _lib.ptr(m)))
        counts = counts[:, 0] if flat else counts
        return (counts, m[:K * total]) if marks else counts

    def report_device(self, codes_t, offsets_t, h_offsets: np.ndarray, rows_t, counts_t=None, marks_t=None,
                      stream=None):
        """Device-resident batch (as :meth:`solve_device`) and rows ``rows_t`` (int32 [n, 3] or [n, K, 3], e.g.
        straight from :meth:`solve_device` / :meth:`solve_topk_device` on the same stream) -> ``counts_t``, an
        int32 tensor [n, 4] / [n, K, 4] (allocated when None). ``marks_t``: None for counts alone, or a uint8
        tensor of K * letters bytes that receives the marker bytes. Queued on ``stream`` (default: the current
        stream); returns immediately."""
        import torch

        h_offsets = np.ascontiguousarray(h_offsets, dtype=np.int64)
        n = h_offsets.shape[0] - 1
        assert rows_t.dtype == torch.int32 and rows_t.is_contiguous() and rows_t.shape[0] == n and rows_t.shape[-1] == 3
        assert rows_t.dim() in (2, 3)
        K = _check_k(1 if rows_t.dim() == 2 else rows_t.shape[1])
        shape = (n, 4) if rows_t.dim() == 2 else (n, K, 4)
        if counts_t is None:
            counts_t = torch.empty(shape, dtype=torch.int32, device=codes_t.device)
        assert codes_t.dtype == torch.uint8 and offsets_t.dtype == torch.int64 and offsets_t.numel() == n + 1
        assert counts_t.dtype == torch.int32 and tuple(counts_t.shape) == shape and counts_t.is_contiguous()
        if marks_t is not None:
            total = int(h_offsets[-1] - h_offsets[0])
            assert marks_t.dtype == torch.uint8 and marks_t.is_contiguous() and marks_t.numel() >= K * total
        if stream is None:
            stream = torch.cuda.current_stream(codes_t.device)
        _lib.check(_lib.lib().moc_engine_report_device(
            self._h, ctypes.c_void_p(codes_t.data_ptr()), ctypes.c_void_p(offsets_t.data_ptr()), _lib.ptr(h_offsets),
            n, K, ctypes.c_void_p(rows_t.data_ptr()), ctypes.c_void_p(counts_t.data_ptr()),
            ctypes.c_void_p(marks_t.data_ptr()) if marks_t is not None else None,
            ctypes.c_void_p(stream.cuda_stream)))
        return counts_t

    # ---- wire-format batches: a device-side decode, then the calls above (csrc/src/hip/wire_kernels.hip)
    def decode_wire_device(self, letters_t, offsets_t, lengths_t, n: int, h_offsets: np.ndarray,
                           h_lengths: Optional[np.ndarray], lengths_bits: int = 8, lengths_base: int = 0,
                           letters: str = "p33", off_shift: int = 0, stream=None):
        """Device-resident wire batch (torch tensors on this engine's GPU, as the rccl transport holds them) ->
        ``(codes_t, offsets_t, h_offsets)``: byte letters, int64 [n + 1] dense offsets and their host copy, which
        feed :meth:`solve_topk_device`, :meth:`solve_hits_device`, :meth:`solve_profile_device` and
        :meth:`report_device` on the same stream. ``letters_t``: P33 fields (``letters="p33"``), 5-bit packed
        (``"p5"``, with one readable byte after the last letter's) or ``"bytes"``; ``offsets_t``: dense, or with
        ``off_shift`` > 0 one entry per 2^off_shift records and the batch end; ``lengths_t``: narrow lengths
        (``lengths_bits`` 8 / 4 / 3 / 6 = base-6, above ``lengths_base``) or None. ``h_offsets`` / ``h_lengths``
        are host copies of those two arrays: the host expands them for planning, the device's dense offsets come
        from the decode kernel. Queued on ``stream`` (default: the current stream) with no sync. Decoded letters
        and expanded offsets are views of buffers of the engine, valid until its next decode; byte letters and dense
        offsets are the caller's own tensors. Packed letters must start at letter 0 of ``letters_t``."""
        import torch

        if letters not in _LETTER_CODES:
            raise ValueError(f"letters must be one of {tuple(_LETTER_CODES)}")
        n, off_shift = int(n), int(off_shift)
        h_offsets = np.ascontiguousarray(h_offsets, dtype=np.int64)
        entries = n + 1 if not off_shift else ((n + (1 << off_shift) - 1) >> off_shift) + 1
        assert letters_t.dtype == torch.uint8 and offsets_t.dtype == torch.int64
        assert offsets_t.numel() == entries and h_offsets.shape[0] == entries
        assert (lengths_t is None) == (h_lengths is None)
        if h_lengths is not None:
            h_lengths = np.ascontiguousarray(h_lengths, dtype=np.uint8)
            assert lengths_t.dtype == torch.uint8 and lengths_t.numel() >= h_lengths.shape[0]
        if letters != "bytes" and n >= 0 and int(h_offsets[0]) != 0:
            raise ValueError("packed letters must start at letter 0 of letters_t (decoded letters are a view from it)")
        # the kernels read what the host copies describe: the device arrays must hold that much
        c1 = int(h_offsets[-1])
        need = {"p33": (33 * ((c1 + 6) // 7) + 7) >> 3, "p5": ((5 * c1 + 7) >> 3) + 1, "bytes": c1}[letters]
        if c1 > int(h_offsets[0]) and letters_t.numel() < need:
            raise ValueError(f"letters_t holds {letters_t.numel()} bytes, the batch's letters end at byte {need}")
        if h_lengths is not None:
            bits = int(lengths_bits)
            need = (n if bits == 8 else (n + 1) // 2 if bits == 4 else 8 * ((n + 23) // 24) if bits == 6
                    else (3 * n + 7) // 8 + 1)
            if h_lengths.shape[0] < need or lengths_t.numel() < need:
                raise ValueError(f"{bits}-bit lengths of {n} records take {need} bytes")
        if stream is None:
            stream = torch.cuda.current_stream(letters_t.device)
        form = dict(n=n, len_base=int(lengths_base), packed=_LETTER_CODES[letters], off_shift=off_shift,
                    len_bits=int(lengths_bits))
        b = _lib.WireBatch(letters=letters_t.data_ptr(), offsets=offsets_t.data_ptr(),
                           lengths=lengths_t.data_ptr() if lengths_t is not None else None, device=1, **form)
        meta = _lib.WireBatch(letters=None, offsets=_addr(h_offsets), lengths=_addr(h_lengths), device=0, **form)
        out3 = np.zeros(3, np.uint64)
        dense = np.zeros(max(n, 0) + 1, np.int64)
        _lib.check(_lib.lib().moc_engine_decode_wire_device(self._h, ctypes.byref(b), ctypes.byref(meta),
                                                            ctypes.c_void_p(stream.cuda_stream), _lib.ptr(out3),
                                                            _lib.ptr(dense), None, None))
        total = int(out3[2])
        dev = letters_t.device
        if letters == "bytes":
            codes_t = letters_t
        elif total == 0:
            codes_t = torch.empty(0, dtype=torch.uint8, device=dev)
        else:
            codes_t = torch.as_tensor(_DeviceMemory(int(out3[0]), total, "|u1"), device=dev)
        dense_t = offsets_t if not off_shift else torch.as_tensor(_DeviceMemory(int(out3[1]), n + 1, "<i8"), device=dev)
        return codes_t, dense_t, dense

    def decode_wire_into(self, batch, codes_t, offsets_t, host_meta=None, shift: int = 0, stream=None) -> np.ndarray:
        """The same decode into the caller's tensors: ``codes_t`` (uint8, one element per letter of the batch) and
        ``offsets_t`` (int64 [n + 1]) on this engine's GPU; nothing outside them is written. ``batch``: a WireSlice
        (``shift`` > 0: through its sparse offsets) or a ``_lib.WireBatch`` — of host pointers (read in place when
        page-locked, else copied in packed form), or of device pointers with ``host_meta``, the ``_lib.WireBatch``
        of the host copies of its offsets and lengths. Queued on ``stream`` (default: the current stream) with no
        sync; returns the host copy of the dense offsets."""
        import torch

        b, keep = (batch, None) if isinstance(batch, _lib.WireBatch) else wire_batch_of(batch, shift)
        n = int(b.n)
        assert codes_t.dtype == torch.uint8 and codes_t.is_contiguous()
        assert offsets_t.dtype == torch.int64 and offsets_t.is_contiguous() and offsets_t.numel() == n + 1
        if stream is None:
            stream = torch.cuda.current_stream(codes_t.device)
        out3 = np.zeros(3, np.uint64)
        dense = np.zeros(max(n, 0) + 1, np.int64)
        # the letter count from the host-readable offsets, before anything is queued: the kernels fill exactly that
        sizes = np.zeros(2, np.int64)
        _lib.check(_lib.lib().moc_cpu_decode_wire(ctypes.byref(b if host_meta is None else host_meta), None, None,
                                                  _lib.ptr(sizes)))
        if codes_t.numel() != int(sizes[0]):
            raise ValueError(f"codes_t holds {codes_t.numel()} letters, the batch {int(sizes[0])}")
        _lib.check(_lib.lib().moc_engine_decode_wire_device(
            self._h, ctypes.byref(b), ctypes.byref(host_meta) if host_meta is not None else None,
            ctypes.c_void_p(stream.cuda_stream), _lib.ptr(out3), _lib.ptr(dense),
            ctypes.c_void_p(codes_t.data_ptr()), ctypes.c_void_p(offsets_t.data_ptr())))
        del keep
        return dense

    def solve_wire(self, ws, shift: int = 0) -> np.ndarray:
        """Host wire batch (a :class:`~..parallel.wire.WireSlice` with its results allocated; ``shift`` > 0: through
        its sparse offsets, as ``./final``'s GPU ranks send their slices) -> the slice's ``results`` in its format
        (``ws.triples(engine)`` decodes them). Zero-copy when every array is page-locked and the streaming kernel
        takes the batch; else the staged pipeline, P33 letters unpacked and sparse offsets expanded on the host
        first. Synchronous."""
        if ws.results is None:
            ws.alloc_results(self)
        b, keep = wire_batch_of(ws, shift)
        _lib.check(_lib.lib().moc_engine_solve_wire(self._h, ctypes.byref(b), _lib.ptr(ws.results),
                                                    _format_id(ws.fmt), int(ws.l2_min), int(ws.l2_max)))
        del keep
        return ws.results

    def solve_profile_wire(self, ws, shift: int = 0):
        """Host wire batch (a :class:`~..parallel.wire.WireSlice`; ``shift`` > 0: through its sparse offsets) ->
        ``(prof, poffsets)`` as :meth:`solve_profile` returns them for the decoded records. The packed letters,
        narrow lengths and sparse offsets are decoded on the GPU — read in place when page-locked (:meth:`pin`),
        else copied to the device in packed form. Synchronous; ``stats()["kernels"]`` names ``wire``."""
        b, keep = wire_batch_of(ws, shift)
        poffsets = np.zeros(ws.n + 1, np.int64)
        _lib.check(_lib.lib().moc_engine_solve_profile_wire(self._h, ctypes.byref(b), _lib.ptr(poffsets), None))
        prof = np.zeros(max(int(poffsets[-1]), 1), dtype=PROFILE_DTYPE)  # never a NULL pointer: NULL asks for poffsets
        _lib.check(_lib.lib().moc_engine_solve_profile_wire(self._h, ctypes.byref(b), _lib.ptr(poffsets),
                                                            _lib.ptr(prof)))
        del keep
        return prof[:int(poffsets[-1])], poffsets

    def solve_topk_wire(self, ws, K: int, shift: int = 0, radius: int = 0) -> np.ndarray:
        """Host wire batch -> int32 [n, K, 3] top-K rows, as :meth:`solve_topk` on the decoded records (same chunks
        under :meth:`set_profile_scratch`, same ``radius``). See :meth:`solve_profile_wire`."""
        K = _check_k(K)
        radius = _check_radius(radius)
        b, keep = wire_batch_of(ws, shift)
        out = np.zeros((ws.n, K, 3), np.int32)
        if radius:
            _lib.check(_lib.lib().moc_engine_solve_topk_wire_distinct(self._h, ctypes.byref(b), K, radius,
                                                                      _lib.ptr(out)))
        else:
            _lib.check(_lib.lib().moc_engine_solve_topk_wire(self._h, ctypes.byref(b), K, _lib.ptr(out)))
        del keep
        return out

    def solve_hits_wire(self, ws, min_score=None, thresholds=None, within=None, max_rows: Optional[int] = None,
                        shift: int = 0, radius: int = 0):
        """Host wire batch -> ``(rows, hoffsets)``, as :meth:`solve_hits` on the decoded records (exactly one of
        ``min_score``, ``thresholds``, ``within``; ``max_rows`` and :meth:`hits_passes` as there). ``within`` takes
        the records' best scores from :meth:`solve_topk_wire`; ``radius`` as :meth:`solve_hits`. See
        :meth:`solve_profile_wire`."""
        radius = _check_radius(radius)
        b, keep = wire_batch_of(ws, shift)
        n = ws.n
        m, t = _hits_thresholds(n, min_score, thresholds, within, lambda: self.solve_topk_wire(ws, 1, shift)[:, 0, 0])
        hoffsets = np.zeros(n + 1, np.int64)
        head = (self._h, ctypes.byref(b), m, _lib.ptr(t))
        tail = (-1 if max_rows is None else int(max_rows), _lib.ptr(hoffsets), None, 0)
        if radius:
            _lib.check(_lib.lib().moc_engine_solve_hits_wire_distinct(*head, radius, *tail))
        else:
            _lib.check(_lib.lib().moc_engine_solve_hits_wire(*head, *tail))
        total = int(hoffsets[-1])
        rows = np.zeros((total, 3), np.int32)
        _lib.check(_lib.lib().moc_engine_hits_rows(_lib.ptr(rows) if total else None, total))
        del keep
        return rows, hoffsets

    def report_wire(self, ws, rows, marks: bool = False, shift: int = 0):
        """Host wire batch + result rows ([n, 3] or [n, K, 3]) -> the counts (and marker bytes) :meth:`report` returns
        for the decoded records. See :meth:`solve_profile_wire`."""
        b, keep = wire_batch_of(ws, shift)
        n = ws.n
        r, K, flat = _report_rows(rows, n)
        total = int(ws.total)
        counts = np.zeros((n, K, 4), np.int32)
        m = np.zeros(max(K * total, 1), np.uint8) if marks else None
        _lib.check(_lib.lib().moc_engine_report_wire(self._h, ctypes.byref(b), K, _lib.ptr(r), _lib.ptr(counts),
                                                     _lib.ptr(m)))
        del keep
        counts = counts[:, 0] if flat else counts
        return (counts, m[:K * total]) if marks else counts

    def kernel_times(self) -> tuple:
        """(kernel_ms, total_ms) of the last solve: the two fields a timed loop reads, without stats()'s dict."""
        v = self._stats_buf
        _lib.check(_lib.lib().moc_engine_stats(self._h, v))
        return v[0], v[1]

    def solve_prepared(self, args: tuple):
        """Re-runs a solve whose native arguments were marshalled once (WireSlice.solve): same call."""
        _lib.check(_lib.lib().moc_engine_solve_ex(self._h, *args))

    def stats(self) -> dict:
        v = (ctypes.c_double * 14)()
        _lib.check(_lib.lib().moc_engine_stats(self._h, v))
        keys = ["kernel_ms", "total_ms", "h2d_bytes", "d2h_bytes", "chunks", "cells", "records", "direct", "format",
                "kernels"]
        d = dict(zip(keys, list(v)[:10]))
        d["r2"] = tuple(int(x) for x in list(v)[10:13])
        d["format"] = _lib.FORMAT_NAMES[int(d["format"])]
        d["kernels"] = [k for b, k in ((1, "swipe"), (2, "short"), (4, "tiles"), (8, "tile16"), (16, "profile"),
                                             (32, "report"), (64, "hits"), (128, "wire"), (256, "peaks"),
                                             (512, "summary"), (1024, "targets"),
                                             (2048, "targets_summary"), (4096, "targets_topk"),
                                             (8192, "targets_hits"), (16384, "targets_peaks"),
                                             (32768, "targets_rank"))
                        if int(d["kernels"]) & b]
        d["forms"] = [k for b, k in FORM_NAMES if int(v[13]) & b]
        return d


# Arithmetic forms of the kernels (csrc/include/moc/kernel_bounds.hpp FormBits), as stats()["forms"] names them.
FORM_NAMES = ((1, "swipe_kbits"), (2, "swipe_rk"), (4, "short_pk"), (8, "short_key32"), (16, "short_key64"),
              (32, "tile16"), (64, "tiles_key32"), (128, "tiles_key64"), (256, "mfma"), (512, "tile16_key32"),
              (1024, "tile16_i16"), (2048, "tile16_slide"))


def kernel_bounds(weights, L1: int, min_l2: int, max_l2: int) -> dict:
    """The host's exactness rules for a batch (csrc/include/moc/kernel_bounds.hpp), no GPU needed:
    ``swipe`` = "swipe_kbits" | "swipe_rk" | None (the swipe kernel's integer bounds refuse it), ``short_pk``
    = the short kernel's packed int16 form is exact, ``key_shift`` = k bits of the int32 hot keys (0: int64
    keys), ``profile16`` = the tile16 int8 profile holds the table, ``tile16_key_bits`` = index bits of tile16's
    32-bit selection keys (0: 64-bit keys), ``profile16_i16`` = the int16 tile16 profile holds the table."""
    out = np.zeros(6, np.int32)
    _lib.check(_lib.lib().moc_kernel_bounds(_lib.weights_arg(Weights.of(weights).as_list()), int(L1), int(min_l2),
                                            int(max_l2), _lib.ptr(out)))
    swipe = {1: "swipe_kbits", 2: "swipe_rk"}.get(int(out[0]))
    return {"swipe": swipe, "short_pk": bool(out[1]), "key_shift": int(out[2]), "profile16": bool(out[3]),
            "tile16_key_bits": int(out[4]), "profile16_i16": bool(out[5])}


def staged_chunks(offsets, chunk_records: int = 0, chunk_bytes: int = 0) -> np.ndarray:
    """The chunks the staged pipeline of a ``HipSearchEngine(chunk_records=, chunk_bytes=)`` cuts a batch into
    (csrc/include/moc/tile_plan.hpp staged_chunk_end), no GPU needed: int64 bounds ``0 = b0 < b1 < ... = n``, chunk c
    holding records ``[b[c], b[c + 1])``. A chunk is the longest run of at most ``chunk_records`` records and
    ``chunk_bytes`` letters, and at least one record; 0 for a size means the engine's default. ``offsets`` as
    :meth:`HipSearchEngine.solve` takes them (absolute, any first offset)."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n = offsets.shape[0] - 1
    if n < 0:
        raise ValueError("offsets needs at least one entry")
    bounds = np.zeros(n + 1, np.int64)
    chunks = int(_lib.lib().moc_staged_chunks(_lib.ptr(offsets), n, int(chunk_records), int(chunk_bytes),
                                              _lib.ptr(bounds)))
    if chunks < 0:
        raise _lib.NativeError(_lib.lib().moc_last_error().decode(errors="replace"))
    return bounds[:chunks + 1].copy()


def search_hip(problem: Problem, semantics=Semantics.REFERENCE, device: Optional[int] = None,
               engine: Optional[HipSearchEngine] = None) -> np.ndarray:
    eng = engine or HipSearchEngine(device)
    eng.set_problem(problem.weights, problem.seq1, semantics)
    return eng.solve(problem.codes, problem.offsets)


def align_search(problem: Problem, backend: str = "auto", semantics=Semantics.REFERENCE, **kw) -> np.ndarray:
    """Best (score, n, k) for every record. backend: auto | hip | cpu."""
    if backend == "auto":
        backend = "hip" if device_count() > 0 else "cpu"
    if backend == "hip":
        return search_hip(problem, semantics, **kw)
    if backend == "cpu":
        return search_cpu(problem, semantics, **kw)
    raise ValueError(f"unknown backend {backend!r}")


def align_search_device(engine: HipSearchEngine, codes_t, offsets_t, h_offsets, stream=None):
    """torch-facing op: returns an int32 [n, 3] tensor (score, n, k) on the codes' device."""
    import torch

    n = int(len(h_offsets) - 1)
    out = torch.empty((n, 3), dtype=torch.int32, device=codes_t.device)
    engine.solve_device(codes_t, offsets_t, h_offsets, out, stream)
    return out


def align_profile_device(engine: HipSearchEngine, codes_t, offsets_t, h_offsets, stream=None):
    """torch-facing op: ``(prof_t, poffsets)`` — an int32 [total, 2] tensor of per-offset (score, k) entries on
    the codes' device and the host int64 [n + 1] index into it."""
    return engine.solve_profile_device(codes_t, offsets_t, h_offsets, None, stream)


def align_topk_device(engine: HipSearchEngine, codes_t, offsets_t, h_offsets, K: int, stream=None, radius: int = 0):
    """torch-facing op: an int32 [n, K, 3] tensor of the K best (score, n, k) rows per record on the codes'
    device; ``[:, 0]`` equals :func:`align_search_device`. ``radius`` > 0: the K best distinct placements
    (:meth:`HipSearchEngine.solve_topk`)."""
    import torch

    n = int(len(h_offsets) - 1)
    out = torch.empty((n, _check_k(K), 3), dtype=torch.int32, device=codes_t.device)
    engine.solve_topk_device(codes_t, offsets_t, h_offsets, K, out, stream, radius)
    return out


def align_hits_device(engine: HipSearchEngine, codes_t, offsets_t, h_offsets, min_score=None, thresholds_t=None,
                      within=None, cap: Optional[int] = None, stream=None, radius: int = 0):
    """torch-facing op: threshold hits as ``(rows_t, hoffsets_t)`` on the codes' device — int32 [cap, 3] rows
    (score, n, k) and the int64 [n + 1] index; see :meth:`HipSearchEngine.solve_hits_device` (``radius`` > 0: the
    distinct placements among them)."""
    return engine.solve_hits_device(codes_t, offsets_t, h_offsets, min_score, thresholds_t, within, cap, None, None,
                                    stream, radius)


def align_summary_device(engine: HipSearchEngine, codes_t, offsets_t, h_offsets, bins: int = 0, lo: int = 0,
                         width: int = 1, stream=None):
    """torch-facing op: the profile summary as ``(summary_t, hist_t)`` on the codes' device — an int64 [n, 7] tensor
    (columns :data:`SUMMARY_COLS`) and an int32 [n, bins] tensor, or None with ``bins = 0``; see
    :meth:`HipSearchEngine.solve_summary_device`."""
    return engine.solve_summary_device(codes_t, offsets_t, h_offsets, bins, lo, width, None, None, stream)


def align_targets_device(engine: HipSearchEngine, codes_t, offsets_t, h_offsets, targets, stream=None):
    """torch-facing op: the multi-target rows as an int32 [n, T, 3] tensor on the codes' device; see
    :meth:`HipSearchEngine.solve_targets_device`."""
    return engine.solve_targets_device(codes_t, offsets_t, h_offsets, targets, None, None, stream)


def align_targets_rank_device(engine: HipSearchEngine, codes_t, offsets_t, h_offsets, targets, M: int, stream=None):
    """torch-facing op: each record's M best targets as an int32 [n, M, 4] tensor (columns :data:`RANK_COLS`) on the
    codes' device; see :meth:`HipSearchEngine.solve_targets_rank_device`."""
    return engine.solve_targets_rank_device(codes_t, offsets_t, h_offsets, targets, M, None, None, stream)


def align_targets_summary_device(engine: HipSearchEngine, codes_t, offsets_t, h_offsets, targets, bins: int = 0,
                                 lo: int = 0, width: int = 1, stream=None):
    """torch-facing op: ``(summary_t, hist_t)``, the per-target summary as an int64 [n, T, 7] tensor and (``bins`` > 0)
    the histograms as an int32 [n, T, bins] tensor on the codes' device; see
    :meth:`HipSearchEngine.solve_targets_summary_device`."""
    return engine.solve_targets_summary_device(codes_t, offsets_t, h_offsets, targets, bins, lo, width, None, None,
                                               None, stream)


def align_targets_topk_device(engine: HipSearchEngine, codes_t, offsets_t, h_offsets, targets, K: int, stream=None,
                              radius: int = 0):
    """torch-facing op: the per-target top-K rows as an int32 [n, T, K, 3] tensor on the codes' device (``radius`` >
    0: the distinct placements per target); see :meth:`HipSearchEngine.solve_targets_topk_device`."""
    return engine.solve_targets_topk_device(codes_t, offsets_t, h_offsets, targets, K, None, None, stream, radius)


def align_targets_hits_device(engine: HipSearchEngine, codes_t, offsets_t, h_offsets, targets, min_score=None,
                              thresholds_t=None, cap: Optional[int] = None, stream=None, radius: int = 0):
    """torch-facing op: the per-target threshold hits as ``(rows_t, toffsets_t)`` on the codes' device (``radius`` >
    0: the distinct placements per target); see :meth:`HipSearchEngine.solve_targets_hits_device`."""
    return engine.solve_targets_hits_device(codes_t, offsets_t, h_offsets, targets, min_score, thresholds_t, cap, None,
                                            None, None, stream, radius)


def align_report_device(engine: HipSearchEngine, codes_t, offsets_t, h_offsets, rows_t, marks: bool = False,
                        stream=None):
    """torch-facing op: the sign counts of device rows (int32 [n, 3] or [n, K, 3]) as an int32 [n, 4] / [n, K, 4]
    tensor on the codes' device; with ``marks`` also the uint8 marker bytes (K * letters, layout as
    :func:`search_report_cpu`): ``(counts_t, marks_t)``."""
    import torch

    marks_t = None
    if marks:
        K = 1 if rows_t.dim() == 2 else int(rows_t.shape[1])
        total = int(h_offsets[-1] - h_offsets[0])
        marks_t = torch.empty(max(K * total, 1), dtype=torch.uint8, device=codes_t.device)
    counts_t = engine.report_device(codes_t, offsets_t, h_offsets, rows_t, None, marks_t, stream)
    return (counts_t, marks_t) if marks else counts_t
