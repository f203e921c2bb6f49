"""Result formatting/writing (reference output line: main.c:204 "#%d: score: %d, n: %d, k: %d")."""
from __future__ import annotations

import sys

import numpy as np

from .. import _lib


def format_results(results: np.ndarray, first_index: int = 0) -> str:
    """Native parallel formatter (csrc/src/io.cpp). ``results`` is a RESULT_DTYPE array or (n, 3) ints."""
    from ..ops.align import as_triples

    r = np.ascontiguousarray(results)
    if r.dtype != _lib.RESULT_DTYPE:
        r = np.ascontiguousarray(as_triples(r)).view(_lib.RESULT_DTYPE).reshape(-1)
    n = r.shape[0]
    cap = 96 * n + 16
    buf = np.empty(cap, np.uint8)
    w = _lib.lib().moc_format_results(_lib.ptr(r), n, int(first_index), _lib.ptr(buf), cap)
    if w < 0:
        raise _lib.NativeError(_lib.lib().moc_last_error().decode())
    return buf[:w].tobytes().decode("ascii")


def format_results_py(results, first_index: int = 0) -> str:
    """Pure-Python formatter (oracle for the native one)."""
    out = []
    for i, (s, n, k) in enumerate(np.asarray(results, dtype=np.int64).reshape(-1, 3)):
        out.append(f"#{i + first_index}: score: {s}, n: {n}, k: {k}\n")
    return "".join(out)


def format_topk(topk, first_index: int = 0) -> str:
    """Top-K rows (int [n, K, 3] of (score, n, k), padded with (INT32_MIN, 0, 0)) as text: rank 1 of record i
    exactly as :func:`format_results` prints it, "#i: score: S, n: N, k: K"; ranks j >= 2 as
    "#i.j: score: S, n: N, k: K", real candidates only."""
    t = np.asarray(topk, dtype=np.int64)
    if t.ndim != 3 or t.shape[2] != 3:
        raise ValueError("format_topk needs an [n, K, 3] array")
    none = np.iinfo(np.int32).min
    out = []
    for i, rows in enumerate(t):
        s, n, k = rows[0]
        out.append(f"#{i + first_index}: score: {s}, n: {n}, k: {k}\n")
        for j, (s, n, k) in enumerate(rows[1:], start=2):
            if s != none:
                out.append(f"#{i + first_index}.{j}: score: {s}, n: {n}, k: {k}\n")
    return "".join(out)


def format_hits(results, rows, hoffsets, first_index: int = 0) -> str:
    """Results with their threshold hits: record i's line as :func:`format_results` prints it, then one line per
    hit (``rows[hoffsets[i]:hoffsets[i + 1]]`` from the hits calls), indented by two spaces:
    "  hit: score: S, n: N, k: K"."""
    from ..ops.align import as_triples

    res = np.asarray(as_triples(results), dtype=np.int64)
    r = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    h = np.asarray(hoffsets, dtype=np.int64).reshape(-1)
    if h.shape[0] != res.shape[0] + 1 or (h.size and (h[0] != 0 or h[-1] != r.shape[0])) or np.any(np.diff(h) < 0):
        raise ValueError("format_hits needs hoffsets [n + 1] that index the rows of the results' n records")
    out = []
    for i, (s, n, k) in enumerate(res):
        out.append(f"#{i + first_index}: score: {s}, n: {n}, k: {k}\n")
        for hs, hn, hk in r[h[i]:h[i + 1]]:
            out.append(f"  hit: score: {hs}, n: {hn}, k: {hk}\n")
    return "".join(out)


def format_summary(summary, hist=None, first_index: int = 0) -> str:
    """Results with their profile summary (int64 [n, 7] rows of ops.align.SUMMARY_COLS from the summary calls):
    record i's line as :func:`format_results` prints it — its (score, n, k) are the summary's (max, n, k) — then
    "  summary: offsets: C, min: A, max: B, mean: M, sd: S, z: Z": mean and population sd over the whole profile to
    3 decimals, z = ops.align.summary_zscore to 2 decimals, each ``nan`` where it is not defined (no offsets; for z
    fewer than 3, or an all-equal rest). With ``hist`` (int [n, B]) one more line "  hist: c0 c1 ...". The moments
    are divided in exact Python integers."""
    import math

    from ..ops.align import SUMMARY_COLS, summary_zscore

    s = np.asarray(summary, dtype=np.int64)
    if s.ndim != 2 or s.shape[1] != len(SUMMARY_COLS):
        raise ValueError(f"format_summary needs an [n, {len(SUMMARY_COLS)}] summary")
    h = None if hist is None else np.asarray(hist, dtype=np.int64)
    if h is not None and (h.ndim != 2 or h.shape[0] != s.shape[0]):
        raise ValueError("format_summary needs a histogram of the summary's n records, [n, B]")
    z = summary_zscore(s)
    out = []
    for i, (c, tot, sq, mn, mx, n, k) in enumerate(s.tolist()):
        out.append(f"#{i + first_index}: score: {mx}, n: {n}, k: {k}\n")
        if c > 0:
            mean = f"{tot / c:.3f}"
            sd = f"{math.sqrt(max(c * sq - tot * tot, 0) / (c * c)):.3f}"
        else:
            mean = sd = "nan"
        zs = "nan" if math.isnan(z[i]) else f"{z[i]:.2f}"
        out.append(f"  summary: offsets: {c}, min: {mn}, max: {mx}, mean: {mean}, sd: {sd}, z: {zs}\n")
        if h is not None:
            out.append("  hist: " + " ".join(str(v) for v in h[i].tolist()) + "\n")
    return "".join(out)


def format_targets(results, rows, first_index: int = 0) -> str:
    """Results with their multi-target rows (int32 [n, T, 3] from the targets calls): record i's line as
    :func:`format_results` prints it, then one line per target, numbered from 1 — "  target t: score: S, n: N, k: K"
    with n relative to that target's start, or "  target t: none" where the record is longer than the target — and
    a final "  best: t" (ops.align.targets_best: the highest score, then the first target; "  best: none" when no
    target fits)."""
    from ..ops.align import as_triples, targets_best

    r = np.asarray(rows, dtype=np.int32)
    res = as_triples(results)
    if r.ndim != 3 or r.shape[2] != 3 or r.shape[0] != res.shape[0]:
        raise ValueError("format_targets needs [n, T, 3] rows for the results' n records")
    best, _ = targets_best(r)
    none = np.iinfo(np.int32).min
    out = []
    for i, (score, n, k) in enumerate(res.tolist()):
        out.append(f"#{i + first_index}: score: {score}, n: {n}, k: {k}\n")
        for t, (ts, tn, tk) in enumerate(r[i].tolist()):
            out.append(f"  target {t + 1}: none\n" if ts == none else f"  target {t + 1}: score: {ts}, n: {tn}, k: {tk}\n")
        out.append(f"  best: {int(best[i]) + 1}\n" if best[i] >= 0 else "  best: none\n")
    return "".join(out)


def format_targets_rank(results, rank, first_index: int = 0) -> str:
    """Results with their target ranking (int32 [n, M, 4] rows of ops.align.RANK_COLS from the rank calls): record i's
    line as :func:`format_results` prints it, then "  best j: target t: score: S, n: N, k: K" for its j-th best
    target, j = 1 .. min(M, fitting targets), targets numbered from 1 and n relative to that target's start — or
    "  best: none" when no target fits the record. No per-target lines."""
    from ..ops.align import as_triples

    r = np.asarray(rank, dtype=np.int32)
    res = as_triples(results)
    if r.ndim != 3 or r.shape[2] != 4 or r.shape[1] < 1 or r.shape[0] != res.shape[0]:
        raise ValueError("format_targets_rank needs [n, M, 4] rank rows for the results' n records")
    out = []
    for i, (score, n, k) in enumerate(res.tolist()):
        out.append(f"#{i + first_index}: score: {score}, n: {n}, k: {k}\n")
        listed = [row for row in r[i].tolist() if row[0] >= 0]
        for j, (t, ts, tn, tk) in enumerate(listed, start=1):
            out.append(f"  best {j}: target {t + 1}: score: {ts}, n: {tn}, k: {tk}\n")
        if not listed:
            out.append("  best: none\n")
    return "".join(out)


def _format_targets_under(results, rows, under, first_index: int) -> str:
    """:func:`format_targets` with the lines ``under(i, t)`` yields below each "  target t: ..." line."""
    from ..ops.align import as_triples, targets_best

    res = as_triples(results)
    best, _ = targets_best(rows)
    none = np.iinfo(np.int32).min
    out = []
    for i, (score, n, k) in enumerate(res.tolist()):
        out.append(f"#{i + first_index}: score: {score}, n: {n}, k: {k}\n")
        for t, (ts, tn, tk) in enumerate(rows[i].tolist()):
            out.append(f"  target {t + 1}: none\n" if ts == none else f"  target {t + 1}: score: {ts}, n: {tn}, k: {tk}\n")
            out.extend(under(i, t))
        out.append(f"  best: {int(best[i]) + 1}\n" if best[i] >= 0 else "  best: none\n")
    return "".join(out)


def format_targets_topk(results, topk, first_index: int = 0) -> str:
    """:func:`format_targets` with every target's top-K rows (int32 [n, T, K, 3] from the per-target top-K calls; rank
    1 is the multi-target row): under each "  target t: ..." line one line per rank j >= 2,
    "    top j: score: S, n: N, k: K", real candidates only."""
    from ..ops.align import as_triples

    r = np.asarray(topk, dtype=np.int32)
    if r.ndim != 4 or r.shape[3] != 3 or r.shape[2] < 1 or r.shape[1] < 1 or r.shape[0] != as_triples(results).shape[0]:
        raise ValueError("format_targets_topk needs [n, T, K, 3] rows for the results' n records")
    none = np.iinfo(np.int32).min

    def under(i, t):
        return [f"    top {j}: score: {s}, n: {n}, k: {k}\n" for j, (s, n, k) in enumerate(r[i, t, 1:].tolist(), start=2)
                if s != none]

    return _format_targets_under(results, np.ascontiguousarray(r[:, :, 0]), under, first_index)


def format_targets_hits(results, rows, hits, toffsets, first_index: int = 0) -> str:
    """:func:`format_targets` (``rows``: the multi-target rows, int32 [n, T, 3]) with every target's threshold hits
    (``hits[toffsets[i * T + t]:toffsets[i * T + t + 1]]`` from the per-target hits calls): under each
    "  target t: ..." line one line per hit, "    hit: score: S, n: N, k: K", n relative to the target's start."""
    from ..ops.align import as_triples

    r = np.asarray(rows, dtype=np.int32)
    if r.ndim != 3 or r.shape[2] != 3 or r.shape[1] < 1 or r.shape[0] != as_triples(results).shape[0]:
        raise ValueError("format_targets_hits needs [n, T, 3] rows for the results' n records")
    h = np.asarray(hits, dtype=np.int64).reshape(-1, 3)
    o = np.asarray(toffsets, dtype=np.int64).reshape(-1)
    T = r.shape[1]
    if o.shape[0] != r.shape[0] * T + 1 or o[0] != 0 or o[-1] != h.shape[0] or np.any(np.diff(o) < 0):
        raise ValueError("format_targets_hits needs toffsets [n * T + 1] that index the hits of the rows' pairs")

    def under(i, t):
        p = i * T + t
        return [f"    hit: score: {s}, n: {n}, k: {k}\n" for s, n, k in h[o[p]:o[p + 1]].tolist()]

    return _format_targets_under(results, r, under, first_index)


def format_targets_summary(summary, hist=None, first_index: int = 0) -> str:
    """:func:`format_targets` with every target's profile summary (int64 [n, T, 7] from the per-target summary calls;
    its (max, n, k) are the multi-target rows, and record i's own line is target 1's row): under each
    "  target t: ..." line "    summary: offsets: C, min: A, max: B, mean: M, sd: S, z: Z" in :func:`format_summary`'s
    number formats and, with ``hist`` (int [n, T, B]), "    hist: c0 c1 ..."; after "  best: t" one more line
    "  best by z: t" — ops.align.targets_best ranked by ops.align.targets_zscore — or "  best by z: none"."""
    import math

    from ..ops.align import SUMMARY_COLS, targets_best, targets_zscore

    s = np.asarray(summary, dtype=np.int64)
    if s.ndim != 3 or s.shape[2] != len(SUMMARY_COLS) or s.shape[1] < 1:
        raise ValueError(f"format_targets_summary needs an [n, T, {len(SUMMARY_COLS)}] summary")
    h = None if hist is None else np.asarray(hist, dtype=np.int64)
    if h is not None and (h.ndim != 3 or h.shape[:2] != s.shape[:2]):
        raise ValueError("format_targets_summary needs a histogram of the summary's pairs, [n, T, B]")
    none = np.iinfo(np.int32).min
    rows = np.ascontiguousarray(s[:, :, 4:7]).astype(np.int32)
    z = targets_zscore(s)
    best, _ = targets_best(rows)
    best_z, _ = targets_best(rows, z)
    out = []
    for i in range(s.shape[0]):
        score, n, k = rows[i, 0].tolist()
        out.append(f"#{i + first_index}: score: {score}, n: {n}, k: {k}\n")
        for t, (c, tot, sq, mn, mx, tn, tk) in enumerate(s[i].tolist()):
            out.append(f"  target {t + 1}: none\n" if mx == none else f"  target {t + 1}: score: {mx}, n: {tn}, k: {tk}\n")
            if c > 0:
                mean = f"{tot / c:.3f}"
                sd = f"{math.sqrt(max(c * sq - tot * tot, 0) / (c * c)):.3f}"
            else:
                mean = sd = "nan"
            zs = "nan" if math.isnan(z[i, t]) else f"{z[i, t]:.2f}"
            out.append(f"    summary: offsets: {c}, min: {mn}, max: {mx}, mean: {mean}, sd: {sd}, z: {zs}\n")
            if h is not None:
                out.append("    hist: " + " ".join(str(v) for v in h[i, t].tolist()) + "\n")
        out.append(f"  best: {int(best[i]) + 1}\n" if best[i] >= 0 else "  best: none\n")
        out.append(f"  best by z: {int(best_z[i]) + 1}\n" if best_z[i] >= 0 else "  best by z: none\n")
    return "".join(out)


def format_report(problem, rows, counts, marks, first_index: int = 0) -> str:
    """Results with their alignments. ``rows`` [n, 3] print as :func:`format_results` does and [n, K, 3] as
    :func:`format_topk` does; after the line of every real row — not an empty one (score INT32_MIN), nor one
    whose counts are -1 — come four lines, indented by two spaces: the counts (``counts``: [n, 4] / [n, K, 4]
    from the report calls), Seq1[n .. n + L2 + (k > 0)), the marker line (``marks``: the report calls' marker
    bytes) with '-' at position k when k > 0, and the record with '-' after its k-th letter."""
    from ..models.scoring import decode

    t = np.asarray(rows)
    if t.dtype == _lib.RESULT_DTYPE:
        t = np.ascontiguousarray(t).view(np.int32).reshape(t.shape + (3,))
    t = t.astype(np.int64)
    flat = t.ndim == 2
    if flat:
        t = t[:, None, :]
    if t.ndim != 3 or t.shape[2] != 3 or t.shape[0] != problem.n:
        raise ValueError("format_report needs [n, 3] or [n, K, 3] rows of the problem's records")
    n, K = t.shape[0], t.shape[1]
    c = np.asarray(counts, dtype=np.int64).reshape(n, K, 4)
    m = np.asarray(marks, dtype=np.uint8).reshape(-1)
    seq1 = decode(problem.seq1)
    offsets = np.asarray(problem.offsets, dtype=np.int64)
    none = np.iinfo(np.int32).min
    out = []
    for i in range(n):
        seq2 = decode(problem.codes[offsets[i]:offsets[i + 1]])
        L2 = len(seq2)
        for j in range(K):
            s, o, k = (int(v) for v in t[i, j])
            if j == 0:
                out.append(f"#{i + first_index}: score: {s}, n: {o}, k: {k}\n")
            elif s != none:
                out.append(f"#{i + first_index}.{j + 1}: score: {s}, n: {o}, k: {k}\n")
            if s == none or c[i, j, 0] < 0:
                continue
            at = K * int(offsets[i] - offsets[0]) + j * L2
            line = m[at:at + L2].tobytes().decode("ascii")
            if k > 0:
                line = line[:k] + "-" + line[k:]
            out.append(f"  $: {c[i, j, 0]}, %: {c[i, j, 1]}, #: {c[i, j, 2]}, space: {c[i, j, 3]}\n")
            out.append(f"  {seq1[o:o + L2 + (1 if k > 0 else 0)]}\n")
            out.append(f"  {line}\n")
            out.append(f"  {seq2[:k] + '-' + seq2[k:] if k > 0 else seq2}\n")
    return "".join(out)


def write_results(results: np.ndarray, stream=None, first_index: int = 0):
    stream = stream or sys.stdout
    stream.write(format_results(results, first_index))
    stream.flush()
