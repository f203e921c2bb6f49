"""Profile summary on the CPU engine (csrc/src/cpu_engine.cpp summary_batch_cpu): against numpy over the
letter-by-letter Python replay (models/reference.brute_force_profile) and over search_profile_cpu, the invariants that
tie it to the search, the histogram against Python-int floor division, argument checking, the exactness bound at its
edge, the host helpers summary_zscore / summary_thresholds against rational arithmetic, format_summary, the Python
CLI (--summary / --hist, one and two gloo ranks) and the stand-alone sanitizer program.

The replay costs O(L1 * L2^2) Python steps per record, so it anchors the random small problems and the goldens it
can finish (inputs 1, 2, 5, 6); every golden is compared with numpy over search_profile_cpu, which
tests/test_profile_cpu.py pins to the same replay."""
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT, expected, input_path
from test_dist import torchrun

from mpi_openmp_cuda_amd import (SUMMARY_COLS, Problem, Semantics, format_results, format_summary, make_synthetic,
                                 search_cpu, search_profile_cpu, search_summary_cpu, summary_thresholds,
                                 summary_zscore)
from mpi_openmp_cuda_amd.models.reference import brute_force_profile
from mpi_openmp_cuda_amd.models.scoring import score_table
from mpi_openmp_cuda_amd.ops.align import (SUMMARY_MAX_BINS, as_triples, profile_offsets, summary_bound,
                                           summary_geometry)

SEMS = [Semantics.REFERENCE, Semantics.SPEC]
I32 = np.iinfo(np.int32)
EMPTY_ROW = [0, 0, 0, I32.max, I32.min, 0, 0]


def problem_of(weights, seq1, recs) -> Problem:
    lens = np.array([len(r) for r in recs], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    codes = np.concatenate([np.asarray(r, np.uint8) for r in recs]) if len(recs) else np.zeros(0, np.uint8)
    return Problem(list(weights), np.asarray(seq1, np.uint8), codes, offsets)


def row_of(entries):
    """The summary row of a list of (score, k) in Python integers."""
    if not entries:
        return list(EMPTY_ROW)
    scores = [int(s) for s, _ in entries]
    mx = max(scores)
    n = scores.index(mx)  # the smallest offset among ties
    return [len(scores), sum(scores), sum(s * s for s in scores), min(scores), mx, n, int(entries[n][1])]


def bin_of(s, lo, width, bins):
    """Python-int floor division, then the clip."""
    return min(max((int(s) - int(lo)) // int(width), 0), bins - 1)


def hist_of(scores, lo, width, bins):
    h = [0] * bins
    for s in scores:
        h[bin_of(s, lo, width, bins)] += 1
    return h


def rows_of_profile(prof, po):
    return [row_of(list(zip(prof["score"][a:b].tolist(), prof["k"][a:b].tolist()))) for a, b in zip(po[:-1], po[1:])]


def test_constants():
    assert SUMMARY_COLS == ("count", "sum", "sumsq", "min", "max", "n", "k")
    g = summary_geometry()
    assert len(g) == 3 and g[0] >= 1 and g[1] == 64 * g[0] and g[2] == SUMMARY_MAX_BINS == 256


# ---- against the replay ----------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_random_small_problems_match_letter_replay(sem):
    rng = np.random.default_rng(50)
    checked = negatives = 0
    for trial in range(60):
        weights = ((1, 5, 5, 5), (10, 2, 3, 4), (0, 0, 0, 0), (3, 0, 7, 1))[trial % 4]
        L1 = int(rng.integers(1, 41))
        seq1 = rng.integers(1, 27, L1)
        lens = [1, min(2, L1), L1, L1 + 1] + [int(rng.integers(1, min(L1, 12) + 1)) for _ in range(3)]
        recs = [rng.integers(1, 4 if trial % 3 == 0 else 27, l) for l in lens]  # small alphabets make ties
        prob = problem_of(weights, seq1, recs)
        t = score_table(prob.weights)
        bins, lo, width = int(rng.integers(1, 9)), int(rng.integers(-30, 10)), int(rng.integers(1, 12))
        summary, hist = search_summary_cpu(prob, bins, lo, width, semantics=sem)
        assert summary.dtype == np.int64 and summary.shape == (prob.n, 7)
        assert hist.dtype == np.int32 and hist.shape == (prob.n, bins)
        for i, r in enumerate(recs):
            replay = brute_force_profile(t, prob.seq1, r, sem)
            assert summary[i].tolist() == row_of(replay), (trial, i, sem)
            assert hist[i].tolist() == hist_of([s for s, _ in replay], lo, width, bins), (trial, i, sem)
            checked += 1
            negatives += 1 if summary[i, 3] < 0 else 0
    assert checked >= 400 and negatives > 50  # weights (1, 5, 5, 5) give negative scores


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("i", [1, 2, 5, 6])
def test_goldens_match_letter_replay(i, sem):
    prob = Problem.read(input_path(i))
    t = score_table(prob.weights)
    summary, hist = search_summary_cpu(prob, 16, -100, 25, semantics=sem)
    for j in range(prob.n):
        replay = brute_force_profile(t, prob.seq1, prob.codes[prob.offsets[j]:prob.offsets[j + 1]], sem)
        assert summary[j].tolist() == row_of(replay)
        assert hist[j].tolist() == hist_of([s for s, _ in replay], -100, 25, 16)


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("i", range(1, 7))
def test_goldens_match_numpy_over_the_profile(i, sem):
    prob = Problem.read(input_path(i))
    prof, po = search_profile_cpu(prob, sem)
    summary, hist = search_summary_cpu(prob, 32, -2000, 150, semantics=sem)
    assert summary.tolist() == rows_of_profile(prof, po)
    sc = prof["score"].astype(np.int64)
    for j in range(prob.n):
        want = np.bincount(np.clip((sc[po[j]:po[j + 1]] + 2000) // 150, 0, 31), minlength=32)
        assert np.array_equal(hist[j], want)
    # threads do not change anything
    s1, h1 = search_summary_cpu(prob, 32, -2000, 150, semantics=sem, threads=1)
    assert np.array_equal(s1, summary) and np.array_equal(h1, hist)
    if sem == Semantics.REFERENCE:
        assert format_results(summary[:, 4:7].astype(np.int32)) == expected(i)


# ---- search invariant ------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("shape,n", [("input6", 1000), ("input1", 200), ("input3", 6), ("input4", 40)])
def test_search_invariant(shape, n, sem):
    prob = make_synthetic(shape, n, seed=3)
    summary, hist = search_summary_cpu(prob, 7, 0, 13, semantics=sem)
    assert np.array_equal(summary[:, 4:7], as_triples(search_cpu(prob, sem)))
    assert np.array_equal(summary[:, 0], np.diff(profile_offsets(prob.L1, prob.lengths, sem)))
    assert np.array_equal(hist.sum(axis=1), summary[:, 0])
    none, _ = search_summary_cpu(prob, semantics=sem)
    assert _ is None and np.array_equal(none, summary)


def test_records_without_offsets_and_empty_batch():
    prob = problem_of((10, 2, 3, 4), np.arange(1, 9), [np.arange(1, 10), np.arange(1, 9), np.arange(1, 3)])
    summary, hist = search_summary_cpu(prob, 3, 0, 5)
    assert summary[0].tolist() == EMPTY_ROW and hist[0].tolist() == [0, 0, 0]
    assert summary[1, 0] == 1 and hist[1].sum() == 1  # L2 == L1: one offset
    empty = problem_of((10, 2, 3, 4), np.arange(1, 9), [])
    summary, hist = search_summary_cpu(empty, 4, 0, 1)
    assert summary.shape == (0, 7) and hist.shape == (0, 4)
    assert search_summary_cpu(empty)[1] is None


# ---- histogram against an independent definition ---------------------------------------------------------
def hist_grid(scores):
    """The B / width / lo grid of the issue for a profile with these scores."""
    lo_s, hi_s = int(min(scores)), int(max(scores))
    los = [I32.min, lo_s - 1000, hi_s + 1000, (lo_s + hi_s) // 2, min(lo_s + 3, -1), I32.max]
    return [(b, lo, w) for b in (1, 2, 255, 256) for w in (1, 7, 2 ** 31 - 1) for lo in los]


def negative_score_problem(L1=300, L2=20, seed=9):
    """One record whose profile has negative and positive scores (weights (1, 5, 5, 5); a planted copy scores L2)."""
    rng = np.random.default_rng(seed)
    seq1 = rng.integers(1, 27, L1)
    rec = seq1[100:100 + L2].copy()
    return problem_of((1, 5, 5, 5), seq1, [rec])


def test_histogram_grid_against_python_floor_division():
    prob = negative_score_problem()
    prof, po = search_profile_cpu(prob)
    scores = prof["score"].tolist()
    assert min(scores) < 0 < max(scores)
    for bins, lo, width in hist_grid(scores):
        summary, hist = search_summary_cpu(prob, bins, lo, width)
        assert hist[0].tolist() == hist_of(scores, lo, width, bins), (bins, lo, width)
        assert hist[0].sum() == summary[0, 0] == len(scores)
    # the edges by hand: below lo -> bin 0, at or past lo + B * width -> the last bin, negative numerators round down
    assert bin_of(-8, -1, 7, 4) == 0 and bin_of(-1, -8, 7, 4) == 1 and bin_of(I32.max, I32.min, 1, 256) == 255
    assert bin_of(I32.max, I32.min, 2 ** 31 - 1, 256) == 2


# ---- argument errors -------------------------------------------------------------------------------------
def test_argument_errors():
    prob = make_synthetic("input6", 8)
    for kw in ({"bins": -1}, {"bins": 257}, {"bins": 4, "width": 0}, {"width": 0}, {"bins": 4, "width": -3},
               {"bins": 4, "lo": 2 ** 31}, {"bins": 4, "width": 2 ** 31}):
        with pytest.raises(ValueError, match="summary"):
            search_summary_cpu(prob, **kw)


# ---- exactness bound -------------------------------------------------------------------------------------
def wide_problem(C, sem):
    """Weights (10^6, 3, 2, 1) and one 500-letter record that matches Seq1 at every offset: every score is 5 * 10^8 =
    M, so M^2 = 2.5e17 and the sum of squares is C * M^2 exactly. L1 gives the record C offsets under ``sem``."""
    L2 = 500
    L1 = L2 + C - (1 if sem == Semantics.SPEC else 0)
    return problem_of((1_000_000, 3, 2, 1), np.full(L1, 1), [np.full(L2, 1)])


@pytest.mark.parametrize("sem", SEMS)
def test_exactness_bound_edge(sem):
    M = 500 * 1_000_000
    assert summary_bound(1_000_000, 500) == 36 == (2 ** 63 - 1) // (M * M)
    assert 36 * M * M < 2 ** 63 < 37 * M * M
    summary, _ = search_summary_cpu(wide_problem(36, sem), semantics=sem)
    assert summary[0].tolist() == [36, 36 * M, 36 * M * M, M, M, 0, 0]
    assert summary[0, 2] > 2 ** 62
    with pytest.raises(ValueError, match="exactness bound"):
        search_summary_cpu(wide_problem(37, sem), semantics=sem)
    # realistic shapes are far inside: weights 10, L2 = 2000, C = 150000 -> 6e13
    assert summary_bound(10, 2000) > 150_000 and 150_000 * (10 * 2000) ** 2 == 6 * 10 ** 13
    assert summary_bound(2 ** 31 - 1, 2 ** 40) == 1  # M capped at 2^31


# ---- derived values --------------------------------------------------------------------------------------
def z_reference(row):
    """(z, mean', sd') of a summary row in rational arithmetic; z is None where it is not defined."""
    c, tot, sq, _, mx = (int(v) for v in row[:5])
    if c < 3:
        return None, None, None
    mean = Fraction(tot - mx, c - 1)
    var = Fraction(sq - mx * mx, c - 1) - mean * mean
    if var <= 0:
        return None, mean, 0.0
    # sqrt of a rational through integers: sqrt(p / q) = sqrt(p * q) / q, math.sqrt of an int rounds once
    sd = math.sqrt(var.numerator * var.denominator) / var.denominator
    return float((mx - mean) / Fraction(sd)), mean, sd


def test_zscore_against_fractions():
    rows = []
    for shape, n in (("input6", 300), ("input1", 100), ("input4", 20)):
        rows.append(search_summary_cpu(make_synthetic(shape, n, seed=8))[0])
    rows.append(search_summary_cpu(negative_score_problem())[0])
    rows.append(search_summary_cpu(wide_problem(36, Semantics.REFERENCE))[0])  # all equal, near 2^63
    rows.append(np.array([[3, 6 * 10 ** 8 + 1, 12 * 10 ** 16 + 4 * 10 ** 8 + 1, 2 * 10 ** 8, 2 * 10 ** 8 + 1, 0, 0],
                          [4, 10, 30, 1, 4, 3, 0], [3, 0, 2, -1, 1, 0, 0]], np.int64))
    summary = np.concatenate(rows)
    z = summary_zscore(summary)
    assert z.dtype == np.float64 and z.shape == (len(summary),)
    defined = 0
    for row, got in zip(summary, z):
        want, _, _ = z_reference(row)
        if want is None:
            assert math.isnan(got), row
        else:
            assert abs(got - want) <= 1e-12 * abs(want), (row, got, want)
            defined += 1
    assert defined > 300


def test_zscore_nan_cases():
    # C = 0, 1, 2, and an all-equal profile (also: all equal but the best, whose rest has no spread)
    s = np.array([EMPTY_ROW, [1, 5, 25, 5, 5, 0, 0], [2, 7, 29, 2, 5, 1, 0], [5, 35, 245, 7, 7, 0, 0],
                  [4, 19, 127, 3, 10, 3, 0], [3, 12, 56, 2, 6, 0, 0]], np.int64)
    z = summary_zscore(s)
    assert np.isnan(z[:5]).all() and z[5] == pytest.approx((6 - 3) / 1.0)
    t = summary_thresholds(s, 2.0)
    assert t.dtype == np.int32 and t[:5].tolist() == [I32.max] * 5 and t[5] == 5  # mean' 3, sd' 1
    # an all-one-letter Seq1 and record: every score equal
    prob = problem_of((10, 2, 3, 4), np.full(30, 3), [np.full(8, 3)])
    assert np.isnan(summary_zscore(search_summary_cpu(prob)[0])).all()


def test_thresholds_against_fractions_and_torch():
    import torch

    summary = np.concatenate([search_summary_cpu(make_synthetic(shape, n, seed=11))[0]
                              for shape, n in (("input6", 300), ("input1", 100), ("input4", 20))]
                             + [search_summary_cpu(negative_score_problem())[0], np.array([EMPTY_ROW], np.int64)])
    for zv in (0.0, 2.5, 4.0, -1.0, 1e12):
        got = summary_thresholds(summary, zv)
        assert got.dtype == np.int32 and got.shape == (len(summary),)
        for row, g in zip(summary, got):
            zr, mean, sd = z_reference(row)
            if zr is None:
                assert g == I32.max
                continue
            exact = float(mean) + zv * sd
            want = min(max(math.ceil(exact), I32.min), I32.max)
            assert abs(int(g) - want) <= 1, (row, zv, g, want)
        via_torch = summary_thresholds(torch.from_numpy(summary), zv)
        assert via_torch.dtype == torch.int32 and via_torch.device.type == "cpu"
        assert np.array_equal(via_torch.numpy(), got)


def test_planted_record_stands_out():
    """The README's case: a 40-letter piece of Seq1 placed again elsewhere in a random 300-letter Seq1 scores far
    above the rest of its profile; a random record of the same length does not."""
    rng = np.random.default_rng(12)
    seq1 = rng.integers(1, 27, 300)
    piece = seq1[30:70].copy()
    seq1[200:240] = piece  # placed twice
    prob = problem_of((10, 2, 3, 4), seq1, [piece, rng.integers(1, 27, 40)])
    summary, _ = search_summary_cpu(prob)
    z = summary_zscore(summary)
    assert summary[0, 4] == 400 and summary[0, 5] == 30  # the first placement wins the tie
    assert z[0] > z[1] and z[0] > 4


# ---- format_summary --------------------------------------------------------------------------------------
def test_format_summary():
    s = np.array([[4, 10, 30, 1, 4, 3, 2], EMPTY_ROW, [1, -5, 25, -5, -5, 0, 0]], np.int64)
    text = format_summary(s, first_index=7)
    assert text == ("#7: score: 4, n: 3, k: 2\n"
                    "  summary: offsets: 4, min: 1, max: 4, mean: 2.500, sd: 1.118, z: 2.45\n"
                    f"#8: score: {I32.min}, n: 0, k: 0\n"
                    f"  summary: offsets: 0, min: {I32.max}, max: {I32.min}, mean: nan, sd: nan, z: nan\n"
                    "#9: score: -5, n: 0, k: 0\n"
                    "  summary: offsets: 1, min: -5, max: -5, mean: -5.000, sd: 0.000, z: nan\n")
    with_hist = format_summary(s, np.array([[1, 3], [0, 0], [1, 0]]))
    assert with_hist.splitlines()[2] == "  hist: 1 3" and len(with_hist.splitlines()) == 9
    assert [l for l in with_hist.splitlines() if not l.startswith("  ")] == \
        format_results(s[:, 4:7].astype(np.int32)).splitlines()
    with pytest.raises(ValueError):
        format_summary(s[:, :6])
    with pytest.raises(ValueError):
        format_summary(s, np.zeros((2, 2)))


# ---- the Python CLI ----------------------------------------------------------------------------------------
def _cli(args, i):
    with open(input_path(i), "rb") as f:
        return subprocess.run([sys.executable, "-m", "mpi_openmp_cuda_amd", "--backend=cpu"] + args, stdin=f,
                              capture_output=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd="/tmp", timeout=120)


@pytest.mark.parametrize("i", [1, 3])
@pytest.mark.parametrize("hist", [None, "-500:100:12"])
def test_cli_summary(i, hist):
    prob = Problem.read(input_path(i))
    r = _cli(["--summary"] + ([f"--hist={hist}"] if hist else []), i)  # the = form: LO is negative
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    out = r.stdout.decode()
    want = format_summary(*search_summary_cpu(prob, *((12, -500, 100) if hist else ())))
    assert out == want
    assert "".join(l + "\n" for l in out.splitlines() if not l.startswith("  ")) == expected(i)  # byte-identical
    assert sum(l.startswith("  summary: ") for l in out.splitlines()) == prob.n
    assert sum(l.startswith("  hist: ") for l in out.splitlines()) == (prob.n if hist else 0)


def test_cli_without_the_flags_is_todays_output():
    r = _cli([], 1)
    assert r.returncode == 0 and r.stdout.decode() == expected(1)


@pytest.mark.parametrize("args", [["--summary", "--top", "2"], ["--summary", "--show-alignment"],
                                  ["--summary", "--min-score", "0"], ["--summary", "--within", "0"],
                                  ["--summary", "--partition", "offsets"], ["--hist", "0:1:4"],
                                  ["--summary", "--hist", "0:0:4"], ["--summary", "--hist", "0:1:257"],
                                  ["--summary", "--hist", "0:1"], ["--summary", "--hist", "a:1:4"]])
def test_cli_refused_combinations(args):
    r = _cli(args, 6)
    assert r.returncode != 0 and r.stdout == b"" and r.stderr != b""


# ---- distributed -------------------------------------------------------------------------------------------
def test_run_summary_two_gloo_ranks():
    """DistributedSearch.run_summary over gloo at 2 ranks (through the CLI, as tests/test_dist.py runs it) prints
    what one process computes."""
    prob = Problem.read(input_path(3))
    want = format_summary(*search_summary_cpu(prob, 12, -500, 100))
    r = torchrun(2, ["--backend=cpu", "--dist-backend=gloo", "--summary", "--hist=-500:100:12",
                     f"--input={input_path(3)}"])
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert r.stdout.decode() == want


def test_run_summary_one_process_and_offsets_partition():
    from mpi_openmp_cuda_amd.parallel import dist as D
    from mpi_openmp_cuda_amd.parallel.search import DistributedSearch

    prob = Problem.read(input_path(1))
    s = DistributedSearch(D.DistContext(), backend="cpu", partition="records")
    summary, hist = s.run_summary(prob, 5, 0, 50, Semantics.SPEC)
    ws, wh = search_summary_cpu(prob, 5, 0, 50, semantics=Semantics.SPEC)
    assert np.array_equal(summary, ws) and np.array_equal(hist, wh) and hist.dtype == np.int32
    assert s.run_summary(prob)[1] is None
    with pytest.raises(ValueError, match="exactness bound"):
        s.run_summary(wide_problem(37, Semantics.REFERENCE))
    s = DistributedSearch(D.DistContext(), backend="cpu", partition="offsets")
    with pytest.raises(ValueError, match="record slices"):
        s.run_summary(prob)


# ---- stand-alone sanitizer program -------------------------------------------------------------------------
def test_summary_sanitizer_program():
    """csrc/tests/summary_san.cpp with the CPU core sources under ASan + UBSan: a plain program with its own main
    (nothing is loaded into Python, nothing runs on a GPU)."""
    r = subprocess.run(["make", "-C", ROOT, "-s", "-j8", "summary-san"], capture_output=True, timeout=600)
    out = (r.stdout + r.stderr).decode()
    assert r.returncode == 0, out[-3000:]
    assert "summary_san ok" in out and "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]
