"""Per-target profile summary on the CPU engine (csrc/src/cpu_engine.cpp targets_summary_batch_cpu). The oracle for
everything is the existing search_summary_cpu run once per target on Problem(weights, target_t, codes, offsets) — the
function tests/test_summary_cpu.py pins to the letter-by-letter replay, and which never sees the catalog. Covered:
random target sets under both semantics with and without a histogram, (max, n, k) against search_targets_cpu, T = 1,
the straddling record, pairs that do not fit, equal lengths and one-letter targets, the histogram at the int32 edges,
the exactness bound at its edge, targets_zscore, targets_best(rows, z=), the z-ranking experiment's determinism, the
Python CLI (--target-summary / --target-hist, one and two gloo ranks) and the stand-alone sanitizer program."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, expected, input_path
from test_dist import torchrun

from mpi_openmp_cuda_amd import (SUMMARY_COLS, Problem, Semantics, TargetSet, format_targets, format_targets_summary,
                                 search_summary_cpu, search_targets_cpu, search_targets_summary_cpu, summary_zscore,
                                 targets_best, targets_zscore)
from mpi_openmp_cuda_amd.ops.align import summary_bound, targets_geometry, targets_summary_geometry

SEMS = [Semantics.REFERENCE, Semantics.SPEC]
I32 = np.iinfo(np.int32)
NO_FIT = [0, 0, 0, I32.max, I32.min, 0, 0]
NONE = [I32.min, 0, 0]


def batch_of(recs):
    lens = np.array([len(r) for r in recs], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    codes = np.concatenate([np.asarray(r, np.uint8) for r in recs]) if len(recs) else np.zeros(0, np.uint8)
    return codes, offsets


def oracle(weights, ts, codes, offsets, sem, bins=0, lo=0, width=1):
    """search_summary_cpu per target alone, stacked: int64 [n, T, 7] and int32 [n, T, bins] (or None)."""
    got = [search_summary_cpu(Problem(weights, ts.target(t), codes, offsets), bins, lo, width, sem) for t in range(ts.T)]
    return np.stack([g[0] for g in got], axis=1), (np.stack([g[1] for g in got], axis=1) if bins else None)


def random_case(rng, n, alphabet):
    """n records and, around every record length L2, targets of L2 - 1, L2, L2 + 1 and L2 + 2 letters, plus a long
    and a single-letter one, in random order."""
    lens = rng.integers(1, 14, size=n)
    recs = [rng.integers(1, alphabet + 1, size=int(l)).astype(np.uint8) for l in lens]
    tl = [1, int(rng.integers(40, 90))]
    for l in lens:
        tl += [max(int(l) - 1, 1), int(l), int(l) + 1, int(l) + 2]
    rng.shuffle(tl)
    ts = TargetSet.from_sequences([rng.integers(1, alphabet + 1, size=l).astype(np.uint8) for l in tl])
    return ts, recs


# ---- against the per-target oracle -------------------------------------------------------------------------
@pytest.mark.parametrize("bins", [0, 5])
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("seed", range(5))
def test_random_problems_equal_per_target_summary(sem, seed, bins):
    rng = np.random.default_rng(300 + seed)
    ts, recs = random_case(rng, 6, (2, 3, 4, 12, 26)[seed])
    codes, offsets = batch_of(recs)
    w = [int(x) for x in rng.integers(0, 15, size=4)]
    prob = Problem(w, ts.seq1, codes, offsets)
    summary, hist = search_targets_summary_cpu(prob, ts, bins, -20, 9, sem)
    assert summary.dtype == np.int64 and summary.shape == (len(recs), ts.T, len(SUMMARY_COLS))
    ws, wh = oracle(w, ts, codes, offsets, sem, bins, -20, 9)
    assert np.array_equal(summary, ws)
    if bins:
        assert hist.dtype == np.int32 and hist.shape == (len(recs), ts.T, bins) and np.array_equal(hist, wh)
        assert np.array_equal(hist.sum(axis=2), summary[:, :, 0])
    else:
        assert hist is None
    # (max, n, k) is the multi-target search's row; pairs that do not fit give the empty row of both
    rows = search_targets_cpu(prob, ts, sem)
    fits = summary[:, :, 0] > 0
    assert np.array_equal(summary[:, :, 4:7][fits], rows[fits].astype(np.int64))
    assert (rows[~fits] == NONE).all() and (summary[~fits] == NO_FIT).all() and (~fits).any()
    for threads in (1, 3):
        s2, h2 = search_targets_summary_cpu(prob, ts.starts, bins, -20, 9, sem, threads)
        assert np.array_equal(s2, summary) and (h2 is None or np.array_equal(h2, hist))


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("i", [1, 6])
def test_one_target_is_the_summary_of_the_catalog(i, sem):
    prob = Problem.read(input_path(i))
    summary, hist = search_targets_summary_cpu(prob, [0, prob.L1], 7, -100, 40, sem)
    ws, wh = search_summary_cpu(prob, 7, -100, 40, sem)
    assert summary.shape == (prob.n, 1, 7) and np.array_equal(summary[:, 0], ws) and np.array_equal(hist[:, 0], wh)


# ---- the straddling case -----------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_straddling_record(sem):
    """Two random 60-letter targets, weights 4 3 2 10, one record: the last 20 letters of target 1 followed by the
    first 20 of target 2. The catalog's summary holds the straddling full match; neither target's does."""
    rng = np.random.default_rng(2024)
    t1, t2 = (rng.integers(1, 27, size=60).astype(np.uint8) for _ in range(2))
    ts = TargetSet.from_sequences([t1, t2])
    codes, offsets = batch_of([np.concatenate([t1[40:], t2[:20]])])
    w = [4, 3, 2, 10]
    catalog = Problem(w, ts.seq1, codes, offsets)
    whole, _ = search_summary_cpu(catalog, 0, 0, 1, sem)
    assert whole[0, 4:7].tolist() == [160, 40, 0]
    summary, _ = search_targets_summary_cpu(catalog, ts, 0, 0, 1, sem)
    for t in range(2):
        alone, _ = search_summary_cpu(Problem(w, ts.target(t), codes, offsets), 0, 0, 1, sem)
        assert np.array_equal(summary[0, t], alone[0])
        assert not np.array_equal(summary[0, t], whole[0]) and summary[0, t, 4] < 160
    # the catalog mixes both targets and the straddling offsets that exist in neither
    assert whole[0, 0] > summary[0, 0, 0] + summary[0, 1, 0]


# ---- edge pairs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_no_fit_equal_lengths_and_one_letter_targets(sem):
    ts = TargetSet.from_strings(["A", "Q", "ABAB", "QQAB", "ABABAB"])
    recs = [TargetSet.from_strings([s]).seq1 for s in ("A", "AB", "ABAB", "ABABABA")]
    codes, offsets = batch_of(recs)
    w = [4, 3, 2, 10]
    summary, hist = search_targets_summary_cpu(Problem(w, ts.seq1, codes, offsets), ts, 3, 0, 4, sem)
    ws, wh = oracle(w, ts, codes, offsets, sem, 3, 0, 4)
    assert np.array_equal(summary, ws) and np.array_equal(hist, wh)
    assert summary[0, 0].tolist() == [1, 4, 16, 4, 4, 0, 0]        # one letter against itself: the boundary entry only
    assert summary[0, 1, 0] == 1 and summary[0, 1, 5:].tolist() == [0, 0]
    assert summary[2, 2].tolist() == [1, 16, 256, 16, 16, 0, 0]    # len_t == L2 under both semantics
    assert summary[1, 0].tolist() == NO_FIT and hist[1, 0].tolist() == [0, 0, 0]
    assert (summary[3] == NO_FIT).all() and (hist[3] == 0).all()  # fits no target
    spec = sem == Semantics.SPEC
    assert summary[1, 2, 0] == 2 + spec and summary[0, 4, 0] == 5 + spec


def test_histogram_rows_sum_to_count_at_the_int32_edges():
    rng = np.random.default_rng(11)
    ts, recs = random_case(rng, 5, 4)
    codes, offsets = batch_of(recs)
    prob = Problem([4, 3, 2, 10], ts.seq1, codes, offsets)
    for bins, lo, width in ((4, I32.min, I32.max), (2, I32.min, I32.max), (256, I32.min, 1), (3, I32.max, 1)):
        summary, hist = search_targets_summary_cpu(prob, ts, bins, lo, width, Semantics.SPEC)
        assert np.array_equal(hist.astype(np.int64).sum(axis=2), summary[:, :, 0])
        assert np.array_equal(hist, oracle([4, 3, 2, 10], ts, codes, offsets, Semantics.SPEC, bins, lo, width)[1])


# ---- the exactness bound -----------------------------------------------------------------------------------
def bound_case(target_lens):
    rng = np.random.default_rng(7)
    ts = TargetSet.from_sequences([rng.integers(1, 27, size=l).astype(np.uint8) for l in target_lens])
    codes, offsets = batch_of([rng.integers(1, 27, size=500).astype(np.uint8)])
    return Problem([1000000, 3, 2, 1], ts.seq1, codes, offsets), ts


def test_exactness_bound_at_its_edge():
    assert summary_bound(1000000, 500) == 36
    prob, ts = bound_case([536])  # 36 entries under the reference semantics
    summary, _ = search_targets_summary_cpu(prob, ts)
    assert summary[0, 0, 0] == 36
    assert np.array_equal(summary[:, 0], search_summary_cpu(prob)[0])
    prob, ts = bound_case([537])
    with pytest.raises(ValueError, match="^summary:"):
        search_targets_summary_cpu(prob, ts)
    with pytest.raises(ValueError, match="^summary:"):
        search_targets_summary_cpu(*bound_case([536]), semantics=Semantics.SPEC)  # the boundary entry is the 37th
    # a catalog of two 536-letter targets: its own profile (572 entries) is refused, every target's is within the bound
    prob, ts = bound_case([536, 536])
    with pytest.raises(ValueError, match="^summary:"):
        search_summary_cpu(prob)
    summary, hist = search_targets_summary_cpu(prob, ts, 4, -10 ** 9, 5 * 10 ** 8)
    ws, wh = oracle(prob.weights, ts, prob.codes, prob.offsets, Semantics.REFERENCE, 4, -10 ** 9, 5 * 10 ** 8)
    assert np.array_equal(summary, ws) and np.array_equal(hist, wh) and (summary[0, :, 0] == 36).all()


def test_argument_and_target_set_errors():
    ts = TargetSet.from_strings(["ABC", "DE"])
    codes, offsets = batch_of([np.ones(2, np.uint8)])
    prob = Problem([1, 1, 1, 1], ts.seq1, codes, offsets)
    for bad in ((-1, 0, 1), (257, 0, 1), (4, 0, 0), (4, 2 ** 31, 1)):
        with pytest.raises(ValueError, match="^summary:"):
            search_targets_summary_cpu(prob, ts, *bad)
    for starts in ([0, 4], [1, 5], [0, 3, 3, 5], []):
        with pytest.raises(ValueError, match="^targets:"):
            search_targets_summary_cpu(prob, starts)
    summary, hist = search_targets_summary_cpu(Problem([1, 2, 3, 4], ts.seq1), ts, 3)
    assert summary.shape == (0, 2, 7) and hist.shape == (0, 2, 3)


def test_geometry():
    threads, max_bins, group4_bins, lds = targets_summary_geometry()
    assert threads == targets_geometry()[1] == 256 and max_bins == 256 and lds == 16 * 1024
    # 64 four-lane groups of group4_bins counters fill the LDS budget; 16 sixteen-lane groups of max_bins fit it
    assert (threads // 4) * group4_bins * 4 == lds and group4_bins == 64
    assert (threads // 16) * max_bins * 4 <= lds


# ---- helpers -----------------------------------------------------------------------------------------------
def helper_case():
    rng = np.random.default_rng(9)
    ts, recs = random_case(rng, 7, 4)
    recs.append(rng.integers(1, 5, size=200).astype(np.uint8))  # fits no target
    codes, offsets = batch_of(recs)
    prob = Problem([4, 3, 2, 10], ts.seq1, codes, offsets)
    return prob, ts, search_targets_summary_cpu(prob, ts, 0, 0, 1, Semantics.SPEC)[0]


def test_targets_zscore_is_summary_zscore_per_pair():
    _, ts, summary = helper_case()
    z = targets_zscore(summary)
    assert z.dtype == np.float64 and z.shape == summary.shape[:2]
    for t in range(ts.T):
        assert np.array_equal(z[:, t], summary_zscore(summary[:, t]), equal_nan=True)
    assert np.isnan(z).any() and not np.isnan(z).all()
    assert np.isnan(z[summary[:, :, 0] < 3]).all()
    with pytest.raises(ValueError):
        targets_zscore(summary[:, 0])


def best_by_z_loop(rows, z):
    best, out = [], []
    for i in range(rows.shape[0]):
        pick = None
        for t in range(rows.shape[1]):
            s = int(rows[i, t, 0])
            if s == I32.min:
                continue
            key = (0, 0.0, s) if math.isnan(z[i, t]) else (1, float(z[i, t]), s)
            if pick is None or key > pick[0]:  # strictly better only: the smaller index keeps a tie
                pick = (key, t)
        best.append(-1 if pick is None else pick[1])
        out.append(NONE if pick is None else rows[i, pick[1]].tolist())
    return np.array(best, np.int32), np.array(out, np.int32)


def crafted_rows_and_z():
    nan = float("nan")
    rows = np.array([
        [[5, 1, 0], [9, 2, 1], [7, 0, 0]],            # plain: the highest z
        [[5, 1, 0], [9, 2, 1], [7, 0, 0]],            # a NaN ranks below every defined z, even a negative one
        [[5, 1, 0], [9, 2, 1], [7, 0, 0]],            # all NaN: the higher score
        [[5, 1, 0], [9, 2, 1], [9, 3, 0]],            # equal z: the higher score, then the smaller index
        [[I32.min, 0, 0], [4, 0, 0], [I32.min, 0, 0]],  # one fitting target with a NaN z
        [[I32.min, 0, 0]] * 3,                        # no target fits
        [[I32.min, 0, 0], [3, 0, 0], [8, 1, 1]],      # a non-fitting pair's z is never read
    ], np.int32)
    z = np.array([[1.0, 2.0, 3.0], [nan, nan, -4.0], [nan, nan, nan], [2.5, 2.5, 2.5], [nan, nan, nan],
                  [nan, nan, nan], [99.0, 1.0, 0.5]])
    want = [2, 2, 1, 1, 1, -1, 1]
    return rows, z, want


def test_targets_best_by_z_against_a_loop():
    rows, z, want = crafted_rows_and_z()
    best, row = targets_best(rows, z=z)
    assert best.dtype == np.int32 and best.tolist() == want
    wb, wr = best_by_z_loop(rows, z)
    assert np.array_equal(best, wb) and np.array_equal(row, wr)
    prob, _, summary = helper_case()
    rows = search_targets_cpu(prob, _, Semantics.SPEC)
    z = targets_zscore(summary)
    best, row = targets_best(rows, z)
    wb, wr = best_by_z_loop(rows, z)
    assert np.array_equal(best, wb) and np.array_equal(row, wr) and best[-1] == -1
    with pytest.raises(ValueError):
        targets_best(rows, z[:, :-1])


def test_targets_best_without_z_is_unchanged():
    prob, ts, _ = helper_case()
    rows = search_targets_cpu(prob, ts, Semantics.SPEC)
    best, row = targets_best(rows)
    b2, r2 = targets_best(rows, z=None)
    assert np.array_equal(best, b2) and np.array_equal(row, r2)
    for i in range(rows.shape[0]):  # the highest score, then the smallest target index
        want_t, want = -1, NONE
        for t in range(ts.T):
            if rows[i, t, 0] != I32.min and (want_t < 0 or rows[i, t, 0] > want[0]):
                want_t, want = t, rows[i, t].tolist()
        assert best[i] == want_t and row[i].tolist() == want


def test_helpers_on_torch_tensors():
    torch = pytest.importorskip("torch")
    prob, ts, summary = helper_case()
    z = targets_zscore(torch.from_numpy(summary))
    want = targets_zscore(summary)
    assert z.dtype == torch.float64 and tuple(z.shape) == want.shape
    assert np.array_equal(np.isnan(z.numpy()), np.isnan(want))
    assert np.allclose(z.numpy(), want, rtol=1e-9, atol=0, equal_nan=True)  # float64 moments against exact integers
    rows, zc, _ = crafted_rows_and_z()
    best, row = targets_best(torch.from_numpy(rows), torch.from_numpy(zc))
    wb, wr = targets_best(rows, zc)
    assert best.dtype == torch.int32 and np.array_equal(best.numpy(), wb) and np.array_equal(row.numpy(), wr)
    rows = search_targets_cpu(prob, ts, Semantics.SPEC)
    best, row = targets_best(torch.from_numpy(rows), torch.from_numpy(want))
    wb, wr = targets_best(rows, want)
    assert np.array_equal(best.numpy(), wb) and np.array_equal(row.numpy(), wr)


# ---- does z ranking help? (the README's experiment; here only that it is deterministic and well-formed) -------
def z_ranking_experiment():
    rng = np.random.default_rng(20261020)
    short, long_ = (rng.integers(1, 21, size=l).astype(np.uint8) for l in (80, 8000))
    ts = TargetSet.from_sequences([short, long_])
    recs = []
    for _ in range(200):
        at = int(rng.integers(0, 41))
        rec = short[at:at + 40].copy()
        where = rng.choice(40, size=24, replace=False)
        rec[where] = rng.integers(1, 21, size=24)
        recs.append(rec)
    codes, offsets = batch_of(recs)
    prob = Problem([4, 3, 2, 10], ts.seq1, codes, offsets)
    summary, _ = search_targets_summary_cpu(prob, ts)
    rows = np.ascontiguousarray(summary[:, :, 4:7]).astype(np.int32)
    by_score, _ = targets_best(rows)
    by_z, _ = targets_best(rows, targets_zscore(summary))
    return int((by_score == 0).sum()), int((by_z == 0).sum())


def test_z_ranking_experiment_is_deterministic():
    a, b = z_ranking_experiment(), z_ranking_experiment()
    assert a == b and all(0 <= x <= 200 for x in a)


# ---- formatting and the Python CLI -------------------------------------------------------------------------
def test_format_targets_summary():
    ts = TargetSet.from_strings(["ABAB", "QQAB", "A"])
    codes, offsets = batch_of([TargetSet.from_strings(["AB"]).seq1, TargetSet.from_strings(["ZZZZZ"]).seq1])
    prob = Problem([4, 3, 2, 10], ts.seq1, codes, offsets)
    summary, hist = search_targets_summary_cpu(prob, ts, 2, 0, 5, Semantics.SPEC)
    text = format_targets_summary(summary, hist)
    rows = search_targets_cpu(prob, ts, Semantics.SPEC)
    plain = format_targets(rows[:, 0], rows)
    kept = [l for l in text.splitlines() if not l.startswith("    ") and not l.startswith("  best by z")]
    assert "".join(l + "\n" for l in kept) == plain
    lines = text.splitlines()
    assert lines[1] == "  target 1: score: 8, n: 0, k: 0"
    assert lines[2].startswith("    summary: offsets: 3, min: ") and lines[2].count(",") == 5
    assert lines[3].startswith("    hist: ") and sum(int(x) for x in lines[3].split()[1:]) == 3
    assert "    summary: offsets: 0, min: 2147483647, max: -2147483648, mean: nan, sd: nan, z: nan" in lines
    assert lines.count("  best by z: none") == 1 and sum(l.startswith("  best by z: ") for l in lines) == 2
    assert "hist" not in format_targets_summary(summary)
    with pytest.raises(ValueError):
        format_targets_summary(summary[:, 0])
    with pytest.raises(ValueError):
        format_targets_summary(summary, hist[:1])


def _cli(args, i):
    with open(input_path(i), "rb") as f:
        return subprocess.run([sys.executable, "-m", "mpi_openmp_cuda_amd", "--backend=cpu"] + args, stdin=f,
                              capture_output=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd="/tmp", timeout=120)


def cli_targets_file(tmp_path, prob):
    """A targets file for a golden input: a piece of its Seq1, a single letter, and its first record."""
    lines = [prob.seq1_str()[3:3 + max(prob.L1 // 2, 1)], "Q", prob.record(0), ""]
    path = tmp_path / "targets.txt"
    path.write_text("\n".join(lines))
    return str(path), TargetSet.from_strings([prob.seq1_str()] + lines[:3])


def cli_want(prob, ts, bins=0, lo=0, width=1):
    catalog = Problem(prob.weights, ts.seq1, prob.codes, prob.offsets)
    return format_targets_summary(*search_targets_summary_cpu(catalog, ts, bins, lo, width))


@pytest.mark.parametrize("i", [1, 6])
def test_cli_target_summary(tmp_path, i):
    prob = Problem.read(input_path(i))
    path, ts = cli_targets_file(tmp_path, prob)
    r = _cli(["--targets", path, "--target-summary"], i)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    out = r.stdout.decode()
    assert out == cli_want(prob, ts)
    assert "".join(l + "\n" for l in out.splitlines() if not l.startswith("  ")) == expected(i)  # unchanged lines
    assert sum(l.startswith("    summary: ") for l in out.splitlines()) == prob.n * 4
    assert sum(l.startswith("  best by z: ") for l in out.splitlines()) == prob.n
    r = _cli(["--targets", path, "--target-summary", "--target-hist=-50:25:6"], i)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout.decode() == cli_want(prob, ts, 6, -50, 25)
    assert sum(l.startswith("    hist: ") for l in r.stdout.decode().splitlines()) == prob.n * 4


def test_cli_target_summary_two_gloo_ranks(tmp_path):
    prob = Problem.read(input_path(3))
    path, ts = cli_targets_file(tmp_path, prob)
    r = torchrun(2, ["--backend=cpu", "--dist-backend=gloo", "--targets", path, "--target-summary",
                     "--target-hist=0:50:4", f"--input={input_path(3)}"])
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert r.stdout.decode() == cli_want(prob, ts, 4, 0, 50)


def test_cli_without_the_new_flags_is_todays_output(tmp_path):
    prob = Problem.read(input_path(1))
    path, ts = cli_targets_file(tmp_path, prob)
    r = _cli([], 1)
    assert r.returncode == 0 and r.stdout.decode() == expected(1)
    r = _cli(["--targets", path], 1)
    rows = search_targets_cpu(Problem(prob.weights, ts.seq1, prob.codes, prob.offsets), ts)
    assert r.returncode == 0 and r.stdout.decode() == format_targets(rows[:, 0], rows)


@pytest.mark.parametrize("extra", [["--top", "2"], ["--show-alignment"], ["--min-score", "0"], ["--within", "0"],
                                   ["--min-score", "0", "--distinct", "2"], ["--summary"],
                                   ["--summary", "--hist", "0:1:4"], ["--partition", "offsets"]])
def test_cli_refused_combinations(tmp_path, extra):
    prob = Problem.read(input_path(6))
    path, _ = cli_targets_file(tmp_path, prob)
    r = _cli(["--targets", path, "--target-summary", "--target-hist", "0:1:4"] + extra, 6)
    assert r.returncode != 0 and r.stdout == b"" and r.stderr != b""


@pytest.mark.parametrize("args", [["--target-summary"], ["--target-hist", "0:1:4"],
                                  ["--targets", "FILE", "--target-hist", "0:1:4"],
                                  ["--targets", "FILE", "--target-summary", "--target-hist", "0:0:4"],
                                  ["--targets", "FILE", "--target-summary", "--target-hist", "0:1:257"],
                                  ["--targets", "FILE", "--target-summary", "--target-hist", "0:1"]])
def test_cli_flags_need_each_other(tmp_path, args):
    prob = Problem.read(input_path(6))
    path, _ = cli_targets_file(tmp_path, prob)
    r = _cli([path if a == "FILE" else a for a in args], 6)
    assert r.returncode != 0 and r.stdout == b"" and r.stderr != b""


def test_run_targets_summary_one_process_and_errors():
    from mpi_openmp_cuda_amd.parallel import dist as D
    from mpi_openmp_cuda_amd.parallel.search import DistributedSearch

    prob, ts, summary = helper_case()
    s = DistributedSearch(D.DistContext(), backend="cpu", partition="records")
    got, hist = s.run_targets_summary(prob, ts, 3, 0, 10, Semantics.SPEC)
    want, wh = search_targets_summary_cpu(prob, ts, 3, 0, 10, Semantics.SPEC)
    assert got.dtype == np.int64 and np.array_equal(got, summary) and np.array_equal(got, want)
    assert hist.dtype == np.int32 and np.array_equal(hist, wh)
    assert s.run_targets_summary(prob, ts, semantics=Semantics.SPEC)[1] is None
    with pytest.raises(ValueError, match="^targets:"):
        s.run_targets_summary(prob, ts.starts[:-1])
    with pytest.raises(ValueError, match="^summary:"):
        s.run_targets_summary(*bound_case([537]))
    got, _ = s.run_targets_summary(*bound_case([536, 536]))
    assert (got[0, :, 0] == 36).all()
    s = DistributedSearch(D.DistContext(), backend="cpu", partition="offsets")
    with pytest.raises(ValueError, match="record slices"):
        s.run_targets_summary(prob, ts)


# ---- stand-alone sanitizer program -------------------------------------------------------------------------
def test_targets_summary_sanitizer_program():
    """csrc/tests/targets_summary_san.cpp with the CPU core sources under ASan + UBSan: a plain program with its own
    main (nothing is loaded into Python, nothing runs on a GPU)."""
    r = subprocess.run(["make", "-C", ROOT, "-s", "-j8", "targets-summary-san"], capture_output=True, timeout=600)
    out = (r.stdout + r.stderr).decode()
    assert r.returncode == 0, out[-3000:]
    assert "targets_summary_san ok" in out and "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]
