"""Multi-target search on the CPU engine (csrc/src/cpu_engine.cpp targets_batch_cpu). The oracle for everything is
the existing search_cpu run once per target on Problem(weights, target_t, codes, offsets) — the function
tests/test_engines_cpu.py pins to the letter-by-letter replay, and which never sees the catalog. Covered: random
problems under both semantics with target lengths around every record length, T = 1 on the goldens, the straddling
case (the trap of a hand-made concatenation), ties, invalid target sets, the helpers targets_best /
targets_catalog_rows, format_targets, the Python CLI (--targets, one and two gloo ranks) and the stand-alone sanitizer
program."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, expected, input_path
from test_dist import torchrun

from mpi_openmp_cuda_amd import (Problem, Semantics, TargetSet, format_results, format_targets, report_scores,
                                 search_cpu, search_report_cpu, search_targets_cpu, targets_best,
                                 targets_catalog_rows)
from mpi_openmp_cuda_amd.models.scoring import decode
from mpi_openmp_cuda_amd.ops.align import TARGETS_MAX, as_triples, check_targets, targets_geometry

SEMS = [Semantics.REFERENCE, Semantics.SPEC]
I32 = np.iinfo(np.int32)
NONE = [I32.min, 0, 0]


def batch_of(recs):
    lens = np.array([len(r) for r in recs], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    codes = np.concatenate([np.asarray(r, np.uint8) for r in recs]) if len(recs) else np.zeros(0, np.uint8)
    return codes, offsets


def oracle(weights, ts, codes, offsets, sem):
    """The stack of per-target search_cpu rows: int32 [n, T, 3]."""
    cols = [as_triples(search_cpu(Problem(weights, ts.target(t), codes, offsets), sem)) for t in range(ts.T)]
    return np.stack(cols, axis=1)


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
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("seed", range(6))
def test_random_problems_equal_per_target_search(sem, seed):
    rng = np.random.default_rng(100 + seed)
    ts, recs = random_case(rng, 6, (2, 3, 4, 6, 12, 26)[seed])
    codes, offsets = batch_of(recs)
    w = [int(x) for x in rng.integers(0, 15, size=4)]
    got = search_targets_cpu(Problem(w, ts.seq1, codes, offsets), ts, sem)
    assert got.dtype == np.int32 and got.shape == (len(recs), ts.T, 3)
    assert np.array_equal(got, oracle(w, ts, codes, offsets, sem))
    for threads in (1, 3):
        assert np.array_equal(search_targets_cpu(Problem(w, ts.seq1, codes, offsets), ts.starts, sem, threads), got)


@pytest.mark.parametrize("i", [1, 2, 3, 4, 5, 6])
def test_one_target_is_the_search_on_the_goldens(i):
    prob = Problem.read(input_path(i))
    rows = search_targets_cpu(prob, [0, prob.L1])
    assert rows.shape == (prob.n, 1, 3)
    assert np.array_equal(rows[:, 0], as_triples(search_cpu(prob)))
    assert format_results(np.ascontiguousarray(rows[:, 0])) == expected(i)


def test_one_target_is_the_search_under_spec():
    prob = Problem.read(input_path(1))
    rows = search_targets_cpu(prob, [0, prob.L1], Semantics.SPEC)
    assert np.array_equal(rows[:, 0], as_triples(search_cpu(prob, Semantics.SPEC)))


# ---- the straddling case -----------------------------------------------------------------------------------
def straddling_case():
    """Two random 60-letter targets, weights 4 3 2 10, one record: the last 20 letters of target 1 followed by the
    first 20 of target 2. On the catalog it matches letter for letter at offset 40, a placement in neither target."""
    rng = np.random.default_rng(2024)
    t1, t2 = (rng.integers(1, 27, size=60).astype(np.uint8) for _ in range(2))
    ts = TargetSet.from_sequences([t1, t2])
    rec = np.concatenate([t1[40:], t2[:20]])
    return [4, 3, 2, 10], ts, [rec]


@pytest.mark.parametrize("sem", SEMS)
def test_straddling_record(sem):
    w, ts, recs = straddling_case()
    codes, offsets = batch_of(recs)
    catalog = Problem(w, ts.seq1, codes, offsets)
    full = 4 * 40  # every pair identical
    trap = as_triples(search_cpu(catalog, sem))[0]
    assert trap.tolist() == [full, 40, 0]  # the trap: the catalog searched as one Seq1
    rows = search_targets_cpu(catalog, ts, sem)
    assert full not in rows[0, :, 0].tolist()
    assert np.array_equal(rows, oracle(w, ts, codes, offsets, sem))


# ---- ties ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_one_repeated_letter_gives_offset_zero(sem):
    ts = TargetSet.from_sequences([np.full(l, 7, np.uint8) for l in (9, 4, 5, 30)])
    codes, offsets = batch_of([np.full(l, 7, np.uint8) for l in (1, 4, 5, 6)])
    w = [5, 1, 2, 3]
    rows = search_targets_cpu(Problem(w, ts.seq1, codes, offsets), ts, sem)
    lens = np.diff(offsets)
    for i in range(4):
        for t in range(ts.T):
            want = [5 * int(lens[i]), 0, 0] if lens[i] <= ts.lengths[t] else NONE
            assert rows[i, t].tolist() == want
    assert np.array_equal(rows, oracle(w, ts, codes, offsets, sem))


@pytest.mark.parametrize("sem", SEMS)
def test_identical_targets_give_identical_rows_and_the_first_is_best(sem):
    rng = np.random.default_rng(5)
    t = rng.integers(1, 5, size=33).astype(np.uint8)
    other = rng.integers(1, 5, size=20).astype(np.uint8)
    ts = TargetSet.from_sequences([other, t, t])
    codes, offsets = batch_of([t[5:17], t[:33], other[3:9]])
    rows = search_targets_cpu(Problem([4, 3, 2, 10], ts.seq1, codes, offsets), ts, sem)
    assert np.array_equal(rows[:, 1], rows[:, 2])
    best, row = targets_best(rows)
    assert best.tolist() == [1, 1, 0]
    assert np.array_equal(row[:2], rows[:2, 1])


def test_boundary_entry_equal_to_the_slice_maximum_loses_under_spec():
    # target ABAB, record AB: un-mutated offsets 0 and 2 both match fully; offset 2 is the target's boundary diagonal
    ts = TargetSet.from_strings(["ABAB", "QQAB"])
    codes, offsets = batch_of([TargetSet.from_strings(["AB"]).seq1])
    rows = search_targets_cpu(Problem([4, 3, 2, 10], ts.seq1, codes, offsets), ts, Semantics.SPEC)
    assert rows[0, 0].tolist() == [8, 0, 0]  # the tie goes to the slice's smaller offset
    assert rows[0, 1].tolist() == [8, 2, 0]  # a strictly higher boundary entry wins
    assert np.array_equal(rows, oracle([4, 3, 2, 10], ts, codes, offsets, Semantics.SPEC))


# ---- invalid target sets -----------------------------------------------------------------------------------
@pytest.mark.parametrize("starts", [[1, 10], [0, 9], [0, 11], [0, 4, 4, 10], [0, 6, 5, 10], [0], [],
                                    list(range(TARGETS_MAX + 2))])
def test_invalid_starts_are_value_errors(starts):
    L1 = 10 if len(starts) < 100 else TARGETS_MAX + 1
    codes, offsets = batch_of([np.ones(3, np.uint8)])
    prob = Problem([1, 1, 1, 1], np.ones(L1, np.uint8), codes, offsets)
    with pytest.raises(ValueError, match="^targets:"):
        search_targets_cpu(prob, starts)
    with pytest.raises(ValueError, match="^targets:"):
        check_targets(starts, L1)


def test_target_set_and_limits():
    assert targets_geometry()[0] == TARGETS_MAX == 4096
    ts = TargetSet.from_strings(["abc", "DEFG", "h"])
    assert ts.T == 3 and ts.starts.tolist() == [0, 3, 7, 8] and ts.lengths.tolist() == [3, 4, 1]
    assert decode(ts.seq1) == "ABCDEFGH" and decode(ts.target(1)) == "DEFG"
    assert ts.starts.dtype == np.int64 and ts.seq1.dtype == np.uint8
    with pytest.raises(ValueError, match="^targets:"):
        TargetSet.from_strings(["ABC", ""])
    with pytest.raises(ValueError, match="^targets:"):
        TargetSet.from_sequences([])
    with pytest.raises(ValueError):
        TargetSet.from_strings(["AB1"])
    many = TargetSet.from_sequences([np.ones(1, np.uint8)] * TARGETS_MAX)  # the largest T
    assert many.T == TARGETS_MAX
    with pytest.raises(ValueError, match="^targets:"):
        TargetSet.from_sequences([np.ones(1, np.uint8)] * (TARGETS_MAX + 1))


def test_empty_batch():
    ts = TargetSet.from_strings(["ABC", "DE"])
    rows = search_targets_cpu(Problem([1, 2, 3, 4], ts.seq1), ts)
    assert rows.shape == (0, 2, 3)


# ---- helpers -----------------------------------------------------------------------------------------------
def helper_rows():
    rng = np.random.default_rng(9)
    ts, recs = random_case(rng, 7, 4)
    recs.append(rng.integers(1, 5, size=200).astype(np.uint8))  # fits no target
    codes, offsets = batch_of(recs)
    w = [4, 3, 2, 10]
    prob = Problem(w, ts.seq1, codes, offsets)
    return prob, ts, search_targets_cpu(prob, ts, Semantics.SPEC)


def test_targets_best_against_a_loop():
    _, ts, rows = helper_rows()
    best, row = targets_best(rows)
    assert best.dtype == np.int32 and row.dtype == np.int32 and row.shape == (rows.shape[0], 3)
    for i in range(rows.shape[0]):
        want_t, want = -1, NONE
        for t in range(ts.T):
            if rows[i, t, 0] != I32.min and (want_t < 0 or rows[i, t, 0] > want[0]):
                want_t, want = t, rows[i, t].tolist()
        assert best[i] == want_t and row[i].tolist() == want
    assert best[-1] == -1 and (best[:-1] >= 0).all()


def test_targets_catalog_rows_against_a_loop_and_the_report():
    prob, ts, rows = helper_rows()
    before = rows.copy()
    cat = targets_catalog_rows(rows, ts.starts)
    assert np.array_equal(rows, before)  # a copy
    assert np.array_equal(cat, targets_catalog_rows(rows, ts))
    for i in range(rows.shape[0]):
        for t in range(ts.T):
            s, n, k = rows[i, t].tolist()
            assert cat[i, t].tolist() == ([s, n, k] if s == I32.min else [s, n + int(ts.starts[t]), k])
    # the catalog rows place every record inside the catalog with exactly the row's score
    scores = report_scores(search_report_cpu(prob, cat), prob.weights)
    real = rows[:, :, 0] != I32.min
    assert real.any() and not real.all()
    assert np.array_equal(scores[real], rows[:, :, 0][real].astype(np.int64))
    with pytest.raises(ValueError):
        targets_catalog_rows(rows, ts.starts[:-1])


def test_helpers_on_torch_tensors():
    torch = pytest.importorskip("torch")
    _, ts, rows = helper_rows()
    best, row = targets_best(torch.from_numpy(rows))
    wb, wr = targets_best(rows)
    assert best.dtype == torch.int32 and np.array_equal(best.numpy(), wb) and np.array_equal(row.numpy(), wr)
    cat = targets_catalog_rows(torch.from_numpy(rows), ts)
    assert cat.dtype == torch.int32 and np.array_equal(cat.numpy(), targets_catalog_rows(rows, ts))


def test_format_targets():
    ts = TargetSet.from_strings(["ABAB", "QQAB", "A"])
    codes, offsets = batch_of([TargetSet.from_strings(["AB"]).seq1, TargetSet.from_strings(["ZZZZZ"]).seq1])
    rows = search_targets_cpu(Problem([4, 3, 2, 10], ts.seq1, codes, offsets), ts, Semantics.SPEC)
    text = format_targets(rows[:, 0], rows)
    assert text == ("#0: score: 8, n: 0, k: 0\n  target 1: score: 8, n: 0, k: 0\n  target 2: score: 8, n: 2, k: 0\n"
                    "  target 3: none\n  best: 1\n"
                    f"#1: score: {I32.min}, n: 0, k: 0\n  target 1: none\n  target 2: none\n  target 3: none\n"
                    "  best: none\n")
    with pytest.raises(ValueError):
        format_targets(rows[:1, 0], rows)


# ---- the Python CLI ----------------------------------------------------------------------------------------
def _cli(args, i):
    with open(input_path(i), "rb") as f:
        return subprocess.run([sys.executable, "-m", "mpi_openmp_cuda_amd", "--backend=cpu"] + args, stdin=f,
                              capture_output=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd="/tmp", timeout=120)


def cli_targets_file(tmp_path, prob):
    """A targets file for a golden input: a piece of its Seq1, a single letter, and its first record."""
    lines = [prob.seq1_str()[3:3 + max(prob.L1 // 2, 1)], "Q", prob.record(0), ""]
    path = tmp_path / "targets.txt"
    path.write_text("\n".join(lines))
    ts = TargetSet.from_strings([prob.seq1_str()] + lines[:3])
    return str(path), ts


def cli_want(prob, ts):
    catalog = Problem(prob.weights, ts.seq1, prob.codes, prob.offsets)
    rows = search_targets_cpu(catalog, ts)
    return format_targets(rows[:, 0], rows), rows


@pytest.mark.parametrize("i", [1, 6])
def test_cli_targets(tmp_path, i):
    prob = Problem.read(input_path(i))
    path, ts = cli_targets_file(tmp_path, prob)
    r = _cli(["--targets", path], i)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    out = r.stdout.decode()
    want, rows = cli_want(prob, ts)
    assert out == want
    assert "".join(l + "\n" for l in out.splitlines() if not l.startswith("  ")) == expected(i)  # unchanged lines
    assert sum(l.startswith("  target ") for l in out.splitlines()) == prob.n * 4
    assert sum(l.startswith("  best: ") for l in out.splitlines()) == prob.n
    assert np.array_equal(rows[:, 0], as_triples(search_cpu(prob)))  # target 1 repeats the usual result


def test_cli_targets_two_gloo_ranks(tmp_path):
    prob = Problem.read(input_path(3))
    path, ts = cli_targets_file(tmp_path, prob)
    r = torchrun(2, ["--backend=cpu", "--dist-backend=gloo", "--targets", path, f"--input={input_path(3)}"])
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert r.stdout.decode() == cli_want(prob, ts)[0]


def test_cli_without_the_flag_is_todays_output():
    r = _cli([], 1)
    assert r.returncode == 0 and r.stdout.decode() == expected(1)


@pytest.mark.parametrize("extra", [["--top", "2"], ["--show-alignment"], ["--min-score", "0"], ["--within", "0"],
                                   ["--min-score", "0", "--distinct", "2"], ["--summary"],
                                   ["--summary", "--hist", "0:1:4"], ["--partition", "offsets"]])
def test_cli_refused_combinations(tmp_path, extra):
    prob = Problem.read(input_path(6))
    path, _ = cli_targets_file(tmp_path, prob)
    r = _cli(["--targets", path] + extra, 6)
    assert r.returncode != 0 and r.stdout == b"" and r.stderr != b""


def test_cli_bad_targets_file(tmp_path):
    bad = tmp_path / "bad.txt"
    bad.write_text("ABC\nAB1\n")
    r = _cli(["--targets", str(bad)], 6)
    assert r.returncode != 0 and r.stdout == b"" and b"input error" in r.stderr
    r = _cli(["--targets", str(tmp_path / "missing.txt")], 6)
    assert r.returncode != 0 and r.stdout == b"" and b"input error" in r.stderr


def test_run_targets_one_process_and_offsets_partition():
    from mpi_openmp_cuda_amd.parallel import dist as D
    from mpi_openmp_cuda_amd.parallel.search import DistributedSearch

    prob, ts, rows = helper_rows()
    s = DistributedSearch(D.DistContext(), backend="cpu", partition="records")
    got = s.run_targets(prob, ts, Semantics.SPEC)
    assert got.dtype == np.int32 and np.array_equal(got, rows)
    with pytest.raises(ValueError, match="^targets:"):
        s.run_targets(prob, ts.starts[:-1])
    s = DistributedSearch(D.DistContext(), backend="cpu", partition="offsets")
    with pytest.raises(ValueError, match="record slices"):
        s.run_targets(prob, ts)


# ---- stand-alone sanitizer program -------------------------------------------------------------------------
def test_targets_sanitizer_program():
    """csrc/tests/targets_san.cpp with the CPU core sources under ASan + UBSan: a plain program with its own main
    (nothing is loaded into Python, nothing runs on a GPU)."""
    r = subprocess.run(["make", "-C", ROOT, "-s", "-j8", "targets-san"], capture_output=True, timeout=600)
    out = (r.stdout + r.stderr).decode()
    assert r.returncode == 0, out[-3000:]
    assert "targets_san ok" in out and "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]
