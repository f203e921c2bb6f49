"""Target ranking on the CPU engine (csrc/src/cpu_engine.cpp targets_rank_batch_cpu) and its host-only parts. The
oracles never see the ranking code: search_targets_cpu's [n, T, 3] rows stably sorted in numpy
(targets_rank_cases.rank_model) and search_cpu run on every target alone. Covered: random problems and the straddling
record under both semantics; row 0 against targets_best; M = 1, F - 1, F, F + 1 and 64; T = 1; a record longer than
every target; identical targets; two different targets that tie; targets_rank_catalog_rows against a loop and through
search_report_cpu; the chunk cut against a Python-int model; every error and their order; the formatter; --target-best
at one and two gloo ranks with its refusals; DistributedSearch on one process; the stand-alone sanitizer program."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, expected, input_path
from test_dist import torchrun

from mpi_openmp_cuda_amd import (RANK_COLS, Problem, Semantics, TargetSet, _lib, format_targets, format_targets_rank,
                                 report_scores, search_cpu, search_report_cpu, search_targets_cpu,
                                 search_targets_rank_cpu, targets_best, targets_rank_catalog_rows, targets_rank_chunks)
from mpi_openmp_cuda_amd.ops.align import REPORT_EMPTY, as_triples, targets_rank_geometry

from targets_rank_cases import (I32, PAD, SEMS, W, around_m_case, batch_of, chunks_model, entries_of, fitting,
                                random_case, rank_model, straddling_case)


def check_rank(prob, ts, M, sem):
    """The ranking against the numpy model over search_targets_cpu's rows, and row by row against search_cpu on the
    listed target alone."""
    rank = search_targets_rank_cpu(prob, ts, M, sem)
    assert rank.dtype == np.int32 and rank.shape == (prob.n, M, 4)
    rows = search_targets_cpu(prob, ts, sem)
    assert np.array_equal(rank, rank_model(rows, M)), (M, sem)
    alone = [as_triples(search_cpu(Problem(prob.weights, ts.target(t), prob.codes, prob.offsets), sem))
             for t in range(ts.T)]
    F = fitting(prob, ts)
    for i in range(prob.n):
        listed = rank[i, :, 0]
        assert (listed[:min(M, F[i])] >= 0).all() and (rank[i, min(M, F[i]):] == PAD).all(), (i, F[i])
        for j in range(min(M, int(F[i]))):
            assert rank[i, j, 1:].tolist() == alone[listed[j]][i].tolist(), (i, j)
    return rank


# ---- against the model -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("seed", range(6))
def test_random_problems_equal_the_sorted_pair_rows(sem, seed):
    rng = np.random.default_rng(seed)
    T, n = int(rng.integers(1, 40)), int(rng.integers(1, 9))
    prob, ts = random_case(100 + seed, rng.integers(1, 16, T), rng.integers(1, 14, n), alphabet=int(rng.integers(1, 5)))
    for M in sorted({1, 3, T, min(T + 1, 64), 64}):
        check_rank(prob, ts, M, sem)


@pytest.mark.parametrize("sem", SEMS)
def test_straddling_record(sem):
    """On the catalog the record matches fully at offset 40, a placement in neither target: no rank row has it."""
    prob, ts = straddling_case()
    rank = check_rank(prob, ts, 2, sem)
    assert 160 not in rank[:, :, 1] and sorted(rank[0, :, 0].tolist()) == [0, 1]
    assert (rank[:, :, 2] + 40 <= 60).all()  # n + L2 <= len_t


# ---- relations -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_row_0_is_targets_best(sem):
    prob, ts = random_case(7, [5, 9, 1, 9, 30, 2], [1, 2, 5, 9, 10, 31, 3])
    rank = search_targets_rank_cpu(prob, ts, 3, sem)
    t, row = targets_best(search_targets_cpu(prob, ts, sem))
    assert np.array_equal(rank[:, 0, 0], t) and np.array_equal(rank[:, 0, 1:], row)
    assert -1 in t  # the record of 31 letters fits nothing: both say (-1, INT32_MIN, 0, 0)


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("T,M", [(8, 3), (63, 63), (64, 64), (65, 64), (65, 2), (5, 1)])
def test_m_around_the_fitting_targets(sem, T, M):
    """Records with 0, 1, M - 1, M, M + 1 and T fitting targets: M = F - 1, F and F + 1 all occur; then M = 1 and 64."""
    prob, ts, counts = around_m_case(T, M)
    rank = check_rank(prob, ts, M, sem)
    assert ((rank[:, :, 0] >= 0).sum(axis=1) == np.minimum(counts, M)).all()
    check_rank(prob, ts, 1, sem)
    full = check_rank(prob, ts, 64, sem)
    assert np.array_equal(full[:, :M], rank)  # a smaller M is a prefix


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("i", [1, 3, 6])
def test_one_target_is_the_search_with_a_leading_0(sem, i):
    prob = Problem.read(input_path(i))
    rank = search_targets_rank_cpu(prob, [0, prob.L1], 1, sem)
    res = as_triples(search_cpu(prob, sem))
    fit = res[:, 0] != I32.min
    assert np.array_equal(rank[fit, 0, 1:], res[fit]) and (rank[fit, 0, 0] == 0).all()
    assert (rank[~fit, 0] == PAD).all()
    two = search_targets_rank_cpu(prob, [0, prob.L1], 2, sem)
    assert np.array_equal(two[:, 0], rank[:, 0]) and (two[:, 1] == PAD).all()


@pytest.mark.parametrize("sem", SEMS)
def test_a_record_longer_than_every_target(sem):
    prob, ts = random_case(3, [4, 6, 2], [7, 3, 12])
    rank = check_rank(prob, ts, 4, sem)
    assert (rank[0] == PAD).all() and (rank[2] == PAD).all() and (rank[1, :2, 0] >= 0).all() and (rank[1, 2:] == PAD).all()


@pytest.mark.parametrize("sem", SEMS)
def test_identical_targets_list_in_ascending_order(sem):
    rng = np.random.default_rng(5)
    one = rng.integers(1, 5, 9)
    ts = TargetSet.from_sequences([one] * 70)
    codes, offsets = batch_of([one[2:6], one, rng.integers(1, 5, 3)])
    prob = Problem(list(W), ts.seq1, codes, offsets)
    rank = check_rank(prob, ts, 64, sem)
    assert (rank[:, :, 0] == np.arange(64)[None, :]).all()
    assert (rank[:, :, 1:] == rank[:, :1, 1:]).all()  # one row, 64 times


@pytest.mark.parametrize("sem", SEMS)
def test_two_different_targets_that_tie(sem):
    """Four different targets hold the record AB at different places, away from their last offset so that both
    semantics see the match, and tie on its score; one between them scores lower: the order is score, then index."""
    ts = TargetSet.from_strings(["ABQQ", "QABQ", "QQQQ", "ABAB", "QQABQ"])
    codes, offsets = batch_of([TargetSet.from_strings(["AB"]).seq1])
    prob = Problem(list(W), ts.seq1, codes, offsets)
    rank = check_rank(prob, ts, 5, sem)
    assert rank[0, :, 1].tolist() == sorted(rank[0, :, 1].tolist(), reverse=True)
    assert len(set(rank[0, :4, 1].tolist())) == 1  # four targets tie on the full match
    assert rank[0, :4, 0].tolist() == [0, 1, 3, 4] and rank[0, 4, 0] == 2
    assert rank[0, 0, 2] != rank[0, 1, 2]  # at different offsets


# ---- catalog rows ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_catalog_rows_against_a_loop_and_through_the_report(sem):
    prob, ts = random_case(11, [5, 9, 1, 9, 30, 2], [1, 2, 5, 9, 10, 31, 3])
    M = 4
    rank = search_targets_rank_cpu(prob, ts, M, sem)
    cat = targets_rank_catalog_rows(rank, ts)
    assert cat.dtype == np.int32 and cat.shape == (prob.n, M, 3)
    for i in range(prob.n):
        for j in range(M):
            t, s, n, k = rank[i, j].tolist()
            assert cat[i, j].tolist() == ([I32.min, 0, 0] if t < 0 else [s, n + int(ts.starts[t]), k])
    assert np.array_equal(targets_rank_catalog_rows(rank, ts.starts), cat)
    scores = report_scores(search_report_cpu(prob, cat), prob.weights)
    real = rank[:, :, 0] >= 0
    assert real.any() and not real.all()
    assert np.array_equal(scores[real], rank[:, :, 1][real].astype(np.int64))  # the counts reproduce the scores
    assert (scores[~real] == REPORT_EMPTY).all()
    with pytest.raises(ValueError):
        targets_rank_catalog_rows(rank[:, :, :3], ts)
    with pytest.raises(ValueError):
        targets_rank_catalog_rows(rank, ts.starts[:3])  # a target index past the set


def test_catalog_rows_on_a_torch_tensor():
    torch = pytest.importorskip("torch")
    prob, ts = random_case(12, [5, 9, 1, 30], [1, 2, 5, 31])
    rank = search_targets_rank_cpu(prob, ts, 3)
    got = targets_rank_catalog_rows(torch.from_numpy(rank), ts)
    assert got.dtype == torch.int32 and np.array_equal(got.numpy(), targets_rank_catalog_rows(rank, ts))


# ---- the chunk cut -------------------------------------------------------------------------------------------------
def test_chunks_hand_list():
    assert targets_rank_geometry()[0] == 12 and RANK_COLS == ("target", "score", "n", "k")
    L1, T = 30, 4
    offsets = np.arange(0, 50, 10, dtype=np.int64) + 7  # four records of 10 letters; any first offset
    ref, spec = Semantics.REFERENCE, Semantics.SPEC
    assert entries_of(L1, 10, ref) == 20 and entries_of(L1, 10, spec) == 21
    one = 8 * 20 + 12 * T  # a record's cost: 208 bytes
    hand = [(2 * one, ref, [0, 2, 4]),          # exactly two records' cost
            (2 * one - 1, ref, [0, 1, 2, 3, 4]),  # one byte less
            (12 * T - 8, ref, [0, 1, 2, 3, 4]),   # below 12 T: every record alone, over the budget
            (100, ref, [0, 1, 2, 3, 4]),          # below one record's entries
            (4 * one, ref, [0, 4]), (4 * one - 1, ref, [0, 3, 4]),
            (2 * one, spec, [0, 1, 2, 3, 4]), (2 * one + 16, spec, [0, 2, 4])]
    for scratch, sem, want in hand:
        got = targets_rank_chunks(L1, offsets, T, scratch, sem)
        assert got.dtype == np.int64 and got.tolist() == want == chunks_model(L1, [10] * 4, T, scratch, sem), (scratch, sem)
    # record_bytes = 0 (T = 0) is the cut of top-K and hits: records while entries <= max(1, scratch // 8)
    for scratch, want in ((8 * 40, [0, 2, 4]), (8 * 40 - 1, [0, 1, 2, 3, 4]), (8 * 60 + 7, [0, 3, 4]), (8, [0, 1, 2, 3, 4])):
        assert targets_rank_chunks(L1, offsets, 0, scratch).tolist() == want == chunks_model(L1, [10] * 4, 0, scratch, ref)
    # records longer than the catalog have no entries, only pair rows
    long = np.arange(0, 60, 10, dtype=np.int64)
    assert targets_rank_chunks(8, long, T, 96).tolist() == [0, 2, 4, 5]
    assert targets_rank_chunks(8, long, 0, 96).tolist() == [0, 5]
    assert targets_rank_chunks(L1, np.zeros(1, np.int64), T, 96).tolist() == [0]
    with pytest.raises(_lib.NativeError, match="profile scratch"):
        targets_rank_chunks(L1, offsets, T, 7)


@pytest.mark.parametrize("seed", range(8))
def test_chunks_seeded_sweep(seed):
    rng = np.random.default_rng(seed)
    for _ in range(40):
        L1 = int(rng.integers(1, 80))
        lens = np.where(rng.random(int(rng.integers(1, 50))) < 0.1, L1 + rng.integers(0, 3), rng.integers(1, min(L1, 40) + 1))
        lens = np.atleast_1d(lens).astype(np.int64)
        offsets = np.concatenate([[3], 3 + np.cumsum(lens)]).astype(np.int64)
        T = int(rng.choice([0, 1, 3, 17, 4096]))
        scratch = int(rng.integers(8, 12 * max(T, 1) * 6 + 8 * 200))
        sem = SEMS[int(rng.integers(2))]
        got = targets_rank_chunks(L1, offsets, T, scratch, sem).tolist()
        assert got == chunks_model(L1, lens.tolist(), T, scratch, sem), (L1, lens.tolist(), T, scratch, sem)


# ---- errors --------------------------------------------------------------------------------------------------
def test_error_paths_and_their_order():
    prob, ts = random_case(31, [4, 7, 3], [2, 5, 3])
    bad_starts = [ts.starts[:-1], ts.starts + 1, np.zeros(0, np.int64), np.concatenate([ts.starts[:2], ts.starts[1:]])]
    for starts in bad_starts:
        for M in (0, 2, 65):
            with pytest.raises(ValueError, match="^targets:"):
                search_targets_rank_cpu(prob, starts, M)  # the target set's error comes before M's
    for M in (0, 65, -3):
        with pytest.raises(ValueError, match=r"^rank: M must be in 1\.\.64"):
            search_targets_rank_cpu(prob, ts, M)
    # the C ABI states the same order
    bad = np.ascontiguousarray(ts.starts + 1)
    out = np.zeros((prob.n, 64, 4), np.int32)

    def call(starts, M):
        rc = _lib.lib().moc_cpu_targets_rank(_lib.weights_arg(prob.weights.as_list()), _lib.ptr(prob.seq1), prob.L1,
                                             _lib.ptr(prob.codes), _lib.ptr(prob.offsets), prob.n, _lib.ptr(starts),
                                             starts.shape[0] - 1, 0, 0, M, _lib.ptr(out))
        return rc, _lib.lib().moc_last_error().decode()

    rc, msg = call(bad, 0)
    assert rc != 0 and msg.startswith("targets:")
    rc, msg = call(ts.starts, 0)
    assert rc != 0 and msg.startswith("rank:")
    rc, msg = call(ts.starts, 65)
    assert rc != 0 and msg.startswith("rank:") and not out.any()
    assert call(ts.starts, 64)[0] == 0 and np.array_equal(out, search_targets_rank_cpu(prob, ts, 64))
    assert _lib.lib().moc_abi_version() == 1


# ---- the formatter -----------------------------------------------------------------------------------------------
def test_formatter():
    ts = TargetSet.from_strings(["ABAB", "QQAB", "A"])
    recs = TargetSet.from_strings(["AB", "QQABA"])
    codes, offsets = batch_of([recs.target(0), recs.target(1)])
    prob = Problem(list(W), ts.seq1, codes, offsets)
    rows = search_targets_cpu(prob, ts, Semantics.SPEC)
    rank = search_targets_rank_cpu(prob, ts, 3, Semantics.SPEC)
    text = format_targets_rank(rows[:, 0], rank)
    assert text.splitlines() == [
        "#0: score: 8, n: 0, k: 0", "  best 1: target 1: score: 8, n: 0, k: 0", "  best 2: target 2: score: 8, n: 2, k: 0",
        f"#1: score: {I32.min}, n: 0, k: 0", "  best: none"]
    assert format_targets_rank(rows[:, 0], rank, first_index=5).startswith("#5: ")
    with pytest.raises(ValueError):
        format_targets_rank(rows[:, 0], rows)
    with pytest.raises(ValueError):
        format_targets_rank(rows[:1, 0], rank)


# ---- the CLI ---------------------------------------------------------------------------------------------------
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
    return str(path), ts, Problem(prob.weights, ts.seq1, prob.codes, prob.offsets)


def want_best(prob, catalog, ts, M):
    return format_targets_rank(as_triples(search_cpu(prob)), search_targets_rank_cpu(catalog, ts, M))


@pytest.mark.parametrize("i", [1, 6])
def test_cli_target_best(tmp_path, i):
    prob = Problem.read(input_path(i))
    path, ts, catalog = cli_targets_file(tmp_path, prob)
    for M in (1, 3, 64):
        r = _cli(["--targets", path, "--target-best", str(M)], i)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        out = r.stdout.decode()
        assert out == want_best(prob, catalog, ts, M), M
        assert "".join(l + "\n" for l in out.splitlines() if not l.startswith("  ")) == expected(i)  # unchanged lines
        under = [l for l in out.splitlines() if l.startswith("  ")]
        assert under and all(l.startswith("  best") for l in under) and not any("  target " == l[:9] for l in under)
    assert any(l.startswith("  best 2: target ") for l in out.splitlines())
    plain = _cli(["--targets", path], i)  # without the flag: today's output
    rows = search_targets_cpu(catalog, ts)
    assert plain.returncode == 0 and plain.stdout.decode() == format_targets(rows[:, 0], rows)


def test_cli_target_best_none_line(tmp_path):
    """A record longer than Seq1 and than the file's target fits nothing: its own line, then "  best: none"."""
    path = tmp_path / "in.txt"
    path.write_text("4 3 2 10\nABC\n2\nABCDE\nAB\n")
    tpath = tmp_path / "t.txt"
    tpath.write_text("QAB\n")
    with open(path, "rb") as f:
        r = subprocess.run([sys.executable, "-m", "mpi_openmp_cuda_amd", "--backend=cpu", "--targets", str(tpath),
                            "--target-best", "2"], stdin=f, capture_output=True, env=dict(os.environ, PYTHONPATH=ROOT),
                           cwd="/tmp", timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = r.stdout.decode().splitlines()
    assert lines[1] == "  best: none" and lines[3].startswith("  best 1: target ") and lines[4].startswith("  best 2: target ")
    assert len(lines) == 5


def test_cli_target_best_two_gloo_ranks(tmp_path):
    prob = Problem.read(input_path(3))
    path, ts, catalog = cli_targets_file(tmp_path, prob)
    r = torchrun(2, ["--backend=cpu", "--dist-backend=gloo", "--targets", path, f"--input={input_path(3)}",
                     "--target-best", "3"])
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert r.stdout.decode() == want_best(prob, catalog, ts, 3)


@pytest.mark.parametrize("args", [
    ["--target-best", "2"],  # needs --targets
    ["--targets", "FILE", "--target-best", "0"], ["--targets", "FILE", "--target-best", "65"],
    ["--targets", "FILE", "--target-best", "2", "--target-top", "2"],
    ["--targets", "FILE", "--target-best", "2", "--target-min-score", "0"],
    ["--targets", "FILE", "--target-best", "2", "--target-within", "0"],
    ["--targets", "FILE", "--target-best", "2", "--target-summary"],
    ["--targets", "FILE", "--target-best", "2", "--target-summary", "--target-hist", "0:1:4"],
    ["--targets", "FILE", "--target-best", "2", "--target-hist", "0:1:4"],
    ["--targets", "FILE", "--target-best", "2", "--target-distinct", "1"],
    ["--targets", "FILE", "--target-best", "2", "--target-top", "2", "--target-distinct", "1"],
    ["--targets", "FILE", "--target-best", "2", "--top", "2"],  # everything --targets refuses stays refused
    ["--targets", "FILE", "--target-best", "2", "--min-score", "0"],
    ["--targets", "FILE", "--target-best", "2", "--within", "1"],
    ["--targets", "FILE", "--target-best", "2", "--show-alignment"],
    ["--targets", "FILE", "--target-best", "2", "--summary"],
    ["--targets", "FILE", "--target-best", "2", "--partition", "offsets"]])
def test_cli_refusals(tmp_path, args):
    prob = Problem.read(input_path(6))
    path, _, _ = cli_targets_file(tmp_path, prob)
    r = _cli([path if a == "FILE" else a for a in args], 6)
    assert r.returncode != 0 and r.stdout == b"" and r.stderr != b""


def test_distributed_search_on_one_process_and_errors():
    from mpi_openmp_cuda_amd.parallel import dist as D
    from mpi_openmp_cuda_amd.parallel.search import DistributedSearch

    prob, ts = random_case(37, [4, 9, 2, 9, 6], [3, 1, 9, 10, 5])
    s = DistributedSearch(D.DistContext(), backend="cpu", partition="records")
    rank = s.run_targets_rank(prob, ts, 3, Semantics.SPEC)
    assert rank.dtype == np.int32 and np.array_equal(rank, search_targets_rank_cpu(prob, ts, 3, Semantics.SPEC))
    with pytest.raises(ValueError, match="^targets:"):
        s.run_targets_rank(prob, ts.starts[:-1], 0)
    with pytest.raises(ValueError, match="^rank:"):
        s.run_targets_rank(prob, ts, 65)
    s = DistributedSearch(D.DistContext(), backend="cpu", partition="offsets")
    with pytest.raises(ValueError, match="record slices"):
        s.run_targets_rank(prob, ts, 2)


# ---- stand-alone sanitizer program -------------------------------------------------------------------------
def test_targets_rank_sanitizer_program():
    """csrc/tests/targets_rank_san.cpp with the CPU core sources under ASan + UBSan: a plain program with its own main
    (nothing is loaded into Python, nothing runs on a GPU)."""
    r = subprocess.run(["make", "-C", ROOT, "-s", "-j8", "targets-rank-san"], capture_output=True, timeout=600)
    out = (r.stdout + r.stderr).decode()
    assert r.returncode == 0, out[-3000:]
    assert "targets_rank_san ok" in out and "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]
