"""Per-target top-K and threshold hits on the CPU engine (csrc/src/cpu_engine.cpp targets_topk_batch_cpu /
targets_hits_batch_cpu). The oracle for everything is the existing search_topk_cpu / search_hits_cpu run once per
target on Problem(weights, target_t, codes, offsets) — functions that never see the catalog. Covered: random problems
under both semantics with target lengths around every record length (pairs that do not fit, len == L2, one-letter
targets), K = 1 against search_targets_cpu, T = 1 against top-K and hits themselves, INT32_MIN against the per-target
profile, the straddling record, ties, the C ABI's capacity contract over poisoned buffers, `within` against thresholds
built by hand, every error path and its prefix, the formatters, the three CLI flags at one and two gloo ranks with
their refusals, DistributedSearch on one process, and the stand-alone sanitizer program."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, expected, input_path
from test_dist import torchrun

from mpi_openmp_cuda_amd import (Problem, Semantics, TargetSet, _lib, format_targets, format_targets_hits,
                                 format_targets_topk, search_hits_cpu, search_profile_cpu, search_targets_cpu,
                                 search_targets_hits_cpu, search_targets_topk_cpu, search_topk_cpu)

SEMS = [Semantics.REFERENCE, Semantics.SPEC]
I32 = np.iinfo(np.int32)
NONE = [I32.min, 0, 0]


def batch_of(recs):
    lens = np.array([len(r) for r in recs], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    codes = np.concatenate([np.asarray(r, np.uint8) for r in recs]) if len(recs) else np.zeros(0, np.uint8)
    return codes, offsets


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


def pair_hits(rows, toffsets, T, i, t):
    p = i * T + t
    return rows[toffsets[p]:toffsets[p + 1]]


def check_against_targets_alone(w, ts, codes, offsets, sem, K, **thr):
    """Top-K and hits of the catalog against search_topk_cpu / search_hits_cpu run on every target alone."""
    n = offsets.shape[0] - 1
    catalog = Problem(w, ts.seq1, codes, offsets)
    topk = search_targets_topk_cpu(catalog, ts, K, sem)
    assert topk.dtype == np.int32 and topk.shape == (n, ts.T, K, 3)
    rows, toffsets = search_targets_hits_cpu(catalog, ts, semantics=sem, **thr)
    assert toffsets.dtype == np.int64 and toffsets.shape == (n * ts.T + 1,) and toffsets[0] == 0
    assert rows.dtype == np.int32 and rows.shape == (toffsets[-1], 3)
    for t in range(ts.T):
        alone = Problem(w, ts.target(t), codes, offsets)
        assert np.array_equal(topk[:, t], search_topk_cpu(alone, K, sem)), (t, "top-K")
        sub = dict(thr)
        if "thresholds" in sub:  # [n, T]: the target's column; [n]: every target's
            th = np.asarray(thr["thresholds"])
            sub["thresholds"] = th[:, t] if th.ndim == 2 else th
        want, h = search_hits_cpu(alone, semantics=sem, **sub)
        for i in range(n):
            assert np.array_equal(pair_hits(rows, toffsets, ts.T, i, t), want[h[i]:h[i + 1]]), (i, t, "hits")
    return topk, rows, toffsets


# ---- against the per-target oracle -------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("seed", range(6))
def test_random_problems_equal_per_target_topk_and_hits(sem, seed):
    rng = np.random.default_rng(300 + seed)
    ts, recs = random_case(rng, 6, (2, 3, 4, 6, 12, 26)[seed])
    codes, offsets = batch_of(recs)
    w = [int(x) for x in rng.integers(0, 15, size=4)]
    K = (1, 2, 5, 17, 63, 64)[seed]
    L2 = np.diff(offsets)
    fits = L2[:, None] <= ts.lengths[None, :]
    assert fits.any() and not fits.all() and (L2[:, None] == ts.lengths[None, :]).any() and 1 in ts.lengths
    topk, rows, toffsets = check_against_targets_alone(w, ts, codes, offsets, sem, K, min_score=int(rng.integers(-40, 10)))
    assert (topk[~fits] == NONE).all() and (np.diff(toffsets).reshape(fits.shape)[~fits] == 0).all()
    check_against_targets_alone(w, ts, codes, offsets, sem, K, within=int(rng.integers(0, 12)))
    per_pair = rng.integers(-40, 10, size=fits.shape).astype(np.int32)
    check_against_targets_alone(w, ts, codes, offsets, sem, K, thresholds=per_pair)
    per_record = rng.integers(-40, 10, size=len(recs)).astype(np.int32)
    check_against_targets_alone(w, ts, codes, offsets, sem, K, thresholds=per_record)  # [n], broadcast over targets
    catalog = Problem(w, ts.seq1, codes, offsets)
    for threads in (1, 3):
        assert np.array_equal(search_targets_topk_cpu(catalog, ts.starts, K, sem, threads), topk)


@pytest.mark.parametrize("sem", SEMS)
def test_k_1_is_the_multi_target_search(sem):
    rng = np.random.default_rng(7)
    ts, recs = random_case(rng, 8, 4)
    codes, offsets = batch_of(recs)
    catalog = Problem([4, 3, 2, 10], ts.seq1, codes, offsets)
    assert np.array_equal(search_targets_topk_cpu(catalog, ts, 1, sem)[:, :, 0], search_targets_cpu(catalog, ts, sem))
    assert np.array_equal(search_targets_topk_cpu(catalog, ts, 9, sem)[:, :, 0], search_targets_cpu(catalog, ts, sem))


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("i", [1, 3, 6])
def test_one_target_is_topk_and_hits_on_the_goldens(sem, i):
    prob = Problem.read(input_path(i))
    topk = search_targets_topk_cpu(prob, [0, prob.L1], 4, sem)
    assert np.array_equal(topk[:, 0], search_topk_cpu(prob, 4, sem))
    rows, toffsets = search_targets_hits_cpu(prob, [0, prob.L1], within=20, semantics=sem)
    want, h = search_hits_cpu(prob, within=20, semantics=sem)
    assert np.array_equal(toffsets, h) and np.array_equal(rows, want)


@pytest.mark.parametrize("sem", SEMS)
def test_int32_min_selects_the_per_target_profile(sem):
    rng = np.random.default_rng(17)
    ts, recs = random_case(rng, 5, 4)
    codes, offsets = batch_of(recs)
    w = [4, 3, 2, 10]
    rows, toffsets = search_targets_hits_cpu(Problem(w, ts.seq1, codes, offsets), ts, min_score=int(I32.min), semantics=sem)
    for t in range(ts.T):
        prof, poff = search_profile_cpu(Problem(w, ts.target(t), codes, offsets), sem)
        for i in range(len(recs)):
            mine, p = pair_hits(rows, toffsets, ts.T, i, t), prof[poff[i]:poff[i + 1]]
            assert np.array_equal(mine[:, 0], p["score"]) and np.array_equal(mine[:, 2], p["k"])
            assert np.array_equal(mine[:, 1], np.arange(len(p)))


# ---- the straddling case -----------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_straddling_record(sem):
    """The last 20 letters of target 1 followed by the first 20 of target 2: on the catalog a full match at offset 40,
    a placement in neither target. No per-target row reaches past its target's end."""
    rng = np.random.default_rng(2024)
    t1, t2 = (rng.integers(1, 27, size=60).astype(np.uint8) for _ in range(2))
    ts = TargetSet.from_sequences([t1, t2])
    codes, offsets = batch_of([np.concatenate([t1[40:], t2[:20]])])
    w = [4, 3, 2, 10]
    catalog = Problem(w, ts.seq1, codes, offsets)
    trap = search_topk_cpu(catalog, 1, sem)[0, 0]
    assert trap.tolist() == [160, 40, 0]
    topk, rows, toffsets = check_against_targets_alone(w, ts, codes, offsets, sem, 64, min_score=int(I32.min))
    real = topk[:, :, :, 0] != I32.min
    assert 160 not in topk[:, :, :, 0] and 160 not in rows[:, 0]
    assert (topk[:, :, :, 1][real] + 40 <= 60).all() and (rows[:, 1] + 40 <= 60).all()  # n + L2 <= len_t
    assert real.sum() == 2 * (20 + (1 if sem == Semantics.SPEC else 0)) == rows.shape[0]


# ---- ties ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_equal_scores_keep_ascending_offsets(sem):
    ts = TargetSet.from_sequences([np.full(l, 7, np.uint8) for l in (9, 4, 5)])
    codes, offsets = batch_of([np.full(4, 7, np.uint8)])
    w = [5, 1, 2, 3]
    topk, rows, toffsets = check_against_targets_alone(w, ts, codes, offsets, sem, 8, min_score=20)
    spec = 1 if sem == Semantics.SPEC else 0
    for t, length in enumerate((9, 4, 5)):
        c = 1 if length == 4 else length - 4 + spec
        want = [[20, o, 0] for o in range(c)] + [NONE] * (8 - c)
        assert topk[0, t].tolist() == want
        assert pair_hits(rows, toffsets, 3, 0, t).tolist() == want[:c]  # inclusive at exact equality
    none, toffsets = search_targets_hits_cpu(Problem(w, ts.seq1, codes, offsets), ts, min_score=21, semantics=sem)
    assert none.shape == (0, 3) and not toffsets.any()


def test_boundary_entry_that_ties_a_slice_entry_ranks_behind_it():
    # target ABAB, record AB: un-mutated offsets 0 and 2 both match fully; offset 2 is the target's boundary entry
    ts = TargetSet.from_strings(["ABAB", "QQAB"])
    rec = TargetSet.from_strings(["AB"]).seq1
    codes, offsets = batch_of([rec])
    w = [4, 3, 2, 10]
    topk, rows, toffsets = check_against_targets_alone(w, ts, codes, offsets, Semantics.SPEC, 3, min_score=8)
    assert topk[0, 0, :2].tolist() == [[8, 0, 0], [8, 2, 0]]
    assert topk[0, 1, 0].tolist() == [8, 2, 0]  # only the boundary entry matches
    assert pair_hits(rows, toffsets, 2, 0, 0).tolist() == [[8, 0, 0], [8, 2, 0]]
    assert pair_hits(rows, toffsets, 2, 0, 1).tolist() == [[8, 2, 0]]
    topk, rows, toffsets = check_against_targets_alone(w, ts, codes, offsets, Semantics.REFERENCE, 3, min_score=8)
    assert topk[0, 0, 0].tolist() == [8, 0, 0] and 2 not in topk[0, :, :, 1]  # no final offset under reference
    assert toffsets.tolist() == [0, 1, 1]


@pytest.mark.parametrize("sem", SEMS)
def test_a_threshold_only_the_boundary_entry_reaches(sem):
    """The GPU test's threshold case on the CPU engine: the record is the last letters of target 0 (spec's final
    offset) and the whole of target 1 (len == L2 under both semantics)."""
    rng = np.random.default_rng(91)
    rec = rng.integers(1, 27, 9).astype(np.uint8)
    t0 = np.concatenate([rng.integers(1, 27, 23).astype(np.uint8), rec])
    t0[22] = rec[0] % 26 + 1
    ts = TargetSet.from_sequences([t0, rec, rng.integers(1, 27, 40).astype(np.uint8)])
    codes, offsets = batch_of([rec, rng.integers(1, 27, 4).astype(np.uint8)])
    rows, toffsets = search_targets_hits_cpu(Problem([4, 3, 2, 10], ts.seq1, codes, offsets), ts, min_score=36, semantics=sem)
    want = ([[36, 23, 0]] if sem == Semantics.SPEC else []) + [[36, 0, 0]]
    assert rows.tolist() == want and toffsets.tolist() == [0, len(want) - 1, len(want)] + [len(want)] * 4


# ---- the C ABI's capacity contract -----------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_capacity_contract_over_poisoned_buffers(sem):
    rng = np.random.default_rng(23)
    ts, recs = random_case(rng, 4, 3)
    codes, offsets = batch_of(recs)
    prob = Problem([4, 3, 2, 10], ts.seq1, codes, offsets)
    want, woff = search_targets_hits_cpu(prob, ts, min_score=-12, semantics=sem)
    total = int(woff[-1])
    inside = next(int(woff[p]) + 1 for p in range(len(woff) - 1) if woff[p + 1] - woff[p] >= 3)
    edge = next(int(woff[p + 1]) for p in range(len(woff) - 1) if woff[p + 1] > woff[p] and woff[p + 1] < total)
    assert total >= 8 and 0 < inside < total and 0 < edge < total
    POISON = -777
    for cap in (0, 1, inside, edge - 1, edge, total - 1, total):
        rows = np.full((total + 8, 3), POISON, np.int32)
        toffsets = np.full(prob.n * ts.T + 1, POISON, np.int64)
        rc = _lib.lib().moc_cpu_targets_hits(
            _lib.weights_arg(prob.weights.as_list()), _lib.ptr(prob.seq1), prob.L1, _lib.ptr(prob.codes),
            _lib.ptr(prob.offsets), prob.n, _lib.ptr(ts.starts), ts.T, int(sem), 0, -12, None, _lib.ptr(toffsets),
            _lib.ptr(rows) if cap else None, cap)
        assert rc == 0
        assert np.array_equal(toffsets, woff), cap  # complete and exact whatever the capacity
        assert np.array_equal(rows[:cap], want[:cap]) and (rows[cap:] == POISON).all(), cap


# ---- within ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_within_is_each_pairs_own_best_minus_d(sem):
    rng = np.random.default_rng(29)
    ts, recs = random_case(rng, 5, 4)
    codes, offsets = batch_of(recs)
    prob = Problem([4, 3, 2, 10], ts.seq1, codes, offsets)
    best = search_targets_cpu(prob, ts, sem)[:, :, 0].astype(np.int64)
    for D in (0, 7, 2 ** 31 - 1):
        by_hand = np.clip(best - D, I32.min, I32.max).astype(np.int32)
        want, woff = search_targets_hits_cpu(prob, ts, thresholds=by_hand, semantics=sem)
        rows, toffsets = search_targets_hits_cpu(prob, ts, within=D, semantics=sem)
        assert np.array_equal(toffsets, woff) and np.array_equal(rows, want)
        fits = best != I32.min
        assert (np.diff(toffsets).reshape(fits.shape)[fits] >= 1).all()  # the best entry itself always qualifies


# ---- errors --------------------------------------------------------------------------------------------------
def test_error_paths_and_their_prefixes():
    rng = np.random.default_rng(31)
    ts, recs = random_case(rng, 3, 4)
    codes, offsets = batch_of(recs)
    prob = Problem([4, 3, 2, 10], ts.seq1, codes, offsets)
    bad_starts = [ts.starts[:-1], ts.starts + 1, np.zeros(0, np.int64), np.concatenate([ts.starts[:2], ts.starts[1:]])]
    for starts in bad_starts:
        with pytest.raises(ValueError, match="^targets:"):
            search_targets_topk_cpu(prob, starts, 0)  # the target set's error comes before K's
        with pytest.raises(ValueError, match="^targets:"):
            search_targets_hits_cpu(prob, starts)  # ... and before the thresholds'
    for K in (0, 65, -3):
        with pytest.raises(ValueError, match=r"^top-K: K must be in 1\.\.64"):
            search_targets_topk_cpu(prob, ts, K)
    for kw in ({}, {"min_score": 0, "within": 1}, {"min_score": 0, "thresholds": np.zeros((3, ts.T), np.int32)}):
        with pytest.raises(ValueError, match="^hits: give exactly one of min_score, thresholds, within"):
            search_targets_hits_cpu(prob, ts, **kw)
    with pytest.raises(ValueError, match="^hits: min_score .* is not an int32"):
        search_targets_hits_cpu(prob, ts, min_score=2 ** 31)
    with pytest.raises(ValueError, match="^hits: within must be >= 0"):
        search_targets_hits_cpu(prob, ts, within=-1)
    for t in (np.zeros((3, ts.T + 1), np.int32), np.zeros(4, np.int32), np.zeros((3, ts.T), np.float64),
              np.zeros((ts.T, 3), np.int32)):
        with pytest.raises(ValueError, match="^hits: thresholds must be"):
            search_targets_hits_cpu(prob, ts, thresholds=t)
    with pytest.raises(ValueError, match="^hits: thresholds must fit int32"):
        search_targets_hits_cpu(prob, ts, thresholds=np.full((3, ts.T), 2 ** 31, np.int64))
    # the C ABI: K and the buffers
    head = (_lib.weights_arg(prob.weights.as_list()), _lib.ptr(prob.seq1), prob.L1, _lib.ptr(prob.codes),
            _lib.ptr(prob.offsets), prob.n, _lib.ptr(ts.starts), ts.T, 0, 0)
    toffsets = np.zeros(prob.n * ts.T + 1, np.int64)
    assert _lib.lib().moc_cpu_targets_topk(*head, 0, None) != 0
    assert _lib.lib().moc_last_error().decode().startswith("top-K:")
    assert _lib.lib().moc_cpu_targets_hits(*head, 0, None, _lib.ptr(toffsets), None, 5) != 0
    assert _lib.lib().moc_last_error().decode().startswith("hits:")
    assert _lib.lib().moc_abi_version() == 1


# ---- formatters ----------------------------------------------------------------------------------------------
def test_formatters():
    ts = TargetSet.from_strings(["ABAB", "QQAB", "A"])
    recs = TargetSet.from_strings(["AB", "QQABA"])
    codes, offsets = batch_of([recs.target(0), recs.target(1)])
    prob = Problem([4, 3, 2, 10], ts.seq1, codes, offsets)
    rows = search_targets_cpu(prob, ts, Semantics.SPEC)
    plain = format_targets(rows[:, 0], rows)
    topk = search_targets_topk_cpu(prob, ts, 3, Semantics.SPEC)
    text = format_targets_topk(topk[:, 0, 0], topk)
    assert "".join(l + "\n" for l in text.splitlines() if not l.startswith("    ")) == plain
    lines = text.splitlines()
    assert lines[:4] == ["#0: score: 8, n: 0, k: 0", "  target 1: score: 8, n: 0, k: 0", "    top 2: score: 8, n: 2, k: 0",
                         f"    top 3: score: {topk[0, 0, 2, 0]}, n: {topk[0, 0, 2, 1]}, k: {topk[0, 0, 2, 2]}"]
    assert "  target 3: none" in lines and not any("-2147483648" in l for l in lines if l.startswith("    "))
    assert format_targets_topk(rows[:, 0], topk[:, :, :1]) == plain  # K = 1: no rank lines
    hits, toffsets = search_targets_hits_cpu(prob, ts, min_score=8, semantics=Semantics.SPEC)
    text = format_targets_hits(rows[:, 0], rows, hits, toffsets)
    assert "".join(l + "\n" for l in text.splitlines() if not l.startswith("    ")) == plain
    assert text.splitlines()[:4] == ["#0: score: 8, n: 0, k: 0", "  target 1: score: 8, n: 0, k: 0",
                                     "    hit: score: 8, n: 0, k: 0", "    hit: score: 8, n: 2, k: 0"]
    assert sum(l.startswith("    hit: ") for l in text.splitlines()) == hits.shape[0]
    with pytest.raises(ValueError):
        format_targets_topk(rows[:, 0], rows)
    with pytest.raises(ValueError):
        format_targets_hits(rows[:, 0], rows, hits, toffsets[:-1])
    with pytest.raises(ValueError):
        format_targets_hits(rows[:, 0], topk, hits, toffsets)


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


def want_topk(catalog, ts, K):
    topk = search_targets_topk_cpu(catalog, ts, K)
    return format_targets_topk(topk[:, 0, 0], topk)


def want_hits(catalog, ts, **thr):
    rows = search_targets_cpu(catalog, ts)
    return format_targets_hits(rows[:, 0], rows, *search_targets_hits_cpu(catalog, ts, **thr))


@pytest.mark.parametrize("i", [1, 6])
def test_cli_target_flags(tmp_path, i):
    prob = Problem.read(input_path(i))
    path, ts, catalog = cli_targets_file(tmp_path, prob)
    plain = _cli(["--targets", path], i)
    rows = search_targets_cpu(catalog, ts)
    assert plain.returncode == 0 and plain.stdout.decode() == format_targets(rows[:, 0], rows)  # today's output
    for args, want in ((["--target-top", "3"], want_topk(catalog, ts, 3)),
                       (["--target-within", "20"], want_hits(catalog, ts, within=20)),
                       (["--target-min-score=-5"], want_hits(catalog, ts, min_score=-5))):
        r = _cli(["--targets", path] + args, i)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        out = r.stdout.decode()
        assert out == want, args
        assert "".join(l + "\n" for l in out.splitlines() if not l.startswith("    ")) == plain.stdout.decode()
        assert "".join(l + "\n" for l in out.splitlines() if not l.startswith("  ")) == expected(i)  # unchanged lines
        assert any(l.startswith("    top 2: " if "--target-top" in args else "    hit: ") for l in out.splitlines())


def test_cli_target_flags_two_gloo_ranks(tmp_path):
    prob = Problem.read(input_path(3))
    path, ts, catalog = cli_targets_file(tmp_path, prob)
    for args, want in ((["--target-top", "4"], want_topk(catalog, ts, 4)),
                       (["--target-within", "20"], want_hits(catalog, ts, within=20)),
                       (["--target-min-score", "0"], want_hits(catalog, ts, min_score=0))):
        r = torchrun(2, ["--backend=cpu", "--dist-backend=gloo", "--targets", path, f"--input={input_path(3)}"] + args)
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        assert r.stdout.decode() == want, args


@pytest.mark.parametrize("args", [
    ["--target-top", "2"], ["--target-min-score", "0"], ["--target-within", "0"],  # need --targets
    ["--targets", "FILE", "--target-top", "0"], ["--targets", "FILE", "--target-top", "65"],
    ["--targets", "FILE", "--target-within=-1"], ["--targets", "FILE", "--target-min-score", "2147483648"],
    ["--targets", "FILE", "--target-top", "2", "--target-min-score", "0"],
    ["--targets", "FILE", "--target-top", "2", "--target-within", "0"],
    ["--targets", "FILE", "--target-min-score", "0", "--target-within", "0"],
    ["--targets", "FILE", "--target-top", "2", "--target-summary"],
    ["--targets", "FILE", "--target-within", "3", "--target-summary"],
    ["--targets", "FILE", "--target-min-score", "3", "--target-summary"],
    ["--targets", "FILE", "--target-top", "2", "--top", "2"],  # everything --targets refuses stays refused
    ["--targets", "FILE", "--target-within", "2", "--min-score", "0"],
    ["--targets", "FILE", "--target-top", "2", "--show-alignment"],
    ["--targets", "FILE", "--target-top", "2", "--summary"],
    ["--targets", "FILE", "--target-top", "2", "--partition", "offsets"],
    ["--targets", "FILE", "--top", "2"], ["--targets", "FILE", "--min-score", "0"]])
def test_cli_refusals(tmp_path, args):
    prob = Problem.read(input_path(6))
    path, _, _ = cli_targets_file(tmp_path, prob)
    r = _cli([path if a == "FILE" else a for a in args], 6)
    assert r.returncode != 0 and r.stdout == b"" and r.stderr != b""


def test_distributed_search_on_one_process_and_errors():
    from mpi_openmp_cuda_amd.parallel import dist as D
    from mpi_openmp_cuda_amd.parallel.search import DistributedSearch

    rng = np.random.default_rng(37)
    ts, recs = random_case(rng, 5, 4)
    codes, offsets = batch_of(recs)
    prob = Problem([4, 3, 2, 10], ts.seq1, codes, offsets)
    s = DistributedSearch(D.DistContext(), backend="cpu", partition="records")
    topk = s.run_targets_topk(prob, ts, 5, Semantics.SPEC)
    assert topk.dtype == np.int32 and np.array_equal(topk, search_targets_topk_cpu(prob, ts, 5, Semantics.SPEC))
    for kw in ({"min_score": -3}, {"within": 6}):
        best, rows, toffsets = s.run_targets_hits(prob, ts, semantics=Semantics.SPEC, **kw)
        want, woff = search_targets_hits_cpu(prob, ts, semantics=Semantics.SPEC, **kw)
        assert np.array_equal(best, search_targets_cpu(prob, ts, Semantics.SPEC))
        assert rows.dtype == np.int32 and np.array_equal(rows, want) and np.array_equal(toffsets, woff)
    with pytest.raises(ValueError, match="^targets:"):
        s.run_targets_topk(prob, ts.starts[:-1], 0)
    with pytest.raises(ValueError, match="^targets:"):
        s.run_targets_hits(prob, ts.starts[:-1])
    with pytest.raises(ValueError, match="^top-K:"):
        s.run_targets_topk(prob, ts, 65)
    with pytest.raises(ValueError, match="^hits: give exactly one"):
        s.run_targets_hits(prob, ts, min_score=0, within=0)
    s = DistributedSearch(D.DistContext(), backend="cpu", partition="offsets")
    with pytest.raises(ValueError, match="record slices"):
        s.run_targets_topk(prob, ts, 2)
    with pytest.raises(ValueError, match="record slices"):
        s.run_targets_hits(prob, ts, min_score=0)


# ---- stand-alone sanitizer program -------------------------------------------------------------------------
def test_targets_rows_sanitizer_program():
    """csrc/tests/targets_rows_san.cpp with the CPU core sources under ASan + UBSan: a plain program with its own main
    (nothing is loaded into Python, nothing runs on a GPU)."""
    r = subprocess.run(["make", "-C", ROOT, "-s", "-j8", "targets-rows-san"], capture_output=True, timeout=600)
    out = (r.stdout + r.stderr).decode()
    assert r.returncode == 0, out[-3000:]
    assert "targets_rows_san ok" in out and "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]
