"""Threshold hits on the CPU engine (csrc/src/cpu_engine.cpp hits_batch_cpu): against a filter of the
letter-by-letter Python replay (models/reference.brute_force_profile), the invariants that tie hits to the profile
and to the search, the goldens, the capacity contract of the C ABI over poisoned buffers, argument checking,
format_hits, the Python CLI (--min-score / --within, one and several gloo ranks) and the stand-alone sanitizer
program."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, expected, input_path
from test_dist import torchrun

from mpi_openmp_cuda_amd import (Problem, Semantics, _lib, format_hits, format_results, make_synthetic, search_cpu,
                                 search_hits_cpu, search_profile_cpu)
from mpi_openmp_cuda_amd.models.reference import brute_force_profile
from mpi_openmp_cuda_amd.models.scoring import score_table
from mpi_openmp_cuda_amd.ops.align import as_triples, hits_geometry, within_thresholds

SEMS = [Semantics.REFERENCE, Semantics.SPEC]
I32 = np.iinfo(np.int32)


def problem_of(weights, seq1, recs) -> Problem:
    lens = np.array([len(r) for r in recs], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    codes = np.concatenate([np.asarray(r, np.uint8) for r in recs]) if len(recs) else np.zeros(0, np.uint8)
    return Problem(list(weights), np.asarray(seq1, np.uint8), codes, offsets)


def hits_of_profile(prof, poffsets, thresholds):
    """numpy reference of the filter: (rows [H, 3], hoffsets) of a flat profile under per-record thresholds."""
    n = len(poffsets) - 1
    rows, h = [], np.zeros(n + 1, np.int64)
    for i in range(n):
        p = prof[poffsets[i]:poffsets[i + 1]]
        o = np.flatnonzero(p["score"].astype(np.int64) >= int(thresholds[i]))
        rows.append(np.stack([p["score"][o], o.astype(np.int32), p["k"][o]], axis=1).astype(np.int32))
        h[i + 1] = h[i] + len(o)
    return (np.concatenate(rows) if rows else np.zeros((0, 3), np.int32)).reshape(-1, 3), h


def best_per_record(prof, poffsets):
    """Each record's best profile score (0 where it has no candidate offsets)."""
    return np.array([prof["score"][a:b].max() if b > a else 0 for a, b in zip(poffsets[:-1], poffsets[1:])], np.int64)


# ---- letter replay ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_hits_match_letter_replay(sem):
    rng = np.random.default_rng(40)
    for weights in ((10, 2, 3, 4), (0, 0, 0, 0), (5, 0, 3, 0)):
        for L1 in (1, 2, 3, 9, 26, 40):
            seq1 = rng.integers(1, 27, L1)
            lens = sorted({1, 2, max(L1 - 1, 1), L1, L1 + 1, int(rng.integers(1, L1 + 1))})
            recs = [rng.integers(1, 5 if L1 % 2 else 27, l) for l in lens]  # small alphabets make ties
            prob = problem_of(weights, seq1, recs)
            t = score_table(prob.weights)
            replay = [brute_force_profile(t, prob.seq1, r, sem) for r in recs]
            scores = sorted({s for p in replay for s, _ in p})
            mid = scores[len(scores) // 2] if scores else 0
            for T in (I32.min, mid, mid + 1, I32.max):
                rows, h = search_hits_cpu(prob, min_score=T, semantics=sem)
                assert rows.dtype == np.int32 and h.dtype == np.int64 and h[0] == 0 and h[-1] == len(rows)
                for i, p in enumerate(replay):
                    want = [[s, o, k] for o, (s, k) in enumerate(p) if s >= T]
                    assert rows[h[i]:h[i + 1]].tolist() == want, (weights, L1, lens[i], sem, T)


# ---- invariants ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("shape,n", [("input6", 1000), ("input1", 200), ("input3", 6), ("input4", 40)])
def test_invariants(shape, n, sem):
    prob = make_synthetic(shape, n, seed=3)
    prof, po = search_profile_cpu(prob, sem)
    ref = as_triples(search_cpu(prob, sem))
    # INT32_MIN: the profile, in order
    rows, h = search_hits_cpu(prob, min_score=I32.min, semantics=sem)
    assert np.array_equal(h, po)
    assert np.array_equal(rows[:, 0], prof["score"]) and np.array_equal(rows[:, 2], prof["k"])
    assert np.array_equal(rows[:, 1], np.concatenate([np.arange(c) for c in np.diff(po)] + [np.zeros(0, int)]))
    # INT32_MAX: nothing
    rows, h = search_hits_cpu(prob, min_score=I32.max, semantics=sem)
    assert len(rows) == 0 and not h.any()
    # each record's best: the search's row is the first hit carrying that score (within=0 says the same)
    best = best_per_record(prof, po)
    rows, h = search_hits_cpu(prob, thresholds=best.astype(np.int32), semantics=sem)
    rows_w, h_w = search_hits_cpu(prob, within=0, semantics=sem)
    assert np.array_equal(rows, rows_w) and np.array_equal(h, h_w)
    for i in range(prob.n):
        mine = rows[h[i]:h[i + 1]]
        if po[i + 1] == po[i]:
            assert len(mine) == 0 and ref[i, 0] == I32.min
            continue
        assert (mine[:, 0] == ref[i, 0]).all() and mine[0].tolist() == ref[i].tolist()
        assert (np.diff(mine[:, 1]) > 0).all()
    # one above the best: nothing
    rows, h = search_hits_cpu(prob, thresholds=(best + 1).astype(np.int32), semantics=sem)
    assert len(rows) == 0 and not h.any()


@pytest.mark.parametrize("sem", SEMS)
def test_threshold_is_inclusive(sem):
    prob = make_synthetic("input1", 60, seed=5)
    prof, po = search_profile_cpu(prob, sem)
    # an entry in the middle of every record's profile: its own score includes it, one above excludes it
    at = (po[:-1] + po[1:]) // 2
    own = prof["score"][at].astype(np.int64)
    assert (np.diff(po) > 0).all()
    for delta, inside in ((0, True), (1, False)):
        thr = (own + delta).astype(np.int32)
        rows, h = search_hits_cpu(prob, thresholds=thr, semantics=sem)
        want_rows, want_h = hits_of_profile(prof, po, thr)
        assert np.array_equal(h, want_h) and np.array_equal(rows, want_rows)
        for i in range(prob.n):
            assert ((at[i] - po[i]) in rows[h[i]:h[i + 1], 1]) == inside
    assert 0 < want_h[-1] < po[-1]


def test_within_is_clipped_int64_arithmetic():
    t = within_thresholds(np.array([I32.min, I32.min + 5, 0, I32.max], np.int32), 10)
    assert t.dtype == np.int32 and t.tolist() == [I32.min, I32.min, -10, I32.max - 10]
    assert within_thresholds(np.array([7], np.int32), 2 ** 40).tolist() == [I32.min]


@pytest.mark.parametrize("i", range(1, 7))
def test_goldens_first_best_hit(i):
    prob = Problem.read(input_path(i))
    rows, h = search_hits_cpu(prob, within=0)
    first = np.array([rows[h[j]] if h[j + 1] > h[j] else (I32.min, 0, 0) for j in range(prob.n)], np.int32)
    assert format_results(first) == expected(i)


# ---- capacity contract of the C ABI ----------------------------------------------------------------------
def _cpu_hits_raw(prob, sem, min_score, thr, hoffsets, rows, cap):
    return _lib.lib().moc_cpu_hits(_lib.weights_arg(prob.weights.as_list()), _lib.ptr(prob.seq1), prob.L1,
                                   _lib.ptr(prob.codes), _lib.ptr(prob.offsets), prob.n, int(sem), 0, min_score,
                                   _lib.ptr(thr), _lib.ptr(hoffsets), _lib.ptr(rows), cap)


@pytest.mark.parametrize("sem", SEMS)
def test_capacity_contract(sem):
    prob = make_synthetic("input1", 40, seed=6)
    prof, po = search_profile_cpu(prob, sem)
    thr = np.array([np.median(prof["score"][a:b]) for a, b in zip(po[:-1], po[1:])]).astype(np.int32)
    want_rows, want_h = hits_of_profile(prof, po, thr)
    total = int(want_h[-1])
    assert 1 < total < po[-1]
    POISON = -777
    for cap in (0, 1, total - 1, total):
        h = np.full(prob.n + 1, POISON, np.int64)
        buf = np.full((total + 8, 3), POISON, np.int32)  # the rows, then guard space
        assert _cpu_hits_raw(prob, sem, 0, thr, h, None if cap == 0 else buf, cap) == 0
        assert np.array_equal(h, want_h), cap  # complete and exact whatever cap is
        assert np.array_equal(buf[:cap], want_rows[:cap]) and (buf[cap:] == POISON).all(), cap
    h = np.zeros(prob.n + 1, np.int64)
    assert _cpu_hits_raw(prob, sem, 0, thr, h, None, 3) == -1 and b"cap" in _lib.lib().moc_last_error()


def test_hits_geometry():
    g = hits_geometry()
    assert len(g) == 2 and g[0] >= 64 and g[1] >= 64 and g[0] * g[1] + 1 < 2 ** 31 - 1


# ---- argument checking -----------------------------------------------------------------------------------
def test_argument_checking():
    prob = make_synthetic("input6", 8)
    thr = np.zeros(prob.n, np.int32)
    with pytest.raises(ValueError, match="exactly one"):
        search_hits_cpu(prob)
    for kw in ({"min_score": 0, "within": 0}, {"min_score": 0, "thresholds": thr}, {"thresholds": thr, "within": 1},
               {"min_score": 0, "thresholds": thr, "within": 1}):
        with pytest.raises(ValueError, match="exactly one"):
            search_hits_cpu(prob, **kw)
    for bad in (thr[:-1], np.zeros(prob.n + 1, np.int32), np.zeros((prob.n, 1), np.int32), np.zeros(prob.n)):
        with pytest.raises(ValueError, match="thresholds"):
            search_hits_cpu(prob, thresholds=bad)
    with pytest.raises(ValueError, match="within"):
        search_hits_cpu(prob, within=-1)
    with pytest.raises(ValueError, match="int32"):
        search_hits_cpu(prob, min_score=2 ** 31)


def test_empty_batch():
    prob = problem_of((10, 2, 3, 4), np.arange(1, 9), [])
    rows, h = search_hits_cpu(prob, min_score=0)
    assert rows.shape == (0, 3) and h.tolist() == [0]


# ---- format_hits -------------------------------------------------------------------------------------------
def test_format_hits():
    res = np.array([[5, 1, 2], [I32.min, 0, 0], [4, 0, 0]], np.int32)
    rows = np.array([[5, 1, 2], [3, 4, 0], [4, 0, 0]], np.int32)
    text = format_hits(res, rows, np.array([0, 2, 2, 3]), first_index=7)
    assert text == ("#7: score: 5, n: 1, k: 2\n  hit: score: 5, n: 1, k: 2\n  hit: score: 3, n: 4, k: 0\n"
                    f"#8: score: {I32.min}, n: 0, k: 0\n"
                    "#9: score: 4, n: 0, k: 0\n  hit: score: 4, n: 0, k: 0\n")
    assert format_hits(res, rows[:0], np.zeros(4, np.int64)) == format_results(res)
    with pytest.raises(ValueError):
        format_hits(res, rows, np.array([0, 2, 3]))
    with pytest.raises(ValueError):
        format_hits(res, rows, np.array([0, 2, 1, 3]))


# ---- the Python CLI ----------------------------------------------------------------------------------------
def _cli(args, i):
    with open(input_path(i), "rb") as f:
        return subprocess.run([sys.executable, "-m", "mpi_openmp_cuda_amd", "--backend=cpu"] + args, stdin=f,
                              capture_output=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd="/tmp", timeout=120)


@pytest.mark.parametrize("i", range(1, 7))
def test_cli_without_the_flags_is_todays_output(i):
    r = _cli([], i)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout.decode() == expected(i)


@pytest.mark.parametrize("nproc", [1, 3])
def test_cli_within0_input3(nproc):
    prob = Problem.read(input_path(3))
    want = format_hits(search_cpu(prob), *search_hits_cpu(prob, within=0))
    if nproc == 1:
        r = _cli(["--within", "0"], 3)
    else:
        r = torchrun(nproc, ["--backend=cpu", "--dist-backend=gloo", "--within", "0", f"--input={input_path(3)}"])
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert r.stdout.decode() == want
    assert [l for l in want.splitlines() if not l.startswith("  ")] == expected(3).splitlines()


def test_cli_min_score_input6():
    prob = Problem.read(input_path(6))
    r = _cli(["--min-score", "0"], 6)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout.decode() == format_hits(search_cpu(prob), *search_hits_cpu(prob, min_score=0))


@pytest.mark.parametrize("args", [["--min-score", "0", "--within", "0"], ["--min-score", "0", "--top", "2"],
                                  ["--within", "0", "--top", "2"], ["--min-score", "0", "--show-alignment"],
                                  ["--within", "0", "--show-alignment"], ["--within", "-1"],
                                  ["--within", "0", "--partition", "offsets"]])
def test_cli_refused_combinations(args):
    r = _cli(args, 6)
    assert r.returncode != 0 and r.stdout == b"" and r.stderr != b""


def test_run_hits_refuses_offsets_partition():
    from mpi_openmp_cuda_amd.parallel import dist as D
    from mpi_openmp_cuda_amd.parallel.search import DistributedSearch

    s = DistributedSearch(D.DistContext(), backend="cpu", partition="offsets")
    with pytest.raises(ValueError, match="record slices"):
        s.run_hits(Problem.read(input_path(1)), min_score=0)


# ---- stand-alone sanitizer program -------------------------------------------------------------------------
def test_hits_sanitizer_program():
    """csrc/tests/hits_san.cpp with the CPU core sources under ASan + UBSan: a plain program with its own main
    (nothing is loaded into Python, nothing runs on a GPU)."""
    r = subprocess.run(["make", "-C", ROOT, "-s", "-j8", "hits-san"], capture_output=True, timeout=600)
    out = (r.stdout + r.stderr).decode()
    assert r.returncode == 0, out[-3000:]
    assert "hits_san ok" in out and "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]
