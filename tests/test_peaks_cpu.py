"""Distinct placements on the CPU engine (csrc/src/cpu_engine.cpp peaks_filter and the radius forms of
topk_batch_cpu / hits_batch_cpu): against models/reference.brute_force_peaks — the definition as a plain double loop
over the letter-by-letter profile — on the goldens and on seeded random problems, the invariants that tie the distinct
forms to the plain ones and to the search, the planted two-placement case, a plateau, the capacity contract of the C
ABI over poisoned buffers, the Python CLI (--distinct) and the stand-alone sanitizer program."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, input_path

from mpi_openmp_cuda_amd import Problem, Semantics, _lib, search_cpu, search_hits_cpu, search_topk_cpu
from mpi_openmp_cuda_amd.models.reference import brute_force_peaks, brute_force_profile
from mpi_openmp_cuda_amd.models.scoring import score_table
from mpi_openmp_cuda_amd.ops.align import MAX_PEAK_RADIUS, as_triples, profile_offsets

SEMS = [Semantics.REFERENCE, Semantics.SPEC]
I32 = np.iinfo(np.int32)
PAD = [I32.min, 0, 0]


def problem_of(weights, seq1, recs) -> Problem:
    lens = np.array([len(r) for r in recs], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    codes = np.concatenate([np.asarray(r, np.uint8) for r in recs]) if len(recs) else np.zeros(0, np.uint8)
    return Problem(list(weights), np.asarray(seq1, np.uint8), codes, offsets)


def records_of(prob):
    return [prob.codes[prob.offsets[i]:prob.offsets[i + 1]] for i in range(prob.n)]


def check_against_oracle(prob, sem, radii, Ks=(1, 3, 64)):
    """search_hits_cpu(radius=R) at INT32_MIN and at a middle threshold, and search_topk_cpu(radius=R), against rows
    derived from brute_force_peaks. The letter-by-letter profile is computed once per record."""
    t = score_table(prob.weights)
    profs = [brute_force_profile(t, prob.seq1, r, sem) for r in records_of(prob)]
    scores = sorted({s for p in profs for s, _ in p})
    mid = scores[len(scores) // 2] if scores else 0
    for R in radii:
        peaks = [brute_force_peaks(t, prob.seq1, None, R, sem, profile=p) for p in profs]
        for T in (I32.min, mid):
            rows, h = search_hits_cpu(prob, min_score=T, semantics=sem, radius=R)
            assert h[0] == 0 and h[-1] == len(rows)
            for i, pk in enumerate(peaks):
                want = [list(row) for row in pk if row[0] >= T]
                assert rows[h[i]:h[i + 1]].tolist() == want, (sem, R, T, i)
        for K in Ks:
            top = search_topk_cpu(prob, K, sem, radius=R)
            for i, pk in enumerate(peaks):
                ranked = sorted(pk, key=lambda row: (-row[0], row[1]))[:K]
                want = [list(row) for row in ranked] + [PAD] * (K - len(ranked))
                assert top[i].tolist() == want, (sem, R, K, i)


# ---- replay oracle ---------------------------------------------------------------------------------------
def test_native_radius_bound():
    assert _lib.lib().moc_peaks_max_radius() == MAX_PEAK_RADIUS == 2048


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("i", [1, 5, 6])
def test_goldens_match_oracle(i, sem):
    check_against_oracle(Problem.read(input_path(i)), sem, (1, 2, 5, 1000))


@pytest.mark.parametrize("sem", SEMS)
def test_random_problems_match_oracle(sem):
    rng = np.random.default_rng(77)
    for weights in ((4, 3, 2, 10), (10, 2, 3, 4), (0, 0, 0, 0)):
        for L1 in (1, 2, 7, 40, 120):
            seq1 = rng.integers(1, 27, L1)
            lens = sorted({1, 2, min(24, L1), min(24, max(L1 - 1, 1)), L1 + 1 if L1 < 24 else 24,
                           int(rng.integers(1, min(L1, 24) + 1))})
            recs = [rng.integers(1, 4 if L1 % 2 else 27, l) for l in lens]  # small alphabets make ties and plateaus
            check_against_oracle(problem_of(weights, seq1, recs), sem, (1, 2, 5, 1000), Ks=(1, 5))


# ---- invariants ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("i", range(1, 7))
def test_invariants_on_goldens(i, sem):
    prob = Problem.read(input_path(i))
    ref = as_triples(search_cpu(prob, sem))
    # radius 0 is the call without the keyword
    rows0, h0 = search_hits_cpu(prob, within=20, semantics=sem)
    rows, h = search_hits_cpu(prob, within=20, semantics=sem, radius=0)
    assert np.array_equal(rows, rows0) and np.array_equal(h, h0)
    assert np.array_equal(search_topk_cpu(prob, 4, sem, radius=0), search_topk_cpu(prob, 4, sem))
    # the largest radius: one hit for every record whose profile it spans, the search's own row
    C = np.diff(profile_offsets(prob.L1, prob.lengths, sem))
    rows, h = search_hits_cpu(prob, min_score=I32.min, semantics=sem, radius=MAX_PEAK_RADIUS)
    spanned = (C >= 1) & (C <= MAX_PEAK_RADIUS + 1)
    assert spanned.any() or i == 4  # input4: every profile is longer than the largest window
    for j in np.flatnonzero(spanned):
        assert h[j + 1] - h[j] == 1 and rows[h[j]].tolist() == ref[j].tolist(), j
    assert (np.diff(h)[C == 0] == 0).all() and (np.diff(h)[C > 0] >= 1).all()
    # row 0 of distinct top-K is the search's row at every radius; the rows are a subsequence of the plain top-C
    for R in (1, 2, 5, 64, 1000, MAX_PEAK_RADIUS):
        top = search_topk_cpu(prob, 3, sem, radius=R)
        assert np.array_equal(top[:, 0], ref), R
        # fewer peaks at a larger radius, never none where there is a candidate
        n_hits = np.diff(search_hits_cpu(prob, min_score=I32.min, semantics=sem, radius=R)[1])
        assert (n_hits <= C).all() and ((n_hits >= 1) == (C >= 1)).all()


@pytest.mark.parametrize("sem", SEMS)
def test_threshold_does_not_interact(sem):
    """Distinct hits under a threshold are the distinct hits of the whole profile that reach it."""
    prob = Problem.read(input_path(3))
    allp, ha = search_hits_cpu(prob, min_score=I32.min, semantics=sem, radius=7)
    best = as_triples(search_cpu(prob, sem))[:, 0].astype(np.int64)
    thr = (best - 30).clip(I32.min, I32.max).astype(np.int32)
    rows, h = search_hits_cpu(prob, thresholds=thr, semantics=sem, radius=7)
    rows_w, h_w = search_hits_cpu(prob, within=30, semantics=sem, radius=7)
    assert np.array_equal(rows, rows_w) and np.array_equal(h, h_w)
    for i in range(prob.n):
        mine = allp[ha[i]:ha[i + 1]]
        assert np.array_equal(rows[h[i]:h[i + 1]], mine[mine[:, 0] >= thr[i]])


# ---- the planted case ------------------------------------------------------------------------------------
def planted_problem():
    """A seeded 300-letter Seq1 that holds a 40-letter record at offsets 100 and 220; the record then has 4 of its
    letters changed. Weights 4 3 2 10."""
    rng = np.random.default_rng(5)
    seq1 = rng.integers(1, 27, 300)
    rec = rng.integers(1, 27, 40)
    seq1[100:140] = rec
    seq1[220:260] = rec
    rec = rec.copy()
    for at in (5, 14, 23, 32):
        rec[at] = rec[at] % 26 + 1
    return problem_of((4, 3, 2, 10), seq1, [rec])


def test_planted_placements():
    prob = planted_problem()
    rows, h = search_hits_cpu(prob, within=20)
    # the input has not gone stale: both placements and both one-column shadows (k = 1, one offset to the left)
    by_n = {int(n): (int(s), int(k)) for s, n, k in rows}
    assert {99, 100, 219, 220} <= set(by_n), rows.tolist()
    assert by_n[99][1] == 1 and by_n[219][1] == 1 and by_n[100][1] == 0 and by_n[220][1] == 0
    assert len(rows) == 4
    top = search_topk_cpu(prob, 4)
    assert sorted(top[0, :, 1].tolist()) == [99, 100, 219, 220]
    # distinct: the two placements, one row each
    drows, dh = search_hits_cpu(prob, within=20, radius=1)
    assert dh.tolist() == [0, 2] and len(drows) == 2
    assert [n in (99, 100) for n in drows[:1, 1]] == [True] and [n in (219, 220) for n in drows[1:, 1]] == [True]
    dtop = search_topk_cpu(prob, 4, radius=1)
    assert sorted(dtop[0, :2].tolist()) == sorted(drows.tolist())
    assert (dtop[0, 2:, 0] < dtop[0, 0, 0] - 20).all()  # ranks 3 and 4 are other, far weaker peaks: no placement
    assert dtop[0, 0].tolist() == as_triples(search_cpu(prob))[0].tolist()


# ---- plateau ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_plateau_keeps_its_first_entry(sem):
    prob = problem_of((4, 3, 2, 10), np.full(208, 1), [np.full(8, 1)])
    plain, _ = search_hits_cpu(prob, min_score=I32.min, semantics=sem)
    assert len(plain) >= 200 and len(set(plain[:, 0].tolist())) == 1  # one score throughout
    rows, h = search_hits_cpu(prob, min_score=I32.min, semantics=sem, radius=3)
    assert h.tolist() == [0, 1] and rows[0, 1] == 0 and rows[0].tolist() == as_triples(search_cpu(prob, sem))[0].tolist()
    assert search_topk_cpu(prob, 3, sem, radius=3)[0].tolist() == [rows[0].tolist(), PAD, PAD]


def test_local_maximum_not_greedy():
    """Scores 10, 9, 8 at R = 1: only the 10 is a peak (the 9 suppresses the 8 although the 10 suppresses the 9)."""
    t = score_table([1, 1, 1, 1])
    prof = [(10, 0), (9, 0), (8, 0)]
    assert brute_force_peaks(t, None, None, 1, profile=prof) == [(10, 0, 0)]
    assert brute_force_peaks(t, None, None, 0, profile=prof) == [(10, 0, 0), (9, 1, 0), (8, 2, 0)]
    assert brute_force_peaks(t, None, None, 1, profile=[(8, 0), (9, 0), (10, 0)]) == [(10, 2, 0)]
    assert brute_force_peaks(t, None, None, 1, profile=[(7, 0), (7, 0), (7, 0)]) == [(7, 0, 0)]


# ---- capacity contract of the C ABI ----------------------------------------------------------------------
def _cpu_hits_distinct_raw(prob, sem, min_score, thr, radius, hoffsets, rows, cap):
    return _lib.lib().moc_cpu_hits_distinct(_lib.weights_arg(prob.weights.as_list()), _lib.ptr(prob.seq1), prob.L1,
                                            _lib.ptr(prob.codes), _lib.ptr(prob.offsets), prob.n, int(sem), 0,
                                            min_score, _lib.ptr(thr), radius, _lib.ptr(hoffsets), _lib.ptr(rows), cap)


@pytest.mark.parametrize("sem", SEMS)
def test_capacity_contract(sem):
    prob = Problem.read(input_path(1))
    want_rows, want_h = search_hits_cpu(prob, min_score=I32.min, semantics=sem, radius=2)
    total = int(want_h[-1])
    assert 2 * prob.n < total < profile_offsets(prob.L1, prob.lengths, sem)[-1]
    POISON = -777
    for cap in (0, 1, total - 1, total):
        h = np.full(prob.n + 1, POISON, np.int64)
        buf = np.full((total + 8, 3), POISON, np.int32)  # the rows, then guard space
        assert _cpu_hits_distinct_raw(prob, sem, I32.min, None, 2, h, None if cap == 0 else buf, cap) == 0
        assert np.array_equal(h, want_h), cap  # complete and exact whatever cap is
        assert np.array_equal(buf[:cap], want_rows[:cap]) and (buf[cap:] == POISON).all(), cap
    h = np.zeros(prob.n + 1, np.int64)
    assert _cpu_hits_distinct_raw(prob, sem, 0, None, 2, h, None, 3) == -1 and b"cap" in _lib.lib().moc_last_error()
    assert _cpu_hits_distinct_raw(prob, sem, 0, None, MAX_PEAK_RADIUS + 1, h, None, 0) == -1
    assert b"radius" in _lib.lib().moc_last_error()
    assert _cpu_hits_distinct_raw(prob, sem, 0, None, -1, h, None, 0) == -1


def test_radius_out_of_range():
    prob = Problem.read(input_path(6))
    for bad in (-1, MAX_PEAK_RADIUS + 1, 2 ** 40):
        with pytest.raises(ValueError, match="radius"):
            search_topk_cpu(prob, 2, radius=bad)
        with pytest.raises(ValueError, match="radius"):
            search_hits_cpu(prob, min_score=0, radius=bad)
    with pytest.raises(ValueError, match="radius"):
        search_hits_cpu(prob, min_score=0, radius=1.5)


# ---- the Python CLI ----------------------------------------------------------------------------------------
def _cli(args, data: bytes):
    return subprocess.run([sys.executable, "-m", "mpi_openmp_cuda_amd", "--backend=cpu"] + args, input=data,
                          capture_output=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd="/tmp", timeout=120)


def _is_subsequence(part, whole):
    it = iter(whole)
    return all(line in it for line in part)


@pytest.mark.parametrize("flags", [["--top", "3"], ["--within", "20"], ["--min-score", "0"]])
def test_cli_distinct_prints_a_subset(flags):
    data = open(input_path(1), "rb").read()
    plain = _cli(flags, data)
    zero = _cli(flags + ["--distinct", "0"], data)
    one = _cli(flags + ["--distinct", "1"], data)
    for r in (plain, zero, one):
        assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert zero.stdout == plain.stdout  # byte-identical
    a, b = one.stdout.decode().splitlines(), plain.stdout.decode().splitlines()
    if flags[0] == "--top":
        # The K best distinct placements are K of the record's offsets, not K of its K best offsets: where a shadow
        # drops out of the first K, the next peak moves up (record 0: n = 14, the shadow of n = 15, makes room for
        # n = 6). So the lines are a subset of the lines that print EVERY offset (--top 64; input1's records have
        # at most 19), ranks aside, and never more than without the flag.
        every = _cli(["--top", "64"], data)
        assert every.returncode == 0

        def unranked(lines):  # "#i.j: score..." -> "#i: score..."
            return [l.split(".", 1)[0] + ":" + l.split(":", 1)[1] if "." in l.split(":")[0] else l for l in lines]

        assert len(a) <= len(b) and a != b and set(unranked(a)) <= set(unranked(every.stdout.decode().splitlines()))
        one64 = _cli(["--top", "64", "--distinct", "1"], data).stdout.decode().splitlines()
        assert len(one64) < len(every.stdout.decode().splitlines())  # fewer lines once K does not cut them
        prob = Problem.read(input_path(1))
        top = search_topk_cpu(prob, 3, radius=1)
        from mpi_openmp_cuda_amd import format_topk

        assert one.stdout.decode() == format_topk(top)
    else:
        assert len(a) < len(b) and _is_subsequence(a, b)
    # the records' own lines are all there
    assert [l for l in a if l.startswith("#") and "." not in l.split(":")[0]] == \
        [l for l in b if l.startswith("#") and "." not in l.split(":")[0]]


@pytest.mark.parametrize("args", [["--distinct", "1"], ["--distinct", "0"], ["--top", "3", "--distinct", "2049"],
                                  ["--top", "3", "--distinct", "-1"], ["--within", "5", "--distinct", "9999"],
                                  ["--top", "1", "--distinct", "1"],
                                  ["--top", "3", "--distinct", "1", "--partition", "offsets"]])
def test_cli_distinct_errors(args):
    r = _cli(args, open(input_path(6), "rb").read())
    assert r.returncode != 0 and r.stdout == b"" and r.stderr != b""


# ---- stand-alone sanitizer program -------------------------------------------------------------------------
def test_peaks_sanitizer_program():
    """csrc/tests/peaks_san.cpp with the CPU core sources under ASan + UBSan: a plain program with its own main
    (nothing is loaded into Python, nothing runs on a GPU)."""
    r = subprocess.run(["make", "-C", ROOT, "-s", "-j8", "peaks-san"], capture_output=True, timeout=600)
    out = (r.stdout + r.stderr).decode()
    assert r.returncode == 0, out[-3000:]
    assert "peaks_san ok" in out and "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]
