"""Per-offset score profile and top-K alignments on the CPU engine (csrc/src/cpu_engine.cpp): against the
letter-by-letter Python replay (models/reference.brute_force_profile), against the search itself (row 0 of
the top-K and the maximum over a profile are search_cpu's rows), against a numpy sort of the profile, on ties,
through the Python CLI (--top, one and several gloo ranks), and the stand-alone sanitizer program."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, expected, input_path
from test_dist import torchrun

from mpi_openmp_cuda_amd import (PROFILE_DTYPE, Problem, Semantics, format_topk, make_synthetic, profile_offsets,
                                 search_cpu, search_profile_cpu, search_topk_cpu)
from mpi_openmp_cuda_amd.models.reference import brute_force_profile
from mpi_openmp_cuda_amd.models.scoring import score_table
from mpi_openmp_cuda_amd.ops.align import as_triples

SEMS = [Semantics.REFERENCE, Semantics.SPEC]
NONE = (np.iinfo(np.int32).min, 0, 0)


def problem_of(weights, seq1, recs) -> Problem:
    lens = np.array([len(r) for r in recs], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    codes = np.concatenate([np.asarray(r, np.uint8) for r in recs]) if len(recs) else np.zeros(0, np.uint8)
    return Problem(list(weights), np.asarray(seq1, np.uint8), codes, offsets)


def letters(s: str) -> np.ndarray:
    return np.frombuffer(s.encode(), np.uint8) - ord("A") + 1


def topk_of_profile(prof, poffsets, K) -> np.ndarray:
    """numpy reference of the selection: each record's profile sorted by (-score, n), truncated and padded."""
    n = len(poffsets) - 1
    out = np.empty((n, K, 3), np.int32)
    out[:] = NONE
    for i in range(n):
        p = prof[poffsets[i]:poffsets[i + 1]]
        order = np.lexsort((np.arange(len(p)), -p["score"].astype(np.int64)))[:K]
        out[i, :len(order), 0] = p["score"][order]
        out[i, :len(order), 1] = order
        out[i, :len(order), 2] = p["k"][order]
    return out


@pytest.mark.parametrize("sem", SEMS)
def test_profile_matches_letter_replay(sem):
    rng = np.random.default_rng(20)
    for weights in ((10, 2, 3, 4), (0, 0, 0, 0), (5, 0, 3, 0), (1, 7, 0, 2)):
        for L1 in (1, 2, 3, 9, 26, 40):
            seq1 = rng.integers(1, 27, L1)
            lens = sorted({1, 2, max(L1 - 1, 1), L1, L1 + 1, int(rng.integers(1, L1 + 1))})
            recs = [rng.integers(1, 5 if L1 % 2 else 27, l) for l in lens]  # small alphabets make ties
            prob = problem_of(weights, seq1, recs)
            prof, poffsets = search_profile_cpu(prob, sem)
            assert prof.dtype == PROFILE_DTYPE
            assert np.array_equal(poffsets, profile_offsets(L1, lens, sem))
            t = score_table(prob.weights)
            for i, r in enumerate(recs):
                want = brute_force_profile(t, prob.seq1, r, sem)
                got = [(int(s), int(k)) for s, k in prof[poffsets[i]:poffsets[i + 1]]]
                assert got == want, (weights, L1, lens[i], sem)


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("shape,n", [("input6", 1000), ("input1", 200), ("input3", 6), ("input4", 40)])
def test_invariants_against_search(shape, n, sem):
    prob = make_synthetic(shape, n, seed=3)
    ref = as_triples(search_cpu(prob, sem))
    prof, poffsets = search_profile_cpu(prob, sem)
    top = search_topk_cpu(prob, 4, sem)
    assert np.array_equal(top[:, 0], ref)  # row 0 is today's result
    assert np.array_equal(topk_of_profile(prof, poffsets, 1)[:, 0], ref)  # and so is the profile's maximum


@pytest.mark.parametrize("i", range(1, 7))
def test_goldens_rank1(i):
    prob = Problem.read(input_path(i))
    top = search_topk_cpu(prob, 3)
    assert format_topk(top[:, :1]) == expected(i)
    body = format_topk(top).splitlines()
    assert [l for l in body if "." not in l.split(":")[0]] == expected(i).splitlines()


@pytest.mark.parametrize("K", [1, 2, 7, 64])
def test_topk_is_the_sorted_profile(K):
    for shape, n, sem in (("input6", 300, Semantics.REFERENCE), ("input1", 50, Semantics.SPEC),
                          ("input4", 12, Semantics.REFERENCE)):
        prob = make_synthetic(shape, n, seed=5)
        prof, poffsets = search_profile_cpu(prob, sem)
        assert np.array_equal(search_topk_cpu(prob, K, sem), topk_of_profile(prof, poffsets, K))


@pytest.mark.parametrize("K", [0, 65])
def test_k_out_of_range(K):
    with pytest.raises(ValueError):
        search_topk_cpu(make_synthetic("input6", 4), K)


def test_k_out_of_range_native():
    from mpi_openmp_cuda_amd import _lib

    prob = make_synthetic("input6", 4)
    out = np.zeros((4, 65, 3), np.int32)
    rc = _lib.lib().moc_cpu_topk(_lib.weights_arg(prob.weights.as_list()), _lib.ptr(prob.seq1), prob.L1,
                                 _lib.ptr(prob.codes), _lib.ptr(prob.offsets), prob.n, 0, 0, 65, _lib.ptr(out))
    assert rc == -1 and b"1..64" in _lib.lib().moc_last_error()


def test_all_ties():
    prob = problem_of((10, 2, 3, 4), letters("A" * 80), [letters("A" * l) for l in (1, 5, 79)])
    top = search_topk_cpu(prob, 8, Semantics.REFERENCE)
    for i, L2 in enumerate((1, 5)):  # C = 80 - L2 > 8: the first eight offsets, un-mutated
        assert top[i].tolist() == [[10 * L2, n, 0] for n in range(8)]
    assert top[2].tolist() == [[790, 0, 0]] + [list(NONE)] * 7  # C = 1
    prof, poffsets = search_profile_cpu(prob, Semantics.REFERENCE)
    assert np.diff(poffsets).tolist() == [79, 75, 1] and not prof["k"].any()


def test_format_topk():
    top = np.array([[[5, 1, 2], [4, 0, 0], list(NONE)], [list(NONE)] * 3], np.int32)
    assert format_topk(top, first_index=7) == ("#7: score: 5, n: 1, k: 2\n#7.2: score: 4, n: 0, k: 0\n"
                                               f"#8: score: {NONE[0]}, n: 0, k: 0\n")


# ---- the Python CLI --------------------------------------------------------------------------------------
def _cli(args, i):
    with open(input_path(i), "rb") as f:
        return subprocess.run([sys.executable, "-m", "mpi_openmp_cuda_amd", "--backend=cpu"] + args, stdin=f,
                              capture_output=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd="/tmp", timeout=120)


@pytest.mark.parametrize("i", range(1, 7))
def test_cli_top1_is_todays_output(i):
    r = _cli(["--top", "1"], i)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout.decode() == expected(i)


@pytest.mark.parametrize("i,nproc", [(3, 1), (6, 1), (3, 3), (2, 3)])
def test_cli_top3(i, nproc):
    want = format_topk(search_topk_cpu(Problem.read(input_path(i)), 3))
    if nproc == 1:
        r = _cli(["--top", "3"], i)
    else:
        r = torchrun(nproc, ["--backend=cpu", "--dist-backend=gloo", "--top", "3", f"--input={input_path(i)}"])
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert r.stdout.decode() == want


def test_cli_top_needs_record_slices():
    r = _cli(["--top", "3", "--partition", "offsets"], 1)
    assert r.returncode != 0 and b"--partition records" in r.stderr and r.stdout == b""


def test_run_topk_refuses_offsets_partition():
    from mpi_openmp_cuda_amd.parallel import dist as D
    from mpi_openmp_cuda_amd.parallel.search import DistributedSearch

    s = DistributedSearch(D.DistContext(), backend="cpu", partition="offsets")
    with pytest.raises(ValueError, match="record slices"):
        s.run_topk(Problem.read(input_path(1)), 3)


# ---- stand-alone sanitizer program -------------------------------------------------------------------------
def test_profile_sanitizer_program():
    """csrc/tests/profile_san.cpp with the CPU core sources under ASan + UBSan: a plain program with its own
    main (nothing is loaded into Python, nothing runs on a GPU)."""
    r = subprocess.run(["make", "-C", ROOT, "-s", "-j8", "profile-san"], capture_output=True, timeout=600)
    out = (r.stdout + r.stderr).decode()
    assert r.returncode == 0, out[-3000:]
    assert "profile_san ok" in out and "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]
