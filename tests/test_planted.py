"""Planted winners (utils/synthetic.make_planted / make_planted_ties): problems in which a chosen offset is the
unique best one, or two chosen offsets tie, so that an engine dropping one offset is caught at that offset
and not with the odds of a random problem. CPU tier: the builders against the pure-Python prefix oracle, then
the CPU engine (the GPU tier's oracle) at every offset around its vector widths, and its context-parallel
keys over more parts than a record has tiles. Every winner planted by those two builders has k = 0; make_planted_k
plants the mutation point too (here against the oracle; tests/test_planted_k.py has the rest)."""
import numpy as np
import pytest

from mpi_openmp_cuda_amd import Semantics, decode_keys, search_cpu, search_keys_cpu
from mpi_openmp_cuda_amd.models.reference import prefix_oracle, solve_problem
from mpi_openmp_cuda_amd.ops.align import as_triples
from mpi_openmp_cuda_amd.utils.synthetic import (differing, make_planted, make_planted_k, make_planted_ties,
                                                 planted_expected, planted_k_expected, seq_no_equal_neighbours)

W = (10, 2, 3, 4)
SEMS = [Semantics.REFERENCE, Semantics.SPEC]


@pytest.mark.parametrize("alphabet", [2, 3, 26])
def test_seq_no_equal_neighbours(alphabet):
    s = seq_no_equal_neighbours(np.random.default_rng(alphabet), 5000, alphabet)
    assert s.dtype == np.uint8 and s.min() >= 1 and s.max() <= alphabet
    assert (s[1:] != s[:-1]).all()
    assert len(np.unique(s)) == alphabet
    assert seq_no_equal_neighbours(np.random.default_rng(0), 0).shape == (0,)
    assert seq_no_equal_neighbours(np.random.default_rng(0), 1).shape == (1,)


@pytest.mark.parametrize("L1,L2", [(300, 12), (70, 8), (400, 40), (200, 150)])
@pytest.mark.parametrize("sem", SEMS)
def test_planted_matches_prefix_oracle(L1, L2, sem):
    prob, pos = make_planted(L1, L2, W, seed=L1 + L2)
    assert pos.tolist() == list(range(L1 - L2 + 1)) and prob.n == L1 - L2 + 1
    assert (prob.seq1[1:] != prob.seq1[:-1]).all()
    oracle = solve_problem(prob, sem, oracle=prefix_oracle)
    # the construction's claim, for every record the claim covers: all under the spec semantics, all but the
    # one at the final offset under the reference semantics (which never try that offset) ...
    claim = np.stack([np.full(prob.n, W[0] * L2), pos, np.zeros(prob.n, np.int64)], axis=1)
    m = prob.n if sem == Semantics.SPEC else prob.n - 1
    assert np.array_equal(oracle[:m], claim[:m]), differing(oracle[:m], claim[:m], pos[:m])
    if sem == Semantics.REFERENCE:
        assert oracle[-1, 0] < W[0] * L2 and oracle[-1, 1] < L1 - L2  # ... where no full match is in reach
    # and planted_expected is that claim with the oracle's answer in the one place
    assert np.array_equal(planted_expected(prob, pos, sem), oracle)
    assert np.array_equal(as_triples(search_cpu(prob, sem)), oracle), differing(as_triples(search_cpu(prob, sem)),
                                                                               oracle, pos)


def test_planted_positions_subset():
    prob, pos = make_planted(300, 12, W, positions=[0, 5, 287, 288, 100], seed=1)
    assert pos.tolist() == [0, 5, 287, 288, 100]
    for i, p in enumerate(pos):
        assert np.array_equal(prob.codes[prob.offsets[i]:prob.offsets[i + 1]], prob.seq1[p:p + 12])
    assert np.array_equal(planted_expected(prob, pos, Semantics.SPEC), solve_problem(prob, Semantics.SPEC))
    with pytest.raises(ValueError):
        make_planted(300, 12, W, positions=[289])


@pytest.mark.parametrize("L1,L2,pairs", [
    (600, 16, [(100, 300)]),
    (600, 16, [(0, 16), (127, 143), (200, 584), (300, 400), (32, 500)]),  # adjacent copies, first and last offsets
    (140, 8, [(0, 132), (8, 16), (60, 100)]),
])
@pytest.mark.parametrize("sem", SEMS)
def test_planted_ties_match_prefix_oracle(L1, L2, pairs, sem):
    prob, pr = make_planted_ties(L1, L2, W, pairs, seed=L1)
    assert (prob.seq1[1:] != prob.seq1[:-1]).all()
    want = np.stack([np.full(len(pairs), W[0] * L2), pr[:, 0], np.zeros(len(pairs), np.int64)], axis=1)
    oracle = solve_problem(prob, sem, oracle=prefix_oracle)
    assert np.array_equal(oracle, want), differing(oracle, want, pr[:, 0])
    got = as_triples(search_cpu(prob, sem))
    assert np.array_equal(got, want), differing(got, want, pr[:, 0])
    for (a, b), i in zip(pairs, range(prob.n)):  # both offsets hold the record
        rec = prob.codes[prob.offsets[i]:prob.offsets[i + 1]]
        assert np.array_equal(prob.seq1[a:a + L2], rec) and np.array_equal(prob.seq1[b:b + L2], rec)


def test_planted_ties_example_and_refusals():
    prob, _ = make_planted_ties(600, 16, W, [(100, 300)])
    assert tuple(solve_problem(prob)[0]) == (160, 100, 0)
    with pytest.raises(ValueError):
        make_planted_ties(600, 16, W, [(100, 110)])  # a + L2 > b
    with pytest.raises(ValueError):
        make_planted_ties(600, 16, W, [(100, 300), (290, 400)])  # segments overlap
    with pytest.raises(ValueError):
        make_planted_ties(600, 16, W, [(100, 590)])  # past the end


# the CPU engine at every offset, the offset count on both sides of 16- and 64-wide vectors, records shorter
# and longer than a vector
@pytest.mark.parametrize("noff", [1, 15, 16, 17, 63, 64, 65])
@pytest.mark.parametrize("L2", [1, 8, 40, 150])
@pytest.mark.parametrize("sem", SEMS)
def test_cpu_engine_every_offset(noff, L2, sem):
    L1 = L2 + noff
    if L2 == 1:
        # a one-letter record matches wherever its letter stands: no unique winner to plant, so the
        # oracle alone decides (the smallest offset holding the letter)
        prob, pos = make_planted(L1, L2, W, seed=noff)
        want = solve_problem(prob, sem, oracle=prefix_oracle)
    else:
        prob, pos = make_planted(L1, L2, W, seed=100 * noff + L2)
        want = planted_expected(prob, pos, sem)
        assert np.array_equal(solve_problem(prob, sem, oracle=prefix_oracle), want)
    for threads in (1, 3):
        got = as_triples(search_cpu(prob, sem, threads=threads))
        assert np.array_equal(got, want), differing(got, want, pos)


@pytest.mark.parametrize("L1,L2", [(300, 12), (200, 150), (1400, 300)])
@pytest.mark.parametrize("parts", [2, 3, 8, 17])
@pytest.mark.parametrize("sem", SEMS)
def test_cpu_keys_combine_over_parts(L1, L2, parts, sem):
    # more parts than a record has 128-offset tiles (200 - 150: one tile; 17 parts), as `--partition=offsets`
    # at 8 ranks and above runs it
    prob, pos = make_planted(L1, L2, W, seed=L1)
    full = search_keys_cpu(prob, 0, 1, sem)
    keys = np.zeros(prob.n, np.uint64)
    for part in range(parts):
        share = search_keys_cpu(prob, part, parts, sem)
        assert (share <= full).all()
        keys = np.maximum(keys, share)
    assert np.array_equal(keys, full), differing(keys[:, None], full[:, None], pos)
    got = as_triples(decode_keys(keys, prob))
    want = planted_expected(prob, pos, sem)
    assert np.array_equal(got, want), differing(got, want, pos)


# every winner above has k = 0. make_planted_k skips one letter of the Seq1 segment, so (p, k) wins: every p and k
@pytest.mark.parametrize("w", [W, (200, 10, 10, 10), (300, 300, 1, 1)], ids=["w", "w_i16", "w_dpp"])
@pytest.mark.parametrize("L1,L2", [(71, 8), (72, 40), (90, 33), (120, 70), (40, 2), (40, 3)])
def test_planted_k_matches_prefix_oracle(L1, L2, w):
    cases = [(p, L2, k) for p in range(L1 - L2) for k in range(1, L2)]
    # (two letters find a rival elsewhere by chance in most Seq1s: a seed whose Seq1 holds none)
    prob, cases = make_planted_k(L1, cases, w, seed=6 if L2 == 2 else L1 + L2)
    assert prob.n == (L1 - L2) * (L2 - 1) and (prob.seq1[1:] != prob.seq1[:-1]).all()
    want = planted_k_expected(prob, cases)
    assert np.array_equal(want, np.stack([np.full(prob.n, w[0] * L2), cases[:, 0], cases[:, 2]], axis=1))
    assert (want[:, 2] >= 1).all()
    for sem in SEMS:
        oracle = solve_problem(prob, sem, oracle=prefix_oracle)
        assert np.array_equal(oracle, want), differing(oracle, want, cases[:, 0])
        for threads in (1, 3):
            got = as_triples(search_cpu(prob, sem, threads=threads))
            assert np.array_equal(got, want), differing(got, want, cases[:, 0])
    with pytest.raises(ValueError):
        make_planted_k(L1, [(L1 - L2, L2, 1)], w)  # the final offset has no letter behind it to skip to
