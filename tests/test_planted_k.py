"""Planted mutation points, CPU tier (utils/synthetic.make_planted_k, make_planted_k_ties, make_extreme_mutants):
the winner's k, which make_planted's exact copies never exercise (k = 0 there). The builders' claims against the
pure-Python prefix oracle and the CPU engine (the GPU tier's oracle) for every (p, k) of the short record lengths
and around the 64-step marks of the long ones, the context-parallel keys, the per-offset profile — and every case
of the lists the GPU tier runs (tests/planted_k.py): each claim against the oracle, no case left out, and a numpy
model of the k rule (planted_k.pick_k) showing that those cases tell each modelled wrong rule from the right one."""
import numpy as np
import pytest

import planted_k as pk
from mpi_openmp_cuda_amd import (Semantics, brute_force_native, decode_keys, search_cpu, search_keys_cpu,
                                 search_profile_cpu, search_topk_cpu)
from mpi_openmp_cuda_amd.models.reference import prefix_oracle, solve_problem
from mpi_openmp_cuda_amd.models.scoring import score_table
from mpi_openmp_cuda_amd.ops.align import as_triples, kernel_bounds
from mpi_openmp_cuda_amd.utils.synthetic import (NEUTRAL, differing, make_extreme, make_extreme_mutants, make_planted_k,
                                                 make_planted_k_ties, planted_k_expected)

W = pk.W
SEMS = [Semantics.REFERENCE, Semantics.SPEC]


def assert_claim(prob, want, pos, threads=(1, 3)):
    """The claim against the prefix oracle and the CPU engine, under both semantics, for every record."""
    for sem in SEMS:
        oracle = solve_problem(prob, sem, oracle=prefix_oracle)
        assert np.array_equal(oracle, want), f"oracle {sem.name}: " + differing(oracle, want, pos)
        for t in threads:
            got = as_triples(search_cpu(prob, sem, threads=t))
            assert np.array_equal(got, want), f"CPU engine {sem.name} threads {t}: " + differing(got, want, pos)


# ---- the builders ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("L2", [2, 3, 8, 16, 17, 32, 33, 40])
def test_every_p_and_k_of_short_records(L2):
    # a swipe-sized Seq1: 63 mutated offsets (the 64th, L1 - L2, has no letter behind it to skip to)
    L1 = L2 + 63
    cases = pk.every_k(L2, range(L1 - L2))
    # (two letters find a rival elsewhere by chance in most Seq1s: a seed whose Seq1 holds none, the claim decides)
    prob, cases = make_planted_k(L1, cases, W, seed={2: 86}.get(L2, L2))
    assert prob.n == 63 * (L2 - 1) and (prob.seq1[1:] != prob.seq1[:-1]).all()
    for i in (0, prob.n - 1):  # the record is the segment with the letter at p + k skipped
        p, _, k = cases[i]
        rec = prob.codes[prob.offsets[i]:prob.offsets[i + 1]]
        assert np.array_equal(rec, np.delete(prob.seq1[p:p + L2 + 1], k))
    want = planted_k_expected(prob, cases)
    assert np.array_equal(want, np.stack([np.full(prob.n, W[0] * L2), cases[:, 0], cases[:, 2]], axis=1))
    assert_claim(prob, want, cases[:, 0])


@pytest.mark.parametrize("L2", [150, 300])
@pytest.mark.parametrize("w", [pk.W, pk.W_I16, pk.W_DPP], ids=["w", "w_i16", "w_dpp"])
def test_k_around_the_64_step_marks(L2, w):
    L1 = L2 + 100
    prob, cases = make_planted_k(L1, pk.some_k(L2, pk.edge_k(L2), (0, 1, 50, 98, 99)), w, seed=L2)
    assert prob.n == 5 * 9
    assert_claim(prob, planted_k_expected(prob, cases), cases[:, 0])


def test_records_of_different_lengths_in_one_problem():
    cases = [(0, 2, 1), (30, 40, 39), (5, 3, 2), (28, 70, 1), (0, 119, 118), (100, 19, 7)]
    prob, cases = make_planted_k(120, cases, W, seed=5)
    assert np.diff(prob.offsets).tolist() == [2, 40, 3, 70, 119, 19]
    assert_claim(prob, planted_k_expected(prob, cases), cases[:, 0])


@pytest.mark.parametrize("w", [pk.W, pk.W_I16, pk.W_DPP], ids=["w", "w_i16", "w_dpp"])
@pytest.mark.parametrize("L1,L2", [(71, 8), (72, 40), (90, 33), (120, 70), (500, 300)])
def test_tie_families(L1, L2, w):
    ps = sorted({0, 1, (L1 - L2) // 2, L1 - L2 - 1})
    inside = [(p, L2, j, k) for p in ps for j, k in pk.inside_pairs(L2)]
    prob, cases = make_planted_k_ties(L1, "inside", inside, w, seed=L1)
    want = planted_k_expected(prob, cases, "inside")
    assert (want[:, 2] == cases[:, 2]).all() and (want[:, 2] < cases[:, 3]).all()  # the smallest k of j .. k
    for i, (p, _, j, k) in enumerate(cases):
        rec = prob.codes[prob.offsets[i]:prob.offsets[i + 1]]
        assert all(c in NEUTRAL and c != prob.seq1[p + s] and c != prob.seq1[p + s + 1]
                   for s, c in zip(range(j, k), rec[j:k]))
    assert_claim(prob, want, cases[:, 0])
    own = [(p, L2, k) for p in ps for k in pk.own_ks(L2)]
    prob, cases = make_planted_k_ties(L1, "own", own, w, seed=L1 + 1)
    want = planted_k_expected(prob, cases, "own")
    assert (want[:, 2] == 0).all() and len(own) == 2 * len(ps)
    assert_claim(prob, want, cases[:, 0])
    # p = L1 - L2: the reference semantics never try that offset, but its shadow, one before
    for s, shadow in enumerate(pk.shadow_sets([1, 4, 5, 32, L1 - L2 - 1, L1 - L2])):
        prob, cases = pk.first_accepted(L1, [(p, L2) for p in shadow if p <= L1 - L2], w, seed=L1 + 2 + s)
        eq = np.nonzero(prob.seq1[1:] == prob.seq1[:-1])[0] + 1
        assert sorted(eq.tolist()) == sorted(cases[:, 0].tolist())  # the only equal neighbours
        want = planted_k_expected(prob, cases, "shadow")
        assert np.array_equal(want[:, 1], cases[:, 0] - 1) and (want[:, 2] == 1).all()
        assert_claim(prob, want, cases[:, 0])


def test_tie_families_on_the_shortest_records():
    # 2 and 3 letters: no room for a 5-letter prefix (nor, with 2, for a tie inside an offset); the shadow tie stands
    for L2 in (2, 3):
        prob, cases = pk.first_accepted(40, [(p, L2) for p in (1, 10, 20, 40 - L2)], W, seed=L2)
        assert_claim(prob, planted_k_expected(prob, cases, "shadow"), cases[:, 0])
        assert pk.own_ks(L2) == [] and pk.inside_pairs(2) == []


def test_refused_constructions():
    for bad in [(0, 8, 0), (0, 8, 8), (0, 1, 1), (32, 8, 3), (-1, 8, 3)]:  # k = 0, k = L2, one letter, no room, p < 0
        with pytest.raises(ValueError):
            make_planted_k(40, [bad], W)
    with pytest.raises(ValueError):
        make_planted_k_ties(40, "inside", [(0, 8, 3, 3)], W)  # j == k
    with pytest.raises(ValueError):
        make_planted_k_ties(40, "own", [(0, 8, 4)], W)  # a prefix of 4 letters: chance beats it
    with pytest.raises(ValueError):
        make_planted_k_ties(40, "own", [(0, 20, 9)], W)  # less than half of the record
    with pytest.raises(ValueError):
        make_planted_k_ties(40, "shadow", [(0, 8)], W)  # no offset before the first
    with pytest.raises(ValueError):
        make_planted_k_ties(40, "shadow", [(10, 8), (11, 8)], W)  # three equal letters in a row
    with pytest.raises(ValueError):
        make_planted_k_ties(40, "nearby", [(10, 8)], W)
    with pytest.raises(ValueError):
        planted_k_expected(make_planted_k(40, [(0, 8, 1)], W)[0], [(0, 8, 1), (1, 8, 1)])  # one case per record


# ---- split searches and per-offset results ----------------------------------------------------------------
@pytest.mark.parametrize("name,family,tag", [("tile16_l2_300_u2", "k", "all"), ("tile16_l2_300_u2", "shadow", "set0"),
                                             ("tile16_l2_300_u2", "shadow", "set1"), ("short_key32", "k", "all"),
                                             ("tile16_l2_40_u8", "shadow", "set0"), ("dpp_tiles_key32", "k", "all")])
@pytest.mark.parametrize("parts", [2, 3, 8, 17])
def test_k_through_cpu_keys_over_parts(name, family, tag, parts):
    prob, cases, want = pk.build(name, family, tag)
    for sem in SEMS:
        full = search_keys_cpu(prob, 0, 1, sem)
        keys = np.zeros(prob.n, np.uint64)
        for part in range(parts):
            share = search_keys_cpu(prob, part, parts, sem)
            assert (share <= full).all()
            keys = np.maximum(keys, share)
        assert np.array_equal(keys, full), differing(keys[:, None], full[:, None], want[:, 1])
        got = as_triples(decode_keys(keys, prob))
        assert np.array_equal(got, want), differing(got, want, want[:, 1])


@pytest.mark.parametrize("parts", [2, 3, 8, 17])
def test_shadow_ties_across_cpu_shares(parts):
    # the CPU engine's share `part` holds the offsets [c part / parts, c (part + 1) / parts) of a record's c = 1100
    # (reference) or 1101 (spec) candidate offsets: these p start a share for some of the part counts, so p - 1 and p
    # lie in different shares and the combined key alone breaks the tie
    L1, L2 = 1400, 300
    for sem, c in ((Semantics.REFERENCE, L1 - L2), (Semantics.SPEC, L1 - L2 + 1)):
        apart = 0
        for s, ps in enumerate(([64, 137, 275, 366, 550, 733], [129, 367])):
            prob, cases = pk.first_accepted(L1, [(p, L2) for p in ps], W, seed=s)
            want = planted_k_expected(prob, cases, "shadow")
            starts = {c * part // parts for part in range(1, parts)}
            keys = np.zeros(prob.n, np.uint64)
            for part in range(parts):
                share = search_keys_cpu(prob, part, parts, sem)
                keys = np.maximum(keys, share)
                rows = as_triples(decode_keys(share, prob))
                for i, p in enumerate(ps):
                    if p in starts and c * part // parts == p:  # the share that starts at p answers (W1 L2, p, 0)
                        assert tuple(rows[i]) == (W[0] * L2, p, 0)
                        apart += 1
            assert np.array_equal(keys, search_keys_cpu(prob, 0, 1, sem))
            got = as_triples(decode_keys(keys, prob))
            assert np.array_equal(got, want), differing(got, want, cases[:, 0])
        assert apart >= 1, (parts, sem)


@pytest.mark.parametrize("name,family,tag", [("swipe_kbits_16", "k", "all"), ("tile16_l2_40_u8", "k", "all"),
                                             ("swipe_rk_64", "inside", "all"), ("tile16_l2_300_u2", "own", "all"),
                                             ("tile16_l2_40_u8", "shadow", "set0")])
def test_k_in_the_cpu_profile_and_topk(name, family, tag):
    prob, cases, want = pk.build(name, family, tag)
    for sem in SEMS:
        prof, poff = search_profile_cpu(prob, sem)
        at = poff[:-1] + want[:, 1]
        got = np.stack([prof["score"][at], prof["k"][at]], axis=1)
        assert np.array_equal(got, want[:, [0, 2]]), differing(got, want[:, [0, 2]], want[:, 1])
        top = search_topk_cpu(prob, 3, sem)
        assert np.array_equal(top[:, 0], want), differing(top[:, 0], want, want[:, 1])
        if family == "shadow":  # the offset the shadow hides comes second: (W1 L2, p, 0)
            second = want + np.array([0, 1, -1])
            assert np.array_equal(top[:, 1], second), differing(top[:, 1], second, want[:, 1])


# ---- the GPU tier's case lists ------------------------------------------------------------------------------
PROBLEMS = pk.all_problems()


def test_case_lists_cover_the_table():
    names = [r[0] for r in pk.ROWS]
    assert len(set(names)) == len(names)
    for row in pk.ROWS:
        fams = {f for f, _, _ in pk.tie_problems(row)}
        assert fams == {"inside", "own", "shadow"}, row[0]
        L2s = pk.lengths_of(row)
        ks = {(c[1], c[2]) for c in row[3]}
        for L2 in L2s:  # the last k of every length, and every k of the rows that promise it
            assert (L2, L2 - 1) in ks and (L2, 1) in ks
    every = [r for r in pk.ROWS if r[0].startswith(("swipe", "short", "tile16_l2", "tile16_windowed", "tile16_byte",
                                                     "tile16_slide_winwide"))]
    for row in every:
        for L2 in pk.lengths_of(row):
            assert {k for _, l, k in row[3] if l == L2} == set(range(1, L2)), row[0]
    # the wire paths' 129 records and the largest code of a result format
    for row in pk.ROWS:
        if row[5] == ["swipe"]:
            L2 = pk.lengths_of(row)[-1]
            assert (row[1] - L2 - 1, L2, L2 - 1) in row[3]


@pytest.mark.parametrize("name,family,tag", PROBLEMS, ids=["-".join(p) for p in PROBLEMS])
def test_every_claim_of_the_case_lists(name, family, tag):
    prob, cases, want = pk.build(name, family, tag)
    assert prob.n == len(cases) == want.shape[0] > 0
    assert_claim(prob, want, want[:, 1], threads=(0,))


def test_kernel_rules_predict_the_rows_forms():
    # the host's exactness rules (ops.align.kernel_bounds, no GPU needed) choose the arithmetic form the GPU tier
    # asserts, for the planted-k problem of every row and for each of its tie problems
    for name, family, tag in PROBLEMS:
        row = pk.ROW[name]
        prob, _, _ = pk.build(name, family, tag)
        L2 = np.diff(prob.offsets)
        kb = kernel_bounds(row[2], row[1], int(L2.min()), int(L2.max()))
        forms = row[6]
        if row[5] == ["swipe"]:
            assert kb["swipe"] == forms[0], (name, family, tag, kb)
        elif row[5] == ["short"]:
            assert (kb["key_shift"] == 0) == (forms == ["short_key64"]), (name, family, tag, kb)
            assert kb["short_pk"] or forms != ["short_pk"]
        elif row[5] == ["tiles"]:
            assert not kb["profile16"] and not kb["profile16_i16"], (name, family, tag, kb)
            assert (kb["key_shift"] == 0) == (forms == ["tiles_key64"]), (name, family, tag, kb)
        else:
            assert kb["profile16"] == ("tile16_i16" not in forms) and kb["profile16_i16"], (name, family, tag, kb)


def test_case_lists_tell_a_wrong_k_rule_from_the_right_one():
    # planted_k.pick_k picks k on the claimed offset's diagonal pair under a named rule. The product's rule gives
    # the claimed k for every record; every modelled slip gives another k for at least one record — in every row,
    # since every kernel finds k its own way (a dropped carry needs a k past the 64th step to show)
    caught = {}
    for name, family, tag in PROBLEMS:
        prob, cases, want = pk.build(name, family, tag)
        table = score_table(prob.weights)
        for i in range(prob.n):
            o, k = int(want[i, 1]), int(want[i, 2])
            assert pk.pick_k(prob, i, o, "first", table) == k, (name, family, tag, i)
            for rule in pk.RULES[1:]:
                if pk.pick_k(prob, i, o, rule, table) != k:
                    caught.setdefault((name, rule), []).append((family, i))
    for row in pk.ROWS:
        if not any(p[0] == row[0] for p in PROBLEMS):
            continue  # an earlier row's problems under another environment
        for rule in pk.RULES[1:]:
            if rule == "carry_dropped" and pk.lengths_of(row)[-1] <= 65:
                assert (row[0], rule) not in caught  # one pass: nothing to carry
                continue
            assert (row[0], rule) in caught, f"no case of {row[0]} tells the rule '{rule}' from the right one"
    # and each family is there for its own slip: the tie inside an offset for the last k, the tie with the
    # offset's own un-mutated candidate for the >=, the planted k itself for the rest
    fams = lambda rule: {f for (n, r), hits in caught.items() if r == rule for f, _ in hits}  # noqa: E731
    assert "inside" in fams("last") and "own" in fams("ge")
    assert "k" in fams("carry_dropped") and "k" in fams("one_short") and "k" in fams("narrow_field")


# ---- mutants at the exactness bounds ------------------------------------------------------------------------
@pytest.mark.parametrize("shape", pk.EXTREME_SWIPE_AT + pk.EXTREME_OTHER, ids=lambda s: f"{s[0]}_{s[2]}_{s[3][0]}")
def test_extreme_mutants(shape):
    L1, lo, hi, w = shape
    prob, cases = make_extreme_mutants(L1, lo, hi, w, copies=2 if L1 <= 200 else 1, seed=L1)
    assert (prob.seq1 == make_extreme(L1, lo, hi, w).seq1).all()
    want = planted_k_expected(prob, cases, "extreme")
    assert np.array_equal(want[:, 1], cases[:, 0] % 2) and np.array_equal(want[:, 2], cases[:, 2])
    # the same lengths as make_extreme's, so the same rules' answers: the kernel form at each bound is the same
    L2, ex = np.diff(prob.offsets), np.diff(make_extreme(L1, lo, hi, w).offsets)
    assert (L2.min(), L2.max()) == (ex.min(), ex.max()) == (lo, hi)
    assert kernel_bounds(w, L1, int(L2.min()), int(L2.max())) == kernel_bounds(w, L1, int(ex.min()), int(ex.max()))
    if (w[0] == w[3]) and L1 <= 200:
        # the winner's D(k) = 2 W k: with k = L2 - 1 one step under the bound's 2 W L2, beside the smallest k field
        i = int(np.nonzero((cases[:, 1] == hi - (hi == L1)) & (cases[:, 2] == cases[:, 1] - 1))[0][0])
        table = score_table(w).astype(np.int64)
        r = prob.codes[prob.offsets[i]:prob.offsets[i + 1]].astype(np.int64)
        o, n = int(want[i, 1]), r.shape[0]
        s1 = prob.seq1.astype(np.int64)
        D = np.cumsum(table[r, s1[o:o + n]] - table[r, s1[o + 1:o + n + 1]])
        assert D[n - 2] == 2 * w[0] * (n - 1) == D.max()
    for sem in SEMS:
        if shape in pk.EXTREME_SWIPE_AT:
            ref = as_triples(brute_force_native(prob, sem))
            assert np.array_equal(ref, want), differing(ref, want, cases[:, 0])
        oracle = solve_problem(prob, sem, oracle=prefix_oracle)
        assert np.array_equal(oracle, want), differing(oracle, want, cases[:, 0])
        got = as_triples(search_cpu(prob, sem))
        assert np.array_equal(got, want), differing(got, want, cases[:, 0])
