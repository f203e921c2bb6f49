"""Per-target distinct placements on the CPU engine (csrc/src/cpu_engine.cpp targets_topk_batch_cpu /
targets_hits_batch_cpu with a radius): the oracle of the GPU tier, anchored here. Every pair of seeded batches is
compared with search_topk_cpu / search_hits_cpu with the same radius run on the target alone — functions that never see
the catalog. Then the fixed properties (T = 1, radius = 0, row 0, one peak past the profile's length, runs of equal
scores, the boundary entry's tie, 10 9 8), the planted and the straddling record by name, the capacity contract over
poisoned buffers, `within`, every error prefix and their order, --target-distinct through the CLI at one and two
ranks with its refusals, DistributedSearch, targets_catalog_rows on top-K rows, a numpy model of the shortcut (the
catalog-wide filter's marks cut to each slice) that must disagree with the expected marks on every case list the GPU
tier uses to test clipping, and the stand-alone sanitizer program."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, input_path
from test_dist import torchrun
from targets_peaks_cases import (CLIPPING_CASES, I32, W, batch_of, count_disagreements, expected_masks, hostile_case,
                                 pair_counts, shortcut_masks, window_peaks)

from mpi_openmp_cuda_amd import (Problem, Semantics, TargetSet, _lib, format_targets_hits, format_targets_topk,
                                 search_hits_cpu, search_profile_cpu, search_report_cpu, search_targets_cpu,
                                 search_targets_hits_cpu, search_targets_topk_cpu, search_topk_cpu, targets_catalog_rows)

SEMS = [Semantics.REFERENCE, Semantics.SPEC]
RADII = [1, 2, 3, 40, 2048]
NONE = [I32.min, 0, 0]
A, B = 1, 2


def seeded_case(rng, T, alphabet):
    """n records and T targets: around the record lengths (L2 - 1, L2, L2 + 1: pairs that do not fit, len == L2), a
    single letter and a long one; the last target is exactly as long as record 0."""
    lens = rng.integers(1, 14, size=5)
    recs = [rng.integers(1, alphabet + 1, size=int(l)).astype(np.uint8) for l in lens]
    pool = [1, int(rng.integers(40, 90))] + [max(int(l) + d, 1) for l in lens for d in (-1, 0, 1)]
    tl = [int(x) for x in rng.choice(pool, T)]
    tl[-1] = int(lens[0])
    ts = TargetSet.from_sequences([rng.integers(1, alphabet + 1, size=l).astype(np.uint8) for l in tl])
    return ts, recs


def pair_hits(rows, toffsets, T, i, t):
    p = i * T + t
    return rows[toffsets[p]:toffsets[p + 1]]


def check_against_targets_alone(w, ts, codes, offsets, sem, K, R, **thr):
    n = offsets.shape[0] - 1
    catalog = Problem(w, ts.seq1, codes, offsets)
    topk = search_targets_topk_cpu(catalog, ts, K, sem, radius=R)
    assert topk.dtype == np.int32 and topk.shape == (n, ts.T, K, 3)
    rows, toffsets = search_targets_hits_cpu(catalog, ts, semantics=sem, radius=R, **thr)
    assert toffsets.dtype == np.int64 and toffsets.shape == (n * ts.T + 1,) and toffsets[0] == 0
    assert rows.dtype == np.int32 and rows.shape == (toffsets[-1], 3)
    for t in range(ts.T):
        alone = Problem(w, ts.target(t), codes, offsets)
        assert np.array_equal(topk[:, t], search_topk_cpu(alone, K, sem, radius=R)), (t, R, "top-K")
        want, h = search_hits_cpu(alone, semantics=sem, radius=R, **thr)
        for i in range(n):
            assert np.array_equal(pair_hits(rows, toffsets, ts.T, i, t), want[h[i]:h[i + 1]]), (i, t, R, "hits")
    return topk, rows, toffsets


# ---- the oracle is anchored --------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("seed", range(3))
def test_every_pair_equals_the_distinct_calls_on_the_target_alone(sem, T, seed):
    rng = np.random.default_rng(500 + 10 * T + seed)
    ts, recs = seeded_case(rng, T, (2, 4, 26)[seed])
    codes, offsets = batch_of(recs)
    best = search_targets_cpu(Problem(list(W), ts.seq1, codes, offsets), ts, sem)
    for R in RADII:
        topk, rows, toffsets = check_against_targets_alone(list(W), ts, codes, offsets, sem, 4, R, min_score=-6)
        assert np.array_equal(topk[:, :, 0], best), R  # row 0 is the multi-target search's row at every radius
        check_against_targets_alone(list(W), ts, codes, offsets, sem, 1, R, within=5)


@pytest.mark.parametrize("sem", SEMS)
def test_radius_0_is_the_call_without_it(sem):
    rng = np.random.default_rng(41)
    ts, recs = seeded_case(rng, 4, 4)
    codes, offsets = batch_of(recs)
    prob = Problem(list(W), ts.seq1, codes, offsets)
    assert np.array_equal(search_targets_topk_cpu(prob, ts, 5, sem, radius=0), search_targets_topk_cpu(prob, ts, 5, sem))
    for a, b in zip(search_targets_hits_cpu(prob, ts, min_score=-3, semantics=sem, radius=0),
                    search_targets_hits_cpu(prob, ts, min_score=-3, semantics=sem)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("sem", SEMS)
def test_a_radius_past_the_profile_leaves_one_peak_per_fitting_pair(sem):
    rng = np.random.default_rng(43)
    ts, recs = seeded_case(rng, 5, 3)
    codes, offsets = batch_of(recs)
    prob = Problem(list(W), ts.seq1, codes, offsets)
    counts = pair_counts(prob, ts, sem)
    best = search_targets_cpu(prob, ts, sem)
    for R in (int(counts.max()) - 1, 2048):
        rows, toffsets = search_targets_hits_cpu(prob, ts, min_score=int(I32.min), semantics=sem, radius=R)
        assert np.array_equal(np.diff(toffsets), (counts.reshape(-1) > 0).astype(np.int64))
        assert np.array_equal(rows, best.reshape(-1, 3)[counts.reshape(-1) > 0])
        topk = search_targets_topk_cpu(prob, ts, 3, sem, radius=R)
        assert np.array_equal(topk[:, :, 0], best) and (topk[:, :, 1:] == NONE).all()


def one_letter_problem(targets, sem_unused=None):
    """A record of the single letter A: its score at an offset is 4 on an A and less elsewhere, and no mutant exists."""
    ts = TargetSet.from_sequences(targets)
    codes, offsets = batch_of([[A]])
    return Problem(list(W), ts.seq1, codes, offsets), ts


@pytest.mark.parametrize("sem", SEMS)
def test_a_run_of_equal_scores_keeps_its_first_offset(sem):
    run = np.full(30, B, np.uint8)
    run[10:17] = A
    prob, ts = one_letter_problem([np.full(9, B, np.uint8), run])
    for R in (1, 3, 40):
        rows, toffsets = search_targets_hits_cpu(prob, ts, min_score=4, semantics=sem, radius=R)
        assert rows.tolist() == [[4, 10, 0]] and toffsets.tolist() == [0, 0, 1]
        flat, _ = search_targets_hits_cpu(prob, ts, min_score=int(I32.min), semantics=sem, radius=R)
        assert flat[0].tolist()[1] == 0  # target 0: equal scores throughout, offset 0 first


def test_a_boundary_entry_that_ties_a_slice_entry_loses_to_it():
    """AAAAA against a target that ends in six A's: the last slice entry and the boundary entry both score a full
    match; the smaller offset wins, so the boundary entry is no peak at any radius >= 1."""
    t = np.full(30, B, np.uint8)
    t[24:] = A
    ts = TargetSet.from_sequences([np.full(8, B, np.uint8), t])
    codes, offsets = batch_of([np.full(5, A, np.uint8)])
    prob = Problem(list(W), ts.seq1, codes, offsets)
    plain, _ = search_targets_hits_cpu(prob, ts, min_score=20, semantics=Semantics.SPEC)
    assert plain.tolist() == [[20, 24, 0], [20, 25, 0]]
    for R in (1, 5, 40):
        rows, _ = search_targets_hits_cpu(prob, ts, min_score=20, semantics=Semantics.SPEC, radius=R)
        assert rows.tolist() == [[20, 24, 0]], R
        assert search_targets_topk_cpu(prob, ts, 2, Semantics.SPEC, radius=R)[0, 1].tolist()[0] == [20, 24, 0]


def test_scores_10_9_8_at_radius_1_keep_the_10_alone():
    """Ten A's against a target of ten A's and then B's, one point per equal letter: the scores run 10 9 8 7 ... from
    offset 0. At R = 1 the 10 alone is a peak: it suppresses the 9, and the 9 — no peak itself — still suppresses
    the 8 (local-maximum suppression, not a greedy one)."""
    t = np.full(24, B, np.uint8)
    t[:10] = A
    ts = TargetSet.from_sequences([np.full(11, B, np.uint8), t])
    codes, offsets = batch_of([np.full(10, A, np.uint8)])
    prob = Problem([1, 0, 0, 0], ts.seq1, codes, offsets)
    prof, toffsets = search_targets_hits_cpu(prob, ts, min_score=int(I32.min), semantics=Semantics.SPEC)
    assert pair_hits(prof, toffsets, 2, 0, 1)[:4, 0].tolist() == [10, 9, 8, 7]
    rows, toffsets = search_targets_hits_cpu(prob, ts, min_score=1, semantics=Semantics.SPEC, radius=1)
    assert rows.tolist() == [[10, 0, 0]] and toffsets.tolist() == [0, 0, 1]
    assert search_targets_topk_cpu(prob, ts, 3, Semantics.SPEC, radius=1)[0, 1, 0].tolist() == [10, 0, 0]


# ---- named cases -------------------------------------------------------------------------------------------
def planted_case():
    rng = np.random.default_rng(7)
    t1 = rng.integers(1, 21, size=300).astype(np.uint8)
    t2 = rng.integers(1, 21, size=200).astype(np.uint8)
    rec = rng.integers(1, 21, size=40).astype(np.uint8)
    t1[100:140] = rec
    t1[220:260] = rec
    rec = rec.copy()
    for at in (5, 14, 23, 32):  # 4 letters changed: the planted copies are no full matches
        rec[at] = rec[at] % 20 + 1
    ts = TargetSet.from_sequences([t1, t2])
    codes, offsets = batch_of([rec])
    return Problem(list(W), ts.seq1, codes, offsets), ts


def test_planted_record_drops_its_shadows():
    """A 40-letter record planted at offsets 100 and 220 of a 300-letter target next to a 200-letter one: without a
    radius the per-target top-4 of target 1 holds each placement and its shadow at n - 1 with k = 1; with radius 1 the
    shadows are gone, and the hits within 20 are exactly the two placements."""
    prob, ts = planted_case()
    plain = search_targets_topk_cpu(prob, ts, 4)[0, 0]
    assert plain[:2, 1].tolist() == [100, 220] and sorted(plain[2:, 1].tolist()) == [99, 219] and plain[2:, 2].tolist() == [1, 1]
    top = search_targets_topk_cpu(prob, ts, 4, radius=1)
    assert top[0, 0, :2, 1].tolist() == [100, 220] and not {99, 219} & set(top[0, 0, :, 1].tolist())
    alone = Problem(list(W), ts.target(0), prob.codes, prob.offsets)
    assert np.array_equal(top[0, 0], search_topk_cpu(alone, 4, radius=1)[0])
    rows, toffsets = search_targets_hits_cpu(prob, ts, within=20, radius=1)
    assert pair_hits(rows, toffsets, 2, 0, 0)[:, 1].tolist() == [100, 220]
    assert np.array_equal(top[0, 1], search_topk_cpu(Problem(list(W), ts.target(1), prob.codes, prob.offsets), 4, radius=1)[0])


def test_straddling_record_suppresses_nothing():
    """Two random 60-letter targets, the record the last 20 letters of the first and the first 20 of the second: on the
    hand-made catalog the straddling placement (160, 40, 0) — in neither target — suppresses everything within 20
    offsets on both sides; per target, each target's own peaks come back."""
    rng = np.random.default_rng(2024)
    t1, t2 = (rng.integers(1, 27, size=60).astype(np.uint8) for _ in range(2))
    ts = TargetSet.from_sequences([t1, t2])
    codes, offsets = batch_of([np.concatenate([t1[40:], t2[:20]])])
    prob = Problem(list(W), ts.seq1, codes, offsets)
    for sem in SEMS:
        by_hand = search_topk_cpu(prob, 3, sem, radius=20)[0]
        assert by_hand[0].tolist() == [160, 40, 0]
        top = search_targets_topk_cpu(prob, ts, 3, sem, radius=20)
        assert 160 not in top[:, :, :, 0]
        for t in range(2):
            alone = search_topk_cpu(Problem(list(W), ts.target(t), codes, offsets), 3, sem, radius=20)[0]
            assert np.array_equal(top[0, t], alone)
        assert (top[0, :, 0, 1] + 40 <= 60).all()


# ---- contracts ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_capacity_contract_over_poisoned_buffers(sem):
    rng = np.random.default_rng(47)
    ts, recs = seeded_case(rng, 4, 4)
    codes, offsets = batch_of(recs)
    prob = Problem(list(W), ts.seq1, codes, offsets)
    R, thr = 2, -4
    want, woff = search_targets_hits_cpu(prob, ts, min_score=thr, semantics=sem, radius=R)
    total, pairs = int(woff[-1]), prob.n * ts.T
    inside = next(int(woff[p]) + 1 for p in range(pairs) if woff[p + 1] - woff[p] >= 2)
    POISON = -777
    for cap in (0, 1, inside, total - 1, total):
        rows = np.full((total + 4, 3), POISON, np.int32)
        toffsets = np.full(pairs + 3, POISON, np.int64)
        rc = _lib.lib().moc_cpu_targets_hits_distinct(
            _lib.weights_arg(list(W)), _lib.ptr(prob.seq1), prob.L1, _lib.ptr(prob.codes), _lib.ptr(prob.offsets), prob.n,
            _lib.ptr(ts.starts), ts.T, int(sem), 0, thr, None, R, toffsets[1:].ctypes.data, _lib.ptr(rows) if cap else None, cap)
        assert rc == 0
        assert np.array_equal(toffsets[1:-1], woff) and toffsets[0] == POISON and toffsets[-1] == POISON, cap
        assert np.array_equal(rows[:cap], want[:cap]) and (rows[cap:] == POISON).all(), cap
    assert total >= 4 and 0 < inside < total


@pytest.mark.parametrize("sem", SEMS)
def test_within_against_thresholds_built_by_hand(sem):
    rng = np.random.default_rng(49)
    ts, recs = seeded_case(rng, 3, 4)
    codes, offsets = batch_of(recs)
    prob = Problem(list(W), ts.seq1, codes, offsets)
    D, R = 6, 3
    best = search_targets_cpu(prob, ts, sem)[:, :, 0].astype(np.int64)
    by_hand = np.clip(best - D, I32.min, I32.max).astype(np.int32)
    want = search_targets_hits_cpu(prob, ts, thresholds=by_hand, semantics=sem, radius=R)
    got = search_targets_hits_cpu(prob, ts, within=D, semantics=sem, radius=R)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (np.diff(got[1]) >= (best.reshape(-1) != I32.min)).all()  # the best entry of a pair is always a peak


def test_error_prefixes_and_their_order():
    prob, ts = hostile_case([3, 9], Semantics.SPEC)
    bad_starts = [1, prob.L1]
    with pytest.raises(ValueError, match="^targets:"):
        search_targets_topk_cpu(prob, bad_starts, 0, radius=-1)
    with pytest.raises(ValueError, match="^targets:"):
        search_targets_hits_cpu(prob, bad_starts, radius=-1)
    with pytest.raises(ValueError, match="^top-K: K must be in 1..64"):
        search_targets_topk_cpu(prob, ts, 65, radius=-1)
    with pytest.raises(ValueError, match="^hits: give exactly one"):
        search_targets_hits_cpu(prob, ts, min_score=0, within=0, radius=-1)
    with pytest.raises(ValueError, match="^hits: within must be"):
        search_targets_hits_cpu(prob, ts, within=-1, radius=-1)
    with pytest.raises(ValueError, match="^hits: thresholds must be"):
        search_targets_hits_cpu(prob, ts, thresholds=np.zeros((3, 3), np.int32), radius=-1)
    for bad in (-1, 2049, 1.0, True, None):
        with pytest.raises(ValueError, match="^distinct: radius must be"):
            search_targets_topk_cpu(prob, ts, 2, radius=bad)
        for thr in ({"min_score": 0}, {"within": 2}):
            with pytest.raises(ValueError, match="^distinct: radius must be"):
                search_targets_hits_cpu(prob, ts, radius=bad, **thr)
    # the C ABI itself: the target set, then K / the buffers, then the radius
    out = np.zeros((prob.n, ts.T, 2, 3), np.int32)
    toffsets = np.zeros(prob.n * ts.T + 1, np.int64)

    def topk(starts, K, R):
        starts = np.asarray(starts, np.int64)
        rc = _lib.lib().moc_cpu_targets_topk_distinct(_lib.weights_arg(list(W)), _lib.ptr(prob.seq1), prob.L1,
                                                      _lib.ptr(prob.codes), _lib.ptr(prob.offsets), prob.n, _lib.ptr(starts),
                                                      starts.shape[0] - 1, 1, 0, K, R, _lib.ptr(out))
        return rc, _lib.lib().moc_last_error().decode()

    def hits(starts, cap, R):
        starts = np.asarray(starts, np.int64)
        rc = _lib.lib().moc_cpu_targets_hits_distinct(_lib.weights_arg(list(W)), _lib.ptr(prob.seq1), prob.L1,
                                                      _lib.ptr(prob.codes), _lib.ptr(prob.offsets), prob.n, _lib.ptr(starts),
                                                      starts.shape[0] - 1, 1, 0, 0, None, R, _lib.ptr(toffsets), None, cap)
        return rc, _lib.lib().moc_last_error().decode()

    for call, prefix in ((topk(bad_starts, 0, -1), "targets:"), (topk(ts.starts, 0, -1), "top-K:"),
                         (topk(ts.starts, 2, -1), "distinct:"), (topk(ts.starts, 2, 2049), "distinct:"),
                         (hits(bad_starts, 3, -1), "targets:"), (hits(ts.starts, 3, -1), "hits:"),
                         (hits(ts.starts, 0, 2049), "distinct:")):
        assert call[0] != 0 and call[1].startswith(prefix), (call, prefix)
    assert topk(ts.starts, 2, 2048)[0] == 0 and hits(ts.starts, 0, 0)[0] == 0


# ---- targets_catalog_rows on top-K rows ----------------------------------------------------------------------
def test_targets_catalog_rows_takes_topk_rows_and_feeds_the_report():
    prob, ts = planted_case()
    K = 3
    top = search_targets_topk_cpu(prob, ts, K, radius=1)
    moved = targets_catalog_rows(top, ts)
    assert moved.shape == top.shape and moved.dtype == np.int32 and moved is not top
    for i in range(prob.n):
        for t in range(ts.T):
            for j in range(K):
                s, n, k = top[i, t, j].tolist()
                assert moved[i, t, j].tolist() == ([s, n, k] if s == I32.min else [s, n + int(ts.starts[t]), k])
    assert (moved[top[:, :, :, 0] == I32.min] == NONE).all()
    assert np.array_equal(targets_catalog_rows(top[:, :, 0], ts), moved[:, :, 0])  # the [n, T, 3] form is unchanged
    report = search_report_cpu(prob, moved.reshape(prob.n, ts.T * K, 3))
    counts = report[0] if isinstance(report, tuple) else report
    assert np.asarray(counts).shape[:2] == (prob.n, ts.T * K)
    torch = pytest.importorskip("torch")
    assert np.array_equal(targets_catalog_rows(torch.from_numpy(top), ts).numpy(), moved)
    assert np.array_equal(targets_catalog_rows(torch.from_numpy(top[:, :, 0].copy()), ts.starts).numpy(), moved[:, :, 0])
    with pytest.raises(ValueError):
        targets_catalog_rows(top[:, :1], ts)
    with pytest.raises(ValueError):
        targets_catalog_rows(top.reshape(prob.n, ts.T * K, 3), ts)


# ---- the shortcut is told from the definition ----------------------------------------------------------------
def test_window_model_is_the_peak_filter():
    rng = np.random.default_rng(53)
    rec = rng.integers(1, 5, 4).astype(np.uint8)
    prob = Problem(list(W), rng.integers(1, 5, 90).astype(np.uint8), rec, np.array([0, 4], np.int64))
    prof, _ = search_profile_cpu(prob, Semantics.SPEC)
    for R in (1, 3, 40):
        rows, _ = search_hits_cpu(prob, min_score=int(I32.min), semantics=Semantics.SPEC, radius=R)
        assert np.flatnonzero(window_peaks(prof["score"], R)).tolist() == rows[:, 1].tolist()


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("name", list(CLIPPING_CASES))
def test_shortcut_disagrees_on_every_clipping_case_list(sem, name):
    """The catalog-wide filter's marks cut to each slice are NOT the pairs' own marks on the case lists the GPU tier
    runs: at every radius of every list the two differ on at least one pair, so a kernel whose windows leak across a
    target edge, or that reads the catalog's value at the boundary offset, cannot pass there."""
    sizes, radii = CLIPPING_CASES[name]
    prob, ts = hostile_case(sizes, sem)
    for R in radii:
        differ, fitting = count_disagreements(prob, ts, sem, R)
        assert fitting == len(sizes) + 2 and differ >= 1, (name, R, differ, fitting)


def test_shortcut_disagreements_on_seeded_small_cases():
    """200 seeded cases of 3 targets of 6..29 letters and a 5-letter record over 4 letters under the spec semantics, R
    in {1, 3}: the count of (pair, R) cases on which the shortcut's marks differ, recomputed here; a sizeable share."""
    differ = total = 0
    for seed in range(200):
        rng = np.random.default_rng(seed)
        ts = TargetSet.from_sequences([rng.integers(1, 5, int(rng.integers(6, 30))).astype(np.uint8) for _ in range(3)])
        codes, offsets = batch_of([rng.integers(1, 5, 5).astype(np.uint8)])
        prob = Problem(list(W), ts.seq1, codes, offsets)
        for R in (1, 3):
            want, cut = expected_masks(prob, ts, Semantics.SPEC, R), shortcut_masks(prob, ts, Semantics.SPEC, R)
            differ += sum(0 if np.array_equal(want[p], cut[p]) else 1 for p in want)
            total += len(want)
    assert total == 1200 and differ >= 120, (differ, total)  # at least one pair in ten


# ---- the CLI -------------------------------------------------------------------------------------------------
def _cli(args, i):
    with open(input_path(i), "rb") as f:
        return subprocess.run([sys.executable, "-m", "mpi_openmp_cuda_amd", "--backend=cpu"] + args, stdin=f,
                              capture_output=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd="/tmp", timeout=120)


def cli_targets_file(tmp_path, prob):
    lines = [prob.seq1_str()[3:3 + max(prob.L1 // 2, 1)], "Q", prob.record(0), ""]
    path = tmp_path / "targets.txt"
    path.write_text("\n".join(lines))
    ts = TargetSet.from_strings([prob.seq1_str()] + lines[:3])
    return str(path), ts, Problem(prob.weights, ts.seq1, prob.codes, prob.offsets)


def want_topk(catalog, ts, K, R):
    topk = search_targets_topk_cpu(catalog, ts, K, radius=R)
    return format_targets_topk(topk[:, 0, 0], topk)


def want_hits(catalog, ts, R, **thr):
    rows = search_targets_cpu(catalog, ts)
    return format_targets_hits(rows[:, 0], rows, *search_targets_hits_cpu(catalog, ts, radius=R, **thr))


@pytest.mark.parametrize("i", [1, 6])
def test_cli_target_distinct(tmp_path, i):
    prob = Problem.read(input_path(i))
    path, ts, catalog = cli_targets_file(tmp_path, prob)
    for args, want, plain in ((["--target-top", "3"], want_topk(catalog, ts, 3, 2), want_topk(catalog, ts, 3, 0)),
                              (["--target-within", "20"], want_hits(catalog, ts, 2, within=20), want_hits(catalog, ts, 0, within=20)),
                              (["--target-min-score=-5"], want_hits(catalog, ts, 2, min_score=-5), want_hits(catalog, ts, 0, min_score=-5))):
        r = _cli(["--targets", path, "--target-distinct", "2"] + args, i)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert r.stdout.decode() == want, args
        if "--target-top" not in args:  # hits: the same lines, fewer of them (top-K fills up with weaker peaks)
            assert len(want.splitlines()) < len(plain.splitlines()), args
            assert set(want.splitlines()) <= set(plain.splitlines()), args
        assert want != plain
    # R = 0 prints what no flag prints, byte for byte
    r0 = _cli(["--targets", path, "--target-distinct", "0", "--target-within", "20"], i)
    none = _cli(["--targets", path, "--target-within", "20"], i)
    assert r0.returncode == 0 and none.returncode == 0 and r0.stdout == none.stdout
    assert none.stdout.decode() == want_hits(catalog, ts, 0, within=20)


def test_cli_target_distinct_two_gloo_ranks(tmp_path):
    prob = Problem.read(input_path(3))
    path, ts, catalog = cli_targets_file(tmp_path, prob)
    for args, want in ((["--target-top", "4"], want_topk(catalog, ts, 4, 3)),
                       (["--target-within", "20"], want_hits(catalog, ts, 3, within=20))):
        r = torchrun(2, ["--backend=cpu", "--dist-backend=gloo", "--targets", path, f"--input={input_path(3)}",
                         "--target-distinct", "3"] + args)
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        assert r.stdout.decode() == want, args


@pytest.mark.parametrize("args", [
    ["--target-distinct", "2"], ["--target-distinct", "2", "--top", "3"],  # needs --targets
    ["--targets", "FILE", "--target-distinct", "2"],  # ... and one of the three
    ["--targets", "FILE", "--target-distinct", "2", "--target-top", "1"],  # K > 1
    ["--targets", "FILE", "--target-distinct", "2", "--target-summary"],
    ["--targets", "FILE", "--target-distinct=-1", "--target-top", "3"],
    ["--targets", "FILE", "--target-distinct", "2049", "--target-within", "3"],
    ["--targets", "FILE", "--distinct", "2", "--target-top", "3"],  # --distinct with --targets stays refused
    ["--targets", "FILE", "--distinct", "2", "--target-distinct", "2", "--target-top", "3"],
    ["--targets", "FILE", "--target-distinct", "2", "--target-top", "3", "--target-within", "3"],
    ["--targets", "FILE", "--target-distinct", "2", "--target-top", "3", "--partition", "offsets"]])
def test_cli_refusals(tmp_path, args):
    prob = Problem.read(input_path(6))
    path, _, _ = cli_targets_file(tmp_path, prob)
    r = _cli([path if a == "FILE" else a for a in args], 6)
    assert r.returncode != 0 and r.stdout == b"" and r.stderr != b""


def test_distributed_search_on_one_process():
    from mpi_openmp_cuda_amd.parallel import dist as D
    from mpi_openmp_cuda_amd.parallel.search import DistributedSearch

    rng = np.random.default_rng(37)
    ts, recs = seeded_case(rng, 4, 4)
    codes, offsets = batch_of(recs)
    prob = Problem(list(W), ts.seq1, codes, offsets)
    s = DistributedSearch(D.DistContext(), backend="cpu", partition="records")
    topk = s.run_targets_topk(prob, ts, 5, Semantics.SPEC, radius=2)
    assert topk.dtype == np.int32 and np.array_equal(topk, search_targets_topk_cpu(prob, ts, 5, Semantics.SPEC, radius=2))
    for kw in ({"min_score": -3}, {"within": 6}):
        best, rows, toffsets = s.run_targets_hits(prob, ts, semantics=Semantics.SPEC, radius=2, **kw)
        want, woff = search_targets_hits_cpu(prob, ts, semantics=Semantics.SPEC, radius=2, **kw)
        assert np.array_equal(best, search_targets_cpu(prob, ts, Semantics.SPEC))
        assert rows.dtype == np.int32 and np.array_equal(rows, want) and np.array_equal(toffsets, woff)
    with pytest.raises(ValueError, match="^targets:"):
        s.run_targets_topk(prob, ts.starts[:-1], 0, radius=-1)
    with pytest.raises(ValueError, match="^top-K:"):
        s.run_targets_topk(prob, ts, 65, radius=-1)
    with pytest.raises(ValueError, match="^distinct:"):
        s.run_targets_topk(prob, ts, 2, radius=2049)
    with pytest.raises(ValueError, match="^hits: give exactly one"):
        s.run_targets_hits(prob, ts, radius=-1)
    with pytest.raises(ValueError, match="^distinct:"):
        s.run_targets_hits(prob, ts, min_score=0, radius=-1)


# ---- stand-alone sanitizer program -------------------------------------------------------------------------
def test_targets_peaks_sanitizer_program():
    """csrc/tests/targets_peaks_san.cpp with the CPU core sources under ASan + UBSan: a plain program with its own main
    (nothing is loaded into Python, nothing runs on a GPU)."""
    r = subprocess.run(["make", "-C", ROOT, "-s", "-j8", "targets-peaks-san"], capture_output=True, timeout=600)
    out = (r.stdout + r.stderr).decode()
    assert r.returncode == 0, out[-3000:]
    assert "targets_peaks_san ok" in out and "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]
