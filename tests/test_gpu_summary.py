"""GPU (MI355X / gfx950) tests of the profile-summary kernels (csrc/src/hip/summary_kernels.hip): the summary rows
and histograms exactly equal to the CPU engine's (tests/test_summary_cpu.py anchors that one to a letter-by-letter
replay) under both semantics, at the smallest shapes that reach each edge — single-pass and multi-pass records,
the records-per-block boundaries, ties, the histogram's bin edges, int64 arithmetic next to 2^63 and its refusal one
entry later, chunks under the scratch bound, the device form on a side stream feeding thresholds to hits, the wire
form and empty batches. Every call must report the summary and profile kernels in its stats."""
import numpy as np
import pytest

from conftest import gpu_available, input_path

pytestmark = pytest.mark.gpu

if not gpu_available():  # pragma: no cover - collected on CPU hosts only with -m gpu
    pytest.skip("no GPU", allow_module_level=True)

import torch  # noqa: E402

from mpi_openmp_cuda_amd import (HipSearchEngine, Problem, Semantics, WireSlice, align_summary_device,  # noqa: E402
                                 make_synthetic, search_hits_cpu, search_summary_cpu, summary_thresholds)
from mpi_openmp_cuda_amd.ops.align import as_triples, summary_geometry  # noqa: E402

SEMS = [Semantics.REFERENCE, Semantics.SPEC]
W = (10, 2, 3, 4)
DEV = torch.device("cuda:0")
I32 = np.iinfo(np.int32)
EMPTY_ROW = [0, 0, 0, I32.max, I32.min, 0, 0]

_engine = []


@pytest.fixture
def engine():
    if not _engine:
        _engine.append(HipSearchEngine(device=0))
    return _engine[0]


@pytest.fixture(scope="module", autouse=True)
def _close_engine():
    yield
    for e in _engine:
        e.close()
    _engine.clear()


def problem_of(weights, seq1, recs) -> Problem:
    lens = np.array([len(r) for r in recs], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return Problem(list(weights), np.asarray(seq1, np.uint8), np.concatenate([np.asarray(r, np.uint8) for r in recs]),
                   offsets)


def random_problem(L1, lens, weights=W, seed=0) -> Problem:
    rng = np.random.default_rng(seed)
    return problem_of(weights, rng.integers(1, 27, L1), [rng.integers(1, 27, l) for l in lens])


_oracle = {}


def oracle(key, prob, sem, bins=0, lo=0, width=1):
    """The CPU engine's (summary, hist) of a shared problem: computed once, read-only."""
    k = (key, sem, bins, lo, width)
    if k not in _oracle:
        s, h = search_summary_cpu(prob, bins, lo, width, semantics=sem)
        s.setflags(write=False)
        if h is not None:
            h.setflags(write=False)
        _oracle[k] = (s, h)
    return _oracle[k]


def same(got, want, what):
    bad = np.flatnonzero((np.asarray(got) != np.asarray(want)).reshape(len(want), -1).any(axis=1))
    assert bad.size == 0, (what, bad[:8], np.asarray(got)[bad[:4]], np.asarray(want)[bad[:4]])


def check(eng, key, prob, sem, bins=0, lo=0, width=1):
    """Host form against the oracle; returns (summary, hist)."""
    want_s, want_h = oracle(key, prob, sem, bins, lo, width)
    eng.set_problem(prob.weights, prob.seq1, sem)
    s, h = eng.solve_summary(prob.codes, prob.offsets, bins, lo, width)
    st = eng.stats()
    assert "summary" in st["kernels"] and "profile" in st["kernels"], st
    assert s.dtype == np.int64 and s.shape == (prob.n, 7)
    same(s, want_s, "summary")
    if bins:
        assert h.dtype == np.int32 and h.shape == (prob.n, bins)
        same(h, want_h, "hist")
        assert np.array_equal(h.sum(axis=1), s[:, 0])
    else:
        assert h is None
    return s, h


# ---- pass edges ----------------------------------------------------------------------------------------------
PASS_L1 = 200
# C = 0, 1, 2, 63, 64, 65, 127, 128, 129, 199 under either semantics (C = L1 - L2, one more under spec)
PASS_LENS = [201, 200, 199, 198, 138, 137, 136, 135, 74, 73, 72, 71, 2, 1]
PASS_C = {0, 1, 2, 63, 64, 65, 127, 128, 129, 199}


@pytest.mark.parametrize("sem", SEMS)
def test_pass_edges(engine, sem):
    prob = random_problem(PASS_L1, PASS_LENS, seed=1)
    s, h = check(engine, "pass", prob, sem, 16, -400, 50)
    assert PASS_C <= set(s[:, 0].tolist())
    assert s[0].tolist() == EMPTY_ROW and not h[0].any()  # C = 0
    # one record of about 1000 offsets: 16 passes of the wave
    long = random_problem(1100, [100], seed=2)
    s, _ = check(engine, "multipass", long, sem, 16, -400, 50)
    assert s[0, 0] in (1000, 1001)


# ---- records per block -----------------------------------------------------------------------------------------
G = summary_geometry()[0]


def tiny_records(n, seed):
    """n records of 1..4 letters against an 8-letter Seq1, built without a Python loop."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 5, n)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return Problem(list(W), rng.integers(1, 27, 8).astype(np.uint8),
                   rng.integers(1, 27, int(offsets[-1])).astype(np.uint8), offsets)


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("n", sorted({1, G - 1, G, G + 1, 3 * G + 1} - {0}))
def test_records_per_block_edges(engine, n, sem):
    check(engine, ("block", n), tiny_records(n, seed=3), sem, 5, -10, 8)


# ---- ties ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_all_equal_letters(engine, sem):
    a = np.ones(80, np.uint8)
    prob = problem_of(W, a, [a[:l] for l in (1, 5, 79)])
    s, h = check(engine, "ones", prob, sem, 3, 0, 30)  # 10 -> bin 0, 50 -> bin 1, 790 -> the last bin
    spec = 1 if sem == Semantics.SPEC else 0
    assert s[:, 0].tolist() == [79 + spec, 75 + spec, 1 + spec]
    assert (s[:, 3] == s[:, 4]).all() and s[:, 4].tolist() == [10, 50, 790]
    assert not s[:, 5].any() and not s[:, 6].any()  # every score equal: n = 0, k = 0
    assert h.tolist() == [[79 + spec, 0, 0], [0, 75 + spec, 0], [0, 0, 1 + spec]]  # 64 lanes on one bin


@pytest.mark.parametrize("sem", SEMS)
def test_equal_maxima_in_different_passes(engine, sem):
    rng = np.random.default_rng(4)
    seq1 = rng.integers(1, 27, 300)
    piece = seq1[10:40].copy()
    seq1[150:180] = piece  # the record's best score at offsets 10 (pass 0) and 150 (pass 2)
    prob = problem_of(W, seq1, [piece])
    s, _ = check(engine, "twice", prob, sem)
    assert s[0, 4:7].tolist() == [300, 10, 0]
    engine.set_problem(prob.weights, prob.seq1, sem)
    prof, _ = engine.solve_profile(prob.codes, prob.offsets)
    assert prof["score"][150] == 300 == prof["score"][10]


# ---- histogram edges -----------------------------------------------------------------------------------------
def negative_score_problem():
    """One record of 300 offsets (301 under spec) with negative and positive scores: weights (1, 5, 5, 5) and a
    planted copy."""
    rng = np.random.default_rng(9)
    seq1 = rng.integers(1, 27, 320)
    return problem_of((1, 5, 5, 5), seq1, [seq1[100:120].copy()])


@pytest.mark.parametrize("sem", SEMS)
def test_histogram_edges(engine, sem):
    prob = negative_score_problem()
    s0, _ = oracle("neg", prob, sem)
    lo_s, hi_s = int(s0[0, 3]), int(s0[0, 4])
    assert s0[0, 0] in (300, 301) and lo_s < 0 < hi_s
    los = [int(I32.min), lo_s - 1000, hi_s + 1000, (lo_s + hi_s) // 2, min(lo_s + 3, -1), int(I32.max)]
    for bins in (1, 2, 255, 256):
        for width in (1, 7, 2 ** 31 - 1):
            for lo in los:
                check(engine, "neg", prob, sem, bins, lo, width)
    # lo below all scores with width 1 and enough bins: the histogram is the plain count of each score
    _, h = check(engine, "neg", prob, sem, 256, lo_s, 1)
    assert h[0, 0] >= 1 and h[0].sum() == s0[0, 0]
    _, h = check(engine, "neg", prob, sem, 4, hi_s + 1000, 7)  # lo above all scores: everything in bin 0
    assert h[0].tolist() == [s0[0, 0], 0, 0, 0]


# ---- wide arithmetic -----------------------------------------------------------------------------------------
def wide_problem(C, sem):
    """Weights (10^6, 3, 2, 1), one 500-letter record matching Seq1 at each of its C offsets: every score is
    M = 5 * 10^8, the sum of squares C * 2.5e17."""
    L1 = 500 + C - (1 if sem == Semantics.SPEC else 0)
    return problem_of((1_000_000, 3, 2, 1), np.full(L1, 1), [np.full(500, 1)])


@pytest.mark.parametrize("sem", SEMS)
def test_wide_arithmetic_and_refusal(engine, sem):
    M = 500_000_000
    s, _ = check(engine, "wide36", wide_problem(36, sem), sem)
    assert s[0].tolist() == [36, 36 * M, 36 * M * M, M, M, 0, 0] and s[0, 2] > 2 ** 62
    before = engine.stats()
    bad = wide_problem(37, sem)
    engine.set_problem(bad.weights, bad.seq1, sem)
    with pytest.raises(ValueError, match="exactness bound"):
        engine.solve_summary(bad.codes, bad.offsets)
    codes_t = torch.from_numpy(bad.codes).to(DEV)
    offs_t = torch.from_numpy(bad.offsets).to(DEV)
    out_t = torch.full((1, 7), -777, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="exactness bound"):
        engine.solve_summary_device(codes_t, offs_t, bad.offsets, summary_t=out_t)
    torch.cuda.synchronize()
    assert (out_t == -777).all() and engine.stats() == before  # refused before any launch


def test_argument_errors(engine):
    prob = tiny_records(5, seed=3)
    engine.set_problem(prob.weights, prob.seq1)
    before = engine.stats()
    for kw in ({"bins": -1}, {"bins": 257}, {"bins": 4, "width": 0}):
        with pytest.raises(ValueError, match="summary"):
            engine.solve_summary(prob.codes, prob.offsets, **kw)
    assert engine.stats() == before


# ---- chunks --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_chunks(engine, sem):
    rng = np.random.default_rng(7)
    prob = random_problem(300, [1, 299, 300, 301] + rng.integers(100, 300, 36).tolist(), seed=7)
    assert prob.n == 40
    engine.set_profile_scratch(256 << 20)
    whole = check(engine, "chunks", prob, sem, 8, -300, 60)
    assert engine.stats()["chunks"] == 1
    try:
        engine.set_profile_scratch(1024)  # 128 entries: the record of 299 offsets is larger and runs alone
        assert whole[0][:, 0].max() * 8 > 1024
        chunked = check(engine, "chunks", prob, sem, 8, -300, 60)
        assert engine.stats()["chunks"] >= 3, engine.stats()
        assert np.array_equal(chunked[0], whole[0]) and np.array_equal(chunked[1], whole[1])
    finally:
        engine.set_profile_scratch(256 << 20)


# ---- device form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_device_form_feeds_hits_on_a_side_stream(engine, sem):
    prob = make_synthetic("input1", 300, seed=8)
    Z = 1.5
    want_s, want_h = oracle("dev", prob, sem, 12, -200, 50)
    thr = summary_thresholds(want_s, Z)  # CPU side
    want_rows, want_ho = search_hits_cpu(prob, thresholds=thr, semantics=sem)
    assert 0 < want_ho[-1] < want_s[:, 0].sum()
    engine.set_problem(prob.weights, prob.seq1, sem)
    codes_t = torch.from_numpy(prob.codes).to(DEV)
    offs_t = torch.from_numpy(prob.offsets).to(DEV)
    POISON = -777
    s_t = torch.full((prob.n, 7), POISON, dtype=torch.int64, device=DEV)
    h_t = torch.full((prob.n, 12), POISON, dtype=torch.int32, device=DEV)
    s0_t = torch.full((prob.n, 7), POISON, dtype=torch.int64, device=DEV)
    untouched_t = torch.full((prob.n, 12), POISON, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        engine.solve_summary_device(codes_t, offs_t, prob.offsets, 12, -200, 50, s_t, h_t, stream=side)
        assert "summary" in engine.stats()["kernels"] and "profile" in engine.stats()["kernels"]
        # bins = 0 with a histogram tensor alongside: no histogram work, the tensor stays as it is
        engine.solve_summary_device(codes_t, offs_t, prob.offsets, 0, 0, 1, s0_t, untouched_t, stream=side)
        thr_t = summary_thresholds(s_t, Z)
        rows_t, ho_t = engine.solve_hits_device(codes_t, offs_t, prob.offsets, thresholds_t=thr_t,
                                                cap=int(want_ho[-1]), stream=side)
        s2_t, h2_t = align_summary_device(engine, codes_t, offs_t, prob.offsets, stream=side)
    side.synchronize()  # once, at the end
    same(s_t.cpu().numpy(), want_s, "summary")
    same(h_t.cpu().numpy(), want_h, "hist")
    assert torch.equal(s0_t, s_t) and (untouched_t == POISON).all()
    assert thr_t.dtype == torch.int32 and thr_t.device == s_t.device and np.array_equal(thr_t.cpu().numpy(), thr)
    assert np.array_equal(ho_t.cpu().numpy(), want_ho) and np.array_equal(rows_t.cpu().numpy(), want_rows)
    assert h2_t is None and torch.equal(s2_t, s_t)


# ---- wire form -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_wire_form(engine, sem):
    prob = make_synthetic("input6", 700, seed=5)
    by_bytes = check(engine, "wire", prob, sem, 9, -20, 6)
    ws = WireSlice.from_csr(prob.codes, prob.offsets)
    s, h = ws.solve_summary_wire(engine, 9, -20, 6, shift=6)
    st = engine.stats()
    assert {"summary", "profile", "wire"} <= set(st["kernels"]), st
    assert np.array_equal(s, by_bytes[0]) and np.array_equal(h, by_bytes[1])
    s, h = ws.solve_summary_wire(engine)
    assert h is None and np.array_equal(s, by_bytes[0])


# ---- empty batch ---------------------------------------------------------------------------------------------
def test_empty_batch(engine):
    prob = make_synthetic("input1", 4, seed=9)
    check(engine, "four", prob, Semantics.REFERENCE, 3, 0, 100)
    before = engine.stats()
    h_offsets = np.zeros(1, np.int64)
    s, h = engine.solve_summary(prob.codes[:0], h_offsets, 4, 0, 1)
    assert s.shape == (0, 7) and s.dtype == np.int64 and h.shape == (0, 4) and h.dtype == np.int32
    assert engine.solve_summary(prob.codes[:0], h_offsets)[1] is None
    codes_t = torch.zeros(16, dtype=torch.uint8, device=DEV)
    offs_t = torch.zeros(1, dtype=torch.int64, device=DEV)
    s_t, h_t = align_summary_device(engine, codes_t, offs_t, h_offsets, 4, 0, 1)
    torch.cuda.synchronize()
    assert tuple(s_t.shape) == (0, 7) and tuple(h_t.shape) == (0, 4)
    assert engine.stats() == before  # nothing ran: the last call's stats stand


def test_no_record_has_an_offset(engine):
    prob = random_problem(20, [21, 25, 40], seed=10)  # every record longer than Seq1
    s, h = check(engine, "none", prob, Semantics.SPEC, 4, 0, 1)
    assert s.tolist() == [EMPTY_ROW] * 3 and not h.any()


# ---- search invariant ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("i", [3, 6])
def test_search_invariant_on_goldens(engine, i, sem):
    prob = Problem.read(input_path(i))
    s, _ = check(engine, ("golden", i), prob, sem, 32, -2000, 150)
    assert np.array_equal(s[:, 4:7], as_triples(engine.solve(prob.codes, prob.offsets)))
