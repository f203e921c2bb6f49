"""GPU (MI355X / gfx950) tests of the threshold-hit kernels (csrc/src/hip/hits_kernels.hip): hoffsets and rows
exactly equal to the CPU engine's (tests/test_hits_cpu.py anchors that one to a letter-by-letter replay) at the
smallest shapes that reach each edge — one-ballot and multi-pass records, the threshold edges, ties, wide int32
arithmetic, a Seq1 past its LDS staging, chunks under the scratch bound (the prefix sum's carry), the scan's
block and pass boundaries, the capacity contract, the host form's second pass, the device form on a side stream
and empty batches. Every call must report the hits kernels in its stats."""
import numpy as np
import pytest

from conftest import gpu_available, input_path

pytestmark = pytest.mark.gpu

if not gpu_available():  # pragma: no cover - collected on CPU hosts only with -m gpu
    pytest.skip("no GPU", allow_module_level=True)

import torch  # noqa: E402

from mpi_openmp_cuda_amd import (HipSearchEngine, Problem, Semantics, align_hits_device,  # noqa: E402
                                 align_search_device, make_synthetic, search_cpu, search_hits_cpu,
                                 search_profile_cpu)
from mpi_openmp_cuda_amd.ops.align import as_triples, hits_geometry  # noqa: E402

SEMS = [Semantics.REFERENCE, Semantics.SPEC]
W = (10, 2, 3, 4)
DEV = torch.device("cuda:0")
I32 = np.iinfo(np.int32)

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


def median_thresholds(prof, po) -> np.ndarray:
    """Each record's (upper) median profile score, 0 for a record without candidate offsets: the median entry
    itself hits, and unless the record's scores all tie some entries miss."""
    n = len(po) - 1
    c = np.diff(po)
    rec = np.repeat(np.arange(n), c)
    by_score = prof["score"][np.lexsort((prof["score"], rec))]
    thr = np.zeros(n, np.int32)
    has = c > 0
    thr[has] = by_score[(po[:-1] + c // 2)[has]]
    return thr


_oracle = {}


def oracle(key, prob, sem, thr):
    """CPU engine's (profile, poffsets, thresholds, rows, hoffsets) of a shared problem: computed once, read-only.
    ``thr``: "median" (the default), an int (one scalar for the batch), "best" or "best+1" (per record)."""
    k = (key, sem, thr)
    if k not in _oracle:
        pk = (key, sem)
        if pk not in _oracle:
            _oracle[pk] = search_profile_cpu(prob, sem)
        prof, po = _oracle[pk]
        if isinstance(thr, int):
            t = None
            rows, h = search_hits_cpu(prob, min_score=thr, semantics=sem)
        else:
            if thr == "median":
                t = median_thresholds(prof, po)
            else:
                best = np.array([prof["score"][a:b].max() if b > a else 0 for a, b in zip(po[:-1], po[1:])], np.int64)
                t = (best + (1 if thr == "best+1" else 0)).astype(np.int32)
            rows, h = search_hits_cpu(prob, thresholds=t, semantics=sem)
        for a in (prof, po, t, rows, h):
            if a is not None:
                a.setflags(write=False)
        _oracle[k] = (prof, po, t, rows, h)
    return _oracle[k]


def check(eng, key, prob, sem, thr="median", **kw):
    """Host form against the oracle; returns (rows, hoffsets)."""
    prof, po, t, want_rows, want_h = oracle(key, prob, sem, thr)
    eng.set_problem(prob.weights, prob.seq1, sem)
    if t is None:
        rows, h = eng.solve_hits(prob.codes, prob.offsets, min_score=thr, **kw)
    else:
        rows, h = eng.solve_hits(prob.codes, prob.offsets, thresholds=t, **kw)
    st = eng.stats()
    assert "hits" in st["kernels"] and "profile" in st["kernels"], st
    assert h.dtype == np.int64 and rows.dtype == np.int32
    bad = np.flatnonzero(h != want_h)
    assert bad.size == 0, (bad[:8], h[bad[:8]], want_h[bad[:8]])
    bad = np.flatnonzero((rows != want_rows).any(axis=1))
    assert bad.size == 0, (bad[:8], rows[bad[:4]], want_rows[bad[:4]], np.searchsorted(h, bad[:8], "right") - 1)
    if thr == "median":  # some hits and some misses
        assert 0 < h[-1] < po[-1], (h[-1], po[-1])
    return rows, h


# ---- wave and ballot edges -----------------------------------------------------------------------------
TILE_L1 = 140
TILE_LENS = [TILE_L1 - d for d in (1, 2, 62, 63, 64, 125, 126, 127)] + [TILE_L1, TILE_L1 + 1, 1, 2]
# C = 62..65 and 126..129 under either semantics (C = L1 - L2, one more under spec)
BALLOT_L1 = 200
BALLOT_LENS = [BALLOT_L1 - c for c in (62, 63, 64, 65, 126, 127, 128, 129)]


def tile_problem():
    return random_problem(TILE_L1, TILE_LENS, seed=1)


@pytest.mark.parametrize("sem", SEMS)
def test_wave_edges(engine, sem):
    prob = tile_problem()
    _, po, _, _, h = oracle("tile", prob, sem, "median")
    c = np.diff(po).tolist()
    assert c[TILE_LENS.index(TILE_L1 + 1)] == 0 and c[TILE_LENS.index(TILE_L1)] == 1
    check(engine, "tile", prob, sem)


@pytest.mark.parametrize("sem", SEMS)
def test_ballot_edges(engine, sem):
    prob = random_problem(BALLOT_L1, BALLOT_LENS, seed=2)
    _, po, _, _, _ = oracle("ballot", prob, sem, "median")
    assert {63, 64, 65, 127, 128, 129} <= set(np.diff(po).tolist())
    check(engine, "ballot", prob, sem)


# ---- threshold edges -----------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_threshold_edges(engine, sem):
    prob = tile_problem()
    rows, h = check(engine, "tile", prob, sem, int(I32.min))
    prof, po = engine.solve_profile(prob.codes, prob.offsets)
    assert np.array_equal(h, po)
    assert np.array_equal(rows[:, 0], prof["score"]) and np.array_equal(rows[:, 2], prof["k"])
    rows, h = check(engine, "tile", prob, sem, int(I32.max))
    assert len(rows) == 0 and not h.any()
    rows, h = check(engine, "tile", prob, sem, "best")
    ref = as_triples(search_cpu(prob, sem))
    for i in range(prob.n):
        if po[i + 1] > po[i]:
            assert rows[h[i]].tolist() == ref[i].tolist() and (rows[h[i]:h[i + 1], 0] == ref[i, 0]).all()
    rows, h = check(engine, "tile", prob, sem, "best+1")
    assert len(rows) == 0 and not h.any()


# ---- ties ----------------------------------------------------------------------------------------------
def test_all_equal_letters(engine):
    a = np.ones(80, np.uint8)
    prob = problem_of(W, a, [a[:l] for l in (1, 5, 79)])
    engine.set_problem(prob.weights, prob.seq1, Semantics.REFERENCE)
    thr = np.array([10, 50, 790], np.int32)  # 10 * L2: every offset hits
    rows, h = engine.solve_hits(prob.codes, prob.offsets, thresholds=thr)
    assert "hits" in engine.stats()["kernels"]
    want_rows, want_h = search_hits_cpu(prob, thresholds=thr)
    assert np.array_equal(h, want_h) and np.array_equal(rows, want_rows)
    assert h.tolist() == [0, 79, 154, 155]
    assert rows.tolist() == ([[10, n, 0] for n in range(79)] + [[50, n, 0] for n in range(75)] + [[790, 0, 0]])


@pytest.mark.parametrize("sem", SEMS)
def test_zero_weights_every_offset_hits(engine, sem):
    prob = random_problem(200, [1, 3, 60, 137, 199, 200], weights=(0, 0, 0, 0), seed=3)
    rows, h = check(engine, "ties_0", prob, sem, 0)
    _, po, _, _, _ = oracle("ties_0", prob, sem, 0)
    assert np.array_equal(h, po) and not rows[:, 0].any() and not rows[:, 2].any()
    for i in range(prob.n):
        assert rows[h[i]:h[i + 1], 1].tolist() == list(range(po[i + 1] - po[i]))


# ---- arithmetic, long Seq1 -------------------------------------------------------------------------------
def test_wide_arithmetic(engine):
    base = make_synthetic("limits", 6, seed=4)
    prob = Problem([200000, 100, 300, 2], base.seq1, base.codes, base.offsets)
    check(engine, "wide", prob, Semantics.REFERENCE)


def test_long_seq1_past_lds_staging(engine):
    prob = random_problem(60_000, [59_990, 100], seed=5)
    check(engine, "long", prob, Semantics.SPEC)


# ---- chunk carry -----------------------------------------------------------------------------------------
def test_chunk_carry(engine):
    rng = np.random.default_rng(7)
    prob = random_problem(300, [1, 299, 300, 301] + rng.integers(1, 300, 36).tolist(), seed=7)
    engine.set_profile_scratch(256 << 20)
    whole = check(engine, "carry", prob, Semantics.REFERENCE)
    assert engine.stats()["chunks"] == 1
    _, po, _, _, _ = oracle("carry", prob, Semantics.REFERENCE, "median")
    try:
        # 4 KiB = 512 entries: a few records per chunk, every chunk's scan starts from the one before
        # 1 KiB = 128 entries: records with more offsets than that run alone in their chunks
        for bound in (4096, 1024):
            engine.set_profile_scratch(bound)
            chunked = check(engine, "carry", prob, Semantics.REFERENCE)
            assert engine.stats()["chunks"] > 1, engine.stats()
            assert np.array_equal(chunked[0], whole[0]) and np.array_equal(chunked[1], whole[1])
        assert (np.diff(po) * 8 > 1024).any()
    finally:
        engine.set_profile_scratch(256 << 20)


# ---- scan edges ------------------------------------------------------------------------------------------
def tiny_records(n, seed):
    """n records of 1..4 letters against an 8-letter Seq1, built without a Python loop."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 5, n)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return Problem(list(W), rng.integers(1, 27, 8).astype(np.uint8), rng.integers(1, 27, int(offsets[-1])).astype(np.uint8),
                   offsets)


G = hits_geometry()


@pytest.mark.parametrize("n", [G[0] - 1, G[0], G[0] + 1, G[0] * G[1] + 1])
def test_scan_edges(engine, n):
    prob = tiny_records(n, seed=8)
    rows, h = check(engine, ("scan", n), prob, Semantics.REFERENCE)
    prof, po, thr, _, _ = oracle(("scan", n), prob, Semantics.REFERENCE, "median")
    rec = np.repeat(np.arange(n), np.diff(po))
    hit = prof["score"] >= thr[rec]
    counts = np.bincount(rec[hit], minlength=n)
    assert np.array_equal(h[1:], np.cumsum(counts)) and h[0] == 0
    assert np.array_equal(rows[:, 0], prof["score"][hit])


# ---- capacity contract -----------------------------------------------------------------------------------
def test_capacity_contract(engine):
    prob = random_problem(BALLOT_L1, BALLOT_LENS, seed=2)
    sem = Semantics.REFERENCE
    _, _, thr, want_rows, want_h = oracle("ballot", prob, sem, "median")
    total = int(want_h[-1])
    mid = int(want_h[3] + (want_h[4] - want_h[3]) // 2)  # inside record 3's run
    assert want_h[3] < mid < want_h[4] and total > 2
    engine.set_problem(prob.weights, prob.seq1, sem)
    codes_t = torch.from_numpy(prob.codes).to(DEV)
    offs_t = torch.from_numpy(prob.offsets).to(DEV)
    thr_t = torch.from_numpy(np.array(thr)).to(DEV)
    POISON = -777
    for cap in (0, 1, mid, total - 1, total):
        rows_t = torch.full((total + 64, 3), POISON, dtype=torch.int32, device=DEV)
        h_t = torch.full((prob.n + 1,), POISON, dtype=torch.int64, device=DEV)
        engine.solve_hits_device(codes_t, offs_t, prob.offsets, thresholds_t=thr_t, cap=cap, rows_t=rows_t,
                                 hoffsets_t=h_t)
        assert "hits" in engine.stats()["kernels"]
        torch.cuda.synchronize()
        rows = rows_t.cpu().numpy()
        assert np.array_equal(h_t.cpu().numpy(), want_h), cap  # identical in every case
        assert np.array_equal(rows[:cap], want_rows[:cap]), cap
        assert (rows[cap:] == POISON).all(), cap


# ---- the host form's second pass ---------------------------------------------------------------------------
def test_host_form_rerun(engine):
    # at most 6 offsets per record: the hits fit the default capacity of 4 n rows
    prob = random_problem(16, np.random.default_rng(11).integers(10, 17, 40).tolist(), seed=11)
    default = check(engine, "rerun", prob, Semantics.REFERENCE)
    assert engine.hits_passes() == 1
    total = int(default[1][-1])
    assert 1 < total <= 4 * prob.n
    again = check(engine, "rerun", prob, Semantics.REFERENCE, max_rows=1)
    assert engine.hits_passes() == 2
    assert np.array_equal(again[0], default[0]) and np.array_equal(again[1], default[1])
    for hint, passes in ((total, 1), (total - 1, 2)):  # the threshold between one pass and two
        exact = check(engine, "rerun", prob, Semantics.REFERENCE, max_rows=hint)
        assert engine.hits_passes() == passes and np.array_equal(exact[0], default[0])


# ---- device form -----------------------------------------------------------------------------------------
def test_device_form_behind_a_search_on_a_side_stream(engine):
    prob = make_synthetic("input1", 300, seed=8)
    D = 40
    want_rows, want_h = search_hits_cpu(prob, within=D)
    engine.set_problem(prob.weights, prob.seq1, Semantics.REFERENCE)
    codes_t = torch.from_numpy(prob.codes).to(DEV)
    offs_t = torch.from_numpy(prob.offsets).to(DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        best_t = align_search_device(engine, codes_t, offs_t, prob.offsets, stream=side)
        thr_t = (best_t[:, 0].to(torch.int64) - D).clamp(int(I32.min), int(I32.max)).to(torch.int32)  # within, by hand
        rows_t, h_t = align_hits_device(engine, codes_t, offs_t, prob.offsets, thresholds_t=thr_t,
                                        cap=int(want_h[-1]), stream=side)
        assert "hits" in engine.stats()["kernels"]
        rows2_t, h2_t = align_hits_device(engine, codes_t, offs_t, prob.offsets, within=D, cap=int(want_h[-1]),
                                          stream=side)
    side.synchronize()
    assert 0 < want_h[-1] < search_profile_cpu(prob)[1][-1]
    assert np.array_equal(h_t.cpu().numpy(), want_h) and np.array_equal(rows_t.cpu().numpy(), want_rows)
    assert torch.equal(h2_t, h_t) and torch.equal(rows2_t, rows_t)


# ---- empty and degenerate batches ----------------------------------------------------------------------------
def test_empty_batch(engine):
    prob = make_synthetic("input1", 4, seed=9)
    engine.set_problem(prob.weights, prob.seq1)
    h_offsets = np.zeros(1, np.int64)
    rows, h = engine.solve_hits(prob.codes[:0], h_offsets, min_score=0)
    assert rows.shape == (0, 3) and h.tolist() == [0] and engine.hits_passes() == 0
    codes_t = torch.zeros(16, dtype=torch.uint8, device=DEV)
    offs_t = torch.zeros(1, dtype=torch.int64, device=DEV)
    rows_t, h_t = align_hits_device(engine, codes_t, offs_t, h_offsets, min_score=0)
    torch.cuda.synchronize()
    assert rows_t.shape == (1, 3) and h_t.tolist() == [0]


def test_no_record_has_an_offset(engine):
    prob = random_problem(20, [21, 25, 40], seed=10)  # every record longer than Seq1
    rows, h = check(engine, "none", prob, Semantics.SPEC, int(I32.min))
    assert rows.shape == (0, 3) and h.tolist() == [0, 0, 0, 0]


def test_argument_checking(engine):
    prob = tile_problem()
    engine.set_problem(prob.weights, prob.seq1)
    with pytest.raises(ValueError, match="exactly one"):
        engine.solve_hits(prob.codes, prob.offsets)
    with pytest.raises(ValueError, match="exactly one"):
        engine.solve_hits(prob.codes, prob.offsets, min_score=0, within=0)
    with pytest.raises(ValueError, match="thresholds"):
        engine.solve_hits(prob.codes, prob.offsets, thresholds=np.zeros(prob.n + 1, np.int32))


# ---- goldens -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(1, 7))
def test_goldens_within0(engine, i):
    prob = Problem.read(input_path(i))
    engine.set_problem(prob.weights, prob.seq1)
    rows, h = engine.solve_hits(prob.codes, prob.offsets, within=0)
    assert "hits" in engine.stats()["kernels"]
    want_rows, want_h = search_hits_cpu(prob, within=0)
    assert np.array_equal(h, want_h) and np.array_equal(rows, want_rows)
    ref = as_triples(search_cpu(prob))
    first = np.array([rows[h[j]] if h[j + 1] > h[j] else (I32.min, 0, 0) for j in range(prob.n)], np.int32)
    assert np.array_equal(first, ref)
