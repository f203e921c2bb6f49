"""GPU (MI355X / gfx950) tests of the per-offset profile and top-K kernels (csrc/src/hip/profile_kernels.hip):
entry-for-entry equal to the CPU engine (tests/test_topk_cpu.py anchors that one to a letter-by-letter replay)
at the smallest shapes that reach each edge — wave-tile and letter-chunk boundaries for every sub-tile count,
ties, wide int32 arithmetic, a Seq1 past its LDS staging, bulk short records, the bounded top-K scratch, the
device-resident forms and the K limits. Every call must report the profile kernel in its stats."""
import numpy as np
import pytest

from conftest import expected, gpu_available, input_path

pytestmark = pytest.mark.gpu

if not gpu_available():  # pragma: no cover - collected on CPU hosts only with -m gpu
    pytest.skip("no GPU", allow_module_level=True)

import torch  # noqa: E402

from mpi_openmp_cuda_amd import (HipSearchEngine, Problem, Semantics, align_profile_device,  # noqa: E402
                                 align_search_device, align_topk_device, format_topk, make_synthetic, search_cpu,
                                 search_profile_cpu, search_topk_cpu)
from mpi_openmp_cuda_amd.ops.align import as_triples  # noqa: E402

SEMS = [Semantics.REFERENCE, Semantics.SPEC]
W = (10, 2, 3, 4)
DEV = torch.device("cuda:0")
NONE = [np.iinfo(np.int32).min, 0, 0]

_engines = {}


def engine_for(tile_u, monkeypatch):
    """One engine per sub-tile count (MOC_TILE_U is read when an engine starts; None = the engine's own choice)."""
    if tile_u not in _engines:
        if tile_u is None:
            monkeypatch.delenv("MOC_TILE_U", raising=False)
        else:
            monkeypatch.setenv("MOC_TILE_U", str(tile_u))
        _engines[tile_u] = HipSearchEngine(device=0)
    return _engines[tile_u]


@pytest.fixture
def engine(monkeypatch):
    return engine_for(None, monkeypatch)


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


def problem_of(weights, seq1, recs) -> Problem:
    lens = np.array([len(r) for r in recs], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return Problem(list(weights), np.asarray(seq1, np.uint8), np.concatenate([np.asarray(r, np.uint8) for r in recs]),
                   offsets)


def random_problem(L1, lens, weights=W, seed=0) -> Problem:
    rng = np.random.default_rng(seed)
    return problem_of(weights, rng.integers(1, 27, L1), [rng.integers(1, 27, l) for l in lens])


_oracle = {}


def oracle(key, prob, sem, K):
    """CPU engine's (profile, poffsets, top-K) of a shared problem: computed once, read-only."""
    k = (key, sem, K)
    if k not in _oracle:
        prof, po = search_profile_cpu(prob, sem)
        top = search_topk_cpu(prob, K, sem)
        for a in (prof, po, top):
            a.setflags(write=False)
        _oracle[k] = (prof, po, top)
    return _oracle[k]


def check(eng, key, prob, sem, K, profile=True):
    want_prof, want_po, want_top = oracle(key, prob, sem, K)
    eng.set_problem(prob.weights, prob.seq1, sem)
    if profile:
        prof, po = eng.solve_profile(prob.codes, prob.offsets)
        assert "profile" in eng.stats()["kernels"], eng.stats()
        assert np.array_equal(po, want_po)
        bad = np.flatnonzero(prof != want_prof)
        assert bad.size == 0, (bad[:8], prof[bad[:8]], want_prof[bad[:8]], np.searchsorted(po, bad[:8], "right") - 1)
    top = eng.solve_topk(prob.codes, prob.offsets, K)
    assert "profile" in eng.stats()["kernels"], eng.stats()
    bad = np.flatnonzero((top != want_top).any(axis=(1, 2)))
    assert bad.size == 0, (bad[:8], top[bad[:4]], want_top[bad[:4]])
    return top


# ---- wave-tile and letter-chunk edges ------------------------------------------------------------------
TILE_L1 = 140
TILE_LENS = [TILE_L1 - d for d in (1, 2, 62, 63, 64, 125, 126, 127)] + [TILE_L1, TILE_L1 + 1, 1, 2]


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("tile_u", [1, 2, 4])
def test_tile_edges(tile_u, sem, monkeypatch):
    prob = random_problem(TILE_L1, TILE_LENS, seed=1)
    check(engine_for(tile_u, monkeypatch), "tile", prob, sem, 8)


@pytest.mark.parametrize("sem", SEMS)
def test_letter_chunk_edges(engine, sem):
    check(engine, "chunk", random_problem(300, [63, 64, 65, 128, 129], seed=2), sem, 8)


# ---- ties ---------------------------------------------------------------------------------------------
def test_all_equal_letters(engine):
    a = np.ones(80, np.uint8)
    prob = problem_of(W, a, [a[:l] for l in (1, 5, 79)])
    top = check(engine, "ties_a", prob, Semantics.REFERENCE, 8)
    for i, L2 in enumerate((1, 5)):
        assert top[i].tolist() == [[10 * L2, n, 0] for n in range(8)]
    assert top[2].tolist() == [[790, 0, 0]] + [NONE] * 7


@pytest.mark.parametrize("sem", SEMS)
def test_zero_weights_order_is_n_ascending(engine, sem):
    prob = random_problem(200, [1, 3, 60, 137, 199, 200], weights=(0, 0, 0, 0), seed=3)
    top = check(engine, "ties_0", prob, sem, 8)
    for i in range(prob.n):
        real = top[i][top[i][:, 0] != NONE[0]]
        assert real[:, 1].tolist() == list(range(len(real))) and not real[:, 0].any() and not real[:, 2].any()


# ---- arithmetic, long Seq1, bulk short records ------------------------------------------------------------
def test_wide_arithmetic(engine):
    base = make_synthetic("limits", 6, seed=4)
    prob = Problem([200000, 100, 300, 2], base.seq1, base.codes, base.offsets)
    check(engine, "wide", prob, Semantics.REFERENCE, 8)


def test_long_seq1_past_lds_staging(engine):
    prob = random_problem(60_000, [59_990, 100], seed=5)
    check(engine, "long", prob, Semantics.SPEC, 8)


@pytest.mark.parametrize("shape,n", [("input6", 20000), ("input1", 2000)])
def test_short_records_in_bulk(engine, shape, n):
    check(engine, shape, make_synthetic(shape, n, seed=6), Semantics.REFERENCE, 4)


# ---- bounded top-K scratch -----------------------------------------------------------------------------
def test_scratch_bound(engine):
    prob = make_synthetic("input4", 300, seed=7)
    engine.set_profile_scratch(256 << 20)
    unbounded = check(engine, "scratch", prob, Semantics.REFERENCE, 8, profile=False)
    assert engine.stats()["chunks"] == 1
    try:
        # 64 KiB: a couple of input4's ~23 KiB profiles per chunk, many chunks
        engine.set_profile_scratch(1 << 16)
        bounded = check(engine, "scratch", prob, Semantics.REFERENCE, 8, profile=False)
        assert 100 <= engine.stats()["chunks"] <= prob.n, engine.stats()
        assert np.array_equal(bounded, unbounded)
        # 4 KiB: every record's profile exceeds the bound and runs alone in its chunk
        engine.set_profile_scratch(1 << 12)
        alone = check(engine, "scratch", prob, Semantics.REFERENCE, 8, profile=False)
        assert engine.stats()["chunks"] == prob.n, engine.stats()
        assert np.array_equal(alone, unbounded)
    finally:
        engine.set_profile_scratch(256 << 20)


# ---- device-resident forms -----------------------------------------------------------------------------
def test_device_forms_on_a_side_stream(engine):
    prob = make_synthetic("input1", 300, seed=8)
    want_prof, want_po, want_top = oracle("dev", prob, Semantics.REFERENCE, 5)
    engine.set_problem(prob.weights, prob.seq1, Semantics.REFERENCE)
    codes_t = torch.from_numpy(prob.codes).to(DEV)
    offs_t = torch.from_numpy(prob.offsets).to(DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        prof_t, po = align_profile_device(engine, codes_t, offs_t, prob.offsets, stream=side)
        assert "profile" in engine.stats()["kernels"]
        top_t = align_topk_device(engine, codes_t, offs_t, prob.offsets, 5, stream=side)
        assert "profile" in engine.stats()["kernels"]
        best_t = align_search_device(engine, codes_t, offs_t, prob.offsets, stream=side)
    side.synchronize()
    assert np.array_equal(po, want_po)
    assert np.array_equal(prof_t.cpu().numpy(), np.stack([want_prof["score"], want_prof["k"]], axis=1))
    assert np.array_equal(top_t.cpu().numpy(), want_top)
    assert torch.equal(top_t[:, 0], best_t)


def test_device_forms_empty_batch(engine):
    prob = make_synthetic("input1", 4, seed=9)
    engine.set_problem(prob.weights, prob.seq1)
    codes_t = torch.zeros(16, dtype=torch.uint8, device=DEV)
    offs_t = torch.zeros(1, dtype=torch.int64, device=DEV)
    h_offsets = np.zeros(1, np.int64)
    prof_t, po = align_profile_device(engine, codes_t, offs_t, h_offsets)
    top_t = align_topk_device(engine, codes_t, offs_t, h_offsets, 3)
    torch.cuda.synchronize()
    assert prof_t.shape == (0, 2) and po.tolist() == [0] and top_t.shape == (0, 3, 3)
    assert engine.solve_topk(prob.codes[:0], h_offsets, 3).shape == (0, 3, 3)


# ---- K edges and the goldens -----------------------------------------------------------------------------
def test_k_edges(engine):
    prob = random_problem(50, [47, 20, 50, 51], seed=10)  # C = 3, 30, 1, 0 under the reference semantics
    engine.set_problem(prob.weights, prob.seq1)
    one = engine.solve_topk(prob.codes, prob.offsets, 1)
    assert np.array_equal(one[:, 0], as_triples(engine.solve(prob.codes, prob.offsets)))
    assert np.array_equal(one[:, 0], as_triples(search_cpu(prob)))
    top = check(engine, "kedge", prob, Semantics.REFERENCE, 64)
    assert (top[0][:3, 0] != NONE[0]).all() and top[0][3:].tolist() == [NONE] * 61
    assert top[3].tolist() == [NONE] * 64
    for K in (0, 65):
        with pytest.raises(ValueError):
            engine.solve_topk(prob.codes, prob.offsets, K)


@pytest.mark.parametrize("i", range(1, 7))
def test_goldens(engine, i):
    prob = Problem.read(input_path(i))
    engine.set_problem(prob.weights, prob.seq1)
    top = engine.solve_topk(prob.codes, prob.offsets, 2)
    assert "profile" in engine.stats()["kernels"]
    assert format_topk(top[:, :1]) == expected(i)
    assert np.array_equal(top, search_topk_cpu(prob, 2))
