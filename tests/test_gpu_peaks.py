"""GPU (MI355X / gfx950) tests of distinct placements (csrc/src/hip/peaks_kernels.hip): top-K and hits over the peaks
of a radius, row for row equal to the CPU engine's (tests/test_peaks_cpu.py anchors that one to the definition as a
double loop over a letter-by-letter profile), at the smallest shapes that reach each edge — profile lengths around the
wave kernel's 64 entries and the tile kernel's tile, radii around the wave's log steps and at the largest window, a
placement exactly at and one past the radius, a plateau across a tile boundary, one record per chunk, the capacity
contract and the host form's second pass, the three threshold forms, the device form on a side stream, a wire batch,
radius 0 and a long Seq1."""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = pytest.mark.gpu

if not gpu_available():  # pragma: no cover - collected on CPU hosts only with -m gpu
    pytest.skip("no GPU", allow_module_level=True)

import torch  # noqa: E402

from mpi_openmp_cuda_amd import (HipSearchEngine, Problem, Semantics, align_hits_device,  # noqa: E402
                                 align_search_device, align_topk_device, make_synthetic, search_cpu,
                                 search_hits_cpu, search_topk_cpu)
from mpi_openmp_cuda_amd.ops.align import as_triples, decode_wire_cpu, peaks_geometry  # noqa: E402
from mpi_openmp_cuda_amd.parallel.wire import WireSlice  # noqa: E402

SEMS = [Semantics.REFERENCE, Semantics.SPEC]
W = (4, 3, 2, 10)
DEV = torch.device("cuda:0")
I32 = np.iinfo(np.int32)
MAX_R, WAVE_C, T = peaks_geometry()
DEFAULT_SCRATCH = 256 << 20

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


def same_rows(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got.reshape(-1, 3) != want.reshape(-1, 3)).any(axis=1))
    assert bad.size == 0, (what, bad[:6], got.reshape(-1, 3)[bad[:4]], want.reshape(-1, 3)[bad[:4]])


def check_hits(eng, prob, sem, R, what, **thr):
    want, want_h = search_hits_cpu(prob, semantics=sem, radius=R, **thr)
    rows, h = eng.solve_hits(prob.codes, prob.offsets, radius=R, **thr)
    st = eng.stats()
    assert {"profile", "hits", "peaks"} <= set(st["kernels"]), st
    assert np.array_equal(h, want_h), (what, h[:8], want_h[:8])
    same_rows(rows, want, what)
    return rows, h


def check_topk(eng, prob, sem, R, K, what):
    want = search_topk_cpu(prob, K, sem, radius=R)
    got = eng.solve_topk(prob.codes, prob.offsets, K, radius=R)
    st = eng.stats()
    assert {"profile", "peaks"} <= set(st["kernels"]) and "hits" not in st["kernels"], st
    same_rows(got, want, what)
    return got


# ---- edge sweep ------------------------------------------------------------------------------------------------
EDGE_C = [1, 2, 3, 63, 64, 65, 127, 128, 129, T - 1, T, T + 1, 2 * T + 1]
EDGE_R = [1, 2, 31, 32, 33, 63, 64, 65, MAX_R - 1, MAX_R]


def edge_problem(C):
    """Three records of 8 letters against a Seq1 of C + 8: C profile entries under reference semantics, C + 1 under
    spec. A four-letter alphabet makes runs of equal scores; one record repeats a piece of Seq1."""
    rng = np.random.default_rng(1000 + C)
    seq1 = rng.integers(1, 5, C + 8)
    at = (C // 2) if C > 1 else 0
    return problem_of(W, seq1, [rng.integers(1, 5, 8), seq1[at:at + 8].copy(), np.full(8, 1)])


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("C", EDGE_C)
def test_edge_sweep(engine, C, sem):
    prob = edge_problem(C)
    engine.set_problem(prob.weights, prob.seq1, sem)
    for R in EDGE_R:
        rows, h = check_hits(engine, prob, sem, R, ("hits", C, R), min_score=int(I32.min))
        assert (np.diff(h) >= 1).all()
        if R >= C:  # the window spans the profile (C or C + 1 entries): one peak per record
            assert np.diff(h).tolist() == [1, 1, 1]
        for K in (1, 5, 64):
            check_topk(engine, prob, sem, R, K, ("topk", C, R, K))


# ---- distance edge ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [5, 64, MAX_R])
def test_distance_edge(engine, R):
    """Two copies of a record (40 letters, or R where the copies would overlap) d apart in a random Seq1, the second
    with one letter changed: at d = R the stronger copy suppresses the weaker one, at d = R + 1 it does not."""
    L2 = min(40, R)
    for d, present in ((R, False), (R + 1, True)):
        rng = np.random.default_rng(31)
        n1, n2 = 70, 70 + d
        seq1 = rng.integers(1, 27, n2 + L2 + 70)
        rec = rng.integers(1, 27, L2)
        seq1[n1:n1 + L2] = rec
        seq1[n2:n2 + L2] = rec
        seq1[n2 + L2 // 2] = seq1[n2 + L2 // 2] % 26 + 1
        seq1[n1 - 1] = rec[0] % 26 + 1  # neither shadow's first letter matches: the shadows score below the copies
        if d > L2:
            seq1[n2 - 1] = rec[0] % 26 + 1
        prob = problem_of(W, seq1, [rec])
        want, _ = search_hits_cpu(prob, min_score=int(I32.min), radius=R)
        best = as_triples(search_cpu(prob))[0]
        assert best.tolist() == [4 * L2, n1, 0] and n1 in want[:, 1]
        assert (n2 in want[:, 1]) == present, (R, d)
        engine.set_problem(prob.weights, prob.seq1)
        check_hits(engine, prob, Semantics.REFERENCE, R, ("distance", R, d), min_score=int(I32.min))
        got = check_topk(engine, prob, Semantics.REFERENCE, R, 2, ("distance top-2", R, d))
        assert (got[0, 1, 1] == n2) == present


# ---- plateau across a tile boundary ----------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_plateau_across_a_tile_boundary(engine, sem):
    C = T + 10
    prob = problem_of(W, np.full(C + 8, 1), [np.full(8, 1)])
    engine.set_problem(prob.weights, prob.seq1, sem)
    rows, h = check_hits(engine, prob, sem, 3, "plateau", min_score=int(I32.min))
    assert h.tolist() == [0, 1] and rows[0].tolist() == [32, 0, 0]
    got = check_topk(engine, prob, sem, 3, 4, "plateau top-4")
    assert got[0, 1:, 0].tolist() == [I32.min] * 3


# ---- chunking --------------------------------------------------------------------------------------------------
def test_one_record_per_chunk(engine):
    rng = np.random.default_rng(12)
    L1 = T + 300
    # a record without candidate offsets shares the chunk of a record before it, so the one here comes first
    lens = [L1 + 1, 1, 8, L1 - 1, L1, L1 - 64, L1 - 65, 200, L1 - T, L1 - T - 1, 40, 7]
    prob = problem_of(W, rng.integers(1, 5, L1), [rng.integers(1, 5, l) for l in lens])
    sem = Semantics.SPEC
    engine.set_problem(prob.weights, prob.seq1, sem)
    engine.set_profile_scratch(DEFAULT_SCRATCH)
    whole_rows, whole_h = check_hits(engine, prob, sem, 9, "whole", min_score=int(I32.min))
    assert engine.stats()["chunks"] == 1
    whole_top = check_topk(engine, prob, sem, 9, 6, "whole top-6")
    try:
        engine.set_profile_scratch(8)  # one entry: every record is its own chunk
        rows, h = check_hits(engine, prob, sem, 9, "chunked", min_score=int(I32.min))
        assert engine.stats()["chunks"] == prob.n
        top = check_topk(engine, prob, sem, 9, 6, "chunked top-6")
        assert engine.stats()["chunks"] == prob.n
    finally:
        engine.set_profile_scratch(DEFAULT_SCRATCH)
    assert np.array_equal(h, whole_h) and np.array_equal(rows, whole_rows) and np.array_equal(top, whole_top)


def test_more_tiles_than_blocks(engine):
    """20 000 records of 70 entries: more tile work items than the tile kernel's grid (64 blocks per CU), so blocks
    take several items one after the other and reuse their LDS."""
    rng = np.random.default_rng(13)
    n = 20_000
    prob = Problem(list(W), rng.integers(1, 5, 78).astype(np.uint8), rng.integers(1, 5, 8 * n).astype(np.uint8),
                   np.arange(n + 1, dtype=np.int64) * 8)
    engine.set_problem(prob.weights, prob.seq1)
    check_hits(engine, prob, Semantics.REFERENCE, 5, "many tiles", min_score=int(I32.min))
    check_topk(engine, prob, Semantics.REFERENCE, 5, 2, "many tiles top-2")


# ---- capacity, thresholds, device form -------------------------------------------------------------------------
def test_capacity_contract(engine):
    prob = make_synthetic("input1", 60, seed=4)
    R = 2
    want, want_h = search_hits_cpu(prob, min_score=int(I32.min), radius=R)
    total = int(want_h[-1])
    assert total > prob.n
    engine.set_problem(prob.weights, prob.seq1)
    codes_t = torch.from_numpy(prob.codes).to(DEV)
    offs_t = torch.from_numpy(prob.offsets).to(DEV)
    POISON = -777
    for cap in (0, total - 1):
        rows_t = torch.full((total + 8, 3), POISON, dtype=torch.int32, device=DEV)
        _, h_t = engine.solve_hits_device(codes_t, offs_t, prob.offsets, min_score=int(I32.min), cap=cap,
                                          rows_t=rows_t, radius=R)
        torch.cuda.synchronize()
        assert "peaks" in engine.stats()["kernels"]
        assert np.array_equal(h_t.cpu().numpy(), want_h), cap
        got = rows_t.cpu().numpy()
        assert np.array_equal(got[:cap], want[:cap]) and (got[cap:] == POISON).all(), cap
    # the host form: room for one row, then exactly one more pass with the exact total
    rows, h = engine.solve_hits(prob.codes, prob.offsets, min_score=int(I32.min), max_rows=1, radius=R)
    assert engine.hits_passes() == 2
    assert np.array_equal(h, want_h) and np.array_equal(rows, want)
    rows, h = engine.solve_hits(prob.codes, prob.offsets, min_score=int(I32.min), max_rows=total, radius=R)
    assert engine.hits_passes() == 1 and np.array_equal(rows, want)


def test_threshold_forms(engine):
    prob = make_synthetic("input1", 80, seed=5)
    sem = Semantics.REFERENCE
    engine.set_problem(prob.weights, prob.seq1, sem)
    best = as_triples(search_cpu(prob, sem))[:, 0].astype(np.int64)
    R = 1
    rows_m, _ = check_hits(engine, prob, sem, R, "min_score", min_score=int(np.median(best)) - 40)
    rows_t, _ = check_hits(engine, prob, sem, R, "thresholds", thresholds=(best - 25).astype(np.int32))
    rows_w, _ = check_hits(engine, prob, sem, R, "within", within=25)
    assert np.array_equal(rows_t, rows_w) and len(rows_m) > 0
    plain, _ = search_hits_cpu(prob, within=25)
    assert prob.n <= len(rows_w) < len(plain)  # the shadows are gone, every record keeps its best


def test_device_form_behind_a_search_on_a_side_stream(engine):
    prob = make_synthetic("input1", 300, seed=8)
    D, R, K = 40, 3, 4
    want_rows, want_h = search_hits_cpu(prob, within=D, radius=R)
    want_top = search_topk_cpu(prob, K, radius=R)
    engine.set_problem(prob.weights, prob.seq1, Semantics.REFERENCE)
    codes_t = torch.from_numpy(prob.codes).to(DEV)
    offs_t = torch.from_numpy(prob.offsets).to(DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        best_t = align_search_device(engine, codes_t, offs_t, prob.offsets, stream=side)
        thr_t = (best_t[:, 0].to(torch.int64) - D).clamp(int(I32.min), int(I32.max)).to(torch.int32)
        rows_t, h_t = align_hits_device(engine, codes_t, offs_t, prob.offsets, thresholds_t=thr_t,
                                        cap=int(want_h[-1]), stream=side, radius=R)
        assert {"hits", "peaks"} <= set(engine.stats()["kernels"])
        top_t = align_topk_device(engine, codes_t, offs_t, prob.offsets, K, stream=side, radius=R)
        assert "peaks" in engine.stats()["kernels"]
    side.synchronize()  # the one sync
    assert np.array_equal(h_t.cpu().numpy(), want_h)
    same_rows(rows_t.cpu().numpy(), want_rows, "device hits")
    same_rows(top_t.cpu().numpy(), want_top, "device top-K")
    assert torch.equal(top_t[:, 0], best_t)


# ---- wire form -------------------------------------------------------------------------------------------------
def test_wire_slice(engine):
    rng = np.random.default_rng(42)
    lengths = rng.integers(5, 11, 1000).astype(np.int64)
    seq1 = rng.integers(1, 27, 26).astype(np.uint8)
    ws = WireSlice(lengths, rng.integers(1, 27, int(lengths.sum())).astype(np.uint8), "p33")
    assert ws.letter_format == "p33" and ws.len_bits == 6
    shift = 6
    codes, offsets = decode_wire_cpu(ws, shift)
    prob = Problem(list(W), seq1, codes, offsets)
    sem = Semantics.SPEC
    engine.set_problem(prob.weights, prob.seq1, sem)
    R = 2
    top = ws.solve_topk_wire(engine, 3, shift, radius=R)
    assert {"wire", "profile", "peaks"} <= set(engine.stats()["kernels"])
    same_rows(top, search_topk_cpu(prob, 3, sem, radius=R), "wire top-3")
    rows, h = ws.solve_hits_wire(engine, within=10, shift=shift, radius=R)
    assert {"wire", "hits", "peaks"} <= set(engine.stats()["kernels"])
    want, want_h = search_hits_cpu(prob, within=10, semantics=sem, radius=R)
    assert np.array_equal(h, want_h)
    same_rows(rows, want, "wire hits")
    assert len(want) < len(search_hits_cpu(prob, within=10, semantics=sem)[0])


# ---- radius 0 and a long Seq1 ----------------------------------------------------------------------------------
def test_radius_zero_is_the_plain_call(engine):
    prob = make_synthetic("input1", 100, seed=6)
    engine.set_problem(prob.weights, prob.seq1)
    top = engine.solve_topk(prob.codes, prob.offsets, 5, radius=0)
    assert "peaks" not in engine.stats()["kernels"] and engine.stats()["kernels"] == ["profile"]
    assert np.array_equal(top, engine.solve_topk(prob.codes, prob.offsets, 5))
    assert np.array_equal(top, search_topk_cpu(prob, 5))
    rows, h = engine.solve_hits(prob.codes, prob.offsets, within=10, radius=0)
    assert engine.stats()["kernels"] == ["profile", "hits"]
    rows0, h0 = engine.solve_hits(prob.codes, prob.offsets, within=10)
    assert np.array_equal(rows, rows0) and np.array_equal(h, h0)
    codes_t = torch.from_numpy(prob.codes).to(DEV)
    offs_t = torch.from_numpy(prob.offsets).to(DEV)
    a = align_topk_device(engine, codes_t, offs_t, prob.offsets, 5, radius=0)
    assert "peaks" not in engine.stats()["kernels"]
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy(), top)
    for bad in (-1, MAX_R + 1):
        with pytest.raises(ValueError, match="radius"):
            engine.solve_topk(prob.codes, prob.offsets, 5, radius=bad)
        with pytest.raises(ValueError, match="radius"):
            engine.solve_hits(prob.codes, prob.offsets, min_score=0, radius=bad)


def test_long_seq1(engine):
    prob = make_synthetic("input3", 6, seed=3)
    sem = Semantics.REFERENCE
    engine.set_problem(prob.weights, prob.seq1, sem)
    check_hits(engine, prob, sem, 40, "input3 hits", within=30)
    check_topk(engine, prob, sem, 40, 8, "input3 top-8")
