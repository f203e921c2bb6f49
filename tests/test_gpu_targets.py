"""GPU (MI355X / gfx950) tests of the multi-target search (csrc/src/hip/targets_kernels.hip): the rows exactly equal to
the CPU engine's search_targets_cpu (tests/test_targets_cpu.py anchors that one to search_cpu run on every target
alone) under both semantics, at the smallest shapes that reach each edge of the lane-group kernel — slice and record
lengths around the group size, pair counts that leave the last wave and block partly idle, targets shorter than,
equal to and one letter long next to the records, the straddling record, one record per chunk, the device form on a
side stream feeding the report, the wire form and empty batches. Every test runs once per forced lane-group size
(MOC_TARGETS_GROUP = 4, 16, 64, read when an engine starts) and once with the host's own choice."""
import os

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = pytest.mark.gpu

if not gpu_available():  # pragma: no cover - collected on CPU hosts only with -m gpu
    pytest.skip("no GPU", allow_module_level=True)

import torch  # noqa: E402

from mpi_openmp_cuda_amd import (HipSearchEngine, Problem, Semantics, TargetSet, WireSlice,  # noqa: E402
                                 align_targets_device, make_synthetic, report_scores, search_cpu, search_targets_cpu,
                                 targets_best, targets_catalog_rows)
from mpi_openmp_cuda_amd.ops.align import as_triples, targets_geometry  # noqa: E402

SEMS = [Semantics.REFERENCE, Semantics.SPEC]
GROUPS = [None, 4, 16, 64]  # None: the host chooses per chunk
W = (4, 3, 2, 10)
DEV = torch.device("cuda:0")
I32 = np.iinfo(np.int32)
NONE = [I32.min, 0, 0]

_engines = {}


@pytest.fixture(params=GROUPS, ids=lambda g: f"G{g or 'auto'}")
def engine(request):
    """One engine per forced group size, started with MOC_TARGETS_GROUP set (the variable is read at engine start)."""
    g = request.param
    if g not in _engines:
        old = os.environ.pop("MOC_TARGETS_GROUP", None)
        if g:
            os.environ["MOC_TARGETS_GROUP"] = str(g)
        try:
            _engines[g] = HipSearchEngine(device=0)
        finally:
            os.environ.pop("MOC_TARGETS_GROUP", None)
            if old is not None:
                os.environ["MOC_TARGETS_GROUP"] = old
    eng = _engines[g]
    eng.group = g
    return eng


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


def batch_of(recs):
    lens = np.array([len(r) for r in recs], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return np.concatenate([np.asarray(r, np.uint8) for r in recs]), offsets


def random_case(seed, target_lens, record_lens, alphabet=4):
    rng = np.random.default_rng(seed)
    ts = TargetSet.from_sequences([rng.integers(1, alphabet + 1, int(l)) for l in target_lens])
    codes, offsets = batch_of([rng.integers(1, alphabet + 1, int(l)) for l in record_lens])
    return Problem(list(W), ts.seq1, codes, offsets), ts


_oracle = {}


def oracle(key, prob, ts, sem):
    """The CPU engine's rows of a shared problem: computed once, read-only."""
    k = (key, sem)
    if k not in _oracle:
        rows = search_targets_cpu(prob, ts, sem)
        rows.setflags(write=False)
        _oracle[k] = rows
    return _oracle[k]


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype)
    bad = np.argwhere((got != want).any(axis=-1))
    assert bad.size == 0, (what, bad[:8].tolist(), [got[tuple(b)].tolist() for b in bad[:4]],
                           [want[tuple(b)].tolist() for b in bad[:4]])


def check(eng, key, prob, ts, sem):
    """Host form against the oracle; returns the rows."""
    want = oracle(key, prob, ts, sem)
    eng.set_problem(prob.weights, prob.seq1, sem)
    rows = eng.solve_targets(prob.codes, prob.offsets, ts)
    st = eng.stats()
    assert "targets" in st["kernels"] and "profile" in st["kernels"], st
    same(rows, want, key)
    return rows


# ---- slice and record lengths around the group size --------------------------------------------------------
def edge_lengths(g):
    slices = [0, 1, g - 1, g, g + 1, 2 * g + 1] + ([127, 129] if g == 64 else [])
    records = [1, 2, g - 1, g + 1]
    return slices, records


@pytest.mark.parametrize("sem", SEMS)
def test_slice_and_record_length_edges(engine, sem):
    """Every record length L2 in {1, 2, G - 1, G + 1} meets a target of L2 + s letters for every slice length s in
    {0, 1, G - 1, G, G + 1, 2G + 1} (G = 64: also 127, 129): the slice loop and the boundary diagonal's letter loop
    each run 0, 1, G - 1, G + 1 and more than 2G steps; spec adds the boundary diagonal to every slice, reference has it
    at s = 0 only. The host's own choice gets the lengths of all three sizes."""
    gs = [engine.group] if engine.group else [4, 16, 64]
    target_lens, record_lens = [], []
    for g in gs:
        slices, records = edge_lengths(g)
        record_lens += records
        target_lens += [l2 + s for l2 in records for s in slices]
    prob, ts = random_case(11, target_lens, record_lens)
    rows = check(engine, ("edges", engine.group), prob, ts, sem)
    L2 = np.diff(prob.offsets)
    fits = L2[:, None] <= ts.lengths[None, :]
    assert np.array_equal(rows[:, :, 0] != I32.min, fits) and fits.any() and not fits.all()
    assert (rows[~fits] == NONE).all()
    assert (rows[:, :, 1][fits] <= (ts.lengths[None, :] - L2[:, None])[fits]).all()  # inside the target


# ---- pair counts: the last wave and block partly idle ------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("n,T", [(1, 1), (5, 3), (15, 1), (17, 1), (1, 17), (9, 7), (5, 13), (257, 1), (1, 257)])
def test_pair_counts(engine, sem, n, T):
    assert n * T in (1, 15, 17, 63, 65, 257)
    rng = np.random.default_rng(n * 1000 + T)
    prob, ts = random_case(n * 1000 + T + 1, rng.integers(1, 40, T), rng.integers(1, 13, n))
    rows = check(engine, ("pairs", n, T), prob, ts, sem)
    if T == 1:  # one target: the search itself
        solo = as_triples(engine.solve(prob.codes, prob.offsets))
        same(rows[:, 0], solo, "T = 1 against solve")
        same(rows[:, 0], as_triples(search_cpu(prob, sem)), "T = 1 against search_cpu")


# ---- target edge lengths -----------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_target_edge_lengths(engine, sem):
    """Records of 7 and 9 letters against: a first target of exactly 7, a target shorter than every record, a
    single-letter target, longer ones, and a last target of exactly 9 (its boundary diagonal ends on the catalog's
    last letter)."""
    prob, ts = random_case(21, [7, 3, 1, 30, 8, 10, 200, 9], [7, 9, 7, 9, 9])
    rows = check(engine, "edge targets", prob, ts, sem)
    assert (rows[:, 1] == NONE).all() and (rows[:, 2] == NONE).all()
    assert (rows[[0, 2], 0, 1:] == 0).all() and (rows[[0, 2], 0, 0] != I32.min).all()  # len == L2: (., 0, 0)
    assert (rows[[1, 3, 4], 0] == NONE).all()
    assert (rows[[1, 3, 4], 7, 1:] == 0).all() and (rows[[1, 3, 4], 7, 0] != I32.min).all()


@pytest.mark.parametrize("sem", SEMS)
def test_single_letter_records_and_targets(engine, sem):
    prob, ts = random_case(22, [1, 1, 2, 1, 5], [1, 1, 2], alphabet=2)
    check(engine, "single letters", prob, ts, sem)


@pytest.mark.parametrize("sem", SEMS)
def test_straddling_record(engine, sem):
    rng = np.random.default_rng(2024)
    t1, t2 = (rng.integers(1, 27, size=60).astype(np.uint8) for _ in range(2))
    ts = TargetSet.from_sequences([t1, t2])
    codes, offsets = batch_of([np.concatenate([t1[40:], t2[:20]])])
    prob = Problem(list(W), ts.seq1, codes, offsets)
    rows = check(engine, "straddle", prob, ts, sem)
    trap = as_triples(engine.solve(prob.codes, prob.offsets))[0]
    assert trap.tolist() == [160, 40, 0]  # the catalog searched as one Seq1 finds the placement in neither target
    assert 160 not in rows[0, :, 0].tolist()


@pytest.mark.parametrize("sem", SEMS)
def test_ties(engine, sem):
    ts = TargetSet.from_sequences([np.full(l, 7, np.uint8) for l in (9, 4, 5, 30, 200)])
    codes, offsets = batch_of([np.full(l, 7, np.uint8) for l in (1, 4, 5, 6)])
    prob = Problem(list(W), ts.seq1, codes, offsets)
    rows = check(engine, "ties", prob, ts, sem)
    assert (rows[:, :, 1:] == 0).all()  # every entry ties: the smallest offset, the un-mutated candidate
    best, _ = targets_best(rows)
    assert best.tolist() == [0, 0, 0, 0]


# ---- chunks --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_one_record_per_chunk(engine, sem):
    """Records whose longest slice is below the 4-lane cut-over, between the two, and past the 16-lane one: with one
    record per chunk the host's choice takes each size in one call."""
    _, _, cut4, cut16 = targets_geometry()
    longest = cut16 + 80
    record_lens = [longest - 3, longest - cut4, longest - cut4 - 1, longest - cut16, longest - cut16 - 1, 5, 1, longest,
                   longest + 1]
    prob, ts = random_case(31, [longest, 7, 60, longest - cut4], record_lens)
    engine.set_profile_scratch(256 << 20)
    whole = check(engine, "chunks", prob, ts, sem)
    assert engine.stats()["chunks"] == 1
    try:
        engine.set_profile_scratch(8)  # one entry: every record runs alone
        chunked = check(engine, "chunks", prob, ts, sem)
        assert engine.stats()["chunks"] == prob.n, engine.stats()
        assert np.array_equal(chunked, whole)
    finally:
        engine.set_profile_scratch(256 << 20)


# ---- device form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_device_form_feeds_the_report_on_a_side_stream(engine, sem):
    rng = np.random.default_rng(41)
    prob, ts = random_case(41, rng.integers(1, 60, 12), rng.integers(1, 30, 50))
    want = oracle("device", prob, ts, sem)
    engine.set_problem(prob.weights, prob.seq1, sem)
    codes_t = torch.from_numpy(prob.codes).to(DEV)
    offs_t = torch.from_numpy(prob.offsets).to(DEV)
    starts_t = torch.from_numpy(ts.starts).to(DEV)
    POISON = -777
    rows_t = torch.full((prob.n, ts.T, 3), POISON, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        engine.solve_targets_device(codes_t, offs_t, prob.offsets, ts, rows_t, stream=side)
        st = engine.stats()
        cat_t = targets_catalog_rows(rows_t, ts)
        counts_t = engine.report_device(codes_t, offs_t, prob.offsets, cat_t, stream=side)
        best_t, best_row_t = targets_best(rows_t)
        rows2_t = engine.solve_targets_device(codes_t, offs_t, prob.offsets, ts.starts, starts_t=starts_t, stream=side)
        rows3_t = align_targets_device(engine, codes_t, offs_t, prob.offsets, ts, stream=side)
    side.synchronize()  # once, at the end
    assert "targets" in st["kernels"] and "profile" in st["kernels"], st
    same(rows_t.cpu().numpy(), want, "device rows")
    assert torch.equal(rows2_t, rows_t) and torch.equal(rows3_t, rows_t)
    assert np.array_equal(cat_t.cpu().numpy(), targets_catalog_rows(want, ts))
    scores = report_scores(counts_t.cpu().numpy(), prob.weights)
    real = want[:, :, 0] != I32.min
    assert real.any() and not real.all()
    assert np.array_equal(scores[real], want[:, :, 0][real].astype(np.int64))  # the counts reproduce the scores
    wb, wr = targets_best(want)
    assert np.array_equal(best_t.cpu().numpy(), wb) and np.array_equal(best_row_t.cpu().numpy(), wr)


# ---- wire form -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_wire_form(engine, sem):
    syn = make_synthetic("input6", 700, seed=5)
    rng = np.random.default_rng(51)
    cuts = np.sort(rng.choice(np.arange(1, syn.L1), size=6, replace=False))
    ts = TargetSet(syn.seq1, np.concatenate([[0], cuts, [syn.L1]]))
    by_bytes = check(engine, "wire", syn, ts, sem)
    ws = WireSlice.from_csr(syn.codes, syn.offsets)
    assert ws.letter_format == "p33"
    rows = ws.solve_targets_wire(engine, ts, shift=6)
    st = engine.stats()
    assert {"targets", "profile", "wire"} <= set(st["kernels"]), st
    same(rows, by_bytes, "wire rows")


# ---- empty batch, invalid target sets ------------------------------------------------------------------------
def test_empty_batch_and_invalid_targets(engine):
    prob, ts = random_case(61, [5, 9], [3, 4])
    check(engine, "two", prob, ts, Semantics.REFERENCE)
    before = engine.stats()
    h_offsets = np.zeros(1, np.int64)
    rows = engine.solve_targets(prob.codes[:0], h_offsets, ts)
    assert rows.shape == (0, 2, 3) and rows.dtype == np.int32
    codes_t = torch.zeros(16, dtype=torch.uint8, device=DEV)
    offs_t = torch.zeros(1, dtype=torch.int64, device=DEV)
    rows_t = align_targets_device(engine, codes_t, offs_t, h_offsets, ts)
    torch.cuda.synchronize()
    assert tuple(rows_t.shape) == (0, 2, 3)
    for starts in ([1, 14], [0, 13], [0, 5, 5, 14], [0], list(range(15)) + [13]):
        with pytest.raises(ValueError, match="^targets:"):
            engine.solve_targets(prob.codes, prob.offsets, starts)
    assert engine.stats() == before  # nothing ran: the last call's stats stand
