"""GPU (MI355X / gfx950) tests of the target ranking (csrc/src/hip/targets_rank_kernels.hip behind the targets select
kernel): the rows exactly equal to the CPU engine's search_targets_rank_cpu (tests/test_targets_rank_cpu.py anchors
that to a stable sort of search_targets_cpu's rows and to search_cpu on every target alone) under both semantics, at
the smallest shapes that reach each edge — target counts around the rank kernel's group size with record counts that
leave the last group, wave and block partly idle, M against the records' fitting targets, ties inside one lane and
between neighbouring lanes, the chunk cut of entries plus pair rows at its byte edges into a guarded slice, the largest
T, the scratch shared with the other profile calls, the host form's copy back, the device form on a side stream, the
wire form and the empty batch. Every test runs once per forced rank group (MOC_TARGETS_RANK_GROUP = 4, 16, 64, read
when an engine starts) and once with the host's own choice."""
import os

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = pytest.mark.gpu

if not gpu_available():  # pragma: no cover - collected on CPU hosts only with -m gpu
    pytest.skip("no GPU", allow_module_level=True)

import torch  # noqa: E402

from mpi_openmp_cuda_amd import (HipSearchEngine, Problem, Semantics, TargetSet, WireSlice,  # noqa: E402
                                 align_targets_rank_device, make_synthetic, report_scores, search_targets_rank_cpu,
                                 targets_rank_catalog_rows, targets_rank_chunks)
from mpi_openmp_cuda_amd.ops.align import REPORT_EMPTY, targets_rank_geometry  # noqa: E402

from targets_rank_cases import I32, PAD, SEMS, W, around_m_case, batch_of, entries_of, fitting, random_case  # noqa: E402

GROUPS = [None, 4, 16, 64]  # None: the host chooses from T
DEV = torch.device("cuda:0")
POISON = -777
BIG = 256 << 20

_engines = {}


def engine_with(**env):
    """A new engine started with these variables set (they are read when an engine starts)."""
    old = {k: os.environ.pop(k, None) for k in ("MOC_TARGETS_RANK_GROUP", "MOC_TARGETS_GROUP")}
    os.environ.update({k: str(v) for k, v in env.items() if v})
    try:
        return HipSearchEngine(device=0)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(params=GROUPS, ids=lambda g: f"R{g or 'auto'}")
def engine(request):
    """One engine per forced rank group."""
    g = request.param
    if g not in _engines:
        _engines[g] = engine_with(MOC_TARGETS_RANK_GROUP=g)
    eng = _engines[g]
    eng.group = g
    return eng


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


_oracle = {}


def want_rank(key, prob, ts, M, sem):
    """The CPU engine's ranking of a shared problem: computed once, read-only."""
    k = (key, M, sem)
    if k not in _oracle:
        _oracle[k] = search_targets_rank_cpu(prob, ts, M, sem)
        _oracle[k].setflags(write=False)
    return _oracle[k]


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype)
    bad = np.argwhere((got != want).reshape(got.shape[0], -1).any(axis=1)) if got.size else np.zeros((0, 1), int)
    assert bad.size == 0, (what, bad[:8].ravel().tolist(), [got[b[0]].tolist() for b in bad[:3]],
                           [want[b[0]].tolist() for b in bad[:3]])


def check_rank(eng, key, prob, ts, M, sem):
    want = want_rank(key, prob, ts, M, sem)
    eng.set_problem(prob.weights, prob.seq1, sem)
    rank = eng.solve_targets_rank(prob.codes, prob.offsets, ts, M)
    st = eng.stats()
    assert {"profile", "targets", "targets_rank"} <= set(st["kernels"]), st
    assert st["d2h_bytes"] == prob.n * M * 16, st  # the rows alone come back, never n * T of anything
    same(rank, want, (key, M, sem))
    return rank


def groups_of(eng):
    return [eng.group] if eng.group else [4, 16, 64]


# ---- target counts around the group size, record counts that leave groups idle ---------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_group_edges(engine, sem):
    """T in {1, G - 1, G, G + 1, 2G + 1}: a lane walks 0, 1, 2 or 3 rows per round; n in {1, 5, 17, 65}: the last wave
    (64 / G records) and the last block (256 / G records) are partly idle. The host's own choice gets every G's T."""
    geo = targets_rank_geometry()
    assert geo == (12, 16, 256)
    for g in groups_of(engine):
        for T in sorted({1, g - 1, g, g + 1, 2 * g + 1}):
            for n in (1, 5, 17, 65):
                rng = np.random.default_rng(1000 * T + n)
                prob, ts = random_case(1000 * T + n + 1, rng.integers(1, 12, T), rng.integers(1, 10, n))
                for M in (1, 5) + ((64,) if T == 2 * g + 1 and n == 17 else ()):
                    rank = check_rank(engine, ("edges", T, n), prob, ts, M, sem)
                    assert ((rank[:, :, 0] >= 0).sum(axis=1) == np.minimum(fitting(prob, ts), M)).all()


# ---- M against the records' fitting targets --------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("M", [1, 2, 63, 64])
@pytest.mark.parametrize("T", [63, 64, 65])
def test_targets_around_m(engine, sem, T, M):
    """Records with 0, 1, M - 1, M, M + 1 and T fitting targets: the rounds stop, pad and fill exactly at M."""
    prob, ts, counts = around_m_case(T, M)
    rank = check_rank(engine, ("around", T, M), prob, ts, M, sem)
    assert ((rank[:, :, 0] >= 0).sum(axis=1) == np.minimum(counts, M)).all()
    assert (rank[rank[:, :, 0] < 0] == PAD).all()


# ---- ties ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_identical_targets(engine, sem):
    rng = np.random.default_rng(5)
    one = rng.integers(1, 5, 9)
    ts = TargetSet.from_sequences([one] * 70)
    codes, offsets = batch_of([one[2:6], one, rng.integers(1, 5, 3)])
    prob = Problem(list(W), ts.seq1, codes, offsets)
    for M in (1, 64):
        rank = check_rank(engine, "identical", prob, ts, M, sem)
        assert (rank[:, :, 0] == np.arange(M)[None, :]).all()  # equal scores: targets ascending


@pytest.mark.parametrize("sem", SEMS)
def test_equal_scores_in_one_lane_and_in_neighbouring_lanes(engine, sem):
    """Four copies of one target that holds the record, among targets of another letter: two exactly G apart (rows of
    one lane, found in successive rounds of that lane) and two next to each other (neighbouring lanes)."""
    hit = TargetSet.from_strings(["QABCDQ"]).seq1
    rec = TargetSet.from_strings(["ABCD"]).seq1
    for g in groups_of(engine):
        rng = np.random.default_rng(9 + g)  # the problem depends on g alone: its oracle is shared between engines
        T = 2 * g + 8
        at = [1, 1 + g, g + 3, g + 4]
        seqs = [hit if t in at else rng.integers(17, 20, int(rng.integers(4, 9))) for t in range(T)]
        ts = TargetSet.from_sequences(seqs)
        codes, offsets = batch_of([rec, rec[:3], rng.integers(17, 20, 5)])
        prob = Problem(list(W), ts.seq1, codes, offsets)
        for M in (3, 4, 6):
            rank = check_rank(engine, ("ties", g), prob, ts, M, sem)
            assert rank[0, :min(M, 4), 0].tolist() == at[:M] and len(set(rank[0, :min(M, 4), 1].tolist())) == 1
            if M > 4:
                assert rank[0, 4, 1] < rank[0, 3, 1]


# ---- chunks ------------------------------------------------------------------------------------------------------
def run_into_guarded_slice(eng, prob, ts, M, codes_t, offs_t):
    """The device form into rows [3, 3 + n) of a poisoned tensor: the rows, after checking that the guards stand."""
    big = torch.full((prob.n + 5, M, 4), POISON, dtype=torch.int32, device=DEV)
    out = big[3:3 + prob.n]
    eng.solve_targets_rank_device(codes_t, offs_t, prob.offsets, ts, M, out)
    st = eng.stats()
    torch.cuda.synchronize()
    got = big.cpu().numpy()
    assert (got[:3] == POISON).all() and (got[3 + prob.n:] == POISON).all()
    return got[3:3 + prob.n], st


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("tg", [4, 16, 64])
def test_chunk_cut_at_its_byte_edges(sem, tg):
    """A new engine per forced select-kernel group (MOC_TARGETS_GROUP), so the first call of each batch grows the
    scratch and the second finds it grown. Budgets: every record alone (one entry's 8 bytes, far below 12 T, and one
    byte below two records' cost), two records exactly, and everything in one chunk."""
    T, M = 5, 3
    eng = engine_with(MOC_TARGETS_GROUP=tg)
    try:
        prob, ts = random_case(77, [30, 2, 9, 12, 40], [10] * 7)
        L1 = prob.L1
        one = 8 * entries_of(L1, 10, sem) + 12 * T
        want = want_rank("chunks", prob, ts, M, sem)
        eng.set_problem(prob.weights, prob.seq1, sem)
        codes_t = torch.from_numpy(prob.codes).to(DEV)
        offs_t = torch.from_numpy(prob.offsets).to(DEV)
        for scratch, chunks in ((8, 7), (12 * T - 1, 7), (2 * one - 1, 7), (2 * one, 4), (3 * one + 5, 3), (BIG, 1)):
            cut = targets_rank_chunks(L1, prob.offsets, T, scratch, sem)
            assert len(cut) - 1 == chunks, (scratch, cut)
            eng.set_profile_scratch(scratch)
            for again in (False, True):
                got, st = run_into_guarded_slice(eng, prob, ts, M, codes_t, offs_t)
                assert st["chunks"] == chunks and "targets_rank" in st["kernels"], (scratch, again, st)
                same(got, want, ("chunks", scratch, again))
            host = eng.solve_targets_rank(prob.codes, prob.offsets, ts, M)
            assert eng.stats()["chunks"] == chunks
            same(host, want, ("chunks, host form", scratch))
    finally:
        eng.close()


@pytest.mark.parametrize("sem", SEMS)
def test_records_of_different_lengths_in_uneven_chunks(engine, sem):
    """Chunks of different record counts, one over-budget record alone, records that fit nothing in between."""
    prob, ts = random_case(31, [600, 7, 60, 40], [597, 560, 80, 5, 1, 600, 601, 30, 3, 3, 3, 700, 2])
    want = want_rank("uneven", prob, ts, 4, sem)
    try:
        for scratch in (8, 1500, 6000, BIG):
            engine.set_profile_scratch(scratch)
            rank = check_rank(engine, "uneven", prob, ts, 4, sem)
            assert engine.stats()["chunks"] == len(targets_rank_chunks(prob.L1, prob.offsets, ts.T, scratch, sem)) - 1
            same(rank, want, ("uneven", scratch))
    finally:
        engine.set_profile_scratch(BIG)


# ---- the largest T -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_largest_t(engine, sem):
    rng = np.random.default_rng(4096)
    prob, ts = random_case(4097, rng.integers(1, 4, 4096), rng.integers(1, 4, 70), alphabet=3)
    assert ts.T == 4096
    scratch = 16 * (8 * prob.L1 + 12 * 4096)  # room for about 16 records: several chunks
    chunks = len(targets_rank_chunks(prob.L1, prob.offsets, 4096, scratch, sem)) - 1
    assert 4 <= chunks <= 6
    try:
        engine.set_profile_scratch(scratch)
        for M in (1, 64):
            rank = check_rank(engine, "largest", prob, ts, M, sem)
            assert engine.stats()["chunks"] == chunks
            assert (rank[:, :, 0] >= 0).all()  # a record of at most 3 letters fits over a thousand targets
    finally:
        engine.set_profile_scratch(BIG)


# ---- the scratch is shared with the other profile calls ----------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_shared_scratch(engine, sem):
    rng = np.random.default_rng(61)
    prob, ts = random_case(61, rng.integers(1, 40, 9), rng.integers(1, 20, 40))
    want = want_rank("shared", prob, ts, 3, sem)
    engine.set_problem(prob.weights, prob.seq1, sem)
    topk = engine.solve_targets_topk(prob.codes, prob.offsets, ts, 2)
    first = engine.solve_targets_rank(prob.codes, prob.offsets, ts, 3)
    hits, hoffsets = engine.solve_hits(prob.codes, prob.offsets, min_score=0)
    second = engine.solve_targets_rank(prob.codes, prob.offsets, ts, 3)
    same(first, want, "after top-K")
    same(second, want, "after hits")
    assert np.array_equal(first, second) and topk.shape == (prob.n, ts.T, 2, 3) and hoffsets[-1] == hits.shape[0]
    fit = first[:, 0, 0] >= 0
    assert np.array_equal(first[fit, 0, 1:], topk[np.flatnonzero(fit), first[fit, 0, 0], 0])  # row 0 is a top-K row


# ---- device form on a side stream --------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_device_form_on_a_side_stream(engine, sem):
    """solve_targets_rank_device -> targets_rank_catalog_rows -> report_device queued on one side stream, one sync."""
    rng = np.random.default_rng(41)
    prob, ts = random_case(41, rng.integers(1, 60, 12), rng.integers(1, 80, 50))  # some records fit few targets or none
    M = 4
    want = want_rank("device", prob, ts, M, sem)
    engine.set_problem(prob.weights, prob.seq1, sem)
    codes_t = torch.from_numpy(prob.codes).to(DEV)
    offs_t = torch.from_numpy(prob.offsets).to(DEV)
    starts_t = torch.from_numpy(ts.starts).to(DEV)
    rank_t = torch.full((prob.n, M, 4), POISON, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        engine.solve_targets_rank_device(codes_t, offs_t, prob.offsets, ts, M, rank_t, stream=side)
        st = engine.stats()
        cat_t = targets_rank_catalog_rows(rank_t, ts)
        counts_t = engine.report_device(codes_t, offs_t, prob.offsets, cat_t, stream=side)
        rank2_t = engine.solve_targets_rank_device(codes_t, offs_t, prob.offsets, ts.starts, M, starts_t=starts_t, stream=side)
        rank3_t = align_targets_rank_device(engine, codes_t, offs_t, prob.offsets, ts, M, stream=side)
    side.synchronize()  # once, at the end
    assert {"profile", "targets", "targets_rank"} <= set(st["kernels"]), st
    same(rank_t.cpu().numpy(), want, "device rows")
    assert torch.equal(rank2_t, rank_t) and torch.equal(rank3_t, rank_t)
    assert np.array_equal(cat_t.cpu().numpy(), targets_rank_catalog_rows(want, ts))
    scores = report_scores(counts_t.cpu().numpy(), prob.weights)
    real = want[:, :, 0] >= 0
    assert real.any() and not real.all()
    assert np.array_equal(scores[real], want[:, :, 1][real].astype(np.int64))  # the counts reproduce the scores
    assert (scores[~real] == REPORT_EMPTY).all()


# ---- wire form, empty batch, refused calls -------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_wire_form(engine, sem):
    syn = make_synthetic("input6", 300, seed=5)
    rng = np.random.default_rng(51)
    cuts = np.sort(rng.choice(np.arange(1, syn.L1), size=6, replace=False))
    ts = TargetSet(syn.seq1, np.concatenate([[0], cuts, [syn.L1]]))
    by_bytes = check_rank(engine, "wire", syn, ts, 3, sem)
    ws = WireSlice.from_csr(syn.codes, syn.offsets)
    assert ws.letter_format == "p33"
    for shift in (0, 6):  # dense and sparse offsets
        rows = ws.solve_targets_rank_wire(engine, ts, 3, shift=shift)
        assert {"targets_rank", "targets", "profile", "wire"} <= set(engine.stats()["kernels"]), engine.stats()
        assert np.array_equal(rows, by_bytes), shift


def test_empty_batch_and_refused_calls(engine):
    prob, ts = random_case(61, [5, 9], [3, 4])
    check_rank(engine, "two", prob, ts, 2, Semantics.REFERENCE)
    before = engine.stats()
    h_offsets = np.zeros(1, np.int64)
    rows = engine.solve_targets_rank(prob.codes[:0], h_offsets, ts, 2)
    assert rows.shape == (0, 2, 4) and rows.dtype == np.int32
    codes_t = torch.zeros(16, dtype=torch.uint8, device=DEV)
    offs_t = torch.zeros(1, dtype=torch.int64, device=DEV)
    rows_t = align_targets_rank_device(engine, codes_t, offs_t, h_offsets, ts, 2)
    torch.cuda.synchronize()
    assert tuple(rows_t.shape) == (0, 2, 4)
    for starts in ([1, 14], [0, 13], [0, 5, 5, 14], [0]):
        for M in (0, 2):
            with pytest.raises(ValueError, match="^targets:"):
                engine.solve_targets_rank(prob.codes, prob.offsets, starts, M)  # the target set's error comes first
    for M in (0, 65, -1):
        with pytest.raises(ValueError, match=r"^rank: M must be in 1\.\.64"):
            engine.solve_targets_rank(prob.codes, prob.offsets, ts, M)
    # the C ABI states the same order, before anything is launched
    from mpi_openmp_cuda_amd import _lib
    out = np.zeros((prob.n, 64, 4), np.int32)
    for starts, M, prefix in ((np.array([1, 14], np.int64), 0, "targets:"), (ts.starts, 0, "rank:"), (ts.starts, 65, "rank:")):
        rc = _lib.lib().moc_engine_solve_targets_rank(engine._h, _lib.ptr(prob.codes), _lib.ptr(prob.offsets), prob.n,
                                                      _lib.ptr(starts), starts.shape[0] - 1, M, _lib.ptr(out))
        assert rc != 0 and _lib.lib().moc_last_error().decode().startswith(prefix)
    assert not out.any() and before["kernels"] == engine.stats()["kernels"]
