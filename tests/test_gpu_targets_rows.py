"""GPU (MI355X / gfx950) tests of per-target top-K and threshold hits (csrc/src/hip/targets_rows_kernels.hip): the
rows exactly equal to the CPU engine's search_targets_topk_cpu / search_targets_hits_cpu (tests/test_targets_rows_cpu.py
anchors those to search_topk_cpu / search_hits_cpu run on every target alone) under both semantics, at the smallest
shapes that reach each edge of the three lane-group kernels — slice and record lengths around the group size and the
held-keys count, K against the pairs' entry counts, pair counts that leave the last group, wave and block idle, one
wave whose groups have slices of different lengths (the compaction's divergence case), the threshold and capacity
edges, the prefix sum over pairs at its block and pass edges, one record per chunk, the device forms on a side stream,
the wire forms, empty batches and refused calls. Every test runs once per forced lane-group size (MOC_TARGETS_GROUP =
4, 16, 64, read when an engine starts) and once with the host's own choice."""
import os

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = pytest.mark.gpu

if not gpu_available():  # pragma: no cover - collected on CPU hosts only with -m gpu
    pytest.skip("no GPU", allow_module_level=True)

import torch  # noqa: E402

from mpi_openmp_cuda_amd import (HipSearchEngine, Problem, Semantics, TargetSet, WireSlice,  # noqa: E402
                                 align_targets_hits_device, align_targets_topk_device, make_synthetic,
                                 search_profile_cpu, search_targets_cpu, search_targets_hits_cpu,
                                 search_targets_topk_cpu)
from mpi_openmp_cuda_amd.ops.align import hits_geometry  # noqa: E402

SEMS = [Semantics.REFERENCE, Semantics.SPEC]
GROUPS = [None, 4, 16, 64]  # None: the host chooses per chunk
W = (4, 3, 2, 10)
DEV = torch.device("cuda:0")
I32 = np.iinfo(np.int32)
NONE = [I32.min, 0, 0]
HELD = 4  # slice keys a lane of the top-K kernel keeps in registers (targets_rows_kernels.hip kHeld)

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


def cached(key, make):
    """A CPU-engine result of a shared problem: computed once, read-only."""
    if key not in _oracle:
        got = make()
        for a in got if isinstance(got, tuple) else (got,):
            a.setflags(write=False)
        _oracle[key] = got
    return _oracle[key]


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype)
    bad = np.argwhere((got != want).reshape(got.shape[0], -1).any(axis=1)) if got.size else np.zeros((0, 1), int)
    assert bad.size == 0, (what, bad[:8].ravel().tolist(), [got[b[0]].tolist() for b in bad[:3]],
                           [want[b[0]].tolist() for b in bad[:3]])


def check_topk(eng, key, prob, ts, sem, K):
    want = cached((key, sem, "topk", K), lambda: search_targets_topk_cpu(prob, ts, K, sem))
    eng.set_problem(prob.weights, prob.seq1, sem)
    rows = eng.solve_targets_topk(prob.codes, prob.offsets, ts, K)
    st = eng.stats()
    assert "targets_topk" in st["kernels"] and "profile" in st["kernels"] and "targets" not in st["kernels"], st
    same(rows.reshape(-1, K * 3), want.reshape(-1, K * 3), (key, "top-K", K))
    return rows


def check_hits(eng, key, prob, ts, sem, **thr):
    tag = tuple((k, v if np.isscalar(v) else "array") for k, v in thr.items())
    want_rows, want_off = cached((key, sem, "hits", tag), lambda: search_targets_hits_cpu(prob, ts, semantics=sem, **thr))
    eng.set_problem(prob.weights, prob.seq1, sem)
    rows, toffsets = eng.solve_targets_hits(prob.codes, prob.offsets, ts, **thr)
    st = eng.stats()
    assert "targets_hits" in st["kernels"] and "profile" in st["kernels"] and "hits" not in st["kernels"], st
    assert toffsets.dtype == np.int64 and np.array_equal(toffsets, want_off), (key, "index")
    same(rows, want_rows, (key, "hits"))
    return rows, toffsets


def mid_threshold(key, prob, ts, sem):
    """A threshold that some entries of most pairs reach: the median best score of the pairs that fit."""
    best = cached((key, sem, "best"), lambda: search_targets_cpu(prob, ts, sem))[:, :, 0]
    return int(np.median(best[best != I32.min])) - 3


# ---- slice and record lengths around the group size and the held keys ---------------------------------------
def edge_lengths(g):
    slices = [0, 1, g - 1, g, g + 1, 2 * g + 1, HELD * g - 1, HELD * g, HELD * g + 1]
    records = [1, 2, g - 1, g + 1]
    return slices, records


@pytest.mark.parametrize("sem", SEMS)
def test_slice_and_record_length_edges(engine, sem):
    """Every record length L2 in {1, 2, G - 1, G + 1} meets a target of L2 + s letters for every slice length s in
    {0, 1, G - 1, G, G + 1, 2G + 1, 4G - 1, 4G, 4G + 1}: the held keys fill exactly, fall one short and spill one entry
    into the re-read loop; the boundary entry's letter loop runs 1, 2, G - 1 and G + 1 steps. The host's own choice gets
    the lengths of all three sizes."""
    gs = [engine.group] if engine.group else [4, 16, 64]
    target_lens, record_lens = [], []
    for g in gs:
        slices, records = edge_lengths(g)
        record_lens += records
        target_lens += [l2 + s for l2 in records for s in slices]
    key = ("edges", engine.group)
    prob, ts = random_case(11, target_lens, record_lens)
    rows = check_topk(engine, key, prob, ts, sem, 5)
    L2 = np.diff(prob.offsets)
    room = (ts.lengths[None, :] - L2[:, None])[:, :, None]
    real = rows[:, :, :, 0] != I32.min
    assert (rows[:, :, :, 1][real] <= np.broadcast_to(room, real.shape)[real]).all()  # inside the target
    assert (rows[~real] == NONE).all() and real.any() and not real.all()
    check_hits(engine, key, prob, ts, sem, min_score=mid_threshold(key, prob, ts, sem))


# ---- K against the pairs' entry counts -----------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("K", [1, 2, 63, 64])
def test_k_against_entry_counts(engine, sem, K):
    """Pairs with C in {0, 1, K - 1, K, K + 1} entries: the rounds stop, pad and fill exactly at K."""
    L2 = 3
    extra = 0 if sem == Semantics.SPEC else 1  # the boundary entry is spec's (or len == L2's)
    counts = sorted({1, max(K - 1, 1), K, K + 1})
    lens = [2] + [L2 if c == 1 else L2 + c - 1 + extra for c in counts]
    prob, ts = random_case(70 + K, lens, [L2, L2, 1])
    rows = check_topk(engine, ("K", K), prob, ts, sem, K)
    got = (rows[0, :, :, 0] != I32.min).sum(axis=1).tolist()
    assert got == [0] + [min(c, K) for c in counts], (got, counts)
    if K == 1:
        engine.set_problem(prob.weights, prob.seq1, sem)
        same(rows[:, :, 0], engine.solve_targets(prob.codes, prob.offsets, ts), "K = 1 against solve_targets")


# ---- pair counts: the last group, wave and block idle --------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("n,T", [(1, 1), (5, 3), (1, 17), (9, 7), (257, 1), (1, 257)])
def test_pair_counts(engine, sem, n, T):
    rng = np.random.default_rng(n * 1000 + T)
    prob, ts = random_case(n * 1000 + T + 1, rng.integers(1, 40, T), rng.integers(1, 13, n))
    key = ("pairs", n, T)
    topk = check_topk(engine, key, prob, ts, sem, 3)
    thr = mid_threshold(key, prob, ts, sem)
    rows, toffsets = check_hits(engine, key, prob, ts, sem, min_score=thr)
    if T == 1:  # one target: top-K and hits themselves
        same(topk[:, 0].reshape(n, -1), engine.solve_topk(prob.codes, prob.offsets, 3).reshape(n, -1), "T = 1 top-K")
        r1, h1 = engine.solve_hits(prob.codes, prob.offsets, min_score=thr)
        assert np.array_equal(h1, toffsets)
        same(rows, r1, "T = 1 hits")


# ---- one wave whose groups have slices of different lengths --------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_groups_of_one_wave_diverge(engine, sem):
    """One record against targets whose slices are 0, 1, G and 2G + 3 entries long next to a target it does not fit,
    twice over so that consecutive groups of a wave differ: the compaction's trip count is the wave's longest slice,
    and a group past its own slice must neither contribute bits nor store."""
    g = engine.group or 4
    L2 = 5
    lens = [L2, L2 + 1, L2 + g, L2 + 2 * g + 3, L2 - 1, L2 + 2 * g + 3, L2 - 1, L2 + 1, L2, L2 + g]
    key = ("diverge", g)
    prob, ts = random_case(81, lens, [L2, L2 + 1])
    check_topk(engine, key, prob, ts, sem, 4)
    rows, toffsets = check_hits(engine, key, prob, ts, sem, min_score=int(I32.min))
    counts = np.diff(toffsets).reshape(2, -1)
    spec = 1 if sem == Semantics.SPEC else 0
    assert counts[0].tolist() == [1, 1 + spec, g + spec, 2 * g + 3 + spec, 0, 2 * g + 3 + spec, 0, 1 + spec, 1, g + spec]
    check_hits(engine, key, prob, ts, sem, min_score=mid_threshold(key, prob, ts, sem))


# ---- thresholds ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_threshold_edges(engine, sem):
    """Nothing reaches INT32_MAX; everything reaches INT32_MIN — a pair's hits are then the per-target profile —; and a
    full-match threshold that only a boundary entry reaches: the record is the last letters of target 0 (spec's final
    offset) and the whole of target 1 (len == L2 under both semantics)."""
    rng = np.random.default_rng(91)
    rec = rng.integers(1, 27, 9).astype(np.uint8)
    t0 = np.concatenate([rng.integers(1, 27, 23).astype(np.uint8), rec])
    t0[22] = rec[0] % 26 + 1  # the letter before the copy differs from the record's first
    ts = TargetSet.from_sequences([t0, rec, rng.integers(1, 27, 40).astype(np.uint8)])
    codes, offsets = batch_of([rec, rng.integers(1, 27, 4).astype(np.uint8)])
    prob = Problem(list(W), ts.seq1, codes, offsets)
    rows, toffsets = check_hits(engine, "thr", prob, ts, sem, min_score=int(I32.max))
    assert rows.shape == (0, 3) and not toffsets.any()
    rows, toffsets = check_hits(engine, "thr", prob, ts, sem, min_score=int(I32.min))
    for t in range(ts.T):
        prof, poff = search_profile_cpu(Problem(list(W), ts.target(t), codes, offsets), sem)
        for i in range(2):
            mine = rows[toffsets[i * ts.T + t]:toffsets[i * ts.T + t + 1]]
            p = prof[poff[i]:poff[i + 1]]
            assert np.array_equal(mine[:, 0], p["score"]) and np.array_equal(mine[:, 2], p["k"])
            assert np.array_equal(mine[:, 1], np.arange(len(p)))
    full = 4 * len(rec)
    rows, toffsets = check_hits(engine, "thr", prob, ts, sem, min_score=full)
    want = ([[full, 23, 0]] if sem == Semantics.SPEC else []) + [[full, 0, 0]]
    assert rows.tolist() == want and toffsets.tolist() == [0, len(want) - 1, len(want)] + [len(want)] * 4
    per_pair = np.full((2, ts.T), I32.max, np.int32)
    per_pair[0, 1] = full
    per_pair[1, 2] = I32.min
    check_hits(engine, "thr", prob, ts, sem, thresholds=per_pair)


# ---- capacity ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_capacity_edges_with_guard_rows(engine, sem):
    prob, ts = random_case(101, [9, 3, 30, 14], [4, 9, 2, 6])
    key = "cap"
    thr = mid_threshold(key, prob, ts, sem) - 5  # pairs with 0, 1, 2, 4, 7 and 19 hits
    want, woff = cached((key, sem, "hits"), lambda: search_targets_hits_cpu(prob, ts, min_score=thr, semantics=sem))
    total = int(woff[-1])
    inside = next(int(woff[p]) + 1 for p in range(len(woff) - 1) if woff[p + 1] - woff[p] >= 3)
    edge = next(int(woff[p + 1]) for p in range(len(woff) - 1) if woff[p + 1] > woff[p] and woff[p + 1] < total)
    engine.set_problem(prob.weights, prob.seq1, sem)
    codes_t = torch.from_numpy(prob.codes).to(DEV)
    offs_t = torch.from_numpy(prob.offsets).to(DEV)
    POISON = -777
    for cap in (0, 1, inside, edge - 1, edge, total - 1, total):
        rows_t = torch.full((total + 8, 3), POISON, dtype=torch.int32, device=DEV)
        toff_t = torch.full((prob.n * ts.T + 1,), POISON, dtype=torch.int64, device=DEV)
        engine.solve_targets_hits_device(codes_t, offs_t, prob.offsets, ts, min_score=thr, cap=cap, rows_t=rows_t,
                                         toffsets_t=toff_t)
        torch.cuda.synchronize()
        assert np.array_equal(toff_t.cpu().numpy(), woff), cap  # complete and exact whatever the capacity
        got = rows_t.cpu().numpy()
        same(got[:cap], want[:cap], ("cap", cap))
        assert (got[cap:] == POISON).all(), cap
    assert total >= 8 and 0 < inside < total and 0 < edge < total


# ---- the prefix sum over pairs -------------------------------------------------------------------------------
@pytest.mark.parametrize("n,T", [(341, 3), (256, 4), (205, 5)])
def test_scan_block_edges(engine, n, T):
    g0, _ = hits_geometry()
    assert n * T in (g0 - 1, g0, g0 + 1)
    rng = np.random.default_rng(n)
    prob, ts = random_case(n + 1, rng.integers(2, 9, T), rng.integers(1, 6, n))
    check_hits(engine, ("scan", n, T), prob, ts, Semantics.SPEC, min_score=-12)


def test_scan_past_one_pass_of_block_sums(engine):
    """More pairs than one pass of the scanning block takes (g0 * g1): n = 4097 records of 1 to 3 letters against
    T = 128 targets of 2 to 4."""
    g0, g1 = hits_geometry()
    n, T = 4097, 128
    assert n * T > g0 * g1
    rng = np.random.default_rng(7)
    prob, ts = random_case(8, rng.integers(2, 5, T), rng.integers(1, 4, n))
    rows, toffsets = check_hits(engine, "scan big", prob, ts, Semantics.SPEC, min_score=-6)
    assert toffsets[-1] == rows.shape[0] > n * T // 4


# ---- chunks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_one_record_per_chunk(engine, sem):
    """With one record per chunk the hit index must continue across chunks (every chunk's scan starts from the total
    the previous one left) and every chunk's lane group is chosen on its own."""
    prob, ts = random_case(31, [600, 7, 60, 40], [597, 560, 80, 5, 1, 600, 601, 30])
    key = "chunks"
    thr = mid_threshold(key, prob, ts, sem)
    engine.set_profile_scratch(256 << 20)
    whole_k = check_topk(engine, key, prob, ts, sem, 6)
    whole_r, whole_o = check_hits(engine, key, prob, ts, sem, min_score=thr)
    assert engine.stats()["chunks"] == 1
    try:
        engine.set_profile_scratch(8)  # one entry: every record runs alone
        assert np.array_equal(check_topk(engine, key, prob, ts, sem, 6), whole_k)
        assert engine.stats()["chunks"] == prob.n, engine.stats()
        rows, toffsets = check_hits(engine, key, prob, ts, sem, min_score=thr)
        assert engine.stats()["chunks"] == prob.n, engine.stats()
        assert np.array_equal(rows, whole_r) and np.array_equal(toffsets, whole_o)
    finally:
        engine.set_profile_scratch(256 << 20)


# ---- the optimistic host form --------------------------------------------------------------------------------
def test_second_pass_when_the_hint_is_too_small(engine):
    prob, ts = random_case(111, [20, 33], [5, 8, 3])
    sem = Semantics.SPEC
    want, woff = search_targets_hits_cpu(prob, ts, min_score=int(I32.min), semantics=sem)
    engine.set_problem(prob.weights, prob.seq1, sem)
    rows, toffsets = engine.solve_targets_hits(prob.codes, prob.offsets, ts, min_score=int(I32.min))
    assert engine.hits_passes() == 2 and woff[-1] > prob.n * ts.T  # the default room is n T rows
    same(rows, want, "two passes")
    rows, toffsets = engine.solve_targets_hits(prob.codes, prob.offsets, ts, min_score=int(I32.min), max_rows=int(woff[-1]))
    assert engine.hits_passes() == 1 and np.array_equal(toffsets, woff)
    same(rows, want, "one pass")
    D = 6
    best = search_targets_cpu(prob, ts, sem)[:, :, 0].astype(np.int64)
    by_hand = np.clip(best - D, I32.min, I32.max).astype(np.int32)
    w_rows, w_off = search_targets_hits_cpu(prob, ts, thresholds=by_hand, semantics=sem)
    rows, toffsets = engine.solve_targets_hits(prob.codes, prob.offsets, ts, within=D)
    assert np.array_equal(toffsets, w_off)
    same(rows, w_rows, "within")


# ---- device forms --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_device_forms_on_a_side_stream(engine, sem):
    """solve_targets_device -> thresholds = best - D -> solve_targets_hits_device queued on one side stream with no sync
    in between; the top-K form and the torch-facing ops beside them."""
    rng = np.random.default_rng(41)
    prob, ts = random_case(41, rng.integers(1, 60, 12), rng.integers(1, 30, 50))
    D, K = 5, 4
    want_k = cached(("device", sem, "topk"), lambda: search_targets_topk_cpu(prob, ts, K, sem))
    want_r, want_o = cached(("device", sem, "hits"), lambda: search_targets_hits_cpu(prob, ts, within=D, semantics=sem))
    engine.set_problem(prob.weights, prob.seq1, sem)
    codes_t = torch.from_numpy(prob.codes).to(DEV)
    offs_t = torch.from_numpy(prob.offsets).to(DEV)
    starts_t = torch.from_numpy(ts.starts).to(DEV)
    POISON = -777
    topk_t = torch.full((prob.n, ts.T, K, 3), POISON, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        best_t = engine.solve_targets_device(codes_t, offs_t, prob.offsets, ts, stream=side)
        thr_t = (best_t[:, :, 0].to(torch.int64) - D).clamp(I32.min, I32.max).to(torch.int32).contiguous()
        rows_t, toff_t = engine.solve_targets_hits_device(codes_t, offs_t, prob.offsets, ts, thresholds_t=thr_t,
                                                          cap=int(want_o[-1]) + 4, starts_t=starts_t, stream=side)
        st_hits = engine.stats()
        engine.solve_targets_topk_device(codes_t, offs_t, prob.offsets, ts, K, topk_t, stream=side)
        st_topk = engine.stats()
        topk2_t = align_targets_topk_device(engine, codes_t, offs_t, prob.offsets, ts.starts, K, stream=side)
        rows2_t, toff2_t = align_targets_hits_device(engine, codes_t, offs_t, prob.offsets, ts, thresholds_t=thr_t,
                                                     cap=0, stream=side)
    side.synchronize()  # once, at the end
    assert "targets_hits" in st_hits["kernels"] and "targets_topk" in st_topk["kernels"], (st_hits, st_topk)
    assert np.array_equal(toff_t.cpu().numpy(), want_o) and torch.equal(toff2_t, toff_t)
    same(rows_t.cpu().numpy()[:int(want_o[-1])], want_r, "device hits")
    same(topk_t.cpu().numpy().reshape(-1, K * 3), want_k.reshape(-1, K * 3), "device top-K")
    assert torch.equal(topk2_t, topk_t) and rows2_t.shape[0] == 0


# ---- wire forms --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_wire_forms(engine, sem):
    syn = make_synthetic("input6", 300, seed=5)
    rng = np.random.default_rng(51)
    cuts = np.sort(rng.choice(np.arange(1, syn.L1), size=6, replace=False))
    ts = TargetSet(syn.seq1, np.concatenate([[0], cuts, [syn.L1]]))
    by_bytes_k = check_topk(engine, "wire", syn, ts, sem, 3)
    by_bytes_r, by_bytes_o = check_hits(engine, "wire", syn, ts, sem, within=8)
    ws = WireSlice.from_csr(syn.codes, syn.offsets)
    assert ws.letter_format == "p33"
    rows = ws.solve_targets_topk_wire(engine, ts, 3, shift=6)
    assert {"targets_topk", "profile", "wire"} <= set(engine.stats()["kernels"]), engine.stats()
    assert np.array_equal(rows, by_bytes_k)
    hits, toffsets = ws.solve_targets_hits_wire(engine, ts, within=8, shift=6)
    assert {"targets_hits", "profile", "wire"} <= set(engine.stats()["kernels"]), engine.stats()
    assert np.array_equal(toffsets, by_bytes_o) and np.array_equal(hits, by_bytes_r)


# ---- the straddling record -----------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_straddling_record(engine, sem):
    rng = np.random.default_rng(2024)
    t1, t2 = (rng.integers(1, 27, size=60).astype(np.uint8) for _ in range(2))
    ts = TargetSet.from_sequences([t1, t2])
    codes, offsets = batch_of([np.concatenate([t1[40:], t2[:20]])])
    prob = Problem(list(W), ts.seq1, codes, offsets)
    topk = check_topk(engine, "straddle", prob, ts, sem, 64)
    rows, _ = check_hits(engine, "straddle", prob, ts, sem, min_score=int(I32.min))
    assert 160 not in topk[:, :, :, 0] and 160 not in rows[:, 0]  # the catalog's full match at offset 40 is in neither
    assert (rows[:, 1] + 40 <= 60).all() and (topk[:, :, :, 1] + 40 <= 60).all()


# ---- empty batch, refused calls --------------------------------------------------------------------------------
def test_empty_batch_and_refused_calls(engine):
    prob, ts = random_case(61, [5, 9], [3, 4])
    check_topk(engine, "two", prob, ts, Semantics.REFERENCE, 2)
    before = engine.stats()
    h_offsets = np.zeros(1, np.int64)
    rows = engine.solve_targets_topk(prob.codes[:0], h_offsets, ts, 2)
    assert rows.shape == (0, 2, 2, 3) and rows.dtype == np.int32
    hits, toffsets = engine.solve_targets_hits(prob.codes[:0], h_offsets, ts, min_score=0)
    assert hits.shape == (0, 3) and toffsets.tolist() == [0]
    codes_t = torch.zeros(16, dtype=torch.uint8, device=DEV)
    offs_t = torch.zeros(1, dtype=torch.int64, device=DEV)
    rows_t = align_targets_topk_device(engine, codes_t, offs_t, h_offsets, ts, 2)
    toff_t = torch.full((1,), -777, dtype=torch.int64, device=DEV)
    engine.solve_targets_hits_device(codes_t, offs_t, h_offsets, ts, min_score=0, toffsets_t=toff_t)
    torch.cuda.synchronize()
    assert tuple(rows_t.shape) == (0, 2, 2, 3) and toff_t.tolist() == [0]  # the one 8-byte memset
    for starts in ([1, 14], [0, 13], [0, 5, 5, 14], [0], list(range(15)) + [13]):
        with pytest.raises(ValueError, match="^targets:"):
            engine.solve_targets_topk(prob.codes, prob.offsets, starts, 0)  # the target set's error comes first
        with pytest.raises(ValueError, match="^targets:"):
            engine.solve_targets_hits(prob.codes, prob.offsets, starts)
    for K in (0, 65, -1):
        with pytest.raises(ValueError, match="^top-K: K must be in 1..64"):
            engine.solve_targets_topk(prob.codes, prob.offsets, ts, K)
    with pytest.raises(ValueError, match="^hits: give exactly one"):
        engine.solve_targets_hits(prob.codes, prob.offsets, ts, min_score=0, within=3)
    with pytest.raises(ValueError, match="^hits: thresholds must be"):
        engine.solve_targets_hits(prob.codes, prob.offsets, ts, thresholds=np.zeros((2, 3), np.int32))
    # the C ABI's host form: a bad capacity next to a bad target set reports the target set
    from mpi_openmp_cuda_amd import _lib
    bad = np.array([1, 14], np.int64)
    toffsets = np.zeros(prob.n * ts.T + 1, np.int64)
    for starts, prefix in ((bad, "targets:"), (ts.starts, "hits:")):
        rc = _lib.lib().moc_engine_solve_targets_hits(engine._h, _lib.ptr(prob.codes), _lib.ptr(prob.offsets), prob.n,
                                                      _lib.ptr(starts), starts.shape[0] - 1, 0, None, -1,
                                                      _lib.ptr(toffsets), None, 5)
        assert rc != 0 and _lib.lib().moc_last_error().decode().startswith(prefix)
    assert engine.stats() == before  # nothing ran: the last call's stats stand
