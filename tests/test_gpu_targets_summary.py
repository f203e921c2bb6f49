"""GPU (MI355X / gfx950) tests of the per-target profile summary (csrc/src/hip/targets_summary_kernels.hip): summary
rows and histograms exactly equal to the CPU engine's search_targets_summary_cpu (tests/test_targets_summary_cpu.py
anchors that one to search_summary_cpu run on every target alone) under both semantics, at the smallest shapes that
reach each edge of the lane-group kernels — slice and record lengths around the group size, pair counts that leave
the last wave and block partly idle, histogram bin counts at the edges of the LDS rule, int64 sums next to 2^63, one
record per chunk, the device form on a side stream feeding targets_zscore and targets_best, the wire form, empty
batches and refused calls. Every test runs once per forced lane-group size (MOC_TARGETS_GROUP = 4, 16, 64, read when an
engine starts) and once with the host's own choice."""
import os

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = pytest.mark.gpu

if not gpu_available():  # pragma: no cover - collected on CPU hosts only with -m gpu
    pytest.skip("no GPU", allow_module_level=True)

import torch  # noqa: E402

from mpi_openmp_cuda_amd import (HipSearchEngine, Problem, Semantics, TargetSet, WireSlice,  # noqa: E402
                                 align_targets_summary_device, make_synthetic, search_targets_summary_cpu, targets_best,
                                 targets_zscore)
from mpi_openmp_cuda_amd.ops.align import (native_score_table, targets_geometry,  # noqa: E402
                                           targets_summary_geometry)

SEMS = [Semantics.REFERENCE, Semantics.SPEC]
GROUPS = [None, 4, 16, 64]  # None: the host chooses per chunk
W = (4, 3, 2, 10)
DEV = torch.device("cuda:0")
I32 = np.iinfo(np.int32)
NO_FIT = [0, 0, 0, I32.max, I32.min, 0, 0]

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


def random_case(seed, target_lens, record_lens, alphabet=4, weights=W):
    rng = np.random.default_rng(seed)
    ts = TargetSet.from_sequences([rng.integers(1, alphabet + 1, int(l)) for l in target_lens])
    codes, offsets = batch_of([rng.integers(1, alphabet + 1, int(l)) for l in record_lens])
    return Problem(list(weights), ts.seq1, codes, offsets), ts


_oracle = {}


def oracle(key, prob, ts, sem, bins=0, lo=0, width=1):
    """The CPU engine's (summary, hist) of a shared problem: computed once, read-only."""
    k = (key, sem, bins, lo, width)
    if k not in _oracle:
        s, h = search_targets_summary_cpu(prob, ts, bins, lo, width, sem)
        s.setflags(write=False)
        if h is not None:
            h.setflags(write=False)
        _oracle[k] = (s, h)
    return _oracle[k]


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype)
    bad = np.argwhere((got != want).any(axis=-1))
    assert bad.size == 0, (what, bad[:8].tolist(), [got[tuple(b)].tolist() for b in bad[:4]],
                           [want[tuple(b)].tolist() for b in bad[:4]])


def check(eng, key, prob, ts, sem, bins=0, lo=0, width=1):
    """Host form against the oracle; returns (summary, hist)."""
    ws, wh = oracle(key, prob, ts, sem, bins, lo, width)
    eng.set_problem(prob.weights, prob.seq1, sem)
    s, h = eng.solve_targets_summary(prob.codes, prob.offsets, ts, bins, lo, width)
    st = eng.stats()
    assert "targets_summary" in st["kernels"] and "profile" in st["kernels"] and "targets" not in st["kernels"], st
    same(s, ws, (key, "summary"))
    if bins:
        same(h, wh, (key, "hist", bins, lo, width))
        assert np.array_equal(h.astype(np.int64).sum(axis=2), s[:, :, 0])
    else:
        assert h is None
    return s, h


# ---- slice and record lengths around the group size --------------------------------------------------------
def edge_lengths(g):
    slices = [0, 1, g - 1, g, g + 1, 2 * g + 1] + ([127, 129] if g == 64 else [])
    records = [1, 2, g - 1, g + 1]
    return slices, records


@pytest.mark.parametrize("bins", [0, 5])
@pytest.mark.parametrize("sem", SEMS)
def test_slice_and_record_length_edges(engine, sem, bins):
    """Every record length L2 in {1, 2, G - 1, G + 1} meets a target of L2 + s letters for every slice length s in
    {0, 1, G - 1, G, G + 1, 2G + 1} (G = 64: also 127, 129): the slice loop and the boundary entry's letter loop each
    run 0, 1, G - 1, G + 1 and more than 2G steps; spec adds the boundary entry to every slice, reference has it at
    s = 0 only. The host's own choice gets the lengths of all three sizes."""
    gs = [engine.group] if engine.group else [4, 16, 64]
    target_lens, record_lens = [], []
    for g in gs:
        slices, records = edge_lengths(g)
        record_lens += records
        target_lens += [l2 + s for l2 in records for s in slices]
    prob, ts = random_case(11, target_lens, record_lens)
    s, _ = check(engine, ("edges", engine.group), prob, ts, sem, bins, -40, 25)
    L2 = np.diff(prob.offsets)
    fits = L2[:, None] <= ts.lengths[None, :]
    assert np.array_equal(s[:, :, 0] > 0, fits) and fits.any() and not fits.all()
    assert (s[~fits] == NO_FIT).all()
    spec = sem == Semantics.SPEC
    count = ts.lengths[None, :] - L2[:, None] + (spec | (ts.lengths[None, :] == L2[:, None]))
    assert np.array_equal(s[:, :, 0][fits], count[fits])


# ---- pair counts: the last wave and block partly idle ------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("n,T", [(1, 1), (5, 3), (17, 1), (1, 17), (9, 7), (257, 1), (1, 257)])
def test_pair_counts(engine, sem, n, T):
    rng = np.random.default_rng(n * 1000 + T)
    prob, ts = random_case(n * 1000 + T + 1, rng.integers(1, 40, T), rng.integers(1, 13, n))
    s, h = check(engine, ("pairs", n, T), prob, ts, sem, 5, -30, 20)
    if T == 1:  # one target: the summary itself
        s1, h1 = engine.solve_summary(prob.codes, prob.offsets, 5, -30, 20)
        same(s[:, 0], s1, "T = 1 against solve_summary")
        same(h[:, 0], h1, "T = 1 against solve_summary's histogram")


# ---- histogram: the LDS rule's edges -----------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_histogram_bin_counts_at_the_lds_rule(engine, sem):
    """bins = 1, 63, 64, 65, 255, 256: up to 64 bins a 4-lane group keeps its counters, past them the histogram's
    group is 16 lanes (bounds::targets_hist_group): the engine forced to 4 lanes crosses the rule between 64 and 65
    bins. Scores lie below lo and past the last edge: both end bins collect."""
    _, max_bins, group4_bins, lds = targets_summary_geometry()
    assert (group4_bins, max_bins, lds) == (64, 256, 16384)
    prob, ts = random_case(71, [9, 30, 31, 70, 3, 140], [8, 9, 2, 1, 40], alphabet=3, weights=(10, 50, 50, 50))
    s0, _ = oracle("lds", prob, ts, sem)
    fit = s0[:, :, 0] > 0
    lo_s, hi_s = int(s0[:, :, 3][fit].min()), int(s0[:, :, 4][fit].max())
    assert lo_s < -1000 and hi_s > 0
    for bins in (1, group4_bins - 1, group4_bins, group4_bins + 1, max_bins - 1, max_bins):
        width = max((hi_s - lo_s) // (2 * bins), 1)
        lo = lo_s + (hi_s - lo_s) // 4  # a quarter of the range lies below lo
        _, h = check(engine, "lds", prob, ts, sem, bins, lo, width)
        assert h[:, :, 0].sum() > 0 and h[:, :, -1].sum() > 0
    _, h = check(engine, "lds", prob, ts, sem, max_bins, hi_s + 1000, 7)  # lo above all scores: everything in bin 0
    assert np.array_equal(h[:, :, 0], s0[:, :, 0]) and (h[:, :, 1:] == 0).all()
    _, h = check(engine, "lds", prob, ts, sem, group4_bins + 1, int(I32.min), int(I32.max))


# ---- wide arithmetic -----------------------------------------------------------------------------------------
def other_class_letters(weights):
    """Three letters whose three pairs all score -w4 (mutually neither identical, conservative nor semi-conservative)."""
    lut = native_score_table(list(weights))  # int32 [32, 32]
    w4 = -int(weights[3])
    for a in range(1, 27):
        for b in range(a + 1, 27):
            for c in range(b + 1, 27):
                if lut[a][b] == w4 and lut[a][c] == w4 and lut[b][c] == w4 and lut[b][a] == w4:
                    return a, b, c
    raise AssertionError("no three mutually unrelated letters")


def wide_case(entries, sem, periodic):
    """Weights (10^6, 3, 2, 10^6) and one 500-letter record, M = 5 * 10^8, against a target with `entries` profile
    entries. periodic: record and target repeat three mutually unrelated letters, so offsets 0, 1, 2 (mod 3) score
    +M (all identical), -M (every candidate all unrelated) and about +M (one unrelated pair, then identical): the sum
    cancels to a third while the sum of squares grows to 36 M^2 > 2^62. Else one repeated letter: every score is M."""
    w = (1_000_000, 3, 2, 1_000_000)
    length = 500 + entries - (1 if sem == Semantics.SPEC else 0)
    pat = np.array(other_class_letters(w) if periodic else (1, 1, 1), np.uint8)
    target = np.resize(pat, length)
    ts = TargetSet.from_sequences([np.full(7, 2, np.uint8), target])  # a short first target: b > 0, and a pair that does not fit
    codes, offsets = batch_of([np.resize(pat, 500)])
    return Problem(list(w), ts.seq1, codes, offsets), ts


@pytest.mark.parametrize("sem", SEMS)
def test_wide_arithmetic_and_refusal(engine, sem):
    M = 500_000_000
    prob, ts = wide_case(36, sem, periodic=False)
    s, _ = check(engine, "wide36", prob, ts, sem)
    assert s[0, 1].tolist() == [36, 36 * M, 36 * M * M, M, M, 0, 0] and s[0, 1, 2] > 2 ** 62
    assert s[0, 0].tolist() == NO_FIT
    prob, ts = wide_case(36, sem, periodic=True)
    s, h = check(engine, "wide36 mixed", prob, ts, sem, 4, -M, M // 2)
    assert s[0, 1, 0] == 36 and s[0, 1, 3] == -M and s[0, 1, 4] == M and s[0, 1, 5:].tolist() == [0, 0]
    assert abs(int(s[0, 1, 1])) < 13 * M and s[0, 1, 2] > 35 * M * M  # the sum cancels, the sum of squares does not
    before = engine.stats()
    bad, bts = wide_case(37, sem, periodic=True)
    engine.set_problem(bad.weights, bad.seq1, sem)
    with pytest.raises(ValueError, match="^summary: exactness bound"):
        engine.solve_targets_summary(bad.codes, bad.offsets, bts)
    codes_t = torch.from_numpy(bad.codes).to(DEV)
    offs_t = torch.from_numpy(bad.offsets).to(DEV)
    out_t = torch.full((1, 2, 7), -777, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="^summary: exactness bound"):
        engine.solve_targets_summary_device(codes_t, offs_t, bad.offsets, bts, summary_t=out_t)
    torch.cuda.synchronize()
    assert (out_t == -777).all() and engine.stats() == before  # refused before any launch


def test_catalog_past_the_bound_is_accepted(engine):
    """Two targets of 36 entries each: the catalog's own profile (572 entries) is refused by solve_summary, every
    target's own is within the bound."""
    w = (1_000_000, 3, 2, 1_000_000)
    rng = np.random.default_rng(5)
    ts = TargetSet.from_sequences([rng.integers(1, 27, 536).astype(np.uint8) for _ in range(2)])
    codes, offsets = batch_of([rng.integers(1, 27, 500).astype(np.uint8)])
    prob = Problem(list(w), ts.seq1, codes, offsets)
    s, _ = check(engine, "two536", prob, ts, Semantics.REFERENCE, 3, -10 ** 8, 10 ** 8)
    assert (s[0, :, 0] == 36).all()
    with pytest.raises(ValueError, match="^summary: exactness bound"):
        engine.solve_summary(prob.codes, prob.offsets)


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
    whole = check(engine, "chunks", prob, ts, sem, 70, -200, 9)
    assert engine.stats()["chunks"] == 1
    try:
        engine.set_profile_scratch(8)  # one entry: every record runs alone
        chunked = check(engine, "chunks", prob, ts, sem, 70, -200, 9)
        assert engine.stats()["chunks"] == prob.n, engine.stats()
        assert np.array_equal(chunked[0], whole[0]) and np.array_equal(chunked[1], whole[1])
    finally:
        engine.set_profile_scratch(256 << 20)


# ---- device form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_device_form_feeds_zscore_and_best_on_a_side_stream(engine, sem):
    rng = np.random.default_rng(41)
    prob, ts = random_case(41, rng.integers(1, 60, 12), rng.integers(1, 30, 50))
    ws, wh = oracle("device", prob, ts, sem, 6, -60, 30)
    engine.set_problem(prob.weights, prob.seq1, sem)
    codes_t = torch.from_numpy(prob.codes).to(DEV)
    offs_t = torch.from_numpy(prob.offsets).to(DEV)
    starts_t = torch.from_numpy(ts.starts).to(DEV)
    POISON = -777
    s_t = torch.full((prob.n, ts.T, 7), POISON, dtype=torch.int64, device=DEV)
    h_t = torch.full((prob.n, ts.T, 6), POISON, dtype=torch.int32, device=DEV)
    h0_t = torch.full((prob.n, ts.T, 6), POISON, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        engine.solve_targets_summary_device(codes_t, offs_t, prob.offsets, ts, 6, -60, 30, s_t, h_t, stream=side)
        st = engine.stats()
        z_t = targets_zscore(s_t)
        rows_t = s_t[:, :, 4:7].to(torch.int32).contiguous()
        best_t, best_row_t = targets_best(rows_t, z_t)
        s2_t, none_t = engine.solve_targets_summary_device(codes_t, offs_t, prob.offsets, ts.starts, hist_t=h0_t,
                                                           starts_t=starts_t, stream=side)  # bins = 0
        s3_t, h3_t = align_targets_summary_device(engine, codes_t, offs_t, prob.offsets, ts, 6, -60, 30, stream=side)
    side.synchronize()  # once, at the end
    assert "targets_summary" in st["kernels"] and "profile" in st["kernels"], st
    same(s_t.cpu().numpy(), ws, "device summary")
    same(h_t.cpu().numpy(), wh, "device hist")
    assert torch.equal(s2_t, s_t) and torch.equal(s3_t, s_t) and torch.equal(h3_t, h_t)
    assert none_t is h0_t and (h0_t == POISON).all()  # bins = 0 touches no histogram buffer
    wz = targets_zscore(ws)
    z = z_t.cpu().numpy()
    assert np.array_equal(np.isnan(z), np.isnan(wz)) and np.allclose(z, wz, rtol=1e-9, atol=0, equal_nan=True)
    wb, wr = targets_best(np.ascontiguousarray(ws[:, :, 4:7]).astype(np.int32), z)
    assert np.array_equal(best_t.cpu().numpy(), wb) and np.array_equal(best_row_t.cpu().numpy(), wr)
    assert (wb >= 0).any()


# ---- wire form -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_wire_form(engine, sem):
    syn = make_synthetic("input6", 700, seed=5)
    rng = np.random.default_rng(51)
    cuts = np.sort(rng.choice(np.arange(1, syn.L1), size=6, replace=False))
    ts = TargetSet(syn.seq1, np.concatenate([[0], cuts, [syn.L1]]))
    by_bytes = check(engine, "wire", syn, ts, sem, 5, -100, 40)
    ws = WireSlice.from_csr(syn.codes, syn.offsets)
    assert ws.letter_format == "p33"
    s, h = ws.solve_targets_summary_wire(engine, ts, 5, -100, 40, shift=6)
    st = engine.stats()
    assert {"targets_summary", "profile", "wire"} <= set(st["kernels"]), st
    same(s, by_bytes[0], "wire summary")
    same(h, by_bytes[1], "wire hist")


# ---- empty batch, refused calls ------------------------------------------------------------------------------
def test_empty_batch_and_refused_calls(engine):
    prob, ts = random_case(61, [5, 9], [3, 4])
    check(engine, "two", prob, ts, Semantics.REFERENCE, 4, 0, 3)
    before = engine.stats()
    assert before["kernels"] == ["profile", "targets_summary"]
    h_offsets = np.zeros(1, np.int64)
    s, h = engine.solve_targets_summary(prob.codes[:0], h_offsets, ts, 4)
    assert s.shape == (0, 2, 7) and s.dtype == np.int64 and h.shape == (0, 2, 4) and h.dtype == np.int32
    codes_t = torch.zeros(16, dtype=torch.uint8, device=DEV)
    offs_t = torch.zeros(1, dtype=torch.int64, device=DEV)
    s_t, h_t = align_targets_summary_device(engine, codes_t, offs_t, h_offsets, ts, 4)
    torch.cuda.synchronize()
    assert tuple(s_t.shape) == (0, 2, 7) and tuple(h_t.shape) == (0, 2, 4)
    for starts in ([1, 14], [0, 13], [0, 5, 5, 14], [0], list(range(15)) + [13]):
        with pytest.raises(ValueError, match="^targets:"):
            engine.solve_targets_summary(prob.codes, prob.offsets, starts)
    for kw in ({"bins": -1}, {"bins": 257}, {"bins": 4, "width": 0}):
        with pytest.raises(ValueError, match="^summary:"):
            engine.solve_targets_summary(prob.codes, prob.offsets, ts, **kw)
    assert engine.stats() == before  # nothing ran: the last call's stats stand
