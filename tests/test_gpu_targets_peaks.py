"""GPU (MI355X / gfx950) tests of the per-target distinct placements (csrc/src/hip/targets_peaks_kernels.hip): per-target
top-K and hits with radius > 0, row for row equal to the CPU engine's search_targets_topk_cpu / search_targets_hits_cpu
with the same radius (tests/test_targets_peaks_cpu.py anchors those to search_topk_cpu / search_hits_cpu on every target
alone, and shows that the hostile case lists used here tell a window that leaks across a target edge from one that
does not). Smallest shapes that reach each edge: pair profiles around every segment width, the segment / tile cut and
the tile edges with hostile neighbours on both sides, the boundary entry as peak, suppressor, suppressed and tied,
candidate peaks exactly R and R + 1 apart, a plateau across a tile boundary, waves whose segments hold different
pairs, one record per chunk with the radius changing between calls on one engine, K against the peaks' count, the
hits contract, the device and wire forms, empty batches and refused calls. Every test runs once per forced lane-group
size (MOC_TARGETS_GROUP = 4, 16, 64), once per forced segment width (MOC_TARGETS_PEAKS_SEG = 4, 8, 16, 32, 64) and once with
the host's own choices, and asserts its path through stats()."""
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
                                 search_targets_cpu, search_targets_hits_cpu, search_targets_topk_cpu)
from targets_peaks_cases import (CLIPPING_CASES, HOSTILE_L2, I32, W, batch_of, hostile_case, pair_counts,  # noqa: E402
                                 target_len)

SEMS = [Semantics.REFERENCE, Semantics.SPEC]
# (forced lane group, forced segment width); None: the host chooses per chunk
CONFIGS = [(None, None), (4, None), (16, None), (64, None), (None, 4), (None, 8), (None, 16), (None, 32), (None, 64)]
DEV = torch.device("cuda:0")
NONE = [I32.min, 0, 0]
A, B = 1, 2  # two letters: a record of the single letter A scores 4 on an A and less on a B

_engines = {}


@pytest.fixture(params=CONFIGS, ids=lambda c: f"G{c[0] or 'auto'}-S{c[1] or 'auto'}")
def engine(request):
    """One engine per configuration, started with the two variables set (they are read at engine start)."""
    cfg = request.param
    if cfg not in _engines:
        names = ("MOC_TARGETS_GROUP", "MOC_TARGETS_PEAKS_SEG")
        old = {k: os.environ.pop(k, None) for k in names}
        for k, v in zip(names, cfg):
            if v:
                os.environ[k] = str(v)
        try:
            _engines[cfg] = HipSearchEngine(device=0)
        finally:
            for k in names:
                os.environ.pop(k, None)
                if old[k] is not None:
                    os.environ[k] = old[k]
    eng = _engines[cfg]
    eng.group, eng.seg = cfg
    return eng


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


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


def assert_path(st, kind, radius):
    names = set(st["kernels"])
    assert {kind, "profile"} <= names and not names & {"targets", "hits"}, st
    if radius > 0:
        assert {"peaks", "targets_peaks"} <= names, st
    else:
        assert not names & {"peaks", "targets_peaks"}, st


def check_topk(eng, key, prob, ts, sem, K, R):
    want = cached((key, sem, "topk", K, R), lambda: search_targets_topk_cpu(prob, ts, K, sem, radius=R))
    eng.set_problem(prob.weights, prob.seq1, sem)
    rows = eng.solve_targets_topk(prob.codes, prob.offsets, ts, K, radius=R)
    assert_path(eng.stats(), "targets_topk", R)
    same(rows.reshape(-1, K * 3), want.reshape(-1, K * 3), (key, "top-K", K, "R", R))
    return rows


def check_hits(eng, key, prob, ts, sem, R, **thr):
    tag = tuple((k, v if np.isscalar(v) else "array") for k, v in thr.items())
    want_rows, want_off = cached((key, sem, "hits", tag, R),
                                 lambda: search_targets_hits_cpu(prob, ts, semantics=sem, radius=R, **thr))
    eng.set_problem(prob.weights, prob.seq1, sem)
    rows, toffsets = eng.solve_targets_hits(prob.codes, prob.offsets, ts, radius=R, **thr)
    assert_path(eng.stats(), "targets_hits", R)
    assert toffsets.dtype == np.int64 and np.array_equal(toffsets, want_off), (key, "index", "R", R)
    same(rows, want_rows, (key, "hits", "R", R))
    return rows, toffsets


def all_peaks(eng, key, prob, ts, sem, R):
    """Every peak of every pair, as hits with every score admitted."""
    return check_hits(eng, key, prob, ts, sem, R, min_score=int(I32.min))


def peaks_of(rows, toffsets, T, i, t):
    p = i * T + t
    return rows[toffsets[p]:toffsets[p + 1], 1].tolist()


# ---- pair profile sizes with hostile neighbours on both sides ------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("name", list(CLIPPING_CASES))
def test_profile_sizes_with_hostile_neighbours(engine, sem, name):
    """Targets that are the pairs themselves — profiles of exactly the sizes around every segment width, the segment /
    tile cut and the tile edges — each between two catalog entries that outscore everything inside it. The lists "seg4"
    to "seg32" hold nothing longer than 4 / 8 / 16 / 32 entries next to the two 7-entry end targets, so the host's own
    choice takes the widths 8, 8, 16 and 32 there, and 64 on the other two."""
    sizes, radii = CLIPPING_CASES[name]
    prob, ts = hostile_case(sizes, sem)
    counts = pair_counts(prob, ts, sem)[0]
    assert counts.tolist() == [7] + list(sizes) + [7]
    full = 4 * HOSTILE_L2
    for R in radii:
        rows, toffsets = all_peaks(engine, ("hostile", name), prob, ts, sem, R)
        topk = check_topk(engine, ("hostile", name), prob, ts, sem, 3, R)
        for t, c in enumerate(counts):
            got = peaks_of(rows, toffsets, ts.T, 0, t)
            assert got and max(got) < c, (t, c, got)  # at least the best entry, and nothing outside the pair
            if R >= c - 1:
                assert len(got) == 1 and topk[0, t, 1].tolist() == NONE, (t, c, R, got)
    # the construction holds: the full matches lie across the edges, in no pair's profile
    best = cached(("hostile", name, sem, "best"), lambda: search_targets_cpu(prob, ts, sem))
    assert (best[0, 1:-1, 0] < full).all()


# ---- the boundary entry --------------------------------------------------------------------------------------
def boundary_targets():
    """Four 30-letter targets of B's for the record AAAAA (a full match scores 20, one A less 13 or less): the record
    at the very end (the boundary entry is the best); there and, shifted by one, nowhere else (it suppresses its
    neighbours); at the last slice offset but not at the boundary (a slice entry suppresses it); and a run of six A's at
    the end (boundary and last slice entry tie, the smaller offset wins)."""
    def t(a_from, a_to, n=30):
        s = np.full(n, B, np.uint8)
        s[a_from:a_to] = A
        return s
    return [t(25, 30), t(25, 30), t(24, 29), t(24, 30)]


def test_boundary_entry_under_spec(engine):
    sem = Semantics.SPEC
    ts = TargetSet.from_sequences(boundary_targets())
    codes, offsets = batch_of([np.full(5, A, np.uint8)])
    prob = Problem(list(W), ts.seq1, codes, offsets)
    slice_ = 25  # the boundary entry's local offset; 26 entries
    rows, toffsets = all_peaks(engine, "boundary", prob, ts, sem, 40)
    assert [peaks_of(rows, toffsets, 4, 0, t) for t in range(4)] == [[25], [25], [24], [24]]  # the only peak
    for R in (1, 3, 5):
        rows, toffsets = all_peaks(engine, "boundary", prob, ts, sem, R)
        p = [peaks_of(rows, toffsets, 4, 0, t) for t in range(4)]
        assert slice_ in p[0] and not set(range(slice_ - R, slice_)) & set(p[0]), (R, p[0])  # suppresses the last R
        assert slice_ not in p[2] and 24 in p[2], (R, p[2])  # suppressed by a slice entry
        assert slice_ not in p[3] and 24 in p[3], (R, p[3])  # tied with a slice entry: the smaller offset
        check_topk(engine, "boundary", prob, ts, sem, 4, R)
        check_hits(engine, "boundary", prob, ts, sem, R, min_score=20)


def test_last_target_of_the_records_length_under_reference(engine):
    """Reference semantics, T > 1, the last target exactly as long as the record: its one entry is the boundary
    entry, whose mark would lie one past the record's entries — the edge of the mark layout."""
    rng = np.random.default_rng(17)
    rec = rng.integers(1, 5, 6).astype(np.uint8)
    ts = TargetSet.from_sequences([rng.integers(1, 5, 20), rng.integers(1, 5, 9), rec])
    codes, offsets = batch_of([rec, rng.integers(1, 5, 6)])
    prob = Problem(list(W), ts.seq1, codes, offsets)
    for R in (1, 2, 64):
        rows, toffsets = all_peaks(engine, "one past", prob, ts, Semantics.REFERENCE, R)
        assert peaks_of(rows, toffsets, 3, 0, 2) == [0] and peaks_of(rows, toffsets, 3, 1, 2) == [0]
        check_topk(engine, "one past", prob, ts, Semantics.REFERENCE, 2, R)


# ---- distance ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("R", [1, 5, 63, 64, 2048])
def test_two_candidates_r_and_r_plus_one_apart(engine, sem, R):
    """A one-letter record A against two targets of B's with two A's each: exactly R apart (the second lies in the
    first's window and loses the tie to the smaller offset) and exactly R + 1 apart (both are peaks)."""
    n = 2 * R + 40
    near, far = np.full(n, B, np.uint8), np.full(n, B, np.uint8)
    near[[10, 10 + R]] = A
    far[[10, 11 + R]] = A
    ts = TargetSet.from_sequences([near, far])
    codes, offsets = batch_of([[A]])
    prob = Problem(list(W), ts.seq1, codes, offsets)
    rows, toffsets = check_hits(engine, ("distance", R), prob, ts, sem, R, min_score=4)
    assert peaks_of(rows, toffsets, 2, 0, 0) == [10] and peaks_of(rows, toffsets, 2, 0, 1) == [10, 11 + R]
    check_topk(engine, ("distance", R), prob, ts, sem, 3, R)


@pytest.mark.parametrize("sem", SEMS)
def test_plateau_across_a_tile_boundary(engine, sem):
    """Equal scores from local offset 2040 to 2060, across the tile kernel's edge at 2048: the run keeps its first
    offset at every radius; a target of equal scores throughout keeps offset 0 alone."""
    run = np.full(4200, B, np.uint8)
    run[2040:2061] = A
    flat = np.full(4200, B, np.uint8)
    ts = TargetSet.from_sequences([run, flat])
    codes, offsets = batch_of([[A]])
    prob = Problem(list(W), ts.seq1, codes, offsets)
    for R in (1, 7, 64, 2048):
        rows, toffsets = check_hits(engine, "plateau", prob, ts, sem, R, min_score=4)
        assert peaks_of(rows, toffsets, 2, 0, 0) == [2040], R
        rows, toffsets = all_peaks(engine, "plateau", prob, ts, sem, R)
        got = peaks_of(rows, toffsets, 2, 0, 1)
        assert got[0] == 0 and all(b - a > R for a, b in zip(got, got[1:])), (R, got[:5])


# ---- mixed waves ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("n,T", [(1, 1), (5, 13), (3, 23), (9, 29)])
def test_waves_of_mixed_segments(engine, sem, n, T):
    """Pairs of different profile sizes side by side in one wave, pairs that do not fit between fitting ones (records
    of 40 letters against targets of fewer), and pair counts that leave the last segment, wave and block partly empty."""
    rng = np.random.default_rng(100 * n + T)
    tl = rng.choice([1, 2, 3, 4, 6, 9, 17, 18, 33, 41, 66, 70, 130], T)
    rl = rng.choice([1, 2, 3, 5, 40], n)
    prob, ts = random_case(100 * n + T + 1, tl, rl)
    key = ("mixed", n, T)
    for R in (1, 3, 16):
        all_peaks(engine, key, prob, ts, sem, R)
        check_topk(engine, key, prob, ts, sem, 4, R)
    if T == 1:  # one target: the single-Seq1 distinct calls themselves
        engine.set_problem(prob.weights, prob.seq1, sem)
        top = engine.solve_targets_topk(prob.codes, prob.offsets, ts, 4, radius=3)
        same(top[:, 0].reshape(n, -1), engine.solve_topk(prob.codes, prob.offsets, 4, radius=3).reshape(n, -1), "T = 1")


# ---- chunks and stale marks ----------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_one_record_per_chunk_and_changing_radius(engine, sem):
    """One record per chunk through a scratch of one entry, then R = 3, R = 1 and R = 0 on the same batch and engine:
    the marks of an earlier chunk or call must never be read (the scratch is reused), and the R = 0 call runs no peak
    pass."""
    prob, ts = random_case(31, [300, 7, 60, 40, 2100], [297, 260, 80, 5, 1, 300, 301, 30])
    key = "chunks"
    engine.set_profile_scratch(256 << 20)
    whole = {R: (check_topk(engine, key, prob, ts, sem, 6, R), all_peaks(engine, key, prob, ts, sem, R)) for R in (3, 1, 0)}
    assert engine.stats()["chunks"] == 1
    try:
        engine.set_profile_scratch(8)  # one entry: every record runs alone
        for R in (3, 1, 0):
            assert np.array_equal(check_topk(engine, key, prob, ts, sem, 6, R), whole[R][0])
            assert engine.stats()["chunks"] == prob.n, engine.stats()
            rows, toffsets = all_peaks(engine, key, prob, ts, sem, R)
            assert engine.stats()["chunks"] == prob.n, engine.stats()
            assert np.array_equal(rows, whole[R][1][0]) and np.array_equal(toffsets, whole[R][1][1])
        assert whole[3][1][1][-1] < whole[1][1][1][-1] < whole[0][1][1][-1]  # fewer peaks at a larger radius
    finally:
        engine.set_profile_scratch(256 << 20)


# ---- K against the number of peaks ---------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("K", [1, 2, 64])
def test_k_against_the_number_of_peaks(engine, sem, K):
    prob, ts = random_case(70, [3, 40, 90, 300], [3, 3, 1])
    for R in (2, 20):
        rows = check_topk(engine, "K", prob, ts, sem, K, R)
        peaks, toffsets = all_peaks(engine, "K", prob, ts, sem, R)
        real = (rows[:, :, :, 0] != I32.min).sum(axis=2).reshape(-1)
        assert np.array_equal(real, np.minimum(np.diff(toffsets), K)), (K, R)  # min(K, #peaks) rows, then padding
        assert (rows[rows[:, :, :, 0] == I32.min] == NONE).all()
        if K == 64:
            assert (real < K).any() and (real > 1).any()
    best = search_targets_cpu(prob, ts, sem)
    same(rows[:, :, 0].reshape(-1, 3), best.reshape(-1, 3), "row 0 is solve_targets' row")


# ---- hits ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_hits_thresholds_capacity_and_second_pass(engine, sem):
    prob, ts = random_case(101, [9, 3, 30, 14, 70], [4, 9, 2, 6])
    key, R = "hits", 2
    rows, toffsets = check_hits(engine, key, prob, ts, sem, R, min_score=int(I32.max))
    assert rows.shape == (0, 3) and not toffsets.any()
    best = cached((key, sem, "best"), lambda: search_targets_cpu(prob, ts, sem))[:, :, 0]
    thr = int(np.median(best[best != I32.min])) - 8
    want, woff = check_hits(engine, key, prob, ts, sem, R, min_score=thr)
    per_pair = np.where(best == I32.min, I32.max, best).astype(np.int32)  # exactly each pair's best: one hit per pair
    rows, toffsets = check_hits(engine, key, prob, ts, sem, R, thresholds=per_pair)
    counts = np.diff(toffsets)
    assert np.array_equal(counts >= 1, best.reshape(-1) != I32.min)  # a pair's best entry is always a peak
    assert np.array_equal(rows[:, 0], np.repeat(best.reshape(-1), counts))
    check_hits(engine, key, prob, ts, sem, R, within=6)
    # the capacity contract over guard rows, the index complete whatever the capacity
    total = int(woff[-1])
    inside = next(int(woff[p]) + 1 for p in range(len(woff) - 1) if woff[p + 1] - woff[p] >= 3)
    assert total >= 6 and 0 < inside < total
    engine.set_problem(prob.weights, prob.seq1, sem)
    codes_t = torch.from_numpy(prob.codes).to(DEV)
    offs_t = torch.from_numpy(prob.offsets).to(DEV)
    POISON = -777
    for cap in (0, 1, inside, total - 1, total):
        rows_t = torch.full((total + 8, 3), POISON, dtype=torch.int32, device=DEV)
        toff_t = torch.full((prob.n * ts.T + 3,), POISON, dtype=torch.int64, device=DEV)
        engine.solve_targets_hits_device(codes_t, offs_t, prob.offsets, ts, min_score=thr, cap=cap, rows_t=rows_t,
                                         toffsets_t=toff_t[1:-1], radius=R)
        torch.cuda.synchronize()
        got_off = toff_t.cpu().numpy()
        assert np.array_equal(got_off[1:-1], woff) and got_off[0] == POISON and got_off[-1] == POISON, cap
        got = rows_t.cpu().numpy()
        same(got[:cap], want[:cap], ("cap", cap))
        assert (got[cap:] == POISON).all(), cap
    # the optimistic host form: a second pass when the hint is too small
    rows, toffsets = engine.solve_targets_hits(prob.codes, prob.offsets, ts, min_score=thr, max_rows=1, radius=R)
    assert engine.hits_passes() == 2 and np.array_equal(toffsets, woff)
    same(rows, want, "two passes")
    rows, toffsets = engine.solve_targets_hits(prob.codes, prob.offsets, ts, min_score=thr, max_rows=total, radius=R)
    assert engine.hits_passes() == 1
    same(rows, want, "one pass")


# ---- device and wire forms -----------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_device_forms_on_a_side_stream(engine, sem):
    """solve_targets_device -> thresholds = best - D -> solve_targets_hits_device(radius=R) queued on one side stream
    with no sync in between; the top-K form and the torch-facing ops beside them."""
    rng = np.random.default_rng(41)
    prob, ts = random_case(41, rng.integers(1, 90, 12), rng.integers(1, 30, 50))
    D, K, R = 5, 4, 3
    want_k = cached(("device", sem, "topk"), lambda: search_targets_topk_cpu(prob, ts, K, sem, radius=R))
    want_r, want_o = cached(("device", sem, "hits"),
                            lambda: search_targets_hits_cpu(prob, ts, within=D, semantics=sem, radius=R))
    engine.set_problem(prob.weights, prob.seq1, sem)
    codes_t = torch.from_numpy(prob.codes).to(DEV)
    offs_t = torch.from_numpy(prob.offsets).to(DEV)
    starts_t = torch.from_numpy(ts.starts).to(DEV)
    topk_t = torch.full((prob.n, ts.T, K, 3), -777, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        best_t = engine.solve_targets_device(codes_t, offs_t, prob.offsets, ts, stream=side)
        thr_t = (best_t[:, :, 0].to(torch.int64) - D).clamp(I32.min, I32.max).to(torch.int32).contiguous()
        rows_t, toff_t = engine.solve_targets_hits_device(codes_t, offs_t, prob.offsets, ts, thresholds_t=thr_t,
                                                          cap=int(want_o[-1]) + 4, starts_t=starts_t, stream=side,
                                                          radius=R)
        st_hits = engine.stats()
        engine.solve_targets_topk_device(codes_t, offs_t, prob.offsets, ts, K, topk_t, stream=side, radius=R)
        st_topk = engine.stats()
        topk2_t = align_targets_topk_device(engine, codes_t, offs_t, prob.offsets, ts.starts, K, stream=side, radius=R)
        rows2_t, toff2_t = align_targets_hits_device(engine, codes_t, offs_t, prob.offsets, ts, thresholds_t=thr_t,
                                                     cap=0, stream=side, radius=R)
    side.synchronize()  # once, at the end
    assert_path(st_hits, "targets_hits", R)
    assert_path(st_topk, "targets_topk", R)
    assert np.array_equal(toff_t.cpu().numpy(), want_o) and torch.equal(toff2_t, toff_t)
    same(rows_t.cpu().numpy()[:int(want_o[-1])], want_r, "device hits")
    same(topk_t.cpu().numpy().reshape(-1, K * 3), want_k.reshape(-1, K * 3), "device top-K")
    assert torch.equal(topk2_t, topk_t) and rows2_t.shape[0] == 0


@pytest.mark.parametrize("sem", SEMS)
def test_wire_forms(engine, sem):
    syn = make_synthetic("input6", 300, seed=5)
    rng = np.random.default_rng(51)
    cuts = np.sort(rng.choice(np.arange(1, syn.L1), size=6, replace=False))
    ts = TargetSet(syn.seq1, np.concatenate([[0], cuts, [syn.L1]]))
    R = 2
    by_bytes_k = check_topk(engine, "wire", syn, ts, sem, 3, R)
    by_bytes_r, by_bytes_o = check_hits(engine, "wire", syn, ts, sem, R, within=8)
    ws = WireSlice.from_csr(syn.codes, syn.offsets)
    rows = ws.solve_targets_topk_wire(engine, ts, 3, shift=6, radius=R)
    assert {"targets_topk", "targets_peaks", "profile", "wire"} <= set(engine.stats()["kernels"]), engine.stats()
    assert np.array_equal(rows, by_bytes_k)
    hits, toffsets = ws.solve_targets_hits_wire(engine, ts, within=8, shift=6, radius=R)
    assert {"targets_hits", "targets_peaks", "profile", "wire"} <= set(engine.stats()["kernels"]), engine.stats()
    assert np.array_equal(toffsets, by_bytes_o) and np.array_equal(hits, by_bytes_r)


# ---- empty batch, refused calls ------------------------------------------------------------------------------
def test_empty_batch_and_refused_calls(engine):
    prob, ts = random_case(61, [5, 9], [3, 4])
    check_topk(engine, "two", prob, ts, Semantics.REFERENCE, 2, 1)
    before = engine.stats()
    h_offsets = np.zeros(1, np.int64)
    rows = engine.solve_targets_topk(prob.codes[:0], h_offsets, ts, 2, radius=3)
    assert rows.shape == (0, 2, 2, 3) and rows.dtype == np.int32
    hits, toffsets = engine.solve_targets_hits(prob.codes[:0], h_offsets, ts, min_score=0, radius=3)
    assert hits.shape == (0, 3) and toffsets.tolist() == [0]
    codes_t = torch.zeros(16, dtype=torch.uint8, device=DEV)
    offs_t = torch.zeros(1, dtype=torch.int64, device=DEV)
    rows_t = align_targets_topk_device(engine, codes_t, offs_t, h_offsets, ts, 2, radius=3)
    toff_t = torch.full((1,), -777, dtype=torch.int64, device=DEV)
    engine.solve_targets_hits_device(codes_t, offs_t, h_offsets, ts, min_score=0, toffsets_t=toff_t, radius=3)
    torch.cuda.synchronize()
    assert tuple(rows_t.shape) == (0, 2, 2, 3) and toff_t.tolist() == [0]
    # the order: the target set, then K / the hits arguments, then the radius
    with pytest.raises(ValueError, match="^targets:"):
        engine.solve_targets_topk(prob.codes, prob.offsets, [1, 14], 0, radius=-1)
    with pytest.raises(ValueError, match="^targets:"):
        engine.solve_targets_hits(prob.codes, prob.offsets, [1, 14], radius=-1)
    with pytest.raises(ValueError, match="^top-K: K must be in 1..64"):
        engine.solve_targets_topk(prob.codes, prob.offsets, ts, 0, radius=-1)
    with pytest.raises(ValueError, match="^hits: give exactly one"):
        engine.solve_targets_hits(prob.codes, prob.offsets, ts, min_score=0, within=3, radius=-1)
    for bad in (-1, 2049, 1.5, True):
        with pytest.raises(ValueError, match="^distinct: radius must be"):
            engine.solve_targets_topk(prob.codes, prob.offsets, ts, 2, radius=bad)
        with pytest.raises(ValueError, match="^distinct: radius must be"):
            engine.solve_targets_hits(prob.codes, prob.offsets, ts, within=3, radius=bad)  # before `within` runs a search
    # the C ABI itself refuses the radius after the target set, before any work
    from mpi_openmp_cuda_amd import _lib
    out = np.zeros((prob.n, ts.T, 2, 3), np.int32)
    for starts, prefix in ((np.array([1, 14], np.int64), "targets:"), (ts.starts, "distinct:")):
        rc = _lib.lib().moc_engine_solve_targets_topk_distinct(engine._h, _lib.ptr(prob.codes), _lib.ptr(prob.offsets),
                                                               prob.n, _lib.ptr(starts), starts.shape[0] - 1, 2, 2049,
                                                               _lib.ptr(out))
        assert rc != 0 and _lib.lib().moc_last_error().decode().startswith(prefix)
    assert engine.stats() == before  # nothing ran: the last call's stats stand
    assert target_len(1, 5, Semantics.SPEC) == 5
