"""GPU (MI355X / gfx950) tests of the alignment report kernels (csrc/src/hip/report_kernels.hip): every case is
exact against the CPU engine's search_report_cpu (tests/test_report_cpu.py anchors that one to the pure-Python
alignment_string) at the smallest shapes that reach each edge — the lane-per-row / wave-per-row threshold (64
letters) and the packed-counter bound (255), 64-letter chunk edges, the first and last Seq1 positions, batch sizes
around a wave's 64 rows, an unaligned letter span, K rows per record with top-K padding, out-of-range rows, a
Seq1 past its LDS staging. Every call must report the report kernels in its stats."""
import numpy as np
import pytest

from conftest import expected, gpu_available, input_path

pytestmark = pytest.mark.gpu

if not gpu_available():  # pragma: no cover - collected on CPU hosts only with -m gpu
    pytest.skip("no GPU", allow_module_level=True)

import torch  # noqa: E402

from mpi_openmp_cuda_amd import (HipSearchEngine, Problem, Semantics, align_report_device,  # noqa: E402
                                 align_search_device, align_topk_device, format_report, report_scores, search_cpu,
                                 search_report_cpu, search_topk_cpu)
from mpi_openmp_cuda_amd.ops.align import as_triples  # noqa: E402

W = (10, 2, 3, 4)
DEV = torch.device("cuda:0")
INT32_MIN = int(np.iinfo(np.int32).min)
SHORT_MAX = 64      # csrc/include/moc/kernel_bounds.hpp kReportShortMaxL2
PACKED_MAX = 255    # ... kReportPackedCountMax


@pytest.fixture(scope="module")
def engine():
    e = HipSearchEngine(device=0)
    yield e
    e.close()


def problem_of(weights, seq1, recs) -> Problem:
    lens = np.array([len(r) for r in recs], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    codes = np.concatenate([np.asarray(r, np.uint8) for r in recs]) if len(recs) else np.zeros(0, np.uint8)
    return Problem(list(weights), np.asarray(seq1, np.uint8), codes, offsets)


def letter(ch: str) -> int:
    return ord(ch) - ord("A") + 1


def check(eng, prob, rows, marks=True):
    """engine.report == search_report_cpu, counts and marker bytes; returns the counts."""
    want_c, want_m = search_report_cpu(prob, rows, marks=True)
    eng.set_problem(prob.weights, prob.seq1)
    got = eng.report(prob.codes, prob.offsets, rows, marks=marks)
    st = eng.stats()
    assert "report" in st["kernels"] or prob.n == 0, st
    got_c, got_m = got if marks else (got, None)
    assert got_c.shape == want_c.shape and got_c.dtype == np.int32
    bad = np.argwhere(got_c != want_c)
    assert bad.size == 0, (bad[:8], got_c[tuple(bad[0][:-1])], want_c[tuple(bad[0][:-1])])
    if marks:
        badm = np.flatnonzero(got_m != want_m)
        assert badm.size == 0, (badm[:8], got_m[badm[:8]], want_m[badm[:8]])
    return got_c


def edge_rows(L1, lens):
    """Per record the issue's seven rows: (n, k) in {0, L1 - L2 - 1} x {0, 1, L2 - 1}, then the spec row."""
    rows = np.zeros((len(lens), 7, 3), np.int32)
    for i, L2 in enumerate(lens):
        q = 0
        for n in (0, L1 - L2 - 1):
            for k in (0, 1, L2 - 1):
                rows[i, q] = (1, n, k)
                q += 1
        rows[i, 6] = (1, L1 - L2, 0)
    return rows


def test_length_sweep(engine):
    L1 = 300
    lens = list(range(1, 131)) + [255, 256, 257, 258]
    assert SHORT_MAX in lens and SHORT_MAX + 1 in lens and PACKED_MAX in lens and PACKED_MAX + 1 in lens
    rng = np.random.default_rng(1)
    prob = problem_of(W, rng.integers(1, 27, L1), [rng.integers(1, 27, l) for l in lens])
    rows = edge_rows(L1, lens)
    counts = check(engine, prob, rows)  # K = 7: nine records per wave
    real = counts[..., 0] >= 0
    assert np.array_equal(counts.sum(-1)[real], np.broadcast_to(np.array(lens)[:, None], real.shape)[real])
    assert real[1:, :].all() and real[0, [0, 3, 6]].all()  # only L2 = 1 with k = 1 is out of range
    for q in range(7):  # and one row per record, K = 1
        check(engine, prob, np.ascontiguousarray(rows[:, q]), marks=(q % 2 == 0))


def test_one_class_takes_everything(engine):
    L1 = 300
    lens = sorted({1, SHORT_MAX, SHORT_MAX + 1, 63, 64, 65, PACKED_MAX, 256, 257})
    recs, cls = [], []
    for c, ch in enumerate("ASCB"):  # against 'A': '$', '%', '#', ' '
        for l in lens:
            recs.append(np.full(l, letter(ch), np.uint8))
            cls.append(c)
    prob = problem_of(W, np.full(L1, letter("A"), np.uint8), recs)
    L2 = np.asarray(prob.lengths)
    rows = np.stack([np.ones(prob.n), np.zeros(prob.n), np.minimum(L2 - 1, 1)], 1).astype(np.int32)
    for r in (rows, rows * [1, 1, 0]):
        counts = check(engine, prob, np.ascontiguousarray(r.astype(np.int32)))
        want = np.zeros((prob.n, 4), np.int64)
        want[np.arange(prob.n), cls] = L2
        assert np.array_equal(counts, want)


def test_long_row_past_lds_and_16_bits(engine):
    L1, L2 = 70_001, 70_000
    recs = [np.full(L2, letter(ch), np.uint8) for ch in "ASCB"]
    prob = problem_of(W, np.full(L1, letter("A"), np.uint8), recs)
    rows = np.tile(np.array([[1, 0, 0], [1, 0, 1], [1, 0, L2 - 1]], np.int32), (4, 1, 1))
    counts = check(engine, prob, rows)
    for c in range(4):
        assert np.all(counts[c, :, c] == L2) and counts[c].sum() == 3 * L2
    # random letters on the same shape: Seq1 read from device memory at every position
    rng = np.random.default_rng(2)
    p2 = problem_of(W, rng.integers(1, 27, L1), [rng.integers(1, 27, L2), rng.integers(1, 27, 7)])
    r2 = np.array([[[1, 0, 0], [1, 0, 1], [1, 0, L2 - 1]], [[1, 0, 0], [1, L1 - 8, 6], [1, L1 - 7, 0]]], np.int32)
    check(engine, p2, r2)


def test_shift_across_the_hyphen(engine):
    L1 = 140
    seq1 = np.where(np.arange(L1) % 2 == 0, letter("A"), letter("S")).astype(np.uint8)  # A S A S ...
    lens = [1, 2, 5, 31, 32, 33, 63, SHORT_MAX, SHORT_MAX + 1, 100, 129]
    prob = problem_of(W, seq1, [np.full(l, letter("A"), np.uint8) for l in lens])
    rows = np.zeros((len(lens), 8, 3), np.int32)
    for i, L2 in enumerate(lens):
        ks = [0, 1, L2 // 2, L2 - 1]
        rows[i] = [(1, n, k) for n in (0, 1) for k in ks]
    counts = check(engine, prob, rows)
    for i, L2 in enumerate(lens):  # 'A' faces 'A' ('$') on even Seq1 positions and 'S' ('%') on odd ones
        for q, (_, n, k) in enumerate(rows[i].tolist()):
            if counts[i, q, 0] < 0:
                continue
            pos = n + np.arange(L2) + ((np.arange(L2) >= k) & (k > 0))
            assert counts[i, q].tolist() == [int((pos % 2 == 0).sum()), int((pos % 2 == 1).sum()), 0, 0], (L2, n, k)


@pytest.mark.parametrize("max_len", [SHORT_MAX, 80])
def test_batch_sizes(engine, max_len):
    """Rows around a wave's 64 lanes; with max_len 80 some records pass the threshold, so both kernels run."""
    rng = np.random.default_rng(3)
    L1 = 90
    seq1 = rng.integers(1, 27, L1)
    for n in (0, 1, 63, 64, 65, 255, 256, 257):
        prob = problem_of(W, seq1, [rng.integers(1, 27, l) for l in rng.integers(1, max_len + 1, n)])
        rows = as_triples(search_cpu(prob, Semantics.SPEC)) if n else np.zeros((0, 3), np.int32)
        counts = check(engine, prob, rows, marks=(n % 2 == 1))
        if n:
            assert np.array_equal(report_scores(counts, W), rows[:, 0].astype(np.int64))
            assert engine.stats()["records"] == n and engine.stats()["chunks"] in (1, 2)


def test_slice_of_a_larger_csr(engine):
    """offsets[0] = 13: the first wave's letter span starts off a 16-byte boundary."""
    rng = np.random.default_rng(4)
    L1 = 90
    lens = [13] + list(rng.integers(1, 81, 150))
    full = problem_of(W, rng.integers(1, 27, L1), [rng.integers(1, 27, l) for l in lens])
    sub = Problem(full.weights, full.seq1, full.codes[13:].copy(), full.offsets[1:] - 13)
    rows = as_triples(search_cpu(sub))
    want_c, want_m = search_report_cpu(sub, rows, marks=True)
    engine.set_problem(full.weights, full.seq1)
    got_c, got_m = engine.report(full.codes, full.offsets[1:], rows, marks=True)
    assert "report" in engine.stats()["kernels"]
    assert np.array_equal(got_c, want_c) and np.array_equal(got_m, want_m)
    # the device-resident form over the same slice
    codes_t, offs_t = torch.from_numpy(full.codes).to(DEV), torch.from_numpy(full.offsets[1:].copy()).to(DEV)
    counts_t, marks_t = align_report_device(engine, codes_t, offs_t, full.offsets[1:], torch.from_numpy(rows).to(DEV),
                                            marks=True)
    torch.cuda.synchronize()
    assert np.array_equal(counts_t.cpu().numpy(), want_c) and np.array_equal(marks_t.cpu().numpy(), want_m)


def test_short_and_long_interleaved(engine):
    rng = np.random.default_rng(5)
    L1 = 400
    lens = [int(rng.integers(1, SHORT_MAX + 1)) if i % 3 else int(rng.integers(SHORT_MAX + 1, 300)) for i in range(200)]
    prob = problem_of(W, rng.integers(1, 27, L1), [rng.integers(1, 27, l) for l in lens])
    check(engine, prob, as_triples(search_cpu(prob)))
    assert engine.stats()["chunks"] == 2  # one launch per regime
    check(engine, prob, search_topk_cpu(prob, 3))


@pytest.mark.parametrize("side_stream", [False, True])
@pytest.mark.parametrize("marks", [False, True])
@pytest.mark.parametrize("K", [1, 2, 3, 64])
def test_rows_from_topk_on_the_same_stream(engine, K, marks, side_stream):
    rng = np.random.default_rng(6)
    L1 = 70
    seq1 = rng.integers(1, 27, L1)
    lens = [70, 69, 68, 1, 2, 64, 65] + list(rng.integers(1, 70, 90))  # 1..3 candidates first: padding rows
    prob = problem_of(W, seq1, [rng.integers(1, 27, l) for l in lens])
    want_rows = search_topk_cpu(prob, K)
    want_c, want_m = search_report_cpu(prob, want_rows, marks=True)
    assert (want_rows[..., 0] == INT32_MIN).any() == (K > 1)  # padding rows whenever K passes a record's candidates
    engine.set_problem(prob.weights, prob.seq1)
    codes_t, offs_t = torch.from_numpy(prob.codes).to(DEV), torch.from_numpy(prob.offsets).to(DEV)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(DEV) if side_stream else torch.cuda.current_stream(DEV)
    with torch.cuda.stream(stream):
        rows_t = align_topk_device(engine, codes_t, offs_t, prob.offsets, K)  # no sync before the report
        got = align_report_device(engine, codes_t, offs_t, prob.offsets, rows_t, marks=marks)
    assert "report" in engine.stats()["kernels"]
    torch.cuda.synchronize()  # the default stream stands for the engine's own compute stream
    counts_t, marks_t = got if marks else (got, None)
    assert np.array_equal(rows_t.cpu().numpy(), want_rows)
    assert np.array_equal(counts_t.cpu().numpy(), want_c)
    if marks:
        assert np.array_equal(marks_t.cpu().numpy(), want_m)
    real = want_rows[..., 0] != INT32_MIN
    assert np.array_equal(report_scores(counts_t.cpu().numpy(), W)[real], want_rows[..., 0].astype(np.int64)[real])


def test_rows_from_solve_device(engine):
    rng = np.random.default_rng(7)
    prob = problem_of(W, rng.integers(1, 27, 120), [rng.integers(1, 27, l) for l in rng.integers(1, 100, 300)])
    engine.set_problem(prob.weights, prob.seq1)
    codes_t, offs_t = torch.from_numpy(prob.codes).to(DEV), torch.from_numpy(prob.offsets).to(DEV)
    rows_t = align_search_device(engine, codes_t, offs_t, prob.offsets)
    counts_t = align_report_device(engine, codes_t, offs_t, prob.offsets, rows_t)
    torch.cuda.synchronize()
    rows = rows_t.cpu().numpy()
    assert counts_t.shape == (prob.n, 4)
    assert np.array_equal(counts_t.cpu().numpy(), search_report_cpu(prob, rows))
    assert np.array_equal(report_scores(counts_t.cpu().numpy(), W), rows[:, 0].astype(np.int64))


def test_rows_out_of_range_by_one(engine):
    """Only rows one past the upper end: a faulty bounds check would read Seq1's zero padding or the record itself
    and fail the comparison. (Hostile values stay in the CPU tests and the sanitizer program.)"""
    rng = np.random.default_rng(8)
    L1 = 100
    lens = [5, 50, SHORT_MAX, SHORT_MAX + 1, 1, 99, 100]
    prob = problem_of(W, rng.integers(1, 27, L1), [rng.integers(1, 27, l) for l in lens])
    rows = np.zeros((len(lens), 5, 3), np.int32)
    for i, L2 in enumerate(lens):
        rows[i] = [(1, 0, 0), (1, L1 - L2 + 1, 0), (1, L1 - L2, 1), (1, 0, L2), (1, L1 - L2, 0)]
    counts = check(engine, prob, rows)
    assert np.all(counts[:, 1:4] == -1)
    assert np.array_equal(counts[:, [0, 4]].sum(-1), np.tile(np.array(lens)[:, None], (1, 2)))
    for q in range(5):
        check(engine, prob, np.ascontiguousarray(rows[:, q]))


@pytest.mark.parametrize("i", range(1, 7))
def test_goldens(engine, i):
    prob = Problem.read(input_path(i))
    engine.set_problem(prob.weights, prob.seq1)
    rows = as_triples(engine.solve(prob.codes, prob.offsets))
    counts, marks = engine.report(prob.codes, prob.offsets, rows, marks=True)
    assert "report" in engine.stats()["kernels"]
    golden = [int(l.split("score: ")[1].split(",")[0]) for l in expected(i).splitlines()]
    assert report_scores(counts, prob.weights).tolist() == golden
    want_c, want_m = search_report_cpu(prob, rows, marks=True)
    assert format_report(prob, rows, counts, marks) == format_report(prob, rows, want_c, want_m)
    assert np.array_equal(counts, want_c) and np.array_equal(marks, want_m)
