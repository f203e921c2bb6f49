"""GPU (MI355X / gfx950) tests of the wire-format decode (csrc/src/hip/wire_kernels.hip) and of profile, top-K, hits
and report on wire batches. The decode kernels byte for byte against decode_wire_cpu (tests/test_wire_decode_cpu.py
anchors that one to WireSlice's numpy decoders) between poisoned guards, at the smallest shapes that reach each
path: every letter form x length form x sparse shift x record count around the 24-record words and 64-record waves,
1537 records (several blocks, a partial last wave), batches that start inside a stream, 1 to 57 letters, extreme P33
digits, 3-bit lengths ending on and past a byte boundary, pageable and page-locked sources. The four host forms on
three batches against the CPU engine and against the byte-letter engine calls on the decoded batch, under both
semantics; chunks, the hits second pass, stats, and the device-resident form on a side stream."""
import numpy as np
import pytest

from conftest import gpu_available, input_path
from wire_cases import COUNTS, FORMS, LETTERS, SHIFTS, make_case, page_alloc, sub_batch

pytestmark = pytest.mark.gpu

if not gpu_available():  # pragma: no cover - collected on CPU hosts only with -m gpu
    pytest.skip("no GPU", allow_module_level=True)

import torch  # noqa: E402

from mpi_openmp_cuda_amd import (HipSearchEngine, Problem, Semantics, WireSlice, _lib, decode_wire_cpu,  # noqa: E402
                                 search_hits_cpu, search_profile_cpu, search_report_cpu, search_topk_cpu)
from mpi_openmp_cuda_amd.ops.align import wire_batch_of  # noqa: E402
from mpi_openmp_cuda_amd.parallel.wire import private_alloc  # noqa: E402

SEMS = [Semantics.REFERENCE, Semantics.SPEC]
DEV = torch.device("cuda:0")
I32 = np.iinfo(np.int32)
POISON8, POISON64 = 0xA5, -0x5A5A5A5A5A5A5A5B
GUARD8, GUARD64 = 64, 8

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


# ---- the decode kernels ------------------------------------------------------------------------------------
def check_decode(eng, batch, shift=0, host_meta=None, ref=None, skew=0, what=None):
    """Decodes ``batch`` on the GPU between poisoned guards (the letters ``skew`` bytes off a 64-byte boundary) and
    compares letters, device offsets, host offsets and both guards with decode_wire_cpu."""
    codes_ref, offs_ref = ref if ref is not None else decode_wire_cpu(batch, shift)
    L, n = codes_ref.shape[0], offs_ref.shape[0] - 1
    buf_c = torch.full((GUARD8 + skew + L + GUARD8,), POISON8, dtype=torch.uint8, device=DEV)
    buf_o = torch.full((GUARD64 + n + 1 + GUARD64,), POISON64, dtype=torch.int64, device=DEV)
    lo = GUARD8 + skew
    dense = eng.decode_wire_into(batch, buf_c[lo:lo + L], buf_o[GUARD64:GUARD64 + n + 1], host_meta=host_meta,
                                 shift=shift)
    torch.cuda.synchronize()
    c, o = buf_c.cpu().numpy(), buf_o.cpu().numpy()
    assert np.array_equal(dense, offs_ref), what
    assert np.array_equal(o[GUARD64:GUARD64 + n + 1], offs_ref), what
    assert np.array_equal(c[lo:lo + L], codes_ref), what
    assert (c[:lo] == POISON8).all() and (c[lo + L:] == POISON8).all(), what
    assert (o[:GUARD64] == POISON64).all() and (o[GUARD64 + n + 1:] == POISON64).all(), what


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("letters", LETTERS)
def test_decode_matrix(engine, letters, form):
    """Pageable sources (copied to the device in packed form), every count and shift; the output's alignment varies."""
    for n in COUNTS:
        ws = make_case(letters, form, n, seed=n)
        for shift in SHIFTS:
            if shift and form == "none":
                continue
            check_decode(engine, ws, shift, skew=(n + shift) % 4, what=(n, shift))


@pytest.mark.parametrize("letters", LETTERS)
def test_decode_page_locked_sources(engine, letters):
    """The kernels read page-locked host arrays in place: the same bytes, and nothing is copied first."""
    for form, n, shift in (("base6", 65, 6), ("3", 129, 3), ("4", 25, 1), ("8", 64, 6), ("none", 23, 0)):
        ws = make_case(letters, form, n, seed=n + 7, alloc=page_alloc)
        engine.pin(*ws.arrays(), ws.wire_offsets(shift))
        check_decode(engine, ws, shift, skew=1, what=(form, n, shift))


@pytest.mark.parametrize("letters", LETTERS)
def test_decode_1537_records(engine, letters):
    """Several blocks of the offsets kernel with a one-record last wave; several blocks of the letter kernel."""
    for form, shift in (("base6", 6), ("3", 0), ("4", 3), ("8", 1), ("none", 0)):
        check_decode(engine, make_case(letters, form, 1537, seed=11), shift, skew=3, what=(form, shift))


@pytest.mark.parametrize("letters", LETTERS)
def test_decode_inside_a_stream_and_few_letters(engine, letters):
    """Batches of 1, 6, 7, 8, 55, 56, 57 letters at the stream's start and 7, 8 and 13 letters into it (c0 % 7 in
    {0, 1, 6}, c0 % 56 != 0): partial first and last P33 fields, sources that end at the batch's last byte."""
    rng = np.random.default_rng(2)
    for total in (1, 6, 7, 8, 55, 56, 57):
        for head in ((), (7,), (7, 1), (7, 1, 5)):
            lengths = np.array(head + (total, 9), np.int64)
            parent = WireSlice(lengths, rng.integers(1, 27, int(lengths.sum())).astype(np.uint8), letters)
            a = len(head)
            c0 = int(parent.offsets[a])
            assert c0 in (0, 7, 8, 13)
            for shift in (0, 6):
                batch, keep, sub = sub_batch(parent, a, a + 1, shift)
                ref = decode_wire_cpu(batch)
                assert ref[0].shape[0] == total and int(ref[1][0]) == c0
                check_decode(engine, batch, ref=ref, skew=total % 4, what=(total, c0, shift))
    # several records from inside a longer stream, pageable and page-locked
    lengths = np.array([7, 1, 5, 8, 6, 9, 7, 6, 10, 5, 6, 11, 7] + [6] * 300, np.int64)
    stream = rng.integers(1, 27, int(lengths.sum())).astype(np.uint8)
    for pinned in (False, True):
        alloc = page_alloc if pinned else private_alloc
        parent = WireSlice(lengths, stream, letters, alloc=alloc)
        for a, b in ((1, 4), (2, 313), (3, 200)):
            batch, keep, sub = sub_batch(parent, a, b, 3, alloc=alloc)
            if pinned:
                engine.pin(*keep[0].arrays(), keep[1], *keep[2].arrays())
            check_decode(engine, batch, skew=2, what=(a, b, pinned))


def test_decode_p33_extreme_digits(engine):
    """P33 fields with all digits 0, all 25, and each single digit 25 with the others 0."""
    fields = [[1] * 7, [26] * 7] + [[26 if j == i else 1 for j in range(7)] for i in range(7)]
    letters = np.array(fields, np.uint8).reshape(-1)
    for lengths in ([63], [7] * 9, [1] * 63):
        ws = WireSlice(np.array(lengths, np.int64), letters, "p33")
        assert np.array_equal(decode_wire_cpu(ws)[0], letters)
        check_decode(engine, ws, 0, ref=(letters, ws.offsets.copy()))
        check_decode(engine, ws, 1, ref=(letters, ws.offsets.copy()), skew=1)


def test_decode_3bit_lengths_at_a_byte_boundary(engine):
    """3-bit lengths whose last field ends exactly at a byte boundary (3 n % 8 == 0) and one record past it."""
    for n in (8, 9, 16, 17, 72, 73):
        for shift in (0, 3, 6):
            check_decode(engine, make_case("p33", "3", n, seed=n), shift, what=(n, shift))


# ---- the four host forms on three batches --------------------------------------------------------------------
W = (10, 2, 3, 4)


def _batches():
    rng = np.random.default_rng(42)
    out = {}
    # 1: input6-shaped, P33 + base 6 + sparse offsets of 64 records
    lengths = rng.integers(5, 11, 1000).astype(np.int64)
    seq1 = rng.integers(1, 27, 26).astype(np.uint8)
    ws = WireSlice(lengths, rng.integers(1, 27, int(lengths.sum())).astype(np.uint8), "p33")
    assert ws.len_bits == 6
    out["input6"] = (list(W), seq1, ws, 6)
    # 2: input3 (records of 56..1152 letters: no narrow form, dense offsets), P33 and 5-bit letters
    p3 = Problem.read(input_path(3))
    for fmt in ("p33", "p5"):
        ws = WireSlice.from_csr(p3.codes, p3.offsets, letter_format=fmt)
        assert ws.lengths is None
        out["input3-" + fmt] = (p3.weights, p3.seq1, ws, 0)
    # 3: mixed, with records longer than Seq1 and as long as it; 8-bit lengths, sparse offsets of 8 records
    lengths = np.array([10, 41, 40, 7, 12, 40, 55, 5, 33, 1, 39, 26, 40, 9] + list(rng.integers(1, 41, 51)), np.int64)
    ws = WireSlice(lengths, rng.integers(1, 27, int(lengths.sum())).astype(np.uint8), "p33")
    assert ws.len_bits == 8
    out["mixed"] = (list(W), rng.integers(1, 27, 40).astype(np.uint8), ws, 3)
    return out


_cache = {}


def batch(name):
    if "batches" not in _cache:
        _cache["batches"] = _batches()
    return _cache["batches"][name]


def decoded(name) -> Problem:
    """The batch as the CPU engine takes it: the problem over decode_wire_cpu's bytes and offsets."""
    k = ("decoded", name)
    if k not in _cache:
        weights, seq1, ws, shift = batch(name)
        codes, offsets = decode_wire_cpu(ws, shift)
        _cache[k] = Problem(weights, seq1, codes, offsets)
    return _cache[k]


def oracle(name, sem, what, *args):
    """The CPU engine's answer on the decoded batch: computed once, read-only."""
    k = (name, sem, what) + args
    if k not in _cache:
        prob = decoded(name)
        if what == "profile":
            _cache[k] = search_profile_cpu(prob, sem)
        elif what == "topk":
            _cache[k] = search_topk_cpu(prob, args[0], sem)
        elif what == "thresholds":  # each record's best score minus 3 (0 for a record without candidates)
            best = search_topk_cpu(prob, 1, sem)[:, 0, 0].astype(np.int64)
            _cache[k] = np.where(best == I32.min, 0, best - 3).astype(np.int32)
    return _cache[k]


NAMES = ("input6", "input3-p33", "input3-p5", "mixed")


def setup(engine, name, sem):
    weights, seq1, ws, shift = batch(name)
    engine.set_problem(weights, seq1, sem)
    return ws, shift, decoded(name)


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("name", NAMES)
def test_profile_wire(engine, name, sem):
    ws, shift, prob = setup(engine, name, sem)
    prof, po = ws.solve_profile_wire(engine, shift)
    want, want_po = oracle(name, sem, "profile")
    assert np.array_equal(po, want_po)
    assert np.array_equal(prof, want)
    assert "wire" in engine.stats()["kernels"] and "profile" in engine.stats()["kernels"]
    got, got_po = engine.solve_profile(prob.codes, prob.offsets)
    assert np.array_equal(prof, got) and np.array_equal(po, got_po)


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("name", NAMES)
def test_topk_wire(engine, name, sem):
    ws, shift, prob = setup(engine, name, sem)
    for K in (1, 3, 64):
        rows = ws.solve_topk_wire(engine, K, shift)
        assert np.array_equal(rows, oracle(name, sem, "topk", K)), K
        st = engine.stats()
        assert "wire" in st["kernels"] and st["records"] == ws.n
        assert np.array_equal(rows, engine.solve_topk(prob.codes, prob.offsets, K)), K


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("name", NAMES)
def test_hits_wire(engine, name, sem):
    ws, shift, prob = setup(engine, name, sem)
    thr = oracle(name, sem, "thresholds")
    for kw in (dict(min_score=int(I32.min)), dict(thresholds=thr), dict(within=0)):
        rows, h = ws.solve_hits_wire(engine, shift=shift, **kw)
        st = engine.stats()
        want_rows, want_h = search_hits_cpu(prob, semantics=sem, **kw)
        assert np.array_equal(h, want_h), kw
        assert np.array_equal(rows, want_rows), kw
        assert "wire" in st["kernels"] and "hits" in st["kernels"]
        got_rows, got_h = engine.solve_hits(prob.codes, prob.offsets, **kw)
        assert np.array_equal(h, got_h) and np.array_equal(rows, got_rows), kw


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("name", NAMES)
def test_report_wire(engine, name, sem):
    ws, shift, prob = setup(engine, name, sem)
    for K in (1, 3):
        rows = oracle(name, sem, "topk", K)
        counts, marks = ws.report_wire(engine, rows, marks=True, shift=shift)
        st = engine.stats()
        want_counts, want_marks = search_report_cpu(prob, rows, marks=True)
        assert np.array_equal(counts, want_counts), K
        assert np.array_equal(marks, want_marks), K
        assert "wire" in st["kernels"] and "report" in st["kernels"]
        got_counts, got_marks = engine.report(prob.codes, prob.offsets, rows, marks=True)
        assert np.array_equal(counts, got_counts) and np.array_equal(marks, got_marks), K
    flat = oracle(name, sem, "topk", 1)[:, 0]
    assert np.array_equal(ws.report_wire(engine, flat, shift=shift), search_report_cpu(prob, flat))


# ---- remaining checks ----------------------------------------------------------------------------------------
def _all_forms(engine, ws, shift, rows3, thr):
    prof, po = engine.solve_profile_wire(ws, shift)
    top = engine.solve_topk_wire(ws, 3, shift)
    hits, h = engine.solve_hits_wire(ws, thresholds=thr, shift=shift)
    counts, marks = engine.report_wire(ws, rows3, marks=True, shift=shift)
    return prof, po, top, hits, h, counts, marks


@pytest.mark.parametrize("name", ("input6", "input3-p5", "mixed"))
def test_page_locked_equals_pageable(engine, name):
    """The same slice decoded from pageable arrays (packed H2D copies) and from arrays pinned through eng.pin
    (read in place): identical results, and the packed bytes are all that is reported as uploaded."""
    sem = Semantics.REFERENCE
    ws, shift, prob = setup(engine, name, sem)
    rows3, thr = oracle(name, sem, "topk", 3), oracle(name, sem, "thresholds")
    _, _, ws0, _ = batch(name)
    fresh = WireSlice.from_csr(prob.codes, prob.offsets, letter_format=ws0.letter_format)  # never pinned
    assert fresh.len_bits == ws0.len_bits
    pageable = _all_forms(engine, fresh, shift, rows3, thr)
    engine.solve_topk_wire(fresh, 1, shift)
    h2d = engine.stats()["h2d_bytes"]
    pinned = WireSlice.from_csr(prob.codes, prob.offsets, letter_format=ws0.letter_format, alloc=page_alloc)
    engine.pin(*pinned.arrays(), pinned.wire_offsets(shift))
    locked = _all_forms(engine, pinned, shift, rows3, thr)
    for a, b in zip(pageable, locked):
        assert np.array_equal(a, b)
    engine.solve_topk_wire(pinned, 1, shift)
    st = engine.stats()
    assert "wire" in st["kernels"] and st["h2d_bytes"] == h2d
    if name == "input6":  # P33 + base 6 + one offset per 64 records: far below 1 + 8 bytes per letter and record
        packed = (33 * ((ws.total + 6) // 7) + 7) // 8 + 8 * ((ws.n + 23) // 24) + 8 * (((ws.n + 63) >> 6) + 1)
        assert h2d == packed < ws.total + 8 * (ws.n + 1)


def test_chunks_under_a_small_scratch(engine):
    """A profile scratch small enough for at least 3 chunks gives the same top-K and hits."""
    sem = Semantics.SPEC
    ws, shift, prob = setup(engine, "input6", sem)
    po = oracle("input6", sem, "profile")[1]
    try:
        engine.set_profile_scratch(int(po[-1]) * 8 // 3 - 64)
        rows = ws.solve_topk_wire(engine, 3, shift)
        assert engine.stats()["chunks"] >= 3
        assert np.array_equal(rows, oracle("input6", sem, "topk", 3))
        thr = oracle("input6", sem, "thresholds")
        hits, h = ws.solve_hits_wire(engine, thresholds=thr, shift=shift)
        assert engine.stats()["chunks"] >= 3
        want, want_h = search_hits_cpu(prob, thresholds=thr, semantics=sem)
        assert np.array_equal(h, want_h) and np.array_equal(hits, want)
    finally:
        engine.set_profile_scratch(256 << 20)


def test_hits_second_pass(engine):
    sem = Semantics.REFERENCE
    ws, shift, prob = setup(engine, "mixed", sem)
    rows, h = ws.solve_hits_wire(engine, min_score=int(I32.min), max_rows=1, shift=shift)
    assert engine.hits_passes() == 2
    want, want_h = search_hits_cpu(prob, min_score=int(I32.min), semantics=sem)
    assert np.array_equal(h, want_h) and np.array_equal(rows, want)
    rows, h = ws.solve_hits_wire(engine, min_score=int(I32.min), max_rows=int(want_h[-1]), shift=shift)
    assert engine.hits_passes() == 1 and np.array_equal(rows, want)


def test_empty_batch(engine):
    engine.set_problem(list(W), np.arange(1, 27, dtype=np.uint8), Semantics.REFERENCE)
    ws = WireSlice(np.zeros(0, np.int64), np.zeros(0, np.uint8), "p33")
    assert ws.solve_topk_wire(engine, 2).shape == (0, 2, 3)
    rows, h = ws.solve_hits_wire(engine, min_score=0)
    assert rows.shape == (0, 3) and h.tolist() == [0]
    prof, po = ws.solve_profile_wire(engine)
    assert prof.shape == (0,) and po.tolist() == [0]
    check_decode(engine, ws, 0)


@pytest.mark.parametrize("name", ("input6", "mixed", "input3-p5"))
def test_device_resident_form(engine, name):
    """Torch tensors of the wire arrays: decode_wire_device, solve_topk_device and report_device queued on one
    non-default stream with no sync in between; the results equal the host forms'."""
    sem = Semantics.SPEC
    ws, shift, prob = setup(engine, name, sem)
    K = 3
    want_rows = ws.solve_topk_wire(engine, K, shift)
    want_counts, want_marks = ws.report_wire(engine, want_rows, marks=True, shift=shift)
    h_offsets = ws.wire_offsets(shift)
    letters_t = torch.from_numpy(np.ascontiguousarray(ws.codes)).to(DEV)
    offsets_t = torch.from_numpy(np.ascontiguousarray(h_offsets)).to(DEV)
    lengths_t = None if ws.lengths is None else torch.from_numpy(np.ascontiguousarray(ws.lengths)).to(DEV)
    rows_t = torch.empty((ws.n, K, 3), dtype=torch.int32, device=DEV)
    counts_t = torch.empty((ws.n, K, 4), dtype=torch.int32, device=DEV)
    marks_t = torch.zeros(K * ws.total, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    codes_t, dense_t, dense = engine.decode_wire_device(letters_t, offsets_t, lengths_t, ws.n, h_offsets, ws.lengths,
                                                        lengths_bits=ws.len_bits or 8, lengths_base=ws.len_base,
                                                        letters=ws.letter_format, off_shift=shift, stream=stream)
    engine.solve_topk_device(codes_t, dense_t, dense, K, rows_t, stream=stream)
    engine.report_device(codes_t, dense_t, dense, rows_t, counts_t, marks_t, stream=stream)
    stream.synchronize()
    assert np.array_equal(dense, prob.offsets)
    assert np.array_equal(dense_t.cpu().numpy(), prob.offsets)
    assert np.array_equal(codes_t.cpu().numpy()[:ws.total], prob.codes)
    assert np.array_equal(rows_t.cpu().numpy(), want_rows)
    assert np.array_equal(counts_t.cpu().numpy(), want_counts)
    assert np.array_equal(marks_t.cpu().numpy(), want_marks)
    # the same device arrays between guards (device sources: nothing is copied from the host)
    b = _lib.WireBatch(letters=letters_t.data_ptr(), offsets=offsets_t.data_ptr(),
                       lengths=None if lengths_t is None else lengths_t.data_ptr(), n=ws.n, len_base=int(ws.len_base),
                       packed={"bytes": 0, "p5": 1, "p33": 3}[ws.letter_format], off_shift=shift,
                       len_bits=int(ws.len_bits or 8), device=1)
    meta, keep = wire_batch_of(ws, shift)
    check_decode(engine, b, host_meta=meta, ref=(prob.codes, prob.offsets), skew=1)
