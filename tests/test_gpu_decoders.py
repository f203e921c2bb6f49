"""GPU (MI355X / gfx950) tests of the wire decoders: the seven pieces of device arithmetic that turn P33 letter fields
and base-6 / 3 / 4 / 8-bit lengths back into letters and lengths, on the inputs where such arithmetic can be wrong —
every P33 field on a digit carry and at every bit phase, all 6^8 base-6 octets, every narrow length field at every
index residue (tests/decoder_cases.py) — and not on random data, which meets a quotient boundary once in thousands
of fields. Results are exact and compared row for row: against closed forms that read every decoded letter and length
back (tests/test_decoder_cases.py proves them against the CPU engine for every record), against the source letters
and numpy's cumsum, or against the CPU engine. Every case asserts through stats() which path ran.

  P33, streaming swipe kernel ((x >> 1) / 13, / 26 chains):
      test_streaming_kernel_reads_every_letter, test_letter_records
  P33, lane-direct kernel (decode_p33_field_lut):
      test_lane_direct_kernel_reads_every_letter, test_letter_records
  P33, unpack33_kernel (p33_letters):
      test_unpack33_kernel_reads_every_letter, test_unpack33_kernel_sub_batches, test_letter_records
  base 6, record_lengths4 and record_length:
      test_streaming_kernel_every_octet, test_streaming_kernel_octet_tails, test_short_kernel_half_end_octets
  base 6, lane_length6:
      test_lane_direct_kernel_every_octet
  base 6 / 3 / 4 / 8-bit, wire_length (wire_offsets_kernel):
      test_wire_offsets_kernel_every_octet, test_narrow_lengths_wire_offsets_kernel
  3 / 4 / 8-bit, record_lengths4 and record_length:
      test_narrow_lengths_streaming_kernel, test_narrow_lengths_device_resident, test_narrow_lengths_short_kernel
"""
import mmap

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = pytest.mark.gpu

if not gpu_available():  # pragma: no cover - collected on CPU hosts only with -m gpu
    pytest.skip("no GPU", allow_module_level=True)

import torch  # noqa: E402

import decoder_cases as dc  # noqa: E402
from wire_cases import forced_slice, sub_batch  # noqa: E402
from mpi_openmp_cuda_amd import HipSearchEngine, Semantics, _lib, search_cpu, search_topk_cpu  # noqa: E402
from mpi_openmp_cuda_amd.ops.align import as_triples  # noqa: E402
from mpi_openmp_cuda_amd.parallel.wire import WireSlice, private_alloc  # noqa: E402
from mpi_openmp_cuda_amd.utils.synthetic import differing  # noqa: E402

SEMS = [Semantics.REFERENCE, Semantics.SPEC]
DEV = torch.device("cuda:0")
POISON = 0x77
POISON8, POISON64 = 0xA5, -0x5A5A5A5A5A5A5A5B
GUARD8, GUARD64 = 64, 8


@pytest.fixture(scope="module")
def engine():
    e = HipSearchEngine(device=0)
    yield e
    e.close()


# ---- helpers ---------------------------------------------------------------------------------------------
def own_pages(name: str, dtype, count: int) -> np.ndarray:
    """A WireSlice allocator for slices that a test page-locks: each array in anonymous pages of its own (page-locking
    covers whole pages: no heap page is shared with another object), unmapped when the array dies."""
    nbytes = max(int(count) * np.dtype(dtype).itemsize, 1)
    return np.frombuffer(mmap.mmap(-1, (nbytes + 4095) & ~4095), dtype=dtype, count=int(count))


def assert_rows(got, want, what):
    msg = differing(got, want, want[:, 1])
    assert not msg, f"{what}: {msg}"


def check_decode(eng, batch, shift, codes_ref, offs_ref, skew=0, what=None):
    """Decodes ``batch`` into tensors between poisoned guards (the letters ``skew`` bytes off a 64-byte boundary):
    letters, device offsets, the returned host offsets and all four guards."""
    L, n = codes_ref.shape[0], offs_ref.shape[0] - 1
    buf_c = torch.full((GUARD8 + skew + L + GUARD8,), POISON8, dtype=torch.uint8, device=DEV)
    buf_o = torch.full((GUARD64 + n + 1 + GUARD64,), POISON64, dtype=torch.int64, device=DEV)
    lo = GUARD8 + skew
    dense = eng.decode_wire_into(batch, buf_c[lo:lo + L], buf_o[GUARD64:GUARD64 + n + 1], shift=shift)
    torch.cuda.synchronize()
    c, o = buf_c.cpu().numpy(), buf_o.cpu().numpy()
    assert np.array_equal(dense, offs_ref), what
    assert np.array_equal(o[GUARD64:GUARD64 + n + 1], offs_ref), what
    assert np.array_equal(c[lo:lo + L], codes_ref), what
    assert (c[:lo] == POISON8).all() and (c[lo + L:] == POISON8).all(), what
    assert (o[:GUARD64] == POISON64).all() and (o[GUARD64 + n + 1:] == POISON64).all(), what


def topk1_wire(eng, ws, shift, what):
    """The best row per record from the profile family on the wire batch: the decode kernels ran ("wire")."""
    rows = ws.solve_topk_wire(eng, 1, shift)[:, 0]
    st = eng.stats()
    assert "wire" in st["kernels"] and "profile" in st["kernels"] and st["records"] == ws.n, (what, st)
    return rows


def solve_pinned(eng, ws, kernel, what, form=None):
    """The slice page-locked and streamed zero-copy (direct == 1) through ``kernel``, results poisoned first."""
    ws.alloc_results(eng)
    with _lib.Pinned(*ws.arrays()):
        ws.results.view(np.uint8)[:] = POISON
        ws.solve(eng)
        st = eng.stats()
        rows = ws.triples(eng)
    assert st["kernels"] == [kernel] and st["direct"] == 1 and st["records"] == ws.n, (what, st)
    assert st["h2d_bytes"] > 0 and (form is None or form in st["forms"]), (what, st)
    return rows


def solve_device(eng, ws, sparse, what, kernel="swipe"):
    """The slice's arrays as device tensors through solve_wire_device: nothing is copied from the host."""
    res = ws.alloc_results(eng)
    letters = torch.from_numpy(ws.codes).to(DEV)
    offsets = torch.from_numpy(ws.sparse_offsets(6) if sparse else np.asarray(ws.offsets)).to(DEV)
    lengths = torch.from_numpy(ws.lengths).to(DEV) if ws.lengths is not None else None
    out = torch.full((max(res.nbytes, 1),), POISON, dtype=torch.uint8, device=DEV)
    eng.solve_wire_device(letters, offsets, lengths, ws.n, out, ws.fmt, (ws.l2_min, ws.l2_max),
                          lengths_bits=ws.len_bits or 8, lengths_base=ws.len_base,
                          packed33=ws.letter_format == "p33", off_shift=6 if sparse else 0)
    st = eng.stats()
    assert st["kernels"] == [kernel] and st["direct"] == 1 and st["records"] == ws.n, (what, st)
    assert st["h2d_bytes"] == 0, (what, st)
    res.view(np.uint8)[:] = out.cpu().numpy()[:res.nbytes]
    return ws.triples(eng)


def solve_staged(eng, ws, what):
    """The slice from pageable memory through the staged pipeline (direct == 0)."""
    ws.alloc_results(eng)
    ws.results.view(np.uint8)[:] = POISON
    ws.solve(eng)
    st = eng.stats()
    assert st["kernels"] == ["swipe"] and st["direct"] == 0 and st["records"] == ws.n, (what, st)
    return ws.triples(eng)


_refs = {}


def cpu_rows(key, prob, sem):
    """The CPU engine's rows of a shared problem: computed once, read-only."""
    if (key, sem) not in _refs:
        _refs[(key, sem)] = as_triples(search_cpu(prob, sem))
    return _refs[(key, sem)]


# ---- letters: every P33 field on a digit carry and at every bit phase, as one-letter records ----------------
@pytest.mark.parametrize("stream", dc.STREAMS)
def test_unpack33_kernel_reads_every_letter(engine, stream):
    """unpack33_kernel's p33_letters (umulhi by 2463805336 >> 14, umulhi by 6353502, (v * 2521) >> 16): the stream
    decoded through decode_wire_into between poisoned guards, dense offsets and 64-record sparse ones, from a pageable
    source (copied in packed form) and from a page-locked one (read in place); then as the profile family's input
    (solve_topk_wire: stats() names "wire" and "profile"), where the best row of record i is (1, letter i - 1, 0)."""
    prob, want = dc.readout(stream)
    ws = WireSlice.from_csr(prob.codes, prob.offsets)
    assert ws.letter_format == "p33" and ws.len_bits == 6
    for shift in (0, 6):
        check_decode(engine, ws, shift, prob.codes, prob.offsets, skew=shift % 4 + 1, what=(stream, shift, "pageable"))
    ws = WireSlice.from_csr(prob.codes, prob.offsets, alloc=own_pages)
    with _lib.Pinned(*ws.arrays(), ws.wire_offsets(6)):
        for shift in (0, 6):
            check_decode(engine, ws, shift, prob.codes, prob.offsets, skew=3, what=(stream, shift, "page-locked"))
        engine.set_problem(prob.weights, prob.seq1, Semantics.SPEC)
        assert_rows(topk1_wire(engine, ws, 6, stream), want, f"{stream} page-locked top-1")
    for sem in SEMS:
        engine.set_problem(prob.weights, prob.seq1, sem)
        assert_rows(topk1_wire(engine, ws, 6, stream), want, f"{stream} {sem.name} top-1")


@pytest.mark.parametrize("stream", dc.STREAMS)
def test_unpack33_kernel_sub_batches(engine, stream):
    """unpack33_kernel on batches that start 1 and 6 letters into the stream (a partial first field, every later field
    at the same bit phase but another lane and block), dense and sparse offsets: the letters from there on."""
    prob, _ = dc.readout(stream)
    parent = WireSlice.from_csr(prob.codes, prob.offsets)
    for a in dc.SUB_STARTS:
        for shift in (0, 6):
            batch, keep, sub = sub_batch(parent, a, parent.n, shift)
            assert int(parent.offsets[a]) == a and sub.n == parent.n - a
            check_decode(engine, batch, 0, prob.codes[a:], prob.offsets[a:], skew=a % 4, what=(stream, a, shift))
            del keep
    # the profile family ran on none of these: the decode kernels alone are under test, between guards


@pytest.mark.parametrize("stream", dc.STREAMS)
def test_streaming_kernel_reads_every_letter(engine, stream):
    """The streaming swipe kernel's P33 loop ((x >> 1) / 13u, then / 26u chains, swipe_impl.hpp): the one-letter
    records as a page-locked WireSlice(..., "p33"), ws.solve: direct == 1, kernels == ["swipe"], the k-bits form."""
    prob, want = dc.readout(stream)
    for sem in SEMS:
        engine.set_problem(prob.weights, prob.seq1, sem)
        ws = WireSlice.from_csr(prob.codes, prob.offsets, letter_format="p33", alloc=own_pages)
        assert_rows(solve_pinned(engine, ws, "swipe", (stream, sem), form="swipe_kbits"), want,
                    f"{stream} {sem.name} pinned p33")


@pytest.mark.parametrize("stream", dc.STREAMS)
def test_lane_direct_kernel_reads_every_letter(engine, stream):
    """The lane-direct swipe kernel's decode_p33_field_lut (umulhi by 2463805336 >> 14, v_mul_hi_u32_u24 by 6353502,
    v_mad_i32_i24, the LDS pair table): device copies of the wire arrays through solve_wire_device, dense offsets and
    64-record sparse ones: direct == 1, kernels == ["swipe"], h2d_bytes == 0. (Records of one word: the lane-direct
    kernel takes device-resident P33 batches of at most 16 record words.)"""
    prob, want = dc.readout(stream)
    for sem in SEMS:
        engine.set_problem(prob.weights, prob.seq1, sem)
        for sparse in (True, False):
            ws = WireSlice.from_csr(prob.codes, prob.offsets, letter_format="p33")
            assert_rows(solve_device(engine, ws, sparse, (stream, sem, sparse)), want,
                        f"{stream} {sem.name} device p33 {'sparse' if sparse else 'dense'}")


@pytest.mark.parametrize("stream", dc.STREAMS)
def test_p5_letters_staged_read_every_letter(engine, stream):
    """5-bit letters have no arithmetic, but unpack5_kernel's eight bit phases see every letter: the same records with
    letter_format="p5" through the staged pipeline: direct == 0, kernels == ["swipe"]."""
    prob, want = dc.readout(stream)
    engine.set_problem(prob.weights, prob.seq1, Semantics.REFERENCE)
    ws = WireSlice.from_csr(prob.codes, prob.offsets, letter_format="p5")
    assert_rows(solve_staged(engine, ws, stream), want, f"{stream} staged p5")


@pytest.mark.parametrize("cut", dc.RECORD_CUTS)
def test_letter_records(engine, cut):
    """A shape whose rows depend on every letter of a record: the boundary stream as 7-letter records (one field each)
    and as records of 1..6 letters cycling (records across field borders), random Seq1 of 40, weights (10, 2, 3, 4),
    against the CPU engine through the streaming kernel's P33 loop (pinned: direct == 1) and the lane-direct kernel's
    decode_p33_field_lut (device-resident, sparse offsets: h2d_bytes == 0), and through unpack33_kernel (top-1)."""
    prob = dc.letter_records(cut)
    for sem in SEMS:
        want = cpu_rows(("records", cut), prob, sem)
        engine.set_problem(prob.weights, prob.seq1, sem)
        ws = WireSlice.from_csr(prob.codes, prob.offsets, letter_format="p33", alloc=own_pages)
        assert ws.len_bits == 6
        assert_rows(solve_pinned(engine, ws, "swipe", (cut, sem)), want, f"{cut} {sem.name} pinned p33")
        ws = WireSlice.from_csr(prob.codes, prob.offsets, letter_format="p33")
        assert_rows(solve_device(engine, ws, True, (cut, sem)), want, f"{cut} {sem.name} device p33")
        assert_rows(topk1_wire(engine, ws, 6, cut), want, f"{cut} {sem.name} top-1")


# ---- base-6 lengths: every octet --------------------------------------------------------------------------
@pytest.mark.parametrize("slice_", dc.OCTET_SLICES, ids=dc.OCTET_IDS)
def test_wire_offsets_kernel_every_octet(engine, slice_):
    """wire_offsets_kernel's wire_length, base 6 (/ 1296, / 36, / 6 by the digit's bits): the slice through
    decode_wire_into with 64-record sparse offsets — device offsets and host offsets against numpy's cumsum of the
    lengths, letters against the source — and with dense offsets (shift 0: they are uploaded, only the letters are
    decoded); then the profile family on the sparse batch (stats() names "wire"): row i is (3 L_i, p_i, 0)."""
    prob, want = dc.octet_copies(*slice_)
    offs = np.zeros(prob.n + 1, np.int64)
    np.cumsum(np.diff(prob.offsets), out=offs[1:])
    ws = WireSlice.from_csr(prob.codes, prob.offsets)
    assert (ws.len_bits, ws.len_base) == (6, 1)
    for shift in (0, 6):
        check_decode(engine, ws, shift, prob.codes, offs, skew=1, what=(slice_, shift))
    engine.set_problem(prob.weights, prob.seq1, Semantics.REFERENCE)
    assert_rows(topk1_wire(engine, ws, 6, slice_), want, f"{slice_} top-1")


@pytest.mark.parametrize("slice_", dc.OCTET_SLICES, ids=dc.OCTET_IDS)
def test_streaming_kernel_every_octet(engine, slice_):
    """record_lengths4, base 6 (/ 1296u for the upper half of an octet, then / 6u chains; kernel_common.hpp), and
    record_length (the / 6u loop) on the records a thread does not take four at a time: the slice as a page-locked P33
    WireSlice through the streaming swipe kernel (direct == 1, kernels == ["swipe"]), and at top digit 5 with byte
    letters too. Row i is (3 L_i, p_i, 0): a wrong length breaks its record and every later start of the tile."""
    prob, want = dc.octet_copies(*slice_)
    for sem in SEMS:
        engine.set_problem(prob.weights, prob.seq1, sem)
        for fmt in ("p33", "bytes") if slice_[0] == 5 else ("p33",):
            ws = WireSlice.from_csr(prob.codes, prob.offsets, letter_format=fmt, alloc=own_pages)
            assert ws.len_bits == 6
            got = solve_pinned(engine, ws, "swipe", (slice_, sem, fmt))
            assert_rows(got, want, f"{slice_} {sem.name} pinned {fmt}")


def test_streaming_kernel_octet_tails(engine):
    """record_length, base 6 (the / 6u loop; kernel_common.hpp): a thread of the streaming kernel takes its records'
    lengths four at a time and the last one, two or three records of a batch one at a time — the slices above are
    whole fours. Batches of 64 + 1, 2, 3, 5, 6, 7 records that end inside each of 20 octets (the ends and steps of the
    octet's halves and upper digits), page-locked P33: direct == 1, kernels == ["swipe"]; row i is (3 L_i, p_i, 0)."""
    for sem in SEMS:
        for value in dc.TAIL_OCTETS:
            for tail in dc.TAILS:
                prob, want = dc.octet_tail(value, tail)
                engine.set_problem(prob.weights, prob.seq1, sem)
                ws = forced_slice(np.diff(prob.offsets), prob.codes, "p33", "base6", alloc=own_pages, base=1)
                assert ws.len_bits == 6 and ws.len_base == 1 and ws.n % 4 != 0
                got = solve_pinned(engine, ws, "swipe", (value, tail, sem))
                assert_rows(got, want, f"octet {value} tail {tail} {sem.name}")


@pytest.mark.parametrize("slice_", dc.OCTET_SLICES, ids=dc.OCTET_IDS)
def test_lane_direct_kernel_every_octet(engine, slice_):
    """lane_length6 (trunc((v + 0.5f) * fl(1 / 6^i)) in f32, 24-bit mads, (u * 11) >> 5 for the octet's word;
    swipe_impl.hpp): the slice device-resident, P33 letters, 64-record sparse offsets, through solve_wire_device:
    direct == 1, kernels == ["swipe"], h2d_bytes == 0. Without its + 0.5f that arithmetic is wrong on 9 octets of all
    6^8 (tests/test_decoder_cases.py): the eight slices hold every one of them."""
    prob, want = dc.octet_copies(*slice_)
    for sem in SEMS:
        engine.set_problem(prob.weights, prob.seq1, sem)
        ws = WireSlice.from_csr(prob.codes, prob.offsets, letter_format="p33")
        assert ws.len_bits == 6
        assert_rows(solve_device(engine, ws, True, (slice_, sem)), want, f"{slice_} {sem.name} device p33 sparse")


def test_short_kernel_half_end_octets(engine):
    """record_lengths4, base 6, in the lane-per-offset short kernel: the octets whose upper or lower half is 0 or 1295
    (short_octets) as lengths 150..155 of byte letters, L1 = 200, page-locked: direct == 1, kernels == ["short"];
    against the CPU engine."""
    prob = dc.short_octets_problem()
    for sem in SEMS:
        want = cpu_rows("short_octets", prob, sem)
        engine.set_problem(prob.weights, prob.seq1, sem)
        ws = WireSlice.from_csr(prob.codes, prob.offsets, letter_format="bytes", alloc=own_pages)
        assert ws.len_bits == 6 and ws.len_base == 150
        assert_rows(solve_pinned(engine, ws, "short", sem), want, f"short octets {sem.name}")


# ---- 3 / 4 / 8-bit lengths: every field value at every index residue ----------------------------------------
def narrow_slice(family, bits, letter_format, alloc=private_alloc):
    prob = dc.narrow(family, bits)
    form, base = dc.narrow_form(family, bits)
    ws = forced_slice(np.diff(prob.offsets), prob.codes, letter_format, form, alloc=alloc, base=base)
    assert ws.len_bits == bits
    return prob, ws


@pytest.mark.parametrize("bits", [3, 4, 8])
def test_narrow_lengths_wire_offsets_kernel(engine, bits):
    """wire_offsets_kernel's wire_length for 3-bit fields (two bytes, a shift), nibbles and bytes: decode_wire_into
    with sparse offsets of 8 and of 64 records against numpy's cumsum and the source letters, then the profile family
    on the batch (stats() names "wire") against the CPU engine."""
    prob, ws = narrow_slice("swipe", bits, "p33")
    for shift in (3, 6):
        check_decode(engine, ws, shift, prob.codes, prob.offsets, skew=2, what=(bits, shift))
    engine.set_problem(prob.weights, prob.seq1, Semantics.SPEC)
    want = search_topk_cpu(prob, 1, Semantics.SPEC)[:, 0]  # (records longer than Seq1 have no row: as top-K says so)
    assert_rows(topk1_wire(engine, ws, 6, bits), want, f"{bits}-bit top-1")


@pytest.mark.parametrize("bits", [3, 4, 8])
def test_narrow_lengths_streaming_kernel(engine, bits):
    """record_lengths4 and record_length for 3 / 4 / 8-bit lengths in the streaming swipe kernel: page-locked P33 and
    byte letters, direct == 1, kernels == ["swipe"]; against the CPU engine. (8-bit: the lengths 1..128 against a Seq1
    of 60, records longer than Seq1 among them.)"""
    for fmt in ("p33", "bytes"):
        prob, ws = narrow_slice("swipe", bits, fmt, own_pages)
        for sem in SEMS:
            want = cpu_rows(("narrow", "swipe", bits), prob, sem)
            engine.set_problem(prob.weights, prob.seq1, sem)
            got = solve_pinned(engine, ws, "swipe", (bits, fmt, sem))
            assert_rows(got, want, f"{bits}-bit {fmt} {sem.name} pinned")


@pytest.mark.parametrize("bits", [3, 4, 8])
def test_narrow_lengths_device_resident(engine, bits):
    """record_length for 3 / 4 / 8-bit lengths in the lane-direct kernel: device-resident P33, 64-record sparse
    offsets, direct == 1, kernels == ["swipe"], h2d_bytes == 0. The lane-direct kernel takes records of at most 16
    words, so its 8-bit batch holds the lengths 1..64; the batch with 1..128 runs too, device-resident through the
    block-synchronous kernel (record_lengths4 from device memory)."""
    for family in ("lane", "swipe") if bits == 8 else ("lane",):
        prob, ws = narrow_slice(family, bits, "p33")
        assert ws.l2_max <= 64 or family == "swipe"
        for sem in SEMS:
            want = cpu_rows(("narrow", family, bits), prob, sem)
            engine.set_problem(prob.weights, prob.seq1, sem)
            got = solve_device(engine, ws, True, (bits, family, sem))
            assert_rows(got, want, f"{bits}-bit {family} {sem.name} device")


@pytest.mark.parametrize("bits", [3, 4])
def test_narrow_lengths_short_kernel(engine, bits):
    """record_lengths4 for 3-bit fields and nibbles in the lane-per-offset short kernel: lengths 150 + field value of
    byte letters, L1 = 200, page-locked: direct == 1, kernels == ["short"]. No 8-bit case: the short kernel takes
    records of more than 128 letters, the 8-bit enumeration is the lengths 1..128."""
    prob, ws = narrow_slice("short", bits, "bytes", own_pages)
    assert ws.len_base == 150
    for sem in SEMS:
        want = cpu_rows(("narrow", "short", bits), prob, sem)
        engine.set_problem(prob.weights, prob.seq1, sem)
        assert_rows(solve_pinned(engine, ws, "short", (bits, sem)), want, f"{bits}-bit {sem.name} short")
