"""CPU tier of the wire-decoder cases (tests/decoder_cases.py, utils/synthetic.py): the inputs the GPU tier
(tests/test_gpu_decoders.py) sends through the seven device decoders are what they claim to be, their closed-form rows
equal the CPU engine's for every record under both semantics (no record is left out of any comparison), the host codec
agrees with Python-int arithmetic on them, and numpy models of each device decoder (tools/p33_magic_check.py) are
right on every case and wrong on a counted number of them as soon as one constant is off by one. No deliberately wrong
kernel exists anywhere: a wrong length could send a kernel out of bounds, so the models are the evidence that these
cases catch such slips."""
import numpy as np
import pytest

import decoder_cases as dc
from wire_cases import forced_slice

from mpi_openmp_cuda_amd import Semantics, WireSlice, brute_force_native, decode_wire_cpu, search_cpu
from mpi_openmp_cuda_amd.models.problem import Problem, pack33, pack_lengths6, unpack33
from mpi_openmp_cuda_amd.ops.align import as_triples, kernel_bounds
from mpi_openmp_cuda_amd.utils.synthetic import (NARROW_PERIOD, OCTET_SLICE, OCTETS, P33_P, P33_TOP, READOUT_WEIGHTS,
                                                 differing, narrow_exhaustive_lengths, octet_digits, short_octets)

SEMS = [Semantics.REFERENCE, Semantics.SPEC]


def assert_every_row(prob, want, sem, what):
    got = as_triples(search_cpu(prob, sem))
    assert got.shape == want.shape == (prob.n, 3)  # every record is compared: none left out
    msg = differing(got, want, want[:, 1])
    assert not msg, f"{what} {sem.name}: {msg}"


# ---- the builders ---------------------------------------------------------------------------------------
def test_boundary_fields_are_the_digit_carries():
    f = dc.fields("boundary")
    assert f.dtype == np.uint64 and f.shape == (41230,) and int(f.max()) == P33_TOP and int(f.min()) == 0
    assert f[:4].tolist() == [P33_P - 1, P33_P, 2 * P33_P - 1, 2 * P33_P] and f[-2:].tolist() == [0, P33_TOP]
    have = set(f.tolist())
    assert all(q * P33_P - 1 in have and q * P33_P in have for q in range(1, 26 ** 3))
    assert all(a * P33_P + 676 * m - d in have for a in (0, 8788, 26 ** 3 - 1) for m in range(1, 676) for d in (0, 1))
    assert all(v * s in have for v in range(676) for s in (1, 676, P33_P))
    s = dc.letters("boundary")
    assert s.dtype == np.uint8 and s.shape == (288610,) and np.unique(s).tolist() == list(range(1, 27))
    back = sum((s.reshape(-1, 7)[:, j].astype(object) - 1) * 26 ** j for j in range(7))  # Python ints
    assert back.tolist() == f.tolist()


def test_phase_fields_visit_every_bit_phase():
    f = dc.fields("phase").reshape(2, 32, 64)
    for half, (mark, fill) in enumerate(((P33_TOP, 0), (0, P33_TOP))):
        for run in range(32):
            want = [fill] * 64
            want[run] = mark
            assert f[half, run].tolist() == want
            field = (half * 32 + run) * 64 + run  # its index in the stream
            assert (33 * field) % 32 == run
    s = dc.letters("phase")
    assert s.shape == (7 * 4096,) and set(np.unique(s).tolist()) == {1, 26}


@pytest.mark.parametrize("bits", [3, 4, 8])
def test_narrow_lengths_hold_every_value_at_every_residue(bits):
    base = 0 if bits == 8 else 5
    lengths = narrow_exhaustive_lengths(bits, base)
    values = list(range(1, 129)) if bits == 8 else [base + v for v in range(1 << bits)]
    period = NARROW_PERIOD[bits]
    assert lengths.shape == (2 * len(values) * period * period,)
    seen = set()
    for i, L in enumerate(lengths.tolist()):
        left, right = lengths[i - 1] if i % period else None, lengths[i + 1] if (i + 1) % period else None
        near = {int(x) for x in (left, right) if x is not None}
        for fill in (values[0], values[-1]):
            if near == {fill}:
                seen.add((L, i % period, fill))
    assert seen >= {(v, r, fill) for v in values for r in range(period) for fill in (values[0], values[-1])}
    for family, forms in dc.NARROW.items():
        if bits in forms:
            prob = dc.narrow(family, bits)
            L1, fbase, top = forms[bits]
            want = narrow_exhaustive_lengths(bits, fbase, top)
            assert np.array_equal(np.diff(prob.offsets), want) and prob.L1 == L1
            form, b = dc.narrow_form(family, bits)
            ws = forced_slice(want, prob.codes, "p33", form, base=b)
            assert ws.len_bits == bits and np.array_equal(ws.decoded_lengths(), want)
            codes, offsets = decode_wire_cpu(ws, 3)
            assert np.array_equal(offsets, prob.offsets) and np.array_equal(codes, prob.codes)


def test_short_octets_are_the_half_ends():
    v = short_octets()
    assert v.shape == (5180,) and np.unique(v).shape == v.shape
    h, l = v // 1296, v % 1296
    assert ((h == 0) | (h == 1295) | (l == 0) | (l == 1295)).all()
    assert all(np.unique(l[h == e]).shape == (1296,) and np.unique(h[l == e]).shape == (1296,) for e in (0, 1295))
    prob = dc.short_octets_problem()
    lengths = np.diff(prob.offsets)
    assert prob.n == 8 * 5180 and prob.L1 == 200 and lengths.min() == 150 and lengths.max() == 155
    assert np.array_equal(lengths, 150 + octet_digits(v).reshape(-1))
    assert WireSlice.from_csr(prob.codes, prob.offsets, letter_format="bytes").len_bits == 6


# ---- the closed forms against the CPU engine, every record ----------------------------------------------
@pytest.mark.parametrize("sem", SEMS, ids=lambda s: s.name)
@pytest.mark.parametrize("stream", dc.STREAMS)
def test_readout_rows_are_the_cpu_engines(stream, sem):
    prob, want = dc.readout(stream)
    assert prob.n == dc.letters(stream).shape[0] and (np.diff(prob.offsets) == 1).all()
    assert np.array_equal(want[:, 1] + 1, dc.letters(stream)) and (want[:, 0] == 1).all() and (want[:, 2] == 0).all()
    assert_every_row(prob, want, sem, f"readout {stream}")
    assert kernel_bounds(READOUT_WEIGHTS, prob.L1, 1, 1)["swipe"] == "swipe_kbits"
    ws = WireSlice.from_csr(prob.codes, prob.offsets)
    assert (ws.len_bits, ws.len_base, ws.letter_format) == (6, 1, "p33")


@pytest.mark.parametrize("slice_", dc.OCTET_SLICES, ids=dc.OCTET_IDS)
def test_octet_copy_rows_are_the_cpu_engines(slice_):
    top, rot = slice_
    prob, want = dc.octet_copies(top, rot)
    lengths = np.diff(prob.offsets)
    assert prob.n == 8 * OCTET_SLICE + 8 * rot and (lengths[:8 * rot] == 1).all()
    values = np.arange(top * OCTET_SLICE, (top + 1) * OCTET_SLICE)
    assert np.array_equal(lengths[8 * rot:], 1 + octet_digits(values).reshape(-1))
    assert (want[:, 1] + lengths <= 25).all() and (want[:, 1] >= 0).all()
    ws = WireSlice.from_csr(prob.codes, prob.offsets)
    assert (ws.len_bits, ws.len_base) == (6, 1)
    for sem in SEMS:
        assert_every_row(prob, want, sem, f"octet copies {slice_}")
    pick = np.sort(np.random.default_rng(top * 3 + rot).choice(prob.n, 2000, replace=False))
    recs = [prob.codes[prob.offsets[i]:prob.offsets[i + 1]] for i in pick]
    offsets = np.zeros(len(recs) + 1, np.int64)
    np.cumsum([len(r) for r in recs], out=offsets[1:])
    sample = Problem(prob.weights, prob.seq1, np.concatenate(recs), offsets)
    for sem in SEMS:
        assert np.array_equal(as_triples(brute_force_native(sample, sem)), want[pick]), sem


def test_octet_tail_rows_are_the_cpu_engines():
    assert len(set(dc.TAIL_OCTETS)) == len(dc.TAIL_OCTETS) == 20
    for value in dc.TAIL_OCTETS:
        for tail in dc.TAILS:
            prob, want = dc.octet_tail(value, tail)
            lengths = np.diff(prob.offsets)
            assert prob.n == 64 + tail and prob.n % 4 != 0
            assert np.array_equal(lengths[64:], 1 + octet_digits([value])[0, :tail])
            ws = forced_slice(lengths, prob.codes, "p33", "base6", base=1)
            assert np.array_equal(ws.decoded_lengths(), lengths)
            for sem in SEMS:
                assert_every_row(prob, want, sem, f"octet tail {value} {tail}")


def test_octet_slices_cover_every_octet_at_every_word_position():
    tops = sorted(t for t, r in dc.OCTET_SLICES if r == 0)
    assert tops == list(range(6)) and 6 * OCTET_SLICE == OCTETS
    assert sorted(r for t, r in dc.OCTET_SLICES if t == 5) == [0, 1, 2]
    assert OCTET_SLICE % 3 == 0  # a slice starts at position 0 of a word: rot is the value's position shift


@pytest.mark.parametrize("cut", dc.RECORD_CUTS)
def test_letter_records_against_brute_force(cut):
    """The CPU engine, the GPU tier's reference on these two batches, against the literal replay on a sample."""
    prob = dc.letter_records(cut)
    lengths = np.diff(prob.offsets)
    assert np.array_equal(prob.codes, dc.letters("boundary")) and prob.L1 == 40
    assert set(lengths.tolist()) == ({7} if cut == "sevens" else set(range(1, 7)))
    pick = np.sort(np.random.default_rng(7).choice(prob.n, 3000, replace=False))
    recs = [prob.codes[prob.offsets[i]:prob.offsets[i + 1]] for i in pick]
    offsets = np.zeros(len(recs) + 1, np.int64)
    np.cumsum([len(r) for r in recs], out=offsets[1:])
    sample = Problem(prob.weights, prob.seq1, np.concatenate(recs), offsets)
    for sem in SEMS:
        assert np.array_equal(as_triples(brute_force_native(sample, sem)), as_triples(search_cpu(prob, sem))[pick])


# ---- the host codec on the same streams -------------------------------------------------------------------
def pack33_python(codes) -> np.ndarray:
    """P33 in Python-int arithmetic: field f = sum (code - 1) 26^j at bits [33 f, 33 f + 33); eight fields are 33
    whole bytes."""
    vals = []
    for f in range(0, len(codes), 7):
        vals.append(sum((int(c) - 1) * 26 ** j for j, c in enumerate(codes[f:f + 7])))
    out = bytearray()
    for g in range(0, len(vals), 8):
        chunk = vals[g:g + 8]
        big = 0
        for i, x in enumerate(chunk):
            big |= x << (33 * i)
        out += big.to_bytes((33 * len(chunk) + 7) // 8, "little")
    return np.frombuffer(bytes(out), np.uint8)


@pytest.mark.parametrize("stream", dc.STREAMS)
def test_host_codec_on_the_streams(stream):
    """pack33 (thousands of fields: past the packer's vector block size) against the Python-int packer; unpack33 and
    decode_wire_cpu give the letters back, from the start and from 1 and 6 letters in."""
    s = dc.letters(stream)
    want = pack33_python(s.tolist())
    assert want.shape[0] == (33 * (s.shape[0] // 7) + 7) // 8
    packed = pack33(s)
    assert np.array_equal(packed[:want.shape[0]], want)
    for begin in (0,) + dc.SUB_STARTS:
        assert np.array_equal(unpack33(packed, begin, s.shape[0] - begin), s[begin:])
    prob, _ = dc.readout(stream)
    ws = WireSlice.from_csr(prob.codes, prob.offsets)
    assert np.array_equal(ws.codes[:want.shape[0]], want)
    for shift in (0, 6):
        codes, offsets = decode_wire_cpu(ws, shift)
        assert np.array_equal(codes, s) and np.array_equal(offsets, prob.offsets)


@pytest.mark.parametrize("top", range(6))
def test_base6_round_trip_of_every_octet(top):
    """pack_lengths6 -> the 21-bit octets by plain shifts, WireSlice.decoded_lengths and decode_wire_cpu, for the 6^7
    octet values of one top digit per case: all 6^8 over the six cases."""
    values = np.arange(top * OCTET_SLICE, (top + 1) * OCTET_SLICE, dtype=np.int64)
    lengths = 1 + octet_digits(values).reshape(-1)
    words = pack_lengths6(lengths, 1).view("<u8")
    octets = np.stack([(words >> np.uint64(21 * f)) & np.uint64(0x1FFFFF) for f in range(3)], axis=1).reshape(-1)
    assert np.array_equal(octets.astype(np.int64), values) and (words >> np.uint64(63) == 0).all()
    ws = WireSlice(lengths, None, "bytes")
    assert ws.len_bits == 6 and ws.len_base == 1
    assert np.array_equal(ws.decoded_lengths(), lengths)
    ws.codes[:] = 1
    assert np.array_equal(decode_wire_cpu(ws, 6)[1], ws.offsets)


# ---- numpy models of the device decoders ---------------------------------------------------------------------
def _wrong(got, want) -> int:
    return int((np.asarray(got) != want).any(axis=1).sum())


def test_p33_models_are_right_on_every_case():
    m = dc.models()
    for stream in dc.STREAMS:
        f, want = dc.fields(stream), dc.letters(stream).reshape(-1, 7)
        for fn in (m.p33_streaming, m.p33_lane_direct, m.p33_unpack):
            assert _wrong(fn(f), want) == 0, (fn.__name__, stream)


def test_p33_slips_are_caught_by_the_boundary_set():
    """One constant off by one, in the model of each decoder that uses it: fields of the boundary set that come out
    wrong. (Among 2 000 000 uniformly random fields the first slip breaks about 80.)"""
    m = dc.models()
    f, want = dc.fields("boundary"), dc.letters("boundary").reshape(-1, 7)
    for fn in (m.p33_lane_direct, m.p33_unpack):
        assert _wrong(fn(f, magic_p4=m.MAGIC_P4 - 1), want) == 18250, fn.__name__   # of 41 230
        assert _wrong(fn(f, magic_676=m.MAGIC_676 - 1), want) == 3425, fn.__name__
    assert _wrong(m.p33_unpack(f, magic_26=m.MAGIC_26 - 1), want) == 1525


@pytest.fixture(scope="module")
def all_octets():
    v = np.arange(OCTETS, dtype=np.int64)
    return v, octet_digits(v)


def test_base6_models_are_right_on_every_octet(all_octets):
    m = dc.models()
    v, want = all_octets
    for fn in (m.len6_lengths4, m.len6_record, m.len6_lane, m.len6_wire):
        assert _wrong(fn(v), want) == 0, fn.__name__


def test_base6_slips_are_caught_by_the_enumeration(all_octets):
    """lane_length6 without its + 0.5f is wrong on 9 octets of 1 679 616 (a batch of 5 000 random octets meets one in
    about 1 run in 40), a split by 1295 on half of them; the short kernel's set catches the latter too."""
    m = dc.models()
    v, want = all_octets
    bad = (m.len6_lane(v, half=0.0) != want).any(axis=1)
    assert int(bad.sum()) == 9 and tuple(v[bad].tolist()) == dc.NO_HALF_OCTETS
    tops = set((v[bad] // OCTET_SLICE).tolist())
    assert tops <= {t for t, r in dc.OCTET_SLICES if r == 0}
    assert _wrong(m.len6_lengths4(v, div_half=1295), want) == 840456
    assert _wrong(m.len6_wire(v, div_half=1295), want) == 840456
    s = short_octets()
    assert _wrong(m.len6_lengths4(s, div_half=1295), octet_digits(s)) == 2591   # of 5 180
