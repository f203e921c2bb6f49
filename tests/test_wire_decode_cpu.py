"""The host wire decode (moc::decode_wire_cpu, the oracle of the GPU decode kernels): every letter form x length
form x sparse shift x record count against WireSlice's own numpy decoders, batches that start inside a longer
stream, every validation error, top-K on the decoded problem, and the stand-alone sanitizer program."""
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from wire_cases import COUNTS, FORMS, LETTERS, SHIFTS, make_case, sub_batch

from mpi_openmp_cuda_amd import Problem, WireSlice, _lib, decode_wire_cpu, make_synthetic, search_topk_cpu


def expected(ws):
    offsets = np.zeros(ws.n + 1, np.int64)
    np.cumsum(ws.decoded_lengths(), out=offsets[1:])
    return np.asarray(ws.letters()), offsets


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("letters", LETTERS)
def test_decode_matrix(letters, form):
    """Letters equal WireSlice.letters() and offsets np.cumsum(decoded_lengths()) at every record count and shift."""
    for n in COUNTS:
        ws = make_case(letters, form, n, seed=n)
        want_codes, want_offsets = expected(ws)
        assert np.array_equal(want_offsets, ws.offsets)
        for shift in SHIFTS:
            if shift and form == "none":
                with pytest.raises(ValueError):
                    decode_wire_cpu(ws, shift)
                continue
            codes, offsets = decode_wire_cpu(ws, shift)
            assert offsets.dtype == np.int64 and np.array_equal(offsets, want_offsets), (n, shift)
            assert codes.dtype == np.uint8 and np.array_equal(codes, want_codes), (n, shift)


@pytest.mark.parametrize("letters", LETTERS)
def test_decode_inside_a_stream(letters):
    """Batches whose first letter lies c0 letters into the stream, c0 % 7 in {0, 1, 6} and c0 % 56 != 0: the first
    and last P33 fields are partial. Offsets stay absolute."""
    rng = np.random.default_rng(5)
    lengths = np.array([7, 1, 5, 8, 6, 9, 7, 6, 10, 5, 6, 11, 7] + [6] * 30, np.int64)
    parent = WireSlice(lengths, rng.integers(1, 27, int(lengths.sum())).astype(np.uint8), letters)
    seen = set()
    for a, b in ((1, 4), (2, 13), (3, 9), (1, 2), (2, 43), (3, 43)):
        c0 = int(parent.offsets[a])
        assert c0 % 56 != 0
        seen.add(c0 % 7)
        for shift in (0, 1, 6):
            batch, keep, sub = sub_batch(parent, a, b, shift)
            codes, offsets = decode_wire_cpu(batch)
            assert np.array_equal(offsets, parent.offsets[a:b + 1]), (a, b, shift)
            assert np.array_equal(codes, parent.letters(c0, int(parent.offsets[b]))), (a, b, shift)
            assert np.array_equal(codes, sub.letters())
    assert seen == {0, 1, 6}


def test_p33_zero_codes_read_back_as_one():
    ws = WireSlice(np.array([3, 4]), np.array([0, 5, 26, 0, 0, 1, 2], np.uint8), "p33")
    codes, _ = decode_wire_cpu(ws)
    assert codes.tolist() == [1, 5, 26, 1, 1, 1, 2]


def _batch(**kw):
    """A valid two-record byte batch with 8-bit lengths, changed by ``kw``."""
    arrays = {"letters": np.ones(11, np.uint8), "offsets": np.array([0, 5, 11], np.int64),
              "lengths": np.array([5, 6], np.uint8)}
    arrays.update({k: kw.pop(k) for k in list(kw) if k in arrays})
    f = dict(n=2, len_base=0, packed=0, off_shift=0, len_bits=8, device=0)
    f.update(kw)
    b = _lib.WireBatch(**{k: (None if a is None else int(a.ctypes.data)) for k, a in arrays.items()}, **f)
    return b, arrays


def test_validation_errors():
    b, keep = _batch()
    codes, offsets = decode_wire_cpu(b)
    assert offsets.tolist() == [0, 5, 11] and codes.tolist() == [1] * 11
    sparse = np.array([0, 11], np.int64)
    for what, kw in (("sparse offsets without lengths", dict(offsets=sparse, off_shift=1, lengths=None)),
                     ("off_shift above 6", dict(off_shift=7)),
                     ("off_shift below 0", dict(off_shift=-1)),
                     ("len_bits 5", dict(len_bits=5)),
                     ("len_bits 0", dict(len_bits=0)),
                     ("n < 0", dict(n=-1)),
                     ("n = 2^31 - 1", dict(n=2 ** 31 - 1)),
                     ("dense end offset against the lengths", dict(offsets=np.array([0, 5, 12], np.int64))),
                     ("sparse end offset against the lengths", dict(offsets=np.array([0, 12], np.int64), off_shift=1))):
        b, keep = _batch(**kw)
        with pytest.raises(_lib.NativeError):
            decode_wire_cpu(b)
        del keep
    # both packings at once cannot be said through the C ABI's one `packed` field: an unknown value is refused
    b, keep = _batch(packed=2)
    with pytest.raises(_lib.NativeError):
        decode_wire_cpu(b)


@pytest.mark.parametrize("letters", LETTERS)
def test_topk_on_the_decoded_problem(letters):
    """search_topk_cpu on the problem rebuilt from the decode equals that on the original bytes."""
    prob = make_synthetic("input6", 200, seed=3)
    ws = WireSlice.from_csr(prob.codes, prob.offsets, letter_format=letters)
    codes, offsets = decode_wire_cpu(ws, 6)
    decoded = Problem(prob.weights, prob.seq1, codes, offsets)
    for sem in ("reference", "spec"):
        assert np.array_equal(search_topk_cpu(decoded, 3, sem), search_topk_cpu(prob, 3, sem))


def test_wire_sanitizer_program():
    """csrc/tests/wire_san.cpp with the CPU core sources under ASan + UBSan: a plain program with its own main
    (make wire-san), every wire array and both outputs in heap blocks of exactly their sizes."""
    r = subprocess.run(["make", "-C", ROOT, "-s", "-j8", "wire-san"], capture_output=True, timeout=600)
    out = r.stdout.decode() + r.stderr.decode()
    assert r.returncode == 0, out[-3000:]
    assert "wire_san ok" in out and "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]
