"""CPU-tier checks of the far-offset inputs (tests/csr_slices.py: arena placements whose offsets pass 2^31 and 2^32)
and of the host code that carries such offsets. The GPU tier (tests/test_gpu_far_offsets.py) relies on the first part:
a kernel that loses the upper half of an offset cannot return the oracle's rows by accident.

The arena here is an anonymous mapping of the arena's 6 GiB + 16 MiB of address space, of which only the landing
windows and the slice are written (zero pages cost nothing)."""
import ctypes
import subprocess

import numpy as np
import pytest

import staged_chunks as sc
from conftest import ROOT
from csr_slices import (ARENA, FAMILIES, FILLS, FRONT, HEAD, LANDING, PLACEMENTS, R_MAX, TAIL, VIEW, WINDOW,
                        WRONG_READERS, far_case, family_case, host_arena, lay, pack5_int, pack33_int, packed_case,
                        packed_placements, packed_position, place_bits, unlay, unpack33_int, wrong_reader_problem)

from mpi_openmp_cuda_amd import _lib, search_cpu
from mpi_openmp_cuda_amd.models.problem import unpack5, unpack33
from mpi_openmp_cuda_amd.ops.align import _LETTER_CODES, as_triples, decode_wire_cpu, empty_results, staged_chunks
from mpi_openmp_cuda_amd.parallel.wire import WireSlice

# model -> the placements at which it reads exactly what the right reader reads
NOT_WRONG = {"uint32": ("bit31", "across31"), "end_takes_start_high": ("bit31", "hi1", "across31")}
PACKED_FAMILY = "swipe_r2"  # 1 100 records of 6..11 letters: base-6 lengths, 18 sparse entries


@pytest.fixture(scope="module")
def arena():
    a, view = host_arena()
    yield a, view
    del view, a


def test_layout():
    assert FRONT == 2**31 and VIEW == 2**32 + 2**24 and ARENA == FRONT + VIEW and 2 * R_MAX <= WINDOW
    assert LANDING == ((0, WINDOW), (FRONT - WINDOW, 2 * WINDOW))
    for name in sorted(FAMILIES):
        sub = family_case(name).sub
        total = int(sub.offsets[-1])
        for p in PLACEMENTS:
            case = far_case(name, p)
            o = [int(x) for x in case.offsets]
            assert np.array_equal(case.sub.codes, sub.codes) and o[0] == case.c0 and o[-1] - o[0] == total
            assert case.offsets.dtype == np.int64 and HEAD <= o[0] and o[-1] + TAIL <= VIEW
            k = 31 if p.endswith("31") else 32
            if p in ("bit31", "hi1"):
                assert all(x >> k == 1 for x in o)  # bit 31 with a zero high word; a high word of 1
            else:
                assert o[0] < 2**k < o[-1]  # records on both sides
                assert (2**k in o) == (p != "inside32")  # between two records, or inside one
            # what a truncating reader makes of any offset lands in the windows that hold letter 1
            for x in o:
                u = x & 0xFFFFFFFF
                for t in (u, u - 2**32 if u >> 31 else u):
                    if t != x:
                        assert any(lo <= FRONT + t and FRONT + t + 4096 <= lo + nb for lo, nb in LANDING), (name, p, x)


def test_every_placement_tells_every_wrong_reader(arena):
    """Every family x placement x wrong-reader model x fill: the rows that the CPU engine gives on the letters the
    wrong reader takes out of the arena differ from the expected ones. A model that reads outside the arena cannot
    return rows at all ("leaves"): the swapped words always do (a low word of at least 32 becomes an offset past
    2^37). A model that reads exactly what the right reader reads is not wrong at that placement ("same"), which is so
    exactly where NOT_WRONG says: an unsigned truncation keeps an offset below 2^32 (``bit31`` and ``across31`` are
    there for the signed one), and ``end_takes_start_high`` errs only where a record ends past a 2^32 boundary that it
    starts below — ``across32`` and ``inside32``. Everywhere else every model must be told, under both fills."""
    a, view = arena
    counts = {m: dict(told=0, leaves=0, same=0, missed=0) for m in WRONG_READERS}
    missed = []
    for name in sorted(FAMILIES):
        want = as_triples(search_cpu(family_case(name).sub))
        for p in PLACEMENTS:
            case = far_case(name, p)
            for fill in FILLS:
                at, nb = lay(view, case, fill)
                for m in WRONG_READERS:
                    prob, changed = wrong_reader_problem(a, case, m)
                    if not changed:
                        counts[m]["same"] += 1
                        assert p in NOT_WRONG.get(m, ()), (name, p, m)
                    elif p in NOT_WRONG.get(m, ()):
                        raise AssertionError((name, p, m, "reads elsewhere after all"))
                    elif prob is None:
                        counts[m]["leaves"] += 1
                        assert m == "words_swapped", (name, p, m)
                    elif (as_triples(search_cpu(prob)) != want).any():
                        counts[m]["told"] += 1
                    else:
                        counts[m]["missed"] += 1
                        missed.append((name, p, fill, m))
                unlay(view, at, nb)
    cases = len(FAMILIES) * len(PLACEMENTS) * len(FILLS)
    for m in WRONG_READERS:
        print(f"wrong reader {m}: {cases} family x placement x fill cases: {counts[m]}")
    assert not missed, missed
    per = len(FAMILIES) * len(FILLS)
    for m in ("uint32", "int32", "end_takes_start_high"):
        same = per * len(NOT_WRONG.get(m, ()))
        assert counts[m] == dict(told=cases - same, leaves=0, same=same, missed=0), (m, counts[m])
    assert counts["words_swapped"] == dict(told=0, leaves=cases, same=0, missed=0)


def test_the_right_reader_gets_the_rows(arena):
    """The CPU engine on the arena with absolute offsets (the base pointer of the view and offsets past 2^31 / 2^32)
    against itself on the slice from 0."""
    a, view = arena
    for name in ("swipe_w4", "short_pk", "tile16", "profile"):
        sub = family_case(name).sub
        want = search_cpu(sub)
        for p in PLACEMENTS:
            case = far_case(name, p)
            at, nb = lay(view, case, "continue")
            out = empty_results(sub.n)
            _lib.check(_lib.lib().moc_cpu_solve(_lib.weights_arg(sub.weights.as_list()), _lib.ptr(sub.seq1), sub.L1,
                                                ctypes.c_void_p(view.ctypes.data), _lib.ptr(case.offsets), sub.n, 0, 0,
                                                _lib.ptr(out)))
            unlay(view, at, nb)
            assert np.array_equal(out, want), (name, p)


def test_place_bits_keeps_the_neighbours():
    buf = np.full(16, 0xA5, np.uint8)
    before = int.from_bytes(bytes(buf), "little")
    assert place_bits(buf, 13, 0b1011001, 7) == (1, 2)
    after = int.from_bytes(bytes(buf), "little")
    assert (after >> 13) & 0x7F == 0b1011001
    mask = 0x7F << 13
    assert after & ~mask == before & ~mask
    v, bits = pack33_int([1] * 6 + [26] + [2] + [1] * 6)
    assert bits == 66 and v == (25 * 26**6) | (1 << 33)
    assert pack5_int([1, 26, 3]) == (1 | 26 << 5 | 3 << 10, 15)


def _wire_batch(view, pc, ws, shift):
    offsets = np.ascontiguousarray((ws.sparse_offsets(shift) if shift else ws.offsets) + pc.case.c0)
    b = _lib.WireBatch(letters=int(view.ctypes.data), offsets=int(offsets.ctypes.data), lengths=int(ws.lengths.ctypes.data),
                       n=ws.n, len_base=int(ws.len_base), packed=_LETTER_CODES[pc.letters], off_shift=shift,
                       len_bits=int(ws.len_bits), device=0)
    return b, offsets


@pytest.mark.parametrize("letters", ["p33", "p5"])
def test_host_codecs_at_far_positions(arena, letters):
    """unpack33 / unpack5 and decode_wire_cpu (p33_first_byte, p33_end_byte, expand_offsets, wire_dense_offsets) where
    the packed stream's bit position, byte position and letter index lie just past 2^31 and 2^32, at each phase:
    against the slice's letters and against Python-int arithmetic on the same bits."""
    _, view = arena
    sub = family_case(PACKED_FAMILY).sub
    total = int(sub.offsets[-1])
    ws = WireSlice.from_csr(sub.codes, sub.offsets, letter_format="bytes")
    assert ws.len_bits == 6 and ws.sparse_offsets(6).shape[0] == 19
    placements = packed_placements(letters)
    assert len(placements) == (18 if letters == "p33" else 48)
    for what in ("bit", "byte", "letter"):
        for k in (31, 32):
            at = [packed_position(letters, c0)[what] for name, c0 in placements if name.startswith(f"{what}{k}_")]
            assert all(2**k <= x < 2**k + 64 for x in at), (what, k, at)
    for name, c0 in placements:
        pc = packed_case(PACKED_FAMILY, letters, c0)
        assert c0 % (7 if letters == "p33" else 8) == int(name.rsplit("ph", 1)[1])
        got = {}
        for fill in FILLS:
            bit, value, bits = pc.run(fill)
            b0, nb = pc.lay(view, fill)
            unpack = unpack33 if letters == "p33" else unpack5
            got[fill] = unpack(view, c0, total)
            assert np.array_equal(got[fill], sub.codes), (name, fill)
            if letters == "p33":  # Python ints on the bytes that were written
                stream = int.from_bytes(bytes(view[b0:b0 + nb]), "little")
                assert np.array_equal(unpack33_int(stream, 8 * b0, c0, total), sub.codes), (name, fill)
            else:
                stream = int.from_bytes(bytes(view[b0:b0 + nb]), "little")
                want = [(stream >> (5 * (c0 + i) - 8 * b0)) & 31 for i in range(total)]
                assert want == sub.codes.tolist(), (name, fill)
            for shift in (0, 6):
                batch, keep = _wire_batch(view, pc, ws, shift)
                codes, dense = decode_wire_cpu(batch)
                assert np.array_equal(codes, sub.codes) and np.array_equal(dense, pc.case.offsets), (name, fill, shift)
            view[b0:b0 + nb] = 1
        assert np.array_equal(got["A"], got["continue"])


def test_staged_chunks_at_far_offsets():
    """ops.align.staged_chunks on offsets past 2^31 and 2^32 against the Python-int model, and against the cut of the
    same records from offset 0 (the rule reads differences only)."""
    for name in ("host", "swipe_w4", "mixed"):
        sub = family_case(name).sub
        for p in PLACEMENTS:
            offsets = far_case(name, p).offsets
            for R, B in ((100, 0), (0, 4096), (7, 50), (64, int(sub.offsets[-1]) // 3), (0, 0)):
                got = staged_chunks(offsets, R, B).tolist()
                assert got == sc.model_chunks(offsets, R, B) == staged_chunks(sub.offsets, R, B).tolist(), (name, p, R, B)


def test_far_offsets_sanitizer_program():
    """csrc/tests/far_offsets_san.cpp with the CPU core sources under ASan + UBSan: a plain program with its own main
    (make far-san) on an anonymous mapping of the arena's layout; nothing is loaded into Python, nothing runs on a
    GPU."""
    r = subprocess.run(["make", "-C", ROOT, "-s", "-j8", "far-san"], capture_output=True, timeout=600)
    out = (r.stdout + r.stderr).decode()
    assert r.returncode == 0, out[-3000:]
    assert "far_offsets_san ok" in out and "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]
