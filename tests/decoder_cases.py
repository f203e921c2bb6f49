"""Case lists of the wire-decoder tests, shared by the GPU tier (tests/test_gpu_decoders.py), which runs them through
every piece of device arithmetic that turns the wire formats back into letters and lengths, and the CPU tier
(tests/test_decoder_cases.py), which proves the closed-form rows against the CPU engine for every record and shows, on
numpy models of that arithmetic (tools/p33_magic_check.py), that these cases tell a constant that is off by one from
the right one. The builders are utils/synthetic.py's. Plain data and numpy: no GPU. Problems are built once, shared,
and must not be written to."""
import importlib.util
import os

import numpy as np

from mpi_openmp_cuda_amd.models.problem import Problem
from mpi_openmp_cuda_amd.models.scoring import Weights
from mpi_openmp_cuda_amd.utils.synthetic import (OCTET_WEIGHTS, OCTETS, make_letter_readout, make_narrow_exhaustive,
                                                 make_octet_copies, make_octet_tail, make_short_octets,
                                                 p33_boundary_fields, p33_field_letters, p33_phase_fields)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (top digit, rot): every octet value once, and the top-digit-5 values at the two other positions of a word
OCTET_SLICES = [(top, 0) for top in range(6)] + [(5, 1), (5, 2)]
OCTET_IDS = [f"top{t}_rot{r}" for t, r in OCTET_SLICES]
# batches that end inside an octet (the slices above hold whole octets, and whole fours of records): the octet that
# ends the batch, after the eight others of this list that follow it cyclically, cut after each count of its records.
# The ends and steps of the two halves (6^4 = 1296), of digits 5 and 6, and the nine octets that the f32 decode of
# lane_length6 gets wrong without its + 0.5f (tests/test_decoder_cases.py shows that they are those).
NO_HALF_OCTETS = (7776, 15552, 31104, 62208, 124416, 248832, 497664, 987552, 995328)
TAIL_OCTETS = (0, OCTETS - 1, 1295, 1296, 1297, 1295 * 1296, 7775, 46655, 46656, 279935, 279936) + NO_HALF_OCTETS
TAILS = (1, 2, 3, 5, 6, 7)
STREAMS = ("boundary", "phase")
SUB_STARTS = (1, 6)  # letters into the stream at which the sub-batches start

W_RECORDS = (10, 2, 3, 4)
RECORD_CUTS = ("sevens", "cycle")

# narrow length forms: bits -> (L1, base, largest 8-bit length) of the batch per consumer family. "swipe": the
# streaming kernel and the offsets kernel; "lane": the lane-direct kernel, which takes records of at most 16 words
# (64 letters); "short": the lane-per-offset kernel, records of more than 128 letters — which no 8-bit batch with the
# lengths 1..128 has.
NARROW = {
    "swipe": {3: (40, 5, None), 4: (40, 5, None), 8: (60, 0, 128)},
    "lane": {3: (40, 5, None), 4: (40, 5, None), 8: (60, 0, 64)},
    "short": {3: (200, 150, None), 4: (200, 150, None)},
}

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def models():
    """tools/p33_magic_check.py as a module."""
    def load():
        path = os.path.join(ROOT, "tools", "p33_magic_check.py")
        spec = importlib.util.spec_from_file_location("p33_magic_check", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod

    return _once("models", load)


def fields(stream: str) -> np.ndarray:
    return _once(("fields", stream), {"boundary": p33_boundary_fields, "phase": p33_phase_fields}[stream])


def letters(stream: str) -> np.ndarray:
    """The stream's letters: 288 610 (boundary) or 28 672 (phase)."""
    return _once(("letters", stream), lambda: p33_field_letters(fields(stream)))


def readout(stream: str):
    """(problem, rows) of make_letter_readout on the stream's letters."""
    return _once(("readout", stream), lambda: make_letter_readout(letters(stream)))


def letter_records(cut: str) -> Problem:
    """The boundary stream cut into records of 7 letters (one field each: "sevens") or of 1..6 letters cycling
    ("cycle", the last record what is left), against a random Seq1 of 40 letters under (10, 2, 3, 4): a shape whose
    result depends on every letter of a record. The reference is the CPU engine."""
    def make():
        stream = letters("boundary")
        total = stream.shape[0]
        if cut == "sevens":
            assert total % 7 == 0
            lengths = np.full(total // 7, 7, np.int64)
        else:
            lengths = np.tile(np.arange(1, 7, dtype=np.int64), total // 21 + 1)
            ends = np.cumsum(lengths)
            lengths = lengths[:int(np.searchsorted(ends, total, side="left")) + 1]
            lengths[-1] -= int(lengths.sum()) - total
            assert lengths.sum() == total and lengths.min() >= 1 and lengths.max() == 6
        offsets = np.zeros(lengths.shape[0] + 1, np.int64)
        np.cumsum(lengths, out=offsets[1:])
        seq1 = np.random.default_rng(40).integers(1, 27, 40).astype(np.uint8)
        return Problem(Weights.of(W_RECORDS), seq1, stream, offsets)

    return _once(("records", cut), make)


def octet_copies(top: int, rot: int):
    """(problem, rows) of make_octet_copies(top, rot). The problem and the starts are kept, the rows made per call."""
    def make():
        prob, rows = make_octet_copies(top, rot)
        return prob, rows[:, 1].astype(np.uint8)

    prob, p = _once(("octets", top, rot), make)
    lengths = np.diff(prob.offsets)
    rows = np.stack([OCTET_WEIGHTS[0] * lengths, p.astype(np.int64), np.zeros_like(lengths)], axis=1).astype(np.int32)
    return prob, rows


def octet_tail(value: int, tail: int):
    """(problem, rows) of make_octet_tail: 64 + ``tail`` records, the last ``tail`` of them digits of ``value``."""
    at = TAIL_OCTETS.index(value)
    values = [TAIL_OCTETS[(at + 1 + j) % len(TAIL_OCTETS)] for j in range(8)] + [value]
    return _once(("tail", value, tail), lambda: make_octet_tail(values, tail))


def narrow(family: str, bits: int) -> Problem:
    L1, base, top = NARROW[family][bits]
    return _once(("narrow", family, bits), lambda: make_narrow_exhaustive(bits, L1, base=base, top=top))


def narrow_form(family: str, bits: int):
    """(form name of wire_cases.forced_slice, base) of the family's batch."""
    return str(bits), NARROW[family][bits][1]


def short_octets_problem() -> Problem:
    return _once("short_octets", make_short_octets)
