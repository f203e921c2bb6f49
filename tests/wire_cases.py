"""Wire batches for the decode tests (tests/test_wire_decode_cpu.py, tests/test_gpu_wire_decode.py): WireSlices
with a chosen length form at any record count, and batches that start inside a longer stream."""
import numpy as np

from mpi_openmp_cuda_amd import _lib
from mpi_openmp_cuda_amd.models.problem import (LEN_BASE6, lengths3_bytes, lengths6_bytes, pack_lengths3, pack_lengths4,
                                                pack_lengths6)
from mpi_openmp_cuda_amd.parallel.wire import WireSlice, private_alloc

LETTERS = ("p33", "p5", "bytes")
FORMS = ("base6", "3", "4", "8", "none")
SHIFTS = (0, 1, 3, 6)
COUNTS = (0, 1, 7, 23, 24, 25, 63, 64, 65, 129)
_BITS = {"base6": LEN_BASE6, "3": 3, "4": 4, "8": 8, "none": 0}
_LETTER_CODES = {"bytes": 0, "p5": 1, "p33": 3}


_page_maps = []


def page_alloc(name: str, dtype, count: int) -> np.ndarray:
    """A WireSlice allocator for arrays that a test page-locks: each array in anonymous pages of its own, kept
    mapped for the life of the process. Page-locking covers whole pages, and a heap page shared with other
    objects would make those objects half page-locked: the runtime refuses copies to or from such a range."""
    import mmap

    nbytes = max(int(count) * np.dtype(dtype).itemsize, 1)
    m = mmap.mmap(-1, (nbytes + 4095) & ~4095)
    _page_maps.append(m)
    return np.frombuffer(m, dtype=dtype, count=int(count))


def random_lengths(n: int, form: str, seed: int) -> np.ndarray:
    """n record lengths every narrow form holds above base 5 (5..10); "none": one record of 300 letters among
    them, which no narrow form holds (dense offsets only)."""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(5, 11, n).astype(np.int64)
    if form == "none" and n:
        lengths[n // 2] = 300
    return lengths


def forced_slice(lengths, letters, letter_format: str, form: str, alloc=private_alloc, base: int = 5) -> WireSlice:
    """A WireSlice whose lengths are re-encoded in ``form`` whatever range they span (WireSlice itself picks the
    narrowest form, base 6 for every batch of one record): by default the lengths lie in 5..10, which every form holds
    above ``base`` 5 (8-bit: base 0)."""
    ws = WireSlice(lengths, letters, letter_format, alloc=alloc)
    bits = _BITS[form]
    if form == "none":
        ws.len_bits, ws.len_base, ws.lengths = 0, 0, None
        return ws
    n = ws.n
    ws.len_bits, ws.len_base = bits, (0 if bits == 8 else base)
    if bits == LEN_BASE6:
        ws.lengths = pack_lengths6(lengths, base, out=alloc("lengths6", np.uint8, lengths6_bytes(n)))
    elif bits == 3:
        ws.lengths = pack_lengths3(lengths, base, out=alloc("lengths3", np.uint8, lengths3_bytes(n)))
    elif bits == 4:
        ws.lengths = pack_lengths4(lengths, base, out=alloc("lengths4", np.uint8, (n + 1) // 2))
    else:
        ws.lengths = alloc("lengths", np.uint8, n)
        ws.lengths[:] = lengths
    ws.__dict__.pop("_sparse", None)
    return ws


def make_case(letter_format: str, form: str, n: int, seed: int = 0, alloc=private_alloc) -> WireSlice:
    lengths = random_lengths(n, form, seed)
    rng = np.random.default_rng(seed + 1)
    return forced_slice(lengths, rng.integers(1, 27, int(lengths.sum())).astype(np.uint8), letter_format, form, alloc)


def sub_batch(parent: WireSlice, a: int, b: int, shift: int = 0, alloc=private_alloc):
    """Records [a, b) of ``parent`` as a native batch over the parent's own letter stream: absolute offsets from
    parent.offsets[a], narrow lengths of a from_csr sub-slice. Returns (batch, keep-alive, sub-slice)."""
    c0 = int(parent.offsets[a])
    sub = WireSlice.from_csr(parent.letters(), parent.offsets[a:b + 1], letter_format="bytes", alloc=alloc)
    offsets = alloc("offsets", np.int64, sub.wire_offsets(shift).shape[0])
    offsets[:] = sub.wire_offsets(shift) + c0
    if shift and sub.lengths is None:
        raise ValueError("sparse offsets need narrow lengths")
    batch = _lib.WireBatch(letters=int(parent.codes.ctypes.data), offsets=int(offsets.ctypes.data),
                           lengths=None if sub.lengths is None else int(sub.lengths.ctypes.data), n=sub.n,
                           len_base=int(sub.len_base), packed=_LETTER_CODES[parent.letter_format], off_shift=shift,
                           len_bits=int(sub.len_bits or 8), device=0)
    return batch, (parent, offsets, sub), sub
