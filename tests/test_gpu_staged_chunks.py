"""GPU (MI355X / gfx950) tests of the staged pipeline (HipEngine::run_staged): the cut into chunks of at most
``chunk_records`` records and ``chunk_bytes`` letters, the ring of two slots over the copy, compute and return
streams, slot buffers that grow on reuse, and one plan per chunk.

Every case runs a batch of tests/staged_chunks.py (a slice of a larger CSR array, offsets[0] = 12 345) on an engine of
its own with the chunk sizes under test, twice — the first solve grows the slots, the second finds them grown — into
a result array that is a row slice of a larger, poisoned one, and asserts
  * the exact rows of the CPU engine on the same records,
  * the poisoned guard rows in front of and behind the results, byte for byte,
  * ``stats()``: ``chunks`` as ``ops.align.staged_chunks`` cuts the batch, ``records``, ``direct == 0``,
    ``d2h_bytes == fb * n`` and the kernels the case is named for.
tests/test_staged_chunks.py shows without a GPU that the batches reach what they are run for and that their rows
tell a stale slot, a misplaced result block or a wrong bit phase from a right run."""
import json

import numpy as np
import pytest

import staged_chunks as sc
from conftest import expected, gpu_available, input_path, run_final

pytestmark = pytest.mark.gpu

if not gpu_available():  # pragma: no cover - collected on CPU hosts only with -m gpu
    pytest.skip("no GPU", allow_module_level=True)

from mpi_openmp_cuda_amd import HipSearchEngine, Problem, Semantics, _lib  # noqa: E402
from mpi_openmp_cuda_amd.models.problem import pack_lengths4  # noqa: E402
from mpi_openmp_cuda_amd.ops.align import as_triples, staged_chunks  # noqa: E402
from mpi_openmp_cuda_amd.parallel.wire import WireSlice  # noqa: E402

REF, SPEC = Semantics.REFERENCE, Semantics.SPEC


class GuardedRows:
    """n result rows of format ``fmt`` as rows GUARD .. GUARD + n of a larger array, poison everywhere."""

    def __init__(self, n, fmt):
        self.fb = sc.FORMAT_BYTES[fmt]
        self.lo, self.hi = sc.GUARD * self.fb, (sc.GUARD + n) * self.fb
        self.big = np.full(self.hi + sc.GUARD * self.fb, sc.POISON, np.uint8)
        self.out = self.big[self.lo:self.hi].view(_lib.FORMAT_DTYPES[_lib.FORMAT_NAMES.index(fmt)])
        assert self.out.shape[0] == n and self.out.flags["C_CONTIGUOUS"]

    def poison(self):
        self.big[:] = sc.POISON

    def check_guards(self, what):
        front, back = np.flatnonzero(self.big[:self.lo] != sc.POISON), np.flatnonzero(self.big[self.hi:] != sc.POISON)
        assert front.size == 0, f"{what}: {front.size} guard bytes in front of the results were written"
        assert back.size == 0, f"{what}: {back.size} guard bytes behind the results were written, first at +{back[0]}"


def differing(got, want, bounds):
    bad = np.flatnonzero((got != want).any(axis=1))
    if bad.size == 0:
        return ""
    chunks = sorted({int(np.searchsorted(bounds, i, side="right")) - 1 for i in bad})
    return (f"{bad.size} of {len(want)} rows differ, in chunks {chunks[:8]} of {len(bounds) - 1}; first rows "
            f"{bad[:4].tolist()}: got {got[bad[:3]].tolist()} want {want[bad[:3]].tolist()}")


def run_batch(b, R=0, B=0, fmt="r12", packed5=False, pinned="no", sem=REF, kernels=None, solves=2, eng=None):
    """Solves batch ``b`` on an engine with chunk sizes (R, B) — a fresh one unless ``eng`` is given — and checks
    rows, guards and stats after every solve. ``pinned``: "no", "all" (letters, offsets and results page-locked;
    the zero-copy path is switched off, the staged copies read and write the page-locked arrays) or "half" (only the
    first half of the results). Returns the last stats."""
    what = f"{b.name} R={R} B={B} {fmt}{' p5' if packed5 else ''} pinned={pinned} {sem.name}"
    fb = sc.FORMAT_BYTES[fmt]
    bounds = staged_chunks(b.offsets, R, B)
    assert bounds.tolist() == b.bounds(R, B)
    want = b.rows(sem)
    if kernels is None:
        kernels = sc.chunk_kernels(b, bounds.tolist(), fb)
    # page-locked runs get arrays of their own (registered for the engine's lifetime)
    letters = b.packed5() if packed5 else b.codes
    offsets = b.offsets
    if pinned == "all":
        letters, offsets = letters.copy(), offsets.copy()
    g = GuardedRows(b.n, fmt)
    kw = {}
    if fmt == "r2":  # as tests/test_gpu.py test_r2_results_and_nibble_lengths asks for them
        lo, hi = int(b.lengths.min()), int(b.lengths.max())
        kw = dict(lengths=pack_lengths4(b.lengths, lo), lengths_bits=4, lengths_base=lo, l2_range=(lo, hi))
    own = eng is None
    if own:
        eng = HipSearchEngine(device=0, chunk_records=R, chunk_bytes=B, allow_direct=pinned != "all")
    try:
        eng.set_problem(b.prob.weights, b.prob.seq1, sem)
        if pinned == "all":
            eng.pin(letters, offsets, g.out, kw.get("lengths"))
        elif pinned == "half":
            eng.pin(g.out.view(np.uint8)[:(g.hi - g.lo) // 2])
        st = None
        for run in range(solves):
            g.poison()
            eng.solve(letters, offsets, out=g.out, fmt=fmt, packed5=packed5, **kw)
            st = eng.stats()
            got = as_triples(g.out, r2=st["r2"])
            msg = differing(got, want, bounds)
            assert not msg, f"{what} solve {run}: {msg}"
            g.check_guards(f"{what} solve {run}")
            assert st["chunks"] == len(bounds) - 1 and st["records"] == b.n and st["direct"] == 0, (what, run, st)
            assert st["d2h_bytes"] == fb * b.n and st["format"] == fmt, (what, run, st)
            assert st["kernels"] == kernels, (what, run, st["kernels"], kernels)
        return st
    finally:
        if own:
            eng.close()


# ---- cut rules ---------------------------------------------------------------------------------------------------
def _cut_params():
    return [pytest.param(name, R, B, id=f"{name}-{tag}")
            for name in sc.CUT_BATCHES for tag, R, B in sc.cut_cases(sc.batch(name).lengths)]


@pytest.mark.parametrize("name,R,B", _cut_params())
def test_cut_rules(name, R, B):
    b = sc.batch(name)
    run_batch(b, R, B)
    if name == "swipe6":
        assert sc.chunk_kernels(b, b.bounds(R, B)) == ["swipe"]


# ---- ring depth: 1, 2, 3, 4, 5, 8 and 9 chunks over the two slots ------------------------------------------------
@pytest.mark.parametrize("count", sc.RING_COUNTS)
def test_ring_depth(count):
    st = run_batch(sc.batch("ring"), sc.ring_records(count), kernels=["swipe"])
    assert st["chunks"] == count


# ---- growth on reuse -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["growth", "growth_reversed"])
def test_slots_grow_on_reuse(name):
    # rising: every chunk finds the slot of the chunk two before it too small and reallocates it behind a device
    # synchronise while the other slot's chunk is in flight; falling: every chunk leaves the longer letters of the
    # chunk two before it behind its own
    st = run_batch(sc.batch(name), sc.GROWTH_R, kernels=["tile16"])
    assert st["chunks"] == len(sc.GROWTH_LENGTHS)


# ---- chunk-start phases ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pinned", ["no", "all"])
@pytest.mark.parametrize("packed5", [False, True], ids=["bytes", "p5"])
@pytest.mark.parametrize("name,kernels", [("phase_swipe", ["swipe"]), ("phase_tile16", ["tile16"])])
def test_chunk_start_phases(name, kernels, packed5, pinned):
    # a chunk starts at every residue of offsets[rb] mod 16 (the copy kernel's byte loop against its 16-byte loop)
    # and, with 5-bit letters, at every bit phase of the staged unpack
    st = run_batch(sc.batch(name), sc.PHASE_R, packed5=packed5, pinned=pinned, kernels=kernels)
    assert st["chunks"] == sc.PHASE_CHUNKS


# ---- result placement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pinned", ["no", "all", "half"])
@pytest.mark.parametrize("fmt", ["r12", "r8", "r4", "r2"])
def test_result_placement(fmt, pinned):
    # chunk c's block lands at out + rb * fb, off the 16-byte boundary for most chunks
    b = sc.batch("placement")
    st = run_batch(b, sc.PLACEMENT_R, fmt=fmt, pinned=pinned, kernels=["swipe"])
    assert st["chunks"] == -(-sc.PLACEMENT_N // sc.PLACEMENT_R)


# ---- a kernel per chunk ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", [REF, SPEC], ids=["reference", "spec"])
@pytest.mark.parametrize("wname", list(sc.KERNEL_WEIGHTS))
def test_a_kernel_per_chunk(wname, sem):
    """Segments of 40 records that each take another kernel, alone and as consecutive chunks of one batch. Two
    facts of the planner's rules that stats() confirms here: at Seq1 = 150 letters the short kernel's LDS still
    holds a 20 000-letter record in a tile of one record, so that segment stays on the short kernel and the
    60 000-letter segment is the one whose every record goes to the tile kernel; and the weights (300, 2, 3, 4) fit
    the int16 tile16 profile, so the LUT tile kernel is reached with (300, 300, 1, 1)."""
    whole = sc.batch(f"kernels_{wname}_all")
    parts = []
    eng = HipSearchEngine(device=0, chunk_records=sc.SEGMENT)
    try:
        for seg in sc.SEGMENTS:  # each segment alone: one chunk, the stated kernels
            b = sc.batch(f"kernels_{wname}_{seg}")
            st = run_batch(b, sc.SEGMENT, sem=sem, kernels=sc.STATED[wname][seg], solves=1, eng=eng)
            assert st["chunks"] == 1
            parts.append(b.rows(sem))
        assert (parts[sc.SEGMENTS.index("unsearchable")] == (sc.INT_MIN, 0, 0)).all()
        assert np.array_equal(whole.rows(sem), np.concatenate(parts))  # the whole batch: the concatenation
        st = run_batch(whole, sc.SEGMENT, sem=sem, kernels=sc.union_kernels(sc.STATED[wname].values()), eng=eng)
        assert st["chunks"] == len(sc.SEGMENTS)  # chunks equal segments
    finally:
        eng.close()
    st = run_batch(whole, 30, sem=sem)  # chunks straddle segments
    if wname == "w10":
        assert st["kernels"] == ["swipe", "short", "tile16"]


# ---- wire forms on the staged path ---------------------------------------------------------------------------------
def guarded_alloc(keep):
    """A WireSlice allocator that makes the results a row slice of a larger, poisoned array."""
    def alloc(name, dtype, count):
        if name != "results":
            return np.empty(count, dtype=dtype)
        fmt = _lib.FORMAT_NAMES[[d.itemsize for d in _lib.FORMAT_DTYPES].index(np.dtype(dtype).itemsize)]
        keep.append(GuardedRows(count, fmt))
        return keep[-1].out
    return alloc


@pytest.mark.parametrize("name,R,shift,kernels", [("swipe6", 7, 0, ["swipe"]), ("swipe6", 7, 3, ["swipe"]),
                                                  ("phase_tile16", 5, 0, ["tile16"]), ("phase_tile16", 5, 3, ["tile16"])])
def test_wire_forms_take_the_staged_path(name, R, shift, kernels):
    # P33 letters in pageable memory are unpacked on the host, sparse offsets (one per 8 records, with the narrow
    # lengths) are rebuilt there; both then run through the chunks
    b = sc.batch(name)
    keep = []
    ws = WireSlice.from_csr(b.codes, b.offsets, letter_format="p33", alloc=guarded_alloc(keep))
    assert ws.lengths is not None and ws.n == b.n
    bounds = staged_chunks(ws.offsets, R)
    assert len(bounds) - 1 == -(-b.n // R)
    eng = HipSearchEngine(device=0, chunk_records=R)
    try:
        eng.set_problem(b.prob.weights, b.prob.seq1)
        ws.alloc_results(eng)
        g = keep[0]
        for run in range(2):
            g.poison()
            if shift:
                eng.solve_wire(ws, shift)
            else:
                ws.solve(eng)
            st = eng.stats()
            msg = differing(ws.triples(eng), b.rows(), bounds)
            assert not msg, (run, msg)
            g.check_guards(f"{name} shift {shift} solve {run}")
            assert st["chunks"] == len(bounds) - 1 and st["records"] == b.n and st["direct"] == 0, st
            assert st["d2h_bytes"] == g.fb * b.n and st["kernels"] == kernels, st
    finally:
        eng.close()


# ---- ./final --------------------------------------------------------------------------------------------------------
def final_chunks(args, i, np_):
    r = run_final(["--backend=hip", "--pin-window=0", "--timing", "--device=0"] + args, stdin_path=input_path(i), np_=np_)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout.decode() == expected(i), args
    d = json.loads([l for l in r.stderr.decode().splitlines() if l.startswith("{")][-1])
    return d["rank_chunks"], d["rank_records"]


@pytest.mark.parametrize("i,np_", [(1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (6, 1), (3, 2)])
def test_final_chunk_flags(i, np_):
    # --chunk-records / --chunk-bytes reach the GPU ranks' engines: byte-equal goldens, and each rank's chunk count
    # in the --timing line is the cut of its records
    offsets = Problem.read(input_path(i)).offsets
    for args, R, B in ((["--chunk-records=3", "--chunk-bytes=4096"], 3, 4096), (["--chunk-records=1"], 1, 0), ([], 0, 0)):
        chunks, records = final_chunks(args, i, np_)
        first = np.concatenate([[0], np.cumsum(records)])
        assert first[-1] == len(offsets) - 1 and len(chunks) == np_
        for q in range(np_):
            mine = offsets[first[q]:first[q + 1] + 1]
            assert chunks[q] == len(staged_chunks(mine, R, B)) - 1, (args, q, chunks, records)
            if not args:
                assert chunks[q] == 1
            elif records[q] > R:
                assert chunks[q] > 1
            if R == 1:
                assert chunks[q] == records[q]
