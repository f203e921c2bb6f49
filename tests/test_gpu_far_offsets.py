"""GPU (MI355X / gfx950) tests of the slice contract at offsets past 2^31 and 2^32: the batch is a slice of an arena
(tests/csr_slices.py: 2^31 guard bytes, then a view of 2^32 + 2^24 bytes, all letter 1) whose first offset has bit 31
set, or a high word, or whose records lie across such a boundary; packed letters where the stream's bit position, byte
position or letter index passes them. A kernel that loses the upper half of an offset reads valid letters elsewhere in
the arena: wrong rows, never an access outside the allocation (tests/test_far_offsets_fixture.py shows on the CPU that
the rows then differ).

Every case asserts what tests/test_gpu_csr_slices.py asserts, through its helpers: the rows equal the CPU engine's on
the slice from offset 0, they are bit-identical between the two neighbour fills, the poisoned guard rows are untouched,
``stats()`` names the kernel and form. No comparison has a tolerance.

Order: the device-resident cases come first (every truncation lands inside the arena); the host forms, which run the
same kernels on an anonymous mapping of which only the slice's pages and the landing windows are page-locked, are
refused once any earlier test of the session has failed."""
import mmap
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, gpu_available
from csr_slices import (ARENA, FEW, FILLS, FRONT, LANDING, far_c0, family_case, host_arena, lay, packed_case,
                        packed_placements, unlay)

pytestmark = pytest.mark.gpu

if not gpu_available():  # pragma: no cover - collected on CPU hosts only with -m gpu
    pytest.skip("no GPU", allow_module_level=True)

import torch  # noqa: E402

from test_gpu_csr_slices import (BINS, DEV, LO, POISON, SEMS, SWIPE, WIDTH, Guarded, differing, feature_forms,  # noqa: E402
                                 keys_case, oracle, rows_of, side_stream, solve_device_case, wire_device_case)

from mpi_openmp_cuda_amd import (HipSearchEngine, Problem, Semantics, TargetSet, _lib,  # noqa: E402
                                 search_hits_cpu, search_summary_cpu, search_targets_cpu, search_targets_summary_cpu,
                                 search_topk_cpu)
from mpi_openmp_cuda_amd.ops.align import as_triples  # noqa: E402
from mpi_openmp_cuda_amd.parallel.wire import WireSlice  # noqa: E402

SPARE = 2 << 30  # free device memory asked for beside the arena
PACKED_FAMILY = "swipe_r2"  # 1 100 records of 6..11 letters: one record word, base-6 lengths, R2 results
_arena = {}


def device_arena():
    """The arena on the device, allocated once per process -> the view (``arena[FRONT:]``, 16-byte aligned)."""
    if "t" not in _arena:
        free, total = torch.cuda.mem_get_info()
        if free < ARENA + SPARE:
            pytest.skip(f"{free} bytes of device memory are free, the arena and its spare need {ARENA + SPARE}")
        _arena["before"] = total - free
        _arena["t"] = torch.full((ARENA,), 1, dtype=torch.uint8, device=DEV)
        assert _arena["t"].data_ptr() % 16 == 0
    return _arena["t"][FRONT:]


@pytest.fixture(scope="module", autouse=True)
def _arena_of_the_module():
    device_arena()
    yield
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    print(f"\nfar offsets: arena {ARENA} bytes; device memory in use at the module's end {total - free} "
          f"(before the arena {_arena['before']}), torch's peak {torch.cuda.max_memory_allocated()}")
    _arena.clear()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def engine():
    e = HipSearchEngine(device=0)
    yield e
    e.close()


class ArenaBatch:
    """A batch maker for ``both_fills`` (as ``device_batch``): the case's patch is written into the arena at its
    absolute offsets; ``restore`` sets the bytes back to 1. ``tail`` is accepted and ignored: the arena goes on."""

    def __init__(self):
        self.written = []

    def __call__(self, case, fill, tail=True, d=0):
        view = device_arena()
        at, letters = case.patch(fill)
        view[at:at + letters.shape[0]] = torch.from_numpy(letters).to(DEV)
        self.written.append((at, letters.shape[0]))
        h_offsets = case.offsets - d
        return view[d:], torch.from_numpy(h_offsets).to(DEV), h_offsets

    def restore(self):
        view = device_arena()
        for at, nb in self.written:
            view[at:at + nb] = 1
        self.written.clear()


ARENA_BATCH = ArenaBatch()


class DeviceBytes:
    """Byte slices of a device tensor as numpy arrays, for ``place_bits``."""

    def __init__(self, t):
        self.t = t

    def __getitem__(self, s):
        return self.t[s].cpu().numpy()

    def __setitem__(self, s, v):
        self.t[s] = torch.from_numpy(np.array(v, dtype=np.uint8)).to(self.t.device)  # a writable copy


def c0_of(name, placement, s=0, j=None):
    return far_c0(family_case(name).sub, placement, s, j)


def staging_placements(name):
    """[(c0, kw)] for a kernel that stages letters in granules: bit 31 and a high word at the residues FEW, the batch
    across 2^31 and 2^32 and with 2^32 inside a record, the base passed as a view once."""
    out = [(c0_of(name, p, s), {}) for p in ("bit31", "hi1") for s in FEW]
    out += [(c0_of(name, p), {}) for p in ("across31", "across32", "inside32")]
    return out + [(c0_of(name, "hi1", 13), dict(d=7))]


def rebasing_placements(name):
    out = [(c0_of(name, p, s), {}) for p, s in (("bit31", 0), ("hi1", 13), ("across32", 0), ("inside32", 0))]
    return out + [(c0_of(name, "hi1", 3), dict(d=7))]


def far_sweep(eng, name, sem, kernels, form, placements):
    for i, (c0, kw) in enumerate(placements(name)):
        solve_device_case(eng, name, sem, c0, 1 + i % 3, kernels, form, batch=ARENA_BATCH, **kw)


# ---- 1. solve_device on the arena --------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("name,form", SWIPE)
def test_swipe_lane_direct(engine, name, form, sem):
    """swipe_impl.hpp's lane-direct kernel: uniform64's two halves, the per-lane record offsets."""
    assert os.environ.get("MOC_SWIPE_DIRECT", "1") != "0"
    far_sweep(engine, name, sem, ["swipe"], form, staging_placements)
    far_sweep(engine, name + "_full", sem, ["swipe"], form, staging_placements)


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("name,form", [("short_pk", "short_pk"), ("short_key32", "short_key32"),
                                       ("short_key64", "short_key64")])
def test_short_kernel(engine, name, form, sem):
    """short_kernels.hip: ``base + offsets[i]`` behind ``a.codes = bv.codes - first_offset``."""
    far_sweep(engine, name, sem, ["short"], form, staging_placements)
    if name == "short_pk":
        far_sweep(engine, "short_full", sem, ["short"], form, staging_placements)


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("name,kernels,form", [("tile16", ["tile16"], "tile16"), ("tile16_i16", ["tile16"], "tile16_i16"),
                                               ("tiles_key64", ["tiles"], "tiles_key64"),
                                               ("tile16_window", ["tile16"], "tile16"),
                                               ("tile16_slide", ["tile16"], "tile16_slide")])
def test_tile_kernels(engine, name, kernels, form, sem):
    """The tile kernels' ``rec = bv.codes + (bv.offsets[r] - bv.offsets[0])``."""
    far_sweep(engine, name, sem, kernels, form, rebasing_placements)


def test_mfma_sweep(monkeypatch):
    monkeypatch.setenv("MOC_MFMA", "1")  # read when an engine starts
    eng = HipSearchEngine(device=0)
    try:
        for sem in SEMS:
            far_sweep(eng, "mfma", sem, ["tile16"], "mfma", rebasing_placements)
    finally:
        eng.close()


@pytest.mark.parametrize("sem", SEMS)
def test_mixed_slice(engine, sem):
    far_sweep(engine, "mixed", sem, ["short", "tile16"], "tile16", staging_placements)


# ---- 2. narrow results, context-parallel keys --------------------------------------------------------------------
def test_narrow_results(engine):
    for s, g in ((15, 1), (0, 3)):
        wire_device_case(engine, "swipe_r2", Semantics.REFERENCE, c0_of("swipe_r2", "hi1", s), g, "r2", ["swipe"],
                         batch=ARENA_BATCH)
        wire_device_case(engine, "swipe_w4", Semantics.REFERENCE, c0_of("swipe_w4", "hi1", s), g, "r4", ["swipe"],
                         batch=ARENA_BATCH)
        wire_device_case(engine, "short_pk", Semantics.REFERENCE, c0_of("short_pk", "hi1", s), g, "r4", ["short"],
                         batch=ARENA_BATCH)
    wire_device_case(engine, "swipe_r2", Semantics.REFERENCE, c0_of("swipe_r2", "across32"), 2, "r2", ["swipe"],
                     batch=ARENA_BATCH)


@pytest.mark.parametrize("name", ["tile16", "tile16_slide"])
def test_context_parallel_keys(engine, name):
    for i, (p, s) in enumerate((("bit31", 0), ("hi1", 13), ("bit31", 15), ("hi1", 1))):
        keys_case(engine, name, c0_of(name, p, s), 1 + i % 3, batch=ARENA_BATCH)


# ---- 3. the profile family ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_feature_device_forms(engine, sem):
    """The profile, report and per-target kernels' views (targets_pair.hpp) and the report's ``bv.offsets[r0] - base``."""
    feature_forms(engine, sem, [c0_of("profile", p) for p in ("bit31", "hi1", "inside32")], batch=ARENA_BATCH)


def test_feature_device_forms_in_chunks(engine):
    engine.set_profile_scratch(1 << 12)
    try:
        feature_forms(engine, Semantics.REFERENCE, [c0_of("profile", "hi1", 13)], chunked=True, batch=ARENA_BATCH)
    finally:
        engine.set_profile_scratch(256 << 20)


# ---- 4. device-resident wire batches at the packed placements ------------------------------------------------------
def packed_refs(sem):
    sub = family_case(PACKED_FAMILY).sub
    return sub, rows_of(PACKED_FAMILY, sem), oracle((PACKED_FAMILY, sem, "top3"), lambda: search_topk_cpu(sub, 3, sem))


def packed_solve_wire(eng, pc, ws, sparse, g):
    """solve_wire_device on the P33 run in the arena: dense offsets, or 64-record sparse ones plus base-6 lengths."""
    sub, view = pc.case.sub, device_arena()
    fmt = eng.auto_format(ws.l2_max, ws.l2_min) if sparse else "r4"
    dt = _lib.FORMAT_DTYPES[_lib.FORMAT_NAMES.index(fmt)]
    offs = np.ascontiguousarray((ws.sparse_offsets(6) if sparse else ws.offsets) + pc.case.c0)
    out = Guarded((sub.n, dt.itemsize), torch.uint8, g)
    lengths_t = torch.from_numpy(ws.lengths).to(DEV)
    torch.cuda.synchronize()  # a synchronous call on the engine's own stream: the run and the poison are in place
    narrow = dict(lengths_bits=ws.len_bits, lengths_base=ws.len_base, off_shift=6) if sparse else {}
    eng.solve_wire_device(view, torch.from_numpy(offs).to(DEV), lengths_t if sparse else None, sub.n, out.raw[out.lo:],
                          fmt, (ws.l2_min, ws.l2_max), packed33=True, **narrow)
    st = eng.stats()
    assert st["kernels"] == ["swipe"] and st["direct"] == 1 and st["format"] == fmt and st["h2d_bytes"] == 0, st
    res = np.ascontiguousarray(out.rows()).reshape(-1).view(dt)
    return as_triples(res, r2=eng.r2_params(ws.l2_min, ws.l2_max) if fmt == "r2" else None)


def packed_decode_topk(eng, pc, ws, sparse, g):
    """The decode kernels on the packed run in the arena, into guarded tensors, and solve_topk_device behind them."""
    sub, view, c0 = pc.case.sub, device_arena(), pc.case.c0
    total = int(sub.offsets[-1])
    shift = 6 if sparse else 0
    offs = np.ascontiguousarray((ws.sparse_offsets(6) if sparse else ws.offsets) + c0)
    offs_t, lengths_t = torch.from_numpy(offs).to(DEV), torch.from_numpy(ws.lengths).to(DEV)
    form = dict(n=sub.n, len_base=int(ws.len_base), packed={"p5": 1, "p33": 3}[pc.letters], off_shift=shift,
                len_bits=int(ws.len_bits))
    b = _lib.WireBatch(letters=view.data_ptr(), offsets=offs_t.data_ptr(), lengths=lengths_t.data_ptr(), device=1, **form)
    meta = _lib.WireBatch(letters=None, offsets=int(offs.ctypes.data), lengths=int(ws.lengths.ctypes.data), device=0, **form)
    codes, dense_g = Guarded((total, 1), torch.uint8, 16 * g + 1, behind=64), Guarded((sub.n + 1,), torch.int64, g)
    dense = eng.decode_wire_into(b, codes.out.view(-1), dense_g.out, host_meta=meta)
    assert np.array_equal(dense, pc.case.offsets)
    assert np.array_equal(dense_g.rows(), pc.case.offsets)
    assert not differing(codes.rows(), sub.codes.reshape(-1, 1)), differing(codes.rows(), sub.codes.reshape(-1, 1))
    # the decoded letters are the batch's alone: record i at codes[dense[i] - dense[0]]
    rel_t = dense_g.out - c0
    rows = Guarded((sub.n, 3, 3), torch.int32, g)
    eng.solve_topk_device(codes.out.view(-1), rel_t, sub.offsets, 3, rows.out)
    assert "profile" in eng.stats()["kernels"], eng.stats()
    return rows.rows()


@pytest.mark.parametrize("sem", SEMS)
def test_p33_wire_device(engine, sem):
    """wire_kernels.hip's and the lane-direct kernel's ``33 * f``, ``(33 * f0) >> 3``, ``(33 * f0) >> 5`` where the bit,
    the byte and the letter position pass 2^31 and 2^32, at the field phases 0, 3 and 6."""
    sub, want, top = packed_refs(sem)
    engine.set_problem(sub.weights, sub.seq1, sem)
    ws = WireSlice.from_csr(sub.codes, sub.offsets, letter_format="bytes")  # the narrow lengths and sparse offsets
    assert ws.len_bits == 6
    for i, (name, c0) in enumerate(packed_placements("p33")):
        pc, got = packed_case(PACKED_FAMILY, "p33", c0), {}
        for fill in FILLS:
            with torch.cuda.stream(side_stream()):
                b0, nb = pc.lay(DeviceBytes(device_arena()), fill)
                try:
                    res = [packed_solve_wire(engine, pc, ws, sparse, 1 + i % 3) for sparse in (False, True)]
                    res.append(packed_decode_topk(engine, pc, ws, i % 2 == 1, 1 + i % 3))
                finally:
                    device_arena()[b0:b0 + nb] = 1
            for r, w in zip(res, (want, want, top)):
                assert not differing(r, w), (name, fill, differing(r, w))
            got[fill] = res
        for x, y in zip(got["A"], got["continue"]):
            assert np.array_equal(x, y), name


def test_p5_wire_device(engine):
    """unpack5_kernel's ``5 * offset`` on host and device, at every letter index mod 8."""
    sem = Semantics.REFERENCE
    sub, want, top = packed_refs(sem)
    engine.set_problem(sub.weights, sub.seq1, sem)
    ws = WireSlice.from_csr(sub.codes, sub.offsets, letter_format="bytes")
    for i, (name, c0) in enumerate(packed_placements("p5")):
        pc, got = packed_case(PACKED_FAMILY, "p5", c0), {}
        for fill in FILLS:
            with torch.cuda.stream(side_stream()):
                b0, nb = pc.lay(DeviceBytes(device_arena()), fill)
                try:
                    got[fill] = packed_decode_topk(engine, pc, ws, i % 2 == 1, 1 + i % 3)
                finally:
                    device_arena()[b0:b0 + nb] = 1
            assert not differing(got[fill], top), (name, fill, differing(got[fill], top))
        assert np.array_equal(got["A"], got["continue"]), name


# ---- 5. the block-tiled swipe kernel from HBM: MOC_SWIPE_DIRECT is read once per process ----------------------------
def child_block_tiled():
    """Runs in a child process with MOC_SWIPE_DIRECT=0, on an arena of its own: grab() / fetch() carry a tile's start
    and end through LDS as 32-bit halves (misc[8..11]). The batches hold two 512-record tiles and a tail (a tile is a
    power of two of at most 512 records): with record 512 at the boundary it lies between two tiles, with record 549
    inside one, whose start and end then differ in the high word (2^32) or in bit 31 (2^31)."""
    assert os.environ["MOC_SWIPE_DIRECT"] == "0"
    eng = HipSearchEngine(device=0)
    ref = Semantics.REFERENCE
    for name, form in SWIPE[:2]:
        for sem in SEMS:
            cases = [(c0_of(name, p, s), {}) for p in ("bit31", "hi1") for s in (0, 13)]
            cases += [(c0_of(name, p, 0, j), {}) for p in ("across31", "across32") for j in (512, 549)]
            cases += [(c0_of(name, "inside32", 0, 512), {}), (c0_of(name, "inside32", 0, 549), {}),
                      (c0_of(name, "hi1", 15), dict(d=7))]
            for i, (c0, kw) in enumerate(cases):
                solve_device_case(eng, name, sem, c0, 1 + i % 3, ["swipe"], form, batch=ARENA_BATCH, **kw)
    for j in (512, 549):
        solve_device_case(eng, "swipe_w32_full", ref, c0_of("swipe_w32_full", "across32", 0, j), 1, ["swipe"], "swipe_rk",
                          batch=ARENA_BATCH)
    for p, j, g in (("hi1", None, 1), ("across32", 512, 3), ("across32", 549, 2), ("inside32", 549, 1), ("across31", 549, 2)):
        wire_device_case(eng, "swipe_r2", ref, c0_of("swipe_r2", p, 0, j), g, "r2", ["swipe"], batch=ARENA_BATCH)
        wire_device_case(eng, "swipe_w4", ref, c0_of("swipe_w4", p, 0, j), g, "r4", ["swipe"], batch=ARENA_BATCH)
    # P33 letters through the block-tiled kernel (what a host stream runs), at the packed placements
    sub, want, _ = packed_refs(ref)
    eng.set_problem(sub.weights, sub.seq1, ref)
    ws = WireSlice.from_csr(sub.codes, sub.offsets, letter_format="bytes")
    for i, (name, c0) in enumerate(packed_placements("p33")):
        pc = packed_case(PACKED_FAMILY, "p33", c0)
        with torch.cuda.stream(side_stream()):
            b0, nb = pc.lay(DeviceBytes(device_arena()), FILLS[i % 2])
            try:
                got = packed_solve_wire(eng, pc, ws, i % 3 != 0, 1 + i % 3)
            finally:
                device_arena()[b0:b0 + nb] = 1
        assert not differing(got, want), (name, differing(got, want))
    eng.close()


def test_swipe_block_tiled_device():
    torch.cuda.synchronize()
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_far_offsets as m; m.child_block_tiled(); print('ok')" % (
        os.path.join(ROOT, "tests"), ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=300,
                       env=dict(os.environ, MOC_SWIPE_DIRECT="0"))
    for line in r.stdout.decode(errors="replace").splitlines():
        if "MOC_DCHECK" in line:  # a bounds-checked library's reports (tools/dcheck.sh counts them)
            print(line)
    assert r.returncode == 0 and b"ok" in r.stdout, (r.stdout.decode()[-2000:], r.stderr.decode()[-4000:])


# ---- 6. host forms on an anonymous mapping of the arena's layout ---------------------------------------------------
@pytest.fixture(scope="module")
def host(request):
    """(engine of 100-record chunks, arena, view). The landing windows hold letter 1 and are page-locked for the
    engine's lifetime; the mapping as a whole is never touched or locked."""
    if request.session.testsfailed:
        pytest.fail("the host forms run only after every earlier test (their device-resident twins) has passed")
    eng = HipSearchEngine(device=0, chunk_records=100)
    arena, view = host_arena()
    eng.pin(*(arena[lo:lo + nb] for lo, nb in LANDING))
    yield eng, arena, view
    eng.close()


def pages_of(view, at, nb):
    """The whole pages of view[at:at + nb] (the view starts on a page boundary)."""
    lo, hi = at & ~4095, (at + nb + 4095) & ~4095
    return view[lo:hi]


def own_pages(dtype, count):
    nbytes = max(int(count) * np.dtype(dtype).itemsize, 1)
    return np.frombuffer(mmap.mmap(-1, (nbytes + 4095) & ~4095), dtype=dtype, count=int(count))


HOST_PLACEMENTS = (("bit31", 13, None), ("hi1", 15, None), ("across32", 0, None), ("inside32", 0, None))


def test_host_staged_pipeline(host):
    """run_staged's ``pb0`` / ``pb1`` and per-chunk rebasing: eng.solve(view, offsets) in 100-record chunks, from
    pageable pages and from page-locked ones (the letters alone: offsets and results are pageable, so the batch is
    staged and its pieces go through launch_copy)."""
    eng, arena, view = host
    sub = family_case("host").sub
    want = rows_of("host", Semantics.REFERENCE)
    eng.set_problem(sub.weights, sub.seq1)
    for p, s, j in HOST_PLACEMENTS:
        case = family_case("host", c0_of("host", p, s, j))
        got = {}
        for fill in FILLS:
            at, nb = lay(view, case, fill)
            res = [as_triples(eng.solve(view, case.offsets))]
            st = eng.stats()
            assert st["chunks"] >= 3 and st["direct"] == 0 and st["records"] == sub.n, st
            with _lib.Pinned(pages_of(view, at, nb)):
                res.append(as_triples(eng.solve(view, case.offsets)))
                st = eng.stats()
                assert st["chunks"] >= 3 and st["direct"] == 0 and st["records"] == sub.n, st
            unlay(view, at, nb)
            for r in res:
                assert not differing(r, want), (p, fill, differing(r, want))
            got[fill] = res
        assert all(np.array_equal(x, y) for x, y in zip(got["A"], got["continue"])), p


@pytest.mark.parametrize("fmt", ["r12", "r8", "r4"])
def test_host_swipe_zero_copy(host, fmt):
    """The block-tiled swipe kernel streaming page-locked host letters (2048-record tiles: record 2048 at the
    boundary lies between two tiles, the middle record inside one)."""
    eng, arena, view = host
    dt = _lib.FORMAT_DTYPES[_lib.FORMAT_NAMES.index(fmt)]
    name = "swipe_w4_host"
    sub = family_case(name).sub
    want = rows_of(name, Semantics.REFERENCE)
    eng.set_problem(sub.weights, sub.seq1)
    offsets, out = own_pages(np.int64, sub.n + 1), own_pages(dt, sub.n + 6)
    with _lib.Pinned(offsets, out):
        for i, (p, s, j) in enumerate(HOST_PLACEMENTS + (("across32", 0, 2048), ("across31", 0, 2048))):
            case, g = family_case(name, c0_of(name, p, s, j)), 1 + i % 3
            got = {}
            for fill in FILLS:
                at, nb = lay(view, case, fill)
                offsets[:] = case.offsets
                out.view(np.uint8)[:] = POISON
                with _lib.Pinned(pages_of(view, at, nb)):
                    eng.solve(view, offsets, out=out[g:g + sub.n], fmt=fmt)
                    st = eng.stats()
                unlay(view, at, nb)
                assert st["direct"] == 1 and st["kernels"] == ["swipe"], st
                raw = out.view(np.uint8).reshape(sub.n + 6, dt.itemsize)
                assert (raw[:g] == POISON).all() and (raw[g + sub.n:] == POISON).all(), (fmt, p, fill)
                got[fill] = as_triples(out[g:g + sub.n]).copy()
                assert not differing(got[fill], want), (fmt, p, fill, differing(got[fill], want))
            assert np.array_equal(got["A"], got["continue"])


def test_host_short_zero_copy_base6(host):
    """The short kernel streaming page-locked host letters with base-6 lengths."""
    eng, arena, view = host
    name = "short_full"
    sub = family_case(name).sub
    want = rows_of(name, Semantics.REFERENCE)
    eng.set_problem(sub.weights, sub.seq1)
    ws = WireSlice.from_csr(sub.codes, sub.offsets, letter_format="bytes", alloc=lambda n_, d, c: own_pages(d, c))
    assert ws.len_bits == 6
    dt = _lib.FORMAT_DTYPES[_lib.FORMAT_NAMES.index("r4")]
    out = own_pages(dt, sub.n + 6)
    with _lib.Pinned(ws.offsets, ws.lengths, out):
        for i, (p, s, j) in enumerate(HOST_PLACEMENTS):
            case, g = family_case(name, c0_of(name, p, s, j)), 1 + i % 3
            for fill in FILLS:
                at, nb = lay(view, case, fill)
                ws.offsets[:] = case.offsets
                out.view(np.uint8)[:] = POISON
                with _lib.Pinned(pages_of(view, at, nb)):
                    eng.solve(view, ws.offsets, out=out[g:g + sub.n], lengths=ws.lengths, fmt="r4",
                              l2_range=(ws.l2_min, ws.l2_max), lengths_bits=6, lengths_base=ws.len_base)
                    st = eng.stats()
                unlay(view, at, nb)
                assert st["direct"] == 1 and st["kernels"] == ["short"], st
                raw = out.view(np.uint8).reshape(sub.n + 6, dt.itemsize)
                assert (raw[:g] == POISON).all() and (raw[g + sub.n:] == POISON).all(), (p, fill)
                got = as_triples(out[g:g + sub.n])
                assert not differing(got, want), (p, fill, differing(got, want))


def test_host_p33_zero_copy(host):
    """P33 letters streamed zero-copy from page-locked host memory at the packed placements (direct_pointers' ``b0`` /
    ``b1``, the streaming kernel's field arithmetic)."""
    eng, arena, view = host
    sub, want, _ = packed_refs(Semantics.REFERENCE)
    eng.set_problem(sub.weights, sub.seq1)
    ws = WireSlice.from_csr(sub.codes, sub.offsets, letter_format="bytes", alloc=lambda n_, d, c: own_pages(d, c))
    fmt = eng.auto_format(ws.l2_max, ws.l2_min)
    dt = _lib.FORMAT_DTYPES[_lib.FORMAT_NAMES.index(fmt)]
    out = own_pages(dt, sub.n + 6)
    r2 = eng.r2_params(ws.l2_min, ws.l2_max) if fmt == "r2" else None
    with _lib.Pinned(ws.offsets, ws.lengths, out):
        for i, (name, c0) in enumerate(packed_placements("p33")):
            pc, g, got = packed_case(PACKED_FAMILY, "p33", c0), 1 + i % 3, {}
            for fill in FILLS:
                b0, nb = pc.lay(view, fill)
                ws.offsets[:] = pc.case.offsets
                out.view(np.uint8)[:] = POISON
                with _lib.Pinned(pages_of(view, b0, nb)):
                    eng.solve(view, ws.offsets, out=out[g:g + sub.n], lengths=ws.lengths, fmt=fmt,
                              l2_range=(ws.l2_min, ws.l2_max), packed33=True, lengths_bits=6, lengths_base=ws.len_base)
                    st = eng.stats()
                view[b0:b0 + nb] = 1
                assert st["direct"] == 1 and st["kernels"] == ["swipe"], st
                raw = out.view(np.uint8).reshape(sub.n + 6, dt.itemsize)
                assert (raw[:g] == POISON).all() and (raw[g + sub.n:] == POISON).all(), (name, fill)
                got[fill] = as_triples(out[g:g + sub.n], r2=r2).copy()
                assert not differing(got[fill], want), (name, fill, differing(got[fill], want))
            assert np.array_equal(got["A"], got["continue"]), name


def test_host_p5_staged(host):
    """5-bit letters through the staged pipeline (run_staged's ``pbit``, launch_unpack5's bit phase) at every letter
    index mod 8 past each boundary."""
    eng, arena, view = host
    sub, want, _ = packed_refs(Semantics.REFERENCE)
    eng.set_problem(sub.weights, sub.seq1)
    for name, c0 in packed_placements("p5"):
        pc, got = packed_case(PACKED_FAMILY, "p5", c0), {}
        for fill in FILLS:
            b0, nb = pc.lay(view, fill)
            got[fill] = as_triples(eng.solve(view, pc.case.offsets, packed5=True))
            st = eng.stats()
            view[b0:b0 + nb] = 1
            assert st["direct"] == 0 and st["chunks"] >= 3 and st["kernels"] == ["swipe"], st
            assert not differing(got[fill], want), (name, fill, differing(got[fill], want))
        assert np.array_equal(got["A"], got["continue"]), name


def test_host_profile_forms(host):
    """The profile-family host forms of test_gpu_csr_slices.test_host_forms on offsets[a : b + 1] of far placements."""
    eng, arena, view = host
    full = family_case("host").sub
    a, b = 17, full.n - 9
    lo = int(full.offsets[a])
    sub = Problem(full.weights, full.seq1, full.codes[lo:int(full.offsets[b])].copy(), full.offsets[a:b + 1] - lo)
    ts = TargetSet(sub.seq1, [0, 40, sub.L1])
    eng.set_problem(sub.weights, sub.seq1)
    w_top = search_topk_cpu(sub, 3)
    w_rows, w_hoff = search_hits_cpu(sub, within=20)
    w_summ, w_hist = search_summary_cpu(sub, BINS, LO, WIDTH)
    w_trows = search_targets_cpu(sub, ts)
    w_tsumm, w_thist = search_targets_summary_cpu(sub, ts, BINS, LO, WIDTH)
    for p, s, j in HOST_PLACEMENTS:
        case = family_case("host", c0_of("host", p, s, j))
        offsets = case.offsets[a:b + 1]
        got = {}
        for fill in FILLS:
            at, nb = lay(view, case, fill)
            res = [eng.solve_topk(view, offsets, 3)]
            assert "profile" in eng.stats()["kernels"]
            rows, hoff = eng.solve_hits(view, offsets, within=20)
            assert "hits" in eng.stats()["kernels"]
            summ, hist = eng.solve_summary(view, offsets, BINS, LO, WIDTH)
            assert "summary" in eng.stats()["kernels"]
            res += [rows, hoff, summ, hist, eng.solve_targets(view, offsets, ts)]
            assert "targets" in eng.stats()["kernels"]
            res += list(eng.solve_targets_summary(view, offsets, ts, BINS, LO, WIDTH))
            assert "targets_summary" in eng.stats()["kernels"]
            unlay(view, at, nb)
            for x, w in zip(res, (w_top, w_rows, w_hoff, w_summ, w_hist, w_trows, w_tsumm, w_thist)):
                assert np.array_equal(x, w), (p, fill)
            got[fill] = res
        assert all(np.array_equal(x, y) for x, y in zip(got["A"], got["continue"])), p
