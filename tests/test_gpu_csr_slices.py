"""GPU (MI355X / gfx950) tests of the device ABI's slice contract: a batch may be a slice of a larger CSR array —
absolute offsets with any first offset, record i at ``codes[offsets[i]]``, letters at any byte alignment, outputs at
the natural alignment of their element type — and nothing outside the slice is read into a result or written.

Every case lays a family's records (tests/csr_slices.py; the shapes that select each kernel in tests/test_gpu.py)
behind ``c0`` neighbour letters, in two neighbour fills of valid letters, and asserts that
  * the rows equal the CPU engine's on the slice alone (offsets from 0),
  * they are bit-identical between the two fills,
  * the poisoned rows in front of and behind the output slice are untouched, byte for byte,
  * ``stats()`` names the kernel (and arithmetic form) the case means to cover.
The kernels that stage letters in 16-byte granules or 4-byte words (both swipe kernels, the short kernel) run at all
sixteen residues of ``(base + offsets[0]) mod 16`` and with every record at the batch's longest length behind a
15-byte head; the others, which read letters byte by byte, at a few first offsets (what is under test there is the
rebasing). tests/test_csr_slices_fixture.py shows on the CPU that these inputs tell a leak from none."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, gpu_available
from csr_slices import FILLS, TARGET_LENS, family_case

pytestmark = pytest.mark.gpu

if not gpu_available():  # pragma: no cover - collected on CPU hosts only with -m gpu
    pytest.skip("no GPU", allow_module_level=True)

import torch  # noqa: E402

from mpi_openmp_cuda_amd import (HipSearchEngine, Problem, Semantics, TargetSet, _lib, search_cpu,  # noqa: E402
                                 search_hits_cpu, search_profile_cpu, search_report_cpu, search_summary_cpu,
                                 search_targets_cpu, search_targets_hits_cpu, search_targets_rank_cpu,
                                 search_targets_summary_cpu, search_targets_topk_cpu, search_topk_cpu)
from mpi_openmp_cuda_amd.ops.align import as_triples  # noqa: E402

DEV = torch.device("cuda:0")
SEMS = [Semantics.REFERENCE, Semantics.SPEC]
POISON = 0x5A  # every guard byte: int32 rows read 0x5A5A5A5A
ALL16 = tuple(range(16))
FEW = (0, 1, 3, 13, 15)
FAR = 3 * 65536 + 13  # a first offset past 16 bits: narrow or truncated offset arithmetic
NP_OF = {torch.int32: np.int32, torch.int64: np.int64, torch.uint8: np.uint8}


@pytest.fixture(scope="module")
def engine():
    e = HipSearchEngine(device=0)
    yield e
    e.close()


_oracle = {}


def oracle(key, fn):
    """A CPU-engine result, computed once per key and read-only afterwards."""
    if key not in _oracle:
        v = fn()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _oracle[key] = v
    return _oracle[key]


def rows_of(name, sem):
    return oracle((name, sem, "rows"), lambda: as_triples(search_cpu(family_case(name).sub, sem)))


class Guarded:
    """A device output of ``shape`` = (n, ...) as rows g .. g + n of a larger buffer filled with the poison."""

    def __init__(self, shape, dtype, g, behind=3):
        self.shape, self.dtype, self.g = tuple(int(x) for x in shape), dtype, int(g)
        self.row = torch.empty(0, dtype=dtype).element_size() * int(np.prod(self.shape[1:], dtype=np.int64))
        self.lo, self.hi = self.g * self.row, (self.g + self.shape[0]) * self.row
        self.raw = torch.full((self.hi + behind * self.row,), POISON, dtype=torch.uint8, device=DEV)
        assert self.raw.data_ptr() % 16 == 0
        self.out = self.raw[self.lo:self.hi].view(dtype).view(self.shape)
        assert self.out.data_ptr() == self.raw.data_ptr() + self.lo and self.out.is_contiguous()

    def rows(self):
        """After a sync: the guards hold the poison; returns the slice as numpy."""
        torch.cuda.synchronize()
        b = self.raw.cpu().numpy()
        front, back = np.flatnonzero(b[:self.lo] != POISON), np.flatnonzero(b[self.hi:] != POISON)
        assert front.size == 0, f"{front.size} guard bytes in front of the output were written, first at -{self.lo - front[0]}"
        assert back.size == 0, f"{back.size} guard bytes behind the output were written, first at +{back[0]}"
        return b[self.lo:self.hi].view(NP_OF[self.dtype]).reshape(self.shape)


def device_batch(case, fill, tail=True, d=0):
    """The storage on the device -> (codes_t, offsets_t, h_offsets): the base is the storage itself, or with ``d`` a
    view ``storage_t[d:]`` with the offsets reduced by ``d`` (the same letters at the same addresses)."""
    st = torch.from_numpy(case.storage(fill, tail)).to(DEV)
    assert st.data_ptr() % 16 == 0  # so (base + offsets[0]) mod 16 is c0 mod 16
    h_offsets = case.offsets - d
    return st[d:], torch.from_numpy(h_offsets).to(DEV), h_offsets


def differing(got, want):
    bad = np.flatnonzero((np.asarray(got) != np.asarray(want)).reshape(len(want), -1).any(axis=1))
    return "" if bad.size == 0 else f"{bad.size} of {len(want)} rows differ, first {bad[:6].tolist()}: got " \
                                    f"{np.asarray(got)[bad[:3]].tolist()} want {np.asarray(want)[bad[:3]].tolist()}"


_side = []


def side_stream():
    """The stream of every device-form case: uploads, poison fills, the engine's launches and torch's own operations
    are ordered on it. (torch's default stream stands for the engine's own compute stream, which torch's operations
    on the default stream are not ordered with.)"""
    if not _side:
        _side.append(torch.cuda.Stream(DEV))
    return _side[0]


def both_fills(case, want, run, batch=device_batch, **kw):
    """run(codes_t, offsets_t, h_offsets) -> rows, for both neighbour fills: equal to ``want`` and to each other.
    ``batch``: what lays the case on the device, ``device_batch`` or a maker of the same signature (whose ``restore``,
    if it has one, runs after each fill)."""
    got = {}
    for fill in FILLS:
        with torch.cuda.stream(side_stream()):
            try:
                got[fill] = run(*batch(case, fill, **kw))
            finally:
                getattr(batch, "restore", lambda: None)()
        msg = differing(got[fill], want)
        assert not msg, f"c0 {case.c0} fill {fill} {kw}: {msg}"
    assert np.array_equal(got["A"], got["continue"])
    return got["A"]


def solve_device_case(eng, name, sem, c0, g, kernels, form, **kw):
    """solve_device on the family's slice at ``c0`` into rows g.. of a poisoned tensor."""
    case, want = family_case(name, c0), rows_of(name, sem)
    eng.set_problem(case.sub.weights, case.sub.seq1, sem)

    def run(codes_t, offs_t, h_offs):
        out = Guarded((case.sub.n, 3), torch.int32, g)
        eng.solve_device(codes_t, offs_t, h_offs, out.out)
        st = eng.stats()
        assert st["kernels"] == kernels and (form is None or form in st["forms"]), st
        return out.rows()

    both_fills(case, want, run, **kw)


def wire_device_case(eng, name, sem, c0, g, fmt, kernels, **kw):
    """solve_wire_device (byte letters, dense offsets) into ``big_u8[fb * g:]``: R2 results from an odd element on
    are 2-byte aligned, R4 ones 4-byte aligned and off the 16-byte boundary."""
    case, want = family_case(name, c0), rows_of(name, sem)
    eng.set_problem(case.sub.weights, case.sub.seq1, sem)
    dt = _lib.FORMAT_DTYPES[_lib.FORMAT_NAMES.index(fmt)]
    lens = np.diff(case.offsets)
    l2 = (int(lens.min()), int(lens.max()))

    def run(codes_t, offs_t, h_offs):
        out = Guarded((case.sub.n, dt.itemsize), torch.uint8, g)
        torch.cuda.synchronize()  # a synchronous call on the engine's own stream: the poison is in place first
        eng.solve_wire_device(codes_t, offs_t, None, case.sub.n, out.raw[out.lo:], fmt, l2, packed33=False)
        st = eng.stats()
        assert st["kernels"] == kernels and st["direct"] == 1 and st["format"] == fmt, st
        res = np.ascontiguousarray(out.rows()).reshape(-1).view(dt)
        return as_triples(res, r2=eng.r2_params(*l2) if fmt == "r2" else None)

    both_fills(case, want, run, **kw)


def staging_sweep(eng, name, full, sem, kernels, form):
    """A staging kernel's cases: every residue of the first letter's address, the far first offset, the base passed
    as a view, a storage that ends at the slice's last letter, and (``full``) the batch of longest records behind a
    15-byte and a 0-byte head."""
    for s in ALL16:
        solve_device_case(eng, name, sem, 32 + s, 1 + s % 3, kernels, form)
    solve_device_case(eng, name, sem, FAR, 2, kernels, form)
    for d in (1, 7):
        solve_device_case(eng, name, sem, 32 + 13, 1, kernels, form, d=d)
    solve_device_case(eng, name, sem, 32 + 15, 3, kernels, form, tail=False)
    for s in (15, 0) if full else ():
        solve_device_case(eng, full, sem, 32 + s, 1, kernels, form)
        solve_device_case(eng, full, sem, 32 + s, 2, kernels, form, tail=False)


# ---- 1. swipe, lane-direct (the default for device-resident byte letters) --------------------------------------
SWIPE = [("swipe_w4", "swipe_kbits"), ("swipe_w16", "swipe_rk"), ("swipe_w32", "swipe_rk")]


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("name,form", SWIPE)
def test_swipe_lane_direct(engine, name, form, sem):
    assert os.environ.get("MOC_SWIPE_DIRECT", "1") != "0"
    staging_sweep(engine, name, name + "_full", sem, ["swipe"], form)


@pytest.mark.parametrize("fmt,name,gs", [("r2", "swipe_r2", (1, 3)), ("r4", "swipe_w4", (1, 2, 3))])
def test_swipe_lane_direct_narrow_results(engine, fmt, name, gs):
    for s, g in zip((15, 1, 8), gs):
        wire_device_case(engine, name, Semantics.REFERENCE, 32 + s, g, fmt, ["swipe"])


# ---- 2a. swipe, block-tiled, device-resident: MOC_SWIPE_DIRECT is read once per process --------------------------
def child_block_tiled():
    """Runs in a child process with MOC_SWIPE_DIRECT=0: the block-tiled kernel's fetch() at every residue, and its
    copy_results to outputs off the 16-byte boundary (R12 rows), at an odd R2 element and at R4 elements."""
    assert os.environ["MOC_SWIPE_DIRECT"] == "0"
    eng = HipSearchEngine(device=0)
    for name, form in SWIPE[:2]:
        for sem in SEMS:
            staging_sweep(eng, name, name + "_full", sem, ["swipe"], form)
    for s in (15, 0):
        solve_device_case(eng, "swipe_w32_full", Semantics.REFERENCE, 32 + s, 1, ["swipe"], "swipe_rk")
    for s, g in ((15, 1), (4, 3), (9, 2)):
        wire_device_case(eng, "swipe_r2", Semantics.REFERENCE, 32 + s, g, "r2", ["swipe"])
        wire_device_case(eng, "swipe_w4", Semantics.REFERENCE, 32 + s, g, "r4", ["swipe"])
    wire_device_case(eng, "swipe_w4_full", Semantics.REFERENCE, 32 + 15, 1, "r4", ["swipe"], tail=False)
    eng.close()


def test_swipe_block_tiled_device():
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_csr_slices as m; m.child_block_tiled(); print('ok')" % (
        os.path.join(ROOT, "tests"), ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=300,
                       env=dict(os.environ, MOC_SWIPE_DIRECT="0"))
    for line in r.stdout.decode(errors="replace").splitlines():
        if "MOC_DCHECK" in line:  # a bounds-checked library's reports (tools/dcheck.sh counts them)
            print(line)
    assert r.returncode == 0 and b"ok" in r.stdout, (r.stdout.decode()[-2000:], r.stderr.decode()[-4000:])


# ---- 2b. swipe, block-tiled, zero-copy from page-locked host memory ---------------------------------------------
@pytest.mark.parametrize("fmt", ["r12", "r8", "r4"])
def test_swipe_zero_copy_host(fmt):
    dt = _lib.FORMAT_DTYPES[_lib.FORMAT_NAMES.index(fmt)]
    eng = HipSearchEngine(device=0)
    try:
        for name, shifts in (("swipe_w4_host", ALL16), ("swipe_w16_host_full", (15, 0))):
            sub = family_case(name).sub
            want = rows_of(name, Semantics.REFERENCE)
            eng.set_problem(sub.weights, sub.seq1)
            # one page-locked letter buffer, offset array and result array for every shift
            buf = np.ones(64 + 32 + 15 + int(sub.offsets[-1]) + 64, np.uint8)
            a0 = (-buf.ctypes.data) % 16  # buf[a0] lies on a 16-byte boundary
            offsets = np.zeros(sub.n + 1, np.int64)
            out = np.zeros(sub.n + 6, dt)
            eng.pin(buf, offsets, out)
            for s in shifts:
                case, g = family_case(name, 32 + s), 1 + s % 3
                got = {}
                for fill in FILLS:
                    st = case.storage(fill)
                    buf[:] = 1
                    buf[a0:a0 + st.shape[0]] = st
                    offsets[:] = case.offsets
                    out.view(np.uint8)[:] = POISON
                    eng.solve(buf[a0:], offsets, out=out[g:g + sub.n], fmt=fmt)
                    stats = eng.stats()
                    assert stats["direct"] == 1 and stats["kernels"] == ["swipe"], stats
                    raw = out.view(np.uint8).reshape(sub.n + 6, dt.itemsize)
                    assert (raw[:g] == POISON).all() and (raw[g + sub.n:] == POISON).all(), (fmt, s, fill)
                    got[fill] = as_triples(out[g:g + sub.n]).copy()
                    assert not differing(got[fill], want), (fmt, s, fill, differing(got[fill], want))
                assert np.array_equal(got["A"], got["continue"])
    finally:
        eng.close()


# ---- 3. short kernel --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("name,form", [("short_pk", "short_pk"), ("short_key32", "short_key32"),
                                       ("short_key64", "short_key64")])
def test_short_kernel(engine, name, form, sem):
    full = "short_full" if name == "short_pk" else None  # the uniform batch: L1 150, every record 150 letters
    staging_sweep(engine, name, full, sem, ["short"], form)


def test_short_kernel_r4_results(engine):
    for s, g in ((15, 1), (6, 2), (0, 3)):
        wire_device_case(engine, "short_pk", Semantics.REFERENCE, 32 + s, g, "r4", ["short"])
    wire_device_case(engine, "short_full", Semantics.REFERENCE, 32 + 15, 1, "r4", ["short"], tail=False)


# ---- 4. tile kernels --------------------------------------------------------------------------------------------
def rebasing_sweep(eng, name, sem, kernels, form):
    for i, s in enumerate(FEW):
        solve_device_case(eng, name, sem, 32 + s, 1 + i % 3, kernels, form)
    solve_device_case(eng, name, sem, FAR, 2, kernels, form)
    solve_device_case(eng, name, sem, 32 + 13, 3, kernels, form, d=7)
    solve_device_case(eng, name, sem, 32 + 15, 1, kernels, form, tail=False)


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("name,kernels,form", [("tile16", ["tile16"], "tile16"), ("tile16_i16", ["tile16"], "tile16_i16"),
                                               ("tiles_key64", ["tiles"], "tiles_key64"),
                                               ("tile16_window", ["tile16"], "tile16"),
                                               ("tile16_slide", ["tile16"], "tile16_slide")])
def test_tile_kernels(engine, name, kernels, form, sem):
    rebasing_sweep(engine, name, sem, kernels, form)


def test_mfma_sweep(monkeypatch):
    monkeypatch.setenv("MOC_MFMA", "1")  # read when an engine starts
    eng = HipSearchEngine(device=0)
    try:
        for sem in SEMS:
            rebasing_sweep(eng, "mfma", sem, ["tile16"], "mfma")
    finally:
        eng.close()


# ---- 5. a mixed slice: short-kernel and tile16 records interleaved in one call -----------------------------------
@pytest.mark.parametrize("sem", SEMS)
def test_mixed_slice(engine, sem):
    for i, s in enumerate(ALL16):
        solve_device_case(engine, "mixed", sem, 32 + s, 1 + i % 3, ["short", "tile16"], "tile16")
    solve_device_case(engine, "mixed", sem, FAR, 2, ["short", "tile16"], "tile16")
    solve_device_case(engine, "mixed", sem, 32 + 13, 1, ["short", "tile16"], "tile16", d=1)


# ---- 6. context-parallel keys -----------------------------------------------------------------------------------
def keys_case(engine, name, c0, g, **kw):
    """search_keys_device over two parts, their uint64 maximum, finalize_keys_device: the rows of ``solve_device``."""
    want = rows_of(name, Semantics.REFERENCE)
    flip = torch.tensor(-2**63, dtype=torch.int64, device=DEV)
    case = family_case(name, c0)
    n = case.sub.n
    engine.set_problem(case.sub.weights, case.sub.seq1)

    def run(codes_t, offs_t, h_offs):
        parts = []
        for part in range(2):
            keys = Guarded((n,), torch.int64, 1)  # 8-byte aligned, off the 16-byte boundary
            engine.search_keys_device(codes_t, offs_t, h_offs, part, 2, keys.out)
            st = engine.stats()
            assert "tile16" in st["kernels"] and "tile16" in st["forms"], st
            keys.rows()
            parts.append(keys.out)
        best = torch.stack([p ^ flip for p in parts]).max(dim=0).values ^ flip  # uint64 max
        out = Guarded((n, 3), torch.int32, g)
        engine.finalize_keys_device(codes_t, offs_t, h_offs, best, out.out)
        return out.rows()

    both_fills(case, want, run, **kw)


@pytest.mark.parametrize("name", ["tile16", "tile16_slide"])
def test_context_parallel_keys(engine, name):
    for i, s in enumerate(FEW + (FAR - 32,)):
        keys_case(engine, name, 32 + s, 1 + i % 3, d=1 if s == 13 else 0)


# ---- 7. feature kernels, device forms: the tile-edge batch of tests/test_gpu_topk.py ------------------------------
FEATURE = "profile"
BINS, LO, WIDTH = 8, -300, 200


def feature_sub():
    return family_case(FEATURE).sub


def targets_of(sub):
    assert sum(TARGET_LENS) == sub.L1 and max(np.diff(sub.offsets)) > TARGET_LENS[0]
    return TargetSet(sub.seq1, [0, TARGET_LENS[0], sub.L1])


def feature_forms(eng, sem, shifts, chunked=False, batch=device_batch):
    """Every device form of the profile family at the first offsets ``shifts``: 32 + s for a small s, the offset
    itself from FAR on."""
    sub = feature_sub()
    n, total = sub.n, int(sub.offsets[-1])
    ts = targets_of(sub)
    key = (FEATURE, sem)
    prof, po = oracle(key + ("prof",), lambda: search_profile_cpu(sub, sem))
    top = {r: oracle(key + ("top", r), lambda: search_topk_cpu(sub, 3, sem, radius=r)) for r in (0, 1)}
    hits, ho = oracle(key + ("hits",), lambda: search_hits_cpu(sub, within=20, semantics=sem))
    summ, hist = oracle(key + ("summary",), lambda: search_summary_cpu(sub, BINS, LO, WIDTH, sem))
    trows = oracle(key + ("targets",), lambda: search_targets_cpu(sub, ts, sem))
    tsumm, thist = oracle(key + ("tsummary",), lambda: search_targets_summary_cpu(sub, ts, BINS, LO, WIDTH, sem))
    ttop = {r: oracle(key + ("ttop", r), lambda: search_targets_topk_cpu(sub, ts, 3, sem, radius=r)) for r in (0, 1)}
    thits = {r: oracle(key + ("thits", r), lambda: search_targets_hits_cpu(sub, ts, within=20, semantics=sem, radius=r))
             for r in (0, 1)}
    trank = oracle(key + ("trank",), lambda: search_targets_rank_cpu(sub, ts, 2, sem))
    best = rows_of(FEATURE, sem)
    counts1, marks1 = oracle(key + ("report1",), lambda: search_report_cpu(sub, best, marks=True))
    counts3, marks3 = oracle(key + ("report3",), lambda: search_report_cpu(sub, top[0], marks=True))
    eng.set_problem(sub.weights, sub.seq1, sem)

    def ran(*kernels):
        st = eng.stats()
        assert all(k in st["kernels"] for k in kernels) and (not chunked or st["chunks"] > 1), st

    for i, s in enumerate(shifts):
        case = family_case(FEATURE, 32 + s if s < FAR else s)
        g = 1 + i % 3
        kw = dict(batch=batch, **(dict(d=7) if s == 13 else {}))

        def profile(c, o, h):
            out = Guarded((len(prof), 2), torch.int32, g)
            _, got_po = eng.solve_profile_device(c, o, h, out.out)
            ran("profile")
            assert np.array_equal(got_po, po)
            return out.rows()

        if not chunked:  # the whole profile is one chunk by definition
            both_fills(case, prof.view(np.int32).reshape(-1, 2), profile, **kw)

        for radius in (0, 1):
            def topk(c, o, h):
                out = Guarded((n, 3, 3), torch.int32, g)
                eng.solve_topk_device(c, o, h, 3, out.out, radius=radius)
                ran("profile", *(["peaks"] if radius else []))
                return out.rows()

            both_fills(case, top[radius], topk, **kw)

        def hits_(c, o, h):
            rows = Guarded((len(hits), 3), torch.int32, g)
            hoff = Guarded((n + 1,), torch.int64, 1)
            eng.solve_hits_device(c, o, h, within=20, cap=len(hits), rows_t=rows.out, hoffsets_t=hoff.out)
            ran("profile", "hits")
            assert np.array_equal(hoff.rows(), ho)
            return rows.rows()

        both_fills(case, hits, hits_, **kw)

        def summary(c, o, h):
            s_out, h_out = Guarded((n, 7), torch.int64, g), Guarded((n, BINS), torch.int32, g)
            eng.solve_summary_device(c, o, h, BINS, LO, WIDTH, s_out.out, h_out.out)
            ran("profile", "summary")
            assert np.array_equal(h_out.rows(), hist)
            return s_out.rows()

        both_fills(case, summ, summary, **kw)

        def targets(c, o, h):
            out = Guarded((n, ts.T, 3), torch.int32, g)
            eng.solve_targets_device(c, o, h, ts, out.out)
            ran("profile", "targets")
            return out.rows()

        both_fills(case, trows, targets, **kw)

        def targets_summary(c, o, h):
            s_out, h_out = Guarded((n, ts.T, 7), torch.int64, g), Guarded((n, ts.T, BINS), torch.int32, g)
            eng.solve_targets_summary_device(c, o, h, ts, BINS, LO, WIDTH, s_out.out, h_out.out)
            ran("profile", "targets_summary")
            assert np.array_equal(h_out.rows(), thist)
            return s_out.rows()

        both_fills(case, tsumm, targets_summary, **kw)

        for radius in (0, 1):
            peaks = ["targets_peaks"] if radius else []

            def targets_topk(c, o, h):
                out = Guarded((n, ts.T, 3, 3), torch.int32, g)
                eng.solve_targets_topk_device(c, o, h, ts, 3, out.out, radius=radius)
                ran("profile", "targets_topk", *peaks)
                return out.rows()

            both_fills(case, ttop[radius], targets_topk, **kw)

            def targets_hits(c, o, h):
                w_rows, w_toff = thits[radius]
                best_t = eng.solve_targets_device(c, o, h, ts)  # within 20 of each pair's best, as the CPU call forms it
                thr_t = (best_t[:, :, 0].to(torch.int64) - 20).clamp(-2**31, 2**31 - 1).to(torch.int32).contiguous()
                rows = Guarded((len(w_rows), 3), torch.int32, g)
                toff = Guarded((n * ts.T + 1,), torch.int64, 1)
                eng.solve_targets_hits_device(c, o, h, ts, thresholds_t=thr_t, cap=len(w_rows), rows_t=rows.out,
                                              toffsets_t=toff.out, radius=radius)
                ran("profile", "targets_hits", *peaks)
                assert np.array_equal(toff.rows(), w_toff)
                return rows.rows()

            both_fills(case, thits[radius][0], targets_hits, **kw)

        def targets_rank(c, o, h):
            out = Guarded((n, 2, 4), torch.int32, g)
            eng.solve_targets_rank_device(c, o, h, ts, 2, out.out)
            ran("profile", "targets", "targets_rank")
            return out.rows()

        both_fills(case, trank, targets_rank, **kw)

        if chunked:
            continue
        for rows, counts, marks, K in ((best, counts1, marks1, 1), (top[0], counts3, marks3, 3)):
            def report(c, o, h):
                rows_t = torch.from_numpy(np.array(rows)).to(DEV)  # a writable copy of the read-only oracle
                c_out = Guarded(counts.shape, torch.int32, g)  # 16-byte rows: the documented alignment holds
                m_out = Guarded((K * total, 1), torch.uint8, 1 + 2 * i, behind=7)  # an odd byte offset
                assert c_out.out.data_ptr() % 16 == 0 and m_out.out.data_ptr() % 2 == 1
                eng.report_device(c, o, h, rows_t, c_out.out, m_out.out.view(-1))
                assert "report" in eng.stats()["kernels"], eng.stats()
                assert np.array_equal(m_out.rows().reshape(-1), marks)
                return c_out.rows()

            both_fills(case, counts, report, **kw)


@pytest.mark.parametrize("sem", SEMS)
def test_feature_device_forms(engine, sem):
    feature_forms(engine, sem, FEW + (FAR,))


def test_feature_device_forms_in_chunks(engine):
    """A profile scratch of 4 KiB: several chunks, whose letter and plan bases come from the absolute offsets."""
    engine.set_profile_scratch(1 << 12)
    try:
        feature_forms(engine, Semantics.REFERENCE, (13, 15, FAR), chunked=True)
    finally:
        engine.set_profile_scratch(256 << 20)


def test_hits_within_on_the_default_stream(engine):
    """``within`` forms its thresholds with torch operations between the search and the hits kernels. On torch's
    default stream, which stands for the engine's own (non-blocking) compute stream, those were ordered with neither:
    a batch whose search ends in the tile kernel got thresholds from rows not yet written."""
    sub, sem = feature_sub(), Semantics.REFERENCE
    hits, ho = oracle((FEATURE, sem, "hits"), lambda: search_hits_cpu(sub, within=20, semantics=sem))
    engine.set_problem(sub.weights, sub.seq1, sem)
    codes_t, offs_t, h_offs = device_batch(family_case(FEATURE, 32 + 13), "continue")
    torch.cuda.synchronize()
    for _ in range(4):
        rows_t, hoff_t = engine.solve_hits_device(codes_t, offs_t, h_offs, within=20, cap=len(hits))
        torch.cuda.synchronize()
        assert np.array_equal(hoff_t.cpu().numpy(), ho) and np.array_equal(rows_t.cpu().numpy(), hits)


# ---- 8. host forms on the storage with offsets[a : b + 1] -------------------------------------------------------
def test_host_forms():
    case = family_case("host", 32 + 13)
    full = case.sub
    a, b = 17, full.n - 9
    lo = int(full.offsets[a])
    sub = Problem(full.weights, full.seq1, full.codes[lo:int(full.offsets[b])].copy(), full.offsets[a:b + 1] - lo)
    offsets = case.offsets[a:b + 1]
    ts = TargetSet(sub.seq1, [0, 40, sub.L1])
    want = as_triples(search_cpu(sub))
    eng = HipSearchEngine(device=0, chunk_records=100)
    try:
        eng.set_problem(sub.weights, sub.seq1)
        got = {}
        for fill in FILLS:
            st = case.storage(fill)
            res = [as_triples(eng.solve(st, offsets))]
            stats = eng.stats()
            assert stats["chunks"] >= 3 and stats["direct"] == 0 and stats["records"] == sub.n, stats
            assert "swipe" in stats["kernels"] or "short" in stats["kernels"], stats
            assert not differing(res[0], want), differing(res[0], want)
            res.append(eng.solve_topk(st, offsets, 3))
            assert "profile" in eng.stats()["kernels"]
            assert np.array_equal(res[-1], search_topk_cpu(sub, 3))
            rows, hoff = eng.solve_hits(st, offsets, within=20)
            assert "hits" in eng.stats()["kernels"]
            w_rows, w_hoff = search_hits_cpu(sub, within=20)
            assert np.array_equal(hoff, w_hoff) and np.array_equal(rows, w_rows)
            res += [rows, hoff]
            summ, hist = eng.solve_summary(st, offsets, BINS, LO, WIDTH)
            assert "summary" in eng.stats()["kernels"]
            w_summ, w_hist = search_summary_cpu(sub, BINS, LO, WIDTH)
            assert np.array_equal(summ, w_summ) and np.array_equal(hist, w_hist)
            res += [summ, hist]
            res.append(eng.solve_targets(st, offsets, ts))
            assert "targets" in eng.stats()["kernels"]
            assert np.array_equal(res[-1], search_targets_cpu(sub, ts))
            summ, hist = eng.solve_targets_summary(st, offsets, ts, BINS, LO, WIDTH)
            assert "targets_summary" in eng.stats()["kernels"]
            w_summ, w_hist = search_targets_summary_cpu(sub, ts, BINS, LO, WIDTH)
            assert np.array_equal(summ, w_summ) and np.array_equal(hist, w_hist)
            res += [summ, hist]
            got[fill] = res
        for x, y in zip(got["A"], got["continue"]):
            assert np.array_equal(x, y)
    finally:
        eng.close()
