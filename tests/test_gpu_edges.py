"""GPU (MI355X / gfx950) edge tests of the search kernels: every offset of a record as the planted, unique
winner (utils/synthetic.make_planted) through every plan of the engine, context-parallel shares of those
problems, ties across tile / window / share boundaries (make_planted_ties), and batches of 0 .. 513 records
through every wire form. Integer-exact against the CPU engine (itself swept the same way in test_planted.py)
and against the builders' own expectation; every test asserts the kernels and forms it ran."""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = pytest.mark.gpu

if not gpu_available():  # pragma: no cover - collected on CPU hosts only with -m gpu
    pytest.skip("no GPU", allow_module_level=True)

import torch  # noqa: E402

from mpi_openmp_cuda_amd import (HipSearchEngine, Problem, Semantics, decode_keys, search_cpu,  # noqa: E402
                                 search_keys_cpu)
from mpi_openmp_cuda_amd import _lib  # noqa: E402
from mpi_openmp_cuda_amd.ops.align import as_triples  # noqa: E402
from mpi_openmp_cuda_amd.parallel.wire import WireSlice  # noqa: E402
from mpi_openmp_cuda_amd.utils.synthetic import (Shape, differing, make_planted, make_planted_ties,  # noqa: E402
                                                 make_shape, planted_expected)

SEMS = [Semantics.REFERENCE, Semantics.SPEC]
W = (10, 2, 3, 4)
W_I16 = (200, 10, 10, 10)  # |Dt| past the byte pairs: the int16 profile
W_DPP = (300, 300, 1, 1)   # |Dt| past the int16 profile: the LUT (DPP) tile kernel
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def engine():
    e = HipSearchEngine(device=0)
    yield e
    e.close()


# ---- problems and their references: built once, shared, read-only -------------------------------------
_planted = {}


def planted(L1, L2, w=W, positions=None):
    """(problem, positions, {semantics: reference triples}) of make_planted; the CPU engine's answer is the
    reference, and it must be what the construction implies — for every record."""
    key = (L1, L2, tuple(w), None if positions is None else tuple(positions))
    if key not in _planted:
        prob, pos = make_planted(L1, L2, w, positions, seed=L1 + L2)
        refs = {}
        for sem in SEMS:
            ref = as_triples(search_cpu(prob, sem)).copy()
            want = planted_expected(prob, pos, sem)
            assert np.array_equal(ref, want), differing(ref, want, pos)
            ref.setflags(write=False)
            refs[sem] = ref
        for a in (prob.codes, prob.offsets, prob.seq1):
            a.setflags(write=False)
        _planted[key] = (prob, pos, refs)
    return _planted[key]


_full_keys = {}


def full_keys(key, prob, sem):
    if (key, sem) not in _full_keys:
        k = search_keys_cpu(prob, 0, 1, sem)
        k.setflags(write=False)
        _full_keys[(key, sem)] = k
    return _full_keys[(key, sem)]


def assert_path(st, kernels, has=(), lacks=()):
    assert st["kernels"] == list(kernels), st
    assert has, "every case names a form it must have run"
    for f in has:
        assert f in st["forms"], st
    for f in lacks:
        assert f not in st["forms"], st


def assert_rows(got, want, pos, what):
    msg = differing(got, want, pos)
    assert not msg, f"{what}: {msg}"


# ---- C1: every offset as the unique winner, one case per plan -----------------------------------------
# id, L1, L2, weights, positions (None: every offset), environment of a fresh engine, kernels, forms the run
# must / must not name. stats() names the kernel and its arithmetic form, not the plan (whole image, window, U):
# there the shape and the environment carry the case, and the environment does reach the engine: its
# constructor reads MOC_TILE_U, MOC_TILE16_WINWIDE, MOC_TILE16_SLIDE and MOC_MFMA for every engine made.
SLIDE_17 = (0, 1, 127, 128, 129, 255, 256, 511, 512, 640, 1023, 1024, 1151, 1152, 1298, 1299, 1300)
EVERY_OFFSET = [
    # swipe takes records of at most 64 lanes (L1 - L2 + 1): 63 offsets under the reference, 64 under the spec
    # is its widest instance (NOFF 64, searching() at its bound) ...
    ("swipe_noff64", 71, 8, W, None, {}, ["swipe"], ["swipe_kbits"], ["swipe_rk"]),
    # ... and one offset more (64 / 65) already belongs to the tile kernels, under both semantics
    ("past_swipe_65_lanes", 72, 8, W, None, {}, ["tile16"], ["tile16"], ["tile16_slide"]),
    ("swipe_l2_40", 72, 40, W, None, {}, ["swipe"], ["swipe_rk"], ["swipe_kbits"]),  # past 32 letters: RK only
    # the lane-per-offset kernel: int32 keys where Seq1 is too long for its LDS profile (L1 > 163), the packed
    # int16 form on the profile
    ("short", 200, 150, W, None, {}, ["short"], ["short_key32"], ["short_pk", "short_key64"]),
    ("short_pk", 150, 130, W, None, {}, ["short"], ["short_pk"], ["short_key32", "short_key64"]),
    ("tile16_wide_u8", 1400, 40, W, None, {}, ["tile16"], ["tile16"], ["tile16_slide", "tile16_i16"]),
    ("tile16_wide_u2", 1400, 300, W, None, {}, ["tile16"], ["tile16"], ["tile16_slide", "tile16_i16"]),
    ("tile16_wide_l2_40_u4", 1400, 40, W, None, {"MOC_TILE_U": "4"}, ["tile16"], ["tile16"], ["tile16_slide"]),
    ("tile16_wide_l2_300_u4", 1400, 300, W, None, {"MOC_TILE_U": "4"}, ["tile16"], ["tile16"], ["tile16_slide"]),
    ("tile16_wide_window_unaligned", 2001, 40, W, None, {}, ["tile16"], ["tile16"], ["tile16_slide"]),
    # without the widened window the sliding windows take these records, unless they are switched off too: then
    # the whole byte-pair image does
    ("tile16_winwide_off", 2001, 40, W, None, {"MOC_TILE16_WINWIDE": "0"}, ["tile16"], ["tile16", "tile16_slide"], []),
    ("tile16_byte_pair_image", 2001, 40, W, None, {"MOC_TILE16_WINWIDE": "0", "MOC_TILE16_SLIDE": "0"}, ["tile16"],
     ["tile16"], ["tile16_slide"]),
    ("tile16_windowed", 6500, 40, W, None, {}, ["tile16"], ["tile16"], ["tile16_slide"]),
    ("tile16_slide", 2400, 1100, W, None, {}, ["tile16"], ["tile16", "tile16_slide"], []),
    # 17 records: a full group of 16 and one of a single record (the int16 profile slides from a quarter filled)
    ("tile16_slide_partial_group", 2400, 1100, W_I16, SLIDE_17, {}, ["tile16"], ["tile16_slide", "tile16_i16"], []),
    ("dpp_tiles", 600, 150, W_DPP, None, {}, ["tiles"], ["tiles_key32"], ["tile16", "tiles_key64"]),
    ("mfma", 1400, 300, W, None, {"MOC_MFMA": "1"}, ["tile16"], ["mfma"], []),
]


@pytest.mark.parametrize("case", EVERY_OFFSET, ids=[c[0] for c in EVERY_OFFSET])
def test_every_offset_wins(engine, monkeypatch, case):
    name, L1, L2, w, positions, env, kernels, has, lacks = case
    prob, pos, refs = planted(L1, L2, w, positions)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = HipSearchEngine(device=0) if env else engine
    try:
        codes_t = torch.from_numpy(prob.codes.copy()).to(DEV)
        offs_t = torch.from_numpy(prob.offsets.copy()).to(DEV)
        for sem in SEMS:
            eng.set_problem(prob.weights, prob.seq1, sem)
            out = np.full(prob.n, -7, dtype=_lib.RESULT_DTYPE)
            eng.solve(prob.codes, prob.offsets, out=out)
            assert_path(eng.stats(), kernels, has, lacks)
            assert_rows(as_triples(out), refs[sem], pos, f"{name} solve {sem.name}")
            out_t = torch.full((prob.n, 3), -7, dtype=torch.int32, device=DEV)
            eng.solve_device(codes_t, offs_t, prob.offsets, out_t)
            torch.cuda.synchronize()
            assert_path(eng.stats(), kernels, has, lacks)
            assert_rows(out_t.cpu().numpy(), refs[sem], pos, f"{name} solve_device {sem.name}")
    finally:
        if env:
            eng.close()


# ---- C2: context-parallel shares of the planted problems ----------------------------------------------
# name, L1, L2, weights, kernel, form of every share
SHARED = [("whole_image", 1400, 300, W, "tile16", "tile16"), ("windowed", 6500, 40, W, "tile16", "tile16"),
          ("dpp_tiles", 600, 150, W_DPP, "tiles", "tiles_key32")]
PARTS = [1, 2, 3, 8, 17, 64]


@pytest.mark.parametrize("parts", PARTS)
@pytest.mark.parametrize("case", SHARED, ids=[c[0] for c in SHARED])
def test_context_parallel_shares_of_planted(engine, case, parts):
    name, L1, L2, w, kernel, form = case
    prob, pos, refs = planted(L1, L2, w)
    for sem in SEMS:
        engine.set_problem(prob.weights, prob.seq1, sem)
        want = full_keys((L1, L2, w), prob, sem)
        keys = np.zeros(prob.n, np.uint64)
        for part in range(parts):
            share = engine.search_keys(prob.codes, prob.offsets, part, parts)
            # (every share launches: its waves may be empty, its plan never is)
            assert_path(engine.stats(), [kernel], [form], ["tile16_slide", "mfma"])
            below = np.nonzero(share > want)[0]
            assert below.size == 0, f"{name} part {part}/{parts}: keys above the full search's at p = {pos[below[:8]]}"
            keys = np.maximum(keys, share)
        assert_rows(keys[:, None], want[:, None], pos, f"{name} keys over {parts} parts {sem.name}")
        assert_rows(as_triples(decode_keys(keys, prob)), refs[sem], pos, f"{name} decoded {sem.name}")


@pytest.mark.parametrize("case", SHARED, ids=[c[0] for c in SHARED])
def test_context_parallel_shares_device(engine, case, parts=8):
    # the device-resident form: keys per share in device memory (poisoned first), MAX-combined there, finalized
    name, L1, L2, w, kernel, form = case
    prob, pos, refs = planted(L1, L2, w)
    codes_t = torch.from_numpy(prob.codes.copy()).to(DEV)
    offs_t = torch.from_numpy(prob.offsets.copy()).to(DEV)
    flip = torch.tensor(-2**63, dtype=torch.int64, device=DEV)  # uint64 order == signed order, top bit flipped
    for sem in SEMS:
        engine.set_problem(prob.weights, prob.seq1, sem)
        shares = []
        for part in range(parts):
            k = torch.full((prob.n,), 0x7777777777777777, dtype=torch.int64, device=DEV)
            engine.search_keys_device(codes_t, offs_t, prob.offsets, part, parts, k)
            assert_path(engine.stats(), [kernel], [form], ["tile16_slide", "mfma"])
            shares.append(k)
        torch.cuda.synchronize()
        best = torch.stack([s ^ flip for s in shares]).max(dim=0).values ^ flip
        want = full_keys((L1, L2, w), prob, sem)
        assert_rows(best.cpu().numpy().view(np.uint64)[:, None], want[:, None], pos, f"{name} device keys {sem.name}")
        out = torch.full((prob.n, 3), -7, dtype=torch.int32, device=DEV)
        engine.finalize_keys_device(codes_t, offs_t, prob.offsets, best, out)
        torch.cuda.synchronize()
        assert_rows(out.cpu().numpy(), refs[sem], pos, f"{name} finalized {sem.name}")


# ---- C3: ties across tile, window and share boundaries ------------------------------------------------
TIE_L2 = 16


def tie_pair_sets(L1):
    """Pair sets (one Seq1 each; their segments must not overlap) around every multiple B of 128 below
    L1 - L2: copies that start on the last offset before B and end up right behind (a = B - 1, b = a + L2),
    copies that start on B (b = B, a = B - L2 - 1), and a few from the first tile to the last."""
    bs = list(range(128, L1 - TIE_L2, 128))
    before = [(B - 1, B - 1 + TIE_L2) for B in bs if B - 1 + 2 * TIE_L2 <= L1]
    onto = [(B - TIE_L2 - 1, B) for B in bs if B + TIE_L2 <= L1]
    last = L1 - TIE_L2  # the final offset (the spec semantics' extra one)
    far = [(x, last - x) for x in (0, 17, 40, 63, 84)]
    return [before, onto, far]


_ties = {}


def ties(L1, L2, w, pairs, seed):
    key = (L1, L2, tuple(w), tuple(pairs))
    if key not in _ties:
        prob, pr = make_planted_ties(L1, L2, w, pairs, seed=seed)
        want = np.stack([np.full(len(pr), w[0] * L2), pr[:, 0], np.zeros(len(pr), np.int64)], axis=1).astype(np.int32)
        for sem in SEMS:  # the smaller offset wins, for the oracle too
            ref = as_triples(search_cpu(prob, sem))
            assert np.array_equal(ref, want), differing(ref, want, pr[:, 0])
        want.setflags(write=False)
        _ties[key] = (prob, pr, want)
    return _ties[key]


@pytest.mark.parametrize("which", [0, 1, 2], ids=["a_before_boundary", "b_on_boundary", "first_to_last_tile"])
@pytest.mark.parametrize("L1", [1400, 6500], ids=["whole_image", "windowed"])
def test_ties_across_boundaries(engine, L1, which):
    pairs = tie_pair_sets(L1)[which]
    prob, pr, want = ties(L1, TIE_L2, W, pairs, seed=L1 + which)
    assert prob.n == len(pairs) >= 5
    for sem in SEMS:
        engine.set_problem(prob.weights, prob.seq1, sem)
        got = as_triples(engine.solve(prob.codes, prob.offsets))
        assert_path(engine.stats(), ["tile16"], ["tile16"], ["tile16_slide"])
        assert_rows(got, want, pr[:, 0], f"ties solve {sem.name}")
        for parts in (3, 8):  # the two copies in different shares: the key encoding alone breaks the tie
            full = search_keys_cpu(prob, 0, 1, sem)
            keys = np.zeros(prob.n, np.uint64)
            for part in range(parts):
                keys = np.maximum(keys, engine.search_keys(prob.codes, prob.offsets, part, parts))
                assert_path(engine.stats(), ["tile16"], ["tile16"], ["tile16_slide"])
            assert_rows(keys[:, None], full[:, None], pr[:, 0], f"ties keys over {parts} parts {sem.name}")
            assert_rows(as_triples(decode_keys(keys, prob)), want, pr[:, 0], f"ties decoded {parts} parts {sem.name}")


@pytest.mark.parametrize("pair", [(127, 1227), (180, 1280), (0, 1300)], ids=lambda p: f"{p[0]}_{p[1]}")
def test_ties_sliding_windows(engine, pair):
    # records of 1100 letters on L1 2400: one tied pair fits a Seq1. The sliding windows need full groups of 16
    # records, so 15 planted pieces of the same Seq1 (unique winners but for the pair's own offsets) ride along
    L1, L2 = 2400, 1100
    tprob, pr, twant = ties(L1, L2, W, [pair], seed=pair[0])
    fill = [p for p in (1, 64, 126, 128, 129, 255, 256, 300, 511, 512, 640, 1023, 1024, 1151, 1299, 1152)
            if p not in pair][:15]
    recs = [tprob.codes] + [tprob.seq1[p:p + L2] for p in fill]
    prob = Problem(tprob.weights, tprob.seq1, np.concatenate(recs),
                   np.arange(len(recs) + 1, dtype=np.int64) * L2)
    pos = np.array([pair[0]] + fill)
    for sem in SEMS:
        ref = as_triples(search_cpu(prob, sem))
        assert tuple(ref[0]) == tuple(twant[0]) == (W[0] * L2, pair[0], 0)
        engine.set_problem(prob.weights, prob.seq1, sem)
        got = as_triples(engine.solve(prob.codes, prob.offsets))
        assert_path(engine.stats(), ["tile16"], ["tile16", "tile16_slide"])
        assert_rows(got, ref, pos, f"ties slide {sem.name}")
        for parts in (3, 8):
            keys = np.zeros(prob.n, np.uint64)
            for part in range(parts):
                keys = np.maximum(keys, engine.search_keys(prob.codes, prob.offsets, part, parts))
                # (shares of a split search do not slide: the whole byte-pair image)
                assert_path(engine.stats(), ["tile16"], ["tile16"], ["tile16_slide"])
            assert_rows(keys[:, None], search_keys_cpu(prob, 0, 1, sem)[:, None], pos, f"ties keys {parts} {sem.name}")
            assert_rows(as_triples(decode_keys(keys, prob)), ref, pos, f"ties decoded {parts} parts {sem.name}")


# ---- C4: record-count sweep ---------------------------------------------------------------------------
COUNTS = [1, 2, 7, 8, 9, 23, 24, 25, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513]
POISON = 0x77
# name, shape: 64- and 128-record tiles, base-6 / 4-bit lengths, P33 fields of 7 letters starting at st % 7
# and the swipe form every slice of the batch runs
BATCHES = [
    ("input6_base6_lengths_h2", Shape((4, 3, 2, 10), 26, 6, 11), "swipe_kbits"),   # the headline: 128-record tiles
    ("nibble_lengths", Shape((5, 2, 3, 4), 40, 20, 32), "swipe_kbits"),
    ("input1_rk", Shape((100, 2, 3, 4), 51, 32, 41), "swipe_rk"),                  # RK form, 64-record tiles
    ("fixed_length_9", Shape((4, 3, 2, 10), 26, 9, 9), "swipe_kbits"),             # 9 n letters: every residue mod 7
]


def _device_wire(engine, ws, res, sparse):
    letters = torch.from_numpy(ws.codes).to(DEV)
    offsets = torch.from_numpy(ws.sparse_offsets(6) if sparse else np.asarray(ws.offsets)).to(DEV)
    lengths = torch.from_numpy(ws.lengths).to(DEV) if ws.lengths is not None else None
    out = torch.full((max(res.nbytes, 1),), POISON, dtype=torch.uint8, device=DEV)
    engine.solve_wire_device(letters, offsets, lengths, ws.n, out, ws.fmt, (ws.l2_min, ws.l2_max),
                             lengths_bits=ws.len_bits or 8, lengths_base=ws.len_base,
                             packed33=ws.letter_format == "p33", off_shift=6 if sparse else 0)
    res.view(np.uint8)[:] = out.cpu().numpy()[:res.nbytes]


@pytest.mark.parametrize("sem", SEMS, ids=lambda s: s.name)
@pytest.mark.parametrize("batch", BATCHES, ids=[b[0] for b in BATCHES])
def test_record_count_sweep(batch, sem):
    # one engine per problem; the first n records of one batch for every n, through every way a batch reaches
    # the swipe kernel; results poisoned before each solve, every row compared, every failure reported
    name, shape, form = batch
    full = make_shape(shape, max(COUNTS), seed=len(name))
    ref = as_triples(search_cpu(full, sem)).copy()
    ref.setflags(write=False)
    eng = HipSearchEngine(device=0)
    eng.set_problem(full.weights, full.seq1, sem)
    failures, judged = [], []

    def judge(what, n, got, st, direct, h2d0=False):
        judged.append(what)
        assert got.shape == (n, 3)
        bad = np.nonzero((got != ref[:n]).any(axis=1))[0]
        if bad.size:
            failures.append(f"{what} n={n}: {bad.size} rows differ, first #{bad[:5].tolist()} got "
                            f"{got[bad[:5]].tolist()} want {ref[bad[:5]].tolist()}")
        if (st["kernels"] != ["swipe"] or st["forms"] != [form] or (direct is not None and st["direct"] != direct) or
                (h2d0 and st["h2d_bytes"] != 0) or st["records"] != n):
            failures.append(f"{what} n={n}: path {st}")

    try:
        for n in COUNTS:
            prob = full.slice(0, n)
            # zero-copy from pinned memory: P33 letters (thrice: plain launch, graph capture, graph replay, each on
            # poisoned results: the self-resetting work counter and the replay see the small grid too), byte
            # letters; 5-bit letters take the staged pipeline
            for letters, direct, solves in (("p33", 1, 3), ("bytes", 1, 2), ("p5", 0, 1)):
                ws = WireSlice.from_csr(prob.codes, prob.offsets, letter_format=letters)
                ws.alloc_results(eng)
                with _lib.Pinned(*ws.arrays()):
                    for rep in range(solves):
                        ws.results.view(np.uint8)[:] = POISON
                        ws.solve(eng)
                        judge(f"pinned {letters} solve {rep}", n, ws.triples(eng), eng.stats(), direct)
            # device-resident wire batches: P33 letters with 64-record sparse offsets (the rccl transport's form)
            # and with dense ones, byte letters with dense offsets and no lengths
            for letters, sparse in (("p33", True), ("p33", False), ("bytes", False)):
                ws = WireSlice.from_csr(prob.codes, prob.offsets, letter_format=letters)
                res = ws.alloc_results(eng)
                if letters == "bytes":
                    ws.lengths, ws.len_bits, ws.len_base = None, 0, 0  # lengths from the offsets, in the kernel
                _device_wire(eng, ws, res, sparse)
                judge(f"device {letters} {'sparse' if sparse else 'dense'}", n, ws.triples(eng), eng.stats(), 1,
                      h2d0=True)
            # device-resident CSR and the plain staged solve
            out_t = torch.full((n, 3), -7, dtype=torch.int32, device=DEV)
            eng.solve_device(torch.from_numpy(prob.codes).to(DEV), torch.from_numpy(prob.offsets).to(DEV), prob.offsets,
                             out_t)
            torch.cuda.synchronize()
            judge("solve_device", n, out_t.cpu().numpy(), eng.stats(), None)
            out = np.full(n, -7, dtype=_lib.RESULT_DTYPE)
            eng.solve(prob.codes, prob.offsets, out=out)
            judge("staged solve", n, as_triples(out), eng.stats(), 0)
    finally:
        eng.close()
    assert len(judged) == 11 * len(COUNTS)  # 6 pinned, 3 device wire, solve_device, staged: none left out
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:40])


def test_zero_records(engine):
    # n = 0 returns early everywhere: an empty result, nothing launched, nothing written
    prob, _, _ = planted(71, 8)
    engine.set_problem(prob.weights, prob.seq1)
    offsets = np.zeros(1, np.int64)
    codes = np.zeros(16, np.uint8)
    got = engine.solve(codes, offsets)
    st = engine.stats()
    assert got.shape == (0,) and st["kernels"] == [] and st["forms"] == [] and st["chunks"] == 0 and st["records"] == 0
    assert st["kernel_ms"] == 0 and st["h2d_bytes"] == 0 and st["d2h_bytes"] == 0, st
    ws = WireSlice.from_csr(codes[:0], offsets)
    assert ws.n == 0 and ws.alloc_results(engine).shape == (0,)
    guard = np.full(8, POISON, np.uint8)
    engine.solve(ws.codes, ws.offsets, out=guard.view(_lib.R2_DTYPE), lengths=None, fmt="r2", l2_range=(0, 0),
                 packed33=True)
    assert engine.stats()["kernels"] == [] and (guard == POISON).all()
    assert engine.search_keys(codes, offsets, 0, 3).shape == (0,)
    out_t = torch.full((4, 3), -7, dtype=torch.int32, device=DEV)
    engine.solve_device(torch.from_numpy(codes).to(DEV), torch.from_numpy(offsets).to(DEV), offsets, out_t[:0])
    raw = torch.full((16,), POISON, dtype=torch.uint8, device=DEV)
    engine.solve_wire_device(torch.from_numpy(codes).to(DEV), torch.from_numpy(offsets).to(DEV), None, 0, raw, "r12",
                             (0, 0), packed33=False)
    torch.cuda.synchronize()
    assert engine.stats()["kernels"] == [] and engine.stats()["records"] == 0
    assert (out_t.cpu().numpy() == -7).all() and (raw.cpu().numpy() == POISON).all()


# the tile kernels' record counts: groups of 16 records (sliding windows) and 16-wave workgroups (windowed)
@pytest.mark.parametrize("n_long", [1, 15, 16, 17, 33])
@pytest.mark.parametrize("plan", ["slide", "windowed"])
def test_tile_kernels_record_counts(engine, plan, n_long):
    if plan == "slide":
        L1, L2, w = 2400, 1100, W_I16  # the int16 profile slides from groups a quarter filled (n = 17, 33: 0.53, 0.69)
    else:
        L1, L2, w = 6500, 40, W
    noff = L1 - L2 + 1
    # the first, the last and the boundary offsets first, then an even spread
    fixed = [0, noff - 1, noff - 2, 127, 128]
    spread = [int(x) for x in np.linspace(1, noff - 3, 33).astype(int) if int(x) not in fixed]
    positions = tuple((fixed + spread)[:n_long])
    assert len(set(positions)) == n_long
    prob, pos, refs = planted(L1, L2, w, positions)
    for sem in SEMS:
        engine.set_problem(prob.weights, prob.seq1, sem)
        out = np.full(prob.n, -7, dtype=_lib.RESULT_DTYPE)
        engine.solve(prob.codes, prob.offsets, out=out)
        st = engine.stats()
        if plan == "slide" and n_long < 4:
            # a lone record (1 of 16 waves) is below the int16 profile's quarter fill: the LUT tile kernel has it
            assert_path(st, ["tiles"], ["tiles_key32"], ["tile16", "tile16_slide"])
        elif plan == "slide":
            assert_path(st, ["tile16"], ["tile16", "tile16_i16", "tile16_slide"])
        else:
            assert_path(st, ["tile16"], ["tile16"], ["tile16_slide", "tile16_i16"])
        assert_rows(as_triples(out), refs[sem], pos, f"{plan} {n_long} records {sem.name}")
