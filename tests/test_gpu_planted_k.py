"""GPU (MI355X / gfx950) tests of the mutation point k: every k of a record as the planted, unique winner
(utils/synthetic.make_planted_k) and the three ties k's tie-break decides (make_planted_k_ties) through every
kernel that finds k its own way — the swipe kernel's key bits and its second walk, the lane-per-offset kernel's
key bits, the tile kernels' mutated bit with resolve_long_kernel behind them, the profile kernels — through the
context-parallel keys, the wire paths and every result format, and skipped-letter mutants at the exactness bounds
(make_extreme_mutants). Integer-exact against the construction's claim, which the CPU engine must give too; every
case asserts the kernels and forms it ran. The case lists are tests/planted_k.py; tests/test_planted_k.py proves
the claims against the prefix oracle and shows that these cases tell a wrong k rule from the right one."""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = pytest.mark.gpu

if not gpu_available():  # pragma: no cover - collected on CPU hosts only with -m gpu
    pytest.skip("no GPU", allow_module_level=True)

import torch  # noqa: E402

import planted_k as pk  # noqa: E402
from mpi_openmp_cuda_amd import (HipSearchEngine, Semantics, brute_force_native, decode_keys, search_cpu,  # noqa: E402
                                 search_hits_cpu, search_keys_cpu, search_profile_cpu, search_topk_cpu)
from mpi_openmp_cuda_amd import _lib  # noqa: E402
from mpi_openmp_cuda_amd.ops.align import SUMMARY_COLS, as_triples  # noqa: E402
from mpi_openmp_cuda_amd.parallel.wire import WireSlice  # noqa: E402
from mpi_openmp_cuda_amd.utils.synthetic import (differing, make_extreme_mutants, make_planted_k,  # noqa: E402
                                                 planted_k_expected)

SEMS = [Semantics.REFERENCE, Semantics.SPEC]
DEV = torch.device("cuda:0")
POISON = 0x77
ROW_IDS = [r[0] for r in pk.ROWS]


@pytest.fixture(scope="module")
def engine():
    e = HipSearchEngine(device=0)
    yield e
    e.close()


# ---- problems and their claims: built once, shared, read-only -----------------------------------------
_checked = set()


def problem(name, family="k", tag="all"):
    """(problem, winner offsets, claimed rows) of tests/planted_k.py; the CPU engine must give the claim, under
    both semantics, for every record."""
    prob, cases, want = pk.build(name, family, tag)
    if (name, family, tag) not in _checked:
        for sem in SEMS:
            ref = as_triples(search_cpu(prob, sem))
            assert np.array_equal(ref, want), differing(ref, want, want[:, 1])
        _checked.add((name, family, tag))
    return prob, want[:, 1], want


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


def fresh(engine, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return HipSearchEngine(device=0) if env else engine


def solve_both_ways(eng, prob, want, pos, path, what):
    """solve and solve_device under both semantics, results poisoned first, the path asserted after each."""
    codes_t = torch.from_numpy(prob.codes.copy()).to(DEV)
    offs_t = torch.from_numpy(prob.offsets.copy()).to(DEV)
    for sem in SEMS:
        eng.set_problem(prob.weights, prob.seq1, sem)
        out = np.full(prob.n, -7, dtype=_lib.RESULT_DTYPE)
        eng.solve(prob.codes, prob.offsets, out=out)
        assert_path(eng.stats(), *path)
        assert_rows(as_triples(out), want, pos, f"{what} solve {sem.name}")
        out_t = torch.full((prob.n, 3), -7, dtype=torch.int32, device=DEV)
        eng.solve_device(codes_t, offs_t, prob.offsets, out_t)
        torch.cuda.synchronize()
        assert_path(eng.stats(), *path)
        assert_rows(out_t.cpu().numpy(), want, pos, f"{what} solve_device {sem.name}")


# ---- every k as the unique winner, one case per way of finding k ---------------------------------------
@pytest.mark.parametrize("name", ROW_IDS)
def test_every_k_wins(engine, monkeypatch, name):
    row = pk.ROW[name]
    prob, pos, want = problem(name)
    eng = fresh(engine, row[4], monkeypatch)
    try:
        solve_both_ways(eng, prob, want, pos, row[5:8], name)
    finally:
        if row[4]:
            eng.close()


# ---- the three ties, through every row ------------------------------------------------------------------
@pytest.mark.parametrize("name", ROW_IDS)
def test_k_ties(engine, monkeypatch, name):
    row = pk.ROW[name]
    families = pk.tie_problems(row)
    assert {f for f, _, _ in families} == {"inside", "own", "shadow"}
    eng = fresh(engine, row[4], monkeypatch)
    try:
        for family, tag, _ in families:
            prob, pos, want = problem(name, family, tag)
            solve_both_ways(eng, prob, want, pos, row[5:8], f"{name} {family} {tag}")
    finally:
        if row[4]:
            eng.close()


# ---- context-parallel shares: the resolve kernel alone turns a combined key back into k -----------------
SHARED = [("tile16_l2_300_u2", "tile16", "tile16"), ("tile16_windowed", "tile16", "tile16"),
          ("dpp_tiles_key32", "tiles", "tiles_key32")]


@pytest.mark.parametrize("parts", [3, 8])
@pytest.mark.parametrize("case", SHARED, ids=[c[0] for c in SHARED])
def test_k_through_split_searches(engine, case, parts):
    name, kernel, form = case
    probs = [("k", "all")] + [(f, t) for f, t, _ in pk.tie_problems(pk.ROW[name]) if f == "shadow"]
    flip = torch.tensor(-2**63, dtype=torch.int64, device=DEV)  # uint64 order == signed order, top bit flipped
    for family, tag in probs:
        prob, pos, want = problem(name, family, tag)
        codes_t = torch.from_numpy(prob.codes.copy()).to(DEV)
        offs_t = torch.from_numpy(prob.offsets.copy()).to(DEV)
        for sem in SEMS:
            what = f"{name} {family} {tag} over {parts} parts {sem.name}"
            engine.set_problem(prob.weights, prob.seq1, sem)
            full = search_keys_cpu(prob, 0, 1, sem)
            keys = np.zeros(prob.n, np.uint64)
            shares = []
            for part in range(parts):
                keys = np.maximum(keys, engine.search_keys(prob.codes, prob.offsets, part, parts))
                assert_path(engine.stats(), [kernel], [form], ["tile16_slide", "mfma"])
                k = torch.full((prob.n,), 0x7777777777777777, dtype=torch.int64, device=DEV)
                engine.search_keys_device(codes_t, offs_t, prob.offsets, part, parts, k)
                assert_path(engine.stats(), [kernel], [form], ["tile16_slide", "mfma"])
                shares.append(k)
            assert_rows(keys[:, None], full[:, None], pos, f"{what} keys")
            assert_rows(as_triples(decode_keys(keys, prob)), want, pos, f"{what} decoded")
            torch.cuda.synchronize()
            best = torch.stack([s ^ flip for s in shares]).max(dim=0).values ^ flip
            assert_rows(best.cpu().numpy().view(np.uint64)[:, None], full[:, None], pos, f"{what} device keys")
            out = torch.full((prob.n, 3), -7, dtype=torch.int32, device=DEV)
            engine.finalize_keys_device(codes_t, offs_t, prob.offsets, best, out)
            torch.cuda.synchronize()
            assert_rows(out.cpu().numpy(), want, pos, f"{what} finalized")


# ---- the wire paths of the swipe kernel -----------------------------------------------------------------
SWIPE_ROWS = [r[0] for r in pk.ROWS if r[5] == ["swipe"]]


def _device_wire(eng, ws, res, sparse):
    letters = torch.from_numpy(ws.codes).to(DEV)
    offsets = torch.from_numpy(ws.sparse_offsets(6) if sparse else np.asarray(ws.offsets)).to(DEV)
    lengths = torch.from_numpy(ws.lengths).to(DEV) if ws.lengths is not None else None
    out = torch.full((max(res.nbytes, 1),), POISON, dtype=torch.uint8, device=DEV)
    eng.solve_wire_device(letters, offsets, lengths, ws.n, out, ws.fmt, (ws.l2_min, ws.l2_max),
                          lengths_bits=ws.len_bits or 8, lengths_base=ws.len_base,
                          packed33=ws.letter_format == "p33", off_shift=6 if sparse else 0)
    res.view(np.uint8)[:] = out.cpu().numpy()[:res.nbytes]


@pytest.mark.parametrize("name", SWIPE_ROWS)
def test_k_through_wire_paths(name):
    row = pk.ROW[name]
    L1, w, form = row[1], row[2], row[6][0]
    # at least 129 records (the 128-record tiles of the H = 2 instances run a second tile); among them the top
    # score at the last mutated offset with k = L2 - 1: the largest code a result format has to hold
    cases = pk.fill_to(row[3], 129)
    L2 = max(c[1] for c in cases)
    assert len(cases) >= 129 and (L1 - L2 - 1, L2, L2 - 1) in cases
    prob, cases = make_planted_k(L1, cases, w, seed=len(name))
    want = planted_k_expected(prob, cases)
    pos = want[:, 1]
    eng = HipSearchEngine(device=0)
    judged = []

    def judge(what, ws, direct, fmt=None, h2d0=False):
        st = eng.stats()
        assert_path(st, ["swipe"], [form], [f for f in ("swipe_kbits", "swipe_rk") if f != form])
        assert st["format"] == ws.fmt and (fmt is None or ws.fmt == fmt), (what, st, ws.fmt)
        assert st["direct"] == direct and st["records"] == prob.n and (not h2d0 or st["h2d_bytes"] == 0), (what, st)
        assert_rows(ws.triples(eng), want, pos, what)
        judged.append(what)

    try:
        for sem in SEMS:
            eng.set_problem(prob.weights, prob.seq1, sem)
            ref = as_triples(search_cpu(prob, sem))
            assert np.array_equal(ref, want), differing(ref, want, pos)
            # zero-copy from pinned memory: plain launch, graph capture, graph replay, each on poisoned results;
            # the narrowest format, then each wider one forced
            for fmt in ("auto", "r4", "r8", "r12"):
                ws = WireSlice.from_csr(prob.codes, prob.offsets, letter_format="p33")
                ws.alloc_results(eng, fmt)
                with _lib.Pinned(*ws.arrays()):
                    for rep in range(3 if fmt == "auto" else 1):
                        ws.results.view(np.uint8)[:] = POISON
                        ws.solve(eng)
                        judge(f"{name} {sem.name} pinned p33 {fmt} solve {rep}", ws, 1, None if fmt == "auto" else fmt)
                if fmt == "auto" and name == "swipe_kbits_8":
                    # R2 where the problem allows: the largest code of the batch is the last mutated offset's top
                    # score with k = L2 - 1, and it is the largest the format's parameters admit for these records
                    smin, kw, j = eng.r2_params(ws.l2_min, ws.l2_max)
                    top = (w[0] * L2 - smin) * j + (L1 - L2 - 1) * kw + (L2 - 1)
                    assert ws.fmt == "r2" and int(ws.results.max()) == top < 0xFFFF, (ws.fmt, top, smin, kw, j)
            ws = WireSlice.from_csr(prob.codes, prob.offsets, letter_format="p5")  # 5-bit letters: staged
            ws.alloc_results(eng)
            ws.results.view(np.uint8)[:] = POISON
            ws.solve(eng)
            judge(f"{name} {sem.name} staged p5", ws, 0)
            for sparse in (True, False):  # device-resident P33: 64-record sparse offsets, dense ones
                ws = WireSlice.from_csr(prob.codes, prob.offsets, letter_format="p33")
                res = ws.alloc_results(eng)
                _device_wire(eng, ws, res, sparse)
                judge(f"{name} {sem.name} device p33 {'sparse' if sparse else 'dense'}", ws, 1, h2d0=True)
    finally:
        eng.close()
    assert len(judged) == 2 * 9


# ---- the profile family: its own strict rule per offset ---------------------------------------------------
PROFILED = [("swipe_kbits_16", "k", "all"), ("tile16_l2_40_u8", "k", "all"), ("swipe_rk_64", "inside", "all"),
            ("tile16_l2_300_u2", "own", "all"), ("tile16_l2_40_u8", "shadow", "set0")]


def assert_profile_path(st, kernel):
    assert "profile" in st["kernels"] and kernel in st["kernels"] and st["forms"] == [], st


@pytest.mark.parametrize("case", PROFILED, ids=["_".join(c) for c in PROFILED])
def test_k_in_the_profile_family(engine, case):
    prob, pos, want = problem(*case)
    codes_t = torch.from_numpy(prob.codes.copy()).to(DEV)
    offs_t = torch.from_numpy(prob.offsets.copy()).to(DEV)
    for sem in SEMS:
        what = f"{case} {sem.name}"
        engine.set_problem(prob.weights, prob.seq1, sem)
        cprof, cpoff = search_profile_cpu(prob, sem)
        at = cpoff[:-1] + want[:, 1]  # the claimed offset's entry of every record
        claim2 = want[:, [0, 2]]
        assert_rows(np.stack([cprof["score"][at], cprof["k"][at]], axis=1), claim2, pos, f"{what} CPU profile")
        prof, poff = engine.solve_profile(prob.codes, prob.offsets)
        assert_profile_path(engine.stats(), "profile")
        assert np.array_equal(poff, cpoff) and np.array_equal(prof, cprof), what
        assert_rows(np.stack([prof["score"][at], prof["k"][at]], axis=1), claim2, pos, f"{what} profile")
        prof_t = torch.full((int(cpoff[-1]), 2), -7, dtype=torch.int32, device=DEV)
        engine.solve_profile_device(codes_t, offs_t, prob.offsets, prof_t)
        torch.cuda.synchronize()
        assert_profile_path(engine.stats(), "profile")
        got = prof_t.cpu().numpy()
        assert np.array_equal(got[:, 0], cprof["score"]) and np.array_equal(got[:, 1], cprof["k"]), what
        assert_rows(got[at], claim2, pos, f"{what} device profile")
        top = engine.solve_topk(prob.codes, prob.offsets, 3)
        assert_profile_path(engine.stats(), "profile")
        assert np.array_equal(top, search_topk_cpu(prob, 3, sem)), what
        assert_rows(top[:, 0], want, pos, f"{what} top-K row 0")
        rows, hoff = engine.solve_hits(prob.codes, prob.offsets, within=0)
        assert_profile_path(engine.stats(), "hits")
        crows, choff = search_hits_cpu(prob, within=0, semantics=sem)
        assert np.array_equal(hoff, choff) and np.array_equal(rows, crows), what
        assert (np.diff(hoff) >= 1).all()
        assert_rows(rows[hoff[:-1]], want, pos, f"{what} first hit within 0")  # ascending offsets: the claim first
        summary, _ = engine.solve_summary(prob.codes, prob.offsets)
        assert_profile_path(engine.stats(), "summary")
        cols = [SUMMARY_COLS.index(c) for c in ("max", "n", "k")]
        assert_rows(summary[:, cols], want, pos, f"{what} summary")


# ---- mutants at the exactness bounds ------------------------------------------------------------------
def _extremes():
    from test_gpu import EXTREMES

    return EXTREMES


def _extreme_problem(case, copies, seed, sem):
    _, L1, lo, hi, w, kernels, forms = case
    prob, cases = make_extreme_mutants(L1, lo, hi, w, copies=copies, seed=seed)
    want = planted_k_expected(prob, cases, "extreme")
    # brute force where it is cheap; the CPU engine (pinned to brute force on these inputs by test_planted_k.py)
    # for the longer Seq1
    ref = as_triples(brute_force_native(prob, sem) if L1 <= 130 else search_cpu(prob, sem))
    assert np.array_equal(ref, want), differing(ref, want, cases[:, 0])
    return prob, want


EXTREME_IDS = [c[0] for c in _extremes() if c[0].endswith(("_at", "_past"))]


def test_extreme_rows_are_the_bounds_rows():
    by_name = {c[0]: c for c in _extremes()}
    assert len(EXTREME_IDS) == 25 and len(SWIPE_EXTREME_IDS) == 8
    at = [tuple(by_name[n][1:5]) for n in EXTREME_IDS if n.endswith("_at") and by_name[n][5] == ["swipe"]]
    assert at == pk.EXTREME_SWIPE_AT  # the shapes the CPU tier checks against brute force


@pytest.mark.parametrize("name", EXTREME_IDS)
@pytest.mark.parametrize("sem", SEMS, ids=lambda s: s.name)
def test_extreme_mutants_staged(engine, name, sem):
    case = next(c for c in _extremes() if c[0] == name)
    _, L1, lo, hi, w, kernels, forms = case
    prob, want = _extreme_problem(case, 40 if L1 <= 130 else 3, L1, sem)
    engine.set_problem(prob.weights, prob.seq1, sem)
    out = np.full(prob.n, -7, dtype=_lib.RESULT_DTYPE)
    engine.solve(prob.codes, prob.offsets, out=out)
    st = engine.stats()
    assert (st["kernels"], st["forms"]) == (kernels, forms), st
    assert_rows(as_triples(out), want, want[:, 1], f"{name} staged {sem.name}")
    got = engine.solve(prob.codes, prob.offsets, fmt="auto")
    st = engine.stats()
    assert (st["kernels"], st["forms"]) == (kernels, forms), st
    assert_rows(as_triples(got, r2=st["r2"]), want, want[:, 1], f"{name} staged auto format {sem.name}")


SWIPE_EXTREME_IDS = [c[0] for c in _extremes() if c[0] in EXTREME_IDS and c[5] == ["swipe"]]


@pytest.mark.parametrize("name", SWIPE_EXTREME_IDS)
def test_extreme_mutants_wire_p33(name):
    # the rows that run the swipe kernel (one past the RK form's bounds the short kernel has them: staged above)
    case = next(c for c in _extremes() if c[0] == name)
    _, L1, lo, hi, w, kernels, forms = case
    assert kernels == ["swipe"]
    prob, want = _extreme_problem(case, 60, L1 + 1, Semantics.REFERENCE)
    eng = HipSearchEngine(device=0)
    try:
        eng.set_problem(prob.weights, prob.seq1)
        ws = WireSlice.from_csr(prob.codes, prob.offsets, letter_format="p33")
        ws.alloc_results(eng)
        with _lib.Pinned(*ws.arrays()):
            ws.results.view(np.uint8)[:] = POISON
            ws.solve(eng)
        st = eng.stats()
        assert (st["kernels"], st["forms"], st["direct"]) == (kernels, forms, 1), st
        assert_rows(ws.triples(eng), want, want[:, 1], f"{name} pinned p33")
    finally:
        eng.close()
