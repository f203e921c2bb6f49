"""The staged pipeline's cut and the cases of its GPU tier, CPU tier (no GPU).

a. ``ops.align.staged_chunks`` (plan::staged_chunk_end through the C ABI, what HipEngine::run_staged calls) against
   a Python-int model of the rule and against a copy of the loop run_staged had before the cut moved out of it, on a
   hand list of the rule's edges and a seeded sweep; the rule's properties.
b. The batches of tests/staged_chunks.py reach what tests/test_gpu_staged_chunks.py runs them for: every byte
   residue and every 5-bit phase at a chunk's start, result blocks off the 16-byte boundary, the stated chunk counts,
   slots that must grow, the stated kernel for every segment.
c. Their expected rows tell a fault from none: a slot reused without new results, rows never written, a result block
   placed a row early or late or with another format's row size, a 5-bit chunk decoded one bit off."""
import bisect

import numpy as np
import pytest

import staged_chunks as sc
from mpi_openmp_cuda_amd import Semantics
from mpi_openmp_cuda_amd.models.reference import prefix_oracle
from mpi_openmp_cuda_amd.models.scoring import score_table
from mpi_openmp_cuda_amd.ops.align import kernel_bounds, staged_chunks


def legacy_chunks(offsets, chunk_records, chunk_bytes):
    """HipEngine::run_staged's cut as it stood inside the engine (std::min, std::upper_bound, std::max), line by
    line."""
    off = [int(x) for x in offsets]
    n = len(off) - 1
    bounds, rb = [0], 0
    while rb < n:
        re = min(n, rb + chunk_records)
        byte_cap = off[rb] + chunk_bytes
        if off[re] > byte_cap:
            re = bisect.bisect_right(off, byte_cap, rb + 1, re + 1) - 1
            re = max(re, rb + 1)
        bounds.append(re)
        rb = re
    return bounds


def check_properties(offsets, bounds, R, B):
    off = [int(x) for x in offsets]
    n = len(off) - 1
    assert bounds[0] == 0 and bounds[-1] == n, bounds            # a partition of [0, n)
    for a, b in zip(bounds, bounds[1:]):
        assert b > a, f"empty or stuck chunk at record {a}: {bounds}"
        assert (b - a <= R and off[b] - off[a] <= B) or b - a == 1, (a, b)  # over a limit: a single record only
        assert b - a <= R


# ---- a. the rule ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.HAND, ids=[c[0] for c in sc.HAND])
def test_hand_list(case):
    _, lengths, base, R, B, want = case
    offsets = sc.hand_offsets(lengths, base)
    got = staged_chunks(offsets, R, B).tolist()
    assert got == want
    assert sc.model_chunks(offsets, R, B) == want
    assert legacy_chunks(offsets, R or sc.DEFAULT_R, B or sc.DEFAULT_B) == want
    check_properties(offsets, got, R or sc.DEFAULT_R, B or sc.DEFAULT_B)


@pytest.mark.parametrize("name", sc.CUT_BATCHES)
def test_cut_cases_of_the_gpu_batches(name):
    b = sc.batch(name)
    n, lengths = b.n, b.lengths.tolist()
    assert int(b.offsets[0]) == sc.BASE == 12345
    seen = {}
    for tag, R, B in sc.cut_cases(lengths):
        got = staged_chunks(b.offsets, R, B).tolist()
        assert got == sc.model_chunks(b.offsets, R, B) == legacy_chunks(b.offsets, R or sc.DEFAULT_R, B or sc.DEFAULT_B), tag
        check_properties(b.offsets, got, R or sc.DEFAULT_R, B or sc.DEFAULT_B)
        seen[tag] = got
    j = n // 3
    assert seen["bytes_exact"][1] == j and seen["bytes_one_less"][1] == j - 1
    assert seen["bytes_one_more"][1] == j + (1 if lengths[j] == 1 else 0)
    over = [i for i, l in enumerate(lengths) if l == max(lengths)]
    assert {0, n // 2, n - 1} <= set(over)  # a record longer than chunk_bytes first, in the middle and last ...
    for i in over:                         # ... each a chunk of its own
        assert i in seen["record_over_bytes"] and i + 1 in seen["record_over_bytes"]
    assert len(seen["bytes_1"]) - 1 == n == len(seen["records_1"]) - 1
    assert seen["records_n_minus_1"] == [0, n - 1, n] and seen["records_n"] == [0, n] == seen["records_n_plus_1"]
    sizes = {(b1 - a) for a, b1 in zip(seen["both_limits"], seen["both_limits"][1:])}
    assert 7 in sizes and len(sizes) > 1  # some chunks end at the record limit, others at the byte limit
    if name == "mixed300":
        assert max(lengths) > b.prob.L1  # records longer than Seq1


def test_seeded_sweep():
    rng = np.random.default_rng(20)
    for it in range(400):
        n = int(rng.integers(1, 60))
        lengths = rng.integers(1, 12 if it % 3 else 400, n)
        offsets = sc.hand_offsets(lengths, int(rng.integers(0, 1 << 40)))
        R, B = int(rng.integers(1, n + 3)), int(rng.integers(1, 500))
        got = staged_chunks(offsets, R, B).tolist()
        assert got == sc.model_chunks(offsets, R, B), (it, lengths.tolist(), R, B)
        assert got == legacy_chunks(offsets, R, B)
        check_properties(offsets, got, R, B)


def test_degenerate_and_refused_inputs():
    from mpi_openmp_cuda_amd._lib import NativeError

    assert staged_chunks([7]).tolist() == [0]  # no records: no chunk
    assert staged_chunks([0, 5], 1, 1).tolist() == [0, 1]
    with pytest.raises(NativeError):
        staged_chunks([0, 5, 3])
    with pytest.raises(NativeError):
        staged_chunks([0, 5], -1, 0)
    with pytest.raises(ValueError):
        staged_chunks([])


# ---- b. the GPU cases reach what they claim ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["phase_swipe", "phase_tile16"])
def test_phase_cases_start_at_every_residue_and_bit_phase(name):
    b = sc.batch(name)
    bounds = b.bounds(sc.PHASE_R)
    assert bounds == list(range(0, b.n + 1, sc.PHASE_R)) and len(bounds) - 1 == sc.PHASE_CHUNKS == 48
    starts = [int(b.offsets[rb]) for rb in bounds[:-1]]
    assert {s % 16 for s in starts} == set(range(16))       # the copy kernel's byte loop against its 16-byte loop
    assert {(5 * s) % 8 for s in starts} == set(range(8))   # pbit of the staged unpack5
    if name == "phase_swipe":
        assert all(int(b.offsets[bounds[c + 1]] - b.offsets[bounds[c]]) == 17 for c in range(48))
        assert sc.chunk_kernels(b, bounds) == ["swipe"]
    else:
        assert b.lengths.min() == 40 and b.lengths.max() == 90
        assert sc.chunk_kernels(b, bounds) == ["tile16"]


def test_cut_batches_take_the_stated_kernels():
    b = sc.batch("swipe6")
    for _, R, B in sc.cut_cases(b.lengths):
        assert sc.chunk_kernels(b, b.bounds(R, B)) == ["swipe"]  # every chunk, whatever the cut
    m = sc.batch("mixed300")
    assert sc.chunk_kernels(m, m.bounds()) == ["short", "tile16"]


@pytest.mark.parametrize("fmt,fb", [("r2", 2), ("r4", 4), ("r8", 8), ("r12", 12)])
def test_placement_cases_leave_the_16_byte_boundary(fmt, fb):
    b = sc.batch("placement")
    bounds = b.bounds(sc.PLACEMENT_R)
    assert len(bounds) - 1 == -(-sc.PLACEMENT_N // sc.PLACEMENT_R)
    off16 = [rb for rb in bounds[1:-1] if (rb * fb) % 16]
    assert len(off16) >= len(bounds) // 2, (fmt, len(off16))
    assert sc.FORMAT_BYTES[fmt] == fb and (bounds[1] * fb) % 16 != 0
    # R2 and the nibble lengths hold the batch (test_r2_results_and_nibble_lengths' request)
    assert b.lengths.min() == 6 and b.lengths.max() == 11
    sc.r2_stand_in(b.rows())
    assert sc.PLACEMENT_N * 2 > 2 * 4096  # the smallest results span more than two pages


@pytest.mark.parametrize("count", sc.RING_COUNTS)
def test_ring_cases_have_the_stated_chunk_counts(count):
    b = sc.batch("ring")
    bounds = b.bounds(sc.ring_records(count))
    assert len(bounds) - 1 == count and staged_chunks(b.offsets, sc.ring_records(count)).tolist() == bounds


@pytest.mark.parametrize("name", ["growth", "growth_reversed"])
def test_growth_case_outgrows_the_slot(name):
    b = sc.batch(name)
    bounds = b.bounds(sc.GROWTH_R)
    letters = [int(b.offsets[e] - b.offsets[a]) for a, e in zip(bounds, bounds[1:])]
    assert len(letters) == len(sc.GROWTH_LENGTHS) == 8
    if name == "growth_reversed":
        letters = letters[::-1]  # later chunks are smaller: the slot keeps the bytes of the larger one
    assert min(letters) >= sc.GROWTH_FLOOR
    for c in range(2, len(letters)):
        assert letters[c] > sc.GROWTH_FACTOR * letters[c - 2] + sc.GROWTH_PAD, (c, letters)
    assert sc.chunk_kernels(b, bounds) == ["tile16"]


@pytest.mark.parametrize("wname", list(sc.KERNEL_WEIGHTS))
def test_every_segment_alone_classifies_as_stated(wname):
    w = sc.KERNEL_WEIGHTS[wname]
    for seg in sc.SEGMENTS:
        b = sc.batch(f"kernels_{wname}_{seg}")
        assert b.n == sc.SEGMENT and b.prob.L1 == sc.KERNEL_L1
        assert sc.classify(w, sc.KERNEL_L1, b.lengths) == sc.STATED[wname][seg], seg
    # the length rules behind the statements
    L = {seg: sc.batch(f"kernels_{wname}_{seg}").lengths for seg in sc.SEGMENTS}
    short_from = sc.KERNEL_L1 - 63
    assert L["swipe"].min() >= short_from and L["swipe"].max() <= 128
    assert (kernel_bounds(w, 150, int(L["swipe"].min()), int(L["swipe"].max()))["swipe"] is not None) == (wname == "w10")
    assert L["short"].min() >= 130 and 0 < (L["short"] > 150).sum() < 8 and L["short"].max() <= 200
    assert L["tile16"].max() < short_from
    assert sorted(set(L["short_tile16"].tolist())) == [20, 100] and 20 < short_from <= 100
    assert L["unsearchable"].min() > 150
    assert (L["long20k"] == 20_000).sum() == 1 and (L["long60k"] == 60_000).sum() == 1
    # the whole batch: chunks of 40 records are the segments; chunks of 30 straddle them
    whole = sc.batch(f"kernels_{wname}_all")
    assert whole.n == sc.SEGMENT * len(sc.SEGMENTS)
    assert whole.bounds(40) == list(range(0, whole.n + 1, 40))
    assert np.array_equal(whole.lengths, np.concatenate([L[s] for s in sc.SEGMENTS]))
    assert sc.chunk_kernels(whole, whole.bounds(40)) == sc.union_kernels(sc.STATED[wname].values())
    if wname == "w10":
        for R in (40, 30):
            assert sc.chunk_kernels(whole, whole.bounds(R)) == ["swipe", "short", "tile16"]


def test_unsearchable_segment_has_no_candidate_anywhere():
    for sem in (Semantics.REFERENCE, Semantics.SPEC):
        rows = sc.batch("kernels_w10_unsearchable").rows(sem)
        assert (rows == (sc.INT_MIN, 0, 0)).all()


# ---- c. the cases tell a fault from none -----------------------------------------------------------------------
def multi_chunk_cases():
    out = [(name, R, B) for name in sc.CUT_BATCHES for _, R, B in sc.cut_cases(sc.batch(name).lengths)]
    out += [("ring", sc.ring_records(c), 0) for c in sc.RING_COUNTS]
    out += [("growth", sc.GROWTH_R, 0), ("growth_reversed", sc.GROWTH_R, 0), ("placement", sc.PLACEMENT_R, 0),
            ("phase_swipe", sc.PHASE_R, 0), ("phase_tile16", sc.PHASE_R, 0)]
    out += [(f"kernels_{w}_all", R, 0) for w in sc.KERNEL_WEIGHTS for R in (40, 30)]
    return out


def test_a_stale_slot_would_show():
    """Chunks c and c - 2 share a slot: had chunk c's results not arrived, its rows would be those of chunk c - 2
    at the same positions."""
    for name, R, B in multi_chunk_cases():
        b = sc.batch(name)
        for sem in (Semantics.REFERENCE, Semantics.SPEC):
            rows, bounds = b.rows(sem), b.bounds(R, B)
            for c in range(2, len(bounds) - 1):
                m = min(bounds[c + 1] - bounds[c], bounds[c - 1] - bounds[c - 2])
                mine, stale = rows[bounds[c]:bounds[c] + m], rows[bounds[c - 2]:bounds[c - 2] + m]
                assert not np.array_equal(mine, stale), (name, R, B, c)


def test_no_expected_row_is_the_poison():
    poison = np.full(3, sc.POISON, np.uint8).repeat(4).view(np.int32)  # 0x5A5A5A5A three times
    for name, _, _ in multi_chunk_cases():
        rows = sc.batch(name).rows()
        assert not (rows == poison).all(axis=1).any(), name
        assert not (rows[:, 0] == poison[0]).any(), name
    # ... in any format's bytes: a narrow row of poison bytes decodes to none of the expected rows
    b = sc.batch("placement")
    r2 = sc.r2_stand_in(b.rows())
    for fmt in sc.FORMAT_BYTES:
        data = sc.encode_rows(b.rows(), fmt, r2).reshape(b.n, -1)
        assert not (data == sc.POISON).all(axis=1).any(), fmt


@pytest.mark.parametrize("fmt", list(sc.FORMAT_BYTES))
def test_a_misplaced_result_block_would_show(fmt):
    b = sc.batch("placement")
    rows, bounds = b.rows(), b.bounds(sc.PLACEMENT_R)
    r2 = sc.r2_stand_in(rows)
    right, intact = sc.place_blocks(rows, bounds, fmt, r2)
    assert np.array_equal(right, rows) and intact
    for shift in (-1, 1):
        got, _ = sc.place_blocks(rows, bounds, fmt, r2, row_shift=shift)
        assert not np.array_equal(got, rows), shift
    for other in sc.FORMAT_BYTES.values():
        if other != sc.FORMAT_BYTES[fmt]:
            got, _ = sc.place_blocks(rows, bounds, fmt, r2, place_fb=other)
            assert not np.array_equal(got, rows), other


@pytest.mark.parametrize("name", ["phase_swipe", "phase_tile16"])
def test_a_wrong_bit_phase_would_show(name):
    """The first record of every chunk is a copy of Seq1: its row is the claim, a changed first letter changes the
    row, and so does the chunk's 5-bit stream read one bit early or late."""
    b = sc.batch(name)
    table = score_table(b.prob.weights)
    w1 = b.prob.weights.as_list()[0]
    packed = b.packed5()
    rows = b.rows()
    for c, rb in enumerate(b.bounds(sc.PHASE_R)[:-1]):
        L2, start = int(b.lengths[rb]), int(b.offsets[rb])
        want = (w1 * L2, sc.phase_position(b, c), 0)
        assert tuple(rows[rb]) == want == tuple(b.rows(Semantics.SPEC)[rb]), c
        rec = b.codes[start:start + L2]
        assert np.array_equal(sc.unpack5_at(packed[(5 * start) // 8:], (5 * start) % 8, L2), rec)  # the right phase
        other = rec.copy()
        other[0] = other[0] % 26 + 1
        assert prefix_oracle(table, b.prob.seq1, other) != want
        for slip in (-1, 1):
            bit0 = (5 * start) % 8 + slip + 8  # one byte of the stream in front: the slip may reach into it
            got = sc.unpack5_at(packed[(5 * start) // 8 - 1:], bit0, L2)
            assert prefix_oracle(table, b.prob.seq1, got) != want, (c, slip)


# ---- ./final --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [["--chunk-records=3", "--chunk-bytes=4096"], ["--chunk-records=1"]])
def test_final_cpu_accepts_the_chunk_flags(flags):
    # the flags size the GPU ranks' staged pipeline (tests/test_gpu_staged_chunks.py); a CPU job takes them and
    # prints the golden, and its --timing line counts no chunks
    import json

    from conftest import expected, input_path, run_final

    r = run_final(["--backend=cpu", "--timing"] + flags, stdin_path=input_path(3), np_=2)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout.decode() == expected(3)
    d = json.loads([l for l in r.stderr.decode().splitlines() if l.startswith("{")][-1])
    assert d["rank_chunks"] == [0, 0], d
