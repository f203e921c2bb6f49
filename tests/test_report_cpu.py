"""Alignment report on the CPU engine (csrc/src/cpu_engine.cpp report_batch_cpu): counts and marker bytes against
the pure-Python models/scoring.alignment_string, the score invariant W . counts == score on goldens, top-K rows
and planted problems, the defined outputs of empty and invalid rows, format_report, the Python CLI's
--show-alignment (one and several gloo ranks), and the stand-alone sanitizer program."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, expected, input_path
from test_dist import torchrun

from mpi_openmp_cuda_amd import (Problem, Semantics, format_report, format_topk, report_scores, search_cpu,
                                 search_report_cpu, search_topk_cpu)
from mpi_openmp_cuda_amd.models.scoring import alignment_string, decode
from mpi_openmp_cuda_amd.ops.align import REPORT_EMPTY, REPORT_INVALID, as_triples
from mpi_openmp_cuda_amd.utils.synthetic import make_planted

SEMS = [Semantics.REFERENCE, Semantics.SPEC]
INT32_MIN = int(np.iinfo(np.int32).min)
INT32_MAX = int(np.iinfo(np.int32).max)


def python_report(prob: Problem, rows3):
    """counts [n, K, 4] and the marker lines (without the hyphen) of real rows, from alignment_string."""
    n, K = rows3.shape[:2]
    seq1 = decode(prob.seq1)
    counts = np.zeros((n, K, 4), np.int32)
    lines = {}
    for i in range(n):
        seq2 = decode(prob.codes[prob.offsets[i]:prob.offsets[i + 1]])
        for j in range(K):
            s, o, k = (int(v) for v in rows3[i, j])
            if s == INT32_MIN:
                continue
            line = alignment_string(seq1, seq2, o, k)
            if k:
                assert line[k] == "-"
                line = line[:k] + line[k + 1:]
            lines[(i, j)] = line
            counts[i, j] = [line.count(c) for c in "$%# "]
    return counts, lines


def check_real_rows(prob: Problem, rows):
    """Every property the issue lists for rows that a search returned."""
    rows3 = np.asarray(rows, np.int32).reshape(prob.n, -1, 3)
    K = rows3.shape[1]
    counts, marks = search_report_cpu(prob, rows3, marks=True)
    want, lines = python_report(prob, rows3)
    assert counts.shape == (prob.n, K, 4) and counts.dtype == np.int32
    assert np.array_equal(counts, want)
    real = rows3[..., 0] != INT32_MIN
    L2 = np.asarray(prob.lengths, np.int64)
    assert np.array_equal(counts.sum(-1)[real], np.broadcast_to(L2[:, None], real.shape)[real])
    scores = report_scores(counts, prob.weights)
    assert scores.dtype == np.int64 and np.array_equal(scores[real], rows3[..., 0].astype(np.int64)[real])
    assert np.all(scores[~real] == REPORT_EMPTY) and not counts[~real].any()
    assert marks.dtype == np.uint8 and marks.shape == (K * prob.total_chars,)
    for i in range(prob.n):
        for j in range(K):
            at = K * int(prob.offsets[i]) + j * int(L2[i])
            got = marks[at:at + int(L2[i])]
            if real[i, j]:
                assert got.tobytes().decode() == lines[(i, j)], (i, j)
            else:
                assert not got.any(), (i, j)
    # without marks: the same counts, one array
    assert np.array_equal(search_report_cpu(prob, rows3), counts)
    return counts, marks


@pytest.mark.parametrize("i", range(1, 7))
def test_golden_rows(i):
    prob = Problem.read(input_path(i))
    rows = as_triples(search_cpu(prob))
    assert "".join(f"#{q}: score: {s}, n: {o}, k: {k}\n" for q, (s, o, k) in enumerate(rows)) == expected(i)
    counts, _ = check_real_rows(prob, rows)
    flat = search_report_cpu(prob, rows)  # [n, 3] rows give [n, 4] counts
    assert flat.shape == (prob.n, 4) and np.array_equal(flat, counts[:, 0])
    assert np.array_equal(search_report_cpu(prob, search_cpu(prob)), flat)  # structured rows, too


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("i", range(1, 7))
def test_topk_rows(i, sem):
    prob = Problem.read(input_path(i))
    check_real_rows(prob, search_topk_cpu(prob, 3, sem))


@pytest.mark.parametrize("sem", SEMS)
def test_planted_rows(sem):
    for L1, L2 in ((40, 1), (40, 7), (64, 33), (300, 130), (90, 90)):
        prob, _ = make_planted(L1, L2, (10, 2, 3, 4), seed=L2)
        rows = as_triples(search_cpu(prob, sem))
        counts, _ = check_real_rows(prob, rows)
        if sem == Semantics.SPEC:  # every record is found where it was planted: all pairs identical
            assert np.array_equal(counts[:, 0], np.tile([L2, 0, 0, 0], (prob.n, 1)))


def test_topk_padding_rows_are_empty():
    prob = Problem.read(input_path(5))
    L1 = prob.L1
    # records of L1 - 1 and L1 letters have 1..2 candidate offsets: K = 64 is mostly padding
    recs = [prob.seq1[:L1 - 1], prob.seq1[:L1], prob.seq1[1:L1]]
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)
    p = Problem(prob.weights, prob.seq1, np.concatenate(recs).astype(np.uint8), offsets)
    rows = search_topk_cpu(p, 64, Semantics.SPEC)
    assert (rows[..., 0] == INT32_MIN).sum() >= 64 * 3 - 5
    check_real_rows(p, rows)


def test_invalid_rows():
    seq1 = np.arange(1, 21, dtype=np.uint8)  # L1 = 20
    recs = [seq1[3:8], seq1, np.concatenate([seq1, [1]]).astype(np.uint8), seq1[:1]]  # L2 = 5, 20, 21, 1
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)
    prob = Problem([10, 2, 3, 4], seq1, np.concatenate(recs).astype(np.uint8), offsets)
    bad = [-1, INT32_MIN, INT32_MAX, 1 << 30]
    pairs = [(a, b) for a in bad for b in bad] + [(a, 0) for a in bad] + [(0, b) for b in bad]
    pairs += [(INT32_MAX - 2, 1), (INT32_MAX - 4, 0), (0, 5), (16, 0), (15, 1), (0, 20), (0, 21)]
    L2 = prob.lengths
    for o, k in pairs:
        rows = np.tile(np.array([[7, o, k]], np.int64), (prob.n, 1))
        counts, marks = search_report_cpu(prob, rows, marks=True)
        for i in range(prob.n):
            valid = (1 <= L2[i] <= 20 and 0 <= k <= L2[i] - 1 and o >= 0 and o + L2[i] + (1 if k > 0 else 0) <= 20)
            m = marks[prob.offsets[i]:prob.offsets[i + 1]]
            if valid:
                assert counts[i].sum() == L2[i] and m.all(), (o, k, i)
            else:
                assert np.array_equal(counts[i], [-1, -1, -1, -1]) and not m.any(), (o, k, i)
        s = report_scores(counts, prob.weights)
        assert np.all((s == REPORT_INVALID) == (counts[:, 0] < 0))
    # the edges of validity: the spec-only final offset and the L2 == L1 row are valid, L2 > L1 never is
    rows = np.array([[0, 15, 0], [0, 0, 0], [0, 0, 0], [0, 19, 0]], np.int32)
    counts = search_report_cpu(prob, rows)
    assert counts[0].sum() == 5 and counts[0].min() >= 0
    assert np.array_equal(counts[1], [20, 0, 0, 0]) and np.array_equal(counts[2], [-1] * 4) and counts[3].sum() == 1
    # an empty record (L2 == 0) is invalid unless its row is empty
    p0 = Problem([1, 1, 1, 1], seq1, np.zeros(0, np.uint8), np.zeros(2, np.int64))
    assert np.array_equal(search_report_cpu(p0, [[5, 0, 0]]), [[-1] * 4])
    assert np.array_equal(search_report_cpu(p0, [[INT32_MIN, 0, 0]]), [[0] * 4])
    # an empty row wins over everything else in it
    e = search_report_cpu(prob, np.tile(np.array([[INT32_MIN, -5, INT32_MAX]], np.int64), (prob.n, 1)))
    assert not e.any() and np.all(report_scores(e, prob.weights) == REPORT_EMPTY)
    with pytest.raises(ValueError):
        search_report_cpu(prob, np.zeros((prob.n, 65, 3), np.int32))
    with pytest.raises(ValueError):
        search_report_cpu(prob, np.zeros((prob.n + 1, 3), np.int32))


def text_from_alignment_string(prob: Problem, rows3) -> str:
    seq1 = decode(prob.seq1)
    out = []
    for i in range(prob.n):
        seq2 = decode(prob.codes[prob.offsets[i]:prob.offsets[i + 1]])
        for j, (s, o, k) in enumerate(rows3[i].tolist()):
            if j and s == INT32_MIN:
                continue
            out.append(f"#{i}: score: {s}, n: {o}, k: {k}\n" if j == 0 else f"#{i}.{j + 1}: score: {s}, n: {o}, k: {k}\n")
            if s == INT32_MIN:
                continue
            line = alignment_string(seq1, seq2, o, k)
            body = line.replace("-", "")
            out.append(f"  $: {body.count('$')}, %: {body.count('%')}, #: {body.count('#')}, space: {body.count(' ')}\n")
            out.append(f"  {seq1[o:o + len(seq2) + (1 if k else 0)]}\n")
            out.append(f"  {line}\n")
            out.append(f"  {seq2[:k] + '-' + seq2[k:] if k else seq2}\n")
    return "".join(out)


def report_text(prob: Problem, rows) -> str:
    counts, marks = search_report_cpu(prob, rows, marks=True)
    return format_report(prob, rows, counts, marks)


@pytest.mark.parametrize("i", [5, 6])
def test_format_report(i):
    prob = Problem.read(input_path(i))
    rows = as_triples(search_cpu(prob))
    text = report_text(prob, rows)
    assert text == text_from_alignment_string(prob, rows.reshape(prob.n, 1, 3))
    # dropping the indented lines leaves today's output
    assert "".join(l + "\n" for l in text.splitlines() if not l.startswith("  ")) == expected(i)
    top = search_topk_cpu(prob, 3)
    ttext = report_text(prob, top)
    assert ttext == text_from_alignment_string(prob, top)
    assert "".join(l + "\n" for l in ttext.splitlines() if not l.startswith("  ")) == format_topk(top)
    if i == 5:  # the issue's example, letter for letter
        assert text == ("#0: score: 27, n: 0, k: 5\n  $: 4, %: 2, #: 3, space: 0\n  APQRSBATAV\n  $#$$#-$#%%\n"
                        "  ASQRE-AVSL\n")


def _cli(args, i):
    with open(input_path(i), "rb") as f:
        return subprocess.run([sys.executable, "-m", "mpi_openmp_cuda_amd", "--backend=cpu"] + args, stdin=f,
                              capture_output=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd="/tmp", timeout=120)


@pytest.mark.parametrize("i,nproc,top", [(5, 1, 1), (6, 1, 3), (1, 1, 1), (6, 3, 1), (2, 3, 3)])
def test_cli_show_alignment(i, nproc, top):
    prob = Problem.read(input_path(i))
    want = report_text(prob, search_topk_cpu(prob, 3) if top > 1 else as_triples(search_cpu(prob)))
    args = ["--show-alignment"] + (["--top", str(top)] if top > 1 else [])
    if nproc == 1:
        r = _cli(args, i)
    else:
        r = torchrun(nproc, ["--backend=cpu", "--dist-backend=gloo", f"--input={input_path(i)}"] + args)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert r.stdout.decode() == want


@pytest.mark.parametrize("i", range(1, 7))
def test_cli_without_the_flag_is_todays_output(i):
    r = _cli([], i)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout.decode() == expected(i)


def test_cli_show_alignment_needs_record_slices():
    r = _cli(["--show-alignment", "--partition", "offsets"], 1)
    assert r.returncode != 0 and b"--partition records" in r.stderr and r.stdout == b""


def test_report_sanitizer_program():
    """csrc/tests/report_san.cpp with the CPU core sources under ASan + UBSan: a plain program with its own main
    (nothing is loaded into Python, nothing runs on a GPU)."""
    r = subprocess.run(["make", "-C", ROOT, "-s", "-j8", "report-san"], capture_output=True, timeout=600)
    out = (r.stdout + r.stderr).decode()
    assert r.returncode == 0, out[-3000:]
    assert "report_san ok" in out and "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]
