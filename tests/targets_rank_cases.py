"""Helpers and case lists shared by the CPU and GPU tiers of the target ranking (tests/test_targets_rank_cpu.py,
tests/test_gpu_targets_rank.py): batches, the numpy model of the ranking (a stable sort of search_targets_cpu's rows),
and a Python-int model of the chunk cut."""
import numpy as np

from mpi_openmp_cuda_amd import Problem, Semantics, TargetSet

SEMS = [Semantics.REFERENCE, Semantics.SPEC]
I32 = np.iinfo(np.int32)
W = (4, 3, 2, 10)
PAD = [-1, I32.min, 0, 0]


def batch_of(recs):
    lens = np.array([len(r) for r in recs], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    codes = np.concatenate([np.asarray(r, np.uint8) for r in recs]) if len(recs) else np.zeros(0, np.uint8)
    return codes, offsets


def random_case(seed, target_lens, record_lens, alphabet=4, weights=W):
    rng = np.random.default_rng(seed)
    ts = TargetSet.from_sequences([rng.integers(1, alphabet + 1, int(l)) for l in target_lens])
    codes, offsets = batch_of([rng.integers(1, alphabet + 1, int(l)) for l in record_lens])
    return Problem(list(weights), ts.seq1, codes, offsets), ts


def fitting(prob, ts):
    """F_i: the targets each record fits (1 <= L2 <= len_t), int [n]."""
    L2 = np.diff(prob.offsets)
    return ((L2[:, None] >= 1) & (L2[:, None] <= ts.lengths[None, :])).sum(axis=1)


def rank_model(rows, M):
    """The ranking of multi-target rows [n, T, 3] by its definition: the rows that fit (score not INT32_MIN), stably
    sorted by descending score — so equal scores keep ascending t — cut or padded to M rows (t, score, n, k)."""
    rows = np.asarray(rows)
    n, T, _ = rows.shape
    out = np.empty((n, M, 4), np.int32)
    out[:] = PAD
    for i in range(n):
        fit = [t for t in range(T) if rows[i, t, 0] != I32.min]
        order = sorted(fit, key=lambda t: -int(rows[i, t, 0]))  # sorted() is stable
        for j, t in enumerate(order[:M]):
            out[i, j] = [t, *rows[i, t]]
    return out


def entries_of(L1, L2, sem):
    """candidate_offsets (csrc/src/cpu_engine.cpp) in Python ints."""
    if L2 > L1 or L2 <= 0:
        return 0
    if L2 == L1:
        return 1
    return L1 - L2 + (1 if Semantics.parse(sem) == Semantics.SPEC else 0)


def chunks_model(L1, lengths, T, scratch_bytes, sem):
    """The rank call's cut in Python ints: a chunk takes records while 8 * entries + 12 * T * records <=
    scratch_bytes, at least one; T = 0 is the cut of top-K and hits, records while entries <= max(1, scratch // 8)."""
    bounds, r0, n = [0], 0, len(lengths)
    ent = [entries_of(L1, int(l), sem) for l in lengths]
    while r0 < n:
        r1, e = r0 + 1, ent[r0]
        while r1 < n:
            e2 = e + ent[r1]
            ok = e2 <= max(1, scratch_bytes // 8) if T == 0 else 8 * e2 + 12 * T * (r1 + 1 - r0) <= scratch_bytes
            if not ok:
                break
            e, r1 = e2, r1 + 1
        bounds.append(r1)
        r0 = r1
    return bounds


def straddling_case():
    """The README's straddling record: the last 20 letters of target 1 followed by the first 20 of target 2."""
    rng = np.random.default_rng(2024)
    t1, t2 = (rng.integers(1, 27, size=60).astype(np.uint8) for _ in range(2))
    ts = TargetSet.from_sequences([t1, t2])
    codes, offsets = batch_of([np.concatenate([t1[40:], t2[:20]])])
    return Problem(list(W), ts.seq1, codes, offsets), ts


def around_m_case(T, M, seed=0):
    """T targets of 1 .. 6 letters (in a shuffled order) and up to six records chosen so that the records have T,
    M + 1, M, M - 1, 1 and 0 fitting targets (the counts among them that are distinct and at most T): record j has
    j + 1 letters and fits the targets of at least j + 1 letters. Returns (problem, target set, the records' counts)."""
    wanted = sorted({c for c in (0, 1, M - 1, M, M + 1, T) if 0 <= c <= T}, reverse=True)  # descending counts
    target_lens = []
    for j, c in enumerate(wanted):  # the targets of exactly j + 1 letters fit record j and not record j + 1
        nxt = wanted[j + 1] if j + 1 < len(wanted) else 0
        target_lens += [j + 1] * (c - nxt)
    assert len(target_lens) == T
    record_lens = [j + 1 for j in range(len(wanted))]
    rng = np.random.default_rng(seed + 1000 * T + M)
    order = rng.permutation(T)
    prob, ts = random_case(seed + 17 * T + M, [target_lens[o] for o in order], record_lens)
    assert fitting(prob, ts).tolist() == wanted
    return prob, ts, wanted
