"""Case lists shared by the CPU and GPU tiers of the per-target distinct placements (tests/test_targets_peaks_cpu.py,
tests/test_gpu_targets_peaks.py), and a numpy model of the SHORTCUT the kernels must not take: the catalog-wide peak
filter's marks cut to each target's slice. No test in here.

hostile_case: one record of five letters against a chain of targets whose pair profiles have exactly the asked sizes.
Every target starts with the record's last two letters and ends with its first three, so the catalog holds a full
match of the record across EVERY target edge, three letters before each target's start: for the pair of a target it
is the catalog entry 3 before its first own entry and the one 2 past its boundary offset, and it outscores everything
inside (a full match is the largest score there is). A window that leaks across either edge, or that reads the
catalog's own value at the boundary offset, changes the marks next to the edges."""
import numpy as np

from mpi_openmp_cuda_amd import Problem, Semantics, TargetSet, search_profile_cpu, search_targets_hits_cpu

W = (4, 3, 2, 10)
I32 = np.iinfo(np.int32)
HOSTILE_L2 = 5

# pair-profile sizes: around every segment width and the wave / tile cut; the tile kernel's edges
SIZES_SEG4 = [1, 2, 3, 4]
SIZES_SEG8 = [1, 2, 3, 4, 5, 7, 8]
SIZES_SEG16 = [1, 2, 3, 4, 5, 8, 9, 15, 16]
SIZES_SEG32 = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32]
SIZES_SHORT = [1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65]
SIZES_TILE = [2047, 2048, 2049, 4097]
RADII_SHORT = [1, 2, 3, 15, 16, 63, 64, 2048]
RADII_TILE = [1, 63, 64, 2048]
# name -> (sizes, radii): what the GPU tier runs to test clipping
CLIPPING_CASES = {
    "seg4": (SIZES_SEG4, [1, 2, 3]),
    "seg8": (SIZES_SEG8, [1, 2, 3, 7]),
    "seg16": (SIZES_SEG16, [1, 2, 3, 15, 16]),
    "seg32": (SIZES_SEG32, [1, 3, 16, 31, 32]),
    "short": (SIZES_SHORT, RADII_SHORT),
    "tile": (SIZES_TILE + [64, 65], RADII_TILE),
}


def batch_of(recs):
    lens = np.array([len(r) for r in recs], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    codes = np.concatenate([np.asarray(r, np.uint8) for r in recs]) if len(recs) else np.zeros(0, np.uint8)
    return codes, offsets


def target_len(count, L2, sem):
    """Letters of a target whose pair profile with a record of L2 letters has `count` entries."""
    if count == 1:
        return L2  # the boundary entry alone, under both semantics
    return L2 + count - 1 if Semantics.parse(sem) == Semantics.SPEC else L2 + count


def hostile_case(sizes, sem, seed=5):
    """(problem, target set): target 1 + j has a pair profile of sizes[j] entries; a first and a last target close the
    chain, so every asked target is a middle one with a full match across both of its edges."""
    rng = np.random.default_rng(seed)
    rec = rng.integers(1, 27, HOSTILE_L2).astype(np.uint8)
    seqs = []
    for c in [7] + list(sizes) + [7]:
        t = rng.integers(1, 27, target_len(c, HOSTILE_L2, sem)).astype(np.uint8)
        t[:2] = rec[3:]
        t[-3:] = rec[:3]
        seqs.append(t)
    ts = TargetSet.from_sequences(seqs)
    codes, offsets = batch_of([rec])
    return Problem(list(W), ts.seq1, codes, offsets), ts


def pair_counts(prob, ts, sem):
    """int64 [n, T]: entries of every pair's profile (0: the record does not fit the target)."""
    L2 = np.diff(prob.offsets)[:, None]
    ln = ts.lengths[None, :]
    spec = Semantics.parse(sem) == Semantics.SPEC
    return np.where((L2 >= 1) & (L2 <= ln), ln - L2 + np.where(spec | (ln == L2), 1, 0), 0)


def expected_masks(prob, ts, sem, radius):
    """Per pair (i, t) a bool array over its profile: the peaks the CPU engine lists with every score admitted."""
    rows, toffsets = search_targets_hits_cpu(prob, ts, min_score=int(I32.min), semantics=sem, radius=radius)
    counts = pair_counts(prob, ts, sem)
    out = {}
    for i in range(prob.n):
        for t in range(ts.T):
            m = np.zeros(int(counts[i, t]), bool)
            p = i * ts.T + t
            m[rows[toffsets[p]:toffsets[p + 1], 1]] = True
            out[i, t] = m
    return out


def _keys(scores):
    o = np.arange(scores.shape[0], dtype=np.uint64)
    return ((scores.astype(np.int64) + 2 ** 31).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xffffffff) - o)


def window_peaks(scores, radius):
    """peaks_filter in numpy: entry o is a peak iff its key is the largest in [o - radius, o + radius]."""
    k = _keys(np.asarray(scores))
    C = k.shape[0]
    return np.array([k[o] == k[max(0, o - radius):min(C, o + radius + 1)].max() for o in range(C)], bool)


def shortcut_masks(prob, ts, sem, radius):
    """The shortcut: the peak filter over each record's whole catalog profile, its marks cut to every target's slice
    (the catalog's own value standing in for the boundary entry; a mark past the record's entries counts as set)."""
    prof, poff = search_profile_cpu(prob, sem)
    counts = pair_counts(prob, ts, sem)
    out = {}
    for i in range(prob.n):
        whole = window_peaks(prof["score"][poff[i]:poff[i + 1]], radius)
        for t in range(ts.T):
            b, c = int(ts.starts[t]), int(counts[i, t])
            m = np.ones(c, bool)
            have = whole[b:b + c]
            m[:have.shape[0]] = have
            out[i, t] = m
    return out


def count_disagreements(prob, ts, sem, radius):
    """(pairs on which the shortcut's marks differ from the expected ones, fitting pairs)."""
    want, cut = expected_masks(prob, ts, sem, radius), shortcut_masks(prob, ts, sem, radius)
    fitting = [p for p, m in want.items() if m.shape[0] > 0]
    return sum(0 if np.array_equal(want[p], cut[p]) else 1 for p in fitting), len(fitting)
