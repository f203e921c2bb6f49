"""CPU-tier check of the slice-contract inputs (tests/csr_slices.py): with the CPU engine alone, every family's
``slice_case`` must tell a leak from none — a base one letter off changes at least half of the rows, and one
neighbour letter too many per record changes a score. The GPU tier (tests/test_gpu_csr_slices.py) relies on it:
a kernel that rebases or stages wrongly cannot return the oracle's rows by accident."""
import numpy as np
import pytest

from csr_slices import FAMILIES, FILLS, TAIL, family_case, slice_case

from mpi_openmp_cuda_amd import Problem, search_cpu
from mpi_openmp_cuda_amd.ops.align import as_triples


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_layout(name):
    case = family_case(name, 32 + 13)
    sub, total = case.sub, int(case.sub.offsets[-1])
    assert case.c0 == 45 and np.array_equal(case.offsets, sub.offsets + 45) and case.offsets.dtype == np.int64
    assert np.array_equal(np.diff(sub.offsets), FAMILIES[name][2]())
    for fill in FILLS:
        st = case.storage(fill)
        assert st.dtype == np.uint8 and st.shape[0] == 45 + total + TAIL
        assert np.array_equal(st[45:45 + total], sub.codes)
        assert st.min() >= 1 and st.max() <= 26  # letter 0 would add an all-zero table row and hide a leak
        assert np.array_equal(case.storage(fill, tail=False), st[:45 + total])
    assert (case.storage("A")[:45] == 1).all() and (case.storage("A")[45 + total:] == 1).all()
    # the records do not depend on where the slice lies
    other = family_case(name, 3 * 65536 + 13)
    assert np.array_equal(other.sub.codes, sub.codes) and np.array_equal(other.offsets - other.c0, sub.offsets)


def test_continue_fill_extends_the_alignments():
    seq1 = np.arange(1, 27, dtype=np.uint8)  # every letter once: a piece's place in Seq1 is its first letter
    case = slice_case((10, 2, 3, 4), seq1, [5] * 40, c0=7, seed=4)
    st = case.storage("continue")
    assert case.first_at >= 0 and np.array_equal(st[:7], seq1[(case.first_at - 7 + np.arange(7)) % 26])
    assert case.next_at >= 0 and np.array_equal(st[-TAIL:], seq1[(case.next_at + np.arange(TAIL)) % 26])
    # wherever a record is an exact piece of Seq1 and the letter behind it starts some piece (of either kind: 6
    # letters of Seq1 must follow it), the next record starts with that letter
    rows = as_triples(search_cpu(case.sub))
    exact = [i for i in range(39) if rows[i, 0] == 50 and rows[i, 2] == 0 and rows[i, 1] + 5 <= 20]
    assert len(exact) >= 5
    for i in exact:
        assert case.sub.codes[case.sub.offsets[i + 1]] == seq1[rows[i, 1] + 5]


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_base_off_by_one_changes_half_of_the_rows(name):
    case = family_case(name, 32 + 3)
    sub, total = case.sub, int(case.sub.offsets[-1])
    want = as_triples(search_cpu(sub))
    for fill in FILLS:
        st = case.storage(fill)
        for d in (1, -1):
            off = Problem(sub.weights, sub.seq1, st[case.c0 + d:case.c0 + d + total].copy(), sub.offsets)
            changed = (as_triples(search_cpu(off)) != want).any(axis=1)
            assert 2 * int(changed.sum()) >= sub.n, (name, fill, d, int(changed.sum()), sub.n)


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_one_neighbour_letter_too_many_changes_a_score(name):
    case = family_case(name, 32 + 3)
    sub = case.sub
    st = case.storage("continue")
    o = case.offsets
    recs = [st[o[i]:o[i + 1] + 1] for i in range(sub.n)]
    longer = Problem(sub.weights, sub.seq1, np.concatenate(recs),
                     np.concatenate([[0], np.cumsum([r.shape[0] for r in recs])]).astype(np.int64))
    got, want = as_triples(search_cpu(longer)), as_triples(search_cpu(sub))
    assert (got[:, 0] != want[:, 0]).any(), name
