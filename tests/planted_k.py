"""Case lists of the planted mutation points (utils/synthetic.make_planted_k / make_planted_k_ties), shared by
the GPU tier (tests/test_gpu_planted_k.py), which runs them through every kernel, and the CPU tier
(tests/test_planted_k.py), which proves every claim against the pure-Python prefix oracle and shows that these
very cases tell a wrong k rule from the right one (``pick_k``). Plain data and numpy: no engine, no GPU."""
import zlib

import numpy as np

from mpi_openmp_cuda_amd.models.scoring import score_table
from mpi_openmp_cuda_amd.utils.synthetic import make_planted_k, make_planted_k_ties, planted_k_expected

W = (10, 2, 3, 4)
W_I16 = (200, 10, 10, 10)  # |Dt| past the byte pairs: the int16 profile
W_DPP = (300, 300, 1, 1)   # |Dt| past the int16 profile: the LUT (DPP) tile kernel
W_K32 = (7, 2, 3, 4)           # records of 32 letters with k in the int16 key: (W1 + W4) * 32 < 2^9
W_RK4 = (1023, 0, 0, 1023)     # records of 16 letters with no room for k in the int16 key: RK
W_KEY64 = (22076, 0, 0, 22076)   # one past the short kernel's int32 keys
W_TILES64 = (5243, 0, 0, 5243)   # one past the LUT tile kernel's int32 keys

K_EDGES = (1, 63, 64, 65, 127, 128, 129)


def every_k(L2, ps):
    return [(p, L2, k) for p in ps for k in range(1, L2)]


def some_k(L2, ks, ps):
    ks = sorted({k for k in ks if 1 <= k <= L2 - 1})
    return [(p, L2, k) for p in ps for k in ks]


def edge_k(L2):
    return K_EDGES + (L2 - 2, L2 - 1)


def fill_to(cases, n):
    """``cases`` and then cases of it again, up to n records (the sliding windows take full groups of 16)."""
    cases = [tuple(int(v) for v in c) for c in cases]
    return cases + [cases[i % len(cases)] for i in range(n - len(cases))]


SLIDE_K = (1, 63, 64, 65, 127, 128, 129, 511, 512, 1023, 1024, 1098, 1099)


def _slide_cases():
    c = some_k(1100, SLIDE_K, (0, 128, 1298))
    return fill_to(c, 48)  # 39 cases and 9 of them again: three full groups of 16 records


def _mixed(L1, lengths, ps):
    # lengths interleaved record by record, so that one wave of the lane-per-offset kernel holds all of them
    per = [every_k(L2, [p for p in ps if p + L2 + 1 <= L1]) for L2 in lengths]
    out = []
    for i in range(max(len(c) for c in per)):
        out += [c[i] for c in per if i < len(c)]
    return out


# name, L1, weights, cases (p, L2, k), environment of a fresh engine, kernels, forms the run must / must not name
ROWS = [
    # swipe, k in the low bits of the int16 key: record words of 4 letters (kb = 5) ...
    ("swipe_kbits_8", 71, W, every_k(8, range(63)), {}, ["swipe"], ["swipe_kbits"], ["swipe_rk"]),
    ("swipe_kbits_16", 79, W, every_k(16, range(63)), {}, ["swipe"], ["swipe_kbits"], ["swipe_rk"]),
    # ... and of 8 (kb = 6)
    ("swipe_kbits_17", 80, W, every_k(17, (0, 1, 3, 4, 31, 62)), {}, ["swipe"], ["swipe_kbits"], ["swipe_rk"]),
    # (with 32 letters the k bits fit the key up to W1 + W4 = 15 only: W itself is the RK form there)
    ("swipe_kbits_32", 95, W_K32, every_k(32, (0, 1, 3, 4, 31, 62)), {}, ["swipe"], ["swipe_kbits"], ["swipe_rk"]),
    ("swipe_rk_32", 95, W, every_k(32, (0, 1, 3, 4, 31, 62)), {}, ["swipe"], ["swipe_rk"], ["swipe_kbits"]),
] + [
    # swipe RK: the winner's k from a second walk of its diagonal, on both sides of every record-word class
    (f"swipe_rk_{L2}", L2 + 63, W, every_k(L2, (0, 21, 42, 62)), {}, ["swipe"], ["swipe_rk"], ["swipe_kbits"])
    for L2 in (33, 48, 49, 64, 65, 96, 97, 128)
] + [
    ("swipe_rk_16_heavy", 79, W_RK4, every_k(16, (0, 21, 42, 62)), {}, ["swipe"], ["swipe_rk"], ["swipe_kbits"]),
    # the lane-per-offset kernel: k in the low bits of the key
    ("short_key32", 200, W, every_k(150, (0, 1, 31, 48)), {}, ["short"], ["short_key32"], ["short_pk", "short_key64"]),
    ("short_pk", 150, W, every_k(130, (0, 1, 9, 18)), {}, ["short"], ["short_pk"], ["short_key32", "short_key64"]),
    ("short_key32_mixed", 200, W, _mixed(200, (150, 170, 190), (0, 8, 28, 48)), {}, ["short"], ["short_key32"],
     ["short_pk", "short_key64"]),
    ("short_key64_mixed", 200, W_KEY64, _mixed(200, (150, 170, 190), (0, 8, 28, 48)), {}, ["short"], ["short_key64"],
     ["short_pk", "short_key32"]),
    # tile16: the sweep keeps a mutated bit, resolve_long_kernel finds k. 1359 / 1099: the last mutated offset
    ("tile16_l2_40_u8", 1400, W, every_k(40, (0, 127, 128, 640, 1000, 1359)), {}, ["tile16"], ["tile16"],
     ["tile16_slide", "tile16_i16"]),
    ("tile16_l2_300_u2", 1400, W, every_k(300, (0, 127, 128, 500, 900, 1099)), {}, ["tile16"], ["tile16"],
     ["tile16_slide", "tile16_i16"]),
    ("tile16_l2_40_u4", 1400, W, every_k(40, (0, 127, 128, 640, 1000, 1359)), {"MOC_TILE_U": "4"}, ["tile16"],
     ["tile16"], ["tile16_slide"]),
    ("tile16_l2_300_u4", 1400, W, every_k(300, (0, 127, 128, 500, 900, 1099)), {"MOC_TILE_U": "4"}, ["tile16"],
     ["tile16"], ["tile16_slide"]),
    # L1 past the widened image with the widened window switched off: the sliding windows take the records, and
    # with those off too the whole byte-pair image
    ("tile16_slide_winwide_off", 2001, W, every_k(40, (0, 127, 128, 1000, 1959, 1960)), {"MOC_TILE16_WINWIDE": "0"},
     ["tile16"], ["tile16", "tile16_slide"], []),
    ("tile16_byte_pair_image", 2001, W, every_k(40, (0, 127, 128, 1000, 1959, 1960)),
     {"MOC_TILE16_WINWIDE": "0", "MOC_TILE16_SLIDE": "0"}, ["tile16"], ["tile16"], ["tile16_slide"]),
    ("tile16_windowed", 6500, W,
     every_k(40, (0, 127, 128, 1023, 1024, 2047, 2048, 3071, 3072, 4095, 4096, 5119, 5120, 6143, 6144, 6459)), {},
     ["tile16"], ["tile16"], ["tile16_slide"]),
    ("tile16_i16", 1400, W_I16, some_k(300, edge_k(300), (0, 127, 128, 500, 900, 1099)), {}, ["tile16"],
     ["tile16", "tile16_i16"], ["tile16_slide"]),
    ("tile16_slide", 2400, W, _slide_cases(), {}, ["tile16"], ["tile16", "tile16_slide"], ["tile16_i16"]),
    ("tile16_slide_i16", 2400, W_I16, _slide_cases(), {}, ["tile16"], ["tile16_slide", "tile16_i16"], []),
    ("dpp_tiles_key32", 600, W_DPP, some_k(150, edge_k(150), (0, 127, 128, 449)), {}, ["tiles"], ["tiles_key32"],
     ["tile16", "tiles_key64"]),
    ("dpp_tiles_key64", 600, W_TILES64,
     some_k(150, edge_k(150), (0, 127, 128, 199)) + some_k(400, edge_k(400) + (255, 256, 257), (0, 127, 128, 199)), {},
     ["tiles"], ["tiles_key64"], ["tile16", "tiles_key32"]),
    ("mfma", 1400, W, some_k(300, edge_k(300), (0, 127, 128, 500, 900, 1099)), {"MOC_MFMA": "1"}, ["tile16"], ["mfma"],
     []),
]
ROW = {r[0]: r for r in ROWS}


def lengths_of(row):
    return sorted({c[1] for c in row[3]})


def inside_pairs(L2):
    """(j, k) of the tie inside an offset: spans that straddle a 4-letter record word, the 64th and the 128th step,
    and one that ends on the last k. (The span (1, L2 - 1) leaves two matching letters: chance beats its claim at
    another offset already with 8 letters, the oracle says, so the last span is three steps long.)"""
    pairs = [(1, 2), (3, 5), (60, 70), (63, 64), (64, 65), (120, 130), (126, 129), (L2 - 4, L2 - 1)]
    return sorted({(j, k) for j, k in pairs if 1 <= j < k <= L2 - 1})


def own_ks(L2):
    """k of the tie of a mutant with its own offset's un-mutated candidate: L2 / 2 and L2 - 1 (with 128 and 300
    letters a multiple of 64 is among them), from 5 letters up."""
    return sorted({k for k in (max(5, (L2 + 1) // 2), L2 - 1) if max(5, (L2 + 1) // 2) <= k <= L2 - 1})


def shadow_sets(ps):
    """Splits offsets into sets without two offsets closer than 3: each set shares one Seq1, and two shadow ties
    next to each other would put three equal letters in a row."""
    sets = []
    for p in ps:
        for s in sets:
            if all(abs(p - q) >= 3 for q in s):
                s.append(p)
                break
        else:
            sets.append([p])
    return sets


def tie_problems(row):
    """The tie problems of a table row, on the row's Seq1 length, weights and record lengths:
    [(family, tag, cases)], several per family where one Seq1 cannot hold all cases."""
    name, L1, w, cases = row[:4]
    out = []
    L2s = lengths_of(row)
    swipe = row[5] == ["swipe"]
    ps = sorted({c[0] for c in cases})
    ps = [ps[0], ps[len(ps) // 2], ps[-1]]
    inside = [(p, L2, j, k) for L2 in L2s for p in ps for j, k in inside_pairs(L2) if p + L2 + 1 <= L1]
    own = [(p, L2, k) for L2 in L2s for p in ps for k in own_ks(L2) if p + L2 + 1 <= L1]
    out.append(("inside", "all", inside))
    if own:
        out.append(("own", "all", own))
    L2 = L2s[-1]
    last = L1 - L2  # the final offset: under the reference semantics never tried, but its shadow is
    want = (1, 4, 5, 32, last) if swipe else (1, 64, 128, 129, 256, last - 1, last)
    for i, ps in enumerate(shadow_sets([p for p in want if 1 <= p <= last])):
        # the row's lengths in turn; the final offset belongs to the longest record
        out.append(("shadow", f"set{i}", [(p, L2 if p >= last - 1 else L2s[n % len(L2s)]) for n, p in enumerate(ps)]))
    return out


def first_accepted(L1, cases, weights, seed):
    """make_planted_k_ties' shadow problem under the first of the seeds seed, seed + 1000, ... whose Seq1 it accepts:
    a shadow tie is refused where the random Seq1 already has its letter on the other side."""
    for attempt in range(8):
        try:
            return make_planted_k_ties(L1, "shadow", cases, weights, seed=seed + 1000 * attempt)
        except ValueError:
            if attempt == 7:
                raise


_built = {}


def build(name, family="k", tag="all"):
    """(problem, cases, claimed rows) of a table row's planted-k problem or of one of its tie problems; built once,
    read-only."""
    key = (name, family, tag)
    if key not in _built:
        row = ROW[name]
        # the seed from the row's problem, not its name: rows that differ in the environment alone share problems
        seed = zlib.crc32(repr((_problem_key(row), family, tag)).encode()) % 100000
        if family == "k":
            prob, cases = make_planted_k(row[1], row[3], row[2], seed=seed)
        else:
            cases = next(c for f, t, c in tie_problems(row) if (f, t) == (family, tag))
            if "slide" in name:
                cases = fill_to(cases, 16 * ((len(cases) + 15) // 16))
            if family == "shadow":
                prob, cases = first_accepted(row[1], cases, row[2], seed)
            else:
                prob, cases = make_planted_k_ties(row[1], family, cases, row[2], seed=seed)
        want = planted_k_expected(prob, cases, family)
        for a in (prob.codes, prob.offsets, prob.seq1, want):
            a.setflags(write=False)
        _built[key] = (prob, cases, want)
    return _built[key]


def _problem_key(row):
    return (row[1], tuple(row[2]), tuple(tuple(c) for c in row[3]), "slide" in row[0])


def all_problems():
    """Every (name, family, tag) the GPU tier runs, each problem once: a row that differs from an earlier one in the
    environment alone (another plan of the same kernel) has that row's problems."""
    out, seen = [], set()
    for row in ROWS:
        if _problem_key(row) in seen:
            continue
        seen.add(_problem_key(row))
        out.append((row[0], "k", "all"))
        out += [(row[0], f, t) for f, t, _ in tie_problems(row)]
    return out


# the swipe rows "at the bound" of EXTREMES (tests/test_gpu.py): L1, shortest and longest record, weights. The GPU
# tier asserts that they are those rows; the CPU tier checks make_extreme_mutants against brute force on them
EXTREME_SWIPE_AT = [(40, 6, 16, (31, 0, 0, 31)), (60, 20, 32, (7, 0, 0, 7)), (70, 40, 64, (255, 0, 0, 255)),
                    (40, 6, 16, (1023, 0, 0, 1023)), (130, 67, 96, (170, 0, 0, 170)), (190, 127, 128, (127, 0, 0, 127))]
# every other shape of EXTREMES' "at" and "past" rows (the CPU engine decides there, checked against the claim)
EXTREME_OTHER = [(150, 130, 150, (109, 0, 0, 109)), (200, 150, 190, (22075, 0, 0, 22075)),
                 (200, 150, 190, (22076, 0, 0, 22076)), (600, 150, 400, (63, 0, 0, 64)), (600, 150, 400, (64, 0, 0, 64)),
                 (600, 150, 400, (255, 0, 0, 256)), (600, 150, 400, (256, 0, 0, 256)), (600, 150, 400, (5242, 0, 0, 5242)),
                 (600, 150, 400, (5243, 0, 0, 5243)), (2400, 900, 1400, (63, 0, 0, 64)), (2600, 2000, 2064, (127, 0, 0, 0)),
                 (2600, 2000, 2065, (127, 0, 0, 0))]


# ---- a numpy model of how k is picked on the winning diagonal, under a named rule -----------------------
RULES = ("first", "last", "ge", "carry_dropped", "one_short", "narrow_field")


def pick_k(prob, i, o, rule="first", table=None):
    """The k of record i's best candidate at offset o (o + L2 + 1 <= L1). d[s] is the gain of letter s on diagonal
    o over diagonal o + 1, D(k) the sum of d[0 .. k - 1]: the mutant k scores tot(o + 1) + D(k), the un-mutated
    candidate tot(o + 1) + D(L2). ``first`` is the product's rule: the first k in 1 .. L2 - 1 with the largest D,
    and k = 0 when D(L2) is at least that. The others are slips a kernel could make:
    ``last`` the last such k; ``ge`` the mutant wins a tie with D(L2); ``carry_dropped`` D starts again from 0 in
    every 64-step pass; ``one_short`` the walk stops before k = L2 - 1; ``narrow_field`` k is kept in one bit less
    than L2 - 1 needs."""
    t = (score_table(prob.weights) if table is None else table).astype(np.int64)
    r = prob.codes[prob.offsets[i]:prob.offsets[i + 1]].astype(np.int64)
    L2 = r.shape[0]
    s1 = prob.seq1.astype(np.int64)
    d = t[r, s1[o:o + L2]] - t[r, s1[o + 1:o + L2 + 1]]
    D = np.cumsum(d)  # D[k - 1] = D(k)
    full = int(D[L2 - 1])
    if rule == "carry_dropped":
        D = np.concatenate([np.cumsum(d[b:b + 64]) for b in range(0, L2, 64)])
    cand = D[:L2 - 2] if rule == "one_short" else D[:L2 - 1]  # k = 1 .. L2 - 1 (or L2 - 2)
    if cand.shape[0] == 0:
        return 0
    top = int(cand.max())
    if top < full or (top == full and rule != "ge"):
        return 0
    hits = np.nonzero(cand == top)[0]
    k = int(hits[-1] if rule == "last" else hits[0]) + 1
    if rule == "narrow_field":
        k &= (1 << (max(int(L2 - 1).bit_length(), 1) - 1)) - 1
    return k
