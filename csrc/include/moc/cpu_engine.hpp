// CPU (OpenMP) search engine — the "GPU kernel stubbed" backend of BASELINE.json config 1, and the
// C++ test oracle for the HIP kernels.
//
// Reference semantics (cudaFunctions.cu:63-176, race-free reading):
//   score(o, 0)  = sum_i T[s2_i][s1_{i+o}]                                  (no hyphen)
//   score(o, k)  = sum_{i<k} T[s2_i][s1_{i+o}] + sum_{i>=k} T[s2_i][s1_{i+o+1}],  k = 1..L2-1
//   offsets o in [0, L1-L2) (exclusive, :116), ties -> first in offset-major / mutant-minor order
//   (strict `max <` at :161); L2 == L1 -> (0,0) only (:74-106); L2 > L1 -> (INT_MIN, 0, 0).
// Closed form used here: with P_d(k) = sum_{i<k} T[s2_i][s1_{i+d}] and Tot_d = P_d(L2),
//   score(o, k>=1) = P_o(k) - P_{o+1}(k) + Tot_{o+1}  -> O(L1*L2) instead of O(L1*L2^2).
#pragma once

#include <cstdint>

#include "moc/common.hpp"
#include "moc/kernel_bounds.hpp"
#include "moc/problem.hpp"
#include "moc/score_table.hpp"

namespace moc {

// Lexicographic "better than" for candidates: higher score, then smaller offset, then smaller k
// (k == 0 is the un-mutated sequence and comes first inside an offset, as in the reference loop).
inline bool better(const Result& a, const Result& b) {
  if (a.score != b.score) return a.score > b.score;
  if (a.n != b.n) return a.n < b.n;
  return a.k < b.k;
}

// Best candidate for one record restricted to offsets [o_begin, o_end) of the full candidate set.
// Returns {kNoCandidateScore, -1, -1} when the range holds no candidate.
Result solve_offsets(const ScoreTable& t, const uint8_t* s1, int64_t L1, const uint8_t* s2, int64_t L2,
                     int64_t o_begin, int64_t o_end, Semantics sem);

// Number of offsets in the candidate set of a record (reference: L1-L2, spec: L1-L2+1; 1 if equal).
int64_t candidate_offsets(int64_t L1, int64_t L2, Semantics sem);

// Full search for one record.
Result solve_record(const ScoreTable& t, const uint8_t* s1, int64_t L1, const uint8_t* s2, int64_t L2,
                    Semantics sem);

// Batch search (OpenMP). Records [0, batch.size()) -> out[0..N). Parallel over records when there are
// many, over offset ranges of each record when there are few (the "context-parallel" split, §5.7).
void solve_batch_cpu(const ScoreTable& t, const uint8_t* s1, int64_t L1, const RecordBatch& batch, Result* out,
                     Semantics sem, int num_threads = 0);

// ---- packed candidate keys: the context-parallel combine
// PASS-1 key = (score ^ 2^31) << 32 | (2^32 - 1 - (2n + mutated)); 0 = "no candidate". The unsigned max
// over keys is the reference's winner up to its k (higher score, then smaller offset, then the un-mutated
// candidate first), so partial searches over disjoint offset ranges combine with one MAX reduction
// (MPI_Allreduce / ncclAllReduce, UINT64); resolve_key then finds k on the winning diagonal (the smallest k
// with that score — the reference's order inside an offset). No o*L2 + k index: L1 * L2 may exceed 2^32.
// Identical to the device encoding (csrc/src/hip/kernel_common.hpp lane_pass1_candidate, resolve_long_kernel).
inline uint64_t encode_key(const Result& r) {
  if (r.n < 0 || r.score == kNoCandidateScore) return 0;
  const uint32_t idx = 2u * static_cast<uint32_t>(r.n) + (r.k > 0 ? 1u : 0u);
  return (static_cast<uint64_t>(static_cast<uint32_t>(r.score) ^ 0x80000000u) << 32) | (0xffffffffu - idx);
}
// The result a MAX-combined key stands for (record s2 of length L2 against Seq1 s1): O(L2).
Result resolve_key(const ScoreTable& t, const uint8_t* s1, int64_t L1, const uint8_t* s2, int64_t L2, uint64_t key);

// Part `part` of `parts` of every record's candidate set (offsets [C*part/parts, C*(part+1)/parts) of
// its C candidate offsets) -> keys[i] (0 where the part holds no candidate). max over all parts of
// keys[i] == encode_key(solve_record(i)).
void solve_keys_cpu(const ScoreTable& t, const uint8_t* s1, int64_t L1, const RecordBatch& batch, int part,
                    int parts, uint64_t* keys, Semantics sem, int num_threads = 0);

// ---- per-offset score profile and top-K alignments
// Profile of a record with C = candidate_offsets(L1, L2, sem) offsets: C entries, entry o = the best candidate
// AT offset o — the maximum of score(o, 0) and, where mutated candidates exist (o < L1 - L2, k = 1..L2-1), of
// score(o, k); ties go to the smallest k, k = 0 first. A batch's profile is one flat array indexed through
// poffsets (int64[n+1], poffsets[i+1] - poffsets[i] = C_i). The better()-maximum over a record's profile is
// solve_record's result. Built on the same one-pass-per-offset recurrence as solve_offsets.
void profile_offsets(int64_t L1, const RecordBatch& batch, Semantics sem, int64_t* poffsets /* n + 1 */);
void profile_batch_cpu(const ScoreTable& t, const uint8_t* s1, int64_t L1, const RecordBatch& batch,
                       const int64_t* poffsets, ProfileEntry* prof, Semantics sem, int num_threads = 0);
// Top-K, 1 <= K <= kMaxTopK: out[i*K .. i*K+K) = record i's min(K, C_i) best offsets in better() order (higher
// score, then smaller n), each as (score, n, that offset's profile k), then no_candidate() rows. Row 0 is
// solve_record's result. One record's profile exists at a time per thread, never the batch's.
// radius > 0: the distinct form — only the record's peaks of that radius (peaks_filter below) are ranked:
// min(K, #peaks) rows, then no_candidate() rows; row 0 is still solve_record's result.
void topk_batch_cpu(const ScoreTable& t, const uint8_t* s1, int64_t L1, const RecordBatch& batch, int K, Result* out,
                    Semantics sem, int num_threads = 0, int64_t radius = 0);

// ---- threshold hits: every offset that scores at least a threshold
// Hits of record i under threshold t_i (thresholds[i], or min_score for every record when thresholds is null): the
// offsets o of its profile with profile[o].score >= t_i, in ascending o, each as a row (score, n = o, k =
// profile[o].k). INT32_MIN selects the whole profile; a record without candidate offsets has no hits.
// hoffsets (int64 [n + 1], always complete and exact): hoffsets[0] = 0, hoffsets[i + 1] - hoffsets[i] = record i's
// hit count; record i's rows are rows[hoffsets[i] .. hoffsets[i + 1]). Capacity contract: a row is written iff its
// flat index is < cap and nothing at or past rows + cap is touched; cap == 0 (rows may be null) counts only.
// Two phases, counts then fill; one record's profile exists at a time per thread, never the batch's.
void hits_batch_cpu(const ScoreTable& t, const uint8_t* s1, int64_t L1, const RecordBatch& batch, int32_t min_score,
                    const int32_t* thresholds, int64_t* hoffsets, Result* rows, int64_t cap, Semantics sem,
                    int num_threads = 0, int64_t radius = 0);

// ---- distinct placements: the peak filter of top-K and hits
// A mutated candidate (o, k) aligns letters < k on diagonal o and letters >= k on diagonal o + 1, so a placement
// at offset n has a shadow at n - 1 with k = 1 that scores within one letter pair of it. Entry o of a C-entry
// profile is a PEAK OF RADIUS R (0 <= R <= bounds::kPeaksMaxRadius) iff no entry o' with 0 < |o - o'| <= R and
// 0 <= o' < C is better() than it: a higher score, or an equal score and a smaller offset. Equivalently the
// order-free key (score ^ 2^31) << 32 | (2^32 - 1 - o) of entry o is the maximum over its window clipped to [0, C).
//   R = 0: every entry is a peak (the plain results). R >= C - 1: exactly one, solve_record's result.
//   A run of equal scores keeps only its first entry: an entry is suppressed by an equal entry to its left within
//   R even when that entry is suppressed itself. Local-maximum suppression, not greedy: scores 10, 9, 8 at R = 1
//   have one peak, the 10 (the 8 is suppressed by the 9, which the 10 suppresses). Every entry depends on its
//   window only.
//   Whatever suppresses an entry scores at least as much, so a threshold does not interact: distinct hits are the
//   peaks with score >= t_i; distinct top-K ranks the peaks.
// peak[o] = 1 or 0 for o in [0, C); O(C) for any R (a monotonic deque). Throws Error for R out of range.
void peaks_filter(const ProfileEntry* prof, int64_t C, int64_t radius, uint8_t* peak);
void check_peaks_radius(int64_t radius);  // throws Error unless 0 <= radius <= bounds::kPeaksMaxRadius

// ---- profile summary: the moments, extremes and a fixed-bin histogram of every record's profile
// Record i with the C_i profile entries {score, k} gives the row summary[i*7 .. i*7+7) =
// (count, sum, sumsq, min, max, n, k), kSummaryCols int64 values: count = C_i; sum and sumsq of the scores, exact;
// min and max over the scores; (max, n, k) the better()-maximum of the profile (highest score, then smallest offset,
// with that entry's k) — solve_record's result and row 0 of top-K. C_i = 0: (0, 0, 0, INT32_MAX, INT32_MIN, 0, 0).
// Histogram (bins = B in 0 .. bounds::kSummaryMaxBins; 0: none, hist may be null): entry o counts in bin
// summary_bin(score, lo, width, B) = clamp(floor((score - lo) / width), 0, B - 1), the subtraction and the floor
// division in int64 (lo = INT32_MIN with a positive score does not wrap; a negative numerator rounds down). Scores
// below lo land in bin 0, scores at or past lo + B * width in bin B - 1. hist: int32 [n * B]; every row sums to
// C_i. width >= 1. No radius and no threshold: the summary is of the whole profile.
// Exactness: check_summary_args throws Error ("summary: ...") unless 0 <= bins <= kSummaryMaxBins, width >= 1 and
// bounds::summary_exact(max |W|, the call's longest record, its longest profile) — then sumsq fits int64.
constexpr int kSummaryCols = 7;
inline int64_t summary_bin(int32_t score, int32_t lo, int32_t width, int32_t bins) {
  const int64_t d = static_cast<int64_t>(score) - lo;
  const int64_t q = d >= 0 ? d / width : -((-d + width - 1) / width);
  return std::min<int64_t>(std::max<int64_t>(q, 0), bins - 1);
}
void check_summary_args(int32_t max_abs_weight, int64_t max_l2, int64_t max_count, int32_t bins, int32_t width);
void summary_batch_cpu(const ScoreTable& t, const uint8_t* s1, int64_t L1, const RecordBatch& batch, int64_t* summary,
                       int32_t* hist, int32_t bins, int32_t lo, int32_t width, Semantics sem, int num_threads = 0);

// ---- multi-target search: every record's best alignment against each of T target sequences
// A target set is T sequences of lengths len_t >= 1, 1 <= T <= bounds::kTargetsMax, stored as their plain
// concatenation (the catalog, no separator letters) with starts (int64 [T + 1]): starts[0] = 0, starts[t + 1] =
// starts[t] + len_t, starts[T] = L1. The catalog IS Seq1 (s1, L1). check_targets throws Error ("targets: ...")
// unless T is in range and starts rises strictly from 0 to L1.
// out[i * T + t] = exactly solve_record(record i against target t alone), n relative to the target's start. With
// P the catalog's profile of record i (L2 letters), b = starts[t] and len = len_t:
//   L2 > len (or L2 > L1, or L2 < 1): no_candidate().
//   slice: the entries P[b + o], o in [0, len - L2). Every read of such an entry stays inside the target
//     (b + o + L2 <= b + len - 1) and b + o < L1 - L2, so its mutated candidates exist under either semantics:
//     they are the target's own profile entries.
//   boundary diagonal: the un-mutated score(b + len - L2, 0) as the entry (score, k = 0) at local offset len - L2,
//     taking part iff sem == Spec (the target's final, k = 0-only offset) or len == L2 (equal lengths: (0, 0)
//     only, under both semantics). Summed from the letters and the table, never read from P: the catalog's entry
//     there also holds mutated candidates that read the next target's first letter.
//   row: the better()-maximum over slice and boundary entry — highest score, then smallest local offset, with that
//     entry's k. The boundary entry has the largest offset, so it wins only with a strictly higher score.
// T = 1: out equals solve_batch_cpu row for row. One record's catalog profile exists at a time per thread.
void check_targets(const int64_t* starts, int64_t T, int64_t L1);
void targets_batch_cpu(const ScoreTable& t, const uint8_t* s1, int64_t L1, const RecordBatch& batch,
                       const int64_t* starts, int64_t T, Result* out, Semantics sem, int num_threads = 0);

// ---- target ranking: each record's M best targets, without the n * T pair rows
// Terms as above. F_i counts the targets that fit record i (1 <= L2 <= len_t). out[i * M + j], j < min(M, F_i), are
// record i's best fitting targets in the order higher score, then smaller target index, as (t, score, n, k) with
// (score, n, k) exactly targets_batch_cpu's row [i, t] (n local to the target); the rows past F_i are no_rank() =
// (-1, INT32_MIN, 0, 0). 1 <= M <= kMaxTopK. So row 0 is the best target; the whole result is targets_batch_cpu's
// rows of the record stably sorted by (-score, t) with the pairs that do not fit dropped (M >= T lists every fitting
// target); T = 1 is solve_batch_cpu with a leading 0. One record's T pair rows exist at a time per thread.
// Errors before any work: check_targets' ("targets: ..."), then check_targets_rank's ("rank: ...").
void check_targets_rank(int64_t M);
void targets_rank_batch_cpu(const ScoreTable& t, const uint8_t* s1, int64_t L1, const RecordBatch& batch,
                            const int64_t* starts, int64_t T, int M, RankRow* out, Semantics sem, int num_threads = 0);

// ---- per-target profile summary: the summary row and histogram of every (record, target) pair's target profile
// Terms as above (catalog, starts, b = starts[t], len = len_t, P the catalog's profile of record i, L2 letters).
// The pair (i, t) fits iff 1 <= L2 <= len. Its target profile holds the slice entries P[b + o], o in [0, len - L2),
// and the boundary entry (sum_l LUT[s2[l]][s1[b + len - L2 + l]], k = 0) at local offset len - L2 iff sem == Spec
// or len == L2 — exactly when it takes part in targets_batch_cpu, summed from the letters and never read from P. By
// the slice identity this is profile_record's profile of the record against target t alone.
// summary[(i * T + t) * 7 ..): (count, sum, sumsq, min, max, n, k) over those entries as summary_batch_cpu defines
// them, n local to the target: (max, n, k) is targets_batch_cpu's row [i, t]. A pair that does not fit gives
// (0, 0, 0, INT32_MAX, INT32_MIN, 0, 0). hist[(i * T + t) * bins ..) (bins > 0): summary_bin of every entry; the row
// sums to count; zeros where the pair does not fit. bins == 0: hist may be null and is not touched.
// Errors before any work: check_targets' ("targets: ..."), then check_summary_args' ("summary: ...") with M from the
// call's longest record and the largest count of any pair, targets_max_count — reached at the longest target with
// the shortest record that fits it. A catalog whose own profile summary_batch_cpu would refuse is accepted as long
// as every target's profile is within the bound.
int64_t targets_max_count(const int64_t* starts, int64_t T, const int64_t* offsets, int64_t n, Semantics sem);
void targets_summary_batch_cpu(const ScoreTable& t, const uint8_t* s1, int64_t L1, const RecordBatch& batch,
                               const int64_t* starts, int64_t T, int64_t* summary, int32_t* hist, int32_t bins,
                               int32_t lo, int32_t width, Semantics sem, int num_threads = 0);

// ---- per-target top-K and threshold hits: the rows of every (record, target) pair's target profile
// Terms and the target profile as above; pair (i, t) has C_{i,t} = bounds::targets_pair_count(len, L2, spec)
// entries, the boundary entry (k = 0, local offset len - L2, summed from the letters) the last of them.
// Top-K, 1 <= K <= kMaxTopK: out[((i * T + t) * K) ..) = the pair's min(K, C_{i,t}) best entries in better() order
// (higher score, then smaller local offset) as (score, n local to the target, that entry's k), then no_candidate()
// rows. It is topk_batch_cpu run on target t alone, row for row; K = 1 is targets_batch_cpu.
// Hits: pair p = i * T + t has the threshold thresholds[p] (int32 [n * T], pair-major), or min_score for every pair
// when thresholds is null; its hits are the entries of its target profile with score >= threshold in ascending local
// offset — hits_batch_cpu run on target t alone. toffsets (int64 [n * T + 1]) is hits_batch_cpu's index over pairs
// and the capacity contract is its own: the index always complete and exact, a row written iff its flat index is
// < cap, nothing at or past rows + cap touched, cap == 0 (rows may be null) counts only. A pair that does not fit
// has no hits. Errors before any work: check_targets' ("targets: ..."), then the top-K / hits messages, then
// check_peaks_radius' ("distinct: ...").
// radius > 0, the distinct forms: local entry o of pair (i, t) is a peak iff its key is the maximum of the keys at
// local offsets [o - radius, o + radius] clipped to the pair's own [0, C_{i,t}) — peaks_filter on the pair's target
// profile, the boundary entry an ordinary entry of it. Nothing outside the pair's profile is ever in a window: not
// the catalog's straddling entries, not the catalog's own value at the boundary offset, not a neighbouring target.
// Top-K then ranks the peaks (min(K, #peaks) rows, then no_candidate()), hits are the peaks at or above the pair's
// threshold in ascending local offset; index and capacity contract unchanged. Pair (i, t)'s rows are those of
// topk_batch_cpu / hits_batch_cpu with the same radius on target t alone; row 0 is targets_batch_cpu's at every
// radius; radius >= C_{i,t} - 1 leaves one peak per fitting pair; radius = 0 is the call without it.
void targets_topk_batch_cpu(const ScoreTable& t, const uint8_t* s1, int64_t L1, const RecordBatch& batch,
                            const int64_t* starts, int64_t T, int K, Result* out, Semantics sem, int num_threads = 0,
                            int64_t radius = 0);
void targets_hits_batch_cpu(const ScoreTable& t, const uint8_t* s1, int64_t L1, const RecordBatch& batch,
                            const int64_t* starts, int64_t T, int32_t min_score, const int32_t* thresholds,
                            int64_t* toffsets, Result* rows, int64_t cap, Semantics sem, int num_threads = 0,
                            int64_t radius = 0);

// ---- alignment report: the signs under a result row's letter pairs
// A row is a Result {score, n, k} of record i (L2 letters) against Seq1; rows[i*K .. i*K+K) belong to record i.
//   empty row   (score == kNoCandidateScore, e.g. top-K padding): counts {0,0,0,0}, marker bytes 0, nothing read
//   valid row   (report_row_valid): letter i faces Seq1[n + i] when k == 0 or i < k, else Seq1[n + i + 1] (the
//               hyphen faces Seq1[n + k] and is not counted); counts[PairClass] of those pairs, summing to L2;
//               marker byte i = ScoreTable::class_char of pair i
//   invalid row (anything else): counts {-1,-1,-1,-1}, marker bytes 0; n and k never form an address
// W1*c[0] - W2*c[1] - W3*c[2] - W4*c[3] is a valid row's true score; it is NOT compared with row.score here.
// Validity does not depend on the semantics: the spec-only final offset (L1 - L2, 0) is valid.
inline bool report_row_valid(int64_t L1, int64_t L2, const Result& r) {
  return L2 >= 1 && L2 <= L1 && r.k >= 0 && static_cast<int64_t>(r.k) <= L2 - 1 && r.n >= 0 &&
         static_cast<int64_t>(r.n) + L2 + (r.k > 0 ? 1 : 0) <= L1;
}
// counts: int32 [n*K*4]. marks (nullable): K * (total letters) bytes; row j of record i is the L2_i bytes at
// K * (offset of record i in the batch) + j * L2_i (64-bit indices). OpenMP over rows.
void report_batch_cpu(const ScoreTable& t, const uint8_t* s1, int64_t L1, const RecordBatch& batch, const Result* rows,
                      int K, int32_t* counts, uint8_t* marks, int num_threads = 0);

// Literal O(L1*L2^2) emulation of calc_result's loops (cudaFunctions.cu:74-172), race-free.
// Test oracle only.
Result brute_force_record(const ScoreTable& t, const uint8_t* s1, int64_t L1, const uint8_t* s2, int64_t L2,
                          Semantics sem);

}  // namespace moc
