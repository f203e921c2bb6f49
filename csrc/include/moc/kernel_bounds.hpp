// Exactness rules of the narrow-integer fast paths, in one place.
//
// The reference scores in plain int (cudaFunctions.cu:103,161). The gfx950 kernels run most batches in
// narrower arithmetic: packed int16 running sums, int8 difference profiles, int32 keys with k packed
// into the low bits. Each form is exact only while no intermediate can wrap. The host picks a form per
// batch with the functions below, and nothing else decides:
//   * the launchers (swipe_kernels.hip, short_kernels.hip, align_kernels.hip, build_profile16) call them;
//   * HipEngine records the form each solve ran (EngineStats::forms);
//   * moc_kernel_forms (capi.h) predicts the forms without a GPU;
//   * csrc/tests/test_core.cpp replays each form's arithmetic on the host, with the same wrap-around, at
//     the bound (exact) and one step past it (the replay wraps, and the rule refuses the form).
//
// Notation: W = max |T| over the pair-score table (max of |W1..W4|), L2 = the batch's longest record
// that is searched (records longer than Seq1 are never scored). Along a diagonal o the kernels sum
// Dt[c][j] = T[c][Seq1[j]] - T[c][Seq1[j+1]], so |Dt| <= 2W and |D_o(k)| <= 2 W L2 = dmax. The bound is
// reached: Seq1 = "AZAZ...", Seq2 = a piece of Seq1 at an even offset, W1 = W4 = W gives Dt = 2W at
// every step (tests/test_extremes.py builds exactly that input).
#pragma once

#include <algorithm>
#include <cstdint>

namespace moc {
namespace bounds {

// |D_o(k)| <= 2 W L2 for every diagonal and prefix length.
inline int64_t diff_bound(int32_t max_abs_weight, int64_t max_l2) {
  return 2 * static_cast<int64_t>(std::max(max_abs_weight, 1)) * std::max<int64_t>(max_l2, 1);
}

// ---- swipe kernel (swipe_impl.hpp): one lane per record, int16 running sums per offset pair.
// Record words per lane (4 letters each): 4 for records <= 16 letters, 8 for <= 32, 12 for <= 48, 16 for
// <= 64, 24 for <= 96, 32 for <= 128 (the longest records the kernel takes). The words size the LDS tables
// (and P33's decode slices), so input1's records of 32..41 letters take 12, not 16.
constexpr int64_t kSwipeMaxL2 = 128;
inline int swipe_record_words(int64_t max_l2) {
  return max_l2 <= 16 ? 4 : max_l2 <= 32 ? 8 : max_l2 <= 48 ? 12 : max_l2 <= 64 ? 16 : max_l2 <= 96 ? 24 : 32;
}
// Bits for k in the int16 keys: k <= 4 * l2w < 2^kb.
constexpr int swipe_kbits(int l2w) {
  int b = 1;
  while ((1 << b) <= 4 * l2w) ++b;
  return b;
}
enum class SwipeKeys { None, KBits, RK };
// Key form of the swipe kernel for a batch:
//   KBits: E = D * 2^kb + (2^kb - 1 - k) in int16. Its largest value is dmax * 2^kb + 2^kb - 2, so
//          dmax * 2^kb + 2^kb < 32767 keeps every key (and B2 = max E) exact.
//   RK:    E = D in int16 (|D| <= dmax < 32767); k is re-found on the winning diagonal afterwards.
//          Records of more than 32 letters (l2w >= 12) always take it: no room for 6 k bits.
//   None:  dmax >= 32767.
// The selection keys carry score + 2^15 in 16 bits: |score| <= W L2 = dmax / 2 < 2^14 under either form; the
// anchor diagonal is summed in int32 from an int32 table (swipe_build_tables), so W itself is not bounded.
inline SwipeKeys swipe_keys(int32_t max_abs_weight, int64_t max_l2) {
  const int64_t dmax = diff_bound(max_abs_weight, max_l2);
  if (dmax >= 32767) return SwipeKeys::None;
  const int l2w = swipe_record_words(max_l2);
  const int kb = swipe_kbits(l2w);
  return (l2w >= 12 || (dmax << kb) + (int64_t{1} << kb) >= 32767) ? SwipeKeys::RK : SwipeKeys::KBits;
}

// ---- short kernel (short_kernels.hip): one lane per offset.
// Pk form: the profile holds (Dt << 16 | S) and one packed int16 add advances D_o (high half, |D| <= dmax)
// and Tot_o (low half, |Tot| <= W L2 < dmax). Exact when dmax < 32767.
inline bool short_pk_exact(int32_t max_abs_weight, int64_t max_l2) {
  return diff_bound(max_abs_weight, max_l2) < 32767;
}

// ---- int32 hot keys of the short (non-Pk) and tile kernels: key = D << shift | (2^shift - 1 - k), with
// 2^shift > L2 >= k. Exact when dmax << shift < 2^31; 0 means 64-bit keys. `max_l2` is capped at L1 + 1 by
// the caller (longer records are not searched).
inline int32_t key_shift(int32_t max_abs_weight, int64_t max_l2) {
  int shift = 1;
  while ((int64_t{1} << shift) < max_l2 + 1) ++shift;  // mask = 2^shift - 1 >= every k used (<= L2)
  if (shift > 24 || (diff_bound(max_abs_weight, max_l2) << shift) >= (int64_t{1} << 31)) return 0;
  return shift;
}

// ---- tile16 / MFMA sweeps (tile16_kernels.hip, tile_mfma_kernels.hip): Dt as int8 bytes of a profile,
// summed in int16 halves for at most kProf16Fold steps before being folded into int32, so the int16
// partial sums stay within kProf16Fold * 128 = 8192. T itself is read as int8 (anchor diagonals).
constexpr int kProf16Fold = 64;
// dmin/dmax: the extreme Dt over letter pairs (including the zero pad past Seq1); tabs: max |T|.
inline bool profile16_exact(int32_t dmin, int32_t dmax, int32_t tabs) {
  return dmin >= -128 && dmax <= 127 && tabs <= 127;
}
static_assert(kProf16Fold * 128 < 32768, "tile16 int16 partial sums");
// The int16 profile (one Dt per entry, staged into widened images only): |Dt| <= 511 keeps a 64-step partial
// sum within int16 (64 * 511 = 32704); T is read from the int32 LUT.
inline bool profile16_i16_exact(int32_t dmin, int32_t dmax) { return dmin >= -511 && dmax <= 511; }
static_assert(kProf16Fold * 511 < 32768, "tile16 int16 partial sums, int16 profile");

// tile16's per-lane selection in 32-bit keys: ((score + 2^(31 - IB)) << IB) | (2^IB - 1 - idx), idx = 2o +
// mutated <= 2 L1 + 1 < 2^IB. Exact when every score fits the 32 - IB score bits: |score| <= max|T| * L2
// < 2^(31 - IB). Returns IB, or 0 when the 64-bit keys are needed.
inline int tile16_key32_bits(int64_t L1, int32_t max_abs_t, int64_t max_l2) {
  int ib = 1;
  while ((int64_t{1} << ib) <= 2 * L1 + 1) ++ib;
  if (ib > 24) return 0;
  return static_cast<int64_t>(max_abs_t) * max_l2 < (int64_t{1} << (31 - ib)) ? ib : 0;
}

// ---- alignment report (report_kernels.hip): rows of records up to kReportShortMaxL2 letters take one lane
// each, their four sign counters packed as the bytes of one register — exact while a count (<= L2) fits a
// byte; longer records take one wave per row with int32 counters (any length).
constexpr int64_t kReportShortMaxL2 = 64;
constexpr int64_t kReportPackedCountMax = 255;
static_assert(kReportShortMaxL2 <= kReportPackedCountMax, "report: packed byte counters of the lane-per-row regime");
inline bool report_short_row(int64_t L2) { return L2 <= kReportShortMaxL2; }

// ---- threshold hits (hits_kernels.hip): the prefix sum over a chunk's per-record hit counts is reduce-then-scan
// in separate launches: blocks of kHitsScanBlockRecords records are summed, ONE block scans those sums
// kHitsScanSumsPerPass at a time with a running carry, then every block rescans its records from its sum. A chunk
// of at most kHitsScanBlockRecords records is one rescan launch from the chunk's base. All of it in int64.
constexpr int32_t kHitsScanThreads = 256;
constexpr int32_t kHitsScanBlockRecords = 4 * kHitsScanThreads;  // four consecutive counts per thread
constexpr int32_t kHitsScanSumsPerPass = 2 * kHitsScanThreads;   // two consecutive sums per thread and pass

// ---- distinct placements (peaks_kernels.hip; definitions: moc/cpu_engine.hpp peaks_filter): the peak filter's
// radius R ranges over 0 .. kPeaksMaxRadius — at least the longest record of the assignment (2000 letters), so "one
// placement per record length" is expressible. Records of at most kPeaksWaveEntries profile entries take one wave
// each; longer ones a workgroup per tile of kPeaksTile entries, which holds the tile and an R-entry halo on each
// side in LDS as 8-byte keys: (kPeaksTile + 2 kPeaksMaxRadius) * 8 bytes = 48 KiB.
constexpr int32_t kPeaksMaxRadius = 2048;
constexpr int32_t kPeaksWaveEntries = 64;
constexpr int32_t kPeaksTile = 2048;
constexpr int32_t kPeaksThreads = 256;
constexpr int32_t kPeaksKeysPerThread = (kPeaksTile + 2 * kPeaksMaxRadius) / kPeaksThreads;  // 24
static_assert((kPeaksTile + 2 * kPeaksMaxRadius) % kPeaksThreads == 0, "peaks: whole keys per thread");
static_assert((kPeaksTile + 2 * kPeaksMaxRadius) * 8 <= 64 * 1024, "peaks: tile + halo within one workgroup's LDS");

// ---- profile summary (summary_kernels.hip; definitions: moc/cpu_engine.hpp summary_batch_cpu): one wave per record,
// kSummaryRecordsPerBlock waves (records) per workgroup; the optional histogram has 0 .. kSummaryMaxBins bins, one
// int32 LDS counter per bin and wave. sum and sumsq are exact int64: every |score| <= M = min(2^31, W * L2) (a score
// is an int32 sum of L2 table entries), so |sum| <= C * M and sumsq <= C * M^2 for a record of C entries.
// summary_max_count is the largest C for which C * M^2 <= 2^63 - 1 (M^2 <= 2^62, so it is at least 2); a call whose
// longest profile has more entries is refused on the host before anything is launched.
constexpr int32_t kSummaryThreads = 256;
constexpr int32_t kSummaryRecordsPerBlock = kSummaryThreads / 64;
constexpr int32_t kSummaryMaxBins = 256;
inline int64_t summary_max_count(int32_t max_abs_weight, int64_t max_l2) {
  const int64_t w = std::max(max_abs_weight, 1), l2 = std::max<int64_t>(max_l2, 1);
  const int64_t cap = int64_t{1} << 31;
  const int64_t m = l2 >= cap || w > cap / l2 ? cap : std::min(cap, w * l2);
  return INT64_MAX / (m * m);
}
inline bool summary_exact(int32_t max_abs_weight, int64_t max_l2, int64_t max_count) {
  return max_count <= summary_max_count(max_abs_weight, max_l2);
}

// ---- multi-target search (targets_kernels.hip; definitions: moc/cpu_engine.hpp targets_batch_cpu): a target set
// holds 1 .. kTargetsMax sequences. A group of G consecutive lanes (4, 16 or 64) owns one (record, target) pair;
// the host picks G per chunk from the chunk's longest slice (entries of a pair's slice of the catalog profile):
// up to kTargetsGroup4MaxSlice entries G = 4, up to kTargetsGroup16MaxSlice G = 16, else a wave. Tuning constants
// only, every G gives the same rows for any slice length. Measured on input6-shaped records (profiles/targets/
// README.md): at slices of up to 20 entries G = 4 takes 0.88 ms where G = 16 takes 1.39, at 46 they tie, from 98 on
// G = 16 is ahead; G = 16 still leads a wave at 410 (0.67 against 0.74 ms) and trails it at 826 (0.78 against 0.65).
constexpr int32_t kTargetsMax = 4096;
constexpr int32_t kTargetsThreads = 256;
constexpr int64_t kTargetsGroup4MaxSlice = 32;
constexpr int64_t kTargetsGroup16MaxSlice = 512;
inline int targets_group(int64_t max_slice) {
  return max_slice <= kTargetsGroup4MaxSlice ? 4 : max_slice <= kTargetsGroup16MaxSlice ? 16 : 64;
}

// ---- per-target profile summary (targets_summary_kernels.hip; definitions: moc/cpu_engine.hpp
// targets_summary_batch_cpu): the lane groups and cut-overs of the multi-target search (targets_group above), one
// summary row per (record, target) pair. The histogram kernel keeps one int32 LDS counter per bin and group; a
// workgroup's counters stay within kTargetsHistLdsBytes = 16 KiB, so that the eight 256-thread workgroups that fill a
// CU's 32 wave slots need 128 of its 160 KiB and LDS never limits occupancy. With G lanes per group a workgroup
// holds kTargetsThreads / G groups: 64 groups of 4 lanes fit up to kTargetsHistGroup4MaxBins = 64 bins each, 16
// groups of 16 lanes (and 4 waves) the full kSummaryMaxBins. targets_hist_group widens a 4-lane choice to 16 lanes
// past 64 bins and leaves every other choice alone; every group size gives the same rows.
constexpr int32_t kTargetsHistLdsBytes = 16 * 1024;
constexpr int32_t kTargetsHistGroup4MaxBins = kTargetsHistLdsBytes / 4 / (kTargetsThreads / 4);
static_assert(kTargetsHistGroup4MaxBins == 64, "targets summary: 64 four-lane groups of 64 bins fill 16 KiB");
static_assert((kTargetsThreads / 16) * kSummaryMaxBins * 4 <= kTargetsHistLdsBytes, "targets summary: 16-lane groups fit");
inline int targets_hist_group(int group, int32_t bins) {
  return group == 4 && bins > kTargetsHistGroup4MaxBins ? 16 : group;
}
// Entries of the target profile of a record of L2 letters against a target of `len` letters (0: it does not fit):
// the slice's len - L2 entries plus the boundary entry under the spec semantics or with len == L2.
inline int64_t targets_pair_count(int64_t len, int64_t L2, bool spec) {
  if (L2 < 1 || L2 > len) return 0;
  return len - L2 + (spec || len == L2 ? 1 : 0);
}

// ---- per-target top-K and threshold hits (targets_rows_kernels.hip; definitions: moc/cpu_engine.hpp
// targets_topk_batch_cpu / targets_hits_batch_cpu): the lane groups of the multi-target search. The count and
// compaction kernels take targets_group's choice (measured crossings: four lanes ahead at slices of 20 entries and
// behind at 46, sixteen level with a wave at 410 — 1.63 against 1.66 ms — and behind it at 826). The top-K kernel's 16-lane range ends
// earlier. Measured at K = 4 on input6-shaped records (profiles/targets_rows/README.md): sixteen lanes lead a wave at
// slices of 202 entries (1.67 against 1.82 ms) and trail it at 410 (2.08 against 1.48), so the crossing lies
// somewhere in 202 .. 410. kTargetsTopKGroup16MaxSlice = 256 was chosen inside that bracket because it is the number
// of slice keys a wave holds in registers (four per lane, 4 * 64; the rest is re-read once per round) — a structural
// reason to prefer that point of the bracket, not a measured crossing. Tuning constants only.
constexpr int64_t kTargetsTopKGroup16MaxSlice = 256;
inline int targets_topk_group(int64_t max_slice) {
  return max_slice <= kTargetsGroup4MaxSlice ? 4 : max_slice <= kTargetsTopKGroup16MaxSlice ? 16 : 64;
}

// ---- per-target distinct placements (targets_peaks_kernels.hip; definitions: moc/cpu_engine.hpp
// targets_topk_batch_cpu / targets_hits_batch_cpu with radius > 0): the peak filter over every (record, target)
// pair's own profile. A pair profile of 2 .. S entries takes a segment of S consecutive lanes of a wave (S = 4, 8, 16,
// 32 or 64, a lane per entry), a longer one a workgroup per tile of kPeaksTile entries with peaks_tile_kernel's LDS
// budget (kPeaksTile + 2 kPeaksMaxRadius keys); a profile of one entry is its own peak and has no mark. The host picks
// S per chunk from the chunk's longest pair profile: the smallest of the five widths that holds it, a wave from 33
// entries on — the narrowest segment that still gives every profile of at most kPeaksWaveEntries entries a lane per
// entry, so none of them goes to a workgroup. MOC_TARGETS_PEAKS_SEG=4|8|16|32|64 at engine start forces S; a profile
// longer than a forced S goes to the tile kernel, so every S gives the same marks. Tuning only. "The narrowest width
// that fits" is a rule, not a set of measured crossings: measured on input6-shaped records against 256 targets (pair
// profiles of 15 .. 20 entries; profiles/targets_peaks/README.md), 32 lanes — the rule's choice — are ahead of a wave,
// and 4, 8 and 16 lanes, which send those profiles to the tile kernel, far behind; no shape with profiles of at most
// 4, 8 or 16 entries was measured.
constexpr int32_t kTargetsPeaksMinSeg = 4;
inline bool targets_peaks_seg_valid(int s) { return s >= kTargetsPeaksMinSeg && s <= kPeaksWaveEntries && (s & (s - 1)) == 0; }
inline int targets_peaks_seg(int64_t max_count) {
  int s = kTargetsPeaksMinSeg;
  while (s < kPeaksWaveEntries && s < max_count) s <<= 1;
  return s;
}
static_assert(kPeaksWaveEntries == 64, "targets peaks: the widest segment is a wave");

// ---- target ranking (targets_rank_kernels.hip; definitions: moc/cpu_engine.hpp targets_rank_batch_cpu): each record's
// M best targets out of the chunk's pair rows, which the select kernel leaves in the profile scratch behind the
// chunk's entries — kTargetsRankRecordBytes = 12 bytes per (record, target) pair, the planner's record_bytes = 12 T.
// A group of G consecutive lanes (4, 16 or 64) owns one record and walks its T rows once per round, ceil(T / G) rows
// per lane; the host picks G from T alone (a record's rows are T whatever its length): up to kTargetsRankGroup4MaxT
// targets G = 4 (at most four rows per lane and round), up to kTargetsRankGroup16MaxT G = 16 (at most sixteen), else a
// wave. The two cut-overs are a rule — "no lane walks more than G rows per round until the group is a wave" — not
// measured crossings (profiles/targets_rank/README.md says what was measured). MOC_TARGETS_RANK_GROUP=4|16|64 at
// engine start forces G. Tuning constants only, every G gives the same rows for any T.
constexpr int64_t kTargetsRankRecordBytes = 12;
constexpr int64_t kTargetsRankGroup4MaxT = 16;
constexpr int64_t kTargetsRankGroup16MaxT = 256;
inline int targets_rank_group(int64_t T) {
  return T <= kTargetsRankGroup4MaxT ? 4 : T <= kTargetsRankGroup16MaxT ? 16 : 64;
}

// Form bits reported per solve (EngineStats::forms; Python: stats()["forms"]).
enum FormBits : int32_t {
  kFormSwipeKBits = 1,    // swipe, int16 keys with k bits
  kFormSwipeRK = 2,       // swipe, int16 sums, k re-walked
  kFormShortPk = 4,       // short, packed (D, Tot) int16 pairs
  kFormShortKey32 = 8,    // short, int32 keys
  kFormShortKey64 = 16,   // short, int64 keys
  kFormTile16 = 32,       // tile16, int8 profile + int16 partial sums
  kFormTilesKey32 = 64,   // LUT tile kernel, int32 keys
  kFormTilesKey64 = 128,  // LUT tile kernel, int64 keys
  kFormMfma = 256,        // matrix-core sweep over the tile16 profile
  kFormTile16Key32 = 512, // tile16's per-lane selection in 32-bit keys (tile16_key32_bits)
  kFormTile16I16 = 1024,  // tile16 over the int16 profile (profile16_i16_exact)
  kFormTile16Slide = 2048,  // tile16 in sliding widened windows (long records, widened image past the LDS)
};

}  // namespace bounds
}  // namespace moc
