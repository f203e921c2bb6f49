// Per-rank GPU engine: problem upload, launches, and host<->device data movement. The tile kernels' work is
// planned on the host by moc/tile_plan.hpp (no HIP call there: plans are checked without a device).
//
// Reference: send_divided_Seq2_To_Cuda (cudaFunctions.cu:178-242) — cudaMalloc per call and per
// record (leaking all but the last dev_count_signs), a blocking H2D of the whole fixed-stride chunk,
// one launch + cudaDeviceSynchronize per record, three blocking D2H copies, and the problem state in
// __constant__ symbols uploaded by four separate calls (cudaFunctions.cu:35-61).
//
// Here two data paths, chosen per call:
//   * direct (zero-copy streaming): when the batch lives in pinned host memory (hipHostMalloc /
//     hipHostRegister — e.g. the node-shared input window) and every record fits the short kernel, ONE
//     persistent kernel reads the letters straight over PCIe into LDS and writes packed results straight
//     back. Measured on MI355X: kernel reads of pinned host memory run at the hipMemcpy rate
//     (~56-57 GB/s, tools/probe_transfers.py), so staging copies would only add a second pass.
//   * staged pipeline: pooled device buffers (grown, never freed per call) and a double-buffered
//     3-stream chunk pipeline — copy stream H2D chunk c+1 | compute stream kernels of chunk c | return
//     stream D2H of chunk c-1 — ordered by events only. Used for pageable memory and for batches with
//     long records (tile kernel + host-planned tile lists).
// Results are written in the smallest wire format that fits the problem (R4/R8/R12, moc/device.hpp).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <initializer_list>
#include <memory>
#include <utility>
#include <vector>

#include "moc/common.hpp"
#include "moc/device.hpp"
#include "moc/runtime/timer.hpp"
#include "moc/score_table.hpp"
#include "moc/tile_plan.hpp"

namespace moc {

struct EngineOptions {
  int device = -1;                   // -1: keep the current device
  int64_t chunk_records = 1 << 21;   // staged pipeline: max records per chunk
  int64_t chunk_bytes = 64ll << 20;  // staged pipeline: max letter bytes per chunk
  bool allow_direct = true;          // use zero-copy streaming when the host buffers are pinned
  bool use_graphs = true;            // replay the direct path's launches as a captured hipGraph
  // kernel files (dev::PreloadSet) whose code objects load when the engine starts, on a helper thread beside
  // the stream set-up, not inside the first timed launch; the rest load at their first launch. MOC_PRELOAD
  // (dev::parse_preload_set) overrides.
  unsigned preload = dev::kPreloadAll;
  // Pinned host batches stream zero-copy: the kernel reads / writes host memory itself. A chunked SDMA
  // pipeline around the HBM-resident kernel was measured slower on the registered node-shared arrays the
  // headline streams from (4.4 vs 4.0 ms/step, profiles/host_stream_ab.log) and was retired in round 4.
  // Top-K: bound of the per-offset profile scratch (8 bytes per candidate offset). A batch runs in chunks of
  // consecutive records whose profiles fit it; a record larger than the bound runs alone in its chunk.
  // HipEngine::set_profile_scratch changes it at run time.
  int64_t profile_scratch_bytes = 256ll << 20;
};

struct EngineStats {
  double kernel_ms = 0;  // device time of the search kernels (events), last solve
  double total_ms = 0;   // wall time of the last solve call
  int64_t h2d_bytes = 0, d2h_bytes = 0, chunks = 0, cells = 0, records = 0;
  int32_t direct = 0;    // 1 if the last solve streamed from pinned host memory (zero-copy)
  int32_t format = 0;    // ResultFormat of the last solve
  int32_t kernels = 0;   // bitmask of kernels used: 1 swipe (lane/record), 2 short (lane/offset), 4 tiles
                         // (LUT tile kernel), 8 tile16, 16 profile (per-offset profile / top-K), 32 report,
                         // 64 hits (count / scan / compact, next to 16), 128 wire (decode kernels of a *_wire call),
                         // 256 peaks (the peak filter and masked select / hits kernels of a distinct call),
                         // 512 summary (the summary / histogram kernels, next to 16),
                         // 1024 targets (the multi-target select kernel, next to 16),
                         // 2048 targets_summary (the per-target summary / histogram kernels, next to 16),
                         // 4096 targets_topk (the per-target top-K kernel, next to 16),
                         // 8192 targets_hits (the per-target count / scan / compact kernels, next to 16),
                         // 16384 targets_peaks (the per-target peak pass and masked per-target kernels of a distinct
                         // per-target call, next to 256 and 4096 or 8192),
                         // 32768 targets_rank (the rank kernel of a target ranking, next to 16 and 1024)
  int32_t forms = 0;     // bitmask of the arithmetic forms they ran (moc::bounds::FormBits)
  R2Params r2;           // parameters of the R2 results of the last solve (when fmt == R2)
};

// Optional metadata about a batch (e.g. known from parsing / generation) that lets the engine skip its
// own scan over the lengths.
struct BatchHints {
  int64_t min_l2 = -1;
  int64_t max_l2 = -1;
};

// One engine per (rank, device). Not thread-safe: calls on one engine must not overlap (the streams,
// pooled buffers, work counter and cached graph are per engine); use one engine per thread instead.
class HipEngine {
 public:
  explicit HipEngine(const EngineOptions& opt = {});
  ~HipEngine();
  HipEngine(const HipEngine&) = delete;
  HipEngine& operator=(const HipEngine&) = delete;

  void set_problem(const Weights& w, const uint8_t* seq1, int64_t L1, Semantics sem);
  // Same, with Seq1 already on this device (e.g. delivered by an RCCL broadcast).
  void set_problem_device(const Weights& w, const uint8_t* d_seq1, int64_t L1, Semantics sem);

  // Host batch in -> host results out as moc::Result. `codes` is the base pointer (record i starts at
  // codes + offsets[i]); `offsets` has n+1 absolute entries.
  void solve(const uint8_t* codes, const int64_t* offsets, int64_t n, Result* out);
  // General form: optional narrow lengths — len_bits 8 (uint8, max L2 <= 255) or 4 (two per byte, low
  // nibble first, record i = len_base + nibble) — results in `fmt`. `packed`: 1 = `codes` is a 5-bit
  // packed stream (moc::pack5; char j at bit 5j), 3 = P33 fields (moc::pack33; 2 was the retired P24 code)
  // 0 = one byte per letter.
  // R2 results are encoded for the hints' [min_l2, max_l2] (or the batch's own range): stats().r2 holds
  // the parameters.
  void solve_ex(const uint8_t* codes, const int64_t* offsets, const uint8_t* lengths, int64_t n, void* out,
                ResultFormat fmt, const BatchHints& hints = {}, int packed = 0, int len_bits = 8,
                int len_base = 0);
  // Any wire-format batch (moc/wire.hpp): packed or byte letters, dense or sparse offsets, narrow lengths.
  // Sparse offsets stream zero-copy when the buffers are pinned and the swipe kernel takes the batch;
  // otherwise dense offsets are rebuilt from the lengths for the staged pipeline.
  void solve_wire(const WireBatch& b, void* out, ResultFormat fmt);
  // The same in two halves: begin_wire queues the zero-copy streaming kernel and returns (any other path
  // completes inside it); finish_wire waits for it and completes stats(). Every other call on the engine
  // finishes an open solve first. A streaming job encodes batch b+1 on the host while batch b streams.
  void begin_wire(const WireBatch& b, void* out, ResultFormat fmt);
  void finish_wire();
  // True when batches of this length range stream packed letters (the swipe kernel takes them).
  bool streams_packed(int64_t min_l2, int64_t max_l2) const;
  // Smallest result format for this problem given the batch's length range (min_l2 <= 0: unknown,
  // R2 not considered).
  ResultFormat auto_format(int64_t max_l2, int64_t min_l2 = 0) const;
  R2Params r2_params_for(int64_t min_l2, int64_t max_l2) const;

  // Device-resident batch: d_codes/d_offsets/d_out on this device; h_offsets is a host copy of the
  // offsets used for planning. Work is queued on `stream` (0 = engine compute stream); no sync.
  // Device time of the last solve_device's kernels (events recorded around its launches, after the host
  // planning): waits for them. Kernel throughput without the host's per-call planning in the interval.
  double device_kernel_ms();
  void solve_device(const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets, int64_t n,
                    Result* d_out, hipStream_t stream);

  // ---- per-offset score profile and top-K alignments (definitions: moc/cpu_engine.hpp; kernels:
  // csrc/src/hip/profile_kernels.hip). Byte letters and dense int64 offsets; wire-format batches go through the
  // *_wire forms below (a device-side decode first). The context-parallel split is not part of these calls.
  // Device-resident forms, queued on `stream` (0 = engine compute stream) with no sync, like solve_device:
  // d_prof receives the batch's flat profile (sum of candidate_offsets entries, record i's at the host-computed
  // profile offset i), d_out the int32 [n, K, 3] top-K rows, 1 <= K <= kMaxTopK. Top-K never materialises the
  // batch's profile: it runs chunk by chunk (profile kernel, then select) in a scratch bounded by
  // EngineOptions::profile_scratch_bytes.
  void solve_profile_device(const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets, int64_t n,
                            ProfileEntry* d_prof, hipStream_t stream);
  // radius (here and in every top-K / hits call below): 0 = the plain results, through exactly the launches above;
  // 1 .. bounds::kPeaksMaxRadius = the distinct forms (moc/cpu_engine.hpp peaks_filter) — per chunk the peak kernels
  // (csrc/src/hip/peaks_kernels.hip) run between the profile kernel and the select / hits launches, on the same
  // stream with no sync, over one byte of peak marks per scratch entry (counted under profile_scratch_bytes), and
  // the select / count / compact kernels take their masked forms. Anything else throws.
  void solve_topk_device(const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets, int64_t n, int K,
                         Result* d_out, hipStream_t stream, int64_t radius = 0);
  // Host forms (upload through the pooled buffers; synchronous). prof_out holds poffsets_out[n] entries;
  // poffsets_out (n + 1) is filled first and may be computed beforehand with profile_offsets().
  void solve_profile(const uint8_t* codes, const int64_t* offsets, int64_t n, ProfileEntry* prof_out,
                     int64_t* poffsets_out);
  void solve_topk(const uint8_t* codes, const int64_t* offsets, int64_t n, int K, Result* out, int64_t radius = 0);
  // poffsets[0..n]: record i's profile starts at entry poffsets[i] (this problem's L1 and semantics)
  void profile_offsets(const int64_t* offsets, int64_t n, int64_t* poffsets) const;
  void set_profile_scratch(int64_t bytes);
  // Device time (ms) of the select launches of the last top-K call; recorded only when MOC_PROFILE_TIMING=1
  // was set at engine start (an event pair per chunk), else 0. Waits for them.
  double topk_select_ms();

  // ---- threshold hits (definitions: moc/cpu_engine.hpp hits_batch_cpu; kernels: csrc/src/hip/hits_kernels.hip):
  // every offset whose profile score is >= the record's threshold, as rows (score, n = o, k) in ascending o, record
  // i's at rows[hoffsets[i] .. hoffsets[i + 1]). Limits as top-K: byte letters and dense int64 offsets (wire batches:
  // solve_hits_wire), n < 2^31 - 1.
  // Device form: queued on `stream` (0 = engine compute stream) with no sync, in the chunks of top-K under
  // profile_scratch_bytes — per chunk the profile kernel, then count, prefix sum and compaction. d_thresholds:
  // device int32 [n], or null for min_score on every record. d_hoffsets (int64 [n + 1]) is always complete and
  // exact; a row is stored iff its flat index is < cap, and nothing at or past d_rows + cap is touched (cap == 0
  // with a null d_rows counts only).
  void solve_hits_device(const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets, int64_t n,
                         int32_t min_score, const int32_t* d_thresholds, int64_t* d_hoffsets, Result* d_rows,
                         int64_t cap, hipStream_t stream, int64_t radius = 0);
  // Host form (uploads through the pooled buffers; synchronous; fills stats()). thresholds: host int32 [n] or null.
  // Optimistic: one pass with room for max(max_rows_hint, 1) rows (hint < 0: 4 n), and exactly one more with
  // hoffsets[n] rows when that was too few (the counts are exact, so the second pass fits). hits_passes() tells.
  void solve_hits(const uint8_t* codes, const int64_t* offsets, int64_t n, int32_t min_score,
                  const int32_t* thresholds, int64_t* hoffsets_out, std::vector<Result>& rows_out,
                  int64_t max_rows_hint = -1, int64_t radius = 0);
  int hits_passes() const { return hits_passes_; }  // passes of the last solve_hits (1 or 2; 0 for n <= 0)
  // Device time (ms) of the count + scan + compact launches of the last hits call; as topk_select_ms().
  double hits_select_ms() { return topk_select_ms(); }

  // ---- profile summary (definitions: moc/cpu_engine.hpp summary_batch_cpu; kernels:
  // csrc/src/hip/summary_kernels.hip): per record the row (count, sum, sumsq, min, max, n, k) of its whole profile as
  // seven int64 and, with bins > 0, an int32 [bins] histogram of its scores (bin = clamp(floor((s - lo) / width), 0,
  // bins - 1)). Limits as hits: byte letters and dense int64 offsets (wire batches: solve_summary_wire), n < 2^31 - 1;
  // no radius and no threshold. Before anything is launched or any state changes, bins (0 .. kSummaryMaxBins), width
  // (>= 1) and the exactness bound of the batch (bounds::summary_exact over max |W|, the longest record and the
  // longest profile) are checked, and a call outside them throws an Error that starts with "summary:".
  // Device form: queued on `stream` (0 = engine compute stream) with no sync, in the chunks of hits under
  // profile_scratch_bytes — per chunk the profile kernel, then the summary kernel and, with bins > 0, the histogram
  // kernel. d_summary: device int64 [n * 7]; d_hist: device int32 [n * bins], never touched with bins == 0. An empty
  // batch launches nothing.
  void solve_summary_device(const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets, int64_t n,
                            int64_t* d_summary, int32_t* d_hist, int32_t bins, int32_t lo, int32_t width,
                            hipStream_t stream);
  // Host form (uploads through the pooled buffers; synchronous; fills stats()). hist_out may be null with bins == 0.
  void solve_summary(const uint8_t* codes, const int64_t* offsets, int64_t n, int64_t* summary_out, int32_t* hist_out,
                     int32_t bins, int32_t lo, int32_t width);
  // Device time (ms) of the summary (and histogram) launches of the last summary call; as topk_select_ms().
  double summary_ms() { return topk_select_ms(); }

  // ---- multi-target search (definitions: moc/cpu_engine.hpp targets_batch_cpu; kernel:
  // csrc/src/hip/targets_kernels.hip): the engine's Seq1 is a catalog of T targets delimited by starts (int64
  // [T + 1], strictly rising from 0 to L1), and every record gets one row per target — what solve would return for
  // that record against that target alone, n relative to the target's start: rows [n * T], record-major. Limits as
  // hits: byte letters and dense int64 offsets (wire batches: solve_targets_wire), n < 2^31 - 1. Before anything is
  // launched or any state changes, T (1 .. bounds::kTargetsMax) and starts are checked, and a call outside them
  // throws an Error that starts with "targets:".
  // Device form: queued on `stream` (0 = engine compute stream) with no sync, in the chunks of hits under
  // profile_scratch_bytes — per chunk the profile kernel over the catalog, then the targets select kernel over the
  // chunk's (record, target) pairs, its lane-group size chosen from the chunk's longest slice
  // (bounds::targets_group; MOC_TARGETS_GROUP=4|16|64 at engine start forces one). d_starts: a device copy of
  // h_starts, or null — then h_starts is uploaded with the plan buffer. h_starts is read during the call only.
  // d_out: device Result [n * T], every row stored. An empty batch launches nothing.
  void solve_targets_device(const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets, int64_t n,
                            const int64_t* d_starts, const int64_t* h_starts, int64_t T, Result* d_out,
                            hipStream_t stream);
  // Host form (uploads through the pooled buffers; synchronous; fills stats()).
  void solve_targets(const uint8_t* codes, const int64_t* offsets, int64_t n, const int64_t* starts, int64_t T,
                     Result* out);
  // The check every targets call makes first: throws unless a problem is set and (h_starts, T) is a valid target set
  // over its Seq1; touches nothing.
  void check_targets_call(const int64_t* h_starts, int64_t T) const;
  // Device time (ms) of the targets select launches of the last targets call (a target ranking: select and rank); as
  // topk_select_ms().
  double targets_ms() { return topk_select_ms(); }

  // ---- per-target profile summary (definitions: moc/cpu_engine.hpp targets_summary_batch_cpu; kernels:
  // csrc/src/hip/targets_summary_kernels.hip): the engine's Seq1 is a catalog as for solve_targets, and every
  // (record, target) pair gets the summary row (count, sum, sumsq, min, max, n, k) of its target profile as seven
  // int64 — summary [n * T * 7], record-major — and, with bins > 0, an int32 [bins] histogram of its scores, hist
  // [n * T * bins]. Limits as solve_targets. Before anything is launched or any state changes, the target set is
  // checked ("targets:" errors), then bins, width and the exactness bound over the largest target profile of the
  // call (targets_max_count; "summary:" errors) — the catalog's own profile may be past the bound.
  // Device form: queued on `stream` (0 = engine compute stream) with no sync, in the chunks of solve_targets — per
  // chunk the profile kernel over the catalog, then the per-target summary kernel and, with bins > 0, the histogram
  // kernel over the chunk's pairs, the lane group chosen as solve_targets chooses it. d_starts / h_starts as
  // solve_targets_device. d_hist is never touched with bins == 0. An empty batch launches nothing.
  void solve_targets_summary_device(const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets,
                                    int64_t n, const int64_t* d_starts, const int64_t* h_starts, int64_t T,
                                    int64_t* d_summary, int32_t* d_hist, int32_t bins, int32_t lo, int32_t width,
                                    hipStream_t stream);
  // Host form (uploads through the pooled buffers; synchronous; fills stats()). hist_out may be null with bins == 0.
  void solve_targets_summary(const uint8_t* codes, const int64_t* offsets, int64_t n, const int64_t* starts, int64_t T,
                             int64_t* summary_out, int32_t* hist_out, int32_t bins, int32_t lo, int32_t width);
  // Device time (ms) of the per-target summary (and histogram) launches of the last such call; as topk_select_ms().
  double targets_summary_ms() { return topk_select_ms(); }

  // ---- per-target top-K and threshold hits (definitions: moc/cpu_engine.hpp targets_topk_batch_cpu /
  // targets_hits_batch_cpu; kernels: csrc/src/hip/targets_rows_kernels.hip): the engine's Seq1 is a catalog as for
  // solve_targets, and every (record, target) pair gets the K best entries of its target profile — rows [n * T * K],
  // pair-major, padded with empty rows — or every entry at or above its threshold in ascending local offset, pair p =
  // i * T + t's rows at rows[toffsets[p] .. toffsets[p + 1]). n is local to the target in both. Limits as
  // solve_targets. Before anything is launched or any state changes the target set is checked ("targets:" errors),
  // then K (solve_topk's message) or the hits buffers (solve_hits_device's messages). targets_ms() covers the new
  // launches.
  // radius > 0, the distinct forms (kernels: csrc/src/hip/targets_peaks_kernels.hip): only the peaks of radius
  // `radius` of every pair's OWN profile are ranked or listed — its windows clipped to the pair's entries, the
  // boundary entry among them — which is solve_topk / solve_hits with that radius on the target alone. Checked after
  // the messages above ("distinct:" errors, 0 .. bounds::kPeaksMaxRadius). Per chunk the segmented peak pass runs
  // between the profile kernel and masked forms of the per-target kernels (segment width: bounds::targets_peaks_seg;
  // MOC_TARGETS_PEAKS_SEG=4|8|16|32|64 at engine start forces one); the profile scratch holds one more byte per entry.
  // radius = 0 is launch for launch the call without it.
  // Device forms: queued on `stream` (0 = engine compute stream) with no sync, in the chunks of solve_targets — per
  // chunk the profile kernel over the catalog, then the per-target top-K kernel, or count, prefix sum over the
  // chunk's pairs (hits' own scan launches) and compaction, the lane group chosen as solve_targets chooses it (top-K:
  // bounds::targets_topk_group, a wave from 257 slice entries on).
  // d_starts / h_starts as solve_targets_device. d_thresholds: device int32 [n * T] (pair-major), or null for
  // min_score on every pair. d_toffsets (int64 [n * T + 1]) is always complete and exact; a row is stored iff its
  // flat index is < cap, and nothing at or past d_rows + cap is touched (cap == 0 with a null d_rows counts only).
  // An empty batch launches nothing, apart from the 8-byte memset of d_toffsets[0] of the hits form.
  void solve_targets_topk_device(const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets, int64_t n,
                                 const int64_t* d_starts, const int64_t* h_starts, int64_t T, int K, Result* d_out,
                                 hipStream_t stream, int64_t radius = 0);
  void solve_targets_hits_device(const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets, int64_t n,
                                 const int64_t* d_starts, const int64_t* h_starts, int64_t T, int32_t min_score,
                                 const int32_t* d_thresholds, int64_t* d_toffsets, Result* d_rows, int64_t cap,
                                 hipStream_t stream, int64_t radius = 0);
  // Host forms (upload through the pooled buffers; synchronous; fill stats()). thresholds: host int32 [n * T] or null.
  // Hits is optimistic as solve_hits is: one pass with room for max(max_rows_hint, 1) rows (hint < 0: n * T), and
  // exactly one more with toffsets[n * T] rows when that was too few; hits_passes() tells.
  void solve_targets_topk(const uint8_t* codes, const int64_t* offsets, int64_t n, const int64_t* starts, int64_t T,
                          int K, Result* out, int64_t radius = 0);
  void solve_targets_hits(const uint8_t* codes, const int64_t* offsets, int64_t n, const int64_t* starts, int64_t T,
                          int32_t min_score, const int32_t* thresholds, int64_t* toffsets_out,
                          std::vector<Result>& rows_out, int64_t max_rows_hint = -1, int64_t radius = 0);

  // ---- target ranking (definitions: moc/cpu_engine.hpp targets_rank_batch_cpu; kernels:
  // csrc/src/hip/targets_kernels.hip, csrc/src/hip/targets_rank_kernels.hip): the engine's Seq1 is a catalog as for
  // solve_targets, and every record gets its M best fitting targets as rows (t, score, n, k) — rows [n * M],
  // record-major, padded with no_rank() — without the n * T pair rows ever existing as a whole. Limits as
  // solve_targets. Before anything is launched or any state changes the target set is checked ("targets:" errors),
  // then M (1 .. kMaxTopK; "rank:" errors).
  // Device form: queued on `stream` (0 = engine compute stream) with no sync. Per chunk the profile kernel over the
  // catalog, then the targets select kernel — its pair rows go into the chunk's part of the profile scratch, laid out
  // entries | pair rows [records * T] — then the rank kernel over the chunk's records. A chunk takes records while
  // 8 * entries + 12 * T * records stay within profile_scratch_bytes (plan::plan_profile's record_bytes; at least one
  // record). The select kernel's lane group is chosen as solve_targets chooses it, the rank kernel's from T
  // (bounds::targets_rank_group; MOC_TARGETS_RANK_GROUP=4|16|64 at engine start forces one). d_starts / h_starts as
  // solve_targets_device. d_out: device RankRow [n * M], every row stored. An empty batch launches nothing.
  // targets_ms() covers the select and rank launches.
  void solve_targets_rank_device(const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets, int64_t n,
                                 const int64_t* d_starts, const int64_t* h_starts, int64_t T, int M, RankRow* d_out,
                                 hipStream_t stream);
  // Host form (uploads through the pooled buffers; synchronous; fills stats()): the result slot and the copy back
  // are n * M * 16 bytes.
  void solve_targets_rank(const uint8_t* codes, const int64_t* offsets, int64_t n, const int64_t* starts, int64_t T,
                          int M, RankRow* out);

  // ---- alignment report (definitions: moc/cpu_engine.hpp report_batch_cpu; kernels:
  // csrc/src/hip/report_kernels.hip): the sign counts and, optionally, the marker bytes of caller-supplied rows.
  // Byte letters and dense int64 offsets (wire batches: report_wire); no Semantics (row validity does not depend on
  // it).
  // Device form: d_rows [n*K] rows, d_counts [n*K*4] int32 (16-byte aligned), d_marks null or K * letters bytes;
  // queued on `stream` (0 = engine compute stream) with no sync — directly behind solve_device /
  // solve_topk_device on the same stream. 1 <= K <= kMaxTopK.
  void report_device(const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets, int64_t n, int K,
                     const Result* d_rows, int32_t* d_counts, uint8_t* d_marks, hipStream_t stream);
  // Host form (uploads through the pooled buffers; synchronous; fills stats()). marks may be null.
  void report(const uint8_t* codes, const int64_t* offsets, int64_t n, int K, const Result* rows, int32_t* counts,
              uint8_t* marks);

  // ---- wire-format input (moc/wire.hpp; kernels: csrc/src/hip/wire_kernels.hip; host reference: decode_wire_cpu)
  // A wire batch as the byte letters and dense int64 offsets the calls above take, decoded on the GPU.
  struct DecodedWire {
    const uint8_t* d_codes;    // base pointer: record i starts at d_codes + offsets[i] (offsets stay absolute)
    const int64_t* d_offsets;  // device, n + 1 entries
    const int64_t* h_offsets;  // host copy, for planning
    int64_t n;
  };
  // Queues the decode on `stream` (0 = engine compute stream) with no sync, into buffers of the engine that grow
  // and are never freed per call (letters + 8 (n + 1) bytes); the result stays valid until the engine's next decode.
  // P33 letters go through launch_unpack33, 5-bit ones through launch_unpack5 (the stream then needs one readable
  // byte after its last letter's, as packed5_bytes leaves), byte letters on the device and dense device offsets are
  // used in place; sparse offsets are expanded by launch_wire_offsets. A host batch's packed letters, lengths and
  // sparse offsets are read in place by those kernels when they are page-locked (and allow_direct is on), else
  // copied to the device in packed form first; its byte letters and dense offsets are uploaded. b.device: every
  // pointer of `b` is device memory and `host_meta` carries host copies of its offsets (sparse or dense) and narrow
  // lengths, from which the host expands h_offsets; the device's dense offsets still come from the kernel.
  // device_kernel_ms() right after it gives the device time of the decode kernels.
  // codes_dst / offsets_dst (device; letters bytes / n + 1 entries): decode there instead of into the engine's
  // buffers, copying what would otherwise be used in place — the caller owns the result's lifetime.
  DecodedWire decode_wire_device(const WireBatch& b, const WireBatch* host_meta, hipStream_t stream,
                                 uint8_t* codes_dst = nullptr, int64_t* offsets_dst = nullptr);
  // Host forms on a host wire batch (pinned or pageable): the decode above, then the profile / top-K / hits / report
  // path of the byte-letter calls on the decoded buffers — same chunking under profile_scratch_bytes, same
  // hits_passes() and capacity contract. Synchronous; fill stats() (kernels bit 128 when a decode kernel ran,
  // h2d_bytes in wire-format bytes). The whole batch is decoded at once.
  void solve_profile_wire(const WireBatch& b, ProfileEntry* prof_out, int64_t* poffsets_out);
  void solve_topk_wire(const WireBatch& b, int K, Result* out, int64_t radius = 0);
  void solve_hits_wire(const WireBatch& b, int32_t min_score, const int32_t* thresholds, int64_t* hoffsets_out,
                       std::vector<Result>& rows_out, int64_t max_rows_hint = -1, int64_t radius = 0);
  void report_wire(const WireBatch& b, int K, const Result* rows, int32_t* counts, uint8_t* marks);
  void solve_summary_wire(const WireBatch& b, int64_t* summary_out, int32_t* hist_out, int32_t bins, int32_t lo,
                          int32_t width);
  void solve_targets_wire(const WireBatch& b, const int64_t* starts, int64_t T, Result* out);
  void solve_targets_summary_wire(const WireBatch& b, const int64_t* starts, int64_t T, int64_t* summary_out,
                                  int32_t* hist_out, int32_t bins, int32_t lo, int32_t width);
  void solve_targets_topk_wire(const WireBatch& b, const int64_t* starts, int64_t T, int K, Result* out,
                               int64_t radius = 0);
  void solve_targets_hits_wire(const WireBatch& b, const int64_t* starts, int64_t T, int32_t min_score,
                               const int32_t* thresholds, int64_t* toffsets_out, std::vector<Result>& rows_out,
                               int64_t max_rows_hint = -1, int64_t radius = 0);
  void solve_targets_rank_wire(const WireBatch& b, const int64_t* starts, int64_t T, int M, RankRow* out);
  // poffsets[0..n] of a host wire batch (profile_offsets of its decoded lengths; no GPU work)
  void wire_profile_offsets(const WireBatch& b, int64_t* poffsets) const;

  // Context-parallel search: this engine evaluates part `part` of `parts` of the batch's
  // global list of offset tiles and writes one packed 64-bit key per record (moc::encode_key; 0 =
  // no candidate in this part). A MAX all-reduce of the keys over the parts + finalize_keys gives the
  // full answer; this splits single huge records across GPUs.
  void search_keys_device(const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets, int64_t n,
                          int part, int parts, unsigned long long* d_keys, hipStream_t stream);
  // MAX-combined pass-1 keys -> results (k resolved on each record's winning diagonal: needs the batch).
  void finalize_keys_device(const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets, int64_t n,
                            const unsigned long long* d_keys, void* d_out, ResultFormat fmt, hipStream_t stream);
  // Host-memory form of search_keys_device (uploads the batch, returns host keys; synchronous).
  void search_keys(const uint8_t* codes, const int64_t* offsets, int64_t n, int part, int parts, uint64_t* keys);

  // Page-locks a host range for the lifetime of the engine (or until unpin); enables the direct path.
  void pin(const void* p, size_t bytes);
  void unpin_all();
  // The registrations made by pin(), handed over to the caller (pinned::unregister them); forgotten here.
  std::vector<void*> detach_pins() {
    finish_wire();
    return std::exchange(pinned_, {});
  }

  const EngineStats& stats() const { return stats_; }
  int device() const { return device_; }
  hipStream_t compute_stream() const { return s_compute_; }
  int64_t L1() const { return cfg_.L1; }
  int num_cus() const { return cfg_.num_cus; }

 private:
  struct Slot;  // one double-buffer half
  // One chunk classified and planned: the short / swipe kernel's arguments and the tile plan of the rest.
  struct PlannedBatch {
    plan::ChunkPlan cp;
    dev::ShortArgs a;
    bool swipe = false, short_ok = false;
    bool all_tiles = false;  // the short kernel cannot hold its records (LDS budget): the tile kernel takes all
    int64_t n_long = 0;
    plan::TilePlan tp;
    std::vector<dev::WaveStart> starts;  // empty: no tile launch
    plan::PlanLayout lay{0, 0};
    const int32_t* lrecs() const { return all_tiles ? nullptr : cp.long_recs.data(); }  // null: the identity list
    size_t plan_bytes() const { return lay.total + (lrecs() ? 0 : sizeof(unsigned long long) * static_cast<size_t>(n_long)); }
  };
  struct Ran {
    int32_t kernels = 0, forms = 0;  // EngineStats bits
  };
  void plan_batch(const int64_t* offsets, int64_t n, ResultFormat fmt, PlannedBatch& pb) const;
  void upload_plan(const PlannedBatch& pb, void*& h_plan, size_t& h_cap, void*& d_plan, size_t& d_cap, hipStream_t s);
  Ran launch_planned(PlannedBatch& pb, const dev::BatchView& bv, int64_t first_offset, void* d_out, unsigned* counter,
                     void* d_plan, ResultFormat fmt, hipStream_t s);
  // A host call's batch once it is on the device, with what the placement adds to stats() and the call's wall
  // clock, started before the placement: the host forms' bodies (*_placed) take it from there. n <= 0: nothing placed.
  struct Placed {
    const uint8_t* d_codes = nullptr;
    const int64_t* d_offsets = nullptr;
    const int64_t* h_offsets = nullptr;
    int64_t n = 0;
    int64_t h2d_bytes = 0;
    int32_t kernels = 0;
    Stopwatch wall;
  };
  // Host byte letters and dense offsets -> slot 0's pooled buffers on the compute stream, its d_out grown to
  // out_bytes, after finish_wire and hipSetDevice. The offsets go up rebased to 0; h_offsets is that copy.
  Placed place_host(const uint8_t* codes, const int64_t* offsets, int64_t n, size_t out_bytes);
  // A validated host wire batch decoded on the compute stream (decode_wire_device), d_out likewise.
  Placed place_wire(const WireBatch& b, size_t out_bytes);
  // The *_placed bodies' tail: the device form has filled consecutive segments of slot 0's d_out; copies each
  // non-empty one back, waits for the compute stream and fills stats().
  struct OutSegment {
    void* host;
    size_t bytes;
  };
  void finish_placed(Placed& p, std::initializer_list<OutSegment> segments);
  void host_call_stats(Placed& p, double kernel_ms, size_t d2h_bytes);
  static size_t report_out_bytes(int64_t n, int K, int64_t mark_letters);
  void profile_placed(Placed& p, ProfileEntry* prof_out, const int64_t* poffsets);
  void topk_placed(Placed& p, int K, Result* out, int64_t radius);
  void hits_placed(Placed& p, int32_t min_score, const int32_t* thresholds, int64_t* hoffsets_out,
                   std::vector<Result>& rows_out, int64_t max_rows_hint, int64_t radius);
  void summary_placed(Placed& p, int64_t* summary_out, int32_t* hist_out, int32_t bins, int32_t lo, int32_t width);
  void targets_placed(Placed& p, const int64_t* starts, int64_t T, Result* out);
  void targets_summary_placed(Placed& p, const int64_t* starts, int64_t T, int64_t* summary_out, int32_t* hist_out,
                              int32_t bins, int32_t lo, int32_t width);
  void targets_topk_placed(Placed& p, const int64_t* starts, int64_t T, int K, Result* out, int64_t radius);
  void targets_hits_placed(Placed& p, const int64_t* starts, int64_t T, int32_t min_score, const int32_t* thresholds,
                           int64_t* toffsets_out, std::vector<Result>& rows_out, int64_t max_rows_hint, int64_t radius);
  void targets_rank_placed(Placed& p, const int64_t* starts, int64_t T, int M, RankRow* out);
  void report_placed(Placed& p, int K, const Result* rows, int32_t* counts, uint8_t* marks);
  void ensure_device_events();  // ev_d0_ / ev_d1_, made by the first call that records them
  dev::Plan device_plan(void* d_plan, size_t n_starts, bool has_long_recs, int64_t n_long, const plan::TilePlan& tp,
                        unsigned long long* keys = nullptr) const;
  // problem view for a plan: without the profile when the plan is for the LUT tile kernel
  dev::ProblemView tile_view(int64_t max_l2, const plan::TilePlan& tp) const {
    dev::ProblemView pv = problem_view(max_l2);
    if (!tp.tile16) {
      pv.prof16 = nullptr;
      pv.mfma_sweep = 0;
    } else {  // the plan's image: whole or windowed, byte pairs or widened
      pv.prof16_window = static_cast<int32_t>(tp.window);
      pv.prof16_bytes = tp.window ? static_cast<int32_t>(dev::tile16_window_bytes(tp.window)) : cfg_.prof16_bytes;
      pv.prof16_wide = tp.wide ? 1 : 0;
      pv.t16_slide = tp.slide ? tp.slide_per_cu : 0;
      if (tp.window) pv.mfma_sweep = 0;
      if (!pv.mfma_sweep) pv.t16_key_bits = bounds::tile16_key32_bits(cfg_.L1, table_.max_abs(), max_l2);
    }
    return pv;
  }
  dev::ProblemView problem_view(int64_t max_l2) const;
  void ensure(void*& ptr, size_t& cap, size_t bytes);
  void ensure_host(void*& ptr, size_t& cap, size_t bytes);
  bool direct_pointers(const WireBatch& b, void* out, int fb, dev::ShortArgs& a) const;
  bool prepare_direct(const dev::ProblemView& pv, const dev::ShortArgs& a, bool swipe);
  void launch_direct(const dev::ProblemView& pv, const dev::ShortArgs& a, bool swipe, bool graph);
  void run_staged(const uint8_t* codes, const int64_t* offsets, int64_t n, void* out, ResultFormat fmt,
                  bool packed5);
  void solve_wire_impl(const WireBatch& b, void* out, ResultFormat fmt, bool async);
  // ---- the profile family: one run loop over plan::plan_profile's chunks; a ProfileCall names the form
  enum class ProfileKind { Profile, TopK, Hits, Summary, Targets, TargetsSummary, TargetsTopK, TargetsHits, TargetsRank };
  struct HitsCall {
    int32_t min_score;
    const int32_t* d_thresholds;
    int64_t* d_hoffsets;
    Result* d_rows;
    int64_t cap;
  };
  struct SummaryCall {
    int64_t* d_summary;
    int32_t* d_hist;  // null: no histogram
    int32_t bins, lo, width;
  };
  struct TargetsCall {
    const int64_t* d_starts;  // device [T + 1], or null: h_starts goes up with the plan buffer
    const int64_t* h_starts;
    int64_t T;
    Result* d_out;            // Targets: [n, T]; TargetsTopK: [n, T, K]
    RankRow* d_rank = nullptr;  // TargetsRank: [n, M] (M in ProfileCall::K); d_out is not used
  };
  struct ProfileCall {
    ProfileKind kind = ProfileKind::Profile;
    void* d_dst = nullptr;  // Profile: ProfileEntry [poffsets[n]], written in one chunk; TopK: Result [n, K]
    int K = 0;              // TopK, TargetsTopK; TargetsRank: M
    int64_t radius = 0;     // TopK, Hits: > 0 selects among the peaks of that radius only
    HitsCall hits{};        // Hits; TargetsHits: over pairs (d_hoffsets is toffsets, d_thresholds int32 [n * T])
    SummaryCall summary{};  // Summary, TargetsSummary
    TargetsCall targets{};  // Targets, TargetsSummary, TargetsTopK, TargetsHits, TargetsRank
  };
  void run_profile(const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets, int64_t n,
                   const ProfileCall& call, hipStream_t stream);
  // These throw unless the call is allowed and touch nothing: bins, width and the batch's exactness bound
  // (bounds::summary_exact); the target set (check_targets_call), then the summary's checks over the call's largest target profile.
  void check_summary(const int64_t* h_offsets, int64_t n, int32_t bins, int32_t width) const;
  void check_targets_summary(const int64_t* h_offsets, int64_t n, const int64_t* h_starts, int64_t T, int32_t bins,
                             int32_t width) const;

  EngineOptions opt_;
  int device_ = 0;
  plan::Config cfg_;  // the problem's length and profile geometry, the device's CUs, the tuning switches
  hipStream_t s_copy_ = nullptr, s_compute_ = nullptr, s_return_ = nullptr;  // copy / return: made on first use
  void ensure_side_streams();
  // problem
  ScoreTable table_{};
  int32_t min_t_ = 0, max_t_ = 0;  // pair-score range over letters (R2 parameters)
  R2Params r2_{};                  // R2 parameters of the current solve
  void* d_image_ = nullptr;  // problem image: LUT | Seq1 | profile (views below)
  size_t d_image_cap_ = 0;
  // page-locked staging of the image: the upload is one copy kernel on the compute stream (dev::launch_copy;
  // a pageable hipMemcpy, or any copy the runtime gives its SDMA engine, cost 8-34 ms of engine start-up
  // inside a tiny job's first search on the box, profiles/copy_path_probe.log)
  void* h_image_ = nullptr;
  size_t h_image_cap_ = 0;
  std::vector<uint8_t> image_;
  Weights last_w_{};                // the last set_problem's inputs: a repeat returns at once
  std::vector<uint8_t> last_seq1_;
  int32_t* d_lut_ = nullptr;
  uint8_t* d_seq1_ = nullptr;
  uint16_t* d_prof16_ = nullptr;  // tile16 profile (null: the problem does not fit it, or MOC_TILE16=0)
  int64_t prof16_entries_ = 0;   // entries of the device profile (windowed staging bounds)
  bool tile16_ = true;            // MOC_TILE16 (A/B switch of the long-record kernel)
  Semantics sem_ = Semantics::Reference;
  bool have_problem_ = false;
  std::vector<std::unique_ptr<Slot>> slots_;
  unsigned* d_counter_ = nullptr;  // direct-path work counter
  hipEvent_t ev_a_ = nullptr, ev_b_ = nullptr;
  // scratch for solve_device
  void* d_plan_ = nullptr;
  size_t d_plan_cap_ = 0;
  void* h_plan_ = nullptr;
  size_t h_plan_cap_ = 0;
  hipEvent_t ev_plan_ = nullptr;
  hipEvent_t ev_d0_ = nullptr, ev_d1_ = nullptr;  // around solve_device's launches (device_kernel_ms)
  // top-K / hits: the chunks' profile scratch, and event pairs around the select / hits launches
  // (MOC_PROFILE_TIMING=1)
  void* d_prof_scratch_ = nullptr;
  size_t d_prof_scratch_cap_ = 0;
  bool profile_timing_ = false;
  int targets_group_ = 0;  // MOC_TARGETS_GROUP: 4, 16 or 64 forces that lane-group size; 0: chosen per chunk
  int targets_rank_group_ = 0;  // MOC_TARGETS_RANK_GROUP: 4, 16 or 64 forces that lane-group size of the rank kernel; 0: from T
  int targets_peaks_seg_ = 0;  // MOC_TARGETS_PEAKS_SEG: 4, 8, 16, 32 or 64 forces that segment width of the per-target peak pass
  std::vector<hipEvent_t> ev_select_;
  size_t ev_select_used_ = 0;
  // hits: the scan's block sums, the host form's row buffer, and its pass count
  void* d_hits_sums_ = nullptr;
  size_t d_hits_sums_cap_ = 0;
  void* d_hits_rows_ = nullptr;
  size_t d_hits_rows_cap_ = 0;
  int hits_passes_ = 0;
  // wire decode: the decoded batch (offsets | letters), the packed input of pageable host batches, the host copy
  // of the dense offsets, and what the last decode moved and launched
  void* d_wire_ = nullptr;
  size_t d_wire_cap_ = 0;
  void* d_wire_in_ = nullptr;
  size_t d_wire_in_cap_ = 0;
  std::vector<int64_t> wire_h_offsets_;
  std::vector<int64_t> host_offsets_;  // place_host: the rebased offsets as uploaded
  int64_t wire_h2d_ = 0;
  int32_t wire_kernels_ = 0;
  std::vector<void*> pinned_;
  struct DirectKey {
    dev::ProblemView pv;
    dev::ShortArgs a;
    int32_t swipe;
  };
  static constexpr int kGraphs = 2;
  DirectKey graph_key_[kGraphs]{};
  hipGraphExec_t graph_exec_[kGraphs] = {nullptr, nullptr};
  int graph_cur_ = 0;
  // the last two argument sets launched without a graph (captured when seen again; a streaming job's ring
  // alternates two)
  DirectKey seen_key_[kGraphs]{};
  bool seen_valid_[kGraphs] = {false, false};
  int seen_next_ = 0;
  bool pending_ = false;  // a begin_wire solve is in flight (ev_a_ .. ev_b_)
  Stopwatch pending_wall_;
  EngineStats stats_;
};

// Picks the int32 hot-loop key width for a problem: bits for k, or 0 (=> 64-bit keys) when
// 2*max|T|*L2 does not fit next to them in an int32.
int32_t choose_key_shift(int32_t max_abs_weight, int64_t max_l2);

}  // namespace moc
