// Host-side work planning for the tile kernels (LUT tiles, tile16 whole / windowed / sliding, MFMA, the
// per-offset profile): which records go to which kernel, the cost-balanced runs of wave tiles every
// persistent wave walks, and the chunks of records the profile family passes through its bounded scratch. Pure integer arithmetic over host offsets — no HIP runtime call — so a plan can be
// built and checked without a device (csrc/tests/test_core.cpp walks every plan the way the kernels do).
// HipEngine owns one plan::Config, uploads what these functions return and launches from it.
#pragma once

#include <cstdint>
#include <vector>

#include "moc/device.hpp"
#include "moc/score_table.hpp"

namespace moc {
namespace plan {

// Everything the planner reads: the problem's profile geometry (set_profile_geometry), the device, and the
// engine's tuning switches (environment, HipEngine's constructor).
struct Config {
  // ---- problem
  int64_t L1 = 0;
  bool has_prof16 = false;       // a tile16 profile exists (else: weights or Seq1 do not fit it, or MOC_TILE16=0)
  int32_t prof16_bytes = 0;      // LDS bytes of the profile part of a workgroup's whole image
  int32_t prof16_overhang = 0;   // zero profile entries past the last row (bounds the tile span)
  int32_t prof16_window = 0;     // > 0: windowed tile16 (columns per workgroup window; Seq1 > one LDS image)
  bool prof16_wide = false;      // the sweep stages widened int16 pairs (dev::ProblemView::prof16_wide)
  bool prof16_i16 = false;       // the profile holds one int16 Dt per entry (dev::ProblemView::prof16_i16)
  // ---- device
  int num_cus = 256;
  // ---- switches
  bool mfma = false;               // MOC_MFMA: tile16 plans swept on the matrix cores (tile_mfma_kernels.hip)
  int tile_u = 0;                  // sub-tiles per wave tile (0 = per batch; MOC_TILE_U = 1|2|4|8)
  bool tile16_window_wide = true;  // widened windows for short records where the widened whole image is too big
  bool short_window_u8 = true;     // ... with 8 sub-tiles per wave tile (MOC_TILE16_WIN_U8=0: 4)
  bool tile16_slide = true;        // long records past the widened image: sliding windows (MOC_TILE16_SLIDE=0: not)
  int slide_wgs_per_cu = 2;        // ... two workgroups per CU, half-LDS windows (MOC_TILE16_SLIDE_WG=1: one)
  int tile_waves_per_cu = 32;      // LUT tile-kernel waves per CU (MOC_TILE_WAVES_PER_CU)
};

// Zero entries a problem's profile carries past its last row: build_profile16's overhang for this L1.
int64_t profile16_overhang(int64_t L1);
// Fills the problem side of `c` for a Seq1 of L1 letters and its profile, built with profile16_overhang(L1)
// (null: none). wide_env: MOC_TILE16_WIDE (0 keeps a whole image's byte pairs; A/B runs, same results).
void set_profile_geometry(Config& c, int64_t L1, const Profile16* prof, bool wide_env);

// A chunk's records split into the short-kernel set (<= 64 lanes) and the long list (tile kernel).
struct ChunkPlan {
  int64_t min_short = 0, max_l2 = 0, n_short = 0, cells = 0;
  std::vector<int32_t> long_recs;  // sorted
};
void plan_chunk(const Config& c, const int64_t* offsets, int64_t n, ChunkPlan& cp);

// The staged pipeline's cut (HipEngine::run_staged). End (exclusive) of the chunk that starts at record rb: the
// longest run rb..re with re - rb <= chunk_records and offsets[re] - offsets[rb] <= chunk_bytes, and at least one
// record (a record longer than chunk_bytes is a chunk of its own). offsets: n + 1 absolute entries (any first
// offset); 0 <= rb < n; both limits >= 1.
int64_t staged_chunk_end(const int64_t* offsets, int64_t n, int64_t rb, int64_t chunk_records, int64_t chunk_bytes);
// Every chunk of a batch: the bounds 0 = b0 < b1 < ... = n into bounds_out (room for n + 1 entries); returns their
// count minus one. Stops after n chunks whatever staged_chunk_end answers (a cut that does not advance cannot hang
// a caller: the last bound is then short of n).
int64_t staged_chunks(const int64_t* offsets, int64_t n, int64_t chunk_records, int64_t chunk_bytes, int64_t* bounds_out);

struct TilePlan {
  int u = 2;              // sub-tiles per wave tile
  int win_tiles = 0;      // windowed tile16: tiles per window stride
  bool tile16 = false;    // the plan is for the tile16 sweep (else the LUT tile kernel)
  int64_t window = 0;     // tile16: columns per LDS window (0: the whole profile is the image)
  bool wide = false;      // tile16: widened int16-pair entries
  bool slide = false;     // tile16: sliding widened windows (window = their columns; dev::Plan::slide_*)
  int64_t slide_items = 0, slide_members = 0, slide_wgs = 0;
  int slide_per_cu = 1;  // workgroups per CU the slide plan is for (1, or 2 with half-LDS windows)
};

// Layout of one chunk's tile plan in a single buffer: wave starts | long_recs | keys (8-aligned). Identity
// record lists upload no long_recs (n_long = 0 here): their keys follow the starts.
struct PlanLayout {
  size_t starts_off = 0, long_off = 0, keys_off = 0, upload_bytes = 0, total = 0;
  PlanLayout(size_t n_starts, size_t n_long) {
    long_off = n_starts * sizeof(dev::WaveStart);
    keys_off = (long_off + n_long * sizeof(int32_t) + 7) & ~size_t{7};
    upload_bytes = long_off + n_long * sizeof(int32_t);
    total = keys_off + n_long * sizeof(unsigned long long);
  }
};

// Per-tile fixed cost in step units (record/tile setup, the wave reduction), for load balancing.
constexpr int64_t kTileOverheadSteps = 24;
// Staging one sliding window (tile16_slide_kernel), per wave, in step units.
constexpr int64_t kSlideStageSteps = 96;

// Letters of long record li: offsets-relative record long_recs[li], or li when long_recs is null.
inline int64_t long_length(const int64_t* offsets, const int32_t* long_recs, int64_t li) {
  const int64_t r = long_recs ? long_recs[li] : li;
  return offsets[r + 1] - offsets[r];
}

// ntiles[li] wave tiles of `span` offsets, of tcost[li] steps each, for every long record; returns their count.
int64_t tile_costs(const Config& c, const int64_t* offsets, const int32_t* long_recs, int64_t n_long, int span,
                   std::vector<int32_t>& ntiles, std::vector<int64_t>& tcost);
// Part `part` of `parts` (by cost) of a record-major tile list — record li has ntiles[li] tiles of tcost[li]
// each — cut into contiguous, cost-balanced runs for at most max_waves waves: n_waves + 1 run boundaries.
std::vector<dev::WaveStart> balanced_runs(const std::vector<int32_t>& ntiles, const std::vector<int64_t>& tcost,
                                          int64_t total_tiles, int part, int parts, int64_t max_waves);
bool plan_slide(const Config& c, const int64_t* offsets, const int32_t* long_recs, int64_t n_long, double min_fill,
                TilePlan& tp, std::vector<dev::WaveStart>& starts);
std::vector<dev::WaveStart> plan_waves(const Config& c, const int64_t* offsets, const int32_t* long_recs,
                                       int64_t n_long, int part, int parts, TilePlan& tp);
// Sub-tiles per wave tile of the per-offset profile kernel (LUT-tile geometry) for a batch of n records with
// sum_l2 letters whose widest record needs max_need lanes; profile_runs: one chunk's runs with them.
int profile_u(const Config& c, int64_t sum_l2, int64_t n, int64_t max_need);
std::vector<dev::WaveStart> profile_runs(const Config& c, const int64_t* offsets, int64_t n, int u);

// ---- the profile family (profile, top-K, hits, summary, targets, per-target summary): the chunks of consecutive
// records that share a pass through the bounded profile scratch, and each chunk's wave runs. A profile call is one
// chunk whatever the budget (its entries go to the caller's buffer); the others take records while their entries fit
// scratch_bytes / entry_bytes (at least one entry), a record alone when its own profile is larger.
struct ProfileChunk {
  int64_t r0 = 0, r1 = 0;              // records [r0, r1)
  size_t starts_at = 0, n_starts = 0;  // its runs: ProfilePlan::starts[starts_at .. starts_at + n_starts), n_starts - 1 waves
  int64_t entries = 0;                 // poff[r1] - poff[r0]
  int64_t min_l2 = 0, max_l2 = 0;      // its shortest and longest record
  // distinct forms (radius > 0), what dev::PeaksArgs states of a chunk: a record of 1 .. bounds::kPeaksWaveEntries
  // entries; tiles of bounds::kPeaksTile entries of its longest profile when that is longer, else 0; the most keys
  // such a tile puts into LDS, halo included
  int32_t any_short = 0, max_tiles = 0, lds_keys = 0;
  // per-target distinct forms (radius > 0 with targets), what dev::TargetsPeaksArgs states of a chunk, from the target
  // lengths and the chunk's shortest and longest record (bounds::targets_pair_count): t_seg, the segment width (4, 8, 16,
  // 32 or 64: bounds::targets_peaks_seg of the longest pair profile, or the forced one); t_any_short, some pair profile
  // may have 2 .. t_seg entries; t_max_tiles, tiles of bounds::kPeaksTile entries of the longest pair profile when
  // that has more than t_seg entries, else 0; t_lds_keys, the most keys such a tile puts into LDS, halo included.
  // All 0 otherwise, and the three fields above stay 0 for such a call (the plain peak pass never runs for it).
  int32_t t_seg = 0, t_any_short = 0, t_max_tiles = 0, t_lds_keys = 0;
};
struct ProfilePlan {
  std::vector<int64_t> poff;           // the batch's profile index, n + 1 entries
  int u = 2;                           // sub-tiles per wave tile, one choice for the batch
  std::vector<dev::WaveStart> starts;  // every chunk's runs, li relative to the chunk's r0
  std::vector<ProfileChunk> chunks;    // in order, together [0, n)
  int64_t max_entries = 0, max_records = 0;  // of the largest chunk
  int64_t max_l2 = 0, cells = 0;       // of the batch
  int64_t max_target = 0;              // the longest target (0 without targets): with a chunk's min_l2, its longest slice
  // plan buffer: poff at 0 | starts at starts_off | the target starts (T + 1, when they travel with the plan) at
  // targets_off; every part 8-byte aligned
  size_t starts_off = 0, targets_off = 0, bytes = 0;
};
// entry_bytes: 8, or 9 with a byte of peak marks beside every entry. radius: 0, or the peaks radius (the chunks'
// peaks facts are filled only then). target_starts: null, or T + 1 host entries; upload_targets: they go into the
// plan buffer. radius > 0 with target_starts is a per-target distinct call: the chunks' t_* facts are filled in
// place of the plain peaks facts; targets_seg: 0, or the forced segment width (4, 8, 16, 32 or 64).
// record_bytes: scratch bytes a chunk needs per record beside its profile entries (the target ranking's pair rows, 12 T).
// 0: a chunk takes records while their entries number at most max(1, scratch_bytes / entry_bytes); > 0: while
// entry_bytes * entries + record_bytes * records <= scratch_bytes. Either way a chunk holds at least one record.
// Throws Error for n >= 2^31 - 1 and for Seq1 / Seq2 lengths of 2^30 and more; n >= 1.
ProfilePlan plan_profile(const Config& c, Semantics sem, const int64_t* offsets, int64_t n, bool chunked,
                         int64_t entry_bytes, int64_t scratch_bytes, int64_t radius, const int64_t* target_starts = nullptr,
                         int64_t T = 0, bool upload_targets = false, int targets_seg = 0, int64_t record_bytes = 0);

// ---- alignment report (report_kernels.hip): which records' rows take a lane each and which a wave each.
// Records of at most bounds::kReportShortMaxL2 letters are short. A wave of the lane-per-row kernel takes up to
// rpw = 64 / K consecutive short records (whole records: their K rows share the staged letters). When every
// record is short the waves are implicit — wave w takes records [w * rpw, min(n, w * rpw + rpw)) — and `items`
// stays empty; otherwise `items` lists each wave's run (never across a long record) and `long_recs` the rest.
struct ReportPlan {
  int K = 1;
  int rpw = 64;
  bool implicit = true;
  int64_t n_items = 0;
  std::vector<dev::ReportItem> items;
  std::vector<int32_t> long_recs;
};
// Throws Error unless 1 <= K <= kMaxTopK and n < 2^31 - 1.
ReportPlan plan_report(const int64_t* offsets, int64_t n, int K);

}  // namespace plan
}  // namespace moc
