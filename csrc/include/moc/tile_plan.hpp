// Host-side work planning for the tile kernels (LUT tiles, tile16 whole / windowed / sliding, MFMA, the
// per-offset profile): which records go to which kernel, and the cost-balanced runs of wave tiles every
// persistent wave walks. Pure integer arithmetic over host offsets — no HIP runtime call — so a plan can be
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
