#include "moc/tile_plan.hpp"

#include <omp.h>

#include <algorithm>
#include <queue>
#include <string>

#include "moc/cpu_engine.hpp"
#include "moc/problem.hpp"

namespace moc {
namespace plan {

namespace {
int64_t whole_profile_bytes(int64_t L1, int64_t oh) { return ((2 * ((kAlphabet - 1) * L1 + oh)) + 15) & ~int64_t{15}; }
}  // namespace

// The overhang (zero entries past the last row) must cover the widest tile span, 128*U entries: 1024 when
// that still fits the LDS (U = 8 for short records), else 512 (U <= 4, L1 up to 3052).
// Occupancy first: a CU holds two 16-wave workgroups when the image fits half its LDS, and the sweep is
// latency-bound, so the wide overhang (U = 8 tiles, for short records only) is kept only where it costs no
// workgroup: input3's 1489-letter Seq1 fits twice with 512 (32 waves per CU), once with 1024 (16).
int64_t profile16_overhang(int64_t L1) {
  const int64_t wide_oh = 2 * dev::kProf16Overhang, half = dev::kProf16MaxLds / 2;
  const int64_t lds = dev::tile16_lds_bytes(whole_profile_bytes(L1, wide_oh), L1);
  if (lds > dev::kProf16MaxLds ||
      (lds > half && dev::tile16_lds_bytes(whole_profile_bytes(L1, dev::kProf16Overhang), L1) <= half))
    return dev::kProf16Overhang;
  return wide_oh;
}

void set_profile_geometry(Config& c, int64_t L1, const Profile16* prof, bool wide_env) {
  const int64_t overhang = profile16_overhang(L1);
  // Seq1 too long for one LDS image: the whole profile lives in device memory and each workgroup stages
  // a window of it (tile16_search_kernel<U, true>); records must then fit a window with two tiles' slack
  const bool whole = dev::tile16_lds_bytes(whole_profile_bytes(L1, overhang), L1) <= dev::kProf16MaxLds;
  const int64_t window = whole ? 0 : dev::tile16_max_window();
  // weights past the byte pairs (|Dt| > 127) up to |Dt| <= 511: one int16 Dt per entry, which only the widened
  // images take (whole where it fits, windows for short records; otherwise the LUT tile kernel)
  const bool t16 = prof != nullptr;
  c.L1 = L1;
  c.has_prof16 = t16;
  c.prof16_i16 = t16 && prof->i16;
  c.prof16_window = t16 && !c.prof16_i16 ? static_cast<int32_t>(window) : 0;
  c.prof16_bytes = t16 ? dev::tile16_profile_lds_bytes(L1, overhang, c.prof16_i16) : 0;
  c.prof16_overhang = t16 ? static_cast<int>(overhang) : 0;
  // widened entries (two int16 halves per column: one packed add per lane and step) where the doubled image
  // still fits one CU
  c.prof16_wide = t16 && (whole || c.prof16_i16) && (wide_env || c.prof16_i16) &&
                  dev::tile16_lds_bytes(2 * static_cast<int64_t>(c.prof16_bytes), L1) <= dev::kProf16MaxLds;
}

// OpenMP: per-thread partial lists are concatenated in thread order, so long_recs stays sorted.
void plan_chunk(const Config& c, const int64_t* offsets, int64_t n, ChunkPlan& cp) {
  cp.long_recs.clear();
  const int64_t short_min_len = std::max<int64_t>(c.L1 - (dev::kWave - 1), 0);  // lanes_needed <= 64
  const int nt = n > (1 << 16) ? omp_get_max_threads() : 1;
  std::vector<std::vector<int32_t>> part(nt);
  std::vector<int64_t> mins(nt, INT64_MAX), maxs(nt, 0), nshort(nt, 0), cells(nt, 0);
#pragma omp parallel for schedule(static, 1) num_threads(nt)  // parts, not thread ids (any team size)
  for (int t = 0; t < nt; ++t) {
    const int64_t b = n * t / nt, e = n * (t + 1) / nt;
    int64_t mn = INT64_MAX, mx = 0, ns = 0, cl = 0;
    for (int64_t i = b; i < e; ++i) {
      const int64_t L2 = offsets[i + 1] - offsets[i];
      mx = std::max(mx, L2);
      cl += record_cells(c.L1, L2);
      if (L2 >= short_min_len) {
        mn = std::min(mn, L2);
        ++ns;
      } else {
        part[t].push_back(static_cast<int32_t>(i));
      }
    }
    mins[t] = mn;
    maxs[t] = mx;
    nshort[t] = ns;
    cells[t] = cl;
  }
  cp.min_short = INT64_MAX;
  cp.max_l2 = 0;
  cp.n_short = 0;
  cp.cells = 0;
  for (int t = 0; t < nt; ++t) {
    cp.min_short = std::min(cp.min_short, mins[t]);
    cp.max_l2 = std::max(cp.max_l2, maxs[t]);
    cp.n_short += nshort[t];
    cp.cells += cells[t];
    cp.long_recs.insert(cp.long_recs.end(), part[t].begin(), part[t].end());
  }
  if (c.L1 >= (int64_t{1} << 30) || cp.max_l2 >= (int64_t{1} << 30))
    throw Error("Seq1 / Seq2 lengths beyond 2^30 exceed the device engine's offset range");
}

int64_t staged_chunk_end(const int64_t* offsets, int64_t n, int64_t rb, int64_t chunk_records, int64_t chunk_bytes) {
  int64_t re = chunk_records < n - rb ? rb + chunk_records : n;  // (no sum that a huge limit could overflow)
  if (offsets[re] - offsets[rb] > chunk_bytes) {
    const int64_t byte_cap = offsets[rb] + chunk_bytes;
    re = std::upper_bound(offsets + rb + 1, offsets + re + 1, byte_cap) - offsets - 1;
    re = std::max(re, rb + 1);
  }
  return re;
}

int64_t staged_chunks(const int64_t* offsets, int64_t n, int64_t chunk_records, int64_t chunk_bytes, int64_t* bounds_out) {
  int64_t chunks = 0;
  bounds_out[0] = 0;
  for (int64_t rb = 0; rb < n && chunks < n; ++chunks) {
    rb = staged_chunk_end(offsets, n, rb, chunk_records, chunk_bytes);
    bounds_out[chunks + 1] = rb;
  }
  return chunks;
}

int64_t tile_costs(const Config& c, const int64_t* offsets, const int32_t* long_recs, int64_t n_long, int span,
                   std::vector<int32_t>& ntiles, std::vector<int64_t>& tcost) {
  ntiles.resize(static_cast<size_t>(n_long));
  tcost.resize(static_cast<size_t>(n_long));
  const int64_t L1 = c.L1;  // a local: the stores below cannot change it
  int64_t total_tiles = 0;
  for (int64_t li = 0; li < n_long; ++li) {
    const int64_t L2 = long_length(offsets, long_recs, li);
    ntiles[li] = static_cast<int32_t>(dev::tiles_of(dev::lanes_needed(L1, L2), span));
    tcost[li] = (L2 <= L1 ? L2 : 0) + kTileOverheadSteps;
    total_tiles += ntiles[li];
  }
  return total_tiles;
}

namespace {
// Position of cost threshold X in a tile list where record li holds count(li) tiles of tcost[li] each, numbered
// from t_base, and pre[li] is the cost before record li: the first tile whose start cost is >= X (`end` past
// the last one).
template <typename Count>
dev::WaveStart locate(const std::vector<int64_t>& pre, const std::vector<int64_t>& tcost, Count count, int64_t X,
                      int64_t t_base, dev::WaveStart end) {
  if (X >= pre.back()) return end;
  const int64_t li = std::upper_bound(pre.begin(), pre.end(), X) - pre.begin() - 1;
  const int64_t t = (X - pre[li] + tcost[li] - 1) / tcost[li];
  if (t >= count(li)) return dev::WaveStart{static_cast<int32_t>(li + 1), static_cast<int32_t>(t_base)};
  return dev::WaveStart{static_cast<int32_t>(li), static_cast<int32_t>(t_base + t)};
}

// The batch's sub-tiles per wave tile before a kernel's own limits: 4 amortises the per-tile setup over short
// records, 2 keeps more waves busy on long ones (measured, both kernels: profiles/tile_variants.log,
// profiles/tile16_variants.log); MOC_TILE_U overrides.
int batch_u(const Config& c, int64_t sum_l2, int64_t n) { return c.tile_u > 0 ? c.tile_u : (sum_l2 < 96 * n ? 4 : 2); }
}  // namespace

std::vector<dev::WaveStart> balanced_runs(const std::vector<int32_t>& ntiles, const std::vector<int64_t>& tcost,
                                          int64_t total_tiles, int part, int parts, int64_t max_waves) {
  const int64_t n_long = static_cast<int64_t>(ntiles.size());
  std::vector<int64_t> pre(static_cast<size_t>(n_long) + 1, 0);
  for (int64_t li = 0; li < n_long; ++li) pre[li + 1] = pre[li] + ntiles[li] * tcost[li];
  const int64_t C = pre[n_long];
  const int64_t lo = C * part / parts, hi = C * (part + 1) / parts;
  const int64_t part_tiles = std::max<int64_t>(1, total_tiles * (hi - lo) / std::max<int64_t>(C, 1));
  const int64_t n_waves = std::min<int64_t>(part_tiles, max_waves);
  std::vector<dev::WaveStart> starts(static_cast<size_t>(n_waves) + 1);
  for (int64_t w = 0; w <= n_waves; ++w)
    starts[w] = locate(pre, tcost, [&](int64_t li) { return ntiles[li]; }, lo + (hi - lo) * w / n_waves, 0,
                       dev::WaveStart{static_cast<int32_t>(n_long), 0});
  return starts;
}

// Sliding-window plan (tile16_slide_kernel): the long records sorted by length (longest first) in groups of 16,
// one per wave of a workgroup; a group's tiles split into items of at most half a workgroup's share, the
// items assigned largest first to the least-loaded workgroup (one 16-wave workgroup per CU: the window takes
// most of the LDS). Encoding in `starts` (dev::Plan::slide_items / slide_members). False: no window fits, or
// the groups would run less than min_fill of their waves (a few huge records: the other plans give every wave
// a tile of its own; an int16 profile's other plan is the LUT tile kernel, so it takes emptier groups).
bool plan_slide(const Config& c, const int64_t* offsets, const int32_t* long_recs, int64_t n_long, double min_fill,
                TilePlan& tp, std::vector<dev::WaveStart>& starts) {
  // 4 sub-tiles by default: limits 14.9 (U = 2) -> 16.7 T cells/s, the int16 profile on limits' lengths
  // 10.6 -> 13.8 (profiles/tile16_r5/README.txt)
  const int u = c.tile_u == 2 || (c.tile_u == 8 && c.slide_wgs_per_cu == 1) ? c.tile_u : 4;
  const int span = dev::tile_span(true, u);
  // two workgroups per CU with half the LDS each (8 waves per SIMD hide the sweep's LDS waits: limits 16.8 ->
  // 17.6 T cells/s, the int16 profile 16.9 -> 18.0), or one with the widest window (MOC_TILE16_SLIDE_WG=1)
  int64_t wmax = dev::tile16_max_window(true);
  if (c.slide_wgs_per_cu == 2)
    while (wmax > 0 && dev::tile16_lds_bytes(2 * dev::tile16_window_bytes(wmax), wmax) > dev::kProf16MaxLds / 2) --wmax;
  const int64_t C = (wmax - span) / 64 * 64;  // steps per window
  if (C < 64) return false;
  constexpr int G = dev::kTile16WavesPerBlock;
  if (static_cast<double>(n_long) < min_fill * static_cast<double>(G * ((n_long + G - 1) / G))) return false;
  std::vector<int32_t> order(static_cast<size_t>(n_long));
  std::vector<int32_t> steps(static_cast<size_t>(n_long));
  for (int64_t li = 0; li < n_long; ++li) {
    const int64_t L2 = long_length(offsets, long_recs, li);
    order[li] = static_cast<int32_t>(li);
    steps[li] = static_cast<int32_t>(L2 <= c.L1 ? L2 : 0);
  }
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return steps[a] > steps[b]; });
  const int64_t n_groups = (n_long + G - 1) / G;
  struct Item {
    int64_t cost;
    int32_t g, t0, t1;
  };
  std::vector<Item> items;
  std::vector<int32_t> glmax(static_cast<size_t>(n_groups), 0);
  int64_t total = 0;
  std::vector<int64_t> gcost(static_cast<size_t>(n_groups), 0);
  std::vector<int32_t> gtiles(static_cast<size_t>(n_groups), 0);
  for (int64_t g = 0; g < n_groups; ++g) {
    int32_t lmax = 0, nt = 0;
    for (int64_t k = g * G; k < std::min<int64_t>(n_long, (g + 1) * G); ++k) {
      const int32_t st = steps[order[k]];
      if (st <= 0) continue;
      lmax = std::max(lmax, st);
      nt = std::max<int32_t>(nt, static_cast<int32_t>(dev::tiles_of(c.L1 - st + 1, span)));
    }
    glmax[g] = lmax;
    gtiles[g] = nt;
    // a tile: every wave in lockstep for the group's longest record, plus the staging of each window
    gcost[g] = G * (lmax + kTileOverheadSteps + kSlideStageSteps * ((lmax + C - 1) / C));
    total += gcost[g] * nt;
  }
  if (total <= 0) return false;
  int64_t all_tiles = 0;
  for (int64_t g = 0; g < n_groups; ++g) all_tiles += gtiles[g];
  const int64_t n_wg = std::min<int64_t>(static_cast<int64_t>(c.num_cus) * c.slide_wgs_per_cu, all_tiles);
  const double share = static_cast<double>(total) / static_cast<double>(n_wg);
  for (int64_t g = 0; g < n_groups; ++g) {
    if (gtiles[g] <= 0) continue;
    const int32_t per = static_cast<int32_t>(std::max<int64_t>(1, static_cast<int64_t>(share / 2) / gcost[g]));
    for (int32_t t0 = 0; t0 < gtiles[g]; t0 += per) {
      const int32_t t1 = std::min(gtiles[g], t0 + per);
      items.push_back(Item{gcost[g] * (t1 - t0), static_cast<int32_t>(g), t0, t1});
    }
  }
  std::stable_sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return a.cost > b.cost; });
  std::vector<std::vector<int32_t>> of(static_cast<size_t>(n_wg));
  std::priority_queue<std::pair<int64_t, int64_t>, std::vector<std::pair<int64_t, int64_t>>, std::greater<>> load;
  for (int64_t b = 0; b < n_wg; ++b) load.emplace(0, b);
  for (size_t k = 0; k < items.size(); ++k) {
    auto [l, b] = load.top();
    load.pop();
    of[static_cast<size_t>(b)].push_back(static_cast<int32_t>(k));
    load.emplace(l + items[k].cost, b);
  }
  starts.clear();
  starts.reserve(static_cast<size_t>(n_wg + 1 + 2 * static_cast<int64_t>(items.size()) + n_groups * G));
  int32_t n_it = 0;
  for (int64_t b = 0; b < n_wg; ++b) {
    starts.push_back(dev::WaveStart{n_it, 0});
    n_it += static_cast<int32_t>(of[b].size());
  }
  starts.push_back(dev::WaveStart{n_it, 0});
  tp.slide_items = static_cast<int64_t>(starts.size());
  for (int64_t b = 0; b < n_wg; ++b)
    for (const int32_t k : of[b]) {
      const Item& it = items[k];
      starts.push_back(dev::WaveStart{it.g, it.t0});
      starts.push_back(dev::WaveStart{glmax[it.g], it.t1});
    }
  tp.slide_members = static_cast<int64_t>(starts.size());
  for (int64_t k = 0; k < n_groups * G; ++k) {
    if (k < n_long)
      starts.push_back(dev::WaveStart{order[k], static_cast<int32_t>(long_length(offsets, long_recs, order[k]))});
    else
      starts.push_back(dev::WaveStart{-1, 0});
  }
  tp.slide_wgs = n_wg;
  tp.slide_per_cu = c.slide_wgs_per_cu;
  tp.tile16 = true;
  tp.wide = true;
  tp.slide = true;
  tp.u = u;
  tp.window = span + C;
  tp.win_tiles = 0;
  return true;
}

// Cost-balanced contiguous wave runs over the record-major tile list of the long records (long_length's
// indexing), restricted to part `part` of `parts` of the total cost (context-parallel shares). Returns
// n_waves + 1 starts (empty: no work).
// tp: sub-tiles per wave tile, and which sweep the plan is for (tile16 when the problem has a profile and,
// for a windowed one, the records fit a window — else the LUT tile kernel).
// Windowed tile16 (Seq1 longer than one LDS image): the list is window-major — window m holds the tiles
// t in [m*T, (m+1)*T) of every record, T = (W - span - max L2) / span so that their profile columns
// [t*span, t*span + span + L2) all lie in [m*T*span, m*T*span + W) — and every window gets whole
// workgroups of waves (16-aligned; its last wave is an empty marker ending at (n_long, m*T)), each
// workgroup staging its window once.
std::vector<dev::WaveStart> plan_waves(const Config& c, const int64_t* offsets, const int32_t* long_recs,
                                       int64_t n_long, int part, int parts, TilePlan& tp) {
  std::vector<dev::WaveStart> starts;
  tp = TilePlan{};
  if (n_long <= 0) return starts;
  int64_t sum_l2 = 0, max_l2 = 0;
  for (int64_t li = 0; li < n_long; ++li) {
    const int64_t L2 = long_length(offsets, long_recs, li);
    sum_l2 += L2;
    max_l2 = std::max(max_l2, L2 <= c.L1 ? L2 : 0);
  }
  int64_t W = c.prof16_window;
  bool wide = c.prof16_wide && !c.mfma && W == 0;
  // a whole byte-pair image whose widened form does not fit (L1 ~ 1500..3050): short records take a widened
  // WINDOW instead (one packed add per lane and step; the window holds U = 4 tiles plus the longest record)
  if (W == 0 && c.has_prof16 && !c.prof16_wide && !c.mfma && c.tile16_window_wide && c.tile_u <= 0 &&
      max_l2 + 2 * 128 * 4 <= dev::tile16_max_window(true)) {
    W = dev::tile16_max_window(true);
    wide = true;
  }
  // records too long for a widened window on a Seq1 whose widened image exceeds the LDS — with the byte pairs
  // whole (limits: L1 3000, records up to 2000 letters), as windows (L1 past ~3050), or an int16 profile:
  // sliding widened windows (limits 12.9 -> 16.8 T cells/s, L1 20 000 with input3's records 17.3 -> 20.7,
  // L1 150 000 9.6 -> 15.9; profiles/tile16_r5/README.txt)
  if ((W == 0 || max_l2 + 2 * 128 * 4 > dev::tile16_max_window(true)) && !wide && c.has_prof16 && !c.mfma &&
      c.tile16_slide && parts == 1 && (c.tile_u <= 0 || c.tile_u == 2 || c.tile_u == 4 || c.tile_u == 8))
    if (plan_slide(c, offsets, long_recs, n_long, c.prof16_i16 ? 0.25 : 0.8, tp, starts)) return starts;
  tp.window = W;
  tp.wide = wide;
  tp.tile16 = c.has_prof16 && (W == 0 || max_l2 + 2 * 128 <= W) && (wide || !c.prof16_i16);
  // sub-tiles per wave tile: batch_u — unless the batch gives every resident wave >= 8 tiles of 4 sub-tiles:
  // with a record's last tile cut to its valid sub-tiles (tile16_search_kernel) 4 then wins on long records
  // too (input3: 17.2 -> 17.7 T cells/s; 4 tiles per wave, heavy3's bench batch, stays on 2: 14.8 vs 14.3;
  // profiles/r6/README.txt)
  int u = batch_u(c, sum_l2, n_long);
  if (c.tile_u <= 0 && u == 2 && W == 0 && tp.tile16) {
    int64_t tiles4 = 0;
    for (int64_t li = 0; li < n_long; ++li)
      tiles4 += dev::tiles_of(dev::lanes_needed(c.L1, long_length(offsets, long_recs, li)), dev::tile_span(true, 4));
    const int64_t lds = dev::tile16_lds_bytes((wide ? 2 : 1) * static_cast<int64_t>(c.prof16_bytes), c.L1);
    const int64_t resident = static_cast<int64_t>(c.num_cus) * dev::tile16_waves_per_cu(static_cast<int>(lds));
    if (tiles4 >= 8 * resident * parts) u = 4;
  }
  if (c.tile_u <= 0 && u == 4 && tp.tile16 && W == 0 && 128 * 8 <= c.prof16_overhang) u = 8;  // tile16: wider tiles
  if (u > 4 && !(tp.tile16 && W == 0 && 128 * u <= c.prof16_overhang)) u = 4;  // the overhang bounds the span
  if (u > 2 && c.mfma && tp.tile16 && W == 0) u = 2;  // the matrix-core sweep's register budget (U = 4 spills)
  if (tp.tile16 && W > 0) {
    // windowed: the widest tiles a window holds twice (L1 = 20 000, input3 records: U = 4 -> 9.3 T cells/s,
    // U = 2 -> 8.4, U = 1 -> 7.0; profiles/kernel_bench_long.log)
    if (c.tile_u <= 0) u = 4;
    while (u > 1 && max_l2 + 2 * 128 * u > W) u /= 2;
    // widened windows (short records): 8 sub-tiles when one tile and the longest record fit the window
    if (wide && c.tile_u <= 0 && c.short_window_u8 && max_l2 + 128 * 8 <= W) u = 8;
  }
  tp.u = u;
  const int span = dev::tile_span(tp.tile16, u);
  std::vector<int64_t> tcost;
  std::vector<int32_t> ntiles;
  const int64_t total_tiles = tile_costs(c, offsets, long_recs, n_long, span, ntiles, tcost);
  const int s1_len = tp.tile16 && W > 0 ? static_cast<int>(W) : static_cast<int>(c.L1);
  const int64_t prof_lds = (wide ? 2 : 1) * (W ? dev::tile16_window_bytes(W) : static_cast<int64_t>(c.prof16_bytes));
  const int waves_per_cu = tp.tile16 ? dev::tile16_waves_per_cu(static_cast<int>(dev::tile16_lds_bytes(prof_lds, s1_len)))
                                     : c.tile_waves_per_cu;
  if (!(tp.tile16 && W > 0))
    return balanced_runs(ntiles, tcost, total_tiles, part, parts, static_cast<int64_t>(c.num_cus) * waves_per_cu);
  // ---- windowed tile16: window-major runs, whole workgroups per window
  // (a widened window, chosen for short records only, packs one more tile: its columns
  // [0, T * span + max L2) still lie inside the window)
  const int64_t T = std::max<int64_t>(1, (W - (wide ? 0 : span) - max_l2) / span);
  tp.win_tiles = static_cast<int32_t>(T);
  int32_t max_nt = 0;
  for (int64_t li = 0; li < n_long; ++li) max_nt = std::max(max_nt, ntiles[li]);
  const int64_t M = (max_nt + T - 1) / T;
  auto count = [&](int64_t li, int64_t m) { return std::clamp<int64_t>(ntiles[li] - m * T, 0, T); };
  std::vector<int64_t> wcost(static_cast<size_t>(M), 0);
  for (int64_t li = 0; li < n_long; ++li)
    for (int64_t m = 0; m * T < ntiles[li]; ++m) wcost[m] += count(li, m) * tcost[li];
  std::vector<int64_t> wstart(static_cast<size_t>(M) + 1, 0);
  for (int64_t m = 0; m < M; ++m) wstart[m + 1] = wstart[m] + wcost[m];
  const int64_t C = wstart[M];
  const int64_t lo = C * part / parts, hi = C * (part + 1) / parts;
  constexpr int kWg = dev::kTile16WavesPerBlock;
  const int64_t target_wgs = std::max<int64_t>(1, static_cast<int64_t>(c.num_cus) * waves_per_cu / kWg);
  // workgroups per window in proportion to its cost, largest remainders first, so that they add up to
  // target_wgs: one workgroup over the resident count waits for a second round (ceil per window put input4's
  // 3 windows at 3 x 86 = 258 on 256 CUs: 2.4 ms instead of 1.3)
  std::vector<int64_t> wgs_of(static_cast<size_t>(M), 0);
  {
    std::vector<std::pair<double, int64_t>> frac;
    int64_t used = 0;
    for (int64_t m = 0; m < M; ++m) {
      const int64_t a = std::max(lo, wstart[m]) - wstart[m], b = std::min(hi, wstart[m + 1]) - wstart[m];
      if (b <= a) continue;
      const double ideal = static_cast<double>(target_wgs) * static_cast<double>(b - a) /
                           static_cast<double>(std::max<int64_t>(hi - lo, 1));
      const int64_t share_tiles = std::max<int64_t>(1, (b - a) / std::max<int64_t>(1, C / std::max<int64_t>(total_tiles, 1)));
      const int64_t cap = std::max<int64_t>(1, (share_tiles + kWg - 2) / (kWg - 1));
      wgs_of[m] = std::clamp<int64_t>(static_cast<int64_t>(ideal), 1, cap);
      used += wgs_of[m];
      if (wgs_of[m] < cap) frac.emplace_back(ideal - static_cast<double>(wgs_of[m]), m);
    }
    std::sort(frac.begin(), frac.end(), [](const auto& x, const auto& y) { return x.first > y.first; });
    for (const auto& f : frac) {
      if (used >= target_wgs) break;
      ++wgs_of[f.second];
      ++used;
    }
  }
  std::vector<int64_t> pre(static_cast<size_t>(n_long) + 1);
  for (int64_t m = 0; m < M; ++m) {
    const int64_t a = std::max(lo, wstart[m]) - wstart[m], b = std::min(hi, wstart[m + 1]) - wstart[m];
    if (b <= a) continue;
    pre[0] = 0;
    for (int64_t li = 0; li < n_long; ++li) pre[li + 1] = pre[li] + count(li, m) * tcost[li];
    const dev::WaveStart end_marker{static_cast<int32_t>(n_long), static_cast<int32_t>(m * T)};
    auto at = [&](int64_t X) { return locate(pre, tcost, [&](int64_t li) { return count(li, m); }, X, m * T, end_marker); };
    const int64_t real = wgs_of[m] * kWg - 1;  // + one empty marker wave that ends the window's list
    for (int64_t q = 0; q < real; ++q) starts.push_back(at(a + (b - a) * q / real));
    // the last real wave ends at the share's end, and the marker wave [end, next window's first start) is
    // empty: its start is the end of this window
    starts.push_back(at(b));
  }
  if (starts.empty()) return starts;
  // every window contributed wgs*16 entries: the real waves' starts + its end; the final entry ends the list
  starts.push_back(starts.back());
  return starts;
}

// The LUT tile kernel's batch_u; MOC_TILE_U = 1 | 2 | 4 overrides (8 is tile16's: 4 here) — and never more
// sub-tiles than the batch's widest offset range fills (short records: one sub-tile)
int profile_u(const Config& c, int64_t sum_l2, int64_t n, int64_t max_need) {
  int u = std::min(batch_u(c, sum_l2, n), 4);
  if (c.tile_u <= 0)
    while (u > 1 && max_need <= dev::kTileOffsets * (u / 2)) u /= 2;
  return u;
}

std::vector<dev::WaveStart> profile_runs(const Config& c, const int64_t* offsets, int64_t n, int u) {
  std::vector<int32_t> ntiles;
  std::vector<int64_t> tcost;
  const int64_t total_tiles = tile_costs(c, offsets, nullptr, n, dev::tile_span(false, u), ntiles, tcost);
  return balanced_runs(ntiles, tcost, total_tiles, 0, 1, static_cast<int64_t>(c.num_cus) * c.tile_waves_per_cu);
}

ProfilePlan plan_profile(const Config& c, Semantics sem, const int64_t* offsets, int64_t n, bool chunked,
                         int64_t entry_bytes, int64_t scratch_bytes, int64_t radius, const int64_t* target_starts, int64_t T,
                         bool upload_targets, int targets_seg, int64_t record_bytes) {
  if (n >= (int64_t{1} << 31) - 1) throw Error("profile / top-K: more than 2^31 - 2 records in one call");
  int64_t min_target = INT64_MAX;  // the shortest and (pp.max_target) the longest target
  for (int64_t t = 0; target_starts && t < T; ++t) min_target = std::min(min_target, target_starts[t + 1] - target_starts[t]);
  const bool target_peaks = radius > 0 && target_starts && T > 0;  // the per-target distinct forms
  const bool spec = sem == Semantics::Spec;
  ProfilePlan pp;
  for (int64_t t = 0; target_starts && t < T; ++t) pp.max_target = std::max(pp.max_target, target_starts[t + 1] - target_starts[t]);
  pp.poff.resize(static_cast<size_t>(n) + 1);
  pp.poff[0] = 0;
  int64_t sum_l2 = 0, max_need = 1;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t L2 = offsets[i + 1] - offsets[i];
    pp.poff[i + 1] = pp.poff[i] + candidate_offsets(c.L1, L2, sem);
    sum_l2 += L2;
    pp.max_l2 = std::max(pp.max_l2, L2);
    max_need = std::max(max_need, dev::lanes_needed(c.L1, L2));
    pp.cells += record_cells(c.L1, L2);
  }
  if (c.L1 >= (int64_t{1} << 30) || pp.max_l2 >= (int64_t{1} << 30))
    throw Error("Seq1 / Seq2 lengths beyond 2^30 exceed the device engine's offset range");
  // sub-tiles per wave tile, as the LUT tile kernel picks them, narrowed to the batch's widest offset range
  pp.u = profile_u(c, sum_l2, n, max_need);
  const std::vector<int64_t>& poff = pp.poff;
  const int64_t cap_entries = std::max<int64_t>(1, scratch_bytes / entry_bytes);
  // records [r0, r1] fit one chunk: their entries alone (record_bytes == 0, the rule of every call without per-record
  // scratch), or their entries and record_bytes for each of them within scratch_bytes; in int64 for every batch the
  // checks above let through (entries < 2^61 / n, record_bytes a few KiB times n < 2^31)
  const auto fits = [&](int64_t r0, int64_t r1) {
    const int64_t entries = poff[r1 + 1] - poff[r0];
    if (record_bytes <= 0) return entries <= cap_entries;
    return entry_bytes * entries + record_bytes * (r1 + 1 - r0) <= scratch_bytes;
  };
  for (int64_t r0 = 0; r0 < n;) {
    int64_t r1 = r0 + 1;
    if (!chunked)
      r1 = n;
    else
      while (r1 < n && fits(r0, r1)) ++r1;
    ProfileChunk k;
    k.r0 = r0;
    k.r1 = r1;
    k.entries = poff[r1] - poff[r0];
    const std::vector<dev::WaveStart> runs = profile_runs(c, offsets + r0, r1 - r0, pp.u);
    k.starts_at = pp.starts.size();
    k.n_starts = runs.size();
    pp.starts.insert(pp.starts.end(), runs.begin(), runs.end());
    k.min_l2 = INT64_MAX;
    int64_t max_c = 0;  // the chunk's longest profile
    for (int64_t r = r0; r < r1; ++r) {
      const int64_t L2 = offsets[r + 1] - offsets[r], C = poff[r + 1] - poff[r];
      k.min_l2 = std::min(k.min_l2, L2);
      k.max_l2 = std::max(k.max_l2, L2);
      if (radius > 0 && !target_peaks && C >= 1 && C <= bounds::kPeaksWaveEntries) k.any_short = 1;
      max_c = std::max(max_c, C);
    }
    if (radius > 0 && !target_peaks && max_c > bounds::kPeaksWaveEntries) {
      k.max_tiles = static_cast<int32_t>((max_c + bounds::kPeaksTile - 1) / bounds::kPeaksTile);
      k.lds_keys = static_cast<int32_t>(std::min<int64_t>(bounds::kPeaksTile, max_c) + 2 * std::min<int64_t>(radius, max_c - 1));
    }
    if (target_peaks) {
      // the chunk's longest pair profile (its shortest record against the longest target) and a lower bound of its
      // shortest fitting one (its longest record against the shortest target)
      const int64_t hi = bounds::targets_pair_count(pp.max_target, std::max<int64_t>(k.min_l2, 1), spec);
      const int64_t lo = k.max_l2 <= min_target ? bounds::targets_pair_count(min_target, std::max<int64_t>(k.max_l2, 1), spec) : 0;
      k.t_seg = bounds::targets_peaks_seg_valid(targets_seg) ? targets_seg : bounds::targets_peaks_seg(hi);
      k.t_any_short = hi >= 2 && lo <= k.t_seg ? 1 : 0;
      if (hi > k.t_seg) {
        k.t_max_tiles = static_cast<int32_t>((hi + bounds::kPeaksTile - 1) / bounds::kPeaksTile);
        k.t_lds_keys = static_cast<int32_t>(std::min<int64_t>(bounds::kPeaksTile, hi) + 2 * std::min<int64_t>(radius, hi - 1));
      }
    }
    pp.max_entries = std::max(pp.max_entries, k.entries);
    pp.max_records = std::max(pp.max_records, r1 - r0);
    pp.chunks.push_back(k);
    r0 = r1;
  }
  pp.starts_off = sizeof(int64_t) * pp.poff.size();
  pp.targets_off = pp.starts_off + sizeof(dev::WaveStart) * pp.starts.size();  // 8-byte aligned: both parts are
  pp.bytes = pp.targets_off + (target_starts && upload_targets ? sizeof(int64_t) * (static_cast<size_t>(T) + 1) : 0);
  return pp;
}

ReportPlan plan_report(const int64_t* offsets, int64_t n, int K) {
  if (K < 1 || K > kMaxTopK) throw Error("report: K must be in 1.." + std::to_string(kMaxTopK));
  if (n >= (int64_t{1} << 31) - 1) throw Error("report: more than 2^31 - 2 records in one call");
  ReportPlan rp;
  rp.K = K;
  rp.rpw = dev::kWave / K;
  if (n <= 0) return rp;
  int64_t max_l2 = 0, min_l2 = 0;  // one pass over the lengths decides the common, all-short case
  const int nt = n > (1 << 16) ? omp_get_max_threads() : 1;
#pragma omp parallel for schedule(static) reduction(max : max_l2) reduction(min : min_l2) num_threads(nt) if (nt > 1)
  for (int64_t i = 0; i < n; ++i) {
    max_l2 = std::max(max_l2, offsets[i + 1] - offsets[i]);
    min_l2 = std::min(min_l2, offsets[i + 1] - offsets[i]);
  }
  if (min_l2 < 0) throw Error("report: record offsets must not decrease");
  if (max_l2 >= (int64_t{1} << 30)) throw Error("report: Seq2 lengths beyond 2^30 exceed the device engine's offset range");
  if (bounds::report_short_row(max_l2)) {
    rp.n_items = (n + rp.rpw - 1) / rp.rpw;
    return rp;
  }
  rp.implicit = false;
  rp.items.reserve(static_cast<size_t>(n / rp.rpw + 1));
  for (int64_t i = 0; i < n;) {
    if (!bounds::report_short_row(offsets[i + 1] - offsets[i])) {
      rp.long_recs.push_back(static_cast<int32_t>(i++));
      continue;
    }
    int64_t e = i + 1;
    while (e < n && e - i < rp.rpw && bounds::report_short_row(offsets[e + 1] - offsets[e])) ++e;
    rp.items.push_back(dev::ReportItem{static_cast<int32_t>(i), static_cast<int32_t>(e - i)});
    i = e;
  }
  rp.n_items = static_cast<int64_t>(rp.items.size());
  return rp;
}

}  // namespace plan
}  // namespace moc
