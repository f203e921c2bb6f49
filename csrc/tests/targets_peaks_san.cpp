// Stand-alone sanitizer check of the per-target distinct placements' host code: built with
// -fsanitize=address,undefined together with the CPU core sources (make targets-peaks-san) and run as a plain program.
// targets_topk_batch_cpu and targets_hits_batch_cpu with a radius on small random catalogs against topk_batch_cpu /
// hits_batch_cpu with the same radius run on every target ALONE — the target in a heap block of exactly its length, so
// the oracle never sees the catalog, a straddling entry or a neighbouring target. The catalog, the starts, the index
// and the rows sit in heap blocks of exactly L1, T + 1, n * T + 1 and cap elements (cap = 0, 1, total - 1 and total):
// the blocks' ends are the guard bytes, a read past a target's end at the catalog's end or a store at or past rows +
// cap is an ASan report. Then the planner's per-target peaks facts (plan::ProfileChunk t_*): bounds over seeded
// batches, hand cases at 64 / 65 entries and at the tile edge, and that every other field of a plan is the same with
// and without them. Exit status 0 = all equal and no sanitizer report.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "moc/cpu_engine.hpp"
#include "moc/kernel_bounds.hpp"
#include "moc/tile_plan.hpp"

namespace {

using moc::Result;
using moc::Semantics;

int failures = 0;
int64_t checked = 0;

#define EXPECT(cond)                                                                   \
  do {                                                                                 \
    ++checked;                                                                         \
    if (!(cond)) {                                                                     \
      std::fprintf(stderr, "targets_peaks_san: line %d: %s\n", __LINE__, #cond);       \
      ++failures;                                                                      \
    }                                                                                  \
  } while (0)

uint32_t rng_state = 777u;
uint32_t rnd(uint32_t m) {
  rng_state = rng_state * 1664525u + 1013904223u;
  return (rng_state >> 8) % m;
}

bool same(const Result& a, const Result& b) { return a.score == b.score && a.n == b.n && a.k == b.k; }

void run_problem(int id, const moc::Weights& w, const std::vector<int64_t>& target_lens, const std::vector<int64_t>& lens,
                 int alphabet, int K, int32_t min_score, int64_t radius) {
  const moc::ScoreTable t = moc::ScoreTable::build(w);
  const int64_t T = static_cast<int64_t>(target_lens.size());
  std::unique_ptr<int64_t[]> starts(new int64_t[static_cast<size_t>(T) + 1]);
  starts[0] = 0;
  for (int64_t q = 0; q < T; ++q) starts[q + 1] = starts[q] + target_lens[static_cast<size_t>(q)];
  const int64_t L1 = starts[T];
  std::unique_ptr<uint8_t[]> s1(new uint8_t[static_cast<size_t>(L1)]);
  for (int64_t j = 0; j < L1; ++j) s1[j] = static_cast<uint8_t>(1 + rnd(static_cast<uint32_t>(alphabet)));
  std::vector<std::vector<uint8_t>> rc;
  for (int64_t l : lens) {
    std::vector<uint8_t> r(static_cast<size_t>(l));
    for (uint8_t& c : r) c = static_cast<uint8_t>(1 + rnd(static_cast<uint32_t>(alphabet)));
    rc.push_back(std::move(r));
  }
  moc::RecordBatch batch;
  for (const auto& r : rc) batch.push_back(r.data(), static_cast<int64_t>(r.size()));
  const int64_t n = batch.size(), pairs = n * T;
  for (Semantics sem : {Semantics::Reference, Semantics::Spec})
    for (int threads : {1, 3}) {
      // the oracle: the single-Seq1 distinct calls on every target alone
      std::vector<std::vector<Result>> want_top(static_cast<size_t>(T)), want_hits(static_cast<size_t>(T));
      std::vector<std::vector<int64_t>> want_idx(static_cast<size_t>(T));
      for (int64_t q = 0; q < T; ++q) {
        const int64_t len = starts[q + 1] - starts[q];
        std::unique_ptr<uint8_t[]> alone(new uint8_t[static_cast<size_t>(len)]);
        for (int64_t j = 0; j < len; ++j) alone[j] = s1[starts[q] + j];
        want_top[static_cast<size_t>(q)].resize(static_cast<size_t>(n * K));
        moc::topk_batch_cpu(t, alone.get(), len, batch, K, want_top[static_cast<size_t>(q)].data(), sem, threads, radius);
        want_idx[static_cast<size_t>(q)].resize(static_cast<size_t>(n) + 1);
        moc::hits_batch_cpu(t, alone.get(), len, batch, min_score, nullptr, want_idx[static_cast<size_t>(q)].data(), nullptr, 0,
                            sem, threads, radius);
        const int64_t m = want_idx[static_cast<size_t>(q)][static_cast<size_t>(n)];
        want_hits[static_cast<size_t>(q)].resize(static_cast<size_t>(std::max<int64_t>(m, 1)));
        moc::hits_batch_cpu(t, alone.get(), len, batch, min_score, nullptr, want_idx[static_cast<size_t>(q)].data(),
                            want_hits[static_cast<size_t>(q)].data(), m, sem, threads, radius);
      }
      // top-K
      std::unique_ptr<Result[]> rows(new Result[static_cast<size_t>(pairs * K)]);
      moc::targets_topk_batch_cpu(t, s1.get(), L1, batch, starts.get(), T, K, rows.get(), sem, threads, radius);
      for (int64_t p = 0; p < pairs; ++p)
        for (int j = 0; j < K; ++j) {
          ++checked;
          const Result& want = want_top[static_cast<size_t>(p % T)][static_cast<size_t>((p / T) * K + j)];
          if (!same(rows[p * K + j], want)) {
            std::fprintf(stderr, "targets_peaks_san: top-K: problem %d sem %d R %lld pair %lld row %d: (%d, %d, %d) != (%d, %d, %d)\n",
                         id, static_cast<int>(sem), static_cast<long long>(radius), static_cast<long long>(p), j,
                         rows[p * K + j].score, rows[p * K + j].n, rows[p * K + j].k, want.score, want.n, want.k);
            ++failures;
          }
        }
      // hits: the flat expectation, then cap = 0, 1, total - 1 and total
      std::vector<Result> flat;
      std::vector<int64_t> want_off(static_cast<size_t>(pairs) + 1, 0);
      for (int64_t p = 0; p < pairs; ++p) {
        const size_t q = static_cast<size_t>(p % T), i = static_cast<size_t>(p / T);
        for (int64_t at = want_idx[q][i]; at < want_idx[q][i + 1]; ++at) flat.push_back(want_hits[q][static_cast<size_t>(at)]);
        want_off[static_cast<size_t>(p) + 1] = static_cast<int64_t>(flat.size());
      }
      const int64_t total = static_cast<int64_t>(flat.size());
      for (int64_t cap : {int64_t{0}, int64_t{1}, total - 1, total}) {
        if (cap < 0) continue;
        std::unique_ptr<int64_t[]> toffsets(new int64_t[static_cast<size_t>(pairs) + 1]);
        std::unique_ptr<Result[]> hits(cap ? new Result[static_cast<size_t>(cap)] : nullptr);
        moc::targets_hits_batch_cpu(t, s1.get(), L1, batch, starts.get(), T, min_score, nullptr, toffsets.get(), hits.get(), cap,
                                    sem, threads, radius);
        for (int64_t p = 0; p <= pairs; ++p) EXPECT(toffsets[p] == want_off[static_cast<size_t>(p)]);
        for (int64_t at = 0; at < std::min(cap, total); ++at) EXPECT(same(hits[at], flat[static_cast<size_t>(at)]));
      }
    }
}

template <class Fn>
void expect_error(const char* what, const char* prefix, Fn&& fn) {
  ++checked;
  try {
    fn();
  } catch (const moc::Error& e) {
    if (std::string(e.what()).rfind(prefix, 0) == 0) return;
    std::fprintf(stderr, "targets_peaks_san: %s: message does not start with %s (%s)\n", what, prefix, e.what());
    ++failures;
    return;
  }
  std::fprintf(stderr, "targets_peaks_san: %s: accepted\n", what);
  ++failures;
}

// ---- the planner's per-target peaks facts
std::vector<int64_t> offsets_of(const std::vector<int64_t>& lengths) {
  std::vector<int64_t> off{3};
  for (int64_t l : lengths) off.push_back(off.back() + l);
  return off;
}
std::vector<int64_t> starts_of(const std::vector<int64_t>& lengths) {
  std::vector<int64_t> s{0};
  for (int64_t l : lengths) s.push_back(s.back() + l);
  return s;
}
moc::plan::Config config_of(int64_t L1) {
  moc::plan::Config c;
  c.L1 = L1;
  return c;
}
moc::plan::ProfilePlan plan_of(const std::vector<int64_t>& tl, const std::vector<int64_t>& rl, Semantics sem, int64_t radius,
                               int64_t scratch, bool targets, int seg = 0) {
  const std::vector<int64_t> off = offsets_of(rl), st = starts_of(tl);
  return moc::plan::plan_profile(config_of(st.back()), sem, off.data(), static_cast<int64_t>(rl.size()), true, radius > 0 ? 9 : 8,
                                 scratch, radius, targets ? st.data() : nullptr, targets ? static_cast<int64_t>(tl.size()) : 0,
                                 targets, seg);
}

// every field that existed before the t_* facts
bool same_old_fields(const moc::plan::ProfilePlan& a, const moc::plan::ProfilePlan& b, bool peaks_too) {
  if (a.poff != b.poff || a.u != b.u || a.chunks.size() != b.chunks.size() || a.starts.size() != b.starts.size() ||
      a.max_entries != b.max_entries || a.max_records != b.max_records || a.max_l2 != b.max_l2 || a.cells != b.cells ||
      a.max_target != b.max_target || a.starts_off != b.starts_off || a.targets_off != b.targets_off || a.bytes != b.bytes)
    return false;
  for (size_t i = 0; i < a.chunks.size(); ++i) {
    const moc::plan::ProfileChunk &x = a.chunks[i], &y = b.chunks[i];
    if (x.r0 != y.r0 || x.r1 != y.r1 || x.starts_at != y.starts_at || x.n_starts != y.n_starts || x.entries != y.entries ||
        x.min_l2 != y.min_l2 || x.max_l2 != y.max_l2)
      return false;
    if (peaks_too && (x.any_short != y.any_short || x.max_tiles != y.max_tiles || x.lds_keys != y.lds_keys)) return false;
  }
  return true;
}

void check_planner() {
  namespace b = moc::bounds;
  const Semantics spec = Semantics::Spec, ref = Semantics::Reference;
  // hand cases, one record of 5 letters: under spec a target of 5 + C - 1 letters is a pair profile of C entries
  struct Hand {
    int64_t count, radius;
    int seg, any_short, max_tiles, lds_keys;
  };
  const Hand hands[] = {
      {1, 3, 4, 0, 0, 0},                                 // one entry: no mark, neither kernel
      {4, 3, 4, 1, 0, 0},    {5, 3, 8, 1, 0, 0},    {8, 3, 8, 1, 0, 0},     {9, 3, 16, 1, 0, 0},
      {16, 1, 16, 1, 0, 0},  {17, 1, 32, 1, 0, 0},  {32, 1, 32, 1, 0, 0},   {33, 1, 64, 1, 0, 0},
      {64, 2048, 64, 1, 0, 0},                            // the widest segment
      {65, 3, 64, 0, 1, 65 + 6},                          // one more: a tile, halo of 3 on each side
      {65, 2048, 64, 0, 1, 65 + 2 * 64},                  // the halo stops at C - 1
      {2048, 64, 64, 0, 1, 2048 + 128},                   // the tile edge
      {2049, 64, 64, 0, 2, 2048 + 128},  {4097, 2048, 64, 0, 3, 2048 + 4096},
  };
  for (const Hand& h : hands) {
    const moc::plan::ProfilePlan pp = plan_of({h.count == 1 ? 5 : 5 + h.count - 1}, {5}, spec, h.radius, 1 << 20, true);
    EXPECT(pp.chunks.size() == 1);
    const moc::plan::ProfileChunk& k = pp.chunks[0];
    EXPECT(k.t_seg == h.seg && k.t_any_short == h.any_short && k.t_max_tiles == h.max_tiles && k.t_lds_keys == h.lds_keys);
    EXPECT(k.any_short == 0 && k.max_tiles == 0 && k.lds_keys == 0);  // the plain pass never runs for such a call
    if (k.t_seg != h.seg || k.t_any_short != h.any_short || k.t_max_tiles != h.max_tiles || k.t_lds_keys != h.lds_keys)
      std::fprintf(stderr, "  hand case C = %lld R = %lld: seg %d any_short %d max_tiles %d lds_keys %d\n",
                   static_cast<long long>(h.count), static_cast<long long>(h.radius), k.t_seg, k.t_any_short, k.t_max_tiles,
                   k.t_lds_keys);
  }
  // a forced width: profiles past it go to the tile kernel
  {
    const moc::plan::ProfileChunk k = plan_of({5 + 63}, {5}, spec, 2, 1 << 20, true, 4).chunks[0];
    EXPECT(k.t_seg == 4 && k.t_any_short == 0 && k.t_max_tiles == 1 && k.t_lds_keys == 64 + 4);
    const moc::plan::ProfileChunk m = plan_of({5 + 63, 7}, {5}, spec, 2, 1 << 20, true, 4).chunks[0];
    EXPECT(m.t_seg == 4 && m.t_any_short == 1 && m.t_max_tiles == 1);
  }
  // seeded batches through small budgets: the facts bound every pair of every chunk
  for (int it = 0; it < 200; ++it) {
    std::vector<int64_t> tl, rl;
    const int T = 1 + static_cast<int>(rnd(5)), n = 1 + static_cast<int>(rnd(9));
    for (int q = 0; q < T; ++q) tl.push_back(1 + rnd(it % 4 == 0 ? 5000 : 90));
    for (int i = 0; i < n; ++i) rl.push_back(1 + rnd(40));
    const Semantics sem = it % 2 ? spec : ref;
    const int64_t radius = 1 + rnd(it % 3 == 0 ? 2048 : 9);
    static const int kForced[7] = {0, 0, 4, 8, 16, 32, 64};
    const int forced = kForced[rnd(7)];
    const moc::plan::ProfilePlan pp = plan_of(tl, rl, sem, radius, 9 * (1 + rnd(400)), true, forced);
    for (const moc::plan::ProfileChunk& k : pp.chunks) {
      EXPECT(b::targets_peaks_seg_valid(k.t_seg));
      EXPECT(!forced || k.t_seg == forced);
      EXPECT(k.t_lds_keys <= b::kPeaksTile + 2 * b::kPeaksMaxRadius);
      EXPECT(k.any_short == 0 && k.max_tiles == 0 && k.lds_keys == 0);
      for (int64_t r = k.r0; r < k.r1; ++r)
        for (int q = 0; q < T; ++q) {
          const int64_t C = b::targets_pair_count(tl[static_cast<size_t>(q)], rl[static_cast<size_t>(r)], sem == spec);
          if (C >= 2 && C <= k.t_seg) EXPECT(k.t_any_short == 1);
          if (C > k.t_seg) {
            EXPECT(k.t_max_tiles >= (C + b::kPeaksTile - 1) / b::kPeaksTile);
            EXPECT(k.t_lds_keys >= std::min<int64_t>(b::kPeaksTile, C) + 2 * std::min<int64_t>(radius, C - 1));
          }
          if (!forced) EXPECT(C <= k.t_seg || C > b::kPeaksWaveEntries);  // the host's own width takes every short profile
        }
    }
    // every field that existed before is what the same call without a radius, and without targets, plans
    const moc::plan::ProfilePlan plain = plan_of(tl, rl, sem, 0, 9 * 400, true), again = plan_of(tl, rl, sem, 0, 9 * 400, true, 16);
    EXPECT(same_old_fields(plain, again, true));
    for (const moc::plan::ProfileChunk& k : plain.chunks) EXPECT(k.t_seg == 0 && k.t_any_short == 0 && k.t_max_tiles == 0 && k.t_lds_keys == 0);
    const moc::plan::ProfilePlan with_r = plan_of(tl, rl, sem, radius, 9 * 400, true), without_t = plan_of(tl, rl, sem, radius, 9 * 400, false, 4);
    // 9-byte entries in both: the same chunks; the radius alone changes no field that existed
    const std::vector<int64_t> off = offsets_of(rl), st = starts_of(tl);
    const moc::plan::ProfilePlan nine = moc::plan::plan_profile(config_of(st.back()), sem, off.data(), n, true, 9, 9 * 400, 0,
                                                                st.data(), T, true);
    EXPECT(same_old_fields(with_r, nine, false));
    for (const moc::plan::ProfileChunk& k : without_t.chunks) EXPECT(k.t_seg == 0 && k.t_any_short == 0 && k.t_max_tiles == 0 && k.t_lds_keys == 0);
  }
}

}  // namespace

int main() {
  const moc::Weights w1{4, 3, 2, 10}, w2{1, 1, 1, 1}, w3{7, 0, 5, 2};
  int id = 0;
  for (int64_t radius : {int64_t{1}, int64_t{2}, int64_t{3}, int64_t{40}, int64_t{2048}}) {
    run_problem(id++, w1, {5, 6, 7, 8, 1, 40}, {6, 1, 2, 7}, 4, 3, -8, radius);      // L2 - 1, L2, L2 + 1, L2 + 2 around the records
    run_problem(id++, w3, {30}, {1, 5, 29, 30, 31}, 3, 64, 0, radius);               // T = 1
    run_problem(id++, w1, {3, 3, 3, 9, 3}, {3, 2, 4}, 1, 5, 8, radius);              // one repeated letter: every entry ties
    run_problem(id++, w2, {64, 1, 65, 2, 63}, {1, 2, 63, 64, 65}, 26, 2, INT32_MIN, radius);
    for (int p = 0; p < 12; ++p) {
      std::vector<int64_t> tl, rl;
      static const int kT[3] = {1, 2, 5};
      const int T = kT[rnd(3)], n = 1 + static_cast<int>(rnd(5));
      for (int q = 0; q < T; ++q) tl.push_back(1 + rnd(30));
      for (int i = 0; i < n; ++i) rl.push_back(1 + rnd(14));
      rl[0] = tl.back();  // len == L2 at the catalog's end
      run_problem(id++, p % 2 ? w1 : w3, tl, rl, 2 + static_cast<int>(rnd(4)), 1 + static_cast<int>(rnd(6)),
                  static_cast<int32_t>(rnd(30)) - 15, radius);
    }
  }
  {
    const moc::ScoreTable t = moc::ScoreTable::build(w1);
    const uint8_t s1[4] = {1, 2, 1, 2}, rec[2] = {1, 2};
    moc::RecordBatch batch;
    batch.push_back(rec, 2);
    const int64_t good[2] = {0, 4}, bad[2] = {1, 4};
    Result rows[64];
    int64_t toffsets[2];
    expect_error("top-K: bad starts before the radius", "targets:",
                 [&] { moc::targets_topk_batch_cpu(t, s1, 4, batch, bad, 1, 1, rows, Semantics::Spec, 1, -1); });
    expect_error("top-K: K before the radius", "top-K:",
                 [&] { moc::targets_topk_batch_cpu(t, s1, 4, batch, good, 1, 0, rows, Semantics::Spec, 1, -1); });
    expect_error("top-K: radius -1", "distinct:",
                 [&] { moc::targets_topk_batch_cpu(t, s1, 4, batch, good, 1, 1, rows, Semantics::Spec, 1, -1); });
    expect_error("top-K: radius 2049", "distinct:",
                 [&] { moc::targets_topk_batch_cpu(t, s1, 4, batch, good, 1, 1, rows, Semantics::Spec, 1, 2049); });
    expect_error("hits: cap before the radius", "hits:", [&] {
      moc::targets_hits_batch_cpu(t, s1, 4, batch, good, 1, 0, nullptr, toffsets, nullptr, 3, Semantics::Spec, 1, -1);
    });
    expect_error("hits: radius 2049", "distinct:", [&] {
      moc::targets_hits_batch_cpu(t, s1, 4, batch, good, 1, 0, nullptr, toffsets, nullptr, 0, Semantics::Spec, 1, 2049);
    });
  }
  check_planner();
  if (failures) {
    std::fprintf(stderr, "targets_peaks_san: %d failures\n", failures);
    return 1;
  }
  std::printf("targets_peaks_san ok: %lld checks\n", static_cast<long long>(checked));
  return 0;
}
