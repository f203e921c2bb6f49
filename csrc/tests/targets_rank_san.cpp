// Stand-alone sanitizer check of the target ranking's host code: built with -fsanitize=address,undefined together
// with the CPU core sources (make targets-rank-san) and run as a plain program.
//  * targets_rank_batch_cpu on small random catalogs against a letter-by-letter replay of every target alone (every
//    candidate (o, k) summed from the table, the target in a heap block of exactly its length), its best rows stably
//    sorted by score. The catalog, the starts and the rank rows sit in heap blocks of exactly L1, T + 1 and n * M
//    elements, so a read past the catalog or a store past the rows is an ASan report. M = 1, F - 1, F, F + 1 and 64.
//  * plan_profile's record_bytes: 0 gives the plan of a call without it, field for field; with it every chunk but a
//    single over-budget record stays within scratch_bytes and no chunk could have taken one more record; the edges of
//    the cut (a budget exactly at two records' cost and one byte less, below 12 T, below one record's entries).
//  * the order of the errors: the target set's first, then M's.
// Exit status 0 = all equal and no sanitizer report.
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

using moc::RankRow;
using moc::Result;
using moc::Semantics;

int failures = 0;
int64_t checked = 0;

#define EXPECT(cond)                                                                 \
  do {                                                                               \
    ++checked;                                                                       \
    if (!(cond)) {                                                                   \
      std::fprintf(stderr, "targets_rank_san: line %d: %s\n", __LINE__, #cond);      \
      ++failures;                                                                    \
    }                                                                                \
  } while (0)

uint32_t rng_state = 977u;
uint32_t rnd(uint32_t m) {
  rng_state = rng_state * 1664525u + 1013904223u;
  return (rng_state >> 8) % m;
}

// The best row of a record against one target alone, letter by letter: every offset o, k = 0 and, where mutated
// candidates exist (o < len - L2), k = 1 .. L2 - 1; higher score, then smaller o, then smaller k.
bool replay_best(const moc::ScoreTable& t, const uint8_t* s1, int64_t len, const uint8_t* s2, int64_t L2, Semantics sem,
                 Result& best) {
  if (L2 < 1 || L2 > len) return false;
  const int64_t C = L2 == len ? 1 : len - L2 + (sem == Semantics::Spec ? 1 : 0);
  bool have = false;
  for (int64_t o = 0; o < C; ++o) {
    const int64_t kmax = o < len - L2 ? L2 - 1 : 0;
    for (int64_t k = 0; k <= kmax; ++k) {
      int32_t s = 0;
      for (int64_t i = 0; i < L2; ++i) s += t.lut[s2[i] * moc::kLutStride + s1[(i < k || k == 0) ? o + i : o + i + 1]];
      if (!have || s > best.score) {
        best = Result{s, static_cast<int32_t>(o), static_cast<int32_t>(k)};
        have = true;
      }
    }
  }
  return true;
}

void run_problem(int id, const moc::Weights& w, const std::vector<int64_t>& target_lens, const std::vector<int64_t>& lens,
                 int alphabet) {
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
  const int64_t n = batch.size();
  for (Semantics sem : {Semantics::Reference, Semantics::Spec}) {
    // the expected ranking of every record: the replay of every target alone, stably sorted by score
    std::vector<std::vector<RankRow>> want(static_cast<size_t>(n));
    int64_t max_f = 0;
    for (int64_t i = 0; i < n; ++i) {
      for (int64_t q = 0; q < T; ++q) {
        const int64_t len = starts[q + 1] - starts[q];
        std::unique_ptr<uint8_t[]> alone(new uint8_t[static_cast<size_t>(len)]);
        for (int64_t j = 0; j < len; ++j) alone[j] = s1[starts[q] + j];
        Result b{};
        if (replay_best(t, alone.get(), len, batch.record(i), batch.length(i), sem, b))
          want[static_cast<size_t>(i)].push_back(RankRow{static_cast<int32_t>(q), b.score, b.n, b.k});
      }
      std::stable_sort(want[static_cast<size_t>(i)].begin(), want[static_cast<size_t>(i)].end(),
                       [](const RankRow& a, const RankRow& b) { return a.score > b.score; });
      max_f = std::max<int64_t>(max_f, static_cast<int64_t>(want[static_cast<size_t>(i)].size()));
    }
    std::vector<int> ms{1, 64};
    for (int64_t m : {max_f - 1, max_f, max_f + 1})
      if (m >= 1 && m <= moc::kMaxTopK) ms.push_back(static_cast<int>(m));
    for (int M : ms)
      for (int threads : {1, 3}) {
        std::unique_ptr<RankRow[]> rows(new RankRow[static_cast<size_t>(std::max<int64_t>(n * M, 1))]);
        moc::targets_rank_batch_cpu(t, s1.get(), L1, batch, starts.get(), T, M, rows.get(), sem, threads);
        for (int64_t i = 0; i < n; ++i)
          for (int j = 0; j < M; ++j) {
            const std::vector<RankRow>& wi = want[static_cast<size_t>(i)];
            const RankRow e = static_cast<size_t>(j) < wi.size() ? wi[static_cast<size_t>(j)] : moc::no_rank();
            const RankRow g = rows[i * M + j];
            ++checked;
            if (g.target != e.target || g.score != e.score || g.n != e.n || g.k != e.k) {
              std::fprintf(stderr, "targets_rank_san: problem %d sem %d M %d record %lld row %d: (%d, %d, %d, %d) != (%d, %d, %d, %d)\n",
                           id, static_cast<int>(sem), M, static_cast<long long>(i), j, g.target, g.score, g.n, g.k, e.target,
                           e.score, e.n, e.k);
              ++failures;
            }
          }
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
    std::fprintf(stderr, "targets_rank_san: %s: message does not start with %s (%s)\n", what, prefix, e.what());
    ++failures;
    return;
  }
  std::fprintf(stderr, "targets_rank_san: %s: accepted\n", what);
  ++failures;
}

// ---- the planner's record_bytes
std::vector<int64_t> offsets_of(const std::vector<int64_t>& lengths) {
  std::vector<int64_t> off{5};
  for (int64_t l : lengths) off.push_back(off.back() + l);
  return off;
}
moc::plan::ProfilePlan plan_of(int64_t L1, const std::vector<int64_t>& rl, Semantics sem, int64_t scratch, int64_t record_bytes) {
  const std::vector<int64_t> off = offsets_of(rl);
  moc::plan::Config c;
  c.L1 = L1;
  return moc::plan::plan_profile(c, sem, off.data(), static_cast<int64_t>(rl.size()), true, 8, scratch, 0, nullptr, 0, false,
                                 0, record_bytes);
}
std::vector<int64_t> cut_of(const moc::plan::ProfilePlan& pp) {
  std::vector<int64_t> b{0};
  for (const moc::plan::ProfileChunk& k : pp.chunks) b.push_back(k.r1);
  return b;
}

void run_planner() {
  const Semantics ref = Semantics::Reference;
  // L1 = 30, records of 10 letters: 20 entries = 160 bytes each; T = 4: 48 bytes of pair rows each; 208 a record
  const std::vector<int64_t> four(4, 10);
  EXPECT(cut_of(plan_of(30, four, ref, 416, 48)) == (std::vector<int64_t>{0, 2, 4}));     // exactly two records
  EXPECT(cut_of(plan_of(30, four, ref, 415, 48)) == (std::vector<int64_t>{0, 1, 2, 3, 4}));  // one byte less
  EXPECT(cut_of(plan_of(30, four, ref, 40, 48)) == (std::vector<int64_t>{0, 1, 2, 3, 4}));   // below 12 T
  EXPECT(cut_of(plan_of(30, four, ref, 100, 48)) == (std::vector<int64_t>{0, 1, 2, 3, 4}));  // below one record's entries
  EXPECT(cut_of(plan_of(30, four, ref, 1 << 20, 48)) == (std::vector<int64_t>{0, 4}));
  EXPECT(cut_of(plan_of(30, four, ref, 416, 0)) == (std::vector<int64_t>{0, 2, 4}));        // 52 entries: two records
  EXPECT(cut_of(plan_of(30, four, ref, 4, 0)) == (std::vector<int64_t>{0, 1, 2, 3, 4}));    // the old rule's one entry
  // records longer than Seq1 have no entries: only their pair rows count
  EXPECT(cut_of(plan_of(8, std::vector<int64_t>(5, 10), ref, 96, 48)) == (std::vector<int64_t>{0, 2, 4, 5}));
  for (int round = 0; round < 300; ++round) {
    const int64_t L1 = 1 + rnd(60);
    std::vector<int64_t> rl(1 + rnd(40));
    for (int64_t& l : rl) l = rnd(8) == 0 ? L1 + rnd(3) : 1 + rnd(static_cast<uint32_t>(std::min<int64_t>(L1, 30)));
    const Semantics sem = rnd(2) ? Semantics::Spec : Semantics::Reference;
    const int64_t scratch = 8 + rnd(6000), record_bytes = 12 * (1 + rnd(40));
    // record_bytes = 0 is the plan of a call that never heard of it, field for field
    const std::vector<int64_t> off = offsets_of(rl);
    moc::plan::Config c;
    c.L1 = L1;
    const int64_t n = static_cast<int64_t>(rl.size());
    const moc::plan::ProfilePlan old = moc::plan::plan_profile(c, sem, off.data(), n, true, 8, scratch, 0);
    const moc::plan::ProfilePlan zero = plan_of(L1, rl, sem, scratch, 0);
    EXPECT(cut_of(old) == cut_of(zero) && old.poff == zero.poff && old.u == zero.u && old.starts.size() == zero.starts.size() &&
           old.max_entries == zero.max_entries && old.max_records == zero.max_records && old.bytes == zero.bytes);
    const int64_t cap = std::max<int64_t>(1, scratch / 8);
    for (const moc::plan::ProfileChunk& k : old.chunks) {
      EXPECT(k.r1 - k.r0 == 1 || k.entries <= cap);
      EXPECT(k.r1 == n || old.poff[static_cast<size_t>(k.r1) + 1] - old.poff[static_cast<size_t>(k.r0)] > cap);
    }
    // with it: within the budget unless a single record, and maximal
    const moc::plan::ProfilePlan pp = plan_of(L1, rl, sem, scratch, record_bytes);
    int64_t at = 0;
    for (const moc::plan::ProfileChunk& k : pp.chunks) {
      EXPECT(k.r0 == at && k.r1 > k.r0);
      at = k.r1;
      EXPECT(k.entries == pp.poff[static_cast<size_t>(k.r1)] - pp.poff[static_cast<size_t>(k.r0)]);
      EXPECT(k.r1 - k.r0 == 1 || 8 * k.entries + record_bytes * (k.r1 - k.r0) <= scratch);
      if (k.r1 < n)
        EXPECT(8 * (pp.poff[static_cast<size_t>(k.r1) + 1] - pp.poff[static_cast<size_t>(k.r0)]) + record_bytes * (k.r1 + 1 - k.r0) > scratch);
    }
    EXPECT(at == n);
  }
}

}  // namespace

int main() {
  const moc::Weights w{4, 3, 2, 10};
  int id = 0;
  run_problem(id++, w, {9}, {3, 9, 10, 1}, 4);                          // T = 1
  run_problem(id++, w, {5, 5, 5, 5, 5, 5}, {2, 5, 6}, 1);               // identical targets: equal scores, t ascending
  run_problem(id++, w, {1, 2, 3, 4, 5, 6, 7, 8}, {1, 4, 8, 9}, 3);      // F = T, some, 1 and 0
  for (int round = 0; round < 12; ++round) {
    std::vector<int64_t> tl(1 + rnd(70)), rl(1 + rnd(6));
    for (int64_t& l : tl) l = 1 + rnd(12);
    for (int64_t& l : rl) l = 1 + rnd(13);
    run_problem(id++, moc::Weights{static_cast<int32_t>(1 + rnd(9)), static_cast<int32_t>(rnd(5)), static_cast<int32_t>(rnd(5)),
                                   static_cast<int32_t>(rnd(12))},
                tl, rl, 2 + static_cast<int>(rnd(3)));
  }
  run_planner();
  {  // the order of the errors
    const moc::ScoreTable t = moc::ScoreTable::build(w);
    const uint8_t s1[4] = {1, 2, 1, 2}, rec[2] = {1, 2};
    moc::RecordBatch batch;
    batch.push_back(rec, 2);
    const int64_t good[3] = {0, 2, 4}, bad[3] = {0, 2, 5};
    RankRow rows[64];
    for (int M : {0, 65, -1}) {
      expect_error("M out of range", "rank:", [&] { moc::targets_rank_batch_cpu(t, s1, 4, batch, good, 2, M, rows, Semantics::Spec); });
      expect_error("bad starts before M", "targets:", [&] { moc::targets_rank_batch_cpu(t, s1, 4, batch, bad, 2, M, rows, Semantics::Spec); });
    }
    expect_error("T = 0 before M", "targets:", [&] { moc::targets_rank_batch_cpu(t, s1, 4, batch, good, 0, 0, rows, Semantics::Spec); });
    moc::targets_rank_batch_cpu(t, s1, 4, batch, good, 2, 64, rows, Semantics::Spec);
    EXPECT(rows[0].target == 0 && rows[1].target == 1 && rows[2].target == -1 && rows[63].target == -1);
  }
  if (failures) {
    std::fprintf(stderr, "targets_rank_san: %d failures\n", failures);
    return 1;
  }
  std::printf("targets_rank_san ok: %lld checks\n", static_cast<long long>(checked));
  return 0;
}
