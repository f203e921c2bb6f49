// Stand-alone sanitizer check of the CPU engine's profile summary: built with -fsanitize=address,undefined together
// with the CPU core sources (make summary-san) and run as a plain program. summary_batch_cpu on small random problems
// against a literal letter-by-letter count written here; the summary and histogram sit in heap blocks of exactly
// n * 7 and n * bins elements, so a store past either is an ASan report. Also: the bin arithmetic at its int32 edges
// (lo = INT32_MIN with s = INT32_MAX, negative numerators, width = INT32_MAX) against a 128-bit-free restatement,
// the exactness bound at its edge, and the argument errors. Exit status 0 = all equal and no sanitizer report.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "moc/cpu_engine.hpp"

namespace {

using moc::ProfileEntry;
using moc::Semantics;

// every (offset, mutant) candidate re-scored from scratch; ties: k = 0 first, then the smallest k
std::vector<ProfileEntry> replay(const moc::ScoreTable& t, const std::vector<uint8_t>& s1, const std::vector<uint8_t>& s2,
                                 Semantics sem) {
  const int64_t L1 = static_cast<int64_t>(s1.size()), L2 = static_cast<int64_t>(s2.size());
  std::vector<ProfileEntry> prof;
  if (L2 > L1 || L2 <= 0) return prof;
  auto plain = [&](int64_t o) {
    int32_t s = 0;
    for (int64_t i = 0; i < L2; ++i) s += t.score(s2[i], s1[i + o]);
    return s;
  };
  if (L2 == L1) {
    prof.push_back(ProfileEntry{plain(0), 0});
    return prof;
  }
  for (int64_t o = 0; o < L1 - L2; ++o) {
    ProfileEntry best{plain(o), 0};
    for (int64_t m = 1; m < L2; ++m) {
      int32_t s = 0;
      for (int64_t i = 0; i < L2; ++i) s += t.score(s2[i], s1[i < m ? i + o : i + o + 1]);
      if (s > best.score) best = ProfileEntry{s, static_cast<int32_t>(m)};
    }
    prof.push_back(best);
  }
  if (sem == Semantics::Spec) prof.push_back(ProfileEntry{plain(L1 - L2), 0});
  return prof;
}

int failures = 0;
int64_t checked = 0;

void fail(const char* what, int problem, int sem, int threads, int bins, int32_t lo, int32_t width) {
  std::fprintf(stderr, "summary_san: %s (problem %d, semantics %d, threads %d, bins %d, lo %d, width %d)\n", what, problem,
               sem, threads, bins, lo, width);
  ++failures;
}

// the bin by repeated comparison with the bin edges lo + j * width, in int64: no division at all
int64_t bin_by_edges(int32_t s, int32_t lo, int32_t width, int32_t bins) {
  int64_t b = 0;
  while (b + 1 < bins && static_cast<int64_t>(lo) + (b + 1) * static_cast<int64_t>(width) <= s) ++b;
  return b;
}

uint32_t rng_state = 4242u;
uint32_t rnd(uint32_t m) {
  rng_state = rng_state * 1664525u + 1013904223u;
  return (rng_state >> 8) % m;
}

struct HistCase {
  int32_t bins, lo, width;
};

void run_problem(int id, const moc::Weights& w, int64_t L1, const std::vector<int64_t>& lens, int alphabet) {
  const moc::ScoreTable t = moc::ScoreTable::build(w);
  std::vector<uint8_t> s1(static_cast<size_t>(L1));
  for (uint8_t& c : s1) c = static_cast<uint8_t>(1 + rnd(static_cast<uint32_t>(alphabet)));
  std::vector<std::vector<uint8_t>> rc;
  moc::RecordBatch batch;
  for (int64_t l : lens) {
    std::vector<uint8_t> r(static_cast<size_t>(l));
    for (uint8_t& c : r) c = static_cast<uint8_t>(1 + rnd(static_cast<uint32_t>(alphabet)));
    rc.push_back(std::move(r));
  }
  for (const auto& r : rc) batch.push_back(r.data(), static_cast<int64_t>(r.size()));
  const int64_t n = batch.size();
  const HistCase cases[] = {{0, 0, 1},          {1, 0, 1},           {2, -3, 7},       {255, INT32_MIN, 1 << 24},
                            {256, -40, 1},      {256, INT32_MIN, 1}, {7, INT32_MAX, 1}, {5, -1000, INT32_MAX},
                            {16, INT32_MIN, INT32_MAX}};
  for (Semantics sem : {Semantics::Reference, Semantics::Spec}) {
    std::vector<std::vector<ProfileEntry>> prof;
    for (int64_t i = 0; i < n; ++i) prof.push_back(replay(t, s1, rc[i], sem));
    for (const HistCase& hc : cases)
      for (int threads : {1, 3}) {
        const size_t sn = static_cast<size_t>(n) * moc::kSummaryCols, hn = static_cast<size_t>(n) * static_cast<size_t>(hc.bins);
        std::unique_ptr<int64_t[]> summary(new int64_t[sn]);  // exactly n * 7
        std::unique_ptr<int32_t[]> hist(hn ? new int32_t[hn] : nullptr);  // exactly n * bins
        std::fill(summary.get(), summary.get() + sn, int64_t{-7});
        if (hn) std::fill(hist.get(), hist.get() + hn, -7);
        moc::summary_batch_cpu(t, s1.data(), L1, batch, summary.get(), hist.get(), hc.bins, hc.lo, hc.width, sem, threads);
        for (int64_t i = 0; i < n; ++i) {
          const auto& p = prof[i];
          int64_t want[moc::kSummaryCols] = {static_cast<int64_t>(p.size()), 0, 0, INT32_MAX, INT32_MIN, 0, 0};
          std::vector<int32_t> wh(static_cast<size_t>(hc.bins), 0);
          for (size_t o = 0; o < p.size(); ++o) {
            const int64_t s = p[o].score;
            want[1] += s;
            want[2] += s * s;
            want[3] = std::min<int64_t>(want[3], s);
            if (s > want[4]) {
              want[4] = s;
              want[5] = static_cast<int64_t>(o);
              want[6] = p[o].k;
            }
            if (hc.bins) ++wh[static_cast<size_t>(bin_by_edges(p[o].score, hc.lo, hc.width, hc.bins))];
          }
          if (!std::equal(want, want + moc::kSummaryCols, summary.get() + i * moc::kSummaryCols))
            fail("summary row differs", id, static_cast<int>(sem), threads, hc.bins, hc.lo, hc.width);
          if (hc.bins && !std::equal(wh.begin(), wh.end(), hist.get() + i * hc.bins))
            fail("histogram row differs", id, static_cast<int>(sem), threads, hc.bins, hc.lo, hc.width);
          ++checked;
        }
      }
  }
}

template <class F>
bool throws_summary(F&& f) {
  try {
    f();
  } catch (const moc::Error& e) {
    return std::string(e.what()).rfind("summary:", 0) == 0;
  }
  return false;
}

void check_bins_and_bound() {
  // bin arithmetic at the int32 edges: the difference s - lo does not fit int32, negative numerators round down
  const int32_t edge[] = {INT32_MIN, INT32_MIN + 1, -8, -7, -1, 0, 1, 6, 7, 8, INT32_MAX - 1, INT32_MAX};
  for (int32_t s : edge)
    for (int32_t lo : edge)
      for (int32_t width : {1, 7, INT32_MAX})
        for (int32_t bins : {1, 2, 255, 256}) {
          // bin_by_edges walks at most `bins` edges
          if (moc::summary_bin(s, lo, width, bins) != bin_by_edges(s, lo, width, bins))
            fail("summary_bin differs from the edge walk", -1, 0, 0, bins, lo, width);
          ++checked;
        }
  if (moc::summary_bin(INT32_MAX, INT32_MIN, 1, 256) != 255) fail("lo = INT32_MIN, s = INT32_MAX wrapped", -1, 0, 0, 256, INT32_MIN, 1);
  if (moc::summary_bin(INT32_MAX, INT32_MIN, INT32_MAX, 256) != 2) fail("(2^32 - 1) / (2^31 - 1) is 2", -1, 0, 0, 256, INT32_MIN, INT32_MAX);
  if (moc::summary_bin(-8, -1, 7, 4) != 0 || moc::summary_bin(-1, -8, 7, 4) != 1) fail("floor of a negative numerator", -1, 0, 0, 4, -1, 7);
  // the bound at its edge: W = 10^6, L2 = 500 -> M^2 = 2.5e17; 36 entries fit int64, 37 do not
  if (moc::bounds::summary_max_count(1000000, 500) != 36) fail("bound of W = 10^6, L2 = 500 is not 36", -2, 0, 0, 0, 0, 0);
  if (!moc::bounds::summary_exact(1000000, 500, 36) || moc::bounds::summary_exact(1000000, 500, 37))
    fail("summary_exact at 36 / 37", -2, 0, 0, 0, 0, 0);
  // M is capped at 2^31: M^2 = 2^62, one entry fits (2^62 <= 2^63 - 1), as do two minus nothing: floor = 1
  if (moc::bounds::summary_max_count(INT32_MAX, int64_t{1} << 40) != 1) fail("bound with M capped at 2^31 is not 1", -2, 0, 0, 0, 0, 0);
  if (moc::bounds::summary_max_count(1, 1) != INT64_MAX) fail("bound of M = 1", -2, 0, 0, 0, 0, 0);
  if (moc::bounds::summary_max_count(0, 0) != INT64_MAX) fail("bound of an all-zero table", -2, 0, 0, 0, 0, 0);
  // 36 scores of magnitude M really do fit: 36 * M^2 <= INT64_MAX without wrapping (checked in unsigned)
  const uint64_t m2 = 500000000ull * 500000000ull;
  if (36 * m2 > static_cast<uint64_t>(INT64_MAX) || 37 * m2 <= static_cast<uint64_t>(INT64_MAX))
    fail("36 / 37 times M^2 against 2^63 - 1", -2, 0, 0, 0, 0, 0);
  // argument errors name the feature and come before anything is written
  if (!throws_summary([] { moc::check_summary_args(10, 100, 10, -1, 1); })) fail("bins = -1 accepted", -3, 0, 0, -1, 0, 1);
  if (!throws_summary([] { moc::check_summary_args(10, 100, 10, 257, 1); })) fail("bins = 257 accepted", -3, 0, 0, 257, 0, 1);
  if (!throws_summary([] { moc::check_summary_args(10, 100, 10, 4, 0); })) fail("width = 0 accepted", -3, 0, 0, 4, 0, 0);
  if (!throws_summary([] { moc::check_summary_args(1000000, 500, 37, 0, 1); })) fail("C = 37 past the bound accepted", -3, 0, 0, 0, 0, 1);
  if (throws_summary([] { moc::check_summary_args(1000000, 500, 36, 256, 1); })) fail("C = 36 at the bound refused", -3, 0, 0, 256, 0, 1);
}

// the wide case end to end: W1 = 10^6 and one 500-letter record that matches Seq1 everywhere, 36 offsets
void check_wide() {
  moc::Weights w;
  w.w[0] = 1000000, w.w[1] = 3, w.w[2] = 2, w.w[3] = 1;
  const moc::ScoreTable t = moc::ScoreTable::build(w);
  const int64_t L2 = 500, C = 36, L1 = L2 + C;  // reference semantics: L1 - L2 offsets
  std::vector<uint8_t> s1(static_cast<size_t>(L1), uint8_t{1}), rec(static_cast<size_t>(L2), uint8_t{1});
  moc::RecordBatch batch;
  batch.push_back(rec.data(), L2);
  std::unique_ptr<int64_t[]> summary(new int64_t[moc::kSummaryCols]);
  moc::summary_batch_cpu(t, s1.data(), L1, batch, summary.get(), nullptr, 0, 0, 1, Semantics::Reference, 1);
  const int64_t s = 500000000;
  const int64_t want[moc::kSummaryCols] = {C, C * s, C * s * s, s, s, 0, 0};
  if (!std::equal(want, want + moc::kSummaryCols, summary.get())) fail("wide row differs", -4, 0, 1, 0, 0, 1);
  std::vector<uint8_t> s1b(static_cast<size_t>(L1 + 1), uint8_t{1});
  if (!throws_summary([&] {
        moc::summary_batch_cpu(t, s1b.data(), L1 + 1, batch, summary.get(), nullptr, 0, 0, 1, Semantics::Reference, 1);
      }))
    fail("C = 37 ran", -4, 0, 1, 0, 0, 1);
  ++checked;
}

}  // namespace

int main() {
  moc::Weights w;
  w.w[0] = 10, w.w[1] = 2, w.w[2] = 3, w.w[3] = 4;
  moc::Weights neg;  // mostly negative scores
  neg.w[0] = 1, neg.w[1] = 5, neg.w[2] = 5, neg.w[3] = 5;
  moc::Weights z;  // all-zero weights: every entry ties at 0
  int id = 0;
  run_problem(id++, w, 23, {23, 24, 1, 2, 22, 7, 11}, 26);
  run_problem(id++, neg, 17, {5, 1, 16, 17, 18, 3}, 3);
  run_problem(id++, z, 12, {1, 4, 11, 12, 13}, 26);
  run_problem(id++, w, 1, {1, 2}, 26);
  std::vector<int64_t> many;  // the parallel-over-records branch of the batch call
  for (int i = 0; i < 40; ++i) many.push_back(1 + i % 9);
  run_problem(id++, neg, 19, many, 4);
  run_problem(id++, w, 3000, {200, 5}, 26);  // one record at a time, its offset chunks in parallel
  check_bins_and_bound();
  check_wide();
  if (failures) {
    std::fprintf(stderr, "summary_san: %d mismatches\n", failures);
    return 1;
  }
  std::printf("summary_san ok (%lld checks)\n", static_cast<long long>(checked));
  return 0;
}
