// Stand-alone sanitizer check of the CPU engine's per-target profile summary: built with -fsanitize=address,undefined
// together with the CPU core sources (make targets-summary-san) and run as a plain program.
// targets_summary_batch_cpu on small random catalogs against a literal letter-by-letter replay written here and run
// once per target on that target alone (it never sees the catalog); the catalog, the starts, the summary and the
// histogram sit in heap blocks of exactly L1, T + 1, n * T * 7 and n * T * bins elements, so a read past a target's
// end at the catalog's end or a store past either output is an ASan report. Also: the exactness bound at its edge
// (36 entries at W = 10^6 and a 500-letter record), a catalog whose own profile is past the bound, and the argument
// and target-set errors. Exit status 0 = all equal and no sanitizer report.
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

// every (offset, mutant) candidate of s2 against s1[0 .. L1) re-scored from scratch; ties: k = 0 first, then the
// smallest k
std::vector<ProfileEntry> replay(const moc::ScoreTable& t, const uint8_t* s1, int64_t L1, const std::vector<uint8_t>& s2,
                                 Semantics sem) {
  const int64_t L2 = static_cast<int64_t>(s2.size());
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

void fail(const char* what, int problem, int sem, int threads, int bins, int64_t i, int64_t q) {
  std::fprintf(stderr, "targets_summary_san: %s (problem %d, semantics %d, threads %d, bins %d, record %lld, target %lld)\n",
               what, problem, sem, threads, bins, static_cast<long long>(i), static_cast<long long>(q));
  ++failures;
}

// the bin by repeated comparison with the bin edges lo + j * width, in int64: no division at all
int64_t bin_by_edges(int32_t s, int32_t lo, int32_t width, int32_t bins) {
  int64_t b = 0;
  while (b + 1 < bins && static_cast<int64_t>(lo) + (b + 1) * static_cast<int64_t>(width) <= s) ++b;
  return b;
}

uint32_t rng_state = 90210u;
uint32_t rnd(uint32_t m) {
  rng_state = rng_state * 1664525u + 1013904223u;
  return (rng_state >> 8) % m;
}

struct HistCase {
  int32_t bins, lo, width;
};

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
  const HistCase cases[] = {{0, 0, 1}, {1, 0, 1}, {5, -20, 9}, {256, -40, 1}, {16, INT32_MIN, INT32_MAX}, {7, INT32_MAX, 1}};
  for (Semantics sem : {Semantics::Reference, Semantics::Spec}) {
    // per pair: the replay of the record against the target alone, in a heap block of exactly its length
    std::vector<std::vector<ProfileEntry>> prof;
    for (int64_t i = 0; i < n; ++i)
      for (int64_t q = 0; q < T; ++q) {
        const int64_t len = starts[q + 1] - starts[q];
        std::unique_ptr<uint8_t[]> alone(new uint8_t[static_cast<size_t>(len)]);
        for (int64_t j = 0; j < len; ++j) alone[j] = s1[starts[q] + j];
        prof.push_back(replay(t, alone.get(), len, rc[static_cast<size_t>(i)], sem));
      }
    for (const HistCase& hc : cases)
      for (int threads : {1, 3}) {
        const size_t pairs = static_cast<size_t>(n * T);
        const size_t sn = pairs * moc::kSummaryCols, hn = pairs * static_cast<size_t>(hc.bins);
        std::unique_ptr<int64_t[]> summary(new int64_t[sn]);              // exactly n * T * 7
        std::unique_ptr<int32_t[]> hist(hn ? new int32_t[hn] : nullptr);  // exactly n * T * bins
        std::fill(summary.get(), summary.get() + sn, int64_t{-7});
        if (hn) std::fill(hist.get(), hist.get() + hn, -7);
        moc::targets_summary_batch_cpu(t, s1.get(), L1, batch, starts.get(), T, summary.get(), hist.get(), hc.bins, hc.lo,
                                       hc.width, sem, threads);
        for (int64_t i = 0; i < n; ++i)
          for (int64_t q = 0; q < T; ++q) {
            const auto& p = prof[static_cast<size_t>(i * T + q)];
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
            if (!std::equal(want, want + moc::kSummaryCols, summary.get() + (i * T + q) * moc::kSummaryCols))
              fail("summary row differs", id, static_cast<int>(sem), threads, hc.bins, i, q);
            if (hc.bins && !std::equal(wh.begin(), wh.end(), hist.get() + (i * T + q) * hc.bins))
              fail("histogram row differs", id, static_cast<int>(sem), threads, hc.bins, i, q);
            ++checked;
          }
      }
  }
}

// 0: accepted, 1: refused with a message that starts with `prefix`, 2: refused with another message
template <class F>
int refusal(F&& f, const char* prefix) {
  try {
    f();
  } catch (const moc::Error& e) {
    return std::string(e.what()).rfind(prefix, 0) == 0 ? 1 : 2;
  }
  return 0;
}

// weights (10^6, 3, 2, 1) and one 500-letter record: M^2 = 2.5e17, 36 entries fit int64 and 37 do not
void check_bound() {
  const moc::Weights w{1000000, 3, 2, 1};
  const moc::ScoreTable t = moc::ScoreTable::build(w);
  std::vector<uint8_t> rec(500);
  for (uint8_t& c : rec) c = static_cast<uint8_t>(1 + rnd(26));
  moc::RecordBatch batch;
  batch.push_back(rec.data(), 500);
  auto run = [&](const std::vector<int64_t>& target_lens, Semantics sem, int64_t* count_out) {
    const int64_t T = static_cast<int64_t>(target_lens.size());
    std::unique_ptr<int64_t[]> starts(new int64_t[static_cast<size_t>(T) + 1]);
    starts[0] = 0;
    for (int64_t q = 0; q < T; ++q) starts[q + 1] = starts[q] + target_lens[static_cast<size_t>(q)];
    const int64_t L1 = starts[T];
    std::unique_ptr<uint8_t[]> s1(new uint8_t[static_cast<size_t>(L1)]);
    for (int64_t j = 0; j < L1; ++j) s1[j] = static_cast<uint8_t>(1 + rnd(26));
    std::unique_ptr<int64_t[]> summary(new int64_t[static_cast<size_t>(T) * moc::kSummaryCols]);
    const int rc = refusal([&] {
      moc::targets_summary_batch_cpu(t, s1.get(), L1, batch, starts.get(), T, summary.get(), nullptr, 0, 0, 1, sem, 1);
    }, "summary:");
    if (rc == 0 && count_out) *count_out = summary[0];
    if (rc == 0) {  // the sums of an accepted call against 128-bit-free doubles: |sumsq| <= 36 * 2.5e17 < 2^63
      const auto p = replay(t, s1.get(), starts[1], rec, sem);
      int64_t sum = 0, sumsq = 0;
      for (const ProfileEntry& e : p) {
        sum += e.score;
        sumsq += static_cast<int64_t>(e.score) * e.score;
      }
      if (summary[1] != sum || summary[2] != sumsq) fail("bound: sums of the first target differ", -1, static_cast<int>(sem), 1, 0, 0, 0);
    }
    ++checked;
    return rc;
  };
  int64_t count = 0;
  if (moc::bounds::summary_max_count(1000000, 500) != 36) fail("bound of W = 10^6, L2 = 500 is not 36", -1, 0, 0, 0, 0, 0);
  if (run({536}, Semantics::Reference, &count) != 0 || count != 36) fail("bound: 36 entries refused", -1, 0, 1, 0, 0, 0);
  if (run({537}, Semantics::Reference, nullptr) != 1) fail("bound: 37 entries accepted", -1, 0, 1, 0, 0, 0);
  if (run({535}, Semantics::Spec, &count) != 0 || count != 36) fail("bound: 35 + 1 entries refused under spec", -1, 1, 1, 0, 0, 0);
  if (run({536}, Semantics::Spec, nullptr) != 1) fail("bound: 36 + 1 entries accepted under spec", -1, 1, 1, 0, 0, 0);
  // the catalog's own profile has 572 entries: summary_batch_cpu refuses it, every target's own is within the bound
  if (run({536, 536}, Semantics::Reference, &count) != 0 || count != 36) fail("bound: two 536-letter targets refused", -1, 0, 1, 0, 0, 0);
  if (run({536, 537}, Semantics::Reference, nullptr) != 1) fail("bound: a 537-letter second target accepted", -1, 0, 1, 0, 0, 0);
  if (run({100, 400}, Semantics::Reference, &count) != 0 || count != 0) fail("bound: a call without a fitting pair refused", -1, 0, 1, 0, 0, 0);
  const int64_t s2[] = {0, 536, 1072}, o2[] = {0, 500};
  if (moc::targets_max_count(s2, 2, o2, 1, Semantics::Reference) != 36 || moc::targets_max_count(s2, 2, o2, 1, Semantics::Spec) != 37)
    fail("targets_max_count of 536 against 500", -1, 0, 0, 0, 0, 0);
  const int64_t o3[] = {0, 536, 1136};  // records of 536 (equal lengths: one entry) and 600 letters (fits nothing)
  if (moc::targets_max_count(s2, 2, o3, 2, Semantics::Reference) != 1) fail("targets_max_count at equal lengths", -1, 0, 0, 0, 0, 0);
}

void check_errors() {
  const moc::ScoreTable t = moc::ScoreTable::build(moc::Weights{1, 1, 1, 1});
  const uint8_t s1[] = {1, 2, 3, 4, 5};
  const uint8_t rec[] = {1, 2};
  moc::RecordBatch batch;
  batch.push_back(rec, 2);
  int64_t summary[2 * moc::kSummaryCols];
  int32_t hist[2 * 4];
  const int64_t good[] = {0, 3, 5};
  auto call = [&](const int64_t* starts, int64_t T, int32_t* h, int32_t bins, int32_t width) {
    moc::targets_summary_batch_cpu(t, s1, 5, batch, starts, T, summary, h, bins, 0, width, Semantics::Reference, 1);
  };
  checked += 8;
  if (refusal([&] { call(good, 2, hist, 4, 1); }, "") != 0) fail("a valid call refused", -2, 0, 1, 4, 0, 0);
  if (refusal([&] { call(good, 2, hist, -1, 1); }, "summary:") != 1) fail("bins = -1 accepted", -2, 0, 1, -1, 0, 0);
  if (refusal([&] { call(good, 2, hist, 257, 1); }, "summary:") != 1) fail("bins = 257 accepted", -2, 0, 1, 257, 0, 0);
  if (refusal([&] { call(good, 2, hist, 4, 0); }, "summary:") != 1) fail("width = 0 accepted", -2, 0, 1, 4, 0, 0);
  if (refusal([&] { call(good, 2, nullptr, 4, 1); }, "summary:") != 1) fail("bins > 0 without a buffer accepted", -2, 0, 1, 4, 0, 0);
  const int64_t short_of[] = {0, 3, 4}, flat[] = {0, 3, 3};
  if (refusal([&] { call(short_of, 2, hist, 4, 1); }, "targets:") != 1) fail("starts short of L1 accepted", -2, 0, 1, 4, 0, 0);
  if (refusal([&] { call(flat, 2, hist, 4, 1); }, "targets:") != 1) fail("an empty target accepted", -2, 0, 1, 4, 0, 0);
  // the target set is checked first
  if (refusal([&] { call(flat, 2, hist, 257, 0); }, "targets:") != 1) fail("summary error before targets error", -2, 0, 1, 257, 0, 0);
}

}  // namespace

int main() {
  const moc::Weights w1{4, 3, 2, 10}, w2{1, 1, 1, 1}, w3{7, 0, 5, 2};
  // target lengths around every record length: L2 - 1, L2, L2 + 1, L2 + 2, a single letter and a long one
  run_problem(0, w1, {5, 6, 7, 8, 1, 40}, {6, 1, 2, 7}, 4);
  run_problem(1, w2, {1}, {1, 2}, 2);
  run_problem(2, w3, {30}, {1, 5, 29, 30, 31}, 3);               // T = 1
  run_problem(3, w1, {3, 3, 3, 3, 3, 3, 3, 3, 3}, {3, 2, 4}, 1);  // one repeated letter
  run_problem(4, w2, {64, 1, 65, 2, 63}, {1, 2, 63, 64, 65}, 26);
  for (int p = 5; p < 17; ++p) {
    std::vector<int64_t> tl, rl;
    const int T = 1 + static_cast<int>(rnd(7)), n = 1 + static_cast<int>(rnd(5));
    for (int q = 0; q < T; ++q) tl.push_back(1 + rnd(24));
    for (int i = 0; i < n; ++i) rl.push_back(1 + rnd(14));
    run_problem(p, p % 2 ? w1 : w3, tl, rl, 2 + static_cast<int>(rnd(4)));
  }
  check_bound();
  check_errors();
  if (failures) {
    std::fprintf(stderr, "targets_summary_san: %d failures\n", failures);
    return 1;
  }
  std::printf("targets_summary_san ok: %lld checks\n", static_cast<long long>(checked));
  return 0;
}
