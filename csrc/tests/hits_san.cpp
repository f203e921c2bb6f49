// Stand-alone sanitizer check of the CPU engine's threshold hits: built with -fsanitize=address,undefined together
// with the CPU core sources (make hits-san) and run as a plain program. hits_batch_cpu on small random problems
// against a literal letter-by-letter count written here, at every threshold edge (the whole profile, nothing, each
// record's best and one above it, an entry's own score and one above it) and with cap = 0 (null rows), 1,
// total - 1 and total rows in heap blocks of exactly cap rows, so a store at or past rows + cap is an ASan report.
// Exit status 0 = all equal and no sanitizer report.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "moc/cpu_engine.hpp"

namespace {

using moc::ProfileEntry;
using moc::Result;
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
int64_t checked_rows = 0;

void fail(const char* what, int problem, int sem, int threads, int edge, int64_t cap) {
  std::fprintf(stderr, "hits_san: %s (problem %d, semantics %d, threads %d, threshold edge %d, cap %lld)\n", what,
               problem, sem, threads, edge, static_cast<long long>(cap));
  ++failures;
}

uint32_t rng_state = 12345u;
uint32_t rnd(uint32_t m) {
  rng_state = rng_state * 1664525u + 1013904223u;
  return (rng_state >> 8) % m;
}

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
  for (Semantics sem : {Semantics::Reference, Semantics::Spec}) {
    std::vector<std::vector<ProfileEntry>> prof;
    int64_t profile_size = 0;
    for (int64_t i = 0; i < n; ++i) {
      prof.push_back(replay(t, s1, rc[i], sem));
      profile_size += static_cast<int64_t>(prof.back().size());
    }
    // threshold edges: 0..2 one scalar for the batch, 3.. one threshold per record
    constexpr int kEdges = 7;
    for (int edge = 0; edge < kEdges; ++edge) {
      int32_t scalar = 0;
      std::vector<int32_t> per(static_cast<size_t>(n), 0);
      for (int64_t i = 0; i < n; ++i) {
        const auto& p = prof[i];
        if (p.empty()) continue;  // no candidate offsets: no hits under any threshold
        int32_t best = INT32_MIN;
        for (const ProfileEntry& e : p) best = std::max(best, e.score);
        const int32_t mid = p[p.size() / 2].score;
        per[i] = edge == 3 ? best : edge == 4 ? best + 1 : edge == 5 ? mid : mid + 1;
      }
      if (edge == 0) scalar = INT32_MIN;
      if (edge == 1) scalar = INT32_MAX;
      if (edge == 2) scalar = prof[0].empty() ? 0 : prof[0][0].score;
      const int32_t* thr = edge >= 3 ? per.data() : nullptr;
      // the expected index and rows, counted entry by entry
      std::vector<int64_t> want_h(static_cast<size_t>(n) + 1, 0);
      std::vector<Result> want;
      for (int64_t i = 0; i < n; ++i) {
        const int32_t ti = thr ? thr[i] : scalar;
        for (size_t o = 0; o < prof[i].size(); ++o)
          if (prof[i][o].score >= ti) want.push_back(Result{prof[i][o].score, static_cast<int32_t>(o), prof[i][o].k});
        want_h[i + 1] = static_cast<int64_t>(want.size());
      }
      const int64_t total = want_h[n];
      if (edge == 0 && total != profile_size)
        fail("INT32_MIN does not select the whole profile", id, static_cast<int>(sem), 0, edge, 0);
      if (edge == 1 && total != 0) fail("INT32_MAX has hits", id, static_cast<int>(sem), 0, edge, 0);
      for (int threads : {1, 3})
        for (int64_t cap : {int64_t{0}, int64_t{1}, total - 1, total}) {
          if (cap < 0) continue;
          std::vector<int64_t> h(static_cast<size_t>(n) + 1, -7);
          std::unique_ptr<Result[]> rows(cap ? new Result[static_cast<size_t>(cap)] : nullptr);  // exactly cap rows
          for (int64_t j = 0; j < cap; ++j) rows[j] = Result{-1, -1, -1};
          moc::hits_batch_cpu(t, s1.data(), L1, batch, scalar, thr, h.data(), rows.get(), cap, sem, threads);
          if (h != want_h) fail("hoffsets differ", id, static_cast<int>(sem), threads, edge, cap);
          for (int64_t j = 0; j < cap; ++j) {
            const Result exp = j < total ? want[static_cast<size_t>(j)] : Result{-1, -1, -1};
            if (rows[j].score != exp.score || rows[j].n != exp.n || rows[j].k != exp.k) {
              fail("rows differ", id, static_cast<int>(sem), threads, edge, cap);
              break;
            }
            ++checked_rows;
          }
        }
    }
  }
}

}  // namespace

int main() {
  moc::Weights w;
  w.w[0] = 10, w.w[1] = 2, w.w[2] = 3, w.w[3] = 4;
  moc::Weights z;  // all-zero weights: every entry ties at 0
  int id = 0;
  // L2 == L1, L2 > L1, 1, 2, L1 - 1, mid lengths; a small alphabet makes equal scores across offsets
  run_problem(id++, w, 23, {23, 24, 1, 2, 22, 7, 11}, 26);
  run_problem(id++, w, 17, {5, 1, 16, 17, 18, 3}, 3);
  run_problem(id++, z, 12, {1, 4, 11, 12, 13}, 26);
  run_problem(id++, w, 1, {1, 2}, 26);
  // many records: the parallel-over-records branch of the batch call
  std::vector<int64_t> many;
  for (int i = 0; i < 40; ++i) many.push_back(1 + i % 9);
  run_problem(id++, w, 19, many, 4);
  // few records with enough cells for a second thread: one record at a time, its offset chunks in parallel
  run_problem(id++, w, 3000, {200, 5}, 26);
  if (failures) {
    std::fprintf(stderr, "hits_san: %d mismatches\n", failures);
    return 1;
  }
  std::printf("hits_san ok (%lld rows checked)\n", static_cast<long long>(checked_rows));
  return 0;
}
