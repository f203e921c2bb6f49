// Stand-alone sanitizer check of the CPU engine's multi-target search: built with -fsanitize=address,undefined together
// with the CPU core sources (make targets-san) and run as a plain program. targets_batch_cpu on small random
// catalogs against brute_force_record run once per target on that target alone (the letter-by-letter loops, which
// never see the catalog); the catalog, the starts and the rows sit in heap blocks of exactly L1, T + 1 and n * T
// elements, so a read past a target's end at the catalog's end or a store past the rows is an ASan report. Also:
// T = 1 against solve_batch_cpu, and check_targets' errors. Exit status 0 = all equal and no sanitizer report.
#include <cstdint>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "moc/cpu_engine.hpp"

namespace {

using moc::Result;
using moc::Semantics;

int failures = 0;
int64_t checked = 0;

uint32_t rng_state = 777u;
uint32_t rnd(uint32_t m) {
  rng_state = rng_state * 1664525u + 1013904223u;
  return (rng_state >> 8) % m;
}

bool same(const Result& a, const Result& b) { return a.score == b.score && a.n == b.n && a.k == b.k; }

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
  for (Semantics sem : {Semantics::Reference, Semantics::Spec})
    for (int threads : {1, 3}) {
      std::unique_ptr<Result[]> rows(new Result[static_cast<size_t>(n * T)]);
      moc::targets_batch_cpu(t, s1.get(), L1, batch, starts.get(), T, rows.get(), sem, threads);
      for (int64_t i = 0; i < n; ++i)
        for (int64_t q = 0; q < T; ++q) {
          // the target alone, in a heap block of exactly its length
          const int64_t len = starts[q + 1] - starts[q];
          std::unique_ptr<uint8_t[]> alone(new uint8_t[static_cast<size_t>(len)]);
          for (int64_t j = 0; j < len; ++j) alone[j] = s1[starts[q] + j];
          const Result want = moc::brute_force_record(t, alone.get(), len, batch.record(i), batch.length(i), sem);
          ++checked;
          if (!same(rows[i * T + q], want)) {
            std::fprintf(stderr, "targets_san: problem %d sem %d threads %d record %lld target %lld: (%d, %d, %d) != (%d, %d, %d)\n",
                         id, static_cast<int>(sem), threads, static_cast<long long>(i), static_cast<long long>(q),
                         rows[i * T + q].score, rows[i * T + q].n, rows[i * T + q].k, want.score, want.n, want.k);
            ++failures;
          }
        }
      if (T == 1) {
        std::unique_ptr<Result[]> solo(new Result[static_cast<size_t>(n)]);
        moc::solve_batch_cpu(t, s1.get(), L1, batch, solo.get(), sem, threads);
        for (int64_t i = 0; i < n; ++i) {
          ++checked;
          if (!same(rows[i], solo[i])) {
            std::fprintf(stderr, "targets_san: problem %d: T = 1 differs from solve_batch_cpu at record %lld\n", id,
                         static_cast<long long>(i));
            ++failures;
          }
        }
      }
    }
}

void expect_error(const char* what, const std::vector<int64_t>& starts, int64_t T, int64_t L1) {
  ++checked;
  try {
    moc::check_targets(starts.empty() ? nullptr : starts.data(), T, L1);
  } catch (const moc::Error& e) {
    if (std::string(e.what()).rfind("targets:", 0) == 0) return;
    std::fprintf(stderr, "targets_san: %s: message does not start with targets: (%s)\n", what, e.what());
    ++failures;
    return;
  }
  std::fprintf(stderr, "targets_san: %s: accepted\n", what);
  ++failures;
}

}  // namespace

int main() {
  const moc::Weights w1{4, 3, 2, 10}, w2{1, 1, 1, 1}, w3{7, 0, 5, 2};
  // target lengths around every record length: L2 - 1, L2, L2 + 1, L2 + 2, a single letter and a long one
  run_problem(0, w1, {5, 6, 7, 8, 1, 40}, {6, 1, 2, 7}, 4);
  run_problem(1, w2, {1}, {1, 2}, 2);
  run_problem(2, w3, {30}, {1, 5, 29, 30, 31}, 3);          // T = 1
  run_problem(3, w1, {3, 3, 3, 3, 3, 3, 3, 3, 3}, {3, 2, 4}, 1);  // one repeated letter: every row (., 0, 0)
  run_problem(4, w2, {64, 1, 65, 2, 63}, {1, 2, 63, 64, 65}, 26);
  for (int p = 5; p < 25; ++p) {
    std::vector<int64_t> tl, rl;
    const int T = 1 + static_cast<int>(rnd(7)), n = 1 + static_cast<int>(rnd(5));
    for (int q = 0; q < T; ++q) tl.push_back(1 + rnd(24));
    for (int i = 0; i < n; ++i) rl.push_back(1 + rnd(14));
    run_problem(p, p % 2 ? w1 : w3, tl, rl, 2 + static_cast<int>(rnd(4)));
  }
  expect_error("starts not from 0", {1, 4}, 1, 4);
  expect_error("starts not ending at L1", {0, 3}, 1, 4);
  expect_error("a repeated value", {0, 2, 2, 4}, 3, 4);
  expect_error("a falling value", {0, 3, 2, 4}, 3, 4);
  expect_error("T = 0", {0}, 0, 0);
  expect_error("no starts", {}, 1, 4);
  {
    std::vector<int64_t> many(static_cast<size_t>(moc::bounds::kTargetsMax) + 2);
    for (size_t j = 0; j < many.size(); ++j) many[j] = static_cast<int64_t>(j);
    expect_error("T > kTargetsMax", many, moc::bounds::kTargetsMax + 1, moc::bounds::kTargetsMax + 1);
    ++checked;
    try {
      moc::check_targets(many.data(), moc::bounds::kTargetsMax, moc::bounds::kTargetsMax);  // the largest T is fine
    } catch (const moc::Error& e) {
      std::fprintf(stderr, "targets_san: T = kTargetsMax refused: %s\n", e.what());
      ++failures;
    }
  }
  if (failures) {
    std::fprintf(stderr, "targets_san: %d failures\n", failures);
    return 1;
  }
  std::printf("targets_san ok: %lld checks\n", static_cast<long long>(checked));
  return 0;
}
