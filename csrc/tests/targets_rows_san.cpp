// Stand-alone sanitizer check of the CPU engine's per-target top-K and threshold hits: built with
// -fsanitize=address,undefined together with the CPU core sources (make targets-rows-san) and run as a plain program.
// targets_topk_batch_cpu and targets_hits_batch_cpu on small random catalogs against a letter-by-letter replay of
// every target alone (every candidate (o, k) summed from the table, the target in a heap block of exactly its length,
// so the replay never sees the catalog). The catalog, the starts, the index and the rows sit in heap blocks of exactly
// L1, T + 1, n * T + 1 and cap elements — cap = 0, 1, total - 1 and total — so a read past a target's end at the
// catalog's end or a store at or past rows + cap is an ASan report. Exit status 0 = all equal and no sanitizer report.
#include <algorithm>
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

uint32_t rng_state = 4242u;
uint32_t rnd(uint32_t m) {
  rng_state = rng_state * 1664525u + 1013904223u;
  return (rng_state >> 8) % m;
}

bool same(const Result& a, const Result& b) { return a.score == b.score && a.n == b.n && a.k == b.k; }

// The profile of a record against one target alone, letter by letter: entry o = the best (score, k) over k = 0 and,
// where mutated candidates exist (o < len - L2), k = 1 .. L2 - 1; ties to the smallest k.
std::vector<Result> replay(const moc::ScoreTable& t, const uint8_t* s1, int64_t len, const uint8_t* s2, int64_t L2,
                           Semantics sem) {
  std::vector<Result> prof;
  if (L2 < 1 || L2 > len) return prof;
  const int64_t C = L2 == len ? 1 : len - L2 + (sem == Semantics::Spec ? 1 : 0);
  for (int64_t o = 0; o < C; ++o) {
    Result best{0, static_cast<int32_t>(o), 0};
    const int64_t kmax = o < len - L2 ? L2 - 1 : 0;
    for (int64_t k = 0; k <= kmax; ++k) {
      int32_t s = 0;
      for (int64_t i = 0; i < L2; ++i) s += t.lut[s2[i] * moc::kLutStride + s1[(i < k || k == 0) ? o + i : o + i + 1]];
      if (k == 0 || s > best.score) best = Result{s, static_cast<int32_t>(o), static_cast<int32_t>(k)};
    }
    prof.push_back(best);
  }
  return prof;
}

void fail(const char* what, int id, Semantics sem, int64_t i, int64_t q, int64_t j, const Result& got, const Result& want) {
  std::fprintf(stderr, "targets_rows_san: %s: problem %d sem %d record %lld target %lld row %lld: (%d, %d, %d) != (%d, %d, %d)\n",
               what, id, static_cast<int>(sem), static_cast<long long>(i), static_cast<long long>(q),
               static_cast<long long>(j), got.score, got.n, got.k, want.score, want.n, want.k);
  ++failures;
}

void run_problem(int id, const moc::Weights& w, const std::vector<int64_t>& target_lens, const std::vector<int64_t>& lens,
                 int alphabet, int K, int32_t min_score, bool per_pair) {
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
  std::unique_ptr<int32_t[]> thr(new int32_t[static_cast<size_t>(std::max<int64_t>(pairs, 1))]);
  for (int64_t p = 0; p < pairs; ++p)  // around min_score, clipped to int32
    thr[p] = static_cast<int32_t>(std::min<int64_t>(std::max<int64_t>(static_cast<int64_t>(min_score) + rnd(9) - 4, INT32_MIN), INT32_MAX));
  const int32_t* thresholds = per_pair ? thr.get() : nullptr;
  for (Semantics sem : {Semantics::Reference, Semantics::Spec})
    for (int threads : {1, 3}) {
      // the replay of every pair: the target alone, in a heap block of exactly its length
      std::vector<std::vector<Result>> profs(static_cast<size_t>(pairs));
      for (int64_t i = 0; i < n; ++i)
        for (int64_t q = 0; q < T; ++q) {
          const int64_t len = starts[q + 1] - starts[q];
          std::unique_ptr<uint8_t[]> alone(new uint8_t[static_cast<size_t>(len)]);
          for (int64_t j = 0; j < len; ++j) alone[j] = s1[starts[q] + j];
          profs[static_cast<size_t>(i * T + q)] = replay(t, alone.get(), len, batch.record(i), batch.length(i), sem);
        }
      // top-K
      std::unique_ptr<Result[]> rows(new Result[static_cast<size_t>(pairs * K)]);
      moc::targets_topk_batch_cpu(t, s1.get(), L1, batch, starts.get(), T, K, rows.get(), sem, threads);
      for (int64_t p = 0; p < pairs; ++p) {
        std::vector<Result> want = profs[static_cast<size_t>(p)];
        std::stable_sort(want.begin(), want.end(), [](const Result& a, const Result& b) { return a.score > b.score; });
        want.resize(static_cast<size_t>(K), moc::no_candidate());
        for (int j = 0; j < K; ++j) {
          ++checked;
          if (!same(rows[p * K + j], want[static_cast<size_t>(j)]))
            fail("top-K", id, sem, p / T, p % T, j, rows[p * K + j], want[static_cast<size_t>(j)]);
        }
      }
      // hits: the index from a counting call, then cap = 0, 1, total - 1 and total
      std::vector<Result> flat;
      std::vector<int64_t> want_off(static_cast<size_t>(pairs) + 1, 0);
      for (int64_t p = 0; p < pairs; ++p) {
        for (const Result& e : profs[static_cast<size_t>(p)])
          if (e.score >= (thresholds ? thresholds[p] : min_score)) flat.push_back(e);
        want_off[static_cast<size_t>(p) + 1] = static_cast<int64_t>(flat.size());
      }
      const int64_t total = static_cast<int64_t>(flat.size());
      for (int64_t cap : {int64_t{0}, int64_t{1}, total - 1, total}) {
        if (cap < 0) continue;
        std::unique_ptr<int64_t[]> toffsets(new int64_t[static_cast<size_t>(pairs) + 1]);
        std::unique_ptr<Result[]> hits(cap ? new Result[static_cast<size_t>(cap)] : nullptr);
        moc::targets_hits_batch_cpu(t, s1.get(), L1, batch, starts.get(), T, min_score, thresholds, toffsets.get(),
                                    hits.get(), cap, sem, threads);
        for (int64_t p = 0; p <= pairs; ++p) {
          ++checked;
          if (toffsets[p] != want_off[static_cast<size_t>(p)]) {
            std::fprintf(stderr, "targets_rows_san: hits: problem %d sem %d cap %lld: toffsets[%lld] = %lld != %lld\n", id,
                         static_cast<int>(sem), static_cast<long long>(cap), static_cast<long long>(p),
                         static_cast<long long>(toffsets[p]), static_cast<long long>(want_off[static_cast<size_t>(p)]));
            ++failures;
          }
        }
        for (int64_t at = 0; at < std::min(cap, total); ++at) {
          ++checked;
          if (!same(hits[at], flat[static_cast<size_t>(at)])) fail("hits", id, sem, -1, -1, at, hits[at], flat[static_cast<size_t>(at)]);
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
    std::fprintf(stderr, "targets_rows_san: %s: message does not start with %s (%s)\n", what, prefix, e.what());
    ++failures;
    return;
  }
  std::fprintf(stderr, "targets_rows_san: %s: accepted\n", what);
  ++failures;
}

}  // namespace

int main() {
  const moc::Weights w1{4, 3, 2, 10}, w2{1, 1, 1, 1}, w3{7, 0, 5, 2};
  // target lengths around every record length: L2 - 1, L2, L2 + 1, L2 + 2, a single letter and a long one
  run_problem(0, w1, {5, 6, 7, 8, 1, 40}, {6, 1, 2, 7}, 4, 3, -8, false);
  run_problem(1, w2, {1}, {1, 2}, 2, 1, INT32_MIN, false);
  run_problem(2, w3, {30}, {1, 5, 29, 30, 31}, 3, 64, 0, true);          // T = 1
  run_problem(3, w1, {3, 3, 3, 9, 3}, {3, 2, 4}, 1, 5, 8, false);        // one repeated letter: every entry ties
  run_problem(4, w2, {64, 1, 65, 2, 63}, {1, 2, 63, 64, 65}, 26, 2, INT32_MIN, false);
  run_problem(5, w1, {12, 9}, {4}, 3, 7, INT32_MAX, false);              // nothing reaches the threshold
  for (int p = 6; p < 26; ++p) {
    std::vector<int64_t> tl, rl;
    const int T = 1 + static_cast<int>(rnd(7)), n = 1 + static_cast<int>(rnd(5));
    for (int q = 0; q < T; ++q) tl.push_back(1 + rnd(24));
    for (int i = 0; i < n; ++i) rl.push_back(1 + rnd(14));
    run_problem(p, p % 2 ? w1 : w3, tl, rl, 2 + static_cast<int>(rnd(4)), 1 + static_cast<int>(rnd(6)),
                static_cast<int32_t>(rnd(30)) - 15, p % 3 == 0);
  }
  {
    const moc::ScoreTable t = moc::ScoreTable::build(w1);
    const uint8_t s1[4] = {1, 2, 1, 2}, rec[2] = {1, 2};
    moc::RecordBatch batch;
    batch.push_back(rec, 2);
    const int64_t good[2] = {0, 4}, bad[2] = {1, 4};
    Result rows[64];
    int64_t toffsets[2];
    expect_error("top-K: bad starts before K", "targets:",
                 [&] { moc::targets_topk_batch_cpu(t, s1, 4, batch, bad, 1, 0, rows, Semantics::Spec); });
    expect_error("top-K: K = 0", "top-K:", [&] { moc::targets_topk_batch_cpu(t, s1, 4, batch, good, 1, 0, rows, Semantics::Spec); });
    expect_error("top-K: K = 65", "top-K:", [&] { moc::targets_topk_batch_cpu(t, s1, 4, batch, good, 1, 65, rows, Semantics::Spec); });
    expect_error("hits: bad starts", "targets:",
                 [&] { moc::targets_hits_batch_cpu(t, s1, 4, batch, bad, 1, 0, nullptr, toffsets, nullptr, 0, Semantics::Spec); });
    expect_error("hits: cap without rows", "hits:",
                 [&] { moc::targets_hits_batch_cpu(t, s1, 4, batch, good, 1, 0, nullptr, toffsets, nullptr, 3, Semantics::Spec); });
    expect_error("hits: negative cap", "hits:",
                 [&] { moc::targets_hits_batch_cpu(t, s1, 4, batch, good, 1, 0, nullptr, toffsets, rows, -1, Semantics::Spec); });
  }
  if (failures) {
    std::fprintf(stderr, "targets_rows_san: %d failures\n", failures);
    return 1;
  }
  std::printf("targets_rows_san ok: %lld checks\n", static_cast<long long>(checked));
  return 0;
}
