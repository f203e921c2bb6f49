// Stand-alone sanitizer check of the CPU engine's distinct placements: built with -fsanitize=address,undefined
// together with the CPU core sources (make peaks-san) and run as a plain program. On small random problems and a
// long plateau, for a range of radii: peaks_filter against the definition written here as a plain double loop (marks
// in heap blocks of exactly C bytes), the radius form of topk_batch_cpu against the ranked peaks, and the radius form
// of hits_batch_cpu against the filtered peaks with cap = 0 (null rows), 1, total - 1 and total rows in heap blocks
// of exactly cap rows, so a store at or past rows + cap is an ASan report. Exit status 0 = all equal and no
// sanitizer report.
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

int failures = 0;
int64_t checked = 0;

void fail(const char* what, int problem, int sem, int64_t radius, int64_t extra) {
  std::fprintf(stderr, "peaks_san: %s (problem %d, semantics %d, radius %lld, %lld)\n", what, problem, sem,
               static_cast<long long>(radius), static_cast<long long>(extra));
  ++failures;
}

uint32_t rng_state = 4242u;
uint32_t rnd(uint32_t m) {
  rng_state = rng_state * 1664525u + 1013904223u;
  return (rng_state >> 8) % m;
}

bool better_entry(const ProfileEntry& a, int64_t oa, const ProfileEntry& b, int64_t ob) {
  return a.score > b.score || (a.score == b.score && oa < ob);
}

// the definition, entry by entry
std::vector<uint8_t> peaks_by_definition(const ProfileEntry* p, int64_t C, int64_t R) {
  std::vector<uint8_t> peak(static_cast<size_t>(C), 1);
  for (int64_t o = 0; o < C; ++o)
    for (int64_t o2 = std::max<int64_t>(0, o - R); o2 <= std::min(C - 1, o + R); ++o2)
      if (o2 != o && better_entry(p[o2], o2, p[o], o)) peak[o] = 0;
  return peak;
}

bool same(const Result& a, const Result& b) { return a.score == b.score && a.n == b.n && a.k == b.k; }

void run_problem(int id, const moc::Weights& w, int64_t L1, const std::vector<int64_t>& lens, int alphabet,
                 const std::vector<int64_t>& radii) {
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
    std::vector<int64_t> po(static_cast<size_t>(n) + 1);
    moc::profile_offsets(L1, batch, sem, po.data());
    std::vector<ProfileEntry> prof(static_cast<size_t>(std::max<int64_t>(po[n], 1)));
    moc::profile_batch_cpu(t, s1.data(), L1, batch, po.data(), prof.data(), sem, 1);
    for (int64_t R : radii) {
      // the filter itself, marks in a block of exactly C bytes
      std::vector<std::vector<uint8_t>> peaks;
      for (int64_t i = 0; i < n; ++i) {
        const int64_t C = po[i + 1] - po[i];
        peaks.push_back(peaks_by_definition(prof.data() + po[i], C, R));
        std::unique_ptr<uint8_t[]> got(C ? new uint8_t[static_cast<size_t>(C)] : nullptr);
        moc::peaks_filter(prof.data() + po[i], C, R, got.get());
        for (int64_t o = 0; o < C; ++o) {
          if (got[o] != peaks.back()[o]) {
            fail("peaks_filter differs from the definition", id, static_cast<int>(sem), R, o);
            break;
          }
          ++checked;
        }
      }
      // distinct top-K: the peaks in better() order, then padding
      for (int K : {1, 3, moc::kMaxTopK}) {
        std::unique_ptr<Result[]> out(new Result[static_cast<size_t>(n * K)]);
        for (int threads : {1, 3}) {
          moc::topk_batch_cpu(t, s1.data(), L1, batch, K, out.get(), sem, threads, R);
          for (int64_t i = 0; i < n; ++i) {
            std::vector<Result> want;
            for (int64_t o = 0; o < po[i + 1] - po[i]; ++o)
              if (peaks[i][o]) want.push_back(Result{prof[po[i] + o].score, static_cast<int32_t>(o), prof[po[i] + o].k});
            std::stable_sort(want.begin(), want.end(), [](const Result& a, const Result& b) { return moc::better(a, b); });
            for (int j = 0; j < K; ++j) {
              const Result exp = j < static_cast<int>(want.size()) ? want[j] : moc::no_candidate();
              if (!same(out[i * K + j], exp)) {
                fail("distinct top-K differs", id, static_cast<int>(sem), R, i * K + j);
                break;
              }
              ++checked;
            }
          }
        }
      }
      // distinct hits under the whole profile and under a middle threshold per record, every capacity
      for (int edge = 0; edge < 2; ++edge) {
        std::vector<int32_t> per(static_cast<size_t>(n), 0);
        for (int64_t i = 0; i < n; ++i)
          if (po[i + 1] > po[i]) per[i] = prof[(po[i] + po[i + 1]) / 2].score;
        const int32_t* thr = edge ? per.data() : nullptr;
        std::vector<int64_t> want_h(static_cast<size_t>(n) + 1, 0);
        std::vector<Result> want;
        for (int64_t i = 0; i < n; ++i) {
          const int32_t ti = thr ? thr[i] : INT32_MIN;
          for (int64_t o = 0; o < po[i + 1] - po[i]; ++o)
            if (peaks[i][o] && prof[po[i] + o].score >= ti)
              want.push_back(Result{prof[po[i] + o].score, static_cast<int32_t>(o), prof[po[i] + o].k});
          want_h[i + 1] = static_cast<int64_t>(want.size());
        }
        const int64_t total = want_h[n];
        for (int threads : {1, 3})
          for (int64_t cap : {int64_t{0}, int64_t{1}, total - 1, total}) {
            if (cap < 0) continue;
            std::vector<int64_t> h(static_cast<size_t>(n) + 1, -7);
            std::unique_ptr<Result[]> rows(cap ? new Result[static_cast<size_t>(cap)] : nullptr);  // exactly cap rows
            for (int64_t j = 0; j < cap; ++j) rows[j] = Result{-1, -1, -1};
            moc::hits_batch_cpu(t, s1.data(), L1, batch, INT32_MIN, thr, h.data(), rows.get(), cap, sem, threads, R);
            if (h != want_h) fail("hoffsets differ", id, static_cast<int>(sem), R, cap);
            for (int64_t j = 0; j < cap; ++j) {
              const Result exp = j < total ? want[static_cast<size_t>(j)] : Result{-1, -1, -1};
              if (!same(rows[j], exp)) {
                fail("distinct hits differ", id, static_cast<int>(sem), R, cap);
                break;
              }
              ++checked;
            }
          }
      }
    }
  }
}

}  // namespace

int main() {
  moc::Weights w;
  w.w[0] = 4, w.w[1] = 3, w.w[2] = 2, w.w[3] = 10;
  moc::Weights z;  // all-zero weights: every profile is one plateau
  const std::vector<int64_t> radii = {0, 1, 2, 3, 5, 8, 22, 23, 1000, moc::bounds::kPeaksMaxRadius};
  int id = 0;
  run_problem(id++, w, 23, {23, 24, 1, 2, 22, 7, 11}, 26, radii);
  run_problem(id++, w, 17, {5, 1, 16, 17, 18, 3}, 3, radii);
  run_problem(id++, z, 12, {1, 4, 11, 12, 13}, 26, radii);
  run_problem(id++, w, 1, {1, 2}, 26, radii);
  run_problem(id++, w, 208, {8}, 1, {3, 199, 200, 201});  // Seq1 and the record all 'A': one long plateau
  std::vector<int64_t> many;
  for (int i = 0; i < 40; ++i) many.push_back(1 + i % 9);
  run_problem(id++, w, 19, many, 4, radii);
  run_problem(id++, w, 3000, {200, 5}, 26, {1, 64, 2047, moc::bounds::kPeaksMaxRadius});
  // a radius out of range is an error, not a clamp
  for (int64_t bad : {int64_t{-1}, int64_t{moc::bounds::kPeaksMaxRadius} + 1}) {
    bool threw = false;
    try {
      uint8_t mark = 0;
      const ProfileEntry e{0, 0};
      moc::peaks_filter(&e, 1, bad, &mark);
    } catch (const moc::Error&) {
      threw = true;
    }
    if (!threw) fail("radius out of range accepted", -1, 0, bad, 0);
  }
  if (failures) {
    std::fprintf(stderr, "peaks_san: %d mismatches\n", failures);
    return 1;
  }
  std::printf("peaks_san ok (%lld values checked)\n", static_cast<long long>(checked));
  return 0;
}
