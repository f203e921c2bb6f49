// Stand-alone sanitizer check of the per-offset profile and top-K code of the CPU engine: built with
// -fsanitize=address,undefined together with the CPU core sources (make profile-san) and run as a plain
// program. profile_batch_cpu and topk_batch_cpu on a few hand-made records against a literal letter-by-
// letter replay written here; exit status 0 = all equal and no sanitizer report.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "moc/cpu_engine.hpp"

namespace {

using moc::ProfileEntry;
using moc::Result;
using moc::Semantics;

std::vector<uint8_t> codes_of(const std::string& s) {
  std::vector<uint8_t> v;
  for (char c : s) v.push_back(static_cast<uint8_t>(moc::letter_code(static_cast<unsigned char>(c))));
  return v;
}

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

void check(bool ok, const char* what, int64_t rec, int sem, int threads) {
  if (ok) return;
  std::fprintf(stderr, "profile_san: %s differs (record %lld, semantics %d, threads %d)\n", what,
               static_cast<long long>(rec), sem, threads);
  ++failures;
}

void run_case(const moc::Weights& w, const std::string& seq1, const std::vector<std::string>& recs) {
  const moc::ScoreTable t = moc::ScoreTable::build(w);
  const std::vector<uint8_t> s1 = codes_of(seq1);
  const int64_t L1 = static_cast<int64_t>(s1.size());
  moc::RecordBatch batch;
  std::vector<std::vector<uint8_t>> rc;
  for (const std::string& r : recs) {
    rc.push_back(codes_of(r));
    batch.push_back(rc.back().data(), static_cast<int64_t>(rc.back().size()));
  }
  const int64_t n = batch.size();
  for (Semantics sem : {Semantics::Reference, Semantics::Spec})
    for (int threads : {1, 3}) {
      std::vector<int64_t> poff(static_cast<size_t>(n) + 1);
      moc::profile_offsets(L1, batch, sem, poff.data());
      std::vector<ProfileEntry> prof(static_cast<size_t>(poff[n]));
      moc::profile_batch_cpu(t, s1.data(), L1, batch, poff.data(), prof.data(), sem, threads);
      for (int K : {1, 3, 64}) {
        std::vector<Result> top(static_cast<size_t>(n) * K);
        moc::topk_batch_cpu(t, s1.data(), L1, batch, K, top.data(), sem, threads);
        for (int64_t i = 0; i < n; ++i) {
          const std::vector<ProfileEntry> want = replay(t, s1, rc[i], sem);
          const int64_t C = static_cast<int64_t>(want.size());
          bool same = poff[i + 1] - poff[i] == C && C == moc::candidate_offsets(L1, batch.length(i), sem);
          for (int64_t o = 0; same && o < C; ++o)
            same = prof[poff[i] + o].score == want[o].score && prof[poff[i] + o].k == want[o].k;
          check(same, "profile", i, static_cast<int>(sem), threads);
          // the K best offsets of the replayed profile: higher score, then smaller offset (a stable sort)
          std::vector<int64_t> order(static_cast<size_t>(C));
          for (int64_t o = 0; o < C; ++o) order[o] = o;
          std::stable_sort(order.begin(), order.end(),
                           [&](int64_t a, int64_t b) { return want[a].score > want[b].score; });
          bool rows = true;
          for (int j = 0; rows && j < K; ++j) {
            const Result got = top[i * K + j];
            const Result exp = j < C ? Result{want[order[j]].score, static_cast<int32_t>(order[j]), want[order[j]].k}
                                     : moc::no_candidate();
            rows = got.score == exp.score && got.n == exp.n && got.k == exp.k;
          }
          check(rows, "top-K", i, static_cast<int>(sem), threads);
          if (K == 1) {  // row 0 is the search's result
            const Result r = moc::solve_record(t, s1.data(), L1, rc[i].data(), batch.length(i), sem);
            const Result got = top[i];
            check(got.score == r.score && got.n == r.n && got.k == r.k, "row 0 vs solve_record", i,
                  static_cast<int>(sem), threads);
          }
        }
      }
    }
}

}  // namespace

int main() {
  moc::Weights w;
  w.w[0] = 10, w.w[1] = 2, w.w[2] = 3, w.w[3] = 4;
  const std::string seq1 = "HELLOWORLDTHISISASEQUENCEOFLETTERSXYZ";  // 37 letters
  // L2 == L1, L2 > L1, L2 == 1, L2 == 2, L2 == L1 - 1 (one offset: K > C), a repeat (ties), mid lengths
  run_case(w, seq1, {seq1, seq1 + "A", "S", "LO", seq1.substr(1), "SS", "ISASEQ", "OWORLDTHISISASEQUENCEOFLETTERS"});
  moc::Weights z;  // all-zero weights: every candidate ties, k = 0 and n ascending
  run_case(z, "AAAAAAAAAAAAAAAAAAAA", {"A", "AAAAA", "AAAAAAAAAAAAAAAAAAA", "AAAAAAAAAAAAAAAAAAAA"});
  // many records: the parallel-over-records branch of the batch calls
  std::vector<std::string> many;
  for (int i = 0; i < 40; ++i) many.push_back(seq1.substr(static_cast<size_t>(i % 30), static_cast<size_t>(1 + i % 7)));
  run_case(w, seq1, many);
  if (failures) {
    std::fprintf(stderr, "profile_san: %d mismatches\n", failures);
    return 1;
  }
  std::puts("profile_san ok");
  return 0;
}
