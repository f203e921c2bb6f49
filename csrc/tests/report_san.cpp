// Stand-alone sanitizer check of the alignment report's host code: built with -fsanitize=address,undefined
// together with the CPU core sources (make report-san) and run as a plain program from the repository root.
//   * report_batch_cpu over every row of the six goldens (tests/data): counts against a letter-by-letter replay
//     written here, their sum, W . counts == the golden score, the marker bytes;
//   * hostile rows — n, k in {-1, INT32_MIN, INT32_MAX, 2^30}, n + L2 wrapping, k == L2, L2 > L1, L2 == 0 —
//     in exactly-sized heap buffers, so a row that formed an address would be a sanitizer report;
//   * K = 64 with padding rows;
//   * plan::plan_report (the host side of the GPU report): every record in exactly one wave item or the long
//     list, items within the lane and letter budgets, the implicit all-short form.
// Exit status 0 and "report_san ok" = all equal and no sanitizer report.
#include <climits>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "moc/cpu_engine.hpp"
#include "moc/io.hpp"
#include "moc/tile_plan.hpp"

namespace {

using moc::Result;

int failures = 0;
void check(bool ok, const char* what, long long a = 0, long long b = 0) {
  if (ok) return;
  std::fprintf(stderr, "report_san: %s (%lld, %lld)\n", what, a, b);
  ++failures;
}

std::string slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  std::stringstream ss;
  ss << f.rdbuf();
  return ss.str();
}

// the reference chain, letter by letter
void replay(const moc::ScoreTable& t, const std::vector<uint8_t>& s1, const uint8_t* s2, int64_t L2, const Result& r,
            int32_t (&c)[4], std::string& marks) {
  c[0] = c[1] = c[2] = c[3] = 0;
  marks.clear();
  for (int64_t i = 0; i < L2; ++i) {
    const int64_t at = (r.k == 0 || i < r.k) ? r.n + i : r.n + i + 1;
    const moc::PairClass pc = t.pair_class(s2[i], s1.at(static_cast<size_t>(at)));
    ++c[pc];
    marks.push_back(moc::ScoreTable::class_char(pc));
  }
}

void run_golden(int idx) {
  const std::string base = "tests/data/";
  const std::string in = slurp(base + "input" + std::to_string(idx) + ".txt");
  const std::string exp = slurp(base + "expected/input" + std::to_string(idx) + ".out");
  check(!in.empty() && !exp.empty(), "golden files missing (run from the repository root)", idx);
  if (in.empty() || exp.empty()) return;
  const moc::Problem p = moc::parse_problem(in.data(), in.size());
  const int64_t n = p.seq2.size();
  std::vector<Result> rows;
  std::istringstream es(exp);
  std::string line;
  while (std::getline(es, line)) {
    int i, s, o, k;
    if (std::sscanf(line.c_str(), "#%d: score: %d, n: %d, k: %d", &i, &s, &o, &k) == 4) rows.push_back(Result{s, o, k});
  }
  check(static_cast<int64_t>(rows.size()) == n, "golden row count", idx, static_cast<long long>(rows.size()));
  if (static_cast<int64_t>(rows.size()) != n) return;
  const moc::ScoreTable t = moc::ScoreTable::build(p.weights);
  for (int threads : {1, 3}) {
    std::vector<int32_t> counts(static_cast<size_t>(n) * 4, 7);
    std::vector<uint8_t> marks(static_cast<size_t>(p.seq2.total_chars()), 7);
    moc::report_batch_cpu(t, p.seq1.data(), p.L1(), p.seq2, rows.data(), 1, counts.data(), marks.data(), threads);
    for (int64_t i = 0; i < n; ++i) {
      int32_t want[4];
      std::string wm;
      const int64_t L2 = p.seq2.length(i);
      replay(t, p.seq1, p.seq2.record(i), L2, rows[i], want, wm);
      const int32_t* c = &counts[4 * i];
      check(c[0] == want[0] && c[1] == want[1] && c[2] == want[2] && c[3] == want[3], "golden counts", idx, i);
      check(c[0] + c[1] + c[2] + c[3] == L2, "golden counts sum", idx, i);
      const int64_t score = int64_t{p.weights.w[0]} * c[0] - int64_t{p.weights.w[1]} * c[1] -
                            int64_t{p.weights.w[2]} * c[2] - int64_t{p.weights.w[3]} * c[3];
      check(score == rows[i].score, "golden W . counts == score", idx, i);
      check(std::string(marks.begin() + p.seq2.offsets[i], marks.begin() + p.seq2.offsets[i + 1]) == wm, "golden marks",
            idx, i);
    }
  }
}

std::vector<uint8_t> codes_of(const std::string& s) {
  std::vector<uint8_t> v;
  for (char c : s) v.push_back(static_cast<uint8_t>(moc::letter_code(static_cast<unsigned char>(c))));
  return v;
}

void run_hostile() {
  moc::Weights w;
  w.w[0] = 10, w.w[1] = 2, w.w[2] = 3, w.w[3] = 4;
  const moc::ScoreTable t = moc::ScoreTable::build(w);
  const std::vector<uint8_t> s1 = codes_of("HELLOWORLDTHISISASEQ");  // L1 = 20, exactly sized on the heap
  const int64_t L1 = static_cast<int64_t>(s1.size());
  // records: L2 = 5, L2 == L1, L2 > L1 (21), L2 == 0, L2 = 1
  const std::vector<std::string> recs = {"WORLD", "HELLOWORLDTHISISASEQ", "HELLOWORLDTHISISASEQA", "", "S"};
  moc::RecordBatch batch;
  for (const std::string& r : recs) {
    const std::vector<uint8_t> c = codes_of(r);
    batch.push_back(c.data(), static_cast<int64_t>(c.size()));
  }
  const int64_t n = batch.size();
  const int32_t bad[] = {-1, INT32_MIN, INT32_MAX, 1 << 30};
  std::vector<std::pair<int32_t, int32_t>> nk;
  for (int32_t a : bad)
    for (int32_t b : bad) nk.push_back({a, b});
  for (int32_t a : bad) {
    nk.push_back({a, 0});
    nk.push_back({0, a});
  }
  nk.push_back({INT32_MAX - 2, 1});  // n + L2 wraps an int32
  nk.push_back({INT32_MAX - 4, 0});
  nk.push_back({0, 5});              // k == L2 of the first record
  nk.push_back({16, 0});             // n + L2 == L1 + 1 for L2 = 5
  nk.push_back({15, 1});             // the hyphen's extra column falls past Seq1
  nk.push_back({20, 0});
  for (const auto& q : nk)
    for (int threads : {1, 3}) {
      std::vector<Result> rows(static_cast<size_t>(n), Result{5, q.first, q.second});
      std::vector<int32_t> counts(static_cast<size_t>(n) * 4, 7);
      std::vector<uint8_t> marks(static_cast<size_t>(batch.total_chars()), 7);
      moc::report_batch_cpu(t, s1.data(), L1, batch, rows.data(), 1, counts.data(), marks.data(), threads);
      for (int64_t i = 0; i < n; ++i) {
        const bool valid = moc::report_row_valid(L1, batch.length(i), rows[i]);
        // a pair that is out of range for one record may be in range for a shorter one ((16, 0) for L2 = 1)
        int32_t want[4] = {-1, -1, -1, -1};
        std::string wm(static_cast<size_t>(batch.length(i)), '\0');
        if (valid) replay(t, s1, batch.record(i), batch.length(i), rows[i], want, wm);
        const int32_t* c = &counts[4 * i];
        check(c[0] == want[0] && c[1] == want[1] && c[2] == want[2] && c[3] == want[3], "hostile counts", q.first,
              q.second);
        check(std::string(marks.begin() + batch.offsets[i], marks.begin() + batch.offsets[i + 1]) == wm, "hostile marks",
              q.first, q.second);
      }
    }
  // the edges of validity themselves
  check(moc::report_row_valid(20, 5, Result{0, 15, 0}), "spec-only final offset is valid");
  check(!moc::report_row_valid(20, 5, Result{0, 16, 0}), "n + L2 > L1");
  check(moc::report_row_valid(20, 5, Result{0, 14, 4}), "last mutated offset, k = L2 - 1");
  check(!moc::report_row_valid(20, 5, Result{0, 15, 1}), "hyphen column past Seq1");
  check(!moc::report_row_valid(20, 5, Result{0, 0, 5}), "k == L2");
  check(moc::report_row_valid(20, 20, Result{0, 0, 0}), "L2 == L1 at (0, 0)");
  check(!moc::report_row_valid(20, 20, Result{0, 0, 1}), "L2 == L1 with a hyphen");
  check(!moc::report_row_valid(20, 21, Result{0, 0, 0}), "L2 > L1");
  check(!moc::report_row_valid(20, 0, Result{0, 0, 0}), "L2 == 0");
  check(!moc::report_row_valid(20, 5, Result{0, INT32_MAX, 1}), "n + L2 wraps");

  // K = 64: top-K rows of every record (few candidates each, so most rows are padding)
  const int K = 64;
  std::vector<Result> top(static_cast<size_t>(n) * K);
  moc::topk_batch_cpu(t, s1.data(), L1, batch, K, top.data(), moc::Semantics::Spec, 1);
  std::vector<int32_t> counts(static_cast<size_t>(n) * K * 4, 7);
  std::vector<uint8_t> marks(static_cast<size_t>(batch.total_chars()) * K, 7);
  moc::report_batch_cpu(t, s1.data(), L1, batch, top.data(), K, counts.data(), marks.data(), 3);
  for (int64_t i = 0; i < n; ++i)
    for (int j = 0; j < K; ++j) {
      const Result r = top[i * K + j];
      const int64_t L2 = batch.length(i);
      int32_t want[4] = {0, 0, 0, 0};
      std::string wm(static_cast<size_t>(L2), '\0');
      if (r.score != moc::kNoCandidateScore) {
        replay(t, s1, batch.record(i), L2, r, want, wm);
        check(w.w[0] * want[0] - w.w[1] * want[1] - w.w[2] * want[2] - w.w[3] * want[3] == r.score,
              "top-K W . counts == score", i, j);
      }
      const int32_t* c = &counts[4 * (i * K + j)];
      check(c[0] == want[0] && c[1] == want[1] && c[2] == want[2] && c[3] == want[3], "top-K counts", i, j);
      const uint8_t* m = marks.data() + K * batch.offsets[i] + j * L2;
      check(std::string(m, m + L2) == wm, "top-K marks", i, j);
    }
  bool threw = false;
  try {
    moc::report_batch_cpu(t, s1.data(), L1, batch, top.data(), 65, counts.data(), nullptr, 1);
  } catch (const moc::Error&) {
    threw = true;
  }
  check(threw, "K = 65 is refused");
}

// plan_report: walks a plan the way the kernels do
void check_plan(const std::vector<int64_t>& lens, int K, int64_t first_offset) {
  const int64_t n = static_cast<int64_t>(lens.size());
  std::vector<int64_t> off(static_cast<size_t>(n) + 1, first_offset);
  for (int64_t i = 0; i < n; ++i) off[i + 1] = off[i] + lens[i];
  const moc::plan::ReportPlan rp = moc::plan::plan_report(off.data(), n, K);
  check(rp.rpw == 64 / K && rp.K == K, "plan rpw", K);
  std::vector<int> seen(static_cast<size_t>(n), 0);
  bool any_long = false;
  for (int64_t L : lens) any_long = any_long || L > moc::bounds::kReportShortMaxL2;
  check(rp.implicit == !any_long, "plan implicit iff no long record", K, n);
  check(rp.implicit ? rp.items.empty() : static_cast<int64_t>(rp.items.size()) == rp.n_items, "plan item count");
  for (int64_t w = 0; w < rp.n_items; ++w) {
    const int64_t r0 = rp.implicit ? w * rp.rpw : rp.items[w].r0;
    const int64_t cnt = rp.implicit ? std::min<int64_t>(rp.rpw, n - r0) : rp.items[w].cnt;
    check(cnt >= 1 && cnt * K <= 64 && r0 >= 0 && r0 + cnt <= n, "plan item bounds", w, cnt);
    check(off[r0 + cnt] - off[r0] <= 64 * moc::bounds::kReportShortMaxL2, "plan item letter span", w);
    for (int64_t r = r0; r < r0 + cnt && r < n; ++r) {
      check(lens[r] <= moc::bounds::kReportShortMaxL2, "plan: long record in a wave item", r);
      ++seen[r];
    }
  }
  int64_t prev = -1;
  for (int32_t r : rp.long_recs) {
    check(r > prev && r < n && lens[r] > moc::bounds::kReportShortMaxL2, "plan long list", r);
    prev = r;
    if (r >= 0 && r < n) ++seen[r];
  }
  for (int64_t r = 0; r < n; ++r) check(seen[r] == 1, "plan: record covered once", r, seen[r]);
}

void run_plans() {
  const int64_t T = moc::bounds::kReportShortMaxL2;
  for (int K : {1, 2, 3, 5, 64}) {
    check_plan({}, K, 0);
    check_plan({1}, K, 0);
    check_plan({T}, K, 13);
    check_plan({T + 1}, K, 13);
    std::vector<int64_t> a, b, c;
    for (int i = 0; i < 257; ++i) a.push_back(1 + i % 40);             // mixed around the threshold
    for (int i = 0; i < 130; ++i) b.push_back(i % 7 == 3 ? 300 : 6);   // interleaved
    for (int i = 0; i < 200; ++i) c.push_back(T);                      // all at the bound: implicit
    check_plan(a, K, 0);
    check_plan(b, K, 5);
    check_plan(c, K, 0);
    check_plan({0, 0, 5, 0}, K, 0);
  }
  for (int K : {0, 65, -1}) {
    bool threw = false;
    const int64_t off[2] = {0, 4};
    try {
      (void)moc::plan::plan_report(off, 1, K);
    } catch (const moc::Error&) {
      threw = true;
    }
    check(threw, "plan refuses K", K);
  }
  bool threw = false;
  const int64_t dec[3] = {0, 4, 2};
  try {
    (void)moc::plan::plan_report(dec, 2, 1);
  } catch (const moc::Error&) {
    threw = true;
  }
  check(threw, "plan refuses decreasing offsets");
  // the class bits the kernels expand: two bits per entry, the table's own classes
  moc::Weights w;
  w.w[0] = 1;
  const moc::ScoreTable t = moc::ScoreTable::build(w);
  const moc::dev::ReportClassBits cb = moc::dev::report_class_bits(t.cls.data());
  for (int e = 0; e < 1024; ++e) check(((cb.w[e >> 4] >> (2 * (e & 15))) & 3u) == t.cls[e], "class bits", e);
}

}  // namespace

int main() {
  for (int i = 1; i <= 6; ++i) run_golden(i);
  run_hostile();
  run_plans();
  if (failures) {
    std::fprintf(stderr, "report_san: %d mismatches\n", failures);
    return 1;
  }
  std::puts("report_san ok");
  return 0;
}
