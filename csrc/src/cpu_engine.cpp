#include "moc/cpu_engine.hpp"

#include <string>

#include <omp.h>

#include <algorithm>
#include <functional>
#include <vector>

namespace moc {

int64_t candidate_offsets(int64_t L1, int64_t L2, Semantics sem) {
  if (L2 > L1 || L2 <= 0) return 0;
  if (L2 == L1) return 1;
  return sem == Semantics::Spec ? L1 - L2 + 1 : L1 - L2;
}

namespace {

inline void consider(Result& best, int32_t score, int64_t o, int64_t k) {
  Result c{score, static_cast<int32_t>(o), static_cast<int32_t>(k)};
  if (best.n < 0 || better(c, best)) best = c;
}


// The one-pass-per-offset recurrence over offsets [o_begin, o_end) of a record's candidate set:
// emit(o, score, k) receives every offset's best candidate (k = 0 first, then the smallest k).
template <class Emit>
inline void sweep_offsets(const ScoreTable& t, const uint8_t* s1, int64_t L1, const uint8_t* s2, int64_t L2,
                          int64_t o_begin, int64_t o_end, Semantics sem, Emit&& emit) {
  const int64_t n_off = candidate_offsets(L1, L2, sem);
  o_end = std::min(o_end, n_off);
  if (o_begin >= o_end) return;
  if (L2 == L1) {  // equal lengths: un-shifted, un-mutated only (cudaFunctions.cu:74-106)
    int32_t s = 0;
    for (int64_t i = 0; i < L2; ++i) s += t.lut[s2[i] * kLutStride + s1[i]];
    emit(int64_t{0}, s, int64_t{0});
    return;
  }
  const int64_t last_mut_off = L1 - L2;  // offsets with a hyphen need o + L2 + 1 <= L1
  // per-thread scratch (no allocation per record): LUT row of every Seq2 letter, and P_o(1..L2) of the
  // current diagonal; each offset then takes ONE fused pass over its neighbour diagonal: prefix
  // P_{o+1}(i+1), difference D_o(i+1) = P_o(i+1) - P_{o+1}(i+1) and its running max (strict '>': the
  // smallest k wins ties, as the reference loop order does)
  thread_local std::vector<const int32_t*> rows;
  thread_local std::vector<int32_t> cur;
  if (static_cast<int64_t>(rows.size()) < L2) rows.resize(static_cast<size_t>(L2));
  if (static_cast<int64_t>(cur.size()) < L2 + 1) cur.resize(static_cast<size_t>(L2) + 1);
  for (int64_t i = 0; i < L2; ++i) rows[i] = t.lut.data() + s2[i] * kLutStride;
  const int32_t* const* rw = rows.data();
  int32_t* P = cur.data();
  {
    int32_t acc = 0;
    const uint8_t* a = s1 + o_begin;
    for (int64_t i = 0; i < L2; ++i) P[i + 1] = acc += rw[i][a[i]];
  }
  for (int64_t o = o_begin; o < o_end; ++o) {
    const int32_t tot = P[L2];  // the un-mutated candidate
    if (o >= last_mut_off) {
      emit(o, tot, int64_t{0});
      continue;
    }
    const uint8_t* a = s1 + o + 1;
    int32_t q = 0, bd = INT32_MIN;
    int64_t bk = 0;
    for (int64_t i = 0; i + 1 < L2; ++i) {  // candidates k = i + 1 = 1 .. L2-1
      q += rw[i][a[i]];
      const int32_t d = P[i + 1] - q;
      P[i + 1] = q;  // becomes P_{o+1}(i+1) for the next offset
      if (d > bd) {
        bd = d;
        bk = i + 1;
      }
    }
    q += rw[L2 - 1][a[L2 - 1]];
    P[L2] = q;  // Tot_{o+1}
    if (L2 >= 2 && bd + q > tot)
      emit(o, bd + q, bk);
    else
      emit(o, tot, int64_t{0});
  }
}

}  // namespace

Result solve_offsets(const ScoreTable& t, const uint8_t* s1, int64_t L1, const uint8_t* s2, int64_t L2,
                     int64_t o_begin, int64_t o_end, Semantics sem) {
  Result best{kNoCandidateScore, -1, -1};
  sweep_offsets(t, s1, L1, s2, L2, o_begin, o_end, sem,
                [&](int64_t o, int32_t score, int64_t k) { consider(best, score, o, k); });
  return best;
}

Result solve_record(const ScoreTable& t, const uint8_t* s1, int64_t L1, const uint8_t* s2, int64_t L2,
                    Semantics sem) {
  Result r = solve_offsets(t, s1, L1, s2, L2, 0, L1 + 1, sem);
  return r.n < 0 ? no_candidate() : r;
}

namespace {
// Threads worth waking for `cells` of search work: a thread per ~0.25 M cells (~0.5 ms at the engine's
// rate), so a reference-sized job (input6: 730 cells) runs on the calling thread without forking a team —
// the team's start-up and spin-down cost more than the whole search (49-63 ms vs 26 ms).
int threads_for(const RecordBatch& batch, int64_t L1, Semantics sem, int nt) {
  if (nt <= 1) return 1;
  const int64_t n = batch.size();
  int64_t cells = 0;
  for (int64_t i = 0; i < n && cells < int64_t{nt} << 18; ++i)
    cells += candidate_offsets(L1, batch.length(i), sem) * std::max<int64_t>(batch.length(i), 1);
  return static_cast<int>(std::clamp<int64_t>(cells >> 18, 1, nt));
}
}  // namespace

void solve_batch_cpu(const ScoreTable& t, const uint8_t* s1, int64_t L1, const RecordBatch& batch, Result* out,
                     Semantics sem, int num_threads) {
  const int64_t n = batch.size();
  const int nt = threads_for(batch, L1, sem, num_threads > 0 ? num_threads : omp_get_max_threads());
  if (n >= 4 * nt || nt == 1) {
    // dynamic balance in chunks: per-record dispatch would dominate tiny records (input6: ~150 cells)
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(1024, n / (64 * nt)));
#pragma omp parallel for schedule(dynamic, chunk) num_threads(nt) if (nt > 1)
    for (int64_t i = 0; i < n; ++i) out[i] = solve_record(t, s1, L1, batch.record(i), batch.length(i), sem);
    return;
  }
  // Few records: split every record's offset range into chunks and run all (record, chunk) items in ONE
  // parallel loop (one fork/join for the batch, dynamic balance), then merge per record — max is
  // order-free, so the result does not depend on the thread count.
  struct Item {
    int64_t rec, ob, oe;
  };
  std::vector<Item> items;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t n_off = candidate_offsets(L1, batch.length(i), sem);
    const int64_t chunk = std::max<int64_t>(16, (n_off + 4 * nt - 1) / (4 * nt));
    if (n_off <= 1) {
      items.push_back(Item{i, 0, L1 + 1});
      continue;
    }
    for (int64_t ob = 0; ob < n_off; ob += chunk) items.push_back(Item{i, ob, std::min(n_off, ob + chunk)});
  }
  std::vector<Result> part(items.size());
#pragma omp parallel for schedule(dynamic, 1) num_threads(nt) if (nt > 1)
  for (int64_t j = 0; j < static_cast<int64_t>(items.size()); ++j) {
    const Item& it = items[j];
    part[j] = solve_offsets(t, s1, L1, batch.record(it.rec), batch.length(it.rec), it.ob, it.oe, sem);
  }
  for (int64_t i = 0; i < n; ++i) out[i] = Result{kNoCandidateScore, -1, -1};
  for (size_t j = 0; j < items.size(); ++j) {
    Result& b = out[items[j].rec];
    const Result& p = part[j];
    if (p.n >= 0 && (b.n < 0 || better(p, b))) b = p;
  }
  for (int64_t i = 0; i < n; ++i)
    if (out[i].n < 0) out[i] = no_candidate();
}

void solve_keys_cpu(const ScoreTable& t, const uint8_t* s1, int64_t L1, const RecordBatch& batch, int part,
                    int parts, uint64_t* keys, Semantics sem, int num_threads) {
  if (parts < 1 || part < 0 || part >= parts) throw Error("solve_keys_cpu: bad part");
  const int64_t n = batch.size();
  const int nt = threads_for(batch, L1, sem, num_threads > 0 ? num_threads : omp_get_max_threads());
  auto range = [&](int64_t i, int64_t& b, int64_t& e) {
    const int64_t c = candidate_offsets(L1, batch.length(i), sem);
    b = c * part / parts;
    e = c * (part + 1) / parts;
  };
  if (n >= 4 * nt || nt == 1) {
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(1024, n / (64 * nt)));
#pragma omp parallel for schedule(dynamic, chunk) num_threads(nt) if (nt > 1)
    for (int64_t i = 0; i < n; ++i) {
      int64_t b, e;
      range(i, b, e);
      const int64_t L2 = batch.length(i);
      keys[i] = encode_key(solve_offsets(t, s1, L1, batch.record(i), L2, b, e, sem));
    }
    return;
  }
  // few records: this part's range of every record in chunks, one parallel loop for the batch
  struct Item {
    int64_t rec, ob, oe;
  };
  std::vector<Item> items;
  for (int64_t i = 0; i < n; ++i) {
    int64_t b, e;
    range(i, b, e);
    const int64_t chunk = std::max<int64_t>(16, (e - b + 4 * nt - 1) / (4 * nt));
    for (int64_t ob = b; ob < e; ob += chunk) items.push_back(Item{i, ob, std::min(e, ob + chunk)});
  }
  std::vector<uint64_t> pk(items.size());
#pragma omp parallel for schedule(dynamic, 1) num_threads(nt) if (nt > 1)
  for (int64_t j = 0; j < static_cast<int64_t>(items.size()); ++j) {
    const Item& it = items[j];
    const int64_t L2 = batch.length(it.rec);
    pk[j] = encode_key(solve_offsets(t, s1, L1, batch.record(it.rec), L2, it.ob, it.oe, sem));
  }
  for (int64_t i = 0; i < n; ++i) keys[i] = 0;
  for (size_t j = 0; j < items.size(); ++j) keys[items[j].rec] = std::max(keys[items[j].rec], pk[j]);
}

void profile_offsets(int64_t L1, const RecordBatch& batch, Semantics sem, int64_t* poffsets) {
  poffsets[0] = 0;
  for (int64_t i = 0; i < batch.size(); ++i) poffsets[i + 1] = poffsets[i] + candidate_offsets(L1, batch.length(i), sem);
}

namespace {
inline void profile_range(const ScoreTable& t, const uint8_t* s1, int64_t L1, const uint8_t* s2, int64_t L2,
                          int64_t o_begin, int64_t o_end, Semantics sem, ProfileEntry* prof) {
  sweep_offsets(t, s1, L1, s2, L2, o_begin, o_end, sem, [&](int64_t o, int32_t score, int64_t k) {
    prof[o] = ProfileEntry{score, static_cast<int32_t>(k)};
  });
}

// The min(K, C) best offsets of a profile in better() order (higher score, then smaller n), then padding.
// Keys as on the device (topk_select_kernel): (score ^ 2^31) << 32 | (2^32 - 1 - o), larger is better.
void select_topk(const ProfileEntry* prof, int64_t C, int K, Result* out, std::vector<uint64_t>& keys) {
  keys.resize(static_cast<size_t>(C));
  for (int64_t o = 0; o < C; ++o)
    keys[o] = (static_cast<uint64_t>(static_cast<uint32_t>(prof[o].score) ^ 0x80000000u) << 32) |
              (0xffffffffu - static_cast<uint32_t>(o));
  const int64_t m = std::min<int64_t>(K, C);
  std::partial_sort(keys.begin(), keys.begin() + m, keys.end(), std::greater<uint64_t>());
  for (int64_t j = 0; j < m; ++j) {
    const int64_t o = 0xffffffffu - static_cast<uint32_t>(keys[j]);
    out[j] = Result{prof[o].score, static_cast<int32_t>(o), prof[o].k};
  }
  for (int64_t j = m; j < K; ++j) out[j] = no_candidate();
}

// (record, offset chunk) work items of a batch with few records, as solve_batch_cpu cuts them
struct OffsetItem {
  int64_t rec, ob, oe;
};
void offset_items(int64_t rec, int64_t n_off, int nt, std::vector<OffsetItem>& items) {
  const int64_t chunk = std::max<int64_t>(16, (n_off + 4 * nt - 1) / (4 * nt));
  for (int64_t ob = 0; ob < n_off; ob += chunk) items.push_back(OffsetItem{rec, ob, std::min(n_off, ob + chunk)});
}
}  // namespace

void profile_batch_cpu(const ScoreTable& t, const uint8_t* s1, int64_t L1, const RecordBatch& batch,
                       const int64_t* poffsets, ProfileEntry* prof, Semantics sem, int num_threads) {
  const int64_t n = batch.size();
  const int nt = threads_for(batch, L1, sem, num_threads > 0 ? num_threads : omp_get_max_threads());
  if (n >= 4 * nt || nt == 1) {
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(1024, n / (64 * nt)));
#pragma omp parallel for schedule(dynamic, chunk) num_threads(nt) if (nt > 1)
    for (int64_t i = 0; i < n; ++i)
      profile_range(t, s1, L1, batch.record(i), batch.length(i), 0, L1 + 1, sem, prof + poffsets[i]);
    return;
  }
  std::vector<OffsetItem> items;
  for (int64_t i = 0; i < n; ++i) offset_items(i, poffsets[i + 1] - poffsets[i], nt, items);
#pragma omp parallel for schedule(dynamic, 1) num_threads(nt) if (nt > 1)
  for (int64_t j = 0; j < static_cast<int64_t>(items.size()); ++j) {
    const OffsetItem& it = items[j];
    profile_range(t, s1, L1, batch.record(it.rec), batch.length(it.rec), it.ob, it.oe, sem, prof + poffsets[it.rec]);
  }
}

namespace {
// fn(i, prof, C) for every record i with its C-entry profile. One record's profile exists at a time per thread,
// never the batch's: records in parallel when there are many, else one record at a time with its offset chunks in
// parallel (fn then runs on the calling thread, in record order).
template <class Fn>
void for_each_profile(const ScoreTable& t, const uint8_t* s1, int64_t L1, const RecordBatch& batch, Semantics sem,
                      int num_threads, Fn&& fn) {
  const int64_t n = batch.size();
  const int nt = threads_for(batch, L1, sem, num_threads > 0 ? num_threads : omp_get_max_threads());
  if (n >= 4 * nt || nt == 1) {
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(1024, n / (64 * nt)));
#pragma omp parallel num_threads(nt) if (nt > 1)
    {
      std::vector<ProfileEntry> prof;
#pragma omp for schedule(dynamic, chunk)
      for (int64_t i = 0; i < n; ++i) {
        const int64_t C = candidate_offsets(L1, batch.length(i), sem);
        prof.resize(static_cast<size_t>(C));
        profile_range(t, s1, L1, batch.record(i), batch.length(i), 0, C, sem, prof.data());
        fn(i, prof.data(), C);
      }
    }
    return;
  }
  std::vector<ProfileEntry> prof;
  std::vector<OffsetItem> items;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t C = candidate_offsets(L1, batch.length(i), sem);
    prof.resize(static_cast<size_t>(C));
    items.clear();
    offset_items(i, C, nt, items);
#pragma omp parallel for schedule(dynamic, 1) num_threads(nt) if (nt > 1)
    for (int64_t j = 0; j < static_cast<int64_t>(items.size()); ++j)
      profile_range(t, s1, L1, batch.record(i), batch.length(i), items[j].ob, items[j].oe, sem, prof.data());
    fn(i, prof.data(), C);
  }
}
}  // namespace

void check_peaks_radius(int64_t radius) {
  if (radius < 0 || radius > bounds::kPeaksMaxRadius)
    throw Error("distinct: radius must be in 0.." + std::to_string(bounds::kPeaksMaxRadius) + ", got " +
                std::to_string(radius));
}

namespace {
inline uint64_t profile_key(const ProfileEntry& e, int64_t o) {
  return (static_cast<uint64_t>(static_cast<uint32_t>(e.score) ^ 0x80000000u) << 32) |
         (0xffffffffu - static_cast<uint32_t>(o));
}
}  // namespace

// Sliding-window maximum of the keys over [o - R, o + R] clipped to [0, C): dq holds the offsets of the window's
// candidates for the maximum, keys decreasing from front to back. Entry o is a peak iff the front is o itself.
void peaks_filter(const ProfileEntry* prof, int64_t C, int64_t radius, uint8_t* peak) {
  check_peaks_radius(radius);
  if (C <= 0) return;
  if (radius == 0) {
    std::fill(peak, peak + C, uint8_t{1});
    return;
  }
  thread_local std::vector<int64_t> dq;  // a ring would do; the offsets only ever move forward
  dq.resize(static_cast<size_t>(C));
  int64_t head = 0, tail = 0, next = 0;  // dq[head .. tail); entries [0, next) have entered the window
  for (int64_t o = 0; o < C; ++o) {
    const int64_t hi = std::min(C - 1, o + radius);
    for (; next <= hi; ++next) {
      const uint64_t k = profile_key(prof[next], next);
      while (tail > head && profile_key(prof[dq[tail - 1]], dq[tail - 1]) < k) --tail;
      dq[tail++] = next;
    }
    while (dq[head] < o - radius) ++head;  // never empties: o itself entered and nothing after it has left
    peak[o] = dq[head] == o ? 1 : 0;
  }
}

void check_summary_args(int32_t max_abs_weight, int64_t max_l2, int64_t max_count, int32_t bins, int32_t width) {
  if (bins < 0 || bins > bounds::kSummaryMaxBins)
    throw Error("summary: bins must be in 0.." + std::to_string(bounds::kSummaryMaxBins) + ", got " + std::to_string(bins));
  if (width < 1) throw Error("summary: width must be at least 1, got " + std::to_string(width));
  if (!bounds::summary_exact(max_abs_weight, max_l2, max_count))
    throw Error("summary: exactness bound: a profile of " + std::to_string(max_count) + " entries with |score| <= min(2^31, " +
                std::to_string(max_abs_weight) + " * " + std::to_string(max_l2) + ") may overflow the int64 sum of squares (at most " +
                std::to_string(bounds::summary_max_count(max_abs_weight, max_l2)) + " entries per record are exact)");
}

void summary_batch_cpu(const ScoreTable& t, const uint8_t* s1, int64_t L1, const RecordBatch& batch, int64_t* summary,
                       int32_t* hist, int32_t bins, int32_t lo, int32_t width, Semantics sem, int num_threads) {
  const int64_t n = batch.size();
  int64_t max_count = 0;
  for (int64_t i = 0; i < n; ++i) max_count = std::max(max_count, candidate_offsets(L1, batch.length(i), sem));
  check_summary_args(t.max_abs(), n ? batch.max_length() : 0, max_count, bins, width);
  if (bins > 0 && !hist) throw Error("summary: bins > 0 need a hist buffer");
  for_each_profile(t, s1, L1, batch, sem, num_threads, [&](int64_t i, const ProfileEntry* prof, int64_t C) {
    int64_t sum = 0, sumsq = 0, best = 0;
    int32_t mn = INT32_MAX, mx = INT32_MIN;
    int32_t* h = bins > 0 ? hist + i * bins : nullptr;
    if (h) std::fill(h, h + bins, 0);
    for (int64_t o = 0; o < C; ++o) {
      const int64_t s = prof[o].score;
      sum += s;
      sumsq += s * s;
      mn = std::min(mn, prof[o].score);
      if (prof[o].score > mx) {  // strict: the smallest offset keeps a tie
        mx = prof[o].score;
        best = o;
      }
      if (h) ++h[summary_bin(prof[o].score, lo, width, bins)];
    }
    int64_t* row = summary + i * kSummaryCols;
    row[0] = C;
    row[1] = sum;
    row[2] = sumsq;
    row[3] = mn;
    row[4] = mx;
    row[5] = C > 0 ? best : 0;
    row[6] = C > 0 ? prof[best].k : 0;
  });
}

void check_targets(const int64_t* starts, int64_t T, int64_t L1) {
  if (T < 1 || T > bounds::kTargetsMax)
    throw Error("targets: T must be in 1.." + std::to_string(bounds::kTargetsMax) + ", got " + std::to_string(T));
  if (!starts) throw Error("targets: no starts");
  if (starts[0] != 0) throw Error("targets: starts[0] must be 0, got " + std::to_string(starts[0]));
  for (int64_t t = 0; t < T; ++t)
    if (starts[t + 1] <= starts[t])
      throw Error("targets: starts must rise strictly (every target holds at least one letter): starts[" +
                  std::to_string(t + 1) + "] = " + std::to_string(starts[t + 1]) + " after " + std::to_string(starts[t]));
  if (starts[T] != L1)
    throw Error("targets: starts[T] must be the catalog's length " + std::to_string(L1) + ", got " + std::to_string(starts[T]));
}

namespace {
// rows[q] = record (s2, L2)'s row against target q alone, from the record's catalog profile `prof`: the definition
// both targets_batch_cpu and targets_rank_batch_cpu state their rows by
inline void target_rows(const ScoreTable& t, const uint8_t* s1, int64_t L1, const uint8_t* s2, int64_t L2,
                        const ProfileEntry* prof, const int64_t* starts, int64_t T, Semantics sem, Result* rows) {
  for (int64_t q = 0; q < T; ++q) {
    const int64_t b = starts[q], len = starts[q + 1] - b;
    if (L2 < 1 || L2 > len || L2 > L1) {
      rows[q] = no_candidate();
      continue;
    }
    Result best = no_candidate();
    bool have = false;
    const int64_t slice = len - L2;  // b + slice <= L1 - L2 <= C
    for (int64_t o = 0; o < slice; ++o) {
      const ProfileEntry& e = prof[b + o];
      if (!have || e.score > best.score) {  // strict: the smallest offset keeps a tie
        best = Result{e.score, static_cast<int32_t>(o), e.k};
        have = true;
      }
    }
    if (sem == Semantics::Spec || slice == 0) {  // the boundary diagonal, from the letters
      const uint8_t* a = s1 + b + slice;
      int32_t s = 0;
      for (int64_t l = 0; l < L2; ++l) s += t.lut[s2[l] * kLutStride + a[l]];
      if (!have || s > best.score) best = Result{s, static_cast<int32_t>(slice), 0};
    }
    rows[q] = best;
  }
}
}  // namespace

void targets_batch_cpu(const ScoreTable& t, const uint8_t* s1, int64_t L1, const RecordBatch& batch,
                       const int64_t* starts, int64_t T, Result* out, Semantics sem, int num_threads) {
  check_targets(starts, T, L1);
  for_each_profile(t, s1, L1, batch, sem, num_threads, [&](int64_t i, const ProfileEntry* prof, int64_t) {
    target_rows(t, s1, L1, batch.record(i), batch.length(i), prof, starts, T, sem, out + i * T);
  });
}

void check_targets_rank(int64_t M) {
  if (M < 1 || M > kMaxTopK) throw Error("rank: M must be in 1.." + std::to_string(kMaxTopK) + ", got " + std::to_string(M));
}

void targets_rank_batch_cpu(const ScoreTable& t, const uint8_t* s1, int64_t L1, const RecordBatch& batch,
                            const int64_t* starts, int64_t T, int M, RankRow* out, Semantics sem, int num_threads) {
  check_targets(starts, T, L1);
  check_targets_rank(M);
  for_each_profile(t, s1, L1, batch, sem, num_threads, [&](int64_t i, const ProfileEntry* prof, int64_t) {
    thread_local std::vector<Result> rows;   // the record's T pair rows: one record's at a time per thread
    thread_local std::vector<int32_t> order;  // its fitting targets, best first
    const int64_t L2 = batch.length(i);
    rows.resize(static_cast<size_t>(T));
    target_rows(t, s1, L1, batch.record(i), L2, prof, starts, T, sem, rows.data());
    order.clear();
    for (int64_t q = 0; q < T; ++q)
      if (L2 >= 1 && L2 <= starts[q + 1] - starts[q]) order.push_back(static_cast<int32_t>(q));
    const size_t keep = std::min(order.size(), static_cast<size_t>(M));
    // higher score, then smaller target index: a total order, so the partial sort is the stable sort's prefix
    std::partial_sort(order.begin(), order.begin() + static_cast<std::ptrdiff_t>(keep), order.end(), [&](int32_t a, int32_t b) {
      return rows[a].score != rows[b].score ? rows[a].score > rows[b].score : a < b;
    });
    RankRow* dst = out + i * M;
    for (size_t j = 0; j < static_cast<size_t>(M); ++j) {
      if (j < keep) {
        const Result& r = rows[order[j]];
        dst[j] = RankRow{order[j], r.score, r.n, r.k};
      } else {
        dst[j] = no_rank();
      }
    }
  });
}

int64_t targets_max_count(const int64_t* starts, int64_t T, const int64_t* offsets, int64_t n, Semantics sem) {
  int64_t max_len = 0;
  for (int64_t q = 0; q < T; ++q) max_len = std::max(max_len, starts[q + 1] - starts[q]);
  int64_t min_l2 = INT64_MAX;  // the shortest record that fits the longest target (and so any target at all)
  for (int64_t i = 0; i < n; ++i) {
    const int64_t L2 = offsets[i + 1] - offsets[i];
    if (L2 >= 1 && L2 <= max_len) min_l2 = std::min(min_l2, L2);
  }
  return min_l2 == INT64_MAX ? 0 : bounds::targets_pair_count(max_len, min_l2, sem == Semantics::Spec);
}

void targets_summary_batch_cpu(const ScoreTable& t, const uint8_t* s1, int64_t L1, const RecordBatch& batch,
                               const int64_t* starts, int64_t T, int64_t* summary, int32_t* hist, int32_t bins,
                               int32_t lo, int32_t width, Semantics sem, int num_threads) {
  check_targets(starts, T, L1);
  const int64_t n = batch.size();
  check_summary_args(t.max_abs(), n ? batch.max_length() : 0, targets_max_count(starts, T, batch.offsets.data(), n, sem),
                     bins, width);
  if (bins > 0 && !hist) throw Error("summary: bins > 0 need a hist buffer");
  for_each_profile(t, s1, L1, batch, sem, num_threads, [&](int64_t i, const ProfileEntry* prof, int64_t C) {
    const int64_t L2 = batch.length(i);
    const uint8_t* s2 = batch.record(i);
    for (int64_t q = 0; q < T; ++q) {
      const int64_t b = starts[q], len = starts[q + 1] - b;
      int64_t* row = summary + (i * T + q) * kSummaryCols;
      int32_t* h = bins > 0 ? hist + (i * T + q) * bins : nullptr;
      if (h) std::fill(h, h + bins, 0);
      int64_t count = 0, sum = 0, sumsq = 0, best = 0;
      int32_t mn = INT32_MAX, mx = INT32_MIN, bk = 0;
      auto take = [&](int32_t score, int64_t o, int32_t k) {
        const int64_t s = score;
        ++count;
        sum += s;
        sumsq += s * s;
        mn = std::min(mn, score);
        if (score > mx) {  // strict: the smallest offset keeps a tie
          mx = score;
          best = o;
          bk = k;
        }
        if (h) ++h[summary_bin(score, lo, width, bins)];
      };
      if (L2 >= 1 && L2 <= len) {
        const int64_t slice = len - L2;  // b + slice <= L1 - L2 <= C
        for (int64_t o = 0; o < slice; ++o) take(prof[b + o].score, o, prof[b + o].k);
        if (sem == Semantics::Spec || slice == 0) {  // the boundary entry, from the letters
          const uint8_t* a = s1 + b + slice;
          int32_t s = 0;
          for (int64_t l = 0; l < L2; ++l) s += t.lut[s2[l] * kLutStride + a[l]];
          take(s, slice, 0);
        }
      }
      row[0] = count;
      row[1] = sum;
      row[2] = sumsq;
      row[3] = mn;
      row[4] = mx;
      row[5] = best;
      row[6] = bk;
    }
    (void)C;
  });
}

namespace {
// Pair (record, target q)'s place in the record's catalog profile: fits, the slice's first catalog offset and
// entry count, and whether the boundary entry takes part (then its score, summed from the letters).
struct TargetPair {
  bool fits = false, boundary = false;
  int64_t b = 0, slice = 0;
  int32_t bscore = 0;
};
inline TargetPair target_pair(const ScoreTable& t, const uint8_t* s1, int64_t L1, const uint8_t* s2, int64_t L2,
                              const int64_t* starts, int64_t q, Semantics sem) {
  TargetPair p;
  p.b = starts[q];
  const int64_t len = starts[q + 1] - p.b;
  p.fits = L2 >= 1 && L2 <= len && L2 <= L1;
  if (!p.fits) return p;
  p.slice = len - L2;  // b + slice <= L1 - L2 <= C
  p.boundary = sem == Semantics::Spec || p.slice == 0;
  if (p.boundary) {
    const uint8_t* a = s1 + p.b + p.slice;
    for (int64_t l = 0; l < L2; ++l) p.bscore += t.lut[s2[l] * kLutStride + a[l]];
  }
  return p;
}
}  // namespace

namespace {
// Pair p's own profile (its slice of the catalog profile, then the boundary entry as an ordinary entry) and the peak
// marks of radius `radius` over exactly those entries: nothing outside the pair's [0, C_p) is ever in a window.
// Returns the marks, or null for radius == 0 (every entry counts).
inline const uint8_t* target_pair_peaks(const ProfileEntry* prof, const TargetPair& p, int64_t radius) {
  if (radius == 0 || !p.fits) return nullptr;
  thread_local std::vector<ProfileEntry> own;
  thread_local std::vector<uint8_t> peak;
  own.assign(prof + p.b, prof + p.b + p.slice);
  if (p.boundary) own.push_back(ProfileEntry{p.bscore, 0});
  peak.resize(own.size());
  peaks_filter(own.data(), static_cast<int64_t>(own.size()), radius, peak.data());
  return peak.data();
}
}  // namespace

void targets_topk_batch_cpu(const ScoreTable& t, const uint8_t* s1, int64_t L1, const RecordBatch& batch,
                            const int64_t* starts, int64_t T, int K, Result* out, Semantics sem, int num_threads,
                            int64_t radius) {
  check_targets(starts, T, L1);
  if (K < 1 || K > kMaxTopK) throw Error("top-K: K must be in 1.." + std::to_string(kMaxTopK));
  check_peaks_radius(radius);
  for_each_profile(t, s1, L1, batch, sem, num_threads, [&](int64_t i, const ProfileEntry* prof, int64_t C) {
    thread_local std::vector<uint64_t> keys;
    const int64_t L2 = batch.length(i);
    for (int64_t q = 0; q < T; ++q) {
      Result* row = out + (i * T + q) * K;
      const TargetPair p = target_pair(t, s1, L1, batch.record(i), L2, starts, q, sem);
      const uint8_t* peak = target_pair_peaks(prof, p, radius);
      keys.clear();
      for (int64_t o = 0; o < p.slice; ++o)
        if (!peak || peak[o]) keys.push_back(profile_key(prof[p.b + o], o));
      if (p.boundary && (!peak || peak[p.slice])) keys.push_back(profile_key(ProfileEntry{p.bscore, 0}, p.slice));
      const int64_t m = std::min<int64_t>(K, static_cast<int64_t>(keys.size()));
      std::partial_sort(keys.begin(), keys.begin() + m, keys.end(), std::greater<uint64_t>());
      for (int64_t j = 0; j < m; ++j) {
        const int64_t o = 0xffffffffu - static_cast<uint32_t>(keys[j]);
        row[j] = o < p.slice ? Result{prof[p.b + o].score, static_cast<int32_t>(o), prof[p.b + o].k}
                             : Result{p.bscore, static_cast<int32_t>(o), 0};
      }
      for (int64_t j = m; j < K; ++j) row[j] = no_candidate();
    }
    (void)C;
  });
}

void targets_hits_batch_cpu(const ScoreTable& t, const uint8_t* s1, int64_t L1, const RecordBatch& batch,
                            const int64_t* starts, int64_t T, int32_t min_score, const int32_t* thresholds,
                            int64_t* toffsets, Result* rows, int64_t cap, Semantics sem, int num_threads,
                            int64_t radius) {
  check_targets(starts, T, L1);
  if (cap < 0 || (cap > 0 && !rows)) throw Error("hits: cap rows need a rows buffer (cap = 0 counts only)");
  if (!toffsets) throw Error("hits: no hoffsets buffer");
  check_peaks_radius(radius);
  const int64_t n_pairs = batch.size() * T;
  auto threshold = [&](int64_t pair) { return thresholds ? thresholds[pair] : min_score; };
  // phase 1: counts into toffsets[pair + 1], then their running totals
  toffsets[0] = 0;
  for_each_profile(t, s1, L1, batch, sem, num_threads, [&](int64_t i, const ProfileEntry* prof, int64_t C) {
    const int64_t L2 = batch.length(i);
    for (int64_t q = 0; q < T; ++q) {
      const TargetPair p = target_pair(t, s1, L1, batch.record(i), L2, starts, q, sem);
      const uint8_t* peak = target_pair_peaks(prof, p, radius);
      const int32_t tp = threshold(i * T + q);
      int64_t c = 0;
      for (int64_t o = 0; o < p.slice; ++o) c += prof[p.b + o].score >= tp && (!peak || peak[o]) ? 1 : 0;
      if (p.boundary && p.bscore >= tp && (!peak || peak[p.slice])) ++c;
      toffsets[i * T + q + 1] = c;
    }
    (void)C;
  });
  for (int64_t pair = 0; pair < n_pairs; ++pair) toffsets[pair + 1] += toffsets[pair];
  if (cap == 0 || toffsets[n_pairs] == 0) return;
  // phase 2: fill, every row under the capacity contract
  for_each_profile(t, s1, L1, batch, sem, num_threads, [&](int64_t i, const ProfileEntry* prof, int64_t C) {
    if (toffsets[i * T] >= cap || toffsets[i * T] == toffsets[(i + 1) * T]) return;
    const int64_t L2 = batch.length(i);
    for (int64_t q = 0; q < T; ++q) {
      int64_t at = toffsets[i * T + q];
      if (at >= cap) return;
      if (at == toffsets[i * T + q + 1]) continue;
      const TargetPair p = target_pair(t, s1, L1, batch.record(i), L2, starts, q, sem);
      const uint8_t* peak = target_pair_peaks(prof, p, radius);
      const int32_t tp = threshold(i * T + q);
      for (int64_t o = 0; o < p.slice && at < cap; ++o) {
        const ProfileEntry& e = prof[p.b + o];
        if (e.score >= tp && (!peak || peak[o])) rows[at++] = Result{e.score, static_cast<int32_t>(o), e.k};
      }
      if (p.boundary && p.bscore >= tp && (!peak || peak[p.slice]) && at < cap)
        rows[at++] = Result{p.bscore, static_cast<int32_t>(p.slice), 0};
    }
    (void)C;
  });
}

void topk_batch_cpu(const ScoreTable& t, const uint8_t* s1, int64_t L1, const RecordBatch& batch, int K, Result* out,
                    Semantics sem, int num_threads, int64_t radius) {
  if (K < 1 || K > kMaxTopK) throw Error("top-K: K must be in 1.." + std::to_string(kMaxTopK));
  check_peaks_radius(radius);
  for_each_profile(t, s1, L1, batch, sem, num_threads, [&](int64_t i, const ProfileEntry* prof, int64_t C) {
    thread_local std::vector<uint64_t> keys;
    if (radius == 0) {
      select_topk(prof, C, K, out + i * K, keys);
      return;
    }
    thread_local std::vector<uint8_t> peak;
    peak.resize(static_cast<size_t>(C));
    peaks_filter(prof, C, radius, peak.data());
    keys.clear();
    for (int64_t o = 0; o < C; ++o)
      if (peak[o]) keys.push_back(profile_key(prof[o], o));
    const int64_t m = std::min<int64_t>(K, static_cast<int64_t>(keys.size()));
    std::partial_sort(keys.begin(), keys.begin() + m, keys.end(), std::greater<uint64_t>());
    Result* row = out + i * K;
    for (int64_t j = 0; j < m; ++j) {
      const int64_t o = 0xffffffffu - static_cast<uint32_t>(keys[j]);
      row[j] = Result{prof[o].score, static_cast<int32_t>(o), prof[o].k};
    }
    for (int64_t j = m; j < K; ++j) row[j] = no_candidate();
  });
}

void hits_batch_cpu(const ScoreTable& t, const uint8_t* s1, int64_t L1, const RecordBatch& batch, int32_t min_score,
                    const int32_t* thresholds, int64_t* hoffsets, Result* rows, int64_t cap, Semantics sem,
                    int num_threads, int64_t radius) {
  if (cap < 0 || (cap > 0 && !rows)) throw Error("hits: cap rows need a rows buffer (cap = 0 counts only)");
  check_peaks_radius(radius);
  const int64_t n = batch.size();
  auto threshold = [&](int64_t i) { return thresholds ? thresholds[i] : min_score; };
  // the record's peak marks (radius > 0), or null: every entry counts
  auto peaks_of = [&](const ProfileEntry* prof, int64_t C) -> const uint8_t* {
    if (radius == 0) return nullptr;
    thread_local std::vector<uint8_t> peak;
    peak.resize(static_cast<size_t>(C));
    peaks_filter(prof, C, radius, peak.data());
    return peak.data();
  };
  // phase 1: counts into hoffsets[i + 1], then their running totals
  hoffsets[0] = 0;
  for_each_profile(t, s1, L1, batch, sem, num_threads, [&](int64_t i, const ProfileEntry* prof, int64_t C) {
    const int32_t ti = threshold(i);
    const uint8_t* peak = peaks_of(prof, C);
    int64_t c = 0;
    for (int64_t o = 0; o < C; ++o) c += prof[o].score >= ti && (!peak || peak[o]) ? 1 : 0;
    hoffsets[i + 1] = c;
  });
  for (int64_t i = 0; i < n; ++i) hoffsets[i + 1] += hoffsets[i];
  if (cap == 0 || hoffsets[n] == 0) return;
  // phase 2: fill, every row under the capacity contract
  for_each_profile(t, s1, L1, batch, sem, num_threads, [&](int64_t i, const ProfileEntry* prof, int64_t C) {
    int64_t at = hoffsets[i];
    if (at >= cap || at == hoffsets[i + 1]) return;
    const int32_t ti = threshold(i);
    const uint8_t* peak = peaks_of(prof, C);
    for (int64_t o = 0; o < C && at < cap; ++o)
      if (prof[o].score >= ti && (!peak || peak[o])) rows[at++] = Result{prof[o].score, static_cast<int32_t>(o), prof[o].k};
  });
}

Result brute_force_record(const ScoreTable& t, const uint8_t* s1, int64_t L1, const uint8_t* s2, int64_t L2,
                          Semantics sem) {
  if (L2 > L1) return no_candidate();
  if (L2 == L1) {
    int32_t s = 0;
    for (int64_t i = 0; i < L2; ++i) s += t.lut[s2[i] * kLutStride + s1[i]];
    return Result{s, 0, 0};
  }
  Result best{kNoCandidateScore, 0, 0};
  bool have = false;
  for (int64_t o = 0; o < L1 - L2; ++o) {
    for (int64_t m = 0; m < L2; ++m) {
      int32_t s = 0;
      for (int64_t i = 0; i < L2; ++i) {
        const int64_t j = (i < m || m == 0) ? i + o : i + o + 1;
        s += t.lut[s2[i] * kLutStride + s1[j]];
      }
      if (!have || best.score < s) {
        best = Result{s, static_cast<int32_t>(o), static_cast<int32_t>(m)};
        have = true;
      }
    }
  }
  if (sem == Semantics::Spec) {
    int32_t s = 0;
    const int64_t o = L1 - L2;
    for (int64_t i = 0; i < L2; ++i) s += t.lut[s2[i] * kLutStride + s1[i + o]];
    if (!have || best.score < s) best = Result{s, static_cast<int32_t>(o), 0};
  }
  return best;
}

void report_batch_cpu(const ScoreTable& t, const uint8_t* s1, int64_t L1, const RecordBatch& batch, const Result* rows,
                      int K, int32_t* counts, uint8_t* marks, int num_threads) {
  if (K < 1 || K > kMaxTopK) throw Error("report: K must be in 1.." + std::to_string(kMaxTopK));
  const int64_t n = batch.size(), n_rows = n * K;
  const int nt = std::max(1, num_threads > 0 ? num_threads : omp_get_max_threads());
#pragma omp parallel for schedule(static) num_threads(nt) if (nt > 1 && n_rows > 256)
  for (int64_t q = 0; q < n_rows; ++q) {
    const int64_t i = q / K, j = q % K, L2 = batch.length(i);
    const Result r = rows[q];
    int32_t* c = counts + 4 * q;
    uint8_t* m = marks ? marks + K * (batch.offsets[i] - batch.offsets[0]) + j * L2 : nullptr;
    const bool empty = r.score == kNoCandidateScore;
    if (empty || !report_row_valid(L1, L2, r)) {
      c[0] = c[1] = c[2] = c[3] = empty ? 0 : -1;
      if (m) std::fill(m, m + std::max<int64_t>(L2, 0), uint8_t{0});
      continue;
    }
    const uint8_t* s2 = batch.record(i);
    int32_t cnt[4] = {0, 0, 0, 0};
    for (int64_t l = 0; l < L2; ++l) {
      const int64_t at = (r.k == 0 || l < r.k) ? r.n + l : r.n + l + 1;
      const uint8_t cl = t.cls[s2[l] * kLutStride + s1[at]];
      ++cnt[cl];
      if (m) m[l] = static_cast<uint8_t>(ScoreTable::class_char(static_cast<PairClass>(cl)));
    }
    c[0] = cnt[0], c[1] = cnt[1], c[2] = cnt[2], c[3] = cnt[3];
  }
}

Result resolve_key(const ScoreTable& t, const uint8_t* s1, int64_t L1, const uint8_t* s2, int64_t L2, uint64_t key) {
  if (key == 0) return no_candidate();
  const int32_t score = static_cast<int32_t>(static_cast<uint32_t>(key >> 32) ^ 0x80000000u);
  const uint32_t idx = 0xffffffffu - static_cast<uint32_t>(key);
  const int64_t o = idx >> 1;
  if (!(idx & 1u)) return Result{score, static_cast<int32_t>(o), 0};
  if (o + L2 >= L1) throw Error("resolve_key: a mutated candidate needs o + L2 < L1");
  // score = D_o(k) + Tot_{o+1}; the smallest k in 1..L2-1 with that value
  int64_t tot1 = 0;
  for (int64_t i = 0; i < L2; ++i) tot1 += t.score(s2[i], s1[o + 1 + i]);
  int64_t d = 0;
  for (int64_t k = 1; k < L2; ++k) {
    d += t.score(s2[k - 1], s1[o + k - 1]) - t.score(s2[k - 1], s1[o + k]);
    if (d + tot1 == score) return Result{score, static_cast<int32_t>(o), static_cast<int32_t>(k)};
  }
  throw Error("resolve_key: no k on diagonal " + std::to_string(o) + " reaches the key's score");
}

}  // namespace moc
