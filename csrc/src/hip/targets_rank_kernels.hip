// Target ranking: each record's M best targets out of its T pair rows (gfx950, wave64).
// Definitions: moc/cpu_engine.hpp targets_rank_batch_cpu; group sizes and cut-overs: moc/kernel_bounds.hpp
// (targets_rank_group).
//
// The kernel reads a chunk's pair rows where targets_select_kernel stored them just before on the same stream
// (pairs[li * T + t], li the record's index within the chunk: the part of the profile scratch behind the chunk's
// entries) and never the profile: a group owns a record, not a pair, and takes only the group maximum and the launch
// splitter from targets_pair.hpp. No atomics on global memory, no kernel waits on another block, no LDS; ordering is
// launch order.
//   targets_rank_kernel<G>  a group of G consecutive lanes (4, 16 or 64; aligned to G, so __shfl_xor steps below G
//                           stay inside it) owns record li of the chunk. M rounds (M is a kernel argument, so the trip
//                           count is uniform): every lane walks rows t = sub, sub + G, ... of the record, forms
//                           final_key(score, t) for a row whose score is not INT32_MIN (a pair that fits) and 0 for
//                           the others, and keeps the largest key strictly below the previous round's winner (the
//                           first round has no bound); a xor-shuffle group maximum; the group's first lane decodes t
//                           from the winner, re-reads that pair row's (n, k) and stores row j. t is part of the key,
//                           so a record's keys are distinct and "strictly below the last winner" removes exactly the
//                           rows already listed: higher score first, then smaller t. A round whose maximum is 0 has
//                           run out of fitting targets: it stores no_rank() and so does every later round, without
//                           walking the rows again. Every lane of a wave reaches every shuffle: groups without a
//                           record and groups out of keys carry 0.
#include <hip/hip_runtime.h>

#include "kernel_common.hpp"
#include "moc/kernel_bounds.hpp"
#include "moc/runtime/hip_check.hpp"
#include "targets_pair.hpp"

namespace moc {
namespace dev {

using namespace kc;
using namespace tp;

namespace {
constexpr int kBlock = bounds::kTargetsThreads;
}  // namespace

// records [rec_at, rec_at + gridDim.x * (kBlock / G)) of the chunk's view.n_rec
template <int G>
__global__ __launch_bounds__(256) void targets_rank_kernel(TargetsRankArgs ra, int64_t rec_at) {
  static_assert(G == 4 || G == 16 || G == 64, "targets rank: a group is 4, 16 or 64 lanes");
  constexpr int kGroupsPerBlock = kBlock / G;
  const int sub = threadIdx.x & (G - 1);
  const int64_t li = rec_at + static_cast<int64_t>(blockIdx.x) * kGroupsPerBlock + (threadIdx.x / G);
  const bool active = li < ra.view.n_rec;  // uniform over the group; an idle group still reaches every shuffle
  const int T = ra.T;
  const int64_t r = ra.view.rec0 + li;
  MOC_DCHECK(!active || (li >= 0 && r >= 0 && r < ra.view.n_total));
  const Result* rows = ra.pairs + (active ? li * T : 0);  // 64-bit: li * T
  bool live = active;  // the group may still have a fitting target that is not listed
  unsigned long long bound = 0ull;  // the previous round's winner (round 0 has none)
  for (int j = 0; j < ra.M; ++j) {
    unsigned long long key = 0ull;  // 0: no row (a real key is never 0: t < 2^31)
    if (live)
      for (int t = sub; t < T; t += G) {
        MOC_DCHECK(li * T + t >= 0 && li * T + t < ra.view.n_rec * static_cast<int64_t>(T));
        const int score = rows[t].score;
        const unsigned long long c = score != INT32_MIN ? final_key(score, static_cast<uint32_t>(t)) : 0ull;
        if (j == 0 || c < bound) key = max_u64(key, c);
      }
    // every lane of the wave reaches the shuffle (the loop above is the only divergent part)
    key = group_max_u64<G>(key);
    live = live && key != 0ull;
    bound = key;  // group-uniform; 0 from here on once the record is out of fitting targets
    if (active && sub == 0) {
      RankRow row{-1, INT32_MIN, 0, 0};
      if (key != 0ull) {
        const int t = static_cast<int>(0xffffffffu - static_cast<uint32_t>(key));
        MOC_DCHECK(t >= 0 && t < T);
        const Result w = rows[t];
        MOC_DCHECK(w.score == static_cast<int>(static_cast<uint32_t>(key >> 32) ^ 0x80000000u));
        row = RankRow{t, w.score, w.n, w.k};
      }
      const int64_t at = r * ra.M + j;  // 64-bit
      MOC_DCHECK(at >= 0 && at < ra.view.n_total * static_cast<int64_t>(ra.M));
      ra.out[at] = row;
    }
  }
}

void preload_targets_rank_kernels() {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&targets_rank_kernel<4>));
}

namespace {
template <int G>
void launch_targets_rank_g(const TargetsRankArgs& ra, hipStream_t stream) {
  for_each_launch<G>(ra.view.n_rec, [&](unsigned blocks, int64_t rec_at) {
    hipLaunchKernelGGL((targets_rank_kernel<G>), dim3(blocks), dim3(kBlock), 0, stream, ra, rec_at);
  });
}
}  // namespace

void launch_targets_rank(const TargetsRankArgs& ra, hipStream_t stream) {
  if (ra.view.n_rec <= 0 || ra.T <= 0 || ra.M <= 0) return;
  with_group(ra.group, [&](auto g) { launch_targets_rank_g<g()>(ra, stream); });
}

}  // namespace dev
}  // namespace moc
