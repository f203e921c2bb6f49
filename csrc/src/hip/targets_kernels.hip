// Multi-target search: every record's best alignment against each target of a catalog (gfx950, wave64).
// Definitions: moc/cpu_engine.hpp targets_batch_cpu; group sizes and cut-overs: moc/kernel_bounds.hpp.
//
// The kernel reads a chunk's catalog profile where hits_count_kernel reads it (prof[poffsets[r] - base + o], written
// by offset_profile_kernel just before on the same stream) and reduces, per (record, target) pair, the target's slice
// of it plus at most one un-mutated boundary diagonal to one row: the pair view of targets_pair.hpp, from which this
// kernel starts like the other per-target kernels (its group reductions and launch splitter too). No atomics on global
// memory, no kernel waits on another block, no LDS; ordering is launch order.
//   targets_select_kernel<G>  a group of G consecutive lanes (4, 16 or 64; aligned to G, so __shfl_xor steps below G
//                             stay inside it) owns pair p = li * T + t of the chunk (64-bit). The group strides over
//                             the slice's len_t - L2 entries keeping the largest order-free key (topk_select_kernel's
//                             final_key over the LOCAL offset, so the better() tie-break is top-K's), then — under the
//                             spec semantics or with len_t == L2 — over the record's L2 letters, summing
//                             LUT[s2[l]][Seq1[starts[t] + len_t - L2 + l]]; xor-shuffle reductions; the group's first
//                             lane re-reads the winning entry's k, merges the boundary entry (it has the largest
//                             offset: it wins only with a strictly higher score) and stores the row at
//                             out[(r - out_rec0) * T + t] — the batch's rows, or (the target ranking) the chunk's
//                             alone in the profile scratch behind the chunk's entries. Every lane of a
//                             wave reaches every shuffle: groups without a pair or with an empty slice carry key 0.
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

// pairs [pair0, pair0 + gridDim.x * (kBlock / G)) of the chunk's n_pairs = n_rec * T
template <int G>
__global__ __launch_bounds__(256) void targets_select_kernel(TargetsArgs ta, ProblemView pv, BatchView bv, int64_t pair0,
                                                             int64_t n_pairs) {
  static_assert(G == 4 || G == 16 || G == 64, "targets: a group is 4, 16 or 64 lanes");
  constexpr int kGroupsPerBlock = kBlock / G;
  const int sub = threadIdx.x & (G - 1);
  // an idle group (no pair: uniform over the group) still reaches every shuffle
  const Pair p = pair_of(ta, pv, bv, pair0 + static_cast<int64_t>(blockIdx.x) * kGroupsPerBlock + (threadIdx.x / G), n_pairs);
  unsigned long long key = 0ull;  // 0: no entry (a real key is never 0: o < 2^31)
  for (int o = sub; o < p.slice; o += G) key = max_u64(key, final_key(slice_entry(ta, p, o).score, static_cast<uint32_t>(o)));
  int bsum = boundary_part(p, pv, sub, G);
  // every lane of the wave reaches the shuffles (the two loops above are the only divergent parts)
  key = group_max_u64<G>(key);
  bsum = group_sum_i32<G>(bsum);
  if (p.active && sub == 0) {
    Result row{INT32_MIN, 0, 0};
    if (key != 0ull) {
      const int o = static_cast<int>(0xffffffffu - static_cast<uint32_t>(key));
      const ProfileEntry e = slice_entry(ta, p, o);
      row = Result{e.score, o, e.k};
    }
    if (p.boundary && (key == 0ull || bsum > row.score)) row = Result{bsum, p.slice, 0};
    const int64_t at = (p.r - ta.out_rec0) * ta.T + p.t;  // 64-bit; out_rec0 is 0 or the chunk's first record
    MOC_DCHECK(at >= 0 && at < (ta.out_rec0 ? ta.view.n_rec : ta.view.n_total) * ta.T);
    ta.out[at] = row;
  }
}

void preload_targets_kernels() {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&targets_select_kernel<4>));
}

namespace {
template <int G>
void launch_targets_g(const TargetsArgs& ta, const ProblemView& pv, const BatchView& bv, hipStream_t stream) {
  const int64_t n_pairs = ta.view.n_rec * ta.T;
  for_each_launch<G>(n_pairs, [&](unsigned blocks, int64_t pair0) {
    hipLaunchKernelGGL((targets_select_kernel<G>), dim3(blocks), dim3(kBlock), 0, stream, ta, pv, bv, pair0, n_pairs);
  });
}
}  // namespace

void launch_targets(const TargetsArgs& ta, const ProblemView& pv, const BatchView& bv, hipStream_t stream) {
  if (ta.view.n_rec <= 0 || ta.T <= 0) return;
  with_group(ta.group, [&](auto g) { launch_targets_g<g()>(ta, pv, bv, stream); });
}

}  // namespace dev
}  // namespace moc
