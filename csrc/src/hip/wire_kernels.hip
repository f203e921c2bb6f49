// Wire-format decode on the device (gfx950, wave64): what ./final's parser writes and the RCCL transport
// delivers — P33 letter fields, narrow record lengths, sparse offsets (moc/wire.hpp) — into the one byte per
// letter and dense int64 offsets the profile / top-K / hits / report kernels read. Host reference:
// moc::decode_wire_cpu. Every source may be device memory or page-locked host memory read in place.
//
// Reference: the letters travel as bytes in a fixed 2000-byte stride per record (main.c:93,174), so there is no
// decode step at all — and 2000 / mean(L2) times the bytes.
//
//   * wire_offsets_kernel: wave w owns records [64w, 64w + 64). 64 is a multiple of every legal sparse stride
//     2^shift, so the wave's first record has a sparse entry; each lane decodes its own record's length (8-bit,
//     nibble, 3-bit field straddling a byte, or base-6 digit i % 8 of octet i / 8, three octets per aligned
//     8-byte word), a wave scan gives the exclusive sums, and the last wave also stores the batch end. Waves
//     are independent: no atomics, no spinning, ordering is launch order.
//   * unpack33_kernel: a block decodes 256 consecutive fields (1792 letters) into LDS, one field per lane with
//     the digit arithmetic of the swipe kernel's decode_p33_field (restated here in plain C++), then stores the
//     block's part of out[0 .. c1 - c0) as aligned dwords with single bytes at the two ends. A lane loads the two
//     aligned dwords around its field's 5 bytes when both lie inside the batch's byte range
//     [p33_first_byte(c0), p33_end_byte(c1)) and the field's bytes one by one otherwise (the first and last
//     dword of the range: a pinned host window may end there).
#include "moc/device.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "kernel_common.hpp"
#include "moc/problem.hpp"
#include "moc/runtime/hip_check.hpp"

namespace moc {
namespace dev {

namespace {
constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kFieldsPerBlock = kBlock;                        // one P33 field per lane
constexpr int kLettersPerBlock = kP33Field * kFieldsPerBlock;  // 1792

// Length of record i above nothing (base included), i < a.n.
__device__ __forceinline__ int32_t wire_length(const WireOffsetsArgs& a, int64_t i) {
  if (a.bits == 8) {
    MOC_DCHECK(i < a.lengths_bytes);
    return a.lengths[i];
  }
  if (a.bits == 4) {
    MOC_DCHECK((i >> 1) < a.lengths_bytes);
    return static_cast<int32_t>(a.base) + ((a.lengths[i >> 1] >> (4 * (i & 1))) & 15);
  }
  if (a.bits == 3) {
    const int64_t bit = 3 * i, b = bit >> 3;
    MOC_DCHECK(b + 1 < a.lengths_bytes);  // the slack byte of narrow_lengths_bytes(n, 3)
    const uint32_t w = a.lengths[b] | (static_cast<uint32_t>(a.lengths[b + 1]) << 8);
    return static_cast<int32_t>(a.base) + ((w >> (bit & 7)) & 7);
  }
  // base 6: word i / 24, octet (i / 8) % 3 at bits [21f, 21f + 21), digit i % 8
  const int64_t word = i / 24;
  MOC_DCHECK(8 * word + 8 <= a.lengths_bytes);
  const uint64_t w = *reinterpret_cast<const uint64_t*>(a.lengths + 8 * word);
  uint32_t v = static_cast<uint32_t>(w >> (21 * static_cast<int>((i >> 3) % 3))) & 0x1FFFFFu;
  const int d = static_cast<int>(i & 7);
  if (d & 4) v /= 1296u;
  if (d & 2) v /= 36u;
  if (d & 1) v /= 6u;
  return static_cast<int32_t>(a.base) + static_cast<int32_t>(v % 6u);
}

__global__ __launch_bounds__(kBlock) void wire_offsets_kernel(const WireOffsetsArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t w = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t r0 = w * kWave;
  if (r0 >= a.n && !(a.n == 0 && w == 0)) return;  // wave-uniform
  const int64_t i = r0 + lane;
  const int32_t len = i < a.n ? wire_length(a, i) : 0;
  int32_t incl = len;  // <= 64 * 255
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const int32_t up = __shfl_up(incl, d, kWave);
    if (lane >= d) incl += up;
  }
  MOC_DCHECK((r0 >> a.shift) < a.sparse_entries);
  const int64_t base = a.sparse[r0 >> a.shift];
  if (i < a.n) a.dense[i] = base + (incl - len);
  if (r0 + kWave >= a.n && lane == 0) {  // the last wave: the batch end
    const int64_t last = ((a.n + (int64_t{1} << a.shift) - 1) >> a.shift);
    MOC_DCHECK(last < a.sparse_entries);
    a.dense[a.n] = a.sparse[last];
  }
}

// 33-bit field value -> its seven letter codes (digit + 1) as bytes 0..6 of (lo, hi); byte 7 is 0. The arithmetic
// of decode_p33_field (swipe_impl.hpp): digits 4..6 = x / 26^4 by a multiply-high on x >> 4, pairs of digits by
// v / 676 as a multiply-high, a pair's two digits by (v * 2521) >> 16 = v / 26 for v < 676.
__device__ __forceinline__ uint32_t p33_pair_bytes(uint32_t v) {  // v < 676 -> bytes (v % 26, v / 26)
  const uint32_t q = (v * 2521u) >> 16;
  return (v - 26u * q) | (q << 8);
}
__device__ __forceinline__ uint2 p33_letters(uint64_t x) {
  const uint32_t A = __umulhi(static_cast<uint32_t>(x >> 4), 2463805336u) >> 14;  // digits 4..6 (< 26^3)
  const uint32_t B = static_cast<uint32_t>(x) - A * 456976u;                     // digits 0..3 (< 26^4)
  const uint32_t b32 = __umulhi(B, 6353502u), a2 = __umulhi(A, 6353502u);         // / 676 for values < 2^24
  const uint32_t b10 = B - b32 * 676u, a10 = A - a2 * 676u;
  return make_uint2((p33_pair_bytes(b10) | (p33_pair_bytes(b32) << 16)) + 0x01010101u,
                    (p33_pair_bytes(a10) | (a2 << 16)) + 0x00010101u);
}

__global__ __launch_bounds__(kBlock) void unpack33_kernel(const Unpack33Args a) {
  __shared__ __attribute__((aligned(8))) uint8_t letters[8 * kFieldsPerBlock];  // field t at 8t: 7 letters + pad
  const int tid = threadIdx.x;
  const int64_t f0 = a.c0 / kP33Field, f1 = (a.c1 + kP33Field - 1) / kP33Field;
  const int64_t fb = f0 + static_cast<int64_t>(blockIdx.x) * kFieldsPerBlock;  // the block's first field
  const int64_t f = fb + tid;
  const int64_t first_byte = (33 * f0) >> 3;  // p33_first_byte(c0): a.src points here
  if (f < f1) {
    const int64_t bit = 33 * f;
    const int64_t at = (bit >> 3) - first_byte;  // the field's 5 bytes: src[at .. at + 5)
    MOC_DCHECK(at >= 0 && at + 5 <= a.src_bytes);
    const uintptr_t p = reinterpret_cast<uintptr_t>(a.src) + static_cast<uintptr_t>(at);
    const int64_t lo_at = at - static_cast<int64_t>(p & 3);  // of the aligned dword holding the first byte
    uint64_t ww;
    int sh;
    if (lo_at >= 0 && lo_at + 8 <= a.src_bytes) {
      const uint32_t* q = reinterpret_cast<const uint32_t*>(a.src + lo_at);
      ww = static_cast<uint64_t>(q[0]) | (static_cast<uint64_t>(q[1]) << 32);
      sh = 8 * static_cast<int>(p & 3) + static_cast<int>(bit & 7);  // <= 31
    } else {
      ww = 0;
#pragma unroll
      for (int j = 0; j < 5; ++j) ww |= static_cast<uint64_t>(a.src[at + j]) << (8 * j);
      sh = static_cast<int>(bit & 7);
    }
    const uint2 v = p33_letters((ww >> sh) & 0x1FFFFFFFFull);
    *reinterpret_cast<uint2*>(letters + 8 * tid) = v;
  }
  __syncthreads();
  // the block's letters [l0, l1) of the stream -> out[l0 - c0 .. l1 - c0)
  const int64_t l0 = std::max(a.c0, kP33Field * fb), l1 = std::min(a.c1, kP33Field * (fb + kFieldsPerBlock));
  if (l1 <= l0) return;
  const int64_t total = a.c1 - a.c0;
  const int nl = static_cast<int>(l1 - l0);
  const int s0 = static_cast<int>(l0 - kP33Field * fb);  // letter index within the block of the first one stored
  uint8_t* dst = a.out + (l0 - a.c0);
  auto letter = [&](int s) { return letters[8 * (s / kP33Field) + s % kP33Field]; };  // s: letter index in the block
  const int head = std::min<int>(nl, static_cast<int>((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3));
  const int nd = (nl - head) >> 2, tail0 = head + 4 * nd;
  MOC_DCHECK(l0 - a.c0 >= 0 && l0 - a.c0 + nl <= total && s0 >= 0 && s0 + nl <= kLettersPerBlock);
  (void)total;
  if (tid < head) dst[tid] = letter(s0 + tid);
  for (int i = tid; i < nd; i += kBlock) {
    const int s = s0 + head + 4 * i;
    const uint32_t v = letter(s) | (static_cast<uint32_t>(letter(s + 1)) << 8) |
                       (static_cast<uint32_t>(letter(s + 2)) << 16) | (static_cast<uint32_t>(letter(s + 3)) << 24);
    *reinterpret_cast<uint32_t*>(dst + head + 4 * i) = v;
  }
  if (tid < nl - tail0) dst[tail0 + tid] = letter(s0 + tail0 + tid);
}
}  // namespace

void preload_wire_kernels() {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&unpack33_kernel));
}

void launch_wire_offsets(const WireOffsetsArgs& a, hipStream_t stream) {
  if (a.n < 0) return;
  if (a.shift < 0 || a.shift > 6) throw Error("wire offsets: shift 0..6");
  if (a.bits != 8 && a.bits != 4 && a.bits != 3 && a.bits != kLenBase6) throw Error("wire offsets: lengths must be 8-, 4-, 3-bit or base-6");
  if (a.bits == kLenBase6 && (reinterpret_cast<uintptr_t>(a.lengths) & 7)) throw Error("wire offsets: base-6 lengths must be 8-byte aligned");
  const int64_t waves = std::max<int64_t>(1, (a.n + kWave - 1) / kWave);
  const int64_t blocks = (waves + kWavesPerBlock - 1) / kWavesPerBlock;
  hipLaunchKernelGGL(wire_offsets_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, stream, a);
}

void launch_unpack33(const Unpack33Args& a, hipStream_t stream) {
  if (a.c1 <= a.c0) return;
  if (a.c0 < 0) throw Error("unpack33: negative letter offset");
  const int64_t fields = (a.c1 + kP33Field - 1) / kP33Field - a.c0 / kP33Field;
  const int64_t blocks = (fields + kFieldsPerBlock - 1) / kFieldsPerBlock;
  if (blocks >= (int64_t{1} << 31)) throw Error("unpack33: more than 2^31 blocks of 1792 letters in one launch");
  hipLaunchKernelGGL(unpack33_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, stream, a);
}

}  // namespace dev
}  // namespace moc
