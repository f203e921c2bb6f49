// Stand-alone sanitizer check of the host code that carries 64-bit letter offsets, at positions past 2^31 and 2^32:
// built with -fsanitize=address,undefined (signed overflow included) together with the CPU core sources (make far-san)
// and run as a plain program. It works on an anonymous mapping laid out as the far-offset tests' arena (2^31 guard
// bytes, then a view of 2^32 + 2^24 bytes; only the pages a case writes are ever touched). P33 and 5-bit runs are
// written bit by bit where the stream's bit position, its byte position or the letter index lies just past 2^31 or
// 2^32, at several phases; byte letters where the first offset has bit 31 or a high word set and where a batch lies
// across 2^32. unpack33, unpack5, p33_first_byte / p33_end_byte, expand_offsets, wire_dense_offsets, decode_wire_cpu
// and staged_chunks are compared with plain per-bit, per-record code written here in 128-bit arithmetic.
// Exit status 0 = all equal and no sanitizer report.
#include <sys/mman.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "moc/problem.hpp"
#include "moc/tile_plan.hpp"
#include "moc/wire.hpp"

namespace {

using i128 = __int128;
constexpr int64_t kFront = int64_t{1} << 31;
constexpr int64_t kView = (int64_t{1} << 32) + (int64_t{1} << 24);

int failures = 0;
int64_t checked = 0;
uint8_t* view = nullptr;

uint32_t rng_state = 77u;
uint32_t rnd(uint32_t m) {
  rng_state = rng_state * 1664525u + 1013904223u;
  return (rng_state >> 8) % m;
}

void fail(const char* what, const char* form, int64_t c0) {
  std::fprintf(stderr, "far_offsets_san: %s (%s, first letter %lld)\n", what, form, static_cast<long long>(c0));
  ++failures;
}

// bit `bit` of the view's little-endian bit stream, 128-bit position arithmetic
void put_bits(i128 bit, uint64_t v, int nbits) {
  for (int j = 0; j < nbits; ++j, ++bit) {
    uint8_t& b = view[static_cast<int64_t>(bit >> 3)];
    const uint8_t m = static_cast<uint8_t>(1u << static_cast<int>(bit & 7));
    b = ((v >> j) & 1) ? (b | m) : (b & ~m);
  }
}
void clear_bits(i128 bit, i128 nbits) {
  const int64_t b0 = static_cast<int64_t>(bit >> 3), b1 = static_cast<int64_t>((bit + nbits + 7) >> 3);
  std::memset(view + b0, 0, static_cast<size_t>(b1 - b0));
}

struct Records {
  std::vector<uint8_t> letters;   // the records' letters
  std::vector<int64_t> offsets;   // from 0
  std::vector<uint8_t> lengths6;  // base-6 lengths above 6
  int64_t n = 0;
};

Records make_records(int64_t n) {
  Records r;
  r.n = n;
  r.offsets.assign(static_cast<size_t>(n) + 1, 0);
  for (int64_t i = 0; i < n; ++i) r.offsets[i + 1] = r.offsets[i] + 6 + rnd(6);
  r.letters.resize(static_cast<size_t>(r.offsets[n]));
  for (auto& c : r.letters) c = static_cast<uint8_t>(1 + rnd(26));
  r.lengths6.resize(static_cast<size_t>(moc::narrow_lengths_bytes(n, moc::kLenBase6)));
  moc::pack_lengths(r.offsets.data(), n, moc::kLenBase6, 6, r.lengths6.data());
  return r;
}

// decode_wire_cpu, wire_dense_offsets and expand_offsets of the batch at first letter c0, dense and 64-record sparse
void check_batch(const Records& r, int letter_form, int64_t c0, const char* form) {
  const int64_t n = r.n, total = r.offsets[n];
  for (int shift : {0, 6}) {
    const int64_t entries = shift ? moc::sparse_count(n, shift) : n + 1;
    std::vector<int64_t> woff(static_cast<size_t>(entries));
    for (int64_t j = 0; j < entries; ++j) woff[j] = c0 + r.offsets[shift ? std::min(j << shift, n) : j];
    moc::WireBatch b;
    b.letters = view;
    b.packed5 = letter_form == 1;
    b.packed33 = letter_form == 3;
    b.offsets = woff.data();
    b.off_shift = shift;
    b.lengths = r.lengths6.data();
    b.len_bits = moc::kLenBase6;
    b.len_base = 6;
    b.n = n;
    const moc::WireDecodedBytes sz = moc::wire_decoded_bytes(b);
    if (sz.codes != total || sz.offsets != 8 * (n + 1) || b.first_letter() != c0 || b.end_letter() != c0 + total) {
      fail("wire_decoded_bytes", form, c0);
      continue;
    }
    i128 want_bytes = total;
    if (letter_form == 3) want_bytes = ((i128{33} * ((i128{c0} + total + 6) / 7) + 7) >> 3) - ((i128{33} * (c0 / 7)) >> 3);
    if (letter_form == 1) want_bytes = (i128{5} * total + 7) / 8;
    if (b.letter_bytes() != static_cast<int64_t>(want_bytes)) fail("letter_bytes", form, c0);
    std::vector<uint8_t> codes(static_cast<size_t>(total) + 1, 0xEE);
    std::vector<int64_t> dense(static_cast<size_t>(n) + 2, -7), dense2(static_cast<size_t>(n) + 2, -7);
    moc::decode_wire_cpu(b, codes.data(), dense.data());
    moc::wire_dense_offsets(b, dense2.data());
    bool ok = codes[total] == 0xEE && dense[n + 1] == -7 && dense2[n + 1] == -7;
    ok = ok && std::equal(r.letters.begin(), r.letters.end(), codes.begin());
    for (int64_t i = 0; i <= n; ++i) ok = ok && dense[i] == c0 + r.offsets[i] && dense2[i] == dense[i];
    if (shift) {
      std::vector<int64_t> dense3(static_cast<size_t>(n) + 1, -7);
      moc::expand_offsets(woff.data(), shift, r.lengths6.data(), moc::kLenBase6, 6, n, dense3.data());
      for (int64_t i = 0; i <= n; ++i) ok = ok && dense3[i] == dense[i];
    }
    checked += n + total;
    if (!ok) fail(shift ? "decode differs (sparse offsets)" : "decode differs (dense offsets)", form, c0);
  }
}

void p33_case(const Records& r, int64_t f0, int ph, const char* form) {
  const int64_t c0 = 7 * f0 + ph, total = r.offsets[r.n];
  const int64_t fields = (ph + total + 6) / 7;
  std::vector<uint8_t> laid(static_cast<size_t>(7 * fields), 1);
  for (int j = 0; j < ph; ++j) laid[j] = static_cast<uint8_t>(1 + rnd(26));  // the neighbours sharing the first field
  std::copy(r.letters.begin(), r.letters.end(), laid.begin() + ph);
  for (int64_t f = 0; f < fields; ++f) put_bits(i128{33} * (f0 + f), moc::p33_field(&laid[7 * f]), 33);
  const i128 first = (i128{33} * f0) >> 3, end = (i128{33} * ((i128{c0} + total + 6) / 7) + 7) >> 3;
  if (moc::p33_first_byte(c0) != static_cast<int64_t>(first) || moc::p33_end_byte(c0 + total) != static_cast<int64_t>(end))
    fail("p33_first_byte / p33_end_byte", form, c0);
  std::vector<uint8_t> out(static_cast<size_t>(total) + 1, 0xEE);
  moc::unpack33(view, c0, total, out.data());
  if (out[total] != 0xEE || !std::equal(r.letters.begin(), r.letters.end(), out.begin())) fail("unpack33", form, c0);
  check_batch(r, 3, c0, form);
  clear_bits(i128{33} * f0, i128{33} * fields);
}

void p5_case(const Records& r, int64_t c0, const char* form) {
  const int64_t total = r.offsets[r.n];
  for (int64_t x = 0; x < total; ++x) put_bits(i128{5} * (c0 + x), r.letters[x], 5);
  std::vector<uint8_t> out(static_cast<size_t>(total) + 1, 0xEE);
  moc::unpack5(view, c0, total, out.data());
  if (out[total] != 0xEE || !std::equal(r.letters.begin(), r.letters.end(), out.begin())) fail("unpack5", form, c0);
  check_batch(r, 1, c0, form);
  clear_bits(i128{5} * c0, i128{5} * total);
}

void bytes_case(const Records& r, int64_t c0, const char* form) {
  std::memcpy(view + c0, r.letters.data(), r.letters.size());
  check_batch(r, 0, c0, form);
  std::memset(view + c0, 0, r.letters.size());
}

// staged_chunks on absolute offsets against the rule as a plain loop in 128-bit arithmetic
void chunks_case(const Records& r, int64_t c0, int64_t R, int64_t B) {
  const int64_t n = r.n;
  std::vector<int64_t> off(static_cast<size_t>(n) + 1);
  for (int64_t i = 0; i <= n; ++i) off[i] = c0 + r.offsets[i];
  std::vector<int64_t> got(static_cast<size_t>(n) + 1, -7), want{0};
  const int64_t chunks = moc::plan::staged_chunks(off.data(), n, R, B, got.data());
  for (int64_t rb = 0; rb < n;) {
    int64_t re = rb + 1;
    while (re < n && (re + 1) - rb <= R && i128{off[re + 1]} - off[rb] <= B) ++re;
    want.push_back(re);
    rb = re;
  }
  bool ok = chunks == static_cast<int64_t>(want.size()) - 1;
  for (int64_t i = 0; ok && i <= chunks; ++i) {
    ok = got[i] == want[i];
    if (i < chunks) ok = ok && moc::plan::staged_chunk_end(off.data(), n, want[i], R, B) == want[i + 1];
  }
  checked += n;
  if (!ok) fail("staged_chunks", "bytes", c0);
}

}  // namespace

int main() {
  void* arena = mmap(nullptr, static_cast<size_t>(kFront + kView), PROT_READ | PROT_WRITE,
                     MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
  if (arena == MAP_FAILED) {
    std::perror("far_offsets_san: mmap");
    return 2;
  }
  view = static_cast<uint8_t*>(arena) + kFront;
  const Records r = make_records(200);  // four sparse entries and the end
  const int64_t total = r.offsets[r.n];
  for (int k : {31, 32}) {
    const i128 two = i128{1} << k, bits = i128{1} << (k + 3);
    // P33: the field's bit position, its byte position and the letter index just past 2^k
    const int64_t f33[3] = {static_cast<int64_t>(two / 33 + 1), static_cast<int64_t>((bits + 32) / 33),
                            static_cast<int64_t>((two + 6) / 7)};
    for (int64_t f0 : f33)
      for (int ph : {0, 3, 6}) p33_case(r, f0, ph, k == 31 ? "p33 past 2^31" : "p33 past 2^32");
    // 5-bit: the same three, at every letter index mod 8
    const int64_t c5[3] = {static_cast<int64_t>(two / 5 + 1), static_cast<int64_t>((bits + 4) / 5), static_cast<int64_t>(two)};
    for (int64_t lo : c5)
      for (int ph = 0; ph < 8; ++ph) p5_case(r, lo + ((ph - lo) % 8 + 8) % 8, k == 31 ? "5-bit past 2^31" : "5-bit past 2^32");
    // byte letters: bit k set, and the batch across 2^k (between two records and inside one)
    const int64_t mid = r.offsets[r.n / 2];
    for (int64_t c0 : {static_cast<int64_t>(two) + 45, static_cast<int64_t>(two) - mid, static_cast<int64_t>(two) - mid - 3}) {
      bytes_case(r, c0, k == 31 ? "bytes at 2^31" : "bytes at 2^32");
      for (int64_t R : {int64_t{7}, int64_t{64}, int64_t{1} << 21})
        for (int64_t B : {int64_t{50}, total / 3, int64_t{64} << 20}) chunks_case(r, c0, R, B);
    }
  }
  munmap(arena, static_cast<size_t>(kFront + kView));
  if (failures) {
    std::fprintf(stderr, "far_offsets_san: %d failures\n", failures);
    return 1;
  }
  std::printf("far_offsets_san ok: %lld records and letters checked\n", static_cast<long long>(checked));
  return 0;
}
