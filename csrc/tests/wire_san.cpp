// Stand-alone sanitizer check of the host wire decode: built with -fsanitize=address,undefined together with the CPU
// core sources (make wire-san) and run as a plain program. decode_wire_cpu over every letter form x length form x
// sparse shift, on batches that start 0, 1, 6 and 57 letters into a longer stream, with the wire arrays and the two
// outputs in heap blocks of exactly their sizes (the letters: the byte range the kernels treat as the batch's; the
// outputs: wire_decoded_bytes), so a load or store outside them is an ASan report. The expected letters and
// offsets come from a plain per-letter, per-record decode written here. Every validation error must throw.
// Exit status 0 = all equal and no sanitizer report.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "moc/problem.hpp"
#include "moc/wire.hpp"

namespace {

int failures = 0;
int64_t checked = 0;

uint32_t rng_state = 2024u;
uint32_t rnd(uint32_t m) {
  rng_state = rng_state * 1664525u + 1013904223u;
  return (rng_state >> 8) % m;
}

std::unique_ptr<uint8_t[]> block(const uint8_t* src, int64_t b0, int64_t b1) {  // exactly the bytes [b0, b1) of src
  std::unique_ptr<uint8_t[]> p(new uint8_t[static_cast<size_t>(b1 - b0)]);
  if (b1 > b0) std::memcpy(p.get(), src + b0, static_cast<size_t>(b1 - b0));
  return p;
}

// plain decoders of the wire forms, one letter / one record at a time
uint8_t letter33(const uint8_t* p, int64_t x) {
  const int64_t f = x / 7;
  unsigned __int128 v = 0;
  for (int j = 0; j < 33; ++j) {
    const int64_t bit = 33 * f + j;
    v |= static_cast<unsigned __int128>((p[bit >> 3] >> (bit & 7)) & 1) << j;
  }
  uint64_t d = static_cast<uint64_t>(v);
  for (int64_t j = x % 7; j > 0; --j) d /= 26;
  return static_cast<uint8_t>(d % 26 + 1);
}
uint8_t letter5(const uint8_t* p, int64_t x) {
  unsigned v = 0;
  for (int j = 0; j < 5; ++j) {
    const int64_t bit = 5 * x + j;
    v |= static_cast<unsigned>((p[bit >> 3] >> (bit & 7)) & 1) << j;
  }
  return static_cast<uint8_t>(v);
}
int64_t length_of(const uint8_t* p, int bits, int64_t base, int64_t i) {
  if (bits == 8) return p[i];
  if (bits == moc::kLenBase6) {
    uint64_t w = 0;
    for (int j = 0; j < 8; ++j) w |= static_cast<uint64_t>(p[8 * (i / 24) + j]) << (8 * j);
    uint64_t v = (w >> (21 * ((i / 8) % 3))) & 0x1FFFFF;
    for (int64_t j = i % 8; j > 0; --j) v /= 6;
    return base + static_cast<int64_t>(v % 6);
  }
  int64_t v = 0;
  for (int j = 0; j < bits; ++j) {
    const int64_t bit = bits * i + j;
    v |= static_cast<int64_t>((p[bit >> 3] >> (bit & 7)) & 1) << j;
  }
  return base + v;
}

void run(int letter_form /* 0 bytes, 1 p5, 3 p33 */, int bits /* 0: none */, int shift, int64_t n, int64_t c0) {
  // ---- the records and the stream around them
  const int64_t base = bits == 8 || bits == 0 ? 0 : 5;
  const int64_t span = bits == moc::kLenBase6 ? 6 : bits == 3 ? 8 : bits == 4 ? 16 : 41;
  std::vector<int64_t> offsets(static_cast<size_t>(n) + 1);
  offsets[0] = c0;
  for (int64_t i = 0; i < n; ++i) {
    int64_t L = base + rnd(static_cast<uint32_t>(span));
    if (bits == 8 && i == n / 2) L = 255;
    if (bits == 0 && i == n / 2) L = 300;
    offsets[i + 1] = offsets[i] + L;
  }
  const int64_t c1 = offsets[n], T = c1 + 9;  // letters after the batch too
  std::vector<uint8_t> stream(static_cast<size_t>(T));
  for (auto& c : stream) c = static_cast<uint8_t>(1 + rnd(26));
  if (letter_form == 3 && c1 > c0) stream[c0] = 0;  // packs as 1
  // ---- wire arrays in exact heap blocks
  std::unique_ptr<uint8_t[]> letters;
  int64_t lb0 = c0;
  if (letter_form == 3) {
    std::vector<uint8_t> p(static_cast<size_t>(moc::packed33_bytes(T)));
    moc::pack33(stream.data(), T, p.data());
    lb0 = moc::p33_first_byte(c0);
    letters = block(p.data(), lb0, moc::p33_end_byte(c1));
  } else if (letter_form == 1) {
    std::vector<uint8_t> p(static_cast<size_t>(moc::packed5_bytes(T)));
    moc::pack5(stream.data(), T, p.data());
    lb0 = (5 * c0) >> 3;
    letters = block(p.data(), lb0, ((5 * c1 + 7) >> 3) + 1);  // + the byte unpack5 loads after the last letter's
  } else {
    letters = block(stream.data(), c0, c1);
  }
  std::unique_ptr<uint8_t[]> lengths;
  if (bits) {
    lengths.reset(new uint8_t[static_cast<size_t>(moc::narrow_lengths_bytes(n, bits))]);
    moc::pack_lengths(offsets.data(), n, bits, base, lengths.get());
  }
  const int64_t entries = shift ? moc::sparse_count(n, shift) : n + 1;
  std::unique_ptr<int64_t[]> woff(new int64_t[static_cast<size_t>(entries)]);
  for (int64_t j = 0; j < entries; ++j) woff[j] = offsets[shift ? std::min(j << shift, n) : j];
  moc::WireBatch b;
  b.letters = letters.get() - lb0;
  b.packed5 = letter_form == 1;
  b.packed33 = letter_form == 3;
  b.offsets = woff.get();
  b.off_shift = shift;
  b.lengths = lengths.get();
  b.len_bits = bits ? bits : 8;
  b.len_base = base;
  b.n = n;
  // ---- decode into exact heap blocks
  const moc::WireDecodedBytes sz = moc::wire_decoded_bytes(b);
  if (sz.codes != c1 - c0 || sz.offsets != 8 * (n + 1)) {
    std::fprintf(stderr, "wire_san: wire_decoded_bytes (form %d bits %d shift %d n %lld c0 %lld)\n", letter_form, bits, shift,
                 static_cast<long long>(n), static_cast<long long>(c0));
    ++failures;
    return;
  }
  std::unique_ptr<uint8_t[]> codes(new uint8_t[static_cast<size_t>(sz.codes)]);
  std::unique_ptr<int64_t[]> dense(new int64_t[static_cast<size_t>(n) + 1]);
  moc::decode_wire_cpu(b, codes.get(), dense.get());
  // ---- against the plain decode of the wire arrays themselves
  bool ok = true;
  int64_t o = woff[0];
  for (int64_t i = 0; i < n; ++i) {
    ok = ok && dense[i] == o && o == offsets[i];
    o += bits ? length_of(lengths.get(), bits, base, i) : woff[i + 1] - woff[i];
  }
  ok = ok && dense[n] == o && o == c1;
  for (int64_t x = c0; x < c1; ++x) {
    const uint8_t want = letter_form == 3 ? letter33(b.letters, x) : letter_form == 1 ? letter5(b.letters, x) : b.letters[x];
    ok = ok && codes[x - c0] == want && want == std::max<uint8_t>(stream[x], 1);
  }
  checked += n + (c1 - c0);
  if (!ok) {
    std::fprintf(stderr, "wire_san: decode differs (form %d bits %d shift %d n %lld c0 %lld)\n", letter_form, bits, shift,
                 static_cast<long long>(n), static_cast<long long>(c0));
    ++failures;
  }
}

template <typename F>
void must_throw(const char* what, F&& f) {
  try {
    f();
  } catch (const moc::Error&) {
    return;
  }
  std::fprintf(stderr, "wire_san: no error for %s\n", what);
  ++failures;
}

void validation() {
  const int64_t off[3] = {0, 5, 11};
  const uint8_t len8[2] = {5, 6};
  uint8_t letters[11];
  std::memset(letters, 1, sizeof(letters));
  uint8_t codes[16];
  int64_t dense[3];
  moc::WireBatch ok;
  ok.letters = letters;
  ok.offsets = off;
  ok.lengths = len8;
  ok.n = 2;
  moc::decode_wire_cpu(ok, codes, dense);  // the valid batch itself
  auto bad = [&](const char* what, auto&& change) {
    moc::WireBatch b = ok;
    change(b);
    must_throw(what, [&] { moc::decode_wire_cpu(b, codes, dense); });
    must_throw(what, [&] { moc::validate_wire(b); moc::wire_dense_offsets(b, dense); });
  };
  const int64_t sparse[2] = {0, 11};
  bad("sparse offsets without lengths", [&](moc::WireBatch& b) { b.offsets = sparse; b.off_shift = 1; b.lengths = nullptr; });
  bad("off_shift 7", [&](moc::WireBatch& b) { b.off_shift = 7; });
  bad("off_shift -1", [&](moc::WireBatch& b) { b.off_shift = -1; });
  bad("len_bits 5", [&](moc::WireBatch& b) { b.len_bits = 5; });
  bad("both packings", [&](moc::WireBatch& b) { b.packed5 = b.packed33 = true; });
  bad("n < 0", [&](moc::WireBatch& b) { b.n = -1; });
  bad("n = 2^31 - 1", [&](moc::WireBatch& b) { b.n = (int64_t{1} << 31) - 1; });
  const int64_t off_bad[3] = {0, 5, 12};
  bad("dense end offset", [&](moc::WireBatch& b) { b.offsets = off_bad; });
  const int64_t sparse_bad[2] = {0, 12};
  bad("sparse end offset", [&](moc::WireBatch& b) { b.offsets = sparse_bad; b.off_shift = 1; });
}

}  // namespace

int main() {
  const int forms[3] = {3, 1, 0};
  const int bit_forms[5] = {moc::kLenBase6, 3, 4, 8, 0};
  const int shifts[4] = {0, 1, 3, 6};
  const int64_t ns[10] = {0, 1, 7, 23, 24, 25, 63, 64, 65, 129};
  const int64_t firsts[4] = {0, 1, 6, 57};
  for (int form : forms)
    for (int bits : bit_forms)
      for (int shift : shifts) {
        if (shift && !bits) continue;  // sparse offsets need lengths
        for (int64_t n : ns)
          for (int64_t c0 : firsts) run(form, bits, shift, n, c0);
      }
  validation();
  if (failures) {
    std::fprintf(stderr, "wire_san: %d failures\n", failures);
    return 1;
  }
  std::printf("wire_san ok: %lld records and letters checked\n", static_cast<long long>(checked));
  return 0;
}
