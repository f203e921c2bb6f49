"""Numpy models of the device decoders of the wire formats, and exhaustive checks of the multiply-by-reciprocal
constants they use. One model per piece of device arithmetic, operation for operation, with the operand widths the
instructions have (24-bit multiplies, 32-bit wrapping subtractions, one f32 rounding per product):

  p33_streaming   csrc/src/hip/swipe_impl.hpp, the streaming swipe kernel's P33 loop: (x >> 1) / 13, / 26 chains
  p33_lane_direct swipe_impl.hpp decode_p33_field_lut: umulhi, v_mul_hi_u32_u24, v_mad_i32_i24, the LDS pair table
  p33_unpack      csrc/src/hip/wire_kernels.hip p33_letters: the same constants, (v * 2521) >> 16 for a pair
  len6_lengths4   csrc/src/hip/kernel_common.hpp record_lengths4: / 1296 for the upper half, / 6 chains
  len6_record     kernel_common.hpp record_length: a / 6 loop
  len6_lane       swipe_impl.hpp lane_length6: trunc((v + 0.5f) * fl(1 / 6^i)) in f32, a 24-bit mad
  len6_wire       wire_kernels.hip wire_length: / 1296, / 36, / 6 by the digit's bits

Every constant is a keyword argument, so that tests/test_decoder_cases.py can show which inputs tell a constant that
is off by one from the right one. (decode_p33_field, the inline-assembly variant in swipe_impl.hpp, has no caller.)
numpy, CPU only.

    python tools/p33_magic_check.py
"""
import numpy as np

U64 = np.uint64
M32 = U64(0xFFFFFFFF)
M24 = U64(0xFFFFFF)
MAGIC_P4 = 2463805336   # ceil(2^46 / 13^4): x / 26^4 = umulhi(x >> 4, .) >> 14
MAGIC_676 = 6353502     # ceil(2^32 / 676)
MAGIC_26 = 2521         # v / 26 = (2521 v) >> 16 for v < 676


def _u64(x):
    return np.asarray(x, dtype=U64)


def umulhi(a, b):  # 32 x 32 -> high 32 (the operands here keep the product below 2^64)
    return (_u64(a) * U64(b)) >> U64(32)


def umul24(a, b):  # v_mul_u32_u24: low 32 bits of the product of the operands' low 24 bits
    return ((_u64(a) & M24) * (U64(b) & M24)) & M32


def mulhi_u24(a, b):  # v_mul_hi_u32_u24: bits 32..47 of that product
    return ((_u64(a) & M24) * (U64(b) & M24)) >> U64(32)


def mad_i24(a, b: int, c):  # v_mad_i32_i24: a and b as signed 24-bit values, a * b + c modulo 2^32
    sa = (_u64(a) & M24).astype(np.int64)
    sa = np.where(sa >= 1 << 23, sa - (1 << 24), sa)
    return ((sa * np.int64(b) + _u64(c).astype(np.int64)) & np.int64(0xFFFFFFFF)).astype(U64)


def _bytes_of(lo, hi):  # bytes 0..6 of the 32-bit pair (lo, hi): the seven letter codes
    cols = [(lo >> U64(8 * j)) & U64(0xFF) for j in range(4)] + [(hi >> U64(8 * j)) & U64(0xFF) for j in range(3)]
    return np.stack(cols, axis=1).astype(np.uint8)


def p33_streaming(x):
    """Field values -> uint8 [n, 7] letter codes as the streaming swipe kernel decodes them."""
    x = _u64(x)
    v = (x >> U64(1)) // U64(13)  # 32-bit: x >> 1 < 2^32
    cols = [((x & M32) - U64(26) * v + U64(1)) & U64(0xFF)]
    for _ in range(6):
        q = v // U64(26)
        cols.append((v - U64(26) * q + U64(1)) & U64(0xFF))
        v = q
    return np.stack(cols, axis=1).astype(np.uint8)


def _split(x, magic_p4, mul_a):
    x = _u64(x)
    a = umulhi(x >> U64(4), magic_p4) >> U64(14)      # digits 4..6
    b = ((x & M32) - mul_a(a, 456976)) & M32           # digits 0..3, wrapping
    return a, b


def p33_lane_direct(x, magic_p4=MAGIC_P4, magic_676=MAGIC_676):
    """decode_p33_field_lut. An index past the 676-entry pair table reads as the code pair (0, 0)."""
    a, b = _split(x, magic_p4, umul24)
    b32, a2 = mulhi_u24(b, magic_676), mulhi_u24(a, magic_676)
    b10, a10 = mad_i24(b32, -676, b), mad_i24(a2, -676, a)
    v = np.arange(676, dtype=U64)
    table = (v % U64(26) + U64(1)) | ((v // U64(26) + U64(1)) << U64(8))

    def pairs(i):
        return np.where(i < U64(676), table[np.minimum(i, U64(675)).astype(np.int64)], U64(0))

    lo = pairs(b10) | (pairs(b32) << U64(16))
    hi = (pairs(a10) | ((a2 + U64(1)) << U64(16))) & M32
    return _bytes_of(lo, hi)


def p33_unpack(x, magic_p4=MAGIC_P4, magic_676=MAGIC_676, magic_26=MAGIC_26):
    """p33_letters of unpack33_kernel: 32-bit multiplies, the pair's bytes by arithmetic, + 0x01010101 on the word."""
    a, b = _split(x, magic_p4, lambda p, q: (p * U64(q)) & M32)
    b32, a2 = umulhi(b, magic_676), umulhi(a, magic_676)
    b10, a10 = (b - b32 * U64(676)) & M32, (a - a2 * U64(676)) & M32

    def pair_bytes(v):
        q = ((v * U64(magic_26)) & M32) >> U64(16)
        return ((v - U64(26) * q) & M32) | ((q << U64(8)) & M32)

    lo = ((pair_bytes(b10) | ((pair_bytes(b32) << U64(16)) & M32)) + U64(0x01010101)) & M32
    hi = ((pair_bytes(a10) | ((a2 << U64(16)) & M32)) + U64(0x00010101)) & M32
    return _bytes_of(lo, hi)


def _chain6(v, count):
    cols = []
    for _ in range(count):
        d = v // U64(6)
        cols.append(v - U64(6) * d)
        v = d
    return cols


def len6_lengths4(v, div_half=1296):
    """Octet values -> int64 [n, 8] digits as record_lengths4 gives them: digits 0..3 and, from v / 1296, 4..7."""
    v = _u64(v)
    return np.stack(_chain6(v, 4) + _chain6(v // U64(div_half), 4), axis=1).astype(np.int64)


def len6_record(v):
    """record_length: digit j after j divisions by 6."""
    v = _u64(v)
    cols = []
    for _ in range(8):
        cols.append(v % U64(6))
        v = v // U64(6)
    return np.stack(cols, axis=1).astype(np.int64)


def len6_lane(v, half=0.5):
    """lane_length6: q_i = trunc((float(v) + half) * fl(1 / 6^i)) in f32, digit j = q_j - 6 q_(j+1) as a 24-bit mad."""
    fv = np.asarray(v).astype(np.float32) + np.float32(half)
    recip = [np.float32(1) / np.float32(6 ** i) for i in range(9)]  # constexpr float division: correctly rounded
    q = [np.trunc(fv * r).astype(np.int64) for r in recip]
    cols = [mad_i24(q[j + 1], -6, q[j]).astype(np.int64) for j in range(8)]
    cols = [np.where(c >= 1 << 31, c - (1 << 32), c) for c in cols]  # the kernel reads the result as an int
    return np.stack(cols, axis=1)


def len6_wire(v, div_half=1296):
    """wire_length: / 1296, / 36 and / 6 where the digit's index has bits 4, 2 and 1."""
    v = _u64(v)
    cols = []
    for d in range(8):
        w = v
        if d & 4:
            w = w // U64(div_half)
        if d & 2:
            w = w // U64(36)
        if d & 1:
            w = w // U64(6)
        cols.append(w % U64(6))
    return np.stack(cols, axis=1).astype(np.int64)


def check_range(lo, hi, fn, want, chunk=1 << 26):
    for s in range(lo, hi, chunk):
        v = np.arange(s, min(s + chunk, hi), dtype=U64)
        assert (fn(v) == want(v)).all(), (fn, s)


def main():
    n = 26 ** 7  # a P33 field's value range
    m = -(-(1 << 46) // 28561)
    assert m == MAGIC_P4
    # A = umulhi(x >> 4, m) >> 14 == (x >> 4) // 13^4 for every x >> 4 of a field
    check_range(0, (n >> 4) + 1, lambda v: ((v * U64(m)) >> U64(32)) >> U64(14), lambda v: v // U64(28561))
    m676 = -(-(1 << 32) // 676)
    assert m676 == MAGIC_676 and m676 < (1 << 24)  # a v_mul_hi_u32_u24 operand
    check_range(0, 1 << 19, lambda v: (v * U64(m676)) >> U64(32), lambda v: v // U64(676))
    check_range(0, 676, lambda v: (v * U64(MAGIC_26)) >> U64(16), lambda v: v // U64(26))
    # record_words_p33: q0 / 7 = (q0 * 9363) >> 16 for every record start q0 <= 6 + 63 * 64 of a tile
    check_range(0, 13110, lambda v: (v * U64(9363)) >> U64(16), lambda v: v // U64(7))
    assert (13110 * 9363) >> 16 != 13110 // 7
    # base-6 length digits (lane_length6): octet v < 2^21, digit j = (v / 6^j) - 6 (v / 6^(j+1)), each
    # quotient trunc((v + 0.5) * fl(1 / 6^i)) in f32 (round-to-nearest product), i = 0..8
    v = np.arange(1 << 21, dtype=np.uint32)
    fv = v.astype(np.float32) + np.float32(0.5)
    for i in range(9):
        q = np.trunc(fv * np.float32(1.0 / 6 ** i)).astype(np.int64)
        assert (q == v // 6 ** i).all(), i
    # the lane's octet position: u / 3 = (u * 11) >> 5 for u = (8 t) % 3 + lane / 8 <= 9
    assert all(((u * 11) >> 5) == u // 3 for u in range(10))
    print("ok")


if __name__ == "__main__":
    main()
