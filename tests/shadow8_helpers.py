"""Reference arithmetic of the 8-bit basis shadow (docs/design/15-shadow8.md), shared by tests/test_shadow8_reference_cpu.py
and tests/test_gpu_shadow8.py: plain numpy integer arithmetic on fp32 bit patterns, pinned against torch in the CPU test."""
import numpy as np


def shadow8_scale(n):
    """S = 2^ceil(log2(n) / 2), at most 2^15"""
    return float(1 << min(15, ((int(n) - 1).bit_length() + 1) // 2))


def e5m2_bits(x_f64):
    """fp64 (already multiplied by S) -> the uint8 the shadow stores: fp64 -> fp32 round-to-nearest-even, then fp32 -> e5m2
    round-to-nearest-even on the fp32 bit pattern.  TWO roundings.  Finite inputs below the overflow threshold 61440."""
    x = np.ascontiguousarray(np.asarray(x_f64, dtype=np.float64))
    with np.errstate(over="ignore", under="ignore"):
        u = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    sign = (u >> np.uint64(24)) & np.uint64(0x80)
    a = u & np.uint64(0x7FFFFFFF)
    # normal codes (|x| >= 2^-14): drop 21 mantissa bits to nearest even, re-bias the exponent 127 -> 15
    normal = (a + np.uint64(0x000FFFFF) + ((a >> np.uint64(21)) & np.uint64(1)) - np.uint64(0x38000000)) >> np.uint64(21)
    # subnormal codes: units of 2^-16; |x| = m 2^(e-150) with the implicit bit set in m, shifted right by 134 - e places
    e = a >> np.uint64(23)
    m = (a & np.uint64(0x7FFFFF)) | np.where(e > 0, np.uint64(0x800000), np.uint64(0)).astype(np.uint64)
    e = np.maximum(e, np.uint64(1))                        # fp32 subnormals share the exponent of 2^-126
    sh = np.minimum(np.uint64(134) - np.minimum(e, np.uint64(113)), np.uint64(40))
    one = np.uint64(1)
    q = m >> sh
    rem = m & ((one << sh) - one)
    half = one << (sh - one)
    sub = q + ((rem > half) | ((rem == half) & ((q & one) == one))).astype(np.uint64)
    code = np.where(a >= np.uint64(0x38800000), normal, sub)
    return (code | sign).astype(np.uint8)


def e5m2_value(bits):
    """the fp64 value of a stored uint8 (exact: an e5m2 code is the upper byte of an fp16)"""
    b = np.ascontiguousarray(np.asarray(bits)).astype(np.uint16)
    return (b << np.uint16(8)).view(np.float16).astype(np.float64)


def e5m2_chosen_values():
    """fp64 inputs where a wrong conversion shows (both signs of each): zero, ties with an even and an odd lower neighbour, a
    two-step rounding that differs from one step, carries into the exponent, the subnormal range (below, at and above half a
    step, ties), the smallest normal, the largest values the scale admits, fp32 subnormals, a value that vanishes."""
    pos = [0.0,
           1.0 + 2.0 ** -3,                    # tie, lower neighbour 0x3C even -> 0x3C
           1.0 + 3.0 * 2.0 ** -3,              # tie, lower neighbour 0x3D odd  -> 0x3E
           1.0 + 2.0 ** -3 + 2.0 ** -40,       # fp32 drops 2^-40, then the tie goes to even: 0x3C (one step: 0x3D)
           float(np.nextafter(2.0, 0.0)), 2.0 - 2.0 ** -23, 1.75 + 2.0 ** -3,      # carry to 0x40
           1.25 - 2.0 ** -20,
           2.0 ** -14, 2.0 ** -14 - 2.0 ** -30,                                   # smallest normal and just below
           2.0 ** -16, 2.0 ** -15, 3.0 * 2.0 ** -16,                              # the three subnormal codes
           2.0 ** -17, 2.0 ** -17 + 2.0 ** -40, 2.0 ** -17 - 2.0 ** -41,            # half a step: tie -> 0, above -> 1, below -> 0
           3.0 * 2.0 ** -17, 5.0 * 2.0 ** -17, 7.0 * 2.0 ** -17,                   # ties -> 2, 2, 4 (= smallest normal)
           2.0 ** -18, 2.0 ** -126, 2.0 ** -140, 1e-300,
           2.0 ** 15, 2.0 ** 15.5, 57344.0, 53248.0, 40960.0 + 4096.0]           # up to the largest finite code
    return np.array(pos + [-v for v in pos], dtype=np.float64)
