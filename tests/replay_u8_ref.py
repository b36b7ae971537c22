"""Host restatement of the uint8 replay ring's number formats (shared by test_replay_u8_host.py and test_gpu_replay_u8.py), written from
the formulas in include/dgvit_hip.h, independent of the kernels.

* ``quantize``:   code = rint(clip(fl(x * 255), 0, 255)) in fp32, halves to even (np.rint), NaN -> 0.
* ``dequantize``: fl(k / 255) in fp32, a correctly rounded division -- what ``uint8_tensor.float() / 255`` computes.
* ``newton_dequantize``: the three fp32 operations the kernels use in place of the division (csrc/replay_ring.hip: dequant_u8), each
  evaluated in exact rational arithmetic and rounded once, as a hardware multiply and fused multiply-add round.
* ``tie_inputs``: fp32 inputs whose product with 255 rounds to exactly m + 0.5, where half-to-even and half-away-from-zero part.
* ``pattern``:    frames of codes for offset tests.  Bytes cannot carry a distinct value per pixel; a prime modulus (251) with
  multipliers coprime to it makes a wrong row, column or image-row offset mismatch almost everywhere.
"""
from fractions import Fraction

import numpy as np

F32 = np.float32
# |dequantize(quantize(x)) - x| for x in [0, 1]: half a code step, 1/510, plus the rounding of the product x * 255 seen through the
# division (255 * 2^-24 / 255 = 2^-24) plus the rounding of the division itself (at most 2^-25 below 1): 2^-23 covers both
ROUND_TRIP_BOUND = 1.0 / 510.0 + 2.0 ** -23


def quantize(x):
    """uint8 codes of an fp32 array (any shape)"""
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.asarray(x, dtype=F32) * F32(255)
        y = np.rint(np.clip(y, F32(0), F32(255)))
    return np.where(np.isnan(y), F32(0), y).astype(np.uint8)


def dequantize(k):
    """fp32 values of uint8 codes"""
    return np.asarray(k).astype(F32) / F32(255)


def tie_inputs():
    """(ms, xs): for every m in 0..254 for which one exists, an fp32 x with fl(x * 255) == m + 0.5 exactly, found by a nextafter search
    around (m + 0.5) / 255 (the product's spacing is at most that of x times 255 / 128, so a few steps either way reach it)"""
    ms, xs = [], []
    for m in range(255):
        target = F32(m + 0.5)
        x0 = F32((m + 0.5) / 255.0)
        cands = [x0]
        lo = hi = x0
        for _ in range(8):
            lo, hi = np.nextafter(lo, F32(-1)), np.nextafter(hi, F32(2))
            cands += [lo, hi]
        for x in cands:
            if F32(x * F32(255)) == target:
                ms.append(m)
                xs.append(x)
                break
    return np.array(ms, dtype=np.int64), np.array(xs, dtype=F32)


def pattern(rows, H, W):
    """(len(rows), H * W) uint8: code = (7919 r + 131 c + 17 (c // W)) mod 251 for ring row r and pixel c"""
    r = np.asarray(rows, dtype=np.int64).reshape(-1, 1)
    c = np.arange(H * W, dtype=np.int64).reshape(1, -1)
    return ((7919 * r + 131 * c + 17 * (c // W)) % 251).astype(np.uint8)


def round_f32(v):
    """an exact Fraction -> the nearest fp32, halves to even (normal range)"""
    if v == 0:
        return F32(0)
    sign, v, e = (-1 if v < 0 else 1), abs(v), 0
    while v >= Fraction(2) ** (e + 1):
        e += 1
    while v < Fraction(2) ** e:
        e -= 1
    scaled = v / Fraction(2) ** (e - 23)
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return F32(sign * float(Fraction(n) * Fraction(2) ** (e - 23)))


def fma_f32(a, b, c):
    """fl(a * b + c) with one rounding"""
    return round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def newton_dequantize(k):
    """q = fl(k * fl(1/255)); fl(q + fl(k - 255 q) * fl(1/255)) for one code k"""
    rinv = F32(float.fromhex("0x1.010102p-8"))
    x = F32(k)
    q = fma_f32(x, rinv, F32(0))
    return fma_f32(fma_f32(-q, F32(255), x), rinv, q)
