"""Host twin of the e4m3 bag format (toad_amd/ingest.py, DESIGN.md "e4m3 bags"): numpy, float64, written from the definition and not from torch or
the product. Not collected by pytest; shared by test_bag_e4m3_host.py and test_gpu_bag_e4m3.py.

    code c: s = c >> 7, e = (c >> 3) & 15, m = c & 7; value = m 2^-9 for e == 0, (8 + m) 2^(e - 10) otherwise; c & 0x7F == 0x7F is NaN.
    element = value(code) 2^-exp, -7 <= exp <= 15.
    quantiser: the code whose value is nearest to |x| 2^exp, a tie to the even code, everything >= 448 to 0x7E, the sign bit of x kept, NaN -> 0x7F | sign.
"""
import math

import numpy as np

EXP_MIN, EXP_MAX = -7, 15


def _value(c: int) -> float:
    s, e, m = c >> 7, (c >> 3) & 15, c & 7
    if e == 15 and m == 7:
        return math.nan
    v = m * 2.0 ** -9 if e == 0 else (8 + m) * 2.0 ** (e - 10)
    return -v if s else v


TABLE = np.array([_value(c) for c in range(256)], dtype=np.float64)          # value(code), NaN at 0x7F and 0xFF
MAGS = TABLE[:127].copy()                                                    # the 127 non-negative finite values, ascending; index == code
MIDS = (MAGS[:-1] + MAGS[1:]) / 2                                            # MIDS[i] lies between codes i and i + 1 (exact in float64)
MAX = 448.0


def decode(codes, exp: int) -> np.ndarray:
    """float64 values of uint8 codes at exponent exp (exact: a 4-bit significand times a power of two)."""
    assert EXP_MIN <= exp <= EXP_MAX
    return TABLE[np.asarray(codes, dtype=np.uint8)] * 2.0 ** -exp


def decode_bits(codes, exp: int, dtype):
    """The decode as dtype (np.float16 or np.float32); the cast is exact for every finite code inside the exponent range."""
    with np.errstate(invalid="ignore"):
        return decode(codes, exp).astype(dtype)


def quantise(x, exp: int) -> np.ndarray:
    """uint8 codes of real numbers x (any float array; taken as float64, so fp16 and fp32 inputs are exact) at exponent exp: a nearest-neighbour search
    over the 127 non-negative values."""
    assert EXP_MIN <= exp <= EXP_MAX
    with np.errstate(invalid="ignore"):                                      # (a signalling NaN among the inputs)
        x = np.asarray(x, dtype=np.float64)
        y = np.abs(x) * 2.0 ** exp                                             # exact: a power of two, far from float64's limits for fp32 inputs
    flat = y.reshape(-1)
    nan = np.isnan(flat)
    yy = np.where(nan, 0.0, flat)
    lo = np.searchsorted(MAGS, yy, side="right") - 1                         # MAGS[lo] <= y, lo in 0 .. 126
    lo = np.clip(lo, 0, 126)
    hi = np.minimum(lo + 1, 126)
    dl, dh = yy - MAGS[lo], MAGS[hi] - yy
    up = (hi > lo) & ((dh < dl) | ((dh == dl) & (hi % 2 == 0)))              # nearer above, or a tie and the code above is the even one
    code = np.where(up, hi, lo)
    code = np.where(yy >= MAX, 0x7E, code)
    code = np.where(nan, 0x7F, code).astype(np.uint8)
    sign = (np.signbit(x.reshape(-1)).astype(np.uint8) << 7).astype(np.uint8)
    return (code | sign).reshape(x.shape)


def e4m3_exponent(amax) -> int:
    """The largest e in -7 .. 15 with amax 2^e <= 448 (-7 where there is none; 0 for amax == 0)."""
    amax = float(amax)
    if math.isnan(amax) or math.isinf(amax):
        raise ValueError("amax must be finite")
    amax = abs(amax)
    if amax == 0.0:
        return 0
    for e in range(EXP_MAX, EXP_MIN, -1):
        if math.ldexp(amax, e) <= MAX:
            return e
    return EXP_MIN


def error_bound(x, exp: int) -> np.ndarray:
    """The derived bound on |decode(quantise(x)) - x| for |x| 2^exp <= 448: 2^-4 |x| where |x| 2^exp >= 2^-6 (half an ulp of a 4-bit significand),
    2^-10 2^-exp below (half the subnormal spacing 2^-9)."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    return np.where(x * 2.0 ** exp >= 2.0 ** -6, x * 2.0 ** -4, 2.0 ** -10 * 2.0 ** -exp)
