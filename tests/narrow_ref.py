"""numpy twin of NARROW OPERANDS (include/fora_hip.h): the codes of f16, FP8 E4M3 and FP8 E5M2 widened to float32 by the
contract's rule, written with integers and ldexp -- nothing here goes through astype(np.float16) or a torch FP8 dtype, which are
what tests/test_narrow_cpu.py holds these functions to."""
import numpy as np

F16, E4M3, E5M2 = "f16", "e4m3", "e5m2"
PROP_TYPE = {F16: 4, E4M3: 5, E5M2: 6}
CODE_DTYPE = {F16: np.uint16, E4M3: np.uint8, E5M2: np.uint8}
KEYWORD = {F16: False, E4M3: "e4m3", E5M2: "e5m2"}     # what the binding's bf16= keyword takes beside the array


def _signed(s, mag):
    # float32 throughout; -0 stays -0 because the sign is applied to the magnitude, zero included
    return np.where(s.astype(bool), -mag, mag).astype(np.float32)


def f16_to_f32(codes):
    """IEEE binary16: e = 0 is m * 2^-24, 1 <= e <= 30 is (1024 + m) * 2^(e - 25), e = 31 is inf (m = 0) or NaN"""
    c = np.asarray(codes).astype(np.int64)
    s, e, m = (c >> 15) & 1, (c >> 10) & 31, c & 1023
    sub = np.ldexp(m.astype(np.float64), -24)
    nor = np.ldexp((1024 + m).astype(np.float64), e - 25)
    mag = np.where(e == 0, sub, nor)
    mag = np.where(e == 31, np.where(m == 0, np.inf, np.nan), mag)
    return _signed(s, mag)


def e5m2_to_f32(codes):
    """the binary16 whose bits are byte << 8"""
    return f16_to_f32(np.asarray(codes).astype(np.int64) << 8)


def e4m3_to_f32(codes):
    """the OCP fn form: e = 0 is m * 2^-9, otherwise (8 + m) * 2^(e - 10); 0x7F and 0xFF are NaN; no infinities"""
    c = np.asarray(codes).astype(np.int64)
    s, e, m = (c >> 7) & 1, (c >> 3) & 15, c & 7
    sub = np.ldexp(m.astype(np.float64), -9)
    nor = np.ldexp((8 + m).astype(np.float64), e - 10)
    mag = np.where(e == 0, sub, nor)
    mag = np.where((c & 0x7F) == 0x7F, np.nan, mag)
    return _signed(s, mag)


WIDEN = {F16: f16_to_f32, E4M3: e4m3_to_f32, E5M2: e5m2_to_f32}


def widen(kind, codes):
    """the float32 array a call reads when it is given these codes as `kind`"""
    return np.ascontiguousarray(WIDEN[kind](codes))


def as_operand(kind, codes):
    """(array, keyword) as Engine's calls take a numpy operand of `kind`: float16 by dtype, FP8 as uint8 with the keyword"""
    codes = np.ascontiguousarray(codes, dtype=CODE_DTYPE[kind])
    return (codes.view(np.float16) if kind == F16 else codes), KEYWORD[kind]


def is_finite_code(kind, codes):
    return np.isfinite(WIDEN[kind](codes))


def moderate_codes(rng, kind, shape):
    """random finite codes of moderate exponent (values within about 2^-3 .. 2^2 in magnitude, both signs, some zeros)"""
    sign = rng.integers(0, 2, size=shape)
    if kind == F16:
        c = (sign << 15) | (rng.integers(12, 18, size=shape) << 10) | rng.integers(0, 1024, size=shape)
    elif kind == E4M3:
        c = (sign << 7) | (rng.integers(4, 10, size=shape) << 3) | rng.integers(0, 8, size=shape)
    else:
        c = (sign << 7) | (rng.integers(12, 18, size=shape) << 2) | rng.integers(0, 4, size=shape)
    c = np.where(rng.random(size=shape) < 0.03, sign << (15 if kind == F16 else 7), c)   # +-0
    return c.astype(CODE_DTYPE[kind])
