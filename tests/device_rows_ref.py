"""Expectations for templates that arrive in device memory (tests/test_rows_norm_host.py, tests/test_gpu_device_rows.py): the exact
widening of f16 / bf16 / f32 bit patterns by numpy, the row normalisation by the oracle's hyo_normalize, and the edge rows both test
files use.  TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

import oracle_lib as O

F16_NANS, BF16_NANS = 2046, 254  # patterns with all exponent bits and a non-zero mantissa: 2 (2^10 - 1) and 2 (2^7 - 1)


def widen_bits(bits, dtype):
    """float64 of the bit patterns `bits` (any shape) read as `dtype` in ("f64", "f32", "f16", "bf16"): numpy's own conversions"""
    bits = np.asarray(bits)
    with np.errstate(invalid="ignore"):  # (widening a signalling NaN)
        return _widen_bits(bits, dtype)


def _widen_bits(bits, dtype):
    if dtype == "f64":
        return bits.astype(np.uint64).view(np.float64).copy()
    if dtype == "f32":
        return bits.astype(np.uint32).view(np.float32).astype(np.float64)
    if dtype == "f16":
        return bits.astype(np.uint16).view(np.float16).astype(np.float64)
    if dtype == "bf16":
        return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)
    raise ValueError(dtype)


def same_bits(a, b):
    """bit for bit (signed zeros and NaN payloads included)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def same_bits_nan_as_nan(got, want, nans):
    """bit for bit except at NaN patterns, which only have to be NaN — and there are exactly `nans` of them, so nothing else is excused"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return int(nan.sum()) == nans and np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))


def hyo_normalize_rows(rows):
    """a normalised copy of float64 rows [n][dim]: the oracle's hyo_normalize row by row"""
    out = np.ascontiguousarray(rows, dtype=np.float64).copy()
    L = O.lib()
    for r in range(out.shape[0]):
        L.hyo_normalize(O._ptr(out[r]), out.shape[1])
    return out


@functools.lru_cache(maxsize=None)
def edge_rows(dim):
    """float64 rows at the edges of the normalisation (read-only): a zero row; a row with one non-zero element; f32 subnormals; f64
    subnormals (their squares vanish: m = 0, the row passes through); f16 maxima; an f64 row whose squared sum overflows (m = inf, the
    row becomes zeros); a mixed-sign row with a negative zero"""
    k = np.arange(dim, dtype=np.float64)
    one = np.zeros(dim)
    one[dim // 3] = -3.0
    mixed = (k - dim / 2) * 0.37
    mixed[0] = -0.0
    rows = np.stack([np.zeros(dim), one, (k + 1) * 2.0 ** -149, (k + 1) * 5e-324, np.full(dim, 65504.0), np.full(dim, 1e200), mixed])
    rows.setflags(write=False)
    return rows


def edge_bits(dim, dtype):
    """the edge rows as bit patterns of `dtype` (those that do not exist in a narrower type are cast by numpy: subnormals flush to
    smaller ones or to zero, 1e200 becomes inf — NaN-free for f64 / f32, and the inf row of the narrow types is left out)"""
    rows = edge_rows(dim)
    if dtype == "f64":
        return rows.view(np.uint64).copy()
    if dtype == "f32":
        return rows[:5].astype(np.float32).view(np.uint32).copy()
    if dtype == "f16":
        return np.concatenate([rows[:5], rows[6:]]).astype(np.float16).view(np.uint16).copy()
    if dtype == "bf16":  # truncation of the float32 pattern: exact for the rows used, and any bf16 pattern is a legitimate input
        return (np.concatenate([rows[:5], rows[6:]]).astype(np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)
    raise ValueError(dtype)
