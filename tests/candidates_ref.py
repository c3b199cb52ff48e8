"""The numpy model of the candidate-list entries (include/hydia.h "candidate lists and matches") and the crafted inputs their tests share.

  select(v, t, cap)   the indices i with v[i] >= t ascending (IEEE: -0.0 >= +0.0 holds, a NaN never), the first cap of them, their values,
                      and the total count
  topk(v, k)          the min(k, n) largest by (NaN last, value descending, index ascending) with -0.0 tying with +0.0 — a stable sort
                      on (isnan, -(v + 0.0)), written without any radix idea; the values are the input's own doubles, bit for bit

wrong_select / wrong_topk are the plausible wrong forms of the kernels (tests/test_candidates_cpu.py shows for each an input of
contents() that it changes)."""
import numpy as np

TILE = 1024              # HY_SEL_TILE: the elements one workgroup of the count / scatter kernels owns
SCAN_TRIP = 1024         # HY_SEL_SCAN_TRIP: tile counts per trip of the scan kernel's loop
ONE_TRIP = TILE * SCAN_TRIP  # what one trip of the scan covers: 2^20 elements


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def select(v, t, cap=None):
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        idx = np.flatnonzero(v >= t)
    w = idx if cap is None else idx[:cap]
    return w, v[w], idx.size


def topk(v, k):
    v = np.asarray(v, dtype=np.float64)
    nan = np.isnan(v)
    key = np.where(nan, 0.0, -(v + 0.0))  # + 0.0: both zeros become +0.0, so they tie
    order = np.lexsort((np.arange(v.size), key, nan))[:k]  # last key first: NaN last, then value descending, then index ascending
    return order, v[order]


# ---- crafted contents.  Each returns n doubles; rng is a numpy Generator
def from_bits(u):
    return np.asarray(u, dtype=np.uint64).view(np.float64)


def contents(n, rng):
    """name -> n doubles: the cases of the device-array tests"""
    c = {}
    c["normal"] = rng.standard_normal(n)
    c["equal"] = np.full(n, 0.4375)
    z = np.where(rng.integers(0, 2, n) == 1, 0.0, -0.0)
    c["zeros"] = z
    s = rng.standard_normal(n)
    special = np.array([np.inf, -np.inf, np.nan, -np.nan, 0.0, -0.0])
    where = rng.random(n) < 0.3
    s[where] = special[rng.integers(0, special.size, int(where.sum()))]
    c["specials"] = s
    c["four"] = np.array([-1.5, 0.25, 0.25000000000000006, 3.0])[rng.integers(0, 4, n)]
    c["negatives"] = -np.abs(rng.standard_normal(n)) - 1e-3
    c["subnormals"] = from_bits(rng.integers(0, 1 << 20, n).astype(np.uint64) | (rng.integers(0, 2, n).astype(np.uint64) << np.uint64(63)))
    # bit patterns that differ only in the lowest byte (the LAST radix pass decides) and only in the highest (the FIRST decides: sign and
    # the top exponent bits; 0x7f / 0xff with this mantissa would be NaN, so the top byte stays off them)
    base = np.uint64(0x3FD5555555555500)
    c["low_byte"] = from_bits(base | rng.integers(0, 256, n).astype(np.uint64))
    tops = np.array([b for b in range(256) if b not in (0x7F, 0xFF)], dtype=np.uint64)
    c["high_byte"] = from_bits((tops[rng.integers(0, tops.size, n)] << np.uint64(56)) | np.uint64(0x0005555555555555))
    return c


def top_group(v):
    """the size of the top tie group of v: how many elements share the best key"""
    i, _ = topk(v, 1)
    b = v[i[0]]
    if np.isnan(b):
        return int(np.isnan(v).sum())
    return int((v == b).sum())


# ---- wrong forms (what a plausible slip in a kernel computes)
def key64(v):
    """the order-preserving key the kernels use, restated in numpy: NaN -> 0, zeros -> 2^63, negatives reversed, positives above"""
    u = bits(v).copy()
    mag = u & np.uint64(0x7FFFFFFFFFFFFFFF)
    neg = (u >> np.uint64(63)) == 1
    k = np.where(neg, ~u, u | np.uint64(1 << 63))
    k = np.where(mag == 0, np.uint64(1 << 63), k)
    return np.where(mag > np.uint64(0x7FF0000000000000), np.uint64(0), k)


def _by_key(key, k, from_end=False, quota_off=0):
    """the kernels' scheme on a given key: everything above the k-th key in index order, then `quota` ties, sorted (key desc, idx asc)"""
    n = key.size
    k = min(k, n)
    kth = np.sort(key)[::-1][k - 1]
    above = np.flatnonzero(key > kth)
    ties = np.flatnonzero(key == kth)
    quota = max(0, min(ties.size, k - above.size + quota_off))
    ties = ties[ties.size - quota:] if from_end else ties[:quota]
    sel = np.concatenate([above, ties])
    return sel[np.lexsort((sel, ~key[sel]))]


def wrong_topk(form, v, k):
    v = np.asarray(v, dtype=np.float64)
    u = bits(v)
    if form == "zeros_not_canonical":  # -0.0 keeps its own key, just below +0.0
        mag = u & np.uint64(0x7FFFFFFFFFFFFFFF)
        key = np.where((mag == 0) & ((u >> np.uint64(63)) == 1), np.uint64((1 << 63) - 1), key64(v))
    elif form == "negatives_not_reversed":  # sign flipped only: negatives ordered by magnitude ascending
        key = np.where(np.isnan(v), np.uint64(0), np.where((u & np.uint64(0x7FFFFFFFFFFFFFFF)) == 0, np.uint64(1 << 63), u ^ np.uint64(1 << 63)))
    elif form == "nan_high":  # NaN left where its bit pattern puts it: above +inf
        mag = u & np.uint64(0x7FFFFFFFFFFFFFFF)
        key = np.where(mag > np.uint64(0x7FF0000000000000), np.uint64(0xFFFFFFFFFFFFFFFF), key64(v))
    else:
        key = key64(v)
    idx = _by_key(key, k, from_end=form == "ties_from_end", quota_off=-1 if form == "quota_off_by_one" else 0)
    return idx, v[idx]


def wrong_select(form, v, t, cap=None):
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        hit = v > t if form == "gt_for_ge" else v >= t
    if form == "tile_last_dropped":  # the last element of every tile never tested
        hit = hit.copy()
        hit[TILE - 1::TILE] = False
    idx = np.flatnonzero(hit)
    w = idx if cap is None else idx[:cap]
    return w, v[w], idx.size


WRONG_TOPK = ["zeros_not_canonical", "negatives_not_reversed", "nan_high", "ties_from_end", "quota_off_by_one"]
WRONG_SELECT = ["gt_for_ge", "tile_last_dropped"]
