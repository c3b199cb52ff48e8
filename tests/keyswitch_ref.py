"""Helpers of the crafted-evaluation-key tests (tests/test_keyswitch_edges_cpu.py, tests/test_gpu_keyswitch_edges.py): residue patterns
that put the KEY operand of a key switch at the bounds of the lazy sums, the same patterns for the polynomial that is switched, and a
Python-integer model of hybrid key switching that the oracle is pinned against.  TEST INFRASTRUCTURE ONLY; no tests in here.

A key is the oracle's own memory, [dnum][2][nT][N]: digit, polynomial (b then a), limb slot m with modulus P.moduli[m], evaluation
slot.  Oracle.rotate / relin / rotate_query read it in place, so an edited view IS the oracle's key; Context.import_eval_key loads
the same array into the GPU context.  A crafted key decrypts to nothing — the requirement is bit-exactness, as with the saturated
ciphertexts of batch_ref.

Patterns (for keys, `phase` is added to the per-row shift so that two rotations' keys differ):
  sat       every residue q_m - 1.  The same for every rotation: on its own it cannot tell rotation x's key from rotation x''s, so a
            test of several keys always holds one of holes / edge / uniform next to it
  holes     q_m - 1, one residue in 16 replaced by a uniform one BELOW q_m - 1 (so the count of holes is exact); the replaced
            position shifts with (digit, polynomial, limb) and the phase, so every position decides the result in some row
  edge      the cycle 0, 1, q_m - 2, q_m - 1 along the slots, started at another point per (digit, polynomial, limb) and phase
  digit-d   digit d saturated, every other digit zero: one term of the sum alone
  uniform   the control; the per-rotation difference comes from the generator the caller seeds per rotation"""
import ctypes as C

import numpy as np

import batch_ref as B

ROW_PATTERNS = ("sat", "holes", "edge", "uniform")
HOLE_EVERY = 16
EDGE_CYCLE = 4


def key_patterns(dnum):
    return ROW_PATTERNS + tuple("digit-%d" % d for d in range(dnum))


def row_shift(d, p, m, nT, phase):
    """the per-row shift of holes and edge: distinct for neighbouring (digit, polynomial, limb) and moved by the phase"""
    return (d * 2 + p) * nT + m + phase


def fill_row(row, q, pattern, rng, shift):
    """one row [N] of residues modulo q, in place"""
    q = int(q)
    N = row.shape[-1]
    if pattern == "sat":
        row[...] = q - 1
    elif pattern == "zero":
        row[...] = 0
    elif pattern == "uniform":
        row[...] = rng.integers(0, q, size=row.shape, dtype=np.uint64)
    elif pattern == "holes":
        row[...] = q - 1
        at = np.arange((-shift) % HOLE_EVERY, N, HOLE_EVERY)
        row[..., at] = rng.integers(0, q - 1, size=row.shape[:-1] + (len(at),), dtype=np.uint64)
    elif pattern == "edge":
        cycle = np.array([0, 1, q - 2, q - 1], dtype=np.uint64)
        row[...] = cycle[(np.arange(N) + shift) % EDGE_CYCLE]
    else:
        raise ValueError("unknown pattern %r" % (pattern,))


def craft_key(P, key_view, pattern, rng, phase=0):
    """Edit the [dnum][2][nT][N] oracle key view IN PLACE; every residue is rewritten.  Returns the view."""
    assert key_view.shape == (P.dnum, 2, P.nT, P.N), key_view.shape
    only = None
    if pattern.startswith("digit-"):
        only = int(pattern[6:])
        assert 0 <= only < P.dnum
    for d in range(P.dnum):
        for p in range(2):
            for m in range(P.nT):
                row_pattern = pattern if only is None else ("sat" if d == only else "zero")
                fill_row(key_view[d, p, m], P.moduli[m], row_pattern, rng, row_shift(d, p, m, P.nT, phase))
    return key_view


def digits_in_use(P, nl):
    return (nl + P.alpha - 1) // P.alpha


def poison_unused_digits(P, key_view, nl, value="sat"):
    """the key rows of the digits a switch at nl limbs does not use (d >= ceil(nl / alpha)) := q_m - 1 (or 0), in place"""
    for d in range(digits_in_use(P, nl), P.dnum):
        for m in range(P.nT):
            key_view[d, :, m] = (P.moduli[m] - np.uint64(1)) if value == "sat" else np.uint64(0)
    return key_view


def craft_ct(P, ct, pattern, rng, phase=0):
    """Every polynomial of the oracle ciphertext ct (any polynomial count) gets the pattern, in place.  sat and uniform are
    batch_ref.saturate / randomise; holes and edge shift per (polynomial, limb) like the key rows."""
    if pattern == "sat":
        return B.saturate(P, ct)
    if pattern == "uniform":
        return B.randomise(P, ct, rng)
    d = ct.data()
    for p in range(ct.npoly):
        for j in range(ct.nl):
            fill_row(d[p, j], P.moduli[j], pattern, rng, p * 5 + j + phase)
    return ct


def oracle_keyswitch(P, c, nl, key):
    """hyo_keyswitch of the oracle on a bare polynomial c [nl][N] (evaluation form) with the key array [dnum][2][nT][N]:
    (out0, out1), each [nl][N]"""
    c = np.ascontiguousarray(c, dtype=np.uint64)
    key = np.ascontiguousarray(key, dtype=np.uint64)
    assert c.shape == (nl, P.N) and key.shape == (P.dnum, 2, P.nT, P.N)
    out0, out1 = np.zeros((nl, P.N), dtype=np.uint64), np.zeros((nl, P.N), dtype=np.uint64)
    P.L.hyo_keyswitch(P.h, c.ctypes.data_as(C.c_void_p), nl, key.ctypes.data_as(C.c_void_p), out0.ctypes.data_as(C.c_void_p),
                      out1.ctypes.data_as(C.c_void_p))
    return out0, out1


# ------------------------------------------------------------------ the Python-integer model
def _ints(a):
    """a uint64 array as an object array of Python ints (no 64-bit wrap in what follows)"""
    a = np.asarray(a)
    out = np.empty(a.shape, dtype=object)
    out[...] = a.tolist()
    return out


def _u64(a):
    return np.array(a.tolist(), dtype=np.uint64)


def _prod(xs):
    r = 1
    for x in xs:
        r *= int(x)
    return r


def keyswitch_model(P, c, nl, key, skip_digit=None):
    """Hybrid key switching of the polynomial c [nl][N] (evaluation form) with key [dnum][2][nT][N], in Python integers: digit split
    (alpha limbs per digit), fast base conversion of every digit to Q_l u P, inner product with the key over Q_l u P, ModDown by P.
    Returns (out0, out1), each [nl][N] uint64 in evaluation form.  Only the transforms are the oracle's (P.ntt_fwd / P.ntt_inv); the
    constants come from P.moduli.  Every sum is formed unreduced and reduced once.  Meant for N = 2^11.
    skip_digit: leave one digit out of the inner product — the mutation the tests use to show the comparison is sensitive."""
    q = [int(v) for v in P.moduli]
    nQ, nP, alpha = P.nQ, P.nP, P.alpha
    ext = list(range(nl)) + list(range(nQ, nQ + nP))  # moduli of the extended basis Q_l u P
    nd = (nl + alpha - 1) // alpha
    c = np.asarray(c)
    coeff = [_ints(P.ntt_inv(c[j], j)) for j in range(nl)]
    acc = [[np.zeros(P.N, dtype=object) for _ in ext] for _ in range(2)]
    for d in range(nd):
        if d == skip_digit:
            continue
        lo, hi = d * alpha, min(d * alpha + alpha, nl)
        D = _prod(q[lo:hi])
        # y_j = c_j (D / q_j)^-1 mod q_j: the digit's value is sum_j y_j (D / q_j) up to a multiple of D
        y = {j: coeff[j] * pow(D // q[j] % q[j], -1, q[j]) % q[j] for j in range(lo, hi)}
        for t, m in enumerate(ext):
            if lo <= m < hi:
                dig = _ints(c[m])  # the digit's own limbs: the input as it is
            else:
                s = 0
                for j in range(lo, hi):
                    s = s + y[j] * (D // q[j] % q[m])
                dig = _ints(P.ntt_fwd(_u64(s % q[m]), m))
            for p in range(2):
                acc[p][t] = acc[p][t] + dig * _ints(key[d, p, m])
    PP = _prod(q[nQ:nQ + nP])
    out = []
    for p in range(2):
        y = []
        for k in range(nP):
            m = nQ + k
            y.append(_ints(P.ntt_inv(_u64(acc[p][nl + k] % q[m]), m)) * pow(PP // q[m] % q[m], -1, q[m]) % q[m])
        res = np.zeros((nl, P.N), dtype=np.uint64)
        for j in range(nl):
            s = 0
            for k in range(nP):
                s = s + y[k] * (PP // q[nQ + k] % q[j])
            conv = _ints(P.ntt_fwd(_u64(s % q[j]), j))
            res[j] = _u64((acc[p][j] - conv) * pow(PP % q[j], -1, q[j]) % q[j])
        out.append(res)
    return out[0], out[1]


def relin_model(P, data, key):
    """relinearisation of a 3-component ciphertext [3][nl][N] through keyswitch_model: [2][nl][N]"""
    data = np.asarray(data)
    nl = data.shape[1]
    k0, k1 = keyswitch_model(P, data[2], nl, key)
    out = np.zeros((2, nl, P.N), dtype=np.uint64)
    for j in range(nl):
        qj = int(P.moduli[j])
        out[0, j] = _u64((_ints(data[0, j]) + _ints(k0[j])) % qj)
        out[1, j] = _u64((_ints(data[1, j]) + _ints(k1[j])) % qj)
    return out


def rotate_model(P, data, key, r):
    """EvalFastRotation of a 2-component ciphertext [2][nl][N] through keyswitch_model: the switch of c1, c0 added, then the
    evaluation-form automorphism (the oracle's slot permutation, no arithmetic)"""
    data = np.asarray(data)
    nl = data.shape[1]
    k0, k1 = keyswitch_model(P, data[1], nl, key)
    g = P.galois(r)
    out = np.zeros((2, nl, P.N), dtype=np.uint64)
    for j in range(nl):
        qj = int(P.moduli[j])
        out[0, j] = P.automorph_eval(_u64((_ints(data[0, j]) + _ints(k0[j])) % qj), g)
        out[1, j] = P.automorph_eval(k1[j], g)
    return out


def first_difference(got, want):
    """(number of differing residues, index tuple of the first, got there, want there) or None"""
    if np.array_equal(got, want):
        return None
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    at = tuple(int(v) for v in bad[0])
    return len(bad), at, int(np.asarray(got)[at]), int(np.asarray(want)[at])
