"""Helpers of the receiver-side edge tests (tests/test_client_edges_cpu.py, tests/test_gpu_client_edges.py): Python-integer models of the
decryption dot product, of the decoder's front (centred CRT of one or two limbs, the conversion to a double, the division by the scale)
and of the encoder on a constant slot vector, and crafted inputs that sit on the boundaries of each.  TEST INFRASTRUCTURE ONLY; no tests
in here, no GPU, and nothing of the product is imported.

Two facts carry the expectations (test_client_edges_cpu.py asserts them as premises):
  1. a constant slot vector v encodes to the coefficient rne(v * scale) at index 0 and to 0 everywhere else, so its evaluation form is the
     constant rne(v * scale) mod q_j in every position of limb j;
  2. a coefficient-form polynomial with the value a at index 0 and 0 elsewhere decodes to centred(a) / scale in every slot, bit for bit
     the value of decode_front_model.
A ciphertext (c0, c1) = (NTT(t), 0) decrypts to t under any secret, so import_ct + decrypt reaches the decoder with a chosen t.

The models take keyword switches that turn them into the WRONG forms a kernel could have (a >= in a centring comparison, a one-step
conversion, ...).  The CPU file shows that each wrong form changes a result on the crafted inputs: that is what makes the inputs a test."""
from fractions import Fraction

import numpy as np

import keyswitch_ref as KS

TWO64 = 1 << 64
MASK64 = TWO64 - 1
DEC_PATTERNS = KS.ROW_PATTERNS  # sat, holes, edge, uniform


def ints(a):
    return [int(v) for v in np.asarray(a).reshape(-1).tolist()]


# ---------------------------------------------------------------------------------------------------------------- the decoder's front
def two_step(mag):
    """(double)(u64)(mag >> 64) * 2^64 + (double)(u64)mag: two correctly rounded conversions, one exact product, one rounded sum"""
    return float(mag >> 64) * 2.0 ** 64 + float(mag & MASK64)


def centred_crt(r0, r1, q0, q1, centre_ge=False, reduce_r0=True):
    """(negative?, magnitude) of the value in [0, q0 q1) with the residues r0 mod q0 and r1 mod q1, centred on (-Q/2, Q/2]: negative when
    x > floor(Q / 2).  reduce_r0=False is the wrong form that subtracts r0 from r1 without reducing it mod q1 first, in 64-bit words"""
    Q = q0 * q1
    if reduce_r0:
        d = (r1 - r0 % q1) % q1
    else:  # submod(r1, r0, q1) on a u64 with r0 possibly >= q1
        d = (r1 - r0 if r1 >= r0 else (r1 + q1 - r0) & MASK64) % q1
    t = d * pow(q0 % q1, -1, q1) % q1
    x = r0 + q0 * t
    neg = x >= (Q >> 1) if centre_ge else x > (Q >> 1)
    return neg, (Q - x if neg else x)


def decode_front_model(residues, moduli, scale, centre_ge=False, one_step=False, drop_second=False, reduce_r0=True):
    """residues [nu][n] (coefficient form, nu = 1 or 2), moduli the chain (q_0, q_1 are read): the n doubles the decoder hands to its FFT.
    nu = 2: centred CRT, the two-step conversion, the sign, ONE IEEE division.  nu = 1: centred on q_0 (negative when r0 > q_0 >> 1), one
    conversion of a value below 2^63, the sign, one division.  The keywords give the wrong forms."""
    residues = np.asarray(residues, dtype=np.uint64)
    nu = residues.shape[0]
    assert nu in (1, 2)
    q0, q1 = int(moduli[0]), int(moduli[1])
    scale = float(scale)
    out = np.empty(residues.shape[1], dtype=np.float64)
    r0s = ints(residues[0])
    r1s = ints(residues[1]) if nu == 2 else None
    for i, r0 in enumerate(r0s):
        if nu == 2 and not drop_second:
            neg, mag = centred_crt(r0, r1s[i], q0, q1, centre_ge, reduce_r0)
            v = float(mag) if one_step else two_step(mag)
        else:
            neg = r0 >= (q0 >> 1) if centre_ge else r0 > (q0 >> 1)
            v = float(q0 - r0 if neg else r0)
        out[i] = (-v if neg else v) / scale
    return out


# ---------------------------------------------------------------------------------------------------------------- the dot product
def dec_dot_model(ct, s, moduli):
    """c0 + s (c1 + s c2) mod q_j on the first nu = min(nl, 2) limbs of ct [npoly][nl][N] (npoly 2 or 3, evaluation form) with the secret s
    [>= nu][N] in evaluation form, in Python integers: [nu][N] uint64, still in evaluation form"""
    ct = np.asarray(ct, dtype=np.uint64)
    npoly, nl, N = ct.shape
    assert npoly in (2, 3)
    nu = min(nl, 2)
    out = np.empty((nu, N), dtype=np.uint64)
    for j in range(nu):
        q = int(moduli[j])
        sv = ints(np.asarray(s)[j])
        acc = ints(ct[npoly - 1, j])
        for p in range(npoly - 2, -1, -1):
            acc = [(a * b + c) % q for a, b, c in zip(acc, sv, ints(ct[p, j]))]
        out[j] = np.array(acc, dtype=np.uint64)
    return out


def dec_patterns(P, X, npoly, nl, pattern, seed):
    """[X][npoly][nl][N] residues of one of DEC_PATTERNS (keyswitch_ref.fill_row); the X ciphertexts differ: the shift of holes / edge
    moves with x and uniform rows are drawn one by one.  sat is the same for every x by its nature"""
    rng = np.random.default_rng(seed)
    out = np.empty((X, npoly, nl, P.N), dtype=np.uint64)
    for x in range(X):
        for p in range(npoly):
            for j in range(nl):
                KS.fill_row(out[x, p, j], P.moduli[j], pattern, rng, x * 7 + p * 5 + j)
    return out


# ---------------------------------------------------------------------------------------------------------------- the encoder
def rne(x):
    """round-half-even of a Fraction, as an exact integer"""
    f = x.numerator // x.denominator  # floor
    rem = x - f
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and f % 2 == 1):
        f += 1
    return f


def half_away(x):
    f = x.numerator // x.denominator
    rem = x - f
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and x > 0):
        f += 1
    return f


def truncate(x):
    return -((-x).numerator // (-x).denominator) if x < 0 else x.numerator // x.denominator


def encode_const_coeff(v, scale, rounding=rne):
    """the coefficient at index 0 of the encoding of the constant slot vector v (a double) at `scale` (a double): the product is exact"""
    return rounding(Fraction(float(v)) * Fraction(float(scale)))


def encode_const_model(v, scale, moduli, rounding=rne, zero_case=True):
    """canonical residues of encode_const_coeff on every limb of `moduli`: a list of Python integers.  zero_case=False is the wrong form
    q - (|m| mod q) of a negative coefficient, which gives q_j instead of 0 on a multiple of q_j"""
    m = encode_const_coeff(v, scale, rounding)
    out = []
    for q in moduli:
        q = int(q)
        if m >= 0 or zero_case:
            out.append(m % q)
        else:
            out.append(q - (-m) % q)
    return out


def encoder_ks(moduli):
    """the k of the crafted constant vectors v = k / scale, all doubles: ties, the ends of the 64-bit range and
    coefficients that are multiples of a limb's modulus.  2^52 + 0.5 is not a double (the spacing there is 1): as an expression in doubles
    it IS 2^52, and that is what stands here; 2^51 + 0.5, the largest tie a double can hold next to a 2^45 scale, stands beside it"""
    half = [0.5, 1.5, 2.5, 2.0 ** 52 + 0.5, 2.0 ** 51 + 0.5]
    ks = [s * h for h in half for s in (1.0, -1.0)]
    ks += [1.0, -1.0, 2.0 ** 62, -(2.0 ** 62), 2.0 ** 63 - 1024.0, -(2.0 ** 63)]
    for j in (1, 2):
        ks += [-float(int(moduli[j])), -2.0 * float(int(moduli[j]))]
    ks += [float(int(moduli[0])), -float(int(moduli[0]))]  # q_0 has 60 bits: the nearest double, a coefficient next to q_0
    return ks


def encoder_slots(moduli, scale, slots):
    """[len(ks)][slots] constant vectors v = k / scale (scale a power of two: the quotient is exact) and the ks"""
    ks = encoder_ks(moduli)
    assert np.log2(scale) == int(np.log2(scale))
    return np.repeat(np.array([k / scale for k in ks], dtype=np.float64)[:, None], slots, axis=1), ks


# ---------------------------------------------------------------------------------------------------------------- crafted coefficients
def double_rounding_values(Q, count=6):
    """magnitudes in [2^64, Q / 2] on which two_step and float() differ.  The low word rounds onto a multiple of 2^11 that is a tie of the
    sum's last place (2^12 there and coarser higher up), and the sum then rounds the tie to even, where one conversion of the whole value
    sees that it lies above the tie.  Found by a walk over high words and low words just above an odd multiple of the half-place; the
    caller asserts the difference again"""
    out = []
    his = [1, 2, 5, (1 << 20) + 1, (1 << 36) + 3, (Q >> 1 >> 64) - 1]
    for hi in his:
        place = max(1 << 12, 1 << ((hi << 64).bit_length() - 53))  # the unit in the last place of the sum
        for odd in (1, 3, 5, 7):
            for low in ((1 << 63) + odd * (place >> 1) + 1, odd * (place >> 1) + 1, (1 << 63) + odd * (place >> 1) - 1):
                mag = (hi << 64) + (low & MASK64)
                if TWO64 <= mag <= (Q >> 1) and two_step(mag) != float(mag):
                    out.append(mag)
                    break
            else:
                continue
            break
    assert len(out) >= 4, out
    return out[:count]


def values_nu2(moduli, delta):
    """crafted coefficient values in [0, Q), Q = q_0 q_1 (see the module docstring of tests/test_gpu_client_edges.py for what each meets)"""
    q0, q1 = int(moduli[0]), int(moduli[1])
    Q, d = q0 * q1, int(delta)
    half = Q >> 1
    v = [0, 1, half - 1, half, half + 1, Q - 2, Q - 1]
    v += [q0 - 1, q0, q0 + 1]  # r0 wraps and t changes
    v += [q1, 2 * q1, (q0 // 2) * q1, (q0 - 1) * q1]  # multiples of q_1: r1 = 0
    v += [d - 1, d, d + 1, Q - d, Q - d + 1]
    dr = double_rounding_values(Q)
    v += dr + [Q - m for m in dr]
    v += [(3 << 64) + (1 << 63), (7 << 64) + MASK64, (1 << 100) + (1 << 63) + (1 << 47) + 1]  # low word >= 2^63
    v += [(1 << 100) + (1 << 47) + 1, (1 << 90), (1 << 90) - (1 << 37)]  # the last two: 1.0 and its predecessor at scale 2^90
    assert all(0 <= a < Q for a in v)
    return v


def values_nu1(moduli, delta):
    """crafted coefficient values in [0, q_0)"""
    q0, d = int(moduli[0]), int(delta)
    half = q0 >> 1
    v = [0, 1, half - 1, half, half + 1, q0 - 1]
    v += [(1 << 53) + 1, (1 << 53) + 3, (1 << 58) + 33, q0 - (1 << 53) - 1, q0 - (1 << 58) - 33]  # above 2^53: the conversion rounds
    v += [d - 1, d, d + 1, q0 - d]
    assert all(0 <= a < q0 for a in v)
    return v


def crafted_values(moduli, delta, nu):
    return values_nu2(moduli, delta) if nu == 2 else values_nu1(moduli, delta)


def describe(a, moduli, delta, nu):
    """a crafted value by its nearest landmark, for failure messages: 'floor(Q/2)+1', 'q_0-1', ... or the number itself"""
    q0, q1, d = int(moduli[0]), int(moduli[1]), int(delta)
    top = q0 * q1 if nu == 2 else q0
    marks = {"0": 0, "floor(Q/2)" if nu == 2 else "floor(q_0/2)": top >> 1, "Q" if nu == 2 else "q_0": top, "delta": d, "Q-delta": top - d}
    if nu == 2:
        marks["q_0"] = q0
    for name, m in marks.items():
        if abs(a - m) <= 2:
            return name + ("%+d" % (a - m) if a != m else "")
    return ("2^64 x %d + 0x%016x" % (a >> 64, a & MASK64)) if a >= TWO64 else str(a)


def scales(P):
    """delta, delta^2 and the non-power-of-two delta^2 / q_11 a rescale leaves (the decoder's division is then not exact)"""
    d = float(P.delta)
    return [d, d * d, d * d / float(int(P.moduli[11]))]


def residues_of(values, moduli, nl):
    """[nl][len(values)] uint64: values mod q_j per limb"""
    return np.array([[a % int(moduli[j]) for a in values] for j in range(nl)], dtype=np.uint64)


def single_batch(values, moduli, nl, N):
    """the `single` layout as ciphertexts (NTT(t), 0): [X][2][nl][N], one value per ciphertext at coefficient 0, whose evaluation form is
    the constant a mod q_j in every position (no transform is needed)"""
    res = residues_of(values, moduli, nl)  # [nl][X]
    out = np.zeros((len(values), 2, nl, N), dtype=np.uint64)
    out[:, 0] = res.T[:, :, None]
    return out


def spread_coeff(values, moduli, nl, N, start=0):
    """the `spread` layout in coefficient form: [nl][N], the values cycled over all N coefficients (N is no multiple of the count, so both
    halves meet every value at shifting positions); `start` rotates the cycle, for batches whose ciphertexts differ"""
    idx = (np.arange(N) + start) % len(values)
    return residues_of(values, moduli, nl)[:, idx]


def spread_ct(P, values, nl, start=0):
    """the `spread` layout as a ciphertext (NTT(t), 0): ([2][nl][N] evaluation form, [nl][N] coefficient form)"""
    t = spread_coeff(values, P.moduli, nl, P.N, start)
    out = np.zeros((2, nl, P.N), dtype=np.uint64)
    for j in range(nl):
        out[0, j] = P.ntt_fwd(t[j], j)
    return out, t


def first_double_difference(got, want):
    """(count, index tuple of the first, got, want, bits) of two double arrays compared as bit patterns, or None"""
    g = np.ascontiguousarray(got, dtype=np.float64)
    w = np.ascontiguousarray(want, dtype=np.float64)
    if g.shape == w.shape and np.array_equal(g.view(np.uint64), w.view(np.uint64)):
        return None
    bad = np.argwhere(g.view(np.uint64) != w.view(np.uint64))
    at = tuple(int(v) for v in bad[0])
    return len(bad), at, float(g[at]), float(w[at]), hex(int(g.view(np.uint64)[at])), hex(int(w.view(np.uint64)[at]))
