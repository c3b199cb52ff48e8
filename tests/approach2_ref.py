"""Restatement of approach 2 (GROTE group testing) for the tests: a plain-arithmetic model on float slot vectors, and the same steps
composed from the CPU oracle's primitives (tests/oracle_lib.py) and approach 1's restatement (tests/approach1_ref.py).  TEST
INFRASTRUCTURE ONLY.  Each function cites the reference lines it follows (/root/reference).  Three conventions under FIXEDMANUAL are
derived from OpenFHE's behaviour and unverified, like DESIGN.md section 2: (a) EvalSquareInPlace and EvalMult(ct, ct) relinearise and
do not rescale; (b) a product of operands on different limb counts first drops the surplus limbs of the longer one without rescaling;
(c) MakeCKKSPackedPlaintext(v) with len(v) < slots is v zero-padded, encoded at 2^scale_bits on the ciphertext's limbs."""
import numpy as np

import approach1_ref as A
import oracle_lib as O

ALPHA_DEPTH = 2  # include/config.h:18
COMP_DEPTH = 10  # include/config.h:14


def row_length(slots):
    """pow(2, ceil(log2(slots) / 2)) (src/sender/sender_grote.cpp:18, :44)."""
    lg = slots.bit_length() - 1
    assert 1 << lg == slots
    return 1 << ((lg + 1) // 2)


def adjusted_threshold(alpha=ALPHA_DEPTH):
    """src/sender/sender_grote.cpp:55-58: MATCH_THRESHOLD squared alpha times, the same products in double."""
    t = 0.44
    for _ in range(alpha):
        t = t * t
    return t


# ------------------------------------------------------------------ plain model
def plain_power(x, alpha=ALPHA_DEPTH):
    """x^(2^alpha) x (src/sender/sender_hers.cpp:122-127): x^5 at alpha 2."""
    a = x
    for _ in range(alpha):
        a = a * a
    return a * x


def plain_rows(scores, rl, alpha=ALPHA_DEPTH):
    """alphaNormRows (src/sender/sender_hers.cpp:118-132): the row sums of x^5 over the colLength x rowLength view of every score
    vector, ciphertext i's colLength sums at flat position i colLength; flat, zero-padded to whole ciphertexts."""
    slots = len(scores[0])
    cl = slots // rl
    flat = np.zeros(-(-(len(scores) * cl) // slots) * slots)
    for i, x in enumerate(scores):
        flat[i * cl:(i + 1) * cl] = plain_power(np.asarray(x), alpha).reshape(cl, rl).sum(axis=1)
    return flat


def plain_cols(scores, rl, alpha=ALPHA_DEPTH):
    """alphaNormColumns (src/sender/sender_hers.cpp:136-178): the column sums, ciphertext i's rowLength sums at flat position i rowLength."""
    slots = len(scores[0])
    cl = slots // rl
    flat = np.zeros(-(-(len(scores) * rl) // slots) * slots)
    for i, x in enumerate(scores):
        flat[i * rl:(i + 1) * rl] = plain_power(np.asarray(x), alpha).reshape(cl, rl).sum(axis=0)
    return flat


def decode(row_vals, col_vals, slots):
    """GroteReceiver::decryptIndex's pairing (src/receiver/receiver_grote.cpp:37-62): matches are values >= 1.0, row R and column C
    pair when R div colLength == C div rowLength, index R rowLength + C mod rowLength, rows outer, columns inner."""
    rl = row_length(slots)
    cl = slots // rl
    rm = [int(i) for i in np.nonzero(np.asarray(row_vals) >= 1.0)[0]]
    cm = [int(i) for i in np.nonzero(np.asarray(col_vals) >= 1.0)[0]]
    return [r * rl + c % rl for r in rm for c in cm if r // cl == c // rl]


def plain_index(scores, alpha=ALPHA_DEPTH):
    """the index scenario on plain score vectors: a sum at or above the adjusted threshold is a match (the comparator's 2, a value
    >= 1.0 for the receiver; below it, its 0)"""
    slots = len(scores[0])
    rl, thr = row_length(slots), adjusted_threshold(alpha)
    r, c = plain_rows(scores, rl, alpha), plain_cols(scores, rl, alpha)
    return decode(np.where(r >= thr, 2.0, 0.0), np.where(c >= thr, 2.0, 0.0), slots)


def score_vectors(cos, slots):
    """n cosine scores as ceil(n / slots) zero-padded slot vectors (computeSimilarity's output layout)."""
    out = np.zeros(-(-len(cos) // slots) * slots)
    out[:len(cos)] = cos
    return list(out.reshape(-1, slots))


# ------------------------------------------------------------------ the same steps on the oracle's ciphertexts
def oracle_drop(P, ct, nl):
    """the limb prefix of ct as a ciphertext of its own (convention (b)): allocated at nl limbs, the prefix copied, the scale kept."""
    out = O.Ct(P, P.L.hyo_ct_alloc(P.h, ct.npoly, nl, ct.scale))
    out.data()[:] = ct.data()[:, :nl]
    return out


def oracle_square_norelin(P, Or, ct, nl=None):
    x = ct if nl in (None, ct.nl) else oracle_drop(P, ct, nl)
    return Or.mult_norelin(x, x)


def oracle_power(P, Or, s, alpha=ALPHA_DEPTH):
    """the prefix alphaNormRows and alphaNormColumns share (src/sender/sender_hers.cpp:122-127, :149-156): alpha x (square, relinearise,
    rescale), then the relinearised product with s on the remaining limbs, NOT rescaled."""
    a = s
    for _ in range(alpha):
        a = Or.mult_norelin(a, a)
        Or.relin(a)
        Or.rescale(a)
    p = Or.mult_norelin(a, oracle_drop(P, s, a.nl))
    Or.relin(p)
    return p


def oracle_rows_from(P, Or, products, rl):
    """src/sender/sender_hers.cpp:127-131: EvalInnerProduct's EvalSum over rowLength slots, one rescale, mergeCiphers(., rowLength)."""
    out = []
    for p in products:
        r = p.clone()
        k = 1
        while k < rl:
            Or.add(r, Or.rotate(r, k))
            k *= 2
        Or.rescale(r)
        out.append(r)
    return A.oracle_merge_ciphers(P, Or, out, rl)


def oracle_cols_from(P, Or, products, rl):
    """src/sender/sender_hers.cpp:157-174."""
    mask = np.zeros(P.slots)
    mask[:rl] = 1.0
    out = [None] * (-(-(len(products) * rl) // P.slots))
    for i, p in enumerate(products):
        c = p.clone()
        Or.rescale(c)
        j = rl
        while j < P.slots:
            Or.add(c, A.oracle_binary_rotate(P, Or, c, -j))
            j *= 2
        c = A.oracle_mult_plain(P, Or, c, mask)
        o, off = (i * rl) // P.slots, (i * rl) % P.slots
        if off == 0:
            out[o] = c
        else:
            Or.add(out[o], A.oracle_binary_rotate(P, Or, c, -off))
    return out


def oracle_rows(P, Or, scores, alpha, rl):
    return oracle_rows_from(P, Or, [oracle_power(P, Or, s, alpha) for s in scores], rl)


def oracle_cols(P, Or, scores, alpha, rl):
    return oracle_cols_from(P, Or, [oracle_power(P, Or, s, alpha) for s in scores], rl)


def oracle_index_scenario(P, Or, scores):
    """GroteSender::indexScenario after computeSimilarity (src/sender/sender_grote.cpp:50-72): (rows, columns), each compared."""
    rl, thr = row_length(P.slots), adjusted_threshold()
    products = [oracle_power(P, Or, s) for s in scores]
    rows = [Or.chebyshev_compare(c, thr, COMP_DEPTH) for c in oracle_rows_from(P, Or, products, rl)]
    cols = [Or.chebyshev_compare(c, thr, COMP_DEPTH) for c in oracle_cols_from(P, Or, products, rl)]
    return rows, cols


def oracle_decrypt_index(P, Or, rows, cols):
    """GroteReceiver::decryptIndex (src/receiver/receiver_grote.cpp:12-65)."""
    return decode(np.concatenate([Or.decrypt(c) for c in rows]), np.concatenate([Or.decrypt(c) for c in cols]), P.slots)


def fresh_scores(P, Or, z, seed, nonce0=50):
    """the rows of z as ciphertexts shaped like computeSimilarity's output: n_q - 3 limbs, scale 2^scale_bits"""
    return [oracle_drop(P, Or.encrypt(v, seed, nonce0 + i), P.nQ - 3) for i, v in enumerate(z)]


def no_shared_line(planted, slots):
    """the condition on planted matches: no two in one row or one column of one matrix (their sum would leave the comparator's [-1, 1])"""
    rl = row_length(slots)
    rows = [(i // slots, (i % slots) // rl) for i in planted]
    cols = [(i // slots, i % rl) for i in planted]
    return len(set(rows)) == len(rows) and len(set(cols)) == len(cols)
