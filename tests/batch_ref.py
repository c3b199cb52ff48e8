"""Helpers of the batch-shape and centring-boundary tests (tests/test_rescale_model_cpu.py, tests/test_gpu_batch_shapes.py): a
big-integer model of the rescale, inputs that put the value a rescale centres exactly on and around q_l / 2, and batches tiled from a
few distinct ciphertexts.  TEST INFRASTRUCTURE ONLY; no tests in here.

The rescale drops limb l = nl - 1: with y the dropped limb in coefficient form, every remaining limb j becomes
    out_j = (x_j - centred(y)) * q_l^-1 mod q_j,    centred(y) = y - q_l if y > (q_l >> 1) else y.
A wrong boundary (>= for >, a double off by one, a lost sign) moves out_j by one unit of q_l^-1 at the coefficients whose y sits next to
q_l / 2 — invisible after decryption, and hit by random residues with probability 2^-44 per coefficient."""
import numpy as np

import oracle_lib as O


def new_ct(P, npoly, nl, scale):
    """An oracle ciphertext of the given shape, zero-filled; data() is a writable view into it."""
    return O.Ct(P, P.L.hyo_ct_alloc(P.h, npoly, nl, float(scale)))


def boundary_targets(q_l, N):
    """[2][N] values of the dropped limb in coefficient form, cycling through the eight values around the centring boundary and the ends
    of the range: polynomial 0 ascending, polynomial 1 descending (so the two polynomials of a ciphertext differ)."""
    q_l = int(q_l)
    half = q_l >> 1
    cycle = np.array([0, 1, half - 1, half, half + 1, half + 2, q_l - 2, q_l - 1], dtype=np.uint64)
    i = np.arange(N) % 8
    return np.stack([cycle[i], cycle[7 - i]])


def rescale_model(P, pre, l, idx=None):
    """Python big-integer model of the rescale that drops limb l of `pre` ([npoly][>= l + 1][N], evaluation form).  Returns the expected
    result in COEFFICIENT form at the coefficients `idx` (default: all), [npoly][l][len(idx)] uint64.  Only the transforms come from the
    oracle; the arithmetic is Python integers."""
    pre = np.asarray(pre)
    idx = np.arange(P.N) if idx is None else np.asarray(idx)
    q_l = int(P.moduli[l])
    half = q_l >> 1
    out = np.zeros((pre.shape[0], l, len(idx)), dtype=np.uint64)
    for p in range(pre.shape[0]):
        y = [int(v) for v in P.ntt_inv(pre[p, l], l)[idx]]
        cen = [v - q_l if v > half else v for v in y]
        for j in range(l):
            q_j = int(P.moduli[j])
            inv = pow(q_l, -1, q_j)
            x = [int(v) for v in P.ntt_inv(pre[p, j], j)[idx]]
            out[p, j] = [((a - c) * inv) % q_j for a, c in zip(x, cen)]
    return out


def to_coeff(P, data, idx=None):
    """[npoly][nl][N] evaluation form -> coefficient form at `idx`, for a comparison with rescale_model."""
    data = np.asarray(data)
    idx = np.arange(P.N) if idx is None else np.asarray(idx)
    return np.stack([np.stack([P.ntt_inv(data[p, j], j)[idx] for j in range(data.shape[1])]) for p in range(data.shape[0])])


def relinearised(Or, a, b):
    """mult_norelin + relinearise of the oracle: the 2-component ciphertext a rescale of the product starts from."""
    d = Or.mult_norelin(a, b)
    Or.relin(d)
    return d


def craft_product_pair(P, Or, a, b):
    """Edit the oracle ciphertexts a, b (2 components, the same limb count >= 2) IN PLACE so that the relinearised product a x b holds
    boundary_targets on its last limb l, in coefficient form, at every coefficient.  On limb l, b becomes (1 in every evaluation slot, 0):
    the product there is d0 = a0, d1 = a1, d2 = 0, so the key switch (which reads d2) does not depend on a's limb l, and the relinearised
    limb is a_p + k_p.  With y0 = that limb for a's limb l zeroed, a_p's limb l = NTT(target_p - y0_p).  Returns the targets."""
    nl = a.nl
    assert nl >= 2 and b.nl == nl and a.npoly == 2 and b.npoly == 2
    l = nl - 1
    q_l = int(P.moduli[l])
    da, db = a.data(), b.data()
    db[0, l] = 1
    db[1, l] = 0
    da[:, l] = 0
    y0 = relinearised(Or, a, b)
    t = boundary_targets(q_l, P.N)
    for p in range(2):
        y = P.ntt_inv(y0.data()[p, l], l)
        da[p, l] = P.ntt_fwd((t[p] + (np.uint64(q_l) - y)) % np.uint64(q_l), l)  # (both below 2^60: no wrap)
    return t


def craft_rescale_input(P, ct):
    """Set the last limb of the 2-component oracle ciphertext ct IN PLACE to NTT(boundary_targets); returns the targets."""
    assert ct.npoly == 2 and ct.nl >= 2
    l = ct.nl - 1
    t = boundary_targets(P.moduli[l], P.N)
    d = ct.data()
    for p in range(2):
        d[p, l] = P.ntt_fwd(t[p], l)
    return t


def saturate(P, ct):
    """every residue of ct = q_j - 1, in place"""
    d = ct.data()
    for j in range(ct.nl):
        d[:, j] = P.moduli[j] - np.uint64(1)
    return ct


def randomise(P, ct, rng):
    """every residue of ct uniform below q_j, in place"""
    d = ct.data()
    for j in range(ct.nl):
        d[:, j] = rng.integers(0, int(P.moduli[j]), size=(ct.npoly, P.N), dtype=np.uint64)
    return ct


def mult_chain(Or, a, b, limb_counts):
    """{nl: (a_nl, b_nl)} from the oracle's own products: a_k+1 = a_k^2, b_k+1 = a_k b_k (each one limb shorter), cloned at the limb counts
    asked for so that the caller may edit them."""
    want, out = set(limb_counts), {}
    assert max(want) <= a.nl and min(want) >= 1
    while True:
        if a.nl in want:
            out[a.nl] = (a.clone(), b.clone())
        if a.nl == min(want):
            return out
        a, b = Or.mult(a, a), Or.mult(a, b)


def tile(distinct, X, expected=None):
    """A batch of X ciphertexts from the D distinct ones ([D][...]): position i holds distinct[i % D], and the last position holds
    distinct[D - 1] where it would repeat position 0 — so the first, the last, an odd and an even slot of the batch hold different data.
    Returns (batch, expected tiled the same way or None, the source index of every position)."""
    D = len(distinct)
    src = [i % D for i in range(X)]
    if X > 1 and src[-1] == 0:
        src[-1] = D - 1
    return distinct[src], None if expected is None else expected[src], src
