"""Seeded keys and seeded secret-key queries (include/hydia.h, hydia_keygen_seeded / hydia_encrypt_query_seeded) restated on the CPU
oracle.  TEST INFRASTRUCTURE ONLY: nothing here touches the product.

  seeded_key    oracle/ckks.c's gen_evk with every a from the uniform stream (EVK_A, id, d, m) under the PUBLIC a_seed and every e from
                the Gaussian stream (EVK_E, id, d, 0) under the secret seed, in the equivalent form that anchors e and P s_from in the
                oracle's own key:  b = b_oracle + (a_oracle - a_seeded) s_enc mod q   (b_oracle = e - a_oracle s_enc + [digit] P s_from)
  seeded_pk     the same for the public key: a from (PK_A, 0, 0, j) under a_seed
  seeded_query  c0 = NTT(e0 + m) - a s, c1 = a: m the encoded tiled normalised probe, e0 from (ENC_E0, nonce, 0, 0) under seed, a limb j
                from (SYM_A = 9, nonce, 0, j) under a_seed
  install       the oracle key set's own arrays overwritten in place with the seeded ones: the whole oracle sender then runs under them
"""
import numpy as np

import oracle_lib as O
from db_rekey_ref import _ints, _u64, stream

DOM_PK_A, DOM_EVK_A, DOM_ENC_E0, DOM_SYM_A = 2, 4, 7, 9


def mulmod(a, b, q):
    """a b mod q on uint64 arrays of canonical residues, q < 2^60, without leaving uint64: b is taken four bits at a time from the top,
    r <- 16 r + a nibble (mod q) — every intermediate is below 2^64 (16 r < 2^64, a nibble < 2^64, and each is reduced before the sum).
    A whole key set is restated with this; test_seeded_cpu.py holds it against Python-integer arithmetic"""
    a, b, q = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64), np.uint64(q)
    assert int(q) < 1 << 60
    r = np.zeros_like(a)
    for shift in range(56, -1, -4):
        nib = (b >> np.uint64(shift)) & np.uint64(15)
        r = ((r * np.uint64(16)) % q + (a * nib) % q) % q
    return r


def rebase(b_or, a_or, a, s, q):
    """b_or + (a_or - a) s mod q, uint64 arrays of canonical residues"""
    q64 = np.uint64(q)
    diff = (a_or + (q64 - a)) % q64
    return (b_or + mulmod(diff, s, q)) % q64


def rotated_secret(P, K, r):
    """s_enc of rotation key r: sigma_{g^-1}(s), g = 5^r, on all nT limbs (what hyo_keygen encrypts key r under)"""
    ginv = pow(P.galois(r), -1, 2 * P.N)
    s = K.s_ntt()
    return np.stack([P.automorph_eval(s[m], ginv) for m in range(P.nT)])


def seeded_key(P, K, seed, a_seed, key_id, s_enc, s_from=None):
    """[dnum][2][nT][N]: key `key_id` (0: relinearisation, r: rotation r) of the oracle key set K = O.Keys(P, seed), re-based onto the
    uniform halves of a_seed.  s_enc [nT][N]: the secret the key encrypts under.  s_from is what the key switches from; it enters only
    through the oracle's own b (the P s_from term is the same in both keys), so it is accepted and not read."""
    base = K.relin() if key_id == 0 else K.rot_key(key_id)
    out = np.zeros_like(base)
    for d in range(P.dnum):
        for m in range(P.nT):
            q = int(P.moduli[m])
            a_or = O.sample_uniform(seed, stream(DOM_EVK_A, key_id, d, m), q, P.N)
            assert np.array_equal(a_or, base[d, 1, m])  # the oracle's key is what this restatement is anchored in
            a = O.sample_uniform(a_seed, stream(DOM_EVK_A, key_id, d, m), q, P.N)
            out[d, 1, m] = a
            out[d, 0, m] = rebase(base[d, 0, m], a_or, a, s_enc[m], q)
    return out


def seeded_relin(P, K, seed, a_seed):
    return seeded_key(P, K, seed, a_seed, 0, K.s_ntt())


def seeded_rot(P, K, seed, a_seed, r):
    return seeded_key(P, K, seed, a_seed, r, rotated_secret(P, K, r), K.s_ntt())


def seeded_pk(P, K, seed, a_seed):
    """[2][nQ][N]: (b, a) = (e - a s, a) with a under a_seed and the oracle's own e"""
    base, s = K.pk(), K.s_ntt()
    out = np.zeros_like(base)
    for j in range(P.nQ):
        q = int(P.moduli[j])
        a_or = O.sample_uniform(seed, stream(DOM_PK_A, 0, 0, j), q, P.N)
        assert np.array_equal(a_or, base[1, j])
        a = O.sample_uniform(a_seed, stream(DOM_PK_A, 0, 0, j), q, P.N)
        out[1, j] = a
        out[0, j] = rebase(base[0, j], a_or, a, s[j], q)
    return out


def tiled_probe(P, query):
    """the slot vector DiagonalReceiver::encryptQuery encrypts: the probe divided by its L2 norm (a zero probe passes through), tiled"""
    qn = np.ascontiguousarray(query, dtype=np.float64).copy()
    P.L.hyo_normalize(O._ptr(qn), P.dim)
    return np.tile(qn, P.slots // P.dim)


def seeded_query(P, K, query, seed, a_seed, nonce):
    """(c0, a), each [nQ][N]"""
    m = P.encode_coeffs(tiled_probe(P, query))
    e0 = O.sample_gauss(seed, stream(DOM_ENC_E0, nonce, 0, 0), P.N)
    t = _ints(m) + _ints(e0)
    s = K.s_ntt()
    c0, a = np.zeros((P.nQ, P.N), dtype=np.uint64), np.zeros((P.nQ, P.N), dtype=np.uint64)
    for j in range(P.nQ):
        q = int(P.moduli[j])
        a[j] = O.sample_uniform(a_seed, stream(DOM_SYM_A, nonce, 0, j), q, P.N)
        t0 = P.ntt_fwd(_u64(t % q), j)
        c0[j] = (t0 + (np.uint64(q) - mulmod(a[j], s[j], q))) % np.uint64(q)
    return c0, a


def install(K, P, seed, a_seed, rotations=None):
    """overwrite K's public key, relinearisation key and rotation keys (all of K.rotations, or `rotations`) in place with their seeded
    forms; returns {id: key} of what was installed (0 = relinearisation) and the public key"""
    rots = list(K.rotations if rotations is None else rotations)
    keys = {0: seeded_relin(P, K, seed, a_seed)}
    for r in rots:
        keys[r] = seeded_rot(P, K, seed, a_seed, r)
    pk = seeded_pk(P, K, seed, a_seed)
    K.pk()[...] = pk
    K.relin()[...] = keys[0]
    for r in rots:
        K.rot_key(r)[...] = keys[r]
    return keys, pk
