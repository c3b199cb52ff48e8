"""The semantics of re-keying a resident database (include/hydia.h, hydia_keygen_switch / hydia_db_rekey) restated on the CPU oracle.
TEST INFRASTRUCTURE ONLY: nothing here touches the product.

  switch_key   the hybrid switching key from the old secret to the new one, digit d:
                   (b_d, a_d) = (-a_d s_new + NTT(e_d) + P [limb in digit d] s_old, a_d),  [dnum][2][nT][N], evaluation form
               a_d limb m from the uniform stream (EVK_A, id, d, m), e_d from the Gaussian stream (EVK_E, id, d, 0), id = 2^24 —
               oracle/ckks.c's gen_evk restated with the oracle's samplers and transform and Python-integer arithmetic
  rekey        every ciphertext (c0, c1) on all n_q limbs := (c0 + ks0, ks1), (ks0, ks1) = hyo_keyswitch(c1, n_q, key)
"""
import numpy as np

import oracle_lib as O
from keyswitch_ref import _ints, _u64, oracle_keyswitch

DOM_EVK_A, DOM_EVK_E = 4, 5
EVK_ID_SWITCH = 1 << 24


def stream(dom, a, b, c):
    """HY_STREAM of oracle/hydia_oracle.h"""
    return (dom << 56) | (a << 16) | (b << 8) | c


def switch_key_parts(P, K_old, K_new, seed):
    """(key [dnum][2][nT][N] uint64, e [dnum][N] int32): the key and the Gaussian errors it was made with"""
    q = [int(v) for v in P.moduli]
    PP = 1
    for m in range(P.nQ, P.nT):
        PP *= q[m]
    s_new, s_old = K_new.s_ntt(), K_old.s_ntt()
    key = np.zeros((P.dnum, 2, P.nT, P.N), dtype=np.uint64)
    errs = np.zeros((P.dnum, P.N), dtype=np.int32)
    for d in range(P.dnum):
        e = O.sample_gauss(seed, stream(DOM_EVK_E, EVK_ID_SWITCH, d, 0), P.N)
        errs[d] = e
        for m in range(P.nT):
            a = O.sample_uniform(seed, stream(DOM_EVK_A, EVK_ID_SWITCH, d, m), q[m], P.N)
            e_ntt = P.ntt_fwd(_u64(_ints(e) % q[m]), m)
            v = _ints(e_ntt) - _ints(a) * _ints(s_new[m])
            if m < P.nQ and m // P.alpha == d:
                v = v + (PP % q[m]) * _ints(s_old[m])
            key[d, 0, m] = _u64(v % q[m])
            key[d, 1, m] = a
    return key, errs


def switch_key(P, K_old, K_new, seed):
    return switch_key_parts(P, K_old, K_new, seed)[0]


def rekey_ct(P, data, key):
    """one ciphertext [2][n_q][N] (uint64, evaluation form) under the switching key: a new array [2][n_q][N]"""
    data = np.asarray(data)
    assert data.shape == (2, P.nQ, P.N)
    k0, k1 = oracle_keyswitch(P, data[1], P.nQ, key)
    out = np.zeros_like(data)
    for j in range(P.nQ):
        qj = P.moduli[j]  # c0 + ks0 < 2 q_j < 2^61: no wrap in uint64
        s = data[0, j] + k0[j]
        out[0, j] = np.where(s >= qj, s - qj, s)
    out[1] = k1
    return out


def rekey(P, cts, key):
    """cts: arrays [2][n_q][N] (or oracle ciphertexts; None entries pass through) -> list of re-keyed arrays"""
    return [None if c is None else rekey_ct(P, c.data() if hasattr(c, "data") and callable(c.data) else c, key) for c in cts]


def as_oracle_cts(P, Or, arrays, scale=None):
    """oracle ciphertexts holding the given [2][n_q][N] arrays (for the oracle's sender and decrypt methods)"""
    out = []
    for a in arrays:
        c = O.Ct(P, P.L.hyo_ct_alloc(P.h, 2, P.nQ, P.delta if scale is None else scale))
        c.data()[...] = a
        out.append(c)
    return out
