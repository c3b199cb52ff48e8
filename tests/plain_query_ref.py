"""The specification of a plain query (include/hydia.h, hydia_encode_query / hydia_*_pq) restated on the CPU oracle.
TEST INFRASTRUCTURE ONLY: nothing here touches the product.

A plain query is, bit for bit, the oracle's existing sender path run on the TRIVIAL ciphertext (c0, c1) = (m, 0):
  - m = P.encode(tiled, normalised query): what hyo_encrypt_query encrypts — scale 2^scale_bits, all n_q limbs, evaluation form;
  - hyo_rotate of (m, 0) is (sigma_r(m), 0) exactly (the key switch of the zero polynomial is zero), hyo_mult_norelin of it with a
    database ciphertext has d2 = 0 and hyo_relin_inplace leaves d0, d1 (tests/test_plain_query_cpu.py), so
    hyo_compute_similarity[_bsgs], hyo_index_scenario[_bsgs] and hyo_membership_scenario[_bsgs] on (m, 0) are what the product
    must return.
"""
import numpy as np

import oracle_lib as O
from plain_gallery_ref import _CtList, pattern_ct, pattern_poly, trivial_ct  # noqa: F401  (pattern_poly: re-exported for the tests)


def query_poly(P, query):
    """[n_q][N] residues of the probe's plaintext: hyo_normalize, tiled to all slots, encoded at 2^scale_bits on all limbs"""
    q = np.ascontiguousarray(query, dtype=np.float64).copy()
    assert q.shape == (P.dim,)
    P.L.hyo_normalize(O._ptr(q), P.dim)
    return P.encode(np.tile(q, P.slots // P.dim))


def trivial_query(P, query):
    """the trivial ciphertext (encode(tiled normalised query), 0) the oracle's sender methods take in place of an encrypted query"""
    return trivial_ct(P, query_poly(P, query))


def pattern_query(P, name):
    """the trivial ciphertext of a pattern polynomial (plain_gallery_ref.pattern_poly) at scale 2^scale_bits"""
    return trivial_ct(P, pattern_poly(P, name))


def pattern_db(P, name, n_cts):
    """an encrypted-database stand-in of n_cts identical ciphertexts whose two polynomials both carry the pattern (one oracle
    ciphertext, shared: the sender only reads); hoisted form"""
    return _CtList([pattern_ct(P, name)] * n_cts, P.dim, P.dim)


def ct_list(cts, dim, babies=None):
    """a database for the oracle's sender methods from a Python list of oracle ciphertexts (shared entries allowed)"""
    return _CtList(list(cts), dim, dim if babies is None else int(babies))
