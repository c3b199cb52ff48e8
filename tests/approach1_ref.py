"""Restatement of approach 1 (the literature baseline) for the tests: a plain-arithmetic model on float slot vectors, and the same steps
composed from the CPU oracle's primitives (tests/oracle_lib.py).  TEST INFRASTRUCTURE ONLY.  Each function cites the reference lines
it follows (/root/reference).  The order inside EvalInnerProduct (EvalMult with relinearisation, then c += Rot(c, 2^k) for ascending k,
everything at full level, the rescale last) is derived from OpenFHE's documentation and unverified, like DESIGN.md section 2."""
import ctypes as C
import math

import numpy as np

import oracle_lib as O

BASE_NONCE = 3 << 36  # database ciphertext t is encrypted with nonce BASE_NONCE + t (csrc/client.cpp HY_BASE_NONCE_BASE)


def approach1_rotations(slots):
    """{2^k} u {slots - 2^k} (src/main.cpp:195-206): every rotation of EvalSum, mergeSingleCipher and mergeCiphers decomposes into these."""
    s, k = set(), 1
    while k < slots:
        s.update((k, slots - k))
        k *= 2
    return sorted(s)


def binary_rotations(factor, slots):
    """OpenFHEWrapper::binaryRotate's greedy signed decomposition (src/openFHE_wrapper.cpp:111-121), each step mod slots."""
    out = []
    while factor != 0:
        sign = 1 if factor > 0 else -1
        bc = int(2 ** math.floor(math.log2(abs(factor)) + 0.5))  # C round(): half away from zero
        if (bc * sign) % slots:
            out.append((bc * sign) % slots)
        factor -= bc * sign
    return out


def merge_mask(slots, dim, seg):
    """generateMergeMask (src/openFHE_wrapper.cpp:253-268): ones at [k dim seg, k dim seg + seg)."""
    m = np.zeros(slots)
    for i in range(0, slots, dim * seg):
        m[i:i + seg] = 1.0
    return m


def merge_schedule(slots, dim):
    """mergeSingleCipher's loop (src/openFHE_wrapper.cpp:231-246) as a list of ("mask", seg) / ("rotadd", factor) steps."""
    vpc, padding, steps, i = slots // dim, 1, [], 1
    while i < vpc:
        if i >= padding:
            steps.append(("mask", i))
            padding = i * dim
        steps.append(("rotadd", (dim - 1) * i))
        i *= 2
    steps.append(("mask", vpc))
    return steps


def row_pack(db_normalised, slots, dim):
    """BaseEnroller::serializeDB's packing (src/enroller/enroller_base.cpp:28-44): ciphertext i = vectors i vpc .. back to back."""
    vpc = slots // dim
    n_cts = -(-db_normalised.shape[0] // vpc)
    out = np.zeros((n_cts, slots))
    flat = db_normalised.reshape(-1)
    out.reshape(-1)[:flat.size] = flat
    return out


# ------------------------------------------------------------------ plain model (numpy roll = EvalRotate, product = EvalMult)
def plain_rotate(v, factor):
    for r in binary_rotations(factor, len(v)):
        v = np.roll(v, -r)
    return v


def plain_similarity(q_tiled, v, dim):
    c = q_tiled * v
    k = 1
    while k < dim:
        c = c + np.roll(c, -k)
        k *= 2
    return c


def plain_merge_single(c, dim):
    for what, arg in merge_schedule(len(c), dim):
        c = c * merge_mask(len(c), dim, arg) if what == "mask" else c + plain_rotate(c, arg)
    return c


def plain_merge_ciphers(cs, dim):
    """OpenFHEWrapper::mergeCiphers (src/openFHE_wrapper.cpp:191-218)."""
    slots = len(cs[0])
    vpc = slots // dim
    out = [None] * (-(-(vpc * len(cs)) // slots))
    for i, c in enumerate(cs):
        m = plain_merge_single(c, dim)
        o, off = (vpc * i) // slots, (vpc * i) % slots
        out[o] = m if off == 0 else out[o] + plain_rotate(m, -off)
    return out


def plain_compute_similarity(db, query, slots, dim):
    dbn = db / np.linalg.norm(db, axis=1, keepdims=True)
    qn = np.tile(query / np.linalg.norm(query), slots // dim)
    return plain_merge_ciphers([plain_similarity(qn, v, dim) for v in row_pack(dbn, slots, dim)], dim)


# ------------------------------------------------------------------ the same steps on the oracle's ciphertexts
def oracle_mult_plain(P, Or, ct, v):
    """EvalMult(ct, MakeCKKSPackedPlaintext(v)) + RescaleInPlace (src/openFHE_wrapper.cpp:235-237).  Vectorised: the plaintext m rides as
    the "ciphertext" (m, 0), whose tensor product with ct has d0 = c0 m, d1 = c1 m (and d2 = 0) — the residue-wise products
    tests/test_gpu_approach1_ring.py::oracle_mult_plain forms one Python integer at a time."""
    m = O.Ct(P, P.L.hyo_ct_alloc(P.h, 2, ct.nl, P.delta))
    md = m.data()
    md[0] = P.encode(v, scale=P.delta, nl=ct.nl)
    md[1] = 0
    prod = Or.mult_norelin(ct, m)
    out = O.Ct(P, P.L.hyo_ct_alloc(P.h, 2, ct.nl, ct.scale * P.delta))
    out.data()[:] = prod.data()[:2]
    Or.rescale(out)
    return out


def oracle_binary_rotate(P, Or, ct, factor):
    """OpenFHEWrapper::binaryRotate (src/openFHE_wrapper.cpp:103-128)."""
    for r in binary_rotations(factor, P.slots):
        ct = Or.rotate(ct, r)
    return ct


def oracle_enroll(P, Or, db, seed):
    """BaseEnroller::serializeDB (src/enroller/enroller_base.cpp:13-56); normalises db in place."""
    for row in db:
        P.L.hyo_normalize(O._ptr(row), P.dim)
    return [Or.encrypt(v, seed, BASE_NONCE + t) for t, v in enumerate(row_pack(db, P.slots, P.dim))]


def oracle_similarity(P, Or, q, dbct):
    """computeSimilarityThread (src/sender/sender_base.cpp:84-98): EvalInnerProduct = EvalMult with relinearisation (no rescale: the
    product through hyo_mult_norelin + hyo_relin_inplace), EvalSum over dim slots, then ONE rescale."""
    c = Or.mult_norelin(q, dbct)
    Or.relin(c)
    k = 1
    while k < P.dim:
        Or.add(c, Or.rotate(c, k))
        k *= 2
    Or.rescale(c)
    return c


def oracle_merge_single(P, Or, c, dim):
    """OpenFHEWrapper::mergeSingleCipher (src/openFHE_wrapper.cpp:223-249)."""
    for what, arg in merge_schedule(P.slots, dim):
        if what == "mask":
            c = oracle_mult_plain(P, Or, c, merge_mask(P.slots, dim, arg))
        else:
            Or.add(c, oracle_binary_rotate(P, Or, c, arg))
    return c


def oracle_merge_ciphers(P, Or, cs, dim, merged=False):
    """OpenFHEWrapper::mergeCiphers (src/openFHE_wrapper.cpp:191-218); merged=True: cs went through mergeSingleCipher already."""
    vpc = P.slots // dim
    out = [None] * (-(-(vpc * len(cs)) // P.slots))
    for i, c in enumerate(cs):
        m = c if merged else oracle_merge_single(P, Or, c.clone(), dim)
        o, off = (vpc * i) // P.slots, (vpc * i) % P.slots
        if off == 0:
            out[o] = m.clone()
        else:
            Or.add(out[o], oracle_binary_rotate(P, Or, m, -off))
    return out


def oracle_compute_similarity(P, Or, q, dbcts):
    """BaseSender::computeSimilarity (src/sender/sender_base.cpp:13-27)."""
    return oracle_merge_ciphers(P, Or, [oracle_similarity(P, Or, q, d) for d in dbcts], P.dim)


def oracle_index_scenario(P, Or, q, dbcts):
    """BaseSender::indexScenario (src/sender/sender_base.cpp:69-81)."""
    return [Or.chebyshev_compare(c) for c in oracle_compute_similarity(P, Or, q, dbcts)]


def oracle_membership_from_index(P, Or, index):
    """the tail of BaseSender::membershipScenario (src/sender/sender_base.cpp:62-63): EvalAddManyInPlace, EvalSum over all slots."""
    acc = index[0].clone()
    for c in index[1:]:
        Or.add(acc, c)
    r = 1
    while r < P.slots:
        Or.add(acc, Or.rotate(acc, r))
        r *= 2
    return acc


def decrypt_index(P, Or, cts):
    """HersReceiver::decryptIndex (src/receiver/receiver_hers.cpp:37-54)."""
    return [j + i * P.slots for i, c in enumerate(cts) for j in np.nonzero(Or.decrypt(c) >= 1.0)[0]]


def stack(cts):
    return np.stack([c.data() for c in cts])
