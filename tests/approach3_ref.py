"""Restatement of approach 3 (the Blind-Match method) for the tests: a plain-arithmetic model on float slot vectors, and the same steps
composed from the CPU oracle's primitives (tests/oracle_lib.py).  TEST INFRASTRUCTURE ONLY.  Each function cites the reference lines
it follows (/root/reference).  Nothing here needs a convention beyond those tests/approach1_ref.py already uses."""
import numpy as np

import oracle_lib as O
from approach1_ref import binary_rotations, oracle_binary_rotate, oracle_mult_plain, plain_rotate, stack  # noqa: F401

BLIND_NONCE = 1 << 38  # database ciphertext t = m K + c is encrypted with nonce BLIND_NONCE + t (csrc/client.cpp HY_BLIND_NONCE_BASE)
CHUNK_LEN = 128        # include/config.h:34


def chunk_pack(db_normalised, slots, chunk):
    """BlindEnroller::serializeDBThread (src/enroller/enroller_blind.cpp:66-80): image [m][c] holds coordinates [c chunk, (c + 1) chunk)
    of vector m spb + v at slots [v chunk, (v + 1) chunk), zeros elsewhere."""
    n, dim = db_normalised.shape
    spb, K = slots // chunk, dim // chunk
    M = -(-n // spb)
    out = np.zeros((M, K, slots))
    for m in range(M):
        rows = db_normalised[m * spb:(m + 1) * spb]
        for c in range(K):
            out[m, c, :rows.shape[0] * chunk] = rows[:, c * chunk:(c + 1) * chunk].reshape(-1)
    return out


def query_tiles(query_normalised, slots, chunk):
    """BlindReceiver::encryptQueryThread (src/receiver/receiver_blind.cpp:58-67): image c = chunk c tiled over all slots."""
    K = len(query_normalised) // chunk
    return np.stack([np.tile(query_normalised[c * chunk:(c + 1) * chunk], slots // chunk) for c in range(K)])


def compress_mask(slots, dimension):
    """the one-hot mask of compressCiphers (src/openFHE_wrapper.cpp:279-283)."""
    m = np.zeros(slots)
    m[::dimension] = 1.0
    return m


def decode_index(values, slots, chunk):
    """BlindReceiver::decryptIndex (src/receiver/receiver_blind.cpp:28-54) on decrypted slot values [outputs][slots]; like the
    reference it does not filter indices that fall into the padding."""
    spb = slots // chunk
    return [i * slots + j // chunk + (j % chunk) * spb for i, v in enumerate(values) for j in np.nonzero(v >= 1.0)[0]]


def score_slot(index, slots, chunk):
    """where decode_index finds vector `index`: (output ciphertext, slot) — the inverse of the decode formula."""
    spb = slots // chunk
    i, rest = divmod(index, slots)
    k, v = divmod(rest, spb)
    return i, v * chunk + k


# ------------------------------------------------------------------ plain model (numpy roll = EvalRotate, product = EvalMult)
def plain_similarity_matrix(q_tiles, images, chunk):
    """computeSimilarityMatrix (src/sender/sender_blind.cpp:59-83)."""
    acc = q_tiles[0] * images[0]
    for c in range(1, len(q_tiles)):
        acc = acc + q_tiles[c] * images[c]
    r = 1
    while r < chunk:
        acc = acc + plain_rotate(acc, r)
        r *= 2
    return acc


def plain_compress(cs, dimension):
    """OpenFHEWrapper::compressCiphers (src/openFHE_wrapper.cpp:273-312)."""
    slots = len(cs[0])
    out = [None] * (-(-len(cs) // dimension))
    mask = compress_mask(slots, dimension)
    for i, c in enumerate(cs):
        m = c * mask
        k = i % dimension
        out[i // dimension] = m if k == 0 else out[i // dimension] + plain_rotate(m, -k)
    return out


def plain_compute_similarity(db, query, slots, chunk):
    """BlindSender::computeSimilarity (src/sender/sender_blind.cpp:43-56) on plain vectors."""
    dbn = db / np.linalg.norm(db, axis=1, keepdims=True)
    qt = query_tiles(query / np.linalg.norm(query), slots, chunk)
    return plain_compress([plain_similarity_matrix(qt, images, chunk) for images in chunk_pack(dbn, slots, chunk)], chunk)


# ------------------------------------------------------------------ the same steps on the oracle's ciphertexts
def oracle_enroll(P, Or, db, chunk, seed):
    """BlindEnroller::serializeDB (src/enroller/enroller_blind.cpp:13-90); normalises db in place.  Returns [m][c]."""
    for row in db:
        P.L.hyo_normalize(O._ptr(row), P.dim)
    K = P.dim // chunk
    return [[Or.encrypt(v, seed, BLIND_NONCE + m * K + c) for c, v in enumerate(images)] for m, images in enumerate(chunk_pack(db, P.slots, chunk))]


def oracle_encrypt_query(P, Or, query, chunk, seed, nonce0=1):
    """BlindReceiver::encryptQuery (src/receiver/receiver_blind.cpp:13-26): normalise, K tiled ciphertexts, nonces nonce0 + c."""
    q = np.array(query, dtype=np.float64)
    P.L.hyo_normalize(O._ptr(q), P.dim)
    return [Or.encrypt(v, seed, nonce0 + c) for c, v in enumerate(query_tiles(q, P.slots, chunk))]


def oracle_dot_norelin(P, Or, qs, cts):
    """the sum of EvalMultNoRelin products of computeSimilarityMatrix (src/sender/sender_blind.cpp:65-71), ascending c."""
    acc = Or.mult_norelin(qs[0], cts[0])
    for c in range(1, len(qs)):
        Or.add(acc, Or.mult_norelin(qs[c], cts[c]))
    return acc


def oracle_similarity_matrix(P, Or, qs, cts, chunk):
    """computeSimilarityMatrix (src/sender/sender_blind.cpp:59-83): the sum, RelinearizeInPlace, RescaleInPlace, then
    acc += binaryRotate(acc, r) for r = 1, 2, 4, .. < chunk."""
    acc = oracle_dot_norelin(P, Or, qs, cts)
    Or.relin(acc)
    Or.rescale(acc)
    r = 1
    while r < chunk:
        Or.add(acc, oracle_binary_rotate(P, Or, acc, r))
        r *= 2
    return acc


def oracle_compress(P, Or, cs, dimension):
    """OpenFHEWrapper::compressCiphers (src/openFHE_wrapper.cpp:273-312): the mask multiply with its rescale (the RelinearizeInPlace
    between them is a no-op on two components), then ciphertext i into output i div dimension, rotated by -(i mod dimension)."""
    mask = compress_mask(P.slots, dimension)
    out = [None] * (-(-len(cs) // dimension))
    for i, c in enumerate(cs):
        m = oracle_mult_plain(P, Or, c, mask)
        k = i % dimension
        if k == 0:
            out[i // dimension] = m
        else:
            Or.add(out[i // dimension], oracle_binary_rotate(P, Or, m, -k))
    return out


def oracle_compute_similarity(P, Or, qs, dbcts, chunk):
    """BlindSender::computeSimilarity (src/sender/sender_blind.cpp:43-56)."""
    return oracle_compress(P, Or, [oracle_similarity_matrix(P, Or, qs, cts, chunk) for cts in dbcts], chunk)


def oracle_index_scenario(P, Or, scores):
    """BlindSender::indexScenario (src/sender/sender_blind.cpp:30-41) from computeSimilarity's result."""
    return [Or.chebyshev_compare(c) for c in scores]
