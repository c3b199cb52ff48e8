"""A seeded database delta (include/hydia.h, "seeded database deltas") restated on the CPU oracle and in the format's own words.  TEST
INFRASTRUCTURE ONLY: nothing here touches the product.

  seeded_ct     one database ciphertext under the SECRET key: c0 = NTT(e0 + m) - a s, c1 = a; m the encoded slot image, e0 from the
                Gaussian stream (ENC_E0, e_nonce, 0, 0) under the secret seed (the enrolment's nonce, 2^36 + (first_block + g) dim + i),
                a limb j from the uniform stream (SYM_A = 9, a_nonce, 0, j) under the PUBLIC a_seed, a_nonce = (first_block + g) dim + i
  seeded_blocks per touched block g the dim ciphertexts of the sparse diagonal image of the rows (db_update_ref.UpdateRef.image)
  build         the container: db_delta_ref's 64-byte header under the magic HYDDELS1, then one type 2 wire message per block
  fold          old + E mod q_j for a block that existed, E for a new one
"""
import numpy as np

import db_delta_ref as DR
import oracle_lib as O
import wire_ref as W
from db_update_ref import DB_NONCE_BASE, UpdateRef
from keyswitch_ref import _ints, _u64
from seeded_ref import DOM_ENC_E0, DOM_SYM_A, mulmod, stream

MAGIC = b"HYDDELS1"


def block_nonce(first_block, g, dim):
    """nonce0 of the message of block g: the enrolment's offset of that block's ciphertext 0"""
    return (first_block + g) * dim


def noisy_plaintext(P, image, seed, e_nonce):
    """NTT(e0 + m) on every Q limb, [nQ][N]: what c0 + a s of a seeded ciphertext must equal bit for bit"""
    m = P.encode_coeffs(image)
    e0 = O.sample_gauss(seed, stream(DOM_ENC_E0, e_nonce, 0, 0), P.N)
    t = _ints(m) + _ints(e0)
    return np.stack([P.ntt_fwd(_u64(t % int(P.moduli[j])), j) for j in range(P.nQ)])


def expand_a(P, a_seed, a_nonce):
    """[nQ][N]: limb j = the uniform stream (9, a_nonce, 0, j) under a_seed — what hydia_ct_expand_seeded makes of a query"""
    return np.stack([O.sample_uniform(a_seed, stream(DOM_SYM_A, a_nonce, 0, j), int(P.moduli[j]), P.N) for j in range(P.nQ)])


def seeded_ct(P, K, image, seed, a_seed, e_nonce, a_nonce):
    """(c0, a), each [nQ][N]"""
    t0, a, s = noisy_plaintext(P, image, seed, e_nonce), expand_a(P, a_seed, a_nonce), K.s_ntt()
    c0 = np.zeros_like(a)
    for j in range(P.nQ):
        q = int(P.moduli[j])
        c0[j] = (t0[j] + (np.uint64(q) - mulmod(a[j], s[j], q))) % np.uint64(q)
    return c0, a


def placed(P, first_vector, rows, normalise):
    """the zero matrix with the rows (normalised in place when asked) at their vector indices, and the blocks they touch"""
    n = rows.shape[0]
    if normalise:
        for v in range(n):
            P.L.hyo_normalize(O._ptr(rows[v]), P.dim)
    touched = DR.touched_blocks(first_vector, n, P.slots)
    Z = np.zeros(((touched[-1] + 1) * P.slots, P.dim), dtype=np.float64)
    Z[first_vector:first_vector + n] = rows
    return Z, touched


def seeded_blocks(P, K, B, first_vector, rows, normalise, seed, a_seed, first_block=0):
    """-> (touched blocks, [per block: ciphertexts [dim][2][nQ][N]])"""
    U = UpdateRef(P, None, babies=B)
    Z, touched = placed(P, first_vector, rows, normalise)
    out = []
    for g in touched:
        cts = np.zeros((P.dim, 2, P.nQ, P.N), dtype=np.uint64)
        for i in range(P.dim):
            a_nonce = block_nonce(first_block, g, P.dim) + i
            cts[i, 0], cts[i, 1] = seeded_ct(P, K, U.image(Z, g * P.dim + i), seed, a_seed, DB_NONCE_BASE + a_nonce, a_nonce)
        out.append(cts)
    return touched, out


def message_bytes(n, vector_dim, moduli):
    """one block's message: vector_dim c0 halves on every limb"""
    return W.HEADER_BYTES + W.payload_bytes(n, vector_dim, 1, [int(q) for q in moduli])


def total_bytes(n, vector_dim, moduli, first_vector, n_rows):
    return DR.HEADER_BYTES + len(DR.touched_blocks(first_vector, n_rows, n // 2)) * message_bytes(n, vector_dim, moduli)


def container(vector_dim, babies, first_vector, n_rows, first_block, messages, **over):
    return DR.container(vector_dim, babies, first_vector, n_rows, first_block, messages, **{"magic": MAGIC, **over})


def build(blocks, touched, moduli, scale, babies, first_vector, n_rows, a_seed, first_block=0):
    """blocks: per touched block [dim][2][nQ][N] (component 1 does not travel) -> the seeded delta"""
    dim = blocks[0].shape[0]
    seed32 = bytes(O.seed_bytes(a_seed))
    msgs = [W.query_message(b[:, 0], moduli, scale, seed32, block_nonce(first_block, g, dim)) for g, b in zip(touched, blocks)]
    return container(dim, babies, first_vector, n_rows, first_block, msgs)


def split(data):
    """-> (header dict, [the bytes of each message]); asserts the exact length"""
    data = bytes(data)
    h = DR.parse_header(data)
    assert h["magic"] == MAGIC
    off, out = DR.HEADER_BYTES, []
    for _ in range(h["n_blocks"]):
        m = W.parse_header(data[off:off + W.HEADER_BYTES])
        end = off + W.HEADER_BYTES + m["payload_bytes"]
        assert end <= len(data)
        out.append(data[off:end])
        off = end
    assert off == len(data)
    return h, out


def fold(P, old, E):
    """old + E mod q_j on [.. ][nQ][N] arrays of canonical residues (old None: a new block, E itself)"""
    if old is None:
        return E.copy()
    out = np.zeros_like(E)
    for j in range(P.nQ):
        q = np.uint64(int(P.moduli[j]))
        out[..., j, :] = (old[..., j, :] + E[..., j, :]) % q  # both < q < 2^60: no wrap in uint64
    return out
