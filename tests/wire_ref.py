"""The wire format of include/hydia.h ("wire messages") restated in numpy, from the format's own words: a 360-byte little-endian
header, then rows in the order [count][poly][limb]; residue c of a row occupies bits [c w, (c + 1) w) of the row read as one
little-endian bit string, w = the bit length of the limb's modulus.  The tests compare the product's bytes with these, never with the
product's own output.  Nothing here imports the product."""
import struct

import numpy as np

HEADER_BYTES = 360
FILE_HEADER_BYTES = 16
MAGIC, FILE_MAGIC = b"HYDWIRE1", b"HYDKEYS1"
CT_BATCH, SEEDED_QUERY, EVAL_KEY, EVAL_KEY_SEEDED, PUBLIC_KEY, PUBLIC_KEY_SEEDED = 1, 2, 3, 4, 5, 6
_HEADER = "<8s6IQd32sQQQ32Q"
assert struct.calcsize(_HEADER) == HEADER_BYTES


def width(q):
    return int(q).bit_length()


def pack_row(residues, w):
    """N uint64 residues -> N w / 8 bytes: the low w bits of each, one after the other, as one little-endian bit string"""
    r = np.ascontiguousarray(residues, dtype="<u8")
    bits = np.unpackbits(r.view(np.uint8).reshape(-1, 8), axis=1, bitorder="little")  # [N][64], bit 0 first
    return np.packbits(bits[:, :w].reshape(-1), bitorder="little").tobytes()


def unpack_row(data, w, n):
    bits = np.unpackbits(np.frombuffer(data, dtype=np.uint8), bitorder="little").reshape(n, w)
    full = np.zeros((n, 64), dtype=np.uint8)
    full[:, :w] = bits
    return np.packbits(full, axis=1, bitorder="little").view("<u8").reshape(n).astype(np.uint64)


def row_bytes(n, q):
    return n * width(q) // 8


def payload_bytes(n, count, n_polys, moduli):
    return count * n_polys * sum(row_bytes(n, q) for q in moduli)


def header(mtype, log_n, count, n_polys, moduli, rot=0, scale=0.0, a_seed=bytes(32), nonce0=0, payload=None, version=1, reserved=0,
           magic=MAGIC, n_limbs=None):
    """the 360 bytes; payload / n_limbs override what the shape implies (for refusal tests)"""
    mods = [int(q) for q in moduli]
    if payload is None:
        payload = payload_bytes(1 << log_n, count, n_polys, mods)
    return struct.pack(_HEADER, magic, version, mtype, log_n, n_polys, len(mods) if n_limbs is None else n_limbs, rot, count, scale,
                       bytes(a_seed), nonce0, payload, reserved, *(mods + [0] * (32 - len(mods))))


def parse_header(data):
    f = struct.unpack(_HEADER, data[:HEADER_BYTES])
    keys = ("magic", "version", "type", "log_n", "n_polys", "n_limbs", "rot", "count", "scale", "a_seed", "nonce0", "payload_bytes", "reserved")
    d = dict(zip(keys, f[:13]))
    d["moduli"] = list(f[13:])
    return d


def payload(rows, moduli):
    """rows [count][poly][limb][N] uint64 -> the packed payload"""
    rows = np.asarray(rows, dtype=np.uint64)
    assert rows.ndim == 4 and rows.shape[2] == len(moduli)
    return b"".join(pack_row(rows[x, p, j], width(moduli[j])) for x in range(rows.shape[0]) for p in range(rows.shape[1])
                    for j in range(rows.shape[2]))


def message(mtype, rows, moduli, rot=0, scale=0.0, a_seed=bytes(32), nonce0=0):
    rows = np.asarray(rows, dtype=np.uint64)
    count, n_polys, _, n = rows.shape
    log_n = n.bit_length() - 1
    return header(mtype, log_n, count, n_polys, moduli, rot, scale, a_seed, nonce0) + payload(rows, moduli)


def unpack_message(data):
    """-> (header dict, rows [count][poly][limb][N])"""
    h = parse_header(data)
    n, mods = 1 << h["log_n"], h["moduli"][:h["n_limbs"]]
    rows = np.zeros((h["count"], h["n_polys"], h["n_limbs"], n), dtype=np.uint64)
    off = HEADER_BYTES
    for x in range(h["count"]):
        for p in range(h["n_polys"]):
            for j, q in enumerate(mods):
                nb = row_bytes(n, q)
                rows[x, p, j] = unpack_row(data[off:off + nb], width(q), n)
                off += nb
    assert off == len(data)
    return h, rows


def ct_message(cts, moduli, scale):
    """ciphertext batch [count][poly][limb][N] -> a type 1 message"""
    cts = np.asarray(cts, dtype=np.uint64)
    return message(CT_BATCH, cts, moduli[:cts.shape[2]], scale=scale)


def query_message(c0, moduli, scale, a_seed, nonce0):
    """c0 [count][n_q][N] -> a type 2 message"""
    c0 = np.asarray(c0, dtype=np.uint64)
    return message(SEEDED_QUERY, c0[:, None], moduli[:c0.shape[1]], scale=scale, a_seed=a_seed, nonce0=nonce0)


def eval_key_message(key, moduli, rot, a_seed=None):
    """key [dnum][2][n_q + n_p][N]; a_seed given: the seeded message of its b halves"""
    key = np.asarray(key, dtype=np.uint64)
    if a_seed is None:
        return message(EVAL_KEY, key, moduli, rot=rot)
    return message(EVAL_KEY_SEEDED, key[:, :1], moduli, rot=rot, a_seed=a_seed)


def public_key_message(pk, moduli, a_seed=None):
    """pk [2][n_q][N]"""
    pk = np.asarray(pk, dtype=np.uint64)
    mods = moduli[:pk.shape[1]]
    if a_seed is None:
        return message(PUBLIC_KEY, pk[None], mods)
    return message(PUBLIC_KEY_SEEDED, pk[None, :1], mods, a_seed=a_seed)


def file_header(n_messages):
    return FILE_MAGIC + struct.pack("<II", 1, n_messages)
