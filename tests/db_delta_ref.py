"""The container of a database delta (include/hydia.h, "database deltas") restated in Python from the format's own words: a 64-byte
little-endian header, then n_blocks type 1 wire messages (tests/wire_ref.py) back to back, nothing after the last.  The tests compare
the product's bytes with these, never with the product's own output.  Nothing here imports the product."""
import struct

import numpy as np

import wire_ref as W

HEADER_BYTES = 64
MAGIC = b"HYDDELT1"
_HEADER = "<8sII6Q"
assert struct.calcsize(_HEADER) == HEADER_BYTES
FIELDS = ("magic", "version", "vector_dim", "babies", "first_vector", "n_rows", "first_block", "n_blocks", "reserved")


def touched_blocks(first_vector, n_rows, slots):
    """the blocks of `slots` vectors that vectors first_vector .. first_vector + n_rows - 1 lie in"""
    assert n_rows >= 1
    return list(range(first_vector // slots, (first_vector + n_rows - 1) // slots + 1))


def header(vector_dim, babies, first_vector, n_rows, first_block, n_blocks, version=1, reserved=0, magic=MAGIC):
    return struct.pack(_HEADER, magic, version, vector_dim, babies, first_vector, n_rows, first_block, n_blocks, reserved)


def parse_header(data):
    return dict(zip(FIELDS, struct.unpack(_HEADER, bytes(data[:HEADER_BYTES]))))


def message_bytes(n, vector_dim, moduli):
    """one block's message: vector_dim ciphertexts of two polynomials on every limb"""
    return W.HEADER_BYTES + W.payload_bytes(n, vector_dim, 2, [int(q) for q in moduli])


def total_bytes(n, vector_dim, moduli, first_vector, n_rows):
    return HEADER_BYTES + len(touched_blocks(first_vector, n_rows, n // 2)) * message_bytes(n, vector_dim, moduli)


def container(vector_dim, babies, first_vector, n_rows, first_block, messages, **over):
    """the delta of the given block messages (each the bytes of a type 1 wire message), in block order"""
    return header(vector_dim, babies, first_vector, n_rows, first_block, over.pop("n_blocks", len(messages)), **over) + b"".join(messages)


def build(blocks, moduli, scale, babies, first_vector, n_rows, first_block=0):
    """blocks: per touched block an array [vector_dim][2][n_q][N] of residues -> the delta"""
    blocks = [np.asarray(b, dtype=np.uint64) for b in blocks]
    dim = blocks[0].shape[0]
    return container(dim, babies, first_vector, n_rows, first_block, [W.ct_message(b, moduli, scale) for b in blocks])


def split(data):
    """-> (header dict, [the bytes of each message]); asserts the exact length"""
    data = bytes(data)
    h = parse_header(data)
    assert h["magic"] == MAGIC
    off, out = HEADER_BYTES, []
    for _ in range(h["n_blocks"]):
        m = W.parse_header(data[off:off + W.HEADER_BYTES])
        end = off + W.HEADER_BYTES + m["payload_bytes"]
        assert end <= len(data)
        out.append(data[off:end])
        off = end
    assert off == len(data)
    return h, out
