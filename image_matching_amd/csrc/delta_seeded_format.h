// image_matching_amd/csrc/delta_seeded_format.h — the container of a SEEDED database delta (include/hydia.h, "seeded database deltas"):
// size arithmetic and validation.  Host only: no HIP, no library type — tests/delta_seeded_header_check.cpp includes this file,
// delta_format.h and wire_format.h alone.
//
// A seeded delta is delta_format.h's 64-byte Header under the magic HYDDELS1, then n_blocks ordinary SEEDED_QUERY (type 2) wire
// messages back to back, nothing after the last.  Message b holds the c0 halves of the vector_dim ciphertexts E that are added to (or
// become) block first_vector / slots + b of the target database: count = vector_dim, one polynomial on all n_q limbs at the scale of a
// fresh encryption.  Ciphertext i of the message is (c0_i, a(a_seed, nonce0 + i)), expanded as a seeded query is; every message of a
// delta carries the same a_seed, and nonce0 = (first_block + first_vector / slots + b) * vector_dim — the enrolment's offset of that
// block's ciphertext 0 — so no two ciphertexts of a delta share a stream.
// Every check below reads the container header and the 360-byte headers of the messages alone, before anything is allocated; all
// size arithmetic is overflow-checked.
#pragma once
#include "delta_format.h"

namespace hydia {
namespace delta_seeded {

using delta::Expect;
using delta::Header;
constexpr uint32_t VERSION = 1;
constexpr char MAGIC[9] = "HYDDELS1";

// nonce0 of the message of block `block` (an absolute block index); false when it or the last nonce of the block is not below 2^40
inline bool block_nonce(uint64_t first_block, uint64_t block, uint32_t vector_dim, uint64_t *out) {
    uint64_t g, n, last;
    if (__builtin_add_overflow(first_block, block, &g) || __builtin_mul_overflow(g, (uint64_t)vector_dim, &n)) return false;
    if (__builtin_add_overflow(n, (uint64_t)vector_dim, &last) || last >= wire::NONCE_LIMIT) return false;
    *out = n;
    return true;
}
// bytes of the whole seeded delta for rows first_vector .. first_vector + n_rows - 1: the header + one message of vector_dim c0 halves
// per touched block; false when there are no rows or the size does not fit 64 bits
inline bool total_bytes(uint32_t log_n, uint32_t n_q, const uint64_t *moduli, uint32_t vector_dim, uint64_t first_vector, uint64_t n_rows,
                        uint64_t *out) {
    uint64_t blocks, msg, b;
    if (log_n < 1 || log_n > 16 || !delta::touched_blocks(first_vector, n_rows, (uint64_t)1 << (log_n - 1), &blocks)) return false;
    if (!wire::payload_bytes(log_n, vector_dim, 1, n_q, moduli, &msg)) return false;
    msg += sizeof(wire::Header);  // (payload_bytes left room for it)
    if (__builtin_mul_overflow(msg, blocks, &b) || b > UINT64_MAX - sizeof(Header)) return false;
    *out = b + sizeof(Header);
    return true;
}
inline Header make_header(uint32_t vector_dim, uint64_t babies, uint64_t first_vector, uint64_t n_rows, uint64_t first_block, uint64_t n_blocks) {
    Header h = delta::make_header(vector_dim, babies, first_vector, n_rows, first_block, n_blocks);
    std::memcpy(h.magic, MAGIC, 8);
    h.version = VERSION;
    return h;
}

// Validate the seeded delta at (buf, len).  true: *out holds the header, *log_n (when given) the ring of its messages, a_seed (when
// given) the 32 bytes every message carries.  false: *err names the field.  Only the container header and the header of every
// message are read.
inline bool check(const void *buf, size_t len, const Expect *e, Header *out, uint32_t *log_n, uint8_t *a_seed, std::string *err) {
    auto no = [&](const std::string &m) {
        if (err) *err = "hydia: seeded database delta refused: " + m;
        return false;
    };
    if (!buf) return no("null buffer");
    if (len < sizeof(Header)) return no("len is shorter than a delta header");
    Header h;
    std::memcpy(&h, buf, sizeof h);
    if (std::memcmp(h.magic, delta::MAGIC, 8) == 0) return no("magic: this is an unseeded delta (HYDDELT1), which hydia_db_delta_apply / hydia_db_delta_peek take");
    if (std::memcmp(h.magic, MAGIC, 8) != 0) return no("magic");
    if (h.version != VERSION) return no("version");
    if (h.reserved != 0) return no("reserved field is not zero");
    if (h.vector_dim < 2 || (h.vector_dim & (h.vector_dim - 1)) != 0) return no("vector_dim is not a power of two >= 2");
    if (e && h.vector_dim != e->vector_dim) return no("vector_dim is not the context's");
    if (!delta::is_form(h.babies, h.vector_dim)) return no("babies is neither vector_dim nor a power of two >= 2 dividing it");
    if (h.n_rows == 0) return no("n_rows is zero");
    uint64_t end;
    if (__builtin_add_overflow(h.first_vector, h.n_rows, &end)) return no("first_vector + n_rows overflows 64 bits");
    if (h.n_blocks == 0) return no("n_blocks is zero");
    const unsigned char *p = (const unsigned char *)buf + sizeof h;
    uint64_t left = (uint64_t)len - sizeof h, ring = 0, block0 = 0;
    uint8_t seed0[32] = {0};
    for (uint64_t b = 0; b < h.n_blocks; b++) {  // (every turn consumes at least a message header of `left`: at most len / 360 turns)
        const std::string where = "message " + std::to_string(b) + ": ";
        if (left < sizeof(wire::Header)) return no(where + "len: the delta is truncated");
        wire::Header m;
        std::string werr;
        if (!wire::check(p, sizeof(wire::Header), false, e ? &e->w : nullptr, &m, &werr)) return no(where + werr);
        if (m.type != wire::SEEDED_QUERY) return no(where + "type is not a seeded query (type 2)");
        if (m.count != h.vector_dim) return no(where + "count is not vector_dim");
        if (m.n_polys != 1) return no(where + "n_polys is not 1");
        if (e && m.n_limbs != e->w.n_q) return no(where + "n_limbs is not n_q of the context");
        if (e && m.scale != e->w.delta) return no(where + "scale is not the context's 2^scale_bits");
        if (b == 0) {
            ring = m.log_n;
            const uint64_t slots = ((uint64_t)1 << ring) / 2;
            if (h.vector_dim > slots) return no("vector_dim exceeds the slots of the messages' ring");
            uint64_t touched = 0;
            (void)delta::touched_blocks(h.first_vector, h.n_rows, slots, &touched);
            if (h.n_blocks != touched) return no("n_blocks is not the number of blocks first_vector .. first_vector + n_rows - 1 touch");
            block0 = h.first_vector / slots;
            std::memcpy(seed0, m.a_seed, 32);
        } else {
            if (m.log_n != ring) return no(where + "log_n differs from the first message's");
            if (std::memcmp(m.a_seed, seed0, 32) != 0) return no(where + "a_seed differs from the first message's");
        }
        uint64_t block, nonce;
        if (__builtin_add_overflow(block0, b, &block) || !block_nonce(h.first_block, block, h.vector_dim, &nonce))
            return no(where + "nonce0 + count: (first_block + block) * vector_dim + vector_dim is not below 2^40");
        if (m.nonce0 != nonce) return no(where + "nonce0 is not (first_block + block) * vector_dim");
        if (m.payload_bytes > left - sizeof(wire::Header)) return no(where + "len: the delta is truncated");
        p += sizeof(wire::Header) + m.payload_bytes;
        left -= sizeof(wire::Header) + m.payload_bytes;
    }
    if (left != 0) return no("len: bytes after the last message");
    if (out) *out = h;
    if (log_n) *log_n = (uint32_t)ring;
    if (a_seed) std::memcpy(a_seed, seed0, 32);
    return true;
}

}  // namespace delta_seeded
}  // namespace hydia
