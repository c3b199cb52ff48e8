// image_matching_amd/csrc/delta_format.h — the containers of a database delta and of a SEEDED database delta (include/hydia.h, "database
// deltas", "seeded database deltas"): header layout, size arithmetic and ONE validator over the Form that names what the two differ in.
// Host only: no HIP, no library type — tests/delta_header_check.cpp includes this file and wire_format.h alone.
//
// A delta is a Header, then n_blocks ordinary wire messages (wire_format.h) back to back, nothing after the last.  It is NOT a wire
// type: a container of its own, like the key-set file.  Message b holds the vector_dim ciphertexts E that are added to (or become)
// block first_vector / slots + b of the target database: count = vector_dim, all n_q limbs at the scale of a fresh encryption;
// ciphertext i of the message belongs to database ciphertext block * vector_dim + i.
//   WHOLE  (HYDDELT1): CT_BATCH messages, two polynomials.
//   SEEDED (HYDDELS1): SEEDED_QUERY (type 2) messages, the c0 halves alone.  Ciphertext i of a message is (c0_i, a(a_seed, nonce0 + i)),
//          expanded as a seeded query is; every message of a delta carries the same a_seed, and nonce0 = (first_block + first_vector /
//          slots + b) * vector_dim — the enrolment's offset of that block's ciphertext 0 — so no two ciphertexts of a delta share a stream.
// Every check below reads the container header and the 360-byte headers of the messages alone, before anything is allocated; all
// size arithmetic is overflow-checked.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "wire_format.h"

namespace hydia {
namespace delta {

constexpr uint32_t VERSION = 1;

struct Header {  // little-endian, no padding
    char magic[8];
    uint32_t version;
    uint32_t vector_dim;
    uint64_t babies;        // the form of the target database: vector_dim (hoisted) or a power of two >= 2 dividing it
    uint64_t first_vector;  // the rows are vectors first_vector .. first_vector + n_rows - 1
    uint64_t n_rows;
    uint64_t first_block;   // recorded for diagnosis: the nonce offset the maker used
    uint64_t n_blocks;      // the blocks those vectors touch = the messages that follow
    uint64_t reserved;      // 0
};
static_assert(sizeof(Header) == 64 && sizeof(Header) % 8 == 0, "the delta header is 64 bytes without padding");

// what a context expects of a delta (nullptr: the context-free checks alone, hydia_db_delta_peek)
struct Expect {
    wire::Expect w;
    uint32_t vector_dim;
};

// everything the two containers differ in; the rest of this file is stated once, over a Form
struct Form {
    char magic[9];
    uint32_t type, n_polys;    // of every message
    const char *refused;       // how every refusal of check begins
    const char *type_refusal;  // the wording of the type refusal
    bool a_seed, nonce0;       // the messages carry ONE a_seed / a nonce0 in step with first_block and the block
};
inline constexpr Form WHOLE{"HYDDELT1", wire::CT_BATCH, 2, "database delta refused: ", "type is not a ciphertext batch", false, false};
inline constexpr Form SEEDED{"HYDDELS1", wire::SEEDED_QUERY, 1, "seeded database delta refused: ", "type is not a seeded query (type 2)", true, true};

inline bool is_form(uint64_t babies, uint32_t dim) {
    return babies == dim || (babies >= 2 && babies < dim && (babies & (babies - 1)) == 0 && dim % babies == 0);
}
// the blocks of `slots` vectors that vectors first_vector .. first_vector + n_rows - 1 touch; false: no rows, or the range overflows
inline bool touched_blocks(uint64_t first_vector, uint64_t n_rows, uint64_t slots, uint64_t *out) {
    uint64_t end;
    if (n_rows == 0 || slots == 0 || __builtin_add_overflow(first_vector, n_rows, &end)) return false;
    *out = (end - 1) / slots - first_vector / slots + 1;
    return true;
}
// nonce0 of a seeded delta's message of block `block` (an absolute block index); false when it or the last nonce of the block is not
// below 2^40
inline bool block_nonce(uint64_t first_block, uint64_t block, uint32_t vector_dim, uint64_t *out) {
    uint64_t g, n, last;
    if (__builtin_add_overflow(first_block, block, &g) || __builtin_mul_overflow(g, (uint64_t)vector_dim, &n)) return false;
    if (__builtin_add_overflow(n, (uint64_t)vector_dim, &last) || last >= wire::NONCE_LIMIT) return false;
    *out = n;
    return true;
}
// bytes of the whole delta for rows first_vector .. first_vector + n_rows - 1: the header + one message of vector_dim ciphertexts (or
// c0 halves) per touched block; false when there are no rows or the size does not fit 64 bits
inline bool total_bytes(const Form &f, uint32_t log_n, uint32_t n_q, const uint64_t *moduli, uint32_t vector_dim, uint64_t first_vector, uint64_t n_rows,
                        uint64_t *out) {
    uint64_t blocks, msg, b;
    if (log_n < 1 || log_n > 16 || !touched_blocks(first_vector, n_rows, (uint64_t)1 << (log_n - 1), &blocks)) return false;
    if (!wire::payload_bytes(log_n, vector_dim, f.n_polys, n_q, moduli, &msg)) return false;
    msg += sizeof(wire::Header);  // (payload_bytes left room for it)
    if (__builtin_mul_overflow(msg, blocks, &b) || b > UINT64_MAX - sizeof(Header)) return false;
    *out = b + sizeof(Header);
    return true;
}
inline Header make_header(const Form &f, uint32_t vector_dim, uint64_t babies, uint64_t first_vector, uint64_t n_rows, uint64_t first_block, uint64_t n_blocks) {
    Header h;
    std::memset(&h, 0, sizeof h);
    std::memcpy(h.magic, f.magic, 8);
    h.version = VERSION; h.vector_dim = vector_dim; h.babies = babies; h.first_vector = first_vector; h.n_rows = n_rows;
    h.first_block = first_block; h.n_blocks = n_blocks;
    return h;
}

// Validate the delta of form f at (buf, len).  true: *out holds the header, *log_n (when given) the ring of its messages, a_seed (when
// given, f.a_seed) the 32 bytes every message carries.  false: *err names the field.  Only the container header and the header of
// every message are read.
inline bool check(const Form &f, const void *buf, size_t len, const Expect *e, Header *out, uint32_t *log_n, uint8_t *a_seed, std::string *err) {
    auto no = [&](const std::string &m) {
        if (err) *err = std::string("hydia: ") + f.refused + m;
        return false;
    };
    if (!buf) return no("null buffer");
    if (len < sizeof(Header)) return no("len is shorter than a delta header");
    Header h;
    std::memcpy(&h, buf, sizeof h);
    if (std::memcmp(f.magic, WHOLE.magic, 8) != 0 && std::memcmp(h.magic, WHOLE.magic, 8) == 0)
        return no("magic: this is an unseeded delta (HYDDELT1), which hydia_db_delta_apply / hydia_db_delta_peek take");
    if (std::memcmp(h.magic, f.magic, 8) != 0) return no("magic");
    if (h.version != VERSION) return no("version");
    if (h.reserved != 0) return no("reserved field is not zero");
    if (h.vector_dim < 2 || (h.vector_dim & (h.vector_dim - 1)) != 0) return no("vector_dim is not a power of two >= 2");
    if (e && h.vector_dim != e->vector_dim) return no("vector_dim is not the context's");
    if (!is_form(h.babies, h.vector_dim)) return no("babies is neither vector_dim nor a power of two >= 2 dividing it");
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
        if (m.type != f.type) return no(where + f.type_refusal);
        if (m.count != h.vector_dim) return no(where + "count is not vector_dim");
        if (m.n_polys != f.n_polys) return no(where + "n_polys is not " + std::to_string(f.n_polys));
        if (e && m.n_limbs != e->w.n_q) return no(where + "n_limbs is not n_q of the context");
        if (e && m.scale != e->w.delta) return no(where + "scale is not the context's 2^scale_bits");
        if (b == 0) {
            ring = m.log_n;
            const uint64_t slots = ((uint64_t)1 << ring) / 2;
            if (h.vector_dim > slots) return no("vector_dim exceeds the slots of the messages' ring");
            uint64_t touched = 0;
            (void)touched_blocks(h.first_vector, h.n_rows, slots, &touched);
            if (h.n_blocks != touched) return no("n_blocks is not the number of blocks first_vector .. first_vector + n_rows - 1 touch");
            block0 = h.first_vector / slots;
            std::memcpy(seed0, m.a_seed, 32);
        } else {
            if (m.log_n != ring) return no(where + "log_n differs from the first message's");
            if (f.a_seed && std::memcmp(m.a_seed, seed0, 32) != 0) return no(where + "a_seed differs from the first message's");
        }
        if (f.nonce0) {
            uint64_t block, nonce;
            if (__builtin_add_overflow(block0, b, &block) || !block_nonce(h.first_block, block, h.vector_dim, &nonce))
                return no(where + "nonce0 + count: (first_block + block) * vector_dim + vector_dim is not below 2^40");
            if (m.nonce0 != nonce) return no(where + "nonce0 is not (first_block + block) * vector_dim");
        }
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
// the whole delta's, as callers that know no other form spell them
inline bool total_bytes(uint32_t log_n, uint32_t n_q, const uint64_t *moduli, uint32_t vector_dim, uint64_t first_vector, uint64_t n_rows, uint64_t *out) {
    return total_bytes(WHOLE, log_n, n_q, moduli, vector_dim, first_vector, n_rows, out);
}
inline Header make_header(uint32_t vector_dim, uint64_t babies, uint64_t first_vector, uint64_t n_rows, uint64_t first_block, uint64_t n_blocks) {
    return make_header(WHOLE, vector_dim, babies, first_vector, n_rows, first_block, n_blocks);
}
inline bool check(const void *buf, size_t len, const Expect *e, Header *out, uint32_t *log_n, std::string *err) {
    return check(WHOLE, buf, len, e, out, log_n, nullptr, err);
}

}  // namespace delta
}  // namespace hydia
