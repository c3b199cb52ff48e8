// image_matching_amd/csrc/wire_format.h — the wire format of include/hydia.h ("wire messages"): header layout, size arithmetic and
// validation.  Host only: no HIP, no library type — tests/wire_header_check.cpp includes this file alone.
//
// A message is a Header followed by its payload, little-endian, nothing after the payload.  The payload holds rows in the order
// [count][poly][limb]; a row is the N residues of one limb, residue c in bits [c w_j, (c + 1) w_j) of the row read as one little-endian
// bit string, w_j = the bit length of the limb's modulus.  N is a multiple of 64, so a row is N w_j / 64 whole 64-bit words.
// Every check below is made on the bytes of the header alone, before anything is allocated; all size arithmetic is overflow-checked.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

namespace hydia {
namespace wire {

constexpr uint32_t MAX_LIMBS = 32;  // HY_MAX_MODS: Q limbs + P limbs
constexpr uint32_t VERSION = 1;
constexpr uint64_t NONCE_LIMIT = 1ull << 40;
constexpr char MAGIC[9] = "HYDWIRE1";
constexpr char FILE_MAGIC[9] = "HYDKEYS1";

enum Type : uint32_t {
    CT_BATCH = 1,          // count ciphertexts of n_polys polynomials on n_limbs limbs
    SEEDED_QUERY = 2,      // count c0 halves (one polynomial each); c1 = the expansion of (a_seed, nonce0 + i)
    EVAL_KEY = 3,          // count = dnum digits of (b, a) on n_q + n_p limbs
    EVAL_KEY_SEEDED = 4,   // the b halves alone
    PUBLIC_KEY = 5,        // (b, a) on n_q limbs, count 1
    PUBLIC_KEY_SEEDED = 6  // b alone
};

struct Header {
    char magic[8];
    uint32_t version, type, log_n, n_polys, n_limbs;
    uint32_t rot;       // types 3 / 4: the key id (0 = relinearisation); otherwise 0
    uint64_t count;
    double scale;       // types 1 / 2; otherwise +0.0
    uint8_t a_seed[32]; // types 2 / 4 / 6; otherwise zero
    uint64_t nonce0;    // type 2; otherwise 0
    uint64_t payload_bytes;
    uint64_t reserved;  // 0
    uint64_t moduli[MAX_LIMBS];  // the moduli of limbs 0 .. n_limbs - 1, then zeros
};
static_assert(sizeof(Header) == 360 && sizeof(Header) % 8 == 0, "the header is 360 bytes without padding");

struct FileHeader {  // a key-set file: this, then n_messages messages back to back (the public key, then evaluation keys by ascending id)
    char magic[8];
    uint32_t version, n_messages;
};
static_assert(sizeof(FileHeader) == 16, "the key-set file header is 16 bytes");

// what a context expects of a message (nullptr: the context-free checks alone, hydia_wire_peek)
struct Expect {
    uint32_t log_n, n_q, n_p, dnum;
    const uint64_t *moduli;  // n_q + n_p
    double delta;            // 2^scale_bits: the scale of a fresh query
};

inline int bit_length(uint64_t q) { return q ? 64 - __builtin_clzll(q) : 0; }
inline bool is_key(uint32_t type) { return type == EVAL_KEY || type == EVAL_KEY_SEEDED; }
inline bool is_seeded(uint32_t type) { return type == SEEDED_QUERY || type == EVAL_KEY_SEEDED || type == PUBLIC_KEY_SEEDED; }

// bytes of one [limb] run of rows: sum_j N w_j / 8.  At most 32 limbs of 2^16 residues of 8 bytes: no overflow
inline uint64_t rows_bytes(uint32_t log_n, uint32_t n_limbs, const uint64_t *moduli) {
    uint64_t s = 0;
    for (uint32_t j = 0; j < n_limbs; j++) s += ((uint64_t)1 << log_n) / 8 * (uint64_t)bit_length(moduli[j]);
    return s;
}
// count x n_polys x sum_j N w_j / 8, false when it does not fit 64 bits (with room for the header)
inline bool payload_bytes(uint32_t log_n, uint64_t count, uint32_t n_polys, uint32_t n_limbs, const uint64_t *moduli, uint64_t *out) {
    uint64_t b = rows_bytes(log_n, n_limbs, moduli);
    if (__builtin_mul_overflow(b, (uint64_t)n_polys, &b)) return false;
    if (__builtin_mul_overflow(b, count, &b)) return false;
    if (b > UINT64_MAX - sizeof(Header)) return false;
    *out = b;
    return true;
}
// a header for the given shape (the caller has validated it); payload_bytes filled in
inline Header make_header(uint32_t type, uint32_t log_n, uint64_t count, uint32_t n_polys, uint32_t n_limbs, uint32_t rot, double scale,
                          const uint8_t *a_seed, uint64_t nonce0, const uint64_t *moduli) {
    Header h;
    std::memset(&h, 0, sizeof h);
    std::memcpy(h.magic, MAGIC, 8);
    h.version = VERSION; h.type = type; h.log_n = log_n; h.count = count; h.n_polys = n_polys; h.n_limbs = n_limbs; h.rot = rot;
    h.scale = scale;
    if (a_seed) std::memcpy(h.a_seed, a_seed, 32);
    h.nonce0 = nonce0;
    for (uint32_t j = 0; j < n_limbs && j < MAX_LIMBS; j++) h.moduli[j] = moduli[j];
    if (!payload_bytes(log_n, count, n_polys, n_limbs < MAX_LIMBS ? n_limbs : MAX_LIMBS, h.moduli, &h.payload_bytes)) h.payload_bytes = 0;
    return h;
}

// Validate the message at (buf, len).  whole: len must be exactly header + payload (a message in memory); otherwise len >= the header
// is enough (a file being streamed: the payload is read after the header passed).  true: *out holds the header.  false: *err names the
// field.  Nothing but the first sizeof(Header) bytes of buf is read.
inline bool check(const void *buf, size_t len, bool whole, const Expect *e, Header *out, std::string *err) {
    auto no = [&](const char *m) {
        if (err) *err = std::string("hydia: wire message refused: ") + m;
        return false;
    };
    if (!buf) return no("null buffer");
    if (len < sizeof(Header)) return no("len is shorter than a header");
    Header h;
    std::memcpy(&h, buf, sizeof h);
    if (std::memcmp(h.magic, MAGIC, 8) != 0) return no("magic");
    if (h.version != VERSION) return no("version");
    if (h.type < CT_BATCH || h.type > PUBLIC_KEY_SEEDED) return no("type is unknown");
    if (h.reserved != 0) return no("reserved field is not zero");
    if (h.log_n < 10 || h.log_n > 16) return no("log_n outside 10 .. 16");
    if (e && h.log_n != e->log_n) return no("log_n is not the context's");
    if (h.count == 0) return no("count is zero");
    const uint32_t slots = (1u << h.log_n) / 2;
    switch (h.type) {
        case CT_BATCH:
            if (h.n_polys != 2 && h.n_polys != 3) return no("n_polys outside {2, 3}");
            break;
        case EVAL_KEY:
        case PUBLIC_KEY:
            if (h.n_polys != 2) return no("n_polys is not 2 for a whole key");
            break;
        default:
            if (h.n_polys != 1) return no("n_polys is not 1 for a seeded type");
    }
    if ((h.type == PUBLIC_KEY || h.type == PUBLIC_KEY_SEEDED) && h.count != 1) return no("count is not 1 for a public key");
    if (h.n_limbs < 1 || h.n_limbs > MAX_LIMBS) return no("n_limbs outside 1 .. 32");
    if (e) {
        if (is_key(h.type)) {
            if (h.n_limbs != e->n_q + e->n_p) return no("n_limbs is not n_q + n_p of the context");
            if (h.count != e->dnum) return no("count is not the context's dnum");
        } else if (h.type == CT_BATCH) {
            if (h.n_limbs > e->n_q) return no("n_limbs outside 1 .. n_q of the context");
        } else if (h.n_limbs != e->n_q) {
            return no("n_limbs is not n_q of the context");
        }
    }
    if (is_key(h.type) ? h.rot >= slots : h.rot != 0) return no("rot outside [0, slots)");
    if (h.type == CT_BATCH || h.type == SEEDED_QUERY) {
        if (!std::isfinite(h.scale) || !(h.scale > 0)) return no("scale is not finite and positive");
        if (e && h.type == SEEDED_QUERY && h.scale != e->delta) return no("scale is not the context's 2^scale_bits");
    } else {
        uint64_t bits;
        std::memcpy(&bits, &h.scale, 8);
        if (bits != 0) return no("scale is not zero for a key");
    }
    if (h.type == SEEDED_QUERY) {
        if (h.nonce0 > NONCE_LIMIT || h.count > NONCE_LIMIT - h.nonce0) return no("nonce0 + count exceeds 2^40");
    } else if (h.nonce0 != 0) {
        return no("nonce0 is not zero");
    }
    if (!is_seeded(h.type))
        for (int i = 0; i < 32; i++)
            if (h.a_seed[i]) return no("a_seed is not zero for an unseeded type");
    for (uint32_t j = 0; j < MAX_LIMBS; j++) {
        if (j < h.n_limbs) {
            if (h.moduli[j] < 2) return no("modulus below 2");
            if (e && h.moduli[j] != e->moduli[j]) return no("modulus is not the context's modulus of that limb");
        } else if (h.moduli[j] != 0) {
            return no("modulus listed past n_limbs");
        }
    }
    uint64_t need;
    if (!payload_bytes(h.log_n, h.count, h.n_polys, h.n_limbs, h.moduli, &need)) return no("count: the payload size overflows 64 bits");
    if (h.payload_bytes != need) return no("payload_bytes is not what the shape implies");
    if (whole && (uint64_t)len - sizeof(Header) != need) return no(((uint64_t)len - sizeof(Header) < need) ? "len: the message is truncated" : "len: bytes after the payload");
    if (out) *out = h;
    return true;
}
inline bool check_file_header(const void *buf, size_t len, FileHeader *out, std::string *err) {
    FileHeader f;
    if (!buf || len < sizeof f) {
        if (err) *err = "hydia: key-set file refused: shorter than its header";
        return false;
    }
    std::memcpy(&f, buf, sizeof f);
    if (std::memcmp(f.magic, FILE_MAGIC, 8) != 0 || f.version != VERSION || f.n_messages == 0) {
        if (err) *err = "hydia: key-set file refused: magic, version or message count";
        return false;
    }
    *out = f;
    return true;
}

}  // namespace wire
}  // namespace hydia
