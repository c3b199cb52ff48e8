// tests/wire_header_check.cpp — the wire format's validator (image_matching_amd/csrc/wire_format.h, included alone) under
// AddressSanitizer and UndefinedBehaviorSanitizer: every prefix of a valid header, every single-byte mutation of it, and shapes whose
// payload size wraps 64 bits.  Every buffer handed to the validator is a heap block of exactly the bytes it may read, so a read past
// the header or past a short buffer is a sanitizer report.  Exits 0 when every expectation held (tests/test_wire_cpu.py runs it).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "wire_format.h"

namespace W = hydia::wire;

static int failures = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);    \
            failures++;                                                \
        }                                                              \
    } while (0)

// check() on a heap copy of exactly `have` bytes of src, claiming `len`
static bool run(const unsigned char *src, size_t have, size_t len, bool whole, const W::Expect *e, W::Header *out, std::string *err) {
    unsigned char *heap = have ? (unsigned char *)std::malloc(have) : nullptr;
    if (have) std::memcpy(heap, src, have);
    const bool ok = W::check(heap, len, whole, e, out, err);
    std::free(heap);
    return ok;
}

int main() {
    // a chain with the default parameters' widths: 60, then 46 / 45 alternating, then four 60-bit special primes (values need not be prime here)
    uint64_t moduli[16];
    for (int j = 0; j < 16; j++) moduli[j] = j == 0 || j >= 12 ? (1ull << 59) + 1001 + j : (j % 2 ? (1ull << 45) + 77 + j : (1ull << 44) + 55 + j);
    const W::Expect ctx{11, 12, 4, 3, moduli, 35184372088832.0};
    uint8_t seed[32];
    for (int i = 0; i < 32; i++) seed[i] = (uint8_t)(i + 1);
    std::vector<W::Header> valid = {
        W::make_header(W::CT_BATCH, 11, 3, 2, 12, 0, 1.5e13, nullptr, 0, moduli),
        W::make_header(W::CT_BATCH, 11, 1, 3, 5, 0, 3.0, nullptr, 0, moduli),
        W::make_header(W::SEEDED_QUERY, 11, 3, 1, 12, 0, ctx.delta, seed, (1ull << 40) - 3, moduli),
        W::make_header(W::EVAL_KEY, 11, 3, 2, 16, 1023, 0.0, nullptr, 0, moduli),
        W::make_header(W::EVAL_KEY_SEEDED, 11, 3, 1, 16, 0, 0.0, seed, 0, moduli),
        W::make_header(W::PUBLIC_KEY, 11, 1, 2, 12, 0, 0.0, nullptr, 0, moduli),
        W::make_header(W::PUBLIC_KEY_SEEDED, 11, 1, 1, 12, 0, 0.0, seed, 0, moduli),
    };
    for (const W::Header &h : valid) {
        const unsigned char *raw = reinterpret_cast<const unsigned char *>(&h);
        const size_t len = sizeof h + h.payload_bytes;
        W::Header out;
        std::string err;
        // the header itself: accepted with and without a context, whole and streamed; one byte short or over is refused
        EXPECT(run(raw, sizeof h, len, true, nullptr, &out, &err));
        EXPECT(run(raw, sizeof h, len, true, &ctx, &out, &err) && out.payload_bytes == h.payload_bytes && out.count == h.count);
        EXPECT(run(raw, sizeof h, sizeof h, false, &ctx, &out, &err));
        EXPECT(!run(raw, sizeof h, len - 1, true, &ctx, &out, &err) && err.find("len") != std::string::npos);
        EXPECT(!run(raw, sizeof h, len + 1, true, &ctx, &out, &err) && err.find("len") != std::string::npos);
        // every prefix: refused, and no byte past the prefix is read
        for (size_t n = 0; n < sizeof h; n++) EXPECT(!run(raw, n, n, true, &ctx, &out, &err));
        EXPECT(!W::check(nullptr, len, true, &ctx, &out, &err));
        // every single-byte mutation, three patterns per byte: never a fault; what is accepted is consistent with the claimed length
        for (size_t i = 0; i < sizeof h; i++)
            for (unsigned char flip : {(unsigned char)0x01, (unsigned char)0x80, (unsigned char)0xFF}) {
                unsigned char m[sizeof h];
                std::memcpy(m, raw, sizeof h);
                m[i] ^= flip;
                for (const W::Expect *e : {(const W::Expect *)nullptr, &ctx}) {
                    if (run(m, sizeof h, len, true, e, &out, &err)) {
                        uint64_t need = 0;
                        EXPECT(W::payload_bytes(out.log_n, out.count, out.n_polys, out.n_limbs, out.moduli, &need) && need == len - sizeof h);
                        // with a context every byte of the header but the seed, the nonce, the scale of a batch and a key's id is pinned
                        const bool free_byte = (i >= 48 && i < 80 && W::is_seeded(h.type)) || (i >= 80 && i < 88 && h.type == W::SEEDED_QUERY) ||
                                               (i >= 40 && i < 48 && h.type == W::CT_BATCH) || (i >= 28 && i < 32 && W::is_key(h.type));
                        if (e) EXPECT(free_byte);
                    }
                    (void)run(m, sizeof h, sizeof h, false, e, &out, &err);
                }
            }
    }
    // shapes whose size wraps 64 bits: refused by the overflow check whatever payload_bytes claims
    {
        W::Header h = valid[0];
        const uint64_t per = W::rows_bytes(h.log_n, h.n_limbs, h.moduli) * h.n_polys;
        for (uint64_t count : {UINT64_MAX / per + 1, UINT64_MAX / per + 2, UINT64_MAX, UINT64_MAX / 2 + 1, (UINT64_MAX - sizeof h) / per + 1}) {
            h.count = count;
            for (uint64_t claim : {(uint64_t)0, per * count /* the wrapped product */, h.payload_bytes}) {
                h.payload_bytes = claim;
                W::Header out;
                std::string err;
                const unsigned char *raw = reinterpret_cast<const unsigned char *>(&h);
                EXPECT(!run(raw, sizeof h, sizeof h + (size_t)claim, true, nullptr, &out, &err));
                EXPECT(!run(raw, sizeof h, sizeof h, false, nullptr, &out, &err));
            }
            uint64_t b;
            EXPECT(!W::payload_bytes(h.log_n, count, h.n_polys, h.n_limbs, h.moduli, &b));
        }
        // the largest count that still fits is arithmetic, not a fault
        uint64_t b;
        EXPECT(W::payload_bytes(h.log_n, (UINT64_MAX - sizeof h) / per, h.n_polys, h.n_limbs, h.moduli, &b));
    }
    // the key-set file header
    {
        W::FileHeader f{};
        std::memcpy(f.magic, W::FILE_MAGIC, 8);
        f.version = W::VERSION;
        f.n_messages = 4;
        W::FileHeader out;
        std::string err;
        const unsigned char *raw = reinterpret_cast<const unsigned char *>(&f);
        for (size_t n = 0; n < sizeof f; n++) {
            unsigned char *heap = n ? (unsigned char *)std::malloc(n) : nullptr;
            if (n) std::memcpy(heap, raw, n);
            EXPECT(!W::check_file_header(heap, n, &out, &err));
            std::free(heap);
        }
        EXPECT(W::check_file_header(raw, sizeof f, &out, &err) && out.n_messages == 4);
    }
    if (failures) return 1;
    std::puts("wire_header_check ok");
    return 0;
}
