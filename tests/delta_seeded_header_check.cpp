// tests/delta_seeded_header_check.cpp — the validator of a SEEDED database delta's container
// (image_matching_amd/csrc/delta_seeded_format.h with delta_format.h and wire_format.h, included alone) under AddressSanitizer and
// UndefinedBehaviorSanitizer: every refusal of the container check — a wrong type, two polynomials, two a_seeds, a nonce0 out of step,
// truncation, trailing bytes, overflowing counts, the unseeded magic — every prefix of a valid delta's headers, every single-byte
// mutation of the container header and of a message header, and the size arithmetic, at the default parameters too.  Every buffer handed
// to the validator is a heap block of exactly the bytes it may read, so a read past a short buffer is a sanitizer report.  Exits 0 when
// every expectation held (tests/test_db_delta_seeded_cpu.py runs it).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "delta_format.h"
#include "delta_seeded_format.h"
#include "wire_format.h"

namespace W = hydia::wire;
namespace D = hydia::delta;
namespace S = hydia::delta_seeded;

static int failures = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);    \
            failures++;                                                \
        }                                                              \
    } while (0)

// check() on a heap copy of exactly `have` bytes of src, claiming `len`
static bool run(const std::vector<unsigned char> &src, size_t have, size_t len, const D::Expect *e, D::Header *out, std::string *err,
                uint8_t *a_seed = nullptr) {
    unsigned char *heap = have ? (unsigned char *)std::malloc(have) : nullptr;
    if (have) std::memcpy(heap, src.data(), have);
    uint32_t log_n = 0;
    const bool ok = S::check(heap, len, e, out, &log_n, a_seed, err);
    if (ok) EXPECT(log_n == 10);
    std::free(heap);
    return ok;
}
static bool names(const std::string &err, const char *field) {
    return err.find("seeded database delta refused") != std::string::npos && err.find(field) != std::string::npos;
}

// a small ring keeps whole deltas in a few hundred kilobytes: N = 1024 (512 slots), vector_dim 4, three limbs of 60 / 46 / 45 bits
static uint64_t moduli[4] = {(1ull << 59) + 1001, (1ull << 45) + 77, (1ull << 44) + 55, (1ull << 59) + 9};
static const double DELTA = 35184372088832.0;
static const uint32_t DIM = 4;
static const uint64_t SLOTS = 512;
static uint8_t SEED[32];

static std::vector<unsigned char> make(uint64_t babies, uint64_t first_vector, uint64_t n_rows, uint64_t n_blocks, uint64_t first_block = 0) {
    const D::Header h = S::make_header(DIM, babies, first_vector, n_rows, first_block, n_blocks);
    W::Header m = W::make_header(W::SEEDED_QUERY, 10, DIM, 1, 3, 0, DELTA, SEED, 0, moduli);
    std::vector<unsigned char> v(sizeof h + n_blocks * (sizeof m + m.payload_bytes), 0);
    std::memcpy(v.data(), &h, sizeof h);
    for (uint64_t b = 0; b < n_blocks; b++) {
        m.nonce0 = (first_block + first_vector / SLOTS + b) * DIM;
        std::memcpy(v.data() + sizeof h + b * (sizeof m + m.payload_bytes), &m, sizeof m);
    }
    return v;
}
static W::Header *message(std::vector<unsigned char> &v, uint64_t b) {
    W::Header m;
    std::memcpy(&m, v.data() + sizeof(D::Header), sizeof m);
    return reinterpret_cast<W::Header *>(v.data() + sizeof(D::Header) + b * (sizeof m + m.payload_bytes));  // (8-byte aligned: every size is a multiple of 8)
}

int main() {
    for (int i = 0; i < 32; i++) SEED[i] = (uint8_t)(0xC0 + i);
    const D::Expect ctx{W::Expect{10, 3, 1, 3, moduli, DELTA}, DIM};
    D::Header out;
    std::string err;
    // ---- valid deltas: one block, two blocks (rows 500 .. 519 straddle slots = 512), three blocks from block 0 in the pre-rotated form
    // with a nonce offset, one that starts in block 3
    const std::vector<unsigned char> one = make(DIM, 0, 512, 1), two = make(DIM, 500, 20, 2), three = make(2, 511, 514, 3, 7),
                                     late = make(DIM, 3 * 512 + 1, 600, 2, 5);
    for (const auto *v : {&one, &two, &three, &late}) {
        EXPECT(run(*v, v->size(), v->size(), nullptr, &out, &err));
        EXPECT(run(*v, v->size(), v->size(), &ctx, &out, &err));
    }
    uint8_t got_seed[32] = {0};
    EXPECT(run(three, three.size(), three.size(), &ctx, &out, &err, got_seed) && out.n_blocks == 3 && out.babies == 2 && out.first_vector == 511 &&
           out.n_rows == 514 && out.first_block == 7 && out.vector_dim == DIM && std::memcmp(got_seed, SEED, 32) == 0);
    EXPECT(std::memcmp(three.data(), "HYDDELS1", 8) == 0 && out.version == 1);
    EXPECT(message(const_cast<std::vector<unsigned char> &>(late), 1)->nonce0 == (5 + 3 + 1) * DIM);  // (first_block + block) * vector_dim
    // the messages are ordinary type 2 wire messages: wire::check takes each whole
    {
        const size_t msg = (two.size() - sizeof(D::Header)) / 2;
        W::Header m;
        EXPECT(W::check(two.data() + sizeof(D::Header) + msg, msg, true, &ctx.w, &m, &err) && m.type == W::SEEDED_QUERY && m.n_polys == 1 && m.nonce0 == DIM);
    }
    // ---- the size arithmetic agrees with the bytes, and is half the unseeded delta's payload
    uint64_t total = 0, whole = 0;
    EXPECT(S::total_bytes(10, 3, moduli, DIM, 500, 20, &total) && total == two.size());
    EXPECT(S::total_bytes(10, 3, moduli, DIM, 511, 514, &total) && total == three.size());
    EXPECT(D::total_bytes(10, 3, moduli, DIM, 500, 20, &whole) && whole - 64 - 2 * 360 == 2 * (two.size() - 64 - 2 * 360));
    {  // the default parameters: N = 2^15, vector_dim 512, q_0 of 60 bits, six limbs of 46 and five of 45 — from the bit lengths alone
        uint64_t q[12];
        q[0] = (1ull << 59) + 1;
        for (int j = 1; j < 12; j++) q[j] = j <= 6 ? (1ull << 45) + 1 : (1ull << 44) + 1;
        uint64_t t = 0, w = 0;
        EXPECT(S::total_bytes(15, 12, q, 512, 0, 16384, &t) && t == 64 + 1176502632ull);
        EXPECT(1176502632ull == 360 + 512ull * 2297856ull);
        EXPECT(S::total_bytes(15, 12, q, 512, 16384 - 1, 2, &t) && t == 64 + 2 * 1176502632ull);  // a range that touches two blocks
        EXPECT(S::total_bytes(15, 12, q, 512, 3 * 16384, 16384, &t) && t == 64 + 1176502632ull);
        EXPECT(D::total_bytes(15, 12, q, 512, 0, 16384, &w) && w == 64 + 2353004904ull && 100 * (t - 64) < 51 * (w - 64));
    }
    // ---- the length: every prefix of the headers, truncated payloads, trailing bytes, no buffer
    const size_t msg = (two.size() - sizeof(D::Header)) / 2;
    for (size_t n = 0; n < sizeof(D::Header) + sizeof(W::Header); n++) EXPECT(!run(two, n, n, &ctx, &out, &err));
    for (size_t n = sizeof(D::Header) + msg; n < sizeof(D::Header) + msg + sizeof(W::Header); n++) EXPECT(!run(two, n, n, &ctx, &out, &err));
    for (size_t n : {two.size() - 1, two.size() - 8, sizeof(D::Header) + msg, sizeof(D::Header) + msg + sizeof(W::Header)}) {
        EXPECT(!run(two, n, n, &ctx, &out, &err) && names(err, "truncated"));
        EXPECT(!run(two, n, n, nullptr, &out, &err) && names(err, "truncated"));
    }
    {
        std::vector<unsigned char> longer = two;
        longer.push_back(0);
        EXPECT(!run(longer, longer.size(), longer.size(), &ctx, &out, &err) && names(err, "bytes after the last message"));
        longer.resize(two.size() + msg, 0);  // a whole extra message is trailing bytes too
        std::memcpy(longer.data() + two.size(), two.data() + sizeof(D::Header), sizeof(W::Header));
        EXPECT(!run(longer, longer.size(), longer.size(), &ctx, &out, &err) && names(err, "bytes after the last message"));
    }
    EXPECT(!S::check(nullptr, two.size(), &ctx, &out, nullptr, nullptr, &err) && names(err, "null"));
    // ---- the container header's fields
    auto with = [&](const std::vector<unsigned char> &base, auto edit) {
        std::vector<unsigned char> v = base;
        D::Header h;
        std::memcpy(&h, v.data(), sizeof h);
        edit(h);
        std::memcpy(v.data(), &h, sizeof h);
        return v;
    };
    auto refused = [&](const std::vector<unsigned char> &v, const char *field, const D::Expect *e) {
        return !run(v, v.size(), v.size(), e, &out, &err) && names(err, field);
    };
    for (const D::Expect *e : {(const D::Expect *)nullptr, &ctx}) {
        EXPECT(refused(with(two, [](D::Header &h) { h.magic[7] = '2'; }), "magic", e));
        // the unseeded container's magic: refused, and the message names the entry point that takes it
        EXPECT(refused(with(two, [](D::Header &h) { std::memcpy(h.magic, "HYDDELT1", 8); }), "hydia_db_delta_apply", e));
        EXPECT(refused(with(two, [](D::Header &h) { h.version = 2; }), "version", e));
        EXPECT(refused(with(two, [](D::Header &h) { h.reserved = 1; }), "reserved", e));
        EXPECT(refused(with(two, [](D::Header &h) { h.vector_dim = 0; }), "vector_dim", e));
        EXPECT(refused(with(two, [](D::Header &h) { h.vector_dim = 3; }), "vector_dim", e));
        for (uint64_t babies : {(uint64_t)0, (uint64_t)1, (uint64_t)3, (uint64_t)8, UINT64_MAX})
            EXPECT(refused(with(two, [&](D::Header &h) { h.babies = babies; }), "babies", e));
        EXPECT(refused(with(two, [](D::Header &h) { h.n_rows = 0; }), "n_rows", e));
        EXPECT(refused(with(two, [](D::Header &h) { h.n_blocks = 0; }), "n_blocks", e));
        EXPECT(refused(with(two, [](D::Header &h) { h.n_rows = 12; }), "n_blocks", e));
        EXPECT(refused(with(two, [](D::Header &h) { h.n_rows = 525; }), "n_blocks", e));
        EXPECT(refused(with(one, [](D::Header &h) { h.n_rows = 513; }), "n_blocks", e));
        EXPECT(refused(with(two, [](D::Header &h) { h.n_blocks = 1; }), "n_blocks", e));
        EXPECT(refused(with(two, [](D::Header &h) { h.n_blocks = 3; h.n_rows = 600; }), "truncated", e));
        // the overflow cases: first_vector + n_rows wraps; a huge n_blocks ends at the buffer's end, not in a long loop
        EXPECT(refused(with(two, [](D::Header &h) { h.first_vector = UINT64_MAX - 5; h.n_rows = 6; }), "overflows", e));
        EXPECT(refused(with(two, [](D::Header &h) { h.first_vector = UINT64_MAX; h.n_rows = 1; }), "overflows", e));
        EXPECT(refused(with(two, [](D::Header &h) { h.first_vector = 0; h.n_rows = UINT64_MAX; h.n_blocks = UINT64_MAX / 512 + 1; }), "truncated", e));
        EXPECT(refused(with(two, [](D::Header &h) { h.n_blocks = UINT64_MAX; }), "n_blocks", e));
        // ---- nonce0 in step with the container: first_block or first_vector's block changed under the messages, and the 2^40 bound
        EXPECT(refused(with(two, [](D::Header &h) { h.first_block = 1; }), "nonce0 is not", e));
        EXPECT(refused(with(two, [](D::Header &h) { h.first_vector += 512; }), "nonce0 is not", e));  // (still two blocks: 1 and 2)
        EXPECT(refused(with(two, [](D::Header &h) { h.first_block = (1ull << 40) / DIM - 1; }), "below 2^40", e));
        EXPECT(refused(with(two, [](D::Header &h) { h.first_block = UINT64_MAX; }), "below 2^40", e));       // first_block + block wraps
        EXPECT(refused(with(two, [](D::Header &h) { h.first_block = UINT64_MAX / DIM; }), "below 2^40", e));  // the product wraps
    }
    EXPECT(refused(with(two, [](D::Header &h) { h.vector_dim = 8; h.babies = 8; }), "vector_dim is not the context's", &ctx));
    {  // the last block that fits the nonce space, and the first that does not: nonce0 + count must stay BELOW 2^40
        uint64_t n = 0;
        EXPECT(S::block_nonce((1ull << 40) / DIM - 2, 0, DIM, &n) && n == (1ull << 40) - 2 * DIM);
        EXPECT(!S::block_nonce((1ull << 40) / DIM - 1, 0, DIM, &n));
        EXPECT(!S::block_nonce((1ull << 40) / DIM - 2, 1, DIM, &n));
        EXPECT(!S::block_nonce(UINT64_MAX, 1, DIM, &n) && !S::block_nonce(UINT64_MAX / 2, 0, DIM, &n));
        std::vector<unsigned char> edge = make(DIM, 0, 512, 1, (1ull << 40) / DIM - 2);
        EXPECT(run(edge, edge.size(), edge.size(), &ctx, &out, &err));
        uint64_t t = 0;
        EXPECT(!S::total_bytes(10, 3, moduli, DIM, 0, UINT64_MAX, &t));  // blocks x message bytes wraps
        EXPECT(!S::total_bytes(10, 3, moduli, DIM, UINT64_MAX, 1, &t));  // first_vector + n wraps
        EXPECT(!S::total_bytes(10, 3, moduli, DIM, 0, 0, &t));           // no rows
    }
    // ---- the messages: each field of the shape, in the first and in the last message
    for (uint64_t b : {(uint64_t)0, (uint64_t)1}) {
        auto msg_with = [&](auto edit, bool resize = true) {
            std::vector<unsigned char> v = two;
            W::Header *m = message(v, b);
            edit(*m);
            if (resize && !W::payload_bytes(m->log_n, m->count, m->n_polys, m->n_limbs < W::MAX_LIMBS ? m->n_limbs : W::MAX_LIMBS, m->moduli, &m->payload_bytes))
                m->payload_bytes = 0;
            return v;  // (the buffer keeps its length: a message of another size is then refused for its shape, before any length)
        };
        const std::string where = "message " + std::to_string(b);
        EXPECT(refused(msg_with([](W::Header &m) { m.count = DIM + 1; }), "count is not vector_dim", &ctx) && err.find(where) != std::string::npos);
        EXPECT(refused(msg_with([](W::Header &m) { m.count = DIM / 2; }), "count is not vector_dim", nullptr));
        // a wrong type: the unseeded delta's ciphertext batch (zero seed and nonce, as that type demands), a key, an unknown one
        EXPECT(refused(msg_with([](W::Header &m) { m.type = W::CT_BATCH; m.n_polys = 2; m.nonce0 = 0; std::memset(m.a_seed, 0, 32); }),
                       "type is not a seeded query", &ctx));
        EXPECT(refused(msg_with([](W::Header &m) { m.type = W::CT_BATCH; m.n_polys = 2; m.nonce0 = 0; std::memset(m.a_seed, 0, 32); }),
                       "type is not a seeded query", nullptr));
        EXPECT(refused(msg_with([](W::Header &m) { m.type = W::PUBLIC_KEY_SEEDED; m.count = 1; m.scale = 0.0; m.nonce0 = 0; }), "type is not a seeded query", nullptr));
        EXPECT(refused(msg_with([](W::Header &m) { m.type = 7; }), "type is unknown", &ctx));
        // n_polys = 2 (the wire validation of a seeded type names it)
        EXPECT(refused(msg_with([](W::Header &m) { m.n_polys = 2; }), "n_polys is not 1", &ctx));
        EXPECT(refused(msg_with([](W::Header &m) { m.n_polys = 2; }), "n_polys is not 1", nullptr));
        EXPECT(refused(msg_with([](W::Header &m) { m.n_limbs = 2; m.moduli[2] = 0; }), "n_limbs is not n_q", &ctx));
        EXPECT(refused(msg_with([](W::Header &m) { m.n_limbs = 4; m.moduli[3] = moduli[3]; }), "n_limbs", &ctx));
        EXPECT(refused(msg_with([](W::Header &m) { m.scale = DELTA * 2; }), "scale is not the context's", &ctx));
        EXPECT(refused(msg_with([](W::Header &m) { m.scale = 0.0; }), "scale", nullptr));
        EXPECT(refused(msg_with([](W::Header &m) { m.moduli[1] += 2; }), "modulus is not the context's", &ctx));
        EXPECT(refused(msg_with([](W::Header &m) { m.log_n = 11; }), "log_n", &ctx));
        EXPECT(refused(msg_with([](W::Header &m) { m.payload_bytes += 8; }, false), "payload_bytes", &ctx));
        EXPECT(refused(msg_with([](W::Header &m) { m.magic[0] = 'X'; }), "magic", nullptr));
        EXPECT(refused(msg_with([](W::Header &m) { m.count = UINT64_MAX / 3; }), "count", nullptr));  // the payload size wraps
        // two different a_seeds: whichever message differs, the second is the one that disagrees with the first
        for (const D::Expect *e : {(const D::Expect *)nullptr, &ctx}) {
            EXPECT(refused(msg_with([](W::Header &m) { m.a_seed[31] ^= 1; }), "a_seed differs", e) && err.find("message 1") != std::string::npos);
            EXPECT(refused(msg_with([](W::Header &m) { m.a_seed[0] ^= 0x80; }), "a_seed differs", e));
            // a nonce0 out of step, by one and by a block, and one beyond the nonce space
            EXPECT(refused(msg_with([](W::Header &m) { m.nonce0 += 1; }), "nonce0 is not", e) && err.find(where) != std::string::npos);
            EXPECT(refused(msg_with([](W::Header &m) { m.nonce0 += DIM; }), "nonce0 is not", e));
            EXPECT(refused(msg_with([](W::Header &m) { m.nonce0 = (1ull << 40) - 1; }), "nonce0", e));
        }
    }
    {  // both messages at one nonce0 (a repeated block message) is out of step too
        std::vector<unsigned char> v = two;
        message(v, 1)->nonce0 = message(v, 0)->nonce0;
        EXPECT(refused(v, "message 1: nonce0 is not", &ctx));
    }
    {  // without a context the messages must still agree on the ring
        std::vector<unsigned char> v = two;
        W::Header *m = message(v, 1);
        m->log_n = 11;
        (void)W::payload_bytes(m->log_n, m->count, m->n_polys, m->n_limbs, m->moduli, &m->payload_bytes);
        EXPECT(refused(v, "log_n differs", nullptr));
    }
    // ---- every single-byte mutation of the container header and of the second message's header: never a fault; with a context only the
    // bytes of first_vector / n_rows that keep the same two blocks are free, and an accepted delta keeps its exact length
    for (size_t base : {(size_t)0, sizeof(D::Header) + msg}) {
        const size_t span = base == 0 ? sizeof(D::Header) : sizeof(W::Header);
        for (size_t i = 0; i < span; i++)
            for (unsigned char flip : {(unsigned char)0x01, (unsigned char)0x80, (unsigned char)0xFF}) {
                std::vector<unsigned char> v = two;
                v[base + i] ^= flip;
                if (run(v, v.size(), v.size(), &ctx, &out, &err)) {
                    const bool free_byte = base == 0 && i >= 24 && i < 40;  // rows that touch the same two blocks (first_block now binds nonce0)
                    EXPECT(free_byte);
                    EXPECT(out.n_blocks == 2);
                }
                (void)run(v, v.size(), v.size(), nullptr, &out, &err);
            }
    }
    // ---- the unseeded validator refuses a seeded container by its magic
    EXPECT(!D::check(two.data(), two.size(), &ctx, &out, nullptr, &err) && err.find("magic") != std::string::npos);
    if (failures) return 1;
    std::puts("delta_seeded_header_check ok");
    return 0;
}
