// tests/delta_header_check.cpp — the validator of a database delta's container (image_matching_amd/csrc/delta_format.h with
// wire_format.h, included alone) under AddressSanitizer and UndefinedBehaviorSanitizer: every refusal of the container check, every
// prefix of a valid delta's headers, every single-byte mutation of the container header and of a message header, and the shapes whose
// arithmetic wraps 64 bits.  Every buffer handed to the validator is a heap block of exactly the bytes it may read, so a read past a
// short buffer is a sanitizer report.  Exits 0 when every expectation held (tests/test_db_delta_cpu.py runs it).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "delta_format.h"
#include "wire_format.h"

namespace W = hydia::wire;
namespace D = hydia::delta;

static int failures = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);    \
            failures++;                                                \
        }                                                              \
    } while (0)

// check() on a heap copy of exactly `have` bytes of src, claiming `len`
static bool run(const std::vector<unsigned char> &src, size_t have, size_t len, const D::Expect *e, D::Header *out, std::string *err) {
    unsigned char *heap = have ? (unsigned char *)std::malloc(have) : nullptr;
    if (have) std::memcpy(heap, src.data(), have);
    uint32_t log_n = 0;
    const bool ok = D::check(heap, len, e, out, &log_n, err);
    if (ok) EXPECT(log_n == 10);
    std::free(heap);
    return ok;
}
static bool names(const std::string &err, const char *field) { return err.find("database delta refused") != std::string::npos && err.find(field) != std::string::npos; }

// a small ring keeps whole deltas in a few hundred kilobytes: N = 1024 (512 slots), vector_dim 4, three limbs of 60 / 46 / 45 bits
static uint64_t moduli[4] = {(1ull << 59) + 1001, (1ull << 45) + 77, (1ull << 44) + 55, (1ull << 59) + 9};
static const double DELTA = 35184372088832.0;
static const uint32_t DIM = 4;

static std::vector<unsigned char> make(uint64_t babies, uint64_t first_vector, uint64_t n_rows, uint64_t n_blocks, uint64_t first_block = 0) {
    const D::Header h = D::make_header(DIM, babies, first_vector, n_rows, first_block, n_blocks);
    const W::Header m = W::make_header(W::CT_BATCH, 10, DIM, 2, 3, 0, DELTA, nullptr, 0, moduli);
    std::vector<unsigned char> v(sizeof h + n_blocks * (sizeof m + m.payload_bytes), 0);
    std::memcpy(v.data(), &h, sizeof h);
    for (uint64_t b = 0; b < n_blocks; b++) std::memcpy(v.data() + sizeof h + b * (sizeof m + m.payload_bytes), &m, sizeof m);
    return v;
}
static W::Header *message(std::vector<unsigned char> &v, uint64_t b) {
    W::Header m;
    std::memcpy(&m, v.data() + sizeof(D::Header), sizeof m);
    return reinterpret_cast<W::Header *>(v.data() + sizeof(D::Header) + b * (sizeof m + m.payload_bytes));  // (8-byte aligned: every size is a multiple of 8)
}

int main() {
    const D::Expect ctx{W::Expect{10, 3, 1, 3, moduli, DELTA}, DIM};
    D::Header out;
    std::string err;
    // ---- valid deltas: one block, two blocks (rows 500 .. 519 straddle slots = 512), three blocks, the pre-rotated form, a nonce offset
    const std::vector<unsigned char> one = make(DIM, 0, 512, 1), two = make(DIM, 500, 20, 2), three = make(2, 511, 514, 3, 7);
    for (const auto *v : {&one, &two, &three}) {
        EXPECT(run(*v, v->size(), v->size(), nullptr, &out, &err));
        EXPECT(run(*v, v->size(), v->size(), &ctx, &out, &err));
    }
    EXPECT(run(three, three.size(), three.size(), &ctx, &out, &err) && out.n_blocks == 3 && out.babies == 2 && out.first_vector == 511 &&
           out.n_rows == 514 && out.first_block == 7 && out.vector_dim == DIM);
    // the size arithmetic agrees with the bytes
    uint64_t total = 0;
    EXPECT(D::total_bytes(10, 3, moduli, DIM, 500, 20, &total) && total == two.size());
    EXPECT(D::total_bytes(10, 3, moduli, DIM, 511, 514, &total) && total == three.size());
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
    EXPECT(!D::check(nullptr, two.size(), &ctx, &out, nullptr, &err) && names(err, "null"));
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
        EXPECT(refused(with(two, [](D::Header &h) { h.version = 2; }), "version", e));
        EXPECT(refused(with(two, [](D::Header &h) { h.reserved = 1; }), "reserved", e));
        EXPECT(refused(with(two, [](D::Header &h) { h.vector_dim = 0; }), "vector_dim", e));
        EXPECT(refused(with(two, [](D::Header &h) { h.vector_dim = 3; }), "vector_dim", e));
        for (uint64_t babies : {(uint64_t)0, (uint64_t)1, (uint64_t)3, (uint64_t)8, UINT64_MAX})
            EXPECT(refused(with(two, [&](D::Header &h) { h.babies = babies; }), "babies", e));
        EXPECT(refused(with(two, [](D::Header &h) { h.n_rows = 0; }), "n_rows", e));
        EXPECT(refused(with(two, [](D::Header &h) { h.n_blocks = 0; }), "n_blocks", e));
        // n_blocks against first_vector / n_rows: the rows touch one block, or three, and the delta carries two
        EXPECT(refused(with(two, [](D::Header &h) { h.n_rows = 12; }), "n_blocks", e));
        EXPECT(refused(with(two, [](D::Header &h) { h.n_rows = 525; }), "n_blocks", e));
        EXPECT(refused(with(two, [](D::Header &h) { h.first_vector = 512; }), "n_blocks", e));
        EXPECT(refused(with(one, [](D::Header &h) { h.n_rows = 513; }), "n_blocks", e));
        EXPECT(refused(with(two, [](D::Header &h) { h.n_blocks = 1; }), "n_blocks", e));  // (before the trailing message is looked at)
        EXPECT(refused(with(two, [](D::Header &h) { h.n_blocks = 3; h.n_rows = 600; }), "truncated", e));
        // the overflow cases: first_vector + n_rows wraps; a huge n_blocks ends at the buffer's end, not in a long loop
        EXPECT(refused(with(two, [](D::Header &h) { h.first_vector = UINT64_MAX - 5; h.n_rows = 6; }), "overflows", e));
        EXPECT(refused(with(two, [](D::Header &h) { h.first_vector = UINT64_MAX; h.n_rows = 1; }), "overflows", e));
        EXPECT(refused(with(two, [](D::Header &h) { h.first_vector = 0; h.n_rows = UINT64_MAX; h.n_blocks = UINT64_MAX / 512 + 1; }), "truncated", e));
        EXPECT(refused(with(two, [](D::Header &h) { h.n_blocks = UINT64_MAX; }), "n_blocks", e));
    }
    EXPECT(refused(with(two, [](D::Header &h) { h.vector_dim = 8; h.babies = 8; }), "vector_dim is not the context's", &ctx));
    {  // the largest range that does not wrap is arithmetic, not a fault
        uint64_t blocks = 0;
        EXPECT(D::touched_blocks(UINT64_MAX - 6, 6, 512, &blocks) && blocks == 1);
        EXPECT(!D::touched_blocks(UINT64_MAX - 5, 6, 512, &blocks) && !D::touched_blocks(0, 0, 512, &blocks));
        EXPECT(D::touched_blocks(0, UINT64_MAX, 512, &blocks) && blocks == UINT64_MAX / 512 + 1);
        uint64_t t = 0;
        EXPECT(!D::total_bytes(10, 3, moduli, DIM, 0, UINT64_MAX, &t));       // blocks x message bytes wraps
        EXPECT(!D::total_bytes(10, 3, moduli, DIM, UINT64_MAX, 1, &t));       // first_vector + n wraps
        EXPECT(!D::total_bytes(10, 3, moduli, DIM, 0, 0, &t));                // no rows
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
        EXPECT(refused(msg_with([](W::Header &m) { m.n_polys = 3; }), "n_polys is not 2", &ctx));
        EXPECT(refused(msg_with([](W::Header &m) { m.n_polys = 3; }), "n_polys is not 2", nullptr));
        EXPECT(refused(msg_with([](W::Header &m) { m.n_limbs = 2; m.moduli[2] = 0; }), "n_limbs is not n_q", &ctx));
        EXPECT(refused(msg_with([](W::Header &m) { m.n_limbs = 4; m.moduli[3] = moduli[3]; }), "n_limbs", &ctx));
        EXPECT(refused(msg_with([](W::Header &m) { m.scale = DELTA * 2; }), "scale is not the context's", &ctx));
        EXPECT(refused(msg_with([](W::Header &m) { m.scale = 0.0; }), "scale", nullptr));
        EXPECT(refused(msg_with([](W::Header &m) { m.type = W::SEEDED_QUERY; m.n_polys = 1; }), "type is not a ciphertext batch", &ctx));
        EXPECT(refused(msg_with([](W::Header &m) { m.type = W::PUBLIC_KEY; m.count = 1; m.scale = 0.0; }), "type is not a ciphertext batch", nullptr));
        EXPECT(refused(msg_with([](W::Header &m) { m.type = 7; }), "type is unknown", &ctx));
        EXPECT(refused(msg_with([](W::Header &m) { m.moduli[1] += 2; }), "modulus is not the context's", &ctx));
        EXPECT(refused(msg_with([](W::Header &m) { m.log_n = 11; }), "log_n", &ctx));
        EXPECT(refused(msg_with([](W::Header &m) { m.payload_bytes += 8; }, false), "payload_bytes", &ctx));
        EXPECT(refused(msg_with([](W::Header &m) { m.magic[0] = 'X'; }), "magic", nullptr));
        EXPECT(refused(msg_with([](W::Header &m) { m.count = UINT64_MAX / 3; }), "count", nullptr));  // the payload size wraps
    }
    {  // without a context the messages must still agree on the ring; vector_dim must fit its slots
        std::vector<unsigned char> v = two;
        W::Header *m = message(v, 1);
        m->log_n = 11;
        (void)W::payload_bytes(m->log_n, m->count, m->n_polys, m->n_limbs, m->moduli, &m->payload_bytes);
        EXPECT(refused(v, "log_n differs", nullptr));
    }
    // ---- every single-byte mutation of the container header and of the second message's header: never a fault; with a context only the
    // bytes of first_block (diagnosis only) are free, and an accepted delta keeps its exact length
    for (size_t base : {(size_t)0, sizeof(D::Header) + msg}) {
        const size_t span = base == 0 ? sizeof(D::Header) : sizeof(W::Header);
        for (size_t i = 0; i < span; i++)
            for (unsigned char flip : {(unsigned char)0x01, (unsigned char)0x80, (unsigned char)0xFF}) {
                std::vector<unsigned char> v = two;
                v[base + i] ^= flip;
                if (run(v, v.size(), v.size(), &ctx, &out, &err)) {
                    const bool free_byte = base == 0 && ((i >= 40 && i < 48) /* first_block */ || (i >= 24 && i < 40) /* rows that touch the same two blocks */);
                    EXPECT(free_byte);
                    EXPECT(out.n_blocks == 2);
                }
                (void)run(v, v.size(), v.size(), nullptr, &out, &err);
            }
    }
    if (failures) return 1;
    std::puts("delta_header_check ok");
    return 0;
}
