// image_matching_amd/csrc/db_delta.cpp — the "database deltas" and "seeded database deltas" sections of include/hydia.h: the
// enroller-to-sender hand-off as a container (delta_format.h) of ordinary wire messages, in its two forms — whole ciphertexts under the
// PUBLIC key (CT_BATCH messages), or the c0 halves alone from an enroller that holds the SECRET key (SEEDED_QUERY messages).  One
// maker, one apply, one size and one peek helper serve both; a Kind names what goes with each form.
//
// Make (the enroller's context): update_blocks' diag_pack + encrypt_device (seeded: encrypt_sym_device) per touched block, k_wire_pack
// straight from the block buffer, the packed rows copied into the caller's buffer (client.cpp, delta_blocks); the headers are written last.
// Apply (the sender's context, database only): the container and every message header are validated on the host before anything is
// allocated; then TWO passes over the packed blocks, each uploaded into ONE pooled buffer: k_wire_check over every block first, and
// only when every residue passed the database is grown and the blocks are added (k_db_accumulate_wire) or stored (k_db_store_wire)
// from their packed form — no 64-bit image of a block, and no device memory that grows with the number of blocks.  Seeded: the same
// two passes over packed HALF blocks; k_db_accumulate_seeded / k_db_store_seeded write c0 and regenerate a straight into the
// resident layout.
#include <algorithm>
#include <cstring>
#include <string>

#include "capi_internal.h"
#include "delta_format.h"

using namespace hydia;
namespace W = hydia::wire;
namespace D = hydia::delta;
#define fail hydia_fail

namespace {

// a container form and what goes with it in the library
struct Kind {
    const D::Form &f;
    bool seeded;                     // the maker holds the secret key and draws a under a public a_seed; pass 2 regenerates a
    const char *no_key;              // the maker's refusal without its key
    const char *store, *accumulate;  // the timers of pass 2
};
const Kind WHOLE{D::WHOLE, false, "hydia: public key not loaded (a delta is encrypted under the receiver's public key)", "k_db_store_wire",
                 "k_db_accumulate_wire"};
const Kind SEEDED{D::SEEDED, true, "hydia: secret key not loaded (a seeded delta is the secret-key holder's; hydia_db_delta_make takes the public key)",
                  "k_db_store_seeded", "k_db_accumulate_seeded"};

const uint64_t *moduli_of(const Context &cx) { return reinterpret_cast<const uint64_t *>(cx.q.data()); }
D::Expect expect_of(const Context &cx) {
    return D::Expect{W::Expect{(uint32_t)cx.prm.logN, (uint32_t)cx.nQ, (uint32_t)cx.nP, (uint32_t)cx.prm.dnum, moduli_of(cx), cx.delta}, (uint32_t)cx.prm.dim};
}
bool delta_size(const Kind &k, const Context &cx, size_t first_vector, size_t n, uint64_t *total) {
    return D::total_bytes(k.f, (uint32_t)cx.prm.logN, (uint32_t)cx.nQ, moduli_of(cx), (uint32_t)cx.prm.dim, first_vector, n, total) && *total <= SIZE_MAX;
}
int delta_bytes(const Kind &k, const hydia_ctx *ctx, size_t first_vector, size_t n, size_t *bytes) {
    REQUIRE(ctx && bytes, "null argument");
    *bytes = 0;
    uint64_t total;
    REQUIRE(n >= 1, "a delta needs at least one row");
    REQUIRE(delta_size(k, ctx->cx, first_vector, n, &total), "first_vector + n, or the size of the delta, overflows");
    *bytes = (size_t)total;
    return HYDIA_OK;
}
int delta_peek(const Kind &k, const void *buf, size_t len, hydia_db_delta_info *out) {
    REQUIRE(buf && out, "null argument");
    D::Header h;
    std::string err;
    if (!D::check(k.f, buf, len, nullptr, &h, nullptr, nullptr, &err)) return fail(HYDIA_ERR_ARG, err);
    std::memset(out, 0, sizeof *out);
    out->version = h.version; out->vector_dim = h.vector_dim; out->babies = h.babies; out->first_vector = h.first_vector; out->n_rows = h.n_rows;
    out->first_block = h.first_block; out->n_blocks = h.n_blocks; out->total_bytes = len;
    return HYDIA_OK;
}
// what the makers check before any work and the frame they share: size, the payloads through run(payload0, stride), then the headers.
// a_seed: the seeded form's public seed, which every message carries (nullptr for a whole delta)
template <class Run>
int make_delta(const Kind &k, hydia_ctx *ctx, size_t first_vector, size_t n, const uint8_t *seed, const uint8_t *a_seed, int babies, size_t first_block,
               void *buf, size_t cap, size_t *len, Run run) {
    Context &cx = ctx->cx;
    const uint32_t dim = (uint32_t)cx.prm.dim;
    REQUIRE(len, "null argument");
    *len = 0;
    REQUIRE(seed && (a_seed || !k.seeded), "null argument");
    REQUIRE(n >= 1, "a delta needs at least one row");
    REQUIRE(D::is_form((uint64_t)(babies < 0 ? 0 : babies), dim), "babies must be vector_dim or a power of two >= 2 dividing it");
    REQUIRE(n <= SIZE_MAX / sizeof(double) / (size_t)dim, "row count out of range");
    REQUIRE(!k.seeded || std::memcmp(seed, a_seed, 32) != 0, "a_seed must differ from seed: a_seed is public, seed keeps the noise secret");
    uint64_t total, blocks, nonce = 0;
    REQUIRE(delta_size(k, cx, first_vector, n, &total), "first_vector + n, or the size of the delta, overflows");
    (void)D::touched_blocks(first_vector, n, (uint64_t)cx.slots, &blocks);
    const uint64_t g0 = first_vector / (uint64_t)cx.slots;
    REQUIRE(!k.f.nonce0 || D::block_nonce(first_block, g0 + blocks - 1, dim, &nonce),
            "first_block + number of blocks exceeds the 2^40 nonce space of the encryption sampler");
    if (!(k.seeded ? cx.d_sk : cx.d_pk)) return fail(HYDIA_ERR_STATE, k.no_key);
    *len = (size_t)total;
    REQUIRE(buf && cap >= total, "cap is smaller than the delta (len holds the bytes it needs)");
    W::Header m = W::make_header(k.f.type, (uint32_t)cx.prm.logN, (uint64_t)dim, k.f.n_polys, (uint32_t)cx.nQ, 0, cx.delta, a_seed, 0, moduli_of(cx));
    const size_t stride = sizeof m + (size_t)m.payload_bytes;
    unsigned char *out = (unsigned char *)buf;
    run(out + sizeof(D::Header) + sizeof m, stride);  // (the check of the noise stream's nonces throws before the first block)
    const D::Header h = D::make_header(k.f, dim, (uint64_t)babies, first_vector, n, first_block, blocks);
    std::memcpy(out, &h, sizeof h);
    for (uint64_t b = 0; b < blocks; b++) {
        if (k.f.nonce0) {
            (void)D::block_nonce(first_block, g0 + b, dim, &nonce);
            m.nonce0 = nonce;
        }
        std::memcpy(out + sizeof h + b * stride, &m, sizeof m);
    }
    return HYDIA_OK;
}
const char *kind_name(int kind) {
    switch (kind) {
        case 1: return "kind 1 (approach 1, row packing)";
        case 3: return "kind 3 (approach 3, chunk packing)";
        case 4: return "kind 4 (HERS, column packing)";
        default: return "an unknown kind";
    }
}
int apply_delta(const Kind &k, hydia_ctx *ctx, const void *buf, size_t len) {
    REQUIRE(ctx && buf, "null argument");
    use_device(ctx);
    Context &cx = ctx->cx;
    const D::Expect e = expect_of(cx);
    D::Header h;
    std::string err;
    ChaChaKey akey;  // (client.cpp make_key: the seed's bytes as eight little-endian words)
    if (!D::check(k.f, buf, len, &e, &h, nullptr, reinterpret_cast<uint8_t *>(akey.k), &err)) return fail(HYDIA_ERR_ARG, err);
    const std::string refused = k.f.refused;
    // ---- the target
    if (cx.db_plain())
        return fail(HYDIA_ERR_STATE, "hydia: a plain gallery (kind 7 / 8) is resident: it holds plaintexts and is updated in place by hydia_plain_db_update (a delta carries ciphertexts)");
    const bool resident = cx.d_db && cx.db_cts && cx.db_kind != 0;
    if (resident && cx.db_kind != 5 && cx.db_kind != 6)
        return fail(HYDIA_ERR_STATE, std::string("hydia: a database of ") + kind_name(cx.db_kind) + " is resident: a delta applies to a diagonal database (kind 5 or 6)");
    if (resident) {
        REQUIRE(h.babies == (uint64_t)cx.db_babies, refused + "babies is not the form of the resident database (hydia_db_babies)");
        REQUIRE(h.first_vector <= cx.db_vectors, refused + "first_vector lies past the end of the database (a delta leaves no holes)");
    } else if (h.first_vector != 0) {
        return fail(HYDIA_ERR_STATE, "hydia: no database resident: only a delta with first_vector = 0 enrols one");
    }
    const int dim = cx.prm.dim, npoly = (int)k.f.n_polys;
    const size_t Nh = (size_t)cx.slots, end = (size_t)(h.first_vector + h.n_rows), g0 = (size_t)h.first_vector / Nh;
    const size_t n_new = std::max(resident ? cx.db_vectors : (size_t)0, end), G_new = (n_new + Nh - 1) / Nh;
    REQUIRE(G_new <= SIZE_MAX / 2 / (size_t)dim, refused + "first_vector + n_rows out of range");
    const WireRows R = hc::wire_rows(cx.q.data(), cx.N, cx.nQ);
    const size_t packed = (size_t)dim * npoly * R.off[cx.nQ] * sizeof(u64), stride = sizeof(W::Header) + packed;  // (check: every payload is this long)
    const unsigned char *payload0 = (const unsigned char *)buf + sizeof(D::Header) + sizeof(W::Header);
    PoolBuf d(cx.pool, packed), f(cx.pool, 8);
    auto upload = [&](size_t b) { HIP_CHECK(hipMemcpyAsync(d.p, payload0 + b * stride, packed, hipMemcpyHostToDevice, cx.stream)); };
    // ---- pass 1: every residue of every block, before the database is grown or a byte of it is written (a seeded delta's a is
    // canonical by construction)
    HIP_CHECK(hipMemsetAsync(f.p, 0, 8, cx.stream));
    for (size_t b = 0; b < h.n_blocks; b++) {
        upload(b);
        cx.timer_begin("k_wire_check");
        hc::wire_check(cx.stream, cx.d_mod, cx.N, d.p, (size_t)dim, npoly, cx.nQ, R, reinterpret_cast<unsigned *>(f.p));
        cx.timer_end("k_wire_check");
    }
    unsigned flag = 1;
    HIP_CHECK(hipMemcpyAsync(&flag, f.p, sizeof flag, hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
    if (flag != 0) return fail(HYDIA_ERR_ARG, "hydia: " + refused + "a residue is at or above its modulus");
    // ---- pass 2: room (throws before anything is touched when it does not fit), then the blocks from their packed form
    size_t G_old = 0;
    if (resident) {
        G_old = cx.db_cts / (size_t)dim;
        cx.db_grow(n_new, G_new * (size_t)dim);
    } else {
        cx.db_kind = 0;
        cx.db_resize(n_new, G_new * (size_t)dim, (int)h.babies);
    }
    for (size_t b = 0; b < h.n_blocks; b++) {
        const bool store = g0 + b >= G_old;
        const size_t t0 = (g0 + b) * (size_t)dim;
        upload(b);
        cx.timer_begin(store ? k.store : k.accumulate);
        if (k.seeded) hc::db_wire_seeded(cx.stream, akey, (u64)(h.first_block + g0 + b) * (u64)dim, cx.d_mod, cx.N, cx.nQ, d.p, R, cx.d_db, t0, dim, cx.db_lay, store);
        else hc::db_wire(cx.stream, cx.d_mod, cx.N, cx.nQ, d.p, R, cx.d_db, t0, dim, cx.db_lay, store);
        cx.timer_end(store ? k.store : k.accumulate);
    }
    cx.sync();
    if (!resident) {
        cx.db_kind = h.babies < (uint64_t)dim ? 6 : 5;
        cx.db_babies = (int)h.babies;
    }
    return HYDIA_OK;
}

}  // namespace

extern "C" {

int hydia_db_delta_bytes(const hydia_ctx *ctx, size_t first_vector, size_t n, size_t *bytes) {
    API_BEGIN
    return delta_bytes(WHOLE, ctx, first_vector, n, bytes);
    API_END
}
int hydia_db_delta_peek(const void *buf, size_t len, hydia_db_delta_info *out) {
    API_BEGIN
    return delta_peek(WHOLE, buf, len, out);
    API_END
}
int hydia_db_delta_make(hydia_ctx *ctx, size_t first_vector, double *rows, size_t n, int normalise, const uint8_t seed[32], int babies,
                        size_t first_block, void *buf, size_t cap, size_t *len) {
    API_BEGIN
    REQUIRE(ctx && rows, "null argument");
    use_device(ctx);
    return make_delta(WHOLE, ctx, first_vector, n, seed, nullptr, babies, first_block, buf, cap, len, [&](unsigned char *payload0, size_t stride) {
        client_db_delta_make(ctx->cx, first_vector, rows, n, normalise, seed, babies, first_block, payload0, stride);
    });
    API_END
}
int hydia_db_delta_make_device(hydia_ctx *ctx, size_t first_vector, const hydia_dev_rows *rows, int normalise, const uint8_t seed[32], int babies,
                               size_t first_block, void *buf, size_t cap, size_t *len) {
    API_BEGIN
    REQUIRE(ctx && rows, "null argument");
    use_device(ctx);
    DevRows r;
    if (int code = hydia_check_dev_rows(ctx, rows, &r)) return code;
    return make_delta(WHOLE, ctx, first_vector, r.n, seed, nullptr, babies, first_block, buf, cap, len, [&](unsigned char *payload0, size_t stride) {
        client_db_delta_make_device(ctx->cx, first_vector, r, normalise, seed, babies, first_block, payload0, stride);
    });
    API_END
}
int hydia_db_delta_apply(hydia_ctx *ctx, const void *buf, size_t len) {
    API_BEGIN
    return apply_delta(WHOLE, ctx, buf, len);
    API_END
}

int hydia_db_delta_seeded_bytes(const hydia_ctx *ctx, size_t first_vector, size_t n, size_t *bytes) {
    API_BEGIN
    return delta_bytes(SEEDED, ctx, first_vector, n, bytes);
    API_END
}
int hydia_db_delta_seeded_peek(const void *buf, size_t len, hydia_db_delta_info *out) {
    API_BEGIN
    return delta_peek(SEEDED, buf, len, out);
    API_END
}
int hydia_db_delta_make_seeded(hydia_ctx *ctx, size_t first_vector, double *rows, size_t n, int normalise, const uint8_t seed[32],
                               const uint8_t a_seed[32], int babies, size_t first_block, void *buf, size_t cap, size_t *len) {
    API_BEGIN
    REQUIRE(ctx && rows, "null argument");
    use_device(ctx);
    return make_delta(SEEDED, ctx, first_vector, n, seed, a_seed, babies, first_block, buf, cap, len, [&](unsigned char *payload0, size_t stride) {
        client_db_delta_make_seeded(ctx->cx, first_vector, rows, n, normalise, seed, a_seed, babies, first_block, payload0, stride);
    });
    API_END
}
int hydia_db_delta_make_seeded_device(hydia_ctx *ctx, size_t first_vector, const hydia_dev_rows *rows, int normalise, const uint8_t seed[32],
                                      const uint8_t a_seed[32], int babies, size_t first_block, void *buf, size_t cap, size_t *len) {
    API_BEGIN
    REQUIRE(ctx && rows, "null argument");
    use_device(ctx);
    DevRows r;
    if (int code = hydia_check_dev_rows(ctx, rows, &r)) return code;
    return make_delta(SEEDED, ctx, first_vector, r.n, seed, a_seed, babies, first_block, buf, cap, len, [&](unsigned char *payload0, size_t stride) {
        client_db_delta_make_seeded_device(ctx->cx, first_vector, r, normalise, seed, a_seed, babies, first_block, payload0, stride);
    });
    API_END
}
int hydia_db_delta_apply_seeded(hydia_ctx *ctx, const void *buf, size_t len) {
    API_BEGIN
    return apply_delta(SEEDED, ctx, buf, len);
    API_END
}

}  // extern "C"
