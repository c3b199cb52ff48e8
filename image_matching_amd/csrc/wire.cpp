// image_matching_amd/csrc/wire.cpp — the "wire messages" section of include/hydia.h: ciphertext batches, seeded queries, evaluation
// keys and the public key as packed, checked, self-describing messages (wire_format.h), and the key-set file.
//
// Out: the rows are packed on the device (k_wire_pack) and the packed bytes are copied to the host, never the 64-bit image.
// In: the header is validated before anything is allocated or any key or handle is touched; the packed bytes are uploaded, unpacked and
// range-checked on the device (k_wire_unpack_check) into a fresh handle or pool scratch, and a key is installed only after the check passed.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "capi_internal.h"
#include "wire_format.h"

using namespace hydia;
namespace W = hydia::wire;
#define fail hydia_fail

namespace {

const uint64_t *moduli_of(const Context &cx) { return reinterpret_cast<const uint64_t *>(cx.q.data()); }
W::Expect expect_of(const Context &cx) {
    return W::Expect{(uint32_t)cx.prm.logN, (uint32_t)cx.nQ, (uint32_t)cx.nP, (uint32_t)cx.prm.dnum, moduli_of(cx), cx.delta};
}
struct PinnedBuf {
    void *p = nullptr;
    explicit PinnedBuf(size_t n) { HIP_CHECK(hipHostMalloc(&p, n, hipHostMallocDefault)); }
    ~PinnedBuf() { (void)hipHostFree(p); }
};
struct FileCloser {
    FILE *f;
    ~FileCloser() {
        if (f) fclose(f);
    }
};
// rows in device memory -> the payload in host memory
void pack_to_host(Context &cx, const u64 *src, size_t item_stride, size_t poly_stride, size_t items, int npoly, int nl, unsigned char *payload) {
    const WireRows R = hc::wire_rows(cx.q.data(), cx.N, nl);
    const size_t bytes = items * (size_t)npoly * R.off[nl] * sizeof(u64);
    PoolBuf d(cx.pool, bytes);
    cx.timer_begin("k_wire_pack");
    hc::wire_pack(cx.stream, cx.d_mod, cx.N, src, item_stride, poly_stride, items, npoly, nl, R, d.p);
    cx.timer_end("k_wire_pack");
    HIP_CHECK(hipMemcpyAsync(payload, d.p, bytes, hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
}
// a payload uploaded once, unpacked in one or several launches, the flag read at the end
struct Unpacker {
    Context &cx;
    WireRows R;
    int nl;
    PoolBuf d, f;
    Unpacker(Context &c, const unsigned char *payload, size_t bytes, int nl_) : cx(c), R(hc::wire_rows(c.q.data(), c.N, nl_)), nl(nl_), d(c.pool, bytes), f(c.pool, 8) {
        HIP_CHECK(hipMemsetAsync(f.p, 0, 8, cx.stream));
        HIP_CHECK(hipMemcpyAsync(d.p, payload, bytes, hipMemcpyHostToDevice, cx.stream));
    }
    // items first .. first + items - 1 of the message, npoly polynomials each
    void rows(size_t first, size_t items, int npoly, u64 *dst, size_t item_stride, size_t poly_stride) {
        cx.timer_begin("k_wire_unpack_check");
        hc::wire_unpack_check(cx.stream, cx.d_mod, cx.N, d.p + first * npoly * R.off[nl], dst, item_stride, poly_stride, items, npoly, nl, R,
                              reinterpret_cast<unsigned *>(f.p));
        cx.timer_end("k_wire_unpack_check");
    }
    bool canonical() {
        unsigned flag = 1;
        HIP_CHECK(hipMemcpyAsync(&flag, f.p, sizeof flag, hipMemcpyDeviceToHost, cx.stream));
        cx.sync();
        return flag == 0;
    }
};
const char *NOT_CANONICAL = "hydia: wire message refused: a residue is at or above its modulus";

size_t eval_key_message_bytes(const Context &cx, bool seeded) {
    return sizeof(W::Header) + (size_t)cx.prm.dnum * (seeded ? 1 : 2) * W::rows_bytes((uint32_t)cx.prm.logN, (uint32_t)cx.nT, moduli_of(cx));
}
size_t public_key_message_bytes(const Context &cx, bool seeded) {
    return sizeof(W::Header) + (size_t)(seeded ? 1 : 2) * W::rows_bytes((uint32_t)cx.prm.logN, (uint32_t)cx.nQ, moduli_of(cx));
}

// hydia_key_to_wire without the exception frame (hydia_keys_save calls it per key)
int key_to_wire(hydia_ctx *ctx, int rot, int seeded, unsigned char *buf, size_t cap, size_t *written) {
    Context &cx = ctx->cx;
    REQUIRE(rot >= -1 && rot < cx.slots, "rot outside -1 (the public key), 0 .. slots - 1");
    const u64 *src;
    W::Header h;
    size_t items, item_stride, poly_stride;
    int nl;
    if (rot < 0) {
        if (!cx.d_pk) return fail(HYDIA_ERR_STATE, "hydia: public key not loaded");
        if (seeded && !(cx.has_key_seed && cx.pk_seeded))
            return fail(HYDIA_ERR_STATE, "hydia: the public key is not covered by the context's key seed (hydia_keygen_seeded makes such a key; send it whole)");
        src = cx.d_pk; items = 1; nl = cx.nQ; poly_stride = (size_t)cx.nQ * cx.N; item_stride = 2 * poly_stride;
        h = W::make_header(seeded ? W::PUBLIC_KEY_SEEDED : W::PUBLIC_KEY, (uint32_t)cx.prm.logN, 1, seeded ? 1 : 2, (uint32_t)nl, 0, 0.0,
                           seeded ? cx.key_seed : nullptr, 0, moduli_of(cx));
    } else {
        const Context::EvalKey *k = nullptr;
        if (rot == 0) k = &cx.relin_key;
        else if (cx.rot_keys.count(rot)) k = &cx.rot_keys[rot];
        if (!k || !k->d) return fail(HYDIA_ERR_STATE, "hydia: evaluation key not loaded");
        if (seeded && !(cx.has_key_seed && k->seeded))
            return fail(HYDIA_ERR_STATE, "hydia: this evaluation key is not covered by the context's key seed (hydia_keygen_seeded makes such keys; send it whole)");
        src = k->d; items = (size_t)cx.prm.dnum; nl = cx.nT; poly_stride = (size_t)cx.nT * cx.N; item_stride = 2 * poly_stride;
        h = W::make_header(seeded ? W::EVAL_KEY_SEEDED : W::EVAL_KEY, (uint32_t)cx.prm.logN, (uint32_t)cx.prm.dnum, seeded ? 1 : 2, (uint32_t)nl,
                           (uint32_t)rot, 0.0, seeded ? cx.key_seed : nullptr, 0, moduli_of(cx));
    }
    const size_t need = sizeof h + h.payload_bytes;
    *written = need;
    REQUIRE(buf && cap >= need, "cap is smaller than the message (written holds the bytes it needs)");
    pack_to_host(cx, src, item_stride, poly_stride, items, (int)h.n_polys, nl, buf + sizeof h);
    std::memcpy(buf, &h, sizeof h);
    return HYDIA_OK;
}
// hydia_key_from_wire without the exception frame; h = the message's header, already validated against the context
int key_from_wire(hydia_ctx *ctx, const W::Header &h, const unsigned char *payload, int *rot_out) {
    Context &cx = ctx->cx;
    if (cx.keys_borrowed) return fail(HYDIA_ERR_STATE, "hydia: this context borrows its keys from another context (re-key the owner)");
    const bool pk = h.type == W::PUBLIC_KEY || h.type == W::PUBLIC_KEY_SEEDED, seeded = W::is_seeded(h.type);
    const int nl = (int)h.n_limbs, npoly = (int)h.n_polys;
    const size_t row = (size_t)nl * cx.N;
    {
        PoolBuf tmp(cx.pool, (size_t)h.count * npoly * row * sizeof(u64));  // pool scratch: the key installed before stays untouched until the check passed
        Unpacker up(cx, payload, (size_t)h.payload_bytes, nl);
        up.rows(0, h.count, npoly, tmp.p, npoly * row, row);
        if (!up.canonical()) return fail(HYDIA_ERR_ARG, NOT_CANONICAL);
        if (pk) client_install_public_key(cx, tmp.p, seeded ? h.a_seed : nullptr);
        else client_install_eval_key(cx, (int)h.rot, tmp.p, seeded ? h.a_seed : nullptr);
    }
    if (rot_out) *rot_out = pk ? -1 : (int)h.rot;
    return HYDIA_OK;
}
int check_public_seed(const uint8_t *seed, const uint8_t *a_seed, uint64_t nonce0, size_t count) {
    REQUIRE(seed && a_seed, "null argument");
    REQUIRE(std::memcmp(seed, a_seed, 32) != 0, "a_seed equals seed: the public expansion seed must be independent of the secret one");
    REQUIRE(nonce0 <= W::NONCE_LIMIT && count <= W::NONCE_LIMIT - nonce0, "nonce0 + count must not exceed 2^40");
    return HYDIA_OK;
}
// the frame both seeded-query entries share: size, header, and run(payload, rows) in between
template <class Run>
int queries_to_wire(hydia_ctx *ctx, size_t count, const uint8_t *a_seed, uint64_t nonce0, void *buf, size_t cap, size_t *written, Run run) {
    Context &cx = ctx->cx;
    REQUIRE(written, "null argument");
    *written = 0;
    if (count == 0) return HYDIA_OK;
    const W::Header h = W::make_header(W::SEEDED_QUERY, (uint32_t)cx.prm.logN, (uint64_t)count, 1, (uint32_t)cx.nQ, 0, cx.delta, a_seed, nonce0, moduli_of(cx));
    REQUIRE(h.payload_bytes != 0, "probe count out of range");
    *written = sizeof h + h.payload_bytes;
    REQUIRE(buf && cap >= *written, "cap is smaller than the message (written holds the bytes it needs)");
    const WireRows R = hc::wire_rows(cx.q.data(), cx.N, cx.nQ);
    run(reinterpret_cast<u64 *>((unsigned char *)buf + sizeof h), &R);
    std::memcpy(buf, &h, sizeof h);
    return HYDIA_OK;
}

}  // namespace

extern "C" {

int hydia_wire_peek(const void *buf, size_t len, hydia_wire_info *out) {
    API_BEGIN
    REQUIRE(buf && out, "null argument");
    W::Header h;
    std::string err;
    if (!W::check(buf, len, true, nullptr, &h, &err)) return fail(HYDIA_ERR_ARG, err);
    std::memset(out, 0, sizeof *out);
    out->type = h.type; out->log_n = h.log_n; out->count = h.count; out->n_polys = h.n_polys; out->n_limbs = h.n_limbs; out->rot = h.rot;
    out->scale = h.scale; out->nonce0 = h.nonce0; out->header_bytes = sizeof h; out->payload_bytes = h.payload_bytes;
    std::memcpy(out->a_seed, h.a_seed, 32);
    return HYDIA_OK;
    API_END
}
size_t hydia_wire_ct_bytes(const hydia_ctx *ctx, uint64_t count, uint32_t n_polys, uint32_t n_limbs, int seeded) {
    if (!ctx || count == 0 || n_limbs < 1 || (int)n_limbs > ctx->cx.nQ) return 0;
    if (seeded ? (n_polys != 1 || (int)n_limbs != ctx->cx.nQ) : (n_polys != 2 && n_polys != 3)) return 0;
    uint64_t b;
    if (!W::payload_bytes((uint32_t)ctx->cx.prm.logN, count, n_polys, n_limbs, moduli_of(ctx->cx), &b) || b > SIZE_MAX - sizeof(W::Header)) return 0;
    return sizeof(W::Header) + (size_t)b;
}
size_t hydia_wire_eval_key_bytes(const hydia_ctx *ctx, int seeded) { return ctx ? eval_key_message_bytes(ctx->cx, seeded != 0) : 0; }
size_t hydia_wire_public_key_bytes(const hydia_ctx *ctx, int seeded) { return ctx ? public_key_message_bytes(ctx->cx, seeded != 0) : 0; }

int hydia_ct_to_wire(hydia_ctx *ctx, const hydia_ct *ct, void *buf, size_t cap, size_t *written) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && ct && written, "null argument");
    Context &cx = ctx->cx;
    const Ct &c = ct->c;
    REQUIRE(std::isfinite(c.scale) && c.scale > 0, "a ciphertext whose scale is not finite and positive has no message");
    const W::Header h = W::make_header(W::CT_BATCH, (uint32_t)cx.prm.logN, (uint64_t)c.X, (uint32_t)c.npoly, (uint32_t)c.nl, 0, c.scale, nullptr, 0, moduli_of(cx));
    const size_t need = sizeof h + h.payload_bytes;
    *written = need;
    REQUIRE(buf && cap >= need, "cap is smaller than the message (written holds the bytes it needs)");
    pack_to_host(cx, c.d, c.ct_elems(), c.poly_elems(), (size_t)c.X, c.npoly, c.nl, (unsigned char *)buf + sizeof h);  // a limb-prefix view: its limb stride
    std::memcpy(buf, &h, sizeof h);
    return HYDIA_OK;
    API_END
}
int hydia_ct_from_wire(hydia_ctx *ctx, const void *buf, size_t len, hydia_ct **out, size_t out_cap, size_t *n_out) {
    if (out)
        for (size_t i = 0; i < out_cap; i++) out[i] = nullptr;
    if (n_out) *n_out = 0;
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && buf && out && n_out, "null argument");
    Context &cx = ctx->cx;
    const W::Expect e = expect_of(cx);
    W::Header h;
    std::string err;
    if (!W::check(buf, len, true, &e, &h, &err)) return fail(HYDIA_ERR_ARG, err);
    REQUIRE(h.type == W::CT_BATCH || h.type == W::SEEDED_QUERY, "wire message refused: type is a key (hydia_key_from_wire installs keys)");
    REQUIRE(h.count <= (uint64_t)INT32_MAX / 4, "wire message refused: count exceeds what one handle holds");
    const size_t handles = h.type == W::CT_BATCH ? 1 : (size_t)h.count;
    if (out_cap < handles) {
        *n_out = handles;
        return fail(HYDIA_ERR_ARG, "hydia: out_cap is smaller than the handles the message makes (n_out holds their number)");
    }
    const unsigned char *payload = (const unsigned char *)buf + sizeof h;
    const size_t elems = (size_t)cx.nQ * cx.N;
    std::vector<Ct> cts;  // freed again on every refusal below
    Unpacker up(cx, payload, (size_t)h.payload_bytes, (int)h.n_limbs);
    if (h.type == W::CT_BATCH) {
        cts.emplace_back(&cx, (int)h.count, (int)h.n_polys, (int)h.n_limbs, h.scale);
        up.rows(0, h.count, (int)h.n_polys, cts[0].d, cts[0].ct_elems(), cts[0].poly_elems());
    } else {
        cts.reserve(handles);
        for (size_t i = 0; i < handles; i++) {  // exactly the handles hydia_ct_expand_seeded makes
            cts.emplace_back(&cx, 1, 2, cx.nQ, cx.delta);
            up.rows(i, 1, 1, cts[i].d, 2 * elems, elems);
            client_sample_query_a(cx, h.a_seed, h.nonce0 + i, cts[i].d + elems);
        }
    }
    if (!up.canonical()) return fail(HYDIA_ERR_ARG, NOT_CANONICAL);
    for (size_t i = 0; i < handles; i++) out[i] = wrap(ctx, std::move(cts[i]));
    *n_out = handles;
    return HYDIA_OK;
    API_END
}
int hydia_encrypt_queries_seeded_wire(hydia_ctx *ctx, const double *queries, size_t count, const uint8_t seed[32], const uint8_t a_seed[32],
                                      uint64_t nonce0, void *buf, size_t cap, size_t *written) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx, "null argument");
    if (int code = check_public_seed(seed, a_seed, nonce0, count)) return code;
    REQUIRE(count == 0 || queries, "null argument");
    REQUIRE(count <= SIZE_MAX / sizeof(double) / (size_t)ctx->cx.prm.dim, "probe count out of range");
    return queries_to_wire(ctx, count, a_seed, nonce0, buf, cap, written, [&](u64 *payload, const WireRows *R) {
        client_encrypt_queries_seeded(ctx->cx, queries, count, seed, a_seed, nonce0, payload, R);
    });
    API_END
}
int hydia_encrypt_queries_seeded_wire_device(hydia_ctx *ctx, const hydia_dev_rows *rows, const uint8_t seed[32], const uint8_t a_seed[32],
                                             uint64_t nonce0, void *buf, size_t cap, size_t *written) {
    API_BEGIN
    REQUIRE(ctx && rows, "null argument");
    use_device(ctx);
    DevRows r;
    if (int code = hydia_check_dev_rows(ctx, rows, &r)) return code;
    if (int code = check_public_seed(seed, a_seed, nonce0, r.n)) return code;
    return queries_to_wire(ctx, r.n, a_seed, nonce0, buf, cap, written, [&](u64 *payload, const WireRows *R) {
        client_encrypt_queries_seeded_device(ctx->cx, r, seed, a_seed, nonce0, payload, R);
    });
    API_END
}
int hydia_key_to_wire(hydia_ctx *ctx, int rot, int seeded, void *buf, size_t cap, size_t *written) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && written, "null argument");
    return key_to_wire(ctx, rot, seeded, (unsigned char *)buf, cap, written);
    API_END
}
int hydia_key_from_wire(hydia_ctx *ctx, const void *buf, size_t len, int *rot_out) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && buf, "null argument");
    const W::Expect e = expect_of(ctx->cx);
    W::Header h;
    std::string err;
    if (!W::check(buf, len, true, &e, &h, &err)) return fail(HYDIA_ERR_ARG, err);
    REQUIRE(h.type >= W::EVAL_KEY, "wire message refused: type is not a key (hydia_ct_from_wire makes ciphertext handles)");
    return key_from_wire(ctx, h, (const unsigned char *)buf + sizeof h, rot_out);
    API_END
}
int hydia_keys_save(hydia_ctx *ctx, const char *path, int seeded) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && path, "null argument");
    Context &cx = ctx->cx;
    if (!cx.d_pk) return fail(HYDIA_ERR_STATE, "hydia: public key not loaded");
    std::vector<int> ids{-1};  // the public key first, then the evaluation keys in ascending key id
    if (cx.relin_key.d) ids.push_back(0);
    for (const auto &kv : cx.rot_keys)
        if (kv.second.d) ids.push_back(kv.first);
    const size_t cap = std::max(eval_key_message_bytes(cx, seeded != 0), public_key_message_bytes(cx, seeded != 0));
    PinnedBuf stage(cap);  // ONE staging buffer: every message is packed on the device, copied here and written out
    FileCloser fc{fopen(path, "wb")};
    if (!fc.f) return fail(HYDIA_ERR_ARG, std::string("hydia: cannot open ") + path + " for writing");
    W::FileHeader fh{};
    std::memcpy(fh.magic, W::FILE_MAGIC, 8);
    fh.version = W::VERSION;
    fh.n_messages = (uint32_t)ids.size();
    if (fwrite(&fh, sizeof fh, 1, fc.f) != 1) return fail(HYDIA_ERR_ARG, "hydia: write failed (header)");
    for (int id : ids) {
        size_t n = 0;
        if (int code = key_to_wire(ctx, id, seeded, (unsigned char *)stage.p, cap, &n)) return code;
        if (fwrite(stage.p, 1, n, fc.f) != n) return fail(HYDIA_ERR_ARG, "hydia: write failed (disk full?)");
    }
    return HYDIA_OK;
    API_END
}
int hydia_keys_load(hydia_ctx *ctx, const char *path) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && path, "null argument");
    Context &cx = ctx->cx;
    FileCloser fc{fopen(path, "rb")};
    if (!fc.f) return fail(HYDIA_ERR_ARG, std::string("hydia: cannot open ") + path);
    W::FileHeader fh;
    unsigned char raw[sizeof fh];
    std::string err;
    const size_t got = fread(raw, 1, sizeof raw, fc.f);
    if (!W::check_file_header(raw, got, &fh, &err)) return fail(HYDIA_ERR_ARG, err);
    const size_t cap = std::max(eval_key_message_bytes(cx, false), public_key_message_bytes(cx, false));
    PinnedBuf stage(cap);
    const W::Expect e = expect_of(cx);
    for (uint32_t i = 0; i < fh.n_messages; i++) {
        const std::string where = "hydia: key-set file refused at message " + std::to_string(i) + ": ";
        unsigned char *m = (unsigned char *)stage.p;
        W::Header h;
        if (fread(m, 1, sizeof h, fc.f) != sizeof h) return fail(HYDIA_ERR_ARG, where + "the file ends inside its header (truncated)");
        if (!W::check(m, sizeof h, false, &e, &h, &err)) return fail(HYDIA_ERR_ARG, where + err);
        if (h.type < W::EVAL_KEY) return fail(HYDIA_ERR_ARG, where + "type is not a key");
        if (h.payload_bytes > cap - sizeof h) return fail(HYDIA_ERR_ARG, where + "payload_bytes exceeds a key of this context");
        if (fread(m + sizeof h, 1, (size_t)h.payload_bytes, fc.f) != (size_t)h.payload_bytes)
            return fail(HYDIA_ERR_ARG, where + "the file ends inside its payload (truncated)");
        if (int code = key_from_wire(ctx, h, m + sizeof h, nullptr)) return fail(code, where + hydia_last_error());
    }
    if (fgetc(fc.f) != EOF) return fail(HYDIA_ERR_ARG, "hydia: key-set file refused: bytes after the last message");
    return HYDIA_OK;
    API_END
}

}  // extern "C"
