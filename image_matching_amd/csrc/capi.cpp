// image_matching_amd/csrc/capi.cpp — the extern "C" boundary of libhydia.so (include/hydia.h).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include <sys/random.h>

#include "capi_internal.h"
#include "select_kernels.h"

using namespace hydia;

static thread_local std::string g_err;
int hydia_fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
#define fail hydia_fail
// the nonce is a 40-bit field of the sampler stream id (client_kernels.h HY_STREAM): a larger value would bleed into the domain byte
#define HYDIA_NONCE_LIMIT (1ull << 40)

Params hydia_to_params(const hydia_params *p) {
    Params r;
    r.logN = (int)p->log_n;
    r.mult_depth = (int)p->mult_depth;
    r.scale_bits = (int)p->scale_bits;
    r.first_bits = (int)p->first_mod_bits;
    r.dnum = (int)p->dnum;
    r.dim = (int)p->vector_dim;
    return r;
}
static void copy_moduli(const HostParams &h, uint64_t *moduli, uint64_t *roots) {
    for (int m = 0; m < h.nT; m++) {
        if (moduli) moduli[m] = h.q[m];
        if (roots) roots[m] = h.psi[m];
    }
}
// HYDIA_OK when `device` is a HIP device of this machine, else the code recorded with its message
static int check_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(HYDIA_ERR_DEVICE, "hydia: no HIP device visible — libhydia has no CPU fallback");
    REQUIRE(device >= 0, "bad device index");
    if (device >= ndev)  // a device this machine does not have (a shard list written for a bigger node): a device error, not a typo
        return fail(HYDIA_ERR_DEVICE, "hydia: device index " + std::to_string(device) + " but only " + std::to_string(ndev) + " HIP device(s) visible");
    return HYDIA_OK;
}
static void fill_info(const HostParams &h, hydia_info *o) {
    o->log_n = h.prm.logN; o->n = h.N; o->slots = h.slots; o->n_q = h.nQ; o->n_p = h.nP; o->dnum = h.prm.dnum;
    o->alpha = h.alpha; o->vector_dim = h.prm.dim; o->delta = h.delta;
}
// ---- what several entry points below do alike, once
template <class H>
static void free_handle(H *h) {
    if (!h) return;
    hydia_ctx *owner = h->owner;
    use_device(owner);  // the buffer goes back to the pool (or the context goes away) under the context's own GPU
    delete h;
    if (owner && owner->refs.fetch_sub(1) == 1) delete owner;
}
// kind and baby count of a resident diagonal database (ciphertexts: kinds 5 / 6, a plain gallery: 7 / 8) in the form of B babies
static void set_diagonal_form(Context &cx, bool plain, int B) {
    cx.db_kind = (plain ? 7 : 5) + (B < cx.prm.dim ? 1 : 0);
    cx.db_babies = B;
}
// the frame of every diagonal enrolment of n vectors: the baby count from the blocks (matvec: hydia_db_enroll_shard_ex), no kind while
// the database is rebuilt, room for it, enrol(B), then the kind and babies it now has
template <class Enrol>
static void enroll_diagonal(hydia_ctx *ctx, size_t n, bool plain, int matvec, Enrol enrol) {
    Context &cx = ctx->cx;
    const size_t G = (n + (size_t)cx.slots - 1) / (size_t)cx.slots;
    const int B = cx.babies_for(G, matvec);
    cx.db_kind = 0;
    cx.db_resize(n, hydia_db_num_cts(ctx, n), B, plain);
    enrol(B);
    set_diagonal_form(cx, plain, B);
}
// a DECLARED form: vector_dim (hoisted) or a power of two >= 2 dividing it — never 0 / 1, which mean "auto" / "hoisted" only in
// hydia_set_matvec's policy and would silently mark an imported hoisted database as pre-rotated
static int check_declared_babies(const Context &cx, int babies) {
    const int dim = cx.prm.dim;
    REQUIRE(babies == dim || (babies >= 2 && babies < dim && (babies & (babies - 1)) == 0 && dim % babies == 0),
            "the declared baby count must be vector_dim or a power of two >= 2 dividing it");
    return HYDIA_OK;
}
// loop B's bounds and the packed layouts (46 / 48 bits of a residue) assume canonical residues: one encoded polynomial [n_q][N] is
// checked before anything is created or written
static int check_canonical(const Context &cx, const uint64_t *data) {
    for (int j = 0; j < cx.nQ; j++)
        for (int c = 0; c < cx.N; c++)
            REQUIRE(data[(size_t)j * cx.N + c] < cx.q[j], "plaintext residue at or above its modulus");
    return HYDIA_OK;
}
// entry t of the resident database from / to host memory through a pooled staging buffer: `polys` polynomials [n_q][N] (a ciphertext
// two, a plaintext of a plain gallery one)
static void db_entry_in(Context &cx, size_t t, const uint64_t *data, int polys) {
    const size_t e = (size_t)polys * cx.nQ * cx.N;
    u64 *tmp = cx.pool.get(e * sizeof(u64));
    cx.sync();
    HIP_CHECK(hipMemcpy(tmp, data, e * sizeof(u64), hipMemcpyHostToDevice));
    cx.db_store(t, tmp, 1);  // (a row-packed database, kind 1, is addressed the same way: its layout is the unpacked ciphertext-major one)
    cx.sync();
    cx.pool.put(tmp);
}
static void db_entry_out(Context &cx, size_t t, uint64_t *data, int polys) {
    const size_t e = (size_t)polys * cx.nQ * cx.N;
    u64 *tmp = cx.pool.get(e * sizeof(u64));
    cx.db_fetch(t, tmp, 1);
    cx.sync();
    HIP_CHECK(hipMemcpy(data, tmp, e * sizeof(u64), hipMemcpyDeviceToHost));
    cx.pool.put(tmp);
}
// what every in-place update checks before any work, in this order: the other kind resident, nothing resident, a null seed (ciphertext
// target only), first_vector past the end, the row count.  HYDIA_OK, or the code recorded with its message
static int check_update(const Context &cx, bool plain, size_t first_vector, size_t n, const uint8_t *seed) {
    if (plain) {
        if (cx.d_db && cx.db_cts && (cx.db_kind == 5 || cx.db_kind == 6))
            return fail(HYDIA_ERR_STATE, "hydia: a ciphertext database (kind 5 / 6) is resident: it is updated in place by hydia_db_update (with a seed)");
        if (!cx.d_db || cx.db_cts == 0 || !cx.db_plain())
            return fail(HYDIA_ERR_STATE, "hydia: no plain gallery resident (an update needs kind 7 or 8: hydia_plain_db_enroll, hydia_plain_db_alloc or hydia_plain_db_load)");
        REQUIRE(first_vector <= cx.db_vectors, "first_vector lies past the end of the gallery (an update leaves no holes)");
    } else {
        if (cx.db_plain()) return fail(HYDIA_ERR_STATE, "hydia: a plain gallery (kind 7 / 8) is resident: it is updated in place by hydia_plain_db_update (no seed: nothing is encrypted)");
        if (!cx.d_db || cx.db_cts == 0 || (cx.db_kind != 5 && cx.db_kind != 6))
            return fail(HYDIA_ERR_STATE, "hydia: no diagonal database resident (an update needs kind 5 or 6: hydia_db_enroll, hydia_db_load or an import)");
        REQUIRE(seed, "null argument");
        REQUIRE(first_vector <= cx.db_vectors, "first_vector lies past the end of the database (an update leaves no holes)");
    }
    // (rows in device memory arrive with n already inside this bound: check_dev_rows, row_stride >= vector_dim)
    REQUIRE(n <= SIZE_MAX / sizeof(double) / (size_t)cx.prm.dim && first_vector + n >= first_vector, "row count out of range");
    return HYDIA_OK;
}
// a batch of queries (H: hydia_ct, or hydia_pt for plain queries) in shared passes over the database, run = the Context's scenario of
// the batch's form: out[q] = the single-query result for queries[q]; on any error every out[q] is NULL.  gallery: a plain gallery's
// batch, refused on a shard of a group
template <class H>
static int batch_call(hydia_ctx *ctx, const H *const *queries, uint32_t n_queries, hydia_ct **out, int what,
                      std::vector<Ct> (Context::*run)(const std::vector<const Ct *> &, int), bool gallery = false) {
    if (out)
        for (uint32_t q = 0; q < n_queries; q++) out[q] = nullptr;
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && queries && out, "null argument");
    REQUIRE(n_queries >= 1, (std::is_same<H, hydia_pt>::value ? "a batch of plain queries needs at least one query" : "a batch of queries needs at least one query"));
    std::vector<const Ct *> qs(n_queries);
    for (uint32_t q = 0; q < n_queries; q++) {
        REQUIRE(queries[q], "null query in the batch");
        qs[q] = &queries[q]->c;
    }
    if (gallery && ctx->in_group) throw StateError("hydia: a plain gallery (kind 7 / 8) is not served on a shard of a group: neither are its batches");
    std::vector<Ct> r = (ctx->cx.*run)(qs, what);
    for (uint32_t q = 0; q < n_queries; q++) out[q] = wrap(ctx, std::move(r[q]));  // compact and owning: no copy, cannot fail
    return HYDIA_OK;
    API_END
}
extern "C" {

const char *hydia_last_error(void) { return g_err.c_str(); }
const char *hydia_version(void) { return "hydia-mi355x 0.1 (gfx950)"; }

/* 32 bytes from the operating system's entropy pool (getrandom(2), /dev/urandom as fall-back): what every role object
 * seeds its encryption randomness from unless the caller supplies a seed of its own */
int hydia_random_seed(uint8_t out[32]) {
    if (!out) return fail(HYDIA_ERR_ARG, "null argument");
    size_t got = 0;
    while (got < 32) {
        ssize_t r = getrandom(out + got, 32 - got, 0);
        if (r <= 0) break;
        got += (size_t)r;
    }
    if (got < 32) {
        FILE *f = fopen("/dev/urandom", "rb");
        if (f) {
            got += fread(out + got, 1, 32 - got, f);
            fclose(f);
        }
    }
    return got == 32 ? HYDIA_OK : fail(HYDIA_ERR_INTERNAL, "hydia: no entropy source (getrandom and /dev/urandom failed)");
}
void hydia_default_params(hydia_params *o) {
    o->log_n = 15;
    o->mult_depth = (uint32_t)hydia_compute_required_depth(5);
    o->scale_bits = 45;
    o->first_mod_bits = 60;
    o->dnum = 3;
    o->vector_dim = 512;
}
/* src/openFHE_wrapper.cpp:6-44 with COMP_DEPTH 10, ALPHA_DEPTH 2 (include/config.h:14,18) */
size_t hydia_compute_required_depth(size_t approach) {
    const size_t COMP_DEPTH = 10, ALPHA_DEPTH = 2;
    switch (approach) {
        case 1: return 1 + 2 + COMP_DEPTH;
        case 2: return 1 + 2 + ALPHA_DEPTH + 3 + COMP_DEPTH;
        case 3: return 1 + 1 + COMP_DEPTH;
        case 4: return 1 + COMP_DEPTH;
        case 5: return 1 + COMP_DEPTH;
        default: return 0;
    }
}
/* src/main.cpp:169-173: HEStd_128_classic picks the smallest ring whose bound holds log2(QP) of the chain the depth implies */
int hydia_params_for_approach(size_t approach, hydia_params *out) {
    API_BEGIN
    REQUIRE(out, "null argument");
    const size_t depth = hydia_compute_required_depth(approach);
    REQUIRE(depth > 0, "approach must be from 1 to 5");
    hydia_params p;
    hydia_default_params(&p);
    p.mult_depth = (uint32_t)depth;
    static const struct { uint32_t log_n; double bits; } bound[] = {{11, 54}, {12, 109}, {13, 218}, {14, 438}, {15, 881}, {16, 1772}};
    for (const auto &b : bound) {
        p.log_n = b.log_n;
        if ((1u << b.log_n) / 2 < p.vector_dim) continue;  // a vector must fit the slots
        const HostParams h(hydia_to_params(&p));
        double bits = 0;
        for (u64 m : h.q) bits += std::log2((double)m);
        if (bits <= b.bits) {
            *out = p;
            return HYDIA_OK;
        }
    }
    return fail(HYDIA_ERR_ARG, "hydia: no ring up to 2^16 holds this modulus chain at 128-bit classic security");
    API_END
}
int hydia_params_describe(const hydia_params *p, hydia_info *info, uint64_t *moduli, uint64_t *roots) {
    API_BEGIN
    REQUIRE(p, "null params");
    HostParams h(hydia_to_params(p));
    if (info) fill_info(h, info);
    copy_moduli(h, moduli, roots);
    return HYDIA_OK;
    API_END
}
int hydia_ctx_create(const hydia_params *p, int device, hydia_ctx **out) {
    API_BEGIN
    REQUIRE(p && out, "null argument");
    if (int code = check_device(device)) return code;
    *out = new hydia_ctx(hydia_to_params(p), device);
    return HYDIA_OK;
    API_END
}
int hydia_ctx_create_custom(const hydia_params *p, const uint64_t *moduli, const uint64_t *roots, uint32_t n_q, uint32_t n_p,
                            int device, hydia_ctx **out) {
    API_BEGIN
    REQUIRE(p && out && moduli, "null argument");
    REQUIRE(n_q >= 2 && n_p >= 1 && n_q + n_p <= HY_MAX_MODS, "bad limb counts");
    if (int code = check_device(device)) return code;
    Params prm = hydia_to_params(p);
    prm.mult_depth = (int)n_q - 1;
    prm.custom_q.assign(moduli, moduli + n_q + n_p);
    if (roots) prm.custom_psi.assign(roots, roots + n_q + n_p);
    prm.custom_nP = (int)n_p;
    *out = new hydia_ctx(prm, device);
    return HYDIA_OK;
    API_END
}
void hydia_ctx_destroy(hydia_ctx *ctx) {
    if (!ctx) return;
    use_device(ctx);
    if (ctx->refs.fetch_sub(1) == 1) delete ctx;  // otherwise the last hydia_ct_free does it
}
int hydia_get_info(const hydia_ctx *ctx, hydia_info *out) {
    REQUIRE(ctx && out, "null argument");
    fill_info(ctx->cx, out);
    return HYDIA_OK;
}
int hydia_get_moduli(const hydia_ctx *ctx, uint64_t *moduli, uint64_t *roots) {
    REQUIRE(ctx, "null ctx");
    copy_moduli(ctx->cx, moduli, roots);
    return HYDIA_OK;
}
int hydia_sync(hydia_ctx *ctx) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx, "null ctx");
    ctx->cx.sync();
    return HYDIA_OK;
    API_END
}
int hydia_memory_stats(hydia_ctx *ctx, uint64_t *live, uint64_t *cached, uint64_t *peak) {
    REQUIRE(ctx, "null ctx");
    if (live) *live = ctx->cx.pool.bytes_live;
    if (cached) *cached = ctx->cx.pool.bytes_cached;
    if (peak) *peak = ctx->cx.pool.peak;
    return HYDIA_OK;
}

// ------------------------------------------------------------------ keys
int hydia_keygen(hydia_ctx *ctx, const uint8_t seed[32]) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && seed, "null argument");
    client_keygen(ctx->cx, seed);
    return HYDIA_OK;
    API_END
}
// the rotation list of a key generation as key ids: each r mod slots in [1, slots), duplicates dropped, in the caller's order
static int rotation_set(const Context &cx, const int32_t *rots, uint32_t n, std::vector<int> &set) {
    const long S = cx.slots;
    for (uint32_t i = 0; i < n; i++) {
        const int r = (int)((((long)rots[i] % S) + S) % S);  // HY_STREAM carries the key id as an unsigned field: never negative
        REQUIRE(r != 0, "a rotation of 0 mod slots has no key");
        if (std::find(set.begin(), set.end(), r) == set.end()) set.push_back(r);
    }
    return HYDIA_OK;
}
int hydia_keygen_rotations(hydia_ctx *ctx, const uint8_t seed[32], const int32_t *rots, uint32_t n) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && seed && (rots || n == 0), "null argument");
    std::vector<int> set;
    if (int code = rotation_set(ctx->cx, rots, n, set)) return code;
    client_keygen_rotations(ctx->cx, seed, set);
    return HYDIA_OK;
    API_END
}
// ---- seeded keys and queries: the uniform halves travel as the 32-byte public seed they are the expansion of
// a_seed == seed would publish the seed of the secret key (and of every error): refused before anything is touched
#define REQUIRE_PUBLIC_SEED(seed, a_seed) REQUIRE(std::memcmp(seed, a_seed, 32) != 0, "a_seed equals seed: the public expansion seed must be independent of the secret one")
int hydia_keygen_seeded(hydia_ctx *ctx, const uint8_t seed[32], const uint8_t a_seed[32]) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && seed && a_seed, "null argument");
    REQUIRE_PUBLIC_SEED(seed, a_seed);
    client_keygen(ctx->cx, seed, a_seed);
    return HYDIA_OK;
    API_END
}
int hydia_keygen_rotations_seeded(hydia_ctx *ctx, const uint8_t seed[32], const uint8_t a_seed[32], const int32_t *rots, uint32_t n) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && seed && a_seed && (rots || n == 0), "null argument");
    REQUIRE_PUBLIC_SEED(seed, a_seed);
    std::vector<int> set;
    if (int code = rotation_set(ctx->cx, rots, n, set)) return code;
    client_keygen_rotations(ctx->cx, seed, set, a_seed);
    return HYDIA_OK;
    API_END
}
int hydia_get_key_seed(const hydia_ctx *ctx, uint8_t out[32]) {
    REQUIRE(ctx && out, "null argument");
    if (!ctx->cx.has_key_seed) return fail(HYDIA_ERR_STATE, "hydia: no seeded key set was generated on this context (hydia_keygen_seeded)");
    std::memcpy(out, ctx->cx.key_seed, 32);
    return HYDIA_OK;
}
size_t hydia_eval_key_seeded_words(const hydia_ctx *ctx) { return ctx ? (size_t)ctx->cx.prm.dnum * ctx->cx.nT * ctx->cx.N : 0; }
int hydia_export_eval_key_seeded(hydia_ctx *ctx, int rot, uint64_t *b_out) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && b_out, "null argument");
    Context &cx = ctx->cx;
    const Context::EvalKey *k = nullptr;
    if (rot == 0) k = &cx.relin_key;
    else if (cx.rot_keys.count(rot)) k = &cx.rot_keys[rot];
    if (!k || !k->d) return fail(HYDIA_ERR_STATE, "hydia: evaluation key not loaded");
    if (!cx.has_key_seed || !k->seeded)
        return fail(HYDIA_ERR_STATE, "hydia: this evaluation key is not covered by the context's key seed (hydia_keygen_seeded makes such keys; export it whole)");
    const size_t half = (size_t)cx.nT * cx.N * sizeof(u64);
    cx.sync();
    HIP_CHECK(hipMemcpy2D(b_out, half, k->d, 2 * half, half, (size_t)cx.prm.dnum, hipMemcpyDeviceToHost));
    return HYDIA_OK;
    API_END
}
int hydia_export_public_key_seeded(hydia_ctx *ctx, uint64_t *b_out) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && b_out, "null argument");
    Context &cx = ctx->cx;
    if (!cx.d_pk) return fail(HYDIA_ERR_STATE, "hydia: public key not loaded");
    if (!cx.has_key_seed || !cx.pk_seeded)
        return fail(HYDIA_ERR_STATE, "hydia: the public key is not covered by the context's key seed (hydia_keygen_seeded makes such a key; export it whole)");
    cx.sync();
    HIP_CHECK(hipMemcpy(b_out, cx.d_pk, (size_t)cx.nQ * cx.N * sizeof(u64), hipMemcpyDeviceToHost));
    return HYDIA_OK;
    API_END
}
int hydia_import_eval_key_seeded(hydia_ctx *ctx, int rot, const uint64_t *b, const uint8_t a_seed[32]) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && b && a_seed && rot >= 0 && rot < ctx->cx.slots, "bad argument");
    client_import_eval_key_seeded(ctx->cx, rot, (const u64 *)b, a_seed);
    return HYDIA_OK;
    API_END
}
int hydia_import_public_key_seeded(hydia_ctx *ctx, const uint64_t *b, const uint8_t a_seed[32]) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && b && a_seed, "null argument");
    client_import_public_key_seeded(ctx->cx, (const u64 *)b, a_seed);
    return HYDIA_OK;
    API_END
}
int hydia_import_eval_key(hydia_ctx *ctx, int rot, const uint64_t *data) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && data && rot >= 0 && rot < ctx->cx.slots, "bad argument");
    ctx->cx.load_eval_key(rot, (const u64 *)data);
    return HYDIA_OK;
    API_END
}
int hydia_export_eval_key(hydia_ctx *ctx, int rot, uint64_t *data) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && data, "null argument");
    Context &cx = ctx->cx;
    const u64 *src = nullptr;
    if (rot == 0) src = cx.relin_key.d;
    else if (cx.rot_keys.count(rot)) src = cx.rot_keys[rot].d;
    if (!src) return fail(HYDIA_ERR_STATE, "hydia: evaluation key not loaded");
    cx.sync();
    HIP_CHECK(hipMemcpy(data, src, (size_t)cx.prm.dnum * 2 * cx.nT * cx.N * sizeof(u64), hipMemcpyDeviceToHost));
    return HYDIA_OK;
    API_END
}
int hydia_fill_eval_keys_random(hydia_ctx *ctx, uint64_t seed) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx, "null ctx");
    Context &cx = ctx->cx;
    std::vector<int> rots;
    rots.push_back(0);
    for (int i = 1; i < cx.prm.dim; i++) rots.push_back(i);
    for (int i = cx.prm.dim; i < cx.slots; i <<= 1) rots.push_back(i);
    for (int r : rots) {
        u64 *d = cx.eval_key_storage(r);
        // [dnum][2][nT][N]: limb slot index modulo nT selects the modulus
        hk::fill_uniform_hash(cx.stream, cx.d_mod, cx.N, d, (size_t)cx.prm.dnum * 2 * cx.nT, cx.nT, seed + 7919ull * r);
    }
    cx.sync();
    return HYDIA_OK;
    API_END
}
int hydia_has_eval_key(hydia_ctx *ctx, int rot) {
    if (!ctx) return 0;
    if (rot == 0) return ctx->cx.relin_key.d != nullptr;
    auto it = ctx->cx.rot_keys.find(rot);
    return it != ctx->cx.rot_keys.end() && it->second.d != nullptr;
}
static int import_buf(Context &cx, u64 **slot, const uint64_t *data, size_t elems) {
    if (cx.keys_borrowed) throw StateError("hydia: this context borrows its keys from another context (re-key the owner)");
    if (!*slot) HIP_CHECK(hipMalloc((void **)slot, elems * sizeof(u64)));
    HIP_CHECK(hipMemcpy(*slot, data, elems * sizeof(u64), hipMemcpyHostToDevice));
    if (slot == &cx.d_pk) cx.pk_seeded = false;  // an imported public key is whatever the caller sent: no seed covers it
    return HYDIA_OK;
}
int hydia_import_public_key(hydia_ctx *ctx, const uint64_t *data) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && data, "null argument");
    return import_buf(ctx->cx, &ctx->cx.d_pk, data, (size_t)2 * ctx->cx.nQ * ctx->cx.N);
    API_END
}
int hydia_import_secret_key(hydia_ctx *ctx, const uint64_t *data) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && data, "null argument");
    return import_buf(ctx->cx, &ctx->cx.d_sk, data, (size_t)ctx->cx.nT * ctx->cx.N);
    API_END
}
static int export_buf(hydia_ctx *ctx, u64 *Context::*key, size_t polys, uint64_t *data, const char *missing) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && data, "null argument");
    if (!(ctx->cx.*key)) return fail(HYDIA_ERR_STATE, missing);
    ctx->cx.sync();
    HIP_CHECK(hipMemcpy(data, ctx->cx.*key, polys * ctx->cx.N * sizeof(u64), hipMemcpyDeviceToHost));
    return HYDIA_OK;
    API_END
}
int hydia_export_public_key(hydia_ctx *ctx, uint64_t *data) {
    return export_buf(ctx, &Context::d_pk, ctx ? (size_t)2 * ctx->cx.nQ : 0, data, "hydia: public key not loaded");
}
int hydia_export_secret_key(hydia_ctx *ctx, uint64_t *data) {
    return export_buf(ctx, &Context::d_sk, ctx ? (size_t)ctx->cx.nT : 0, data, "hydia: secret key not loaded");
}

// ------------------------------------------------------------------ ciphertext handles
int hydia_ct_import(hydia_ctx *ctx, const uint64_t *data, uint32_t count, uint32_t n_polys, uint32_t n_limbs, double scale,
                    hydia_ct **out) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && data && out, "null argument");
    REQUIRE(count >= 1 && (n_polys == 2 || n_polys == 3) && n_limbs >= 1 && (int)n_limbs <= ctx->cx.nQ, "bad ciphertext shape");
    Ct c(&ctx->cx, (int)count, (int)n_polys, (int)n_limbs, scale);
    ctx->cx.sync();
    HIP_CHECK(hipMemcpy(c.d, data, c.bytes(), hipMemcpyHostToDevice));
    *out = wrap(ctx, std::move(c));
    return HYDIA_OK;
    API_END
}
int hydia_ct_export(hydia_ctx *ctx, const hydia_ct *ct, uint64_t *data) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && ct && data, "null argument");
    REQUIRE(ct->c.compact(), "a limb-prefix view is not exported: copy it with hydia_level_reduce first");
    ctx->cx.sync();
    HIP_CHECK(hipMemcpy(data, ct->c.d, ct->c.bytes(), hipMemcpyDeviceToHost));
    return HYDIA_OK;
    API_END
}
int hydia_ct_shape(const hydia_ct *ct, uint32_t *count, uint32_t *n_polys, uint32_t *n_limbs, double *scale) {
    REQUIRE(ct, "null ct");
    if (count) *count = ct->c.X;
    if (n_polys) *n_polys = ct->c.npoly;
    if (n_limbs) *n_limbs = ct->c.nl;
    if (scale) *scale = ct->c.scale;
    return HYDIA_OK;
}
int hydia_ct_device_ptr(const hydia_ct *ct, void **ptr, size_t *bytes) {
    REQUIRE(ct && ptr, "null argument");
    *ptr = ct->c.d;
    if (bytes) *bytes = ct->c.bytes();
    return HYDIA_OK;
}
int hydia_ct_copy_to_device(hydia_ctx *ctx, const hydia_ct *ct, void *dev_dst) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && ct && dev_dst, "null argument");
    REQUIRE(ct->c.compact(), "a limb-prefix view is not copied out: copy it with hydia_level_reduce first");
    HIP_CHECK(hipMemcpyAsync(dev_dst, ct->c.d, ct->c.bytes(), hipMemcpyDeviceToDevice, ctx->cx.stream));
    ctx->cx.sync();
    return HYDIA_OK;
    API_END
}
int hydia_ct_from_device(hydia_ctx *ctx, const void *dev_ptr, uint32_t count, uint32_t n_polys, uint32_t n_limbs,
                         double scale, hydia_ct **out) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && dev_ptr && out, "null argument");
    REQUIRE(count >= 1 && (n_polys == 2 || n_polys == 3) && n_limbs >= 1 && (int)n_limbs <= ctx->cx.nQ, "bad ciphertext shape");
    Ct c(&ctx->cx, (int)count, (int)n_polys, (int)n_limbs, scale);
    HIP_CHECK(hipMemcpyAsync(c.d, dev_ptr, c.bytes(), hipMemcpyDeviceToDevice, ctx->cx.stream));
    ctx->cx.sync();  // the caller's buffer is free again, and later work on the context's stream is ordered behind the copy
    *out = wrap(ctx, std::move(c));
    return HYDIA_OK;
    API_END
}
// a handle over ciphertexts that stay in the CALLER's device memory (no copy): e.g. the all-gathered rotations of a rotation-split
// loop A.  The memory must stay valid and unchanged while the handle or any operation enqueued on it is alive.
int hydia_ct_view_device(hydia_ctx *ctx, void *dev_ptr, uint32_t count, uint32_t n_polys, uint32_t n_limbs, double scale, hydia_ct **out) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && dev_ptr && out, "null argument");
    REQUIRE(count >= 1 && (n_polys == 2 || n_polys == 3) && n_limbs >= 1 && (int)n_limbs <= ctx->cx.nQ, "bad ciphertext shape");
    hydia_ct *h = new hydia_ct;
    h->c.ctx = &ctx->cx;
    h->c.d = static_cast<u64 *>(dev_ptr);
    h->c.X = (int)count;
    h->c.npoly = (int)n_polys;
    h->c.nl = h->c.lstride = (int)n_limbs;
    h->c.scale = scale;
    h->c.view = true;
    h->owner = ctx;
    ctx->refs.fetch_add(1);
    *out = h;
    return HYDIA_OK;
    API_END
}
// a handle over the first n_limbs limbs of ct, read where they lie (no copy; the limb stride stays ct's): what a level drop without
// rescaling leaves, and how the tests hand limb-strided operands to kernels that take a stride.  ct must outlive the handle
int hydia_ct_limb_prefix(hydia_ctx *ctx, const hydia_ct *ct, uint32_t n_limbs, hydia_ct **out) {
    API_BEGIN
    REQUIRE(ctx && ct && out, "null argument");
    REQUIRE(n_limbs >= 1 && (int)n_limbs <= ct->c.nl, "limb count outside 1 .. the ciphertext's");
    hydia_ct *h = new hydia_ct;
    h->c = ct->c.alias((int)n_limbs);
    h->owner = ctx;
    ctx->refs.fetch_add(1);
    *out = h;
    return HYDIA_OK;
    API_END
}
void hydia_ct_free(hydia_ct *ct) { free_handle(ct); }

// ------------------------------------------------------------------ receiver
int hydia_encrypt_query(hydia_ctx *ctx, const double *query, const uint8_t seed[32], uint64_t nonce, hydia_ct **out) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && query && seed && out, "null argument");
    REQUIRE(nonce < HYDIA_NONCE_LIMIT, "nonce must be below 2^40");
    *out = wrap(ctx, client_encrypt_query(ctx->cx, query, seed, nonce));
    return HYDIA_OK;
    API_END
}
int hydia_encrypt(hydia_ctx *ctx, const double *slots, uint32_t count, const uint8_t seed[32], uint64_t nonce0,
                  hydia_ct **out) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && slots && seed && out && count >= 1, "bad argument");
    REQUIRE(nonce0 < HYDIA_NONCE_LIMIT && nonce0 + count <= HYDIA_NONCE_LIMIT, "nonce must be below 2^40");
    *out = wrap(ctx, client_encrypt(ctx->cx, slots, (int)count, seed, nonce0));
    return HYDIA_OK;
    API_END
}
int hydia_decrypt(hydia_ctx *ctx, const hydia_ct *ct, double *out) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && ct && out, "null argument");
    client_decrypt(ctx->cx, ct->c, out);
    return HYDIA_OK;
    API_END
}
/* receiver_hers.cpp:26-35 */
int hydia_decrypt_membership(hydia_ctx *ctx, const hydia_ct *ct, int *result) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && ct && result, "null argument");
    *result = client_decrypt_slot0(ctx->cx, ct->c) >= 1.0 ? 1 : 0;
    return HYDIA_OK;
    API_END
}
/* receiver_hers.cpp:37-54: hydia_decrypt_matches at threshold 1.0 over all slots, without values */
int hydia_decrypt_index(hydia_ctx *ctx, const hydia_ct *cts, size_t *out, size_t cap, size_t *n_out) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && cts && n_out, "null argument");
    const Ct *one = &cts->c;
    client_select(ctx->cx, SelectSource{&one, nullptr, 1, 0}, 1.0, out, nullptr, cap, n_out);
    return HYDIA_OK;
    API_END
}

// ------------------------------------------------------------------ candidate lists and matches
// n doubles at p in the memory of the context's GPU (the checks of check_dev_rows): HYDIA_OK, or the code recorded with its message
static int check_dev_doubles(hydia_ctx *ctx, const double *p, size_t n) {
    REQUIRE(n >= 1 && n <= HY_SEL_MAX_N, "element count outside 1 .. 2^31 - 1");
    REQUIRE(p, "null device pointer");
    REQUIRE((uintptr_t)p % sizeof(double) == 0, "device pointer is not aligned to a double");
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();  // (an address the runtime has never seen: not an error of the device)
        return fail(HYDIA_ERR_ARG, "hydia: the pointer is not device memory");
    }
    REQUIRE(at.type == hipMemoryTypeDevice, "the pointer is not device memory (managed memory is not supported)");
    REQUIRE(at.device == ctx->cx.device, "the array lies in the memory of another GPU than the context's");
    return HYDIA_OK;
}
// the results of a decrypt entry as a SelectSource: every handle present, n_vectors within every result
static int check_results(hydia_ctx *ctx, const hydia_ct *const *results, uint32_t n_results, size_t n_vectors, std::vector<const Ct *> &cts) {
    REQUIRE(results && n_results >= 1, "bad argument");
    for (uint32_t r = 0; r < n_results; r++) {
        REQUIRE(results[r], "null result");
        const size_t all = (size_t)results[r]->c.X * ctx->cx.slots;
        REQUIRE(all <= HY_SEL_MAX_N, "a result of more than 2^31 - 1 slots");
        REQUIRE(n_vectors <= all, "n_vectors exceeds the slots of a result");
        cts.push_back(&results[r]->c);
    }
    return HYDIA_OK;
}
int hydia_decrypt_device(hydia_ctx *ctx, const hydia_ct *ct, double *dev_out) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && ct, "null argument");
    if (int code = check_dev_doubles(ctx, dev_out, (size_t)ct->c.X * ctx->cx.slots)) return code;
    client_decrypt_device(ctx->cx, ct->c, dev_out);
    return HYDIA_OK;
    API_END
}
int hydia_slots_select_device(hydia_ctx *ctx, const double *dev_vals, size_t n, double threshold, size_t *idx_out, double *val_out, size_t cap,
                              size_t *n_out) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && n_out, "null argument");
    if (int code = check_dev_doubles(ctx, dev_vals, n)) return code;
    client_select(ctx->cx, SelectSource{nullptr, dev_vals, 1, n}, threshold, idx_out, val_out, cap, n_out);
    return HYDIA_OK;
    API_END
}
int hydia_slots_topk_device(hydia_ctx *ctx, const double *dev_vals, size_t n, size_t k, size_t *idx_out, double *val_out, size_t *n_out) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && idx_out && n_out, "null argument");
    REQUIRE(k >= 1, "k must be at least 1");
    if (int code = check_dev_doubles(ctx, dev_vals, n)) return code;
    client_topk(ctx->cx, SelectSource{nullptr, dev_vals, 1, n}, k, idx_out, val_out, n_out);
    return HYDIA_OK;
    API_END
}
int hydia_decrypt_matches_multi(hydia_ctx *ctx, const hydia_ct *const *results, uint32_t n_results, size_t n_vectors, double threshold,
                                size_t *idx_out, double *val_out, size_t cap, size_t *n_out) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && n_out, "null argument");
    std::vector<const Ct *> cts;
    if (int code = check_results(ctx, results, n_results, n_vectors, cts)) return code;
    client_select(ctx->cx, SelectSource{cts.data(), nullptr, n_results, n_vectors}, threshold, idx_out, val_out, cap, n_out);
    return HYDIA_OK;
    API_END
}
int hydia_decrypt_topk_multi(hydia_ctx *ctx, const hydia_ct *const *results, uint32_t n_results, size_t n_vectors, size_t k, size_t *idx_out,
                             double *val_out, size_t *n_out) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && idx_out && n_out, "null argument");
    REQUIRE(k >= 1, "k must be at least 1");
    std::vector<const Ct *> cts;
    if (int code = check_results(ctx, results, n_results, n_vectors, cts)) return code;
    client_topk(ctx->cx, SelectSource{cts.data(), nullptr, n_results, n_vectors}, k, idx_out, val_out, n_out);
    return HYDIA_OK;
    API_END
}
int hydia_decrypt_matches(hydia_ctx *ctx, const hydia_ct *cts, size_t n_vectors, double threshold, size_t *idx_out, double *val_out, size_t cap,
                          size_t *n_out) {
    return hydia_decrypt_matches_multi(ctx, &cts, 1, n_vectors, threshold, idx_out, val_out, cap, n_out);
}
int hydia_decrypt_topk(hydia_ctx *ctx, const hydia_ct *cts, size_t n_vectors, size_t k, size_t *idx_out, double *val_out, size_t *n_out) {
    return hydia_decrypt_topk_multi(ctx, &cts, 1, n_vectors, k, idx_out, val_out, n_out);
}

// ------------------------------------------------------------------ enroller / database
size_t hydia_db_num_cts(const hydia_ctx *ctx, size_t n) {
    if (!ctx) return 0;
    const size_t dim = ctx->cx.prm.dim, per = ctx->cx.slots / dim;
    const size_t nblk = (n + dim - 1) / dim;
    return ((nblk + per - 1) / per) * dim;
}
int hydia_db_alloc(hydia_ctx *ctx, size_t n_vectors) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && n_vectors >= 1, "bad argument");
    ctx->cx.db_resize(n_vectors, hydia_db_num_cts(ctx, n_vectors), ctx->cx.prm.dim);
    set_diagonal_form(ctx->cx, false, ctx->cx.prm.dim);
    return HYDIA_OK;
    API_END
}
int hydia_db_import_ct(hydia_ctx *ctx, size_t t, const uint64_t *data) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && data, "null argument");
    Context &cx = ctx->cx;
    if (!cx.d_db) return fail(HYDIA_ERR_STATE, "hydia: no database resident (call hydia_db_alloc)");
    if (cx.db_plain()) return fail(HYDIA_ERR_STATE, "hydia: a plain gallery (kind 7 / 8) is resident: it holds plaintexts (hydia_plain_db_import_pt), not ciphertexts");
    REQUIRE(t < cx.db_cts, "ciphertext index out of range");
    db_entry_in(cx, t, data, 2);
    if (cx.db_kind == 0) set_diagonal_form(cx, false, cx.prm.dim);
    return HYDIA_OK;
    API_END
}
int hydia_db_export_ct(hydia_ctx *ctx, size_t t, uint64_t *data) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && data, "null argument");
    Context &cx = ctx->cx;
    if (!cx.d_db) return fail(HYDIA_ERR_STATE, "hydia: no database resident");
    if (cx.db_plain()) return fail(HYDIA_ERR_STATE, "hydia: a plain gallery (kind 7 / 8) is resident: it holds plaintexts (hydia_plain_db_export_pt), not ciphertexts");
    REQUIRE(t < cx.db_cts, "ciphertext index out of range");
    db_entry_out(cx, t, data, 2);
    return HYDIA_OK;
    API_END
}
int hydia_db_fill_random(hydia_ctx *ctx, size_t n_vectors, uint64_t seed) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && n_vectors >= 1, "bad argument");
    Context &cx = ctx->cx;
    const size_t cts = hydia_db_num_cts(ctx, n_vectors);
    const int babies = cx.babies_for((n_vectors + (size_t)cx.slots - 1) / (size_t)cx.slots);  // random residues: the cost model of the split auto picks
    cx.db_resize(n_vectors, cts, babies);
    const size_t chunk = (size_t)cx.prm.dim, e = (size_t)2 * cx.nQ * cx.N;
    u64 *tmp = cx.pool.get(chunk * e * sizeof(u64));
    for (size_t t0 = 0; t0 < cts; t0 += chunk) {
        const size_t cnt = std::min(chunk, cts - t0);
        hk::fill_uniform_hash(cx.stream, cx.d_mod, cx.N, tmp, cnt * 2 * cx.nQ, cx.nQ, seed + 0x9E37ull * t0);
        cx.db_store(t0, tmp, (int)cnt);
    }
    cx.sync();
    cx.pool.put(tmp);
    set_diagonal_form(cx, false, babies);
    return HYDIA_OK;
    API_END
}
// matvec: 0 = the context's own policy (hydia_set_matvec; auto looks at the blocks THIS context holds), 1 hoisted, otherwise the baby
// count — a sharded enrolment passes the group-wide decision so that every shard of one database uses the same split
int hydia_db_enroll_shard_ex(hydia_ctx *ctx, double *db, size_t n, const uint8_t seed[32], size_t first_block, int matvec) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && db && seed && n >= 1 && matvec >= 0, "bad argument");
    enroll_diagonal(ctx, n, false, matvec, [&](int B) { client_enroll(ctx->cx, db, n, seed, first_block, B); });
    return HYDIA_OK;
    API_END
}
int hydia_db_enroll(hydia_ctx *ctx, double *db, size_t n, const uint8_t seed[32]) { return hydia_db_enroll_shard_ex(ctx, db, n, seed, 0, 0); }
int hydia_db_enroll_shard(hydia_ctx *ctx, double *db, size_t n, const uint8_t seed[32], size_t first_block) {
    return hydia_db_enroll_shard_ex(ctx, db, n, seed, first_block, 0);
}
int hydia_db_update_shard(hydia_ctx *ctx, size_t first_vector, double *rows, size_t n, int normalise, const uint8_t seed[32], size_t first_block) {
    API_BEGIN
    REQUIRE(ctx, "null argument");
    use_device(ctx);
    Context &cx = ctx->cx;
    if (int code = check_update(cx, false, first_vector, n, seed)) return code;
    if (n == 0) return HYDIA_OK;
    REQUIRE(rows, "null rows");
    client_db_update(cx, first_vector, rows, n, normalise, seed, first_block);
    return HYDIA_OK;
    API_END
}
int hydia_db_update(hydia_ctx *ctx, size_t first_vector, double *rows, size_t n, int normalise, const uint8_t seed[32]) {
    return hydia_db_update_shard(ctx, first_vector, rows, n, normalise, seed, 0);
}
size_t hydia_switch_key_words(const hydia_ctx *ctx) { return ctx ? (size_t)ctx->cx.prm.dnum * 2 * ctx->cx.nT * ctx->cx.N : 0; }
int hydia_keygen_switch(hydia_ctx *ctx, const uint64_t *old_secret, const uint8_t seed[32], uint64_t *key_out) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && old_secret && seed && key_out, "null argument");
    client_keygen_switch(ctx->cx, reinterpret_cast<const u64 *>(old_secret), seed, reinterpret_cast<u64 *>(key_out));
    return HYDIA_OK;
    API_END
}
int hydia_db_rekey_chunked(hydia_ctx *ctx, const uint64_t *switch_key, int max_chunk) {
    API_BEGIN
    REQUIRE(ctx, "null argument");
    use_device(ctx);
    ctx->cx.db_rekey(reinterpret_cast<const u64 *>(switch_key), max_chunk);  // (every refusal — the resident kind, then a null key — before any work is enqueued)
    return HYDIA_OK;
    API_END
}
int hydia_db_rekey(hydia_ctx *ctx, const uint64_t *switch_key) { return hydia_db_rekey_chunked(ctx, switch_key, 0); }
int hydia_set_matvec(hydia_ctx *ctx, int mode) {
    API_BEGIN
    REQUIRE(ctx && mode >= 0, "mat-vec mode is 0 (auto), 1 (hoisted) or a baby count");
    if (mode > 1) (void)ctx->cx.babies_for(1, mode);  // validates: a power of two dividing vector_dim
    ctx->cx.matvec_mode = mode;
    return HYDIA_OK;
    API_END
}
/* form of an IMPORTED database: babies == vector_dim (hoisted: what hydia_db_alloc + hydia_db_import_ct assume, the reference
 * enroller's ciphertexts) or the baby count its diagonals were pre-rotated for */
int hydia_db_set_babies(hydia_ctx *ctx, int babies) {
    API_BEGIN
    REQUIRE(ctx, "null argument");
    Context &cx = ctx->cx;
    if (cx.db_plain()) return fail(HYDIA_ERR_STATE, "hydia: a plain gallery (kind 7 / 8) is resident: its form is declared at allocation (hydia_plain_db_alloc)");
    if (!cx.d_db || cx.db_cts == 0 || (cx.db_kind != 5 && cx.db_kind != 6)) return fail(HYDIA_ERR_STATE, "hydia: no diagonal database resident");
    if (int code = check_declared_babies(cx, babies)) return code;
    use_device(ctx);
    cx.db_relayout(babies);  // no-op unless the resident order was chosen for another form (hydia_db_alloc assumes the hoisted one)
    set_diagonal_form(cx, false, babies);
    return HYDIA_OK;
    API_END
}
int hydia_get_matvec(const hydia_ctx *ctx) { return ctx ? ctx->cx.matvec_mode : -1; }
int hydia_db_kind(const hydia_ctx *ctx) { return ctx ? ctx->cx.db_kind : 0; }
int hydia_db_babies(const hydia_ctx *ctx) { return ctx && ctx->cx.db_kind >= 5 && ctx->cx.db_kind <= 8 ? ctx->cx.db_babies : 0; }
int hydia_auto_babies(const hydia_ctx *ctx, size_t blocks) { return ctx ? ctx->cx.babies_for(blocks) : 0; }
// ------------------------------------------------------------------ plain gallery (database kinds 7 / 8)
// the sender owns the templates: plaintext t is the slot image of hydia_db_enroll's ciphertext t, encoded at scale 2^scale_bits on all
// n_q limbs, evaluation form, ONE polynomial — no seed, no nonce, no public key
int hydia_plain_db_enroll(hydia_ctx *ctx, double *db, size_t n) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && db && n >= 1, "bad argument");
    if (ctx->in_group) return fail(HYDIA_ERR_STATE, "hydia: a plain gallery (kind 7 / 8) is not enrolled on a shard of a group: the sharded senders do not serve it yet");
    enroll_diagonal(ctx, n, true, 0, [&](int B) { client_plain_enroll(ctx->cx, db, n, B); });
    return HYDIA_OK;
    API_END
}
int hydia_plain_db_alloc(hydia_ctx *ctx, size_t n_vectors, int babies) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && n_vectors >= 1, "bad argument");
    if (ctx->in_group) return fail(HYDIA_ERR_STATE, "hydia: a plain gallery (kind 7 / 8) is not enrolled on a shard of a group: the sharded senders do not serve it yet");
    Context &cx = ctx->cx;
    if (int code = check_declared_babies(cx, babies)) return code;
    cx.db_kind = 0;
    cx.db_resize(n_vectors, hydia_db_num_cts(ctx, n_vectors), babies, true);
    HIP_CHECK(hipMemsetAsync(cx.d_db, 0, cx.db_alloc_bytes, cx.stream));  // plaintexts never imported are zero polynomials
    cx.sync();
    set_diagonal_form(cx, true, babies);
    return HYDIA_OK;
    API_END
}
int hydia_plain_db_import_pt(hydia_ctx *ctx, size_t t, const uint64_t *data) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && data, "null argument");
    Context &cx = ctx->cx;
    if (!cx.d_db || !cx.db_plain()) return fail(HYDIA_ERR_STATE, "hydia: no plain gallery resident (call hydia_plain_db_alloc)");
    REQUIRE(t < cx.db_cts, "plaintext index out of range");
    if (int code = check_canonical(cx, data)) return code;
    db_entry_in(cx, t, data, 1);
    return HYDIA_OK;
    API_END
}
int hydia_plain_db_export_pt(hydia_ctx *ctx, size_t t, uint64_t *data) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && data, "null argument");
    Context &cx = ctx->cx;
    if (!cx.d_db || !cx.db_plain()) return fail(HYDIA_ERR_STATE, "hydia: no plain gallery resident");
    REQUIRE(t < cx.db_cts, "plaintext index out of range");
    db_entry_out(cx, t, data, 1);
    return HYDIA_OK;
    API_END
}
int hydia_plain_db_update(hydia_ctx *ctx, size_t first_vector, double *rows, size_t n, int normalise) {
    API_BEGIN
    REQUIRE(ctx, "null argument");
    use_device(ctx);
    Context &cx = ctx->cx;
    if (int code = check_update(cx, true, first_vector, n, nullptr)) return code;
    if (n == 0) return HYDIA_OK;
    REQUIRE(rows, "null rows");
    client_plain_db_update(cx, first_vector, rows, n, normalise);
    return HYDIA_OK;
    API_END
}
int hydia_plain_db_save(hydia_ctx *ctx, const char *path) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && path, "null argument");
    ctx->cx.plain_db_save(path);
    return HYDIA_OK;
    API_END
}
int hydia_plain_db_load(hydia_ctx *ctx, const char *path) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && path, "null argument");
    if (ctx->in_group) return fail(HYDIA_ERR_STATE, "hydia: a plain gallery (kind 7 / 8) is not loaded on a shard of a group: the sharded senders do not serve it yet");
    ctx->cx.plain_db_load(path);
    return HYDIA_OK;
    API_END
}
int hydia_hers_db_enroll(hydia_ctx *ctx, double *db, size_t n, const uint8_t seed[32]) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && db && seed && n >= 1, "bad argument");
    Context &cx = ctx->cx;
    const size_t G = (n + cx.slots - 1) / cx.slots;  // enroller_hers.cpp:59-60
    cx.db_resize(n, G * cx.prm.dim, -1);
    client_hers_enroll(cx, db, n, seed);
    cx.db_kind = 4;
    return HYDIA_OK;
    API_END
}
int hydia_hers_encrypt_query(hydia_ctx *ctx, const double *query, const uint8_t seed[32], uint64_t nonce0, hydia_ct **out) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && query && seed && out, "null argument");
    REQUIRE(nonce0 < HYDIA_NONCE_LIMIT && nonce0 + ctx->cx.prm.dim <= HYDIA_NONCE_LIMIT, "nonce must be below 2^40");
    *out = wrap(ctx, client_hers_encrypt_query(ctx->cx, query, seed, nonce0));
    return HYDIA_OK;
    API_END
}
// ------------------------------------------------------------------ approach 1 (the literature baseline)
size_t hydia_base_db_num_cts(const hydia_ctx *ctx, size_t n) {
    if (!ctx) return 0;
    const int dim = ctx->cx.prm.dim;
    if (dim < 1 || dim > ctx->cx.slots || (dim & (dim - 1))) return 0;
    return ctx->cx.base_db_cts(n);
}
int hydia_base_db_enroll(hydia_ctx *ctx, double *db, size_t n, const uint8_t seed[32]) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && db && seed && n >= 1, "bad argument");
    Context &cx = ctx->cx;
    const int dim = cx.prm.dim;
    REQUIRE(dim >= 1 && dim <= cx.slots && (dim & (dim - 1)) == 0, "row packing needs vector_dim to be a power of two of at most `slots`");
    cx.db_kind = 0;
    cx.db_resize_rows(n, cx.base_db_cts(n));
    client_base_enroll(cx, db, n, seed);
    cx.db_kind = 1;
    cx.db_babies = 0;
    return HYDIA_OK;
    API_END
}
int hydia_base_rotations(uint32_t slots, int32_t *rots, size_t cap, size_t *n_out) {
    REQUIRE(n_out && slots >= 2 && (slots & (slots - 1)) == 0 && slots <= (1u << 30), "slots must be a power of two");
    std::vector<int32_t> v;
    for (uint32_t k = 1; k < slots; k <<= 1) {
        v.push_back((int32_t)k);
        v.push_back((int32_t)(slots - k));
    }
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    for (size_t i = 0; i < v.size() && i < cap && rots; i++) rots[i] = v[i];
    *n_out = v.size();
    return HYDIA_OK;
}
// ------------------------------------------------------------------ approach 2 (GROTE group testing)
uint32_t hydia_grote_row_length(uint32_t slots) {
    if (slots < 2 || (slots & (slots - 1)) || slots > (1u << 30)) return 0;
    return (uint32_t)Context::grote_row_length((long)slots);
}
/* receiver_grote.cpp:12-65 */
int hydia_grote_decrypt_index(hydia_ctx *ctx, const hydia_ct *rows, const hydia_ct *cols, size_t n_vectors, size_t *out, size_t cap, size_t *n_out) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && rows && cols && n_out, "null argument");
    const size_t S = ctx->cx.slots, rl = (size_t)Context::grote_row_length((long)S), cl = S / rl;
    const size_t mats = (n_vectors + S - 1) / S, num_row = (mats + rl - 1) / rl, num_col = (mats + cl - 1) / cl;  // :20-21
    REQUIRE((size_t)rows->c.X == num_row && (size_t)cols->c.X == num_col, "incorrect parsing of index query results: the row / column ciphertext counts do not fit n_vectors");
    std::vector<double> rv(num_row * S), cv(num_col * S);
    client_decrypt(ctx->cx, rows->c, rv.data());
    client_decrypt(ctx->cx, cols->c, cv.data());
    std::vector<size_t> rm, cm;
    for (size_t i = 0; i < rv.size(); i++)
        if (rv[i] >= 1.0) rm.push_back(i);
    for (size_t i = 0; i < cv.size(); i++)
        if (cv[i] >= 1.0) cm.push_back(i);
    size_t cnt = 0;
    for (size_t r : rm)      // :51-62: rows outer, columns inner
        for (size_t c : cm)
            if (r / cl == c / rl) {
                if (out && cnt < cap) out[cnt] = r * rl + c % rl;
                cnt++;
            }
    *n_out = cnt;
    return HYDIA_OK;
    API_END
}
// ------------------------------------------------------------------ approach 3 (the Blind-Match method)
size_t hydia_blind_db_num_cts(const hydia_ctx *ctx, size_t n, size_t chunk_len) {
    if (!ctx || chunk_len > (size_t)INT32_MAX) return 0;
    try {
        (void)ctx->cx.blind_chunks((int)chunk_len);
    } catch (...) {
        return 0;
    }
    return ctx->cx.blind_db_cts(n, (int)chunk_len);
}
int hydia_blind_db_enroll(hydia_ctx *ctx, double *db, size_t n, size_t chunk_len, const uint8_t seed[32]) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && db && seed && n >= 1, "bad argument");
    REQUIRE(chunk_len <= (size_t)INT32_MAX, "chunk_len must be a power of two in 2 .. slots that divides vector_dim");
    Context &cx = ctx->cx;
    (void)cx.blind_chunks((int)chunk_len);  // validates before the resident database is touched
    cx.db_kind = 0;
    cx.db_resize_rows(n, cx.blind_db_cts(n, (int)chunk_len));
    client_blind_enroll(cx, db, n, (int)chunk_len, seed);
    cx.db_kind = 3;
    cx.db_babies = 0;
    cx.db_chunk_len = (int)chunk_len;
    return HYDIA_OK;
    API_END
}
int hydia_blind_encrypt_query(hydia_ctx *ctx, const double *query, size_t chunk_len, const uint8_t seed[32], uint64_t nonce0, hydia_ct **out) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && query && seed && out, "null argument");
    REQUIRE(chunk_len <= (size_t)INT32_MAX, "chunk_len must be a power of two in 2 .. slots that divides vector_dim");
    const int K = ctx->cx.blind_chunks((int)chunk_len);
    REQUIRE(nonce0 < HYDIA_NONCE_LIMIT && nonce0 + (uint64_t)K <= HYDIA_NONCE_LIMIT, "nonce must be below 2^40");
    *out = wrap(ctx, client_blind_encrypt_query(ctx->cx, query, (int)chunk_len, seed, nonce0));
    return HYDIA_OK;
    API_END
}
/* receiver_blind.cpp:28-54 */
int hydia_blind_decrypt_index(hydia_ctx *ctx, const hydia_ct *cts, size_t chunk_len, size_t *out, size_t cap, size_t *n_out) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && cts && n_out, "null argument");
    const size_t S = ctx->cx.slots;
    REQUIRE(chunk_len >= 1 && chunk_len <= S && (chunk_len & (chunk_len - 1)) == 0, "chunk_len must be a power of two of at most `slots`");
    const size_t spb = S / chunk_len;  // scoresPerBatch
    std::vector<double> v((size_t)cts->c.X * S);
    client_decrypt(ctx->cx, cts->c, v.data());
    size_t cnt = 0;
    for (size_t i = 0; i < (size_t)cts->c.X; i++)
        for (size_t j = 0; j < S; j++)
            if (v[i * S + j] >= 1.0) {  // indices of the padding past n_vectors are NOT filtered: the reference does not either
                if (out && cnt < cap) out[cnt] = i * S + j / chunk_len + (j % chunk_len) * spb;
                cnt++;
            }
    *n_out = cnt;
    return HYDIA_OK;
    API_END
}
int hydia_db_save(hydia_ctx *ctx, const char *path) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && path, "null argument");
    ctx->cx.db_save(path);
    return HYDIA_OK;
    API_END
}
int hydia_db_load(hydia_ctx *ctx, const char *path) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && path, "null argument");
    ctx->cx.db_load(path);
    return HYDIA_OK;
    API_END
}
int hydia_db_stats(const hydia_ctx *ctx, size_t *n_vectors, size_t *n_cts, size_t *bytes) {
    REQUIRE(ctx, "null ctx");
    if (n_vectors) *n_vectors = ctx->cx.db_vectors;
    if (n_cts) *n_cts = ctx->cx.db_cts;
    if (bytes) *bytes = ctx->cx.db_cts * ctx->cx.db_layout().ct_bytes;
    return HYDIA_OK;
}
int hydia_db_group(const hydia_ctx *ctx) { return ctx && ctx->cx.d_db ? ctx->cx.db_lay.seq : 0; }
int hydia_db_residue_bits(const hydia_ctx *ctx) {
    if (!ctx || !ctx->cx.d_db) return 0;
    const DbLayout &L = ctx->cx.db_lay;
    return !L.packed ? 64 : (L.seq && L.bits46) ? 46 : 48;
}

// ------------------------------------------------------------------ sender
#define SENDER_CALL(expr)                                 \
    API_BEGIN                                             \
    use_device(ctx);                                      \
    REQUIRE(ctx && query && out, "null argument");        \
    *out = wrap(ctx, expr);                                  \
    return HYDIA_OK;                                      \
    API_END
int hydia_rotate_query(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out) { SENDER_CALL(ctx->cx.rotate_query(query->c)) }
int hydia_compute_similarity(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out) { SENDER_CALL(ctx->cx.similarity(query->c)) }
int hydia_rotate_query_range_into(hydia_ctx *ctx, const hydia_ct *query, uint32_t first, uint32_t count, void *dev_dst) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && query && dev_dst, "null argument");
    if (ctx->cx.db_plain()) return fail(HYDIA_ERR_STATE, "hydia: a plain gallery (kind 7 / 8) is resident: split rotations are not served on it yet");
    REQUIRE(first <= (uint32_t)ctx->cx.prm.dim && count <= (uint32_t)ctx->cx.prm.dim - first, "rotation range outside 0 .. vector_dim");
    ctx->cx.rotate_query_range(query->c, (int)first, (int)count, static_cast<u64 *>(dev_dst));
    return HYDIA_OK;
    API_END
}
int hydia_rotate_query_range(hydia_ctx *ctx, const hydia_ct *query, uint32_t first, uint32_t count, hydia_ct **out) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && query && out && count >= 1, "bad argument");
    if (ctx->cx.db_plain()) return fail(HYDIA_ERR_STATE, "hydia: a plain gallery (kind 7 / 8) is resident: split rotations are not served on it yet");
    // validated on the unsigned values BEFORE anything is allocated (first + count must not wrap)
    REQUIRE(first <= (uint32_t)ctx->cx.prm.dim && count <= (uint32_t)ctx->cx.prm.dim - first, "rotation range outside 0 .. vector_dim");
    Ct r(&ctx->cx, (int)count, 2, query->c.nl, query->c.scale);
    ctx->cx.rotate_query_range(query->c, (int)first, (int)count, r.d);
    *out = wrap(ctx, std::move(r));
    return HYDIA_OK;
    API_END
}
int hydia_compute_similarity_rotated(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out) { SENDER_CALL(ctx->cx.similarity_rot(query->c)) }
int hydia_index_scenario_rotated(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out) { SENDER_CALL(ctx->cx.index_scenario_rot(query->c)) }
int hydia_index_scenario(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out) { SENDER_CALL(ctx->cx.index_scenario(query->c)) }
int hydia_membership_scenario(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out) { SENDER_CALL(ctx->cx.membership_scenario(query->c)) }
// ------------------------------------------------------------------ plain query (the sender knows the probe; kinds 5 / 6 only)
int hydia_encode_query(hydia_ctx *ctx, const double *query, hydia_pt **out) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && query && out, "null argument");
    *out = wrap<hydia_pt>(ctx, client_encode_query(ctx->cx, query));
    return HYDIA_OK;
    API_END
}
int hydia_pt_import(hydia_ctx *ctx, const uint64_t *data, double scale, hydia_pt **out) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && data && out, "null argument");
    Context &cx = ctx->cx;
    if (int code = check_canonical(cx, data)) return code;
    Ct c(&cx, 1, 1, cx.nQ, scale);
    cx.sync();
    HIP_CHECK(hipMemcpy(c.d, data, c.bytes(), hipMemcpyHostToDevice));
    *out = wrap<hydia_pt>(ctx, std::move(c));
    return HYDIA_OK;
    API_END
}
int hydia_pt_export(hydia_ctx *ctx, const hydia_pt *pt, uint64_t *data) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && pt && data, "null argument");
    ctx->cx.sync();
    HIP_CHECK(hipMemcpy(data, pt->c.d, pt->c.bytes(), hipMemcpyDeviceToHost));
    return HYDIA_OK;
    API_END
}
void hydia_pt_free(hydia_pt *pt) { free_handle(pt); }
// ------------------------------------------------------------------ templates already in device memory (hydia_dev_rows)
// every check of a descriptor, before anything is launched: HYDIA_OK, or the code recorded with its message.  A context that is a shard
// of a group is refused (the group enrols and serves its shards' databases), then the descriptor itself is looked at
static int check_dev_rows(hydia_ctx *ctx, const hydia_dev_rows *rows, DevRows &out) {
    if (ctx->in_group) return fail(HYDIA_ERR_STATE, "hydia: rows in device memory are not taken on a shard of a group: the group enrols and serves its shards");
    REQUIRE((int)rows->dtype >= (int)HYDIA_F64 && (int)rows->dtype <= (int)HYDIA_BF16, "element type outside HYDIA_F64 / HYDIA_F32 / HYDIA_F16 / HYDIA_BF16");
    const size_t dim = (size_t)ctx->cx.prm.dim, esz = rows->dtype == HYDIA_F64 ? 8 : rows->dtype == HYDIA_F32 ? 4 : 2;
    REQUIRE(rows->row_stride >= dim, "row_stride is smaller than vector_dim");
    REQUIRE(rows->n <= SIZE_MAX / 8 / rows->row_stride, "row count out of range");
    out = DevRows{rows->ptr, (int)rows->dtype, rows->n, rows->row_stride, (hipStream_t)rows->stream};
    if (rows->n == 0) return HYDIA_OK;
    REQUIRE(rows->ptr, "null rows");
    REQUIRE((uintptr_t)rows->ptr % esz == 0, "rows pointer is not aligned to its element type");
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, rows->ptr) != hipSuccess) {
        (void)hipGetLastError();  // (an address the runtime has never seen: not an error of the device)
        return fail(HYDIA_ERR_ARG, "hydia: rows pointer is not device memory (host rows go to the host entry point)");
    }
    REQUIRE(at.type == hipMemoryTypeDevice, "rows pointer is not device memory (host rows go to the host entry point)");
    REQUIRE(at.device == ctx->cx.device, "rows lie in the memory of another GPU than the context's");
    return HYDIA_OK;
}
// (the same checks for wire.cpp's hydia_encrypt_queries_seeded_wire_device; internal, not declared in include/hydia.h)
int hydia_check_dev_rows(hydia_ctx *ctx, const hydia_dev_rows *rows, DevRows *out) { return check_dev_rows(ctx, rows, *out); }
#define CHECK_DEV_ROWS(r)                              \
    REQUIRE(ctx && rows, "null argument");             \
    use_device(ctx);                                   \
    DevRows r;                                         \
    if (int code_ = check_dev_rows(ctx, rows, r)) return code_;

int hydia_rows_widen_device(hydia_ctx *ctx, const hydia_dev_rows *rows, int normalise, double *dev_dst) {
    API_BEGIN
    CHECK_DEV_ROWS(r)
    if (r.n == 0) return HYDIA_OK;
    REQUIRE(dev_dst, "null argument");
    client_rows_widen(ctx->cx, r, normalise, dev_dst);
    return HYDIA_OK;
    API_END
}
int hydia_db_enroll_device(hydia_ctx *ctx, const hydia_dev_rows *rows, const uint8_t seed[32]) {
    API_BEGIN
    CHECK_DEV_ROWS(r)
    REQUIRE(seed && r.n >= 1, "bad argument");
    Context &cx = ctx->cx;
    if (!cx.d_pk) return fail(HYDIA_ERR_STATE, "hydia: public key not loaded");
    enroll_diagonal(ctx, r.n, false, 0, [&](int B) { client_enroll_device(cx, r, seed, 0, B); });
    return HYDIA_OK;
    API_END
}
int hydia_plain_db_enroll_device(hydia_ctx *ctx, const hydia_dev_rows *rows) {
    API_BEGIN
    CHECK_DEV_ROWS(r)
    REQUIRE(r.n >= 1, "bad argument");
    enroll_diagonal(ctx, r.n, true, 0, [&](int B) { client_plain_enroll_device(ctx->cx, r, B); });
    return HYDIA_OK;
    API_END
}
int hydia_db_update_device(hydia_ctx *ctx, size_t first_vector, const hydia_dev_rows *rows, int normalise, const uint8_t seed[32]) {
    API_BEGIN
    CHECK_DEV_ROWS(r)
    Context &cx = ctx->cx;
    if (int code = check_update(cx, false, first_vector, r.n, seed)) return code;
    if (r.n == 0) return HYDIA_OK;
    if (!cx.d_pk) return fail(HYDIA_ERR_STATE, "hydia: public key not loaded");
    client_db_update_device(cx, first_vector, r, normalise, seed, 0);
    return HYDIA_OK;
    API_END
}
int hydia_plain_db_update_device(hydia_ctx *ctx, size_t first_vector, const hydia_dev_rows *rows, int normalise) {
    API_BEGIN
    CHECK_DEV_ROWS(r)
    Context &cx = ctx->cx;
    if (int code = check_update(cx, true, first_vector, r.n, nullptr)) return code;
    if (r.n == 0) return HYDIA_OK;
    client_plain_db_update_device(cx, first_vector, r, normalise);
    return HYDIA_OK;
    API_END
}
int hydia_encrypt_queries_device(hydia_ctx *ctx, const hydia_dev_rows *rows, const uint8_t seed[32], uint64_t nonce0, hydia_ct **out) {
    if (out && rows)
        for (size_t q = 0; q < rows->n; q++) out[q] = nullptr;
    API_BEGIN
    CHECK_DEV_ROWS(r)
    REQUIRE(seed && out, "null argument");
    REQUIRE(r.n >= 1, "a batch of probes needs at least one row");
    REQUIRE(nonce0 < HYDIA_NONCE_LIMIT && r.n <= HYDIA_NONCE_LIMIT - nonce0, "nonce must be below 2^40");
    if (!ctx->cx.d_pk) return fail(HYDIA_ERR_STATE, "hydia: public key not loaded");
    std::vector<Ct> cts = client_encrypt_queries_device(ctx->cx, r, seed, nonce0);
    for (size_t q = 0; q < r.n; q++) out[q] = wrap(ctx, std::move(cts[q]));  // compact and owning: no copy, cannot fail
    return HYDIA_OK;
    API_END
}
// ---- seeded secret-key queries: the receiver sends c0 and (a_seed, nonce0); the sender expands c1
// what the three encrypting entries check alike before any work: the seeds and the nonce range (probe i takes nonce0 + i)
static int check_seeded(const uint8_t *seed, const uint8_t *a_seed, uint64_t nonce0, size_t count) {
    REQUIRE(seed && a_seed, "null argument");
    REQUIRE_PUBLIC_SEED(seed, a_seed);
    REQUIRE(nonce0 <= HYDIA_NONCE_LIMIT && count <= HYDIA_NONCE_LIMIT - nonce0, "nonce0 + count must not exceed 2^40");
    return HYDIA_OK;
}
int hydia_encrypt_queries_seeded(hydia_ctx *ctx, const double *queries, size_t count, const uint8_t seed[32], const uint8_t a_seed[32],
                                 uint64_t nonce0, uint64_t *c0_out) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx, "null argument");
    if (int code = check_seeded(seed, a_seed, nonce0, count)) return code;
    if (count == 0) return HYDIA_OK;
    REQUIRE(queries && c0_out, "null argument");
    REQUIRE(count <= SIZE_MAX / sizeof(double) / (size_t)ctx->cx.prm.dim, "probe count out of range");
    client_encrypt_queries_seeded(ctx->cx, queries, count, seed, a_seed, nonce0, (u64 *)c0_out);
    return HYDIA_OK;
    API_END
}
int hydia_encrypt_query_seeded(hydia_ctx *ctx, const double *query, const uint8_t seed[32], const uint8_t a_seed[32], uint64_t nonce,
                               uint64_t *c0_out) {
    return hydia_encrypt_queries_seeded(ctx, query, 1, seed, a_seed, nonce, c0_out);
}
int hydia_encrypt_queries_seeded_device(hydia_ctx *ctx, const hydia_dev_rows *rows, const uint8_t seed[32], const uint8_t a_seed[32],
                                        uint64_t nonce0, uint64_t *c0_out) {
    API_BEGIN
    CHECK_DEV_ROWS(r)
    if (int code = check_seeded(seed, a_seed, nonce0, r.n)) return code;
    if (r.n == 0) return HYDIA_OK;
    REQUIRE(c0_out, "null argument");
    client_encrypt_queries_seeded_device(ctx->cx, r, seed, a_seed, nonce0, (u64 *)c0_out);
    return HYDIA_OK;
    API_END
}
int hydia_ct_expand_seeded(hydia_ctx *ctx, const uint64_t *c0, size_t count, const uint8_t a_seed[32], uint64_t nonce0, hydia_ct **out) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && a_seed, "null argument");
    REQUIRE(nonce0 <= HYDIA_NONCE_LIMIT && count <= HYDIA_NONCE_LIMIT - nonce0, "nonce0 + count must not exceed 2^40");
    if (count == 0) return HYDIA_OK;
    REQUIRE(c0 && out, "null argument");
    for (size_t q = 0; q < count; q++) out[q] = nullptr;  // (what a device error below leaves behind)
    std::vector<Ct> cts = client_expand_seeded(ctx->cx, (const u64 *)c0, count, a_seed, nonce0);
    for (size_t q = 0; q < count; q++) out[q] = wrap(ctx, std::move(cts[q]));  // compact and owning: no copy, cannot fail
    return HYDIA_OK;
    API_END
}
int hydia_encode_queries_device(hydia_ctx *ctx, const hydia_dev_rows *rows, hydia_pt **out) {
    if (out && rows)
        for (size_t q = 0; q < rows->n; q++) out[q] = nullptr;
    API_BEGIN
    CHECK_DEV_ROWS(r)
    REQUIRE(out, "null argument");
    REQUIRE(r.n >= 1, "a batch of probes needs at least one row");
    std::vector<Ct> pts = client_encode_queries_device(ctx->cx, r);
    for (size_t q = 0; q < r.n; q++) out[q] = wrap<hydia_pt>(ctx, std::move(pts[q]));
    return HYDIA_OK;
    API_END
}
int hydia_compute_similarity_pq(hydia_ctx *ctx, const hydia_pt *query, hydia_ct **out) { SENDER_CALL(ctx->cx.similarity_pq(query->c)) }
int hydia_index_scenario_pq(hydia_ctx *ctx, const hydia_pt *query, hydia_ct **out) { SENDER_CALL(ctx->cx.index_scenario_pq(query->c)) }
int hydia_membership_scenario_pq(hydia_ctx *ctx, const hydia_pt *query, hydia_ct **out) { SENDER_CALL(ctx->cx.membership_scenario_pq(query->c)) }

int hydia_compute_similarity_multi(hydia_ctx *ctx, const hydia_ct *const *queries, uint32_t n_queries, hydia_ct **out) {
    return batch_call(ctx, queries, n_queries, out, 0, &Context::scenario_multi);
}
int hydia_index_scenario_multi(hydia_ctx *ctx, const hydia_ct *const *queries, uint32_t n_queries, hydia_ct **out) {
    return batch_call(ctx, queries, n_queries, out, 1, &Context::scenario_multi);
}
int hydia_membership_scenario_multi(hydia_ctx *ctx, const hydia_ct *const *queries, uint32_t n_queries, hydia_ct **out) {
    return batch_call(ctx, queries, n_queries, out, 2, &Context::scenario_multi);
}
int hydia_compute_similarity_pq_multi(hydia_ctx *ctx, const hydia_pt *const *queries, uint32_t n_queries, hydia_ct **out) {
    return batch_call(ctx, queries, n_queries, out, 0, &Context::scenario_pq_multi);
}
int hydia_index_scenario_pq_multi(hydia_ctx *ctx, const hydia_pt *const *queries, uint32_t n_queries, hydia_ct **out) {
    return batch_call(ctx, queries, n_queries, out, 1, &Context::scenario_pq_multi);
}
int hydia_membership_scenario_pq_multi(hydia_ctx *ctx, const hydia_pt *const *queries, uint32_t n_queries, hydia_ct **out) {
    return batch_call(ctx, queries, n_queries, out, 2, &Context::scenario_pq_multi);
}
int hydia_set_pq_batch_width(hydia_ctx *ctx, uint32_t width) {
    API_BEGIN
    REQUIRE(ctx, "null argument");
    REQUIRE(width == 0 || width == 1 || width == 2 || width == 4, "a plain-query batch serves 1, 2 or 4 queries per pass (0 = the default)");
    ctx->cx.pq_mq_width = (int)width;
    return HYDIA_OK;
    API_END
}
// a batch of encrypted queries against a plain gallery (kinds 7 / 8)
int hydia_compute_similarity_gallery_multi(hydia_ctx *ctx, const hydia_ct *const *queries, uint32_t n_queries, hydia_ct **out) {
    return batch_call(ctx, queries, n_queries, out, 0, &Context::scenario_gallery_multi, true);
}
int hydia_index_scenario_gallery_multi(hydia_ctx *ctx, const hydia_ct *const *queries, uint32_t n_queries, hydia_ct **out) {
    return batch_call(ctx, queries, n_queries, out, 1, &Context::scenario_gallery_multi, true);
}
int hydia_membership_scenario_gallery_multi(hydia_ctx *ctx, const hydia_ct *const *queries, uint32_t n_queries, hydia_ct **out) {
    return batch_call(ctx, queries, n_queries, out, 2, &Context::scenario_gallery_multi, true);
}
int hydia_set_gallery_batch_width(hydia_ctx *ctx, uint32_t width) {
    API_BEGIN
    REQUIRE(ctx, "null argument");
    REQUIRE(width == 0 || width == 1 || width == 2 || width == 4, "a plain gallery's batch serves 1, 2 or 4 queries per pass (0 = the default)");
    ctx->cx.plain_mq_width = (int)width;
    return HYDIA_OK;
    API_END
}
int hydia_chebyshev_compare(hydia_ctx *ctx, const hydia_ct *query, double delta, size_t sign_depth, hydia_ct **out) {
    SENDER_CALL(ctx->cx.chebyshev_compare(query->c, delta, (int)sign_depth))
}
int hydia_sum_and_evalsum(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out) { SENDER_CALL(ctx->cx.sum_and_evalsum(query->c)) }
int hydia_add_many(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out) { SENDER_CALL(ctx->cx.add_many(query->c)) }
int hydia_eval_sum(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out) { SENDER_CALL(ctx->cx.eval_sum(query->c)) }
int hydia_ct_add_raw(hydia_ctx *ctx, hydia_ct *acc, const void *dev_src, int src_device) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && acc && dev_src, "null argument");
    Context &cx = ctx->cx;
    // the source is compact: its size follows the accumulator's limb COUNT (bytes() follows the limb stride, which a limb-prefix view
    // keeps from its parent and which would read past the end of the source)
    const size_t bytes = (size_t)acc->c.X * acc->c.npoly * acc->c.nl * cx.N * sizeof(u64);
    u64 *tmp = cx.pool.get(bytes);
    // on the context's own stream: a plain device-to-device hipMemcpy would run on the null stream, unordered with it
    if (src_device < 0 || src_device == cx.device)
        HIP_CHECK(hipMemcpyAsync(tmp, dev_src, bytes, hipMemcpyDeviceToDevice, cx.stream));
    else
        HIP_CHECK(hipMemcpyPeerAsync(tmp, cx.device, dev_src, src_device, bytes, cx.stream));
    cx.add_raw_inplace(acc->c, tmp);
    cx.sync();
    cx.pool.put(tmp);
    return HYDIA_OK;
    API_END
}
int hydia_ct_mod_reduce(hydia_ctx *ctx, hydia_ct *ct) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && ct, "null argument");
    ctx->cx.mod_reduce_inplace(ct->c);
    return HYDIA_OK;
    API_END
}
int hydia_hers_compute_similarity(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out) { SENDER_CALL(ctx->cx.hers_similarity(query->c)) }
int hydia_hers_index_scenario(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out) { SENDER_CALL(ctx->cx.hers_index_scenario(query->c)) }
int hydia_hers_membership_scenario(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out) { SENDER_CALL(ctx->cx.hers_membership_scenario(query->c)) }
int hydia_base_compute_similarity(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out) { SENDER_CALL(ctx->cx.base_similarity(query->c)) }
int hydia_base_index_scenario(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out) { SENDER_CALL(ctx->cx.base_index_scenario(query->c)) }
int hydia_base_membership_scenario(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out) { SENDER_CALL(ctx->cx.base_membership_scenario(query->c)) }
int hydia_merge_ciphers(hydia_ctx *ctx, const hydia_ct *query, size_t dimension, hydia_ct **out) {
    if (dimension > (size_t)INT32_MAX) return fail(HYDIA_ERR_ARG, "hydia: the merge dimension must be a power of two in 2 .. slots");
    SENDER_CALL(ctx->cx.merge_ciphers(query->c, (int)dimension))
}

int hydia_alpha_norm_rows(hydia_ctx *ctx, const hydia_ct *query, size_t alpha, size_t row_length, hydia_ct **out) {
    if (alpha > 64 || row_length > (size_t)INT32_MAX) return fail(HYDIA_ERR_ARG, "hydia: row_length must be a power of two in 2 .. slots");
    SENDER_CALL(ctx->cx.alpha_norm_rows(query->c, (int)alpha, (int)row_length))
}
int hydia_alpha_norm_columns(hydia_ctx *ctx, const hydia_ct *query, size_t alpha, size_t row_length, hydia_ct **out) {
    if (alpha > 64 || row_length > (size_t)INT32_MAX) return fail(HYDIA_ERR_ARG, "hydia: row_length must be a power of two in 2 .. slots");
    SENDER_CALL(ctx->cx.alpha_norm_columns(query->c, (int)alpha, (int)row_length))
}
int hydia_grote_index_scenario(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **rows, hydia_ct **cols) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && query && rows && cols, "null argument");
    Ct r, c;
    ctx->cx.grote_index_scenario(query->c, r, c);
    *rows = wrap(ctx, std::move(r));
    *cols = wrap(ctx, std::move(c));
    return HYDIA_OK;
    API_END
}
int hydia_grote_membership_scenario(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out) { SENDER_CALL(ctx->cx.grote_membership_scenario(query->c)) }
int hydia_eval_square_no_relin(hydia_ctx *ctx, const hydia_ct *query, uint32_t n_limbs, hydia_ct **out) {
    if (query && n_limbs > (uint32_t)query->c.nl) return fail(HYDIA_ERR_ARG, "hydia: more limbs than the ciphertext has");
    SENDER_CALL(ctx->cx.grote_square(query->c.alias(n_limbs ? (int)n_limbs : query->c.nl)))
}
int hydia_blind_compute_similarity(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out) { SENDER_CALL(ctx->cx.blind_similarity(query->c)) }
int hydia_blind_index_scenario(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out) { SENDER_CALL(ctx->cx.blind_index_scenario(query->c)) }
int hydia_blind_membership_scenario(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out) { SENDER_CALL(ctx->cx.blind_membership_scenario(query->c)) }
int hydia_compress_ciphers(hydia_ctx *ctx, const hydia_ct *query, size_t dimension, hydia_ct **out) {
    if (dimension > (size_t)INT32_MAX) return fail(HYDIA_ERR_ARG, "hydia: the compression dimension must be a power of two in 2 .. slots");
    SENDER_CALL(ctx->cx.compress_ciphers(query->c, (int)dimension))
}
int hydia_eval_dot_no_relin(hydia_ctx *ctx, const hydia_ct *query, const hydia_ct *b, hydia_ct **out) {
    if (!b) return fail(HYDIA_ERR_ARG, "null argument");
    SENDER_CALL(ctx->cx.eval_dot_no_relin(query->c, b->c))
}
// ------------------------------------------------------------------ primitives
int hydia_ntt(hydia_ctx *ctx, uint64_t *data, uint32_t count, uint32_t m, int inverse) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && data && count >= 1 && (int)m < ctx->cx.nT, "bad argument");
    Context &cx = ctx->cx;
    const size_t bytes = (size_t)count * cx.N * sizeof(u64);
    u64 *d = cx.pool.get(bytes);
    cx.sync();
    HIP_CHECK(hipMemcpy(d, data, bytes, hipMemcpyHostToDevice));
    LimbSel s = cx.sel_range((int)m, (int)m + 1);
    if (inverse) cx.ntt_inv(d, d, cx.N, cx.N, (int)count, s, cx.scale_ninv(s));
    else cx.ntt_fwd(d, cx.N, (int)count, s);
    cx.sync();
    HIP_CHECK(hipMemcpy(data, d, bytes, hipMemcpyDeviceToHost));
    cx.pool.put(d);
    return HYDIA_OK;
    API_END
}
int hydia_ntt_engine(const hydia_ctx *ctx) {
    if (!ctx || ctx->cx.tabs.generic) return 0;
    const int logN = ctx->cx.prm.logN;  // what hk::ntt_forward / ntt_inverse dispatch to
    return logN == 15 ? 15 : (logN == 16 && ctx->cx.tabs.ntt16) ? 16 : 0;
}
int hydia_eval_rotate(hydia_ctx *ctx, const hydia_ct *query, int rot, hydia_ct **out) { SENDER_CALL(ctx->cx.rotate(query->c, rot)) }
int hydia_eval_mult(hydia_ctx *ctx, const hydia_ct *query, const hydia_ct *b, hydia_ct **out) {
    if (!b) return fail(HYDIA_ERR_ARG, "null argument");
    SENDER_CALL(ctx->cx.mult(query->c, b->c))
}
int hydia_eval_mult_no_relin(hydia_ctx *ctx, const hydia_ct *query, const hydia_ct *b, hydia_ct **out) {
    if (!b) return fail(HYDIA_ERR_ARG, "null argument");
    SENDER_CALL(ctx->cx.mult_norelin(query->c, b->c))
}
int hydia_relinearize(hydia_ctx *ctx, hydia_ct *ct) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && ct, "null argument");
    ctx->cx.relinearize(ct->c);
    return HYDIA_OK;
    API_END
}
int hydia_rescale(hydia_ctx *ctx, hydia_ct *ct) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && ct, "null argument");
    ctx->cx.rescale(ct->c);
    return HYDIA_OK;
    API_END
}
int hydia_eval_add(hydia_ctx *ctx, hydia_ct *a, const hydia_ct *b) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && a && b, "null argument");
    ctx->cx.add_inplace(a->c, b->c);
    return HYDIA_OK;
    API_END
}
int hydia_level_reduce(hydia_ctx *ctx, hydia_ct *ct, uint32_t n_limbs) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && ct && n_limbs >= 1, "bad argument");
    if ((int)n_limbs < ct->c.nl) {
        Ct v = ct->c.alias((int)n_limbs);
        ct->c = ctx->cx.clone(v);
    }
    return HYDIA_OK;
    API_END
}

int hydia_eval_mult_plain(hydia_ctx *ctx, const hydia_ct *ct, const double *slots, hydia_ct **out) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && ct && slots && out, "null argument");
    REQUIRE(ct->c.npoly == 2 && ct->c.nl >= 2, "a plaintext multiply needs a 2-component ciphertext with a limb to rescale");
    Context &cx = ctx->cx;
    Ct pt(&cx, 1, 2, ct->c.nl, cx.delta);  // residues, Shoup companions
    client_encode_plain(cx, slots, ct->c.nl, pt.d);
    *out = wrap(ctx, cx.mult_plain_rescale(ct->c, pt.d));
    return HYDIA_OK;
    API_END
}
int hydia_binary_rotate(hydia_ctx *ctx, const hydia_ct *ct, int32_t factor, hydia_ct **out) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && ct && out, "null argument");
    *out = wrap(ctx, ctx->cx.binary_rotate(ct->c, factor));
    return HYDIA_OK;
    API_END
}

// ------------------------------------------------------------------ measurement
int hydia_byte_ledger(int enable, char *out, size_t cap, size_t *needed) {
    const size_t n = (out || needed) ? hk::ledger_dump(out, cap) : 0;
    if (needed) *needed = n;
    if (enable >= 0) hk::ledger_enable(enable != 0);  // (re)starts or stops the recording; -1 = just read
    return HYDIA_OK;
}
/* transform `polys` polynomials x limbs [first_mod, first_mod + n_mods) of pooled scratch memory `iters` times (in place; the
 * data is whatever the pool holds — cost is data independent) and report the HIP-event time per iteration */
int hydia_bench_ntt(hydia_ctx *ctx, uint32_t polys, uint32_t first_mod, uint32_t n_mods, int inverse, uint32_t iters, double *ms_per_iter) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && ms_per_iter && polys >= 1 && n_mods >= 1 && iters >= 1 && (int)(first_mod + n_mods) <= ctx->cx.nT, "bad argument");
    Context &cx = ctx->cx;
    const size_t outer = (size_t)n_mods * cx.N;
    u64 *buf = cx.pool.get((size_t)polys * outer * sizeof(u64));
    HIP_CHECK(hipMemsetAsync(buf, 0, (size_t)polys * outer * sizeof(u64), cx.stream));
    const LimbSel s = cx.sel_range((int)first_mod, (int)(first_mod + n_mods));
    auto once = [&] {
        if (inverse) cx.ntt_inv(buf, buf, outer, outer, (int)polys, s, cx.scale_ninv(s));
        else cx.ntt_fwd(buf, outer, (int)polys, s);
    };
    once();
    hipEvent_t a, b;
    HIP_CHECK(hipEventCreate(&a));
    HIP_CHECK(hipEventCreate(&b));
    HIP_CHECK(hipEventRecord(a, cx.stream));
    for (uint32_t i = 0; i < iters; i++) once();
    HIP_CHECK(hipEventRecord(b, cx.stream));
    HIP_CHECK(hipEventSynchronize(b));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, a, b));
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    cx.pool.put(buf);
    *ms_per_iter = ms / iters;
    return HYDIA_OK;
    API_END
}
int hydia_kernel_time(hydia_ctx *ctx, const char *name, double *total_ms, uint64_t *launches) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx && name, "null argument");
    ctx->cx.base_phase_collect();
    ctx->cx.timer_collect();
    auto it = ctx->cx.timers.find(name);
    if (total_ms) *total_ms = it == ctx->cx.timers.end() ? 0.0 : it->second.total_ms;
    if (launches) *launches = it == ctx->cx.timers.end() ? 0 : (uint64_t)it->second.launches;
    return HYDIA_OK;
    API_END
}
int hydia_kernel_time_reset(hydia_ctx *ctx) {
    API_BEGIN
    use_device(ctx);
    REQUIRE(ctx, "null ctx");
    ctx->cx.base_phase_collect();
    ctx->cx.timer_collect();
    ctx->cx.timers.clear();
    return HYDIA_OK;
    API_END
}

}  // extern "C"
