// image_matching_amd/csrc/client.cpp — receiver / enroller / key generation engines on the GPU.
//
//   client_keygen         cc->KeyGen, EvalMultKeyGen, EvalRotateKeyGen           /root/reference/src/main.cpp:184-206
//   client_encrypt        OpenFHEWrapper::encryptFromVector                      /root/reference/src/openFHE_wrapper.cpp:74-77
//   client_encrypt_query  DiagonalReceiver::encryptQuery                         /root/reference/src/receiver/receiver_diag.cpp:13-26
//   client_decrypt        OpenFHEWrapper::decryptToVector                        /root/reference/src/openFHE_wrapper.cpp:81-85
//   client_enroll         DiagonalEnroller::serializeDB                          /root/reference/src/enroller/enroller_diag.cpp:12-53
// All ring arithmetic, sampling and the canonical-embedding FFT run in HIP kernels; the host only normalises vectors
// (VectorUtils::plaintextNormalize, /root/reference/src/vector_utils.cpp:32-51) and schedules launches.
#include "client.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/hydia.h"  // HY_EVK_ID_SWITCH
#include "client_kernels.h"
#include "rows_norm.h"
#include "select_kernels.h"

namespace hydia {

static ChaChaKey make_key(const uint8_t seed[32]) {
    ChaChaKey k;
    for (int i = 0; i < 8; i++)
        k.k[i] = (unsigned)seed[4 * i] | ((unsigned)seed[4 * i + 1] << 8) | ((unsigned)seed[4 * i + 2] << 16) |
                 ((unsigned)seed[4 * i + 3] << 24);
    return k;
}

// canonical-embedding tables: 5^j mod 2N and exp(2 pi i k / 2N)
static void ensure_embedding_tables(Context &cx) {
    if (cx.d_rot_group) return;
    const int M = 2 * cx.N;
    std::vector<unsigned> rg(cx.slots);
    u64 g = 1;
    for (int j = 0; j < cx.slots; j++) {
        rg[j] = (unsigned)g;
        g = (g * 5) % (u64)M;
    }
    std::vector<double> ksi(2 * (size_t)(M + 1));
    for (int k = 0; k <= M; k++) {
        // explicit glibc sincos(): the specification's table (a compiler may or may not fuse sin()+cos() itself)
        const double ang = 2.0 * M_PI * (double)k / (double)M;
        double sn, cs;
        ::sincos(ang, &sn, &cs);
        ksi[2 * (size_t)k] = cs;
        ksi[2 * (size_t)k + 1] = sn;
    }
    HIP_CHECK(hipMalloc((void **)&cx.d_rot_group, sizeof(unsigned) * rg.size()));
    HIP_CHECK(hipMalloc((void **)&cx.d_ksi, sizeof(double) * ksi.size()));
    HIP_CHECK(hipMemcpy(cx.d_rot_group, rg.data(), sizeof(unsigned) * rg.size(), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(cx.d_ksi, ksi.data(), sizeof(double) * ksi.size(), hipMemcpyHostToDevice));
}

static u64 inv_mod_pow2(u64 g, u64 M) {
    u64 x = 1;
    for (int i = 0; i < 6; i++) x = x * (2 - g * x);
    return x & (M - 1);
}

// hybrid switching key from secret s_from (Q limbs) to secret s_enc (Q u P limbs), written to evk [dnum][2][nT][N] (device memory);
// key_id addresses the sampler streams.  The uniform halves are sampled under akey (a seeded key set: the PUBLIC expansion seed; every
// other caller passes akey == key), the Gaussian errors under key.
// evk_sample_a / pk_sample_a: the ONE launch each that draws the uniform halves — key generation and the import of a half key share it
static void evk_sample_a(Context &cx, const ChaChaKey &akey, u64 key_id, u64 *evk) {
    const int N = cx.N, nT = cx.nT;
    hc::sample_uniform(cx.stream, akey, cx.d_mod, N, HY_STREAM(HY_DOM_EVK_A, key_id, 0, 0), 1ull, 1ull << 8,
                       evk + (size_t)nT * N, (size_t)N, (size_t)2 * nT * N, cx.sel_range(0, nT), cx.prm.dnum);
}
static void pk_sample_a(Context &cx, const ChaChaKey &akey, u64 *pk) {
    hc::sample_uniform(cx.stream, akey, cx.d_mod, cx.N, HY_STREAM(HY_DOM_PK_A, 0, 0, 0), 1ull, 0, pk + (size_t)cx.nQ * cx.N,
                       (size_t)cx.N, 0, cx.sel_q(cx.nQ), 1);
}
static void gen_evk(Context &cx, const ChaChaKey &key, const ChaChaKey &akey, u64 key_id, const u64 *s_enc, const u64 *s_from, u64 *evk) {
    const int N = cx.N, nT = cx.nT, dnum = cx.prm.dnum;
    const LimbSel all = cx.sel_range(0, nT);
    evk_sample_a(cx, akey, key_id, evk);
    int *e32 = (int *)cx.pool.get(sizeof(int) * (size_t)dnum * N);
    hc::sample_gauss(cx.stream, key, N, HY_STREAM(HY_DOM_EVK_E, key_id, 0, 0), 1ull << 8, e32, dnum);
    u64 *e = cx.pool.get(sizeof(u64) * (size_t)dnum * nT * N);
    hc::small_to_limbs(cx.stream, cx.d_mod, N, e32, nullptr, e, (size_t)nT * N, dnum, all);
    cx.ntt_fwd(e, (size_t)nT * N, dnum, all);
    ScaleSel pm{};
    for (int j = 0; j < cx.nQ; j++) pm.s[j] = cx.P_mod_q[j];
    hc::evk_combine(cx.stream, cx.d_mod, N, nT, cx.nQ, cx.alpha, dnum, evk, e, s_enc, s_from, pm);
    cx.pool.put(e);
    cx.pool.put((u64 *)e32);
}

static void keygen_impl(Context &cx, const uint8_t seed[32], const uint8_t *a_seed, const std::vector<int> &rots);
void client_keygen(Context &cx, const uint8_t seed[32], const uint8_t *a_seed) {
    // rotation keys {1..dim-1} u {dim, 2 dim, ... < slots}
    std::vector<int> rots;
    for (int i = 1; i < cx.prm.dim; i++) rots.push_back(i);
    for (int i = cx.prm.dim; i < cx.slots; i <<= 1) rots.push_back(i);
    keygen_impl(cx, seed, a_seed, rots);
}
void client_keygen_rotations(Context &cx, const uint8_t seed[32], const std::vector<int> &rots, const uint8_t *a_seed) {
    for (int r : rots)
        if (r < 1 || r >= cx.slots) throw std::runtime_error("hydia: rotation keys are indexed by r mod slots in [1, slots)");
    if (cx.keys_borrowed) throw StateError("hydia: this context borrows its keys from another context (re-key the owner)");
    // keys outside the new set would belong to the previous secret: release them (and every table that points at rotation keys)
    cx.sync_all();
    for (auto it = cx.rot_keys.begin(); it != cx.rot_keys.end();) {
        if (std::find(rots.begin(), rots.end(), it->first) != rots.end()) {
            ++it;
            continue;
        }
        for (void *p : {(void *)it->second.d, (void *)it->second.d_cell, (void *)it->second.d_gal})
            if (p) HIP_CHECK(hipFree(p));
        it = cx.rot_keys.erase(it);
    }
    cx.rotptrs_valid = cx.giants_valid = false;
    keygen_impl(cx, seed, a_seed, rots);
}
// a_seed != nullptr: the seeded key set — every uniform half under a_seed (the caller has refused a_seed == seed), which the context
// then remembers, and every key written here marked as covered by it
static void keygen_impl(Context &cx, const uint8_t seed[32], const uint8_t *a_seed, const std::vector<int> &rots) {
    const int N = cx.N, nT = cx.nT, nQ = cx.nQ;
    const ChaChaKey key = make_key(seed), akey = a_seed ? make_key(a_seed) : key;
    const LimbSel all = cx.sel_range(0, nT), qsel = cx.sel_q(nQ);
    if (cx.keys_borrowed) throw StateError("hydia: this context borrows its keys from another context (re-key the owner)");
    if (!cx.d_sk) HIP_CHECK(hipMalloc((void **)&cx.d_sk, sizeof(u64) * (size_t)nT * N));
    if (!cx.d_pk) HIP_CHECK(hipMalloc((void **)&cx.d_pk, sizeof(u64) * (size_t)2 * nQ * N));
    int *s32 = (int *)cx.pool.get(sizeof(int) * (size_t)N);
    hc::sample_ternary(cx.stream, key, N, HY_STREAM(HY_DOM_SK, 0, 0, 0), 0, s32, 1);
    hc::small_to_limbs(cx.stream, cx.d_mod, N, s32, nullptr, cx.d_sk, 0, 1, all);
    cx.ntt_fwd(cx.d_sk, 0, 1, all);
    // public key (b, a) = (-a s + e, a)
    pk_sample_a(cx, akey, cx.d_pk);
    hc::sample_gauss(cx.stream, key, N, HY_STREAM(HY_DOM_PK_E, 0, 0, 0), 0, s32, 1);
    hc::small_to_limbs(cx.stream, cx.d_mod, N, s32, nullptr, cx.d_pk, 0, 1, qsel);
    cx.ntt_fwd(cx.d_pk, 0, 1, qsel);
    hc::pk_combine(cx.stream, cx.d_mod, N, nQ, cx.d_pk, cx.d_pk + (size_t)nQ * N, cx.d_sk);
    cx.pool.put((u64 *)s32);
    // relinearisation key: s^2 -> s
    u64 *tmp = cx.pool.get(sizeof(u64) * (size_t)nT * N);
    hc::mul(cx.stream, cx.d_mod, N, cx.d_sk, cx.d_sk, tmp, qsel);
    gen_evk(cx, key, akey, 0, cx.d_sk, tmp, cx.eval_key_storage(0));
    // rotation keys: key r switches s -> sigma_g^{-1}(s), g = 5^r, so EvalFastRotation needs a single automorphism at the very end
    // (see evaluator.cpp, rotate_query); the sampler streams are addressed by r, whatever set r belongs to
    const u64 M = 2ull * N;
    for (int r : rots) {
        const u64 ginv = inv_mod_pow2(cx.galois_elt(r), M);
        hc::automorph(cx.stream, cx.prm.logN, cx.d_sk, tmp, (unsigned)ginv, nT);
        gen_evk(cx, key, akey, (u64)r, tmp, cx.d_sk, cx.eval_key_storage(r));
    }
    cx.pool.put(tmp);
    cx.sync();
    // (eval_key_storage has cleared the mark of every key written above)
    cx.pk_seeded = a_seed != nullptr;
    if (!a_seed) return;
    if (cx.has_key_seed && std::memcmp(cx.key_seed, a_seed, 32) != 0)  // keys an earlier seeded set left behind are another seed's
        for (auto &kv : cx.rot_keys) kv.second.seeded = false;
    std::memcpy(cx.key_seed, a_seed, 32);
    cx.has_key_seed = true;
    cx.relin_key.seeded = true;
    for (int r : rots) cx.rot_keys[r].seeded = true;
}
// The sender's side of a half key: b (host, the [d][0] halves [dnum][nT][N] of key `rot`, or the public key's [nQ][N]) into its strided
// place, and the a halves expanded on the GPU by the launch key generation makes.  Residues are not range-checked.  The key is NOT
// marked seeded here (eval_key_storage clears the mark; the importing context made no key set)
void client_import_eval_key_seeded(Context &cx, int rot, const u64 *b, const uint8_t a_seed[32]) {
    const size_t half = (size_t)cx.nT * cx.N;
    u64 *dst = cx.eval_key_storage(rot);
    cx.sync();
    HIP_CHECK(hipMemcpy2D(dst, 2 * half * sizeof(u64), b, half * sizeof(u64), half * sizeof(u64), (size_t)cx.prm.dnum, hipMemcpyHostToDevice));
    evk_sample_a(cx, make_key(a_seed), (u64)rot, dst);
    cx.sync();
}
void client_import_public_key_seeded(Context &cx, const u64 *b, const uint8_t a_seed[32]) {
    if (cx.keys_borrowed) throw StateError("hydia: this context borrows its keys from another context (re-key the owner)");
    const size_t half = (size_t)cx.nQ * cx.N;
    if (!cx.d_pk) HIP_CHECK(hipMalloc((void **)&cx.d_pk, 2 * half * sizeof(u64)));
    cx.sync();
    HIP_CHECK(hipMemcpy(cx.d_pk, b, half * sizeof(u64), hipMemcpyHostToDevice));
    pk_sample_a(cx, make_key(a_seed), cx.d_pk);
    cx.sync();
    cx.pk_seeded = false;
}
// A key that arrived as a wire message (wire.cpp) and passed its range check: d_src, its unpacked rows in device memory, into its place.
// a_seed == nullptr: the whole key ([dnum][2][nT][N], the public key [2][nQ][N]); otherwise d_src holds the b halves ([dnum][nT][N],
// [nQ][N]) and the a halves are expanded as the two imports above expand them.  What follows a key write follows as for them
void client_install_eval_key(Context &cx, int rot, const u64 *d_src, const uint8_t *a_seed) {
    const size_t half = (size_t)cx.nT * cx.N * sizeof(u64);
    u64 *dst = cx.eval_key_storage(rot);
    if (!a_seed) {
        HIP_CHECK(hipMemcpyAsync(dst, d_src, 2 * half * (size_t)cx.prm.dnum, hipMemcpyDeviceToDevice, cx.stream));
    } else {
        HIP_CHECK(hipMemcpy2DAsync(dst, 2 * half, d_src, half, half, (size_t)cx.prm.dnum, hipMemcpyDeviceToDevice, cx.stream));
        evk_sample_a(cx, make_key(a_seed), (u64)rot, dst);
    }
    cx.sync();
}
void client_install_public_key(Context &cx, const u64 *d_src, const uint8_t *a_seed) {
    if (cx.keys_borrowed) throw StateError("hydia: this context borrows its keys from another context (re-key the owner)");
    const size_t half = (size_t)cx.nQ * cx.N * sizeof(u64);
    if (!cx.d_pk) HIP_CHECK(hipMalloc((void **)&cx.d_pk, 2 * half));
    HIP_CHECK(hipMemcpyAsync(cx.d_pk, d_src, a_seed ? half : 2 * half, hipMemcpyDeviceToDevice, cx.stream));
    if (a_seed) pk_sample_a(cx, make_key(a_seed), cx.d_pk);
    cx.sync();
    cx.pk_seeded = false;
}

// The switching key of a re-keyed database (Context::db_rekey): from the OLD receiver's secret (old_secret, host memory, [nT][N] in
// evaluation form as hydia_export_secret_key gives it; its Q limbs are read) to THIS context's secret — gen_evk's key with the
// reserved id HY_EVK_ID_SWITCH, into out (host memory, [dnum][2][nT][N]).  Nothing of the context changes
void client_keygen_switch(Context &cx, const u64 *old_secret, const uint8_t seed[32], u64 *out) {
    if (!cx.d_sk) throw StateError("hydia: secret key not loaded (a switching key is generated by the NEW receiver, which holds its secret)");
    const size_t sk_elems = (size_t)cx.nT * cx.N, key_elems = (size_t)cx.prm.dnum * 2 * sk_elems;
    u64 *d_old = cx.pool.get(sk_elems * sizeof(u64)), *d_key = cx.pool.get(key_elems * sizeof(u64));
    cx.sync();
    HIP_CHECK(hipMemcpy(d_old, old_secret, sk_elems * sizeof(u64), hipMemcpyHostToDevice));
    const ChaChaKey key = make_key(seed);
    gen_evk(cx, key, key, HY_EVK_ID_SWITCH, cx.d_sk, d_old, d_key);
    cx.sync();
    HIP_CHECK(hipMemcpy(out, d_key, key_elems * sizeof(u64), hipMemcpyDeviceToHost));
    cx.pool.put(d_key);
    cx.pool.put(d_old);
}

// encode + encrypt X slot vectors that already sit in HBM; writes [X][2][nQ][N] at dst
static void encrypt_device(Context &cx, const double *d_slots, int X, const ChaChaKey &key, u64 nonce0, u64 *dst) {
    if (!cx.d_pk) throw StateError("hydia: public key not loaded");
    ensure_embedding_tables(cx);
    const int N = cx.N, nQ = cx.nQ, Nh = cx.slots;
    const LimbSel qsel = cx.sel_q(nQ);
    double2 *work = (double2 *)cx.pool.get(sizeof(double2) * (size_t)X * Nh);
    long long *coeffs = (long long *)cx.pool.get(sizeof(long long) * (size_t)X * N);
    hc::encode(cx.stream, d_slots, work, coeffs, N, X, cx.delta, cx.d_rot_group, (const double2 *)cx.d_ksi);
    int *u32 = (int *)cx.pool.get(sizeof(int) * (size_t)X * N);
    int *e0 = (int *)cx.pool.get(sizeof(int) * (size_t)X * N);
    int *e1 = (int *)cx.pool.get(sizeof(int) * (size_t)X * N);
    const u64 step = 1ull << 16;  // the nonce sits in stream-id field `a`
    hc::sample_ternary(cx.stream, key, N, HY_STREAM(HY_DOM_ENC_U, nonce0, 0, 0), step, u32, X);
    hc::sample_gauss(cx.stream, key, N, HY_STREAM(HY_DOM_ENC_E0, nonce0, 0, 0), step, e0, X);
    hc::sample_gauss(cx.stream, key, N, HY_STREAM(HY_DOM_ENC_E1, nonce0, 0, 0), step, e1, X);
    const size_t pe = (size_t)nQ * N;
    u64 *U = cx.pool.get(sizeof(u64) * X * pe), *T0 = cx.pool.get(sizeof(u64) * X * pe), *T1 = cx.pool.get(sizeof(u64) * X * pe);
    hc::small_to_limbs(cx.stream, cx.d_mod, N, u32, nullptr, U, pe, X, qsel);
    hc::small_to_limbs(cx.stream, cx.d_mod, N, e0, coeffs, T0, pe, X, qsel);
    hc::small_to_limbs(cx.stream, cx.d_mod, N, e1, nullptr, T1, pe, X, qsel);
    cx.ntt_fwd(U, pe, X, qsel);
    cx.ntt_fwd(T0, pe, X, qsel);
    cx.ntt_fwd(T1, pe, X, qsel);
    hc::enc_combine(cx.stream, cx.d_mod, N, nQ, cx.d_pk, U, T0, T1, dst, X);
    for (void *p : {(void *)work, (void *)coeffs, (void *)u32, (void *)e0, (void *)e1, (void *)U, (void *)T0, (void *)T1})
        cx.pool.put((u64 *)p);
}

// encode + encrypt X slot vectors under the SECRET key with a seeded c1: c0 = NTT(e0 + m) - a s, where e0 is encrypt_device's (the
// stream (ENC_E0, nonce) under the secret `key`) and a limb j is the uniform stream (SYM_A, nonce, 0, j) under the PUBLIC akey, drawn
// inside k_enc_sym.  One sampled polynomial and one transform batch where encrypt_device takes three of each.  Writes c0 [X][nQ][N] at
// c0 and, when c1 != nullptr, a [X][nQ][N] at c1.  The two streams take nonces of their own: e0 of element x is at nonce0 + x, a at
// a_nonce0 + x (a query: the same; a database block: the enrolment's nonce and the one its wire message names)
static void encrypt_sym_device(Context &cx, const double *d_slots, int X, const ChaChaKey &key, const ChaChaKey &akey, u64 nonce0, u64 a_nonce0,
                               u64 *c0, u64 *c1 = nullptr) {
    if (!cx.d_sk) throw StateError("hydia: secret key not loaded (seeded encryption is the secret-key holder's; hydia_encrypt_query takes the public key)");
    ensure_embedding_tables(cx);
    const int N = cx.N, nQ = cx.nQ, Nh = cx.slots;
    const LimbSel qsel = cx.sel_q(nQ);
    double2 *work = (double2 *)cx.pool.get(sizeof(double2) * (size_t)X * Nh);
    long long *coeffs = (long long *)cx.pool.get(sizeof(long long) * (size_t)X * N);
    hc::encode(cx.stream, d_slots, work, coeffs, N, X, cx.delta, cx.d_rot_group, (const double2 *)cx.d_ksi);
    int *e0 = (int *)cx.pool.get(sizeof(int) * (size_t)X * N);
    hc::sample_gauss(cx.stream, key, N, HY_STREAM(HY_DOM_ENC_E0, nonce0, 0, 0), 1ull << 16, e0, X);
    const size_t pe = (size_t)nQ * N;
    u64 *T0 = cx.pool.get(sizeof(u64) * X * pe);
    hc::small_to_limbs(cx.stream, cx.d_mod, N, e0, coeffs, T0, pe, X, qsel);
    cx.ntt_fwd(T0, pe, X, qsel);
    hc::enc_sym(cx.stream, akey, cx.d_mod, N, nQ, HY_STREAM(HY_DOM_SYM_A, a_nonce0, 0, 0), T0, cx.d_sk, c0, c1, X);
    for (void *p : {(void *)work, (void *)coeffs, (void *)e0, (void *)T0}) cx.pool.put((u64 *)p);
}

Ct client_encrypt(Context &cx, const double *slots, int count, const uint8_t seed[32], uint64_t nonce0) {
    const size_t bytes = sizeof(double) * (size_t)count * cx.slots;
    double *d_slots = (double *)cx.pool.get(bytes);
    HIP_CHECK(hipMemcpyAsync(d_slots, slots, bytes, hipMemcpyHostToDevice, cx.stream));
    Ct out(&cx, count, 2, cx.nQ, cx.delta);
    encrypt_device(cx, d_slots, count, make_key(seed), nonce0, out.d);
    cx.pool.put((u64 *)d_slots);
    cx.sync();  // `slots` is caller memory
    return out;
}

// the plaintext of EvalMult(ct, MakeCKKSPackedPlaintext(v)) under FIXEDMANUAL: v encoded at scale 2^scale_bits (the encoder of
// encrypt_device) and reduced onto limbs 0..nl-1 of the ciphertext it multiplies, then transformed; the Shoup companions
// floor(m 2^64 / q_j) are formed on the host once per plaintext
void client_encode_plain(Context &cx, const double *slots, int nl, u64 *pt) {
    if (nl < 1 || nl > cx.nQ) throw std::runtime_error("hydia: plaintext limb count outside 1 .. n_q");
    ensure_embedding_tables(cx);
    const int N = cx.N, Nh = cx.slots;
    const LimbSel qsel = cx.sel_q(nl);
    double *d_slots = (double *)cx.pool.get(sizeof(double) * (size_t)Nh);
    double2 *work = (double2 *)cx.pool.get(sizeof(double2) * (size_t)Nh);
    long long *coeffs = (long long *)cx.pool.get(sizeof(long long) * (size_t)N);
    HIP_CHECK(hipMemcpyAsync(d_slots, slots, sizeof(double) * (size_t)Nh, hipMemcpyHostToDevice, cx.stream));
    hc::encode(cx.stream, d_slots, work, coeffs, N, 1, cx.delta, cx.d_rot_group, (const double2 *)cx.d_ksi);
    hc::small_to_limbs(cx.stream, cx.d_mod, N, nullptr, coeffs, pt, 0, 1, qsel);
    cx.ntt_fwd(pt, 0, 1, qsel);
    std::vector<u64> m((size_t)nl * N);
    HIP_CHECK(hipMemcpyAsync(m.data(), pt, sizeof(u64) * m.size(), hipMemcpyDeviceToHost, cx.stream));
    cx.sync();  // `slots` is caller memory, m is read below
    for (int j = 0; j < nl; j++)
        for (int c = 0; c < N; c++) {
            u64 &v = m[(size_t)j * N + c];
            v = (u64)(((unsigned __int128)v << 64) / cx.q[j]);
        }
    HIP_CHECK(hipMemcpy(pt + (size_t)nl * N, m.data(), sizeof(u64) * m.size(), hipMemcpyHostToDevice));  // the stream is idle
    cx.pool.put((u64 *)coeffs);
    cx.pool.put((u64 *)work);
    cx.pool.put((u64 *)d_slots);
}

// VectorUtils::plaintextNormalize (vector_utils.cpp:42-51): divide by the L2 norm, zero vector passes through
// (the arithmetic lives in rows_norm.h, where k_rows_widen and the host check share it)
static void normalize(double *x, int dim) { rn_normalise_row(x, dim); }

Ct client_encrypt_query(Context &cx, const double *query, const uint8_t seed[32], uint64_t nonce) {
    const int dim = cx.prm.dim;
    std::vector<double> qn(query, query + dim), batch(cx.slots);
    normalize(qn.data(), dim);                                                       // receiver_diag.cpp:17
    for (int i = 0; i < cx.slots; i += dim) std::memcpy(&batch[i], qn.data(), sizeof(double) * dim);  // :18-21
    return client_encrypt(cx, batch.data(), 1, seed, nonce);                          // :23
}

// pooled device buffers of one call, back in the pool when it ends (after the stream has been synchronised)
namespace {
struct PoolHold {
    Context &cx;
    std::vector<u64 *> held;
    explicit PoolHold(Context &c) : cx(c) {}
    PoolHold(const PoolHold &) = delete;
    template <class T>
    T *get(size_t count) {
        held.push_back(cx.pool.get(sizeof(T) * count));
        return (T *)held.back();
    }
    ~PoolHold() {
        for (auto it = held.rbegin(); it != held.rend(); ++it) cx.pool.put(*it);
    }
};
}  // namespace
// dec_dot, inverse transform and decode of ct, enqueued on the stream: the X * slots doubles land at d_out (device memory)
static void decrypt_enqueue(Context &cx, const Ct &ct, double *d_out, PoolHold &hold) {
    if (!cx.d_sk) throw StateError("hydia: secret key not loaded");
    ensure_embedding_tables(cx);
    const int N = cx.N, Nh = cx.slots, X = ct.X, nu = ct.nl < 2 ? ct.nl : 2;
    u64 *t = hold.get<u64>((size_t)X * nu * N);
    hc::dec_dot(cx.stream, cx.d_mod, N, ct.npoly, ct.lstride, ct.d, cx.d_sk, t, nu, X);
    const LimbSel s = cx.sel_q(nu);
    cx.ntt_inv(t, t, (size_t)nu * N, (size_t)nu * N, X, s, cx.scale_ninv(s));
    double2 *work = hold.get<double2>((size_t)X * Nh);
    const u64 q0inv = cx.nQ >= 2 ? invmod_u64(cx.q[0] % cx.q[1], cx.q[1]) : 0;
    hc::decode(cx.stream, cx.d_mod, t, nu, N, X, ct.scale, q0inv, work, d_out, cx.d_rot_group, (const double2 *)cx.d_ksi);
}
void client_decrypt(Context &cx, const Ct &ct, double *out) {
    PoolHold hold(cx);
    const size_t n = (size_t)ct.X * cx.slots;
    double *d_out = hold.get<double>(n);
    decrypt_enqueue(cx, ct, d_out, hold);
    HIP_CHECK(hipMemcpyAsync(out, d_out, sizeof(double) * n, hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
}
void client_decrypt_device(Context &cx, const Ct &ct, double *dev_out) {
    PoolHold hold(cx);
    decrypt_enqueue(cx, ct, dev_out, hold);
    cx.sync();
}
double client_decrypt_slot0(Context &cx, const Ct &ct) {
    PoolHold hold(cx);
    double *d_out = hold.get<double>((size_t)ct.X * cx.slots);
    decrypt_enqueue(cx, ct, d_out, hold);
    double v = 0;
    HIP_CHECK(hipMemcpyAsync(&v, d_out, sizeof(double), hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
    return v;
}

// ---- candidate lists and matches (select_kernels.hip): the selection stage behind the decoder
static_assert(sizeof(size_t) == sizeof(uint64_t), "the kernels write indices as 64-bit words straight into size_t arrays");
// the ordered compaction of v[0..n) under p, enqueued: count, scan, scatter (no scatter when nothing can be written)
static void compact_enqueue(Context &cx, const double *v, size_t n, const SelPred &p, unsigned *tiles, unsigned *total, uint64_t *d_idx, double *d_val) {
    cx.timer_begin("k_select_count");
    hc::select_count(cx.stream, v, n, p, tiles);
    cx.timer_end("k_select_count");
    cx.timer_begin("k_select_scan");
    hc::select_scan(cx.stream, tiles, hc::select_tiles(n), total);
    cx.timer_end("k_select_scan");
    if (!d_idx) return;
    cx.timer_begin("k_select_scatter");
    hc::select_scatter(cx.stream, v, n, p, tiles, d_idx, d_val);
    cx.timer_end("k_select_scatter");
}
// result r of a batch: its decoded slots (decrypted here, or the caller's device array) and how many of them are searched
static const double *select_source(Context &cx, const SelectSource &src, size_t r, PoolHold &hold, size_t &n) {
    if (src.dev_vals) {
        n = src.n;
        return src.dev_vals;
    }
    const Ct &ct = *src.cts[r];
    const size_t all = (size_t)ct.X * cx.slots;
    double *d = hold.get<double>(all);
    decrypt_enqueue(cx, ct, d, hold);
    n = src.n ? src.n : all;
    return d;
}
void client_select(Context &cx, const SelectSource &src, double threshold, size_t *idx_out, double *val_out, size_t cap, size_t *n_out) {
    PoolHold hold(cx);
    const size_t R = src.n_results;
    if (!idx_out) cap = 0;
    unsigned *d_total = hold.get<unsigned>(R);
    std::vector<uint64_t *> d_idx(R, nullptr);
    std::vector<double *> d_val(R, nullptr);
    std::vector<size_t> room(R);
    for (size_t r = 0; r < R; r++) {
        size_t n;
        const double *v = select_source(cx, src, r, hold, n);
        room[r] = std::min(cap, n);
        if (room[r]) {
            d_idx[r] = hold.get<uint64_t>(room[r]);
            if (val_out) d_val[r] = hold.get<double>(room[r]);
        }
        const SelPred p{HY_SEL_GE, threshold, (unsigned)room[r], 0, nullptr};
        compact_enqueue(cx, v, n, p, hold.get<unsigned>(hc::select_tiles(n)), d_total + r, d_idx[r], d_val[r]);
    }
    std::vector<unsigned> total(R);
    HIP_CHECK(hipMemcpyAsync(total.data(), d_total, sizeof(unsigned) * R, hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
    // (the stream is idle: only the entries that were written cross to the host)
    for (size_t r = 0; r < R; r++) {
        const size_t w = std::min((size_t)total[r], room[r]);
        if (w) HIP_CHECK(hipMemcpy(idx_out + r * cap, d_idx[r], sizeof(uint64_t) * w, hipMemcpyDeviceToHost));
        if (w && val_out) HIP_CHECK(hipMemcpy(val_out + r * cap, d_val[r], sizeof(double) * w, hipMemcpyDeviceToHost));
        n_out[r] = total[r];
    }
}
void client_topk(Context &cx, const SelectSource &src, size_t k, size_t *idx_out, double *val_out, size_t *n_out) {
    PoolHold hold(cx);
    const size_t R = src.n_results;
    std::vector<size_t> kk(R);
    size_t vs = 0;  // the row stride of the values: the caller's k, or the largest row when the caller wants none (the final sort needs them)
    for (size_t r = 0; r < R; r++) {
        const size_t n = src.dev_vals || src.n ? src.n : (size_t)src.cts[r]->X * cx.slots;
        vs = std::max(vs, kk[r] = std::min(k, n));
    }
    std::vector<double> vals;
    if (val_out) vs = k;
    else vals.resize(R * vs);
    double *const vrow = val_out ? val_out : vals.data();
    for (size_t r = 0; r < R; r++) {
        size_t n;
        const double *v = select_source(cx, src, r, hold, n);
        const size_t kr = kk[r];
        SelState *state = hold.get<SelState>(1);
        unsigned *tiles = hold.get<unsigned>(hc::select_tiles(n)), *total = hold.get<unsigned>(1);
        uint64_t *d_idx = hold.get<uint64_t>(kr);
        double *d_val = hold.get<double>(kr);
        HIP_CHECK(hipMemsetAsync(state, 0, sizeof(SelState), cx.stream));
        for (int pass = 0; pass < 8; pass++) {
            cx.timer_begin("k_topk_hist");
            hc::topk_hist(cx.stream, v, n, pass, state);
            cx.timer_end("k_topk_hist");
            cx.timer_begin("k_topk_pick");
            hc::topk_pick(cx.stream, pass, (unsigned)kr, state);
            cx.timer_end("k_topk_pick");
        }
        compact_enqueue(cx, v, n, SelPred{HY_SEL_ABOVE, 0.0, 0, (unsigned)kr, state}, tiles, total, d_idx, d_val);
        compact_enqueue(cx, v, n, SelPred{HY_SEL_TIE, 0.0, 0, (unsigned)kr, state}, tiles, total, d_idx, d_val);
        HIP_CHECK(hipMemcpyAsync(idx_out + r * k, d_idx, sizeof(uint64_t) * kr, hipMemcpyDeviceToHost, cx.stream));
        HIP_CHECK(hipMemcpyAsync(vrow + r * vs, d_val, sizeof(double) * kr, hipMemcpyDeviceToHost, cx.stream));
    }
    cx.sync();
    // the survivors arrive as (keys above the k-th in index order, then ties of the k-th in index order): value descending, index ascending
    std::vector<std::pair<uint64_t, size_t>> order;
    std::vector<double> tmp;
    for (size_t r = 0; r < R; r++) {
        size_t *ix = idx_out + r * k;
        double *vv = vrow + r * vs;
        order.resize(kk[r]);
        tmp.assign(vv, vv + kk[r]);
        for (size_t i = 0; i < kk[r]; i++) {
            uint64_t bits;
            std::memcpy(&bits, &vv[i], 8);
            order[i] = {~hy_sel_key(bits), ix[i]};
        }
        std::vector<size_t> perm(kk[r]);
        for (size_t i = 0; i < kk[r]; i++) perm[i] = i;
        std::sort(perm.begin(), perm.end(), [&](size_t a, size_t b) { return order[a] < order[b]; });
        for (size_t i = 0; i < kk[r]; i++) {
            ix[i] = order[perm[i]].second;
            vv[i] = tmp[perm[i]];
        }
        n_out[r] = kk[r];
    }
}

// encode X slot vectors that already sit in HBM as plaintexts: the front half of encrypt_device (the encoder at scale 2^scale_bits,
// the coefficients onto all n_q limbs with no error term, the forward transform); writes [X][nQ][N] canonical residues at dst.
// Needs no key and no sampler
static void encode_device(Context &cx, const double *d_slots, int X, u64 *dst) {
    ensure_embedding_tables(cx);
    const int N = cx.N, nQ = cx.nQ, Nh = cx.slots;
    const LimbSel qsel = cx.sel_q(nQ);
    double2 *work = (double2 *)cx.pool.get(sizeof(double2) * (size_t)X * Nh);
    long long *coeffs = (long long *)cx.pool.get(sizeof(long long) * (size_t)X * N);
    hc::encode(cx.stream, d_slots, work, coeffs, N, X, cx.delta, cx.d_rot_group, (const double2 *)cx.d_ksi);
    const size_t pe = (size_t)nQ * N;
    hc::small_to_limbs(cx.stream, cx.d_mod, N, nullptr, coeffs, dst, pe, X, qsel);
    cx.ntt_fwd(dst, pe, X, qsel);
    cx.pool.put((u64 *)coeffs);
    cx.pool.put((u64 *)work);
}
// DiagonalSender::encodeQuery — a probe the sender knows: exactly the plaintext client_encrypt_query encrypts (normalised, tiled to all
// slots, encoded at 2^scale_bits on all n_q limbs), as ONE polynomial [1][1][nQ][N].  No seed, no nonce, no public key
Ct client_encode_query(Context &cx, const double *query) {
    const int dim = cx.prm.dim;
    std::vector<double> qn(query, query + dim), batch(cx.slots);
    normalize(qn.data(), dim);
    for (int i = 0; i < cx.slots; i += dim) std::memcpy(&batch[i], qn.data(), sizeof(double) * dim);
    const size_t bytes = sizeof(double) * (size_t)cx.slots;
    double *d_slots = (double *)cx.pool.get(bytes);
    HIP_CHECK(hipMemcpyAsync(d_slots, batch.data(), bytes, hipMemcpyHostToDevice, cx.stream));
    Ct out(&cx, 1, 1, cx.nQ, cx.delta);
    encode_device(cx, d_slots, 1, out.d);
    cx.pool.put((u64 *)d_slots);
    cx.sync();  // `batch` is host memory of this call
    return out;
}
// ---- where the rows of a block loop come from: the caller's host array (normalised up front by the host entry point, copied block by
// block) or rows already in device memory (hydia_dev_rows: widened and normalised by ONE k_rows_widen launch per block on that block's
// slice).  Either way d_rows holds dense normalised doubles afterwards, and everything behind it is shared
struct RowSource {
    const double *host = nullptr;
    const DevRows *dev = nullptr;
    int normalise = 0;  // device rows only
    // rows first .. first + count - 1 of the source -> d_rows[count][dim], on the context's stream
    void stage(Context &cx, size_t first, size_t count, double *d_rows) const {
        const int dim = cx.prm.dim;
        if (dev)
            hc::rows_widen(cx.stream, (const char *)dev->ptr + first * dev->stride * hc::rows_elem_size(dev->dtype), dev->dtype, count, dim,
                           dev->stride, normalise, d_rows);
        else
            HIP_CHECK(hipMemcpyAsync(d_rows, host + first * dim, sizeof(double) * count * dim, hipMemcpyHostToDevice, cx.stream));
    }
};
// the context's stream waits for what the producer stream has enqueued so far (no host synchronisation); NULL: the caller guarantees
// that the rows are complete
static void wait_for_producer(Context &cx, hipStream_t producer) {
    if (!producer) return;
    hipEvent_t ev;
    HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, producer);
    if (e == hipSuccess) e = hipStreamWaitEvent(cx.stream, ev, 0);
    (void)hipEventDestroy(ev);  // (released once the recorded work has completed)
    HIP_CHECK(e);
}
void client_rows_widen(Context &cx, const DevRows &rows, int normalise, double *dev_dst) {
    wait_for_producer(cx, rows.stream);
    hc::rows_widen(cx.stream, rows.ptr, rows.dtype, rows.n, cx.prm.dim, rows.stride, normalise, dev_dst);
    cx.sync();
}

#define HY_DB_NONCE_BASE (1ull << 36)
#define HY_NONCE_LIMIT (1ull << 40)
// The block loop of an enrolment.  key != nullptr: DiagonalEnroller::serializeDB — per group of `slots` rows pack the generalised
// diagonals (enroller_diag.cpp:37-45) and encrypt the vector_dim slot vectors (:48-52) into the resident HBM layout.  key == nullptr:
// PlainEnroller::serializeDB — the same slot vectors ENCODED (one polynomial each): plaintext t is the slot image of ciphertext t
static void enroll_blocks(Context &cx, const RowSource &src, size_t n, const ChaChaKey *key, size_t first_block, int babies) {
    const int dim = cx.prm.dim, Nh = cx.slots;
    const size_t G = cx.db_cts / dim, out_elems = (size_t)(key ? 2 : 1) * cx.nQ * cx.N;
    double *d_rows = (double *)cx.pool.get(sizeof(double) * (size_t)Nh * dim);
    double *d_slots = (double *)cx.pool.get(sizeof(double) * (size_t)dim * Nh);
    u64 *d_out = cx.pool.get(sizeof(u64) * (size_t)dim * out_elems);  // one group of fresh ciphertexts / plaintexts before packing
    for (size_t g = 0; g < G; g++) {
        const size_t first = g * (size_t)Nh;
        const size_t rows = n > first ? std::min((size_t)Nh, n - first) : 0;
        if (rows) src.stage(cx, first, rows, d_rows);
        hc::diag_pack(cx.stream, d_rows, (long long)rows, dim, Nh, d_slots, (babies > 0 && babies < dim) ? babies : 0);
        if (key) encrypt_device(cx, d_slots, dim, *key, HY_DB_NONCE_BASE + (first_block + g) * dim, d_out);
        else encode_device(cx, d_slots, dim, d_out);
        cx.db_store(g * dim, d_out, dim);
    }
    cx.sync();
    cx.pool.put(d_out);
    cx.pool.put((u64 *)d_slots);
    cx.pool.put((u64 *)d_rows);
}
// nonces are a 40-bit field of the sampler stream id: block first_block + g uses HY_DB_NONCE_BASE + (first_block + g) dim ..
static void check_db_nonces(size_t first_block, size_t blocks, int dim) {
    if (first_block > (HY_NONCE_LIMIT - HY_DB_NONCE_BASE) / (size_t)dim || blocks > (HY_NONCE_LIMIT - HY_DB_NONCE_BASE) / (size_t)dim - first_block)
        throw std::runtime_error("hydia: first_block + number of blocks exceeds the 2^40 nonce space of the encryption sampler");
}
// PlainEnroller::serializeDB — a gallery the sender may see (database kinds 7 / 8): normalise IN PLACE and pack the generalised
// diagonals exactly as client_enroll does, then ENCODE the vector_dim slot vectors of each block (one polynomial each) into the resident
// layout.  Plaintext t is the slot image of client_enroll's ciphertext t.
void client_plain_enroll(Context &cx, double *db, size_t n, int babies) {
    const int dim = cx.prm.dim;
    for (size_t v = 0; v < n; v++) normalize(db + v * dim, dim);
    RowSource src;
    src.host = db;
    enroll_blocks(cx, src, n, nullptr, 0, babies);
}
// the same from rows in device memory: every row is normalised by the kernel, the source is not written
void client_plain_enroll_device(Context &cx, const DevRows &rows, int babies) {
    RowSource src;
    src.dev = &rows;
    src.normalise = 1;
    wait_for_producer(cx, rows.stream);
    enroll_blocks(cx, src, rows.n, nullptr, 0, babies);
}

// DiagonalEnroller::serializeDB: normalise IN PLACE (enroller_diag.cpp:32-35), then the block loop above.
void client_enroll(Context &cx, double *db, size_t n, const uint8_t seed[32], size_t first_block, int babies) {
    const int dim = cx.prm.dim;
    for (long long v = 0; v < (long long)n; v++) normalize(db + (size_t)v * dim, dim);
    const ChaChaKey key = make_key(seed);
    check_db_nonces(first_block, cx.db_cts / dim, dim);
    RowSource src;
    src.host = db;
    enroll_blocks(cx, src, n, &key, first_block, babies);
}
void client_enroll_device(Context &cx, const DevRows &rows, const uint8_t seed[32], size_t first_block, int babies) {
    const int dim = cx.prm.dim;
    const ChaChaKey key = make_key(seed);
    check_db_nonces(first_block, cx.db_cts / dim, dim);
    RowSource src;
    src.dev = &rows;
    src.normalise = 1;
    wait_for_producer(cx, rows.stream);
    enroll_blocks(cx, src, rows.n, &key, first_block, babies);
}

// The walk over the blocks that source rows placed at vectors first_vector .. first_vector + n - 1 touch, shared by an in-place update
// and a delta: per touched block g the rows are staged and packed into the block's vector_dim slot images (diag_pack with the form
// `babies` and the rows' first slot), then block(g, d_slots) encrypts or encodes them and places the result.
template <class Block>
static void walk_touched_blocks(Context &cx, size_t first_vector, const RowSource &src, size_t n, int babies, Block block) {
    const int dim = cx.prm.dim;
    const size_t Nh = (size_t)cx.slots, end = first_vector + n;
    PoolBuf rows(cx.pool, sizeof(double) * Nh * dim), slots(cx.pool, sizeof(double) * (size_t)dim * Nh);
    double *d_rows = (double *)rows.p, *d_slots = (double *)slots.p;
    for (size_t g = first_vector / Nh; g * Nh < end; g++) {
        const size_t lo = std::max(first_vector, g * Nh), hi = std::min(end, (g + 1) * Nh);
        src.stage(cx, lo - first_vector, hi - lo, d_rows);
        hc::diag_pack(cx.stream, d_rows, (long long)(hi - lo), dim, (int)Nh, d_slots, (babies > 0 && babies < dim) ? babies : 0, (int)(lo - g * Nh));
        block(g, d_slots);
    }
}
// The block loop of an in-place update of a resident diagonal database (kind 5 / 6, key != nullptr) or plain gallery (kind 7 / 8,
// key == nullptr): the sparse diagonal image of the n source rows at vectors first_vector .. first_vector + n - 1, freshly ENCRYPTED
// with the enrolment's nonces or ENCODED, is added to the blocks they touch.  Per touched block: the walk above, encrypt_device /
// encode_device, then db_accumulate for a block that existed or db_store for a new one — a new block is bit-identical to that block of
// an enrolment of the same rows (with the same seed).  Form and kind stay.
static void update_blocks(Context &cx, size_t first_vector, const RowSource &src, size_t n, const ChaChaKey *key, size_t first_block) {
    const int dim = cx.prm.dim, Nh = cx.slots;
    const size_t G_old = cx.db_cts / dim, out_elems = (size_t)(key ? 2 : 1) * cx.nQ * cx.N;
    const size_t n_new = std::max(cx.db_vectors, first_vector + n), G_new = (n_new + (size_t)Nh - 1) / (size_t)Nh;
    if (key) check_db_nonces(first_block, G_new, dim);
    cx.db_grow(n_new, G_new * (size_t)dim);  // (throws before anything is touched when a larger database does not fit)
    PoolBuf out(cx.pool, sizeof(u64) * (size_t)dim * out_elems);
    walk_touched_blocks(cx, first_vector, src, n, cx.db_babies, [&](size_t g, const double *d_slots) {
        if (key) encrypt_device(cx, d_slots, dim, *key, HY_DB_NONCE_BASE + (first_block + g) * dim, out.p);
        else encode_device(cx, d_slots, dim, out.p);
        if (g < G_old) cx.db_accumulate(g * dim, out.p, dim);
        else cx.db_store(g * dim, out.p, dim);
    });
    cx.sync();
}
// In-place update of a resident diagonal database (kind 5 / 6): a FRESH encryption of the sparse diagonal image of `rows` at vectors
// first_vector .. first_vector + n - 1 is added to the blocks they touch (append: first_vector = the vector count — the padding slots
// hold encryptions of zero; remove: the negated template; replace: new - old, normalise = 0).
void client_db_update(Context &cx, size_t first_vector, double *rows, size_t n, int normalise, const uint8_t seed[32], size_t first_block) {
    if (n == 0) return;
    const int dim = cx.prm.dim;
    if (normalise)
        for (size_t v = 0; v < n; v++) normalize(rows + v * dim, dim);
    const ChaChaKey key = make_key(seed);
    RowSource src;
    src.host = rows;
    update_blocks(cx, first_vector, src, n, &key, first_block);
}
void client_db_update_device(Context &cx, size_t first_vector, const DevRows &rows, int normalise, const uint8_t seed[32], size_t first_block) {
    if (rows.n == 0) return;
    const ChaChaKey key = make_key(seed);
    RowSource src;
    src.dev = &rows;
    src.normalise = normalise;
    wait_for_producer(cx, rows.stream);
    update_blocks(cx, first_vector, src, rows.n, &key, first_block);
}

// The enroller's half of update_blocks, for a database that lies on ANOTHER machine (hydia_db_delta_make[_seeded]): per touched block
// the same walk (form `babies`) and an encryption under the enrolment's nonces, then k_wire_pack straight from the block buffer and a
// copy of the packed rows to host memory at payload0 + b * stride for the b-th touched block.  The resident database, if there is one,
// is neither read nor written.  One block is in flight at a time.
//   akey == nullptr: encrypt_device, both polynomials packed.  Needs the public key alone.
//   akey != nullptr (the SEEDED delta of a key-holding enroller): encrypt_sym_device — one sampled polynomial (e0 under `key` at the same
//   nonce) and one transform batch; a is drawn inside k_enc_sym under the PUBLIC akey at (first_block + block) * vector_dim, the nonce0
//   of the block's message, and c1 is never written; c0 alone is packed.  Needs the secret key.
static void delta_blocks(Context &cx, size_t first_vector, const RowSource &src, size_t n, const ChaChaKey &key, const ChaChaKey *akey, int babies,
                         size_t first_block, unsigned char *payload0, size_t stride) {
    const int dim = cx.prm.dim, npoly = akey ? 1 : 2;
    const size_t g0 = first_vector / (size_t)cx.slots, elems = (size_t)cx.nQ * cx.N;
    const WireRows R = hc::wire_rows(cx.q.data(), cx.N, cx.nQ);
    const size_t packed_bytes = (size_t)dim * npoly * R.off[cx.nQ] * sizeof(u64);
    PoolBuf out(cx.pool, sizeof(u64) * (size_t)dim * npoly * elems), packed(cx.pool, packed_bytes);
    walk_touched_blocks(cx, first_vector, src, n, babies, [&](size_t g, const double *d_slots) {
        const u64 block0 = (first_block + g) * dim;
        if (akey) encrypt_sym_device(cx, d_slots, dim, key, *akey, HY_DB_NONCE_BASE + block0, block0, out.p);
        else encrypt_device(cx, d_slots, dim, key, HY_DB_NONCE_BASE + block0, out.p);
        cx.timer_begin("k_wire_pack");
        hc::wire_pack(cx.stream, cx.d_mod, cx.N, out.p, npoly * elems, akey ? 0 : elems, (size_t)dim, npoly, cx.nQ, R, packed.p);
        cx.timer_end("k_wire_pack");
        HIP_CHECK(hipMemcpyAsync(payload0 + (g - g0) * stride, packed.p, packed_bytes, hipMemcpyDeviceToHost, cx.stream));
        cx.sync();  // the host buffer is the caller's; the block buffers are reused by the next block
    });
}
// what the four front-ends share: the nonce space (a refused call leaves host rows as they were), the rows (host_rows normalised IN
// PLACE, or dev_rows by the kernel that stages them), the walk
static void delta_make(Context &cx, size_t first_vector, double *host_rows, const DevRows *dev_rows, size_t n, int normalise, const uint8_t seed[32],
                       const uint8_t *a_seed, int babies, size_t first_block, unsigned char *payload0, size_t stride) {
    const int dim = cx.prm.dim;
    check_db_nonces(first_block, (first_vector + n + (size_t)cx.slots - 1) / (size_t)cx.slots, dim);
    RowSource src;
    src.host = host_rows;
    src.dev = dev_rows;
    if (dev_rows) {
        src.normalise = normalise;
        wait_for_producer(cx, dev_rows->stream);
    } else if (normalise) {
        for (size_t v = 0; v < n; v++) normalize(host_rows + v * dim, dim);
    }
    const ChaChaKey akey = a_seed ? make_key(a_seed) : ChaChaKey{};
    delta_blocks(cx, first_vector, src, n, make_key(seed), a_seed ? &akey : nullptr, babies, first_block, payload0, stride);
}
void client_db_delta_make(Context &cx, size_t first_vector, double *rows, size_t n, int normalise, const uint8_t seed[32], int babies,
                          size_t first_block, unsigned char *payload0, size_t stride) {
    delta_make(cx, first_vector, rows, nullptr, n, normalise, seed, nullptr, babies, first_block, payload0, stride);
}
void client_db_delta_make_device(Context &cx, size_t first_vector, const DevRows &rows, int normalise, const uint8_t seed[32], int babies,
                                 size_t first_block, unsigned char *payload0, size_t stride) {
    delta_make(cx, first_vector, nullptr, &rows, rows.n, normalise, seed, nullptr, babies, first_block, payload0, stride);
}
void client_db_delta_make_seeded(Context &cx, size_t first_vector, double *rows, size_t n, int normalise, const uint8_t seed[32],
                                 const uint8_t a_seed[32], int babies, size_t first_block, unsigned char *payload0, size_t stride) {
    delta_make(cx, first_vector, rows, nullptr, n, normalise, seed, a_seed, babies, first_block, payload0, stride);
}
void client_db_delta_make_seeded_device(Context &cx, size_t first_vector, const DevRows &rows, int normalise, const uint8_t seed[32],
                                        const uint8_t a_seed[32], int babies, size_t first_block, unsigned char *payload0, size_t stride) {
    delta_make(cx, first_vector, nullptr, &rows, rows.n, normalise, seed, a_seed, babies, first_block, payload0, stride);
}

// In-place update of a resident PLAIN gallery (kind 7 / 8): the update loop with encode_device in place of encrypt_device — no seed,
// no nonce.  The encoder rounds once per update, and symmetrically: encode(-x) + encode(x) = 0 in every residue, so the negated rows
// restore an existing block exactly.
void client_plain_db_update(Context &cx, size_t first_vector, double *rows, size_t n, int normalise) {
    if (n == 0) return;
    const int dim = cx.prm.dim;
    if (normalise)
        for (size_t v = 0; v < n; v++) normalize(rows + v * dim, dim);
    RowSource src;
    src.host = rows;
    update_blocks(cx, first_vector, src, n, nullptr, 0);
}
void client_plain_db_update_device(Context &cx, size_t first_vector, const DevRows &rows, int normalise) {
    if (rows.n == 0) return;
    RowSource src;
    src.dev = &rows;
    src.normalise = normalise;
    wait_for_producer(cx, rows.stream);
    update_blocks(cx, first_vector, src, rows.n, nullptr, 0);
}

// Probes in device memory, as encrypted queries (key != nullptr: query i is client_encrypt_query(row i, seed, nonce0 + i), bit for
// bit) or as plain queries (client_encode_query(row i)): per pass ONE k_rows_widen launch normalises the probes, ONE k_query_tile tiles
// them over all slots, ONE encrypt_device / encode_device over the whole pass makes the polynomials (encrypt_device steps the nonce
// per batch element), and each query gets a handle of its own.  A pass takes what free HBM holds of the encoder's and the
// encryption's temporaries
static std::vector<Ct> queries_device(Context &cx, const DevRows &rows, const ChaChaKey *key, u64 nonce0) {
    if (key && !cx.d_pk) throw StateError("hydia: public key not loaded");
    const int dim = cx.prm.dim, Nh = cx.slots, np = key ? 2 : 1;
    const size_t poly = (size_t)cx.nQ * cx.N * sizeof(u64), elems = (size_t)np * cx.nQ * cx.N;
    // per probe: slots + complex work + coefficients (4 N doubles' worth), three sampled polynomials and their limbs, the output twice
    const double per_query = 32.0 * cx.N + (key ? 12.0 * cx.N + 3.0 * poly : 0.0) + 2.0 * np * poly + 8.0 * dim;
    size_t free_b = 0, total_b = 0;
    size_t pass = 1;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
        pass = (size_t)std::max(1.0, std::floor(0.5 * ((double)free_b + (double)cx.pool.bytes_cached) / per_query));
    pass = std::min({pass, rows.n, (size_t)4096});
    wait_for_producer(cx, rows.stream);
    double *d_q = (double *)cx.pool.get(sizeof(double) * pass * dim);
    double *d_slots = (double *)cx.pool.get(sizeof(double) * pass * Nh);
    u64 *d_out = cx.pool.get(sizeof(u64) * pass * elems);
    std::vector<Ct> out;
    out.reserve(rows.n);
    RowSource src;
    src.dev = &rows;
    src.normalise = 1;
    for (size_t q0 = 0; q0 < rows.n; q0 += pass) {
        const int Q = (int)std::min(pass, rows.n - q0);
        src.stage(cx, q0, (size_t)Q, d_q);
        hc::query_tile(cx.stream, d_q, Q, dim, Nh, d_slots);
        if (key) encrypt_device(cx, d_slots, Q, *key, nonce0 + q0, d_out);
        else encode_device(cx, d_slots, Q, d_out);
        for (int q = 0; q < Q; q++) {
            out.emplace_back(&cx, 1, np, cx.nQ, cx.delta);
            HIP_CHECK(hipMemcpyAsync(out.back().d, d_out + (size_t)q * elems, sizeof(u64) * elems, hipMemcpyDeviceToDevice, cx.stream));
        }
    }
    cx.sync();
    cx.pool.put(d_out);
    cx.pool.put((u64 *)d_slots);
    cx.pool.put((u64 *)d_q);
    return out;
}
std::vector<Ct> client_encrypt_queries_device(Context &cx, const DevRows &rows, const uint8_t seed[32], uint64_t nonce0) {
    const ChaChaKey key = make_key(seed);
    return queries_device(cx, rows, &key, nonce0);
}
std::vector<Ct> client_encode_queries_device(Context &cx, const DevRows &rows) { return queries_device(cx, rows, nullptr, 0); }

// Seeded queries: n probes (src: normalised host rows, or rows in device memory that k_rows_widen normalises) -> their c0 halves in
// host memory, c0_out [n][nQ][N]; probe i takes nonce0 + i.  queries_device's passes — ONE k_query_tile and ONE encrypt_sym_device over
// what free HBM holds of the encoder's temporaries, one sampled polynomial, its limbs and the output — then one copy out per pass.
// wire != nullptr: c0_out is the payload of a wire message (wire_format.h) — every pass's c0 goes through k_wire_pack and leaves the
// GPU packed, wire->off[nQ] words per probe
static void queries_seeded(Context &cx, const RowSource &src, size_t n, const ChaChaKey &key, const ChaChaKey &akey, u64 nonce0, u64 *c0_out,
                           const WireRows *wire = nullptr) {
    if (!cx.d_sk) throw StateError("hydia: secret key not loaded (seeded encryption is the secret-key holder's; hydia_encrypt_query takes the public key)");
    const int dim = cx.prm.dim, Nh = cx.slots;
    const size_t elems = (size_t)cx.nQ * cx.N, poly = elems * sizeof(u64);
    const double per_query = 32.0 * cx.N + 4.0 * cx.N + 2.0 * poly + 8.0 * dim;
    size_t free_b = 0, total_b = 0, pass = 1;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
        pass = (size_t)std::max(1.0, std::floor(0.5 * ((double)free_b + (double)cx.pool.bytes_cached) / per_query));
    pass = std::min({pass, n, (size_t)4096});
    double *d_q = (double *)cx.pool.get(sizeof(double) * pass * dim);
    double *d_slots = (double *)cx.pool.get(sizeof(double) * pass * Nh);
    u64 *d_out = cx.pool.get(pass * poly);
    const size_t packed = wire ? (size_t)wire->off[cx.nQ] : 0;  // words per probe on the wire
    u64 *d_packed = wire ? cx.pool.get(pass * packed * sizeof(u64)) : nullptr;
    for (size_t q0 = 0; q0 < n; q0 += pass) {
        const int Q = (int)std::min(pass, n - q0);
        src.stage(cx, q0, (size_t)Q, d_q);
        hc::query_tile(cx.stream, d_q, Q, dim, Nh, d_slots);
        encrypt_sym_device(cx, d_slots, Q, key, akey, nonce0 + q0, nonce0 + q0, d_out);
        if (wire) {
            cx.timer_begin("k_wire_pack");
            hc::wire_pack(cx.stream, cx.d_mod, cx.N, d_out, elems, 0, (size_t)Q, 1, cx.nQ, *wire, d_packed);
            cx.timer_end("k_wire_pack");
            HIP_CHECK(hipMemcpyAsync(c0_out + q0 * packed, d_packed, (size_t)Q * packed * sizeof(u64), hipMemcpyDeviceToHost, cx.stream));
        } else {
            HIP_CHECK(hipMemcpyAsync(c0_out + q0 * elems, d_out, (size_t)Q * poly, hipMemcpyDeviceToHost, cx.stream));
        }
        cx.sync();  // d_out is written again by the next pass; the caller's rows and c0_out are host memory
    }
    if (d_packed) cx.pool.put(d_packed);
    cx.pool.put(d_out);
    cx.pool.put((u64 *)d_slots);
    cx.pool.put((u64 *)d_q);
}
void client_encrypt_queries_seeded(Context &cx, const double *queries, size_t n, const uint8_t seed[32], const uint8_t a_seed[32], uint64_t nonce0,
                                   u64 *c0_out, const WireRows *wire) {
    const int dim = cx.prm.dim;
    std::vector<double> qn(queries, queries + n * (size_t)dim);
    for (size_t v = 0; v < n; v++) normalize(qn.data() + v * dim, dim);
    RowSource src;
    src.host = qn.data();
    queries_seeded(cx, src, n, make_key(seed), make_key(a_seed), nonce0, c0_out, wire);
}
void client_encrypt_queries_seeded_device(Context &cx, const DevRows &rows, const uint8_t seed[32], const uint8_t a_seed[32], uint64_t nonce0,
                                          u64 *c0_out, const WireRows *wire) {
    RowSource src;
    src.dev = &rows;
    src.normalise = 1;
    wait_for_producer(cx, rows.stream);
    queries_seeded(cx, src, rows.n, make_key(seed), make_key(a_seed), nonce0, c0_out, wire);
}
// the sender's side: handle i = (c0[i], a) with a limb j = the uniform stream (SYM_A, nonce0 + i, 0, j) under a_seed — the launch of
// sample_uniform whose thread k_enc_sym repeats — an ordinary fresh ciphertext [1][2][nQ][N] at scale 2^scale_bits
// (the same launch on its own, for a c0 that was unpacked from a wire message straight into its handle: dst = the handle's c1 [nQ][N])
void client_sample_query_a(Context &cx, const uint8_t a_seed[32], uint64_t nonce, u64 *dst) {
    hc::sample_uniform(cx.stream, make_key(a_seed), cx.d_mod, cx.N, HY_STREAM(HY_DOM_SYM_A, nonce, 0, 0), 1ull, 0, dst, (size_t)cx.N, 0,
                       cx.sel_q(cx.nQ), 1);
}
std::vector<Ct> client_expand_seeded(Context &cx, const u64 *c0, size_t n, const uint8_t a_seed[32], uint64_t nonce0) {
    const size_t elems = (size_t)cx.nQ * cx.N;
    const ChaChaKey akey = make_key(a_seed);
    const LimbSel qsel = cx.sel_q(cx.nQ);
    std::vector<Ct> out;
    out.reserve(n);
    for (size_t i = 0; i < n; i++) {
        out.emplace_back(&cx, 1, 2, cx.nQ, cx.delta);
        HIP_CHECK(hipMemcpyAsync(out.back().d, c0 + i * elems, elems * sizeof(u64), hipMemcpyHostToDevice, cx.stream));
        hc::sample_uniform(cx.stream, akey, cx.d_mod, cx.N, HY_STREAM(HY_DOM_SYM_A, nonce0 + i, 0, 0), 1ull, 0, out.back().d + elems,
                           (size_t)cx.N, 0, qsel, 1);
    }
    cx.sync();  // c0 is caller memory
    return out;
}

#define HY_HERS_NONCE_BASE (1ull << 37)
// HersEnroller::serializeDB (/root/reference/src/enroller/enroller_hers.cpp:40-93): normalise in place, then per matrix of
// `slots` vectors one ciphertext per dimension holding that coordinate of every vector
void client_hers_enroll(Context &cx, double *db, size_t n, const uint8_t seed[32]) {
    const int dim = cx.prm.dim, Nh = cx.slots;
    for (size_t v = 0; v < n; v++) normalize(db + v * dim, dim);
    const ChaChaKey key = make_key(seed);
    const size_t G = cx.db_cts / dim, ct_elems = (size_t)2 * cx.nQ * cx.N;
    double *d_rows = (double *)cx.pool.get(sizeof(double) * (size_t)Nh * dim);
    double *d_slots = (double *)cx.pool.get(sizeof(double) * (size_t)dim * Nh);
    u64 *d_cts = cx.pool.get(sizeof(u64) * (size_t)dim * ct_elems);
    for (size_t g = 0; g < G; g++) {
        const size_t first = g * (size_t)Nh;
        const size_t rows = n > first ? std::min((size_t)Nh, n - first) : 0;
        if (rows)
            HIP_CHECK(hipMemcpyAsync(d_rows, db + first * dim, sizeof(double) * rows * dim, hipMemcpyHostToDevice, cx.stream));
        hc::hers_pack(cx.stream, d_rows, (long long)rows, dim, Nh, d_slots);
        encrypt_device(cx, d_slots, dim, key, HY_HERS_NONCE_BASE + g * dim, d_cts);
        cx.db_store(g * dim, d_cts, dim);
    }
    cx.sync();
    cx.pool.put(d_cts);
    cx.pool.put((u64 *)d_slots);
    cx.pool.put((u64 *)d_rows);
}
#define HY_BASE_NONCE_BASE (3ull << 36)
// BaseEnroller::serializeDB (/root/reference/src/enroller/enroller_base.cpp:13-56): normalise in place, then database ciphertext t =
// vectors t vpc .. t vpc + vpc - 1 back to back, encrypted with nonce HY_BASE_NONCE_BASE + t straight into the resident kind-1 layout
void client_base_enroll(Context &cx, double *db, size_t n, const uint8_t seed[32]) {
    const int dim = cx.prm.dim, Nh = cx.slots;
    for (size_t v = 0; v < n; v++) normalize(db + v * dim, dim);
    const ChaChaKey key = make_key(seed);
    const size_t cts = cx.db_cts, ct_elems = (size_t)2 * cx.nQ * cx.N, elems = n * (size_t)dim;
    if (cts > HY_NONCE_LIMIT - HY_BASE_NONCE_BASE) throw std::runtime_error("hydia: the database exceeds the 2^40 nonce space of the encryption sampler");
    const size_t B = std::min<size_t>(cts, 16);  // ciphertexts encoded and encrypted per pass
    double *d_rows = (double *)cx.pool.get(sizeof(double) * B * Nh);
    double *d_slots = (double *)cx.pool.get(sizeof(double) * B * Nh);
    u64 *d_cts = cx.pool.get(sizeof(u64) * B * ct_elems);
    for (size_t t0 = 0; t0 < cts; t0 += B) {
        const size_t X = std::min(B, cts - t0), first = t0 * (size_t)Nh;
        const size_t have = elems > first ? std::min(X * (size_t)Nh, elems - first) : 0;
        if (have) HIP_CHECK(hipMemcpyAsync(d_rows, db + first, sizeof(double) * have, hipMemcpyHostToDevice, cx.stream));
        hc::row_pack(cx.stream, d_rows, (long long)have, Nh, d_slots, (int)X);
        encrypt_device(cx, d_slots, (int)X, key, HY_BASE_NONCE_BASE + t0, d_cts);
        cx.db_store(t0, d_cts, (int)X);
    }
    cx.sync();
    cx.pool.put(d_cts);
    cx.pool.put((u64 *)d_slots);
    cx.pool.put((u64 *)d_rows);
}
#define HY_BLIND_NONCE_BASE (1ull << 38)
// BlindEnroller::serializeDB (/root/reference/src/enroller/enroller_blind.cpp:13-90): normalise in place, then per matrix m of
// slots / chunk_len vectors the K = dim / chunk_len slot images of k_chunk_pack, encrypted with nonces HY_BLIND_NONCE_BASE + m K + c
// straight into the resident kind-3 layout (ciphertext t = m K + c)
void client_blind_enroll(Context &cx, double *db, size_t n, int chunk_len, const uint8_t seed[32]) {
    const int dim = cx.prm.dim, Nh = cx.slots, K = dim / chunk_len;
    for (size_t v = 0; v < n; v++) normalize(db + v * dim, dim);
    const ChaChaKey key = make_key(seed);
    const size_t cts = cx.db_cts, ct_elems = (size_t)2 * cx.nQ * cx.N, spb = (size_t)(Nh / chunk_len), M = cts / (size_t)K;
    if (cts > HY_NONCE_LIMIT - HY_BLIND_NONCE_BASE) throw std::runtime_error("hydia: the database exceeds the 2^40 nonce space of the encryption sampler");
    double *d_rows = (double *)cx.pool.get(sizeof(double) * spb * dim);
    double *d_slots = (double *)cx.pool.get(sizeof(double) * (size_t)K * Nh);
    u64 *d_cts = cx.pool.get(sizeof(u64) * (size_t)K * ct_elems);
    for (size_t m = 0; m < M; m++) {
        const size_t first = m * spb, rows = n > first ? std::min(spb, n - first) : 0;
        if (rows) HIP_CHECK(hipMemcpyAsync(d_rows, db + first * dim, sizeof(double) * rows * dim, hipMemcpyHostToDevice, cx.stream));
        hc::chunk_pack(cx.stream, d_rows, (long long)rows, dim, chunk_len, Nh, d_slots);
        encrypt_device(cx, d_slots, K, key, HY_BLIND_NONCE_BASE + m * (size_t)K, d_cts);
        cx.db_store(m * (size_t)K, d_cts, K);
    }
    cx.sync();
    cx.pool.put(d_cts);
    cx.pool.put((u64 *)d_slots);
    cx.pool.put((u64 *)d_rows);
}
// BlindReceiver::encryptQuery (/root/reference/src/receiver/receiver_blind.cpp:13-26, :58-71): normalise, then K = dim / chunk_len
// ciphertexts, ciphertext c = chunk c tiled over all slots, nonce nonce0 + c
Ct client_blind_encrypt_query(Context &cx, const double *query, int chunk_len, const uint8_t seed[32], uint64_t nonce0) {
    const int dim = cx.prm.dim, Nh = cx.slots, K = dim / chunk_len;
    std::vector<double> qn(query, query + dim);
    normalize(qn.data(), dim);
    double *d_q = (double *)cx.pool.get(sizeof(double) * (size_t)dim);
    double *d_slots = (double *)cx.pool.get(sizeof(double) * (size_t)K * Nh);
    HIP_CHECK(hipMemcpyAsync(d_q, qn.data(), sizeof(double) * dim, hipMemcpyHostToDevice, cx.stream));
    hc::chunk_tile(cx.stream, d_q, dim, chunk_len, Nh, d_slots);
    Ct out(&cx, K, 2, cx.nQ, cx.delta);
    encrypt_device(cx, d_slots, K, make_key(seed), nonce0, out.d);
    cx.sync();  // qn is a stack-owned buffer
    cx.pool.put((u64 *)d_slots);
    cx.pool.put((u64 *)d_q);
    return out;
}
// HersReceiver::encryptQuery (/root/reference/src/receiver/receiver_hers.cpp:13-24): vector_dim ciphertexts
Ct client_hers_encrypt_query(Context &cx, const double *query, const uint8_t seed[32], uint64_t nonce0) {
    const int dim = cx.prm.dim, Nh = cx.slots;
    std::vector<double> qn(query, query + dim);
    normalize(qn.data(), dim);
    double *d_q = (double *)cx.pool.get(sizeof(double) * (size_t)dim);
    double *d_slots = (double *)cx.pool.get(sizeof(double) * (size_t)dim * Nh);
    HIP_CHECK(hipMemcpyAsync(d_q, qn.data(), sizeof(double) * dim, hipMemcpyHostToDevice, cx.stream));
    hc::broadcast_rows(cx.stream, d_q, dim, Nh, d_slots);
    Ct out(&cx, dim, 2, cx.nQ, cx.delta);
    encrypt_device(cx, d_slots, dim, make_key(seed), nonce0, out.d);
    cx.sync();  // qn is a stack-owned buffer
    cx.pool.put((u64 *)d_slots);
    cx.pool.put((u64 *)d_q);
    return out;
}

}  // namespace hydia
