/*
 * include/hydia.h — C-ABI of libhydia.so: the MI355X-native drop-in for the HyDia (approach 5) path of
 * n7koirala/image_matching.  Plain pointers and sizes only; no torch / OpenFHE / C++ types cross this boundary.
 *
 * The reference has no FFI: its seam is the C++ virtual surface main.cpp programs against
 * (/root/reference/include/sender.h:19-43, include/receiver.h:17-43, include/enroller_diag.h:7-27), carrying OpenFHE
 * shared_ptr handles.  Each entry point below names the reference interface it replaces; INTEGRATION.md shows the
 * adapter a maintainer adds on the reference side.
 *
 * Data crossing the boundary:
 *   ciphertext  = uint64 residues, limb-major [poly][limb][N], EVALUATION form in bit-reversed order
 *                 (out[j] = a(psi^(2*bitrev(j)+1)) mod q_limb), limb j <-> modulus j of hydia_get_moduli();
 *                 what OpenFHE exposes as ct->GetElements()[p].GetElementAtIndex(j).GetValues() after
 *                 SetFormat(EVALUATION) when the moduli/roots agree (otherwise cross in COEFFICIENT form and
 *                 convert with hydia_ntt — INTEGRATION.md).
 *   eval key    = [digit][2][limb over Q then P][N] residues, poly 0 = b, poly 1 = a (hybrid key switching, dnum digits)
 *   slots       = IEEE doubles
 * All functions return 0 on success and a negative hydia_status otherwise; hydia_last_error() has the message
 * (the reference prints to cerr and carries on — src/sender/sender_diag.cpp:89-91 — callers that want that behaviour
 * ignore the code).  One host thread per context at a time; contexts are independent (one per GPU, or several per GPU) and
 * every entry point selects its context's GPU itself.  A context stays alive until its last hydia_ct handle is freed.
 */
#ifndef HYDIA_H
#define HYDIA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    HYDIA_OK = 0,
    HYDIA_ERR_ARG = -1,      /* bad argument / shape */
    HYDIA_ERR_STATE = -2,    /* missing key / database / wrong level */
    HYDIA_ERR_DEVICE = -3,   /* HIP failure (no GPU, out of memory, ...) */
    HYDIA_ERR_INTERNAL = -4
} hydia_status;

/* CKKS parameters — the knobs of /root/reference/src/main.cpp:169-173 plus VECTOR_DIM (include/config.h:30). */
typedef struct {
    uint32_t log_n;          /* 15  (HEStd_128_classic at this modulus size); 10 .. 16.  The small rings exist for tests.  At 10 a
                              * context serves the receiver's side only — keys, encryption, decryption, ciphertext handles — and
                              * key switching and a resident database answer HYDIA_ERR_ARG: they start at 11 */
    uint32_t mult_depth;     /* 11  = OpenFHEWrapper::computeRequiredDepth(5), src/openFHE_wrapper.cpp:37-40 */
    uint32_t scale_bits;     /* 45  SetScalingModSize */
    uint32_t first_mod_bits; /* 60  OpenFHE default first modulus */
    uint32_t dnum;           /* 3   OpenFHE default numLargeDigits (HYBRID) */
    uint32_t vector_dim;     /* 512 VECTOR_DIM */
} hydia_params;

typedef struct {
    uint32_t log_n, n, slots, n_q, n_p, dnum, alpha, vector_dim;
    double delta;            /* 2^scale_bits */
} hydia_info;

typedef struct hydia_ctx hydia_ctx;
typedef struct hydia_ct hydia_ct; /* a batch of >= 1 ciphertexts of identical shape, resident in HBM */

const char *hydia_last_error(void);
const char *hydia_version(void);

/* hydia_default_params: the context of ./ImageMatching <file> 5 (src/main.cpp:82, :169-173). */
void hydia_default_params(hydia_params *out);
/* Host-only parameter derivation (no GPU needed): moduli/roots are length n_q + n_p, Q limbs first. */
int hydia_params_describe(const hydia_params *p, hydia_info *info, uint64_t *moduli, uint64_t *roots);
/* OpenFHEWrapper::computeRequiredDepth, src/openFHE_wrapper.cpp:6-44 */
size_t hydia_compute_required_depth(size_t approach);
/* Host-only: the context ./ImageMatching <file> <approach> needs (src/main.cpp:169-173 with SetMultiplicativeDepth(
 * computeRequiredDepth(approach))): hydia_default_params with mult_depth = hydia_compute_required_depth(approach) and the smallest
 * log_n whose log2(QP) of the derived chain fits the HEStd_128_classic bound (54, 109, 218, 438, 881, 1772 bits at 2^11 .. 2^16) —
 * what OpenFHE selects.  Approaches 4 and 5 (depth 11, 795 bits): log_n 15 = hydia_default_params; approach 1 (depth 13: 14 Q limbs,
 * 5 special primes, 945 bits): log_n 16.  An approach outside 1..5: HYDIA_ERR_ARG. */
int hydia_params_for_approach(size_t approach, hydia_params *out);

/* replaces GenCryptoContext + Enable(...) (src/main.cpp:169-179) for the sender/receiver on GPU `device`.  No HIP device, or a
 * device index beyond the ones visible: HYDIA_ERR_DEVICE (a negative index: HYDIA_ERR_ARG) — there is no CPU fallback. */
int hydia_ctx_create(const hydia_params *p, int device, hydia_ctx **out);
/* Same, on a caller-supplied prime chain — the adapter path of SURVEY 8f-3: an OpenFHE context's ciphertext primes
 * (cc->GetElementParams()->GetParams()[j]->GetModulus(), q_0 first) followed by its special primes
 * (GetParamsP()), and optionally the 2N-th roots OpenFHE uses (GetRootOfUnity()) so evaluation-form data can cross the
 * boundary unconverted.  n_q = mult_depth + 1.  Every modulus must be a distinct prime < 2^60 that is 1 mod 2N; limbs
 * of at most 47 bits take the FP64 NTT path; limbs below 2^48 are stored packed in the database (46-bit residues in the
 * group-sequential layout when every limb but q_0 is below 2^46, 48-bit otherwise: hydia_db_residue_bits).
 * The fused key-switching pipeline (column-fused conversions) serves up to four special primes of any width — OpenFHE's choice for the
 * reference's parameter set — or five below 2^48; other counts run the same arithmetic through the unfused kernels (bit-identical, slower). */
int hydia_ctx_create_custom(const hydia_params *p, const uint64_t *moduli, const uint64_t *roots /* may be NULL */,
                            uint32_t n_q, uint32_t n_p, int device, hydia_ctx **out);
void hydia_ctx_destroy(hydia_ctx *ctx);
int hydia_get_info(const hydia_ctx *ctx, hydia_info *out);
int hydia_get_moduli(const hydia_ctx *ctx, uint64_t *moduli, uint64_t *roots);
int hydia_sync(hydia_ctx *ctx);
int hydia_memory_stats(hydia_ctx *ctx, uint64_t *pool_live, uint64_t *pool_cached, uint64_t *pool_peak);

/* ---- randomness.  Every seed below is a 32-byte ChaCha20 key; samples are addressed by (seed, nonce), so a (seed, nonce) pair
 * must NEVER be used for two different plaintexts (the two ciphertexts would differ by exactly the plaintext difference).
 * The reference draws OpenFHE's PRNG seed from the OS; callers that do not need reproducibility do the same with
 * hydia_random_seed (getrandom(2)).  Nonces are 40-bit: encryption calls refuse nonce (+ count) >= 2^40. */
int hydia_random_seed(uint8_t out[32]);

/* ---- keys: cc->KeyGen / EvalMultKeyGen / EvalRotateKeyGen (src/main.cpp:184-206) ---- */
/* generate sk, pk, relin key and rotation keys {1..dim-1} u {dim, 2dim, .., slots/2} on the GPU from a 32-byte seed */
int hydia_keygen(hydia_ctx *ctx, const uint8_t seed[32]);
/* the same sk, pk and relinearisation key, and rotation keys for exactly the rotations rots[0 .. n-1] (EvalRotateKeyGen with a list of
 * its own, src/main.cpp:195-206): each r is taken as r mod slots in [1, slots) — a negative rotation is the key of slots + r — and
 * r = 0 mod slots is HYDIA_ERR_ARG.  Rotation keys outside the set are released.  A key hydia_keygen also makes comes out bit-identical
 * to it.  Approach 1 needs {2^k} u {slots - 2^k} (29 keys at 2^16 where hydia_keygen's set would take ~30 GB). */
int hydia_keygen_rotations(hydia_ctx *ctx, const uint8_t seed[32], const int32_t *rots, uint32_t n);
/* or import keys produced elsewhere (the reference's serial/{multkey,rotkey}.bin contents after unmarshalling):
 * rot = 0 is the relinearisation key, rot >= 1 the key of EvalRotate(., rot); data [dnum][2][n_q+n_p][N] */
int hydia_import_eval_key(hydia_ctx *ctx, int rot, const uint64_t *data);
int hydia_export_eval_key(hydia_ctx *ctx, int rot, uint64_t *data);
int hydia_import_public_key(hydia_ctx *ctx, const uint64_t *data /* [2][n_q][N] (b, a) */);
int hydia_import_secret_key(hydia_ctx *ctx, const uint64_t *data /* [n_q+n_p][N], evaluation form */);
int hydia_export_public_key(hydia_ctx *ctx, uint64_t *data);
int hydia_export_secret_key(hydia_ctx *ctx, uint64_t *data);
int hydia_has_eval_key(hydia_ctx *ctx, int rot);
/* profiling filler: relin + rotation keys {1..dim-1} u {dim..slots/2 powers of two} of uniformly random residues
 * (kernel cost is data independent; results decrypt to noise) */
int hydia_fill_eval_keys_random(hydia_ctx *ctx, uint64_t seed);

/* ---- ciphertext handles (Ciphertext<DCRTPoly>) ---- */
int hydia_ct_import(hydia_ctx *ctx, const uint64_t *data, uint32_t count, uint32_t n_polys, uint32_t n_limbs,
                    double scale, hydia_ct **out);
int hydia_ct_export(hydia_ctx *ctx, const hydia_ct *ct, uint64_t *data);
int hydia_ct_shape(const hydia_ct *ct, uint32_t *count, uint32_t *n_polys, uint32_t *n_limbs, double *scale);
/* raw HBM address of the batch (for RCCL gathers through torch.distributed; layout [count][poly][limb][N]) */
int hydia_ct_device_ptr(const hydia_ct *ct, void **ptr, size_t *bytes);
/* device-to-device copy of the whole batch into caller-owned HBM (e.g. a torch tensor used as RCCL send buffer) */
int hydia_ct_copy_to_device(hydia_ctx *ctx, const hydia_ct *ct, void *dev_dst);
int hydia_ct_from_device(hydia_ctx *ctx, const void *dev_ptr, uint32_t count, uint32_t n_polys, uint32_t n_limbs,
                         double scale, hydia_ct **out); /* copies */
/* a handle over ciphertexts that STAY in the caller's device memory (no copy): the all-gathered rotations of a rotation-split loop A.
 * The memory must stay valid and unchanged while the handle, or work enqueued on it, is alive */
int hydia_ct_view_device(hydia_ctx *ctx, void *dev_ptr, uint32_t count, uint32_t n_polys, uint32_t n_limbs, double scale,
                         hydia_ct **out);
/* a handle over the first n_limbs limbs of ct, read in place: no copy, the limb stride stays ct's (what dropping limbs without a rescale
 * leaves).  ct must stay alive and unchanged while the handle or any operation enqueued on it is alive */
int hydia_ct_limb_prefix(hydia_ctx *ctx, const hydia_ct *ct, uint32_t n_limbs, hydia_ct **out);
void hydia_ct_free(hydia_ct *ct);

/* ---- receiver: DiagonalReceiver / HersReceiver ---- */
/* Receiver::encryptQuery, src/receiver/receiver_diag.cpp:13-26: normalise, tile to all slots, encode, encrypt */
int hydia_encrypt_query(hydia_ctx *ctx, const double *query /* vector_dim */, const uint8_t seed[32], uint64_t nonce,
                        hydia_ct **out);
/* OpenFHEWrapper::encryptFromVector, src/openFHE_wrapper.cpp:74-77 (count vectors of `slots` doubles each).
 * The encoder's range: the coefficients of the encoded polynomial are 64-bit integers, each the slot values' transform times
 * 2^scale_bits rounded half to even.  max|slot| * 2^scale_bits < 2^63 is sufficient: a coefficient is at most the mean absolute slot
 * value times the scale.  Beyond that range the residues are unspecified (the device conversion saturates where the CPU oracle's llrint
 * is undefined); no fault occurs */
int hydia_encrypt(hydia_ctx *ctx, const double *slots, uint32_t count, const uint8_t seed[32], uint64_t nonce0,
                  hydia_ct **out);
/* OpenFHEWrapper::decryptToVector, src/openFHE_wrapper.cpp:81-85: out = count * slots doubles */
int hydia_decrypt(hydia_ctx *ctx, const hydia_ct *ct, double *out);
/* HersReceiver::decryptMembership, src/receiver/receiver_hers.cpp:26-35: slot 0 >= 1.0 */
int hydia_decrypt_membership(hydia_ctx *ctx, const hydia_ct *ct, int *result);
/* HersReceiver::decryptIndex, src/receiver/receiver_hers.cpp:37-54: every slot >= 1.0 -> j + i*slots.
 * *n_out receives the number of matches; at most cap are written. */
int hydia_decrypt_index(hydia_ctx *ctx, const hydia_ct *cts, size_t *out, size_t cap, size_t *n_out);

/* ---- candidate lists and matches (an extension; the reference returns the comparator's booleans or every score).  A selection stage
 * behind the decoder, on the GPU: the decoded slots stay in device memory and only what was asked for crosses to the host — the k best
 * entries, or the entries at or above a threshold of the caller's choosing, never all slots.  Exact and deterministic: the same input
 * gives the same output on every run.
 * INDICES  index j + i * slots is slot j of ciphertext i: hydia_decrypt_index's rule, the order of hydia_decrypt's output.
 * MATCHES  (threshold select) the indices i with v[i] >= threshold in ASCENDING order, optionally with their values.  *n_out always
 *          receives the total count; at most cap entries are written.  The comparison is IEEE: -0.0 >= +0.0 holds, a NaN is never
 *          selected.  idx_out == NULL counts only.
 * TOP-K    the k largest values, by VALUE DESCENDING, TIES BY ASCENDING INDEX.  -0.0 ties with +0.0.  A NaN ranks below every number,
 *          after -inf; NaNs tie with each other by index.  k >= n returns all n; *n_out = min(k, n).
 * VALUES   bit for bit the doubles hydia_decrypt writes for those slots (val_out may be NULL).
 * n_vectors  the decrypt entries search the first n_vectors slots only: the padding slots of the last block decode to noise around 0 and
 *          would otherwise enter a top-k of negative scores.  0 = all count * slots; above that: HYDIA_ERR_ARG.
 * BATCHES  the *_multi entries take n_results results (each a batch handle of its own count), enqueue them on the context's stream
 *          result after result and read back after one synchronisation.  Row r of idx_out / val_out starts at r * cap (matches) or
 *          r * k (top-k); n_out has n_results entries.
 * DEVICE ARRAYS  hydia_decrypt_device leaves the decoded slots in the caller's device memory; the hydia_slots_* entries select from any
 *          array of n doubles there.  The memory must be ordinary device memory of the context's GPU, complete (not being written on
 *          another stream) at the call: host memory, another GPU or managed memory answers HYDIA_ERR_ARG.
 * REFUSALS (HYDIA_ERR_ARG, outputs untouched): k == 0, n == 0, n above 2^31 - 1, a null n_out, a null handle, a null idx_out for top-k.
 * TRUST    a receiver that asks for scores sees EVERY score, as with hydia_compute_similarity + hydia_decrypt today: these entries save
 *          work, they hide nothing.  The fixed-threshold boolean path (hydia_index_scenario, then hydia_decrypt_index) remains the one
 *          that reveals only matches.
 * hydia_decrypt_index is hydia_decrypt_matches at threshold 1.0 over all slots without values; hydia_decrypt_membership reads one double. */
int hydia_decrypt_device(hydia_ctx *ctx, const hydia_ct *ct, double *dev_out /* [count][slots], the context's GPU */);
int hydia_slots_select_device(hydia_ctx *ctx, const double *dev_vals, size_t n, double threshold, size_t *idx_out,
                              double *val_out /* may be NULL */, size_t cap, size_t *n_out);
int hydia_slots_topk_device(hydia_ctx *ctx, const double *dev_vals, size_t n, size_t k, size_t *idx_out, double *val_out /* may be NULL */,
                            size_t *n_out);
int hydia_decrypt_matches(hydia_ctx *ctx, const hydia_ct *cts, size_t n_vectors, double threshold, size_t *idx_out, double *val_out,
                          size_t cap, size_t *n_out);
int hydia_decrypt_topk(hydia_ctx *ctx, const hydia_ct *cts, size_t n_vectors, size_t k, size_t *idx_out, double *val_out, size_t *n_out);
int hydia_decrypt_matches_multi(hydia_ctx *ctx, const hydia_ct *const *results, uint32_t n_results, size_t n_vectors, double threshold,
                                size_t *idx_out /* [n_results][cap] */, double *val_out, size_t cap, size_t *n_out /* [n_results] */);
int hydia_decrypt_topk_multi(hydia_ctx *ctx, const hydia_ct *const *results, uint32_t n_results, size_t n_vectors, size_t k,
                             size_t *idx_out /* [n_results][k] */, double *val_out, size_t *n_out /* [n_results] */);

/* ---- enroller: DiagonalEnroller ---- */
/* number of DB ciphertexts for n vectors (concatenateRows, src/enroller/enroller_diag.cpp:120-122) */
size_t hydia_db_num_cts(const hydia_ctx *ctx, size_t n_vectors);
/* DiagonalEnroller::serializeDB, src/enroller/enroller_diag.cpp:12-53: normalises db IN PLACE (like the reference),
 * diagonalises, encodes and encrypts straight into the HBM-resident layout (no serial/db_diagonal files).
 * For a multi-GPU database each rank enrols its own contiguous range of 16384-vector blocks (multi-GPU). */
int hydia_db_enroll(hydia_ctx *ctx, double *db /* n x vector_dim row-major */, size_t n, const uint8_t seed[32]);
/* One shard of a database that is cut by 16384-vector row-blocks over several contexts (multi-GPU): `db` holds only
 * this shard's rows and first_block is the index of its first block in the whole database, so the shard encrypts with exactly
 * the nonces the unsharded enrolment uses for those blocks (bit-identical ciphertexts). */
int hydia_db_enroll_shard(hydia_ctx *ctx, double *db, size_t n, const uint8_t seed[32], size_t first_block);
/* ---- in-place update of a resident diagonal database (kind 5 or 6): append, remove, replace rows.
 * ONE primitive: a FRESH encryption of the sparse diagonal image of rows[n][vector_dim], placed at vectors first_vector ..
 * first_vector + n - 1, is added to the resident ciphertexts of the blocks those vectors touch (residue by residue, mod q_j); every
 * other block is not read, not written and not re-encrypted.  With slots = N / 2 and n_old = the resident vector count:
 *   normalise != 0  every row is normalised IN PLACE like hydia_db_enroll's (a zero row passes through); 0 takes the rows as given
 *   first_vector <= n_old (no holes); afterwards the database holds max(n_old, first_vector + n) vectors
 *   a block that existed: ciphertext g vector_dim + i becomes old + E; a block the update creates: it becomes E — bit-identical to
 *     that block of hydia_db_enroll_shard on the same rows with the same seed.  E = the encryption of the block's sparse image (in the
 *     resident form: pre-rotated when hydia_db_babies < vector_dim) under `seed` with the ENROLMENT's nonce of that ciphertext.
 *   append   first_vector = n_old, normalise = 1 (the padding slots of a ragged last block hold encryptions of zero: adding is appending)
 *   remove   the NEGATED template at its index, normalise = 1 (a negated unit vector normalises to itself); the slot then holds 0 up to noise
 *   replace  new_normalised - old_normalised at the index, normalise = 0
 * The kind and the form (hydia_db_babies) stay what they are — hydia_set_matvec's auto policy is NOT re-run for the new block count —
 * and the database lies afterwards where an enrolment of the new size in that form would put it: growing past 8 blocks moves a hoisted
 * database from the ciphertext-major 48-bit layout to the group-sequential 46-bit one (hydia_db_group, hydia_db_residue_bits).  An
 * update that adds blocks needs a second buffer of the NEW size for its duration; when that does not fit: HYDIA_ERR_DEVICE and the
 * database is untouched.  A sender or receiver object built for the old vector count is rebuilt by the caller for the new one.
 * NOISE: every update adds one fresh encryption's noise (about 2^-30 of the scale) to the blocks it touches; after k updates of one
 * block its noise is that of a sum of k + 1 fresh ciphertexts — re-enrol a block that has seen many thousands.
 * SEED: the seed of an update MUST NEVER HAVE BEEN USED ON THIS DATABASE BEFORE — not by its enrolment, not by an earlier update.  The
 * nonces are the enrolment's, so a reused seed encrypts a changed plaintext under the same randomness and the difference of the two
 * ciphertexts reveals the difference of the plaintexts.  Take every update's seed from hydia_random_seed.
 * Errors: no database, or kind 1 / 3 / 4: HYDIA_ERR_STATE; first_vector > n_old, null seed, or null rows with n > 0: HYDIA_ERR_ARG;
 * n == 0: HYDIA_OK and nothing changes.  hydia_db_update_shard: this context holds the blocks first_block .. of a larger database
 * (first_vector counts within the shard); it is what a multi-GPU wrapper would call on the rank that owns the rows. */
int hydia_db_update(hydia_ctx *ctx, size_t first_vector, double *rows /* n x vector_dim row-major */, size_t n, int normalise, const uint8_t seed[32]);
int hydia_db_update_shard(hydia_ctx *ctx, size_t first_vector, double *rows, size_t n, int normalise, const uint8_t seed[32], size_t first_block);
/* ---- re-keying a resident database in place under a NEW receiver key (kinds 4, 5 and 6; no counterpart in the reference, which
 * re-enrols from the plaintext templates).  The receiver's key expires, is suspected lost or passes to another custodian: the NEW
 * receiver makes one switching key from the old secret to its own, and the sender key-switches every resident ciphertext with it.
 *   hydia_keygen_switch   on the NEW receiver's context (it needs that context's secret; without one: HYDIA_ERR_STATE).  old_secret is
 *                         the OLD receiver's secret [n_q+n_p][N] in evaluation form, as hydia_export_secret_key gives it.  key_out
 *                         [dnum][2][n_q+n_p][N] (hydia_switch_key_words() words), evaluation form, laid out as hydia_export_eval_key
 *                         lays keys out: digit d holds (b_d, a_d) = (-a_d s_new + e_d + P [limb in digit d] s_old, a_d) — exactly the
 *                         key of a rotation without its automorphism.  Its sampler streams are the evaluation keys' with the reserved
 *                         key id HY_EVK_ID_SWITCH (rotation ids are below slots <= 2^15, relinearisation is 0, the field is 40 bits
 *                         wide: nothing collides).  The context's own keys are not changed.
 *   hydia_db_rekey        on the SENDER's context: every resident ciphertext (c0, c1), on all n_q limbs, becomes (c0 + ks0, ks1) with
 *                         (ks0, ks1) the hybrid key switch of c1 under switch_key (ModUp per digit, inner product, ModDown; no
 *                         automorphism).  Scale, limb count, ciphertext order, layout (hydia_db_group, hydia_db_residue_bits), kind
 *                         and form (hydia_db_babies) all stay; the stored residues are canonical.  The key is uploaded to a
 *                         temporary buffer and released at the end: the context's own evaluation keys are neither read nor changed,
 *                         so a context that shares another's keys, or one shard of a group (hydia_group_ctx: call it on every
 *                         shard with the same key), is served like any other.  The database is walked in chunks of at most 256
 *                         ciphertexts, sized from free device memory.
 * TRUST MODEL: the sender learns neither secret.  The switching key is a proxy re-encryption key from the old key to the new one:
 * whoever holds it can turn ANY ciphertext under the old key into one under the new key, so treat it like an evaluation key (the new
 * receiver makes it, the sender uses it and may discard it afterwards).  Making it needs BOTH secrets in one place for the duration of
 * hydia_keygen_switch — the hand-over between custodians.  Use a FRESH seed (hydia_random_seed) for every switching key.
 * NOISE: every re-key adds one key switch's noise (that of one rotation, far below the scale) to every ciphertext.
 * AFTERWARDS the caller imports the NEW receiver's relinearisation / rotation keys (hydia_import_eval_key) and public key into the
 * sender, queries are encrypted under the new public key, and every later hydia_db_update encrypts under the NEW public key — a
 * re-keyed database no longer opens under the old secret.
 * Errors, all BEFORE any work is enqueued and with the database untouched: no database, kinds 1 and 3, and a plain gallery (kinds 7 /
 * 8: nothing is encrypted) answer HYDIA_ERR_STATE with a message naming the kind; a null key HYDIA_ERR_ARG.  A device error in
 * mid-pass (HYDIA_ERR_DEVICE) leaves a MIXED database — the chunks already stored are under the new key, the rest under the old one;
 * there is no way to tell them apart afterwards: enrol again, or restore a saved file (hydia_db_load) and re-key that. */
#define HY_EVK_ID_SWITCH (1ull << 24)
int hydia_keygen_switch(hydia_ctx *ctx, const uint64_t *old_secret /* [n_q+n_p][N] */, const uint8_t seed[32], uint64_t *key_out);
int hydia_db_rekey(hydia_ctx *ctx, const uint64_t *switch_key /* [dnum][2][n_q+n_p][N] */);
size_t hydia_switch_key_words(const hydia_ctx *ctx);
/* hydia_db_rekey with the chunk capped at max_chunk ciphertexts (0 = no cap): for tests of the chunk boundaries; same result */
int hydia_db_rekey_chunked(hydia_ctx *ctx, const uint64_t *switch_key, int max_chunk);
/* ---- the split of the diagonalised mat-vec.  With rotation i = b + B g: B - 1 hoisted ("baby") rotations of the
 * query per QUERY, vector_dim / B relinearised partial sums per BLOCK of which all but the first are rotated by B g ("giant" steps,
 * ordinary key switches with the rotation keys B, 2B, .. that src/main.cpp:195-206 already generates).  The enroller rotates
 * diagonal i by -B (i div B) slots in the clear; ciphertext order and nonces do not change.
 *   B = vector_dim      "hoisted": the reference's own form (src/sender/sender_diag.cpp:22-26), no pre-rotation, no giant step
 *   B = 32 (dim 512)    "bsgs": the classic square-root split BASELINE.json's north_star names
 *   any power of two dividing vector_dim in between
 * Decrypted results agree within CKKS noise (1e-4 on scores) whatever B; ciphertexts are bit-identical between runs with the same B.
 * hydia_set_matvec mode: 0 auto (hydia_auto_babies: B grows with the blocks the enrolling context holds — at vector_dim 512: 64 up
 * to 3 blocks, 128 up to 12, 256 up to 40, hoisted above; measured, profiles/r04/matvec_sweep.txt), 1 hoisted, otherwise B itself; initial value from HYDIA_MATVEC=auto|hoisted|bsgs|<B>.
 * It takes effect at the NEXT enrolment; hydia_db_kind / hydia_db_babies tell what is resident (kind 0 none, 5 hoisted diagonals,
 * 6 pre-rotated diagonals, 4 HERS columns, 1 the rows of approach 1 — hydia_base_db_enroll, 3 the chunks of approach 3 — hydia_blind_db_enroll,
 * 7 a plain gallery's hoisted diagonals and 8 its pre-rotated ones — hydia_plain_db_enroll; hydia_db_babies answers for kinds 5 to 8).  Ciphertexts imported one by one (hydia_db_alloc + hydia_db_import_ct: the reference
 * enroller's) are taken as hoisted unless hydia_db_set_babies says otherwise (a database of more than 8 blocks is then re-ordered in
 * HBM for the declared form, through a second buffer of its size — see hydia_db_group).  hydia_db_set_babies takes a DECLARED form:
 * vector_dim (hoisted) or a power of two >= 2 dividing it — 0, 1 and anything else are HYDIA_ERR_ARG; without a diagonal database
 * HYDIA_ERR_STATE; when the second buffer does not fit HYDIA_ERR_DEVICE, and the database, its layout and its form are untouched. */
int hydia_set_matvec(hydia_ctx *ctx, int mode);
int hydia_get_matvec(const hydia_ctx *ctx);
int hydia_db_kind(const hydia_ctx *ctx);
int hydia_db_babies(const hydia_ctx *ctx);
int hydia_db_set_babies(hydia_ctx *ctx, int babies);
int hydia_auto_babies(const hydia_ctx *ctx, size_t blocks); /* what an enrolment of `blocks` blocks on this context would pick */
/* hydia_db_enroll_shard with an explicit split (0 = the context's policy, 1 = hoisted, else B): a sharded enrolment passes ONE
 * decision to every shard */
int hydia_db_enroll_shard_ex(hydia_ctx *ctx, double *db, size_t n, const uint8_t seed[32], size_t first_block, int matvec);
/* or load ciphertexts produced elsewhere: t = block*vector_dim + diagonal, i.e. serial/db_diagonal/index<t>.bin
 * (src/enroller/enroller_diag.cpp:161; read back at src/sender/sender_diag.cpp:87-91) */
int hydia_db_alloc(hydia_ctx *ctx, size_t n_vectors);
int hydia_db_import_ct(hydia_ctx *ctx, size_t t, const uint64_t *data /* [2][n_q][N] */);
int hydia_db_export_ct(hydia_ctx *ctx, size_t t, uint64_t *data);
/* ---- plain gallery (database kinds 7 / 8): an encrypted query against UNENCRYPTED templates.  An extension with no counterpart in
 * the reference, for the deployment where the operator of the sender owns the gallery (a watchlist, an access list) and only the
 * probe is private.  TRUST MODEL:
 *   - the sender SEES the gallery: the templates lie in its memory as encoded plaintexts;
 *   - the query and every result stay encrypted under the receiver's key — the receiver, the query, the keys and the decrypt rules
 *     are exactly those of an encrypted database;
 *   - no circuit privacy is claimed, as before: a result ciphertext may reveal more about the gallery than the scores it decrypts to.
 * Plaintext t = block * vector_dim + diagonal is the slot image hydia_db_enroll makes for ciphertext t (pre-rotated when
 * hydia_db_babies < vector_dim), encoded at scale 2^scale_bits on all n_q limbs, in evaluation form, as ONE polynomial [n_q][N] of
 * canonical residues — no seed, no nonce, no public key.  The gallery lies where a ciphertext database of the same block count and
 * form lies (hydia_db_group, hydia_db_residue_bits) with one polynomial per entry: hydia_db_stats reports the count of plaintexts
 * and half the bytes.  Loop B forms the two components c_p * m directly (no third component), so hydia_compute_similarity on a plain
 * gallery needs NO relinearisation key; the comparator of the scenarios still does.
 *   hydia_plain_db_enroll     normalises db IN PLACE like hydia_db_enroll, follows hydia_set_matvec exactly as an encrypted
 *                             enrolment does (hydia_auto_babies' thresholds were measured on encrypted databases and are
 *                             unmeasured for this kind), replaces the resident database
 *   hydia_plain_db_alloc      room for n_vectors in a DECLARED form: babies = vector_dim, or a power of two >= 2 dividing it (else
 *                             HYDIA_ERR_ARG); every plaintext starts as the zero polynomial
 *   hydia_plain_db_import_pt  a residue at or above its q_j: HYDIA_ERR_ARG, nothing written; without a plain gallery HYDIA_ERR_STATE
 * Served on a plain gallery, by dispatch on the resident kind: hydia_compute_similarity, hydia_index_scenario,
 * hydia_membership_scenario, hydia_rotate_query, hydia_db_kind / _babies / _stats / _group / _residue_bits; batches of queries by
 * entry points of their own, hydia_*_gallery_multi (below, after hydia_*_multi).
 * In-place updates and files have entry points of their own: hydia_plain_db_update, hydia_plain_db_save / hydia_plain_db_load (below).
 * NOT served yet — each answers HYDIA_ERR_STATE with a message naming the plain gallery, before any work is enqueued and with the
 * gallery untouched: hydia_*_multi, hydia_*_rotated, hydia_rotate_query_range*, hydia_db_import_ct, hydia_db_export_ct,
 * hydia_db_set_babies, and the ciphertext database's hydia_db_update* and hydia_db_save (their messages name hydia_plain_db_update /
 * hydia_plain_db_save); there is no hydia_group_* enrolment of a plain gallery, and hydia_plain_db_enroll / hydia_plain_db_alloc /
 * hydia_plain_db_load on a context that is a shard of a group (hydia_group_ctx) answer HYDIA_ERR_STATE the same way.  hydia_db_load of a
 * ciphertext file, like any enrolment, replaces the gallery. */
int hydia_plain_db_enroll(hydia_ctx *ctx, double *db /* n x vector_dim row-major */, size_t n);
int hydia_plain_db_alloc(hydia_ctx *ctx, size_t n_vectors, int babies);
int hydia_plain_db_import_pt(hydia_ctx *ctx, size_t t, const uint64_t *data /* [n_q][N] */);
int hydia_plain_db_export_pt(hydia_ctx *ctx, size_t t, uint64_t *data);
/* In-place update of a resident plain gallery: hydia_db_update's one primitive without seed and nonce.  With n_old the resident vector
 * count: normalise != 0 normalises every row IN PLACE like hydia_plain_db_enroll, 0 takes the rows as given; first_vector <= n_old (no
 * holes); afterwards the gallery holds max(n_old, first_vector + n) vectors.  Per block touched by vectors first_vector ..
 * first_vector + n - 1 the sparse slot image of the rows at their slots (pre-rotated when hydia_db_babies < vector_dim) is encoded as
 * hydia_plain_db_enroll encodes, giving E_t for plaintext t = block * vector_dim + diagonal:
 *   a block that existed:        plaintext t := (old_t + E_t) mod q_j, residue by residue, stored canonical;
 *   a block the update creates:  plaintext t := E_t — bit for bit that block of hydia_plain_db_enroll on the same rows;
 *   every other block is neither read nor written.
 * Append: first_vector = n_old, normalise = 1.  Remove: the negated template at its index.  Replace: new_normalised - old_normalised
 * with normalise = 0.  Kind and form stay; the gallery lies afterwards where an enrolment of the new size in that form would put it
 * (growing a hoisted gallery past 8 blocks moves it from ciphertext-major 48-bit to group-sequential 46-bit residues, a grown
 * group-sequential gallery may get another group size, a pre-rotated gallery counts (block, giant step) pairs).  Growth needs a second
 * buffer for its duration: when it does not fit the call answers HYDIA_ERR_DEVICE before anything is touched.
 * ROUNDING: the encoder rounds once per update.  encode(a) + encode(b) differs from encode(a + b) by at most 1 per coefficient before
 * the transform — about 2^-45 of the scale per update — so an updated existing block is NOT bit-identical to a fresh enrolment of the
 * same rows.
 * THE EXACT INVERSE: the encoder rounds symmetrically, encode(-x) + encode(x) = 0 mod q_j in every residue.  The same rows negated, at
 * the same first_vector with the same normalise, restore every plaintext of a block that existed bit for bit; blocks the first call
 * created become zero polynomials, and the vector count stays grown.  Removing one row out of several added in one call leaves at
 * most the rounding residue above.
 * Errors, all before any launch and with the gallery untouched: no database resident or a ciphertext database: HYDIA_ERR_STATE (for
 * kinds 5 / 6 the message names hydia_db_update); first_vector > n_old, null rows with n > 0, or a row count that overflows:
 * HYDIA_ERR_ARG; n == 0: HYDIA_OK and nothing changes.  It orders itself against queries in flight as hydia_db_update does. */
int hydia_plain_db_update(hydia_ctx *ctx, size_t first_vector, double *rows /* n x vector_dim row-major */, size_t n, int normalise);
/* Persistence of a plain gallery in hydia_db_save's streaming format: the same header with kind 7 / 8 and the baby count, n_cts = the
 * number of plaintexts, ct_bytes = the bytes of ONE plaintext in the ciphertext-major layout of the context's packing; then the
 * plaintexts in order, ciphertext-major (a group-sequential gallery is converted on the way).  hydia_plain_db_save without a plain
 * gallery: HYDIA_ERR_STATE.  hydia_plain_db_load checks the header before anything is allocated or the resident database is touched,
 * each failure HYDIA_ERR_ARG: parameters, prime chain, packing, a valid baby count for kind 8, n_cts equal to what n_vectors implies,
 * the exact file size (neither truncated nor with trailing bytes); a ciphertext file is refused with a message naming hydia_db_load, as
 * hydia_db_load refuses a plain-gallery file naming hydia_plain_db_load.  The file is UNTRUSTED and nothing authenticates a plaintext:
 * every residue is checked on the device while the file streams in, and a residue at or above its q_j — found in mid-load, like a
 * short read — answers HYDIA_ERR_ARG and leaves NO database resident (kind 0, zero counts): the load is not transactional.  A loaded
 * gallery takes the form the file declares, whatever hydia_set_matvec says.  On a shard of a group: HYDIA_ERR_STATE. */
int hydia_plain_db_save(hydia_ctx *ctx, const char *path);
int hydia_plain_db_load(hydia_ctx *ctx, const char *path);
/* Persistence of the enrolled database (the reference keeps one serial/db_diagonal/index<t>.bin per ciphertext,
 * src/enroller/enroller_diag.cpp:158-166, and re-reads them every query; here the database stays in HBM and a file is only
 * what a server restart needs).  Own streaming format: a header (parameters, prime chain, packing) + the ciphertexts in order, each
 * as its packed residues (the ciphertext-major resident layout verbatim; a group-sequential database is converted on the way);
 * hydia_db_load refuses a file written for other parameters / primes / residue width.
 * A row-packed database (kind 1, approach 1) is NOT saved: the header's `packed` word states how the 45-bit limbs of EVERY ciphertext
 * in the file are stored and is checked against the context's own packing on load, while kind 1 is resident as plain 8-byte residues
 * whatever the context packs — hydia_db_save answers HYDIA_ERR_STATE for it, and no file carries kind 1. */
int hydia_db_save(hydia_ctx *ctx, const char *path);
int hydia_db_load(hydia_ctx *ctx, const char *path);
/* benchmark filler: n_vectors worth of uniformly random residues (the kernels' cost is data independent) */
int hydia_db_fill_random(hydia_ctx *ctx, size_t n_vectors, uint64_t seed);
int hydia_db_stats(const hydia_ctx *ctx, size_t *n_vectors, size_t *n_cts, size_t *bytes);
/* How the resident database lies in HBM: 0 = ciphertext after ciphertext; g > 0 = group-sequential, the layout a hoisted database of
 * more than 8 blocks takes — the bytes one loop-B workgroup reads (one 128-coefficient tile of one limb of g blocks) form one
 * sequential run, which HBM serves at 7.0 TB/s instead of 6.05.  Transparent to every entry point
 * (hydia_db_import_ct / hydia_db_export_ct address ciphertexts, hydia_db_save writes the ciphertext-major file format whatever the
 * resident layout); HYDIA_DB_CT_MAJOR=1 at context creation keeps every database ciphertext-major. */
int hydia_db_group(const hydia_ctx *ctx);
/* bits per stored residue of the 45/46-bit limbs of the resident database: 46 (group-sequential layout: 128 residues in a 736-byte
 * unit; round 4), 48 (6-byte residues: ciphertext-major layout, HYDIA_DB_48BIT, files) or 64 (HYDIA_DB_UNPACKED); 0 without a database.
 * Limb 0 (60 bit) always takes 8 bytes.  hydia_db_stats reports the bytes this makes resident. */
int hydia_db_residue_bits(const hydia_ctx *ctx);

/* ---- sender: DiagonalSender (src/sender/sender_diag.cpp) ---- */
/* loop A alone (:20-26): the vector_dim rotated queries, rot[0] = q */
int hydia_rotate_query(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out);
/* Sender::computeSimilarity (:12-33): one score ciphertext per 16384-vector block, level 1 */
int hydia_compute_similarity(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out);
/* Sender::indexScenario (:52-63) */
int hydia_index_scenario(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out);
/* Loop A split over the GPUs of a node (the `#pragma omp parallel for` over i of src/sender/sender_diag.cpp:23-26, cut into ranges):
 * rotations first .. first+count-1 of the query (rotation 0 = the query itself) written to dev_dst [count][2][n_q][N]; the ranges of
 * all ranks, all-gathered into one [vector_dim][2][n_q][N] buffer, are what hydia_rotate_query returns — and what the *_rotated
 * forms of computeSimilarity / indexScenario take instead of the query (a hydia_ct_view_device over the gathered buffer) */
int hydia_rotate_query_range(hydia_ctx *ctx, const hydia_ct *query, uint32_t first, uint32_t count, hydia_ct **out);
int hydia_rotate_query_range_into(hydia_ctx *ctx, const hydia_ct *query, uint32_t first, uint32_t count, void *dev_dst);
int hydia_compute_similarity_rotated(hydia_ctx *ctx, const hydia_ct *rotations, hydia_ct **out);
int hydia_index_scenario_rotated(hydia_ctx *ctx, const hydia_ct *rotations, hydia_ct **out);
/* Sender::membershipScenario (:35-50) */
int hydia_membership_scenario(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out);
/* Q independent queries against the resident database in one pass (an extension: the reference serves one query per
 * call).  queries[q] as hydia_encrypt_query returns it; out[q] receives exactly what the single-query entry returns for
 * queries[q], bit for bit, and is freed on its own.  On any error every out[q] is NULL. */
int hydia_compute_similarity_multi(hydia_ctx *ctx, const hydia_ct *const *queries, uint32_t n_queries, hydia_ct **out);
int hydia_index_scenario_multi(hydia_ctx *ctx, const hydia_ct *const *queries, uint32_t n_queries, hydia_ct **out);
int hydia_membership_scenario_multi(hydia_ctx *ctx, const hydia_ct *const *queries, uint32_t n_queries, hydia_ct **out);
/* The same for a PLAIN GALLERY (database kinds 7 / 8; hydia_*_multi above keep answering HYDIA_ERR_STATE on one): n_queries encrypted
 * queries share passes over the gallery, out[q] receives exactly what the single-query entry returns for queries[q] on that gallery,
 * bit for bit, and is freed on its own.  On any error every out[q] is NULL, nothing has been enqueued and the gallery is as it was:
 * an empty batch, a NULL handle, a query that is not one fresh 2-component ciphertext at full level, unequal scales: HYDIA_ERR_ARG;
 * a ciphertext database of kind 5 / 6 (its batches are hydia_*_multi's), any other kind, no database, a shard context of a group, a
 * key the scenario needs that is not loaded (the single entry's message): HYDIA_ERR_STATE. */
int hydia_compute_similarity_gallery_multi(hydia_ctx *ctx, const hydia_ct *const *queries, uint32_t n_queries, hydia_ct **out);
int hydia_index_scenario_gallery_multi(hydia_ctx *ctx, const hydia_ct *const *queries, uint32_t n_queries, hydia_ct **out);
int hydia_membership_scenario_gallery_multi(hydia_ctx *ctx, const hydia_ct *const *queries, uint32_t n_queries, hydia_ct **out);
/* UNSTABLE, for measurements and tests only (tools/bench_plain_gallery.py --batch).  The queries one pass over the gallery of a
 * *_gallery_multi call serves on this context, 1, 2 or 4; 0 = the library's choice (the default).  The results do not depend on it.
 * Another value: HYDIA_ERR_ARG. */
int hydia_set_gallery_batch_width(hydia_ctx *ctx, uint32_t width);
/* ---- plain query: a KNOWN probe against the ENCRYPTED database (kinds 5 / 6).  An extension with no counterpart in the reference,
 * for the deployment where the operator of the sender produces the probe itself (it runs the cameras or the door) and the gallery
 * belongs to someone else (an agency's watchlist, another company's staff list).  TRUST MODEL:
 *   - the sender SEES the probe: it lies in its memory as an encoded plaintext;
 *   - the gallery and every result stay encrypted under the receiver's key — enrolment, the database layouts, the receiver and the
 *     decrypt rules are exactly those of an encrypted query;
 *   - no circuit privacy is claimed, as before: a result ciphertext may reveal more about the probe than the scores it decrypts to.
 * A hydia_pt is ONE encoded polynomial [n_q][N], evaluation form, canonical residues, resident in HBM; a type of its own, so no
 * ciphertext entry point can be handed one.  A context stays alive until its last hydia_pt is freed, as for hydia_ct.
 *   hydia_encode_query   exactly the plaintext hydia_encrypt_query encrypts: normalise, tile to all slots, encode at 2^scale_bits on
 *                        all n_q limbs — no seed, no nonce, no public key
 *   hydia_pt_import      for adapters and tests; a residue at or above its q_j: HYDIA_ERR_ARG, nothing is created
 * The *_pq entries return what the encrypted-query entries return (the same count, limbs, scale and block order): bit for bit the
 * sender's path on the trivial ciphertext (m, 0).  Rotating a plaintext is a permutation and plaintext x ciphertext has two
 * components, so rotation keys 1 .. vector_dim-1 are never looked at and nothing is relinearised per block: hydia_compute_similarity_pq
 * on a hoisted database needs NO evaluation key at all.  A key that IS needed and missing answers HYDIA_ERR_STATE naming it, before
 * any work is enqueued: the relinearisation key (the comparator of the scenarios), a giant-step key B g (kind 6), a power-of-two key
 * (the EvalSum of membership).
 * Served on kinds 5 and 6 only.  A plain gallery (kind 7 / 8) answers HYDIA_ERR_STATE: with both sides in the clear nothing would be
 * private.  No database, or kinds 1 / 3 / 4: HYDIA_ERR_STATE.  NOT served: caller-supplied rotations, hydia_group_*.
 * The *_pq_multi entries serve n_queries plain queries in one pass over the database, with the output convention of hydia_*_multi:
 * out[q] receives exactly what the single *_pq entry returns for queries[q], bit for bit, and is freed on its own; on any error every
 * out[q] is NULL.  Every refusal is made for every query before any work is enqueued and leaves the database as it was: an empty
 * batch, a NULL handle, a plaintext not at full level, unequal scales: HYDIA_ERR_ARG; what the single entry refuses (a plain gallery,
 * no database or another kind, a missing key): HYDIA_ERR_STATE with the single entry's message. */
typedef struct hydia_pt hydia_pt;
int hydia_encode_query(hydia_ctx *ctx, const double *query /* vector_dim */, hydia_pt **out);
int hydia_pt_import(hydia_ctx *ctx, const uint64_t *data /* [n_q][N] */, double scale, hydia_pt **out);
int hydia_pt_export(hydia_ctx *ctx, const hydia_pt *pt, uint64_t *data);
void hydia_pt_free(hydia_pt *pt);
int hydia_compute_similarity_pq(hydia_ctx *ctx, const hydia_pt *query, hydia_ct **out);
int hydia_index_scenario_pq(hydia_ctx *ctx, const hydia_pt *query, hydia_ct **out);
int hydia_membership_scenario_pq(hydia_ctx *ctx, const hydia_pt *query, hydia_ct **out);
int hydia_compute_similarity_pq_multi(hydia_ctx *ctx, const hydia_pt *const *queries, uint32_t n_queries, hydia_ct **out);
int hydia_index_scenario_pq_multi(hydia_ctx *ctx, const hydia_pt *const *queries, uint32_t n_queries, hydia_ct **out);
int hydia_membership_scenario_pq_multi(hydia_ctx *ctx, const hydia_pt *const *queries, uint32_t n_queries, hydia_ct **out);
/* UNSTABLE, for measurements and tests only (tools/bench_plain_query.py --batch): not part of the interface an integration should
 * rely on, and it may change or go without notice.  The queries one database pass of a *_pq_multi call serves on this context, 1, 2
 * or 4; 0 = the library's measured choice (the default).  The results do not depend on it.  Another value: HYDIA_ERR_ARG. */
int hydia_set_pq_batch_width(hydia_ctx *ctx, uint32_t width);
/* ---- templates already in device memory (an extension; no counterpart in the reference).  A template usually leaves an embedding
 * network as an f16 / bf16 / f32 tensor on the GPU that will enrol or match it; these entries take it where it lies.  A
 * hydia_dev_rows describes n rows of vector_dim elements, row_stride elements apart (row_stride >= vector_dim; elements of a row are
 * contiguous).  The rows are widened exactly to doubles and normalised on the device, bit for bit as the host entry points normalise
 * (divide by the L2 norm, squared sum in index order, a zero row passes through), so each *_device entry leaves exactly what its host
 * twin leaves when handed the widened rows: the same ciphertexts under the same seed, the same plaintexts, the same form
 * (hydia_set_matvec).  NaN and infinite elements follow IEEE arithmetic as on the host.
 * Ordering and lifetime: `stream` is the hipStream_t on which the rows were produced.  The library records an event on it and makes
 * its own stream wait — no host synchronisation on the way in; whatever is enqueued on `stream` AFTER the call begins is not waited
 * for.  stream == NULL: the caller guarantees that the rows are complete.  The rows are only ever read, never written (a host entry
 * point normalises its array in place; these do not), must stay valid and unchanged during the call, and may be reused or freed when
 * it returns: every call is synchronous on return.
 * Refusals, all made before anything is launched and leaving the resident database as it was: ptr is not device memory, or lies on
 * another GPU than the context's, or is not aligned to its element type; row_stride < vector_dim; a dtype out of range: HYDIA_ERR_ARG.
 * A context that is a shard of a hydia_group: HYDIA_ERR_STATE.  Otherwise what the host twin refuses, with its message (no public key;
 * an update with no database or the wrong kind resident).  n == 0: an enrolment answers HYDIA_ERR_ARG and an update HYDIA_OK, as the
 * host entries do; the two query entries answer HYDIA_ERR_ARG.
 *   hydia_rows_widen_device       the kernel alone: dev_dst [n][vector_dim] doubles in device memory of the same GPU
 *   hydia_encrypt_queries_device  out[i] = hydia_encrypt_query(row i, seed, nonce0 + i), bit for bit; nonce0 + n <= 2^40
 *   hydia_encode_queries_device   out[i] = hydia_encode_query(row i), bit for bit
 * Both make all n queries with one encoder / encryption pass per batch (batches sized from free device memory) and return n handles,
 * each freed on its own; on any error every out[i] is NULL.
 * NOT served: approaches 1 - 4, hydia_db_enroll_shard* and hydia_group_*, integer templates. */
typedef enum { HYDIA_F64 = 0, HYDIA_F32 = 1, HYDIA_F16 = 2, HYDIA_BF16 = 3 } hydia_dtype;
typedef struct {
    const void *ptr;    /* device memory of the context's GPU; never written */
    hydia_dtype dtype;
    size_t n;           /* rows */
    size_t row_stride;  /* elements between rows, >= vector_dim */
    void *stream;       /* hipStream_t that produced the rows, or NULL */
} hydia_dev_rows;
int hydia_rows_widen_device(hydia_ctx *ctx, const hydia_dev_rows *rows, int normalise, double *dev_dst /* [n][vector_dim] */);
int hydia_db_enroll_device(hydia_ctx *ctx, const hydia_dev_rows *rows, const uint8_t seed[32]);
int hydia_plain_db_enroll_device(hydia_ctx *ctx, const hydia_dev_rows *rows);
int hydia_db_update_device(hydia_ctx *ctx, size_t first_vector, const hydia_dev_rows *rows, int normalise, const uint8_t seed[32]);
int hydia_plain_db_update_device(hydia_ctx *ctx, size_t first_vector, const hydia_dev_rows *rows, int normalise);
int hydia_encrypt_queries_device(hydia_ctx *ctx, const hydia_dev_rows *rows, const uint8_t seed[32], uint64_t nonce0, hydia_ct **out /* n handles */);
int hydia_encode_queries_device(hydia_ctx *ctx, const hydia_dev_rows *rows, hydia_pt **out /* n handles */);
/* ---- seeded keys and queries (an extension; no counterpart in the reference): the uniform half of every key and of every query
 * travels as the 32-byte seed it is the expansion of.  Half of an evaluation key (every [d][1] row), of the public key (a) and of a
 * ciphertext made by the holder of the secret (c1) is uniform; the sampler is addressed by (seed, stream, block), so the other side
 * regenerates those halves on its GPU, bit for bit.  At the default parameters an evaluation key shrinks from 25 165 824 to
 * 12 582 912 bytes and a query from 6 291 456 to 3 145 728 (+ 32 bytes of seed and the nonce).
 * CONTRACT
 *   a_seed is PUBLIC and travels with the data.  Draw it from hydia_random_seed, independently of `seed`: a_seed == seed (32 equal
 *     bytes) would publish the seed of the secret key and of every error term, and is refused with HYDIA_ERR_ARG before anything is
 *     touched.
 *   For one secret key a pair (a_seed, nonce) MUST NEVER ENCRYPT TWO QUERIES: the two c0 would differ by exactly the plaintext
 *     difference plus noise.  This is the (seed, nonce) rule above, applied to the public seed as well.
 *   One a_seed may cover a whole key set (the streams are addressed by key id), and it may also be the one used for queries (the
 *     stream domains differ).
 *   Seeded encryption needs the SECRET key: it is for the receiver of the reference's roles.  A client of a plain gallery that holds
 *     only the public key keeps hydia_encrypt_query.
 *   Noise: one fresh Gaussian (e0), lower than the public-key path's (e0 + e1 s + u e_pk).  No circuit privacy is claimed, as before.
 * KEYS, receiver side
 *   hydia_keygen_seeded / hydia_keygen_rotations_seeded   exactly hydia_keygen / hydia_keygen_rotations, except that every uniform
 *     half is sampled under a_seed at the unchanged stream addresses; the secret and every Gaussian error stay under seed, so the
 *     secret key is the one hydia_keygen(seed) makes.  The context remembers a_seed (hydia_get_key_seed; HYDIA_ERR_STATE when no
 *     seeded set was made) and marks every key generated this way; any other writer of a key (hydia_import_eval_key,
 *     hydia_import_public_key, hydia_fill_eval_keys_random, hydia_keygen, hydia_keygen_rotations, the *_seeded imports below) clears
 *     that key's mark.
 *   hydia_export_eval_key_seeded    the [d][0] halves of key `rot`, [dnum][n_q+n_p][N] (hydia_eval_key_seeded_words() words)
 *   hydia_export_public_key_seeded  b, [n_q][N].  Both answer HYDIA_ERR_STATE for a key that is not marked.
 * KEYS, sender side
 *   hydia_import_eval_key_seeded / hydia_import_public_key_seeded   upload the b halves into their places and expand the a halves on
 *     the GPU under a_seed; afterwards hydia_export_eval_key / hydia_export_public_key give the receiver's full key bit for bit, and
 *     everything that follows a key write follows as for hydia_import_eval_key.  Residues are NOT range-checked, as in
 *     hydia_import_eval_key.  The imported key is not marked seeded on the importing context.
 * QUERIES
 *   hydia_encrypt_query_seeded             c0 = NTT(e0 + m) - a s into HOST memory c0_out [n_q][N].  m is exactly the plaintext
 *     hydia_encrypt_query encrypts; e0 is its error e0 (under the secret seed, at `nonce`); a limb j is the uniform stream
 *     (domain 9, nonce, 0, j) under a_seed.  a never reaches memory on the receiver.
 *   hydia_encrypt_queries_seeded           count probes (count x vector_dim, not written), probe i with nonce0 + i, c0_out
 *     [count][n_q][N]; batches sized from free device memory.
 *   hydia_encrypt_queries_seeded_device    the same from rows in device memory (hydia_dev_rows above); c0_out is host memory
 *   hydia_ct_expand_seeded                 on the SENDER: out[i] = the ciphertext (c0[i], a(a_seed, nonce0 + i)), two polynomials on
 *     n_q limbs at scale 2^scale_bits — an ordinary hydia_ct that every single, *_multi, *_gallery_multi, *_rotated and group entry
 *     point takes unchanged, each freed on its own.  c0 is not range-checked.
 *   Errors: no secret key on the encrypting context: HYDIA_ERR_STATE.  nonce0 + count > 2^40, a null pointer, a_seed == seed:
 *     HYDIA_ERR_ARG.  count == 0: HYDIA_OK and nothing is written.
 * NOT seeded: the switching key of hydia_db_rekey, hydia_group_keygen, approaches 1 - 4, a LOCAL database enrolment or update
 * (hydia_db_enroll*, hydia_db_update).  An enrolment or update that is SHIPPED to a sender is: "seeded database deltas" below. */
int hydia_keygen_seeded(hydia_ctx *ctx, const uint8_t seed[32], const uint8_t a_seed[32]);
int hydia_keygen_rotations_seeded(hydia_ctx *ctx, const uint8_t seed[32], const uint8_t a_seed[32], const int32_t *rots, uint32_t n);
int hydia_get_key_seed(const hydia_ctx *ctx, uint8_t out[32]);
size_t hydia_eval_key_seeded_words(const hydia_ctx *ctx);
int hydia_export_eval_key_seeded(hydia_ctx *ctx, int rot, uint64_t *b_out /* [dnum][n_q+n_p][N] */);
int hydia_export_public_key_seeded(hydia_ctx *ctx, uint64_t *b_out /* [n_q][N] */);
int hydia_import_eval_key_seeded(hydia_ctx *ctx, int rot, const uint64_t *b /* [dnum][n_q+n_p][N] */, const uint8_t a_seed[32]);
int hydia_import_public_key_seeded(hydia_ctx *ctx, const uint64_t *b /* [n_q][N] */, const uint8_t a_seed[32]);
int hydia_encrypt_query_seeded(hydia_ctx *ctx, const double *query /* vector_dim */, const uint8_t seed[32], const uint8_t a_seed[32],
                               uint64_t nonce, uint64_t *c0_out /* [n_q][N] host */);
int hydia_encrypt_queries_seeded(hydia_ctx *ctx, const double *queries /* count x vector_dim */, size_t count, const uint8_t seed[32],
                                 const uint8_t a_seed[32], uint64_t nonce0, uint64_t *c0_out /* [count][n_q][N] host */);
int hydia_encrypt_queries_seeded_device(hydia_ctx *ctx, const hydia_dev_rows *rows, const uint8_t seed[32], const uint8_t a_seed[32],
                                        uint64_t nonce0, uint64_t *c0_out /* [n][n_q][N] host */);
int hydia_ct_expand_seeded(hydia_ctx *ctx, const uint64_t *c0 /* [count][n_q][N] host */, size_t count, const uint8_t a_seed[32],
                           uint64_t nonce0, hydia_ct **out /* count handles */);
/* ---- wire messages (an extension; the reference ships OpenFHE's serialised files, serial/multkey.bin, rotkey.bin and one file per
 * ciphertext — INTEGRATION.md maps them): ONE packed, checked, self-describing format for everything that crosses between receiver,
 * sender and enroller: ciphertext batches, seeded queries, evaluation keys and the public key, whole or seeded.  Residues travel in the
 * bit length of their modulus instead of 64 bits; packing happens on the GPU on the way out, unpacking and range-checking on the GPU on
 * the way in.  THE WIRE ENTRIES ARE THE CHECKED PATH: the raw-limb calls above (hydia_ct_import, hydia_import_eval_key,
 * hydia_ct_expand_seeded, ...) stay what they are, unchecked, for callers that bind OpenFHE objects directly.
 * At the default parameters (q_0 and the four special primes 60 bits, six limbs 46 and five 45) a seeded query message is 2 298 216 bytes
 * against 3 145 728 raw, a seeded evaluation key 9 843 048 against 12 582 912, a whole one 19 685 736 against 25 165 824.
 * NOT AUTHENTICATED: a message carries no MAC and is not encrypted beyond what a ciphertext is; transport security is the caller's.  What
 * the library guarantees is that a message it accepts is well-formed and canonical (every residue below its modulus).
 * FORMAT (little-endian; big-endian hosts are not served).  A message is a 360-byte header followed by the payload, nothing after it.
 *   header   offset 0 magic "HYDWIRE1" | 8 u32 version = 1 | 12 u32 type | 16 u32 log_n | 20 u32 n_polys | 24 u32 n_limbs | 28 u32 rot |
 *            32 u64 count | 40 f64 scale | 48 u8 a_seed[32] | 80 u64 nonce0 | 88 u64 payload_bytes | 96 u64 reserved = 0 |
 *            104 u64 moduli[32]: the moduli of the limbs carried, in order, then zeros
 *   type     1 ciphertext batch (n_polys 2 or 3, n_limbs 1 .. n_q) | 2 seeded query batch (one polynomial c0 per query on n_q limbs, scale
 *            2^scale_bits; c1 of query i = the expansion of (a_seed, nonce0 + i)) | 3 evaluation key (count = dnum, n_polys 2 = (b, a),
 *            n_limbs = n_q + n_p) | 4 seeded evaluation key (n_polys 1: the [d][0] rows) | 5 public key (count 1, n_polys 2, n_limbs n_q) |
 *            6 seeded public key (b alone)
 *   rot      types 3 / 4: the key id, 0 = relinearisation, otherwise in [1, slots); every other type 0
 *   unused   a field a type does not use is zero and is checked: scale (keys), a_seed (types 1, 3, 5), nonce0 (all but 2), moduli past
 *            n_limbs, reserved
 *   payload  rows in the order [count][poly][limb], each the N residues of one limb.  w_j = the bit length of q_j (60 and 45 / 46 at the
 *            default parameters); residue c occupies bits [c w_j, (c + 1) w_j) of the row read as one little-endian bit string; a row is
 *            N w_j / 8 bytes — N is a multiple of 64, so 64 consecutive residues make exactly w_j 64-bit words — and rows follow one
 *            another without padding.  payload_bytes = count x n_polys x sum_j N w_j / 8.
 *   seeded types carry only the half that is not the seed's expansion; the other half is regenerated on import exactly as
 *            hydia_ct_expand_seeded / hydia_import_eval_key_seeded / hydia_import_public_key_seeded do.
 *   key-set file   16 bytes (magic "HYDKEYS1", u32 version = 1, u32 number of messages), then the messages back to back: the public key
 *            first, then the evaluation keys in ascending key id.
 * VALIDATION happens on the header alone, before anything is allocated or any key or handle is touched; each refusal is HYDIA_ERR_ARG
 * with a message naming the field: magic, version, an unknown type, len shorter than a header, len != 360 + payload_bytes (neither
 * truncated nor trailing bytes), payload_bytes other than the shape implies (all size arithmetic is overflow-checked), log_n other than
 * the context's, count == 0, n_polys, n_limbs outside 1 .. n_q (ciphertexts) or other than n_q + n_p (keys), dnum, rot outside
 * [0, slots), a listed modulus that is not the context's modulus of that limb, scale not finite or <= 0, nonce0 + count > 2^40, a
 * non-zero unused field.  Then the packed bytes are uploaded and every residue is checked on the device while it is unpacked: one at or
 * above its modulus answers HYDIA_ERR_ARG, no handle is returned, no key is changed and nothing stays allocated.
 *   hydia_wire_peek        the context-free part of the validation, without a GPU (like hydia_params_describe): type, shape, rot, scale,
 *                          seed, nonce and bytes of the message at (buf, len)
 *   hydia_wire_*_bytes     the size of a message of that shape on this context; 0 for a shape no message has
 *   hydia_ct_to_wire       any handle, a hydia_ct_limb_prefix view included -> a type 1 message.  cap too small (or buf NULL):
 *                          HYDIA_ERR_ARG with *written = the bytes needed; otherwise *written = the bytes written
 *   hydia_ct_from_wire     type 1 -> ONE batch handle with the message's shape and scale; type 2 -> count single-ciphertext handles,
 *                          exactly those hydia_ct_expand_seeded makes.  out_cap too small: HYDIA_ERR_ARG with *n_out = the handles needed
 *   hydia_encrypt_queries_seeded_wire / _wire_device   hydia_encrypt_queries_seeded / _device with c0 leaving the GPU packed, as one type 2
 *                          message; refusals as theirs (count == 0: HYDIA_OK, *written = 0)
 *   hydia_key_to_wire      rot = -1 the public key, 0 the relinearisation key, r >= 1 the key of rotation r.  seeded != 0 on a key that is
 *                          not marked seeded: HYDIA_ERR_STATE, as the seeded exports answer
 *   hydia_key_from_wire    installs whichever key the message carries (rot_out: its id, -1 the public key), expanding seeded halves.  The
 *                          rows are unpacked into scratch and installed only after the check passed: a refused message leaves the key
 *                          installed before, and its seeded mark, untouched.  What follows a key write follows as for hydia_import_eval_key
 *   hydia_keys_save / hydia_keys_load   the key-set file of every key the context holds, through one pinned staging buffer.  A refused load
 *                          names the message index; the load is NOT transactional: keys of earlier messages stay installed.
 * NOT served: hydia_pt handles, the switching key of hydia_db_rekey, hydia_group_*, the database files (they keep their own format). */
typedef struct {
    uint32_t type, log_n, n_polys, n_limbs, rot, reserved;
    uint64_t count;
    double scale;
    uint8_t a_seed[32];
    uint64_t nonce0, header_bytes, payload_bytes;
} hydia_wire_info;
int hydia_wire_peek(const void *buf, size_t len, hydia_wire_info *out);
size_t hydia_wire_ct_bytes(const hydia_ctx *ctx, uint64_t count, uint32_t n_polys, uint32_t n_limbs, int seeded);
size_t hydia_wire_eval_key_bytes(const hydia_ctx *ctx, int seeded);
size_t hydia_wire_public_key_bytes(const hydia_ctx *ctx, int seeded);
int hydia_ct_to_wire(hydia_ctx *ctx, const hydia_ct *ct, void *buf, size_t cap, size_t *written);
int hydia_ct_from_wire(hydia_ctx *ctx, const void *buf, size_t len, hydia_ct **out, size_t out_cap, size_t *n_out);
int hydia_encrypt_queries_seeded_wire(hydia_ctx *ctx, const double *queries /* count x vector_dim */, size_t count, const uint8_t seed[32],
                                      const uint8_t a_seed[32], uint64_t nonce0, void *buf, size_t cap, size_t *written);
int hydia_encrypt_queries_seeded_wire_device(hydia_ctx *ctx, const hydia_dev_rows *rows, const uint8_t seed[32], const uint8_t a_seed[32],
                                             uint64_t nonce0, void *buf, size_t cap, size_t *written);
int hydia_key_to_wire(hydia_ctx *ctx, int rot, int seeded, void *buf, size_t cap, size_t *written);
int hydia_key_from_wire(hydia_ctx *ctx, const void *buf, size_t len, int *rot_out);
int hydia_keys_save(hydia_ctx *ctx, const char *path, int seeded);
int hydia_keys_load(hydia_ctx *ctx, const char *path);
/* ---- database deltas (an extension; the reference's enroller writes serial/db_diagonal/index<t>.bin for the sender to read —
 * INTEGRATION.md maps them): the enroller-to-sender hand-off as a checked message of CIPHERTEXTS.
 * TRUST MODEL: the enroller holds the templates and the receiver's PUBLIC key and nothing else; the sender holds the encrypted
 * database and never sees a template.  hydia_db_update needs both on one context.  A delta cuts it in two: hydia_db_delta_make, on the
 * ENROLLER's context, makes the fresh encryption E of the rows' sparse diagonal image that hydia_db_update would add (public key only:
 * no secret key, no evaluation key, no database — one that happens to be resident is neither read nor written);
 * hydia_db_delta_apply, on the SENDER's context, adds E to the resident blocks (database only: no key, no plaintext).  The database
 * is afterwards BIT FOR BIT what hydia_db_update(first_vector, rows, n, normalise, seed) leaves on it.  With no database resident a
 * delta at first_vector = 0 ENROLS: the result is bit for bit hydia_db_enroll_shard_ex's on the same rows, seed, first_block and form.
 * NOT AUTHENTICATED, like every wire message: whoever can hand the sender a delta can change its database; transport security is
 * the caller's.  What the library guarantees is that a delta it accepts is well-formed and canonical and that a refused one changes
 * nothing.
 * SEED: the seed of a delta MUST NEVER HAVE BEEN USED ON THIS DATABASE BEFORE — not by its enrolment, not by an earlier update or
 * delta.  The nonces are the enrolment's, so a reused seed encrypts a changed plaintext under the same randomness and the difference
 * of the two ciphertexts reveals the difference of the plaintexts.  Take every delta's seed from hydia_random_seed.
 * FORMAT (little-endian).  NOT a wire type — a container of its own, like the key-set file: a 64-byte header, then n_blocks ordinary
 * type 1 (ciphertext batch) wire messages back to back, nothing after the last.
 *   header   offset 0 magic "HYDDELT1" | 8 u32 version = 1 | 12 u32 vector_dim | 16 u64 babies: the form of the target database,
 *            vector_dim (hoisted) or a power of two >= 2 dividing it | 24 u64 first_vector | 32 u64 n_rows | 40 u64 first_block
 *            (recorded for diagnosis: the nonce offset the maker used) | 48 u64 n_blocks | 56 u64 reserved = 0
 *   message b is block first_vector / slots + b: count = vector_dim, n_polys = 2, n_limbs = n_q, scale = 2^scale_bits; ciphertext i of
 *            it is E for database ciphertext block * vector_dim + i.
 * At the default parameters a block's message is 2 353 004 904 bytes against 2 390 753 280 resident (group-sequential, 46-bit);
 * hydia_db_save would ship the whole database for every change.
 * VALIDATION reads the container header and the 360-byte headers of the messages only, before anything is allocated or uploaded,
 * with overflow-checked arithmetic; each refusal is HYDIA_ERR_ARG with a message naming the field: magic, version, reserved,
 * vector_dim, babies, n_rows == 0, n_blocks other than the blocks first_vector .. first_vector + n_rows - 1 touch, a message that
 * fails the wire validation against the context or is not of exactly the shape above, a total length that is not exact (truncated, or
 * bytes after the last message).
 *   hydia_db_delta_bytes   the size of a delta for rows first_vector .. first_vector + n - 1 on this context (host arithmetic only);
 *                          n == 0 or a size that overflows: HYDIA_ERR_ARG
 *   hydia_db_delta_peek    the context-free part of the validation, without a GPU: the header fields and the total bytes
 *   hydia_db_delta_make    normalise as in hydia_db_update (rows normalised IN PLACE); babies = the form of the target database
 *                          (hydia_db_babies of the sender's; vector_dim = hoisted); first_block = the nonce offset (0 unless the target
 *                          is a shard that holds blocks first_block .. of a larger database).  No public key: HYDIA_ERR_STATE.  n == 0,
 *                          a bad babies, a null argument, first_block + blocks beyond the nonce space, or cap too small (*len = the bytes
 *                          needed): HYDIA_ERR_ARG with nothing written.  Otherwise *len = the bytes written.  One block is in flight
 *                          on the device at a time
 *   hydia_db_delta_make_device   the same from rows in device memory (hydia_dev_rows above); the rows are never written
 *   hydia_db_delta_apply   a ciphertext database (kind 5 / 6) resident: babies must be hydia_db_babies and first_vector <= n_old
 *                          (HYDIA_ERR_ARG otherwise); blocks that existed become old + E mod q_j, stored canonical, new blocks become
 *                          E; growth as in hydia_db_update (the layout may change; no room: HYDIA_ERR_DEVICE); the vector count
 *                          becomes max(n_old, first_vector + n_rows).  NO database resident: first_vector must be 0 (HYDIA_ERR_STATE
 *                          otherwise) and the database is created in the form the delta declares.  A plain gallery (kind 7 / 8; the
 *                          message names hydia_plain_db_update) or kinds 1, 3, 4: HYDIA_ERR_STATE naming the kind.
 *                          TRANSACTIONAL AGAINST BAD INPUT: every header and every residue of every block is checked (on the device,
 *                          k_wire_check) before the first byte of the database is written or the database is grown; a residue at or
 *                          above its modulus anywhere: HYDIA_ERR_ARG, and the database, its layout, form and counts stay exactly as they
 *                          were.  The packed blocks are uploaded twice, one at a time: device memory beyond the database is one packed
 *                          block however many the delta holds.  It orders itself against queries in flight as hydia_db_update does.
 * NOT served: plain galleries and approaches 1 - 4, hydia_group_* (a shard context is served like any other; first_block exists for
 * it), a streaming file form. */
typedef struct {
    uint32_t version, vector_dim;
    uint64_t babies, first_vector, n_rows, first_block, n_blocks, total_bytes;
} hydia_db_delta_info;
int hydia_db_delta_bytes(const hydia_ctx *ctx, size_t first_vector, size_t n, size_t *bytes);
int hydia_db_delta_peek(const void *buf, size_t len, hydia_db_delta_info *out);
int hydia_db_delta_make(hydia_ctx *ctx, size_t first_vector, double *rows /* n x vector_dim row-major */, size_t n, int normalise,
                        const uint8_t seed[32], int babies, size_t first_block, void *buf, size_t cap, size_t *len);
int hydia_db_delta_make_device(hydia_ctx *ctx, size_t first_vector, const hydia_dev_rows *rows, int normalise, const uint8_t seed[32],
                               int babies, size_t first_block, void *buf, size_t cap, size_t *len);
int hydia_db_delta_apply(hydia_ctx *ctx, const void *buf, size_t len);
/* ---- seeded database deltas (an extension): the delta of an enroller that holds the SECRET key — half the bytes.
 * Under the secret key c1 of a fresh encryption is the uniform polynomial a, the expansion of a 32-byte public seed, so only c0 travels:
 * at the default parameters a block's message is 1 176 502 632 bytes against 2 353 004 904, 0.50 of the unseeded delta.  The maker
 * samples one polynomial and runs one transform batch per ciphertext where hydia_db_delta_make takes three of each; the sender
 * regenerates a on its GPU straight into the resident layout (k_db_accumulate_seeded / k_db_store_seeded: no 64-bit image of either
 * component in device memory).
 * TRUST MODEL: the ENROLLER's context now holds the SECRET key and the templates — this is for an owner who is both enroller and
 * receiver and has its own gallery matched on someone else's GPU.  An enroller that holds only the receiver's public key keeps
 * hydia_db_delta_make.  The SENDER still never sees a template and needs no key at all to apply.
 * SEEDS: two, and they must differ.  `seed` is secret and addresses the noise e0 at the enrolment's nonces; its rule stays the one of
 * hydia_db_update and "database deltas" above: never used on this database before.  `a_seed` is PUBLIC and travels in every message.
 * For one secret key a pair (a_seed, nonce) MUST NEVER ENCRYPT TWO PLAINTEXTS, and database ciphertexts and seeded queries share
 * stream domain 9: a delta's a_seed must never have been used for a QUERY under that key, and never for ANOTHER DELTA on that database
 * (nor for its enrolment).  Take every one from hydia_random_seed.
 * NOT AUTHENTICATED, like every delta.  Noise: one fresh Gaussian e0 — lower than the public-key path's e0 + e1 s + u e_pk; the noise of
 * a key switch is not involved.
 * FORMAT (little-endian): a container of its own next to "HYDDELT1", NOT a wire type (hydia_wire_peek keeps refusing type 7 and up).
 *   header   the 64 bytes of a delta header, same fields at the same offsets, under magic "HYDDELS1", version 1
 *   then n_blocks ordinary type 2 (seeded query batch) wire messages back to back, nothing after the last.  Message b is block
 *            first_vector / slots + b: count = vector_dim, n_polys = 1, n_limbs = n_q, scale = 2^scale_bits, a_seed = the delta's,
 *            nonce0 = (first_block + block) * vector_dim.  Ciphertext i of it is E = (c0_i, a(a_seed, nonce0 + i)), expanded exactly as
 *            hydia_ct_expand_seeded expands a query: hydia_ct_from_wire of one block's message yields the block's ciphertexts.
 * VALIDATION as for a delta (container header and the 360-byte message headers only, overflow-checked, HYDIA_ERR_ARG naming the
 * field), and beyond it: type is 2, n_polys is 1, every message carries one a_seed, nonce0 of message b is (first_block + block) *
 * vector_dim, nonce0 + count is below 2^40.  The two containers refuse each other by the magic: hydia_db_delta_apply_seeded and
 * hydia_db_delta_seeded_peek name hydia_db_delta_apply for a "HYDDELT1" buffer; hydia_db_delta_apply / hydia_db_delta_peek refuse
 * a "HYDDELS1" buffer as a bad magic.
 *   hydia_db_delta_seeded_bytes   the size for rows first_vector .. first_vector + n - 1 on this context (host arithmetic only)
 *   hydia_db_delta_seeded_peek    the context-free part of the validation, without a GPU
 *   hydia_db_delta_make_seeded    arguments as hydia_db_delta_make, plus a_seed.  Per touched block: the update's diag_pack, ONE
 *                          secret-key encryption pass (e0 under seed at the enrolment's nonce, a under a_seed; c1 is never written)
 *                          and k_wire_pack of c0; one block in flight on the device at a time.  No secret key: HYDIA_ERR_STATE.
 *                          a_seed == seed, n == 0, a bad babies, a null argument, nonces beyond 2^40, or cap too small (*len = the
 *                          bytes needed): HYDIA_ERR_ARG with nothing written
 *   hydia_db_delta_make_seeded_device   the same from rows in device memory; the rows are never written
 *   hydia_db_delta_apply_seeded   targets, growth and refusals as hydia_db_delta_apply (kinds 5 and 6; nothing resident: first_vector
 *                          must be 0; a plain gallery and kinds 1, 3, 4: HYDIA_ERR_STATE naming the kind; babies must be
 *                          hydia_db_babies).  Needs no key.  TRANSACTIONAL AGAINST BAD INPUT: every header and every c0 residue of
 *                          every block is range-checked (k_wire_check) before the database is grown or a byte is written; a is
 *                          canonical by construction.  The packed c0 blocks are uploaded twice, one at a time: device memory beyond
 *                          the database is one packed HALF block.  Ordered against queries in flight as hydia_db_update is.
 * The result is bit for bit what hydia_db_delta_apply of the type 1 messages holding the expanded ciphertexts leaves.
 * NOT served: a local hydia_db_update / hydia_db_enroll under the secret key, plain galleries, approaches 1 - 4, hydia_group_*, a
 * streaming file form. */
int hydia_db_delta_seeded_bytes(const hydia_ctx *ctx, size_t first_vector, size_t n, size_t *bytes);
int hydia_db_delta_seeded_peek(const void *buf, size_t len, hydia_db_delta_info *out);
int hydia_db_delta_make_seeded(hydia_ctx *ctx, size_t first_vector, double *rows /* n x vector_dim row-major */, size_t n, int normalise,
                               const uint8_t seed[32], const uint8_t a_seed[32], int babies, size_t first_block, void *buf, size_t cap,
                               size_t *len);
int hydia_db_delta_make_seeded_device(hydia_ctx *ctx, size_t first_vector, const hydia_dev_rows *rows, int normalise,
                                      const uint8_t seed[32], const uint8_t a_seed[32], int babies, size_t first_block, void *buf,
                                      size_t cap, size_t *len);
int hydia_db_delta_apply_seeded(hydia_ctx *ctx, const void *buf, size_t len);
/* OpenFHEWrapper::chebyshevCompare (src/openFHE_wrapper.cpp:143-185) on every ciphertext of the batch */
int hydia_chebyshev_compare(hydia_ctx *ctx, const hydia_ct *in, double delta, size_t sign_depth, hydia_ct **out);
/* multi-GPU membership tail: sum the batch into one ciphertext, then EvalSum over all slots (:46-47) */
int hydia_sum_and_evalsum(hydia_ctx *ctx, const hydia_ct *in, hydia_ct **out);

/* The two halves of that tail on their own — what a sharded membership query is composed of (sender_diag.cpp:46-47):
 * EvalAddManyInPlace over the batch -> ONE ciphertext; EvalSum(ct, batchSize) of one ciphertext. */
int hydia_add_many(hydia_ctx *ctx, const hydia_ct *in, hydia_ct **out);
int hydia_eval_sum(hydia_ctx *ctx, const hydia_ct *in, hydia_ct **out);
/* Cross-shard reduction of the partial sums: acc += src as plain 64-bit integers (src: same shape, compact, in HBM of
 * src_device; -1 = this context's GPU), and afterwards every value -> its canonical residue.  At most 16 residues below 2^60
 * fit 64 bits, so an RCCL all-reduce(SUM) on int64 over the handle's memory (hydia_ct_device_ptr) followed by
 * hydia_ct_mod_reduce is the multi-process form of the same step. */
int hydia_ct_add_raw(hydia_ctx *ctx, hydia_ct *acc, const void *dev_src, int src_device);
int hydia_ct_mod_reduce(hydia_ctx *ctx, hydia_ct *ct);

/* ---- sharded sender: one database over R contexts of ONE process (one per GPU of a node; shards may share a GPU) ----
 * Replaces the serial block loop of DiagonalSender::computeSimilarity (src/sender/sender_diag.cpp:28-30): shard r owns the
 * contiguous block range hydia_shard_blocks(G, R, r), every shard has the keys (same seed; one resident copy per GPU) and
 * runs loop A + its own mat-vec + comparator on its own host thread.  Queries enter and results leave through shard 0
 * (hydia_group_ctx(g, 0): encrypt / import the query there, decrypt there); result batches are in GLOBAL block order, so
 * hydia_decrypt_index returns database indices.  Results are bit-identical to one context holding the whole database. */
typedef struct hydia_group hydia_group;
/* block range [lo, hi) of `rank`: the first total_blocks % world ranks take one extra block (host only, no GPU needed) */
void hydia_shard_blocks(size_t total_blocks, uint32_t world, uint32_t rank, size_t *lo, size_t *hi);
/* a device index this node does not have: HYDIA_ERR_DEVICE, nothing is created (1 to 16 shards; a negative index: HYDIA_ERR_ARG) */
int hydia_group_create(const hydia_params *p, const int *devices /* [n_shards] GPU index of each shard */, uint32_t n_shards,
                       hydia_group **out);
void hydia_group_destroy(hydia_group *g);
uint32_t hydia_group_size(const hydia_group *g);
hydia_ctx *hydia_group_ctx(hydia_group *g, uint32_t shard); /* borrowed: never hydia_ctx_destroy it */
int hydia_group_keygen(hydia_group *g, const uint8_t seed[32]);
/* DiagonalEnroller::serializeDB over the group (normalises db IN PLACE); shard r enrols rows [first, first + n) of
 * hydia_group_shard_range */
int hydia_group_db_enroll(hydia_group *g, double *db /* n x vector_dim */, size_t n, const uint8_t seed[32]);
int hydia_group_shard_range(const hydia_group *g, uint32_t shard, size_t *first_vector, size_t *n_vectors);
/* How loop A (the 511 hoisted rotations) is shared: 0 = every shard computes all of them itself (nothing exchanged before the
 * mat-vec); 1 = shard k of the K active ones computes the contiguous range hydia_shard_blocks(vector_dim, K, k) and the ranges are
 * exchanged by peer copies (SURVEY 8e option B: loop A's work is done once per node instead of once per GPU).  Default 1.
 * Results are bit-identical either way. */
int hydia_group_set_rotation_split(hydia_group *g, int on);
/* Sender::computeSimilarity / indexScenario / membershipScenario over all shards; query and *out live in shard 0 */
int hydia_group_compute_similarity(hydia_group *g, const hydia_ct *query, hydia_ct **out);
int hydia_group_index_scenario(hydia_group *g, const hydia_ct *query, hydia_ct **out);
int hydia_group_membership_scenario(hydia_group *g, const hydia_ct *query, hydia_ct **out);

/* ---- HERS, approach 4: the paper's main comparison on the same kernels ---- */
/* HersEnroller::serializeDB, src/enroller/enroller_hers.cpp:40-93: index-batched (column) packing, vector_dim ciphertexts per
 * `slots`-vector matrix, normalises db IN PLACE; replaces the resident database */
int hydia_hers_db_enroll(hydia_ctx *ctx, double *db /* n x vector_dim */, size_t n, const uint8_t seed[32]);
/* HersReceiver::encryptQuery, src/receiver/receiver_hers.cpp:13-24: vector_dim ciphertexts, coordinate i in every slot */
int hydia_hers_encrypt_query(hydia_ctx *ctx, const double *query, const uint8_t seed[32], uint64_t nonce0, hydia_ct **out);
/* HersSender::computeSimilarity / indexScenario / membershipScenario, src/sender/sender_hers.cpp:13-58
 * (relinearise + rescale after every one of the vector_dim products of a block, :70-75) */
int hydia_hers_compute_similarity(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out);
int hydia_hers_index_scenario(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out);
int hydia_hers_membership_scenario(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out);

/* ---- the literature baseline, approach 1 (BaseEnroller / BaseReceiver / BaseSender): row-packed database, one query ciphertext ----
 * vpc = slots / vector_dim vectors per database ciphertext (64 at N = 2^16, dim 512).  The query is what hydia_encrypt_query returns
 * (BaseReceiver::encryptQuery, src/receiver/receiver_base.cpp:13-26, is DiagonalReceiver's); results decrypt with
 * hydia_decrypt_membership / hydia_decrypt_index.  Keys: hydia_keygen_rotations with the set of hydia_base_rotations.
 * The database is walked in chunks of C ciphertexts (C from the free device memory; HYDIA_BASE_CHUNK=<C> overrides); every C gives
 * the same bits.  A missing rotation or relinearisation key: HYDIA_ERR_STATE naming it, before any work is enqueued; another database
 * kind resident: HYDIA_ERR_STATE; a query that is not one fresh 2-component ciphertext at full level: HYDIA_ERR_ARG. */
/* ceil(n / vpc): database ciphertexts of n vectors (src/enroller/enroller_base.cpp:20-22) */
size_t hydia_base_db_num_cts(const hydia_ctx *ctx, size_t n_vectors);
/* BaseEnroller::serializeDB, src/enroller/enroller_base.cpp:13-56: normalises db IN PLACE, ciphertext i = vectors i vpc .. i vpc + vpc - 1
 * back to back (zeros after a ragged end), encoded and encrypted on the GPU into database kind 1 (plain 8-byte residues
 * [ct][2][n_q][N]; hydia_db_import_ct / hydia_db_export_ct then address these ciphertexts).  vector_dim must be a power of two
 * <= slots (HYDIA_ERR_ARG). */
int hydia_base_db_enroll(hydia_ctx *ctx, double *db /* n x vector_dim row-major */, size_t n, const uint8_t seed[32]);
/* BaseSender::computeSimilarity, src/sender/sender_base.cpp:13-27 + :84-98: per database ciphertext EvalInnerProduct(query, db_i,
 * vector_dim) (EvalMult with relinearisation, then c += Rot(c, 2^k), k = 0 .. log2(dim) - 1, at full level), one rescale, then
 * OpenFHEWrapper::mergeCiphers.  out: ceil(vpc n_cts / slots) ciphertexts on n_q - 3 limbs, score of vector j in slot j mod slots of
 * ciphertext j div slots */
int hydia_base_compute_similarity(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out);
/* BaseSender::indexScenario, src/sender/sender_base.cpp:69-81 */
int hydia_base_index_scenario(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out);
/* BaseSender::membershipScenario, src/sender/sender_base.cpp:50-66 */
int hydia_base_membership_scenario(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out);
/* OpenFHEWrapper::mergeCiphers, src/openFHE_wrapper.cpp:191-218 (with mergeSingleCipher :223-249 and generateMergeMask :253-268) on a
 * caller's batch: slot k dimension of ciphertext i -> slot (i slots / dimension + k) mod slots of output (i slots / dimension) div
 * slots.  dimension: a power of two, 2 <= dimension <= slots; every ciphertext needs a limb per mask multiply. */
int hydia_merge_ciphers(hydia_ctx *ctx, const hydia_ct *in, size_t dimension, hydia_ct **out);
/* Host only: the rotation keys approach 1 needs on a ring of `slots` slots — {2^k} u {slots - 2^k}, 1 <= 2^k < slots, ascending —
 * what src/main.cpp:195-206 generates for binaryRotate.  Writes at most cap entries; *n_out = the size of the set. */
int hydia_base_rotations(uint32_t slots, int32_t *rots, size_t cap, size_t *n_out);

/* ---- approach 2, GROTE group testing (GroteSender / GroteReceiver) ----
 * Enrolment (hydia_base_db_enroll), the query (hydia_encrypt_query), the keys (hydia_base_rotations) and computeSimilarity
 * (hydia_base_compute_similarity) are approach 1's, on the chain of hydia_params_for_approach(2): depth 18, 19 + 6 limbs, N = 2^16.
 * The S merged score ciphertexts are read as matrices of colLength rows x rowLength columns, rowLength = hydia_grote_row_length(slots),
 * colLength = slots / rowLength; the row sums and column sums of score^(2^alpha + 1) go through the comparator in place of the scores:
 * ceil(S / rowLength) + ceil(S / colLength) ciphertexts instead of S.  Conventions derived from OpenFHE's behaviour under FIXEDMANUAL,
 * unverified: EvalSquareInPlace / EvalMult(ct, ct) relinearise and do not rescale; a product of operands on
 * different limb counts drops the surplus limbs of the longer one without rescaling; a short packed plaintext is zero-padded.
 * Errors: a missing rotation or relinearisation key, too few limbs, another database kind resident: HYDIA_ERR_STATE, before any work is
 * enqueued; a row_length that is not a power of two in 2 .. slots: HYDIA_ERR_ARG.  HYDIA_GROTE_NO_SQ=1 routes the squares through the
 * general product kernel; the same bits. */
/* pow(2, ceil(log2(slots) / 2)), src/sender/sender_grote.cpp:18 and :44, src/receiver/receiver_grote.cpp:16.  Host only; 0 unless slots
 * is a power of two >= 2 */
uint32_t hydia_grote_row_length(uint32_t slots);
/* HersSender::alphaNormRows, src/sender/sender_hers.cpp:118-132, on a caller's batch of `count` 2-component ciphertexts: per ciphertext
 * alpha x (square, relinearise, rescale), the product with the input on the remaining limbs, c += Rot(c, 2^k) for 2^k < row_length, one
 * rescale, then OpenFHEWrapper::mergeCiphers(., row_length).  out: ceil(count (slots / row_length) / slots) ciphertexts */
int hydia_alpha_norm_rows(hydia_ctx *ctx, const hydia_ct *in, size_t alpha, size_t row_length, hydia_ct **out);
/* HersSender::alphaNormColumns, src/sender/sender_hers.cpp:136-178: the same power, a rescale, c += binaryRotate(c, -j) for j =
 * row_length, 2 row_length, .. < slots, the mask ones[0, row_length) with its rescale, ciphertext i into output (i row_length) div slots
 * at slot offset (i row_length) mod slots.  out: ceil(count row_length / slots) ciphertexts */
int hydia_alpha_norm_columns(hydia_ctx *ctx, const hydia_ct *in, size_t alpha, size_t row_length, hydia_ct **out);
/* GroteSender::indexScenario, src/sender/sender_grote.cpp:38-73: computeSimilarity, the rows and the columns (the shared power formed
 * once), each through chebyshevCompare(., 0.44^(2^ALPHA_DEPTH), COMP_DEPTH).  The reference returns the rows followed by the columns
 * in one vector; their limb counts differ by one, so they are two batches here */
int hydia_grote_index_scenario(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **rows, hydia_ct **cols);
/* GroteSender::membershipScenario, src/sender/sender_grote.cpp:13-36: its alphaNormColumns result is never read and is not computed
 * here; the ciphertext is hydia_base_membership_scenario's on this chain */
int hydia_grote_membership_scenario(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out);
/* GroteReceiver::decryptIndex, src/receiver/receiver_grote.cpp:12-65: matches are values >= 1.0; flat row R and flat column C pair when
 * R div colLength == C div rowLength (the same matrix) and give index R rowLength + C mod rowLength, rows outer, columns inner.  Two
 * matches of one matrix on different rows and columns decode to all four crossings (group testing).  rows / cols must hold
 * ceil(ceil(n_vectors / slots) / rowLength) and ceil(ceil(n_vectors / slots) / colLength) ciphertexts (:20-24; the reference prints an
 * error): otherwise HYDIA_ERR_ARG.  Writes at most cap entries; *n_out = the number of indices */
int hydia_grote_decrypt_index(hydia_ctx *ctx, const hydia_ct *rows, const hydia_ct *cols, size_t n_vectors, size_t *out, size_t cap, size_t *n_out);

/* ---- approach 3, the Blind-Match method (BlindEnroller / BlindReceiver / BlindSender) ----
 * On the chain of hydia_params_for_approach(3): depth 12, 13 + 5 limbs, N = 2^16.  A vector is cut into K = vector_dim / chunk_len
 * chunks (CHUNK_LEN 128, include/config.h:34: K = 4); spb = slots / chunk_len vectors make one database "matrix" of K ciphertexts, and
 * the query is K ciphertexts.  Per matrix the sender sums the K unrelinearised products in one kernel, relinearises and rescales once,
 * and adds log2(chunk_len) rotations; OpenFHEWrapper::compressCiphers interleaves chunk_len matrices into one score ciphertext.
 * Keys: hydia_keygen_rotations with the set of hydia_base_rotations.  The database is walked in passes of C matrices (C from the free
 * device memory; HYDIA_BLIND_PASS=<C> overrides); HYDIA_BLIND_NO_DOT=1 routes the sum of products through the general product kernel and
 * additions; every setting gives the same bits.  Errors: a chunk_len that is not a power of two in 2 .. slots dividing vector_dim, or
 * K > 32: HYDIA_ERR_ARG; a query that is not one batch of K fresh 2-component ciphertexts at full level: HYDIA_ERR_ARG; a missing
 * rotation or relinearisation key, no database or another database kind resident, fewer than four limbs: HYDIA_ERR_STATE, before any
 * work is enqueued.  hydia_db_save refuses this database kind (3), as it refuses kind 1. */
#define HYDIA_BLIND_CHUNK_LEN 128
/* K ceil(n / spb): database ciphertexts of n vectors (src/enroller/enroller_blind.cpp:15-17, :55); 0 for a chunk_len the packing cannot take */
size_t hydia_blind_db_num_cts(const hydia_ctx *ctx, size_t n_vectors, size_t chunk_len);
/* BlindEnroller::serializeDB, src/enroller/enroller_blind.cpp:13-90: normalises db IN PLACE; ciphertext m K + c holds coordinates
 * [c chunk_len, (c + 1) chunk_len) of vector m spb + v at slots [v chunk_len, (v + 1) chunk_len), zeros elsewhere; encoded and encrypted
 * on the GPU into database kind 3 (plain 8-byte residues [ct][2][n_q][N]; hydia_db_export_ct addresses these ciphertexts) */
int hydia_blind_db_enroll(hydia_ctx *ctx, double *db /* n x vector_dim row-major */, size_t n, size_t chunk_len, const uint8_t seed[32]);
/* BlindReceiver::encryptQuery, src/receiver/receiver_blind.cpp:13-26 and :58-71: normalise, then K ciphertexts in one batch, ciphertext c
 * = chunk c tiled over all slots, nonces nonce0 .. nonce0 + K - 1 */
int hydia_blind_encrypt_query(hydia_ctx *ctx, const double *query, size_t chunk_len, const uint8_t seed[32], uint64_t nonce0, hydia_ct **out);
/* BlindSender::computeSimilarity, src/sender/sender_blind.cpp:43-83, with the chunk length of the resident database.  out:
 * ceil(matrices / chunk_len) ciphertexts on n_q - 2 limbs; the score of vector i slots + k spb + v sits in slot v chunk_len + k of output i */
int hydia_blind_compute_similarity(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out);
/* BlindSender::indexScenario, src/sender/sender_blind.cpp:30-41 */
int hydia_blind_index_scenario(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out);
/* BlindSender::membershipScenario, src/sender/sender_blind.cpp:13-28 */
int hydia_blind_membership_scenario(hydia_ctx *ctx, const hydia_ct *query, hydia_ct **out);
/* OpenFHEWrapper::compressCiphers, src/openFHE_wrapper.cpp:273-312, on a caller's batch: every ciphertext times the mask with ones at slots
 * = 0 mod dimension and a rescale; ciphertext i into output i div dimension, rotated by binaryRotate(., -(i mod dimension)) unless that
 * is 0.  dimension: a power of two, 2 <= dimension <= slots; the ciphertexts need a limb to rescale away */
int hydia_compress_ciphers(hydia_ctx *ctx, const hydia_ct *in, size_t dimension, hydia_ct **out);
/* BlindReceiver::decryptIndex, src/receiver/receiver_blind.cpp:28-54: a value >= 1.0 at slot j of ciphertext i is vector
 * i slots + j div chunk_len + (j mod chunk_len) spb.  As in the reference, indices that fall into the padding past the number of enrolled
 * vectors are not filtered.  Writes at most cap entries; *n_out = the number of indices */
int hydia_blind_decrypt_index(hydia_ctx *ctx, const hydia_ct *index_cts, size_t chunk_len, size_t *out, size_t cap, size_t *n_out);

/* ---- evaluator primitives (used by the parity tests and by adapters) ---- */
/* sum_c q[c] (x) b[m K + c] without relinearisation: q a batch of K <= 32 ciphertexts, b a batch of M K ciphertexts (matrix-major), both
 * 2 components on the same limbs (limb-strided views allowed) -> M 3-component ciphertexts at scale(q) scale(b): what K calls of
 * hydia_eval_mult_no_relin summed with hydia_eval_add give (approach 3's fused product kernel; HYDIA_BLIND_NO_DOT) */
int hydia_eval_dot_no_relin(hydia_ctx *ctx, const hydia_ct *q, const hydia_ct *b, hydia_ct **out);
/* EvalSquare without relinearisation on the first n_limbs limbs of ct, read in place (0 = all): (c0^2, 2 c0 c1, c1^2), 3 components at
 * scale^2 — what hydia_eval_mult_no_relin(ct, ct) gives on those limbs (approach 2's squaring kernel; HYDIA_GROTE_NO_SQ) */
int hydia_eval_square_no_relin(hydia_ctx *ctx, const hydia_ct *ct, uint32_t n_limbs, hydia_ct **out);
int hydia_ntt(hydia_ctx *ctx, uint64_t *data /* host, [count][N] in place */, uint32_t count, uint32_t modulus_index,
              int inverse);
/* The ring size (15 or 16) whose specialised two-pass register-radix transform this context's plain transforms run on; 0 when they run
 * on the ring-size-generic kernels: any other ring, a context created under HYDIA_NTT_GENERIC=1 (the bit-identical parity switch), and
 * N = 2^16 unless the context was created under HYDIA_NTT16=1 — the 2^16 transforms are opt-in until they are measured */
int hydia_ntt_engine(const hydia_ctx *ctx);
int hydia_eval_rotate(hydia_ctx *ctx, const hydia_ct *in, int rot, hydia_ct **out);
int hydia_eval_mult(hydia_ctx *ctx, const hydia_ct *a, const hydia_ct *b, hydia_ct **out); /* mult+relin+rescale */
int hydia_eval_mult_no_relin(hydia_ctx *ctx, const hydia_ct *a, const hydia_ct *b, hydia_ct **out);
int hydia_relinearize(hydia_ctx *ctx, hydia_ct *ct);
int hydia_rescale(hydia_ctx *ctx, hydia_ct *ct);
int hydia_eval_add(hydia_ctx *ctx, hydia_ct *a, const hydia_ct *b);
int hydia_level_reduce(hydia_ctx *ctx, hydia_ct *ct, uint32_t n_limbs);
/* helpers of approach 1 (src/openFHE_wrapper.cpp), on every ciphertext of the batch:
 * EvalMult(ct, MakeCKKSPackedPlaintext(slots)) + RescaleInPlace under FIXEDMANUAL (:235-237): `slots` (slots doubles) encoded at scale
 * 2^scale_bits on the ciphertext's current limbs, multiplied residue-wise in evaluation form (scale ct.scale * 2^scale_bits), then
 * rescaled — out has one limb less.  `slots` is in the encoder's range stated at hydia_encrypt: max|slot| * 2^scale_bits < 2^63 is
 * sufficient, beyond it the plaintext's residues are unspecified, and no fault occurs */
int hydia_eval_mult_plain(hydia_ctx *ctx, const hydia_ct *ct, const double *slots, hydia_ct **out);
/* OpenFHEWrapper::binaryRotate (:103-128): the greedy signed power-of-two decomposition of `factor` (round(log2 |f|), largest first),
 * applied in that order; every step needs the key of its rotation mod slots */
int hydia_binary_rotate(hydia_ctx *ctx, const hydia_ct *ct, int32_t factor, hydia_ct **out);

/* ---- measurement: HIP-event time of named kernels on the context's stream since the last reset
 * ("hydia_tensor" = loop B's tensor-accumulate kernel, "hydia_tensor_multi" = its multi-query form, "ks_inner_product") ---- */
int hydia_kernel_time(hydia_ctx *ctx, const char *name, double *total_ms, uint64_t *launches);
int hydia_kernel_time_reset(hydia_ctx *ctx);
/* Byte ledger (process-wide): while enabled every kernel launcher records the bytes its launch has to move, by kernel name.
 * The current table ("kernel<TAB>launches<TAB>bytes" lines) is written to out (NUL-terminated, at most cap bytes; needed = full
 * size), THEN enable is applied: 1 = clear and record, 0 = stop and clear, -1 = leave as is.  tools/kernel_rooflines.py divides
 * by the rocprofv3 kernel times of the same run. */
int hydia_byte_ledger(int enable, char *out, size_t cap, size_t *needed);
/* NTT microbenchmark on pooled scratch memory: `polys` polynomials x moduli [first_mod, first_mod + n_mods), in place,
 * HIP-event milliseconds per iteration (tools/bench_ntt.py; 512 KiB algorithmic per limb-transform) */
int hydia_bench_ntt(hydia_ctx *ctx, uint32_t polys, uint32_t first_mod, uint32_t n_mods, int inverse, uint32_t iters,
                    double *ms_per_iter);

#ifdef __cplusplus
}
#endif
#endif
