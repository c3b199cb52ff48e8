// image_matching_amd/csrc/client.h — receiver / enroller / key-generation engines (GPU): sampling, canonical-embedding
// encode/decode, public-key encryption, decryption, on-GPU enrolment into the HBM-resident diagonal layout.
#pragma once
#include "client_kernels.h"
#include "hydia_core.h"

namespace hydia {
// a_seed != nullptr (both key generations): the SEEDED key set — every uniform half (the public key's a, every evk[d][1]) is sampled
// under the public a_seed at the unchanged stream addresses, the secret and every Gaussian error stay under seed; the context
// remembers a_seed and marks the keys it wrote.  The caller refuses a_seed == seed.  nullptr: not a bit changes
void client_keygen(Context &cx, const uint8_t seed[32], const uint8_t *a_seed = nullptr);
// sk, pk and relinearisation key exactly as client_keygen, rotation keys for exactly `rots` (each in [1, slots)); every other
// rotation key is released.  A key that client_keygen also makes comes out bit-identical (same sampler streams).
void client_keygen_rotations(Context &cx, const uint8_t seed[32], const std::vector<int> &rots, const uint8_t *a_seed = nullptr);
// half keys on the importing side: b = the [d][0] halves [dnum][nT][N] (the public key: [nQ][N]) from host memory into their strided
// places, the a halves expanded on the GPU under a_seed by key generation's own sample_uniform launch.  Not range-checked, not marked
void client_import_eval_key_seeded(Context &cx, int rot, const u64 *b, const uint8_t a_seed[32]);
void client_import_public_key_seeded(Context &cx, const u64 *b, const uint8_t a_seed[32]);
// a key from a wire message that passed its range check: d_src = its unpacked rows in DEVICE memory; a_seed == nullptr the whole key,
// otherwise the b halves, with the a halves expanded as the seeded imports expand them
void client_install_eval_key(Context &cx, int rot, const u64 *d_src, const uint8_t *a_seed);
void client_install_public_key(Context &cx, const u64 *d_src, const uint8_t *a_seed);
// seeded secret-key queries (k_enc_sym): c0 = NTT(e0 + m) - a s of probe i (normalised, tiled, encoded as client_encrypt_query does;
// e0 under seed, a under the public a_seed, nonce nonce0 + i) into HOST memory c0_out [n][nQ][N].  StateError without a secret key
void client_encrypt_queries_seeded(Context &cx, const double *queries /* n x vector_dim */, size_t n, const uint8_t seed[32],
                                   const uint8_t a_seed[32], uint64_t nonce0, u64 *c0_out, const WireRows *wire = nullptr);
// (wire != nullptr, here and in the _device twin: c0_out is the payload of a wire message — c0 leaves the GPU packed by k_wire_pack,
// wire->off[nQ] words per probe)
// and the sender's expansion: handle i = (c0[i], a(a_seed, nonce0 + i)), an ordinary [1][2][nQ][N] ciphertext at scale 2^scale_bits
std::vector<Ct> client_expand_seeded(Context &cx, const u64 *c0, size_t n, const uint8_t a_seed[32], uint64_t nonce0);
// c1 of seeded query `nonce` alone, enqueued on the stream: dst [nQ][N] in device memory (wire.cpp: c0 was unpacked into its handle)
void client_sample_query_a(Context &cx, const uint8_t a_seed[32], uint64_t nonce, u64 *dst);
// the switching key of Context::db_rekey: old_secret (host, [nT][N], evaluation form) -> this context's secret, into out (host,
// [dnum][2][nT][N]); sampler streams of key id HY_EVK_ID_SWITCH.  StateError without a secret; the context's own keys are untouched
void client_keygen_switch(Context &cx, const u64 *old_secret, const uint8_t seed[32], u64 *out);
// MakeCKKSPackedPlaintext(slots) at scale 2^scale_bits on limbs 0..nl-1 in evaluation form, with the Shoup companion of every
// residue for hk::mul_plain: pt [2][nl][N] (row 0 residues, row 1 companions)
void client_encode_plain(Context &cx, const double *slots, int nl, u64 *pt);
Ct client_encrypt(Context &cx, const double *slots, int count, const uint8_t seed[32], uint64_t nonce0);
Ct client_encrypt_query(Context &cx, const double *query, const uint8_t seed[32], uint64_t nonce);
void client_decrypt(Context &cx, const Ct &ct, double *out);
// the same slots left in DEVICE memory of the context's GPU (dev_out: X * slots doubles); slot 0 of the batch alone
void client_decrypt_device(Context &cx, const Ct &ct, double *dev_out);
double client_decrypt_slot0(Context &cx, const Ct &ct);
// ---- candidate lists and matches (include/hydia.h; select_kernels.hip).  A batch of n_results results, each either a ciphertext batch
// cts[r] that is decrypted on the way (n: the first n slots are searched, 0 = all X * slots of that result) or, with n_results == 1,
// the caller's device array dev_vals[0..n).  The C-ABI has checked every argument.  The whole batch is enqueued on the stream, result
// after result, and read back after ONE synchronisation; only counters and the selected entries cross to the host
struct SelectSource {
    const Ct *const *cts;
    const double *dev_vals;
    size_t n_results, n;
};
// row r of idx_out / val_out (cap entries apart; val_out may be null; idx_out null: count only): the indices i with v[i] >= threshold
// ascending, with their values; n_out[r] = how many there are, at most cap of them written
void client_select(Context &cx, const SelectSource &src, double threshold, size_t *idx_out, double *val_out, size_t cap, size_t *n_out);
// row r (k entries apart; val_out may be null): the min(k, n) largest by (value descending, index ascending), -0.0 tying with +0.0 and
// NaN below -inf; n_out[r] = min(k, n)
void client_topk(Context &cx, const SelectSource &src, size_t k, size_t *idx_out, double *val_out, size_t *n_out);
// first_block: index of this context's first 16384-vector block inside the whole database (a shard of a multi-GPU database
// encrypts with the nonces the unsharded enrolment would use, so shards hold bit-identical ciphertexts)
// babies < vector_dim: diagonals pre-rotated for the baby-step / giant-step mat-vec with that many hoisted rotations
// (Context::similarity_bsgs_sum); same ciphertext order and nonces.  0 or vector_dim: the reference's layout
void client_enroll(Context &cx, double *db, size_t n, const uint8_t seed[32], size_t first_block = 0, int babies = 0);
// resident kind 5 / 6 database += a fresh encryption of the sparse diagonal image of rows[n][dim] at vectors first_vector ..
// a plain gallery (kinds 7 / 8): the same slot images, encoded and not encrypted, into the resident one-polynomial layout
void client_plain_enroll(Context &cx, double *db, size_t n, int babies);
// a plain query: the plaintext client_encrypt_query encrypts, encoded and not encrypted ([1][1][nQ][N])
Ct client_encode_query(Context &cx, const double *query);
void client_db_update(Context &cx, size_t first_vector, double *rows, size_t n, int normalise, const uint8_t seed[32], size_t first_block = 0);
// resident kind 7 / 8 gallery += the ENCODED sparse diagonal image of rows[n][dim] at vectors first_vector .. (no seed, no nonce)
void client_plain_db_update(Context &cx, size_t first_vector, double *rows, size_t n, int normalise);
// ---- rows that already lie in device memory (include/hydia.h, hydia_dev_rows; the C-ABI has checked pointer, type, stride and state):
// n rows of vector_dim elements of `dtype` (hydia_dtype), `stride` elements apart, produced on `stream` (nullptr: complete already).
// The context's stream waits for an event recorded on `stream` — no host synchronisation on the way in; every call is synchronous on
// return.  The rows are never written.  Each *_device entry runs the block loop of its host twin from d_rows on (one k_rows_widen
// launch per block in place of the host normalisation and the copy), so the resident database comes out bit-identical
struct DevRows {
    const void *ptr;
    int dtype;
    size_t n, stride;
    hipStream_t stream;
};
void client_rows_widen(Context &cx, const DevRows &rows, int normalise, double *dev_dst /* [n][vector_dim] */);
void client_enroll_device(Context &cx, const DevRows &rows, const uint8_t seed[32], size_t first_block, int babies);
void client_plain_enroll_device(Context &cx, const DevRows &rows, int babies);
void client_db_update_device(Context &cx, size_t first_vector, const DevRows &rows, int normalise, const uint8_t seed[32], size_t first_block = 0);
void client_plain_db_update_device(Context &cx, size_t first_vector, const DevRows &rows, int normalise);
// a database delta (hydia_db_delta_make): the fresh encryptions E client_db_update would add, block by block, as the packed payloads of
// CT_BATCH messages in HOST memory — the b-th touched block's at payload0 + b * stride.  Public key only; no database is touched
void client_db_delta_make(Context &cx, size_t first_vector, double *rows, size_t n, int normalise, const uint8_t seed[32], int babies,
                          size_t first_block, unsigned char *payload0, size_t stride);
void client_db_delta_make_device(Context &cx, size_t first_vector, const DevRows &rows, int normalise, const uint8_t seed[32], int babies,
                                 size_t first_block, unsigned char *payload0, size_t stride);
// a SEEDED database delta (hydia_db_delta_make_seeded): the c0 halves of the secret-key encryptions (c0, a) of the same diagonal images,
// e0 under `seed` at the enrolment's nonces, a under the public a_seed at (first_block + block) * vector_dim + i, as the packed payloads
// of SEEDED_QUERY messages in host memory.  Needs the secret key (StateError otherwise); no database is touched
void client_db_delta_make_seeded(Context &cx, size_t first_vector, double *rows, size_t n, int normalise, const uint8_t seed[32],
                                 const uint8_t a_seed[32], int babies, size_t first_block, unsigned char *payload0, size_t stride);
void client_db_delta_make_seeded_device(Context &cx, size_t first_vector, const DevRows &rows, int normalise, const uint8_t seed[32],
                                        const uint8_t a_seed[32], int babies, size_t first_block, unsigned char *payload0, size_t stride);
// one handle per probe: query i = client_encrypt_query(row i, seed, nonce0 + i) / client_encode_query(row i), bit for bit
std::vector<Ct> client_encrypt_queries_device(Context &cx, const DevRows &rows, const uint8_t seed[32], uint64_t nonce0);
std::vector<Ct> client_encode_queries_device(Context &cx, const DevRows &rows);
// client_encrypt_queries_seeded from rows in device memory (one k_rows_widen and one k_query_tile per pass); c0_out is host memory
void client_encrypt_queries_seeded_device(Context &cx, const DevRows &rows, const uint8_t seed[32], const uint8_t a_seed[32], uint64_t nonce0,
                                          u64 *c0_out, const WireRows *wire = nullptr);
// HERS (approach 4): column-packed enrolment and the vector_dim broadcast query ciphertexts
void client_hers_enroll(Context &cx, double *db, size_t n, const uint8_t seed[32]);
Ct client_hers_encrypt_query(Context &cx, const double *query, const uint8_t seed[32], uint64_t nonce0);
// BaseEnroller (approach 1, the literature baseline): row-packed enrolment into database kind 1; ciphertext t takes nonce base + t
void client_base_enroll(Context &cx, double *db, size_t n, const uint8_t seed[32]);
// BlindEnroller / BlindReceiver (approach 3, Blind-Match): chunk-packed enrolment into database kind 3 (ciphertext m K + c = chunk c of
// matrix m, nonce base + m K + c, K = vector_dim / chunk_len) and the K tiled query ciphertexts (nonces nonce0 + c)
void client_blind_enroll(Context &cx, double *db, size_t n, int chunk_len, const uint8_t seed[32]);
Ct client_blind_encrypt_query(Context &cx, const double *query, int chunk_len, const uint8_t seed[32], uint64_t nonce0);
}  // namespace hydia
