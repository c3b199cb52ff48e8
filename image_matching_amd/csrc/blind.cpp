// image_matching_amd/csrc/blind.cpp — approach 3, the Blind-Match method, on the batched evaluator: BlindSender
// (/root/reference/src/sender/sender_blind.cpp) and OpenFHEWrapper::compressCiphers (/root/reference/src/openFHE_wrapper.cpp:273-312).
//
// A vector of dim coordinates is cut into K = dim / chunk_len chunks.  Database "matrix" m holds spb = slots / chunk_len vectors as K
// ciphertexts (ciphertext m K + c = chunk c of every vector of the matrix, vector v at slots [v chunk_len, (v + 1) chunk_len)); the query
// is K ciphertexts, chunk c tiled over all slots.  Per matrix: acc = sum_c q_c (x) db_{m,c} without relinearisation (three components,
// ascending c), ONE relinearisation, ONE rescale, then acc += Rot(acc, r) for r = 1, 2, 4, .. < chunk_len: slot v chunk_len holds the
// score of vector m spb + v.  compressCiphers masks those slots and interleaves chunk_len matrices into one ciphertext.
//
// Every matrix takes the same steps, so the database goes through them in passes of C matrices: one launch sequence per step whatever C
// is, and every matrix's arithmetic is what it would be alone, so the pass size changes no bit.  Only compressCiphers' placement
// rotations differ per ciphertext and run one ciphertext at a time.
#include <algorithm>
#include <cmath>
#include <set>

#include "client.h"
#include "hydia_core.h"

namespace hydia {

static bool is_pow2(long v) { return v >= 1 && (v & (v - 1)) == 0; }

#define BLIND_MATCH_THRESHOLD 0.44  // MATCH_THRESHOLD, include/config.h:9
#define BLIND_COMP_DEPTH 10         // COMP_DEPTH, include/config.h:14

// chunks per vector; a chunk length the packing cannot take is an argument error
int Context::blind_chunks(int chunk_len) const {
    if (!is_pow2(chunk_len) || chunk_len < 2 || chunk_len > slots || chunk_len > prm.dim || prm.dim % chunk_len)
        throw std::runtime_error("hydia: chunk_len must be a power of two in 2 .. slots that divides vector_dim");
    const int K = prm.dim / chunk_len;
    if (K > HY_BLIND_MAX_CHUNKS)
        throw std::runtime_error("hydia: vector_dim / chunk_len must be at most " + std::to_string(HY_BLIND_MAX_CHUNKS) + " (the lazy sums of the fused product)");
    return K;
}

// sum_c q[c] (x) b[x][c] for x < C: q [K][2][q_ls][N], b [C][K][2][b_ls][N], nl limbs in use -> [C][3][nl][N].  k_tensor_dot, or
// (HYDIA_BLIND_NO_DOT) the launchers it replaces: per chunk the query replicated per matrix, the database operand staged, k_tensor,
// and the three-component sum taken in ascending c — the same residues
Ct Context::blind_dot(const u64 *q, int q_ls, const u64 *b, int b_ls, int C, int K, int nl, double scale) {
    if (blind_fused) {
        op_bytes("op:mult_dot", N, 0, (2.0 * K + (2.0 * K + 3.0) * C) * nl * N * 8);
        Ct prod(this, C, 3, nl, scale);
        hk::tensor_dot(stream, d_mod, N, q, q_ls, b, b_ls, prod.d, C, K, nl);
        return prod;
    }
    Ct rep(this, C, 2, nl, 1.0), dbc(this, C, 2, nl, scale), prod;
    const size_t qp = (size_t)q_ls * N, bp = (size_t)b_ls * N, ce = (size_t)2 * nl * N;
    for (int c = 0; c < K; c++) {
        for (int p = 0; p < 2; p++) {
            hk::copy_limbs(stream, N, q + ((size_t)c * 2 + p) * qp, rep.d + (size_t)p * nl * N, 0, ce, C, nl);
            hk::copy_limbs(stream, N, b + ((size_t)c * 2 + p) * bp, dbc.d + (size_t)p * nl * N, (size_t)K * 2 * bp, ce, C, nl);
        }
        Ct t = mult_norelin(rep, dbc);
        if (c == 0)
            prod = std::move(t);
        else
            add_inplace(prod, t);
    }
    return prod;
}
// the relin-free entry on caller's batches: q = K ciphertexts, b = M K ciphertexts (matrix-major), both 2 components on the same limbs
Ct Context::eval_dot_no_relin(const Ct &q, const Ct &b) {
    if (q.X < 1 || q.npoly != 2 || b.npoly != 2 || q.nl != b.nl) throw std::runtime_error("hydia: the dot product takes 2-component ciphertexts on the same limbs");
    if (q.X > HY_BLIND_MAX_CHUNKS) throw std::runtime_error("hydia: at most " + std::to_string(HY_BLIND_MAX_CHUNKS) + " query ciphertexts (the lazy sums of the fused product)");
    if (b.X < q.X || b.X % q.X) throw std::runtime_error("hydia: the database batch must hold a multiple of the query's ciphertext count");
    return blind_dot(q.d, q.lstride, b.d, b.lstride, b.X / q.X, q.X, q.nl, q.scale * b.scale);
}

// matrices per pass: what the free device memory (and the pool's cache) holds of one matrix's product, key-switch digits and
// temporaries; the K x 2 database operands are read in place and cost nothing.  At most 1024, at least 1; HYDIA_BLIND_PASS overrides
int Context::blind_pass(size_t matrices) {
    if (blind_pass_env > 0) return (int)std::min<size_t>(matrices, (size_t)blind_pass_env);
    const int nE = nQ + nP, nd = (nQ + alpha - 1) / alpha;
    // [3][nQ] product, [2][nQ] relinearised, digits [nd][nE], accumulator [2][nE], [2][nP] + [2][nQ] ModDown images, two more [2][nQ]
    // ciphertexts alive across a rotate-and-accumulate step (+ the unfused product's replicated query, staged operand and second product)
    const double per_m = (double)(3 * nQ + 2 * nQ + nd * nE + 2 * nE + 2 * nP + 2 * nQ + 4 * nQ + (blind_fused ? 0 : 7 * nQ)) * N * 8;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return 1;
    const double avail = 0.8 * ((double)free_b + (double)pool.bytes_cached);
    return (int)std::max(1.0, std::min({(double)matrices, 1024.0, std::floor(avail / per_m)}));
}

// computeSimilarityMatrix (sender_blind.cpp:59-83) on matrices m0 .. m0+C-1: the sum of the K products, RelinearizeInPlace,
// RescaleInPlace, then c += binaryRotate(c, r) for r = 1, 2, 4, .. < chunk_len — each r a power of two, so one key switch — on n_q - 1 limbs
Ct Context::blind_similarity_chunk(const Ct &qc, size_t m0, int C) {
    const int K = prm.dim / db_chunk_len;
    const u64 *dbp = reinterpret_cast<const u64 *>(d_db) + m0 * (size_t)K * 2 * nQ * N;
    Ct acc = blind_dot(qc.d, qc.lstride, dbp, nQ, C, K, nQ, qc.scale * delta);
    relinearize(acc);
    rescale(acc);
    for (int r = 1; r < db_chunk_len; r <<= 1) acc = rotate_acc(acc, r, acc);
    return acc;
}

// the key-switch rotations of compressCiphers on n_cts ciphertexts: binaryRotate(., -(i mod dimension))
std::vector<int> Context::compress_rotations(size_t n_cts, int dimension) const {
    std::set<int> need;
    for (size_t k = 1; k < std::min(n_cts, (size_t)dimension); k++)
        for (int r : binary_rotations(-(long)k)) need.insert(r);
    return std::vector<int>(need.begin(), need.end());
}
// compressCiphers' second loop (openFHE_wrapper.cpp:299-309) for masked ciphertexts i0 .. i0+X-1: ciphertext i goes to output
// i div dimension, as it is when i mod dimension = 0, otherwise rotated by binaryRotate(., -(i mod dimension)) and added, in ciphertext order
void Context::compress_place(const Ct &masked, size_t i0, int dimension, Ct &out, size_t n_out) {
    if (out.X == 0) out = Ct(this, (int)n_out, 2, masked.nl, masked.scale);
    for (int x = 0; x < masked.X; x++) {
        const size_t i = i0 + (size_t)x, o = i / (size_t)dimension, k = i % (size_t)dimension;
        Ct src = masked.alias(masked.nl);
        src.X = 1;
        src.d = masked.d + (size_t)x * masked.ct_elems();
        Ct dst = out.alias(out.nl);
        dst.X = 1;
        dst.d = out.d + o * out.ct_elems();
        if (k == 0) {
            hk::copy_limbs(stream, N, src.d, dst.d, src.poly_elems(), dst.poly_elems(), 2, src.nl);
            continue;
        }
        const std::vector<int> rots = binary_rotations(-(long)k);
        Ct t;
        for (size_t s = 0; s < rots.size(); s++) t = rotate(s == 0 ? src : t, rots[s]);
        op_bytes("op:add", N, 0, 3.0 * 2 * dst.nl * N * 8);
        hk::add(stream, d_mod, N, dst.d, t.d, dst.d, 2, sel_q(dst.nl), dst.lstride, t.lstride, dst.lstride);
    }
}
// OpenFHEWrapper::compressCiphers on a caller's batch: the one-hot mask at slots = 0 mod dimension (generateMergeMask's shape with
// segment 1; the RelinearizeInPlace after it is a no-op on two components) and its rescale on the whole batch, then the placement
Ct Context::compress_ciphers(const Ct &in, int dimension) {
    if (!is_pow2(dimension) || dimension < 2 || dimension > slots) throw std::runtime_error("hydia: the compression dimension must be a power of two in 2 .. slots");
    if (in.X < 1 || in.npoly != 2) throw std::runtime_error("hydia: compressCiphers takes 2-component ciphertexts");
    if (in.nl < 2) throw StateError("hydia: compressCiphers needs a limb to rescale away");
    base_check_keys(compress_rotations((size_t)in.X, dimension));
    const size_t n_out = ((size_t)in.X + dimension - 1) / (size_t)dimension;
    Ct masked = mult_plain_rescale(in, merge_mask(dimension, 1, in.nl)), out;
    compress_place(masked, 0, dimension, out, n_out);
    return out;
}

void Context::blind_check_query(const Ct &q) const {
    if (!d_db || db_cts == 0 || db_kind != 3) throw StateError("hydia: no database resident (chunk packing, approach 3)");
    const int K = prm.dim / db_chunk_len;
    if (q.X != K || q.npoly != 2 || q.nl != nQ || !q.compact())
        throw std::runtime_error("hydia: the Blind-Match query must be one batch of " + std::to_string(K) + " fresh 2-component ciphertexts at full level");
    if (nQ < 4) throw StateError("hydia: approach 3 needs a chain of at least four limbs");
}

// BlindSender::computeSimilarity (sender_blind.cpp:43-56)
Ct Context::blind_similarity(const Ct &qc) {
    blind_check_query(qc);
    const int cl = db_chunk_len, K = prm.dim / cl;
    const size_t M = db_cts / (size_t)K, n_out = (M + cl - 1) / (size_t)cl;
    std::vector<int> need = compress_rotations(M, cl);
    for (int r = 1; r < cl; r <<= 1) need.push_back(r);
    base_check_keys(need);
    Ct out;
    for (size_t m0 = 0; m0 < M;) {
        const int C = blind_pass(M - m0);
        Ct s;
        phase(*this, "blind_similarity", [&] { s = blind_similarity_chunk(qc, m0, C); });
        phase(*this, "blind_compress", [&] {
            Ct masked = mult_plain_rescale(s, merge_mask(cl, 1, s.nl));
            compress_place(masked, m0, cl, out, n_out);
        });
        m0 += (size_t)C;
    }
    return out;
}
// BlindSender::indexScenario (sender_blind.cpp:30-41)
Ct Context::blind_index_scenario(const Ct &qc) {
    Ct s = blind_similarity(qc);
    Ct r;
    phase(*this, "blind_compare", [&] { r = chebyshev_compare(s, BLIND_MATCH_THRESHOLD, BLIND_COMP_DEPTH); });
    return r;
}
// BlindSender::membershipScenario (sender_blind.cpp:13-28): EvalAddMany, then EvalSum over all slots — approach 1's tail; needs EvalSum's
// keys 2^k < slots on top of computeSimilarity's
Ct Context::blind_membership_scenario(const Ct &qc) {
    blind_check_query(qc);
    std::vector<int> need;
    for (int r = 1; r < slots; r <<= 1) need.push_back(r);
    base_check_keys(need);
    Ct s = blind_index_scenario(qc);
    return sum_and_evalsum(s);
}

}  // namespace hydia
