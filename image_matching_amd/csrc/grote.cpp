// image_matching_amd/csrc/grote.cpp — approach 2, GROTE group testing, on the batched evaluator: GroteSender
// (/root/reference/src/sender/sender_grote.cpp) and HersSender::alphaNormRows / alphaNormColumns
// (/root/reference/src/sender/sender_hers.cpp:118-178).  Enrolment, query, keys and computeSimilarity are approach 1's (base.cpp).
//
// The S merged score ciphertexts are read as matrices of colLength rows x rowLength columns (rowLength = 2^ceil(log2(slots) / 2)).
// Per ciphertext s: p = s^(2^alpha) s (alpha squarings, each relinearised and rescaled, then one product with s on the lower limbs);
// the row sums and the column sums of p go through the comparator in place of the S score ciphertexts.  All S ciphertexts take the
// same steps, so they go through them as one batch; only the column placement differs per ciphertext.
//
// The reference forms s^(2^alpha) and the product once in alphaNormRows and again in alphaNormColumns; the values are identical, so
// the index scenario computes them once (alpha_norm_product) and feeds both.
//
// GroteSender::membershipScenario (sender_grote.cpp:13-36) calls alphaNormColumns and never reads the result: the ciphertext it
// returns is BaseSender::membershipScenario's on this chain.  The dead columns are NOT computed here.
//
// Three conventions under FIXEDMANUAL are derived from OpenFHE's behaviour and unverified: (a) EvalSquareInPlace
// and EvalMult(ct, ct) relinearise and do not rescale; (b) a ct x ct product of operands on different limb counts first drops the
// surplus limbs of the longer operand without rescaling, scales multiply; (c) MakeCKKSPackedPlaintext(v) with len(v) < slots is v
// zero-padded, encoded at 2^scale_bits on the ciphertext's current limbs (mult_plain_rescale).
#include <algorithm>
#include <set>

#include "hydia_core.h"

namespace hydia {

#define GROTE_ALPHA_DEPTH 2  // ALPHA_DEPTH, include/config.h:18
#define GROTE_COMP_DEPTH 10  // COMP_DEPTH, include/config.h:14

static bool is_pow2(long v) { return v >= 1 && (v & (v - 1)) == 0; }

// pow(2.0, ceil(log2(batchSize) / 2.0)) (sender_grote.cpp:18, :44; receiver_grote.cpp:16)
int Context::grote_row_length(long slots) {
    int lg = 0;
    while ((1L << lg) < slots) lg++;
    return 1 << ((lg + 1) / 2);
}
// mask multiplies (each a rescale) of mergeCiphers(., row_length): mergeSingleCipher's loop (openFHE_wrapper.cpp:231-246) + the last mask
int Context::grote_masks(int row_length) const {
    const long vpc = slots / row_length;
    int masks = 1;
    for (long i = 1, padding = 1; i < vpc; i *= 2)
        if (i >= padding) masks++, padding = i * row_length;
    return masks;
}

// EvalSquareInPlace's product (sender_hers.cpp:124, :153): 3 components, the caller relinearises and does not rescale (convention (a))
Ct Context::grote_square(const Ct &a) {
    if (a.npoly != 2) throw std::runtime_error("hydia: a square takes 2-component ciphertexts");
    Ct o;
    if (grote_sq) {
        op_bytes("op:square", N, 0, 5.0 * a.X * a.nl * N * 8);
        o = Ct(this, a.X, 3, a.nl, a.scale * a.scale);
        hk::tensor_sq(stream, d_mod, N, a.d, o.d, a.X, a.nl, a.lstride);
    } else {
        o = mult_norelin(a, a);
    }
    return o;
}

// every key-switch rotation of alphaNormRows / alphaNormColumns on n_cts ciphertexts
std::vector<int> Context::grote_rotations(size_t n_cts, int row_length, bool rows, bool cols) const {
    std::set<int> need;
    if (rows) {
        for (int r = 1; r < row_length; r <<= 1) need.insert(r);  // EvalInnerProduct's EvalSum
        for (int r : merge_rotations(n_cts, row_length)) need.insert(r);
    }
    if (cols) {
        for (long j = row_length; j < slots; j *= 2)
            for (int r : binary_rotations(-j)) need.insert(r);
        // placement offsets (row_length i) mod slots repeat with period slots / row_length
        for (size_t i = 0; i < std::min(n_cts, (size_t)(slots / row_length)); i++)
            for (int r : binary_rotations(-(long)(((size_t)row_length * i) % (size_t)slots))) need.insert(r);
    }
    return std::vector<int>(need.begin(), need.end());
}
void Context::grote_check(const Ct &in, int alpha_depth, int row_length, bool rows, bool cols) const {
    if (!is_pow2(row_length) || row_length < 2 || row_length > slots) throw std::runtime_error("hydia: row_length must be a power of two in 2 .. slots");
    if (alpha_depth < 0 || alpha_depth > HY_MAX_MODS) throw std::runtime_error("hydia: alpha out of range");
    if (in.X < 1 || in.npoly != 2) throw std::runtime_error("hydia: the alpha norm takes 2-component ciphertexts");
    // alpha squarings and the product rescale once each; the rows then lose a limb per mask of mergeCiphers, the columns one (the row mask)
    const int need = alpha_depth + 1 + std::max(rows ? grote_masks(row_length) : 0, cols ? 1 : 0);
    if (in.nl <= need) throw StateError("hydia: the alpha norm needs " + std::to_string(need) + " limbs to rescale away at this row length, the input has " + std::to_string(in.nl));
    base_check_keys(grote_rotations((size_t)in.X, row_length, rows, cols));
}

// alphaNorm*'s shared prefix (sender_hers.cpp:122-127, :149-156), every ciphertext of the batch
Ct Context::alpha_norm_product(const Ct &s, int alpha_depth) {
    Ct a = s.alias(s.nl);
    for (int k = 0; k < alpha_depth; k++) {
        Ct sq = grote_square(a);
        relinearize(sq);
        rescale(sq);
        a = std::move(sq);
    }
    Ct sd = s.alias(a.nl);  // convention (b): s on a's limbs, read in place
    Ct p = mult_norelin(a, sd);
    relinearize(p);
    return p;
}
// alphaNormRows after the product (sender_hers.cpp:127-131): EvalInnerProduct's EvalSum over rowLength slots (c += Rot(c, 2^k), k
// ascending, approach 1's order), ONE rescale, mergeCiphers(., rowLength)
Ct Context::alpha_norm_rows_from(const Ct &p, int row_length) {
    Ct r = rotate_acc(p, 1, p);
    for (int k = 2; k < row_length; k <<= 1) r = rotate_acc(r, k, r);
    rescale(r);
    merge_single(r, row_length);
    const size_t vpc = (size_t)(slots / row_length), n_out = (vpc * (size_t)p.X + slots - 1) / slots;
    Ct out;
    merge_place(r, 0, row_length, out, n_out);
    return out;
}
// alphaNormColumns after the product (sender_hers.cpp:157-174): rescale, c += binaryRotate(c, -j) for j = rowLength, 2 rowLength, ..
// < slots, the mask ones[0, rowLength) (convention (c)), then ciphertext i into output (i rowLength) div slots at offset
// (i rowLength) mod slots — merge_place's structure with rowLength values per ciphertext
Ct Context::alpha_norm_columns_from(const Ct &p, int row_length) {
    Ct c = p.alias(p.nl);
    rescale(c);
    for (long j = row_length; j < slots; j *= 2) add_binary_rotated(*this, c, -j);
    const int col_length = slots / row_length;
    c = mult_plain_rescale(c, merge_mask(col_length, row_length, c.nl));  // dimension x segment = slots: the one segment [0, rowLength)
    const size_t n_out = ((size_t)row_length * (size_t)p.X + slots - 1) / slots;
    Ct out;
    merge_place(c, 0, col_length, out, n_out);
    return out;
}

// HersSender::alphaNormRows / alphaNormColumns on a caller's batch
Ct Context::alpha_norm_rows(const Ct &in, int alpha_depth, int row_length) {
    grote_check(in, alpha_depth, row_length, true, false);
    Ct p = alpha_norm_product(in, alpha_depth);
    return alpha_norm_rows_from(p, row_length);
}
Ct Context::alpha_norm_columns(const Ct &in, int alpha_depth, int row_length) {
    grote_check(in, alpha_depth, row_length, false, true);
    Ct p = alpha_norm_product(in, alpha_depth);
    return alpha_norm_columns_from(p, row_length);
}

// GroteSender::indexScenario (sender_grote.cpp:38-73): rows first, then columns; their limb counts differ by one, so two batches
void Context::grote_index_scenario(const Ct &qc, Ct &rows, Ct &cols) {
    if (!d_db || db_cts == 0 || db_kind != 1) throw StateError("hydia: no database resident (row packing, approaches 1 and 2)");
    base_check_query(qc);
    const int rl = grote_row_length(slots), masks = grote_masks(rl);
    // computeSimilarity leaves n_q - 3 limbs; the rows reach the comparator on n_q - 3 - ALPHA_DEPTH - 1 - masks of them, and it takes
    // COMP_DEPTH more
    if (nQ < 3 + GROTE_ALPHA_DEPTH + 1 + masks + 1)
        throw StateError("hydia: approach 2 needs a chain of at least " + std::to_string(3 + GROTE_ALPHA_DEPTH + 1 + masks + 1) + " limbs");
    if (nQ - 3 - GROTE_ALPHA_DEPTH - 1 - masks < GROTE_COMP_DEPTH + 1)
        throw StateError("hydia: the chain is too short for approach 2: the comparator needs " + std::to_string(GROTE_COMP_DEPTH + 1) + " limbs after the alpha norm, " +
                         std::to_string(nQ - 3 - GROTE_ALPHA_DEPTH - 1 - masks) + " are left (hydia_params_for_approach(2))");
    const size_t S = ((size_t)(slots / prm.dim) * db_cts + slots - 1) / slots;
    base_check_keys(grote_rotations(S, rl, true, true));
    Ct s = base_similarity(qc);  // checks its own keys before its own work
    Ct p;
    phase(*this, "grote_alpha", [&] { p = alpha_norm_product(s, GROTE_ALPHA_DEPTH); });
    phase(*this, "grote_rows", [&] { rows = alpha_norm_rows_from(p, rl); });
    phase(*this, "grote_cols", [&] { cols = alpha_norm_columns_from(p, rl); });
    // the scores were raised to 2^ALPHA_DEPTH, so is the threshold (sender_grote.cpp:55-58: the same two products in double)
    double threshold = 0.44;  // MATCH_THRESHOLD
    for (int a = 0; a < GROTE_ALPHA_DEPTH; a++) threshold = threshold * threshold;
    phase(*this, "grote_compare", [&] {
        rows = chebyshev_compare(rows, threshold, GROTE_COMP_DEPTH);
        cols = chebyshev_compare(cols, threshold, GROTE_COMP_DEPTH);
    });
}
// GroteSender::membershipScenario (sender_grote.cpp:13-36): BaseSender::membershipScenario on this chain (header comment)
Ct Context::grote_membership_scenario(const Ct &qc) { return base_membership_scenario(qc); }

}  // namespace hydia
