// image_matching_amd/csrc/base.cpp — approach 1, the literature baseline, on the batched evaluator: BaseSender
// (/root/reference/src/sender/sender_base.cpp) and OpenFHEWrapper::mergeCiphers / mergeSingleCipher / generateMergeMask
// (/root/reference/src/openFHE_wrapper.cpp:191-268).
//
// Every database ciphertext takes the SAME rotations through EvalInnerProduct and mergeSingleCipher, so the database goes through
// them as batches of C ciphertexts (a "chunk"): one launch sequence per step whatever C is, and every ciphertext's arithmetic is
// what it would be alone, so the chunk size changes no bit.  Evaluator steps per chunk (each a launch sequence) at dim 512, vpc 64: 1 product + 1 relinearisation +
// 9 rotate-and-accumulate key switches + 1 rescale (step 3); 2 mask products with their rescales + 6 x (1 rotation + 1
// rotate-and-accumulate) (step 4); then the placement rotations of step 5, which differ per ciphertext and run one ciphertext at a time.
#include <algorithm>
#include <cmath>
#include <set>

#include "client.h"
#include "hydia_core.h"

namespace hydia {

static bool is_pow2(long v) { return v >= 1 && (v & (v - 1)) == 0; }

#define HY_MERGE_MASKS 32

void Context::base_phase_collect() {
    for (auto &e : base_phase_pending) {
        float ms = 0;
        if (hipEventSynchronize(e.b) == hipSuccess && hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
            timers[e.name].total_ms += ms;
            timers[e.name].launches++;
        }
        (void)hipEventDestroy(e.a);
        (void)hipEventDestroy(e.b);
    }
    base_phase_pending.clear();
}

void Context::base_check_query(const Ct &q) const {
    if (q.X != 1 || q.npoly != 2 || q.nl != nQ || !q.compact())
        throw std::runtime_error("hydia: the baseline query must be one fresh 2-component ciphertext at full level");
}
void Context::base_check_keys(const std::vector<int> &rots) const {
    if (!relin_key.d) throw StateError("hydia: relinearisation key not loaded");
    for (int r : rots)
        if (!rot_keys.count(r)) throw StateError("hydia: rotation key " + std::to_string(r) + " not loaded (approach 1 needs the set of hydia_base_rotations)");
}
// the key-switch rotations mergeCiphers applies to a batch of n_cts ciphertexts (mergeSingleCipher's loop, then the placements)
std::vector<int> Context::merge_rotations(size_t n_cts, int dimension) const {
    std::set<int> need;
    const long vpc = slots / dimension;
    for (long i = 1; i < vpc; i *= 2)
        for (int r : binary_rotations((long)(dimension - 1) * i)) need.insert(r);
    // placement offsets (vpc i) mod slots repeat with period slots / vpc = dimension
    for (size_t i = 0; i < std::min(n_cts, (size_t)dimension); i++)
        for (int r : binary_rotations(-(long)((vpc * (long)i) % slots))) need.insert(r);
    return std::vector<int>(need.begin(), need.end());
}

// generateMergeMask (openFHE_wrapper.cpp:253-268): ones at [k dimension seg, k dimension seg + seg) for every k
const u64 *Context::merge_mask(int dimension, int seg, int nl) {
    const std::vector<int> key{dimension, seg, nl};
    auto it = merge_masks.find(key);
    if (it != merge_masks.end()) return it->second;
    if (merge_masks.size() >= HY_MERGE_MASKS) {  // a caller walking many (dimension, level) pairs: start over rather than grow without bound
        sync_all();  // enqueued mask products may still read the old entries
        for (auto &kv : merge_masks) (void)hipFree(kv.second);
        merge_masks.clear();
    }
    std::vector<double> mask((size_t)slots, 0.0);
    for (size_t i = 0; i < (size_t)slots; i += (size_t)dimension * seg)
        std::fill(mask.begin() + i, mask.begin() + std::min((size_t)slots, i + (size_t)seg), 1.0);
    u64 *pt = nullptr;
    HIP_CHECK(hipMalloc((void **)&pt, sizeof(u64) * 2 * (size_t)nl * N));
    try {
        client_encode_plain(*this, mask.data(), nl, pt);
    } catch (...) {
        (void)hipFree(pt);
        throw;
    }
    merge_masks[key] = pt;
    return pt;
}

// database ciphertexts per pass: what the free device memory (and the pool's cache) holds of one ciphertext's product, key-switch
// digits and temporaries, at most 1024 (the launchers' grid limits), at least 1; HYDIA_BASE_CHUNK overrides
int Context::base_chunk(size_t cts) {
    if (base_chunk_env > 0) return (int)std::min<size_t>(cts, (size_t)base_chunk_env);
    const int nE = nQ + nP, nd = (nQ + alpha - 1) / alpha;
    // [3][nQ] product, [2][nQ] relinearised, digits [nd][nE], accumulator [2][nE], [2][nP] + [2][nQ] ModDown images, two more
    // [2][nQ] ciphertexts alive across a rotate-and-accumulate step (+ the staged copies of the unfused product)
    const double per_ct = (double)(3 * nQ + 2 * nQ + nd * nE + 2 * nE + 2 * nP + 2 * nQ + 4 * nQ + (base_bcast ? 0 : 4 * nQ)) * N * 8;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return 1;
    const double avail = 0.8 * ((double)free_b + (double)pool.bytes_cached);
    return (int)std::max(1.0, std::min({(double)cts, 1024.0, std::floor(avail / per_ct)}));
}

// computeSimilarityThread (sender_base.cpp:84-98) on database ciphertexts t0 .. t0+C-1: EvalInnerProduct(query, db_i, dim) =
// EvalMult with relinearisation, then EvalSum over dim slots (c += Rot(c, 2^k), k ascending) at full level and scale delta^2; the
// RelinearizeInPlace that follows is a no-op on two components; ONE rescale last.  (The order inside EvalInnerProduct is derived
// from OpenFHE's documentation, unverified: DESIGN.md section 2.)
Ct Context::base_similarity_chunk(const Ct &qc, size_t t0, int C) {
    const size_t ce = (size_t)2 * nQ * N;
    const u64 *dbp = reinterpret_cast<const u64 *>(d_db) + t0 * ce;
    Ct prod;
    if (base_bcast) {
        op_bytes("op:mult_bcast", N, 0, (2.0 + 5.0 * C) * nQ * N * 8);
        prod = Ct(this, C, 3, nQ, qc.scale * delta);
        hk::tensor_bcast(stream, d_mod, N, qc.d, qc.lstride, dbp, nQ, prod.d, C, nQ);
    } else {  // the existing launchers: the query replicated per ciphertext, the database operand staged
        Ct rep(this, C, 2, nQ, qc.scale), dbc(this, C, 2, nQ, delta);
        for (int x = 0; x < C; x++) hk::copy_limbs(stream, N, qc.d, rep.d + (size_t)x * ce, qc.poly_elems(), (size_t)nQ * N, 2, nQ);
        db_fetch(t0, dbc.d, C);
        prod = mult_norelin(rep, dbc);
    }
    relinearize(prod);
    for (int r = 1; r < prm.dim; r <<= 1) prod = rotate_acc(prod, r, prod);
    rescale(prod);
    return prod;
}

// c += binaryRotate(c, factor) (openFHE_wrapper.cpp:241): all steps but the last are plain rotations, the last one accumulates
void add_binary_rotated(Context &cx, Ct &c, long factor) {
    const std::vector<int> rots = cx.binary_rotations(factor);
    if (rots.empty()) {  // a multiple of the slot count: binaryRotate returns its input
        Ct t = cx.clone(c);
        cx.add_inplace(c, t);
        return;
    }
    Ct t;
    for (size_t k = 0; k + 1 < rots.size(); k++) t = cx.rotate(k == 0 ? c : t, rots[k]);
    c = cx.rotate_acc(rots.size() == 1 ? c : t, rots.back(), c);
}

// mergeSingleCipher (openFHE_wrapper.cpp:223-249) on every ciphertext of the batch
void Context::merge_single(Ct &c, int dimension) {
    const long vpc = slots / dimension;
    long padding = 1;
    for (long i = 1; i < vpc; i *= 2) {
        if (i >= padding) {
            c = mult_plain_rescale(c, merge_mask(dimension, (int)i, c.nl));
            padding = i * dimension;
        }
        add_binary_rotated(*this, c, (long)(dimension - 1) * i);
    }
    c = mult_plain_rescale(c, merge_mask(dimension, (int)vpc, c.nl));
}

// mergeCiphers' second loop (openFHE_wrapper.cpp:206-215) for merged ciphertexts i0 .. i0+X-1: ciphertext i goes to output
// (vpc i) div slots, rotated by -((vpc i) mod slots) unless that is 0, and is added there.  The rotations differ per ciphertext, so
// each ciphertext takes its own binary_rotations(-offset) in order
void Context::merge_place(const Ct &merged, size_t i0, int dimension, Ct &out, size_t n_out) {
    const size_t vpc = (size_t)(slots / dimension);
    if (out.X == 0) out = Ct(this, (int)n_out, 2, merged.nl, merged.scale);
    for (int x = 0; x < merged.X; x++) {
        const size_t i = i0 + (size_t)x, o = (vpc * i) / (size_t)slots, off = (vpc * i) % (size_t)slots;
        Ct src = merged.alias(merged.nl);
        src.X = 1;
        src.d = merged.d + (size_t)x * merged.ct_elems();
        Ct dst = out.alias(out.nl);
        dst.X = 1;
        dst.d = out.d + o * out.ct_elems();
        if (off == 0) {
            hk::copy_limbs(stream, N, src.d, dst.d, src.poly_elems(), dst.poly_elems(), 2, src.nl);
            continue;
        }
        const std::vector<int> rots = binary_rotations(-(long)off);
        Ct t;
        for (size_t k = 0; k < rots.size(); k++) t = rotate(k == 0 ? src : t, rots[k]);
        op_bytes("op:add", N, 0, 3.0 * 2 * dst.nl * N * 8);
        hk::add(stream, d_mod, N, dst.d, t.d, dst.d, 2, sel_q(dst.nl), dst.lstride, t.lstride, dst.lstride);
    }
}

// OpenFHEWrapper::mergeCiphers on a caller's batch
Ct Context::merge_ciphers(const Ct &in, int dimension) {
    if (!is_pow2(dimension) || dimension < 2 || dimension > slots) throw std::runtime_error("hydia: the merge dimension must be a power of two in 2 .. slots");
    if (in.X < 1 || in.npoly != 2) throw std::runtime_error("hydia: mergeCiphers takes 2-component ciphertexts");
    const long vpc = slots / dimension;
    int masks = 1;
    for (long i = 1, padding = 1; i < vpc; i *= 2)
        if (i >= padding) masks++, padding = i * dimension;
    if (in.nl <= masks) throw StateError("hydia: mergeCiphers needs " + std::to_string(masks) + " limbs to rescale away at this dimension");
    base_check_keys(merge_rotations((size_t)in.X, dimension));
    const size_t n_out = ((size_t)vpc * in.X + slots - 1) / slots;
    Ct c = clone(in), out;
    merge_single(c, dimension);
    merge_place(c, 0, dimension, out, n_out);
    return out;
}

// BaseSender::computeSimilarity (sender_base.cpp:13-27)
Ct Context::base_similarity(const Ct &qc) {
    if (!d_db || db_cts == 0 || db_kind != 1) throw StateError("hydia: no database resident (row packing, approach 1)");
    base_check_query(qc);
    const int dim = prm.dim;
    std::vector<int> need = merge_rotations(db_cts, dim);
    for (int r = 1; r < dim; r <<= 1) need.push_back(r);
    base_check_keys(need);
    if (nQ < 5) throw StateError("hydia: approach 1 needs a chain of at least five limbs");
    const size_t vpc = (size_t)(slots / dim), n_out = (vpc * db_cts + slots - 1) / slots;
    Ct out;
    for (size_t t0 = 0; t0 < db_cts;) {
        const int C = base_chunk(db_cts - t0);
        Ct s;
        phase(*this, "base_similarity", [&] { s = base_similarity_chunk(qc, t0, C); });
        phase(*this, "base_merge", [&] {
            merge_single(s, dim);
            merge_place(s, t0, dim, out, n_out);
        });
        t0 += (size_t)C;
    }
    return out;
}
// BaseSender::indexScenario (sender_base.cpp:69-81)
Ct Context::base_index_scenario(const Ct &qc) {
    Ct s = base_similarity(qc);
    Ct r;
    phase(*this, "base_compare", [&] { r = chebyshev_compare(s, 0.44 /* MATCH_THRESHOLD */, 10 /* COMP_DEPTH */); });
    return r;
}
// BaseSender::membershipScenario (sender_base.cpp:50-66): needs EvalSum's keys 2^k < slots on top of computeSimilarity's
Ct Context::base_membership_scenario(const Ct &qc) {
    std::vector<int> need;
    for (int r = 1; r < slots; r <<= 1) need.push_back(r);
    base_check_keys(need);
    Ct s = base_index_scenario(qc);
    return sum_and_evalsum(s);
}

}  // namespace hydia
