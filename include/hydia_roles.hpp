// include/hydia_roles.hpp — the reference's C++ role surface for approach 5 (HyDia), approach 4 (HERS), approach 1 (the literature
// baseline: include/{enroller,receiver,sender}_base.h) and approach 2 (GROTE: include/{receiver,sender}_grote.h), over the C-ABI of hydia.h.
//
// Same class and method names as /root/reference/include/{sender,sender_diag,receiver,receiver_hers,receiver_diag,
// enroller_diag,enroller_hers}.h and the same constructor arguments (include/sender.h:22 `(cc, pk, numVectors)`,
// include/receiver.h:20-21 `(cc, pk, sk, numVectors)`, include/enroller_hers.h:19), so that src/main.cpp's cases 4 and 5
// (:183-192, :243-247, :319-327, :333-374) read unchanged; the OpenFHE handle types are replaced by thin handles onto HBM-resident
// objects:
//     CryptoContext<DCRTPoly>            ->  hydia::CryptoContext (context + keys + resident database)
//     PublicKey / PrivateKey<DCRTPoly>   ->  hydia::PublicKey / PrivateKey (placeholders: the key material lives in the context)
//     Ciphertext<DCRTPoly>               ->  hydia::Ciphertext   (one element of a device batch)
// `using namespace hydia::ofhe;` gives these the reference's template spelling (Ciphertext<DCRTPoly>, ...).
// Randomness: like the reference (OpenFHE seeds its PRNG from the OS) every role object draws its 32-byte sampler key from the
// operating system (hydia_random_seed) unless the caller passes one for reproducibility; nonces count up per object.
// Error behaviour mirrors the reference: a message on cerr and carry on (src/sender/sender_diag.cpp:89-91); the
// status code of the last failing call is kept in CryptoContext::last_status for callers that want to assert.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "hydia.h"

namespace hydia {

const double MATCH_THRESHOLD = 0.44;  // include/config.h:9
const size_t COMP_DEPTH = 10;         // include/config.h:14
const size_t VECTOR_DIM = 512;        // include/config.h:30
const size_t CHUNK_LEN = HYDIA_BLIND_CHUNK_LEN;  // include/config.h:34

inline void role_seed(uint8_t out[32], const uint8_t *seed32) {
    if (seed32) {
        for (int i = 0; i < 32; i++) out[i] = seed32[i];
    } else if (hydia_random_seed(out) != 0) {
        std::cerr << "Error: " << hydia_last_error() << std::endl;
        std::abort();  // never encrypt under a predictable key
    }
}

class CryptoContextImpl;
// Placeholders for OpenFHE's PublicKey<DCRTPoly> / PrivateKey<DCRTPoly>: the key material stays inside the context (HBM), the
// handles only say "this context's keys" so that the reference's constructor calls keep their shape.
struct PublicKey {
    const CryptoContextImpl *owner = nullptr;
    explicit operator bool() const { return owner != nullptr; }
};
struct PrivateKey {
    const CryptoContextImpl *owner = nullptr;
    explicit operator bool() const { return owner != nullptr; }
};
struct KeyPair {  // what cc->KeyGen() returns (src/main.cpp:183-185)
    PublicKey publicKey;
    PrivateKey secretKey;
    bool good() const { return (bool)publicKey && (bool)secretKey; }
    explicit operator bool() const { return good(); }
};

class CryptoContextImpl {
  public:
    hydia_ctx *h = nullptr;
    hydia_info info{};
    int last_status = 0;
    hydia_group *group = nullptr;  // set when the context is sharded over several GPUs; h is then the group's shard 0
    explicit CryptoContextImpl(const hydia_params &p, int device = 0) {
        last_status = hydia_ctx_create(&p, device, &h);
        if (last_status != 0) {
            std::cerr << "Error: " << hydia_last_error() << std::endl;
            h = nullptr;
            return;
        }
        hydia_get_info(h, &info);
    }
    // one context per entry of `devices` (DB row-blocks sharded across them); queries and results use shard 0
    CryptoContextImpl(const hydia_params &p, const std::vector<int> &devices) {
        last_status = hydia_group_create(&p, devices.data(), (uint32_t)devices.size(), &group);
        if (last_status != 0) {
            std::cerr << "Error: " << hydia_last_error() << std::endl;
            group = nullptr;
            return;
        }
        h = hydia_group_ctx(group, 0);
        hydia_get_info(h, &info);
    }
    ~CryptoContextImpl() {
        if (group) hydia_group_destroy(group);
        else hydia_ctx_destroy(h);
    }
    CryptoContextImpl(const CryptoContextImpl &) = delete;
    CryptoContextImpl &operator=(const CryptoContextImpl &) = delete;
    bool check(int code, const char *what) {
        if (code != 0) {
            last_status = code;
            std::cerr << "Error: " << what << ": " << hydia_last_error() << std::endl;
        }
        return code == 0;
    }
    size_t GetRingDimension() const { return info.n; }
    size_t GetBatchSize() const { return info.slots; }
    // cc->KeyGen() (src/main.cpp:183): secret, public, relinearisation, rotation {1..dim-1, dim*2^k} keys in ONE call — everything
    // EvalMultKeyGen / EvalSumKeyGen / EvalRotateKeyGen (:187-206) would add; seed32 == nullptr draws the key material from the OS.
    // The returned pair is empty (good() == false) when generation failed.
    KeyPair KeyGen(const uint8_t *seed32 = nullptr) {
        uint8_t seed[32];
        role_seed(seed, seed32);
        if (!check(group ? hydia_group_keygen(group, seed) : hydia_keygen(h, seed), "key generation")) return KeyPair{};
        return KeyPair{PublicKey{this}, PrivateKey{this}};
    }
    // KeyGen with every uniform half sampled under a PUBLIC expansion seed (hydia_keygen_seeded; no counterpart in the reference): the
    // receiver then ships half keys (DiagonalReceiver::exportKeysSeeded).  aSeed32 == nullptr draws the public seed from the OS too,
    // independently of the secret one.  Not on a sharded context: an error, empty
    KeyPair KeyGenSeeded(const uint8_t *seed32 = nullptr, const uint8_t *aSeed32 = nullptr) {
        if (group) {
            last_status = HYDIA_ERR_STATE;
            std::cerr << "Error: key generation: a seeded key set is generated on the receiver's own context" << std::endl;
            return KeyPair{};
        }
        uint8_t seed[32], aSeed[32];
        role_seed(seed, seed32);
        role_seed(aSeed, aSeed32);
        if (!check(hydia_keygen_seeded(h, seed, aSeed), "key generation")) return KeyPair{};
        return KeyPair{PublicKey{this}, PrivateKey{this}};
    }
    // approach 1's key set: secret, public, relinearisation and rotation keys {2^k} u {batch - 2^k} (hydia_base_rotations) — what
    // src/main.cpp:195-206 generates for binaryRotate; hydia_keygen's set would not fit a 2^16 ring
    KeyPair KeyGenBaseline(const uint8_t *seed32 = nullptr) {
        uint8_t seed[32];
        role_seed(seed, seed32);
        if (group) {
            last_status = HYDIA_ERR_STATE;
            std::cerr << "Error: key generation: approach 1 does not run on a sharded context" << std::endl;
            return KeyPair{};
        }
        size_t n = 0;
        if (!check(hydia_base_rotations(info.slots, nullptr, 0, &n), "key generation")) return KeyPair{};
        std::vector<int32_t> rots(n);
        if (!check(hydia_base_rotations(info.slots, rots.data(), n, &n), "key generation")) return KeyPair{};
        if (!check(hydia_keygen_rotations(h, seed, rots.data(), (uint32_t)n), "key generation")) return KeyPair{};
        return KeyPair{PublicKey{this}, PrivateKey{this}};
    }
    // src/main.cpp:187-206: the evaluation keys exist since KeyGen; these keep the reference's call sequence compiling
    void EvalMultKeyGen(const PrivateKey &) {}
    void EvalSumKeyGen(const PrivateKey &) {}
    template <class IndexList>
    void EvalRotateKeyGen(const PrivateKey &, const IndexList &) {}
};
using CryptoContext = std::shared_ptr<CryptoContextImpl>;

inline CryptoContext GenCryptoContext(size_t multDepth = 11, uint32_t scalingModSize = 45, uint32_t vectorDim = 512,
                                      uint32_t logN = 15, int device = 0) {
    hydia_params p;
    hydia_default_params(&p);
    p.mult_depth = (uint32_t)multDepth;
    p.scale_bits = scalingModSize;
    p.vector_dim = vectorDim;
    p.log_n = logN;
    return std::make_shared<CryptoContextImpl>(p, device);
}
// the same context sharded over several GPUs (or several shards on one): DiagonalEnroller / DiagonalSender then work on
// the whole group, each GPU owning a contiguous range of 16384-vector blocks
inline CryptoContext GenShardedCryptoContext(const std::vector<int> &devices, size_t multDepth = 11, uint32_t scalingModSize = 45,
                                             uint32_t vectorDim = 512, uint32_t logN = 15) {
    hydia_params p;
    hydia_default_params(&p);
    p.mult_depth = (uint32_t)multDepth;
    p.scale_bits = scalingModSize;
    p.vector_dim = vectorDim;
    p.log_n = logN;
    return std::make_shared<CryptoContextImpl>(p, devices);
}

// one ciphertext = (shared device batch, index inside it)
struct CtBatch {
    CryptoContext cc;
    hydia_ct *h = nullptr;
    CtBatch(CryptoContext c, hydia_ct *p) : cc(std::move(c)), h(p) {}
    ~CtBatch() { hydia_ct_free(h); }
    uint32_t count() const {
        uint32_t c = 0;
        if (h) hydia_ct_shape(h, &c, nullptr, nullptr, nullptr);
        return c;
    }
};
struct Ciphertext {
    std::shared_ptr<CtBatch> batch;
    uint32_t index = 0;
    explicit operator bool() const { return batch && batch->h; }
};
// a plain query (hydia.h, "plain query"): a probe the sender knows, ONE encoded polynomial in HBM.  A type of its own — the methods
// that take ciphertexts do not take it
struct PtHandle {
    CryptoContext cc;
    hydia_pt *h = nullptr;
    PtHandle(CryptoContext c, hydia_pt *p) : cc(std::move(c)), h(p) {}
    PtHandle(const PtHandle &) = delete;
    PtHandle &operator=(const PtHandle &) = delete;
    ~PtHandle() { hydia_pt_free(h); }
};
struct Plaintext {
    std::shared_ptr<PtHandle> pt;
    explicit operator bool() const { return pt && pt->h; }
};
// templates already in device memory (hydia.h, hydia_dev_rows): n rows of vector_dim elements of `dtype`, rowStride elements apart,
// on the context's GPU, produced on `stream` (a hipStream_t; nullptr: complete already).  The rows are only read, and may be reused
// when the call that takes them returns.  The overloads that take one do what their std::vector twins do, bit for bit
struct DeviceRows {
    hydia_dev_rows d;
    DeviceRows(const void *ptr, hydia_dtype dtype, size_t n, size_t rowStride, void *stream = nullptr) : d{ptr, dtype, n, rowStride, stream} {}
    size_t size() const { return d.n; }
};
// seeded queries and keys as they travel (hydia.h, "seeded keys and queries"): the uniform halves are the expansion of the PUBLIC
// aSeed, so only the other halves are carried.  SeededQuery: c0 [count][n_q][N]; query i was made with nonce0 + i
struct SeededQuery {
    std::vector<uint64_t> c0;
    uint8_t aSeed[32] = {};
    uint64_t nonce0 = 0;
    size_t count = 0;
    size_t nbytes() const { return c0.size() * sizeof(uint64_t) + 32 + sizeof(uint64_t); }
    explicit operator bool() const { return count > 0 && !c0.empty(); }
};
// SeededKeys: the public key's b [n_q][N] and per key id (0 = relinearisation) the b halves [dnum][n_q+n_p][N]
struct SeededKeys {
    uint8_t aSeed[32] = {};
    std::vector<uint64_t> publicKey;
    std::map<int, std::vector<uint64_t>> evalKeys;
    explicit operator bool() const { return !publicKey.empty(); }
};
inline std::vector<Ciphertext> split_batch(const CryptoContext &cc, hydia_ct *h) {
    std::vector<Ciphertext> v;
    if (!h) return v;
    auto b = std::make_shared<CtBatch>(cc, h);
    for (uint32_t i = 0; i < b->count(); i++) v.push_back(Ciphertext{b, i});
    return v;
}

// Wire messages (hydia.h, "wire messages"): what crosses between receiver, sender and enroller as BYTES — residues packed into the bit
// length of their modulus on the GPU, and on arrival validated, unpacked and range-checked on the GPU.  Not authenticated: transport
// security is the caller's.  toWire takes the whole of one device batch (what every role method here returns); fromWire gives the
// batch of a type 1 message.  Approaches 1 - 4 use these two through their handles.  Empty on failure
inline std::vector<uint8_t> toWire(const CryptoContext &cc, const std::vector<Ciphertext> &ctxts) {
    if (ctxts.empty() || !ctxts[0] || ctxts[0].batch->count() != ctxts.size()) {
        cc->last_status = HYDIA_ERR_ARG;
        std::cerr << "Error: toWire takes the whole of one ciphertext batch" << std::endl;
        return {};
    }
    size_t n = 0;
    hydia_ct_to_wire(cc->h, ctxts[0].batch->h, nullptr, 0, &n);  // the size: HYDIA_ERR_ARG with n = the need
    std::vector<uint8_t> buf(n);
    if (!n || !cc->check(hydia_ct_to_wire(cc->h, ctxts[0].batch->h, buf.data(), buf.size(), &n), "toWire")) return {};
    return buf;
}
// every handle a ciphertext message makes: one batch (type 1), or one single-ciphertext handle per seeded query (type 2)
inline std::vector<std::vector<Ciphertext>> handlesFromWire(const CryptoContext &cc, const std::vector<uint8_t> &message, const char *what) {
    hydia_wire_info info;
    if (!cc->check(hydia_wire_peek(message.data(), message.size(), &info), what)) return {};
    std::vector<hydia_ct *> h(info.type == 1 ? 1 : (size_t)info.count, nullptr);
    size_t n = 0;
    if (!cc->check(hydia_ct_from_wire(cc->h, message.data(), message.size(), h.data(), h.size(), &n), what)) return {};
    std::vector<std::vector<Ciphertext>> r;
    for (size_t i = 0; i < n; i++) r.push_back(split_batch(cc, h[i]));
    return r;
}
inline std::vector<Ciphertext> fromWire(const CryptoContext &cc, const std::vector<uint8_t> &message) {
    std::vector<std::vector<Ciphertext>> r = handlesFromWire(cc, message, "fromWire");
    if (r.size() != 1) {
        if (!r.empty()) std::cerr << "Error: fromWire takes a message of one batch or one query (queriesFromWire takes several)" << std::endl;
        return {};
    }
    return r[0];
}

// the reference's template spelling of the handle types: `using namespace hydia::ofhe;` in place of `using namespace lbcrypto;`
namespace ofhe {
struct DCRTPoly {};
template <class Element>
using CryptoContext = ::hydia::CryptoContext;
template <class Element>
using Ciphertext = ::hydia::Ciphertext;
template <class Element>
using PublicKey = ::hydia::PublicKey;
template <class Element>
using PrivateKey = ::hydia::PrivateKey;
}  // namespace ofhe

namespace OpenFHEWrapper {
// src/openFHE_wrapper.cpp:6-44
inline size_t computeRequiredDepth(size_t approach) { return hydia_compute_required_depth(approach); }
// src/openFHE_wrapper.cpp:81-85 (whole batch the ciphertext belongs to; returns the slots of ct.index)
inline std::vector<double> decryptToVector(CryptoContext cc, Ciphertext ctxt) {
    std::vector<double> all((size_t)ctxt.batch->count() * cc->info.slots);
    cc->check(hydia_decrypt(cc->h, ctxt.batch->h, all.data()), "decrypt");
    return std::vector<double>(all.begin() + (size_t)ctxt.index * cc->info.slots,
                               all.begin() + (size_t)(ctxt.index + 1) * cc->info.slots);
}
// the reference's three-argument spelling (include/openFHE_wrapper.h): the key handle only says "this context's key"
inline std::vector<double> decryptToVector(CryptoContext cc, PrivateKey, Ciphertext ctxt) { return decryptToVector(cc, ctxt); }
// src/openFHE_wrapper.cpp:88-99: the slots of every ciphertext, one after the other (one decryption per distinct device batch)
inline std::vector<double> decryptVectorToVector(CryptoContext cc, PrivateKey, std::vector<Ciphertext> ctxts) {
    const size_t S = cc->info.slots;
    std::vector<double> out(S * ctxts.size()), all;
    const CtBatch *have = nullptr;
    for (size_t i = 0; i < ctxts.size(); i++) {
        if (!ctxts[i]) continue;
        if (ctxts[i].batch.get() != have) {
            have = ctxts[i].batch.get();
            all.assign((size_t)have->count() * S, 0.0);
            cc->check(hydia_decrypt(cc->h, have->h, all.data()), "decrypt");
        }
        std::copy(all.begin() + (size_t)ctxts[i].index * S, all.begin() + (size_t)(ctxts[i].index + 1) * S, out.begin() + i * S);
    }
    return out;
}
// src/openFHE_wrapper.cpp:74-77: one ciphertext of vec (padded with zeros to the slot count) under a fresh sampler key from the OS
inline Ciphertext encryptFromVector(CryptoContext cc, PublicKey, std::vector<double> vec) {
    uint8_t seed[32];
    role_seed(seed, nullptr);
    vec.resize(cc->info.slots, 0.0);
    hydia_ct *out = nullptr;
    if (!cc->check(hydia_encrypt(cc->h, vec.data(), 1, seed, 0, &out), "encryptFromVector")) return {};
    return split_batch(cc, out)[0];
}
// src/openFHE_wrapper.cpp:143-185 (the comparator runs on the whole batch the ciphertext belongs to; returns the element of ctxt.index)
inline Ciphertext chebyshevCompare(CryptoContext cc, Ciphertext ctxt, double delta, size_t signDepth) {
    hydia_ct *out = nullptr;
    if (!ctxt || !cc->check(hydia_chebyshev_compare(cc->h, ctxt.batch->h, delta, signDepth, &out), "chebyshevCompare")) return {};
    return split_batch(cc, out)[ctxt.index];
}
// src/openFHE_wrapper.cpp:191-218: every dimension-th slot of every ciphertext, packed in order.  The ciphertexts must be the
// elements 0 .. n-1 of ONE device batch, in order (what every role method here returns); otherwise an error and an empty result
inline std::vector<Ciphertext> mergeCiphers(CryptoContext cc, std::vector<Ciphertext> &ctxts, size_t dimension) {
    if (ctxts.empty() || !ctxts[0] || ctxts[0].batch->count() != ctxts.size()) {
        std::cerr << "Error: mergeCiphers takes the whole of one ciphertext batch" << std::endl;
        return {};
    }
    for (size_t i = 0; i < ctxts.size(); i++)
        if (ctxts[i].batch != ctxts[0].batch || ctxts[i].index != i) {
            std::cerr << "Error: mergeCiphers takes the whole of one ciphertext batch" << std::endl;
            return {};
        }
    hydia_ct *out = nullptr;
    if (!cc->check(hydia_merge_ciphers(cc->h, ctxts[0].batch->h, dimension, &out), "mergeCiphers")) return {};
    return split_batch(cc, out);
}
}  // namespace OpenFHEWrapper

// ---- include/sender.h:19-43
class Sender {
  public:
    Sender(CryptoContext ccParam, size_t vectorParam) : cc(std::move(ccParam)), numVectors(vectorParam) {}
    Sender(CryptoContext ccParam, PublicKey pkParam, size_t vectorParam) : cc(std::move(ccParam)), pk(pkParam), numVectors(vectorParam) {}  // include/sender.h:22
    virtual ~Sender() = default;
    virtual std::vector<Ciphertext> computeSimilarity(std::vector<Ciphertext> &queryCipher) = 0;
    virtual Ciphertext membershipScenario(std::vector<Ciphertext> &queryCipher) = 0;
    virtual std::vector<Ciphertext> indexScenario(std::vector<Ciphertext> &queryCipher) = 0;

  protected:
    CryptoContext cc;
    PublicKey pk;
    size_t numVectors;
};
// ---- include/sender_diag.h:5-28 (HersSender, approach 4, is further down).  On a sharded context (GenShardedCryptoContext)
// the same three methods run over every GPU of the group: per-shard mat-vec, results back in global block order, membership
// as per-shard EvalAddMany -> integer sum -> mod q -> EvalSum (hydia.h, "sharded sender").
class DiagonalSender : public Sender {
  public:
    DiagonalSender(CryptoContext ccParam, size_t vectorParam) : Sender(std::move(ccParam), vectorParam) {}
    DiagonalSender(CryptoContext ccParam, PublicKey pkParam, size_t vectorParam) : Sender(std::move(ccParam), pkParam, vectorParam) {}
    std::vector<Ciphertext> computeSimilarity(std::vector<Ciphertext> &queryCipher) override {
        hydia_ct *out = run(queryCipher, hydia_compute_similarity, hydia_group_compute_similarity, "computeSimilarity");
        return out ? split_batch(cc, out) : std::vector<Ciphertext>{};
    }
    Ciphertext membershipScenario(std::vector<Ciphertext> &queryCipher) override {
        hydia_ct *out = run(queryCipher, hydia_membership_scenario, hydia_group_membership_scenario, "membershipScenario");
        return out ? split_batch(cc, out)[0] : Ciphertext{};
    }
    std::vector<Ciphertext> indexScenario(std::vector<Ciphertext> &queryCipher) override {
        hydia_ct *out = run(queryCipher, hydia_index_scenario, hydia_group_index_scenario, "indexScenario");
        return out ? split_batch(cc, out) : std::vector<Ciphertext>{};
    }
    // Several queries in one pass over the resident database (an extension: the reference serves one query per call).  One
    // queryCipher per query in; per query exactly what the single-query method returns.  Not on a sharded context: an error, empty.
    std::vector<std::vector<Ciphertext>> computeSimilarityMulti(std::vector<std::vector<Ciphertext>> &queryCiphers) {
        std::vector<std::vector<Ciphertext>> r;
        for (hydia_ct *h : run_multi(queryCiphers, hydia_compute_similarity_multi, "computeSimilarityMulti")) r.push_back(split_batch(cc, h));
        return r;
    }
    std::vector<Ciphertext> membershipScenarioMulti(std::vector<std::vector<Ciphertext>> &queryCiphers) {
        std::vector<Ciphertext> r;
        for (hydia_ct *h : run_multi(queryCiphers, hydia_membership_scenario_multi, "membershipScenarioMulti")) r.push_back(split_batch(cc, h)[0]);
        return r;
    }
    std::vector<std::vector<Ciphertext>> indexScenarioMulti(std::vector<std::vector<Ciphertext>> &queryCiphers) {
        std::vector<std::vector<Ciphertext>> r;
        for (hydia_ct *h : run_multi(queryCiphers, hydia_index_scenario_multi, "indexScenarioMulti")) r.push_back(split_batch(cc, h));
        return r;
    }
    // The same against a PLAIN gallery (PlainEnroller, database kinds 7 / 8; the *Multi methods above keep refusing one): the queries
    // share passes over the gallery; per query exactly what the single-query method returns.  Not on a sharded context: an error, empty.
    std::vector<std::vector<Ciphertext>> computeSimilarityGalleryMulti(std::vector<std::vector<Ciphertext>> &queryCiphers) {
        std::vector<std::vector<Ciphertext>> r;
        for (hydia_ct *h : run_multi(queryCiphers, hydia_compute_similarity_gallery_multi, "computeSimilarityGalleryMulti")) r.push_back(split_batch(cc, h));
        return r;
    }
    std::vector<Ciphertext> membershipScenarioGalleryMulti(std::vector<std::vector<Ciphertext>> &queryCiphers) {
        std::vector<Ciphertext> r;
        for (hydia_ct *h : run_multi(queryCiphers, hydia_membership_scenario_gallery_multi, "membershipScenarioGalleryMulti")) r.push_back(split_batch(cc, h)[0]);
        return r;
    }
    std::vector<std::vector<Ciphertext>> indexScenarioGalleryMulti(std::vector<std::vector<Ciphertext>> &queryCiphers) {
        std::vector<std::vector<Ciphertext>> r;
        for (hydia_ct *h : run_multi(queryCiphers, hydia_index_scenario_gallery_multi, "indexScenarioGalleryMulti")) r.push_back(split_batch(cc, h));
        return r;
    }
    // Seeded keys and queries (an extension; hydia.h): the sender regenerates the uniform halves on its GPU from the public seed.
    // importKeysSeeded takes DiagonalReceiver::exportKeysSeeded's set; expandQuery / expandQueries turn a SeededQuery into ordinary
    // queryCiphers, one per probe, that every method above takes.  Not on a sharded context: an error, false / empty
    bool importKeysSeeded(const SeededKeys &keys) {
        if (cc->group || !keys) {
            cc->last_status = cc->group ? HYDIA_ERR_STATE : HYDIA_ERR_ARG;
            std::cerr << "Error: importKeysSeeded: " << (cc->group ? "seeded keys are imported into one context" : "empty key set") << std::endl;
            return false;
        }
        const size_t pk_words = (size_t)cc->info.n_q * cc->info.n, key_words = hydia_eval_key_seeded_words(cc->h);
        bool sized = keys.publicKey.size() == pk_words;
        for (auto &kv : keys.evalKeys) sized = sized && kv.second.size() == key_words;
        if (!sized) {
            cc->last_status = HYDIA_ERR_ARG;
            std::cerr << "Error: importKeysSeeded: a half key of another size than this context's" << std::endl;
            return false;
        }
        if (!cc->check(hydia_import_public_key_seeded(cc->h, keys.publicKey.data(), keys.aSeed), "importKeysSeeded")) return false;
        for (auto &kv : keys.evalKeys)
            if (!cc->check(hydia_import_eval_key_seeded(cc->h, kv.first, kv.second.data(), keys.aSeed), "importKeysSeeded")) return false;
        return true;
    }
    std::vector<std::vector<Ciphertext>> expandQueries(const SeededQuery &q) {
        if (cc->group || !q || q.c0.size() != q.count * (size_t)cc->info.n_q * cc->info.n) {
            cc->last_status = cc->group ? HYDIA_ERR_STATE : HYDIA_ERR_ARG;
            std::cerr << "Error: expandQueries: " << (cc->group ? "seeded queries are expanded on one context" : "c0 does not hold count polynomials [n_q][N]") << std::endl;
            return {};
        }
        std::vector<hydia_ct *> h(q.count, nullptr);
        if (!cc->check(hydia_ct_expand_seeded(cc->h, q.c0.data(), q.count, q.aSeed, q.nonce0, h.data()), "expandQueries")) return {};
        std::vector<std::vector<Ciphertext>> r;
        for (size_t i = 0; i < q.count; i++) r.push_back(split_batch(cc, h[i]));
        return r;
    }
    std::vector<Ciphertext> expandQuery(const SeededQuery &q) {
        if (q.count != 1) {
            cc->last_status = HYDIA_ERR_ARG;
            std::cerr << "Error: expandQuery takes one probe (expandQueries takes a batch)" << std::endl;
            return {};
        }
        std::vector<std::vector<Ciphertext>> r = expandQueries(q);
        return r.empty() ? std::vector<Ciphertext>{} : r[0];
    }
    // Wire messages (an extension; hydia.h): the checked path for what arrives from outside.  importKeysWire loads
    // DiagonalReceiver::exportKeysWire's file (not transactional: a refused file leaves the keys of earlier messages installed);
    // queryFromWire turns a query message into the queryCipher every method above takes (a type 2 message of one probe, or a type 1
    // batch), queriesFromWire a message of several probes into one queryCipher each; resultToWire ships a scenario's output.  Not on a
    // sharded context: an error, false / empty
    bool importKeysWire(const std::string &path) {
        if (cc->group) {
            cc->last_status = HYDIA_ERR_STATE;
            std::cerr << "Error: importKeysWire: keys are loaded into one context" << std::endl;
            return false;
        }
        return cc->check(hydia_keys_load(cc->h, path.c_str()), "importKeysWire");
    }
    std::vector<std::vector<Ciphertext>> queriesFromWire(const std::vector<uint8_t> &message) {
        if (cc->group) {
            cc->last_status = HYDIA_ERR_STATE;
            std::cerr << "Error: queriesFromWire: messages are unpacked on one context" << std::endl;
            return {};
        }
        return handlesFromWire(cc, message, "queriesFromWire");
    }
    std::vector<Ciphertext> queryFromWire(const std::vector<uint8_t> &message) {
        std::vector<std::vector<Ciphertext>> r = queriesFromWire(message);
        if (r.size() > 1) {
            cc->last_status = HYDIA_ERR_ARG;
            std::cerr << "Error: queryFromWire takes one probe (queriesFromWire takes a batch)" << std::endl;
            return {};
        }
        return r.empty() ? std::vector<Ciphertext>{} : r[0];
    }
    // A delta message of DiagonalEnroller::updateToWire / appendToWire / serializeDBToWire into this sender's database
    // (hydia_db_delta_apply: every header and residue is checked first, a refused message changes nothing).  Returns the new vector
    // count, which numVectors follows; 0 on an error.  Not on a sharded context
    size_t applyDBWire(const std::vector<uint8_t> &message) { return apply_db_wire("applyDBWire", false, message); }
    // The same for a SEEDED delta of DiagonalEnroller::updateToWireSeeded / appendToWireSeeded / serializeDBToWireSeeded
    // (hydia_db_delta_apply_seeded: c0 from the message, a regenerated on the GPU; no key needed)
    size_t applyDBWireSeeded(const std::vector<uint8_t> &message) { return apply_db_wire("applyDBWireSeeded", true, message); }
    std::vector<uint8_t> resultToWire(const std::vector<Ciphertext> &result) { return toWire(cc, result); }
    // computeSimilarity's scores as one message of their first `limbs` limbs (1 or 2): the decoder reads at most two, so with 2 the
    // receiver decrypts the same doubles from a sixth of the bytes; with 1 it decodes from q_0 alone.  For resultFromWire
    std::vector<uint8_t> scoresToWire(const std::vector<Ciphertext> &scores, uint32_t limbs = 2) {
        if (scores.empty() || !scores[0] || scores[0].batch->count() != scores.size() || limbs < 1 || limbs > 2) {
            cc->last_status = HYDIA_ERR_ARG;
            std::cerr << "Error: scoresToWire takes the whole of one ciphertext batch and 1 or 2 limbs" << std::endl;
            return {};
        }
        hydia_ct *view = nullptr;
        if (!cc->check(hydia_ct_limb_prefix(cc->h, scores[0].batch->h, limbs, &view), "scoresToWire")) return {};
        std::vector<uint8_t> message = toWire(cc, split_batch(cc, view));  // (the view is freed with its batch, before `scores`)
        return message;
    }
    std::vector<uint8_t> resultToWire(const Ciphertext &result) {
        if (!result || result.batch->count() != 1) {
            cc->last_status = HYDIA_ERR_ARG;
            std::cerr << "Error: resultToWire takes one ciphertext that is its own batch, or the whole of a batch" << std::endl;
            return {};
        }
        return toWire(cc, std::vector<Ciphertext>{result});
    }
    // A plain query (an extension; hydia.h): the sender knows the probe, the database (kinds 5 / 6) stays encrypted and so does every
    // result.  encodeQuery makes exactly the plaintext DiagonalReceiver::encryptQuery encrypts — no seed, no key; the overloads return
    // what the ciphertext methods return.  No rotation key 1 .. vector_dim-1 is needed.  Not on a sharded context: an error, empty.
    Plaintext encodeQuery(std::vector<double> query) {
        if (cc->group) {
            cc->last_status = HYDIA_ERR_STATE;
            std::cerr << "Error: encodeQuery: a plain query is not served on a sharded context" << std::endl;
            return {};
        }
        query.resize(cc->info.vector_dim, 0.0);
        hydia_pt *h = nullptr;
        if (!cc->check(hydia_encode_query(cc->h, query.data(), &h), "encodeQuery")) return {};
        return Plaintext{std::make_shared<PtHandle>(cc, h)};
    }
    // one Plaintext per probe of `rows`, each what encodeQuery makes of that row: ONE library call (hydia_encode_queries_device)
    std::vector<Plaintext> encodeQueries(const DeviceRows &rows) {
        if (cc->group) {
            cc->last_status = HYDIA_ERR_STATE;
            std::cerr << "Error: encodeQueries: a plain query is not served on a sharded context" << std::endl;
            return {};
        }
        std::vector<hydia_pt *> h(rows.size() ? rows.size() : 1, nullptr);
        if (!cc->check(hydia_encode_queries_device(cc->h, &rows.d, h.data()), "encodeQueries")) return {};
        std::vector<Plaintext> r;
        for (size_t i = 0; i < rows.size(); i++) r.push_back(Plaintext{std::make_shared<PtHandle>(cc, h[i])});
        return r;
    }
    std::vector<Ciphertext> computeSimilarity(const Plaintext &query) {
        hydia_ct *out = run_pq(query, hydia_compute_similarity_pq, "computeSimilarity");
        return out ? split_batch(cc, out) : std::vector<Ciphertext>{};
    }
    Ciphertext membershipScenario(const Plaintext &query) {
        hydia_ct *out = run_pq(query, hydia_membership_scenario_pq, "membershipScenario");
        return out ? split_batch(cc, out)[0] : Ciphertext{};
    }
    std::vector<Ciphertext> indexScenario(const Plaintext &query) {
        hydia_ct *out = run_pq(query, hydia_index_scenario_pq, "indexScenario");
        return out ? split_batch(cc, out) : std::vector<Ciphertext>{};
    }
    // Several plain queries in one pass over the database (names of their own: the *Multi methods take ciphertexts).  One Plaintext
    // per query in; per query exactly what the single-query overload returns.  Not on a sharded context: an error, empty.
    std::vector<std::vector<Ciphertext>> computeSimilarityPlainMulti(const std::vector<Plaintext> &queries) {
        std::vector<std::vector<Ciphertext>> r;
        for (hydia_ct *h : run_pq_multi(queries, hydia_compute_similarity_pq_multi, "computeSimilarityPlainMulti")) r.push_back(split_batch(cc, h));
        return r;
    }
    std::vector<Ciphertext> membershipScenarioPlainMulti(const std::vector<Plaintext> &queries) {
        std::vector<Ciphertext> r;
        for (hydia_ct *h : run_pq_multi(queries, hydia_membership_scenario_pq_multi, "membershipScenarioPlainMulti")) r.push_back(split_batch(cc, h)[0]);
        return r;
    }
    std::vector<std::vector<Ciphertext>> indexScenarioPlainMulti(const std::vector<Plaintext> &queries) {
        std::vector<std::vector<Ciphertext>> r;
        for (hydia_ct *h : run_pq_multi(queries, hydia_index_scenario_pq_multi, "indexScenarioPlainMulti")) r.push_back(split_batch(cc, h));
        return r;
    }

  private:
    size_t apply_db_wire(const char *what, bool seeded, const std::vector<uint8_t> &message) {
        if (cc->group) {
            cc->last_status = HYDIA_ERR_STATE;
            std::cerr << "Error: " << what << ": database deltas are not applied on a sharded context (one per shard context)" << std::endl;
            return 0;
        }
        if (!cc->check((seeded ? hydia_db_delta_apply_seeded : hydia_db_delta_apply)(cc->h, message.data(), message.size()), what)) return 0;
        size_t cts = 0, bytes = 0;
        if (!cc->check(hydia_db_stats(cc->h, &numVectors, &cts, &bytes), what)) return 0;
        return numVectors;
    }
    // the C call of every batch method: one result handle per query, or nothing after an error (reported by check)
    template <class H>
    std::vector<hydia_ct *> batch_call(const std::vector<const H *> &in, int (*multi)(hydia_ctx *, const H *const *, uint32_t, hydia_ct **),
                                       const char *what) {
        std::vector<hydia_ct *> out(in.size(), nullptr);
        if (!cc->check(multi(cc->h, in.data(), (uint32_t)in.size(), out.data()), what)) return {};
        return out;
    }
    std::vector<hydia_ct *> run_pq_multi(const std::vector<Plaintext> &qs,
                                         int (*multi)(hydia_ctx *, const hydia_pt *const *, uint32_t, hydia_ct **), const char *what) {
        if (cc->group) {
            std::cerr << "Error: " << what << ": a plain query is not served on a sharded context" << std::endl;
            return {};
        }
        std::vector<const hydia_pt *> in;
        for (auto &q : qs) {
            if (!q) {
                std::cerr << "Error: " << what << ": empty plain query" << std::endl;
                return {};
            }
            in.push_back(q.pt->h);
        }
        return batch_call(in, multi, what);
    }
    hydia_ct *run_pq(const Plaintext &q, int (*one)(hydia_ctx *, const hydia_pt *, hydia_ct **), const char *what) {
        if (!q || cc->group) {
            std::cerr << "Error: " << what << ": " << (q ? "a plain query is not served on a sharded context" : "empty plain query") << std::endl;
            return nullptr;
        }
        hydia_ct *out = nullptr;
        return cc->check(one(cc->h, q.pt->h, &out), what) ? out : nullptr;
    }
    std::vector<hydia_ct *> run_multi(std::vector<std::vector<Ciphertext>> &qs,
                                      int (*multi)(hydia_ctx *, const hydia_ct *const *, uint32_t, hydia_ct **), const char *what) {
        if (cc->group) {
            std::cerr << "Error: " << what << " is not available on a sharded context" << std::endl;
            return {};
        }
        std::vector<const hydia_ct *> in;
        for (auto &q : qs) {
            if (q.empty() || !q[0]) {
                std::cerr << "Error: empty query ciphertext" << std::endl;
                return {};
            }
            in.push_back(q[0].batch->h);
        }
        return batch_call(in, multi, what);
    }
    hydia_ct *run(std::vector<Ciphertext> &q, int (*one)(hydia_ctx *, const hydia_ct *, hydia_ct **),
                  int (*sharded)(hydia_group *, const hydia_ct *, hydia_ct **), const char *what) {
        if (q.empty() || !q[0]) {
            std::cerr << "Error: empty query ciphertext" << std::endl;
            return nullptr;
        }
        hydia_ct *out = nullptr;
        const int code = cc->group ? sharded(cc->group, q[0].batch->h, &out) : one(cc->h, q[0].batch->h, &out);
        return cc->check(code, what) ? out : nullptr;
    }
};

// ---- include/receiver.h:17-43, include/receiver_hers.h, include/receiver_diag.h
class Receiver {
  public:
    Receiver(CryptoContext ccParam, size_t vectorParam, const uint8_t *seed32 = nullptr) : cc(std::move(ccParam)), numVectors(vectorParam) {
        role_seed(seed, seed32);
    }
    Receiver(CryptoContext ccParam, PublicKey pkParam, PrivateKey skParam, size_t vectorParam)  // include/receiver.h:20-21
        : cc(std::move(ccParam)), pk(pkParam), sk(skParam), numVectors(vectorParam) {
        role_seed(seed, nullptr);
    }
    virtual ~Receiver() = default;
    virtual std::vector<Ciphertext> encryptQuery(std::vector<double> query) = 0;
    virtual bool decryptMembership(Ciphertext &membershipCipher) = 0;
    virtual std::vector<size_t> decryptIndex(std::vector<Ciphertext> &indexCipher) = 0;

  protected:
    CryptoContext cc;
    PublicKey pk;
    PrivateKey sk;
    size_t numVectors;
    uint8_t seed[32];    // this object's sampler key (OS entropy unless supplied); nonces count up per object
    uint64_t nonce = 0;
};
// approach 4's receiver (include/receiver_hers.h:9-28); DiagonalReceiver inherits its decrypt* and overrides encryptQuery
class HersReceiver : public Receiver {
  public:
    using Receiver::Receiver;
    // src/receiver/receiver_hers.cpp:13-24: vector_dim ciphertexts, one per dimension
    std::vector<Ciphertext> encryptQuery(std::vector<double> query) override {
        hydia_ct *out = nullptr;
        if (query.size() < cc->info.vector_dim) query.resize(cc->info.vector_dim, 0.0);
        nonce += cc->info.vector_dim;
        if (!cc->check(hydia_hers_encrypt_query(cc->h, query.data(), seed, nonce, &out), "encryptQuery")) return {};
        return split_batch(cc, out);
    }
    // src/receiver/receiver_hers.cpp:26-35
    bool decryptMembership(Ciphertext &membershipCipher) override {
        if (!membershipCipher) return false;
        return OpenFHEWrapper::decryptToVector(cc, membershipCipher)[0] >= 1.0;
    }
    // src/receiver/receiver_hers.cpp:37-54
    std::vector<size_t> decryptIndex(std::vector<Ciphertext> &indexCipher) override {
        size_t batchSize = cc->GetBatchSize();
        std::vector<size_t> outputValues;
        for (size_t i = 0; i < indexCipher.size(); i++) {
            if (!indexCipher[i]) continue;
            std::vector<double> indexValues = OpenFHEWrapper::decryptToVector(cc, indexCipher[i]);
            for (size_t j = 0; j < batchSize; j++)
                if (indexValues[j] >= 1.0) outputValues.push_back(j + (i * batchSize));
        }
        return outputValues;
    }
};
using HersQueryReceiver = HersReceiver;  // round-2 name of the approach-4 receiver
class DiagonalReceiver : public HersReceiver {
  public:
    using HersReceiver::HersReceiver;
    // src/receiver/receiver_diag.cpp:13-26
    std::vector<Ciphertext> encryptQuery(std::vector<double> query) override {
        hydia_ct *out = nullptr;
        if (query.size() < cc->info.vector_dim) query.resize(cc->info.vector_dim, 0.0);
        if (!cc->check(hydia_encrypt_query(cc->h, query.data(), seed, ++nonce, &out), "encryptQuery")) return {};
        return split_batch(cc, out);
    }
    // one queryCipher per probe of `rows` (hydia_encrypt_queries_device: ONE library call), each what encryptQuery makes of that row;
    // the probes take the next rows.size() nonces of this receiver.  Not on a sharded context: an error, empty
    std::vector<std::vector<Ciphertext>> encryptQueries(const DeviceRows &rows) {
        if (cc->group) {
            cc->last_status = HYDIA_ERR_STATE;
            std::cerr << "Error: encryptQueries: rows in device memory are not taken on a sharded context" << std::endl;
            return {};
        }
        std::vector<hydia_ct *> h(rows.size() ? rows.size() : 1, nullptr);
        if (!cc->check(hydia_encrypt_queries_device(cc->h, &rows.d, seed, nonce + 1, h.data()), "encryptQueries")) return {};
        nonce += rows.size();
        std::vector<std::vector<Ciphertext>> r;
        for (size_t i = 0; i < rows.size(); i++) r.push_back(split_batch(cc, h[i]));
        return r;
    }
    // Seeded secret-key queries (hydia_encrypt_queries_seeded; hydia.h): half the bytes of encryptQuery's ciphertext — c0 and the
    // public seed c1 is the expansion of.  The error term comes from this receiver's secret sampler key and its next nonces, like
    // encryptQuery's; the PUBLIC seed is drawn fresh from the OS per call unless aSeed32 is given (a pair (aSeed, nonce) must never
    // encrypt two queries).  Needs the secret key.  Not on a sharded context: an error, an empty record
    SeededQuery encryptQueriesSeeded(const std::vector<std::vector<double>> &queries, const uint8_t *aSeed32 = nullptr) {
        const size_t dim = cc->info.vector_dim;
        std::vector<double> flat(queries.size() * dim, 0.0);
        for (size_t i = 0; i < queries.size(); i++)
            for (size_t j = 0; j < dim && j < queries[i].size(); j++) flat[i * dim + j] = queries[i][j];
        SeededQuery q;
        if (!seeded_begin(q, queries.size(), aSeed32, "encryptQueriesSeeded")) return {};
        if (!cc->check(hydia_encrypt_queries_seeded(cc->h, flat.data(), q.count, seed, q.aSeed, q.nonce0, q.c0.data()), "encryptQueriesSeeded")) return {};
        nonce += q.count;
        return q;
    }
    SeededQuery encryptQuerySeeded(std::vector<double> query, const uint8_t *aSeed32 = nullptr) {
        return encryptQueriesSeeded(std::vector<std::vector<double>>{std::move(query)}, aSeed32);
    }
    SeededQuery encryptQueriesSeeded(const DeviceRows &rows, const uint8_t *aSeed32 = nullptr) {
        SeededQuery q;
        if (!seeded_begin(q, rows.size(), aSeed32, "encryptQueriesSeeded")) return {};
        if (!cc->check(hydia_encrypt_queries_seeded_device(cc->h, &rows.d, seed, q.aSeed, q.nonce0, q.c0.data()), "encryptQueriesSeeded")) return {};
        nonce += q.count;
        return q;
    }
    // the seeded key set of CryptoContextImpl::KeyGenSeeded as it travels: the public key's b and the b halves of the relinearisation
    // key and of every rotation key the context holds (half of what hydia_export_eval_key would ship).  Empty on failure
    SeededKeys exportKeysSeeded() {
        SeededKeys k;
        if (cc->group) {
            cc->last_status = HYDIA_ERR_STATE;
            std::cerr << "Error: exportKeysSeeded: a seeded key set lives on the receiver's own context" << std::endl;
            return {};
        }
        if (!cc->check(hydia_get_key_seed(cc->h, k.aSeed), "exportKeysSeeded")) return {};
        k.publicKey.resize((size_t)cc->info.n_q * cc->info.n);
        if (!cc->check(hydia_export_public_key_seeded(cc->h, k.publicKey.data()), "exportKeysSeeded")) return {};
        for (int r = 0; r < (int)cc->info.slots; r++) {
            if (!hydia_has_eval_key(cc->h, r)) continue;
            std::vector<uint64_t> &b = k.evalKeys[r];
            b.resize(hydia_eval_key_seeded_words(cc->h));
            if (!cc->check(hydia_export_eval_key_seeded(cc->h, r, b.data()), "exportKeysSeeded")) return {};
        }
        return k;
    }
    // Wire messages (hydia.h, "wire messages"): the seeded queries above as ONE type 2 message that carries the public seed and the
    // nonce itself, c0 leaving the GPU packed; the key-set file (the public key, then the evaluation keys in ascending id: every key
    // the context holds, or the relinearisation key and `rotations`); a scenario's result back from the sender.  seeded = true ships
    // half keys and needs CryptoContextImpl::KeyGenSeeded's set.  Empty / false on failure
    std::vector<uint8_t> encryptQueriesWire(const std::vector<std::vector<double>> &queries, const uint8_t *aSeed32 = nullptr) {
        const size_t dim = cc->info.vector_dim;
        std::vector<double> flat(queries.size() * dim, 0.0);
        for (size_t i = 0; i < queries.size(); i++)
            for (size_t j = 0; j < dim && j < queries[i].size(); j++) flat[i * dim + j] = queries[i][j];
        return wire_queries(queries.size(), aSeed32, [&](const uint8_t *a, void *buf, size_t cap, size_t *n) {
            return hydia_encrypt_queries_seeded_wire(cc->h, flat.data(), queries.size(), seed, a, nonce + 1, buf, cap, n);
        });
    }
    std::vector<uint8_t> encryptQueryWire(std::vector<double> query, const uint8_t *aSeed32 = nullptr) {
        return encryptQueriesWire(std::vector<std::vector<double>>{std::move(query)}, aSeed32);
    }
    std::vector<uint8_t> encryptQueriesWire(const DeviceRows &rows, const uint8_t *aSeed32 = nullptr) {
        return wire_queries(rows.size(), aSeed32, [&](const uint8_t *a, void *buf, size_t cap, size_t *n) {
            return hydia_encrypt_queries_seeded_wire_device(cc->h, &rows.d, seed, a, nonce + 1, buf, cap, n);
        });
    }
    bool exportKeysWire(const std::string &path, bool seeded = true, const std::vector<int> &rotations = {}) {
        if (cc->group) {
            cc->last_status = HYDIA_ERR_STATE;
            std::cerr << "Error: exportKeysWire: a key set lives on the receiver's own context" << std::endl;
            return false;
        }
        if (rotations.empty()) return cc->check(hydia_keys_save(cc->h, path.c_str(), seeded ? 1 : 0), "exportKeysWire");
        std::map<int, bool> ids{{0, true}};
        for (int r : rotations) ids[(int)((((long)r % (long)cc->info.slots) + (long)cc->info.slots) % (long)cc->info.slots)] = true;
        FILE *f = std::fopen(path.c_str(), "wb");
        if (!f) {
            cc->last_status = HYDIA_ERR_ARG;
            std::cerr << "Error: exportKeysWire: cannot open " << path << std::endl;
            return false;
        }
        const uint32_t head[2] = {1u, (uint32_t)ids.size() + 1u};  // the key-set file header: magic, version, number of messages
        bool ok = std::fwrite("HYDKEYS1", 1, 8, f) == 8 && std::fwrite(head, sizeof head, 1, f) == 1;
        std::vector<uint8_t> buf(std::max(hydia_wire_eval_key_bytes(cc->h, seeded), hydia_wire_public_key_bytes(cc->h, seeded)));
        ids[-1] = true;  // (sorts first: the public key)
        for (auto it = ids.begin(); ok && it != ids.end(); ++it) {
            size_t n = 0;
            ok = cc->check(hydia_key_to_wire(cc->h, it->first, seeded ? 1 : 0, buf.data(), buf.size(), &n), "exportKeysWire") &&
                 std::fwrite(buf.data(), 1, n, f) == n;
        }
        std::fclose(f);
        return ok;
    }
    std::vector<Ciphertext> resultFromWire(const std::vector<uint8_t> &message) { return fromWire(cc, message); }
    // Candidate lists and matches (an extension; hydia.h) from computeSimilarity's scores, selected on the GPU behind the decoder: only
    // the entries asked for reach the host.  Index j + i * slots is slot j of ciphertext i, decryptIndex's rule.  nVectors restricts the
    // search to the first nVectors slots (0: all) and keeps the padding slots of the last block out of a top-k.  The receiver sees
    // every score here, as with decryptToVector; indexScenario + decryptIndex stays the path that reveals only matches.
    // A Candidates is empty with total 0 on failure (cc->last_status says why)
    struct Candidates {
        std::vector<size_t> index;
        std::vector<double> value;
        size_t total = 0;  // matches: how many slots are at or above the threshold (index holds at most cap of them); top-k: index.size()
    };
    // the slots >= threshold in ascending index order, at most cap of them (0: all), with their scores
    Candidates decryptMatches(std::vector<Ciphertext> &scores, double threshold, size_t nVectors = 0, size_t cap = 0) {
        std::vector<std::vector<Ciphertext>> one{scores};
        std::vector<Candidates> r = decryptMatchesMulti(one, threshold, nVectors, cap);
        return r.empty() ? Candidates{} : r[0];
    }
    // the k best slots by score descending, ties by ascending index (-0.0 ties with +0.0, a NaN ranks last)
    Candidates decryptTopK(std::vector<Ciphertext> &scores, size_t k, size_t nVectors = 0) {
        std::vector<std::vector<Ciphertext>> one{scores};
        std::vector<Candidates> r = decryptTopKMulti(one, k, nVectors);
        return r.empty() ? Candidates{} : r[0];
    }
    // a batch of results in one library call: enqueued result after result, read back after one synchronisation
    std::vector<Candidates> decryptMatchesMulti(std::vector<std::vector<Ciphertext>> &results, double threshold, size_t nVectors = 0, size_t cap = 0) {
        std::vector<const hydia_ct *> h;
        size_t most = 0;
        if (!result_handles(results, h, most, "decryptMatchesMulti")) return {};
        if (cap == 0) cap = nVectors ? nVectors : most;
        const size_t R = h.size();
        std::vector<size_t> idx(R * cap), n(R);
        std::vector<double> val(R * cap);
        if (!cc->check(hydia_decrypt_matches_multi(cc->h, h.data(), (uint32_t)R, nVectors, threshold, idx.data(), val.data(), cap, n.data()),
                       "decryptMatchesMulti"))
            return {};
        return rows_of(idx, val, n, cap, true);
    }
    std::vector<Candidates> decryptTopKMulti(std::vector<std::vector<Ciphertext>> &results, size_t k, size_t nVectors = 0) {
        std::vector<const hydia_ct *> h;
        size_t most = 0;
        if (!result_handles(results, h, most, "decryptTopKMulti")) return {};
        if (k > most) k = most;  // (rows are k entries apart; no result has more than `most` slots)
        const size_t R = h.size();
        std::vector<size_t> idx(R * (k ? k : 1)), n(R);
        std::vector<double> val(R * (k ? k : 1));
        if (!cc->check(hydia_decrypt_topk_multi(cc->h, h.data(), (uint32_t)R, nVectors, k, idx.data(), val.data(), n.data()), "decryptTopKMulti"))
            return {};
        return rows_of(idx, val, n, k, false);
    }
    // The switching key of a re-keyed database (hydia_keygen_switch; no counterpart in the reference): from the OLD receiver's secret
    // (oldSecret, [n_q+n_p][N] as hydia_export_secret_key gives it) to THIS receiver's, for DiagonalEnroller::rekeyDB.  Treat it like an
    // evaluation key.  seed32 == nullptr draws a fresh sampler key from the OS (use a fresh one per switching key).  Empty on failure.
    std::vector<uint64_t> genSwitchKey(const std::vector<uint64_t> &oldSecret, const uint8_t *seed32 = nullptr) {
        const size_t sk_words = (size_t)(cc->info.n_q + cc->info.n_p) * cc->info.n;
        if (cc->group || oldSecret.size() != sk_words) {
            cc->last_status = cc->group ? HYDIA_ERR_STATE : HYDIA_ERR_ARG;
            std::cerr << "Error: genSwitchKey: " << (cc->group ? "a switching key is generated on the receiver's own context" : "the old secret holds (n_q + n_p) N words")
                      << std::endl;
            return {};
        }
        uint8_t s[32];
        role_seed(s, seed32);
        std::vector<uint64_t> key(hydia_switch_key_words(cc->h));
        if (!cc->check(hydia_keygen_switch(cc->h, oldSecret.data(), s, key.data()), "genSwitchKey")) return {};
        return key;
    }

  private:
    // the frame of a query message of `count` probes: the public seed, the size (a NULL buffer answers HYDIA_ERR_ARG with the need),
    // the message; the probes take this receiver's next `count` nonces
    template <class Call>
    std::vector<uint8_t> wire_queries(size_t count, const uint8_t *aSeed32, Call call) {
        if (cc->group || count == 0) {
            cc->last_status = cc->group ? HYDIA_ERR_STATE : HYDIA_ERR_ARG;
            std::cerr << "Error: encryptQueriesWire: " << (cc->group ? "seeded queries are not made on a sharded context" : "no probe") << std::endl;
            return {};
        }
        uint8_t a[32];
        role_seed(a, aSeed32);
        size_t n = 0;
        const int sized = call(a, nullptr, 0, &n);
        if (n == 0) {
            cc->check(sized, "encryptQueriesWire");
            return {};
        }
        std::vector<uint8_t> buf(n);
        if (!cc->check(call(a, buf.data(), buf.size(), &n), "encryptQueriesWire")) return {};
        nonce += count;
        return buf;
    }
    // the frame of a SeededQuery of `count` probes: the public seed, this receiver's next nonce, room for c0
    bool seeded_begin(SeededQuery &q, size_t count, const uint8_t *aSeed32, const char *what) {
        if (cc->group || count == 0) {
            cc->last_status = cc->group ? HYDIA_ERR_STATE : HYDIA_ERR_ARG;
            std::cerr << "Error: " << what << ": " << (cc->group ? "seeded queries are not made on a sharded context" : "no probe") << std::endl;
            return false;
        }
        role_seed(q.aSeed, aSeed32);
        q.nonce0 = nonce + 1;
        q.count = count;
        q.c0.resize(count * (size_t)cc->info.n_q * cc->info.n);
        return true;
    }
    // the batch handle of every result (each the whole of one device batch) and the slots of the largest
    bool result_handles(const std::vector<std::vector<Ciphertext>> &results, std::vector<const hydia_ct *> &h, size_t &most, const char *what) {
        bool ok = !cc->group && !results.empty();
        for (size_t r = 0; ok && r < results.size(); r++) {
            ok = !results[r].empty() && (bool)results[r][0] && results[r][0].batch->count() == results[r].size();
            if (ok) {
                h.push_back(results[r][0].batch->h);
                most = std::max(most, results[r].size() * (size_t)cc->info.slots);
            }
        }
        if (!ok) {
            cc->last_status = cc->group ? HYDIA_ERR_STATE : HYDIA_ERR_ARG;
            std::cerr << "Error: " << what << ": "
                      << (cc->group ? "candidate lists are decrypted on one context" : "every result is the whole of one ciphertext batch") << std::endl;
        }
        return ok;
    }
    std::vector<Candidates> rows_of(const std::vector<size_t> &idx, const std::vector<double> &val, const std::vector<size_t> &n, size_t stride,
                                    bool counted) {
        std::vector<Candidates> out(n.size());
        for (size_t r = 0; r < n.size(); r++) {
            const size_t w = std::min(n[r], stride);
            out[r].index.assign(idx.begin() + r * stride, idx.begin() + r * stride + w);
            out[r].value.assign(val.begin() + r * stride, val.begin() + r * stride + w);
            out[r].total = counted ? n[r] : w;
        }
        return out;
    }
};

// ---- enrollers.  Randomness: without a caller-supplied seed EVERY serializeDB call draws a fresh sampler key from the OS (the
// database nonces restart at the same base on every call, so a key must never serve two enrolments: ct2 - ct1 would be the
// plaintext difference); with a supplied seed (reproducible tests) a second enrolment on the same object is refused.
class EnrollerBase {
  protected:
    EnrollerBase(CryptoContext ccParam, PublicKey pkParam, size_t vectorParam, const uint8_t *seed32)
        : cc(std::move(ccParam)), pk(pkParam), numVectors(vectorParam), own_seed(seed32 == nullptr) {
        if (seed32) role_seed(seed, seed32);
    }
    bool next_seed(const char *what) {
        if (own_seed) {
            role_seed(seed, nullptr);
        } else if (enrolled) {
            cc->last_status = HYDIA_ERR_STATE;
            std::cerr << "Error: " << what << ": a caller-supplied seed enrols ONE database; construct a new enroller" << std::endl;
            return false;
        }
        enrolled = true;
        return true;
    }
    std::vector<double> flatten(const std::vector<std::vector<double>> &database) const {
        const size_t dim = cc->info.vector_dim;
        std::vector<double> flat(numVectors * dim, 0.0);
        for (size_t i = 0; i < numVectors && i < database.size(); i++)
            for (size_t j = 0; j < dim && j < database[i].size(); j++) flat[i * dim + j] = database[i][j];
        return flat;
    }
    void write_back(const std::vector<double> &flat, std::vector<std::vector<double>> &database) const {  // normalised in place
        const size_t dim = cc->info.vector_dim;
        for (size_t i = 0; i < numVectors && i < database.size(); i++)
            for (size_t j = 0; j < dim && j < database[i].size(); j++) database[i][j] = flat[i * dim + j];
    }
    CryptoContext cc;
    PublicKey pk;
    size_t numVectors;
    uint8_t seed[32] = {};
    bool own_seed, enrolled = false;
};
// ---- include/enroller_diag.h:7-27
class DiagonalEnroller : public EnrollerBase {
  public:
    DiagonalEnroller(CryptoContext ccParam, size_t vectorParam, const uint8_t *seed32 = nullptr)
        : EnrollerBase(std::move(ccParam), PublicKey{}, vectorParam, seed32) {}
    DiagonalEnroller(CryptoContext ccParam, PublicKey pkParam, size_t vectorParam)  // src/main.cpp:246
        : EnrollerBase(std::move(ccParam), pkParam, vectorParam, nullptr) {}
    // src/enroller/enroller_diag.cpp:12-53 — normalises `database` in place; ciphertexts go to HBM, not to
    // serial/db_diagonal/index<t>.bin
    void serializeDB(std::vector<std::vector<double>> &database) {
        if (!next_seed("serializeDB")) return;
        std::vector<double> flat = flatten(database);
        if (!cc->check(cc->group ? hydia_group_db_enroll(cc->group, flat.data(), numVectors, seed)
                                 : hydia_db_enroll(cc->h, flat.data(), numVectors, seed),
                       "serializeDB"))
            return;
        write_back(flat, database);
    }
    // In-place update of the enrolled database (hydia_db_update; no counterpart in the reference, which re-enrols): a fresh
    // encryption of `rows` placed at vectors first_vector .. is ADDED to the resident blocks they touch.  append: appendDB; remove:
    // the negated template with normalise = true; replace: new_normalised - old_normalised with normalise = false.  Normalised rows are
    // written back like serializeDB's.  seed32 == nullptr (the default) draws a fresh sampler key from the OS for this call; a
    // supplied seed must NEVER have been used on this database before (not by serializeDB, not by an earlier update).  numVectors
    // follows the database; senders and receivers constructed for the old count are rebuilt by the caller.
    bool updateRows(size_t first_vector, std::vector<std::vector<double>> &rows, bool normalise = true, const uint8_t *seed32 = nullptr) {
        if (cc->group) {
            cc->last_status = HYDIA_ERR_STATE;
            std::cerr << "Error: updateRows: a sharded database is updated shard by shard (hydia_db_update_shard)" << std::endl;
            return false;
        }
        const size_t dim = cc->info.vector_dim;
        std::vector<double> flat(rows.size() * dim, 0.0);
        for (size_t i = 0; i < rows.size(); i++)
            for (size_t j = 0; j < dim && j < rows[i].size(); j++) flat[i * dim + j] = rows[i][j];
        uint8_t s[32];
        role_seed(s, seed32);
        if (!cc->check(hydia_db_update(cc->h, first_vector, flat.data(), rows.size(), normalise ? 1 : 0, s), "updateRows")) return false;
        for (size_t i = 0; i < rows.size(); i++)
            for (size_t j = 0; j < dim && j < rows[i].size(); j++) rows[i][j] = flat[i * dim + j];
        if (first_vector + rows.size() > numVectors) numVectors = first_vector + rows.size();
        return true;
    }
    bool appendDB(std::vector<std::vector<double>> &rows, const uint8_t *seed32 = nullptr) { return updateRows(numVectors, rows, true, seed32); }
    // The same from rows in device memory (hydia_db_enroll_device / hydia_db_update_device): normalised on the device, never written.
    // Not on a sharded context
    void serializeDB(const DeviceRows &database) {
        if (!device_rows_ok("serializeDB", database.size() == numVectors) || !next_seed("serializeDB")) return;
        cc->check(hydia_db_enroll_device(cc->h, &database.d, seed), "serializeDB");
    }
    bool updateRows(size_t first_vector, const DeviceRows &rows, bool normalise = true, const uint8_t *seed32 = nullptr) {
        if (!device_rows_ok("updateRows", true)) return false;
        uint8_t s[32];
        role_seed(s, seed32);
        if (!cc->check(hydia_db_update_device(cc->h, first_vector, &rows.d, normalise ? 1 : 0, s), "updateRows")) return false;
        if (first_vector + rows.size() > numVectors) numVectors = first_vector + rows.size();
        return true;
    }
    bool appendDB(const DeviceRows &rows, const uint8_t *seed32 = nullptr) { return updateRows(numVectors, rows, true, seed32); }
    // Database deltas (an extension; hydia.h): updateRows / appendDB / serializeDB for a database that lies on ANOTHER machine.  This
    // enroller's context holds the public key and nothing else; the message goes to DiagonalSender::applyDBWire, which leaves the
    // sender's database bit for bit what updateRows with the same arguments would.  babies = the form of the sender's database
    // (0: vector_dim, the hoisted form); first_block = the nonce offset of a shard's first block.  Nothing resident here is touched;
    // numVectors follows as in updateRows.  The seed rule is updateRows'.  Not on a sharded context: an error, empty
    std::vector<uint8_t> updateToWire(size_t first_vector, std::vector<std::vector<double>> &rows, bool normalise = true,
                                      const uint8_t *seed32 = nullptr, int babies = 0, size_t first_block = 0) {
        return rows_to_wire("updateToWire", false, first_vector, rows, normalise, seed32, nullptr, babies, first_block);
    }
    std::vector<uint8_t> updateToWire(size_t first_vector, const DeviceRows &rows, bool normalise = true, const uint8_t *seed32 = nullptr,
                                      int babies = 0, size_t first_block = 0) {
        return delta_to_wire("updateToWire", false, first_vector, nullptr, &rows.d, rows.size(), normalise, seed32, nullptr, babies, first_block);
    }
    // append `rows` after the n_resident vectors the sender's database holds
    std::vector<uint8_t> appendToWire(std::vector<std::vector<double>> &rows, size_t n_resident, const uint8_t *seed32 = nullptr, int babies = 0,
                                      size_t first_block = 0) {
        return updateToWire(n_resident, rows, true, seed32, babies, first_block);
    }
    std::vector<uint8_t> appendToWire(const DeviceRows &rows, size_t n_resident, const uint8_t *seed32 = nullptr, int babies = 0, size_t first_block = 0) {
        return updateToWire(n_resident, rows, true, seed32, babies, first_block);
    }
    // serializeDB for a sender on another machine: one message per block of `slots` vectors, in order — the first enrols on an empty
    // sender context, every later one appends.  ONE seed for the whole database, as an enrolment uses (the blocks differ in their
    // nonces).  A failure: an error, and the messages made so far are dropped
    std::vector<std::vector<uint8_t>> serializeDBToWire(std::vector<std::vector<double>> &database, const uint8_t *seed32 = nullptr, int babies = 0,
                                                        size_t first_block = 0) {
        return db_to_wire("serializeDBToWire", false, database, seed32, nullptr, babies, first_block);
    }
    // Seeded database deltas (an extension; hydia.h): the ToWire methods for an enroller whose context holds the SECRET key — an owner
    // who is also the receiver.  Only the c0 halves travel: half the bytes; the message goes to DiagonalSender::applyDBWireSeeded.
    // seed32 (secret, the noise): updateRows' rule.  a_seed32 (PUBLIC, travels in the message; nullptr: a fresh hydia_random_seed) must
    // never have served a query under this key or another delta on that database, and must differ from seed32
    std::vector<uint8_t> updateToWireSeeded(size_t first_vector, std::vector<std::vector<double>> &rows, bool normalise = true,
                                            const uint8_t *seed32 = nullptr, const uint8_t *a_seed32 = nullptr, int babies = 0,
                                            size_t first_block = 0) {
        return rows_to_wire("updateToWireSeeded", true, first_vector, rows, normalise, seed32, a_seed32, babies, first_block);
    }
    std::vector<uint8_t> updateToWireSeeded(size_t first_vector, const DeviceRows &rows, bool normalise = true, const uint8_t *seed32 = nullptr,
                                            const uint8_t *a_seed32 = nullptr, int babies = 0, size_t first_block = 0) {
        return delta_to_wire("updateToWireSeeded", true, first_vector, nullptr, &rows.d, rows.size(), normalise, seed32, a_seed32, babies, first_block);
    }
    std::vector<uint8_t> appendToWireSeeded(std::vector<std::vector<double>> &rows, size_t n_resident, const uint8_t *seed32 = nullptr,
                                            const uint8_t *a_seed32 = nullptr, int babies = 0, size_t first_block = 0) {
        return updateToWireSeeded(n_resident, rows, true, seed32, a_seed32, babies, first_block);
    }
    std::vector<uint8_t> appendToWireSeeded(const DeviceRows &rows, size_t n_resident, const uint8_t *seed32 = nullptr,
                                            const uint8_t *a_seed32 = nullptr, int babies = 0, size_t first_block = 0) {
        return updateToWireSeeded(n_resident, rows, true, seed32, a_seed32, babies, first_block);
    }
    // one message per block, in order; ONE seed and ONE a_seed for the whole database (the blocks differ in their nonces)
    std::vector<std::vector<uint8_t>> serializeDBToWireSeeded(std::vector<std::vector<double>> &database, const uint8_t *seed32 = nullptr,
                                                              const uint8_t *a_seed32 = nullptr, int babies = 0, size_t first_block = 0) {
        return db_to_wire("serializeDBToWireSeeded", true, database, seed32, a_seed32, babies, first_block);
    }
    // Re-key the enrolled database in place under a new receiver key (hydia_db_rekey; no counterpart in the reference, which re-enrols):
    // every resident ciphertext is key-switched with `key`, the NEW receiver's DiagonalReceiver::genSwitchKey.  Afterwards the caller
    // imports the new receiver's evaluation and public keys; later updateRows / appendDB calls encrypt under the new public key.
    bool rekeyDB(const std::vector<uint64_t> &key) {
        if (cc->group) {
            cc->last_status = HYDIA_ERR_STATE;
            std::cerr << "Error: rekeyDB: a sharded database is re-keyed shard by shard (hydia_db_rekey on every hydia_group_ctx)" << std::endl;
            return false;
        }
        if (key.size() != hydia_switch_key_words(cc->h)) {
            cc->last_status = HYDIA_ERR_ARG;
            std::cerr << "Error: rekeyDB: the switching key holds dnum * 2 * (n_q + n_p) * N words" << std::endl;
            return false;
        }
        return cc->check(hydia_db_rekey(cc->h, key.data()), "rekeyDB");
    }
    size_t size() const { return numVectors; }

  private:
    bool delta_ok(const char *what) {
        if (cc->group) {
            cc->last_status = HYDIA_ERR_STATE;
            std::cerr << "Error: " << what << ": database deltas are not made on a sharded context (one per shard context, with its first_block)" << std::endl;
            return false;
        }
        return true;
    }
    // one delta message, whole (hydia_db_delta_make[_device]) or seeded (hydia_db_delta_make_seeded[_device]: the public a_seed is
    // a_seed32 or freshly drawn), of n rows in host memory (flat) or in device memory (dev)
    std::vector<uint8_t> delta_to_wire(const char *what, bool seeded, size_t first_vector, double *flat, const hydia_dev_rows *dev, size_t n,
                                       bool normalise, const uint8_t *seed32, const uint8_t *a_seed32, int babies, size_t first_block) {
        if (!delta_ok(what)) return {};
        uint8_t s[32], a[32];
        role_seed(s, seed32);
        if (seeded) role_seed(a, a_seed32);
        const int B = babies ? babies : (int)cc->info.vector_dim, norm = normalise ? 1 : 0;
        size_t need = 0, len = 0;
        if (!cc->check(seeded ? hydia_db_delta_seeded_bytes(cc->h, first_vector, n, &need) : hydia_db_delta_bytes(cc->h, first_vector, n, &need), what))
            return {};
        std::vector<uint8_t> message(need);
        uint8_t *buf = message.data();
        int status;
        if (seeded)
            status = dev ? hydia_db_delta_make_seeded_device(cc->h, first_vector, dev, norm, s, a, B, first_block, buf, need, &len)
                         : hydia_db_delta_make_seeded(cc->h, first_vector, flat, n, norm, s, a, B, first_block, buf, need, &len);
        else
            status = dev ? hydia_db_delta_make_device(cc->h, first_vector, dev, norm, s, B, first_block, buf, need, &len)
                         : hydia_db_delta_make(cc->h, first_vector, flat, n, norm, s, B, first_block, buf, need, &len);
        if (!cc->check(status, what)) return {};
        message.resize(len);
        if (first_vector + n > numVectors) numVectors = first_vector + n;
        return message;
    }
    // the same from host rows, which are padded to vector_dim on the way in and take the normalised values on the way out
    std::vector<uint8_t> rows_to_wire(const char *what, bool seeded, size_t first_vector, std::vector<std::vector<double>> &rows, bool normalise,
                                      const uint8_t *seed32, const uint8_t *a_seed32, int babies, size_t first_block) {
        const size_t dim = cc->info.vector_dim;
        std::vector<double> flat(rows.size() * dim, 0.0);
        for (size_t i = 0; i < rows.size(); i++)
            for (size_t j = 0; j < dim && j < rows[i].size(); j++) flat[i * dim + j] = rows[i][j];
        std::vector<uint8_t> message = delta_to_wire(what, seeded, first_vector, flat.data(), nullptr, rows.size(), normalise, seed32, a_seed32, babies, first_block);
        if (message.empty()) return {};
        for (size_t i = 0; i < rows.size(); i++)
            for (size_t j = 0; j < dim && j < rows[i].size(); j++) rows[i][j] = flat[i * dim + j];
        return message;
    }
    // one message per block of `slots` vectors, in order, under ONE seed (and ONE a_seed) for the whole database
    std::vector<std::vector<uint8_t>> db_to_wire(const char *what, bool seeded, std::vector<std::vector<double>> &database, const uint8_t *seed32,
                                                 const uint8_t *a_seed32, int babies, size_t first_block) {
        if (!delta_ok(what)) return {};
        uint8_t s[32], a[32];
        role_seed(s, seed32);
        if (seeded) role_seed(a, a_seed32);
        const size_t slots = cc->info.slots;
        std::vector<std::vector<uint8_t>> messages;
        for (size_t lo = 0; lo < database.size(); lo += slots) {
            const size_t hi = std::min(database.size(), lo + slots);
            std::vector<std::vector<double>> rows(database.begin() + lo, database.begin() + hi);
            messages.push_back(rows_to_wire(seeded ? "updateToWireSeeded" : "updateToWire", seeded, lo, rows, true, s, seeded ? a : nullptr, babies, first_block));
            if (messages.back().empty()) return {};
            std::copy(rows.begin(), rows.end(), database.begin() + lo);
        }
        numVectors = database.size();
        return messages;
    }
    bool device_rows_ok(const char *what, bool count_ok) {
        if (cc->group || !count_ok) {
            cc->last_status = cc->group ? HYDIA_ERR_STATE : HYDIA_ERR_ARG;
            std::cerr << "Error: " << what << ": "
                      << (cc->group ? "rows in device memory are not taken on a sharded context" : "the rows are not the enroller's number of vectors") << std::endl;
            return false;
        }
        return true;
    }
};

// ---- a plain gallery (database kinds 7 / 8; an extension with no counterpart in the reference): the operator of the sender owns the
// templates, so they are ENCODED, not encrypted — DiagonalEnroller's constructor shape, serializeDB with no seed (nothing is sampled).
// DiagonalSender and DiagonalReceiver are used unchanged.  Trust model (include/hydia.h): the sender sees the gallery; the query
// and the result stay encrypted under the receiver's key; no circuit privacy is claimed.  A sharded context is refused.
class PlainEnroller {
  public:
    PlainEnroller(CryptoContext ccParam, size_t vectorParam) : cc(std::move(ccParam)), numVectors(vectorParam) {}
    PlainEnroller(CryptoContext ccParam, PublicKey, size_t vectorParam) : cc(std::move(ccParam)), numVectors(vectorParam) {}
    // normalises `database` in place like DiagonalEnroller::serializeDB; the form follows hydia_set_matvec
    void serializeDB(std::vector<std::vector<double>> &database) {
        if (cc->group) {
            cc->last_status = HYDIA_ERR_STATE;
            std::cerr << "Error: serializeDB: a plain gallery (kind 7 / 8) is not enrolled on a sharded context" << std::endl;
            return;
        }
        const size_t dim = cc->info.vector_dim;
        std::vector<double> flat(numVectors * dim, 0.0);
        for (size_t i = 0; i < numVectors && i < database.size(); i++)
            for (size_t j = 0; j < dim && j < database[i].size(); j++) flat[i * dim + j] = database[i][j];
        if (!cc->check(hydia_plain_db_enroll(cc->h, flat.data(), numVectors), "serializeDB")) return;
        for (size_t i = 0; i < numVectors && i < database.size(); i++)
            for (size_t j = 0; j < dim && j < database[i].size(); j++) database[i][j] = flat[i * dim + j];
    }
    // In-place update of the gallery (hydia_plain_db_update): DiagonalEnroller::updateRows without the seed — the ENCODED image of
    // `rows` placed at vectors first_vector .. is added to the resident blocks they touch.  append: appendDB; remove: the negated
    // template with normalise = true (the same rows negated restore an existing block bit for bit); replace: new_normalised -
    // old_normalised with normalise = false.  Normalised rows are written back like serializeDB's.  numVectors follows the gallery;
    // senders and receivers constructed for the old count are rebuilt by the caller.
    bool updateRows(size_t first_vector, std::vector<std::vector<double>> &rows, bool normalise = true) {
        if (cc->group) {
            cc->last_status = HYDIA_ERR_STATE;
            std::cerr << "Error: updateRows: a plain gallery (kind 7 / 8) is not served on a sharded context" << std::endl;
            return false;
        }
        const size_t dim = cc->info.vector_dim;
        std::vector<double> flat(rows.size() * dim, 0.0);
        for (size_t i = 0; i < rows.size(); i++)
            for (size_t j = 0; j < dim && j < rows[i].size(); j++) flat[i * dim + j] = rows[i][j];
        if (!cc->check(hydia_plain_db_update(cc->h, first_vector, flat.data(), rows.size(), normalise ? 1 : 0), "updateRows")) return false;
        for (size_t i = 0; i < rows.size(); i++)
            for (size_t j = 0; j < dim && j < rows[i].size(); j++) rows[i][j] = flat[i * dim + j];
        if (first_vector + rows.size() > numVectors) numVectors = first_vector + rows.size();
        return true;
    }
    bool appendDB(std::vector<std::vector<double>> &rows) { return updateRows(numVectors, rows, true); }
    // The same from rows in device memory (hydia_plain_db_enroll_device / hydia_plain_db_update_device): normalised on the device,
    // never written
    void serializeDB(const DeviceRows &database) {
        if (!device_rows_ok("serializeDB", database.size() == numVectors)) return;
        cc->check(hydia_plain_db_enroll_device(cc->h, &database.d), "serializeDB");
    }
    bool updateRows(size_t first_vector, const DeviceRows &rows, bool normalise = true) {
        if (!device_rows_ok("updateRows", true)) return false;
        if (!cc->check(hydia_plain_db_update_device(cc->h, first_vector, &rows.d, normalise ? 1 : 0), "updateRows")) return false;
        if (first_vector + rows.size() > numVectors) numVectors = first_vector + rows.size();
        return true;
    }
    bool appendDB(const DeviceRows &rows) { return updateRows(numVectors, rows, true); }
    size_t size() const { return numVectors; }

  private:
    bool device_rows_ok(const char *what, bool count_ok) {
        if (cc->group || !count_ok) {
            cc->last_status = cc->group ? HYDIA_ERR_STATE : HYDIA_ERR_ARG;
            std::cerr << "Error: " << what << ": "
                      << (cc->group ? "a plain gallery (kind 7 / 8) is not served on a sharded context" : "the rows are not the enroller's number of vectors") << std::endl;
            return false;
        }
        return true;
    }
    CryptoContext cc;
    size_t numVectors;
};

// ---- HERS, approach 4: include/sender_hers.h:9-44, include/receiver_hers.h:9-28, include/enroller_hers.h:16-37.
// The query is vector_dim ciphertexts (one batch handle, split per element like the reference's vector).
class HersSender : public Sender {
  public:
    HersSender(CryptoContext ccParam, size_t vectorParam) : Sender(std::move(ccParam), vectorParam) {}
    HersSender(CryptoContext ccParam, PublicKey pkParam, size_t vectorParam) : Sender(std::move(ccParam), pkParam, vectorParam) {}
    std::vector<Ciphertext> computeSimilarity(std::vector<Ciphertext> &queryCipher) override {
        hydia_ct *out = nullptr;
        if (queryCipher.empty() || !queryCipher[0] ||
            !cc->check(hydia_hers_compute_similarity(cc->h, queryCipher[0].batch->h, &out), "computeSimilarity"))
            return {};
        return split_batch(cc, out);
    }
    Ciphertext membershipScenario(std::vector<Ciphertext> &queryCipher) override {
        hydia_ct *out = nullptr;
        if (queryCipher.empty() || !queryCipher[0] ||
            !cc->check(hydia_hers_membership_scenario(cc->h, queryCipher[0].batch->h, &out), "membershipScenario"))
            return Ciphertext{};
        return split_batch(cc, out)[0];
    }
    std::vector<Ciphertext> indexScenario(std::vector<Ciphertext> &queryCipher) override {
        hydia_ct *out = nullptr;
        if (queryCipher.empty() || !queryCipher[0] ||
            !cc->check(hydia_hers_index_scenario(cc->h, queryCipher[0].batch->h, &out), "indexScenario"))
            return {};
        return split_batch(cc, out);
    }
};
class HersEnroller : public EnrollerBase {  // include/enroller_hers.h:16-37
  public:
    HersEnroller(CryptoContext ccParam, size_t vectorParam, const uint8_t *seed32 = nullptr)
        : EnrollerBase(std::move(ccParam), PublicKey{}, vectorParam, seed32) {}
    HersEnroller(CryptoContext ccParam, PublicKey pkParam, size_t vectorParam)  // src/main.cpp:243
        : EnrollerBase(std::move(ccParam), pkParam, vectorParam, nullptr) {}
    void serializeDB(std::vector<std::vector<double>> &database) {  // enroller_hers.cpp:40-93
        if (!next_seed("serializeDB")) return;
        std::vector<double> flat = flatten(database);
        if (!cc->check(hydia_hers_db_enroll(cc->h, flat.data(), numVectors, seed), "serializeDB")) return;
        write_back(flat, database);
    }
};

// ---- the literature baseline, approach 1: include/sender_base.h (derives from HersSender), include/receiver_base.h (from
// HersReceiver), include/enroller_base.h.  The query is ONE ciphertext; the database is row-packed (hydia_base_db_enroll).
class BaseSender : public HersSender {
  public:
    BaseSender(CryptoContext ccParam, size_t vectorParam) : HersSender(std::move(ccParam), vectorParam) {}
    BaseSender(CryptoContext ccParam, PublicKey pkParam, size_t vectorParam) : HersSender(std::move(ccParam), pkParam, vectorParam) {}  // sender_base.cpp:7-9
    std::vector<Ciphertext> computeSimilarity(std::vector<Ciphertext> &queryCipher) override {  // sender_base.cpp:13-27
        hydia_ct *out = run(queryCipher, hydia_base_compute_similarity, "computeSimilarity");
        return out ? split_batch(cc, out) : std::vector<Ciphertext>{};
    }
    Ciphertext membershipScenario(std::vector<Ciphertext> &queryCipher) override {  // sender_base.cpp:50-66
        hydia_ct *out = run(queryCipher, hydia_base_membership_scenario, "membershipScenario");
        return out ? split_batch(cc, out)[0] : Ciphertext{};
    }
    std::vector<Ciphertext> indexScenario(std::vector<Ciphertext> &queryCipher) override {  // sender_base.cpp:69-81
        hydia_ct *out = run(queryCipher, hydia_base_index_scenario, "indexScenario");
        return out ? split_batch(cc, out) : std::vector<Ciphertext>{};
    }

  protected:
    hydia_ct *run(std::vector<Ciphertext> &q, int (*fn)(hydia_ctx *, const hydia_ct *, hydia_ct **), const char *what) {
        hydia_ct *out = nullptr;
        if (q.empty() || !q[0]) {
            std::cerr << "Error: empty query ciphertext" << std::endl;
            return nullptr;
        }
        return cc->check(fn(cc->h, q[0].batch->h, &out), what) ? out : nullptr;
    }
};
class BaseReceiver : public HersReceiver {
  public:
    using HersReceiver::HersReceiver;
    // src/receiver/receiver_base.cpp:13-26: normalise, tile to all slots, one ciphertext
    std::vector<Ciphertext> encryptQuery(std::vector<double> query) override {
        hydia_ct *out = nullptr;
        if (query.size() < cc->info.vector_dim) query.resize(cc->info.vector_dim, 0.0);
        if (!cc->check(hydia_encrypt_query(cc->h, query.data(), seed, ++nonce, &out), "encryptQuery")) return {};
        return split_batch(cc, out);
    }
};
class BaseEnroller : public EnrollerBase {  // include/enroller_base.h
  public:
    BaseEnroller(CryptoContext ccParam, size_t vectorParam, const uint8_t *seed32 = nullptr)
        : EnrollerBase(std::move(ccParam), PublicKey{}, vectorParam, seed32) {}
    BaseEnroller(CryptoContext ccParam, PublicKey pkParam, size_t vectorParam) : EnrollerBase(std::move(ccParam), pkParam, vectorParam, nullptr) {}
    void serializeDB(std::vector<std::vector<double>> &database) {  // enroller_base.cpp:13-56
        if (!next_seed("serializeDB")) return;
        std::vector<double> flat = flatten(database);
        if (!cc->check(hydia_base_db_enroll(cc->h, flat.data(), numVectors, seed), "serializeDB")) return;
        write_back(flat, database);
    }
};

// ---- GROTE group testing, approach 2: include/sender_grote.h (derives from BaseSender), include/receiver_grote.h (from BaseReceiver).
// The enroller is BaseEnroller (src/main.cpp:236-238), the keys are KeyGenBaseline's, computeSimilarity is BaseSender's.
class GroteSender : public BaseSender {
  public:
    GroteSender(CryptoContext ccParam, size_t vectorParam) : BaseSender(std::move(ccParam), vectorParam) {}
    GroteSender(CryptoContext ccParam, PublicKey pkParam, size_t vectorParam) : BaseSender(std::move(ccParam), pkParam, vectorParam) {}  // sender_grote.cpp:7-9
    // sender_grote.cpp:13-36: the reference's alphaNormColumns result is never read; BaseSender's ciphertext on this chain
    Ciphertext membershipScenario(std::vector<Ciphertext> &queryCipher) override {
        hydia_ct *out = run(queryCipher, hydia_grote_membership_scenario, "membershipScenario");
        return out ? split_batch(cc, out)[0] : Ciphertext{};
    }
    // sender_grote.cpp:38-73: the row ciphertexts followed by the column ciphertexts (two device batches: their limb counts differ)
    std::vector<Ciphertext> indexScenario(std::vector<Ciphertext> &queryCipher) override {
        if (queryCipher.empty() || !queryCipher[0]) {
            std::cerr << "Error: empty query ciphertext" << std::endl;
            return {};
        }
        hydia_ct *rows = nullptr, *cols = nullptr;
        if (!cc->check(hydia_grote_index_scenario(cc->h, queryCipher[0].batch->h, &rows, &cols), "indexScenario")) return {};
        std::vector<Ciphertext> r = split_batch(cc, rows), c = split_batch(cc, cols);
        r.insert(r.end(), c.begin(), c.end());
        return r;
    }
};
class GroteReceiver : public BaseReceiver {
  public:
    using BaseReceiver::BaseReceiver;
    // receiver_grote.cpp:12-65: the vector is split by the reference's counts (:20-26); each part must be the whole of one batch
    std::vector<size_t> decryptIndex(std::vector<Ciphertext> &indexCipher) override {
        const size_t batchSize = cc->GetBatchSize(), rowLength = hydia_grote_row_length((uint32_t)batchSize), colLength = batchSize / rowLength;
        const size_t mats = (numVectors + batchSize - 1) / batchSize;
        const size_t numRowCiphers = (mats + rowLength - 1) / rowLength, numColCiphers = (mats + colLength - 1) / colLength;
        if (numRowCiphers + numColCiphers != indexCipher.size() || !indexCipher[0] || !indexCipher[numRowCiphers] ||
            indexCipher[0].batch->count() != numRowCiphers || indexCipher[numRowCiphers].batch->count() != numColCiphers) {
            std::cerr << "Error: incorrect parsing of index query results" << std::endl;
            return {};
        }
        const hydia_ct *rows = indexCipher[0].batch->h, *cols = indexCipher[numRowCiphers].batch->h;
        size_t n = 0;
        if (!cc->check(hydia_grote_decrypt_index(cc->h, rows, cols, numVectors, nullptr, 0, &n), "decryptIndex")) return {};
        std::vector<size_t> out(n);
        if (n && !cc->check(hydia_grote_decrypt_index(cc->h, rows, cols, numVectors, out.data(), n, &n), "decryptIndex")) return {};
        return out;
    }
};

// ---- the Blind-Match method, approach 3: include/sender_blind.h (derives from HersSender), include/receiver_blind.h (from HersReceiver),
// include/enroller_blind.h (from HersEnroller).  The query is K = VECTOR_DIM / CHUNK_LEN ciphertexts (one batch handle); the database is
// chunk-packed (hydia_blind_db_enroll); the keys are KeyGenBaseline's (src/main.cpp:195-206).
class BlindSender : public HersSender {
  public:
    BlindSender(CryptoContext ccParam, size_t vectorParam) : HersSender(std::move(ccParam), vectorParam) {}
    BlindSender(CryptoContext ccParam, PublicKey pkParam, size_t vectorParam) : HersSender(std::move(ccParam), pkParam, vectorParam) {}  // sender_blind.cpp:7-9
    std::vector<Ciphertext> computeSimilarity(std::vector<Ciphertext> &queryCipher) override {  // sender_blind.cpp:43-56
        hydia_ct *out = run(queryCipher, hydia_blind_compute_similarity, "computeSimilarity");
        return out ? split_batch(cc, out) : std::vector<Ciphertext>{};
    }
    Ciphertext membershipScenario(std::vector<Ciphertext> &queryCipher) override {  // sender_blind.cpp:13-28
        hydia_ct *out = run(queryCipher, hydia_blind_membership_scenario, "membershipScenario");
        return out ? split_batch(cc, out)[0] : Ciphertext{};
    }
    std::vector<Ciphertext> indexScenario(std::vector<Ciphertext> &queryCipher) override {  // sender_blind.cpp:30-41
        hydia_ct *out = run(queryCipher, hydia_blind_index_scenario, "indexScenario");
        return out ? split_batch(cc, out) : std::vector<Ciphertext>{};
    }

  protected:
    hydia_ct *run(std::vector<Ciphertext> &q, int (*fn)(hydia_ctx *, const hydia_ct *, hydia_ct **), const char *what) {
        hydia_ct *out = nullptr;
        if (q.empty() || !q[0]) {
            std::cerr << "Error: empty query ciphertext" << std::endl;
            return nullptr;
        }
        return cc->check(fn(cc->h, q[0].batch->h, &out), what) ? out : nullptr;
    }
};
class BlindReceiver : public HersReceiver {
  public:
    using HersReceiver::HersReceiver;
    // src/receiver/receiver_blind.cpp:13-26: normalise, K ciphertexts, chunk c tiled over all slots
    std::vector<Ciphertext> encryptQuery(std::vector<double> query) override {
        hydia_ct *out = nullptr;
        if (query.size() < cc->info.vector_dim) query.resize(cc->info.vector_dim, 0.0);
        const uint64_t first = nonce + 1;
        nonce += cc->info.vector_dim / CHUNK_LEN;
        if (!cc->check(hydia_blind_encrypt_query(cc->h, query.data(), CHUNK_LEN, seed, first, &out), "encryptQuery")) return {};
        return split_batch(cc, out);
    }
    // src/receiver/receiver_blind.cpp:28-54: slot j of ciphertext i -> i batchSize + j / CHUNK_LEN + (j % CHUNK_LEN) scoresPerBatch; like
    // the reference, indices in the padding past numVectors are not filtered.  The ciphertexts must be the whole of one device batch
    std::vector<size_t> decryptIndex(std::vector<Ciphertext> &indexCipher) override {
        if (indexCipher.empty() || !indexCipher[0] || indexCipher[0].batch->count() != indexCipher.size()) {
            std::cerr << "Error: decryptIndex takes the whole of one ciphertext batch" << std::endl;
            return {};
        }
        const hydia_ct *h = indexCipher[0].batch->h;
        size_t n = 0;
        if (!cc->check(hydia_blind_decrypt_index(cc->h, h, CHUNK_LEN, nullptr, 0, &n), "decryptIndex")) return {};
        std::vector<size_t> out(n);
        if (n && !cc->check(hydia_blind_decrypt_index(cc->h, h, CHUNK_LEN, out.data(), n, &n), "decryptIndex")) return {};
        return out;
    }
};
class BlindEnroller : public EnrollerBase {  // include/enroller_blind.h
  public:
    BlindEnroller(CryptoContext ccParam, size_t vectorParam, const uint8_t *seed32 = nullptr)
        : EnrollerBase(std::move(ccParam), PublicKey{}, vectorParam, seed32) {}
    BlindEnroller(CryptoContext ccParam, PublicKey pkParam, size_t vectorParam) : EnrollerBase(std::move(ccParam), pkParam, vectorParam, nullptr) {}
    void serializeDB(std::vector<std::vector<double>> &database, size_t chunkLength) {  // enroller_blind.cpp:13-62
        if (!next_seed("serializeDB")) return;
        std::vector<double> flat = flatten(database);
        if (!cc->check(hydia_blind_db_enroll(cc->h, flat.data(), numVectors, chunkLength, seed), "serializeDB")) return;
        write_back(flat, database);
    }
};

}  // namespace hydia
