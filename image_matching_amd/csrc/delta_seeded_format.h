// image_matching_amd/csrc/delta_seeded_format.h — the container of a SEEDED database delta (include/hydia.h, "seeded database deltas")
// under the names its callers use: delta_format.h's size arithmetic, header and validator on the form delta::SEEDED (described
// there).  Host only: no HIP, no library type — tests/delta_seeded_header_check.cpp includes this file, delta_format.h and
// wire_format.h alone.
#pragma once
#include "delta_format.h"

namespace hydia {
namespace delta_seeded {

using delta::block_nonce;
using delta::Expect;
using delta::Header;

inline bool total_bytes(uint32_t log_n, uint32_t n_q, const uint64_t *moduli, uint32_t vector_dim, uint64_t first_vector, uint64_t n_rows,
                        uint64_t *out) {
    return delta::total_bytes(delta::SEEDED, log_n, n_q, moduli, vector_dim, first_vector, n_rows, out);
}
inline Header make_header(uint32_t vector_dim, uint64_t babies, uint64_t first_vector, uint64_t n_rows, uint64_t first_block, uint64_t n_blocks) {
    return delta::make_header(delta::SEEDED, vector_dim, babies, first_vector, n_rows, first_block, n_blocks);
}
inline bool check(const void *buf, size_t len, const Expect *e, Header *out, uint32_t *log_n, uint8_t *a_seed, std::string *err) {
    return delta::check(delta::SEEDED, buf, len, e, out, log_n, a_seed, err);
}

}  // namespace delta_seeded
}  // namespace hydia
