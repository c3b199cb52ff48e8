// image_matching_amd/csrc/select_kernels.h — launch interface of select_kernels.hip: threshold select and top-k over decoded slots
// (include/hydia.h "candidate lists and matches").
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

// one workgroup of the count / scatter kernels owns HY_SEL_TILE consecutive elements; the scan kernel takes HY_SEL_SCAN_TRIP tile
// counts per trip of its loop (one trip covers HY_SEL_TILE * HY_SEL_SCAN_TRIP = 2^20 elements)
#define HY_SEL_TILE 1024
#define HY_SEL_SCAN_TRIP 1024
// the largest n the entries take: counts and positions are 32-bit
#define HY_SEL_MAX_N 0x7fffffffull

// the order-preserving 64-bit key of a double: a > b as doubles <=> key(a) > key(b) as unsigned integers, with -0.0 and +0.0 on ONE key
// and every NaN on key 0, below -inf (key 0x000f...f).  Shared by the kernels and by the host's final sort of the k survivors
__host__ __device__ inline uint64_t hy_sel_key(uint64_t bits) {
    if ((bits & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) return 0;       // NaN: the lowest key
    if ((bits & 0x7fffffffffffffffull) == 0) return 0x8000000000000000ull;      // both zeros
    return (bits >> 63) ? ~bits : bits | 0x8000000000000000ull;                 // negatives reversed, positives above them
}

// what the radix select of one top-k keeps in device memory (zeroed before the first pass)
struct SelState {
    uint64_t kth;        // the bytes of the k-th largest key decided so far, from the top; the key itself after the eighth pass
    unsigned want;       // how many keys are still wanted among those that share kth's decided bytes; after the eighth pass: how many
                         // keys EQUAL to kth belong to the top k (>= 1), so k - want keys lie above it
    unsigned pad;
    unsigned hist[256];  // the pass's histogram; the pick kernel leaves it zero
};

// the predicate of a compaction.  GE: v >= t as IEEE doubles, at most cap positions written.  ABOVE / TIE read st after the select:
// key(v) > kth into positions [0, k - want), key(v) == kth into [k - want, k) — the first `want` of them in index order
enum { HY_SEL_GE = 0, HY_SEL_ABOVE = 1, HY_SEL_TIE = 2 };
struct SelPred {
    int mode;
    double t;
    unsigned cap, k;
    const SelState *st;
};

namespace hc {
inline size_t select_tiles(size_t n) { return (n + HY_SEL_TILE - 1) / HY_SEL_TILE; }
// the ordered compaction in its three steps.  tiles: select_tiles(n) unsigneds (counts, then in place their exclusive scan); *total:
// the number of elements the predicate holds for.  idx_out / val_out (val_out may be null): position p receives the p-th such element
// in ascending index order; positions at or past the predicate's limit are not written
void select_count(hipStream_t st, const double *v, size_t n, const SelPred &p, unsigned *tiles);
void select_scan(hipStream_t st, unsigned *tiles, size_t ntiles, unsigned *total);
void select_scatter(hipStream_t st, const double *v, size_t n, const SelPred &p, const unsigned *tiles, uint64_t *idx_out, double *val_out);
// radix select, pass 0 .. 7 from the top byte of the key: the histogram of that byte over the keys that share kth's decided bytes,
// then the bin the want-th largest of them lies in (1 <= k <= n; pass 0 starts from want = k on a zeroed state)
void topk_hist(hipStream_t st, const double *v, size_t n, int pass, SelState *state);
void topk_pick(hipStream_t st, int pass, unsigned k, SelState *state);
}  // namespace hc
