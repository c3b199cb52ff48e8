// image_matching_amd/csrc/select_kernels.hip — gfx950 kernels behind the decoder: threshold select and top-k over n doubles in HBM
// (include/hydia.h "candidate lists and matches").
//
// Exact and deterministic: no output position comes from an atomic.  Both operations rest on ONE ordered compaction in three steps:
//   k_select_count    a workgroup owns a tile of HY_SEL_TILE consecutive elements (4 rounds of 256 lanes); every wave ballots its
//                     predicate, the popcounts of the tile's 16 (round, wave) cells are summed -> tiles[tile]
//   k_select_scan     one workgroup: the exclusive scan of the tile counts in place, HY_SEL_SCAN_TRIP of them per trip with the carry
//                     in a register, and the total
//   k_select_scatter  the predicate again; an element's position = tiles[tile] + the popcounts of the cells before its own (an LDS
//                     table of 16) + the number of set ballot bits below its lane (mbcnt)
// Waves are 64 lanes, __ballot is 64 bits.  Counts and positions are 32-bit (n <= 2^31 - 1).
//
// Top-k is a radix select on hy_sel_key (select_kernels.h): eight passes over the key's bytes from the top, each an LDS histogram per
// workgroup added to the state's 256 bins with integer atomics (sums of integers: the same in any order), then a one-workgroup kernel
// that picks the bin the k-th key lies in — no pass needs the host.  The k-th key known, the compaction runs twice: every key above it,
// then the first (k - that count) keys equal to it in index order.  The host sorts the k survivors.
#include "select_kernels.h"

#include <stdexcept>

#include "kernels.h"

namespace {

template <int MODE>
__device__ __forceinline__ bool sel_test(const SelPred &p, uint64_t kth, double v) {
    if (MODE == HY_SEL_GE) return v >= p.t;  // IEEE: false for a NaN, true for -0.0 >= +0.0
    const uint64_t key = hy_sel_key((uint64_t)__double_as_longlong(v));
    return MODE == HY_SEL_ABOVE ? key > kth : key == kth;
}
// exclusive scan of x over the NW waves of the workgroup, and the sum over all of them; wsum: NW unsigneds of LDS, free again on return
template <int NW>
__device__ __forceinline__ unsigned block_excl_scan(unsigned x, unsigned *wsum, unsigned &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned incl = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned y = __shfl_up(incl, d);
        if (lane >= d) incl += y;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    unsigned before = 0;
    total = 0;
    for (int w = 0; w < NW; w++) {
        const unsigned t = wsum[w];
        if (w < wave) before += t;
        total += t;
    }
    __syncthreads();
    return before + incl - x;
}

// grid (tiles), 256 lanes.  Lanes past n take part in every ballot with a false predicate
template <int MODE>
__global__ __launch_bounds__(256) void k_select_count(const double *__restrict__ v, size_t n, SelPred p, unsigned *__restrict__ tiles) {
    __shared__ unsigned cell[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t kth = MODE == HY_SEL_GE ? 0 : p.st->kth;
    const size_t i0 = (size_t)blockIdx.x * HY_SEL_TILE + threadIdx.x;
    unsigned c = 0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const size_t i = i0 + (size_t)r * 256;
        const bool hit = i < n && sel_test<MODE>(p, kth, v[i]);
        c += (unsigned)__popcll(__ballot(hit));
    }
    if (lane == 0) cell[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) tiles[blockIdx.x] = cell[0] + cell[1] + cell[2] + cell[3];
}
// one workgroup of HY_SEL_SCAN_TRIP lanes
__global__ __launch_bounds__(HY_SEL_SCAN_TRIP) void k_select_scan(unsigned *__restrict__ tiles, size_t ntiles, unsigned *__restrict__ total) {
    __shared__ unsigned wsum[HY_SEL_SCAN_TRIP / 64];
    unsigned carry = 0;
    for (size_t t0 = 0; t0 < ntiles; t0 += HY_SEL_SCAN_TRIP) {
        const size_t t = t0 + threadIdx.x;
        const unsigned x = t < ntiles ? tiles[t] : 0;
        unsigned sum;
        const unsigned ex = block_excl_scan<HY_SEL_SCAN_TRIP / 64>(x, wsum, sum);
        if (t < ntiles) tiles[t] = carry + ex;
        carry += sum;
    }
    if (threadIdx.x == 0) *total = carry;
}
// grid (tiles), 256 lanes
template <int MODE>
__global__ __launch_bounds__(256) void k_select_scatter(const double *__restrict__ v, size_t n, SelPred p, const unsigned *__restrict__ tiles,
                                                        uint64_t *__restrict__ idx_out, double *__restrict__ val_out) {
    __shared__ unsigned cell[16];  // [round][wave]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t kth = 0;
    unsigned base = 0, limit = p.cap;
    if (MODE != HY_SEL_GE) {
        kth = p.st->kth;
        const unsigned above = p.k - p.st->want;
        base = MODE == HY_SEL_TIE ? above : 0;
        limit = MODE == HY_SEL_TIE ? p.st->want : above;
    }
    const size_t i0 = (size_t)blockIdx.x * HY_SEL_TILE + threadIdx.x;
    double x[4];
    unsigned long long hits[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const size_t i = i0 + (size_t)r * 256;
        x[r] = i < n ? v[i] : 0.0;
        hits[r] = __ballot(i < n && sel_test<MODE>(p, kth, x[r]));
        if (lane == 0) cell[r * 4 + wave] = (unsigned)__popcll(hits[r]);
    }
    __syncthreads();
    unsigned before = tiles[blockIdx.x];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        for (int w = 0; w < 4; w++)
            if (w < wave) before += cell[r * 4 + w];
        if ((hits[r] >> lane) & 1ull) {
            const unsigned below = __builtin_amdgcn_mbcnt_hi((unsigned)(hits[r] >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)hits[r], 0u));
            const unsigned pos = before + below;
            if (pos < limit) {
                idx_out[base + pos] = i0 + (size_t)r * 256;
                if (val_out) val_out[base + pos] = x[r];
            }
        }
        for (int w = 0; w < 4; w++)
            if (w >= wave) before += cell[r * 4 + w];
    }
}

// grid-stride over the elements, 256 lanes.  A wave whose live lanes all fall into one bin (the usual case in the top passes, where
// scores share their sign and exponent) adds its popcount once
__global__ __launch_bounds__(256) void k_topk_hist(const double *__restrict__ v, size_t n, int pass, SelState *__restrict__ state) {
    __shared__ unsigned h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int shift = 56 - 8 * pass, lane = threadIdx.x & 63;
    const uint64_t decided = pass == 0 ? 0 : ~0ull << (shift + 8), kth = state->kth;
    const size_t stride = (size_t)gridDim.x * 256, rounds = (n + stride - 1) / stride;
    for (size_t r = 0; r < rounds; r++) {
        const size_t i = r * stride + (size_t)blockIdx.x * 256 + threadIdx.x;
        const uint64_t key = i < n ? hy_sel_key((uint64_t)__double_as_longlong(v[i])) : 0;
        const bool live = i < n && (key & decided) == (kth & decided);
        const unsigned bin = (unsigned)(key >> shift) & 255u;
        const unsigned long long m = __ballot(live);
        if (m == 0) continue;
        const unsigned first = (unsigned)__shfl((int)bin, __ffsll((long long)m) - 1);
        if (__ballot(live && bin == first) == m) {
            if (lane == 0) atomicAdd(&h[first], (unsigned)__popcll(m));
        } else if (live) {
            atomicAdd(&h[bin], 1u);
        }
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&state->hist[threadIdx.x], h[threadIdx.x]);
}
// one workgroup of 256 lanes: lane l looks at bin 255 - l, so the exclusive scan counts the keys in the bins ABOVE its own
// (pass 0 starts from want = k: the state arrives zeroed)
__global__ __launch_bounds__(256) void k_topk_pick(int pass, unsigned k, SelState *__restrict__ state) {
    __shared__ unsigned wsum[4];
    const int bin = 255 - (int)threadIdx.x;
    const unsigned here = state->hist[bin], want = pass == 0 ? k : state->want;
    unsigned sum;
    const unsigned above = block_excl_scan<4>(here, wsum, sum);
    state->hist[bin] = 0;
    if (above < want && want <= above + here) {  // exactly one lane while 1 <= want <= the keys counted
        state->kth |= (uint64_t)bin << (56 - 8 * pass);
        state->want = want - above;
    }
}

}  // namespace

namespace hc {

static unsigned tiles_grid(size_t n) {
    if (n == 0 || n > HY_SEL_MAX_N) throw std::runtime_error("hydia: select: element count outside 1 .. 2^31 - 1");
    return (unsigned)select_tiles(n);
}
void select_count(hipStream_t st, const double *v, size_t n, const SelPred &p, unsigned *tiles) {
    hk::ledger_add("k_select_count", (double)n * 8 + (double)select_tiles(n) * 4);
    const dim3 g(tiles_grid(n)), b(256);
    if (p.mode == HY_SEL_GE) hipLaunchKernelGGL(k_select_count<HY_SEL_GE>, g, b, 0, st, v, n, p, tiles);
    else if (p.mode == HY_SEL_ABOVE) hipLaunchKernelGGL(k_select_count<HY_SEL_ABOVE>, g, b, 0, st, v, n, p, tiles);
    else hipLaunchKernelGGL(k_select_count<HY_SEL_TIE>, g, b, 0, st, v, n, p, tiles);
}
void select_scan(hipStream_t st, unsigned *tiles, size_t ntiles, unsigned *total) {
    hk::ledger_add("k_select_scan", (double)ntiles * 8);
    hipLaunchKernelGGL(k_select_scan, dim3(1), dim3(HY_SEL_SCAN_TRIP), 0, st, tiles, ntiles, total);
}
void select_scatter(hipStream_t st, const double *v, size_t n, const SelPred &p, const unsigned *tiles, uint64_t *idx_out, double *val_out) {
    hk::ledger_add("k_select_scatter", (double)n * 8 + (double)select_tiles(n) * 4);
    const dim3 g(tiles_grid(n)), b(256);
    if (p.mode == HY_SEL_GE) hipLaunchKernelGGL(k_select_scatter<HY_SEL_GE>, g, b, 0, st, v, n, p, tiles, idx_out, val_out);
    else if (p.mode == HY_SEL_ABOVE) hipLaunchKernelGGL(k_select_scatter<HY_SEL_ABOVE>, g, b, 0, st, v, n, p, tiles, idx_out, val_out);
    else hipLaunchKernelGGL(k_select_scatter<HY_SEL_TIE>, g, b, 0, st, v, n, p, tiles, idx_out, val_out);
}
void topk_hist(hipStream_t st, const double *v, size_t n, int pass, SelState *state) {
    hk::ledger_add("k_topk_hist", (double)n * 8);
    const size_t blocks = (n + 255) / 256;
    tiles_grid(n);
    hipLaunchKernelGGL(k_topk_hist, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, st, v, n, pass, state);
}
void topk_pick(hipStream_t st, int pass, unsigned k, SelState *state) {
    hk::ledger_add("k_topk_pick", 2.0 * 256 * 4);
    hipLaunchKernelGGL(k_topk_pick, dim3(1), dim3(256), 0, st, pass, k, state);
}

}  // namespace hc
