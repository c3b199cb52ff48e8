// image_matching_amd/csrc/wire_kernels.hip — gfx950 kernels of the wire format (wire_format.h, include/hydia.h "wire messages"): residues
// packed into the bit length of their modulus on the way out, unpacked and range-checked on the way in.
//
// Pure data movement.  The unit of both kernels is the GRANULE: 64 consecutive residues of one limb = exactly w 64-bit words of the
// packed row (w = the bit length of q_j, wave-uniform, read from ModC at run time — one kernel serves every width).  One wave owns one
// granule, so no two waves ever write one word and the pack needs no atomics.  Both sides of a granule are coalesced: lane c loads /
// stores residue c (512 contiguous bytes per wave), lane k < w stores / loads word k (8 w contiguous bytes); the bit gather between
// the two goes through a 512-byte LDS tile per wave.  A word holds pieces of at most ceil(64 / w) + 1 residues (three for the 45 .. 60
// bit limbs of this library's chains); the gather loop is general in w.
#include "client_kernels.h"

#include <stdexcept>

namespace {

// rows [item][poly][limb] of N residues at src + item * item_stride + poly * poly_stride + limb * N (a limb-prefix view keeps its
// limb stride inside poly_stride; the b halves of a key skip the a halves through item_stride) -> packed rows, back to back.
// grid (N / 256, limbs, items * npoly), 4 granules per workgroup
__global__ __launch_bounds__(256) void k_wire_pack(const ModC *__restrict__ mod, int N, const u64 *__restrict__ src, size_t item_stride,
                                                   size_t poly_stride, int npoly, WireRows R, u64 *__restrict__ dst) {
    __shared__ u64 tile[4][64];
    const int j = blockIdx.y, z = blockIdx.z, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t g = (size_t)blockIdx.x * 4 + wave;
    const int w = 64 - __clzll((long long)mod[j].q);
    const u64 mask = w == 64 ? ~0ull : (1ull << w) - 1;  // a residue wider than its field must not reach its neighbour's bits
    tile[wave][lane] = src[(size_t)(z / npoly) * item_stride + (size_t)(z % npoly) * poly_stride + (size_t)j * N + g * 64 + lane] & mask;
    __syncthreads();
    if (lane < w) {
        int c = (64 * lane) / w;            // the residue bit 64 * lane of the granule belongs to
        const int off = 64 * lane - c * w;  // its bits below that one went into the word before
        u64 word = tile[wave][c] >> off;
        for (int filled = w - off; filled < 64; filled += w) word |= tile[wave][++c] << filled;
        dst[(size_t)z * R.off[gridDim.y] + R.off[j] + g * w + lane] = word;
    }
}
// the inverse, and the range check: *flag := 1 when any residue is at or above its modulus (never cleared here), in the style of
// k_db_check_canonical.  Same grid
__global__ __launch_bounds__(256) void k_wire_unpack_check(const ModC *__restrict__ mod, int N, const u64 *__restrict__ src, WireRows R,
                                                           u64 *__restrict__ dst, size_t item_stride, size_t poly_stride, int npoly,
                                                           unsigned *__restrict__ flag) {
    __shared__ u64 tile[4][64];
    const int j = blockIdx.y, z = blockIdx.z, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t g = (size_t)blockIdx.x * 4 + wave;
    const u64 q = mod[j].q;
    const int w = 64 - __clzll((long long)q);
    const u64 mask = w == 64 ? ~0ull : (1ull << w) - 1;
    if (lane < w) tile[wave][lane] = src[(size_t)z * R.off[gridDim.y] + R.off[j] + g * w + lane];
    __syncthreads();
    const int k = (lane * w) >> 6, off = (lane * w) & 63;
    u64 v = tile[wave][k] >> off;
    if (off + w > 64) v |= tile[wave][k + 1] << (64 - off);  // (off > 0 here; the last residue ends with word w - 1)
    v &= mask;
    dst[(size_t)(z / npoly) * item_stride + (size_t)(z % npoly) * poly_stride + (size_t)j * N + g * 64 + lane] = v;
    if (__syncthreads_or(v >= q) && threadIdx.x == 0) *flag = 1u;
}

}  // namespace

namespace hc {

WireRows wire_rows(const u64 *moduli, int N, int nl) {
    WireRows R{};
    if (nl < 1 || nl > HY_MAX_MODS || N < 256 || N % 256) throw std::runtime_error("hydia: wire rows: bad shape");
    for (int j = 0; j < nl; j++) R.off[j + 1] = R.off[j] + (unsigned)(N / 64) * (unsigned)(64 - __builtin_clzll(moduli[j]));
    return R;
}
// the launches take at most 65535 (item, poly) pairs each
void wire_pack(hipStream_t st, const ModC *mod, int N, const u64 *src, size_t item_stride, size_t poly_stride, size_t items, int npoly,
               int nl, const WireRows &R, u64 *dst) {
    hk::ledger_add("k_wire_pack", (double)items * npoly * ((double)nl * N * 8 + (double)R.off[nl] * 8));
    const size_t per = 65535 / (size_t)npoly;
    for (size_t i0 = 0; i0 < items; i0 += per) {
        const size_t n = items - i0 < per ? items - i0 : per;
        hipLaunchKernelGGL(k_wire_pack, dim3(N / 256, nl, (unsigned)(n * npoly)), dim3(256), 0, st, mod, N, src + i0 * item_stride, item_stride,
                           poly_stride, npoly, R, dst + i0 * npoly * R.off[nl]);
    }
}
void wire_unpack_check(hipStream_t st, const ModC *mod, int N, const u64 *src, u64 *dst, size_t item_stride, size_t poly_stride, size_t items,
                       int npoly, int nl, const WireRows &R, unsigned *flag) {
    hk::ledger_add("k_wire_unpack_check", (double)items * npoly * ((double)nl * N * 8 + (double)R.off[nl] * 8));
    const size_t per = 65535 / (size_t)npoly;
    for (size_t i0 = 0; i0 < items; i0 += per) {
        const size_t n = items - i0 < per ? items - i0 : per;
        hipLaunchKernelGGL(k_wire_unpack_check, dim3(N / 256, nl, (unsigned)(n * npoly)), dim3(256), 0, st, mod, N,
                           src + i0 * npoly * R.off[nl], R, dst + i0 * item_stride, item_stride, poly_stride, npoly, flag);
    }
}

}  // namespace hc
