// image_matching_amd/csrc/ntt15_ipq.h — the relinearise + rescale product's inner product as two dependent launches whose Q-limb half
// runs in the pipeline's last pass (ntt15.hip: k_ntt15_p2_ip_tail, k_ntt15_p2_ipq).  Same results as ntt15_p2_inner_product followed by
// ntt15_forward_p2_fused (mode 3), without the accumulator's trip through memory.
#pragma once
#include "kernels.h"

namespace hk {

// the inner product's arguments as ntt15_p2_inner_product sets them (no dropped limb)
IpArgs ntt15_ip_args(int nl, int nP, int nT, int alpha, const u64 *const *keys, const u64 *key, const u64 *c2, size_t c2_xs, u64 *acc, u64 *inv_out,
                     size_t inv_outer, int inv_row0, bool per_x_keys);
// first launch: the special-prime rows and the dropped limb's row, through the first pass of their inverse transform into ip.inv_out;
// and the sums of the 60-bit limb 0 into ip.acc [2X][N]; nd = 2 or 3, drop.l = ip.nl - 1, ip.inv_row0 >= 1
void ntt15_p2_ip_tail(hipStream_t st, const NttTables &T, const u64 *dig, size_t dig_x_stride, int nd, int X, const IpArgs &ip, const DropLimb &drop);
// second launch, behind the column-fused ModDown conversion: the sums of limbs 1 .. ip.nl - 2 (all on the FP64 path) and the second pass
// of w [2X][w_outer] with the merged ModDown + Rescale epilogue `epi` (mode 3 without a product subtrahend; epi.in = limb 0's sums
// [2X][N], in_ls = 1) in one workgroup per (chunk, limb, ciphertext)
void ntt15_p2_ipq(hipStream_t st, const NttTables &T, const u64 *dig, size_t dig_x_stride, int nd, int X, const IpArgs &ip, u64 *w, size_t w_outer,
                  const NttStore &epi);

}  // namespace hk
