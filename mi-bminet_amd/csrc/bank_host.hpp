// bank_host.hpp — the HIP-free part of a parameter bank (net_bank_create, include/mibminet.h): which
// sets may share a bank, the exact-division form every slice of a mixed bank takes, and the
// partition of an epoch list over the workgroups of bank::k_forward_ep_bank (forward_bank.hpp).
// HIP-free like params_host.hpp; the kernel includes it for range_of alone.
#pragma once
#include "params_host.hpp"

#ifdef __HIPCC__
#define MIB_BANK_HD __host__ __device__
#else
#define MIB_BANK_HD
#endif

namespace mib {
namespace bank {

// The sets of a bank run one kernel instantiation on one LDS carve: C, T and N fix the carve,
// REORDER_BN and the clip the instantiation (F1 = F2 = 16 and D = 1 are the family's,
// gen_supported).  Exact division is not compared: a mixed bank takes the exact form (force_exact).
inline bool agree(const HostParams& a, const HostParams& b) {
  return a.d.C == b.d.C && a.d.T == b.d.T && a.d.N == b.d.N && a.d.F1 == b.d.F1 && a.d.F2 == b.d.F2 &&
         a.d.D == b.d.D && a.reorder_bn == b.reorder_bn && a.clip_balanced == b.clip_balanced;
}

// The first set that disagrees with set 0, or -1.
inline long first_mismatch(const HostParams* const* sets, size_t n) {
  for (size_t i = 1; i < n; i++)
    if (!agree(*sets[0], *sets[i])) return (long)i;
  return -1;
}

// The plan of a set whose float forms are all proven, as make_plan leaves one that has an unproven
// requant: no float form, the C-inits without their magic.  xdiv is exact for every divisor and
// numerator (requant_host.hpp), so the exact-division kernels compute the same logits from it, only
// slower.  (xr_layer, xr_filter) stay (0, -1): no requant of the set asked for it.
inline void force_exact(const HostParams& hp, Plan& pl) {
  if (pl.xr) return;
  pl.xr = true;
  for (int f = 0; f < F2; f++) {
    pl.f1[f] = pl.f2[f] = pl.f4[f] = FloatForm();
    pl.ci1[f] = hp.l1_offset[f];
    pl.ci2[f] = hp.l2_offset[f] >> 3;
    pl.ci4[f] = hp.l4_offset[f] >> 3;
  }
}

// Workgroup w of G takes the items [lo, hi) = [floor(w E / G), floor((w + 1) E / G)): contiguous, so
// that on a list grouped by set a workgroup changes sets at most once per set its range touches.
// The ranges of w = 0 .. G - 1 tile [0, E) in order; w E < 2^63 for every grid and every E the
// entries admit (64-bit product: w E passes 2^32 from E = 2^23 on at 512 workgroups).
struct Range64 {
  long long lo, hi;
};
MIB_BANK_HD inline Range64 range_of(unsigned w, unsigned G, unsigned long long E) {
  return Range64{(long long)((unsigned long long)w * E / G), (long long)(((unsigned long long)w + 1) * E / G)};
}

}  // namespace bank
}  // namespace mib
