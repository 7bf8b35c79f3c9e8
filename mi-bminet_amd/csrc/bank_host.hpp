// bank_host.hpp — the HIP-free part of a parameter bank (net_bank_create, include/mibminet.h): which
// sets may share a bank, the exact-division form every slice of a mixed bank takes, the images of
// a bank built from its blobs (bank::build: all of net_bank_create but the allocation), the image
// of a set that replaces one of a resident bank (bank::replace_set: all of net_bank_replace but the
// locking and the copy), the partition of an item list over the workgroups of bank::bank_loop (forward_bank.hpp), and the
// layout and lists of many recordings' windows (net_bank_windows_starts, net_bank_windows_lists).
// HIP-free like params_host.hpp, entry_host.hpp (whose windows_count the lists use) and images.hpp:
// included by mibminet.hip and the stand-alone host programs (tests/bank_host_main.cpp,
// tests/bank_replace_host_main.cpp, tests/windows_bank_host_main.cpp); forward_bank.hpp includes it
// for range_of alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "entry_host.hpp"
#include "image_layout.hpp"  // MIB_HD, gen::GenParams, bank::Scale
#include "images.hpp"
#include "params_host.hpp"

namespace mib {
namespace bank {

// The sets of a bank run one kernel instantiation on one LDS carve: C, T and N fix the carve,
// REORDER_BN and the clip the instantiation (F1 = F2 = 16 and D = 1 are the family's,
// gen_supported).  Exact division is not compared: a mixed bank takes the exact form (force_exact).
inline bool agree(const HostParams& a, const HostParams& b) {
  return a.d.C == b.d.C && a.d.T == b.d.T && a.d.N == b.d.N && a.d.F1 == b.d.F1 && a.d.F2 == b.d.F2 &&
         a.d.D == b.d.D && a.reorder_bn == b.reorder_bn && a.clip_balanced == b.clip_balanced;
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

// One set of a bank: the blob through the loader's own path (parse_blob, build_set), its window
// image kept.  hp comes back as build_set leaves it.
inline int bank_set(const void* blob, size_t len, bool force_general, HostParams& hp, gen::GenParams& gp) {
  if (const int rc = parse_blob(blob, len, hp)) return rc;
  Image img, win;
  if (const int rc = build_set(hp, force_general, &img, &win)) return rc;
  if (!win.data) return NET_ERR_UNSUPPORTED;
  gp = *(const gen::GenParams*)win.data.get();
  return NET_OK;
}

// The image of a float set in the exact-division form (force_exact), for a bank some other set of
// which needs exact division.
inline int bank_set_exact(const HostParams& hp, gen::GenParams& gp) {
  Ranges rg;
  if (const int rc = check_ranges(hp, rg)) return rc;
  Plan pl = make_plan(hp, rg);
  force_exact(hp, pl);
  return build_genparams(hp, pl, gp);
}

// What a bank was created with, kept for the sets that replace one of its own later
// (net_bank_replace): the geometry and build variant every set agreed on, the form its kernels run
// (exact division iff some set needed it at creation), how its images were built and whether it has
// scales.  It never changes: a set that replaces set 0 is held to it like any other.
struct Record {
  Dims d;
  bool reorder_bn = true, clip_balanced = false;
  bool xr = false;
  bool force_general = false;
  bool has_scales = false;
};
inline bool agree(const Record& r, const HostParams& b) {
  HostParams a;
  a.d = r.d;
  a.reorder_bn = r.reorder_bn;
  a.clip_balanced = r.clip_balanced;
  return agree(a, b);
}

// The images of a bank of n_sets blobs (scales: one per set, or null), in order: each set parsed and
// built as bank_set does, held to set 0 (agree), its scale checked; then, where some sets need exact
// division and others do not, the others promoted (bank_set_exact).  Returns the first error, *failed
// (if non-null) the set it belongs to; sets and scales then hold nothing a caller may use.  *rec (if
// non-null) is the bank's creation record.
inline int build(const void* const* blobs, const size_t* sizes, const float* scales, size_t n_sets, bool force_general,
                 std::vector<gen::GenParams>& sets, std::vector<Scale>& out_scales, size_t* failed,
                 Record* rec = nullptr) {
  auto fail = [&](size_t i, int rc) {
    if (failed) *failed = i;
    return rc;
  };
  sets.clear();
  sets.resize(n_sets);
  out_scales.clear();
  std::vector<HostParams> hps(n_sets);
  bool any_xr = false, all_xr = true;
  for (size_t i = 0; i < n_sets; i++) {
    if (const int rc = bank_set(blobs[i], sizes[i], force_general, hps[i], sets[i])) return fail(i, rc);
    if (!agree(hps[0], hps[i])) return fail(i, NET_ERR_UNSUPPORTED);
    if (scales) {
      if (const int rc = check_scale(scales[i])) return fail(i, rc);
      out_scales.push_back(Scale{scales[i], recip_scale(scales[i])});
    }
    any_xr = any_xr || sets[i].xr;
    all_xr = all_xr && sets[i].xr;
  }
  if (any_xr && !all_xr)
    for (size_t i = 0; i < n_sets; i++)
      if (!sets[i].xr)
        if (const int rc = bank_set_exact(hps[i], sets[i])) return fail(i, rc);
  if (rec) *rec = Record{hps[0].d, hps[0].reorder_bn, hps[0].clip_balanced, any_xr, force_general, scales != nullptr};
  return NET_OK;
}

// The decision of net_bank_replace: the image (and, for a bank with scales, the scale entry) that
// `blob` with `scale` gets as a set of the bank created with `rec`, or why it cannot be one.  The blob
// goes through the loader's path as in bank_set and comes back with its own code if that refuses it;
// it must agree with the record (NET_ERR_UNSUPPORTED), not with whatever set 0 is now.  A bank that
// runs the exact-division form takes a float set in that form (bank_set_exact); a bank that runs the
// float form refuses a set that needs exact division (NET_ERR_UNSUPPORTED): promoting the resident
// sets would change the kernel instantiation under calls in flight.  The scale is checked and given
// its reciprocal iff the bank has scales, and ignored otherwise (sc then {0, 0}).  The result is what
// bank::build gives that slot in a bank created with the new list.  On an error gp and sc hold
// nothing a caller may use.
inline int replace_set(const Record& rec, const void* blob, size_t len, float scale, gen::GenParams& gp, Scale& sc) {
  HostParams hp;
  if (const int rc = bank_set(blob, len, rec.force_general, hp, gp)) return rc;
  if (!agree(rec, hp)) return NET_ERR_UNSUPPORTED;
  if (gp.xr && !rec.xr) return NET_ERR_UNSUPPORTED;
  if (!gp.xr && rec.xr)
    if (const int rc = bank_set_exact(hp, gp)) return rc;
  sc = Scale{0.0f, 0.0f};
  if (rec.has_scales) {
    if (const int rc = check_scale(scale)) return rc;
    sc = Scale{scale, recip_scale(scale)};
  }
  return NET_OK;
}

// Workgroup w of G takes the items [lo, hi) = [floor(w E / G), floor((w + 1) E / G)): contiguous, so
// that on a list grouped by set a workgroup changes sets at most once per set its range touches.
// The ranges of w = 0 .. G - 1 tile [0, E) in order; w E < 2^63 for every grid and every E the
// entries admit (64-bit product: w E passes 2^32 from E = 2^23 on at 512 workgroups).
struct Range64 {
  long long lo, hi;
};
MIB_HD inline Range64 range_of(unsigned w, unsigned G, unsigned long long E) {
  return Range64{(long long)((unsigned long long)w * E / G), (long long)(((unsigned long long)w + 1) * E / G)};
}

// ---- windows through a bank (net_model_compute_windows_bank): the layout of R recordings -----
// Recording r starts at starts[r], a multiple of 16 samples: starts[0] = 0, starts[r + 1] =
// starts[r] + lengths[r] rounded up to 16, and L = starts[R - 1] + lengths[R - 1] (no rounding after
// the last).  Fills starts[0 .. R - 1] if non-null and returns L; 0 (starts then unspecified) for
// R == 0, null lengths, or an L or a start past INT64_MAX (the onsets are int64).
inline size_t windows_starts(const size_t* lengths, size_t R, int64_t* starts) {
  if (R == 0 || !lengths) return 0;
  constexpr size_t LIM = (size_t)INT64_MAX;
  size_t at = 0;  // <= LIM, a multiple of 16
  for (size_t r = 0; r < R; r++) {
    if (starts) starts[r] = (int64_t)at;
    if (lengths[r] > LIM - at) return 0;
    const size_t e = at + lengths[r];  // <= LIM
    if (r + 1 == R) return e;
    if (e > LIM - 15) return 0;
    at = (e + 15) / 16 * 16;
  }
  return 0;
}

// The lists of the sliding windows (hop) of those recordings for a bank of n_sets sets of T samples:
// blk_set (every block from starts[r] / 16 up to the block before starts[r + 1] / 16, for the last
// recording up to ceil(L / 16), gets sets[r]; filled if non-null and n_blk >= ceil(L / 16)), onsets
// (starts[r] + k hop, k < the windows of lengths[r]; filled if non-null and cap >= W) and
// first[0 .. R] (if non-null).  Returns W; 0 and nothing written for hop == 0, null lengths or sets,
// R == 0, overflow, or a set outside the bank.
inline size_t windows_lists(size_t T, size_t n_sets, const size_t* lengths, const int32_t* sets, size_t R,
                            size_t hop, int32_t* blk_set, size_t n_blk, int64_t* onsets, size_t cap, size_t* first) {
  if (hop == 0 || !sets || T == 0) return 0;
  const size_t L = windows_starts(lengths, R, nullptr);
  if (L == 0) {
    // L == 0 is also R recordings of no samples: then there is nothing to fill but first
    bool empty = R > 0 && lengths;
    for (size_t r = 0; empty && r < R; r++) empty = lengths[r] == 0;
    if (!empty) return 0;
  }
  for (size_t r = 0; r < R; r++)
    if (sets[r] < 0 || (size_t)sets[r] >= n_sets) return 0;
  size_t W = 0;  // <= L
  for (size_t r = 0; r < R; r++) W += windows_count(T, lengths[r], hop);
  const size_t nb = L / 16 + (L % 16 != 0);
  const bool fill_b = blk_set && n_blk >= nb, fill_o = onsets && cap >= W;
  size_t at = 0, i = 0;
  for (size_t r = 0; r < R; r++) {
    const size_t e = at + lengths[r], next = r + 1 == R ? nb * 16 : (e + 15) / 16 * 16;
    if (fill_b)
      for (size_t b = at / 16; b < next / 16; b++) blk_set[b] = sets[r];
    if (first) first[r] = i;
    const size_t n = windows_count(T, lengths[r], hop);
    if (fill_o)
      for (size_t k = 0; k < n; k++) onsets[i + k] = (int64_t)(at + k * hop);
    i += n;
    at = next;
  }
  if (first) first[R] = W;
  return W;
}

}  // namespace bank
}  // namespace mib
