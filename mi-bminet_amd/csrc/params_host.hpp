// params_host.hpp — a parameter set on the host: the blob parser, the checks of the reference's
// own int32 arithmetic, constant-filter folding and the requant plan that both parameter images
// (images.hpp) lay out.  HIP-free like requant_host.hpp.
#pragma once
#include <vector>

#include "../../include/mibminet.h"
#include "net_consts.hpp"
#include "requant_host.hpp"

namespace mib {

constexpr int HEADER_SIZE = 64;
constexpr uint32_t FLAG_REORDER_BN = 1;
constexpr uint32_t FLAG_CLIP_BALANCED = 2;  // golden-model clip_balanced=True (functional.py:89-91)

struct Dims {
  int C = 0, T = 0, F1 = 0, F2 = 0, D = 0, N = 0, wbits = 8;
  // (unsigned: a header may carry INT_MAX, and the parser asks before it has sized anything)
  int C_ALIGN() const { return (int)(((unsigned)C + 3u) & ~3u); }
  int T_ALIGN() const { return (int)(((unsigned)T + 3u) & ~3u); }
  int T8() const { return T / 8; }
  int T8_ALIGN() const { return (T8() + 3) & ~3; }
  int T64() const { return T8() / 8; }
  int T64_ALIGN() const { return (T64() + 3) & ~3; }
};

// Host copy of the net.h arrays (weights unpacked to int8).
struct HostParams {
  Dims d;
  std::vector<int32_t> l1_factor, l1_offset, l2_factor, l2_offset, l4_factor, l4_offset;
  std::vector<int8_t> l1_weight_align, l2_weight_reverse, l3_weight, l4_weight, l5_bias, l5_weight;
  int32_t l3_factor = 0, l5_factor = 0;
  bool reorder_bn = true;  // blob flag: -DREORDER_BN variant (canonical) or the plain BN branches
  bool clip_balanced = false;  // blob flag: clip to [-127, 127] (golden model's default; the C clips to -128)
  bool xr = false;             // set at load: exact integer division at layers 1, 2, 4 (Cfg::XR)
  int xr_layer = 0, xr_filter = -1;  // the first requant without a proven float form (xr = true)
  bool general = false;        // set at load: the run-time-dimension kernels (forward_gen.hpp)
  int folded = 0;              // set at load: constant filters folded (fold_constant_filters)
};

// The dimensions of a header, a blob's and a net_arrays_t's alike: positive, T of at least one
// layer-5 sample, and F2 = F1 D without trusting int to hold the product.  What the kernels support
// of them is build_set's business (images.hpp).
inline int check_dims(const Dims& d) {
  if (d.C <= 0 || d.T < 64 || d.F1 <= 0 || d.D < 1 || d.F2 < 1 || d.N <= 0) return NET_ERR_BLOB;
  return (int64_t)d.F2 == (int64_t)d.F1 * d.D ? NET_OK : NET_ERR_BLOB;
}

// ---- blob parsing ------------------------------------------------------------------------
// Every array is sized from the header, so each read first tests that the bytes left cover it: a
// header cannot make the reader allocate more than the blob holds.  pos <= n while ok.
struct Reader {
  const uint8_t* p;
  size_t n, pos;
  bool ok = true;
  const uint8_t* take(size_t bytes) {
    if (!ok || bytes > n - pos) { ok = false; return nullptr; }
    const uint8_t* r = p + pos;
    pos += bytes;
    const size_t pad = (4 - bytes % 4) % 4;
    if (pad > n - pos) { ok = false; return nullptr; }
    pos += pad;
    return r;
  }
  int32_t one() {
    int32_t v = 0;
    if (const uint8_t* s = take(4)) std::memcpy(&v, s, 4);
    return v;
  }
  std::vector<int32_t> i32(size_t count) {
    if (count > (n - pos) / 4) ok = false;
    const uint8_t* s = take(4 * count);
    std::vector<int32_t> v(s ? count : 0);
    if (s) std::memcpy(v.data(), s, 4 * count);
    return v;
  }
  // count = a b weights of wbits bits (a product past size_t covers nothing)
  std::vector<int8_t> w(size_t a, size_t b, int wbits) {
    const size_t count = b && a > SIZE_MAX / b ? SIZE_MAX : a * b;
    const uint8_t* s = take(wbits == 8 ? count : count / 2 + count % 2);
    std::vector<int8_t> v(s ? count : 0);
    if (!s) return v;
    if (wbits == 8) {
      std::memcpy(v.data(), s, count);
    } else {
      for (size_t i = 0; i < count; i++) {
        int nib = (s[i / 2] >> (4 * (i & 1))) & 0xF;
        v[i] = (int8_t)(nib >= 8 ? nib - 16 : nib);
      }
    }
    return v;
  }
};

// The reference multiplies the weight pads too (func_dotp over all C_ALIGN / F2 * T64_ALIGN bytes,
// layer1.c:90, layer5.c:81) and gen_net_header.py writes them as zeros; the GPU skips them, so a
// set with non-zero pads is rejected (NET_ERR_BLOB), as ParamSet.validate does.
inline int check_pads(const HostParams& hp) {
  const Dims& d = hp.d;
  const int F2 = d.F2;
  for (int f = 0; f < F2; f++)
    for (int c = d.C; c < d.C_ALIGN(); c++)
      if (hp.l1_weight_align[(size_t)f * d.C_ALIGN() + c] != 0) return NET_ERR_BLOB;
  for (int n = 0; n < d.N; n++)
    for (int k = 0; k < F2; k++)
      for (int v = d.T64(); v < d.T64_ALIGN(); v++)
        if (hp.l5_weight[((size_t)n * F2 + k) * d.T64_ALIGN() + v] != 0) return NET_ERR_BLOB;
  return NET_OK;
}

inline int parse_blob(const void* blob, size_t len, HostParams& hp) {
  if (!blob || len < (size_t)HEADER_SIZE) return NET_ERR_BLOB;
  const uint8_t* b = (const uint8_t*)blob;
  if (std::memcmp(b, "MIBMINET", 8) != 0) return NET_ERR_BLOB;
  uint32_t h[11];
  std::memcpy(h, b + 8, sizeof(h));
  const uint32_t version = h[0];
  Dims d;
  d.C = (int)h[1]; d.T = (int)h[2]; d.F1 = (int)h[3]; d.F2 = (int)h[4]; d.D = (int)h[5];
  d.N = (int)h[6]; d.wbits = (int)h[7];
  const uint32_t l2t = h[8], l3t = h[9], flags = h[10];
  if (version != 1 || l2t != 64 || l3t != 16) return NET_ERR_BLOB;
  if (flags & ~(FLAG_REORDER_BN | FLAG_CLIP_BALANCED)) return NET_ERR_BLOB;
  hp.reorder_bn = (flags & FLAG_REORDER_BN) != 0;
  hp.clip_balanced = (flags & FLAG_CLIP_BALANCED) != 0;
  if (d.wbits != 8 && d.wbits != 4) return NET_ERR_BLOB;
  if (const int rc = check_dims(d)) return rc;
  Reader r{b, len, (size_t)HEADER_SIZE};
  const size_t F2 = (size_t)d.F2;
  hp.d = d;
  hp.l1_factor = r.i32(F2); hp.l1_offset = r.i32(F2);
  hp.l1_weight_align = r.w(F2, (size_t)d.C_ALIGN(), d.wbits);
  hp.l2_factor = r.i32(F2); hp.l2_offset = r.i32(F2);
  hp.l2_weight_reverse = r.w(F2, 64, d.wbits);
  hp.l3_factor = r.one();
  hp.l3_weight = r.w(F2, 16, d.wbits);
  hp.l4_factor = r.i32(F2); hp.l4_offset = r.i32(F2);
  hp.l4_weight = r.w(F2, F2, d.wbits);
  hp.l5_factor = r.one();
  hp.l5_bias = r.w((size_t)d.N, 1, 8);
  hp.l5_weight = r.w((size_t)d.N, F2 * (size_t)d.T64_ALIGN(), d.wbits);  // F2 T64_ALIGN < 2^56
  if (!r.ok || r.pos != len) return NET_ERR_BLOB;
  return check_pads(hp);
}

// net_blob_widen: the blob over R source rows.  Layer 1 is a dense contraction over its K-slots
// whatever C is, so the set whose layer-1 weight column channels[c] is the blob's column c, every
// other column zero, computes on u[R][T] what the blob computes on u[channels]: the same int32
// accumulators (zeros add nothing), hence the same reachable ranges, requant path and range
// verdict.  The output is the input with C := R and l1_weight_align as [F2][R_ALIGN]; every other
// byte is copied.  The parser's verdict comes first; then R in 1 .. 64 and channels, C distinct
// entries in 0 .. R - 1 (two equal entries would add two columns, and the sum may leave int8); then
// the size: *out_len (if non-null) is set whenever the arguments pass, out == NULL asks for it only.
inline int widen_blob(const void* blob, size_t len, int R, const int32_t* channels, void* out, size_t cap,
                      size_t* out_len) {
  HostParams hp;
  if (const int rc = parse_blob(blob, len, hp)) return rc;
  const Dims& d = hp.d;
  if (R < 1 || R > 64 || !channels || d.C > R) return NET_ERR_INVALID;  // C > R: no C distinct entries
  bool seen[64] = {};
  for (int c = 0; c < d.C; c++) {
    if (channels[c] < 0 || channels[c] >= R || seen[channels[c]]) return NET_ERR_INVALID;
    seen[channels[c]] = true;
  }
  // the layer-1 weights follow the header and the two int32[F2] arrays; F2 C_ALIGN is a multiple of
  // 4, so int4 rows pack to whole bytes (Reader::w)
  const size_t F2n = (size_t)d.F2, CA = (size_t)d.C_ALIGN(), RA = ((size_t)R + 3) & ~(size_t)3;
  auto packed = [&](size_t count) { return ((d.wbits == 8 ? count : count / 2) + 3) & ~(size_t)3; };
  const size_t at = (size_t)HEADER_SIZE + 8 * F2n, old_bytes = packed(F2n * CA), new_bytes = packed(F2n * RA);
  const size_t need = len - old_bytes + new_bytes;  // parse_blob read old_bytes from at: len >= at + old_bytes
  if (out_len) *out_len = need;
  if (!out) return NET_OK;
  if (cap < need) return NET_ERR_INVALID;
  std::vector<int8_t> w(F2n * RA, 0);
  for (size_t f = 0; f < F2n; f++)
    for (int c = 0; c < d.C; c++) w[f * RA + (size_t)channels[c]] = hp.l1_weight_align[f * CA + (size_t)c];
  uint8_t* o = (uint8_t*)out;
  const uint8_t* b = (const uint8_t*)blob;
  std::memcpy(o, b, at);
  const uint32_t r32 = (uint32_t)R;
  std::memcpy(o + 12, &r32, 4);  // the header's C (parse_blob: h[1])
  std::memset(o + at, 0, new_bytes);
  if (d.wbits == 8) {
    std::memcpy(o + at, w.data(), w.size());
  } else {
    for (size_t i = 0; i < w.size(); i++) o[at + i / 2] |= (uint8_t)((w[i] & 0xF) << (4 * (i & 1)));
  }
  std::memcpy(o + at + new_bytes, b + at + old_bytes, len - at - old_bytes);
  return NET_OK;
}

// net_params_load_arrays: the blob header's checks (parse_blob, check_dims), then the arrays it would carry
inline int parse_arrays(const net_arrays_t* a, HostParams& hp) {
  if (!a) return NET_ERR_INVALID;
  if (a->flags & ~(FLAG_REORDER_BN | FLAG_CLIP_BALANCED)) return NET_ERR_BLOB;
  Dims d;
  d.C = a->C; d.T = a->T; d.F1 = a->F1; d.F2 = a->F2; d.D = a->D; d.N = a->N; d.wbits = 8;
  if (const int rc = check_dims(d)) return rc;
  if ((size_t)d.C * d.T > ((size_t)1 << 30) || d.N > 4096 || d.F2 > 4096) return NET_ERR_UNSUPPORTED;
  if (!a->l1_factor || !a->l1_offset || !a->l1_weight_align || !a->l2_factor || !a->l2_offset ||
      !a->l2_weight_reverse || !a->l3_weight || !a->l4_factor || !a->l4_offset || !a->l4_weight || !a->l5_bias ||
      !a->l5_weight)
    return NET_ERR_INVALID;
  hp.d = d;
  hp.reorder_bn = (a->flags & FLAG_REORDER_BN) != 0;
  hp.clip_balanced = (a->flags & FLAG_CLIP_BALANCED) != 0;
  const size_t F2 = (size_t)d.F2;
  auto i32 = [](const int32_t* p, size_t n) { return std::vector<int32_t>(p, p + n); };
  auto i8 = [](const int8_t* p, size_t n) { return std::vector<int8_t>(p, p + n); };
  hp.l1_factor = i32(a->l1_factor, F2);
  hp.l1_offset = i32(a->l1_offset, F2);
  hp.l1_weight_align = i8(a->l1_weight_align, F2 * d.C_ALIGN());
  hp.l2_factor = i32(a->l2_factor, F2);
  hp.l2_offset = i32(a->l2_offset, F2);
  hp.l2_weight_reverse = i8(a->l2_weight_reverse, F2 * 64);
  hp.l3_factor = a->l3_factor;
  hp.l3_weight = i8(a->l3_weight, F2 * 16);
  hp.l4_factor = i32(a->l4_factor, F2);
  hp.l4_offset = i32(a->l4_offset, F2);
  hp.l4_weight = i8(a->l4_weight, F2 * F2);
  hp.l5_factor = a->l5_factor;
  hp.l5_bias = i8(a->l5_bias, (size_t)d.N);
  hp.l5_weight = i8(a->l5_weight, (size_t)d.N * F2 * d.T64_ALIGN());
  return check_pads(hp);
}

// ---- range checks ---------------------------------------------------------------------------
// Three outcomes per parameter set:
//  * NET_ERR_RANGE where the reference's own int32 arithmetic is undefined for some input: a zero
//    divisor (factor, or factor >> 3 in the plain branches), INT_MIN / -1, or an overflowing sum
//    (acc + off of layer1.c:90-91, the pooled partial sums and sum + off of layer2.c:97-111 /
//    layer4.c:99-130, the plain layer 4's sum of eight unclipped elements, layer4.c:113-130);
//  * the float requant kernels (xr = false) when every layer-1, -2 and -4 requant has a proven
//    float form (make_plan below);
//  * otherwise the exact-division kernels (xr = true, Cfg::XR: xdiv at layers 1, 2 and 4).
// Reachable ranges of the layer-1, -2 and -4 requant numerators (both kernel families): e1 = dot +
// off1 (layer 1); REORDER_BN: the pooled sums + offset of layers 2 and 4; plain: the per-element
// numerators conv + (off >> 3).  All sixteen filters (F1 = F2 = 16, what both families take).
struct Ranges {
  Range e1[F2], s2[F2], s4[F2];
};
inline int check_ranges(const HostParams& hp, Ranges& rg) {
  const Dims& d = hp.d;
  if (d.F1 != F2 || d.F2 != F2) return NET_ERR_UNSUPPORTED;
  const int C = d.C, CA = d.C_ALIGN();
  Range* e1 = rg.e1;
  Range* s2 = rg.s2;
  Range* s4 = rg.s4;
  for (int f = 0; f < F2; f++) {
    const Range r1 = dot_range(&hp.l1_weight_align[(size_t)f * CA], C);
    const Range r2 = dot_range(&hp.l2_weight_reverse[(size_t)f * 64], 64);
    const Range r4 = dot_range(&hp.l4_weight[(size_t)f * F2], F2);
    e1[f].lo = r1.lo + hp.l1_offset[f];
    e1[f].hi = r1.hi + hp.l1_offset[f];
    if (!div_ok(e1[f], hp.l1_factor[f])) return NET_ERR_RANGE;
    if (hp.reorder_bn) {
      if (!pooled_range(r2, hp.l2_offset[f], &s2[f]) || !div_ok(s2[f], hp.l2_factor[f])) return NET_ERR_RANGE;
      if (!pooled_range(r4, hp.l4_offset[f], &s4[f]) || !div_ok(s4[f], hp.l4_factor[f])) return NET_ERR_RANGE;
    } else {
      const int32_t f2 = hp.l2_factor[f] >> 3, o2 = hp.l2_offset[f] >> 3;
      const int32_t f4 = hp.l4_factor[f] >> 3, o4 = hp.l4_offset[f] >> 3;
      s2[f].lo = r2.lo + o2; s2[f].hi = r2.hi + o2;
      s4[f].lo = r4.lo + o4; s4[f].hi = r4.hi + o4;
      if (!div_ok(s2[f], f2) || !div_ok(s4[f], f4)) return NET_ERR_RANGE;
      // the eight elements max((v + off) / fac, 0) are summed unclipped: trunc is monotone in v
      const int64_t q4 = std::max({(int64_t)0, s4[f].lo / f4, s4[f].hi / f4});
      if (!fits_i32(8 * q4)) return NET_ERR_RANGE;
    }
  }
  if (hp.l3_factor == 0 || hp.l5_factor == 0) return NET_ERR_RANGE;
  return NET_OK;
}

// Per-filter classification ahead of the float / exact choice.  A layer-1, -2 or -4 filter whose
// output is one value y over its whole reachable numerator range
// (a rail: an offset far past anything the weights reach, a factor that sends every sum to zero, a
// REORDER_BN threshold above every conv value) is folded into zero weights with offset y and
// factor 1, or offset -y and factor -1 when y < 0 (a pooled sum of zeros with offset |y| and
// threshold -(|y| >> 3) <= 0 is |y|).  The kernels then produce the same y for every input with
// either requant form, and the filter no longer takes the set off the float kernels.  trunc(v /
// fac) and the clip are monotone in v, so the output is constant iff it is equal at both ends of
// the range.  Returns the count.
inline int fold_constant_filters(HostParams& h, const Ranges& rg) {
  const Dims& d = h.d;
  const int64_t lo = h.clip_balanced ? -127 : -128;
  auto q = [&](int64_t v, int64_t fac) { return std::min<int64_t>(127, std::max<int64_t>(lo, v / fac)); };
  auto constant = [&](const Range& r, int32_t fac, int32_t* y) {
    const int64_t a = q(r.lo, fac), b = q(r.hi, fac);
    *y = (int32_t)a;
    return a == b;
  };
  int n = 0;
  // filter f of a layer (len weights each) becomes zero weights with offset o and factor fc
  auto fold = [&](std::vector<int8_t>& w, int len, int f, int32_t& off, int32_t& fac, int32_t o, int32_t fc) {
    std::fill_n(&w[(size_t)f * len], len, (int8_t)0);
    off = o;
    fac = fc;
    n++;
  };
  for (int f = 0; f < d.F2; f++) {
    int32_t y;
    if (constant(rg.e1[f], h.l1_factor[f], &y))
      fold(h.l1_weight_align, d.C_ALIGN(), f, h.l1_offset[f], h.l1_factor[f], y, 1);
    if (!h.reorder_bn) {
      // plain branches: the elements e = trunc((conv + (off >> 3)) / (fac >> 3)) (clipped in layer
      // 2, not in the C's layer 4) go through max(e, 0), a sum of 8 and // 8 (and the final clip in
      // layer 4): the output is 0 when every e <= 0, 127 when every e >= 127, e when e is
      // constant.  Folded: factor 8 and offset 8 y, so every element is y (in [0, 127]).
      auto plain = [&](const Range& r, int32_t fac, int32_t* yp) {
        const int64_t a = r.lo / (int64_t)(fac >> 3), b = r.hi / (int64_t)(fac >> 3);
        const int64_t emin = std::min(a, b), emax = std::max(a, b);
        if (emax > 0 && emin < 127 && emin != emax) return false;
        *yp = (int32_t)std::min<int64_t>(127, std::max<int64_t>(0, emin));
        return true;
      };
      if (plain(rg.s2[f], h.l2_factor[f], &y))
        fold(h.l2_weight_reverse, 64, f, h.l2_offset[f], h.l2_factor[f], 8 * y, 8);
      if (plain(rg.s4[f], h.l4_factor[f], &y)) fold(h.l4_weight, d.F2, f, h.l4_offset[f], h.l4_factor[f], 8 * y, 8);
      continue;
    }
    if (constant(rg.s2[f], h.l2_factor[f], &y))
      fold(h.l2_weight_reverse, 64, f, h.l2_offset[f], h.l2_factor[f], y < 0 ? -y : y, y < 0 ? -1 : 1);
    if (constant(rg.s4[f], h.l4_factor[f], &y))
      fold(h.l4_weight, d.F2, f, h.l4_offset[f], h.l4_factor[f], y < 0 ? -y : y, y < 0 ? -1 : 1);
  }
  return n;
}

// ---- the requant plan -----------------------------------------------------------------------
// Every requantisation constant of a set, searched once; the two image builders (images.hpp) only
// lay it out.  Layers 1, 2 and 4 take a float form per filter: REORDER_BN layers 2 and 4 a
// reciprocal of the factor over the pooled sum (|v| < 2^24, converted); layer 1 the magic-offset
// form (C-init offset + FMAGIC_I, |v| < 2^22); the plain branches the floor form of factor >> 3
// (C-init mbits + (offset >> 3), |x| < 2^22; layer 2's elements clamp to [0, 127], layer 4's to
// [0, 1024]: anything above saturates the result).  A range outside the window or an unproven form
// makes the set exact (xr): the search stops there, (xr_layer, xr_filter) name that requant (every
// layer-1 filter first, then layers 2 and 4 filter by filter) and the float forms are all zero.
// The exact-division constants x1, x2, x4 (divisor: the factor, factor >> 3 in the plain branches),
// x3 and x5 are always there.  Layer 3 (|acc| <= 16 * 128^2 < 2^22, magic form) and layer 5 (|acc|
// <= F2 T64 128^2 + 128) have a float form for every int32 factor within 2^24
// (tests/test_requant_exact.py); what an unproven one means is the image's business.
struct FloatForm {
  float r = 0.0f, c = 0.0f;
  int32_t mbits = 0;  // floor form: the magic bits
};
struct Plan {
  bool xr = false;
  int xr_layer = 0, xr_filter = -1;
  FloatForm f1[F2], f2[F2], f4[F2];
  // the MFMA C-inits that carry a float form's magic: layer 1 offset + FMAGIC_I, the plain
  // branches' mbits + (offset >> 3); exact: the offset, offset >> 3.  (REORDER_BN: ci2, ci4 unused.)
  int32_t ci1[F2] = {}, ci2[F2] = {}, ci4[F2] = {};
  XDiv x1[F2], x2[F2], x4[F2], x3, x5;
  bool l3_ok = false, l5_ok = false;
  float l3_r = 0.0f, l3_c = 0.0f, l5_r = 0.0f;
};

inline Plan make_plan(const HostParams& hp, const Ranges& rg) {
  Plan pl;
  const bool rb = hp.reorder_bn;
  const int64_t A = 128 * 128;
  auto div2 = [&](int f) { return rb ? hp.l2_factor[f] : hp.l2_factor[f] >> 3; };
  auto div4 = [&](int f) { return rb ? hp.l4_factor[f] : hp.l4_factor[f] >> 3; };
  for (int f = 0; f < F2; f++) {
    pl.x1[f] = xdiv_consts(hp.l1_factor[f]);
    pl.x2[f] = xdiv_consts(div2(f));
    pl.x4[f] = xdiv_consts(div4(f));
  }
  pl.x3 = xdiv_consts(hp.l3_factor);
  pl.x5 = xdiv_consts(hp.l5_factor);
  pl.l3_ok = choose_reciprocal(hp.l3_factor, &pl.l3_r, &pl.l3_c, 128, 16 * A);
  pl.l5_ok = choose_reciprocal(hp.l5_factor, &pl.l5_r, nullptr, 128, (int64_t)F2 * hp.d.T64() * A + 128);
  // one requant: the range check, then the search
  auto form = [&](int layer, int f) -> bool {
    const Range& v = layer == 1 ? rg.e1[f] : layer == 2 ? rg.s2[f] : rg.s4[f];
    FloatForm& ff = layer == 1 ? pl.f1[f] : layer == 2 ? pl.f2[f] : pl.f4[f];
    if (v.amax() >= (layer == 1 || !rb ? 1 << 22 : 1 << 24)) return false;
    if (layer == 1) return choose_reciprocal(hp.l1_factor[f], &ff.r, &ff.c, 128, v.amax());
    if (rb) return choose_reciprocal(layer == 2 ? div2(f) : div4(f), &ff.r, nullptr, 128, v.amax());
    return choose_floor_form(layer == 2 ? div2(f) : div4(f), layer == 2 ? 127 : 1024, v.amax(), &ff.mbits, &ff.r, &ff.c);
  };
  auto floats = [&]() -> bool {
    for (int f = 0; f < F2; f++)
      if (!form(1, f)) { pl.xr_layer = 1; pl.xr_filter = f; return false; }
    for (int f = 0; f < F2; f++)
      for (int layer = 2; layer <= 4; layer += 2)
        if (!form(layer, f)) { pl.xr_layer = layer; pl.xr_filter = f; return false; }
    return true;
  };
  pl.xr = !floats();
  for (int f = 0; f < F2; f++) {
    if (pl.xr) pl.f1[f] = pl.f2[f] = pl.f4[f] = FloatForm();
    // float: every numerator range is within 2^22 and holds the offset itself, so no sum wraps
    pl.ci1[f] = hp.l1_offset[f] + (pl.xr ? 0 : FMAGIC_I);
    pl.ci2[f] = (hp.l2_offset[f] >> 3) + pl.f2[f].mbits;
    pl.ci4[f] = (hp.l4_offset[f] >> 3) + pl.f4[f].mbits;
  }
  return pl;
}

}  // namespace mib
