// requant_host.hpp — the host's requantisation proofs: float reciprocals, floor forms, the exact
// division constants and the reachable-range arithmetic they rest on.  Pure C++17 (no HIP, no vector
// types), so it also builds into a stand-alone host program (tests/host_arith_main.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace mib {

// ---- exact requantisation ------------------------------------------------------------------
// y = clip(trunc(v / fac), -128, 127) is computed on the GPU as clip((int)((float)v * r)).
// (float)v is exact for |v| < 2^24 and (int) truncates toward zero.  q(v) = (int)RN(v * r) is
// monotone in v, so it equals trunc(v / fac) on a whole constant interval of trunc(v / fac) iff it
// does at both ends.  verify() checks both ends of the intervals for k = -129 .. 128 that hold a
// reachable v (|v| <= vmax, the layer's accumulator bound), which pins the clipped result for
// every reachable v.  choose_reciprocal() starts two floats below RN(1/|fac|) and nudges upward
// until verify() passes: for large factors the admissible window is only a few floats wide
// (about 1 / (|fac| * 129) relative), so it must not be stepped over.

inline int64_t trunc_div(int64_t a, int64_t b) { return a / b; }  // C semantics

inline int64_t qf(int64_t v, float r) { return (int64_t)(int32_t)((float)v * r); }

// kmax: largest output step that must be exact (128 for int8 clipping; the non-REORDER_BN
// layer 4 clamps its unclipped elements at 1024 instead).  vmax: largest reachable |v|;
// intervals beyond it are not checked.
inline bool verify_reciprocal(int32_t fac, float r, int64_t kmax = 128, int64_t vmax = (1 << 24) - 1) {
  const int64_t F = fac < 0 ? -(int64_t)fac : (int64_t)fac;
  for (int64_t k = -129; k <= kmax; k++) {
    // interval of v (for |fac|) with trunc(v / F) == k
    int64_t lo, hi;
    if (k > 0) { lo = k * F; hi = k * F + F - 1; }
    else if (k == 0) { lo = -(F - 1); hi = F - 1; }
    else { lo = k * F - (F - 1); hi = k * F; }
    if (fac < 0) {  // trunc(v / fac) = trunc(-v / F): result k on the mirrored interval -[lo, hi]
      const int64_t a = -hi, b = -lo;
      lo = a; hi = b;
    }
    const int64_t want = k;
    if (lo > vmax || hi < -vmax) continue;  // unreachable
    lo = std::max(lo, -vmax);
    hi = std::min(hi, vmax);
    if (std::llabs(lo) >= (1 << 24) || std::llabs(hi) >= (1 << 24)) return false;
    if (qf(lo, r) != want || qf(hi, r) != want) return false;
    if (trunc_div(lo, fac) != want || trunc_div(hi, fac) != want) return false;  // self-check
  }
  return true;
}

inline bool choose_reciprocal(int32_t fac, float* out, float* magic_c = nullptr, int64_t kmax = 128,
                              int64_t vmax = (1 << 24) - 1) {
  // magic_c != nullptr: additionally require c = -(1.5 * 2^23) * r to be exact in f32, so that
  // fma(bits_as_float(v + 0x4B400000), r, c) == RN(v * r) (layer 1's one-instruction requant).
  if (fac == 0) return false;
  const double F = std::fabs((double)fac);
  float r = std::nextafterf(std::nextafterf((float)(1.0 / F), 0.0f), 0.0f);
  for (int tries = 0; tries < 4096; tries++) {
    const float rs = fac < 0 ? -r : r;
    bool ok = true;
    if (magic_c) {
      const double cd = -12582912.0 * (double)rs;
      const float cf = (float)cd;
      ok = ((double)cf == cd);
      if (ok) *magic_c = cf;
    }
    if (ok && verify_reciprocal(fac, rs, kmax, vmax)) { *out = rs; return true; }
    r = std::nextafterf(r, INFINITY);
  }
  return false;
}

// ---- floor-form element requant (plain-BN branches) ----------------------------------------
// The plain branches requantise every conv element and apply the ReLU right after:
// e = max(clip(trunc(x / fac)), 0) (layer2.c:139-210, layer4.c:113-130).  Behind the ReLU, trunc and
// floor agree (they differ only for negative quotients, which both clamp to 0), so
// e = clamp(floor(x / fac), 0, emax).  The GPU computes it without a float->int convert:
//   g(x) = fma(bits_as_float(Mbits + x), r, c)        (one rounding, round-to-nearest-even)
//   e    = bits(fmed3(g, K, K + emax)) - bits(K),       K = 1.5 * 2^23 (FMAGIC)
// The MFMA C-init carries Mbits + offset, so the accumulator's bits are exactly float(M + x).  The
// exact value of the fma is K + delta + x r with delta = M r + c - K; c is an integer-valued float
// that f32 holds exactly, so delta = M r - n for the integer n = K - c, and M is searched so that delta
// sits just below -1/2: then RN(K + delta + x r) = K + floor(x / fac) at every step boundary.  g is
// monotone in x, so checking both ends of every step interval k = -1 .. emax of the reachable range
// |x| <= vmax (with std::fmaf, the same correctly rounded fma) proves it for every reachable x.
inline float floor_form(int32_t mbits, int64_t x, float r, float c) {
  float m;
  const int32_t b = mbits + (int32_t)x;
  std::memcpy(&m, &b, 4);
  return std::fmaf(m, r, c);
}

inline bool verify_floor_form(int32_t fac, int32_t mbits, float r, float c, int64_t emax, int64_t vmax) {
  const int64_t F = fac < 0 ? -(int64_t)fac : (int64_t)fac;
  const float K = 12582912.0f;
  for (int64_t k = -1; k <= emax; k++) {
    // x with floor(x / fac) == k: fac > 0: [k F, k F + F - 1]; fac < 0: [-(k + 1) F + 1, -k F]
    int64_t lo = fac > 0 ? k * F : -(k + 1) * F + 1;
    int64_t hi = fac > 0 ? k * F + F - 1 : -k * F;
    if (lo > vmax || hi < -vmax) continue;
    lo = std::max(lo, -vmax);
    hi = std::min(hi, vmax);
    const int64_t want = std::min(std::max(k, (int64_t)0), emax);
    for (const int64_t x : {lo, hi}) {
      const float g = floor_form(mbits, x, r, c);
      const double e = std::min(std::max((double)g, (double)K), (double)K + (double)emax) - (double)K;
      if (e != (double)want) return false;
    }
  }
  return true;
}

inline bool choose_floor_form(int32_t fac, int64_t emax, int64_t vmax, int32_t* mbits, float* r_out, float* c_out) {
  if (fac == 0 || vmax >= (1 << 22) || emax > 1024) return false;
  const double F = std::fabs((double)fac);
  const double K = 12582912.0;
  const int64_t mlo = (1 << 23) + vmax, mhi = (1 << 24) - 1 - vmax;  // M + x stays in [2^23, 2^24)
  // target delta: -1/2 + 1/(2F), the middle of the window that maps each step to its floor
  const double target = -0.5 + 0.5 / F;
  float r = std::nextafterf(std::nextafterf((float)(1.0 / F), 0.0f), 0.0f);
  for (int tries = 0; tries < 16; tries++, r = std::nextafterf(r, INFINITY)) {
    const double rs = fac < 0 ? -(double)r : (double)r;
    // for each integer n, M = round((n + target) / rs) puts delta = M rs - n within rs / 2 of the
    // target; successive n give different residues, and the check below decides
    const double t0 = std::min((double)mlo * rs, (double)mhi * rs);
    const int64_t n0 = (int64_t)std::ceil(t0 - target) + 1;
    for (int64_t i = 0; i < 512 + 128; i++) {
      int64_t n, M;
      if (i < 512) {
        n = n0 + i;
        M = std::llround(((double)n + target) / rs);
      } else {
        // |fac| so large that M r moves by less than 1 over the whole magic range (every reachable
        // output is 0 or 1): the first magics with n on either side of M r
        M = mlo + (i - 512) / 2;
        n = (int64_t)((i & 1) ? std::ceil((double)M * rs) : std::floor((double)M * rs));
      }
      if (M < mlo || M > mhi) continue;
      const double c = K - (double)n;  // integer-valued (exact in f32 below 2^24, and when even below 2^25)
      if ((double)(float)c != c) continue;
      const float Mf = (float)M;
      int32_t mb;
      std::memcpy(&mb, &Mf, 4);
      if (verify_floor_form(fac, mb, (float)rs, (float)c, emax, vmax)) {
        *mbits = mb;
        *r_out = (float)rs;
        *c_out = (float)c;
        return true;
      }
    }
  }
  return false;
}

// ---- exact integer division (XR builds) ------------------------------------------------------
// Parameter sets outside the float envelope above (large folded BN offsets, or factors whose
// reciprocal window the check cannot prove) run the Cfg::XR kernels, which divide exactly
// (forward_common.hpp, xdiv): trunc(e r) in IEEE double with r = sign(d) RU(1 / |d|) equals C's
// trunc(e / d) for every int32 e.  For e, d > 0 with e / d = q + f (f a multiple of 1 / d,
// f <= 1 - 1 / d): 0 <= e r - e / d <= e 2^-52 / d, so the exact product lies in
// [q + f, q + f + e 2^-52 / d]; rounding it cannot go below q (q is a double), and its distance
// from q + 1 is at least (1 - e 2^-52) / d, more than half an ulp of the product ((e / d) 2^-53)
// for every e <= 2^31.  Negative e or d mirror it (the product changes sign only).  Round 5's
// integer form (m = ceil(2^(31 + l) / |d|), a 32 x 32 -> 64 product and a shift) took about
// twice the issue cycles.
// Exact division constants (forward_common.hpp, xdiv): the double r = sign(d) RU(1 / |d|), split
// into its low word (m) and high word (xs).  RU: 1 / |d| rounded to nearest, then one ulp up when
// that fell below (the fma residual r |d| - 1 is exact in sign).  Powers of two are exact.
struct XDiv {
  uint32_t m;
  int32_t xs;
};

inline XDiv xdiv_consts(int32_t d) {
  const double D = std::fabs((double)d);
  double r = 1.0 / D;
  if (std::fma(r, D, -1.0) < 0.0) r = std::nextafter(r, INFINITY);
  if (d < 0) r = -r;
  uint64_t bits;
  std::memcpy(&bits, &r, 8);
  return XDiv{(uint32_t)bits, (int32_t)(uint32_t)(bits >> 32)};
}

// the device sequence of xdiv on the host (mibminet_test_xdiv_host): IEEE double product, truncation
inline int32_t xdiv_host(int32_t e, XDiv c) {
  const uint64_t bits = ((uint64_t)(uint32_t)c.xs << 32) | c.m;
  double r;
  std::memcpy(&r, &bits, 8);
  return (int32_t)((double)e * r);
}

// Reachable range of an int8 dot product sum_i w[i] x[i] over inputs x in [-128, 127] (every
// layer entry point takes arbitrary int8 input, and the zero pads lie inside the range).
struct Range {
  int64_t lo = 0, hi = 0;
  int64_t amax() const { return std::max(std::llabs(lo), std::llabs(hi)); }
};
inline Range dot_range(const int8_t* w, int n) {
  Range r;
  for (int i = 0; i < n; i++) {
    r.lo += std::min(-128 * (int64_t)w[i], 127 * (int64_t)w[i]);
    r.hi += std::max(-128 * (int64_t)w[i], 127 * (int64_t)w[i]);
  }
  return r;
}
inline bool fits_i32(int64_t v) { return v >= INT32_MIN && v <= INT32_MAX; }
// the reference's int32 division v / d over v in [lo, hi] is defined (no zero divisor, no
// INT_MIN / -1) and its operands fit
inline bool div_ok(Range v, int64_t d) {
  return d != 0 && fits_i32(v.lo) && fits_i32(v.hi) && !(d == -1 && v.lo == INT32_MIN);
}
// REORDER_BN pooled sum of 8: sum_i max(v_i, thr) + off, accumulated in int32 (layer2.c:97-111,
// layer4.c:99-130): every partial sum and the total must fit
inline bool pooled_range(Range v, int32_t off, Range* s) {
  const int64_t thr = -((int64_t)off >> 3);
  const int64_t mlo = std::max(v.lo, thr), mhi = std::max(v.hi, thr);
  if (!fits_i32(8 * mlo) || !fits_i32(8 * mhi)) return false;
  s->lo = 8 * mlo + off;
  s->hi = 8 * mhi + off;
  return fits_i32(s->lo) && fits_i32(s->hi);
}

// REORDER_BN pooling constants (images.hpp, build_devparams): the threshold clamped to [-V, V] and
// the offset term off + 8 max(thr, -V), thr = -(off >> 3).
inline void pool_consts(int32_t off, int64_t V, int32_t* thr_c, int32_t* offm) {
  const int64_t thr = -((int64_t)off >> 3);
  *thr_c = (int32_t)std::min(std::max(thr, -V), V);
  *offm = (int32_t)(uint32_t)((int64_t)off + 8 * std::max(thr, -V));  // the pooled sums wrap mod 2^32
}

}  // namespace mib
