// images.hpp — the two parameter images the kernels read, laid out from a parsed set and its
// requant plan (params_host.hpp) in the layouts of image_layout.hpp: DevParams for the compiled
// geometries (forward_wg.hpp) and gen::GenParams for the run-time-dimension kernels
// (forward_gen.hpp, forward_win.hpp, forward_ep.hpp).  Neither builder searches for a constant.
// HIP-free like params_host.hpp: included by device_state.hpp and bank_host.hpp, and built into the
// stand-alone host programs (tests/host_arith_main.cpp, tests/bank_host_main.cpp).
#pragma once
#include <memory>

#include "entry_host.hpp"  // gen::Layout
#include "image_layout.hpp"
#include "params_host.hpp"

namespace mib {

// A parameter image as uploaded: a wg DevParams (compiled geometries) or a gen::GenParams.
struct Image {
  std::shared_ptr<const void> data;
  size_t bytes = 0;
  bool same(const Image& o) const {
    return data == o.data || (bytes == o.bytes && std::memcmp(data.get(), o.data.get(), bytes) == 0);
  }
};
template <class P>
Image make_image(std::shared_ptr<P> p) {
  Image im;
  im.bytes = sizeof(P);
  im.data = std::move(p);
  return im;
}
// FNV-1a over an image's bytes (mibminet_test_image_digest; the pinned digests of tests/support.py)
inline uint64_t fnv1a(const Image& im) {
  uint64_t h = 1469598103934665603ull;
  const uint8_t* p = (const uint8_t*)im.data.get();
  for (size_t i = 0; i < im.bytes; i++) h = (h ^ p[i]) * 1099511628211ull;
  return h;
}

// ---- fragments both families read ------------------------------------------------------------
// Layer-2 A operand = banded weights (wg::layer2 and gen::layer2): row i <-> shift n(i) so that
// lane (c, h) register r holds output shift 16h + r (two complete pool-8 windows per lane).  PL:
// layer-1 row layout, 2 = parity-split planes (the specialised C <= 32 kernels), 1 = natural order.
inline void l2_bands(const HostParams& hp, int PL, v4i (*afrag)[3][64]) {
  for (int f = 0; f < F2; f++)
    for (int s = 0; s < 3; s++)
      for (int lane = 0; lane < 64; lane++) {
        const int i = lane & 31, hh = lane >> 5;
        const int n = 16 * ((i >> 2) & 1) + (i & 3) + 4 * (i >> 3);
        int8_t bytes[16];
        for (int jj = 0; jj < 16; jj++) {
          const int kq = 32 * s + 16 * hh + jj;  // K-slot
          // position in the 96-byte row window.  PL == 2: lane half hh reads
          // parity plane hh, bytes 16s .. 16s+15 of the block's window; PL == 1: natural order.
          const int kp = PL == 2 ? 2 * (16 * s + jj) + hh : kq;
          const int idx = kp - n - 1;            // tap (torch order)
          bytes[jj] = (int8_t)((idx >= 0 && idx < 64) ? hp.l2_weight_reverse[(size_t)f * 64 + idx] : 0);
        }
        std::memcpy(&afrag[f][s][lane], bytes, 16);
      }
}

// Layer 3 (wg::layer3 tile 1, gen::layer3): net_l3_weight is stored flipped (true convolution), so
// the torch-order taps are W3t[t] = net_l3_weight[f][15 - t].  A operand of MFMA i32_16x16x64_i8
// with a block-diagonal K: wave w's lane (row r = lane & 15, K group kg = lane >> 4) holds K-slots
// 16 (kg & 1) .. +15 of filter 2w + (kg >> 1)'s 32-byte window (byte 16 col + k of its layer-2 row
// window holds position k - 8 + 16 col; output 16 col + r uses bytes +1 .. +16), A[r][k] =
// W3t[k - r - 1].  Tile 2 of the compiled kernels (sh = 4) carries shift g on row 4g only.
inline void l3_bands(const HostParams& hp, int sh, v4i (*a)[64]) {
  for (int w = 0; w < F2 / 2; w++)
    for (int lane = 0; lane < 64; lane++) {
      const int r = lane & 15, kg = lane >> 4, f = 2 * w + (kg >> 1);
      int8_t bytes[16];
      for (int jj = 0; jj < 16; jj++) {
        const int t = 16 * (kg & 1) + jj - r / sh - 1;
        bytes[jj] = (r % sh == 0 && t >= 0 && t < 16) ? hp.l3_weight[(size_t)f * 16 + 15 - t] : 0;
      }
      std::memcpy(&a[w][lane], bytes, 16);
    }
}

// Layer 4 (wg::layer4, gen::layer4): B operand of MFMA 32x32x32 = W4^T, block diagonal: lane (column
// k, half h) holds K-slots 16h..16h+15; columns 0..15 carry output channels 0..15 on slots 0..15 and
// columns 16..31 repeat them on slots 16..31 (a second 32-sample time block rides in the other K
// half).
inline void l4_bfrag(const HostParams& hp, v4i* b) {
  for (int lane = 0; lane < 64; lane++) {
    const int k = lane & 31, hh = lane >> 5;
    int8_t bytes[16] = {0};
    if ((k >> 4) == hh) std::memcpy(bytes, &hp.l4_weight[(size_t)(k & 15) * F2], 16);
    std::memcpy(&b[lane], bytes, 16);
  }
}

// ---- compiled-geometry parameter image (forward_wg.hpp) ---------------------------------------
// Layers 1, 2 and 4 take the plan's float forms or, for an exact set, its xdiv constants.  Layers 3
// and 5 always use the float form; a set without one is NET_ERR_RANGE.
inline int build_devparams(const HostParams& hp, const Plan& pl, DevParams& dp) {
  const Dims& d = hp.d;
  if (d.F1 != F2 || d.F2 != F2 || d.N != N_OUT) return NET_ERR_UNSUPPORTED;
  if (d.C > 64) return NET_ERR_UNSUPPORTED;
  const int P = d.C <= 32 ? 2 : 1;
  const int C = d.C, CA = d.C_ALIGN();
  std::memset(&dp, 0, sizeof(dp));
  SmallParams& sp = dp.sp;
  auto w1 = [&](int f, int c) -> int { return hp.l1_weight_align[(size_t)f * CA + c]; };
  const bool xr = pl.xr;
  for (int t = 0; t < P; t++)
    for (int j = 0; j < 16; j++) {  // N-tile column j: filter 8t + j/2 (P == 2) or j (P == 1)
      const int f = P == 2 ? 8 * t + (j >> 1) : j;
      dp.l1_cinit[t][j] = pl.ci1[f];
      if (xr) {
        dp.l1_m[t][j] = pl.x1[f].m;
        dp.l1_xs[t][j] = pl.x1[f].xs;
      } else {
        dp.l1_r[t][j] = pl.f1[f].r;
        dp.l1_c[t][j] = pl.f1[f].c;
      }
    }
  for (int f = 0; f < F2; f++) {
    if (hp.reorder_bn) {
      // biased relu pooling (forward_common.hpp, pool8b): sum_8 max(v, thr) + off =
      // sum_8 max(v - thr, 0) + (off + 8 thr), thr = -(off >> 3) (layer2.c:97-111), with thr
      // clamped to the conv range [-V, V] (V = 64 * 128^2 = 2^20 in layer 2, 16 * 128^2 = 2^18 in
      // layer 4) so that the biased values cannot wrap.  Past the upper end every max(v, thr) is
      // thr: the relu terms are 0 either way and the offset term keeps the true thr.  Past the
      // lower end every max(v, thr) is v: with thr' = -V the relu terms are v + V, so the offset
      // term is off - 8 V.  Hence offm = off + 8 max(thr, -V).
      int32_t t2, t4;
      pool_consts(hp.l2_offset[f], 1 << 20, &t2, &dp.l2_offm[f]);
      pool_consts(hp.l4_offset[f], 1 << 18, &t4, &sp.l4_offm[f]);
      dp.l2_thrb[f] = pbias(f & 1) + t2;  // the wave's filter slot f & 1 (forward_wg.hpp, layer2)
      sp.l4_thr[f] = t4;
      int32_t rbits = 0, xs2 = 0;
      if (xr) {
        dp.l2_m[f] = pl.x2[f].m;
        sp.l2_xs[f] = pl.x2[f].xs;
        sp.l4_m[f] = pl.x4[f].m;
        sp.l4_xs[f] = pl.x4[f].xs;
        rbits = (int32_t)pl.x2[f].m;
        xs2 = pl.x2[f].xs;
      } else {
        dp.l2_r[f] = pl.f2[f].r;
        sp.l4_r[f] = pl.f4[f].r;
        std::memcpy(&rbits, &dp.l2_r[f], 4);
      }
      sp.l2_tpar[f] = (v4i){PBIAS_TAIL + t2, dp.l2_offm[f], rbits, xs2};
    } else {
      // plain branches: per-element BN with offset >> 3 and factor >> 3, ReLU right after.  Float:
      // the floor form, MFMA C-init = per-filter magic plus the offset.  Exact: C-init = the
      // offset, each element xdiv and a clamp.
      sp.l2n_ci[f] = pl.ci2[f];
      sp.l4n_ci[f] = pl.ci4[f];
      if (xr) {
        sp.l2n_m[f] = pl.x2[f].m;
        sp.l2_xs[f] = pl.x2[f].xs;
        sp.l4n_m[f] = pl.x4[f].m;
        sp.l4_xs[f] = pl.x4[f].xs;
      } else {
        sp.l2n_r[f] = pl.f2[f].r;
        sp.l2n_c[f] = pl.f2[f].c;
        sp.l4n_r[f] = pl.f4[f].r;
        sp.l4n_c[f] = pl.f4[f].c;
      }
    }
  }
  // layer 1: B operand (column j of N-tile t: filter 8t + j/2, parity j&1 when P == 2)
  for (int t = 0; t < P; t++) {
    for (int lane = 0; lane < 64; lane++) {
      const int j = lane & 15, g = lane >> 4;
      const int f = P == 2 ? 8 * t + (j >> 1) : j;
      const int p = P == 2 ? (j & 1) : 0;
      int8_t bytes[16];
      for (int jj = 0; jj < 16; jj++) {
        const int k = 16 * g + jj;  // byte of the 64-byte window
        const int c = k - C * p;    // channel of sample p in the window
        bytes[jj] = (int8_t)((c >= 0 && c < C) ? w1(f, c) : 0);
      }
      std::memcpy(&dp.l1_wfrag[t][lane], bytes, 16);
      // channel-major staging (forward_wg.hpp, stage_block): P == 2 K-slot 2c + p holds channel
      // c at sample 16 p + j of MFMA row j (column parity p selects it); P == 1 is the same slot
      // order as above
      for (int jj = 0; jj < 16; jj++) {
        const int k = 16 * g + jj;
        const int c = P == 2 ? k >> 1 : k, pk = P == 2 ? k & 1 : 0;
        bytes[jj] = (int8_t)((c < C && pk == p) ? w1(f, c) : 0);
      }
      std::memcpy(&dp.l1_wfrag_ct[t][lane], bytes, 16);
    }
  }
  l2_bands(hp, P, dp.l2_afrag);
  // layer-2 tail bands (forward_wg.hpp, layer2_tail_mfma): filter pair w = filters 2w, 2w+1;
  // lane (m, g) of K-step s holds K-slots 64 s + 16 g + jj = chunk kap = 4 s + g, byte jj, which
  // is chunk mq = kap - 6 kf of filter kf = kap / 6; its window position q (tail_q) meets tap
  // q - m - 1 of the output shift m.
  for (int w = 0; w < F2 / 2; w++)
    for (int s = 0; s < 3; s++)
      for (int lane = 0; lane < 64; lane++) {
        const int m = lane & 15, g = lane >> 4, kap = 4 * s + g, kf = kap / 6, mq = kap - 6 * kf;
        const int f = 2 * w + kf;
        int8_t bytes[16];
        for (int jj = 0; jj < 16; jj++) {
          const int q = P == 2 ? 32 * (mq >> 1) + 2 * jj + (mq & 1) : 16 * mq + jj;
          const int idx = q - m - 1;
          bytes[jj] = (int8_t)((idx >= 0 && idx < 64 && (P == 2 || mq < 5)) ? hp.l2_weight_reverse[(size_t)f * 64 + idx] : 0);
        }
        std::memcpy(&dp.l2t_afrag[w][s][lane], bytes, 16);
      }
  l3_bands(hp, 1, dp.l3_a1);
  l3_bands(hp, 4, dp.l3_a2);
  if (!pl.l3_ok) return NET_ERR_RANGE;
  sp.l3_r = pl.l3_r;
  sp.l3_c = pl.l3_c;
  l4_bfrag(hp, sp.l4_bfrag);
  const int T64 = d.T64(), T64A = d.T64_ALIGN();
  if (F2 * T64A / 4 > ND5_MAX) return NET_ERR_UNSUPPORTED;
  for (int n = 0; n < N_OUT; n++) {
    int8_t* dst = (int8_t*)sp.l5_w[n];
    for (int k = 0; k < F2; k++)
      for (int v = 0; v < T64; v++) dst[k * T64A + v] = hp.l5_weight[(size_t)n * F2 * T64A + k * T64A + v];
    sp.l5_b[n] = hp.l5_bias[n];
  }
  if (!pl.l5_ok) return NET_ERR_RANGE;
  sp.l5_r = pl.l5_r;
  return NET_OK;
}

// ---- general-geometry parameter image (forward_gen.hpp) ------------------------------------
// Every network gen_net_header.py emits with F1 = F2 = 16: C <= 64, 64 <= T <= gen::TMAX,
// 1 <= N <= gen::NMAX.
inline int gen_supported(const Dims& d) {
  if (d.F1 != F2 || d.F2 != F2 || d.D != 1) return NET_ERR_UNSUPPORTED;
  if (d.C < 1 || d.C > 64 || d.T < 64 || d.T > gen::TMAX || d.N < 1 || d.N > gen::NMAX) return NET_ERR_UNSUPPORTED;
  return NET_OK;
}

// The geometry of a supported set, the part of the image that depends on its dimensions alone (and
// all gen::carve_of takes): the layer-1 blocks, layer 2's tiles, the last wave's share of layer 1 and
// the time-major trial stride.
inline void gen_geometry(const Dims& d, gen::GenParams& gp) {
  const int T8 = d.T8(), T64 = d.T64();
  gp.C = d.C;
  gp.T = d.T;
  gp.N = d.N;
  gp.T8 = T8;
  gp.T64 = T64;
  gp.T64A = d.T64_ALIGN();
  gp.NB1 = (d.T + 15) / 16;
  const int NB2 = (8 * T8 + 31) / 32;  // layer-2 column blocks of 32 outputs
  // full 32x32 tiles of 32 blocks; at most 16 blocks left go to 16x16x64 tail tiles (16 columns of
  // 16 outputs each), more to one more full tile
  const int rest = NB2 % 32;
  gp.MT = NB2 / 32 + (rest > 16 ? 1 : 0);
  gp.NTT = (rest > 0 && rest <= 16) ? (2 * rest + 15) / 16 : 0;
  // the last wave runs layers 4-5 (about two layer-1 blocks' time per 64 samples of layer 4, on
  // the phase stamps) and then the trial's last K7 layer-1 blocks; the other seven share the rest:
  // (NB1 - K7) / 7 = 2 NP + K7, NP = layer-4 parts
  const int NP = (T64 + 7) / 8;
  gp.K7 = std::max(0, (gp.NB1 - 14 * NP) / 8);
  // time-major at one workgroup per CU: two fewer (same box: -0.9 ... -2.6 %; channel-major
  // measured +1.5 % and keeps K7, profiles/r06_ab_k7.txt)
  gp.K7T1 = std::max(0, gp.K7 - 2);
  gp.xstride = (int)trial_stride(d);
}

// Requant: the plan's float forms at layers 1-4 where every one is proven (gp.xr = 0), exact integer
// division (xdiv) at layers 1-4 otherwise (gp.xr = 1, the float fields zero); layer 5 always
// divides exactly.  The xdiv constants are there either way.
inline int build_genparams(const HostParams& hp, const Plan& pl, gen::GenParams& gp) {
  const Dims& d = hp.d;
  if (const int rc = gen_supported(d)) return rc;
  std::memset(&gp, 0, sizeof(gp));
  gen_geometry(d, gp);
  const int C = d.C, CA = d.C_ALIGN(), T64 = d.T64(), T64A = d.T64_ALIGN();
  const bool rb = hp.reorder_bn, xr = pl.xr || !pl.l3_ok;
  gp.rb = rb ? 1 : 0;
  gp.lo = hp.clip_balanced ? -127 : -128;
  gp.xr = xr ? 1 : 0;
  // layer 1: lane (filter j, K group g) holds channels 16 c .. 16 c + 15 (zero past C) of chunk c:
  // time-major c = gen::l1_chunk(g, C), zero in K groups 1 and 3 when C <= 32 (their lanes re-read
  // the previous group's bytes); natural order (channel-major, float32) c = g
  for (int lane = 0; lane < 64; lane++) {
    const int j = lane & 15, g = lane >> 4;
    int8_t bytes[16], nat[16];
    for (int i = 0; i < 16; i++) {
      const int c = 16 * gen::l1_chunk(g, C) + i, cn = 16 * g + i;
      bytes[i] = (c < C && !(C <= 32 && (g & 1))) ? hp.l1_weight_align[(size_t)j * CA + c] : 0;
      nat[i] = cn < C ? hp.l1_weight_align[(size_t)j * CA + cn] : 0;
    }
    std::memcpy(&gp.l1_b[lane], bytes, 16);
    std::memcpy(&gp.l1_bn[lane], nat, 16);
  }
  for (int f = 0; f < F2; f++) {
    // layers 2 and 4: REORDER_BN pools max(v, -(off >> 3)) and divides by factor; the plain
    // branches divide each element by factor >> 3 after adding offset >> 3 (float: the floor form,
    // whose magic bits ride in the MFMA C-init)
    const int32_t o2 = hp.l2_offset[f] >> 3, o4 = hp.l4_offset[f] >> 3;
    gp.l1_off[f] = xr ? hp.l1_offset[f] : pl.ci1[f];
    gp.l1_m[f] = pl.x1[f].m;
    gp.l1_xs[f] = pl.x1[f].xs;
    gp.l2_thr[f] = xr || rb ? -o2 : pl.ci2[f];
    gp.l2_off[f] = rb ? hp.l2_offset[f] : o2;
    gp.l2_m[f] = pl.x2[f].m;
    gp.l2_xs[f] = pl.x2[f].xs;
    gp.sg.l4_thr[f] = -o4;
    gp.sg.l4_off[f] = rb ? hp.l4_offset[f] : o4;
    gp.sg.l4_m[f] = pl.x4[f].m;
    gp.sg.l4_xs[f] = pl.x4[f].xs;
    if (xr) continue;
    gp.l1_r[f] = pl.f1[f].r;
    gp.l1_c[f] = pl.f1[f].c;
    gp.l2_r[f] = pl.f2[f].r;
    gp.l2_c[f] = pl.f2[f].c;
    gp.sg.l4_r[f] = pl.f4[f].r;
    gp.sg.l4_c[f] = pl.f4[f].c;
    if (!rb) gp.sg.l4_ci[f] = pl.ci4[f];
  }
  if (!xr) {
    gp.l3_r = pl.l3_r;
    gp.l3_c = pl.l3_c;
  }
  gp.l3_m = pl.x3.m;
  gp.l3_xs = pl.x3.xs;
  gp.l5_m = pl.x5.m;
  gp.l5_xs = pl.x5.xs;
  l4_bfrag(hp, gp.sg.l4_b);
  static_assert(gen::NW == F2 / 2, "one layer-3 fragment per filter pair");
  l3_bands(hp, 1, gp.sg.l3_a);
  l2_bands(hp, 1, gp.l2_a);
  // tail bands (gen::layer2): lane (shift m = lane & 15, g) of K-step s holds K-slots
  // 64 s + 16 g .. +15, window position k of the column meets tap k - m - 1
  for (int f = 0; f < F2; f++)
    for (int s = 0; s < 2; s++)
      for (int lane = 0; lane < 64; lane++) {
        const int m = lane & 15, g = lane >> 4;
        int8_t bytes[16];
        for (int jj = 0; jj < 16; jj++) {
          const int idx = 64 * s + 16 * g + jj - m - 1;
          bytes[jj] = (idx >= 0 && idx < 64) ? hp.l2_weight_reverse[(size_t)f * 64 + idx] : 0;
        }
        std::memcpy(&gp.l2t_a[f][s][lane], bytes, 16);
      }
  for (int n = 0; n < d.N; n++) {
    gp.l5_b[n] = hp.l5_bias[n];
    for (int k = 0; k < F2; k++)
      for (int v = 0; v < T64; v++) gp.l5_w[n][k * T64A + v] = hp.l5_weight[((size_t)n * F2 + k) * T64A + v];
  }
  return NET_OK;
}

// ---- compiled configurations --------------------------------------------------------------
// The compiled geometry of (C, T, N), or -1: 0: 22 x 1125 (BCI-IV-2a: configs A, B, D, E), 1:
// 64 x 1000 (config C), 2: 64 x 480 (the reference's PhysioNet MMMI edgeEEGNet,
// QuantLab/PhysionetMMMI/config_INQ.json).  Every other geometry (and N != 4) runs the general
// kernels.
inline int compiled_shape(const Dims& d) {
  if (d.F1 != F2 || d.F2 != F2 || d.N != N_OUT) return -1;
  if (d.C == 22 && d.T == 1125) return 0;
  if (d.C == 64 && d.T == 1000) return 1;
  if (d.C == 64 && d.T == 480) return 2;
  return -1;
}

// Both images of a set whose ranges are known, from one plan.  img: what the batched kernels read
// (DevParams, or the GenParams when h.general).  win: the gen::GenParams of the window and epoch
// kernels: img itself on the general path, one of its own for a compiled geometry (empty where
// none can be built: such a set has no window kernels).  Sets h.xr and the first unproven requant.
inline int build_images(HostParams& h, const Ranges& rg, Image* img, Image* win) {
  const Plan pl = make_plan(h, rg);
  auto gp = std::make_shared<gen::GenParams>();
  const int grc = build_genparams(h, pl, *gp);
  *win = grc == NET_OK ? make_image(gp) : Image();
  if (h.general) {
    if (grc) return grc;
    *img = *win;
    h.xr = gp->xr != 0;
    return NET_OK;
  }
  auto dp = std::make_shared<DevParams>();
  if (const int rc = build_devparams(h, pl, *dp)) return rc;
  *img = make_image(dp);
  h.xr = pl.xr;
  h.xr_layer = pl.xr_layer;
  h.xr_filter = pl.xr_filter;
  return NET_OK;
}

// The images of a parsed set: the compiled kernels' where its geometry has them (and force_general
// is off), the general kernels' otherwise.  A set off the float envelope has its constant filters
// folded into an equivalent copy (the reference ranges, NET_ERR_RANGE included, are checked on the
// set as given) and keeps that copy's images, float if every remaining requant is proven, exact
// otherwise (xr_layer / xr_filter then name a filter that really varies).
inline int build_set(HostParams& hp, bool force_general, Image* img, Image* win) {
  hp.general = force_general || compiled_shape(hp.d) < 0;
  if (hp.general)
    if (const int rc = gen_supported(hp.d)) return rc;
  Ranges rg;
  if (const int rc = check_ranges(hp, rg)) return rc;
  if (const int rc = build_images(hp, rg, img, win)) return rc;
  if (!hp.xr) return NET_OK;
  HostParams fh = hp;
  Ranges frg;
  Image fimg, fwin;
  if ((fh.folded = fold_constant_filters(fh, rg)) > 0 && check_ranges(fh, frg) == NET_OK &&
      build_images(fh, frg, &fimg, &fwin) == NET_OK) {
    *img = fimg;
    *win = fwin;
    hp.xr = fh.xr;
    hp.xr_layer = fh.xr_layer;
    hp.xr_filter = fh.xr_filter;
    hp.folded = fh.folded;
  }
  return NET_OK;
}

}  // namespace mib
