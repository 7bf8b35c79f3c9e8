// forward_gen.hpp — gfx950 fused forward for every network geometry the reference's generator
// emits (edge-eegnet_wolf/data/gen_net_header.py:78-89): C <= 64 channels (channel-selected
// MI-BMInet inputs, QuantLab/.../PhysionetMMMI/edgeEEGNet/preprocess.py:86-87), 64 <= T <= 4096
// samples (every time window of the loaders: 480 and 960 in get_data.py:156-159, 1125 for
// BCI-IV-2a), 1 <= N <= 16 classes (the 2- and 3-class PhysioNet nets, get_data.py:73-82), with
// F1 = F2 = 16 and D = 1 as layer2.c:246 fixes them.
//
// The dimensions are kernel-uniform run-time values (GenParams), so one compiled kernel per input
// layout serves every geometry; the three geometries of the reference's own configurations keep
// their compile-time specialisations (forward_wg.hpp), which this file does not touch.
//
// One workgroup of NW = 8 wave64s owns one trial at a time (persistent, grid-strided), with two
// barriers per trial: waves 0-6 run layer 1 while wave 7 runs layers 4-5 of the previous trial
// and then the trial's last K7 layer-1 blocks.  Int8 trials arrive in LDS a trial ahead by
// LDS-DMA.  Every intermediate stays in LDS:
//   layer1  MFMA i32_16x16x64_i8: A = 16 samples x 64 channel slots, B = the 16 filters' weights
//           (zero past C), C-init = the offset.  Time-major trials: a lane's 16 bytes of sample
//           t are t C + 16 c .. +15 of the trial (chunk c = l1_chunk(g, C)), read as five aligned
//           dwords and realigned by v_alignbyte (one ds_read_b128 when every fragment is
//           16-byte aligned); channel-major trials (int8 or float32, quantised here) go through
//           the same LDS transpose as the specialised kernels (wg::stage_block, ds_read_b64_tr_b8).
//                                                               (reference: layer1.c:53-101)
//   layer2  the 64-tap depthwise xcorr as a banded-Toeplitz GEMM on MFMA i32_32x32x32_i8 (A = 32
//           output shifts x 96-tap band, rows permuted so that a lane holds two whole pool-8
//           windows; B = 16-byte slices of the layer-1 row), ReLU-pool and requant per lane.
//                                                               (reference: layer2.c:56-118, 139-210)
//   layer3  16-tap depthwise conv on MFMA i32_16x16x64_i8 with a block-diagonal K (the wave's two
//           filters), written transposed [u][f] (the reference's flip is index math).
//                                                               (reference: layer3.c:49-79)
//   layer4  16x16 pointwise on MFMA i32_32x32x32_i8 with a block-diagonal B (two 32-sample
//           blocks), ReLU-pool and requant per lane.               (reference: layer4.c:51-149)
//   layer5  N-class linear layer: four classes per pass, 16 lanes each, v_dot4 + a DPP prefix.
//                                                               (reference: layer5.c:43-89)
// Requantisation as in the compiled kernels: where the host proves the float form exact on every
// reachable value (requant_host.hpp: choose_reciprocal, choose_floor_form) the XR = false build runs
// it; any requant without a proven float form sends the set to the XR = true build, exact
// division (xdiv, forward_common.hpp) at layers 1-4.  Layer 5 always divides exactly (its
// sums pass 2^24 at T = 4096).  CB: balanced clipping ([-127, 127], golden model clip_balanced).
#pragma once
#include "entry_host.hpp"  // gen::Layout
#include "forward_wg.hpp"
#include "image_layout.hpp"  // GenParams, SmallG, Carve, carve_of, l1_chunk

namespace mib {
namespace gen {

__device__ __forceinline__ int clampq(int v, int lo) { return min(max(v, lo), 127); }
__device__ __forceinline__ unsigned pack4(int a, int b, int c, int d) {
  return (unsigned)(a & 255) | ((unsigned)(b & 255) << 8) | ((unsigned)(c & 255) << 16) | ((unsigned)d << 24);
}

typedef unsigned v4u __attribute__((ext_vector_type(4)));

// 16 bytes at byte offset o of the view, from five aligned dwords: each dword lies wholly inside
// or wholly outside num_records (which is a multiple of 4), so the range check zeroes no byte the
// trial holds.  v_alignbyte_b32(hi, lo, s) = bytes s .. s + 3 of hi:lo.  The offset is unsigned (the
// builtin's operand is the same 32 bits, and the hardware compares it with num_records unsigned):
// the arithmetic stays defined for the offsets just past 2^31 that the recording and epoch
// fetches form (forward_win.hpp, forward_ep.hpp).
__device__ __forceinline__ v4i load16u(wg::Rsrc r, unsigned o) {
  const unsigned o4 = o & ~3u, s = o & 3u;
  const v4u a = __builtin_amdgcn_raw_buffer_load_b128(r, (int)o4, 0, 0);
  const unsigned e = __builtin_amdgcn_raw_buffer_load_b32(r, (int)(o4 + 16u), 0, 0);
  return (v4i){(int)__builtin_amdgcn_alignbyte(a[1], a[0], s), (int)__builtin_amdgcn_alignbyte(a[2], a[1], s),
               (int)__builtin_amdgcn_alignbyte(a[3], a[2], s), (int)__builtin_amdgcn_alignbyte(e, a[3], s)};
}

// 16 float32 samples at byte offset o (a multiple of 4) of the view -> 16 int8: the reference's
// input quantisation (gen_input_header.py:66-76); the truncating convert lies in [-127, 127]
__device__ __forceinline__ v4i load16f(wg::Rsrc r, unsigned o, float qs, float qy) {
  v4i w;
#pragma unroll
  for (int m = 0; m < 4; m++) {
    const v4u f = __builtin_amdgcn_raw_buffer_load_b128(r, (int)(o + 16u * m), 0, 0);
    int q[4];
#pragma unroll
    for (int i = 0; i < 4; i++) q[i] = (int)wg::quantize1_f(__uint_as_float(f[i]), qs, qy);
    w[m] = (int)pack4(q[0], q[1], q[2], q[3]);
  }
  return w;
}

// The view of `bytes` bytes from p: base = p rounded down to a dword, delta = the rest,
// num_records = the bytes from base rounded up to a dword (a dword holding a byte of the span is
// inside the page of that byte, so the rounding reads no unmapped memory).  Unsigned: delta +
// bytes + 3 may pass 2^31 - 1 (a recording, forward_win.hpp).
struct View {
  wg::Rsrc r;
  int delta;
};
__device__ __forceinline__ View make_view(const int8_t* p, unsigned bytes) {
  const unsigned delta = (unsigned)((size_t)p & 3);
  View v;
  v.r = __builtin_amdgcn_make_buffer_rsrc((void*)(p - delta), (short)0, (int)((delta + bytes + 3u) & ~3u), 0x00020000);
  v.delta = (int)delta;
  return v;
}
// The view of trial b.
template <int L>
__device__ __forceinline__ View trial_view(const int8_t* x, long long b, int C, int T, int xstride) {
  const long long ct = (long long)C * T;
  return make_view(L == TM ? x + b * xstride : L == CT ? x + b * ct : x + 4 * b * ct, (unsigned)((L == F32 ? 4 : 1) * ct));
}

// The A fragment of layer-1 block blk (samples 16 blk .. +15), before staging: time-major, lane
// (j, g) holds channels 16 c .. +15 (c = l1_chunk(g, C)) of sample 16 blk + j (int8, or float32
// quantised here: F32TM, the layer-1 kernels of the windows and streams only); channel-major,
// lane c holds samples 16 blk .. +15 of channel c.  K-slots past C meet zero weights, so what those lanes read does not
// matter: the loads are unconditional (no per-lane branch between one block's loads and the next
// block's), and channel-major rows past C re-read row C - 1.  T: the row stride of the
// channel-major layouts, the trial's length or a whole recording's (win::k_layer1_rec).  The byte
// offsets are computed unsigned: the host admits recordings up to 2^31 - 1 bytes, so the offsets
// of the partial last block (samples >= T, rows past the last) reach a little past 2^31 (below
// 2^31 + 2^11).  The hardware compares the offset with num_records unsigned, so those loads return
// zeros; unsigned, the arithmetic that gets there is defined too.
template <int L>
__device__ __forceinline__ v4i l1_fetch(const View& v, int blk, int C, int T, int lane, float qs, float qy) {
  const unsigned uC = (unsigned)C, uT = (unsigned)T, ub = 16u * (unsigned)blk, d = (unsigned)v.delta;
  if constexpr (L == TM) {
    const unsigned j = lane & 15, g = lane >> 4;
    return load16u(v.r, d + (ub + j) * uC + 16u * (unsigned)l1_chunk((int)g, C));
  } else if constexpr (L == CT) {
    return load16u(v.r, d + (unsigned)min(lane, C - 1) * uT + ub);
  } else if constexpr (L == F32TM) {
    // TM's fragment in floats: the 64 bytes of channels 16 c .. +15 of sample 16 blk + j, quantised
    // here (delta = 0: the view is 4-byte aligned).  A slot past C holds the next sample's float or a
    // zero past the view, a finite int8 once quantised (NaN and the infinities too), and meets a
    // zero weight.
    const unsigned j = lane & 15, g = lane >> 4;
    return load16f(v.r, 4u * ((ub + j) * uC + 16u * (unsigned)l1_chunk((int)g, C)), qs, qy);
  } else {
    return load16f(v.r, 4u * ((unsigned)min(lane, C - 1) * uT + ub), qs, qy);
  }
}

struct TrK {
  static constexpr bool TR16 = false;  // wg::stage_block's P == 1 transpose (ds_read_b64_tr_b8)
};

// 16 bytes at p + s of the staged trial (p 4-byte aligned, s < 4): five aligned dwords, realigned
// by v_alignbyte.  Not a ds_read_b128 at p: off its 16-byte alignment that one is replayed at 64
// LDS cycles per wave-instruction (MI355X_MICROARCH.md, LDS), which made layer 1 the LDS array's
// largest user (general kernels)
__device__ __forceinline__ v4i lds16u(const int8_t* p, unsigned s) {
  const unsigned* q = (const unsigned*)p;
  unsigned d[5];
#pragma unroll
  for (int i = 0; i < 5; i++) d[i] = q[i];
  return (v4i){(int)__builtin_amdgcn_alignbyte(d[1], d[0], s), (int)__builtin_amdgcn_alignbyte(d[2], d[1], s),
               (int)__builtin_amdgcn_alignbyte(d[3], d[2], s), (int)__builtin_amdgcn_alignbyte(d[4], d[3], s)};
}

// A lane's layer-1 fragments in the staged trial: block blk's 16 bytes start at lb + step blk, with
// lb = delta + j C + 16 l1_chunk(g, C) (time-major) or delta + c T (channel-major, c = min(lane,
// C - 1)) and
// step = 16 C or 16.  step is a multiple of 4, so the byte shift lb & 3 is the same for every block
// and each block costs one address add.  AL: every fragment 16-byte aligned (delta = 0 and the row
// length a multiple of 16), one ds_read_b128 each; otherwise lds16u (at C = 64 its five dwords per
// lane would also meet 8-way bank conflicts).
struct L1Src {
  const int8_t* p;  // sraw + (lb & ~3)
  int step;
  unsigned sh;      // lb & 3
};
template <int L>
__device__ __forceinline__ L1Src l1_src(const int8_t* raw, int delta, int C, int T, int lane) {
  const int lb = L == TM ? delta + (lane & 15) * C + 16 * l1_chunk(lane >> 4, C) : delta + min(lane, C - 1) * T;
  return L1Src{raw + (lb & ~3), L == TM ? 16 * C : 16, (unsigned)(lb & 3)};
}
template <bool AL>
__device__ __forceinline__ v4i l1_fetch_lds(const L1Src& q, int blk) {
  const int8_t* p = q.p + q.step * blk;
  if constexpr (AL) return *(const v4i*)p;
  else return lds16u(p, q.sh);
}

// LDS-DMA of trial view v into the raw area: 1 KB pieces i = wave, wave + NW, ... (lane L's 16
// bytes land at byte 16 L of its piece); pieces past num_records land as zeros.  wg::dma_b128 is
// inline asm, so no barrier waits for it: the wave waits vmcnt(0) before barrier B (k_forward).
__device__ __forceinline__ void stage_trial(const View& v, int8_t* raw, int chunks, int wave, int lane) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's reads of the area have returned
  const unsigned base = wg::lds_addr(raw);
  for (int i = wave; i < chunks; i += NW) wg::dma_b128(v.r, 1024 * i + 16 * lane, 0, base + 1024 * i);
}

// Requant of one layer-1 output (acc = dot + offset, or its float-magic form): exact division
// (XR) or fma(acc bits, r, c) = RN((dot + off) r), truncated (the host proves it equals C's
// division on every reachable value).  Both clip to [LO, 127] (the upper bound and -128 by the
// saturating pack).
template <bool XR, bool CB>
__device__ __forceinline__ int rq1(int acc, unsigned m, int xs, float r, float c) {
  int y = XR ? xdiv(acc, m, xs) : (int)__builtin_fmaf(__int_as_float(acc), r, c);
  if (XR) y = min(y, 127);
  return CB ? max(y, -127) : XR ? max(y, -128) : y;
}
// four outputs in [-128, 127] (or to be saturated there) -> bytes 0..3
typedef unsigned short v2us __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned sat4(int a, int b, int c, int d) {
  // two saturating pairs joined as a 2 x 16-bit vector: one v_perm_b32, no masking
  const v2us t = {__builtin_amdgcn_ashr_pk_i8_i32(a, b, 0), __builtin_amdgcn_ashr_pk_i8_i32(c, d, 0)};
  return __builtin_bit_cast(unsigned, t);
}

struct L1C {  // a lane's layer-1 constants (filter lane & 15)
  v4i wf;
  int off, xs;
  unsigned m;
  float r, c;
};
// layout L's: time-major fragments (int8 or float32) take the K order of l1_chunk, the others the
// natural one
template <int L>
__device__ __forceinline__ L1C l1_consts(const GenParams* __restrict__ gp, int lane) {
  const int j = lane & 15;
  return L1C{is_time_major(L) ? gp->l1_b[lane] : gp->l1_bn[lane], gp->l1_off[j], gp->l1_xs[j], gp->l1_m[j], gp->l1_r[j], gp->l1_c[j]};
}

// The arithmetic of one layer-1 block: the fragment `raw` of 16 samples (l1_fetch; transposed
// through the wave's staging area stg unless time-major) -> y[r], the output of filter lane & 15 at
// sample 4 (lane >> 4) + r of the block, before the saturating pack.
template <int L, bool XR, bool CB>
__device__ __forceinline__ void l1_outputs(v4i raw, int8_t* stg, const L1C& k, int lane, int (&y)[4]) {
  const v4i a = is_time_major(L) ? raw : wg::stage_block<TrK>(raw, stg, lane);
  const v4i acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, k.wf, (v4i){k.off, k.off, k.off, k.off}, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 4; r++) y[r] = rq1<XR, CB>(acc[r], k.m, k.xs, k.r, k.c);
}

// One layer-1 block: the fragment `raw` of samples 16 blk .. +15 (l1_outputs) -> bytes 16 blk ..
// +15 of the sixteen filters' rows, `row` being that of the lane's filter lane & 15
// (g = lane >> 4).  last: the block holds samples >= lim, which are stored as zeros.
template <int L, bool XR, bool CB>
__device__ __forceinline__ void l1_block(v4i raw, int8_t* stg, const L1C& k, int blk, bool last, int lim, int8_t* row,
                                         int g, int lane) {
  int y[4];
  l1_outputs<L, XR, CB>(raw, stg, k, lane, y);
  // lane column j = filter j, rows 4 g + r = samples 16 blk + 4 g + r
  const int t0 = 16 * blk + 4 * g;
  if (last) {
#pragma unroll
    for (int r = 0; r < 4; r++) y[r] = t0 + r < lim ? y[r] : 0;
  }
  *(unsigned*)(row + t0) = sat4(y[0], y[1], y[2], y[3]);
}

// Layer 1: the blocks first, first + nw, ... < end -> y1 rows (position 32 + t).
// ST: the trial is staged in LDS (sraw).  The U blocks' loads are all issued before the first MFMA
// (slots past NB1 re-read the last block; their results are not stored).  U4: four blocks per
// group, else two (float32: always two).
template <int L, bool ST, bool XR, bool CB, bool U4 = true>
__device__ __forceinline__ void layer1(const GenParams* __restrict__ gp, const View& v, const int8_t* sraw, int8_t* y1,
                                       int y1s, int8_t* stg, const L1C& k, int first, int nw, int end, int lane,
                                       float qs, float qy) {
  const int C = gp->C, T = gp->T, NB1 = gp->NB1;
  const int j = lane & 15, g = lane >> 4;
  constexpr int U = L == F32 || !U4 ? 2 : 4;
  // staged fragments all 16-byte aligned (wave-uniform: a scalar branch per group of U blocks)
  const bool al = ST && v.delta == 0 && ((L == TM ? C : T) & 15) == 0;
  const L1Src src = l1_src<L>(sraw, v.delta, C, T, lane);
  for (int b0 = first; b0 < end; b0 += U * nw) {  // the blocks first, first + nw, ... < end
    v4i raw[U];
    if (al) {
#pragma unroll
      for (int u = 0; u < U; u++) raw[u] = l1_fetch_lds<true>(src, min(b0 + u * nw, end - 1));
    } else {
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int blk = min(b0 + u * nw, end - 1);
        if constexpr (ST) raw[u] = l1_fetch_lds<false>(src, blk);
        else raw[u] = l1_fetch<L>(v, blk, C, T, lane, qs, qy);
      }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int blk = b0 + u * nw;
      // (wave-uniform)  the trial's last block: samples >= T are zero (the xcorr's pad)
      if (blk < end) l1_block<L, XR, CB>(raw[u], stg, k, blk, blk == NB1 - 1, T, y1 + j * y1s + 32, g, lane);
    }
  }
}

// Layer 2 (layer2.c:56-118 REORDER_BN, :139-210 plain): the wave's filters 2 wave + fi.  Lane
// (n, h) of tile mt holds conv outputs 1024 mt + 32 n + 16 h + r (r < 16), i.e. the pool windows
// u0 = 128 mt + 4 n + 2 h and u0 + 1.
struct L2C {  // a wave's layer-2 constants (filters 2 wave, 2 wave + 1)
  v4i af[2][3];
  v4i at[2][2];   // tail bands
  int thr[2], off[2], xs[2];
  unsigned m[2];
  float r[2], c[2];
};

// floor form of one plain-branch element (requant_host.hpp, choose_floor_form): acc holds the bits of
// float(M + x) (MFMA C-init M + offset), and bits(fmed3(fma(acc, r, c), K, K + emax)) - bits(K) =
// clamp(floor(x / fac), 0, emax) = the element after its clip and ReLU
template <int EMAX>
__device__ __forceinline__ int floor_el(int acc, float r, float c) {
  const float g = __builtin_fmaf(__int_as_float(acc), r, c);
  return __float_as_int(__builtin_amdgcn_fmed3f(g, FMAGIC_F, FMAGIC_F + (float)EMAX)) - FMAGIC_I;
}

template <bool RB, bool XR, bool CB>
__device__ __forceinline__ void layer2(const GenParams* __restrict__ gp, const int8_t* y1, int y1s, int8_t* y2, int y2s,
                                       const L2C& k, int wave, int lane) {
  constexpr int LO = CB ? -127 : -128;
  const int T8 = gp->T8, MT = gp->MT;
  constexpr bool rb = RB;  // the blob's REORDER_BN flag (gp->rb), an instantiation
  const int n = lane & 31, h = lane >> 5;
  for (int mt = 0; mt < MT; mt++) {
    // both filters' B slices first: the six LDS reads overlap instead of each MFMA waiting on one
    v4i bs[2][3];
#pragma unroll
    for (int fi = 0; fi < 2; fi++)
#pragma unroll
      for (int s = 0; s < 3; s++)
        bs[fi][s] = *(const v4i*)(y1 + (2 * wave + fi) * y1s + 1024 * mt + 32 * n + 16 * h + 32 * s);
#pragma unroll
    for (int fi = 0; fi < 2; fi++) {
      const int f = 2 * wave + fi;
      // plain float form: the chain starts from the floor form's magic (+ offset >> 3)
      const int ci = (!rb && !XR) ? k.thr[fi] : 0;
      v16i acc;
#pragma unroll
      for (int i = 0; i < 16; i++) acc[i] = ci;
#pragma unroll
      for (int s = 0; s < 3; s++) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(k.af[fi][s], bs[fi][s], acc, 0, 0, 0);
      int q[2];
#pragma unroll
      for (int w = 0; w < 2; w++) {
        int sum = 0;
        if constexpr (rb) {
#pragma unroll
          for (int i = 0; i < 8; i++) sum += max(acc[8 * w + i], k.thr[fi]);
          sum += k.off[fi];
          q[w] = XR ? clampq(xdiv(sum, k.m[fi], k.xs[fi]), LO) : clampq((int)((float)sum * k.r[fi]), LO);
        } else {
          // func_xcorr_scale per element (clip to int8), ReLU, sum of 8 >> 3
#pragma unroll
          for (int i = 0; i < 8; i++)
            sum += XR ? min(max(xdiv(acc[8 * w + i] + k.off[fi], k.m[fi], k.xs[fi]), 0), 127)
                      : floor_el<127>(acc[8 * w + i], k.r[fi], k.c[fi]);
          q[w] = sum >> 3;  // in [0, 127]
        }
      }
      const int u0 = 128 * mt + 4 * n + 2 * h;
      int8_t* dst = y2 + f * y2s + 8 + u0;
      if (u0 + 1 < T8) *(unsigned short*)dst = (unsigned short)((q[0] & 255) | ((q[1] & 255) << 8));
      else if (u0 < T8) *dst = (int8_t)q[0];
    }
  }
  // Tail: the column blocks past the full tiles, when at most 16 per filter are left (gp->NTT
  // tiles): MFMA i32_16x16x64_i8, 16 output shifts x 16 columns of 16 outputs, K = the 128
  // window positions from the column's first output (the band reaches 79 of them).  Lane (col, g)
  // holds shifts 4 g .. 4 g + 3 of its column: half a pool window, whose other half sits in row
  // g ^ 1 and arrives by v_permlane16_swap.
  const int NTT = gp->NTT;
  const int col = lane & 15, g = lane >> 4;
  for (int tt = 0; tt < NTT; tt++) {
    const int p0 = 1024 * MT + 256 * tt + 16 * col;  // the column's first output (row position p0 + 32 - 32)
    v4i bt[2][2];
#pragma unroll
    for (int fi = 0; fi < 2; fi++)
#pragma unroll
      for (int s = 0; s < 2; s++) bt[fi][s] = *(const v4i*)(y1 + (2 * wave + fi) * y1s + p0 + 64 * s + 16 * g);
#pragma unroll
    for (int fi = 0; fi < 2; fi++) {
      const int ci = (!rb && !XR) ? k.thr[fi] : 0;
      v4i acc = (v4i){ci, ci, ci, ci};
#pragma unroll
      for (int s = 0; s < 2; s++) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(k.at[fi][s], bt[fi][s], acc, 0, 0, 0);
      int part = 0;
      if constexpr (rb) {
#pragma unroll
        for (int i = 0; i < 4; i++) part += max(acc[i], k.thr[fi]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; i++)
          part += XR ? min(max(xdiv(acc[i] + k.off[fi], k.m[fi], k.xs[fi]), 0), 127) : floor_el<127>(acc[i], k.r[fi], k.c[fi]);
      }
      const auto sw = __builtin_amdgcn_permlane16_swap((unsigned)part, (unsigned)part, false, false);
      const int tot = (int)(sw[0] + sw[1]);  // the whole window (rows g and g ^ 1 hold the same)
      int q;
      if constexpr (rb) q = XR ? clampq(xdiv(tot + k.off[fi], k.m[fi], k.xs[fi]), LO) : clampq((int)((float)(tot + k.off[fi]) * k.r[fi]), LO);
      else q = tot >> 3;
      const int u = (p0 >> 3) + (g >> 1);
      if (!(g & 1) && u < T8) y2[(2 * wave + fi) * y2s + 8 + u] = (int8_t)q;
    }
  }
}

// Layer 3 (layer3.c:49-79, conv.c:105): output u of filter f = sum_j y2p[u + j] W3t[j], y2p[i] at
// row byte i + 1, so a block of 16 outputs from u0 reads row bytes u0 + 1 .. u0 + 31.  One MFMA
// i32_16x16x64_i8 per 128 outputs of the wave's two filters, with a block-diagonal K as in the
// compiled kernels (forward_wg.hpp, layer3): columns 0..7 are filter 2w's blocks j = 0..7,
// columns 8..15 filter 2w+1's; K-slots 0..31 carry filter 2w's 32-byte windows and band
// (A[r][k] = W3t[k - r - 1], SmallG::l3_a), slots 32..63 filter 2w+1's; a lane whose K half
// belongs to the other filter reads 16 zero bytes.  D lane (col, g) holds outputs
// u0 + 4 g .. u0 + 4 g + 3 of its column's block, written to y3t[u][f] (net_layer3_flip_inplace as
// index math); windows past T8 read zero pads or other rows, and their outputs are not stored.
template <bool XR, bool CB>
__device__ __forceinline__ void layer3(const GenParams* __restrict__ gp, const SmallG* sg, const int8_t* y2, int y2s,
                                       int8_t* y3, int wave, int lane) {
  constexpr int LO = CB ? -127 : -128;
  const int T8 = gp->T8;
  const unsigned m = gp->l3_m;
  const int xs = gp->l3_xs;
  const float r = gp->l3_r, c = gp->l3_c;
  const int col = lane & 15, g = lane >> 4, fi = col >> 3, j = col & 7;
  const int f = 2 * wave + fi;
  asm volatile("" ::: "memory");  // the A fragment is read here, not kept in registers across the trial loop
  const v4i a = sg->l3_a[wave][lane];
  // this lane's 16 window bytes: its column's filter row when the K half is that filter's, else zeros
  const int8_t* src = (g >> 1) == fi ? y2 + f * y2s + 16 * j + 16 * (g & 1) : (const int8_t*)sg->zero16;
  const int step = (g >> 1) == fi ? 128 : 0;
  const int ci = XR ? 0 : FMAGIC_I;  // float form: |conv| < 2^22 rides on the magic (exact)
  for (int t = 0; 128 * t < T8; t++) {
    const v4i b = *(const v4i*)(src + step * t);
    const v4i acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, (v4i){ci, ci, ci, ci}, 0, 0, 0);
    const int u0 = 128 * t + 16 * j + 4 * g;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int y = XR ? xdiv(acc[q], m, xs) : (int)__builtin_fmaf(__int_as_float(acc[q]), r, c);
      if (u0 + q < T8) y3[16 * (u0 + q) + f] = (int8_t)clampq(y, LO);
    }
  }
}

// Layer 4 (layer4.c:51-149, FLIP_LAYERS): b[k][u] = W4[k] . y3t[u], pooled over u = 8 v .. 8 v + 7;
// REORDER_BN: sum max(b, thr) + off, / fac; plain: sum max(tdiv(b + off >> 3, fac >> 3), 0) >> 3.
// One MFMA i32_32x32x32_i8 per part p of 64 samples, as the compiled kernels' layer 4: A row i of
// lane (i, h) = y3t[64 p + 32 h + n(i)] in K-slots 16 h .. 16 h + 15 (n(i) = 16 ((i >> 2) & 1) +
// 4 (i >> 3) + (i & 3)); B block-diagonal (SmallG::l4_b: column c < 16 = channel c on slots 0..15,
// column c >= 16 = channel c - 16 on slots 16..31).  Lane (c, h) register r then holds
// b[c & 15][64 p + 32 (c >> 4) + 16 h + r]: the two pool windows v = 8 p + 4 (c >> 4) + 2 h + {0, 1}.
// Parts p0, p0 + pstep, ...; samples past T8 read other LDS bytes and feed only windows v >= T64,
// which are not stored.
template <bool RB, bool XR, bool CB>
__device__ __forceinline__ void layer4(const GenParams* __restrict__ gp, const int8_t* y3, int8_t* y4,
                                       const SmallG* sg, int lane, int p0, int pstep) {
  constexpr int LO = CB ? -127 : -128;
  const int T64 = gp->T64, T64A = gp->T64A;
  constexpr bool rb = RB;  // the blob's REORDER_BN flag (gp->rb), an instantiation
  // the lane's addresses and constants are derived and read here, per call: hoisted out of the
  // trial loop they were held in registers (and spilled in the plain float builds)
  int ln;
  asm volatile("v_mov_b32 %0, %1" : "=v"(ln) : "v"(lane));
  const int c = ln & 31, h = ln >> 5, k = c & 15;
  const int i = c;  // A row of this lane
  const int n = 16 * ((i >> 2) & 1) + 4 * (i >> 3) + (i & 3);
  asm volatile("" ::: "memory");
  const v4i bw = sg->l4_b[ln];
  const int thr = sg->l4_thr[k], off = sg->l4_off[k], xs = sg->l4_xs[k];
  const unsigned m = sg->l4_m[k];
  const float r4 = sg->l4_r[k], c4 = sg->l4_c[k];
  const int ci = (!rb && !XR) ? sg->l4_ci[k] : 0;  // plain float form: the floor form's C-init
  const int NP = (T64 + 7) / 8;
  for (int p = p0; p < NP; p += pstep) {
    const v4i a = *(const v4i*)(y3 + 16 * (64 * p + 32 * h + n));
    const v16i acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bw, (v16i){ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci}, 0, 0, 0);
    int q[2];
#pragma unroll
    for (int w = 0; w < 2; w++) {
      int sum = 0;
      if constexpr (rb) {
#pragma unroll
        for (int e = 0; e < 8; e++) sum += max(acc[8 * w + e], thr);
        q[w] = clampq(XR ? xdiv(sum + off, m, xs) : (int)((float)(sum + off) * r4), LO);
      } else {
        // plain: layer4.c:113-118 clips no element (the float form clamps at 1024, past which the
        // result saturates anyway)
#pragma unroll
        for (int e = 0; e < 8; e++) sum += XR ? max(xdiv(acc[8 * w + e] + off, m, xs), 0) : floor_el<1024>(acc[8 * w + e], r4, c4);
        q[w] = clampq(sum >> 3, LO);
      }
    }
    const int v = 8 * p + 4 * (c >> 4) + 2 * h;
    int8_t* dst = y4 + k * T64A + v;
    if (v + 1 < T64) *(unsigned short*)dst = (unsigned short)((q[0] & 255) | ((q[1] & 255) << 8));
    else if (v < T64) *dst = (int8_t)q[0];
  }
}

// Layer 5 (layer5.c:43-89, transform.c:47): z = W5[n] . y4 + b5[n], clip(z / fac) (pad columns
// meet zero weights).  Four classes per wave pass, sixteen lanes each: lane (n, c) sums dwords
// c, c + 16, ... of its class, a DPP row_shr prefix sum leaves the class total in the row's lane
// 15.  Class groups g0, g0 + gstep, ... of four classes.
template <bool CB>
__device__ __forceinline__ void layer5(const GenParams* __restrict__ gp, const int8_t* y4, const int8_t* w5,
                                       int8_t* out, int g0, int gstep, int lane) {
  constexpr int LO = CB ? -127 : -128;
  const int N = gp->N, rp = w5_row(gp->T64A) / 4;  // dwords of a padded y4 / weight row
  const int c = lane & 15;
  const int* b5 = (const int*)(w5 + N * 4 * rp);
  for (int n0 = 4 * g0; n0 < N; n0 += 4 * gstep) {
    const int n = n0 + (lane >> 4);
    const int* w = (const int*)(w5 + (n < N ? n : 0) * 4 * rp);
    int part = 0;
    for (int d = c; d < rp; d += 64) {  // rp is a multiple of 64: four independent reads per pass
#pragma unroll
      for (int q = 0; q < 4; q++)
        part = __builtin_amdgcn_sdot4(((const int*)y4)[d + 16 * q], w[d + 16 * q], part, false);
    }
    part += __builtin_amdgcn_update_dpp(0, part, 0x111, 0xF, 0xF, true);  // row_shr:1
    part += __builtin_amdgcn_update_dpp(0, part, 0x112, 0xF, 0xF, true);  // row_shr:2
    part += __builtin_amdgcn_update_dpp(0, part, 0x114, 0xF, 0xF, true);  // row_shr:4
    part += __builtin_amdgcn_update_dpp(0, part, 0x118, 0xF, 0xF, true);  // row_shr:8
    if (c == 15 && n < N) out[n] = (int8_t)clampq(xdiv(part + b5[n], gp->l5_m, gp->l5_xs), LO);
  }
}

// The workgroup's LDS areas (carve_of; layout: its argument).
struct Lds {
  Carve cv;
  SmallG* sg;
  int8_t *y1, *y2, *y3, *y4;
  int8_t* w5;  // the layer-5 weight rows, then the biases
};
__device__ __forceinline__ Lds lds_of(const GenParams* __restrict__ gp, int8_t* smem, int layout) {
  const Carve cv = carve_of(gp->C, gp->T, gp->N, gp->T8, gp->T64A, gp->NB1, gp->MT, gp->NTT, layout);
  return Lds{cv, (SmallG*)(smem + cv.sg), smem, smem + cv.y2, smem + cv.y3, smem + cv.y4, smem + cv.w5};
}

// What setup() brings in of one parameter set, in two pieces that a kernel changing sets between
// items (forward_bank.hpp) runs again: the wave's layer-2 constants ...
__device__ __forceinline__ void set_l2c(const GenParams* __restrict__ gp, L2C& k2, int wave, int lane) {
#pragma unroll
  for (int fi = 0; fi < 2; fi++) {
    const int f = 2 * wave + fi;
#pragma unroll
    for (int s = 0; s < 3; s++) k2.af[fi][s] = gp->l2_a[f][s][lane];
#pragma unroll
    for (int s = 0; s < 2; s++) k2.at[fi][s] = gp->l2t_a[f][s][lane];
    k2.thr[fi] = gp->l2_thr[f];
    k2.off[fi] = gp->l2_off[f];
    k2.m[fi] = gp->l2_m[f];
    k2.xs[fi] = gp->l2_xs[f];
    k2.r[fi] = gp->l2_r[f];
    k2.c[fi] = gp->l2_c[f];
  }
}
// ... and the LDS copies of the small params, the layer-5 rows and the biases.
__device__ __forceinline__ void set_lds(const GenParams* __restrict__ gp, const Lds& m, int tid) {
  const v4i* src = (const v4i*)&gp->sg;
  v4i* dst = (v4i*)m.sg;
  for (int i = tid; i < (int)(sizeof(SmallG) / 16); i += NT) dst[i] = src[i];
  const int row5 = F2 * gp->T64A, rp = w5_row(gp->T64A) / 4;  // layer-5 weight rows, [N][rp dwords]
  int* w5 = (int*)m.w5;
  for (int i = tid; i < gp->N * rp; i += NT) {
    const int n = i / rp, d = i - n * rp;
    w5[i] = 4 * d < row5 ? ((const int*)gp->l5_w[n])[d] : 0;
  }
  for (int n = tid; n < gp->N; n += NT) w5[gp->N * rp + n] = gp->l5_b[n];
}

// The wave's layer-2 constants and the LDS initialisation shared by every kernel of the family.
__device__ __forceinline__ void setup(const GenParams* __restrict__ gp, const Lds& m, L2C& k2, int tid, int wave,
                                      int lane) {
  set_l2c(gp, k2, wave, lane);
  // zero pads of every row (positions past the data are never rewritten), then the small params
  v4i* z = (v4i*)m.y1;
  for (int i = tid; i < m.cv.sg / 16; i += NT) z[i] = (v4i){0, 0, 0, 0};
  set_lds(gp, m, tid);
}

// Layers 4-5 of the trial whose layer-3 rows are in y3, on one wave: its logits -> out[N].
template <bool RB, bool XR, bool CB>
__device__ __forceinline__ void finish_trial(const GenParams* __restrict__ gp, const Lds& m, int8_t* out, int lane) {
  layer4<RB, XR, CB>(gp, m.y3, m.y4, m.sg, lane, 0, 1);
  wg::wave_sync_lds();
  layer5<CB>(gp, m.y4, m.w5, out, 0, 1, lane);
}

// What the last wave owes the previous item of a persistent loop (item_loop's `prev`: i valid,
// -2 - i invalid, -1 none): its layers 4-5, or a zero logit row and a count in *n_bad.
template <bool RB, bool XR, bool CB, bool ONSETS>
__device__ __forceinline__ void finish_prev(const GenParams* __restrict__ gp, const Lds& m, int8_t* __restrict__ out,
                                            int* __restrict__ n_bad, int prev, int N, int lane) {
  if (prev != -1) {
    const bool vprev = !ONSETS || prev >= 0;
    int8_t* o = out + (size_t)(vprev ? prev : -2 - prev) * N;
    if (vprev) {
      __builtin_amdgcn_s_setprio(wg::PRIO_L45);
      finish_trial<RB, XR, CB>(gp, m, o, lane);
      __builtin_amdgcn_s_setprio(0);
    } else {
      if (lane < N) o[lane] = 0;
      if (lane == 0 && n_bad) atomicAdd(n_bad, 1);
    }
  }
}

// The layer-4 activations of the item whose y4 rows this wave has just written, for the entries that
// return them beside the logits (net_model_compute_epochs_bank_feat, net_streams_windows_at_feat):
// rows k < 16, columns v < T64 of y4 (row stride T64A) -> dst[k T64 + v], the T64_ALIGN pad columns
// dropped: the bytes layer 5 multiplies.  dst is 16-byte aligned and an item's row is 16 T64 bytes,
// so where T64 is a multiple of 4 (T64A = T64: the rows are contiguous in LDS too) it is T64 pieces
// of 16 bytes, one per lane; otherwise each y4 row leaves as T64 bytes.  T64 <= 64 (TMAX / 64).
__device__ __forceinline__ void store_feat(const int8_t* y4, int T64, int T64A, int8_t* __restrict__ dst, int ln) {
  // the lane's addresses are derived here, per call, from an opaque copy of the lane (layer4's device)
  int lane;
  asm volatile("v_mov_b32 %0, %1" : "=v"(lane) : "v"(ln));
  if ((T64 & 3) == 0) {
    if (lane < T64) ((v4i*)dst)[lane] = ((const v4i*)y4)[lane];
  } else {
    if (lane < T64) {
      // (by four: all sixteen rows' addresses at once cost the plain float builds up to 132 bytes of scratch)
#pragma unroll 4
      for (int k = 0; k < F2; k++) dst[k * T64 + lane] = y4[k * T64A + lane];
    }
  }
}

// finish_prev with the feature row beside the logit row.  A SIBLING OF finish_prev (and of
// finish_trial inside it), not a flag on them: a template parameter there changed the names, and a
// run-time one the code, of every existing instantiation (tools/asm_cmp.py).  The features leave
// after layer 4 and the wave's LDS sync, before layer 5: y4 is this wave's until its next call, so no
// barrier is added.  An invalid item gets 16 T64 zero bytes (T64 pieces of 16) as it gets N zero
// logits, and is counted once.  T64: every set's (the geometry), so the invalid branch reads no set.
template <bool RB, bool XR, bool CB>
__device__ __forceinline__ void finish_prev_feat(const GenParams* __restrict__ gp, const Lds& m,
                                                 int8_t* __restrict__ out, int8_t* __restrict__ feat,
                                                 int* __restrict__ n_bad, int prev, int N, int T64, int lane) {
  if (prev != -1) {
    const bool vprev = prev >= 0;
    const size_t item = (size_t)(vprev ? prev : -2 - prev);
    int8_t* o = out + item * N;
    int8_t* f = feat + item * (size_t)(F2 * T64);
    if (vprev) {
      __builtin_amdgcn_s_setprio(wg::PRIO_L45);
      layer4<RB, XR, CB>(gp, m.y3, m.y4, m.sg, lane, 0, 1);
      wg::wave_sync_lds();
      store_feat(m.y4, T64, (T64 + 3) & ~3, f, lane);
      layer5<CB>(gp, m.y4, m.w5, o, 0, 1, lane);
      __builtin_amdgcn_s_setprio(0);
    } else {
      if (lane < N) o[lane] = 0;
      // (the zero is made here: as a constant it was hoisted out of the loop, held in four registers
      // across every layer and spilled in the plain float builds)
      int zero;
      asm volatile("v_mov_b32 %0, 0" : "=v"(zero));
      if (lane < T64) ((v4i*)f)[lane] = (v4i){zero, zero, zero, zero};
      if (lane == 0 && n_bad) atomicAdd(n_bad, 1);
    }
  }
}

// The persistent loop of the kernels that read their items where they lie (win::k_forward_y1,
// win::k_forward_y1_at, ep::k_forward_ep): items blockIdx.x, + gridDim.x, ... < n, logits [n][N].
// Two barriers per item, as k_forward: waves 0 .. NW-2 bring in item i's y1 rows while the last
// wave finishes the previous item (layers 4-5; its y3t and y4 are untouched until this item's
// layer 3); A: layer 2 reads every wave's part of the y1 rows; B: layer 4 reads every filter's
// layer-3 rows.  One pass more than the workgroup has items: the last pass only finishes the last
// item (one copy of that code in the kernel).  The source src says where an item's data comes from:
//   src.open(i, more)   (wave-uniform) item i's descriptor, with .valid; on the pass past the last
//                       item (more false) it loads nothing;
//   src.rows(it)        what waves 0 .. NW-2 do with the item;
//   src.rows_last(it)   what the last wave does with it after finishing the previous item (both
//                       leave the wave at priority 0: a reset at the join of the two branches
//                       cost the window kernels up to 2 %);
//   S::ONSETS           items may be invalid (a caller-given onset out of range): such an item's
//                       layers 2-3 run on whatever the y1 rows hold and their result is dropped, its
//                       logit row is written as zeros and *n_bad (if non-null) counts it.  The
//                       previous item and its validity travel in one register: i valid, -2 - i
//                       invalid, -1 none.
// (phase stamps in tools/ builds with -DMIB_STAMPS, as k_forward: 0 the rows / the last wave's
// layers 4-5, 1 barrier A, 2 layer 2, 3 layer 3, 4 barrier B, 7 loop top)
template <bool RB, bool XR, bool CB, class S>
__device__ __forceinline__ void item_loop(const GenParams* __restrict__ gp, const Lds& m, const L2C& k2, const S& src,
                                          int8_t* __restrict__ out, int* __restrict__ n_bad, int n, int wave,
                                          int lane) {
  const int N = gp->N;
  MIB_STAMP_INIT
  int prev = -1;
  for (int i = blockIdx.x;; i += gridDim.x) {
    const bool more = i < n;  // uniform over the workgroup
    MIB_STAMP(7)
    const auto it = src.open(i, more);
    if (wave < NW - 1) {
      if (more) src.rows(it);
    } else {
      finish_prev<RB, XR, CB, S::ONSETS>(gp, m, out, n_bad, prev, N, lane);
      if (more) src.rows_last(it);
    }
    MIB_STAMP(0)
    if (!more) break;
    __syncthreads();  // A
    MIB_STAMP(1)
    layer2<RB, XR, CB>(gp, m.y1, m.cv.y1s, m.y2, m.cv.y2s, k2, wave, lane);
    wg::wave_sync_lds();  // layer 3 of filter f reads only y2 row f, written by this wave
    MIB_STAMP(2)
    __builtin_amdgcn_s_setprio(wg::PRIO_L3);
    layer3<XR, CB>(gp, m.sg, m.y2, m.cv.y2s, m.y3, wave, lane);
    __builtin_amdgcn_s_setprio(0);
    MIB_STAMP(3)
    __syncthreads();  // B
    MIB_STAMP(4)
    prev = !S::ONSETS || it.valid ? i : -2 - i;
  }
  MIB_STAMP_FLUSH(lane == 0, wave)
}

// Fused forward over a batch of B trials (layout L), logits [B][N].
// ST: int8 trials staged in LDS (the carve's raw area fits; the host picks the instantiation)
template <int L, bool ST, bool RB, bool XR, bool CB>
// two workgroups per CU (4 waves per SIMD): at most 128 VGPRs
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_forward(
    const GenParams* __restrict__ gp, const int8_t* __restrict__ x,
                                                 int8_t* __restrict__ out, int B, float qs, float qy) {
  static_assert(!ST || L != F32, "float32 trials are not staged");
  extern __shared__ v4i smem_v[];
  int8_t* smem = (int8_t*)smem_v;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const Lds m = lds_of(gp, smem, L);
  const Carve& cv = m.cv;
  const L1C k1 = l1_consts<L>(gp, lane);
  L2C k2;
  setup(gp, m, k2, tid, wave, lane);
  int8_t* stg = smem + cv.stg + 1024 * wave;
  // layer-1 groups of two blocks when two workgroups share the CU (the other one's waves cover the
  // latency; a wave's ~10 blocks then leave no slot re-reading the last block), of four at one
  // workgroup per CU (general kernels)
  const bool two_wg = cv.bytes <= LDS_2WG;
  const int C = gp->C, T = gp->T, N = gp->N, xstride = gp->xstride, NB1 = gp->NB1;
  const int K7 = L == TM && !two_wg ? gp->K7T1 : gp->K7;
  // int8 trials staged in LDS (cv.raw >= 0, uniform): the first one now; after that each trial a
  // grid stride ahead, by LDS-DMA issued after barrier A (layer 1 has read the area) and waited for
  // before barrier B, so it lands during layers 2-3 and no wave waits on HBM in layer 1
  int8_t* sraw = ST ? smem + cv.raw : nullptr;
  if (ST && (int)blockIdx.x < B) {
    stage_trial(trial_view<L>(x, blockIdx.x, C, T, xstride), sraw, cv.chunks, wave, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  // (phase stamps in tools/ builds with -DMIB_STAMPS: 0 layer 1 / the last wave's layers 4-5,
  // 1 barrier A, 2 layer 2, 3 layer 3, 4 barrier B, 7 loop top)
  MIB_STAMP_INIT
  // Two barriers per trial.  Waves 0 .. NW-2 run layer 1 while the last wave runs layers 4 and 5
  // of the previous trial (its y3t and y4 are untouched until this trial's layer 3, after barrier
  // A), as the compiled kernels do (forward_wg.hpp); A: layer 2 reads every wave's layer-1 rows;
  // B: layer 4 reads every filter's layer-3 rows.  The next trial's LDS-DMA goes out after A (layer
  // 1 has read the area) and is waited for before B.
  int bprev = -1;
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const View v = trial_view<L>(x, b, C, T, xstride);
    // layer-1 groups of two or of four blocks.  Captures by value: by reference the kernels came
    // out up to about 60 instructions longer and two VGPRs wider ("One layer-1 block")
    const auto l1 = [=](int first, int nw, int end) __attribute__((always_inline)) {
      if (two_wg) layer1<L, ST, XR, CB, false>(gp, v, sraw, m.y1, cv.y1s, stg, k1, first, nw, end, lane, qs, qy);
      else layer1<L, ST, XR, CB>(gp, v, sraw, m.y1, cv.y1s, stg, k1, first, nw, end, lane, qs, qy);
    };
    MIB_STAMP(7)
    // priorities as in the compiled kernels (wg::PRIO_*): the last wave's layers 4-5 are the longest
    // dependency chain of the interval and issue first; layer 1 ahead of the other workgroup's 2-3
    if (wave < NW - 1) {
      __builtin_amdgcn_s_setprio(wg::PRIO_L1);
      l1(wave, NW - 1, NB1 - K7);
    } else {
      if (bprev >= 0) {
        __builtin_amdgcn_s_setprio(wg::PRIO_L45);
        finish_trial<RB, XR, CB>(gp, m, out + (size_t)bprev * N, lane);
      }
      // then the trial's last K7 layer-1 blocks (host-balanced against layers 4-5)
      if (K7 > 0) {
        __builtin_amdgcn_s_setprio(wg::PRIO_L1);
        l1(NB1 - K7, 1, NB1);
      }
    }
    __builtin_amdgcn_s_setprio(0);
    MIB_STAMP(0)
    __syncthreads();  // A
    const int bn = b + (int)gridDim.x;
    if (ST && bn < B) stage_trial(trial_view<L>(x, bn, C, T, xstride), sraw, cv.chunks, wave, lane);
    MIB_STAMP(1)
    layer2<RB, XR, CB>(gp, m.y1, cv.y1s, m.y2, cv.y2s, k2, wave, lane);
    wg::wave_sync_lds();  // layer 3 of filter f reads only y2 row f, written by this wave
    MIB_STAMP(2)
    __builtin_amdgcn_s_setprio(wg::PRIO_L3);
    layer3<XR, CB>(gp, m.sg, m.y2, cv.y2s, m.y3, wave, lane);
    __builtin_amdgcn_s_setprio(0);
    MIB_STAMP(3)
    if (ST) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's part of the next trial
    __syncthreads();  // B
    MIB_STAMP(4)
    bprev = b;
  }
  // the last trial's layers 4-5
  if (wave == NW - 1 && bprev >= 0) finish_trial<RB, XR, CB>(gp, m, out + (size_t)bprev * N, lane);
  MIB_STAMP_FLUSH(lane == 0, wave)
}

// Single-trial, single-layer kernel for the reference's per-layer entry points on the general
// path: stage 1..5 = net_layerN, 6 = net_layer3_flip_inplace; reference layouts in and out (pads
// zero).  Stage 1 takes the trial packed time-major [T][C] (the batched layout).
template <bool RB, bool XR, bool CB>
__global__ __launch_bounds__(NT) void k_layer(const GenParams* __restrict__ gp, const int8_t* __restrict__ in,
                                              int8_t* __restrict__ out, int stage) {
  extern __shared__ v4i smem_v[];
  int8_t* smem = (int8_t*)smem_v;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const Lds m = lds_of(gp, smem, 3);
  const Carve& cv = m.cv;
  const L1C k1 = l1_consts<TM>(gp, lane);
  L2C k2;
  setup(gp, m, k2, tid, wave, lane);
  const int C = gp->C, T = gp->T, T8 = gp->T8, T64 = gp->T64, T64A = gp->T64A;
  const int TA = (T + 3) & ~3, T8A = (T8 + 3) & ~3;
  __syncthreads();
  if (stage == 1) {  // [T][C] packed -> [F1][T_ALIGN]
    const View v = trial_view<TM>(in, 0, C, T, gp->xstride);
    layer1<TM, false, XR, CB>(gp, v, nullptr, m.y1, cv.y1s, nullptr, k1, wave, NW, gp->NB1, lane, 0.0f, 0.0f);
    __syncthreads();
    for (int i = tid; i < F2 * TA; i += NT) {
      const int f = i / TA, t = i - f * TA;
      out[i] = t < T ? m.y1[f * cv.y1s + 32 + t] : 0;
    }
  } else if (stage == 2) {  // [F1][T_ALIGN] -> [F2][T8_ALIGN]
    for (int i = tid; i < F2 * T; i += NT) {
      const int f = i / T, t = i - f * T;
      m.y1[f * cv.y1s + 32 + t] = in[f * TA + t];
    }
    __syncthreads();
    layer2<RB, XR, CB>(gp, m.y1, cv.y1s, m.y2, cv.y2s, k2, wave, lane);
    __syncthreads();
    for (int i = tid; i < F2 * T8A; i += NT) {
      const int f = i / T8A, u = i - f * T8A;
      out[i] = u < T8 ? m.y2[f * cv.y2s + 8 + u] : 0;
    }
  } else if (stage == 3) {  // [F2][T8_ALIGN] -> [F2][T8_ALIGN]
    for (int i = tid; i < F2 * T8; i += NT) {
      const int f = i / T8, u = i - f * T8;
      m.y2[f * cv.y2s + 8 + u] = in[f * T8A + u];
    }
    __syncthreads();
    layer3<XR, CB>(gp, m.sg, m.y2, cv.y2s, m.y3, wave, lane);
    __syncthreads();
    for (int i = tid; i < F2 * T8A; i += NT) {
      const int f = i / T8A, u = i - f * T8A;
      out[i] = u < T8 ? m.y3[16 * u + f] : 0;
    }
  } else if (stage == 4) {  // [T8][F2] -> [F2][T64_ALIGN]
    for (int i = tid; i < T8 * F2; i += NT) m.y3[i] = in[i];
    __syncthreads();
    layer4<RB, XR, CB>(gp, m.y3, m.y4, m.sg, lane, wave, NW);
    __syncthreads();
    for (int i = tid; i < F2 * T64A; i += NT) out[i] = m.y4[i];
  } else if (stage == 5) {  // [F2][T64_ALIGN] -> [N] (the pad columns read as zero)
    for (int i = tid; i < F2 * T64A; i += NT) m.y4[i] = (i % T64A) < T64 ? in[i] : 0;
    __syncthreads();
    layer5<CB>(gp, m.y4, m.w5, out, wave, NW, lane);  // class group w on wave w
  } else if (stage == 6) {  // flip [F2][T8_ALIGN] -> [T8][F2]
    for (int i = tid; i < F2 * T8A; i += NT) {
      const int u = i / F2, f = i - u * F2;
      out[i] = u < T8 ? in[f * T8A + u] : 0;
    }
  }
}

}  // namespace gen
}  // namespace mib
