// forward_ep.hpp — epochs cut out of a wider array (gfx950): channel selection, cropping and
// event-locked epochs straight from the source, with no gathered [E][C][T] copy
// (net_model_compute_epochs, include/mibminet.h).
//
// Epoch e, network channel c, sample t is element onsets[e] + channels[c] row_stride + t of the
// flat source.  In the channel-major layer 1 lane c already forms its own row address
// (gen::l1_fetch<CT>: min(lane, C - 1) T + 16 blk); here the row part comes from a per-lane table
// entry and the base from the epoch's onset:
//   per epoch  (wave-uniform) the onset is loaded and range-checked, and the epoch's span becomes
//              one buffer view as gen::trial_view builds it;
//   per lane   (once per kernel) rowoff = elem_size channels[min(lane, C - 1)] row_stride;
//   per block  one unaligned 16-byte fetch at delta + rowoff + 16 blk (float32: four 16-byte loads
//              and the input quantiser, as gen::l1_fetch<F32>).
// Layers 2-5, the persistent loop and its two barriers are gen::'s own, on a gen::GenParams image
// (every geometry, the compiled ones included: the image the window kernels use).
#pragma once
#include "forward_win.hpp"

namespace mib {
namespace ep {

// The loaded network's channel -> source row table, a by-value kernel argument.
struct ChanTab {
  int c[64];
};

// The view of the epoch at element onset `on` (valid: 0 <= on <= n_elems - span): base = its first
// byte rounded down to a dword, delta = the rest, num_records = the span's bytes from the base
// rounded up to a dword (gen::trial_view).  The span lies inside the source, so no load through
// the view leaves it by more than the dword rounding.
template <int L>
__device__ __forceinline__ gen::View epoch_view(const int8_t* x, long long on, unsigned span_bytes) {
  const int8_t* p = x + (L == gen::F32 ? 4 : 1) * on;
  const unsigned delta = (unsigned)((size_t)p & 3);
  gen::View v;
  v.r = __builtin_amdgcn_make_buffer_rsrc((void*)(p - delta), (short)0, (int)((delta + span_bytes + 3u) & ~3u), 0x00020000);
  v.delta = (int)delta;
  return v;
}

// The lane's 16 samples of block blk (from its row's byte offset rowoff inside the view), offsets
// unsigned: elem_size span + 6 < 2^31 (the host's limit) keeps every in-range offset below 2^31,
// and the partial last block's reads past the span (zeros: past num_records) stay defined.
template <int L>
__device__ __forceinline__ v4i ep_fetch(const gen::View& v, unsigned rowoff, int blk, float qs, float qy) {
  if constexpr (L == gen::CT) {
    return win::load16u_u(v.r, (unsigned)v.delta + rowoff + 16u * (unsigned)blk);
  } else {
    v4i w;
#pragma unroll
    for (int m = 0; m < 4; m++) {
      const gen::v4u f = __builtin_amdgcn_raw_buffer_load_b128(v.r, (int)(rowoff + 64u * (unsigned)blk + 16u * m), 0, 0);
      int q[4];
#pragma unroll
      for (int i = 0; i < 4; i++) q[i] = (int)wg::quantize1_f(__uint_as_float(f[i]), qs, qy);
      w[m] = (int)gen::pack4(q[0], q[1], q[2], q[3]);
    }
    return w;
  }
}

// gen::layer1's unstaged loop (ST = false) with ep_fetch: blocks first, first + nw, ... < end ->
// y1 rows (position 32 + t), the U blocks' loads issued before their MFMAs.  A partial last block
// reads whatever follows the epoch in its row (zeros past the view's end); its samples >= T are
// stored as zeros, so nothing read there (a non-finite float included) reaches a stored sample.
template <int L, bool XR, bool CB, bool U4>
__device__ __forceinline__ void layer1_ep(const gen::GenParams* __restrict__ gp, const gen::View& v, unsigned rowoff,
                                          int8_t* y1, int y1s, int8_t* stg, const gen::L1C& k, int first, int nw,
                                          int end, int lane, float qs, float qy) {
  const int T = gp->T, NB1 = gp->NB1;
  // the store addresses are derived here, per call (gen::layer4's device): hoisted out of the epoch
  // loop they were held in registers across layers 2-3, and spilled in the plain float builds
  int ln;
  asm volatile("v_mov_b32 %0, %1" : "=v"(ln) : "v"(lane));
  const int j = ln & 15, g = ln >> 4;
  constexpr int U = L == gen::F32 || !U4 ? 2 : 4;
  for (int b0 = first; b0 < end; b0 += U * nw) {
    v4i raw[U];
#pragma unroll
    for (int u = 0; u < U; u++) raw[u] = ep_fetch<L>(v, rowoff, min(b0 + u * nw, end - 1), qs, qy);
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int blk = b0 + u * nw;
      if (blk < end) {  // wave-uniform
        const v4i a = wg::stage_block<gen::TrK>(raw[u], stg, lane);
        const v4i acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, k.wf, (v4i){k.off, k.off, k.off, k.off}, 0, 0, 0);
        const int t0 = 16 * blk + 4 * g;
        int y[4];
#pragma unroll
        for (int r = 0; r < 4; r++) y[r] = gen::rq1<XR, CB>(acc[r], k.m, k.xs, k.r, k.c);
        if (blk == NB1 - 1) {
#pragma unroll
          for (int r = 0; r < 4; r++) y[r] = t0 + r < T ? y[r] : 0;
        }
        *(unsigned*)(y1 + j * y1s + 32 + t0) = gen::sat4(y[0], y[1], y[2], y[3]);
      }
    }
  }
}

// Fused forward over E epochs of the source x (layout L: CT int8, F32 float32), logits [E][N].
// last = n_elems - span, the largest valid onset; span_bytes = elem_size span.  An onset outside
// [0, last] forms no address: its epoch is read at onset 0 and discarded, its logit row is written
// as zeros and *n_bad (if non-null) counts it.  gen::k_forward's loop in win::k_forward_y1's form
// (one pass more than the workgroup has epochs; the last pass only finishes the last epoch).
template <int L, bool RB, bool XR, bool CB>
__global__ __launch_bounds__(gen::NT) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_forward_ep(
    const gen::GenParams* __restrict__ gp, const int8_t* __restrict__ x, const long long* __restrict__ onsets,
    int8_t* __restrict__ out, int* __restrict__ n_bad, int E, long long last, unsigned span_bytes,
    unsigned long long row_stride, const ChanTab tab, float qs, float qy) {
  using namespace gen;
  static_assert(L == CT || L == F32, "epochs are channel-major");
  extern __shared__ v4i smem_v[];
  int8_t* smem = (int8_t*)smem_v;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // the float32 carve for both layouts: the transpose staging, no staged trial
  const Carve cv = carve_of(gp->C, gp->T, gp->N, gp->T8, gp->T64A, gp->NB1, gp->MT, gp->NTT, F32);
  L1C k1;
  L2C k2;
  setup(gp, smem, cv, k1, k2, tid, wave, lane);
  k1.wf = gp->l1_bn[lane];  // channel-major fragments keep the natural K order
  const SmallG* sg = (const SmallG*)(smem + cv.sg);
  int8_t* y1 = smem;
  int8_t* y2 = smem + cv.y2;
  int8_t* y3 = smem + cv.y3;
  int8_t* y4 = smem + cv.y4;
  int8_t* stg = smem + cv.stg + 1024 * wave;
  const bool two_wg = cv.bytes <= LDS_2WG;  // layer-1 groups of two blocks (gen::k_forward)
  const int N = gp->N, NB1 = gp->NB1, K7 = gp->K7;
  // rows past C re-read row C - 1 (their K-slots meet zero weights); below 2^31 by the host's limit
  const unsigned rowoff =
      (unsigned)((L == F32 ? 4ull : 1ull) * (unsigned long long)tab.c[min(lane, gp->C - 1)] * row_stride);
  __syncthreads();
  // (phase stamps as gen::k_forward: 0 layer 1 / the last wave's layers 4-5, 1 barrier A,
  // 2 layer 2, 3 layer 3, 4 barrier B, 7 loop top)
  MIB_STAMP_INIT
  // the previous epoch and whether its onset was valid, in one register: e valid, -2 - e invalid, -1 none
  int eprev = -1;
  for (int e = blockIdx.x;; e += gridDim.x) {
    const bool more = e < E;  // uniform over the workgroup
    MIB_STAMP(7)
    const long long on = more ? onsets[e] : 0;
    const bool valid = (unsigned long long)on <= (unsigned long long)last;  // last >= 0: negative onsets fail too
    const View v = epoch_view<L>(x, valid ? on : 0, span_bytes);  // (the pass past the last epoch loads nothing)
    if (wave < NW - 1) {
      if (more) {
        __builtin_amdgcn_s_setprio(wg::PRIO_L1);
        if (two_wg) layer1_ep<L, XR, CB, false>(gp, v, rowoff, y1, cv.y1s, stg, k1, wave, NW - 1, NB1 - K7, lane, qs, qy);
        else layer1_ep<L, XR, CB, true>(gp, v, rowoff, y1, cv.y1s, stg, k1, wave, NW - 1, NB1 - K7, lane, qs, qy);
      }
    } else {
      if (eprev != -1) {
        const bool vprev = eprev >= 0;
        int8_t* o = out + (size_t)(vprev ? eprev : -2 - eprev) * N;
        if (vprev) {
          __builtin_amdgcn_s_setprio(wg::PRIO_L45);
          layer4<RB, XR, CB>(gp, y3, y4, sg, lane, 0, 1);
          wg::wave_sync_lds();
          layer5<CB>(gp, y4, smem + cv.w5, o, 0, 1, lane);
        } else {
          if (lane < N) o[lane] = 0;
          if (lane == 0 && n_bad) atomicAdd(n_bad, 1);
        }
      }
      // then the epoch's last K7 layer-1 blocks (host-balanced against layers 4-5)
      if (more && K7 > 0) {
        __builtin_amdgcn_s_setprio(wg::PRIO_L1);
        if (two_wg) layer1_ep<L, XR, CB, false>(gp, v, rowoff, y1, cv.y1s, stg, k1, NB1 - K7, 1, NB1, lane, qs, qy);
        else layer1_ep<L, XR, CB, true>(gp, v, rowoff, y1, cv.y1s, stg, k1, NB1 - K7, 1, NB1, lane, qs, qy);
      }
    }
    __builtin_amdgcn_s_setprio(0);
    MIB_STAMP(0)
    if (!more) break;
    __syncthreads();  // A: layer 2 reads every wave's layer-1 rows
    MIB_STAMP(1)
    layer2<RB, XR, CB>(gp, y1, cv.y1s, y2, cv.y2s, k2, wave, lane);
    wg::wave_sync_lds();  // layer 3 of filter f reads only y2 row f, written by this wave
    MIB_STAMP(2)
    __builtin_amdgcn_s_setprio(wg::PRIO_L3);
    layer3<XR, CB>(gp, sg, y2, cv.y2s, y3, wave, lane);
    __builtin_amdgcn_s_setprio(0);
    MIB_STAMP(3)
    __syncthreads();  // B: layer 4 reads every filter's layer-3 rows
    MIB_STAMP(4)
    eprev = valid ? e : -2 - e;
  }
  MIB_STAMP_FLUSH(lane == 0, wave)
}

}  // namespace ep
}  // namespace mib
