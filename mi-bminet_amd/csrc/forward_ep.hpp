// forward_ep.hpp — epochs cut out of a wider array (gfx950): channel selection, cropping and
// event-locked epochs straight from the source, with no gathered [E][C][T] copy
// (net_model_compute_epochs, include/mibminet.h).
//
// Epoch e, network channel c, sample t is element onsets[e] + channels[c] row_stride + t of the
// flat source.  In the channel-major layer 1 lane c already forms its own row address
// (gen::l1_fetch<CT>: min(lane, C - 1) T + 16 blk); here the row part comes from a per-lane table
// entry and the base from the epoch's onset:
//   per epoch  (wave-uniform) the onset is loaded and range-checked, and the epoch's span becomes
//              one buffer view (gen::make_view);
//   per lane   (once per kernel) rowoff = elem_size channels[min(lane, C - 1)] row_stride;
//   per block  one unaligned 16-byte fetch at delta + rowoff + 16 blk (gen::load16u; float32: four
//              16-byte loads and the input quantiser, gen::load16f).
// Layers 2-5, the persistent loop and its two barriers are gen::'s own (gen::item_loop, which the
// window kernels run too), on a gen::GenParams image (every geometry, the compiled ones included:
// the image the window kernels use).
#pragma once
#include "entry_host.hpp"  // ep::ChanTab
#include "forward_gen.hpp"

namespace mib {
namespace ep {

// The view of the epoch at element onset `on` (valid: 0 <= on <= n_elems - span).  The span lies
// inside the source, so no load through the view leaves it by more than the dword rounding.
template <int L>
__device__ __forceinline__ gen::View epoch_view(const int8_t* x, long long on, unsigned span_bytes) {
  return gen::make_view(x + (L == gen::F32 ? 4 : 1) * on, span_bytes);
}

// The lane's 16 samples of block blk (from its row's byte offset rowoff inside the view), offsets
// unsigned: elem_size span + 6 < 2^31 (the host's limit) keeps every in-range offset below 2^31,
// and the partial last block's reads past the span (zeros: past num_records) stay defined.
template <int L>
__device__ __forceinline__ v4i ep_fetch(const gen::View& v, unsigned rowoff, int blk, float qs, float qy) {
  if constexpr (L == gen::CT) return gen::load16u(v.r, (unsigned)v.delta + rowoff + 16u * (unsigned)blk);
  else return gen::load16f(v.r, rowoff + 64u * (unsigned)blk, qs, qy);
}

// Layer 1 with ep_fetch: blocks first, first + nw, ... < end -> y1 rows (position 32 + t), the U
// blocks' loads issued before their MFMAs (the group loop is this kernel's own, the block is
// gen::l1_block: DESIGN.md §3, "One layer-1 block").  A partial last block reads whatever
// follows the epoch in its row (zeros past the view's end); its samples >= T are stored as zeros,
// so nothing read there (a non-finite float included) reaches a stored sample.
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
      const int blk = b0 + u * nw;  // (the test is wave-uniform)
      if (blk < end) gen::l1_block<L, XR, CB>(raw[u], stg, k, blk, blk == NB1 - 1, T, y1 + j * y1s + 32, g, lane);
    }
  }
}

// Where gen::item_loop finds epoch e: the view at onsets[e], range-checked.  last = n_elems -
// span, the largest valid onset; span_bytes = elem_size span.  An onset outside [0, last] forms no
// address: its epoch is read at onset 0 and discarded.  Waves 0 .. NW-2 run layer 1 of all but the
// epoch's last K7 blocks, which the last wave runs after finishing the previous epoch
// (host-balanced against layers 4-5), in groups of two blocks when two workgroups share the CU,
// else of four (gen::k_forward).
template <int L, bool XR, bool CB>
struct Epochs {
  static constexpr bool ONSETS = true;
  const gen::GenParams* gp;
  const int8_t* x;
  const long long* onsets;
  long long last;
  unsigned span_bytes, rowoff;
  int8_t *y1, *stg;
  int y1s, NB1, K7, wave, lane;
  bool two_wg;
  gen::L1C k1;
  float qs, qy;
  struct Item {
    gen::View v;
    bool valid;
  };
  __device__ __forceinline__ Item open(int e, bool more) const {
    const long long on = more ? onsets[e] : 0;  // (wave-uniform: one scalar load)
    const bool valid = (unsigned long long)on <= (unsigned long long)last;  // last >= 0: negative onsets fail too
    return Item{epoch_view<L>(x, valid ? on : 0, span_bytes), valid};
  }
  // (layer 1 ahead of the other workgroup's layers 2-3, as gen::k_forward; the priority it raises it resets)
  __device__ __forceinline__ void l1(const gen::View& v, int first, int nw, int end) const {
    __builtin_amdgcn_s_setprio(wg::PRIO_L1);
    if (two_wg) layer1_ep<L, XR, CB, false>(gp, v, rowoff, y1, y1s, stg, k1, first, nw, end, lane, qs, qy);
    else layer1_ep<L, XR, CB, true>(gp, v, rowoff, y1, y1s, stg, k1, first, nw, end, lane, qs, qy);
    __builtin_amdgcn_s_setprio(0);
  }
  __device__ __forceinline__ void rows(const Item& it) const { l1(it.v, wave, gen::NW - 1, NB1 - K7); }
  __device__ __forceinline__ void rows_last(const Item& it) const {
    if (K7 > 0) l1(it.v, NB1 - K7, 1, NB1);
  }
};

// Fused forward over E epochs of the source x (layout L: CT int8, F32 float32), logits [E][N]:
// gen::item_loop over Epochs<L>.
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
  const Lds m = lds_of(gp, smem, F32);
  L2C k2;
  setup(gp, m, k2, tid, wave, lane);
  // rows past C re-read row C - 1 (their K-slots meet zero weights); below 2^31 by the host's limit
  const unsigned rowoff =
      (unsigned)((L == F32 ? 4ull : 1ull) * (unsigned long long)tab.c[min(lane, gp->C - 1)] * row_stride);
  const Epochs<L, XR, CB> src{gp, x, onsets, last, span_bytes, rowoff, m.y1, smem + m.cv.stg + 1024 * wave, m.cv.y1s,
                              gp->NB1, gp->K7, wave, lane, m.cv.bytes <= LDS_2WG, l1_consts<L>(gp, lane), qs, qy};
  __syncthreads();
  item_loop<RB, XR, CB>(gp, m, k2, src, out, n_bad, E, wave, lane);
}

}  // namespace ep
}  // namespace mib
