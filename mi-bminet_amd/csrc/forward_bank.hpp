// forward_bank.hpp — epochs classified by many resident networks in one launch (gfx950):
// net_model_compute_epochs_bank[_f32] and, with the layer-4 activations beside the logits,
// net_model_compute_epochs_bank_feat[_f32], include/mibminet.h.  A bank is an array of gen::GenParams
// images of one geometry; epoch e is classified by image set_of[e].
//
// The fetch is ep::Epochs and the layers are gen::'s, as in ep::k_forward_ep.  The persistent loop
// is this file's own, because it carries a current set: bank::set_loop, the one loop of the three
// kernels here and of the four of forward_stream.hpp, each of which is its prologue, its source and
// one call ("One set-switching loop").  What belongs to a set and changes together at
// a switch:
//   the wave's layer-2 fragments and constants   (gen::L2C, registers: gen::set_l2c)
//   the lane's layer-1 constants                 (gen::L1C, registers: gen::l1_consts)
//   the LDS copies of SmallG, the layer-5 rows and biases          (gen::set_lds)
//   the GenParams pointer layers 1, 3 and 5 read through, and for float input qs and qy.
// The zero pads and the carve depend on the geometry alone: written once, left alone by a switch.
//
// The hazard: the loop overlaps item i's layer 1 (waves 0 .. NW-2) with the last wave's layers 4-5
// of item i - 1, which read SmallG::l4_*, the layer-5 rows and gp->l5_*.  At a switch item i - 1
// therefore finishes first, on its own set: the last wave runs its layers 4-5, a barrier, every
// wave reloads, a barrier, and item i starts with no previous item pending.  Two barriers more per
// switch, none otherwise.
//
// Schedule: workgroup w of G takes the contiguous items bank::range_of(w, G, E), not the grid
// stride, so that on a list grouped by set it switches once per set its range touches; the first
// item of a range is a switch from no set.  An invalid item (its onset or its set index out of
// range) forms no address from either, keeps the current set and costs no switch; its layers 2-3
// run on whatever the rows hold and are dropped, as in gen::item_loop.  The first item of a range,
// if invalid, loads set 0.
//
// The windows of many recordings, each under its own set (net_model_compute_windows_bank), follow:
// layer 1 per sample with a current set per wave (k_layer1_rec_bank), then set_loop over win::Rows.
#pragma once
#include "bank_host.hpp"
#include "forward_ep.hpp"
#include "forward_win.hpp"
#include "image_layout.hpp"  // bank::Scale

namespace mib {
namespace bank {

// The persistent loop of every kernel that carries a current set: the three below and the four of
// forward_stream.hpp.  Workgroup w of G takes the contiguous items range_of(w, G, n).  The source S
// (BankEpochs, win::Rows<true, HT, true>, stream::RingRows, EachRows, AtRows) provides
//   open(i, more)      the item: .valid and, if valid, its set .s (wave-uniform scalar loads; no
//                      address is formed from an index that failed its unsigned range check)
//   rows(it)           waves 0 .. NW-2: the item's layer-1 rows into y1
//   rows_last(it)      the last wave's share of them, after it finished item i - 1
//   on_switch(cur, t)  what the source itself holds of a set (t: the opaque thread index)
//   gp                 the current set's image, changed here
//   SKIP               an item that is not valid is absent, not invalid: the loop passes over it
//                      before any barrier (open() is uniform over the workgroup) and leaves `prev`
//                      as it is, so the last item that did exist is still finished, on its own
//                      set, at the next switch or on the pass past the last item.
// FEAT: each item's layer-4 activations go to feat [n][16][T64] beside the logits
// (gen::finish_prev_feat), an invalid item's as zeros; feat is touched under FEAT alone.
// n_bad counts the invalid items, or is null.
// (phase stamps in tools/ builds with -DMIB_STAMPS, as gen::item_loop, and 5: a switch)
template <bool RB, bool XR, bool CB, bool FEAT, class S>
__device__ __forceinline__ void set_loop(const gen::GenParams* __restrict__ sets, const gen::Lds& m, S& src,
                                         int8_t* __restrict__ out, int8_t* __restrict__ feat,
                                         int* __restrict__ n_bad, int n, int tid, int wave, int lane) {
  using namespace gen;
  const int N = sets->N;  // the geometry is every set's
  // (T64 is one scalar load where a feature row is stored: held across the loop it cost the _feat
  // builds 20-30 more spilled scalar registers)
  const auto finish = [&](const GenParams* __restrict__ gp, int prev) {
    if constexpr (FEAT) finish_prev_feat<RB, XR, CB>(gp, m, out, feat, n_bad, prev, N, sets->T64, lane);
    else finish_prev<RB, XR, CB, true>(gp, m, out, n_bad, prev, N, lane);
  };
  L2C k2;
  const Range64 rg = range_of(blockIdx.x, gridDim.x, (unsigned long long)n);
  const int end = (int)rg.hi;
  MIB_STAMP_INIT
  int cur = -1;   // the set in registers and LDS
  int prev = -1;  // gen::item_loop's: i valid, -2 - i invalid, -1 none
  for (int i = (int)rg.lo;; i++) {
    const bool more = i < end;  // uniform over the workgroup
    MIB_STAMP(7)
    const auto it = src.open(i, more);
    if constexpr (S::SKIP) {
      if (more && !it.valid) continue;
    }
    const int need = it.valid ? it.s : max(cur, 0);  // an invalid item stays where the workgroup is
    if (more && need != cur) {
      // item i - 1 ends on its own set before any of that set's state goes
      if (wave == NW - 1) finish(src.gp, prev);
      prev = -1;
      __syncthreads();
      cur = need;
      src.gp = sets + cur;
      // the reload's addresses are derived here, per switch (gen::layer4's device): hoisted out of
      // the loop they were held in registers across every layer, and spilled in the plain float
      // builds
      int t;
      asm volatile("v_mov_b32 %0, %1" : "=v"(t) : "v"(tid));
      src.on_switch(cur, t);
      set_l2c(src.gp, k2, wave, t & 63);
      set_lds(src.gp, m, t);
      __syncthreads();
      MIB_STAMP(5)
    }
    const GenParams* __restrict__ gp = src.gp;
    if (wave < NW - 1) {
      if (more) src.rows(it);
    } else {
      finish(gp, prev);
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
    prev = it.valid ? i : -2 - i;
  }
  MIB_STAMP_FLUSH(lane == 0, wave)
}

// A kernel's prologue before set_loop: the carve (the geometry is every set's, so set 0 stands for
// it until the first switch) and the zero pads (gen::setup), which the first switch's barriers
// publish.
__device__ __forceinline__ gen::Lds carve_and_pads(const gen::GenParams* __restrict__ sets, int8_t* smem, int layout,
                                                   int tid) {
  const gen::Lds m = gen::lds_of(sets, smem, layout);
  v4i* z = (v4i*)m.y1;
  for (int i = tid; i < m.cv.sg / 16; i += gen::NT) z[i] = (v4i){0, 0, 0, 0};
  return m;
}

// ep::Epochs in its bank form: epoch e's set is set_of[e] (null: set 0), compared unsigned with
// n_sets before any address is formed from it and folded into .valid; a switch reloads the lane's
// layer-1 constants and, for float input, the set's scales (scales: n_sets entries, else null).
template <int L, bool XR, bool CB>
struct BankEpochs : ep::Epochs<L, XR, CB> {
  static constexpr bool SKIP = false;
  const int* set_of;
  int n_sets;
  const Scale* scales;
  struct Item {
    gen::View v;
    bool valid;
    int s;
  };
  __device__ __forceinline__ Item open(int e, bool more) const {
    const auto it = ep::Epochs<L, XR, CB>::open(e, more);
    const int s = more && set_of ? set_of[e] : 0;  // (wave-uniform: one scalar load)
    return Item{it.v, it.valid && (unsigned)s < (unsigned)n_sets, s};
  }
  __device__ __forceinline__ void rows(const Item& it) const { this->l1(it.v, this->wave, gen::NW - 1, this->NB1 - this->K7); }
  __device__ __forceinline__ void rows_last(const Item& it) const {
    if (this->K7 > 0) this->l1(it.v, this->NB1 - this->K7, 1, this->NB1);
  }
  __device__ __forceinline__ void on_switch(int cur, int t) {
    this->k1 = gen::l1_consts<L>(this->gp, t & 63);
    if constexpr (L == gen::F32) {
      const Scale q = scales[cur];
      this->qs = q.qs;
      this->qy = q.qy;
    }
  }
};

// The body of k_forward_ep_bank and k_forward_ep_bank_feat.
template <int L, bool RB, bool XR, bool CB, bool FEAT>
__device__ __forceinline__ void forward_ep_bank(const gen::GenParams* __restrict__ sets, int n_sets,
                                                const int* __restrict__ set_of, const Scale* __restrict__ scales,
                                                const int8_t* __restrict__ x, const long long* __restrict__ onsets,
                                                int8_t* __restrict__ out, int8_t* __restrict__ feat,
                                                int* __restrict__ n_bad, int E, long long last, unsigned span_bytes,
                                                unsigned long long row_stride, const ep::ChanTab& tab) {
  using namespace gen;
  static_assert(L == CT || L == F32, "epochs are channel-major");
  extern __shared__ v4i smem_v[];
  int8_t* smem = (int8_t*)smem_v;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const Lds m = carve_and_pads(sets, smem, F32, tid);
  const unsigned rowoff =
      (unsigned)((L == F32 ? 4ull : 1ull) * (unsigned long long)tab.c[min(lane, sets->C - 1)] * row_stride);
  BankEpochs<L, XR, CB> src{{sets, x, onsets, last, span_bytes, rowoff, m.y1, smem + m.cv.stg + 1024 * wave, m.cv.y1s,
                             sets->NB1, sets->K7, wave, lane, m.cv.bytes <= LDS_2WG, L1C{}, 0.0f, 0.0f},
                            set_of, n_sets, scales};
  set_loop<RB, XR, CB, FEAT>(sets, m, src, out, feat, n_bad, E, tid, wave, lane);
}

// Fused forward over E epochs of the source x (layout L: CT int8, F32 float32), logits [E][N].
// sets: n_sets images of one geometry and one (RB, XR, CB); set_of: E set indices, or null (set 0);
// scales: n_sets entries (F32), else null.  The other arguments are ep::k_forward_ep's.
template <int L, bool RB, bool XR, bool CB>
__global__ __launch_bounds__(gen::NT) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_forward_ep_bank(
    const gen::GenParams* __restrict__ sets, int n_sets, const int* __restrict__ set_of,
    const Scale* __restrict__ scales, const int8_t* __restrict__ x, const long long* __restrict__ onsets,
    int8_t* __restrict__ out, int* __restrict__ n_bad, int E, long long last, unsigned span_bytes,
    unsigned long long row_stride, const ep::ChanTab tab) {
  forward_ep_bank<L, RB, XR, CB, false>(sets, n_sets, set_of, scales, x, onsets, out, nullptr, n_bad, E, last,
                                        span_bytes, row_stride, tab);
}

// k_forward_ep_bank with the layer-4 activations beside the logits
// (net_model_compute_epochs_bank_feat[_f32]): feat [E][16][T64] int8, 16-byte aligned.  The logits
// are that kernel's logits and an invalid item's feature row is zeros.
template <int L, bool RB, bool XR, bool CB>
__global__ __launch_bounds__(gen::NT) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_forward_ep_bank_feat(
    const gen::GenParams* __restrict__ sets, int n_sets, const int* __restrict__ set_of,
    const Scale* __restrict__ scales, const int8_t* __restrict__ x, const long long* __restrict__ onsets,
    int8_t* __restrict__ out, int8_t* __restrict__ feat, int* __restrict__ n_bad, int E, long long last,
    unsigned span_bytes, unsigned long long row_stride, const ep::ChanTab tab) {
  forward_ep_bank<L, RB, XR, CB, true>(sets, n_sets, set_of, scales, x, onsets, out, feat, n_bad, E, last, span_bytes,
                                       row_stride, tab);
}

// ---- windows through a bank (net_model_compute_windows_bank, include/mibminet.h) -------------
// R recordings lie along time in one array, each starting at a multiple of 16 samples, and
// blk_set[b] names the set of samples 16 b .. 16 b + 15.  Layer 1 and the float quantiser see one
// sample at a time, so ws[f][t] depends on sample t and on that sample's set alone: layer 1 still
// runs once per sample (k_layer1_rec_bank), and each window's layers 2-5 run under the set of its
// blocks, switching as k_forward_ep_bank does (k_forward_y1_bank).

// win::k_layer1_rec with a current set per wave.  Wave g of gridDim.x NW1 takes the contiguous
// blocks range_of(g, gridDim.x NW1, NB), so it reloads at most once per run of equal entries in
// its range.  Per block one scalar load of blk_set[blk]; the index is compared unsigned before any
// address is formed from it.  An entry outside 0 .. n_sets - 1 (-1: a gap) stores the block's 16
// bytes of all sixteen rows as zeros, one dword per lane, and keeps the current set.  scales: F32.
template <int L, bool XR, bool CB>
__global__ __launch_bounds__(win::NT1) void k_layer1_rec_bank(const gen::GenParams* __restrict__ sets, int n_sets,
                                                              const int* __restrict__ blk_set,
                                                              const Scale* __restrict__ scales,
                                                              const int8_t* __restrict__ x, int8_t* __restrict__ ws,
                                                              int Lr, int rs) {
  __shared__ v4i stg_v[win::NW1 * 64];  // channel-major transpose staging, 1 KB per wave
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int8_t* stg = (int8_t*)stg_v + 1024 * wave;
  const int C = sets->C;  // every set's
  const gen::View v = gen::make_view(x, gen::elem_bytes(L) * (unsigned)C * (unsigned)Lr);
  const int NB = (Lr + 15) / 16;
  int8_t* row = ws + (size_t)(lane & 15) * (size_t)rs;
  const Range64 rg = range_of(blockIdx.x * win::NW1 + (unsigned)wave, gridDim.x * win::NW1, (unsigned long long)NB);
  const int end = (int)rg.hi;
  gen::L1C k{};
  float qs = 0.0f, qy = 0.0f;
  int cur = -1;
  for (int blk = (int)rg.lo; blk < end; blk++) {  // wave-uniform
    const int s = blk_set[blk];
    if ((unsigned)s >= (unsigned)n_sets) {
      *(unsigned*)(row + 16 * blk + 4 * (lane >> 4)) = 0u;  // inside the row stride, as l1_block's store
      continue;
    }
    if (s != cur) {
      cur = s;
      k = gen::l1_consts<L>(sets + s, lane);
      if constexpr (gen::is_float(L)) {
        const Scale q = scales[s];
        qs = q.qs;
        qy = q.qy;
      }
    }
    gen::l1_block<L, XR, CB>(gen::l1_fetch<L>(v, blk, C, Lr, lane, qs, qy), stg, k, blk, blk == NB - 1, Lr, row,
                             lane >> 4, lane);
  }
}

// set_loop over the windows at onsets[i] of the workspace rows (win::Rows in its bank form), logits
// [W][N].  Layer 1 is not here, so the carve is the one without staging and a switch reloads the
// layer-2 constants, the LDS copies and the pointer alone.  last = Lr - T.
template <bool RB, bool XR, bool CB>
__global__ __launch_bounds__(gen::NT) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_forward_y1_bank(
    const gen::GenParams* __restrict__ sets, int n_sets, const int* __restrict__ blk_set,
    const int8_t* __restrict__ ws, const long long* __restrict__ onsets, int8_t* __restrict__ out,
    int* __restrict__ n_bad, int W, long long last, int rs) {
  extern __shared__ v4i smem_v[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const gen::Lds m = carve_and_pads(sets, (int8_t*)smem_v, 3, tid);
  win::Rows<true, RB || XR, true> src{ws,  onsets,   last, sets, 1,       rs,     sets->T,
                                      sets->NB1, m.cv.y1s, tid,  m.y1, blk_set, n_sets};
  set_loop<RB, XR, CB, false>(sets, m, src, out, nullptr, n_bad, W, tid, wave, lane);
}

}  // namespace bank
}  // namespace mib
