// forward_bank.hpp — epochs classified by many resident networks in one launch (gfx950):
// net_model_compute_epochs_bank[_f32] and, with the layer-4 activations beside the logits,
// net_model_compute_epochs_bank_feat[_f32], include/mibminet.h.  A bank is an array of gen::GenParams
// images of one geometry; epoch e is classified by image set_of[e].
//
// The fetch is ep::Epochs and the layers are gen::'s, as in ep::k_forward_ep.  The persistent loop
// is this file's own, because it carries a current set.  What belongs to a set and changes together
// at a switch:
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
// run on whatever the rows hold and are dropped, as in gen::item_loop.
#pragma once
#include "bank_host.hpp"
#include "forward_ep.hpp"
#include "forward_win.hpp"
#include "image_layout.hpp"  // bank::Scale

namespace mib {
namespace bank {

// Fused forward over E epochs of the source x (layout L: CT int8, F32 float32), logits [E][N].
// sets: n_sets images of one geometry and one (RB, XR, CB); set_of: E set indices, or null (set 0);
// scales: n_sets entries (F32), else null.  The other arguments are ep::k_forward_ep's.
// (phase stamps in tools/ builds with -DMIB_STAMPS, as gen::item_loop, and 5: a switch)
template <int L, bool RB, bool XR, bool CB>
__global__ __launch_bounds__(gen::NT) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_forward_ep_bank(
    const gen::GenParams* __restrict__ sets, int n_sets, const int* __restrict__ set_of,
    const Scale* __restrict__ scales, const int8_t* __restrict__ x, const long long* __restrict__ onsets,
    int8_t* __restrict__ out, int* __restrict__ n_bad, int E, long long last, unsigned span_bytes,
    unsigned long long row_stride, const ep::ChanTab tab) {
  using namespace gen;
  static_assert(L == CT || L == F32, "epochs are channel-major");
  extern __shared__ v4i smem_v[];
  int8_t* smem = (int8_t*)smem_v;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // the geometry is every set's: set 0 stands for it until the first switch
  const Lds m = lds_of(sets, smem, F32);
  const int N = sets->N;
  v4i* z = (v4i*)m.y1;  // the zero pads (gen::setup); the first switch's barriers publish them
  for (int i = tid; i < m.cv.sg / 16; i += NT) z[i] = (v4i){0, 0, 0, 0};
  const unsigned rowoff =
      (unsigned)((L == F32 ? 4ull : 1ull) * (unsigned long long)tab.c[min(lane, sets->C - 1)] * row_stride);
  ep::Epochs<L, XR, CB> src{sets, x, onsets, last, span_bytes, rowoff, m.y1, smem + m.cv.stg + 1024 * wave, m.cv.y1s,
                            sets->NB1, sets->K7, wave, lane, m.cv.bytes <= LDS_2WG, L1C{}, 0.0f, 0.0f};
  L2C k2;
  const Range64 rg = range_of(blockIdx.x, gridDim.x, (unsigned long long)E);
  const int end = (int)rg.hi;
  MIB_STAMP_INIT
  int cur = -1;   // the set in registers and LDS
  int prev = -1;  // gen::item_loop's: i valid, -2 - i invalid, -1 none
  for (int i = (int)rg.lo;; i++) {
    const bool more = i < end;  // uniform over the workgroup
    MIB_STAMP(7)
    auto it = src.open(i, more);
    // (wave-uniform: one scalar load)  no address is formed from an index outside the bank
    const int s = more && set_of ? set_of[i] : 0;
    it.valid = it.valid && (unsigned)s < (unsigned)n_sets;
    const int need = it.valid ? s : max(cur, 0);  // an invalid item stays where the workgroup is
    if (more && need != cur) {
      // item i - 1 ends on its own set before any of that set's state goes
      if (wave == NW - 1) finish_prev<RB, XR, CB, true>(src.gp, m, out, n_bad, prev, N, lane);
      prev = -1;
      __syncthreads();
      cur = need;
      src.gp = sets + cur;
      // the reload's addresses are derived here, per switch (gen::layer4's device): hoisted out of
      // the epoch loop they were held in registers across every layer, and spilled in the plain
      // float builds
      int t;
      asm volatile("v_mov_b32 %0, %1" : "=v"(t) : "v"(tid));
      src.k1 = l1_consts<L>(src.gp, t & 63);
      if constexpr (L == F32) {
        const Scale q = scales[cur];
        src.qs = q.qs;
        src.qy = q.qy;
      }
      set_l2c(src.gp, k2, wave, t & 63);
      set_lds(src.gp, m, t);
      __syncthreads();
      MIB_STAMP(5)
    }
    const GenParams* __restrict__ gp = src.gp;
    if (wave < NW - 1) {
      if (more) src.rows(it);
    } else {
      finish_prev<RB, XR, CB, true>(gp, m, out, n_bad, prev, N, lane);
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

// k_forward_ep_bank with the layer-4 activations beside the logits
// (net_model_compute_epochs_bank_feat[_f32]): feat [E][16][T64] int8, 16-byte aligned.  A SIBLING OF
// k_forward_ep_bank, kept in step with it by hand: the same loop with gen::finish_prev_feat where
// that kernel has gen::finish_prev, so the logits are its logits and an invalid item's feature row
// is zeros.  A flag on the shared kernel would rename every existing instantiation (DESIGN.md §3,
// "Features beside the logits").
template <int L, bool RB, bool XR, bool CB>
__global__ __launch_bounds__(gen::NT) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_forward_ep_bank_feat(
    const gen::GenParams* __restrict__ sets, int n_sets, const int* __restrict__ set_of,
    const Scale* __restrict__ scales, const int8_t* __restrict__ x, const long long* __restrict__ onsets,
    int8_t* __restrict__ out, int8_t* __restrict__ feat, int* __restrict__ n_bad, int E, long long last,
    unsigned span_bytes, unsigned long long row_stride, const ep::ChanTab tab) {
  using namespace gen;
  static_assert(L == CT || L == F32, "epochs are channel-major");
  extern __shared__ v4i smem_v[];
  int8_t* smem = (int8_t*)smem_v;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // the geometry is every set's: set 0 stands for it until the first switch
  const Lds m = lds_of(sets, smem, F32);
  const int N = sets->N, T64 = sets->T64;
  v4i* z = (v4i*)m.y1;  // the zero pads (gen::setup); the first switch's barriers publish them
  for (int i = tid; i < m.cv.sg / 16; i += NT) z[i] = (v4i){0, 0, 0, 0};
  const unsigned rowoff =
      (unsigned)((L == F32 ? 4ull : 1ull) * (unsigned long long)tab.c[min(lane, sets->C - 1)] * row_stride);
  ep::Epochs<L, XR, CB> src{sets, x, onsets, last, span_bytes, rowoff, m.y1, smem + m.cv.stg + 1024 * wave, m.cv.y1s,
                            sets->NB1, sets->K7, wave, lane, m.cv.bytes <= LDS_2WG, L1C{}, 0.0f, 0.0f};
  L2C k2;
  const Range64 rg = range_of(blockIdx.x, gridDim.x, (unsigned long long)E);
  const int end = (int)rg.hi;
  int cur = -1;   // the set in registers and LDS
  int prev = -1;  // gen::item_loop's: i valid, -2 - i invalid, -1 none
  for (int i = (int)rg.lo;; i++) {
    const bool more = i < end;  // uniform over the workgroup
    auto it = src.open(i, more);
    // (wave-uniform: one scalar load)  no address is formed from an index outside the bank
    const int s = more && set_of ? set_of[i] : 0;
    it.valid = it.valid && (unsigned)s < (unsigned)n_sets;
    const int need = it.valid ? s : max(cur, 0);  // an invalid item stays where the workgroup is
    if (more && need != cur) {
      // item i - 1 ends on its own set before any of that set's state goes
      if (wave == NW - 1) finish_prev_feat<RB, XR, CB>(src.gp, m, out, feat, n_bad, prev, N, T64, lane);
      prev = -1;
      __syncthreads();
      cur = need;
      src.gp = sets + cur;
      // the reload's addresses are derived here, per switch, from an opaque copy of the thread
      // index (k_forward_ep_bank)
      int t;
      asm volatile("v_mov_b32 %0, %1" : "=v"(t) : "v"(tid));
      src.k1 = l1_consts<L>(src.gp, t & 63);
      if constexpr (L == F32) {
        const Scale q = scales[cur];
        src.qs = q.qs;
        src.qy = q.qy;
      }
      set_l2c(src.gp, k2, wave, t & 63);
      set_lds(src.gp, m, t);
      __syncthreads();
    }
    const GenParams* __restrict__ gp = src.gp;
    if (wave < NW - 1) {
      if (more) src.rows(it);
    } else {
      finish_prev_feat<RB, XR, CB>(gp, m, out, feat, n_bad, prev, N, T64, lane);
      if (more) src.rows_last(it);
    }
    if (!more) break;
    __syncthreads();  // A
    layer2<RB, XR, CB>(gp, m.y1, m.cv.y1s, m.y2, m.cv.y2s, k2, wave, lane);
    wg::wave_sync_lds();  // layer 3 of filter f reads only y2 row f, written by this wave
    __builtin_amdgcn_s_setprio(wg::PRIO_L3);
    layer3<XR, CB>(gp, m.sg, m.y2, m.cv.y2s, m.y3, wave, lane);
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();  // B
    prev = it.valid ? i : -2 - i;
  }
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

// k_forward_ep_bank's loop over the windows at onsets[i] of the workspace rows (win::Rows in its
// bank form), logits [W][N]: the contiguous ranges, item i - 1 finished on its own set before a
// switch with its two barriers, an invalid window keeps the current set, the zero pads written
// once.  Layer 1 is not here, so the carve is the one without staging and a switch reloads the
// layer-2 constants, the LDS copies and the pointer alone.  last = Lr - T.  The loop is a copy, not
// shared with k_forward_ep_bank: shared, that kernel's sixteen builds came out with other opcode
// counts ("Windows through a bank").
template <bool RB, bool XR, bool CB>
__global__ __launch_bounds__(gen::NT) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_forward_y1_bank(
    const gen::GenParams* __restrict__ sets, int n_sets, const int* __restrict__ blk_set,
    const int8_t* __restrict__ ws, const long long* __restrict__ onsets, int8_t* __restrict__ out,
    int* __restrict__ n_bad, int W, long long last, int rs) {
  using namespace gen;
  extern __shared__ v4i smem_v[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // the geometry is every set's: set 0 stands for it until the first switch
  const Lds m = lds_of(sets, (int8_t*)smem_v, 3);
  const int N = sets->N;
  v4i* z = (v4i*)m.y1;  // the zero pads (gen::setup); the first switch's barriers publish them
  for (int i = tid; i < m.cv.sg / 16; i += NT) z[i] = (v4i){0, 0, 0, 0};
  win::Rows<true, RB || XR, true> src{ws,  onsets,   last, sets, 1,       rs,     sets->T,
                                      sets->NB1, m.cv.y1s, tid,  m.y1, blk_set, n_sets};
  L2C k2;
  const Range64 rg = range_of(blockIdx.x, gridDim.x, (unsigned long long)W);
  const int end = (int)rg.hi;
  MIB_STAMP_INIT
  int cur = -1;   // the set in registers and LDS
  int prev = -1;  // gen::item_loop's: i valid, -2 - i invalid, -1 none
  for (int i = (int)rg.lo;; i++) {
    const bool more = i < end;  // uniform over the workgroup
    MIB_STAMP(7)
    // (wave-uniform: three scalar loads)  valid: the onset in range, the set of its first block
    // inside the bank and its last block of the same set; no address is formed from anything else
    const auto it = src.open(i, more);
    const int need = it.valid ? it.s : max(cur, 0);  // an invalid window stays where the workgroup is
    if (more && need != cur) {
      // window i - 1 ends on its own set before any of that set's state goes
      if (wave == NW - 1) finish_prev<RB, XR, CB, true>(src.gp, m, out, n_bad, prev, N, lane);
      prev = -1;
      __syncthreads();
      cur = need;
      src.gp = sets + cur;
      // the reload's addresses are derived here, per switch, from an opaque copy of the thread
      // index (k_forward_ep_bank)
      int t;
      asm volatile("v_mov_b32 %0, %1" : "=v"(t) : "v"(tid));
      set_l2c(src.gp, k2, wave, t & 63);
      set_lds(src.gp, m, t);
      __syncthreads();
      MIB_STAMP(5)
    }
    const GenParams* __restrict__ gp = src.gp;
    if (wave < NW - 1) {
      if (more) src.rows(it);
    } else {
      finish_prev<RB, XR, CB, true>(gp, m, out, n_bad, prev, N, lane);
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

}  // namespace bank
}  // namespace mib
