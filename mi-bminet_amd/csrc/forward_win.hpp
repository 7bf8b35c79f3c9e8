// forward_win.hpp — sliding-window classification of a continuous recording (gfx950):
// logits of every window w = samples w hop .. w hop + T - 1 of a C x L recording
// (net_model_compute_windows, include/mibminet.h).
//
// Layer 1 is pointwise in time: y1[f][t] depends on x[:, t] alone (layer1.c:53-101), and so does
// the float input quantiser.  Window-dependent arithmetic starts at layer 2 (the xcorr's zero pad
// and the pool-8 phase).  So layer 1 runs once per sample of the recording, not once per window:
//   k_layer1_rec   layer 1 over the recording in 16-sample blocks -> workspace [16][row_stride]
//                  int8 (row f = filter f, byte t = sample t; bytes L .. 16 ceil(L / 16) - 1 zero)
//   k_forward_y1   gen::item_loop (layers 2-5, the persistent loop and its two barriers) over the
//                  windows at samples w hop: in place of layer 1, a copy of the window's sixteen
//                  workspace rows (T bytes each) into the LDS y1 rows;
//   k_forward_y1_at  the same body with each window's first sample read from a device list and
//                  range-checked (net_model_compute_windows_at): irregular and overlapping
//                  windows, and the windows of many recordings laid end to end.
// The same windows with the network chosen per recording (net_model_compute_windows_bank) are
// forward_bank.hpp's kernels, on Rows in its bank form below.
// All read a gen::GenParams image (every geometry, the compiled ones included) and are built
// from the run-time-dimension family (forward_gen.hpp); the compiled wg:: kernels are untouched.
#pragma once
#include "forward_gen.hpp"

namespace mib {
namespace win {

constexpr int NW1 = 4;          // waves per workgroup of k_layer1_rec, one 16-sample block each per step
constexpr int NT1 = 64 * NW1;

// Layer 1 of recording blocks blk = 16 samples (gen::l1_fetch with the recording length Lr as the
// row stride of the channel-major layouts, gen::l1_block), one wave per block, grid-strided.
// x: the recording in layout L (gen::Layout: [Lr][C] int8, [C][Lr] int8, [C][Lr] float32, [Lr][C]
// float32), any byte alignment (float32: 4); the view's bound keeps every load inside the recording (a partial
// last block reads zeros or the next row, and its samples >= Lr are stored as zeros inside the
// row stride).  ws: [F1][rs], rs >= 16 ceil(Lr / 16).
template <int L, bool XR, bool CB>
__global__ __launch_bounds__(NT1) void k_layer1_rec(const gen::GenParams* __restrict__ gp,
                                                    const int8_t* __restrict__ x, int8_t* __restrict__ ws, int Lr,
                                                    int rs, float qs, float qy) {
  __shared__ v4i stg_v[NW1 * 64];  // channel-major transpose staging, 1 KB per wave
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int8_t* stg = (int8_t*)stg_v + 1024 * wave;
  const int C = gp->C;
  const gen::L1C k = gen::l1_consts<L>(gp, lane);
  // the whole recording as one "trial"
  const gen::View v = gen::make_view(x, gen::elem_bytes(L) * (unsigned)C * (unsigned)Lr);
  const int NB = (Lr + 15) / 16;
  int8_t* row = ws + (size_t)(lane & 15) * (size_t)rs;
  for (int blk = (int)blockIdx.x * NW1 + wave; blk < NB; blk += (int)gridDim.x * NW1)  // wave-uniform
    gen::l1_block<L, XR, CB>(gen::l1_fetch<L>(v, blk, C, Lr, lane, qs, qy), stg, k, blk, blk == NB - 1, Lr, row, lane >> 4, lane);
}

// The view of the sixteen workspace rows of the window at sample on: base = ws + on rounded down
// to a dword, delta = the rest (the same for every row: ws is 16-byte aligned and rs a multiple of
// 16), row f at byte f rs.  num_records ends with the dword holding row 15's last window byte,
// which lies inside the workspace (on + T <= L <= rs): (delta + 15 rs + T + 3) & ~3 =
// 15 rs + ((delta + T + 3) & ~3), rs being a multiple of 16.  Offsets stay below 2^31 (16 rs <= 2^31, the host's limit).
__device__ __forceinline__ gen::View window_view(const int8_t* ws, long long on, int T, int rs) {
  return gen::make_view(ws + on, 15u * (unsigned)rs + (unsigned)T);
}

// Copies window rows into the LDS y1 rows (position 32 + t), as layer 1 leaves them: row f's T
// bytes, zeros from T to 16 NB1.  16-byte chunk i < 16 NB1 is chunk k = i mod NB1 of row
// f = i / NB1 (consecutive lanes read consecutive chunks of a row); the source has any byte
// alignment (hop is arbitrary): gen::load16u's aligned dwords + v_alignbyte.  Threads t of nt,
// four chunks' loads issued before their LDS stores.
__device__ __forceinline__ void copy_rows(const gen::View& v, int8_t* y1, int y1s, int T, int NB1, int rs, int t,
                                          int nt) {
  const int total = 16 * NB1;
  const float inv = 1.0f / (float)NB1;  // i / NB1 = floor((i + 1/2) inv) for i < 4096, NB1 <= 256
  constexpr int U = 4;
  for (int i0 = t; i0 < total; i0 += U * nt) {
    v4i d[U];
    int dst[U], rem[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int i = min(i0 + u * nt, total - 1);  // slots past the end re-read the last chunk
      const int f = (int)(((float)i + 0.5f) * inv), k = i - f * NB1;
      d[u] = gen::load16u(v.r, v.delta + f * rs + 16 * k);
      dst[u] = f * y1s + 32 + 16 * k;
      rem[u] = T - 16 * k;  // the row's bytes from this chunk on
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      if (i0 + u * nt < total) {
        v4i q = d[u];
        if (rem[u] < 16) {  // the row's last chunk: bytes >= T are zero (the xcorr's pad)
#pragma unroll
          for (int m = 0; m < 4; m++) {
            const int n = rem[u] - 4 * m;  // bytes of dword m inside the row
            q[m] = n >= 4 ? q[m] : n <= 0 ? 0 : q[m] & (int)((1u << (8 * n)) - 1u);
          }
        }
        *(v4i*)(y1 + dst[u]) = q;
      }
    }
  }
}

// Where gen::item_loop finds window w: the workspace rows ([F1][rs]) from sample w hop, or, AT,
// from the caller-given sample onsets[w] (net_model_compute_windows_at; any order, duplicates
// allowed).  last = Lr - T, the largest valid onset.  A regular window is always valid; an onset
// outside [0, last] forms no address and its rows are not copied.  Waves 0 .. NW-2 copy the rows;
// the last wave only finishes the previous window.  HT: T is held across the loop; else it is one
// scalar load per window.  The plain-BN float builds read it (held, they spilled 13 more scalar
// registers and ran 1-2 % slower), the others hold it (reading cost them 0.7 %).
// BK (with AT): the windows of many recordings, each under its own set of a bank
// (net_model_compute_windows_bank).  blk_set[b] is the set of samples 16 b .. 16 b + 15, the list
// layer 1 ran by (bank::k_layer1_rec_bank).  A window is valid when its onset is in range, the set
// s of its first block lies in 0 .. n_sets - 1 and its last block has the same entry; the two
// entries are read only after the range check (both blocks then lie inside the list), and s
// travels in the item.  gp is then the current set's, changed by the bank loop.
template <bool AT, bool HT, bool BK = false>
struct Rows {
  static_assert(AT || !BK, "a bank's windows come from an onset list");
  static constexpr bool ONSETS = AT;
  const int8_t* ws;
  const long long* onsets;
  long long last;
  const gen::GenParams* gp;
  int hop, rs, T, NB1, y1s, tid;
  int8_t* y1;
  const int* blk_set = nullptr;  // BK
  int n_sets = 0;
  struct Item {
    long long on;  // the window's first sample
    bool valid;
    int s;         // BK: the window's set, meaningful if valid
  };
  __device__ __forceinline__ Item open(int w, bool more) const {
    if constexpr (!AT) return Item{(long long)w * hop, true, 0};
    const long long on = more ? onsets[w] : 0;  // (wave-uniform: one scalar load)
    const bool in = (unsigned long long)on <= (unsigned long long)last;  // last >= 0: negative onsets fail too
    if constexpr (!BK) return Item{on, in, 0};
    int s = 0;
    bool valid = false;
    if (more && in) {  // (wave-uniform: two scalar loads)
      s = blk_set[on >> 4];
      const int e = blk_set[(on + (HT ? T : gp->T) - 1) >> 4];
      valid = (unsigned)s < (unsigned)n_sets && e == s;
    }
    return Item{on, valid, s};
  }
  __device__ __forceinline__ void rows(const Item& it) const {
    const int t = HT ? T : gp->T;
    if (it.valid) copy_rows(window_view(ws, it.on, t, rs), y1, y1s, t, NB1, rs, tid, gen::NT - 64);
  }
  __device__ __forceinline__ void rows_last(const Item&) const {}
  // BK, for bank::set_loop: an invalid window is finished as zeros, and the source holds nothing of a set
  static constexpr bool SKIP = false;
  __device__ __forceinline__ void on_switch(int, int) const {}
};

// Fused forward over W windows of a recording whose layer-1 output is in ws, logits [W][N]:
// gen::item_loop over Rows<AT, HT>.
template <bool RB, bool XR, bool CB, bool AT>
__device__ __forceinline__ void forward_y1(const gen::GenParams* __restrict__ gp, const int8_t* __restrict__ ws,
                                           const long long* __restrict__ onsets, int8_t* __restrict__ out,
                                           int* __restrict__ n_bad, int W, long long last, int hop, int rs) {
  using namespace gen;
  extern __shared__ v4i smem_v[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const Lds m = lds_of(gp, (int8_t*)smem_v, 3);
  L2C k2;
  setup(gp, m, k2, tid, wave, lane);
  const Rows<AT, RB || XR> src{ws, onsets, last, gp, hop, rs, gp->T, gp->NB1, m.cv.y1s, tid, m.y1};
  __syncthreads();
  item_loop<RB, XR, CB>(gp, m, k2, src, out, n_bad, W, wave, lane);
}

// The windows at samples w hop (net_model_compute_windows).
template <bool RB, bool XR, bool CB>
__global__ __launch_bounds__(gen::NT) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_forward_y1(
    const gen::GenParams* __restrict__ gp, const int8_t* __restrict__ ws, int8_t* __restrict__ out, int W, int hop,
    int rs) {
  forward_y1<RB, XR, CB, false>(gp, ws, nullptr, out, nullptr, W, 0, hop, rs);
}

// The windows at the onsets of a device list (net_model_compute_windows_at).
template <bool RB, bool XR, bool CB>
__global__ __launch_bounds__(gen::NT) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_forward_y1_at(
    const gen::GenParams* __restrict__ gp, const int8_t* __restrict__ ws, const long long* __restrict__ onsets,
    int8_t* __restrict__ out, int* __restrict__ n_bad, int W, long long last, int rs) {
  forward_y1<RB, XR, CB, true>(gp, ws, onsets, out, n_bad, W, last, 1, rs);
}

}  // namespace win
}  // namespace mib
