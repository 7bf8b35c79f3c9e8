// forward_win.hpp — sliding-window classification of a continuous recording (gfx950):
// logits of every window w = samples w hop .. w hop + T - 1 of a C x L recording
// (net_model_compute_windows, include/mibminet.h).
//
// Layer 1 is pointwise in time: y1[f][t] depends on x[:, t] alone (layer1.c:53-101), and so does
// the float input quantiser.  Window-dependent arithmetic starts at layer 2 (the xcorr's zero pad
// and the pool-8 phase).  So layer 1 runs once per sample of the recording, not once per window:
//   k_layer1_rec   layer 1 over the recording in 16-sample blocks -> workspace [16][row_stride]
//                  int8 (row f = filter f, byte t = sample t; bytes L .. 16 ceil(L / 16) - 1 zero)
//   k_forward_y1   gen::k_forward with its layer-1 phase replaced by a copy of the window's
//                  sixteen workspace rows (T bytes each, from byte w hop) into the LDS y1 rows;
//                  layers 2-5, the persistent loop and its two barriers are gen::'s own.
//   k_forward_y1_at  the same with each window's first sample read from a device list and
//                  range-checked (net_model_compute_windows_at): irregular and overlapping
//                  windows, and the windows of many recordings laid end to end.
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
// x: the recording in layout L (gen::Layout: [Lr][C] int8, [C][Lr] int8, [C][Lr] float32), any
// byte alignment (float32: 4); the view's bound keeps every load inside the recording (a partial
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
  const gen::View v = gen::make_view(x, (L == gen::F32 ? 4u : 1u) * (unsigned)C * (unsigned)Lr);
  const int NB = (Lr + 15) / 16;
  int8_t* row = ws + (size_t)(lane & 15) * (size_t)rs;
  for (int blk = (int)blockIdx.x * NW1 + wave; blk < NB; blk += (int)gridDim.x * NW1)  // wave-uniform
    gen::l1_block<L, XR, CB>(gen::l1_fetch<L>(v, blk, C, Lr, lane, qs, qy), stg, k, blk, blk == NB - 1, Lr, row, lane >> 4, lane);
}

// The view of window w's sixteen workspace rows: base = ws + w hop rounded down to a dword, delta
// = the rest (the same for every row: ws is 16-byte aligned and rs a multiple of 16), row f at
// byte f rs.  num_records ends with the dword holding row 15's last window byte, which lies inside
// the workspace (w hop + T <= L <= rs): (delta + 15 rs + T + 3) & ~3 = 15 rs + ((delta + T + 3) & ~3),
// rs being a multiple of 16.  Offsets stay below 2^31 (16 rs <= 2^31, the host's limit).
__device__ __forceinline__ gen::View window_view(const int8_t* ws, long long w, int hop, int T, int rs) {
  return gen::make_view(ws + w * hop, 15u * (unsigned)rs + (unsigned)T);
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

// Fused forward over the W windows of a recording whose layer-1 output is in ws ([F1][rs]),
// logits [W][N].  gen::k_forward's loop: waves 0 .. NW-2 copy window w's rows while the last wave
// runs layers 4-5 of the previous window; barrier A; layers 2-3; barrier B.
template <bool RB, bool XR, bool CB>
__global__ __launch_bounds__(gen::NT) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_forward_y1(
    const gen::GenParams* __restrict__ gp, const int8_t* __restrict__ ws, int8_t* __restrict__ out, int W, int hop,
    int rs) {
  using namespace gen;
  extern __shared__ v4i smem_v[];
  int8_t* smem = (int8_t*)smem_v;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const Lds m = lds_of(gp, smem, 3);
  const Carve& cv = m.cv;
  L2C k2;
  setup(gp, m, k2, tid, wave, lane);
  const int T = gp->T, N = gp->N, NB1 = gp->NB1;
  __syncthreads();
  // (phase stamps as gen::k_forward: 0 the copy / the last wave's layers 4-5, 1 barrier A,
  // 2 layer 2, 3 layer 3, 4 barrier B, 7 loop top)
  MIB_STAMP_INIT
  // one pass more than the workgroup has windows: the last pass only runs the last window's
  // layers 4-5 (one copy of that code in the kernel)
  int wprev = -1;
  for (int w = blockIdx.x;; w += gridDim.x) {
    const bool more = w < W;  // uniform over the workgroup
    MIB_STAMP(7)
    if (wave < NW - 1) {
      if (more) copy_rows(window_view(ws, w, hop, T, rs), m.y1, cv.y1s, T, NB1, rs, tid, NT - 64);
    } else if (wprev >= 0) {
      __builtin_amdgcn_s_setprio(wg::PRIO_L45);
      finish_trial<RB, XR, CB>(gp, m, out + (size_t)wprev * N, lane);
      __builtin_amdgcn_s_setprio(0);
    }
    MIB_STAMP(0)
    if (!more) break;
    __syncthreads();  // A: layer 2 reads every wave's part of the y1 rows
    MIB_STAMP(1)
    layer2<RB, XR, CB>(gp, m.y1, cv.y1s, m.y2, cv.y2s, k2, wave, lane);
    wg::wave_sync_lds();  // layer 3 of filter f reads only y2 row f, written by this wave
    MIB_STAMP(2)
    __builtin_amdgcn_s_setprio(wg::PRIO_L3);
    layer3<XR, CB>(gp, m.sg, m.y2, cv.y2s, m.y3, wave, lane);
    __builtin_amdgcn_s_setprio(0);
    MIB_STAMP(3)
    __syncthreads();  // B: layer 4 reads every filter's layer-3 rows
    MIB_STAMP(4)
    wprev = w;
  }
  MIB_STAMP_FLUSH(lane == 0, wave)
}

// The same over W windows at caller-given sample onsets (net_model_compute_windows_at): window w
// covers samples onsets[w] .. onsets[w] + T - 1 of the workspace rows, in any order, duplicates
// allowed.  last = Lr - T, the largest valid onset.  An onset outside [0, last] forms no address:
// its rows are not copied (layers 2-3 run on whatever the y1 rows hold and their result is
// dropped), its logit row is written as zeros and *n_bad (if non-null) counts it, as
// ep::k_forward_ep does; the previous window and its validity travel in one register.
template <bool RB, bool XR, bool CB>
__global__ __launch_bounds__(gen::NT) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_forward_y1_at(
    const gen::GenParams* __restrict__ gp, const int8_t* __restrict__ ws, const long long* __restrict__ onsets,
    int8_t* __restrict__ out, int* __restrict__ n_bad, int W, long long last, int rs) {
  using namespace gen;
  extern __shared__ v4i smem_v[];
  int8_t* smem = (int8_t*)smem_v;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const Lds m = lds_of(gp, smem, 3);
  const Carve& cv = m.cv;
  L2C k2;
  setup(gp, m, k2, tid, wave, lane);
  const int T = gp->T, N = gp->N, NB1 = gp->NB1;
  __syncthreads();
  // (phase stamps as k_forward_y1)
  MIB_STAMP_INIT
  // the previous window and whether its onset was valid: w valid, -2 - w invalid, -1 none
  int wprev = -1;
  for (int w = blockIdx.x;; w += gridDim.x) {
    const bool more = w < W;  // uniform over the workgroup
    MIB_STAMP(7)
    const long long on = more ? onsets[w] : 0;  // (wave-uniform: one scalar load)
    const bool valid = (unsigned long long)on <= (unsigned long long)last;  // last >= 0: negative onsets fail too
    if (wave < NW - 1) {
      if (more && valid) copy_rows(window_view(ws, on, 1, T, rs), m.y1, cv.y1s, T, NB1, rs, tid, NT - 64);
    } else if (wprev != -1) {
      const bool vprev = wprev >= 0;
      int8_t* o = out + (size_t)(vprev ? wprev : -2 - wprev) * N;
      if (vprev) {
        __builtin_amdgcn_s_setprio(wg::PRIO_L45);
        finish_trial<RB, XR, CB>(gp, m, o, lane);
        __builtin_amdgcn_s_setprio(0);
      } else {
        if (lane < N) o[lane] = 0;
        if (lane == 0 && n_bad) atomicAdd(n_bad, 1);
      }
    }
    MIB_STAMP(0)
    if (!more) break;
    __syncthreads();  // A: layer 2 reads every wave's part of the y1 rows
    MIB_STAMP(1)
    layer2<RB, XR, CB>(gp, m.y1, cv.y1s, m.y2, cv.y2s, k2, wave, lane);
    wg::wave_sync_lds();  // layer 3 of filter f reads only y2 row f, written by this wave
    MIB_STAMP(2)
    __builtin_amdgcn_s_setprio(wg::PRIO_L3);
    layer3<XR, CB>(gp, m.sg, m.y2, cv.y2s, m.y3, wave, lane);
    __builtin_amdgcn_s_setprio(0);
    MIB_STAMP(3)
    __syncthreads();  // B: layer 4 reads every filter's layer-3 rows
    MIB_STAMP(4)
    wprev = valid ? w : -2 - w;
  }
  MIB_STAMP_FLUSH(lane == 0, wave)
}

}  // namespace win
}  // namespace mib
