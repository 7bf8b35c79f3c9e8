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
// Both read a gen::GenParams image (every geometry, the compiled ones included) and are built
// from the run-time-dimension family (forward_gen.hpp); the compiled wg:: kernels are untouched.
#pragma once
#include "forward_gen.hpp"

namespace mib {
namespace win {

constexpr int NW1 = 4;          // waves per workgroup of k_layer1_rec, one 16-sample block each per step
constexpr int NT1 = 64 * NW1;

// gen::load16u with an unsigned byte offset (the builtin's offset operand is the same 32 bits).
__device__ __forceinline__ v4i load16u_u(wg::Rsrc r, unsigned o) {
  const unsigned o4 = o & ~3u, s = o & 3u;
  const gen::v4u a = __builtin_amdgcn_raw_buffer_load_b128(r, (int)o4, 0, 0);
  const unsigned e = __builtin_amdgcn_raw_buffer_load_b32(r, (int)(o4 + 16u), 0, 0);
  return (v4i){(int)__builtin_amdgcn_alignbyte(a[1], a[0], s), (int)__builtin_amdgcn_alignbyte(a[2], a[1], s),
               (int)__builtin_amdgcn_alignbyte(a[3], a[2], s), (int)__builtin_amdgcn_alignbyte(e, a[3], s)};
}

// gen::l1_fetch over the recording (row stride Lr), with the byte offsets computed unsigned: the
// host admits recordings up to 2^31 - 1 bytes, so the offsets of the partial last block (samples
// >= Lr, rows past the last) reach a little past 2^31 (below 2^31 + 2^11).  The hardware compares
// the offset with num_records unsigned, so those loads return zeros, as in gen::l1_fetch; here the
// arithmetic that gets there is defined too.
template <int L>
__device__ __forceinline__ v4i rec_fetch(const gen::View& v, int blk, int C, int Lr, int lane, float qs, float qy) {
  const unsigned uC = (unsigned)C, uL = (unsigned)Lr, ub = 16u * (unsigned)blk, d = (unsigned)v.delta;
  if constexpr (L == gen::TM) {
    const unsigned j = lane & 15, g = lane >> 4;
    return load16u_u(v.r, d + (ub + j) * uC + 16u * (unsigned)gen::l1_chunk((int)g, C));
  } else if constexpr (L == gen::CT) {
    return load16u_u(v.r, d + (unsigned)min(lane, C - 1) * uL + ub);
  } else {
    const unsigned c = (unsigned)min(lane, C - 1);
    v4i w;
#pragma unroll
    for (int m = 0; m < 4; m++) {
      const gen::v4u f = __builtin_amdgcn_raw_buffer_load_b128(v.r, (int)(4u * (c * uL + ub) + 16u * m), 0, 0);
      int q[4];
#pragma unroll
      for (int i = 0; i < 4; i++) q[i] = (int)wg::quantize1_f(__uint_as_float(f[i]), qs, qy);
      w[m] = (int)gen::pack4(q[0], q[1], q[2], q[3]);
    }
    return w;
  }
}

// Layer 1 of recording blocks blk = 16 samples (gen::layer1's block, the recording length Lr as the
// row stride of the channel-major layouts), one wave per block, grid-strided.  x: the recording in
// layout L (gen::Layout: [Lr][C] int8, [C][Lr] int8, [C][Lr] float32), any byte alignment (float32:
// 4); the view's bound keeps every load inside the recording (a partial last block reads zeros or
// the next row, and its samples >= Lr are stored as zeros).  ws: [F1][rs], rs >= 16 ceil(Lr / 16).
template <int L, bool XR, bool CB>
__global__ __launch_bounds__(NT1) void k_layer1_rec(const gen::GenParams* __restrict__ gp,
                                                    const int8_t* __restrict__ x, int8_t* __restrict__ ws, int Lr,
                                                    int rs, float qs, float qy) {
  __shared__ v4i stg_v[NW1 * 64];  // channel-major transpose staging, 1 KB per wave
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int8_t* stg = (int8_t*)stg_v + 1024 * wave;
  const int C = gp->C;
  const int j = lane & 15, g = lane >> 4;
  gen::L1C k;
  k.wf = L == gen::TM ? gp->l1_b[lane] : gp->l1_bn[lane];
  k.off = gp->l1_off[j];
  k.m = gp->l1_m[j];
  k.xs = gp->l1_xs[j];
  k.r = gp->l1_r[j];
  k.c = gp->l1_c[j];
  // the whole recording as one "trial" (gen::trial_view; unsigned: delta + bytes + 3 may pass 2^31 - 1)
  gen::View v;
  v.delta = (int)((size_t)x & 3);
  const unsigned bytes = (L == gen::F32 ? 4u : 1u) * (unsigned)C * (unsigned)Lr;
  v.r = __builtin_amdgcn_make_buffer_rsrc((void*)(x - v.delta), (short)0, (int)(((unsigned)v.delta + bytes + 3u) & ~3u),
                                          0x00020000);
  const int NB = (Lr + 15) / 16;
  int8_t* row = ws + (size_t)j * (size_t)rs;
  for (int blk = (int)blockIdx.x * NW1 + wave; blk < NB; blk += (int)gridDim.x * NW1) {  // wave-uniform
    const v4i raw = rec_fetch<L>(v, blk, C, Lr, lane, qs, qy);
    const v4i a = L == gen::TM ? raw : wg::stage_block<gen::TrK>(raw, stg, lane);
    const v4i acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, k.wf, (v4i){k.off, k.off, k.off, k.off}, 0, 0, 0);
    // lane column j = filter j, rows 4 g + r = samples 16 blk + 4 g + r
    const int t0 = 16 * blk + 4 * g;
    int y[4];
#pragma unroll
    for (int r = 0; r < 4; r++) y[r] = gen::rq1<XR, CB>(acc[r], k.m, k.xs, k.r, k.c);
    if (blk == NB - 1) {  // the recording's last block: samples >= Lr are zero inside the row stride
#pragma unroll
      for (int r = 0; r < 4; r++) y[r] = t0 + r < Lr ? y[r] : 0;
    }
    *(unsigned*)(row + t0) = gen::sat4(y[0], y[1], y[2], y[3]);
  }
}

// The view of window w's sixteen workspace rows: base = ws + w hop rounded down to a dword, delta
// = the rest (the same for every row: ws is 16-byte aligned and rs a multiple of 16), row f at
// byte f rs.  num_records ends with the dword holding row 15's last window byte, which lies inside
// the workspace (w hop + T <= L <= rs).  Offsets stay below 2^31 (16 rs <= 2^31, the host's limit).
__device__ __forceinline__ gen::View window_view(const int8_t* ws, long long w, int hop, int T, int rs) {
  const int8_t* p = ws + w * hop;
  const int delta = (int)((size_t)p & 3);
  gen::View v;
  v.r = __builtin_amdgcn_make_buffer_rsrc((void*)(p - delta), (short)0, 15 * rs + ((delta + T + 3) & ~3), 0x00020000);
  v.delta = delta;
  return v;
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
  const Carve cv = carve_of(gp->C, gp->T, gp->N, gp->T8, gp->T64A, gp->NB1, gp->MT, gp->NTT, 3);
  L1C k1;  // unused here (setup's layer-1 constants)
  L2C k2;
  setup(gp, smem, cv, k1, k2, tid, wave, lane);
  const SmallG* sg = (const SmallG*)(smem + cv.sg);
  int8_t* y1 = smem;
  int8_t* y2 = smem + cv.y2;
  int8_t* y3 = smem + cv.y3;
  int8_t* y4 = smem + cv.y4;
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
      if (more) copy_rows(window_view(ws, w, hop, T, rs), y1, cv.y1s, T, NB1, rs, tid, NT - 64);
    } else if (wprev >= 0) {
      __builtin_amdgcn_s_setprio(wg::PRIO_L45);
      layer4<RB, XR, CB>(gp, y3, y4, sg, lane, 0, 1);
      wg::wave_sync_lds();
      layer5<CB>(gp, y4, smem + cv.w5, out + (size_t)wprev * N, 0, 1, lane);
      __builtin_amdgcn_s_setprio(0);
    }
    MIB_STAMP(0)
    if (!more) break;
    __syncthreads();  // A: layer 2 reads every wave's part of the y1 rows
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
    wprev = w;
  }
  MIB_STAMP_FLUSH(lane == 0, wave)
}

}  // namespace win
}  // namespace mib
