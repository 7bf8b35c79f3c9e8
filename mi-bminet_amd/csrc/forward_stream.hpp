// forward_stream.hpp — live streams (gfx950): net_streams_push[_f32[_tm]], include/mibminet.h.  A stream
// group is S sessions of one bank's geometry, each decoded by its own set of the bank, all advancing
// by the same n samples per push.  Layer 1 is pointwise in time (forward_win.hpp), so its output is
// state that persists between calls: a push runs layer 1 on the n new samples of every session
// (k_layer1_ring) and layers 2-5 on the windows of the global grid o = j hop whose last sample
// arrived in it (k_forward_ring), reading each window's sixteen rows out of the session's ring.
//
// The ring.  Per session sixteen rows of 2 cap bytes (cap a multiple of 16, stream_host.hpp).  The
// output of absolute sample t for filter f is stored twice, at t mod cap and t mod cap + cap, so a
// window (T <= cap) is one contiguous run of T bytes from o mod cap, wherever the seam lies, and
// win::copy_rows reads it as it reads a workspace: almost every window wraps (cap - T is about
// max_push), so the seam must cost the reader nothing; the doubled stores are 32 n bytes per session
// and push against the 16 T a window reads.  A push keeps every sample its windows read
// (cap >= T + n - 1, stream_host.hpp).
//
// Per session the ring is followed, at the end of the group's one allocation, by origin[s] (int64:
// the first sample a window of the session may read) and set[s] (int32).  k_stream_restart changes
// both, stream-ordered; the push kernels read them with scalar loads.
//
// Each-groups (net_streams_push_each[_f32]): every session has its own position pos[s] in device
// memory and its own count per push.  k_stream_plan turns count and position into one record per
// session (plan_each, stream_host.hpp) and advances the position; k_layer1_ring_each and
// k_forward_ring_each are the two kernels above with n, p0, k and the first window's ring position
// read per session from that record, and from nothing else: the same three launches are valid on
// every replay of a captured graph.
//
// Queries (net_streams_windows_at): the window of a given session from a given sample, read out of
// the ring as it is, for cue-locked trials.  A retained window is one contiguous run of T bytes like
// any grid window, so k_forward_ring_at runs over a device list of (session, onset) items with
// AtRows as its source; it writes logits and *n_bad alone.  Which windows are retained, and for how
// long, is stream_host.hpp's at_item.  k_forward_ring_at_feat (net_streams_windows_at_feat) is that
// kernel writing each item's layer-4 activations as well.
//
// A decimator (net_streams_push_raw_f32_tm): raw float32 frames at q times the network's rate.
// k_layer1_ring_decim is k_layer1_ring<F32TM> with another fragment source, fir_fragment: each lane
// runs the K-tap FIR of its output sample over the chunk and the session's history of K - 1 raw
// frames, then the quantiser, so no decimated float array exists; k_history_update behind it moves
// the chunk's last frames into the histories; layers 2-5 are k_forward_ring as it is.
//
// An each-group's decimator (net_streams_push_each_raw_f32_tm): every session has its own raw
// position, phase and history slot in device memory.  k_stream_plan_raw turns raw count and raw
// position into the session's EachRec and a second record, RawRec (plan_each_raw, stream_host.hpp),
// and advances both positions; k_layer1_ring_each_decim is layer1_ring with EACH and DEC, off and
// slot0 read per session from that record; k_history_update_each moves each session's last frames;
// layers 2-5 are k_forward_ring_each as it is.  Four launches that read nothing from the host.
//
// A prefilter (net_streams_set_prefilter): M second-order sections that every raw frame passes, per
// session and electrode, before the FIR.  k_prefilter runs ahead of layer 1 (an each-group: after the
// plan, its trip counts from the raw records) and writes the filtered frames to a scratch of the
// group's; the layer-1 and history kernels above then take the scratch where they took x.
//
// One body each: the four layer-1 kernels are layer1_ring, and the four kernels of layers 2-5 are
// bank::set_loop (forward_bank.hpp) over their sources RingRows, EachRows and AtRows, which say
// where an item's rows are, whether it is valid and under which set.
#pragma once
#include "forward_bank.hpp"
#include "stream_host.hpp"  // EachRec, plan_each: shared with the host

namespace mib {
namespace stream {

using bank::Range64;
using bank::range_of;
using bank::Scale;

// ---- a decimator's fragment source (net_streams_push_raw_f32_tm) ----------------------------------
// What layer 1 of a raw push needs beside a plain push's arguments (stream_host.hpp, PushRaw): the
// taps and the histories in device memory, K, q, off = q D(P) - P, slot0 = P mod (K - 1) and the
// bytes of a session's history.
struct Decim {
  const float* taps;   // [K]
  const int8_t* hist;  // [S][K - 1][C] float32, frame a at slot a mod (K - 1)
  int K, q, off, slot0;
  unsigned per;        // 4 (K - 1) C
};

// The sixteen decimated floats of output sample dl of the push (dl counted from the push's first,
// in block blk: 16 blk <= dl < 16 blk + 16, blk wave-uniform) for the electrodes from float column
// col of a frame of C floats:
//   acc = +0; for k = 0 .. K - 1: acc = RN(acc + RN(taps[k] frame(q dl + off - k)[col + i])),
// every product and sum rounded to float32 on its own (contraction is off in this function).
// Subnormal intermediates follow the device's float mode.  Frame rel >= 0 is the chunk's (view vc),
// rel < 0 the history's slot (slot0 + rel) mod (K - 1) (view vh; rel >= -(K - 1)).  Both are buffer
// views: an offset past either end (a sample past the push's last, a column past the last frame's
// end) reads zeros, and a lane whose frame is in the other view is given an offset past the end of
// this one (~15u: beyond any num_records here, and +48 does not wrap).  Which of the two loads a tap
// needs at all is decided per wave from blk.  The tap is read uniformly (a scalar load).
__device__ __forceinline__ void fir_taps16(const gen::View& vc, const gen::View& vh, const Decim& dc, int dl, int blk,
                                           unsigned col, unsigned C, float (&acc)[16]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 16; i++) acc[i] = 0.0f;
  const int r_lo = dc.q * 16 * blk + dc.off, r_hi = r_lo + dc.q * 15;  // the block's rel at k = 0
  // four taps' loads in flight (a wave has few neighbours on its SIMD here); the sums of one
  // accumulator stay in tap order.  This loop is where the time of a raw push over a plain one goes
  // ("Raw frames")
#pragma unroll 4
  for (int k = 0; k < dc.K; k++) {  // wave-uniform
    const float h = dc.taps[k];
    const int rel = dc.q * dl + dc.off - k;
    const bool in_chunk = rel >= 0;
    gen::v4u f[4];
#pragma unroll
    for (int m = 0; m < 4; m++) f[m] = (gen::v4u){0u, 0u, 0u, 0u};
    if (r_hi - k >= 0) {  // some lane's frame is in the chunk
      const unsigned o = in_chunk ? 4u * ((unsigned)rel * C + col) : ~15u - 48u;
#pragma unroll
      for (int m = 0; m < 4; m++) f[m] = __builtin_amdgcn_raw_buffer_load_b128(vc.r, (int)(o + 16u * m), 0, 0);
    }
    if (r_lo - k < 0) {  // some lane's frame is in the history
      const int sl = dc.slot0 + rel;  // >= -(K - 1) where the lane reads it
      const unsigned o = in_chunk ? ~15u - 48u : 4u * ((unsigned)(sl < 0 ? sl + dc.K - 1 : sl) * C + col);
#pragma unroll
      for (int m = 0; m < 4; m++) {
        const gen::v4u e = __builtin_amdgcn_raw_buffer_load_b128(vh.r, (int)(o + 16u * m), 0, 0);
        f[m] |= e;  // the other view gave zeros
      }
    }
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const float p = h * __uint_as_float(f[i >> 2][i & 3]);
      acc[i] = acc[i] + p;
    }
  }
}

// The A fragment of block blk of a raw push, in place of gen::l1_fetch<F32TM>: lane (j, g) owns
// output sample 16 blk + j and the electrodes 16 c .. 16 c + 15, c = l1_chunk(g, C); the sixteen
// floats of fir_taps16 quantised as gen::load16f quantises a frame's.
__device__ __forceinline__ v4i fir_fragment(const gen::View& vc, const gen::View& vh, const Decim& dc, int blk, int C,
                                            int lane, float qs, float qy) {
  float acc[16];
  fir_taps16(vc, vh, dc, 16 * blk + (lane & 15), blk, 16u * (unsigned)gen::l1_chunk(lane >> 4, C), (unsigned)C, acc);
  v4i w;
#pragma unroll
  for (int m = 0; m < 4; m++) {
    int q[4];
#pragma unroll
    for (int i = 0; i < 4; i++) q[i] = (int)wg::quantize1_f(acc[4 * m + i], qs, qy);
    w[m] = (int)gen::pack4(q[0], q[1], q[2], q[3]);
  }
  return w;
}

// Layer 1 of the new samples, the body of k_layer1_ring and k_layer1_ring_each.  Items are (session
// s, 16-sample block b of its chunk), session-major (item = s nb + b); wave g of gridDim.x NW1 takes
// the contiguous items range_of(g, gridDim.x NW1, S nb) with a current set per wave, as
// bank::k_layer1_rec_bank does.  x: the S chunks of n_view samples each, contiguous, in layout L
// ([n][C] int8, [C][n] int8, [C][n] float32, [n][C] float32) at any byte alignment (float32: 4); the
// view is one session's chunk, the row stride of the channel-major layouts n_view (so a time-major
// fragment's K-slots past C read the session's own next sample, or zeros past its last).  A set
// index is compared unsigned before any address is formed from it; a session whose index is outside
// the bank stores nothing.  Stores: sample 16 b + 4 g + r < n of the chunk goes to position
// (p0 + 16 b + 4 g + r) mod cap of the lane's row and to that + cap.  Samples >= n of a partial last
// block are not stored: their positions hold live older samples.  Where p0 is a multiple of 4 a
// lane's four positions do not cross the seam (cap is a multiple of 4) and, when all four samples
// exist, leave as two dwords; otherwise as bytes.
// DEC (a raw push, L = F32TM): x holds the S chunks of n_view raw frames, n is the m decimated
// samples they complete, and block b's fragment is fir_fragment's, from the chunk and the session's
// history; everything after the fragment is a plain push's.
// EACH: n and p0 are the session's own, read from its plan record (wave-uniform: one scalar load;
// k_stream_plan validated the record, so n <= n_view = n_max and p0 < cap), and a wave skips the
// blocks b >= ceil(n / 16); samples >= n are read inside the session's slot and not stored.
// EACH and DEC (an each-group's raw push): x holds the S fixed slots of n_view raw frames, n is the
// session's m, and off and slot0 are the session's own, read from its raw record (wave-uniform: one
// more scalar load per item) into the item's copy of dc, so fir_taps16's r_lo and r_hi stay
// wave-uniform: a wave's item is one session's block.  The chunk's view ends with the session's
// n_raw-th frame: the rest of its slot is never read.
template <int L, bool XR, bool CB, bool EACH, bool DEC = false>
__device__ __forceinline__ void layer1_ring(const gen::GenParams* __restrict__ sets, int n_sets,
                                            const int* __restrict__ set_of, const Scale* __restrict__ scales,
                                            const int8_t* __restrict__ x, int8_t* __restrict__ ring,
                                            const EachRec* __restrict__ plan, int items, int nb, int n_view, int n,
                                            int p0, int cap, const Decim& dc = Decim{},
                                            const RawRec* __restrict__ raw = nullptr) {
  __shared__ v4i stg_v[win::NW1 * 64];  // channel-major transpose staging, 1 KB per wave
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int8_t* stg = (int8_t*)stg_v + 1024 * wave;
  const int C = sets->C;  // every set's
  const unsigned chunk = gen::elem_bytes(L) * (unsigned)C * (unsigned)n_view;  // <= 2^24
  const int g = lane >> 4;
  const Range64 rg = range_of(blockIdx.x * win::NW1 + (unsigned)wave, gridDim.x * win::NW1, (unsigned long long)items);
  const int end = (int)rg.hi;
  gen::L1C k{};
  float qs = 0.0f, qy = 0.0f;
  int cur = -1;
  for (int it = (int)rg.lo; it < end; it++) {  // wave-uniform
    const int s = it / nb, b = it - s * nb;
    if constexpr (EACH) {
      const EachRec rec = plan[s];
      n = rec.n;
      p0 = rec.p0;
      if (16 * b >= n) continue;
    }
    const int set = set_of[s];
    if ((unsigned)set >= (unsigned)n_sets) continue;
    if (set != cur) {
      cur = set;
      k = gen::l1_consts<L>(sets + set, lane);
      if constexpr (gen::is_float(L)) {
        const Scale q = scales[set];
        qs = q.qs;
        qy = q.qy;
      }
    }
    const gen::View v = gen::make_view(x + (size_t)s * chunk, chunk);
    int y[4];
    if constexpr (DEC && EACH) {
      const RawRec rr = raw[s];
      Decim ds = dc;
      ds.off = rr.off;
      ds.slot0 = rr.slot0;
      const gen::View vs = gen::make_view(x + (size_t)s * chunk, 4u * (unsigned)C * (unsigned)rr.n_raw);
      const gen::View vh = gen::make_view(dc.hist + (size_t)s * dc.per, dc.per);
      gen::l1_outputs<L, XR, CB>(fir_fragment(vs, vh, ds, b, C, lane, qs, qy), stg, k, lane, y);
    } else if constexpr (DEC) {
      const gen::View vh = gen::make_view(dc.hist + (size_t)s * dc.per, dc.per);
      gen::l1_outputs<L, XR, CB>(fir_fragment(v, vh, dc, b, C, lane, qs, qy), stg, k, lane, y);
    } else {
      gen::l1_outputs<L, XR, CB>(gen::l1_fetch<L>(v, b, C, n_view, lane, qs, qy), stg, k, lane, y);
    }
    const unsigned w = gen::sat4(y[0], y[1], y[2], y[3]);
    int8_t* row = ring + ((size_t)s * 16 + (size_t)(lane & 15)) * (size_t)(2 * cap);
    const int t0 = 16 * b + 4 * g;  // the lane's first sample of the chunk
    int q = p0 + t0;                // < 2 cap: p0 < cap, t0 < n <= cap
    q = q >= cap ? q - cap : q;
    if ((p0 & 3) == 0 && t0 + 3 < n) {
      *(unsigned*)(row + q) = w;
      *(unsigned*)(row + q + cap) = w;
    } else {
#pragma unroll
      for (int r = 0; r < 4; r++) {
        if (t0 + r < n) {
          const int qr = q + r >= cap ? q + r - cap : q + r;
          const int8_t byte = (int8_t)(w >> (8 * r));
          row[qr] = byte;
          row[qr + cap] = byte;
        }
      }
    }
  }
}

// A uniform group's layer 1 (net_streams_push): every session's chunk is n samples from ring
// position p0.
template <int L, bool XR, bool CB>
__global__ __launch_bounds__(win::NT1) void k_layer1_ring(const gen::GenParams* __restrict__ sets, int n_sets,
                                                          const int* __restrict__ set_of,
                                                          const Scale* __restrict__ scales,
                                                          const int8_t* __restrict__ x, int8_t* __restrict__ ring,
                                                          int items, int nb, int n, int p0, int cap) {
  layer1_ring<L, XR, CB, false>(sets, n_sets, set_of, scales, x, ring, nullptr, items, nb, n, n, p0, cap);
}

// Layer 1 of a raw push (net_streams_push_raw_f32_tm): the S chunks of n_raw float32 frames [n_raw][C]
// complete n decimated samples per session, which go to the rings from position p0 as a plain
// push's do.  It reads the histories and writes none: k_history_update follows it.
template <bool XR, bool CB>
__global__ __launch_bounds__(win::NT1) void k_layer1_ring_decim(const gen::GenParams* __restrict__ sets, int n_sets,
                                                                const int* __restrict__ set_of,
                                                                const Scale* __restrict__ scales,
                                                                const int8_t* __restrict__ x, int8_t* __restrict__ ring,
                                                                int items, int nb, int n_raw, int n, int p0, int cap,
                                                                Decim dc) {
  layer1_ring<gen::F32TM, XR, CB, false, true>(sets, n_sets, set_of, scales, x, ring, nullptr, items, nb, n_raw, n, p0, cap,
                                               dc);
}

// The second kernel of a raw push (K > 1), after layer 1 has read the old histories: the last keep =
// min(n_raw, K - 1) frames of every session's chunk go to their history slots, frame rel of the chunk
// (n_raw - keep <= rel < n_raw) to slot (slot0 + rel) mod (K - 1).  One thread per float, grid-stride
// over the S keep C floats in 64 bits.
__global__ void k_history_update(const float* __restrict__ x, float* __restrict__ hist, unsigned long long items,
                                 unsigned C, unsigned n_raw, unsigned keep, unsigned K, unsigned slot0) {
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < items;
       i += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned c = (unsigned)(i % C);
    const unsigned long long sf = i / C, s = sf / keep;
    const unsigned rel = n_raw - keep + (unsigned)(sf - s * keep);
    const unsigned slot = (slot0 + rel) % (K - 1);
    hist[(s * (K - 1) + slot) * C + c] = x[(s * n_raw + rel) * C + c];
  }
}

// test hook (mibminet_test_fir_decimate): fir_taps16 on one session's chunk x [n_raw][R] and history
// hist [K - 1][R] (views of their sizes), one wave per 16-sample block and lane (j, g) on electrodes
// 16 g .. 16 g + 15 as layer 1 places them at R > 32; out [m][R] float32, the bits as they are.
__global__ void k_fir_decimate(const float* __restrict__ x, const float* __restrict__ hist, float* __restrict__ out,
                               int n_raw, int R, int m, Decim dc) {
  const int lane = threadIdx.x & 63, blk = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (16 * blk >= m) return;  // wave-uniform
  const gen::View vc = gen::make_view((const int8_t*)x, 4u * (unsigned)n_raw * (unsigned)R);
  const gen::View vh = gen::make_view((const int8_t*)hist, dc.per);
  const int dl = 16 * blk + (lane & 15), col = 16 * (lane >> 4);
  float acc[16];
  fir_taps16(vc, vh, dc, dl, blk, (unsigned)col, (unsigned)R, acc);
  if (dl < m)
    for (int i = 0; i < 16; i++)
      if (col + i < R) out[(size_t)dl * R + col + i] = acc[i];
}

// An each-group's layer 1 (net_streams_push_each): items are (s, b) with b < nb = ceil(n_max / 16),
// the view is the session's fixed slot of n_max samples.
template <int L, bool XR, bool CB>
__global__ __launch_bounds__(win::NT1) void k_layer1_ring_each(const gen::GenParams* __restrict__ sets, int n_sets,
                                                               const int* __restrict__ set_of,
                                                               const Scale* __restrict__ scales,
                                                               const int8_t* __restrict__ x, int8_t* __restrict__ ring,
                                                               const EachRec* __restrict__ plan, int items, int nb,
                                                               int n_max, int cap) {
  layer1_ring<L, XR, CB, true>(sets, n_sets, set_of, scales, x, ring, plan, items, nb, n_max, 0, 0, cap);
}

// Layer 1 of an each-group's raw push (net_streams_push_each_raw_f32_tm): items are (s, b) with
// b < nb = ceil(ceil(n_raw_max / q) / 16), x the S fixed slots of n_raw_max float32 frames [n_raw_max][C].
// Session s's m samples, ring position, phase and history slot come from its two records; dc's off
// and slot0 are unused.  It reads the histories and writes none: k_history_update_each follows it.
template <bool XR, bool CB>
__global__ __launch_bounds__(win::NT1) void k_layer1_ring_each_decim(
    const gen::GenParams* __restrict__ sets, int n_sets, const int* __restrict__ set_of, const Scale* __restrict__ scales,
    const int8_t* __restrict__ x, int8_t* __restrict__ ring, const EachRec* __restrict__ plan,
    const RawRec* __restrict__ raw, int items, int nb, int n_raw_max, int cap, Decim dc) {
  layer1_ring<gen::F32TM, XR, CB, true, true>(sets, n_sets, set_of, scales, x, ring, plan, items, nb, n_raw_max, 0, 0, cap, dc,
                                              raw);
}

// The history kernel of an each-group's raw push (K > 1), after layer 1 has read the old histories:
// the last keep[s] = min(n_raw[s], K - 1) frames of session s's slot go to its history slots, frame
// rel (n_raw - keep <= rel < n_raw) to slot (slot0[s] + rel) mod (K - 1).  Grid-stride over the
// S keep_max C floats in 64 bits, keep_max = min(n_raw_max, K - 1); an index at or past its session's
// keep is passed over, so a refused or skipped session (keep = 0) moves nothing.  It runs when no
// session completed a sample too.
__global__ void k_history_update_each(const float* __restrict__ x, float* __restrict__ hist,
                                      const RawRec* __restrict__ raw, unsigned long long items, unsigned C,
                                      unsigned n_raw_max, unsigned keep_max, unsigned K) {
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < items;
       i += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned c = (unsigned)(i % C);
    const unsigned long long sf = i / C, s = sf / keep_max;
    const unsigned j = (unsigned)(sf - s * keep_max);
    const RawRec r = raw[s];
    if (j >= (unsigned)r.keep) continue;
    const unsigned rel = (unsigned)(r.n_raw - r.keep) + j;  // < n_raw <= n_raw_max
    const unsigned slot = ((unsigned)r.slot0 + rel) % (K - 1);
    hist[(s * (K - 1) + slot) * C + c] = x[(s * n_raw_max + rel) * C + c];
  }
}

// ---- a prefilter: an IIR cascade ahead of the decimator (net_streams_set_prefilter) ----------------
// One raw sample v of one electrode through the M sections, ascending, transposed direct form II
// with z[j] = {z1, z2} of section j:
//   w = RN(RN(b0 v) + z1);  z1' = RN(RN(RN(b1 v) - RN(a1 w)) + z2);  z2' = RN(RN(b2 v) - RN(a2 w))
// and w the next section's v.  Every product and every sum or difference is a float32 operation of
// its own (contraction is off in this function).  The coefficients are kernel arguments, indexed by
// constants: scalar registers.
template <int M>
__device__ __forceinline__ float sos_sample(const Sos& c, float (&z)[M][2], float v) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < M; j++) {
    const float p0 = c.c[j][0] * v;
    const float w = p0 + z[j][0];
    const float p1 = c.c[j][1] * v, q1 = c.c[j][3] * w;
    const float d1 = p1 - q1;
    const float p2 = c.c[j][2] * v, q2 = c.c[j][4] * w;
    z[j][0] = d1 + z[j][1];
    z[j][1] = p2 - q2;
    v = w;
  }
  return v;
}

constexpr int PF_AHEAD = 8;  // frames whose loads are issued ahead of the recurrence

// One lane's electrode over its session's n frames, in arrival order.  x and y point at the lane's
// float of the session's first frame (frames R floats apart), st at its float of the session's state
// [M][2][R].  The 2 M states stay in registers from the first frame to the last.  The loads of the
// next PF_AHEAD frames are issued before the current ones go through the recurrence: they do not
// depend on it, and a wave has few neighbours on its SIMD here to hide them behind.  A frame at or
// past n is neither read nor written.
template <int M>
__device__ __forceinline__ void sos_lane(const float* __restrict__ x, float* __restrict__ y, float* __restrict__ st,
                                         size_t R, int n, const Sos& c) {
  float z[M][2];
#pragma unroll
  for (int j = 0; j < M; j++) {
    z[j][0] = st[(size_t)(2 * j) * R];
    z[j][1] = st[(size_t)(2 * j + 1) * R];
  }
  float cur[PF_AHEAD], nxt[PF_AHEAD];
#pragma unroll
  for (int u = 0; u < PF_AHEAD; u++) cur[u] = u < n ? x[(size_t)u * R] : 0.0f;
  for (int t = 0; t < n; t += PF_AHEAD) {
#pragma unroll
    for (int u = 0; u < PF_AHEAD; u++) nxt[u] = t + PF_AHEAD + u < n ? x[(size_t)(t + PF_AHEAD + u) * R] : 0.0f;
#pragma unroll
    for (int u = 0; u < PF_AHEAD; u++)
      if (t + u < n) y[(size_t)(t + u) * R] = sos_sample<M>(c, z, cur[u]);
#pragma unroll
    for (int u = 0; u < PF_AHEAD; u++) cur[u] = nxt[u];
  }
#pragma unroll
  for (int j = 0; j < M; j++) {
    st[(size_t)(2 * j) * R] = z[j][0];
    st[(size_t)(2 * j + 1) * R] = z[j][1];
  }
}

// The prefilter of a raw push, ahead of layer 1: one lane per (session, electrode), flat index
// i = s R + r over lanes = S R (64 bits; grid-stride), so the lanes of a session read the 4 R
// contiguous bytes of a frame.  x: the S chunks (EACH: fixed slots) of n_view raw frames [n_view][R];
// y: the scratch, the same frames filtered at the same stride; state: [S][M][2][R].  A session's
// trip count is n_view, or (EACH) its RawRec.n_raw, which k_stream_plan_raw validated (compared with
// n_view all the same): a refused or skipped session (n_raw = 0) moves no state, and the rest of a
// slot is never read.  Offsets are formed in 64 bits: S n_view R 4 can pass 2^32.  No LDS, no
// scratch memory.  The recurrence is serial in time by contract: the parallelism is the S R lanes.
// It is also the kernel of the test hook (mibminet_test_sos_filter), with S = 1.
template <bool EACH, int M>
__global__ __launch_bounds__(64) void k_prefilter(const float* __restrict__ x, float* __restrict__ y,
                                                  float* __restrict__ state, const RawRec* __restrict__ raw,
                                                  unsigned long long lanes, unsigned R, unsigned n_view, Sos c) {
  for (unsigned long long i = (unsigned long long)blockIdx.x * 64u + threadIdx.x; i < lanes;
       i += (unsigned long long)gridDim.x * 64u) {
    const unsigned long long s = i / R;
    const unsigned r = (unsigned)(i - s * R);
    unsigned n = n_view;
    if constexpr (EACH) n = min((unsigned)raw[s].n_raw, n_view);
    const size_t at = (size_t)s * n_view * R + r;
    sos_lane<M>(x + at, y + at, state + (size_t)s * (2 * M) * R + r, R, (int)n, c);
  }
}

// The first kernel of an each-group's raw push: one thread per session.  It reads cnt_in[s] and the
// raw position P[s], writes both of the session's records (plan_each_raw, stream_host.hpp: the count
// is validated there, unsigned, before anything is formed from it), cnt_out[s] (the windows
// completed, -1 for a refused count), win0[s] and *n_bad, and advances P[s] and pos[s] = D(P[s]).
// The kernels after it read only the records, never cnt_in, P or pos.
__global__ void k_stream_plan_raw(const int* __restrict__ cnt_in, long long* __restrict__ raw_pos,
                                  long long* __restrict__ pos, EachRec* __restrict__ plan, RawRec* __restrict__ raw,
                                  int* __restrict__ cnt_out, long long* __restrict__ win0, int* __restrict__ n_bad, int S,
                                  int T, unsigned long long hop, int cap, int q, int K, int n_raw_max) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const long long P = raw_pos[s];
  const EachRawPlan e = plan_each_raw((unsigned)T, hop, (unsigned)cap, (unsigned)q, (unsigned)K, P, cnt_in[s],
                                      (unsigned)n_raw_max);
  plan[s] = e.each.rec;
  raw[s] = e.raw;
  cnt_out[s] = e.each.ok ? e.each.rec.k : -1;
  if (win0) win0[s] = e.each.W0;
  if (!e.each.ok && n_bad) atomicAdd(n_bad, 1);
  raw_pos[s] = P + e.raw.n_raw;
  pos[s] = pos[s] + e.each.rec.n;
}

// The first kernel of an each-group's push: one thread per session.  It reads cnt_in[s] and pos[s],
// writes the session's record (plan_each, stream_host.hpp: the count is validated there, unsigned,
// before anything is formed from it; the 64-bit divisions happen here, once per session and push),
// cnt_out[s] (the windows completed, -1 for a refused count), win0[s] and *n_bad, and advances
// pos[s].  The two kernels after it read only the records, never cnt_in or pos: the advance cannot
// race with them, and a refused count (n = k = 0) reaches no address.
__global__ void k_stream_plan(const int* __restrict__ cnt_in, long long* __restrict__ pos, EachRec* __restrict__ plan,
                              int* __restrict__ cnt_out, long long* __restrict__ win0, int* __restrict__ n_bad, int S,
                              int T, unsigned long long hop, int cap, int n_max) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const long long p = pos[s];
  const EachPlan e = plan_each((unsigned)T, hop, (unsigned)cap, p, cnt_in[s], (unsigned)n_max);
  plan[s] = e.rec;
  cnt_out[s] = e.ok ? e.rec.k : -1;
  if (win0) win0[s] = e.W0;
  if (!e.ok && n_bad) atomicAdd(n_bad, 1);
  pos[s] = p + e.rec.n;
}

// Where the bank loop finds item i = s k + j of a push: window j of session s, the window of the
// global grid at onset o = first + j hop (64 bits).  open() reads origin[s] and set[s] (wave-uniform:
// two scalar loads); the set is compared unsigned against n_sets before any address is formed from
// it, and the item is valid iff o >= origin[s] and the set is in range.  Its rows are win::copy_rows
// on the view of session s's ring from o mod cap, row stride 2 cap: o mod cap = (first mod cap +
// j hop) mod cap in 32 bits with one conditional subtraction, the onsets of one push lying less than
// n <= cap apart.  T is held or read per window as win::Rows does (HT).  gp is the current set's,
// changed by the loop.
template <bool HT>
struct RingRows {
  const int8_t* ring;
  const long long* origin;
  const int* set_of;
  const gen::GenParams* gp;
  long long first, hop;
  int k, first_mod, cap, n_sets, T, NB1, y1s, tid;
  int8_t* y1;
  struct Item {
    int session, at;  // the window's session and its first byte in the session's rows
    bool valid;
    int s;            // the window's set, meaningful if valid
  };
  __device__ __forceinline__ Item open(int i, bool more) const {
    if (!more) return Item{0, 0, false, 0};
    const int session = i / k, j = i - session * k;
    const long long d = (long long)j * hop;  // < n
    const int st = set_of[session];
    const bool valid = first + d >= origin[session] && (unsigned)st < (unsigned)n_sets;
    const int at = first_mod + (int)d;  // < 2 cap
    return Item{session, at >= cap ? at - cap : at, valid, st};
  }
  __device__ __forceinline__ void rows(const Item& it) const {
    const int t = HT ? T : gp->T;
    if (it.valid)
      win::copy_rows(win::window_view(ring + (size_t)it.session * (size_t)(32 * cap), it.at, t, 2 * cap), y1, y1s, t, NB1,
                     2 * cap, tid, gen::NT - 64);
  }
  __device__ __forceinline__ void rows_last(const Item&) const {}
  static constexpr bool SKIP = false;
  __device__ __forceinline__ void on_switch(int, int) const {}
};

// bank::set_loop over the W = S k windows of a push, logits [S][k][N] (session-major items: a range
// changes sets when it changes sessions).
template <bool RB, bool XR, bool CB>
__global__ __launch_bounds__(gen::NT) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_forward_ring(
    const gen::GenParams* __restrict__ sets, int n_sets, const int8_t* __restrict__ ring,
    const long long* __restrict__ origin, const int* __restrict__ set_of, int8_t* __restrict__ out,
    int* __restrict__ n_bad, int W, int k, long long first, long long hop, int first_mod, int cap) {
  extern __shared__ v4i smem_v[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const gen::Lds m = bank::carve_and_pads(sets, (int8_t*)smem_v, 3, tid);
  RingRows<RB || XR> src{ring, origin, set_of, sets,      first, hop, k,  first_mod,
                         cap,  n_sets, sets->T, sets->NB1, m.cv.y1s, tid, m.y1};
  bank::set_loop<RB, XR, CB, false>(sets, m, src, out, nullptr, n_bad, W, tid, wave, lane);
}

// Where the loop finds item i = s kmax + j of an each-group's push: window j of those session s
// completes in it.  open() reads the session's record and set[s] (wave-uniform: scalar loads).  The
// item exists iff j < k[s] (and the set is in the bank, which create and restart see to): its rows
// start at ring position (at0 + j hop) mod cap, one conditional subtraction (at0 < cap and
// j hop < n[s] <= cap).  An item that does not exist is no invalid window: bank::set_loop passes
// over it (SKIP) and nothing is written.
template <bool HT>
struct EachRows {
  const int8_t* ring;
  const EachRec* plan;
  const int* set_of;
  const gen::GenParams* gp;
  int kmax, hop, cap, n_sets, T, NB1, y1s, tid;
  int8_t* y1;
  struct Item {
    int session, at;
    bool valid;  // the item exists
    int s;       // its set, meaningful if valid
  };
  __device__ __forceinline__ Item open(int i, bool more) const {
    if (!more) return Item{0, 0, false, 0};
    const int session = i / kmax, j = i - session * kmax;
    const EachRec r = plan[session];
    const int st = set_of[session];
    const bool valid = j < r.k && (unsigned)st < (unsigned)n_sets;
    const int at = r.at0 + j * hop;  // j hop < n_max + hop <= 2^17; < 2 cap where the item exists
    return Item{session, at >= cap ? at - cap : at, valid, st};
  }
  __device__ __forceinline__ void rows(const Item& it) const {
    const int t = HT ? T : gp->T;
    win::copy_rows(win::window_view(ring + (size_t)it.session * (size_t)(32 * cap), it.at, t, 2 * cap), y1, y1s, t, NB1,
                   2 * cap, tid, gen::NT - 64);
  }
  __device__ __forceinline__ void rows_last(const Item&) const {}
  static constexpr bool SKIP = true;
  __device__ __forceinline__ void on_switch(int, int) const {}
};

// bank::set_loop over the S kmax items of an each-group's push, logits [S][kmax][N]: row s kmax + j
// is written iff the item exists (EachRows::SKIP).  Every item that is not skipped is valid, so
// nothing is counted here.
template <bool RB, bool XR, bool CB>
__global__ __launch_bounds__(gen::NT) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_forward_ring_each(
    const gen::GenParams* __restrict__ sets, int n_sets, const int8_t* __restrict__ ring,
    const EachRec* __restrict__ plan, const int* __restrict__ set_of, int8_t* __restrict__ out, int W, int kmax, int hop,
    int cap) {
  extern __shared__ v4i smem_v[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const gen::Lds m = bank::carve_and_pads(sets, (int8_t*)smem_v, 3, tid);
  EachRows<RB || XR> src{ring, plan, set_of, sets, kmax, hop, cap, n_sets, sets->T, sets->NB1, m.cv.y1s, tid, m.y1};
  bank::set_loop<RB, XR, CB, false>(sets, m, src, out, nullptr, nullptr, W, tid, wave, lane);
}

// Where the loop finds item i of a query (net_streams_windows_at): the window of session
// session[i] whose first sample is onsets[i], read from the ring as it is.  open() reads the two
// (wave-uniform: scalar loads, as RingRows reads origin[s]), compares the session unsigned with S
// before anything is indexed by it, then reads set[s] and lim[s], the session's origin (a uniform
// group, whose position pos and pos mod cap come by argument) or its position (EACH: the onset's
// floor is 0, and pos[s] mod cap is one 64-bit remainder here, per item, beside layers 2-5 of a
// window; a plan pass would be a second launch and S records for W items).  Validity is
// stream::at_item, the function the host program walks; an invalid item forms no ring or parameter
// address.  The window's first byte is at_ring(pos mod cap, pos - o), its rows win::copy_rows on
// the view from there, row stride 2 cap, as RingRows'.
template <bool HT, bool EACH>
struct AtRows {
  const int8_t* ring;
  const int* session_of;
  const long long* onsets;
  const long long* lim;
  const int* set_of;
  const gen::GenParams* gp;
  long long pos;
  int pos_mod, S, cap, n_sets, T, NB1, y1s, tid;
  int8_t* y1;
  struct Item {
    int session, at;  // the window's session and its first byte in the session's rows
    bool valid;
    int s;            // the window's set, meaningful if valid
  };
  __device__ __forceinline__ Item open(int i, bool more) const {
    if (!more) return Item{0, 0, false, 0};
    const int session = session_of[i];
    const long long o = onsets[i];
    if ((unsigned)session >= (unsigned)S) return Item{0, 0, false, 0};
    const int st = set_of[session];
    const long long l = lim[session];
    const long long p = EACH ? l : pos;
    const int t = HT ? T : gp->T;
    const AtItem a = at_item(o, EACH ? 0ll : l, p, (unsigned)t, (unsigned)cap);
    if (!a.valid || (unsigned)st >= (unsigned)n_sets) return Item{0, 0, false, 0};
    const int pm = EACH ? (int)((unsigned long long)p % (unsigned)cap) : pos_mod;
    return Item{session, at_ring(pm, a.d, cap), true, st};
  }
  __device__ __forceinline__ void rows(const Item& it) const {
    const int t = HT ? T : gp->T;
    if (it.valid)
      win::copy_rows(win::window_view(ring + (size_t)it.session * (size_t)(32 * cap), it.at, t, 2 * cap), y1, y1s, t, NB1,
                     2 * cap, tid, gen::NT - 64);
  }
  __device__ __forceinline__ void rows_last(const Item&) const {}
  static constexpr bool SKIP = false;
  __device__ __forceinline__ void on_switch(int, int) const {}
};

// The body of k_forward_ring_at and k_forward_ring_at_feat: bank::set_loop over the W items of a
// query.  An invalid item keeps the current set and is finished as zeros and a count in *n_bad.
// Items are in the caller's order: sorted by session a range changes sets as seldom as a push's does.
template <bool RB, bool XR, bool CB, bool EACH, bool FEAT>
__device__ __forceinline__ void forward_ring_at(const gen::GenParams* __restrict__ sets, int n_sets,
                                                const int8_t* __restrict__ ring, const int* __restrict__ session_of,
                                                const long long* __restrict__ onsets,
                                                const long long* __restrict__ lim, const int* __restrict__ set_of,
                                                int8_t* __restrict__ out, int8_t* __restrict__ feat,
                                                int* __restrict__ n_bad, int W, int S, long long pos, int pos_mod,
                                                int cap) {
  extern __shared__ v4i smem_v[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const gen::Lds m = bank::carve_and_pads(sets, (int8_t*)smem_v, 3, tid);
  AtRows<RB || XR, EACH> src{ring, session_of, onsets, lim,     set_of,    sets,     pos, pos_mod,
                             S,    cap,        n_sets, sets->T, sets->NB1, m.cv.y1s, tid, m.y1};
  bank::set_loop<RB, XR, CB, FEAT>(sets, m, src, out, feat, n_bad, W, tid, wave, lane);
}

// The windows of a query, logits [W][N].  It reads the rings, the sets and the origins or positions,
// and writes out and *n_bad alone.
template <bool RB, bool XR, bool CB, bool EACH>
__global__ __launch_bounds__(gen::NT) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_forward_ring_at(
    const gen::GenParams* __restrict__ sets, int n_sets, const int8_t* __restrict__ ring,
    const int* __restrict__ session_of, const long long* __restrict__ onsets, const long long* __restrict__ lim,
    const int* __restrict__ set_of, int8_t* __restrict__ out, int* __restrict__ n_bad, int W, int S, long long pos,
    int pos_mod, int cap) {
  forward_ring_at<RB, XR, CB, EACH, false>(sets, n_sets, ring, session_of, onsets, lim, set_of, out, nullptr, n_bad, W, S,
                                           pos, pos_mod, cap);
}

// k_forward_ring_at with the layer-4 activations beside the logits (net_streams_windows_at_feat):
// feat [W][16][T64] int8, 16-byte aligned.  It writes out, feat and *n_bad alone.
template <bool RB, bool XR, bool CB, bool EACH>
__global__ __launch_bounds__(gen::NT) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_forward_ring_at_feat(
    const gen::GenParams* __restrict__ sets, int n_sets, const int8_t* __restrict__ ring,
    const int* __restrict__ session_of, const long long* __restrict__ onsets, const long long* __restrict__ lim,
    const int* __restrict__ set_of, int8_t* __restrict__ out, int8_t* __restrict__ feat, int* __restrict__ n_bad, int W,
    int S, long long pos, int pos_mod, int cap) {
  forward_ring_at<RB, XR, CB, EACH, true>(sets, n_sets, ring, session_of, onsets, lim, set_of, out, feat, n_bad, W, S,
                                          pos, pos_mod, cap);
}

// net_streams_restart: from the pushes enqueued after it session i is decoded by `set`, and no
// window that starts before sample `pos` is answered.  One thread, its values by argument.  An
// each-group passes its positions and pos = 0: the session's count starts again.
__global__ void k_stream_restart(long long* __restrict__ origin, int* __restrict__ set_of, int i, long long pos, int set) {
  origin[i] = pos;
  set_of[i] = set;
}

}  // namespace stream
}  // namespace mib
