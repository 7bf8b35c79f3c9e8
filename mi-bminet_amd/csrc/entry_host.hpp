// entry_host.hpp — the HIP-free argument arithmetic of the entries that take a caller's size_t to the
// kernels' 32-bit buffer offsets and int item indices (include/mibminet.h): the float scale's
// domain, the strides and counts of the windows entries, the onset list of many recordings
// (net_windows_multi_onsets), and the argument checks the windows and epochs entries share between the
// loaded set and a bank, each with the launch geometry it has validated.  Also the two types those
// checks hand to the kernels' side, under the namespaces the kernels know them by.  HIP-free like
// params_host.hpp, so it also builds into a stand-alone host program (tests/entry_host_main.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/mibminet.h"
#include "params_host.hpp"

namespace mib {

constexpr int MAX_DEVICES = 64;

namespace gen {
// TM [t][c] int8, CT [c][t] int8, F32 [c][t] float32, F32TM [t][c] float32 (element (t, c) at float
// index t C + c: frames as an amplifier delivers them).  3 is the carve's "no staging" code
// (image_layout.hpp, carve_of), no layout.
enum Layout { TM = 0, CT = 1, F32 = 2, F32TM = 4 };
constexpr bool is_float(int layout) { return layout == F32 || layout == F32TM; }
constexpr bool is_time_major(int layout) { return layout == TM || layout == F32TM; }
constexpr unsigned elem_bytes(int layout) { return is_float(layout) ? 4u : 1u; }
// the layout of a float32 entry: channel-major unless its caller names F32TM
constexpr int float_layout(int arg_layout) { return arg_layout == F32TM ? (int)F32TM : (int)F32; }
}  // namespace gen

namespace ep {
// The loaded network's channel -> source row table, a by-value kernel argument (forward_ep.hpp).
struct ChanTab {
  int c[64];
};
}  // namespace ep

// RN(1 / scale) of the float32 entries: IEEE division on the host (0: an int8 entry)
inline float recip_scale(float qs) { return qs > 0.0f ? 1.0f / qs : 0.0f; }

// The scale of a float32 entry.  The in-kernel quotient correction stays exact while its products
// are normal floats: scales in [2^-60, 2^60] (checked on every float32 input,
// tests/test_gpu_f32.py); others: the two-pass quantiser (net_quantize_input_f32), which divides.
inline int check_scale(float qs) {
  if (!(qs > 0.0f && qs <= 3.4e38f)) return NET_ERR_INVALID;
  return qs >= 0x1p-60f && qs <= 0x1p60f ? NET_OK : NET_ERR_RANGE;
}

// The feature buffer of a _feat entry (DEVICE [items][16][T64] int8): there where there are items,
// and 16-byte aligned, because an item's 16 T64 bytes leave the kernel in 16-byte pieces.
inline int check_feat(size_t items, const void* feat) {
  return (items && !feat) || ((uintptr_t)feat & 15) != 0 ? NET_ERR_INVALID : NET_OK;
}

inline size_t trial_stride(const Dims& d) { return ((size_t)d.C * d.T + 15) / 16 * 16; }

// ---- sliding windows over a recording (forward_win.hpp) --------------------------------------
inline size_t windows_row_stride(size_t L) { return L > SIZE_MAX - 15 ? 0 : (L + 15) / 16 * 16; }

// the windows of T samples at every hop-th sample of L
inline size_t windows_count(size_t T, size_t L, size_t hop) { return hop == 0 || L < T ? 0 : (L - T) / hop + 1; }

inline size_t windows_workspace(size_t L) {
  const size_t rs = windows_row_stride(L);
  return rs > SIZE_MAX / 16 ? 0 : 16 * rs;
}

// The sliding windows of R recordings laid end to end (lengths[r] samples each) for a network of T
// samples: recording r, at sample s_r = the sum of the lengths before it, contributes the onsets
// s_r + k hop, k < windows_count(T, lengths[r], hop).  Returns their number W (0 on an error, writing
// nothing); fills onsets if cap >= W and first[0 .. R] (each recording's first index, first[R] = W)
// if non-null.
inline size_t windows_multi(size_t T, const size_t* lengths, size_t R, size_t hop, int64_t* onsets, size_t cap,
                            size_t* first) {
  if (hop == 0 || (R && !lengths)) return 0;
  size_t sum = 0, W = 0;  // W <= sum
  for (size_t r = 0; r < R; r++) {
    if (lengths[r] > (size_t)INT64_MAX - sum) return 0;  // the onsets are int64
    sum += lengths[r];
    W += windows_count(T, lengths[r], hop);
  }
  const bool fill = onsets && cap >= W;
  size_t start = 0, i = 0;
  for (size_t r = 0; r < R; r++) {
    if (first) first[r] = i;
    const size_t n = windows_count(T, lengths[r], hop);
    if (fill)
      for (size_t k = 0; k < n; k++) onsets[i + k] = (int64_t)(start + k * hop);
    i += n;
    start += lengths[r];
  }
  if (first) first[R] = W;
  return W;
}

// The argument checks the windows entries share (the loaded set's and a bank's), in their
// documented order, for a network of C channels and T samples.  arg_layout: the int8 entries' layout
// argument (0 time-major, 1 channel-major); f32: a float32 entry (channel-major; time-major for the
// _f32_tm entries, which pass gen::F32TM as arg_layout: gen::float_layout).  at: false, the
// windows at every hop-th sample (onsets, W_at and n_bad unused); true, the W_at windows at the
// device list onsets (hop unused).  nw1: the 16-sample blocks a layer-1 workgroup takes per step
// (win::NW1).  On NET_OK what the launches take: the gen::Layout, W and the geometry of L.
struct WindowsGeom {
  int layout;
  size_t W;
  int rs;          // windows_row_stride(L)
  size_t blocks;   // 16-sample blocks of the recording
  size_t wgs;      // layer-1 workgroups of nw1 blocks
  long long last;  // L - T, the largest valid onset (0 when L < T: then W == 0 and nothing is launched)
};
inline int check_windows(int C, int T, const void* x, int arg_layout, bool f32, size_t L, bool at, size_t hop,
                         const int64_t* onsets, size_t W_at, const int8_t* y, const int32_t* n_bad, const void* ws,
                         size_t ws_bytes, int device, int nw1, WindowsGeom& g) {
  if ((!at && hop == 0) || (!f32 && arg_layout != 0 && arg_layout != 1)) return NET_ERR_INVALID;
  const int layout = f32 ? gen::float_layout(arg_layout) : arg_layout;  // gen::Layout
  const size_t W = at ? W_at : windows_count((size_t)T, L, hop);
  if (W && (!x || !y || !ws || (at && !onsets))) return NET_ERR_INVALID;
  if (((uintptr_t)y & 3) != 0 || (gen::is_float(layout) && ((uintptr_t)x & 3) != 0)) return NET_ERR_INVALID;
  if (at && (((uintptr_t)n_bad & 3) != 0 || ((uintptr_t)onsets & 7) != 0)) return NET_ERR_INVALID;
  if (L > SIZE_MAX / 32) return NET_ERR_INVALID;  // (far past the offset limit below; 16 rs cannot wrap)
  const size_t rs = windows_row_stride(L);
  if (((uintptr_t)ws & 15) != 0 || ws_bytes < 16 * rs) return NET_ERR_INVALID;
  if (at && W && L < (size_t)T) return NET_ERR_INVALID;  // no onset can be valid
  if (device < 0 || device >= MAX_DEVICES) return NET_ERR_INVALID;
  // window indices are int in the kernel: w + gridDim.x (grid <= 2 per CU) must not wrap
  if (W > (size_t)INT32_MAX - 65535) return NET_ERR_INVALID;
  // the recording and the workspace are each one buffer view with 32-bit offsets
  const size_t per = std::max((size_t)16, (size_t)C * gen::elem_bytes(layout));
  if (L > (((size_t)1 << 31) - 1) / per) return NET_ERR_INVALID;
  g.layout = layout;
  g.W = W;
  g.rs = (int)rs;  // rs <= L + 15 < 2^27 + 15
  g.blocks = rs / 16;
  g.wgs = (g.blocks + (size_t)nw1 - 1) / (size_t)nw1;
  g.last = L < (size_t)T ? 0 : (long long)(L - (size_t)T);
  return NET_OK;
}

// ---- epochs cut out of a wider array (forward_ep.hpp) -----------------------------------------
// The argument checks both epochs entries share (the loaded set's and a bank's), in their documented
// order, for a network of C channels and T samples; on NET_OK what the kernels take of the geometry.
struct EpochGeom {
  ep::ChanTab tab;
  long long last;       // n_elems - span, the largest valid onset
  unsigned span_bytes;
};
inline int check_epochs(int C, int T, const void* x, bool f32, size_t n_elems, size_t row_stride,
                        const int32_t* channels, const int64_t* onsets, size_t E, const int8_t* y,
                        const int32_t* n_bad, int device, EpochGeom& g) {
  if (E && (!x || !y || !onsets)) return NET_ERR_INVALID;
  if (((uintptr_t)y & 3) != 0 || ((uintptr_t)n_bad & 3) != 0 || ((uintptr_t)onsets & 7) != 0) return NET_ERR_INVALID;
  if (f32 && ((uintptr_t)x & 3) != 0) return NET_ERR_INVALID;
  if (row_stride == 0) return NET_ERR_INVALID;
  size_t cmax = (size_t)C - 1;  // channels == NULL: rows 0 .. C - 1
  if (channels) {
    cmax = 0;
    for (int c = 0; c < C; c++) {
      if (channels[c] < 0) return NET_ERR_INVALID;
      cmax = std::max(cmax, (size_t)channels[c]);
    }
  }
  // span = max(channels) row_stride + T elements, inside the source
  if (cmax && row_stride > (SIZE_MAX - (size_t)T) / cmax) return NET_ERR_INVALID;
  const size_t span = cmax * row_stride + (size_t)T;
  if (span > n_elems) return NET_ERR_INVALID;
  // each epoch is one buffer view with 32-bit offsets (delta <= 3 and the dword rounding on top)
  const size_t esz = f32 ? sizeof(float) : 1;
  if (span > (((size_t)1 << 31) - 7) / esz) return NET_ERR_INVALID;
  // epoch indices are int in the kernel: e + gridDim.x (grid <= 2 per CU) must not wrap
  if (E > (size_t)INT32_MAX - 65535) return NET_ERR_INVALID;
  if (device < 0 || device >= MAX_DEVICES) return NET_ERR_INVALID;
  for (int c = 0; c < 64; c++) g.tab.c[c] = c < C ? (channels ? channels[c] : c) : 0;
  g.last = (long long)std::min(n_elems - span, (size_t)INT64_MAX);
  g.span_bytes = (unsigned)(esz * span);
  return NET_OK;
}

}  // namespace mib
