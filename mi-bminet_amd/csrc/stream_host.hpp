// stream_host.hpp — the HIP-free part of a stream group (net_streams_create, include/mibminet.h):
// the size of a session's layer-1 ring, the arithmetic of one push (which windows of the global grid
// o = j hop end in it, where they and the new samples lie in the ring, how many items the two
// kernels take) and the argument checks of create and push.  HIP-free like entry_host.hpp, whose
// windows_count it uses: included by mibminet.hip and a stand-alone host program
// (tests/stream_host_main.cpp).
//
// The ring.  A session's ring holds the layer-1 output of its last cap samples, sample t at position
// t mod cap (and again at t mod cap + cap, forward_stream.hpp).  A push of n samples at position p0
// (the samples p0 .. p0 + n - 1) overwrites the positions of samples p0 - cap .. p0 + n - 1 - cap.  The
// windows it completes are those whose last sample lies in p0 .. p0 + n - 1, so the earliest sample
// any of them reads is p0 - T + 1.  That sample survives the push iff p0 - T + 1 > p0 + n - 1 - cap,
// i.e. cap >= T + n - 1.  cap = 16 ceil((T + max_push) / 16) >= T + max_push > T + n - 1 for every
// n <= max_push.
#pragma once
#include <cstddef>
#include <cstdint>

#include "entry_host.hpp"  // windows_count, MAX_DEVICES

namespace mib {
namespace stream {

constexpr size_t MAX_PUSH = 65536;                     // samples per session and push
constexpr size_t MAX_ITEMS = (size_t)INT32_MAX - 65535;  // item indices are int in the kernels

// samples of a session's ring for a network of T samples; 0: max_push outside 1 .. MAX_PUSH
inline size_t ring_samples(size_t T, size_t max_push) {
  return max_push < 1 || max_push > MAX_PUSH ? 0 : (T + max_push + 15) / 16 * 16;
}

// the windows of the global grid whose last sample is one of pos .. pos + n - 1; 0 for hop == 0 or
// when pos + n overflows
inline size_t push_windows(size_t T, size_t hop, uint64_t pos, size_t n) {
  if (hop == 0 || (uint64_t)n > UINT64_MAX - pos) return 0;
  return windows_count(T, (size_t)(pos + n), hop) - windows_count(T, (size_t)pos, hop);
}

// ---- create ---------------------------------------------------------------------------------
// sets: S host entries or null (set 0).  NET_ERR_INVALID before any device call for: no bank or no
// out, S == 0, hop == 0, max_push outside 1 .. MAX_PUSH, a set outside the bank, S max_push >
// MAX_ITEMS (then neither kernel's item count, S k <= S n and S ceil(n / 16), can pass it) and a
// bad device.
inline int check_create(bool have_bank, size_t n_sets, const int32_t* sets, size_t S, size_t hop, size_t max_push,
                        int device, bool have_out) {
  if (!have_bank || !have_out || S == 0 || hop == 0) return NET_ERR_INVALID;
  if (max_push < 1 || max_push > MAX_PUSH) return NET_ERR_INVALID;
  if (S > MAX_ITEMS / max_push) return NET_ERR_INVALID;
  if (device < 0 || device >= MAX_DEVICES) return NET_ERR_INVALID;
  if (sets)
    for (size_t i = 0; i < S; i++)
      if (sets[i] < 0 || (size_t)sets[i] >= n_sets) return NET_ERR_INVALID;
  return NET_OK;
}

// bytes of a group's one allocation: the rings [S][16][2 cap], then origin int64[S], then set
// int32[S] (the rings' size is a multiple of 512, so both arrays are aligned)
struct Alloc {
  size_t ring, origin, set, bytes;  // bytes per session's ring; offsets of the arrays; the total
};
inline Alloc alloc_of(size_t S, size_t cap) {
  Alloc a;
  a.ring = 32 * cap;  // S 32 cap < 2^31 2^22: no wrap
  a.origin = S * a.ring;
  a.set = a.origin + 8 * S;
  a.bytes = a.set + 4 * S;
  return a;
}

// ---- push -----------------------------------------------------------------------------------
// What one push of n samples at position pos hands to the kernels.
struct Push {
  size_t k;          // windows per session that end in this push
  uint64_t W0;       // the global index of the first of them
  long long first;   // its onset W0 hop (0 when k == 0: unused, and W0 hop may not fit then)
  long long hop;     // the hop as the kernel takes it (j hop < n for every j < k)
  int first_mod;     // first mod cap
  int p0;            // pos mod cap: where the first new sample goes
  size_t blocks;     // 16-sample blocks of a session's chunk
  size_t l1_items;   // S blocks
  size_t items;      // S k
};

// f32: the float entry; have_scales: the bank's.  The checks in their documented order; n == 0 is
// NET_OK with nothing to do (the caller returns before it looks at g).  A window that ends in this
// push has its onset in pos + n - T - (n - 1) .. pos + n - T, so every onset is below 2^63 once
// pos + n is, and the onsets of one push lie less than n <= 65,536 apart.
inline int check_push(size_t T, size_t S, size_t hop, size_t max_push, size_t cap, uint64_t pos, const void* x,
                      int layout, bool f32, bool have_scales, size_t n, const void* y, const void* n_bad, Push& g) {
  if (n == 0) return NET_OK;
  if (n > max_push) return NET_ERR_INVALID;
  if (!f32 && layout != 0 && layout != 1) return NET_ERR_INVALID;
  if (!x || (f32 && ((uintptr_t)x & 3) != 0)) return NET_ERR_INVALID;
  if (f32 && !have_scales) return NET_ERR_INVALID;
  if (pos > (uint64_t)INT64_MAX - n) return NET_ERR_INVALID;  // the onsets and origins are int64
  const size_t k = push_windows(T, hop, pos, n);
  if (k && (!y || ((uintptr_t)y & 3) != 0)) return NET_ERR_INVALID;
  if (((uintptr_t)n_bad & 3) != 0) return NET_ERR_INVALID;
  g.k = k;
  g.W0 = windows_count(T, (size_t)pos, hop);
  g.first = k ? (long long)(g.W0 * hop) : 0;
  g.hop = (long long)std::min(hop, (size_t)INT64_MAX);  // hop > n: k <= 1 and j hop = 0
  g.first_mod = (int)((uint64_t)g.first % cap);
  g.p0 = (int)(pos % cap);
  g.blocks = (n + 15) / 16;
  g.l1_items = S * g.blocks;  // <= S max_push <= MAX_ITEMS
  g.items = S * k;            // k <= n
  return NET_OK;
}

}  // namespace stream
}  // namespace mib
