// stream_host.hpp — the HIP-free part of a stream group (net_streams_create, include/mibminet.h):
// the size of a session's layer-1 ring, the arithmetic of one push (which windows of the global grid
// o = j hop end in it, where they and the new samples lie in the ring, how many items the two
// kernels take) and the argument checks of create and push; for an each-group, whose sessions have
// a position each, the per-session plan of a push (plan_each, shared with the plan kernel of
// forward_stream.hpp), the rows of its logits, its allocation and its checks; for a query
// (net_streams_windows_at) which windows a ring still holds and where (at_item, shared with
// k_forward_ring_at), the span and the checks; for a group with a decimator
// (net_streams_set_decimator) the samples a raw push completes, the history's size and slots and
// the checks and plan of a raw push; for an each-group with a decimator
// (net_streams_set_decimator_each) the per-session plan of a raw push (plan_each_raw, shared with its
// plan kernel), its allocation and its checks; for a prefilter (net_streams_set_prefilter) the
// sections as the kernel takes them, the checks and the allocation; for the test hook that places a
// fresh group at a position (mibminet_test_streams_seek) its checks.  HIP-free like entry_host.hpp,
// whose windows_count it uses: included by mibminet.hip, forward_stream.hpp and six stand-alone host
// programs (tests/stream_host_main.cpp, tests/stream_each_host_main.cpp, tests/stream_at_host_main.cpp,
// tests/decim_host_main.cpp, tests/decim_each_host_main.cpp, tests/prefilter_host_main.cpp).
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

#include "entry_host.hpp"    // windows_count, MAX_DEVICES
#include "image_layout.hpp"  // MIB_HD

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

// ---- each-groups: a position per session, on the device ---------------------------------------
// An each-group (net_streams_create_each) keeps pos[s] (int64, the samples session s was given since
// creation or its last restart) in device memory, and a push hands session s cnt[s] <= n_max samples
// of its own.  What the kernels need of a session and push is one record, computed by one thread of
// k_stream_plan (forward_stream.hpp) with plan_each below; the host tests run the same function
// (tests/stream_each_host_main.cpp), as image_layout.hpp and bank_host.hpp's range_of are shared.

// the most windows a session can complete in a push of at most n_max samples: ceil(n_max / hop).
// (The windows that end in n consecutive samples end hop apart.)  0: hop == 0 or n_max outside
// 1 .. MAX_PUSH.
inline size_t each_rows(size_t hop, size_t n_max) {
  if (hop == 0 || n_max < 1 || n_max > MAX_PUSH) return 0;
  return n_max / hop + (n_max % hop != 0);
}

// a position may not pass this: every onset and pos + n stay int64 without a check on the host
constexpr long long EACH_POS_LIMIT = INT64_MAX - 65536;

// One session's record of one push, as the layer-1 and the window kernel read it (16 bytes, one
// scalar load): n samples go to ring positions p0, p0 + 1, ... mod cap; k windows are completed, the
// first read from ring position at0, the next ones hop further each.
struct EachRec {
  int n, p0, k, at0;
};
struct EachPlan {
  EachRec rec;
  long long W0;  // the index on the session's grid of its first window of this push
  bool ok;       // false: the count was refused (n = k = 0, nothing stored, the position stays)
};

// windows_count (entry_host.hpp) for a device caller; hop >= 1
MIB_HD inline unsigned long long each_count(unsigned long long T, unsigned long long L, unsigned long long hop) {
  return L < T ? 0 : (L - T) / hop + 1;
}

// The plan of a session at position pos (0 <= pos <= EACH_POS_LIMIT) that is handed cnt samples of
// a push of at most n_max (<= max_push <= cap - T).  cnt is compared unsigned before anything is
// formed from it; a count outside 0 .. n_max, or one that would take the position past
// EACH_POS_LIMIT, is refused.  k <= ceil(cnt / hop) <= each_rows(hop, n_max); W0 hop + T <= pos + cnt
// where k > 0, so the onset fits; with k == 0 at0 is 0 (unused, and W0 hop may not fit).
MIB_HD inline EachPlan plan_each(unsigned T, unsigned long long hop, unsigned cap, long long pos, int cnt,
                                 unsigned n_max) {
  EachPlan e;
  const unsigned long long p = (unsigned long long)pos;
  e.W0 = (long long)each_count(T, p, hop);
  e.ok = (unsigned)cnt <= n_max && pos <= EACH_POS_LIMIT - (long long)(unsigned)cnt;
  e.rec.p0 = (int)(p % cap);
  e.rec.n = e.ok ? cnt : 0;
  e.rec.k = (int)(each_count(T, p + (unsigned)e.rec.n, hop) - (unsigned long long)e.W0);
  e.rec.at0 = e.rec.k ? (int)((unsigned long long)e.W0 * hop % cap) : 0;
  return e;
}

// bytes of an each-group's one allocation: a uniform group's (the origins stay zero and unread),
// then the records EachRec[S] at a multiple of 16 and the positions int64[S]
struct AllocEach {
  Alloc base;
  size_t plan, pos, bytes;
};
inline AllocEach alloc_each(size_t S, size_t cap) {
  AllocEach a;
  a.base = alloc_of(S, cap);
  a.plan = (a.base.bytes + 15) / 16 * 16;
  a.pos = a.plan + sizeof(EachRec) * S;
  a.bytes = a.pos + 8 * S;
  return a;
}

// What one push of an each-group hands to the kernels.
struct PushEach {
  size_t kmax;      // rows of y per session: each_rows(hop, n_max)
  int hop;          // the hop as the kernel takes it (j hop < n_max + hop for every j < kmax)
  size_t blocks;    // 16-sample blocks of a session's slot
  size_t l1_items;  // S blocks
  size_t items;     // S kmax
};

// The checks of net_streams_push_each[_f32] in their documented order (the group itself, NULL or
// uniform, is the caller's first check).  kmax <= n_max <= max_push, so both item counts are at most
// S max_push <= MAX_ITEMS (check_create).
inline int check_push_each(size_t S, size_t hop, size_t max_push, const void* x, int layout, bool f32, bool have_scales,
                           const void* cnt_in, size_t n_max, const void* y, const void* cnt_out, const void* win0,
                           const void* n_bad, PushEach& g) {
  if (n_max < 1 || n_max > max_push) return NET_ERR_INVALID;
  if (!f32 && layout != 0 && layout != 1) return NET_ERR_INVALID;
  if (!x || !cnt_in || !y || !cnt_out) return NET_ERR_INVALID;
  if (((uintptr_t)y & 3) != 0 || ((uintptr_t)cnt_in & 3) != 0 || ((uintptr_t)cnt_out & 3) != 0 ||
      ((uintptr_t)win0 & 7) != 0 || ((uintptr_t)n_bad & 3) != 0 || (f32 && ((uintptr_t)x & 3) != 0))
    return NET_ERR_INVALID;
  if (f32 && !have_scales) return NET_ERR_INVALID;
  g.kmax = each_rows(hop, n_max);
  g.hop = (int)std::min(hop, MAX_PUSH);  // hop > n_max: kmax = 1 and j hop = 0
  g.blocks = (n_max + 15) / 16;
  g.l1_items = S * g.blocks;
  g.items = S * g.kmax;
  return NET_OK;
}

// ---- windows at given onsets (net_streams_windows_at) -----------------------------------------
// A query asks for the window of a session whose first sample is o, read from the ring as it is.
// With pos the session's position (0 <= pos <= INT64_MAX) and lo the first sample a window of it may
// read (its origin, >= 0; 0 for an each-group), the window is there iff o >= lo and
// T <= pos - o <= cap: complete, and its first sample not yet overwritten.
//
// Retention.  A window completes in the push that takes pos to o + T or beyond.  That push had
// n <= max_push samples and started below o + T, so right after it pos - o < T + n <= T + max_push
// <= cap: a query enqueued after the push that completes a window always finds it, and the window
// stays for cap - (pos - o) more samples.

// What a valid query reads: d = pos - o, in T .. cap.
struct AtItem {
  bool valid;
  unsigned d;
};

// The predicate, shared by k_forward_ring_at and the host (tests/stream_at_host_main.cpp).  In 64
// bits, in a form that cannot overflow: o >= 0 first, then o <= pos, then the difference of two
// non-negative values, compared unsigned with T and cap.  A value whose low 32 bits alone would pass
// fails.  pos < 0 (no session has one) fails every o.
MIB_HD inline AtItem at_item(long long o, long long lo, long long pos, unsigned T, unsigned cap) {
  if (o < 0 || o < lo || o > pos) return AtItem{false, 0};
  const unsigned long long d = (unsigned long long)pos - (unsigned long long)o;
  if (d < T || d > cap) return AtItem{false, 0};
  return AtItem{true, (unsigned)d};
}

// The ring position of the first byte of a valid query, (pos mod cap - d) mod cap: pos_mod < cap and
// T <= d <= cap, so the difference is in -cap .. cap - 1 and one conditional correction does.
MIB_HD inline int at_ring(int pos_mod, unsigned d, int cap) {
  const int at = pos_mod - (int)d;
  return at < 0 ? at + cap : at;
}

// net_streams_at_span on a uniform group at position pos: the onsets lo .. hi have their window in
// the ring (hi < lo: none yet); a session's origin applies on top.
inline void at_span(size_t T, size_t cap, uint64_t pos, int64_t* lo, int64_t* hi) {
  *lo = pos > cap ? (int64_t)(pos - cap) : 0;
  *hi = (int64_t)pos - (int64_t)T;  // pos <= INT64_MAX (check_push), T < 2^31
}

// The checks of net_streams_windows_at in their documented order; W == 0 is NET_OK with nothing to
// do (the caller returns before it looks further).  A uniform group's capturing stream comes after
// them.
inline int check_windows_at(bool have_group, size_t W, const void* session, const void* onsets, const void* y,
                            const void* n_bad) {
  if (!have_group) return NET_ERR_INVALID;
  if (W == 0) return NET_OK;
  if (W > MAX_ITEMS) return NET_ERR_INVALID;
  if (!session || !onsets || !y) return NET_ERR_INVALID;
  if (((uintptr_t)session & 3) != 0 || ((uintptr_t)onsets & 7) != 0 || ((uintptr_t)y & 3) != 0 ||
      ((uintptr_t)n_bad & 3) != 0)
    return NET_ERR_INVALID;
  return NET_OK;
}

// ---- a decimator: raw frames at q times the network's rate (net_streams_set_decimator) ------------
// A uniform group with a decimator is pushed raw float32 frames [n_raw][R] per session.  With P the
// raw frames a session was given so far, decimated sample d (the FIR of raw frames q d - K + 1 .. q d)
// exists once frame q d has arrived: D(P) = ceil(P / q) samples, and a push of n_raw frames at P adds
// m = D(P + n_raw) - D(P).  The group's position (the ring's, the windows', the origins') stays on the
// decimated axis, pos = D(P).
//
// The history.  A session's last K - 1 raw frames live in device memory, frame a at slot
// a mod (K - 1): slots that no frame has reached yet hold zeros, which is what the frames a < 0 are.
// Relative to the chunk's first frame P, output sample j of the push (d = D(P) + j) reads the frames
// rel = q j + off - k, k = 0 .. K - 1, off = q D(P) - P in 0 .. q - 1: the chunk's frame rel where
// rel >= 0, else the history's slot (slot0 + rel) mod (K - 1) with slot0 = P mod (K - 1) and
// rel >= -(K - 1), one conditional addition.

constexpr size_t MAX_Q = 16;      // the decimation factor
constexpr size_t MAX_TAPS = 128;  // K

// D(P); P / q + 1 cannot wrap for q >= 1
inline uint64_t raw_decimated(size_t q, uint64_t P) { return P / q + (P % q != 0); }

// m: the decimated samples a push of n_raw frames at raw position raw_pos completes; 0 for q == 0 or
// when raw_pos + n_raw overflows
inline size_t raw_samples(size_t q, uint64_t raw_pos, size_t n_raw) {
  if (q == 0 || (uint64_t)n_raw > UINT64_MAX - raw_pos) return 0;
  return (size_t)(raw_decimated(q, raw_pos + n_raw) - raw_decimated(q, raw_pos));
}

// the history slot of raw frame a (K >= 2)
inline size_t hist_slot(uint64_t a, size_t K) { return (size_t)(a % (K - 1)); }

// bytes of a decimator's one allocation: the taps float[K], then at a multiple of 16 the histories
// [S][K - 1][R] float (R <= 64, K <= 128, S < 2^31: below 2^46)
struct AllocDecim {
  size_t taps, hist, per, bytes;  // offsets of the two; bytes per session's history; the total
};
inline AllocDecim alloc_decim(size_t S, size_t R, size_t K) {
  AllocDecim a;
  a.taps = 0;
  a.hist = (4 * K + 15) / 16 * 16;
  a.per = 4 * (K - 1) * R;
  a.bytes = a.hist + S * a.per;
  return a;
}

inline bool finite_f32(float v) { return v - v == 0.0f; }  // false for NaN and the infinities

// The checks of net_streams_set_decimator before its capturing stream's, in their documented order.
// pushed: the group has taken a push; have_decim: it has a decimator already.
inline int check_set_decimator(bool have_group, bool each, bool have_scales, bool have_decim, bool pushed, size_t q,
                               const float* taps, size_t K) {
  if (!have_group) return NET_ERR_INVALID;
  if (each) return NET_ERR_UNSUPPORTED;
  if (have_decim || pushed) return NET_ERR_INVALID;
  if (q < 1 || q > MAX_Q || K < 1 || K > MAX_TAPS || !taps) return NET_ERR_INVALID;
  for (size_t k = 0; k < K; k++)
    if (!finite_f32(taps[k])) return NET_ERR_INVALID;
  if (!have_scales) return NET_ERR_INVALID;
  return NET_OK;
}

// What one raw push of n_raw frames at raw position P hands to the kernels.
struct PushRaw {
  size_t m;             // decimated samples completed
  uint64_t d0;          // D(P): the decimated position, the first new sample
  int off;              // q d0 - P, in 0 .. q - 1: the chunk's frame that sample d0 ends in
  int slot0;            // P mod (K - 1), the history's slot of the chunk's first frame (K == 1: 0)
  size_t keep;          // min(n_raw, K - 1): the chunk's last frames that go to the history
  size_t hist_items;    // S keep R: the floats the history kernel copies
  Push push;            // check_push's plan of the m samples at d0 (m > 0)
};

// The checks of net_streams_push_raw_f32_tm in check_push's order, all before anything is enqueued;
// n_raw == 0 is NET_OK with nothing to do (the caller returns before it looks at g).  d0 <= P and
// m <= ceil(n_raw / q) <= max_push, so the decimated position passes INT64_MAX only if the raw one
// does.  m == 0 is legal (k == 0, y unread): only the history moves.
inline int check_push_raw(size_t T, size_t S, size_t R, size_t hop, size_t max_push, size_t cap, size_t q, size_t K,
                          uint64_t raw_pos, const void* x, bool have_scales, size_t n_raw, const void* y,
                          const void* n_bad, PushRaw& g) {
  if (n_raw == 0) return NET_OK;
  if (n_raw > q * max_push) return NET_ERR_INVALID;  // q max_push <= 2^20
  if (!x || ((uintptr_t)x & 3) != 0) return NET_ERR_INVALID;
  if (!have_scales) return NET_ERR_INVALID;
  if (raw_pos > (uint64_t)INT64_MAX - n_raw) return NET_ERR_INVALID;
  const size_t m = raw_samples(q, raw_pos, n_raw);
  const uint64_t d0 = raw_decimated(q, raw_pos);
  const size_t k = push_windows(T, hop, d0, m);
  if (k && (!y || ((uintptr_t)y & 3) != 0)) return NET_ERR_INVALID;
  if (((uintptr_t)n_bad & 3) != 0) return NET_ERR_INVALID;
  Push p{};
  if (m)
    if (const int rc = check_push(T, S, hop, max_push, cap, d0, x, 0, true, have_scales, m, y, n_bad, p)) return rc;
  g.m = m;
  g.d0 = d0;
  g.off = (int)(raw_pos % q == 0 ? 0 : q - raw_pos % q);  // q d0 - P without the product
  g.slot0 = K > 1 ? (int)hist_slot(raw_pos, K) : 0;
  g.keep = n_raw < K - 1 ? n_raw : K - 1;
  g.hist_items = S * g.keep * R;  // S < 2^31, keep < 2^7, R <= 2^6
  g.push = p;
  return NET_OK;
}

// ---- an each-group's decimator (net_streams_set_decimator_each) -----------------------------------
// Every session has its own raw position P[s] (int64, device memory) beside its decimated position
// pos[s] = D(P[s]), its own phase off = q D(P) - P and its own history slot: the plan of a raw push
// is made per session on the device (k_stream_plan_raw, forward_stream.hpp) with plan_each_raw
// below, which the host tests run too (tests/decim_each_host_main.cpp).

// a raw position may not pass this: a count is at most q MAX_PUSH <= 2^20, so P + cnt and D(P) stay
// int64 without a check on the host, and D(P) + m <= P + cnt stays below EACH_POS_LIMIT
constexpr long long EACH_RAW_LIMIT = INT64_MAX - (1ll << 20);
static_assert(MAX_Q * MAX_PUSH <= (1u << 20) && EACH_RAW_LIMIT <= EACH_POS_LIMIT, "the raw limit covers every count");

// rows of y per session of a raw push of at most n_raw_max frames: each_rows(hop, ceil(n_raw_max / q));
// 0 for hop == 0, q outside 1 .. MAX_Q or ceil(n_raw_max / q) outside 1 .. MAX_PUSH
inline size_t each_raw_rows(size_t hop, size_t q, size_t n_raw_max) {
  if (q < 1 || q > MAX_Q) return 0;
  return each_rows(hop, n_raw_max / q + (n_raw_max % q != 0));
}

// The raw part of a session's record of one raw push (16 bytes, one scalar load), beside its EachRec:
// the first n_raw frames of its slot are new, output sample j reads the frames q j + off - k of the
// slot, the slot's first frame has history slot slot0, and the slot's last keep frames go to the
// history.
struct RawRec {
  int n_raw, off, slot0, keep;
};
struct EachRawPlan {
  EachPlan each;  // plan_each of the m decimated samples at D(P); ok: the raw count's verdict
  RawRec raw;
  int m;          // the decimated samples the count completes
};

// The plan of a session at raw position P (0 <= P <= EACH_RAW_LIMIT) that is handed cnt frames of a
// raw push of at most n_raw_max (<= q max_push), under factor q in 1 .. MAX_Q and K in 1 .. MAX_TAPS
// taps.  cnt is compared unsigned before anything is formed from it; a count outside 0 .. n_raw_max,
// or one that would take P past EACH_RAW_LIMIT, is refused: n_raw = m = k = keep = 0, nothing is
// stored and neither position moves.  m = D(P + cnt) - D(P) <= ceil(cnt / q) <= ceil(n_raw_max / q);
// where m > 0, q (m - 1) + off = q (D(P + cnt) - 1) - P <= cnt - 1: no answered sample reads a frame
// at or past cnt.
MIB_HD inline EachRawPlan plan_each_raw(unsigned T, unsigned long long hop, unsigned cap, unsigned q, unsigned K,
                                        long long P, int cnt, unsigned n_raw_max) {
  EachRawPlan e;
  const bool ok = (unsigned)cnt <= n_raw_max && P <= EACH_RAW_LIMIT - (long long)(unsigned)cnt;
  const unsigned n = ok ? (unsigned)cnt : 0u;
  const unsigned long long p = (unsigned long long)P, p1 = p + n;
  const unsigned long long d0 = p / q + (p % q != 0), d1 = p1 / q + (p1 % q != 0);
  e.m = (int)(d1 - d0);
  e.raw.n_raw = (int)n;
  e.raw.off = (int)(p % q == 0 ? 0 : q - p % q);
  e.raw.slot0 = K > 1 ? (int)(p % (K - 1)) : 0;
  e.raw.keep = (int)(n < K - 1 ? n : K - 1);
  e.each = plan_each(T, hop, cap, (long long)d0, e.m, n_raw_max / q + (n_raw_max % q != 0));
  e.each.ok = ok;  // (plan_each refuses nothing here: m is within its bound and D(P) + m within its limit)
  return e;
}

// bytes of an each-group's decimator's one allocation: a uniform group's (the taps, then the
// histories), then at multiples of 16 the raw positions int64[S] and the raw records RawRec[S]
struct AllocDecimEach {
  AllocDecim base;
  size_t raw_pos, rec, bytes;
};
inline AllocDecimEach alloc_decim_each(size_t S, size_t R, size_t K) {
  AllocDecimEach a;
  a.base = alloc_decim(S, R, K);
  a.raw_pos = (a.base.bytes + 15) / 16 * 16;
  a.rec = (a.raw_pos + 8 * S + 15) / 16 * 16;
  a.bytes = a.rec + sizeof(RawRec) * S;
  return a;
}

// What one raw push of an each-group hands to the kernels.
struct PushEachRaw {
  size_t n_max;       // ceil(n_raw_max / q): the most decimated samples a session completes
  size_t keep_max;    // min(n_raw_max, K - 1): the most frames a session moves to its history
  size_t hist_items;  // S keep_max R: the floats the history kernel walks
  PushEach each;      // check_push_each's plan of at most n_max samples per session
};

// The checks of net_streams_push_each_raw_f32_tm in their documented order (the group itself, NULL,
// uniform or without a decimator, is the caller's first check): n_raw_max in 1 .. q max_push, then
// those of net_streams_push_each_f32_tm, whose n_max = ceil(n_raw_max / q) is then in 1 .. max_push.
inline int check_push_each_raw(size_t S, size_t R, size_t hop, size_t max_push, size_t q, size_t K, const void* x,
                               bool have_scales, const void* cnt_in, size_t n_raw_max, const void* y,
                               const void* cnt_out, const void* win0, const void* n_bad, PushEachRaw& g) {
  if (n_raw_max < 1 || n_raw_max > q * max_push) return NET_ERR_INVALID;  // q max_push <= 2^20
  const size_t n_max = n_raw_max / q + (n_raw_max % q != 0);
  PushEach p{};
  if (const int rc = check_push_each(S, hop, max_push, x, 0, true, have_scales, cnt_in, n_max, y, cnt_out, win0, n_bad, p))
    return rc;
  g.n_max = n_max;
  g.keep_max = n_raw_max < K - 1 ? n_raw_max : K - 1;
  g.hist_items = S * g.keep_max * R;  // S < 2^31, keep_max < 2^7, R <= 2^6
  g.each = p;
  return NET_OK;
}

// ---- a fresh group placed at a position (mibminet_test_streams_seek, include/mibminet_testing.h) ----
// The test hook's checks, in their documented order.  fresh: the group has taken no push, no restart
// and no seek.  pos: S entries, raw positions on a group with a decimator (q != 0), else sample
// positions; origin: null or S entries, a uniform group's only.  An entry is refused when negative
// or, on an each-group, above the limit its plan keeps (EACH_RAW_LIMIT with a decimator, else
// EACH_POS_LIMIT; a uniform group's bound, INT64_MAX, is the type's); a uniform group's entries must
// all be equal; an origin must lie in 0 .. D(pos), D(pos) = pos without a decimator.
inline int check_seek(bool have_group, bool each, bool fresh, size_t S, size_t q, const int64_t* pos,
                      const int64_t* origin) {
  if (!have_group || !pos) return NET_ERR_INVALID;
  if (!fresh) return NET_ERR_INVALID;
  if (each && origin) return NET_ERR_INVALID;
  const int64_t limit = !each ? INT64_MAX : q ? EACH_RAW_LIMIT : EACH_POS_LIMIT;
  for (size_t s = 0; s < S; s++)
    if (pos[s] < 0 || pos[s] > limit || (!each && pos[s] != pos[0])) return NET_ERR_INVALID;
  if (origin)
    for (size_t s = 0; s < S; s++) {
      const uint64_t d = q ? raw_decimated(q, (uint64_t)pos[s]) : (uint64_t)pos[s];
      if (origin[s] < 0 || (uint64_t)origin[s] > d) return NET_ERR_INVALID;
    }
  return NET_OK;
}

// ---- a prefilter: an IIR cascade ahead of the decimator (net_streams_set_prefilter) ----------------
// A group with a decimator, uniform or each, may be given M second-order sections that every raw
// frame passes, per session and electrode, before the FIR sees it (k_prefilter, forward_stream.hpp).
// The group owns the states [S][M][2][R] float32 (z1 then z2 of a section, a session's contiguous)
// and a scratch [S][q max_push][R] float32 that holds the filtered frames of one push.

constexpr size_t MAX_SECTIONS = 8;  // M

// The sections as the kernel takes them, by value in its arguments (160 bytes): {b0, b1, b2, a1, a2}
// of section j, a0 = 1.  Rows at and past M are unread.
struct Sos {
  float c[MAX_SECTIONS][5];
};

// The checks of net_streams_set_prefilter before its capturing stream's, in their documented order.
// have_decim: the group has a decimator; pushed: it has taken a push; have_prefilter: it has a
// prefilter already.  Of the flags check_set_decimator takes, two are not taken here because they
// could decide nothing: `each` (either kind of group may have a prefilter) and `have_scales` (a group
// has a decimator only if its bank has scales).  No coefficient is read before M is known to be in
// range.
inline int check_set_prefilter(bool have_group, bool have_decim, bool have_prefilter, bool pushed, const float* sos,
                               size_t M) {
  if (!have_group) return NET_ERR_INVALID;
  if (!have_decim || have_prefilter || pushed) return NET_ERR_INVALID;
  if (M < 1 || M > MAX_SECTIONS || !sos) return NET_ERR_INVALID;
  for (size_t i = 0; i < 5 * M; i++)
    if (!finite_f32(sos[i])) return NET_ERR_INVALID;
  return NET_OK;
}

// bytes of a prefilter's one allocation: the states, then at a multiple of 256 the scratch.
// S max_push <= MAX_ITEMS < 2^31 (check_create), q <= 2^4, R <= 2^6, M <= 2^3: both products stay
// below 2^45.
struct AllocPrefilter {
  size_t state, per_state, scratch, per_scratch, bytes;  // offsets of the two, bytes per session of each, the total
};
inline AllocPrefilter alloc_prefilter(size_t S, size_t R, size_t M, size_t q, size_t max_push) {
  AllocPrefilter a;
  a.state = 0;
  a.per_state = 4 * 2 * M * R;
  a.scratch = (S * a.per_state + 255) / 256 * 256;
  a.per_scratch = 4 * q * max_push * R;
  a.bytes = a.scratch + S * a.per_scratch;
  return a;
}

}  // namespace stream
}  // namespace mib
