// entry_host_main.cpp — the entries' argument arithmetic (csrc/entry_host.hpp) as a stand-alone
// program (tests/test_host_sanitizers.py builds it with -fsanitize=address,undefined and runs it):
// check_windows, check_epochs, windows_multi and check_scale at the edges include/mibminet.h
// documents.  Every expected result is worked out here from the header's stated rule, in 128-bit
// arithmetic where a size_t product or sum could wrap, never by calling the function under test.
// The pointers handed to the checks are made-up addresses: the checks look at their alignment and
// never read through them (channels and lengths, which they do read, are real arrays of exactly the
// size asked for, so a read or write past either end is an AddressSanitizer report).
// Prints "cases <n>"; exits 0 when every check held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "entry_host.hpp"

using namespace mib;
typedef unsigned __int128 u128;

static int g_bad = 0, g_cases = 0;
#define CHECK(cond, ...) \
  do { \
    if (!(cond)) { \
      if (g_bad++ < 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    } \
  } while (0)

static const size_t IMAX = (size_t)INT64_MAX;
static const size_t WMAX = (size_t)INT32_MAX - 65535;  // the largest item count
static const int NW1 = 4;                              // win::NW1
static void* addr(uintptr_t a) { return (void*)a; }
static const uintptr_t X = 0x10000, Y = 0x20000, WS = 0x30000, ON = 0x40000, NB = 0x50000;

// ---- check_windows ----------------------------------------------------------------------------
struct WinArgs {
  int C, T;
  uintptr_t x;
  int layout;
  bool f32;
  size_t L;
  bool at;
  size_t hop;
  uintptr_t onsets;
  size_t W_at;
  uintptr_t y, n_bad, ws;
  size_t ws_bytes;
  int device;
};

static u128 round16(size_t L) { return ((u128)L + 15) / 16 * 16; }

// net_model_compute_windows[_at][_f32]'s documented refusals (all NET_ERR_INVALID; the scale and
// the loaded set are the caller's)
static int windows_rule(const WinArgs& a, size_t& W) {
  W = a.at ? a.W_at : (a.hop == 0 || a.L < (size_t)a.T ? 0 : (a.L - (size_t)a.T) / a.hop + 1);
  bool bad = (!a.at && a.hop == 0) || (!a.f32 && a.layout != 0 && a.layout != 1);
  bad = bad || (W > 0 && (!a.x || !a.y || !a.ws || (a.at && !a.onsets)));
  bad = bad || (a.y & 3) || (a.f32 && (a.x & 3)) || (a.at && ((a.n_bad & 3) || (a.onsets & 7)));
  bad = bad || (a.ws & 15) || (u128)a.ws_bytes < 16 * round16(a.L);
  bad = bad || (a.at && W > 0 && a.L < (size_t)a.T) || W > WMAX;
  const u128 per = (u128)a.C * (a.f32 ? 4 : 1);
  bad = bad || (u128)a.L * (per > 16 ? per : 16) >= ((u128)1 << 31);
  bad = bad || a.device < 0 || a.device >= 64;
  return bad ? NET_ERR_INVALID : NET_OK;
}

static void win_case(const WinArgs& a) {
  size_t W;
  const int want = windows_rule(a, W);
  WindowsGeom g;
  const int rc = check_windows(a.C, a.T, addr(a.x), a.layout, a.f32, a.L, a.at, a.hop, (const int64_t*)addr(a.onsets),
                               a.W_at, (const int8_t*)addr(a.y), (const int32_t*)addr(a.n_bad), addr(a.ws), a.ws_bytes,
                               a.device, NW1, g);
  CHECK(rc == want, "windows C %d f32 %d at %d L %zu hop %zu W %zu ws_bytes %zu: %d, want %d", a.C, (int)a.f32, (int)a.at,
        a.L, a.hop, a.W_at, a.ws_bytes, rc, want);
  if (rc == NET_OK && want == NET_OK) {
    const size_t rs = (size_t)round16(a.L), nb = rs / 16;
    CHECK(g.layout == (a.f32 ? 2 : a.layout) && g.W == W, "windows L %zu: layout %d W %zu", a.L, g.layout, g.W);
    CHECK(g.rs >= 0 && (size_t)g.rs == rs && g.blocks == nb && g.wgs == (nb + NW1 - 1) / NW1,
          "windows L %zu: rs %d blocks %zu wgs %zu", a.L, g.rs, g.blocks, g.wgs);
    CHECK(g.last == (a.L < (size_t)a.T ? 0 : (long long)(a.L - (size_t)a.T)), "windows L %zu: last %lld", a.L, g.last);
    CHECK(W == 0 || a.L >= (size_t)a.T, "windows L %zu: %zu windows of %d samples", a.L, W, a.T);
  }
  g_cases++;
}

static size_t clip(u128 v) { return v > (u128)SIZE_MAX ? SIZE_MAX : (size_t)v; }

static void windows_cases() {
  const int geom[3][2] = {{4, 64}, {22, 1125}, {64, 480}};
  for (int f32 = 0; f32 < 2; f32++)
    for (int at = 0; at < 2; at++)
      for (const auto& ct : geom) {
        const int C = ct[0], T = ct[1];
        const size_t per = std::max((size_t)16, (size_t)C * (f32 ? 4 : 1));
        const size_t lmax = (((size_t)1 << 31) - 1) / per;  // the last L with L per < 2^31
        const WinArgs base{C, T, X, 1, f32 != 0, (size_t)T + 100, at != 0, 7, ON, 5, Y, NB, WS, 0, 0};
        for (size_t L : {(size_t)0, (size_t)T - 1, (size_t)T, (size_t)T + 100, lmax - 1, lmax, lmax + 1, (size_t)1 << 31,
                         (size_t)1 << 40, SIZE_MAX / 32, SIZE_MAX / 32 + 1, SIZE_MAX - 15, SIZE_MAX}) {
          const size_t need = clip(16 * round16(L));
          for (size_t ws_bytes : {need, need - (need ? 1 : 0), SIZE_MAX}) {
            WinArgs a = base;
            a.L = L;
            a.ws_bytes = ws_bytes;
            if (at) {
              for (size_t W : {(size_t)0, (size_t)1, WMAX, WMAX + 1, SIZE_MAX}) {
                a.W_at = W;
                win_case(a);
              }
            } else {
              for (size_t hop : {(size_t)0, (size_t)1, (size_t)7, SIZE_MAX}) {
                a.hop = hop;
                win_case(a);
              }
            }
          }
        }
        // every alignment, null, layout and device refusal on a call that otherwise passes, and the
        // W == 0 passes (nothing but a large enough workspace size is needed then)
        WinArgs ok = base;
        ok.ws_bytes = clip(16 * round16(ok.L));
        win_case(ok);
        for (uintptr_t off : {1, 2, 3}) {
          WinArgs a = ok;
          a.y += off;
          win_case(a);
          a = ok;
          a.x += off;  // refused for float32 only
          win_case(a);
          a = ok;
          a.n_bad += off;  // refused at onsets only
          win_case(a);
        }
        for (uintptr_t off : {1, 4, 8, 12}) {
          WinArgs a = ok;
          a.onsets += off;  // 8: aligned again
          win_case(a);
          a = ok;
          a.ws += off;
          win_case(a);
        }
        for (int which = 0; which < 5; which++)
          for (int empty = 0; empty < 2; empty++) {
            WinArgs a = ok;
            if (empty) a.W_at = 0, a.L = (size_t)T - 1, a.ws_bytes = clip(16 * round16(a.L));
            (which == 0 ? a.x : which == 1 ? a.y : which == 2 ? a.ws : which == 3 ? a.onsets : a.n_bad) = 0;
            win_case(a);
          }
        {
          WinArgs a = ok;  // W == 0 with every pointer null
          a.W_at = 0, a.L = (size_t)T - 1, a.ws_bytes = clip(16 * round16(a.L));
          a.x = a.y = a.ws = a.onsets = a.n_bad = 0;
          win_case(a);
          a.L = 0, a.ws_bytes = 0;
          win_case(a);
        }
        for (int layout : {-1, 0, 1, 2, INT32_MAX}) {
          WinArgs a = ok;
          a.layout = layout;  // the float entry has no layout argument: ignored there
          win_case(a);
        }
        for (int device : {-1, 0, 63, 64, INT32_MIN, INT32_MAX}) {
          WinArgs a = ok;
          a.device = device;
          win_case(a);
        }
      }
}

// ---- check_epochs -----------------------------------------------------------------------------
struct EpArgs {
  int C, T;
  uintptr_t x;
  bool f32;
  size_t n_elems, row_stride;
  const std::vector<int32_t>* channels;  // null: rows 0 .. C - 1
  uintptr_t onsets;
  size_t E;
  uintptr_t y, n_bad;
  int device;
};

// net_model_compute_epochs[_f32]'s documented refusals; on NET_OK the span
static int epochs_rule(const EpArgs& a, u128& span) {
  bool bad = a.E > 0 && (!a.x || !a.y || !a.onsets);
  bad = bad || (a.y & 3) || (a.n_bad & 3) || (a.onsets & 7) || (a.f32 && (a.x & 3)) || a.row_stride == 0;
  long long cmax = a.C - 1;
  if (a.channels) {
    cmax = 0;
    for (int32_t c : *a.channels) {
      bad = bad || c < 0;
      cmax = std::max(cmax, (long long)c);
    }
  }
  if (bad) return NET_ERR_INVALID;
  span = (u128)cmax * a.row_stride + (u128)a.T;
  bad = span > (u128)SIZE_MAX || span > (u128)a.n_elems;
  bad = bad || (a.f32 ? 4 : 1) * span + 6 >= ((u128)1 << 31);
  bad = bad || a.E > WMAX || a.device < 0 || a.device >= 64;
  return bad ? NET_ERR_INVALID : NET_OK;
}

static void ep_case(const EpArgs& a) {
  u128 span = 0;
  const int want = epochs_rule(a, span);
  EpochGeom g;
  const int rc = check_epochs(a.C, a.T, addr(a.x), a.f32, a.n_elems, a.row_stride, a.channels ? a.channels->data() : nullptr,
                              (const int64_t*)addr(a.onsets), a.E, (const int8_t*)addr(a.y),
                              (const int32_t*)addr(a.n_bad), a.device, g);
  CHECK(rc == want, "epochs C %d f32 %d n %zu rs %zu E %zu: %d, want %d", a.C, (int)a.f32, a.n_elems, a.row_stride, a.E, rc,
        want);
  if (rc == NET_OK && want == NET_OK) {
    for (int c = 0; c < 64; c++)
      CHECK(g.tab.c[c] == (c < a.C ? (a.channels ? (*a.channels)[c] : c) : 0), "epochs: table entry %d = %d", c, g.tab.c[c]);
    const u128 last = (u128)a.n_elems - span;
    CHECK(g.last == (long long)(last > (u128)IMAX ? IMAX : (size_t)last), "epochs n %zu: last %lld", a.n_elems, g.last);
    CHECK((u128)g.span_bytes == (a.f32 ? 4 : 1) * span, "epochs: span_bytes %u", g.span_bytes);
  }
  g_cases++;
}

static void epochs_cases() {
  const int geom[3][2] = {{4, 64}, {22, 1125}, {64, 480}};
  for (int f32 = 0; f32 < 2; f32++)
    for (const auto& ct : geom) {
      const int C = ct[0], T = ct[1];
      const size_t esz = f32 ? 4 : 1, smax = (((size_t)1 << 31) - 7) / esz;  // the largest span
      std::vector<int32_t> perm(C), two(C), neg(C), imin(C), big(C);
      for (int c = 0; c < C; c++) {
        perm[c] = (c * 7 + 3) % (C + 3);
        two[c] = c & 1;                  // max 1: span = row_stride + T
        neg[c] = c == C - 1 ? -1 : c;
        imin[c] = c == 0 ? INT32_MIN : c;
        big[c] = c == 1 ? INT32_MAX : c;
      }
      const EpArgs base{C, T, X, f32 != 0, (size_t)1 << 20, 2000, nullptr, ON, 9, Y, NB, 0};
      ep_case(base);
      const std::vector<int32_t>* const tables[] = {nullptr, &perm, &two, &neg, &imin, &big};
      for (const std::vector<int32_t>* ch : tables) {
        const size_t cmax = !ch ? (size_t)C - 1 : ch == &perm ? (size_t)C + 2 : ch == &two ? 1 : (size_t)INT32_MAX;
        // row strides at 0, at the span's limit, where cmax row_stride + T wraps size_t, and at the end
        for (size_t rs : {(size_t)0, (size_t)1, (size_t)T, (smax - T) / cmax, (smax - T) / cmax + 1,
                          (SIZE_MAX - T) / cmax, (SIZE_MAX - T) / cmax + 1, SIZE_MAX / cmax, SIZE_MAX / cmax + 1,
                          ((size_t)1 << 33) + 2, ((size_t)1 << 33) + 3, SIZE_MAX})
          for (int room = 0; room < 4; room++) {
            EpArgs a = base;
            a.channels = ch;
            a.row_stride = rs;
            const u128 span = (u128)cmax * rs + (u128)T;
            // n_elems: the span itself, one short, everything, and where n_elems - span passes INT64_MAX
            a.n_elems = room == 0 ? clip(span) : room == 1 ? clip(span) - 1 : room == 2 ? SIZE_MAX : clip(span + IMAX + 1);
            ep_case(a);
          }
      }
      // the span at its limit exactly (channels 0 and 1: span = row_stride + T) and one past it
      for (size_t d : {(size_t)0, (size_t)1}) {
        EpArgs a = base;
        a.channels = &two;
        a.row_stride = smax - T + d;
        a.n_elems = smax + d;
        ep_case(a);
        a.n_elems = smax + d - 1;
        ep_case(a);
      }
      for (size_t E : {(size_t)0, (size_t)1, WMAX, WMAX + 1, SIZE_MAX}) {
        EpArgs a = base;
        a.E = E;
        ep_case(a);
      }
      for (uintptr_t off : {1, 2, 3, 4}) {
        EpArgs a = base;
        a.y += off;
        ep_case(a);
        a = base;
        a.x += off;  // refused for float32 only
        ep_case(a);
        a = base;
        a.n_bad += off;
        ep_case(a);
        a = base;
        a.onsets += off;
        ep_case(a);
      }
      for (int which = 0; which < 4; which++)
        for (size_t E : {(size_t)0, (size_t)3}) {
          EpArgs a = base;
          a.E = E;
          (which == 0 ? a.x : which == 1 ? a.y : which == 2 ? a.onsets : a.n_bad) = 0;
          ep_case(a);
        }
      for (int device : {-1, 0, 63, 64, INT32_MIN, INT32_MAX}) {
        EpArgs a = base;
        a.device = device;
        ep_case(a);
      }
    }
}

// ---- windows_multi ----------------------------------------------------------------------------
// net_windows_multi_onsets' rule for a network of T samples; every array exactly as large as asked.
static void multi_case(size_t T, const std::vector<size_t>& len, size_t hop, bool null_lengths = false) {
  const size_t R = len.size();
  u128 sum = 0;
  for (size_t v : len) sum += v;
  const bool refused = hop == 0 || (R && null_lengths) || sum > (u128)IMAX;
  size_t W = 0;
  for (size_t v : len) W += refused || v < T ? 0 : (v - T) / hop + 1;
  const size_t* lp = null_lengths ? nullptr : len.data();
  CHECK(windows_multi(T, lp, R, hop, nullptr, 0, nullptr) == W, "multi R %zu hop %zu: the count alone", R, hop);
  g_cases++;
  if (W > ((size_t)1 << 24)) return;  // a count no array here could hold stays a count
  std::vector<size_t> first(R + 1, 77);
  if (refused) {  // 0, and nothing written although there is room
    std::vector<int64_t> o4(4, -9);
    CHECK(windows_multi(T, lp, R, hop, o4.data(), 4, first.data()) == 0, "multi R %zu hop %zu: refused", R, hop);
    for (size_t v : first) CHECK(v == 77, "multi R %zu hop %zu: a refused call wrote first", R, hop);
    for (int64_t v : o4) CHECK(v == -9, "multi R %zu hop %zu: a refused call wrote an onset", R, hop);
    return;
  }
  std::vector<int64_t> on(W, -9);
  CHECK(windows_multi(T, lp, R, hop, on.data(), W, first.data()) == W, "multi R %zu hop %zu: the count", R, hop);
  size_t i = 0, start = 0;
  for (size_t r = 0; r < R; r++) {
    CHECK(first[r] == i, "multi: first[%zu] = %zu, want %zu", r, first[r], i);
    for (size_t k = 0; len[r] >= T && k <= (len[r] - T) / hop; k++, i++)
      CHECK(on[i] == (int64_t)(start + k * hop), "multi: onset %zu = %lld", i, (long long)on[i]);
    start += len[r];
  }
  CHECK(first[R] == W && i == W, "multi: first[R] = %zu, W = %zu", first[R], W);
  // a capacity one short writes no onset (the array is exactly that short); first is still filled
  if (W) {
    std::vector<int64_t> o1(W - 1, -9);
    std::vector<size_t> f1(R + 1, 77);
    CHECK(windows_multi(T, lp, R, hop, o1.data(), W - 1, f1.data()) == W, "multi: the count with a short list");
    for (int64_t v : o1) CHECK(v == -9, "multi: a short onset list was written");
    CHECK(f1 == first, "multi: first with a short list");
  }
}

static void multi_cases() {
  for (size_t T : {(size_t)64, (size_t)1125})
    for (size_t hop : {(size_t)0, (size_t)1, (size_t)3, (size_t)1000, SIZE_MAX}) {
      multi_case(T, {T + 17, T, T - 1, 0, T + 2000, 1}, hop);
      multi_case(T, {T}, hop);
      multi_case(T, {T - 1, 0}, hop);    // no window at all
      multi_case(T, {}, hop);            // R == 0: first[0] = 0 is written (hop > 0)
      multi_case(T, {T, T}, hop, true);  // no lengths
      // sums at and past INT64_MAX, and one that wraps size_t
      multi_case(T, {IMAX}, hop);
      multi_case(T, {IMAX - 5, 5}, hop);
      multi_case(T, {5, IMAX - 5, 0}, hop);
      multi_case(T, {IMAX, 1}, hop);
      multi_case(T, {IMAX - 5, 5, 1}, hop);
      multi_case(T, {IMAX + 1}, hop);
      multi_case(T, {SIZE_MAX - 7, 8}, hop);
      multi_case(T, {SIZE_MAX, SIZE_MAX, 2}, hop);
    }
}

// ---- the scale, the strides and the counts -----------------------------------------------------
static void scalar_cases() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float lo = std::ldexp(1.0f, -60), hi = std::ldexp(1.0f, 60);
  struct { float v; int want; } sc[] = {
      {0.0f, NET_ERR_INVALID}, {-0.0f, NET_ERR_INVALID}, {-1.0f, NET_ERR_INVALID}, {-inf, NET_ERR_INVALID},
      {inf, NET_ERR_INVALID}, {nan, NET_ERR_INVALID}, {-nan, NET_ERR_INVALID},
      {std::numeric_limits<float>::denorm_min(), NET_ERR_RANGE}, {std::numeric_limits<float>::min(), NET_ERR_RANGE},
      {std::nextafter(lo, 0.0f), NET_ERR_RANGE}, {lo, NET_OK}, {std::nextafter(lo, 1.0f), NET_OK}, {1.0f, NET_OK},
      {std::nextafter(hi, 1.0f), NET_OK}, {hi, NET_OK}, {std::nextafter(hi, inf), NET_ERR_RANGE}, {1e38f, NET_ERR_RANGE}};
  for (const auto& s : sc) {
    CHECK(check_scale(s.v) == s.want, "check_scale(%a) = %d, want %d", (double)s.v, check_scale(s.v), s.want);
    const float want = s.v > 0.0f ? 1.0f / s.v : 0.0f;
    CHECK(s.v != s.v || recip_scale(s.v) == want, "recip_scale(%a) = %a", (double)s.v, (double)recip_scale(s.v));
    g_cases++;
  }
  CHECK(recip_scale(nan) == 0.0f, "recip_scale(NaN)");
  for (size_t L : {(size_t)0, (size_t)1, (size_t)15, (size_t)16, (size_t)17, ((size_t)1 << 31) - 1, SIZE_MAX / 16 - 15,
                   SIZE_MAX / 16, SIZE_MAX / 16 + 1, SIZE_MAX - 16, SIZE_MAX - 15, SIZE_MAX - 14, SIZE_MAX}) {
    // >= L and a multiple of 16, 0 where there is none; the workspace 16 rows, 0 where that wraps
    const u128 rs = round16(L);
    CHECK(windows_row_stride(L) == (rs > (u128)SIZE_MAX ? 0 : (size_t)rs), "row stride of %zu: %zu", L, windows_row_stride(L));
    CHECK(windows_workspace(L) == (16 * rs > (u128)SIZE_MAX ? 0 : (size_t)(16 * rs)), "workspace of %zu: %zu", L,
          windows_workspace(L));
    for (size_t T : {(size_t)64, (size_t)4096})
      for (size_t hop : {(size_t)0, (size_t)1, (size_t)5, SIZE_MAX}) {
        const size_t want = hop == 0 || L < T ? 0 : (size_t)(((u128)L - T) / hop + 1);
        CHECK(windows_count(T, L, hop) == want, "windows_count(%zu, %zu, %zu)", T, L, hop);
      }
    g_cases++;
  }
  Dims d;
  for (const auto& ct : {std::pair<int, int>{22, 1125}, {64, 4096}, {1, 64}, {3, 65}}) {
    d.C = ct.first, d.T = ct.second;
    const size_t n = (size_t)d.C * d.T;
    CHECK(trial_stride(d) >= n && trial_stride(d) < n + 16 && trial_stride(d) % 16 == 0, "trial stride of %d x %d", d.C, d.T);
    g_cases++;
  }
}

int main() {
  windows_cases();
  epochs_cases();
  multi_cases();
  scalar_cases();
  std::printf("cases %d\n", g_cases);
  if (g_bad) std::printf("%d checks failed\n", g_bad);
  return g_bad ? 1 : 0;
}
