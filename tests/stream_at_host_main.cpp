// stream_at_host_main.cpp — the host arithmetic of net_streams_windows_at (csrc/stream_host.hpp:
// at_item, at_ring, at_span, check_windows_at) as a stand-alone program
// (tests/test_streams_at_host_sanitizers.py builds it with -fsanitize=address,undefined and runs it).
// at_item is the predicate every workgroup of k_forward_ring_at runs per item; here it and the ring
// position walk positions and onsets around 0, T, cap, the seam, INT64_MIN/MAX and EACH_POS_LIMIT,
// origins on both sides of the window, and onsets whose low 32 bits alone would be valid, each held
// to a restatement in 128-bit integers.  Every value is printed, one case per line, and the Python
// side compares each with its own restatement in unbounded integers; an overflow that the header's
// arithmetic performed would be an UndefinedBehaviorSanitizer report.  Prints "cases <n>" last; exits
// 0 when every check here held.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "stream_host.hpp"

using namespace mib;
typedef __int128 i128;

static int g_bad = 0, g_cases = 0;
#define CHECK(cond, ...) \
  do { \
    if (!(cond)) { \
      if (g_bad++ < 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    } \
  } while (0)

static bool fits(i128 v) { return v >= (i128)INT64_MIN && v <= (i128)INT64_MAX; }

static void item_case(long long o, long long lo, long long pos, unsigned T, unsigned cap) {
  const stream::AtItem a = stream::at_item(o, lo, pos, T, cap);
  const i128 d = (i128)pos - (i128)o;
  const bool want = o >= 0 && (i128)o >= (i128)lo && d >= (i128)T && d <= (i128)cap;
  int at = -1;
  if (a.valid) {
    at = stream::at_ring((int)((unsigned long long)pos % cap), a.d, (int)cap);
    CHECK((i128)a.d == d, "d %u", a.d);
    CHECK(at >= 0 && (unsigned)at < cap, "a ring position outside: %d", at);
    CHECK((i128)at == (i128)o % (i128)cap, "at %d is not o mod cap", at);  // o >= 0
    CHECK((unsigned)at + T <= 2 * cap, "the window leaves the doubled row");
  }
  CHECK(a.valid == want, "o %lld lo %lld pos %lld T %u cap %u", o, lo, pos, T, cap);
  CHECK(a.valid || a.d == 0, "an invalid item carries a distance");
  std::printf("item %lld %lld %lld %u %u : %d %u %d\n", o, lo, pos, T, cap, (int)a.valid, a.d, at);
  g_cases++;
}

// every (pos mod cap, d) pair of a small ring: the one correction reaches (pos mod cap - d) mod cap
static void ring_case(unsigned T, unsigned cap) {
  int bad = 0;
  for (unsigned pm = 0; pm < cap; pm++)
    for (unsigned d = T; d <= cap; d++) {
      const int at = stream::at_ring((int)pm, d, (int)cap);
      bad += at != (int)(((i128)pm - (i128)d + 2 * (i128)cap) % (i128)cap);
    }
  CHECK(bad == 0, "at_ring T %u cap %u: %d wrong", T, cap, bad);
  std::printf("ring %u %u : %d\n", T, cap, bad);
  g_cases++;
}

static void span_case(size_t T, size_t cap, uint64_t pos) {
  int64_t lo = -7, hi = -7;
  stream::at_span(T, cap, pos, &lo, &hi);
  const i128 wl = (i128)pos - (i128)cap > 0 ? (i128)pos - (i128)cap : 0, wh = (i128)pos - (i128)T;
  CHECK((i128)lo == wl && (i128)hi == wh, "span T %zu cap %zu pos %" PRIu64, T, cap, pos);
  // the ends are valid onsets of a session with origin 0, and one past each is not
  if (hi >= lo) {
    CHECK(stream::at_item(lo, 0, (long long)pos, (unsigned)T, (unsigned)cap).valid, "lo is no valid onset");
    CHECK(stream::at_item(hi, 0, (long long)pos, (unsigned)T, (unsigned)cap).valid, "hi is no valid onset");
    CHECK(!stream::at_item(lo - 1, 0, (long long)pos, (unsigned)T, (unsigned)cap).valid, "lo - 1 is valid");
  }
  CHECK(!stream::at_item(hi + 1, 0, (long long)pos, (unsigned)T, (unsigned)cap).valid, "hi + 1 is valid");
  std::printf("span %zu %zu %" PRIu64 " : %" PRId64 " %" PRId64 "\n", T, cap, pos, lo, hi);
  g_cases++;
}

// one check with valid pointers unless an offset or a flag says otherwise; `no` is a bit set of the
// pointers passed as NULL: 1 session, 2 onsets, 4 y, 8 n_bad
static void check_case(bool group, size_t W, int soff = 0, int ooff = 0, int yoff = 0, int boff = 0, int no = 0) {
  alignas(16) static char buf[96];
  const int rc = stream::check_windows_at(group, W, no & 1 ? nullptr : buf + soff, no & 2 ? nullptr : buf + 16 + ooff,
                                          no & 4 ? nullptr : buf + 32 + yoff, no & 8 ? nullptr : buf + 48 + boff);
  std::printf("check %d %zu %d %d %d %d %d : %d\n", (int)group, W, soff, ooff, yoff, boff, no, rc);
  g_cases++;
}

int main() {
  const long long LIM = stream::EACH_POS_LIMIT;
  std::printf("limit %lld %zu\n", LIM, stream::MAX_ITEMS);
  g_cases++;
  for (unsigned T : {64u, 1125u, 4096u})
    for (unsigned mp : {1u, 37u, 65536u}) {
      const unsigned cap = (unsigned)stream::ring_samples(T, mp);
      const i128 c = cap, t = T;
      std::vector<i128> poss = {0, 1, t - 1, t, t + 1, c - 1, c, c + 1, 2 * c - 1, 2 * c, 2 * c + 1, 7 * c - 3, 7 * c,
                                ((i128)1 << 32) + 5, ((i128)1 << 40) * c + 5, (i128)LIM - 1, (i128)LIM, (i128)INT64_MAX};
      for (i128 p : poss) {
        std::vector<i128> os = {0, 1, -1, (i128)INT64_MIN, (i128)INT64_MIN + 1, (i128)INT64_MAX, (i128)INT64_MAX - 1, p,
                                p + 1, p - 1};
        for (int k = -2; k <= 2; k++) {
          os.push_back(p - t + k);
          os.push_back(p - c + k);
        }
        // the low 32 bits of a valid onset under other high halves, and the valid distance from a
        // position whose high half differs
        for (i128 good : {p - t, p - c, p - t - 1})
          for (i128 hi : {(i128)1 << 32, -((i128)1 << 32), (i128)1 << 62, -((i128)1 << 63), (i128)0xFFFFFFFFll << 32})
            os.push_back(good + hi);
        std::vector<i128> los = {0, 1, p - t - 1, p - t, p - t + 1, p - c + 3, p, (i128)INT64_MAX};
        for (i128 o : os)
          for (i128 lo : los)
            if (fits(o) && fits(lo) && lo >= 0) item_case((long long)o, (long long)lo, (long long)p, T, cap);
      }
      // a position no session has: every onset fails, nothing overflows
      for (long long o : {0ll, -1ll, (long long)INT64_MIN, (long long)INT64_MAX})
        for (long long p : {-1ll, (long long)INT64_MIN}) item_case(o, 0, p, T, cap);
      for (i128 p : poss) span_case(T, cap, (uint64_t)p);
    }
  for (unsigned T : {1u, 15u, 64u})
    for (unsigned mp : {1u, 16u, 37u}) ring_case(T, (unsigned)stream::ring_samples(T, mp));
  // the argument checks in their documented order
  check_case(false, 0);
  check_case(false, 5);
  check_case(false, 0, 1, 1, 1, 1, 15);
  check_case(true, 0);
  check_case(true, 0, 1, 1, 1, 1, 15);                         // W == 0: nothing is looked at
  for (size_t W : {(size_t)1, (size_t)5, stream::MAX_ITEMS - 1, stream::MAX_ITEMS, stream::MAX_ITEMS + 1, (size_t)1 << 31,
                   (size_t)1 << 40, SIZE_MAX})
    check_case(true, W);
  for (int no : {1, 2, 4, 8, 3, 7, 15}) check_case(true, 5, 0, 0, 0, 0, no);
  for (int off : {1, 2, 3, 4, 5, 6, 7, 8}) {
    check_case(true, 5, off);              // session
    check_case(true, 5, 0, off);           // onsets: int64
    check_case(true, 5, 0, 0, off);        // y
    check_case(true, 5, 0, 0, 0, off);     // n_bad
  }
  check_case(true, 5, 0, 0, 0, 2, 8);                          // a NULL n_bad has no alignment
  check_case(true, stream::MAX_ITEMS + 1, 0, 0, 0, 0, 7);      // W comes before the pointers
  check_case(true, 5, 1, 0, 0, 0, 2);                          // NULL before alignment
  std::printf("cases %d\n", g_cases);
  if (g_bad) std::printf("%d checks failed\n", g_bad);
  return g_bad ? 1 : 0;
}
