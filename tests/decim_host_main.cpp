// decim_host_main.cpp — the host arithmetic and checks of a stream group's decimator
// (csrc/stream_host.hpp) as a stand-alone program (tests/test_decim_host_sanitizers.py builds it with
// -fsanitize=address,undefined and runs it).  It walks raw_samples, check_set_decimator,
// check_push_raw and the history's slots at the edges where a sum, a product or a conversion could
// wrap: raw positions near 2^63 and 2^64, n_raw at q max_push and one more, m = 0.  Every value is
// printed, one case per line, and the Python side compares each with its own restatement in unbounded
// integers.  Prints "cases <n>" last; exits 0 when every check here held.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "stream_host.hpp"

using namespace mib;

static int g_bad = 0, g_cases = 0;
#define CHECK(cond, ...) \
  do { \
    if (!(cond)) { \
      if (g_bad++ < 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    } \
  } while (0)

static void m_case(size_t q, uint64_t P, size_t n) {
  std::printf("m %zu %" PRIu64 " %zu %zu\n", q, P, n, stream::raw_samples(q, P, n));
  g_cases++;
}

// what: 0 finite taps, 1 a NaN, 2 +inf, 3 -inf (at the last tap), 4 no taps
static void set_case(bool group, bool each, bool scales, bool have, bool pushed, size_t q, size_t K, int what) {
  // a K outside 1 .. 128 is refused before a tap is read: the array is one tap long then, and a read
  // past it would be an AddressSanitizer report
  std::vector<float> h(K >= 1 && K <= stream::MAX_TAPS ? K : 1, 0.25f);
  if (what == 1) h.back() = std::numeric_limits<float>::quiet_NaN();
  if (what == 2) h.back() = std::numeric_limits<float>::infinity();
  if (what == 3) h.back() = -std::numeric_limits<float>::infinity();
  const int rc = stream::check_set_decimator(group, each, scales, have, pushed, q, what == 4 ? nullptr : h.data(), K);
  std::printf("set %d %d %d %d %d %zu %zu %d : %d\n", (int)group, (int)each, (int)scales, (int)have, (int)pushed, q, K,
              what, rc);
  g_cases++;
}

static void alloc_case(size_t S, size_t R, size_t K) {
  const stream::AllocDecim a = stream::alloc_decim(S, R, K);
  std::printf("alloc %zu %zu %zu : %zu %zu %zu %zu\n", S, R, K, a.taps, a.hist, a.per, a.bytes);
  g_cases++;
}

static void slot_case(uint64_t a, size_t K) {
  std::printf("slot %" PRIu64 " %zu %zu\n", a, K, stream::hist_slot(a, K));
  g_cases++;
}

// one raw push check with valid pointers unless a flag says otherwise
static void raw_case(size_t T, size_t S, size_t R, size_t hop, size_t mp, size_t q, size_t K, uint64_t P, size_t n,
                     bool scales = true, int xoff = 0, int yoff = 0, int boff = 0, bool nox = false, bool noy = false) {
  alignas(16) static char buf[64];
  const size_t cap = stream::ring_samples(T, mp);
  stream::PushRaw g{};
  g.m = 777;
  const int rc = stream::check_push_raw(T, S, R, hop, mp, cap, q, K, P, nox ? nullptr : buf + xoff, scales, n,
                                        noy ? nullptr : buf + 16 + yoff, buf + 32 + boff, g);
  std::printf("raw %zu %zu %zu %zu %zu %zu %zu %" PRIu64 " %zu %d %d %d %d %d %d : %d", T, S, R, hop, mp, q, K, P, n,
              (int)scales, xoff, yoff, boff, (int)nox, (int)noy, rc);
  if (rc == NET_OK && n) {
    const stream::Push& p = g.push;
    std::printf(" %zu %" PRIu64 " %d %d %zu %zu", g.m, g.d0, g.off, g.slot0, g.keep, g.hist_items);
    if (g.m)
      std::printf(" %zu %" PRIu64 " %lld %d %d %zu %zu %zu", p.k, p.W0, p.first, p.first_mod, p.p0, p.blocks, p.l1_items,
                  p.items);
    CHECK(g.m <= mp, "m past max_push");
    CHECK(g.off >= 0 && (size_t)g.off < q, "off outside 0 .. q - 1");
    CHECK(g.slot0 >= 0 && (K == 1 ? g.slot0 == 0 : (size_t)g.slot0 < K - 1), "slot0 outside");
    CHECK(g.keep <= K - 1 && g.keep <= n, "keep");
    CHECK(g.d0 <= (uint64_t)INT64_MAX - g.m, "the decimated position past int64");
    // every frame a sample of the push reads: in the chunk, or at most K - 1 frames before it
    if (g.m) {
      const long long last = (long long)q * (long long)(g.m - 1) + g.off;
      CHECK(last >= 0 && (size_t)last < n, "the last sample's frame %lld outside the chunk of %zu", last, n);
    }
  } else {
    CHECK(g.m == 777 || n == 0 || rc == NET_OK, "a refused push wrote its plan");
  }
  std::printf("\n");
  g_cases++;
}

int main() {
  const uint64_t I63 = (uint64_t)INT64_MAX;
  for (size_t q : {(size_t)0, (size_t)1, (size_t)2, (size_t)3, (size_t)5, (size_t)16, (size_t)17, SIZE_MAX})
    for (uint64_t P : {(uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)15, (uint64_t)16, (uint64_t)17, (uint64_t)1 << 40,
                       I63 - 65536, I63 - 1, I63, I63 + 1, UINT64_MAX - 65536, UINT64_MAX - 1, UINT64_MAX})
      for (size_t n : {(size_t)0, (size_t)1, (size_t)2, (size_t)15, (size_t)16, (size_t)47, (size_t)65536, (size_t)1 << 20})
        m_case(q, P, n);
  // set_decimator: the kind of group first, then its state, the limits, the taps, the scales
  set_case(false, false, true, false, false, 2, 7, 0);
  set_case(true, true, true, false, false, 2, 7, 0);
  set_case(true, true, false, true, true, 0, 0, 4);  // an each-group is UNSUPPORTED whatever else is wrong
  set_case(true, false, true, true, false, 2, 7, 0);
  set_case(true, false, true, false, true, 2, 7, 0);
  for (size_t q : {(size_t)0, (size_t)1, (size_t)16, (size_t)17, SIZE_MAX}) set_case(true, false, true, false, false, q, 7, 0);
  for (size_t K : {(size_t)0, (size_t)1, (size_t)2, (size_t)128, (size_t)129, SIZE_MAX})
    set_case(true, false, true, false, false, 2, K, 0);
  for (int what : {0, 1, 2, 3, 4}) set_case(true, false, true, false, false, 3, 33, what);
  set_case(true, false, true, false, false, 1, 1, 1);
  set_case(true, false, false, false, false, 2, 7, 0);
  for (size_t S : {(size_t)1, (size_t)5, stream::MAX_ITEMS})
    for (size_t R : {(size_t)1, (size_t)22, (size_t)64})
      for (size_t K : {(size_t)1, (size_t)2, (size_t)7, (size_t)33, (size_t)128}) alloc_case(S, R, K);
  for (size_t K : {(size_t)2, (size_t)3, (size_t)7, (size_t)128})
    for (uint64_t a : {(uint64_t)0, (uint64_t)1, (uint64_t)K - 2, (uint64_t)K - 1, (uint64_t)K, (uint64_t)1 << 40, I63,
                       UINT64_MAX})
      slot_case(a, K);
  // raw pushes: every (q, K) at positions of every residue, n_raw at the limit and one more, m = 0
  for (size_t T : {(size_t)64, (size_t)4096})
    for (size_t mp : {(size_t)1, (size_t)37, (size_t)65536})
      for (size_t q : {(size_t)1, (size_t)2, (size_t)3, (size_t)16})
        for (size_t K : {(size_t)1, (size_t)2, (size_t)33, (size_t)128})
          for (uint64_t P : {(uint64_t)0, (uint64_t)1, (uint64_t)q - 1, (uint64_t)q, (uint64_t)q + 1, (uint64_t)q * T - 1,
                             (uint64_t)q * T, (uint64_t)q * T + 1, ((uint64_t)1 << 40) + 5, I63 - q * mp - 1, I63 - q * mp,
                             I63 - q * mp + 1, I63 - 1, I63})
            for (size_t n : {(size_t)0, (size_t)1, q - 1, q, q + 1, K - 1, K, q * mp - 1, q * mp, q * mp + 1})
              raw_case(T, 5, 22, 3, mp, q, K, P, n);
  // S at the item limit, R at its own
  raw_case(64, stream::MAX_ITEMS / 65536, 64, 1, 65536, 16, 128, 16 << 20, 16 * 65536);
  raw_case(64, stream::MAX_ITEMS, 64, 1, 1, 16, 128, 1 << 20, 16);
  raw_case(64, stream::MAX_ITEMS, 64, 1, 1, 16, 128, (1 << 20) + 1, 15);  // m == 0, the history moves
  // the argument checks in their order (position 300 at q 3: decimated position 100, k > 0 for n >= 3)
  raw_case(64, 5, 22, 3, 37, 3, 33, 300, 15, false);                         // no scales
  raw_case(64, 5, 22, 3, 37, 3, 33, 300, 15, true, 2);                       // misaligned x
  raw_case(64, 5, 22, 3, 37, 3, 33, 300, 15, true, 0, 2);                    // misaligned y, k > 0
  raw_case(64, 5, 22, 3, 37, 3, 33, 30, 15, true, 0, 2);                     // misaligned y, k == 0
  raw_case(64, 5, 22, 3, 37, 3, 33, 30, 15, true, 0, 0, 0, false, true);     // no y, k == 0
  raw_case(64, 5, 22, 3, 37, 3, 33, 300, 15, true, 0, 0, 0, false, true);    // no y, k > 0
  raw_case(64, 5, 22, 3, 37, 3, 33, 301, 2, true, 0, 2, 0, false, true);     // m == 0: y is not looked at
  raw_case(64, 5, 22, 3, 37, 3, 33, 301, 2, true, 0, 0, 1);                  // m == 0, misaligned n_bad
  raw_case(64, 5, 22, 3, 37, 3, 33, 300, 15, true, 0, 0, 1);                 // misaligned n_bad
  raw_case(64, 5, 22, 3, 37, 3, 33, 300, 15, true, 0, 0, 0, true);           // no x
  raw_case(64, 5, 22, 3, 37, 3, 33, 300, 112, false, 2, 2, 1, true, true);   // n_raw > q max_push comes first
  raw_case(64, 5, 22, 3, 37, 3, 33, 300, 0, false, 2, 2, 1, true, true);     // n_raw == 0 comes before that
  std::printf("cases %d\n", g_cases);
  if (g_bad) std::printf("%d checks failed\n", g_bad);
  return g_bad ? 1 : 0;
}
