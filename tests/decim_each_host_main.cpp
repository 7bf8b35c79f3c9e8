// decim_each_host_main.cpp — the host arithmetic of an each-group's decimator (csrc/stream_host.hpp:
// plan_each_raw, each_raw_rows, alloc_decim_each, check_push_each_raw) as a stand-alone program
// (tests/test_decim_each_host_sanitizers.py builds it with -fsanitize=address,undefined and runs it).
// plan_each_raw is the function one thread of k_stream_plan_raw runs per session and raw push; here it
// walks q in {1, 2, 3, 16}, K in {1, 2, 7, 128}, raw positions at 0, small, on and off the grid and
// around the limit INT64_MAX - 2^20, and counts inside and outside 0 .. n_raw_max, each against a
// restatement in 128-bit integers.  Every value is printed, one case per line, for the Python side's
// own restatement in unbounded integers; an overflow that the header's arithmetic performed would be
// an UndefinedBehaviorSanitizer report.  Prints "cases <n>" last; exits 0 when every check here held.
#include <cinttypes>
#include <cstdint>
#include <cstdio>

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

static i128 D(i128 P, i128 q) { return (P + q - 1) / q; }
static i128 count(i128 T, i128 L, i128 hop) { return L < T ? 0 : (L - T) / hop + 1; }

static void plan_case(unsigned T, unsigned long long hop, unsigned mp, unsigned q, unsigned K, long long P, int cnt,
                      unsigned n_raw_max) {
  const unsigned cap = (unsigned)stream::ring_samples(T, mp);
  const stream::EachRawPlan e = stream::plan_each_raw(T, hop, cap, q, K, P, cnt, n_raw_max);
  const stream::EachRec& r = e.each.rec;
  std::printf("plan %u %llu %u %u %u %lld %d %u : %d %d %d %d %d %d %d %d %d %d %lld\n", T, hop, mp, q, K, P, cnt, n_raw_max,
              (int)e.each.ok, e.m, e.raw.n_raw, e.raw.off, e.raw.slot0, e.raw.keep, r.n, r.p0, r.k, r.at0, e.each.W0);
  // the restatement: nothing here can wrap
  const bool ok = cnt >= 0 && (i128)cnt <= (i128)n_raw_max && (i128)P + cnt <= (i128)stream::EACH_RAW_LIMIT;
  const i128 n = ok ? cnt : 0, d0 = D(P, q), d1 = D((i128)P + n, q), m = d1 - d0;
  const i128 W0 = count(T, d0, hop), k = count(T, d1, hop) - W0;
  CHECK(e.each.ok == ok, "the verdict");
  CHECK(e.raw.n_raw == n && e.m == m && r.n == m, "n_raw %d m %d n %d", e.raw.n_raw, e.m, r.n);
  CHECK(e.raw.off == q * d0 - P && e.raw.off >= 0 && (unsigned)e.raw.off < q, "off %d", e.raw.off);
  CHECK(e.raw.slot0 == (K > 1 ? (i128)P % (K - 1) : 0), "slot0 %d", e.raw.slot0);
  CHECK(K == 1 ? e.raw.slot0 == 0 : (unsigned)e.raw.slot0 < K - 1, "slot0 outside 0 .. K - 2");
  CHECK(e.raw.keep == (n < (i128)K - 1 ? n : (i128)K - 1), "keep %d", e.raw.keep);
  CHECK(r.p0 == d0 % cap && e.each.W0 == W0 && r.k == k, "p0 %d W0 %lld k %d", r.p0, e.each.W0, r.k);
  CHECK(r.at0 == (k ? W0 * hop % cap : 0), "at0 %d", r.at0);
  // pos = D(P) before and after: the plan kernel adds n_raw to P and n to pos
  CHECK(d0 + r.n == D((i128)P + e.raw.n_raw, q), "pos is not D(P) after the push");
  CHECK(m <= D(n, q) && m <= D(n_raw_max, q), "m past ceil(cnt / q)");
  CHECK((size_t)r.k <= stream::each_raw_rows(hop, q, n_raw_max) || stream::each_raw_rows(hop, q, n_raw_max) == 0, "k past kmax");
  if (m > 0) CHECK((i128)q * (m - 1) + e.raw.off <= n - 1, "an answered sample reads a frame at or past cnt");
  if (!ok) CHECK(e.raw.n_raw == 0 && e.m == 0 && r.n == 0 && r.k == 0 && e.raw.keep == 0, "a refused count plans something");
  g_cases++;
}

static void rows_case(size_t hop, size_t q, size_t n_raw_max) {
  std::printf("rows %zu %zu %zu %zu\n", hop, q, n_raw_max, stream::each_raw_rows(hop, q, n_raw_max));
  g_cases++;
}

static void alloc_case(size_t S, size_t R, size_t K) {
  const stream::AllocDecimEach a = stream::alloc_decim_each(S, R, K);
  std::printf("alloc %zu %zu %zu : %zu %zu %zu %zu %zu %zu %zu\n", S, R, K, a.base.taps, a.base.hist, a.base.per,
              a.base.bytes, a.raw_pos, a.rec, a.bytes);
  CHECK(a.raw_pos % 16 == 0 && a.rec % 16 == 0 && a.raw_pos >= a.base.bytes && a.rec >= a.raw_pos + 8 * S, "the arrays overlap");
  g_cases++;
}

// one raw push check with valid pointers unless an offset or a flag says otherwise; `no` is a bit set
// of the pointers passed as NULL: 1 x, 2 cnt_in, 4 y, 8 cnt_out, 16 win0, 32 n_bad
static void push_case(size_t S, size_t R, size_t hop, size_t mp, size_t q, size_t K, size_t n_raw_max, bool scales = true,
                      int xoff = 0, int coff = 0, int yoff = 0, int ooff = 0, int woff = 0, int boff = 0, int no = 0) {
  alignas(16) static char buf[128];
  stream::PushEachRaw g{};
  g.n_max = 777;
  const int rc = stream::check_push_each_raw(S, R, hop, mp, q, K, no & 1 ? nullptr : buf + xoff, scales,
                                             no & 2 ? nullptr : buf + 16 + coff, n_raw_max, no & 4 ? nullptr : buf + 32 + yoff,
                                             no & 8 ? nullptr : buf + 48 + ooff, no & 16 ? nullptr : buf + 64 + woff,
                                             no & 32 ? nullptr : buf + 80 + boff, g);
  std::printf("push %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d %d %d %d : %d", S, R, hop, mp, q, K, n_raw_max, (int)scales, xoff,
              coff, yoff, ooff, woff, boff, no, rc);
  if (rc == NET_OK) {
    std::printf(" %zu %zu %zu %zu %d %zu %zu %zu", g.n_max, g.keep_max, g.hist_items, g.each.kmax, g.each.hop, g.each.blocks,
                g.each.l1_items, g.each.items);
    CHECK(g.each.items <= stream::MAX_ITEMS && g.each.l1_items <= stream::MAX_ITEMS, "items past the limit");
    CHECK(g.n_max >= 1 && g.n_max <= mp && g.keep_max <= K - 1 && g.keep_max <= n_raw_max, "n_max or keep_max");
    CHECK(g.each.kmax == stream::each_raw_rows(hop, q, n_raw_max), "kmax is not each_raw_rows");
  } else {
    CHECK(g.n_max == 777, "a refused push wrote its geometry");
  }
  std::printf("\n");
  g_cases++;
}

int main() {
  static_assert(sizeof(stream::RawRec) == 16 && sizeof(stream::EachRec) == 16, "one record is one 16-byte scalar load");
  const long long LIM = stream::EACH_RAW_LIMIT;
  std::printf("limit %lld\n", LIM);
  g_cases++;
  for (unsigned T : {64u, 480u})
    for (unsigned mp : {37u, 65536u})
      for (unsigned q : {1u, 2u, 3u, 16u})
        for (unsigned K : {1u, 2u, 7u, 128u}) {
          const unsigned nm = q * mp;
          const long long qT = (long long)q * T;
          for (long long P : {0ll, 1ll, 5ll, (long long)q - 1, (long long)q, (long long)q + 1, qT - 1, qT, qT + 1, 1000 * qT + 1,
                              ((1ll << 40) + 5) * q, ((1ll << 40) + 5) * q + 1, LIM - (long long)nm - 1, LIM - (long long)nm,
                              LIM - (long long)nm + 1, LIM - 1, LIM, LIM + 1})
            for (int cnt : {-1, 0, 1, (int)q - 1, (int)q, (int)q + 1, (int)K - 1, (int)K, (int)nm - 1, (int)nm, (int)nm + 1, INT32_MIN,
                            INT32_MAX})
              plan_case(T, 3, mp, q, K, P, cnt, nm);
        }
  // n_raw_max below q max_push: the bound of a count is the push's; other hops
  for (int cnt : {0, 5, 16, 17, 18, 111, -3}) plan_case(64, 3, 37, 3, 33, 1000, cnt, 17);
  for (unsigned long long hop : {1ull, 70ull, 1ull << 40, (unsigned long long)UINT64_MAX})
    for (int cnt : {0, 1, 7, 74}) plan_case(64, hop, 37, 2, 7, 2 * 64 + 1, cnt, 74);
  for (size_t hop : {(size_t)0, (size_t)1, (size_t)3, (size_t)37, (size_t)65536, SIZE_MAX})
    for (size_t q : {(size_t)0, (size_t)1, (size_t)2, (size_t)3, (size_t)16, (size_t)17, SIZE_MAX})
      for (size_t n : {(size_t)0, (size_t)1, (size_t)2, (size_t)3, (size_t)74, (size_t)65536, (size_t)65537, (size_t)1 << 20,
                       ((size_t)1 << 20) + 1, SIZE_MAX})
        rows_case(hop, q, n);
  for (size_t S : {(size_t)1, (size_t)5, (size_t)1024, stream::MAX_ITEMS})
    for (size_t R : {(size_t)1, (size_t)22, (size_t)64})
      for (size_t K : {(size_t)1, (size_t)2, (size_t)7, (size_t)33, (size_t)128}) alloc_case(S, R, K);
  // the argument checks in their documented order: n_raw_max first, then push_each_f32_tm's
  for (size_t q : {(size_t)1, (size_t)3, (size_t)16})
    for (size_t n : {(size_t)0, (size_t)1, q - 1, q, q + 1, q * 37 - 1, q * 37, q * 37 + 1, SIZE_MAX})
      for (size_t K : {(size_t)1, (size_t)2, (size_t)33, (size_t)128}) push_case(5, 22, 3, 37, q, K, n);
  for (int no : {1, 2, 4, 8, 16, 32, 48, 63}) push_case(5, 22, 3, 37, 3, 33, 50, true, 0, 0, 0, 0, 0, 0, no);
  for (int off : {1, 2, 3}) {
    push_case(5, 22, 3, 37, 3, 33, 50, true, off);                 // misaligned float x
    push_case(5, 22, 3, 37, 3, 33, 50, true, 0, off);              // cnt_in
    push_case(5, 22, 3, 37, 3, 33, 50, true, 0, 0, off);           // y
    push_case(5, 22, 3, 37, 3, 33, 50, true, 0, 0, 0, off);        // cnt_out
    push_case(5, 22, 3, 37, 3, 33, 50, true, 0, 0, 0, 0, off);     // win0
    push_case(5, 22, 3, 37, 3, 33, 50, true, 0, 0, 0, 0, 0, off);  // n_bad
  }
  push_case(5, 22, 3, 37, 3, 33, 50, true, 0, 0, 0, 0, 4);         // win0 is int64: 4 is misaligned
  push_case(5, 22, 3, 37, 3, 33, 50, false);                       // no scales
  push_case(5, 22, 3, 37, 3, 33, 112, false, 2, 1, 1, 1, 1, 1, 63);  // n_raw_max comes first
  push_case(5, 22, 3, 37, 3, 33, 50, false, 0, 0, 1, 0, 0, 0, 4);    // then NULL, then alignment, then the scales
  push_case(5, 22, 3, 37, 3, 33, 50, false, 2);
  // the item limits: S max_push at MAX_ITEMS, hop 1 makes kmax = ceil(n_raw_max / q)
  push_case(stream::MAX_ITEMS / 65536, 64, 1, 65536, 16, 128, 16 * 65536);
  push_case(stream::MAX_ITEMS, 64, 1, 1, 16, 128, 16);
  push_case(stream::MAX_ITEMS / 37, 64, SIZE_MAX, 37, 16, 128, 16 * 37);
  std::printf("cases %d\n", g_cases);
  if (g_bad) std::printf("%d checks failed\n", g_bad);
  return g_bad ? 1 : 0;
}
