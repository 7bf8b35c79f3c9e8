// stream_each_host_main.cpp — the host arithmetic of an each-group (csrc/stream_host.hpp: plan_each,
// each_rows, check_push_each, alloc_each) as a stand-alone program (tests/test_streams_each_cpu.py
// builds it with -fsanitize=address,undefined and runs it).  plan_each is the function one thread of
// k_stream_plan runs per session and push; here it walks positions around 0, T - 1, T, multiples of
// the ring and the position limit INT64_MAX - 65,536, counts inside and outside 0 .. n_max and hops
// up to 2^64 - 1.  Every value is printed, one case per line, and the Python side compares each with
// its own restatement in unbounded integers; an overflow that the header's arithmetic performed
// would be an UndefinedBehaviorSanitizer report.  Prints "cases <n>" last; exits 0 when every check
// here held.
#include <cinttypes>
#include <cstdint>
#include <cstdio>

#include "stream_host.hpp"

using namespace mib;

static int g_bad = 0, g_cases = 0;
#define CHECK(cond, ...) \
  do { \
    if (!(cond)) { \
      if (g_bad++ < 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    } \
  } while (0)

static void plan_case(unsigned T, unsigned long long hop, unsigned mp, long long pos, int cnt, unsigned n_max) {
  const unsigned cap = (unsigned)stream::ring_samples(T, mp);
  const stream::EachPlan e = stream::plan_each(T, hop, cap, pos, cnt, n_max);
  std::printf("plan %u %llu %u %lld %d %u : %d %d %d %d %d %lld\n", T, hop, mp, pos, cnt, n_max, (int)e.ok, e.rec.n, e.rec.p0,
              e.rec.k, e.rec.at0, e.W0);
  CHECK(e.rec.n >= 0 && (unsigned)e.rec.n <= n_max, "n outside 0 .. n_max");
  CHECK(e.rec.p0 >= 0 && (unsigned)e.rec.p0 < cap && e.rec.at0 >= 0 && (unsigned)e.rec.at0 < cap, "a ring position outside");
  CHECK(e.rec.k >= 0 && (size_t)e.rec.k <= stream::each_rows(hop, n_max), "k past kmax");
  // the last window's rows start inside two laps, and its hop multiple stays below n
  if (e.rec.k > 1) CHECK((unsigned long long)(e.rec.k - 1) * hop < (unsigned long long)e.rec.n, "j hop reaches n");
  if (!e.ok) CHECK(e.rec.n == 0 && e.rec.k == 0, "a refused count plans something");
  g_cases++;
}

static void rows_case(size_t hop, size_t n_max) {
  std::printf("rows %zu %zu %zu\n", hop, n_max, stream::each_rows(hop, n_max));
  g_cases++;
}

// one push check with valid pointers unless an offset or a flag says otherwise; `no` is a bit set of
// the pointers passed as NULL: 1 x, 2 cnt_in, 4 y, 8 cnt_out, 16 win0, 32 n_bad
static void push_case(size_t S, size_t hop, size_t mp, size_t n_max, int layout = 1, bool f32 = false, bool scales = true,
                      int xoff = 0, int coff = 0, int yoff = 0, int ooff = 0, int woff = 0, int boff = 0, int no = 0) {
  alignas(16) static char buf[128];
  stream::PushEach g{};
  g.kmax = 777;
  const int rc = stream::check_push_each(S, hop, mp, no & 1 ? nullptr : buf + xoff, layout, f32, scales,
                                         no & 2 ? nullptr : buf + 16 + coff, n_max, no & 4 ? nullptr : buf + 32 + yoff,
                                         no & 8 ? nullptr : buf + 48 + ooff, no & 16 ? nullptr : buf + 64 + woff,
                                         no & 32 ? nullptr : buf + 80 + boff, g);
  std::printf("push %zu %zu %zu %zu %d %d %d %d %d %d %d %d %d %d : %d", S, hop, mp, n_max, layout, (int)f32, (int)scales, xoff,
              coff, yoff, ooff, woff, boff, no, rc);
  if (rc == NET_OK) {
    std::printf(" %zu %d %zu %zu %zu", g.kmax, g.hop, g.blocks, g.l1_items, g.items);
    CHECK(g.items <= stream::MAX_ITEMS && g.l1_items <= stream::MAX_ITEMS, "items past the limit");
    CHECK((unsigned long long)g.kmax * (unsigned long long)g.hop < (unsigned long long)n_max + (unsigned long long)g.hop,
          "kmax hop past n_max + hop");
  } else {
    CHECK(g.kmax == 777, "a refused push wrote its geometry");
  }
  std::printf("\n");
  g_cases++;
}

static void alloc_case(size_t S, size_t cap) {
  const stream::AllocEach a = stream::alloc_each(S, cap);
  std::printf("alloc %zu %zu : %zu %zu %zu %zu %zu %zu %zu\n", S, cap, a.base.ring, a.base.origin, a.base.set, a.base.bytes,
              a.plan, a.pos, a.bytes);
  g_cases++;
}

int main() {
  static_assert(sizeof(stream::EachRec) == 16, "one record is one 16-byte scalar load");
  const long long LIM = stream::EACH_POS_LIMIT;
  std::printf("limit %lld\n", LIM);
  g_cases++;
  for (unsigned T : {64u, 1125u, 4096u})
    for (unsigned mp : {1u, 37u, 65536u})
      for (unsigned long long hop : {1ull, 3ull, (unsigned long long)T + 7, 1ull << 40, (unsigned long long)UINT64_MAX}) {
        const long long cap = (long long)stream::ring_samples(T, mp);
        for (long long pos : {0ll, 1ll, (long long)T - 2, (long long)T - 1, (long long)T, (long long)T + 1, cap - 1, cap, cap + 1,
                              7 * cap - 3, 7 * cap, (1ll << 40) * cap, LIM - 2 * (long long)mp, LIM - (long long)mp - 1,
                              LIM - (long long)mp, LIM - (long long)mp + 1, LIM - 1, LIM})
          for (int cnt : {0, 1, 2, (int)mp / 2, (int)mp - 1, (int)mp, (int)mp + 1, -1, INT32_MIN, INT32_MAX})
            plan_case(T, hop, mp, pos, cnt, mp);
      }
  // n_max below max_push: the bound of a count is the push's, not the group's
  for (int cnt : {0, 5, 16, 17, 37, 38, -3}) plan_case(64, 3, 37, 1000, cnt, 16);
  for (size_t hop : {(size_t)0, (size_t)1, (size_t)2, (size_t)3, (size_t)16, (size_t)37, (size_t)38, (size_t)65536,
                     (size_t)1 << 40, SIZE_MAX})
    for (size_t n : {(size_t)0, (size_t)1, (size_t)2, (size_t)3, (size_t)36, (size_t)37, (size_t)65535, (size_t)65536,
                     (size_t)65537, SIZE_MAX})
      rows_case(hop, n);
  // the argument checks in their documented order
  for (size_t n_max : {(size_t)0, (size_t)1, (size_t)16, (size_t)37, (size_t)38, SIZE_MAX}) push_case(5, 3, 37, n_max);
  for (int layout : {0, 1, 2, -1, 7}) push_case(5, 3, 37, 16, layout);
  push_case(5, 3, 37, 16, 7, true);                           // the float entry ignores the layout
  for (int no : {1, 2, 4, 8, 16, 32, 48, 63}) push_case(5, 3, 37, 16, 1, false, true, 0, 0, 0, 0, 0, 0, no);
  for (int off : {1, 2, 3}) {
    push_case(5, 3, 37, 16, 1, false, true, off);             // int8 x at any alignment
    push_case(5, 3, 37, 16, 1, true, true, off);              // misaligned float x
    push_case(5, 3, 37, 16, 1, false, true, 0, off);          // cnt_in
    push_case(5, 3, 37, 16, 1, false, true, 0, 0, off);       // y
    push_case(5, 3, 37, 16, 1, false, true, 0, 0, 0, off);    // cnt_out
    push_case(5, 3, 37, 16, 1, false, true, 0, 0, 0, 0, off); // win0
    push_case(5, 3, 37, 16, 1, false, true, 0, 0, 0, 0, 0, off);  // n_bad
  }
  push_case(5, 3, 37, 16, 1, false, true, 0, 0, 0, 0, 4);     // win0 is int64: 4 is misaligned
  push_case(5, 3, 37, 16, 1, true, false);                    // no scales
  push_case(5, 3, 37, 16, 1, false, false);                   // int8 needs none
  push_case(5, 3, 37, 38, 2, true, false, 2, 1, 1, 1, 1, 1, 63);  // n_max comes first
  push_case(5, 3, 37, 16, 2, false, false, 0, 0, 1, 0, 0, 0, 4);  // then the layout, then NULL, then alignment
  push_case(5, 3, 37, 16, 1, true, false, 2);                 // alignment before the scales
  // the item limits: S max_push at MAX_ITEMS, hop 1 makes kmax = n_max
  push_case(stream::MAX_ITEMS / 65536, 1, 65536, 65536);
  push_case(stream::MAX_ITEMS, 1, 1, 1);
  push_case(stream::MAX_ITEMS / 37, SIZE_MAX, 37, 37);
  push_case(5, (size_t)1 << 40, 65536, 65536);
  for (size_t S : {(size_t)1, (size_t)5, (size_t)1024, stream::MAX_ITEMS})
    for (size_t cap : {(size_t)16, (size_t)112, (size_t)4144, (size_t)69632}) alloc_case(S, cap);
  std::printf("cases %d\n", g_cases);
  if (g_bad) std::printf("%d checks failed\n", g_bad);
  return g_bad ? 1 : 0;
}
