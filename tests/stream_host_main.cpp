// stream_host_main.cpp — the host arithmetic and checks of a stream group (csrc/stream_host.hpp) as
// a stand-alone program (tests/test_streams_host_sanitizers.py builds it with
// -fsanitize=address,undefined and runs it).  It walks the edges where a sum, a product or a
// conversion could wrap: positions near 2^63 and 2^64, S k at the item limit, max_push at both
// bounds, hops past INT64_MAX, and the checks of the test hook that places a group (check_seek) at
// both ends of each kind's range.  Every value is printed, one case per line, and the Python side
// compares each with its own restatement; an overflow that the header's arithmetic performed would
// be an UndefinedBehaviorSanitizer report.  Prints "cases <n>" last; exits 0 when every check here held.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
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

static void cap_case(size_t T, size_t mp) {
  std::printf("cap %zu %zu %zu\n", T, mp, stream::ring_samples(T, mp));
  g_cases++;
}

static void k_case(size_t T, size_t hop, uint64_t pos, size_t n) {
  std::printf("k %zu %zu %" PRIu64 " %zu %zu\n", T, hop, pos, n, stream::push_windows(T, hop, pos, n));
  g_cases++;
}

// one push check with valid pointers unless a flag says otherwise
static void push_case(size_t T, size_t S, size_t hop, size_t mp, uint64_t pos, size_t n, int layout = 1, bool f32 = false,
                      bool scales = true, int xoff = 0, int yoff = 0, int boff = 0, bool nox = false, bool noy = false) {
  alignas(16) static char buf[64];
  const size_t cap = stream::ring_samples(T, mp);
  stream::Push g{};
  g.k = 777;
  const int rc = stream::check_push(T, S, hop, mp, cap, pos, nox ? nullptr : buf + xoff, layout, f32, scales, n,
                                    noy ? nullptr : buf + 16 + yoff, buf + 32 + boff, g);
  std::printf("push %zu %zu %zu %zu %" PRIu64 " %zu %d %d %d %d %d %d %d %d : %d", T, S, hop, mp, pos, n, layout, (int)f32,
              (int)scales, xoff, yoff, boff, (int)nox, (int)noy, rc);
  if (rc == NET_OK && n) {
    std::printf(" %zu %" PRIu64 " %lld %lld %d %d %zu %zu %zu", g.k, g.W0, g.first, g.hop, g.first_mod, g.p0, g.blocks,
                g.l1_items, g.items);
    CHECK(g.items <= stream::MAX_ITEMS && g.l1_items <= stream::MAX_ITEMS, "items past the limit");
    CHECK(g.p0 >= 0 && (size_t)g.p0 < cap && g.first_mod >= 0 && (size_t)g.first_mod < cap, "a ring position outside");
    // every onset of the push below 2^63, the last one's ring position inside two laps
    if (g.k) CHECK((uint64_t)g.first + (uint64_t)(g.k - 1) * (uint64_t)g.hop <= (uint64_t)INT64_MAX - T, "an onset past int64");
    if (g.k) CHECK((uint64_t)g.first_mod + (uint64_t)(g.k - 1) * (uint64_t)g.hop < 2 * cap, "more than one wrap");
  } else {
    CHECK(g.k == 777 || n == 0 || rc == NET_OK, "a refused push wrote its geometry");
  }
  std::printf("\n");
  g_cases++;
}

static void create_case(bool bank, size_t n_sets, const std::vector<int32_t>* sets, size_t S, size_t hop, size_t mp,
                        int device, bool out) {
  const int rc = stream::check_create(bank, n_sets, sets ? sets->data() : nullptr, S, hop, mp, device, out);
  std::printf("create %d %zu %d %zu %zu %zu %d %d : %d\n", (int)bank, n_sets, sets ? (int)sets->size() : -1, S, hop, mp,
              device, (int)out, rc);
  if (rc == NET_OK) {
    const size_t cap = stream::ring_samples(4096, mp);
    const stream::Alloc a = stream::alloc_of(S, cap);
    CHECK(a.ring == 32 * cap && a.origin == S * a.ring && a.origin % 8 == 0 && a.set == a.origin + 8 * S &&
              a.bytes == a.set + 4 * S && a.bytes / S >= a.ring,
          "the allocation of S %zu cap %zu", S, cap);
  }
  g_cases++;
}

// one seek check (the test hook's): the lists are printed, so the Python side restates the verdict
static void seek_case(bool group, bool each, bool fresh, size_t q, const std::vector<int64_t>* pos,
                      const std::vector<int64_t>* origin) {
  const size_t S = pos ? pos->size() : origin ? origin->size() : 3;
  const int rc = stream::check_seek(group, each, fresh, S, q, pos ? pos->data() : nullptr, origin ? origin->data() : nullptr);
  std::printf("seek %d %d %d %zu %zu %d %d", (int)group, (int)each, (int)fresh, q, S, (int)(pos != nullptr), (int)(origin != nullptr));
  if (pos) for (int64_t v : *pos) std::printf(" %" PRId64, v);
  if (origin) for (int64_t v : *origin) std::printf(" %" PRId64, v);
  std::printf(" : %d\n", rc);
  g_cases++;
}

int main() {
  const uint64_t I63 = (uint64_t)INT64_MAX;
  for (size_t T : {(size_t)64, (size_t)1125, (size_t)4096})
    for (size_t mp : {(size_t)0, (size_t)1, (size_t)2, (size_t)15, (size_t)16, (size_t)17, (size_t)37, (size_t)65535,
                      (size_t)65536, (size_t)65537, (size_t)1 << 32, SIZE_MAX})
      cap_case(T, mp);
  for (size_t T : {(size_t)64, (size_t)4096})
    for (size_t hop : {(size_t)0, (size_t)1, (size_t)3, T, T + 1, (size_t)1 << 40, (size_t)I63, (size_t)I63 + 1, SIZE_MAX})
      for (uint64_t pos : {(uint64_t)0, (uint64_t)1, (uint64_t)T - 1, (uint64_t)T, (uint64_t)T + 1, (uint64_t)1 << 40,
                           I63 - 65536, I63 - 1, I63, I63 + 1, UINT64_MAX - 65536, UINT64_MAX - 1, UINT64_MAX})
        for (size_t n : {(size_t)0, (size_t)1, (size_t)2, (size_t)37, (size_t)65536})
          k_case(T, hop, pos, n);
  // pushes: the position at both ends, at multiples of the ring and just around them
  for (size_t T : {(size_t)64, (size_t)4096})
    for (size_t mp : {(size_t)1, (size_t)37, (size_t)65536})
      for (size_t hop : {(size_t)1, (size_t)3, T + 7, (size_t)1 << 40, SIZE_MAX}) {
        const uint64_t cap = stream::ring_samples(T, mp);
        for (uint64_t pos : {(uint64_t)0, (uint64_t)T - 1, (uint64_t)T, cap - 1, cap, cap + 1, 7 * cap - 3, (uint64_t)1 << 40,
                             I63 - mp - 1, I63 - mp, I63 - mp + 1, I63 - 1, I63})
          for (size_t n : {(size_t)0, (size_t)1, mp, mp + 1})
            push_case(T, 5, hop, mp, pos, n);
      }
  // S k at the item limit: hop 1 makes k = n once pos >= T
  push_case(64, stream::MAX_ITEMS / 65536, 1, 65536, 1 << 20, 65536);
  push_case(64, stream::MAX_ITEMS, 1, 1, 1 << 20, 1);
  push_case(64, stream::MAX_ITEMS / 37, 1, 37, I63 - 37, 37);
  // the argument checks in their order
  push_case(64, 5, 3, 37, 100, 5, 2);                          // layout
  push_case(64, 5, 3, 37, 100, 5, -1);
  push_case(64, 5, 3, 37, 100, 5, 0);
  push_case(64, 5, 3, 37, 100, 5, 7, true);                    // the float entry ignores the layout
  push_case(64, 5, 3, 37, 100, 5, 1, true, false);             // no scales
  push_case(64, 5, 3, 37, 100, 5, 1, true, true, 2);           // misaligned float x
  push_case(64, 5, 3, 37, 100, 5, 1, false, true, 3);          // int8 x at any alignment
  push_case(64, 5, 3, 37, 100, 5, 1, false, true, 0, 2);       // misaligned y, k > 0
  push_case(64, 5, 3, 37, 10, 5, 1, false, true, 0, 2);        // misaligned y, k == 0
  push_case(64, 5, 3, 37, 10, 5, 1, false, true, 0, 0, 0, false, true);   // no y, k == 0
  push_case(64, 5, 3, 37, 100, 5, 1, false, true, 0, 0, 0, false, true);  // no y, k > 0
  push_case(64, 5, 3, 37, 100, 5, 1, false, true, 0, 0, 1);    // misaligned n_bad
  push_case(64, 5, 3, 37, 100, 5, 1, false, true, 0, 0, 0, true);  // no x
  push_case(64, 5, 3, 37, 100, 0, 9, false, true, 0, 0, 1, true);  // n == 0 comes first
  // create
  const std::vector<int32_t> good = {0, 1, 1, 3, 0}, neg = {0, -1, 0, 0, 0}, past = {0, 1, 5, 0, 0}, min = {INT32_MIN, 0, 0, 0, 0};
  create_case(true, 5, &good, 5, 3, 37, 0, true);
  create_case(false, 5, &good, 5, 3, 37, 0, true);
  create_case(true, 5, &good, 5, 3, 37, 0, false);
  create_case(true, 5, &good, 0, 3, 37, 0, true);
  create_case(true, 5, &good, 5, 0, 37, 0, true);
  create_case(true, 5, &good, 5, SIZE_MAX, 37, 0, true);
  for (size_t mp : {(size_t)0, (size_t)1, (size_t)65536, (size_t)65537, SIZE_MAX}) create_case(true, 5, &good, 5, 3, mp, 0, true);
  create_case(true, 5, &neg, 5, 3, 37, 0, true);
  create_case(true, 5, &past, 5, 3, 37, 0, true);
  create_case(true, 5, &min, 5, 3, 37, 0, true);
  create_case(true, 4, &good, 5, 3, 37, 0, true);  // set 3 of a bank of four is the last one
  create_case(true, 3, &good, 5, 3, 37, 0, true);
  create_case(true, 5, nullptr, 5, 3, 37, 0, true);
  for (int dev : {-1, 0, 63, 64}) create_case(true, 5, nullptr, 5, 3, 37, dev, true);
  for (size_t mp : {(size_t)1, (size_t)37, (size_t)65536})
    for (size_t S : {stream::MAX_ITEMS / mp - 1, stream::MAX_ITEMS / mp, stream::MAX_ITEMS / mp + 1, SIZE_MAX / mp, SIZE_MAX})
      create_case(true, 5, nullptr, S, 3, mp, 0, true);
  // seek: positions at both ends of each kind's range and around 2^31, 2^32 and 2^53, with and
  // without a decimator, origins at both ends of 0 .. D(pos) and one past them
  {
    using V = std::vector<int64_t>;
    const int64_t top = INT64_MAX, lim = stream::EACH_POS_LIMIT, raw = stream::EACH_RAW_LIMIT;
    const V edges = {0, 1, ((int64_t)1 << 31) - 1, (int64_t)1 << 31, ((int64_t)1 << 32) - 1, (int64_t)1 << 32,
                     ((int64_t)1 << 53) + 3 * ((int64_t)1 << 32) + 7, raw - 1, raw, raw + 1, lim - 1, lim, lim + 1, top - 1, top,
                     -1, INT64_MIN};
    for (size_t q : {(size_t)0, (size_t)1, (size_t)3, (size_t)16})
      for (int64_t p : edges) {
        const V same = {p, p, p}, mixed = {5, p, 5}, last = {p, p, p - (p > 0) + (p <= 0)};
        for (int each = 0; each < 2; each++) {
          seek_case(true, each, true, q, &same, nullptr);
          seek_case(true, each, true, q, &mixed, nullptr);
          seek_case(true, each, true, q, &last, nullptr);
        }
        if (p < 0) continue;
        const int64_t d = q ? (int64_t)stream::raw_decimated(q, (uint64_t)p) : p;
        const V o_lo = {0, 0, 0}, o_hi = {d, 0, d}, o_neg = {0, -1, 0}, o_min = {INT64_MIN, 0, 0};
        for (const V* o : {&o_lo, &o_hi, &o_neg, &o_min}) seek_case(true, false, true, q, &same, o);
        if (d < top) {
          const V o_past = {0, 0, d + 1};
          seek_case(true, false, true, q, &same, &o_past);
        }
        seek_case(true, true, true, q, &same, &o_lo);  // an each-group takes no origin
      }
    const V ok = {7, 7, 7}, zero = {0, 0, 0};
    for (int each = 0; each < 2; each++) {
      seek_case(false, each, true, 0, &ok, nullptr);
      seek_case(true, each, false, 0, &ok, nullptr);
      seek_case(true, each, true, 0, nullptr, nullptr);
      seek_case(true, each, true, 2, nullptr, &zero);
      seek_case(true, each, true, 2, &zero, nullptr);
    }
  }
  std::printf("cases %d\n", g_cases);
  if (g_bad) std::printf("%d checks failed\n", g_bad);
  return g_bad ? 1 : 0;
}
