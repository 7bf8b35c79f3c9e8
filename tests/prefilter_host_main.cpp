// prefilter_host_main.cpp — the host checks and the allocation of a stream group's prefilter
// (csrc/stream_host.hpp) as a stand-alone program (tests/test_prefilter_host_sanitizers.py builds it
// with -fsanitize=address,undefined and runs it).  It walks check_set_prefilter through every refusal,
// in the documented order, against a restatement written here, with coefficient arrays of exactly
// 5 M floats (a read past them, or of any of them before M is known to be in range, would be an
// AddressSanitizer report), and holds alloc_prefilter's offsets and total to 128-bit arithmetic over
// the corners of S, R, M, q and max_push, S max_push at its limit among them.  Every case is printed,
// one per line; the Python side compares each with its own restatement in unbounded integers.  Prints
// "cases <n>" last; exits 0 when every check here held.
#include <cinttypes>
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

// what: 0 finite coefficients, 1 a NaN, 2 +inf, 3 -inf (at coefficient `at`), 4 no array
static void set_case(bool group, bool decim, bool have, bool pushed, size_t M, int what, size_t at = 0) {
  const bool in_range = M >= 1 && M <= stream::MAX_SECTIONS;
  std::vector<float> c(in_range ? 5 * M : 1, 0.25f);  // exactly what the callee may read
  if (what == 1) c[at] = std::numeric_limits<float>::quiet_NaN();
  if (what == 2) c[at] = std::numeric_limits<float>::infinity();
  if (what == 3) c[at] = -std::numeric_limits<float>::infinity();
  const int rc = stream::check_set_prefilter(group, decim, have, pushed, what == 4 ? nullptr : c.data(), M);
  // the documented order, restated: the group; its state; M; the array; the coefficients
  int want = NET_OK;
  if (!group) want = NET_ERR_INVALID;
  else if (!decim || have || pushed) want = NET_ERR_INVALID;
  else if (!in_range) want = NET_ERR_INVALID;
  else if (what == 4) want = NET_ERR_INVALID;
  else if (what != 0) want = NET_ERR_INVALID;
  CHECK(rc == want, "group %d decim %d have %d pushed %d M %zu what %d: %d, want %d", (int)group, (int)decim, (int)have,
        (int)pushed, M, what, rc, want);
  std::printf("set %d %d %d %d %zu %d : %d\n", (int)group, (int)decim, (int)have, (int)pushed, M, what, rc);
  g_cases++;
}

static void alloc_case(size_t S, size_t R, size_t M, size_t q, size_t mp) {
  const stream::AllocPrefilter a = stream::alloc_prefilter(S, R, M, q, mp);
  typedef unsigned __int128 u128;
  const u128 per_state = (u128)8 * M * R, states = (u128)S * per_state;
  const u128 scratch = (states + 255) / 256 * 256, per_scratch = (u128)4 * q * mp * R;
  const u128 bytes = scratch + (u128)S * per_scratch;
  CHECK(bytes <= (u128)SIZE_MAX, "the total does not fit size_t");
  CHECK(a.state == 0 && (u128)a.per_state == per_state && (u128)a.scratch == scratch && (u128)a.per_scratch == per_scratch &&
            (u128)a.bytes == bytes,
        "S %zu R %zu M %zu q %zu mp %zu", S, R, M, q, mp);
  CHECK(a.scratch % 256 == 0 && a.per_state % 4 == 0 && a.per_scratch % 4 == 0, "alignment");
  // the last session's last state and last scratch float lie inside
  CHECK((u128)a.state + (u128)S * a.per_state <= (u128)a.scratch && (u128)a.scratch + (u128)S * a.per_scratch == (u128)a.bytes,
        "the arrays overlap or pass the end");
  std::printf("alloc %zu %zu %zu %zu %zu : %zu %zu %zu %zu %zu\n", S, R, M, q, mp, a.state, a.per_state, a.scratch,
              a.per_scratch, a.bytes);
  g_cases++;
}

int main() {
  std::printf("max %zu\n", stream::MAX_SECTIONS);
  g_cases++;
  // every refusal in its order: each one with everything that comes later wrong as well
  set_case(false, false, true, true, 0, 4);
  set_case(false, true, false, false, 3, 0);
  set_case(true, false, false, false, 3, 0);
  set_case(true, false, true, true, 0, 4);
  set_case(true, true, true, false, 3, 0);
  set_case(true, true, false, true, 3, 0);
  set_case(true, true, true, false, 9, 4);
  for (size_t M : {(size_t)0, (size_t)1, (size_t)2, (size_t)3, (size_t)7, (size_t)8, (size_t)9, (size_t)1 << 40, SIZE_MAX,
                   SIZE_MAX / 5 + 1, SIZE_MAX / 5 + 2})
    for (int what : {0, 1, 4}) set_case(true, true, false, false, M, what);
  for (size_t M : {(size_t)1, (size_t)3, (size_t)8})
    for (int what : {1, 2, 3})
      for (size_t at : {(size_t)0, (size_t)3, 5 * M - 1}) set_case(true, true, false, false, M, what, at);
  // the allocation at the corners
  for (size_t mp : {(size_t)1, (size_t)16, (size_t)37, (size_t)65536})
    for (size_t S : {(size_t)1, (size_t)5, (size_t)1024, stream::MAX_ITEMS / mp})
      for (size_t R : {(size_t)1, (size_t)22, (size_t)64})
        for (size_t M : {(size_t)1, (size_t)3, (size_t)8})
          for (size_t q : {(size_t)1, (size_t)4, (size_t)16}) alloc_case(S, R, M, q, mp);
  std::printf("cases %d\n", g_cases);
  if (g_bad) std::printf("%d checks failed\n", g_bad);
  return g_bad ? 1 : 0;
}
