// windows_bank_host_main.cpp — the layout and list arithmetic of the windows of a bank
// (bank::windows_starts, bank::windows_lists, csrc/bank_host.hpp) as a stand-alone program
// (tests/test_windows_bank_cpu.py builds it with -fsanitize=address,undefined and runs it).  The
// lists are written into heap arrays of exactly the size asked for, so a write past either end is an
// AddressSanitizer report; lengths near SIZE_MAX and INT64_MAX, where a sum or a rounding could
// wrap, must be refused, not computed.  Prints "cases <n>"; exits 0 when every check held.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "bank_host.hpp"

using namespace mib;

static int g_bad = 0, g_cases = 0;
#define CHECK(cond, ...) \
  do { \
    if (!(cond)) { \
      if (g_bad++ < 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    } \
  } while (0)

// One layout against its definition, the arrays sized exactly; then every capacity one short.
static void run_case(size_t T, size_t n_sets, const std::vector<size_t>& len, const std::vector<int32_t>& sets,
                     size_t hop) {
  const size_t R = len.size();
  std::vector<int64_t> starts(R);
  const size_t L = bank::windows_starts(len.data(), R, starts.data());
  CHECK(L == bank::windows_starts(len.data(), R, nullptr), "R %zu: L depends on starts", R);
  size_t at = 0, W = 0;
  for (size_t r = 0; r < R; r++) {
    CHECK((size_t)starts[r] == at && at % 16 == 0, "start %zu = %lld, want %zu", r, (long long)starts[r], at);
    W += len[r] < T ? 0 : (len[r] - T) / hop + 1;
    at = r + 1 == R ? at + len[r] : (at + len[r] + 15) / 16 * 16;
  }
  CHECK(L == at, "L %zu, want %zu", L, at);
  const size_t nb = (L + 15) / 16;
  CHECK(bank::windows_lists(T, n_sets, len.data(), sets.data(), R, hop, nullptr, 0, nullptr, 0, nullptr) == W,
        "the count without arrays");
  std::vector<int32_t> blk(nb, -9);
  std::vector<int64_t> on(W, -9);
  std::vector<size_t> first(R + 1, 77);
  CHECK(bank::windows_lists(T, n_sets, len.data(), sets.data(), R, hop, blk.data(), nb, on.data(), W, first.data()) == W,
        "the count with arrays");
  size_t i = 0;
  for (size_t r = 0; r < R; r++) {
    CHECK(first[r] == i, "first[%zu] = %zu, want %zu", r, first[r], i);
    const size_t hi = r + 1 == R ? nb : (size_t)starts[r + 1] / 16;
    for (size_t b = (size_t)starts[r] / 16; b < hi; b++) CHECK(blk[b] == sets[r], "block %zu of recording %zu", b, r);
    for (size_t k = 0; len[r] >= T && k <= (len[r] - T) / hop; k++, i++)
      CHECK(on[i] == starts[r] + (int64_t)(k * hop), "onset %zu", i);
  }
  CHECK(first[R] == W && i == W, "first[R] = %zu, W = %zu", first[R], W);
  // a capacity one short writes nothing of that list (the arrays are exactly that short)
  if (nb) {
    std::vector<int32_t> b1(nb - 1, -9);
    bank::windows_lists(T, n_sets, len.data(), sets.data(), R, hop, b1.data(), nb - 1, nullptr, 0, nullptr);
    for (int32_t v : b1) CHECK(v == -9, "a short blk_set was written");
  }
  if (W) {
    std::vector<int64_t> o1(W - 1, -9);
    bank::windows_lists(T, n_sets, len.data(), sets.data(), R, hop, nullptr, 0, o1.data(), W - 1, nullptr);
    for (int64_t v : o1) CHECK(v == -9, "a short onset list was written");
  }
  g_cases++;
}

static void refused(const char* what, size_t T, size_t n_sets, const std::vector<size_t>& len,
                    const std::vector<int32_t>& sets, size_t hop) {
  int32_t blk[4] = {-9, -9, -9, -9};
  int64_t on[4] = {-9, -9, -9, -9};
  size_t first[8] = {77, 77, 77, 77, 77, 77, 77, 77};
  const size_t W = bank::windows_lists(T, n_sets, len.empty() ? nullptr : len.data(), sets.empty() ? nullptr : sets.data(),
                                       len.size(), hop, blk, 4, on, 4, first);
  CHECK(W == 0, "%s: W = %zu", what, W);
  for (int i = 0; i < 4; i++) CHECK(blk[i] == -9 && on[i] == -9, "%s: a list was written", what);
  for (int i = 0; i < 8; i++) CHECK(first[i] == 77, "%s: first was written", what);
  g_cases++;
}

int main() {
  const size_t IMAX = (size_t)INT64_MAX;
  for (size_t T : {(size_t)64, (size_t)480})
    for (size_t hop : {(size_t)1, (size_t)3, (size_t)1000}) {
      run_case(T, 5, {T + 17, T, T - 1, T + 38, T + 9, T + 16, T + 31}, {0, 1, 1, 3, 4, 0, 2}, hop);
      run_case(T, 5, {T + 5}, {4}, hop);
      run_case(T, 1, {16, 32, T + 16}, {0, 0, 0}, hop);  // lengths that are multiples of 16: no pad
      run_case(T, 2, {1, 0, 15, T}, {1, 0, 1, 0}, hop);   // an empty recording takes no block
    }
  // the layout alone at the ends of the range
  int64_t st[3];
  CHECK(bank::windows_starts(nullptr, 0, st) == 0 && bank::windows_starts(nullptr, 3, st) == 0, "R == 0 or no lengths");
  const size_t one[1] = {IMAX};
  CHECK(bank::windows_starts(one, 1, st) == IMAX && st[0] == 0, "one recording of INT64_MAX samples");
  const size_t over[1] = {IMAX + 1};
  CHECK(bank::windows_starts(over, 1, st) == 0, "one recording past INT64_MAX");
  const size_t smax[2] = {SIZE_MAX, SIZE_MAX};
  CHECK(bank::windows_starts(smax, 2, st) == 0 && bank::windows_starts(smax, 1, nullptr) == 0, "SIZE_MAX");
  const size_t wrap[2] = {SIZE_MAX - 7, 8};  // the plain sum wraps to 0
  CHECK(bank::windows_starts(wrap, 2, st) == 0, "a sum that wraps");
  const size_t round_[2] = {IMAX - 7, 0};  // the rounding up to 16 passes INT64_MAX
  CHECK(bank::windows_starts(round_, 2, st) == 0, "a rounding past INT64_MAX");
  const size_t fits[2] = {IMAX - 15 - 16, 16};  // the largest two that fit: the second starts at 2^63 - 32
  {
    const size_t L = bank::windows_starts(fits, 2, st);
    CHECK(L == IMAX - 15 && st[1] == (int64_t)(IMAX - 31), "the largest layout: L %zu start %lld", L, (long long)st[1]);
  }
  const size_t last[2] = {16, IMAX - 15};  // ends at INT64_MAX + 1
  CHECK(bank::windows_starts(last, 2, st) == 0, "a last recording that ends past INT64_MAX");
  g_cases += 9;
  // the lists' refusals: nothing written
  refused("hop 0", 64, 5, {100, 100}, {0, 1}, 0);
  refused("R 0", 64, 5, {}, {}, 3);
  refused("a set at n_sets", 64, 5, {100, 100}, {0, 5}, 3);
  refused("a negative set", 64, 5, {100, 100}, {-1, 0}, 3);
  refused("INT32_MIN", 64, 5, {100}, {INT32_MIN}, 3);
  refused("overflow", 64, 5, {SIZE_MAX - 7, 8}, {0, 1}, 3);
  refused("past INT64_MAX", 64, 5, {IMAX, 1}, {0, 1}, 3);
  // a count that no array could hold is still only a count
  {
    const size_t len[1] = {IMAX};
    const int32_t s[1] = {0};
    const size_t W = bank::windows_lists(64, 1, len, s, 1, 1, nullptr, 0, nullptr, 0, nullptr);
    CHECK(W == IMAX - 63, "the windows of INT64_MAX samples: %zu", W);
    g_cases++;
  }
  std::printf("cases %d\n", g_cases);
  if (g_bad) std::printf("%d checks failed\n", g_bad);
  return g_bad ? 1 : 0;
}
