// bank_replace_host_main.cpp — the decision part of net_bank_replace as a stand-alone program (tests/
// test_bank_replace_host_sanitizers.py builds it with -fsanitize=address,undefined and runs it).
//   bank_replace_host_main <has_scales 0|1> <n> <blob> x n  [<slot> <blob> <scale>] ...
// The first n blobs are a bank, built by bank::build with its creation record; every triple after
// them is one replacement, decided by bank::replace_set, the function net_bank_replace calls, on a
// candidate of its own and installed into the slot only when it is accepted, as mibminet.hip does.
// After each accepted one the whole bank is held, byte for byte, to a bank freshly built from the
// list of blobs as it now stands (where that bank runs the same kernel form), the slot's scale entry
// to the scale and its reciprocal, and the head of the image (all before gen::GenParams::l3_m, which
// other threads read unlocked) to what it was; after each refused one to what it was before.  Prints
// "bank <n> rc <code> xr <0|1>" and per replacement "replace <slot> rc <code>"; exits 0 when every
// check held.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "bank_host.hpp"

using namespace mib;

static int g_bad = 0;
#define CHECK(cond, ...) \
  do { \
    if (!(cond)) { \
      if (g_bad++ < 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    } \
  } while (0)

static std::vector<char> slurp(const char* path) {
  std::ifstream in(path, std::ios::binary);
  return std::vector<char>((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}

static bool same(const std::vector<gen::GenParams>& a, const std::vector<gen::GenParams>& b) {
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(gen::GenParams)) == 0;
}

static bool same(const std::vector<bank::Scale>& a, const std::vector<bank::Scale>& b) {  // (empty: no pointer)
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(bank::Scale)) == 0);
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const bool has_scales = std::atoi(argv[1]) != 0;
  const size_t n = (size_t)std::atoi(argv[2]);
  if (n == 0 || (size_t)argc < 3 + n || (argc - 3 - (int)n) % 3 != 0) return 2;
  std::vector<std::vector<char>> blobs(n);
  std::vector<float> scales(n);
  for (size_t i = 0; i < n; i++) {
    blobs[i] = slurp(argv[3 + i]);
    scales[i] = 1.0f + (float)i;
  }
  auto lists = [&](std::vector<const void*>& ptrs, std::vector<size_t>& sizes) {
    ptrs.clear();
    sizes.clear();
    for (const auto& b : blobs) {
      ptrs.push_back(b.data());
      sizes.push_back(b.size());
    }
  };
  std::vector<const void*> ptrs;
  std::vector<size_t> sizes;
  lists(ptrs, sizes);
  std::vector<gen::GenParams> sets;
  std::vector<bank::Scale> sc;
  bank::Record rec;
  const int rc = bank::build(ptrs.data(), sizes.data(), has_scales ? scales.data() : nullptr, n, false, sets, sc, nullptr,
                             &rec);
  std::printf("bank %zu rc %d xr %d\n", n, rc, rc == NET_OK && rec.xr ? 1 : 0);
  if (rc != NET_OK) return g_bad ? 1 : 0;
  CHECK(rec.has_scales == has_scales && rec.d.C == sets[0].C && rec.d.T == sets[0].T && rec.d.N == sets[0].N &&
            (int)rec.xr == sets[0].xr,
        "the record is not the bank's");
  constexpr size_t HEAD = offsetof(gen::GenParams, l3_m);
  for (int a = 3 + (int)n; a < argc; a += 3) {
    const size_t slot = (size_t)std::atoi(argv[a]);
    std::vector<char> blob = slurp(argv[a + 1]);
    const float scale = (float)std::atof(argv[a + 2]);
    const std::vector<gen::GenParams> before = sets;
    const std::vector<bank::Scale> sc_before = sc;
    auto cand = std::make_unique<gen::GenParams>();
    bank::Scale cs{};
    const int rr = slot < n ? bank::replace_set(rec, blob.data(), blob.size(), scale, *cand, cs) : NET_ERR_INVALID;
    std::printf("replace %zu rc %d\n", slot, rr);
    if (rr != NET_OK) {
      CHECK(same(sets, before) && same(sc, sc_before), "a refused replacement changed the bank");
      continue;
    }
    CHECK(std::memcmp(cand.get(), &sets[slot], HEAD) == 0, "slot %zu: the head of the image changed", slot);
    sets[slot] = *cand;
    if (has_scales) sc[slot] = cs;
    // the caller may free its blob at once: nothing of the candidate points into it
    std::vector<char>(blob.size(), (char)0x5A).swap(blob);
    blobs[slot] = slurp(argv[a + 1]);
    scales[slot] = scale;
    for (size_t i = 0; i < n; i++)
      if (i != slot)
        CHECK(std::memcmp(&sets[i], &before[i], sizeof(gen::GenParams)) == 0, "slot %zu changed set %zu", slot, i);
    if (has_scales)
      CHECK(sc[slot].qs == scale && sc[slot].qy == 1.0f / scale, "slot %zu: scale %g, %g", slot, sc[slot].qs, sc[slot].qy);
    else
      CHECK(cs.qs == 0.0f && cs.qy == 0.0f, "a bank without scales got one");
    std::vector<gen::GenParams> fresh;
    std::vector<bank::Scale> fsc;
    bank::Record frec;
    lists(ptrs, sizes);
    const int fr = bank::build(ptrs.data(), sizes.data(), has_scales ? scales.data() : nullptr, n, false, fresh, fsc, nullptr,
                               &frec);
    CHECK(fr == NET_OK, "the new list builds no bank: rc %d", fr);
    if (fr == NET_OK && frec.xr == rec.xr) {
      CHECK(same(sets, fresh), "slot %zu: not the bank freshly built from the new list", slot);
      CHECK(same(fsc, sc), "slot %zu: not the scales of the fresh bank", slot);
    }
  }
  if (g_bad) std::printf("%d checks failed\n", g_bad);
  return g_bad ? 1 : 0;
}
