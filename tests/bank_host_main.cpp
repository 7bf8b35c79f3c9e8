// bank_host_main.cpp — the HIP-free part of a parameter bank as a stand-alone program (tests/
// test_bank_host_sanitizers.py builds it with -fsanitize=address,undefined and runs it).  The blobs
// named on the command line are one bank: each is parsed and range-checked as net_bank_create does,
// the agreement check names the first set that disagrees with set 0, and every set's plan is forced
// to the exact-division form, which must keep the xdiv constants and drop every float form.  Then
// bank::range_of is swept: the ranges of the G workgroups must tile [0, E) in order, each holding
// floor(E / G) or one more item.  Prints "bank <n> mismatch <i> xr <flags>" and "ranges <cases>";
// exits 0 when every check held.
#include <cstdio>
#include <fstream>
#include <iterator>
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

static void run_bank(int n, char** paths) {
  std::vector<HostParams> hps((size_t)n);
  std::vector<const HostParams*> ptrs;
  std::string flags;
  for (int i = 0; i < n; i++) {
    std::ifstream in(paths[i], std::ios::binary);
    const std::vector<char> blob((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    HostParams& hp = hps[(size_t)i];
    int rc = parse_blob(blob.data(), blob.size(), hp);
    Ranges rg;
    if (rc == NET_OK) rc = check_ranges(hp, rg);
    CHECK(rc == NET_OK, "%s: rc %d", paths[i], rc);
    if (rc != NET_OK) continue;
    ptrs.push_back(&hp);
    const Plan was = make_plan(hp, rg);
    Plan pl = was;
    bank::force_exact(hp, pl);
    flags += was.xr ? '1' : '0';
    CHECK(pl.xr, "%s: not exact after force_exact", paths[i]);
    for (int f = 0; f < F2; f++) {
      CHECK(pl.f1[f].r == 0.0f && pl.f1[f].c == 0.0f && pl.f2[f].r == 0.0f && pl.f2[f].mbits == 0 &&
                pl.f4[f].r == 0.0f && pl.f4[f].mbits == 0,
            "%s: filter %d keeps a float form", paths[i], f);
      CHECK(pl.ci1[f] == hp.l1_offset[f] && pl.ci2[f] == (hp.l2_offset[f] >> 3) && pl.ci4[f] == (hp.l4_offset[f] >> 3),
            "%s: filter %d keeps a magic in its C-init", paths[i], f);
      CHECK(pl.x1[f].m == was.x1[f].m && pl.x1[f].xs == was.x1[f].xs && pl.x2[f].m == was.x2[f].m &&
                pl.x4[f].m == was.x4[f].m && pl.x3.m == was.x3.m && pl.x5.m == was.x5.m,
            "%s: filter %d lost an xdiv constant", paths[i], f);
    }
    if (was.xr) CHECK(pl.xr_layer == was.xr_layer && pl.xr_filter == was.xr_filter, "%s: an exact plan changed", paths[i]);
  }
  const long mm = (int)ptrs.size() == n ? bank::first_mismatch(ptrs.data(), ptrs.size()) : -2;
  std::printf("bank %d mismatch %ld xr %s\n", n, mm, flags.c_str());
}

static void run_ranges() {
  int cases = 0;
  for (unsigned G : {1u, 3u, 512u})
    for (unsigned long long E : {0ull, 1ull, (unsigned long long)G - 1, (unsigned long long)G, (unsigned long long)G + 1,
                                 (1ull << 31) - 65536}) {
      long long at = 0;
      for (unsigned w = 0; w < G; w++) {
        const bank::Range64 r = bank::range_of(w, G, E);
        CHECK(r.lo == at && r.hi >= r.lo, "G %u E %llu w %u: [%lld, %lld) after %lld", G, E, w, r.lo, r.hi, at);
        const long long n = r.hi - r.lo, q = (long long)(E / G);
        CHECK(n == q || n == q + 1, "G %u E %llu w %u: %lld items", G, E, w, n);
        at = r.hi;
      }
      CHECK(at == (long long)E, "G %u E %llu: the ranges end at %lld", G, E, at);
      cases++;
    }
  std::printf("ranges %d\n", cases);
}

int main(int argc, char** argv) {
  if (argc > 1) run_bank(argc - 1, argv + 1);
  run_ranges();
  if (g_bad) std::printf("%d checks failed\n", g_bad);
  return g_bad ? 1 : 0;
}
