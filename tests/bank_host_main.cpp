// bank_host_main.cpp — the HIP-free part of a parameter bank as a stand-alone program (tests/
// test_bank_host_sanitizers.py builds it with -fsanitize=address,undefined and runs it).  The blobs
// named on the command line are one bank, built by bank::build, the function net_bank_create calls:
// the first set refused and its code are printed with, per set, whether it needs exact division
// when loaded alone (build_set on that blob, so the flags exist for a refused bank too).  A bank that
// is not mixed must hold, byte for byte, the window image each blob gets alone; in a mixed bank that
// holds for the sets that need exact division, and every promoted set must have xr = 1, no float
// form and no magic in a C-init, and the xdiv constants of its own plan.  Then bank::range_of is
// swept: the ranges of the G workgroups must tile [0, E) in order, each holding floor(E / G) or one
// more item.  Prints "bank <n> refused <i> rc <code> xr <flags>" and "ranges <cases>"; exits 0 when
// every check held.
#include <cstdio>
#include <cstring>
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
  const size_t ns = (size_t)n;
  std::vector<std::vector<char>> blobs(ns);
  std::vector<const void*> ptrs(ns);
  std::vector<size_t> sizes(ns);
  std::vector<float> scales(ns);
  // each set alone, as net_params_load would take it
  std::vector<HostParams> hps(ns);
  std::vector<Image> wins(ns);
  std::string flags;
  for (size_t i = 0; i < ns; i++) {
    std::ifstream in(paths[i], std::ios::binary);
    blobs[i].assign((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    ptrs[i] = blobs[i].data();
    sizes[i] = blobs[i].size();
    scales[i] = 1.0f + (float)i;
    Image img;
    int rc = parse_blob(ptrs[i], sizes[i], hps[i]);
    if (rc == NET_OK) rc = build_set(hps[i], false, &img, &wins[i]);
    CHECK(rc == NET_OK && wins[i].bytes == sizeof(gen::GenParams), "%s: rc %d", paths[i], rc);
    if (rc != NET_OK) return;
    flags += hps[i].xr ? '1' : '0';
  }
  std::vector<gen::GenParams> sets;
  std::vector<bank::Scale> sc;
  size_t failed = (size_t)-1;
  const int rc = bank::build(ptrs.data(), sizes.data(), scales.data(), ns, false, sets, sc, &failed);
  std::printf("bank %d refused %ld rc %d xr %s\n", n, rc ? (long)failed : -1L, rc, flags.c_str());
  CHECK((rc == NET_OK) == (failed == (size_t)-1), "rc %d with failed %zu", rc, failed);
  if (rc != NET_OK) return;
  CHECK(sets.size() == ns && sc.size() == ns, "%zu sets, %zu scales", sets.size(), sc.size());
  const bool mixed = flags.find('0') != std::string::npos && flags.find('1') != std::string::npos;
  for (size_t i = 0; i < ns; i++) {
    const gen::GenParams& g = sets[i];
    CHECK(sc[i].qs == scales[i] && sc[i].qy == 1.0f / scales[i], "%s: scale %g, %g", paths[i], sc[i].qs, sc[i].qy);
    if (!mixed || hps[i].xr) {
      CHECK(std::memcmp(&g, wins[i].data.get(), sizeof(g)) == 0, "%s: not the image it gets alone", paths[i]);
      continue;
    }
    // promoted: the exact-division form of a set whose float forms were all proven
    const HostParams& hp = hps[i];
    Ranges rg;
    CHECK(check_ranges(hp, rg) == NET_OK, "%s: ranges", paths[i]);
    const Plan pl = make_plan(hp, rg);
    CHECK(g.xr == 1, "%s: not exact after promotion", paths[i]);
    CHECK(g.l3_r == 0.0f && g.l3_c == 0.0f, "%s: layer 3 keeps a float form", paths[i]);
    CHECK(g.l3_m == pl.x3.m && g.l3_xs == pl.x3.xs && g.l5_m == pl.x5.m && g.l5_xs == pl.x5.xs,
          "%s: lost an xdiv constant of layer 3 or 5", paths[i]);
    for (int f = 0; f < F2; f++) {
      CHECK(g.l1_r[f] == 0.0f && g.l1_c[f] == 0.0f && g.l2_r[f] == 0.0f && g.l2_c[f] == 0.0f && g.sg.l4_r[f] == 0.0f &&
                g.sg.l4_c[f] == 0.0f,
            "%s: filter %d keeps a float form", paths[i], f);
      CHECK(g.l1_off[f] == hp.l1_offset[f] && g.l2_thr[f] == -(hp.l2_offset[f] >> 3) && g.sg.l4_ci[f] == 0,
            "%s: filter %d keeps a magic in its C-init", paths[i], f);
      CHECK(g.l1_m[f] == pl.x1[f].m && g.l1_xs[f] == pl.x1[f].xs && g.l2_m[f] == pl.x2[f].m &&
                g.l2_xs[f] == pl.x2[f].xs && g.sg.l4_m[f] == pl.x4[f].m && g.sg.l4_xs[f] == pl.x4[f].xs,
            "%s: filter %d lost an xdiv constant", paths[i], f);
    }
  }
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
