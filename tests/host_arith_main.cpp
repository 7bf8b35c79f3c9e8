// host_arith_main.cpp — the loader's host arithmetic as a stand-alone program (tests/
// test_host_sanitizers.py builds it with -fsanitize=address,undefined and runs it): parses the
// blobs named on the command line and runs range check, folding and requant plan on each as
// net_params_load does, then sweeps the requant searches over the factor classes and checks every
// proven form against 64-bit integer division at both ends of every output step.  Prints one line
// per blob ("set <file> rc xr layer filter folded") and exits 0 when every check held.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "params_host.hpp"
#include "requant_host.hpp"

using namespace mib;

static int g_bad = 0;
#define CHECK(cond, ...) \
  do { \
    if (!(cond)) { \
      if (g_bad++ < 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    } \
  } while (0)

static int64_t floor_div(int64_t a, int64_t b) {
  const int64_t q = a / b;
  return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q;
}

// what build_set (images.hpp) does with a parsed set, without the images
static void run_set(const char* path) {
  std::ifstream in(path, std::ios::binary);
  const std::vector<char> blob((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  HostParams hp;
  int rc = parse_blob(blob.data(), blob.size(), hp);
  Ranges rg;
  if (rc == NET_OK) rc = check_ranges(hp, rg);
  Plan pl;
  int folded = 0;
  if (rc == NET_OK) {
    pl = make_plan(hp, rg);
    if (pl.xr) {
      HostParams fh = hp;
      Ranges frg;
      const int n = fold_constant_filters(fh, rg);
      if (n > 0 && check_ranges(fh, frg) == NET_OK) {
        pl = make_plan(fh, frg);
        folded = n;
      }
    }
    CHECK(pl.l3_ok, "%s: layer 3 has no float form", path);
  }
  std::printf("set %s %d %d %d %d %d\n", path, rc, pl.xr ? 1 : 0, pl.xr ? pl.xr_layer : 0, pl.xr ? pl.xr_filter : -1, folded);
}

// both ends of every step interval of trunc(v / fac) = k (k0 <= k <= k1) inside |v| <= vmax
template <class F>
static void step_ends(int32_t fac, int64_t k0, int64_t k1, int64_t vmax, bool floor, F&& f) {
  const int64_t A = fac < 0 ? -(int64_t)fac : (int64_t)fac;
  for (int64_t k = k0; k <= k1; k++)
    for (int64_t v : {k * A - A, k * A - 1, k * A, k * A + 1, k * A + A - 1, k * A + A})
      for (int64_t s : {v, -v})
        if (s >= -vmax && s <= vmax) f(s, floor ? floor_div(s, fac) : s / fac);
}

static int sweep() {
  std::vector<int32_t> facs = {1, -1, INT32_MAX, -INT32_MAX, INT32_MIN};
  for (int k = 1; k <= 30; k++)
    for (int64_t f : {((int64_t)1 << k) - 1, ((int64_t)1 << k) + 1}) {
      facs.push_back((int32_t)f);
      facs.push_back((int32_t)-f);
    }
  int n_rec = 0, n_magic = 0, n_floor = 0;
  for (const int32_t fac : facs) {
    // the converted form (REORDER_BN layers 2 and 4, layer 5) and the magic form (layers 1 and 3)
    for (const int64_t vmax : {((int64_t)1 << 24) - 1, ((int64_t)1 << 22) - 1, (int64_t)16 * 128 * 128, (int64_t)100000}) {
      float r = 0, c = 0;
      if (choose_reciprocal(fac, &r, nullptr, 128, vmax)) {
        n_rec++;
        step_ends(fac, -129, 128, vmax, false, [&](int64_t v, int64_t want) {
          if (want < -129 || want > 128) return;
          CHECK(qf(v, r) == want, "reciprocal fac %d vmax %lld v %lld", fac, (long long)vmax, (long long)v);
        });
      }
      if (vmax < (1 << 22) && choose_reciprocal(fac, &r, &c, 128, vmax)) {
        n_magic++;
        CHECK((double)c == -12582912.0 * (double)r, "magic c of fac %d", fac);
        step_ends(fac, -129, 128, vmax, false, [&](int64_t v, int64_t want) {
          if (want < -129 || want > 128) return;
          const float g = floor_form(FMAGIC_I, v, r, c);  // the device's fma on the accumulator's bits
          CHECK(g == (float)v * r && (int64_t)(int32_t)g == want, "magic fac %d vmax %lld v %lld", fac, (long long)vmax,
                (long long)v);
        });
      }
    }
    // the floor form (plain layers 2 and 4)
    for (const int64_t emax : {(int64_t)127, (int64_t)1024})
      for (const int64_t vmax : {((int64_t)1 << 22) - 1, ((int64_t)1 << 20) + 12345, (int64_t)4000}) {
        int32_t mb = 0;
        float r = 0, c = 0;
        if (!choose_floor_form(fac, emax, vmax, &mb, &r, &c)) continue;
        n_floor++;
        step_ends(fac, -2, emax + 1, vmax, true, [&](int64_t x, int64_t fl) {
          const int64_t want = std::min(std::max(fl, (int64_t)0), emax);
          const float K = 12582912.0f, g = floor_form(mb, x, r, c);
          const float e = std::min(std::max(g, K), K + (float)emax) - K;
          CHECK((double)e == (double)want, "floor form fac %d emax %lld vmax %lld x %lld", fac, (long long)emax,
                (long long)vmax, (long long)x);
        });
      }
    // exact division: every int32 dividend is in its domain, except INT32_MIN / -1
    const XDiv xd = xdiv_consts(fac);
    auto one = [&](int64_t e, int64_t want) {
      if (e < INT32_MIN || e > INT32_MAX || (fac == -1 && e == INT32_MIN)) return;
      CHECK((int64_t)xdiv_host((int32_t)e, xd) == want, "xdiv %lld / %d", (long long)e, fac);
    };
    step_ends(fac, -130, 130, INT32_MAX, false, one);
    for (const int64_t e : {(int64_t)INT32_MIN, (int64_t)INT32_MIN + 1, (int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)INT32_MAX})
      one(e, e / fac);
  }
  std::printf("sweep %zu factors: %d reciprocals, %d magic forms, %d floor forms proven\n", facs.size(), n_rec, n_magic,
              n_floor);
  CHECK(n_rec > 0 && n_magic > 0 && n_floor > 0, "nothing proven");
  return 0;
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; i++) run_set(argv[i]);
  sweep();
  if (g_bad) std::printf("%d checks failed\n", g_bad);
  return g_bad ? 1 : 0;
}
