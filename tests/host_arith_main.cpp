// host_arith_main.cpp — the loader's host arithmetic as a stand-alone program (tests/
// test_host_sanitizers.py builds it with -fsanitize=address,undefined and runs it): loads the blobs
// named on the command line through the loader's own functions (parse_blob and build_set,
// images.hpp), each normally and on the general path, and prints what net_params_info would report
// with the FNV-1a digests of both images ("set <file> <normal|general> rc xr layer filter folded
// kernels-image window-image").  Then the header's dimension cases on the first blob and on a
// net_arrays_t of its arrays ("dims <cases>"), gen::carve_of over every geometry gen_supported admits
// ("carve <cases> max <bytes>"), and the requant searches swept over the factor classes, every
// proven form checked against 64-bit integer division at both ends of every output step.  Exits 0
// when every check held.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "images.hpp"
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

static std::vector<char> read_file(const char* path) {
  std::ifstream in(path, std::ios::binary);
  return std::vector<char>((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}

// net_params_load on the blob, normally and under mibminet_test_force_general
static void run_set(const char* path) {
  const std::vector<char> blob = read_file(path);
  for (const bool force : {false, true}) {
    HostParams hp;
    Image img, win;
    int rc = parse_blob(blob.data(), blob.size(), hp);
    if (rc == NET_OK) rc = build_set(hp, force, &img, &win);
    const bool named = rc == NET_OK && !hp.general && hp.xr;  // net_params_info: info[1], info[2]
    std::printf("set %s %s %d %d %d %d %d %016llx %016llx\n", path, force ? "general" : "normal", rc,
                rc == NET_OK && hp.xr ? 1 : 0, named ? hp.xr_layer : 0, named ? hp.xr_filter : -1, hp.folded,
                (unsigned long long)fnv1a(img), (unsigned long long)fnv1a(win));
  }
}

// A valid blob whose header claims other dimensions, and the same through a net_arrays_t: refused
// with a code, by both parsers, before anything is sized from them.
static void run_dims(const char* path) {
  const std::vector<char> blob = read_file(path);
  HostParams hp;
  CHECK(parse_blob(blob.data(), blob.size(), hp) == NET_OK, "%s does not parse", path);
  if (hp.l5_weight.empty()) return;
  net_arrays_t a = {hp.d.C, hp.d.T, hp.d.F1, hp.d.F2, hp.d.D, hp.d.N,
                    (hp.reorder_bn ? FLAG_REORDER_BN : 0) | (hp.clip_balanced ? FLAG_CLIP_BALANCED : 0),
                    hp.l1_factor.data(), hp.l1_offset.data(), hp.l1_weight_align.data(), hp.l2_factor.data(),
                    hp.l2_offset.data(), hp.l2_weight_reverse.data(), hp.l3_factor, hp.l3_weight.data(),
                    hp.l4_factor.data(), hp.l4_offset.data(), hp.l4_weight.data(), hp.l5_factor, hp.l5_bias.data(),
                    hp.l5_weight.data()};
  HostParams out;
  CHECK(parse_arrays(&a, out) == NET_OK, "%s: its arrays do not load", path);
  // (F1, F2, D, the arrays' code).  The last is refused by size before the arrays are looked at
  // (NET_ERR_UNSUPPORTED, F2 > 4096); as a blob its first array is longer than the blob.
  const int cases[4][4] = {{hp.d.F1, -16, -1, NET_ERR_BLOB},
                           {hp.d.F1, 0, 0, NET_ERR_BLOB},
                           {65536, 0, 65536, NET_ERR_BLOB},
                           {1 << 15, 1 << 30, 1 << 15, NET_ERR_UNSUPPORTED}};
  int n = 0;
  for (const auto& c : cases) {
    std::vector<char> bad = blob;
    const int32_t f1 = c[0], f2 = c[1], dd = c[2];  // header: magic, version, C, T, F1, F2, D
    std::memcpy(&bad[8 + 4 * 3], &f1, 4);
    std::memcpy(&bad[8 + 4 * 4], &f2, 4);
    std::memcpy(&bad[8 + 4 * 5], &dd, 4);
    HostParams b;
    const int rb = parse_blob(bad.data(), bad.size(), b);
    CHECK(rb == NET_ERR_BLOB, "blob F1 %d F2 %d D %d: rc %d", f1, f2, dd, rb);
    net_arrays_t aa = a;
    aa.F1 = f1; aa.F2 = f2; aa.D = dd;
    const int ra = parse_arrays(&aa, b);
    CHECK(ra == c[3], "arrays F1 %d F2 %d D %d: rc %d", f1, f2, dd, ra);
    n++;
  }
  std::printf("dims %d\n", n);
}

// gen::carve_of over every geometry gen_supported admits and the four layouts: inside the LDS, its
// areas in order, the staged trial (if any) behind them.  The dimensions are gen_geometry's.
static void run_carve() {
  static gen::GenParams g;
  long long cases = 0;
  int most = 0;
  Dims d;
  d.F1 = d.F2 = F2;
  d.D = 1;
  for (d.C = 1; d.C <= 64; d.C++)
    for (d.T = 64; d.T <= gen::TMAX; d.T++) {
      d.N = 1;
      CHECK(gen_supported(d) == NET_OK, "C %d T %d refused", d.C, d.T);
      gen_geometry(d, g);
      for (int N = 1; N <= gen::NMAX; N++)
        for (int layout = 0; layout < 4; layout++) {
          const gen::Carve c = gen::carve_of(g.C, g.T, N, g.T8, g.T64A, g.NB1, g.MT, g.NTT, layout);
          CHECK(c.bytes <= gen::LDS_MAX, "C %d T %d N %d layout %d: %d bytes", d.C, d.T, N, layout, c.bytes);
          CHECK(0 < c.y2 && c.y2 < c.y3 && c.y3 < c.y4 && c.y4 < c.sg && c.sg < c.w5 && c.w5 < c.stg && c.stg <= c.bytes,
                "C %d T %d N %d layout %d: areas out of order", d.C, d.T, N, layout);
          CHECK(c.raw < 0 || c.raw >= c.stg, "C %d T %d N %d layout %d: raw %d before stg %d", d.C, d.T, N, layout, c.raw,
                c.stg);
          most = std::max(most, c.bytes);
          cases++;
        }
    }
  std::printf("carve %lld max %d\n", cases, most);
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
  if (argc > 1) run_dims(argv[1]);
  run_carve();
  sweep();
  if (g_bad) std::printf("%d checks failed\n", g_bad);
  return g_bad ? 1 : 0;
}
