// widen_host_main.cpp — net_blob_widen's transform (widen_blob, csrc/params_host.hpp) as a
// stand-alone program (tests/test_widen_host_sanitizers.py builds it with -fsanitize=address,undefined
// and runs it).  usage: widen_host_main <blob file> <R> <seed>.  Every buffer the transform is given
// is a heap block of exactly the size it is told, so a read or write past it is a sanitizer report:
//   * every truncation of the blob, and the blob with a byte appended, a spoilt magic, version, flag
//     word and weight width: NET_ERR_BLOB, whatever R and the channels are, *out_len untouched;
//   * R at -1, 0, C - 1, 65 and INT_MAX, a NULL channel list, an entry at -1, R and INT_MIN, a
//     duplicate: NET_ERR_INVALID, *out_len untouched;
//   * the size query; cap one byte short (refused, the size reported, the output untouched); cap exact;
//   * R = C with the identity gives the blob back; R = 64 with rows 0 and 63 in use;
//   * a seeded map into R rows: the output parses, C is R, column channels[c] of its layer-1 weights
//     is column c of the input's, every other column zero, every other field and byte equal.
// Prints "widen C <C> R <R> wbits <b> bytes <in> -> <out> checks <n>"; exits 0 when every check held.
#include <cinttypes>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <vector>

#include "params_host.hpp"

using namespace mib;

static int g_bad = 0, g_checks = 0;
#define CHECK(cond, ...) \
  do { \
    g_checks++; \
    if (!(cond)) { \
      if (g_bad++ < 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    } \
  } while (0)

// a heap copy of exactly n bytes (n == 0: a one-byte block nobody may read)
static std::unique_ptr<uint8_t[]> exact(const uint8_t* p, size_t n) {
  std::unique_ptr<uint8_t[]> b(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(b.get(), p, n);
  return b;
}

static const size_t UNTOUCHED = 0x5A5A5A5A;

// widen_blob on exact-size copies of the blob and of the channel list (nch entries)
static int widen(const std::vector<uint8_t>& blob, int R, const std::vector<int32_t>* ch, std::vector<uint8_t>* out,
                 size_t cap, size_t* out_len) {
  const auto b = exact(blob.data(), blob.size());
  std::unique_ptr<int32_t[]> c;
  if (ch) {
    c.reset(new int32_t[ch->size() ? ch->size() : 1]);
    std::copy(ch->begin(), ch->end(), c.get());
  }
  std::unique_ptr<uint8_t[]> o;
  if (out) {
    o.reset(new uint8_t[cap ? cap : 1]);
    std::memset(o.get(), 0xAA, cap ? cap : 1);
  }
  *out_len = UNTOUCHED;
  const int rc = widen_blob(b.get(), blob.size(), R, c.get(), o.get(), cap, out_len);
  if (out) out->assign(o.get(), o.get() + cap);
  return rc;
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  const std::vector<uint8_t> blob((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  const int R = std::atoi(argv[2]);
  unsigned seed = (unsigned)std::atoi(argv[3]);
  HostParams hp;
  if (parse_blob(blob.data(), blob.size(), hp) != NET_OK) return 2;
  const Dims d = hp.d;
  const int C = d.C;
  if (C > R || R > 64) return 2;

  // a seeded map: C distinct rows of R, shuffled
  std::vector<int32_t> ch(R);
  for (int i = 0; i < R; i++) ch[i] = i;
  for (int i = R - 1; i > 0; i--) {
    seed = seed * 1664525u + 1013904223u;
    std::swap(ch[i], ch[(seed >> 8) % (unsigned)(i + 1)]);
  }
  ch.resize(C);
  size_t n = 0;
  std::vector<uint8_t> out;

  // ---- malformed and truncated blobs: the parser's verdict, before R and the channels are looked at
  for (size_t len = 0; len < blob.size(); len += (len < 200 || len + 200 > blob.size()) ? 1 : 97) {
    const std::vector<uint8_t> cut(blob.begin(), blob.begin() + (long)len);
    for (int r : {R, 0}) {
      CHECK(widen(cut, r, &ch, &out, blob.size() + 4096, &n) == NET_ERR_BLOB && n == UNTOUCHED, "truncated to %zu", len);
    }
    CHECK(widen(cut, R, nullptr, nullptr, 0, &n) == NET_ERR_BLOB && n == UNTOUCHED, "truncated to %zu, no list", len);
  }
  {
    std::vector<uint8_t> b = blob;
    b.push_back(0);
    CHECK(widen(b, R, &ch, &out, b.size() + 4096, &n) == NET_ERR_BLOB, "a byte appended");
    for (size_t at : {(size_t)0, (size_t)8, (size_t)36, (size_t)40, (size_t)44, (size_t)48, (size_t)51}) {
      b = blob;
      b[at] ^= 0x10;  // magic, version, weight_bits, l2_taps, l3_taps, flags (low and high byte)
      CHECK(widen(b, R, &ch, &out, b.size() + 4096, &n) == NET_ERR_BLOB && n == UNTOUCHED, "byte %zu spoilt", at);
    }
    // a header that promises more channels than the blob holds, or than any list could name
    for (uint32_t c : {(uint32_t)C + 4, (uint32_t)65, (uint32_t)INT32_MAX, (uint32_t)0, (uint32_t)0x80000000u}) {
      b = blob;
      std::memcpy(&b[12], &c, 4);
      const int rc = widen(b, R, &ch, &out, b.size() + 4096, &n);
      CHECK(rc == NET_ERR_BLOB && n == UNTOUCHED, "C = %u in the header: %d", c, rc);
    }
  }

  // ---- R and the channels at their limits
  for (int r : {-1, 0, C - 1, 65, INT_MAX, INT_MIN}) {
    CHECK(widen(blob, r, &ch, &out, blob.size() + 4096, &n) == NET_ERR_INVALID && n == UNTOUCHED, "R = %d", r);
  }
  CHECK(widen(blob, R, nullptr, &out, blob.size() + 4096, &n) == NET_ERR_INVALID && n == UNTOUCHED, "no list");
  for (int i : {0, C - 1}) {
    for (int32_t v : {(int32_t)-1, (int32_t)R, (int32_t)64, INT32_MAX, INT32_MIN}) {
      std::vector<int32_t> c = ch;
      c[i] = v;
      CHECK(widen(blob, R, &c, &out, blob.size() + 4096, &n) == NET_ERR_INVALID && n == UNTOUCHED, "channels[%d] = %d", i, v);
    }
  }
  if (C > 1) {
    std::vector<int32_t> c = ch;
    c[C - 1] = c[0];
    CHECK(widen(blob, R, &c, &out, blob.size() + 4096, &n) == NET_ERR_INVALID && n == UNTOUCHED, "a duplicate");
  }

  // ---- the size query, cap one byte short, cap exact
  const size_t CA = (size_t)d.C_ALIGN(), RA = ((size_t)R + 3) & ~(size_t)3, F2n = (size_t)d.F2;
  const size_t need = blob.size() + F2n * (RA - CA) * (size_t)d.wbits / 8;
  CHECK(widen(blob, R, &ch, nullptr, 0, &n) == NET_OK && n == need, "size query: %zu, want %zu", n, need);
  CHECK(widen_blob(blob.data(), blob.size(), R, ch.data(), nullptr, 0, nullptr) == NET_OK, "size query, no out_len");
  CHECK(widen(blob, R, &ch, &out, need - 1, &n) == NET_ERR_INVALID && n == need, "one byte short: %zu", n);
  bool clean = true;
  for (uint8_t v : out) clean = clean && v == 0xAA;
  CHECK(clean, "a refused call wrote to out");
  const int rc = widen(blob, R, &ch, &out, need, &n);
  CHECK(rc == NET_OK && n == need && out.size() == need, "exact cap: %d", rc);
  if (rc != NET_OK) return 1;

  // ---- the output: C := R, the columns scattered, everything else the input's
  HostParams wp;
  CHECK(parse_blob(out.data(), out.size(), wp) == NET_OK, "the output does not parse");
  CHECK(wp.d.C == R && wp.d.T == d.T && wp.d.F1 == d.F1 && wp.d.F2 == d.F2 && wp.d.D == d.D && wp.d.N == d.N &&
            wp.d.wbits == d.wbits && wp.reorder_bn == hp.reorder_bn && wp.clip_balanced == hp.clip_balanced,
        "header");
  std::vector<int> from(RA, -1);
  for (int c = 0; c < C; c++) from[(size_t)ch[c]] = c;
  bool cols = wp.l1_weight_align.size() == F2n * RA;
  for (size_t f = 0; cols && f < F2n; f++)
    for (size_t r = 0; r < RA; r++)
      cols = cols && wp.l1_weight_align[f * RA + r] == (from[r] < 0 ? 0 : hp.l1_weight_align[f * CA + (size_t)from[r]]);
  CHECK(cols, "layer-1 columns");
  CHECK(wp.l1_factor == hp.l1_factor && wp.l1_offset == hp.l1_offset && wp.l2_factor == hp.l2_factor &&
            wp.l2_offset == hp.l2_offset && wp.l2_weight_reverse == hp.l2_weight_reverse && wp.l3_factor == hp.l3_factor &&
            wp.l3_weight == hp.l3_weight && wp.l4_factor == hp.l4_factor && wp.l4_offset == hp.l4_offset &&
            wp.l4_weight == hp.l4_weight && wp.l5_factor == hp.l5_factor && wp.l5_bias == hp.l5_bias &&
            wp.l5_weight == hp.l5_weight,
        "the other fields");
  const size_t at = (size_t)HEADER_SIZE + 8 * F2n, oldb = F2n * CA * (size_t)d.wbits / 8, newb = F2n * RA * (size_t)d.wbits / 8;
  CHECK(std::memcmp(out.data(), blob.data(), 12) == 0 && std::memcmp(&out[16], &blob[16], at - 16) == 0 &&
            std::memcmp(&out[at + newb], &blob[at + oldb], blob.size() - at - oldb) == 0,
        "bytes outside the header's C and the layer-1 weights");
  // the reachable ranges are the same: the same verdict of the range check, the same plan
  {
    Ranges ra, rb;
    const int va = check_ranges(hp, ra), vb = check_ranges(wp, rb);
    CHECK(va == vb, "range verdicts %d, %d", va, vb);
    if (va == NET_OK && vb == NET_OK) {
      CHECK(std::memcmp(&ra, &rb, sizeof(Ranges)) == 0, "reachable ranges");
      const Plan pa = make_plan(hp, ra), pb = make_plan(wp, rb);
      CHECK(pa.xr == pb.xr && pa.xr_layer == pb.xr_layer && pa.xr_filter == pb.xr_filter, "requant path");
    }
  }

  // ---- R = C with the identity: the blob back; R = 64 with rows 0 and 63 in use
  {
    std::vector<int32_t> id(C);
    for (int c = 0; c < C; c++) id[c] = c;
    CHECK(widen(blob, C, &id, &out, blob.size(), &n) == NET_OK && n == blob.size() && out == blob, "identity");
    std::vector<int32_t> c64 = id;
    c64[0] = 63;
    if (C > 1) c64[C - 1] = 0;
    const size_t need64 = blob.size() + F2n * (64 - CA) * (size_t)d.wbits / 8;
    CHECK(widen(blob, 64, &c64, &out, need64, &n) == NET_OK && n == need64, "R = 64");
    HostParams p64;
    CHECK(parse_blob(out.data(), out.size(), p64) == NET_OK && p64.d.C == 64, "R = 64 parses");
    bool ok = p64.l1_weight_align.size() == F2n * 64;
    for (size_t f = 0; ok && f < F2n; f++) ok = p64.l1_weight_align[f * 64 + 63] == hp.l1_weight_align[f * CA];
    CHECK(ok, "R = 64, row 63");
  }
  std::printf("widen C %d R %d wbits %d bytes %zu -> %zu checks %d\n", C, R, d.wbits, blob.size(), need, g_checks);
  return g_bad ? 1 : 0;
}
