// image_layout.hpp — the layouts of everything the host writes and the kernels read: the two
// parameter images (DevParams of the compiled geometries, gen::GenParams of the run-time-dimension
// kernels), the LDS carve both sides compute alike, and a bank's scale entry.  HIP-free (no runtime
// header, no device function): included by images.hpp, bank_host.hpp and device_state.hpp on the
// host side, by forward_common.hpp, forward_gen.hpp and forward_bank.hpp on the kernels' side, and
// through images.hpp by the stand-alone host programs (tests/host_arith_main.cpp,
// tests/bank_host_main.cpp).
#pragma once
#include <stdint.h>

#include "net_consts.hpp"  // F2, N_OUT

// host and device under hipcc, plain otherwise
#ifdef __HIPCC__
#define MIB_HD __host__ __device__
#else
#define MIB_HD
#endif

namespace mib {

// Four dwords, the unit of every operand fragment.  Off clang the same 16 bytes as a GCC vector.
#ifdef __clang__
typedef int v4i __attribute__((ext_vector_type(4)));
#else
typedef int v4i __attribute__((vector_size(16)));
#endif
static_assert(sizeof(v4i) == 16 && alignof(v4i) == 16, "a fragment is 16 aligned bytes");

constexpr int ND5_MAX = 96;     // dwords of the layer-4 output [F2][T64_ALIGN] (F2*T64_ALIGN <= 384)
// REORDER_BN pooling bias: the layer-2 MFMA chains start from a bias B (the bits of a
// float MFMA srcC inline constant), so every conv value a lies at a + B with no wrap (|a| < 2^22),
// and max(a, thr) - thr = sat_u32((a + B) - (thr + B)): one full-rate v_sub_u32 clamp per element
// instead of a quarter-rate v_max_i32 (tools/vthru.hip: 2.45 vs 4.21 SIMD cycles).  Each chain
// gets a constant of its own (filter slot 0: 1.0, slot 1: 2.0, the tail: 4.0): a constant shared
// by two chains is hoisted into a 16-register tuple instead of riding in the instruction.
// (layer 4 uses 0.5, -0.5 and -1.0: forward_wg.hpp, bias4)
MIB_HD constexpr int pbias(int slot) { return slot == 0 ? 0x3F800000 : slot == 1 ? 0x40000000 : 0x40800000; }
constexpr int PBIAS_TAIL = pbias(2);

MIB_HD constexpr int align16(int x) { return (x + 15) & ~15; }
MIB_HD constexpr int cmax(int a, int b) { return a > b ? a : b; }
MIB_HD constexpr int cmin(int a, int b) { return a < b ? a : b; }
// smallest multiple of 4 >= x whose dword count is odd (conflict-free strided dword reads)
MIB_HD constexpr int odd_dwords(int x) { return ((x + 3) / 4 % 2) ? (x + 3) / 4 * 4 : (x + 3) / 4 * 4 + 4; }

// Parameters read into LDS by every workgroup.
struct SmallParams {
  v4i l4_bfrag[64];       // layer-4 B operand per lane (block diagonal, see host)
  v4i l2_tpar[F2];        // layer-2 tail per filter: {PBIAS_TAIL + thr, off + 8 thr, bits of r, 0}
                          // (thr = -(net_l2_offset >> 3); off + 8 thr = net_l2_offset & 7);
                          // XR: {.., .., xdiv magic, shift word}
  int l4_thr[F2];         // -(net_l4_offset >> 3), clamped to the conv range (images.hpp)
  int l4_offm[F2];        // net_l4_offset + 8 thr
  union {
    float l4_r[F2];
    unsigned l4_m[F2];    // XR: xdiv magic
  };
  // plain (non-REORDER_BN) layer-2/4 branches: per-element BN with offset >> 3 and factor >> 3 in
  // the floor form (requant_host.hpp, choose_floor_form): MFMA C-init = per-filter magic bits + offset,
  // reciprocal r and integer-valued c, so that fma(acc bits, r, c) = FMAGIC + floor(element).
  // XR: C-init = offset >> 3, xdiv magic and shift word; l2_xs / l4_xs are also the shift words of
  // the REORDER_BN builds' layer-2 / layer-4 requant (whose plain fields are unused)
  int l2n_ci[F2];
  union {
    float l2n_r[F2];
    unsigned l2n_m[F2];
  };
  union {
    float l2n_c[F2];
    int l2_xs[F2];
  };
  int l4n_ci[F2];
  union {
    float l4n_r[F2];
    unsigned l4n_m[F2];
  };
  union {
    float l4n_c[F2];
    int l4_xs[F2];
  };
  int l5_w[N_OUT][ND5_MAX];  // [k][v] with row stride T64_ALIGN, zero padded
  int l5_b[N_OUT];
  float l3_r;
  float l5_r;
  float l3_c;             // -(1.5 * 2^23) * l3_r (layer 3's magic C-init requant)
  int pad[1];
};

// Operand fragments and requantisation constants, built by the host from the net.h arrays.
struct DevParams {
  v4i l1_wfrag[2][64];      // layer-1 B operand per N-tile and lane
  int l1_cinit[2][16];      // offset + FMAGIC_I per N-tile column (XR: offset)
  union {
    float l1_r[2][16];      // reciprocal per N-tile column
    unsigned l1_m[2][16];   // XR: xdiv magic
  };
  union {
    float l1_c[2][16];      // -(1.5 * 2^23) * r, exact
    int l1_xs[2][16];       // XR: xdiv shift word
  };
  v4i l2_afrag[F2][3][64];  // layer-2 A operand (banded weights) per filter, K-step and lane
  int l2_thrb[F2];          // pbias(f & 1) + thr, thr = -(net_l2_offset >> 3) clamped: full-tile threshold
  int l2_offm[F2];          // net_l2_offset + 8 thr
  union {
    float l2_r[F2];
    unsigned l2_m[F2];      // XR: xdiv magic (shift word: sp.l2_xs)
  };
  // layer-3 A operands per filter pair (wave) and lane, MFMA 16x16x64 with a block-diagonal K
  // (forward_wg.hpp, layer3): tile 1 = 16 shifts x both filters' 32-slot bands, tile 2 = the same
  // with shift g on row 4g and the other rows zero
  v4i l3_a1[F2 / 2][64];
  v4i l3_a2[F2 / 2][64];
  // layer-2 tail A operand per filter pair (wave) and K-step: MFMA 16x16x64, 16 shifts x 192
  // K-slots = the two filters' 96-slot bands side by side (K block diagonal, see forward_wg.hpp)
  v4i l2t_afrag[F2 / 2][3][64];
  SmallParams sp;
  v4i l1_wfrag_ct[2][64];   // layer-1 B operand for the channel-major staging's K-slot order (stage_block)
};

namespace gen {

constexpr int NW = 8;                  // waves per workgroup
constexpr int NT = 64 * NW;
constexpr int TMAX = 4096;             // samples per trial (16 s at 250 Hz)
constexpr int NMAX = 16;               // classes
constexpr int T64A_MAX = TMAX / 64;
constexpr int L5W = F2 * T64A_MAX;     // bytes of one class's layer-5 weight row

// Per-filter constants read by layers 3 and 4 of every wave: copied into LDS once per workgroup.
struct SmallG {
  v4i l3_a[NW][64];       // layer 3: wave w's A fragment per lane (filters 2w, 2w + 1; layer3)
  v4i l4_b[64];           // layer 4: the block-diagonal B fragment per lane (layer4)
  int l4_thr[F2];         // REORDER_BN: -(offset >> 3); plain: unused
  int l4_off[F2];         // REORDER_BN: offset; plain: offset >> 3
  unsigned l4_m[F2];      // XR: xdiv magic of factor (plain: factor >> 3)
  int l4_xs[F2];
  float l4_r[F2];         // float form: reciprocal (REORDER_BN) / floor-form r (plain)
  float l4_c[F2];         // plain floor form: c
  int l4_ci[F2];          // plain floor form: magic bits + offset >> 3
  int zero16[4];          // 16 zero bytes (layer 3's off-diagonal K halves)
};
static_assert(sizeof(SmallG) % 16 == 0, "SmallG is copied in 16-byte pieces");

// Device parameter image of the general path (built on the host: images.hpp, build_genparams).
struct GenParams {
  int C, T, N, T8;
  int T64, T64A, NB1, MT;       // NB1: layer-1 blocks of 16 samples; MT: full layer-2 tiles of 1024 outputs
  int NTT;                      // layer-2 tail tiles of 256 outputs per filter past the MT full tiles
  int K7;                       // layer-1 blocks of the last wave (its layers 4-5 first), the trial's last ones
  int K7T1;                     // the same for time-major trials at one workgroup per CU
  int pad2;
  int rb, lo, xstride, xr;      // REORDER_BN branches; lower clip bound; time-major trial stride;
                                // exact division (no proven float form for some requant)
  unsigned l3_m;
  int l3_xs;
  unsigned l5_m;
  int l5_xs;
  float l3_r, l3_c;             // float form of layer 3: magic C-init, fma(acc bits, r, c)
  int pad1[2];
  v4i l1_b[64];                 // layer-1 B operand, time-major: lane (filter lane & 15, g) = W1[f] chunk
                                // l1_chunk(g, C) (zero in K groups 1 and 3 when C <= 32)
  v4i l1_bn[64];                // the same in natural order (channel-major, float32): chunk g
  int l1_off[F2];               // XR: offset (the MFMA C-init); float: offset + FMAGIC_I
  unsigned l1_m[F2];            // XR: xdiv magic
  int l1_xs[F2];
  float l1_r[F2], l1_c[F2];     // float form: fma(acc bits, r, c) = RN((dot + off) r)
  int l2_thr[F2];               // REORDER_BN: -(offset >> 3); plain float form: magic bits + offset >> 3
  int l2_off[F2];               // REORDER_BN: offset; plain: offset >> 3
  unsigned l2_m[F2];            // XR: xdiv magic of factor (plain: factor >> 3)
  int l2_xs[F2];
  float l2_r[F2], l2_c[F2];     // float form: reciprocal (REORDER_BN); floor-form r, c (plain)
  int l5_b[NMAX];
  SmallG sg;
  v4i l2_a[F2][3][64];          // layer-2 A operand (banded weights) per filter, K-step and lane
  v4i l2t_a[F2][2][64];         // layer-2 tail A operand (16 shifts x 128 K-slots) per filter, K-step, lane
  int8_t l5_w[NMAX][L5W];       // [n][k T64A + v], zero pads
};

constexpr int LDS_MAX = 160 * 1024;    // LDS per CU
constexpr int LDS_2WG = LDS_MAX / 2;    // two workgroups per CU at most this much each

// bytes of one layer-5 weight row in LDS: F2 T64A rounded up to 256 (64 dwords: the four reads
// per pass of layer5's sixteen lanes per class need no bound check; the pads are zero)
MIB_HD constexpr int w5_row(int T64A) { return (F2 * T64A + 255) / 256 * 256; }

// LDS carve of one workgroup (host and device compute it alike).  Int8 trials (time-major and
// channel-major) are staged whole in LDS ("raw", the trial a grid stride ahead arriving by LDS-DMA
// during layers 2-5) when that fits in LDS_MAX; otherwise, and for float32 trials, layer 1 loads
// its fragments from memory.
struct Carve {
  int y1s, y2s;                 // row strides of y1 (positions t + 32) and y2 (positions u + 8)
  int y2, y3, y4, sg, w5, stg, raw, chunks, bytes;  // raw < 0: not staged; chunks: 1 KB DMA pieces
};
MIB_HD inline Carve carve_of(int C, int T, int N, int T8, int T64A, int NB1, int MT, int NTT, int layout) {
  Carve c;
  // layer 2 reads positions < 1024 MT + 64 (full tiles) and < 1024 MT + 256 NTT + 112 (tail);
  // layer 1 writes positions < 32 + 16 NB1.  Stride = 16 (mod 256): the sixteen filters' layer-1
  // dword stores of a block fall on distinct banks
  const int need = cmax(cmax(32 + 16 * NB1, 1024 * MT + 64), NTT ? 1024 * MT + 256 * NTT + 112 : 0);
  c.y1s = (need + 239) / 256 * 256 + 16;
  c.y2s = align16(T8 + 32);     // 8 pad bytes, T8 outputs, zeros under layer 3's 20-byte windows
  c.y2 = 16 * c.y1s;
  c.y3 = c.y2 + 16 * c.y2s;
  c.y4 = c.y3 + align16(16 * (T8 + 3));       // rows < T8 (layer 3), zeros past them
  c.sg = c.y4 + w5_row(T64A);                 // y4 padded with zeros to whole 256-byte rows
  c.w5 = c.sg + (int)sizeof(SmallG);          // layer-5 weights [N][w5_row], then the N biases
  c.stg = c.w5 + N * w5_row(T64A) + align16(4 * N);  // channel-major transpose staging, 1 KB per wave
  // layout: 0 time-major, 1 channel-major, 2 float32 (gen::Layout); 3: the single-layer kernel
  const int base = c.stg + ((layout == 1 || layout == 2) ? NW * 1024 : 0);
  // the trial's bytes from its dword-aligned base (delta <= 3), in 1 KB pieces, plus the slack the
  // 20-byte fragment windows read past them (time-major: 16 NB1 samples of C bytes; channel-major:
  // row C - 1 read 16 NB1 samples in)
  const int bytes = C * T + 3;
  c.chunks = (bytes + 1023) / 1024;
  const int region = align16(cmax(cmax(1024 * c.chunks, 16 * NB1 * C + 96), C * T + 16 * NB1 + 96));
  c.raw = ((layout == 0 || layout == 1) && base + region <= LDS_MAX) ? base : -1;
  c.bytes = base + (c.raw >= 0 ? region : 0);
  return c;
}

// Time-major K groups: with C <= 32 channels 0..15 go to K group 0 and 16..31 to K group 2, and
// groups 1 and 3 (zero weights) re-read the same 16 bytes.  A ds_read_b32 serves lanes 0-31 and
// 32-63 in separate cycles, so each cycle then reads only 16 distinct windows, whose dwords
// (5.5 j apart at C = 22) fall on distinct banks; groups 0 and 1 together, 16 bytes apart, met
// 2-way conflicts (profiles/r06_lds_conflicts.txt).
MIB_HD inline int l1_chunk(int g, int C) { return C <= 32 ? g >> 1 : g; }

}  // namespace gen

namespace bank {

// The input quantiser's scale of one set and RN(1 / scale), both from the host.
struct Scale {
  float qs, qy;
};

}  // namespace bank
}  // namespace mib
