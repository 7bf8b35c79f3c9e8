// mibminet.hip — libmibminet.so's one translation unit: kernel dispatch, launch and the C ABI
// declared in include/mibminet.h.  The rest of the host side lives in headers by concern:
// * requant_host.hpp: the requantisation proofs (float reciprocals, floor forms, exact division);
// * params_host.hpp: the blob parser (mibminet/params.py, ParamSet.to_blob, holding the reference's
//   net.h arrays, edge-eegnet_wolf/data/gen_net_header.py:91-224), range checks, folding and the
//   requant plan;
// * entry_host.hpp: the entries' argument arithmetic (scale, strides, counts, the windows and epochs
//   checks with the launch geometry they validate);
// * image_layout.hpp: the layouts of both parameter images, the LDS carve and a bank's scale entry,
//   shared with the kernels (HIP-free);
// * images.hpp: the gfx950 operand fragments and both parameter images, laid out from the plan
//   (HIP-free);
// * bank_host.hpp: the HIP-free part of a parameter bank, the build of its images and the decision
//   of a replacement (net_bank_replace) included;
// * stream_host.hpp: the HIP-free part of a stream group: ring size, per-push arithmetic, checks,
//   an each-group's per-session plan, shared with its plan kernel, and a query's validity
//   predicate, shared with its kernel; the group's record (net_streams, one stream::AllocEach for
//   its allocation) and the launching entries' shared prologue (OpenGroup) are here;
// * device_state.hpp: the loaded set, the per-device image cache and the scoped launch entry;
// * test_hooks.hpp: include/mibminet_testing.h.
// There is no CPU compute path: without a usable HIP device every entry point returns an error.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <atomic>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/mibminet.h"
#include "../../include/mibminet_testing.h"
#include "entry_host.hpp"
#include "forward_wg.hpp"
#include "forward_gen.hpp"
#include "forward_win.hpp"
#include "forward_ep.hpp"
#include "forward_bank.hpp"
#include "forward_stream.hpp"
#include "stream_host.hpp"
#include "quantize.hpp"
#include "classify.hpp"
#include "device_state.hpp"

using namespace mib;

// A stream group (net_streams_t, include/mibminet.h): S live sessions of one bank's geometry on one
// device.  mem is the group's one allocation, laid out by at: at.base (stream::alloc_of) is the
// layer-1 rings, then the sessions' origins and sets, of which origin and set are the host's
// mirrors.  pos and emitted advance on the host when a push is enqueued.  An each-group
// (net_streams_create_each) keeps its plan records and a position per session on the device behind
// them (at.plan and at.pos, stream::alloc_each; unused on a uniform group); its pos counts the
// pushes enqueued.  A decimator (net_streams_set_decimator) adds q, K, the raw position and a
// second allocation dmem (stream::alloc_decim: the taps, then every session's last K - 1 raw
// frames); pos stays the decimated position.  An each-group's decimator
// (net_streams_set_decimator_each) lays dmem out by dea (stream::alloc_decim_each, whose base is
// dat): behind the histories come the sessions' raw positions and raw records, and raw_pos stays 0.
// A prefilter (net_streams_set_prefilter) adds M, the sections and a third allocation pmem
// (stream::alloc_prefilter: the states, then the scratch of one push's filtered frames).
// restarted and seeked record that a session was restarted or that the test hook
// mibminet_test_streams_seek placed the group: a seek wants a group that has seen neither, and a
// seeked group counts as pushed to the two setters above.
// A launching entry reaches all of this through OpenGroup (section "live streams").
struct net_streams {
  const net_bank* bank = nullptr;
  int device = 0;
  size_t S = 0, hop = 0, max_push = 0, cap = 0;
  uint64_t pos = 0, emitted = 0;
  void* mem = nullptr;
  stream::AllocEach at{};
  bool each = false;
  std::vector<int64_t> origin;
  std::vector<int32_t> set;
  size_t q = 0, K = 0;  // q == 0: no decimator
  uint64_t raw_pos = 0;
  void* dmem = nullptr;
  stream::AllocDecim dat{};
  stream::AllocDecimEach dea{};
  size_t M = 0;  // M == 0: no prefilter
  stream::Sos sos{};
  void* pmem = nullptr;
  stream::AllocPrefilter pat{};
  bool restarted = false, seeked = false;
};

// test hook (mibminet_test_xdiv_gpu): xdiv against C division in 64 bits over e0 .. e0 + count - 1;
// each thread writes its own mismatch count (plain stores, summed on the host)
__global__ void k_xdiv_check(int d, unsigned m, int xs, long long e0, long long count, unsigned long long* out) {
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, nt = (long long)gridDim.x * blockDim.x;
  unsigned long long bad = 0;
  for (long long i = tid; i < count; i += nt) {
    const int e = (int)(e0 + i);
    const long long want = (long long)e / (long long)d;
    bad += (long long)xdiv(e, m, xs) != (long long)(int)want;
  }
  out[tid] = bad;
}

namespace {

// test hook (mibminet_test_force_general): load every later set on the general path
std::atomic<int> g_force_general{0};
thread_local int t_last_error = NET_OK;

// ---- compiled configurations --------------------------------------------------------------
// Three shapes (images.hpp, compiled_shape), each compiled with and without -DREORDER_BN, with both
// clip modes and with float or exact requant: wg::Cfg<C, T, RB, CB, CT, FQ, XR>.  Every other
// geometry (and N != 4) runs the general kernels (gen::k_forward<Layout>, run-time dimensions).
struct Variant {
  int shape = -1;  // 0: 22 x 1125, 1: 64 x 1000, 2: 64 x 480, 3: general, -1: unsupported
  bool rb = true;  // -DREORDER_BN branches (canonical)
  bool cb = false; // golden-model clip_balanced (clip to [-127, 127])
  bool xr = false; // exact integer division (parameters outside the float requant envelope)
  bool ok() const { return shape >= 0; }
  bool general() const { return shape == 3; }
};

Variant variant_of(const HostParams& hp) {
  Variant v;
  v.shape = hp.general ? 3 : compiled_shape(hp.d);
  v.rb = hp.reorder_bn;
  v.cb = hp.clip_balanced;
  v.xr = hp.xr;
  return v;
}

template <int C, int T, bool CT, bool FQ, bool XR, class F>
int with_variant_x(const Variant& v, F&& f) {
  if (v.rb) return v.cb ? f(wg::Cfg<C, T, true, true, CT, FQ, XR>{}) : f(wg::Cfg<C, T, true, false, CT, FQ, XR>{});
  return v.cb ? f(wg::Cfg<C, T, false, true, CT, FQ, XR>{}) : f(wg::Cfg<C, T, false, false, CT, FQ, XR>{});
}

template <int C, int T, bool CT, bool FQ, class F>
int with_variant(const Variant& v, F&& f) {
  return v.xr ? with_variant_x<C, T, CT, FQ, true>(v, f) : with_variant_x<C, T, CT, FQ, false>(v, f);
}

// Calls f(K{}) with the kernel configuration K of the variant (CT: channel-major input trials;
// FQ: float32 channel-major trials quantised in the kernel).
template <bool CT = false, bool FQ = false, class F>
int dispatch(const Variant& v, F&& f) {
  switch (v.shape) {
    case 0: return with_variant<22, 1125, CT, FQ>(v, f);
    case 1: return with_variant<64, 1000, CT, FQ>(v, f);
    case 2: return with_variant<64, 480, CT, FQ>(v, f);
    default: return NET_ERR_UNSUPPORTED;
  }
}

// The general kernels' instantiation of an image: calls f(rb, xr, cb) with the blob's flags as
// std::bool_constant values: REORDER_BN, exact division, balanced clip.
template <class F>
int with_flags(const gen::GenParams& g, F&& f) {
  auto cb = [&](auto rb, auto xr) {
    return g.lo == -127 ? f(rb, xr, std::true_type{}) : f(rb, xr, std::false_type{});
  };
  auto xr = [&](auto rb) { return g.xr ? cb(rb, std::true_type{}) : cb(rb, std::false_type{}); };
  return g.rb ? xr(std::true_type{}) : xr(std::false_type{});
}

// The same for a run-time layout (0 time-major int8, 1 channel-major int8, 2 channel-major
// float32): calls f with the gen::Layout as a std::integral_constant.  L1: a layer-1 kernel of the
// windows or streams, which also takes gen::F32TM (time-major float32); the batched kernels do not.
template <bool L1 = false, class F>
int with_layout(int layout, F&& f) {
  if constexpr (L1) {
    if (layout == gen::F32TM) return f(std::integral_constant<int, gen::F32TM>{});
  }
  if (layout == 2) return f(std::integral_constant<int, gen::F32>{});
  return layout == 1 ? f(std::integral_constant<int, gen::CT>{}) : f(std::integral_constant<int, gen::TM>{});
}

// the LDS carve of an image's dimensions (layout 3: no trial staging, no transpose staging)
gen::Carve carve_of(const gen::GenParams& g, int layout) {
  return gen::carve_of(g.C, g.T, g.N, g.T8, g.T64A, g.NB1, g.MT, g.NTT, layout);
}
// the LDS bytes of the windows' layers 2-5 (the loaded set's and a bank's), and of the epoch kernels
// (the float32 carve for both layouts)
int windows_lds(const gen::GenParams& g) { return carve_of(g, 3).bytes; }
int epochs_lds(const gen::GenParams& g) { return carve_of(g, gen::F32).bytes; }

// test hook (mibminet_test_grid_cap): at most this many workgroups per persistent grid (0: no cap)
std::atomic<int> g_grid_cap{0};

// persistent grid: one workgroup per item, at most what the occupancy keeps resident
int capped_grid(const DeviceState& ds, size_t items, int blocks_per_cu) {
  const size_t grid = std::min(items, (size_t)ds.cus * (size_t)blocks_per_cu);
  const int cap = g_grid_cap.load();
  return (int)(cap > 0 ? std::min(grid, (size_t)cap) : grid);
}

// Persistent grid: as many resident workgroups as the occupancy allows (two per CU).
template <class K>
int launch_forward_t(DeviceState& ds, const DevParams* p, const int8_t* x, int8_t* y, size_t B,
                     hipStream_t st, int32_t* info, float qs = 0.0f) {
  static std::atomic<int> bpc{0};  // per kernel instantiation (LDS and registers differ)
  int blocks_per_cu = bpc.load();
  if (blocks_per_cu == 0) {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks_per_cu, wg::k_forward<K>, wg::NTHREADS, 0) != hipSuccess ||
        blocks_per_cu < 1)
      blocks_per_cu = 1;
    bpc.store(blocks_per_cu);
  }
  const int grid = capped_grid(ds, B, blocks_per_cu);
  if (info) { info[0] = grid; info[1] = wg::NTHREADS; info[2] = K::LDS; return NET_OK; }
  if (B == 0) return NET_OK;
  hipLaunchKernelGGL(wg::k_forward<K>, dim3(grid), dim3(wg::NTHREADS), 0, st, p, x, y, (int)B, qs, recip_scale(qs));
  return hip_err(hipGetLastError());
}

// General path: dynamic LDS from the run-time dimensions (gen::carve_of); the occupancy of each
// (kernel, LDS size) is queried once, and each kernel may take more than the default 64 KB of
// dynamic LDS.  Keyed by the kernel's address: every instantiation has the same function type.
int gen_blocks_per_cu(const void* k, int lds) {
  static std::mutex mu;
  static std::vector<std::pair<const void*, int>> attr;          // kernels with the LDS attribute set
  static std::vector<std::pair<std::pair<const void*, int>, int>> cache;  // ((kernel, lds), blocks per CU)
  std::lock_guard<std::mutex> lk(mu);
  bool seen = false;
  for (const auto& a : attr) seen = seen || a.first == k;
  if (!seen) {
    (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr.emplace_back(k, 1);
  }
  for (const auto& c : cache)
    if (c.first.first == k && c.first.second == lds) return c.second;
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k, gen::NT, (size_t)lds) != hipSuccess || n < 1) n = 1;
  cache.push_back({{k, lds}, n});
  return n;
}

// The grid of a general-family kernel with `lds` bytes of dynamic LDS over `items` (gen_blocks_per_cu
// also lets the kernel take that much), and its launch.
int gen_grid(const DeviceState& ds, const void* kern, int lds, size_t items) {
  return capped_grid(ds, items, gen_blocks_per_cu(kern, lds));
}
template <class K, class... A>
int launch_items(const DeviceState& ds, K kern, int lds, size_t items, hipStream_t st, A... args) {
  hipLaunchKernelGGL(kern, dim3(gen_grid(ds, (const void*)kern, lds, items)), dim3(gen::NT), (size_t)lds, st, args...);
  return hip_err(hipGetLastError());
}
// The launch of a layer-1 kernel over `wgs` workgroups of win::NT1 threads: 8 workgroups of 4 waves
// fill a CU.
template <class K, class... A>
int launch_l1(const DeviceState& ds, K kern, size_t wgs, hipStream_t st, A... args) {
  hipLaunchKernelGGL(kern, dim3((unsigned)capped_grid(ds, wgs, 8)), dim3(win::NT1), 0, st, args...);
  return hip_err(hipGetLastError());
}

// hg: the host copy of the gen::GenParams p points to (the general path reads its dimensions and
// flags).  Int8 trials that fit in LDS run the staged instantiation (gen::carve_of).
int launch_gen(DeviceState& ds, const gen::GenParams& hg, const void* p, const int8_t* x, int8_t* y, size_t B,
               hipStream_t st, int32_t* info, int layout, float qs) {
  return with_layout(layout, [&](auto lc) {
    constexpr int L = decltype(lc)::value;
    const gen::Carve cv = carve_of(hg, L);
    return with_flags(hg, [&](auto rb, auto xr, auto cb) {
      auto go = [&](auto staged) {
        auto kern = gen::k_forward<L, decltype(staged)::value, decltype(rb)::value, decltype(xr)::value, decltype(cb)::value>;
        if (info) {
          info[0] = gen_grid(ds, (const void*)kern, cv.bytes, B); info[1] = gen::NT; info[2] = cv.bytes;
          return NET_OK;
        }
        if (B == 0) return NET_OK;
        return launch_items(ds, kern, cv.bytes, B, st, (const gen::GenParams*)p, x, y, (int)B, qs, recip_scale(qs));
      };
      if constexpr (L != gen::F32) {
        if (cv.raw >= 0) return go(std::true_type{});
      }
      return go(std::false_type{});
    });
  });
}

// layout: 0 time-major int8, 1 channel-major int8, 2 channel-major float32 (scale qs).  himg: the
// host copy of the image p points to.
int launch_forward(const Variant& v, const void* himg, DeviceState& ds, const void* p, const int8_t* x, int8_t* y,
                   size_t B, hipStream_t st, int32_t* info = nullptr, int layout = 0, float qs = 0.0f) {
  if (v.general()) return launch_gen(ds, *(const gen::GenParams*)himg, p, x, y, B, st, info, layout, qs);
  const DevParams* dp = (const DevParams*)p;
  auto f = [&](auto k) { return launch_forward_t<decltype(k)>(ds, dp, x, y, B, st, info, qs); };
  if (layout == 2) return dispatch<true, true>(v, f);
  return layout == 1 ? dispatch<true, false>(v, f) : dispatch<false, false>(v, f);
}

int launch_layer(const Variant& v, const void* himg, const void* p, const int8_t* in, int8_t* out, int stage,
                 hipStream_t st) {
  if (v.general()) {
    const gen::GenParams& hg = *(const gen::GenParams*)himg;
    const int lds = carve_of(hg, 3).bytes;
    return with_flags(hg, [&](auto rb, auto xr, auto cb) {
      auto kern = gen::k_layer<decltype(rb)::value, decltype(xr)::value, decltype(cb)::value>;
      (void)gen_blocks_per_cu((const void*)kern, lds);  // the LDS attribute
      hipLaunchKernelGGL(kern, dim3(1), dim3(gen::NT), (size_t)lds, st, (const gen::GenParams*)p, in, out, stage);
      return hip_err(hipGetLastError());
    });
  }
  return dispatch(v, [&](auto k) {
    hipLaunchKernelGGL(wg::k_layer<decltype(k)>, dim3(1), dim3(wg::NTHREADS), 0, st, (const DevParams*)p, in, out, stage);
    return hip_err(hipGetLastError());
  });
}

// ---- sliding windows over a recording (forward_win.hpp) --------------------------------------
// Layer 1 over the recording (g.layout) into ws, then the g.W windows' layers 2-5: window w at
// sample w hop, or, with onsets (a device list, net_model_compute_windows_at), at onsets[w], invalid
// ones counted in *n_bad.  g: check_windows' geometry of the Lr samples; hg: the host copy of the
// gen::GenParams p points to.
int launch_windows(DeviceState& ds, const gen::GenParams& hg, const void* p, const WindowsGeom& g, const int8_t* x,
                   size_t Lr, size_t hop, int8_t* y, int8_t* ws, hipStream_t st, float qs,
                   const int64_t* onsets = nullptr, int32_t* n_bad = nullptr) {
  const int lds = windows_lds(hg);
  const gen::GenParams* gp = (const gen::GenParams*)p;
  return with_layout<true>(g.layout, [&](auto lc) {
    return with_flags(hg, [&](auto rb, auto xr, auto cb) {
      constexpr bool RB = decltype(rb)::value, XR = decltype(xr)::value, CB = decltype(cb)::value;
      if (const int rc = launch_l1(ds, win::k_layer1_rec<decltype(lc)::value, XR, CB>, g.wgs, st, gp, x, ws, (int)Lr,
                                   g.rs, qs, recip_scale(qs)))
        return rc;
      // hop > INT32_MAX: a single window (hop <= L - T < 2^27 otherwise), at sample 0 whatever hop is
      const int rc = onsets ? launch_items(ds, win::k_forward_y1_at<RB, XR, CB>, lds, g.W, st, gp, (const int8_t*)ws,
                                           (const long long*)onsets, y, (int*)n_bad, (int)g.W, g.last, g.rs)
                            : launch_items(ds, win::k_forward_y1<RB, XR, CB>, lds, g.W, st, gp, (const int8_t*)ws, y,
                                           (int)g.W, (int)std::min(hop, (size_t)INT32_MAX), g.rs);
      note_launch(ds, p, st);  // the layer-1 kernel reads the copy even if the second launch failed
      return rc;
    });
  });
}

// Both windows entries of the loaded set.  at selects the entry (check_windows, entry_host.hpp); the
// float scale qs.  The list may be null only with W_at == 0, which returns before any launch, so
// launch_windows, reached with W > 0 only, tells the two by the list.  Every argument and parameter
// check comes before the first device call.
int windows_async(const void* x, int arg_layout, bool f32, size_t L, bool at, size_t hop, const int64_t* onsets,
                  size_t W_at, float qs, int8_t* y, int32_t* n_bad, void* ws, size_t ws_bytes, int device,
                  void* stream) {
  const Snapshot s = snapshot();
  if (!s.host) return NET_ERR_NO_PARAMS;
  const Dims& d = s.host->d;
  WindowsGeom g;
  if (const int rc = check_windows(d.C, d.T, x, arg_layout, f32, L, at, hop, onsets, W_at, y, n_bad, ws, ws_bytes, device,
                                   win::NW1, g))
    return rc;
  if (gen::is_float(g.layout))
    if (const int rc = check_scale(qs)) return rc;
  const Image& win = s.img[IMG_WINDOWS];
  if (!win.data) return NET_ERR_UNSUPPORTED;
  if (g.W == 0) return NET_OK;
  DeviceScope sc(device, s, IMG_WINDOWS);
  if (sc.rc) return sc.rc;
  return launch_windows(sc.ds, *(const gen::GenParams*)win.data.get(), sc.image, g, (const int8_t*)x, L, hop, y,
                        (int8_t*)ws, (hipStream_t)stream, qs, onsets, n_bad);
}

// net_windows_multi_count / _onsets: windows_multi (entry_host.hpp) for the loaded network's T; 0
// when no set is loaded.
size_t windows_multi_loaded(const size_t* lengths, size_t R, size_t hop, int64_t* onsets, size_t cap, size_t* first) {
  const Snapshot s = snapshot();
  return s.host ? windows_multi((size_t)s.host->d.T, lengths, R, hop, onsets, cap, first) : 0;
}

// ---- epochs cut out of a wider array (forward_ep.hpp) -----------------------------------------
// f32: the float32 entry (scale qs).  Every argument and parameter check (check_epochs,
// entry_host.hpp) comes before the first device call.
int epochs_async(const void* x, bool f32, size_t n_elems, size_t row_stride, const int32_t* channels,
                 const int64_t* onsets, size_t E, float qs, int8_t* y, int32_t* n_bad, int device, void* stream) {
  const Snapshot s = snapshot();
  if (!s.host) return NET_ERR_NO_PARAMS;
  const Dims& d = s.host->d;
  EpochGeom g;
  if (const int rc = check_epochs(d.C, d.T, x, f32, n_elems, row_stride, channels, onsets, E, y, n_bad, device, g))
    return rc;
  if (f32)
    if (const int rc = check_scale(qs)) return rc;
  const Image& win = s.img[IMG_WINDOWS];
  if (!win.data) return NET_ERR_UNSUPPORTED;
  if (E == 0) return NET_OK;
  DeviceScope sc(device, s, IMG_WINDOWS);
  if (sc.rc) return sc.rc;
  const gen::GenParams& hg = *(const gen::GenParams*)win.data.get();
  const hipStream_t st = (hipStream_t)stream;
  return with_flags(hg, [&](auto rb, auto xr, auto cb) {
    auto go = [&](auto kern) {
      const int rc = launch_items(sc.ds, kern, epochs_lds(hg), E, st, (const gen::GenParams*)sc.image, (const int8_t*)x,
                                  (const long long*)onsets, y, (int*)n_bad, (int)E, g.last, g.span_bytes,
                                  (unsigned long long)row_stride, g.tab, qs, recip_scale(qs));
      if (rc == NET_OK) note_launch(sc.ds, sc.image, st);
      return rc;
    };
    constexpr bool RB = decltype(rb)::value, XR = decltype(xr)::value, CB = decltype(cb)::value;
    return f32 ? go(ep::k_forward_ep<gen::F32, RB, XR, CB>) : go(ep::k_forward_ep<gen::CT, RB, XR, CB>);
  });
}

// A launch on a capturing stream would be replayed with the host state its arguments were computed
// from (a stream group's position, a replacement's bytes); a status that cannot be read counts as
// capturing.
bool capturing(hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
}

// ---- parameter banks (forward_bank.hpp, bank_host.hpp) ---------------------------------------
// (a bank's images are built by bank::build, bank_host.hpp: net_bank_create below only allocates)
void bank_destroy(net_bank* b) {
  if (!b) return;
  for (const auto& c : b->dev) {
    DeviceState& ds = g_devs[c.first];
    std::lock_guard<std::mutex> lk(ds.mu);
    DeviceGuard guard(c.first);
    if (guard.err == hipSuccess) (void)hipDeviceSynchronize();  // no launch still reads the copy
    (void)hipFree(c.second);
  }
  for (const auto& sb : b->staging) {  // the devices are idle: every copy out of a buffer has finished
    (void)hipEventDestroy(sb.second);
    (void)hipHostFree(sb.first);
  }
  delete b;
}

// net_bank_replace (include/mibminet.h).  The decision is bank::replace_set's (bank_host.hpp); here
// are the locks and the copy.  Order of the locks as in a launching call: the device's, then the
// bank's (ensure_bank).  The device's copy of the slot is overwritten by copies enqueued on `stream`
// out of a pinned buffer of the bank's own, never out of the master or the caller's blob: the call
// returns before they run, and both may change right after it.  The master changes last, and only
// its body: the head (geometry and flags) is the record's and is read by other threads unlocked.
int bank_replace(net_bank* b, size_t set, const void* blob, size_t len, float scale, int device, void* stream) {
  if (!b || set >= b->sets.size() || !blob) return NET_ERR_INVALID;
  if (device < 0 || device >= MAX_DEVICES) return NET_ERR_INVALID;
  auto cand = std::make_unique<gen::GenParams>();
  bank::Scale sc{};
  if (const int rc = bank::replace_set(b->rec, blob, len, scale, *cand, sc)) return rc;
  constexpr size_t HEAD = offsetof(gen::GenParams, l3_m), IMG = sizeof(gen::GenParams);
  const hipStream_t st = (hipStream_t)stream;
  std::lock_guard<std::mutex> dl(g_devs[device].mu);
  std::lock_guard<std::mutex> bl(b->mu);
  void* copy = nullptr;
  bool elsewhere = false;
  for (const auto& c : b->dev) {
    if (c.first == device) copy = c.second;
    else elsewhere = true;
  }
  // host data is copied, which a replay would not do again (asked only where something is enqueued:
  // a bank without a copy touches no device here)
  if (copy && capturing(st)) return NET_ERR_UNSUPPORTED;
  if (elsewhere) return NET_ERR_UNSUPPORTED;  // replacing across devices is not part of this entry
  // (agree and the exact-division rule fix every field of the head; held to it all the same)
  if (std::memcmp(cand.get(), &b->sets[set], HEAD) != 0) return NET_ERR_UNSUPPORTED;
  if (copy) {
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return hip_err(guard.err);
    std::pair<void*, hipEvent_t>* buf = nullptr;
    for (auto& sb : b->staging)
      if (hipEventQuery(sb.second) == hipSuccess) {
        buf = &sb;
        break;
      }
    if (!buf) {
      void* p = nullptr;
      hipEvent_t ev = nullptr;
      hipError_t e = hipHostMalloc(&p, IMG + sizeof(bank::Scale), hipHostMallocDefault);
      if (e != hipSuccess) return hip_err(e);
      e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
      if (e != hipSuccess) {
        (void)hipHostFree(p);
        return hip_err(e);
      }
      b->staging.emplace_back(p, ev);
      buf = &b->staging.back();
    }
    std::memcpy(buf->first, cand.get(), IMG);
    std::memcpy((char*)buf->first + IMG, &sc, sizeof(sc));
    char* slot = (char*)copy + set * IMG;
    hipError_t e = hipMemcpyAsync(slot, buf->first, IMG, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && !b->scales.empty())
      e = hipMemcpyAsync((char*)copy + b->sets.size() * IMG + set * sizeof(bank::Scale), (char*)buf->first + IMG,
                         sizeof(bank::Scale), hipMemcpyHostToDevice, st);
    // recorded even after a failed copy: the buffer is not written again while one may still read it
    const hipError_t er = hipEventRecord(buf->second, st);
    if (e != hipSuccess || er != hipSuccess) return hip_err(e != hipSuccess ? e : er);
  }
  std::memcpy((char*)&b->sets[set] + HEAD, (const char*)cand.get() + HEAD, IMG - HEAD);
  if (!b->scales.empty()) b->scales[set] = sc;
  return NET_OK;
}

// The device view of a bank's upload on sc's device: the images, their count and, for float input
// (f32), the scales that follow them.
struct BankView {
  const gen::GenParams* sets;
  int n_sets;
  const bank::Scale* scales;
};
BankView bank_view(const DeviceScope& sc, const net_bank& b, bool f32) {
  const auto* sets = (const gen::GenParams*)sc.image;
  return BankView{sets, (int)b.sets.size(), f32 ? (const bank::Scale*)(sets + b.sets.size()) : nullptr};
}

// epochs_async on a bank: the same checks in the same order, C and T the bank's; then the set
// indices' and, for float input, the bank's scales.  with_feat: the _feat entries, which also write
// the layer-4 activations to feat (its check stands with y's: check_epochs' are all NET_ERR_INVALID).
int bank_epochs_async(const net_bank* b, const void* x, bool f32, size_t n_elems, size_t row_stride,
                      const int32_t* channels, const int64_t* onsets, const int32_t* set_of, size_t E, int8_t* y,
                      int32_t* n_bad, int device, void* stream, bool with_feat = false, int8_t* feat = nullptr) {
  if (!b) return NET_ERR_INVALID;
  const gen::GenParams& hg = b->sets[0];
  EpochGeom g;
  if (const int rc = check_epochs(hg.C, hg.T, x, f32, n_elems, row_stride, channels, onsets, E, y, n_bad, device, g))
    return rc;
  if (with_feat)
    if (const int rc = check_feat(E, feat)) return rc;
  if (((uintptr_t)set_of & 3) != 0 || (E && !set_of && b->sets.size() != 1)) return NET_ERR_INVALID;
  if (f32 && b->scales.empty()) return NET_ERR_INVALID;
  if (E == 0) return NET_OK;
  DeviceScope sc(device, *b);
  if (sc.rc) return sc.rc;
  const BankView v = bank_view(sc, *b, f32);
  return with_flags(hg, [&](auto rb, auto xr, auto cb) {
    // f: nothing, or the feature rows' pointer, which the _feat kernels take after y
    auto go = [&](auto kern, auto... f) {
      return launch_items(sc.ds, kern, epochs_lds(hg), E, (hipStream_t)stream, v.sets, v.n_sets, (const int*)set_of,
                          v.scales, (const int8_t*)x, (const long long*)onsets, y, f..., (int*)n_bad, (int)E, g.last,
                          g.span_bytes, (unsigned long long)row_stride, g.tab);
    };
    constexpr bool RB = decltype(rb)::value, XR = decltype(xr)::value, CB = decltype(cb)::value;
    if (with_feat)
      return f32 ? go(bank::k_forward_ep_bank_feat<gen::F32, RB, XR, CB>, feat)
                 : go(bank::k_forward_ep_bank_feat<gen::CT, RB, XR, CB>, feat);
    return f32 ? go(bank::k_forward_ep_bank<gen::F32, RB, XR, CB>) : go(bank::k_forward_ep_bank<gen::CT, RB, XR, CB>);
  });
}

// The windows of many recordings, each under its own set (forward_bank.hpp): check_windows with the
// bank's C and T, then the block list's and, for float input, the bank's scales.
int bank_windows_async(const net_bank* b, const void* x, int arg_layout, bool f32, size_t L, const int32_t* blk_set,
                       const int64_t* onsets, size_t W, int8_t* y, int32_t* n_bad, void* ws, size_t ws_bytes,
                       int device, void* stream) {
  if (!b) return NET_ERR_INVALID;
  const gen::GenParams& hg = b->sets[0];
  WindowsGeom g;
  if (const int rc = check_windows(hg.C, hg.T, x, arg_layout, f32, L, true, 0, onsets, W, y, n_bad, ws, ws_bytes, device,
                                   win::NW1, g))
    return rc;
  if ((W && !blk_set) || ((uintptr_t)blk_set & 3) != 0) return NET_ERR_INVALID;
  if (f32 && b->scales.empty()) return NET_ERR_INVALID;
  if (W == 0) return NET_OK;
  DeviceScope sc(device, *b);
  if (sc.rc) return sc.rc;
  const BankView v = bank_view(sc, *b, f32);
  const hipStream_t st = (hipStream_t)stream;
  return with_layout<true>(g.layout, [&](auto lc) {
    return with_flags(hg, [&](auto rb, auto xr, auto cb) {
      constexpr bool RB = decltype(rb)::value, XR = decltype(xr)::value, CB = decltype(cb)::value;
      if (const int rc = launch_l1(sc.ds, bank::k_layer1_rec_bank<decltype(lc)::value, XR, CB>, g.wgs, st, v.sets,
                                   v.n_sets, (const int*)blk_set, v.scales, (const int8_t*)x, (int8_t*)ws, (int)L, g.rs))
        return rc;
      return launch_items(sc.ds, bank::k_forward_y1_bank<RB, XR, CB>, windows_lds(hg), W, st, v.sets, v.n_sets,
                          (const int*)blk_set, (const int8_t*)ws, (const long long*)onsets, y, (int*)n_bad, (int)W,
                          g.last, g.rs);
    });
  });
}

// ---- live streams (forward_stream.hpp, stream_host.hpp) --------------------------------------

int streams_create(const net_bank* b, const int32_t* sets, size_t S, size_t hop, size_t max_push, int device,
                   net_streams** out, bool each = false) {
  if (out) *out = nullptr;
  if (const int rc = stream::check_create(b != nullptr, b ? b->sets.size() : 0, sets, S, hop, max_push, device,
                                          out != nullptr))
    return rc;
  auto g = std::make_unique<net_streams>();
  g->bank = b;
  g->device = device;
  g->S = S;
  g->hop = hop;
  g->max_push = max_push;
  g->cap = stream::ring_samples((size_t)b->sets[0].T, max_push);
  g->each = each;
  g->at = stream::alloc_each(S, g->cap);
  if (!each) g->at.bytes = g->at.base.bytes;  // a uniform group ends with the sets: no plan, no positions
  const size_t bytes = g->at.bytes;
  g->origin.assign(S, each ? -1 : 0);
  g->set.assign(S, 0);
  if (sets) g->set.assign(sets, sets + S);
  DeviceScope sc(device, *b);  // uploads the bank if this device has no copy yet
  if (sc.rc) return sc.rc;
  hipError_t e = hipMalloc(&g->mem, bytes);
  if (e != hipSuccess) return hip_err(e);
  e = hipMemset(g->mem, 0, bytes);
  if (e == hipSuccess && sets)
    e = hipMemcpy((char*)g->mem + g->at.base.set, g->set.data(), 4 * S, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipDeviceSynchronize();  // the null stream's memset precedes every stream's push
  if (e != hipSuccess) {
    (void)hipFree(g->mem);
    return hip_err(e);
  }
  *out = g.release();
  return NET_OK;
}

void streams_destroy(net_streams* g) {
  if (!g) return;
  {
    DeviceState& ds = g_devs[g->device];
    std::lock_guard<std::mutex> lk(ds.mu);
    DeviceGuard guard(g->device);
    if (guard.err == hipSuccess) (void)hipDeviceSynchronize();  // no push still uses the rings
    (void)hipFree(g->mem);
    (void)hipFree(g->dmem);
    (void)hipFree(g->pmem);
  }
  delete g;
}

// A group opened for one launching call, after the entry's argument checks: the scope on the group's
// device and bank (which may upload the bank), the stream, the capture refusal where the entry has
// one (REFUSE_CAPTURE: a stream that is capturing gives NET_ERR_UNSUPPORTED), the bank's view (f32:
// with its scales) and the arrays of mem.  plan and pos are an each-group's.  rc != NET_OK: the
// entry returns it, and nothing else here is valid.  Constructed in place: the scope holds the
// device's lock.
enum Capture { ALLOW_CAPTURE, REFUSE_CAPTURE };
struct OpenGroup {
  DeviceScope sc;
  hipStream_t st;
  int rc;
  BankView v{};
  int8_t* ring;
  long long *origin, *pos;
  int* set_of;
  stream::EachRec* plan;
  OpenGroup(const net_streams& g, void* stream, Capture capture, bool f32 = false)
      : sc(g.device, *g.bank), st((hipStream_t)stream), rc(sc.rc), ring((int8_t*)g.mem),
        origin((long long*)(ring + g.at.base.origin)), pos((long long*)(ring + g.at.pos)),
        set_of((int*)(ring + g.at.base.set)), plan((stream::EachRec*)(ring + g.at.plan)) {
    if (rc == NET_OK && capture == REFUSE_CAPTURE && capturing(st)) rc = NET_ERR_UNSUPPORTED;
    if (rc == NET_OK) v = bank_view(sc, *g.bank, f32);
  }
  OpenGroup(const OpenGroup&) = delete;
};

// workgroups of a layer-1 launch over l1_items 16-sample blocks
size_t l1_wgs(size_t l1_items) { return (l1_items + win::NW1 - 1) / win::NW1; }

// The windows that end in a push, out of the rings: the launch that ends net_streams_push* and
// net_streams_push_raw_f32_tm.
template <bool RB, bool XR, bool CB>
int launch_ring_windows(const OpenGroup& o, const net_streams& g, const stream::Push& p, int8_t* y, int32_t* n_bad) {
  return launch_items(o.sc.ds, stream::k_forward_ring<RB, XR, CB>, windows_lds(g.bank->sets[0]), p.items, o.st, o.v.sets,
                      o.v.n_sets, o.ring, o.origin, o.set_of, y, (int*)n_bad, (int)p.items, (int)p.k, p.first, p.hop,
                      p.first_mod, (int)g.cap);
}

// Both push entries: every check (stream::check_push, then the stream's capture status) comes before
// the first launch and before pos moves.
int streams_push(net_streams* g, const void* x, int arg_layout, bool f32, size_t n, int8_t* y, int32_t* n_bad,
                 void* stream) {
  if (!g || g->each || g->q) return NET_ERR_INVALID;
  const net_bank& b = *g->bank;
  const gen::GenParams& hg = b.sets[0];
  stream::Push p;
  if (const int rc = stream::check_push((size_t)hg.T, g->S, g->hop, g->max_push, g->cap, g->pos, x, arg_layout, f32,
                                        !b.scales.empty(), n, y, n_bad, p))
    return rc;
  if (n == 0) return NET_OK;
  const OpenGroup o(*g, stream, REFUSE_CAPTURE, f32);
  if (o.rc) return o.rc;
  const int rc = with_layout<true>(f32 ? gen::float_layout(arg_layout) : arg_layout, [&](auto lc) {
    return with_flags(hg, [&](auto rb, auto xr, auto cb) {
      constexpr bool RB = decltype(rb)::value, XR = decltype(xr)::value, CB = decltype(cb)::value;
      if (const int rc = launch_l1(o.sc.ds, stream::k_layer1_ring<decltype(lc)::value, XR, CB>, l1_wgs(p.l1_items), o.st,
                                   o.v.sets, o.v.n_sets, o.set_of, o.v.scales, (const int8_t*)x, o.ring, (int)p.l1_items,
                                   (int)p.blocks, (int)n, p.p0, (int)g->cap))
        return rc;
      if (p.k == 0) return (int)NET_OK;
      return launch_ring_windows<RB, XR, CB>(o, *g, p, y, n_bad);
    });
  });
  if (rc) return rc;
  g->pos += n;
  g->emitted += p.k;
  return NET_OK;
}

int streams_restart(net_streams* g, size_t i, int32_t set, void* stream) {
  if (!g || i >= g->S || set < 0 || (size_t)set >= g->bank->sets.size()) return NET_ERR_INVALID;
  const OpenGroup o(*g, stream, REFUSE_CAPTURE);  // a replay would move the origin to a stale position
  if (o.rc) return o.rc;
  if (g->q && g->K > 1)  // a decimator: the session's raw frames before the restart count as zeros
    if (const int rc = hip_err(hipMemsetAsync((char*)g->dmem + g->dat.hist + i * g->dat.per, 0, g->dat.per, o.st)))
      return rc;
  if (g->M)  // a prefilter: zero state is the steady state of zero input
    if (const int rc = hip_err(hipMemsetAsync((char*)g->pmem + g->pat.state + i * g->pat.per_state, 0, g->pat.per_state, o.st)))
      return rc;
  if (g->q && g->each)  // an each-group's decimator: the session's raw position goes back to 0 too
    if (const int rc = hip_err(hipMemsetAsync((char*)g->dmem + g->dea.raw_pos + 8 * i, 0, 8, o.st))) return rc;
  // an each-group: the session's position goes back to 0 (its origin stays -1: there is none)
  hipLaunchKernelGGL(stream::k_stream_restart, dim3(1), dim3(1), 0, o.st, g->each ? o.pos : o.origin, o.set_of, (int)i,
                     g->each ? 0ll : (long long)g->pos, (int)set);
  if (const int rc = hip_err(hipGetLastError())) return rc;
  if (!g->each) g->origin[i] = (int64_t)g->pos;
  g->set[i] = set;
  g->restarted = true;
  return NET_OK;
}

// net_streams_set_decimator: every check, the capturing stream's last, comes before the allocation;
// the group changes only once the taps are on the device and the histories zero.  The stream is
// waited for, so the caller's taps are free on return.
// each: net_streams_set_decimator_each, the same on an each-group (whose pos counts its pushes); its
// allocation holds the raw positions and raw records too, zeroed with the rest.
int streams_set_decimator(net_streams* g, size_t q, const float* taps, size_t K, void* stream, bool each = false) {
  if (each && (!g || !g->each)) return NET_ERR_INVALID;
  if (const int rc = stream::check_set_decimator(g != nullptr, g && g->each && !each, g && !g->bank->scales.empty(),
                                                 g && g->q != 0, g && (g->pos != 0 || g->seeked), q, taps, K))
    return rc;
  const OpenGroup o(*g, stream, REFUSE_CAPTURE);
  if (o.rc) return o.rc;
  const stream::AllocDecimEach ea = stream::alloc_decim_each(g->S, (size_t)g->bank->sets[0].C, K);
  stream::AllocDecim a = ea.base;
  if (each) a.bytes = ea.bytes;
  void* mem = nullptr;
  hipError_t e = hipMalloc(&mem, a.bytes);
  if (e != hipSuccess) return hip_err(e);
  e = hipMemsetAsync(mem, 0, a.bytes, o.st);
  if (e == hipSuccess) e = hipMemcpyAsync((char*)mem + a.taps, taps, 4 * K, hipMemcpyHostToDevice, o.st);
  if (e == hipSuccess) e = hipStreamSynchronize(o.st);
  if (e != hipSuccess) {
    (void)hipFree(mem);
    return hip_err(e);
  }
  g->dmem = mem;
  g->dat = ea.base;
  g->dea = ea;
  g->q = q;
  g->K = K;
  return NET_OK;
}

// net_streams_set_prefilter, on either kind of group: every check, the capturing stream's last, comes
// before the allocation; the group changes only once the states are zero.  The sections travel by
// value in the prefilter kernel's arguments, so the device holds no copy of them.  The stream is
// waited for, as streams_set_decimator waits.
int streams_set_prefilter(net_streams* g, const float* sos, size_t M, void* stream) {
  if (const int rc = stream::check_set_prefilter(g != nullptr, g && g->q != 0, g && g->M != 0,
                                                 g && (g->pos != 0 || g->raw_pos != 0 || g->seeked), sos, M))
    return rc;
  const OpenGroup o(*g, stream, REFUSE_CAPTURE);
  if (o.rc) return o.rc;
  const stream::AllocPrefilter a = stream::alloc_prefilter(g->S, (size_t)g->bank->sets[0].C, M, g->q, g->max_push);
  void* mem = nullptr;
  hipError_t e = hipMalloc(&mem, a.bytes);
  if (e != hipSuccess) return hip_err(e);
  e = hipMemsetAsync(mem, 0, a.scratch, o.st);  // the states; the scratch is written before it is read
  if (e == hipSuccess) e = hipStreamSynchronize(o.st);
  if (e != hipSuccess) {
    (void)hipFree(mem);
    return hip_err(e);
  }
  g->pmem = mem;
  g->pat = a;
  std::memcpy(g->sos.c, sos, 5 * sizeof(float) * M);
  g->M = M;
  return NET_OK;
}

// calls f with M as a std::integral_constant (M in 1 .. stream::MAX_SECTIONS)
template <class F>
int with_sections(size_t M, F&& f) {
  switch (M) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    case 8: return f(std::integral_constant<int, 8>{});
  }
  return NET_ERR_INVALID;
}

// The prefilter's launch (stream::k_prefilter) over S sessions of R electrodes and n_view frames each
// (EACH: at most, the trip counts from raw): one lane per (session, electrode) in waves of their own,
// at most 32 per CU, grid-stride beyond that.
template <bool EACH>
int launch_prefilter(const DeviceState& ds, hipStream_t st, const float* x, float* y, float* state,
                     const stream::RawRec* raw, size_t S, size_t R, size_t n_view, size_t M, const stream::Sos& sos) {
  const size_t lanes = S * R;  // S < 2^31, R <= 2^6
  return with_sections(M, [&](auto m) {
    hipLaunchKernelGGL((stream::k_prefilter<EACH, decltype(m)::value>), dim3((unsigned)capped_grid(ds, (lanes + 63) / 64, 32)),
                       dim3(64), 0, st, x, y, state, raw, (unsigned long long)lanes, (unsigned)R, (unsigned)n_view, sos);
    return hip_err(hipGetLastError());
  });
}

// net_streams_push_raw_f32_tm: every check (stream::check_push_raw, then the stream's capture status)
// comes before the first launch and before a position moves.  Layer 1 reads the histories, the
// history kernel behind it rewrites them, the windows' kernel is a plain push's.
int streams_push_raw(net_streams* g, const float* x, size_t n_raw, int8_t* y, int32_t* n_bad, void* stream) {
  if (!g || g->each || !g->q) return NET_ERR_INVALID;
  const net_bank& b = *g->bank;
  const gen::GenParams& hg = b.sets[0];
  stream::PushRaw r;
  if (const int rc = stream::check_push_raw((size_t)hg.T, g->S, (size_t)hg.C, g->hop, g->max_push, g->cap, g->q, g->K,
                                            g->raw_pos, x, !b.scales.empty(), n_raw, y, n_bad, r))
    return rc;
  if (n_raw == 0) return NET_OK;
  const OpenGroup o(*g, stream, REFUSE_CAPTURE, true);
  if (o.rc) return o.rc;
  char* dmem = (char*)g->dmem;
  const stream::Push& p = r.push;
  if (g->M) {  // a prefilter: the kernels below take the filtered frames where they took x
    float* const f = (float*)((char*)g->pmem + g->pat.scratch);
    if (const int rc = launch_prefilter<false>(o.sc.ds, o.st, x, f, (float*)((char*)g->pmem + g->pat.state), nullptr, g->S,
                                               (size_t)hg.C, n_raw, g->M, g->sos))
      return rc;
    x = f;
  }
  const int rc = with_flags(hg, [&](auto rb, auto xr, auto cb) {
    constexpr bool RB = decltype(rb)::value, XR = decltype(xr)::value, CB = decltype(cb)::value;
    if (r.m) {
      const stream::Decim dc{(const float*)(dmem + g->dat.taps), (const int8_t*)(dmem + g->dat.hist), (int)g->K, (int)g->q,
                             r.off, r.slot0, (unsigned)g->dat.per};
      if (const int rc = launch_l1(o.sc.ds, stream::k_layer1_ring_decim<XR, CB>, l1_wgs(p.l1_items), o.st, o.v.sets,
                                   o.v.n_sets, o.set_of, o.v.scales, (const int8_t*)x, o.ring, (int)p.l1_items, (int)p.blocks,
                                   (int)n_raw, (int)r.m, p.p0, (int)g->cap, dc))
        return rc;
    }
    if (r.keep) {
      const size_t blocks = std::min((r.hist_items + 255) / 256, (size_t)o.sc.ds.cus * 8);
      hipLaunchKernelGGL(stream::k_history_update, dim3((unsigned)blocks), dim3(256), 0, o.st, x,
                         (float*)(dmem + g->dat.hist), (unsigned long long)r.hist_items, (unsigned)hg.C, (unsigned)n_raw,
                         (unsigned)r.keep, (unsigned)g->K, (unsigned)r.slot0);
      if (const int rc = hip_err(hipGetLastError())) return rc;
    }
    if (r.m == 0 || p.k == 0) return (int)NET_OK;
    return launch_ring_windows<RB, XR, CB>(o, *g, p, y, n_bad);
  });
  if (rc) return rc;
  g->raw_pos += n_raw;
  g->pos += r.m;
  g->emitted += r.m ? p.k : 0;
  return NET_OK;
}

// Both push entries of an each-group: every check comes before the first launch.  A launch that
// fails after the plan's leaves the positions advanced (include/mibminet.h says so); nothing here
// depends on what earlier pushes did (the positions are on the device), so the three launches are
// the same on every call with the same arguments and may be captured; pos counts the enqueues.
int streams_push_each(net_streams* g, const void* x, int arg_layout, bool f32, const int32_t* cnt_in, size_t n_max,
                      int8_t* y, int32_t* cnt_out, int64_t* win0, int32_t* n_bad, void* stream) {
  if (!g || !g->each || g->q) return NET_ERR_INVALID;  // (with a decimator: the raw push below)
  const net_bank& b = *g->bank;
  const gen::GenParams& hg = b.sets[0];
  stream::PushEach p;
  if (const int rc = stream::check_push_each(g->S, g->hop, g->max_push, x, arg_layout, f32, !b.scales.empty(), cnt_in,
                                             n_max, y, cnt_out, win0, n_bad, p))
    return rc;
  const OpenGroup o(*g, stream, ALLOW_CAPTURE, f32);
  if (o.rc) return o.rc;
  hipLaunchKernelGGL(stream::k_stream_plan, dim3((unsigned)((g->S + 255) / 256)), dim3(256), 0, o.st, (const int*)cnt_in,
                     o.pos, o.plan, (int*)cnt_out, (long long*)win0, (int*)n_bad, (int)g->S, hg.T,
                     (unsigned long long)g->hop, (int)g->cap, (int)n_max);
  if (const int rc = hip_err(hipGetLastError())) return rc;
  const int rc = with_layout<true>(f32 ? gen::float_layout(arg_layout) : arg_layout, [&](auto lc) {
    return with_flags(hg, [&](auto rb, auto xr, auto cb) {
      constexpr bool RB = decltype(rb)::value, XR = decltype(xr)::value, CB = decltype(cb)::value;
      if (const int rc = launch_l1(o.sc.ds, stream::k_layer1_ring_each<decltype(lc)::value, XR, CB>, l1_wgs(p.l1_items),
                                   o.st, o.v.sets, o.v.n_sets, o.set_of, o.v.scales, (const int8_t*)x, o.ring, o.plan,
                                   (int)p.l1_items, (int)p.blocks, (int)n_max, (int)g->cap))
        return rc;
      return launch_items(o.sc.ds, stream::k_forward_ring_each<RB, XR, CB>, windows_lds(hg), p.items, o.st, o.v.sets,
                          o.v.n_sets, o.ring, o.plan, o.set_of, y, (int)p.items, (int)p.kmax, p.hop, (int)g->cap);
    });
  });
  if (rc) return rc;
  g->pos++;
  return NET_OK;
}

// net_streams_push_each_raw_f32_tm: every check comes before the first launch.  Four launches that
// read nothing from the host: the plan (k_stream_plan_raw: both records, both positions), layer 1
// with the FIR from the session's slot and history, the history update (K > 1; also when no session
// completes a sample), the windows (k_forward_ring_each as it is).  Capturable as
// streams_push_each is, on the caller's one stream.
int streams_push_each_raw(net_streams* g, const float* x, const int32_t* cnt_in, size_t n_raw_max, int8_t* y,
                          int32_t* cnt_out, int64_t* win0, int32_t* n_bad, void* stream) {
  if (!g || !g->each || !g->q) return NET_ERR_INVALID;
  const net_bank& b = *g->bank;
  const gen::GenParams& hg = b.sets[0];
  stream::PushEachRaw r;
  if (const int rc = stream::check_push_each_raw(g->S, (size_t)hg.C, g->hop, g->max_push, g->q, g->K, x, !b.scales.empty(),
                                                 cnt_in, n_raw_max, y, cnt_out, win0, n_bad, r))
    return rc;
  const OpenGroup o(*g, stream, ALLOW_CAPTURE, true);
  if (o.rc) return o.rc;
  char* dmem = (char*)g->dmem;
  auto* raw = (stream::RawRec*)(dmem + g->dea.rec);
  const stream::PushEach& p = r.each;
  hipLaunchKernelGGL(stream::k_stream_plan_raw, dim3((unsigned)((g->S + 255) / 256)), dim3(256), 0, o.st,
                     (const int*)cnt_in, (long long*)(dmem + g->dea.raw_pos), o.pos, o.plan, raw, (int*)cnt_out,
                     (long long*)win0, (int*)n_bad, (int)g->S, hg.T, (unsigned long long)g->hop, (int)g->cap, (int)g->q,
                     (int)g->K, (int)n_raw_max);
  if (const int rc = hip_err(hipGetLastError())) return rc;
  if (g->M) {  // a prefilter, its trip counts from the raw records: the kernels below take the filtered slots
    float* const f = (float*)((char*)g->pmem + g->pat.scratch);
    if (const int rc = launch_prefilter<true>(o.sc.ds, o.st, x, f, (float*)((char*)g->pmem + g->pat.state), raw, g->S,
                                              (size_t)hg.C, n_raw_max, g->M, g->sos))
      return rc;
    x = f;
  }
  const int rc = with_flags(hg, [&](auto rb, auto xr, auto cb) {
    constexpr bool RB = decltype(rb)::value, XR = decltype(xr)::value, CB = decltype(cb)::value;
    const stream::Decim dc{(const float*)(dmem + g->dat.taps), (const int8_t*)(dmem + g->dat.hist), (int)g->K, (int)g->q, 0, 0,
                           (unsigned)g->dat.per};
    if (const int rc = launch_l1(o.sc.ds, stream::k_layer1_ring_each_decim<XR, CB>, l1_wgs(p.l1_items), o.st, o.v.sets,
                                 o.v.n_sets, o.set_of, o.v.scales, (const int8_t*)x, o.ring, o.plan,
                                 (const stream::RawRec*)raw, (int)p.l1_items, (int)p.blocks, (int)n_raw_max, (int)g->cap, dc))
      return rc;
    if (r.keep_max) {
      const size_t blocks = std::min((r.hist_items + 255) / 256, (size_t)o.sc.ds.cus * 8);
      hipLaunchKernelGGL(stream::k_history_update_each, dim3((unsigned)blocks), dim3(256), 0, o.st, x,
                         (float*)(dmem + g->dat.hist), (const stream::RawRec*)raw, (unsigned long long)r.hist_items,
                         (unsigned)hg.C, (unsigned)n_raw_max, (unsigned)r.keep_max, (unsigned)g->K);
      if (const int rc = hip_err(hipGetLastError())) return rc;
    }
    return launch_items(o.sc.ds, stream::k_forward_ring_each<RB, XR, CB>, windows_lds(hg), p.items, o.st, o.v.sets,
                        o.v.n_sets, o.ring, o.plan, o.set_of, y, (int)p.items, (int)p.kmax, p.hop, (int)g->cap);
  });
  if (rc) return rc;
  g->pos++;
  return NET_OK;
}

// net_streams_windows_at[_feat]: every check comes before the one launch.  A uniform group's arguments
// come from the host's position, so its launch is not capturable; an each-group's reads nothing from
// the host.  Nothing of the group changes.
int streams_windows_at(net_streams* g, const int32_t* session, const int64_t* onsets, size_t W, int8_t* y,
                       int32_t* n_bad, void* stream, bool with_feat = false, int8_t* feat = nullptr) {
  if (const int rc = stream::check_windows_at(g != nullptr, W, session, onsets, y, n_bad)) return rc;
  if (W == 0) return NET_OK;
  if (with_feat)
    if (const int rc = check_feat(W, feat)) return rc;
  const gen::GenParams& hg = g->bank->sets[0];
  const OpenGroup o(*g, stream, g->each ? ALLOW_CAPTURE : REFUSE_CAPTURE);  // layer 1 ran at the push: no scales
  if (o.rc) return o.rc;
  const long long* lim = g->each ? o.pos : o.origin;
  const long long pos = g->each ? 0ll : (long long)g->pos;
  const int pos_mod = g->each ? 0 : (int)(g->pos % g->cap);
  return with_flags(hg, [&](auto rb, auto xr, auto cb) {
    constexpr bool RB = decltype(rb)::value, XR = decltype(xr)::value, CB = decltype(cb)::value;
    // f: nothing, or the feature rows' pointer, which the _feat kernel takes after y
    auto go = [&](auto kern, auto... f) {
      return launch_items(o.sc.ds, kern, windows_lds(hg), W, o.st, o.v.sets, o.v.n_sets, o.ring, (const int*)session,
                          (const long long*)onsets, lim, o.set_of, y, f..., (int*)n_bad, (int)W, (int)g->S, pos, pos_mod,
                          (int)g->cap);
    };
    if (with_feat)
      return g->each ? go(stream::k_forward_ring_at_feat<RB, XR, CB, true>, feat)
                     : go(stream::k_forward_ring_at_feat<RB, XR, CB, false>, feat);
    return g->each ? go(stream::k_forward_ring_at<RB, XR, CB, true>) : go(stream::k_forward_ring_at<RB, XR, CB, false>);
  });
}

int streams_at_span(const net_streams* g, int64_t* lo, int64_t* hi) {
  if (!g || g->each || !lo || !hi) return NET_ERR_INVALID;
  stream::at_span((size_t)g->bank->sets[0].T, g->cap, g->pos, lo, hi);
  return NET_OK;
}

int streams_positions(net_streams* g, int64_t* pos_out, void* stream) {
  if (!g || !g->each || !pos_out || ((uintptr_t)pos_out & 7) != 0) return NET_ERR_INVALID;
  const OpenGroup o(*g, stream, ALLOW_CAPTURE);
  if (o.rc) return o.rc;
  return hip_err(hipMemcpyAsync(pos_out, o.pos, 8 * g->S, hipMemcpyDeviceToDevice, o.st));
}

int streams_raw_positions(net_streams* g, int64_t* raw_pos_out, void* stream) {
  if (!g || !g->each || !raw_pos_out || ((uintptr_t)raw_pos_out & 7) != 0 || !g->q) return NET_ERR_INVALID;
  const OpenGroup o(*g, stream, ALLOW_CAPTURE);
  if (o.rc) return o.rc;
  return hip_err(hipMemcpyAsync(raw_pos_out, (char*)g->dmem + g->dea.raw_pos, 8 * g->S, hipMemcpyDeviceToDevice, o.st));
}

// Runs one reference-layout single-trial stage on the single-trial device.
// stage 0 = whole model (input [T][C_ALIGN]); 1..5 = net_layerN; 6 = flip.
int run_single(int stage, const int8_t* in, int8_t* out) {
  if (!in || !out) return NET_ERR_INVALID;
  Snapshot s = snapshot();
  if (!s.host) return NET_ERR_NO_PARAMS;
  const Dims& d = s.host->d;
  const Variant v = variant_of(*s.host);
  if (!v.ok()) return NET_ERR_UNSUPPORTED;
  DeviceScope sc(g_single_device.load(), s, IMG_KERNELS, false);  // net_set_device checked the device
  if (sc.rc) return sc.rc;
  DeviceState& ds = sc.ds;
  const size_t xs = trial_stride(d);
  int rc = ensure_scratch(ds, xs > (size_t)d.F1 * d.T_ALIGN() ? xs + 64 : (size_t)d.F1 * d.T_ALIGN() + 64);
  if (rc) return rc;
  size_t in_bytes, out_bytes;
  switch (stage) {
    case 0:
    case 1: {  // reference input [T][C_ALIGN] -> packed [T][C], straight into the pinned staging
      for (int t = 0; t < d.T; t++) std::memcpy(ds.h_in + (size_t)t * d.C, in + (size_t)t * d.C_ALIGN(), d.C);
      std::memset(ds.h_in + (size_t)d.T * d.C, 0, xs - (size_t)d.T * d.C);
      in_bytes = xs;
      out_bytes = stage == 0 ? (size_t)d.N : (size_t)d.F1 * d.T_ALIGN();
      break;
    }
    case 2: in_bytes = (size_t)d.F1 * d.T_ALIGN(); out_bytes = (size_t)d.F2 * d.T8_ALIGN(); break;
    case 3: in_bytes = out_bytes = (size_t)d.F2 * d.T8_ALIGN(); break;
    case 4: in_bytes = (size_t)d.T8() * d.F2; out_bytes = (size_t)d.F2 * d.T64_ALIGN(); break;
    case 5: in_bytes = (size_t)d.F2 * d.T64_ALIGN(); out_bytes = (size_t)d.N; break;
    case 6: in_bytes = out_bytes = (size_t)d.F2 * d.T8_ALIGN(); break;
    default: return NET_ERR_INVALID;
  }
  if (stage > 1) std::memcpy(ds.h_in, in, in_bytes);
  hipError_t e;
#ifdef MIB_SINGLE_COPIES
  e = hipMemcpyAsync(ds.d_in, ds.h_in, in_bytes, hipMemcpyHostToDevice, ds.st);
  if (e != hipSuccess) return hip_err(e);
  int8_t* kin = ds.d_in;
  int8_t* kout = ds.d_out;
#else
  // zero copy: the kernel reads the trial from the pinned staging and writes its result there
  // (one launch per call instead of copy + launch + copy)
  int8_t* kin = nullptr;
  int8_t* kout = nullptr;
  e = hipHostGetDevicePointer((void**)&kin, ds.h_in, 0);
  if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&kout, ds.h_out, 0);
  if (e != hipSuccess) return hip_err(e);
#endif
  const void* himg = s.img[IMG_KERNELS].data.get();
  if (stage == 0)
    rc = launch_forward(v, himg, ds, sc.image, kin, kout, 1, ds.st);
  else
    rc = launch_layer(v, himg, sc.image, kin, kout, stage, ds.st);
  if (rc) {
    (void)hipStreamSynchronize(ds.st);  // a copy may still read the staging
    return rc;
  }
#ifdef MIB_SINGLE_COPIES
  e = hipMemcpyAsync(ds.h_out, ds.d_out, out_bytes, hipMemcpyDeviceToHost, ds.st);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(ds.st);
    return hip_err(e);
  }
#endif
  e = hipStreamSynchronize(ds.st);
  if (e != hipSuccess) return hip_err(e);
  std::memcpy(out, ds.h_out, out_bytes);
  return NET_OK;
}

template <class F>
int quantize_input(const F* x, int8_t* y, size_t B, int C, int T, F scale, int device, void* stream) {
  if ((!x || !y) && B) return NET_ERR_INVALID;
  if (C < 1 || C > quant::CMAX || T < 1 || device < 0 || device >= MAX_DEVICES) return NET_ERR_INVALID;
  // trial indices are int in the kernel: b + gridDim.y (<= B + YMAX) must not wrap
  if (B > (size_t)INT32_MAX - quant::YMAX || !(scale > 0)) return NET_ERR_INVALID;
  // one trial's input bytes form one buffer view (32-bit range); the tiles leave as 16-byte stores
  if ((size_t)C * T * sizeof(F) >= (size_t)1 << 31 || ((uintptr_t)y & 15)) return NET_ERR_INVALID;
  if (B == 0) return NET_OK;
  if (const int rc = check_device(device)) return rc;
  const int stride = (int)(((size_t)C * T + 15) / 16 * 16);
  DeviceGuard guard(device);
  if (guard.err != hipSuccess) return hip_err(guard.err);
  // each workgroup walks a few trials, loading one trial ahead
  constexpr size_t per = quant::qtrials<F>();
  const size_t rows = std::min((B + per - 1) / per, (size_t)quant::YMAX);
  dim3 grid((T + quant::TT - 1) / quant::TT, (unsigned)rows);
  hipLaunchKernelGGL(quant::k_quantize<F>, grid, dim3(quant::QTHREADS), 0, (hipStream_t)stream, x, y, C, T, stride, scale,
                     (int)B);
  return hip_err(hipGetLastError());
}

int argmax_batch(const int8_t* logits, int32_t* out, size_t B, int N, int device, void* stream) {
  if ((!logits || !out) && B) return NET_ERR_INVALID;
  // trial indices are int in the kernels: 4 q + 3 and blockIdx.x * CTHREADS + threadIdx.x reach
  // at most B + 4 CTHREADS, which must not wrap
  if (N < 1 || N > cls::NMAX || device < 0 || device >= MAX_DEVICES || B > (size_t)INT32_MAX - 4 * cls::CTHREADS)
    return NET_ERR_INVALID;
  if (B == 0) return NET_OK;
  if (const int rc = check_device(device)) return rc;
  DeviceGuard guard(device);
  if (guard.err != hipSuccess) return hip_err(guard.err);
  if (N == 4 && ((uintptr_t)logits & 15) == 0 && ((uintptr_t)out & 15) == 0) {
    const unsigned grid = (unsigned)((B + 4 * cls::CTHREADS - 1) / (4 * cls::CTHREADS));
    hipLaunchKernelGGL(cls::k_argmax4, dim3(grid), dim3(cls::CTHREADS), 0, (hipStream_t)stream,
                       (const unsigned*)logits, out, (int)B);
    return hip_err(hipGetLastError());
  }
  const unsigned grid = (unsigned)((B + cls::CTHREADS - 1) / cls::CTHREADS);
  hipLaunchKernelGGL(cls::k_argmax, dim3(grid), dim3(cls::CTHREADS), 0, (hipStream_t)stream, logits, out, (int)B, N);
  return hip_err(hipGetLastError());
}

// Builds the images of a parsed set (images.hpp, build_set) and makes it the loaded set.
int install(std::shared_ptr<HostParams> hp) {
  Image img, win;
  if (const int rc = build_set(*hp, g_force_general.load() != 0, &img, &win)) return rc;
  std::lock_guard<std::mutex> lk(g_mu);
  g_set = Snapshot{hp, {img, win}, g_set.gen + 1};
  return NET_OK;
}

// layout: 0 time-major int8 (16-byte aligned, stride net_trial_stride()), 1 channel-major int8
// trials [B][C][T] (any alignment, trial stride C T bytes), 2 channel-major float32 (scale qs)
int batch_async_s(const Snapshot& s, const int8_t* x, int8_t* y, size_t B, int device, void* stream, int layout,
                  float qs = 0.0f) {
  if ((!x || !y) && B) return NET_ERR_INVALID;
  const uintptr_t xa = layout == 0 ? 15 : layout == 2 ? 3 : 0;
  if (((uintptr_t)x & xa) != 0 || ((uintptr_t)y & 3) != 0) return NET_ERR_INVALID;
  if (layout == 2)
    if (const int rc = check_scale(qs)) return rc;
  // trial indices are int in the kernel: b + gridDim.x (grid <= 2 per CU) must not wrap
  if (device < 0 || device >= MAX_DEVICES || B > (size_t)INT32_MAX - 65536) return NET_ERR_INVALID;
  if (!s.host) return NET_ERR_NO_PARAMS;
  const Variant v = variant_of(*s.host);
  if (!v.ok()) return NET_ERR_UNSUPPORTED;
  DeviceScope sc(device, s, IMG_KERNELS);
  if (sc.rc) return sc.rc;
  const int rc = launch_forward(v, s.img[IMG_KERNELS].data.get(), sc.ds, sc.image, x, y, B, (hipStream_t)stream, nullptr,
                                layout, qs);
  if (rc == NET_OK && B) note_launch(sc.ds, sc.image, (hipStream_t)stream);
  return rc;
}

int batch_async(const int8_t* x, int8_t* y, size_t B, int device, void* stream, int layout, float qs = 0.0f) {
  return batch_async_s(snapshot(), x, y, B, device, stream, layout, qs);
}

// the blocking entries: the launch on the null stream, then its completion
int batch_sync(const int8_t* x, int8_t* y, size_t B, int device, int layout) {
  if (const int rc = batch_async(x, y, B, device, nullptr, layout)) return rc;
  DeviceGuard guard(device);
  if (guard.err != hipSuccess) return hip_err(guard.err);
  return hip_err(hipStreamSynchronize(nullptr));
}

// The multi-device driver: (1) every listed device gets the parameter image before any shard is
// enqueued, so a first call uploads to all devices up front instead of starting them one after
// another; (2) every shard is enqueued (asynchronous launches), then (3) waited for.  On an
// enqueue error the shards already enqueued are waited for before returning.
template <class Prep, class Enq, class Wait>
int multi_driver(int ndev, const int* devices, bool wait_all, Prep&& prep, Enq&& enq, Wait&& wait) {
  for (int i = 0; i < ndev; i++) {
    bool seen = false;
    for (int j = 0; j < i; j++) seen = seen || devices[j] == devices[i];
    if (seen) continue;
    if (const int rc = prep(devices[i])) return rc;
  }
  for (int i = 0; i < ndev; i++) {
    if (const int rc = enq(i)) {
      (void)wait(i);
      return rc;
    }
  }
  return wait_all ? wait(ndev) : NET_OK;
}

int batch_multi(int ndev, const int* devices, const int8_t* const* x, int8_t* const* y, const size_t* B,
                void* const* streams, bool ct) {
  if (ndev < 1 || ndev > MAX_DEVICES || !devices || !x || !y || !B) return NET_ERR_INVALID;
  // one parameter snapshot for every shard (a concurrent net_params_load cannot split the batch)
  const Snapshot s = snapshot();
  if (!s.host) return NET_ERR_NO_PARAMS;
  auto wait = [&](int n) -> int {
    int first = NET_OK;
    for (int i = 0; i < n; i++) {
      DeviceGuard guard(devices[i]);
      hipError_t e = guard.err;
      if (e == hipSuccess) e = hipStreamSynchronize(streams ? (hipStream_t)streams[i] : nullptr);
      if (e != hipSuccess && first == NET_OK) first = hip_err(e);
    }
    return first;
  };
  auto enq = [&](int i) -> int {
    t_enqueueing = true;
    const int rc = batch_async_s(s, x[i], y[i], B[i], devices[i], streams ? streams[i] : nullptr, ct ? 1 : 0);
    t_enqueueing = false;
    return rc;
  };
  // the image made resident on the device (uploaded on first use)
  auto prep = [&](int d) { return DeviceScope(d, s, IMG_KERNELS).rc; };
  return multi_driver(ndev, devices, !streams, prep, enq, wait);
}

int launch_info(size_t B, int device, int32_t* out, bool ct) {
  if (!out || device < 0 || device >= MAX_DEVICES) return NET_ERR_INVALID;
  Snapshot s = snapshot();
  if (!s.host) return NET_ERR_NO_PARAMS;
  const Variant v = variant_of(*s.host);
  DeviceScope sc(device, s, IMG_KERNELS);
  if (sc.rc) return sc.rc;
  return launch_forward(v, s.img[IMG_KERNELS].data.get(), sc.ds, nullptr, nullptr, nullptr, B, nullptr, out, ct);
}

}  // namespace

// ================================ C ABI ======================================================
extern "C" {

int net_version(void) { return MIBMINET_VERSION; }

const char* net_error_string(int code) {
  switch (code) {
    case NET_OK: return "ok";
    case NET_ERR_INVALID: return "invalid argument";
    case NET_ERR_NO_PARAMS: return "no parameters loaded";
    case NET_ERR_UNSUPPORTED: return "unsupported network configuration";
    case NET_ERR_BLOB: return "malformed parameter blob";
    case NET_ERR_RANGE: return "value outside the defined range (the reference's int32 arithmetic overflows or divides by zero on these parameters, or a float-input scale outside [2^-60, 2^60])";
    default:
      if (code <= NET_ERR_HIP) return hipGetErrorString((hipError_t)(NET_ERR_HIP - code));
      return "unknown error";
  }
}

int net_params_load(const void* blob, size_t len) {
  auto hp = std::make_shared<HostParams>();
  if (const int rc = parse_blob(blob, len, *hp)) return rc;
  return install(hp);
}

int net_blob_widen(const void* blob, size_t len, int R, const int32_t* channels, void* out, size_t cap,
                   size_t* out_len) {
  return widen_blob(blob, len, R, channels, out, cap, out_len);
}

int net_params_load_arrays(const net_arrays_t* a) {
  auto hp = std::make_shared<HostParams>();
  if (const int rc = parse_arrays(a, *hp)) return rc;
  return install(hp);
}

int net_params_info(int32_t* info) {
  if (!info) return NET_ERR_INVALID;
  Snapshot s = snapshot();
  for (int i = 0; i < 5; i++) info[i] = 0;
  if (!s.host) return NET_ERR_NO_PARAMS;
  const HostParams& hp = *s.host;
  info[0] = hp.general ? NET_PATH_GENERAL : hp.xr ? NET_PATH_EXACT : NET_PATH_FLOAT;
  info[1] = hp.general || !hp.xr ? 0 : hp.xr_layer;
  info[2] = hp.general || !hp.xr ? -1 : hp.xr_filter;
  info[3] = hp.general ? -1 : compiled_shape(hp.d);
  info[4] = hp.xr ? 1 : 0;
  return NET_OK;
}

void net_params_unload(void) {
  {
    std::lock_guard<std::mutex> lk(g_mu);
    g_set = Snapshot{nullptr, {}, g_set.gen + 1};
  }
  // free every device copy once the launches that may read it have finished
  for (int d = 0; d < MAX_DEVICES; d++) {
    DeviceState& ds = g_devs[d];
    std::lock_guard<std::mutex> lk(ds.mu);
    if (ds.images.empty()) continue;
    DeviceGuard guard(d);
    if (guard.err != hipSuccess || hipDeviceSynchronize() != hipSuccess) continue;  // keep them
    for (DevImage& im : ds.images) free_image(im);
    ds.images.clear();
    ds.cur[0] = ds.cur[1] = nullptr;
  }
}

int net_params_dims(int32_t* dims) {
  if (!dims) return NET_ERR_INVALID;
  Snapshot s = snapshot();
  if (!s.host) {
    for (int i = 0; i < 7; i++) dims[i] = 0;
    return NET_ERR_NO_PARAMS;
  }
  const Dims& d = s.host->d;
  dims[0] = d.C; dims[1] = d.T; dims[2] = d.F1; dims[3] = d.F2; dims[4] = d.N; dims[5] = d.wbits; dims[6] = 1;
  return NET_OK;
}

size_t net_trial_stride(void) {
  Snapshot s = snapshot();
  return s.host ? trial_stride(s.host->d) : 0;
}

int net_set_device(int device) {
  if (const int rc = check_device(device)) return rc;
  g_single_device.store(device);
  return NET_OK;
}

int net_model_compute_batch_async(const int8_t* x, int8_t* y, size_t B, int device, void* stream) {
  return batch_async(x, y, B, device, stream, 0);
}

int net_model_compute_batch_ct(const int8_t* x, int8_t* y, size_t B, int device, void* stream) {
  return batch_async(x, y, B, device, stream, 1);
}

int net_model_compute_batch_f32(const float* x, int8_t* y, size_t B, float scale, int device, void* stream) {
  return batch_async((const int8_t*)x, y, B, device, stream, 2, scale);
}

int net_model_compute_batch(const int8_t* x, int8_t* y, size_t B, int device) { return batch_sync(x, y, B, device, 0); }

int net_model_compute_batch_ct_sync(const int8_t* x, int8_t* y, size_t B, int device) {
  return batch_sync(x, y, B, device, 1);
}

size_t net_streams_ring_samples(const net_bank_t* bank, size_t max_push) {
  return bank ? stream::ring_samples((size_t)bank->sets[0].T, max_push) : 0;
}

size_t net_streams_push_windows(const net_bank_t* bank, size_t hop, size_t pos, size_t n) {
  return bank ? stream::push_windows((size_t)bank->sets[0].T, hop, (uint64_t)pos, n) : 0;
}

int net_streams_create(const net_bank_t* bank, const int32_t* sets, size_t S, size_t hop, size_t max_push, int device,
                       net_streams_t** out) {
  return streams_create(bank, sets, S, hop, max_push, device, out);
}

void net_streams_destroy(net_streams_t* st) { streams_destroy(st); }

int net_streams_info(const net_streams_t* st, int64_t* info) {
  if (!st || !info) return NET_ERR_INVALID;
  info[0] = (int64_t)st->S; info[1] = (int64_t)std::min(st->hop, (size_t)INT64_MAX); info[2] = (int64_t)st->max_push;
  info[3] = (int64_t)st->cap; info[4] = (int64_t)st->pos; info[5] = st->each ? -1 : (int64_t)st->emitted;
  return NET_OK;
}

int net_streams_origin(const net_streams_t* st, size_t i, int64_t* origin, int32_t* set) {
  if (!st || i >= st->S || !origin || !set) return NET_ERR_INVALID;
  *origin = st->origin[i];
  *set = st->set[i];
  return NET_OK;
}

int net_streams_push(net_streams_t* st, const int8_t* x, int layout, size_t n, int8_t* y, int32_t* n_bad,
                     void* stream) {
  return streams_push(st, x, layout, false, n, y, n_bad, stream);
}

int net_streams_push_f32(net_streams_t* st, const float* x, size_t n, int8_t* y, int32_t* n_bad, void* stream) {
  return streams_push(st, x, 1, true, n, y, n_bad, stream);
}

int net_streams_push_f32_tm(net_streams_t* st, const float* x, size_t n, int8_t* y, int32_t* n_bad, void* stream) {
  return streams_push(st, x, gen::F32TM, true, n, y, n_bad, stream);
}

int net_streams_restart(net_streams_t* st, size_t i, int32_t set, void* stream) {
  return streams_restart(st, i, set, stream);
}

int net_streams_set_decimator(net_streams_t* st, size_t q, const float* taps, size_t K, void* stream) {
  return streams_set_decimator(st, q, taps, K, stream);
}

size_t net_streams_raw_samples(size_t q, size_t raw_pos, size_t n_raw) {
  return stream::raw_samples(q, (uint64_t)raw_pos, n_raw);
}

int net_streams_push_raw_f32_tm(net_streams_t* st, const float* x, size_t n_raw, int8_t* y, int32_t* n_bad,
                                void* stream) {
  return streams_push_raw(st, x, n_raw, y, n_bad, stream);
}

int net_streams_raw_info(const net_streams_t* st, int64_t* info) {
  if (!st || !info) return NET_ERR_INVALID;
  info[0] = (int64_t)st->q; info[1] = (int64_t)st->K; info[2] = (int64_t)st->raw_pos; info[3] = (int64_t)st->pos;
  if (st->each && st->q) info[2] = info[3] = -1;  // the positions are on the device
  return NET_OK;
}

int net_streams_set_decimator_each(net_streams_t* st, size_t q, const float* taps, size_t K, void* stream) {
  return streams_set_decimator(st, q, taps, K, stream, true);
}

int net_streams_set_prefilter(net_streams_t* st, const float* sos, size_t M, void* stream) {
  return streams_set_prefilter(st, sos, M, stream);
}

int net_streams_prefilter_info(const net_streams_t* st, int64_t* info) {
  if (!st || !info) return NET_ERR_INVALID;
  info[0] = (int64_t)st->M;
  info[1] = st->M ? (int64_t)(st->q * st->max_push) : 0;
  info[2] = st->M ? (int64_t)st->pat.bytes : 0;
  return NET_OK;
}

size_t net_streams_each_raw_rows(size_t hop, size_t q, size_t n_raw_max) {
  return stream::each_raw_rows(hop, q, n_raw_max);
}

int net_streams_push_each_raw_f32_tm(net_streams_t* st, const float* x, const int32_t* cnt_in, size_t n_raw_max, int8_t* y,
                                     int32_t* cnt_out, int64_t* win0, int32_t* n_bad, void* stream) {
  return streams_push_each_raw(st, x, cnt_in, n_raw_max, y, cnt_out, win0, n_bad, stream);
}

int net_streams_raw_positions(net_streams_t* st, int64_t* raw_pos_out, void* stream) {
  return streams_raw_positions(st, raw_pos_out, stream);
}

int net_streams_create_each(const net_bank_t* bank, const int32_t* sets, size_t S, size_t hop, size_t max_push,
                            int device, net_streams_t** out) {
  return streams_create(bank, sets, S, hop, max_push, device, out, true);
}

size_t net_streams_each_rows(size_t hop, size_t n_max) { return stream::each_rows(hop, n_max); }

int net_streams_push_each(net_streams_t* st, const int8_t* x, int layout, const int32_t* cnt_in, size_t n_max, int8_t* y,
                          int32_t* cnt_out, int64_t* win0, int32_t* n_bad, void* stream) {
  return streams_push_each(st, x, layout, false, cnt_in, n_max, y, cnt_out, win0, n_bad, stream);
}

int net_streams_push_each_f32(net_streams_t* st, const float* x, const int32_t* cnt_in, size_t n_max, int8_t* y,
                              int32_t* cnt_out, int64_t* win0, int32_t* n_bad, void* stream) {
  return streams_push_each(st, x, 1, true, cnt_in, n_max, y, cnt_out, win0, n_bad, stream);
}

int net_streams_push_each_f32_tm(net_streams_t* st, const float* x, const int32_t* cnt_in, size_t n_max, int8_t* y,
                                 int32_t* cnt_out, int64_t* win0, int32_t* n_bad, void* stream) {
  return streams_push_each(st, x, gen::F32TM, true, cnt_in, n_max, y, cnt_out, win0, n_bad, stream);
}

int net_streams_positions(net_streams_t* st, int64_t* pos_out, void* stream) {
  return streams_positions(st, pos_out, stream);
}

int net_streams_windows_at(net_streams_t* st, const int32_t* session, const int64_t* onsets, size_t W, int8_t* y,
                           int32_t* n_bad, void* stream) {
  return streams_windows_at(st, session, onsets, W, y, n_bad, stream);
}

int net_streams_windows_at_feat(net_streams_t* st, const int32_t* session, const int64_t* onsets, size_t W, int8_t* y,
                                int8_t* feat, int32_t* n_bad, void* stream) {
  return streams_windows_at(st, session, onsets, W, y, n_bad, stream, true, feat);
}

int net_streams_at_span(const net_streams_t* st, int64_t* lo, int64_t* hi) { return streams_at_span(st, lo, hi); }

int net_model_compute_batch_multi(int ndev, const int* devices, const int8_t* const* x, int8_t* const* y,
                                  const size_t* B, void* const* streams) {
  return batch_multi(ndev, devices, x, y, B, streams, false);
}

int net_model_compute_batch_multi_ct(int ndev, const int* devices, const int8_t* const* x, int8_t* const* y,
                                     const size_t* B, void* const* streams) {
  return batch_multi(ndev, devices, x, y, B, streams, true);
}

size_t net_windows_count(size_t L, size_t hop) {
  const Snapshot s = snapshot();
  return s.host ? windows_count((size_t)s.host->d.T, L, hop) : 0;
}

size_t net_windows_row_stride(size_t L) { return windows_row_stride(L); }

size_t net_windows_workspace(size_t L) { return windows_workspace(L); }

int net_model_compute_windows(const int8_t* x, int layout, size_t L, size_t hop, int8_t* y, void* ws, size_t ws_bytes,
                              int device, void* stream) {
  return windows_async(x, layout, false, L, false, hop, nullptr, 0, 0.0f, y, nullptr, ws, ws_bytes, device, stream);
}

int net_model_compute_windows_f32(const float* x, size_t L, size_t hop, float scale, int8_t* y, void* ws,
                                  size_t ws_bytes, int device, void* stream) {
  return windows_async(x, 1, true, L, false, hop, nullptr, 0, scale, y, nullptr, ws, ws_bytes, device, stream);
}

int net_model_compute_windows_at(const int8_t* x, int layout, size_t L, const int64_t* onsets, size_t W, int8_t* y,
                                 int32_t* n_bad, void* ws, size_t ws_bytes, int device, void* stream) {
  return windows_async(x, layout, false, L, true, 0, onsets, W, 0.0f, y, n_bad, ws, ws_bytes, device, stream);
}

int net_model_compute_windows_at_f32(const float* x, size_t L, const int64_t* onsets, size_t W, float scale, int8_t* y,
                                     int32_t* n_bad, void* ws, size_t ws_bytes, int device, void* stream) {
  return windows_async(x, 1, true, L, true, 0, onsets, W, scale, y, n_bad, ws, ws_bytes, device, stream);
}

int net_model_compute_windows_f32_tm(const float* x, size_t L, size_t hop, float scale, int8_t* y, void* ws,
                                     size_t ws_bytes, int device, void* stream) {
  return windows_async(x, gen::F32TM, true, L, false, hop, nullptr, 0, scale, y, nullptr, ws, ws_bytes, device, stream);
}

int net_model_compute_windows_at_f32_tm(const float* x, size_t L, const int64_t* onsets, size_t W, float scale,
                                        int8_t* y, int32_t* n_bad, void* ws, size_t ws_bytes, int device, void* stream) {
  return windows_async(x, gen::F32TM, true, L, true, 0, onsets, W, scale, y, n_bad, ws, ws_bytes, device, stream);
}

size_t net_windows_multi_count(const size_t* lengths, size_t R, size_t hop) {
  return windows_multi_loaded(lengths, R, hop, nullptr, 0, nullptr);
}

size_t net_windows_multi_onsets(const size_t* lengths, size_t R, size_t hop, int64_t* onsets, size_t cap,
                                size_t* first) {
  return windows_multi_loaded(lengths, R, hop, onsets, cap, first);
}

int net_model_compute_epochs(const int8_t* x, size_t n_elems, size_t row_stride, const int32_t* channels,
                             const int64_t* onsets, size_t E, int8_t* y, int32_t* n_bad, int device, void* stream) {
  return epochs_async(x, false, n_elems, row_stride, channels, onsets, E, 0.0f, y, n_bad, device, stream);
}

int net_model_compute_epochs_f32(const float* x, size_t n_elems, size_t row_stride, const int32_t* channels,
                                 const int64_t* onsets, size_t E, float scale, int8_t* y, int32_t* n_bad,
                                 int device, void* stream) {
  return epochs_async(x, true, n_elems, row_stride, channels, onsets, E, scale, y, n_bad, device, stream);
}

// The images of the sets (bank::build, bank_host.hpp) in a net_bank of their own.
int net_bank_create(const void* const* blobs, const size_t* sizes, const float* scales, size_t n_sets,
                    net_bank_t** bank, size_t* failed) {
  if (bank) *bank = nullptr;
  if (!blobs || !sizes || !bank || n_sets == 0 || n_sets > NET_BANK_MAX_SETS) return NET_ERR_INVALID;
  auto b = std::make_unique<net_bank>();
  if (const int rc = bank::build(blobs, sizes, scales, n_sets, g_force_general.load() != 0, b->sets, b->scales, failed,
                                 &b->rec))
    return rc;
  *bank = b.release();
  return NET_OK;
}

int net_bank_info(const net_bank_t* bank, int32_t* info) {
  if (!bank || !info) return NET_ERR_INVALID;
  const gen::GenParams& g = bank->sets[0];
  info[0] = (int32_t)bank->sets.size(); info[1] = g.C; info[2] = g.T; info[3] = g.N; info[4] = g.xr;
  info[5] = bank->scales.empty() ? 0 : 1; info[6] = (int32_t)sizeof(gen::GenParams);
  return NET_OK;
}

void net_bank_destroy(net_bank_t* bank) { bank_destroy(bank); }

int net_bank_replace(net_bank_t* bank, size_t set, const void* blob, size_t len, float scale, int device,
                     void* stream) {
  return bank_replace(bank, set, blob, len, scale, device, stream);
}

size_t net_bank_feature_bytes(const net_bank_t* bank) { return bank ? (size_t)16 * (size_t)bank->sets[0].T64 : 0; }

int net_model_compute_epochs_bank(const net_bank_t* bank, const int8_t* x, size_t n_elems, size_t row_stride,
                                  const int32_t* channels, const int64_t* onsets, const int32_t* set_of, size_t E,
                                  int8_t* y, int32_t* n_bad, int device, void* stream) {
  return bank_epochs_async(bank, x, false, n_elems, row_stride, channels, onsets, set_of, E, y, n_bad, device, stream);
}

int net_model_compute_epochs_bank_f32(const net_bank_t* bank, const float* x, size_t n_elems, size_t row_stride,
                                      const int32_t* channels, const int64_t* onsets, const int32_t* set_of, size_t E,
                                      int8_t* y, int32_t* n_bad, int device, void* stream) {
  return bank_epochs_async(bank, x, true, n_elems, row_stride, channels, onsets, set_of, E, y, n_bad, device, stream);
}

int net_model_compute_epochs_bank_feat(const net_bank_t* bank, const int8_t* x, size_t n_elems, size_t row_stride,
                                       const int32_t* channels, const int64_t* onsets, const int32_t* set_of, size_t E,
                                       int8_t* y, int8_t* feat, int32_t* n_bad, int device, void* stream) {
  return bank_epochs_async(bank, x, false, n_elems, row_stride, channels, onsets, set_of, E, y, n_bad, device, stream,
                           true, feat);
}

int net_model_compute_epochs_bank_feat_f32(const net_bank_t* bank, const float* x, size_t n_elems, size_t row_stride,
                                           const int32_t* channels, const int64_t* onsets, const int32_t* set_of,
                                           size_t E, int8_t* y, int8_t* feat, int32_t* n_bad, int device, void* stream) {
  return bank_epochs_async(bank, x, true, n_elems, row_stride, channels, onsets, set_of, E, y, n_bad, device, stream,
                           true, feat);
}

int net_model_compute_windows_bank(const net_bank_t* bank, const int8_t* x, int layout, size_t L,
                                   const int32_t* blk_set, const int64_t* onsets, size_t W, int8_t* y,
                                   int32_t* n_bad, void* ws, size_t ws_bytes, int device, void* stream) {
  return bank_windows_async(bank, x, layout, false, L, blk_set, onsets, W, y, n_bad, ws, ws_bytes, device, stream);
}

int net_model_compute_windows_bank_f32(const net_bank_t* bank, const float* x, size_t L, const int32_t* blk_set,
                                       const int64_t* onsets, size_t W, int8_t* y, int32_t* n_bad, void* ws,
                                       size_t ws_bytes, int device, void* stream) {
  return bank_windows_async(bank, x, 1, true, L, blk_set, onsets, W, y, n_bad, ws, ws_bytes, device, stream);
}

int net_model_compute_windows_bank_f32_tm(const net_bank_t* bank, const float* x, size_t L, const int32_t* blk_set,
                                          const int64_t* onsets, size_t W, int8_t* y, int32_t* n_bad, void* ws,
                                          size_t ws_bytes, int device, void* stream) {
  return bank_windows_async(bank, x, gen::F32TM, true, L, blk_set, onsets, W, y, n_bad, ws, ws_bytes, device, stream);
}

size_t net_bank_windows_starts(const size_t* lengths, size_t R, int64_t* starts) {
  return bank::windows_starts(lengths, R, starts);
}

size_t net_bank_windows_lists(const net_bank_t* bank, const size_t* lengths, const int32_t* sets, size_t R,
                              size_t hop, int32_t* blk_set, size_t n_blk, int64_t* onsets, size_t cap, size_t* first) {
  if (!bank) return 0;
  return bank::windows_lists((size_t)bank->sets[0].T, bank->sets.size(), lengths, sets, R, hop, blk_set, n_blk, onsets,
                             cap, first);
}

int net_quantize_input_f32(const float* x, int8_t* y, size_t B, int C, int T, float scale, int device, void* stream) {
  return quantize_input<float>(x, y, B, C, T, scale, device, stream);
}

int net_quantize_input_f64(const double* x, int8_t* y, size_t B, int C, int T, double scale, int device, void* stream) {
  return quantize_input<double>(x, y, B, C, T, scale, device, stream);
}

int net_pack_trials_i8(const int8_t* x, int8_t* y, size_t B, int C, int T, int device, void* stream) {
  return quantize_input<int8_t>(x, y, B, C, T, (int8_t)1, device, stream);
}

int net_argmax_batch(const int8_t* logits, int32_t* cls, size_t B, int N, int device, void* stream) {
  return argmax_batch(logits, cls, B, N, device, stream);
}

int net_launch_info(size_t B, int device, int32_t* out) { return launch_info(B, device, out, false); }

int net_launch_info_ct(size_t B, int device, int32_t* out) { return launch_info(B, device, out, true); }

int net_forward(const int8_t* p_data, int8_t* p_output) { return run_single(0, p_data, p_output); }

void net_model_compute(const int8_t* p_data, int8_t* p_output) { t_last_error = run_single(0, p_data, p_output); }
void net_layer1(const int8_t* p_data, int8_t* p_result) { t_last_error = run_single(1, p_data, p_result); }
void net_layer2(const int8_t* p_data, int8_t* p_result) { t_last_error = run_single(2, p_data, p_result); }
void net_layer3(const int8_t* p_data, int8_t* p_result) { t_last_error = run_single(3, p_data, p_result); }
void net_layer3_flip_inplace(int8_t* p_data) { t_last_error = run_single(6, p_data, p_data); }
void net_layer4(const int8_t* p_data, int8_t* p_result) { t_last_error = run_single(4, p_data, p_result); }
void net_layer5(const int8_t* p_data, int8_t* p_result) { t_last_error = run_single(5, p_data, p_result); }

int net_last_error(void) { return t_last_error; }

}  // extern "C"

#include "test_hooks.hpp"
