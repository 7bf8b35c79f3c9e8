// device_state.hpp — the loaded set and the per-device state of libmibminet.so: the parameter-image
// cache, the single-trial scratch and the scoped entry every launching call goes through.  Holds
// the library's globals: included by mibminet.hip only.  (MAX_DEVICES, which the entries' argument
// checks need too, is entry_host.hpp's.)
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>
#include <optional>
#include <utility>
#include <vector>

#include "bank_host.hpp"     // bank::Record
#include "entry_host.hpp"    // MAX_DEVICES
#include "image_layout.hpp"  // gen::GenParams, bank::Scale
#include "images.hpp"        // Image

// A parameter bank (net_bank_t, include/mibminet.h): the images of its sets (the host master) and
// one device copy per device that has run a call on it.  A copy is the n_sets images followed, for a
// bank with scales, by n_sets bank::Scale entries.  net_bank_replace changes one slot of the master
// and of a device's copy; what it never changes is rec, the number of sets and the head of every
// image (the geometry and flags before gen::GenParams::l3_m, which the record fixes), so the
// launching calls read those of sets[0] without the lock.  Banks live beside the loaded set, not in
// it: nothing here touches g_set or a device's image cache.
struct net_bank {
  std::vector<mib::gen::GenParams> sets;
  std::vector<mib::bank::Scale> scales;  // empty: created without scales
  mib::bank::Record rec;                 // what the bank was created with
  mutable std::mutex mu;                           // guards dev, staging and the slots' bodies
  mutable std::vector<std::pair<int, void*>> dev;  // (device, its copy)
  // net_bank_replace's pinned sources (one image and one scale entry each) with the event recorded
  // behind the copies that read them: a buffer is used again once its event has completed
  std::vector<std::pair<void*, hipEvent_t>> staging;
};

namespace mib {
namespace {

// One device copy of the parameter image per loaded generation: a load never overwrites a copy
// that a kernel may still read, so launches in flight and launches captured into a HIP graph keep
// the image (and with it the compiled variant) they were enqueued with.  A reload of a
// byte-identical image reuses its copy.  When a new image would make more than MAX_IMAGES copies,
// only copies that no launch can still read are freed, least recently used first: every batched
// launch records an event per (copy, stream), and a copy is free once all its events have
// completed.  A copy used by a launch under stream capture (a HIP graph may replay it at any
// time) or on more than MAX_STREAMS streams is kept until net_params_unload.  Nothing here waits
// for the device, so a load never stalls or breaks a caller's capture; if no copy can be freed
// the device simply keeps more than MAX_IMAGES.  net_params_unload synchronises each device and
// frees every copy (graphs that captured a launch must not be replayed after it).
constexpr size_t MAX_IMAGES = 8;
constexpr size_t MAX_STREAMS = 16;

struct DevImage {
  Image host;                             // what was uploaded
  void* dev = nullptr;
  uint64_t used = 0;                      // DeviceState::tick at the last selection
  bool pinned = false;                    // captured into a graph (or too many streams): kept
  std::vector<std::pair<hipStream_t, hipEvent_t>> last;  // the last launch per stream
};

// The two images of a set: what the batched kernels read (DevParams or gen::GenParams) and the
// window and epoch kernels' gen::GenParams (the same copy on the general path).
enum { IMG_KERNELS = 0, IMG_WINDOWS = 1 };

struct DeviceState {
  std::mutex mu;
  void* cur[2] = {nullptr, nullptr};  // device copy of each image of generation gen[i]
  uint64_t gen[2] = {0, 0};
  std::vector<DevImage> images; // the copies uploaded to this device
  uint64_t tick = 0;
  int8_t* d_in = nullptr;       // single-trial scratch
  int8_t* d_out = nullptr;
  int8_t* h_in = nullptr;       // pinned host staging of the single-trial copies
  int8_t* h_out = nullptr;
  hipStream_t st = nullptr;     // the single-trial path's own non-blocking stream
  size_t scratch = 0;
  int cus = 0;
};

struct Snapshot {
  std::shared_ptr<const HostParams> host;
  Image img[2];  // IMG_KERNELS, IMG_WINDOWS (empty: none could be built)
  uint64_t gen = 0;
};

std::mutex g_mu;
Snapshot g_set;  // the loaded set
DeviceState g_devs[MAX_DEVICES];
std::atomic<int> g_single_device{0};  // net_set_device (read by every single-trial call)
std::atomic<int> g_device_count{-1};
// test counters (mibminet_test_upload_stats): parameter uploads, and those made while
// batch_multi was enqueueing shards (must stay 0: every device is prepared first)
std::atomic<long> g_uploads{0}, g_uploads_enqueue{0};
thread_local bool t_enqueueing = false;

inline int hip_err(hipError_t e) { return e == hipSuccess ? NET_OK : NET_ERR_HIP - (int)e; }

// NET_OK if `device` names a visible HIP device, NET_ERR_INVALID otherwise (or the HIP error).
int check_device(int device) {
  int n = g_device_count.load();
  if (n < 0) {
    const hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return hip_err(e);
    g_device_count.store(n);
  }
  return (device >= 0 && device < n && device < MAX_DEVICES) ? NET_OK : NET_ERR_INVALID;
}

struct DeviceGuard {  // makes `dev` current and restores the caller's device; err: hipSetDevice's status
  int old = -1;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&old) != hipSuccess) old = -1;
    err = hipSetDevice(dev);
  }
  ~DeviceGuard() { if (old >= 0) (void)hipSetDevice(old); }
};

Snapshot snapshot() {
  std::lock_guard<std::mutex> lk(g_mu);
  return g_set;
}

void free_image(DevImage& im) {
  for (auto& se : im.last) (void)hipEventDestroy(se.second);
  im.last.clear();
  (void)hipFree(im.dev);
  im.dev = nullptr;
}

// no launch recorded on the copy can still be running (graph-captured copies never qualify)
bool image_idle(const DevImage& im) {
  if (im.pinned) return false;
  for (const auto& se : im.last)
    if (hipEventQuery(se.second) != hipSuccess) return false;
  return true;
}

// Frees least-recently-used idle copies (never a current one) until fewer than MAX_IMAGES remain or
// none is idle.  No device synchronisation.
void evict_idle(DeviceState& ds) {
  while (ds.images.size() >= MAX_IMAGES) {
    int victim = -1;
    for (int i = 0; i < (int)ds.images.size(); i++) {
      const DevImage& im = ds.images[i];
      if (im.dev == ds.cur[0] || im.dev == ds.cur[1] || !image_idle(im)) continue;
      if (victim < 0 || im.used < ds.images[victim].used) victim = i;
    }
    if (victim < 0) return;
    free_image(ds.images[victim]);
    ds.images.erase(ds.images.begin() + victim);
  }
}

// After a batched launch that reads the device copy `dev` on `st` (ds.mu held, device current):
// remember it, so that the copy is freed only once the launch has finished.  Under stream capture
// the copy is pinned.
void note_launch(DeviceState& ds, const void* dev, hipStream_t st) {
  for (DevImage& im : ds.images) {
    if (im.dev != dev) continue;
    if (im.pinned) return;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
      im.pinned = true;  // a graph may replay this launch at any time
      return;
    }
    for (auto& se : im.last)
      if (se.first == st) {
        if (hipEventRecord(se.second, st) != hipSuccess) im.pinned = true;
        return;
      }
    hipEvent_t ev = nullptr;
    if (im.last.size() >= MAX_STREAMS || hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
      im.pinned = true;
      return;
    }
    if (hipEventRecord(ev, st) != hipSuccess) {
      (void)hipEventDestroy(ev);
      im.pinned = true;
      return;
    }
    im.last.emplace_back(st, ev);
    return;
  }
}

// ds.cus, the device's compute units (asked once); ds.mu held.
int ensure_cus(DeviceState& ds, int dev) {
  if (ds.cus) return NET_OK;
  int cus = 0;
  hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e != hipSuccess) return hip_err(e);
  ds.cus = cus;
  return NET_OK;
}

// Ensure `dev` holds image `which` of snapshot s, ds.cur[which] pointing to its copy; called with
// ds.mu held and the device current.  The window image of a general set is the copy of its kernels'
// image (the same bytes).
int ensure_image(DeviceState& ds, int dev, const Snapshot& s, int which) {
  if (!s.host) return NET_ERR_NO_PARAMS;
  const Image& img = s.img[which];
  if (!img.data) return NET_ERR_UNSUPPORTED;
  if (const int rc = ensure_cus(ds, dev)) return rc;
  void*& cur = ds.cur[which];
  if (ds.gen[which] == s.gen && cur) return NET_OK;
  for (DevImage& im : ds.images)  // a set loaded before: its copy is still there, unchanged
    if (im.host.same(img)) {
      cur = im.dev;
      ds.gen[which] = s.gen;
      im.used = ++ds.tick;
      return NET_OK;
    }
  evict_idle(ds);
  DevImage im;
  im.host = img;
  im.used = ++ds.tick;
  hipError_t e = hipMalloc(&im.dev, img.bytes);
  if (e != hipSuccess) return hip_err(e);
  e = hipMemcpy(im.dev, img.data.get(), img.bytes, hipMemcpyHostToDevice);
  g_uploads++;
  if (t_enqueueing) g_uploads_enqueue++;
  if (e != hipSuccess) {
    (void)hipFree(im.dev);
    return hip_err(e);
  }
  ds.images.push_back(std::move(im));
  cur = ds.images.back().dev;
  ds.gen[which] = s.gen;
  return NET_OK;
}

// Single-trial scratch: device buffers, pinned host staging (the copies run as DMA without the
// runtime's pageable bounce) and a non-blocking stream (no implicit sync with the null stream).
int ensure_scratch(DeviceState& ds, size_t bytes) {
  if (!ds.st) {
    hipError_t e = hipStreamCreateWithFlags(&ds.st, hipStreamNonBlocking);
    if (e != hipSuccess) {
      ds.st = nullptr;
      return hip_err(e);
    }
  }
  if (ds.scratch >= bytes) return NET_OK;
  if (ds.d_in) (void)hipFree(ds.d_in);
  if (ds.d_out) (void)hipFree(ds.d_out);
  if (ds.h_in) (void)hipHostFree(ds.h_in);
  if (ds.h_out) (void)hipHostFree(ds.h_out);
  ds.d_in = ds.d_out = ds.h_in = ds.h_out = nullptr;
  ds.scratch = 0;
  hipError_t e = hipMalloc((void**)&ds.d_in, bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&ds.d_out, bytes);
  if (e == hipSuccess) e = hipHostMalloc((void**)&ds.h_in, bytes, hipHostMallocMapped | hipHostMallocCoherent);
  if (e == hipSuccess) e = hipHostMalloc((void**)&ds.h_out, bytes, hipHostMallocMapped | hipHostMallocCoherent);
  if (e != hipSuccess) return hip_err(e);
  ds.scratch = bytes;
  return NET_OK;
}

// The device copy of a bank on `dev`, uploaded on the first call there; ds.mu held and the device
// current.  The upload is the one allocation and host sync of a bank call.
int ensure_bank(const net_bank& b, int dev, void** copy) {
  std::lock_guard<std::mutex> lk(b.mu);
  for (const auto& c : b.dev)
    if (c.first == dev) {
      *copy = c.second;
      return NET_OK;
    }
  const size_t ib = b.sets.size() * sizeof(gen::GenParams), sb = b.scales.size() * sizeof(bank::Scale);
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, ib + sb);
  if (e != hipSuccess) return hip_err(e);
  e = hipMemcpy(p, b.sets.data(), ib, hipMemcpyHostToDevice);
  if (e == hipSuccess && sb) e = hipMemcpy((char*)p + ib, b.scales.data(), sb, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(p);
    return hip_err(e);
  }
  b.dev.emplace_back(dev, p);
  *copy = p;
  return NET_OK;
}

// The entry of every call that launches on `device`: checks the device (unless net_set_device
// already did), takes its lock and makes it current for the scope; then, with the loaded set,
// ensures image `which` of snapshot s, or, with a bank, the bank's copy.  rc != NET_OK: nothing
// else is valid.
struct DeviceScope {
  int rc;
  DeviceState& ds;
  std::unique_lock<std::mutex> lk;
  std::optional<DeviceGuard> guard;  // after lk: the caller's device comes back before the lock goes
  void* image = nullptr;             // the device copy of the requested image (of the bank)
  DeviceScope(int device, const Snapshot& s, int which, bool check = true)
      : rc(check ? check_device(device) : NET_OK), ds(g_devs[rc ? 0 : device]) {
    if (enter(device)) return;
    rc = ensure_image(ds, device, s, which);
    image = ds.cur[which];
  }
  DeviceScope(int device, const net_bank& b) : rc(check_device(device)), ds(g_devs[rc ? 0 : device]) {
    if (enter(device)) return;
    rc = ensure_cus(ds, device);
    if (rc == NET_OK) rc = ensure_bank(b, device, &image);
  }

 private:
  int enter(int device) {
    if (rc) return rc;
    lk = std::unique_lock<std::mutex>(ds.mu);
    guard.emplace(device);
    return rc = guard->err != hipSuccess ? hip_err(guard->err) : NET_OK;
  }
};

}  // namespace
}  // namespace mib
