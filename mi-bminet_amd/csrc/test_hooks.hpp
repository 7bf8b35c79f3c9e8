// test_hooks.hpp — the hooks of include/mibminet_testing.h.  Included last by mibminet.hip: they
// call into its internals and the headers it includes.
#pragma once

extern "C" {

int mibminet_test_reciprocal(int32_t fac, int64_t vmax, int32_t kmax, int32_t magic, float* r, float* c) {
  if (!r || (magic && !c) || vmax < 0 || vmax >= (1 << 24)) return NET_ERR_INVALID;
  return choose_reciprocal(fac, r, magic ? c : nullptr, kmax, vmax) ? NET_OK : NET_ERR_RANGE;
}

int mibminet_test_quantize_f32(const float* x, int8_t* q, size_t n, float scale, int device, void* stream) {
  if ((!x || !q) && n) return NET_ERR_INVALID;
  if (const int rc = check_scale(scale)) return rc;
  if (const int rc = check_device(device)) return rc;
  if (n == 0) return NET_OK;
  DeviceGuard guard(device);
  if (guard.err != hipSuccess) return hip_err(guard.err);
  hipLaunchKernelGGL(wg::k_quantize_flat, dim3(4096), dim3(256), 0, (hipStream_t)stream, x, q, (long long)n, scale,
                     recip_scale(scale));
  return hip_err(hipGetLastError());
}

int mibminet_test_floor_form(int32_t fac, int64_t emax, int64_t vmax, int32_t* mbits, float* r, float* c) {
  if (!mbits || !r || !c || vmax < 0 || emax < 0) return NET_ERR_INVALID;
  return choose_floor_form(fac, emax, vmax, mbits, r, c) ? NET_OK : NET_ERR_RANGE;
}

int mibminet_test_multi_order(int ndev, const int* devices, int fail_at, char* log, size_t len) {
  if (!log || !len || ndev < 1 || ndev > MAX_DEVICES || !devices) return NET_ERR_INVALID;
  std::string out;
  auto prep = [&](int d) { out += "P" + std::to_string(d) + " "; return NET_OK; };
  auto enq = [&](int i) {
    out += "E" + std::to_string(i) + " ";
    return i == fail_at ? NET_ERR_INVALID : NET_OK;
  };
  auto wait = [&](int n) { out += "W" + std::to_string(n) + " "; return NET_OK; };
  const int rc = multi_driver(ndev, devices, true, prep, enq, wait);
  std::snprintf(log, len, "%s", out.c_str());
  return rc;
}

int mibminet_test_upload_stats(int64_t* uploads, int64_t* uploads_while_enqueueing) {
  if (!uploads || !uploads_while_enqueueing) return NET_ERR_INVALID;
  *uploads = g_uploads.load();
  *uploads_while_enqueueing = g_uploads_enqueue.load();
  return NET_OK;
}

int mibminet_test_xdiv_host(const int32_t* e, size_t n, int32_t d, int32_t* q) {
  if ((!e || !q) && n) return NET_ERR_INVALID;
  if (d == 0) return NET_ERR_INVALID;
  const XDiv c = xdiv_consts(d);
  for (size_t i = 0; i < n; i++) q[i] = xdiv_host(e[i], c);
  return NET_OK;
}

int mibminet_test_xdiv_gpu(int32_t d, int64_t e0, int64_t count, int64_t* mismatches, int device) {
  if (!mismatches || d == 0 || count < 0 || e0 < INT32_MIN || e0 + count - 1 > INT32_MAX) return NET_ERR_INVALID;
  if (const int rc = check_device(device)) return rc;
  DeviceGuard guard(device);
  if (guard.err != hipSuccess) return hip_err(guard.err);
  constexpr int GRID = 2048, THREADS = 256;
  unsigned long long* dn = nullptr;
  hipError_t e = hipMalloc((void**)&dn, sizeof(unsigned long long) * GRID * THREADS);
  if (e != hipSuccess) return hip_err(e);
  const XDiv c = xdiv_consts(d);
  hipLaunchKernelGGL(k_xdiv_check, dim3(GRID), dim3(THREADS), 0, nullptr, d, c.m, c.xs, (long long)e0, (long long)count, dn);
  e = hipGetLastError();
  std::vector<unsigned long long> h((size_t)GRID * THREADS);
  if (e == hipSuccess) e = hipMemcpy(h.data(), dn, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost);
  (void)hipFree(dn);
  if (e != hipSuccess) return hip_err(e);
  int64_t n = 0;
  for (unsigned long long v : h) n += (int64_t)v;
  *mismatches = n;
  return NET_OK;
}

int mibminet_test_pool_consts(int32_t off, int32_t layer, int32_t* thr, int32_t* offm) {
  if (!thr || !offm || (layer != 2 && layer != 4)) return NET_ERR_INVALID;
  pool_consts(off, layer == 2 ? (1 << 20) : (1 << 18), thr, offm);
  return NET_OK;
}

int mibminet_test_image_digest(uint64_t* digest) {
  if (!digest) return NET_ERR_INVALID;
  Snapshot s = snapshot();
  if (!s.host) return NET_ERR_NO_PARAMS;
  *digest = fnv1a(s.img[IMG_KERNELS]);
  return NET_OK;
}

int mibminet_test_image_copy(int which, void* buf, size_t cap, size_t* bytes) {
  if (!bytes) return NET_ERR_INVALID;
  *bytes = 0;
  if (which != IMG_KERNELS && which != IMG_WINDOWS) return NET_ERR_INVALID;
  Snapshot s = snapshot();
  if (!s.host) return NET_ERR_NO_PARAMS;
  const Image& img = s.img[which];
  if (!img.data) return NET_ERR_UNSUPPORTED;
  *bytes = img.bytes;
  if (!buf) return NET_OK;
  if (cap < img.bytes) return NET_ERR_INVALID;
  std::memcpy(buf, img.data.get(), img.bytes);
  return NET_OK;
}

int mibminet_test_folded_filters(int32_t* count) {
  if (!count) return NET_ERR_INVALID;
  Snapshot s = snapshot();
  if (!s.host) return NET_ERR_NO_PARAMS;
  *count = s.host->folded;
  return NET_OK;
}

int mibminet_test_force_general(int on) {
  g_force_general.store(on ? 1 : 0);
  return NET_OK;
}

int mibminet_test_grid_cap(int workgroups) {
  if (workgroups < 0) return NET_ERR_INVALID;
  g_grid_cap.store(workgroups);
  return NET_OK;
}

int mibminet_test_params_xr(void) {
  Snapshot s = snapshot();
  if (!s.host) return NET_ERR_NO_PARAMS;
  return s.host->xr ? 1 : 0;
}

int mibminet_test_device_images(int device) {
  if (device < 0 || device >= MAX_DEVICES) return NET_ERR_INVALID;
  DeviceState& ds = g_devs[device];
  std::lock_guard<std::mutex> lk(ds.mu);
  return (int)ds.images.size();
}

int mibminet_test_bank_copy(const net_bank_t* bank, size_t set, void* buf, size_t cap, size_t* bytes) {
  if (!bytes) return NET_ERR_INVALID;
  *bytes = 0;
  if (!bank || set >= bank->sets.size()) return NET_ERR_INVALID;
  *bytes = sizeof(gen::GenParams);
  if (!buf) return NET_OK;
  if (cap < *bytes) return NET_ERR_INVALID;
  std::lock_guard<std::mutex> lk(bank->mu);  // net_bank_replace writes a slot under it
  std::memcpy(buf, &bank->sets[set], *bytes);
  return NET_OK;
}

int mibminet_test_bank_device_copies(const net_bank_t* bank) {
  if (!bank) return NET_ERR_INVALID;
  std::lock_guard<std::mutex> lk(bank->mu);
  return (int)bank->dev.size();
}

int mibminet_test_streams_ring(const net_streams_t* st, size_t i, void* out) {
  if (!st || i >= st->S || !out) return NET_ERR_INVALID;
  DeviceState& ds = g_devs[st->device];
  std::lock_guard<std::mutex> lk(ds.mu);
  DeviceGuard guard(st->device);
  if (guard.err != hipSuccess) return hip_err(guard.err);
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, (const char*)st->mem + i * st->at.base.ring, st->at.base.ring, hipMemcpyDeviceToHost);
  return hip_err(e);
}

int mibminet_test_streams_seek(net_streams_t* st, const int64_t* pos, const int64_t* origin) {
  if (!st) return NET_ERR_INVALID;
  DeviceState& ds = g_devs[st->device];
  std::lock_guard<std::mutex> lk(ds.mu);
  const bool fresh = st->pos == 0 && st->raw_pos == 0 && !st->restarted && !st->seeked;
  if (const int rc = stream::check_seek(true, st->each, fresh, st->S, st->q, pos, origin)) return rc;
  DeviceGuard guard(st->device);
  if (guard.err != hipSuccess) return hip_err(guard.err);
  const size_t S = st->S, q = st->q;
  auto D = [q](int64_t P) { return q ? (int64_t)stream::raw_decimated(q, (uint64_t)P) : P; };
  // what the device gets: a uniform group's origins, an each-group's (decimated) positions
  std::vector<int64_t> v(S);
  for (size_t s = 0; s < S; s++) v[s] = st->each ? D(pos[s]) : origin ? origin[s] : D(pos[0]);
  char* const to = (char*)st->mem + (st->each ? st->at.pos : st->at.base.origin);
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess && st->each && q)  // the raw positions first: a failure leaves the pair as it was or unread
    e = hipMemcpy((char*)st->dmem + st->dea.raw_pos, pos, 8 * S, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(to, v.data(), 8 * S, hipMemcpyHostToDevice);
  if (e != hipSuccess) return hip_err(e);
  if (!st->each) {
    st->raw_pos = q ? (uint64_t)pos[0] : 0;
    st->pos = (uint64_t)D(pos[0]);
    st->origin = v;
  }
  st->seeked = true;
  return NET_OK;
}

int mibminet_test_fir_decimate(const float* x, size_t n_raw, size_t R, const float* hist, const float* taps, size_t K,
                               size_t q, size_t raw_pos, float* out, int device, void* stream) {
  if (R < 1 || R > 64 || q < 1 || q > stream::MAX_Q || K < 1 || K > stream::MAX_TAPS || !taps) return NET_ERR_INVALID;
  if (n_raw > stream::MAX_Q * stream::MAX_PUSH || (uint64_t)raw_pos > (uint64_t)INT64_MAX - n_raw) return NET_ERR_INVALID;
  if ((!x && n_raw) || (!hist && K > 1)) return NET_ERR_INVALID;
  if (const int rc = check_device(device)) return rc;
  const size_t m = stream::raw_samples(q, raw_pos, n_raw);
  if (m == 0) return NET_OK;
  if (!out) return NET_ERR_INVALID;
  DeviceGuard guard(device);
  if (guard.err != hipSuccess) return hip_err(guard.err);
  const uint64_t d0 = stream::raw_decimated(q, raw_pos);
  const stream::Decim dc{taps, (const int8_t*)hist, (int)K, (int)q, (int)(d0 * q - raw_pos),
                         K > 1 ? (int)stream::hist_slot(raw_pos, K) : 0, (unsigned)(4 * (K - 1) * R)};
  const size_t blocks = (m + 15) / 16;
  hipLaunchKernelGGL(stream::k_fir_decimate, dim3((unsigned)((blocks + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, hist,
                     out, (int)n_raw, (int)R, (int)m, dc);
  return hip_err(hipGetLastError());
}

int mibminet_test_sos_filter(const float* x, size_t n, size_t R, const float* sos, size_t M, const float* state_in,
                             float* out, float* state_out, int device, void* stream) {
  if (R < 1 || R > 64 || n > stream::MAX_Q * stream::MAX_PUSH || !state_in || !state_out) return NET_ERR_INVALID;
  if (M < 1 || M > stream::MAX_SECTIONS || !sos || (n && (!x || !out))) return NET_ERR_INVALID;
  if (const int rc = check_device(device)) return rc;
  DeviceState& ds = g_devs[device];
  std::lock_guard<std::mutex> lk(ds.mu);
  DeviceGuard guard(device);
  if (guard.err != hipSuccess) return hip_err(guard.err);
  if (const int rc = ensure_cus(ds, device)) return rc;
  const hipStream_t st = (hipStream_t)stream;
  if (state_out != state_in)
    if (const int rc = hip_err(hipMemcpyAsync(state_out, state_in, 8 * M * R, hipMemcpyDeviceToDevice, st))) return rc;
  if (n == 0) return NET_OK;
  stream::Sos c{};
  std::memcpy(c.c, sos, 5 * sizeof(float) * M);
  return launch_prefilter<false>(ds, st, x, out, state_out, nullptr, 1, R, n, M, c);
}

}  // extern "C"
