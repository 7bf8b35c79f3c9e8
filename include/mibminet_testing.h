/*
 * mibminet_testing.h — test hooks of libmibminet (not part of the reference's interface).
 *
 * The library turns every C truncating division of the path, y = clip(trunc(v / fac)), into a
 * float multiply by a reciprocal r that it chooses and verifies on the host (DESIGN.md §3,
 * "Exact requantisation"), or, for parameter sets outside that envelope, into an exact integer
 * division by a magic multiplier.  These hooks expose both so the tests can check them against
 * exhaustive integer division.
 */
#ifndef MIBMINET_TESTING_H
#define MIBMINET_TESTING_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The reciprocal the library would use for factor `fac` when |v| <= vmax and outputs must be
 * exact up to step kmax (128 for int8 clipping).  magic != 0 also requires and returns
 * c = -1.5 * 2^23 * r exact (the layer-1/3 fma form).  Returns 0, or NET_ERR_RANGE when no
 * float reciprocal is exact over that range. */
int mibminet_test_reciprocal(int32_t fac, int64_t vmax, int32_t kmax, int32_t magic, float* r, float* c);

/* The floor-form constants of the plain-BN branches (layer2.c:139-210, layer4.c:113-130: every
 * element requantised, then the ReLU): for |x| <= vmax, e = clamp(floor(x / fac), 0, emax) is
 * computed as bits(fmed3(fma(f32 bits (mbits + x), r, c), K, K + emax)) - bits(K), K = 1.5 * 2^23.
 * Returns 0 with mbits (the magic the MFMA C-init adds to the offset), r and c, or NET_ERR_RANGE. */
int mibminet_test_floor_form(int32_t fac, int64_t emax, int64_t vmax, int32_t* mbits, float* r, float* c);

/* The float32 input quantiser of net_model_compute_batch_f32 (in-kernel, Markstein-corrected
 * quotient) on a flat device array: q[i] = quantize(x[i]) for i < n.  Enqueued on `stream`. */
int mibminet_test_quantize_f32(const float* x, int8_t* q, size_t n, float scale, int device, void* stream);

/* The multi-device driver of net_model_compute_batch_multi[_ct] run with recording stand-ins
 * instead of device work (no device needed): writes the order of its steps into `log` as
 * "P<device>" (parameter image made resident), "E<shard>" (shard enqueued) and "W<n>" (the first
 * n shards waited for), with the enqueue of shard `fail_at` failing (-1: none).  Returns what the
 * driver returns. */
int mibminet_test_multi_order(int ndev, const int* devices, int fail_at, char* log, size_t len);

/* Parameter-image uploads so far, and how many of them happened while the multi-device entry
 * points were enqueueing shards (0 when every device is prepared before the first enqueue). */
int mibminet_test_upload_stats(int64_t* uploads, int64_t* uploads_while_enqueueing);

/* Number of parameter-image copies resident on `device`. */
int mibminet_test_device_images(int device);

/* Exact-division builds (Cfg::XR, parameter sets outside the float requant envelope): the
 * integer division the kernels use at layers 1, 2 and 4 (forward_common.hpp, xdiv; constants from
 * requant_host.hpp, xdiv_consts).  _host: the device instruction sequence emulated on the host,
 * q[i] = xdiv(e[i], d) for i < n (no device needed).  _gpu: the device function itself over
 * e = e0 .. e0 + count - 1 against C division in 64 bits, on `device`; *mismatches = the number of
 * e where they differ.  d != 0 (NET_ERR_INVALID otherwise). */
int mibminet_test_xdiv_host(const int32_t* e, size_t n, int32_t d, int32_t* q);
int mibminet_test_xdiv_gpu(int32_t d, int64_t e0, int64_t count, int64_t* mismatches, int device);

/* The REORDER_BN pooling constants of layer 2 or 4 for offset `off`: the threshold as the kernels
 * use it (thr = -(off >> 3) clamped to the layer's conv range [-V, V], V = 2^20 / 2^18) and the
 * offset term, so that sum_8 max(v - thr_c, 0) + offm (mod 2^32) = sum_8 max(v, thr) + off for
 * every reachable v. */
int mibminet_test_pool_consts(int32_t off, int32_t layer, int32_t* thr, int32_t* offm);

/* 1 when the loaded parameter set runs the exact-division kernels, 0 when the float requant
 * kernels, NET_ERR_NO_PARAMS when none is loaded. */
int mibminet_test_params_xr(void);

/* on != 0: every parameter set loaded after this call runs the run-time-dimension kernels
 * (forward_gen.hpp), the compiled geometries included, so that both kernel families can be
 * checked against the oracle on the same set; 0 restores the normal choice. */
int mibminet_test_force_general(int on);

/* workgroups > 0: every persistent grid launched after this call (the compiled and the general
 * batched kernels, layer 1 over a recording, the window and the epoch loops) has at most that many
 * workgroups, and net_launch_info[_ct] reports it, so that a few items walk a workgroup through
 * its second and later passes at any geometry; 0 restores the normal choice (the occupancy's).
 * No kernel reads the cap: only the grid changes.  NET_ERR_INVALID for a negative argument, which
 * leaves the cap as it was. */
int mibminet_test_grid_cap(int workgroups);

/* FNV-1a digest of the loaded set's device parameter image (the bytes uploaded to every device):
 * equal digests mean the two loads produce the same kernels' inputs. */
int mibminet_test_image_digest(uint64_t* digest);

/* The bytes of one parameter image of the loaded set: which = 0 the batched kernels' image (what
 * mibminet_test_image_digest hashes), 1 the window and epoch kernels' image.  *bytes is always set:
 * the image's size, or 0 when there is none (NET_ERR_NO_PARAMS; NET_ERR_UNSUPPORTED for a set
 * without a window image).  buf == NULL only asks for the size; otherwise cap >= *bytes
 * (NET_ERR_INVALID if not) and the image is copied to buf. */
int mibminet_test_image_copy(int which, void* buf, size_t cap, size_t* bytes);

/* Number of constant filters the loaded set had folded (zero weights, offset +-y, factor +-1) to
 * stay on the float requant kernels: 0 unless the set as given needed exact division. */
int mibminet_test_folded_filters(int32_t* count);

/* Parameter banks (net_bank_create, include/mibminet.h).  _copy: the host image of slice `set` of
 * the bank, with mibminet_test_image_copy's conventions for buf, cap and *bytes (NET_ERR_INVALID
 * for a NULL bank or a set past the last): what each device receives for that set.
 * _device_copies: how many devices hold a copy of the bank (0 until the first call on it). */
typedef struct net_bank net_bank_t;
int mibminet_test_bank_copy(const net_bank_t* bank, size_t set, void* buf, size_t cap, size_t* bytes);
int mibminet_test_bank_device_copies(const net_bank_t* bank);

/* Live streams (net_streams_create, include/mibminet.h): the layer-1 ring of session i, its sixteen
 * rows of 2 * cap bytes (cap = net_streams_info's info[3]; filter f's output of sample t at bytes
 * t mod cap and t mod cap + cap of row f), copied to the HOST buffer out of 32 * cap bytes after the
 * group's device has been synchronised.  It tells a wrong ring from a wrong window.
 * NET_ERR_INVALID for a NULL group or buffer or a session past the last. */
typedef struct net_streams net_streams_t;
int mibminet_test_streams_ring(const net_streams_t* st, size_t i, void* out);

/* Places a fresh stream group at a position, so that its kernels can be run where a session is
 * after days: the group behaves from then on as one whose samples before the position were all
 * zero frames (net_streams_restart's definition of what a session does not remember).  pos: S HOST
 * entries, raw positions if the group has a decimator, else sample positions; origin: NULL or S
 * HOST entries, for a uniform group only.  Call it after net_streams_set_decimator[_each] and
 * net_streams_set_prefilter, which refuse a group that is no longer at 0, and before the first push
 * or restart.
 *   A uniform group: the entries of pos are all equal, P.  Its position becomes P, or with a
 * decimator its raw position P and its position D(P) = ceil(P / q); the windows returned so far
 * stay 0; every session's origin, on the host and on the device, becomes origin[s] if given, else
 * the new (decimated) position, so that with the default every window that starts before the seek
 * is a zero row counted in n_bad, exactly as after a restart.
 *   An each-group: the device's position of session s becomes pos[s], or with a decimator its raw
 * position pos[s] and its position D(pos[s]).  The count of pushes enqueued (net_streams_info) stays 0.
 *   Rings, histories and prefilter states stay as creation left them, all zero.  Synchronous: the
 * group's device is synchronised and the values are copied with plain copies; no kernel runs.
 * NET_ERR_INVALID, the group unchanged, for: a NULL group or pos; a group that has taken a push, a
 * restart or a seek; a negative entry; on an each-group an entry above INT64_MAX - 65,536 (with a
 * decimator: INT64_MAX - 2^20, the limits its plan keeps; a uniform group's bound is INT64_MAX
 * itself); entries of a uniform group that are not all equal; origin given for an each-group; an
 * origin outside 0 .. D(P) (D(P) = P without a decimator). */
int mibminet_test_streams_seek(net_streams_t* st, const int64_t* pos, const int64_t* origin);

/* The FIR decimator of net_streams_push_raw_f32_tm before its quantiser: the device function the
 * layer-1 kernel runs, on one session.  x: DEVICE [n_raw][R] float32, the chunk at raw position
 * raw_pos; hist: DEVICE [K - 1][R] float32, raw frame a < raw_pos at slot a mod (K - 1) (NULL for
 * K == 1); taps: DEVICE float32[K]; out: DEVICE [m][R] float32, m = net_streams_raw_samples(q,
 * raw_pos, n_raw), the decimated floats as they are.  Enqueued on `stream`.  A one-ulp error would
 * hide behind the int8 rounding without it.  NET_ERR_INVALID for R outside 1 .. 64, q outside
 * 1 .. 16, K outside 1 .. 128, n_raw > 16 * 65,536, a raw position that would pass INT64_MAX, a NULL
 * pointer that is needed. */
int mibminet_test_fir_decimate(const float* x, size_t n_raw, size_t R, const float* hist, const float* taps, size_t K,
                               size_t q, size_t raw_pos, float* out, int device, void* stream);

/* The prefilter of net_streams_set_prefilter before the FIR and the quantiser: the kernel a raw push
 * runs, on one session.  x: DEVICE [n][R] float32, the chunk in arrival order; sos: HOST float32[M][5]
 * = {b0, b1, b2, a1, a2}; state_in: DEVICE [M][2][R] float32 (z1 then z2 of a section), the state
 * before the chunk; out: DEVICE [n][R] float32, the filtered floats as they are; state_out: DEVICE
 * [M][2][R], the state after it (it may be state_in).  Enqueued on `stream`.  A one-ulp error would
 * hide behind the FIR and the int8 rounding without it.  n == 0 copies the state.  NET_ERR_INVALID
 * for R outside 1 .. 64, M outside 1 .. 8, n > 16 * 65,536, a NULL pointer that is needed. */
int mibminet_test_sos_filter(const float* x, size_t n, size_t R, const float* sos, size_t M, const float* state_in,
                             float* out, float* state_out, int device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
