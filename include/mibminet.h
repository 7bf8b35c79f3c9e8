/*
 * mibminet.h — C ABI of the MI355X-native int8 MI-BMInet (edgeEEGNet) inference path.
 *
 * Drop-in for the reference's model/layer call API (pulp-platform/MI-BMInet,
 * edge-eegnet_wolf/src/cl/net/model.h and layers.h): same symbols, same argument meaning and the
 * same single-trial buffer layouts, backed by hand-written CDNA4 (gfx950) HIP kernels.  Everything
 * the reference links in as generated C globals (src/cl/net/net.{h,c}) is loaded at run time from
 * a versioned parameter blob instead (net_params_load).
 *
 * Layout conventions (reference layouts, "_ALIGN" = rounded up to a multiple of 4):
 *   input       [T][C_ALIGN]   int8   (model.h:37 / model.c:81, gen_input_header.py:74-75)
 *   layer1 out  [F1][T_ALIGN]  int8   (layer1.c:116)
 *   layer2 out  [F2][T8_ALIGN] int8   (layer2.c:225)
 *   layer3 out  [F2][T8_ALIGN] int8   (layer3.c:95), [T8][F2] after net_layer3_flip_inplace
 *   layer4 out  [F2][T64_ALIGN] int8  (layer4.c:168)
 *   output      [N]            int8   (model.h:38)
 * Padding bytes of every produced buffer are written as zero.
 *
 * Batched layout (net_model_compute_batch): trial b starts at x + b * net_trial_stride(); each
 * trial is time-major [T][C] without channel padding, trial stride = C*T rounded up to 16 bytes.
 * Output is [B][N] int8.  Both pointers are DEVICE pointers on `device`.
 *
 * Errors: functions returning int return NET_OK (0) or a negative code; the reference's void
 * entry points keep their void signature and record the status for net_last_error().
 * Thread safety: every entry point may be called from any host thread; calls on one device are
 * serialised internally, different devices run concurrently.
 */
#ifndef MIBMINET_H
#define MIBMINET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIBMINET_VERSION 1

#define NET_OK 0
#define NET_ERR_INVALID (-1)     /* bad argument (null pointer, bad size, bad device) */
#define NET_ERR_NO_PARAMS (-2)   /* no parameter blob loaded */
#define NET_ERR_UNSUPPORTED (-3) /* network dimensions outside what the kernels take: F1 = F2 = 16, D = 1,
                                    C <= 64, 64 <= T <= 4096, N <= 16 */
#define NET_ERR_BLOB (-4)        /* malformed parameter blob */
#define NET_ERR_RANGE (-5)       /* parameters on which the reference's int32 arithmetic is undefined
                                    (overflow, zero divisor), or a float-input scale outside
                                    [2^-60, 2^60] (net_model_compute_batch_f32) */
#define NET_ERR_HIP (-100)       /* HIP runtime error: code = NET_ERR_HIP - hipError_t */

/* ---- reference entry points (host pointers, single trial) -------------------------------- */

/* edge-eegnet_wolf/src/cl/net/model.h:40 — whole forward pass of one trial.
 * p_data: [T][C_ALIGN] int8, p_output: [N] int8 (host memory). */
void net_model_compute(const int8_t* p_data, int8_t* p_output);

/* north_star name for the same entry, with a status return. */
int net_forward(const int8_t* p_data, int8_t* p_output);

/* edge-eegnet_wolf/src/cl/net/layers.h:46 (layer1.c:121): [T][C_ALIGN] -> [F1][T_ALIGN] */
void net_layer1(const int8_t* p_data, int8_t* p_result);
/* layers.h:74 (layer2.c:228): [F1][T_ALIGN] -> [F2][T8_ALIGN] */
void net_layer2(const int8_t* p_data, int8_t* p_result);
/* layers.h:97 (layer3.c:98): [F2][T8_ALIGN] -> [F2][T8_ALIGN] */
void net_layer3(const int8_t* p_data, int8_t* p_result);
/* layers.h:107 (layer3.c:243): [F2][T8_ALIGN] -> [T8][F2] in place */
void net_layer3_flip_inplace(int8_t* p_data);
/* layers.h:123 (layer4.c:172, FLIP_LAYERS): [T8][F2] -> [F2][T64_ALIGN] */
void net_layer4(const int8_t* p_data, int8_t* p_result);
/* layers.h:134 (layer5.c:43): [F2][T64_ALIGN] -> [N] */
void net_layer5(const int8_t* p_data, int8_t* p_result);

/* Status of the last void entry point called on this host thread. */
int net_last_error(void);

/* ---- parameters (replace the link-time globals of the generated net.h/net.c) ------------- */

/* Load a parameter blob (format: net_params_load_arrays below; mibminet/params.py, ParamSet.to_blob): the
 * net.h arrays net_l1_factor ... net_l5_weight with their dimensions, int8 or packed int4
 * weights, and the build variant (flag bit 0: -DREORDER_BN, the canonical build; clear: the plain
 * BN branches of layer2.c:139-210 / layer4.c:91-133.  Flag bit 1: clip every requantised output to
 * [-127, 127], the golden model's clip_balanced=True, functional.py:89-91; clear: [-128, 127] as
 * the C's __CLIP_R).  Other flag bits are rejected (NET_ERR_BLOB).  Validates, precomputes the gfx950 operand fragments and exact requantisation
 * constants, and uploads lazily to each device on first use.  Geometry: F1 = F2 = 16 and D = 1
 * (layer2.c:246), any C <= 64, 64 <= T <= 4096 and 1 <= N <= 16 (the channel-selected and 2- or
 * 3-class networks of QuantLab's loaders included); 22 x 1125, 64 x 1000 and 64 x 480 with N = 4
 * run kernels compiled for those shapes, every other geometry the run-time-dimension kernels
 * (net_params_info reports which).  Every set on which the reference's
 * own int32 arithmetic is defined for every int8 input loads: sets inside the float requant
 * envelope run the float-requant kernels, the others (e.g. large folded BN offsets) kernels that
 * divide exactly in integers.  NET_ERR_RANGE only where the reference's arithmetic is undefined:
 * a zero factor (or factor >> 3 in the plain branches), INT_MIN / -1, or an int32 overflow of
 * acc + offset (layer1.c:90-91), of the pooled sum or sum + offset (layer2.c:97-111,
 * layer4.c:99-130), or of the plain layer 4's sum of eight elements (layer4.c:113-130).  Replaces any previous set.  Pad
 * bytes of net_l1_weight_align (channels C..C_ALIGN-1) and of net_l5_weight (columns
 * T64..T64_ALIGN-1 of every row) must be zero, as gen_net_header.py writes them (NET_ERR_BLOB
 * otherwise).  Each distinct set gets its own device copy (about 144 KB per set and device), which
 * is never overwritten: launches already enqueued, and launches captured into a HIP graph, keep
 * running the set (and build variant) they were enqueued with, whatever is loaded later.  A load
 * never waits for the device.  When a device already holds 8 copies, the least recently used
 * copies whose launches have all completed are freed first (a copy is freed only once no launch
 * can still read it); if none is idle, the device keeps more than 8.  A copy used by a launch
 * under stream capture (which a HIP graph may replay at any time) is pinned until
 * net_params_unload, so captured graphs stay valid across any number of later loads.  A set
 * loaded again reuses its copy. */
int net_params_load(const void* blob, size_t len);

/* Which kernels the loaded set runs, for integrators who need to see a slower path coming:
 * info[0] = NET_PATH_FLOAT (compiled geometry, float requant proven exact on every reachable
 * value), NET_PATH_EXACT (compiled geometry, exact division at layers 1, 2 and 4: about
 * 1.1x the float kernels' time on 22 x 1125) or NET_PATH_GENERAL (run-time-dimension kernels,
 * float or exact requant as info[4] says); info[1] = the layer (1, 2 or 4) of the first requant that has no
 * proven float form (NET_PATH_EXACT), else 0; info[2] = its filter, else -1; info[3] = the
 * compiled geometry (0: 22 x 1125, 1: 64 x 1000, 2: 64 x 480), -1 on the general path; info[4] = 1
 * when the set divides exactly at layers 1-4 (NET_PATH_EXACT, or NET_PATH_GENERAL without a proven
 * float form for every requant), 0 when it runs the proven float requant.  info holds 5 entries.
 * A layer-1, -2 or -4 filter whose output is one constant over its whole reachable range (an
 * offset past the weights' reach, a factor that sends every sum to zero, a suppressed ReLU) is
 * folded into an equivalent constant filter before the choice, so such filters alone never force
 * exact division; info[1] / info[2] name a filter whose output varies. */
#define NET_PATH_FLOAT 0
#define NET_PATH_EXACT 1
#define NET_PATH_GENERAL 2
int net_params_info(int32_t* info);

/* Host only: the blob over R source rows, for input that carries every electrode of the cap.  The
 * output is the input blob with C := R and l1_weight_align as [F2][R_ALIGN]: column channels[c] of
 * the new array is column c of the old one, every other column is zero (int8 and packed int4
 * alike); every other field is byte-identical.  channels: HOST, the blob's C entries.  Layer 1 is a
 * dense contraction over its channel slots whatever C is, so for every int8 input u[R][T] the
 * widened set gives on u, at every layer, what the original gives on u[channels]: the same int32
 * accumulators, zeros adding nothing.  The reachable ranges are therefore the same: the widened
 * blob loads iff the original does, with the same code, and takes the same requant path
 * (net_params_info's info[4], exact division or not).  A compiled geometry (22 x 1125, 64 x 1000,
 * 64 x 480) becomes a general-path one once R != C; 64 -> 64 with a permutation stays compiled.
 * Sets of different C widened to one R agree on C for net_bank_create (T, N and the variant still
 * have to), so subjects with different electrode selections share one bank and one stream group;
 * net_bank_info then reports R as C.  Widen once at set-up, then feed the [n][R] frames to the
 * _f32_tm entries ("Frames as the amplifier delivers them").
 * out: HOST, cap bytes, not overlapping the blob; *out_len (if non-NULL) is set to the size the
 * output needs whenever the arguments pass; out == NULL asks for the size only.  Returns
 * NET_ERR_BLOB as net_params_load's parser returns it (first); then NET_ERR_INVALID for R outside
 * 1 .. 64, a NULL channels, an entry outside 0 .. R-1 or a duplicate entry (two columns would add,
 * and the sum may leave int8); then NET_ERR_INVALID for a cap too small, *out_len set.  Whether the
 * kernels take the set is net_params_load's business, here as for any blob. */
int net_blob_widen(const void* blob, size_t len, int R, const int32_t* channels, void* out, size_t cap,
                   size_t* out_len);

/* The reference's generated globals (edge-eegnet_wolf/data/gen_net_header.py:78-224, written by
 * python_utils/header_file.py as src/cl/net/net.{h,c}), by pointer, in their own layouts: a C host
 * that links the reference's net.c loads them with net_params_load_arrays and needs no blob file
 * and no Python.  include/mibminet_net_h.h fills this struct from the NET_* macros and net_l*
 * arrays of an included net.h (and the build variant from -DREORDER_BN, as the reference's
 * Makefile selects it).  Weights are int8, as net.c holds them. */
typedef struct {
    int32_t C, T, F1, F2, D, N;         /* NET_C, NET_T, NET_F1, NET_F2, NET_D, NET_N */
    uint32_t flags;                     /* NET_FLAG_REORDER_BN | NET_FLAG_CLIP_BALANCED (blob flag bits) */
    const int32_t* l1_factor;           /* net_l1_factor [F2] */
    const int32_t* l1_offset;           /* net_l1_offset [F2] */
    const int8_t* l1_weight_align;      /* net_l1_weight_align [F2][C_ALIGN], zero pad */
    const int32_t* l2_factor;           /* net_l2_factor [F2] (pool 8 folded in) */
    const int32_t* l2_offset;           /* net_l2_offset [F2] */
    const int8_t* l2_weight_reverse;    /* net_l2_weight_reverse [F2][64] (torch order) */
    int32_t l3_factor;                  /* NET_L3_FACTOR */
    const int8_t* l3_weight;            /* net_l3_weight [F2][16] (flipped) */
    const int32_t* l4_factor;           /* net_l4_factor [F2] */
    const int32_t* l4_offset;           /* net_l4_offset [F2] */
    const int8_t* l4_weight;            /* net_l4_weight [F2][F2] */
    int32_t l5_factor;                  /* NET_L5_FACTOR */
    const int8_t* l5_bias;              /* net_l5_bias [N] */
    const int8_t* l5_weight;            /* net_l5_weight [N][F2 * T64_ALIGN], zero pad per row */
} net_arrays_t;
#define NET_FLAG_REORDER_BN 1u
#define NET_FLAG_CLIP_BALANCED 2u

/* Loads the arrays of `a` exactly as net_params_load loads a blob holding them (same checks,
 * codes and device images; the arrays are copied, so they may go away after the call).  A blob
 * is the same fields serialised: a 64-byte header "MIBMINET", then uint32 version = 1, C, T, F1,
 * F2, D, N, weight_bits (8, or 4 for packed nibbles: element 2i in the low nibble of byte i),
 * l2_taps = 64, l3_taps = 16, flags, zero to byte 64; then l1_factor, l1_offset, l1_weight_align,
 * l2_factor, l2_offset, l2_weight_reverse, l3_factor, l3_weight, l4_factor, l4_offset, l4_weight,
 * l5_factor, l5_bias, l5_weight in that order, little endian, each section zero-padded to a
 * multiple of 4 bytes (mibminet/params.py, ParamSet.to_blob, writes it). */
int net_params_load_arrays(const net_arrays_t* a);

/* dims[0..6] = C, T, F1, F2, N, weight_bits, loaded(0/1). */
int net_params_dims(int32_t* dims);

/* Drops the loaded set and frees every device copy of every set, after synchronising each device
 * that holds copies (HIP graphs capturing launches must be dropped first: this is the one call
 * after which a captured launch may no longer be replayed). */
void net_params_unload(void);

/* ---- batched device entry points ---------------------------------------------------------- */

/* Bytes between consecutive trials of the batched input for the loaded network (0 if none). */
size_t net_trial_stride(void);

/* Forward B trials resident on `device`; x: device pointer [B][trial_stride], y: device pointer
 * [B][N].  x must be 16-byte aligned and y 4-byte aligned (NET_ERR_INVALID otherwise; hipMalloc
 * and torch allocations are).  Launches on the device's null stream and waits for completion.
 * TIME-MAJOR trials ([T][C] each, the reference's own single-trial orientation): a caller holding
 * channel-major [B][C][T] trials (SURVEY §8(b)'s layout, input.npz before gen_input_header.py:74
 * transposes it) must call net_model_compute_batch_ct_sync / net_model_compute_batch_ct instead;
 * the pointers carry no layout, and a [B][C][T] buffer passed here returns wrong logits. */
int net_model_compute_batch(const int8_t* x, int8_t* y, size_t B, int device);

/* SURVEY §8(b)'s batched signature, channel-major: x: DEVICE pointer to B trials [B][C][T] int8,
 * contiguous (trial stride C*T bytes, any alignment); y: DEVICE pointer [B][N], 4-byte aligned.
 * Launches on the device's null stream and waits for completion (net_model_compute_batch_ct is
 * the stream-ordered form). */
int net_model_compute_batch_ct_sync(const int8_t* x, int8_t* y, size_t B, int device);

/* Same, enqueued on `stream` (a hipStream_t of `device`, NULL = null stream), no host sync. */
int net_model_compute_batch_async(const int8_t* x, int8_t* y, size_t B, int device, void* stream);

/* Channel-major trials (SURVEY §8(b)'s batched signature; the layout of the reference's
 * input.npz before gen_input_header.py:74 transposes it): x: DEVICE pointer to B trials
 * [B][C][T] int8, contiguous (trial stride C*T bytes, any alignment); y: DEVICE pointer [B][N],
 * 4-byte aligned.  The same fused forward, with each layer-1 block transposed through LDS inside
 * the kernel (no separate pack pass).  Enqueued on `stream` (NULL = null stream), no host sync. */
int net_model_compute_batch_ct(const int8_t* x, int8_t* y, size_t B, int device, void* stream);

/* Float EEG straight into the forward: x: DEVICE pointer to B float32 trials [B][C][T] (the
 * reference's input.npz, 4-byte aligned), y: DEVICE pointer [B][N].  Each layer-1 block is
 * quantised in the kernel exactly as net_quantize_input_f32 does it (x / scale, clip to [-1, 1],
 * * 127, truncate, in float32; gen_input_header.py:66-76), then staged as in
 * net_model_compute_batch_ct: no int8 copy of the batch in memory.  scale = absMaxValue of quant1,
 * in [2^-60, 2^60] (NET_ERR_RANGE otherwise: the in-kernel quotient is exact there; use
 * net_quantize_input_f32 + net_model_compute_batch_async beyond).  Enqueued on `stream` (NULL =
 * null stream), no host sync. */
int net_model_compute_batch_f32(const float* x, int8_t* y, size_t B, float scale, int device, void* stream);

/* ---- continuous recordings: the logits of every sliding window ------------------------------
 * Window w of a recording of L samples covers samples w*hop .. w*hop + T - 1 (T of the loaded
 * network).  Layer 1 and the float input quantiser act on each sample alone, so they run once per
 * sample of the recording into a workspace, and each window's layers 2-5 read its 16 rows of T
 * bytes from there: no materialised [W][C][T] batch, no layer 1 per window (INTEGRATION.md,
 * "Continuous recordings"). */

/* Windows of the loaded network's T samples at hop `hop` in a recording of L samples:
 * L < T ? 0 : (L - T) / hop + 1   (0 if no set is loaded or hop == 0). */
size_t net_windows_count(size_t L, size_t hop);

/* Workspace layout: the layer-1 output of the whole recording, [F1 = 16][row_stride] int8 (row f
 * = filter f, byte t = sample t). */
size_t net_windows_row_stride(size_t L);      /* >= L, a multiple of 16 */
size_t net_windows_workspace(size_t L);       /* 16 * row_stride bytes */

/* layout: 0 = time-major recording [L][C] int8, 1 = channel-major [C][L] int8 (DEVICE pointers,
 * any byte alignment).  y: DEVICE [W][N] int8, 4-byte aligned, W = net_windows_count(L, hop); row
 * w is byte-identical to what net_model_compute_batch_ct returns for the trial x[:, w*hop :
 * w*hop + T].  ws: DEVICE, 16-byte aligned, ws_bytes >= net_windows_workspace(L); after the call
 * ws[f][t], t < L, is the reference net_layer1 output of sample t (bytes L .. row_stride - 1 of a
 * row are zero), and no window's result depends on a byte at t >= L.  Enqueued on
 * `stream` (NULL = null stream), no host sync, no allocation: capturable into a HIP graph after
 * one eager call has uploaded the parameters, like the batched entries.
 * Checks, all before any device call: NET_ERR_NO_PARAMS first; then NET_ERR_INVALID for hop == 0,
 * a layout other than 0 or 1, a null x, y or ws with W > 0, a misaligned y, a ws that is
 * misaligned or too small (for any W), W > INT32_MAX - 65,535, and
 * L * max(16, C * sizeof(element)) >= 2^31: the kernels address the recording and the workspace
 * through one buffer descriptor each, with 32-bit offsets.  Feed a longer recording in chunks that
 * overlap by T - hop samples (chunk k + 1 starts at the sample where chunk k's last window + hop
 * starts); the chunks' logit rows then concatenate to the recording's.  W == 0 returns NET_OK and
 * writes nothing. */
int net_model_compute_windows(const int8_t* x, int layout, size_t L, size_t hop, int8_t* y, void* ws,
                              size_t ws_bytes, int device, void* stream);

/* The same for a float32 channel-major recording [C][L] (4-byte aligned), quantised per sample
 * exactly as net_model_compute_batch_f32 / net_quantize_input_f32 do: scale in [2^-60, 2^60],
 * NET_ERR_RANGE otherwise (NET_ERR_INVALID for a scale that is not positive and finite). */
int net_model_compute_windows_f32(const float* x, size_t L, size_t hop, float scale, int8_t* y, void* ws,
                                  size_t ws_bytes, int device, void* stream);

/* The same for a float32 time-major recording [L][C] (sample-major frames, element (t, c) at float
 * index t*C + c; 4-byte aligned): the arguments, checks, check order, return codes and capture rules
 * of net_model_compute_windows_f32, only the shape of x differs.  This is the contract of every
 * _f32_tm entry below, each against its _f32 sibling: y, and where there is one the workspace or the
 * rings, are byte-identical to what the sibling writes for the transposed array, and therefore to
 * what the int8 time-major entry (layout 0) writes for net_quantize_input_f32's quantisation of the
 * same samples.  No transpose pass and no staging: a lane reads 64 contiguous bytes of one frame. */
int net_model_compute_windows_f32_tm(const float* x, size_t L, size_t hop, float scale, int8_t* y, void* ws,
                                     size_t ws_bytes, int device, void* stream);

/* ---- windows at given onsets: dense irregular windows, many recordings in one call -----------
 * The same two kernels with the window starts read from a device list: window i covers samples
 * onsets[i] .. onsets[i] + T - 1 of the recording and is valid iff 0 <= onsets[i] <= L - T.
 * Layer 1 still runs once per sample of the whole recording, so overlapping crops around markers,
 * irregular hops, and the sliding windows of several recordings laid end to end along time (no
 * window crossing a boundary: net_windows_multi_onsets) share it exactly as the regular windows
 * do: ws[f][t] does not depend on which recording sample t belongs to.  Prefer
 * net_model_compute_epochs for sparse onsets (W*T << L: layer 1 here covers all L samples) and
 * strided sources ("Windows at given onsets"); a channel subset of up to 64 source
 * rows is served here by a set widened over those rows (net_blob_widen).
 * x, layout, L, ws, ws_bytes, scale, device and stream are those of net_model_compute_windows
 * [_f32], and ws holds the same after the call.  onsets (W int64, 8-byte aligned, duplicates and
 * any order allowed), y ([W][N] int8, 4-byte aligned) and n_bad (one int32, 4-byte aligned, or
 * NULL; the caller zeroes it) are DEVICE pointers.  Logit row i of a valid onset is byte-identical
 * to what net_model_compute_batch_ct returns for the trial x[:, onsets[i] : onsets[i] + T] (the
 * float entry quantises first, as net_quantize_input_f32 does).  The kernel checks the onsets:
 * from an invalid one no address is formed, its row is written as N zeros, and *n_bad (if
 * non-NULL) is incremented once.  Two kernels are enqueued on `stream`, no host sync, no
 * allocation: capturable into a HIP graph after one eager call has uploaded the parameters.
 * Checks, all before any device call: NET_ERR_NO_PARAMS first; then NET_ERR_INVALID for a layout
 * other than 0 or 1, a null x, y, onsets or ws with W > 0, a misaligned y, n_bad, onsets or float
 * x, a ws that is misaligned or too small (for any W), W > 0 with L < T, W > INT32_MAX - 65,535,
 * L * max(16, C * sizeof(element)) >= 2^31 and a bad device; the float scale's domain as in
 * net_model_compute_windows_f32; NET_ERR_UNSUPPORTED for a network outside the general kernels'
 * family.  W == 0 returns NET_OK and touches nothing, the workspace included. */
int net_model_compute_windows_at(const int8_t* x, int layout, size_t L, const int64_t* onsets, size_t W,
                                 int8_t* y, int32_t* n_bad, void* ws, size_t ws_bytes, int device, void* stream);
int net_model_compute_windows_at_f32(const float* x, size_t L, const int64_t* onsets, size_t W, float scale,
                                     int8_t* y, int32_t* n_bad, void* ws, size_t ws_bytes, int device, void* stream);
/* net_model_compute_windows_at_f32 on a float32 time-major recording [L][C]
 * (net_model_compute_windows_f32_tm). */
int net_model_compute_windows_at_f32_tm(const float* x, size_t L, const int64_t* onsets, size_t W, float scale,
                                        int8_t* y, int32_t* n_bad, void* ws, size_t ws_bytes, int device, void* stream);

/* Host only: the onset list of the sliding windows of R recordings laid end to end along time.
 * Recording r has lengths[r] samples and starts at sample s_r = lengths[0] + .. + lengths[r - 1];
 * it contributes the onsets s_r + k*hop, k < net_windows_count(lengths[r], hop), in order (none
 * if it is shorter than T).  Both return the total W.  net_windows_multi_onsets fills onsets (a
 * HOST array) if it is non-NULL and cap >= W, and first (HOST, R + 1 entries) if it is non-NULL:
 * first[r] = the index of recording r's first window, first[R] = W.  Both return 0 and write
 * nothing when no set is loaded, hop == 0, or the lengths' sum overflows int64.  The list depends
 * on the geometry alone: copy it to the device once and reuse it. */
size_t net_windows_multi_count(const size_t* lengths, size_t R, size_t hop);
size_t net_windows_multi_onsets(const size_t* lengths, size_t R, size_t hop, int64_t* onsets, size_t cap,
                                size_t* first);

/* ---- epochs from a wider array: channel map, row stride and onsets --------------------------
 * The source x is a flat DEVICE array of n_elems elements; epoch e, network channel c, sample t is
 * element onsets[e] + channels[c]*row_stride + t.  One formula covers a recording [R][L] with cue
 * markers (row_stride = L, onsets = sample indices), a batch [B][R][Tf] cropped at t0 with a
 * channel subset (row_stride = Tf, onsets[b] = b*R*Tf + t0) and overlapping or irregular windows;
 * the kernel reads each epoch's rows where they lie, so no gathered [E][C][T] copy is written
 * ("Epochs from a wider array").  Duplicate and unsorted channels and onsets are
 * allowed.
 * x (int8, any byte alignment), onsets (E int64, 8-byte aligned), y ([E][N] int8, 4-byte aligned)
 * and n_bad (one int32, 4-byte aligned, or NULL) are DEVICE pointers; channels is a HOST array of
 * the loaded network's C entries, NULL = 0 .. C-1.  span = max(channels)*row_stride + T elements,
 * and an onset is valid iff 0 <= onset <= n_elems - span.  Logit row e of a valid onset is
 * byte-identical to what net_model_compute_batch_ct returns for the materialised [C][T] trial.
 * The onsets live on the device, so the kernel checks them: from an invalid onset no address is
 * formed, its logit row is written as N zeros, and *n_bad (if non-NULL; the caller zeroes it) is
 * incremented once per invalid onset.  Enqueued on `stream` (NULL = null stream), no host sync, no
 * allocation: capturable into a HIP graph after one eager call has uploaded the parameters.
 * Checks, all before any device call: NET_ERR_NO_PARAMS first; then NET_ERR_INVALID for a null x,
 * y or onsets with E > 0, a misaligned y, n_bad or onsets, row_stride == 0, a negative channel, a
 * span that overflows or exceeds n_elems, sizeof(element)*span + 6 >= 2^31 (each epoch is one
 * buffer view with 32-bit offsets; n_elems itself has no limit), E > INT32_MAX - 65,535 and a bad
 * device; NET_ERR_UNSUPPORTED for a network outside the general kernels' family.  E == 0 returns
 * NET_OK and touches nothing. */
int net_model_compute_epochs(const int8_t* x, size_t n_elems, size_t row_stride, const int32_t* channels,
                             const int64_t* onsets, size_t E, int8_t* y, int32_t* n_bad, int device, void* stream);

/* The same for a float32 source (4-byte aligned), quantised per sample exactly as
 * net_model_compute_batch_f32 / net_quantize_input_f32 do: scale in [2^-60, 2^60], NET_ERR_RANGE
 * otherwise (NET_ERR_INVALID for a scale that is not positive and finite). */
int net_model_compute_epochs_f32(const float* x, size_t n_elems, size_t row_stride, const int32_t* channels,
                                 const int64_t* onsets, size_t E, float scale, int8_t* y, int32_t* n_bad,
                                 int device, void* stream);

/* ---- parameter banks: many networks resident, one set index per epoch -------------------------
 * A bank is a collection of parameter sets of one geometry (per-subject, per-fold or per-repeat
 * models), resident on the device side by side; the epochs-bank entries classify epoch e with set
 * set_of[e], all in one launch ("Many networks in one call").  Its number of sets,
 * geometry, build variant and kernel form are fixed at creation; one set at a time may be replaced
 * in stream order (net_bank_replace).  A bank is
 * independent of the loaded set: creating, using and destroying one leaves the set net_params_load
 * installed, net_params_info and the devices' copies of loaded sets as they were, and the bank
 * entries need no loaded set. */
typedef struct net_bank net_bank_t;
#define NET_BANK_MAX_SETS 1024

/* blobs / sizes: HOST arrays of n_sets net_params_load blobs and their lengths; scales: NULL, or
 * n_sets input-quantiser scales (each network's own quant1 absMaxValue; the domain of
 * net_model_compute_epochs_f32's scale).  Every blob passes the checks of net_params_load and
 * becomes the parameter image that set has when loaded alone.  All sets must agree with set 0 on C,
 * T, N, the REORDER_BN flag and the clip: NET_ERR_UNSUPPORTED otherwise.  A malformed or refused
 * blob returns its own code (NET_ERR_BLOB, NET_ERR_RANGE, NET_ERR_UNSUPPORTED), a bad scale
 * NET_ERR_INVALID or NET_ERR_RANGE; *failed (if non-NULL) is then the index of the first such set.
 * If some sets need exact integer division (net_params_info) and others do not, every set of the
 * bank runs in the exact-division form: the same logits, and only that bank is slower
 * (net_bank_info reports it).  n_sets == 0 or > NET_BANK_MAX_SETS: NET_ERR_INVALID.  Host work only:
 * no device is touched; each device receives its copy on the first call that uses the bank there.
 * On success *bank is the new bank, otherwise NULL. */
int net_bank_create(const void* const* blobs, const size_t* sizes, const float* scales, size_t n_sets,
                    net_bank_t** bank, size_t* failed);

/* info[0..6] = n_sets, C, T, N, exact_division (0/1), has_scales (0/1), bytes per set on the device.
 * C is the sets' as loaded: for sets widened by net_blob_widen it is R, the source rows. */
int net_bank_info(const net_bank_t* bank, int32_t* info);

/* Synchronises every device that holds a copy of the bank, frees the copies and the bank.  NULL is
 * allowed.  Destroying a bank while a call on it is in flight in another thread, or replaying a HIP
 * graph that captured a call on it afterwards, is the caller's error. */
void net_bank_destroy(net_bank_t* bank);

/* A refitted network goes into service: set `set` of a resident bank becomes the network of `blob`
 * (a HOST net_params_load blob of `len` bytes), ordered on `stream`.  The calls on the bank enqueued
 * on `stream` before it read the old set, those enqueued on it after it the new one; every other set,
 * and every stream group on the bank, stays as it is ("Recalibrating a live
 * decoder").  Calls on OTHER streams that may run while the copy does must be ordered with it by the
 * caller (events): unordered, they may read a slot half written.
 * The blob goes through net_params_load's checks like a blob of net_bank_create and must agree with
 * what the bank was CREATED with on C, T, N, the REORDER_BN flag and the clip, not with whatever set
 * 0 is now: set 0 is replaceable like any other.  The new image is byte-identical to the one that
 * slot has in a bank freshly created with the new list of blobs (as long as that list still makes a
 * bank of the same kernel form).  Exact division: a bank that runs the exact-division form
 * (net_bank_info) takes a float set in that form.  A bank that runs the float form REFUSES a set
 * that needs exact division: promoting the resident sets would change the kernel under calls in
 * flight.  Remedy: if such sets may arrive, create the bank with one set that needs exact division.
 * scale: the set's input-quantiser scale, checked and installed iff the bank was created with
 * scales; ignored otherwise.
 * device: the device whose copy of the bank is updated.  If it holds one, the slot (the image and
 * the scale entry) is overwritten by copies enqueued on `stream` out of a pinned buffer the bank
 * keeps: the call may return before the device has the bytes, and the caller may free the blob and
 * replace the same slot again right away (the later call wins).  If no device holds a copy yet,
 * only the host master changes, `stream` is not looked at, and each device receives the new bank on
 * its first call as usual.  A bank with a copy on any device other than `device` is refused:
 * replacing across several devices is not part of this entry.
 * Checks, all before anything changes, in this order: NET_ERR_INVALID for a NULL bank,
 * set >= n_sets, a NULL blob or a device outside the library's range; the blob's own code
 * (NET_ERR_BLOB, NET_ERR_RANGE, NET_ERR_UNSUPPORTED); NET_ERR_UNSUPPORTED for a disagreement with
 * the bank's geometry or variant, and for the exact-division case above; NET_ERR_INVALID or
 * NET_ERR_RANGE for a bad scale (bank with scales); NET_ERR_UNSUPPORTED for a `stream` that is
 * capturing (host data is copied; asked where the device holds a copy); NET_ERR_UNSUPPORTED for a
 * copy on another device.  A refused call leaves the master, every copy and every result exactly as
 * they were.  A HIP error of a copy (NET_ERR_HIP and below) is no refusal: the device's slot may
 * then be partly written while the master is unchanged; replace the slot again or destroy the bank.
 * HIP graphs: a bank or stream call captured earlier reads the bank's copy when it REPLAYS, so after
 * a replacement it decodes under the new set without recapture.
 * Stream groups: a session's ring holds layer-1 outputs of the set that was there.  After replacing
 * a set, call net_streams_restart(st, i, set, stream) for every session i under it.  The exception
 * is a new set whose layer 1 is the old one's (a refitted head, or new layers 2-5): then nothing
 * need be done, and every later row, windows that began before the replacement included, is exact
 * under the new set.  Without a restart the rows are still defined: layers 2-5 of the new set over
 * the ring as it is.
 * Host threads: the call may run while other threads enqueue calls on the bank; two replacements of
 * one bank are serialised.  No allocation after the first replacement on a device whose earlier
 * copies have finished; no host sync.
 * Out of scope: promoting a resident float bank to the exact-division form, a bank resident on
 * several devices, growing a bank's set count. */
int net_bank_replace(net_bank_t* bank, size_t set, const void* blob, size_t len, float scale, int device,
                     void* stream);

/* Bytes of one item's layer-4 feature row, 16 * (T / 64): what the _feat entries below write per
 * item.  0 for a NULL bank. */
size_t net_bank_feature_bytes(const net_bank_t* bank);

/* net_model_compute_epochs with the network chosen per epoch: x, n_elems, row_stride, channels,
 * onsets, E, y, n_bad, device and stream are that entry's, with C and T the bank's, and so are the
 * checks and their order (a NULL bank, NET_ERR_INVALID, stands where NET_ERR_NO_PARAMS does).
 * set_of: DEVICE array of E int32 set indices, 4-byte aligned; NULL means set 0 for every epoch
 * and is allowed only for a bank of one set (NET_ERR_INVALID otherwise).  Logit row e is
 * byte-identical to what net_model_compute_epochs returns for that epoch with set set_of[e]
 * loaded.  An index outside 0 .. n_sets - 1 is treated exactly as an invalid onset: no parameter
 * address is formed from it, the row is N zeros and *n_bad is incremented, once per epoch even if
 * onset and index are both invalid.  Any order of set_of is correct; GROUPING THE EPOCHS BY SET IS
 * WHAT MAKES THE CALL FAST: each workgroup takes a contiguous range of epochs and reloads its
 * parameters whenever the set changes from one valid epoch to the next, so a grouped list costs one
 * reload per set and workgroup, a shuffled one nearly one per epoch.  The first call on a device
 * uploads the bank (one allocation, one host sync); after it the entry makes no allocation and no
 * host sync and is capturable into a HIP graph, like net_model_compute_epochs. */
int net_model_compute_epochs_bank(const net_bank_t* bank, const int8_t* x, size_t n_elems, size_t row_stride,
                                  const int32_t* channels, const int64_t* onsets, const int32_t* set_of, size_t E,
                                  int8_t* y, int32_t* n_bad, int device, void* stream);

/* The same for a float32 source (4-byte aligned).  No scale argument: epoch e is quantised with
 * the scale the bank was given for set set_of[e]; NET_ERR_INVALID for a bank created without
 * scales. */
int net_model_compute_epochs_bank_f32(const net_bank_t* bank, const float* x, size_t n_elems, size_t row_stride,
                                      const int32_t* channels, const int64_t* onsets, const int32_t* set_of, size_t E,
                                      int8_t* y, int32_t* n_bad, int device, void* stream);

/* The two entries above with the layer-4 activations beside the logits: what a head refit (layer 5
 * over 16 x T/64 features) reads, for calibration epochs where they lie (INTEGRATION.md,
 * "Recalibrating a live decoder").  feat: DEVICE [E][16][T64] int8, T64 = T / 64
 * (net_bank_feature_bytes per row), 16-BYTE ALIGNED.  Row e is the reference's net_layer4 output of
 * epoch e under set set_of[e] with the T64_ALIGN pad columns dropped: feat[e][k][v] =
 * layer4[k][v], v < T64, the bytes layer 5 multiplies.  An invalid epoch (onset or set index) gets
 * a zero feature row as it gets a zero logit row, and is counted once.  The logits are
 * byte-identical to the plain entry's, and everything else of its contract carries over: the
 * checks and their order, with NET_ERR_INVALID for a NULL feat with E > 0 or a feat that is not
 * 16-byte aligned standing beside y's check; one kernel, no allocation, no host sync, capturable.
 * Features from the other entries (batched, windows, pushes) are out of scope. */
int net_model_compute_epochs_bank_feat(const net_bank_t* bank, const int8_t* x, size_t n_elems, size_t row_stride,
                                       const int32_t* channels, const int64_t* onsets, const int32_t* set_of, size_t E,
                                       int8_t* y, int8_t* feat, int32_t* n_bad, int device, void* stream);
int net_model_compute_epochs_bank_feat_f32(const net_bank_t* bank, const float* x, size_t n_elems, size_t row_stride,
                                           const int32_t* channels, const int64_t* onsets, const int32_t* set_of,
                                           size_t E, int8_t* y, int8_t* feat, int32_t* n_bad, int device, void* stream);

/* ---- windows through a bank: many recordings, each with its own network ----------------------
 * The windows-at entries with the network chosen per recording.  R recordings lie along time in one
 * array x of L samples, in the layouts of net_model_compute_windows[_f32] (0 = [L][C] int8, 1 =
 * [C][L] int8; float32 [C][L]).  Recording r starts at starts[r], a multiple of 16 samples:
 * starts[0] = 0, starts[r+1] = starts[r] + lengths[r] rounded up to 16, and L = starts[R-1] +
 * lengths[R-1] (no rounding after the last recording); the pad samples between recordings may hold
 * anything.  blk_set (DEVICE, ceil(L/16) int32, 4-byte aligned) names the set of each 16-sample
 * block: samples 16b .. 16b+15 are processed by set blk_set[b].  C, T and N are the bank's; no
 * loaded set is needed, and the loaded set, net_params_info and the image cache are untouched.
 * Workspace: ws is the [16][net_windows_row_stride(L)] workspace of the windows entries.  For a
 * block with s = blk_set[b] in 0 .. n_sets-1, after the call ws[f][t] is the reference net_layer1
 * output of sample t under set s, for t in the block and t < L (the float entry quantises each
 * sample with set s's scale first, as net_quantize_input_f32 does).  For any other value of
 * blk_set[b] no parameter address is formed and the block's 16 bytes of all sixteen rows are zeros;
 * -1 is the documented "gap" value.  Bytes L .. row_stride-1 of each row are zero.
 * Windows: window i covers samples onsets[i] .. onsets[i]+T-1.  With s = blk_set[onsets[i] >> 4] it
 * is valid iff 0 <= onsets[i] <= L-T, s is in 0 .. n_sets-1, and blk_set[(onsets[i]+T-1) >> 4] == s
 * (the two blk_set reads happen only after the onset has passed its range check).  A valid window's
 * logit row is byte-identical to what net_model_compute_batch_ct returns for x[:, on : on+T] with
 * set s loaded (the float entry quantises with set s's scale first).  From an invalid window no
 * workspace or parameter address is formed, its row is N zeros and *n_bad (if non-NULL; the caller
 * zeroes it) is incremented once.  There is no per-window set argument: the window's set is read
 * from the list layer 1 ran by, so the two cannot disagree, and a window that starts in one
 * network's recording and ends in another's is counted as invalid, not answered.  A window that
 * crosses between two adjacent recordings of the same set is an ordinary window of the array, pad
 * samples included.  ONLY THE FIRST AND LAST BLOCK OF A WINDOW ARE CHECKED: a block of another set
 * (or a gap) strictly inside a window is the caller's error, and the result is then set s's layers
 * 2-5 over ws as it is.
 * onsets (W int64, 8-byte aligned), y ([W][N] int8, 4-byte aligned) and n_bad (one int32, 4-byte
 * aligned, or NULL) are DEVICE pointers, as in net_model_compute_windows_at.
 * Checks, all before any device call, in this order: a NULL bank, NET_ERR_INVALID (where
 * NET_ERR_NO_PARAMS stands in the windows-at entries); every argument check of
 * net_model_compute_windows_at[_f32] with the bank's C and T; blk_set NULL with W > 0, or misaligned
 * for any W, NET_ERR_INVALID; the float entry on a bank created without scales, NET_ERR_INVALID.
 * W == 0 returns NET_OK and touches nothing.  Two kernels are enqueued on `stream`.  The first call
 * on a device uploads the bank (one allocation, one host sync); after it the entry makes no
 * allocation and no host sync and is capturable into a HIP graph, like
 * net_model_compute_epochs_bank.  Each workgroup takes a contiguous range of windows and reloads
 * its parameters when the set changes, so list the windows recording by recording
 * (net_bank_windows_lists does). */
int net_model_compute_windows_bank(const net_bank_t* bank, const int8_t* x, int layout, size_t L,
                                   const int32_t* blk_set, const int64_t* onsets, size_t W, int8_t* y,
                                   int32_t* n_bad, void* ws, size_t ws_bytes, int device, void* stream);
int net_model_compute_windows_bank_f32(const net_bank_t* bank, const float* x, size_t L,
                                       const int32_t* blk_set, const int64_t* onsets, size_t W, int8_t* y,
                                       int32_t* n_bad, void* ws, size_t ws_bytes, int device, void* stream);
/* net_model_compute_windows_bank_f32 on a float32 time-major array [L][C]
 * (net_model_compute_windows_f32_tm): block b's samples are quantised with blk_set[b]'s scale. */
int net_model_compute_windows_bank_f32_tm(const net_bank_t* bank, const float* x, size_t L,
                                          const int32_t* blk_set, const int64_t* onsets, size_t W, int8_t* y,
                                          int32_t* n_bad, void* ws, size_t ws_bytes, int device, void* stream);

/* Host only: the layout above.  starts[0..R-1] (HOST, may be NULL); returns L, 0 on overflow of
 * int64 or R == 0. */
size_t net_bank_windows_starts(const size_t* lengths, size_t R, int64_t* starts);
/* Host only: the lists of the sliding windows of those recordings; sets[r] = the set of recording r.
 * Fills blk_set (HOST, if non-NULL and n_blk >= ceil(L/16)): every block from starts[r] >> 4 up to
 * the block before starts[r+1] >> 4 (for the last recording, up to ceil(L/16)) gets sets[r]; onsets
 * (HOST, if non-NULL and cap >= W) and first[0..R] (if non-NULL) as net_windows_multi_onsets does,
 * with the aligned starts: recording r contributes starts[r] + k*hop, k < the windows of
 * lengths[r] (none if it is shorter than T, though it still has its blocks).  Returns W.  0 and
 * nothing written for a NULL bank, hop == 0, overflow, or a set outside the bank. */
size_t net_bank_windows_lists(const net_bank_t* bank, const size_t* lengths, const int32_t* sets, size_t R,
                              size_t hop, int32_t* blk_set, size_t n_blk, int64_t* onsets, size_t cap, size_t* first);

/* ---- live streams: chunks pushed into a layer-1 ring, windows as they end --------------------
 * A stream group is S live sessions of one bank's geometry on one device.  Session i is decoded by
 * its own set of the bank, and all sessions advance by the same n samples per push.  The group owns
 * a device-resident ring of layer-1 outputs per session: a push runs layer 1 on the n new samples
 * only and returns the logits of exactly those windows of the global grid o = j*hop (j = 0, 1, ...)
 * whose last sample arrived in it.  Over any sequence of pushes the rows of session i, concatenated,
 * are byte-identical to what net_model_compute_windows_bank returns for the concatenation of its
 * chunks under its set ("Live streams").
 * The ring holds cap = net_streams_ring_samples(bank, max_push) = 16*ceil((T + max_push)/16)
 * samples per session, sample t at position t mod cap.  A push of n samples at position p0
 * overwrites the positions of samples p0-cap .. p0+n-1-cap, and the windows it completes reach back
 * to sample p0-T+1; that sample survives iff cap >= T+n-1, which holds for every n <= max_push.
 * ALL PUSHES AND RESTARTS OF ONE GROUP MUST BE ORDERED WITH RESPECT TO ONE ANOTHER (one HIP stream,
 * or events between streams), and none of them may run concurrently in two host threads: each reads
 * what the one before it wrote.  A push of such a group is not capturable into a HIP graph: the
 * position its arguments are computed from lives on the host.  Sessions that advance at their own
 * pace, and a push that is capturable, are an each-group's (net_streams_create_each, below). */
typedef struct net_streams net_streams_t;

/* Host only, no device, no group.  _ring_samples: cap as above; 0 for a NULL bank or max_push
 * outside 1 .. 65,536.  _push_windows: the windows per session that a push of n samples at position
 * pos returns, net_windows_count(pos + n, hop) - net_windows_count(pos, hop) for the bank's T; 0 for a
 * NULL bank, hop == 0, or when pos + n overflows. */
size_t net_streams_ring_samples(const net_bank_t* bank, size_t max_push);
size_t net_streams_push_windows(const net_bank_t* bank, size_t hop, size_t pos, size_t n);

/* sets: HOST array of S set indices, NULL = set 0 for every session.  Any hop >= 1 is allowed
 * (hop > T and hop > max_push included).  Checks, NET_ERR_INVALID before any device call: a NULL
 * bank or out, S == 0, hop == 0, max_push outside 1 .. 65,536, a sets[i] outside the bank,
 * S*max_push > INT32_MAX - 65,535, a bad device.  Then the bank is uploaded to `device` if it is not
 * there, and one allocation is made and zeroed: the rings (32*cap bytes per session) followed by
 * the sessions' origins (int64) and sets (int32).  The position is 0 and every origin 0.  The bank
 * must outlive the group.  The loaded set, net_params_info and the image cache are untouched. */
int net_streams_create(const net_bank_t* bank, const int32_t* sets, size_t S, size_t hop, size_t max_push,
                       int device, net_streams_t** out);

/* Synchronises the group's device, then frees the group.  NULL is allowed. */
void net_streams_destroy(net_streams_t* st);

/* info[0..5] = S, hop, max_push, cap, the position (samples pushed per session so far), the windows
 * returned per session so far. */
int net_streams_info(const net_streams_t* st, int64_t* info);

/* The host's record of session i: its origin (the position at its last restart, 0 before any) and
 * its set.  NET_ERR_INVALID for a NULL group or pointer or i >= S. */
int net_streams_origin(const net_streams_t* st, size_t i, int64_t* origin, int32_t* set);

/* One push: n new samples of every session.  x: DEVICE pointer to the S chunks, contiguous, any byte
 * alignment: layout 0 = [S][n][C] int8, 1 = [S][C][n] int8; the float entry [S][C][n] float32,
 * 4-byte aligned, session i quantised with the bank's scale of its set exactly as
 * net_quantize_input_f32 does.  With pos the position before the call and
 * k = net_streams_push_windows(bank, hop, pos, n), y is DEVICE [S][k][N] int8, 4-byte aligned: row
 * (i, j) is global window W0 + j, W0 = net_windows_count(pos, hop) for the bank's T, whose onset is
 * (W0 + j)*hop.  A window is answered iff its onset >= the session's origin; otherwise no ring or
 * parameter address is formed from it, its row is N zeros, and *n_bad (DEVICE, 4-byte aligned, or
 * NULL; the caller zeroes it) is incremented once.  An answered row is byte-identical to what
 * net_model_compute_batch_ct returns for that window of the session's samples with its set loaded.
 * k == 0 enqueues layer 1 only and writes nothing to y; otherwise two kernels go on `stream`.  No
 * host sync, no allocation.  The position advances on the host when the push is enqueued.
 * Checks, all before anything is enqueued and before the position moves: a NULL group,
 * NET_ERR_INVALID; n == 0, NET_OK and nothing done; then NET_ERR_INVALID for n > max_push, a layout
 * other than 0 or 1, a NULL x, a misaligned float x, the float entry on a bank without scales, a
 * position that would pass INT64_MAX, with k > 0 a NULL or misaligned y, a misaligned n_bad; then
 * NET_ERR_UNSUPPORTED for a `stream` that is capturing (a replay would not advance the position the
 * arguments were computed from).  A refused push leaves the group exactly as it was. */
int net_streams_push(net_streams_t* st, const int8_t* x, int layout, size_t n, int8_t* y, int32_t* n_bad,
                     void* stream);
int net_streams_push_f32(net_streams_t* st, const float* x, size_t n, int8_t* y, int32_t* n_bad, void* stream);
/* net_streams_push_f32 on [S][n][C] float32 chunks, frames as an amplifier delivers them
 * (net_model_compute_windows_f32_tm): the same rings and rows, no transpose before the push. */
int net_streams_push_f32_tm(net_streams_t* st, const float* x, size_t n, int8_t* y, int32_t* n_bad, void* stream);

/* A session that reconnects, or a new user who takes the slot: from the pushes enqueued after it,
 * session i is decoded by `set` and its origin is the current position.  Samples from before the
 * origin are never read by an answered window (they went through layer 1 under the old set).  The
 * window grid stays the global one, so the session's first answered window starts up to hop - 1
 * samples after its origin.  One one-thread kernel on `stream`, its two values passed by argument:
 * no host copy, no sync.  NET_ERR_INVALID for a NULL group, i >= S or a set outside the bank;
 * NET_ERR_UNSUPPORTED for a capturing stream. */
int net_streams_restart(net_streams_t* st, size_t i, int32_t set, void* stream);

/* ---- live streams: frames at q times the network's rate, FIR-decimated ---------------------------
 * A uniform group may be given a decimator: an integer factor q and K float32 FIR taps h.  It is then
 * pushed raw float32 frames [S][n_raw][C] (every electrode of the bank's geometry, as
 * net_streams_push_f32_tm takes them) at q times the rate the network runs at.  A raw push computes
 * the decimated samples the new frames complete inside the layer-1 kernel (no decimated float array
 * is written), quantises them with each session's set's scale, runs layer 1 on them into the rings
 * and returns the windows that end in them.  The last K-1 raw frames of every session live in device
 * memory owned by the group.
 * Arithmetic, bit for bit.  With raw_s[a] session s's raw frame a on the group's raw axis and
 * raw_s[a] = 0 for a < 0, decimated sample d, electrode r, is
 *     acc = +0.0f;  for k = 0 .. K-1, ascending:  acc = RN(acc + RN(h[k] * raw_s[q*d - k][r]))
 * with every product and every sum rounded to float32 on its own; nothing is contracted into an fma.
 * In exact arithmetic this is scipy.signal.upfirdn(h, x, 1, q); it does not depend on how the frames
 * are split into pushes.  What happens to SUBNORMAL intermediates follows the device's float mode and
 * is not part of the contract.  An unselected electrode of a widened set may carry anything, NaN
 * included: whatever the filter makes of it is quantised to a finite int8 and meets a zero weight.
 * Sample d exists once raw frame q*d has arrived: after P raw frames a session has D(P) = ceil(P/q)
 * samples, and a push of n_raw frames at P adds m = D(P+n_raw) - D(P) <= ceil(n_raw/q).  Those m
 * floats are quantised exactly as net_streams_push_f32_tm quantises a frame's, and from there on the
 * push IS net_streams_push_f32_tm of the m samples at position D(P): q = 1, K = 1, h = {1.0f} gives
 * that entry's rings and rows, and K = 1, h = {1.0f} with q > 1 is plain striding, x[::q].
 * The group's position, the origins, net_streams_info, net_streams_windows_at[_feat] and
 * net_streams_at_span all stay on the DECIMATED axis: a cue at raw frame a is the onset ceil(a/q).
 *
 * _set_decimator: once, before the group's first push.  taps: HOST float32[K].  One allocation (the
 * taps, then K-1 frames of C floats per session, zeroed), none afterwards; the call waits for
 * `stream`.  Checks: a NULL group, NET_ERR_INVALID; an each-group, NET_ERR_UNSUPPORTED; then
 * NET_ERR_INVALID for a group that has a decimator or has been pushed to, q outside 1 .. 16, K outside
 * 1 .. 128, NULL taps, a tap that is not finite, a bank without scales; then NET_ERR_UNSUPPORTED for a
 * capturing stream.  A refused call leaves the group unchanged.  A group with a decimator refuses
 * net_streams_push[_f32[_tm]] with NET_ERR_INVALID, and a group without one refuses the raw push the
 * same way.
 * _raw_samples: host only; m above, 0 for q == 0 or when raw_pos + n_raw overflows.
 * _push_raw_f32_tm: x is DEVICE [S][n_raw][C] float32, 4-byte aligned, n_raw <= q*max_push (hence
 * m <= max_push); y is DEVICE [S][k][N] with k = net_streams_push_windows(bank, hop, D(P), m), rows,
 * *n_bad and origins as net_streams_push defines them.  m == 0 is legal: only the history moves.
 * Layer 1 (m > 0), then for K > 1 a small kernel that copies the chunk's last min(n_raw, K-1) frames
 * to the histories, then the windows' kernel (k > 0) go on `stream`; no host sync, no allocation.
 * Checks, all before anything is enqueued and before a position moves: a NULL group, an each-group
 * or a group without a decimator, NET_ERR_INVALID; n_raw == 0, NET_OK and nothing done; then
 * NET_ERR_INVALID for n_raw > q*max_push, a NULL or misaligned x, a raw position that would pass
 * INT64_MAX, with k > 0 a NULL or misaligned y, a misaligned n_bad; then NET_ERR_UNSUPPORTED for a
 * capturing stream.  A refused push leaves the group exactly as it was.
 * _raw_info: info[0..3] = q (0: no decimator), K, the raw position P, the decimated position D(P).
 * net_streams_restart on such a group also zeroes session i's history, in stream order: from then on
 * the session is one whose frames before the restart were all zero.  Its decimated samples stay on
 * the group's axis q*d, and its origin is the decimated position. */
int net_streams_set_decimator(net_streams_t* st, size_t q, const float* taps, size_t K, void* stream);
size_t net_streams_raw_samples(size_t q, size_t raw_pos, size_t n_raw);
int net_streams_push_raw_f32_tm(net_streams_t* st, const float* x, size_t n_raw, int8_t* y, int32_t* n_bad,
                                void* stream);
int net_streams_raw_info(const net_streams_t* st, int64_t* info);

/* ---- live streams, each session at its own pace ------------------------------------------------
 * An each-group is a stream group whose sessions each have their own position pos[s], an int64 in
 * DEVICE memory: the samples session s was given since the group was created or the session last
 * restarted.  One push hands session s cnt_in[s] new samples, 0 <= cnt_in[s] <= n_max <= max_push
 * (0: the session skips the tick), and session s gets the windows of ITS OWN grid o = j*hop
 * (j = 0, 1, ..., counted in its own samples) whose last sample lies in pos[s] .. pos[s]+cnt_in[s]-1.
 * The contract is the uniform group's, per session: over any sequence of pushes the rows session s
 * received, concatenated, are byte-identical to what net_model_compute_windows_bank returns for the
 * concatenation of the chunks it was given since its origin, under its set.  The ring, cap and the
 * survival argument above are unchanged; pos[s] mod cap differs per session.
 * The counts are a device array and the positions live on the device, so a push reads nothing from
 * the host: the same enqueue is valid again and again, AND A PUSH IS CAPTURABLE INTO A HIP GRAPH
 * (below).  The ordering rule is the uniform group's: all pushes, restarts and position copies of
 * one group ordered with respect to one another, none concurrently in two host threads.
 *
 * _create_each: the arguments, checks, single allocation and opaque type of net_streams_create; the
 * allocation additionally holds, after the sets, one 16-byte plan record per session (at a multiple
 * of 16) and the positions (int64[S]), all zero.  An each-group refuses net_streams_push[_f32] with
 * NET_ERR_INVALID, and a uniform group refuses the entries below the same way.  net_streams_destroy
 * serves both kinds.  On an each-group net_streams_info returns S, hop, max_push, cap, THE PUSHES
 * ENQUEUED SO FAR and -1 (info[4] counts enqueues on the host, not the replays of a captured graph),
 * and net_streams_origin the host's record of the set and origin -1. */
int net_streams_create_each(const net_bank_t* bank, const int32_t* sets, size_t S, size_t hop, size_t max_push,
                            int device, net_streams_t** out);

/* Host only.  kmax = ceil(n_max / hop): the most windows any session can complete in a push of at
 * most n_max samples, the rows per session of y below.  0 for hop == 0 or n_max outside 1 .. 65,536. */
size_t net_streams_each_rows(size_t hop, size_t n_max);

/* One push.  x: DEVICE memory in fixed slots of n_max samples per session, so no address depends on
 * a count: layout 0 = [S][n_max][C] int8, the first cnt_in[s] samples of slot s used; 1 =
 * [S][C][n_max] int8, row stride n_max, the first cnt_in[s] samples of each row used; the float
 * entry [S][C][n_max] float32, 4-byte aligned, session s quantised with the bank's scale of its set.
 * Int8 x at any byte alignment.  The rest of a slot is read (it must be mapped) and ignored.
 * cnt_in: DEVICE int32[S], 4-byte aligned.
 * y: DEVICE [S][kmax][N] int8, 4-byte aligned, kmax = net_streams_each_rows(hop, n_max).  Rows
 * j < cnt_out[s] of session s are written: row j is window win0[s] + j of the session's grid, byte-
 * identical to what net_model_compute_batch_ct returns for that window of the session's samples
 * with its set loaded.  Rows j >= cnt_out[s] are not touched.
 * cnt_out: DEVICE int32[S], 4-byte aligned, required: the windows session s completed in this push.
 * win0: DEVICE int64[S], 8-byte aligned, or NULL: the index on the session's grid of its row 0 (the
 * onset is win0[s]*hop); written for every session, whatever its count.
 * A count outside 0 .. n_max is the caller's error and harmless: it is compared unsigned before any
 * address or loop bound is formed from it, the session stores nothing and its position does not
 * move, cnt_out[s] = -1 and *n_bad (DEVICE, 4-byte aligned, or NULL; the caller zeroes it) is
 * incremented once.  So is a count that would take the position past INT64_MAX - 65,536.
 * Three kernels go on `stream`: one thread per session plans the push (validates the count, writes
 * the session's record, cnt_out and win0, advances pos[s]), layer 1 of the new samples goes into the
 * rings, layers 2-5 run on the completed windows; the last two read only the records.  No host sync,
 * no allocation, no host-side state a replay would miss: THE ENTRY MAY BE CALLED ON A CAPTURING
 * STREAM after one eager call on the device (which may pass zeros and all counts 0; it uploads the
 * bank if create has not and asks the runtime for the kernels' occupancy).  A replay reads x and
 * cnt_in as they then are, writes y, cnt_out, win0 and n_bad again and advances the positions again.
 * Checks, all before anything is enqueued: a NULL group or a uniform group, NET_ERR_INVALID; then
 * NET_ERR_INVALID for n_max outside 1 .. max_push; a layout other than 0 or 1; a NULL x, cnt_in, y
 * or cnt_out; a misaligned y, cnt_in, cnt_out, win0, n_bad or float x; the float entry on a bank
 * without scales.  A refused push leaves the group as it was.  A HIP error of a launch (NET_ERR_HIP
 * and below) is no refusal: the three launches go out one after another, so if the second or third
 * fails the plan has already run and the positions have moved past samples whose layer 1 or windows
 * never ran.  Treat such a group as lost: destroy it, or restart every session. */
int net_streams_push_each(net_streams_t* st, const int8_t* x, int layout, const int32_t* cnt_in, size_t n_max,
                          int8_t* y, int32_t* cnt_out, int64_t* win0, int32_t* n_bad, void* stream);
int net_streams_push_each_f32(net_streams_t* st, const float* x, const int32_t* cnt_in, size_t n_max, int8_t* y,
                              int32_t* cnt_out, int64_t* win0, int32_t* n_bad, void* stream);
/* net_streams_push_each_f32 on [S][n_max][C] float32 fixed slots, the first cnt_in[s] frames of slot
 * s used (net_model_compute_windows_f32_tm).  Capturable into a HIP graph as its sibling is. */
int net_streams_push_each_f32_tm(net_streams_t* st, const float* x, const int32_t* cnt_in, size_t n_max, int8_t* y,
                                 int32_t* cnt_out, int64_t* win0, int32_t* n_bad, void* stream);

/* A stream-ordered copy of an each-group's positions to pos_out (DEVICE int64[S], 8-byte aligned).
 * NET_ERR_INVALID for a NULL group, a uniform group, a NULL or misaligned pos_out.
 *
 * net_streams_restart on an each-group: the same one-thread kernel sets pos[i] = 0 and the session's
 * set.  A window of the new run starts at o >= 0 of the new count and reads samples o .. o+T-1 <
 * pos[i], all written after the restart, so stale ring contents are never read and an each-group has
 * no unanswered window.  A capturing stream is refused, as for a uniform group. */
int net_streams_positions(net_streams_t* st, int64_t* pos_out, void* stream);

/* ---- live streams: raw frames at each session's own pace, FIR-decimated ---------------------------
 * An each-group may be given a decimator too (q, K taps h, as net_streams_set_decimator defines
 * them; one q and one filter for the whole group).  Every session then has, beside pos[s], its own
 * RAW position P[s] (int64, DEVICE memory: the raw frames it was given since creation or its last
 * restart), its own phase off = q*D(P[s]) - P[s] and its own history of K-1 raw frames, and a raw
 * push hands session s cnt_in[s] raw frames of its own.  All of it is planned on the device, so the
 * raw push reads nothing from the host and IS CAPTURABLE as net_streams_push_each is.
 * Per session the contract is the uniform raw push's: a push of cnt frames at P completes
 * m = D(P+cnt) - D(P) decimated samples, D(P) = ceil(P/q); sample d is the sum stated above (each
 * product and each sum rounded to float32 on its own, raw_s[a] = 0 for a < 0); the m floats are
 * quantised under the session's set's scale, and from there on the push IS
 * net_streams_push_each_f32_tm of m samples at position D(P[s]).  Over any sequence of pushes a
 * session's rows are byte-identical to net_model_compute_windows_bank on the quantised decimation
 * of the concatenation of its raw chunks.  pos[s] = D(P[s]) after every push, so
 * net_streams_positions and net_streams_windows_at[_feat] stay on the session's DECIMATED axis: a
 * cue at raw frame a of session s is the onset ceil(a/q).  m == 0 is legal and usual (one frame off
 * the grid): only the history and P[s] move.
 *
 * _set_decimator_each: each-groups only; a NULL or a uniform group is NET_ERR_INVALID.  Then the
 * checks of net_streams_set_decimator in its order: NET_ERR_INVALID for a group that has a decimator
 * or has been pushed to, q outside 1 .. 16, K outside 1 .. 128, NULL taps, a tap that is not finite,
 * a bank without scales; then NET_ERR_UNSUPPORTED for a capturing stream.  One allocation, zeroed,
 * none afterwards: the taps, the histories [S][K-1][C] float32, the raw positions int64[S] and one
 * 16-byte raw record per session.  The call waits for `stream`; a refused call leaves the group
 * unchanged.  (net_streams_set_decimator on an each-group stays NET_ERR_UNSUPPORTED.)  An each-group
 * with a decimator refuses net_streams_push_each[_f32[_tm]] with NET_ERR_INVALID, and one without
 * refuses the raw push the same way.  On such a group net_streams_raw_info returns q, K, -1, -1: the
 * positions are on the device.
 * _each_raw_rows: host only; net_streams_each_rows(hop, ceil(n_raw_max/q)), the rows per session of
 * y below.  0 for hop == 0, q outside 1 .. 16 or ceil(n_raw_max/q) outside 1 .. 65,536.
 * _push_each_raw_f32_tm: x is DEVICE [S][n_raw_max][C] float32 in fixed slots, 4-byte aligned,
 * 1 <= n_raw_max <= q*max_push; session s uses the first cnt_in[s] frames of its slot, 0 skips the
 * tick.  The rest of a slot must be mapped and never influences a stored byte, NaN included: an
 * answered sample d <= D(P+cnt) - 1 has q*d <= P + cnt - 1, so it reads no frame at or past cnt (the
 * kernel's view of a slot ends with its cnt-th frame).  y, cnt_out, win0, n_bad, their alignments and
 * their NULL rules are those of net_streams_push_each_f32_tm with
 * kmax = net_streams_each_raw_rows(hop, q, n_raw_max).  A count is compared unsigned before anything
 * is formed from it: one outside 0 .. n_raw_max, or one that would take P[s] past INT64_MAX - 2^20,
 * stores nothing, moves neither position nor the history, sets cnt_out[s] = -1 and counts once in
 * *n_bad.  Four kernels go on `stream`: the plan (one thread per session: both records, cnt_out,
 * win0, *n_bad, P[s] and pos[s]), layer 1 with the FIR, for K > 1 the history update (also when no
 * session completes a sample), the windows.  No host sync, no allocation: after one eager call the
 * same enqueue may be captured and replayed, on the one stream the caller passes.  Checks, all before
 * anything is enqueued: a NULL group, a uniform group or a group without a decimator,
 * NET_ERR_INVALID; then NET_ERR_INVALID for n_raw_max outside 1 .. q*max_push, then the checks of
 * net_streams_push_each_f32_tm in its order.  A HIP error of a launch is no refusal (see there).
 * _raw_positions: a stream-ordered copy of the raw positions to raw_pos_out (DEVICE int64[S], 8-byte
 * aligned).  NET_ERR_INVALID as net_streams_positions refuses, and for a group without a decimator.
 * net_streams_restart on such a group sets pos[i] = 0, P[i] = 0 and the set and zeroes session i's
 * history, in stream order: the session is a fresh one on its own axis.  A capturing stream is
 * refused.  Not offered: a q or taps per session, rational resampling. */
int net_streams_set_decimator_each(net_streams_t* st, size_t q, const float* taps, size_t K, void* stream);
size_t net_streams_each_raw_rows(size_t hop, size_t q, size_t n_raw_max);
int net_streams_push_each_raw_f32_tm(net_streams_t* st, const float* x, const int32_t* cnt_in, size_t n_raw_max,
                                     int8_t* y, int32_t* cnt_out, int64_t* win0, int32_t* n_bad, void* stream);
int net_streams_raw_positions(net_streams_t* st, int64_t* raw_pos_out, void* stream);

/* ---- live streams: an IIR prefilter (biquad cascade) ahead of the FIR decimator ---------------------
 * A group that has a decimator, uniform or each, and has not been pushed to may be given a prefilter:
 * M second-order sections, 1 <= M <= 8, sos[M][5] = {b0, b1, b2, a1, a2} float32, section j being
 * H(z) = (b0 + b1 z^-1 + b2 z^-2) / (1 + a1 z^-1 + a2 z^-2) with a0 = 1, scipy's sign convention.
 * Every raw frame then passes the cascade, per session and electrode, with state the group owns,
 * before the decimator sees it: a DC offset, electrode drift and mains hum need a low-order IIR
 * (a Butterworth high-pass and a notch), which no FIR of K <= 128 taps at the raw rate replaces.  For
 * IIR at the network's own rate use q = 1, K = 1, h = {1.0f}.
 * Arithmetic, bit for bit.  Per session s and electrode r, per raw frame in arrival order, sections
 * j = 0 .. M-1 ascending, transposed direct form II; with v the section's input (the raw sample for
 * j = 0, the previous section's w otherwise):
 *     w   = RN(RN(b0*v) + z1)
 *     z1' = RN(RN(RN(b1*v) - RN(a1*w)) + z2)
 *     z2' = RN(RN(b2*v) - RN(a2*w))
 * with every product and every sum or difference rounded to float32 on its own; nothing is contracted
 * into an fma.  All states start at +0.0f.  In exact arithmetic this is scipy.signal.sosfilt; it
 * does not depend on how the frames are split into pushes.  SUBNORMAL intermediates follow the
 * device's float mode and are outside the contract, as for the FIR.  From there on the push IS the
 * raw push of the filtered frames: the FIR, the histories (which then hold filtered frames), the
 * quantiser, the rings, the rows, n_bad and the positions are as net_streams_push_raw_f32_tm and
 * net_streams_push_each_raw_f32_tm define them.
 * Electrodes are independent.  A NaN or an infinity on an electrode enters that electrode's state
 * alone and stays there until the session restarts.  An unselected electrode of a widened set may
 * therefore still carry anything: its filtered value is quantised to a finite int8 and meets a zero
 * weight.  ON A SELECTED ELECTRODE A NON-FINITE SAMPLE NOW POISONS THE SESSION UNTIL ITS RESTART (the
 * FIR alone forgets it after K frames).  Stability of the filter is the caller's business and is not
 * checked.
 * _set_prefilter: one entry for both kinds of group.  sos: HOST float32[M][5].  One allocation, none
 * afterwards: the states [S][M][2][C] float32, zeroed, a session's contiguous, and the scratch
 * [S][q*max_push][C] float32 that holds the filtered frames of one push (5.8 MB for 1,024 sessions of
 * 22 electrodes at q = 4 and max_push = 16).  The coefficients travel in the kernel's arguments, so
 * they survive in a captured graph.  The call waits for `stream`.  Checks, in this order, all before
 * the allocation: a NULL group, NET_ERR_INVALID; then NET_ERR_INVALID for a group without a
 * decimator, a group that has a prefilter or has been pushed to, M outside 1 .. 8, NULL sos, a
 * coefficient that is not finite; then NET_ERR_UNSUPPORTED for a capturing stream.  A refused call
 * leaves the group unchanged.
 * A raw push of such a group enqueues one kernel more, ahead of layer 1 (an each-group: after the
 * plan, its trip counts from the plan's records, so a refused count moves no state, the rest of a
 * slot is never read, and the five launches stay capturable after one eager call); no host read is
 * added.  Without a prefilter a raw push enqueues exactly what it did.  Every CHECK of a raw push
 * still comes before anything is enqueued.  A HIP error of a launch (NET_ERR_HIP and below) is no
 * refusal, here as for an each-group's push: the prefilter goes out first, so if a later launch of
 * the same push fails, the states have moved past frames whose layer 1 never ran, on a uniform group
 * although its positions have not moved.  Treat such a group as lost: destroy it, or restart every
 * session.
 * net_streams_restart on such a group additionally zeroes session i's states in stream order: the
 * session is one whose earlier frames were all zero (zero state is the steady state of zero input).
 * _prefilter_info: info[0..2] = M (0: none), the scratch's frames per session, the bytes allocated.
 * NET_ERR_INVALID for a NULL group or info.
 * Not offered: coefficients per session or electrode, zero-phase filtering. */
int net_streams_set_prefilter(net_streams_t* st, const float* sos, size_t M, void* stream);
int net_streams_prefilter_info(const net_streams_t* st, int64_t* info);

/* ---- live streams: windows at given onsets, read from the rings ---------------------------------
 * The live counterpart of net_model_compute_windows_at, for cue-locked trials of a recording that is
 * still arriving ("Cue-locked trials").  One entry serves both kinds of group.
 * session: DEVICE int32[W], 4-byte aligned.  onsets: DEVICE int64[W], 8-byte aligned.  y: DEVICE
 * [W][N] int8, 4-byte aligned.  n_bad: DEVICE, 4-byte aligned, or NULL; the caller zeroes it.
 * Item w asks for the window of session session[w] whose first sample is onsets[w]: on a uniform
 * group on the group's position axis (the one net_streams_info's position and the origins live on),
 * on an each-group in the session's own count since its last restart.  Any order, duplicates
 * allowed; a workgroup reloads its parameters whenever neighbouring items change sets, so sort the
 * items by session where the order is free.
 * Validity.  With pos the session's position when the call runs (the host's position; pos[s] in
 * device memory for an each-group), item w is valid iff the session index, compared unsigned, is
 * below S; the session's set is inside the bank; o >= origin[s] (each-group: o >= 0); and
 * T <= pos - o <= cap: the window is complete and its first sample is still in the ring.  The
 * comparisons are made in 64 bits in a form that cannot overflow, so a value whose low 32 bits
 * alone would be valid fails.  From an invalid item no ring or parameter address is formed, its row
 * is N zeros and *n_bad is incremented once.  The row of a valid item is byte-identical to what
 * net_model_compute_batch_ct returns for samples o .. o+T-1 of the session with its set loaded.
 * Retention.  A window completes in the push that takes pos to o+T or beyond; right after that push
 * pos - o < T + n <= T + max_push <= cap, so a query enqueued after the push that completes a window
 * always finds it, and the window stays for cap - (pos - o) more samples.  A caller who wants more
 * slack creates the group with a larger max_push.
 * State.  The call reads the rings, the sets, the origins and the positions and writes y and *n_bad
 * alone: no position moves and nothing is stored into a ring.  It is ordered like a push: with
 * respect to the group's pushes and restarts.  One kernel goes on `stream`; no host sync, no
 * allocation.
 * Checks, all before anything is enqueued, in this order: a NULL group, NET_ERR_INVALID; W == 0,
 * NET_OK and nothing done; then NET_ERR_INVALID for W > INT32_MAX - 65,535, a NULL session, onsets or
 * y, a misaligned session, onsets, y or n_bad; then, on a uniform group, NET_ERR_UNSUPPORTED for a
 * `stream` that is capturing (the arguments are computed from the host's position).  On an
 * each-group the call reads nothing from the host: after one eager call on the device it may be
 * captured, as net_streams_push_each may, and a push plus a query replayed every tick read the
 * sessions and onsets as they then are. */
int net_streams_windows_at(net_streams_t* st, const int32_t* session, const int64_t* onsets, size_t W, int8_t* y,
                           int32_t* n_bad, void* stream);

/* net_streams_windows_at with the layer-4 activations beside the logits, for the cue-locked trials
 * of a live session that a recalibration refits on.  feat: DEVICE [W][16][T64] int8, 16-byte
 * aligned, row w as net_model_compute_epochs_bank_feat defines it for item w under its session's
 * set; an invalid item gets a zero feature row beside its zero logit row and is counted once.  The
 * logits are byte-identical to net_streams_windows_at's and the rest of its contract carries over
 * (state, ordering, one kernel, capturability on an each-group).  Checks: that entry's, with
 * NET_ERR_INVALID for a NULL or misaligned feat after y's and before the capturing stream's. */
int net_streams_windows_at_feat(net_streams_t* st, const int32_t* session, const int64_t* onsets, size_t W, int8_t* y,
                                int8_t* feat, int32_t* n_bad, void* stream);

/* Host only.  On a uniform group the onsets lo = max(pos - cap, 0) .. hi = pos - T have their window
 * in the ring now; hi < lo: none yet.  A session's own origin applies on top of the span.
 * NET_ERR_INVALID for a NULL group or pointer and for an each-group, whose positions are on the
 * device (net_streams_positions; a session's span is max(pos[s] - cap, 0) .. pos[s] - T). */
int net_streams_at_span(const net_streams_t* st, int64_t* lo, int64_t* hi);

/* Several devices from one host thread (static split, no collectives): shard i is
 * x[i] / y[i] / B[i] on devices[i] (DEVICE pointers of that device).  Every shard is enqueued
 * before any is waited for, so the devices run concurrently.  streams == NULL: each device's null
 * stream, and the call returns when all shards are done; otherwise streams[i] (a hipStream_t of
 * devices[i]) and no host sync.  Returns the first error; the shards enqueued before it have
 * finished by then (in both modes). */
int net_model_compute_batch_multi(int ndev, const int* devices, const int8_t* const* x, int8_t* const* y,
                                  const size_t* B, void* const* streams);

/* The same split over channel-major shards: x[i] is [B[i]][C][T] int8 on devices[i] (as
 * net_model_compute_batch_ct takes it). */
int net_model_compute_batch_multi_ct(int ndev, const int* devices, const int8_t* const* x, int8_t* const* y,
                                     const size_t* B, void* const* streams);

/* Input quantiser / transposer (the step before the path; reference
 * edge-eegnet_wolf/data/gen_input_header.py:66-76 with python_utils/functional.py:308-334):
 * x: DEVICE pointer to B float trials [B][C][T]; y: DEVICE pointer to the batched int8 layout
 * ([B][stride], stride = C*T rounded up to 16, each trial [T][C], pad bytes zero), computed as
 * trunc(clip(x / scale, -1, 1) * 127) in the input's precision.  scale = absMaxValue of the
 * network's quant1 activation.  Enqueued on `stream` (NULL = null stream), no host sync.
 * Any B up to INT32_MAX - 65,535 in one call (batches past 65,535 trials loop inside the kernel).  y must be
 * 16-byte aligned (as net_model_compute_batch requires of its input) and one trial's input must
 * stay below 2 GiB (C * T * sizeof(element) < 2^31); NET_ERR_INVALID otherwise. */
int net_quantize_input_f32(const float* x, int8_t* y, size_t B, int C, int T, float scale, int device,
                           void* stream);
int net_quantize_input_f64(const double* x, int8_t* y, size_t B, int C, int T, double scale, int device,
                           void* stream);

/* The step after the path: cls[b] = index of the largest of the N int8 logits of trial b, the
 * first one on ties (torch.max(pr_outs, dim=1) of the reference's accuracy meter,
 * QuantLab/quantlab/BCI-CompIV-2a/edgeEEGNet/postprocess.py:6-8).  logits: DEVICE pointer [B][N]
 * (as net_model_compute_batch writes it), cls: DEVICE pointer [B].  1 <= N <= 64,
 * B <= INT32_MAX - 1024 (NET_ERR_INVALID otherwise).  Enqueued on
 * `stream` (NULL = null stream), no host sync. */
int net_argmax_batch(const int8_t* logits, int32_t* cls, size_t B, int N, int device, void* stream);

/* Already-quantised int8 trials in channel-major [B][C][T] (the layout of the reference's
 * input.npz, transposed by gen_input_header.py:74 on the host): the same GPU transpose into the
 * batched [B][stride] layout, without the quantisation.  DEVICE pointers, B <= INT32_MAX - 65,535,
 * C <= 64, y 16-byte aligned, enqueued on `stream`, no host sync. */
int net_pack_trials_i8(const int8_t* x, int8_t* y, size_t B, int C, int T, int device, void* stream);

/* Device used by the single-trial API (default 0). */
int net_set_device(int device);

/* Kernel launch geometry used for a batch of B trials (for profiling/roofline bookkeeping):
 * out[0] = grid size (workgroups), out[1] = threads per workgroup, out[2] = LDS bytes. */
int net_launch_info(size_t B, int device, int32_t* out);
/* The same for the channel-major kernel (net_model_compute_batch_ct). */
int net_launch_info_ct(size_t B, int device, int32_t* out);

const char* net_error_string(int code);
int net_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MIBMINET_H */
