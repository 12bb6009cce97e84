/*
 * stofnet_amd.h -- C ABI of the MI355X-native StofNet inference hot path.
 *
 * One shared library (libstofnet_amd.so, gfx950 code objects embedded) replaces
 * the ATen calls that the reference's hot path makes (the reference has no native
 * code of its own).  Every entry point cites the reference
 * interface it stands in for (paths relative to hahnec/stofnet).
 *
 * Conventions
 *   - plain pointers and sizes only; device pointers are raw HIP device
 *     addresses, `stream` is a hipStream_t passed as void*.
 *   - ownership: the caller owns every buffer including workspaces; the library
 *     allocates nothing per call and keeps no data between calls (its only state is a
 *     per-device "LDS limit already raised" bit per kernel, set with atomics), so one host
 *     thread per GPU -- or several GPUs from one process -- may call concurrently.
 *   - all device work is enqueued asynchronously on `stream`; no hidden syncs.
 *   - every function returns a stof_status (0 = ok); nothing throws or aborts
 *     across the ABI.  stof_status_string() gives a static message.
 *   - activations are fp32, contiguous, NCL as in the reference.
 */
#ifndef STOFNET_AMD_H
#define STOFNET_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STOF_ABI_VERSION 3

typedef enum stof_status {
    STOF_OK = 0,
    STOF_ERR_BAD_ARG = 1,         /* null pointer, negative size, ...                          */
    STOF_ERR_ODD_SGB_REMAINDER = 2,/* L - 80*floor(L/80) is odd: the reference raises RuntimeError
                                      at models/stofnet.py:115                       */
    STOF_ERR_UNSUPPORTED = 3,     /* shape/mode outside what the kernels implement              */
    STOF_ERR_WORKSPACE = 4,       /* workspace or packed-weight buffer too small                */
    STOF_ERR_HIP = 5,             /* a HIP runtime call or launch failed                        */
    STOF_ERR_CHANNELS = 6,        /* channel count not divisible by r (view error in the reference,
                                      utils/sample_shuffle.py:24)                                */
    STOF_ERR_POOL_EMPTY = 7       /* SemiGlobalBlock on a row shorter than one pooling window (L < 80): the reference's
                                      MaxPool1d raises RuntimeError at models/stofnet.py:103       */
} stof_status;

const char* stof_status_string(int status);
int stof_abi_version(void);

/* ------------------------------------------------------------------------- *
 * Network description (models/stofnet.py:11 ctor arguments that the shipped
 * checkpoints use: num_features=64, num_blocks=13, kernel_sizes=[9,7,3],
 * in_channels=1).
 * ------------------------------------------------------------------------- */
typedef struct stof_net_desc {
    int32_t upsample_factor;     /* r: conv_last has r output channels (1..64)                  */
    int32_t semi_global_scale;   /* 80 = SemiGlobalBlock present, 1 = ablation without it       */
    int32_t precision;           /* STOF_PREC_*                                                 */
    int32_t seg_policy;           /* body sweep at small batches: 0 = automatic (waveforms are cut into 2^k segments
                                   * with +-38 rows of context while fewer than one per CU exists); k+1 forces 2^k   */
} stof_net_desc;

#define STOF_PREC_FP32 0          /* exact fp32 MFMA (v_mfma_f32_32x32x2_f32), parity baseline     */
#define STOF_PREC_F16X3 1         /* split-fp16 hi/lo operands, 3 MFMA passes, fp32 accumulate     */

/* Parameter order for stof_pack_weights(): the reference's state_dict tensors
 * (models/stofnet.py:23-31,88,94), each a host pointer to contiguous fp32:
 *   [0] conv1.weight (64,1,9)      [1] conv1.bias (64)
 *   [2+2i] conv{2+i}.weight (64,64,7), [3+2i] conv{2+i}.bias (64)   i = 0..10
 *   [24] conv_last.weight (r,64,3) [25] conv_last.bias (r)
 *   [26] semi_global_block.contract_conv.weight (512,64,5) [27] .bias (512)
 *   [28] semi_global_block.expand_conv.weight (64,512,5)   [29] .bias (64)
 * Entries 26..29 are ignored (may be NULL) when semi_global_scale == 1.      */
#define STOF_NUM_PARAMS 30

/* Bytes of the packed (kernel-layout) weight blob for `desc`. */
size_t stof_packed_weights_bytes(const stof_net_desc* desc);

/* One-time repack of the state_dict into the kernels' streaming layout.  Pure
 * host function (no GPU needed): writes `stof_packed_weights_bytes()` bytes to
 * `packed_host`; the caller uploads the blob to device memory once.
 * Replaces: nn.Module.load_state_dict + .to(device) (main.py:169,176-177).   */
int stof_pack_weights(const stof_net_desc* desc, const float* const* params,
                      void* packed_host, size_t packed_bytes);

/* Device workspace needed by stof_forward for a batch of N rows of length L. */
size_t stof_forward_workspace_bytes(const stof_net_desc* desc, int64_t N, int64_t L);

/* StofNet.forward (models/stofnet.py:42-67): x[N,1,L] -> y[N,1,L*r], both fp32
 * device buffers.  `packed_dev` is the uploaded blob from stof_pack_weights.
 * Returns STOF_ERR_ODD_SGB_REMAINDER for the lengths on which the reference's
 * SemiGlobalBlock raises (Q1).                                               */
int stof_forward(const stof_net_desc* desc, const void* packed_dev,
                 const float* x, float* y, int64_t N, int64_t L,
                 void* workspace, size_t workspace_bytes, void* stream);

/* Same as stof_forward, plus a range guard: bit 0 of *status_dev (a device int32 the caller has
 * zeroed) is set when the network produced a non-finite output.  In STOF_PREC_F16X3 that is what an
 * activation beyond the fp16 range (|a| > 65504; trained nets on max-abs-normalised inputs peak
 * near 50) turns into; the caller can then re-run in STOF_PREC_FP32.  No host sync.             */
int stof_forward_checked(const stof_net_desc* desc, const void* packed_dev,
                         const float* x, float* y, int64_t N, int64_t L,
                         void* workspace, size_t workspace_bytes, void* stream, int32_t* status_dev);

/* The default mode of the Python module (precision='auto'): STOF_PREC_F16X3 with the range guard of
 * stof_forward_checked, followed by an exact STOF_PREC_FP32 re-run of the same call whose kernels are gated ON THE
 * DEVICE by the guard word (they return at once while it is 0).  The result is the f16x3 map unless an activation left
 * the fp16 range, in which case it is the fp32 map -- no host sync either way.  `desc->precision` is ignored; the two
 * packed blobs come from stof_pack_weights with the respective precision.  *status_dev is zeroed by the call and reads
 * 1 afterwards iff the fp32 re-run happened.  `events` may be NULL or as in stof_forward_events (f16x3 pass only).   */
int stof_forward_auto(const stof_net_desc* desc, const void* packed_f16x3_dev, const void* packed_fp32_dev,
                      const float* x, float* y, int64_t N, int64_t L, void* workspace, size_t workspace_bytes,
                      void* stream, int32_t* status_dev, void* const* events);

/* StofNet.forward with get_maxima_positions in arg-max mode (utils/mask2samples.py:26-34, threshold = None) fused into
 * conv_last's epilogue (main.py:314 -> 320 for th = Null): per row the positions of the maximum of the NMS output, ties
 * and the constant-negative-row rule exactly as stof_pick_maxima reports them, WITHOUT the [N, 1, L*r] map going
 * through HBM -- `y` may be NULL (picker-only consumers: 4 bytes per onset instead of 4*L*r per waveform) or receive
 * the map as stof_forward would write it.  counts / idx / idx_cap as in stof_pick_maxima.  STOF_PREC_F16X3 and
 * upsample_factor <= 16 only (else STOF_ERR_UNSUPPORTED: use stof_forward + stof_pick_maxima); status_dev as in
 * stof_forward_checked (may be NULL).                                                                              */
size_t stof_forward_onsets_workspace_bytes(const stof_net_desc* desc, int64_t N, int64_t L);
int stof_forward_onsets(const stof_net_desc* desc, const void* packed_dev, const float* x, float* y, int64_t N,
                        int64_t L, int32_t window_size, int32_t* counts, int32_t* idx, int64_t idx_cap,
                        void* workspace, size_t workspace_bytes, void* stream, int32_t* status_dev);

/* Same as stof_forward, with instrumentation for bench.py: `events` is an array of
 * STOF_FORWARD_EVENTS hipEvent_t recorded on `stream` before the first kernel and after each
 * kernel of the first sub-batch (SemiGlobalBlock contract+pool, expand, body sweep), so the
 * caller can read per-kernel durations with stof_event_elapsed_ms after a sync.  `status_dev` may be NULL or
 * the range-guard word of stof_forward_checked.
 * Wraps nothing in the reference (its only timing is time.process_time(), main.py:313-315). */
#define STOF_FORWARD_EVENTS 4
int stof_forward_events(const stof_net_desc* desc, const void* packed_dev,
                        const float* x, float* y, int64_t N, int64_t L,
                        void* workspace, size_t workspace_bytes, void* stream, void* const* events,
                        int32_t* status_dev);
int stof_events_create(int32_t count, void** events_out);
int stof_events_destroy(int32_t count, void* const* events);
int stof_event_elapsed_ms(void* start, void* stop, float* ms_out);

/* SampleShuffle1D.forward (utils/sample_shuffle.py:10-28):
 * in[N, C_in, W] -> out[N, C_in/r, W*r], out[n,c,w*r+k] = in[n,k*C+c,w].     */
int stof_sample_shuffle(const float* in, float* out, int64_t N, int64_t C_in,
                        int64_t W, int32_t r, void* stream);
/* The same permutation for elements of elem_bytes = 1, 2, 4, 8 or 16 bytes, bit for bit: the reference's
 * view / permute / contiguous (utils/sample_shuffle.py:24-27) is dtype-agnostic (int64 ramps, float64, float16, complex).
 * Any r >= 1: an LDS-tiled kernel while its [r][257] tile fits in 64 KiB (r * 257 * elem_bytes), a plain gather kernel
 * beyond.  STOF_ERR_UNSUPPORTED only when the grid would exceed 2^31 - 1 work-groups. */
int stof_sample_shuffle_bytes(const void* in, void* out, int64_t N, int64_t C_in,
                              int64_t W, int32_t r, int32_t elem_bytes, void* stream);

/* get_maxima_positions (utils/mask2samples.py:26-34) per row of scores[N,1,M]:
 * NMS window `window_size` (made odd, :7), then threshold mode (has_threshold
 * != 0, the reference's `if threshold:`) or per-row arg-max mode.
 *   counts[N]       : detections per row (int32)
 *   idx[N, idx_cap] : time indices (int32, ascending) of the first idx_cap
 *                     detections of each row; unwritten tail is left untouched
 * The caller sizes idx_cap; a row with counts > idx_cap is truncated in `idx`
 * only (counts is exact), so the caller can re-run with a larger cap.        */
int stof_pick_maxima(const float* scores, int64_t N, int64_t M, int32_t window_size,
                     int32_t has_threshold, float threshold,
                     int32_t* counts, int32_t* idx, int64_t idx_cap, void* stream);

/* Second half of mask2coords (utils/mask2samples.py:92-112): scatter the first
 * kmax indices of each row into coords[N, kmax] (fp32, zero padded) and divide
 * by upsample_factor.                                                        */
int stof_indices_to_coords(const int32_t* counts, const int32_t* idx, int64_t idx_cap,
                           int64_t N, int64_t kmax, float upsample_factor,
                           float* coords, void* stream);

/* mask2coords with echo_max < kmax (utils/mask2samples.py:105-107,117-136): coords[N, echo_max] = the echo_max entries
 * of every row with the largest score amplitude (the reference's zero padding takes part with amplitude scores[row, 0]),
 * in ascending coordinate order, divided by upsample_factor.  counts / idx as written by stof_pick_maxima.            */
int stof_reduce_echoes(const float* scores, int64_t N, int64_t M, const int32_t* counts, const int32_t* idx,
                       int64_t idx_cap, int64_t kmax, int64_t echo_max, float upsample_factor, float* coords,
                       void* stream);

/* hilbert_transform (utils/hilbert.py:5-21) along the last dim of x[N, n]:
 * writes any of env[N,n] = |v|, re[N,n], im[N,n] that is non-NULL.           */
size_t stof_hilbert_workspace_bytes(int64_t N, int64_t n);
int stof_hilbert(const float* x, int64_t N, int64_t n, float* env, float* re, float* im,
                 void* workspace, size_t workspace_bytes, void* stream);
/* The same call for an output that nobody reads again soon (a result handed back to the framework): the envelope is
 * written with non-temporal stores and stays out of L2 / Infinity Cache ([4096,2000]: 23.9 -> 21.6 us).  A consumer that
 * follows immediately (GradPeak's row kernels) is better served by stof_hilbert, whose output it finds in the cache.  */
int stof_hilbert_streamed(const float* x, int64_t N, int64_t n, float* env, float* re, float* im,
                 void* workspace, size_t workspace_bytes, void* stream);

/* float64 rows: utils/hilbert.py:11 (torch.fft.fft) follows the input's dtype, so a float64 frame gives a complex128
 * analytic signal.  Same outputs in double; any n (mixed-radix plan over n's prime factors, O(n log n) for smooth n).
 * workspace: stof_hilbert_f64_workspace_bytes(N, n) bytes of device memory.                                       */
size_t stof_hilbert_f64_workspace_bytes(int64_t N, int64_t n);
int stof_hilbert_f64(const double* x, int64_t N, int64_t n, double* env, double* re, double* im,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * GradPeak (models/gradpeak.py).  Common arguments:
 *   grad_step, taps[2*radius+1], radius : gradient spacing g and the Gaussian taps for sigma = (2g-1)/6, prepared
 *                                         by the host exactly as models/gradpeak.py:71-76 does (fp64 -> fp32)
 *   ival_min, ival_max                  : hysteresis gate ival_min < peak - onset < ival_max (:20,:49)
 *   echoes[N, cap, 3], counts[N]        : (onset, peak, env[peak]) of the first `cap` echoes of each row, exact counts
 *   echo_max, reduced[N, echo_max, 3]   : echo_max > 0 also writes toa_detect's reduction (:107-114: echo_max largest
 *                                         amplitudes, then ascending time, the reference's zero padding taking part);
 *                                         the caller uses it iff flags[1] > echo_max; echo_max > 0 with cap > 4096
 *                                         returns STOF_ERR_UNSUPPORTED (the reduction ranks <= 4096 entries per row)
 *   flags[2] (zeroed by the call)       : flags[0] = 1 if some row has edges but no surviving candidate (Q9: the
 *                                         reference then returns an empty tensor for the batch), flags[1] = max(counts)
 * Nothing synchronises with the host; one read of `flags` after the call tells the caller what to slice.
 * ------------------------------------------------------------------------- */

/* Pre-pass of the default threshold (Q7, models/gradpeak.py:18): adds the sum and the sum of squares of the smoothed
 * gradient of env[N, L] to stats[0], stats[1] (double, zeroed by the caller; the caller puts N*L -- or the
 * all-reduced values of a sharded batch -- into stats[0..2] = (sum, sum of squares, count)).                        */
int stof_gradpeak_moments(const float* env, int64_t N, int64_t L, int32_t grad_step, const float* taps,
                          int32_t radius, double* stats, void* stream);
/* The same pre-pass that also keeps what it computed: blurred[N, stof_gradpeak_blurred_stride(L, radius)] receives the
 * smoothed gradient of every row (in the kernels' streaming order, zero outside the row), so that the detection after
 * the threshold is known does not redo gradient and blur (stof_grad_peak_detect_blurred).                            */
int64_t stof_gradpeak_blurred_stride(int64_t L, int32_t radius);
int stof_gradpeak_moments_store(const float* env, int64_t N, int64_t L, int32_t grad_step, const float* taps,
                                int32_t radius, double* stats, float* blurred, void* stream);
/* thres_pos = std**16 * 1.2e13 (:18) from stats[3] = (sum, sum of squares, count) into threshold_out[0], on the device. */
int stof_gradpeak_threshold(const double* stats, float* threshold_out, void* stream);

/* grad_peak_detect (models/gradpeak.py:8-68) on an envelope env[N, L]: gradient -> Gaussian blur -> threshold
 * crossings -> hysteresis pairing in one launch (one wavefront per row).  The positive threshold is `threshold`, or
 * *threshold_dev when that device pointer is non-NULL (the default threshold from stof_gradpeak_threshold).        */
int stof_grad_peak_detect(const float* env, int64_t N, int64_t L, int32_t grad_step, const float* taps,
                          int32_t radius, float threshold, const float* threshold_dev, int32_t ival_min,
                          int32_t ival_max, int64_t echo_max, float* echoes, int64_t cap, float* reduced,
                          int32_t* counts, int32_t* flags, void* stream);

/* grad_peak_detect from the smoothed gradient kept by stof_gradpeak_moments_store: threshold crossings and pairing only
 * (env supplies the amplitudes of the kept peaks).  Same outputs as stof_grad_peak_detect.                            */
int stof_grad_peak_detect_blurred(const float* env, const float* blurred, int64_t N, int64_t L, int32_t radius,
                                  float threshold, const float* threshold_dev, int32_t ival_min, int32_t ival_max,
                                  int64_t echo_max, float* echoes, int64_t cap, float* reduced, int32_t* counts,
                                  int32_t* flags, void* stream);

/* toa_detect (models/gradpeak.py:99-116) with an explicit threshold in ONE launch on waveforms frame[N, L]:
 * Hilbert envelope (utils/hilbert.py:5-21) -> grad_peak_detect -> echo_max reduction; the envelope stays in LDS
 * (env_out, optional [N, L], receives a copy).  Available when stof_toa_detect_fused_ok(L, radius) != 0 (even L with
 * prime factors 2, 3, 5, a pair of rows within the LDS budget); otherwise STOF_ERR_UNSUPPORTED and the caller chains
 * stof_hilbert + stof_grad_peak_detect.                                                                              */
int stof_toa_detect_fused_ok(int64_t L, int32_t radius);
int stof_toa_detect(const float* frame, int64_t N, int64_t L, int32_t grad_step, const float* taps, int32_t radius,
                    float threshold, int32_t ival_min, int32_t ival_max, int64_t echo_max, float* echoes,
                    int64_t cap, float* reduced, int32_t* counts, int32_t* flags, float* env_out, void* stream);

/* Pre-pass of the default threshold (Q7, models/gradpeak.py:18) on WAVEFORMS frame[N, L], for row lengths the fused
 * kernel takes (stof_toa_detect_fused_ok): Hilbert envelope -> gradient -> blur in LDS as in stof_toa_detect; the
 * envelope goes to env_out[N, L] (required: the detection launch after the threshold, stof_grad_peak_detect, reads it)
 * and the sum / sum of squares of the smoothed gradient are added to stats[0], stats[1] as stof_gradpeak_moments does.
 * partials: device scratch of STOF_MOMENT_SLOTS * 16 doubles (zeroed here; the work-groups' sums are spread over that
 * many cache lines and folded into stats at the end of the call, on the stream).                                      */
#define STOF_MOMENT_SLOTS 64
int stof_toa_moments(const float* frame, int64_t N, int64_t L, int32_t grad_step, const float* taps, int32_t radius,
                     float* env_out, double* partials, double* stats, void* stream);

/* GradPeak on float64 envelopes env[N, L] (the envelope of a float64 frame, stof_hilbert_f64): the reference keeps a
 * float64 input in double at every stage, so these take double taps (models/gradpeak.py:71-76 without the fp32 cast),
 * a double threshold, and write double echoes / reduced rows; the other arguments and the outputs are those of the fp32
 * entries above.  Rows need L >= 2 (torch.gradient), else STOF_ERR_UNSUPPORTED.
 * Pre-pass of the default threshold: adds the sum and the sum of squares of the smoothed gradient to stats[0], stats[1]
 * (the caller's triple, as for stof_gradpeak_moments) in a fixed order -- the same inputs give the same bits.
 * workspace: stof_gradpeak_moments_f64_workspace_bytes(N) bytes of device memory (one slot per work-group).          */
size_t stof_gradpeak_moments_f64_workspace_bytes(int64_t N);
int stof_gradpeak_moments_f64(const double* env, int64_t N, int64_t L, int32_t grad_step, const double* taps,
                              int32_t radius, double* stats, void* workspace, size_t workspace_bytes, void* stream);
/* thres_pos = std**16 * 1.2e13 (:18) in double from stats[3] = (sum, sum of squares, count) into threshold_out[0].     */
int stof_gradpeak_threshold_f64(const double* stats, double* threshold_out, void* stream);
/* grad_peak_detect in double: comparisons (> threshold, < -threshold/4) and amplitudes in float64; the positive
 * threshold is `threshold`, or *threshold_dev when that device pointer is non-NULL (stof_gradpeak_threshold_f64).      */
int stof_grad_peak_detect_f64(const double* env, int64_t N, int64_t L, int32_t grad_step, const double* taps,
                              int32_t radius, double threshold, const double* threshold_dev, int32_t ival_min,
                              int32_t ival_max, int64_t echo_max, double* echoes, int64_t cap, double* reduced,
                              int32_t* counts, int32_t* flags, void* stream);

/* ------------------------------------------------------------------------- *
 * Neighbours of the hot path (SURVEY.md section 8f "next rows").
 * ------------------------------------------------------------------------- */

/* ChirpDataset.iq2rf (datasets/chirp_dataset.py:80-91) + NormalizeVol
 * (utils/transforms.py:13): iq[N, len, 2] (re, im) fp32 -> rf[N, int(len*rescale_factor)] fp32:
 * linear resampling on endpoint-inclusive grids, Re{y * exp(2 pi i fc t)}, then (normalize != 0)
 * division by the per-waveform max |.|.                                         */
int stof_iq2rf(const float* iq, float* rf, int64_t N, int64_t len, double rescale_factor,
               double fc, double fs, int32_t normalize, void* stream);

/* Training augmentation (utils/transforms.py: NormalizeVol -> CropChannelData -> AddNoise, chained per sample at
 * main.py:49,54,82) for a batch of rows in one launch.  Per row, in this order:
 *   normalize   x / max|x| over the whole row.
 *   crop        when 0 < crop_ratio < 1 (else the row passes through, start = 0, gt_out = gt):
 *                 width = rint(L * crop_ratio), ref = rint(gt[row, 0]) (half to even; a NaN gt counts as 0),
 *                 start = max(0, ref - width/2), end = min(ref + width/2, L); end == L -> start = end - width;
 *                 start == 0 -> end = width; max_dist = min(ref - start, end - ref);
 *                 shift uniform on the integers [-min(start, max_dist/2), min(L - end, max_dist/2)) (floor divisions),
 *                 0 where that range is empty (the reference's randint raises there);
 *                 y[j] = x[start + shift + j] for j < width, 0 beyond; gt_out[row, 0] = gt[row, 0] - (start + shift);
 *                 columns c >= 1 move alike and become 0 (the "no echo" value of main.py:217) when they were <= 0 or NaN
 *                 or land outside [0, width); start[row] = start + shift.
 *   noise       U[j] uniform on [0, 1) for all L samples of the padded row; n = 2 (U - 0.5) when the cropped row has a
 *               negative sample, else U; y += n * sqrt(10^(-snr_db/10) * sum y^2 / sum n^2).  The sums are double
 *               accumulators combined in a fixed tree: bitwise the same from run to run.
 * Generator: Philox4x32-10, key = (seed & 0xffffffff, seed >> 32), counter = (j >> 2, row, call, (rank << 1) | stream_id);
 * word j & 3 gives U = (word >> 8) * 2^-24.  Stream 0 is the noise.  Stream 1 is the crop shift: with w = word 0 of block 0,
 * shift = low + (((w >> 8) * (high - low)) >> 24) on [low, high).  A draw depends on its coordinates only.
 * Overrides: noise[N, L] (uniforms used instead of stream 0) and shift[N] (used instead of the drawn shift; start + shift
 * is clamped into [0, L - width]); either may be NULL.
 * x[N, L], gt[N, G] (NULL with G = 0; a crop needs G >= 1) -> y[N, L] (y != x), gt_out[N, G], start[N].  One launch on
 * `stream`.  NULL x / y / start / desc, negative sizes, y == x, a missing gt, rank >= 2^31 or (add_noise) a non-finite
 * snr_db -> STOF_ERR_BAD_ARG; an odd crop width (the reference asserts on it) or N, L >= 2^31 -> STOF_ERR_UNSUPPORTED;
 * N == 0 or L == 0 -> STOF_OK without a launch.                                                                       */
typedef struct stof_augment_desc {
    uint64_t seed;
    double crop_ratio;           /* crop when 0 < crop_ratio < 1                                     */
    double snr_db;               /* read when add_noise != 0                                         */
    int32_t normalize;
    int32_t add_noise;
    uint32_t rank;               /* < 2^31                                                           */
    uint32_t call;               /* one value per training step                                      */
} stof_augment_desc;
int stof_augment(const stof_augment_desc* desc, const float* x, const float* gt, int64_t N, int64_t L, int64_t G,
                 const float* noise, const int32_t* shift, float* y, float* gt_out, int32_t* start, void* stream);
/* out[N, L] = the uniforms stream `stream_id` (0 or 1) of the generator above hands out for (seed, rank, call). */
int stof_augment_uniforms(uint64_t seed, uint32_t rank, uint32_t call, int32_t stream_id, float* out, int64_t N, int64_t L,
                          void* stream);

/* ------------------------------------------------------------------------- *
 * Plane-wave delay-and-sum beamformer (utils/beamform.py: bf_das, bf_das_rx) for a batch of frames.
 *
 * sig[F][A][S][Ne] (frames, transmit angles, samples, elements; element fastest) in one of four dtypes; complex values
 * are interleaved (re, im).  Pixels are a LIST of P points (x[p], z[p]) in any order.  Per frame f, angle a, pixel p and
 * element k, all in double:
 *     drx = hypot(x - xe[k], z),  tau = (dtx[a][p] + drx) / c,  i = (tau - t0) * fs,  fl = floor(i)
 *     the term counts iff |x - xe[k]| < z / fnumber / 2 (strict) and 1 <= i <= S - 1 (NaN and +-inf fail both):
 *     term = sig[f][a][fl][k] * (fl + 1 - i) + sig[f][a][fl + 1][k] * (i - fl)
 *     (at i == S - 1 the second weight is 0 and row S is not read: no input value leads to a read outside sig);
 *     complex dtypes with rotate[f][a][k] != 0: term *= exp(2 pi i f0 tau), f0 tau reduced to [0, 1) cycles in double.
 * The terms of one (f, a, p) are added in accumulators of sig's scalar type starting at 0, in a fixed order: the host entry
 * for k ascending; the kernel as eight partial sums (k = g mod 8, ascending) combined pairwise (g ^ 1, g ^ 2, g ^ 4).
 * compound != 0: out[f][p] = the angle sums added for a ascending; compound == 0: out[f][a][p] = the angle sum.  No atomics:
 * a frame's result is bitwise independent of F and of its place in the batch.
 * rotate[F][A][Ne] (bytes; read for complex dtypes only): the reference rotates a channel iff any value it gathered from
 * it is not purely real; callers set the byte iff column sig[f][a][:, k] has a non-zero imaginary part anywhere.
 *
 * dtx[A][P] comes from stof_das_tx_distance (host, libm): W = xe[Ne - 1] - xe[0], beta = 1e-8,
 *     v = (-W cos(t) sin(t) / beta, -W cos(t)^2 / beta),  g = |v0| - W/2 if |v0| > W/2 else 0,
 *     dtx = hypot(x - v0, z - v1) - hypot(g, v1)
 * -- a difference of two numbers near 1e6 m, so every consumer has to read the same doubles.
 *
 * stof_das_beamform_host: the same arithmetic (one shared header) in plain loops on host pointers; no GPU needed.
 * stof_das_beamform: sig, x, z, dtx, xe, rotate, out are device pointers; one launch on `stream`.
 * stof_das_bmode: img[F][n] of `dtype` -> bmode[F][n] of its real type (float for F32 / C64, else double):
 *     20 log10 |img|; pixels whose value is not finite (magnitude 0, NaN or inf) take the smallest finite value of their
 *     frame; the frame's maximum is subtracted.  A frame without any finite value gives zeros.  Two launches on `stream`, no
 *     host read; workspace: stof_das_workspace_bytes(F, n) bytes of device memory (block partials of the fixed-tree min / max).
 * Errors: NULL desc / bad dtype / negative sizes / a missing pointer -> STOF_ERR_BAD_ARG; more than 262140 frames (bmode:
 * 65535) or 2^39 pixels -> STOF_ERR_UNSUPPORTED; a short workspace -> STOF_ERR_WORKSPACE.  F, P or n == 0 -> STOF_OK without
 * work; A == 0 or Ne == 0 -> zeros.
 * ------------------------------------------------------------------------- */
#define STOF_DAS_F32 0
#define STOF_DAS_F64 1
#define STOF_DAS_C64 2
#define STOF_DAS_C128 3
typedef struct stof_das_desc {
    double c, t0, fs, f0;        /* speed of sound, time of sample 0, sampling and demodulation frequency */
    double fnumber;              /* receive cone: |x - xe| < z / fnumber / 2                              */
    int32_t dtype;               /* STOF_DAS_*                                                            */
    int32_t compound;            /* != 0: sum the angles                                                  */
} stof_das_desc;
int stof_das_tx_distance(const double* xe, int64_t Ne, const double* angles, int64_t A, const double* x, const double* z,
                         int64_t P, double* dtx);
int stof_das_beamform_host(const stof_das_desc* desc, const void* sig, int64_t F, int64_t A, int64_t S, int64_t Ne,
                           const double* x, const double* z, const double* dtx, int64_t P, const double* xe,
                           const uint8_t* rotate, void* out);
int stof_das_beamform(const stof_das_desc* desc, const void* sig, int64_t F, int64_t A, int64_t S, int64_t Ne,
                      const double* x, const double* z, const double* dtx, int64_t P, const double* xe,
                      const uint8_t* rotate, void* out, void* stream);
size_t stof_das_workspace_bytes(int64_t F, int64_t n);
int stof_das_bmode(int32_t dtype, const void* img, int64_t F, int64_t n, void* bmode, void* workspace, size_t workspace_bytes,
                   void* stream);

/* ------------------------------------------------------------------------- *
 * Zonzini baselines (models/zonzini.py: ZonziniNetSmall / ZonziniNetLarge), inference in exact fp32.
 * ------------------------------------------------------------------------- */
#define STOF_ZONZINI_SMALL 0      /* Conv1d 1->16->32->64->64, fc1 64->1024;   rows need L >= 936   */
#define STOF_ZONZINI_LARGE 1      /* Conv1d 1->50->100->150->200->250, fc1 250->1024; L >= 3752     */
typedef struct stof_zonzini_desc {
    int32_t variant;             /* STOF_ZONZINI_*                                                  */
    int32_t reserved;            /* 0                                                               */
} stof_zonzini_desc;
/* Host-only packer (no HIP call): params = the state_dict's fp32 tensors in module order, conv_layers.{i}.weight,
 * conv_layers.{i}.bias for every layer, then fc1.weight, fc1.bias, fc2.weight, fc2.bias (12 pointers for Small, 14
 * for Large).  out: stof_zonzini_packed_bytes(desc) bytes of host memory, copied to the device by the caller.
 * stof_zonzini_packed_bytes returns 0 for an unknown variant.                                                        */
size_t stof_zonzini_packed_bytes(const stof_zonzini_desc* desc);
int stof_zonzini_pack_weights(const stof_zonzini_desc* desc, const float* const* params, void* out, size_t out_bytes);
/* Device workspace of stof_zonzini_forward for N rows of length L (0 for an unknown variant, N <= 0 or L below the
 * minimum).  Linear in N up to 256-byte rounding per buffer.                                                         */
size_t stof_zonzini_workspace_bytes(const stof_zonzini_desc* desc, int64_t N, int64_t L);
/* x[N, 1, L] fp32 -> y[N, 1] fp32; features (optional, NULL = not written) [N, C_last] = the global average pool's
 * output.  packed: the packed blob in device memory.  Launches layer 1, one implicit-GEMM kernel per further conv
 * layer and the head on `stream`; no host sync.  Argument checks come before any HIP call: NULL pointers, N <= 0 or an
 * unknown variant -> STOF_ERR_BAD_ARG, L below the minimum -> STOF_ERR_POOL_EMPTY (the reference raises in max_pool1d
 * or in the conv), workspace too small -> STOF_ERR_WORKSPACE.                                                       */
int stof_zonzini_forward(const stof_zonzini_desc* desc, const float* x, int64_t N, int64_t L, const void* packed,
                         float* y, float* features, void* workspace, size_t workspace_bytes, void* stream);

/* The same nets for training (csrc/zonzini_train.hip): one entry per stage, exact fp32, fixed summation orders, no float atomic
 * and no library call; two runs give bitwise equal results.  Buffers of conv layer l (0-based; Lp_l its pooled length, cpad_l
 * its channels rounded up to 4): act_l [N][Lp_l][cpad_l] fp32, pad channels 0; sel_l [N][Lp_l][cpad_l] bytes: 0 = the stored
 * output is not > 0 (no gradient), 1 = conv output 2p won the pool, 2 = conv output 2p + 1 won (a tie goes to 2p, as in
 * max_pool1d's backward).  Every entry takes the frame's N and L and derives each layer's lengths from them.  Argument checks
 * come before any HIP call, as for stof_zonzini_forward: NULL pointers, N <= 0, an unknown variant or a layer outside
 * 1 .. layers - 1 -> STOF_ERR_BAD_ARG, L below the minimum -> STOF_ERR_POOL_EMPTY, N L >= 2^31 -> STOF_ERR_UNSUPPORTED, a short
 * workspace -> STOF_ERR_WORKSPACE.  All buffers are 16-byte aligned.
 *
 *   stof_zonzini_train_pack        stof_zonzini_pack_weights on the device: params = the same pointers in the same order, in
 *                                  device memory; out = stof_zonzini_packed_bytes(desc) bytes of device memory, byte for byte
 *                                  the host packer's blob (a training step packs again after every optimizer step)
 *   stof_zonzini_train_forward     the inference chain, keeping acts[l] and sel[l] of every layer, f [N][C_last] (the global
 *                                  mean) and h [N][1024] (fc1 after ReLU); y [N] is bitwise stof_zonzini_forward's
 *   stof_zonzini_train_head_bwd    from dy [N]: dfc1w [1024][C], dfc1b, dfc2w [1024], dfc2b (sums over n = 0 .. N - 1 in order)
 *                                  and df [N][cpad_last] (pad 0).  fc1w, fc2w: the parameters in torch layout.
 *   stof_zonzini_train_conv_wgrad  layer >= 1 on v_mfma_f32_32x32x2_f32: dw (cout, cin, 10), db (cout) from in = act_(layer-1),
 *                                  sel = sel_layer and dout = the gradient of act_layer [N][Lp][cpad] -- for the last layer df of
 *                                  the head instead, whose readers divide by Lp on the fly.  Per-chunk partials in the workspace
 *                                  (stof_zonzini_train_conv_wgrad_workspace_bytes, at most 64 MiB), added in a fixed order.
 *   stof_zonzini_train_dgrad_image layer's weight (cout, cin, 10) -> the stof_zonzini_train_dgrad_image_floats floats of the
 *                                  operand image of stof_zonzini_train_conv_dgrad (on the device; again when the weight changes)
 *   stof_zonzini_train_conv_dgrad  din [N][Lp_(layer-1)][cpad_(layer-1)] = the gradient of act_(layer-1); rows that no kept conv
 *                                  output reads are exactly 0.  The ReLU / pool of layer - 1 is applied by din's readers (sel).
 *   stof_zonzini_train_in_wgrad    layer 0 (Cin = 1, vector pipe): dw (cout, 1, 10), db (cout) from x [N][L], dout and sel_0
 *   stof_zonzini_train_in_dgrad    dx [N][L] from dout, sel_0 and w = conv_layers.0.weight; samples past the last kept window 0.0 */
int stof_zonzini_train_pack(const stof_zonzini_desc* desc, const float* const* params, void* out, size_t out_bytes, void* stream);
int stof_zonzini_train_forward(const stof_zonzini_desc* desc, const float* x, int64_t N, int64_t L, const void* packed,
                               float* const* acts, uint8_t* const* sel, float* f, float* h, float* y, void* stream);
int stof_zonzini_train_head_bwd(const stof_zonzini_desc* desc, const float* dy, const float* f, const float* h, const float* fc1w,
                                const float* fc2w, float* dfc1w, float* dfc1b, float* dfc2w, float* dfc2b, float* df, int64_t N,
                                void* stream);
size_t stof_zonzini_train_conv_wgrad_workspace_bytes(const stof_zonzini_desc* desc, int32_t layer);
int stof_zonzini_train_conv_wgrad(const stof_zonzini_desc* desc, int32_t layer, const float* in, const float* dout,
                                  const uint8_t* sel, float* dw, float* db, int64_t N, int64_t L, void* workspace,
                                  size_t workspace_bytes, void* stream);
size_t stof_zonzini_train_dgrad_image_floats(const stof_zonzini_desc* desc, int32_t layer);
int stof_zonzini_train_dgrad_image(const stof_zonzini_desc* desc, int32_t layer, const float* w, float* out, void* stream);
int stof_zonzini_train_conv_dgrad(const stof_zonzini_desc* desc, int32_t layer, const float* dout, const uint8_t* sel,
                                  const float* image, float* din, int64_t N, int64_t L, void* stream);
size_t stof_zonzini_train_in_wgrad_workspace_bytes(const stof_zonzini_desc* desc);
int stof_zonzini_train_in_wgrad(const stof_zonzini_desc* desc, const float* x, const float* dout, const uint8_t* sel, float* dw,
                                float* db, int64_t N, int64_t L, void* workspace, size_t workspace_bytes, void* stream);
int stof_zonzini_train_in_dgrad(const stof_zonzini_desc* desc, const float* dout, const uint8_t* sel, const float* w, float* dx,
                                int64_t N, int64_t L, void* stream);

/* ------------------------------------------------------------------------- *
 * SincNet baseline (models/sincnet.py: SincNet with the option dict of main.py:145-157: sinc conv 128 x 1023 taps,
 * Conv1d 128->128 k 11, 128->128 k 9, 128->1 k 7, each "same" padded + BatchNorm1d (eval) + LeakyReLU(0.2), the
 * last one linear), inference in exact fp32.  Rows of any length L >= 1.
 * ------------------------------------------------------------------------- */
typedef struct stof_sincnet_desc {
    double fs;                   /* sample rate the sinc layer was built with (SincConv_fast sample_rate), finite, > 0 */
    double bn_eps;               /* BatchNorm1d eps (1e-5)                                                            */
    int32_t stop_after;          /* 0 = whole network; 1..3 = run layers 0 .. stop_after - 1 only and leave the last
                                    one's post-activation output in the workspace (diagnostics; y is not written):
                                    y may then be NULL.  Buffer (stop_after - 1) & 1 at byte offset 0 or workspace_bytes(desc, N, L) / 2,
                                    float (8 + n (L + 8) + t) * 128 + c = act[n][c][t]                             */
    int32_t reserved;            /* 0                                                                                 */
} stof_sincnet_desc;
/* Host-only packer (no HIP call): params = 24 host pointers to the state_dict's fp32 tensors in module order,
 *   [0] conv.0.low_hz_ (128,1)  [1] conv.0.band_hz_ (128,1)
 *   [2] conv.1.weight (128,128,11) [3] conv.1.bias  [4] conv.2.weight (128,128,9) [5] conv.2.bias
 *   [6] conv.3.weight (1,128,7)    [7] conv.3.bias
 *   [8 + 4i .. 11 + 4i] bn.i.weight, bn.i.bias, bn.i.running_mean, bn.i.running_var   (i = 0..3)
 * The sinc filter bank is synthesised here from low_hz_ / band_hz_ (SincConv_fast.forward, models/sincnet.py:147-188)
 * in double and rounded to fp32; each BatchNorm (with the conv bias before it) becomes a per-channel affine.
 * stof_sincnet_packed_bytes returns 0 for a bad desc.                                                                */
size_t stof_sincnet_packed_bytes(const stof_sincnet_desc* desc);
int stof_sincnet_pack_weights(const stof_sincnet_desc* desc, const float* const* params, void* out, size_t out_bytes);
/* The filter bank the packer uses, bank[128][1023] fp32 (host memory; SincConv_fast.filters).                       */
int stof_sincnet_filter_bank(const stof_sincnet_desc* desc, const float* low_hz, const float* band_hz, float* bank);
/* Device workspace of stof_sincnet_forward for N rows of length L (0 for a bad desc, N <= 0 or L <= 0): two
 * channel-last ping-pong buffers of (N (L + 8) + 8) x 128 floats each.                                              */
size_t stof_sincnet_workspace_bytes(const stof_sincnet_desc* desc, int64_t N, int64_t L);
/* x[N, 1, L] fp32 -> y[N, 1, L] fp32.  packed: the packed blob in device memory.  Launches 5 kernels on `stream`;
 * no host sync.  Argument checks come before any HIP call: NULL pointers, N <= 0, L <= 0, fs non-finite or <= 0 ->
 * STOF_ERR_BAD_ARG, workspace too small -> STOF_ERR_WORKSPACE, N (L + 8) >= 2^31 -> STOF_ERR_UNSUPPORTED.           */
int stof_sincnet_forward(const stof_sincnet_desc* desc, const float* x, int64_t N, int64_t L, const void* packed,
                         float* y, void* workspace, size_t workspace_bytes, void* stream);
/* The chain rule of the filter synthesis on the host, in double: bank_grad[128][1023] = d loss / d bank ->
 * dlow_hz[128], dband_hz[128] = d loss / d low_hz_, band_hz_ (through the window, the divisions, the mirrored right half,
 * the constant centre tap, clamp: gradient 1 inside the closed interval, else 0, and abs: the sign, 0 at 0).        */
int stof_sincnet_band_grad(const stof_sincnet_desc* desc, const float* low_hz, const float* band_hz, const float* bank_grad,
                           double* dlow_hz, double* dband_hz);

/* SincNet training in exact fp32 (csrc/sincnet_train.hip; the host side is stofnet_amd/sincnet_training.py), one entry per
 * stage, all on `stream` without a host sync, an allocation or a float atomic.  128-channel tensors are in the GAP layout of
 * the inference workspace, (N (L + 8) + 8) x 128 floats (stof_sincnet_train_buffer_floats, 0 for bad dimensions), row
 * 8 + n (L + 8) + t, zero gap rows; every entry that writes such a tensor zeroes its gap rows.  The one-channel tensors of
 * layer 3 are flat [N L].  `channels` is 128 or 1.  BatchNorm runs in train mode: batch statistics over the N L >= 2 rows,
 * sums in double.  The module's running statistics are read, never written: the new ones go to new_mean / new_var.     */
size_t stof_sincnet_train_buffer_floats(int64_t N, int64_t L);
/* out[0..5]: float offsets of frag0, bank_t [1024][128], frag1, frag2, w3 [7][128] in the training blob, and its size */
int stof_sincnet_train_blob_layout(int64_t* out);
/* params (device): low_hz_, band_hz_, conv.1.weight, conv.2.weight, conv.3.weight -> the blob of the forward kernels;
 * the bank is synthesised in double on the device.                                                                   */
int stof_sincnet_train_pack(const stof_sincnet_desc* desc, const float* const* params, void* out, size_t out_bytes, void* stream);
/* stof_sincnet_pack_weights on the device: the same 24 arrays in device memory -> the inference blob, the host packer's
 * bytes up to the last bit of the device's sin / cos (no trip through the host after an optimizer step).                 */
int stof_sincnet_device_pack(const stof_sincnet_desc* desc, const float* const* params, void* out, size_t out_bytes, void* stream);
/* the flipped, transposed fragment image of conv.`layer`.weight (layer 1 or 2; 128 x taps x 128 floats)               */
int stof_sincnet_train_dgrad_image(int32_t layer, const float* w, float* out, void* stream);
/* z_l = conv_l(in) + bias without BatchNorm.  layer 0: in = x [N][L] (bias ignored); 1, 2: in = a_{l-1}; 3: in = a_2 and
 * out = z_3 [N L]                                                                                                      */
int stof_sincnet_train_conv(int32_t layer, const float* in, int64_t N, int64_t L, const void* blob_dev, const float* bias,
                            float* out, void* stream);
int stof_sincnet_train_conv_dgrad(int32_t layer, const float* dz, int64_t N, int64_t L, const float* image, float* da, void* stream);
size_t stof_sincnet_train_stats_workspace_bytes(void);
/* stat [4][channels] doubles: mean, rstd, s = gamma rstd and t = beta - mean s                                       */
int stof_sincnet_train_stats(const stof_sincnet_desc* desc, const float* z, int64_t N, int64_t L, int32_t channels,
                             const float* gamma, const float* beta, const float* run_mean, const float* run_var,
                             double momentum, double* stat, float* new_mean, float* new_var, void* workspace,
                             size_t workspace_bytes, void* stream);
/* a = leaky(z s + t) (channels = 128) or y = z s + t (channels = 1), the affine in double and rounded once            */
int stof_sincnet_train_apply(const float* z, int64_t N, int64_t L, int32_t channels, const double* stat, float* out, void* stream);
/* da (channels = 1: dy), a (the LeakyReLU decision is a > 0; NULL for channels = 1), z, stat -> dgamma, dbeta, dz       */
int stof_sincnet_train_bn_bwd(const float* da, const float* a, const float* z, const double* stat, const float* gamma,
                              int64_t N, int64_t L, int32_t channels, float* dgamma, float* dbeta, float* dz,
                              void* workspace, size_t workspace_bytes, void* stream);
size_t stof_sincnet_train_conv_wgrad_workspace_bytes(int32_t layer);
int stof_sincnet_train_conv_wgrad(int32_t layer, const float* a_prev, const float* dz, int64_t N, int64_t L, float* dw,
                                  float* db, void* workspace, size_t workspace_bytes, void* stream);
size_t stof_sincnet_train_out_wgrad_workspace_bytes(void);
int stof_sincnet_train_out_wgrad(const float* a2, const float* dz3, int64_t N, int64_t L, float* dw, float* db, void* workspace,
                                 size_t workspace_bytes, void* stream);
int stof_sincnet_train_out_dgrad(const float* dz3, const float* w, int64_t N, int64_t L, float* da2, void* stream);
size_t stof_sincnet_train_bank_grad_workspace_bytes(void);
/* G [128][1023] = d loss / d bank from x [N][L] and dz_0                                                               */
int stof_sincnet_train_bank_grad(const float* x, const float* dz0, int64_t N, int64_t L, float* G, void* workspace,
                                 size_t workspace_bytes, void* stream);
/* stof_sincnet_band_grad on the device, rounded to fp32                                                                */
int stof_sincnet_train_band_grad(const stof_sincnet_desc* desc, const float* low_hz, const float* band_hz, const float* G,
                                 float* dlow_hz, float* dband_hz, void* stream);
/* dx [N][L] from dz_0 and the training blob (vector pipe; only when the frame asks for its gradient)                   */
int stof_sincnet_train_in_dgrad(const float* dz0, const void* blob_dev, int64_t N, int64_t L, float* dx, void* stream);

/* ------------------------------------------------------------------------- *
 * EDSR_1D and ESPCN_1D (models/edsr_1d.py, models/espcn_1d.py), the baselines riding on SampleShuffle1D, inference
 * in exact fp32.  Rows of any length L >= 1.  Conventions as for stof_zonzini_*: host-only packers, the packed blob
 * is copied to the device by the caller, no allocation and no host sync, argument checks before any HIP call (NULL
 * pointers, N <= 0, L <= 0 or a bad desc -> STOF_ERR_BAD_ARG, workspace too small -> STOF_ERR_WORKSPACE,
 * N (L + 1) >= 2^31 - 64 -> STOF_ERR_UNSUPPORTED).
 * ------------------------------------------------------------------------- */
typedef struct stof_edsr_desc {
    int32_t num_blocks;          /* residual blocks, 0 .. 1024 (num_features is 64, num_channels is 1)                */
    int32_t upscale_factor;      /* r in {1, 2, 4, 8, 16, 32, 64}: 64 / r channels survive the shuffle                */
} stof_edsr_desc;
/* params = 2 (2 B + 3) host pointers in state_dict order: conv_input.weight (64,1,3), .bias, then per block
 * conv1.weight (64,64,3), conv1.bias, conv2.weight, conv2.bias, then conv_mid.weight, .bias, conv_output.weight
 * (1,64/r,3), .bias.  stof_edsr_packed_bytes returns 0 for a bad desc.                                               */
size_t stof_edsr_packed_bytes(const stof_edsr_desc* desc);
int stof_edsr_pack_weights(const stof_edsr_desc* desc, const float* const* params, void* out, size_t out_bytes);
/* Three channel-last buffers of (N (L + 1) + 1) x 64 floats (0 for a bad desc, N <= 0 or L <= 0).                    */
size_t stof_edsr_workspace_bytes(const stof_edsr_desc* desc, int64_t N, int64_t L);
/* x[N, 1, L] -> y[N, 1, L r]; trunk (optional, NULL = not written) [N, L, 64] = conv_mid + the long skip, the input
 * of the shuffle in channel-last order.  Launches 4 + 2 B kernels on `stream`.                                       */
int stof_edsr_forward(const stof_edsr_desc* desc, const float* x, int64_t N, int64_t L, const void* packed, float* y,
                      float* trunk, void* workspace, size_t workspace_bytes, void* stream);

typedef struct stof_espcn_desc {
    int32_t upscale_factor;      /* r in 1 .. 64                                                                      */
    int32_t reserved;            /* 0                                                                                 */
} stof_espcn_desc;
/* params = 6 host pointers: conv1.weight (64,1,5), .bias, conv2.weight (32,64,3), .bias, conv3.weight (r,32,3), .bias */
size_t stof_espcn_packed_bytes(const stof_espcn_desc* desc);
int stof_espcn_pack_weights(const stof_espcn_desc* desc, const float* const* params, void* out, size_t out_bytes);
/* x[N, 1, L] -> y[N, 1, L r] = sigmoid(logits); logits (optional, NULL = not written) [N, 1, L r] = the shuffled
 * conv3 output.  One kernel on `stream`, no workspace.                                                               */
int stof_espcn_forward(const stof_espcn_desc* desc, const float* x, int64_t N, int64_t L, const void* packed, float* y,
                       float* logits, void* stream);

/* ------------------------------------------------------------------------- *
 * Wave-U-Net (models/wave_unet.py, `main.py model=unet`), inference in exact fp32 with eval-mode BatchNorm folded
 * into the convolutions by the host packer (in double).  Served: channels_interval = 16, n_layers 1 .. 12, rows of a
 * length L that is a multiple of 2^n_layers.  Conventions as for stof_edsr_*; anything outside the served range ->
 * STOF_ERR_BAD_ARG (0 from the size functions), N = 0 -> STOF_OK without a launch, N L >= 2^31 - 64 ->
 * STOF_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------- */
typedef struct stof_waveunet_desc {
    int32_t n_layers;            /* n in 1 .. 12                                                                      */
    int32_t channels_interval;   /* 16                                                                                */
} stof_waveunet_desc;
/* params = 6 (2 n + 1) + 2 host pointers, the state dict in module order without the num_batches_tracked entries:
 * per block (encoder.0 .. n-1, middle, decoder.0 .. n-1) conv weight, conv bias, BN weight, BN bias, running mean,
 * running var; then out.0.weight (1,17,1) and out.0.bias.  The blob layout is documented in csrc/waveunet.hip.      */
size_t stof_waveunet_packed_bytes(const stof_waveunet_desc* desc);
int stof_waveunet_pack_weights(const stof_waveunet_desc* desc, const float* const* params, void* out, size_t out_bytes);
/* The n skips [N, L / 2^i, 16 (i + 1)], the middle map and two decoder buffers [N, L, 16] (0 for a bad desc, N <= 0
 * or a bad L).                                                                                                      */
size_t stof_waveunet_workspace_bytes(const stof_waveunet_desc* desc, int64_t N, int64_t L);
/* x[N, 1, L] -> y[N, 1, L]; bottleneck (optional) [N, L / 2^n, 16 n] = the middle block's output, channel-last;
 * logits (optional) [N, 1, L] = the output convolution before the tanh.  Launches 2 n + 2 kernels on `stream`.      */
int stof_waveunet_forward(const stof_waveunet_desc* desc, const float* x, int64_t N, int64_t L, const void* packed, float* y,
                          float* bottleneck, float* logits, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * Wave-U-Net training (csrc/waveunet_train.hip): one entry per stage of a step, each on one convolution or one
 * Conv + BatchNorm + LeakyReLU(0.1) block, exact fp32, no float atomic: two runs are bitwise equal.  Activations and
 * gradients are dense channel-last fp32 [N, L, C] device arrays, C a multiple of 16 up to 384; taps is 15 or 5;
 * `mode` names the virtual input of a convolution of output length Lout: 0 = every second position of src
 * [N, 2 Lout, cin] (taps 15), 1 = the x2 align-corners interpolation of low [N, Lout / 2, cu] concatenated with src
 * [N, Lout, cin - cu] (taps 5), 2 = src [N, Lout, cin].  Every entry launches on `stream` and returns a stof_status;
 * the size functions return 0 for arguments they do not serve.  The chunk rules are documented in the .hip file.
 * ------------------------------------------------------------------------- */
/* out[10]: rows per partial / partials at the most of the statistics (0, 1), the head's weight gradient (2, 3),
 * encoder 0's weight gradient (4, 5) and the convolutions' weight gradient (6, 7); the positions per tile (8); the
 * largest low length M the interpolation transpose serves (9).                                                       */
int stof_waveunet_train_constants(int64_t* out);
/* Host only, no device: for M low positions the fp32 coordinates i0, i1, l0, l1 [2 M] of every high position as the
 * kernels compute them, and the window lo, hi [M] (inclusive) of high positions that the transpose visits per low one. */
int stof_waveunet_interp_table(int64_t M, int32_t* i0, int32_t* i1, float* l0, float* l1, int32_t* lo, int32_t* hi);
/* The fragment image of weight w [cout][cin][taps] for stof_waveunet_train_conv: flip = 0 the forward's, flip = 1 the
 * data gradient's (cin and cout swapped, taps reversed).                                                             */
size_t stof_waveunet_train_frag_floats(int32_t cin, int32_t cout, int32_t taps, int32_t flip);
int stof_waveunet_train_pack_frag(const float* w, int32_t cin, int32_t cout, int32_t taps, int32_t flip, float* frag, void* stream);
/* encoder 0: weight [16][1][15], bias [16] -> image [256] */
int stof_waveunet_train_pack_in(const float* w, const float* b, float* image, void* stream);
/* encoder 0: z [N, L, 16] = conv(x [N, L]) + bias */
int stof_waveunet_train_in_conv(const float* x, int64_t N, int64_t L, const float* image, float* z, void* stream);
/* out [N, Lout, cout] = conv(virtual input) (+ bias, if not NULL); frag: an image whose input width is cin */
int stof_waveunet_train_conv(const float* src, const float* low, int64_t N, int64_t Lout, int32_t cin, int32_t cu, int32_t cout,
                             int32_t taps, int32_t mode, const float* frag, const float* bias, float* out, void* stream);
size_t stof_waveunet_train_stats_workspace_bytes(void);
/* z [rows, ch] -> stat [4][ch] double (mean, rstd, s, t) and the blended running statistics (not in place) */
int stof_waveunet_train_stats(const float* z, int64_t rows, int32_t ch, const float* gamma, const float* beta, const float* run_mean,
                              const float* run_var, double eps, double momentum, double* stat, float* new_mean, float* new_var,
                              void* workspace, size_t workspace_bytes, void* stream);
/* a = leaky_0.1(z s + t) */
int stof_waveunet_train_apply(const float* z, int64_t rows, int32_t ch, const double* stat, float* a, void* stream);
/* y [N, L] = tanh(w[0:16] . o [N, L, 16] + w[16] x + b) */
int stof_waveunet_train_head(const float* o, const float* x, int64_t N, int64_t L, const float* w, const float* b, float* y, void* stream);
size_t stof_waveunet_train_head_bwd_workspace_bytes(void);
/* dout [N, L, 16], dw [17], db [1]; dxh [N, L] (NULL = not wanted) = w[16] dy (1 - y^2) */
int stof_waveunet_train_head_bwd(const float* dy, const float* y, const float* o, const float* x, int64_t N, int64_t L, const float* w,
                                 float* dout, float* dxh, float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream);
/* da, a, z [rows, ch] -> dgamma, dbeta [ch], dz [rows, ch]; workspace as for the statistics */
int stof_waveunet_train_bn_bwd(const float* da, const float* a, const float* z, const double* stat, int64_t rows, int32_t ch,
                               float* dgamma, float* dbeta, float* dz, void* workspace, size_t workspace_bytes, void* stream);
size_t stof_waveunet_train_wgrad_workspace_bytes(int64_t N, int64_t Lout, int32_t cin, int32_t cout, int32_t taps);
/* dw [cout][cin][taps], db [cout] from dz [N, Lout, cout] and the forward's virtual input (cout <= 192) */
int stof_waveunet_train_wgrad(const float* src, const float* low, const float* dz, int64_t N, int64_t Lout, int32_t cin, int32_t cu,
                              int32_t cout, int32_t taps, int32_t mode, float* dw, float* db, void* workspace, size_t workspace_bytes,
                              void* stream);
size_t stof_waveunet_train_in_wgrad_workspace_bytes(void);
/* encoder 0: dw [16][1][15], db [16] from x [N, L] and dz [N, L, 16] */
int stof_waveunet_train_in_wgrad(const float* x, const float* dz, int64_t N, int64_t L, float* dw, float* db, void* workspace,
                                 size_t workspace_bytes, void* stream);
/* g [N, 2 M, cg] (its first cu channels) -> dlow [N, M, cu]: the transpose of the interpolation */
int stof_waveunet_train_interp_t(const float* g, int64_t N, int64_t M, int32_t cg, int32_t cu, float* dlow, void* stream);
/* out [N, L, cs] = gdec [N, L, cu + cs][.., cu:] + (at even positions) genc [N, L / 2, cs] */
int stof_waveunet_train_skip_sum(const float* gdec, const float* genc, int64_t N, int64_t L, int32_t cu, int32_t cs, float* out,
                                 void* stream);
/* encoder 0: dx [N, L] = (dxh, if not NULL) + the data gradient of dz [N, L, 16] through w [16][1][15] */
int stof_waveunet_train_in_dgrad(const float* dz, const float* w, const float* dxh, int64_t N, int64_t L, float* dx, void* stream);

/* ------------------------------------------------------------------------- *
 * Kuleshov (models/kuleshov.py with num_layers = 4, `main.py model=kuleshov`), inference in exact fp32 with eval-mode
 * BatchNorm as a per-channel affine computed by the host packer in double.  Served: input_length >= 641 (the
 * shortest row for which every convolution has an output), output_length >= 1.  Conventions as for stof_edsr_*;
 * anything outside the served range -> STOF_ERR_BAD_ARG (0 from the size functions), N = 0 -> STOF_OK without a
 * launch, N x (length of the last concatenation) >= 2^31 - 256 -> STOF_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------- */
typedef struct stof_kuleshov_desc {
    int64_t input_length;        /* L: rows are cropped to their first L samples                                      */
    int64_t output_length;       /* O: outputs of output_fc                                                           */
    double bn_eps;               /* eps of every BatchNorm1d (torch default 1e-5)                                     */
    int32_t tile_variant;        /* 0: the wave tile of each convolution is chosen by its size; 1, 2, 3: every
                                  * convolution runs the 32 x 32, 32 x 128 or 64 x 128 wave tile (bitwise the same)  */
    int32_t reserved;            /* 0                                                                                 */
} stof_kuleshov_desc;
/* params = 54 host pointers, the state dict in module order without the num_batches_tracked entries: per down block
 * i = 0..3 down_conv{i}.weight, .bias, down_bn{i}.weight, .bias, .running_mean, .running_var; bottleneck.weight,
 * .bias; per up block the same six of up_conv{i} / up_bn{i}; final_conv.weight (2,128,9), .bias; output_fc.weight
 * (O, fc_dim), .bias.  The blob layout is documented in csrc/kuleshov.hip.                                          */
size_t stof_kuleshov_packed_bytes(const stof_kuleshov_desc* desc);
int stof_kuleshov_pack_weights(const stof_kuleshov_desc* desc, const float* const* params, void* out, size_t out_bytes);
/* The four concatenation buffers, the bottleneck map and the Linear layer's input for N rows (0 for a bad desc or
 * N <= 0); about 5.4 MB per row at L = 2000.                                                                        */
size_t stof_kuleshov_workspace_bytes(const stof_kuleshov_desc* desc, int64_t N);
/* x: N rows of at least L samples, x_row_stride (>= L) floats apart -> y[N, 1, O].  Optional taps (NULL = not
 * written), channel-last: bottleneck [N, B, 512] = the output of bottleneck_last; final_in [N, Lc3, 128] = the input
 * of final_conv (shuffled up_conv3 output, then down block 0's output); final_out [N, F, 2] = final_conv's output =
 * the Linear layer's input.  Launches 12 kernels on `stream`.                                                       */
int stof_kuleshov_forward(const stof_kuleshov_desc* desc, const float* x, int64_t N, int64_t x_row_stride,
                          const void* packed, float* y, float* bottleneck, float* final_in, float* final_out,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * Kuleshov training (csrc/kuleshov_train.hip; the host side is stofnet_amd/kuleshov_training.py): one entry per stage,
 * exact fp32 with double where the file says so, no float atomic: two runs are bitwise equal.  Activations and gradients
 * are channel-last fp32 device arrays; widths are multiples of 128 up to 1024, taps 9, 17, 33 or 65.  A concatenation
 * buffer is addressed by a pointer to its first served row and the floats between waveforms (`*_n_stride`).  Every
 * argument is checked before the first device call: STOF_ERR_BAD_ARG outside the served range (0 from the size
 * functions), STOF_ERR_WORKSPACE for a short workspace, STOF_ERR_UNSUPPORTED where 32-bit indexing would overflow.
 *
 * Dropout: the keep-mask is a pure function of (seed, call, rank, site, row n, element e = t C + c of the layer's
 * unshuffled [position][channel] output): Philox4x32-10 with key (seed lo, seed hi), counter (e >> 2, n, call,
 * (rank << 3) | site), word e & 3; site 0 = the bottleneck, 1..4 = up 0..3; kept when word >= floor(p 2^32), kept
 * values are scaled by 1.0f / (1.0f - p); p in [0, 1).  It is never stored.
 * ------------------------------------------------------------------------- */
/* Host only, no device: keep[count] = 1 where element e = 0 .. count - 1 of row n is kept.                            */
int stof_kuleshov_dropout_keep(uint64_t seed, uint32_t call, uint32_t rank, int32_t site, int64_t n, int64_t count, double p,
                               uint8_t* keep);
/* out[8]: rows per partial / partials at the most of the statistics, BN backward and bias sums (0, 1), the wide
 * convolutions' weight gradient (2, 3), final_conv's (4, 5) and down_conv0's (6, 7).                                  */
int stof_kuleshov_train_constants(int64_t* out);
/* The fragment image of weight w [cout][cin][taps] for stof_kuleshov_train_conv: kind 0 the forward's, 1 the stride-1
 * data gradient's, 2 and 3 the even and odd tap class of the stride-2 data gradient's.                               */
size_t stof_kuleshov_train_frag_floats(int32_t cin, int32_t cout, int32_t taps, int32_t kind);
int stof_kuleshov_train_pack_frag(const float* w, int32_t cin, int32_t cout, int32_t taps, int32_t kind, float* frag, void* stream);
/* final_conv.weight [2][128][9] -> image [2][9][128]; output_fc.weight [O][2 F] -> its fragment image                 */
int stof_kuleshov_train_pack_final(const float* w, float* image, void* stream);
size_t stof_kuleshov_train_fc_frag_floats(const stof_kuleshov_desc* desc);
int stof_kuleshov_train_pack_fc(const stof_kuleshov_desc* desc, const float* w, float* frag, void* stream);
/* down_conv0: u [N][D0][128] = leaky0.01(conv(x[:, :L]) + b), w [128][1][65]                                          */
int stof_kuleshov_train_down0(const float* x, int64_t x_row_stride, int64_t N, int64_t L, const float* w, const float* b, float* u,
                              void* stream);
/* out[n][t][c] = sum over the `rows` x cin floats of `in` from row stride t on, times the image (+ bias, if not NULL;
 * through leaky0.01 if slope01), at out + n out_n_stride + t out_t_stride + c                                         */
int stof_kuleshov_train_conv(const float* in, int64_t in_n_stride, int64_t N, int64_t Lout, int32_t cin, int32_t cout, int32_t rows,
                             int32_t stride, const float* frag, const float* bias, int32_t slope01, float* out, int64_t out_n_stride,
                             int64_t out_t_stride, void* stream);
size_t stof_kuleshov_train_stats_workspace_bytes(void);
/* z [rows, ch] -> stat [4][ch] double (mean, rstd, s, t) and the blended running statistics (not in place)            */
int stof_kuleshov_train_stats(const float* z, int64_t rows, int32_t ch, const float* gamma, const float* beta, const float* run_mean,
                              const float* run_var, double eps, double momentum, double* stat, float* new_mean, float* new_var,
                              void* workspace, size_t workspace_bytes, void* stream);
/* a = leaky0.2(u s + t) at out + n out_n_stride + t ch + c                                                            */
int stof_kuleshov_train_apply_down(const float* u, int64_t N, int64_t D, int32_t ch, const double* stat, float* out, int64_t out_n_stride,
                                   void* stream);
/* a = (z s + t) keep scale of z [N][U][ch] at the pixel-shuffled address out + n out_n_stride + (2 t + (c & 1)) ch / 2 + c / 2 */
int stof_kuleshov_train_apply_up(const float* z, int64_t N, int64_t U, int32_t ch, const double* stat, uint64_t seed, uint32_t call,
                                 uint32_t rank, int32_t site, double p, float* out, int64_t out_n_stride, void* stream);
/* out [N][B][512] = leaky0.2(z keep scale), site 0                                                                    */
int stof_kuleshov_train_apply_bott(const float* z, int64_t N, int64_t B, uint64_t seed, uint32_t call, uint32_t rank, double p, float* out,
                                   void* stream);
/* final_conv and output_fc as in inference: cat3 [N][Lc3][128] -> flat [N][Kp] (kept for the backward), y [N][O]       */
int stof_kuleshov_train_tail(const stof_kuleshov_desc* desc, const float* cat3, int64_t N, const float* final_image, const float* final_bias,
                             const float* fc_frag, const float* fc_bias, float* flat, float* y, void* stream);
/* output_fc: dflat [N][Kp] = dy w, dw [O][2 F] = dy^T flat, db [O]                                                    */
int stof_kuleshov_train_fc_bwd(const stof_kuleshov_desc* desc, const float* dy, const float* flat, const float* w, int64_t N, float* dflat,
                               float* dw, float* db, void* stream);
size_t stof_kuleshov_train_final_bwd_workspace_bytes(void);
/* final_conv: dcat3 [N][Lc3][128], dw [2][128][9], db [2] from dflat and cat3                                         */
int stof_kuleshov_train_final_bwd(const stof_kuleshov_desc* desc, const float* dflat, const float* cat3, const float* w, int64_t N,
                                  float* dcat3, float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream);
/* g [N][U][ch] = (the gradient at the shuffled address of dcat) keep scale                                            */
int stof_kuleshov_train_gather_up(const float* dcat, int64_t dcat_n_stride, int64_t N, int64_t U, int32_t ch, uint64_t seed, uint32_t call,
                                  uint32_t rank, int32_t site, double p, float* g, void* stream);
/* g [N][D][ch] = (dskip, then + dnext [N][D][ch] if not NULL) (a > 0 ? 1 : 0.2); dskip and a are rows of concatenation buffers */
int stof_kuleshov_train_gather_down(const float* dskip, int64_t dskip_n_stride, const float* dnext, const float* a, int64_t a_n_stride,
                                    int64_t N, int64_t D, int32_t ch, float* g, void* stream);
/* the bottleneck: dz [N][B][512] = g (z keep > 0 ? 1 : 0.2) keep scale                                                */
int stof_kuleshov_train_gather_bott(const float* g, const float* z, int64_t N, int64_t B, uint64_t seed, uint32_t call, uint32_t rank,
                                    double p, float* dz, void* stream);
/* g, zu [rows, ch] -> dgamma, dbeta [ch], dz [rows, ch] (slope01: times the leaky0.01 decision zu > 0); workspace as
 * for the statistics                                                                                                  */
int stof_kuleshov_train_bn_bwd(const float* g, const float* zu, const double* stat, int64_t rows, int32_t ch, int32_t slope01, float* dgamma,
                               float* dbeta, float* dz, void* workspace, size_t workspace_bytes, void* stream);
size_t stof_kuleshov_train_wgrad_workspace_bytes(int64_t N, int64_t Lout, int32_t cin, int32_t cout, int32_t taps);
/* dw [cout][cin][taps], db [cout] from dz [N][Lout][cout] and the convolution's input (stride 1 or 2)                 */
int stof_kuleshov_train_wgrad(const float* in, int64_t in_n_stride, const float* dz, int64_t N, int64_t Lout, int32_t cin, int32_t cout,
                              int32_t taps, int32_t stride, float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream);
size_t stof_kuleshov_train_dgrad_workspace_bytes(int64_t N, int64_t Lout, int32_t cout, int32_t taps, int32_t stride);
/* out [N][Lin][cin]: the gradient of the convolution's input from dz [N][Lout][cout]; frag0: the image of kind 1
 * (stride 1) or 2 (stride 2), frag1: of kind 3 (stride 2 only).  Input rows that no output reaches come out as zeros. */
int stof_kuleshov_train_dgrad(const float* dz, int64_t N, int64_t Lout, int32_t cin, int32_t cout, int32_t taps, int32_t stride,
                              const float* frag0, const float* frag1, int64_t Lin, float* out, void* workspace, size_t workspace_bytes,
                              void* stream);
size_t stof_kuleshov_train_down0_bwd_workspace_bytes(void);
/* down_conv0: dw [128][1][65], db [128] from x and dz [N][D0][128]; dx (NULL = not wanted): N rows of L floats          */
int stof_kuleshov_train_down0_bwd(const float* x, int64_t x_row_stride, const float* dz, const float* w, int64_t N, int64_t L, float* dw,
                                  float* db, float* dx, int64_t dx_row_stride, void* workspace, size_t workspace_bytes, void* stream);

/* toa_rmse (utils/metrics.py:9-41): gt[N, G], es[N, E] fp32 with 0/NaN/inf as padding ->
 * out[N, 7] = (rmse, precision, recall, jaccard, tp, fp, fn).                  */
int stof_toa_rmse(const float* gt, const float* es, int64_t N, int64_t G, int64_t E, float tol,
                  float* out, void* stream);

/* ------------------------------------------------------------------------- *
 * Training step building blocks (main.py:204-248), exact fp32.
 * Activations are channel-last [N][L][C] fp32 device buffers owned by the caller.
 * ------------------------------------------------------------------------- */
#define STOF_ACT_NONE 0
#define STOF_ACT_RELU 1
#define STOF_ACT_LRELU 2

/* Conv1d weights (cout, cin, K) -> tap-major [K][cout][cin] (transpose_flip = 0, forward) or the
 * data-gradient operand [K][cin][cout] with flipped taps (transpose_flip = 1).  precision = STOF_PREC_F16X3
 * writes the split-fp16 operand image instead ([K][A][B_pad/64][64 hi | 64 lo]); `out` must hold
 * stof_train_repack_floats() floats.  stof_train_conv must be called with the same precision.       */
size_t stof_train_repack_floats(int32_t cout, int32_t cin, int32_t K, int32_t transpose_flip, int32_t precision);
int stof_train_repack(const float* w, float* out, int32_t cout, int32_t cin, int32_t K, int32_t transpose_flip,
                      int32_t precision, void* stream);
/* y = act(bias + conv_same(x, w)) + residual                     (saved == NULL: F.conv1d forward,
 *                                                                   models/stofnet.py:45,56,62,65,100,106)
 * y = (conv_same(x, w) + residual) * act'(saved)                  (saved != NULL: autograd of the same ops)
 * x[N,L,cin], w tap-major [K][cout][cin], y/residual/saved [N,L,cout]; K odd <= 9.                  */
int stof_train_conv(const float* x, const float* w_tapmajor, const float* bias, const float* residual,
                    const float* saved, float* y, int64_t N, int64_t L, int32_t cin, int32_t cout,
                    int32_t K, int32_t act, int32_t precision, void* stream);
/* dw (cout,cin,K) = sum_t dy[t][o] x[t+d-pad][c];  db[cout] = sum_t dy[t][o]  (db may be NULL).  Overwrites
 * dw/db; partial sums go through `workspace` and are added in a fixed order (bitwise reproducible).   */
size_t stof_train_wgrad_workspace_bytes(int32_t cin, int32_t cout, int32_t K);
int stof_train_wgrad(const float* x, const float* dy, float* dw, float* db, int64_t N, int64_t L,
                     int32_t cin, int32_t cout, int32_t K, float out_scale, int32_t precision, void* workspace,
                     size_t workspace_bytes, void* stream);
/* r4: the weight / bias gradients of `count` (<= 12) 64 -> 64 layers of kernel size K in ONE launch pair (split-fp16 arithmetic):
 * the eleven k7 layers of the body (models/stofnet.py:31) in the training step.  x[i], dy[i] channel-last [N][L][64];
 * dw[i] (64,64,K), db[i] (64) are overwritten; partial sums are added in a fixed order (bitwise reproducible).          */
size_t stof_train_wgrad_batch_workspace_bytes(int32_t count, int32_t K);
int stof_train_wgrad_batch(const float* const* x, const float* const* dy, float* const* dw, float* const* db, int32_t count,
                           int64_t N, int64_t L, int32_t K, float out_scale, void* workspace, size_t workspace_bytes,
                           void* stream);
/* The same with operands stored as SPLIT ROWS (bit i of x_split / dy_split: operand i): a [N][L] tensor of 256-byte rows
 * [64 x fp16 hi | 64 x fp16 lo] with value = hi + lo -- what stof_train_sweep_split / stof_train_sweep_bwd_split dump (the halves the
 * sweeps compute anyway), so this kernel stages them into LDS without converting.  Split operands must be 16-byte aligned.  */
int stof_train_wgrad_batch_split(const float* const* x, const float* const* dy, float* const* dw, float* const* db, int32_t count,
                                 uint32_t x_split, uint32_t dy_split, int64_t N, int64_t L, int32_t K, float out_scale,
                                 void* workspace, size_t workspace_bytes, void* stream);
/* conv1 (1->64, k9) + ReLU forward to channel-last, and its weight gradient (g masked by relu').    */
int stof_train_conv1(const float* x, const float* w, const float* b, float* y, int64_t N, int64_t L, void* stream);
size_t stof_train_conv1_wgrad_workspace_bytes(void);
int stof_train_conv1_wgrad(const float* x, const float* g, const float* saved, float* dw, float* db,
                           int64_t N, int64_t L, float out_scale, void* workspace, size_t workspace_bytes,
                           void* stream);
/* Gradient with respect to the input frame, which the reference's autograd yields for free (models/stofnet.py:45):
 * dx[N][L] = out_scale * conv1^T(g * relu'(saved)), g and saved channel-last [N][L][64], w = conv1.weight (64,1,9).   */
int stof_train_conv1_dgrad(const float* g, const float* saved, const float* w, float* dx, int64_t N, int64_t L,
                           float out_scale, void* stream);
/* The same three for any width of models/stofnet.py:11,23 (in_channels Cin = 1..16, num_features F = 1..256; 9 taps, padding
 * 4), exact fp32 on the vector pipe.  x and dx are NCL [N][Cin][L] as the module receives them, y / g / saved channel-last
 * [N][L][F], w = conv1.weight (F,Cin,9), dw (F,Cin,9), db (F).  One fixed-order fmaf chain per output (bias, then input
 * channels in order, taps 0..8 within each; dx: per tile of 64 output channels a chain over them in order, taps within, the
 * tiles' sums added in order); the weight gradient adds per-group partials in a fixed order (no float atomics: bitwise
 * repeatable), workspace = stof_train_conv1_c_wgrad_workspace_bytes.
 * STOF_ERR_BAD_ARG on NULL or a width out of range, STOF_OK on an empty batch (dw / db zeroed), STOF_ERR_UNSUPPORTED where
 * N L exceeds 2^31.  The 1 -> 64 entry points above stay what the shipped geometry runs.                                 */
int stof_train_conv1_c(const float* x, const float* w, const float* b, float* y, int64_t N, int32_t Cin, int64_t L,
                       int32_t F, void* stream);
size_t stof_train_conv1_c_wgrad_workspace_bytes(int32_t Cin, int32_t F);
int stof_train_conv1_c_wgrad(const float* x, const float* g, const float* saved, float* dw, float* db, int64_t N,
                             int32_t Cin, int64_t L, int32_t F, float out_scale, void* workspace, size_t workspace_bytes,
                             void* stream);
int stof_train_conv1_c_dgrad(const float* g, const float* saved, const float* w, float* dx, int64_t N, int32_t Cin,
                             int64_t L, int32_t F, float out_scale, void* stream);
/* The two ends of EDSR_1D(1, 64, B, r | 64) (models/edsr_1d.py:22-45) for training; the 2 B + 1 body convolutions 64 -> 64,
 * k 3 are stof_train_conv / stof_train_wgrad.  Exact fp32 on the vector pipe, activations channel-last [N][L][64], x / dx
 * [N][L], y / dy [N][L r]: read channel-last, the trunk [N][L][64] IS its SampleShuffle1D(r) image [N][L r][64 / r].
 * r in {1, 2, 4, 8, 16, 32, 64}.  Every [N][L][64] operand (a0, g, g2, saved, trunk, dtrunk) must be 16-byte aligned: all
 * six kernels, stof_train_edsr_out included, move them as 16-byte vectors.
 *   stof_train_edsr_in         a0 = relu(conv_input(x)), w (64,1,3), padding 1: one fmaf chain per output (bias, taps 0..2)
 *   stof_train_edsr_in_wgrad   dw (64,1,3), db (64) = out_scale * gradient from (g + g2) * [saved > 0]; g2 (may be NULL) carries
 *                              the long skip's gradient, saved = a0
 *   stof_train_edsr_in_dgrad   dx = out_scale * conv_input^T((g + g2) * [saved > 0])
 *   stof_train_edsr_out        y = conv_output(shuffle(trunk)), w (1,64/r,3): bias, then taps 0..2 over the channels in order
 *   stof_train_edsr_out_dgrad  dtrunk[n][t][j (64/r) + c] = sum_k w[c][k] dy[n][t r + j - k + 1] (zero outside the waveform)
 *   stof_train_edsr_out_wgrad  dw[c][k] = out_scale * sum dy[n][m] shuffle(trunk)[n][m + k - 1][c], db = out_scale * sum dy
 * The weight gradients add per-group partials from `workspace` (the *_workspace_bytes query) in a fixed order: no float
 * atomics, two runs are bitwise equal.  STOF_ERR_BAD_ARG on NULL or a bad r, STOF_OK on an empty batch (dw / db zeroed),
 * STOF_ERR_UNSUPPORTED where N L 64 reaches 2^31.                                                                        */
int stof_train_edsr_in(const float* x, const float* w, const float* b, float* y, int64_t N, int64_t L, void* stream);
size_t stof_train_edsr_in_wgrad_workspace_bytes(void);
int stof_train_edsr_in_wgrad(const float* x, const float* g, const float* g2, const float* saved, float* dw, float* db,
                             int64_t N, int64_t L, float out_scale, void* workspace, size_t workspace_bytes, void* stream);
int stof_train_edsr_in_dgrad(const float* g, const float* g2, const float* saved, const float* w, float* dx, int64_t N,
                             int64_t L, float out_scale, void* stream);
int stof_train_edsr_out(const float* trunk, const float* w, const float* b, float* y, int64_t N, int64_t L, int32_t r,
                        void* stream);
int stof_train_edsr_out_dgrad(const float* dy, const float* w, float* dtrunk, int64_t N, int64_t L, int32_t r, void* stream);
size_t stof_train_edsr_out_wgrad_workspace_bytes(int32_t r);
int stof_train_edsr_out_wgrad(const float* trunk, const float* dy, float* dw, float* db, int64_t N, int64_t L, int32_t r,
                              float out_scale, void* workspace, size_t workspace_bytes, void* stream);
/* ESPCN_1D(r) (models/espcn_1d.py:31-36), r = 1..64, for training: one entry per stage, exact fp32, activations saved in
 * device memory channel-last and un-gapped: h1 [N][L][64], h2 [N][L][32], x / dx [N][L], y / dy [N][L r] (channel-last z
 * [N][L][r] IS the shuffled row, so y[n][l r + j] = sigmoid(z[n][l][j])).  The zero padding of conv2 and conv3 is zeros of h1
 * and h2.  h1, h2, g1, g2 and the fragment image must be 16-byte aligned (moved as 16-byte vectors); x, y, dy, dx and the
 * parameters, read in torch layout from device memory, need 4 bytes.
 *   stof_train_espcn_in         h1 = tanh(conv1(x)), w (64,1,5), padding 2: one fmaf chain per output (bias, taps 0..4)
 *   stof_train_espcn_repack     conv2.weight (32,64,3) -> the stof_train_espcn_repack_floats() floats of the MFMA operand image
 *                               that stof_train_espcn_mid reads (on the device; repack when the weight changes)
 *   stof_train_espcn_mid        h2 = tanh(conv2(h1) + b2) on v_mfma_f32_32x32x2_f32: k = tap 64 + ci, K group q (8 products) into
 *                               partial sum q mod 8, the eight sums added in order, then the bias
 *   stof_train_espcn_out        y = sigmoid(conv3(h2) + b3), w (r,32,3): bias, then taps 0..2 over the channels in order
 *   stof_train_espcn_out_wgrad  dw (r,32,3), db (r) = out_scale * gradient from dz = dy y (1 - y) and h2; y = the saved output
 *   stof_train_espcn_out_dgrad  g2 [N][L][32] = conv3^T(dz) (1 - h2^2): tanh' of conv2's output is applied here, so conv2's two
 *                               gradients are stof_train_wgrad(h1, g2, 64 -> 32) and stof_train_conv(g2, flipped image, 32 -> 64)
 *   stof_train_espcn_in_wgrad   dw (64,1,5), db (64) = out_scale * gradient from g1 (1 - h1^2) and x
 *   stof_train_espcn_in_dgrad   dx = out_scale * conv1^T(g1 (1 - h1^2))
 * The weight gradients add per-group partials from `workspace` (the *_workspace_bytes query) in a fixed order: no float
 * atomics, two runs are bitwise equal.  STOF_ERR_BAD_ARG on NULL or r outside 1..64, STOF_OK on an empty batch (dw / db
 * zeroed), STOF_ERR_UNSUPPORTED where N L 64 reaches 2^31.                                                               */
size_t stof_train_espcn_repack_floats(void);
int stof_train_espcn_repack(const float* w2, float* out, void* stream);
int stof_train_espcn_in(const float* x, const float* w, const float* b, float* h1, int64_t N, int64_t L, void* stream);
int stof_train_espcn_mid(const float* h1, const float* frag2, const float* b2, float* h2, int64_t N, int64_t L, void* stream);
int stof_train_espcn_out(const float* h2, const float* w, const float* b, float* y, int64_t N, int64_t L, int32_t r,
                         void* stream);
size_t stof_train_espcn_out_wgrad_workspace_bytes(int32_t r);
int stof_train_espcn_out_wgrad(const float* h2, const float* y, const float* dy, float* dw, float* db, int64_t N, int64_t L,
                               int32_t r, float out_scale, void* workspace, size_t workspace_bytes, void* stream);
int stof_train_espcn_out_dgrad(const float* y, const float* dy, const float* h2, const float* w, float* g2, int64_t N,
                               int64_t L, int32_t r, void* stream);
size_t stof_train_espcn_in_wgrad_workspace_bytes(void);
int stof_train_espcn_in_wgrad(const float* x, const float* g1, const float* h1, float* dw, float* db, int64_t N, int64_t L,
                              float out_scale, void* workspace, size_t workspace_bytes, void* stream);
int stof_train_espcn_in_dgrad(const float* g1, const float* h1, const float* w, float* dx, int64_t N, int64_t L,
                              float out_scale, void* stream);
/* SemiGlobalBlock pieces (models/stofnet.py:103,108-115), channel-last: MaxPool1d(scale, scale) with arg-max
 * (scale = sample_scale <= 256, P = floor(L / scale) windows), its routing backward (times lrelu' of the pre-pool
 * activation), nearest upsample x scale + pad (rem_half = (L - P*scale) / 2 on each side) + add and its backward.
 * ABI 3: `scale` is an argument (ABI 2 fixed it at 80, the value of every shipped checkpoint).             */
int stof_train_pool(const float* c, float* pooled, uint8_t* arg, int64_t N, int64_t L, int64_t P, int32_t C,
                    int32_t scale, void* stream);
/* pool backward: `c` (the pre-pool activation) may be NULL when `pooled` is given -- the activation at the arg-max IS the
 * pooled value, which is all the leaky-ReLU derivative needs (the fused forward below never materialises c). */
int stof_train_pool_bwd(const float* gpool, const uint8_t* arg, const float* c, const float* pooled, float* gc, int64_t N,
                        int64_t L, int64_t P, int32_t C, int32_t scale, void* stream);

/* Data gradient of conv_last (64 -> r channels, k3) on the vector pipe, exact fp32: out[N, L, 64] from dz[N, L, r] and
 * conv_last.weight in torch layout [r][64][3] = what stof_train_conv computes with the repacked data-gradient weights.
 * r = 4 or 10; otherwise STOF_ERR_UNSUPPORTED.  `out` is written with 16-byte stores and must be 16-byte aligned (else
 * STOF_ERR_BAD_ARG, here and in stof_train_conv_last_dgrad_split); dz and weight are read float by float: any fp32 pointer.  */
int stof_train_conv_last_dgrad(const float* dz, const float* weight, float* out, int64_t N, int64_t L, int32_t r, void* stream);

/* SemiGlobalBlock backward, contract_conv's weight / bias gradient straight from the pool's SPARSE gradient (one non-zero
 * row per (waveform, window, channel)): dw[C][64][5], db[C] = out_scale * the gradient that stof_train_pool_bwd +
 * stof_train_wgrad(a1, gc, cin 64, cout C, K 5) produce, without the dense [N, L, C] tensor.  gpool / arg / pooled[N, P, C]
 * as for stof_train_pool_bwd, a1[N, L, 64] the convolution's input.  STOF_ERR_UNSUPPORTED when C is not a multiple of 128
 * or scale > 92 (the caller then takes the dense route).                                                            */
/* ... and its data gradient: out[N, L, 64] = resid (may be NULL) + conv_transpose(gc, weight[C][64][5]) = what
 * stof_train_pool_bwd + the data-gradient stof_train_conv produce, from the same sparse inputs, in a fixed summation
 * order.  workspace: stof_train_sgb_dgrad_workspace_bytes(C) bytes.  STOF_ERR_UNSUPPORTED when C is not a multiple of 64,
 * C > 512, scale > 88, scale < 4 or P == 0.                                                                          */
size_t stof_train_sgb_dgrad_workspace_bytes(int32_t C);
int stof_train_sgb_contract_dgrad(const float* gpool, const uint8_t* arg, const float* pooled, const float* weight,
                                  const float* resid, float* out, int64_t N, int64_t L, int64_t P, int32_t C, int32_t scale,
                                  void* workspace, size_t workspace_bytes, void* stream);
size_t stof_train_sgb_wgrad_workspace_bytes(int32_t C);
int stof_train_sgb_contract_wgrad(const float* gpool, const uint8_t* arg, const float* pooled, const float* a1, float* dw,
                                  float* db, int64_t N, int64_t L, int64_t P, int32_t C, int32_t scale, float out_scale,
                                  void* workspace, size_t workspace_bytes, void* stream);
/* Training forward of the SemiGlobalBlock's contracting path at sample_scale 80, split-fp16: relu(conv1) -> contract_conv ->
 * lrelu -> MaxPool1d(80) fused as in inference (models/stofnet.py:45,100-103; the [N, L, 512] activation never reaches HBM):
 * pooled[N][P][512] and arg[N][P][512] = row offset of each window's FIRST maximum (torch's max_pool1d backward routing).
 * The four parameter tensors are device pointers; blob_dev = stof_train_sgb_blob_bytes() bytes of scratch the call packs. */
size_t stof_train_sgb_blob_bytes(void);
int stof_train_sgb_contract_pool(const float* conv1_w, const float* conv1_b, const float* contract_w, const float* contract_b,
                                 void* blob_dev, const float* x, float* pooled, uint8_t* arg, int64_t N, int64_t L, void* stream);
int stof_train_upsample_add(const float* a, const float* e, float* out, int64_t N, int64_t L, int64_t P,
                            int32_t rem_half, int32_t scale, void* stream);
/* The same for rows of C channels (any C >= 1): the standalone SemiGlobalBlock (models/stofnet.py:80) takes any width. */
int stof_train_upsample_add_c(const float* a, const float* e, float* out, int64_t N, int64_t L, int64_t P,
                              int32_t rem_half, int32_t scale, int32_t C, void* stream);
int stof_train_upsample_bwd(const float* g, const float* e, float* ge, int64_t N, int64_t L, int64_t P,
                            int32_t rem_half, int32_t scale, void* stream);
/* The same for rows of C channels (any C >= 1): ge[N][P][C] = lrelu'(e) * the sum of g[N][L][C] over each window, taken in
 * a fixed order.  STOF_ERR_UNSUPPORTED where N L exceeds 2^31.                                                            */
int stof_train_upsample_bwd_c(const float* g, const float* e, float* ge, int64_t N, int64_t L, int64_t P,
                              int32_t rem_half, int32_t scale, int32_t C, void* stream);
/* Training forward on the fused sweep (split-fp16 mode; main.py:221 with the model in train mode): conv2 .. conv12 +
 * conv_last of models/stofnet.py:51-65 in ONE launch of the inference body sweep, which additionally writes every layer's
 * output to HBM for the backward pass -- instead of twelve stof_train_conv launches.
 *   stof_train_sweep_pack : device-side packing of the CURRENT parameters (26 device pointers in stof_pack_weights order:
 *                           conv1.weight, conv1.bias, conv2.weight, ..., conv12.bias, conv_last.weight, conv_last.bias) into
 *                           the sweep's operand blob (stof_train_sweep_blob_bytes); no host copy of the weights
 *   stof_train_sweep      : x[N][L] fp32; sgb_expand[N][floor(L/80)][64] = lrelu(expand_conv(pooled)) (stof_train_conv's
 *                           output on the pooled grid; NULL for semi_global_scale 1); dump = stof_train_sweep_dump_floats
 *                           floats: 12 channel-last tensors [N][L][64] (0: relu(conv1)+SemiGlobalBlock, 1..10: outputs of
 *                           conv2..conv11 after their leaky ReLU / residual add, 11: conv12's) + a scratch tail;
 *                           y[N][L*r] = the sample-shuffled prediction.  semi_global_scale 1 or 80 only.                  */
size_t stof_train_sweep_blob_bytes(const stof_net_desc* desc);
int stof_train_sweep_pack(const stof_net_desc* desc, const float* const* params_dev, void* blob_dev, void* stream);
size_t stof_train_sweep_dump_floats(int64_t N, int64_t L);
int stof_train_sweep(const stof_net_desc* desc, const void* blob_dev, const float* x, const float* sgb_expand, float* dump,
                     float* y, int64_t N, int64_t L, void* stream);
/* stof_train_sweep with dump tensors 0..10 written as SPLIT ROWS (see stof_train_wgrad_batch_split); tensor 11 (conv12's output,
 * read by conv_last's weight gradient) stays fp32.  STOF_ERR_UNSUPPORTED when the two-pass sweep kernel is switched off.  */
int stof_train_sweep_split(const stof_net_desc* desc, const void* blob_dev, const float* x, const float* sgb_expand, float* dump,
                           float* y, int64_t N, int64_t L, void* stream);
/* The data-gradient chain of the same step as ONE backward sweep (the mirror image of stof_train_sweep): from
 * g6[N][L][64] = dL/d(conv12 output) (= stof_train_conv of conv_last's transposed weights on dL/dpred) it runs conv12^T,
 * conv11^T .. conv2^T with the leaky-ReLU derivatives (read off the sign of the saved activations in fwd_dump = the dump
 * stof_train_sweep wrote) and the residual additions of models/stofnet.py:51-62 reversed, and writes every layer's output for the weight-gradient
 * kernels: dump tensor j (1..11; stof_train_sweep_dump_floats) = output of sweep layer j = conv(13-j)^T: j odd: dL/dx_k with
 * k = (11-j)/2 (before the long-skip term), j even: dL/d(conv(12-j) output before its leaky ReLU).  blob: the eleven
 * conv2..conv12 weights (device pointers, forward order) packed on the device by stof_train_sweep_bwd_pack into
 * stof_train_sweep_blob_bytes bytes.                                                                                   */
int stof_train_sweep_bwd_pack(const float* const* conv_weights_dev, void* blob_dev, void* stream);
int stof_train_sweep_bwd(const stof_net_desc* desc, const void* blob_dev, const float* g6, const float* fwd_dump,
                         float* dump, int64_t N, int64_t L, void* stream);
/* Loss of main.py:228-232: target = amplitude * blur7(coords2mask(gt)) / max, loss = MSE + lambda * mean|pred|;
 * writes target[N*M], tmax[1], dpred[N*M] = grad_scale * dloss/dpred and loss[1] (double).  grad_scale is a power
 * of two (loss scaling: keeps the back-propagated values inside the fp16 range of the f16x3 mode); the weight-
 * gradient entry points undo it with out_scale = 1/grad_scale, both exactly.                           */
int stof_train_loss(const float* pred, const int64_t* gt_idx, int64_t G, const float* taps7, int64_t N, int64_t M,
                    float amplitude, float lambda, float grad_scale, float* target, float* tmax, float* dpred,
                    double* loss, void* stream);
/* The two halves of stof_train_loss: target[N*M] = blur7(coords2mask(gt)) and its maximum tmax[0]; then the loss and
 * dpred from (pred, target, tmax).  A batch sharded over ranks MAX-all-reduces tmax in between, because the reference
 * normalises by the maximum over the WHOLE batch (main.py:230).                                                    */
int stof_train_loss_target(const int64_t* gt_idx, int64_t G, const float* taps7, int64_t N, int64_t M,
                           float* target, float* tmax, void* stream);
int stof_train_loss_grad(const float* pred, float* target, const float* tmax, int64_t N, int64_t M, float amplitude,
                         float lambda, float grad_scale, float* dpred, double* loss, void* stream);
/* stof_train_sweep_bwd on a forward dump written by stof_train_sweep_split (the leaky-ReLU derivative is read off the sign of the
 * saved activation's hi half: an activation with |y| < 2^-25 counts as not positive), all eleven output tensors as split rows;
 * g6 is a split-row tensor too (stof_train_conv_last_dgrad_split or stof_train_to_split_rows).                              */
int stof_train_sweep_bwd_split(const stof_net_desc* desc, const void* blob_dev, const float* g6, const float* fwd_dump,
                               float* dump, int64_t N, int64_t L, void* stream);
/* fp32 rows in[rows][64] -> split rows out (conv12's output gradient g6, so that every operand of
 * stof_train_wgrad_batch_split is split: that case runs on the global_load_lds kernel).                                   */
int stof_train_to_split_rows(const float* in, float* out, int64_t rows, void* stream);
/* out[rows][64] = (hi + lo of the split rows a_split) + b  (the long-skip join on the backward sweep's split-row dL/dx_0).  */
int stof_train_add_split(const float* a_split, const float* b, float* out, int64_t rows, void* stream);
/* The same with b a split-row tensor as well.                                                                              */
int stof_train_add_split2(const float* a_split, const float* b_split, float* out, int64_t rows, void* stream);
/* stof_train_conv_last_dgrad with out written as split rows: the g6 operand of stof_train_sweep_bwd_split (which expects its g6
 * as split rows) and of stof_train_wgrad_batch_split, which both need it 16-byte aligned: a misaligned `out` is
 * STOF_ERR_BAD_ARG.                                                                                                        */
int stof_train_conv_last_dgrad_split(const float* dz, const float* weight, float* out, int64_t N, int64_t L, int32_t r, void* stream);
/* out = a + b (gradient joins of the residual / long-skip branches, models/stofnet.py:56,62).         */
int stof_train_add(const float* a, const float* b, float* out, int64_t n, void* stream);
/* torch.optim.AdamW step on one flat parameter vector (main.py:179,248).                             */
int stof_train_adamw(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                     float beta1, float beta2, float eps, float weight_decay, int64_t step, void* stream);
/* The same step behind the range guard of the split-fp16 training arithmetic (the reference trains in plain fp32,
 * main.py:221-248): one scan of the gradient bucket (and of *loss, if given) for non-finite values, then AdamW -- if the scan
 * found one, the gradients count as zero (and are zeroed) and guard_words[1] is raised (sticky; the caller reads and clears
 * it whenever it likes).  guard_words: two device ints owned by the caller, zero before the first step; guard_words[0] is
 * scratch (the number of the last bad step).  Two launches, no host read.                                              */
int stof_train_adamw_guarded(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                             float beta1, float beta2, float eps, float weight_decay, int64_t step, const double* loss,
                             int32_t* guard_words, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* STOFNET_AMD_H */
