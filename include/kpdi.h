/* kpdi.h - C ABI of libkpdi.so, the MI355X (gfx950) dictionary-indexing engine.
 *
 * This is the drop-in boundary for ONE path of kikuchipy (reference =
 * /root/reference, paths below relative to its src/kikuchipy/):
 *
 *   EBSD.dictionary_indexing()            signals/ebsd.py:1827-1984
 *     -> _dictionary_indexing()           indexing/_dictionary_indexing.py:36-169
 *        -> SimilarityMetric.prepare_*()  indexing/similarity_metrics/_normalized_cross_correlation.py:88-159
 *                                         indexing/similarity_metrics/_normalized_dot_product.py:80-194
 *        -> SimilarityMetric.match()      ..._normalized_cross_correlation.py:161-183
 *        -> argtopk/topk + merge          indexing/_dictionary_indexing.py:172-203, :94-128
 *   EBSD.remove_static_background()       signals/ebsd.py:442-573   + pattern/_pattern.py:392-435, :484-509, :96-111
 *   EBSD.remove_dynamic_background()      signals/ebsd.py:575-696   + pattern/_pattern.py:438-481, :604-631,
 *                                         filters/fft_barnes.py:29-177
 *
 * The reference has no FFI for this path (it is pure Python + NumPy/Dask/Numba);
 * these entry points are what a ctypes binding inside a kikuchipy
 * `SimilarityMetric` subclass calls (INTEGRATION.md shows that binding).
 *
 * Conventions
 *  - plain C: pointers + sizes, no C++ or torch types; every function returns
 *    0 on success or a negative KPDI_E* code, and kpdi_last_error() returns
 *    the message for the calling thread's last failure.
 *  - one context (kpdi_ctx) = one GPU = one HIP stream; one OS thread drives a context.  Several GPUs from ONE
 *    thread of ONE process: a kpdi_group (below) - the kpdi_create(device_ids*, n_dev, &ctx) of SURVEY.md 8(b).
 *  - the caller owns all host buffers; the library owns all device buffers.
 *  - host inputs are never modified (tests/test_indexing/test_dictionary_indexing.py:41-43).
 *  - masks follow the reference: nonzero = EXCLUDED (similarity_metrics/_similarity_metric.py:51-58).
 *  - there is no CPU fallback: without a usable GPU kpdi_create() fails.
 *
 * Degenerate patterns
 *  A pattern whose normalisation is undefined is DEGENERATE:
 *    ncc - a CONSTANT pattern (a dead or saturated detector frame): all kept pixels EQUAL.  The test is exact (minimum
 *          == maximum of the pixels as read, after the cast to the compute dtype's float32) - there is no contrast floor:
 *          uint16 data around 60 000 counts with ONE pixel of 3600 off by one count is an ordinary pattern and correlates
 *          as in the reference (tests/test_gpu_degenerate.py::test_no_contrast_floor);
 *    ndp - all kept pixels zero;
 *    either metric - NaN or +-inf among the kept pixels, or a sum of squares that is not a positive finite float32
 *          (overflow; differences so small that their squares underflow).
 *  The verdict is the float32 one in EVERY arithmetic: KPDI_COMPUTE_F64 rescores in double from the raw patterns but asks
 *  of each pattern what the float32 screen asked (csrc/rescore.hip: f32_degenerate) - a float64 pattern whose contrast is
 *  below float32 resolution (1 + 1e-10 u), or whose centred squares overflow (1e25 u) or underflow (1e-30 u) float32, is
 *  degenerate there too, although its double arithmetic is ordinary.  Otherwise it would score 0 where the screen decides
 *  what is rescored and a real score where a chunk is small enough to be rescored completely
 *  (tests/test_gpu_rescore.py::test_the_float32_verdict_holds_whatever_the_chunk_size).
 *  The reference divides 0 by 0 there (similarity_metrics/_normalized_cross_correlation.py:228-233,
 *  _normalized_dot_product.py:181-194): the prepared row is NaN, every score of it is NaN, and Dask's topk ranks NaN
 *  FIRST (dask/array/chunk.py:167-258) - a degenerate dictionary pattern becomes every experimental pattern's best
 *  match, a degenerate experimental pattern gets arbitrary indices with NaN scores.  SURVEY.md 8(a) puts that out
 *  of contract; THIS library's rule, on the experimental and on the dictionary side, in every arithmetic
 *  (KPDI_COMPUTE_*) and independent of chunking, tiling and sharding:
 *    a degenerate pattern is prepared as the ALL-ZERO row, so its score against every pattern is exactly +0.0
 *    ("no correlation") and ranks among the real scores like any other 0 - ties: lower dictionary index first.
 *  Hence a degenerate EXPERIMENTAL pattern comes back with scores 0 and the indices global_start .. of the lowest
 *  dictionary patterns pushed; a degenerate DICTIONARY pattern is selected only where fewer than keep_n real scores
 *  are positive; no other pattern's result changes (tests/test_gpu_degenerate.py, against oracle/kpdi_oracle.py which
 *  states the same rule).  Results never contain NaN.
 */
#ifndef KPDI_H
#define KPDI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kpdi_ctx kpdi_ctx;

/* error codes */
#define KPDI_OK 0
#define KPDI_EINVAL (-1)  /* bad argument / call order */
#define KPDI_EHIP (-2)    /* HIP runtime error */
#define KPDI_ENODEV (-3)  /* no usable GPU */
#define KPDI_ECOMM (-4)   /* RCCL error */
#define KPDI_ENOMEM (-5)
#define KPDI_ETIMEOUT (-6) /* a collective did not complete in time (kpdi_comm_selftest) */

/* similarity metric: "ncc" / "ndp" of EBSD._prepare_metric (signals/ebsd.py:3058-3061) */
#define KPDI_METRIC_NCC 0 /* zero-mean + L2 normalise, then dot product */
#define KPDI_METRIC_NDP 1 /* L2 normalise only, then dot product */

/* element type of a pattern array handed to the library */
#define KPDI_U8 0
#define KPDI_U16 1
#define KPDI_F32 2
#define KPDI_F64 3
#define KPDI_I8 4
#define KPDI_I16 5
#define KPDI_I32 6
#define KPDI_U32 7
#define KPDI_F16 8 /* IEEE half: dictionaries stored at half the bytes; not for background removal */

/* arithmetic of the match kernel */
#define KPDI_COMPUTE_F32 0 /* exact f32 MFMA (v_mfma_f32_32x32x2_f32), f32 accumulate: the default */
/* OPT-IN: every prepared value v is held as two f16, 2^12 v = hi + lo (22 significant bits),
 * and a product is hi.hi + hi.lo + lo.hi on v_mfma_f32_32x32x16_f16 with f32 accumulation.
 * Scores differ from the f32 path by a few 1e-7 (the reference's own sgemm differs from exact
 * arithmetic by as much); inside the 1e-5 contract, not bit-identical to KPDI_COMPUTE_F32. */
#define KPDI_COMPUTE_F16X2 1
/* OPT-IN, REDUCED PRECISION (the "fp16 MFMA, fp32 accumulate" variant BASELINE.json configs[4]
 * names): every prepared value is ONE f16 (2^12 v rounded to 11 significant bits), one
 * v_mfma_f32_32x32x16_f16 per 16 pixels, f32 accumulation.  The rounding errors of the 2 K
 * operands of a score average out: measured against the f32 path at K = 3600, max 2e-5 / mean
 * 4e-6 - OUTSIDE the 1e-5 contract, and near-ties rank differently (1.3 % of the best-20 entries
 * of a random dictionary); a few 1e-4 for small K. */
#define KPDI_COMPUTE_F16 2
/* FLOAT64 ARITHMETIC (the reference's `dtype=float64`, _similarity_metric.py:244-253): scores are those of a
 * float64 evaluation (to ~1e-15; summation order differs from a dgemm's), returned by kpdi_finalize_f64.  The
 * KPDI_COMPUTE_F32 path screens keep_n + 12 candidates per pattern and chunk, csrc/rescore.hip rescores them in
 * double from the RAW patterns, keeps the best keep_n in double and checks that no unscreened candidate can
 * belong to them: an unscreened candidate's float32 score is at most the last screened one's, and its float64
 * score at most eps above its float32 score.  eps = the worst-case error of a K-term float32 dot product of unit
 * vectors, (K + 2) 2^-24 (2.1e-4 at K = 3600): a certificate that holds for ANY data - the default since round 5 (the
 * gap between the keep_n-th and the last screened score is an order of magnitude wider on ordinary data, so the proof
 * costs no extra pass: profiles/r05_f64_bounds.txt, also on an adversarial near-tie set).  KPDI_F64_EPS=statistical in
 * the environment selects round 4's bound instead: 8 x the largest |f32 - f64| difference seen among the rescored pairs
 * of the sweep, at least 1e-6 (about 1e5 samples per chunk, drawn from the best-scoring pairs) - fewer passes where
 * scores are closer than the worst case, no proof.  Where the check fails more screening passes run;
 * kpdi_counters.uncertified_patterns counts what is left (0 in every test and stress case).  Needs the
 * raw chunk: not available for resident (held) dictionaries. */
#define KPDI_COMPUTE_F64 3

/* background operations (`operation=` of remove_*_background) */
#define KPDI_OP_SUBTRACT 0
#define KPDI_OP_DIVIDE 1
/* `filter_domain=` of remove_dynamic_background (signals/ebsd.py:652-672) */
#define KPDI_DOMAIN_FREQUENCY 0 /* Barnes FFT filter == edge-replicating correlation */
#define KPDI_DOMAIN_SPATIAL 1   /* scipy.ndimage.gaussian_filter (reflect boundary) */

/* ---- library / device ---------------------------------------------------- */
const char *kpdi_version(void);
int kpdi_device_count(void);
/* message of the last failed call made by the CALLING THREAD (thread-local storage: contexts
 * driven from different threads never see each other's errors; valid until that thread's next call) */
const char *kpdi_last_error(void);

int kpdi_create(int device_id, kpdi_ctx **out);
int kpdi_destroy(kpdi_ctx *ctx);
int kpdi_synchronize(kpdi_ctx *ctx);

/* ---- problem set-up -------------------------------------------------------
 * Fixes what SimilarityMetric carries (similarity_metrics/_similarity_metric.py:69-86):
 * detector shape, signal mask (sy*sx bytes or NULL), metric and keep_n
 * (`keep_n = min(keep_n, dictionary_size)` is the caller's job,
 * indexing/_dictionary_indexing.py:67).  Resets the running top-k. */
int kpdi_set_problem(kpdi_ctx *ctx, int sy, int sx, const uint8_t *signal_mask,
                     int metric, int compute_dtype, int keep_n);

/* change keep_n only (forgets the running best-k, keeps everything else) */
int kpdi_set_keep_n(kpdi_ctx *ctx, int keep_n);

/* ---- experimental patterns (prepare_experimental, ..._cross_correlation.py:88-128)
 * `patterns`: m_all x sy x sx, C order, HOST memory.  `nav_mask`: m_all bytes or
 * NULL.  Uploads the raw patterns; they stay resident (and can be pre-processed
 * in place with kpdi_remove_*_background) until the first dictionary chunk is
 * pushed, when they are cast/masked/normalised once into the K-padded f32
 * matrix the match kernel reads. */
int kpdi_set_experimental(kpdi_ctx *ctx, const void *patterns, int dtype,
                          int64_t m_all, const uint8_t *nav_mask);
/* same, `patterns` already in DEVICE memory (copied device-to-device) */
int kpdi_set_experimental_dev(kpdi_ctx *ctx, const void *d_patterns, int dtype,
                              int64_t m_all, const uint8_t *nav_mask);
/* number of patterns that will be matched (nav mask applied) */
int64_t kpdi_n_experimental(kpdi_ctx *ctx);

/* ---- pre-processing of the resident experimental patterns -------------------
 * Both calls RECORD their step (arguments are validated and copied before they return); the
 * kernels run when the patterns are needed: fused with the metric's preparation of the
 * patterns into ONE kernel (static -> truncate -> dynamic -> truncate -> signal-mask gather ->
 * normalise -> tiled matrix; detectors up to 19 200 pixels, streaming kernels above that)
 * at the first dictionary chunk, or on their own in kpdi_get_experimental.  One static step
 * followed by one dynamic step fuse; any other sequence runs step by step.  Results are
 * identical either way: every step sees the truncated output of the previous one.
 * remove_static_background: pattern/_pattern.py:392-435 (+ :484-509, :96-111).
 * `static_bg`: sy*sx float32 (the caller did `static_bg.astype(float32)`,
 * signals/ebsd.py:547).  Output keeps the input dtype, truncated like `.astype`. */
int kpdi_remove_static_background(kpdi_ctx *ctx, const float *static_bg,
                                  int operation, int scale_bg);
/* remove_dynamic_background: pattern/_pattern.py:438-481; std <= 0 selects the
 * reference default sx/8 (signals/ebsd.py:648-649). */
int kpdi_remove_dynamic_background(kpdi_ctx *ctx, int operation, int filter_domain,
                                   double std, double truncate);
/* copy the (pre-processed) resident patterns back: m_all*sy*sx elements of the
 * dtype given to kpdi_set_experimental */
int kpdi_get_experimental(kpdi_ctx *ctx, void *patterns_out);

/* ---- image quality (EBSD.get_image_quality, signals/ebsd.py:1312-1375; pattern/_pattern.py:698-775) ------------
 * Krieger Lassen's Q of every resident pattern, AFTER the recorded background steps (they run first, as in
 * kpdi_get_experimental); the navigation mask is ignored.  `weights`: sy*sx float64 frequency vectors, NULL = the
 * reference's fft_frequency_vectors((sy, sx)); `inertia_max` <= 0: sum(weights) / (sy*sx).  `iq_out`: m_all floats,
 * NaN for a pattern with a non-finite value, a constant pattern with `normalize`, or an all-zero one.  uint8 / int8 /
 * uint16 / int16 / float32 / float64 patterns; kernels and paths: csrc/iq.hip, csrc/iq_plan.h. */
int kpdi_image_quality(kpdi_ctx *ctx, int normalize, const double *weights, double inertia_max, float *iq_out);

/* ---- sums over detector rectangles (EBSD.get_virtual_bse_intensity, signals/ebsd.py:1555-1598; imaging/vbse.py) ----
 * np.nansum of every resident pattern over `n_rects` rectangles, AFTER the recorded background steps (they run first,
 * as in kpdi_get_experimental); the navigation mask is ignored and the patterns are only read - once, whatever
 * `n_rects`.  `rects`: n_rects x (row0, row1, col0, col1), half-open, 0 <= row0 <= row1 <= sy and 0 <= col0 <= col1 <= sx;
 * rectangles may overlap, an empty one sums to 0.  `sums_out`: m_all * n_rects values, pattern-major: uint64 for uint8 /
 * uint16 patterns and int64 for int8 / int16 (exact), float32 for float32 and float64 for float64 patterns (summed in
 * float64 in a fixed order, NaN counted as 0, rounded once).  n_rects == 0 does nothing; a bad argument gives
 * KPDI_EINVAL before anything runs.  Kernels and paths: csrc/regionsum.hip, csrc/regionsum_plan.h. */
int kpdi_region_sums(kpdi_ctx *ctx, const int32_t *rects, int n_rects, void *sums_out);

/* ---- axis reductions (EBSD.sum / mean / max / min / std / var: HyperSpy's BaseSignal methods) ------------------------
 * Reduces the resident patterns, taken as the C-contiguous array (ny, nx, sy, sx) with ny * nx == m_all, over the axes
 * of `axis_mask` (bit k: array axis k; 1 ... 15), AFTER the recorded background steps (they run first, as in
 * kpdi_get_experimental); the navigation mask is ignored and the patterns are only read.  `out`: the kept axes in
 * order, C-contiguous, of NumPy's result dtype -
 *   KPDI_REDUCE_SUM: uint64 (uint8 / uint16 patterns), int64 (int8 / int16), float32, float64;
 *   KPDI_REDUCE_MEAN / STD / VAR: float64 for integer patterns, else the patterns' dtype (no ddof);
 *   KPDI_REDUCE_MAX / MIN: the patterns' dtype -
 * and `out_bytes` its size, which is checked.  Integer sums are exact (64-bit); std / var of integers come from the exact
 * sums of x and x^2; float patterns are accumulated in float64 in a fixed order and rounded once (std / var: in two
 * passes, about the mean); NaN propagates through every op.  The same call gives the same bits.  A bad argument gives
 * KPDI_EINVAL before anything runs and leaves the context as it was.  Kernels and plan: csrc/reduce.hip,
 * csrc/reduce_plan.h. */
#define KPDI_REDUCE_SUM 0
#define KPDI_REDUCE_MEAN 1
#define KPDI_REDUCE_MAX 2
#define KPDI_REDUCE_MIN 3
#define KPDI_REDUCE_STD 4
#define KPDI_REDUCE_VAR 5
int kpdi_reduce_experimental(kpdi_ctx *ctx, int op, int axis_mask, int ny, int nx, void *out, size_t out_bytes);
/* The plan such a call follows, without a context: desc[0 ... 16] = regime (0: the inner axis survives, 1: contiguous
 * runs are reduced), A, R1, M, R2, B of in[A][R1][M][R2][B] -> out[A][M][B], slice, slices, vector elements, lanes per
 * output, grid x, grid y, passes, planes, workspace bytes, result bytes, lanes per output of the combine kernel.
 * KPDI_EINVAL for what the call would refuse. */
int kpdi_reduce_plan_describe(int dtype, int op, int axis_mask, int ny, int nx, int sy, int sx, int64_t *desc);

/* ---- FFT filter (EBSD.fft_filter, signals/ebsd.py:805-930; pattern/chunk.py:75-127) ------------------------------
 * Filters every resident pattern in place, AFTER the recorded background steps (they run first), and rescales it to
 * the range of its dtype as the reference's rescale_intensity(dtype_out=<dtype>) does; the navigation mask is ignored
 * and prepared rows made before the call are invalidated.
 * KPDI_DOMAIN_FREQUENCY: `table` is the folded half spectrum of the transfer function, ty = sy rows of
 *   tx = sx / 2 + 1 complex values stored as (re, im) float64 pairs: Hs(k, l) = (H'(k, l) + conj(H'(-k, -l))) / 2 with
 *   H' the transfer function as applied to the unshifted spectrum (ifftshift(H) for shift=True).
 * KPDI_DOMAIN_SPATIAL: `table` is a ty x tx float64 kernel, applied as Barnes' FFT filter does: a correlation with
 *   edge-replicated borders centred at (ty / 2, tx / 2).
 * A pattern holding a non-finite value, or whose filtered result is constant, becomes 0 (integer dtypes) or NaN (float
 * dtypes).  uint8 / int8 / uint16 / int16 / float32 / float64 patterns; kernels and paths: csrc/fftfilter.hip,
 * csrc/fftfilter_plan.h. */
int kpdi_fft_filter(kpdi_ctx *ctx, int function_domain, const double *table, int ty, int tx);

/* ---- intensity rescaling / normalization (EBSD.rescale_intensity / normalize_intensity,
 * signals/_kikuchipy_signal.py:88-338; pattern/_pattern.py:31-111, :154-210) -----------------------------------------
 * Each call maps every resident pattern, AFTER the recorded background steps (they run first), into `dtype_out`
 * (KPDI_U8 / I8 / U16 / I16 / F32 / F64; the patterns themselves may be any of these).  A new dtype replaces the resident
 * patterns (kpdi_get_experimental then returns `dtype_out`); the navigation mask is ignored and prepared rows made
 * before the call are invalidated.  The arithmetic is the reference's under NumPy 1.26 dtype rules, float64 for integer
 * and float64 patterns, float32 for float32 patterns; casts to integer dtypes truncate to int32 (NaN and values outside
 * int32: INT32_MIN) and keep the low bits, as ndarray.astype does on x86-64.  Kernels and paths: csrc/intensity.hip,
 * csrc/intensity_plan.h.
 * kpdi_rescale_intensity: ((clip(p, imin, imax) - imin) / (imax - imin)) * (omax - omin) + omin with (imin, imax) =
 *   `in_range` (2 doubles; no clip when NULL), else np.nanpercentile(p, `percentiles`) per pattern (2 doubles in
 *   [0, 100]), else the pattern's nanmin / nanmax; in_range and percentiles are exclusive.  Integer patterns are
 *   computed exactly (the reference's int8 / int16 arithmetic can wrap).
 * kpdi_normalize_intensity: (p - mean) / (num_std * std [* sqrt(sy * sx)]) per pattern, sums in float64.
 * kpdi_intensity_range: out[0], out[1] = min and max over all resident patterns (NaN if any value is NaN), for the
 *   reference's relative=True. */
int kpdi_rescale_intensity(kpdi_ctx *ctx, const double *in_range, const double *percentiles, double omin, double omax,
                           int dtype_out);
int kpdi_normalize_intensity(kpdi_ctx *ctx, double num_std, int divide_by_square_root, int dtype_out);
int kpdi_intensity_range(kpdi_ctx *ctx, double *out);

/* ---- adaptive histogram equalization (EBSD.adaptive_histogram_equalization, signals/_kikuchipy_signal.py:340-470;
 * pattern/_pattern.py:810-840: scikit-image 0.18.3's equalize_adapthist, then rescale_intensity to the dtype's range) --
 * Equalizes every resident pattern in place, AFTER the recorded background steps (they run first); the dtype stays,
 * the navigation mask is ignored and prepared rows made before the call are invalidated.  `ky` x `kx`: the kernel
 * (contextual region) in rows x columns, any size >= 1 (larger than the pattern too); `clip_count`: the integer clip
 * limit the reference derives, int(max(clip_limit * ky * kx, 1)) for clip_limit > 0, else ky * kx (no clipping);
 * 1 <= `nbins` <= 16384.  Float patterns are taken as the reference takes values in [-1, 1] (the caller checks the
 * range; values outside are clipped, NaN counts as 0).  Bit-exact with the reference under NumPy 1.26; kernels and
 * paths: csrc/clahe.hip, csrc/clahe_plan.h.  KPDI_EINVAL where no path takes the shape, kernel and bins. */
int kpdi_adaptive_histogram_equalization(kpdi_ctx *ctx, int ky, int kx, int clip_count, int nbins);

/* ---- neighbour pattern averaging and neighbour dot products (EBSD.average_neighbour_patterns, signals/ebsd.py:943-1111,
 * pattern/chunk.py:130-164; EBSD.get_neighbour_dot_product_matrices / get_average_neighbour_dot_product_map,
 * signals/ebsd.py:1221-1491, signals/util/_map_helper.py) --------------------------------------------------------------
 * The two ops whose result at a map point depends on the patterns around it.  The resident patterns are taken as a map
 * of `ny` rows of `nx` points, row-major, ny * nx = the resident pattern count (a 1-D map: nx = 1 and a window of
 * wy x 1); the navigation mask is ignored; both run AFTER the recorded background steps.  The window has `wy` x `wx`
 * entries with its origin at (wy / 2, wx / 2), also for even sizes; a neighbour outside the map does not exist (it adds
 * 0 to an average and is NaN in a dot product matrix).  Output is produced for the rows [row0, row1) only; the other
 * resident rows serve as neighbours, so that a map can be split by rows over several contexts, each holding its rows
 * plus a halo of wy / 2 rows above and wy - wy / 2 - 1 below (clipped at the map's edge) - the results then equal
 * those of one context bit for bit.  Errors are KPDI_EINVAL before any launch.  Kernels: csrc/neighbours.hip.
 * kpdi_average_neighbour_patterns: per point q, c = float32(sum_j window[j] * float32(p_{q+j})) accumulated in float64
 *   over the non-zero coefficients in C order; a = float64(c) / window_sums[q]; the pattern (a - min a) / (max a -
 *   min a) * (omax - omin) + omin in float64 with the dtype's range, truncated (integer dtypes) or rounded (float
 *   dtypes) to the patterns' dtype, which stays.  `window_sums`: ny * nx integers, the reference's truncated window sum
 *   of every resident point, computed by the caller from the WHOLE map (never from the rows held here); 0 for a point
 *   in [row0, row1) is refused.  A constant averaged pattern becomes 0 (integer dtypes) or NaN (float dtypes), as in
 *   kpdi_rescale_intensity.  The averaged patterns replace the resident ones (rows outside [row0, row1) keep theirs)
 *   and prepared rows made before the call are invalidated.
 * kpdi_neighbour_dot_products: `footprint`: wy * wx bytes, non-zero = the neighbour takes part; it must be true at its
 *   origin.  Every pattern as float64, minus its mean (`zero_mean`), divided by sqrt(sum x^2) (`normalize`, after the
 *   centring); dp[q, j] = x_{q+j} . x_q, accumulated in float64.  `matrices_out` (or NULL): (row1 - row0) * nx * wy * wx
 *   values, NaN where the footprint is false or the neighbour is outside the map, sum x_q^2 at the origin; `map_out`
 *   (or NULL): (row1 - row0) * nx values, the mean of the point's non-NaN dot products with its neighbours, NaN without
 *   any.  Both are float64 for `f64`, else float32, and come from the same launch.  A pattern of zero norm under
 *   `normalize` or one holding a NaN gives NaN dot products.  The patterns are only read. */
int kpdi_average_neighbour_patterns(kpdi_ctx *ctx, int ny, int nx, const double *window, int wy, int wx,
                                    const int64_t *window_sums, int row0, int row1);
int kpdi_neighbour_dot_products(kpdi_ctx *ctx, int ny, int nx, const uint8_t *footprint, int wy, int wx, int zero_mean,
                                int normalize, int f64, int row0, int row1, void *matrices_out, void *map_out);

/* ---- downsampling (EBSD.downsample, signals/ebsd.py:1113-1219; pattern/_pattern.py:776-807) -----------------------
 * Replaces every resident pattern (sy x sx, uint8 / int8 / uint16 / int16 / float32 / float64) by its binned and
 * rescaled image of (sy / factor) x (sx / factor) in `dtype_out` (the same six), AFTER the recorded background steps
 * (they run first, as in kpdi_rescale_intensity).  The reference's _downsample2d as NumPy 1.26 evaluates it: the
 * pattern as float32; every binned pixel the float32 sum of its factor x factor pixels added one by one, rows outer and
 * columns inner; (b - min b) / float32(max b - min b) * (omax - omin) + omin with the range of `dtype_out`, every
 * operation rounded to float32; then the cast of kpdi_rescale_intensity (a float64 `dtype_out` is the float32 result
 * widened).  min / max propagate NaN as np.min / np.max do, so a pattern holding a NaN, like a constant binned pattern
 * (0 / 0), becomes NaN for float `dtype_out` and 0 for integer ones.  Bit-exact with the reference; the result does not
 * depend on the number of patterns or on the kernel path (csrc/downsample.hip, csrc/downsample_plan.h).
 * Afterwards the problem's detector shape is (sy / factor, sx / factor) with no signal mask, the patterns' dtype is
 * `dtype_out` (kpdi_get_experimental returns the new shape and dtype), and prepared rows and the running best-k are
 * forgotten; metric, arithmetic, keep_n and the navigation mask stay.  The binned patterns can be indexed at once.  To
 * index them under a signal mask call kpdi_set_problem with the NEW shape and the mask next: kpdi_set_problem keeps the
 * resident patterns whenever the number of detector pixels is unchanged, so neither that call nor a plain
 * kpdi_set_problem with the new shape loses them.
 * KPDI_EINVAL before anything runs (the resident set stays as it was): factor < 2, a factor that does not divide both
 * sy and sx, a `dtype_out` outside the six, no resident patterns, a signal mask set for the old shape, held dictionary
 * chunks (their layout depends on the shape), or a shape no kernel path takes. */
int kpdi_downsample(kpdi_ctx *ctx, int factor, int dtype_out);

/* ---- the dynamic background itself (EBSD.get_dynamic_background, signals/ebsd.py:698-803; pattern/chunk.py:33-72;
 * pattern/_pattern.py:634-695) ----------------------------------------------------------------------------------------
 * The Gaussian-blurred image of every resident pattern - what kpdi_remove_dynamic_background subtracts or divides
 * away - into `out`: m_all * sy * sx values of `dtype_out` (the six dtypes above) in host memory.  The resident patterns
 * are only read, AFTER the recorded background steps; the navigation mask is ignored; std <= 0 selects sx / 8.  In the
 * reference's order every pattern is cast to `dtype_out` FIRST (the cast of kpdi_rescale_intensity) and then filtered:
 * KPDI_DOMAIN_FREQUENCY: the cast pattern as float32, correlated with the normalised Gaussian window of
 *   int(truncate * std) samples per axis with edge-replicated borders (what the reference's FFT filter computes, here
 *   as two 1-D passes accumulated in float64), rounded to float32 and cast to `dtype_out` (integers truncate).
 * KPDI_DOMAIN_SPATIAL: scipy.ndimage.gaussian_filter(sigma=std, truncate=truncate) of the cast pattern: reflect
 *   boundary, radius int(truncate * std + 0.5), each of the two 1-D passes (rows of the detector last) accumulated in
 *   float64 and stored in `dtype_out`, integers by truncation toward zero - so the second pass sees the quantised
 *   first one.  (kpdi_remove_dynamic_background blurs a float32 copy instead.)
 * KPDI_EINVAL before anything runs: an unknown domain, a window of no samples, a `dtype_out` outside the six, NULL, or a
 * detector above 256 MB of float64 per pattern (5792 x 5792).  Kernel: csrc/preproc.hip (dynamic_background_kernel). */
int kpdi_get_dynamic_background(kpdi_ctx *ctx, int filter_domain, double std, double truncate, int dtype_out, void *out);

/* ---- PCA decomposition and its model (EBSD.decomposition as the reference's multivariate-analysis workflow uses it;
 * EBSD.get_decomposition_model, signals/ebsd.py:2665-2723, signals/util/_dask.py:283-332) --------------------------------
 * All four calls work on the resident patterns (the six dtypes of kpdi_rescale_intensity) AFTER the recorded background
 * steps and ignore the navigation mask.  M is the number of resident patterns, K = sy * sx, X the M x K matrix of the
 * patterns with row-major pixels, every value widened exactly to float64.
 * `centre`: KPDI_CENTRE_NONE; KPDI_CENTRE_NAVIGATION subtracts from every pixel its mean over all patterns (the mean
 * pattern); KPDI_CENTRE_SIGNAL subtracts from every pattern its mean over its pixels.  Means are float64 sums in a fixed
 * order without atomics, divided once (csrc/decomp.hip states the order); xc = double(x) - mean is rounded once, when a
 * tile is staged: the centred matrix Xc is never stored.
 * The products are float64 MFMA tile kernels with one fixed summation order per output: results do not depend on the
 * launch, bit for bit (csrc/decomp.hip, csrc/decomp_plan.h).  The eigen-solve between kpdi_decomposition_gram and
 * kpdi_decomposition_apply is the caller's (kikuchipy_amd/pattern/_decomposition.py: numpy.linalg.eigh).
 *
 * kpdi_decomposition_gram: the Gram matrix of Xc over its shorter side into `gram_out` (host, side * side float64, both
 *   triangles, symmetric bit for bit): K <= M gives Xc^T Xc with *side = K, *transposed = 0; K > M gives Xc Xc^T with
 *   *side = M, *transposed = 1.  `mean_out` (host; may be NULL) receives the M ("signal") or K ("navigation") means.
 *   KPDI_EINVAL: an unknown `centre`, NULL, side = min(M, K) above 8192 (bin the patterns first: kpdi_downsample) - all
 *   before any launch - and patterns that hold non-finite values (the trace is not finite; the outputs are written).
 * kpdi_decomposition_apply: transposed_op 0: out (M x c) = Xc basis (K x c); transposed_op 1: out (K x c) = Xc^T basis
 *   (M x c); host float64, row-major, 1 <= c <= min(M, K).
 * kpdi_decomposition_model: every resident pattern becomes sum_j loadings[m, j] factors[k, j] + mean, accumulated in
 *   float64 and rounded once to `dtype_out` (KPDI_F32 or KPDI_F64 only).  `loadings` (M x c) and `factors` (K x c) are
 *   host arrays of `dtype_out`; `mean` is NULL or host float64: K means per pixel (mean_kind KPDI_CENTRE_NAVIGATION) or M
 *   means per pattern (KPDI_CENTRE_SIGNAL).  As in kpdi_rescale_intensity the patterns take the new dtype and prepared
 *   rows are forgotten.
 * kpdi_change_dtype: ndarray.astype(dtype_out) of the resident patterns with the casts of kpdi_rescale_intensity
 *   (to integers: truncate to int32, NaN and out-of-range values give INT32_MIN, keep the low bits; to float32: round
 *   to nearest); `dtype_out` is one of the six. */
#define KPDI_CENTRE_NONE 0
#define KPDI_CENTRE_NAVIGATION 1
#define KPDI_CENTRE_SIGNAL 2
int kpdi_decomposition_gram(kpdi_ctx *ctx, int centre, double *gram_out, double *mean_out, int64_t *side, int *transposed);
int kpdi_decomposition_apply(kpdi_ctx *ctx, int centre, int transposed_op, const double *basis, int n_components,
                             double *out);
int kpdi_decomposition_model(kpdi_ctx *ctx, const void *loadings, const void *factors, int n_components, const double *mean,
                             int mean_kind, int dtype_out);
int kpdi_change_dtype(kpdi_ctx *ctx, int dtype_out);

/* ---- selecting patterns, rows and columns (EBSD.inav / isig / crop / extract_grid, signals/ebsd.py:267-378; deepcopy) ----
 * kpdi_select_patterns: out[i, r, c] = in[pattern_index[i], row0 + r * row_step, col0 + c * col_step] for i < n_out,
 *   r < n_rows, c < n_cols, on the resident patterns of `src` (the six dtypes of kpdi_rescale_intensity), a byte-exact
 *   copy AFTER the recorded background steps.  `pattern_index` is a host array of n_out entries in [0, m_all), in any order
 *   and with repeats, or NULL for every pattern in order (n_out must then be m_all).
 *   dst == src: the selection replaces the resident patterns; the problem's detector shape becomes (n_rows, n_cols);
 *     prepared rows, the running best-k and the navigation mask are forgotten; metric, arithmetic and keep_n stay, and so
 *     does a signal mask when the shape does not change.
 *   dst != src (same device): `src` is left as it is, its recorded steps stay recorded (they run on dst's copy).  `dst`
 *     receives the patterns and their dtype without a navigation mask, and, unless it already has a problem of the shape
 *     (n_rows, n_cols), that shape with src's metric, arithmetic and keep_n and no signal mask.  With NULL, the whole
 *     detector and steps of 1 this is a device-to-device copy of the set.
 *   KPDI_EINVAL before anything is launched or freed (both resident sets stay as they were): no resident patterns in
 *   `src`, n_out < 1, an index outside [0, m_all), a step < 1, rows or columns that leave the detector, contexts on
 *   different devices, and - when the detector shape of `dst` would change - a signal mask set or dictionary chunks held
 *   there.  Kernel: csrc/select.hip, its three paths: csrc/select_plan.h.
 * kpdi_set_navigation_mask: `nav_mask` (m_all bytes, non-zero = the pattern is not matched; NULL: none) becomes the
 *   navigation mask of the resident patterns, as if it had come with kpdi_set_experimental of the patterns as
 *   kpdi_get_experimental returns them: recorded background steps run first, on their own (not fused into the
 *   preparation of the next sweep), so the scores of that sweep have the bits of a sweep after such an upload; prepared
 *   rows and the running best-k are forgotten. */
int kpdi_select_patterns(kpdi_ctx *src, kpdi_ctx *dst, const int64_t *pattern_index, int64_t n_out, int row0, int row_step,
                         int n_rows, int col0, int col_step, int n_cols);
int kpdi_set_navigation_mask(kpdi_ctx *ctx, const uint8_t *nav_mask);

/* ---- kinematical master pattern in the stereographic projection (KikuchiPatternSimulator.calculate_master_pattern,
 * simulations/kikuchi_pattern_simulator.py:162-199, get_pattern :685-700) ---------------------------------------------------
 * Independent of the resident patterns.  `unit_vectors` (m x 3), `theta` (m Bragg angles, rad) and `intensity` (m) are host
 * float64; `out` is host float64 of (n_hemispheres, size, size), size = 2 half_size + 1, the upper hemisphere first for
 * KPDI_HEMISPHERE_BOTH.  Pixel (row, col) looks along the inverse stereographic projection of x = arr[col], y = arr[row],
 * arr = np.linspace(-1, 1, size): (2x, 2y, 1 - x^2 - y^2) / (1 + x^2 + y^2), z negated on the lower hemisphere; the
 * directions are formed on the host with NumPy's operations one by one (csrc/kinematical_plan.h) and equal them bit for
 * bit.  For every pixel the reflectors are visited in rising index, in float64 without contraction:
 *   D = ((u0 v0) + u1 v1) + u2 v2;  |D| <= 1e-7 adds 0.5 intensity;  otherwise intensity is added when
 *   pi/2 - theta <= acos(D) <= pi/2  (one-sided: D < 0 adds nothing; D > 1 by rounding adds nothing).
 * acos is evaluated only for pairs within 1e-6 in D of the band edge, every other pair falls on the same side whatever the
 * last bits of acos are: a pixel differs from the reference's plain-Python evaluation only where some reflector's acos(D)
 * lies within the last bits of pi/2 - theta.  One thread per pixel, both hemispheres in one launch, no atomics, one
 * summation order: results do not depend on the launch or the reflector chunk, bit for bit (csrc/kinematical.hip).
 * KPDI_EINVAL before anything runs: NULL, m < 1, half_size < 0 or above 4096, an unknown hemisphere code. */
#define KPDI_HEMISPHERE_UPPER 0
#define KPDI_HEMISPHERE_LOWER 1
#define KPDI_HEMISPHERE_BOTH 2
int kpdi_kinematical_master_pattern(kpdi_ctx *ctx, const double *unit_vectors, const double *theta, const double *intensity,
                                    int64_t m, int half_size, int hemispheres, double *out);

/* ---- cubochoric sampling of the fundamental zone of a rotation group (get_sample_fundamental; Rosca, Morawiec &
 * De Graef 2014; Singh & De Graef 2016) -----------------------------------------------------------------------------------
 * Independent of the resident patterns.  The grid has (2 n + 1)^3 points, n = `semi_edge_steps`, over the cube of
 * semi-edge pi^(2/3) / 2, surface included; a point goes cube -> homochoric ball -> axis-angle -> unit quaternion
 * (q0 >= 0, qv), all in float64 (csrc/sampling_plan.h).  `faces` (n_faces x 4, host float64) holds one row
 * (ax, ay, az, tan(omega/4)) per face pair of the zone, a a unit rotation axis of the group and omega the smallest
 * rotation angle about it; a point is kept iff |qv . a| <= tan(omega/4) q0 + 1e-9 for every row (closed: both faces of
 * a pair are kept).  n_faces = 0 keeps every point (the group 1).
 * kpdi_sample_fundamental_count: the number of kept points into `*count`.
 * kpdi_sample_fundamental_fill: the kept quaternions into `out` (capacity x 4, host float64) in lexicographic grid order,
 *   x slowest - the host sampler's order, whatever the launch looks like (per-workgroup counts, a device scan, no atomics:
 *   csrc/sampling.hip) - and their number into `*count`.  After a count call of the same grid and faces on this context
 *   the points are not counted again.  KPDI_EINVAL with `*count` set when `capacity` is smaller than the kept number.
 * KPDI_EINVAL before anything runs: NULL, semi_edge_steps outside [1, 2048], n_faces outside [0, 23], capacity < 0.
 * KPDI_ENOMEM, nothing launched and the context usable, when the per-workgroup counts or the kept quaternions (32 bytes
 * each) exceed the free device memory. */
int kpdi_sample_fundamental_count(kpdi_ctx *ctx, int semi_edge_steps, const double *faces, int n_faces, int64_t *count);
int kpdi_sample_fundamental_fill(kpdi_ctx *ctx, int semi_edge_steps, const double *faces, int n_faces, double *out,
                                 int64_t capacity, int64_t *count);

/* ---- disorientation angles, zone reduction and kernel average misorientation maps (kikuchipy_amd/orientations.py;
 * DESIGN.md section 25; csrc/orientations.hip, csrc/orientations_plan.h) ---------------------------------------------------
 * Independent of the resident patterns, all in float64.  Quaternions are rows (a, b, c, d) of host float64; a row is
 * normalised first, a row whose norm is not a positive finite number gives NaN wherever it enters.  `ops` (n_ops x 4,
 * 1 <= n_ops <= 24) are the proper operations of a rotation group as unit quaternions, the equivalents of g are s g.
 * The disorientation angle of g1 under ops1 and g2 under ops2 is the smallest rotation angle of (s2 g2)(s1 g1)^-1: the
 * candidate (s1, s2) with the largest |(s1 g1) . (s2 g2)| (the lowest s1 n_ops2 + s2 among equal maxima) evaluated again
 * as 2 atan2(|v|, |w|) of that product.  Equal groups: pass ops1 = the identity alone, one side's equivalents suffice.
 * `degrees` != 0 multiplies the angle by 180 / pi.
 * kpdi_orientation_pairs: `count` = prod(shape[0 .. ndim)) angles into `out`; output element (i_0, ..., i_ndim-1), C
 *   order, takes row sum_d i_d stride1[d] of q1 (rows1 x 4) and row sum_d i_d stride2[d] of q2 (rows2 x 4): NumPy
 *   broadcasting as strides, 0 where an input is broadcast.  ndim in [0, 8], every row addressed inside its input.
 * kpdi_orientation_outer: the n x m angles of every row of q1 with every row of q2 into `out` (host, row-major, of
 *   `dtype_out` KPDI_F64 or KPDI_F32: the float64 angle rounded once).  Output that does not fit in half of the free
 *   device memory is walked in passes of rows; KPDI_ORIENT_PASS_ROWS=r in the environment, read at each call, forces
 *   passes of r rows.  The result does not depend on the passes.
 * kpdi_orientation_reduce: per row the equivalent s g with the largest |a| (the lowest s among equal maxima) with a >= 0
 *   (a half turn: its first non-zero component positive) into `out` (n x 4) and s into `index` (n; -1 for a NaN row).
 * kpdi_orientation_kam: per point of a ny x nx map the mean angle to its neighbours at `offsets` (n_offsets x (dy, dx)
 *   int32, in window order; at most 1024), a float64 sum in that order, into `out` (ny x nx).  Left out of the mean:
 *   neighbours outside the map, where `in_data` (ny x nx bytes, or NULL: all in) is 0, and those further than
 *   `max_angle` (radians; negative: no limit).  NaN for a point not in the data or with no neighbour left.
 * KPDI_EINVAL before anything runs: NULL, counts below 1, n_ops outside [1, 24], ndim outside [0, 8], a stride that
 *   leaves its input, a dtype_out other than the two floats, more than 1024 offsets.  KPDI_ENOMEM, nothing launched and
 *   the context usable, when the inputs and one output row (outer) or the whole output (the others) exceed the free
 *   device memory. */
int kpdi_orientation_pairs(kpdi_ctx *ctx, const double *q1, int64_t rows1, const double *q2, int64_t rows2, int ndim,
                           const int64_t *shape, const int64_t *stride1, const int64_t *stride2, const double *ops1,
                           int n_ops1, const double *ops2, int n_ops2, int degrees, double *out);
int kpdi_orientation_outer(kpdi_ctx *ctx, const double *q1, int64_t n, const double *q2, int64_t m, const double *ops1,
                           int n_ops1, const double *ops2, int n_ops2, int degrees, int dtype_out, void *out);
int kpdi_orientation_reduce(kpdi_ctx *ctx, const double *q, int64_t n, const double *ops, int n_ops, double *out,
                            int32_t *index);
int kpdi_orientation_kam(kpdi_ctx *ctx, const double *q, int ny, int nx, const double *ops, int n_ops,
                         const int32_t *offsets, int n_offsets, const uint8_t *in_data, double max_angle, int degrees,
                         double *out);

/* ---- Hough indexing (kikuchipy_amd/indexing/_hough_indexing.py; csrc/hough.hip, csrc/hough_plan.h,
 * csrc/hough_vote.h) ---------------------------------------------------------------------------------------------------
 * kpdi_hough_bands: the Radon transform of every resident pattern (after the recorded background steps; the six pattern
 *   dtypes) and the `n_bands` (1 ... 16) strongest bands of each into `bands_out` (m_all x n_bands records of 32 bytes:
 *   float32 theta [rad], rho [px], value; int32 valid, a, k; float32 da, dk).  A pattern is masked by its inscribed circle
 *   and its masked mean removed; S[a][k] sums it, sampled bilinearly at unit steps, along the line
 *   cos(theta) (j - cx) + sin(theta) (i - cy) = rho, theta = a pi / n_theta, rho = (k - (n_rho - 1) / 2) drho,
 *   drho = 2 floor(R) / (n_rho - 1), R = (min(ny, nx) - 1) / 2, cx = (nx - 1) / 2, cy = (ny - 1) / 2.  `cos_sin` holds
 *   the n_theta cosines, then the n_theta sines, as float32: the caller's table, so that a restatement works from the same
 *   bits.  The sinogram is smoothed along rho (zeros beyond the ends) by the 2 rho_radius + 1 float32 `rho_taps`, then
 *   along theta (the axis wraps with rho flipped) by the 2 theta_radius + 1 `theta_taps` (radii 0 ... 16), `rim` >= 1
 *   cells at either end of the rho axis hold no band, a band is a positive maximum of its 7 x 7
 *   window (the first cell of a plateau), the strongest are kept (ties: the lower cell index a n_rho + k first) and placed
 *   within their cell by a parabola per axis; bands that do not exist have valid = 0.  `sinogram_out` (NULL, or m_all x
 *   n_theta x n_rho float32) receives the unsmoothed sinograms.  Deterministic: no atomics, fixed summation orders.  The
 *   workspace is walked in passes sized from the free device memory; KPDI_HOUGH_PASS=n in the environment forces passes
 *   of n patterns.  The result does not depend on the passes.
 * kpdi_hough_index: per pattern the orientation that explains its bands under one phase.  `bands` (m x n_bands records,
 *   host), `pcs` (n_pc x 3 Bruker projection centres, n_pc = 1 or m), the detector's shape and `s2d` (3 x 3
 *   sample-to-detector matrix, row-major), the phase's reflectors as lines: `normals` (n x 3 unit vectors, crystal
 *   Cartesian, one of g and -g), `family` (n, in [0, n_families)), `angles` (n x n folded interplanar angles, radians),
 *   and the tolerance `tol` (radians).  Triplet voting with integer votes, hypotheses from band pairs, an orthogonal fit
 *   (hough_vote.h).  Out: `quat` (m x 4, the convention of the refinement results), `fit` (mean angular deviation in
 *   degrees, 180 when not indexed), `cm` (matched bands / n_bands), `nmatch` (0 when not indexed).
 * kpdi_hough_plan_describe: {ok, lds, lds_bytes, pattern_bytes, pass_patterns, n_passes, tail_patterns} of the plan for
 *   `room_bytes` of workspace; host arithmetic.  kpdi_hough_default_n_rho: one pixel per rho cell.
 * kpdi_hough_optimize_pc: per pattern the projection centre that explains its bands best under one phase (DESIGN.md
 *   section 28; csrc/hough_search.h): SciPy 1.15.3's Nelder-Mead (csrc/nelder_mead.h) from `pc0` (3 doubles, the same
 *   start for every pattern) over the objective "mean `fit` of kpdi_hough_index with every valid band that found no
 *   reflector charged `tol_deg`; 180 where PCz <= 0; `tol_deg` for a pattern without a valid band", one search per
 *   pattern on one lane each, the whole search on the device.  `bands`, the detector, the phase tables and `tol` as for
 *   kpdi_hough_index; `tol_deg` is `tol` in degrees as the caller rounds it.  `xatol`, `fatol`; `maxiter`, `maxfev`: <= 0
 *   = unset, resolved as SciPy does (both unset: 600 each; one unset: that one unlimited); a budget that allows a search
 *   more than 10000 evaluations (maxfev, or 4 + 5 maxiter where maxfev is unlimited) is refused with KPDI_EINVAL.  The kernel is launched until
 *   every search has ended, each launch advancing every search by at most `evals_per_launch` evaluations (0: the
 *   environment's KPDI_HOUGH_SEARCH_EVALS, else 6) - a bound on the duration of one kernel; `lanes` patterns share a
 *   workgroup (0: from the plan, few while m is small so that the searches spread over the CUs, 64 at the most).  Neither
 *   changes a bit of the result.  Out: `pc` (m x 3, the best vertex), `fun` (m), `nfev`, `nit` and `status` (m each;
 *   SciPy's: 0 converged, 1 evaluations ran out, 2 iterations ran out). */
int kpdi_hough_default_n_rho(int ny, int nx);
int kpdi_hough_plan_describe(int ny, int nx, int n_theta, int n_rho, int64_t m, int64_t room_bytes, int64_t forced,
                             int64_t *desc);
int kpdi_hough_bands(kpdi_ctx *ctx, int n_theta, int n_rho, const float *cos_sin, const float *theta_taps, int theta_radius,
                     const float *rho_taps, int rho_radius, int rim, int n_bands, void *bands_out, float *sinogram_out);
int kpdi_hough_index(kpdi_ctx *ctx, const void *bands, int64_t m, int n_bands, const double *pcs, int64_t n_pc, int ny, int nx,
                     const double *s2d, const double *normals, const int32_t *family, int n_reflectors, int n_families,
                     const double *angles, double tol, double *quat, double *fit, double *cm, int32_t *nmatch);
int kpdi_hough_optimize_pc(kpdi_ctx *ctx, const void *bands, int64_t m, int n_bands, const double *pc0, int ny, int nx,
                           const double *s2d, const double *normals, const int32_t *family, int n_reflectors, int n_families,
                           const double *angles, double tol, double tol_deg, double xatol, double fatol, int maxiter, int maxfev,
                           int evals_per_launch, int lanes, double *pc, double *fun, int32_t *nfev, int32_t *nit,
                           int32_t *status);

/* ---- geometrical simulations: Kikuchi lines and zone axes on the detector (KikuchiPatternSimulator.on_detector,
 * simulations/kikuchi_pattern_simulator.py:217-380; _kikuchi_pattern_features.py; _kikuchi_pattern_simulation.py:468-534) -----
 * Independent of the resident patterns.  All arrays are host memory, float64 unless said otherwise, row vectors.
 * `rotations` (n_points x 4) are unit quaternions; U_o is the matrix of rotate_vector (orix's Rotation.to_matrix()).
 * `u_s` (3 x 3) is detector.sample_to_detector transposed; `a_star` (3 x 3) has rows a*, b*, c*, `a_direct` rows a, b, c.
 * Per point U_os = U_o u_s, hkl_d = hkl (a_star U_os), uvw_d = uvw (a_direct U_os), formed once per point.
 * `pcs` (n_pc x 8, n_pc 1 or n_points) holds per projection centre: the gnomonic x_min, x_max, y_min, y_max each widened by
 * one pixel, pcx / pcz * aspect_ratio, pcy / pcz, x_scale, y_scale.
 *
 * kpdi_geometrical_visibility: `kind` KPDI_GEOMETRICAL_LINES takes `vectors` (m x 3) as hkl and `basis` as a_star,
 * KPDI_GEOMETRICAL_ZONE_AXES as uvw and a_direct.  flags[i] (uint8, m) gets bit 0 when z > 0 at one point at least, and for
 * zone axes bit 1 when x / z and y / z lie inside the widened bounds of one point at least (any sign of z; comparisons with
 * NaN or inf are false).
 *
 * kpdi_geometrical_coordinates: for n_points x m lines and n_points x z zone axes (z may be 0, its four pointers then
 * unused): in_pattern (uint8) = z > 0; lines: the plane trace R (cos a1, sin a1, cos a2, sin a2) in gnomonic coordinates
 * (n_points x m x 4), NaN unless |h| < R and z > -1e-5 with h = z / sqrt(x^2 + y^2), R = r_gnomonic, and in pixels
 * ((g + xoff) / x_scale, (-g + yoff) / y_scale); zone axes: (x / z, y / z) (n_points x z x 2), NaN unless
 * sqrt((x/z)^2 + (y/z)^2) < R and z > -1e-5, and in pixels, NaN also outside the point's widened bounds.  The map is
 * walked in passes sized from free device memory; results do not depend on the pass or chunk length
 * (csrc/geometrical.hip, csrc/geometrical_plan.h).
 * KPDI_EINVAL before anything runs: NULL, m < 1, z < 0, n_points < 1, n_pc neither 1 nor n_points, an unknown kind. */
#define KPDI_GEOMETRICAL_LINES 0
#define KPDI_GEOMETRICAL_ZONE_AXES 1
int kpdi_geometrical_visibility(kpdi_ctx *ctx, const double *vectors, int64_t m, int kind, const double *rotations,
                                int64_t n_points, const double *u_s, const double *basis, const double *pcs, int64_t n_pc,
                                uint8_t *flags);
int kpdi_geometrical_coordinates(kpdi_ctx *ctx, const double *hkl, int64_t m, const double *uvw, int64_t z,
                                 const double *rotations, int64_t n_points, const double *u_s, const double *a_star,
                                 const double *a_direct, const double *pcs, int64_t n_pc, double r_gnomonic,
                                 uint8_t *line_in_pattern, double *line_gnomonic, double *line_pixel,
                                 uint8_t *zone_in_pattern, double *zone_gnomonic, double *zone_pixel);

/* ---- dictionary sweep (_dictionary_indexing loop, indexing/_dictionary_indexing.py:94-128)
 * One call = one loop iteration: prepare_dictionary (cast, mask, normalise) +
 * match + top-k of the chunk + merge into the running best-k, all on the GPU.
 * `global_start` is the dictionary index of the chunk's first pattern
 * (`simulation_indices_i += start`, :118).  Chunks may arrive in any order and,
 * with several ranks, each rank pushes only its own shard.
 * The host-pointer form returns as soon as the upload has consumed `patterns` (the sweep
 * of the chunk is still running; it is ordered before every later call on the context);
 * uploads go through two staging buffers on a copy stream and overlap the sweep of the
 * previous piece / chunk - also with KPDI_COMPUTE_F64, whose look at a chunk's certification (and the extra screening
 * passes it may ask for) is left to the next call on the context.
 * SMALL CHUNKS ARE SWEPT TOGETHER.  The reference's call hands over `n_per_iteration` patterns per iteration - a tenth
 * of the dictionary in its tutorial, 3044 patterns - and one such chunk fills three quarters of ONE tile round of the
 * chip.  A pushed chunk of fewer than two tile rounds (8192 patterns against 4096 experimental ones) therefore only
 * joins the context's pending rows (its raw patterns are copied device-to-device); they are prepared and matched as
 * one launch set once three rounds' worth have come in, or when anything reads or ends the sweep (finalize,
 * synchronize, counters, export; a new experimental set, problem or keep_n forgets them with the running lists), and the
 * merge kernel translates rows of the coalesced matrix back to dictionary indices.  Chunks join in rising
 * dictionary order, one dtype, at most 16 per sweep; anything else sweeps the pending rows first.  The result never
 * depends on it (tests/test_gpu_engine.py); not in KPDI_COMPUTE_F64 (rescoring reads a chunk's own raw patterns);
 * KPDI_NO_COALESCE=1 switches it off.  Chunks handed over to be HELD (kpdi_hold_*) wait the same way and become one
 * resident chunk, eight rounds' worth at a time.  configs[1] pushed as 33 chunks of 3044: 26.6 -> 23.6 ms per call (one pass: 21.3; profiles/r05_group_chunks.txt). */
int kpdi_push_dictionary_chunk(kpdi_ctx *ctx, const void *patterns, int dtype,
                               int64_t n_chunk, int64_t global_start);
int kpdi_push_dictionary_chunk_dev(kpdi_ctx *ctx, const void *d_patterns, int dtype,
                                   int64_t n_chunk, int64_t global_start);
/* forget the running best-k (start another sweep over the same experimental set) */
int kpdi_reset_topk(kpdi_ctx *ctx);
/* scores: M x keep_n float32, descending; indices: M x keep_n int64 (the
 * reference's `simulation_indices` end up int64).  Ties: lower
 * dictionary index first.  With a communicator (kpdi_comm_init) every rank first
 * all-gathers the per-shard lists over RCCL and merges them, so all ranks get
 * the same, global result. */
int kpdi_finalize(kpdi_ctx *ctx, float *scores_out, int64_t *indices_out);
/* kpdi_finalize in two halves, for a caller that indexes map after map against one dictionary: kpdi_finalize_async queues
 * the (all-gather + merge over the ranks and the) result's device-to-host copies and returns a ticket at once;
 * kpdi_finalize_wait(ticket) blocks until they have landed and hands the result over.  Between the two the caller may
 * already queue the NEXT map (kpdi_set_experimental*, kpdi_push_*): the hand-over of a result - synchronisation, copies,
 * widening the indices, ~0.1 ms - then costs the GPU nothing.  At most two results may be pending; not available with
 * KPDI_COMPUTE_F64.  Same results as kpdi_finalize (= async + wait); the reference has no counterpart (its loop is
 * synchronous, indexing/_dictionary_indexing.py:94-128).  kpdi_pending_result_size: the number of (pattern, rank) entries
 * kpdi_finalize_wait will write for a ticket (m * keep_n at the time of the async call). */
int kpdi_finalize_async(kpdi_ctx *ctx, int *ticket);
int kpdi_finalize_wait(kpdi_ctx *ctx, int ticket, float *scores_out, int64_t *indices_out);
int kpdi_pending_result_size(kpdi_ctx *ctx, int ticket, int64_t *n);
/* The indices kpdi_finalize handed out last, as it left them in its page-locked staging buffer (int32, row-major
 * (m, keep_n)): valid until the next but one kpdi_finalize[_async] / kpdi_destroy of this context; *indices = NULL when there is none.
 * What a host layer compares a caller's array with before it tells kpdi_orientation_similarity_map to use the lists still
 * resident in HBM (indexing/_orientation_similarity_map.py:30-152 reads `simulation_indices` the caller may have edited). */
int kpdi_result_indices_i32(kpdi_ctx *ctx, const int32_t **indices, int64_t *n);
/* KPDI_COMPUTE_F64: the float64 scores (kpdi_finalize then returns them rounded to float32) */
int kpdi_finalize_f64(kpdi_ctx *ctx, double *scores_out, int64_t *indices_out);

/* ---- dictionary generation on the device ------------------
 * EBSDMasterPattern.get_patterns (signals/ebsd_master_pattern.py:95-330): project a
 * square-Lambert master pattern onto the detector, one simulated pattern per
 * rotation, without the dictionary ever existing in host memory.
 *
 * kpdi_set_master_pattern: the arrays `_get_master_pattern_arrays_from_energy`
 * returns (signals/_kikuchi_master_pattern.py:303-345): npy rows x npx columns per
 * hemisphere, dtype U8 / U16 / F32 (F64 is rounded to F32).  `lower` may be NULL
 * (hemisphere != "both": lower = upper). */
int kpdi_set_master_pattern(kpdi_ctx *ctx, const void *upper, const void *lower,
                            int dtype, int npx, int npy);
/* kpdi_set_detector: arguments of `_get_direction_cosines_for_fixed_pc`
 * (signals/util/_master_pattern.py:133-204) for the whole detector:
 * gnomonic_bounds = (x_min, x_max, y_min, y_max), om_detector_to_sample = 3x3
 * row-major.  The direction cosines (nrows*ncols x 3 f64) are computed on the host
 * in that function's operation order and kept on the device. */
int kpdi_set_detector(kpdi_ctx *ctx, const double *gnomonic_bounds, double pcz,
                      int nrows, int ncols, const double *om_detector_to_sample);
/* alternative: hand over direction cosines computed elsewhere (npix x 3 f64) */
int kpdi_set_direction_cosines(kpdi_ctx *ctx, const double *direction_cosines, int64_t npix);
/* the resident direction cosines, npix*3 doubles */
int kpdi_get_direction_cosines(kpdi_ctx *ctx, double *out);
/* `_project_patterns_from_master_pattern_with_fixed_pc` (:299-370): `rotations` =
 * n x 4 unit quaternions (a, b, c, d) f64; out = n x npix of `dtype_out` (F32, F64,
 * U8, U16; integers truncate like ndarray.astype) in HOST memory.  `rescale` != 0:
 * every pattern is min-max rescaled to [out_min, out_max] (pattern/_pattern.py:97-111). */
int kpdi_project_patterns(kpdi_ctx *ctx, const double *rotations, int64_t n, int rescale,
                          double out_min, double out_max, int dtype_out, void *out);
/* `_project_patterns_from_master_pattern_with_varying_pc` (:374-445) with
 * `_get_direction_cosines_for_varying_pc` (:216-295): pattern i is projected with its own
 * PC pcs[i] = (PCx, PCy, PCz), Bruker convention; the direction cosines are formed on the
 * device.  Needs only kpdi_set_master_pattern. */
int kpdi_project_patterns_varying_pc(kpdi_ctx *ctx, const double *rotations, const double *pcs,
                                     int64_t n, int nrows, int ncols,
                                     const double *om_detector_to_sample, int rescale,
                                     double out_min, double out_max, int dtype_out, void *out);
/* generate + match in one call - what the reference does when the dictionary is a lazy
 * `get_patterns(..., compute=False)` signal: the chunk is computed inside the indexing loop
 * (indexing/_dictionary_indexing.py:106-108).  The chunk of the dictionary belonging to
 * `rotations` is projected as float32 straight into device memory and swept like
 * kpdi_push_dictionary_chunk(..., KPDI_F32, n, global_start); the detector must have
 * sy*sx pixels (kpdi_set_problem). */
int kpdi_push_rotations_chunk(kpdi_ctx *ctx, const double *rotations, int64_t n,
                              int64_t global_start, int rescale, double out_min, double out_max);
/* the same with ONE PROJECTION CENTRE PER PATTERN - a lazy `get_patterns(rotations, detector)` whose detector holds a PC
 * for every rotation (signals/ebsd_master_pattern.py:236-241, :274-283: `nav_shape_det != (1,)`): pattern i of the chunk is
 * projected with pcs[i] = (PCx, PCy, PCz), Bruker convention, on the problem's sy x sx detector (the direction cosines are
 * formed on the device, as in kpdi_project_patterns_varying_pc), then the chunk is swept.  Needs kpdi_set_master_pattern;
 * no kpdi_set_detector. */
int kpdi_push_rotations_chunk_varying_pc(kpdi_ctx *ctx, const double *rotations, const double *pcs, int64_t n,
                                         int64_t global_start, const double *om_detector_to_sample, int rescale,
                                         double out_min, double out_max);

/* ---- resident dictionary: one dictionary, many maps -------------------------------
 * The reference prepares the dictionary again for every `dictionary_indexing()` call
 * (`metric.prepare_dictionary` inside the loop, indexing/_dictionary_indexing.py:106-110),
 * because host memory rarely holds it twice.  A prepared 60 x 60 dictionary of 100 000
 * patterns is 1.45 GB of the 288 GB of HBM, so a series of maps of the same phase and
 * detector (one `kpdi_set_problem`) can be indexed against chunks that are uploaded /
 * simulated and prepared ONCE: `hold` = prepare_dictionary into a buffer that stays,
 * `kpdi_sweep_held` = the match + top-k + merge of every held chunk against the current
 * experimental set (like pushing all of them again, results identical), then
 * kpdi_finalize.  kpdi_set_problem releases the held chunks (their layout depends on
 * shape, mask, metric and arithmetic); set_experimental / reset_topk / set_keep_n do not.
 * With several ranks each rank holds its own shard. */
int kpdi_hold_dictionary_chunk(kpdi_ctx *ctx, const void *patterns, int dtype, int64_t n_chunk,
                               int64_t global_start);
int kpdi_hold_dictionary_chunk_dev(kpdi_ctx *ctx, const void *d_patterns, int dtype,
                                   int64_t n_chunk, int64_t global_start);
/* simulated on the device like kpdi_push_rotations_chunk, then held */
int kpdi_hold_rotations_chunk(kpdi_ctx *ctx, const double *rotations, int64_t n,
                              int64_t global_start, int rescale, double out_min, double out_max);
int kpdi_sweep_held(kpdi_ctx *ctx);
int kpdi_release_held(kpdi_ctx *ctx);
/* patterns held and the device memory they occupy; either pointer may be NULL */
int kpdi_held_size(kpdi_ctx *ctx, int64_t *n_patterns, int64_t *n_bytes);

/* ---- refinement of orientations / projection centres ---------
 * EBSD.refine_orientation / refine_projection_center / refine_orientation_projection_center
 * with the default optimiser (scipy.optimize.minimize, Nelder-Mead): the chunk functions
 * `_refine_*_chunk_scipy` (indexing/_refinement/_refinement.py:441-503, :642-668, :779-809),
 * i.e. `_prepare_pattern` + the objective functions
 * (indexing/_refinement/_objective_functions.py:36-190) + the simplex search, all on the GPU:
 * one workgroup per (pattern, start) runs the whole optimisation.
 * The master pattern is the one given to kpdi_set_master_pattern (the caller passes the
 * float32 hemispheres of `_get_master_pattern_data`, _refinement.py:1288-1320). */
#define KPDI_REFINE_ORI 0     /* x = (phi1, Phi, phi2) [rad];            fixed = (PCx, PCy, PCz)   */
#define KPDI_REFINE_PC 1      /* x = (PCx, PCy, PCz) Bruker convention;  fixed = quaternion (a,b,c,d) */
#define KPDI_REFINE_ORI_PC 2  /* x = (phi1, Phi, phi2, PCx, PCy, PCz);   no fixed values            */
#define KPDI_REFINE_RESULT_STRIDE 9  /* result row: fun (= 1 - NCC), nfev, nit, x[0..nvar), padding */
/* Patterns to refine: `n` patterns of nrows x ncols `dtype` values in host memory.
 * signal_mask: nonzero = pixel NOT used, or NULL.  `rescale` != 0: intensities are rescaled
 * to [-1, 1] first (the reference does so exactly when the patterns are float32,
 * _refinement.py:956).  om_detector_to_sample: 3x3 row-major. */
int kpdi_refine_set_patterns(kpdi_ctx *ctx, const void *patterns, int dtype, int64_t n,
                             int nrows, int ncols, const uint8_t *signal_mask, int rescale,
                             const double *om_detector_to_sample);
/* the prepared patterns (n x k float32, centred) and their squared norms (n float64) */
int kpdi_refine_get_prepared(kpdi_ctx *ctx, float *patterns_out, double *sqnorm_out);
/* Objective values: out[e] = 1 - NCC(pattern[pattern_index[e]], projection(x[e], fixed[e])).
 * x: n_eval x nvar, fixed: n_eval x nfixed (nvar/nfixed = 3/3, 3/4, 6/0 for the three modes). */
int kpdi_refine_objective(kpdi_ctx *ctx, int mode, int64_t n_eval, const int32_t *pattern_index,
                          const double *x, const double *fixed, double *out);
/* Nelder-Mead from every start of every pattern.  x0 / fixed / lower / upper:
 * n_patterns x n_starts x (nvar | nfixed); lower/upper NULL = unbounded (no trust region).
 * maxiter / maxfev <= 0 select SciPy's defaults (200 * nvar each when both are unset, else
 * unlimited).  results: n_patterns x n_starts x KPDI_REFINE_RESULT_STRIDE doubles. */
int kpdi_refine_solve(kpdi_ctx *ctx, int mode, int64_t n_patterns, int n_starts,
                      const double *x0, const double *fixed, const double *lower,
                      const double *upper, double xatol, double fatol, int maxiter, int maxfev,
                      double *results);
/* The optimiser (csrc/nelder_mead.h) alone on an analytic f64 objective (kinds 0..4 of
 * kpdi_powell_selftest), nvar <= 6: lets a test compare the device's simplex path with
 * SciPy's bit for bit.  result: fun, nfev, nit, x[0..nvar). */
int kpdi_nelder_mead_selftest(kpdi_ctx *ctx, int kind, int nvar, const double *x0,
                              const double *lower, const double *upper, double xatol,
                              double fatol, int maxiter, int maxfev, double *result);
/* scipy.optimize.minimize(method="Powell") of SciPy 1.15.3 (csrc/powell.h) from every start of every pattern: the
 * arguments of kpdi_refine_solve with Powell's xtol / ftol.  Bounds: none, or finite for every variable (lower == upper
 * allowed); non-finite bounds are refused.  maxiter / maxfev <= 0 = unset, by Powell's rule: 1000 * nvar each when both
 * are unset, else the unset one is unlimited.  Result rows as kpdi_refine_solve.
 * trace: NULL, or room for trace_capacity rows of nvar + 1 doubles: (x[0..nvar), f) of every objective evaluation of
 * job trace_job (= pattern * n_starts + start), in order; evaluations beyond the capacity are counted (the job's nfev)
 * but not stored. */
int kpdi_refine_solve_powell(kpdi_ctx *ctx, int mode, int64_t n_patterns, int n_starts,
                             const double *x0, const double *fixed, const double *lower,
                             const double *upper, double xtol, double ftol, int maxiter, int maxfev,
                             double *results, int64_t trace_job, double *trace, int trace_capacity);
/* Powell alone on an analytic f64 objective, nvar <= 6 (kind 0: Rosenbrock, 1: weighted bowl, 2: kind 1 rounded to
 * float32 and back, 3: kind 1 but NaN where x[0] > 1.9, 4: NaN everywhere).
 * result: fun, nfev, nit, status (SciPy's 0..4), x[0..nvar). */
int kpdi_powell_selftest(kpdi_ctx *ctx, int kind, int nvar, const double *x0, const double *lower,
                         const double *upper, double xtol, double ftol, int maxiter, int maxfev,
                         double *result);
/* The simplex search NLopt offers as LN_NELDERMEAD, as csrc/nlopt_simplex.h restates it from the text of DESIGN.md
 * section 21 (NLopt itself is not compared with), from every start of every pattern: each (pattern, start) is one
 * independent optimisation with its own evaluation count.  lower / upper: both NULL or both given; infinite bounds and
 * lower == upper (the variable is held) are allowed, NaN is refused.  xstep: NULL (the default step of the text) or
 * one initial step per variable (nvar values, shared by every job).  maxeval <= 0: no limit; ftol_rel <= 0 together
 * with maxeval <= 0 is refused, as are starting points and steps that are not finite.
 * Result rows as kpdi_refine_solve: fun = the lowest value seen, nfev, x = the point it was seen at; the `nit` slot holds
 * the status (NLopt's codes: 1 success, 3 ftol reached, 4 xtol reached, 5 maxeval reached, -1 failure: a step that
 * does not move its variable, -2 invalid arguments: a start outside its bounds). */
int kpdi_refine_solve_nlopt(kpdi_ctx *ctx, int mode, int64_t n_patterns, int n_starts,
                            const double *x0, const double *fixed, const double *lower,
                            const double *upper, const double *xstep, double ftol_rel, int maxeval,
                            double *results);
/* csrc/nlopt_simplex.h alone on an analytic f64 objective, nvar <= 6: kinds 0..4 of kpdi_powell_selftest, 5: the sum
 * of (i + 1) |d| / (1 + |d|), d = x[i] - 0.3 (i + 1), whose concave arms make contractions fail (the shrink step).
 * result: fun, nfev, status, x[0..nvar). */
int kpdi_nlopt_simplex_selftest(kpdi_ctx *ctx, int kind, int nvar, const double *x0,
                                const double *lower, const double *upper, const double *xstep,
                                double ftol_rel, int maxeval, double *result);
/* scipy.optimize.differential_evolution of SciPy 1.15.3 with strategy="best1bin" and polish=False
 * (csrc/differential_evolution.h) for every start of every pattern, each from numpy.random.RandomState(seeds[job]).
 * There is no x0.  lower / upper: required and finite, lower == upper allowed (the variable is held).
 * members: the population SciPy works out, max(5, popsize * max(1, nvar - number of held variables)), the same for
 * every job, within 5..KPDI_DE_POP_MAX.  maxiter >= 0 generations.  mutation_hi = NaN: `mutation` is the number
 * mutation_lo; else the dither pair, mutation_lo <= mutation_hi; both within [0, 2).  init: 0 "latinhypercube",
 * 1 "random".  updating: 0 "immediate", 1 "deferred".  seeds: one per job, n_patterns x n_starts.
 * Result rows and trace as kpdi_refine_solve_powell (fun, nfev, nit, x). */
#define KPDI_DE_POP_MAX 256
int kpdi_refine_solve_de(kpdi_ctx *ctx, int mode, int64_t n_patterns, int n_starts, const double *fixed,
                         const double *lower, const double *upper, int members, int maxiter, double tol,
                         double atol, double mutation_lo, double mutation_hi, double recombination, int init,
                         int updating, const uint32_t *seeds, double *results, int64_t trace_job,
                         double *trace, int trace_capacity);
/* csrc/differential_evolution.h alone on an analytic f64 objective, nvar <= 6: kinds 0..4 of kpdi_powell_selftest,
 * 5: the sum of (i + 1) (d d + 0.1 d), d = |x[i]|, whose minimum sits on the lower bound of a box from 0 (trial
 * vectors leave the box and are drawn again), 6: +inf everywhere, 7: 0.1 everywhere.  Options as
 * kpdi_refine_solve_de.  result: fun, nfev, nit, success (1 | 0), x[0..nvar). */
int kpdi_de_selftest(kpdi_ctx *ctx, int kind, int nvar, const double *lower, const double *upper, int members,
                     int maxiter, double tol, double atol, double mutation_lo, double mutation_hi,
                     double recombination, int init, int updating, uint32_t seed, double *result);
/* scipy.optimize.basinhopping of SciPy 1.15.3 around minimize(method="Nelder-Mead"), with the default step and the
 * default (Metropolis) acceptance test (csrc/basinhopping.h), from every start of every pattern, each from
 * numpy.random.RandomState(seeds[job]).  Unbounded.  niter >= 0 hops after the initial quench; T: the temperature (0:
 * no uphill hop is taken); stepsize finite; interval >= 1; niter_success < 0: SciPy's None (niter + 2);
 * target_accept_rate and stepwise_factor within (0, 1); a NaN among the options is refused.  xatol / fatol / maxiter /
 * maxfev: the options of every quench, as kpdi_refine_solve takes them.  seeds: one per job, n_patterns x n_starts.
 * Result rows and trace as kpdi_refine_solve_powell: fun and x of the lowest result, nfev the sum over all quenches
 * (the initial one included), nit. */
int kpdi_refine_solve_basinhopping(kpdi_ctx *ctx, int mode, int64_t n_patterns, int n_starts, const double *x0,
                                   const double *fixed, int niter, double T, double stepsize, int interval,
                                   int niter_success, double target_accept_rate, double stepwise_factor,
                                   double xatol, double fatol, int maxiter, int maxfev, const uint32_t *seeds,
                                   double *results, int64_t trace_job, double *trace, int trace_capacity);
/* csrc/basinhopping.h alone on an analytic f64 objective, nvar <= 6: kinds 0..4 of kpdi_powell_selftest.  Options as
 * kpdi_refine_solve_basinhopping.  result: fun, nfev, nit, success (1 | 0), minimization_failures, x[0..nvar). */
int kpdi_basinhopping_selftest(kpdi_ctx *ctx, int kind, int nvar, const double *x0, int niter, double T,
                               double stepsize, int interval, int niter_success, double target_accept_rate,
                               double stepwise_factor, double xatol, double fatol, int maxiter, int maxfev,
                               uint32_t seed, double *result);
/* The random stream of csrc/differential_evolution.h alone, from numpy.random.RandomState(seed): `program` holds n
 * rows (op, a, b) of doubles - 0: uniform(), 1: uniform(a, b), 2: randint(0, a) with 1 <= a < 2^31, 3: shuffle of a
 * persistent arange(a) (made anew when a changes), 4: permutation(range(a)); a <= KPDI_DE_POP_MAX for 3 and 4.
 * out: the raw 64 bits of what they return, one word per draw, `a` words for 3 and 4; out_words must be their exact
 * count. */
int kpdi_mt19937_selftest(kpdi_ctx *ctx, uint32_t seed, const double *program, int n, uint64_t *out,
                          int64_t out_words);

/* The top-k merge kernels alone, on lists the caller makes (tests/test_gpu_merge.py): everything is host memory.
 * kpdi_merge_selftest: n_src <= 3 sources; src_scores / src_idx / src_cnt are arrays of n_src host pointers
 * (src_cnt[j] NULL: no counts, else m x src_lists[j]), src_elems[j] the elements of source j's two buffers, so that
 * padded (list_stride > len, row_stride > lists * len) and gathered (row_stride < list_stride) layouts can be given.
 * seg_n segments (row0 / delta) translate the sources whose bit is set in seg_sources.  out_scores / out_idx:
 * m x out_stride, prefilled by the caller, uploaded, merged into (columns out_offset .. out_offset + k) and read back
 * whole.  force: -1 = the kernel the candidate count selects, 0..6 = merge_cached_kernel<4 | 12 | 24 | 48>,
 * merge_block_kernel<24 | 64>, merge_kernel (csrc/merge_plan.h).  *launch_error: the HIP error of the launch (1,
 * invalid value, when the forced kernel cannot hold the candidates - nothing is launched); *plan_ran: the kernel. */
int kpdi_merge_selftest(kpdi_ctx *ctx, int n_src, const float *const *src_scores,
                        const int32_t *const *src_idx, const int32_t *const *src_cnt,
                        const int64_t *src_elems, const int32_t *src_lists, const int32_t *src_len,
                        const int32_t *src_row_stride, const int32_t *src_list_stride, int m, int k,
                        int out_stride, int out_offset, int seg_n, const int32_t *seg_row0,
                        const int32_t *seg_delta, uint32_t seg_sources, float *out_scores,
                        int32_t *out_idx, int force, int32_t *launch_error, int32_t *plan_ran);
/* The float64 merge: run_s / run_i m x k or both NULL; in_place: the result replaces the running list (as the sweep
 * does), else it goes to a buffer of its own, prefilled from out_s / out_i.  Candidates: `lists` lists of `len` per
 * pattern in buffers of cand_elems elements.  cand_s32 (m x s32_stride) and uncertified both non-NULL: certification
 * with max_diff, eps_floor and enumerated_all; *uncertified = patterns that failed it.  *launch_error as above (a
 * pattern's entries beyond 150 KB of LDS are refused). */
int kpdi_merge64_selftest(kpdi_ctx *ctx, int m, int k, const double *run_s, const int32_t *run_i,
                          int in_place, const double *cand_s64, const int32_t *cand_i,
                          int64_t cand_elems, int lists, int len, int64_t row_stride,
                          int64_t list_stride, const float *cand_s32, int s32_stride, int s32_col,
                          int enumerated_all, float max_diff, float eps_floor, double *out_s,
                          int32_t *out_i, int32_t *uncertified, int32_t *launch_error);
/* The float64 rescoring kernel alone (csrc/rescore.hip: rescore_kernel; tests/test_gpu_rescore.py), every field of its
 * launch the caller's.  exp_raw: m_all x npix of exp_dtype; row_map: m source rows, or NULL (then the first m rows).
 * dict_raw: n_chunk x npix of dict_dtype, the dictionary patterns global_start .. global_start + n_chunk.  pix_map: k
 * detector pixels, or NULL (then the first k).  cand_s / cand_i / cand_s64: m x cand_stride; the kernel rescores columns
 * cand_offset .. cand_offset + n_cand; cand_s64 is uploaded as given and comes back whole.  max_diff_in: what the
 * running maximum of |f32 score - f64 score| starts from (>= 0); *max_diff_out: what it ends at.  KPDI_EINVAL before
 * anything reaches the GPU: a dtype code outside the nine, k < 1, a row_map entry outside [0, m_all), a pix_map entry
 * outside [0, npix), cand_offset + n_cand > cand_stride, k > npix without a pix_map, m > m_all without a row_map. */
int kpdi_rescore_selftest(kpdi_ctx *ctx, const void *exp_raw, int exp_dtype, int64_t m_all,
                          const int32_t *row_map, int m, const void *dict_raw, int dict_dtype,
                          int64_t n_chunk, int64_t global_start, const int32_t *pix_map, int k, int npix,
                          int metric, const float *cand_s, const int32_t *cand_i, int cand_stride,
                          int cand_offset, int n_cand, float max_diff_in, double *cand_s64,
                          float *max_diff_out, int32_t *launch_error);
/* The queued initialisations' one launch: n <= 8 ranges of words[i] 32-bit words at byte_offset[i] (a multiple of 4)
 * of one device buffer of buffer_words words, uploaded from and read back into `buffer`; value[i], or the shared
 * bound's pattern when bound_used[i] >= 0. */
int kpdi_fill_selftest(kpdi_ctx *ctx, int n, const int64_t *words, const uint32_t *value,
                       const int32_t *bound_used, const int64_t *byte_offset, uint32_t *buffer,
                       int64_t buffer_words);

/* ---- orientation similarity map ---------------------------------
 * kikuchipy.indexing.orientation_similarity_map
 * (indexing/_orientation_similarity_map.py:30-152).  simulation_indices: ny*nx x keep_n
 * int64 in host memory, or NULL = the best-k lists still resident from the last sweep
 * (kpdi_finalize; needs ny*nx == number of matched patterns).  footprint_offsets: n_fp
 * (dy, dx) pairs, the non-zero footprint elements in row-major order relative to the
 * footprint's centre (shape // 2); center_index as in the reference.  out: ny x nx x
 * (n_best - from_n_best + 1) float32, layer 0 = n_best; NaN where a point has no
 * neighbour. */
int kpdi_orientation_similarity_map(kpdi_ctx *ctx, const int64_t *simulation_indices, int ny,
                                    int nx, int keep_n, int n_best, int from_n_best,
                                    const int32_t *footprint_offsets, int n_fp, int center_index,
                                    int normalize, float *out);

/* ---- kikuchipy h5ebsd files --------------------------------------
 * What `kikuchipy.load("file.h5")` reads for this path
 * (io/plugins/kikuchipy_h5ebsd/_api.py:64-160, io/plugins/_h5ebsd.py:303-390): the scan's
 * header, `EBSD/Data/patterns` as (n_rows, n_columns, pattern_height, pattern_width) -
 * zero padded when the file holds fewer patterns -, `EBSD/Header/static_background` and
 * the projection centres.  The HDF5 C library is dlopen()ed (libhdf5.so from the
 * loader path, /opt/conda/lib, or $KPDI_HDF5_LIB); without it these calls fail.
 * `scan`: group name ("Scan 1"), NULL or "" = the first scan of the file. */
typedef struct kpdi_h5ebsd_info {
  char scan[64];                 /* the scan group that was read */
  int32_t ny, nx, sy, sx;        /* n_rows, n_columns, pattern_height, pattern_width */
  int32_t dtype;                 /* KPDI_* element type of the patterns */
  int32_t has_static_background; /* EBSD/Header/static_background of shape sy x sx present */
  int32_t static_background_dtype;
  int32_t binning;
  int64_t n_stored;              /* pattern values actually in the file (< ny*nx*sy*sx: padded) */
  int64_t n_pc;                  /* projection centres in the header (1 or ny*nx), 0 = none */
  double step_y, step_x, detector_pixel_size, sample_tilt, azimuth_angle, elevation_angle;
} kpdi_h5ebsd_info;
size_t kpdi_dtype_size(int dtype);
int kpdi_h5ebsd_info_read(const char *path, const char *scan, kpdi_h5ebsd_info *info);
int kpdi_h5ebsd_read_patterns(const char *path, const char *scan, void *out, size_t out_bytes);
int kpdi_h5ebsd_read_static_background(const char *path, const char *scan, void *out, size_t out_bytes);
/* out: n_pc x (PCx, PCy, PCz) float64 (Bruker convention, as stored) */
int kpdi_h5ebsd_read_pc(const char *path, const char *scan, double *out, int64_t n_pc);
/* read the scan's patterns through a pinned host buffer straight into the context's
 * experimental set (= kpdi_set_experimental of the file's contents) */
int kpdi_set_experimental_h5ebsd(kpdi_ctx *ctx, const char *path, const char *scan,
                                 const uint8_t *nav_mask);

/* ---- multi-GPU: dictionary sharded over ranks, one process per GPU -------- */
#define KPDI_UNIQUE_ID_BYTES 128
int kpdi_comm_unique_id(uint8_t *id_out /* KPDI_UNIQUE_ID_BYTES */);
int kpdi_comm_init(kpdi_ctx *ctx, int rank, int nranks, const uint8_t *id);
/* The fallback chain of a multi-process job (kikuchipy_amd/parallel.py: Communicator.attach; the sharding replaces the
 * chunk loop of indexing/_dictionary_indexing.py:100-128, whose merge :120-128 is what the gather feeds):
 *   kpdi_comm_selftest - ONE all-gather of n_bytes per rank, awaited for at most timeout_ms (KPDI_ETIMEOUT): a
 *       communicator that bootstrapped can still hang in its first collective;
 *   kpdi_comm_drop - forget (abort) the communicator, also while a kpdi_comm_init of this context hangs on another
 *       thread: finalize then returns this context's own lists, or what kpdi_import_lists gave it;
 *   kpdi_export_lists / kpdi_import_lists - the HOST-STAGED gather: every rank exports its own m x keep_n lists
 *       (scores float, or double in KPDI_COMPUTE_F64; indices int32), the caller's transport all-gathers them
 *       (M * keep_n * 8 bytes per rank: 0.66 MB at configs[1]), every rank imports the n_ranks lists (rank-major) and
 *       its next kpdi_finalize[_f64 / _async] merges them with the kernel - and the total order - of the RCCL path. */
int kpdi_comm_selftest(kpdi_ctx *ctx, int64_t n_bytes, int timeout_ms);
int kpdi_comm_drop(kpdi_ctx *ctx);
int kpdi_export_lists(kpdi_ctx *ctx, void *scores_out, int32_t *indices_out);
int kpdi_import_lists(kpdi_ctx *ctx, const void *scores_all, const int32_t *indices_all, int n_ranks);

/* ---- multi-GPU from ONE process: a group of contexts ----------------------------------------------------
 * The reference's call is one call in one interpreter (signals/ebsd.py:1827-1984; its loop over dictionary
 * chunks, indexing/_dictionary_indexing.py:100-128, never crosses a process boundary).  A kpdi_group keeps that
 * shape on a node with several MI355X: it owns one context per entry of `device_ids` and one host thread per
 * member, and its entry points are the per-context ones fanned out -
 *   set_problem / set_keep_n / set_experimental / remove_*_background / set_master_pattern / set_detector: every member
 *       (the experimental set is replicated from the caller's ONE host buffer);
 *   push_* / hold_*: a dictionary chunk is handed to the member(s) the assignment rule names (csrc/group_assign.h,
 *       kpdi_group_assign_chunk).  With the dictionary size announced (kpdi_group_set_dictionary_size) member i has
 *       a quota = the i-th of n_dev near-equal parts of the dictionary; a chunk goes to the member that has taken the
 *       fewest patterns so far, never beyond its quota - the rest spills to the next.  A single-pass call (one chunk =
 *       the dictionary) is thereby cut into the contiguous n_dev parts, while the chunks of a CHUNKED call - the
 *       reference's own shape: n_per_iteration patterns per iteration, _dictionary_indexing.py:100-128 - stay whole
 *       and go round the members (a tenth of the dictionary cut 8 ways would leave a member a fraction of one tile
 *       round per launch).  Size unknown: a chunk is cut into min(n_dev, n_chunk / (2 tile rounds)) >= 1 near-equal
 *       pieces for the least-loaded members.  A piece is pushed with global_start + its first row, so a global
 *       index is still chunk start + row (`simulation_indices_i += start`, :118).  Pushes only QUEUE the pieces on the
 *       members' host threads and return (at most 2 chunks wait per member): the next chunk can be fetched while
 *       the previous ones are uploaded / generated / swept.  A failure of queued work is reported by the next
 *       joining call (synchronize, finalize, any set_* call);
 *   finalize: the members' best-k lists are gathered and merged by the same (score desc, index asc) kernel used
 *       between chunks, and the caller gets ONE result - identical, bit for bit, to the single-context result.
 * Gather = KPDI_GATHER_RCCL: an in-process RCCL communicator (ncclCommInitAll - no sockets, no environment) and the
 * ncclAllGather of kpdi_finalize, or KPDI_GATHER_P2P: hipMemcpyPeerAsync of the members' M * keep_n * 8 bytes into
 * member 0 (xGMI between devices) - which also works when several members share ONE device (RCCL refuses duplicate
 * devices), so the whole multi-device code path runs on a 1-GPU box.  KPDI_GATHER_AUTO: $KPDI_GATHER = "rccl" | "p2p"
 * if set, else P2P when a device appears twice, else RCCL (falling back to P2P, with the reason kept for
 * kpdi_group_describe, if the communicator cannot be created or its first all-gather - a small one, run by
 * kpdi_group_create on every member at once under $KPDI_COMM_TIMEOUT seconds, default 60 - does not complete; with
 * KPDI_GATHER_RCCL asked for by name that is an error instead).  A group of one device gathers nothing.
 * Calls other than the chunk pushes are synchronous with respect to the members' host work (they return when every
 * member's call has) and, like the per-context calls, asynchronous with respect to the GPUs.  One thread at a time
 * drives a group.
 * The members stay reachable (kpdi_group_member) for the per-context calls that have no group form - device buffers,
 * counters, refinement; the caller must not use a member while a group call is running. */
typedef struct kpdi_group kpdi_group;
#define KPDI_GATHER_AUTO 0
#define KPDI_GATHER_RCCL 1
#define KPDI_GATHER_P2P 2
#define KPDI_GATHER_NONE 3 /* reported by kpdi_group_gather for a group of one device */
int kpdi_group_create(const int *device_ids, int n_dev, int gather, kpdi_group **out);
int kpdi_group_destroy(kpdi_group *g);
int kpdi_group_size(const kpdi_group *g);
int kpdi_group_gather(const kpdi_group *g);        /* the KPDI_GATHER_* mode in use */
const char *kpdi_group_describe(const kpdi_group *g); /* "8 devices [0,1,...], gather rccl" (+ why a fallback was taken) */
kpdi_ctx *kpdi_group_member(kpdi_group *g, int i); /* borrowed; NULL when i is out of range */
/* rows [*start, *end) of the i-th of n_dev near-equal contiguous parts of n rows (a member's quota of the dictionary) */
int kpdi_group_chunk_share(int64_t n_chunk, int i, int n_dev, int64_t *start, int64_t *end);
/* The assignment rule as a pure function (planning, tests; needs no GPU): the pieces of a chunk of n_chunk patterns
 * for a group of n_dev members that have taken load[i] patterns so far (updated), dictionary size n_total (0 =
 * unknown, then min_piece decides between the n_dev-way cut and a whole chunk).  Up to max_pieces pieces are written
 * (member, first row, rows - in row order), *n_pieces = how many there are. */
int kpdi_group_assign_chunk(int n_dev, int64_t n_total, int64_t min_piece, int64_t *load, int64_t n_chunk, int max_pieces,
                            int *member_out, int64_t *row0_out, int64_t *rows_out, int *n_pieces);
/* Dictionary patterns the coming sweep(s) will push in total (0 = unknown); starts a new assignment.  The members'
 * takes are also reset by set_problem / set_keep_n / set_experimental* / reset_topk (a new sweep). */
int kpdi_group_set_dictionary_size(kpdi_group *g, int64_t n_total);
int kpdi_group_synchronize(kpdi_group *g);
int kpdi_group_set_problem(kpdi_group *g, int sy, int sx, const uint8_t *signal_mask, int metric, int compute_dtype,
                           int keep_n);
int kpdi_group_set_keep_n(kpdi_group *g, int keep_n);
int kpdi_group_set_experimental(kpdi_group *g, const void *patterns, int dtype, int64_t m_all, const uint8_t *nav_mask);
/* d_patterns[i]: the set in the memory of member i's device (callers that keep their inputs resident) */
int kpdi_group_set_experimental_dev(kpdi_group *g, const void *const *d_patterns, int dtype, int64_t m_all,
                                    const uint8_t *nav_mask);
int64_t kpdi_group_n_experimental(kpdi_group *g);
int kpdi_group_remove_static_background(kpdi_group *g, const float *static_bg, int operation, int scale_bg);
int kpdi_group_remove_dynamic_background(kpdi_group *g, int operation, int filter_domain, double std, double truncate);
int kpdi_group_get_experimental(kpdi_group *g, void *patterns_out); /* member 0's (all members hold the same) */
/* returns when the members' uploads have consumed `patterns` (reference loop: the chunk is a temporary, :106-108) */
int kpdi_group_push_dictionary_chunk(kpdi_group *g, const void *patterns, int dtype, int64_t n_chunk,
                                     int64_t global_start);
/* the same, returning at once: `patterns` is BORROWED until kpdi_group_chunks_consumed reports a ticket >= *ticket
 * (tickets count up from 1), or until kpdi_group_synchronize / a finalize has returned */
int kpdi_group_push_dictionary_chunk_borrowed(kpdi_group *g, const void *patterns, int dtype, int64_t n_chunk,
                                              int64_t global_start, int64_t *ticket);
int kpdi_group_chunks_consumed(kpdi_group *g, int64_t *ticket); /* every borrowed chunk up to *ticket has been consumed */
/* explicit per-member chunks in device memory: member i sweeps n_chunk[i] patterns at d_patterns[i] (n_chunk[i] = 0:
 * nothing) whose first pattern has dictionary index global_start[i] */
int kpdi_group_push_dictionary_chunk_dev(kpdi_group *g, const void *const *d_patterns, int dtype, const int64_t *n_chunk,
                                         const int64_t *global_start);
int kpdi_group_set_master_pattern(kpdi_group *g, const void *upper, const void *lower, int dtype, int npx, int npy);
int kpdi_group_set_detector(kpdi_group *g, const double *gnomonic_bounds, double pcz, int nrows, int ncols,
                            const double *om_detector_to_sample);
int kpdi_group_push_rotations_chunk(kpdi_group *g, const double *rotations, int64_t n, int64_t global_start, int rescale,
                                    double out_min, double out_max);
int kpdi_group_hold_dictionary_chunk(kpdi_group *g, const void *patterns, int dtype, int64_t n_chunk,
                                     int64_t global_start);
int kpdi_group_hold_rotations_chunk(kpdi_group *g, const double *rotations, int64_t n, int64_t global_start, int rescale,
                                    double out_min, double out_max);
int kpdi_group_sweep_held(kpdi_group *g);
int kpdi_group_release_held(kpdi_group *g);
int kpdi_group_held_size(kpdi_group *g, int64_t *n_patterns, int64_t *n_bytes); /* summed over the members */
int kpdi_group_reset_topk(kpdi_group *g);
/* as kpdi_finalize / _f64 / _async / _wait / kpdi_pending_result_size, the result being the merge over all members */
int kpdi_group_finalize(kpdi_group *g, float *scores_out, int64_t *indices_out);
int kpdi_group_finalize_f64(kpdi_group *g, double *scores_out, int64_t *indices_out);
int kpdi_group_finalize_async(kpdi_group *g, int *ticket);
int kpdi_group_finalize_wait(kpdi_group *g, int ticket, float *scores_out, int64_t *indices_out);
int kpdi_group_pending_result_size(kpdi_group *g, int ticket, int64_t *n);
int kpdi_group_set_profiling(kpdi_group *g, int on);
int kpdi_group_reset_counters(kpdi_group *g);

/* ---- the launch planner, as data (csrc/plan.h; needs no GPU) -----------------
 * How a sweep of n_chunk dictionary patterns against m experimental patterns (k_kept pixels, keep_n) is laid on a
 * device of n_cu compute units: which f32 kernel (`form` -1 = the automatic choice, 0 = match.hip's 128-pattern
 * tiles, 3 = match16.hip's 256-pattern tiles), how many workgroups share a row block's dictionary tiles (nsplit), how
 * many row blocks a launch covers, each launch's XCD grid (and its padding), the tail plan.  The environment's
 * developer switches are read as kpdi_set_problem reads them. */
#define KPDI_PLAN_MAX_LAUNCHES 64
typedef struct kpdi_plan {
  int32_t form, tile;          /* kernel form (0 / 3) and its dictionary patterns per tile */
  int32_t row_blocks;          /* 256-pattern blocks of the experimental set */
  int32_t n_tiles, nsplit, rows_per_launch, launches;
  int64_t round_rows;          /* dictionary patterns one full round of the chip covers */
  int32_t n_main;              /* tiles of the main launch(es) */
  int32_t tail_tiles, tail_units, tail_nsplit, fixed_draws; /* match.hip: quarter-tile tail launch, fixed hand-out */
  int32_t tail_first, tail_shift;                           /* match16.hip f32: partial units from tile tail_first on */
  int32_t perm_rounds, perm_stride; /* match16.hip: round j < perm_rounds of split sp takes tile sp + nsplit * ((j * perm_stride)
                                       mod perm_rounds) - a low-discrepancy walk, so that the order of the dictionary
                                       (sampler order, sorted by score) does not matter to the fused top-k; 0 = natural order */
  int32_t tail_gemm_rows;           /* match16.hip f32: dictionary rows behind the whole rounds that tailgemm.hip takes as a kernel of
                                       its own (32 x 128 workgroups, scores -> select -> a merge source); then tail_shift = 0 */
  int32_t n_launch_desc;
  struct {
    int32_t row_first, rows, xcd_rows, xcd_splits, rows_grid;
  } launch[KPDI_PLAN_MAX_LAUNCHES];
} kpdi_plan;
int kpdi_plan_describe(int64_t m, int64_t n_chunk, int k_kept, int keep_n, int n_cu, int form, kpdi_plan *out);

/* ---- device buffers for callers that keep data resident (bench.py) -------- */
int kpdi_dev_alloc(kpdi_ctx *ctx, size_t bytes, void **d_out);
int kpdi_dev_free(kpdi_ctx *ctx, void *d_ptr);
int kpdi_h2d(kpdi_ctx *ctx, void *d_dst, const void *src, size_t bytes);
int kpdi_d2h(kpdi_ctx *ctx, void *dst, const void *d_src, size_t bytes);

/* ---- measurement ------------------------------------------------------------
 * kpdi_set_profiling(ctx, level): 0 off; 1 every phase of a sweep (preparation, match, merge, all-gather, ...) is
 * bracketed by HIP events on the context's stream; 2 only the match launches (and the all-gather) are - an event
 * record between two kernels leaves the GPU idle for ~6 us, 0.05 ms per step with level 1, which a 3 ms step
 * notices; 3 = level 1 + the fused top-k of match16.hip counts what its epilogues do (kpdi_counters.epi_*: a few
 * thousand atomics per launch, ~50 us - a developer level).  kpdi_get_counters() synchronises and sums the events. */
typedef struct kpdi_counters {
  double match_ms;      /* sum of match-kernel durations (HIP events) */
  int64_t match_launches;
  double match_flops;   /* 2 * M * n_chunk * K summed over launches (K = kept pixels) */
  double prep_ms;       /* dictionary + experimental normalisation kernels */
  double merge_ms;      /* top-k merge kernels */
  double h2d_bytes;     /* bytes copied host->device by push/set calls */
  int32_t match_grid;   /* workgroups of the last match launch */
  int32_t match_nsplit; /* dictionary splits of the last match launch */
  int32_t kpad;         /* padded reduction length */
  int32_t k_kept;       /* kept pixels K */
  double project_ms;    /* master-pattern projection kernels */
  double refine_ms;     /* refinement solve kernels */
  double preproc_ms;    /* background-removal kernels (incl. the fused preparation of the patterns) */
  int64_t preproc_launches;
  double rescore_ms;             /* KPDI_COMPUTE_F64: float64 rescoring + merge kernels */
  int64_t rescore_extra_passes;  /* ... screening passes beyond the first keep_n + 12 candidates of a chunk */
  int64_t uncertified_patterns;  /* ... (pattern, chunk) pairs whose best-k could not be certified; 0 in practice */
  int32_t match_form;            /* operand form of the last match launch: 0 match.hip f32, 1 split f16, 2 float16 (match16.hip),
                                    3 f32 on match16.hip's one-wave-per-SIMD kernel (chosen per sweep, KPDI_F32_WIDE forces) */
  int32_t comm_ranks;            /* ranks of the RCCL communicator (ncclCommCount), 0 = none attached */
  double comm_ms;                /* RCCL all-gather of the per-rank best-k lists inside kpdi_finalize (incl. waiting for the
                                    slowest rank to arrive) */
  double fixed_ms;               /* per-sweep bookkeeping kernels around the match: list / bound / counter initialisation */
  int32_t f64_certificate;       /* KPDI_COMPUTE_F64: 2 = worst-case bound (default), 1 = statistical bound (KPDI_F64_EPS=statistical
                                    at kpdi_set_problem); 0 = not float64 arithmetic.  `uncertified_patterns == 0` is a proof only for 2 */
  int32_t gather_ranks;          /* lists merged by the last finalize: RCCL ranks or peer-copied group members, 0 = this context's own only */
  int64_t coalesced_sweeps;      /* sweeps that took several small pushed chunks together (kpdi_push_dictionary_chunk: coalescing) */
  /* what the fused top-k of match16.hip did (collected at profiling level 1 only; per-lane lists: one per lane and 32
   * experimental patterns of a wave tile): lists that ran, candidates that passed the shared bound and were appended to
   * a lane's buffer, buffers that overflowed (the list is then built from the tile directly: the slow path), first
   * tiles that took that path because the bound was not complete in time */
  int64_t epi_lists;
  int64_t epi_appended;
  int64_t epi_overflows;
  int64_t epi_direct_first;
  double kinematical_ms;         /* the kernel of the last kpdi_kinematical_master_pattern, between two events (profiling on) */
  double geometrical_visibility_ms;   /* the kernels of the last kpdi_geometrical_visibility (profiling on) */
  double geometrical_coordinates_ms;  /* the kernels of the last kpdi_geometrical_coordinates, summed over its passes (profiling on) */
  double sampling_ms;            /* the kernels of the last kpdi_sample_fundamental_count or _fill: the passes it ran (profiling on) */
  double orientation_ms;         /* the kernels of the last kpdi_orientation_* call, summed over its passes (profiling on) */
} kpdi_counters;
/* sizeof(kpdi_counters) as the LIBRARY was built: a binding whose struct differs must refuse to call kpdi_get_counters
 * (the struct has grown between versions; kpdi_version() changes with it) */
size_t kpdi_counters_size(void);
int kpdi_set_profiling(kpdi_ctx *ctx, int on);
int kpdi_get_counters(kpdi_ctx *ctx, kpdi_counters *out);
int kpdi_reset_counters(kpdi_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* KPDI_H */
