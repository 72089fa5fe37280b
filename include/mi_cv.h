/*
 * mi_cv.h -- C ABI of the MI355X-native per-pixel CV kernel library (libmicv.so).
 *
 * Drop-in boundary for the cv::Mat-in / cv::Mat-out functions of
 * tanmaniac/IntroToComputerVision (paths below are relative to that repository).
 * Every entry point replaces one reference function; the header-only C++ shim in
 * introtocomputervision_amd/shim/micv_shim.hpp puts the reference's namespaces and
 * signatures (lk::, pyr::, harris::, sift::, cuda::, serial::) on top of these calls.
 *
 * Conventions
 *   - plain pointers + sizes; no C++ / torch / OpenCV types.
 *   - images are row-major, single channel; `*_stride` is the row pitch in BYTES
 *     (cv::Mat::step), must be a multiple of the element size.
 *   - `_dev` functions take DEVICE pointers, enqueue on `stream` (a hipStream_t, NULL =
 *     default stream) and do not synchronise; `_host` functions take HOST pointers, do
 *     H2D / D2H themselves and return after the result is in host memory (this is the
 *     behaviour of the reference's functions, which upload/download inside every call).
 *   - return value: MICV_OK (0) or a negative MICV_E* code; micv_last_error() returns a
 *     thread-local message.  Nothing calls exit() (the reference's checkCudaErrors does,
 *     common/include/common/CudaCommon.cuh:13-22).
 *   - a micv_ctx owns the device ordinal and a scratch arena that is reused between
 *     calls; use one ctx per host thread / stream (the reference's functions are not
 *     re-entrant either: global texture references, Harris.cu:28-31).
 */
#ifndef MI_CV_H
#define MI_CV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MICV_OK            0
#define MICV_EINVAL       -1   /* bad argument (size, stride, window, null pointer) */
#define MICV_EHIP         -2   /* HIP runtime error (message has hipGetErrorString) */
#define MICV_ENOMEM       -3   /* device allocation failed */
#define MICV_EUNSUPPORTED -4   /* valid in the reference but not implemented here */

typedef struct micv_ctx micv_ctx;
typedef void *micv_stream; /* hipStream_t */
typedef struct micv_comm micv_comm; /* a communicator over RCCL (multi-GPU entry points, below) */

const char *micv_version(void);
const char *micv_last_error(void);

int micv_ctx_create(int device, micv_ctx **out);
void micv_ctx_destroy(micv_ctx *ctx);
/* Bytes of device scratch currently held by the context. */
size_t micv_ctx_scratch_bytes(const micv_ctx *ctx);
/* Execution options of a context.  None of them changes a result: they select between kernels
 * that produce identical bits (tests compare the alternatives) or how a batch is scheduled.
 * The library reads NO environment variables. */
#define MICV_OPT_LK_STREAM_GROUPS  1 /* stream groups a batch is split into: 0 = default (1), 1..4 */
#define MICV_OPT_LK_FORCE_GENERIC  2 /* LK through the generic kernels: 1 = two or four launches per level by size (as for windows the fused kernels do not cover), 2 = always four, 3 = always two */
#define MICV_OPT_LK_NARROW_TILES   3 /* win-15 level kernel: 256-thread tiles instead of 512 */
#define MICV_OPT_SOBEL_GENERIC     4 /* Sobel through the generic row / column passes */
#define MICV_OPT_HARRIS_GENERIC    5 /* Harris response: one-thread-per-pixel kernel */
#define MICV_OPT_NMS_SCAN          6 /* Harris NMS: scanning kernel instead of the separable one */
#define MICV_OPT_STEREO_ROWS       7 /* rows per stereo strip: 0 = automatic, 8 or 10 */
#define MICV_OPT_LK_CHAIN          8 /* fused LK tile chains: 0 = pairs of tiles only for launches a little over one or two rounds of workgroups (default), 1 = never, n = longest chain (<= 32), -1 = schedule only */
#define MICV_OPT_LK_SHORT_TILES    9 /* win-15 level kernel, 64x16 tiles: 0 = up to 512 tiles (one round), n = up to n, -1 = never */
#define MICV_OPT_LK_STREAM         10 /* level kernel as a persistent grid that stages the next tile ahead: 1 = on, 0 = off (default; measured slower) */
#define MICV_OPT_LK_TALL_TILES     11 /* 1024-thread tiles, one workgroup per CU, for big launches: window 15 on 64x64 tiles only with 1 (measured slower); window 21 on 64x32 tiles by default (0 or 1; measured faster); 2 = window 15 on 32x64 tiles, 512 threads, two workgroups per CU; 3 = window 15 on 64x32 tiles, 1024 threads, eight waves per SIMD (r04 experiments, both measured slower: DESIGN.md section 5); -1 = never */
#define MICV_OPT_COMPACT_3PASS     12 /* ordered lists (corners, edge points, peak candidates, matches): 0 = one-launch chained scan up to 1 M elements, count / scan / emit launches beyond; 1 = always three launches; -1 = always one */
#define MICV_OPT_LK_DIRECT_LEVELS  13 /* fused LK: pyramid levels >= n read straight from level 0 with a pixel stride (n = 1: no pyramid-build launch): 0 = off (default: measured faster one pass at a time, slower with two passes in flight), n = 1..15 */
#define MICV_OPT_LK_BUILD_OVERLAP  14 /* fused LK, window 15, >= 3 levels: no pyramid-build launch -- the top level reads level 0 itself and the launch of every level k >= 2 carries the build of level k - 1 as extra workgroups behind its tiles: 0 = for single pairs only (default: the latency case; with several passes in flight a batch is faster with the build launch), -1 = never, 1 = for every batch */
#define MICV_OPT_LK_SPLIT          15 /* fused LK, window 15: a level launch SPLIT in two (r05, lk_split.hip) -- a pre-pass (pyrUp + warp + Sobel once per pixel, Ix / Iy / It into padded planes in HBM) plus a streaming window-sum kernel that carries its row-pass rows from block to block: 0 = never (default: measured 28-42 % slower than the fused launch, HBM traffic 2.4-3x), 1 = every whole-frame launch of at least 64 x 64 with a doubling coarse flow, 2 = 1 with the base flow through u, v, 3 = the pre-pass leaves only the warped image and the second half is the fused kernel in its no-flow mode */
#define MICV_OPT_LK_STRIP          16 /* fused LK, window 15: the INTERIOR tiles of a level launch as vertical strips that a workgroup streams down in blocks of 16 rows, carrying the last 14 row-pass rows of the five product fields and two warped rows from block to block (lk_strip.hpp) -- no vertical halo recomputation; the border tiles of the same launch stay tiles: 0 = off (default: 15 % fewer instructions, the same time -- DESIGN.md section 5), n > 0 = on with row segments of n blocks (16 = 256 rows); + 8192 = only for launches of 4096 tiles or more */
#define MICV_OPT_STEREO_EXACT      17 /* disparitySSD on 8-bit-valued images (integers 0..255 in both f32 images, radius <= 7; serial:: semantics radius <= 5): 0 = the exact-sum kernels (stereo_exact.hip: integer dot products, sliding window sums, lanes = disparities), chosen on the device per call by a pre-pass that tests every pixel (default); -1 = always the float kernels that add every window in the contract's order.  Same disparities either way: all sums are integers below 2^24, exact in f32 in any order.  (disparityNCorr always takes the float kernels; its u8 entries, micv_disparity_ncorr_u8_*, take the byte-reading float kernels of stereo_ncc_u8.hip.) */
#define MICV_OPT_STEREO_BATCH_MB   18 /* micv_disparity_ssd_u8_batch_dev: MiB of packed planes one launch may hold before the batch is processed in pieces: 0 = 64 (default), n = 1..4096; micv_disparity_ncorr_u8_batch_dev: the same bound on a launch's f32 window-energy planes (NCC, radius 1..10 without ROLLING) */
#define MICV_OPT_HARRIS_BATCH_MB   19 /* micv_harris_corners_u8_batch_dev: MiB of scratch (R planes the caller does not keep, mask words) one launch may hold before the batch is processed in pieces: 0 = 64 (default), n = 1..4096 */
#define MICV_OPT_COUNT            20
int micv_ctx_set_option(micv_ctx *ctx, int option, int value);
int micv_ctx_get_option(const micv_ctx *ctx, int option, int *value);

/* Device memory for callers that keep images resident between calls (the role cv::cuda::GpuMat's
 * allocator plays for the reference's GpuMat overloads, ps1_cpp/src/Hough.h:22-25,48-51,73-75).
 * Copies are blocking, like GpuMat::upload / download without a Stream; pitches in bytes. */
int micv_device_malloc(micv_ctx *ctx, size_t bytes, void **out);
void micv_device_free(micv_ctx *ctx, void *p);
int micv_memcpy2d_h2d(micv_ctx *ctx, void *dst, size_t dpitch, const void *src, size_t spitch,
                      size_t width_bytes, int rows);
int micv_memcpy2d_d2h(micv_ctx *ctx, void *dst, size_t dpitch, const void *src, size_t spitch,
                      size_t width_bytes, int rows);

/* ---------------------------------------------------------------- common/ (a17) ---- */
/* Kernel-timing log lines.  The reference brackets each kernel with a GpuTimer and logs
 * "<kernel> execution took {} ms" through spdlog (ps4_cpp/lib/Harris.cu:144-155,290;
 * ps2_cpp/lib/DisparitySSD.cu:192-203, DisparityNCorr.cu:236-247; ps1_cpp/src/Hough.cu:289,345,391;
 * ps5_cpp/lib/Pyramids.cu:69,123).  With a sink registered here (process-wide; NULL removes it), the
 * `_host` entry points of exactly those functions time their device call with an event pair and call
 * fn(kernel, ms, user) after their final synchronisation, `kernel` being the reference's kernel name
 * ("cornerResponseKernel", "refineCornersKernel", "disparitySSDKernel", "disparityNCorrKernel",
 * "houghLinesAccumulateKernel", "houghCirclesAccumulateKernel", "findLocalMaximaKernel",
 * "pyrDownsampleKernel", "pyrUpsampleKernel").  The shim formats the reference's lines from it
 * (micv_shim::log_kernel_times_to).  Costs nothing when no sink is set. */
typedef void (*micv_kernel_log_fn)(const char *kernel, float ms, void *user);
int micv_set_kernel_log(micv_kernel_log_fn fn, void *user);

/* common::warmup, common/src/CudaWarmup.cu:5-19 (10 blocks x 64 threads). */
int micv_warmup(micv_ctx *ctx, micv_stream stream);
/* common::divRoundUp, common/include/common/Utils.h:12-15: max(1, ceil(float(n)/float(d))). */
size_t micv_div_round_up(size_t num, size_t denom);
/* GpuTimer, common/include/common/GpuTimer.h:5-22 (event pair; stop() synchronises). */
typedef struct micv_timer micv_timer;
int micv_timer_create(micv_timer **out);
int micv_timer_start(micv_timer *t, micv_stream stream);
int micv_timer_stop(micv_timer *t, micv_stream stream);
int micv_timer_elapsed_ms(micv_timer *t, float *ms);
void micv_timer_destroy(micv_timer *t);

/* Per-launch timing of the pyramid-level kernels: the reference wraps every kernel launch in
 * a GpuTimer and logs "<kernel> took {} ms" (Pyramids.cu:61-69, Harris.cu:144-155); this is the
 * same measurement without the log.  While enabled, micv_lk_flow_pyr*_dev brackets each
 * pyramid level's launch(es) with an event pair on the caller's stream.
 * micv_profile_lk_level synchronises on those events and returns their summed duration. */
int micv_profile_enable(micv_ctx *ctx, int on);
int micv_profile_reset(micv_ctx *ctx);
int micv_profile_lk_level(micv_ctx *ctx, int level, double *total_ms, int64_t *launches);
/* Frame pairs covered by each profiled level launch: micv_lk_flow_pyr_batch_dev splits a batch
 * into groups that run on separate streams (MICV_OPT_LK_STREAM_GROUPS, default 1 = no split); the events bracket
 * the launches of the first group. */
int micv_profile_lk_pairs(micv_ctx *ctx, int *pairs_per_launch);
/* In-kernel phase stamps of the fused LK level kernel.  Compiled in only with -DMICV_DIAG (a
 * diagnostic build for timing studies; the default build returns MICV_EUNSUPPORTED when asked to
 * enable them): while enabled, wave 0 of every workgroup adds the s_memtime ticks it spent
 * in each phase to 16 device counters ([0..5] interior tiles, [8..13] border tiles: stage, pyrUp
 * rows, warp, gradients, window sums, solve).  Reads the counters into ticks16 (may be NULL),
 * then enables/disables and zeroes them.  Synchronises the device. */
int micv_profile_lk_phases(micv_ctx *ctx, int enable, uint64_t *ticks16);

/* --------------------------------------------------------- ps5: LK + pyramids ------ */

/* lk::calcOpticalFlowPyr, ps5_cpp/lib/OpticalFlow.cpp:122-167 (a1).  `levels` replaces
 * the hard-coded pyrDepth = 4 (:127).  Inputs are single-channel f32 (grey); u, v are
 * rows x cols f32.  win odd, 1..63. */
int micv_lk_flow_pyr_dev(micv_ctx *ctx, const float *prev, const float *next, int rows, int cols,
                         size_t stride, int win, int levels, float *u, float *v, size_t ostride,
                         micv_stream stream);
int micv_lk_flow_pyr_host(micv_ctx *ctx, const float *prev, const float *next, int rows, int cols,
                          size_t stride, int win, int levels, float *u, float *v, size_t ostride);
/* The same over `batch` independent frame pairs in one set of launches.  Pair i lives at
 * prev + i*pair_stride (bytes), likewise next / u / v with opair_stride. */
int micv_lk_flow_pyr_batch_dev(micv_ctx *ctx, const float *prev, const float *next, int batch,
                               size_t pair_stride, int rows, int cols, size_t stride, int win,
                               int levels, float *u, float *v, size_t opair_stride,
                               size_t ostride, micv_stream stream);

/* Row-sharded execution with a DECLARED bound on the vertical flow: a rank that holds
 * only band + margin rows of `next` must know when a flow value would make lk::warp read beyond them.
 * Sets bit 0 of *flag (device memory, zeroed by the caller) when |v| > bound or v is not finite anywhere in
 * rows [row_begin, row_end) of the `batch` fields (field i at v + i*pair_stride bytes); asynchronous on
 * `stream`, no host synchronisation.  introtocomputervision_amd/shard.py reruns the step with the whole
 * frame when the flag comes back set. */
int micv_flow_bound_check_dev(micv_ctx *ctx, const float *v, int batch, size_t pair_stride, int rows, int cols,
                              size_t stride, int row_begin, int row_end, float bound, uint32_t *flag,
                              micv_stream stream);

/* ------------------------------------------------- multi-GPU: one process per GPU, RCCL -------- */
/* SURVEY.md section 8e.  The reference has no multi-GPU code; its caller (`denseLKWrapper`,
 * ps5_cpp/src/Solution.cpp:60-64) is what these entry points let shard: every rank (one process per GPU) holds the
 * whole frames and computes a band of rows; the only dynamic exchange is the coarse-flow halo per pyramid level --
 * (win/2 + 2)/2 + 3 rows per neighbour -- sent point to point (ncclSend / ncclRecv in one group, on the launch
 * stream).  RCCL is loaded at run time (dlopen "librccl.so.1": libmicv.so itself links only libamdhip64, and a
 * process that already holds an RCCL shares it); without it these calls return MICV_EUNSUPPORTED.
 *
 * A communicator wraps an existing ncclComm_t (borrowed, e.g. the application's own) or is created from an RCCL
 * unique id: rank 0 calls micv_comm_unique_id, ships the MICV_COMM_ID_BYTES bytes to the other ranks by any means
 * (MPI, a file, torch.distributed), every rank calls micv_comm_create(ctx, NULL, id, rank, world, &comm) -- a
 * collective call, like ncclCommInitRank. */
#define MICV_COMM_ID_BYTES 128
int micv_comm_unique_id(void *id128);
int micv_comm_create(micv_ctx *ctx, void *nccl_comm, const void *unique_id128, int rank, int world, micv_comm **out);
int micv_comm_destroy(micv_comm *comm);
int micv_comm_rank(const micv_comm *comm, int *rank, int *world);
/* A communicator owns ONE device block (pyramids, per-level flow, exchange slabs) that every sharded call carves anew:
 * use a communicator from ONE stream at a time (calls on one stream queue up correctly; two streams would race on the
 * block silently), and with the context of the device it was created on (checked: MICV_EINVAL otherwise). */
/* Fabric check to run once before timing or trusting sharded results (collective, synchronises `stream`): a ring of
 * grouped ncclSend / ncclRecv of a rank-stamped 256 KB slab -- the row-shard driver's exchange pattern -- and one int32
 * sum all-reduce, both verified ON THE DEVICE.  MICV_OK, or MICV_EHIP with micv_last_error() naming the rank, the peer
 * and the step: a fabric or ordering failure then reads as such, not as a parity mismatch of the flow. */
int micv_comm_selftest(micv_ctx *ctx, micv_comm *comm, micv_stream stream);
/* The row plan, host only: rows [row_begin, row_end) of pyramid level `level` that `rank` of `world` computes
 * (the coarsest level is cut evenly, finer levels double the cuts), and optionally the rows of that level it
 * needs to compute the next finer one (its band + halo). */
int micv_rowshard_band(int rows, int cols, int levels, int world, int win, int rank, int level, int *row_begin,
                       int *row_end, int *need_begin, int *need_end);
/* lk::calcOpticalFlowPyr (OpticalFlow.cpp:122-167) of `batch` pairs, every pair split by rows over the ranks of
 * `comm`: this rank writes rows micv_rowshard_band(..., level 0) of u / v (full-size buffers) and nothing else.
 * prev / next: the whole frames on every rank.  Same bits as micv_lk_flow_pyr_batch_dev.  Collective: every rank
 * calls it with the same sizes.  Asynchronous on `stream`. */
int micv_lk_flow_pyr_rowshard_dev(micv_ctx *ctx, micv_comm *comm, const float *prev, const float *next, int batch,
                                  size_t pair_stride, int rows, int cols, size_t stride, int win, int levels,
                                  float *u, float *v, size_t opair_stride, size_t ostride, micv_stream stream);
/* The same plan, packing and band launches for `world` VIRTUAL ranks in this process on one device, the exchange
 * done by copies between the ranks' private slabs: whole u / v come back (every rank writes its band).  What a
 * one-GPU box can run at world sizes > 1; `poison` != 0 fills every rank's private memory with NaNs first, so a halo
 * row that was neither computed nor received shows up in the result.  Synchronises `stream` before it returns. */
int micv_lk_flow_pyr_rowshard_virtual_dev(micv_ctx *ctx, int world, const float *prev, const float *next, int batch,
                                          size_t pair_stride, int rows, int cols, size_t stride, int win, int levels,
                                          float *u, float *v, size_t opair_stride, size_t ostride, int poison,
                                          micv_stream stream);
/* The cv::Mat caller's form: host frames in, the WHOLE flow fields out on every rank (the bands are gathered
 * with one broadcast per rank and field); synchronous. */
int micv_lk_flow_pyr_rowshard_host(micv_ctx *ctx, micv_comm *comm, const float *prev, const float *next, int rows,
                                   int cols, size_t stride, int win, int levels, float *u, float *v, size_t ostride);
/* cuda::houghLinesAccumulate (Hough.cu:251-309) with the edge points sharded by rows: micv_hough_lines_band_dev
 * into this rank's private accumulator, then ONE int32 sum all-reduce in place -- the only real collective of the
 * whole path; integer sums make it bit-exact in any order.  acc: rho_bins x theta_bins on every rank. */
int micv_hough_lines_rowshard_dev(micv_ctx *ctx, micv_comm *comm, const uint8_t *mask_band, int band_rows, int cols,
                                  size_t mstride, int row0, int rows, unsigned rho_bin, unsigned theta_bin,
                                  int32_t *acc, micv_stream stream);
int micv_allreduce_sum_i32_dev(micv_ctx *ctx, micv_comm *comm, int32_t *buf, size_t count, micv_stream stream);

/* Diagnostic, host only (no device call): the work list the optional chain / streamed launches of the
 * level kernel walk (MICV_OPT_LK_CHAIN, MICV_OPT_LK_STREAM) for a rows x cols level of `batch` pairs.
 * Entry i = (tile x, first tile y, tiles in the chain, pair), 0 tiles = padding; tiles are
 * tile_w x tile_h pixels.  *count = entries of the list (also when entries_xycp is NULL or smaller).
 * Every tile of every pair must appear in exactly one entry -- tests/test_capi_and_host.py checks it. */
/* Diagnostic, no launch: the name (as rocprofv3 prints it, without the `micv::` prefix and the argument list) of the
 * kernel instantiation(s) the fused path launches for a rows x cols pyramid level of `batch` pairs with a doubling
 * coarse flow under this context's options -- answered by the launch dispatch itself, so that tools filtering profiler
 * rows by kernel name cannot drift from it.  cap >= 96. */
int micv_lk_level_kernel_name(micv_ctx *ctx, int win, int rows, int cols, int batch, char *buf, size_t cap);
int micv_lk_schedule_host(int rows, int cols, int batch, int win, int max_chain, int32_t *entries_xycp,
                          int64_t capacity, int64_t *count, int *tile_w, int *tile_h);

/* One iteration of the coarse-to-fine loop of lk::calcOpticalFlowPyr (OpticalFlow.cpp:135-163) on
 * one pyramid level, restricted to output rows [row_begin, row_end): the building block of
 * row-sharded execution (a rank owns a band of rows of every level and exchanges only coarse-flow
 * halo rows with its neighbours; introtocomputervision_amd/shard.py).  prev/next are the level's
 * images (rows x cols); flow_u/flow_v the coarser level's flow (flow_rows x flow_cols, dense pitch)
 * or NULL at the coarsest level.  Output rows outside the band are not written. */
int micv_lk_level_dev(micv_ctx *ctx, const float *prev, const float *next, int rows, int cols,
                      size_t stride, int win, const float *flow_u, const float *flow_v,
                      int flow_rows, int flow_cols, int row_begin, int row_end, float *u, float *v,
                      size_t ostride, micv_stream stream);
/* The same over `batch` pairs in one launch per level (pair i at prev + i*pair_stride bytes, its
 * coarse flow at flow_u + i*flow_pair_stride, its output at u + i*opair_stride): what a rank of a
 * row-sharded batch runs per level. */
int micv_lk_level_batch_dev(micv_ctx *ctx, const float *prev, const float *next, int batch,
                            size_t pair_stride, int rows, int cols, size_t stride, int win,
                            const float *flow_u, const float *flow_v, int flow_rows, int flow_cols,
                            size_t flow_pair_stride, int row_begin, int row_end, float *u, float *v,
                            size_t opair_stride, size_t ostride, micv_stream stream);

/* lk::calcOpticalFlow, OpticalFlow.cpp:41-104 (a2; includes computeGradients :12-39, a3). */
int micv_lk_flow_dev(micv_ctx *ctx, const float *prev, const float *next, int rows, int cols,
                     size_t stride, int win, float *u, float *v, size_t ostride,
                     micv_stream stream);
int micv_lk_flow_host(micv_ctx *ctx, const float *prev, const float *next, int rows, int cols,
                      size_t stride, int win, float *u, float *v, size_t ostride);

/* lk::warp, OpticalFlow.cpp:106-120 (a4).  src/du/dv/dst are rows x cols f32. */
int micv_lk_warp_dev(micv_ctx *ctx, const float *src, size_t sstride, const float *du,
                     const float *dv, size_t fstride, int rows, int cols, float *dst,
                     size_t dstride, micv_stream stream);
int micv_lk_warp_host(micv_ctx *ctx, const float *src, size_t sstride, const float *du,
                      const float *dv, size_t fstride, int rows, int cols, float *dst,
                      size_t dstride);

/* pyr::pyrDown, ps5_cpp/lib/Pyramids.cu:34-73 (a5): dst is (rows/2) x (cols/2). */
int micv_pyr_down_dev(micv_ctx *ctx, const float *src, int rows, int cols, size_t sstride,
                      float *dst, size_t dstride, micv_stream stream);
int micv_pyr_down_host(micv_ctx *ctx, const float *src, int rows, int cols, size_t sstride,
                       float *dst, size_t dstride);
/* pyr::pyrUp, Pyramids.cu:94-131 (a6): dst is (2 rows) x (2 cols). */
int micv_pyr_up_dev(micv_ctx *ctx, const float *src, int rows, int cols, size_t sstride,
                    float *dst, size_t dstride, micv_stream stream);
int micv_pyr_up_host(micv_ctx *ctx, const float *src, int rows, int cols, size_t sstride,
                     float *dst, size_t dstride);
/* pyr::makeGaussianPyramid, ps5_cpp/lib/Pyramids.cpp:5-26 (a7).  Level 0 is a copy of the
 * (grey f32) input; level l is (rows>>l) x (cols>>l), written densely (pitch = cols_l*4)
 * at dst_levels[l].  All levels are produced by one launch. */
int micv_gaussian_pyramid_dev(micv_ctx *ctx, const float *src, int rows, int cols, size_t sstride,
                              int levels, float *const *dst_levels, micv_stream stream);
int micv_gaussian_pyramid_host(micv_ctx *ctx, const float *src, int rows, int cols,
                               size_t sstride, int levels, float *const *dst_levels);
/* The grey planes AND the Gaussian pyramids of a frame sequence in ONE launch that reads the frames once (what
 * micv_lk_flow_seq_async runs in front of its level chain): nframes (1 .. 32768) device frames of one format, frame t at
 * frames + t*frame_pitch bytes, rows `stride` bytes apart, in the formats of micv_to_gray_f32_dev (8-bit frames at any
 * address and pitch; float frames 4-byte aligned).  gray + t*gray_pitch bytes receives frame t's dense grey plane (pitch
 * cols) with the bytes of micv_to_gray_f32_dev; dst_levels[l] + t*rows_l*cols_l floats, l = 1 .. levels - 1, level l of
 * its pyramid as micv_gaussian_pyramid_batch_dev lays it out and with its bytes (dst_levels[0] is not read: level 0 is
 * the grey plane).  A lane takes four pixels with 16-byte accesses when cols % 4 == 0 and every address and pitch keeps
 * the alignment, one pixel otherwise; the bytes are the same. */
int micv_gray_pyramid_seq_async(micv_ctx *ctx, const void *frames, size_t frame_pitch, int nframes, int rows, int cols, size_t stride,
                                int channels, int depth, int levels, float *gray, size_t gray_pitch, float *const *dst_levels,
                                micv_stream stream);
/* The Laplacian pyramid of sol::runProblem2, ps5_cpp/src/Solution.cpp:187-200 (SURVEY.md §8f row
 * N4): L_i = G_i - resize_if_smaller(pyrUp(G_{i+1})), L_{levels-1} = G_{levels-1}; level l is
 * (rows>>l) x (cols>>l), written densely at dst_levels[l].  Device-resident throughout. */
int micv_laplacian_pyramid_dev(micv_ctx *ctx, const float *src, int rows, int cols,
                               size_t sstride, int levels, float *const *dst_levels,
                               micv_stream stream);
/* The same for `batch` images in one launch (image i at src + i*image_stride bytes; level l of image i
 * at dst_levels[l] + i*rows_l*cols_l floats, dense; dst_levels[0] may be NULL = no level-0 copy).
 * row_begin / row_end (both NULL = everything): level l is written for rows
 * [row_begin[l], row_end[l]) only -- a rank of a row-sharded run builds just the rows its band and
 * halos touch. */
int micv_gaussian_pyramid_batch_dev(micv_ctx *ctx, const float *src, int batch, size_t image_stride,
                                    int rows, int cols, size_t sstride, int levels, float *const *dst_levels,
                                    const int *row_begin, const int *row_end, micv_stream stream);
/* cv::cvtColor(COLOR_RGB2GRAY) + convertTo(CV_32F) for 8-bit 3-channel input
 * (Pyramids.cpp:10-15). */
int micv_rgb8_to_gray_f32_dev(micv_ctx *ctx, const uint8_t *rgb, int rows, int cols,
                              size_t sstride, float *dst, size_t dstride, micv_stream stream);
/* The general form of the same step, as pyr::makeGaussianPyramid (Pyramids.cpp:9-15) and
 * denseLKWrapper (ps5_cpp/src/Solution.cpp:48-56) apply it to whatever cv::imread returned:
 * `channels` 1 (convertTo only), 3 or 4 interleaved samples per pixel (cv::cvtColor(COLOR_RGB2GRAY)
 * accepts both; alpha is ignored), `depth` MICV_DEPTH_8U (fixed-point weights 4899/9617/1868 >> 14,
 * rounded) or MICV_DEPTH_32F ((c0*0.299f + c1*0.587f) + c2*0.114f, unfused).  sstride in bytes. */
#define MICV_DEPTH_8U  0 /* CV_8U  */
#define MICV_DEPTH_8S  1 /* CV_8S: the disparity maps; a source depth of the "display" block only */
#define MICV_DEPTH_32F 5 /* CV_32F */
int micv_to_gray_f32_dev(micv_ctx *ctx, const void *src, int rows, int cols, size_t sstride,
                         int channels, int depth, float *dst, size_t dstride, micv_stream stream);
int micv_to_gray_f32_host(micv_ctx *ctx, const void *src, int rows, int cols, size_t sstride,
                          int channels, int depth, float *dst, size_t dstride);
/* lk::calcOpticalFlowPyr on the frames as the unchanged ps5 caller passes them: denseLKWrapper hands
 * the COLOUR frames to lk::calcOpticalFlowPyr (ps5_cpp/src/Solution.cpp:63) and
 * makeGaussianPyramid converts them (Pyramids.cpp:9-15).  One upload of the interleaved frames,
 * grey conversion on the device, then micv_lk_flow_pyr_dev. */
int micv_lk_flow_pyr_frames_host(micv_ctx *ctx, const void *prev, const void *next, int rows, int cols,
                                 size_t stride, int channels, int depth, int win, int levels, float *u,
                                 float *v, size_t ostride);
/* lk::calcOpticalFlowPyr over a sequence of frames: pairs (0, 1), (1, 2), ..., (nframes - 2, nframes - 1) -- the way
 * the ps5 driver walks the frames of a directory (ps5_cpp/lib/Config.cpp:17-46, src/Solution.cpp:255-285; frame t is
 * `next` of one lk::calcOpticalFlowPyr call and `prev` of the following one).  frames[t]: nframes host images of one
 * format (as micv_lk_flow_pyr_frames_host); u[p], v[p]: nframes - 1 host outputs, rows x cols f32, ostride bytes.
 * Every frame crosses PCIe once; upload of frame t + 2, the chain of pair t + 1 and the download of pair t run at
 * the same time (uploads on the calling thread, the chains on their own stream, downloads on two helper threads: a
 * copy from / to the caller's pageable memory occupies the thread that issues it).  Byte-identical to nframes - 1 calls
 * of micv_lk_flow_pyr_frames_host.  Blocking; one call at a time per context, like every other entry point. */
int micv_lk_flow_seq_host(micv_ctx *ctx, const void *const *frames, int nframes, int rows, int cols, size_t stride,
                          int channels, int depth, int win, int levels, float *const *u, float *const *v,
                          size_t ostride);
/* The same sequence on the DEVICE, all pairs as one batch.  frames: nframes (2 .. 32768) device frames of one format,
 * frame t at frames + t*frame_pitch bytes, rows `stride` bytes apart; the formats of micv_to_gray_f32_dev (1, 3 or 4
 * interleaved channels, MICV_DEPTH_8U or MICV_DEPTH_32F).  8-bit frames may have any address and any pitch; float frames
 * need a 4-byte aligned address, stride and frame_pitch.  frame_pitch >= (rows - 1)*stride + cols*channels*elem.  Pair p
 * is (frame p, frame p + 1); its fields are at u + p*opair_pitch and v + p*opair_pitch bytes, rows ostride bytes apart,
 * and hold the bytes that micv_to_gray_f32_dev on frames p and p + 1 followed by micv_lk_flow_pyr_dev(win, levels)
 * writes -- for every window, every level count that fits, and any max_pairs.
 *   One launch (seq_gray_pyr_kernel, pyramid.hip) reads the frames once and writes every frame's grey plane and every
 * level of its pyramid; the level chain then runs once for all pairs with `next` = `prev` one frame on, so a frame is
 * converted and decimated once although it is `next` of one pair and `prev` of the following one.  Single-channel float
 * frames are read where they lie (no grey plane).
 *   max_pairs bounds the scratch: a sequence with more pairs runs as pieces of max_pairs pairs (0 = 8, the measured point
 * of the batch) one after the other on the stream, piece i on frames [i*max_pairs, i*max_pairs + npairs_i]; the frame two
 * pieces share is converted twice, and the bytes do not depend on the cut.  micv_lk_flow_seq_plan (host only, no device)
 * returns that list: first_frame[i], npairs[i] for i < *npieces; a `cap` below the count gives MICV_EINVAL with the
 * count in *npieces.
 *   The call only enqueues on `stream`: nothing is read back, and the frames are not written.  A refusal enqueues
 * nothing.  The build-shaping experiment options
 * (MICV_OPT_LK_BUILD_OVERLAP, MICV_OPT_LK_DIRECT_LEVELS, MICV_OPT_LK_STREAM_GROUPS, MICV_OPT_LK_SPLIT) are NOT honoured
 * here; the tile options the level launches read from the context pass through as everywhere. */
int micv_lk_flow_seq_async(micv_ctx *ctx, const void *frames, size_t frame_pitch, int nframes, int rows, int cols,
                           size_t stride, int channels, int depth, int win, int levels, int max_pairs, float *u, float *v,
                           size_t opair_pitch, size_t ostride, micv_stream stream);
int micv_lk_flow_seq_plan(int nframes, int max_pairs, int *first_frame, int *npairs, int cap, int *npieces);
/* cv::resize(..., INTER_LINEAR) on f32 as used at OpticalFlow.cpp:149-150. */
int micv_resize_linear_dev(micv_ctx *ctx, const float *src, int srows, int scols, size_t sstride,
                           float *dst, int drows, int dcols, size_t dstride, micv_stream stream);

/* ------------------------------------------------------------- ps4: Harris --------- */

/* harris::getGradients, ps4_cpp/lib/Harris.cpp:14-41 (a8) and computeGradients,
 * OpticalFlow.cpp:12-39 (a3): Sobel pair, ksize in {1,3,5,7}, scale folded into the
 * smoothing taps (1 for Harris, 1/9 for LK). */
int micv_sobel_dev(micv_ctx *ctx, const float *src, int rows, int cols, size_t sstride, int ksize,
                   float scale, float *gx, float *gy, size_t gstride, micv_stream stream);
int micv_sobel_host(micv_ctx *ctx, const float *src, int rows, int cols, size_t sstride,
                    int ksize, float scale, float *gx, float *gy, size_t gstride);

/* harris::{cpu,gpu}::getCornerResponse, Harris.cpp:43-97 / Harris.cu:96-159 (a9). */
int micv_harris_response_dev(micv_ctx *ctx, const float *gx, const float *gy, int rows, int cols,
                             size_t gstride, int win, double sigma, float alpha, float *resp,
                             size_t rstride, micv_stream stream);
int micv_harris_response_host(micv_ctx *ctx, const float *gx, const float *gy, int rows, int cols,
                              size_t gstride, int win, double sigma, float alpha, float *resp,
                              size_t rstride);
/* The same with the arithmetic selected.  flags = 0: harris::gpu (Harris.cu:36-43,85-91: `fma.rn` accumulation in
 * (wy, wx) raster order, float `det - alpha tr^2`) -- the default of both functions above, because the reference's
 * configuration sets use_gpu: true (config/ps4.yaml:16).  MICV_HARRIS_CPU: harris::cpu::getCornerResponse as
 * written (ps4_cpp/lib/Harris.cpp:78-92): `secondMoment + weight * gradVals` is a multiply then an add per element,
 * cv::determinant is taken in double, `harrisScore * trace * trace` in float, and the difference is rounded to
 * float once.  Same window, weights, clamping and raster order. */
#define MICV_HARRIS_CPU 1
int micv_harris_response_ex_dev(micv_ctx *ctx, const float *gx, const float *gy, int rows, int cols,
                                size_t gstride, int win, double sigma, float alpha, int flags, float *resp,
                                size_t rstride, micv_stream stream);
int micv_harris_response_ex_host(micv_ctx *ctx, const float *gx, const float *gy, int rows, int cols,
                                 size_t gstride, int win, double sigma, float alpha, int flags, float *resp,
                                 size_t rstride);
/* harris::{cpu,gpu}::refineCorners, Harris.cpp:99-147 / Harris.cu:243-329 (a10).
 * corners: rows x cols f32, zero except kept maxima.  locs_yx: capacity `cap` (y,x) int32
 * pairs, filled in row-major order; *count receives the number found (may exceed cap).
 * The list follows Harris.cpp: every kept pixel, whatever its value (Harris.cu:301-306 lists only map entries > 0 and so
 * drops kept corners of value <= 0 when the threshold is <= 0).  min_distance 0 keeps every pixel >= threshold.
 * The _dev flavour leaves count/locs in device memory. */
int micv_harris_refine_dev(micv_ctx *ctx, const float *resp, int rows, int cols, size_t rstride,
                           double threshold, int min_distance, float *corners, size_t cstride,
                           int32_t *locs_yx, int64_t cap, int64_t *count, micv_stream stream);
int micv_harris_refine_host(micv_ctx *ctx, const float *resp, int rows, int cols, size_t rstride,
                            double threshold, int min_distance, float *corners, size_t cstride,
                            int32_t *locs_yx, int64_t cap, int64_t *count);

/* The ps4 caller's chain as ONE device call (harrisHelper, ps4_cpp/src/Solution.cpp:77-124: harris::getGradients ->
 * getCornerResponse -> refineCorners): image -> [gradients] -> R -> ordered corner list.  With a 3x3 Sobel and a window
 * of 3 / 5 / 7 the gradients are formed inside the response kernel's LDS tile (image in, R out: 8 B per pixel instead of
 * 12 + 12, two launches instead of three); other sizes run the three launches of the separate entry points.  Same bits
 * as micv_sobel_dev(scale 1) + micv_harris_response_ex_dev + micv_harris_refine_dev either way.
 * Optional outputs (NULL = not wanted): gx / gy (both or neither; sift::getKeypoints reads them), resp (R; context
 * scratch otherwise), corners (the sparse map harris::refineCorners also returns).  locs_yx / cap / count as
 * micv_harris_refine_dev; flags as micv_harris_response_ex_dev. */
int micv_harris_corners_dev(micv_ctx *ctx, const float *img, int rows, int cols, size_t stride, int sobel_ksize, int win,
                            double sigma, float alpha, int flags, double threshold, int min_distance, float *gx, float *gy,
                            size_t gstride, float *resp, size_t rstride, float *corners, size_t cstride, int32_t *locs_yx,
                            int64_t cap, int64_t *count, micv_stream stream);
int micv_harris_corners_host(micv_ctx *ctx, const float *img, int rows, int cols, size_t stride, int sobel_ksize, int win,
                             double sigma, float alpha, int flags, double threshold, int min_distance, float *gx, float *gy,
                             size_t gstride, float *resp, size_t rstride, float *corners, size_t cstride, int32_t *locs_yx,
                             int64_t cap, int64_t *count);

/* The same chain on 8-BIT images: what every ps4 call of the reference starts from (Solution::harrisHelper,
 * ps4_cpp/src/Solution.cpp:73-74, convertTo(CV_32F)s its picture only because harris::getGradients wants floats).
 * The arguments of micv_harris_corners_dev, with `img` bytes at a pitch of `stride` bytes (>= cols) and, before the
 * stream, kp_size / kp_xysa: the keypoints of sift::getKeypoints at the listed corners.
 *
 * Contract.  For every argument set micv_harris_corners_dev accepts (any Sobel size it accepts, any odd window <= 63,
 * MICV_HARRIS_CPU, any threshold including <= 0 and -inf, min_distance >= 0, cap below, at and above the count), every
 * requested output -- gx, gy, resp, corners, the first min(count, cap) rows of locs_yx, count -- is byte-identical to that
 * entry on the image converted to f32.  Batch element i is byte-identical to the single call on image i.
 * Keypoints: with kp_xysa non-NULL, its first min(count, cap) rows ([x, y, size, angle]) are byte-identical to
 * micv_sift_keypoints_dev(kp_size) on the f32 entry's gradient planes and list, whether or not gx / gy were requested;
 * rows past min(count, cap) are not written.  kp_xysa == NULL: no keypoints, kp_size is ignored.  A non-NULL kp_xysa
 * needs locs_yx.
 * Memory: the image pointer and pitch need NO alignment; output planes keep the f32 entry's rules (strides multiples
 * of 4, >= cols * 4).  No byte of an output plane outside rows x cols, no byte of a list outside the rows named above and
 * no byte between a batch's planes or lists is written; no byte of the input outside the `cols` bytes of each of its
 * `rows` rows is read (the image is read with byte loads only).  No entry synchronises the host.  batch < 1 is refused
 * with MICV_EINVAL and a message before anything runs, and so are outputs of one batch that overlap each other: a plane's
 * image is the (rows - 1) * stride + cols * 4 bytes from its first pixel, its image stride a multiple of 4 and at least
 * that (planes with one image stride may interleave), and locs_yx, count and kp_xysa are dense arrays of the batch.
 *
 * Dispatch, decided on the host:
 *   - 3 x 3 Sobel, window 3 / 5 / 7, neither MICV_OPT_HARRIS_GENERIC nor MICV_OPT_SOBEL_GENERIC (the fused form of
 *     micv_harris_corners_dev): the fused response kernel reads the bytes itself and converts them as it loads them.
 *     Device memory holds the bytes, R and what the caller asked for -- no f32 image, and no gradient plane unless
 *     requested: on bytes every 3 x 3 Sobel value is an integer of magnitude <= 1020, the same float in any evaluation
 *     order, so the one gradient sample a keypoint reads is recomputed at the corner from its 3 x 3 neighbourhood.
 *   - every other form: the image is converted to f32 in the context's scratch and handed to micv_harris_corners_dev,
 *     image by image; keypoints are then read from the gradient planes.
 *
 * Batch (fused form): `batch` images of one size, image i at img + i * image_stride bytes (any value), its planes at
 * i * {g,r,c}image_stride bytes; locs_yx is [batch][cap][2], count [batch] int64, kp_xysa [batch][cap][4].  Three
 * launches for the whole batch: the image is a grid dimension of the response launch and of the NMS launch, and the
 * ordered lists, counts and keypoints come from one launch with ONE workgroup per image, which walks that image's
 * rows * ceil(cols / 64) mask words in order -- no workgroup waits for another.  An image of more than 65536 such words
 * (4 Mpx at widths that are multiples of 64) takes the list step of micv_harris_refine_dev instead, one launch per
 * image, and one more launch for the keypoints; so does a batch of ONE image (and micv_harris_corners_u8_dev) above
 * 8192 words, where a single workgroup would be slower than that step.  A batch that does not keep resp needs rows * cols * 4 bytes of R per
 * image plus the mask words: past 64 MiB (MICV_OPT_HARRIS_BATCH_MB) it goes in pieces, one after the other on the
 * stream; a piece is as many images as keep within the bound, one at least and 65535 at most.  64 x 32 response tiles
 * are used when a launch (a piece) has 1024 of them or more, 64 x 16 otherwise; the bits do not depend on it. */
int micv_harris_corners_u8_dev(micv_ctx *ctx, const uint8_t *img, int rows, int cols, size_t stride, int sobel_ksize, int win,
                               double sigma, float alpha, int flags, double threshold, int min_distance, float *gx, float *gy,
                               size_t gstride, float *resp, size_t rstride, float *corners, size_t cstride, int32_t *locs_yx,
                               int64_t cap, int64_t *count, float kp_size, float *kp_xysa, micv_stream stream);
/* Uploads 1 B per pixel (micv_harris_corners_host: 4). */
int micv_harris_corners_u8_host(micv_ctx *ctx, const uint8_t *img, int rows, int cols, size_t stride, int sobel_ksize, int win,
                                double sigma, float alpha, int flags, double threshold, int min_distance, float *gx, float *gy,
                                size_t gstride, float *resp, size_t rstride, float *corners, size_t cstride, int32_t *locs_yx,
                                int64_t cap, int64_t *count, float kp_size, float *kp_xysa);
int micv_harris_corners_u8_batch_dev(micv_ctx *ctx, const uint8_t *img, size_t image_stride, int batch, int rows, int cols, size_t stride,
                                     int sobel_ksize, int win, double sigma, float alpha, int flags, double threshold, int min_distance,
                                     float *gx, float *gy, size_t gimage_stride, size_t gstride, float *resp, size_t rimage_stride,
                                     size_t rstride, float *corners, size_t cimage_stride, size_t cstride, int32_t *locs_yx, int64_t cap,
                                     int64_t *count, float kp_size, float *kp_xysa, micv_stream stream);

/* sift::getAnglesFromGradients, ps4_cpp/lib/Descriptors.cpp:7-25 (a11). */
int micv_sift_angles_dev(micv_ctx *ctx, const float *gx, const float *gy, int rows, int cols,
                         size_t gstride, float *angles, size_t astride, micv_stream stream);
int micv_sift_angles_host(micv_ctx *ctx, const float *gx, const float *gy, int rows, int cols,
                          size_t gstride, float *angles, size_t astride);
/* sift::getKeypoints, Descriptors.cpp:27-47 (a11): kp_xysa is [n][4] = x, y, size, angle. */
int micv_sift_keypoints_dev(micv_ctx *ctx, const float *gx, const float *gy, int rows, int cols,
                            size_t gstride, const int32_t *locs_yx, int64_t n, float size,
                            float *kp_xysa, micv_stream stream);
int micv_sift_keypoints_host(micv_ctx *ctx, const float *gx, const float *gy, int rows, int cols,
                             size_t gstride, const int32_t *locs_yx, int64_t n, float size,
                             float *kp_xysa);

/* The SIFT-style descriptor window at those keypoints: the step Solution::siftHelper runs next
 * (ps4_cpp/src/Solution.cpp:166-169, cv::xfeatures2d::SIFT::compute).  OpenCV's SIFT is third-party
 * code outside the reference tree (parity unpinned); this is its published per-keypoint algorithm
 * -- 4 x 4 spatial x 8 orientation bins, window rotated by the keypoint angle, bin width
 * 3 * size / 2 px, Gaussian weight, trilinear distribution, normalise -> clamp 0.2 -> renormalise to
 * 512 -> 8-bit values stored as float -- sampled on the harris::getGradients fields, with the
 * arithmetic fixed as DESIGN.md section 2 states (bit-exact between library and checker).
 * kp_xysa: n x {x, y, size, angle_deg} as micv_sift_keypoints writes them; desc: n rows of 128
 * floats, dstride bytes apart.  Keypoints without a positive finite size get an all-zero row. */
int micv_sift_descriptors_dev(micv_ctx *ctx, const float *gx, const float *gy, int rows, int cols,
                              size_t gstride, const float *kp_xysa, int64_t n, float *desc,
                              size_t dstride, micv_stream stream);
int micv_sift_descriptors_host(micv_ctx *ctx, const float *gx, const float *gy, int rows, int cols,
                               size_t gstride, const float *kp_xysa, int64_t n, float *desc,
                               size_t dstride);

/* The same descriptors from the 8-BIT image itself, the list length read on the device: what follows
 * micv_harris_corners_u8_batch_dev, which ends with device-resident keypoints and counts and keeps no gradient plane.
 * `img`: bytes at a pitch of `stride` bytes (>= cols).  kp_xysa: `cap` rows; count: a DEVICE word, or NULL for "all cap
 * rows".  The list length is n = min(max(*count, 0), cap): a count word above cap means cap, a negative one 0.
 *
 * Contract.  Bytes: row k < n of desc is byte-identical to micv_sift_descriptors_dev on the planes of
 * micv_sobel_dev(ksize 3, scale 1) of the image converted to f32, for every keypoint that entry accepts -- NaN or
 * infinite coordinates, a size <= 0 or not finite, angles outside [0, 360) and keypoints outside the picture included
 * (all-zero rows, as there).  The descriptor samples interior pixels only (0 < r < rows - 1, 0 < c < cols - 1), where a
 * 3 x 3 Sobel of bytes is an integer of magnitude <= 1020: the same float in any evaluation order, with no border rule;
 * the kernel recomputes it from the sample's eight neighbours.
 * Counts: rows at and past n are not written.  Batch: element i is byte-identical to the single call on image i with
 * list i.  kp_xysa is [batch][cap][4], count [batch] int64 (or NULL), image i at img + i * image_stride bytes (any value),
 * its descriptor block at desc + i * dimage_stride bytes.
 * Input reads: the image is read with byte loads only; its pointer, pitch and image stride need no alignment; nothing
 * outside the `cols` bytes of each of its `rows` rows is read.  Output writes: desc follows the f32 entry's rules (dstride
 * a multiple of 4, >= 512); nothing outside the 128 floats of a written row and nothing between a batch's descriptor
 * blocks is written.
 * Host and device state: no entry synchronises the host or reads a count there.  Device memory holds the bytes, the
 * lists and the descriptors: no f32 image, no gradient plane, no context scratch.
 * Refusals (MICV_EINVAL and a message, before anything is enqueued): batch < 1 or > 65535; descriptor blocks of one batch
 * that overlap (dimage_stride not a multiple of 4 or below (cap - 1) * dstride + 512); the f32 entry's size limits (cap
 * < 2^33, rows and cols <= 65535, dstride / 4 < 2^30).
 *
 * Kernel.  The descriptor body of the f32 entry on a byte source; the grid is sized from cap x batch, and a workgroup
 * whose keypoint index is at or past its image's n leaves as a whole.  Every sample's eight neighbours are byte loads
 * from the image (L1 / L2 hits within a window).  Copying a keypoint's window of up to 109 x 109 bytes to LDS first was
 * measured and lost in every case (11.9 KB per keypoint cost occupancy at 2 and 1 waves per keypoint and the copy was
 * never repaid; profiles/sift_u8/staged_experiment.jsonl), so there is no such form.
 * Waves per keypoint: the host cannot see n, so the f32 entry's rule (4 below 1800 keypoints, 2 below 6144, else 1) is
 * applied inside the kernel to n x batch, n the list length of the workgroup's own image.  The host launches every form a
 * list of at most cap rows can pick (one when count is NULL, up to three otherwise, a form's grid covering the longest
 * list that picks it) and the workgroups of the forms that do not apply leave at once.  The bytes do not depend on
 * the number of waves. */
int micv_sift_descriptors_u8_dev(micv_ctx *ctx, const uint8_t *img, int rows, int cols, size_t stride, const float *kp_xysa, int64_t cap,
                                 const int64_t *count, float *desc, size_t dstride, micv_stream stream);
/* n host rows; uploads 1 B per pixel (micv_sift_descriptors_host: 8). */
int micv_sift_descriptors_u8_host(micv_ctx *ctx, const uint8_t *img, int rows, int cols, size_t stride, const float *kp_xysa, int64_t n,
                                  float *desc, size_t dstride);
int micv_sift_descriptors_u8_batch_dev(micv_ctx *ctx, const uint8_t *img, size_t image_stride, int batch, int rows, int cols, size_t stride,
                                       const float *kp_xysa, int64_t cap, const int64_t *count, float *desc, size_t dimage_stride,
                                       size_t dstride, micv_stream stream);

/* ------------------------------------------------------------- ps2: stereo --------- */

#define MICV_STEREO_COLS_2R     1 /* window of (2r+1) rows x 2r columns, DisparitySSD.cu:84 */
#define MICV_STEREO_MIN_SSD_5E6 2 /* leave -1 where best SSD >= 5e6, DisparitySSD.cu:16 */
#define MICV_STEREO_SERIAL      4 /* serial::disparitySSD as written (DisparitySSD.cpp:35-61):
                                     per-term round() into an int sum, search clamped to the padded
                                     image, best = (99999999, 0) initially.  SSD only, and alone:
                                     with COLS_2R, MIN_SSD_5E6 or ROLLING the call fails with
                                     MICV_EINVAL before anything runs (the function has a (2r+1)^2
                                     window and no threshold). */
#define MICV_STEREO_ROLLING     8 /* column sums as the CUDA kernels keep them (DisparitySSD.cu:97-138,
                                     DisparityNCorr.cu:117-173): strips of ROWS_PER_THREAD = 40 rows;
                                     a strip's first row sums its 2r+1 terms top -> bottom from 0, each
                                     further row subtracts the term that left the window from the
                                     previous row's sum, then adds the one that entered.  Same result
                                     as the fresh sums on integer-valued images; on general f32 the
                                     two round differently.  Runs a slower, strip-serial kernel. */

/* cuda::disparitySSD / serial::disparitySSD, ps2_cpp/lib/DisparitySSD.cu:143-207 and
 * DisparitySSD.cpp:9-62 (a12).  disp is rows x cols int8 (CV_8SC1), dstride in bytes.
 * flags = 0: CUDA-path semantics with the window corrected to (2r+1)^2 columns (clamp-to-edge
 * addressing, every d in [min,max] tried in ascending order, strict '<').
 * flags = COLS_2R | MIN_SSD_5E6 | ROLLING: the CUDA kernel as written, source order of operations,
 * no contraction (COLS_2R | MIN_SSD_5E6 alone keeps its window and threshold but sums every row's
 * columns afresh -- identical on integer-valued images).  flags = SERIAL: the CPU function exactly as
 * written. */
int micv_disparity_ssd_dev(micv_ctx *ctx, const float *left, const float *right, int rows,
                           int cols, size_t stride, int window_rad, int min_disparity,
                           int max_disparity, int flags, int8_t *disp, size_t dstride,
                           micv_stream stream);
int micv_disparity_ssd_host(micv_ctx *ctx, const float *left, const float *right, int rows,
                            int cols, size_t stride, int window_rad, int min_disparity,
                            int max_disparity, int flags, int8_t *disp, size_t dstride);
/* disparitySSD on 8-BIT images: what every stereo call of the reference starts from (main.cpp:87-88 loads 8-bit pictures
 * and convertTo(CV_32FC1)s them only because cuda::disparitySSD asserts CV_32FC1, DisparitySSD.cu:149-150).
 *
 * Contract.  For every argument set micv_disparity_ssd_dev accepts (the same refusals, radius 0..31, all four flags), disp
 * is byte-identical to micv_disparity_ssd_dev on the two images converted to f32.  Each image has its own row pitch in
 * bytes (>= cols); pointers and pitches need NO alignment (a cv::Mat ROI of an 8-bit image starts at any byte).  Bytes of
 * disp outside rows x cols (row padding) are not written.  No entry synchronises the host.
 *
 * Dispatch, decided on the host before anything is enqueued:
 *   - radius 1..7, except SERIAL at radius 6 and 7 and COLS_2R at radius 1: the exact-sum kernels (stereo_exact.hip), from a
 *     pre-pass that packs the bytes as they are -- no eligibility test, no write to the context's flag word, no float tiles
 *     in the search launch; the call neither depends on nor disturbs the flag word of f32 calls on other streams.
 *     (That removes one hazard, not the rule: calls that may overlap still need a context each, for the scratch arena.)  ROLLING is
 *     served by the same kernels with the flag stripped (ROLLING | COLS_2R: the COLS_2R form; otherwise the full window):
 *     the rolling column sums differ from the fresh ones only in the order of their roundings, and on bytes with a window
 *     of at most 15 x 15 every sum is an integer below 2^24 -- exact in f32 in any order.
 *   - everything else (radius 0 or > 7, SERIAL at radius 6 and 7, COLS_2R at radius 1, MICV_OPT_STEREO_EXACT = -1): the
 *     pair is converted to f32 in the context's scratch by a small kernel and handed to micv_disparity_ssd_dev.
 *
 * Batch: `batch` pairs of one size, pair i at base + i * pair_stride (bytes; any value for the inputs, the disparity maps
 * must not overlap), searched in ONE pre-pass and ONE search launch whose tiling sees the strips of all pairs -- a batch of
 * small images fills the device where a single one cannot.  Element i is byte-identical to the single call on pair i;
 * the gaps between the maps are not written.  Scratch: the packed planes of all pairs of a launch come from the context's
 * arena, roughly 12 B per pixel and pair (16 B with MIN_SSD_5E6); a batch whose planes pass 64 MiB
 * (MICV_OPT_STEREO_BATCH_MB) is processed in pieces.  A piece is as many pairs as keep its planes -- sized with the tiling
 * the piece itself gets -- within the bound, one pair at least (a single pair may be larger than the bound) and at most 32768
 * eight-row strips; the shorter last piece is tiled as the full ones, so no launch holds more than a full piece does. */
int micv_disparity_ssd_u8_dev(micv_ctx *ctx, const uint8_t *left, size_t lstride, const uint8_t *right, size_t rstride,
                              int rows, int cols, int window_rad, int min_disparity, int max_disparity, int flags,
                              int8_t *disp, size_t dstride, micv_stream stream);
/* Uploads 1 B per pixel and image (micv_disparity_ssd_host: 4). */
int micv_disparity_ssd_u8_host(micv_ctx *ctx, const uint8_t *left, size_t lstride, const uint8_t *right, size_t rstride,
                               int rows, int cols, int window_rad, int min_disparity, int max_disparity, int flags,
                               int8_t *disp, size_t dstride);
int micv_disparity_ssd_u8_batch_dev(micv_ctx *ctx, const uint8_t *left, size_t lpair_stride, size_t lstride,
                                    const uint8_t *right, size_t rpair_stride, size_t rstride, int batch, int rows, int cols,
                                    int window_rad, int min_disparity, int max_disparity, int flags, int8_t *disp,
                                    size_t dpair_stride, size_t dstride, micv_stream stream);
/* disparityNCorr on 8-BIT images, with the arguments of the SSD u8 entries above (main.cpp:227-229, 304-306 convertTo(CV_32FC1)
 * only because cuda::disparityNCorr asserts that type).
 *
 * Contract.  For every argument set micv_disparity_ncorr_dev accepts (radius 0..31; COLS_2R, MIN_SSD_5E6, ROLLING; SERIAL is
 * refused with MICV_EINVAL before anything runs), disp is byte-identical to micv_disparity_ncorr_dev on the two images
 * converted to f32.  Each image has its own row pitch in bytes (>= cols); pointers and pitches need NO alignment.  Bytes of
 * disp outside rows x cols, and the gaps between a batch's maps, are not written.  No entry synchronises the host, and none
 * reads or writes the context's stereo flag word.  batch < 1 and overlapping maps are refused with MICV_EINVAL.
 *
 * Dispatch, decided on the host:
 *   - radius 1..10 without ROLLING (the tile forms): the float search itself reads the bytes (stereo_ncc_u8.hip) -- one
 *     launch for the window energy of `right`, one for the search, bytes converted to f32 as they are staged in registers
 *     and LDS.  Device memory holds the bytes and one f32 energy plane per pair (the context's arena), no f32 image.  On
 *     bytes every operand is in the range of the short exact sqrt / division (ncc_arith.hpp), so that form is compiled in
 *     and the per-value range tracking of the f32 kernel is not.
 *   - radius 0, 11..31 and ROLLING: the pair is converted to f32 in the context's scratch and handed to
 *     micv_disparity_ncorr_dev, pair by pair.
 *
 * Batch: the pair is a grid dimension of both launches.  Element i is byte-identical to the single call on pair i.  A
 * batch whose energy planes pass 64 MiB (MICV_OPT_STEREO_BATCH_MB) goes in pieces, one after the other on the stream: a
 * piece is as many pairs as keep its planes within the bound, one at least and 65535 at most. */
int micv_disparity_ncorr_u8_dev(micv_ctx *ctx, const uint8_t *left, size_t lstride, const uint8_t *right, size_t rstride,
                                int rows, int cols, int window_rad, int min_disparity, int max_disparity, int flags,
                                int8_t *disp, size_t dstride, micv_stream stream);
/* Uploads 1 B per pixel and image (micv_disparity_ncorr_host: 4). */
int micv_disparity_ncorr_u8_host(micv_ctx *ctx, const uint8_t *left, size_t lstride, const uint8_t *right, size_t rstride,
                                 int rows, int cols, int window_rad, int min_disparity, int max_disparity, int flags,
                                 int8_t *disp, size_t dstride);
int micv_disparity_ncorr_u8_batch_dev(micv_ctx *ctx, const uint8_t *left, size_t lpair_stride, size_t lstride,
                                      const uint8_t *right, size_t rpair_stride, size_t rstride, int batch, int rows, int cols,
                                      int window_rad, int min_disparity, int max_disparity, int flags, int8_t *disp,
                                      size_t dpair_stride, size_t dstride, micv_stream stream);
/* cuda::disparityNCorr, ps2_cpp/lib/DisparityNCorr.cu:177-251 (a13). */
int micv_disparity_ncorr_dev(micv_ctx *ctx, const float *left, const float *right, int rows,
                             int cols, size_t stride, int window_rad, int min_disparity,
                             int max_disparity, int flags, int8_t *disp, size_t dstride,
                             micv_stream stream);
int micv_disparity_ncorr_host(micv_ctx *ctx, const float *left, const float *right, int rows,
                              int cols, size_t stride, int window_rad, int min_disparity,
                              int max_disparity, int flags, int8_t *disp, size_t dstride);

/* -------------------------------------------------------------- ps1: Hough --------- */

/* Accumulator shape of cuda::houghLinesAccumulate, ps1_cpp/src/Hough.cu:258-263. */
int micv_hough_lines_dims(int rows, int cols, unsigned rho_bin, unsigned theta_bin,
                          int *rho_bins, int *theta_bins);
/* cuda::houghLinesAccumulate, Hough.cu:251-309 (a14): mask u8 -> acc i32 [rho_bins x theta_bins]
 * (dense, zeroed here). */
int micv_hough_lines_dev(micv_ctx *ctx, const uint8_t *mask, int rows, int cols, size_t mstride,
                         unsigned rho_bin, unsigned theta_bin, int32_t *acc, micv_stream stream);
int micv_hough_lines_host(micv_ctx *ctx, const uint8_t *mask, int rows, int cols, size_t mstride,
                          unsigned rho_bin, unsigned theta_bin, int32_t *acc);
/* cuda::houghCirclesAccumulate, Hough.cu:311-364 (a15): acc i32 [rows x cols] (dense, zeroed
 * here -- the reference forgets to, Hough.cu:318). */
int micv_hough_circles_dev(micv_ctx *ctx, const uint8_t *mask, int rows, int cols, size_t mstride,
                           unsigned radius, int32_t *acc, micv_stream stream);
int micv_hough_circles_host(micv_ctx *ctx, const uint8_t *mask, int rows, int cols,
                            size_t mstride, unsigned radius, int32_t *acc);
/* Row-sharded forms: `mask` points at row `row0` of a `rows`-row image and holds
 * `band_rows` rows; votes of those edge points go into a full-size (zeroed here) accumulator.
 * Integer sums of the per-shard accumulators (RCCL all-reduce) equal the unsharded accumulator
 * bit for bit.  The unsharded entry points are these with row0 = 0, band_rows = rows. */
int micv_hough_lines_band_dev(micv_ctx *ctx, const uint8_t *mask, int band_rows, int cols,
                              size_t mstride, int row0, int rows, unsigned rho_bin,
                              unsigned theta_bin, int32_t *acc, micv_stream stream);
int micv_hough_circles_band_dev(micv_ctx *ctx, const uint8_t *mask, int band_rows, int cols,
                                size_t mstride, int row0, int rows, unsigned radius, int32_t *acc,
                                micv_stream stream);
/* cuda::findLocalMaxima, Hough.cu:366-426 (a16): peaks_rc receives up to num_peaks (row,col)
 * pairs ordered by votes descending (stable); *count = number written. */
int micv_hough_peaks_dev(micv_ctx *ctx, const int32_t *acc, int rows, int cols,
                         unsigned num_peaks, int threshold, uint32_t *peaks_rc, int64_t *count,
                         micv_stream stream);
int micv_hough_peaks_host(micv_ctx *ctx, const int32_t *acc, int rows, int cols,
                          unsigned num_peaks, int threshold, uint32_t *peaks_rc, int64_t *count);

/* ------------------------------ ps1: edge front-end ------------ */

/* sol::generateEdge, ps1_cpp/src/Solution.cpp:21-47, on a single-channel 8-bit image: Gaussian
 * blur (cv::cuda::createGaussianFilter, odd size <= 31; size 1 = identity) then Canny with Sobel
 * aperture 3 and the L1 gradient norm; edges = 255 / 0.  The hysteresis pass reads one device
 * flag per round, so this entry point SYNCHRONISES `stream` (OpenCV's CUDA Canny does the same
 * with its queue counter). */
int micv_generate_edge_dev(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t stride,
                           int gauss_size, double gauss_sigma, double low_thresh, double high_thresh,
                           uint8_t *edges, size_t estride, micv_stream stream);
int micv_generate_edge_host(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t stride,
                            int gauss_size, double gauss_sigma, double low_thresh,
                            double high_thresh, uint8_t *edges, size_t estride);

/* ------------------------------ ps1: circle search over a radius range ----------------- */

/* The radius loops of the ps1 driver (ps1_cpp/src/main.cpp:173-180, :263-270, :299-307): for every radius r in
 * [min_radius, max_radius], what micv_hough_circles_dev(r) followed by micv_hough_peaks_dev(num_peaks, threshold) gives --
 * the votes of Hough.cu:85-93 and the peak rule of Hough.cu:148-157 with its exclusive upper bounds, peaks ordered by
 * (votes descending, index ascending).  peaks_rc is u32 [n_radii][num_peaks][2] (row, col), counts i64 [n_radii] =
 * min(num_peaks, candidates) (device memory in the _dev form); rows of peaks_rc past a radius' count are unspecified.
 * acc, when not NULL, receives the accumulators, i32 [n_radii][rows][cols].  The edge-point list is built once, one grid
 * covers (tile, radius), and with num_peaks <= 64 and acc == NULL no accumulator is written to memory: every tile
 * applies the threshold and the peak rule on chip and hands on at most num_peaks keys.  The _dev form does not
 * synchronise.  min_radius > max_radius is zero radii: MICV_OK, nothing written.  rows, cols <= 32767, num_peaks <= 4096. */
int micv_hough_circles_range_peaks_dev(micv_ctx *ctx, const uint8_t *mask, int rows, int cols, size_t mstride,
                                       unsigned min_radius, unsigned max_radius, unsigned num_peaks, int threshold,
                                       uint32_t *peaks_rc, int64_t *counts, int32_t *acc, micv_stream stream);
int micv_hough_circles_range_peaks_host(micv_ctx *ctx, const uint8_t *mask, int rows, int cols, size_t mstride,
                                        unsigned min_radius, unsigned max_radius, unsigned num_peaks, int threshold,
                                        uint32_t *peaks_rc, int64_t *counts, int32_t *acc);

/* ------------------------------ ps1: pre-processing -------------------------------------- */

/* sol::gaussianBlur, ps1_cpp/src/Solution.cpp:49-61, on CV_8UC1: cv::cuda::createGaussianFilter with
 * getGaussianKernel(size, sigma, CV_32F) taps (odd size <= 31, sigma > 0), BORDER_REFLECT_101, row pass then column
 * pass, each an fmaf chain from +0 with the taps ascending; round half to even and saturate at the end (the blur stage
 * of micv_generate_edge_*). */
int micv_gaussian_blur_u8_dev(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t sstride, int gauss_size,
                              double gauss_sigma, uint8_t *dst, size_t dstride, micv_stream stream);
int micv_gaussian_blur_u8_host(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t sstride, int gauss_size,
                               double gauss_sigma, uint8_t *dst, size_t dstride);
/* The same on CV_32FC1 (main.cpp:102, :144): float in, float out, no rounding. */
int micv_gaussian_blur_f32_dev(micv_ctx *ctx, const float *src, int rows, int cols, size_t sstride, int gauss_size,
                               double gauss_sigma, float *dst, size_t dstride, micv_stream stream);
int micv_gaussian_blur_f32_host(micv_ctx *ctx, const float *src, int rows, int cols, size_t sstride, int gauss_size,
                                double gauss_sigma, float *dst, size_t dstride);
/* sol::generateEdge, Solution.cpp:21-47, as it runs on CV_32FC1 input (main.cpp:98, :107): the float blur, convertTo(CV_8U)
 * = saturate_cast<uchar>(cvRound(v)) with cvRound half to even and NaN, +-inf and everything outside int -> INT_MIN -> 0
 * (DESIGN.md section 2), then the Canny stages of micv_generate_edge_dev.  SYNCHRONISES `stream` as that call does. */
int micv_generate_edge_f32_dev(micv_ctx *ctx, const float *src, int rows, int cols, size_t stride, int gauss_size,
                               double gauss_sigma, double low_thresh, double high_thresh, uint8_t *edges, size_t estride,
                               micv_stream stream);
int micv_generate_edge_f32_host(micv_ctx *ctx, const float *src, int rows, int cols, size_t stride, int gauss_size,
                                double gauss_sigma, double low_thresh, double high_thresh, uint8_t *edges,
                                size_t estride);

/* ------------------------------ ps1: edges without a host wait, and a batch ------------------ */

/* The entries above stop the host: their hysteresis is a loop of launches that ends when a polled word says so.  The
 * `_async` entries below compute the same bytes with a FIXED sequence of launches, whatever the pixels are: the
 * hysteresis is connected-component labelling of weak | strong with a lock-free union-find over horizontal runs of the
 * bit planes (init, union, mark, emit: DESIGN.md "Hysteresis without the host").  No word is read on the host and no
 * workgroup waits for another, so they ENQUEUE ON `stream` AND RETURN WITHOUT WAITING for the device; they may sit in a
 * captured stream once the context's arena has the size (a first call of the shape outside the capture sees to that:
 * growing the arena synchronises).  As everywhere in this library a context is used from one stream at a time: the arena
 * is shared.  A refusal enqueues nothing.  rows * cols >= 2^31 is MICV_EINVAL (labels are 32-bit pixel indices).
 * Scratch per image: rows * cols bytes (blur), 2 * rows * ceil(cols / 64) words (bit planes), 4 * rows * cols bytes (parents).
 *
 * micv_hysteresis_u8: the stage on its own.  cand and strong are byte masks, non-zero = set, each plane with its own pitch
 * and any address; edges = 255 where the pixel lies in an 8-connected component of cand | strong that holds a strong
 * pixel (a strong pixel outside cand counts), 0 elsewhere. */
int micv_hysteresis_u8_async(micv_ctx *ctx, const uint8_t *cand, size_t cstride, const uint8_t *strong, size_t sstride, int rows,
                             int cols, uint8_t *edges, size_t estride, micv_stream stream);
int micv_hysteresis_u8_host(micv_ctx *ctx, const uint8_t *cand, size_t cstride, const uint8_t *strong, size_t sstride, int rows, int cols,
                            uint8_t *edges, size_t estride);
/* micv_generate_edge_dev / micv_generate_edge_f32_dev without the wait: the same arguments accepted and refused, the same
 * bytes. */
int micv_generate_edge_async(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t stride, int gauss_size, double gauss_sigma,
                             double low_thresh, double high_thresh, uint8_t *edges, size_t estride, micv_stream stream);
int micv_generate_edge_f32_async(micv_ctx *ctx, const float *src, int rows, int cols, size_t stride, int gauss_size, double gauss_sigma,
                                 double low_thresh, double high_thresh, uint8_t *edges, size_t estride, micv_stream stream);
/* `batch` images of one size, image i at src + i * image_bytes, its edges at edges + i * edges_image_bytes: element i holds
 * the bytes of micv_generate_edge_dev on image i.  The image is a grid dimension of every launch.  A batch whose scratch
 * (above, per image) passes scratch_mb MiB (0 = 64) goes in pieces of as many images as fit, one at least, one after the
 * other on the stream.  batch >= 1; the images of a batch must not overlap. */
int micv_generate_edge_batch_async(micv_ctx *ctx, const uint8_t *src, int batch, size_t image_bytes, int rows, int cols, size_t stride,
                                   int gauss_size, double gauss_sigma, double low_thresh, double high_thresh, uint8_t *edges,
                                   size_t edges_image_bytes, size_t estride, int scratch_mb, micv_stream stream);
/* The same on host memory: per-image pointers and pitches (cv::Mat ROIs go in as they are); one upload block, one batch
 * call, one download block.  Synchronous, as every _host entry. */
int micv_generate_edge_batch_host(micv_ctx *ctx, const uint8_t *const *srcs, const size_t *strides, int batch, int rows, int cols,
                                  int gauss_size, double gauss_sigma, double low_thresh, double high_thresh, uint8_t *const *edges,
                                  const size_t *estrides);

/* cv::erode with cv::getStructuringElement(MORPH_ELLIPSE, Size(ksize, ksize)), main.cpp:246-248, :282-284; ksize odd,
 * 1..7.  Row i of the footprint (dy = i - r, r = ksize / 2) has half-width cvRound(r * sqrt((r*r - dy*dy) / r*r)), 0 when
 * r = 0; anchor at the centre; BORDER_CONSTANT with morphologyDefaultBorderValue(): a tap outside the image is FLT_MAX
 * (f32) or 255 (u8).  The minimum is v = first tap, then v = (x < v) ? x : v over the footprint in raster order: a NaN
 * after the first tap never replaces, and of -0 / +0 the earlier one stays. */
int micv_erode_ellipse_f32_dev(micv_ctx *ctx, const float *src, int rows, int cols, size_t sstride, int ksize, float *dst,
                               size_t dstride, micv_stream stream);
int micv_erode_ellipse_f32_host(micv_ctx *ctx, const float *src, int rows, int cols, size_t sstride, int ksize, float *dst,
                                size_t dstride);
int micv_erode_ellipse_u8_dev(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t sstride, int ksize,
                              uint8_t *dst, size_t dstride, micv_stream stream);
int micv_erode_ellipse_u8_host(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t sstride, int ksize,
                               uint8_t *dst, size_t dstride);

/* ------------------------------ ps1: after the peaks ------------------------------------- */

/* sol::findParallelLines, Solution.cpp:134-173: of the first min(*count, max_peaks) (row, col) pairs of peaks_rc
 * (max_peaks <= 4096), those whose key (row / delta_rho * delta_rho, col / delta_theta * delta_theta) -- unsigned
 * integer division -- is shared by at least one other pair.  ORDER: the pairs come out in INPUT order; the reference
 * emits them in the bucket order of libstdc++'s unordered_multimap, which is no property of the algorithm (every use
 * draws the result in one colour, so no image depends on it).  delta_rho == 0 or delta_theta == 0 is MICV_EINVAL
 * (the reference divides by zero).  out_rc holds up to max_peaks pairs; `count`, `out_count` are device words in the _dev form. */
int micv_parallel_lines_dev(micv_ctx *ctx, const uint32_t *peaks_rc, const int64_t *count, unsigned max_peaks,
                            unsigned delta_rho, unsigned delta_theta, uint32_t *out_rc, int64_t *out_count,
                            micv_stream stream);
int micv_parallel_lines_host(micv_ctx *ctx, const uint32_t *peaks_rc, int64_t count, unsigned delta_rho,
                             unsigned delta_theta, uint32_t *out_rc, int64_t *out_count);
/* cv::cvtColor(CV_GRAY2RGB) (main.cpp:88, :130, :167, :262, :298) of a MICV_DEPTH_8U or MICV_DEPTH_32F image to 8-bit,
 * three interleaved channels; f32 goes through the saturate_cast<uchar> rule of micv_generate_edge_f32_*.  (The
 * reference draws into a float image that cv::imwrite converts; converting first and drawing 8-bit colour gives the same file.) */
int micv_gray_to_rgb8_dev(micv_ctx *ctx, const void *src, int depth, int rows, int cols, size_t sstride, uint8_t *dst,
                          size_t dstride, micv_stream stream);
int micv_gray_to_rgb8_host(micv_ctx *ctx, const void *src, int depth, int rows, int cols, size_t sstride, uint8_t *dst,
                           size_t dstride);
/* sol::rowColToRhoTheta + sol::drawLinesParametric, Solution.cpp:81-123, for the first min(*count, max_peaks) (row, col)
 * peaks: rho = row * rho_bin - diag (diag of micv_hough_lines_dims), theta = col * theta_bin - 90, the end points of
 * Solution.cpp:95-112 in float (sin / cos: the correctly rounded double function of the float radian, cast to float),
 * Point2f -> Point by lrintf, then cv::line, thickness 1, LINE_8, as micv_viz::line walks it (one thread per major-axis
 * step inside the image).  img is 8-bit, three interleaved channels, rows x cols; color = 3 bytes in memory order.
 * Peaks with col * theta_bin >= 180 are not drawn. */
int micv_draw_lines_parametric_dev(micv_ctx *ctx, uint8_t *img, int rows, int cols, size_t stride,
                                   const uint32_t *peaks_rc, const int64_t *count, unsigned max_peaks, unsigned rho_bin,
                                   unsigned theta_bin, const uint8_t *color, micv_stream stream);
int micv_draw_lines_parametric_host(micv_ctx *ctx, uint8_t *img, int rows, int cols, size_t stride,
                                    const uint32_t *peaks_rc, int64_t count, unsigned rho_bin, unsigned theta_bin,
                                    const uint8_t *color);
/* sol::drawCircles, Solution.cpp:125-132, for the peaks of micv_hough_circles_range_peaks_*: peaks_rc u32
 * [n_radii][num_peaks][2] (row, col), counts i64 [n_radii], circle j < min(counts[i], num_peaks) of radius index i has
 * centre (col, row) and radius min_radius + i.  cv::circle, thickness 1, as its midpoint walk, every
 * pixel bounds-checked.  Centres beyond 65535 in either coordinate are not drawn. */
int micv_draw_circles_dev(micv_ctx *ctx, uint8_t *img, int rows, int cols, size_t stride, const uint32_t *peaks_rc,
                          const int64_t *counts, unsigned n_radii, unsigned num_peaks, unsigned min_radius,
                          const uint8_t *color, micv_stream stream);
int micv_draw_circles_host(micv_ctx *ctx, uint8_t *img, int rows, int cols, size_t stride, const uint32_t *peaks_rc,
                           const int64_t *counts, unsigned n_radii, unsigned num_peaks, unsigned min_radius,
                           const uint8_t *color);

/* --------------------------- ps4: descriptor matching ----------- */

/* cv::BFMatcher::create()->knnMatch(query, train, matches, 2), ps4_cpp/src/Solution.cpp:172-179:
 * NORM_L2, no cross-check.  query is nq x dim, train nt x dim (f32, strides in bytes, nt >= 2).
 * idx2 [nq][2] = train indices of the nearest and second nearest, dist2 [nq][2] their distances,
 * ordered by (distance, index).  +inf is a distance like any other.  A NaN distance is never selected: with fewer than
 * two non-NaN distances the empty places hold index -1 and distance +inf (an all-NaN train set: both). */
int micv_bf_knn2_dev(micv_ctx *ctx, const float *query, int nq, size_t qstride, const float *train,
                     int nt, size_t tstride, int dim, int32_t *idx2, float *dist2,
                     micv_stream stream);
int micv_bf_knn2_host(micv_ctx *ctx, const float *query, int nq, size_t qstride, const float *train,
                      int nt, size_t tstride, int dim, int32_t *idx2, float *dist2);
/* The same match with both lengths read on the DEVICE: nq = min(max(*nq_count, 0), nq_cap), nt likewise (nq_cap,
 * nt_cap >= 1).  Rows < nq of idx2 / dist2 hold the bytes of micv_bf_knn2_dev(nq, nt) when nt >= 2; with nt < 2 the empty
 * places hold index -1 and distance +inf, as in the all-NaN case above.  Rows in [nq, nq_cap) hold {-1, -1} and
 * {+inf, +inf}, so micv_bf_ratio_filter_dev over nq_cap rows never keeps them and returns the matches and the count of
 * the sliced run.  Query rows at and past nq and train rows at and past nt are not read.  The grid, the train slices and
 * the scratch are sized from the caps; nothing is read back. */
int micv_bf_knn2_counted_dev(micv_ctx *ctx, const float *query, int nq_cap, size_t qstride, const int64_t *nq_count, const float *train,
                             int nt_cap, size_t tstride, const int64_t *nt_count, int dim, int32_t *idx2, float *dist2,
                             micv_stream stream);
/* The ratio test of Solution.cpp:180-184: keep query q when dist0 < ratio * dist1.  matches_qt
 * [cap][2] = (queryIdx, trainIdx) in query order, distances [cap]; *count (device) = number kept.  The compare is
 * double(dist0) < ratio * double(dist1): a query with one finite distance (dist1 = +inf) is kept, one with none is not. */
int micv_bf_ratio_filter_dev(micv_ctx *ctx, const int32_t *idx2, const float *dist2, int nq,
                             double ratio, int32_t *matches_qt, float *distances, int64_t cap,
                             int64_t *count, micv_stream stream);
int micv_bf_ratio_filter_host(micv_ctx *ctx, const int32_t *idx2, const float *dist2, int nq,
                              double ratio, int32_t *matches_qt, float *distances, int64_t cap,
                              int64_t *count);
/* Matcher and ratio test on a BATCH OF PAIRS of one descriptor batch, two launches for the whole batch, nothing read back.
 * desc holds `images` lists of `cap` rows x dim f32 (row r of image i at desc + i*dimage_stride + r*dstride, bytes; what
 * micv_sift_descriptors_u8_batch_dev leaves), count [images] their DEVICE lengths (clamped to [0, cap]; NULL: all cap
 * rows), pairs [npairs][2] int32 on the DEVICE: (query image, train image).  Element p of every output holds the bytes of
 * micv_bf_knn2_counted_dev(query = image pairs[p][0], train = image pairs[p][1], their count words, nq_cap = nt_cap = cap)
 * followed by micv_bf_ratio_filter_dev over cap rows with capacity mcap:
 *   idx2, dist2 [npairs][cap][2]  optional, both or neither;
 *   match_count [npairs]          the total kept, which may exceed mcap;
 *   matches_qt [npairs][mcap][2], distances [npairs][mcap]: rows < min(match_count[p], mcap); the rows at and past that
 *                                 are not written (mcap == 0: counts only, both may be NULL).
 * A pair may name one image twice, pairs may repeat, (a, b) and (b, a) may both appear.  A pair index outside [0, images)
 * behaves as two empty lists: idx2 / dist2 rows {-1, -1} / {+inf, +inf}, match_count[p] = 0.
 * Slicing of the train set: a launch has S = min(ceil(2048 / (ceil(cap / 64) * npairs)), ceil(cap / 128)) slices (at
 * least 1, and no more than keep ONE pair's partial lists within the bound below), and a pair's slice holds ceil(ceil(nt / 128) / S) * 128 rows of ITS clamped train count nt, read on the
 * device -- a short list spreads over as many workgroups as it has 128-row passes, not over slice 0 alone.  The top-2
 * order (distance, index) is total, so no byte depends on S.  The partial top-2 lists (16 * S * cap bytes per pair) are
 * bounded at 64 MiB per launch: larger batches go in pieces on the stream.  One workgroup per pair folds the slices,
 * applies the ratio test and compacts in query order; no workgroup waits for another, and neither compact_state nor the
 * context's status words are touched.
 * Errors (MICV_EINVAL, before anything is enqueued): a null ctx / desc / pairs / match_count, one of idx2 / dist2
 * without the other, images < 1, npairs outside 1 .. 65535, cap < 1, dim < 1, mcap < 0 or mcap > 0 without matches_qt
 * and distances, a dstride that is no multiple of 4 or below dim * 4, a dimage_stride that is no multiple of 4 or below
 * (cap - 1) * dstride + dim * 4. */
int micv_bf_match_pairs_dev(micv_ctx *ctx, const float *desc, int images, size_t dimage_stride, int cap, size_t dstride,
                            const int64_t *count, int dim, const int32_t *pairs, int npairs, double ratio, int32_t *idx2,
                            float *dist2, int32_t *matches_qt, float *distances, int64_t mcap, int64_t *match_count,
                            micv_stream stream);

/* ------------------------------------------------------------- ps4: RANSAC --------- */

/* ransac::solve, ps4_cpp/lib/RANSAC.cpp:27-152 (called from Solution::ransacHelper,
 * ps4_cpp/src/Solution.cpp:214-242), with the arithmetic DESIGN.md section 2 fixes.  type is the
 * reference's TransformType value, which is also the sample size k. */
#define MICV_RANSAC_TRANSLATION 1
#define MICV_RANSAC_SIMILARITY  2
#define MICV_RANSAC_AFFINE      3

/* The reference's sampler (RANSAC.cpp:11-13,20-25,39-40,53): one std::mt19937 seeded once from
 * std::seed_seq(seed_words, seed_words + nwords) (Config.cpp:85-99; the config default is the one
 * word 1; seed_words == NULL leaves the engine default-constructed, as before any ransac::seed),
 * and per solve call a fresh iota index vector that every iteration std::shuffle's in place,
 * WITHOUT resetting it between iterations; the sample of iteration i is the first k entries
 * of the vector after i + 1 shuffles.  Host-side, libstdc++'s std::shuffle, no device work.
 *   samples:     iters x k indices of the next solve over n points; the generator is NOT advanced.
 *   permutation: the whole index vector after iteration `iter` (0-based) of that solve; not advanced.
 *   advance:     consumes `iterations` shuffles of n points -- what a solve that ran that many
 *                iterations consumed -- so the next call sees the next solve's samples. */
typedef struct micv_ransac_rng micv_ransac_rng;
int micv_ransac_rng_create(const uint32_t *seed_words, int nwords, micv_ransac_rng **out);
void micv_ransac_rng_destroy(micv_ransac_rng *rng);
int micv_ransac_rng_samples(const micv_ransac_rng *rng, int64_t n, int k, int iters, int32_t *samples);
int micv_ransac_rng_permutation(const micv_ransac_rng *rng, int64_t n, int iter, int32_t *perm);
int micv_ransac_rng_advance(micv_ransac_rng *rng, int64_t n, int iterations);

/* One solve on the device with the caller's samples (iters x k int32, device; iteration i uses
 * samples[i*k .. i*k+k-1]).  src_xy / dst_xy: n x {x, y} f32 (device), 1 <= n <= 2^30.
 * Iteration i scores the hypothesis of its sample against every point whose index is not in the
 * sample; the run stops after the first i with (double)count_i / (double)n >= min_ratio, or after
 * iters iterations.  min_ratio <= 0 runs no iteration, as the reference's while loop.
 * Outputs (device):
 *   transforms [2][6] f32: [0] the LAST iteration's 2x3 transform -- what the reference returns --
 *                          [1] the best iteration's (first maximum of count); zeros when none ran;
 *   inlier_mask [n] u8:    1 where the best iteration counted the point (original indices);
 *   stats [3] i32:         {iterations, best_iter (-1 when none ran), best_count}.
 * The reference's consensusSet is the sorted positions, in the best iteration's permutation, of
 * the points the mask marks (micv_ransac_rng_permutation); its ratio is best_count / n.
 * A sample index outside [0, n) makes stats = {-1, -1, 0} and every output zero.
 * Errors (MICV_EINVAL, before anything is enqueued): n < k, a bad type, iters < 1, thresh < 0,
 * min_ratio NaN, a null pointer. */
int micv_ransac_solve_dev(micv_ctx *ctx, const float *src_xy, const float *dst_xy, int64_t n,
                          const int32_t *samples, int iters, int type, int thresh, double min_ratio,
                          float *transforms, uint8_t *inlier_mask, int32_t *stats, micv_stream stream);
/* The same with host pointers (the sample indices are checked here): upload, solve, download, sync. */
int micv_ransac_solve_host(micv_ctx *ctx, const float *src_xy, const float *dst_xy, int64_t n,
                           const int32_t *samples, int iters, int type, int thresh, double min_ratio,
                           float *transforms, uint8_t *inlier_mask, int32_t *stats);

/* The device-resident end of the ps4 chain: the points of Solution::ransacHelper
 * (Solution.cpp:222-225: src = kp_a[queryIdx].xy, dst = kp_b[trainIdx].xy) gathered from the
 * outputs of micv_sift_keypoints_dev (kp_a [na][4], kp_b [nb][4]) and micv_bf_ratio_filter_dev
 * (matches_qt [cap][2] and the DEVICE *count, read on the device: n = min(*count, cap)), then the
 * solve above.  No host round trip.  Since n is not known on the host this form draws its own
 * samples -- NOT the reference's sequence: for iteration i, draw j = 0 .. k-1, attempt a = 0, 1, ..
 *     r   = splitmix64(seed ^ ((uint64)i << 32 | (uint64)j << 30 | a))
 *     idx = ((r >> 32) * n) >> 32                       (64-bit product)
 * and the first attempt whose idx differs from the sample's earlier entries is entry j.
 * splitmix64(x): z = x + 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *                z = (z ^ z >> 27) * 0x94D049BB133111EB; return z ^ z >> 31.
 * inlier_mask has cap entries (zero at and above n).  n < k on the device gives stats = {0, -1, 0}
 * and zero outputs; a match index outside kp_a / kp_b gives stats = {-1, -1, 0}. */
int micv_ransac_solve_matches_dev(micv_ctx *ctx, const float *kp_a, int64_t na, const float *kp_b,
                                  int64_t nb, const int32_t *matches_qt, const int64_t *count,
                                  int64_t cap, uint64_t seed, int iters, int type, int thresh,
                                  double min_ratio, float *transforms, uint8_t *inlier_mask,
                                  int32_t *stats, micv_stream stream);
/* The same solve on a BATCH OF PAIRS: one memset, one gather over (match, pair), one score launch over (hypothesis
 * chunk, pair) and one finalize launch with a workgroup per pair, whatever npairs is.  kp_xysa holds `images` lists of kcap
 * keypoint rows (image i at kp_xysa + i*kimage_stride bytes), pairs [npairs][2] int32 on the DEVICE as for
 * micv_bf_match_pairs_dev, whose matches_qt [npairs][mcap][2] and match_count [npairs] go straight in.  Element p of
 * transforms [npairs][2][6], inlier_mask [npairs][mcap] and stats [npairs][3] holds the bytes of
 * micv_ransac_solve_matches_dev(kp_a = image pairs[p][0], na = kcap, kp_b = image pairs[p][1], nb = kcap, pair p's
 * matches and count word, cap = mcap, seed_p) with
 *     seed_p = splitmix64(seed + p)          (64-bit addition, wrapping; splitmix64 as written above).
 * The sampler xors the seed with the draw's counter word, so seed + p alone would hand pair p + 1 the draws of pair p
 * under another counter; the hash keeps adjacent pairs' draws apart.  Control words, stop words and count rows are per
 * pair: n < k gives that pair {0, -1, 0}, a match index outside the lists gives it {-1, -1, 0} and zero outputs, and its
 * neighbours are not affected.  A pair index outside [0, images) gives {-1, -1, 0} and zero outputs.
 * Errors: those of micv_ransac_solve_matches_dev, images < 1, npairs outside 1 .. 65535, a kimage_stride that is no
 * multiple of 4 or below kcap * 16. */
int micv_ransac_solve_pairs_dev(micv_ctx *ctx, const float *kp_xysa, int images, size_t kimage_stride, int64_t kcap,
                                const int32_t *pairs, int npairs, const int32_t *matches_qt, const int64_t *match_count,
                                int64_t mcap, uint64_t seed, int iters, int type, int thresh, double min_ratio,
                                float *transforms, uint8_t *inlier_mask, int32_t *stats, micv_stream stream);

/* -------------------------------------------------------- ps4: registration --------- */

/* The tail of Solution::runProblem3 (ps4_cpp/src/Solution.cpp:315-325 for the similarity, :344-354 for the affine
 * case): cv::invertAffineTransform(transform, transform), cv::warpAffine(simB, reverseWarp, transform, size) and
 * blended = simA * 0.5 + reverseWarp * 0.5 (ps4-3-d, ps4-3-e).  Single-channel images of depth MICV_DEPTH_8U (the
 * parity case: BasicConfig.h:61 reads the images 8-bit) or MICV_DEPTH_32F; strides in bytes; rows, cols <= 32767
 * on both sides (cv::remap's int16 cell).  A 2x3 transform is six f32, row-major.  The `_dev` forms read it from
 * DEVICE memory and never synchronise, so `transforms` of micv_ransac_solve_*_dev goes straight in (row [0] is what
 * the reference returns).  OpenCV's source is not available to this repository: the arithmetic below is a decision
 * of this library that restates OpenCV 3.4.1's imgwarp.cpp (unpinned; DESIGN.md section 2, "ps4 registration").
 *
 * cv::invertAffineTransform, all in double from the float entries, unfused, each result rounded once to float:
 *   D = m0*m4 - m1*m3;  D = D != 0 ? 1/D : 0;  A11 = m4*D, A22 = m0*D, A12 = -m1*D, A21 = -m3*D;
 *   b1 = -A11*m2 - A12*m5, b2 = -A21*m2 - A22*m5;  inv = {A11, A12, b1, A21, A22, b2}.
 * `count` transforms, one lane each; count == 0 is a no-op. */
int micv_invert_affine_dev(micv_ctx *ctx, const float *m, int count, float *inv, micv_stream stream);
int micv_invert_affine_host(micv_ctx *ctx, const float *m, int count, float *inv);

/* cv::warpAffine(src, dst, M, dsize, flags) with BORDER_CONSTANT 0.  flags = 0 is INTER_LINEAR with M mapping
 * src -> dst (it is inverted again, in double); MICV_WARP_INVERSE_MAP uses M as the dst -> src map as given;
 * MICV_WARP_NEAREST is INTER_NEAREST.  With cvRound = round half to even, INT_MIN for NaN or out of range, and
 * int32 arithmetic that wraps:
 *   X0(y) = cvRound((M1*y + M2)*1024) + d,  Y0(y) = cvRound((M4*y + M5)*1024) + d,
 *   X = (X0 + cvRound(M0*x*1024)) >> s,     Y = (Y0 + cvRound(M3*x*1024)) >> s,    (d, s) = (16, 5) linear, (512, 10) nearest;
 *   linear:  cell (sat16(X >> 5), sat16(Y >> 5)), fraction (X & 31, Y & 31) / 32; the four taps p00 p01 p10 p11, 0 outside;
 *            u8:  (sum w*p + 16384) >> 15 with w = (32-fx)(32-fy)*32, fx(32-fy)*32, (32-fx)fy*32, fx*fy*32;
 *            f32: p00*(ay0*ax0) + p01*(ay0*ax1) + p10*(ay1*ax0) + p11*(ay1*ax1), left to right, unfused -- the blend
 *                 of micv_lk_warp (outside taps are 0.f and still multiplied: 0 * inf = NaN);
 *   nearest: the pixel at (sat16(X), sat16(Y)), 0 outside.
 * dst (drows x dcols) may differ in size from src; src == dst is an error.  One launch. */
#define MICV_WARP_INVERSE_MAP 16 /* cv::WARP_INVERSE_MAP */
#define MICV_WARP_NEAREST     1  /* INTER_NEAREST instead of INTER_LINEAR */
int micv_warp_affine_dev(micv_ctx *ctx, const void *src, int depth, int srows, int scols, size_t sstride, const float *m,
                         int flags, void *dst, int drows, int dcols, size_t dstride, micv_stream stream);
int micv_warp_affine_host(micv_ctx *ctx, const void *src, int depth, int srows, int scols, size_t sstride, const float *m,
                          int flags, void *dst, int drows, int dcols, size_t dstride);
/* `count` warps in ONE launch: image i (src + i*src_pitch_bytes) by transform i (m + 6 i) into dst + i*dst_pitch_bytes
 * -- a sequence registered to a key frame; src_pitch_bytes == 0 warps one shared source by `count` transforms.
 * Same bits as `count` single calls.  count == 0 is a no-op. */
int micv_warp_affine_batch_dev(micv_ctx *ctx, const void *src, size_t src_pitch_bytes, int depth, int srows, int scols,
                               size_t sstride, const float *m, int count, int flags, void *dst, size_t dst_pitch_bytes,
                               int drows, int dcols, size_t dstride, micv_stream stream);

/* a * alpha + b * beta [+ gamma] on cv::Mat's = cv::addWeighted(a, alpha, b, beta, gamma): alpha, beta, gamma rounded to
 * float, t = (a*alpha + b*beta) + gamma in float, unfused; f32 stores t, u8 stores cvRound(t) (ties to even) saturated to
 * 0..255.  With alpha = beta = 0.5, gamma = 0 on u8 -- the only case the reference exercises (Solution.cpp:325,354) --
 * every term is exact, so any evaluation order gives these bits.  dst may alias a or b. */
int micv_add_weighted_dev(micv_ctx *ctx, const void *a, size_t astride, double alpha, const void *b, size_t bstride,
                          double beta, double gamma, int depth, int rows, int cols, void *dst, size_t dstride,
                          micv_stream stream);
int micv_add_weighted_host(micv_ctx *ctx, const void *a, size_t astride, double alpha, const void *b, size_t bstride,
                           double beta, double gamma, int depth, int rows, int cols, void *dst, size_t dstride);

/* Solution.cpp:315-325 as ONE launch: m_a_to_b (what ransacHelper returns: it maps simA's points onto simB's) is
 * inverted, b is warped back onto a (flags 0) and blended = a*0.5 + warped*0.5, the warped pixel staying in registers
 * unless `warped` (optional, NULL = not wanted) asks for it.  Same bytes as micv_invert_affine + micv_warp_affine +
 * micv_add_weighted.  a, b, warped, blended: rows x cols of `depth`. */
int micv_register_blend_dev(micv_ctx *ctx, const void *a, size_t astride, const void *b, size_t bstride, int depth, int rows,
                            int cols, const float *m_a_to_b, void *warped, size_t wstride, void *blended, size_t ostride,
                            micv_stream stream);
int micv_register_blend_host(micv_ctx *ctx, const void *a, size_t astride, const void *b, size_t bstride, int depth, int rows,
                             int cols, const float *m_a_to_b, void *warped, size_t wstride, void *blended, size_t ostride);

/* ------------------------------------------------------------------ display -------- */

/* The step that ends almost every runProblem* of the reference, on the device:
 *   cv::normalize(x, x, 0, 255, cv::NORM_MINMAX, CV_8U)      ps2 main.cpp:94-320, ps4 Solution.cpp:67,108, ps5 :74-75,124
 *   ones * 255 - x                                            ps2 main.cpp:126-127
 *   cv::applyColorMap(x, x, cv::COLORMAP_JET)                 ps5 Solution.cpp:76-77
 * and ps2's driver around it: addNoise (main.cpp:140-153), the contrast gain (:191-193), the left / right pair
 * (:21-78).  OpenCV's source is not available to this repository: the arithmetic is a decision of this library that
 * restates OpenCV 3.4's published behaviour (unpinned; DESIGN.md section 2, "display").
 *
 * Normalisation.  src is single-channel MICV_DEPTH_32F, MICV_DEPTH_8U or MICV_DEPTH_8S.  lo and hi are the minimum and
 * maximum of the image as floats, NaNs skipped, +/-Inf taking part; then, in double and unfused,
 *   scale = 255.0 * (hi - lo > DBL_EPSILON ? 1.0 / (hi - lo) : 0.0),  shift = 0.0 - lo * scale,
 *   a = (float)scale, b = (float)shift,  t = (float)src * a + b   (float, unfused),
 *   dst = isfinite(t) ? clamp(rint(t), 0, 255) : 0                (ties to even).
 * An image without a single non-NaN value gives a = b = 0 (all zeros).  One pass writes up to three images, each
 * optional (NULL), at least one wanted: dst_u8 (1 byte per pixel), dst_inverted = 255 - dst and dst_jet = the JET
 * colour of dst, 3 bytes per pixel B, G, R.  The JET table is entry i = cvRound(255 * clamp(1.5 - |4 x - k|, 0, 1)),
 * k = 1 (B), 2 (G), 3 (R), x = i / 255.0 in double, built once per context on the host.  minmax_out (optional, DEVICE,
 * 2 floats per image) receives lo and hi (NaN, NaN for an image of NaNs).  Strides in bytes; rows * cols < 2^31.
 * Two launches (min / max, apply) however many images; lo and hi are exact, so nothing depends on the grid.  A context
 * keeps the min / max words of the running call: it serves one stream at a time, like its scratch arena. */
int micv_normalize_minmax_dev(micv_ctx *ctx, const void *src, int depth, int rows, int cols, size_t sstride,
                              uint8_t *dst_u8, size_t u8_stride, uint8_t *dst_inverted, size_t inverted_stride,
                              uint8_t *dst_jet, size_t jet_stride, float *minmax_out, micv_stream stream);
int micv_normalize_minmax_host(micv_ctx *ctx, const void *src, int depth, int rows, int cols, size_t sstride,
                               uint8_t *dst_u8, size_t u8_stride, uint8_t *dst_inverted, size_t inverted_stride,
                               uint8_t *dst_jet, size_t jet_stride, float *minmax_out);
/* `batch` images of one shape, image i at base + i * pitch (bytes) on every side, each normalised by its own range: the
 * same bytes as `batch` single calls, in two launches.  batch == 0 is a no-op.  (minmax_out of the _host form is host
 * memory, as all its pointers are.) */
int micv_normalize_minmax_batch_dev(micv_ctx *ctx, const void *src, size_t src_pitch, int depth, int batch, int rows, int cols,
                                    size_t sstride, uint8_t *dst_u8, size_t u8_pitch, size_t u8_stride,
                                    uint8_t *dst_inverted, size_t inverted_pitch, size_t inverted_stride, uint8_t *dst_jet,
                                    size_t jet_pitch, size_t jet_stride, float *minmax_out, micv_stream stream);
int micv_normalize_minmax_batch_host(micv_ctx *ctx, const void *src, size_t src_pitch, int depth, int batch, int rows, int cols,
                                     size_t sstride, uint8_t *dst_u8, size_t u8_pitch, size_t u8_stride,
                                     uint8_t *dst_inverted, size_t inverted_pitch, size_t inverted_stride, uint8_t *dst_jet,
                                     size_t jet_pitch, size_t jet_stride, float *minmax_out);

/* cv::applyColorMap(src, dst, cv::COLORMAP_JET) alone: CV_8UC1 -> CV_8UC3 (B, G, R) through the same table. */
int micv_apply_colormap_jet_dev(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t sstride, uint8_t *dst_jet,
                                size_t jet_stride, micv_stream stream);
int micv_apply_colormap_jet_host(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t sstride, uint8_t *dst_jet,
                                 size_t jet_stride);

/* dst = src * gain + (noise ? noise : 0.f) in float, unfused.  gain = 1: `first + noise` (main.cpp:148) bit for bit;
 * noise = NULL: `left * contrastFactor` (main.cpp:192: convertTo with a float scale and a float zero shift).  dst may
 * alias src. */
int micv_gain_noise_f32_dev(micv_ctx *ctx, const float *src, size_t sstride, float gain, const float *noise, size_t nstride,
                            int rows, int cols, float *dst, size_t dstride, micv_stream stream);
int micv_gain_noise_f32_host(micv_ctx *ctx, const float *src, size_t sstride, float gain, const float *noise, size_t nstride,
                             int rows, int cols, float *dst, size_t dstride);

/* cv::randn(dst, mean, sigma) on a CV_32FC1 image from a cv::RNG whose 64-bit state is *state (cv::theRNG() starts at
 * 0xffffffff; 0 is taken as that): sample i in row-major order is the i-th ziggurat draw z of the generator (the one
 * micv_pf_create draws its tables from), stored as z * sigma + mean in float, unfused.  *state comes back advanced, so
 * consecutive calls continue one generator.  Host memory, host code: the ziggurat takes a data-dependent number of
 * words from a serial generator. */
int micv_cv_randn_f32_host(uint64_t *state, float mean, float sigma, int rows, int cols, float *dst, size_t dstride);

/* disparitySSDPair / disparityNCorrPair (main.cpp:21-78): disp_left = search(left, right) over [-disparity_range, 0],
 * disp_right = search(right, left) over [0, disparity_range]; the bytes of the two micv_disparity_* calls, which are
 * what it issues on `stream`.  flags as there; disparity_range 0..127. */
#define MICV_DISPARITY_SSD 0
#define MICV_DISPARITY_NCC 1
int micv_disparity_pair_dev(micv_ctx *ctx, const float *left, const float *right, int rows, int cols, size_t stride,
                            int window_rad, int disparity_range, int metric, int flags, int8_t *disp_left,
                            int8_t *disp_right, size_t dstride, micv_stream stream);
int micv_disparity_pair_host(micv_ctx *ctx, const float *left, const float *right, int rows, int cols, size_t stride,
                             int window_rad, int disparity_range, int metric, int flags, int8_t *disp_left,
                             int8_t *disp_right, size_t dstride);
/* One pair-and-display block of a runProblem* after the grey conversion, on one stream without a host synchronise:
 * left' = left * gain + noise_left, right' = right * gain + noise_right (gain 1.f and both noise images NULL: the
 * images as they are; the noise images come together or not at all), the pair on left', right', then the images the
 * driver writes: image_left = normalised disp_left, image_left_inverted = 255 - image_left (optional), image_right =
 * normalised disp_right.  The maps come back too.  `work` (device, 2 * rows * cols floats) holds left' and right'
 * and is needed only with a gain other than 1.f or with noise.  The _host form uploads left, right (and the noise images) and
 * downloads the two maps and the 8-bit images, nothing else. */
int micv_disparity_pair_display_dev(micv_ctx *ctx, const float *left, const float *right, int rows, int cols, size_t stride,
                                    float gain, const float *noise_left, const float *noise_right, size_t nstride,
                                    int window_rad, int disparity_range, int metric, int flags, int8_t *disp_left,
                                    int8_t *disp_right, size_t dstride, uint8_t *image_left, uint8_t *image_left_inverted,
                                    uint8_t *image_right, size_t istride, float *work, micv_stream stream);
int micv_disparity_pair_display_host(micv_ctx *ctx, const float *left, const float *right, int rows, int cols, size_t stride,
                                     float gain, const float *noise_left, const float *noise_right, size_t nstride,
                                     int window_rad, int disparity_range, int metric, int flags, int8_t *disp_left,
                                     int8_t *disp_right, size_t dstride, uint8_t *image_left, uint8_t *image_left_inverted,
                                     uint8_t *image_right, size_t istride);

/* --------------------------------------------------- ps6: particle filter ---------- */

/* ParticleFilter, ps6_cpp/include/ParticleFilter.h and lib/ParticleFilter.cpp, on the device: one tick is
 * three launches on one stream (score, resample + estimate, model update) with no host sync and no parallel
 * branch.  The arithmetic is DESIGN.md section 2 ("Particle filter"); in short:
 *
 * RNG (cv::RNG, host side, once at create).  state = seed ? seed : 0xffffffff;
 *   next():  state = (uint64)(uint32)state * 4164903690u + (state >> 32); return (uint32)state;
 *   uniform(float a, float b) = (float)next() * 2^-32f * (b - a) + a, float arithmetic, unfused;
 *   gaussian(sigma) = (double)z * sigma with z = randn_0_1_32f, OpenCV 3.4's ziggurat:
 *     tables (double, then rounded): m1 = 2^31, dn = tn = 3.442619855899, vn = 9.91256303526217e-3,
 *       q = vn / exp(-.5*dn*dn); kn[0] = (uint32)((dn/q)*m1); kn[1] = 0; wn[0] = (float)(q/m1);
 *       wn[127] = (float)(dn/m1); fn[0] = 1; fn[127] = (float)exp(-.5*dn*dn);
 *       for i = 126 .. 1: dn = sqrt(-2*log(vn/dn + exp(-.5*dn*dn))); kn[i+1] = (uint32)((dn/tn)*m1);
 *                         tn = dn; fn[i] = (float)exp(-.5*dn*dn); wn[i] = (float)(dn/m1);
 *     draw (NOTE: a word is read from the state BEFORE the state steps, so the first word of a fresh
 *     generator is its seed's low half):
 *       loop: hz = (int32)state; step; iz = hz & 127; x = (float)hz * wn[iz];
 *             if ((uint32)abs(hz) < kn[iz]) return x;                  (abs(INT_MIN) = INT_MIN)
 *             if (iz == 0) {                                             base strip, r = 3.442620f
 *               do { x = (float)(uint32)state * 2^-32f; step; y = (float)(uint32)state * 2^-32f; step;
 *                    x = (float)((double)logf(x + FLT_MIN) * -0.2904764); y = -logf(y + FLT_MIN);
 *               } while (y + y < x * x);
 *               return hz > 0 ? r + x : -r - x; }
 *             y = (float)(uint32)state * 2^-32f; step;
 *             if ((double)(fn[iz] + y * (fn[iz-1] - fn[iz])) < exp(-.5 * (double)x * (double)x)) return x;
 *     exp is the library's own double exp (below); logf(v) is (float)log((double)v), log and sqrt the C
 *     library's (correctly rounded sqrt; the tables are built once).
 * The RNG quirk of the reference is kept: displaceParticles, resampleMultinomial and genParticles each
 * construct a fresh cv::RNG, so every tick displaces particle i by the same (gx_i, gy_i) = the i-th pair
 * of gaussian(sample_sigma) draws of a fresh generator, and resamples with the same n uniform(0, 1)
 * draws of another fresh generator.  Both tables are made once at create and uploaded once.
 * Initial particles (genParticles, host, once): a fresh generator; UNIFORM when init == (-1, -1):
 *   (x, y) = (uniform(0, img_cols), uniform(0, img_rows)); otherwise GAUSSIAN around the model centre
 *   c = init + (float)size / 2: (x, y) = ((float)(g_x + c.x), (float)(g_y + c.y)) with gaussian(sample_sigma);
 *   a pair equal (float ==) to an earlier one is drawn again.
 *
 * exp(x), double, no contraction (fdlibm's e_exp.c scheme): NaN -> NaN; x > 709.782712893383973096 -> inf;
 *   x < -745.13321910194110842 -> 0; k = (int)(x * 1.44269504088896338700 + (x < 0 ? -0.5 : 0.5)) (truncation);
 *   hi = x - k * 6.93147180369123816490e-01; lo = k * 1.90821492927058770002e-10; r = hi - lo; t = r * r;
 *   c = r - t*(P1 + t*(P2 + t*(P3 + t*(P4 + t*P5)))) with P1..P5 = 1.66666666666666019037e-01,
 *   -2.77777777770155933842e-03, 6.61375632143793436117e-05, -1.65339022054652515390e-06,
 *   4.13813679705723846039e-08; y = 1 - ((lo - (r*c)/(2 - c)) - hi); then y * 2^k, as
 *   (y * 2^1000) * 2^(k-1000) for k > 1000 and (y * 2^(k+1000)) * 2^-1000 for k < -1000.
 *
 * One tick (frame: img_rows x img_cols x channels u8, interleaved, `stride` bytes per row):
 *   displace:  p = ((float)((double)p.x + gx_i), (float)((double)p.y + gy_i));
 *   weight 0 when p.x < 0 || p.x >= img_cols || p.y < 0 || p.y >= img_rows (float p); otherwise the
 *   patch's top-left pixel is (cvRound(p.x) - xOff, cvRound(p.y) - yOff) of the frame, xOff = ceil(mcols/2),
 *   yOff = ceil(mrows/2), cvRound rounds halves to even, coordinates outside clamp (BORDER_REPLICATE);
 *   MICV_PF_MSE: S = sum over every byte of min(max(m - c, 0)^2, 255) (cv::Mat u8 arithmetic as written:
 *     the difference and the product saturate), or of (m - c)^2 with MICV_PF_MSE_SIGNED, an exact integer;
 *     sim = exp(-(S / (double)(mrows*mcols)) / (2 * mse_sigma * mse_sigma));
 *   MICV_PF_HIST: per channel 32 bins of v >> 3, exact counts; cv::normalize(NORM_L2): h = (float)((double)h
 *     * (1.0 / sqrt(sum h^2))); chi-square against the model histogram a: sum over bins in order, where
 *     |a| > DBL_EPSILON, of (double)d * (double)d / a with d = a - h in float; averaged over the channels
 *     in double, sim = exp(-comp);
 *   weights: w_i = (float)sim_i; simSum = sum of the double sims in particle order; w_i = (float)(w_i / simSum).
 *     simSum == 0 or not finite: the displaced particles are kept, w_i = (float)sim_i, and status bit
 *     MICV_PF_STATUS_NO_WEIGHT is set (the reference divides by zero);
 *   resample: cum = sequential float prefix sum of w; particle i = old particle upper_bound(cum, u_i),
 *     the index clamped to n - 1 (MICV_PF_STATUS_CLAMPED; the reference reads one past the end);
 *   estimate: float mean and variance summed sequentially in particle order, divided by (float)n;
 *   model update at (cvRound(mean.x), cvRound(mean.y)) (the mean clamped to +-2^24 first; the patch read
 *     as above): blend = saturate_cast<uchar>((float)alpha * new + (float)(1 - alpha) * old), unfused, with
 *     cvRound; MICV_PF_MSE blends into the model patch; MICV_PF_HIST always blends from the ORIGINAL model
 *     patch (the reference never updates _modelPatch there) and the blend's normalized histogram becomes
 *     the model histogram.
 * The model is copied at create: the reference's driver keeps a view into frame 0, into which it then paints particles
 * and the bounding box.  The painting is reproduced ("ps6: driver" below); the view is not: the model stays a copy,
 * so the tracker never sees the paint. */
#define MICV_PF_MSE  0 /* ParticleFilter::SimilarityMode::MEAN_SQ_ERR */
#define MICV_PF_HIST 1 /* ParticleFilter::SimilarityMode::MEAN_SHIFT_LT */
#define MICV_PF_MSE_SIGNED 1u /* flag: the intended (m - c)^2 instead of the saturating u8 arithmetic */
#define MICV_PF_STATUS_NO_WEIGHT 1u /* simSum was 0 or not finite: no resampling this tick */
#define MICV_PF_STATUS_CLAMPED   2u /* some u_i >= cum[n-1]: its index was clamped to n - 1 */
#define MICV_PF_MAX_PARTICLES 4096
#define MICV_PF_DEFAULT_SEED 0xffffffffull /* cv::RNG's default state */
typedef struct micv_pf micv_pf;
typedef struct micv_pf_state {
    float x, y, x_var, y_var; /* estimateState(): the particle mean and the x / y variances */
    uint32_t status;          /* MICV_PF_STATUS_* bits of this tick */
} micv_pf_state;
/* model: mrows x mcols x channels u8 (host, mstride bytes per row), copied.  channels 1 or 3;
 * 1 <= mrows <= img_rows, 1 <= mcols <= img_cols; 1 <= n <= MICV_PF_MAX_PARTICLES; mode MICV_PF_MSE needs
 * 0 < mse_sigma < inf (MICV_PF_HIST ignores it); sample_sigma finite and >= 0; alpha finite; init_x / init_y
 * finite ((-1, -1) selects UNIFORM init); flags 0 or MICV_PF_MSE_SIGNED; seed 0 means 0xffffffff as in
 * cv::RNG.  MICV_EINVAL also when GAUSSIAN init cannot draw n distinct particles in 64 n + 4096 tries.
 * Synchronous (the tables and the model are uploaded before it returns). */
int micv_pf_create(micv_ctx *ctx, const uint8_t *model, int mrows, int mcols, size_t mstride, int channels,
                   int img_rows, int img_cols, int n, int mode, double mse_sigma, double sample_sigma,
                   float init_x, float init_y, double alpha, uint32_t flags, uint64_t seed, micv_pf **pf);
void micv_pf_destroy(micv_pf *pf);
/* One tick on `stream`: frame (device, img_rows x img_cols x channels u8, stride >= img_cols * channels).
 * The state goes to state_dev (device, may be NULL) and stays readable through the calls below.
 * Asynchronous; MICV_EINVAL (nothing enqueued) for a null pf / frame or a bad stride. */
int micv_pf_tick_dev(micv_pf *pf, const uint8_t *frame, size_t stride, micv_stream stream,
                     micv_pf_state *state_dev);
/* The same from a host frame: upload, tick, download of the state, sync. */
int micv_pf_tick_host(micv_pf *pf, const uint8_t *frame, size_t stride, micv_pf_state *state);
/* The current particles (n x {x, y} f32) and weights (n f32: the normalized weights of the last tick,
 * before resampling, as the reference's _weights; 1/n before the first tick).  _dev copies on `stream`
 * into device memory, _host copies out and syncs.  The _host calls (and micv_pf_tick_host) run on the null
 * stream: after a micv_pf_tick_dev on a non-blocking stream, synchronise that stream first. */
int micv_pf_particles_dev(micv_pf *pf, float *xy, micv_stream stream);
int micv_pf_particles_host(micv_pf *pf, float *xy);
int micv_pf_weights_dev(micv_pf *pf, float *w, micv_stream stream);
int micv_pf_weights_host(micv_pf *pf, float *w);
/* The model: patch (mrows x mcols x channels u8, dense; MICV_PF_MSE: the current model patch, MICV_PF_HIST:
 * the last blend, the original model before the first tick) and hist (channels x 32 f32, MICV_PF_HIST's
 * model histogram, zeros in MICV_PF_MSE).  Either may be NULL.  Syncs. */
int micv_pf_model_host(micv_pf *pf, uint8_t *patch, float *hist);
/* nframes ticks over host frames (each img_rows x img_cols x channels u8, `stride` bytes per row): every
 * frame uploaded once, the upload of frame t + 1 beside tick t.  states: nframes entries; particles (may be
 * NULL): nframes x n x {x, y} f32, the particles after each tick.  Byte-identical to nframes calls of
 * micv_pf_tick_host (and micv_pf_particles_host).  Blocking. */
int micv_pf_track_seq_host(micv_pf *pf, const uint8_t *const *frames, int nframes, size_t stride,
                           micv_pf_state *states, float *particles);

/* A group of filters ticked together: the six trackers of the ps6 driver, or several targets in one video.  A group
 * BORROWS its members: it owns no particles, model or tables, only a device table of member descriptors (uploaded at
 * create, synchronous like micv_pf_create) and, for the host-sequence calls, two frame buffers.  Members share the
 * device and the frame's rows, cols and channels and may differ in everything else.  MICV_EINVAL for count outside
 * 1 .. MICV_PF_GROUP_MAX, a null member, the same member twice, members on different devices or of different frame
 * sizes.  The members live on after micv_pf_group_destroy; destroying a member before its group, or using a member
 * (through its group or alone) from two streams at once, is the caller's error.
 * micv_pf_group_tick_dev: frames / strides are HOST arrays of device pointers and row strides, nframes == 1 (one frame
 * for every member) or nframes == count (frame k for member k); they travel by value in the launch arguments, so the
 * call copies nothing, allocates nothing and never synchronises.  Three launches on `stream` whatever count is: score
 * (grid max n x count; a workgroup past its member's n exits at once), resample + estimate and model update (one
 * workgroup per member each).  Afterwards EVERY member is, byte for byte, in the state micv_pf_tick_dev on its own
 * frame would have left it in (particles, weights, model, histogram, state, status bits): the stages are the same code.
 * states_dev (device, may be NULL): count entries, entry k member k's.  Every accessor above and micv_ps6_overlay_dev
 * work on the members afterwards; group ticks and single ticks of members may be interleaved on one stream in any
 * order (the group caches nothing).  MICV_EINVAL (nothing enqueued) for nframes other than 1 or count, a null frame
 * or a stride < img_cols * channels.
 * micv_pf_group_track_seq_host: micv_pf_track_seq_host for the whole group over ONE host video: each frame uploaded
 * once, the upload of frame t + 1 beside tick t, two streams of its own, blocking.  states: [nframes][count];
 * particles: NULL, or count pointers, each NULL or [nframes][n_k][2] f32.  Byte-identical to micv_pf_track_seq_host on
 * each member alone. */
#define MICV_PF_GROUP_MAX 64
typedef struct micv_pf_group micv_pf_group;
int micv_pf_group_create(micv_pf *const *members, int count, micv_pf_group **group);
void micv_pf_group_destroy(micv_pf_group *group);
int micv_pf_group_tick_dev(micv_pf_group *g, const uint8_t *const *frames, const size_t *strides, int nframes,
                           micv_stream stream, micv_pf_state *states_dev);
int micv_pf_group_track_seq_host(micv_pf_group *g, const uint8_t *const *frames, int nframes, size_t stride,
                                 micv_pf_state *states, float *const *particles);

/* ----------------------------------- ps7: motion history ----- */

/* mhi::frameDifference, ps7_cpp/lib/MotionHistory.cpp:26-77, for single-channel CV_8U frames:
 * Gaussian blur with the reference's `const cv::Size& blurSize` (MotionHistory.h:14: blur_w taps
 * along x, blur_h along y, each odd <= 31; blur_sigma > 0 for both directions as
 * cv::cuda::createGaussianFilter(type, -1, ksize, sigma1) does), saturating f2 - f1,
 * AbsThreshold -> {0,1}, 7x7 elliptical morphological open.  diff is rows x cols u8. */
int micv_mhi_frame_difference_dev(micv_ctx *ctx, const uint8_t *f1, const uint8_t *f2, int rows,
                                  int cols, size_t stride, double thresh, int blur_w, int blur_h,
                                  double blur_sigma, uint8_t *diff, size_t dstride,
                                  micv_stream stream);
int micv_mhi_frame_difference_host(micv_ctx *ctx, const uint8_t *f1, const uint8_t *f2, int rows,
                                   int cols, size_t stride, double thresh, int blur_w, int blur_h,
                                   double blur_sigma, uint8_t *diff, size_t dstride);
/* mhi::energyFromHistory, MotionHistory.cpp:98-105: mei = mhi > 0 ? 1 : 0. */
int micv_mhi_energy_dev(micv_ctx *ctx, const uint8_t *mhi, int rows, int cols, size_t sstride,
                        uint8_t *mei, size_t dstride, micv_stream stream);
int micv_mhi_energy_host(micv_ctx *ctx, const uint8_t *mhi, int rows, int cols, size_t sstride,
                         uint8_t *mei, size_t dstride);
/* thresholdDifference / AbsThreshold<uint8_t>, ps7_cpp/lib/MotionHistory.cu:17-48. */
int micv_mhi_threshold_dev(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t sstride,
                           double thresh, uint8_t *dst, size_t dstride, micv_stream stream);
int micv_mhi_threshold_host(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t sstride,
                            double thresh, uint8_t *dst, size_t dstride);
/* mhi::calcMotionHistory -> motionHistoryKernel, MotionHistory.cu:52-83: in place,
 * history = mask == 1 ? tau : max(history - 1, 0). */
int micv_mhi_update_dev(micv_ctx *ctx, uint8_t *history, size_t hstride, const uint8_t *mask,
                        size_t mstride, int rows, int cols, int tau, micv_stream stream);
int micv_mhi_update_host(micv_ctx *ctx, uint8_t *history, size_t hstride, const uint8_t *mask,
                         size_t mstride, int rows, int cols, int tau);

/* MHI sequence: mhiHelper's loop (ps7_cpp/src/Solution.cpp:16-101) over F frames of one video.  Frame f (0-based) is
 * at frames + f * frame_pitch, rows of `stride` bytes.  The history starts at zero; update number j (j = 1..F-1) is
 * frameDifference(frame j-1, frame j) then calcMotionHistory, and save[i] = j stores the history after update j into
 * out + i * out_pitch (rows of out_stride bytes): mhiHelper's frameNum.  A save number outside 1..F-1 is MICV_EINVAL.
 * The history and difference planes live in the context scratch beside frameDifference's own. */
int micv_mhi_history_seq_dev(micv_ctx *ctx, const uint8_t *frames, int nframes, size_t frame_pitch, size_t stride,
                             int rows, int cols, double thresh, int blur_w, int blur_h, double blur_sigma, int tau,
                             const int *save, int nsave, uint8_t *out, size_t out_pitch, size_t out_stride,
                             micv_stream stream);
/* Uploads every frame once, runs the _dev form on the null stream, downloads the saved histories. */
int micv_mhi_history_seq_host(micv_ctx *ctx, const uint8_t *frames, int nframes, size_t frame_pitch, size_t stride,
                              int rows, int cols, double thresh, int blur_w, int blur_h, double blur_sigma, int tau,
                              const int *save, int nsave, uint8_t *out, size_t out_pitch, size_t out_stride);

/* mhi::frameDifference on the frames mhiHelper hands it (Solution.cpp:16-101: `vid >> frame`, CV_8UC3): `channels`
 * is 1, 3 or 4, samples interleaved, `stride` in bytes and >= cols * channels, any base address.  diff is rows x cols
 * u8 as above.  Contract for 3 and 4 channels (MotionHistory.cpp:50-73; the arithmetic of cv::cuda is restated, not
 * pinned to a build of it):
 *   blur      every channel as a plane of its own by the single-channel contract: gaussian taps, row pass then column
 *             pass, acc = fmaf(x, k, acc) from +0, BORDER_REFLECT_101, round half to even, saturate to u8.  The 4th
 *             channel is not blurred: nothing reads it.
 *   subtract  per channel, d_c = max(b2_c - b1_c, 0) (cv::cuda::subtract on CV_8UC3).
 *   grey      g = (d_0 * 4899 + d_1 * 9617 + d_2 * 1868 + 8192) >> 14, the 8-bit rule of micv_to_gray_f32: channel 0
 *             carries the 0.299 weight AS WRITTEN (cvtColor(COLOR_RGB2GRAY) on the capture's BGR data).  The weights
 *             sum to 16384, so g <= 255.  Channel 3 is ignored.
 *   then      AbsThreshold on g and the 7x7 elliptical open, as above.
 * channels == 1 gives the bytes of micv_mhi_frame_difference_dev.  The grey step follows the subtraction: a channel
 * whose difference saturates at 0 does not pull the others down, which grey-then-subtract would. */
int micv_mhi_frame_difference_c_dev(micv_ctx *ctx, const uint8_t *f1, const uint8_t *f2, int rows, int cols, int channels,
                                    size_t stride, double thresh, int blur_w, int blur_h, double blur_sigma, uint8_t *diff,
                                    size_t dstride, micv_stream stream);
int micv_mhi_frame_difference_c_host(micv_ctx *ctx, const uint8_t *f1, const uint8_t *f2, int rows, int cols, int channels,
                                     size_t stride, double thresh, int blur_w, int blur_h, double blur_sigma, uint8_t *diff,
                                     size_t dstride);
/* micv_mhi_history_seq_* on frames of 1, 3 or 4 channels, with mhiHelper's second list: save_diff[i] = j stores the
 * {0,1} mask of update j into diff_out + i * diff_pitch (rows of diff_stride bytes), as save[i] = j stores the history
 * (saveDiffFrames and saveMHIFrames).  Either list may be empty (count 0, pointers NULL) but not both; the loop runs to
 * the larger of the two maxima.  One channel and no diff saves give the bytes of micv_mhi_history_seq_dev. */
int micv_mhi_history_seq_c_dev(micv_ctx *ctx, const uint8_t *frames, int nframes, size_t frame_pitch, size_t stride, int rows,
                               int cols, int channels, double thresh, int blur_w, int blur_h, double blur_sigma, int tau,
                               const int *save, int nsave, uint8_t *out, size_t out_pitch, size_t out_stride,
                               const int *save_diff, int nsave_diff, uint8_t *diff_out, size_t diff_pitch, size_t diff_stride,
                               micv_stream stream);
int micv_mhi_history_seq_c_host(micv_ctx *ctx, const uint8_t *frames, int nframes, size_t frame_pitch, size_t stride, int rows,
                                int cols, int channels, double thresh, int blur_w, int blur_h, double blur_sigma, int tau,
                                const int *save, int nsave, uint8_t *out, size_t out_pitch, size_t out_stride,
                                const int *save_diff, int nsave_diff, uint8_t *diff_out, size_t diff_pitch, size_t diff_stride);
/* getAllMHIs' loop (Solution.cpp:113-146) over nvideos videos in one call.  Shared: rows, cols, channels, stride,
 * frame_pitch and the blur.  Per video v (host arrays of nvideos entries): frames[v], a DEVICE pointer to its frame 0;
 * nframes[v]; thresh[v]; tau[v]; save[v] in 1..nframes[v]-1.  out + v * out_pitch (rows of out_stride bytes) receives
 * the history after update save[v], byte-equal to micv_mhi_history_seq_c_dev with that one save number.  Step j is two
 * launches over every video with save[v] >= j (the update is fused into the open's byte write, and the output plane is
 * the history); a video past its save number is skipped and its output not touched again.  Stream-ordered, no host
 * synchronisation; the host arrays are not read after the call returns (the table travels by value with the launches).
 * Batches above 32 videos, or whose mask words exceed 64 MiB, run in pieces.  Bad arguments return MICV_EINVAL before
 * anything is enqueued. */
int micv_mhi_history_batch_dev(micv_ctx *ctx, const uint8_t *const *frames, const int *nframes, size_t frame_pitch, size_t stride,
                               int nvideos, int rows, int cols, int channels, const double *thresh, const int *tau, const int *save,
                               int blur_w, int blur_h, double blur_sigma, uint8_t *out, size_t out_pitch, size_t out_stride,
                               micv_stream stream);

/* ------------------------------------------------------- ps7: central moments ------- */

/* moments::centralMoment (ps7_cpp/lib/Moments.cpp) for `batch` single-channel images: image b starts at
 * imgs + b * img_pitch bytes, rows of `stride` bytes, `type` MICV_MOMENTS_U8 or MICV_MOMENTS_F32.  `orders` (host) holds
 * n pairs (p, q), p, q >= 0, p + q <= MICV_MOMENTS_MAX_ORDER, n <= MICV_MOMENTS_MAX_ORDERS.  Out (f32): mu[batch][n],
 * eta[batch][n] and, when raw is not NULL, raw[batch][3] = M00, M10, M01.  Stream-ordered, no host sync; bad arguments
 * return MICV_EINVAL before anything is enqueued.  Images above 2^24 pixels are MICV_EINVAL (the exact sums' int64
 * headroom: a term is below 2^39 in its bin).
 *
 * Arithmetic contract (each step as Moments.cpp and the driver write it):
 *   v     u8 -> (float)v (convertTo CV_32FC1, :14); f32 as given.  MICV_MOMENTS_NORM_INF (u8 only) first applies
 *         cv::normalize(mhi, mhi, 1.0, 0.0, NORM_INF, CV_32FC1) (Solution.cpp:243-245): v = fl((float)u * s) with
 *         s = (float)(1.0 / max) computed in double, s = 0 when the image max is 0 (OpenCV 3's normalize -> convertTo
 *         with a float work type).
 *   x, y  column and row as f32 (the iota matrices, :17-39).  M00 = S v, M10 = S fl(x v), M01 = S fl(y v) (:45-47);
 *         xBar = fl(M10 / M00), yBar = fl(M01 / M00), f32, correctly rounded (:49-50).
 *   dx    fl(x - xBar).  dy = fl(x - yBar) AS WRITTEN (:59 is cv::pow(xFull - yBar, q, yPow)); MICV_MOMENTS_Y_FIXED
 *         uses fl(y - yBar).
 *   pow   cv::pow with an integer power on f32: power 0 -> 1.0f (even for NaN), 1 -> copy, otherwise iPow_'s loop
 *         a = 1, b = d; while (p > 1) { if (p & 1) a *= b; b *= b; p >>= 1; } a *= b, in f32.
 *   term  fl(dy^q * fl(dx^p * v)) (yPow.mul(xPow.mul(fltImg)), :61).
 *   S     every sum is the exact sum of its f32 terms, rounded once to double (RNE), then to f32
 *         (float M = cv::sum(...)[0]).  OpenCV's own order -- a serial double chain over float partials of four, SIMD
 *         dependent -- cannot be reproduced by a parallel reduction; exact-then-round is the order-independent limit
 *         of all such orders (tests/test_ps7_ref.py bounds the difference on a 480 x 640 MHI: <= 4 f32 ulp).
 *   eta   (float)((double)mu / P), P = pow(M00, 1 + (p+q)/2) from IEEE basic operations only: d = (double)M00,
 *         P = d * d * ... * d (the integer part of the power, left to right), times sqrt(d) (correctly rounded) when
 *         p + q is odd.  P is within 3 ulp of glibc pow over the sweep tests/test_ps7_ref.py runs (M00 in
 *         [1e-3, 1e7], powers 1 .. 5); host, device and the tests agree bit for bit.
 *   non-finite  M00 = 0 gives NaN centroids and whatever the steps make of them; a NaN term, or +Inf with -Inf, makes
 *         a sum NaN, otherwise +-Inf terms make it +-Inf.  Output NaNs are the canonical quiet NaN 0x7FC00000. */
#define MICV_MOMENTS_U8 0
#define MICV_MOMENTS_F32 1
#define MICV_MOMENTS_NORM_INF 1u
#define MICV_MOMENTS_Y_FIXED 2u
#define MICV_MOMENTS_MAX_ORDERS 16
#define MICV_MOMENTS_MAX_ORDER 8
int micv_central_moments_dev(micv_ctx *ctx, const void *imgs, int batch, size_t img_pitch, size_t stride, int rows,
                             int cols, int type, const int *orders, int n, uint32_t flags, float *mu, float *eta,
                             float *raw, micv_stream stream);
int micv_central_moments_host(micv_ctx *ctx, const void *imgs, int batch, size_t img_pitch, size_t stride, int rows,
                              int cols, int type, const int *orders, int n, uint32_t flags, float *mu, float *eta,
                              float *raw);

/* ----------------------------------------- ps7: k-NN and confusion matrices --------- */

/* cv::ml::KNearest::train(ROW_SAMPLE) + findNearest(test, k, results), brute force, classifier mode.  train is
 * ntrain x dims f32 (row stride in bytes), labels int32; test is ntest x dims.  pred[ntest] int32.  dims <= 64,
 * k <= 32, row counts below 2^24.  One lane per test row.
 *
 * The contract, written from OpenCV 3.4's knearest.cpp as recalled: UNPINNED (OpenCV is not available to check it,
 * as DESIGN.md section 3 says of the other OpenCV-carried arithmetic).
 *   distance  f32 s = 0; per group of four dims t_i = fl(u_i - v_i), s = fl(s + (((t0*t0 + t1*t1) + t2*t2) + t3*t3))
 *             without FMA; then the remaining dims one at a time, s = fl(s + t*t); the distance is (float)s.
 *             MICV_KNN_F64_ACC: double s and double t_i = (double)fl(u_i - v_i) (OpenCV 2.4's CvKNearest form).
 *   insertion k = min(k, train rows); k slots start at FLT_MAX with response 0; a candidate goes after every slot whose
 *             distance bits (int32) are <= its own, so equal distances keep the earlier train row; +Inf and NaN (any
 *             sign bit) compare above FLT_MAX and are never inserted.
 *   vote      bubble-sort the k responses ascending and take the longest run; on a tie the first (smallest) label
 *             wins.  Empty slots vote 0. */
#define MICV_KNN_F64_ACC 1u
#define MICV_KNN_MAX_DIMS 64
#define MICV_KNN_MAX_K 32
#define MICV_KNN_MAX_LABELS 16
#define MICV_KNN_MAX_GROUPS 32
int micv_knn_predict_dev(micv_ctx *ctx, const float *train, int ntrain, size_t train_stride, const int *train_labels,
                         const float *test, int ntest, size_t test_stride, int dims, int k, uint32_t flags, int *pred,
                         micv_stream stream);
int micv_knn_predict_host(micv_ctx *ctx, const float *train, int ntrain, size_t train_stride, const int *train_labels,
                          const float *test, int ntest, size_t test_stride, int dims, int k, uint32_t flags, int *pred);
/* matching::naiveConfusionMatrix (groups NULL) and matching::confusionMatrix (Matching.cpp) over n rows of features
 * with labels in 1..num_labels (L <= 16).
 *   groups NULL  leave-one-out: each row is tested against all others in their original order; confusion holds one
 *                L x L matrix.
 *   groups       for g = 1..num_groups (G <= 32) the train set is the rows with group != g in original order, the test
 *                set the rows with group == g; confusion holds G matrices and then their average ((G + 1) x L x L).  A
 *                row whose group is outside 1..G is in no fold (prediction 0) but is trained on in every fold.
 * pred[n] (may be NULL) receives each tested row's vote in its own fold.  A row whose label or vote is outside 1..L is
 * left out of the matrices and counted in *left_out (may be NULL); the reference asserts there, the library does not.
 * Matrices: confusion[expected-1][result-1] += 1 and counts[expected-1] += 1 in f32; each row divided by its count as
 * OpenCV 3's divide does (0 where the count is 0); the average is fl(fl(fl(0 + C1) + C2) + ...) * (float)(1.0 / G)
 * (avg / float(n) is a MatExpr evaluated as convertTo(alpha = 1/n), not a division).
 * Not restated: arrangeTrainingData's BOTH mode (Solution.cpp:166-182) indexes past the moment vector -- undefined
 * behaviour the driver never reaches. */
int micv_knn_confusion_dev(micv_ctx *ctx, const float *features, int n, size_t stride, int dims, const int *labels,
                           const int *groups, int num_labels, int num_groups, int k, uint32_t flags, float *confusion,
                           int *pred, int *left_out, micv_stream stream);
int micv_knn_confusion_host(micv_ctx *ctx, const float *features, int n, size_t stride, int dims, const int *labels,
                            const int *groups, int num_labels, int num_groups, int k, uint32_t flags, float *confusion,
                            int *pred, int *left_out);

/* ------------------------------------------------------------- ps3: geometry -------- */

/* Camera calibration and the fundamental matrix of ps3 (ps3_cpp/lib/Calibration.cpp, lib/Fundamental.cpp and the
 * driver ps3_cpp/src/Solution.cpp), batched: T systems share their point arrays and differ in an index list, one wave
 * per system, nothing gathered on the host.  Points are ROWS here: pts2d [n][2], pts3d [n][3] f32 (the reference's
 * cv::Mats are 2 x n / 3 x n; the Python layer and the shim transpose).  indices is [T][stride] int32; NULL (T = 1
 * only) means 0, 1, 2, ...  Stream-ordered, no host sync; bad arguments return MICV_EINVAL before anything is
 * enqueued.  An index outside [0, n) (or a kcount outside [0, k]) cannot be seen on the host by a _dev entry: the
 * system's outputs are NaN and *status (device int32, zeroed by the call) becomes 1; the _host entries check the lists
 * first and return MICV_EINVAL with every output untouched.
 *
 * Arithmetic contract.  R is float, or double with MICV_GEOM_F64: the same operations in the same order, inputs still
 * f32, every output rounded once to f32 (residuals stay double).  No fused multiply-add.
 *   normal equations   S = A^T A and A^T b are summed entry by entry, from 0, over the rows of A in order (constraint
 *         0 first, its x row before its y row), s = fl(s + fl(a_r * a_c)), zero entries of A included (0 * inf = NaN
 *         as written); A is never formed.  Calibration rows: [X Y Z 1 0 0 0 0 (-x)X (-x)Y (-x)Z | x] and
 *         [0 0 0 0 X Y Z 1 (-y)X (-y)Y (-y)Z | y]; fundamental rows [u u', v u', u', u v', v v', v', u, v | -1]
 *         with (u, v) from image A and (u', v') from image B.
 *   LDL^T  diagonal pivoting: at step p the first largest |S[i][i]|, i >= p (a NaN is never larger), rows and columns
 *         swapped; S[i][j] -= fl(S[p][max(i,j)] / d) * S[p][min(i,j)] for i, j > p and b[i] -= fl(S[p][i] / d) * b[p];
 *         L[i][p] = fl(S[p][i] / d).  z[p] = b[p] / d[p]; x[p] = z[p] - L[p+1][p] x[p+1] - .. (ascending), p
 *         descending; the permutation undone.  No threshold: a zero pivot gives inf / NaN.  A 1 is appended.
 *   trial residual (Solution.cpp:243-318)  per test point p_r = (R)(((m_r0 X + m_r1 Y) + m_r2 Z) + m_r3 * 1) with
 *         double products and sums (the gemm rule of the RANSAC block), w = (R)(1.0 / (double)p_2), u = fl(p_0 * w),
 *         v = fl(p_1 * w) (cv::Mat / scalar multiplies by the reciprocal), d = sqrt(D(u - x)^2 + D(v - y)^2) in double
 *         with D() the R difference widened; residual = (d_0 + d_1 + ..) / (double)j from 0.0 in order; j = 0 gives
 *         NaN.  With MICV_GEOM_F64 the unrounded double M is projected.
 *   arg-min  per group and overall, the first trial whose residual is strictly below every earlier one and below
 *         DBL_MAX (the reference's start value): NaN and +inf never win.  No winner: index -1, residual DBL_MAX, M = 0.
 *   SVD   one-sided (Hestenes) Jacobi on the columns of A (calibration: the rows above with -x / -y as 12th entry),
 *         V = I.  Pairs (p, q), p < q, in the cyclic order (0,1), (0,2), .., (10,11).  alpha = S a_p^2, beta = S a_q^2,
 *         gamma = S a_p a_q: 64 serial partials (partial l sums rows l, l + 64, .. from 0) joined by
 *         v_l = v_l + v_(l xor m) for m = 32, 16, 8, 4, 2, 1.  The pair rotates when |gamma| > eps sqrt(alpha beta),
 *         eps = 1e-7f (R = float) or 1e-15 (double): zeta = (beta - alpha) / (2 gamma),
 *         t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)) with sign(0) = +1, c = 1 / sqrt(1 + t^2), s = c t,
 *         a_p' = c a_p - s a_q, a_q' = s a_p + c a_q, the same on the columns of V.  The loop ends after a sweep
 *         without a rotation or after 30 sweeps.  The answer is the column of V whose column of A has the smallest
 *         squared norm (summed the same way), the first one on ties; unit norm, sign as it falls.
 *   rank reduction  the same Jacobi on the 3 x 3 matrix; the column of the rotated A with the smallest norm is set to
 *         zero and out[r][c] = ((0 + a_r0 v_c0) + a_r1 v_c1) + a_r2 v_c2 (U Sigma V^T with the smallest sigma = 0).
 *   3 x 3 products  double accumulation from the first product, ascending, one rounding to R.
 *   normalised chain (Solution.cpp:381-445)  mean = (R)(s / n), s a double chain over R partial sums of four
 *         (cv::mean); m = max(1, |coordinates|) (the row of ones takes part; NaN ignored); T = scale * offset with
 *         scale = diag(w, w, 1), w = (R)(1.0 / (double)m), offset = [1 0 -mean_x; 0 1 -mean_y; 0 0 1]; the points
 *         T [x y 1]^T; F_Hat = rank reduction of the normal-equation solve; F = (T_b^T F_Hat) T_a.
 *   epipolar end points (Solution.cpp:124-163, :343-362)  side 0: l = (p^T F)^T for p of image B, lines in image A;
 *         side 1: l = F p for p of image A.  I_L = (0,0,1) x (0,rows-1,1), I_R = (cols-1,0,1) x (cols-1,rows-1,1);
 *         P = l x I (cv::Mat::cross in R), then P * (R)(1.0 / (double)P_2).  out [n][6] = P_iL, P_iR.
 *   camera centre (Solution.cpp:320-326)  Q^-1 by the closed form of the RANSAC block (determinant and cofactors in
 *         double, each rounded to R, zeros when det = 0), centre_r = (R)(-1.0 * ((q_r0 m_03 + q_r1 m_13) + q_r2 m_23)).
 * Degenerate systems (too few constraints, repeated points, NaN / inf points) run as written and give inf / NaN.
 * Limits: n <= 2^24, j <= 64, at most 64 groups, k <= 1024 for the SVD.  Shared scratch: one call at a time per
 * context, as everywhere. */
#define MICV_GEOM_F64 1u

/* calib::solveLeastSquares for T index subsets, the trial of Solution.cpp:243-318 and its arg-min in ONE call.
 * Trial t takes indices[t][0 .. kc-1] as constraints, kc = kcount ? kcount[t] : k (kcount device, each <= k), and the
 * next j entries as test points: the first kc + j entries of a permutation, as genUniqueRands hands them out.
 * group_sizes (HOST, G entries summing to T, or NULL with G = 0) are the reference's set sizes' trial counts.
 * Out (device): M [T][12] f32, residual [T] f64, and, unless the three are NULL, G + 1 arg-min records (the groups,
 * then all trials): best_idx [G+1] i32, best_res [G+1] f64, best_M [G+1][12] f32.  T = 1, j = 0, indices NULL is the
 * plain calib::solveLeastSquares of the first k points. */
int micv_calib_ls_trials_dev(micv_ctx *ctx, const float *pts2d, const float *pts3d, int n, const int32_t *indices,
                             int stride, int k, int j, int T, const int32_t *kcount, const int *group_sizes, int G,
                             uint32_t flags, float *M, double *residual, int32_t *best_idx, double *best_res,
                             float *best_M, int32_t *status, micv_stream stream);
int micv_calib_ls_trials_host(micv_ctx *ctx, const float *pts2d, const float *pts3d, int n, const int32_t *indices,
                              int stride, int k, int j, int T, const int32_t *kcount, const int *group_sizes, int G,
                              uint32_t flags, float *M, double *residual, int32_t *best_idx, double *best_res,
                              float *best_M);
/* calib::solveSVD for T index subsets of k points each: M [T][12]. */
int micv_calib_svd_dev(micv_ctx *ctx, const float *pts2d, const float *pts3d, int n, const int32_t *indices, int stride,
                       int k, int T, uint32_t flags, float *M, int32_t *status, micv_stream stream);
int micv_calib_svd_host(micv_ctx *ctx, const float *pts2d, const float *pts3d, int n, const int32_t *indices, int stride,
                        int k, int T, uint32_t flags, float *M);
/* fundamental::solveLeastSquares for T index subsets of k correspondences: F [T][9]. */
int micv_fundamental_ls_dev(micv_ctx *ctx, const float *ptsA, const float *ptsB, int n, const int32_t *indices,
                            int stride, int k, int T, uint32_t flags, float *F, int32_t *status, micv_stream stream);
int micv_fundamental_ls_host(micv_ctx *ctx, const float *ptsA, const float *ptsB, int n, const int32_t *indices,
                             int stride, int k, int T, uint32_t flags, float *F);
/* fundamental::rankReduce of T 3 x 3 matrices (row-major). */
int micv_fundamental_rank_reduce_dev(micv_ctx *ctx, const float *F, int T, uint32_t flags, float *out,
                                     micv_stream stream);
int micv_fundamental_rank_reduce_host(micv_ctx *ctx, const float *F, int T, uint32_t flags, float *out);
/* The extra-credit chain: Ta, Tb, Fhat, F, 9 f32 each. */
int micv_fundamental_normalized_dev(micv_ctx *ctx, const float *ptsA, const float *ptsB, int n, uint32_t flags,
                                    float *Ta, float *Tb, float *Fhat, float *F, micv_stream stream);
int micv_fundamental_normalized_host(micv_ctx *ctx, const float *ptsA, const float *ptsB, int n, uint32_t flags,
                                     float *Ta, float *Tb, float *Fhat, float *F);
int micv_epipolar_endpoints_dev(micv_ctx *ctx, const float *F, const float *pts, int n, int side, int rows, int cols,
                                uint32_t flags, float *out, micv_stream stream);
int micv_epipolar_endpoints_host(micv_ctx *ctx, const float *F, const float *pts, int n, int side, int rows, int cols,
                                 uint32_t flags, float *out);
/* Camera centres of T projection matrices M [T][12]: center [T][3]. */
int micv_camera_center_dev(micv_ctx *ctx, const float *M, int T, uint32_t flags, float *center, micv_stream stream);
int micv_camera_center_host(micv_ctx *ctx, const float *M, int T, uint32_t flags, float *center);

/* genUniqueRands (Solution.cpp:68-96) on the shared engine of the RANSAC block: per trial a FRESH iota 0 .. n-1,
 * std::shuffle'd (libstdc++) by the engine -- unlike ransac::solve's persistent vector.  out [trials][n] receives the
 * whole permutations (the first k are the constraints, the next j the test points); the engine advances by `trials`
 * shuffles.  Host-side, no device work. */
int micv_geom_trial_indices(micv_ransac_rng *rng, int64_t n, int trials, int32_t *out);
/* For batches too large to draw on the host: `count` distinct indices of [0, n) per trial, on the device, NOT the
 * reference's sequence.  Trial t, entry e = 0 .. count-1, attempt a = 0, 1, ..:
 *     r = splitmix64(seed ^ ((uint64)t << 32 | (uint64)e << 20 | (a & 0xFFFFF))), idx = ((r >> 32) * n) >> 32
 * (splitmix64 as in the RANSAC block); the first attempt whose idx differs from the trial's earlier entries is entry e.
 * out [T][count] i32 (device); count <= min(n, 4096), T < 2^31. */
int micv_geom_sample_indices_dev(micv_ctx *ctx, uint64_t seed, int n, int count, int64_t T, int32_t *out,
                                 micv_stream stream);

/* ------------------------------------------------------------------ ps5: driver ------ */
/* What ProblemSets/ps5_cpp/src/Solution.cpp does around lk:: and pyr::, on the device: every runProblem* of ps5 runs
 * from the uploaded frames to the images it would write without a host synchronisation.  The drawing and the montage
 * follow shim/micv_viz.hpp (drawVelocityVectors, arrowed_line, line, savePyramid), which restates OpenCV 3.4.1's
 * cv::arrowedLine / cv::LineIterator / cv::resize(INTER_NEAREST) / cv::normalize, PARITY UNPINNED;
 * the `_dev` forms equal those host loops byte for byte (see DESIGN.md for the one condition, a tip point within an ulp
 * of a rounding tie, which no lattice point can meet).  Every `_dev` entry is asynchronous on `stream`; every `_host`
 * entry uploads, runs the same kernels and downloads. */

/* drawVelocityVectors (Solution.cpp:13-37): on `batch` 8-bit 3-channel interleaved images (image i at img + i*img_pitch,
 * rows `stride` bytes apart), drawn on in place, the arrows (x, y) -> (x + u, y + v) at the lattice points
 * y = 0, max(1, rows/30), ..., x = 0, max(1, cols/30), ... of field i (u + i*field_pitch bytes, rows `fstride` bytes
 * apart).  A lattice point whose u or v is not finite or exceeds 1e6 in magnitude draws nothing.  End points are lrint of
 * the float32 sums; tip length, angle and tip points in double; every stroke is cv::LineIterator's walk, each pixel
 * bounds-checked.  color: 3 bytes, stored as they are.  rows, cols <= 32767; batch <= 65535. */
int micv_draw_velocity_vectors_dev(micv_ctx *ctx, uint8_t *img, size_t img_pitch, size_t stride, const float *u, const float *v,
                                   size_t field_pitch, size_t fstride, int batch, int rows, int cols, const uint8_t *color,
                                   micv_stream stream);
int micv_draw_velocity_vectors_host(micv_ctx *ctx, uint8_t *img, size_t img_pitch, size_t stride, const float *u, const float *v,
                                    size_t field_pitch, size_t fstride, int batch, int rows, int cols, const uint8_t *color);
/* prevImg.clone() and, for a grey frame, cv::cvtColor(GRAY2RGB) (Solution.cpp:66, :17-19): the 3-channel image the
 * arrows are drawn on, so that they never touch the caller's frame.  depth MICV_DEPTH_8U and 1 or 3 channels; anything
 * else is MICV_EINVAL (micv_viz::drawVelocityVectors requires 8 bit as well). */
int micv_gray_or_bgr_to_bgr8_dev(micv_ctx *ctx, const void *src, int depth, int channels, int rows, int cols, size_t sstride,
                                 uint8_t *dst, size_t dstride, micv_stream stream);
int micv_gray_or_bgr_to_bgr8_host(micv_ctx *ctx, const void *src, int depth, int channels, int rows, int cols, size_t sstride,
                                  uint8_t *dst, size_t dstride);
/* savePyramid (Solution.cpp:86-99): levels[0..3] with the sizes the caller gives (level 0 is R x C; the others need not
 * be R >> l), depth MICV_DEPTH_32F or MICV_DEPTH_8U, into one 2R x 2C 8-bit image, level k at tile (k / 2, k % 2).
 * 32F levels are normalised first, each by its own range, with the arithmetic of micv_normalize_minmax_* (NaNs are
 * ignored by the range and give 0; a range <= DBL_EPSILON gives scale 0); a tile pixel (y, x) shows the level's pixel
 * (min((int)floor(y * ((double)rows_k / R)), rows_k - 1), likewise x): cv::resize(INTER_NEAREST).  Two launches (the
 * four ranges, the montage); one for 8U.  With micv_laplacian_pyramid_dev in front this is ps5-2-b-1.  Level sizes up
 * to 16383. */
int micv_pyramid_montage_dev(micv_ctx *ctx, const void *const *levels, const int *level_rows, const int *level_cols,
                             const size_t *level_strides, int depth, uint8_t *dst, size_t dstride, micv_stream stream);
int micv_pyramid_montage_host(micv_ctx *ctx, const void *const *levels, const int *level_rows, const int *level_cols,
                              const size_t *level_strides, int depth, uint8_t *dst, size_t dstride);
/* warpHelper's `prev - warped` (Solution.cpp:118-123) in one kernel: diff = prev - remap(next, x + du, y + dv) with
 * micv_lk_warp_dev's sample (taps, border, rounding), then one unfused f32 subtraction: bit-identical to
 * micv_lk_warp_dev followed by a subtraction.  diff must not alias an input (MICV_EINVAL). */
int micv_lk_warp_diff_dev(micv_ctx *ctx, const float *prev, size_t pstride, const float *next, size_t nstride, const float *du,
                          const float *dv, size_t fstride, int rows, int cols, float *diff, size_t dstride, micv_stream stream);
int micv_lk_warp_diff_host(micv_ctx *ctx, const float *prev, size_t pstride, const float *next, size_t nstride, const float *du,
                           const float *dv, size_t fstride, int rows, int cols, float *diff, size_t dstride);
/* warpHelper (Solution.cpp:101-128) over `nframes` grey f32 images of one size (frame t at frames + t*frame_pitch
 * bytes: one pyramid level of every frame, as micv_gaussian_pyramid_batch_dev lays it out): for every consecutive pair
 * (t - 1, t) micv_lk_flow_dev(prev, next, win) and the fused warp-diff with that flow, then ONE batched min-max
 * normalisation of the nframes - 1 differences to 8 bit (pair p at diff_u8 + p*u8_pitch).  diff_f32, u, v: optional
 * (NULL = not wanted) dense outputs, pair p at + p*rows*cols floats.  Temporaries come from the context. */
int micv_ps5_warp_diff_seq_dev(micv_ctx *ctx, const float *frames, size_t frame_pitch, int nframes, int rows, int cols,
                               size_t stride, int win, uint8_t *diff_u8, size_t u8_pitch, size_t u8_stride, float *diff_f32,
                               float *u, float *v, micv_stream stream);
/* The host form takes the frames as micv_lk_flow_seq_host does (nframes host images of one format: 1 / 3 / 4 channels,
 * 8U or 32F) plus the pyramid level: grey conversion and micv_gaussian_pyramid_batch_dev on the device, then the chain
 * on level `level` of `levels`.  Outputs are (rows >> level) x (cols >> level), dense, pair after pair. */
int micv_ps5_warp_diff_seq_host(micv_ctx *ctx, const void *const *frames, int nframes, int rows, int cols, size_t stride,
                                int channels, int depth, int levels, int level, int win, uint8_t *diff_u8, float *diff_f32,
                                float *u, float *v);
/* One denseLKWrapper (Solution.cpp:40-84) as one call: two 8-bit frames of 1 or 3 channels -> grey conversion
 * (micv_to_gray_f32_dev: naive mode converts first, :48-61; pyramidal mode hands the frames to the chain, which converts
 * them the same way, as micv_lk_flow_pyr_frames_host), the flow (micv_lk_flow_dev, or micv_lk_flow_pyr_dev with `levels`),
 * the arrows on a copy of `prev` (the two entries above), and, when jet_u / jet_v are given, the JET maps of the
 * normalised u and v: one micv_normalize_minmax_batch_dev of two where v lies behind u and jet_v behind jet_u in memory
 * (allocate each pair as one block), otherwise one micv_normalize_minmax_dev per field, with the same bytes.  The
 * caller's frames are not written. */
#define MICV_LK_NAIVE     0 /* LKMode::NAIVE */
#define MICV_LK_PYRAMIDAL 1 /* LKMode::HEIRARCHICAL (sic) */
int micv_dense_lk_display_dev(micv_ctx *ctx, const void *prev, const void *next, int rows, int cols, size_t stride, int channels,
                              int depth, int mode, int win, int levels, const uint8_t *color, float *u, float *v, size_t ostride,
                              uint8_t *arrows, size_t astride, uint8_t *jet_u, uint8_t *jet_v, size_t jstride,
                              micv_stream stream);
int micv_dense_lk_display_host(micv_ctx *ctx, const void *prev, const void *next, int rows, int cols, size_t stride, int channels,
                               int depth, int mode, int win, int levels, const uint8_t *color, float *u, float *v, size_t ostride,
                               uint8_t *arrows, size_t astride, uint8_t *jet_u, uint8_t *jet_v, size_t jstride);
/* denseLKWrapper in pyramidal mode over consecutive frames (Solution.cpp:40-84 called as :254-285 does) as one call:
 * nframes 8-bit device frames of 1 or 3 channels, laid out as micv_lk_flow_seq_async takes them.  Per pair p = (frame p,
 * frame p + 1): u and v (at + p*opair_pitch bytes), the arrows on a copy of frame p (arrows + p*apitch, rows astride
 * apart) and, when jet_u / jet_v are given, the JET maps of the normalised u and v (at + p*jpitch, rows jstride apart).
 * On the device only: micv_lk_flow_seq_async (max_pairs 0), micv_gray_or_bgr_to_bgr8_dev per frame, ONE
 * micv_draw_velocity_vectors_dev for all pairs, one micv_normalize_minmax_batch_dev for all u and one for all v.  Every
 * output of pair p holds the bytes of micv_dense_lk_display_dev(MICV_LK_PYRAMIDAL) on frames p and p + 1.  A refusal
 * enqueues nothing.  The _host form takes per-frame and per-pair host pointers with one stride each, as
 * micv_lk_flow_seq_host does: one block of frames up, one call, one block of outputs down. */
int micv_dense_lk_display_seq_async(micv_ctx *ctx, const void *frames, size_t frame_pitch, int nframes, int rows, int cols,
                                    size_t stride, int channels, int depth, int win, int levels, const uint8_t *color, float *u,
                                    float *v, size_t opair_pitch, size_t ostride, uint8_t *arrows, size_t apitch, size_t astride,
                                    uint8_t *jet_u, uint8_t *jet_v, size_t jpitch, size_t jstride, micv_stream stream);
int micv_dense_lk_display_seq_host(micv_ctx *ctx, const void *const *frames, int nframes, int rows, int cols, size_t stride, int channels,
                                   int depth, int win, int levels, const uint8_t *color, float *const *u, float *const *v, size_t ostride,
                                   uint8_t *const *arrows, size_t astride, uint8_t *const *jet_u, uint8_t *const *jet_v, size_t jstride);

/* ------------------------------------------------------------------ ps4: driver ------ */
/* What ProblemSets/ps4_cpp/src/Solution.cpp writes out between harris::, sift::, the matcher and ransac::, on the
 * device: drawDots (:59-69), cv::hconcat, cv::drawKeypoints with random colours (:147-158), the match lines (:190-207)
 * and the consensus lines (:240-250).  OpenCV's source is not available to this repository, so its drawing is restated,
 * PARITY UNPINNED (DESIGN.md sections 2 and 3); the statement of the contract is the host loops of shim/micv_ps4.hpp,
 * and the `_dev` forms equal them byte for byte.  Every `_dev` entry is asynchronous on `stream`, reads its counts on
 * the device and never synchronises; every `_host` entry uploads, runs the same kernels and downloads.
 * Painter's order: every glyph and every line has a colour of its own, and the result is what drawing stroke 0, 1, ..
 * one after the other would leave: the stroke of the highest index owns a pixel that several strokes cross.
 * Colours come from cv::RNG (state = (uint32)state * 4164903690 + (state >> 32), a draw is the low word).  One colour
 * is three draws d0, d1, d2 in that order, reduced modulo m and stored as bytes {d2 % m, d1 % m, d0 % m}: the
 * reference's toolchain evaluates the arguments of cv::Scalar(..) right to left.  A state or seed of 0 is taken as
 * 0xffffffff.  At most 2^24 strokes per call. */

/* drawDots: dst (8-bit, 3 channels) = the grey image (MICV_DEPTH_32F converted by saturate_cast<uchar>(cvRound(v)) as
 * micv_gray_to_rgb8_*, or MICV_DEPTH_8U) replicated to three channels, and (0, 0, 255) where the byte that
 * micv_normalize_minmax_* stores for `corners` (f32, the sparse map of micv_harris_refine_*) is non-zero.  As the
 * reference wrote it: a corner weaker than about 1/510 of the strongest is not dotted, a map with a negative entry dots
 * every pixel except the minimum's, an all-equal map dots nothing, NaN entries are never dotted. */
int micv_draw_dots_dev(micv_ctx *ctx, const void *gray, int depth, int rows, int cols, size_t gstride, const float *corners,
                       size_t cstride, uint8_t *dst, size_t dstride, micv_stream stream);
int micv_draw_dots_host(micv_ctx *ctx, const void *gray, int depth, int rows, int cols, size_t gstride, const float *corners,
                        size_t cstride, uint8_t *dst, size_t dstride);
/* cv::hconcat of two 8-bit images of `rows` rows and bpp = 1 or 3 bytes per pixel: dst = [a | b], every side pitched. */
int micv_hconcat_dev(micv_ctx *ctx, const uint8_t *a, size_t astride, int acols, const uint8_t *b, size_t bstride, int bcols,
                     int rows, int bpp, uint8_t *dst, size_t dstride, micv_stream stream);
int micv_hconcat_host(micv_ctx *ctx, const uint8_t *a, size_t astride, int acols, const uint8_t *b, size_t bstride, int bcols,
                      int rows, int bpp, uint8_t *dst, size_t dstride);
/* cv::drawKeypoints(src, kp, out, Scalar::all(-1), DRAW_RICH_KEYPOINTS) into the column window [x0, x0 + cols) of a BGR
 * canvas of canvas_cols columns: the window receives src (8-bit, 1 or 3 channels; NULL: the canvas keeps what it holds)
 * and then glyph j = 0 .. n-1, n = min(*count, cap) read on the DEVICE (count and kp_xysa as micv_harris_refine_dev and
 * micv_sift_keypoints_dev leave them).  Glyph j: a thickness-1 circle (the midpoint walk of micv_draw_circles_*) of
 * centre (cvRound(x), cvRound(y)) and radius cvRound(size / 2), ties to even, and, unless angle == -1, a stroke
 * (micv_viz::line's walk) from the centre to centre + (cvRound(c * radius), cvRound(s * radius)), (s, c) the fixed
 * polynomial sine and cosine of the descriptor window at `angle` degrees.  8-connected glyphs are a decision of this
 * library (OpenCV draws them anti-aliased).  Glyphs are clipped to the window.  A keypoint whose x or y is not finite or
 * is 1e9 or more in magnitude, or whose size / 2 is not in [0, 32767], draws nothing; an angle that is not finite or is
 * 1e9 or more in magnitude draws no stroke.  Every keypoint takes its colour (modulo 256) whether it draws or not:
 * *rng_state (a DEVICE word) advances by exactly 3 n draws, so the next panel continues the generator.
 * The `_host` form takes n and the state word in host memory. */
int micv_draw_keypoints_dev(micv_ctx *ctx, const uint8_t *src, int channels, int rows, int cols, size_t sstride, uint8_t *canvas,
                            int canvas_cols, size_t cstride, int x0, const float *kp_xysa, const int64_t *count, int64_t cap,
                            uint64_t *rng_state, micv_stream stream);
int micv_draw_keypoints_host(micv_ctx *ctx, const uint8_t *src, int channels, int rows, int cols, size_t sstride, uint8_t *canvas,
                             int canvas_cols, size_t cstride, int x0, const float *kp_xysa, int64_t n, uint64_t *rng_state);
/* The lines of siftHelper and ransacHelper on a BGR canvas (rows x cols, drawn on in place): for match i < n =
 * min(*count, cap) (matches_qt and the DEVICE count of micv_bf_ratio_filter_dev), from (cvRound(kp_a[q].x),
 * cvRound(kp_a[q].y)) to (cvRound(kp_b[t].x + x_offset), cvRound(kp_b[t].y)), the sum in float, micv_viz::line's walk,
 * every pixel bounds-checked.  mask (u8 [cap], or NULL = all): match i is drawn iff mask[i] != 0, so inlier_mask of
 * micv_ransac_solve*_dev goes straight in.  A match whose q is outside [0, na) or whose t is outside [0, nb) is skipped,
 * and so are its draws.  The r-th DRAWN line (r = drawn matches before it) takes draws 3r .. 3r+2 (modulo 255:
 * rng.uniform(0, 255)) of a generator seeded with `seed` per call (the reference: 12345).  A drawn line with an end
 * point that is not finite or is 1e9 or more in magnitude paints nothing and keeps its draws. */
int micv_draw_match_lines_dev(micv_ctx *ctx, uint8_t *canvas, int rows, int cols, size_t stride, const float *kp_a, int64_t na,
                              const float *kp_b, int64_t nb, const int32_t *matches_qt, const int64_t *count, int64_t cap,
                              const uint8_t *mask, int x_offset, uint64_t seed, micv_stream stream);
int micv_draw_match_lines_host(micv_ctx *ctx, uint8_t *canvas, int rows, int cols, size_t stride, const float *kp_a, int64_t na,
                               const float *kp_b, int64_t nb, const int32_t *matches_qt, int64_t n, const uint8_t *mask,
                               int x_offset, uint64_t seed);
/* harrisHelper (Solution.cpp:71-132) as one call: micv_harris_corners_dev with its four fields in `fields`
 * ([4][rows * cols] f32, dense: gx, gy, R, corners), then the three pictures: grad_panel (rows x 2 cols, the normalised
 * gx beside the normalised gy, :80-86), resp_u8 (the normalised R, :108) and dots (micv_draw_dots of img and corners).
 * The four ranges come from one min-max launch; the bytes are those of the separate calls. */
int micv_ps4_harris_display_dev(micv_ctx *ctx, const float *img, int rows, int cols, size_t stride, int sobel_ksize, int win,
                                double sigma, float alpha, int flags, double threshold, int min_distance, float *fields,
                                int32_t *locs_yx, int64_t cap, int64_t *count, uint8_t *grad_panel, size_t gstride,
                                uint8_t *resp_u8, size_t rstride, uint8_t *dots, size_t dstride, micv_stream stream);
int micv_ps4_harris_display_host(micv_ctx *ctx, const float *img, int rows, int cols, size_t stride, int sobel_ksize, int win,
                                 double sigma, float alpha, int flags, double threshold, int min_distance, float *fields,
                                 int32_t *locs_yx, int64_t cap, int64_t *count, uint8_t *grad_panel, size_t gstride,
                                 uint8_t *resp_u8, size_t rstride, uint8_t *dots, size_t dstride);
/* The two pictures of siftHelper as one call, asynchronous on one stream: keypoint_panel (optional) = both grey 8-bit
 * images side by side with their glyphs (A's, then B's continuing *rng_state), match_panel = the same plus the lines
 * (x_offset = cols_a; the index bounds of the lines are cap_a and cap_b).  With MICV_PS4_NO_GLYPHS no glyph is drawn
 * and *rng_state stays: match_panel is the grey pair expanded to BGR with the masked lines, ransacHelper's picture. */
#define MICV_PS4_NO_GLYPHS 1
int micv_ps4_match_panels_dev(micv_ctx *ctx, const uint8_t *img_a, size_t astride, int cols_a, const uint8_t *img_b, size_t bstride,
                              int cols_b, int rows, const float *kp_a, const int64_t *count_a, int64_t cap_a, const float *kp_b,
                              const int64_t *count_b, int64_t cap_b, const int32_t *matches_qt, const int64_t *match_count,
                              int64_t match_cap, const uint8_t *mask, int flags, uint64_t seed, uint64_t *rng_state,
                              uint8_t *keypoint_panel, uint8_t *match_panel, size_t pstride, micv_stream stream);
int micv_ps4_match_panels_host(micv_ctx *ctx, const uint8_t *img_a, size_t astride, int cols_a, const uint8_t *img_b, size_t bstride,
                               int cols_b, int rows, const float *kp_a, int64_t n_a, const float *kp_b, int64_t n_b,
                               const int32_t *matches_qt, int64_t n_matches, const uint8_t *mask, int flags, uint64_t seed,
                               uint64_t *rng_state, uint8_t *keypoint_panel, uint8_t *match_panel, size_t pstride);

/* ------------------------------------------------------------------ ps6: driver ------ */
/* What pfDriver (ProblemSets/ps6_cpp/src/Solution.cpp:16-107) does around ParticleFilter::tick, on the device: the dot
 * per particle of ParticleFilter::drawParticles, cv::rectangle around the estimate, and the loop itself with the frames
 * the driver keeps coming back annotated.  OpenCV's source is not available to this repository, so its drawing is
 * restated, PARITY UNPINNED ("ps6 driver"); the statement of the contract is the two host loops of
 * the shim, ParticleFilter::drawParticles (shim/micv_shim.hpp) and micv_viz::rectangle (shim/micv_viz.hpp), and the
 * device forms equal them byte for byte.  Every `_dev` entry is asynchronous on `stream`, reads particles and the
 * estimate on the device and never synchronises; MICV_EINVAL is returned before anything is enqueued.
 * Images: 8-bit, 1, 3 or 4 interleaved channels, rows and cols in 1 .. 32767, `stride` bytes per row (>= cols *
 * channels, < 2^32); only the first min(channels, 4) bytes of a painted pixel are written, padding never.
 * Colours: four doubles; byte k of a painted pixel is saturate(nearbyint(color[k])) (NaN gives 0).
 * Dots (cv::circle(img, p, 1, color, -1) restated): a particle is skipped unless -2 < p.x < cols + 2 and
 *   -2 < p.y < rows + 2 in float (NaN is skipped); the centre is (nearbyint(p.x), nearbyint(p.y)), halves to even; the
 *   dot is the centre and its four neighbours, each clipped to the image.
 * Rectangle (cv::rectangle(img, Rect(x, y, w, h), color), thickness 1): nothing when w <= 0 or h <= 0, otherwise the
 *   one-pixel ring of [x, x + w - 1] x [y, y + h - 1] (64-bit arithmetic, x may be INT_MIN) intersected with the image.
 * The driver's box around the estimate c (:76-78), bbox_w and bbox_h floats: x = cvRound(c.x - bbox_w / 2),
 *   y = cvRound(c.y - bbox_h / 2), w = cvRound(bbox_w), h = cvRound(bbox_h), the subtraction and the halving in float;
 *   cvRound rounds halves to even and gives INT_MIN for NaN, +-inf and every value outside int.
 * Order: dots first, box second; the box wins wherever they overlap.  All in one launch. */
/* xy: n x {x, y} f32 (device for _dev), 0 <= n; n = 0 is a no-op. */
int micv_draw_particles_dev(micv_ctx *ctx, uint8_t *img, int rows, int cols, int channels, size_t stride, const float *xy, int n,
                            const double *color, micv_stream stream);
int micv_draw_particles_host(micv_ctx *ctx, uint8_t *img, int rows, int cols, int channels, size_t stride, const float *xy, int n,
                             const double *color);
int micv_draw_rectangle_dev(micv_ctx *ctx, uint8_t *img, int rows, int cols, int channels, size_t stride, int x, int y, int w, int h,
                            const double *color, micv_stream stream);
int micv_draw_rectangle_host(micv_ctx *ctx, uint8_t *img, int rows, int cols, int channels, size_t stride, int x, int y, int w, int h,
                             const double *color);
/* The driver's overlay of a caller's particle list: the dots, then the box around centre[0..1] (device memory for _dev:
 * the estimate where a chain left it). */
int micv_ps6_overlay_list_dev(micv_ctx *ctx, uint8_t *img, int rows, int cols, int channels, size_t stride, const float *xy, int n,
                              const double *dot_color, const float *centre, float bbox_w, float bbox_h, const double *box_color,
                              micv_stream stream);
int micv_ps6_overlay_list_host(micv_ctx *ctx, uint8_t *img, int rows, int cols, int channels, size_t stride, const float *xy, int n,
                               const double *dot_color, const float *centre, float bbox_w, float bbox_h, const double *box_color);
/* The same from the filter's own device state, in place in `frame` (device, the filter's rows x cols x channels): its
 * current particles and the box around its current mean.  Ordered behind the ticks enqueued on `stream`. */
int micv_ps6_overlay_dev(micv_pf *pf, uint8_t *frame, size_t stride, const double *dot_color, float bbox_w, float bbox_h,
                         const double *box_color, micv_stream stream);
/* One pass of pfDriver's loop body: micv_pf_tick_dev on `frame`, then the overlay into `out`.  out may be the frame
 * itself (then ostride == stride); a separate out receives a copy of the frame first and the frame stays as it is.  The
 * overlay is ordered after the model update, so the tracker never sees the paint.  _host: upload, the same, download of
 * out and the state, sync (null stream, as micv_pf_tick_host). */
int micv_ps6_tick_display_dev(micv_pf *pf, const uint8_t *frame, size_t stride, uint8_t *out, size_t ostride, const double *dot_color,
                              float bbox_w, float bbox_h, const double *box_color, micv_stream stream, micv_pf_state *state_dev);
int micv_ps6_tick_display_host(micv_pf *pf, const uint8_t *frame, size_t stride, uint8_t *out, size_t ostride, const double *dot_color,
                               float bbox_w, float bbox_h, const double *box_color, micv_pf_state *state);
/* pfDriver as one call over host frames, on the pattern of micv_pf_track_seq_host: two frame buffers, the upload of
 * frame t + 1 beside tick t, the overlay painted in place in the device buffer, and a download of only the frames that
 * are kept: out_frames[k] (rows x cols x channels u8, ostride bytes per row) receives frame save[k] (0-based, the
 * driver's saveFrames; an index may repeat), or with all_frames != 0 frame k for every k < nframes (what the driver
 * hands to the video writer; save is ignored).  The next upload into a buffer waits for that buffer's download.  states:
 * nframes entries, bit-identical to micv_pf_track_seq_host.  MICV_EINVAL for a save index outside 0 .. nframes - 1.
 * Two streams of its own, like micv_pf_track_seq_host.  Blocking. */
int micv_ps6_track_display_seq_host(micv_pf *pf, const uint8_t *const *frames, int nframes, size_t stride, const double *dot_color,
                                    float bbox_w, float bbox_h, const double *box_color, const int *save, int nsave, int all_frames,
                                    uint8_t *const *out_frames, size_t ostride, micv_pf_state *states);
/* The same for a group over one host video (micv_pf_group_track_seq_host with the driver's pictures): every member gets
 * its OWN annotated pictures, as the reference's six pfDriver runs each paint their own copy of the video.  For every
 * frame t that member k keeps (t in save[k][0 .. nsave[k]), or every frame with all_frames != 0) the device frame buffer
 * is copied into a scratch picture, painted there by the overlay launch above from member k's particles and state
 * (bbox_wh[k] = {width, height} of its box) and downloaded into out_frames[k][j]; the frame buffer itself is never
 * painted, and the next upload into it waits for these copies as for the tick.  save, nsave and out_frames: count
 * entries; save[k] / out_frames[k] may be NULL where member k keeps nothing.  out_frames[k][j] and states[t][k]
 * ([nframes][count]) are byte-identical to micv_ps6_track_display_seq_host on member k alone with the same save list;
 * the argument rules of that call hold per member.  Blocking. */
int micv_ps6_group_track_display_seq_host(micv_pf_group *g, const uint8_t *const *frames, int nframes, size_t stride,
                                          const double *dot_color, const float *bbox_wh, const double *box_color,
                                          const int *const *save, const int *nsave, int all_frames,
                                          uint8_t *const *const *out_frames, size_t ostride, micv_pf_state *states);

/* ------------------------------------------------------------------ ps0 ------ */
/* ps0 of the reference (ProblemSets/ps0_cpp/main.cpp) on the device.  OpenCV's behaviour is restated, PARITY UNPINNED
 * ("ps0"); the statement of the contract is the host loops of shim/micv_ps0.hpp, and the `_dev` forms
 * equal them byte for byte.  All images are 8-bit; strides are bytes per row, padding is never written.  `_dev` entries
 * are asynchronous on `stream`, never synchronise the host and read every scalar they depend on from device memory;
 * `_host` entries upload, run the same kernels and download (null stream).  rows * cols < 2^31.
 *   cvRound  rounds halves to even and gives INT_MIN for NaN, +-inf and values outside int; sat (to u8) then gives 0. */
typedef struct micv_ps0_stats {
    double mean, stddev;
    uint64_t sum, sqsum;
    int32_t min, max;
} micv_ps0_stats;
/* cv::mixChannels on one image: dst channel k = src channel map[k] (map on the host, dcn entries, 1 <= scn, dcn <= 4; an
 * entry outside the source is MICV_EINVAL).  swapRedBlue (main.cpp:17-23) is scn = dcn = 3, map {2, 1, 0};
 * cv::extractChannel (:118, :123, :129, :169) is dcn = 1. */
int micv_mix_channels_u8_dev(micv_ctx *ctx, const uint8_t *src, int rows, int cols, int scn, size_t sstride, const int *map, uint8_t *dst,
                             int dcn, size_t dstride, micv_stream stream);
int micv_mix_channels_u8_host(micv_ctx *ctx, const uint8_t *src, int rows, int cols, int scn, size_t sstride, const int *map, uint8_t *dst,
                              int dcn, size_t dstride);
/* pixelReplacement (:25-42): dst (rows2 x cols2) = img2 with the size x size square of img1 at (cols1 / 2 - size / 2,
 * rows1 / 2 - size / 2) pasted at (cols2 / 2 - size / 2, rows2 / 2 - size / 2), integer division; the driver's size is 100.
 * The images may differ in size and share `channels` (1..4).  A square that leaves either image is MICV_EINVAL (OpenCV
 * throws there).  One launch; dst must not alias an input. */
int micv_pixel_replacement_u8_dev(micv_ctx *ctx, const uint8_t *img1, int rows1, int cols1, size_t stride1, const uint8_t *img2, int rows2,
                                  int cols2, size_t stride2, int channels, int size, uint8_t *dst, size_t dstride, micv_stream stream);
int micv_pixel_replacement_u8_host(micv_ctx *ctx, const uint8_t *img1, int rows1, int cols1, size_t stride1, const uint8_t *img2, int rows2,
                                   int cols2, size_t stride2, int channels, int size, uint8_t *dst, size_t dstride);
/* cv::minMaxLoc + cv::meanStdDev (:135-138) of a single-channel image into a record (device for _dev): sum and sqsum are
 * exact integers, mean = (double)sum * (1.0 / N), stddev = sqrt(max((double)sqsum * (1.0 / N) - mean * mean, 0.0)), unfused,
 * N = rows * cols.  Two launches: one partial per workgroup (a thread sums at most 8192 pixels in 32 bits, everything
 * after that in 64), then one workgroup adds the partials; no workgroup waits for another, and the result does not
 * depend on the grid. */
int micv_mean_stddev_u8_dev(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t stride, micv_ps0_stats *stats, micv_stream stream);
int micv_mean_stddev_u8_host(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t stride, micv_ps0_stats *stats);
/* doArithmeticOperations (:47-56): the four in-place steps of an 8-bit cv::Mat, each saturating before the next, one kernel:
 *   t1 = sat(cvRound((double)p - mean)); t2 = sat(cvRound((float)t1 * a)), a = (float)(1.0 / stddev);
 *   t3 = sat(cvRound((float)t2 * 10.f)); t4 = sat(cvRound((double)t3 + mean)).
 * stddev = 0 runs as written: a = inf, 0 * inf = NaN -> 0.  _dev: mean_stddev points at {mean, stddev} on the device, the
 * head of micv_ps0_stats; _host takes the two doubles. */
int micv_ps0_arithmetic_u8_dev(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t sstride, const double *mean_stddev, uint8_t *dst,
                               size_t dstride, micv_stream stream);
int micv_ps0_arithmetic_u8_host(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t sstride, double mean, double stddev, uint8_t *dst,
                                size_t dstride);
/* `a -= b` on 8-bit images (:156-157): sat(a - b); the bytes of micv_add_weighted_*(a, 1, b, -1, 0). */
int micv_subtract_sat_u8_dev(micv_ctx *ctx, const uint8_t *a, size_t astride, const uint8_t *b, size_t bstride, int rows, int cols, uint8_t *dst,
                             size_t dstride, micv_stream stream);
int micv_subtract_sat_u8_host(micv_ctx *ctx, const uint8_t *a, size_t astride, const uint8_t *b, size_t bstride, int rows, int cols, uint8_t *dst,
                              size_t dstride);
/* addGaussianNoise (:64-79) as the reference wrote it: `noise` is a float plane holding z * sigma + mean as
 * micv_cv_randn_f32_host draws it; n = sat_s8(cvRound(noise)) (cv::randn into CV_8SC1; a NaN sample is -128), and
 * out = max(0, clamp(min(p, 127) + n, -128, 127)).  The clip of the image at 127 is the reference's
 * image.convertTo(output, CV_8SC1) (:76): a bright pixel loses its value before the noise is added. */
int micv_add_noise_s8_u8_dev(micv_ctx *ctx, const uint8_t *src, size_t sstride, const float *noise, size_t nstride, int rows, int cols,
                             uint8_t *dst, size_t dstride, micv_stream stream);
int micv_add_noise_s8_u8_host(micv_ctx *ctx, const uint8_t *src, size_t sstride, const float *noise, size_t nstride, int rows, int cols,
                              uint8_t *dst, size_t dstride);
/* main.cpp:110-171 as one call, THREE launches: image1 and image2 are B, G, R.  Pass one reads image1 once, writes
 * `swapped` and the green and red planes and reduces green's partials; a paste launch makes `replaced` (rows2 x cols2) from
 * the red channels of the two images; pass two forms mean and stddev from the integer sums in its prologue, writes the
 * record, and writes the arithmetic image, green translated by (-2, 0) with zero fill (the bytes of micv_warp_affine_* with
 * m = {1, 0, -2, 0, 1, 0}, flags 0), green - translated, and the noisy green and blue planes (blue is read from image1).
 * planes: seven rows1 x cols1 planes plane_pitch bytes apart, pstride bytes per row: green, red, arithmetic, translated,
 * difference, noisy green, noisy blue.  Every output equals the separate calls above byte for byte.  _host draws green's
 * noise plane, then blue's, from one generator (micv_cv_randn_f32_host on *rng_state, which comes back advanced). */
int micv_ps0_run_dev(micv_ctx *ctx, const uint8_t *image1, int rows1, int cols1, size_t stride1, const uint8_t *image2, int rows2, int cols2,
                     size_t stride2, int size, const float *noise_green, const float *noise_blue, size_t nstride, uint8_t *swapped,
                     size_t wstride, uint8_t *planes, size_t pstride, size_t plane_pitch, uint8_t *replaced, size_t rstride,
                     micv_ps0_stats *stats, micv_stream stream);
int micv_ps0_run_host(micv_ctx *ctx, const uint8_t *image1, int rows1, int cols1, size_t stride1, const uint8_t *image2, int rows2, int cols2,
                      size_t stride2, int size, uint64_t *rng_state, float noise_mean, float noise_sigma, uint8_t *swapped, size_t wstride,
                      uint8_t *planes, size_t pstride, size_t plane_pitch, uint8_t *replaced, size_t rstride, micv_ps0_stats *stats);

/* ------------------------------------------------------------------ ps3: driver ------ */
/* What runProblem2 and runExtraCredit (ProblemSets/ps3_cpp/src/Solution.cpp:323-481) do after the fundamental matrix:
 * drawEpipolarLines (:122-158) calls cv::line(img, Point2f(P_iL), Point2f(P_iR), color) for every epipolar line (:153-156).
 * OpenCV's source is not available to this repository, so its drawing is restated, PARITY UNPINNED (DESIGN.md section 2,
 * "ps3 driver"); the statement of the contract is the host loop micv_ps3::line_wide (shim/micv_ps3.hpp), and the device
 * forms equal it byte for byte.  Every `_dev` entry is asynchronous on `stream`, reads the end points on the device and
 * never synchronises; MICV_EINVAL is returned before anything is enqueued.
 * Images: 8-bit, 1, 3 or 4 interleaved channels, rows and cols in 1 .. 32768, `stride` bytes per row (>= cols *
 * channels, < 2^32); only the bytes of a painted pixel are written, padding never.
 * Colours: as for micv_draw_rectangle_*: four doubles; byte k of a painted pixel is saturate(nearbyint(color[k])).
 * End points (Point2f -> Point): each coordinate through cvRound, which rounds halves to even (2.5 -> 2, 3.5 -> 4) and
 *   gives INT_MIN for NaN, +-inf and every value outside int; INT_MIN then takes part as a number.
 * Segment: the walk of micv_viz::line (shim/micv_viz.hpp: the ends swapped when p1.x > p2.x, major = max(dx, |dy|) with
 *   the tie going to x, major + 1 steps, err = major - 2 minor) WITH ITS INTEGERS AS WIDE AS THEY NEED TO BE.  The walk in
 *   `int` overflows from |dx| or |dy| >= 2^30 on; the end points of a near-vertical epipolar line lie at |y| ~ 2^31.
 *   Here the result is exact for every pair of int32 end points: step i sits at the major coordinate start +- i and the
 *   minor coordinate start +- (2 minor i + major - 1) div (2 major), in unbounded integers.  Pixels outside the image
 *   are dropped.  All segments of a call share the colour, so the order of drawing does not matter.
 * One launch: a wave per segment, a lane per step whose major coordinate is in the image (at most max(rows, cols)).
 * 0 <= n <= 2^28; n = 0 is a no-op.  _host: upload, the same launch, download, sync (null stream). */
/* segments: n x {x1, y1, x2, y2} f32 (device for _dev). */
int micv_draw_segments_dev(micv_ctx *ctx, uint8_t *img, int rows, int cols, int channels, size_t stride, const float *segments, int n,
                           const double *color, micv_stream stream);
int micv_draw_segments_host(micv_ctx *ctx, uint8_t *img, int rows, int cols, int channels, size_t stride, const float *segments, int n,
                            const double *color);
/* drawEpipolarLines from the [n][6] block of micv_epipolar_endpoints_* (P_iL then P_iR, three floats each): the segment
 * (e[0], e[1]) -> (e[3], e[4]) for every line; e[2] and e[5] are not read.  A vertical epipolar line (l_1 = 0) meets
 * neither the left nor the right border: its end points are NaN / +-inf, both x become INT_MIN, both ends sit on one
 * side of the image and the image stays untouched (the reference hands the same values to cv::line). */
int micv_draw_epipolar_lines_dev(micv_ctx *ctx, uint8_t *img, int rows, int cols, int channels, size_t stride, const float *endpoints,
                                 int n, const double *color, micv_stream stream);
int micv_draw_epipolar_lines_host(micv_ctx *ctx, uint8_t *img, int rows, int cols, int channels, size_t stride, const float *endpoints,
                                  int n, const double *color);
/* Part c of runProblem2 and part e of runExtraCredit (:341-363, :459-475) as one call: F 3 x 3 (row-major; device for
 * _dev, where a chain left it), ptsA and ptsB n x {x, y} as micv_epipolar_endpoints_* takes them, 1 <= n <= 2^27.  outA
 * receives imgA with the lines of image B's points (side 0), outB imgB with the lines of image A's points (side 1); the
 * two pictures may differ in size and share `channels`.  out may be the picture itself (then ostride == stride); a
 * separate out receives a copy of the picture first and the picture stays as it is.  ONE launch over (image, line): a
 * wave computes the end points of its line with the device function of micv_epipolar_endpoints_dev and walks them at
 * once, so nothing but F and the points is read.  flags: MICV_GEOM_F64, passed through to the end points.  endpoints
 * (or NULL): [2][n][6], side 0 then side 1, the bits of micv_epipolar_endpoints_*.  The bytes equal
 * micv_epipolar_endpoints_* followed by micv_draw_epipolar_lines_* on each image. */
int micv_ps3_epipolar_display_dev(micv_ctx *ctx, const float *F, const float *ptsA, const float *ptsB, int n, const uint8_t *imgA,
                                  size_t astride, int rowsA, int colsA, const uint8_t *imgB, size_t bstride, int rowsB, int colsB,
                                  int channels, uint32_t flags, const double *color, uint8_t *outA, size_t oastride, uint8_t *outB,
                                  size_t obstride, float *endpoints, micv_stream stream);
int micv_ps3_epipolar_display_host(micv_ctx *ctx, const float *F, const float *ptsA, const float *ptsB, int n, const uint8_t *imgA,
                                   size_t astride, int rowsA, int colsA, const uint8_t *imgB, size_t bstride, int rowsB, int colsB,
                                   int channels, uint32_t flags, const double *color, uint8_t *outA, size_t oastride, uint8_t *outB,
                                   size_t obstride, float *endpoints);

#ifdef __cplusplus
}
#endif
#endif /* MI_CV_H */
