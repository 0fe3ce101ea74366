/*
 * gsd.h -- C ABI of libgsd.so: MI355X (gfx950) kernels for the gelslim_depth U-Net train step.
 *
 * The reference (MMintLab/gelslim_depth) is pure Python and has NO FFI of its own: every device
 * operation of its hot path is a torch (ATen) operator call.  Each entry point below therefore
 * cites the reference call site whose ATen operator(s) it replaces (paths relative to
 * /root/reference/).  A maintainer binds this library with ctypes; the
 * shipped binding is gelslim_depth_amd/_lib.py.
 *
 * Conventions
 *   - all tensors fp32, NCHW, allocated by the caller (PyTorch caching allocator); the library
 *     never allocates, frees or retains device memory;
 *   - `stream` is a hipStream_t passed as void*; kernels are launched on it and nothing
 *     synchronises (safe for hipGraph capture and for the autograd thread);
 *   - return 0 on success, a negative gsd_status otherwise; gsd_last_error() returns a
 *     thread-local message; no exceptions, no exit();
 *   - every call is re-entrant and no result depends on library state: tuning knobs (GSD_* environment
 *     variables) are read on every call; the only process-wide state is an atomic per-device cache of an
 *     idempotent launch attribute (hipFuncSetAttribute(MaxDynamicSharedMemorySize), gsd_common.h).
 *
 * "Deferred BatchNorm": a convolution never materialises relu(bn(raw)).  It writes the raw
 * convolution output plus per-block partial sums; gsd_bn_finalize turns the partials into a
 * per-channel (scale, shift); every consumer applies  max(0, raw*scale+shift)  while it loads
 * the tensor (gsd_src.scale/shift/relu).  F.pad + torch.cat (unet.py:46-48) are likewise never
 * materialised: a consumer takes up to two channel segments, each with its own extent/offset,
 * and reads zeros outside a segment's extent.
 */
#ifndef GSD_H
#define GSD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  GSD_OK = 0,
  GSD_ERR_BAD_ARG = -1,       /* null pointer, non-positive size, inconsistent shapes          */
  GSD_ERR_UNSUPPORTED = -2,   /* shape outside what the kernels tile (message says which)      */
  GSD_ERR_HIP = -3,           /* a HIP runtime call failed (message carries hipGetErrorString) */
  GSD_ERR_WORKSPACE = -4      /* caller-provided workspace too small                           */
} gsd_status;

/* Non-finite guard of a train step -- the device-side form of the reference's `if pred_loss.isnan()`
 * (train_utils/train_unet.py:371-372; there it costs a host sync and makes backward() raise).
 * words: two int32 on the device, zero-initialised by the caller.  A kernel that sees a non-finite BatchNorm
 * batch statistic (gsd_bn_finalize) or loss (gsd_loss_fwd_bwd) stores `tick` (the caller's step number,
 * never 0) into words[0]; gsd_adam_ema called with the same tick then leaves parameters, moments and EMA
 * untouched and adds 1 to words[1].  No host synchronisation; the caller reads words[1] when it likes.
 * Independently of the guard, non-finite batch statistics never reach running_mean/running_var.
 * Running statistics of a SKIPPED step: layers in front of the first bad one (and, racily, its finite channels) have
 * already been updated when the step is found bad.  A caller that wants a skipped step to leave no trace -- and every
 * data-parallel rank with the same buffers -- brackets the step with gsd_guard_snapshot / gsd_guard_restore over its
 * BatchNorm buffer arena: the restore puts the snapshot back iff words[0] == tick. */
typedef struct {
  int32_t* words;
  int32_t tick;
} gsd_guard;
int gsd_guard_snapshot(const float* live, float* snapshot, int64_t n, void* stream);
int gsd_guard_restore(const gsd_guard* guard, float* live, const float* snapshot, int64_t n, void* stream);

/* One channel segment of an input operand as a consumer sees it. */
typedef struct {
  const float* ptr;     /* element (n=0, c=0, h=0, w=0) of the stored tensor                    */
  const float* scale;   /* per-channel affine applied on load, or NULL for identity             */
  const float* shift;
  int32_t C;            /* channels in this segment                                             */
  int32_t H, W;         /* stored extent                                                        */
  int32_t off_h, off_w; /* where stored (0,0) sits in the consumer's grid (F.pad top/left)      */
  int32_t relu;         /* max(0, .) after the affine                                           */
  int32_t w_stride;     /* elements between rows (row pitch, >= W).  Kernels that take a pitched
                           operand say so; the others require w_stride == W.  With a pitch that is
                           a multiple of 4 floats (and 16-byte aligned strides) the Winograd kernels
                           move the operand as aligned 16-byte LDS-DMA pieces; columns W .. pitch-1
                           must then hold the operand's padding value (0 for a plain tensor).      */
  int32_t slack;        /* the caller vouches for this many READABLE floats before the first and after
                           the last element of the stored tensor (0: none).  With slack >= 4 the Winograd
                           dW kernel moves activation windows as 16-byte pieces straight from unaligned
                           rows -- a piece that straddles an image edge reads up to 3 floats of the
                           neighbouring row, at the tensor's two ends of the slack; the two-dimensional
                           dW form also parks masked lanes on the 4 floats in front of a plane -- a quarter
                           of the fill instructions.  (Keeps the 64-bit members aligned.)           */
  int64_t n_stride;     /* elements between images                                              */
  int64_t c_stride;     /* elements between channels                                            */
} gsd_src;

/* One channel segment of an output operand. Positions outside (H, W) after subtracting the
 * offset are dropped (this is the backward of F.pad: a crop). */
typedef struct {
  float* ptr;
  int32_t C;
  int32_t H, W;
  int32_t off_h, off_w;
  int32_t w_stride;     /* elements between rows (row pitch, >= W); see gsd_src                  */
  int64_t n_stride;
  int64_t c_stride;
} gsd_dst;

/* Addressing.  n_stride and c_stride are 64-bit and every kernel forms n * n_stride + c * c_stride in 64 bits: images and planes may
 * lie any distance apart (tests/test_gpu_far_strides_fp64.py runs every strided entry point with bases past 2^31 bytes, 2^32
 * bytes, 2^31 and 2^32 elements).  INSIDE a plane, and in a few forms inside a block's group of planes, offsets are 32-bit; where
 * an operand does not fit, the call is refused before anything is launched (GSD_ERR_UNSUPPORTED unless stated) or another
 * kernel of the same entry point takes it -- each limit is stated at its entry point below and crossed on the host in
 * tests/test_addressing_limits_cpu.py:
 *   conv3x3 (all forms)      H, W < 32768; a source plane H * w_stride < 2^31 floats ("plane too large")
 *   gsd_conv3x3_w2d          also a destination plane < 2^31 floats, and a source plane H * w_stride + 4 < 2^30 floats (its fills
 *                            address a plane by an unsigned 32-bit BYTE offset); a destination whose 12 * c_stride * 4 + plane
 *                            bytes reach 2^32 takes the 64-bit store path (same results)
 *   gsd_conv3x3_w43          a FOLDED plan (images folded into tile rows: gsd_conv3x3_w43_partial_rows counts one image) needs
 *                            N * n_stride < 2^31 floats for every source and destination ("batch too large for row folding");
 *                            the call is refused, never run unfolded: the caller sized its partial rows for the folded plan
 *   gsd_conv3x3_wgrad        the 2-D form needs 64 * c_stride * 4 < 2^31 bytes for dy and every segment, else the row form runs;
 *                            the row form moves activations as 16-byte pieces only while BN * c_stride < 2^31 floats
 *   grid.y / grid.z kernels  N, C <= 65535: gsd_maxpool2[_pitched], gsd_bnrelu_pitched, gsd_bn_bwd_reduce, gsd_bn_bwd_apply,
 *                            gsd_conv1x1_out (N), gsd_conv1x1_out_wgrad, gsd_gather_affine (B, C), gsd_gather_augment (B, Ci + Cd;
 *                            H * W < 2^30), gsd_ingest_images[_interp], gsd_[area_]resize_affine, gsd_conv3x3_dgrad_bn (Cout)
 *   gsd_conv1x1_out          dense planes (c_stride == H * W; GSD_ERR_BAD_ARG), any n_stride
 *   gsd_convT2x2_wgrad       any strides for dW; the bias gradient needs a dense dy (see there) */

/* ---- library ------------------------------------------------------------------------------ */
const char* gsd_version(void);
const char* gsd_last_error(void);
/* MFMA fragment-layout self test (v_mfma_f32_16x16x4_f32 A/B/D lane maps used by every conv
 * kernel); writes 16x16 D = A*B for asymmetric integer A (16x4), B (4x16) to `out`. */
int gsd_selftest_mfma(const float* a, const float* b, float* out, void* stream);

/* ---- weight re-layouts (cheap, once per optimiser step) ----------------------------------- */
/* mode 0: conv3x3 forward   W[Co][Ci][3][3]  -> k = ci*9+t,           m = co
 * mode 1: conv3x3 dgrad     W[Co][Ci][3][3]  -> k = co*9+(8-t) flipped, m = ci
 * mode 2: retired (the image of a ConvT forward kernel that no longer exists; the ConvT forward layout is mode 6):
 *         gsd_weight_layout_size returns 0 for it and gsd_weight_layout GSD_ERR_BAD_ARG
 * mode 3: convT   dgrad,   register-staged kernel: W[Ci][Co][2][2]  -> k = co*4+kh*2+kw,     m = ci
 * mode 4: conv3x3 forward, Winograd F(4,3) rows: k = ci*18+r*6+f, m = co   (see gsd_conv3x3_w43)
 * mode 5: conv3x3 dgrad,   Winograd F(4,3) rows: k = co*18+r*6+f (flipped kernel), m = ci
 * mode 6: convT   forward, LDS-DMA kernel: k = ci (rows padded to 32), m = co*4+kh*2+kw in 128-column blocks
 * mode 7: convT   dgrad,   LDS-DMA kernel: k = co*4+kh*2+kw (rows padded to 32), m = ci in 128-column blocks
 * mode 8: conv3x3 forward, Winograd F(2x4,3x3): k = ci*24+fr*6+fc, m = co   (see gsd_conv3x3_w2d)
 * mode 9: conv3x3 dgrad,   Winograd F(2x4,3x3): k = co*24+fr*6+fc (flipped kernel), m = ci
 * Modes 0/1 are tiled for the LDS-DMA kernel: [m-block][k row][BM] with BM = 64 (M <= 64) or 128, columns
 * permuted inside each 64-group (slot l*4+t = column t*16+l), so one K-chunk of one m-block is a contiguous LDS
 * image whose A operands are aligned float4s; mode 3 is [k row][M rounded up to 64].
 * k rows are zero-padded to whole K-chunks. gsd_weight_layout_size returns the element count; the buffer
 * must be 16-byte aligned. */
int64_t gsd_weight_layout_size(int mode, int Co, int Ci);
int gsd_weight_layout(int mode, const float* w, int Co, int Ci, float* wt, void* stream);
/* Several layouts in as few launches as possible: the 2-D Winograd images (modes 8 / 9) of all jobs in ONE launch (up to 40 per
 * launch), every other mode as gsd_weight_layout would.  `jobs` is read on the host during the call. */
typedef struct {
  const float* w;   /* (Co, Ci, 3, 3) weights */
  float* wt;        /* gsd_weight_layout_size(mode, Co, Ci) floats */
  int32_t mode, Co, Ci, reserved;
} gsd_wl_job;
int gsd_weight_layout_batch(const gsd_wl_job* jobs, int n, void* stream);

/* ---- convolution family (implicit GEMM on v_mfma_f32_16x16x4_f32) -------------------------- */
/* conv3x3, stride 1, pad 1, no bias.  Replaces aten::convolution at unet.py:11,14 (forward,
 * weights from mode 0) and the dX half of aten::convolution_backward (weights from mode 1,
 * src = gradient w.r.t. the raw output).  `partials` (optional) receives per-block
 * (sum, sum of squares) of the raw output per output channel for BatchNorm:
 * layout [n_partial_rows][2*Mpad]; gsd_conv3x3_partial_rows gives n_partial_rows. */
int gsd_conv3x3_partial_rows(int N, int H, int W, int Cout);
int gsd_conv3x3(const gsd_src* src, int nsrc, const float* wt, int Cin, int Cout,
                const gsd_dst* dst, int ndst, float* partials, int N, int H, int W, void* stream);

/* conv3x3 dX fused with the backward of the relu(bn(raw)) that produced this convolution's INPUT: instead of
 * da it writes dz = da * [raw*scale+shift > 0] to dst (one full (Cout,H,W) buffer with raw's strides) and the
 * partials hold (sum dz, sum dz*xhat) per channel, layout as gsd_conv3x3 -- saves the separate
 * gsd_bn_bwd_reduce pass (one read and one write of the tensor). aten: convolution_backward(dX) +
 * threshold_backward + the reduction half of native_batch_norm_backward (unet.py:11-16). */
int gsd_conv3x3_dgrad_bnrelu(const gsd_src* src, const float* wt, int Cin, int Cout, const gsd_dst* dst,
                             const float* raw, const float* scale, const float* shift, const float* mean,
                             const float* invstd, float* partials, int N, int H, int W, void* stream);

/* The same two operators with the Winograd F(4,3) minimal-filtering identity along image rows (half the MFMA work,
 * same fp32 storage and accumulation; weights from gsd_weight_layout modes 4 (forward) / 5 (dX):
 * [m-block of 64][k row = ci*18 + r*6 + f][64], U = G g per kernel row r).  gsd_conv3x3_algo says which form the
 * library prefers for a shape (0 direct, 1 Winograd: tile padding can eat the gain on small images); the caller
 * lays the weights out for the form it calls.  Partial-row layout as gsd_conv3x3, its own row count.
 * A plan that folds images into tile rows (small H * W, N > 1; GSD_W43_FOLD=0 switches folding off) carries n * n_stride in
 * 32-bit lane offsets: with N * n_stride >= 2^31 floats for any source or destination the call returns GSD_ERR_UNSUPPORTED
 * ("batch too large for row folding") and launches nothing.  It does not fall back to the unfolded plan: gsd_conv3x3_w43_partial_rows
 * depends on the shape alone and told the caller the folded row count. */
int gsd_conv3x3_algo(int N, int H, int W, int Cin, int Cout);
int gsd_conv3x3_w43_partial_rows(int N, int H, int W, int Cout);
int64_t gsd_conv3x3_w43_mfma_count(int N, int H, int W, int Cin, int Cout);
int gsd_conv3x3_w43(const gsd_src* src, int nsrc, const float* wt, int Cin, int Cout,
                    const gsd_dst* dst, int ndst, float* partials, int N, int H, int W, void* stream);
int gsd_conv3x3_w43_dgrad_bnrelu(const gsd_src* src, const float* wt, int Cin, int Cout, const gsd_dst* dst,
                                 const float* raw, const float* scale, const float* shift, const float* mean,
                                 const float* invstd, float* partials, int N, int H, int W, void* stream);
/* "K slab" form of the two Winograd entry points for launches whose tile grid leaves most of the chip idle (the 40x53 and
 * 20x26 levels at small per-GPU batches: 150-600 blocks for 512 block slots): the input channels are cut into S slabs, block
 * (tile, slab) writes its un-reduced output tile to `ws`, and a second launch adds the slabs in slab order (run-to-run
 * bitwise) and runs the usual epilogue (crop, statistics, fused BatchNorm-backward).  gsd_conv3x3_w43_workspace gives the
 * floats of scratch the library would like for a shape (0: it runs the shape unsplit); a smaller or null `ws` reduces S, down
 * to the plain launch.  The rounding differs from the unsplit launch (two partial sums instead of one), so a caller that
 * needs batch-size-independent bits (eval-mode inference) passes ws = NULL.  Same operators as above (unet.py:11,14). */
int64_t gsd_conv3x3_w43_workspace(int N, int H, int W, int Cin, int Cout);
int gsd_conv3x3_w43_ws(const gsd_src* src, int nsrc, const float* wt, int Cin, int Cout, const gsd_dst* dst, int ndst,
                       float* partials, float* ws, int64_t ws_elems, int N, int H, int W, void* stream);
int gsd_conv3x3_w43_dgrad_bnrelu_ws(const gsd_src* src, const float* wt, int Cin, int Cout, const gsd_dst* dst,
                                    const float* raw, const float* scale, const float* shift, const float* mean,
                                    const float* invstd, float* partials, float* ws, int64_t ws_elems, int N, int H, int W,
                                    void* stream);

/* The same two operators with the TWO-dimensional Winograd identity F(2x4, 3x3): F(4,3) along the rows combined with F(2,3)
 * down the columns -- 24 products per 2x4 outputs and input channel, a third of the direct form's and two thirds of the
 * row-only form's MFMA work; same fp32 storage and accumulation.  Weights from gsd_weight_layout modes 8 (forward) / 9 (dX):
 * [m-block of 64][k row = ci*24 + fr*6 + fc][64], U = G2 g G4^T.  Needs Cin % 4 == 0 and a first source segment of a multiple
 * of 4 channels (gsd_conv3x3_w2d_supported); no row folding (an eval-mode forward in this form gives image i of a batch the bits
 * the image alone gets).  Partial-row layout as gsd_conv3x3, its own row count (two rows per pixel tile).
 * K slabs (the _ws entries, as gsd_conv3x3_w43_ws): with scratch lent by the caller a launch whose tile grid leaves most of the
 * chip idle is cut along the input channels, the slabs summed in a fixed order by a second kernel that also runs the epilogue
 * (run-to-run bitwise; not bit-equal to the unsplit launch).  gsd_conv3x3_w2d_workspace: the floats such a launch wants (0: it runs
 * unsplit); any capacity is safe -- the launcher shrinks the slab count to what fits.
 * Planes: every source plane H * w_stride + 4 < 2^30 floats and every destination plane < 2^31 floats, else GSD_ERR_UNSUPPORTED;
 * planes and images may lie any distance apart. */
int gsd_conv3x3_w2d_supported(int Cin, int C0);
int gsd_conv3x3_prefers_w2d(int N, int H, int W, int Cin, int Cout, int train);   /* 1: run this Winograd launch in the 2-D form */
double gsd_conv3x3_w2d_estimate_us(int N, int H, int W, int Cin, int Cout);          /* the planner's run-time models */
double gsd_conv3x3_w43_estimate_us(int N, int H, int W, int Cin, int Cout, int slabs);
int gsd_conv3x3_w2d_partial_rows(int N, int H, int W, int Cout);
int64_t gsd_conv3x3_w2d_mfma_count(int N, int H, int W, int Cin, int Cout);
/* The deep levels' unsplit launches of source class 1 -- one plain source, rows 16-byte aligned on a pitch of a multiple of 4
 * floats: every dX launch, the "activate once" forwards -- run a band-major flat list of the Winograd tiles instead of a grid of
 * rectangles per image where that takes fewer blocks (gsd_conv3x3_w2d_strips.hip; GSD_W2D_STRIPS = 0 never, 1 wherever the list is
 * admitted, unset: where the run-time model has the shorter list finish sooner): same outputs and the same partial rows bit for bit (a launch
 * with partial rows leaves per-tile sums in the workspace of the _ws entries -- gsd_conv3x3_w2d_strips_scratch floats -- and a second
 * kernel adds them in the rectangles' rows and order; without that much workspace it keeps the rectangles).
 * _mfma_count_class: the MFMAs such a launch issues; _strips_plan / _strips_tile: the listing itself, for tests (out: 7 / 5 ints). */
int gsd_conv3x3_w2d_source_class(const gsd_src* src, int nsrc);
int64_t gsd_conv3x3_w2d_strips_scratch(int N, int H, int W, int Cin, int Cout);
int64_t gsd_conv3x3_w2d_mfma_count_class(int N, int H, int W, int Cin, int Cout, int source_class, int with_workspace);
int gsd_conv3x3_w2d_strips_plan(int N, int H, int W, int Cin, int Cout, int* out);
int gsd_conv3x3_w2d_strips_tile(int N, int H, int W, int t, int* out);
int gsd_conv3x3_w2d(const gsd_src* src, int nsrc, const float* wt, int Cin, int Cout,
                    const gsd_dst* dst, int ndst, float* partials, int N, int H, int W, void* stream);
int gsd_conv3x3_w2d_dgrad_bnrelu(const gsd_src* src, const float* wt, int Cin, int Cout, const gsd_dst* dst,
                                 const float* raw, const float* scale, const float* shift, const float* mean,
                                 const float* invstd, float* partials, int N, int H, int W, void* stream);
double gsd_conv3x3_w2d_estimate_slabs_us(int N, int H, int W, int Cin, int Cout);    /* ... with the K-slab form where it pays */
int64_t gsd_conv3x3_w2d_workspace(int N, int H, int W, int Cin, int Cout);
int gsd_conv3x3_w2d_ws(const gsd_src* src, int nsrc, const float* wt, int Cin, int Cout, const gsd_dst* dst, int ndst,
                       float* partials, float* workspace, int64_t workspace_elems, int N, int H, int W, void* stream);
int gsd_conv3x3_w2d_dgrad_bnrelu_ws(const gsd_src* src, const float* wt, int Cin, int Cout, const gsd_dst* dst,
                                    const float* raw, const float* scale, const float* shift, const float* mean,
                                    const float* invstd, float* partials, float* workspace, int64_t workspace_elems,
                                    int N, int H, int W, void* stream);

/* ConvTranspose2d(k=2,s=2)+bias. Replaces aten::convolution(transposed) at unet.py:36,41.
 * src is the (h,w) input (deferred BN allowed), dst the (2h,2w) output (a row pitch is allowed, an even one). weights: mode 6.
 * The forward and dX run on LDS-DMA kernels; dX falls back to a register-staged kernel (weights: mode 3) for an odd-width
 * gradient without slack and under GSD_CONVT_DG_DMA=0.  Every entry point below validates its operands the same way: dy is
 * the plain (Cout,2H,2W) gradient, 8-byte aligned with even strides. */
int gsd_convT2x2(const gsd_src* src, const float* wt, const float* bias, int Cin, int Cout,
                 const gsd_dst* dst, int N, int H, int W, void* stream);
/* dX of the above: src = gradient w.r.t. the (2h,2w) output (plain), dst (h,w).  weights: the gsd_weight_layout mode that
 * gsd_convT2x2_dgrad_layout returns for the same arguments -- 7 (LDS-DMA kernel; an odd-width plane needs src->slack >= 2:
 * its last pixel pair reads two floats past the end of a row) or 3 (register-staged kernel). */
int gsd_convT2x2_dgrad_layout(const gsd_src* src, int Cin, int Cout, int N, int H, int W);
int gsd_convT2x2_dgrad(const gsd_src* src, const float* wt, int Cin, int Cout,
                       const gsd_dst* dst, int N, int H, int W, void* stream);
/* The same with the layout mode of `wt` (3 or 7) STATED by the caller instead of re-derived at launch: a caller that lays its
 * weights out once per buffer shape cannot be handed the other kernel by GSD_CONVT_DG_DMA or a different `slack` at launch
 * time; a mode the arguments do not admit is refused with GSD_ERR_BAD_ARG. */
int gsd_convT2x2_dgrad_as(int wt_mode, const gsd_src* src, const float* wt, int Cin, int Cout,
                          const gsd_dst* dst, int N, int H, int W, void* stream);
/* dX of the transposed convolution fused with the backward of the relu(bn(raw)) that produced its INPUT (unet.py:41 reads the
 * output of the DoubleConv below, unet.py:12-16): dst receives dz = dx * [raw*scale+shift > 0] and `partials` the per-channel
 * (sum dz, sum dz*xhat) as rows of 2*round_up(Cin,64) floats -- the layout gsd_conv3x3_dgrad_bnrelu leaves, for
 * gsd_bn_reduce_partials / gsd_bn_bwd_reduce_finalize -- so gsd_bn_bwd_reduce(mode 0) over that unit disappears.  `raw` has dst's
 * strides; wt: layout mode 7 (the LDS-DMA kernel only).  gsd_convT2x2_dgrad_bnrelu_partial_rows: the row count, 0 when the
 * arguments do not admit the kernel (odd W without src->slack >= 2); it does not read the environment. */
int gsd_convT2x2_dgrad_bnrelu_partial_rows(const gsd_src* src, int Cin, int Cout, int N, int H, int W);
int gsd_convT2x2_dgrad_bnrelu(const gsd_src* src, const float* wt, int Cin, int Cout, const gsd_dst* dst, const float* raw,
                              const float* scale, const float* shift, const float* mean, const float* invstd,
                              float* partials, int N, int H, int W, void* stream);

/* dW of conv3x3: dW[co][ci][kh][kw] = sum_{n,h,w} dy[n,co,h,w] * a[n,ci,h+kh-1,w+kw-1].
 * `a` is given as up to two segments with deferred BN (recomputed on load), `dy` plain.
 * Deterministic split-K: partial slabs in `workspace` (gsd_conv3x3_wgrad_workspace elements),
 * then an ordered reduction writes dW in the reference's (Co,Ci,3,3) layout.
 * The library picks the arithmetic form per shape (direct taps, or the transposed Winograd F(4,3) identity
 * dg = G^T[(A dy).(B^T d)] along rows for Cin, Cout >= 16: half the MFMA work, fp32 throughout; GSD_WGRAD_ALGO=0|1
 * forces one); the workspace query covers either. */
int64_t gsd_conv3x3_wgrad_workspace(int N, int H, int W, int Cin, int Cout);
int gsd_conv3x3_wgrad(const gsd_src* a, int nsrc, const gsd_src* dy, int Cin, int Cout,
                      float* dw, float* workspace, int64_t workspace_elems,
                      int N, int H, int W, void* stream);
/* Which arithmetic form gsd_conv3x3_wgrad takes for exactly these operands: 0 direct taps, 1 Winograd F(4,3) along rows,
 * 2 the two-dimensional F(2x4,3x3) form dg = G2^T[(A2 dY A4^T).(B2^T d B4)]G4 (a third of the direct form's MFMA work; it needs
 * Cout % 128 == 0 or Cout == 64, Cin a multiple of its 32/64-channel block, a dy with 16-byte aligned rows (w_stride % 4 == 0,
 * pad columns 0) and slack >= 4 around every activation segment; GSD_WGRAD_W2D=0 switches it off).  Reads no device memory.
 * gsd_conv3x3_wgrad_mfma_count: v_mfma_f32_16x16x4_f32 instructions that form executes (tile padding included). */
int gsd_conv3x3_wgrad_form(const gsd_src* a, int nsrc, const gsd_src* dy, int Cin, int Cout, int N, int H, int W);
int64_t gsd_conv3x3_wgrad_mfma_count(int form, int N, int H, int W, int Cin, int Cout);
/* 1 when gsd_conv3x3_wgrad serves this shape with a kernel that takes a pitched dy (dy->w_stride > W, see gsd_src). */
int gsd_conv3x3_wgrad_takes_pitched_dy(int N, int H, int W, int Cin, int Cout);
/* 1 when it serves this shape with a kernel that takes pitched ACTIVATION segments (a[i].w_stride > W): the Winograd forms. */
int gsd_conv3x3_wgrad_takes_pitched_act(int N, int H, int W, int Cin, int Cout);
/* dW of a conv3x3 with FEW input channels (Cin * 9 <= 32: the network's first layer, unet.py:15) with the BatchNorm
 * backward of its output applied on the fly: d_raw = scale * (dz - c1 - (raw - mean) * invstd * c2) is formed in registers
 * from dz and raw -- what gsd_bn_bwd_apply would have written.  The first layer has no dX, so dW is d_raw's only reader and
 * the apply pass disappears.  With scale == raw == NULL dz is taken as the conv output's gradient as it is.
 * `a`: ONE plain segment (no deferred BN: the input image); dz, raw: contiguous (N,Cout,H,W).  Deterministic (slabs in
 * `workspace`, ordered reduction); dW in the reference's (Co,Ci,3,3) layout.
 * gsd_conv3x3_wgrad_bn_supported: 1 when the shape is served (0: use gsd_bn_bwd_apply + gsd_conv3x3_wgrad). */
int gsd_conv3x3_wgrad_bn_supported(int N, int H, int W, int Cin, int Cout);
int64_t gsd_conv3x3_wgrad_bn_workspace(int N, int H, int W, int Cin, int Cout);
int gsd_conv3x3_wgrad_bn(const gsd_src* a, const float* dz, const float* raw, const float* scale,
                         const float* mean, const float* invstd, const float* c1, const float* c2,
                         int Cin, int Cout, float* dw, float* workspace, int64_t workspace_elems,
                         int N, int H, int W, void* stream);
/* dX of the same few-input-channel conv3x3 (Cin * 9 <= 32: the network's first layer) with the same BatchNorm backward applied
 * on the fly: dx = conv3x3_dX(d_raw, w), d_raw = scale * (dz - c1 - (raw - mean) * invstd * c2) formed in registers exactly as
 * gsd_conv3x3_wgrad_bn forms it (scale == raw == NULL: dz is the conv output's gradient as it is).  dz, raw: contiguous
 * (N,Cout,H,W); w: the reference's (Cout,Cin,3,3) weights, no layout pass; dx: contiguous (N,Cin,H,W), every element written.
 * Deterministic (no atomics), no workspace.  Replaces the dX half of aten::convolution_backward at unet.py:11 for `inc` plus the
 * apply half of aten::native_batch_norm_backward -- the gradient with respect to the network's input.
 * gsd_conv3x3_dgrad_bn_supported: 1 when the shape is served (Cin * 9 <= 32, 1 <= Cout <= 65535). */
int gsd_conv3x3_dgrad_bn_supported(int N, int H, int W, int Cin, int Cout);
int gsd_conv3x3_dgrad_bn(const float* dz, const float* raw, const float* scale, const float* mean,
                         const float* invstd, const float* c1, const float* c2, const float* w,
                         int Cin, int Cout, float* dx, int N, int H, int W, void* stream);
/* dW and db of ConvTranspose2d(k2,s2): x (h,w) with deferred BN, dy (2h,2w) plain;
 * dW in the reference's (Ci,Co,2,2) layout.  x and dy may have any n_stride / c_stride (64-bit; 8-byte aligned, even, for dy) as
 * long as dbias == NULL: the bias gradient sums dy as ONE dense (N,Cout,2H,2W) array, and a call that asks for it with a
 * dy that is not dense is refused (GSD_ERR_UNSUPPORTED, "bias gradient needs a contiguous dy") before anything is launched. */
int64_t gsd_convT2x2_wgrad_workspace(int N, int H, int W, int Cin, int Cout);
int gsd_convT2x2_wgrad(const gsd_src* x, const gsd_src* dy, int Cin, int Cout,
                       float* dw, float* dbias, float* workspace, int64_t workspace_elems,
                       int N, int H, int W, void* stream);

/* ---- BatchNorm2d (unet.py:12,15; aten::native_batch_norm / _backward) ---------------------- */
/* Reduce conv partials -> sums[0..2*C) (fp64: sum, sum of squares), two ordered stages. Separate from
 * finalize so a data-parallel run can all-reduce sums[0..2C) (SyncBN) in between.
 * `sums` must hold 65*2*C doubles: the result followed by 64*2*C doubles of stage-1 scratch. */
int gsd_bn_reduce_partials(const float* partials, int rows, int Mpad, int C, double* sums, void* stream);
/* Per-channel sums (fp32) of what a conv launch STORED, channels [c_begin, c_begin+c_count): the first halves of its partial
 * rows summed in fp64 in the same two ordered stages.  The ConvT bias gradient (aten::convolution_backward of unet.py:36,41)
 * comes out of the statistics epilogue of the dX launch that writes the up-sampled tensor's gradient this way, without a
 * second pass over it.  `sums`: 65*2*C doubles of scratch (sums[0..C) receives all C channel sums). */
int gsd_partials_channel_sums(const float* partials, int rows, int Mpad, int C, int c_begin, int c_count, float* out,
                              double* sums, void* stream);
/* *counters[i] += delta for n int64 device counters (host array of device pointers): BatchNorm2d.num_batches_tracked of
 * every layer of a train-mode forward (aten::native_batch_norm's `num_batches_tracked += 1`, unet.py:12,15), one launch. */
int gsd_add_counters(int64_t* const* counters, int n, int64_t delta, void* stream);
/* sums -> mean, invstd, (scale, shift) = (gamma*invstd, beta - mean*scale); updates running stats
 * (momentum 0.1, unbiased variance) when running_mean != NULL and the batch statistics are finite.
 * count = N*H*W (global if synced). guard may be NULL. */
int gsd_bn_finalize(const double* sums, int C, double count, const float* gamma, const float* beta,
                    float eps, float momentum, float* running_mean, float* running_var,
                    float* mean, float* invstd, float* scale, float* shift, const gsd_guard* guard, void* stream);
/* eval mode: (scale, shift) from running stats. */
int gsd_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, float eps, int C, float* scale, float* shift, void* stream);

/* eval mode with a backward to follow: gsd_bn_eval_coeffs's (scale, shift) -- the same fp32 expressions, so the same bits --
 * plus mean = running_mean and invstd = 1 / sqrt(running_var + eps), the statistics the backward kernels normalise with. */
int gsd_bn_eval_coeffs_bwd(const float* gamma, const float* beta, const float* running_mean,
                           const float* running_var, float eps, int C, float* scale, float* shift,
                           float* mean, float* invstd, void* stream);

/* Backward of relu(bn(raw)), pass 1.  dz = da * [raw*scale+shift > 0]; writes dz and per-block
 * partials of (sum dz, sum dz*xhat) [+ sum dout*a for mode OUTC].
 *   mode 0 PLAIN: da given by `da` (gsd_src, plain).
 *   mode 1 POOL : da = da (may be NULL ptr => 0) + max-pool routed `dpool` (N,C,H/2,W/2):
 *                 the 2x2 arg-max is recomputed from raw (first maximum wins, like aten).
 *   mode 2 OUTC : da[c] = sum_k dout[k]*wout[k][c]   (1x1 output conv unet.py:54, n_classes K <= 8), extra
 *                 partial dWout[0][c] = sum dout[0]*a[c]  (a = relu(bn(raw))): all of dWout for K == 1; for K > 1 see
 *                 gsd_conv1x1_out_wgrad.
 * partial layout: [rows][3*C] (third block only meaningful in mode 2), rows from
 * gsd_bn_bwd_partial_rows. */
int gsd_bn_bwd_partial_rows(int N, int C, int H, int W);
int gsd_bn_bwd_reduce(int mode, const float* raw, const float* scale, const float* shift,
                      const float* mean, const float* invstd,
                      const gsd_src* da, const float* dpool, const float* dout, const float* wout,
                      int K, float* dz, float* partials, int N, int C, int H, int W, void* stream);
/* pass 2: reduce partials -> sums[0..3*C) (fp64; exposed for the SyncBN all-reduce), then
 * dgamma, dbeta (+ dWout), and the coefficient vectors c1 = sum_dz/n, c2 = sum_dz_xhat/n.
 * `sums` must hold 65*3*C doubles (result + stage-1 scratch). dwout may be NULL.
 * finalize: dgamma/dbeta/dwout come from sums_local (this rank's batch: data-parallel averaging of
 * parameter gradients happens later), c1/c2 from sums_global/count (sums_global == NULL: local). */
int gsd_bn_bwd_reduce_partials(const float* partials, int rows, int C, double* sums, void* stream);
int gsd_bn_bwd_finalize(const double* sums_local, const double* sums_global, int C, double count,
                        float* dgamma, float* dbeta, float* dwout, float* c1, float* c2, void* stream);

/* One-launch forms of (gsd_bn_reduce_partials + gsd_bn_finalize) and (gsd_bn_[bwd_]reduce_partials +
 * gsd_bn_bwd_finalize) for launches that leave only a few hundred partial rows (the persistent bf16 kernels; no SyncBN
 * exchange in between).  `sums` (3*C doubles) still receives the totals.  layout_mpad: 0 for rows of 3*C floats from
 * the stand-alone backward reduce kernels, mpad for rows of 2*mpad floats from a dX epilogue. */
int gsd_bn_reduce_finalize(const float* partials, int rows, int Mpad, int C, double* sums, double count, const float* gamma,
                           const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                           float* mean, float* invstd, float* scale, float* shift, const gsd_guard* guard, void* stream);
int gsd_bn_bwd_reduce_finalize(const float* partials, int rows, int layout_mpad, int C, double* sums, double count,
                               float* dgamma, float* dbeta, float* dwout, float* c1, float* c2, void* stream);
/* pass 3: d_raw = scale_g * (dz - c1 - xhat*c2); scale_g = gamma*invstd = scale.
 * out == NULL: in place on dz.  Otherwise the result goes to `out`, an (N,C,H,out_w_stride) buffer whose rows are
 * PITCHED (out_w_stride >= W, a multiple of 4 floats, base 16-byte aligned; columns W.. are written 0) and dz is left
 * as it is: the dW / dX kernels that read d_raw next move a pitched operand as aligned 16-byte pieces. */
int gsd_bn_bwd_apply(float* dz, const float* raw, const float* scale, const float* mean,
                     const float* invstd, const float* c1, const float* c2,
                     int N, int C, int H, int W, float* out, int out_w_stride, void* stream);
/* relu(bn(raw)) written ONCE: dst = max(0, fma(raw, scale, shift)) -- the single-rounded expression every deferred consumer
 * applies on load, so a consumer of dst as a plain source gets the bits it computes itself from src.  src: a deferred segment
 * (scale, shift, relu) with dense rows; dst: the same (C,H,W) with PITCHED rows (16-byte aligned base, w_stride / c_stride /
 * n_stride multiples of 4 floats; a channel-offset view of a larger buffer is fine).  Columns W .. w_stride-1 are written 0 on
 * every call.  A conv3x3 in the two-dimensional form then reads dst as aligned 16-byte pieces (the launch class of the dX convs).
 * gsd_act_once_pays: the host model's answer for an (N,Cin,H,W) tensor and its train-mode conv3x3 consumer Cin -> Cout that reads
 * it at pad offset (off_h, off_w): 1 when the consumer's modelled saving exceeds the pass (bytes / copy rate + launch); 0 also
 * when the consumer is not the two-dimensional form, the offset is not (0,0) or the tile's halo does not admit aligned pieces.
 * pass_kind: 0 a pass of its own (read + write + launch), 1 written on the way by a kernel that reads the tensor anyway (the skip
 * tensor from gsd_maxpool2_pitched), 2 the producer writes pitched rows instead of dense ones (the pooled tensor: no cost). */
int gsd_bnrelu_pitched(const gsd_src* src, const gsd_dst* dst, int N, void* stream);
int gsd_act_once_pays(int N, int H, int W, int Cact, int Cin, int Cout, int off_h, int off_w, int pass_kind);
/* out[k] = sum over n, p of x[n][k][p] (contiguous [N][K][HW]); deterministic two-stage.
 * workspace >= 64*K floats. Used for dbias of the output conv / transposed conv. */
int gsd_sum_planes(const float* x, int N, int K, int64_t HW, float* out, float* workspace, void* stream);

/* ---- MaxPool2d(2) floor mode (unet.py:26; aten::max_pool2d_with_indices) -------------------- */
/* y = maxpool(max(0, raw*scale+shift)) materialised at (H/2, W/2). No index tensor is kept. */
int gsd_maxpool2(const gsd_src* src, float* y, int N, int C, int H, int W, void* stream);
/* The same pool with PITCHED outputs: `pooled` (C,H/2,W/2) and, when `act` is not NULL, the activated full-resolution tensor
 * max(0, raw*scale+shift) itself (C,H,W) -- the decoder's skip tensor, one extra write and no extra read.  Both destinations:
 * 16-byte aligned base, w_stride / c_stride / n_stride multiples of 4 floats (channel-offset views of a larger buffer are fine);
 * columns W.. of every row are written 0 on every call.  pooled holds the bits gsd_maxpool2 writes, act the bits
 * gsd_bnrelu_pitched writes.  src: the full tensor, dense rows. */
int gsd_maxpool2_pitched(const gsd_src* src, const gsd_dst* pooled, const gsd_dst* act, int N, void* stream);

/* ---- output conv + loss (unet.py:54; train_unet.py:51-52) ----------------------------------- */
/* out[n,k,p] = b[k] + sum_c w[k][c] * max(0, raw[c]*scale[c]+shift[c]). */
int gsd_conv1x1_out(const gsd_src* src, const float* w, const float* b, int C, int K,
                    float* out, int N, int H, int W, void* stream);
/* dW of the output conv for n_classes K > 1 (1 <= K <= 8; for K == 1 it is the third sum of gsd_bn_bwd_reduce mode 2):
 * dw[k][c] = sum_{n,p} dout[n,k,p] * max(0, raw[n,c,p]*scale[c]+shift[c])  (aten::convolution_backward of unet.py:54).
 * raw: dense (N,C,H,W); partials: gsd_conv1x1_out_wgrad_rows(N,H,W) * K*C floats; sums: 65*K*C doubles of scratch. */
int gsd_conv1x1_out_wgrad_rows(int N, int H, int W);
int gsd_conv1x1_out_wgrad(const float* raw, const float* scale, const float* shift, const float* dout, int C, int K,
                          float* dw, float* partials, double* sums, int N, int H, int W, void* stream);
/* loss = mean((o-t)^2) (kind 0) or mean(|o-t|) (kind 1); grad = d loss/d o * grad_scale.
 * loss_out: 1 float (device). workspace >= 2048 floats. grad and guard may be NULL. */
int gsd_loss_fwd_bwd(int kind, const float* o, const float* t, int64_t numel, float grad_scale,
                     float* loss_out, float* grad, float* workspace, const gsd_guard* guard, void* stream);

/* ---- depth-aware loss (an addition: the reference trains on the plain MSE above) ------------- */
/* o, t: dense fp32 (N, K, H, W).  e = o - t in fp32, M = N*K*H*W.
 *   L_data = (1/M) sum w * rho(e)     rho = e^2 (data_kind 0) | |e| (1) | huber (2): e^2/2 for |e| <= huber_delta, else
 *                                     huber_delta * (|e| - huber_delta/2)
 *                                     w = 1 + contact_weight * [ |t - background| > contact_eps ]   (both tests in fp32)
 *   L_grad = sum_{k < grad_scales} (1/M_k) sum_{h mod s = 0, w mod s = 0} ( phi(e[h,w+s] - e[h,w]) [w+s < W]
 *                                                                         + phi(e[h+s,w] - e[h,w]) [h+s < H] )
 *            s = 2^k, M_k = N*K*ceil(H/s)*ceil(W/s), phi = |g| (grad_kind 0) | g^2 (1), differences in fp32; no wrap-around,
 *            no padding, nothing across images or classes
 *   L      = L_data + grad_weight * L_grad
 * The normalisers are element counts, never sum(w): the loss of a batch is the mean of the losses of its equal shards.
 * terms (6 device floats) = L, L_data, L_grad, mean e^2, mean |e|, the fraction of contact pixels.
 * grad (may be NULL: evaluation) = dL/do * grad_scale, each element the sum of the derivatives of the pairs it is an end of
 * (gather form, no atomics), sign(0) = 0, huber' = clamp(e, -huber_delta, huber_delta); fp32, within 2^-19 of the sum of the
 * magnitudes of its at most 17 summands.
 * guard (may be NULL): a non-finite L stores the tick, as gsd_loss_fwd_bwd does.
 * Two stages, no floating-point atomics: per-block fp64 partial sums (w*rho, the slope term, e^2, |e|, contact count), then
 * one wave adds them in a fixed order; the block count depends on the shape alone, so the terms are bitwise reproducible
 * and the same bits with and without grad.  workspace: gsd_depth_loss_workspace doubles, 8-byte aligned.
 * GSD_ERR_BAD_ARG (null pointer, a dimension <= 0, an unknown kind, grad_scales outside 0..4, a non-zero reserved word, a
 * negative or non-finite contact_weight / grad_weight / contact_eps / huber_delta, huber_delta == 0 for huber, a non-finite
 * background, a guard without words or tick) and GSD_ERR_WORKSPACE (workspace_elems too small) are returned before any launch. */
typedef struct gsd_depth_loss {
  int32_t data_kind;     /* 0 mse, 1 l1, 2 huber */
  int32_t grad_kind;     /* 0 l1, 1 l2 */
  int32_t grad_scales;   /* 0..4 */
  int32_t reserved;      /* 0 */
  float huber_delta;     /* read for data_kind 2 only */
  float contact_weight;
  float contact_eps;
  float background;
  float grad_weight;
} gsd_depth_loss;
int64_t gsd_depth_loss_workspace(int N, int K, int H, int W);
int gsd_depth_loss_fwd_bwd(const gsd_depth_loss* spec, const float* o, const float* t, int N, int K, int H, int W,
                           float grad_scale, float* terms, float* grad, double* workspace, int64_t workspace_elems,
                           const gsd_guard* guard, void* stream);

/* ---- per-image depth metrics (an addition: the reference reports one mean loss per pass) ---- */
/* o, t: dense fp32 (N, K, H, W), never written.  e = o - t in fp32.  The kernel works in the network's units only (a
 * conversion to physical units is one factor on the host), so every decision is an fp32 comparison.  Row n of `table`
 * (N x GSD_DM_COLS doubles) describes image n alone, over its K*H*W elements:
 *    0  sum e                    1  sum |e|                  2  sum e^2                3  max |e|
 *    4  n_t: elements with the target in contact, |t - background| > contact_eps (gsd_depth_loss's test, in fp32)
 *    5  n_p: the same test on o  6  n_tp: both
 *    7  sum |e| over target-contact elements                 8  sum e^2 over target-contact elements
 *    9  max |t - background|     10 max |o - background|     (the fp32 differences: peak indentation)
 *    11 sum over existing pairs of |e[h,w+1] - e[h,w]| + |e[h+1,w] - e[h,w]|, differences in fp32, inside one (image, class)
 *       plane, no wrap-around, no padding: scale 0 of gsd_depth_loss's slope term, not normalised
 *    12 number of elements whose e is not finite             13..15  0
 * Sums are fp64 of exact summands (|e|, e^2 formed in fp64 from the fp32 e), counts exact, maxima exact fp32 values; a NaN
 * never wins a maximum (v > m ? v : m, from m = 0), a non-finite e makes the sums of its own image non-finite and is counted
 * in column 12; no other row is affected.
 * Two stages, no floating-point atomics: blocks of one image each write a partial row, then one wave per image adds its
 * image's partial rows in a fixed order.  The number of blocks per image depends on K*H*W alone, so a row is bitwise
 * reproducible and does not depend on N or on the image's position in the batch.
 * workspace: gsd_depth_metrics_workspace doubles, 8-byte aligned (as table).  GSD_ERR_BAD_ARG (null pointer, a dimension <= 0,
 * a non-zero reserved word, a negative or non-finite contact_eps, a non-finite background) and GSD_ERR_WORKSPACE
 * (workspace_elems too small) are returned before any launch; GSD_ERR_UNSUPPORTED for more than 2^23 blocks (N above 131072). */
struct gsd_depth_metrics {
  float background;    /* value of the undeformed gel in the network's units (0 under min_max_to_0_-1) */
  float contact_eps;   /* a pixel v is "contact" when |v - background| > contact_eps, tested in fp32: DepthLoss's test */
  int32_t reserved[2]; /* 0 */
};   /* no typedef: the function below bears the same name (as stat does), so the type is written `struct gsd_depth_metrics` */
#define GSD_DM_COLS 16
int64_t gsd_depth_metrics_workspace(int N, int K, int H, int W);            /* doubles */
int gsd_depth_metrics(const struct gsd_depth_metrics* spec, const float* o, const float* t, int N, int K, int H, int W,
                      double* table /* N x GSD_DM_COLS */, double* workspace, int64_t workspace_elems, void* stream);

/* ---- ground-truth depth images from a mesh (gelslim_depth/mesh_utils/depth_from_mesh.py, restated exactly) ---- */
/* The label maker: for every pixel of either finger, the outermost surface of a rigid triangle mesh under an in-hand pose
 * (DESIGN.md section 16 has the definition; gsd_mesh_depth.hip the kernels).  Everything that depends on the mesh alone is
 * built once, by plan -> count -> (one host read of the pair total, to allocate the list) -> fill; render then serves any
 * number of poses and never synchronises.  The library allocates nothing.
 *
 * tri: T x 9 floats on the device, per triangle three prepared vertices (a, b, q): a, b the two in-plane coordinates in
 *   ascending axis order, in mm, RELATIVE TO (grid.cx, grid.cy); q the signed perpendicular coordinate in mm.
 * records: T x GSD_MESH_RECORD_FLOATS floats, 16-byte aligned (written by count, read by fill and render).
 * cells: gsd_mesh_depth_workspace(grid) int32 words, 8-byte aligned: words 0..1 the pair total as one int64, then
 *   nx*ny + 1 list starts (exclusive scan of the per-cell counts), then nx*ny fill cursors.
 * list: triangle ids, grouped by cell; `list_elems` must be at least the pair total (fill never writes past it; a shorter
 *   list loses triangles).  The order inside a cell is not deterministic; the rendered image is (max and min).
 * poses: N x 3 floats (t1 [m], t2 [m], theta [rad]); widths: N floats, g = widths[n] + view.width_offset in mm.  A sample whose
 *   g is negative or not finite gets NaN images (the caller, who may hold the widths on the host, refuses it beforehand).
 * out: N x 2 x H x W floats in mm, channel 0 the left finger and 1 the right, swapped when view.lr_flip.
 * workspace: gsd_mesh_depth_render_workspace(N) floats (the pose table).
 * GSD_ERR_BAD_ARG (null pointer, a dimension <= 0, T above 2^24, a grid outside 1..2048 cells per axis or with a non-finite
 * field, a non-zero reserved word, misaligned records / cells) and GSD_ERR_WORKSPACE are returned before any launch. */
typedef struct gsd_mesh_grid {
  float x0, y0;        /* grid origin in the centred in-plane frame, mm                                   */
  float cell, inv_cell;/* side of a square cell in mm, and its reciprocal                                 */
  float cx, cy;        /* the in-plane point the prepared vertices are relative to (the bounding box's centre) */
  int32_t nx, ny;      /* cells per axis, 1..2048                                                         */
  int32_t reserved[2]; /* 0 */
} gsd_mesh_grid;
typedef struct gsd_mesh_view {
  float mpp;             /* mm per pixel: image_height_mm / H                                              */
  float width_offset;    /* added to every grasp width, mm                                                 */
  int32_t swap_axes;     /* 0: the unaligned axis is the lower-numbered in-plane axis, 1: the aligned one is */
  int32_t invert_affine; /* the poses are those of the grasp frame in the mesh frame                       */
  int32_t lr_flip;       /* channel order (right, left)                                                    */
  int32_t reserved;      /* 0 */
} gsd_mesh_view;
#define GSD_MESH_RECORD_FLOATS 12
/* Host only: the grid over the in-plane bounding box bbox = {amin, bmin, amax, bmax} (mm, not centred) with cells of
 * cell_mm, raised where an axis would need more than 2048 cells. */
int gsd_mesh_depth_plan(const double* bbox, double cell_mm, gsd_mesh_grid* grid);
int64_t gsd_mesh_depth_workspace(const gsd_mesh_grid* grid);                 /* int32 words of `cells` */
int gsd_mesh_depth_count(const gsd_mesh_grid* grid, const float* tri, int T, float* records, int32_t* cells, int64_t cells_elems,
                         void* stream);
int gsd_mesh_depth_fill(const gsd_mesh_grid* grid, const float* records, int T, int32_t* cells, int64_t cells_elems, int32_t* list,
                        int64_t list_elems, void* stream);
int64_t gsd_mesh_depth_render_workspace(int N);                              /* floats */
int gsd_mesh_depth_render(const gsd_mesh_grid* grid, const gsd_mesh_view* view, const float* records, int T, const int32_t* cells,
                          const int32_t* list, int64_t list_elems, const float* poses, const float* widths, int N, int H, int W,
                          float* out, float* workspace, int64_t workspace_elems, void* stream);

/* ---- in-hand pose from a depth image: score candidate poses against an observed image ---- */
/* Render-and-compare without the images: for each of B observations and each of its P candidate poses, one row of
 * GSD_POSE_ROW doubles
 *   sum_sq = sum e^2,  sum_abs = sum |e|,  inter = #{R < -c and D < -c},  n_rendered = #{R < -c},  n_observed = #{D < -c}
 * with R the depth gsd_mesh_depth_render stores for that candidate, width and pixel (the same bits), D the observed depth,
 * e = (double)R - (double)D and c = contact_depth >= 0.  The sums run over both channels and over the pixel lattice
 * r = stride/2 + i*stride < H, c = stride/2 + j*stride < W of the full H x W image (mpp = image_height_mm / H: a stride thins
 * the lattice, it does not resample the image).
 * grid, view, records, T, cells, list, list_elems: as for gsd_mesh_depth_render.
 * observed: B x 2 x H x W floats in mm, channels as gsd_mesh_depth_render writes them (view.lr_flip is honoured).
 * candidates: B x P x 3 floats (t1 [m], t2 [m], theta [rad]); widths: B floats, g = widths[b] + view.width_offset.
 * rows: B x P x GSD_POSE_ROW doubles, 8-byte aligned.  A non-finite D on the lattice makes the row's two sums non-finite and is
 *   not contact in the counts; off the lattice it has no effect.  An observation whose g is negative or not finite gets rows of
 *   five NaN.
 * workspace: gsd_mesh_pose_score_workspace(B, P, H, W, stride) doubles, 8-byte aligned (0 for arguments the call refuses).
 * A row depends on its own observation, candidate, stride and image alone -- not on B, P or its position -- and a repeated call
 * gives the same bits: no float atomics; 16 x 16 tiles of lattice points are reduced in fp64 in a fixed order and a second
 * kernel sums a candidate's tiles in a fixed order.  Nothing is allocated, every launch is on `stream`, nothing synchronises.
 * GSD_ERR_BAD_ARG before any launch: a null pointer, B, P, H, W or stride below 1, contact_depth negative or not finite,
 * a workspace that is too small, 2^31 or more blocks (2 * B * P * tiles), and what gsd_mesh_depth_render refuses. */
#define GSD_POSE_ROW 5
int64_t gsd_mesh_pose_score_workspace(int B, int P, int H, int W, int stride);   /* doubles */
int gsd_mesh_pose_score(const gsd_mesh_grid* grid, const gsd_mesh_view* view, const float* records, int T, const int32_t* cells,
                        const int32_t* list, int64_t list_elems, const float* observed, int B, const float* candidates,
                        const float* widths, int P, int H, int W, int stride, float contact_depth, double* rows, double* workspace,
                        int64_t workspace_elems, void* stream);

/* ---- the same for G grasp widths per observation, one render per candidate ---- */
/* For each of B observations, each of its P candidates and each of its G widths one row of GSD_POSE_ROW doubles:
 *   rows[b][p][k] is, in all five entries, THE SAME BITS as the row gsd_mesh_pose_score gives for observation b, candidate p
 *   and the width widths[b][k] -- the five NaN of a refused width (g = widths[b][k] + view.width_offset negative or not
 *   finite) and the non-finite sums of a non-finite D included.  A row therefore does not depend on B, P, G or its position.
 * The width enters a pixel's depth only in its last step, d = -max(0, m - g/2): the kernel finds the surface value m of a
 * lattice point once (the map into the mesh frame, the cell, the walk over its triangles) and forms the G depths, errors and
 * contact predicates from it, reduced in gsd_mesh_pose_score's order.  G widths cost one walk, not G.
 * widths: B x G floats [mm]; rows: B x P x G x GSD_POSE_ROW doubles, 8-byte aligned; every other argument as for
 * gsd_mesh_pose_score.  workspace: gsd_mesh_pose_score_widths_workspace(B, P, G, H, W, stride) doubles, 8-byte aligned (0 for
 * arguments the call refuses).  Nothing is allocated, every launch is on `stream`, nothing synchronises, no float atomics.
 * GSD_ERR_BAD_ARG before any launch: what gsd_mesh_pose_score refuses, G below 1 or above GSD_POSE_WIDTHS_MAX, 2^31 or more
 * rows (B * P * G). */
#define GSD_POSE_WIDTHS_MAX 32
int64_t gsd_mesh_pose_score_widths_workspace(int B, int P, int G, int H, int W, int stride);   /* doubles */
int gsd_mesh_pose_score_widths(const gsd_mesh_grid* grid, const gsd_mesh_view* view, const float* records, int T,
                               const int32_t* cells, const int32_t* list, int64_t list_elems, const float* observed, int B,
                               const float* candidates, const float* widths, int P, int G, int H, int W, int stride,
                               float contact_depth, double* rows, double* workspace, int64_t workspace_elems, void* stream);

/* ---- refinement past the lattice: normal-equation rows and a damped Gauss-Newton step ---- */
/* For one lattice point of one (observation, candidate, channel), in section 16's notation:
 *   winner: among the triangles that cover the point, the one with the largest sg * q, THE LOWEST TRIANGLE ID among equal
 *     values (the order of a cell's list changes from build to build, the ids do not).  m is that largest value and
 *     R = -max(0, m - g/2): the bits of gsd_mesh_depth_render.  No covering triangle: no winner, R = 0.
 *   slope, in fp64 from the winner's record floats (sorted vertices, inv), a = q1 - q0, b = q2 - q0:
 *     qx = (a (y2 - y0) - b (y1 - y0)) inv,   qy = (b (x1 - x0) - a (x2 - x0)) inv;   the clamp of q to the triangle's range is ignored.
 *   point derivatives, in fp64 from the floats of the pixel -> mesh map (cs, sn, pa, pb, da = pa - t1, db = pb - t2), for the
 *     parameters a1 = 1000 t1 [mm], a2 = 1000 t2 [mm], theta [rad]:
 *       invert_affine = 0:  x_a1 = -cs, x_a2 = -sn, y_a1 = sn, y_a2 = -cs, x_th = -sn da + cs db, y_th = -sn db - cs da
 *       invert_affine = 1:  x_a1 = 1,   x_a2 = 0,   y_a1 = 0,  y_a2 = 1,   x_th = -sn pa - cs pb, y_th = cs pa - sn pb
 *   Jacobian: a point is active when R < 0.  There J_k = -sg (qx x_k + qy y_k) for k = a1, a2, theta and J_g = dR/dg = 0.5
 *     (g the width in mm); at an inactive point all four are 0.
 * gsd_mesh_pose_normal: one row of GSD_POSE_NORMAL_ROW doubles per candidate, summed over both channels and gsd_mesh_pose_score's
 * pixel lattice, e = (double)R - (double)D:
 *   [0] sum e^2   [1] #active   [2..5] sum J_k e (a1, a2, theta, g)   [6..15] sum J_j J_k, j <= k, row-major upper triangle
 * Entry 0 is gsd_mesh_pose_score's sum_sq of that candidate, width and stride BIT FOR BIT (the same tiles, tree and order), entry
 * 1 its n_rendered at contact_depth = 0.  widths: B x P floats, ONE PER CANDIDATE (g = widths[b][p] + view.width_offset); a
 * negative or non-finite g gives 16 NaN, a non-finite D on the lattice non-finite sums.  A row depends on its own observation,
 * candidate, width, stride and image alone and repeats bitwise: no float atomics, nothing added in memory.
 * workspace: gsd_mesh_pose_normal_workspace doubles, 8-byte aligned (0 for arguments the call refuses).  Every other argument,
 * and what is refused with GSD_ERR_BAD_ARG before any launch, as for gsd_mesh_pose_score.  Nothing is allocated or synchronised. */
#define GSD_POSE_NORMAL_ROW 16
int64_t gsd_mesh_pose_normal_workspace(int B, int P, int H, int W, int stride);   /* doubles */
int gsd_mesh_pose_normal(const gsd_mesh_grid* grid, const gsd_mesh_view* view, const float* records, int T, const int32_t* cells,
                         const int32_t* list, int64_t list_elems, const float* observed, int B, const float* candidates,
                         const float* widths, int P, int H, int W, int stride, double* rows, double* workspace,
                         int64_t workspace_elems, void* stream);
/* gsd_mesh_depth_render's arguments and workspace; out: N x 2 x 3 x H x W DOUBLES, 8-byte aligned: J_a1, J_a2, J_theta of every
 * pixel of every channel, the terms gsd_mesh_pose_normal sums, for inspection. */
int gsd_mesh_depth_render_jacobian(const gsd_mesh_grid* grid, const gsd_mesh_view* view, const float* records, int T,
                                   const int32_t* cells, const int32_t* list, int64_t list_elems, const float* poses,
                                   const float* widths, int N, int H, int W, double* out, float* workspace, int64_t workspace_elems,
                                   void* stream);
/* One Levenberg-Marquardt bookkeeping step for B independent problems, on the device in fp64, one thread each; nothing is read
 * back.  Per problem the state is pose (3 floats: t1 [m], t2 [m], theta [rad]), width (float, mm), lambda (double), row (its
 * GSD_POSE_NORMAL_ROW doubles), accepted (int32); the trial is trial_pose, trial_width and trial_row, its normal row.
 *   1. accept iff trial_row[0] < row[0] (strict; a NaN never wins): the state and row become the trial's, ++accepted and
 *      lambda = max(lambda * down, lambda_min); otherwise lambda = min(lambda * up, lambda_max).
 *      With `first` != 0 the trial is taken as the state unconditionally, accepted = 0 and lambda is left as it is.
 *   2. solve (A + lambda diag(A)) d = -b, A = row[6..15], b = row[2..5], on the free parameters (bit k of free_mask, order a1,
 *      a2, theta, g; bits 0..2 must be set, bit 3 frees the width) by a Cholesky factorisation in that fixed order.  A pivot
 *      that is <= 0 or not finite, or a solution that is not finite, gives d = 0.  d is clipped per component to max_step
 *      (mm, mm, rad, mm).
 *   3. trial_pose = (float)((double)t + d_a / 1000) for the translations, (float)((double)theta + d_theta); trial_width =
 *      (float)((double)g + d_g): the next trial.  trace[i] = row[0] of the state (the accepted cost, one double per problem),
 *      last_step[4 i + k] = |d_k|.
 * GSD_ERR_BAD_ARG before the launch: a null pointer, B < 1, a free_mask without bits 0..2 or with a bit above 3, a factor outside
 * 0 < down <= 1 <= up, lambda bounds that are negative, unordered or not finite, a max_step that is negative or not finite. */
typedef struct gsd_pose_lm {
  double down, up;                /* factors of lambda after an accepted / a rejected trial */
  double lambda_min, lambda_max;
  double max_step[4];             /* mm, mm, rad, mm */
  int32_t free_mask;              /* bit k: parameter k (a1, a2, theta, g) is free */
  int32_t first;                  /* != 0: the trial initialises the state */
} gsd_pose_lm;
int gsd_mesh_pose_lm_update(const gsd_pose_lm* lm, int B, float* pose, float* width, double* lambda, double* row, float* trial_pose,
                            float* trial_width, const double* trial_row, double* trace, int32_t* accepted, double* last_step,
                            void* stream);

/* ---- contact point clouds and normals from depth images ---- */
/* The inverse of section 16's pixel -> mesh map: every contact pixel of a batch of depth images becomes a 3-D point with a unit
 * normal, in the sensor, the grasp or the object frame, by a stream compaction whose order is part of the contract.
 *   lattice: r = stride/2 + i*stride < H, k = stride/2 + j*stride < W (gsd_mesh_pose_score's).  A lattice pixel is a point iff
 *     its depth d < -contact_depth, compared in fp32 (a NaN is not a point).  Points are ordered by image, then channel as stored,
 *     then r, then k, all ascending.
 *   sensor frame (0): (x, y, z) = (mpp (r - H/2), mpp (k - W/2), d), normal n = (d_x, d_y, -1) / |.|.  d_x (along r) and d_y (along k)
 *     are differences between the IMMEDIATE neighbours in the full image, whatever the stride; a neighbour is usable iff it is
 *     inside the image and itself below -contact_depth: both usable (d+ - d-) / (2 mpp), one usable the one-sided difference
 *     over mpp, none 0.
 *   grasp frame (1): s = +1 for the right finger, -1 for the left (channel 1 is the right one, channel 0 with view.lr_flip);
 *     (u, v, q) = (s x, y, s (g/2 - d)), g = widths[b] + view.width_offset; n = (s d_x, d_y, s) / |.|.
 *   object frame (2): the mesh file's coordinates times pc_scale.  (ta, tb) = (u, v), or (v, u) with view.swap_axes;
 *     (a, b) = M^-1 (ta, tb) with M = [[cos th, -sin th, 1000 t1], [sin th, cos th, 1000 t2]], M itself with view.invert_affine;
 *     a goes to the lower in-plane axis, b to the higher one, q / multiplier + mid to axis perp_ind.  The normal's in-plane pair
 *     goes through the linear part of the same map, its third component is divided by multiplier.
 *   Everything after the fp32 loads is fp64 (contraction off), rounded to fp32 once at the store.
 *   An image whose g is negative or not finite has no points in frames 1 and 2 (frame 0 reads no widths).
 * depth: B x 2 x H x W floats in mm, channels as gsd_mesh_depth_render writes them.  widths: B floats, required for frames 1 and
 * 2; poses: B x 3 floats (t1 [m], t2 [m], theta [rad]), required for frame 2.
 * workspace: gsd_depth_points_workspace(B, H, W, stride) int32 words, 8-byte aligned; 0 for arguments the calls refuse (a
 *   dimension below 1, 2 B H W >= 2^31, 2^31 or more blocks).  Words 0..1 hold the call's total as one int64 once
 *   gsd_depth_points_count has run; the write needs the workspace as the count of the same depth, view, widths and dims left it.
 * gsd_depth_points_count: counts (B x 2 int32) receives the true number of points of every (image, channel), the workspace the
 *   total and the offsets.  Blocks of 1024 lattice points of one (image, channel) count by wave ballots, one block scans the
 *   block counts in as many passes as it takes.
 * gsd_depth_points_write: recomputes the predicate and writes points (rows x 3 floats), normals (rows x 3 floats, may be NULL)
 *   and pixel (rows int32, ((b*2 + ch)*H + r)*W + k, may be NULL).  `rows` is what the three outputs hold; no row at or beyond it
 *   is written.
 *     packed, capacity = 0: point number i of the call goes to row i; the caller sized the outputs from the total.
 *     padded, capacity = M > 0: image b's points, both channels in order, go to rows b*M .. b*M + min(n_b, M) - 1, later points
 *       are dropped, and the rows from min(n_b, M) to M - 1 are written as NaN (pixel: -1); rows must be at least B*M.
 *       `counts` keeps the true numbers, so an overflow stays visible.
 * Nothing is allocated, every launch is on `stream`, nothing synchronises; no float atomics and no atomics for placement, so a
 * repeated call gives the same bits and an image's points do not depend on its batch.
 * GSD_ERR_BAD_ARG before any launch: a null pointer that is required, bad dims, a view with a non-zero reserved word, a frame
 * outside 0..2, mpp not finite and positive, width_offset or mid not finite, contact_depth negative or not finite, perp_ind
 * outside 0..2, multiplier not +-1, a flag that is not 0 or 1, capacity or rows negative, rows below B*capacity or above
 * 2^31 - 1, a misaligned workspace.  GSD_ERR_WORKSPACE: a workspace that is too small. */
typedef struct gsd_depth_points_view {
  double mpp;            /* mm per pixel: image_height_mm / H                                              */
  double width_offset;   /* added to every grasp width, mm                                                 */
  double contact_depth;  /* c >= 0, mm: a pixel is a point iff d < -(float)c                               */
  double mid;            /* what the perpendicular object coordinate is relative to (MeshGrid.mid), mm     */
  int32_t perp_ind;      /* the object axis perpendicular to the image plane, 0..2                         */
  int32_t swap_axes;     /* 0: the unaligned axis is the lower-numbered in-plane axis, 1: the aligned one is */
  int32_t multiplier;    /* +1 or -1: the right finger looks along multiplier * axis perp_ind              */
  int32_t invert_affine; /* the poses are those of the grasp frame in the mesh frame                       */
  int32_t lr_flip;       /* channel order (right, left)                                                    */
  int32_t frame;         /* 0 sensor, 1 grasp, 2 object                                                    */
  int32_t reserved[2];   /* 0 */
} gsd_depth_points_view;
#define GSD_DEPTH_POINTS_BLOCK 1024      /* lattice points per block of the count and write launches */
#define GSD_DEPTH_POINTS_SCAN_PASS 4096  /* block counts per pass of the scan                          */
int64_t gsd_depth_points_workspace(int B, int H, int W, int stride);            /* int32 words */
int gsd_depth_points_count(const gsd_depth_points_view* view, const float* depth, const float* widths, int B, int H, int W, int stride,
                           int32_t* counts, int32_t* workspace, int64_t workspace_elems, void* stream);
int gsd_depth_points_write(const gsd_depth_points_view* view, const float* depth, const float* widths, const float* poses, int B, int H,
                           int W, int stride, int capacity, int64_t rows, float* points, float* normals, int32_t* pixel,
                           int32_t* workspace, int64_t workspace_elems, void* stream);

/* ---- connected contact patches of depth images ---- */
/* Connected-component labelling of the contact mask of a batch of depth images, integer statistics per patch, and a filter that
 * removes the patches that are not kept.  Everything is an integer or a bit copy: one result whatever the schedule.
 *   contact: d < -(float)contact_depth, compared in fp32 (gsd_depth_points' rule): a NaN is not contact, -inf is, -c itself is not.
 *   patch: a maximal 4- or 8-connected set of contact pixels of one (image, channel) plane; planes never connect.
 *   numbering: patches of fewer than min_area pixels are dropped, the rest are numbered 1, 2, ... per plane in raster order of each
 *     patch's first pixel (the smallest r W + k): scipy.ndimage.label's order.
 * depth: B x 2 x H x W floats in mm.  2 B H W must be below 2^31.
 * gsd_contact_patches_workspace(B, H, W): int32 words the label call needs (one per pixel and one per 1024 pixels of a plane), 0
 *   for dims the calls refuse.  What the workspace holds before the call does not matter.
 * gsd_contact_patches_label: labels (B x 2 x H x W int32) receives 0 for background and dropped patches, else the patch number
 *   (numbers above any K included); counts (B x 2 int32) the true number of kept patches per plane.  A union-find over the row
 *   runs of 64-column segments, the parents in `labels` itself; every loop that follows parents is limited to H W steps.
 * gsd_contact_patches_stats: stats (B x 2 x K x 12 int64), row j of a plane for patch number j + 1; rows without a patch are
 *   all zero (the call clears the table first).  Columns: 0 area; 1..4 r_min, r_max, k_min, k_max; 5..9 sum r, sum k, sum r^2,
 *   sum k^2, sum r k; 10 sum dq, dq = (int64) rint((double) max(d, -1024.0f) * 2^20), half to even; 11 the minimum over the patch
 *   of (ord(d) << 32) | (r W + k), ord(d) = ~u if the sign bit of the fp32 bits u is set, else u | 0x80000000: the deepest pixel,
 *   among equals the first in raster order.  Patches numbered above K have no row.  Integer atomics only.
 * gsd_contact_patches_filter: out = depth bit for bit, except +0.0 where a pixel is contact and its patch is not kept.  A patch
 *   is kept when its label is non-zero and, with a keep table (B x 2 x (K + 1) uint8, entry 0 unused), its number is at most K
 *   with a non-zero entry; keep = NULL keeps every numbered patch.  The view supplies contact_depth: a dropped patch has label 0
 *   like the background, so the predicate is evaluated again.  out may be depth itself.
 * Nothing is allocated, every launch is on `stream`, nothing synchronises.  GSD_ERR_BAD_ARG before any launch: a null pointer
 * that is required, bad dims, contact_depth negative or not finite, connectivity other than 4 or 8, min_area below 1, K below 1
 * or a table of 2^31 entries or more.  GSD_ERR_WORKSPACE: a workspace that is too small. */
typedef struct gsd_contact_patches_view {
  double contact_depth;  /* c >= 0, mm: a pixel is contact iff d < -(float)c */
  int32_t connectivity;  /* 4 or 8                                            */
  int32_t min_area;      /* >= 1: patches with fewer pixels are dropped       */
} gsd_contact_patches_view;
#define GSD_CONTACT_PATCHES_SEG 64   /* columns of a row that one wave labels: runs are cut at multiples of it */
#define GSD_CONTACT_PATCHES_COLS 12  /* int64 columns per row of the statistics                                */
int64_t gsd_contact_patches_workspace(int B, int H, int W);                     /* int32 words */
int gsd_contact_patches_label(const gsd_contact_patches_view* view, const float* depth, int B, int H, int W, int32_t* labels,
                              int32_t* counts, int32_t* workspace, int64_t workspace_elems, void* stream);
int gsd_contact_patches_stats(const gsd_contact_patches_view* view, const float* depth, const int32_t* labels, int B, int H, int W, int K,
                              int64_t* stats, void* stream);
int gsd_contact_patches_filter(const gsd_contact_patches_view* view, const float* depth, const int32_t* labels, const uint8_t* keep, int B,
                               int H, int W, int K, float* out, void* stream);

/* ---- closest points on a mesh and rigid registration of point clouds ---- */
/* Exact nearest surface points of a triangle mesh, the normal-equation rows of a point-to-plane or point-to-point fit over SE(3),
 * and the Levenberg-Marquardt bookkeeping of that fit.  Frame: gsd_depth_points' object frame (the mesh file's coordinates times
 * pc_scale, mm).
 *   tri: T x 9 floats on the device, per triangle the vertices a, b, c (x, y, z).  A triangle whose cross product (b - a) x (c - a),
 *     formed in fp64 from two rounded products and one subtraction per component, is exactly (0, 0, 0) is SKIPPED: no cell lists it.
 *   volume: cubic cells over the mesh's bounding box (gsd_mesh_volume_plan, host only).  cells: gsd_mesh_volume_workspace int32
 *     words, 8-byte aligned: words 0..1 the pair total as one int64, then nx*ny*nz + 1 list starts, then nx*ny*nz fill cursors
 *     (cell (ix, iy, iz) has the index (iz*ny + iy)*nx + ix).  list: triangle ids grouped by cell, at least the pair total.  A
 *     triangle is listed in every cell its axis-aligned box touches (the index range is widened, rounding can only add a cell).
 *     plan -> count -> (one host read of the pair total) -> fill, as for gsd_mesh_depth_*.
 *   closest point of p on a triangle: the region method on
 *       d1 = ab.ap, d2 = ac.ap, d3 = ab.bp, d4 = ac.bp, d5 = ab.cp, d6 = ac.cp   (u.v = (ux vx + uy vy) + uz vz, ap = p - a, ...)
 *       vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4, e1 = d4 - d3, e2 = d5 - d6,
 *     the first of: d1 <= 0 and d2 <= 0: a | d3 >= 0 and d4 <= d3: b | vc <= 0, d1 >= 0, d3 <= 0: a + (d1 / (d1 - d3)) ab |
 *       d6 >= 0 and d5 <= d6: c | vb <= 0, d2 >= 0, d6 <= 0: a + (d2 / (d2 - d6)) ac | va <= 0, e1 >= 0, e2 >= 0: b + (e1 / (e1 + e2)) (c - b) |
 *       else (a + (vb / s) ab) + (vc / s) ac with s = (va + vb) + vc;
 *     d^2 = ((px - x)^2 + (py - y)^2) + (pz - z)^2.  All of it in fp64 from the fp32 loads on, no contraction.
 *   winner of p: the triangle with the smallest d^2, THE LOWEST TRIANGLE ID among bit-equal ones; with max_distance D (+inf:
 *     unlimited) it needs d^2 <= D*D.  The result depends on p and the mesh alone: not on the cells, N or p's place.
 * gsd_mesh_closest_points: points N x 3 floats; triangle (N int32), closest (N x 3 floats, (float)x), distance (N floats,
 *   (float)sqrt(d^2)), sq_distance (N doubles, 8-byte aligned).  No winner, or a non-finite coordinate: -1, NaN, +inf, +inf.
 * gsd_mesh_icp_rows: for each of S transforms (12 doubles, a row-major 3 x 4 [R | t]) one row of GSD_ICP_ROW doubles over the N
 *   points p' = R p + t, p'_x = ((R00 px + R01 py) + R02 pz) + t0, kept in fp64; weights (N floats >= 0) may be NULL (1).  A point is
 *   active iff it has a winner within D; one with a non-finite p' adds nothing.
 *     [0] sum_active w d^2 + D^2 sum_inactive w (the second term only for a finite D)   [1] #active   [2] sum_active w r^2
 *     [3..8] sum w J^T r   [9..29] sum w J^T J, upper triangle, row-major; parameters: the left twist (v, omega), dp' = v + omega x p'.
 *     kind 0, point to plane: n = cross / |cross| of the winner, r = n.(p' - x), J = [n, p' x n];
 *     kind 1, point to point: r = p' - x, J = [I, -[p']x].
 *   Blocks of 256 points are summed by a fixed tree, a second launch adds a start's blocks in ascending order: no float atomics, a
 *   row repeats bitwise and does not depend on S or its place.  workspace: gsd_mesh_icp_rows_workspace(N, S) doubles (0 for
 *   arguments the call refuses).
 * gsd_mesh_icp_lm_update: gsd_mesh_pose_lm_update for S starts on six parameters.  State: transforms (S x 12), lambda, row (S x
 *   GSD_ICP_ROW), accepted; trial: trial_transforms, trial_row.
 *   1. accept iff trial_row[0] < row[0] (strict; a NaN never wins), lambda = max(lambda * down, lambda_min), else lambda =
 *      min(lambda * up, lambda_max); `first` != 0 takes the trial unconditionally, accepted = 0, lambda untouched.
 *   2. (A + lambda diag A) xi = -b, A = row[9..29], b = row[3..8], by Cholesky in the order v1 v2 v3 w1 w2 w3; a pivot <= 0 or not
 *      finite, or a non-finite solution, gives xi = 0; xi is clipped per component to max_step (mm x 3, rad x 3).
 *   3. trial_transforms = exp(xi) T of the state: E = I + A K + B K^2, u = (I + B K + C K^2) v, K = [omega]x, th = |omega|,
 *      A = sin th / th, B = (1 - cos th) / th^2, C = (th - sin th) / th^3, below th = 1e-8 their series 1 - th^2/6, 1/2 - th^2/24,
 *      1/6 - th^2/120; R' = E R, t' = E t + u.  trace[i] = row[0] of the state, last_step[6 i + k] = |xi_k|.
 * Nothing is allocated, every launch is on `stream`, nothing synchronises.  GSD_ERR_BAD_ARG before any launch: a null pointer
 * (weights excepted), N, S or T below 1, a max_distance that is negative or NaN, a kind other than 0 or 1, a volume outside 1..1024
 * cells per axis or 2^24 in all or with a non-finite field, a non-zero reserved word, misaligned fp64 arrays or cells, what
 * gsd_mesh_pose_lm_update refuses of its constants.  GSD_ERR_WORKSPACE: a workspace that is too small. */
typedef struct gsd_mesh_volume {
  double x0, y0, z0;     /* grid origin, mm                                                             */
  double x1, y1, z1;     /* x0 + nx * cell, ...: the box that holds every vertex, queries are clamped into it */
  double cell, inv_cell; /* side of a cubic cell in mm, and its reciprocal                              */
  int32_t nx, ny, nz;    /* cells per axis, 1..1024, at most 2^24 in all                                */
  int32_t reserved;      /* 0 */
} gsd_mesh_volume;
typedef struct gsd_icp_lm {
  double down, up;                /* factors of lambda after an accepted / a rejected trial */
  double lambda_min, lambda_max;
  double max_step[6];             /* mm, mm, mm, rad, rad, rad */
  int32_t first;                  /* != 0: the trial initialises the state */
  int32_t reserved;               /* 0 */
} gsd_icp_lm;
#define GSD_ICP_ROW 30
/* Host only: the grid over bbox = {xmin, ymin, zmin, xmax, ymax, zmax} (mm) with cells of cell_mm, enlarged where an axis would
 * need more than 1024 cells or the grid more than 2^24. */
int gsd_mesh_volume_plan(const double* bbox, double cell_mm, gsd_mesh_volume* volume);
int64_t gsd_mesh_volume_workspace(const gsd_mesh_volume* volume);            /* int32 words of `cells` */
int gsd_mesh_volume_count(const gsd_mesh_volume* volume, const float* tri, int T, int32_t* cells, int64_t cells_elems, void* stream);
int gsd_mesh_volume_fill(const gsd_mesh_volume* volume, const float* tri, int T, int32_t* cells, int64_t cells_elems, int32_t* list,
                         int64_t list_elems, void* stream);
int gsd_mesh_closest_points(const gsd_mesh_volume* volume, const float* tri, int T, const int32_t* cells, const int32_t* list,
                            int64_t list_elems, const float* points, int64_t N, double max_distance, int32_t* triangle, float* closest,
                            float* distance, double* sq_distance, void* stream);
int64_t gsd_mesh_icp_rows_workspace(int N, int S);                           /* doubles */
int gsd_mesh_icp_rows(const gsd_mesh_volume* volume, const float* tri, int T, const int32_t* cells, const int32_t* list,
                      int64_t list_elems, const float* points, const float* weights, int N, const double* transforms, int S,
                      double max_distance, int kind, double* rows, double* workspace, int64_t workspace_elems, void* stream);
int gsd_mesh_icp_lm_update(const gsd_icp_lm* lm, int S, double* transforms, double* lambda, double* row, double* trial_transforms,
                           const double* trial_row, double* trace, int32_t* accepted, double* last_step, void* stream);

/* ---- touches fused into a surface: TSDF volume and marching tetrahedra ---- */
/* Many depth images of one object, each with a rigid map object -> grasp frame, are fused into a truncated signed distance volume,
 * and the volume's zero level is extracted as triangles.  Both are gathers in a fixed order without float atomics: a numpy twin
 * holds them bit for bit.  Frame: gsd_depth_points' object frame, mm.
 *   volume: nx x ny x nz voxels, voxel (ix, iy, iz) at origin + voxel * (ix, iy, iz) (fp64, one product and one sum per component),
 *     linear index (iz*ny + iy)*nx + ix.  State: acc = sum w * sample and weight = sum w, nz x ny x nx floats each.
 *   touch k: depth image k (2 x H x W floats, channels as gsd_mesh_depth_render writes them), widths[k], transforms + 12 k (row-major
 *     3 x 4 [A | t], gsd_mesh_icp_rows' layout; rows give u (unaligned), v (aligned), q (perpendicular, right finger at q > 0); A may
 *     be improper and is not checked), weights[k] (weights may be NULL: 1).
 *   one sample (voxel p, touch k, channel ch), fp64 without contraction after the fp32 loads:
 *     s = +1 for the right finger (channel 1, channel 0 with view.lr_flip), -1 for the left
 *     u = ((A00 px + A01 py) + A02 pz) + t0, likewise v, q;   g = (double)widths[k] + view.width_offset; a negative or non-finite g
 *     makes the touch contribute nothing;   mpp = image_height_mm / H, inv_mpp = 1 / mpp (host)
 *     rf = (s u) inv_mpp + H/2, kf = v inv_mpp + W/2, r0 = floor(rf), k0 = floor(kf)
 *     usable: 0 <= r0 <= H - 2 and 0 <= k0 <= W - 2 (compared in fp64) and the pixels d00, d01, d10, d11 (row offset, column offset)
 *       all finite;   a = rf - r0, b = kf - k0, top = d00 + b (d01 - d00), bot = d10 + b (d11 - d10), dbar = top + a (bot - top)
 *     phi = (s q - g/2) + dbar;   contact: all four pixels d < -(float)contact_depth (fp32)
 *     update in fp32, products and sums rounded separately, w = weights[k]:
 *       contact and phi >= -truncation:      acc += w * (float)min(phi * inv_truncation, 1), weight += w
 *       usable, not contact and phi > 0:     acc += wc, weight += wc, wc = w * (float)carve_weight
 *   Per voxel the updates run in touch order, channel 0 before channel 1, onto the stored state: K touches in one call equal any
 *   split of them into consecutive calls, bit for bit.
 * gsd_touch_integrate: one thread per voxel, a block of 256 owns a brick of 16 x 4 x 4 voxels and walks the K touches; state is read
 *   once and stored once.  With view.cull != 0 a block skips a touch whose image rectangle, grown by one pixel, cannot hold any voxel
 *   of the brick's box: a bound, so it never changes a bit.  2 K H W must be below 2^31.
 * field: f = (double)acc / (double)weight; a voxel is observed iff weight > (float)min_weight, inside iff f < 0.
 * surface: a cell (ix, iy, iz), ix < nx - 1, ..., is valid iff its eight corners are observed; it is split into the six Kuhn
 *   tetrahedra around the diagonal (0,0,0)-(1,1,1) (axis permutations in lexicographic order) and each is triangulated by the table
 *   of section 24, normals out of the object.  A vertex on the edge between the voxels lo < hi (linear index):
 *   t = f_lo / (f_lo - f_hi), p = p_lo + (p_hi - p_lo) t per component in fp64, rounded to fp32 at the store: every cell that shares
 *   the edge stores the same bits.  Order: cell index (iz*(ny-1) + iy)*(nx-1) + ix, tetrahedron 0..5, the table's order.
 * gsd_touch_extract_workspace: int32 words of the workspace (8-byte aligned), 0 for a volume the calls refuse.
 * gsd_touch_extract_count: blocks of 256 cells count their triangles, one block scans the block totals (4096 per pass, with a
 *   carry); the total is left as one int64 at the head of the workspace and in *total (device).
 * gsd_touch_extract_write: needs the workspace as the count of the same volume, state and min_weight left it; writes triangles
 *   (rows x 9 floats: a, b, c) and cell (rows int32, may be NULL).  No row at or beyond `rows` is written.
 *     packed, capacity = 0: triangle i goes to row i.
 *     padded, capacity = M > 0: the first min(total, M) triangles, then NaN (cell: -1) up to row M - 1; rows must be at least M.
 * Nothing is allocated, every launch is on `stream`, nothing synchronises.  GSD_ERR_BAD_ARG before any launch: a null pointer
 * (weights and cell excepted), K < 1, H or W < 2, 2 K H W >= 2^31, an axis outside 2..1024, voxel or truncation not finite and
 * positive, a non-finite origin, image height or width offset, a negative or non-finite contact_depth, carve_weight or min_weight, a
 * non-zero reserved word, a negative capacity or rows, rows below capacity or above 2^31 - 1, a misaligned workspace, total or
 * transforms.  GSD_ERR_WORKSPACE: a workspace that is too small. */
typedef struct gsd_touch_volume {
  double x0, y0, z0;      /* position of voxel (0, 0, 0), mm                  */
  double voxel;           /* spacing h, mm                                    */
  double truncation;      /* tau, mm                                          */
  int32_t nx, ny, nz;     /* voxels per axis, 2..1024                         */
  int32_t reserved;       /* 0 */
} gsd_touch_volume;
typedef struct gsd_touch_view {
  double image_height_mm; /* the H rows of an image span this many mm         */
  double width_offset;    /* added to every grasp width, mm                   */
  double contact_depth;   /* c >= 0, mm: a pixel is contact iff d < -(float)c */
  double carve_weight;    /* weight of a free-space sample relative to w      */
  int32_t lr_flip;        /* channel order (right, left)                      */
  int32_t cull;           /* != 0: blocks skip touches that cannot reach them */
  int32_t reserved[2];    /* 0 */
} gsd_touch_view;
#define GSD_TOUCH_EXTRACT_BLOCK 256    /* cells per block of the count and write launches */
#define GSD_TOUCH_EXTRACT_SCAN_PASS 4096 /* block totals per pass of the scan             */
int gsd_touch_integrate(const gsd_touch_volume* volume, const gsd_touch_view* view, const float* depth, const float* widths,
                        const double* transforms, const float* weights, int K, int H, int W, float* acc, float* weight, void* stream);
int64_t gsd_touch_extract_workspace(const gsd_touch_volume* volume);            /* int32 words */
int gsd_touch_extract_count(const gsd_touch_volume* volume, const float* acc, const float* weight, double min_weight, int64_t* total,
                            int32_t* workspace, int64_t workspace_elems, void* stream);
int gsd_touch_extract_write(const gsd_touch_volume* volume, const float* acc, const float* weight, double min_weight, int64_t capacity,
                            int64_t rows, float* triangles, int32_t* cell, int32_t* workspace, int64_t workspace_elems, void* stream);

/* ---- optimiser (train_unet.py:306,375-376) -------------------------------------------------- */
/* Fused torch.optim.Adam(lr, betas, eps, weight_decay: coupled L2) + torch_ema update over a flat
 * parameter arena. step is the 1-based Adam step; ema may be NULL; ema_decay already resolved
 * (min(decay,(1+n)/(10+n))). grad_scale multiplies g first (1/world_size after all-reduce).
 * guard (may be NULL): skip the whole update when words[0] == tick (see gsd_guard). */
int gsd_adam_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t numel,
                 int step, float lr, float beta1, float beta2, float eps, float weight_decay,
                 float ema_decay, float grad_scale, const gsd_guard* guard, void* stream);

/* ---- gradient clipping by global norm (an addition: the reference trains unclipped) --------- */
/* torch.nn.utils.clip_grad_norm_(parameters, max_norm, norm_type=2) over the flat gradient arena, on the device:
 *   S       = sum g[i]^2, accumulated in fp64 (the square of an fp32 value is exact there)
 *   clip[0] = total = (float)(sqrt(S) * (double)grad_scale)   the L2 norm of the averaged gradient, rounded once
 *   clip[1] = coef  = min(1, max_norm / (total + 1e-6f))      in fp32: clip_grad_norm_'s clip_coef_clamped
 * g is left as it is; the coefficient is applied by gsd_adam_ema_clip.  grad_scale is gsd_adam_ema's (1/world_size
 * after the all-reduce).  max_norm = +inf is legal: coef is 1 and the call only measures.
 * A non-finite total is never hidden: coef becomes NaN (not 1), and with a guard `tick` is stored into words[0] as
 * gsd_loss_fwd_bwd does, so gsd_adam_ema_clip skips and counts the step.
 * Two stages, no floating-point atomics: group k of four consecutive floats belongs to thread k mod (blocks * 256),
 * with blocks = gsd_grad_norm_workspace(numel) a function of numel alone, so the result is bitwise reproducible and does
 * not depend on the alignment of g (any 4-byte aligned address; a 16-byte aligned one is read with 16-byte loads).
 * workspace: gsd_grad_norm_workspace(numel) doubles, 8-byte aligned.  clip: two floats on the device.
 * GSD_ERR_BAD_ARG (null pointer, numel <= 0, max_norm <= 0 or NaN, a guard without words or tick) and
 * GSD_ERR_WORKSPACE (workspace_elems too small) are returned before any launch. */
int64_t gsd_grad_norm_workspace(int64_t numel);
int gsd_grad_norm(const float* g, int64_t numel, float grad_scale, float max_norm, float* clip, double* workspace,
                  int64_t workspace_elems, const gsd_guard* guard, void* stream);
/* gsd_adam_ema with the gradient scale grad_scale * clip[1], the product formed in fp32 on the device from
 * gsd_grad_norm's coefficient (clip: its two floats).  Same arithmetic otherwise: with clip[1] == 1.0f the results are
 * gsd_adam_ema's bit for bit.  Same guard behaviour: skip and count when words[0] == tick.  A NaN coefficient without
 * a guard reaches the parameters, as a NaN gradient would. */
int gsd_adam_ema_clip(float* p, const float* g, float* m, float* v, float* ema, int64_t numel,
                      int step, float lr, float beta1, float beta2, float eps, float weight_decay,
                      float ema_decay, float grad_scale, const float* clip, const gsd_guard* guard, void* stream);

/* ---- inference pre/post-processing (test_utils/test_depth_estimation.py:14-20, complete_prediction.py:4-10) ---- */
/* F.interpolate(mode='area') (image_utils.py:12-15; == adaptive_avg_pool2d) fused with the difference image
 * (image_utils.py:6-10, when base != NULL: pre(x) = (x - base + pre_add) * pre_mul) and a per-channel affine
 * (normalize_tactile_image / denormalize_depth_image, normalization_utils.py:4-35,101-129):
 *   out[n,c,oh,ow] = A[min(c,nab-1)] * mean_window(pre(in)) + B[min(c,nab-1)]. */
int gsd_area_resize_affine(const float* in, const float* base, int N, int C, int H, int W, float* out, int OH, int OW,
                           const float* A, const float* B, int nab, float pre_add, float pre_mul, void* stream);

/* F.interpolate(size=(OH, OW), mode=interp_method, align_corners=None, antialias=False) for every 4-D mode the reference's
 * one resampling knob `interp_method` can reach (train_unet.py:18, image_utils.py:12-15).  Indices and weights are those of
 * ATen's CPU kernels in fp32 (gsd_resize.hip states them); nearest modes copy a pixel, bilinear / bicubic are separable.
 * GSD_INTERP_AREA forwards to gsd_area_resize_affine / gsd_ingest_images unchanged. */
typedef enum {
  GSD_INTERP_AREA = 0,
  GSD_INTERP_NEAREST = 1,
  GSD_INTERP_NEAREST_EXACT = 2,
  GSD_INTERP_BILINEAR = 3,
  GSD_INTERP_BICUBIC = 4
} gsd_interp;
/* gsd_area_resize_affine with any gsd_interp mode:
 *   out[n,c,oh,ow] = A[min(c,nab-1)] * resize(pre(in))[n,c,oh,ow] + B[min(c,nab-1)].
 * A mode outside gsd_interp, a null pointer or a non-positive size returns GSD_ERR_BAD_ARG; N, C <= 65535 per call. */
int gsd_resize_affine(int mode, const float* in, const float* base, int N, int C, int H, int W, float* out, int OH, int OW,
                      const float* A, const float* B, int nab, float pre_add, float pre_mul, void* stream);

/* ---- device-resident dataset path (gelslim_depth/datasets/general_dataset.py) ----------------- */
/* Ingest of one object file's images into the dataset arena: finger split (the caller passes the channel view
 * through strides; general_dataset.py:69-72), difference image (image_utils.py:6-10, when base != NULL:
 * pre(x) = (x - base + pre_add) * pre_mul) and F.interpolate(mode='area') (image_utils.py:12-15) in one pass.
 * dtype: 0 = float32, 1 = uint8 source (strides in ELEMENTS). out is contiguous (N,C,OH,OW) float32. */
int gsd_ingest_images(const void* in, const void* base, int dtype, int N, int C, int H, int W, int64_t in_n_stride,
                      int64_t in_c_stride, int64_t base_n_stride, int64_t base_c_stride, float* out, int OH, int OW,
                      float pre_add, float pre_mul, void* stream);
/* gsd_ingest_images with any gsd_interp mode (same arguments after `mode`; general_dataset.py:71-121 with interp_method). */
int gsd_ingest_images_interp(int mode, const void* in, const void* base, int dtype, int N, int C, int H, int W,
                             int64_t in_n_stride, int64_t in_c_stride, int64_t base_n_stride, int64_t base_c_stride, float* out,
                             int OH, int OW, float pre_add, float pre_mul, void* stream);
/* torchvision.transforms.functional.gaussian_blur of `planes` contiguous HxW planes (blur_depth_images, image_utils.py:17-19;
 * general_dataset.py:74-76,84-86 when depth_image_blur_kernel > 1): reflect padding of K/2, then the depthwise correlation
 * with the K x K kernel (device pointer, row-major; the caller builds it as torchvision does -- gelslim_depth_amd/dataset.py).
 * Out of place (in != out).  torchvision is a third-party dependency the reference does not pin and this image lacks:
 * its published algorithm is restated, parity unpinned for this one function. */
int gsd_gaussian_blur(const float* in, int64_t planes, int H, int W, const float* kernel2d, int K, float* out, void* stream);
/* Per-channel {min, max, mean, unbiased std} over x (N,C,HW) -> out[4*C] doubles
 * (calculate_image_normalization_params / calculate_depth_normalization_params, general_dataset.py:199-220).
 * workspace: gsd_channel_stats_workspace(C) doubles. Deterministic (fixed reduction order).
 * Non-finite input answers as torch's tensor.min() / .max() / .mean() / .std() do: a NaN element makes all four statistics of
 * its channel NaN; an infinity gives an infinite mean and a NaN std; N * HW == 1 gives a NaN std. */
int64_t gsd_channel_stats_workspace(int C);
int gsd_channel_stats(const float* x, int64_t N, int C, int64_t HW, double* out, double* workspace, void* stream);
/* Batch assembly (__getitem__ + normalize_sample, general_dataset.py:222-236, behind DataLoader's shuffle):
 *   out[b,c,:] = A[min(c,nab-1)] * src[idx[b],c,:] + B[min(c,nab-1)],  src (M,C,HW), idx int64[B] on the device.
 * An index outside [0,M) fills its row with NaN (never reads out of bounds). */
int gsd_gather_affine(const float* src, const int64_t* idx, int64_t M, int B, int C, int64_t HW, const float* A,
                      const float* Bc, int nab, float* out, void* stream);

/* On-device data augmentation riding in the batch gather (an addition: the reference's __getitem__ only normalises).
 * Every random choice is a pure function of (seed, epoch, dataset row) -- never of the position in the batch, of the batch
 * size, of the rank or of any host generator -- so a resumed run, a data-parallel run and a single process see the same
 * samples.  The stream (uint64, wrap-around; g = 0x9E3779B97F4A7C15; fin = splitmix64's finaliser; mix(z) = fin(z + g)):
 *   K   = mix(mix(mix(seed) ^ epoch) ^ index)                 the sample key
 *   r_k = fin(K + (k+1) g)                                    draw k of the sample
 *   r_0: hflip = (r_0 >> 40) 2^-24 < p_hflip,  vflip = ((r_0 >> 16) & 0xFFFFFF) 2^-24 < p_vflip
 *   r_1: dy = -max_dy + (((r_1 >> 32) (2 max_dy + 1)) >> 32),  dx the same from the low 32 bits with max_dx
 *   r_{2+c}: u, u' as in r_0;  gain[c] = fmaf(gain, 2u - 1, 1),  offset[c] = offset (2u' - 1)
 *   noise: Kn = mix(K ^ 0x6E6F697365), r = fin(Kn + (e+1) g), n = float(sum of r's four 16-bit fields - 131070) * fp32(sqrt(3)/65536)
 *          for element e = c*H*W + h*W + w of the OUTPUT image: unit variance, |n| <= 3.47, no transcendental function.
 * Geometry (image AND depth, the same draw): output pixel (h, w) reads
 *   hs = clamp(h - dy, 0, H-1), ws = clamp(w - dx, 0, W-1), then hs = H-1-hs if vflip, ws = W-1-ws if hflip
 * -- shift(flip(src)) with edge replication; every read stays inside the sample's own plane.
 * Photometry (image only, raw units, fp32): t = x - pivot; x1 = fmaf(gain[c], t, pivot) + offset[c];
 *   x2 = fmaf(noise_std, n, x1); y = fmaf(x2, A[c], B[c]).  With gain == offset == noise_std == 0 it is exactly
 *   y = fmaf(x, A[c], B[c]): a geometry-only augmentation is a bitwise permutation of gsd_gather_affine's output.
 *   Depth is always fmaf(x, A, B). */
typedef struct gsd_augment {
  uint64_t seed;
  int64_t epoch;
  float p_hflip, p_vflip;  /* probabilities in [0, 1]                             */
  int32_t max_dy, max_dx;  /* shifts uniform on [-max, max] pixels, 0 <= max <= 2^20 */
  float gain;              /* per-channel gain uniform on 1 +- gain, in [0, 1)     */
  float offset;            /* per-channel offset uniform on +- offset, >= 0        */
  float noise_std;         /* per-pixel noise scale, >= 0                          */
  float pivot;             /* the value the gain leaves in place                   */
} gsd_augment;

/* One launch assembles the image batch and the depth batch of a train step: gsd_gather_affine of img (M,Ci,H,W) and of
 * dep (M,Cd,H,W) with the sample's augmentation applied on the way; out_img (B,Ci,H,W), out_dep (B,Cd,H,W).
 * A null pointer, a non-positive size, a probability outside [0,1], a shift outside [0, 2^20], gain outside [0,1), a
 * negative offset / noise_std or any non-finite field returns GSD_ERR_BAD_ARG before any launch; Ci > 8 (or B,
 * Ci + Cd > 65535, H*W >= 2^30) returns GSD_ERR_UNSUPPORTED.  An index outside [0,M) fills that sample's image and depth rows
 * with NaN and reads nothing out of bounds. */
int gsd_gather_augment(const float* img, const float* dep, const int64_t* idx, int64_t M, int B, int Ci, int Cd, int H, int W,
                       const float* Ai, const float* Bi, int nabi, const float* Ad, const float* Bd, int nabd,
                       const gsd_augment* aug, float* out_img, float* out_dep, void* stream);

/* Host only, touches no device: what the kernel draws for dataset row `index` (gain / offset of channels >= Ci: 1 / 0). */
typedef struct gsd_augment_draw {
  int32_t hflip, vflip, dy, dx;
  float gain[8], offset[8];
} gsd_augment_draw;
int gsd_augment_sample(const gsd_augment* aug, int64_t index, int Ci, gsd_augment_draw* out);
/* Host only: the unit-variance noise values of image elements [first, first+n) of row `index`
 * (element e = c*H*W + h*W + w of the OUTPUT image). */
int gsd_augment_noise(const gsd_augment* aug, int64_t index, int64_t first, int64_t n, float* out);

#ifdef __cplusplus
}
#endif
#endif /* GSD_H */
