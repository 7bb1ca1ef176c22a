/*
 * dau_conv.h -- C ABI of the MI355X-native DAU convolution operator.
 *
 * This is the drop-in boundary for the reference's DAU forward/backward path.  Every
 * entry point takes plain device pointers, sizes and a HIP stream handle; there are no
 * framework types in the signatures.  What each entry point replaces in
 * skokec/DAU-ConvNet (paths relative to the reference tree):
 *
 *   dau_conv_plan_create / _destroy   BaseDAUConvLayer::LayerSetUp + Reshape
 *                                     (src/dau_conv/base_dau_conv_layer.cpp:29-187,190-394),
 *                                     DAUConvForward / DAUConvBackward constructors
 *                                     (src/dau_conv/dau_conv_impl/dau_conv_forward.cpp:28-77,
 *                                      dau_conv_backward.cpp:11-89), DAUConvSettings
 *                                     (include/dau_conv/base_dau_conv_layer.hpp:109-130)
 *   dau_conv_workspace_bytes          DAUConvForward::get_allocation_sizes
 *                                     (include/dau_conv/dau_conv_impl/dau_conv_forward.hpp:30-33),
 *                                     DAUConvBackward::get_allocation_sizes (dau_conv_backward.hpp:41-42),
 *                                     allocate_workspace_mem (base_dau_conv_layer.hpp:263)
 *   dau_conv_forward                  DAUConvOp::Compute (plugins/tensorflow/src/dau_conv_op.cpp:150-324)
 *                                     -> BaseDAUConvLayer::Forward_gpu (src/dau_conv/base_dau_conv_layer.cu:15-127)
 *                                     -> DAUConvForward::forward_pass (dau_conv_forward.cpp:128-174)
 *   dau_conv_backward                 DAUConvGradOp::Compute (plugins/tensorflow/src/dau_conv_grad_op.cpp:115-318)
 *                                     -> BaseDAUConvLayer::Backward_gpu (base_dau_conv_layer.cu:130-363)
 *                                     -> DAUConvBackward::backward_pass (dau_conv_backward.cpp:173-232)
 *   dau_conv_forward_epilogue /       the bias add and activation of the Python layer (plugins/tensorflow/dau_conv/dau_conv.py:500-525)
 *   dau_conv_forward_residual /       (_residual: with a residual block's shortcut added between the two)
 *   dau_conv_epilogue_backward        fused into the forward store, and their gradients in one pass (no reference kernel: TF's own ops)
 *   dau_conv_backward_param_sums /    the two halves of Backward_gpu's parameter-gradient path: the raw sums of K4
 *   dau_conv_finalize_param_grads     (base_dau_conv_layer.cu:232-241) and its elementwise tail (dmu *= w, ignored units,
 *                                     NaN -> 0, :335-355; lr factor, dau_conv_grad_op.cpp:297-303), split so that a
 *                                     data-parallel caller can all-reduce the sums in between
 *   dau_conv_check_status /           the max|mu| / NaN precondition checks of the ops
 *   dau_conv_last_status              (dau_conv_op.cpp:223-262, dau_conv_grad_op.cpp:209-250); done on the
 *                                     device without a host sync, read back only on request (check_status waits for
 *                                     the stream; last_status reads what completed calls left in pinned host
 *                                     memory, without waiting; a bad status stays there until it has been reported)
 *   dau_conv_filters                  BaseDAUKernelCompute::get_kernels (base_dau_conv_layer.cu:537-710)
 *   dau_conv_unit_table               perpare_weights_and_offsets (dau_conv_forward_core.hpp:1858-2215)
 *   dau_conv_last_error               DAUException::what (include/dau_conv/util/common.hpp:40-66)
 *
 * Tensor layouts (identical to the reference): activations NCHW contiguous float32 (or,
 * with DAU_FLAG_IO_BF16 / DAU_FLAG_IO_F16, bfloat16 / binary16 storage of x, y, dy, dx -- arithmetic stays fp32;
 * with DAU_FLAG_IO_NHWC the same activations as [N][H][W][C] arrays);
 * parameters and their gradients [1,S,G,F] contiguous float32 (f fastest); sigma is a
 * full [1,S,G,F] tensor whose element 0 is used (base_dau_conv_layer.hpp:266-275).
 * Alignment: every pointer need only be aligned to its element type (4 bytes for float32, 2 bytes for the 16-bit activation
 * formats) -- the kernels take their wider loads only where a base allows them, with the same results bit for bit -- so a
 * contiguous slice of a larger tensor can be passed as it is; the workspace wants the 256 bytes a hipMalloc gives.
 *
 * Ownership: the caller owns every buffer, including one workspace per in-flight call.
 * A plan's configuration is immutable after creation, so concurrent calls on different
 * streams with different workspaces are safe.  Only dau_conv_plan_create / _destroy allocate
 * (the plan and 32 bytes of pinned host memory for its status mirror) and only
 * dau_conv_check_status synchronises (it waits for the stream); no other call allocates,
 * frees or synchronises.  A plan may be used on any device (the kernels' launch attributes are
 * set once per device, on the first call there, behind a lock).
 * dau_conv_backward OVERWRITES the gradient outputs (the reference op zero-fills them and
 * then accumulates, dau_conv_grad_op.cpp:202-205 -- same net result).
 *
 * Images are independent.  y[n] and dx[n] depend only on image n of the input (x[n], dy[n]) and on the
 * parameters -- not on the other images of the batch, and not on how the batch is cut into slabs (below): the
 * same image gives the same bits in any batch.  That holds for every gather-sum kernel, the two-limb f16 dense
 * members (DAU_FLAG_DENSE_SPLIT_F16) included, which scale each image by a power of two of its own.  A
 * non-finite input element affects only the outputs its taps reach within its own image.
 *
 * Offset buckets.  The kernels stage a border of R pixels around every tile, R in
 * {4, 8, 16, 18, 20, 24, 32}.  The reference picks R per call from a blocking amax of mu1/mu2
 * (dau_conv_op.cpp:223-253).  Here a plan holds the kernel sets of every R up to the one
 * max_kernel_size allows; a call enqueues the set that covered the previous call's max|mu|
 * (read from the pinned mirror, no sync) plus the largest set, each guarded on the device by
 * THIS call's max|mu|, so exactly one does the work and results never depend on the hint (with
 * DAU_FLAG_DENSE_BF16 the bucket-4 member, the only one with bf16 arithmetic, is enqueued as a guarded
 * candidate on EVERY call, so that too is decided by the call's own offsets alone).  That is the rule of the
 * gather-sum passes (y, dx), whose sums do not depend on the tile: every set gives the same bits.  The tiled
 * parameter-gradient kernel sums over regions that differ from set to set, so its bits depend on the set: that
 * pass takes no hint and enqueues every set it holds, each guarded by its own range of offsets -- the smallest
 * set that covers THIS call's max|mu| runs.  So all six results of a call are, bit for bit, a function of the
 * call's own arguments, whatever other calls, streams or threads that share the plan left in the mirror.
 *
 * Streams and threads.  One plan; any number of streams and host threads; one workspace per call in flight.  Per
 * workspace: the status block a call writes, hence dau_conv_check_status and the _status queries that take a
 * workspace -- they report the call that used THAT workspace, whatever ran beside it.  Per plan, shared by all its
 * callers: the pinned mirror -- the most recent completed call (of any stream: the hint, and what
 * dau_conv_last_status reports without an error), the sticky bad-offset record (an error of any stream stays
 * until dau_conv_last_status, or dau_conv_check_status on the workspace of the bad call, has returned it once)
 * and the sigma record.  dau_conv_last_error is per host thread.
 *
 * Workspace.  Every pass stages its input before it gathers.  Where the staged copy of the
 * whole batch would exceed 12 GB (DAU_WORKSPACE_BUDGET_GB in the environment at plan
 * creation; only 512 x 512 maps get there) the pass runs over the batch in slabs of an even
 * divisor of N images, and dau_conv_workspace_bytes reports the smaller requirement.  y and dx
 * of a slabbed pass are bit-identical to the whole-batch pass (images are independent).
 *
 * HIP graphs.  After one ordinary call (which sets the kernels' launch attributes) forward and
 * backward only enqueue kernels on the caller's stream (what a pass clears in its workspace it clears with a kernel), so they can be
 * captured into a graph; the bucket candidates are frozen at capture time, the device-side
 * guards still pick the kernels the replay's offsets need.  A plan's prefilter support k is frozen
 * too, like its bucket candidates: it was chosen from sigma_hint when the plan was made, the taps
 * are computed from the device's sigma on every call, and a replay runs no host code that could
 * choose another plan when a trained sigma crosses a support boundary.  The device therefore
 * records, in the plan's pinned mirror, the support each call's sigma would have needed; a caller
 * who replays must ask dau_conv_sigma_status (and dau_conv_last_status for the offsets) and capture
 * again with a new plan when more was needed than the plan holds.  A captured call may use a
 * workspace of its own that is released after the capture in capture order: no pass reads what an
 * earlier call left in its workspace.  The plan must outlive every graph that holds a call of it
 * (each replay writes its mirror), and the queries that read a workspace back
 * (dau_conv_check_status and the _status entries that take one) need that workspace to be alive.
 */
#ifndef DAU_CONV_H_
#define DAU_CONV_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DAU_CONV_ABI_VERSION 4

#if defined(__GNUC__)
#define DAU_API __attribute__((visibility("default")))
#else
#define DAU_API
#endif

/* Status codes; they map 1:1 onto the TensorFlow codes the reference ops raise. */
enum {
    DAU_OK = 0,
    DAU_INVALID_ARGUMENT = 1,    /* bad shape/attr, |mu| larger than the offset bucket allows   */
    DAU_FAILED_PRECONDITION = 2, /* NaN in mu1/mu2, sigma <= 0                                   */
    DAU_INTERNAL = 3             /* HIP runtime error (reference: DAUException -> INTERNAL)      */
};

/* dau_conv_desc.flags */
enum {
    DAU_FLAG_USE_INTERPOLATION = 1 << 0,    /* attr use_interpolation (default true)              */
    DAU_FLAG_UNIT_TESTING = 1 << 1,         /* attr unit_testing: drop last error row/col per the
                                               oracle rule (dau_conv_test.py:110-136)             */
    DAU_FLAG_SINGLE_DIM_KERNEL = 1 << 2,    /* attr single_dim_kernel (DAUConv1d)                 */
    DAU_FLAG_FORBID_POSITIVE_DIM1 = 1 << 3, /* attr forbid_positive_dim1                          */
    DAU_FLAG_IO_BF16 = 1 << 4,              /* x, y, dy, dx are bfloat16 arrays (passed through the
                                               float* parameters); parameters, their gradients and all
                                               arithmetic stay fp32.  Needs the tiled kernels: plan
                                               creation fails where only the direct ones apply.        */
    DAU_FLAG_STATIC_BUCKET = 1 << 5,        /* always run the kernels of the bucket max_kernel_size allows (no
                                               per-call selection from the actual offsets)             */
    DAU_FLAG_DENSE_BF16 = 1 << 6,           /* with DAU_FLAG_IO_BF16: calls whose offsets lie within +-4 run their
                                               two gather-sum passes (y, dx) as a DENSIFIED implicit GEMM on the
                                               bf16 matrix cores (units scattered into a 9x9 kernel per channel
                                               pair -- 7x7 when the call's offsets lie within +-3, decided on the
                                               device; taps and blurred activations rounded to bf16, fp32 sums),
                                               and -- from three units per channel on -- their parameter gradients as dense cross-correlations on the
                                               same matrix cores (filtered input and error rounded to bf16, fp32
                                               sums).  Otherwise the exact fp32 path.                        */
    DAU_FLAG_DENSE_WGRAD_NEVER = 1 << 7,    /* with DAU_FLAG_DENSE_BF16: keep the exact fp32 gather-dot for the
                                               parameter gradients whatever the unit count                   */
    DAU_FLAG_DENSE_WGRAD_ALWAYS = 1 << 8,   /* with DAU_FLAG_DENSE_BF16: dense parameter gradients from ONE unit
                                               per channel on (default: from three, where they start to pay) */
    DAU_FLAG_DENSE_SPLIT_F16 = 1 << 9,      /* The two gather-sum passes (y, dx) of calls whose offsets lie within +-2 / +-3 / +-4 can run
                                               as a DENSIFIED 5x5 / 7x7 / 9x9 implicit GEMM on the f16 matrix cores with BOTH operands
                                               split into two binary16 limbs (hi + lo, 22 significant bits; products hi*hi + lo*hi +
                                               hi*lo, fp32 sums, k_dense_split.hip): fp32 accuracy -- the same parity bar as the exact
                                               gather, measured margins in profiles/ -- at 3 * taps / 16 of the fp32 rate per (pixel,
                                               channel pair) instead of 4 G.  float32, bfloat16 or float16 activations; the call's offsets decide
                                               on the device which member runs; every other call keeps the exact kernels.
                                               The limbs are taken after an exact power-of-two scaling, ONE SCALE PER IMAGE (from the
                                               image's largest finite |value|; the dense taps likewise from the finite units): y[n] and
                                               dx[n] depend only on image n of the input and on the parameters, whatever the other
                                               images hold and however the batch is cut into slabs; a non-finite element (Inf, NaN)
                                               affects only the outputs its taps reach within its own image -- in the dense form the
                                               whole (2R+1)^2 kernel around the prefiltered element.  Dynamic range within one image:
                                               values below 2^-17 of that image's maximum carry an absolute error below 2^-39 of it.
                                               The parameter gradients of interpolating, 2-D calls within +-4 likewise run as a
                                               two-limb f16 GEMM with the four kinds x four bilinear corners as rows (k_split_dot.hip,
                                               fp32 accuracy), for float32, float16 and bfloat16 activations alike.  A bfloat16 layer's
                                               error enters in ONE limb (a bf16 dy times its channel's power-of-two scale is exactly
                                               representable in binary16: two products per tile instead of three): its parameter
                                               gradients meet the fp32 bar; an error value of at least 2^-27 of its output channel's
                                               largest finite |dy| enters exactly, smaller ones are rounded to the f16 subnormal grid
                                               (an absolute error below 2^-38 of that maximum); a non-finite dy element affects only
                                               its own output channel's gradients, a non-finite x element only its own input
                                               channel's.  DEFAULT (neither flag): the members that pay for the plan's unit count
                                               (on whole tiles: radius 2 from two units per channel pair, radius 3 from three, radius 4 from four;
                                               the parameter-gradient member where blocks of four units are at least 3/4 full: G = 3, 4, 7, 8, ...).
                                               This flag: all members whatever the unit count.                             */
    DAU_FLAG_NO_DENSE_SPLIT = 1 << 10,      /* never: always the exact fp32 gather and gather-dot (excludes DAU_FLAG_DENSE_SPLIT_F16) */
    DAU_FLAG_IO_F16 = 1 << 11,              /* x, y, dy, dx are IEEE binary16 arrays (passed through the float* parameters, as with
                                               DAU_FLAG_IO_BF16); parameters, their gradients, the raw sums of
                                               dau_conv_backward_param_sums and all arithmetic stay fp32.  The plan runs exactly
                                               the members, and the arithmetic, of the fp32 plan of the same desc on the widened
                                               input; results are stored rounded to nearest even (f16 subnormals kept, beyond
                                               65504 +-inf, a NaN stays a NaN), once per offset-window pass.  Needs the tiled
                                               kernels; excludes DAU_FLAG_IO_BF16, DAU_FLAG_DENSE_BF16 and its qualifiers.   */
    DAU_FLAG_DENSE_SPLIT_OUTLIERS = 1 << 12, /* opt-in: a call whose offsets reach into (3, 4] in FEW units keeps the radius-3 two-limb
                                               GEMM for its gather-sum passes (y, dx).  The bilinear corners that land inside 7x7 stay
                                               in the dense kernel; the corners on the ring |tap| = 4 (at most three per such unit)
                                               are gathered by a list-driven fp32 pass of their own (k_dense_ring.hip) whose sums join
                                               the GEMM's before the one rounding of the store.  The device takes this member when
                                               max|mu| lies in (3, 4] and the units beyond +-3 are at most a fraction of the plan's
                                               live units that is fixed at plan creation; every other call runs what it runs without
                                               the flag.  Holds where the plan holds the radius-3 member (DAU_FLAG_DENSE_SPLIT_F16
                                               forces that); inert elsewhere; excludes DAU_FLAG_NO_DENSE_SPLIT and DAU_FLAG_DENSE_BF16.
                                               The parameter gradients are not affected.                                     */
    DAU_FLAG_IO_NHWC = 1 << 13,             /* x, y, dy, dx of dau_conv_forward, dau_conv_backward and dau_conv_backward_param_sums are
                                               [N][H][W][C] arrays (C = S for x / dx, F for y / dy: torch.channels_last) instead of
                                               [N][C][H][W].  Parameters, their gradients, the raw sums, the unit table and the filters
                                               do not change, nor does anything inside the workspace: the plan is the NCHW plan of the
                                               same desc (members, buckets, windows, tilings, batch slabs, dau_conv_plan_info,
                                               dau_conv_workspace_bytes) in everything but the addresses of the activations, and a call
                                               returns, bit for bit, what the NCHW call returns on the permuted arrays.  Combines with
                                               DAU_FLAG_IO_BF16 / DAU_FLAG_IO_F16 and every other flag except DAU_FLAG_DENSE_BF16 and
                                               its qualifiers; needs the tiled kernels (not DAU_ALGO_DIRECT, nor a shape that falls
                                               back to the direct kernels).  Alignment: none beyond that of an element -- the 16-byte
                                               load and store paths check the base address and the channel count at run time and
                                               fall back to element-wise access.                                              */
    DAU_FLAG_INPUT_RELU = 1 << 14,          /* a ReLU in front of the layer, fused into it (conv -> BatchNorm -> ReLU -> DAU: the caller passes
                                               the BatchNorm output as x, no ReLU pass runs and its output is never materialised).
                                               dau_conv_forward (and _epilogue / _residual), every parameter-gradient pass and
                                               dau_conv_backward_param_sums compute exactly -- bit for bit -- what the plan without the flag
                                               computes on x' = (x <= 0) ? +0 : x: a NaN stays a NaN, -0 becomes +0, 16-bit formats are
                                               widened first; the clamp sits where the staging kernels widen the x they load (the per-image
                                               scales of the two-limb members are those of x').  The dx pass of dau_conv_backward stores
                                               dx = (x <= 0) ? 0 : s, s the value the plan without the flag would store -- the rule of a
                                               threshold at zero: a NaN x passes s through -- applied after the sum, before the store's one
                                               rounding, in the last window of a pass of several offset windows: mask(old + v).  x is the
                                               pointer dau_conv_backward receives anyway (dx's shape, format and layout; under batch slabs
                                               indexed by the global image) and must be non-NULL with DAU_NEED_DX alone too; where the
                                               channel count is a multiple of four the NHWC stores load it four channels at once if x's
                                               OWN base allows (16 bytes float32, 8 bytes 16-bit), element-wise otherwise -- same bits.
                                               The plan is the plan of the same desc without the flag (members, buckets, windows, slabs,
                                               dau_conv_plan_info, dau_conv_workspace_bytes); images stay independent.  Combines with
                                               DAU_FLAG_IO_BF16 / _IO_F16 / _IO_NHWC, the split flags, DAU_FLAG_DENSE_SPLIT_OUTLIERS,
                                               DAU_FLAG_STATIC_BUCKET and the fused output epilogue and residual of the same call;
                                               excludes DAU_FLAG_DENSE_BF16; needs the tiled kernels (not DAU_ALGO_DIRECT, nor a shape
                                               that falls back to the direct kernels).                                          */
    DAU_FLAG_DENSE_SPLIT_LINE = 1 << 15,    /* opt-in, single-dimension layers (needs DAU_FLAG_SINGLE_DIM_KERNEL): the gather-sum passes (y, dx)
                                               of a call whose units all lie on the row of their pixel -- mu2 == 0, i.e. every entry of the
                                               pass's unit table has a vertical displacement of 0 and no weight on the row below; ignored
                                               units count -- run as the two-limb f16 GEMM over ONE row of taps: 1 x 9 for offsets within
                                               +-4, 1 x 17 within +-8 (where max_kernel_size >= 11 allows such offsets) instead of the
                                               9 x 9 kernel or the exact gather.  fp32 accuracy, as the 2-D two-limb members.  The device
                                               decides per call: a call with a unit off the line (a NaN / Inf weight counts as one) runs
                                               exactly the kernels of the plan without the flag and returns its bits.  A line member is
                                               held where the cost model says it pays in both directions (DAU_FLAG_DENSE_SPLIT_F16: always)
                                               and the prefilter support has a two-limb staging kernel (<= 11); dau_conv_plan_info
                                               .gather_dense_split bits 6 / 7 report it.  Without the flag no plan changes.  Inert under
                                               DAU_FLAG_STATIC_BUCKET and DAU_ALGO_DIRECT; excludes DAU_FLAG_NO_DENSE_SPLIT and
                                               DAU_FLAG_DENSE_BF16; combines with every other flag.  The parameter gradients are not
                                               affected.                                                                         */
    DAU_FLAG_SPLIT_DOT_LINE = 1 << 16,      /* opt-in, single-dimension layers (needs DAU_FLAG_SINGLE_DIM_KERNEL and
                                               DAU_FLAG_USE_INTERPOLATION): the parameter-gradient pass (dw, dmu1, dsigma; dmu2 stays zero) of
                                               a call whose units all lie on the row of their pixel -- every entry of the pass's bare unit
                                               table has a vertical displacement of 0 and no factor on the row below; ignored units count --
                                               runs as the line member of the two-limb f16 gather-dot: horizontal radius 4 for offsets within
                                               +-4, radius 8 within +-8 (where max_kernel_size >= 11 allows such offsets), no vertical halo,
                                               instead of the exact fp32 gather-dot of bucket 4 / 8 (the kernels behind the reference's
                                               DAUConvBackward for such layers, dau_conv_backward_core.hpp).  fp32 accuracy, as the 2-D
                                               two-limb member; a bf16 layer's error is staged in one limb.  The device decides per call: a
                                               call with a unit off the line runs exactly the kernels of the plan without the flag and
                                               returns its bits.  Held where the 2-D member would be held for a layer that is not
                                               single-dimension (bucket 4's set, the whole batch in one pass, three or four units of every
                                               block of four or DAU_FLAG_DENSE_SPLIT_F16, the workspace under the budget);
                                               dau_conv_plan_info.gather_dense_split bits 8 / 9 report it, dau_conv_dot_line_status what a call
                                               took.  dau_conv_backward and dau_conv_backward_param_sums alike.  Without the flag no plan
                                               changes.  Inert under DAU_FLAG_STATIC_BUCKET and DAU_ALGO_DIRECT; excludes
                                               DAU_FLAG_NO_DENSE_SPLIT and DAU_FLAG_DENSE_BF16; independent of DAU_FLAG_DENSE_SPLIT_LINE (the
                                               gather-sum passes) and combines with it and with every other flag.                 */
    DAU_FLAG_DEFAULT = DAU_FLAG_USE_INTERPOLATION
};

/* dau_conv_desc.algo */
enum {
    DAU_ALGO_AUTO = 0,      /* fastest kernels that support the shape                            */
    DAU_ALGO_DIRECT = 1,    /* plain one-thread-per-output HIP kernels (any shape)               */
    DAU_ALGO_TILED = 2      /* LDS-tiled MFMA gather / wave-reduced gradient kernels             */
};

/* which pass a workspace is sized for (DAU_PASS_EPILOGUE_BACKWARD: the partial sums of dau_conv_epilogue_backward's dbias -- small:
 * one float per output channel and 16384 elements or so of the activations) */
enum { DAU_PASS_FORWARD = 1, DAU_PASS_BACKWARD = 2, DAU_PASS_EPILOGUE_BACKWARD = 3 };

/* the epilogue fused into the forward pass's store (dau_conv_forward_epilogue): y = act(sum + bias[f]) */
enum {
    DAU_EPILOGUE_BIAS = 1,   /* add bias[f] (F floats, always float32) to output channel f                       */
    DAU_EPILOGUE_RELU = 2    /* then v <= 0 ? 0 : v (a NaN stays a NaN)                                          */
};

/* dau_conv_backward need-mask (params_propagate_down of Backward_gpu) */
enum {
    DAU_NEED_DX = 1 << 0,
    DAU_NEED_DW = 1 << 1,
    DAU_NEED_DMU1 = 1 << 2,
    DAU_NEED_DMU2 = 1 << 3,
    DAU_NEED_DSIGMA = 1 << 4,
    DAU_NEED_ALL = 31
};

typedef struct dau_conv_desc {
    int32_t struct_size;            /* sizeof(dau_conv_desc), for ABI evolution                   */
    int32_t batch;                  /* N                                                          */
    int32_t in_channels;            /* S                                                          */
    int32_t out_channels;           /* F  (attr num_output)                                       */
    int32_t units_per_channel;      /* G  (number_units_x * number_units_y, incl. ignored units)  */
    int32_t height, width;          /* H, W (output size == input size, dau_conv_op.cpp:185-188)  */
    int32_t max_kernel_size;        /* attr kernel_size: 9/17/33/37/41/49/65 -> largest offset
                                       bucket 4/8/16/18/20/24/32                                  */
    int32_t number_units_ignore;    /* attr number_units_ignore                                   */
    int32_t flags;                  /* DAU_FLAG_*                                                 */
    int32_t algo;                   /* DAU_ALGO_*                                                 */
    float sigma_hint;               /* host copy of sigma; sizes the blur support 2*ceil(5s)+1 as
                                       LayerSetUp does (base_dau_conv_layer.cpp:140-147); the taps
                                       themselves are computed from the device tensor each call   */
    float mu_learning_rate_factor;  /* attr mu_learning_rate_factor (grad op only)                */
} dau_conv_desc;

typedef struct dau_conv_plan dau_conv_plan; /* opaque */

typedef struct dau_conv_plan_info {
    int32_t offset_bucket;     /* largest (static) R in {4,8,16,18,20,24,32}                      */
    int32_t blur_support;      /* k of the k x k prefilter                                        */
    int32_t algo_forward;      /* DAU_ALGO_* actually used by dau_conv_forward / the dx pass      */
    int32_t algo_backward;     /* DAU_ALGO_* actually used for the parameter gradients            */
    int32_t drop_last_col;     /* unit_testing edge rule outcome for this W                       */
    int32_t drop_last_row;     /* ... and H                                                       */
    int32_t gather_patch;      /* tiled gather-sum: pixels per patch side (0: direct kernel)      */
    int32_t gather_stack;      /* ... and (image pair, patch) planes gathered per workgroup       */
    int32_t dot_windows;       /* tiled gather-dot: offset windows (1 for kernels <= 17)          */
    int32_t gather_windows;    /* tiled gather-sum: offset-window passes (1 for kernels <= 33)    */
    int32_t bucket_sets;       /* kernel sets a call can choose from (1: static bucket only)      */
    int32_t gather_dense_bf16; /* 1: the bucket-4 gather-sum passes use the densified bf16 GEMM;
                                  2: the parameter gradients too (three or more units)          */
    int32_t batch_slab_gather; /* images staged and gathered at a time by the y / dx passes and   */
    int32_t batch_slab_dot;    /* by the parameter-gradient pass of the static bucket (= batch
                                  unless the staged copy would exceed the workspace budget)      */
    int32_t dot_region;        /* tiled gather-dot of the static bucket: 100 * columns + rows of the
                                  positions one sweep covers (808, 807, 1404, 804; 0: direct)     */
    int32_t gather_fblock;     /* tiled gather-sum y pass of the static bucket: output channels per
                                  workgroup (4, 8, 12, 16; 0: direct)                             */
    int32_t gather_variant;    /* ... and the row of its kernel table (k_gather_mfma.hip kVariants) */
    int32_t dense_bf16_radius3; /* DAU_FLAG_DENSE_BF16 plans: 1 if calls within +-3 take the 7x7 members (gather-sum), 2 if the parameter
                                   gradients do too (49 displacements); 0: the 9x9 members only */
    int32_t gather_dense_split; /* bit r (r = 2, 3, 4): calls whose offsets lie within +-r can run their gather-sum passes as the
                                   two-limb f16 GEMM of that radius (0: never); bit 5: calls within +-4 with few units beyond +-3
                                   can run theirs as the radius-3 GEMM plus the ring pass (DAU_FLAG_DENSE_SPLIT_OUTLIERS); bits 6 and
                                   7: calls whose units lie on a line, offsets within +-4 / within (4, 8], can run theirs as the 1 x 9 /
                                   1 x 17 line member (DAU_FLAG_DENSE_SPLIT_LINE); bits 8 and 9: such calls can run their parameter
                                   gradients as the line member of the two-limb gather-dot of radius 4 / 8 (DAU_FLAG_SPLIT_DOT_LINE) */
} dau_conv_plan_info;

DAU_API int dau_conv_abi_version(void);
/* sha-256 prefix (16 hex digits) over the kernel sources this library was built from (the .hip and .hpp files of csrc, its Makefile, this
 * header), set by the Makefile: measurement files (profiles/) name the build they were taken from by it. */
DAU_API const char *dau_conv_build_id(void);
DAU_API const char *dau_conv_last_error(void); /* thread-local message of the last failing call */

/* Support k of the k x k prefilter a sigma needs: 2*ceil(5*sigma)+1 in float32 (base_dau_conv_layer.cpp:146).  A plan depends on
 * sigma_hint only through this number, so callers that cache plans key them on it (a trainable sigma changes every step). */
DAU_API int dau_conv_filter_support(float sigma);

DAU_API int dau_conv_plan_create(const dau_conv_desc *desc, dau_conv_plan **plan_out);
DAU_API int dau_conv_plan_destroy(dau_conv_plan *plan);
DAU_API int dau_conv_plan_get_info(const dau_conv_plan *plan, dau_conv_plan_info *info);
DAU_API int dau_conv_workspace_bytes(const dau_conv_plan *plan, int pass, size_t *bytes_out);
/* Geometry of the two-limb f16 parameter-gradient kernel (k_split_dot.hip) of a plan that holds it: the region width (columns of a
 * region = K steps of a full item: 10 or 12), the regions (items) of one column strip and the K steps the kernel runs for a strip --
 * region_width per item, ceil(region_width / 4) for a strip's last item where (H + 1) % 4 == 1 leaves it one real row.  All three are 0
 * for a plan without that kernel.  Needs no device.  Any pointer may be NULL. */
DAU_API int dau_conv_split_dot_geometry(const dau_conv_plan *plan, int32_t *region_width, int32_t *strip_items, int32_t *strip_k_steps);

/* stream is a hipStream_t (NULL = default stream).  All pointers are device pointers. */
DAU_API int dau_conv_forward(const dau_conv_plan *plan, void *stream, const float *x, const float *w,
                     const float *mu1, const float *mu2, const float *sigma, float *y,
                     void *workspace, size_t workspace_bytes);

/* The bias add and the activation of the reference's layer (plugins/tensorflow/dau_conv/dau_conv.py:500-525: tf.nn.bias_add, then
 * self.activation), fused into the store of dau_conv_forward: y = act(sum + bias[f]) with act the identity or ReLU, computed in fp32
 * from the very value dau_conv_forward would have stored, BEFORE the store's one rounding -- for float32 activations the bits of
 * relu(dau_conv_forward(...) + bias), for 16-bit activations one rounding where the unfused form rounds twice, and y keeps the
 * activations' format.  bias: F floats, always float32; may be NULL without DAU_EPILOGUE_BIAS.  With several offset windows
 * (dau_conv_plan_info.gather_windows > 1) the epilogue belongs to the last window's store: act(old + v + bias).  epilogue == 0 is
 * dau_conv_forward exactly.  The workspace is the DAU_PASS_FORWARD one.  y of a DAU_FLAG_IO_NHWC plan is, bit for bit, y of the NCHW
 * plan on the permuted arrays.  _supported: DAU_OK, or DAU_INVALID_ARGUMENT (and dau_conv_last_error names the reason) for a plan
 * whose forward pass runs on the direct kernels, for a DAU_FLAG_DENSE_BF16 plan and for unknown epilogue bits; _forward_epilogue
 * refuses the same.  The input-gradient pass takes no epilogue. */
DAU_API int dau_conv_epilogue_supported(const dau_conv_plan *plan, int epilogue);
DAU_API int dau_conv_forward_epilogue(const dau_conv_plan *plan, void *stream, const float *x, const float *w,
                     const float *mu1, const float *mu2, const float *sigma, const float *bias, int epilogue,
                     float *y, void *workspace, size_t workspace_bytes);

/* dau_conv_forward_epilogue with the shortcut of a residual block added between the reference layer's bias_add and its activation
 * (plugins/tensorflow/dau_conv/dau_conv.py:500-525; the add itself is the network's, e.g. relu(dau(x) + bias + shortcut)):
 *   y = act((sum + bias[f]) + residual[n,f,h,w])
 * in that order -- the bias add first, the residual second, each one float32 add, then the optional ReLU, then the store's one
 * rounding -- so that float32 activations give the bits of relu((dau_conv_forward(...) + bias) + residual).  `residual` has y's shape,
 * the plan's activation format (float32 / bfloat16 / binary16 behind the float*, widened exactly) and layout ([N][F][H][W], or
 * [N][H][W][F] under DAU_FLAG_IO_NHWC), and under batch slabs is indexed by the global image as y is.  It is only read, and it must
 * NOT overlap y (not checked).  Alignment: none beyond the element's; where F is a multiple of four the NHWC stores load four
 * channels at once if the residual's OWN base is 16-byte (float32) or 8-byte (16-bit) aligned, whatever y's alignment, and fall back
 * to element loads otherwise -- same bits.  A NaN or Inf in the residual reaches exactly its own element of y.  With several offset
 * windows the last window's store takes it: act(((old + v) + bias) + residual).  The residual is NOT an epilogue bit: `epilogue` keeps
 * DAU_EPILOGUE_BIAS | DAU_EPILOGUE_RELU, and a residual with epilogue == 0 is a plain fused add.  residual == NULL is
 * dau_conv_forward_epilogue exactly (with epilogue == 0: dau_conv_forward).  A non-NULL residual is accepted where
 * dau_conv_epilogue_supported(plan, DAU_EPILOGUE_BIAS) is; plans on the direct kernels and DAU_FLAG_DENSE_BF16 plans are refused
 * with DAU_INVALID_ARGUMENT.  Backward: dau_conv_epilogue_backward's dz is also the residual's gradient (without ReLU: dy itself). */
DAU_API int dau_conv_forward_residual(const dau_conv_plan *plan, void *stream, const float *x, const float *w,
                     const float *mu1, const float *mu2, const float *sigma, const float *bias, const float *residual,
                     int epilogue, float *y, void *workspace, size_t workspace_bytes);

/* Backward of that epilogue -- what autodiff derives from the reference layer's bias_add and activation (same lines) -- in one pass
 * over dy (and, with DAU_EPILOGUE_RELU, the stored y):
 *   dz = (y <= 0) ? 0 : dy     in the activations' format and layout; the rule of a threshold at zero: a NaN y passes dy through.
 *                              Written only with DAU_EPILOGUE_RELU; without it dz IS dy, nothing is copied, y and dz may be NULL.
 *                              dz may alias dy.
 *   dbias[f] = sum of dz over n, h, w, in float32 (F floats), with DAU_EPILOGUE_BIAS only (without the bit the pointer is ignored);
 *                              may be NULL, then only dz is written.  epilogue == 0 does nothing.
 * The caller passes dz (or dy) on to dau_conv_backward / dau_conv_backward_param_sums as their dy.  No atomics: partial sums in the
 * workspace (DAU_PASS_EPILOGUE_BACKWARD; not needed without dbias), reduced in a fixed order -- two calls give the same bits -- and
 * hierarchically: no value passes through more than 256 float32 additions (148 at most, for tensors up to 2^31 elements), so
 * |dbias[f] - exact| <= 2^-16 * sum |dz[:, f]|.  dz of a DAU_FLAG_IO_NHWC plan is the bits of the NCHW plan's on the permuted arrays;
 * dbias is the ONE exception to that contract: the order of a sum over positions follows memory, so the two layouts agree within
 * that bound, not bit for bit. */
DAU_API int dau_conv_epilogue_backward(const dau_conv_plan *plan, void *stream, const float *dy, const float *y, int epilogue,
                     float *dz, float *dbias, void *workspace, size_t workspace_bytes);

DAU_API int dau_conv_backward(const dau_conv_plan *plan, void *stream, const float *x, const float *dy,
                      const float *w, const float *mu1, const float *mu2, const float *sigma,
                      float *dx, float *dw, float *dmu1, float *dmu2, float *dsigma,
                      void *workspace, size_t workspace_bytes, int need_mask);

/* The parameter-gradient path of dau_conv_backward in two steps, for data-parallel callers (batch sharded over
 * ranks): _param_sums writes the raw sums r[k][s][g][f], k = {w, mu1, mu2, sigma} (4*S*G*F floats, linear in the
 * batch) into sums_out; the caller all-reduces that ONE flat buffer; _finalize_param_grads then applies the
 * elementwise tail on the reduced sums (dw = r0, dmu1 = w*r1*lr, dmu2 = w*r2*lr, dsigma = w*r3, ignored units -> 0,
 * NaN in dmu -> 0), so that every rank ends up bit-identical and a NaN on one rank is not zeroed before the exchange.
 * dau_conv_backward(need_mask of the four) == _param_sums followed by _finalize_param_grads. */
DAU_API int dau_conv_backward_param_sums(const dau_conv_plan *plan, void *stream, const float *x, const float *dy,
                                 const float *mu1, const float *mu2, const float *sigma, float *sums_out,
                                 void *workspace, size_t workspace_bytes);
DAU_API int dau_conv_finalize_param_grads(const dau_conv_plan *plan, void *stream, const float *sums, const float *w,
                                  float *dw, float *dmu1, float *dmu2, float *dsigma, int need_mask);

/* Waits for `stream`, then reports what the last call that used `workspace` found in mu1/mu2:
 * DAU_OK, DAU_FAILED_PRECONDITION (NaN) or DAU_INVALID_ARGUMENT (|mu| beyond the bucket).
 * max_abs_mu_out (may be NULL) receives max(|mu1|,|mu2|). */
DAU_API int dau_conv_check_status(const dau_conv_plan *plan, void *stream, const void *workspace,
                          float *max_abs_mu_out);

/* Waits for `stream`, then reports of the last call that used `workspace`: outlier_units = the live units (those not among the
 * number_units_ignore last of their channel pair) with max(|mu1|,|mu2|) > 3; ring_taken = 1 if a gather-sum pass of that call ran
 * as the radius-3 GEMM plus the ring pass (DAU_FLAG_DENSE_SPLIT_OUTLIERS), 0 if another member did the work.  Either may be NULL. */
DAU_API int dau_conv_gather_outlier_status(const dau_conv_plan *plan, void *stream, const void *workspace,
                                   int32_t *outlier_units, int32_t *ring_taken);

/* Waits for `stream`, then reports of the last call that used `workspace`: off_line_units = the units of its gather-sum table that
 * do not lie on the row of their pixel (vertical displacement != 0, or a weight on the row below that is not zero -- a NaN counts;
 * ignored units count), counted only by plans that hold a line member; line_radius_taken = 4 or 8 if the call's gather-sum pass ran
 * as the line member of that radius (DAU_FLAG_DENSE_SPLIT_LINE), 0 if another member did the work.  Either may be NULL. */
DAU_API int dau_conv_gather_line_status(const dau_conv_plan *plan, void *stream, const void *workspace,
                                int32_t *off_line_units, int32_t *line_radius_taken);

/* Waits for `stream`, then reports of the last backward call (dau_conv_backward, dau_conv_backward_param_sums) that used `workspace`:
 * off_line_units = the units of its bare parameter-gradient table that do not lie on the row of their pixel (vertical displacement
 * != 0 or a factor on the row below that is not zero; ignored units count), counted only by plans that hold a line member of the
 * gather-dot; line_radius_taken = 4 or 8 if the call's parameter gradients ran as the line member of that radius
 * (DAU_FLAG_SPLIT_DOT_LINE) in place of the exact gather-dot, 0 if another member did the work.  Either may be NULL. */
DAU_API int dau_conv_dot_line_status(const dau_conv_plan *plan, void *stream, const void *workspace,
                             int32_t *off_line_units, int32_t *line_radius_taken);

/* The same report without waiting, from pinned host memory.  A NaN or an out-of-range offset seen by ANY completed call of
 * this plan since the last report is STICKY: it stays until this function (or dau_conv_check_status) has returned it once,
 * however many good calls completed in between -- plans are shared by all layers of one shape, and a later layer's clean
 * status must not hide an earlier layer's error.  Without such an error: DAU_OK and max|mu| of the most recent completed
 * call (valid_out = 0 when none has completed yet).  A caller that checks this before each call learns of a bad offset
 * at most a few calls late, without ever stalling the stream. */
DAU_API int dau_conv_last_status(const dau_conv_plan *plan, float *max_abs_mu_out, int32_t *valid_out);

/* The prefilter support against the sigma the calls really saw, without waiting, from pinned host memory: planned_out = the plan's k
 * (2*ceil(5*sigma_hint)+1, dau_conv_plan_info.blur_support); needed_out = what the sigma of the most recent call needs by the same
 * rule, computed on the device from the tensor the call was given (0: not a positive finite number; any support beyond 17 reads 19);
 * worst_needed_out = the largest such value ABOVE the plan's k that any call has recorded since this function last returned --
 * sticky, and cleared by this call; 0: none.  A call whose sigma needs more than the plan holds has run with too few taps: make a
 * plan from the new sigma (and capture again if the call was replayed from a graph).  needed_out < planned_out is no error: the
 * wider support is still a correct truncation.  A host that sees a call's status in dau_conv_last_status sees its record here.
 * All three pointers are required (DAU_INVALID_ARGUMENT otherwise); a plan created without a device answers 0, k, 0. */
DAU_API int dau_conv_sigma_status(const dau_conv_plan *plan, int32_t *needed_out, int32_t *planned_out, int32_t *worst_needed_out);

/* Building blocks exposed for parity tests (device pointers in and out).
 * filters_out: 6 planes of k*k floats in the order Gn, Dw, Dmu1, Dmu2, Dsigma, Gerr.
 * unit table: THE table the gather kernels consume, written by the very kernel every forward / backward call runs first
 * (prepare_units_kernel): S*G*F entries of 6 dwords {int32 floor(mu1'), int32 floor(mu2'), float w'*b00, w'*b01, w'*b10,
 * w'*b11} (factor index 2*dy + dx).  form 0: entry order [S][G][F], mu' = mu (forward, and with w = NULL -> w' = 1 the
 * parameter-gradient pass); form 1: entry order [F][G][S], mu' = -mu (the input-gradient pass,
 * base_dau_conv_layer.cu:299-325).  Ignored units have w' = 0. */
DAU_API int dau_conv_filters(const dau_conv_plan *plan, void *stream, const float *sigma, float *filters_out);
DAU_API int dau_conv_unit_table(const dau_conv_plan *plan, void *stream, const float *w, const float *mu1, const float *mu2,
                        int form, void *table_out);

/* Optional per-kernel timing for benchmarks (no reference counterpart; the reference only has the
 * compile-time PROFILE_CUDA block, dau_conv_forward_core.hpp:2506-2563).  Between _begin and _end every
 * dominant kernel launch is bracketed by HIP events on the caller's stream (asynchronous, no host sync).
 * Slots: 0 = gather-sum of dau_conv_forward, 1 = gather-sum of the dx pass, 2 = gather-dot (parameter
 * gradients).  _end waits for the events and returns, per slot, the summed milliseconds of those launches and the
 * number of PASSES they made up (a pass over large offsets takes several window launches).
 * Not thread-safe; one profiling session per plan at a time. */
enum { DAU_PROFILE_SLOTS = 3 };
DAU_API int dau_conv_profile_begin(dau_conv_plan *plan);
DAU_API int dau_conv_profile_end(dau_conv_plan *plan, double *ms_out, int32_t *passes_out);

#ifdef __cplusplus
}
#endif
#endif /* DAU_CONV_H_ */
