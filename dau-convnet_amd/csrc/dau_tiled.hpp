// Interface of the LDS-tiled kernels (DAU_ALGO_TILED).
//   gather-sum (forward y and input gradient dx): MFMA 4x4x1 outer products with
//     tap-separated accumulators over image-pair-interleaved LDS planes  (k_gather_mfma.hip)
//   gather-dot (parameter gradients): lane-per-unit packed-FMA kernel     (k_gather_dot.hip)
#pragma once
#include "dau_common.hpp"

namespace dau {

// Geometry of one gather-sum pass  (in-channels Cin -> out-channels Cout).
struct TiledConfig {
    int N, Cin, Cout, G, H, W;
    int R;            // offset bucket
    int blur_k;       // prefilter support
    int NP;           // image pairs = ceil(N/2)
    int windows;      // gather passes: 1, or 4 offset windows of radius R/2 for buckets 24 and 32 (every unit belongs to
                      // exactly one window; a pass gathers only its own units)
    int stack;        // (image pair, patch) planes gathered per workgroup
    int patches;      // patches per image: big or odd-sized images are gathered patch by patch
    int rows, pitch;  // staged plane of a patch: rows = ph + 2R + 1, pitch (in positions) >= pw + 2R + 1 with pitch % 32 == 8
    int tiles_x, tiles_y;   // position tiles of a patch
    int tile_w;             // their width: 8 (8 x 8 positions) or 32 (32 x 2)
    int fblock;       // out-channels per workgroup
    int variant;      // kernel instantiation id
    int debug;        // DAU_GATHER_DEBUG at plan creation (timing experiments)
    int act;          // storage format of the activations in and out (ActFormat, dau_common.hpp)
    int nhwc;         // DAU_FLAG_IO_NHWC: in and out are [N][H][W][C] arrays (set by the plan after configure; addresses only)
    int in_relu;      // DAU_FLAG_INPUT_RELU (set by the plan after configure, forward direction only): prepare clamps `in` at zero as it loads it
};

bool tiled_gather_configure(int N, int Cin, int Cout, int G, int H, int W, int R, int blur_k, int act, TiledConfig* cfg);
size_t tiled_gather_workspace_bytes(const TiledConfig& cfg);
// prepare: blur `in` ([N,Cin,H,W]) with the Gaussian (`filters` = output of launch_synth_filters; `mirrored`
// selects the flipped kernel of the input-gradient pass) into the staged pair-interleaved planes and pack the
// unit table (`table` is indexed [Cin][G][Cout]).  run: the gather itself, writing `out` ([N,Cout,H,W]).
int tiled_gather_windows(const TiledConfig& cfg);
// one pass per offset window: prepare(window) then run(accumulate = window > 0)
// guard: see dau_common.hpp (every kernel of the pass returns at once unless max|mu| lies in the guard's range)
void tiled_gather_prepare(hipStream_t st, const TiledConfig& cfg, const float* in, const float* filters, bool mirrored,
                          const UnitRef* table, void* workspace, int window, const Guard& guard);
// epi: the store is act(sum + bias[f]) (a call with an epilogue passes it to its LAST window pass only: act(old + sum + bias))
void tiled_gather_run(hipStream_t st, const TiledConfig& cfg, float* out, void* workspace, bool accumulate, const Guard& guard,
                      const Epilogue& epi = Epilogue{});
// once per plan and device, before the first run: raises the kernels' dynamic-LDS limit
void tiled_gather_init(const TiledConfig& cfg);

// Densified bf16 gather-sum (k_dense_bf16.hip; DAU_FLAG_DENSE_BF16, offset bucket 4, bfloat16 activations): the units of
// every (input, output) channel pair scattered into a dense 9 x 9 kernel, implicit GEMM on the bf16 matrix cores.
struct DenseConfig {
    int N, Cin, Cout, G, H, W;
    int R, blur_k;
    int act;          // storage format of the activations in and out (ActFormat; the dense bf16 form requires kActBF16)
    int nsub;         // 8-pixel subtiles per column block = kernel instantiation
    int ftiles;       // 32-channel accumulator tiles per wave (2: four waves per workgroup, 1: eight)
    int nhwc;         // DAU_FLAG_IO_NHWC (the split forms only): in and out are [N][H][W][C] arrays (set by the plan after configure)
    int in_relu;      // DAU_FLAG_INPUT_RELU (the split forms, forward direction only; set by the plan after configure): prepare clamps `in`
                      // at zero as it loads it, the per-image maxima included
};
// The functions exist once per offset radius of the dense form, in the namespaces r4 (|mu| <= 4: 9 x 9 taps) and r3 (|mu| <= 3:
// 7 x 7): the same source compiled twice (Makefile); `R` of configure must be the namespace's radius.
#define DAU_DECLARE_DENSE_GATHER(NS)                                                                                           \
    namespace NS {                                                                                                            \
    bool dense_gather_configure(int N, int Cin, int Cout, int G, int H, int W, int R, int blur_k, int act, DenseConfig* cfg);  \
    size_t dense_gather_workspace_bytes(const DenseConfig& cfg);                                                              \
    void dense_gather_init(const DenseConfig& cfg);                                                                           \
    /* prepare: dense kernel synthesis from the unit table ([Cin][G][Cout]) + blurred bf16 staging of `in`; run: the GEMM */  \
    void dense_gather_prepare(hipStream_t st, const DenseConfig& cfg, const float* in, const float* filters, bool mirrored,   \
                              const UnitRef* table, void* workspace, const Guard& guard);                                     \
    void dense_gather_run(hipStream_t st, const DenseConfig& cfg, float* out, void* workspace, const Guard& guard);           \
    }
DAU_DECLARE_DENSE_GATHER(r4)
DAU_DECLARE_DENSE_GATHER(r3)

// Densified gather-sum at fp32 accuracy (k_dense_split.hip): the same dense form with both operands split into two binary16
// limbs, three f16 MFMAs per tap -- fp32, bf16 or f16 activations, inside the fp32 parity bar; the same source compiled once per
// offset radius (Makefile): namespaces s2, s3, s4 = offsets within +-2, +-3, +-4 (5 x 5, 7 x 7, 9 x 9 taps).
#define DAU_DECLARE_SPLIT_GATHER(NS)                                                                                           \
    namespace NS {                                                                                                            \
    bool split_gather_configure(int N, int Cin, int Cout, int G, int H, int W, int R, int blur_k, int act, DenseConfig* cfg);  \
    size_t split_gather_workspace_bytes(const DenseConfig& cfg);                                                              \
    void split_gather_init(const DenseConfig& cfg);                                                                           \
    void split_gather_prepare(hipStream_t st, const DenseConfig& cfg, const float* in, const float* filters, bool mirrored,   \
                              const UnitRef* table, void* workspace, const Guard& guard);                                     \
    /* epi: the store is act(sum + bias[f]) (dau_conv_forward_epilogue) */                                                  \
    void split_gather_run(hipStream_t st, const DenseConfig& cfg, float* out, void* workspace, const Guard& guard,            \
                          const Epilogue& epi = Epilogue{});                                                                  \
    }
DAU_DECLARE_SPLIT_GATHER(s2)
DAU_DECLARE_SPLIT_GATHER(s3)
DAU_DECLARE_SPLIT_GATHER(s4)
// the line forms (-DDAU_SPLIT_1D): one row of 2 R + 1 taps, R = 4 and 8 (DAU_FLAG_DENSE_SPLIT_LINE)
DAU_DECLARE_SPLIT_GATHER(l4)
DAU_DECLARE_SPLIT_GATHER(l8)

// Radius 3 with outliers (DAU_FLAG_DENSE_SPLIT_OUTLIERS): a call whose offsets reach into (3, 4] in few units runs the radius-3
// GEMM on the corners inside 7 x 7 (split_densify_kernel drops the others) plus a list-driven fp32 pass over the corners on the
// ring |tap| = 4 (k_dense_ring.hip), whose sums the GEMM's epilogue adds before the store.
struct SplitStaged {          // the radius-3 form's staged input, for the ring pass
    const float* sx;          // device, [N]: power-of-two scale of each image's staged limbs
    const _Float16* xs;       // XS[n][chunk][limb][half][Hs][Ws][8]: staged position (r, c) = image (r - 3, c - 3)
    int Hs, Ws, nchunk;
};
namespace s3 {
SplitStaged split_gather_staged(const DenseConfig& cfg, const void* workspace);
// split_gather_run with partial[N][Cout][H][W] (fp32) added to the sums before the store's one rounding (the bias of an epilogue joins
// after that partial sum)
void split_gather_run_add(hipStream_t st, const DenseConfig& cfg, float* out, const float* partial, void* workspace, const Guard& guard,
                          const Epilogue& epi = Epilogue{});
}
struct RingConfig {
    int N, Cin, Cout, G, H, W;
    int nchunk;               // 16-channel chunks of Cin
    int capacity;             // entries the list holds (3 per outlier unit the member's guard admits)
};
void ring_configure(const DenseConfig& dense, long max_outlier_units, RingConfig* cfg);
size_t ring_workspace_bytes(const RingConfig& cfg);
// once per pass: the CSR list of (input channel, ring tap, summed weight) entries per (16-channel chunk, output channel) cell, from the
// pass's unit table ([Cin][G][Cout]) by count -> exclusive scan -> fill (deterministic)
void ring_build_list(hipStream_t st, const RingConfig& cfg, const UnitRef* table, void* workspace, const Guard& guard);
// once per batch slab: partial[n][f][y][x] = sum over the entries e of cell (., f) of w_e * Xb[n, c_e, y + dy_e, x + dx_e], Xb from the
// staged limbs; marks the status block (kRingTakenBit)
void ring_run(hipStream_t st, const RingConfig& cfg, const SplitStaged& staged, void* workspace, Status* status, const Guard& guard);
float* ring_partial(const RingConfig& cfg, void* workspace);
void ring_init();             // once per plan and device: raises the pass's dynamic-LDS limit

struct TiledDotConfig {
    Shape sh;
    int R, blur_k;
    int NP;
    int variant;
    int windows;      // offset windows of radius 8: 1 for R <= 8, 4 for R = 16, 9 for R = 24, 16 for R = 32; with more than
                      // one window the units are binned by window on the device and a window pass visits only its own
    bool as1, one_tile;   // tuning choices read from the environment at plan creation
    bool rw8;             // DAU_DOT_RW=8 at plan creation: 8-column regions only
    bool ring;            // window passes keep the error tile as a ring of rows (k_gather_dot.hip, RING)
    int region_cols, region_rows;   // positions per (item, input channel) sweep: 8 x 8, 8 x 7, 14 x 4 (or 8 x 4 in bucket 18)
    int rounds;           // DAU_DOT_ROUNDS at plan creation: workgroups per CU the chunking aims at (0: default)
    int act;              // storage format of x and dy (ActFormat)
    int ignore;           // number_units_ignore: binned window passes give those units no slot
    int debug;
    int nhwc;             // DAU_FLAG_IO_NHWC: x and dy are [N][H][W][C] arrays (set by the plan after configure)
    int in_relu;          // DAU_FLAG_INPUT_RELU: x is clamped at zero as it is loaded (set by the plan after configure)
};

bool tiled_dot_configure(const Shape& sh, int R, int blur_k, int act, int ignore, TiledDotConfig* cfg);
size_t tiled_dot_workspace_bytes(const TiledDotConfig& cfg);
// r4[k][s][g][f] = sum_{n,p} dy'[n,f,p] * bilinear(x * D_k, p + o);  `filters` = output of launch_synth_filters.
void tiled_dot_prepare(hipStream_t st, const TiledDotConfig& cfg, const float* x, const float* dy,
                       const float* filters, const UnitRef* table_bare, int drop_col, int drop_row, void* workspace,
                       const Guard& guard);
// accumulate: add this batch slab's sums to r4 instead of overwriting it
void tiled_dot_run(hipStream_t st, const TiledDotConfig& cfg, float* r4, void* workspace, const Guard& guard, bool accumulate);
void tiled_dot_init(const TiledDotConfig& cfg);

// The four derivative-filtered copies of x, staged position-major (k_gather_dot.hip): x[N,C,H,W] -> xk[NP][cstride][Hp][Wp][4][2].
// kmax (optional, [cstride][4 kinds] float bits, zeroed by the caller): max |value| per (channel, kind) over the finite values,
// taken while they are written (a kernel instantiation of its own: callers that pass none run the plain one)
// in_relu: x is clamped at zero as it is widened (DAU_FLAG_INPUT_RELU; a kernel argument, the same instantiations)
void launch_blur4_pack(hipStream_t st, const float* x, const float* filters, int N, int C, int cstride, int H, int W, int Hp,
                       int Wp, int blur_k, int act, float* xk, const Guard& guard, unsigned* kmax = nullptr, bool nhwc = false,
                       bool in_relu = false);
void blur4_pack_init(int blur_k, bool kmax = false, bool nhwc = false);
bool blur4_pack_fits(int blur_k, int Hp, int Wp);

// r4[k][u] = sum over the slabs of partial[slab][k][u] in double (the gather-dot's deterministic reduction, k_gather_dot.hip)
void launch_dot_reduce(hipStream_t st, const void* partial, int partial_f32, long n, int G, int F, int g_split, int slabs0,
                       int slabs1, int zero_from, bool accumulate, float* r4, const Guard& guard);

// Parameter gradients at fp32 accuracy on the f16 matrix cores (k_split_dot.hip): per input channel a GEMM with the four kinds x
// four bilinear corners as rows, the units as columns and (position, image) as K, both operands split into two binary16 limbs.
// Offsets within +-4, interpolation on; the whole batch in one pass.  fp32 and f16 activations: both operands in two limbs, three
// products.  bf16 activations: a bf16 dy times its channel's power-of-two scale is its own hi limb, so the error is staged in
// ONE limb (ES1, half the bytes) and a tile takes two products per K step (sd_e1_dot_kernel); Xk keeps two limbs.
struct SplitDotConfig {
    Shape sh;
    int blur_k;
    int RW;               // region columns = K steps per item (10 or 12: the ring of error-window rows fills the LDS at 12)
    int act;              // storage format of x and dy (ActFormat)
    int e_limbs;          // binary16 limbs of the staged error: 2, or 1 for bf16 activations
    int nhwc;             // DAU_FLAG_IO_NHWC: x and dy are [N][H][W][C] arrays (set by the plan after configure)
    int in_relu;          // DAU_FLAG_INPUT_RELU: x is clamped at zero as it is loaded (set by the plan after configure)
};
bool split_dot_configure(const Shape& sh, int blur_k, int act, SplitDotConfig* cfg);
size_t split_dot_workspace_bytes(const SplitDotConfig& cfg);
// the regions (items) of one column strip and the K steps the main kernel runs for them: RW per item, ceil(RW / 4) for a strip's
// last item where it holds a single real row ((H + 1) % 4 == 1)
void split_dot_strip(const SplitDotConfig& cfg, int* items, int* k_steps);
void split_dot_init(const SplitDotConfig& cfg);
// prepare: fp32 derivative filtering (blur4_pack), per-channel maxima, limb staging of Xk and of the error; run: the GEMM + the
// reduction into r4 (all four kinds; x, dy fp32 or f16 NCHW; table = bare unit table [S][G][F])
void split_dot_prepare(hipStream_t st, const SplitDotConfig& cfg, const float* x, const float* dy, const float* filters,
                       int drop_col, int drop_row, void* workspace, const Guard& guard);
void split_dot_run(hipStream_t st, const SplitDotConfig& cfg, const UnitRef* table, float* r4, void* workspace, const Guard& guard);
// The line forms (-DDAU_SD_1D: namespaces d4 and d8; DAU_FLAG_SPLIT_DOT_LINE): the same source compiled with a horizontal radius
// of 4 / 8 and a vertical radius of 0, for calls whose units all lie on the row of their pixel -- the parameter gradients of
// single-dimension layers.  The kind mu2 is computed and discarded.  The dy maxima kernel of a form whose guard has passed writes
// the form's radius to Status::dot_line_radius.
#define DAU_DECLARE_SPLIT_DOT_LINE(NS)                                                                                         \
    namespace NS {                                                                                                            \
    bool split_dot_configure(const Shape& sh, int blur_k, int act, SplitDotConfig* cfg);                                      \
    size_t split_dot_workspace_bytes(const SplitDotConfig& cfg);                                                              \
    void split_dot_strip(const SplitDotConfig& cfg, int* items, int* k_steps);                                                \
    void split_dot_init(const SplitDotConfig& cfg);                                                                           \
    void split_dot_prepare(hipStream_t st, const SplitDotConfig& cfg, const float* x, const float* dy, const float* filters,  \
                           int drop_col, int drop_row, void* workspace, const Guard& guard);                                  \
    void split_dot_run(hipStream_t st, const SplitDotConfig& cfg, const UnitRef* table, float* r4, void* workspace,           \
                       const Guard& guard);                                                                                   \
    }
DAU_DECLARE_SPLIT_DOT_LINE(d4)
DAU_DECLARE_SPLIT_DOT_LINE(d8)

// Densified parameter gradients on the bf16 matrix cores (k_dense_wgrad.hip; DAU_FLAG_DENSE_BF16, bucket 4, bfloat16
// activations, three or more units): C_k[d][s][f] = sum_{n,q} Xk[n,s,q+d] * E'[n,f,q] for the 9 x 9 displacements d as a GEMM
// with K = (image, position), then r_k[u] = sum_taps b_t(u) * C_k[o_u + t].
struct WgradConfig {
    Shape sh;
    int blur_k;
    int SB, FB, NC;       // 32-channel blocks of S and F, 16-image chunks of N
    int HsT, WsT, WT, nseg;   // staged Xk plane (H+8 rows, nseg*WT+8 columns rounded up to 8); a row is walked in nseg segments of WT
                          // columns (an instantiated length)
    int splits;           // the image chunks are cut into `splits` ranges (partial sums per range)
    int Hp, Wp;           // plane of the intermediate fp32 copy (blur4_pack)
    bool fused;           // XkT is written from x through the transposed bf16 copy (instantiated prefilter supports); else
                          // through the fp32 copy of blur4_pack
};
// (once per radius, as the dense gather-sum: namespaces r4 and r3)
// r4[k][s][g][f] = raw parameter-gradient sums; x, dy bfloat16 NCHW; table = bare unit table [S][G][F].  nk: kinds computed (w, mu1,
// mu2, sigma in this order): 3 leaves the sigma block of r4 untouched (a caller that does not want dsigma; the reference's
// last_k_optional: base_dau_conv_layer.hpp:213, src/dau_conv/dau_conv_impl/dau_conv_backward.cpp:219)
#define DAU_DECLARE_DENSE_WGRAD(NS)                                                                                            \
    namespace NS {                                                                                                            \
    bool dense_wgrad_configure(const Shape& sh, int blur_k, bool bf16, WgradConfig* cfg);                                     \
    size_t dense_wgrad_workspace_bytes(const WgradConfig& cfg);                                                               \
    void dense_wgrad_init(const WgradConfig& cfg);                                                                            \
    void dense_wgrad_run(hipStream_t st, const WgradConfig& cfg, const float* x, const float* dy, const float* filters,       \
                         const UnitRef* table, int drop_col, int drop_row, float* r4, void* workspace, const Guard& guard, int nk); \
    }
DAU_DECLARE_DENSE_WGRAD(r4)
DAU_DECLARE_DENSE_WGRAD(r3)

// Backward of the fused epilogue (k_epilogue_grad.hip): dz = (y <= 0) ? 0 : dy in the activations' format and layout (relu only;
// dz may be dy), dbias[f] = sum of dz over n, h, w in fp32 (may be null) through partial sums in `workspace`, reduced in a fixed order.
// x-like arguments: dy, y, dz are [N][F][H][W] (nhwc: [N][H][W][F]) arrays of format `act`.  false: a grid beyond 2^31 workgroups.
size_t epilogue_grad_workspace_bytes(long N, int F, int H, int W, int act, bool nhwc);
bool epilogue_grad_run(hipStream_t st, long N, int F, int H, int W, int act, bool nhwc, const float* dy, const float* y, bool relu,
                       float* dz, float* dbias, void* workspace);

}  // namespace dau
