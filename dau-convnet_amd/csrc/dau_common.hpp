// Shared declarations of the HIP implementation behind include/dau_conv.h.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cmath>
#include <cstdint>
#include <type_traits>
#include "dau_conv.h"

// Tuning knobs.  The shipped library's behaviour is fully determined by dau_conv_desc (plus DAU_WORKSPACE_BUDGET_GB): the
// environment variables that pin a kernel variant, a chunking or a staging tile for same-box A/B runs and for the variant
// tests exist only in the TUNING build (-DDAU_TUNING: libdau_conv_hip_tuning.so, `make tuning`), where these macros read the
// environment at plan creation.  In the release build they are their defaults and the names are not in the binary
// (tests/test_capi_symbols.py checks that).
#ifdef DAU_TUNING
#include <cstdlib>
#define DAU_TUNE_INT(name, dflt) (getenv(name) ? atoi(getenv(name)) : (dflt))
#define DAU_TUNE_SET(name) (getenv(name) != nullptr)
#else
#define DAU_TUNE_INT(name, dflt) (dflt)
#define DAU_TUNE_SET(name) (false)
#endif

namespace dau {

// Storage format of the activations (x, y, dy, dx) behind the float* of the ABI: fp32, bfloat16 (DAU_FLAG_IO_BF16: the upper
// 16 bits of an fp32) or IEEE binary16 (DAU_FLAG_IO_F16).  The arithmetic is fp32 for all three; only loads and stores differ.
enum ActFormat : int { kActF32 = 0, kActBF16 = 1, kActF16 = 2 };
__device__ __forceinline__ float f16_bits_to_float(unsigned bits) {      // v_cvt_f32_f16 (subnormals, Inf and NaN widen exactly)
    return (float)__builtin_bit_cast(_Float16, (unsigned short)bits);
}
__device__ __forceinline__ float load_act(const float* base, long idx, int act) {
    if (act == kActF32) return base[idx];
    const unsigned b = reinterpret_cast<const unsigned short*>(base)[idx];
    return act == kActF16 ? f16_bits_to_float(b) : __uint_as_float(b << 16);
}
// the stored bits of an activation, untouched (no arithmetic on a value still in flight), and their conversion
struct F16Bits { unsigned bits; };                            // an f16 activation, zero-extended by the load
template <int A> struct RawAct { typedef float type; };
template <> struct RawAct<kActBF16> { typedef unsigned type; };   // (zero-extended by the load; a 16-bit pair would be packed = arithmetic)
template <> struct RawAct<kActF16> { typedef F16Bits type; };
template <int A>
__device__ __forceinline__ typename RawAct<A>::type load_raw(const float* base, long idx) {
    if constexpr (A == kActF32) return base[idx];
    else if constexpr (A == kActBF16) return reinterpret_cast<const unsigned short*>(base)[idx];
    else return F16Bits{reinterpret_cast<const unsigned short*>(base)[idx]};
}
__device__ __forceinline__ float act_of(float v) { return v; }
__device__ __forceinline__ float act_of(unsigned v) { return __uint_as_float(v << 16); }
__device__ __forceinline__ float act_of(F16Bits v) { return f16_bits_to_float(v.bits); }
template <int A>
__device__ __forceinline__ float load_act_t(const float* base, long idx) { return act_of(load_raw<A>(base, idx)); }
// f(std::integral_constant<int, A>) for the run-time format `act` (staging kernels: one instantiation of the body per format)
template <class F>
__device__ __forceinline__ void with_act(int act, F&& f) {
    if (act == kActBF16) f(std::integral_constant<int, kActBF16>{});
    else if (act == kActF16) f(std::integral_constant<int, kActF16>{});
    else f(std::integral_constant<int, kActF32>{});
}
// DAU_FLAG_IO_NHWC: the user's activations are [N][H][W][C] arrays.  Every kernel that loads x / dy or stores y / dx has NHWC
// instantiations of its own; only the addresses differ, the arithmetic and the order of every sum are the NCHW instantiation's.
// The NCHW instantiations must stay the code -- and the symbols -- they were, so a kernel template takes no new argument for it: an
// NHWC instantiation is the template with kNhwcArg or'ed into its FIRST int argument (blur_pack_kernel<7 | kNhwcArg>), the gather-sum
// with its traits wrapped in NhwcOut<>.  (A common body inlined into two kernels was tried first: it changed the code of the NCHW ones.)
// blur4_pack_kernel, whose instantiations the tests count by name, is one text compiled under two names (k_blur4_pack_body.hpp); the
// small kernels that are no templates (pack_error, sd_stage_e / _e1, sd_absmax_e) have NHWC kernels written for that layout.
constexpr int kNhwcArg = 0x100;
template <class T> struct NhwcOut : T {};
template <class T> struct IsNhwcOut : std::false_type {};
template <class T> struct IsNhwcOut<NhwcOut<T>> : std::true_type {};
// The fused epilogue of a gather-sum's store (dau_conv_forward_epilogue / _residual): y = act((sum + bias[f]) + r[n,f,h,w]), act the
// identity or ReLU, in fp32 before the store's one rounding.  Like the NHWC instantiations these are kernels of their own, marked the same way -- kEpiArg or'ed
// into the template's first int argument, the gather-sum's traits wrapped in EpiOut<> -- so that a call without an epilogue runs the
// kernels it ran before.  One instantiation serves bias, residual, ReLU and their combinations: which of them apply is a kernel argument.
constexpr int kEpiArg = 0x200;
template <class T> struct EpiOut : T {};
template <class T> struct IsEpiOut : std::false_type {};
template <class T> struct IsEpiOut<EpiOut<T>> : std::true_type {};
template <class T> struct IsNhwcOut<EpiOut<T>> : IsNhwcOut<T> {};
struct Epilogue {
    const float* bias = nullptr;     // [Cout] fp32, or none
    bool relu = false;
    // dau_conv_forward_residual: an array of y's shape, format and layout, added after the bias and before the activation -- or none.
    // Read only, never y itself.  A run-time pointer inside the same instantiations: one wave-uniform branch per store.
    const float* residual = nullptr;
    // DAU_FLAG_INPUT_RELU, the dx pass: the layer's raw x -- out's shape, format and layout -- or none.  The store becomes
    // (gate[o] <= 0) ? 0 : v, the rule of a threshold at zero (a NaN gate passes v through), after everything above and before the
    // store's one rounding.  Like the residual a run-time pointer inside the same instantiations, read after the tap loop.
    const float* gate = nullptr;
    bool on() const { return bias != nullptr || relu || residual != nullptr || gate != nullptr; }
};
// the gate of a store: v where the gate's element is > 0 or a NaN, +0 elsewhere
__device__ __forceinline__ float gate_value(float v, float g) { return g <= 0.0f ? 0.0f : v; }
// act((v + b) + r) of the value v the kernel would have stored.  Each add is an fp32 add of THAT value: the empty asm in front keeps a
// multiply that produced v from being contracted into it, the one behind keeps the add out of a 16-bit store's conversion
// (v_fma_mixlo_f16 rounds the exact sum once; the unfused form rounds the fp32 sum).  The order is fixed, bias first and residual
// second: for float32 the bits of relu((y + bias) + r).  ReLU as torch.relu: a NaN stays a NaN.
__device__ __forceinline__ float epilogue_value(float v, float b, bool has_bias, bool relu, float r = 0.0f, bool has_res = false) {
    asm("" : "+v"(v));
    if (has_bias) v = v + b;
    asm("" : "+v"(v));
    if (has_res) v = v + r;
    asm("" : "+v"(v));
    return (relu && v <= 0.0f) ? 0.0f : v;
}
// element index of (n, c, y, x) in an [N][H][W][C] array
__device__ __forceinline__ long nhwc_index(long n, int c, int y, int x, int C, int H, int W) { return ((n * H + y) * W + x) * C + c; }
// Workgroups b and b + 8 run on the same XCD and share its L2: the logical id under which every XCD takes a contiguous range of
// ids.  The NHWC staging kernels whose workgroups own ONE channel give consecutive ids to the channels of a window, so that the
// 128-byte lines their strided loads share are fetched into one L2.
__device__ __forceinline__ int xcd_contiguous_id(int b, int nblk) {
    const int xcd = b % 8, idx = b / 8, per = nblk / 8, rem = nblk % 8;
    return (xcd < rem ? xcd * (per + 1) : rem * (per + 1) + (xcd - rem) * per) + idx;
}
// v where keep, +0 elsewhere, as a bit mask: with a select hipcc moves the load that produced v under a branch on `keep`
// DAU_FLAG_INPUT_RELU: the ReLU in front of the layer, applied where a staging kernel widens the x it has loaded: (v <= 0) ? +0 : v, so
// a NaN stays a NaN and -0 becomes +0.  `on` is a kernel argument (wave-uniform): the same kernels stage dy for the dx pass, unclamped.
// A select on the loaded value, no branch around the load.
__device__ __forceinline__ float relu_in(float v, bool on) { return (on && v <= 0.0f) ? 0.0f : v; }
__device__ __forceinline__ float mask_act(float v, bool keep) { return __uint_as_float(__float_as_uint(v) & (keep ? 0xffffffffu : 0u)); }
// Load phase of the staging kernels: rows_ x cols_ items of one plane split over the nw waves of its wave group, the loads of
// kLoadBatch items issued back to back before the first of them is stored to LDS.  These kernels are HBM bound, and a wave with
// one or two loads in flight keeps far fewer bytes in the air than the memory latency needs (Little's law: ~50 KB per CU).
// ld(r, x) -> value must be BRANCH FREE (clamped address + select): a branch around a load makes hipcc wait for it at the
// join, one load at a time.  It returns the loaded bits untouched (RawAct / load_raw); st converts and masks them.  Items past the end load item (rows_-1, cols_-1) again and store nothing.  st(r, x, value).
// A wave per row when the rows are wide, a flat index when they are narrow.
#ifndef DAU_LOAD_BATCH
#define DAU_LOAD_BATCH 6
#endif
constexpr int kLoadBatch = DAU_LOAD_BATCH;
template <class V, class Load, class Store>
__device__ __forceinline__ void load_phase(int rows_, int cols_, int wave, int nw, int lane, Load&& ld, Store&& st) {
    if (cols_ >= 56) {
        for (int x0 = 0; x0 < cols_; x0 += 64) {
            const int x = x0 + lane, xc = x < cols_ ? x : cols_ - 1;
            for (int r0 = wave; r0 < rows_; r0 += nw * kLoadBatch) {
                V v[kLoadBatch];
#pragma unroll
                for (int u = 0; u < kLoadBatch; ++u) { const int r = r0 + u * nw; v[u] = ld(r < rows_ ? r : rows_ - 1, xc); }
#pragma unroll
                for (int u = 0; u < kLoadBatch; ++u) { const int r = r0 + u * nw; if (r < rows_ && x < cols_) st(r, x, v[u]); }
            }
        }
    } else {
        const int total = rows_ * cols_;
        for (int t0 = wave * 64 + lane; t0 < total; t0 += nw * 64 * kLoadBatch) {
            V v[kLoadBatch];
            int rr[kLoadBatch];
#pragma unroll
            for (int u = 0; u < kLoadBatch; ++u) {
                const int t = t0 + u * nw * 64, tc = t < total ? t : total - 1;
                rr[u] = tc / cols_;
                v[u] = ld(rr[u], tc - rr[u] * cols_);
            }
#pragma unroll
            for (int u = 0; u < kLoadBatch; ++u) { const int t = t0 + u * nw * 64; if (t < total) st(rr[u], t - rr[u] * cols_, v[u]); }
        }
    }
}
__device__ __forceinline__ void store_act(float* base, long idx, float v, bool bf16, bool accumulate) {
    if (!bf16) { base[idx] = accumulate ? base[idx] + v : v; return; }
    unsigned short* p = reinterpret_cast<unsigned short*>(base) + idx;
    if (accumulate) v += __uint_as_float((unsigned)*p << 16);
    unsigned u = __float_as_uint(v);
    // round to nearest even on the bits; a NaN must stay a NaN (the rounding add can carry a NaN payload into the sign /
    // exponent: 0xFFFFFFFF -> +0, 0x7F800001 -> +inf), so it is stored as the quiet NaN pattern instead
    u = (v != v) ? 0x7fc00000u : u + 0x7fffu + ((u >> 16) & 1u);
    *p = (unsigned short)(u >> 16);
}
// the bfloat16 bits store_act writes for v (round to nearest even, a NaN as the quiet NaN pattern): for stores of several values at once
__device__ __forceinline__ unsigned bf16_bits(float v) {
    const unsigned u = __float_as_uint(v);
    return ((v != v) ? 0x7fc00000u : u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
// binary16: v_cvt_f16_f32 -- round to nearest even, f16 subnormals kept, beyond the largest finite value +-inf, a NaN stays a
// NaN (the IEEE conversion, as torch.Tensor.half()); a window pass re-reads the stored value, adds and rounds once more
__device__ __forceinline__ void store_act_f16(float* base, long idx, float v, bool accumulate) {
    unsigned short* p = reinterpret_cast<unsigned short*>(base) + idx;
    if (accumulate) v += f16_bits_to_float(*p);
    *p = __builtin_bit_cast(unsigned short, (_Float16)v);
}
template <int A>
__device__ __forceinline__ void store_act_t(float* base, long idx, float v, bool accumulate) {
    if constexpr (A == kActF16) store_act_f16(base, idx, v, accumulate);
    else store_act(base, idx, v, A == kActBF16, accumulate);
}
// run-time format (epilogues of kernels whose instantiations serve all three)
__device__ __forceinline__ void store_act(float* base, long idx, float v, int act, bool accumulate) {
    if (act == kActF16) store_act_f16(base, idx, v, accumulate);
    else store_act(base, idx, v, act == kActBF16, accumulate);
}


constexpr int kMaxBlurSupport = 17;                       // convolve.cu:40 caps the prefilter at 17x17
constexpr int kFilterPlane = kMaxBlurSupport * kMaxBlurSupport;
constexpr int kNumK = 4;                                  // gradient kinds {w, mu1, mu2, sigma}
// The prefilters are separable: Gn = gx (x) gy, Dmu1 = ax (x) gy, Dmu2 = gx (x) ay, Dsigma = cx (x) gy + gx (x) by
// (SURVEY.md Appendix A item 1 rewritten with 1-D factors).  synth_filters_kernel also emits these taps, after
// the six 2-D planes: eight arrays of kTapPitch floats.
constexpr int kTapPitch = 32;
enum Tap1d { kTapGX = 0, kTapGY, kTapAX, kTapAY, kTapCX, kTapBY, kTapGXR, kTapGYR, kNumTap1d };
constexpr int kTaps1dOffset = 6 * kFilterPlane;
constexpr int kFilterFloats = kTaps1dOffset + kNumTap1d * kTapPitch;

// Device-side status block at the head of every workspace (see dau_conv_check_status).
struct Status {
    unsigned int max_abs_mu_bits;  // float bits of max(|mu1|,|mu2|); valid because |x| bits order like uints
    unsigned int nan_seen;
    unsigned int ticket;           // ticket counter of prepare_units_kernel's workgroups
    // bits 0..30 the live units with max(|mu1|,|mu2|) > 3 ("outlier units", counted by prepare_units_kernel), bit 31
    // (kRingTakenBit) set by the ring pass of a call whose gather-sum ran as the radius-3 GEMM plus ring (k_dense_ring.hip;
    // dau_conv_gather_outlier_status reports both)
    unsigned int outlier_units;
    // DAU_FLAG_DENSE_SPLIT_LINE.  off_line_units: the units of the call's gather-sum table that do NOT lie on the row of their pixel
    // (oy != 0 or a weight on the row below that is not zero -- a NaN counts; ignored units count too), counted by
    // prepare_units_kernel.  line_radius: the radius of the line member that ran the pass (written by its scales kernel), 0 if none did.
    unsigned int off_line_units, line_radius;
    // DAU_FLAG_SPLIT_DOT_LINE (dau_conv_dot_line_status).  dot_off_line_units: the units of the call's bare parameter-gradient table
    // that do not lie on the row of their pixel, counted by the prepare_units_kernel of that pass -- which counts them into
    // off_line_units too, where the guards read the count; the pass puts off_line_units back to zero behind itself, so that after
    // a backward call off_line_units is the count of the input-gradient table alone.  dot_line_radius: the radius of the line
    // member of the gather-dot that ran the pass (written by its dy maxima kernel), 0 if none did.
    unsigned int dot_off_line_units, dot_line_radius;
};
constexpr unsigned kRingTakenBit = 0x80000000u;
// synth_filters_kernel clears the block by word count, run_param_sums clears one word of it, and the queries read a copy of it
static_assert(sizeof(Status) == 32, "the status block is eight words");
static_assert(offsetof(Status, max_abs_mu_bits) == 0 && offsetof(Status, nan_seen) == 4 && offsetof(Status, ticket) == 8 &&
              offsetof(Status, outlier_units) == 12 && offsetof(Status, off_line_units) == 16 && offsetof(Status, line_radius) == 20 &&
              offsetof(Status, dot_off_line_units) == 24 && offsetof(Status, dot_line_radius) == 28,
              "the status block keeps the order of its words");

// Pinned host mirror of a plan (written by the last workgroup of prepare_units_kernel, read by dau_conv_last_status and as
// the next call's offset-bucket hint): the most recent completed call's status, and the sticky record of bad ones.
// sigma_needed / sigma_worst (written by synth_filters_kernel, read by dau_conv_sigma_status): the prefilter support the most recent
// call's sigma needs (0: not a positive finite number; 19: more than 17 taps), and the largest such support beyond the plan's own
// since the host last asked (sticky; 0: none).
struct HostStatus {
    unsigned int max_abs_mu_bits, nan_seen, valid, sigma_needed;      // most recent completed call
    unsigned int bad_max_abs_mu_bits, bad_nan_seen, sigma_worst, pad1;  // worst status since the host last reported one (sticky)
};
static_assert(sizeof(HostStatus) == 32, "the pinned status mirror is 32 bytes (include/dau_conv.h, Ownership)");

// Offset-bucket guard of a launch.  The bucket a call needs depends on max|mu|, which only the device knows when the
// kernels are enqueued (prepare_units_kernel leaves it in the status block).  The host enqueues the kernel sets of up to
// two candidate buckets; every kernel of a set starts with guard_pass() and returns at once unless the actual max|mu|
// falls into (lo, hi] -- exactly one set does the work, without a device->host sync (the reference blocks on a D2H copy
// of the amax for this, dau_conv_op.cpp:229-253).  status == nullptr: unguarded.
// A guard may also ask for the call's outlier-unit count (Status::outlier_units) to lie in [cnt_lo, cnt_hi] while max|mu| <= cnt_upto
// (the default range means "any"): the radius-3 + ring member runs below a count limit, the members that share its offset range
// above it.
struct Guard {
    const Status* status;
    float lo, hi;
    unsigned cnt_lo = 0u, cnt_hi = 0xffffffffu;
    float cnt_upto = INFINITY;
    // DAU_FLAG_DENSE_SPLIT_LINE, DAU_FLAG_SPLIT_DOT_LINE (Status::off_line_units, the units off the line of the pass's table).  +R: a line member, runs only where that count is 0.
    // -R: a member that shares offsets within +-R with a line member, runs there only where the count is not 0.  0: any.
    // Kernels only READ the status block through their guard, with one exception: the scales kernel of a line member whose guard
    // has passed writes its radius to Status::line_radius (k_dense_split.hip, split_scales_kernel under DAU_SPLIT_1D).
    int line = 0;
};
__device__ __forceinline__ bool guard_pass(const Guard& g) {
    if (!g.status) return true;
    const float mx = __uint_as_float(g.status->max_abs_mu_bits);
    const unsigned cnt = g.status->outlier_units & ~kRingTakenBit;
    if (!(mx > g.lo && mx <= g.hi && (mx > g.cnt_upto || (cnt >= g.cnt_lo && cnt <= g.cnt_hi)))) return false;
    if (g.line == 0) return true;
    const bool on_line = g.status->off_line_units == 0u;
    return g.line > 0 ? on_line : (mx > (float)-g.line || !on_line);
}

// One prepared unit for the gather kernels: integer displacement and the four
// bilinear weights already multiplied by w (dau_conv_forward_core.hpp:2155-2213).
struct UnitRef {
    int ox, oy;
    float w00, w01, w10, w11;
};

struct Shape {
    int N, S, F, G, H, W;
};

// ---- launchers implemented in the kernel TUs --------------------------------------
// k_filters.hip
// host_status (may be null): the plan's pinned mirror, which takes the support this call's sigma needs
// status (may be null): the call's status block, which the kernel clears for the prepare_units_kernel behind it
void launch_synth_filters(hipStream_t st, const float* sigma_dev, int k, int flags, float* filters6, HostStatus* host_status = nullptr,
                          Status* status = nullptr);
void launch_synth_filters_compact(hipStream_t st, const float* sigma_dev, int k, int flags, float* planes6);
// k_units.hip
// host_status (may be null): pinned host copy of the status block, written by the last workgroup to finish
// count_ignore: the units left out of the status block's outlier count (-1: `ignore`; the input-gradient table ignores no unit)
// line_status (may be null; DAU_FLAG_DENSE_SPLIT_LINE / DAU_FLAG_SPLIT_DOT_LINE): the status block whose off_line_units takes the count of this
// table's units off the line; line_dot: the table of the parameter-gradient pass, whose count goes to dot_off_line_units as well
void launch_prepare_units(hipStream_t st, const float* w, const float* mu1, const float* mu2, Shape sh,
                          int ignore, int flags, int bucket, bool transposed_negated, UnitRef* table,
                          Status* status, HostStatus* host_status, int count_ignore = -1, Status* line_status = nullptr,
                          bool line_dot = false);
void launch_finalize_grads(hipStream_t st, const float* r4, const float* w, Shape sh, int ignore, float lr,
                           int need_mask, bool single_dim, float* dw, float* dmu1, float* dmu2, float* dsigma);
// `bytes` (a multiple of four) at p set to zero by a kernel: what the passes clear in their workspace, in stream order also in a
// replayed graph (where a memset node was seen to land among the kernels behind it)
void launch_zero_words(hipStream_t st, void* p, size_t bytes);
// k_direct.hip  (DAU_ALGO_DIRECT: plain kernels, any shape)
void launch_blur_direct(hipStream_t st, const float* x, long planes, int H, int W, const float* filters,
                        int nfilt, int k, float* out);
void launch_gather_sum_direct(hipStream_t st, const float* xb, const UnitRef* table, int N, int Sin, int Fout,
                              int G, int H, int W, float* y);
void launch_gather_dot_direct(hipStream_t st, const float* xk4, const float* err, const UnitRef* table, Shape sh,
                              int drop_col, int drop_row, float* r4);

}  // namespace dau
