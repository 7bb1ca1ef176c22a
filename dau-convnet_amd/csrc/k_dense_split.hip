// Densified gather-sum at fp32 accuracy on the f16 matrix cores: two-limb ("split") operands.
//
//   out[n,f,y,x] = sum_{c} sum_{ty,tx < K} Wd[f][c][ty][tx] * Xb[n,c, y+ty-R, x+tx-R]          (K = 2R+1, offsets within +-R)
//
// is the dense form of k_dense_bf16.hip -- the G units of every (input channel, output channel) pair scattered into one K x K
// kernel, the pass an implicit GEMM  M = output channels, N = pixels, K = input channels x taps -- but with both operands kept
// to fp32 accuracy: every fp32 value v (blurred activation, dense tap) is scaled by a power of two and split into two
// binary16 limbs  hi = f16(v), lo = f16(v - hi)  (22 significant bits together), and the product is accumulated as
//      hi_w * hi_x  +  lo_w * hi_x  +  hi_w * lo_x          (the dropped lo * lo term is 2^-22 of the product)
// -- three v_mfma_f32_32x32x16_f16 per tap and 16 input channels, products exact, fp32 accumulation.  At radius 3 that is
// 3 * 49 / 16 = 9.2 fp32-rate MACs per (pixel, channel pair) against the 4 G = 16 of the exact gather at four units
// (k_gather_mfma.hip, v_mfma_f32_4x4x1 at the fp32 vector rate), inside the SAME parity bar (1e-4 relative + 1e-6 of the
// max-norm against the oracle: tests/test_gpu_dense_split.py records the margins).  It replaces the same reference code as
// the gather: DAUConv_forward_pipeline_kernel + interleave_input_data_kernel + perpare_weights_and_offsets
// (include/dau_conv/dau_conv_impl/dau_conv_forward_core.hpp:804-1605, 1607-1732, 1858-2215) and caffe_gpu_convolve2
// (src/dau_conv/util/convolve.cu:48-131), for calls whose offsets lie within +-R (the call's device guard decides).
//
// Power-of-two scales (binary16 has five exponent bits): sx[n] brings the largest finite |x| of IMAGE n to [2^13, 2^14), sw the
// bound G * max|w| of a dense tap (finite units) likewise; both come from a two-launch max reduction over the pass's input and its
// unit table, the epilogue multiplies by 1 / sw and then by 1 / sx[n].  Scaling by a power of two is exact, so the only effect is
// that the limbs cannot overflow and that values down to 2^-17 of their image's maximum keep all 22 bits (smaller ones: an
// absolute error below 2^-39 of that maximum).  One scale per image, not per call: y[n] (dx[n]) is a function of image n and the
// parameters alone -- the same bits whatever its batch-mates hold and however the batch is cut into slabs -- and a non-finite
// element (left out of the maxima; it passes through the arithmetic) reaches only the outputs of its own image that its taps touch.
//
// Layouts (HBM, all in the pass's workspace):
//   header      SplitScales (sw, 1 / sw), sx[N], 1 / sx[N], the partial maxima of the reduction
//   XS[n][chunk][limb][half][Hs][Ws][8]  f16: Gaussian-blurred, scaled input; 16 input channels per chunk as two halves of 8
//       (one 16-byte unit per position = the B fragment of one lane), limb 0 = hi, 1 = lo; staged position (r, c) = image
//       (r-R, c-R), zero outside the image.
//   WS[chunk][tap][limb][CoutP][16]      f16: the dense kernel (A fragments of the two lane halves).
// Workgroup = 128 output channels x 8 rows x NSUB*8 columns as 8 waves = 4 (32 channels) x 2 (4 rows), two per SIMD; a wave
// owns NSUB <= 4 tiles.  Per chunk the window of the four (limb, half) planes is copied into LDS by global_load_lds
// (double buffered, no registers); per tap a wave reads NSUB hi and NSUB lo B fragments (ds_read_b128) and two A fragments
// (global memory, two taps ahead) and issues 3 * NSUB MFMAs.
//
// Accumulation is hierarchical.  v_mfma_f32_32x32x16_f16 aligns its sixteen products to the accumulator's exponent and drops
// what falls more than about two bits below its last place (tools/microbench/mfma_f16_accum: sixteen products of 1/16 ulp each
// vanish), so a long chain through one accumulator loses bits of the RUNNING SUM with every instruction: 2352 chained MFMAs at
// S = 256 measured 3.9e-6 of the max-norm against the oracle, four times the exact gather.  So a tile has TWO accumulators:
// kFlushRows rows of taps (4 x 21 MFMAs) are chained into `part`, and `part` is added to the tile's running sum by v_pk_add_f32
// (round to nearest).  Both ends lose: every external add costs half an ulp of the running sum, every chained MFMA an ulp of the
// chain -- measured max error / max-norm of y at S = F = 256 (and at S = F = 512, 28 x 28) per chain length:
//   3 MFMAs 1.5e-6 (2.5e-6), 9: 8.7e-7 (1.3e-6), 21 (one row): 5.8e-7 (7.9e-7), 42: 4.3e-7 (5.9e-7), 84: 4.0e-7 (4.5e-7),
//   147 (one chunk): 5.1e-7 (4.9e-7), 294: 8.3e-7 (6.4e-7)                        -- profiles/r4_ab_split_chain_length.txt
// at the same speed.  Two accumulators of 16 registers per tile is why a wave owns at most four tiles (a 56-pixel row is a block of
// four and a block of three).
//
// Radius 3 runs the same GEMM on v_mfma_f32_16x16x32_f16, one instruction per tap of a PAIR of chunks (kK32 below; the fragment
// mapping stands at the loop in split_gather_kernel): the staged layouts, the bytes, the LDS reads and the matrix-pipe cycles are
// those of the 32x32x16 loop, a chain of kFlushRows rows of taps holds the products of two chunks.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "dau_tiled.hpp"

#ifndef DAU_SPLIT_R
#define DAU_SPLIT_R 3
#endif
#ifndef DAU_SPLIT_NS
#define DAU_SPLIT_NS s3
#endif

namespace dau {
namespace DAU_SPLIT_NS {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef __attribute__((address_space(1))) const void* glb_ptr_t;

namespace {

constexpr int kDR = DAU_SPLIT_R;        // offset radius of the form
constexpr int kDK = 2 * kDR + 1;        // taps per axis (an offset of exactly +R has fraction 0: the tap at R + 1 carries weight 0)
constexpr int kDSpan = kDK - 1;
// The line forms (-DDAU_SPLIT_1D, namespaces l4 ...; DAU_FLAG_DENSE_SPLIT_LINE): the same GEMM over ONE row of taps, for calls whose
// units all lie on the row of their pixel (oy == 0 and no weight on the row below: the call's device guard decides).  The vertical
// radius is 0: no halo rows in the staged copy or in the LDS window, one row of the dense kernel, a tap loop over tx alone.
#ifndef DAU_SPLIT_1D
#define DAU_SPLIT_1D 0
#endif
constexpr bool kLine = DAU_SPLIT_1D != 0;
// The kernels of the line forms are named line_*_kernel (l4::line_gather_kernel, ...): tools and the built-code tests pick the 2-D
// forms' kernels by the name split_*_kernel.  EVERY __global__ function of this file is listed here.
#if DAU_SPLIT_1D
#define split_absmax_kernel line_absmax_kernel
#define split_scales_kernel line_scales_kernel
#define split_densify_kernel line_densify_kernel
#define split_stage_kernel line_stage_kernel
#define split_stage_walk_kernel line_stage_walk_kernel
#define split_gather_kernel line_gather_kernel
#endif
constexpr int kDRV = kLine ? 0 : kDR;   // vertical radius, taps and span
constexpr int kDKV = 2 * kDRV + 1;
constexpr int kDSpanV = kDKV - 1;
constexpr int kDTaps = kDKV * kDK;
constexpr int kDRows = 8;               // output rows per workgroup
constexpr int kDFB = 128;               // output channels per workgroup
constexpr int kAhead = 2;               // taps the A stream runs ahead
#ifndef DAU_SPLIT_FLUSH_TAPS
#define DAU_SPLIT_FLUSH_TAPS 0          // 0: a whole row of taps per chain
#endif
constexpr int kFlushTaps = DAU_SPLIT_FLUSH_TAPS > 0 ? DAU_SPLIT_FLUSH_TAPS : kDK;   // taps chained through `part` before it joins the running sum
#ifndef DAU_SPLIT_FLUSH_ROWS
#if DAU_SPLIT_1D
#define DAU_SPLIT_FLUSH_ROWS 1          // line forms: a row of taps is a whole chunk, 27 / 51 MFMAs per chain (profiles/r17_ab_line_chain_length.txt)
#else
#define DAU_SPLIT_FLUSH_ROWS 4          // rows of taps per chain (> 1: the chain runs across rows and chunks, `part` is zeroed by moves)
#endif
#endif
constexpr int kFlushRows = DAU_SPLIT_FLUSH_ROWS;
// The MFMA shape of the gather-sum, chosen per radius at compile time (every form of a radius shares one tap loop):
// v_mfma_f32_16x16x32_f16 over a PAIR of 16-channel chunks per tap ("K32", see split_gather_kernel) where it was measured to win,
// v_mfma_f32_32x32x16_f16 over one chunk elsewhere.  -DDAU_SPLIT_MFMA32 keeps the 32x32x16 loop at every radius: the A/B partner
// (libdau_conv_hip_mfma32.so).
#if !defined(DAU_SPLIT_K32)
#if !defined(DAU_SPLIT_MFMA32) && DAU_SPLIT_R == 3 && !DAU_SPLIT_1D
#define DAU_SPLIT_K32 1
#else
#define DAU_SPLIT_K32 0
#endif
#endif
constexpr bool kK32 = DAU_SPLIT_K32 != 0;

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// device-side scales of one pass (head of its workspace): this block, then sx[N] and 1 / sx[N] -- one power-of-two scale per IMAGE,
// so that an image's limbs (and with them its outputs) depend on no other image of the batch -- then the partial maxima
struct SplitScales {
    unsigned max_w_bits;                // float bits of the max over the finite units of |w| (sum of the four tap weights)
    float sw, inv_sw;                   // power-of-two scale of the dense taps and 1 / sw
    float pad[5];
};
__host__ __device__ __forceinline__ const float* scales_sx(const SplitScales* sc) { return reinterpret_cast<const float*>(sc + 1); }
__host__ __device__ __forceinline__ const float* scales_inv_sx(const SplitScales* sc, int N) { return reinterpret_cast<const float*>(sc + 1) + N; }
constexpr int kPartials = 1024;         // workgroups of the max reduction (at least one per image: kPartials + N bounds them)
// workgroups that share one image's maximum: all of kPartials over the batch, no more than the image has 1024-element pieces
inline int absmax_groups_per_image(int N, long per) {
    const long fit = std::max(1, kPartials / N), want = (per / 4 + 255) / 256 + 1;
    return (int)std::min(fit, want);
}
inline size_t scales_bytes(int N) { return sizeof(SplitScales) + (size_t)2 * N * sizeof(float); }

constexpr int kMaxSub = 4;              // 8-pixel tiles per column block (two accumulators per tile: see the header)
struct SplitGeom {
    int sub;                 // 8-pixel tiles per row
    // column blocks: nb_a blocks of nsub_a tiles from column 0, then nb_b blocks of nsub_b = nsub_a - 1 tiles (0 blocks when even)
    int nsub_a, nb_a, nsub_b, nb_b;
    // row blocks: nrb8 blocks of eight rows from row 0, then -- where 1 .. 4 rows are left -- one block of four (nrb4 = 1)
    int nrb8, nrb4;
    int tall;                // > 0: the eight-row blocks run as ONE column block of `tall` tiles of 8 rows x 4 columns (5 or 7)
    int Hs, Ws, nchunk, CoutP;
    size_t hdr_bytes, xs_bytes, ws_bytes;
};

SplitGeom split_geometry(const DenseConfig& c) {
    SplitGeom g{};
    g.sub = (c.W + 7) / 8;
    const int nblocks = (g.sub + kMaxSub - 1) / kMaxSub, base = g.sub / nblocks, rem = g.sub % nblocks;
    if (rem) { g.nsub_a = base + 1; g.nb_a = rem; g.nsub_b = base; g.nb_b = nblocks - rem; }
    else { g.nsub_a = base; g.nb_a = nblocks; g.nsub_b = 0; g.nb_b = 0; }
    const int left = c.H % kDRows;
    // the block of four rows is a launch of its own: it pays where the launches are many rounds of workgroups long (C3, 2048 workgroups:
    // gather 6.6 -> 6.1 ms per pass), not where a pass is two rounds and the split makes it three (C1, 512 workgroups: 0.34 -> 0.41 ms)
    const long wgs = (long)c.N * ((c.H + kDRows - 1) / kDRows) * nblocks * ((c.Cout + kDFB - 1) / kDFB);
    const int rows4 = DAU_TUNE_INT("DAU_SPLIT_ROWS4", 1);    // tuning build: 0 never, 2 always (the variant tests)
    g.nrb4 = (left >= 1 && left <= 4 && rows4 != 0 && (wgs >= 1024 || rows4 == 2)) ? 1 : 0;
    g.nrb8 = c.H / kDRows + (left && !g.nrb4 ? 1 : 0);
    g.Hs = g.nrb8 * kDRows + g.nrb4 * 4 + kDSpanV;
    {
        // tall tiles where they compute at least 5 % fewer tile positions than the 4 x 8 ones (whose waves skip dead groups of four rows):
        // 28 x 28 with a block of four rows: 24 x 28 + 4 x 32 against 28 x 32
        const int t4 = (c.W + 3) / 4;
        const long rows8 = (long)g.nrb8 * kDRows;
        const long flat = (long)(g.nrb4 ? rows8 + 4 : (c.H + 3) / 4 * 4) * g.sub * 8;
        const long tall = rows8 * t4 * 4 + (g.nrb4 ? 4L * g.sub * 8 : 0);
        const int want = DAU_TUNE_INT("DAU_SPLIT_TALL", 1);  // tuning build: 0 never, 2 wherever the width allows (the variant tests)
        g.tall = (want != 0 && g.nrb8 > 0 && (t4 == 5 || t4 == 7) && (tall * 20 <= flat * 19 || want == 2)) ? t4 : 0;
    }
    g.Ws = g.sub * 8 + kDSpan;
    g.nchunk = (c.Cin + 15) / 16;
    g.CoutP = (int)round_up(c.Cout, kDFB);
    g.hdr_bytes = round_up(scales_bytes(c.N) + (size_t)2 * (kPartials + c.N) * sizeof(unsigned), 256);
    // + 4 KiB: the window copy reads whole LDS-pitch rows, i.e. a few units past the last plane's last row
    g.xs_bytes = round_up((size_t)c.N * g.nchunk * 4 * g.Hs * g.Ws * 16 + 4096, 256);
    g.ws_bytes = round_up(((size_t)g.nchunk * kDTaps + 8) * 2 * g.CoutP * 32, 256);   // + look-ahead taps of the A stream
    return g;
}

constexpr int lds_pitch(int nsub) {       // positions; = 8 (mod 16) and >= nsub*8 + span: the four rows of a B fragment hit different banks
    int p = nsub * 8 + kDSpan;
    while (p % 16 != 8) ++p;
    return p;
}
// narrow tiles (8 rows x 4 columns): sixteen lanes read four columns of four rows -- conflict free at a pitch = 4 or 12 (mod 16)
constexpr int lds_pitch_narrow(int ntiles) {
    int p = ntiles * 4 + kDSpan;
    while (p % 16 != 4 && p % 16 != 12) ++p;
    return p;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// scales: max|input| per image and max|w|, finite values only (two launches: per-workgroup maxima, then one workgroup per image --
// and one for the units -- reduces them and derives the scales)
// ------------------------------------------------------------------------------------------------
// float bits of |v| for the maximum over the FINITE values: Inf and NaN (0x7f800000 and above) count as 0
__device__ __forceinline__ unsigned finite_bits(unsigned b) { return b < 0x7f800000u ? b : 0u; }

// elements in front of the first one whose address is a multiple of `vec_bytes` (all of them where the base is not even a
// multiple of the element size: scalar loads only)
__device__ __forceinline__ long absmax_head(const void* p, long per, int elem_bytes, int vec_bytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if (a % elem_bytes) return per;
    const long head = (long)((vec_bytes - a % vec_bytes) % vec_bytes) / elem_bytes;
    return head < per ? head : per;
}

// Workgroup (image n, share j of gpi): the maximum of the image's finite |values|.  An image's own base is in general not
// aligned to a vector load (S * H * W = 7 * 9 * 6 elements): `head` scalar elements, whole four-element pieces from the first
// aligned address, the tail scalar again -- a maximum does not depend on which load fetched an element.  Every workgroup also
// takes its share of the unit table.
// relu_in (DAU_FLAG_INPUT_RELU): the maximum of the CLAMPED input, x' = (x <= 0) ? 0 : x -- the scales, and with them the staged
// limbs, are those of the plan without the flag on x'.  One mask: with the sign bit kept, a negative value's bits lie above every
// finite magnitude and finite_bits drops them like an Inf.
__global__ void __launch_bounds__(256) split_absmax_kernel(const float* __restrict__ in, long per, int gpi, int act, const UnitRef* __restrict__ table,
                                                           long units, unsigned* __restrict__ partial, int cap, const Guard guard, int relu_in) {
    if (!guard_pass(guard)) return;
    unsigned mx = 0, mw = 0;
    const unsigned keep = relu_in ? 0xffffffffu : 0x7fffffffu, keep_hi = keep & 0xffff0000u;
    const int n = blockIdx.x / gpi, j = blockIdx.x - n * gpi;
    const long stride = (long)gpi * blockDim.x, t0 = j * (long)blockDim.x + threadIdx.x;
    if (act == kActF16) {
        // the widened values' bits, so that the maximum (and the scales) are those of the same input given as fp32
        auto wide = [keep](unsigned h) { return finite_bits(__float_as_uint(f16_bits_to_float(h)) & keep); };
        const unsigned short* e = reinterpret_cast<const unsigned short*>(in) + n * per;
        const long head = absmax_head(e, per, 2, 8), n4 = (per - head) / 4;
        const uint2* p = reinterpret_cast<const uint2*>(e + head);    // four f16 per load
        for (long i = t0; i < n4; i += stride) {
            const uint2 v = p[i];
            mx = max(mx, max(max(wide(v.x & 0xffffu), wide(v.x >> 16)), max(wide(v.y & 0xffffu), wide(v.y >> 16))));
        }
        for (long i = t0; i < per - n4 * 4; i += stride) mx = max(mx, wide(e[i < head ? i : i + n4 * 4]));
    } else if (act == kActBF16) {
        const unsigned short* e = reinterpret_cast<const unsigned short*>(in) + n * per;
        const long head = absmax_head(e, per, 2, 8), n4 = (per - head) / 4;
        const uint2* p = reinterpret_cast<const uint2*>(e + head);    // four bf16 per load
        for (long i = t0; i < n4; i += stride) {
            const uint2 v = p[i];
            mx = max(mx, max(max(finite_bits((v.x << 16) & keep), finite_bits(v.x & keep_hi)),
                             max(finite_bits((v.y << 16) & keep), finite_bits(v.y & keep_hi))));
        }
        for (long i = t0; i < per - n4 * 4; i += stride) mx = max(mx, finite_bits(((unsigned)e[i < head ? i : i + n4 * 4] << 16) & keep));
    } else {
        const float* e = in + n * per;
        const long head = absmax_head(e, per, 4, 16), n4 = (per - head) / 4;
        const uint4* p = reinterpret_cast<const uint4*>(e + head);
        for (long i = t0; i < n4; i += stride) {
            const uint4 v = p[i];
            mx = max(mx, max(max(finite_bits(v.x & keep), finite_bits(v.y & keep)),
                             max(finite_bits(v.z & keep), finite_bits(v.w & keep))));
        }
        for (long i = t0; i < per - n4 * 4; i += stride) mx = max(mx, finite_bits(__float_as_uint(e[i < head ? i : i + n4 * 4]) & keep));
    }
    for (long u = blockIdx.x * (long)blockDim.x + threadIdx.x; u < units; u += (long)gridDim.x * blockDim.x) {
        const UnitRef r = table[u];
        mw = max(mw, finite_bits(__float_as_uint(fabsf(r.w00) + fabsf(r.w01) + fabsf(r.w10) + fabsf(r.w11))));
    }
    __shared__ unsigned sx[4], sw[4];
    for (int m = 32; m >= 1; m >>= 1) { mx = max(mx, (unsigned)__shfl_xor((int)mx, m)); mw = max(mw, (unsigned)__shfl_xor((int)mw, m)); }
    if ((threadIdx.x & 63) == 0) { sx[threadIdx.x >> 6] = mx; sw[threadIdx.x >> 6] = mw; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = max(max(sx[0], sx[1]), max(sx[2], sx[3]));
        partial[cap + blockIdx.x] = max(max(sw[0], sw[1]), max(sw[2], sw[3]));
    }
}

// 2^(13 - floor(log2 m)) for a finite m > 0 (m * scale in [2^13, 2^14)), 1 otherwise (an image or a table without a finite
// non-zero value; Inf / NaN pass through the arithmetic)
__device__ __forceinline__ float limb_scale(float m) {
    if (!(m > 0.0f) || !(m < INFINITY)) return 1.0f;
    int e = ilogbf(m);
    e = 13 - e;
    e = e > 100 ? 100 : (e < -100 ? -100 : e);
    return ldexpf(1.0f, e);
}

// workgroup n < N: sx[n], 1 / sx[n] from the image's gpi partial maxima; workgroup N: sw, 1 / sw from all the workgroups' unit maxima
__global__ void __launch_bounds__(256) split_scales_kernel(const unsigned* __restrict__ partial, int N, int gpi, int cap, int G,
                                                           SplitScales* __restrict__ out, const Guard guard) {
    if (!guard_pass(guard)) return;
    const int n = blockIdx.x;
    const unsigned* src = n < N ? partial + (long)n * gpi : partial + cap;
    const int cnt = n < N ? gpi : N * gpi;
    unsigned m = 0;
    for (int i = threadIdx.x; i < cnt; i += 256) m = max(m, src[i]);
    __shared__ unsigned sm[4];
    for (int k = 32; k >= 1; k >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, k));
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = max(max(sm[0], sm[1]), max(sm[2], sm[3]));
        float* sx = reinterpret_cast<float*>(out + 1);
        if (n < N) {
            const float s = limb_scale(__uint_as_float(m));
            sx[n] = s; sx[N + n] = 1.0f / s;
        } else {
            const float s = limb_scale(__uint_as_float(m) * (float)G);    // a dense tap sums at most G units
            out->max_w_bits = m; out->sw = s; out->inv_sw = 1.0f / s;
            // a line form's guard has passed: this member does the pass's work (dau_conv_gather_line_status reports it).  The one
            // write a kernel makes through its guard (dau_common.hpp, Guard): one thread, the same value in every slab of a pass
            if constexpr (kLine) { if (guard.status) const_cast<Status*>(guard.status)->line_radius = (unsigned)kDR; }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// dense kernel synthesis: WS[chunk][tap][limb][f][sl] = limbs of sw * (sum over the units g of (c = 16*chunk + sl, f) of the
// bilinear weights that land on the tap).  One thread per (input channel, output channel): its K x K kernel is summed in LDS
// ([tap][thread] floats; the four taps of each of its G units added in unit order) and written out tap by tap.
// ------------------------------------------------------------------------------------------------
constexpr int kScT = 64;
__global__ void __launch_bounds__(kScT) split_densify_kernel(const UnitRef* __restrict__ table, int Cin, int G, int Cout, int CoutP, int nchunk,
                                                             const SplitScales* __restrict__ sc, _Float16* __restrict__ wsd, const Guard guard) {
    __shared__ float acc[kDTaps * kScT];
    if (!guard_pass(guard)) return;
    constexpr int FPB = kScT / 16;                         // output channels per workgroup
    const int tid = threadIdx.x, sl = tid & 15;
    const int fq = blockIdx.x % (CoutP / FPB), chunk = blockIdx.x / (CoutP / FPB);
    const int f = fq * FPB + (tid >> 4), c = chunk * 16 + sl;
#pragma unroll 7
    for (int tap = 0; tap < kDTaps; ++tap) acc[tap * kScT + tid] = 0.0f;
    if (c < Cin && f < Cout) {
        for (int g = 0; g < G; ++g) {
            const UnitRef u = table[((long)c * G + g) * Cout + f];
            const int ty = u.oy + kDRV, tx = u.ox + kDR;
            // (a tap outside the kernel belongs to an offset of exactly +R, weight 0, or to a call whose guard does not pass)
            const bool y0 = ty >= 0 && ty < kDKV, y1 = ty + 1 >= 0 && ty + 1 < kDKV, x0 = tx >= 0 && tx < kDK, x1 = tx + 1 >= 0 && tx + 1 < kDK;
            if (y0 && x0) acc[(ty * kDK + tx) * kScT + tid] += u.w00;
            if (y0 && x1) acc[(ty * kDK + tx + 1) * kScT + tid] += u.w01;
            if (y1 && x0) acc[((ty + 1) * kDK + tx) * kScT + tid] += u.w10;
            if (y1 && x1) acc[((ty + 1) * kDK + tx + 1) * kScT + tid] += u.w11;
        }
    }
    const float sw = sc->sw;
    _Float16* dst = wsd + ((long)chunk * kDTaps * 2 * CoutP + f) * 16 + sl;
    const long limb = (long)CoutP * 16, tapstride = 2 * limb;
#pragma unroll 7
    for (int tap = 0; tap < kDTaps; ++tap) {
        const float v = acc[tap * kScT + tid] * sw;
        const _Float16 hi = (_Float16)v;
        dst[tap * tapstride] = hi;
        dst[tap * tapstride + limb] = (_Float16)(v - (float)hi);
    }
}

// ------------------------------------------------------------------------------------------------
// staging: in[N,C,H,W] (f32 or bf16) -> XS (separable Gaussian, scaled, two f16 limbs, chunked, zero border).
// Workgroup = (image, group of 8 channels, band of rows, segment of <= 64 columns).  The raw window of the eight channels goes
// to LDS as fp32; then every wave walks its share of the band's rows with lane = column: horizontal pass from LDS, vertical
// pass over a register ring of K rows, two 16-byte units (hi, lo) = 8 channels per position.
// ------------------------------------------------------------------------------------------------
constexpr int kSP = 80;                   // LDS row of one channel: [8 spare | 64 columns | 8 spare] floats
struct SplitStageArgs {
    const float* in;
    const float* taps;
    const SplitScales* sc;
    _Float16* xs;
    int N, C, H, W, mirrored;
    int Hs, Ws, nchunk;
    int RB, nbands, nsegs;   // rows per band, bands and 64-column segments per plane (walking form: STAGED rows per band, bands, column tiles)
    int TW;                  // walking form: staged columns per tile
    int vec;                 // rows are whole 4-element pieces (W % 4 == 0, base aligned)
    int relu_in;             // DAU_FLAG_INPUT_RELU, forward direction: the widened input is clamped at zero, (v <= 0) ? +0 : v
    Guard guard;
};

// i / d for 0 <= i < 2^22 and a runtime d
__device__ __forceinline__ int fast_div(int i, int d, float inv) {
    int q = (int)(((float)i + 0.5f) * inv);
    const int r = i - q * d;
    q += (r >= d) - (r < 0);
    return q;
}

// Horizontal pass, IN PLACE: the waves share the rows of the band's window (row r = wave, wave + nw, ...); a lane filters its column
// of NCH channels and writes the results over the raw values.  In place is safe because a row segment belongs to ONE wave: every read
// of a channel's row precedes the write of that channel in the wave's instruction stream (the written value depends on all of them)
// and a wave's LDS operations execute in order.  (Before: every wave filtered the K - 1 halo rows of its own rows again -- ten rows
// for four at the north-star shape.)
template <int K, int NCH>
__device__ __forceinline__ void split_stage_rows(float* rawl, const float* px, int col, int ch0, int wave, int nw, int lh, int ncols) {
    constexpr int kr = (K - 1) / 2;
    if (col >= ncols) return;
    float gx[K];
#pragma unroll
    for (int j = 0; j < K; ++j) gx[j] = px[j];
    for (int r = wave; r < lh; r += nw) {
        float* row = rawl + (r * 8 + ch0) * kSP + 8 + col;
        float acc[NCH];
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            acc[ch] = 0.0f;
#pragma unroll
            for (int i = 0; i < K; ++i) acc[ch] = fmaf(row[ch * kSP + i - kr], gx[i], acc[ch]);
        }
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) row[ch * kSP] = acc[ch];
    }
}

// the walk of one wave over its rows ya .. yb: lane column `col`, channels ch0 .. ch0 + NCH - 1 of the group's eight; vertical pass over
// a register ring of K horizontally filtered rows (rawl after split_stage_rows), scale, split, store
template <int K, int NCH>
__device__ __forceinline__ void split_stage_walk(const float* rawl, const float* py, float sx, int col, int ch0, int ya, int yb,
                                                 int y0, int x0, int x1, int Ws, u32x4* xhi, u32x4* xlo) {
    constexpr int kr = (K - 1) / 2;
    const int x = x0 + col;
    if (x >= x1) return;
    float gy[K];
#pragma unroll
    for (int j = 0; j < K; ++j) gy[j] = py[j];
    float ring[K][NCH];
    const int nin = yb - ya + 2 * kr;                        // input rows ya - kr .. yb + kr - 1
    char* dhi = reinterpret_cast<char*>(xhi + (long)kDRV * Ws + kDR + x) + ch0 * 2;
    char* dlo = reinterpret_cast<char*>(xlo + (long)kDRV * Ws + kDR + x) + ch0 * 2;
    for (int s0 = 0; s0 < nin; s0 += K) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const int s = s0 + j;
            if (s < nin) {
                const float* row = rawl + ((ya - y0 + s) * 8 + ch0) * kSP + 8 + col;
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) ring[j][ch] = row[ch * kSP];
                if (s >= K - 1) {
                    typedef _Float16 f16xn __attribute__((ext_vector_type(NCH)));
                    f16xn oh, ol;
#pragma unroll
                    for (int ch = 0; ch < NCH; ++ch) {
                        float acc = 0.0f;
#pragma unroll
                        for (int i = 0; i < K; ++i) acc = fmaf(ring[(j + 1 + i) % K][ch], gy[i], acc);
                        acc *= sx;
                        const _Float16 hi = (_Float16)acc;
                        oh[ch] = hi;
                        ol[ch] = (_Float16)(acc - (float)hi);
                    }
                    const long o = (long)(ya + s - (K - 1)) * Ws * 16;
                    *reinterpret_cast<f16xn*>(dhi + o) = oh;
                    *reinterpret_cast<f16xn*>(dlo + o) = ol;
                }
            }
        }
    }
}

#ifndef DAU_SPLIT_STAGE_THREADS
#define DAU_SPLIT_STAGE_THREADS 512        // eight waves share a band (same box: 375 us per pass at the north-star shape with 256 threads, 362 with 512)
#endif
constexpr int kStageThreads = DAU_SPLIT_STAGE_THREADS;
// KN = K | kNhwcArg: `in` is [N][H][W][C].  The group's eight channels of a pixel are 32 (fp32) or 16 (16-bit) contiguous bytes: a piece
// is 16 of them -- four fp32 channels or all eight 16-bit ones -- of one pixel, adjacent lanes take the pieces of adjacent pixels of a
// row, and a lane scatters its piece into the same [row][8 channels][kSP] image (consecutive lanes, consecutive columns: no bank
// conflict), so that the filter passes are the NCHW kernel's.  a.vec: C is a multiple of the piece's channels and the base is 16-byte
// aligned; otherwise the piece is loaded element by element.
template <int KN, int A>
__global__ void __launch_bounds__(kStageThreads) split_stage_kernel(const SplitStageArgs a) {
    constexpr int K = KN & (kNhwcArg - 1);
    constexpr bool NHWC = (KN & kNhwcArg) != 0;
    extern __shared__ __attribute__((aligned(16))) float rawl[];   // [row][8 channels][kSP]
    if (!guard_pass(a.guard)) return;
    constexpr int kr = (K - 1) / 2;
    constexpr int PPR = kSP / 4;                                   // 4-element pieces per LDS row
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int t = blockIdx.x;
    const int seg = t % a.nsegs; t /= a.nsegs;
    const int band = t % a.nbands; t /= a.nbands;
    const int grp = t % (2 * a.nchunk);                             // chunk = grp / 2, half = grp & 1
    const int n = t / (2 * a.nchunk);
    const int y0 = band * a.RB, y1 = y0 + a.RB < a.H ? y0 + a.RB : a.H;
    const int x0 = seg * 64, x1 = x0 + 64 < a.W ? x0 + 64 : a.W;
    const int lh = y1 - y0 + 2 * kr;
    const long plane = (long)a.H * a.W;
    const bool ri = a.relu_in != 0;
    if constexpr (NHWC) {
        // ---- raw window -> LDS: piece (r, j, part) covers image row y0 - kr + r, column x0 - 8 + j, channels grp*8 + part*CPP .. + CPP - 1
        constexpr int CPP = A == kActF32 ? 4 : 8, PARTS = 8 / CPP;
        const int pieces = lh * kSP * PARTS;
        constexpr int UB = (13 * 256 + kStageThreads - 1) / kStageThreads;   // (as below)
        for (int i0 = threadIdx.x; i0 < pieces; i0 += kStageThreads * UB) {
            float v[UB][CPP];
            // branch-free loads (clamped address, masked value), as below
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const int i = i0 + u * kStageThreads, part = i % PARTS, rj = i / PARTS, r = rj / kSP, j = rj - r * kSP;
                const int c = grp * 8 + part * CPP, y = y0 - kr + r, x = x0 - 8 + j;
                const bool pix = y >= 0 && y < a.H && x >= 0 && x < a.W && i < pieces;
                if (a.vec) {
                    const bool ok = pix && c < a.C;                  // (C is a multiple of CPP: the whole piece lies inside)
                    const long idx = ok ? nhwc_index(n, c, y, x, a.C, a.H, a.W) : 0;
                    if constexpr (A == kActF32) {
                        const float4 w = *reinterpret_cast<const float4*>(a.in + idx);
                        v[u][0] = mask_act(w.x, ok); v[u][1] = mask_act(w.y, ok); v[u][2] = mask_act(w.z, ok); v[u][3] = mask_act(w.w, ok);
                    } else {
                        const uint4 w = *reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned short*>(a.in) + idx);
                        const unsigned q[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            if constexpr (A == kActF16) {
                                v[u][2 * k] = mask_act(f16_bits_to_float(q[k] & 0xffffu), ok);
                                v[u][2 * k + 1] = mask_act(f16_bits_to_float(q[k] >> 16), ok);
                            } else {
                                const unsigned m = ok ? 0xffffffffu : 0u;
                                v[u][2 * k] = __uint_as_float((q[k] << 16) & m);
                                v[u][2 * k + 1] = __uint_as_float(q[k] & 0xffff0000u & m);
                            }
                        }
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < CPP; ++k) {
                        const bool ok = pix && c + k < a.C;
                        v[u][k] = mask_act(load_act_t<A>(a.in, ok ? nhwc_index(n, c + k, y, x, a.C, a.H, a.W) : 0), ok);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const int i = i0 + u * kStageThreads, part = i % PARTS, rj = i / PARTS, r = rj / kSP, j = rj - r * kSP;
                if (i < pieces) {
#pragma unroll
                    for (int k = 0; k < CPP; ++k) rawl[(r * 8 + part * CPP + k) * kSP + j] = relu_in(v[u][k], ri);
                }
            }
        }
    } else
    // ---- raw window -> LDS: piece (r, ch, q) covers image row y0 - kr + r, columns x0 - 8 + 4q .. + 3 of channel grp*8 + ch
    {
        const int pieces = lh * 8 * PPR;
        constexpr int UB = (13 * 256 + kStageThreads - 1) / kStageThreads;   // loads in flight per thread: the whole window of a 14-row band (12.5 pieces per thread of 256) in one batch
        for (int i0 = threadIdx.x; i0 < pieces; i0 += kStageThreads * UB) {
            float4 v[UB];
            // branch-free loads (clamped address, masked value): a branch around a load makes hipcc wait for it at the join
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const int i = i0 + u * kStageThreads, rc = i / PPR, q = i - rc * PPR, r = rc >> 3, ch = rc & 7;
                const int c = grp * 8 + ch, y = y0 - kr + r, xs = x0 - 8 + 4 * q;
                const bool row_in = c < a.C && y >= 0 && y < a.H && i < pieces;
                const long base = ((long)n * a.C + (c < a.C ? c : 0)) * plane;
                if (a.vec) {
                    const bool ok = row_in && xs >= 0 && xs + 4 <= a.W;
                    const long idx = base + (ok ? (long)y * a.W + xs : 0);
                    if constexpr (A == kActF16) {
                        const uint2 w = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(a.in) + idx);
                        v[u] = make_float4(mask_act(f16_bits_to_float(w.x & 0xffffu), ok), mask_act(f16_bits_to_float(w.x >> 16), ok),
                                           mask_act(f16_bits_to_float(w.y & 0xffffu), ok), mask_act(f16_bits_to_float(w.y >> 16), ok));
                    } else if constexpr (A == kActBF16) {
                        const uint2 w = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(a.in) + idx);
                        const unsigned m = ok ? 0xffffffffu : 0u;
                        v[u] = make_float4(__uint_as_float((w.x << 16) & m), __uint_as_float(w.x & 0xffff0000u & m),
                                           __uint_as_float((w.y << 16) & m), __uint_as_float(w.y & 0xffff0000u & m));
                    } else {
                        const float4 w = *reinterpret_cast<const float4*>(a.in + idx);
                        v[u] = make_float4(mask_act(w.x, ok), mask_act(w.y, ok), mask_act(w.z, ok), mask_act(w.w, ok));
                    }
                } else {
                    float e[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const bool ok = row_in && xs + k >= 0 && xs + k < a.W;
                        e[k] = mask_act(load_act_t<A>(a.in, base + (ok ? (long)y * a.W + xs + k : 0)), ok);
                    }
                    v[u] = make_float4(e[0], e[1], e[2], e[3]);
                }
            }
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const int i = i0 + u * kStageThreads;
                if (i < pieces)                                                                // piece i sits at [r][ch][4q]: i * 4 floats
                    *reinterpret_cast<float4*>(rawl + (long)i * 4) = make_float4(relu_in(v[u].x, ri), relu_in(v[u].y, ri), relu_in(v[u].z, ri), relu_in(v[u].w, ri));
            }
        }
    }
    // ---- zero border of the staged planes (both limbs): what this workgroup's rows / columns touch outside the image
    const int chunk = grp >> 1, half = grp & 1;
    const long splane = (long)a.Hs * a.Ws;
    u32x4* xhi = reinterpret_cast<u32x4*>(a.xs) + ((((long)n * a.nchunk + chunk) * 2 + 0) * 2 + half) * splane;
    u32x4* xlo = xhi + 2 * splane;
    {
        const int rs0 = band == 0 ? 0 : y0 + kDRV, rs1 = band == a.nbands - 1 ? a.Hs : y1 + kDRV;
        const int cs0 = seg == 0 ? 0 : x0 + kDR, cs1 = seg == a.nsegs - 1 ? a.Ws : x1 + kDR;
        const int cw = cs1 - cs0, cnt = (rs1 - rs0) * cw;
        const float inv = 1.0f / (float)cw;
        const u32x4 z = {0u, 0u, 0u, 0u};
        for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
            const int rr = fast_div(i, cw, inv), r = rs0 + rr, cc = cs0 + i - rr * cw;
            if (r >= y0 + kDRV && r < y1 + kDRV && cc >= x0 + kDR && cc < x1 + kDR) continue;
            xhi[(long)r * a.Ws + cc] = z;
            xlo[(long)r * a.Ws + cc] = z;
        }
    }
    __syncthreads();
    // lane = column; segments of at most 32 columns (maps up to 32 pixels wide) give the two half waves four channels each instead of
    // leaving half of the lanes idle
    const float* px = a.taps + (a.mirrored ? kTapGXR : kTapGX) * kTapPitch;
    const float* py = a.taps + (a.mirrored ? kTapGYR : kTapGY) * kTapPitch;
    // ---- horizontal pass over every row of the window, in place (the waves share the rows)
    if (x1 - x0 <= 32) split_stage_rows<K, 4>(rawl, px, lane & 31, (lane >> 5) * 4, wave, nw, lh, x1 - x0);
    else split_stage_rows<K, 8>(rawl, px, lane, 0, wave, nw, lh, x1 - x0);
    __syncthreads();
    // ---- vertical pass, scale, split, store: rows ya .. yb of this wave
    const int SR = (y1 - y0 + nw - 1) / nw;
    const int ya = y0 + wave * SR, yb = ya + SR < y1 ? ya + SR : y1;
    if (ya >= yb) return;
    const float sx = scales_sx(a.sc)[n];                           // this image's scale (n is uniform over the workgroup)
    if (x1 - x0 <= 32) split_stage_walk<K, 4>(rawl, py, sx, lane & 31, (lane >> 5) * 4, ya, yb, y0, x0, x1, a.Ws, xhi, xlo);
    else split_stage_walk<K, 8>(rawl, py, sx, lane, 0, ya, yb, y0, x0, x1, a.Ws, xhi, xlo);
}

// ------------------------------------------------------------------------------------------------
// staging, walking form (NCHW inputs; -DDAU_SPLIT_STAGE_REF keeps the kernel above for every plan: libdau_conv_hip_split_stage_ref.so,
// the bit-for-bit reference of tests/test_gpu_split_stage_walk.py and the A/B partner).  The kernel above runs its phases one after
// the other -- the band's raw window to LDS, barrier, horizontal pass, barrier, vertical pass and stores -- so a workgroup's loads,
// arithmetic and stores never overlap.  Here a wave (= a workgroup) owns (image, group of 8 channels, tile of <= 64 STAGED columns,
// band of staged rows) and walks down the rows, as sd_xk_walk_kernel (k_split_dot.hip) does:
//  * Lane = staged column cs0 + lane (image column x = cs - R); on tiles of <= 32 columns each half wave takes four of the channels.
//    The tiles cut the STAGED row, so the zero border left and right of the image (and the rows above and below it) are lanes and
//    steps of the same code whose values are masked to +0: every unit of the plane is written by exactly one store.
//  * Per step one raw row of the eight channels (the tile's columns plus the filter's reach) goes through LDS, channel pairs interleaved:
//    element loads, branch free (clamped address, masked value: rows / columns outside the image and the absent channels of a ragged
//    last group are +0).  Two row buffers and one wave-level barrier per row; the loads of the rows kAhead steps on are in flight.
//  * Horizontal pass from LDS, acc = fma(row[x - kr + i], gx[i], acc) for i = 0 .. K - 1 from acc = 0 -- split_stage_rows' order.  The K
//    filtered rows live in a register ring; the row loop is unrolled K times, so that every slot is a fixed register.  Vertical pass
//    in split_stage_walk's order, then * sx[n], hi = f16(v), lo = f16(v - hi) and one hi and one lo store per lane, consecutive lanes
//    to consecutive units.  The fmas are v_pk_fma_f32 on channel pairs: per element the same fused multiply-add.
// ------------------------------------------------------------------------------------------------
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void stage_wave_sync() {     // orders a wave's LDS writes before the reads of its other lanes
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <int N, class F>
__device__ __forceinline__ void stage_unroll(F&& f) {   // f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>)
    [&]<int... I>(std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }(std::make_integer_sequence<int, N>{});
}
#ifndef DAU_SPLIT_WALK_AHEAD
#define DAU_SPLIT_WALK_AHEAD 2
#endif
constexpr int stage_walk_buf(int K) { return (8 * (64 + K - 1) + 63) / 64 * 64; }   // floats of one row buffer (the 64-column form's)

template <int K, int A, int NCH>
__device__ __forceinline__ void split_stage_walk_tile(const SplitStageArgs& a, float* lds, int n, int grp, int cs0, int cs1, int b0, int b1) {
    typedef typename RawAct<A>::type Raw;
    typedef _Float16 f16xn __attribute__((ext_vector_type(NCH)));
    constexpr int kr = (K - 1) / 2, CW = (NCH == 8 ? 64 : 32) + K - 1, kBuf = stage_walk_buf(K);
    constexpr int CWL = CW < 64 ? CW : 64, XT = CW - CWL, NX = (8 * XT + 63) / 64, NL = 8 + NX;   // (see the loads below)
    constexpr int kAhead = K > 3 ? DAU_SPLIT_WALK_AHEAD : 2;   // rows whose loads are in flight (slots of the unrolled loop: < K)
    static_assert(8 * CW <= kBuf, "the eight channels' rows lie inside the row buffer");
    const int lane = threadIdx.x, col = NCH == 8 ? lane : lane & 31, ch0 = NCH == 8 ? 0 : (lane >> 5) * 4;
    const int H = a.H, W = a.W;
    const long plane = (long)H * W;
    const float* px = a.taps + (a.mirrored ? kTapGXR : kTapGX) * kTapPitch;
    const float* py = a.taps + (a.mirrored ? kTapGYR : kTapGY) * kTapPitch;
    f32x2 gx[K], gy[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { gx[j] = f32x2{px[j], px[j]}; gy[j] = f32x2{py[j], py[j]}; }
    // The raw row of the tile: 8 channels x CW columns (image x = cs0 - R - kr + column) as NL loads per lane.  Load l < 8 is
    // channel l, lane = column (the first 64 columns: one contiguous run per load, one lane offset for all eight); the columns
    // beyond the 64th of the eight channels share NX further loads, XT columns per channel.  A load outside the row or of an
    // absent channel reads a valid element of the image and is masked.  A value sits at buf[channel pair][column][channel of the
    // pair], so that one 8-byte LDS read is the operand of a packed fma.
    const int xm = cs0 - kDR - kr + lane;
    const bool okm = lane < CWL && xm >= 0 && xm < W;
    const unsigned offm = (unsigned)(xm < 0 ? 0 : xm < W ? xm : W - 1);
    unsigned offx[NX > 0 ? NX : 1], posx[NX > 0 ? NX : 1], okx = 0u;       // (elements from the group's first channel: 8 planes, 32 bits)
#pragma unroll
    for (int e = 0; e < NX; ++e) {
        const int tt = e * 64 + lane, tc = tt < 8 * XT ? tt : 0;
        const int ch = XT > 0 ? tc / (XT > 0 ? XT : 1) : 0, cl = 64 + tc - ch * XT;
        const bool chan = grp * 8 + ch < a.C;
        const int xx = cs0 - kDR - kr + cl;
        okx |= (tt < 8 * XT ? 1u : 0u) << (2 * e) | (tt < 8 * XT && chan && xx >= 0 && xx < W ? 2u : 0u) << (2 * e);
        offx[e] = (unsigned)((chan ? ch : 0) * plane) + (unsigned)(xx < 0 ? 0 : xx < W ? xx : W - 1);
        posx[e] = (unsigned)((ch >> 1) * 2 * CW + cl * 2 + (ch & 1));
    }
    const long gbase = ((long)n * a.C + (grp * 8 < a.C ? grp * 8 : 0)) * plane;
    const float sx = scales_sx(a.sc)[n];                // this image's scale
    // stream row (image row b0 - R - kr + u) enters at step u; staged row rs = b0 + u - (K - 1) leaves at step u.  The steps are
    // rounded up to whole rounds of the unrolled loop and a step has no branch but the one around its stores: the steps before the
    // band's first row and after its last one compute on clamped rows and store nothing.
    const int steps = (b1 - b0 + K - 1 + K - 1) / K * K;
    Raw rv[K][NL];
    f32x2 ring[K][NCH / 2];
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
        for (int cp = 0; cp < NCH / 2; ++cp) ring[i][cp] = f32x2{0.0f, 0.0f};
    auto load_row = [&](int u, Raw* dst) {
        const int r = b0 - kDRV - kr + u, rc = r < 0 ? 0 : r < H ? r : H - 1;
        const long rowbase = gbase + (long)rc * W;
#pragma unroll
        for (int l = 0; l < 8; ++l) dst[l] = load_raw<A>(a.in, rowbase + (grp * 8 + l < a.C ? l : 0) * plane + (long)offm);
#pragma unroll
        for (int e = 0; e < NX; ++e) dst[8 + e] = load_raw<A>(a.in, rowbase + (long)offx[e]);
    };
#pragma unroll
    for (int d = 0; d < kAhead; ++d) load_row(d, rv[d]);
    const int chunk = grp >> 1, half = grp & 1;
    const long splane = (long)a.Hs * a.Ws;
    u32x4* const xhi = reinterpret_cast<u32x4*>(a.xs) + ((((long)n * a.nchunk + chunk) * 2 + 0) * 2 + half) * splane;
    u32x4* const xlo = xhi + 2 * splane;
    const int cs = cs0 + col, x = cs - kDR;
    const bool col_in = x >= 0 && x < W, col_st = cs < cs1;
    const bool ri = a.relu_in != 0;
    auto step = [&](auto pc, int u) {
        constexpr int P = decltype(pc)::value;
        load_row(u + kAhead, rv[(P + kAhead) % K]);
        const int r = b0 - kDRV - kr + u;
        const bool row_in = r >= 0 && r < H;
        float* buf = lds + (u & 1) * kBuf;
        if (CWL == 64 || lane < CWL) {
#pragma unroll
            for (int l = 0; l < 8; ++l)
                buf[(l >> 1) * 2 * CW + lane * 2 + (l & 1)] = mask_act(relu_in(act_of(rv[P][l]), ri), okm && row_in && grp * 8 + l < a.C);
        }
#pragma unroll
        for (int e = 0; e < NX; ++e)
            if ((okx >> (2 * e)) & 1u) buf[posx[e]] = mask_act(relu_in(act_of(rv[P][8 + e]), ri), ((okx >> (2 * e)) & 2u) && row_in);
        stage_wave_sync();
        f32x2 h[NCH / 2];
#pragma unroll
        for (int cp = 0; cp < NCH / 2; ++cp) h[cp] = f32x2{0.0f, 0.0f};
        const f32x2* row = reinterpret_cast<const f32x2*>(buf) + (ch0 / 2) * CW + col;
        // (two channel pairs at a time: the LDS reads in flight are registers)
#pragma unroll
        for (int c0 = 0; c0 < NCH / 2; c0 += 2) {
            stage_unroll<K>([&](auto ic) {
                constexpr int I = decltype(ic)::value;
#pragma unroll
                for (int cp = c0; cp < c0 + 2; ++cp) h[cp] = __builtin_elementwise_fma(row[cp * CW + I], gx[I], h[cp]);
            });
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int cp = 0; cp < NCH / 2; ++cp) ring[P][cp] = h[cp];
        const int rs = b0 + u - (K - 1), y = rs - kDRV;
        f32x2 o[NCH / 2];
#pragma unroll
        for (int cp = 0; cp < NCH / 2; ++cp) o[cp] = f32x2{0.0f, 0.0f};
        stage_unroll<K>([&](auto jc) {
            constexpr int J = decltype(jc)::value, sl = (P + 1 + J) % K;   // (P + 1: the slot of stream row y - kr)
#pragma unroll
            for (int cp = 0; cp < NCH / 2; ++cp) o[cp] = __builtin_elementwise_fma(ring[sl][cp], gy[J], o[cp]);
        });
        // (rows and columns outside the image: +0 in both limbs, whatever the sums over the neighbouring rows gave)
        const bool in = col_in && y >= 0 && y < H;
        f16xn oh, ol;
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            float acc = o[ch / 2][ch & 1];
            acc *= sx;
            const _Float16 hi = (_Float16)acc;
            oh[ch] = in ? hi : (_Float16)0.0f;
            ol[ch] = in ? (_Float16)(acc - (float)hi) : (_Float16)0.0f;
        }
        if (col_st && rs >= b0 && rs < b1) {
            const long o16 = ((long)rs * a.Ws + cs) * 16 + ch0 * 2;
            *reinterpret_cast<f16xn*>(reinterpret_cast<char*>(xhi) + o16) = oh;
            *reinterpret_cast<f16xn*>(reinterpret_cast<char*>(xlo) + o16) = ol;
        }
    };
#pragma unroll 1
    for (int u0 = 0; u0 < steps; u0 += K) {
        stage_unroll<K>([&](auto pc) { step(pc, u0 + decltype(pc)::value); });
    }
}

// (four waves per SIMD -- 128 registers -- up to a support of 7, where the ring and the rows in flight fit)
#ifndef DAU_SPLIT_WALK_WAVES
#define DAU_SPLIT_WALK_WAVES 4
#endif
template <int K, int A>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(K <= 7 ? DAU_SPLIT_WALK_WAVES : 2))) split_stage_walk_kernel(const SplitStageArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[2 * stage_walk_buf(K)];
    if (!guard_pass(a.guard)) return;
    int t = blockIdx.x;
    const int seg = t % a.nsegs; t /= a.nsegs;
    const int band = t % a.nbands; t /= a.nbands;
    const int grp = t % (2 * a.nchunk), n = t / (2 * a.nchunk);      // chunk = grp / 2, half = grp & 1
    const int cs0 = seg * a.TW, cs1 = cs0 + a.TW < a.Ws ? cs0 + a.TW : a.Ws;
    const int b0 = band * a.RB, b1 = b0 + a.RB < a.Hs ? b0 + a.RB : a.Hs;
    if (a.TW <= 32) split_stage_walk_tile<K, A, 4>(a, lds, n, grp, cs0, cs1, b0, b1);
    else split_stage_walk_tile<K, A, 8>(a, lds, n, grp, cs0, cs1, b0, b1);
}

// ------------------------------------------------------------------------------------------------
// main kernel
// ------------------------------------------------------------------------------------------------
struct SplitArgs {
    const _Float16* xs;
    const _Float16* wsd;
    const SplitScales* sc;
    float* out;               // [N][Cout][H][W] (NHWC instantiations: [N][H][W][Cout]), f32, bf16 or f16
    const float* partial;     // ADD instantiations: [N][Cout][H][W] fp32 (always planar), added to the sums before the store's rounding
    int N, Cout, CoutP, H, W, Hs, Ws, nchunk, ncb, nrb, out_act;   // out_act: ActFormat of out (NHWC instantiations: | kNhwcVecOut)
    int col0;                 // first column of this launch's blocks (a row is covered by blocks of NSUB and of NSUB - 1 tiles)
    int row0;                 // first row of this launch's row blocks (a map whose height leaves 1 .. 4 rows after its 8-row blocks
                              // ends with one block of FOUR rows: RG = 1)
    Guard guard;
};
// the arguments of the kEpiArg instantiations (kernels of their own: the others keep SplitArgs, and so the offsets of everything that
// follows it in their argument segment)
struct SplitArgsEpi : SplitArgs {
    const float* bias;        // [Cout] fp32 added to the sums before the store's rounding, or null
    int relu;                 // ... then ReLU
    const float* residual;    // out's shape, format and layout: added after the bias, before the ReLU; or null
    int res_vec;              // NHWC: Cout is a multiple of four and the RESIDUAL's base is aligned for loads of four channels
    const float* gate;        // out's shape, format and layout: the store is (gate <= 0) ? 0 : value, after everything else (the dx pass
                              // of DAU_FLAG_INPUT_RELU: the layer's raw x); or null
    int gate_vec;             // ... and the GATE's own base likewise
};

// RG: row groups (of four rows) per workgroup.  2: the eight waves are 4 (32 channels) x 2 (row groups), a wave owns the NSUB tiles of its
// row group.  1: a block of four rows -- 4 (32 channels) x 2 (column halves), a wave owns (NSUB + 1) / 2 tiles; used for the last
// 1 .. 4 rows of a map (28- and 27-pixel maps: 24 + 4 rows instead of 32).
// TT ("tall tiles", RG = 2 only): a tile is 8 rows x 4 columns instead of 4 rows x 8 columns and NSUB counts those; the workgroup is
// 8 rows x NSUB*4 columns, its eight waves 4 (32 channels) x 2 (column halves of (NSUB + 1) / 2 and NSUB / 2 tiles -- the two waves of a
// SIMD, so the SIMD's work is NSUB tiles).  For maps whose width is 1 .. 4 columns more than a multiple of eight (28 = 7 x 4: no padded
// columns where 4 x 8 tiles pad to 32).
// H16: out is binary16 (an instantiation of its own, so that the fp32 / bf16 kernels keep their epilogue as it was)
// ADD (radius 3 only): the epilogue adds the fp32 partial sums of the ring pass (k_dense_ring.hip) before the one rounding of the store
// NSUBN = NSUB | kNhwcArg: out is [N][H][W][Cout].  A lane's sixteen results of a tile are four groups of four CONSECUTIVE channels of
// its pixel: one 16-byte (fp32) or 8-byte (16-bit) store per group where Cout is a multiple of four and the base is aligned (kNhwcVecOut
// in out_act), element stores otherwise.  The values and their one rounding are the NCHW epilogue's.
// NSUBN | kEpiArg: the store is act(v + bias[f]) of the value v the kernel would have stored (with ADD: after the ring's partial sum has
// joined), in fp32 before the one rounding; the bias is read in the epilogue, after the tap loop, with the channel clamped to Cout - 1.
// With a residual (a run-time pointer: a wave-uniform branch per store) it is act((v + bias[f]) + r[o]), r read at out's index o in
// out's format: the NHWC forms with one 16- or 8-byte load per group of four channels where Cout is a multiple of four and the
// RESIDUAL's base is aligned (res_vec, whatever out's own alignment), element loads with the channel clamped otherwise.
// With a gate (likewise a run-time pointer and a wave-uniform branch) the value is then masked, (g[o] <= 0) ? 0 : value, g read like the
// residual, by its own alignment flag (gate_vec).
constexpr int kNhwcVecOut = 0x100;
template <int NSUBN, int RG = 2, bool TT = false, bool H16 = false, bool ADD = false>
__global__ void __launch_bounds__(512) split_gather_kernel(const typename std::conditional<(NSUBN & kEpiArg) != 0, SplitArgsEpi, SplitArgs>::type a) {
    constexpr int NSUB = NSUBN & (kNhwcArg - 1);
    constexpr bool NHWC = (NSUBN & kNhwcArg) != 0;
    constexpr bool EPI = (NSUBN & kEpiArg) != 0;
    static_assert(!TT || RG == 2, "tall tiles: blocks of eight rows");
    constexpr int TW = TT ? 4 : 8;                           // columns of a tile
    constexpr int P = TT ? lds_pitch_narrow(NSUB) : lds_pitch(NSUB);   // LDS pitch (positions)
    constexpr int kRowsWG = 4 * RG;                          // output rows per workgroup
    constexpr int NT0 = (RG == 2 && !TT) ? NSUB : (NSUB + 1) / 2;      // tiles per wave
    constexpr int NT1 = TT ? NSUB / 2 : NT0;                 // ... of the second column half (tall tiles)
    constexpr int WR = kRowsWG + kDSpanV;                    // window rows
    // K32: K groups 0 and 1 of a ds_read_b128 lane group read planes one `HALF` apart: a whole number of bank rows (16 positions)
    constexpr int PLANE = kK32 ? (WR * P + 15) / 16 * 16 : WR * P;   // 16-byte units of one (limb, half) plane window
    constexpr int HALF = PLANE * 16;                         // ... in bytes
    constexpr int BUFU = 4 * PLANE;                          // 16-byte units of a chunk's window: [limb][half][row][P]
    constexpr int NPIECE = (BUFU + 63) / 64;                 // 1 KiB pieces (one global_load_lds wave instruction each)
    constexpr int BUF1 = NPIECE * 1024;                      // one chunk's window
    constexpr int BUF = kK32 ? 2 * BUF1 : BUF1;              // K32: the windows of a chunk pair, one after the other
    constexpr int PPW = (NPIECE + 7) / 8;                    // pieces per wave
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (!guard_pass(a.guard)) return;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fw = wave & 3, pw = wave >> 2;                 // channel part / row group (RG = 2) or column half (RG = 1, TT) of the workgroup tile
    const int prow = (RG == 2 && !TT) ? 4 * pw : 0, ptile = (RG == 2 && !TT) ? 0 : pw * NT0;   // first row / first tile of this wave inside the workgroup tile
    // Workgroups are dealt to the eight XCDs round robin (block b runs on XCD b % 8) and every XCD has its own L2: consecutive
    // LOGICAL ids -- the channel blocks of one window, then the next column block, the next row block (both share halo with it),
    // the same image -- are mapped to one XCD, so that a window is fetched from HBM once, not once per channel block
    int t;
#ifdef DAU_SPLIT_NO_XCD_MAP                // (timing experiment: tools/build_variant.sh)
    t = blockIdx.x;
#else
    {
        const int nblk = gridDim.x, xcd = blockIdx.x % 8, idx = blockIdx.x / 8;
        const int per = nblk / 8, rem = nblk % 8;
        t = (xcd < rem ? xcd * (per + 1) : rem * (per + 1) + (xcd - rem) * per) + idx;
    }
#endif
    const int fb = t % (a.CoutP / kDFB); t /= (a.CoutP / kDFB);       // channel blocks fastest: they share the window
    const int cb = t % a.ncb; t /= a.ncb;
    const int rb = t % a.nrb;
    const int n = t / a.nrb;
    const int h = lane >> 5, nn = lane & 31;

    // window copy: LDS unit L = ((limb*2 + half) * WR + r) * P + c  <-  plane (limb, half), staged position (rb*8 + r, cb*NSUB*8 + c).
    // Whole pitch rows are copied (c up to P - 1 reads past the window, into the row's tail or the next row: never used).
    const long xs_plane = (long)a.Hs * a.Ws;                 // 16-byte units per (n, chunk, limb, half)
    const int colb = a.col0 + cb * NSUB * TW;                // first column of this block
    const int rowb = a.row0 + rb * kRowsWG;                  // first row of this block
    const u32x4* xsrc = reinterpret_cast<const u32x4*>(a.xs) + ((long)n * a.nchunk * 4) * xs_plane + (long)rowb * a.Ws + colb;
    int goff[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        int piece = wave + 8 * i;
        piece = piece < NPIECE ? piece : NPIECE - 1;         // surplus pieces repeat the last one
        int L = piece * 64 + lane;
        L = L < BUFU ? L : BUFU - 1;
        const int ph = L / PLANE;
        int rem = L - ph * PLANE;
        rem = rem < WR * P ? rem : WR * P - 1;               // (K32: the units that pad a plane repeat its last one)
        const int r = rem / P, c = rem - r * P;
        goff[i] = (int)(ph * xs_plane + (long)r * a.Ws + c);
    }
    auto issue = [&](int chunk, int buf) {
        const u32x4* src = xsrc + (long)chunk * 4 * xs_plane;
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            int piece = wave + 8 * i;
            piece = piece < NPIECE ? piece : NPIECE - 1;
            __builtin_amdgcn_global_load_lds((glb_ptr_t)(src + goff[i]), (lds_ptr_t)(smem + buf * BUF + piece * 1024), 16, 0, 0);
        }
        if constexpr (kK32) {                                // `chunk` is the first of a pair; a last chunk without a partner is copied alone
            if (chunk + 1 < a.nchunk) {
#pragma unroll
                for (int i = 0; i < PPW; ++i) {
                    int piece = wave + 8 * i;
                    piece = piece < NPIECE ? piece : NPIECE - 1;
                    __builtin_amdgcn_global_load_lds((glb_ptr_t)(src + 4 * xs_plane + goff[i]), (lds_ptr_t)(smem + buf * BUF + BUF1 + piece * 1024), 16, 0, 0);
                }
            }
        }
    };

    const int prr = TT ? nn >> 2 : nn >> 3, pcc = TT ? nn & 3 : nn & 7;   // this lane's position inside a tile
    // (kernel arguments the epilogue uses, read once: inside the lambda hipcc reloads them from the argument segment at every store)
    float* const out_ptr = a.out;
    const float* const part_ptr = a.partial;
    const bool out_bf16 = NHWC ? (a.out_act & 0xff) != 0 : a.out_act != 0;   // (the fp32 / bf16 instantiations: kActF32 or kActBF16)
    const bool vec_out = NHWC && (a.out_act & kNhwcVecOut) != 0;
    const int out_c = a.Cout, out_h = a.H, out_w = a.W;
    const float* bias_ptr = nullptr;
    const float* res_ptr = nullptr;
    const float* gate_ptr = nullptr;
    bool relu = false, vec_res = false, vec_gate = false;
    if constexpr (EPI) { bias_ptr = a.bias; relu = a.relu != 0; }
    // The residual's pointer and its alignment flag are read from the argument segment AFTER the tap loop (the empty asm ties the
    // address to a sum), as the exact gather reads its epilogue arguments.  Read up front with the bias pointer, they stay in SGPRs
    // across the loop, and tests/test_built_code.py (test_hot_kernels_touch_no_scratch_between_their_mfmas, at most 8 lane moves
    // between a kernel's first and last MFMA) then counted 10 in s3::split_gather_kernel<7 | kNhwcArg | kEpiArg, 2, true, false, true>,
    // the tall-tile NHWC ADD form; with the late read every form is within that test's limit again.
    auto read_residual = [&](float tie) __attribute__((always_inline)) {
        if constexpr (EPI) {
            unsigned long kargs = (unsigned long)__builtin_amdgcn_kernarg_segment_ptr();   // (the kernel's one parameter: offset 0)
            asm volatile("" : "+s"(kargs) : "v"(tie));
            const auto* late = reinterpret_cast<const __attribute__((address_space(4))) SplitArgsEpi*>(kargs);
            res_ptr = late->residual;
            vec_res = NHWC && late->res_vec != 0;
            gate_ptr = late->gate;
            vec_gate = NHWC && late->gate_vec != 0;
        }
    };
    // EPI: act((v + bias[f]) + r) of the value the store would have rounded (the channel clamped: a padded channel's value is not stored)
    auto finished = [&](float v, int f, float r) __attribute__((always_inline)) {
        const int fc = f < out_c ? f : out_c - 1;
        return epilogue_value(v, bias_ptr ? bias_ptr[fc] : 0.0f, bias_ptr != nullptr, relu, r, res_ptr != nullptr);
    };
    // element `o` of the residual or the gate, widened exactly from out's format
    auto element_at = [&](const float* ptr, long o) __attribute__((always_inline)) {
        if constexpr (H16) return load_act_t<kActF16>(ptr, o);
        else return out_bf16 ? load_act_t<kActBF16>(ptr, o) : ptr[o];
    };
    // NHWC: the four channels f0 .. f0 + 3 of pixel `pix` of the residual or the gate (vec: one load; else element loads, clamped address)
    auto load4 = [&](const float* ptr, bool vec, long pix, int f0, float (&r)[4]) __attribute__((always_inline)) {
        const long o = pix * out_c + f0;
        if (vec) {                                         // (Cout is a multiple of four: a group lies inside or outside as a whole)
            if (f0 < out_c) {
                if constexpr (H16) {
                    typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
                    const f16x4 q = *reinterpret_cast<const f16x4*>(reinterpret_cast<const unsigned short*>(ptr) + o);
#pragma unroll
                    for (int k = 0; k < 4; ++k) r[k] = (float)q[k];
                } else if (out_bf16) {
                    const uint2 q = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(ptr) + o);
                    r[0] = __uint_as_float(q.x << 16); r[1] = __uint_as_float(q.x & 0xffff0000u);
                    r[2] = __uint_as_float(q.y << 16); r[3] = __uint_as_float(q.y & 0xffff0000u);
                } else {
                    const float4 q = *reinterpret_cast<const float4*>(ptr + o);
                    r[0] = q.x; r[1] = q.y; r[2] = q.z; r[3] = q.w;
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {                  // (clamped address; the value is not stored)
                const int fc = f0 + k < out_c ? f0 + k : out_c - 1;
                r[k] = element_at(ptr, pix * out_c + fc);
            }
        }
    };
    // ADD: the GEMM's sum joins the ring pass's in fp32, and the store rounds THAT fp32 value once more.  Left to itself hipcc folds
    // the multiply-add into the binary16 store's conversion (v_fma_mixlo_f16), which rounds the exact sum to binary16 at once: not
    // always the binary16 rounding of what the fp32 plan stores.  The empty asm keeps the fp32 value a value.
    auto joined = [&](float s, float inv_w, float inv_x, float part) __attribute__((always_inline)) {
        float v = s * inv_w * inv_x + part;
        if constexpr (H16) asm("" : "+v"(v));
        return v;
    };
    // epilogue of four CONSECUTIVE output channels f0 .. f0 + 3 of pixel (y, x): the sums `s` as a lane holds them after either MFMA shape
    auto store4 = [&](int y, int x, bool tile, int f0, const float (&s)[4], float inv_w, float inv_x) __attribute__((always_inline)) {
        const long plane = (long)out_h * out_w;
        if (!(y < out_h && x < out_w && tile)) return;       // (RG = 1, odd NSUB: the second column half's last tile does not exist)
        if constexpr (NHWC) {
            const long pix = ((long)n * out_h + y) * out_w + x;
            float v[4];
            float r[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if constexpr (EPI) {
                if (res_ptr) load4(res_ptr, vec_res, pix, f0, r);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if constexpr (ADD) {
                    const int fc = f0 + k < out_c ? f0 + k : out_c - 1;      // (clamped address; the value is not stored)
                    v[k] = joined(s[k], inv_w, inv_x, part_ptr[((long)n * out_c + fc) * plane + (long)y * out_w + x]);
                } else {
                    v[k] = s[k] * inv_w * inv_x;
                }
                if constexpr (EPI) v[k] = finished(v[k], f0 + k, r[k]);
            }
            if constexpr (EPI) {
                if (gate_ptr) {
                    float g[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    load4(gate_ptr, vec_gate, pix, f0, g);
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = gate_value(v[k], g[k]);
                }
            }
            const long o = pix * out_c + f0;
            if (vec_out) {                                     // (Cout is a multiple of four: the whole group lies inside)
                if (f0 < out_c) {
                    if constexpr (H16) {
                        typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
                        *reinterpret_cast<f16x4*>(reinterpret_cast<unsigned short*>(out_ptr) + o) =
                            f16x4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
                    } else if (out_bf16) {
                        *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(out_ptr) + o) =
                            make_uint2(bf16_bits(v[0]) | (bf16_bits(v[1]) << 16), bf16_bits(v[2]) | (bf16_bits(v[3]) << 16));
                    } else {
                        *reinterpret_cast<float4*>(out_ptr + o) = make_float4(v[0], v[1], v[2], v[3]);
                    }
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (f0 + k < out_c) {
                        if constexpr (H16) store_act_t<kActF16>(out_ptr, o + k, v[k], false);
                        else store_act(out_ptr, o + k, v[k], out_bf16, false);
                    }
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int f = f0 + k;
                if (f < out_c) {
                    const long o = ((long)n * out_c + f) * plane + (long)y * out_w + x;
                    if constexpr (EPI) {
                        float v;
                        if constexpr (ADD) v = joined(s[k], inv_w, inv_x, part_ptr[o]);
                        else v = s[k] * inv_w * inv_x;
                        v = finished(v, f, res_ptr ? element_at(res_ptr, o) : 0.0f);
                        if (gate_ptr) v = gate_value(v, element_at(gate_ptr, o));
                        if constexpr (H16) store_act_t<kActF16>(out_ptr, o, v, false);
                        else store_act(out_ptr, o, v, out_bf16, false);
                    } else
                    if constexpr (ADD) {
                        const float v = joined(s[k], inv_w, inv_x, part_ptr[o]);
                        if constexpr (H16) store_act_t<kActF16>(out_ptr, o, v, false);
                        else store_act(out_ptr, o, v, out_bf16, false);
                    } else if constexpr (H16) store_act_t<kActF16>(out_ptr, o, s[k] * inv_w * inv_x, false);
                    else store_act(out_ptr, o, s[k] * inv_w * inv_x, out_bf16, false);
                }
            }
        }
    };
    auto body = [&](auto ntc) __attribute__((always_inline)) {
    constexpr int NT = decltype(ntc)::value;                 // tiles of this wave
    f32x16 sum[NT], acc[NT];                                 // running sums; the rows of taps being chained
    f32x16 zero;
#pragma unroll
    for (int i = 0; i < 16; ++i) zero[i] = 0.0f;
#pragma unroll
    for (int j = 0; j < NT; ++j) { sum[j] = zero; acc[j] = zero; }
    int rows_chained = 0;

    // A fragments: lane (nn, h) reads 16 bytes of channel fb*128 + fw*32 + nn; lo limb CoutP*2 units further
    const f16x8* wp = reinterpret_cast<const f16x8*>(a.wsd) + ((long)(fb * kDFB + fw * 32 + nn)) * 2 + h;
    const long wlo = (long)a.CoutP * 2, wtap = 2 * wlo;      // f16x8 units
    const unsigned lane_base = (unsigned)(h * HALF + ((prow + prr) * P + ptile * TW + pcc) * 16);

    // A wave whose four rows lie below the image (H = 28: the second half of the fourth row block) or whose 32 output channels lie
    // beyond Cout (96 channels padded to 128) has nothing to compute: it keeps copying its share of the windows and meeting the
    // barriers, and leaves the matrix pipe to its SIMD partner -- the kernel is bound by that pipe, so the workgroup finishes sooner.
#ifdef DAU_SPLIT_NO_IDLE_WAVES           // (timing experiment: tools/build_variant.sh)
    const bool live = true;
#else
    const bool live = rowb + prow < a.H && ptile < NSUB && colb + ptile * TW < a.W && fb * kDFB + fw * 32 < a.Cout;
#endif
    issue(0, 0);
    f16x8 ah[kDK], al[kDK], an[2], bn[2];                   // A fragments (hi, lo) of a row of taps; the next row's first two
    // (a fragment lives from its request to its tap, two taps on: the seventeen taps of the radius-8 line form need no more registers)
    static_assert(kAhead == 2 && kDK >= 5 && (kDK <= 9 || kLine), "the A ring below is written for two taps ahead");
#pragma unroll
    for (int i = 0; i < kAhead; ++i) { ah[i] = wp[i * wtap]; al[i] = wp[i * wtap + wlo]; }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int chunk = 0; chunk < a.nchunk; ++chunk) {
        const int buf = chunk & 1;
        if (chunk + 1 < a.nchunk) issue(chunk + 1, buf ^ 1);   // lands under this chunk's taps
        const unsigned bbase = lane_base + buf * BUF;
        // One row of taps per iteration, and NOTHING in flight across the back-edge: hipcc merges the wait-counter states at a loop
        // header conservatively (an LDS read or an A fragment carried over costs a wait for everything at its first use), so a row
        // starts with its own first hi read, and the next row's first two A fragments -- requested at taps 2 and 3, long landed --
        // are copied into place at the row's end.  Within a row: tap tx requests the A fragments of tap tx + 2 after its first
        // MFMA group, reads its lo fragments under the hi MFMAs and the next tap's hi fragments under the lo MFMAs.
#pragma unroll 1
        for (int ty = 0; ty < (live ? kDKV : 0); ++ty) {
            const unsigned brow = bbase + ty * P * 16;
            f16x8 xh[NT], xl[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) xh[j] = *reinterpret_cast<const f16x8*>(smem + brow + (TW * j) * 16);
#pragma unroll
            for (int tx = 0; tx < kDK; ++tx) {
#pragma unroll
                for (int j = 0; j < NT; ++j) xl[j] = *reinterpret_cast<const f16x8*>(smem + brow + 2 * HALF + (tx + TW * j) * 16);
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[tx], xh[j], (kFlushRows == 1 && tx % kFlushTaps == 0) ? zero : acc[j], 0, 0, 0);
                if (tx + kAhead < kDK) { ah[tx + kAhead] = wp[(tx + kAhead) * wtap]; al[tx + kAhead] = wp[(tx + kAhead) * wtap + wlo]; }
                if (tx == 2 || tx == 3) { an[tx - 2] = wp[(kDK + tx - 2) * wtap]; bn[tx - 2] = wp[(kDK + tx - 2) * wtap + wlo]; }
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[tx], xh[j], acc[j], 0, 0, 0);
                if (tx + 1 < kDK) {
#pragma unroll
                    for (int j = 0; j < NT; ++j) xh[j] = *reinterpret_cast<const f16x8*>(smem + brow + (tx + 1 + TW * j) * 16);
                }
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[tx], xl[j], acc[j], 0, 0, 0);
                // the order hipcc must keep (left alone it sinks every LDS read to just before its MFMA and waits for it there)
                if (tx == 0) __builtin_amdgcn_sched_group_barrier(0x100, 2 * NT, 0);
                else __builtin_amdgcn_sched_group_barrier(0x100, NT, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, NT, 0);
                if (tx == 2 || tx == 3) __builtin_amdgcn_sched_group_barrier(0x020, 4, 0);
                else if (tx + kAhead < kDK) __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, NT, 0);
                if (tx + 1 < kDK) __builtin_amdgcn_sched_group_barrier(0x100, NT, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, NT, 0);
                if ((tx + 1) % kFlushTaps == 0 && tx + 1 < kDK) {
#pragma unroll
                    for (int j = 0; j < NT; ++j) sum[j] += acc[j];
                }
            }
            wp += kDK * wtap;
            ah[0] = an[0]; al[0] = bn[0]; ah[1] = an[1]; al[1] = bn[1];
            if constexpr (kFlushRows == 1) {
#pragma unroll
                for (int j = 0; j < NT; ++j) sum[j] += acc[j];    // round-to-nearest adds of the row's partial sums
            } else {
                if (++rows_chained == kFlushRows) {
                    rows_chained = 0;
#pragma unroll
                    for (int j = 0; j < NT; ++j) { sum[j] += acc[j]; acc[j] = zero; }
                }
            }
        }
        if (chunk + 1 < a.nchunk) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the next window has landed (this wave's pieces; the barrier joins the rest)
            __syncthreads();
        }
    }

    if constexpr (kFlushRows > 1) {
#pragma unroll
        for (int j = 0; j < NT; ++j) sum[j] += acc[j];     // the chain in progress
    }
    // epilogue: C/D layout of the 32x32 tile: column (pixel) = lane & 31, row (channel) = (i & 3) + 8 (i >> 2) + 4 (lane >> 5)
    // the scales are undone by two exact power-of-two multiplies, 1 / sw then this image's 1 / sx[n]: their product may lie outside
    // the fp32 range where the result does not
    const float inv_w = a.sc->inv_sw, inv_x = scales_inv_sx(a.sc, a.N)[n];
    read_residual(sum[0][0]);
    const int y = rowb + prow + prr;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int x = colb + TW * (ptile + j) + pcc;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const float s4[4] = {sum[j][4 * g4], sum[j][4 * g4 + 1], sum[j][4 * g4 + 2], sum[j][4 * g4 + 3]};
            store4(y, x, ptile + j < NSUB, fb * kDFB + fw * 32 + 8 * g4 + 4 * h, s4, inv_w, inv_x);
        }
    }
    };
    // K32: one v_mfma_f32_16x16x32_f16 covers one tap of a PAIR of chunks.  Lane l = 16 g + q: K group g is half g & 1 of chunk
    // 2 c + (g >> 1), row / column q.  The wave's output tile is the same 32 channels x NT tiles of 32 pixels, as 2 channel halves m
    // (A row q = channel 16 m + q) x 2 NT pixel groups of 16 (B column q = pixel 16 (p & 1) + q of tile p >> 1: two rows of a 4 x 8
    // tile, four of a tall one), four accumulator registers each (C/D: pixel q, channel 16 m + 4 g + reg).  Both operands are the
    // planes and the WS rows of the 32x32x16 loop at one more per-lane offset: the second chunk's window lies BUF1 further in LDS, its
    // dense kernel kDTaps taps further in WS.  Per tap a wave loads 4 A fragments (2 m x hi, lo), reads 4 NT B fragments and issues
    // 12 NT MFMAs -- the bytes, LDS reads and matrix-pipe cycles of two steps of the other loop.
    // The A stream runs through buffer loads: a descriptor per row of taps (scalar base = the row's first tap in WS, records = what
    // is left of the real chunks from there), one 32-bit per-lane offset (channel, half, + one chunk for K groups 2 and 3) and scalar
    // offsets per tap -- no per-lane address arithmetic, and a load whose per-lane offset lies beyond the records returns zeros.
    // A last chunk WITHOUT a partner (an odd number of chunks) runs the same row of taps with K groups 2 and 3 idle: their A fragments
    // are those zeros (the absent chunk's rows lie beyond the records: nothing of them is read) and their B fragments repeat those
    // of groups 0 and 1 -- finite values add exact zeros, and a non-finite one meets there only the outputs it reaches anyway (every
    // channel of the pixels whose taps touch it), with nothing read from the absent chunk's window.
    auto body32 = [&](auto ntc) __attribute__((always_inline)) {
    constexpr int NT = decltype(ntc)::value;                 // tiles of this wave
    constexpr int NG = 2 * NT;                               // ... as groups of 16 pixels
    constexpr int U = kDK * NG;                              // (tap, group) units of a row of taps: 6 MFMAs each
    constexpr int GR = TT ? 4 : 2;                           // rows of a group
    f32x4 sum[NG][2], acc[NG][2];                            // running sums; the rows of taps being chained
    const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int p = 0; p < NG; ++p) { sum[p][0] = zero; sum[p][1] = zero; acc[p][0] = zero; acc[p][1] = zero; }
    int rows_chained = 0;
    const int g = lane >> 4, q = lane & 15;
    const int qr = TT ? q >> 2 : q >> 3, qc = TT ? q & 3 : q & 7;     // this lane's position inside a group
    const bool upper = g >= 2;                               // the K groups of a pair's second chunk

    // A fragments: lane (g, q) reads 16 bytes of channel fb*128 + fw*32 + 16 m + q; lo limb CoutP*2 units further
    const int wlo = a.CoutP * 32, wtap = 2 * wlo;            // bytes
    const long wchunk = (long)kDTaps * wtap, wend = a.nchunk * wchunk;
    const unsigned wlane = (unsigned)(((fb * kDFB + fw * 32 + q) * 2 + (g & 1)) * 16) + (upper ? (unsigned)wchunk : 0u);
    // descriptor of the WS rows from byte `off` on
    auto rows_from = [&](long off) __attribute__((always_inline)) {
        const long left = wend - off;
        const unsigned records = left <= 0 ? 0u : left > 0xffffffffl ? 0xffffffffu : (unsigned)left;
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(a.wsd)) + off, 0, records, 0x00020000);
    };
    auto load_a = [&](__amdgpu_buffer_rsrc_t rows, int soff, int m) __attribute__((always_inline)) {
        return __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(rows, wlane + 512 * m, soff, 0));
    };
    const unsigned lane_base = (unsigned)((g & 1) * HALF + ((prow + qr) * P + ptile * TW + qc) * 16);
#ifdef DAU_SPLIT_NO_IDLE_WAVES           // (timing experiment: tools/build_variant.sh)
    const bool live = true;
#else
    const bool live = rowb + prow < a.H && ptile < NSUB && colb + ptile * TW < a.W && fb * kDFB + fw * 32 < a.Cout;
#endif
    issue(0, 0);
    f16x8 ah[kDK][2], al[kDK][2], an[2][2], bn[2][2];       // A fragments (hi, lo) x m of a row of taps; the next row's first two
    static_assert(kAhead == 2 && kDK >= 5 && (kDK <= 9 || !kK32), "the A ring below is written for two taps ahead");
#pragma unroll
    for (int i = 0; i < kAhead; ++i) {
#pragma unroll
        for (int m = 0; m < 2; ++m) { ah[i][m] = load_a(rows_from(0), i * wtap, m); al[i][m] = load_a(rows_from(0), i * wtap + wlo, m); }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int npair = (a.nchunk + 1) >> 1;
    for (int pair = 0; pair < npair; ++pair) {
        const int buf = pair & 1;
        const bool more = pair + 1 < npair;
        if (more) issue(2 * pair + 2, buf ^ 1);              // lands under this pair's taps
        const bool lone = 2 * pair + 1 >= a.nchunk;
        const unsigned bbase = lane_base + buf * BUF + (lone || !upper ? 0u : (unsigned)BUF1);
        // One row of taps per iteration, and NOTHING in flight across the back-edge (see the 32x32x16 loop below).  Within a row the
        // B fragments run through a ring of three (tap, group) units: unit u reads the hi and lo fragments of unit u + 2 in front of
        // its six MFMAs (hi.hi, lo.hi, hi.lo for both channel halves) and drops its own after them; a tap's first unit requests the
        // A fragments of tap tx + 2 after its first two MFMAs; the next row's first two are requested at the row's last taps but one and
        // have landed at its end.
#pragma unroll 1
        for (int ty = 0; ty < (live ? kDKV : 0); ++ty) {
            const unsigned brow = bbase + ty * P * 16;
            const long wrow = 2 * pair * wchunk + (long)ty * kDK * wtap;
            const __amdgpu_buffer_rsrc_t wcur = rows_from(wrow);
            // the next row of taps (after a pair's last row: of the next pair)
            const __amdgpu_buffer_rsrc_t wnxt = rows_from(wrow + kDK * wtap + (ty == kDKV - 1 && more ? wchunk : 0));
            f16x8 xb[3][2];
            auto read = [&](int u, int limb) __attribute__((always_inline)) {
                const int tx = u / NG, p = u % NG;
                return *reinterpret_cast<const f16x8*>(smem + brow + limb * 2 * HALF + ((p & 1) * GR * P + tx + TW * (p >> 1)) * 16);
            };
            xb[0][0] = read(0, 0); xb[0][1] = read(0, 1); xb[1][0] = read(1, 0); xb[1][1] = read(1, 1);
            __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int tx = u / NG, p = u % NG;
                if (u + 2 < U) { xb[(u + 2) % 3][0] = read(u + 2, 0); xb[(u + 2) % 3][1] = read(u + 2, 1); }
                const f16x8 xh = xb[u % 3][0], xl = xb[u % 3][1];
                const f16x8 h0 = ah[tx][0], h1 = ah[tx][1], l0 = al[tx][0], l1 = al[tx][1];
                const bool fresh = kFlushRows == 1 && tx % kFlushTaps == 0;
                acc[p][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(h0, xh, fresh ? zero : acc[p][0], 0, 0, 0);
                acc[p][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(h1, xh, fresh ? zero : acc[p][1], 0, 0, 0);
                if (p == 0) {
                    if (tx + kAhead < kDK) {
#pragma unroll
                        for (int m = 0; m < 2; ++m) { ah[tx + kAhead][m] = load_a(wcur, (tx + kAhead) * wtap, m); al[tx + kAhead][m] = load_a(wcur, (tx + kAhead) * wtap + wlo, m); }
                    }
                    if (tx == kDK - 3 || tx == kDK - 2) {         // (where the row's own ring has a slot to spare)
                        const int i = tx - (kDK - 3);
#pragma unroll
                        for (int m = 0; m < 2; ++m) { an[i][m] = load_a(wnxt, i * wtap, m); bn[i][m] = load_a(wnxt, i * wtap + wlo, m); }
                    }
                }
                acc[p][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(l0, xh, acc[p][0], 0, 0, 0);
                acc[p][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(l1, xh, acc[p][1], 0, 0, 0);
                acc[p][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(h0, xl, acc[p][0], 0, 0, 0);
                acc[p][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(h1, xl, acc[p][1], 0, 0, 0);
                // the order hipcc must keep (left alone it sinks every LDS read to just before its MFMA and waits for it there)
                if (u + 2 < U) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
                if (p == 0 && tx + kAhead < kDK && tx == kDK - 3) __builtin_amdgcn_sched_group_barrier(0x020, 8, 0);
                else if (p == 0 && (tx + kAhead < kDK || tx == kDK - 2)) __builtin_amdgcn_sched_group_barrier(0x020, 4, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
                if ((tx + 1) % kFlushTaps == 0 && tx + 1 < kDK) { sum[p][0] += acc[p][0]; sum[p][1] += acc[p][1]; }
            }
#pragma unroll
            for (int m = 0; m < 2; ++m) { ah[0][m] = an[0][m]; al[0][m] = bn[0][m]; ah[1][m] = an[1][m]; al[1][m] = bn[1][m]; }
            if constexpr (kFlushRows == 1) {
#pragma unroll
                for (int p = 0; p < NG; ++p) { sum[p][0] += acc[p][0]; sum[p][1] += acc[p][1]; }   // round-to-nearest adds of the row's partial sums
            } else {
                if (++rows_chained == kFlushRows) {
                    rows_chained = 0;
#pragma unroll
                    for (int p = 0; p < NG; ++p) { sum[p][0] += acc[p][0]; sum[p][1] += acc[p][1]; acc[p][0] = zero; acc[p][1] = zero; }
                }
            }
        }
        if (more) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the next windows have landed (this wave's pieces; the barrier joins the rest)
            __syncthreads();
        }
    }
    if constexpr (kFlushRows > 1) {
#pragma unroll
        for (int p = 0; p < NG; ++p) { sum[p][0] += acc[p][0]; sum[p][1] += acc[p][1]; }   // the chain in progress
    }
    // epilogue: C/D layout of a 16x16 tile: column (pixel) = lane & 15, row (channel) = 4 (lane >> 4) + i; the scales as below
    const float inv_w = a.sc->inv_sw, inv_x = scales_inv_sx(a.sc, a.N)[n];
    read_residual(sum[0][0][0]);
#pragma unroll
    for (int p = 0; p < NG; ++p) {
        const int y = rowb + prow + (p & 1) * GR + qr, x = colb + TW * (ptile + (p >> 1)) + qc;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const float s4[4] = {sum[p][m][0], sum[p][m][1], sum[p][m][2], sum[p][m][3]};
            store4(y, x, ptile + (p >> 1) < NSUB, fb * kDFB + fw * 32 + 16 * m + 4 * g, s4, inv_w, inv_x);
        }
    }
    };
    // (both branches meet the same barriers: one per chunk)
    auto run = [&](auto ntc) __attribute__((always_inline)) {
        if constexpr (kK32) body32(ntc);
        else body(ntc);
    };
    if constexpr (TT) {
        if (pw == 0) run(std::integral_constant<int, NT0>{});
        else run(std::integral_constant<int, NT1>{});
    } else {
        run(std::integral_constant<int, NT0>{});
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
namespace {

template <int NSUB, int RG, bool TT>
constexpr size_t split_lds_bytes() {
    constexpr int plane = (4 * RG + kDSpanV) * (TT ? lds_pitch_narrow(NSUB) : lds_pitch(NSUB));
    return (kK32 ? 4 : 2) * (size_t)((4 * (kK32 ? (plane + 15) / 16 * 16 : plane) + 63) / 64) * 1024;
}

template <int NSUB, int RG, bool TT = false>
void launch_split(hipStream_t st, const SplitArgsEpi* a, int grid, bool h16, bool add, bool nhwc, bool epi) {
    constexpr int NH = NSUB | kNhwcArg;                      // the instantiations that store [N][H][W][Cout]
    constexpr int EP = NSUB | kEpiArg, EH = NH | kEpiArg;    // ... and those whose store is act(v + bias[f])
    constexpr size_t lds = split_lds_bytes<NSUB, RG, TT>();      // (a comma inside the launch macro's arguments would split them)
    if (epi) {
        auto kern = h16 ? split_gather_kernel<EP, RG, TT, true> : split_gather_kernel<EP, RG, TT, false>;
        if (nhwc) kern = h16 ? split_gather_kernel<EH, RG, TT, true> : split_gather_kernel<EH, RG, TT, false>;
#if DAU_SPLIT_R == 3
        if (add) kern = h16 ? split_gather_kernel<EP, RG, TT, true, true> : split_gather_kernel<EP, RG, TT, false, true>;
        if (add && nhwc) kern = h16 ? split_gather_kernel<EH, RG, TT, true, true> : split_gather_kernel<EH, RG, TT, false, true>;
#endif
        if (!a) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); return; }
        hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, st, *a);
        return;
    }
    auto kern = h16 ? split_gather_kernel<NSUB, RG, TT, true> : split_gather_kernel<NSUB, RG, TT, false>;
    if (nhwc) kern = h16 ? split_gather_kernel<NH, RG, TT, true> : split_gather_kernel<NH, RG, TT, false>;
#if DAU_SPLIT_R == 3
    if (add) kern = h16 ? split_gather_kernel<NSUB, RG, TT, true, true> : split_gather_kernel<NSUB, RG, TT, false, true>;
    if (add && nhwc) kern = h16 ? split_gather_kernel<NH, RG, TT, true, true> : split_gather_kernel<NH, RG, TT, false, true>;
#endif
    if (!a) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); return; }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, st, static_cast<const SplitArgs&>(*a));
}

void dispatch_split(int nsub, int rg, bool h16, hipStream_t st, const SplitArgsEpi* a, int grid, bool tall, bool add, bool nhwc, bool epi) {
    if (tall) {                                              // nsub = tiles of four columns: 5 or 7 (split_geometry)
        if (nsub == 5) launch_split<5, 2, true>(st, a, grid, h16, add, nhwc, epi);
        else launch_split<7, 2, true>(st, a, grid, h16, add, nhwc, epi);
        return;
    }
    if (rg == 1) {
        switch (nsub) {
            case 1: launch_split<1, 1>(st, a, grid, h16, add, nhwc, epi); break;
            case 2: launch_split<2, 1>(st, a, grid, h16, add, nhwc, epi); break;
            case 3: launch_split<3, 1>(st, a, grid, h16, add, nhwc, epi); break;
            default: launch_split<4, 1>(st, a, grid, h16, add, nhwc, epi); break;
        }
        return;
    }
    switch (nsub) {
        case 1: launch_split<1, 2>(st, a, grid, h16, add, nhwc, epi); break;
        case 2: launch_split<2, 2>(st, a, grid, h16, add, nhwc, epi); break;
        case 3: launch_split<3, 2>(st, a, grid, h16, add, nhwc, epi); break;
        default: launch_split<4, 2>(st, a, grid, h16, add, nhwc, epi); break;
    }
}

const void* stage_for(int blur_k, int act, bool nhwc = false) {
#define DAU_SPLIT_STAGE(K) case K: if (nhwc) return act == kActF16 ? reinterpret_cast<const void*>(split_stage_kernel<K | kNhwcArg, kActF16>) : \
                                          act == kActBF16 ? reinterpret_cast<const void*>(split_stage_kernel<K | kNhwcArg, kActBF16>) : \
                                                            reinterpret_cast<const void*>(split_stage_kernel<K | kNhwcArg, kActF32>); \
                                   return act == kActF16 ? reinterpret_cast<const void*>(split_stage_kernel<K, kActF16>) : \
                                          act == kActBF16 ? reinterpret_cast<const void*>(split_stage_kernel<K, kActBF16>) : \
                                                            reinterpret_cast<const void*>(split_stage_kernel<K, kActF32>)
    switch (blur_k) {
        DAU_SPLIT_STAGE(3);
        DAU_SPLIT_STAGE(5);
        DAU_SPLIT_STAGE(7);
        DAU_SPLIT_STAGE(9);
        DAU_SPLIT_STAGE(11);
        default: return nullptr;                 // wider prefilters: no split form (the exact gather runs)
    }
#undef DAU_SPLIT_STAGE
}
// the walking form of the staging: NCHW inputs (-DDAU_SPLIT_STAGE_REF: never)
const void* stage_walk_for(int blur_k, int act) {
#ifdef DAU_SPLIT_STAGE_REF
    return nullptr;
#else
#define DAU_SPLIT_STAGE_WALK(K) case K: return act == kActF16 ? reinterpret_cast<const void*>(split_stage_walk_kernel<K, kActF16>) : \
                                               act == kActBF16 ? reinterpret_cast<const void*>(split_stage_walk_kernel<K, kActBF16>) : \
                                                                 reinterpret_cast<const void*>(split_stage_walk_kernel<K, kActF32>)
    switch (blur_k) {
        DAU_SPLIT_STAGE_WALK(3);
        DAU_SPLIT_STAGE_WALK(5);
        DAU_SPLIT_STAGE_WALK(7);
        DAU_SPLIT_STAGE_WALK(9);
        DAU_SPLIT_STAGE_WALK(11);
        default: return nullptr;
    }
#undef DAU_SPLIT_STAGE_WALK
#endif
}
// Its tiles and bands.  The staged row in equal tiles of at most 64 columns.  One band -- a wave walks the whole plane -- where that
// already gives the box two waves per SIMD (2048: the north-star pass is 4096 waves of 68 steps); smaller passes cut the plane into
// bands of at least 2 K rows (a band filters the K - 1 rows around it again).
void stage_walk_plan(const DenseConfig& c, const SplitGeom& g, SplitStageArgs* s) {
    s->nsegs = (g.Ws + 63) / 64;
    s->TW = (g.Ws + s->nsegs - 1) / s->nsegs;
    s->nsegs = (g.Ws + s->TW - 1) / s->TW;
    const long waves = (long)c.N * 2 * g.nchunk * s->nsegs;
    long nb = (2048 + waves - 1) / waves;
    nb = std::min<long>(nb, std::max(1, g.Hs / (2 * c.blur_k)));
    const int rb = DAU_TUNE_INT("DAU_SPLIT_STAGE_WALK_RB", 0);   // tuning build: staged rows per band
    s->RB = rb > 0 ? rb : (int)((g.Hs + nb - 1) / nb);
    s->nbands = (g.Hs + s->RB - 1) / s->RB;
}
// bands of rows whose raw window (eight channels, rows of kSP floats) stays below ~52 KiB of LDS: three workgroups per CU
void stage_plan(const DenseConfig& c, int* RB, int* nbands, size_t* lds) {
    const int kr = (c.blur_k - 1) / 2;
    int rows = 52 * 1024 / (8 * kSP * 4) - 2 * kr;
    const int rb = DAU_TUNE_INT("DAU_SPLIT_STAGE_RB", 0);
    if (rb > 0) rows = rb;
    rows = rows < 4 ? 4 : rows;
    const int nb = (c.H + rows - 1) / rows;
    *nbands = nb; *RB = (c.H + nb - 1) / nb;
    *lds = (size_t)(*RB + 2 * kr) * 8 * kSP * 4;
}

}  // namespace

bool split_gather_configure(int N, int Cin, int Cout, int G, int H, int W, int R, int blur_k, int act, DenseConfig* cfg) {
    if (R != kDR || !stage_for(blur_k, act)) return false;
    DenseConfig c{};
    c.N = N; c.Cin = Cin; c.Cout = Cout; c.G = G; c.H = H; c.W = W; c.R = R; c.blur_k = blur_k; c.act = act;
    const SplitGeom g = split_geometry(c);
    c.nsub = g.nsub_a;
    c.ftiles = 1;
    // 32-bit unit offsets inside one image's staged planes
    if ((size_t)g.nchunk * 4 * g.Hs * g.Ws > (size_t)1 << 30) return false;
    *cfg = c;
    return true;
}

size_t split_gather_workspace_bytes(const DenseConfig& c) {
    const SplitGeom g = split_geometry(c);
    return g.hdr_bytes + g.xs_bytes + g.ws_bytes;
}

void split_gather_init(const DenseConfig& c) {
    const SplitGeom g = split_geometry(c);
    const bool h16 = c.act == kActF16;
    for (int rg = 1; rg <= 2; ++rg) {
        if (!(rg == 2 ? g.nrb8 : g.nrb4)) continue;
        for (int v = 0; v < (kDR == 3 ? 4 : 2); ++v) {           // (the radius-3 form also exists with the ring pass's partial sums added; every form with the fused epilogue)
            const bool add = (v & 2) != 0, epi = (v & 1) != 0;
            if (rg == 2 && g.tall) { dispatch_split(g.tall, 2, h16, nullptr, nullptr, 0, true, add, c.nhwc != 0, epi); continue; }
            dispatch_split(g.nsub_a, rg, h16, nullptr, nullptr, 0, false, add, c.nhwc != 0, epi);
            if (g.nb_b) dispatch_split(g.nsub_b, rg, h16, nullptr, nullptr, 0, false, add, c.nhwc != 0, epi);
        }
    }
    (void)hipFuncSetAttribute(stage_for(c.blur_k, c.act, c.nhwc != 0), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}

void split_gather_prepare(hipStream_t st, const DenseConfig& c, const float* in, const float* filters, bool mirrored,
                          const UnitRef* table, void* workspace, const Guard& guard) {
    const SplitGeom g = split_geometry(c);
    char* ws = static_cast<char*>(workspace);
    SplitScales* sc = reinterpret_cast<SplitScales*>(ws);
    unsigned* partial = reinterpret_cast<unsigned*>(ws + scales_bytes(c.N));
    _Float16* xs = reinterpret_cast<_Float16*>(ws + g.hdr_bytes);
    _Float16* wsd = reinterpret_cast<_Float16*>(ws + g.hdr_bytes + g.xs_bytes);
    const long per = (long)c.Cin * c.H * c.W, units = (long)c.Cin * c.G * c.Cout;
    const int gpi = absmax_groups_per_image(c.N, per), cap = kPartials + c.N;
    hipLaunchKernelGGL(split_absmax_kernel, dim3(c.N * gpi), dim3(256), 0, st, in, per, gpi, c.act, table, units, partial, cap, guard,
                       (c.in_relu && !mirrored) ? 1 : 0);
    hipLaunchKernelGGL(split_scales_kernel, dim3(c.N + 1), dim3(256), 0, st, partial, c.N, gpi, cap, c.G, sc, guard);
    hipLaunchKernelGGL(split_densify_kernel, dim3(g.nchunk * (g.CoutP / (kScT / 16))), dim3(kScT), 0, st, table, c.Cin, c.G, c.Cout, g.CoutP,
                       g.nchunk, sc, wsd, guard);
    SplitStageArgs s{};
    s.in = in; s.taps = filters + kTaps1dOffset; s.sc = sc; s.xs = xs;
    s.N = c.N; s.C = c.Cin; s.H = c.H; s.W = c.W; s.mirrored = mirrored ? 1 : 0;
    s.Hs = g.Hs; s.Ws = g.Ws; s.nchunk = g.nchunk; s.guard = guard;
    s.relu_in = (c.in_relu && !mirrored) ? 1 : 0;
    if (const void* walk = c.nhwc ? nullptr : stage_walk_for(c.blur_k, c.act)) {
        stage_walk_plan(c, g, &s);
        void* args[] = {&s};
        (void)hipLaunchKernel(walk, dim3(c.N * 2 * g.nchunk * s.nbands * s.nsegs), dim3(64), args, 0, st);
        return;
    }
    size_t lds;
    stage_plan(c, &s.RB, &s.nbands, &lds);
    s.nsegs = (c.W + 63) / 64;
    s.vec = c.W % 4 == 0 && reinterpret_cast<uintptr_t>(in) % 16 == 0;
    if (c.nhwc) s.vec = c.Cin % (c.act == kActF32 ? 4 : 8) == 0 && reinterpret_cast<uintptr_t>(in) % 16 == 0;   // 16-byte pieces of a pixel's channels
    void* args[] = {&s};
    (void)hipLaunchKernel(stage_for(c.blur_k, c.act, c.nhwc != 0), dim3(c.N * 2 * g.nchunk * s.nbands * s.nsegs), dim3(kStageThreads), args, lds, st);
}

namespace {
// partial != nullptr (radius 3): the ADD instantiations
void run_split(hipStream_t st, const DenseConfig& c, float* out, const float* partial, void* workspace, const Guard& guard,
               const Epilogue& epilogue) {
    const SplitGeom g = split_geometry(c);
    const bool add = partial != nullptr;
    const bool h16 = c.act == kActF16;
    char* ws = static_cast<char*>(workspace);
    SplitArgsEpi a{};
    a.sc = reinterpret_cast<const SplitScales*>(ws);
    a.xs = reinterpret_cast<const _Float16*>(ws + g.hdr_bytes);
    a.wsd = reinterpret_cast<const _Float16*>(ws + g.hdr_bytes + g.xs_bytes);
    a.out = out; a.partial = partial;
    a.N = c.N; a.Cout = c.Cout; a.CoutP = g.CoutP; a.H = c.H; a.W = c.W; a.Hs = g.Hs; a.Ws = g.Ws; a.nchunk = g.nchunk;
    a.out_act = c.act; a.guard = guard;
    a.bias = epilogue.bias; a.relu = epilogue.relu ? 1 : 0; a.residual = epilogue.residual;
    const bool epi = epilogue.on();
    const bool nhwc = c.nhwc != 0;
    if (nhwc && c.Cout % 4 == 0 && reinterpret_cast<uintptr_t>(out) % (c.act == kActF32 ? 16 : 8) == 0) a.out_act |= kNhwcVecOut;
    // (the residual is another allocation: its own base decides whether its groups of four channels are loaded at once)
    a.res_vec = epilogue.residual && nhwc && c.Cout % 4 == 0 && reinterpret_cast<uintptr_t>(epilogue.residual) % (c.act == kActF32 ? 16 : 8) == 0;
    a.gate = epilogue.gate;
    a.gate_vec = epilogue.gate && nhwc && c.Cout % 4 == 0 && reinterpret_cast<uintptr_t>(epilogue.gate) % (c.act == kActF32 ? 16 : 8) == 0;
    for (int rg = 2; rg >= 1; --rg) {                        // the eight-row blocks, then the block of four rows where there is one
        a.nrb = rg == 2 ? g.nrb8 : g.nrb4;
        if (!a.nrb) continue;
        a.row0 = rg == 2 ? 0 : g.nrb8 * kDRows;
        if (rg == 2 && g.tall) {                             // one column block of tall tiles
            a.ncb = 1; a.col0 = 0;
            dispatch_split(g.tall, 2, h16, st, &a, c.N * a.nrb * (g.CoutP / kDFB), true, add, nhwc, epi);
            continue;
        }
        a.ncb = g.nb_a; a.col0 = 0;
        dispatch_split(g.nsub_a, rg, h16, st, &a, c.N * a.nrb * g.nb_a * (g.CoutP / kDFB), false, add, nhwc, epi);
        if (g.nb_b) {
            a.ncb = g.nb_b; a.col0 = g.nb_a * g.nsub_a * 8;
            dispatch_split(g.nsub_b, rg, h16, st, &a, c.N * a.nrb * g.nb_b * (g.CoutP / kDFB), false, add, nhwc, epi);
        }
    }
}
}  // namespace

void split_gather_run(hipStream_t st, const DenseConfig& c, float* out, void* workspace, const Guard& guard, const Epilogue& epi) {
    run_split(st, c, out, nullptr, workspace, guard, epi);
}

#if DAU_SPLIT_R == 3
void split_gather_run_add(hipStream_t st, const DenseConfig& c, float* out, const float* partial, void* workspace, const Guard& guard,
                          const Epilogue& epi) {
    run_split(st, c, out, partial, workspace, guard, epi);
}

SplitStaged split_gather_staged(const DenseConfig& c, const void* workspace) {
    const SplitGeom g = split_geometry(c);
    const char* ws = static_cast<const char*>(workspace);
    SplitStaged s{};
    s.sx = scales_sx(reinterpret_cast<const SplitScales*>(ws));
    s.xs = reinterpret_cast<const _Float16*>(ws + g.hdr_bytes);
    s.Hs = g.Hs; s.Ws = g.Ws; s.nchunk = g.nchunk;
    return s;
}
#endif

}  // namespace DAU_SPLIT_NS
}  // namespace dau
