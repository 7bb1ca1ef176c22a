// Parameter gradients (gather-dot) on the f16 matrix cores at fp32 accuracy: two-limb GEMM, bilinear corners as rows.
//
//   r_k[u] = sum_{n,p} E'[n,f,p] * sum_d b_d(u) Xk[n,s,k, p + o_u + d]          (u = (s, g, f), d in {0,1}^2)
//          = sum_d b_d(u) * D[(k,d), u],   D[(k,d), u] = sum_{n,q} Xk[n,s,k, q + d] * E'[n,f, q - o_u]
//
// (q = p + o_u).  For one input channel s, D is a GEMM: M = 16 rows (k, d) that do not depend on the unit, N = the units of s,
// K = (position q, image).  It runs as v_mfma_f32_16x16x32_f16 with both operands split into two binary16 limbs (hi = f16(v),
// lo = f16(v - hi), three products hi*hi + lo*hi + hi*lo, fp32 sums), as the two-limb gather-sum does (k_dense_split.hip).
//  * Fragments.  Lane l holds A row l % 16 = 4k + d and B column l % 16 for the K group l / 16 = one position x 8 images, and
//    receives D rows 4(l / 16) .. +3: the four corners d of kind k = l / 16 of its unit.  The bilinear combination is lane-local.
//  * No interpolation in the loop; the FLOPs do not depend on the offsets -- only the halo of the error window does.  One radius
//    (4, the layer's clip of 3.99 included) serves every call within +-4.
//  * Staging (8 images innermost, so that a 16-byte fragment is aligned at any displacement):
//      XS[oct][s][k][Ty][Tx][limb][8 img]   Ty, Tx = image position + 1 (a zero row / column in front for the corner d = 0 of q = -1)
//      ES[oct][fb][Vy][Vx][limb][16 f][8 img]   Vy, Vx = image position + R + 1, zero halo, the unit_testing edge rule applied
//      ES1[oct][fb][Vy][Vx][16 f][8 img]        the same with the hi limb only: bf16 activations (below)
//    Exact power-of-two scales per (s, k) and per f bring each maximum to [2^13, 2^14); the maxima are taken over finite values only
//    (an Inf / NaN does not remove the scaling of the other channels).  The epilogue undoes them exactly.
//    XS comes straight from x where the plan allows (sd_xk_walk_kernel below: the filter computed twice, no fp32 copy in between);
//    other plans filter into the fp32 copy XK (blur4_pack_kernel<K, true>, which also takes the maxima) and split it (sd_stage_x_kernel).
//  * Main kernel.  Workgroup = (chunk of (image octet, region) items, 16 output channels, 16 input channels, 4 units); region =
//    4 rows x RW columns of q; the ES window of the 16 channels (RH + 2R rows x RW + 2R columns x 512 B) sits in LDS as a ring of
//    rows, the items walking down column strips so that each copies only its RH new rows, one item ahead.  A wave owns
//    2 input channels x 4 units = 8 tiles of 16 units (s, g, the block's 16 f) for the whole kernel.  Lane group j = row j of
//    the region, K step = one column: every address is a per-lane base plus an immediate.
//  * A operand.  A lane's row is m = 4 k + 2 dy + dx: at K step c + 1 the lane with dx = 0 needs the 32 bytes its quad neighbour
//    (dx = 1) held at step c.  Each Xk column is therefore loaded once per wave, per PAIR of K steps, and the odd step's fragment
//    is built from the neighbour's registers with one select and one quad-permute DPP move per dword (no LDS traffic):
//    RW / 2 + 1 loads per item, channel and limb instead of RW (the + 1: column RW of the item's own rows for the last step).
//  * Bank conflicts.  The LDS window is position-major with the 16 output channels of a position in consecutive 16-byte groups, so
//    the bank group of a ds_read_b128 is (lane % 16) whatever the unit's displacement: every read phase of 16 lanes touches 16
//    distinct groups.  The unit-to-lane placement (lane % 16 = f % 16) is conflict-free by construction; no placement table.
//  * Thin items.  Where H + 1 = 4 n + 1 (every map whose height is a multiple of four) the last region of a strip holds one real
//    row; that item takes the row's columns four at a time as its K groups: ceil(RW / 4) K steps instead of RW (sd_dot_body).
//  * Accuracy.  Per item a tile's accumulator chains 3 x RW MFMAs (hierarchical accumulation, as in the gather-sum); the bilinear
//    combination joins a running fp32 sum per unit, flushed every few items into the float partial sums [chunk][4][S][G][F] with a
//    no-return atomic add (the slot belongs to one lane: the program's order), summed over the chunks in double (dot_reduce).
//  * bf16 activations (SplitDotConfig::e_limbs = 1).  A bf16 dy has 8 significant bits: times its channel's power-of-two scale it
//    IS its binary16 hi limb (down to the f16 subnormal grid, 2^-27 of the channel's maximum; smaller values round to that grid)
//    and its lo limb is zero.  The product hi_x * lo_e therefore adds nothing: the error is staged in one limb (ES1, 256 B per
//    window position instead of 512: half the window copy, half the ring) and a tile takes two MFMAs per K step instead of
//    three (sd_e1_dot_kernel).  Xk is blurred in fp32 and keeps its two limbs.  Every accumulator chain is that of the
//    three-product kernel on the widened values with its zero products left out: the same bits.
#include <algorithm>
#include <cfloat>

#include "dau_tiled.hpp"

// The line forms (-DDAU_SD_1D with -DDAU_SD_RX=4 / 8 and -DDAU_SD_NS=d4 / d8; DAU_FLAG_SPLIT_DOT_LINE): the same GEMM for calls whose
// units all lie on the row of their pixel (oy == 0 and no factor on the row below: the call's device guard decides), i.e. the
// parameter gradients of single-dimension layers.  The horizontal radius of the error window is RX, the vertical one 0: no halo
// rows in ES or in the LDS ring (2 RH = 8 slots, every row of an item new), which leaves room for RX = 8.  The corners dy = 1
// are left out of the bilinear combination (their A rows repeat the dy = 0 rows): half of a tile's rows carry no result.
// The plain object is the 2-D member (radius 4 both ways), its kernels the bytes they were.
#ifndef DAU_SD_RX
#define DAU_SD_RX 4
#endif
#ifndef DAU_SD_1D
#define DAU_SD_1D 0
#endif
// The kernels of the line forms are named ld_*_kernel / line_dot_kernel (d4::line_dot_kernel, ...): tools and the built-code
// tests pick the 2-D member's kernels by the names below.  EVERY __global__ function of this file is listed here.
#if DAU_SD_1D
#define sd_zero_kernel ld_zero_kernel
#define sd_absmax_x_kernel ld_absmax_x_kernel
#define sd_absmax_e_kernel ld_absmax_e_kernel
#define sd_absmax_nhwc_e_kernel ld_absmax_nhwc_e_kernel
#define sd_stage_x_kernel ld_stage_x_kernel
#define sd_xk_walk_kernel ld_xk_walk_kernel
#define sd_stage_e_kernel ld_stage_e_kernel
#define sd_stage_e1_kernel ld_stage_e1_kernel
#define sd_stage_nhwc_e_kernel ld_stage_nhwc_e_kernel
#define split_gather_dot_kernel line_dot_kernel
#define sd_e1_dot_kernel line_e1_dot_kernel
#endif

namespace dau {
#ifdef DAU_SD_NS
namespace DAU_SD_NS {
#endif

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f4s __attribute__((ext_vector_type(4)));

namespace {

constexpr int kSdWaves = 8;             // waves per workgroup (two per SIMD)
constexpr int kSdAS = 2;                // input channels per wave (four spill the accumulators)
constexpr int kSdGT = 4;                // units per (input channel, output channel) in one workgroup
constexpr int kSdSB = kSdWaves * kSdAS; // input channels per workgroup
constexpr int kSdFB = 16;               // output channels per workgroup = B columns of a tile
constexpr bool kSdLine = DAU_SD_1D != 0;
constexpr int kSdRX = DAU_SD_RX;        // offset radius of the error window: horizontal,
constexpr int kSdRY = kSdLine ? 0 : kSdRX;   // vertical (a line form has no rows above or below)
constexpr int kSdRH = 4;                // region rows = K groups of one MFMA
constexpr int kSdFlushItems = 16;       // items per flush of the running sums (at most 16 float additions per slot and chunk)
// s_waitcnt immediates (gfx9 encoding: vmcnt in bits 3:0, expcnt 6:4 and lgkmcnt 11:8 left at their maxima)
constexpr unsigned kVmcnt0 = 0x0F70, kVmcnt8 = 0x0F78;

inline size_t rup(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

// Thin items: where the H + 1 rows of q leave ONE real row in a strip's last region ((H + 1) % 4 == 1: every map whose height is a
// multiple of four), that item takes its row's columns four at a time as the K groups of an MFMA, ceil(RW / 4) K steps instead
// of RW (sd_dot_body).  -DDAU_SD_NO_THIN (libdau_conv_hip_no_thin.so of `make tuning`) runs every item in full: the A/B partner
// and, for shapes without such a row, the bit-exact reference of tests/test_gpu_split_dot_thin_row.py.
#ifdef DAU_SD_NO_THIN
constexpr bool kSdThin = false;
#else
constexpr bool kSdThin = true;
#endif

struct SdGeom {
    int Hq, Wq, rq, cq, XTr, XTc, EYs, EXs, octs, nfb, nsb, ngb, items, chunks, per, NP;
    int thin;               // the last region of every strip is a thin item
    int strip_steps;        // K steps of a column strip of regions
};

SdGeom sd_geom(const SplitDotConfig& c) {
    const Shape& s = c.sh;
    SdGeom g{};
    g.Hq = (s.H + 1 + kSdRH - 1) / kSdRH * kSdRH;
    g.Wq = (s.W + 1 + c.RW - 1) / c.RW * c.RW;
    g.rq = g.Hq / kSdRH; g.cq = g.Wq / c.RW;
    g.thin = kSdThin && (s.H + 1) % kSdRH == 1 && g.rq >= 2;
    g.strip_steps = (g.rq - g.thin) * c.RW + g.thin * ((c.RW + kSdRH - 1) / kSdRH);
    g.XTr = g.Hq + 1; g.XTc = g.Wq + 1;
    g.EYs = g.Hq + 2 * kSdRY; g.EXs = g.Wq + 2 * kSdRX;
    g.octs = (s.N + 7) / 8;
    g.NP = (s.N + 1) / 2;
    g.nfb = (s.F + kSdFB - 1) / kSdFB;
    g.nsb = (s.S + kSdSB - 1) / kSdSB;
    g.ngb = (s.G + kSdGT - 1) / kSdGT;
    g.items = g.octs * g.rq * g.cq;
    // about four rounds of one workgroup per CU (the LDS window leaves room for one), no chunk without items
    const int per_chunk = g.nfb * g.nsb * g.ngb;
    int chunks = (1024 + per_chunk - 1) / per_chunk;
    chunks = std::max(1, std::min(chunks, g.items));
    g.per = (g.items + chunks - 1) / chunks;
    g.chunks = (g.items + g.per - 1) / g.per;
    return g;
}

struct SdLayout { size_t maxes_off, xk_off, xs_off, es_off, partial_off, total; };

SdLayout sd_layout(const SplitDotConfig& c, const SdGeom& g) {
    const Shape& s = c.sh;
    SdLayout l{};
    size_t off = 0;
    l.maxes_off = off; off += rup((size_t)(s.S * kNumK + s.F) * 4);
    l.xk_off = off; off += rup((size_t)g.NP * s.S * s.H * s.W * 32);                              // blur4_pack output, fp32
    // + one position: the pair load of column Wq (sd_next_col) reads, unused, the position after the last plane's last column
    l.xs_off = off; off += rup((size_t)g.octs * s.S * kNumK * g.XTr * g.XTc * 32 + 32);
    l.es_off = off; off += rup((size_t)g.octs * g.nfb * g.EYs * g.EXs * 256 * c.e_limbs);
    l.partial_off = off; off += rup((size_t)g.chunks * kNumK * s.S * s.G * s.F * 4);
    l.total = off;
    return l;
}

// power-of-two scale exponent that brings a maximum (float bits, finite, >= 0) to [2^13, 2^14); 0 for a zero maximum
__device__ __forceinline__ int sd_shift(unsigned maxbits) {
    if (maxbits == 0u) return 0;
    const int e = (int)(maxbits >> 23) - 127;          // denormal maxima count as 2^-127: the shift is clamped below
    const int sh = 13 - e;
    return sh > 120 ? 120 : sh;
}

__device__ __forceinline__ bool finite_abs(float v, float* a) {
    *a = fabsf(v);
    return *a <= FLT_MAX;
}

// On the XK chain max |Xk| per (input channel, kind) is taken by blur4_pack itself while it writes XK (launch_blur4_pack's kmax).
// -DDAU_SD_STAGE_REF (libdau_conv_hip_stage_ref.so of `make tuning`) keeps the staging that came before: this pass over XK and
// the sd_stage_e_kernel with one thread per position -- the bit-exact reference of tests/test_gpu_split_dot_stage_fused.py and
// the A side of kernel-level timings.
#ifdef DAU_SD_STAGE_REF
// max |Xk| per (input channel, kind) over the fp32 staging of blur4_pack ([NP][S][H][W][4 kinds][2 images]): grid (S, split)
__global__ void __launch_bounds__(256) sd_absmax_x_kernel(const float* __restrict__ xk, int NP, int S, int HW, int split,
                                                          unsigned* __restrict__ xmax, const Guard guard) {
    if (!guard_pass(guard)) return;
    const int s = blockIdx.x % S, part = blockIdx.x / S;
    float m[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const long per_np = (long)HW * 2;                    // float4 per (np, s) plane: HW positions x 8 floats / 4
    const long total = (long)NP * per_np;
    for (long i = part * 256L + threadIdx.x; i < total; i += 256L * split) {
        const long np = i / per_np, r = i - np * per_np;
        const float4 v = reinterpret_cast<const float4*>(xk + ((size_t)np * S + s) * HW * 8)[r];
        const int k0 = (int)(r & 1) * 2;                 // float4 0 of a position: kinds 0, 1; float4 1: kinds 2, 3
        float a;
        if (finite_abs(v.x, &a)) m[k0] = fmaxf(m[k0], a);
        if (finite_abs(v.y, &a)) m[k0] = fmaxf(m[k0], a);
        if (finite_abs(v.z, &a)) m[k0 + 1] = fmaxf(m[k0 + 1], a);
        if (finite_abs(v.w, &a)) m[k0 + 1] = fmaxf(m[k0 + 1], a);
    }
    // (per thread both parities of r visit the same kinds only if the stride is even: 256 * split is)
    __shared__ float red[4][256];
    for (int k = 0; k < 4; ++k) red[k][threadIdx.x] = m[k];
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int k = 0; k < 4; ++k) red[k][threadIdx.x] = fmaxf(red[k][threadIdx.x], red[k][threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x < 4) atomicMax(&xmax[s * kNumK + threadIdx.x], __float_as_uint(red[threadIdx.x][0]));
}
#endif

// A line form's guard has passed: this member does the pass's work (dau_conv_dot_line_status reports it).  The one write a kernel
// of this file makes through its guard (dau_common.hpp, Guard): one thread of the pass's dy maxima kernel.
__device__ __forceinline__ void sd_mark_taken(const Guard& guard) {
    if constexpr (kSdLine) {
        if (guard.status && blockIdx.x == 0 && threadIdx.x == 0) const_cast<Status*>(guard.status)->dot_line_radius = (unsigned)kSdRX;
    }
}

// the pass's maxima and partial sums start from zero (unguarded, as the memsets it stands for were)
__global__ void __launch_bounds__(256) sd_zero_kernel(unsigned* __restrict__ a, long na, unsigned* __restrict__ b, long nb) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < na + nb; i += (long)gridDim.x * 256L) {
        if (i < na) a[i] = 0u;
        else b[i - na] = 0u;
    }
}

// max |dy| per output channel: grid (F, split); dy is fp32, f16 or bf16 (act)
__global__ void __launch_bounds__(256) sd_absmax_e_kernel(const float* __restrict__ dy, int N, int F, int HW, int split, int act,
                                                          unsigned* __restrict__ emax, const Guard guard) {
    if (!guard_pass(guard)) return;
    sd_mark_taken(guard);
    const int f = blockIdx.x % F, part = blockIdx.x / F;
    float m = 0.0f;
    const long total = (long)N * HW;
    for (long i = part * 256L + threadIdx.x; i < total; i += 256L * split) {
        const long n = i / HW, p = i - n * HW;
        float a;
        if (finite_abs(load_act(dy, ((long)n * F + f) * HW + p, act), &a)) m = fmaxf(m, a);
    }
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) atomicMax(&emax[f], __float_as_uint(m));
}

// the same maxima from an [N][H][W][F] dy (DAU_FLAG_IO_NHWC): a workgroup takes 64 consecutive channels, a lane one of them, and its
// four waves every fourth pixel of the workgroup's share; grid (ceil(F / 64), split).  A maximum does not depend on the order.
__global__ void __launch_bounds__(256) sd_absmax_nhwc_e_kernel(const float* __restrict__ dy, int N, int F, int HW, int split, int act,
                                                               unsigned* __restrict__ emax, const Guard guard) {
    if (!guard_pass(guard)) return;
    sd_mark_taken(guard);
    const int nfb = (F + 63) / 64;
    const int f = (blockIdx.x % nfb) * 64 + (threadIdx.x & 63), part = blockIdx.x / nfb;
    if (f >= F) return;
    float m = 0.0f;
    const long total = (long)N * HW;
    for (long i = part * 4L + (threadIdx.x >> 6); i < total; i += 4L * split) {
        float a;
        if (finite_abs(load_act(dy, i * F + f, act), &a)) m = fmaxf(m, a);
    }
    atomicMax(&emax[f], __float_as_uint(m));
}

__device__ __forceinline__ void split_limbs(float v, _Float16* hi, _Float16* lo) {
    const _Float16 h = (_Float16)v;
    const float hf = (float)h;
    *hi = h;
    *lo = (hf - hf == 0.0f) ? (_Float16)(v - hf) : (_Float16)0.0f;   // a non-finite value keeps its hi limb only
}

// XS[oct][s][k][Ty][Tx][limb][8] from the fp32 staging: one thread per (oct, s, Ty, Tx), all four kinds
__global__ void __launch_bounds__(256) sd_stage_x_kernel(const float* __restrict__ xk, const unsigned* __restrict__ xmax, int N,
                                                         int NP, int S, int H, int W, int octs, int XTr, int XTc,
                                                         h8* __restrict__ xs, const Guard guard) {
    if (!guard_pass(guard)) return;
    const long total = (long)octs * S * XTr * XTc;
    for (long idx = blockIdx.x * 256L + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        long t = idx;
        const int tx = (int)(t % XTc); t /= XTc;
        const int ty = (int)(t % XTr); t /= XTr;
        const int s = (int)(t % S);
        const int oct = (int)(t / S);
        const int y = ty - 1, x = tx - 1;
        const bool in = y >= 0 && y < H && x >= 0 && x < W;
        float v[4][8];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int np = oct * 4 + p;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
            if (in && np < NP) {
                const float4* src = reinterpret_cast<const float4*>(xk + ((((size_t)np * S + s) * H + y) * W + x) * 8);
                a = src[0]; b = src[1];
            }
            // [k][image of the pair]: (k0 i0, k0 i1, k1 i0, k1 i1) (k2 ...)
            v[0][2 * p] = a.x; v[0][2 * p + 1] = a.y; v[1][2 * p] = a.z; v[1][2 * p + 1] = a.w;
            v[2][2 * p] = b.x; v[2][2 * p + 1] = b.y; v[3][2 * p] = b.z; v[3][2 * p + 1] = b.w;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float sc = ldexpf(1.0f, sd_shift(xmax[s * kNumK + k]));
            h8 hi, lo;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                _Float16 h, l;
                split_limbs(v[k][i] * sc, &h, &l);
                hi[i] = h; lo[i] = l;
            }
            h8* dst = xs + ((((size_t)oct * S + s) * kNumK + k) * XTr * XTc + (size_t)ty * XTc + tx) * 2;
            dst[0] = hi; dst[1] = lo;
        }
    }
}

// XS straight from x, without the fp32 copy XK in between (NCHW plans with an instantiated prefilter support): the filter is
// computed twice, by the two instantiations of ONE kernel text.  STORE = false keeps only max |Xk| per (input channel, kind),
// as the keys of blur4_pack_kernel<K, true>; STORE = true filters again, scales, splits and stores the limbs.  x is read twice
// (0.41 GB each at the flagship shape) instead of XK being written and read back (1.64 GB each).  Every value is, bit for bit, the
// one blur4_pack_kernel writes: the same masking of the loads, the same fma chains in the same order (k_blur4_pack_body.hpp).
//  * A wave (= a workgroup) takes kXwCols columns Tx of one (octet, input channel) and walks down the rows Ty.  Lane 4 c + p owns
//    column c and the image pair p of the octet (v_pk_fma_f32 on the pair, as blur4_pack packs its pair).
//  * Per step one raw row of the eight images (the tile's columns plus the filter's reach) goes through LDS, [column][8 images]:
//    a lane reads the K neighbours of its column as K ds_read_b64, lane-linear.  Two row buffers, so that one wave-level barrier
//    per row orders the writes of a row before its reads (LDS serves a wave's instructions in order).  The loads of the rows
//    kXwAhead steps on are in flight meanwhile.
//  * The K horizontally filtered rows (h1, h2, h3) live in a register ring; the row loop is unrolled K times, so that every slot
//    is a fixed register.  The vertical pass of output row y runs out of the ring once row y + (K - 1) / 2 is in.
//  * Store: a lane holds one dword of the hi and one of the lo piece of its column for each kind.  The row's pieces are put
//    together in LDS in the order of XS, [kind][column][limb][8 images], and go out as two 16-byte stores per lane, 32 consecutive
//    lanes to 512 consecutive bytes.  The zero row / column in front, those behind the image and the absent images of a partial
//    octet come out of the same code as masked values.
constexpr int kXwCols = 16;             // Tx columns per wave
constexpr int kXwAhead = 3;             // rows whose loads are in flight
constexpr int kXwOut = kNumK * kXwCols * 2 * 4;   // dwords of a tile row of XS
struct XkWalkArgs {
    const float* x;
    const float* taps;                  // filters + kTaps1dOffset
    unsigned* xmax;                     // [S][4 kinds] float bits
    h8* xs;
    int N, S, H, W, XTr, XTc, nct, act;
    int relu_in;                        // DAU_FLAG_INPUT_RELU: x is clamped at zero as it is widened (both passes: the maxima are those of the clamped x)
    Guard guard;
};

__device__ __forceinline__ void xw_wave_sync() {         // orders a wave's LDS writes before the reads of its other lanes
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

typedef float f2 __attribute__((ext_vector_type(2)));
template <int N, class F>
__device__ __forceinline__ void xw_unroll(F&& f) {       // f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>)
    [&]<int... I>(std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }(std::make_integer_sequence<int, N>{});
}
// fma(a, {t, t}, c) on an image pair with t one half of a PAIR of taps held in two scalar registers: the op_sel bits pick the half
// for both lanes.  (As a splat vector hipcc keeps {t, t} per tap: 2 x 6 x K scalar registers, more than there are, and the taps
// of some loops end up in vector registers.)  The instruction -- and its rounding -- is the v_pk_fma_f32 of blur4_pack_kernel.
template <int HALF>
__device__ __forceinline__ f2 xw_fma_tap(f2 a, unsigned long taps, f2 c) {
    f2 d;
    if constexpr (HALF == 0) asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1]" : "=v"(d) : "v"(a), "s"(taps), "v"(c));
    else asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "=v"(d) : "v"(a), "s"(taps), "v"(c));
    return d;
}

template <int K, bool STORE, int AF>
__device__ __forceinline__ void sd_xk_walk(const XkWalkArgs& a, float* lds) {
    typedef int i4s __attribute__((ext_vector_type(4)));
    typedef _Float16 h2s __attribute__((ext_vector_type(2)));
    typedef typename RawAct<AF>::type Raw;
    constexpr int KR = (K - 1) / 2, CW = kXwCols + 2 * KR, NL = (8 * CW + 63) / 64, kBuf = NL * 64;
    static_assert(kXwAhead < K, "the rows in flight are slots of the unrolled loop");
    int t = blockIdx.x;
    const int ct = t % a.nct; t /= a.nct;
    const int s = t % a.S, oct = t / a.S;
    const int lane = threadIdx.x, c = lane >> 2, p = lane & 3;
    const int H = a.H, W = a.W;
    const int tx0 = ct * kXwCols, x = tx0 + c - 1;
    const float* tp[6] = {a.taps + kTapGX * kTapPitch, a.taps + kTapAX * kTapPitch, a.taps + kTapCX * kTapPitch,
                          a.taps + kTapGY * kTapPitch, a.taps + kTapAY * kTapPitch, a.taps + kTapBY * kTapPitch};
    unsigned long tq[6][(K + 1) / 2];                   // taps 2 j and 2 j + 1 (the array's pitch holds the one past an odd K)
#pragma unroll
    for (int f = 0; f < 6; ++f)
#pragma unroll
        for (int j = 0; j < (K + 1) / 2; ++j) tq[f][j] = __builtin_bit_cast(unsigned long, f2{tp[f][2 * j], tp[f][2 * j + 1]});
    // The raw row of the tile: 8 images x CW columns (image x = tx0 - 1 - KR + column), NL loads per lane, a lane's loads of
    // one image running along x.  Image slot n of the octet: itself if n < N; the absent second image of the last pair is
    // 0 * (its partner's value), as blur4_pack computes it (m1); beyond the last pair, +0.  A load outside the row or of an
    // absent image reads a valid element and is masked.  Slots past the 8 * CW values write the buffer's spare words.
    long poff[NL];
    int lw[NL];
    float mf[NL];
    bool keep[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        const int tt = l * 64 + lane, tc = tt < 8 * CW ? tt : 8 * CW - 1;
        const int img = tc / CW, col = tc - img * CW;
        const int n = oct * 8 + img;
        const bool second = (n & 1) && n - 1 < a.N;          // (n >= N) the second image of a pair whose first exists
        const int src = n < a.N ? n : second ? n - 1 : oct * 8;
        const int xx = tx0 - 1 - KR + col;
        keep[l] = tt < 8 * CW && xx >= 0 && xx < W && (n < a.N || second);
        mf[l] = n < a.N ? 1.0f : 0.0f;
        poff[l] = ((long)src * a.S + s) * H * W + (xx < 0 ? 0 : xx < W ? xx : W - 1);
        lw[l] = tt < 8 * CW ? col * 8 + img : tt;
    }
    constexpr unsigned kKeyZero = 1u << 24;              // (the keys of blur4_pack_kernel<K, true>)
    unsigned km[4] = {kKeyZero, kKeyZero, kKeyZero, kKeyZero}, seen[4] = {0u, 0u, 0u, 0u};
    float sc[4] = {1.0f, 1.0f, 1.0f, 1.0f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if constexpr (STORE) sc[k] = ldexpf(1.0f, sd_shift(a.xmax[s * kNumK + k]));
        else seen[k] = __hip_atomic_load(a.xmax + s * kNumK + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // stream row r = u - 1 - KR enters at step u; output row Ty = u - (K - 1) (image row y = Ty - 1) leaves at step u.  The steps
    // are rounded up to whole rounds of the unrolled loop and a step has no branch but the one around its stores: the steps
    // before the first output row and after the last one compute on zeros and store nothing.
    const int steps = (a.XTr + K - 1 + K - 1) / K * K;
    Raw rv[K][NL];
    f2 hr[K][3];                                         // ring: slot, filter (h1, h2, h3)
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
        for (int f = 0; f < 3; ++f) hr[i][f] = f2{0.0f, 0.0f};
    auto load_row = [&](int u, Raw* dst) {
        const int r = u - 1 - KR, rc = r < 0 ? 0 : r < H ? r : H - 1;
#pragma unroll
        for (int l = 0; l < NL; ++l) dst[l] = load_raw<AF>(a.x, poff[l] + (long)rc * W);
    };
#pragma unroll
    for (int d = 0; d < kXwAhead; ++d) load_row(d, rv[d]);
    // piece lane + 64 i of the tile row: kind 2 i + lane / 32, column (lane % 32) / 2, limb lane % 2
    const size_t plane = (size_t)a.XTr * a.XTc;
    h8* const out = a.xs + ((size_t)(oct * a.S + s) * kNumK + (lane >> 5)) * plane * 2 + (size_t)tx0 * 2 + (lane & 31);
    const bool col_in = tx0 + ((lane & 31) >> 1) < a.XTc;
    float* obuf = lds + 2 * kBuf;
    const bool ri = a.relu_in != 0;
    auto step = [&](auto pc, int u) {
        constexpr int P = decltype(pc)::value;
        load_row(u + kXwAhead, rv[(P + kXwAhead) % K]);
        const int r = u - 1 - KR;
        const bool row_in = r >= 0 && r < H;
        float* buf = lds + (u & 1) * kBuf;
#pragma unroll
        for (int l = 0; l < NL; ++l) buf[lw[l]] = mask_act(mf[l] * relu_in(act_of(rv[P][l]), ri), keep[l] && row_in);
        xw_wave_sync();
        f2 h[3] = {{0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}};
        xw_unroll<K>([&](auto ic) {
            constexpr int I = decltype(ic)::value, i = I;
            const f2 v = *reinterpret_cast<const f2*>(buf + (c + i) * 8 + 2 * p);
#pragma unroll
            for (int f = 0; f < 3; ++f) h[f] = xw_fma_tap<I & 1>(v, tq[f][I / 2], h[f]);
        });
#pragma unroll
        for (int f = 0; f < 3; ++f) hr[P][f] = h[f];
        const int ty = u - (K - 1), y = ty - 1;
        f2 o[4] = {{0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}};
        xw_unroll<K>([&](auto jc) {
            constexpr int J = decltype(jc)::value, sl = (P + 1 + J) % K;   // (P + 1: the slot of stream row y - KR)
            const unsigned long gy = tq[3][J / 2], ay = tq[4][J / 2], by = tq[5][J / 2];
            const f2 b1 = hr[sl][0], b2 = hr[sl][1], b3 = hr[sl][2];
            o[0] = xw_fma_tap<J & 1>(b1, gy, o[0]);
            o[1] = xw_fma_tap<J & 1>(b2, gy, o[1]);
            o[2] = xw_fma_tap<J & 1>(b1, ay, o[2]);
            o[3] = xw_fma_tap<J & 1>(b3, gy, o[3]);
            o[3] = xw_fma_tap<J & 1>(b1, by, o[3]);
        });
        // (rows and columns outside the image: +0, whatever the sums over the neighbouring rows gave)
        const bool in = y >= 0 && y < H && x >= 0 && x < W;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float v0 = mask_act(o[k].x, in), v1 = mask_act(o[k].y, in);
            if constexpr (!STORE) {
                km[k] = max(max(km[k], (__float_as_uint(v0) << 1) + kKeyZero), (__float_as_uint(v1) << 1) + kKeyZero);
            } else {
                h2s hi, lo;
                _Float16 hh, ll;
                split_limbs(v0 * sc[k], &hh, &ll);
                hi[0] = hh; lo[0] = ll;
                split_limbs(v1 * sc[k], &hh, &ll);
                hi[1] = hh; lo[1] = ll;
                obuf[(k * kXwCols + c) * 8 + p] = __builtin_bit_cast(float, hi);
                obuf[(k * kXwCols + c) * 8 + 4 + p] = __builtin_bit_cast(float, lo);
            }
        }
        if constexpr (STORE) {
            xw_wave_sync();
            const i4s piece0 = *reinterpret_cast<const i4s*>(obuf + lane * 4);
            const i4s piece1 = *reinterpret_cast<const i4s*>(obuf + (64 + lane) * 4);
            if (col_in && ty >= 0 && ty < a.XTr) {
                h8* dst = out + (size_t)ty * a.XTc * 2;
                dst[0] = __builtin_bit_cast(h8, piece0);
                dst[2 * plane * 2] = __builtin_bit_cast(h8, piece1);
            }
        }
    };
#pragma unroll 1
    for (int u0 = 0; u0 < steps; u0 += K) {
        xw_unroll<K>([&](auto pc) { step(pc, u0 + decltype(pc)::value); });
    }
    if constexpr (!STORE) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            unsigned m = km[k];
            for (int w = 32; w >= 1; w >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, w));
            // a maximum only grows: what does not exceed the value read when the wave began changes nothing
            const unsigned bits = (m - kKeyZero) >> 1;
            if (lane == 0 && bits > seen[k]) atomicMax(a.xmax + s * kNumK + k, bits);
        }
    }
}

template <int K, bool STORE>
__global__ void __launch_bounds__(64) sd_xk_walk_kernel(const XkWalkArgs a) {
    constexpr int kBuf = (8 * (kXwCols + K - 1) + 63) / 64 * 64;
    __shared__ __attribute__((aligned(16))) float lds[2 * kBuf + (STORE ? kXwOut : 0)];
    if (!guard_pass(a.guard)) return;
    with_act(a.act, [&](auto actc) { sd_xk_walk<K, STORE, decltype(actc)::value>(a, lds); });
}

// ES[oct][fb][Vy][Vx][limb][16 f][8] from dy[N][F][H][W] (fp32 or f16: act).  An f16 dy times the power-of-two scale is its own
// hi limb; its lo limb is zero.
#ifndef DAU_SD_STAGE_REF
constexpr int kSeTX = 80;               // window columns per workgroup of the row kernels: 40 KiB of LDS, four workgroups per CU
#endif
#if !defined(DAU_SD_STAGE_REF) && !defined(DAU_SD_STAGE_E_ROWS)
// The walking form (NCHW plans).  A wave (= a workgroup) owns (octet, block of 16 channels, tile of kSeCols window columns, band of
// window rows) and walks down the band's rows, as sd_xk_walk_kernel does:
//  * Lane 16 j + c owns window column vx0 + c and the four channels j, j + 4, j + 8, j + 12 of the block for the whole walk; its 32
//    element loads of a row (4 channels x the octet's 8 images) are one lane offset per channel plus a wave-uniform (image, row)
//    base, so the row loop holds no division.  A load instruction reads 16 consecutive x of four channels.
//  * The loads of the row kSeAhead steps on are in flight while the current row is processed: the row loop is unrolled over the
//    ring of raw rows, so that every slot is a fixed register.
//  * A lane then holds the eight images of its (channel, column) pairs: it scales, splits and puts the hi and the lo piece where
//    they go in the row's image in LDS -- position-major, the 32 pieces of a position permuted by (position & 7) as in the row
//    kernel below, so that the eight lanes of a ds_write_b128 group (eight consecutive x, one channel) reach all 32 banks.  Two
//    row images, one wave-level barrier per row.  The row leaves as 16-byte pieces, lane-linear: 1 KiB of ES per store instruction.
//  * Halo rows and columns, the row / column the edge rule drops, the absent images of a ragged octet and the absent channels of a
//    ragged block are loads of a valid element masked to +0 (0 * scale = +0 in both limbs): one code path, and every 16-byte piece
//    of ES is written by exactly one store.
//  * The grid runs (column tile, band, block, octet), column tile fastest, under xcd_contiguous_id: the tiles of a row, whose loads
//    share 128-byte lines, go to one L2.
// -DDAU_SD_STAGE_E_ROWS (libdau_conv_hip_stage_e_rows.so of `make tuning`) keeps the workgroup-per-window-row kernel below: the A/B
// partner; -DDAU_SD_STAGE_REF keeps the oldest form (one thread per position), the bit-exact reference of
// tests/test_gpu_split_dot_stage_e_walk.py.
constexpr int kSeCols = 16;             // window columns per wave: an 8 KiB row image
constexpr int kSeAhead = 1;             // rows whose loads are in flight (32 loads per lane and row; vmcnt counts to 63)
struct SeWalkArgs {
    const float* dy;
    const unsigned* emax;               // [F] float bits
    h8* es;
    int N, F, H, W, nfb, EYs, EXs, nct, nbands, RB, wlim, hlim, act;
    Guard guard;
};

template <int AF>
__device__ __forceinline__ void sd_stage_e_walk(const SeWalkArgs& a, h8* lds) {
    typedef typename RawAct<AF>::type Raw;
    constexpr int kRing = kSeAhead + 1, kRow = kSeCols * 32;   // kRow: 16-byte pieces of a row image
    int t = xcd_contiguous_id(blockIdx.x, gridDim.x);
    const int ct = t % a.nct; t /= a.nct;
    const int band = t % a.nbands; t /= a.nbands;
    const int fb = t % a.nfb, oct = t / a.nfb;
    const int lane = threadIdx.x, c = lane & (kSeCols - 1), j = lane >> 4;
    const int H = a.H, W = a.W;
    const long plane = (long)H * W;
    const int vx0 = ct * kSeCols, x = vx0 + c - (kSdRX + 1);
    const bool col_in = x >= 0 && x < a.wlim;
    long off[4];                                         // elements from (image, first channel of the block, row)
    float sc[4];
    bool keep[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int fl = j + 4 * m, f = fb * kSdFB + fl;
        keep[m] = col_in && f < a.F;
        sc[m] = f < a.F ? ldexpf(1.0f, sd_shift(a.emax[f])) : 0.0f;
        off[m] = (f < a.F ? fl : 0) * plane + (x < 0 ? 0 : x < W ? x : W - 1);
    }
    const int b0 = band * a.RB, b1 = min(b0 + a.RB, a.EYs);
    // the steps are rounded up to whole rounds of the unrolled loop: a step past the band's last row loads a clamped row and
    // stores nothing
    const int steps = (b1 - b0 + kRing - 1) / kRing * kRing;
    Raw rv[kRing][32];
    auto load_row = [&](int vy, Raw* dst) {
        const int y = vy - (kSdRY + 1), yc = y < 0 ? 0 : y < H ? y : H - 1;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int n = oct * 8 + i;
            const long rowbase = (((long)(n < a.N ? n : oct * 8) * a.F + fb * kSdFB) * H + yc) * W;
#pragma unroll
            for (int m = 0; m < 4; ++m) dst[4 * i + m] = load_raw<AF>(a.dy, rowbase + off[m]);
        }
    };
#pragma unroll
    for (int d = 0; d < kSeAhead; ++d) load_row(b0 + d, rv[d]);
    h8* const out = a.es + (((size_t)oct * a.nfb + fb) * a.EYs * a.EXs + vx0) * 32 + lane;
    auto step = [&](auto pc, int u) {
        constexpr int P = decltype(pc)::value;
        const int vy = b0 + u, y = vy - (kSdRY + 1);
        load_row(vy + kSeAhead, rv[(P + kSeAhead) % kRing]);
        const bool row_in = y >= 0 && y < a.hlim;
        h8* buf = lds + (u & 1) * kRow;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int fl = j + 4 * m;
            h8 hi, lo;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float v = mask_act(act_of(rv[P][4 * i + m]), keep[m] && row_in && oct * 8 + i < a.N);
                _Float16 h, l;
                split_limbs(v * sc[m], &h, &l);
                hi[i] = h; lo[i] = l;
            }
            buf[c * 32 + (fl ^ (c & 7))] = hi;
            buf[c * 32 + ((kSdFB + fl) ^ (c & 7))] = lo;
        }
        xw_wave_sync();
        // piece lane + 64 i of the row image: position 2 i + lane / 32, piece lane % 32
        h8 piece[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int lx = 2 * i + (lane >> 5);
            piece[i] = buf[lx * 32 + ((lane & 31) ^ (lx & 7))];
        }
        h8* dst = out + (size_t)vy * a.EXs * 32;
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (vy < b1 && vx0 + 2 * i + (lane >> 5) < a.EXs) dst[64 * i] = piece[i];
    };
#pragma unroll 1
    for (int u0 = 0; u0 < steps; u0 += kRing) {
        xw_unroll<kRing>([&](auto pc) { step(pc, u0 + decltype(pc)::value); });
    }
}

__global__ void __launch_bounds__(64) sd_stage_e_kernel(const SeWalkArgs a) {
    __shared__ h8 lds[2 * kSeCols * 32];
    if (!guard_pass(a.guard)) return;
    with_act(a.act, [&](auto actc) { sd_stage_e_walk<decltype(actc)::value>(a, lds); });
}
#elif !defined(DAU_SD_STAGE_REF)
// (the form before the walking one) A workgroup writes one window row (oct, fb, Vy) -- a column tile of it where the row is wider
// than kSeTX positions.  A thread
// takes one (channel, x) of the row's image part: its eight loads (the octet's images) run along x across the lanes, it scales
// and splits in registers and puts the two 16-byte pieces of its eight values where they go in the row's image in LDS; then
// the workgroup copies the image out, 16 bytes per lane, consecutive lanes to consecutive addresses.  Halo rows and columns
// (the edge rule's dropped row / column included) are plain zero stores.  The 32 pieces of a position are permuted by
// (position & 7), so that the eight lanes of a ds_write_b128 group (eight consecutive x, one channel) reach all 32 banks.
__global__ void __launch_bounds__(256) sd_stage_e_kernel(const float* __restrict__ dy, const unsigned* __restrict__ emax, int N,
                                                         int F, int H, int W, int nfb, int EYs, int EXs, int nct, int TX,
                                                         int drop_col, int drop_row, int act, h8* __restrict__ es,
                                                         const Guard guard) {
    __shared__ h8 tile[kSeTX * 32];
    if (!guard_pass(guard)) return;
    int t = blockIdx.x;
    const int ct = t % nct; t /= nct;
    const int vy = t % EYs; t /= EYs;
    const int fb = t % nfb;
    const int oct = t / nfb;
    const int wlim = drop_col ? W - 1 : W, hlim = drop_row ? H - 1 : H;
    const int vx0 = ct * TX, nvx = min(TX, EXs - vx0);   // this tile's window columns [vx0, vx0 + nvx)
    const int y = vy - (kSdRY + 1);
    // its columns inside the image: [c0, c1)
    const int c0 = max(vx0, kSdRX + 1), c1 = (y >= 0 && y < hlim) ? min(vx0 + nvx, kSdRX + 1 + wlim) : c0;
    const int nd = max(c1 - c0, 0);
    for (int i = threadIdx.x; i < kSdFB * nd; i += 256) {
        const int fl = i / nd, vx = c0 + (i - fl * nd), x = vx - (kSdRX + 1), lx = vx - vx0;
        const int f = fb * kSdFB + fl;
        const float sc = f < F ? ldexpf(1.0f, sd_shift(emax[f])) : 0.0f;
        float v[8];
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            const int img = oct * 8 + n;
            v[n] = (f < F && img < N) ? load_act(dy, (((long)img * F + f) * H + y) * W + x, act) : 0.0f;
        }
        h8 hi, lo;
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            _Float16 h, l;
            split_limbs(v[n] * sc, &h, &l);
            hi[n] = h; lo[n] = l;
        }
        tile[lx * 32 + (fl ^ (lx & 7))] = hi;
        tile[lx * 32 + ((kSdFB + fl) ^ (lx & 7))] = lo;
    }
    if (nd > 0) __syncthreads();                         // (nd is the same for the whole workgroup)
    h8* dst = es + ((((size_t)oct * nfb + fb) * EYs + vy) * EXs + vx0) * 32;
    for (int q = threadIdx.x; q < nvx * 32; q += 256) {
        const int lx = q >> 5, vx = vx0 + lx;
        h8 piece = {0, 0, 0, 0, 0, 0, 0, 0};
        if (vx >= c0 && vx < c1) piece = tile[lx * 32 + ((q & 31) ^ (lx & 7))];
        dst[q] = piece;
    }
}
#else
// (the earlier form) one thread per (oct, fb, Vy, Vx), the 16 channels of the block
__global__ void __launch_bounds__(256) sd_stage_e_kernel(const float* __restrict__ dy, const unsigned* __restrict__ emax, int N,
                                                         int F, int H, int W, int octs, int nfb, int EYs, int EXs, int drop_col,
                                                         int drop_row, int act, int nhwc, h8* __restrict__ es, const Guard guard) {
    if (!guard_pass(guard)) return;
    const long total = (long)octs * nfb * EYs * EXs;
    const int wlim = drop_col ? W - 1 : W, hlim = drop_row ? H - 1 : H;
    for (long idx = blockIdx.x * 256L + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        long t = idx;
        const int vx = (int)(t % EXs); t /= EXs;
        const int vy = (int)(t % EYs); t /= EYs;
        const int fb = (int)(t % nfb);
        const int oct = (int)(t / nfb);
        const int y = vy - (kSdRY + 1), x = vx - (kSdRX + 1);
        const bool in = y >= 0 && y < hlim && x >= 0 && x < wlim;
        h8* dst = es + (size_t)idx * 32;
        for (int fl = 0; fl < kSdFB; ++fl) {
            const int f = fb * kSdFB + fl;
            const float sc = f < F ? ldexpf(1.0f, sd_shift(emax[f])) : 0.0f;
            h8 hi, lo;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int n = oct * 8 + i;
                const float v = (in && f < F && n < N) ? load_act(dy, nhwc ? nhwc_index(n, f, y, x, F, H, W) : (((long)n * F + f) * H + y) * W + x, act) : 0.0f;
                _Float16 h, l;
                split_limbs(v * sc, &h, &l);
                hi[i] = h; lo[i] = l;
            }
            dst[fl] = hi; dst[kSdFB + fl] = lo;
        }
    }
}
#endif

// ES1[oct][fb][Vy][Vx][16 f][8]: the one-limb form of the workgroup-per-window-row sd_stage_e_kernel above (bf16 activations:
// hi = f16(v * scale) is the whole value).  The same structure -- the row's image in LDS, whole-run stores, zero halo, the edge
// rule -- with 16 pieces of 16 bytes per position.  Bank permutation: a position is 256 B = twice the 128 B that the 32 banks of
// a ds_write_b128 span, so a piece's bank group is (piece & 7) whatever the position; the eight lanes of a write group (eight
// consecutive x, one channel fl) write pieces fl ^ (lx & 7), whose low three bits take all eight values: all 32 banks.
// (-DDAU_SD_STAGE_REF keeps the earlier form of the two-limb kernel only; one-limb plans stage through this kernel there too.)
constexpr int kSe1TX = 80;              // window columns per workgroup: 20 KiB of LDS
__global__ void __launch_bounds__(256) sd_stage_e1_kernel(const float* __restrict__ dy, const unsigned* __restrict__ emax, int N,
                                                          int F, int H, int W, int nfb, int EYs, int EXs, int nct, int TX,
                                                          int drop_col, int drop_row, int act, h8* __restrict__ es,
                                                          const Guard guard) {
    __shared__ h8 tile[kSe1TX * kSdFB];
    if (!guard_pass(guard)) return;
    int t = blockIdx.x;
    const int ct = t % nct; t /= nct;
    const int vy = t % EYs; t /= EYs;
    const int fb = t % nfb;
    const int oct = t / nfb;
    const int wlim = drop_col ? W - 1 : W, hlim = drop_row ? H - 1 : H;
    const int vx0 = ct * TX, nvx = min(TX, EXs - vx0);   // this tile's window columns [vx0, vx0 + nvx)
    const int y = vy - (kSdRY + 1);
    // its columns inside the image: [c0, c1)
    const int c0 = max(vx0, kSdRX + 1), c1 = (y >= 0 && y < hlim) ? min(vx0 + nvx, kSdRX + 1 + wlim) : c0;
    const int nd = max(c1 - c0, 0);
    for (int i = threadIdx.x; i < kSdFB * nd; i += 256) {
        const int fl = i / nd, vx = c0 + (i - fl * nd), x = vx - (kSdRX + 1), lx = vx - vx0;
        const int f = fb * kSdFB + fl;
        const float sc = f < F ? ldexpf(1.0f, sd_shift(emax[f])) : 0.0f;
        float v[8];
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            const int img = oct * 8 + n;
            v[n] = (f < F && img < N) ? load_act(dy, (((long)img * F + f) * H + y) * W + x, act) : 0.0f;
        }
        h8 hi;
#pragma unroll
        for (int n = 0; n < 8; ++n) hi[n] = (_Float16)(v[n] * sc);   // (a non-finite value keeps its hi limb, as in split_limbs)
        tile[lx * kSdFB + (fl ^ (lx & 7))] = hi;
    }
    if (nd > 0) __syncthreads();                         // (nd is the same for the whole workgroup)
    h8* dst = es + ((((size_t)oct * nfb + fb) * EYs + vy) * EXs + vx0) * kSdFB;
    for (int q = threadIdx.x; q < nvx * kSdFB; q += 256) {
        const int lx = q >> 4, vx = vx0 + lx;
        h8 piece = {0, 0, 0, 0, 0, 0, 0, 0};
        if (vx >= c0 && vx < c1) piece = tile[lx * kSdFB + ((q & 15) ^ (lx & 7))];
        dst[q] = piece;
    }
}

// ES (LIMBS = 2) or ES1 (LIMBS = 1) from an [N][H][W][F] dy (DAU_FLAG_IO_NHWC): the workgroups, window rows and column tiles of the two
// kernels above.  The sixteen channels of a position, which ES keeps together, are one contiguous run of the input, so nothing goes
// through LDS: a thread takes one (position, channel) -- sixteen lanes read the sixteen channels of a pixel, once per image of the
// octet -- scales and splits as above and stores its one or two 16-byte pieces, consecutive lanes to consecutive addresses.  Halo
// positions (the edge rule's dropped row / column included), channels beyond F and images beyond N are masked to +0 and give zero pieces.
template <int LIMBS>
__global__ void __launch_bounds__(256) sd_stage_nhwc_e_kernel(const float* __restrict__ dy, const unsigned* __restrict__ emax, int N,
                                                              int F, int H, int W, int nfb, int EYs, int EXs, int nct, int TX,
                                                              int drop_col, int drop_row, int act, h8* __restrict__ es,
                                                              const Guard guard) {
    if (!guard_pass(guard)) return;
    int t = blockIdx.x;
    const int ct = t % nct; t /= nct;
    const int vy = t % EYs; t /= EYs;
    const int fb = t % nfb;
    const int oct = t / nfb;
    const int wlim = drop_col ? W - 1 : W, hlim = drop_row ? H - 1 : H;
    const int vx0 = ct * TX, nvx = min(TX, EXs - vx0);   // this tile's window columns [vx0, vx0 + nvx)
    const int y = vy - (kSdRY + 1);
    // its columns inside the image: [c0, c1)
    const int c0 = max(vx0, kSdRX + 1), c1 = (y >= 0 && y < hlim) ? min(vx0 + nvx, kSdRX + 1 + wlim) : c0;
    h8* dst = es + ((((size_t)oct * nfb + fb) * EYs + vy) * EXs + vx0) * (kSdFB * LIMBS);
    for (int i = threadIdx.x; i < nvx * kSdFB; i += 256) {
        const int lx = i / kSdFB, fl = i - lx * kSdFB, vx = vx0 + lx, x = vx - (kSdRX + 1);
        const int f = fb * kSdFB + fl;
        const bool in = vx >= c0 && vx < c1 && f < F;
        const float sc = f < F ? ldexpf(1.0f, sd_shift(emax[f])) : 0.0f;
        float v[8];
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            const int img = oct * 8 + n;
            const bool ok = in && img < N;
            v[n] = mask_act(load_act(dy, ok ? nhwc_index(img, f, y, x, F, H, W) : 0, act), ok);
        }
        h8 hi, lo;
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            if constexpr (LIMBS == 2) {
                _Float16 h, l;
                split_limbs(v[n] * sc, &h, &l);
                hi[n] = h; lo[n] = l;
            } else {
                hi[n] = (_Float16)(v[n] * sc);
            }
        }
        dst[lx * (kSdFB * LIMBS) + fl] = hi;
        if constexpr (LIMBS == 2) dst[lx * (kSdFB * LIMBS) + kSdFB + fl] = lo;
    }
}

struct SdArgs {
    const h8* xs;
    const char* es;
    const unsigned* xmax;
    const unsigned* emax;
    const UnitRef* table;       // bare unit table [S][G][F]
    float* partial;             // [chunk][4][S][G][F]
    int S, F, G;
    int nfb, nsb, ngb, per, items, rq, cq, XTr, XTc, EYs, EXs;
    int thin;                   // SdGeom::thin
    Guard guard;
};

// One 1 KiB piece of the error window: 16 bytes per lane from `src` into the LDS bytes [dst, dst + 1024) (lane-linear), with no
// VGPR in between.  Inline asm, so that hipcc leaves it out of its wait bookkeeping: as a builtin it would put a vmcnt wait in
// front of every following LDS read and A-fragment use and drain the copy at once.  Its completion is counted by hand (below);
// hipcc's own counted waits only ever wait MORE for it (its place in the in-order queue of vector loads is not counted there).
__device__ __forceinline__ void sd_glds16(const char* src, unsigned dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
}

// The A fragment of the next K step from those of a pair of steps: a lane offers its quad neighbour the column that lane needs
// (`cur` if it holds dx = 1, `nxt`, the pair after, if it holds dx = 0) and takes what the neighbour offers (lanes 2 q <-> 2 q + 1)
#ifndef DAU_SD_STEP_LOADS
__device__ __forceinline__ h8 sd_next_col(h8 cur, h8 nxt, int dx) {
    typedef int i4s __attribute__((ext_vector_type(4)));
    const i4s c = __builtin_bit_cast(i4s, cur), n = __builtin_bit_cast(i4s, nxt);
    i4s r;
#pragma unroll
    for (int d = 0; d < 4; ++d)
        r[d] = __builtin_amdgcn_update_dpp(0, dx ? c[d] : n[d], 0xB1 /* quad_perm:[1,0,3,2] */, 0xF, 0xF, true);
    return __builtin_bit_cast(h8, r);
}
#endif

// RW: columns per region (K steps per item).  The error window of an item is WR = RH + 2R rows x RW + 2R columns x 512 B; the
// LDS holds a RING of WR + RH rows.  The items of a chunk walk DOWN a column strip of regions (one image octet), so the window of
// the next item is the current one moved down by RH rows: its RH new rows are copied into the ring's RH free slots while the
// current item computes, and one barrier per item publishes them.  The whole window is copied only at the first item of a chunk
// and where a strip begins.
// Timing experiments of a tuning build (tools/build_variant.sh; results are garbage): DAU_SD_DIAG_NOFILL copies no window
// (waits and barriers stay), DAU_SD_DIAG_NOA reloads no A fragment, DAU_SD_DIAG_AFIXED reads the A fragments of the chunk's
// first item for every item (the same loads, hitting in the caches).
// EL: limbs of the staged error = 256-byte halves of a window position.  EL = 2 is split_gather_dot_kernel; EL = 1
// (sd_e1_dot_kernel, bf16 activations) reads ES1, holds half the ring and leaves out the product with the lo limb of the error.
template <int RW, int EL>
__device__ __forceinline__ void sd_dot_body(const SdArgs& a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    if (!guard_pass(a.guard)) return;
    constexpr int WL = RW + 2 * kSdRX, WR = kSdRH + 2 * kSdRY;
    constexpr int kRing = WR + kSdRH;                    // ring slots (rows)
    constexpr int PB = EL * 256;                         // bytes per window position: 16 channels x 8 images x EL limbs
    constexpr unsigned RB = WL * PB;                     // bytes per window row
    // 1 KiB pieces per row: a whole number for EL = 2 (WL is even); for EL = 1 and RW = 10 the last piece of a row is half
    // a piece (its upper 32 lanes are masked off: `within < RB` below)
    constexpr int kRowPieces = (RB + 1023) / 1024;
    static_assert((kRing & (kRing - 1)) == 0, "ring slot = (origin + row) & (kRing - 1)");
    static_assert(RW % 2 == 0, "A fragment sets by the parity of the K step / of the pair of K steps");
#ifdef DAU_SD_STEP_LOADS
    constexpr int kSdAStride = 2;                        // 16-byte units between the two A sets at the start of an item: a column
#else
    constexpr int kSdAStride = 4;                        // a pair of columns
#endif
    static_assert((size_t)kRing * RB <= 160 * 1024, "the ring fills the LDS");
    int t = blockIdx.x;
    const int gb = t % a.ngb; t /= a.ngb;
    const int sb = t % a.nsb; t /= a.nsb;
    const int fb = t % a.nfb; t /= a.nfb;
    const int chunk = t;
    const int it0 = chunk * a.per, it1 = min(it0 + a.per, a.items);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int fl = lane & 15, j = lane >> 4;
    const int f = fb * kSdFB + fl;
    const bool f_ok = f < a.F;
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)lds;
    // A operand of this lane: row m = 4 k + d, K group j
    const int m = lane & 15, ak = m >> 2, ady = (m >> 1) & 1, adx = m & 1;
    const size_t xplane = (size_t)a.XTr * a.XTc;         // positions per (oct, s, k) plane
    unsigned aoff[kSdAS];                                // lane offset (in 16-byte units) of its A row, per input channel
    int sidx[kSdAS];
    bool s_ok[kSdAS];
    unsigned uw[kSdAS][kSdGT];                           // the unit's B column at K step 0: window row | byte offset in the row << 4
    f4s wb[kSdAS][kSdGT];                                // the unit's bilinear factors (w00, w01, w10, w11)
    float run[kSdAS][kSdGT];
#pragma unroll
    for (int i = 0; i < kSdAS; ++i) {
        const int s = sb * kSdSB + wave * kSdAS + i;
        s_ok[i] = s < a.S;
        sidx[i] = s_ok[i] ? s : a.S - 1;
        aoff[i] = (unsigned)((((size_t)sidx[i] * kNumK + ak) * xplane + (size_t)(j + (kSdLine ? 0 : ady)) * a.XTc + adx) * 2);
#pragma unroll
        for (int gg = 0; gg < kSdGT; ++gg) {
            const int g = gb * kSdGT + gg;
            UnitRef u{0, 0, 0.0f, 0.0f, 0.0f, 0.0f};
            if (s_ok[i] && g < a.G && f_ok) u = a.table[((size_t)sidx[i] * a.G + g) * a.F + f];
            uw[i][gg] = (unsigned)(j - u.oy + kSdRY) | (unsigned)((kSdRX - u.ox) * PB + fl * 16) << 4;
            wb[i][gg] = f4s{u.w00, u.w01, u.w10, u.w11};
            run[i][gg] = 0.0f;
        }
    }
    // the scale exponents, read once: with loads in the flush, hipcc's wait bookkeeping at the item loop's header would
    // become conservative and drain the window copy in flight
    int shx[kSdAS];
    const int she = f_ok ? sd_shift(a.emax[f]) : 0;
#pragma unroll
    for (int i = 0; i < kSdAS; ++i) shx[i] = sd_shift(a.xmax[sidx[i] * kNumK + j]);
    auto flush = [&]() {
        // (the lane's kind goes through an empty asm statement: the slots' addresses are computed here, every kSdFlushItems items,
        // and hold no registers while the items run -- the three kinds of item below each end with a copy of this code)
        int jf = j;
        asm volatile("" : "+v"(jf));
#pragma unroll
        for (int i = 0; i < kSdAS; ++i) {
            // undo the scales: 2^-(shift of (s, k) + shift of f), in two exact steps
#pragma unroll
            for (int gg = 0; gg < kSdGT; ++gg) {
                const int g = gb * kSdGT + gg;
                if (s_ok[i] && g < a.G && f_ok) {
                    const float v = ldexpf(ldexpf(run[i][gg], -shx[i]), -she);
                    float* dst = a.partial + ((((size_t)chunk * kNumK + jf) * a.S + sidx[i]) * a.G + g) * a.F + f;
                    __hip_atomic_fetch_add(dst, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                run[i][gg] = 0.0f;
            }
        }
    };
    // item -> (octet, region row ry, region column rx); the regions of an octet are numbered down the column strips
    const int per_oct = a.rq * a.cq;
    auto item_off = [&](int item) {                       // A offset (16-byte units) of an item's region corner
        const int oct = item / per_oct, reg = item - oct * per_oct, rx = reg / a.rq, ry = reg - rx * a.rq;
        return ((size_t)oct * a.S * kNumK * xplane + (size_t)(ry * kSdRH) * a.XTc + (size_t)rx * RW) * 2;
    };
    // window rows [w0, w0 + nrows) of the item at (oct, ry, rx) into the ring slots (origin + w0 ..) & (kRing - 1), spread over the
    // eight waves row by row (a piece must be contiguous in LDS)
    auto fill = [&](int oct, int ry, int rx, int w0, int nrows, int origin) {
#ifndef DAU_SD_DIAG_NOFILL
        const char* src = a.es + ((((size_t)oct * a.nfb + fb) * a.EYs + (size_t)(ry * kSdRH + w0)) * a.EXs + (size_t)rx * RW) * PB;
        for (int u = wave_u; u < nrows * kRowPieces; u += kSdWaves) {
            const int rr = u / kRowPieces, pc = u - rr * kRowPieces;
            const unsigned within = pc * 1024 + lane * 16;
            const unsigned slot = (unsigned)(origin + w0 + rr) & (kRing - 1);
            // (readfirstlane: hipcc may form this wave-uniform address in vector registers, and the asm statement's m0 takes a scalar one)
            if (within < RB) sd_glds16(src + (size_t)rr * a.EXs * PB + within, __builtin_amdgcn_readfirstlane(lds0 + slot * RB + pc * 1024));
        }
#endif
    };
    // A fragments.  A lane's row is m = 4 k + 2 dy + dx, so at K step c + 1 the lane with dx = 0 needs the 32 bytes its quad
    // neighbour (dx = 1) held at step c: the columns are loaded per PAIR of K steps.  Pair r of an item is P_r = X[row j + dy,
    // column 2 r + dx]; step 2 r uses it as is, step 2 r + 1 takes the neighbour's P_r (dx = 0) or P_{r + 1} (dx = 1): one select
    // and one quad-permute DPP move per dword (sd_next_col), no LDS traffic.  Set p holds the pairs of parity p; a set is
    // reloaded with pair r + 2 once pair r's odd-step fragment is built: two K steps ahead, as the per-step loads were.  The
    // last odd step needs column RW of the item's own rows (the next item is the region below): pair RW / 2, of which only the
    // dx = 0 lanes' half is used (XTc = Wq + 1 holds that column; the dx = 1 lanes read one position on, inside the staging's
    // padding).  RW / 2 + 1 loads per item, channel and limb instead of RW.  The last pair fetches the first two pairs of the
    // next item into sets 0 and 1 (software pipeline).
    // -DDAU_SD_STEP_LOADS (tuning builds) keeps one load per K step, set p holding the steps of parity p: the same fragments
    // into the same MFMAs, bit for bit.
    // Thin items (a.thin: the last region of every strip holds one real row, t = 4 ry; rows 4 ry + 1 .. + 3 are zero on both
    // sides).  K group j of a thin item is the row's column 4 k + j instead of row j of column k: ceil(RW / 4) K steps.
    //  * A: lane (m, j) reads X[row 4 ry + dy, column 4 k + j + dx] -- its offset aoff with the row term j * XTc replaced by the
    //    column term j (thin_adjust below, derived where it is used: no register array of its own).  Adjacent columns sit in
    //    different lane groups, so every K step loads its own fragment: no pair / DPP scheme.
    //  * B: the unit's window row is that of K group 0 for all four groups, its byte offset grows by j * PB, a K step advances
    //    4 * PB (PB is a multiple of 256 B: the bank group of a read stays lane % 16).
    //  * RW = 10: the third K step covers columns 8 .. 11; the groups of columns 10 and 11 (the next region's) get a zero A
    //    fragment by a select and read the B column of group 0, so no lane reads beyond the window row and nothing is counted twice.
    //  * The counted wait.  vmcnt(8) at the top of an item names the eight A loads of the item's first two K steps, sets 0 and 1
    //    in this order, whatever kind of item follows whatever kind: the item in front of a thin item fetches the thin item's
    //    fragments of K steps 0 and 1 in exactly the slots where it would fetch pairs 0 and 1 (the look-ahead address gets the
    //    lane term nadj and the stride nstep), and a thin item loads its third fragment (into the registers the odd steps'
    //    fragments use elsewhere) BEFORE it fetches the next item's sets 0 and 1, again as its last eight loads.  A thin item is
    //    the last of its strip and copies no window rows; it also waits for its look-ahead loads before it ends (below), which
    //    costs part of one load's latency per strip: the loads have been in flight for one to two of its three K steps.
    //  * A thin K step reads the B fragments of one input channel at a time (the full items read channel 1's while channel 0's
    //    MFMAs run): 32 registers less, and 3 K steps in 180 are not where the time goes.
    // (mod 2^32: aoff + tadj >= 0; the lane's j goes through an empty asm statement, so that the term is computed where it
    // is used and holds no register while the full items run)
    auto thin_adjust = [&]() {
        int jj = j;
        asm volatile("" : "+v"(jj));
        return (unsigned)(jj * 2) - (unsigned)(jj * a.XTc * 2);
    };
    constexpr int kThinStride = 2 * kSdRH;               // 16-byte units between the A fragments of a thin item's K steps
    constexpr int kThinSteps = (RW + kSdRH - 1) / kSdRH;
    static_assert(kThinSteps == 3, "a thin item: sets 0 and 1, then the third fragment");
    auto is_thin = [&](int item) { return a.thin && item % a.rq == a.rq - 1; };
    h8 ahi[2][kSdAS], alo[2][kSdAS];
    if (it0 < it1) {
        const bool th = is_thin(it0);
        const unsigned adj0 = th ? thin_adjust() : 0u;
        const size_t stride0 = th ? kThinStride : kSdAStride;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int i = 0; i < kSdAS; ++i) {
                const h8* ap = a.xs + item_off(it0) + (size_t)p * stride0 + (aoff[i] + adj0);
                ahi[p][i] = ap[0]; alo[p][i] = ap[1];
            }
    }
    int since_flush = 0;
    int origin = 0;                                      // ring slot of the current window's row 0
    // One item of kind kind_c (a std::integral_constant): a full item, the full item in front of a thin one (its look-ahead loads
    // take the thin item's addresses), a thin item.  Three instantiations of this text, and the full items run in a loop of
    // their own (below), which is the item loop of a plan without thin items: with the kinds as the arms of a branch inside one
    // loop, hipcc no longer keeps the look-ahead loads in the registers of sets 0 and 1 and waits for them -- and for the window
    // copy -- at the end of every item.
    constexpr int kItemFull = 0, kItemBeforeThin = 1, kItemThin = 2;
    auto item = [&](const int it, auto kind_c) {
        constexpr bool thin = decltype(kind_c)::value == kItemThin, next_thin = decltype(kind_c)::value == kItemBeforeThin;
        const int oct = it / per_oct, reg = it - oct * per_oct, rx = reg / a.rq, ry = reg - rx * a.rq;
        // This wave's rows of the window were requested one item ago, before all of that item's A fragments; the newest eight
        // vector memory operations (the A fragments of this item's first two K steps) may stay in flight.  The barrier then
        // publishes every wave's rows, and every wave is done with the previous window.  (The builtin, not an asm statement:
        // hipcc takes it into its own bookkeeping and needs no wait of its own for registers reused in the item.)
        __builtin_amdgcn_s_waitcnt(kVmcnt8);
        __syncthreads();
        if (it > it0 && ry > 0) {
            origin = (origin + kSdRH) & (kRing - 1);     // the previous item is the region above: its rows RH .. WR - 1 stay
        } else {
            origin = 0;                                  // first item of the chunk or of a strip: the whole window
            fill(oct, ry, rx, 0, WR, 0);
            __builtin_amdgcn_s_waitcnt(kVmcnt0);
            __syncthreads();
        }
        // the RH new rows of the next item (the region below) into the slots of the previous window's first rows
        if (it + 1 < it1 && ry + 1 < a.rq) fill(oct, ry, rx, WR, kSdRH, origin);
        // LDS byte address of the unit's B column at K step 0; in a thin item: of K group 0's window row, j columns on
        const unsigned jt = thin ? (unsigned)j : 0u;
        int base[kSdAS][kSdGT];
#pragma unroll
        for (int i = 0; i < kSdAS; ++i)
#pragma unroll
            for (int gg = 0; gg < kSdGT; ++gg)
                base[i][gg] = (int)((((unsigned)origin + (uw[i][gg] & 15u) - jt) & (kRing - 1)) * RB + (uw[i][gg] >> 4) + jt * PB);
#ifdef DAU_SD_DIAG_AFIXED
        const size_t ioff = item_off(it0), ioff_next = ioff;
#else
        const size_t ioff = item_off(it);
        const size_t ioff_next = item_off(it + 1 < it1 ? it + 1 : it);
#endif
        // lane terms of the look-ahead loads / of a thin item's own third load (the chunk's last item looks ahead at its own
        // region, a dead load, as it did)
        unsigned nadj = 0u, tadj = 0u;
        if constexpr (next_thin) nadj = thin_adjust();
        if constexpr (thin) tadj = thin_adjust();
        constexpr size_t nstep = next_thin ? kThinStride : kSdAStride;
        (void)nadj; (void)tadj;
        f4s part[kSdAS][kSdGT];
#pragma unroll
        for (int i = 0; i < kSdAS; ++i)
#pragma unroll
            for (int gg = 0; gg < kSdGT; ++gg) part[i][gg] = f4s{0.0f, 0.0f, 0.0f, 0.0f};
        // Inside a K step the two input channels are two groups of 12 MFMAs (8 for EL = 1); the B fragments of group i + 1 are read from LDS
        // while group i runs, and what follows the MFMAs of group i (the odd step's fragment, the loads of channel i) is issued
        // while they run (sched barriers pin it).  The item is not unrolled whole: hipcc hoists loads of later steps until it
        // spills.
#ifdef DAU_SD_DIAG_NOA
#define SD_LOAD_INTO(AH, AL, i, an, ladj)
#else
#define SD_LOAD_INTO(AH, AL, i, an, ladj) { const h8* ap = a.xs + (an) + (aoff[i] + (ladj)); AH[i] = ap[0]; AL[i] = ap[1]; }
#endif
        // set P of channel i from the uniform offset `an`; SD_LOAD_NEXT: a look-ahead load of the next item (thin or not)
#define SD_LOAD_A(P, i, an) SD_LOAD_INTO(ahi[P], alo[P], i, an, 0u)
#define SD_LOAD_NEXT(P, i, an) SD_LOAD_INTO(ahi[P], alo[P], i, an, nadj)
#define SD_READ_B(i, bh, bl)                                                                                    \
    _Pragma("unroll") for (int gg = 0; gg < kSdGT; ++gg) {                                                      \
        const char* bp = lds + base[i][gg] + k * PB;                                                            \
        bh[gg] = *reinterpret_cast<const h8*>(bp);                                                              \
        if constexpr (EL == 2) bl[gg] = *reinterpret_cast<const h8*>(bp + 256);                                 \
    }
        // group i of a K step: the MFMAs on the fragment (AH, AL), then AFTER, between two sched barriers
#define SD_GROUP(i, AH, AL, bh, bl, AFTER)                                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                                          \
    _Pragma("unroll") for (int gg = 0; gg < kSdGT; ++gg) {                                                      \
        part[i][gg] = __builtin_amdgcn_mfma_f32_16x16x32_f16(AH, bh[gg], part[i][gg], 0, 0, 0);                 \
        part[i][gg] = __builtin_amdgcn_mfma_f32_16x16x32_f16(AL, bh[gg], part[i][gg], 0, 0, 0);                 \
        if constexpr (EL == 2) part[i][gg] = __builtin_amdgcn_mfma_f32_16x16x32_f16(AH, bl[gg], part[i][gg], 0, 0, 0); \
    }                                                                                                           \
    AFTER                                                                                                       \
    __builtin_amdgcn_sched_barrier(0);
#define SD_STEP(kk, AH, AL, AFTER0, AFTER1)                                                                     \
    {                                                                                                           \
        const int k = (kk);                                                                                     \
        h8 b0h[kSdGT], b0l[kSdGT], b1h[kSdGT], b1l[kSdGT];                                                      \
        SD_READ_B(0, b0h, b0l)                                                                                  \
        SD_READ_B(1, b1h, b1l)                                                                                  \
        SD_GROUP(0, AH[0], AL[0], b0h, b0l, AFTER0)                                                             \
        SD_GROUP(1, AH[1], AL[1], b1h, b1l, AFTER1)                                                             \
    }
        // bilinear combination of the four corners (lane-local), into the running sums
        auto combine = [&]() {
#pragma unroll
            for (int i = 0; i < kSdAS; ++i)
#pragma unroll
                for (int gg = 0; gg < kSdGT; ++gg) {
                    const int g = gb * kSdGT + gg;
                    const bool ok = s_ok[i] && g < a.G && f_ok;
                    const f4s p = part[i][gg], w = wb[i][gg];
                    float v = w[0] * p[0];
                    v = fmaf(w[1], p[1], v);
                    // (a line form: the corners on the row below are no terms at all -- a zero factor times a non-finite sum would be a NaN)
                    if constexpr (!kSdLine) {
                        v = fmaf(w[2], p[2], v);
                        v = fmaf(w[3], p[3], v);
                    }
                    run[i][gg] += ok ? v : 0.0f;
                }
        };
        static_assert(kSdAS == 2, "two groups per K step");
        h8 aqh[kSdAS], aql[kSdAS];                       // the odd steps' fragments; a thin item's third fragment
        if constexpr (thin) {
#define SD_READ_BT(kk, i, bh, bl)                                                                                 \
    _Pragma("unroll") for (int gg = 0; gg < kSdGT; ++gg) {                                                      \
        const char* bp = lds + base[i][gg] + 4 * (kk) * PB - dead;                                               \
        bh[gg] = *reinterpret_cast<const h8*>(bp);                                                              \
        if constexpr (EL == 2) bl[gg] = *reinterpret_cast<const h8*>(bp + 256);                                 \
    }
            // K step kk of a thin item: columns 4 kk + j; a group whose column lies in the next region reads column 4 kk
#define SD_THIN_STEP(kk, AH, AL, AFTER0, AFTER1)                                                                \
    {                                                                                                           \
        const int dead = 4 * (kk) + kSdRH <= RW || 4 * (kk) + j < RW ? 0 : j * PB;                              \
        h8 bh[kSdGT], bl[kSdGT];                                                                                \
        SD_READ_BT(kk, 0, bh, bl)                                                                               \
        SD_GROUP(0, AH[0], AL[0], bh, bl, AFTER0)                                                               \
        SD_READ_BT(kk, 1, bh, bl)                                                                               \
        SD_GROUP(1, AH[1], AL[1], bh, bl, AFTER1)                                                               \
    }
#define SD_LOAD_THIRD(i) SD_LOAD_INTO(aqh, aql, i, ioff + (size_t)(2 * kThinStride), tadj)
            SD_THIN_STEP(0, ahi[0], alo[0], SD_LOAD_THIRD(0) SD_LOAD_THIRD(1) SD_LOAD_NEXT(0, 0, ioff_next), SD_LOAD_NEXT(0, 1, ioff_next))
            SD_THIN_STEP(1, ahi[1], alo[1], SD_LOAD_NEXT(1, 0, ioff_next + nstep), SD_LOAD_NEXT(1, 1, ioff_next + nstep))
            if constexpr (4 * kThinSteps > RW) {
                const bool live = 4 * (kThinSteps - 1) + j < RW;
                const h8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int i = 0; i < kSdAS; ++i) { aqh[i] = live ? aqh[i] : zero; aql[i] = live ? aql[i] : zero; }
            }
            SD_THIN_STEP(2, aqh, aql, , )
            combine();
            // The look-ahead loads complete here, with no window copy in flight behind them: the next item then finds no load
            // of this instantiation outstanding, and hipcc's waits in the full items stay those of a kernel without thin items
            // (a wait it added there for a register loaded here would also drain the window copy, which it does not count).
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int i = 0; i < kSdAS; ++i) asm volatile("" : "+v"(ahi[p][i]), "+v"(alo[p][i]));
#undef SD_LOAD_THIRD
#undef SD_THIN_STEP
#undef SD_READ_BT
        } else {
#ifdef DAU_SD_STEP_LOADS
        // K step kk with the A set of its parity P; the set then fetches step kk + 2 (of the next item past the last step)
#define SD_STEP1(P, kk)                                                                                         \
    {                                                                                                           \
        const size_t an = (kk) + 2 < RW ? ioff + (size_t)((kk) + 2) * 2 : ioff_next + (size_t)((kk) + 2 - RW) * nstep; \
        const unsigned la = (kk) + 2 < RW ? 0u : nadj;                                                          \
        (void)an; (void)la;                                                                                     \
        SD_STEP(kk, ahi[P], alo[P], SD_LOAD_INTO(ahi[P], alo[P], 0, an, la), SD_LOAD_INTO(ahi[P], alo[P], 1, an, la)) \
    }
#pragma unroll 1
        for (int k2 = 0; k2 < RW; k2 += 2) {
            SD_STEP1(0, k2)
            SD_STEP1(1, k2 + 1)
        }
#undef SD_STEP1
#else
        // Pair r = K steps 2 r, 2 r + 1, its columns in set P.  Group i of the even step builds the odd step's fragment of
        // channel i from the two sets and then reloads set P with pair r + 2 of the item (r + 2 <= RW / 2).
#define SD_NEXT_COL(P, i)                                                                                       \
    aqh[i] = sd_next_col(ahi[P][i], ahi[1 - (P)][i], adx);                                                      \
    aql[i] = sd_next_col(alo[P][i], alo[1 - (P)][i], adx);
#define SD_PAIR(P, rr)                                                                                          \
    {                                                                                                           \
        const size_t an = ioff + (size_t)((rr) + 2) * 4;                                                        \
        (void)an;                                                                                               \
        SD_STEP(2 * (rr), ahi[P], alo[P], SD_NEXT_COL(P, 0) SD_LOAD_A(P, 0, an), SD_NEXT_COL(P, 1) SD_LOAD_A(P, 1, an)) \
        SD_STEP(2 * (rr) + 1, aqh, aql, , )                                                                     \
    }
        // the item's last pair: both sets are free once the odd step's fragment is built, and fetch pairs 0 and 1 of the next item
#define SD_PAIR_LAST(P, rr)                                                                                     \
    {                                                                                                           \
        SD_STEP(2 * (rr), ahi[P], alo[P], SD_NEXT_COL(P, 0) SD_LOAD_NEXT(0, 0, ioff_next), SD_NEXT_COL(P, 1) SD_LOAD_NEXT(0, 1, ioff_next)) \
        SD_STEP(2 * (rr) + 1, aqh, aql, SD_LOAD_NEXT(1, 0, ioff_next + nstep), SD_LOAD_NEXT(1, 1, ioff_next + nstep)) \
    }
        constexpr int kPairs = RW / 2, kLoopPairs = (kPairs - 1) / 2 * 2;   // the loop takes two pairs (one per set) at a time
#pragma unroll 1
        for (int r2 = 0; r2 < kLoopPairs; r2 += 2) {
            SD_PAIR(0, r2)
            SD_PAIR(1, r2 + 1)
        }
        if constexpr (kPairs - kLoopPairs == 2) {
            SD_PAIR(0, kPairs - 2)
            SD_PAIR_LAST(1, kPairs - 1)
        } else {
            SD_PAIR_LAST(0, kPairs - 1)
        }
#undef SD_NEXT_COL
#undef SD_PAIR
#undef SD_PAIR_LAST
#endif
            combine();
        }
#undef SD_LOAD_NEXT
#undef SD_LOAD_INTO
#undef SD_READ_B
#undef SD_GROUP
#undef SD_LOAD_A
#undef SD_STEP
        if (++since_flush == kSdFlushItems) { flush(); since_flush = 0; }
    };
    // the chunk's items: runs of full items, each up to its strip's thin item (or to the chunk's end), and that item
    for (int it = it0; it < it1;) {
        const int run_end = a.thin ? min(it1, it + (a.rq - 1 - it % a.rq)) : it1;   // the strip's thin item, if the chunk reaches it
        const int full_end = run_end < it1 ? run_end - 1 : run_end;
#pragma unroll 1
        for (; it < full_end; ++it) item(it, std::integral_constant<int, kItemFull>{});
        if (it < run_end) { item(it, std::integral_constant<int, kItemBeforeThin>{}); ++it; }
        if (it < it1) { item(it, std::integral_constant<int, kItemThin>{}); ++it; }
    }
    // the last item's look-ahead (a dead load) completes before any register is reused
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (since_flush) flush();
}

template <int RW>
__global__ void __launch_bounds__(kSdWaves * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) split_gather_dot_kernel(const SdArgs a) {
    sd_dot_body<RW, 2>(a);
}

// the one-limb-error member (bf16 activations): ES1, two products per tile and K step
template <int RW>
__global__ void __launch_bounds__(kSdWaves * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) sd_e1_dot_kernel(const SdArgs a) {
    sd_dot_body<RW, 1>(a);
}

template <int RW, int EL>
void launch_sd(hipStream_t st, const SdArgs* a, int grid) {
    auto kern = [] { if constexpr (EL == 2) return split_gather_dot_kernel<RW>; else return sd_e1_dot_kernel<RW>; }();
    const size_t lds = (size_t)(2 * kSdRH + 2 * kSdRY) * (RW + 2 * kSdRX) * 256 * EL;
    if (!a) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); return; }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kSdWaves * 64), lds, st, *a);
}
// Whether the x side of a plan is staged by sd_xk_walk_kernel (from the plan's shape alone): NCHW activations and an instantiated
// prefilter support.  Everything else -- NHWC plans, other supports -- keeps blur4_pack -> XK -> sd_stage_x_kernel, and so does
// every plan of the xk_copy build (-DDAU_SD_XK_COPY, libdau_conv_hip_xk_copy.so of `make tuning`: the A/B partner of the walking
// kernels and the bit-exact reference of tests/test_gpu_split_dot_xk_walk.py) and of the stage_ref build.
bool sd_walks(const SplitDotConfig& c) {
#if defined(DAU_SD_XK_COPY) || defined(DAU_SD_STAGE_REF)
    return false;
#else
    const SdGeom g = sd_geom(c);
    const long nct = (g.XTc + kXwCols - 1) / kXwCols;
    return !c.nhwc && (c.blur_k == 5 || c.blur_k == 7 || c.blur_k == 9) && (long)g.octs * c.sh.S * nct < (1L << 31);
#endif
}
template <int K, bool STORE>
void launch_xk_walk(hipStream_t st, const XkWalkArgs& a, int grid) {
    hipLaunchKernelGGL((sd_xk_walk_kernel<K, STORE>), dim3(grid), dim3(64), 0, st, a);
}
template <bool STORE>
void dispatch_xk_walk(hipStream_t st, const SplitDotConfig& c, const SdGeom& g, const float* x, const float* filters, unsigned* xmax,
                      h8* xs, const Guard& guard) {
    XkWalkArgs a{};
    a.x = x; a.taps = filters + kTaps1dOffset; a.xmax = xmax; a.xs = xs;
    a.N = c.sh.N; a.S = c.sh.S; a.H = c.sh.H; a.W = c.sh.W; a.XTr = g.XTr; a.XTc = g.XTc; a.act = c.act; a.relu_in = c.in_relu;
    a.nct = (g.XTc + kXwCols - 1) / kXwCols;
    a.guard = guard;
    const int grid = g.octs * c.sh.S * a.nct;
    if (c.blur_k == 5) launch_xk_walk<5, STORE>(st, a, grid);
    else if (c.blur_k == 7) launch_xk_walk<7, STORE>(st, a, grid);
    else launch_xk_walk<9, STORE>(st, a, grid);
}

void dispatch_sd(int RW, int e_limbs, hipStream_t st, const SdArgs* a, int grid) {
    if (e_limbs == 1) {
        if (RW == 10) launch_sd<10, 1>(st, a, grid);
        else launch_sd<12, 1>(st, a, grid);
    } else {
        if (RW == 10) launch_sd<10, 2>(st, a, grid);
        else launch_sd<12, 2>(st, a, grid);
    }
}

}  // namespace

bool split_dot_configure(const Shape& sh, int blur_k, int act, SplitDotConfig* cfg) {
    // the region width whose ring of error-window rows fits the LDS (RW <= 12) with the least work: the q columns (W + 1) padded
    // to a multiple of RW, plus about two K steps' worth of per-item cost (barrier, bilinear epilogue) per region
    int best = 0;
    long best_cost = 1L << 40;
    for (int rw = 12; rw >= 10; rw -= 2) {
        const long wq = (sh.W + 1 + rw - 1) / rw * rw;
        const long cost = wq * (rw + 2) * (60 / rw);                // wq * (rw + 2) / rw, scaled to an integer
        if (cost < best_cost) { best_cost = cost; best = rw; }
    }
    if ((size_t)(2 * kSdRH + 2 * kSdRY) * (best + 2 * kSdRX) * 512 > 160 * 1024) return false;
    if (!blur4_pack_fits(blur_k, sh.H, sh.W)) return false;
    SplitDotConfig c{};
    c.sh = sh; c.blur_k = blur_k; c.RW = best; c.act = act;
    // bf16 activations: the error in one limb.  -DDAU_SD_BF16_E2 (libdau_conv_hip_bf16_e2.so of `make tuning`) gives bf16 plans the
    // three-product kernel and the two-limb ES through widening loads instead: the bit-exact reference of
    // tests/test_gpu_bf16_split_dot.py and the A/B partner that tells what the one-limb form itself is worth.
#ifdef DAU_SD_BF16_E2
    c.e_limbs = 2;
#else
    c.e_limbs = act == kActBF16 ? 1 : 2;
#endif
    const SdGeom g = sd_geom(c);
    // 32-bit LDS / lane offsets; h8 offsets of the staged planes stay in size_t
    if ((long)g.EXs * 512 * 32 > (1L << 31)) return false;   // (the two-limb row; a one-limb row is half of it)
    *cfg = c;
    return true;
}

size_t split_dot_workspace_bytes(const SplitDotConfig& c) { return sd_layout(c, sd_geom(c)).total; }

void split_dot_strip(const SplitDotConfig& c, int* items, int* k_steps) {
    const SdGeom g = sd_geom(c);
    *items = g.rq; *k_steps = g.strip_steps;
}

void split_dot_init(const SplitDotConfig& c) {
    dispatch_sd(c.RW, c.e_limbs, nullptr, nullptr, 0);
#ifndef DAU_SD_STAGE_REF
    blur4_pack_init(c.blur_k, true, c.nhwc != 0);
#else
    blur4_pack_init(c.blur_k, false, c.nhwc != 0);
#endif
}

void split_dot_prepare(hipStream_t st, const SplitDotConfig& c, const float* x, const float* dy, const float* filters,
                       int drop_col, int drop_row, void* workspace, const Guard& guard) {
    const SdGeom g = sd_geom(c);
    const SdLayout l = sd_layout(c, g);
    const Shape& s = c.sh;
    char* ws = static_cast<char*>(workspace);
    unsigned* xmax = reinterpret_cast<unsigned*>(ws + l.maxes_off);
    unsigned* emax = xmax + s.S * kNumK;
    float* xk = reinterpret_cast<float*>(ws + l.xk_off);
    // (a kernel, not two memsets: in a replayed graph a memset node was seen to land among the maxima kernels that follow it --
    // every fourth word of the maxima cleared late -- while kernel follows kernel in order)
    hipLaunchKernelGGL(sd_zero_kernel, dim3(64), dim3(256), 0, st, xmax, (long)(s.S * kNumK + s.F),
                       reinterpret_cast<unsigned*>(ws + l.partial_off), (long)g.chunks * kNumK * s.S * s.G * s.F);
    const int HW = s.H * s.W;
    const bool walks = sd_walks(c);
    h8* xs = reinterpret_cast<h8*>(ws + l.xs_off);
#ifndef DAU_SD_STAGE_REF
    if (walks) dispatch_xk_walk<false>(st, c, g, x, filters, xmax, xs, guard);
    else launch_blur4_pack(st, x, filters, s.N, s.S, s.S, s.H, s.W, s.H, s.W, c.blur_k, c.act, xk, guard, xmax, c.nhwc != 0, c.in_relu != 0);
#else
    launch_blur4_pack(st, x, filters, s.N, s.S, s.S, s.H, s.W, s.H, s.W, c.blur_k, c.act, xk, guard, nullptr, c.nhwc != 0, c.in_relu != 0);
    const int xsplit = std::max(1, std::min(16, 2048 / std::max(1, s.S)));
    hipLaunchKernelGGL(sd_absmax_x_kernel, dim3(s.S * xsplit), dim3(256), 0, st, xk, g.NP, s.S, HW, xsplit, xmax, guard);
#endif
    if (c.nhwc) {
        const int nfb64 = (s.F + 63) / 64;
        const int esplit = (int)std::max(1L, std::min((long)(2048 / nfb64), ((long)s.N * HW + 3) / 4));
        hipLaunchKernelGGL(sd_absmax_nhwc_e_kernel, dim3(nfb64 * esplit), dim3(256), 0, st, dy, s.N, s.F, HW, esplit, c.act, emax, guard);
    } else {
        const int esplit = std::max(1, std::min(16, 2048 / std::max(1, s.F)));
        hipLaunchKernelGGL(sd_absmax_e_kernel, dim3(s.F * esplit), dim3(256), 0, st, dy, s.N, s.F, HW, esplit, c.act, emax, guard);
    }
    if (walks) dispatch_xk_walk<true>(st, c, g, x, filters, xmax, xs, guard);
    else hipLaunchKernelGGL(sd_stage_x_kernel, dim3(8192), dim3(256), 0, st, xk, xmax, s.N, g.NP, s.S, s.H, s.W, g.octs, g.XTr, g.XTc, xs, guard);
    if (c.e_limbs == 1) {
        const int nct = (g.EXs + kSe1TX - 1) / kSe1TX, tx = (g.EXs + nct - 1) / nct;  // column tiles of a window row, evenly wide
        if (c.nhwc) {
            hipLaunchKernelGGL(sd_stage_nhwc_e_kernel<1>, dim3((unsigned)(g.octs * g.nfb * g.EYs * nct)), dim3(256), 0, st, dy, emax, s.N, s.F,
                               s.H, s.W, g.nfb, g.EYs, g.EXs, nct, tx, drop_col, drop_row, c.act, reinterpret_cast<h8*>(ws + l.es_off), guard);
            return;
        }
        hipLaunchKernelGGL(sd_stage_e1_kernel, dim3((unsigned)(g.octs * g.nfb * g.EYs * nct)), dim3(256), 0, st, dy, emax, s.N, s.F,
                           s.H, s.W, g.nfb, g.EYs, g.EXs, nct, tx, drop_col, drop_row, c.act, reinterpret_cast<h8*>(ws + l.es_off), guard);
        return;
    }
#ifndef DAU_SD_STAGE_REF
    const int nct = (g.EXs + kSeTX - 1) / kSeTX, tx = (g.EXs + nct - 1) / nct;    // column tiles of a window row, evenly wide
    if (c.nhwc) {
        hipLaunchKernelGGL(sd_stage_nhwc_e_kernel<2>, dim3((unsigned)(g.octs * g.nfb * g.EYs * nct)), dim3(256), 0, st, dy, emax, s.N, s.F,
                           s.H, s.W, g.nfb, g.EYs, g.EXs, nct, tx, drop_col, drop_row, c.act, reinterpret_cast<h8*>(ws + l.es_off), guard);
        return;
    }
#ifndef DAU_SD_STAGE_E_ROWS
    // Bands: about two rounds of the ten waves per CU that the row images leave room for (5120 waves: the north-star pass is 1280
    // (octet, block, tile) columns in 4 bands of 17 rows), no band below four rows
    SeWalkArgs w{};
    w.dy = dy; w.emax = emax; w.es = reinterpret_cast<h8*>(ws + l.es_off);
    w.N = s.N; w.F = s.F; w.H = s.H; w.W = s.W; w.nfb = g.nfb; w.EYs = g.EYs; w.EXs = g.EXs;
    w.nct = (g.EXs + kSeCols - 1) / kSeCols;
    w.wlim = drop_col ? s.W - 1 : s.W; w.hlim = drop_row ? s.H - 1 : s.H; w.act = c.act; w.guard = guard;
    const long cols = (long)g.octs * g.nfb * w.nct, nb = (5120 + cols - 1) / cols;
    const int rb = DAU_TUNE_INT("DAU_SD_STAGE_E_RB", 0);     // tuning build: window rows per band
    w.RB = rb > 0 ? rb : std::max(4, (int)((g.EYs + nb - 1) / nb));
    w.nbands = (g.EYs + w.RB - 1) / w.RB;
    hipLaunchKernelGGL(sd_stage_e_kernel, dim3((unsigned)(cols * w.nbands)), dim3(64), 0, st, w);
    return;
#else
    hipLaunchKernelGGL(sd_stage_e_kernel, dim3((unsigned)(g.octs * g.nfb * g.EYs * nct)), dim3(256), 0, st, dy, emax, s.N, s.F, s.H,
                       s.W, g.nfb, g.EYs, g.EXs, nct, tx, drop_col, drop_row, c.act, reinterpret_cast<h8*>(ws + l.es_off), guard);
#endif
#else
    hipLaunchKernelGGL(sd_stage_e_kernel, dim3(4096), dim3(256), 0, st, dy, emax, s.N, s.F, s.H, s.W, g.octs, g.nfb, g.EYs, g.EXs,
                       drop_col, drop_row, c.act, c.nhwc, reinterpret_cast<h8*>(ws + l.es_off), guard);
#endif
}

void split_dot_run(hipStream_t st, const SplitDotConfig& c, const UnitRef* table, float* r4, void* workspace, const Guard& guard) {
    const SdGeom g = sd_geom(c);
    const SdLayout l = sd_layout(c, g);
    const Shape& s = c.sh;
    char* ws = static_cast<char*>(workspace);
    SdArgs a{};
    a.xs = reinterpret_cast<const h8*>(ws + l.xs_off);
    a.es = ws + l.es_off;
    a.xmax = reinterpret_cast<const unsigned*>(ws + l.maxes_off);
    a.emax = a.xmax + s.S * kNumK;
    a.table = table;
    a.partial = reinterpret_cast<float*>(ws + l.partial_off);
    a.S = s.S; a.F = s.F; a.G = s.G;
    a.nfb = g.nfb; a.nsb = g.nsb; a.ngb = g.ngb; a.per = g.per; a.items = g.items; a.rq = g.rq; a.cq = g.cq;
    a.XTr = g.XTr; a.XTc = g.XTc; a.EYs = g.EYs; a.EXs = g.EXs;
    a.thin = g.thin;
    a.guard = guard;
    dispatch_sd(c.RW, c.e_limbs, st, &a, g.chunks * g.nfb * g.nsb * g.ngb);
    launch_dot_reduce(st, a.partial, 1, (long)kNumK * s.S * s.G * s.F, s.G, s.F, s.G, g.chunks, g.chunks, s.G, false, r4, guard);
}

#ifdef DAU_SD_NS
}  // namespace DAU_SD_NS
#endif
}  // namespace dau
