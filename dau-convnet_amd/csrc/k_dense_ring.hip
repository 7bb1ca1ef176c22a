// The ring pass of the radius-3 two-limb dense gather-sum with outliers (DAU_FLAG_DENSE_SPLIT_OUTLIERS).
//
// A unit whose offset lies in (3, 4] (or [-4, -3)) on an axis puts its bilinear corners on taps 3 and 4 of that axis.  The 7 x 7
// dense kernel of k_dense_split.hip (namespace s3) keeps the corners inside 7 x 7 and drops the others; the dropped ones all lie
// on the RING of the 9 x 9 kernel, |ty| = 4 or |tx| = 4 -- at most three per unit, integer displacements, no interpolation left:
//
//   P[n,f,y,x] = sum over the entries e of output channel f of  w_e * Xb[n, c_e, y + dy_e, x + dx_e]
//
// with Xb the blurred input the GEMM has already staged (XS: two binary16 limbs scaled by sx; Xb = (hi + lo) / sx, 22 bits).  The
// GEMM's epilogue adds P to its sums before the one rounding of the store (split_gather_kernel, ADD).  It replaces, for those
// corners, the same reference code as the gather (dau_conv_forward_core.hpp:804-1605).
//
// The list is built once per pass from the pass's unit table ([Cin][G][Cout]; the input-gradient pass hands in its mirrored table,
// so one mechanism serves both directions): one thread per (input channel, output channel) pair sums its units' ring corners per
// tap in unit order (as split_densify_kernel does for the inner taps), counts the non-zero taps; one workgroup scans the counts;
// the same threads then write their entries at their scanned position -- the list does not depend on scheduling.  Pairs are
// ordered (16-channel chunk, output channel, channel in chunk): the entries of a (chunk, output channel) cell are contiguous, and
// so are those of a chunk's run of output channels.
//
// The pass: workgroup = (image, 8 rows x 64 columns of pixels, 64 output channels); wave = row, lane = column, one accumulator
// register per output channel.  Per chunk that has entries for these channels the fp32 tile of the 16 input channels (with the halo
// of 4) is rebuilt in LDS from the limbs; the wave-uniform entry stream comes in through one vector load per 64 entries and is
// read lane by lane (v_readlane), one ds_read_b32 + FMA per entry.  Every output element is stored once, no atomics.
#include <algorithm>
#include <cstdint>

#include "dau_tiled.hpp"

namespace dau {

namespace {

constexpr int kRingTaps = 32;             // 9 x 9 less 7 x 7
constexpr int kRows = 8, kCols = 64;      // pixels of a workgroup tile
constexpr int kTR = kRows + 8, kTP = kCols + 8;   // tile with halo: rows, pitch
constexpr int kFB = 64;                   // output channels per workgroup
constexpr int kPassThreads = kRows * 64;
constexpr size_t kTileBytes = (size_t)16 * kTR * kTP * sizeof(float);
constexpr int kScanThreads = 1024;
constexpr int kPairThreads = 64;

struct RingEntry {
    float w;
    int off;      // byte offset of (channel in chunk, tap row, tap column) inside the LDS tile
};

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct RingLayout {
    long npairs;
    size_t pos_bytes, entry_bytes, partial_bytes;
};
RingLayout ring_layout(const RingConfig& c) {
    RingLayout l{};
    l.npairs = (long)c.nchunk * c.Cout * 16;
    l.pos_bytes = round_up((size_t)(l.npairs + 1) * sizeof(int), 256);
    l.entry_bytes = round_up((size_t)std::max(c.capacity, 1) * sizeof(RingEntry), 256);
    l.partial_bytes = round_up((size_t)c.N * c.Cout * c.H * c.W * sizeof(float), 256);
    return l;
}

// ring tap id of position (r, c) of the 9 x 9 kernel (r or c is 0 or 8), and back
__device__ __forceinline__ int ring_id(int r, int c) { return r == 0 ? c : r == 8 ? 9 + c : c == 0 ? 17 + r : 24 + r; }
__device__ __forceinline__ void ring_pos(int t, int& r, int& c) {
    if (t < 9) { r = 0; c = t; }
    else if (t < 18) { r = 8; c = t - 9; }
    else if (t < 25) { r = t - 17; c = 0; }
    else { r = t - 24; c = 8; }
}
__device__ __forceinline__ bool on_ring(int r, int c) { return r >= 0 && r <= 8 && c >= 0 && c <= 8 && (r == 0 || r == 8 || c == 0 || c == 8); }

}  // namespace

// pos[pair] = non-zero ring taps of the pair (FILL = false), or the pair's entries written at pos[pair] (FILL = true, after the scan)
template <bool FILL>
__global__ void __launch_bounds__(kPairThreads) ring_pairs_kernel(const UnitRef* __restrict__ table, int Cin, int G, int Cout, int* __restrict__ pos,
                                                                  RingEntry* __restrict__ entries, int capacity, const Guard guard) {
    __shared__ float acc[kRingTaps * kPairThreads];
    if (!guard_pass(guard)) return;
    const int tid = threadIdx.x, fblocks = (Cout + kPairThreads - 1) / kPairThreads;
    const int f = (blockIdx.x % fblocks) * kPairThreads + tid, c = blockIdx.x / fblocks;      // c < 16 * nchunk
    if (f >= Cout) return;
    const long pair = ((long)(c >> 4) * Cout + f) * 16 + (c & 15);
    int count = 0;
    bool any = false;
    if (c < Cin) {
        for (int g = 0; g < G; ++g) {
            const UnitRef u = table[((long)c * G + g) * Cout + f];
            const int r = u.oy + 4, q = u.ox + 4;
            any = any || on_ring(r, q) || on_ring(r, q + 1) || on_ring(r + 1, q) || on_ring(r + 1, q + 1);
        }
    }
    if (any) {
        for (int t = 0; t < kRingTaps; ++t) acc[t * kPairThreads + tid] = 0.0f;
        for (int g = 0; g < G; ++g) {                        // unit order, as split_densify_kernel sums the inner taps
            const UnitRef u = table[((long)c * G + g) * Cout + f];
            const int r = u.oy + 4, q = u.ox + 4;
            if (on_ring(r, q)) acc[ring_id(r, q) * kPairThreads + tid] += u.w00;
            if (on_ring(r, q + 1)) acc[ring_id(r, q + 1) * kPairThreads + tid] += u.w01;
            if (on_ring(r + 1, q)) acc[ring_id(r + 1, q) * kPairThreads + tid] += u.w10;
            if (on_ring(r + 1, q + 1)) acc[ring_id(r + 1, q + 1) * kPairThreads + tid] += u.w11;
        }
        int at = FILL ? pos[pair] : 0;
        for (int t = 0; t < kRingTaps; ++t) {
            const float w = acc[t * kPairThreads + tid];
            if (w != 0.0f) {
                if (FILL) {
                    int r, q;
                    ring_pos(t, r, q);
                    if (at < capacity) entries[at] = RingEntry{w, (((c & 15) * kTR + r) * kTP + q) * 4};
                    ++at;
                }
                ++count;
            }
        }
    }
    if (!FILL) pos[pair] = count;
}

// exclusive scan of pos[0 .. n) in place, pos[n] = total; one workgroup
__global__ void __launch_bounds__(kScanThreads) ring_scan_kernel(int* __restrict__ pos, long n, const Guard guard) {
    __shared__ int part[kScanThreads];
    if (!guard_pass(guard)) return;
    const int tid = threadIdx.x;
    const long seg = (n + kScanThreads - 1) / kScanThreads, a = tid * seg, b = a + seg < n ? a + seg : n;
    int sum = 0;
    for (long i = a; i < b; ++i) sum += pos[i];
    part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {             // inclusive scan of the segment sums
        const int v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - sum;
    for (long i = a; i < b; ++i) { const int v = pos[i]; pos[i] = run; run += v; }
    if (tid == kScanThreads - 1) pos[n] = part[tid];
}

struct RingPassArgs {
    const _Float16* xs;
    const float* sx;
    const int* pos;
    const RingEntry* entries;
    float* partial;
    Status* status;
    int N, Cout, H, W, Hs, Ws, nchunk, capacity;
    int nrb, ncb, nfb;
    Guard guard;
};

__global__ void __launch_bounds__(kPassThreads) ring_pass_kernel(const RingPassArgs a) {
    extern __shared__ __attribute__((aligned(16))) float tile[];   // [16 channels][kTR][kTP]
    typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
    if (!guard_pass(a.guard)) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&a.status->outlier_units, kRingTakenBit);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int t = blockIdx.x;
    const int fb = t % a.nfb; t /= a.nfb;                    // channel blocks fastest: they share the tile's window in L2
    const int cb = t % a.ncb; t /= a.ncb;
    const int rb = t % a.nrb;
    const int n = t / a.nrb;
    const int y0 = rb * kRows, x0 = cb * kCols, f0 = fb * kFB;
    const int nf = a.Cout - f0 < kFB ? a.Cout - f0 : kFB;
    const float inv_sx = 1.0f / a.sx[n];                     // this image's scale: a power of two
    const long splane = (long)a.Hs * a.Ws;
    const unsigned lane_base = (unsigned)((wave * kTP + lane) * 4);
    const char* tile_b = reinterpret_cast<const char*>(tile);

    float acc[kFB];
#pragma unroll
    for (int j = 0; j < kFB; ++j) acc[j] = 0.0f;

    for (int chunk = 0; chunk < a.nchunk; ++chunk) {
        // entry ranges of this chunk's cells (chunk, f0 + j): lane j holds the cell's begin and end
        const long cell0 = (long)chunk * a.Cout + f0;
        const int jl = lane < nf ? lane : nf, jh = lane + 1 < nf ? lane + 1 : nf;
        int ob = a.pos[(cell0 + jl) * 16], oe = a.pos[(cell0 + jh) * 16];
        ob = ob < a.capacity ? ob : a.capacity;
        oe = oe < a.capacity ? oe : a.capacity;
        const int e_begin = __builtin_amdgcn_readlane(ob, 0), e_end = __builtin_amdgcn_readlane(oe, kFB - 1);
        if (e_begin >= e_end) continue;                      // (uniform over the workgroup: every wave sees the same cells)
        __syncthreads();                                     // the previous chunk's reads of the tile are done
        {
            // the fp32 tile of the chunk's 16 channels: image rows y0 - 4 .. y0 + 11, columns x0 - 4 .. x0 + 67, zero outside the image
            const u32x4* src = reinterpret_cast<const u32x4*>(a.xs) + ((long)n * a.nchunk + chunk) * 4 * splane;
            for (int u = threadIdx.x; u < 2 * kTR * kTP; u += kPassThreads) {
                const int half = u / (kTR * kTP), rem = u - half * (kTR * kTP), r = rem / kTP, c = rem - r * kTP;
                const int y = y0 - 4 + r, x = x0 - 4 + c;
                const bool in = y >= 0 && y < a.H && x >= 0 && x < a.W;
                const long at = half * splane + (long)((in ? y : 0) + 3) * a.Ws + (in ? x : 0) + 3;   // staged position = image + 3
                const u32x4 hi = src[at], lo = src[at + 2 * splane];
                float* dst = tile + (half * 8 * kTR + r) * kTP + c;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float v0 = (f16_bits_to_float(hi[k] & 0xffffu) + f16_bits_to_float(lo[k] & 0xffffu)) * inv_sx;
                    const float v1 = (f16_bits_to_float(hi[k] >> 16) + f16_bits_to_float(lo[k] >> 16)) * inv_sx;
                    dst[(2 * k) * kTR * kTP] = in ? v0 : 0.0f;
                    dst[(2 * k + 1) * kTR * kTP] = in ? v1 : 0.0f;
                }
            }
        }
        __syncthreads();
        for (int b0 = e_begin; b0 < e_end; b0 += 64) {
            const int idx = b0 + lane < e_end ? b0 + lane : e_end - 1;
            const RingEntry ev = a.entries[idx];
            const int ew = __float_as_int(ev.w), eo = ev.off;
            const int b1 = b0 + 64 < e_end ? b0 + 64 : e_end;
#pragma unroll
            for (int j = 0; j < kFB; ++j) {
                int lo = __builtin_amdgcn_readlane(ob, j), hi = __builtin_amdgcn_readlane(oe, j);
                lo = lo > b0 ? lo : b0;
                hi = hi < b1 ? hi : b1;
                for (int i = lo; i < hi; ++i) {
                    const float w = __int_as_float(__builtin_amdgcn_readlane(ew, i - b0));
                    const unsigned off = (unsigned)__builtin_amdgcn_readlane(eo, i - b0);
                    acc[j] = fmaf(w, *reinterpret_cast<const float*>(tile_b + lane_base + off), acc[j]);
                }
            }
        }
    }
    const int y = y0 + wave, x = x0 + lane;
    if (y < a.H && x < a.W) {
        float* dst = a.partial + (((long)n * a.Cout + f0) * a.H + y) * a.W + x;
        const long plane = (long)a.H * a.W;
#pragma unroll
        for (int j = 0; j < kFB; ++j)
            if (j < nf) dst[j * plane] = acc[j];
    }
}

void ring_configure(const DenseConfig& d, long max_outlier_units, RingConfig* cfg) {
    RingConfig c{};
    c.N = d.N; c.Cin = d.Cin; c.Cout = d.Cout; c.G = d.G; c.H = d.H; c.W = d.W;
    c.nchunk = (d.Cin + 15) / 16;
    c.capacity = (int)std::min<long>(3 * max_outlier_units, (long)1 << 28);
    *cfg = c;
}

size_t ring_workspace_bytes(const RingConfig& c) {
    const RingLayout l = ring_layout(c);
    return l.pos_bytes + l.entry_bytes + l.partial_bytes;
}

void ring_init() {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(ring_pass_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTileBytes);
}

float* ring_partial(const RingConfig& c, void* workspace) {
    const RingLayout l = ring_layout(c);
    return reinterpret_cast<float*>(static_cast<char*>(workspace) + l.pos_bytes + l.entry_bytes);
}

void ring_build_list(hipStream_t st, const RingConfig& c, const UnitRef* table, void* workspace, const Guard& guard) {
    const RingLayout l = ring_layout(c);
    char* ws = static_cast<char*>(workspace);
    int* pos = reinterpret_cast<int*>(ws);
    RingEntry* entries = reinterpret_cast<RingEntry*>(ws + l.pos_bytes);
    const int grid = c.nchunk * 16 * ((c.Cout + kPairThreads - 1) / kPairThreads);
    hipLaunchKernelGGL(ring_pairs_kernel<false>, dim3(grid), dim3(kPairThreads), 0, st, table, c.Cin, c.G, c.Cout, pos, entries, c.capacity, guard);
    hipLaunchKernelGGL(ring_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, pos, l.npairs, guard);
    hipLaunchKernelGGL(ring_pairs_kernel<true>, dim3(grid), dim3(kPairThreads), 0, st, table, c.Cin, c.G, c.Cout, pos, entries, c.capacity, guard);
}

void ring_run(hipStream_t st, const RingConfig& c, const SplitStaged& staged, void* workspace, Status* status, const Guard& guard) {
    const RingLayout l = ring_layout(c);
    char* ws = static_cast<char*>(workspace);
    RingPassArgs a{};
    a.xs = staged.xs; a.sx = staged.sx;
    a.pos = reinterpret_cast<const int*>(ws);
    a.entries = reinterpret_cast<const RingEntry*>(ws + l.pos_bytes);
    a.partial = reinterpret_cast<float*>(ws + l.pos_bytes + l.entry_bytes);
    a.status = status;
    a.N = c.N; a.Cout = c.Cout; a.H = c.H; a.W = c.W; a.Hs = staged.Hs; a.Ws = staged.Ws; a.nchunk = c.nchunk; a.capacity = c.capacity;
    a.nrb = (c.H + kRows - 1) / kRows; a.ncb = (c.W + kCols - 1) / kCols; a.nfb = (c.Cout + kFB - 1) / kFB;
    a.guard = guard;
    hipLaunchKernelGGL(ring_pass_kernel, dim3(c.N * a.nrb * a.ncb * a.nfb), dim3(kPassThreads), kTileBytes, st, a);
}

}  // namespace dau
