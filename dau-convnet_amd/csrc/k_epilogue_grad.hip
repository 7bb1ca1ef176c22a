// Backward of the fused epilogue y = act(sum + bias[f]) (dau_conv_epilogue_backward): one pass over dy (and, with ReLU, the stored y)
//   dz      = (y <= 0) ? 0 : dy          the rule of aten::threshold_backward: a NaN y passes dy through; dz keeps dy's bits, in the
//                                        activations' format and layout; written only with ReLU (without it dz IS dy)
//   dbias[f] = sum over n, h, w of dz    in fp32
// No atomics: every workgroup leaves one partial sum per channel in the workspace, partial[f][b], and reduce_partials_kernel adds them
// up in a fixed order, 4096 per workgroup and level, until one is left -- two runs give the same bits.
//
// Chain length (fp32 additions a value passes through on its way into dbias[f]):
//   first pass    at most 64 in its thread (kPerThread values, one after the other)
//                 + 6 across the wave (butterfly) + 3 across the four waves (NCHW), or + 8 across the rows of the workgroup (NHWC tree)
//                 = at most 73
//   every level   16 in a thread + 6 across the wave + 3 across the waves = 25; a workgroup of the first pass covers 16384 elements of a
//                 channel (NCHW) or 64 rows of pixels (NHWC), so a channel of 2^31 elements leaves at most 2^31 / 64 = 2^25 partials:
//                 at most three levels (4096^3 = 2^36)
//   total         at most 73 + 3 * 25 = 148 <= 256 for every tensor up to 2^31 elements, whatever its shape.
// Loads and stores are 16 bytes wide (four fp32 or eight 16-bit elements) where the bases are 16-byte aligned and the run length (H * W
// for NCHW, the channel count for NHWC) is a multiple of the vector, element-wise otherwise: the alignment rule of DAU_FLAG_IO_NHWC.
// Both forms add the same values in the same order.
#include "dau_common.hpp"
#include "dau_tiled.hpp"

namespace dau {

namespace {

constexpr int kThreads = 256;
constexpr int kPerThread = 64;                       // values a thread of the first pass adds up, one after the other
constexpr int kChunk = kThreads * kPerThread;        // elements of one channel a workgroup of the NCHW pass covers
constexpr int kLevel = kThreads * 16;                // partials a workgroup of reduce_partials_kernel adds up
constexpr int kBatch = 4;                            // vector loads a thread keeps in flight per tensor

template <int A> constexpr int vec_of() { return A == kActF32 ? 4 : 8; }

// V elements from element index idx on, as zero-extended bits
template <int A, int V>
__device__ __forceinline__ void load_bits(const void* base, long idx, unsigned (&b)[V]) {
    if constexpr (V == 1) {
        if constexpr (A == kActF32) b[0] = static_cast<const unsigned*>(base)[idx];
        else b[0] = static_cast<const unsigned short*>(base)[idx];
    } else {
        const uint4 w = *reinterpret_cast<const uint4*>(static_cast<const char*>(base) + idx * (A == kActF32 ? 4 : 2));
        const unsigned q[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if constexpr (A == kActF32) b[k] = q[k];
            else { b[2 * k] = q[k] & 0xffffu; b[2 * k + 1] = q[k] >> 16; }
        }
    }
}
template <int A, int V>
__device__ __forceinline__ void store_bits(void* base, long idx, const unsigned (&b)[V]) {
    if constexpr (V == 1) {
        if constexpr (A == kActF32) static_cast<unsigned*>(base)[idx] = b[0];
        else static_cast<unsigned short*>(base)[idx] = (unsigned short)b[0];
    } else {
        uint4 w;
        if constexpr (A == kActF32) w = make_uint4(b[0], b[1], b[2], b[3]);
        else w = make_uint4(b[0] | (b[1] << 16), b[2] | (b[3] << 16), b[4] | (b[5] << 16), b[6] | (b[7] << 16));
        *reinterpret_cast<uint4*>(static_cast<char*>(base) + idx * (A == kActF32 ? 4 : 2)) = w;
    }
}
template <int A>
__device__ __forceinline__ float widen(unsigned bits) {
    if constexpr (A == kActF32) return __uint_as_float(bits);
    else if constexpr (A == kActBF16) return __uint_as_float(bits << 16);
    else return f16_bits_to_float(bits);
}

struct GradArgs {
    const void* dy;
    const void* y;            // with relu
    void* dz;                 // with relu (may be dy)
    float* partial;           // [F][B], with sum
    long N, HW, P;            // images, positions per plane, pixels N * H * W
    int F;
    long B;                   // partials per channel
    int ipb, cpp;             // NCHW: images per workgroup (planes shorter than a chunk), chunks per plane (longer ones)
    int gcols, rows, ntile;   // NHWC: channel groups and pixel rows of a workgroup, channel tiles
    int relu, sum;
};

// the sum of `v` over the workgroup's four waves, in thread 0 (6 + 3 additions)
__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// dz bits and the value that enters the sum, of one element
template <int A>
__device__ __forceinline__ unsigned dz_of(unsigned dy_bits, unsigned y_bits, bool relu, bool valid, float* add) {
    const bool cut = relu && widen<A>(y_bits) <= 0.0f;
    const unsigned bits = cut ? 0u : dy_bits;
    *add = valid ? widen<A>(bits) : 0.0f;
    return bits;
}

// NCHW: lanes run along a plane.  Workgroup (b, f): elements j0 .. j0 + cnt - 1 of channel f in the images from n0 on -- a chunk of one
// long plane, or up to ipb whole short planes.
template <int A, int V>
__global__ void __launch_bounds__(kThreads) epilogue_grad_nchw_kernel(const GradArgs a) {
    __shared__ float red[4];
    const int f = (int)(blockIdx.x % (unsigned)a.F);
    const long b = blockIdx.x / (unsigned)a.F;
    long n0, j0, cnt;
    if (a.cpp > 1) {
        n0 = b / a.cpp; j0 = (b % a.cpp) * kChunk;
        cnt = a.HW - j0 < kChunk ? a.HW - j0 : kChunk;
    } else {
        n0 = b * a.ipb; j0 = 0;
        cnt = (a.N - n0 < a.ipb ? a.N - n0 : a.ipb) * a.HW;
    }
    const unsigned hw = a.cpp > 1 ? 1u : (unsigned)a.HW;     // (short planes: HW <= kChunk)
    float acc = 0.0f;
    for (int it0 = 0; it0 < kPerThread / V; it0 += kBatch) {
        unsigned dyb[kBatch][V], yb[kBatch][V];
        long idx[kBatch];
        bool valid[kBatch];
        // branch-free loads: a thread past the end loads element 0 and keeps nothing of it
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const long j = ((long)(it0 + u) * kThreads + threadIdx.x) * V;
            valid[u] = j < cnt;
            long e = 0;
            if (a.cpp > 1) e = (n0 * a.F + f) * a.HW + j0 + j;
            else { const unsigned q = (unsigned)j / hw, r = (unsigned)j - q * hw; e = ((n0 + q) * a.F + f) * a.HW + r; }
            idx[u] = valid[u] ? e : 0;
            load_bits<A, V>(a.dy, idx[u], dyb[u]);
            if (a.relu) load_bits<A, V>(a.y, idx[u], yb[u]);
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            unsigned out[V];
#pragma unroll
            for (int k = 0; k < V; ++k) {
                float add;
                out[k] = dz_of<A>(dyb[u][k], a.relu ? yb[u][k] : 0u, a.relu != 0, valid[u], &add);
                acc += add;
            }
            if (a.relu && valid[u]) store_bits<A, V>(a.dz, idx[u], out);
        }
    }
    if (!a.sum) return;
    const float total = block_sum(acc, red);
    if (threadIdx.x == 0) a.partial[(long)f * a.B + b] = total;
}

// NHWC: lanes run along channels.  Workgroup (bx, tile): gcols channel groups of V channels x rows pixel rows; a thread walks kPerThread
// pixels, rows apart; the rows are added up through LDS (a tree: at most eight additions).
template <int A, int V>
__global__ void __launch_bounds__(kThreads) epilogue_grad_nhwc_kernel(const GradArgs a) {
    __shared__ float red[kThreads * V];
    const int tile = (int)(blockIdx.x % (unsigned)a.ntile);
    const long bx = blockIdx.x / (unsigned)a.ntile;
    const int col = threadIdx.x % a.gcols, row = threadIdx.x / a.gcols;
    const long c0 = ((long)tile * kThreads + col) * V;
    const bool live = row < a.rows && c0 < a.F;               // (vector form: F is a multiple of V, the whole group lies inside)
    const long p0 = bx * (long)a.rows * kPerThread + row;
    float acc[V];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.0f;
    for (int it0 = 0; it0 < kPerThread; it0 += kBatch) {
        unsigned dyb[kBatch][V], yb[kBatch][V];
        long idx[kBatch];
        bool valid[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const long p = p0 + (long)(it0 + u) * a.rows;
            valid[u] = live && p < a.P;
            idx[u] = valid[u] ? p * a.F + c0 : 0;
            load_bits<A, V>(a.dy, idx[u], dyb[u]);
            if (a.relu) load_bits<A, V>(a.y, idx[u], yb[u]);
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            unsigned out[V];
#pragma unroll
            for (int k = 0; k < V; ++k) {
                float add;
                out[k] = dz_of<A>(dyb[u][k], a.relu ? yb[u][k] : 0u, a.relu != 0, valid[u], &add);
                acc[k] += add;
            }
            if (a.relu && valid[u]) store_bits<A, V>(a.dz, idx[u], out);
        }
    }
    if (!a.sum) return;
    float* mine = red + (row * a.gcols + col) * V;
    if (row < a.rows) {
#pragma unroll
        for (int k = 0; k < V; ++k) mine[k] = acc[k];
    }
    int half = 1;
    while (half < a.rows) half <<= 1;
    for (half >>= 1; half >= 1; half >>= 1) {
        __syncthreads();
        if (row < half && row + half < a.rows) {
#pragma unroll
            for (int k = 0; k < V; ++k) mine[k] += mine[half * a.gcols * V + k];
        }
    }
    if (row == 0 && c0 < a.F) {
#pragma unroll
        for (int k = 0; k < V; ++k) a.partial[(c0 + k) * a.B + bx] = mine[k];
    }
}

// out[f][j] = the sum of in[f][j * 4096 .. + 4095] (what there is of them); workgroup (j, f)
__global__ void __launch_bounds__(kThreads) reduce_partials_kernel(const float* __restrict__ in, long B, float* __restrict__ out, long B2) {
    __shared__ float red[4];
    const long f = blockIdx.x / (unsigned long)B2, j = blockIdx.x % (unsigned long)B2;
    const float* src = in + f * B + j * kLevel;
    const long cnt = B - j * kLevel < kLevel ? B - j * kLevel : kLevel;
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < kLevel / kThreads; ++i) {
        const long k = (long)i * kThreads + threadIdx.x;
        acc += k < cnt ? src[k] : 0.0f;
    }
    const float total = block_sum(acc, red);
    if (threadIdx.x == 0) out[f * B2 + j] = total;
}

struct GradGeom {
    long B;                   // partials per channel after the first pass
    int ipb, cpp, gcols, rows, ntile;
    long blocks;
};

GradGeom grad_geometry(long N, int F, long HW, bool nhwc, int V) {
    GradGeom g{};
    if (nhwc) {
        const long gp = (F + V - 1) / V;                     // channel groups of a pixel
        g.gcols = (int)(gp < kThreads ? gp : kThreads);
        g.rows = kThreads / g.gcols;
        g.ntile = (int)((gp + kThreads - 1) / kThreads);
        const long per = (long)g.rows * kPerThread, P = N * HW;
        g.B = (P + per - 1) / per;
        g.blocks = g.B * g.ntile;
    } else {
        if (HW > kChunk) { g.cpp = (int)((HW + kChunk - 1) / kChunk); g.ipb = 1; g.B = N * g.cpp; }
        else { g.cpp = 1; g.ipb = (int)(kChunk / HW); g.B = (N + g.ipb - 1) / g.ipb; }
        g.blocks = g.B * F;
    }
    return g;
}

inline size_t round256(size_t v) { return (v + 255) / 256 * 256; }

template <int A>
void launch_first(hipStream_t st, const GradArgs& a, bool nhwc, bool vec, long blocks) {
    constexpr int V = vec_of<A>();
    if (nhwc) {
        if (vec) hipLaunchKernelGGL((epilogue_grad_nhwc_kernel<A, V>), dim3((unsigned)blocks), dim3(kThreads), 0, st, a);
        else hipLaunchKernelGGL((epilogue_grad_nhwc_kernel<A, 1>), dim3((unsigned)blocks), dim3(kThreads), 0, st, a);
    } else {
        if (vec) hipLaunchKernelGGL((epilogue_grad_nchw_kernel<A, V>), dim3((unsigned)blocks), dim3(kThreads), 0, st, a);
        else hipLaunchKernelGGL((epilogue_grad_nchw_kernel<A, 1>), dim3((unsigned)blocks), dim3(kThreads), 0, st, a);
    }
}

}  // namespace

size_t epilogue_grad_workspace_bytes(long N, int F, int H, int W, int act, bool nhwc) {
    // the element-wise form of an NHWC call has fewer pixel rows per workgroup, hence more partials, than the vector form: room for both
    const long HW = (long)H * W;
    const long b1 = grad_geometry(N, F, HW, nhwc, 1).B, bv = grad_geometry(N, F, HW, nhwc, act == kActF32 ? 4 : 8).B;
    const long B = b1 > bv ? b1 : bv;
    return round256((size_t)F * B * sizeof(float)) + round256((size_t)F * ((B + kLevel - 1) / kLevel) * sizeof(float));
}

bool epilogue_grad_run(hipStream_t st, long N, int F, int H, int W, int act, bool nhwc, const float* dy, const float* y, bool relu,
                       float* dz, float* dbias, void* workspace) {
    if (!relu && !dbias) return true;
    const long HW = (long)H * W;
    const int V = act == kActF32 ? 4 : 8;
    auto aligned = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
    const bool vec = (nhwc ? F % V == 0 : HW % V == 0) && aligned(dy) && (!relu || (aligned(y) && aligned(dz)));
    const GradGeom g = grad_geometry(N, F, HW, nhwc, vec ? V : 1);
    if (g.blocks > 0x7fffffffl || g.B > 0x7fffffffl) return false;
    GradArgs a{};
    a.dy = dy; a.y = y; a.dz = dz;
    a.N = N; a.HW = HW; a.P = N * HW; a.F = F; a.B = g.B;
    a.ipb = g.ipb; a.cpp = g.cpp; a.gcols = g.gcols; a.rows = g.rows; a.ntile = g.ntile;
    a.relu = relu ? 1 : 0; a.sum = dbias ? 1 : 0;
    char* ws = static_cast<char*>(workspace);
    float* bufs[2] = {reinterpret_cast<float*>(ws), nullptr};
    {
        const long b1 = grad_geometry(N, F, HW, nhwc, 1).B, bv = grad_geometry(N, F, HW, nhwc, V).B;
        bufs[1] = reinterpret_cast<float*>(ws + round256((size_t)F * (b1 > bv ? b1 : bv) * sizeof(float)));
    }
    a.partial = bufs[0];
    if (act == kActF16) launch_first<kActF16>(st, a, nhwc, vec, g.blocks);
    else if (act == kActBF16) launch_first<kActBF16>(st, a, nhwc, vec, g.blocks);
    else launch_first<kActF32>(st, a, nhwc, vec, g.blocks);
    if (!dbias) return true;
    // levels of 4096 until one partial per channel is left; the last level writes dbias
    long B = g.B;
    int cur = 0;
    for (;;) {
        const long B2 = (B + kLevel - 1) / kLevel;
        float* out = B2 == 1 ? dbias : bufs[cur ^ 1];
        hipLaunchKernelGGL(reduce_partials_kernel, dim3((unsigned)(B2 * F)), dim3(kThreads), 0, st, bufs[cur], B, out, B2);
        if (B2 == 1) break;
        B = B2; cur ^= 1;
    }
    return true;
}

}  // namespace dau
