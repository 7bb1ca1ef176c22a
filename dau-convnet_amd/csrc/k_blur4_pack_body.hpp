// The definition of blur4_pack_kernel (k_gather_dot.hip), included once per layout of the input: DAU_BLUR4_KERNEL names the kernel
// template, DAU_BLUR4_NHWC (false / true) says whether `in` is [N][C][H][W] or [N][H][W][C] (DAU_FLAG_IO_NHWC).  Two kernels from one
// text rather than one template with a layout argument or one body inlined into two kernels: the first would rename the NCHW
// instantiations, the second changed their code, and both must stay what they were.  NHWC: a lane's loads are C elements apart,
// so the workgroups of a window's channels are made neighbours on one XCD, whose L2 then serves the lines they share.
// (no include guard: included twice on purpose)
template <int K, bool KMAX>
__global__ void __launch_bounds__(512) DAU_BLUR4_KERNEL(const Blur4Args a) {
    constexpr bool NHWC = DAU_BLUR4_NHWC;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if (!guard_pass(a.guard)) return;
    // C counts the channel slots of the staged copy (cstride = input channels padded to whole workgroups of the
    // gather-dot); slots beyond the real channels are written as zero planes
    const int C = a.cstride, H = a.H, W = a.W, k = K ? K : a.k;
    const int Creal = a.C;
    const int lane = threadIdx.x & 63;
    const int nw = (blockDim.x >> 6) / a.ppb;     // waves per window
    const int sub = (threadIdx.x >> 6) / nw, wave = (threadIdx.x >> 6) % nw;
    int t = (NHWC ? xcd_contiguous_id(blockIdx.x, gridDim.x) : blockIdx.x) * a.ppb + sub;
    const bool active = t < a.items;              // idle wave groups of the last workgroup still reach the barriers
    if (!active) t = a.items - 1;
    const int c = t % C; t /= C;
    const int wx = t % a.nwx; t /= a.nwx;
    const int wy = t % a.nwy;
    const int np = t / a.nwy;
    const int oy0 = wy * a.WY, ox0 = wx * a.WX;
    const int oh = oy0 + a.WY < a.Hp ? a.WY : a.Hp - oy0, ow = ox0 + a.WX < a.Wp ? a.WX : a.Wp - ox0;
    const int kr = (k - 1) / 2;
    const int lw = ow + 2 * kr, lh = oh + 2 * kr;
    f2* A = reinterpret_cast<f2*>(lds + (size_t)sub * a.lds_item_floats);   // raw [lh][lw], image (oy0 - kr + r, ox0 - kr + xl)
    f2* B = A + (size_t)lh * lw;                             // [3][lh][ow]
    const float* tp[6] = {a.taps + kTapGX * kTapPitch, a.taps + kTapAX * kTapPitch, a.taps + kTapCX * kTapPitch,
                          a.taps + kTapGY * kTapPitch, a.taps + kTapAY * kTapPitch, a.taps + kTapBY * kTapPitch};
    float tr[6][K ? K : 1];
    if (K) {
#pragma unroll
        for (int q = 0; q < 6; ++q)
#pragma unroll
            for (int i = 0; i < K; ++i) tr[q][i] = tp[q][i];
    }
    auto tap = [&](int q, int i) { return K ? tr[q][i] : tp[q][i]; };
    const int n0 = 2 * np, n1 = 2 * np + 1;
    const bool real = c < Creal;
    const int cs = real ? c : 0;
    const long p0 = NHWC ? (long)n0 * H * W * Creal + cs : ((long)n0 * Creal + cs) * H * W;                    // element offsets
    const long p1 = NHWC ? (long)(n1 < a.N ? n1 : n0) * H * W * Creal + cs : ((long)(n1 < a.N ? n1 : n0) * Creal + cs) * H * W;
    const float m0 = real ? 1.0f : 0.0f;
    const float m1 = (real && n1 < a.N) ? 1.0f : 0.0f;
    // rows x cols of work for this window's waves: a wave per row when the rows are wide, a flat index when they are narrow
    auto for_each = [&](int rows_, int cols_, auto&& body) {
        if (cols_ >= 56) {
            for (int r = wave; r < rows_; r += nw)
                for (int x = lane; x < cols_; x += 64) body(r, x);
        } else {
            for (int t = wave * 64 + lane; t < rows_ * cols_; t += nw * 64) { const int r = t / cols_; body(r, t - r * cols_); }
        }
    };
    // raw window -> LDS, the loads of a batch in flight together (load_phase, dau_common.hpp)
    const bool ri = a.relu_in != 0;
    auto fill = [&](auto actc) {
        constexpr int AF = decltype(actc)::value;
        struct Raw2 { typename RawAct<AF>::type v0, v1; };
        load_phase<Raw2>(lh, lw, wave, nw, lane,
            [&](int r, int xl) {
                const int yy = oy0 - kr + r, xx = ox0 - kr + xl;
                const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
                const long off = in ? (NHWC ? ((long)yy * W + xx) * Creal : (long)yy * W + xx) : 0;   // outside the image: element 0 (valid), discarded
                return Raw2{load_raw<AF>(a.in, p0 + off), load_raw<AF>(a.in, p1 + off)};
            },
            [&](int r, int xl, Raw2 v) {
                const int yy = oy0 - kr + r, xx = ox0 - kr + xl;
                const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
                A[r * lw + xl] = f2{mask_act(m0 * relu_in(act_of(v.v0), ri), in), mask_act(m1 * relu_in(act_of(v.v1), ri), in)};
            });
    };
    with_act(a.act, fill);
    __syncthreads();
    for_each(lh, ow, [&](int r, int x) {
        const int yy = oy0 - kr + r;
        f2 h1 = {0.0f, 0.0f}, h2 = {0.0f, 0.0f}, h3 = {0.0f, 0.0f};
        if (yy >= 0 && yy < H) {
#pragma unroll
            for (int i = 0; i < k; ++i) {
                const f2 v = A[r * lw + x + i];
                h1 = __builtin_elementwise_fma(v, f2{tap(0, i), tap(0, i)}, h1);
                h2 = __builtin_elementwise_fma(v, f2{tap(1, i), tap(1, i)}, h2);
                h3 = __builtin_elementwise_fma(v, f2{tap(2, i), tap(2, i)}, h3);
            }
        }
        B[(0 * lh + r) * ow + x] = h1; B[(1 * lh + r) * ow + x] = h2; B[(2 * lh + r) * ow + x] = h3;
    });
    __syncthreads();
    f8* out = reinterpret_cast<f8*>(a.xk) + ((size_t)np * a.cstride + c) * a.Hp * a.Wp;
    // KMAX: the maxima are kept as keys (bits << 1) + 2^24: the shift drops the sign, and the addition wraps an Inf / NaN
    // (exponent 255) below the key of zero, so that an unsigned maximum passes over it: one v_lshl_add_u32 per value, one
    // v_max3_u32 per pair.  What kmax holds so far is read here, long before it is needed (below).
    constexpr unsigned kKeyZero = 1u << 24;
    unsigned km[4] = {kKeyZero, kKeyZero, kKeyZero, kKeyZero}, seen[4] = {0u, 0u, 0u, 0u};
    if constexpr (KMAX) {
#pragma unroll
        for (int q = 0; q < 4; ++q) seen[q] = __hip_atomic_load(a.kmax + c * kNumK + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for_each(active ? oh : 0, ow, [&](int yr, int xc) {
        const int yy = oy0 + yr, xx = ox0 + xc;
        f2 dw = {0.0f, 0.0f}, d1 = {0.0f, 0.0f}, d2 = {0.0f, 0.0f}, ds = {0.0f, 0.0f};
        if (yy < H && xx < W) {
#pragma unroll
            for (int j = 0; j < k; ++j) {
                const f2 b1 = B[(0 * lh + yr + j) * ow + xc], b2 = B[(1 * lh + yr + j) * ow + xc], b3 = B[(2 * lh + yr + j) * ow + xc];
                dw = __builtin_elementwise_fma(b1, f2{tap(3, j), tap(3, j)}, dw);
                d1 = __builtin_elementwise_fma(b2, f2{tap(3, j), tap(3, j)}, d1);
                d2 = __builtin_elementwise_fma(b1, f2{tap(4, j), tap(4, j)}, d2);
                ds = __builtin_elementwise_fma(b3, f2{tap(3, j), tap(3, j)}, ds);
                ds = __builtin_elementwise_fma(b1, f2{tap(5, j), tap(5, j)}, ds);
            }
        }
        out[(size_t)yy * a.Wp + xx] = f8{dw.x, dw.y, d1.x, d1.y, d2.x, d2.y, ds.x, ds.y};
        if constexpr (KMAX) {
            const f2 kv[4] = {dw, d1, d2, ds};
#pragma unroll
            for (int q = 0; q < 4; ++q)
                km[q] = max(max(km[q], (__float_as_uint(kv[q].x) << 1) + kKeyZero), (__float_as_uint(kv[q].y) << 1) + kKeyZero);
        }
    });
    if constexpr (KMAX) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            unsigned m = km[q];
            for (int o = 32; o >= 1; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
            // a maximum only grows: a value that does not exceed what was there when the workgroup began changes nothing (a
            // stale, smaller reading only costs the atomic) -- most waves issue none, and none waits for one
            const unsigned bits = (m - kKeyZero) >> 1;
            if (lane == 0 && bits > seen[q]) atomicMax(a.kmax + c * kNumK + q, bits);
        }
    }
}
