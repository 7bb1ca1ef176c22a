// The epilogue of gather_body (k_gather_mfma.hip), one text compiled twice inside it: on the kernel's arguments as they are
// (DAU_E = a), and -- the instantiations with the fused bias / ReLU -- on a copy of them read after the tap loop (DAU_E = late).
// Uses gather_body's locals.
    // ---- epilogue: out[p] = Z0[p] + Z1[p+(0,1)] + Z2[p+(1,0)] + Z3[p+(1,1)] through LDS ---------------
    // per round: one image of the pair, kEpiF output channels, all SK planes
    const unsigned zpitch = DAU_E.zpitch;
    const unsigned zplane = (unsigned)(H + 1) * zpitch;       // floats per tap plane
    const unsigned zchan = 4 * zplane;                        // floats per (plane, output channel)
    float* zs = reinterpret_cast<float*>(smem);
    const int HW = H * W;
    const long plane_out = (long)DAU_E.H * DAU_E.W;
#pragma unroll
    for (int img = 0; img < 2; ++img) {   // unrolled: acc[i][img] must be a static register index
#pragma unroll 1
        for (int fh = 0; fh < T::FB / T::kEpiF; ++fh) {
            __syncthreads();
            if (fi / T::kEpiF == fh) {
#pragma unroll
                for (int i = 0; i < KP; ++i) {
                    constexpr int first = PART * KP;
                    const int flat = first + i;
                    const int k = flat / T::kPlaneTiles, tile = flat % T::kPlaneTiles;
                    int y, x; bool ok;
                    if (flat >= T::kTiles) { y = 0; x = 0; ok = false; }
                    else if (tile < T::kRegular) { y = (tile / TX) * T::TH + ly; x = (tile % TX) * T::TW + lx; ok = (y <= H) && (x <= W); }
                    else if (tile == T::kRegular) { y = ey[0]; x = ex[0]; ok = evalid[0]; }
                    else { y = ey[1]; x = ex[1]; ok = evalid[1]; }
                    if (ok) {
                        const f4 v = acc[i][img];
                        float* q = zs + (size_t)(k * T::kEpiF + fi % T::kEpiF) * zchan + (unsigned)y * zpitch + x;
                        q[0] = v[0]; q[zplane] = v[1]; q[2 * zplane] = v[2]; q[3 * zplane] = v[3];
                    }
                }
            }
            __syncthreads();
            for (int o = threadIdx.x; o < SK * T::kEpiF * HW; o += T::kThreads) {
                const int kf = o / HW;                     // (plane, channel of the round)
                const int k = kf / T::kEpiF, fl = kf % T::kEpiF;
                const int p = o % HW, y = p / W, x = p % W;
                const int f = fb * T::FB + fh * T::kEpiF + fl;
                const int npp = npp0 + k;
                const int n = 2 * (npp / npatch) + img, patch = npp % npatch;
                const int gy = (patch / DAU_E.npx) * H + y, gx = (patch % DAU_E.npx) * W + x;
                const float* zf = zs + (size_t)kf * zchan + (unsigned)y * zpitch + x;
                const float v = zf[0] + zf[zplane + 1] + zf[2 * zplane + zpitch] + zf[3 * zplane + zpitch + 1];
                if (npp < npp_total && n < DAU_E.N && f < DAU_E.Cout && gy < DAU_E.H && gx < DAU_E.W)
                {
                    const long o = NHWC ? nhwc_index(n, f, gy, gx, DAU_E.Cout, DAU_E.H, DAU_E.W) : ((long)n * DAU_E.Cout + f) * plane_out + (long)gy * DAU_E.W + gx;
                    if constexpr (EPI) {
                        const float sum = DAU_E.accumulate ? load_act(DAU_E.out, o, H16 ? (int)kActF16 : DAU_E.act) + v : v;
                        const float res = DAU_E.residual ? load_act(DAU_E.residual, o, H16 ? (int)kActF16 : DAU_E.act) : 0.0f;
                        float r = epilogue_value(sum, DAU_E.bias ? DAU_E.bias[f] : 0.0f, DAU_E.bias != nullptr, DAU_E.relu != 0, res,
                                                 DAU_E.residual != nullptr);
                        if (gate_ptr) r = gate_value(r, load_act(gate_ptr, o, H16 ? (int)kActF16 : DAU_E.act));
                        if constexpr (H16) store_act_t<kActF16>(DAU_E.out, o, r, false);
                        else store_act(DAU_E.out, o, r, DAU_E.act != 0, false);
                    } else
                    if constexpr (H16) store_act_t<kActF16>(DAU_E.out, o, v, DAU_E.accumulate != 0);
                    else store_act(DAU_E.out, o, v, DAU_E.act != 0, DAU_E.accumulate != 0);          // act: kActF32 or kActBF16
                }
            }
        }
    }
