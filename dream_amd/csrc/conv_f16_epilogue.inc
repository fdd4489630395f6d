// Epilogue of the implicit-GEMM kernels on the fp16 matrix cores, included at the end of conv_f16x3_kernel and conv_f16_kernel (one
// text, and the split kernel's machine code stays what was measured).  In scope: p, acc[MR][NR], inv, wm, wn, li, lh, b, y0, x0, n0,
// TW, pool, EPI_MASK (a bool constant).  acc * (inv * scale) + shift (+ residual) (ReLU) -> y, or the 2x2 window maximum; publishes
// max|y|.  EPI_MASK (conv_f16_mask_kernel only): `residual` is a ReLU mask, y = residual > 0 ? value : 0, max|y| taken after it.
    // ---- epilogue -----------------------------------------------------------------------------------------
    const bool relu = (p.flags & DREAM_CONV_RELU) != 0;
    const bool nchw = (p.flags & DREAM_CONV_OUT_NCHW) != 0;
    float scale_v[NR], shift_v[NR];
    int ncol[NR];
#pragma unroll
    for (int ns = 0; ns < NR; ++ns) {
        ncol[ns] = n0 + (wn * NR + ns) * 32 + li;
        const bool cok = ncol[ns] < p.Cout;
        scale_v[ns] = inv * ((p.scale != nullptr && cok) ? p.scale[ncol[ns]] : 1.0f);
        shift_v[ns] = (p.shift != nullptr && cok) ? p.shift[ncol[ns]] : 0.0f;
    }
    const int npix = p.TH * TW;
    float amax = 0.0f;
#pragma unroll
    for (int ms = 0; ms < MR; ++ms) {
        if (!pool) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = (wm * MR + ms) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                const int ty = (m * p.rcpTW) >> 16, tx = m - ty * TW;
                const int oy = (y0 + ty) * p.out_scale + p.out_oy, ox = (x0 + tx) * p.out_scale + p.out_ox;
                const bool ok = (m < npix) && (y0 + ty < p.H) && (x0 + tx < p.W) && oy < p.Ho && ox < p.Wo;
#pragma unroll
                for (int ns = 0; ns < NR; ++ns) {
                    if (ok && ncol[ns] < p.Cout) {
                        const size_t o = nchw
                            ? (((size_t)b * p.Cout + ncol[ns]) * p.Ho + oy) * p.Wo + ox
                            : (((size_t)b * p.Ho + oy) * p.Wo + ox) * p.Cout + ncol[ns];
                        float v = acc[ms][ns][r] * scale_v[ns] + shift_v[ns];
                        if constexpr (EPI_MASK) v = p.residual[o] > 0.0f ? v : 0.0f;
                        else if (p.residual != nullptr) v = v + p.residual[o];
                        if (relu) v = fmaxf(v, 0.0f);
                        p.y[o] = v;
                        amax = fmaxf(amax, fabsf(v));
                    }
                }
            }
        } else {
            // fused MaxPool2d(2): registers 4g..4g+3 of a lane are one 2x2 window (window-major tile order)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int m0 = (wm * MR + ms) * 32 + 8 * g4 + 4 * lh;
                const int q = m0 >> 2, hw = TW >> 1;
                const int wy = (q * p.rcpTW) >> 16, wx = q - wy * hw;
                const bool ok = (m0 < npix) && (y0 + 2 * wy + 1 < p.H) && (x0 + 2 * wx + 1 < p.W);
                const int oy = (y0 >> 1) + wy, ox = (x0 >> 1) + wx;
#pragma unroll
                for (int ns = 0; ns < NR; ++ns) {
                    if (ok && ncol[ns] < p.Cout) {
                        float best = -__builtin_huge_valf();
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            float v = acc[ms][ns][4 * g4 + j] * scale_v[ns] + shift_v[ns];
                            if (relu) v = fmaxf(v, 0.0f);
                            best = fmaxf(best, v);
                        }
                        p.y[(((size_t)b * p.Ho + oy) * p.Wo + ox) * p.Cout + ncol[ns]] = best;
                        amax = fmaxf(amax, fabsf(best));
                    }
                }
            }
        }
    }
    if (p.amax_out != nullptr) publish_amax(p.amax_out, amax);
