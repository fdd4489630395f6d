// Epilogue of the implicit-GEMM kernels on the fp16 matrix cores, included at the end of conv_f16x3_kernel and conv_f16_kernel (one
// text, and the split kernel's machine code stays what was measured).  In scope: p, acc[MR][NR], inv, wm, wn, li, lh, b, y0, x0, n0,
// TW, pool, EPI_MASK and ACT16 (bool constants).  acc * (inv * scale) + shift (+ residual) (ReLU) -> y, or the 2x2 window maximum; publishes
// max|y|.  The constants are those of a form of conv_f16_kernel (the kForms table of conv_f16.hip; all false / 0 in the split kernel).
// EPI_MASK: `residual` is a ReLU mask, y = residual > 0 ? value : 0, max|y| taken after it; MASK16: that mask is a tensor of IEEE halfs.
// ACT16 (the half-storage kernels of conv_f16.hip): an NHWC y is IEEE half -- the same value, saturated to +-65504 and rounded to
// nearest even (sat_half); max|y| is taken BEFORE the saturation, so the side channel tells a caller that it happened.  The NCHW
// output (the K-channel belief maps) stays fp32.
// GRAD16 (int constant; conv_f16.hip, 0 everywhere else): the forms of a half-stored data gradient -- 1 entry: y * 2^e_g stored as half
// whatever ACT16 says (x is fp32); 2 interior: ACT16's store with MASK16's mask; 3 exit: y * 2^-e_g stored as fp32 (x is half).
// RES16 (bool constant; conv_f16.hip, false everywhere else): with ACT16, `residual` is a tensor of IEEE halfs of the output's shape,
// added before the ReLU; the peak is taken behind both.  The paired store reads it as the pair of halfs that the lane stores.
    // ---- epilogue -----------------------------------------------------------------------------------------
    constexpr bool OUT16 = GRAD16 == 0 ? ACT16 : GRAD16 != 3;      // an NHWC y is IEEE half
    float gs = 1.0f;                                               // (GRAD16 entry / exit) 2^e_g / 2^-e_g, applied to the finished value
    if constexpr (GRAD16 == 1 || GRAD16 == 3) {
        const int eg = grad_scale_exponent(*p.grad_amax);
        gs = pow2f(GRAD16 == 1 ? eg : -eg);
    }
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
    bool stored = false;
    // ACT16, NHWC, not pooled, even Cout: a lane owns one channel, so the plain store below is 2 bytes per lane.  Here the two lanes of
    // a pair (channels 2j, 2j + 1) swap one of every two values (DPP quad_perm [1,0,3,2]): the even lane stores both channels of the
    // first tile row of the two, the odd lane those of the second -- half the store instructions, 4 bytes per lane (+2 .. +9 % on the
    // layer; the pooled form, a quarter of the stores to begin with, measured no gain and keeps the plain store:
    // profiles/ab_act16_store.txt).  Every lane runs every exchange (the validity tests only guard the stores).
    if constexpr (OUT16) {
        if (!nchw && !pool && (p.Cout & 1) == 0) {
            stored = true;
            typedef _Float16 f16x2_ __attribute__((ext_vector_type(2)));
            _Float16 *yh = (_Float16 *)p.y;
            const int odd = li & 1;
#pragma unroll
            for (int ms = 0; ms < MR; ++ms) {
#pragma unroll
                for (int r2 = 0; r2 < 8; ++r2) {                 // registers 2 r2, 2 r2 + 1: two tile rows
                    bool ok[2];
                    size_t pix[2];
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const int r = 2 * r2 + j;
                        const int m = (wm * MR + ms) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                        const int ty = (m * p.rcpTW) >> 16, tx = m - ty * TW;
                        const int oy = (y0 + ty) * p.out_scale + p.out_oy, ox = (x0 + tx) * p.out_scale + p.out_ox;
                        ok[j] = (m < npix) && (y0 + ty < p.H) && (x0 + tx < p.W) && oy < p.Ho && ox < p.Wo;
                        pix[j] = ((size_t)b * p.Ho + oy) * p.Wo + ox;
                    }
#pragma unroll
                    for (int ns = 0; ns < NR; ++ns) {
                        const bool cok = ncol[ns] < p.Cout;
                        float v[2];
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            v[j] = acc[ms][ns][2 * r2 + j] * scale_v[ns] + shift_v[ns];
                            if (!RES16 && relu) v[j] = fmaxf(v[j], 0.0f);     // (RES16: behind the residual, below)
                            if constexpr (GRAD16 == 1) v[j] *= gs;
                            if constexpr (GRAD16 == 0 && !RES16) {
                                if (ok[j] && cok) amax = fmaxf(amax, fabsf(v[j]));
                            }
                        }
                        const float got = quad_perm_1032(odd ? v[0] : v[1]);
                        if constexpr (RES16) {
                            // the lane's two channels of pixel pix[odd]: the half residual is read as the pair that is stored, then
                            // the ReLU, the peak (before the saturation) and the store
                            float a0 = odd ? got : v[0], a1 = odd ? v[1] : got;
                            if (ok[odd] && cok) {
                                const size_t o2 = pix[odd] * p.Cout + (ncol[ns] & ~1);
                                const f16x2_ rs = *(const f16x2_ *)((const _Float16 *)p.residual + o2);
                                a0 = a0 + (float)rs[0];
                                a1 = a1 + (float)rs[1];
                                if (relu) { a0 = fmaxf(a0, 0.0f); a1 = fmaxf(a1, 0.0f); }
                                amax = fmaxf(amax, fmaxf(fabsf(a0), fabsf(a1)));
                                const f16x2_ h = {sat_half(a0), sat_half(a1)};
                                *(f16x2_ *)(yh + o2) = h;
                            }
                        } else if constexpr (GRAD16 != 0) {
                            // the lane's two channels of pixel pix[odd]: the half mask is read as the pair that is stored, the peak is
                            // taken after the mask, of what is stored
                            float a0 = odd ? got : v[0], a1 = odd ? v[1] : got;
                            if (ok[odd] && cok) {
                                const size_t o2 = pix[odd] * p.Cout + (ncol[ns] & ~1);
                                if constexpr (EPI_MASK) {
                                    const f16x2_ mk = *(const f16x2_ *)((const _Float16 *)p.residual + o2);
                                    a0 = (float)mk[0] > 0.0f ? a0 : 0.0f;
                                    a1 = (float)mk[1] > 0.0f ? a1 : 0.0f;
                                }
                                amax = fmaxf(amax, fmaxf(fabsf(a0), fabsf(a1)));
                                const f16x2_ h = {sat_half(a0), sat_half(a1)};
                                *(f16x2_ *)(yh + o2) = h;
                            }
                        } else {
                            const f16x2_ h = {sat_half(odd ? got : v[0]), sat_half(odd ? v[1] : got)};
                            if (ok[odd] && cok) *(f16x2_ *)(yh + pix[odd] * p.Cout + (ncol[ns] & ~1)) = h;
                        }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int ms = 0; ms < MR; ++ms) {
        if (stored) break;
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
                        if constexpr (GRAD16 == 1 || GRAD16 == 3) v *= gs;
                        if constexpr (EPI_MASK && MASK16) v = (float)((const _Float16 *)p.residual)[o] > 0.0f ? v : 0.0f;
                        else if constexpr (EPI_MASK) v = p.residual[o] > 0.0f ? v : 0.0f;
                        else if constexpr (RES16) v = v + (float)((const _Float16 *)p.residual)[o];
                        else if (p.residual != nullptr) v = v + p.residual[o];
                        if (relu) v = fmaxf(v, 0.0f);
                        if constexpr (OUT16) {
                            if (nchw) p.y[o] = v;
                            else ((_Float16 *)p.y)[o] = sat_half(v);
                        } else {
                            p.y[o] = v;
                        }
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
                        const size_t o = (((size_t)b * p.Ho + oy) * p.Wo + ox) * p.Cout + ncol[ns];
                        if constexpr (OUT16) ((_Float16 *)p.y)[o] = sat_half(best);
                        else p.y[o] = best;
                        amax = fmaxf(amax, fabsf(best));
                    }
                }
            }
        }
    }
    if (p.amax_out != nullptr) publish_amax(p.amax_out, amax);
