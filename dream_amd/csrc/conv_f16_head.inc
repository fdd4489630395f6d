// Epilogue of convT4_head_f16_kernel (conv_head_f16.hip; inference_head_fusion="on", DESIGN.md 4.8m), included by conv_f16_body.inc in
// place of conv_f16_epilogue.inc: the 1x1 head conv contracted inside the launch of the last decoder stage.  In scope: what the
// epilogue sees (p, acc[MR][NR], inv, wm, wn, li, lh, b, y0, x0, TW, smem, tid, wave; ACT16) and h, the head's Head16Params.  The
// workgroup owns all BN == p.Cout == 256 stage channels of its BM pixels (blockIdx.y == 0).
//   1. the act16 epilogue, element for element: v = acc * (inv * scale) + shift, ReLU, max|v| of the pixels inside the image into the
//      peak scalar, sat_half -- stored not to HBM but into sT [BM][BN + 8] halfs, which aliases the loop's LDS (every wave has passed
//      the loop's last barrier).  The lane pair exchange of the act16 store makes these 4-byte LDS writes;
//   2. rows 0 .. K-1 of the head's packed plane [32][256] into sH [K][BN + 8], once per workgroup (its loads are issued before step 1).
//      The MFMA's B operand has 32 columns: lanes of a column >= K read row K-1 again, and what they compute is never stored -- so the
//      LDS request is (BM + K) rows, and two workgroups fit a CU up to K = 27;
//   3. wavefront i < BM / 32 contracts pixels 32 i .. 32 i + 31 with the plane: ONE accumulator from zero, 16 MFMAs in ascending k --
//      the sequence the unfused head (dream_conv2d_f16_nhwc_f16, DREAM_CONV_OUT_NCHW) runs, pixels the A operand there as here -- then
//      its affine, acc2 * 2^-ew_head + bias.  No ReLU, no peak;
//   4. the [32 channels][32 pixels] fp32 block goes through LDS (16-byte writes; the staging rows are dead behind a barrier), so that a
//      store instruction writes 64 consecutive tile pixels of ONE plane of the NCHW maps: at the phase's stride of 2 in x half-used
//      lines, not the lane-per-plane 4 scattered bytes of the unfused head.
// Rows of the staging buffer outside the tile or the image hold values nothing reads back: a row of A reaches its own row of D only.
    {
        constexpr int BM = 32 * MR * WM;
        constexpr int ST = BN + 8;                      // staging row stride in halfs: 528 B, an odd number of 16-byte slots
        constexpr int KP = 32;                          // the head's padded channels: one MFMA column block
        constexpr int SO = 36;                          // row stride in floats of a [KP][32 px] result block (144 B: 9 slots)
        constexpr int NH_IT = KP * (BN / 8) / NT;       // 16-byte pieces of the head's plane per thread
        static_assert(BN == 256 && BM / 32 <= WM * WN && KP * (BN / 8) % NT == 0 && NT % BM == 0, "the fused head's tile");
        static_assert((BM / 32) * KP * SO * sizeof(float) <= BM * ST * sizeof(_Float16), "result blocks inside the staging buffer");
        typedef _Float16 f16x2_ __attribute__((ext_vector_type(2)));
        _Float16 *sT = smem;                            // [BM][ST]
        _Float16 *sH = sT + BM * ST;                    // [h.K][ST]

        f16x8 h_reg[NH_IT];
#pragma unroll
        for (int it = 0; it < NH_IT; ++it) {
            const int idx = tid + it * NT, n = idx / (BN / 8);
            if (n < h.K) h_reg[it] = *(const f16x8 *)(h.w + n * BN + (idx % (BN / 8)) * 8);
        }

        const bool relu = (p.flags & DREAM_CONV_RELU) != 0;
        float scale_v[NR], shift_v[NR];
        int ncol[NR];
#pragma unroll
        for (int ns = 0; ns < NR; ++ns) {
            ncol[ns] = (wn * NR + ns) * 32 + li;
            scale_v[ns] = inv * (p.scale != nullptr ? p.scale[ncol[ns]] : 1.0f);
            shift_v[ns] = p.shift != nullptr ? p.shift[ncol[ns]] : 0.0f;
        }
        const int npix = p.TH * TW;
        float amax = 0.0f;
        const int odd = li & 1;
#pragma unroll
        for (int ms = 0; ms < MR; ++ms) {
#pragma unroll
            for (int r2 = 0; r2 < 8; ++r2) {             // registers 2 r2, 2 r2 + 1: two tile rows
                bool ok[2];
                int mrow[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int r = 2 * r2 + j;
                    const int m = (wm * MR + ms) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    const int ty = (m * p.rcpTW) >> 16, tx = m - ty * TW;
                    ok[j] = (m < npix) && (y0 + ty < p.H) && (x0 + tx < p.W);
                    mrow[j] = m;
                }
#pragma unroll
                for (int ns = 0; ns < NR; ++ns) {
                    float v[2];
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        v[j] = acc[ms][ns][2 * r2 + j] * scale_v[ns] + shift_v[ns];
                        if (relu) v[j] = fmaxf(v[j], 0.0f);
                        if (ok[j]) amax = fmaxf(amax, fabsf(v[j]));
                    }
                    // the even lane keeps channels 2j, 2j + 1 of the first row, the odd lane those of the second
                    const float got = quad_perm_1032(odd ? v[0] : v[1]);
                    const f16x2_ h2 = {sat_half(odd ? got : v[0]), sat_half(odd ? v[1] : got)};
                    *(f16x2_ *)(sT + mrow[odd] * ST + (ncol[ns] & ~1)) = h2;
                }
            }
        }
#pragma unroll
        for (int it = 0; it < NH_IT; ++it) {
            const int idx = tid + it * NT, n = idx / (BN / 8);
            if (n < h.K) *(f16x8 *)(sH + n * ST + (idx % (BN / 8)) * 8) = h_reg[it];
        }
        __syncthreads();

        f32x16 acc2;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc2[r] = 0.0f;
        if (wave < BM / 32) {
            const _Float16 *pa = sT + (wave * 32 + li) * ST + lh * 8;
            const _Float16 *pb = sH + (li < h.K ? li : h.K - 1) * ST + lh * 8;
#pragma unroll
            for (int kk = 0; kk < BN; kk += 16) acc2 = mfma_f32_32x32x16_f16(*(const f16x8 *)(pa + kk), *(const f16x8 *)(pb + kk), acc2);
        }
        __syncthreads();                                // every fragment of sT is in registers: its rows may take the result blocks
        float *sO = (float *)smem;                      // [BM / 32][KP][SO]
        if (wave < BM / 32) {
            const int he = -*h.w_exp;
            const float inv_h = pow2f(he < -126 ? -126 : (he > 127 ? 127 : he));
            const float bias_v = (h.bias != nullptr && li < h.K) ? h.bias[li] : 0.0f;
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {            // registers 4 r4 .. 4 r4 + 3: pixels 8 r4 + 4 lh .. + 3 of the block
                f32x4 o;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = acc2[4 * r4 + j] * inv_h + bias_v;
                *(f32x4 *)(sO + (wave * KP + li) * SO + 8 * r4 + 4 * lh) = o;
            }
        }
        __syncthreads();

        // a thread owns one tile pixel and every (NT / BM)-th plane
        const int m = tid % BM;
        const int ty = (m * p.rcpTW) >> 16, tx = m - ty * TW;
        if ((m < npix) && (y0 + ty < p.H) && (x0 + tx < p.W)) {
            const int oy = (y0 + ty) * p.out_scale + p.out_oy, ox = (x0 + tx) * p.out_scale + p.out_ox;
            const size_t plane = (size_t)p.Ho * p.Wo;
            float *dst = h.maps + (size_t)b * h.K * plane + (size_t)oy * p.Wo + ox;
            const float *src = sO + (m >> 5) * KP * SO + (m & 31);
            for (int k = tid / BM; k < h.K; k += NT / BM) dst[(size_t)k * plane] = src[k * SO];
        }
        if (p.amax_out != nullptr) publish_amax(p.amax_out, amax);
    }
