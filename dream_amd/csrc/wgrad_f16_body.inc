// Body of wgrad_f16_kernel / wgrad_f16_x16_kernel (wgrad_f16.hip), included once per kernel so that the fp32-x kernel keeps the machine
// code that was measured (as conv_f16_body.inc).  In scope: the argument p and X16 (bool constant: x lives in HBM as IEEE half --
// train_activation_storage="fp16"; p.x points to halfs, and the stored half IS the operand: a lane copies its four channels (8 bytes) of
// each of the 10 positions, no convert, no multiply, ex = 0, amax_x is not read) and DY16 (bool constant, with X16: dy lives in HBM as
// IEEE half times 2^e_g -- train_gradient_storage="fp16"; p.dy points to halfs that are copied the same way, amax_dy is not read).
    DREAM_DYNAMIC_LDS(_Float16, smem);
    _Float16 *sY = smem;                  // [RW][SY]
    _Float16 *sX = smem + RW * SY;        // [3][CW][SX]
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_index();
    const int wo = wave >> 1, wi = wave & 1;
    const int li = lane & 31, lh = lane >> 5;
    // XCD-aware placement as in wgrad.hip: the (row block, column block) tiles of one split-K slice share an XCD's L2
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int nblk = p.nrb * p.ncb;
    const int blk = slot % nblk, ks = (slot / nblk) * 8 + xcd;
    if (ks >= p.splitk) return;
    const int rbk = blk % p.nrb, cbk = blk / p.nrb;
    const int co0 = rbk * RW, ci0 = cbk * CW;
    float sx = 1.0f;                                 // (X16: the stored half is the operand, amax_x is not read)
    if constexpr (!X16) sx = pow2f(scale_exponent(*p.amax_x));
    float sg = 1.0f;                                 // (DY16: the stored half is the operand, amax_dy is not read)
    if constexpr (!DY16) sg = pow2f(scale_exponent(*p.amax_dy));

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    f32x4 bsum = {0.0f, 0.0f, 0.0f, 0.0f};           // this thread's share of the channel sums of the unrounded dy
    const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};

    const int q = tid & 15;                          // channel quad of the staging
    const int grp = tid >> 4;                        // dy staging: the 8 positions (ty = grp >> 1, tx = 8 * (grp & 1) ..)
    const bool y_chan_ok = co0 + q * 4 < p.Ct;       // channel counts are multiples of 4
    const bool x_chan_ok = ci0 + q * 4 < p.Cin;

    for (int tile = ks; tile < p.tiles_total; tile += p.splitk) {
        int t = tile;
        const int tix = t % p.tiles_x;
        t /= p.tiles_x;
        const int tiy = t % p.tiles_y;
        const int b = t / p.tiles_y;
        const int y0 = tiy * TH, x0 = tix * TW;
        const float *xb = p.x + (size_t)b * p.H * p.W * p.Cin + ci0 + q * 4;
        const _Float16 *xh = (const _Float16 *)p.x + (size_t)b * p.H * p.W * p.Cin + ci0 + q * 4;      // (X16)
        const float *gb = p.dy + (size_t)b * p.H * p.W * p.Ct + co0 + q * 4;
        const _Float16 *gh = (const _Float16 *)p.dy + (size_t)b * p.H * p.W * p.Ct + co0 + q * 4;     // (DY16)

        __syncthreads();                             // previous tile fully consumed
        // ---- dy: 8 consecutive positions x 4 channels per thread (loads from clamped, always-legal addresses + a select) -----------
        if constexpr (DY16) {
            // a copy: the producer rounded; the bias sums the stored halfs in fp32, in the order of the fp32 form
            const int oy = y0 + (grp >> 1), ox0 = x0 + (grp & 1) * 8;
            const f16x4 zero4h = {0, 0, 0, 0};
            f16x4 v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool ok = y_chan_ok && oy < p.H && ox0 + j < p.W;
                v[j] = *(const f16x4 *)(ok ? gh + ((size_t)oy * p.W + ox0 + j) * p.Ct : (const _Float16 *)p.dy);
                v[j] = ok ? v[j] : zero4h;
#pragma unroll
                for (int c = 0; c < 4; ++c) bsum[c] += (float)v[j][c];
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                f16x8 h;
#pragma unroll
                for (int j = 0; j < 8; ++j) h[j] = v[j][c];
                *(f16x8 *)(sY + (q * 4 + c) * SY + grp * 8) = h;
            }
        } else {
            const int oy = y0 + (grp >> 1), ox0 = x0 + (grp & 1) * 8;
            f32x4 v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool ok = y_chan_ok && oy < p.H && ox0 + j < p.W;
                v[j] = *(const f32x4 *)(ok ? gb + ((size_t)oy * p.W + ox0 + j) * p.Ct : p.dy);
                v[j] = ok ? v[j] : zero4;
                bsum += v[j];
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                f16x8 h;
#pragma unroll
                for (int j = 0; j < 8; ++j) h[j] = (_Float16)(v[j][c] * sg);      // the one rounding of dy
                *(f16x8 *)(sY + (q * 4 + c) * SY + grp * 8) = h;
            }
        }
        // ---- x: 10 consecutive positions of a patch row x 4 channels per unit; three shifted copies ----------------------------------
        for (int u = tid >> 4; u < PH * 2; u += 16) {
            const int py = u >> 1, half = u & 1;
            const int gy = y0 - 1 + py, gx0 = x0 - 1 + half * 8;
            f16x4 h[10];
#pragma unroll
            for (int j = 0; j < 10; ++j) {
                const bool ok = x_chan_ok && gy >= 0 && gy < p.H && gx0 + j >= 0 && gx0 + j < p.W;
                if constexpr (X16) {
                    const f16x4 zero4h = {0, 0, 0, 0};
                    const f16x4 v = *(const f16x4 *)(ok ? xh + ((size_t)gy * p.W + gx0 + j) * p.Cin : (const _Float16 *)p.x);
                    h[j] = ok ? v : zero4h;                                           // a copy: the producer rounded
                } else {
                    f32x4 v = *(const f32x4 *)(ok ? xb + ((size_t)gy * p.W + gx0 + j) * p.Cin : p.x);
                    v = ok ? v : zero4;
#pragma unroll
                    for (int c = 0; c < 4; ++c) h[j][c] = (_Float16)(v[c] * sx);      // the one rounding of x
                }
            }
#pragma unroll
            for (int dx = 0; dx < 3; ++dx)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    f16x8 piece;
#pragma unroll
                    for (int j = 0; j < 8; ++j) piece[j] = h[j + dx][c];
                    *(f16x8 *)(sX + (dx * CW + q * 4 + c) * SX + py * TW + half * 8) = piece;
                }
        }
        __syncthreads();

        // ---- k-steps: one tile row (16 positions) each; patch row s + dy serves tap row dy -------------------------------------------
        const _Float16 *aY = sY + (wo * 32 + li) * SY + lh * 8;
        const _Float16 *bX = sX + (wi * 32 + li) * SX + lh * 8;
        f16x8 row[3][3];                             // [patch row % 3][shift]
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) row[r][dx] = *(const f16x8 *)(bX + dx * CW * SX + r * TW);
#pragma unroll
        for (int s = 0; s < TH; ++s) {
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) row[(s + 2) % 3][dx] = *(const f16x8 *)(bX + dx * CW * SX + (s + 2) * TW);
            const f16x8 a = *(const f16x8 *)(aY + s * TW);
#pragma unroll
            for (int ty = 0; ty < 3; ++ty)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) acc[ty * 3 + dx] = mfma_f32_32x32x16_f16(a, row[(s + ty) % 3][dx], acc[ty * 3 + dx]);
        }
    }

    // ---- partials (still in the scaled domain) ------------------------------------------------------------------------------------
#pragma unroll
    for (int tp = 0; tp < 9; ++tp) {
        float *part = p.part + ((size_t)ks * 9 + tp) * p.RowsPad * p.Cin;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = co0 + wo * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            const int i = ci0 + wi * 32 + li;
            if (o < p.RowsPad && i < p.Cin) part[(size_t)o * p.Cin + i] = acc[tp][r];
        }
    }
    if (cbk == 0 && p.bias_part != nullptr) {
        // threads sharing q (the same 4 channels) differ in grp: reduce the 16 groups through LDS, in group order
        float *red = (float *)smem;
        __syncthreads();
        *(f32x4 *)(red + (grp * 16 + q) * 4) = bsum;
        __syncthreads();
        if (tid < RW) {
            float s = 0.0f;
#pragma unroll
            for (int g = 0; g < 16; ++g) s += red[(g * 16 + (tid >> 2)) * 4 + (tid & 3)];
            if (co0 + tid < p.RowsPad) p.bias_part[(size_t)ks * p.RowsPad + co0 + tid] = s;
        }
    }
