// Body of the ConvTranspose2d(k4,s2,p1) weight-gradient kernels of wgrad_f16.hip (included once per kernel, so that each keeps its own
// machine code).  The including kernel defines
//   constexpr bool XS   x is staged as half(x * 2^e_x), e_x = scale_exponent(*amax_x) (the rounding of a forward that scales by the
//                       tensor's amax: no clamp); false: half(clamp(x, +-65504)), e_x = 0 (a ReLU'd BatchNorm output)
// and has the parameter ``const WgradT4Params p`` and a ``const unsigned *amax_x`` in scope (read only with XS).
    DREAM_DYNAMIC_LDS(_Float16, smem);
    _Float16 *sY = smem;                  // [RW][SY]      x, transposed: [ci][position]
    _Float16 *sX = smem + RW * SY;        // [2][CW][SXT]  the phase's dz patch, transposed, shifted by dx = 0 | 1
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_index();
    const int wo = wave >> 1, wi = wave & 1;
    const int li = lane & 31, lh = lane >> 5;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int nblk = p.nrb * p.ncb * 4;
    const int blk = slot % nblk, ks = (slot / nblk) * 8 + xcd;
    if (ks >= p.splitk) return;
    const int ph = blk & 3, pa = ph >> 1, pb = ph & 1;
    const int rbk = (blk >> 2) % p.nrb, cbk = (blk >> 2) / p.nrb;
    const int ci0 = rbk * RW, co0 = cbk * CW;
    const float sg = pow2f(scale_exponent(*p.amax_dz));
    const float sx = XS ? pow2f(scale_exponent(*amax_x)) : 1.0f;

    f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};

    const int q = tid & 15;                          // channel quad of the staging
    const int grp = tid >> 4;                        // x staging: the 8 positions (ty = grp >> 1, tx = 8 * (grp & 1) ..)
    const bool x_chan_ok = ci0 + q * 4 < p.Cin;      // channel counts are multiples of 4
    const bool g_chan_ok = co0 + q * 4 < p.Cdz;
    const int Ho = 2 * p.H, Wo = 2 * p.W;

    for (int tile = ks; tile < p.tiles_total; tile += p.splitk) {
        int t = tile;
        const int tix = t % p.tiles_x;
        t /= p.tiles_x;
        const int tiy = t % p.tiles_y;
        const int b = t / p.tiles_y;
        const int y0 = tiy * TH, x0 = tix * TW;
        const float *xb = p.x + (size_t)b * p.H * p.W * p.Cin + ci0 + q * 4;
        const float *gb = p.dz + (size_t)b * Ho * Wo * p.Cdz + co0 + q * 4;

        __syncthreads();                             // previous tile fully consumed
        // ---- x: 8 consecutive positions x 4 channels per thread (loads from clamped, always-legal addresses + a select) --------------
        {
            const int oy = y0 + (grp >> 1), ox0 = x0 + (grp & 1) * 8;
            f32x4 v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool ok = x_chan_ok && oy < p.H && ox0 + j < p.W;
                v[j] = *(const f32x4 *)(ok ? xb + ((size_t)oy * p.W + ox0 + j) * p.Cin : p.x);
                v[j] = ok ? v[j] : zero4;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                f16x8 h;
#pragma unroll
                for (int j = 0; j < 8; ++j)                  // the one rounding of x
                    h[j] = XS ? (_Float16)(v[j][c] * sx) : (_Float16)fminf(fmaxf(v[j][c], -65504.0f), 65504.0f);
                *(f16x8 *)(sY + (q * 4 + c) * SY + grp * 8) = h;
            }
        }
        // ---- dz: 9 positions of a patch row of the phase (position stride 2) x 4 channels per unit; two shifted copies ---------------
        for (int u = tid >> 4; u < TPH * 2; u += 16) {
            const int py = u >> 1, half = u & 1;
            const int gu = y0 - pa + py, gv0 = x0 - pb + half * 8;
            f16x4 h[9];
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                const bool ok = g_chan_ok && gu >= 0 && gu < p.H && gv0 + j >= 0 && gv0 + j < p.W;
                f32x4 v = *(const f32x4 *)(ok ? gb + ((size_t)(2 * gu + pa) * Wo + 2 * (gv0 + j) + pb) * p.Cdz : p.dz);
                v = ok ? v : zero4;
#pragma unroll
                for (int c = 0; c < 4; ++c) h[j][c] = (_Float16)(v[c] * sg);      // the one rounding of dz
            }
#pragma unroll
            for (int dx = 0; dx < 2; ++dx)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    f16x8 piece;
#pragma unroll
                    for (int j = 0; j < 8; ++j) piece[j] = h[j + dx][c];
                    *(f16x8 *)(sX + (dx * CW + q * 4 + c) * SXT + py * TW + half * 8) = piece;
                }
        }
        __syncthreads();

        // ---- k-steps: one tile row (16 positions) each; patch row s + dy serves tap row dy -------------------------------------------
        const _Float16 *aY = sY + (wo * 32 + li) * SY + lh * 8;
        const _Float16 *bX = sX + (wi * 32 + li) * SXT + lh * 8;
        f16x8 row[2][2];                             // [patch row % 2][shift]
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) row[0][dx] = *(const f16x8 *)(bX + dx * CW * SXT);
#pragma unroll
        for (int s = 0; s < TH; ++s) {
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) row[(s + 1) % 2][dx] = *(const f16x8 *)(bX + dx * CW * SXT + (s + 1) * TW);
            const f16x8 a = *(const f16x8 *)(aY + s * TW);
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) acc[dy * 2 + dx] = mfma_f32_32x32x16_f16(a, row[(s + dy) % 2][dx], acc[dy * 2 + dx]);
        }
    }

    // ---- partials (still in the scaled domain): tap (dy, dx) of this phase is slice 4 (2 dy + 1 - a) + 2 dx + 1 - b ---------------------
#pragma unroll
    for (int tp = 0; tp < 4; ++tp) {
        const int slice = 4 * (2 * (tp >> 1) + 1 - pa) + 2 * (tp & 1) + 1 - pb;
        float *part = p.part + ((size_t)ks * 16 + slice) * p.RowsPad * p.Cdz;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = ci0 + wo * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            const int i = co0 + wi * 32 + li;
            if (o < p.RowsPad && i < p.Cdz) part[(size_t)o * p.Cdz + i] = acc[tp][r];
        }
    }
