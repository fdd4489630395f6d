// Body of conv3x3_first_kernel / conv3x3_first_f16_kernel (conv_first.hip), included once per kernel so that the fp32 kernel keeps the
// machine code that was measured.  In scope: the template parameter CIN, the argument p, and OUT16 (bool constant: y is IEEE half
// NHWC -- the same fp32 arithmetic, saturated and rounded at the store; max|y| is taken before the saturation).
    DREAM_DYNAMIC_LDS(float, smem);     // 2 x [CIN][FPH][FPW]
    constexpr int NPATCH = CIN * FPLANE;
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_index();
    const int cq = lane & 15, lg = lane >> 4;               // channel quad of the 64-channel block, pixel quad of the 16-pixel row
    const int cout = blockIdx.y * 64 + 4 * cq;
    int t = blockIdx.x;
    if (t >= p.ntiles) return;

    // this lane's filters: w[cout + j][c][ky][kx] (OIHW as stored by torch), tap-major, the four channels side by side
    // (plain floats, not float4s: a register tuple per tap made the compiler copy the loaded weights into place, both sets live)
    float wq[CIN * 9][4];
#pragma unroll
    for (int i = 0; i < CIN * 9; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) wq[i][j] = p.w[(size_t)(cout + j) * (CIN * 9) + i];
    f32x4 bv = {0.0f, 0.0f, 0.0f, 0.0f};
    if (p.bias)
#pragma unroll
        for (int j = 0; j < 4; ++j) bv[j] = p.bias[cout + j];

    // staging: threads 0 .. 239 are a 12-row x 20-column window that steps down the patch's CIN x 18 rows: thread (ry, px) takes
    // the elements 240 k + tid -- row ry + 12 k, always column px.  One division by a constant per thread and tile (recomputed: the
    // kernel has no registers to keep (ry, px) in); the channel of a row comes from a compare (twelve consecutive rows cross at
    // most one channel boundary).
    constexpr int SROWS = 12, SN = SROWS * FPW, NSTG = (CIN * FPH + SROWS - 1) / SROWS;
    struct Tile { int b, y0, x0; };
    auto decode = [&](int tt) {
        const int tix = tt % p.tiles_x;
        tt /= p.tiles_x;
        const int tiy = tt % p.tiles_y;
        return Tile{tt / p.tiles_y, tiy * FT, tix * FT};
    };
    // coalesced along x inside each NCHW plane; buffer loads: an element outside the image carries an out-of-range offset and
    // comes back as zero -- no branch, no 64-bit address per element
    auto stage_load = [&](const Tile &tl, float (&v)[NSTG]) {
        const BufferRsrc img = make_buffer(p.x + (size_t)tl.b * CIN * p.H * p.W, (size_t)CIN * p.H * p.W * sizeof(float));
        int ti = tid;
        asm volatile("" : "+v"(ti));
        const int ry = ti / FPW, px = ti - ry * FPW;
        const int gx = (ti < SN && px < FT + 2) ? tl.x0 - 1 + px : -1;                // pad columns, idle threads: never inside the image
        const bool xok = (unsigned)gx < (unsigned)p.W;
#pragma unroll
        for (int k = 0; k < NSTG; ++k) {
            const int R = ry + SROWS * k, c0 = (SROWS * k) / FPH;
            const int c = c0 + (R >= FPH * (c0 + 1) ? 1 : 0), gy = tl.y0 - 1 + R - FPH * c;
            const bool ok = xok && R < CIN * FPH && (unsigned)gy < (unsigned)p.H;
            v[k] = buffer_load_f32(img, ok ? (unsigned)((c * p.H + gy) * p.W + gx) * 4u : BUFFER_OOB, 0u);
        }
    };
    auto stage_write = [&](float *buf, const float (&v)[NSTG]) {
#pragma unroll
        for (int k = 0; k < NSTG; ++k)
            if (tid < SN && tid + SN * k < NPATCH) buf[tid + SN * k] = v[k];
    };

    float amax = 0.0f;
    // byte offsets inside a row of the tile (OUT16: 2-byte elements, and the offset of the lane PAIR's eight channels)
    const unsigned px_b = (unsigned)p.Cout * (OUT16 ? 2u : 4u);
    const unsigned voff = (unsigned)(4 * lg) * px_b + (OUT16 ? (unsigned)(cout & ~7) * 2u : (unsigned)cout * 4u);
    // wave w owns rows 4w .. 4w + 3 of the tile; lane (lg, cq): pixels 4 lg .. 4 lg + 3 of the row, channels 4 cq .. 4 cq + 3
    auto compute = [&](const Tile &tl, const float *buf) {
#pragma unroll 1
        for (int r = 0; r < 4; ++r) {
            const int row = wave * 4 + r, oy = tl.y0 + row;
            if (oy >= p.H) break;                                               // wave-uniform
            f32x4 acc[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = bv;
            // input row (row + ky) of channel c, pixels 4 lg .. 4 lg + 5 of the patch; group g = 3 c + ky is read while group
            // g - 1 is multiplied (the fences keep the compiler from fetching all 9 CIN groups up front: registers)
            const float *src = buf + row * FPW + 4 * lg;
            f32x4 q0 = *(const f32x4 *)src;
            f32x2 q1 = *(const f32x2 *)(src + 4);
#pragma unroll
            for (int g = 0; g < CIN * 3; ++g) {
                const float v[6] = {q0[0], q0[1], q0[2], q0[3], q1[0], q1[1]};
                if (g + 1 < CIN * 3) {
                    const float *nsrc = src + ((g + 1) / 3) * FPLANE + ((g + 1) % 3) * FPW;
                    q0 = *(const f32x4 *)nsrc;
                    q1 = *(const f32x2 *)(nsrc + 4);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_fmaf(v[i + kx], wq[g * 3 + kx][j], acc[i][j]);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (p.relu) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = fmaxf(acc[i][j], 0.0f);
            }
            // the row's 16 pixels as one buffer that ends with the image row: pixels past it are dropped by the bounds check
            const int npx = p.W - tl.x0 < FT ? p.W - tl.x0 : FT;
            const BufferRsrc yrow = OUT16
                ? make_buffer((const _Float16 *)p.y + (((size_t)tl.b * p.H + oy) * p.W + tl.x0) * p.Cout, (size_t)npx * p.Cout * sizeof(_Float16))
                : make_buffer(p.y + (((size_t)tl.b * p.H + oy) * p.W + tl.x0) * p.Cout, (size_t)npx * p.Cout * sizeof(float));
            if constexpr (OUT16) {
                // 8 bytes of halfs per pixel and lane: the two lanes of a pair (channel quads 2j, 2j + 1) swap two of their four pixels
                // (DPP) and each stores TWO pixels' eight channels as dwordx4 -- half the store instructions of the fp32 form, 16 bytes each
                f32x2 hp[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const f16x4 h = {sat_half(acc[i][0]), sat_half(acc[i][1]), sat_half(acc[i][2]), sat_half(acc[i][3])};
                    hp[i] = __builtin_bit_cast(f32x2, h);
                }
                const bool odd = (cq & 1) != 0;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    // the even lane keeps pixels 0 and 2 and sends 1 and 3; the odd lane the other way round
                    const f32x2 mine = odd ? hp[2 * j + 1] : hp[2 * j], send = odd ? hp[2 * j] : hp[2 * j + 1];
                    const f32x2 got = {quad_perm_1032(send[0]), quad_perm_1032(send[1])};
                    const f32x4 v = odd ? f32x4{got[0], got[1], mine[0], mine[1]} : f32x4{mine[0], mine[1], got[0], got[1]};
                    buffer_store_x4(yrow, v, voff + (unsigned)(2 * j + (odd ? 1 : 0)) * px_b, 0u);
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) buffer_store_x4(yrow, acc[i], voff + (unsigned)i * px_b, 0u);
            }
            if (p.amax_out != nullptr) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float m = fmaxf(fmaxf(fabsf(acc[i][0]), fabsf(acc[i][1])), fmaxf(fabsf(acc[i][2]), fabsf(acc[i][3])));
                    amax = fmaxf(amax, 4 * lg + i < npx ? m : 0.0f);
                }
            }
        }
    };

    Tile cur = decode(t);
    float sv[NSTG];
    stage_load(cur, sv);
    stage_write(smem, sv);
    __syncthreads();
    int ib = 0;
    while (true) {
        const int tn = t + (int)gridDim.x;
        const bool more = tn < p.ntiles;                                        // workgroup-uniform
        const Tile nxt = decode(more ? tn : t);
        if (more) stage_load(nxt, sv);
        compute(cur, smem + ib * NPATCH);
        if (!more) break;
        // the other buffer was last read before the previous barrier: one barrier per tile
        ib ^= 1;
        stage_write(smem + ib * NPATCH, sv);
        __syncthreads();
        t = tn;
        cur = nxt;
    }
    if (p.amax_out != nullptr) publish_amax(p.amax_out, amax);
