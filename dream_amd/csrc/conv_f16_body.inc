// Body of conv_f16_kernel<FORM, ...> (conv_f16.hip; the forms and their constants: the kForms table there), a kernel of its own per form
// so that each keeps the machine code that was measured (as conv_wino_body.inc).  In scope: the template parameters MR, NR, WM, WN, NPM, DB, PRIO, the argument p, and
// EPI_MASK (bool constant: the DREAM_CONV_RELUMASK epilogue) and ACT16 (bool constant: activations live in HBM as IEEE half --
// p.x and an NHWC p.y point to halfs; the patch is copied, not converted: 16-byte pieces of 8 halfs, no input scale) and MASK16
// (bool constant, read by the epilogue: the ReLU mask of EPI_MASK is a tensor of IEEE halfs) and KSPLIT (bool constant, with ACT16:
// slice blockIdx.z of the gridDim.z slices of the contraction -- a contiguous range of the (channel chunk, tap) stages, the leftover
// spread over the first slices -- whose raw fp32 accumulators go to p.y = workspace[slice] in NHWC fp32: no scale, no shift, no ReLU,
// no peak; conv_f16_ksplit_finish_kernel sums the slices and runs the epilogue) and GRAD16 (int constant, read by the epilogue: the
// entry / interior / exit form of a half-stored data gradient, 0 otherwise; the loader follows ACT16 as ever) and RES16 (bool constant,
// read by the epilogue: `residual` is a tensor of IEEE halfs) and DGT4 (bool constant: the data gradient of ConvTranspose2d(k4,s2,p1) -- p.x is
// dz [B, 2 p.H, 2 p.W, Cin]; the contraction runs over (32-channel chunk, sub-pixel phase (a, b) of dz, tap): a "chunk" of the loop below is
// one (channel chunk, phase), numbered 4 * chunk + phase, whose patch row py / column px is dz[2 (y0 - a + py) + a][2 (x0 - b + px) + b] --
// zero outside the map -- and whose tap (dy, dx) multiplies weight slice 4 (2 dy + 1 - a) + 2 dx + 1 - b; p.tap_dy / p.tap_dx hold the 2 x 2
// taps, p.tap_w is not read) and SAT0 (bool constant, fp32 x: p.amax_in is not read, e_a = 0, and the rounding saturates to +-65504).
    constexpr int NT = 64 * WM * WN;                // 4 or 8 wavefronts per workgroup
    constexpr int BN = 32 * NR * WN;
    constexpr int QW = ACT16 ? 8 : 4;               // elements of a 16-byte piece
    constexpr int Q = KC / QW;                      // 16-byte pieces per patch row
    constexpr int NA_IT = (NPM * Q + NT - 1) / NT;
    constexpr int NB_PIECES = BN * (KC / 8);        // 16-B pieces of the weight tile per stage
    constexpr int NB_IT = (NB_PIECES + NT - 1) / NT;
    static_assert(WM * WN == 4 || WM * WN == 8, "4 or 8 wavefronts per workgroup");

    DREAM_DYNAMIC_LDS(_Float16, smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_index();
    const int wm = wave / WN, wn = wave % WN;
    const int li = lane & 31, lh = lane >> 5;
    const int PW = p.PW, TW = p.TW, NP = p.PH * PW;
    _Float16 *sA = smem;                            // [DB ? 2 : 1][NP][S16]
    _Float16 *sB = sA + (DB ? 2 : 1) * NP * S16;    // [2][BN][S16]

    // XCD-aware placement (see conv_mfma.hip): each XCD works on a contiguous range of tiles so halos meet in its L2
    int t = (int)(blockIdx.x & 7) * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3);
    if (t >= p.B * p.tiles_x * p.tiles_y) return;
    const int tix = t % p.tiles_x;
    t /= p.tiles_x;
    const int tiy = t % p.tiles_y;
    const int b = t / p.tiles_y;
    const int y0 = tiy * p.TH, x0 = tix * TW;
    const int n0 = blockIdx.y * BN;
    const bool zst = (p.flags & DREAM_CONV_ZEROSTUFF2X) != 0;
    const bool ups = (p.flags & DREAM_CONV_UPSAMPLE2X) != 0 || zst;
    const bool pool = (p.flags & DREAM_CONV_POOL2) != 0;
    const float *xb = p.x + (size_t)b * p.Hs * p.Ws * p.Cin;
    const _Float16 *xh = (const _Float16 *)p.x + (size_t)b * p.Hs * p.Ws * p.Cin;     // (ACT16)

    // input scale: max|x| * 2^ea in [2^13, 2^14); stored halfs (ACT16) are the operand as they are: ea = 0, amax_in is not read
    int ea = 0;
    if constexpr (!ACT16 && !SAT0) {             // (SAT0: an operand without an amax, rounded unscaled and saturated below)
        const unsigned abits = *p.amax_in;
        const int aexp = (int)((abits >> 23) & 255) - 127;
        ea = (abits == 0u) ? 0 : 13 - aexp;
        ea = ea < -100 ? -100 : (ea > 100 ? 100 : ea);
    }
    const float sa = pow2f(ea);
    const float inv = pow2f(-(ea + *p.w_exp) < -126 ? -126 : (-(ea + *p.w_exp) > 127 ? 127 : -(ea + *p.w_exp)));

    int a_goff[NA_IT], a_soff[NA_IT];
    int a_pyx[DGT4 ? NA_IT : 1];                     // (DGT4) patch row << 16 | patch column: the address follows the phase
#pragma unroll
    for (int it = 0; it < NA_IT; ++it) {
        const int idx = tid + it * NT;
        const int pp = idx / Q, q = idx % Q;
        a_soff[it] = (pp < NP) ? pp * S16 + q * QW : -1;
        const int py = pp / PW, px = pp - py * PW;
        if constexpr (DGT4) {
            a_goff[it] = q * QW;
            a_pyx[it] = (py << 16) | px;
            continue;
        }
        const int gy = y0 * p.in_scale - p.pad_y + py * p.in_step, gx = x0 * p.in_scale - p.pad_x + px * p.in_step;
        const bool inb = (pp < NP) && gy >= 0 && gy < p.Hin && gx >= 0 && gx < p.Win && !(zst && ((gy | gx) & 1));
        const int sy = ups ? (gy >> 1) : gy, sx = ups ? (gx >> 1) : gx;
        a_goff[it] = inb ? (sy * p.Ws + sx) * p.Cin + q * QW : -1;
    }
    int b_goff[NB_IT], b_soff[NB_IT];
#pragma unroll
    for (int it = 0; it < NB_IT; ++it) {
        const int idx = tid + it * NT;
        const int n = idx / (KC / 8), q = idx % (KC / 8);
        b_soff[it] = (idx < NB_PIECES) ? n * S16 + q * 8 : -1;
        b_goff[it] = (n0 + n) * p.Cin + q * 8;
    }
    const size_t w_tap_stride = (size_t)p.CoutPad * p.Cin;

    int a_frag[MR], b_frag[NR];
#pragma unroll
    for (int ms = 0; ms < MR; ++ms) {
        int m = (wm * MR + ms) * 32 + li;
        if (m >= p.TH * TW) m = 0;
        int ty, tx;
        tile_xy(m, TW, p.rcpTW, pool, &ty, &tx);
        a_frag[ms] = (ty * PW + tx) * p.lane_stride * S16 + lh * 8;
    }
#pragma unroll
    for (int ns = 0; ns < NR; ++ns) b_frag[ns] = ((wn * NR + ns) * 32 + li) * S16 + lh * 8;

    f32x16 acc[MR][NR];
#pragma unroll
    for (int ms = 0; ms < MR; ++ms)
#pragma unroll
        for (int ns = 0; ns < NR; ++ns)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ms][ns][r] = 0.0f;

    f32x4 a_reg[ACT16 ? 1 : NA_IT];
    f16x8 a_reg16[ACT16 ? NA_IT : 1];
    f16x8 b_reg[NB_IT];
    const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};

    auto load_a = [&](int c0) {
        if constexpr (DGT4) {
            // c0 = KC * (4 * channel chunk + phase): the phase's patch, gathered with position stride 2 (32 contiguous channels a position)
            const int sc = c0 / KC, pa = (sc >> 1) & 1, pb = sc & 1, cc = (sc >> 2) * KC;
#pragma unroll
            for (int it = 0; it < NA_IT; ++it) {
                const int u = y0 - pa + (a_pyx[it] >> 16), v = x0 - pb + (a_pyx[it] & 0xffff);
                const bool inb = a_soff[it] >= 0 && u >= 0 && u < p.H && v >= 0 && v < p.W;
                a_reg[it] = inb ? *(const f32x4 *)(xb + ((2 * u + pa) * p.Ws + 2 * v + pb) * p.Cin + a_goff[it] + cc) : zero4;
            }
        } else if constexpr (ACT16) {
            const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int it = 0; it < NA_IT; ++it)
                a_reg16[it] = (a_goff[it] >= 0) ? *(const f16x8 *)(xh + a_goff[it] + c0) : zero8;
        } else {
#pragma unroll
            for (int it = 0; it < NA_IT; ++it)
                a_reg[it] = (a_goff[it] >= 0) ? *(const f32x4 *)(xb + a_goff[it] + c0) : zero4;
        }
    };
    auto store_a = [&](int abuf) {     // the one rounding of the activations: fp16(v * 2^ea), to nearest even (ACT16: none, a copy)
        _Float16 *d = sA + abuf * NP * S16;
        if constexpr (ACT16) {
#pragma unroll
            for (int it = 0; it < NA_IT; ++it)
                if (a_soff[it] >= 0) *(f16x8 *)(d + a_soff[it]) = a_reg16[it];
        } else {
#pragma unroll
            for (int it = 0; it < NA_IT; ++it) {
                if (a_soff[it] >= 0) {
                    f16x4 h;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if constexpr (SAT0) h[k] = (_Float16)fminf(fmaxf(a_reg[it][k], -65504.0f), 65504.0f);
                        else h[k] = (_Float16)(a_reg[it][k] * sa);
                    }
                    *(f16x4 *)(d + a_soff[it]) = h;
                }
            }
        }
    };
    auto load_b = [&](int tap, int c0) {
        size_t base;
        if constexpr (DGT4) {
            const int sc = c0 / KC, pa = (sc >> 1) & 1, pb = sc & 1;
            base = (size_t)(4 * (2 * (tap >> 1) + 1 - pa) + 2 * (tap & 1) + 1 - pb) * w_tap_stride + (sc >> 2) * KC;
        } else {
            base = (size_t)((p.tap_w >> (4 * tap)) & 15) * w_tap_stride + c0;
        }
#pragma unroll
        for (int it = 0; it < NB_IT; ++it)
            if (b_soff[it] >= 0) b_reg[it] = *(const f16x8 *)(p.w_hi + base + b_goff[it]);
    };
    auto store_b = [&](int buf) {
        _Float16 *d = sB + buf * BN * S16;
#pragma unroll
        for (int it = 0; it < NB_IT; ++it)
            if (b_soff[it] >= 0) *(f16x8 *)(d + b_soff[it]) = b_reg[it];
    };

    const int nchunks = DGT4 ? 4 * (p.Cin / KC) : p.Cin / KC;
    // KSPLIT: this workgroup runs the stages [ks_first, ks_end) of the launch's nchunks * ntaps
    int ks_first = 0, ks_end = 0;
    if constexpr (KSPLIT) {
        const int all = nchunks * p.ntaps, S = (int)gridDim.z, s = (int)blockIdx.z, per = all / S, rem = all % S;
        ks_first = s * per + (s < rem ? s : rem);
        ks_end = ks_first + per + (s < rem ? 1 : 0);
        if (ks_first >= ks_end) ks_first = ks_end = 0;   // an empty slice (a caller's S beyond the stages) stores its zeros: no stage, valid loads
    }
    load_a(KSPLIT ? ks_first / p.ntaps * KC : 0);
    load_b(KSPLIT ? ks_first % p.ntaps : 0, KSPLIT ? ks_first / p.ntaps * KC : 0);
    store_a(0);
    store_b(0);
    __syncthreads();

    int buf = 0, abuf = 0, tap = KSPLIT ? ks_first % p.ntaps : 0, chunk = KSPLIT ? ks_first / p.ntaps : 0;
    const int ntaps = p.ntaps, nstages = KSPLIT ? ks_end : nchunks * ntaps;
    for (int st = KSPLIT ? ks_first : 0; st < nstages; ++st) {
        const bool last_tap = (tap == ntaps - 1);
        // (KSPLIT: the next chunk only where the slice reaches it)
        const bool more_chunks = KSPLIT ? ((chunk + 1) * ntaps < nstages) : (chunk + 1 < nchunks);
        const bool have_next = (st + 1 < nstages);
        if (have_next) load_b(last_tap ? 0 : tap + 1, last_tap ? (chunk + 1) * KC : chunk * KC);
        // DB: the next chunk's patch is fetched at the first tap and held in registers until the last; SB: one stage ahead
        // (KSPLIT: a slice that begins inside a chunk fetches at its first stage)
        if ((DB ? (tap == 0 || (KSPLIT && st == ks_first)) : last_tap) && more_chunks) load_a((chunk + 1) * KC);

        const int tdy = (int)((p.tap_dy >> (4 * tap)) & 15), tdx = (int)((p.tap_dx >> (4 * tap)) & 15);
        const _Float16 *pa = sA + abuf * NP * S16 + (tdy * PW + tdx) * S16;
        const _Float16 *pb = sB + buf * BN * S16;
#pragma unroll
        for (int kk = 0; kk < KC; kk += 16) {
            f16x8 a[MR], w[NR];
#pragma unroll
            for (int ms = 0; ms < MR; ++ms) a[ms] = *(const f16x8 *)(pa + a_frag[ms] + kk);
#pragma unroll
            for (int ns = 0; ns < NR; ++ns) w[ns] = *(const f16x8 *)(pb + b_frag[ns] + kk);
            if (PRIO) __builtin_amdgcn_s_setprio(1);     // co-resident waves of the other workgroup are in their load phase
#pragma unroll
            for (int ms = 0; ms < MR; ++ms)
#pragma unroll
                for (int ns = 0; ns < NR; ++ns) acc[ms][ns] = mfma_f32_32x32x16_f16(a[ms], w[ns], acc[ms][ns]);
            if (PRIO) __builtin_amdgcn_s_setprio(0);
        }

        if (have_next) store_b(buf ^ 1);
        if (last_tap && more_chunks) {
            if (DB) {
                // the other patch buffer was last read in the previous chunk: every wave has passed a barrier since
                store_a(abuf ^ 1);
                abuf ^= 1;
            } else {
                __syncthreads();
                store_a(0);
            }
        }
        __syncthreads();
        buf ^= 1;
        if (last_tap) { tap = 0; ++chunk; } else ++tap;
    }

    if constexpr (KSPLIT) {
        // the raw accumulators of this slice, every element of the tile inside the image (a lane owns one channel: 128 bytes per
        // half-wave and pixel); slices lie round_up(B H W Cout, 8) floats apart (conv_f16_ksplit_finish_kernel reads 32-byte pieces)
        const size_t slice = ((size_t)p.B * p.H * p.W * p.Cout + 7) & ~(size_t)7;
        float *ws = p.y + (size_t)blockIdx.z * slice;
        const int npix = p.TH * TW;
#pragma unroll
        for (int ms = 0; ms < MR; ++ms) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = (wm * MR + ms) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                const int ty = (m * p.rcpTW) >> 16, tx = m - ty * TW;
                const bool ok = (m < npix) && (y0 + ty < p.H) && (x0 + tx < p.W);
                const size_t o = (((size_t)b * p.H + y0 + ty) * p.W + x0 + tx) * p.Cout;
#pragma unroll
                for (int ns = 0; ns < NR; ++ns) {
                    const int n = n0 + (wn * NR + ns) * 32 + li;
                    if (ok && n < p.Cout) ws[o + n] = acc[ms][ns][r];
                }
            }
        }
        return;
    }
// (a kernel that includes this body may name its own epilogue: conv_head_f16.hip -- text substitution, so that every kernel of
// conv_f16.hip keeps its machine code)
#ifdef CONV_F16_BODY_EPILOGUE
#include CONV_F16_BODY_EPILOGUE
#else
#include "conv_f16_epilogue.inc"
#endif
