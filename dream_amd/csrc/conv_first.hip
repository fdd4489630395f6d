// First encoder convolution: NCHW fp32 image (Cin <= 4) -> NHWC fp32 [B,H,W,Cout], 3x3 s1 p1 + bias
// (+ReLU): the fresh Conv2d(3,64,3,1,1) in front of the VGG encoder.
//
// K = 9*Cin = 27 is far too shallow for the matrix cores and the layer is store-bound (it writes
// 256 B per pixel for 1.7 kFLOP), so it runs on the vector ALU and everything is arranged around the stores:
//   * a lane owns FOUR consecutive output channels of a pixel and writes them as one dwordx4: the sixteen lanes of a
//     quarter-wave cover a pixel's 256 B, one wave-instruction four pixels -- a quarter of the store instructions of the
//     lane == channel form (which was bound by their issue: 3.55 TB/s against the 6 TB/s plain stores reach);
//   * the lane's 4 x 9*Cin weights live in VGPRs, loaded ONCE per workgroup: the workgroups are persistent (the grid is what
//     the chip holds) and walk over the 16 x 16-pixel tiles;
//   * the input patch of a tile sits in LDS, read as b128 + b64 per (channel, filter row) for the lane's four pixels (four
//     addresses per instruction, one per quarter-wave, 16 B apart: no bank conflict); two patch buffers: the next tile's
//     patch is fetched into registers before the current tile is computed and written to the other buffer after it -- one
//     barrier per tile, the global latency behind the FMAs;
//   * a thread stages the same patch column in every tile and steps down the rows: no division per element.
// Every output element starts from the bias and takes one fmaf per tap in the order (channel, filter row, filter column).
#include <stdlib.h>
#include <dream_cdna4.h>
#include "common.h"
#include "../../include/dream_hip.h"

namespace {
constexpr int FT = 16;            // 16 x 16 output pixels per tile
constexpr int FPW = FT + 4;       // patch row: 1 halo + 16 + 1 halo, padded to 20 pixels (rows stay 16-byte aligned)
constexpr int FPH = FT + 2;
constexpr int FMAXC = 4;
constexpr int FPLANE = FPH * FPW;             // floats per channel: [row][pixel]
constexpr int FIRST_WG_PER_CU = 3;            // 256-thread workgroups a CU holds at the kernel's register count (3 waves per SIMD)
constexpr int FIRST_CUS = 256;

struct FirstParams {
    const float *x;
    const float *w;
    const float *bias;
    float *y;
    unsigned *amax_out;
    int B, H, W, Cin, Cout;
    int tiles_x, tiles_y, ntiles;
    int relu;
};

template <int CIN>
__global__ void __launch_bounds__(256, CIN <= 3 ? 3 : 2) conv3x3_first_kernel(const FirstParams p) {
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
    const unsigned px_b = (unsigned)p.Cout * 4u, voff = (unsigned)(4 * lg) * px_b + (unsigned)cout * 4u;   // byte offsets inside a row of the tile
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
            const BufferRsrc yrow = make_buffer(p.y + (((size_t)tl.b * p.H + oy) * p.W + tl.x0) * p.Cout, (size_t)npx * p.Cout * sizeof(float));
#pragma unroll
            for (int i = 0; i < 4; ++i) buffer_store_x4(yrow, acc[i], voff + (unsigned)i * px_b, 0u);
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
}

template <int CIN>
void launch_first(const FirstParams &p, int gx, void *stream) {
    void (*kernel)(const FirstParams) = conv3x3_first_kernel<CIN>;
    const size_t lds = (size_t)2 * CIN * FPLANE * sizeof(float);
    hipLaunchKernelGGL(kernel, dim3((unsigned)gx, (unsigned)(p.Cout / 64)), dim3(256), lds, (hipStream_t)stream, p);
}
}  // namespace

static int first_impl(const float *x_nchw, const float *w_oihw, const float *bias, float *y_nhwc, int B, int H, int W,
                      int Cin, int Cout, int relu, void *stream, unsigned *amax_out) {
    DREAM_REQUIRE(x_nchw && w_oihw && y_nhwc, "null pointer");
    DREAM_REQUIRE(B > 0 && H > 0 && W > 0, "bad shape");
    DREAM_REQUIRE(Cin >= 1 && Cin <= FMAXC, "first conv supports Cin <= %d (got %d)", FMAXC, Cin);
    DREAM_REQUIRE(Cout % 64 == 0, "first conv needs Cout %% 64 == 0 (got %d)", Cout);
    DREAM_REQUIRE((size_t)Cin * H * W * sizeof(float) < ((size_t)1 << 31), "first conv: image too large for 32-bit offsets");
    FirstParams p;
    p.x = x_nchw; p.w = w_oihw; p.bias = bias; p.y = y_nhwc; p.amax_out = amax_out;
    p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.relu = relu;
    p.tiles_x = ceil_div(W, FT); p.tiles_y = ceil_div(H, FT);
    const size_t ntiles = (size_t)B * p.tiles_x * p.tiles_y;
    DREAM_REQUIRE(ntiles < ((size_t)1 << 31), "first conv: too many tiles");
    p.ntiles = (int)ntiles;
    // persistent grid: what the chip holds, shared among the 64-channel blocks.  DREAM_FIRST_MAX_WORKGROUPS (tests): a smaller
    // grid, so that a workgroup walks over several tiles of a small problem -- same bits
    int resident = FIRST_CUS * FIRST_WG_PER_CU;
    if (const char *e = getenv("DREAM_FIRST_MAX_WORKGROUPS")) {
        const int cap = atoi(e);
        if (cap > 0) resident = cap;
    }
    int gx = resident / (Cout / 64);
    if (gx < 1) gx = 1;
    if (gx > p.ntiles) gx = p.ntiles;
    switch (Cin) {
        case 1: launch_first<1>(p, gx, stream); break;
        case 2: launch_first<2>(p, gx, stream); break;
        case 3: launch_first<3>(p, gx, stream); break;
        default: launch_first<4>(p, gx, stream); break;
    }
    DREAM_LAUNCH_OK();
    return 0;
}

extern "C" int dream_conv3x3_first_nchw_f32(const float *x_nchw, const float *w_oihw, const float *bias,
                                            float *y_nhwc, int B, int H, int W, int Cin, int Cout,
                                            int relu, void *stream) {
    return first_impl(x_nchw, w_oihw, bias, y_nhwc, B, H, W, Cin, Cout, relu, stream, nullptr);
}
extern "C" int dream_conv3x3_first_nchw_amax_f32(const float *x_nchw, const float *w_oihw, const float *bias,
                                                 float *y_nhwc, unsigned *amax_out, int B, int H, int W, int Cin,
                                                 int Cout, int relu, void *stream) {
    return first_impl(x_nchw, w_oihw, bias, y_nhwc, B, H, W, Cin, Cout, relu, stream, amax_out);
}
