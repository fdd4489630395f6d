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
#include "half_store.h"
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
    constexpr bool OUT16 = false;
#include "conv_first_body.inc"
}

// The same kernel storing IEEE half NHWC (activation_storage="fp16"): a kernel of its own from the same text.
template <int CIN>
__global__ void __launch_bounds__(256, CIN <= 3 ? 3 : 2) conv3x3_first_f16_kernel(const FirstParams p) {
    constexpr bool OUT16 = true;
#include "conv_first_body.inc"
}

template <int CIN>
void launch_first(const FirstParams &p, int gx, void *stream, bool out16) {
    void (*kernel)(const FirstParams) = out16 ? conv3x3_first_f16_kernel<CIN> : conv3x3_first_kernel<CIN>;
    const size_t lds = (size_t)2 * CIN * FPLANE * sizeof(float);
    hipLaunchKernelGGL(kernel, dim3((unsigned)gx, (unsigned)(p.Cout / 64)), dim3(256), lds, (hipStream_t)stream, p);
}
}  // namespace

static int first_impl(const float *x_nchw, const float *w_oihw, const float *bias, void *y_nhwc, int B, int H, int W,
                      int Cin, int Cout, int relu, void *stream, unsigned *amax_out, bool out16 = false) {
    DREAM_REQUIRE(x_nchw && w_oihw && y_nhwc, "null pointer");
    DREAM_REQUIRE(B > 0 && H > 0 && W > 0, "bad shape");
    DREAM_REQUIRE(Cin >= 1 && Cin <= FMAXC, "first conv supports Cin <= %d (got %d)", FMAXC, Cin);
    DREAM_REQUIRE(Cout % 64 == 0, "first conv needs Cout %% 64 == 0 (got %d)", Cout);
    DREAM_REQUIRE((size_t)Cin * H * W * sizeof(float) < ((size_t)1 << 31), "first conv: image too large for 32-bit offsets");
    FirstParams p;
    p.x = x_nchw; p.w = w_oihw; p.bias = bias; p.y = (float *)y_nhwc; p.amax_out = amax_out;
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
        case 1: launch_first<1>(p, gx, stream, out16); break;
        case 2: launch_first<2>(p, gx, stream, out16); break;
        case 3: launch_first<3>(p, gx, stream, out16); break;
        default: launch_first<4>(p, gx, stream, out16); break;
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
// y_nhwc [B,H,W,Cout] IEEE half (16-byte aligned): the same fp32 arithmetic, each value saturated to +-65504 and rounded once at the
// store.  amax_out (optional) is NOT zeroed: max|y| before the saturation, atomicMax'ed into a scalar the caller may share.
extern "C" int dream_conv3x3_first_nchw_f16(const float *x_nchw, const float *w_oihw, const float *bias, void *y_nhwc,
                                            unsigned *amax_out, int B, int H, int W, int Cin, int Cout, int relu, void *stream) {
    DREAM_REQUIRE(((size_t)y_nhwc & 15) == 0, "first conv: the half output must be 16-byte aligned");
    return first_impl(x_nchw, w_oihw, bias, y_nhwc, B, H, W, Cin, Cout, relu, stream, amax_out, true);
}
