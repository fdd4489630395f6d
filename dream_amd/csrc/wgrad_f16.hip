// Half-precision weight + bias gradient of a 3x3 stride-1 conv (train_precision="fp16"; replaces ATen's conv backward-weight reached
// from loss.backward(), dream/network.py:335, for the plain Conv2d layers of dream/models.py:594-615, 695-747):
//
//   dW[t][co][ci] = 2^-(ex+eg) * sum over (b, y, x) of  fp16(dy[b,y,x,co] * 2^eg) * fp16(x[b, y+dy(t), x+dx(t), ci] * 2^ex)
//
// Both operands are fp32 NHWC in HBM and are rounded once, while they are staged into LDS; 2^ex / 2^eg put max|x| / max|dy| (the amax
// scalars, as in conv_f16.hip) into [2^13, 2^14).  The products run on v_mfma_f32_32x32x16_f16 (a product of two halfs is exact in
// fp32), accumulation is fp32.  The bias gradient is the channel sum of the UNROUNDED fp32 dy, summed while dy is staged.
//
// The contraction runs over POSITIONS, and an MFMA operand is 8 consecutive k's of one row / column in one lane: so LDS holds the
// TRANSPOSED images, [channel][position].  A position tile is 8 rows x 16 columns; a k-step (16 positions) is one tile row, a lane's 8 k's
// are 8 consecutive x's of it -- the same order for both operands.
//   sY[co][ty*16 + tx]                    channel stride 136 halfs (272 B: an odd number of 16-B slots -> ds_read_b128 conflict-free)
//   sX[dx][ci][py*16 + tx] = x[y0-1+py][x0-1+tx+dx][ci]     THREE copies of the 10-row patch, shifted by the tap's dx = 0 | 1 | 2, so the
//                                         operand of every tap is an ALIGNED 16-byte read (a tap's dy only selects the row);
//                                         channel stride 168 halfs (336 B: 21 slots).
// Staging: a lane loads the same four channels (one float4) of 8 (dy) or 10 (x) consecutive positions, converts, and writes one
// position-contiguous 16-byte piece per channel (x: per channel and shift).  LDS: 17 + 63 KB = 80 KB, two workgroups per CU.
// Workgroup: 4 waves as 2 x 2 blocks of 32 co x 32 ci, NINE tap accumulators each (144 VGPRs), as wgrad.hip's <1,1,9,128>.  A patch row is
// read once per shift and serves the three taps rows that use it (registers, rolling over the k-steps).
//
// Split-K over position tiles; partials go to the workspace and a second kernel sums them in a FIXED order (deterministic, no
// floating-point atomics) and applies 2^-ex * 2^-eg.
#include <dream_cdna4.h>
#include "common.h"
#include "half_scale.h"
#include "../../include/dream_hip.h"

namespace {

constexpr int TH = 8, TW = 16, PIX = TH * TW;        // position tile
constexpr int PH = TH + 2;                            // patch rows
constexpr int RW = 64, CW = 64;                       // dW tile of a workgroup: rows (co) x columns (ci)
constexpr int SY = PIX + 8;                           // halfs per dy channel
constexpr int SX = PH * TW + 8;                       // halfs per x channel of one shifted copy
constexpr size_t LDS_BYTES = ((size_t)RW * SY + (size_t)3 * CW * SX) * sizeof(_Float16);

struct Wgrad16Params {
    const float *x;          // [B,H,W,Cin]
    const float *dy;         // [B,H,W,Ct]
    const unsigned *amax_x, *amax_dy;
    float *part;             // [splitk][9][RowsPad][Cin]
    float *bias_part;        // [splitk][RowsPad] or null
    int B, H, W, Cin, Ct, RowsPad;
    int tiles_x, tiles_y, tiles_total, splitk, nrb, ncb;
};

DREAM_DEVICE float pow2f(int e) { return __uint_as_float((unsigned)(e + 127) << 23); }

__global__ void __launch_bounds__(256, 2) wgrad_f16_kernel(const Wgrad16Params p) {
    constexpr bool X16 = false;
    constexpr bool DY16 = false;
#include "wgrad_f16_body.inc"
}

// The same kernel on an x stored as IEEE half (train_activation_storage="fp16"; dream_conv3x3_wgrad_f16_x16_nhwc_f32): half the x
// staging bytes, no v_cvt, no multiply.  A kernel of its own from the same text, so that the one above stays instruction-identical.
__global__ void __launch_bounds__(256, 2) wgrad_f16_x16_kernel(const Wgrad16Params p) {
    constexpr bool X16 = true;
    constexpr bool DY16 = false;
#include "wgrad_f16_body.inc"
}

// ... and on a dy stored as IEEE half times 2^e_g (train_gradient_storage="fp16"; dream_conv3x3_wgrad_f16_x16_dy16_nhwc_f32): the stored
// half IS the operand -- dy staging copies 8-byte pieces of four halfs: half the bytes, no v_cvt, no multiply; amax_dy is not read.
// The bias partial is the fp32 channel sum of the stored halfs.  2^-e_g is applied by wgrad_f16_reduce_g16_kernel.
__global__ void __launch_bounds__(256, 2) wgrad_f16_x16_dy16_kernel(const Wgrad16Params p) {
    constexpr bool X16 = true;
    constexpr bool DY16 = true;
#include "wgrad_f16_body.inc"
}

// fixed-order sum over the split-K partials, times 2^-ex * 2^-eg (two exact steps: either factor alone is a normal number)
__global__ void __launch_bounds__(256) wgrad_f16_reduce_kernel(const float *part, float *out, size_t n, int splitk,
                                                               const unsigned *amax_x, const unsigned *amax_dy) {
    const float ix = amax_x ? pow2f(-scale_exponent(*amax_x)) : 1.0f, ig = amax_dy ? pow2f(-scale_exponent(*amax_dy)) : 1.0f;
    const size_t n4 = n / 4;                         // n is a multiple of 4 (channel counts are)
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        f32x4 s = {0.0f, 0.0f, 0.0f, 0.0f};
        const f32x4 *src = (const f32x4 *)part + i;
        int k = 0;
        for (; k + 8 <= splitk; k += 8) {            // eight independent loads in flight, summed in index order
            f32x4 v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = src[(size_t)(k + j) * n4];
#pragma unroll
            for (int j = 0; j < 8; ++j) s += v[j];
        }
        for (; k < splitk; ++k) s += src[(size_t)k * n4];
        ((f32x4 *)out)[i] = (s * ix) * ig;
    }
}

// wgrad_f16_reduce_kernel for the launches of wgrad_f16_x16_dy16_kernel (weights and bias): the same fixed-order sum, times 2^-e_g where
// that kernel applies 2^-eg -- e_g = grad_scale_exponent of the loss gradient's amax (half_scale.h), an exact power of two.
__global__ void __launch_bounds__(256) wgrad_f16_reduce_g16_kernel(const float *part, float *out, size_t n, int splitk,
                                                                   const unsigned *grad_amax) {
    const float ig = pow2f(-grad_scale_exponent(*grad_amax));
    const size_t n4 = n / 4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        f32x4 s = {0.0f, 0.0f, 0.0f, 0.0f};
        const f32x4 *src = (const f32x4 *)part + i;
        int k = 0;
        for (; k + 8 <= splitk; k += 8) {
            f32x4 v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = src[(size_t)(k + j) * n4];
#pragma unroll
            for (int j = 0; j < 8; ++j) s += v[j];
        }
        for (; k < splitk; ++k) s += src[(size_t)k * n4];
        ((f32x4 *)out)[i] = s * ig;
    }
}

// ---- ResnetSimple's train_decoder_precision="fp16" (DESIGN.md 4.8n): the weight gradient of ConvTranspose2d(k4,s2,p1) ---------------------
//   dW[ci][co][ty][tx] = 2^-eg * sum over (b, i, j) of  fp16(clamp(x[b,i,j,ci])) * fp16(dz[b, 2i+ty-1, 2j+tx-1, co] * 2^eg)
// Sixteen 32 x 32 tap accumulators do not fit beside the operands (the 3x3 kernel's nine sit on the 256-VGPR limit), so a workgroup owns ONE
// sub-pixel phase (a, b) of dz: against the phase plane P[u][v] = dz[2u+a][2v+b] the four taps ty = 2 dy + 1 - a, tx = 2 dx + 1 - b are the
// 2 x 2 taps P[i - a + dy][j - b + dx] of a stride-1 problem -- the 3x3 kernel's scheme with 4 accumulators, a 9-row patch and TWO shifted
// copies.  x plays the unshifted operand (rows of the dW tile: ci), dz the patch (columns: co); dz is staged with position stride 2, 4
// contiguous channels a lane and position.  x is a ReLU output: e_x = 0, clamped to +-65504 (4.8j).  Split over position tiles into
// part[ks][16][RowsPad][Cdz] (every tap is written by exactly one phase), summed in slice order and scaled by wgrad_f16_reduce_kernel.
constexpr int TPH = TH + 1;                              // patch rows of a phase
constexpr int SXT = TPH * TW + 8;                        // halfs per dz channel of one shifted copy (304 B: 19 16-byte slots)
constexpr size_t LDS_BYTES_T4 = ((size_t)RW * SY + (size_t)2 * CW * SXT) * sizeof(_Float16);

struct WgradT4Params {
    const float *x;          // [B,H,W,Cin]
    const float *dz;         // [B,2H,2W,Cdz]
    const unsigned *amax_dz;
    float *part;             // [splitk][16][RowsPad][Cdz]
    int B, H, W, Cin, Cdz, RowsPad;
    int tiles_x, tiles_y, tiles_total, splitk, nrb, ncb;
};

__global__ void __launch_bounds__(256, 2) wgrad_convT4_f16_kernel(const WgradT4Params p) {
    constexpr bool XS = false;
    const unsigned *const amax_x = nullptr;          // (not read)
#include "wgrad_convT4_f16_body.inc"
}

// ---- DreamHourglass's train_upsample_precision="fp16" (DESIGN.md 4.8o): the weight gradient of nn.Upsample(2) + Conv2d(3x3) as that of the
// equivalent ConvTranspose2d(k4,s2,p1).  The hourglass scales every operand by its tensor's amax (the input of upsample_0_3.4 is the output
// of a conv without a ReLU), so x is staged as half(x * 2^e_x), e_x = scale_exponent(amax_x): the rounding the forward applied, no clamp.
// A kernel of its own from the same text, so that the one above stays instruction-identical.
__global__ void __launch_bounds__(256, 2) wgrad_convT4_f16_xs_kernel(const WgradT4Params p, const unsigned *amax_x) {
    constexpr bool XS = true;
#include "wgrad_convT4_f16_body.inc"
}

// ... and its reduce, which also folds the 4x4 gradient back to the 3x3 one: per (co, ci) the sixteen tap slots of part[ks][4 ky + kx][ci][co]
// are summed over the slices in slice order, then dw3[r][c] = sum over ky in K(r), kx in K(c) of dwT[ky][kx], K(0) = {2,3}, K(1) = {1,2},
// K(2) = {0,1} (the adjoint of dream_upsample_conv3x3_weight_as_convT4x4; wgrad_wino.hip's convT4x4_grad_to_conv3x3_kernel), the four
// slots added in ascending (ky, kx); times 2^-ex * 2^-eg once (two exact steps; a null amax: factor 1) -> OIHW [Cdz][Cin][3][3].  A fixed
// order throughout: two runs give the same bits.  Lanes run along co (the contiguous index of the partials).
__global__ void __launch_bounds__(256) wgrad_convT4_fold3x3_reduce_kernel(const float *part, float *dw, int splitk, int Cin, int Cdz, int RowsPad,
                                                                          const unsigned *amax_x, const unsigned *amax_dz) {
    const float ix = amax_x ? pow2f(-scale_exponent(*amax_x)) : 1.0f, ig = amax_dz ? pow2f(-scale_exponent(*amax_dz)) : 1.0f;
    const size_t n = (size_t)Cin * Cdz, slot_stride = (size_t)RowsPad * Cdz;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int ci = (int)(i / (size_t)Cdz), co = (int)(i - (size_t)ci * Cdz);
        const float *src = part + (size_t)ci * Cdz + co;
        float v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = 0.0f;
        for (int ks = 0; ks < splitk; ++ks) {
            float t[16];                             // sixteen independent loads in flight, added in slice order
#pragma unroll
            for (int k = 0; k < 16; ++k) t[k] = src[((size_t)ks * 16 + k) * slot_stride];
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] += t[k];
        }
        float *o = dw + ((size_t)co * Cin + ci) * 9;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int ky = 2 - r, kx = 2 - c;               // K(r) = {2 - r, 3 - r}
                const float s = ((v[4 * ky + kx] + v[4 * ky + kx + 1]) + v[4 * ky + 4 + kx]) + v[4 * ky + 4 + kx + 1];
                o[3 * r + c] = (s * ix) * ig;
            }
    }
}

int plan_splitk_T4(int B, int H, int W, int Cdz, int RowsPad) {
    const long tiles = (long)B * ceil_div(H, TH) * ceil_div(W, TW);
    const long ctiles = (long)ceil_div(RowsPad, RW) * ceil_div(Cdz, CW) * 4;      // x 4 phases
    long sk = wgrad_target_workgroups(512) / ctiles;
    if (sk < 1) sk = 1;
    if (sk > tiles) sk = tiles;
    if (sk > 1024) sk = 1024;
    return (int)sk;
}

bool shape_ok_T4(int B, int H, int W, int Cin, int Cdz, int RowsPad) {
    return B > 0 && H > 0 && W > 0 && Cin > 0 && Cin % 32 == 0 && Cdz > 0 && Cdz % 4 == 0 && RowsPad >= Cin && RowsPad % 64 == 0;
}

int plan_splitk(int B, int H, int W, int Cin, int RowsPad) {
    const long tiles = (long)B * ceil_div(H, TH) * ceil_div(W, TW);
    const long ctiles = (long)ceil_div(RowsPad, RW) * ceil_div(Cin, CW);
    long sk = wgrad_target_workgroups(512) / ctiles;      // 512 workgroups = 256 CUs x 2 resident (wgrad.hip)
    if (sk < 1) sk = 1;
    if (sk > tiles) sk = tiles;
    if (sk > 1024) sk = 1024;
    return (int)sk;
}

bool shape_ok(int B, int H, int W, int Cin, int RowsPad) {
    return B > 0 && H > 0 && W > 0 && Cin > 0 && Cin % 32 == 0 && RowsPad > 0 && RowsPad % 64 == 0;
}

}  // namespace

// number of position slices the contraction of this problem is split into (a pure host computation: no GPU is touched)
extern "C" int dream_conv3x3_wgrad_f16_splitk(int B, int H, int W, int Cin, int RowsPad) {
    return shape_ok(B, H, W, Cin, RowsPad) ? plan_splitk(B, H, W, Cin, RowsPad) : 0;
}

extern "C" size_t dream_conv3x3_wgrad_f16_workspace(int B, int H, int W, int Cin, int RowsPad) {
    if (!shape_ok(B, H, W, Cin, RowsPad)) return 0;
    const size_t sk = (size_t)plan_splitk(B, H, W, Cin, RowsPad);
    return (sk * 9 * RowsPad * Cin + (sk + 1) * RowsPad) * sizeof(float);
}

namespace {

// The three forms of the launch: the kernel and which operands it reads as IEEE half.  x16: amax_x is not used, the reduce takes a null
// amax_x (factor 1); dy16: dy is half times 2^e_g, amax_dy is the scalar e_g is derived from (the loss gradient's amax) by the g16 reduce
enum WgradForm { kWgradF32, kWgradX16, kWgradX16Dy16 };
const struct { void (*kernel)(const Wgrad16Params); bool x16, dy16; } kWgradForms[] = {
    {wgrad_f16_kernel, false, false}, {wgrad_f16_x16_kernel, true, false}, {wgrad_f16_x16_dy16_kernel, true, true}};

int launch_wgrad16(WgradForm form, const void *x, const unsigned *amax_x, const void *dy, const unsigned *amax_dy, float *dw_packed,
                   float *dbias, void *workspace, int B, int H, int W, int Cin, int Cdy, int RowsPad, int flags, void *stream) {
    const auto &f = kWgradForms[form];
    DREAM_REQUIRE(x && (amax_x || f.x16) && dy && amax_dy && dw_packed && workspace, "wgrad_f16: null pointer");
    DREAM_REQUIRE(flags == 0, "wgrad_f16: flags %d not supported (plain 3x3 stride-1 convs only)", flags);
    DREAM_REQUIRE(shape_ok(B, H, W, Cin, RowsPad) && Cdy > 0 && Cdy % 4 == 0 && RowsPad >= Cdy,
                  "wgrad_f16: bad shape (B %d, %d x %d, Cin %d, Cdy %d, pad %d): Cin %% 32, Cdy %% 4, pad %% 64", B, H, W, Cin, Cdy, RowsPad);
    DREAM_REQUIRE((size_t)B * H * W * (size_t)(Cin > Cdy ? Cin : Cdy) < ((size_t)1 << 40), "wgrad_f16: tensor too large");
    DREAM_REQUIRE(!f.x16 || ((size_t)x & 15) == 0, "wgrad_f16: a half x must be 16-byte aligned");
    DREAM_REQUIRE(!f.dy16 || ((size_t)dy & 15) == 0, "wgrad_f16: a half dy must be 16-byte aligned");
    Wgrad16Params p;
    p.x = (const float *)x; p.dy = (const float *)dy; p.amax_x = f.x16 ? nullptr : amax_x; p.amax_dy = amax_dy;
    p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.Ct = Cdy; p.RowsPad = RowsPad;
    p.tiles_x = ceil_div(W, TW); p.tiles_y = ceil_div(H, TH);
    p.tiles_total = B * p.tiles_x * p.tiles_y;
    p.splitk = plan_splitk(B, H, W, Cin, RowsPad);
    p.nrb = ceil_div(RowsPad, RW); p.ncb = ceil_div(Cin, CW);
    p.part = (float *)workspace;
    float *bias_part = p.part + (size_t)p.splitk * 9 * RowsPad * Cin;
    p.bias_part = dbias ? bias_part : nullptr;
    if (dream_allow_full_lds((const void *)f.kernel)) return 2;
    const dim3 grid((unsigned)(p.nrb * p.ncb * ceil_div(p.splitk, 8) * 8));
    hipLaunchKernelGGL(f.kernel, grid, dim3(256), LDS_BYTES, (hipStream_t)stream, p);
    DREAM_LAUNCH_OK();
    // the form's reduce kernel over n sums: times 2^-e_g (a half dy), else times 2^-ex * 2^-eg of the amax scalars given (null: 1)
    const auto reduce = [&](size_t blocks, const float *part, float *out, size_t n, const unsigned *ax, const unsigned *ady) {
        if (f.dy16)
            hipLaunchKernelGGL(wgrad_f16_reduce_g16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, part, out, n, p.splitk, amax_dy);
        else
            hipLaunchKernelGGL(wgrad_f16_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, part, out, n, p.splitk, ax, ady);
    };
    const size_t n = (size_t)9 * RowsPad * Cin;
    reduce((n / 4 + 255) / 256 > 2048 ? 2048 : (n / 4 + 255) / 256, p.part, dw_packed, n, p.amax_x, amax_dy);
    DREAM_LAUNCH_OK();
    if (dbias) {
        // bias partials are [splitk][RowsPad] of unscaled sums (a half dy's carry 2^e_g as well); only the first Cdy entries are wanted
        float *total = bias_part + (size_t)p.splitk * RowsPad;
        reduce(1, bias_part, total, (size_t)RowsPad, nullptr, nullptr);
        DREAM_LAUNCH_OK();
        if (dream_copy_words(dbias, total, (size_t)Cdy * sizeof(float), (hipStream_t)stream)) return 2;
    }
    return 0;
}

}  // namespace

// x [B,H,W,Cin], dy [B,H,W,Cdy] (fp32 NHWC), amax_x / amax_dy: device scalars, bit patterns of (an upper bound of) max|x| / max|dy|
// -> dw_packed [9][RowsPad][Cin] (mode-0 layout: dream_unpack_conv3x3_weight), dbias [Cdy] or null.  Cin % 32 == 0, Cdy % 4 == 0,
// RowsPad >= Cdy a multiple of 64; flags must be 0.
extern "C" int dream_conv3x3_wgrad_f16_nhwc_f32(const float *x, const unsigned *amax_x, const float *dy, const unsigned *amax_dy,
                                                float *dw_packed, float *dbias, void *workspace, int B, int H, int W, int Cin,
                                                int Cdy, int RowsPad, int flags, void *stream) {
    return launch_wgrad16(kWgradF32, x, amax_x, dy, amax_dy, dw_packed, dbias, workspace, B, H, W, Cin, Cdy, RowsPad, flags, stream);
}

// The same with x stored as IEEE half (train_activation_storage="fp16"): x [B,H,W,Cin] half, 16-byte aligned, is the operand as it is
// (no scale, no amax_x); dy, the outputs, the workspace (dream_conv3x3_wgrad_f16_workspace) and the split are unchanged.
extern "C" int dream_conv3x3_wgrad_f16_x16_nhwc_f32(const void *x, const float *dy, const unsigned *amax_dy, float *dw_packed,
                                                    float *dbias, void *workspace, int B, int H, int W, int Cin, int Cdy,
                                                    int RowsPad, int flags, void *stream) {
    return launch_wgrad16(kWgradX16, x, nullptr, dy, amax_dy, dw_packed, dbias, workspace, B, H, W, Cin, Cdy, RowsPad, flags, stream);
}

// The same with dy stored as IEEE half as well (train_gradient_storage="fp16"): dy [B,H,W,Cdy] half, 16-byte aligned, holds the gradient
// times 2^e_g and is the operand as it is (no amax of dy is read); grad_amax: device scalar, bit pattern of the loss gradient's amax,
// from which e_g = 9 - exponent is derived as by every launch of that backward.  dw and dbias (the fp32 channel sum of the stored halfs)
// are multiplied by 2^-e_g once, in the reduce kernel.  Workspace, split and summation order are those of the other two forms.
extern "C" int dream_conv3x3_wgrad_f16_x16_dy16_nhwc_f32(const void *x, const void *dy, const unsigned *grad_amax, float *dw_packed,
                                                         float *dbias, void *workspace, int B, int H, int W, int Cin, int Cdy,
                                                         int RowsPad, int flags, void *stream) {
    return launch_wgrad16(kWgradX16Dy16, x, nullptr, dy, grad_amax, dw_packed, dbias, workspace, B, H, W, Cin, Cdy, RowsPad, flags, stream);
}

// ---- the weight gradient of ConvTranspose2d(k4,s2,p1) on the fp16 matrix cores (ResnetSimple's train_decoder_precision="fp16"; replaces
// ATen's conv-transpose backward-weight reached from loss.backward() for the decoder stages of dream/models.py:37-136) ------------------
// position slices of this problem (a pure host computation: no GPU is touched); 0 for a shape the launch refuses
extern "C" int dream_convT4x4_wgrad_f16_splitk(int B, int H, int W, int Cin, int Cdz, int RowsPad) {
    return shape_ok_T4(B, H, W, Cin, Cdz, RowsPad) ? plan_splitk_T4(B, H, W, Cdz, RowsPad) : 0;
}

extern "C" size_t dream_convT4x4_wgrad_f16_workspace(int B, int H, int W, int Cin, int Cdz, int RowsPad) {
    if (!shape_ok_T4(B, H, W, Cin, Cdz, RowsPad)) return 0;
    return (size_t)plan_splitk_T4(B, H, W, Cdz, RowsPad) * 16 * RowsPad * Cdz * sizeof(float);
}

// x [B,H,W,Cin] fp32 (a ReLU output: rounded as it is, clamped to +-65504), dz [B,Ho,Wo,Cdz] fp32 with Ho = 2 H, Wo = 2 W, amax_dz: device
// scalar, bit pattern of (an upper bound of) max|dz| -> dw_packed [16][RowsPad][Cdz], slice 4 ty + tx (dream_unpack_conv_weight gives
// [Cin,Cdz,4,4]).  Cin % 32 == 0, Cdz % 4 == 0, RowsPad >= Cin a multiple of 64; x, dz, dw_packed and the workspace 16-byte aligned; flags 0.
extern "C" int dream_convT4x4_wgrad_f16_nhwc_f32(const float *x, const float *dz, const unsigned *amax_dz, float *dw_packed, void *workspace,
                                                 int B, int Ho, int Wo, int Cin, int Cdz, int RowsPad, int flags, void *stream) {
    DREAM_REQUIRE(flags == 0, "convT4x4_wgrad_f16: flags %d not supported", flags);
    DREAM_REQUIRE(Ho >= 2 && Wo >= 2 && Ho % 2 == 0 && Wo % 2 == 0,
                  "convT4x4_wgrad_f16: dz of %d x %d: the output of the transposed conv has even dimensions", Ho, Wo);
    const int H = Ho / 2, W = Wo / 2;
    DREAM_REQUIRE(shape_ok_T4(B, H, W, Cin, Cdz, RowsPad),
                  "convT4x4_wgrad_f16: bad shape (B %d, %d x %d, Cin %d, Cdz %d, pad %d): Cin %% 32, Cdz %% 4, pad %% 64", B, H, W, Cin, Cdz, RowsPad);
    DREAM_REQUIRE((size_t)B * Ho * Wo * (size_t)(Cin > Cdz ? Cin : Cdz) < ((size_t)1 << 40), "convT4x4_wgrad_f16: tensor too large");
    DREAM_REQUIRE(x && dz && amax_dz && dw_packed && workspace, "convT4x4_wgrad_f16: null pointer");
    DREAM_REQUIRE((((size_t)x | (size_t)dz | (size_t)dw_packed | (size_t)workspace) & 15) == 0, "convT4x4_wgrad_f16: pointers must be 16-byte aligned");
    WgradT4Params p;
    p.x = x; p.dz = dz; p.amax_dz = amax_dz; p.part = (float *)workspace;
    p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.Cdz = Cdz; p.RowsPad = RowsPad;
    p.tiles_x = ceil_div(W, TW); p.tiles_y = ceil_div(H, TH);
    p.tiles_total = B * p.tiles_x * p.tiles_y;
    p.splitk = plan_splitk_T4(B, H, W, Cdz, RowsPad);
    p.nrb = ceil_div(RowsPad, RW); p.ncb = ceil_div(Cdz, CW);
    if (dream_allow_full_lds((const void *)wgrad_convT4_f16_kernel)) return 2;
    const dim3 grid((unsigned)(p.nrb * p.ncb * 4 * ceil_div(p.splitk, 8) * 8));
    hipLaunchKernelGGL(wgrad_convT4_f16_kernel, grid, dim3(256), LDS_BYTES_T4, (hipStream_t)stream, p);
    DREAM_LAUNCH_OK();
    const size_t n = (size_t)16 * RowsPad * Cdz;
    hipLaunchKernelGGL(wgrad_f16_reduce_kernel, dim3((unsigned)((n / 4 + 255) / 256 > 2048 ? 2048 : (n / 4 + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, (const float *)p.part, dw_packed, n, p.splitk, (const unsigned *)nullptr, amax_dz);
    DREAM_LAUNCH_OK();
    return 0;
}

// ---- the weight gradient of nn.Upsample(2) + Conv2d(3x3) on the fp16 matrix cores (DreamHourglass's train_upsample_precision="fp16"; replaces
// ATen's conv backward-weight reached from loss.backward() for the upsample convs of dream/models.py:688-733) -------------------------------
// H x W: the low-resolution input of the upsample.  The contraction is that of the equivalent ConvTranspose2d(k4,s2,p1): split and workspace
// are the convT4 launch's, with the rows padded to whole 64-channel tiles here.
extern "C" int dream_upsample_conv3x3_wgrad_f16_splitk(int B, int H, int W, int Cin, int Cdz) {
    return dream_convT4x4_wgrad_f16_splitk(B, H, W, Cin, Cdz, Cin > 0 ? ceil_div(Cin, 64) * 64 : 0);
}

extern "C" size_t dream_upsample_conv3x3_wgrad_f16_workspace(int B, int H, int W, int Cin, int Cdz) {
    return dream_convT4x4_wgrad_f16_workspace(B, H, W, Cin, Cdz, Cin > 0 ? ceil_div(Cin, 64) * 64 : 0);
}

// The reduce of that launch on its own: part [splitk][16][RowsPad][Cdz] (slot 4 ky + kx of the 4x4 gradient, scaled domain) -> dw_oihw
// [Cdz][Cin][3][3] = 2^-(ex+eg) * fold(sum over the slices); amax_x / amax_dz may be null (factor 1).
extern "C" int dream_upsample_conv3x3_wgrad_f16_fold(const float *part, const unsigned *amax_x, const unsigned *amax_dz, float *dw_oihw,
                                                     int splitk, int Cin, int Cdz, int RowsPad, void *stream) {
    DREAM_REQUIRE(part && dw_oihw, "upsample_conv3x3_wgrad_f16_fold: null pointer");
    DREAM_REQUIRE(splitk > 0 && Cin > 0 && Cdz > 0 && RowsPad >= Cin, "upsample_conv3x3_wgrad_f16_fold: bad shape (split %d, Cin %d, Cdz %d, pad %d)",
                  splitk, Cin, Cdz, RowsPad);
    size_t grid = ((size_t)Cin * Cdz + 255) / 256;
    if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(wgrad_convT4_fold3x3_reduce_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, part, dw_oihw, splitk, Cin, Cdz,
                       RowsPad, amax_x, amax_dz);
    DREAM_LAUNCH_OK();
    return 0;
}

// x [B,H,W,Cin] fp32 with H = Ho / 2, W = Wo / 2 (the input of the upsample), amax_x: device scalar, bit pattern of (an upper bound of) max|x|:
// x is rounded as half(x 2^e_x), what the forward launch did; dz [B,Ho,Wo,Cdz] fp32 with its amax_dz likewise -> dw_oihw [Cdz][Cin][3][3], the
// gradient of the 3x3 weight.  Cin % 32 == 0, Cdz % 4 == 0; x, dz, dw_oihw and the workspace (dream_upsample_conv3x3_wgrad_f16_workspace)
// 16-byte aligned; flags 0.  Two launches, no atomics: two runs give the same bits.
extern "C" int dream_upsample_conv3x3_wgrad_f16_nhwc_f32(const float *x, const unsigned *amax_x, const float *dz, const unsigned *amax_dz,
                                                         float *dw_oihw, void *workspace, int B, int Ho, int Wo, int Cin, int Cdz, int flags,
                                                         void *stream) {
    DREAM_REQUIRE(flags == 0, "upsample_conv3x3_wgrad_f16: flags %d not supported", flags);
    DREAM_REQUIRE(Ho >= 2 && Wo >= 2 && Ho % 2 == 0 && Wo % 2 == 0,
                  "upsample_conv3x3_wgrad_f16: dz of %d x %d: the output of an upsample has even dimensions", Ho, Wo);
    const int H = Ho / 2, W = Wo / 2, RowsPad = Cin > 0 ? ceil_div(Cin, 64) * 64 : 0;
    DREAM_REQUIRE(shape_ok_T4(B, H, W, Cin, Cdz, RowsPad), "upsample_conv3x3_wgrad_f16: bad shape (B %d, %d x %d, Cin %d, Cdz %d): Cin %% 32, Cdz %% 4",
                  B, H, W, Cin, Cdz);
    DREAM_REQUIRE((size_t)B * Ho * Wo * (size_t)(Cin > Cdz ? Cin : Cdz) < ((size_t)1 << 40), "upsample_conv3x3_wgrad_f16: tensor too large");
    DREAM_REQUIRE(x && amax_x && dz && amax_dz && dw_oihw && workspace, "upsample_conv3x3_wgrad_f16: null pointer");
    DREAM_REQUIRE((((size_t)x | (size_t)dz | (size_t)dw_oihw | (size_t)workspace) & 15) == 0, "upsample_conv3x3_wgrad_f16: pointers must be 16-byte aligned");
    WgradT4Params p;
    p.x = x; p.dz = dz; p.amax_dz = amax_dz; p.part = (float *)workspace;
    p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.Cdz = Cdz; p.RowsPad = RowsPad;
    p.tiles_x = ceil_div(W, TW); p.tiles_y = ceil_div(H, TH);
    p.tiles_total = B * p.tiles_x * p.tiles_y;
    p.splitk = plan_splitk_T4(B, H, W, Cdz, RowsPad);
    p.nrb = ceil_div(RowsPad, RW); p.ncb = ceil_div(Cdz, CW);
    if (dream_allow_full_lds((const void *)wgrad_convT4_f16_xs_kernel)) return 2;
    const dim3 grid((unsigned)(p.nrb * p.ncb * 4 * ceil_div(p.splitk, 8) * 8));
    hipLaunchKernelGGL(wgrad_convT4_f16_xs_kernel, grid, dim3(256), LDS_BYTES_T4, (hipStream_t)stream, p, amax_x);
    DREAM_LAUNCH_OK();
    return dream_upsample_conv3x3_wgrad_f16_fold(p.part, amax_x, amax_dz, dw_oihw, p.splitk, Cin, Cdz, RowsPad, stream);
}
