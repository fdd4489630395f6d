// ResnetSimple's last decoder stage and its head as ONE entry point (inference_head_fusion="on"): ConvTranspose2d(256,
// 256, 4, 2, 1) + folded BatchNorm + ReLU, then Conv2d(256, K, 1) to the K belief maps (dream/models.py:37-136), on half-stored
// activations.  Four launches, one per sub-pixel phase, of the act16 main loop of conv_f16.hip (conv_f16_body.inc) on a tile that owns
// all 256 stage channels of its 128 pixels -- (MR, NR, WM, WN) = (2, 2, 2, 4): 8 wavefronts, 64 accumulator registers, a 192-pixel
// patch --, whose epilogue (conv_f16_head.inc) rounds the stage output to the halfs the unfused stage stores, keeps them in LDS and
// contracts them with the head's packed plane in a second GEMM on v_mfma_f32_32x32x16_f16.  The [B, 2H, 2W, 256] half tensor is never
// allocated; the fp32 NCHW maps land on (2y + a, 2x + b).
//
// Element by element these are the IEEE operations of dream_conv_transpose4x4s2_f16_nhwc_f16 followed by dream_conv2d_f16_nhwc_f16
// (DREAM_CONV_OUT_NCHW), in their order: the same stage loop (a tile shape changes which workgroup sums a pixel, not the order of its
// stages), the same affine and sat_half, 16 MFMAs in ascending k from a zero accumulator, the same head affine -- maps and peak scalar
// are bit-identical to the pair of launches.  LDS: max(loop: 2 x <= 192 x 80 B patch + 2 x 256 x 80 B weights <= 71 680 B,
// head: 128 x 528 B staging + K x 528 B of the head's plane: 76 560 B at K = 17) -- with 121 VGPRs two workgroups a CU up to K = 27.
#include "conv_f16_common.h"

namespace {

struct Head16Params {
    const _Float16 *w;       // [KPad >= 32][256]: the head's packed plane (dream_pack_conv_weight_f16x3's `hi`, mode 0); rows 0 .. 31 are read
    const int *w_exp;        // device scalar: its exponent
    const float *bias;       // [K] or null
    float *maps;             // [B, K, 2H, 2W] fp32
    int K;
};

template <int MR, int NR, int WM, int WN, int NPM, bool DB, bool PRIO = false>
__global__ void __launch_bounds__(64 * WM * WN, 2) convT4_head_f16_kernel(const Conv16Params p, const Head16Params h) {
    // the act16 form of conv_f16_kernel (conv_f16.hip, kForms)
    constexpr bool EPI_MASK = false, ACT16 = true, MASK16 = false, KSPLIT = false, RES16 = false, DGT4 = false, SAT0 = false;
    constexpr int GRAD16 = 0;
#define CONV_F16_BODY_EPILOGUE "conv_f16_head.inc"
#include "conv_f16_body.inc"
#undef CONV_F16_BODY_EPILOGUE
}

constexpr int kHeadBM = 128, kHeadBN = 256, kHeadNPM = 192, kHeadThreads = 512, kHeadKPad = 32;
constexpr int kHeadFlagsOk = DREAM_CONV_RELU;

bool head_shape_ok(int Cin, int Cmid, int K) { return Cin >= KC && Cin % KC == 0 && Cmid == kHeadBN && K >= 1 && K <= kHeadKPad; }

}  // namespace

// 1 exactly for the channel counts dream_conv_transpose4x4s2_head_f16_nhwc_f16 accepts: a host computation
extern "C" int dream_conv_transpose4x4s2_head_f16_applies(int Cin, int Cmid, int K) { return head_shape_ok(Cin, Cmid, K) ? 1 : 0; }

extern "C" int dream_conv_transpose4x4s2_head_f16_nhwc_f16(const void *x, const void *w, const int *w_exp, const float *scale,
                                                           const float *shift, const void *head_w, const int *head_w_exp,
                                                           const float *head_bias, float *maps, unsigned *peak, int B, int H, int W,
                                                           int Cin, int Cmid, int CmidPad, int K, int KPad, int flags, void *stream) {
    DREAM_REQUIRE(x && w && w_exp && head_w && head_w_exp && maps, "conv_transpose4x4s2_head_f16: null pointer");
    DREAM_REQUIRE(B >= 1 && H >= 1 && W >= 1, "conv_transpose4x4s2_head_f16: empty input %d x %d x %d", B, H, W);
    // (the head's plane as the packer pads it, [KPad][Cmid] with KPad a multiple of 32: its first 32 rows are the tile that is read)
    DREAM_REQUIRE(head_shape_ok(Cin, Cmid, K) && CmidPad == kHeadBN && KPad >= kHeadKPad && KPad % kHeadKPad == 0,
                  "conv_transpose4x4s2_head_f16: Cin=%d (a multiple of %d), Cmid=%d / CmidPad=%d (both %d), K=%d (1 .. %d), KPad=%d (a multiple of %d)",
                  Cin, KC, Cmid, CmidPad, kHeadBN, K, kHeadKPad, KPad, kHeadKPad);
    DREAM_REQUIRE((flags & ~kHeadFlagsOk) == 0, "conv_transpose4x4s2_head_f16: unsupported flags %d (only the ReLU flag)", flags & ~kHeadFlagsOk);
    DREAM_REQUIRE((((size_t)x | (size_t)w | (size_t)head_w) & 15) == 0 && ((size_t)maps & 3) == 0,
                  "conv_transpose4x4s2_head_f16: half tensors must be 16-byte aligned");
    void (*const kernel)(const Conv16Params, const Head16Params) = convT4_head_f16_kernel<2, 2, 2, 4, kHeadNPM, true>;
    Head16Params h;
    h.w = (const _Float16 *)head_w; h.w_exp = head_w_exp; h.bias = head_bias; h.maps = maps; h.K = K;
    return for_convT4_phases(H, W, Cin, CmidPad, [&](const Geom16 &g, size_t off) {
        Conv16Params p;
        p.x = (const float *)x; p.w_hi = (const _Float16 *)w + off; p.w_lo = nullptr; p.w_exp = w_exp; p.amax_in = nullptr;
        p.scale = scale; p.shift = shift; p.residual = nullptr; p.y = nullptr; p.amax_out = peak;
        p.B = B;
        p.Cin = Cin; p.Cout = Cmid; p.CoutPad = CmidPad;
        fill_params16(p, g, kHeadBM, kHeadNPM, flags);
        DREAM_REQUIRE(p.PH * p.PW <= kHeadNPM && p.TH * p.TW <= kHeadBM, "conv_transpose4x4s2_head_f16: tile %d x %d does not fit", p.TH, p.TW);
        const size_t loop = ((size_t)2 * p.PH * p.PW + (size_t)2 * kHeadBN) * S16 * sizeof(_Float16);
        const size_t head = (size_t)(kHeadBM + K) * (kHeadBN + 8) * sizeof(_Float16);         // (staging + K rows of the head's plane)
        const size_t lds = loop > head ? loop : head;
        DREAM_REQUIRE(lds <= 160 * 1024, "LDS request %zu too large", lds);
        if (dream_allow_full_lds((const void *)kernel)) return 2;
        const dim3 grid((unsigned)(ceil_div((int)((size_t)B * p.tiles_x * p.tiles_y), 8) * 8), 1, 1);
        hipLaunchKernelGGL(kernel, grid, dim3(kHeadThreads), lds, (hipStream_t)stream, p, h);
        DREAM_LAUNCH_OK();
        return 0;
    });
}
