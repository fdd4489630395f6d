// Half-precision ("fp16") implicit-GEMM convolution: fp32 in, fp32 out, fp16 operands with fp32 accumulation on the fp16 matrix
// cores:   y = epilogue( 2^-(ea+ew) * sum fp16(x * 2^ea) * fp16(w * 2^ew) ),   one v_mfma_f32_32x32x16_f16 per 16 k's.
// The power-of-two scales are those of the split kernel (conv_f16x3.hip): 2^ea puts max|x| (amax side channel of the producing
// kernel) into [2^13, 2^14), 2^ew the weight maximum; the weight plane IS the `hi` plane that dream_pack_conv_weight_f16x3 /
// dream_pack_convT4x4_weight_f16x3 write.  Activations stay fp32 in HBM and are rounded once, while the patch is staged into LDS.
// A product of two halfs is exact in fp32, so the result differs from an exact conv of the rounded operands only by the fp32
// accumulation; what the mode costs is the operand rounding (2^-11 relative per operand).  Tiling, tap tables, fused upsample /
// sub-pixel phases and the epilogue are the split kernel's (conv_f16_common.h, conv_f16_epilogue.inc; same reference call sites:
// dream/models.py:594-615, 695-747).
//
// A stage (one tap x 32 channels) is MR*NR*2 MFMAs = 256 cycles on the 2x2 register block -- a third of the split kernel's -- so what
// the MFMAs used to hide shows: the fp32 patch loads, their conversion and the barriers.  Two loops, chosen per layer by measurement
// (launch_f16):
//   SB  the split kernel's loop without its `lo` lines: one patch buffer, fetched one stage ahead, two barriers at a chunk change;
//   DB  the patch double-buffered in the LDS the `lo` planes occupied: the next 32-channel patch is written into the other buffer
//       during the last tap of the current one, so a channel-chunk change costs no barrier of its own (one per stage, always), and
//       its fp32 loads are issued at the FIRST tap of the current chunk and converted at its last (ntaps stages of cover, not one).
// Per 16 k's a wave reads MR + NR 16-byte fragments for MR*NR MFMAs: one ds_read_b128 per MFMA on the 2x2 block.
#include "conv_f16_common.h"

namespace {

// ---- the forms of the kernel ---------------------------------------------------------------------------------------------------------
// One kernel text (conv_f16_body.inc, conv_f16_epilogue.inc), ten kernels per tile: each form is a kernel of its own from the same
// text, so that adding one leaves the machine code of the measured ones as it is (tools/isa_same.py).  This table is the
// one place that says what a form is: the six constants the body and the epilogue read, and what launch_f16 accepts with it.
//   plain          fp32 x (scaled by its amax while staged), fp32 y: precision="fp16"
//   mask           + the DREAM_CONV_RELUMASK epilogue, y = residual > 0 ? conv : 0 -- the data gradient of a conv behind a ReLU
//                  (train_precision="fp16")
//   act16          x and an NHWC y are IEEE halfs (activation_storage="fp16"): the stored half IS the MFMA operand -- the patch is copied
//                  into LDS in 16-byte pieces of 8 halfs (no v_cvt, no multiply), 2^-ew is the whole output scale, amax_in is not read;
//                  the epilogue saturates, rounds and stores halfs (the NCHW output stays fp32)
//   mask16         mask with the mask tensor stored as IEEE half (train_activation_storage="fp16")
//   ksplit         act16 on slice blockIdx.z of the gridDim.z slices of the Cin/32 x taps stages (conv_ksplit="auto"):
//                  the raw fp32 accumulator tile goes to p.y = workspace[slice] (NHWC fp32), no atomics -- conv_f16_ksplit_finish_kernel
//                  sums the slices in a fixed order.  Plain stride-1 convs only (no pool, upsample, NCHW)
//   g16 ...        data gradients stored as IEEE half (train_gradient_storage="fp16"): every data gradient of the
//                  encoder's half run lives in HBM as half(clamp(g * 2^e_g)), e_g = grad_scale_exponent(*p.grad_amax) -- one exponent per
//                  backward pass, derived by every launch from the loss gradient's amax (half_scale.h).  The chain is linear, so the
//                  factor travels: GRAD16 = 1 "entry" (the boundary conv: fp32 g in, scaled by its own amax as the plain form does;
//                  y * 2^e_g stored as half), 2 "interior" (half g in and out: act16's loader and saturating store, no scale), 3 "exit"
//                  (half g in, y * 2^-e_g stored as fp32, amax_out after the mask).  The mask, where there is one, is a half tensor; the
//                  unmasked interior form is act16 itself.  amax_out of the half-writing forms: max|y * 2^e_g| of what is stored, before
//                  the saturation.
//   act16 + residual   act16 with a half residual of the output's shape (ResnetSimple's inference_activation_storage="fp16": a Bottleneck's
//                  conv3): v = acc * (2^-ew * scale) + shift + float(residual), ReLU, max|v| into the peak scalar, sat_half.
//                  The residual is read as the pair of halfs the lane stores (4-byte aligned).  Stride-1 NHWC convs only (no pool,
//                  upsample, NCHW)
//   convT4 dgrad   the data gradient of ConvTranspose2d(k4,s2,p1) (ResnetSimple's train_decoder_precision="fp16"): plain's
//                  operands and epilogue over the H x W grid of dx, x = dz [B,2H,2W,Cin].  By sub-pixel phase (a, b) of dz it is four 2x2-tap
//                  stride-1 convs whose sum is dx; ONE launch runs them into the same accumulators: the contraction is (32-channel chunk,
//                  phase, tap), and the patch of a (chunk, phase) is gathered with position stride 2 -- dz[2 (y0 - a + py) + a][2 (x0 - b + px)
//                  + b], (TH + 1) x (TW + 1) positions of 32 contiguous channels each.  Tap (dy, dx) of phase (a, b) multiplies slice
//                  4 (2 dy + 1 - a) + 2 dx + 1 - b of the 16-slice plane [ky kx][CoutPad][Cin]: 16 tap products per output, no structural zeros
//   plain, sat     plain for an operand that carries no amax (the forward of the same switch): e_a = 0, amax_in is not read, and the one rounding
//                  saturates -- half(clamp(x, +-65504)), the activation rule of 4.8j -- so an outlier stays finite
enum Form16 { kPlain, kMask, kAct16, kMask16, kKsplit, kG16Entry, kG16EntryMask, kG16Interior, kG16Exit, kRes16, kConvT4Dgrad, kPlainSat, kNumForms };

// the flags whose launches are never split (conv_ksplit: the large-map layers and the K-channel output)
constexpr int kKsplitRefused = DREAM_CONV_POOL2 | DREAM_CONV_UPSAMPLE2X | DREAM_CONV_ZEROSTUFF2X | DREAM_CONV_OUT_NCHW | DREAM_CONV_RELUMASK;
// ... and those the residual form does not take
constexpr int kRes16Refused = kKsplitRefused | DREAM_CONV_RES_AFTER_RELU;

struct Form16Row {
    const char *name;
    bool EPI_MASK, ACT16, MASK16, KSPLIT;     // the kernel's constants
    int GRAD16;
    bool RES16;
    bool DGT4;                                // the convT4 dgrad loader (conv_f16_body.inc)
    bool SAT0;                                // fp32 x rounded unscaled and saturated: amax_in is not read
    bool affine;                              // launch_f16: scale / shift may be given
    bool residual;                            //             `residual` may be a true residual (a form with EPI_MASK: it IS the mask)
    int flags_ok;                             //             the flag bits the form accepts
    // what follows from the constants: x is half (16-byte aligned, amax_in unused); an NHWC y is half; grad_amax is read
    constexpr bool x16() const { return ACT16; }
    constexpr bool y16() const { return GRAD16 == 0 ? ACT16 : GRAD16 != 3; }
    constexpr bool needs_grad_amax() const { return GRAD16 == 1 || GRAD16 == 3; }
};
constexpr Form16Row kForms[kNumForms] = {
    //  name                EPI_MASK ACT16  MASK16 KSPLIT GRAD16 RES16  DGT4   SAT0   affine residual flags_ok
    {"plain",               false,   false, false, false, 0,     false, false, false, true,  true,    ~DREAM_CONV_RELUMASK},
    {"mask",                true,    false, false, false, 0,     false, false, false, true,  false,   ~0},
    {"act16",               false,   true,  false, false, 0,     false, false, false, true,  false,   ~DREAM_CONV_RELUMASK},
    {"mask16",              true,    false, true,  false, 0,     false, false, false, true,  false,   ~0},
    {"ksplit",              false,   true,  false, true,  0,     false, false, false, false, false,   ~kKsplitRefused},
    {"g16 entry",           false,   false, false, false, 1,     false, false, false, false, false,   0},
    {"g16 entry + mask",    true,    false, true,  false, 1,     false, false, false, false, false,   DREAM_CONV_RELUMASK},
    {"g16 interior",        true,    true,  true,  false, 2,     false, false, false, false, false,   DREAM_CONV_RELUMASK},
    {"g16 exit",            true,    true,  true,  false, 3,     false, false, false, false, false,   DREAM_CONV_RELUMASK},
    {"act16 + residual",    false,   true,  false, false, 0,     true,  false, false, true,  true,    ~kRes16Refused},
    {"convT4 dgrad",        false,   false, false, false, 0,     false, true, false,  false, false,   0},
    {"plain, saturating",   false,   false, false, false, 0,     false, false, true,  true,  false,   ~DREAM_CONV_RELUMASK},
};

template <int FORM, int MR, int NR, int WM, int WN, int NPM, bool DB, bool PRIO = false>
__global__ void __launch_bounds__(64 * WM * WN, 2) conv_f16_kernel(const Conv16Params p) {
    constexpr bool EPI_MASK = kForms[FORM].EPI_MASK;
    constexpr bool ACT16 = kForms[FORM].ACT16;
    constexpr bool MASK16 = kForms[FORM].MASK16;
    constexpr bool KSPLIT = kForms[FORM].KSPLIT;
    constexpr int GRAD16 = kForms[FORM].GRAD16;
    constexpr bool RES16 = kForms[FORM].RES16;
    constexpr bool DGT4 = kForms[FORM].DGT4;
    constexpr bool SAT0 = kForms[FORM].SAT0;
#include "conv_f16_body.inc"
}

// y = half(sat(epilogue(sum_s workspace[s]))): the partial sums of the S slices added in slice order 0 .. S-1 (fp32; two runs give the
// same bits), then the expression of conv_f16_epilogue.inc -- v * (2^-ew * scale) + shift, ReLU --, max|v| before the saturation into
// the peak scalar, sat_half, half NHWC.  Elementwise over the flattened tensor, 8 consecutive elements (channels) per lane: two
// 16-byte loads per slice, one 16-byte store; `slice` = round_up(n, 8) floats.
__global__ void __launch_bounds__(256) conv_f16_ksplit_finish_kernel(const float *ws, size_t slice, int S, const int *w_exp,
                                                                     const float *scale, const float *shift, _Float16 *y, size_t n,
                                                                     int Cout, int relu, unsigned *amax) {
    const int e = -*w_exp;
    const float inv = pow2f(e < -126 ? -126 : (e > 127 ? 127 : e));
    const size_t n8 = (n + 7) / 8;
    float m = 0.f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (size_t)gridDim.x * 256) {
        f32x4 lo = *(const f32x4 *)(ws + i * 8), hi = *(const f32x4 *)(ws + i * 8 + 4);
        for (int s = 1; s < S; ++s) {
            const float *q = ws + (size_t)s * slice + i * 8;
            lo += *(const f32x4 *)q;
            hi += *(const f32x4 *)(q + 4);
        }
        int c = (int)((i * 8) % (size_t)Cout);
        f16x8 o;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float v = (k < 4 ? lo[k & 3] : hi[k & 3]) * (inv * (scale != nullptr ? scale[c] : 1.0f)) + (shift != nullptr ? shift[c] : 0.0f);
            if (relu) v = fmaxf(v, 0.0f);
            if (i * 8 + k < n) m = fmaxf(m, fabsf(v));
            o[k] = sat_half(v);
            if (++c == Cout) c = 0;
        }
        if (i * 8 + 8 <= n) {
            *(f16x8 *)(y + i * 8) = o;
        } else {
            for (int k = 0; i * 8 + k < n; ++k) y[i * 8 + k] = o[k];
        }
    }
    if (amax) publish_amax(amax, m);
}

// The finishing pass of the split ConvTranspose2d(k4,s2,p1) (inference_conv_ksplit="auto"): elementwise over the OUTPUT
// [B, 2H, 2W, Cout], 8 consecutive channels of one output pixel per lane (Cout % 8 == 0).  Output pixel (oy, ox) belongs to sub-pixel
// phase ph = 2 (oy & 1) + (ox & 1) at position (oy >> 1, ox >> 1); the S partial tiles of phase ph lie at ws + (ph * S + s) * slice, each
// [B, H, W, Cout] fp32 (slice = B H W Cout floats).  Added in slice order 0 .. S-1 (fp32; no atomics: two runs give the same bits), then
// the IEEE operations of conv_f16_ksplit_finish_kernel: v * (2^-ew * scale) + shift, ReLU, max|v| before the saturation into the peak
// scalar, sat_half.  Two 16-byte loads per slice, one 16-byte store.
__global__ void __launch_bounds__(256) convT4_f16_ksplit_finish_kernel(const float *ws, size_t slice, int S, const int *w_exp,
                                                                       const float *scale, const float *shift, _Float16 *y, int B, int H,
                                                                       int W, int Cout, int relu, unsigned *amax) {
    const int e = -*w_exp;
    const float inv = pow2f(e < -126 ? -126 : (e > 127 ? 127 : e));
    const int c8n = Cout / 8, Wo = 2 * W, Ho = 2 * H;
    const size_t n8 = (size_t)B * Ho * Wo * c8n;
    float m = 0.f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (size_t)gridDim.x * 256) {
        const size_t pix = i / (size_t)c8n;
        const int c0 = (int)(i - pix * c8n) * 8;
        const int ox = (int)(pix % (size_t)Wo);
        const size_t row = pix / (size_t)Wo;
        const int oy = (int)(row % (size_t)Ho);
        const size_t b = row / (size_t)Ho;
        const int ph = 2 * (oy & 1) + (ox & 1);
        const float *q = ws + (size_t)ph * S * slice + ((b * H + (oy >> 1)) * W + (ox >> 1)) * (size_t)Cout + c0;
        f32x4 lo = *(const f32x4 *)q, hi = *(const f32x4 *)(q + 4);
        for (int s = 1; s < S; ++s) {
            q += slice;
            lo += *(const f32x4 *)q;
            hi += *(const f32x4 *)(q + 4);
        }
        f16x8 o;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int c = c0 + k;
            float v = (k < 4 ? lo[k & 3] : hi[k & 3]) * (inv * (scale != nullptr ? scale[c] : 1.0f)) + (shift != nullptr ? shift[c] : 0.0f);
            if (relu) v = fmaxf(v, 0.0f);
            m = fmaxf(m, fabsf(v));
            o[k] = sat_half(v);
        }
        *(f16x8 *)(y + i * 8) = o;
    }
    if (amax) publish_amax(amax, m);
}

struct Variant16h {
    const char *name;
    int BM, BN, NP_MAX, threads, abufs;
    void (*kernel[kNumForms])(const Conv16Params);
};
#define F16_KERNELS(...) /* in the order of Form16 */ \
    {conv_f16_kernel<kPlain, __VA_ARGS__>, conv_f16_kernel<kMask, __VA_ARGS__>, conv_f16_kernel<kAct16, __VA_ARGS__>, \
     conv_f16_kernel<kMask16, __VA_ARGS__>, conv_f16_kernel<kKsplit, __VA_ARGS__>, conv_f16_kernel<kG16Entry, __VA_ARGS__>, \
     conv_f16_kernel<kG16EntryMask, __VA_ARGS__>, conv_f16_kernel<kG16Interior, __VA_ARGS__>, conv_f16_kernel<kG16Exit, __VA_ARGS__>, \
     conv_f16_kernel<kRes16, __VA_ARGS__>, conv_f16_kernel<kConvT4Dgrad, __VA_ARGS__>, conv_f16_kernel<kPlainSat, __VA_ARGS__>}
// Tile shapes are the split kernel's; "db" / "sb": double- / single-buffered patch.
const Variant16h kVariantsF16[] = {
    {"f16 m2n2w2x2 db", 128, 128, 192, 256, 2, F16_KERNELS(2, 2, 2, 2, 192, true)},
    {"f16 m2n2w4x1 db", 256, 64, 352, 256, 2, F16_KERNELS(2, 2, 4, 1, 352, true)},
    {"f16 m2n1w4x1 db", 256, 32, 352, 256, 2, F16_KERNELS(2, 1, 4, 1, 352, true)},
    {"f16 m1n2w2x2 db", 64, 128, 128, 256, 2, F16_KERNELS(1, 2, 2, 2, 128, true)},
    {"f16 m2n2w4x2 db", 256, 128, 352, 512, 2, F16_KERNELS(2, 2, 4, 2, 352, true)},             // 8 waves
    {"f16 m2n2w4x1 sb", 256, 64, 352, 256, 1, F16_KERNELS(2, 2, 4, 1, 352, false)},            // the split kernel's loop: 64-channel 3x3 convs
    {"f16 m2n2w4x2 sb", 256, 128, 352, 512, 1, F16_KERNELS(2, 2, 4, 2, 352, false)},
    {"f16 m2n2w4x2 db prio", 256, 128, 352, 512, 2, F16_KERNELS(2, 2, 4, 2, 352, true, true)},  // A/B arm: s_setprio around the MFMAs
};
constexpr int kNumF16 = 8;
int g_forced_f16 = -1;
thread_local int g_forced_ksplit = -1;

// the tile of a launch of `pixels` positions
int variant_f16(long pixels, int Cin, int Cout, int ntaps) {
    // the variant rule, measured per layer at 128 frames (profiles/r07_ab_f16_variants.txt): from 128 output channels on
    // the 128 x 128 tile wins by 5-12 % (160 VGPRs and 51 KB of LDS: three workgroups per CU; the 256-px tiles hold two); a 64-channel
    // 3x3 conv is 3 % faster on the single-buffered 256 x 64 tile, a 64-channel 1x1 conv (a chunk change per stage) 15 % on the
    // double-buffered one
    int v = Cout <= 32 ? 2 : (Cout <= 64 ? (ntaps == 1 ? 1 : 5) : 0);
    // tiny grids: 64-px tiles -- unless the launch is deep (the first decoder conv: 4 taps x 2048 channels on 13 x 13 maps), where the
    // weight tile is what a workgroup streams and the 256-px tile re-reads it a quarter as often (0.645 against 0.780 ms)
    if (Cout > 64 && ((pixels + 255) / 256) * ceil_div(Cout, 64) < 512) v = (long)Cin * ntaps >= 4096 ? 1 : 3;
    return g_forced_f16 >= 0 ? g_forced_f16 : v;
}

// conv_ksplit (the flags whose launches are never split: kKsplitRefused above): the workgroups a split launch may reach, the fewest
// stages a slice is left with, the most slices.  Measured per layer at 1 .. 16 frames
// (profiles/ab_f16_ksplit.txt): a split pays where the unsplit grid is at most ~190 workgroups AND the contraction is
// long -- 512->512 at 25 x 25, one frame: 0.071 -> 0.028 ms with 8 slices; at 50 x 50: 0.072 -> 0.041 with 4 --; from ~310 workgroups
// on every split lost, and so did slices of 9 .. 18 stages (a 128->128 conv of 36 stages at 157 workgroups: 0.022 -> 0.025 ms in two
// slices: the finishing pass costs what the halved workgroups save)
constexpr int kKsplitTargetWorkgroups = 384;
constexpr int kKsplitMinStages = 24;
constexpr int kKsplitMax = 16;

// The rule is one body over a table of these three (ksplit_slices below).  The hourglass's table is the three constants above; ResnetSimple's
// walk (inference_conv_ksplit="auto": its 1x1 / 3x3 / gathered convs without a residual and the sub-pixel phases of its 4x4 transposed
// convs) has a table of its own, measured per layer on its own shapes (profiles/ab_resnet_ksplit.txt)
// ... plus one stated condition: a launch of fewer than short_stages stages counts against short_target_workgroups instead (0: none).
// ResnetSimple's numbers (per launch, 1 .. 128 frames): contractions of 64 stages and more win in 2 .. 16 slices up to ~130 unsplit
// workgroups (the first decoder stage, 256 stages on 4 workgroups a phase and frame: 0.527 -> 0.088 ms in 16 slices at one frame, 0.531 ->
// 0.317 in 2 at 32 frames) and down to 16 stages a slice; from ~190 workgroups on every split tied or lost.  The 32- and 36-stage
// launches (layer3's 1024->256, a 256->256 decoder stage on 26 x 26) win in 2 slices up to ~50 workgroups and tie at 80 .. 96, hence the
// condition; slices of 8 stages lost everywhere (the 16- and 18-stage launches are never split)
struct KsplitRule { int target_workgroups, min_stages, max_slices, short_stages, short_target_workgroups; };
constexpr KsplitRule kKsplitHourglass = {kKsplitTargetWorkgroups, kKsplitMinStages, kKsplitMax, 0, 0};
constexpr KsplitRule kKsplitResnet = {256, 16, 16, 64, 128};

// One launch of `form` (kForms).  `residual`: the true residual or, with DREAM_CONV_RELUMASK, the mask (fp32 or half, as the form
// says); ksplit: the slices of the ksplit form, y = the fp32 workspace (dream_conv2d_f16_ksplit_nhwc_f16); grad_amax: the scalar the g16
// entry / exit forms derive e_g from
int launch_f16(Form16 form, const void *x, const unsigned *amax_in, const void *w, const int *w_exp, const float *scale,
               const float *shift, const void *residual, void *y, unsigned *amax_out, int B, int Cin, int Cout, int CoutPad,
               const Geom16 &g, int flags, void *stream, int ksplit = 0, const unsigned *grad_amax = nullptr) {
    const Form16Row &f = kForms[form];
    DREAM_REQUIRE(x && (amax_in || f.x16() || f.SAT0) && w && w_exp && y, "conv_f16: null pointer");
    DREAM_REQUIRE((flags & ~f.flags_ok) == 0, "conv_f16: the %s form does not take flags %d", f.name, flags & ~f.flags_ok);
    DREAM_REQUIRE(f.affine || (scale == nullptr && shift == nullptr), "conv_f16: the %s form takes no scale / shift", f.name);
    DREAM_REQUIRE(f.EPI_MASK || f.residual || residual == nullptr, "conv_f16: the %s form takes no residual", f.name);
    DREAM_REQUIRE(!(f.x16() || f.y16()) || ((((size_t)x | (size_t)y) & 15) == 0), "conv_f16: half tensors must be 16-byte aligned");
    DREAM_REQUIRE(!(f.GRAD16 && f.MASK16) || ((size_t)residual & 3) == 0, "conv_f16: the half mask of the %s form must be 4-byte aligned", f.name);
    DREAM_REQUIRE(!f.RES16 || (residual != nullptr && ((size_t)residual & 3) == 0), "conv_f16: the %s form needs its half residual, 4-byte aligned", f.name);
    DREAM_REQUIRE(!f.needs_grad_amax() || grad_amax != nullptr, "conv_f16: the %s form needs the loss gradient's amax", f.name);
    DREAM_REQUIRE(Cin % KC == 0, "conv_f16: Cin=%d must be a multiple of %d", Cin, KC);
    Conv16Params p;
    p.x = (const float *)x; p.w_hi = (const _Float16 *)w; p.w_lo = nullptr; p.w_exp = w_exp; p.amax_in = amax_in;
    p.scale = scale; p.shift = shift; p.residual = (const float *)residual; p.y = (float *)y; p.amax_out = amax_out;
    p.B = B;
    p.Cin = Cin; p.Cout = Cout; p.CoutPad = CoutPad;
    const long pixels = (long)B * g.H * g.W;
    const int v = variant_f16(pixels, Cin, Cout, g.ntaps);
    const Variant16h &var = kVariantsF16[v];
    DREAM_REQUIRE(CoutPad % var.BN == 0 && CoutPad >= Cout, "CoutPad=%d must be a multiple of %d", CoutPad, var.BN);
    const bool pool = (flags & DREAM_CONV_POOL2) != 0;
    DREAM_REQUIRE(!pool || (!(flags & DREAM_CONV_OUT_NCHW) && residual == nullptr && g.H >= 2 && g.W >= 2 && g.out_scale == 1),
                  "fused max-pool: NHWC output, no residual");
    const bool mask = (flags & DREAM_CONV_RELUMASK) != 0;
    DREAM_REQUIRE(!mask || (residual != nullptr && !pool && !(flags & (DREAM_CONV_OUT_NCHW | DREAM_CONV_RES_AFTER_RELU)) && g.out_scale == 1),
                  "ReLU mask: needs the mask tensor (residual), NHWC output, no pool");
    DREAM_REQUIRE(!f.EPI_MASK || mask, "conv_f16: the %s form goes with DREAM_CONV_RELUMASK", f.name);
    DREAM_REQUIRE(f.KSPLIT ? ksplit >= 1 && ksplit <= 1024 : ksplit == 0, "conv_f16: a split launch is the ksplit form in 1 .. 1024 slices");
    // (the ksplit form stores position coordinates [B, p.H, p.W, Cout] and never reads out_scale: a sub-pixel phase runs as it is)
    DREAM_REQUIRE(!f.GRAD16 || g.out_scale == 1, "conv_f16: the %s form is a plain conv", f.name);
    if (f.GRAD16) p.grad_amax = grad_amax;         // (shares w_lo's slot, which these kernels do not read)
    void (*const kernel)(const Conv16Params) = var.kernel[form];
    fill_params16(p, g, var.BM, var.NP_MAX, flags);
    DREAM_REQUIRE(p.PH * p.PW <= var.NP_MAX, "conv_f16: patch of %d pixels exceeds the variant's %d", p.PH * p.PW, var.NP_MAX);
    const size_t lds = ((size_t)var.abufs * p.PH * p.PW + (size_t)2 * var.BN) * S16 * sizeof(_Float16);
    DREAM_REQUIRE(lds <= 160 * 1024, "LDS request %zu too large", lds);
    if (dream_allow_full_lds((const void *)kernel)) return 2;
    const dim3 grid((unsigned)(ceil_div((int)((size_t)B * p.tiles_x * p.tiles_y), 8) * 8), (unsigned)ceil_div(Cout, var.BN),
                    (unsigned)(ksplit ? ksplit : 1));
    hipLaunchKernelGGL(kernel, grid, dim3(var.threads), lds, (hipStream_t)stream, p);
    DREAM_LAUNCH_OK();
    return 0;
}

// what the k x k entry points require of their shape arguments
int check_conv2d_f16(int H, int W, int ksize, int stride, int flags) {
    DREAM_REQUIRE(ksize == 1 || ksize == 3, "conv2d_f16: kernel size %d not supported", ksize);
    DREAM_REQUIRE(stride == 1, "conv2d_f16: stride %d not supported (strided convs stay on the fp32 kernel)", stride);
    DREAM_REQUIRE(!(flags & DREAM_CONV_UPSAMPLE2X) || (H % 2 == 0 && W % 2 == 0), "fused x2 upsample needs even H, W");
    return 0;
}

// the two transposed convs by their sub-pixel phases, on fp32 (kPlain) or half (kAct16: amax_in null) activations
int convT4_f16(Form16 form, const void *x, const unsigned *amax_in, const void *w, const int *w_exp, const float *scale,
               const float *shift, void *y, unsigned *amax_out, int B, int H, int W, int Cin, int Cout, int CoutPad, int flags,
               void *stream) {
    DREAM_REQUIRE((flags & (DREAM_CONV_UPSAMPLE2X | DREAM_CONV_ZEROSTUFF2X | DREAM_CONV_OUT_NCHW | DREAM_CONV_POOL2)) == 0,
                  "convT4x4_f16: unsupported flags");
    return for_convT4_phases(H, W, Cin, CoutPad, [&](const Geom16 &g, size_t off) {
        return launch_f16(form, x, amax_in, (const _Float16 *)w + off, w_exp, scale, shift, nullptr, y, amax_out, B, Cin, Cout, CoutPad, g,
                          flags, stream);
    });
}

int convT3_f16(Form16 form, const void *x, const unsigned *amax_in, const void *w, const int *w_exp, const float *bias, void *y,
               unsigned *amax_out, int B, int H, int W, int Cin, int Cout, int CoutPad, int flags, void *stream) {
    DREAM_REQUIRE((flags & ~DREAM_CONV_RELU) == 0, "convT3x3_f16: only the ReLU flag is supported");
    return for_convT3_phases(H, W, [&](const Geom16 &g) {
        return launch_f16(form, x, amax_in, w, w_exp, nullptr, bias, nullptr, y, amax_out, B, Cin, Cout, CoutPad, g, flags, stream);
    });
}

}  // namespace

extern "C" int dream_conv_f16_set_variant(int v) {
    DREAM_REQUIRE(v >= -1 && v < kNumF16, "variant out of range");
    g_forced_f16 = v;
    return 0;
}

// k x k (1 | 3) stride-1 conv, same contract as dream_conv2d_f16x3_nhwc_f32 without the `lo` plane.  Cin % 32 == 0.
extern "C" int dream_conv2d_f16_nhwc_f32(const float *x, const unsigned *amax_in, const void *w, const int *w_exp,
                                         const float *scale, const float *shift, const float *residual, float *y,
                                         unsigned *amax_out, int B, int H, int W, int Cin, int Cout, int CoutPad, int ksize,
                                         int stride, int flags, void *stream) {
    if (int rc = check_conv2d_f16(H, W, ksize, stride, flags)) return rc;
    const Geom16 g = geom16_conv(H, W, ksize, flags);
    return launch_f16((flags & DREAM_CONV_RELUMASK) ? kMask : kPlain, x, amax_in, w, w_exp, scale, shift, residual, y, amax_out, B, Cin,
                      Cout, CoutPad, g, flags, stream);
}

// dream_conv2d_f16_nhwc_f32 with DREAM_CONV_RELUMASK (set here) and the mask stored as IEEE half (train_activation_storage="fp16"):
// y = mask > 0 ? conv : 0, fp32 NHWC; amax_out = max|y| after the mask.  mask [B,H,W,Cout] half.
extern "C" int dream_conv2d_f16_mask16_nhwc_f32(const float *x, const unsigned *amax_in, const void *w, const int *w_exp,
                                                const float *scale, const float *shift, const void *mask, float *y,
                                                unsigned *amax_out, int B, int H, int W, int Cin, int Cout, int CoutPad, int ksize,
                                                int stride, int flags, void *stream) {
    if (int rc = check_conv2d_f16(H, W, ksize, stride, flags)) return rc;
    DREAM_REQUIRE(mask != nullptr && !(flags & DREAM_CONV_UPSAMPLE2X), "conv2d_f16_mask16: needs the mask, takes no upsample");
    flags |= DREAM_CONV_RELUMASK;
    const Geom16 g = geom16_conv(H, W, ksize, flags);
    return launch_f16(kMask16, x, amax_in, w, w_exp, scale, shift, mask, y, amax_out, B, Cin, Cout, CoutPad, g, flags, stream);
}

// ConvTranspose2d(k=4,s=2,p=1) on the fp16 path: the four 2x2-tap sub-pixel phases of dream_conv_transpose4x4s2_f16x3_nhwc_f32.
extern "C" int dream_conv_transpose4x4s2_f16_nhwc_f32(const float *x, const unsigned *amax_in, const void *w, const int *w_exp,
                                                      const float *scale, const float *shift, float *y, unsigned *amax_out,
                                                      int B, int H, int W, int Cin, int Cout, int CoutPad, int flags,
                                                      void *stream) {
    return convT4_f16(kPlain, x, amax_in, w, w_exp, scale, shift, y, amax_out, B, H, W, Cin, Cout, CoutPad, flags, stream);
}

// ... for an activation without an amax (ResnetSimple's train_decoder_precision="fp16"): x rounded as half(clamp(x, +-65504)),
// e_x = 0 -- the saturating plain form; everything else as above.
extern "C" int dream_conv_transpose4x4s2_f16_sat_nhwc_f32(const float *x, const void *w, const int *w_exp, const float *scale,
                                                          const float *shift, float *y, int B, int H, int W, int Cin, int Cout, int CoutPad,
                                                          int flags, void *stream) {
    return convT4_f16(kPlainSat, x, nullptr, w, w_exp, scale, shift, y, nullptr, B, H, W, Cin, Cout, CoutPad, flags, stream);
}

// ConvTranspose2d(k=3,s=2,p=1,output_padding 1) on the fp16 path: the phases of dream_conv_transpose3x3s2_f16x3_nhwc_f32.
extern "C" int dream_conv_transpose3x3s2_f16_nhwc_f32(const float *x, const unsigned *amax_in, const void *w, const int *w_exp,
                                                      const float *bias, float *y, unsigned *amax_out, int B, int H, int W,
                                                      int Cin, int Cout, int CoutPad, int flags, void *stream) {
    return convT3_f16(kPlain, x, amax_in, w, w_exp, bias, y, amax_out, B, H, W, Cin, Cout, CoutPad, flags, stream);
}

// ---- ResnetSimple's train_decoder_precision="fp16" (DESIGN.md 4.8n): the data gradient of ConvTranspose2d(k4,s2,p1) -- the 4x4 stride-2
// pad-1 conv of dz (dream/models.py:37-136: the decoder stages, reached from loss.backward()) -- in ONE launch of the convT4 dgrad form ----
namespace {

// the H x W grid of dx; a (TH + 1) x (TW + 1) patch of one sub-pixel phase of dz and its 2 x 2 taps
Geom16 geom16_convT4_dgrad(int H, int W) {
    Geom16 g;
    g.H = H; g.W = W; g.Hin = H; g.Win = W; g.Hs = 2 * H; g.Ws = 2 * W; g.Ho = H; g.Wo = W;
    g.pad = 0; g.kext = 2; g.ntaps = 4;
    for (int t = 0; t < 4; ++t) { g.tap_dy[t] = t >> 1; g.tap_dx[t] = t & 1; }
    g.out_scale = 1; g.out_oy = 0; g.out_ox = 0;
    return g;
}

}  // namespace

// dz [B,Ho,Wo,Cdz] fp32 (Ho, Wo even), amax_dz: device scalar, bit pattern of (an upper bound of) max|dz| -> dx [B,Ho/2,Wo/2,Cdx] fp32:
//   dx[b,i,j,ci] = 2^-(eg+ew) sum_{ty,tx in 0..3} sum_co fp16(dz 2^eg)[b,2i+ty-1,2j+tx-1,co] * w[4 ty + tx][ci][co],   zero outside the map,
// w: halfs [16][CdxPad][Cdz] of wT[ci][co][ty][tx] * 2^ew (dream_pack_conv_weight_f16x3's `hi` plane of the [Cdx,Cdz,4,4] tensor, mode 0),
// w_exp: its exponent.  Cdz % 32 == 0; dz and w 16-byte aligned; flags must be 0.
extern "C" int dream_conv_transpose4x4s2_dgrad_f16_nhwc_f32(const float *dz, const unsigned *amax_dz, const void *w, const int *w_exp,
                                                            float *dx, int B, int Ho, int Wo, int Cdz, int Cdx, int CdxPad, int flags,
                                                            void *stream) {
    DREAM_REQUIRE(flags == 0, "conv_transpose4x4s2_dgrad_f16: flags %d not supported", flags);
    DREAM_REQUIRE(B >= 1 && Ho >= 2 && Wo >= 2 && Ho % 2 == 0 && Wo % 2 == 0,
                  "conv_transpose4x4s2_dgrad_f16: dz of %d x %d: the output of the transposed conv has even dimensions", Ho, Wo);
    DREAM_REQUIRE(Cdz >= KC && Cdz % KC == 0 && Cdx >= 1, "conv_transpose4x4s2_dgrad_f16: Cdz=%d must be a multiple of %d", Cdz, KC);
    DREAM_REQUIRE((size_t)Ho * Wo * (size_t)Cdz < ((size_t)1 << 31), "conv_transpose4x4s2_dgrad_f16: a frame of dz exceeds 2^31 elements");
    DREAM_REQUIRE(dz && w && dx && ((((size_t)dz | (size_t)w) & 15) == 0) && ((size_t)dx & 3) == 0,
                  "conv_transpose4x4s2_dgrad_f16: dz and w must be 16-byte aligned, dx 4-byte");
    return launch_f16(kConvT4Dgrad, dz, amax_dz, w, w_exp, nullptr, nullptr, nullptr, dx, nullptr, B, Cdz, Cdx, CdxPad,
                      geom16_convT4_dgrad(Ho / 2, Wo / 2), 0, stream);
}

// ---- activations stored as IEEE half (activation_storage="fp16") -----------------------------------------------------------------
// The siblings of the three entry points above (and of the 4x4 transposed conv an upsample + conv runs as) on half NHWC tensors:
// x [B,H,W,Cin] half, y half NHWC -- fp32 NCHW with DREAM_CONV_OUT_NCHW --, same weight plane and exponent, no amax_in.
// amax_out (optional) is NOT zeroed and may be shared by every launch of a forward pass: max|y| before the saturation.
extern "C" int dream_conv2d_f16_nhwc_f16(const void *x, const void *w, const int *w_exp, const float *scale, const float *shift,
                                         void *y, unsigned *amax_out, int B, int H, int W, int Cin, int Cout, int CoutPad,
                                         int ksize, int stride, int flags, void *stream) {
    if (int rc = check_conv2d_f16(H, W, ksize, stride, flags)) return rc;
    const Geom16 g = geom16_conv(H, W, ksize, flags);
    return launch_f16(kAct16, x, nullptr, w, w_exp, scale, shift, nullptr, y, amax_out, B, Cin, Cout, CoutPad, g, flags, stream);
}

// ... with a residual stored as half, [B,H,W,Cout], 4-byte aligned: y = half(sat(relu?(conv * scale + shift + float(residual)))), amax_out =
// max|.| before the saturation.  NHWC only: a fused pool / upsample and DREAM_CONV_OUT_NCHW are refused.
extern "C" int dream_conv2d_f16_res16_nhwc_f16(const void *x, const void *w, const int *w_exp, const float *scale, const float *shift,
                                               const void *residual, void *y, unsigned *amax_out, int B, int H, int W, int Cin, int Cout,
                                               int CoutPad, int ksize, int stride, int flags, void *stream) {
    if (int rc = check_conv2d_f16(H, W, ksize, stride, flags)) return rc;
    const Geom16 g = geom16_conv(H, W, ksize, flags);
    return launch_f16(kRes16, x, nullptr, w, w_exp, scale, shift, residual, y, amax_out, B, Cin, Cout, CoutPad, g, flags, stream);
}

extern "C" int dream_conv_transpose4x4s2_f16_nhwc_f16(const void *x, const void *w, const int *w_exp, const float *scale,
                                                      const float *shift, void *y, unsigned *amax_out, int B, int H, int W,
                                                      int Cin, int Cout, int CoutPad, int flags, void *stream) {
    return convT4_f16(kAct16, x, nullptr, w, w_exp, scale, shift, y, amax_out, B, H, W, Cin, Cout, CoutPad, flags, stream);
}

extern "C" int dream_conv_transpose3x3s2_f16_nhwc_f16(const void *x, const void *w, const int *w_exp, const float *bias, void *y,
                                                      unsigned *amax_out, int B, int H, int W, int Cin, int Cout, int CoutPad,
                                                      int flags, void *stream) {
    return convT3_f16(kAct16, x, nullptr, w, w_exp, bias, y, amax_out, B, H, W, Cin, Cout, CoutPad, flags, stream);
}

// ---- data gradients stored as IEEE half (train_gradient_storage="fp16") ------------------------------------------
// Three forms of the 3x3 stride-1 conv with the mode-1 packed plane.  grad_amax: device scalar, bit pattern of the loss gradient's
// amax; every launch of one backward derives e_g = 9 - exponent from it (0 for a zero scalar, clamped to +-100).  mask: [B,H,W,Cout]
// half or null, y = mask > 0 ? conv : 0.  peak (optional, not zeroed): max|v| of what a half-writing launch stores, before the
// saturation.  Half tensors must be 16-byte aligned.
// entry: x fp32, scaled by its own amax_in as dream_conv2d_f16_nhwc_f32 does -> y = half(clamp(conv * 2^e_g))
extern "C" int dream_conv2d_f16_g16_entry_nhwc_f16(const float *x, const unsigned *amax_in, const void *w, const int *w_exp,
                                                   const void *mask, void *y, const unsigned *grad_amax, unsigned *peak, int B, int H,
                                                   int W, int Cin, int Cout, int CoutPad, int ksize, int stride, int flags, void *stream) {
    DREAM_REQUIRE(ksize == 3 && stride == 1 && flags == 0, "conv2d_f16_g16_entry: a plain 3x3 stride-1 conv (flags 0)");
    DREAM_REQUIRE(grad_amax != nullptr, "conv2d_f16_g16_entry: needs the loss gradient's amax");
    const int fl = mask ? DREAM_CONV_RELUMASK : 0;
    const Geom16 g = geom16_conv(H, W, ksize, fl);
    return launch_f16(mask ? kG16EntryMask : kG16Entry, x, amax_in, w, w_exp, nullptr, nullptr, mask, y, peak, B, Cin, Cout, CoutPad, g, fl,
                      stream, 0, grad_amax);
}

// interior: x half (already times 2^e_g) -> y = half(clamp(conv)): no scale is read.  Without a mask this IS dream_conv2d_f16_nhwc_f16.
extern "C" int dream_conv2d_f16_g16_nhwc_f16(const void *x, const void *w, const int *w_exp, const void *mask, void *y, unsigned *peak,
                                             int B, int H, int W, int Cin, int Cout, int CoutPad, int ksize, int stride, int flags,
                                             void *stream) {
    DREAM_REQUIRE(ksize == 3 && stride == 1 && flags == 0, "conv2d_f16_g16: a plain 3x3 stride-1 conv (flags 0)");
    const Geom16 g = geom16_conv(H, W, ksize, 0);
    return launch_f16(mask ? kG16Interior : kAct16, x, nullptr, w, w_exp, nullptr, nullptr, mask, y, peak, B, Cin, Cout, CoutPad, g,
                      mask ? DREAM_CONV_RELUMASK : 0, stream);
}

// exit: x half (times 2^e_g), mask required -> y = (mask > 0 ? conv : 0) * 2^-e_g as fp32; amax_out = max|y| after the mask
extern "C" int dream_conv2d_f16_g16_exit_nhwc_f32(const void *x, const void *w, const int *w_exp, const void *mask, float *y,
                                                  const unsigned *grad_amax, unsigned *amax_out, int B, int H, int W, int Cin, int Cout,
                                                  int CoutPad, int ksize, int stride, int flags, void *stream) {
    DREAM_REQUIRE(ksize == 3 && stride == 1 && flags == 0, "conv2d_f16_g16_exit: a plain 3x3 stride-1 conv (flags 0)");
    DREAM_REQUIRE(mask != nullptr && grad_amax != nullptr, "conv2d_f16_g16_exit: needs the mask and the loss gradient's amax");
    const Geom16 g = geom16_conv(H, W, ksize, DREAM_CONV_RELUMASK);
    return launch_f16(kG16Exit, x, nullptr, w, w_exp, nullptr, nullptr, mask, y, amax_out, B, Cin, Cout, CoutPad, g, DREAM_CONV_RELUMASK,
                      stream, 0, grad_amax);
}

// ---- conv_ksplit="auto": the contraction of a small-grid conv divided over workgroups ---------------------------
extern "C" int dream_conv_f16_set_ksplit(int n) {
    DREAM_REQUIRE(n == -1 || n >= 1, "ksplit: -1 (the rule) or a slice count >= 1");
    g_forced_ksplit = n;
    return 0;
}

namespace {

// Slices of one launch of geometry g: fixed constants, no device query -- the emulator, a meta-device trace and the GPU agree.  1 wherever
// the unsplit grid already has r.target_workgroups workgroups (r.short_target_workgroups for a launch of fewer than r.short_stages
// stages); never more than r.max_slices, never fewer than r.min_stages stages a slice.
// Non-increasing in B: a tile never spans frames, and the tile of a launch with more than 64 output channels
// changes with B only where the answer is 1 on both sides (the tiny-grid rule of variant_f16 holds below 512 units of 256 px x 64
// channels; above it the 128 x 128 tiles alone are >= 512 workgroups).
int ksplit_slices(const KsplitRule &r, int B, const Geom16 &g, int Cin, int Cout, int flags) {
    const int nstages = (Cin / KC) * g.ntaps;
    if (g_forced_ksplit >= 1) return g_forced_ksplit < nstages ? g_forced_ksplit : nstages;
    const long pixels = (long)B * g.H * g.W;
    if (Cout > 64 && ((pixels + 255) / 256) * ceil_div(Cout, 64) >= 512) return 1;
    const Variant16h &var = kVariantsF16[variant_f16(pixels, Cin, Cout, g.ntaps)];
    Conv16Params p;
    fill_params16(p, g, var.BM, var.NP_MAX, flags);
    const long wgs = (long)B * p.tiles_x * p.tiles_y * ceil_div(Cout, var.BN);
    long s = (nstages < r.short_stages ? r.short_target_workgroups : r.target_workgroups) / wgs;
    if (s > nstages / r.min_stages) s = nstages / r.min_stages;
    if (s > r.max_slices) s = r.max_slices;
    return s < 1 ? 1 : (int)s;
}

// ... of a k x k conv (what both dream_conv2d_f16_ksplit* answer)
int ksplit_conv(const KsplitRule &r, int B, int H, int W, int Cin, int Cout, int ksize, int flags) {
    if (B < 1 || H < 1 || W < 1 || Cin < KC || Cin % KC != 0 || Cout < 1 || (ksize != 1 && ksize != 3) || (flags & kKsplitRefused)) return 1;
    return ksplit_slices(r, B, geom16_conv(H, W, ksize, flags), Cin, Cout, flags);
}

}  // namespace

extern "C" int dream_conv2d_f16_ksplit(int B, int H, int W, int Cin, int Cout, int ksize, int flags) {
    return ksplit_conv(kKsplitHourglass, B, H, W, Cin, Cout, ksize, flags);
}

// The same rule over ResnetSimple's table (inference_conv_ksplit="auto").
extern "C" int dream_conv2d_f16_ksplit_resnet(int B, int H, int W, int Cin, int Cout, int ksize, int flags) {
    return ksplit_conv(kKsplitResnet, B, H, W, Cin, Cout, ksize, flags);
}

// bytes of S slices of round_up(B H W Cout, 8) floats
extern "C" size_t dream_conv2d_f16_ksplit_workspace(int B, int H, int W, int Cout, int S) {
    if (B < 1 || H < 1 || W < 1 || Cout < 1 || S < 1) return 0;
    return (size_t)S * ((((size_t)B * H * W * Cout) + 7) & ~(size_t)7) * sizeof(float);
}

// dream_conv2d_f16_nhwc_f16 in S slices: S launches' worth of workgroups in one grid (the ksplit form), then the finishing
// pass.  S == 1 is dream_conv2d_f16_nhwc_f16 itself (the workspace is not touched).
extern "C" int dream_conv2d_f16_ksplit_nhwc_f16(const void *x, const void *w, const int *w_exp, const float *scale,
                                                const float *shift, void *y, unsigned *amax_out, void *workspace, int S, int B,
                                                int H, int W, int Cin, int Cout, int CoutPad, int ksize, int stride, int flags,
                                                void *stream) {
    DREAM_REQUIRE(S >= 1, "conv2d_f16_ksplit: S=%d", S);
    if (S == 1) return dream_conv2d_f16_nhwc_f16(x, w, w_exp, scale, shift, y, amax_out, B, H, W, Cin, Cout, CoutPad, ksize, stride, flags, stream);
    if (int rc = check_conv2d_f16(H, W, ksize, stride, flags)) return rc;
    DREAM_REQUIRE(!(flags & kKsplitRefused), "conv2d_f16_ksplit: flags %d: a launch with a fused pool / upsample / NCHW output is not split", flags);
    DREAM_REQUIRE(workspace && y && (((size_t)workspace | (size_t)y) & 15) == 0, "conv2d_f16_ksplit: workspace and y must be 16-byte aligned");
    const Geom16 g = geom16_conv(H, W, ksize, flags);
    if (int rc = launch_f16(kKsplit, x, nullptr, w, w_exp, nullptr, nullptr, nullptr, workspace, nullptr, B, Cin, Cout, CoutPad, g,
                            flags & ~DREAM_CONV_RELU, stream, S))
        return rc;
    const size_t n = (size_t)B * H * W * Cout, slice = (n + 7) & ~(size_t)7;
    hipLaunchKernelGGL(conv_f16_ksplit_finish_kernel, dim3((unsigned)(slice / 8 / 256 < 4096 ? slice / 8 / 256 + 1 : 4096)), dim3(256), 0, (hipStream_t)stream,
                       (const float *)workspace, slice, S, w_exp, scale, shift, (_Float16 *)y, n, Cout,
                       (flags & DREAM_CONV_RELU) ? 1 : 0, amax_out);
    DREAM_LAUNCH_OK();
    return 0;
}

// ---- inference_conv_ksplit="auto": ResnetSimple's decoder, ConvTranspose2d(k4,s2,p1) -> BatchNorm -> ReLU (dream/models.py:37-136), with the
// contraction of each sub-pixel phase divided over S slices ----------------------------------------------------------
// Slices of one phase (4 taps, kext 3) under ResnetSimple's table; 1 when Cout % 8 != 0 (the finishing pass handles 8 channels a lane).
// Honours dream_conv_f16_set_ksplit.
extern "C" int dream_conv_transpose4x4s2_f16_ksplit(int B, int H, int W, int Cin, int Cout) {
    if (B < 1 || H < 1 || W < 1 || Cin < KC || Cin % KC != 0 || Cout < 1 || Cout % 8 != 0) return 1;
    return ksplit_slices(kKsplitResnet, B, geom16_convT4_phase(H, W, 0), Cin, Cout, 0);
}

// bytes of 4 phases x S slices of round_up(B H W Cout, 8) floats
extern "C" size_t dream_conv_transpose4x4s2_f16_ksplit_workspace(int B, int H, int W, int Cout, int S) {
    return 4 * dream_conv2d_f16_ksplit_workspace(B, H, W, Cout, S);
}

// dream_conv_transpose4x4s2_f16_nhwc_f16 with every phase in S slices: four ksplit-form launches (phase ph writes its slices at
// workspace + (ph * S + s) * slice), then convT4_f16_ksplit_finish_kernel.  S == 1 is dream_conv_transpose4x4s2_f16_nhwc_f16 itself (the
// workspace is not touched).
extern "C" int dream_conv_transpose4x4s2_f16_ksplit_nhwc_f16(const void *x, const void *w, const int *w_exp, const float *scale,
                                                             const float *shift, void *y, unsigned *amax_out, void *workspace, int S,
                                                             int B, int H, int W, int Cin, int Cout, int CoutPad, int flags,
                                                             void *stream) {
    DREAM_REQUIRE(S >= 1, "conv_transpose4x4s2_f16_ksplit: S=%d", S);
    if (S == 1) return dream_conv_transpose4x4s2_f16_nhwc_f16(x, w, w_exp, scale, shift, y, amax_out, B, H, W, Cin, Cout, CoutPad, flags, stream);
    DREAM_REQUIRE((flags & (DREAM_CONV_UPSAMPLE2X | DREAM_CONV_ZEROSTUFF2X | DREAM_CONV_OUT_NCHW | DREAM_CONV_POOL2 | DREAM_CONV_RELUMASK)) == 0,
                  "conv_transpose4x4s2_f16_ksplit: unsupported flags %d: such a launch is not split", flags);
    DREAM_REQUIRE(B >= 1 && H >= 1 && W >= 1 && Cout >= 1 && Cout % 8 == 0,
                  "conv_transpose4x4s2_f16_ksplit: Cout=%d: a split launch needs a multiple of 8 output channels", Cout);
    DREAM_REQUIRE(workspace && y && (((size_t)workspace | (size_t)y) & 15) == 0,
                  "conv_transpose4x4s2_f16_ksplit: workspace and y must be 16-byte aligned");
    const size_t slice = (size_t)B * H * W * Cout;          // (Cout % 8 == 0: already a multiple of 8 floats)
    int ph = 0;
    if (int rc = for_convT4_phases(H, W, Cin, CoutPad, [&](const Geom16 &g, size_t off) {
            return launch_f16(kKsplit, x, nullptr, (const _Float16 *)w + off, w_exp, nullptr, nullptr, nullptr,
                              (float *)workspace + (size_t)(ph++) * S * slice, nullptr, B, Cin, Cout, CoutPad, g, 0, stream, S);
        }))
        return rc;
    const size_t n8 = 4 * slice / 8;
    hipLaunchKernelGGL(convT4_f16_ksplit_finish_kernel, dim3((unsigned)(n8 / 256 < 4096 ? n8 / 256 + 1 : 4096)), dim3(256), 0, (hipStream_t)stream,
                       (const float *)workspace, slice, S, w_exp, scale, shift, (_Float16 *)y, B, H, W, Cout, (flags & DREAM_CONV_RELU) ? 1 : 0,
                       amax_out);
    DREAM_LAUNCH_OK();
    return 0;
}
