// What the two implicit-GEMM kernels on the fp16 matrix cores share: conv_f16x3.hip (split precision, three MFMAs per product) and
// conv_f16.hip (plain fp16 operands, one MFMA per product).  Launch parameters, the LDS row layout, the tap-table geometry, the tile
// chooser are one text for both; so is the epilogue, conv_f16_epilogue.inc, which each kernel includes at its end.
#pragma once
#include <dream_cdna4.h>
#include "common.h"
#include "half_store.h"
#include "half_scale.h"
#include "../../include/dream_hip.h"

struct Conv16Params {
    const float *x;
    const _Float16 *w_hi;    // [ntaps][CoutPad][Cin]
    union {                  // (one slot, so that the layout every measured kernel was compiled against stays)
        const _Float16 *w_lo;       // (split kernel only)
        const unsigned *grad_amax;  // (the GRAD16 kernels of conv_f16.hip only) device scalar: bit pattern of the loss gradient's amax
    };
    const int *w_exp;        // device scalar: weights were multiplied by 2^w_exp before the split
    const unsigned *amax_in; // device scalar: bit pattern of max|x| of the input tensor
    const float *scale;
    const float *shift;
    const float *residual;
    float *y;
    unsigned *amax_out;
    int B, H, W, Hin, Win, Hs, Ws, Ho, Wo;
    int Cin, Cout, CoutPad;
    int TH, TW, PH, PW, tiles_x, tiles_y, rcpTW;
    int in_scale, in_step, lane_stride, pad_y, pad_x;
    unsigned long long tap_w;   // 16 x 4-bit: weight slice of each tap of this launch
    int ntaps;
    unsigned long long tap_dy, tap_dx;
    int out_scale, out_oy, out_ox;
    int flags;
};

namespace {

constexpr int KC = 32;              // k's per stage (two 32x32x16 MFMA k-steps)
constexpr int S16 = KC + 8;         // LDS row stride in halfs (80 B: odd number of 16-B slots)

DREAM_DEVICE float pow2f(int e) { return __uint_as_float((unsigned)(e + 127) << 23); }

struct Geom16 {
    int H, W, Hin, Win, Hs, Ws, Ho, Wo;      // position grid, logical / stored input extent, output extent
    int pad, kext, ntaps;
    int tap_dy[16], tap_dx[16];
    int out_scale, out_oy, out_ox;
    int tap_w[16] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
};

void choose_tile16(int H, int W, int BM, int np_max, int lane_stride, int kext, bool even, int *th_out, int *tw_out) {
    long best_tiles = -1;
    int best_np = 0, bth = even ? 2 : 1, btw = even ? 2 : 1;
    const int He = even ? (H + 1) / 2 * 2 : H, We = even ? (W + 1) / 2 * 2 : W;
    // divisor (tw, or tw/2 with the fused pool) < 128 keeps the (m * rcpTW) >> 16 division exact for m < 512
    for (int tw = even ? 2 : 1; tw <= BM && tw <= (even ? 254 : 127); tw += even ? 2 : 1) {
        int th = BM / tw;
        if (even) th &= ~1;
        if (th < 1) break;
        if (th > He) th = He;
        const int twc = tw > We ? We : tw;
        const int np = ((th - 1) * lane_stride + kext) * ((twc - 1) * lane_stride + kext);
        if (np > np_max) continue;
        const long tiles = (long)ceil_div(H, th) * ceil_div(W, twc);
        if (best_tiles < 0 || tiles < best_tiles || (tiles == best_tiles && np < best_np)) {
            best_tiles = tiles; best_np = np; bth = th; btw = twc;
        }
    }
    *th_out = bth;
    *tw_out = btw;
}

// k x k (1 | 3) stride-1 conv over an H x W grid; with an upsample / zero-stuff flag the stored input is half that size
Geom16 geom16_conv(int H, int W, int ksize, int flags) {
    const bool ups = (flags & (DREAM_CONV_UPSAMPLE2X | DREAM_CONV_ZEROSTUFF2X)) != 0;
    Geom16 g;
    g.H = H; g.W = W; g.Hin = H; g.Win = W; g.Hs = ups ? (H + 1) / 2 : H; g.Ws = ups ? (W + 1) / 2 : W; g.Ho = H; g.Wo = W;
    g.pad = ksize / 2; g.kext = ksize; g.ntaps = ksize * ksize;
    for (int t = 0; t < g.ntaps; ++t) { g.tap_dy[t] = t / ksize; g.tap_dx[t] = t % ksize; }
    g.out_scale = 1; g.out_oy = 0; g.out_ox = 0;
    return g;
}

// sub-pixel phase ph = 2a + b of ConvTranspose2d(k4,s2,p1): a 2x2-tap conv of the input whose outputs land on (2y + a, 2x + b);
// weight slices 0..3 of the phase's own block of the packed planes
Geom16 geom16_convT4_phase(int H, int W, int ph) {
    const int a = ph >> 1, b = ph & 1;
    Geom16 g;
    g.H = H; g.W = W; g.Hin = H; g.Win = W; g.Hs = H; g.Ws = W; g.Ho = 2 * H; g.Wo = 2 * W;
    g.pad = 1; g.kext = 3; g.ntaps = 4;
    for (int t = 0; t < 4; ++t) { g.tap_dy[t] = (t >> 1) + a; g.tap_dx[t] = (t & 1) + b; }
    g.out_scale = 2; g.out_oy = a; g.out_ox = b;
    return g;
}

// sub-pixel phase of ConvTranspose2d(k3,s2,p1,output_padding 1): 1 / 2 / 2 / 4 taps picking their slices of the mode-1 packed planes
Geom16 geom16_convT3_phase(int H, int W, int ph) {
    const int a = ph >> 1, b = ph & 1;
    Geom16 g;
    g.H = H; g.W = W; g.Hin = H; g.Win = W; g.Hs = H; g.Ws = W; g.Ho = 2 * H; g.Wo = 2 * W;
    g.pad = 0; g.kext = 2; g.ntaps = 0;
    for (int iy = 0; iy <= a; ++iy)
        for (int ix = 0; ix <= b; ++ix) {
            const int ky = a ? 2 - 2 * iy : 1, kx = b ? 2 - 2 * ix : 1, t = g.ntaps++;
            g.tap_dy[t] = iy; g.tap_dx[t] = ix;
            g.tap_w[t] = 8 - (3 * ky + kx);
        }
    g.out_scale = 2; g.out_oy = a; g.out_ox = b;
    return g;
}

// The four phases of the two transposed convs: launch(geometry[, element offset of the phase's block of the packed planes]) for each,
// stopping at the first launch that fails
template <class Launch> int for_convT4_phases(int H, int W, int Cin, int CoutPad, Launch launch) {
    for (int ph = 0; ph < 4; ++ph)
        if (int rc = launch(geom16_convT4_phase(H, W, ph), (size_t)ph * 4 * CoutPad * Cin)) return rc;
    return 0;
}

template <class Launch> int for_convT3_phases(int H, int W, Launch launch) {
    for (int ph = 0; ph < 4; ++ph)
        if (int rc = launch(geom16_convT3_phase(H, W, ph))) return rc;
    return 0;
}

// tile, patch and tap tables of one launch of variant (BM, NP_MAX) into p (everything but the pointers and B / Cin / Cout / CoutPad)
void fill_params16(Conv16Params &p, const Geom16 &g, int BM, int np_max, int flags) {
    const bool pool = (flags & DREAM_CONV_POOL2) != 0;
    p.Hin = g.Hin; p.Win = g.Win; p.Hs = g.Hs; p.Ws = g.Ws; p.Ho = g.Ho; p.Wo = g.Wo; p.H = g.H; p.W = g.W;
    choose_tile16(g.H, g.W, BM, np_max, 1, g.kext, pool, &p.TH, &p.TW);
    p.PH = p.TH - 1 + g.kext; p.PW = p.TW - 1 + g.kext;
    p.tiles_x = ceil_div(g.W, p.TW); p.tiles_y = ceil_div(g.H, p.TH);
    p.rcpTW = pool ? (65536 + p.TW / 2 - 1) / (p.TW / 2) : (65536 + p.TW - 1) / p.TW;
    if (pool) { p.Ho = g.H / 2; p.Wo = g.W / 2; }
    p.in_scale = 1; p.in_step = 1; p.lane_stride = 1; p.pad_y = g.pad; p.pad_x = g.pad;
    p.ntaps = g.ntaps;
    p.tap_dy = 0; p.tap_dx = 0; p.tap_w = 0;
    for (int t = 0; t < g.ntaps; ++t) {
        p.tap_dy |= (unsigned long long)g.tap_dy[t] << (4 * t);
        p.tap_dx |= (unsigned long long)g.tap_dx[t] << (4 * t);
        p.tap_w |= (unsigned long long)g.tap_w[t] << (4 * t);
    }
    p.out_scale = g.out_scale; p.out_oy = g.out_oy; p.out_ox = g.out_ox;
    p.flags = flags;
}

}  // namespace
