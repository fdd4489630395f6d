// The 1x1 GEMM of gemm1x1.hip and its weight gradient on the fp16 matrix cores (v_mfma_f32_32x32x16_f16): ResnetSimple with
// train_gemm_precision="fp16".  Replaces the same torch.nn.Conv2d(k=1) launches of the ResNet-101 Bottlenecks behind dream/models.py:22-32
// (forward with the following BatchNorm's statistics, data gradient with the producer's BatchNorm backward sums, weight gradient).
//
// Everything in HBM stays fp32: a launch rounds each operand ONCE, while it loads it.
//   * activation operand: half(clamp(v, +-65504)) -- e_x = 0: the inputs of these convs have amax 1.3 .. 6.3; with PRE the
//     producer's BatchNorm + ReLU is applied in fp32 first (bn_relu: the single-rounded fmaf the backward's mask recomputes);
//   * gradient operand: half(v * 2^e_g), e_g = scale_exponent(*amax) with the amax published by the launch that wrote the tensor
//     (dream_bn_bwd_apply_amax_nhwc_f32): max|v| 2^e_g lies in [2^13, 2^14); a zero tensor has e_g = 0;
//   * weights: packed as half(w * 2^e_w) (dream_pack_conv1x1_weight_f16), e_w = scale_exponent(amax w) taken on the device at pack time;
//   * fp32 accumulation; 2^-e_w and 2^-e_g are applied in the epilogue, two exact multiplications by powers of two.
//
// Lane layout of v_mfma_f32_32x32x16_f16: A lane l holds row l & 31, k = 8 (l >> 5) .. + 7; B likewise for its column; D register r of
// lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31.  Both operands are contiguous along K, so a lane feeds an MFMA from two
// 16-byte loads of fp32 activations (8 consecutive k of its row) and ONE 16-byte load of packed half weights.
//
// Epilogue orientation: POSITIONS ARE ROWS.  A lane then holds 16 rows of ONE output channel per 32 x 32 block: the
// per-channel sums of the statistics forms are in-lane fp64 additions plus one exchange with lane ^ 32, and the 4-byte stores of a
// register cover 128 contiguous bytes per half-wave.  The transposed product would store 16 bytes per lane, but its per-channel sums
// become 32-lane fp64 reductions (five exchanges of two doubles per channel pair and register: ~1000 cross-lane operations per wave
// tile) on a kernel whose matrix time is already below its load time.
//
// Wave tile 64 positions x 64 channels (2 x 2 blocks, 64 accumulator registers), workgroup = four wave tiles, or two / one whose K range
// is split over the waves and summed through LDS in wave order (gemm1x1.hip's levels and rule); StatTree / bn_finish_forward as there:
// deterministic statistics finished inside the launch.
//
// Load schedule.  As in gemm1x1_kernel (its header comment tells what the compiler did when left alone: every load sunk behind the MFMAs
// and waited for on the spot) the order is pinned with a scheduling barrier per MFMA: the loads of chunk t + 1 are issued between the four
// MFMAs of chunk t, into the register set the previous chunk freed.
#include <stdlib.h>
#include <dream_cdna4.h>
#include "common.h"
#include "half_scale.h"
#include "stat_tree.h"
#include "../../include/dream_hip.h"

namespace {

DREAM_DEVICE float pow2_of(int e) { return __uint_as_float((unsigned)(e + 127) << 23); }      // |e| <= 100 (scale_exponent)

// the rounding of an operand: v * s (s a power of two, 1 for activations), saturated, nearest even
DREAM_DEVICE _Float16 half_operand(float v, float s) { return (_Float16)fminf(fmaxf(v * s, -65504.0f), 65504.0f); }

struct Gemm16Params {
    const float *x;          // [M][x_stride] (first K columns used), fp32
    const unsigned *amax_x;  // bit pattern of max|x| (a gradient operand), or null: e_x = 0 (an activation operand)
    const _Float16 *w;       // packed [K/16][NPad][16] halfs of w * 2^(*w_exp)
    const int *w_exp;
    const float *shift;      // [N] or null
    const float *residual;   // [M][N] or null
    float *y;                // [M][N]
    int M, K, N, NPad, x_stride;
    int nrb, ncb;            // 64-row / 64-column blocks
    const float *pre_ab;     // PRE: [2][K]
    StatTree st;             // EPI 1 / 2: one row of partial sums per 64-row block
    BnFwdOut st_fwd;         // EPI 1
    const float *st_z;       // EPI 2: [M][N]
    const float *st_zab;     // EPI 2: [2][N], or null when the mask comes from st_yact
    const float *st_yact;    // EPI 2: [M][N] or null
    const float *st_mean, *st_invstd;
    float *st_dgamma, *st_dbeta;
};

// EPI 0: y = acc + shift (+ residual);  EPI 1: y = acc + shift and the statistics of y -> the following BatchNorm;
// EPI 2: y = (acc (+ residual)) masked, sums of y and y * xhat -> dbeta / dgamma of the masked BatchNorm (gemm1x1.hip, GemmParams)
template <int KS, bool PRE, int EPI, bool RES>
__global__ void __launch_bounds__(256, 2) gemm1x1_f16_kernel(const Gemm16Params p) {
    __shared__ float s_part[KS > 1 ? 4 * 4 * 16 * 64 : 1];               // [wave][block][register][lane]: the waves' partial tiles
    __shared__ double s_stat[(KS > 1 && EPI != 0) ? 4 * 64 * 2 : 1];     // [wave][column][2]
    const int lane = threadIdx.x & 63;
    const int wave = wave_index();
    const int nwg = (int)gridDim.x;                                       // (a multiple of 8: one contiguous range of tiles per XCD)
    const int wg = (int)(blockIdx.x & 7) * (nwg >> 3) + (int)(blockIdx.x >> 3);
    const int tile = wg * (4 / KS) + wave / KS;
    const int kpart = wave % KS;
    const bool live = tile < p.nrb * p.ncb;
    if (KS == 1 && !live) return;
    const int cb = tile % p.ncb, rb = tile / p.ncb;
    const int li = lane & 31, lh = lane >> 5;

    const BufferRsrc xbuf = make_buffer(p.x, (size_t)p.M * p.x_stride * sizeof(float));
    const BufferRsrc wbuf = make_buffer(p.w, (size_t)(p.K / 16) * p.NPad * 16 * sizeof(_Float16));
    const BufferRsrc abbuf = make_buffer(PRE ? p.pre_ab : p.x, PRE ? (size_t)2 * p.K * sizeof(float) : 0);
    unsigned a_off[2], b_off[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int row = rb * 64 + 32 * m + li;
        a_off[m] = live && row < p.M ? (unsigned)((row * p.x_stride + 8 * lh) * 4) : BUFFER_OOB;
    }
#pragma unroll
    for (int n = 0; n < 2; ++n) b_off[n] = (unsigned)(((cb * 64 + 32 * n + li) * 16 + 8 * lh) * 2);
    const unsigned b_chunk = (unsigned)(p.NPad * 16 * 2);                 // bytes between k chunks of the packed weights
    const float sa = p.amax_x != nullptr ? pow2_of(scale_exponent(*p.amax_x)) : 1.0f;

    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.0f;

    f32x4 xa[2][2][2], xb[2][2], pab[2][2][2];       // [set][row block][k half] / [set][column block] (8 halfs) / [set][a | b][k half]
    constexpr int NLOADS = (PRE ? 10 : 6);
    // the i-th load of chunk t (16 k's) into register set `set`: weights, the PRE scale / shift, the activation rows
    auto issue = [&](int set, int t, int i) {
        if (i < 2) xb[set][i] = buffer_load_x4(wbuf, b_off[i], (unsigned)t * b_chunk);
        else if (PRE && i < 6) {
            const int j = i - 2;                                          // a: k half 0, 1; b: k half 0, 1
            pab[set][j >> 1][j & 1] = buffer_load_x4(abbuf, (unsigned)(((j >> 1) * p.K + 8 * lh + 4 * (j & 1)) * 4), (unsigned)t * 64u);
        } else {
            const int j = i - (NLOADS - 4);
            xa[set][j >> 1][j & 1] = buffer_load_x4(xbuf, a_off[j >> 1] + 16u * (unsigned)(j & 1), (unsigned)t * 64u);
        }
    };
    // multiply the chunk in set S, meanwhile issue the loads of chunk tn into the other set (pinned: one MFMA, its share of the loads)
    auto step = [&](auto s_tag, int tn, auto load_tag) {
        constexpr int S = decltype(s_tag)::value;
        constexpr bool LOAD = decltype(load_tag)::value;
        f16x8 ha[2], hb[2];
#pragma unroll
        for (int n = 0; n < 2; ++n) hb[n] = __builtin_bit_cast(f16x8, xb[S][n]);
#pragma unroll
        for (int m = 0; m < 2; ++m) {
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float v = xa[S][m][h][e];
                    if (PRE) v = fmaxf(__builtin_fmaf(pab[S][0][h][e], v, pab[S][1][h][e]), 0.0f);
                    ha[m][4 * h + e] = half_operand(v, sa);
                }
        }
        constexpr int PER = (NLOADS + 3) / 4;
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                acc[m][n] = mfma_f32_32x32x16_f16(ha[m], hb[n], acc[m][n]);
                const int g = 2 * m + n;
#pragma unroll
                for (int i = 0; i < PER; ++i)
                    if (LOAD && g * PER + i < NLOADS) issue(1 - S, tn, g * PER + i);
                __builtin_amdgcn_sched_barrier(0);
            }
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using Yes = std::integral_constant<bool, true>;
    using No = std::integral_constant<bool, false>;
    const int nchunks = p.K / 16 / KS;               // even (host side); this wave's chunks start at t0
    const int t0 = kpart * nchunks;
    if (live) {
#pragma unroll
        for (int i = 0; i < NLOADS; ++i) issue(0, t0, i);
        __builtin_amdgcn_sched_barrier(0);
        for (int t = 0; t + 2 < nchunks; t += 2) {
            step(I0{}, t0 + t + 1, Yes{});
            step(I1{}, t0 + t + 2, Yes{});
        }
        step(I0{}, t0 + nchunks - 1, Yes{});
        step(I1{}, 0, No{});
    }
    // A wavefront owns NU = 8 / KS of the 8 units (block row m = u >> 2, register quad q = u & 3: rows 32 m + 8 q + 4 lh + 0..3) of its
    // tile, in order: unit u belongs to wave kpart = u / NU.  Split K: partial tiles through LDS, summed in wave order.
    constexpr int NU = 8 / KS;
    if (KS > 1) {
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) s_part[((wave * 4 + 2 * m + n) * 16 + r) * 64 + lane] = acc[m][n][r];
        __syncthreads();
        const int w0 = wave - kpart;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (u / NU == kpart) {
#pragma unroll
                for (int n = 0; n < 2; ++n)
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        const int r = 4 * (u & 3) + rr, b = 2 * (u >> 2) + n;
                        float v = s_part[(((w0 + 0) * 4 + b) * 16 + r) * 64 + lane];
#pragma unroll
                        for (int k = 1; k < KS; ++k) v = v + s_part[(((w0 + k) * 4 + b) * 16 + r) * 64 + lane];
                        acc[u >> 2][n][r] = v;
                    }
            }
        if (EPI == 0 && !live) return;               // (with statistics the dead waves stay for the second barrier)
    }

    // ---- epilogue: lane holds, per block (m, n), 16 rows of column li ------------------------------------------------------------
    const float so_w = pow2_of(-*p.w_exp), so_x = 1.0f / sa;              // exact powers of two
    constexpr bool HAS_RES = RES || EPI == 2;
    const long trow = (long)rb * 64;
    const size_t tbytes = live ? (size_t)(p.M - trow) * p.N * sizeof(float) : 0;
    const BufferRsrc rbuf = make_buffer(HAS_RES && p.residual ? p.residual + trow * p.N : p.x, HAS_RES && p.residual ? tbytes : 0);
    const BufferRsrc zbuf = make_buffer(EPI == 2 ? p.st_z + trow * p.N : p.x, EPI == 2 ? tbytes : 0);
    const BufferRsrc yabuf = make_buffer(EPI == 2 && p.st_yact ? p.st_yact + trow * p.N : p.x, EPI == 2 && p.st_yact ? tbytes : 0);
    const BufferRsrc ybuf = make_buffer(p.y + trow * p.N, tbytes);
    const bool mask_y = EPI == 2 && p.st_yact != nullptr;
    unsigned c_off[2];                                                    // byte offset of this lane's two columns inside a row
    bool c_ok[2];
    float sh[2] = {0.0f, 0.0f}, za[2] = {0.0f, 0.0f}, zb[2] = {0.0f, 0.0f}, zmu[2] = {0.0f, 0.0f}, zis[2] = {0.0f, 0.0f};
    double st0[2] = {0.0, 0.0}, st1[2] = {0.0, 0.0};
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int c = cb * 64 + 32 * n + li;
        const bool cok = live && c < p.N;
        c_ok[n] = cok;
        c_off[n] = cok ? (unsigned)c * 4u : BUFFER_OOB;                   // (stays out of range under the row offsets: descriptors < 2 GB)
        if (cok && EPI != 2 && p.shift != nullptr) sh[n] = p.shift[c];
        if (cok && EPI == 2) {
            if (!mask_y) { za[n] = p.st_zab[c]; zb[n] = p.st_zab[p.N + c]; }
            zmu[n] = p.st_mean[c];
            zis[n] = p.st_invstd[c];
        }
    }
    const unsigned row_bytes = (unsigned)p.N * 4u;
    const int mrows = p.M - (int)trow;                                    // rows of this tile that exist
    if (live) {
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (u / NU == kpart) {
                const int m = u >> 2, q = u & 3;
                float res[4][2], z[4][2], ya[4][2];
                unsigned off[4][2];
                // the unit's operands first (up to 24 loads in flight), then its arithmetic and stores
#pragma unroll
                for (int rr = 0; rr < 4; ++rr)
#pragma unroll
                    for (int n = 0; n < 2; ++n) {
                        const int row = 32 * m + 8 * q + 4 * lh + rr;
                        off[rr][n] = (row < mrows && c_ok[n]) ? c_off[n] + (unsigned)row * row_bytes : BUFFER_OOB;
                        res[rr][n] = z[rr][n] = ya[rr][n] = 0.0f;
                        if (HAS_RES) res[rr][n] = buffer_load_f32(rbuf, off[rr][n], 0u);
                        if (EPI == 2) {
                            z[rr][n] = buffer_load_f32(zbuf, off[rr][n], 0u);
                            ya[rr][n] = buffer_load_f32(yabuf, off[rr][n], 0u);
                        }
                    }
#pragma unroll
                for (int rr = 0; rr < 4; ++rr)
#pragma unroll
                    for (int n = 0; n < 2; ++n) {
                        const bool ok = off[rr][n] != BUFFER_OOB;          // the row and the column exist
                        float v = acc[m][n][4 * q + rr] * so_w * so_x;
                        if (EPI != 2) v = v + sh[n];
                        if (HAS_RES) v = v + res[rr][n];
                        if (EPI == 1) {
                            const float vm = ok ? v : 0.0f;
                            st0[n] += (double)vm;
                            st1[n] += (double)vm * (double)vm;
                        }
                        if (EPI == 2) {
                            const bool on = mask_y ? ya[rr][n] > 0.0f : __builtin_fmaf(za[n], z[rr][n], zb[n]) > 0.0f;
                            v = (on && ok) ? v : 0.0f;
                            const float xh = (z[rr][n] - zmu[n]) * zis[n];
                            st0[n] += (double)v;
                            st1[n] += (double)v * (double)xh;
                        }
                        buffer_store_f32(ybuf, v, off[rr][n], 0u);
                    }
                // one unit at a time (gemm1x1_kernel: left alone the scheduler interleaves every row's fp64 sums)
                __builtin_amdgcn_sched_barrier(0);
            }
    }
    if (EPI != 0) {
        // lanes l and l ^ 32 hold the same two channels on different rows
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            st0[n] += lane_xor(st0[n], 32);
            st1[n] += lane_xor(st1[n], 32);
        }
        if (KS > 1) {
            // the KS waves of a tile hold disjoint rows: summed through LDS in wave order, wave kpart == 0 carries on
            if (lh == 0) {
#pragma unroll
                for (int n = 0; n < 2; ++n) { s_stat[(wave * 64 + 32 * n + li) * 2] = st0[n]; s_stat[(wave * 64 + 32 * n + li) * 2 + 1] = st1[n]; }
            }
            __syncthreads();
            if (!live || kpart != 0) return;
            if (lh == 0) {
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    double a = 0.0, b = 0.0;
#pragma unroll
                    for (int k = 0; k < KS; ++k) {
                        a += s_stat[((wave + k) * 64 + 32 * n + li) * 2];
                        b += s_stat[((wave + k) * 64 + 32 * n + li) * 2 + 1];
                    }
                    st0[n] = a;
                    st1[n] = b;
                }
            }
        }
        if (lh == 0) {
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const int c = cb * 64 + 32 * n + li;
                if (c < p.N) {
                    double *dst = p.st.rows + ((size_t)rb * p.N + c) * 2;
                    coherent_store(dst, st0[n]);
                    coherent_store(dst + 1, st1[n]);
                }
            }
        }
        double s0, s1;
        if (!stat_tree_arrive(p.st, cb, rb, lane, &s0, &s1)) return;
        const int c = cb * 64 + lane;
        if (EPI == 1) {
            bn_finish_forward(p.st_fwd, c, p.N, (double)p.M, s0, s1);
        } else if (c < p.N) {
            p.st_dbeta[c] = (float)s0;
            p.st_dgamma[c] = (float)s1;
        }
    }
}

// ---- the half packer: [Cout][Cin] fp32 -> [K/16][RowsPad][16] halfs of w * 2^e_w, rows in their natural order (an MFMA column IS a channel)
__global__ void __launch_bounds__(256) absmax16_kernel(const float *x, size_t n, unsigned *out) {
    float m = 0.0f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) m = fmaxf(m, fabsf(x[i]));
    publish_amax(out, m);
}

// (blk / nblk: this workgroup's index and the number of workgroups that share the tensor, as in pack_device.h)
DREAM_DEVICE void pack16_body(const float *w, _Float16 *packed, const unsigned *amax, int *exp_out, int Cout, int Cin, int mode, int blk,
                              int nblk) {
    const int e = scale_exponent(*amax);
    const float s = pow2_of(e);
    if (blk == 0 && threadIdx.x == 0) *exp_out = e;
    const int rows = mode == 0 ? Cout : Cin, K = mode == 0 ? Cin : Cout;
    const int RowsPad = (rows + 63) / 64 * 64;
    const size_t total = (size_t)(K / 16) * RowsPad * 16;
    for (size_t i = (size_t)blk * 256 + threadIdx.x; i < total; i += (size_t)nblk * 256) {
        const int kk = (int)(i & 15);
        const size_t rest = i >> 4;
        const int row = (int)(rest % RowsPad), k = 16 * (int)(rest / RowsPad) + kk;
        float v = 0.0f;
        if (row < rows) v = mode == 0 ? w[(size_t)row * Cin + k] : w[(size_t)k * Cin + row];
        packed[i] = half_operand(v, s);
    }
}

__global__ void __launch_bounds__(256) gemm1x1_f16_pack_kernel(const float *w, _Float16 *packed, const unsigned *amax, int *exp_out,
                                                               int Cout, int Cin, int mode) {
    pack16_body(w, packed, amax, exp_out, Cout, Cin, mode, (int)blockIdx.x, (int)gridDim.x);
}

// Every half copy of a network refreshed by three launches per step (zero the amax words, the amax of every weight, every pack;
// grid = (workgroups per job, jobs)) instead of three per copy: a training step re-packs each weight after the optimizer changed it,
// and at 16 frames the 2 x 70 half copies of ResNet-101 packed one by one cost more than the fp16 GEMMs save (pack_batched.hip tells
// the same story for the fp32 copies).  Same values, bit for bit: the maximum does not depend on the order it is taken in.
// Modes 2 / 3 (ResnetSimple's train_decoder_precision="fp16"): src is a ConvTranspose2d(k4,s2,p1) weight [cout = Cin_T][cin =
// Cout_T][4][4]; 2 = the sub-pixel phase planes [phase][tap][RowsPad][ColsPad] of dream_pack_convT4x4_weight_f16x3's `hi`, 3 = the 16-slice
// plane [4 ty + tx][RowsPad][ColsPad] of dream_pack_conv_weight_f16x3's `hi` (mode 0 of the tensor read as [O = Cin_T, I = Cout_T]); rows padded
// to 128 (dream_conv3x3_cout_pad), columns to 32, as ops.py allocates them.  The one-tensor packers' halfs and exponents, bit for bit.
DREAM_DEVICE void pack16_convT4_body(const float *wT, _Float16 *hi, const unsigned *amax, int *exp_out, int CinT, int CoutT, int mode, int blk,
                                     int nblk) {
    const int e = scale_exponent(*amax);
    const float s = pow2_of(e);
    if (blk == 0 && threadIdx.x == 0) *exp_out = e;
    const int rows = mode == 2 ? CoutT : CinT, cols = mode == 2 ? CinT : CoutT;
    const int RowsPad = (rows + 127) / 128 * 128, ColsPad = (cols + 31) / 32 * 32;
    const size_t total = (size_t)16 * RowsPad * ColsPad;
    for (size_t idx = (size_t)blk * 256 + threadIdx.x; idx < total; idx += (size_t)nblk * 256) {
        const int c = (int)(idx % ColsPad);
        const size_t q = idx / ColsPad;
        const int r = (int)(q % RowsPad), pt = (int)(q / RowsPad);
        float v = 0.0f;
        if (r < rows && c < cols) {
            if (mode == 2) {
                const int ph = pt >> 2, t = pt & 3;
                const int ky = 3 - 2 * (t >> 1) - (ph >> 1), kx = 3 - 2 * (t & 1) - (ph & 1);
                v = wT[(((size_t)c * CoutT + r) * 4 + ky) * 4 + kx];
            } else {
                v = wT[((size_t)r * CoutT + c) * 16 + pt];
            }
        }
        hi[idx] = (_Float16)(v * s);
    }
}

__global__ void __launch_bounds__(256) pack16_amax_batched_kernel(const dream_pack16_job *jobs) {
    const dream_pack16_job j = jobs[blockIdx.y];
    const size_t n = (size_t)j.cout * j.cin * (j.mode >= 2 ? 16 : 1);
    float m = 0.0f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) m = fmaxf(m, fabsf(j.src[i]));
    publish_amax(j.scratch, m);
}

__global__ void __launch_bounds__(256) pack16_batched_kernel(const dream_pack16_job *jobs) {
    const dream_pack16_job j = jobs[blockIdx.y];
    if (j.mode >= 2) {
        pack16_convT4_body(j.src, (_Float16 *)j.dst, j.scratch, j.exp, j.cout, j.cin, j.mode, (int)blockIdx.x, (int)gridDim.x);
        return;
    }
    pack16_body(j.src, (_Float16 *)j.dst, j.scratch, j.exp, j.cout, j.cin, j.mode, (int)blockIdx.x, (int)gridDim.x);
}

// ---- weight gradient: dW[co][ci] = sum_pos dy[pos][co] x[pos][ci] ---------------------------------------------------------------------
// The contraction runs over positions and an MFMA lane wants 8 consecutive k of one row.  Lane (i = l & 31, h = l >> 5) loads the SAME
// two channels 2 i, 2 i + 1 of the 8 consecutive positions 8 h .. 8 h + 7 of a chunk of 16 (eight 8-byte loads per operand: every load
// instruction reads 256 contiguous bytes per position) and holds, component by component, two MFMA operands: component e of dy is the
// A operand whose row i is channel co = 2 i + e, component f of x the B operand whose column i is channel ci = 2 i + f.  2 x 2 MFMAs =
// a 64 x 64 tile of channel pairs from 16 loads, nothing staged, nothing transformed.  The four waves of a workgroup take a quarter
// each of the workgroup's positions, sum through LDS in wave order and write one partial tile; the reduce kernel sums the workgroups'
// partials in index order and applies 2^-e_g.  No floating-point atomics: two runs give the same bits.
struct Wgrad16Params {
    const float *x;          // [M][Cin]
    const float *dy;         // [M][Cdy]
    const unsigned *amax_dy; // bit pattern of max|dy|
    float *partial;          // [nsplit][Cout][Cin], times 2^e_g
    int M, Cin, Cout, Cdy;
    int ncob, ncib;
    int chunks_per_wave;     // chunks of 16 positions per wave (even)
    const float *pre_ab;     // PRE: [2][Cin]
};

template <bool PRE>
__global__ void __launch_bounds__(256, 2) wgrad1x1_f16_kernel(const Wgrad16Params p) {
    __shared__ float s_part[4 * 4 * 16 * 64];
    const int lane = threadIdx.x & 63;
    const int wave = wave_index();
    const int tile = (int)blockIdx.x % (p.ncob * p.ncib), split = (int)blockIdx.x / (p.ncob * p.ncib);
    const int cob = tile % p.ncob, cib = tile / p.ncob;
    const int li = lane & 31, lh = lane >> 5;
    const BufferRsrc xbuf = make_buffer(p.x, (size_t)p.M * p.Cin * sizeof(float));
    const BufferRsrc ybuf = make_buffer(p.dy, (size_t)p.M * p.Cdy * sizeof(float));
    const long pos0 = ((long)split * 4 + wave) * p.chunks_per_wave * 16;          // first position of this wave
    // this wave's chunks that hold a position of the tensor, rounded up to an even count (<= chunks_per_wave, which is even): the
    // offsets below pass the end of the tensor by fewer than 32 positions (the entry point leaves 64), beyond it the hardware returns zeros
    int nchunks = 0;
    if (pos0 < p.M) {
        const long left = (p.M - pos0 + 15) / 16;
        nchunks = (int)(left < p.chunks_per_wave ? (left + 1) / 2 * 2 : p.chunks_per_wave);
    }
    const int co = cob * 64 + 2 * li;
    const unsigned y_off = co < p.Cdy ? (unsigned)(((pos0 + 8 * lh) * p.Cdy + co) * 4) : BUFFER_OOB;
    const unsigned x_off = (unsigned)(((pos0 + 8 * lh) * p.Cin + cib * 64 + 2 * li) * 4);
    const unsigned y_row = (unsigned)(p.Cdy * 4), x_row = (unsigned)(p.Cin * 4);
    const float sg = pow2_of(scale_exponent(*p.amax_dy));

    f32x16 acc[2][2];
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[e][f][r] = 0.0f;
    f32x2 ya[2][8], xa[2][8];                        // [register set][position of the lane's eight]
    f32x2 pa = {1.0f, 1.0f}, pb = {0.0f, 0.0f};      // a lane's two input channels never change
    if (PRE) {
        pa = *(const f32x2 *)(p.pre_ab + cib * 64 + 2 * li);
        pb = *(const f32x2 *)(p.pre_ab + p.Cin + cib * 64 + 2 * li);
    }
    // the i-th of the sixteen loads of chunk c into register set `set` (the whole offset in the VECTOR operand: the bounds check does not
    // see the scalar offset)
    auto issue = [&](int set, int c, int i) {
        const int j = i >> 1;
        if ((i & 1) == 0) ya[set][j] = buffer_load_x2(ybuf, y_off == BUFFER_OOB ? BUFFER_OOB : y_off + (unsigned)(16 * c + j) * y_row, 0);
        else xa[set][j] = buffer_load_x2(xbuf, x_off + (unsigned)(16 * c + j) * x_row, 0);
    };
    auto step = [&](auto s_tag, int cn, auto load_tag) {
        constexpr int S = decltype(s_tag)::value;
        constexpr bool LOAD = decltype(load_tag)::value;
        f16x8 hy[2], hx[2];
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                float v = xa[S][j][e];
                // (positions beyond the tensor read zeros on BOTH operands: relu(b) there meets dy = 0)
                if (PRE) v = fmaxf(__builtin_fmaf(pa[e], v, pb[e]), 0.0f);
                hx[e][j] = half_operand(v, 1.0f);
                hy[e][j] = half_operand(ya[S][j][e], sg);
            }
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                acc[e][f] = mfma_f32_32x32x16_f16(hy[e], hx[f], acc[e][f]);
                const int g = 2 * e + f;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (LOAD) issue(1 - S, cn, 4 * g + i);
                __builtin_amdgcn_sched_barrier(0);
            }
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using Yes = std::integral_constant<bool, true>;
    using No = std::integral_constant<bool, false>;
    if (nchunks > 0) {
#pragma unroll
        for (int i = 0; i < 16; ++i) issue(0, 0, i);
        __builtin_amdgcn_sched_barrier(0);
        for (int c = 0; c + 2 < nchunks; c += 2) {
            step(I0{}, c + 1, Yes{});
            step(I1{}, c + 2, Yes{});
        }
        step(I0{}, nchunks - 1, Yes{});
        step(I1{}, 0, No{});
    }
    // the workgroup's four partial tiles through LDS; wave w then owns block (e, f) = (w >> 1, w & 1)
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
            for (int r = 0; r < 16; ++r) s_part[((wave * 4 + 2 * e + f) * 16 + r) * 64 + lane] = acc[e][f][r];
    __syncthreads();
    float *out = p.partial + (size_t)split * p.Cout * p.Cin;
    const int e = wave >> 1, f = wave & 1;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float v = s_part[((0 * 4 + wave) * 16 + r) * 64 + lane];
#pragma unroll
        for (int k = 1; k < 4; ++k) v = v + s_part[((k * 4 + wave) * 16 + r) * 64 + lane];
        // register r of lane: row (r & 3) + 8 (r >> 2) + 4 lh -> channel co = 2 row + e; column li -> channel ci = 2 li + f
        const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
        const int oc = cob * 64 + 2 * row + e, ic = cib * 64 + 2 * li + f;
        if (oc < p.Cout) out[(size_t)oc * p.Cin + ic] = v;
    }
}

__global__ void __launch_bounds__(256) wgrad1x1_f16_reduce_kernel(const float *partial, float *dw, const unsigned *amax_dy, int nsplit, size_t n) {
    const float inv = pow2_of(-scale_exponent(*amax_dy));
    for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (size_t)gridDim.x * 256 * 4) {
        f32x4 s = *(const f32x4 *)(partial + i);
        for (int k = 1; k < nsplit; ++k) s = s + *(const f32x4 *)(partial + (size_t)k * n + i);      // index order
        *(f32x4 *)(dw + i) = s * inv;
    }
}

struct Wgrad16Plan { int nsplit, chunks_per_wave; };

Wgrad16Plan wgrad1x1_f16_plan(long M, int Cin, int Cout) {
    const int tiles = ((Cout + 63) / 64) * (Cin / 64);
    const long chunks = (M + 15) / 16;
    const long target = wgrad_target_workgroups(768);             // ~3 workgroups per CU in total at full width
    long nsplit = (target + tiles - 1) / tiles;
    const long max_by_work = (chunks + 31) / 32;                   // at least 8 chunks per wave
    if (nsplit > max_by_work) nsplit = max_by_work;
    if (nsplit < 1) nsplit = 1;
    long cpw = (chunks + nsplit * 4 - 1) / (nsplit * 4);
    cpw = (cpw + 1) / 2 * 2;
    Wgrad16Plan pl;
    pl.chunks_per_wave = (int)cpw;
    pl.nsplit = (int)((chunks + cpw * 4 - 1) / (cpw * 4));
    return pl;
}

int g_conv1x1_f16_ksplit = 0;     // test hook: 0 = by shape, 1 / 2 / 4 = force

template <bool PRE, int EPI, bool RES>
int gemm16_launch_ks(const Gemm16Params &p, int ks, unsigned grid, void *stream) {
    if (ks == 1) hipLaunchKernelGGL((gemm1x1_f16_kernel<1, PRE, EPI, RES>), dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    else if (ks == 2) hipLaunchKernelGGL((gemm1x1_f16_kernel<2, PRE, EPI, RES>), dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((gemm1x1_f16_kernel<4, PRE, EPI, RES>), dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    DREAM_LAUNCH_OK();
    return 0;
}

int gemm16_launch(Gemm16Params p, long M, int K, int N, int x_stride, bool pre, int epi, void *stream) {
    p.M = (int)M; p.K = K; p.N = N; p.NPad = (N + 63) / 64 * 64; p.x_stride = x_stride;
    p.nrb = (int)((M + 63) / 64); p.ncb = p.NPad / 64;
    const long tiles = (long)p.nrb * p.ncb;
    // gemm1x1.hip's levels: split K until the tiles give ~2 waves per SIMD
    int ks = 1;
    if (g_conv1x1_f16_ksplit > 0) ks = g_conv1x1_f16_ksplit;
    else if (tiles < 768 && K % 128 == 0) ks = 4;
    else if (tiles < 2 * 768 && K % 64 == 0) ks = 2;
    DREAM_REQUIRE(K % (32 * ks) == 0, "conv1x1_f16: K=%d cannot be split %d ways", K, ks);
    const int per_wg = 4 / ks;
    const unsigned grid = (unsigned)(((tiles + per_wg - 1) / per_wg + 7) / 8 * 8);
    if (epi == 0) return p.residual != nullptr ? gemm16_launch_ks<false, 0, true>(p, ks, grid, stream) : gemm16_launch_ks<false, 0, false>(p, ks, grid, stream);
    if (epi == 1) return pre ? gemm16_launch_ks<true, 1, false>(p, ks, grid, stream) : gemm16_launch_ks<false, 1, false>(p, ks, grid, stream);
    return gemm16_launch_ks<false, 2, false>(p, ks, grid, stream);
}

}  // namespace

#define DREAM_G16_SHAPE_OK(name, M, K, N, stride)                                                                                          \
    DREAM_REQUIRE(M > 0 && K > 0 && N > 0 && stride >= K, name ": bad shape M=%ld K=%d N=%d stride=%d", M, K, N, stride);                 \
    DREAM_REQUIRE(K % 32 == 0 && N % 4 == 0 && stride % 4 == 0, name ": K %% 32, N %% 4, stride %% 4 (got %d, %d, %d)", K, N, stride);    \
    DREAM_REQUIRE((size_t)M * (size_t)stride * 4 < ((size_t)1 << 31) && (size_t)M * (size_t)N * 4 < ((size_t)1 << 33),                    \
                  name ": tensor too large for 32-bit offsets")

// Test hook: force the K split (0 = by problem size).  The result depends on it only through the summation order.
extern "C" int dream_conv1x1_f16_set_ksplit(int ks) {
    DREAM_REQUIRE(ks == 0 || ks == 1 || ks == 2 || ks == 4, "conv1x1_f16: K split %d", ks);
    g_conv1x1_f16_ksplit = ks;
    return 0;
}

extern "C" size_t dream_conv1x1_weight_halfs(int rows, int K) {
    return (size_t)(K / 16) * (size_t)((rows + 63) / 64 * 64) * 16;
}

// w_oihw [Cout][Cin][1][1] -> packed halfs of w * 2^(*exp_out); mode as dream_pack_conv1x1_weight; scratch: one uint32 (zeroed here)
extern "C" int dream_pack_conv1x1_weight_f16(const float *w_oihw, void *packed, int *exp_out, unsigned *scratch, int Cout, int Cin, int mode,
                                             void *stream) {
    DREAM_REQUIRE(w_oihw && packed && exp_out && scratch && Cout > 0 && Cin > 0 && (mode == 0 || mode == 1), "conv1x1 pack (f16): bad arguments");
    const int rows = mode == 0 ? Cout : Cin, K = mode == 0 ? Cin : Cout;
    DREAM_REQUIRE(K % 32 == 0, "conv1x1 pack (f16): contraction length %d must be a multiple of 32", K);
    if (dream_zero_words(scratch, sizeof(unsigned), (hipStream_t)stream)) return 2;
    const size_t n = (size_t)Cout * Cin;
    size_t g = (n + 255) / 256;
    if (g > 1024) g = 1024;
    hipLaunchKernelGGL(absmax16_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, w_oihw, n, scratch);
    DREAM_LAUNCH_OK();
    const size_t total = dream_conv1x1_weight_halfs(rows, K);
    g = (total + 255) / 256;
    if (g > 2048) g = 2048;
    hipLaunchKernelGGL(gemm1x1_f16_pack_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, w_oihw, (_Float16 *)packed,
                       (const unsigned *)scratch, exp_out, Cout, Cin, mode);
    DREAM_LAUNCH_OK();
    return 0;
}

extern "C" size_t dream_pack16_job_bytes(void) { return sizeof(dream_pack16_job); }

// jobs: DEVICE array of njobs entries; scratch: the njobs uint32 words the jobs' `scratch` fields point into (zeroed here)
extern "C" int dream_pack_conv1x1_weights_f16_batched(const dream_pack16_job *jobs_device, int njobs, unsigned *scratch,
                                                      int workgroups_per_job, void *stream) {
    DREAM_REQUIRE(jobs_device && scratch && njobs > 0 && njobs <= 65535 && workgroups_per_job > 0, "batched pack (f16): bad arguments");
    if (dream_zero_words(scratch, (size_t)njobs * sizeof(unsigned), (hipStream_t)stream)) return 2;
    const dim3 grid((unsigned)workgroups_per_job, (unsigned)njobs);
    hipLaunchKernelGGL(pack16_amax_batched_kernel, grid, dim3(256), 0, (hipStream_t)stream, jobs_device);
    DREAM_LAUNCH_OK();
    hipLaunchKernelGGL(pack16_batched_kernel, grid, dim3(256), 0, (hipStream_t)stream, jobs_device);
    DREAM_LAUNCH_OK();
    return 0;
}

// y[M][N] = half(x * 2^e_x)[M][:K] . half(w * 2^e_w)^T * 2^-(e_x + e_w) + shift (+ residual); amax_x null: e_x = 0, x saturated to half
extern "C" int dream_conv1x1_f16_nhwc_f32(const float *x, const unsigned *amax_x, const void *w_packed, const int *w_exp, const float *shift,
                                          const float *residual, float *y, long M, int K, int N, int x_stride, void *stream) {
    DREAM_REQUIRE(x && w_packed && w_exp && y, "conv1x1_f16: null pointer");
    DREAM_G16_SHAPE_OK("conv1x1_f16", M, K, N, x_stride);
    Gemm16Params p = {};
    p.x = x; p.amax_x = amax_x; p.w = (const _Float16 *)w_packed; p.w_exp = w_exp; p.shift = shift; p.residual = residual; p.y = y;
    return gemm16_launch(p, M, K, N, x_stride, false, 0, stream);
}

// dream_conv1x1_bnstats_nhwc_f32 on the fp16 matrix cores (the activation operand has e_x = 0); workspace / counters: the fp32 form's
extern "C" int dream_conv1x1_bnstats_f16_nhwc_f32(const float *x, const void *w_packed, const int *w_exp, const float *shift,
                                                  const float *pre_ab, float *y, long M, int K, int N, int x_stride, const float *gamma,
                                                  const float *beta, float *running_mean, float *running_var,
                                                  long long *num_batches_tracked, float eps, float momentum, float *out_ab,
                                                  float *save_mean, float *save_invstd, void *workspace, unsigned *counters, void *stream) {
    DREAM_REQUIRE(x && w_packed && w_exp && y && gamma && beta && out_ab && save_mean && save_invstd && workspace && counters,
                  "conv1x1_bnstats_f16: null pointer");
    DREAM_G16_SHAPE_OK("conv1x1_bnstats_f16", M, K, N, x_stride);
    Gemm16Params p = {};
    p.x = x; p.w = (const _Float16 *)w_packed; p.w_exp = w_exp; p.shift = shift; p.y = y; p.pre_ab = pre_ab;
    p.st = stat_tree_make(workspace, counters, (int)((M + 63) / 64), N);
    p.st_fwd.gamma = gamma; p.st_fwd.beta = beta; p.st_fwd.running_mean = running_mean; p.st_fwd.running_var = running_var;
    p.st_fwd.nbt = num_batches_tracked; p.st_fwd.eps = eps; p.st_fwd.momentum = momentum;
    p.st_fwd.ab = out_ab; p.st_fwd.mean = save_mean; p.st_fwd.invstd = save_invstd;
    return gemm16_launch(p, M, K, N, x_stride, pre_ab != nullptr, 1, stream);
}

// dream_conv1x1_bwd_bnmask_nhwc_f32 on the fp16 matrix cores; amax_dy: the scalar the launch that wrote dy published
extern "C" int dream_conv1x1_bwd_bnmask_f16_nhwc_f32(const float *dy, const unsigned *amax_dy, const void *w_packed_t, const int *w_exp,
                                                     const float *residual, float *g_out, long M, int K, int N, int dy_stride,
                                                     const float *z, const float *ab, const float *y_act, const float *mean,
                                                     const float *invstd, float *dgamma, float *dbeta, void *workspace, unsigned *counters,
                                                     void *stream) {
    DREAM_REQUIRE(dy && amax_dy && w_packed_t && w_exp && g_out && z && (ab || y_act) && mean && invstd && dgamma && dbeta && workspace && counters,
                  "conv1x1_bwd_bnmask_f16: null pointer");
    DREAM_G16_SHAPE_OK("conv1x1_bwd_bnmask_f16", M, K, N, dy_stride);
    Gemm16Params p = {};
    p.x = dy; p.amax_x = amax_dy; p.w = (const _Float16 *)w_packed_t; p.w_exp = w_exp; p.y = g_out; p.residual = residual;
    p.st = stat_tree_make(workspace, counters, (int)((M + 63) / 64), N);
    p.st_z = z; p.st_zab = ab; p.st_yact = y_act; p.st_mean = mean; p.st_invstd = invstd;
    p.st_dgamma = dgamma; p.st_dbeta = dbeta;
    return gemm16_launch(p, M, K, N, dy_stride, false, 2, stream);
}

extern "C" size_t dream_conv1x1_wgrad_f16_workspace(long M, int Cin, int Cout) {
    if (M <= 0 || Cin <= 0 || Cout <= 0 || Cin % 64 != 0) return 0;
    const Wgrad16Plan pl = wgrad1x1_f16_plan(M, Cin, Cout);
    return (size_t)pl.nsplit * Cout * Cin * sizeof(float);
}

// x [M][Cin] (pre_ab: the input of a BatchNorm + ReLU applied while loading), dy [M][Cdy >= Cout] with its amax -> dw [Cout][Cin],
// overwritten.  Cin % 64 == 0, Cout % 4 == 0, Cdy % 4 == 0; workspace: dream_conv1x1_wgrad_f16_workspace() bytes.
extern "C" int dream_conv1x1_wgrad_f16_nhwc_f32(const float *x, const float *dy, const unsigned *amax_dy, float *dw, void *workspace, long M,
                                                int Cin, int Cout, int Cdy, const float *pre_ab, void *stream) {
    DREAM_REQUIRE(x && dy && amax_dy && dw && workspace, "conv1x1 wgrad (f16): null pointer");
    DREAM_REQUIRE(M > 0 && Cin > 0 && Cout > 0 && Cdy >= Cout, "conv1x1 wgrad (f16): bad shape");
    DREAM_REQUIRE(Cin % 64 == 0 && Cout % 4 == 0 && Cdy % 4 == 0, "conv1x1 wgrad (f16): Cin %% 64, Cout %% 4, Cdy %% 4 (got %d, %d, %d)", Cin, Cout, Cdy);
    DREAM_REQUIRE((size_t)(M + 64) * (size_t)(Cin > Cdy ? Cin : Cdy) * 4 < ((size_t)1 << 31), "conv1x1 wgrad (f16): tensor too large for 32-bit offsets");
    const Wgrad16Plan pl = wgrad1x1_f16_plan(M, Cin, Cout);
    Wgrad16Params p;
    p.x = x; p.dy = dy; p.amax_dy = amax_dy; p.partial = (float *)workspace;
    p.M = (int)M; p.Cin = Cin; p.Cout = Cout; p.Cdy = Cdy;
    p.ncob = (Cout + 63) / 64; p.ncib = Cin / 64;
    p.chunks_per_wave = pl.chunks_per_wave;
    p.pre_ab = pre_ab;
    const dim3 wgrid((unsigned)(p.ncob * p.ncib * pl.nsplit));
    if (pre_ab != nullptr) hipLaunchKernelGGL(wgrad1x1_f16_kernel<true>, wgrid, dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(wgrad1x1_f16_kernel<false>, wgrid, dim3(256), 0, (hipStream_t)stream, p);
    DREAM_LAUNCH_OK();
    const size_t n = (size_t)Cout * Cin;
    size_t rgrid = (n / 4 + 255) / 256;
    if (rgrid > 1024) rgrid = 1024;
    hipLaunchKernelGGL(wgrad1x1_f16_reduce_kernel, dim3((unsigned)rgrid), dim3(256), 0, (hipStream_t)stream, (const float *)workspace, dw,
                       amax_dy, pl.nsplit, n);
    DREAM_LAUNCH_OK();
    return 0;
}
