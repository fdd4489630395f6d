// The two steps immediately BEFORE the hot path, moved onto the device so that a training
// step no longer uploads 245.8 MB of normalised fp32 frames + 35.8 MB of fp32 targets per batch of 128:
//   * ToTensor + Normalize(mean, stdev) of uint8 RGB frames  (/root/reference/dream/datasets.py:87-94,
//     /root/reference/dream/network.py:449-459): out = ((u8 / 255) - mean) / stdev in IEEE fp32, HWC -> CHW;
//   * create_belief_map  (/root/reference/dream/image_proc.py:866-910): a (4*sigma+1)^2 Gaussian blob stamped at
//     the int()-truncated keypoint when the window (plus one) fits, otherwise an all-zero map.  The blob values
//     are computed on the host in float64 with NumPy exactly as the reference does and cast to fp32 there, so
//     the device result is bit-identical to `torch.tensor(create_belief_map(...)).float()`.
// Both are pure streaming kernels (HBM-bound: 3 B in / 12 B out per pixel, resp. 4 B out per map pixel).
#include <dream_cdna4.h>
#include "common.h"
#include "../../include/dream_hip.h"

namespace {

__global__ void __launch_bounds__(256) normalize_u8_kernel(const unsigned char *img, float *out, int B, int H, int W,
                                                           float m0, float m1, float m2, float s0, float s1, float s2) {
    const size_t npix = (size_t)B * H * W;
    const size_t hw = (size_t)H * W;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (size_t)gridDim.x * 256) {
        const size_t b = i / hw, p = i - b * hw;
        const unsigned char *src = img + i * 3;
        float *dst = out + b * 3 * hw + p;
        dst[0] = (((float)src[0] / 255.0f) - m0) / s0;
        dst[hw] = (((float)src[1] / 255.0f) - m1) / s1;
        dst[2 * hw] = (((float)src[2] / 255.0f) - m2) / s2;
    }
}

__global__ void __launch_bounds__(256) belief_maps_kernel(const double *kps, const float *blob, float *out, int N, int H, int W,
                                                          int w) {
    const int side = 2 * w + 1;
    const size_t total = (size_t)N * H * W;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int x = (int)(i % W);
        const size_t r = i / W;
        const int y = (int)(r % H);
        const size_t n = r / H;
        // Python's int() on the reference's float64 coordinate: truncation toward zero, done on the float64 value
        // (57.9999999 must stay pixel 57; an fp32 upload would round it to 58).  Clamped so the cast is defined.
        const int u = (int)fmin(fmax(kps[n * 2 + 0], -1.0e9), 1.0e9), v = (int)fmin(fmax(kps[n * 2 + 1], -1.0e9), 1.0e9);
        float val = 0.0f;
        if (u - w >= 0 && u + w + 1 < W && v - w >= 0 && v + w + 1 < H) {
            const int dx = x - u, dy = y - v;
            if (dx >= -w && dx <= w && dy >= -w && dy <= w) val = blob[(dy + w) * side + (dx + w)];
        }
        out[i] = val;
    }
}

// Raw camera frame -> network input (dream/image_proc.py:26-51 preprocess_image + :291-351, then ToTensor + Normalize as
// dream/network.py:449-459), batched: optional crop, PIL's 8-bit BILINEAR resize, normalise.  Bit-identical to Pillow's
// Resample.c: per-axis int32 coefficients (float64 weights scaled by 2^22 and rounded, built on the host), a horizontal
// pass over the rows the vertical pass needs, rounded to uint8 (clip8), then the vertical pass on those uint8 rows,
// rounded to uint8 again.  The intermediate rounding is part of the result, so the intermediate stays uint8.
//
// One workgroup = 64 output columns x `tile_rows` output rows of one frame.  LDS (dynamic, 16-byte aligned):
//   in_s  [span_rows][rs]    the tile's input window (crop-relative rows r0.., columns c0..), copied with 16-byte loads from
//                            a 16-byte aligned global address; each row starts `shift` bytes into its LDS row;
//   mid_s [span_rows][192]   horizontal pass: uint8 RGB of the 64 output columns for every input row of the window;
//   hk_s / hb_s, vk_s / vb_s the tile's coefficients and (lo, n) bounds.
// The vertical pass and the normalise store each fp32 plane row as 64 consecutive floats per wave.
constexpr int kPrepTileW = 64;
constexpr int kPrepMidRow = kPrepTileW * 3;
typedef unsigned u32x4_prep __attribute__((ext_vector_type(4)));

__device__ inline unsigned char prep_clip8(int acc) {
    return acc <= 0 ? 0 : (acc >= (255 << 22) ? 255 : (unsigned char)(acc >> 22));
}

__global__ void __launch_bounds__(256) preprocess_frames_kernel(
    const unsigned char *img, float *out, unsigned char *out_u8, int B, int H, int W, int cx, int cy, int OH, int OW,
    const int *hb, const int *hk, int ksx, const int *vb, const int *vk, int ksy, int tile_rows, int span_rows, int span_cols,
    int rs, int ntx, int nty, float m0, float m1, float m2, float s0, float s1, float s2) {
    DREAM_DYNAMIC_LDS(unsigned char, lds);
    unsigned char *in_s = lds;
    unsigned char *mid_s = in_s + (size_t)span_rows * rs;
    int *hk_s = (int *)(mid_s + (size_t)span_rows * kPrepMidRow);
    int *hb_s = hk_s + kPrepTileW * ksx;
    int *vk_s = hb_s + kPrepTileW * 2;
    int *vb_s = vk_s + tile_rows * ksy;

    const int tid = threadIdx.x;
    const int tx = blockIdx.x % ntx, ty = (blockIdx.x / ntx) % nty, b = blockIdx.x / (ntx * nty);
    const int ox0 = tx * kPrepTileW, oy0 = ty * tile_rows;
    const int ncol = OW - ox0 < kPrepTileW ? OW - ox0 : kPrepTileW, nrow_out = OH - oy0 < tile_rows ? OH - oy0 : tile_rows;
    // crop-relative input window of the tile (Pillow's bounds are monotone in the output index)
    const int c0 = hb[2 * ox0], c1 = hb[2 * (ox0 + ncol - 1)] + hb[2 * (ox0 + ncol - 1) + 1];
    const int r0 = vb[2 * oy0], r1 = vb[2 * (oy0 + nrow_out - 1)] + vb[2 * (oy0 + nrow_out - 1) + 1];
    const int nrows = r1 - r0, ncols = c1 - c0;
    if (nrows > span_rows || ncols > span_cols) {
        // the caller's span sizes do not cover this tile: nothing is read into LDS, the tile is marked NaN
        for (int i = tid; i < 3 * nrow_out * kPrepTileW; i += 256) {
            const int x = i % kPrepTileW, y = (i / kPrepTileW) % nrow_out, c = i / (kPrepTileW * nrow_out);
            if (x < ncol && out) out[(((size_t)b * 3 + c) * OH + oy0 + y) * OW + ox0 + x] = __builtin_nanf("");
        }
        return;
    }

    for (int i = tid; i < kPrepTileW * ksx; i += 256) {
        const int x = i / ksx;
        hk_s[i] = x < ncol ? hk[(size_t)(ox0 + x) * ksx + i % ksx] : 0;
    }
    for (int i = tid; i < kPrepTileW * 2; i += 256) hb_s[i] = (i >> 1) < ncol ? hb[2 * ox0 + i] : 0;
    for (int i = tid; i < tile_rows * ksy; i += 256) {
        const int y = i / ksy;
        vk_s[i] = y < nrow_out ? vk[(size_t)(oy0 + y) * ksy + i % ksy] : 0;
    }
    for (int i = tid; i < tile_rows * 2; i += 256) vb_s[i] = (i >> 1) < nrow_out ? vb[2 * oy0 + i] : 0;

    // input window -> LDS, 16 bytes per lane from the 16-byte aligned address at or below each row's first byte.  The frame
    // buffer is 16-byte aligned (checked on the host); a chunk that would run past its end is read byte by byte.
    const size_t total = (size_t)B * H * W * 3;
    const int chunks = rs / 16;
    for (int i = tid; i < nrows * chunks; i += 256) {
        const int r = i / chunks, j = i - r * chunks;
        const size_t start = (((size_t)b * H + cy + r0 + r) * W + cx + c0) * 3;
        const int shift = (int)(start & 15);
        if (16 * j >= shift + ncols * 3) continue;
        const size_t g = (start & ~(size_t)15) + 16 * (size_t)j;
        u32x4_prep v;
        if (g + 16 <= total) {
            v = *(const u32x4_prep *)(img + g);
        } else {
            unsigned char tmp[16];
            for (int k = 0; k < 16; ++k) tmp[k] = g + k < total ? img[g + k] : 0;
            __builtin_memcpy(&v, tmp, 16);
        }
        *(u32x4_prep *)(in_s + (size_t)r * rs + 16 * j) = v;
    }
    __syncthreads();

    // horizontal pass: lane = output column, the four waves stride over the window's rows
    const int x = tid & (kPrepTileW - 1);
    if (x < ncol) {
        const int lo = hb_s[2 * x] - c0, n = hb_s[2 * x + 1];
        const int *k = hk_s + x * ksx;
        for (int r = tid >> 6; r < nrows; r += 4) {
            const size_t start = (((size_t)b * H + cy + r0 + r) * W + cx + c0) * 3;
            const unsigned char *p = in_s + (size_t)r * rs + (start & 15) + lo * 3;
            int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
            for (int t = 0; t < n; ++t) {
                a0 += (int)p[3 * t] * k[t];
                a1 += (int)p[3 * t + 1] * k[t];
                a2 += (int)p[3 * t + 2] * k[t];
            }
            unsigned char *q = mid_s + (size_t)r * kPrepMidRow + 3 * x;
            q[0] = prep_clip8(a0);
            q[1] = prep_clip8(a1);
            q[2] = prep_clip8(a2);
        }
    }
    __syncthreads();

    // vertical pass + ToTensor + Normalize: each wave stores whole 64-float runs of a plane row
    if (x < ncol) {
        const int ox = ox0 + x;
        for (int y = tid >> 6; y < nrow_out; y += 4) {
            const int lo = vb_s[2 * y] - r0, n = vb_s[2 * y + 1];
            const int *k = vk_s + y * ksy;
            const unsigned char *p = mid_s + (size_t)lo * kPrepMidRow + 3 * x;
            int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
            for (int t = 0; t < n; ++t) {
                a0 += (int)p[t * kPrepMidRow] * k[t];
                a1 += (int)p[t * kPrepMidRow + 1] * k[t];
                a2 += (int)p[t * kPrepMidRow + 2] * k[t];
            }
            const unsigned char v0 = prep_clip8(a0), v1 = prep_clip8(a1), v2 = prep_clip8(a2);
            const int oy = oy0 + y;
            const size_t plane = (size_t)OH * OW, o = ((size_t)b * 3 * OH + oy) * OW + ox;
            if (out) {                          // NULL: only the resized uint8 frames are wanted (the augmentation reads those)
                out[o] = (((float)v0 / 255.0f) - m0) / s0;
                out[o + plane] = (((float)v1 / 255.0f) - m1) / s1;
                out[o + 2 * plane] = (((float)v2 / 255.0f) - m2) / s2;
            }
            if (out_u8) {
                unsigned char *d = out_u8 + (((size_t)b * OH + oy) * OW + ox) * 3;
                d[0] = v0;
                d[1] = v1;
                d[2] = v2;
            }
        }
    }
}

inline unsigned sgrid(size_t n) {
    size_t g = (n + 255) / 256;
    if (g > 2048) g = 2048;
    return (unsigned)(g ? g : 1);
}
// Keypoint frame conversion right after peak extraction (dream/image_proc.py:135-147 net-output -> net-input,
// :215-260 net-input -> raw image): two affine maps in float64 with the reference's operation order (divide, then
// multiply, then add), applied to every row including the -999.999 sentinels, as the reference does.
//   netin = k / out_res * in_res            raw = netin                      (mode 0: "none")
//                                           raw = netin / in_res * span + origin   (mode 1: resize / shrink /
//                                                 shrink-and-crop; span / origin = raw or cropped resolution / corner)
__global__ void __launch_bounds__(256) convert_keypoints_kernel(const float *kps, double *netin, double *raw, int N,
                                                                double ow, double oh, double iw, double ih, double sw,
                                                                double sh, double x0, double y0, int mode) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const double nx = dmul(ddiv((double)kps[2 * i], ow), iw), ny = dmul(ddiv((double)kps[2 * i + 1], oh), ih);
    netin[2 * i] = nx;
    netin[2 * i + 1] = ny;
    if (mode == 0) {
        raw[2 * i] = nx;
        raw[2 * i + 1] = ny;
    } else {
        raw[2 * i] = dadd(dmul(ddiv(nx, iw), sw), x0);
        raw[2 * i + 1] = dadd(dmul(ddiv(ny, ih), sh), y0);
    }
}

// ---- training batches from raw frames (dream/datasets.py:127-208 on the device) ------------------------------------
// One row of the augmentation parameter table per frame, 16 doubles: [0..5] the forward 2x3 affine matrix in net-input pixel
// coordinates (keypoints), [6..11] its inverse (image), [12] noise sigma, [13] contrast alpha, [14] brightness beta (fp32 values),
// [15] the 32-bit noise seed.
constexpr int kAugRow = 16;
constexpr int kAugChunk = 16384;         // frame bytes per workgroup of the noise / sum pass
constexpr int kAugQuantiles = 4096;      // entries of the standard-normal quantile table (indexed by the top 12 hash bits)

// Keypoints of a training batch, float64 with individually rounded operations in the reference's order: raw frame -> net input
// (image_proc.py:165-212: mode 0 "none"; mode 1 (k - origin) / span * target, origin 0 for "resize" / "shrink") -> k' = M k for
// a non-identity table row -> net output (image_proc.py:150-162) -> float32 (datasets.py:190-192), also widened back to float64
// for belief_maps_kernel, which truncates it like create_belief_map's int() does.
__global__ void __launch_bounds__(256) training_keypoints_kernel(const double *raw, const double *table, double *netin,
                                                                 float *netout32, double *netout64, int N, int K, int mode,
                                                                 double x0, double y0, double sw, double sh, double tw, double th,
                                                                 double iw, double ih, double ow, double oh) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    double x = raw[2 * i], y = raw[2 * i + 1];
    if (mode) {
        x = dmul(ddiv(dadd(x, -x0), sw), tw);
        y = dmul(ddiv(dadd(y, -y0), sh), th);
    }
    if (table) {
        const double *m = table + (size_t)(i / K) * kAugRow;
        if (!(m[0] == 1.0 && m[1] == 0.0 && m[2] == 0.0 && m[3] == 0.0 && m[4] == 1.0 && m[5] == 0.0)) {
            const double ax = dadd(dadd(dmul(m[0], x), dmul(m[1], y)), m[2]);
            const double ay = dadd(dadd(dmul(m[3], x), dmul(m[4], y)), m[5]);
            x = ax;
            y = ay;
        }
    }
    netin[2 * i] = x;
    netin[2 * i + 1] = y;
    const float fx = (float)dmul(ddiv(x, iw), ow), fy = (float)dmul(ddiv(y, ih), oh);
    netout32[2 * i] = fx;
    netout32[2 * i + 1] = fy;
    netout64[2 * i] = (double)fx;
    netout64[2 * i + 1] = (double)fy;
}

// murmur3's 32-bit finaliser over (frame seed, linear index of pixel and channel in the net-input frame): a pure function of the
// source position, so the noise does not depend on the launch geometry or on the frame's place in the batch.
__device__ inline unsigned aug_mix(unsigned seed, unsigned idx) {
    unsigned h = seed + idx * 0x9E3779B9u;
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

__device__ inline int aug_round_clip(float v) {        // rint (half to even), then clip to 0..255; NaN -> 0
    v = rintf(v);
    return !(v > 0.0f) ? 0 : (v >= 255.0f ? 255 : (int)v);
}

// Pass 1: n(p) = clip(rint(float(u(p)) + sigma * z(p))) for every byte of the resized frames, stored as uint8, and the integer sum of
// each workgroup's kAugChunk bytes (wave shuffles, LDS, one partial per workgroup: exact, so the order is free).
__global__ void __launch_bounds__(256) augment_noise_kernel(const unsigned char *u8, const double *table, const float *quantiles,
                                                            unsigned char *noised, unsigned long long *partials, int n, int G) {
    __shared__ float z_s[kAugQuantiles];
    __shared__ int wave_sum[4];
    const int tid = threadIdx.x, b = blockIdx.x / G, g = blockIdx.x - b * G;
    const float sigma = (float)table[(size_t)b * kAugRow + 12];
    const unsigned seed = (unsigned)table[(size_t)b * kAugRow + 15];
    const bool noisy = sigma != 0.0f;
    if (noisy)
        for (int i = tid; i < kAugQuantiles; i += 256) z_s[i] = quantiles[i];
    __syncthreads();
    const int i0 = g * kAugChunk, i1 = n - i0 < kAugChunk ? n : i0 + kAugChunk;
    const unsigned char *src = u8 + (size_t)b * n;
    unsigned char *dst = noised + (size_t)b * n;
    int sum = 0;
    for (int i = i0 + tid; i < i1; i += 256) {
        int v = src[i];
        if (noisy) {
            const float t = sigma * z_s[aug_mix(seed, (unsigned)i) >> 20];
            v = aug_round_clip((float)v + t);
        }
        dst[i] = (unsigned char)v;
        sum += v;
    }
    for (int m = 32; m >= 1; m >>= 1) sum += lane_xor(sum, m);
    if ((tid & 63) == 0) wave_sum[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) partials[blockIdx.x] = (unsigned long long)(wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3]);
}

// Between the passes: m = fp32(sum / count in float64) of the noised frame and beta * m, once per frame.
__global__ void __launch_bounds__(64) augment_mean_kernel(const unsigned long long *partials, const double *table, float *mean,
                                                          float *beta_mean, int n, int G) {
    __shared__ unsigned long long s[64];
    const int tid = threadIdx.x, b = blockIdx.x;
    unsigned long long t = 0;
    for (int g = tid; g < G; g += 64) t += partials[(size_t)b * G + g];
    s[tid] = t;
    __syncthreads();
    if (tid == 0) {
        unsigned long long total = 0;
        for (int i = 0; i < 64; ++i) total += s[i];
        const float m = (float)ddiv((double)total, (double)n);
        mean[b] = m;
        beta_mean[b] = (float)table[(size_t)b * kAugRow + 14] * m;
    }
}

__device__ inline int aug_reflect101(long long i, int n) {     // -1 -> 1, n -> n - 2, periodic
    if (i >= 0 && i < n) return (int)i;
    if (n == 1) return 0;
    const long long p = 2 * (long long)(n - 1);
    long long r = i % p;
    if (r < 0) r += p;
    return (int)(r < n ? r : p - r);
}

__device__ inline long long aug_fixed5(double s) {              // floor(s * 32 + 0.5), kept inside +-2^40
    const double f = floor(dadd(dmul(s, 32.0), 0.5));
    return (long long)fmin(fmax(f, -1099511627776.0), 1099511627776.0);
}

// Pass 2: one thread per output pixel.  Source position M^-1 (x, y) in float64, 5 fractional bits, four reflect-101 taps of the
// noised frame, each through the brightness / contrast c = clip(rint(alpha * n + beta * m)), integer bilinear blend, then ToTensor +
// Normalize with normalize_u8_kernel's arithmetic.  The 64 lanes of a wave store 64 consecutive floats of each plane.
__global__ void __launch_bounds__(256) augment_warp_kernel(const unsigned char *noised, const double *table, const float *beta_mean,
                                                           float *out, unsigned char *out_u8, int H, int W, int chunks, float m0,
                                                           float m1, float m2, float s0, float s1, float s2) {
    const int b = blockIdx.x / chunks, p = (blockIdx.x - b * chunks) * 256 + threadIdx.x;
    const int hw = H * W;
    if (p >= hw) return;
    const int y = p / W, x = p - y * W;
    const double *row = table + (size_t)b * kAugRow;
    const float alpha = (float)row[13], bm = beta_mean[b];
    const double sx = dadd(dadd(dmul(row[6], (double)x), dmul(row[7], (double)y)), row[8]);
    const double sy = dadd(dadd(dmul(row[9], (double)x), dmul(row[10], (double)y)), row[11]);
    const long long X = aug_fixed5(sx), Y = aug_fixed5(sy);
    const int fx = (int)(X & 31), fy = (int)(Y & 31);
    const int xa = aug_reflect101(X >> 5, W), xb = aug_reflect101((X >> 5) + 1, W);
    const int ya = aug_reflect101(Y >> 5, H), yb = aug_reflect101((Y >> 5) + 1, H);
    const int w00 = (32 - fx) * (32 - fy), w10 = fx * (32 - fy), w01 = (32 - fx) * fy, w11 = fx * fy;
    const unsigned char *src = noised + (size_t)b * hw * 3;
    const unsigned char *t00 = src + ((size_t)ya * W + xa) * 3, *t10 = src + ((size_t)ya * W + xb) * 3;
    const unsigned char *t01 = src + ((size_t)yb * W + xa) * 3, *t11 = src + ((size_t)yb * W + xb) * 3;
    int v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a00 = alpha * (float)t00[c], a10 = alpha * (float)t10[c], a01 = alpha * (float)t01[c], a11 = alpha * (float)t11[c];
        const int acc = w00 * aug_round_clip(a00 + bm) + w10 * aug_round_clip(a10 + bm) + w01 * aug_round_clip(a01 + bm) +
                        w11 * aug_round_clip(a11 + bm);
        v[c] = (acc + 512) >> 10;
    }
    float *dst = out + (size_t)b * 3 * hw + p;
    dst[0] = (((float)v[0] / 255.0f) - m0) / s0;
    dst[hw] = (((float)v[1] / 255.0f) - m1) / s1;
    dst[2 * (size_t)hw] = (((float)v[2] / 255.0f) - m2) / s2;
    if (out_u8) {
        unsigned char *d = out_u8 + ((size_t)b * hw + p) * 3;
        d[0] = (unsigned char)v[0];
        d[1] = (unsigned char)v[1];
        d[2] = (unsigned char)v[2];
    }
}

}  // namespace

extern "C" int dream_training_keypoints_f64(const double *kps_raw, const double *aug_table, double *kps_netin, float *kps_netout_f32,
                                            double *kps_netout_f64, int B, int K, int mode, double origin_x, double origin_y,
                                            double span_w, double span_h, double target_w, double target_h, double in_w,
                                            double in_h, double out_w, double out_h, void *stream) {
    DREAM_REQUIRE(kps_raw && kps_netin && kps_netout_f32 && kps_netout_f64 && B > 0 && K > 0 && (long)B * K < (1l << 30) &&
                  (mode == 0 || mode == 1) && in_w > 0 && in_h > 0 && out_w > 0 && out_h > 0,
                  "training_keypoints: bad arguments");
    DREAM_REQUIRE(mode == 0 || (span_w > 0 && span_h > 0 && target_w > 0 && target_h > 0), "training_keypoints: bad span / target");
    const int N = B * K;
    hipLaunchKernelGGL(training_keypoints_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, kps_raw, aug_table,
                       kps_netin, kps_netout_f32, kps_netout_f64, N, K, mode, origin_x, origin_y, span_w, span_h, target_w, target_h,
                       in_w, in_h, out_w, out_h);
    DREAM_LAUNCH_OK();
    return 0;
}

extern "C" size_t dream_augment_partials_per_frame(int H, int W) {
    if (H <= 0 || W <= 0) return 0;
    return ((size_t)H * W * 3 + kAugChunk - 1) / kAugChunk;
}

extern "C" int dream_augment_frames_u8_f32(const unsigned char *frames_u8, const double *aug_table, const float *quantiles,
                                           unsigned char *noised, uint64_t *partials, float *frame_mean, float *beta_mean,
                                           float *out, unsigned char *out_u8, int B, int H, int W, const float *mean3,
                                           const float *stdev3, void *stream) {
    DREAM_REQUIRE(frames_u8 && aug_table && quantiles && noised && partials && frame_mean && beta_mean && out && mean3 && stdev3 &&
                  B > 0 && H > 0 && W > 0, "augment_frames: bad arguments");
    DREAM_REQUIRE(noised != frames_u8 && out_u8 != noised, "augment_frames: the noised frames need a buffer of their own");
    const size_t n = (size_t)H * W * 3, G = dream_augment_partials_per_frame(H, W), chunks = ((size_t)H * W + 255) / 256;
    DREAM_REQUIRE(n < (1ul << 31) && G * B < (1ul << 31) && chunks * B < (1ul << 31), "augment_frames: batch too large");
    hipLaunchKernelGGL(augment_noise_kernel, dim3((unsigned)(G * B)), dim3(256), 0, (hipStream_t)stream, frames_u8, aug_table,
                       quantiles, noised, (unsigned long long *)partials, (int)n, (int)G);
    DREAM_LAUNCH_OK();
    hipLaunchKernelGGL(augment_mean_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream,
                       (const unsigned long long *)partials, aug_table, frame_mean, beta_mean, (int)n, (int)G);
    DREAM_LAUNCH_OK();
    hipLaunchKernelGGL(augment_warp_kernel, dim3((unsigned)(chunks * B)), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char *)noised, aug_table, (const float *)beta_mean, out, out_u8, H, W, (int)chunks, mean3[0],
                       mean3[1], mean3[2], stdev3[0], stdev3[1], stdev3[2]);
    DREAM_LAUNCH_OK();
    return 0;
}

extern "C" int dream_normalize_u8_hwc_to_chw_f32(const unsigned char *img, float *out, int B, int H, int W,
                                                 const float *mean3, const float *stdev3, void *stream) {
    DREAM_REQUIRE(img && out && mean3 && stdev3 && B > 0 && H > 0 && W > 0, "normalize_u8: bad arguments");
    hipLaunchKernelGGL(normalize_u8_kernel, dim3(sgrid((size_t)B * H * W)), dim3(256), 0, (hipStream_t)stream, img, out, B, H, W,
                       mean3[0], mean3[1], mean3[2], stdev3[0], stdev3[1], stdev3[2]);
    DREAM_LAUNCH_OK();
    return 0;
}

// LDS bytes of preprocess_frames_kernel for the given plan (the layout at the kernel; the input row padded for the alignment shift)
static size_t preprocess_lds_bytes(int tile_rows, int span_rows, int span_cols, int ksx, int ksy, int *rs) {
    *rs = ((span_cols * 3 + 15) + 15) / 16 * 16;
    return (size_t)span_rows * (*rs + kPrepMidRow) + 4 * ((size_t)kPrepTileW * (ksx + 2) + (size_t)tile_rows * (ksy + 2));
}

extern "C" int dream_preprocess_frames_u8_f32(const unsigned char *frames, float *out, unsigned char *out_u8, int B, int H, int W,
                                              int crop_x0, int crop_y0, int crop_w, int crop_h, int OH, int OW,
                                              const int32_t *hbounds, const int32_t *hcoeffs, int ksize_x,
                                              const int32_t *vbounds, const int32_t *vcoeffs, int ksize_y, int tile_rows,
                                              int span_rows, int span_cols, const float *mean3, const float *stdev3,
                                              void *stream) {
    DREAM_REQUIRE(frames && (out || out_u8) && hbounds && hcoeffs && vbounds && vcoeffs && mean3 && stdev3 && B > 0 && H > 0 && W > 0 &&
                  OH > 0 && OW > 0 && ksize_x > 0 && ksize_y > 0 && tile_rows > 0 && span_rows > 0 && span_cols > 0,
                  "preprocess_frames: bad arguments");
    DREAM_REQUIRE(crop_x0 >= 0 && crop_y0 >= 0 && crop_w > 0 && crop_h > 0 && crop_x0 + crop_w <= W && crop_y0 + crop_h <= H,
                  "preprocess_frames: crop window (%d,%d)+(%d,%d) outside the %dx%d frame", crop_x0, crop_y0, crop_w, crop_h, W, H);
    DREAM_REQUIRE(span_rows <= crop_h && span_cols <= crop_w, "preprocess_frames: span (%d rows, %d columns) exceeds the crop",
                  span_rows, span_cols);
    DREAM_REQUIRE(((uintptr_t)frames & 15) == 0, "preprocess_frames: the frame buffer must be 16-byte aligned");
    int rs = 0;
    const size_t lds = preprocess_lds_bytes(tile_rows, span_rows, span_cols, ksize_x, ksize_y, &rs);
    DREAM_REQUIRE(lds <= 65536, "preprocess_frames: %zu bytes of LDS (tile_rows %d, span %dx%d): use fewer tile rows", lds,
                  tile_rows, span_rows, span_cols);
    const int ntx = ceil_div(OW, kPrepTileW), nty = ceil_div(OH, tile_rows);
    DREAM_REQUIRE((long)ntx * nty * B < (1l << 31), "preprocess_frames: batch too large");
    hipLaunchKernelGGL(preprocess_frames_kernel, dim3((unsigned)(ntx * nty * B)), dim3(256), lds, (hipStream_t)stream, frames, out,
                       out_u8, B, H, W, crop_x0, crop_y0, OH, OW, (const int *)hbounds, (const int *)hcoeffs, ksize_x,
                       (const int *)vbounds, (const int *)vcoeffs, ksize_y, tile_rows, span_rows, span_cols, rs, ntx, nty,
                       mean3[0], mean3[1], mean3[2], stdev3[0], stdev3[1], stdev3[2]);
    DREAM_LAUNCH_OK();
    return 0;
}

// kps: [N,2] (x, y) FLOAT64 device (the reference truncates the float64 coordinate); blob: [(2w+1)^2] fp32 device (host-computed, see above); out: [N,H,W]
extern "C" int dream_create_belief_maps_f32(const float *, const float *, float *, int, int, int, int, void *) {
    DREAM_REQUIRE(false, "dream_create_belief_maps_f32 (fp32 keypoints, ABI 1) was withdrawn: pass float64 keypoints to "
                         "dream_create_belief_maps_f64kps_f32");
    return 1;
}

extern "C" int dream_create_belief_maps_f64kps_f32(const double *kps, const float *blob, float *out, int N, int H, int W, int w,
                                                   void *stream) {
    DREAM_REQUIRE(kps && blob && out && N > 0 && H > 0 && W > 0 && w >= 0, "create_belief_maps: bad arguments");
    hipLaunchKernelGGL(belief_maps_kernel, dim3(sgrid((size_t)N * H * W)), dim3(256), 0, (hipStream_t)stream, kps, blob, out, N, H,
                       W, w);
    DREAM_LAUNCH_OK();
    return 0;
}

extern "C" int dream_convert_keypoints_f64(const float *kps_netout, double *kps_netin, double *kps_raw, int N,
                                           double out_w, double out_h, double in_w, double in_h, double span_w,
                                           double span_h, double origin_x, double origin_y, int mode, void *stream) {
    DREAM_REQUIRE(kps_netout && kps_netin && kps_raw && N > 0 && out_w > 0 && out_h > 0 && in_w > 0 && in_h > 0 &&
                  (mode == 0 || mode == 1), "convert_keypoints: bad arguments");
    hipLaunchKernelGGL(convert_keypoints_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, kps_netout, kps_netin,
                       kps_raw, N, out_w, out_h, in_w, in_h, span_w, span_h, origin_x, origin_y, mode);
    DREAM_LAUNCH_OK();
    return 0;
}
