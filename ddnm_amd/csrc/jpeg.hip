// JPEG-artifact restoration: quantisation-cell projection in one fused step kernel -- gfx950.
//
// T (linear) = the planes of chroma subsampling (ddnm_step.hip: Y = w_Y . x at every pixel, Cb / Cr averaged over sites of
// rw columns x rh rows) followed, per plane and per 8 x 8 block, by the orthonormal 2-D DCT-II  C X C^T,
//   C[k][n] = s_k cos((2n + 1) k pi / 16),  s_0 = sqrt(1/8),  s_k = sqrt(2/8).
// Layout in place: coefficient (u, v) of block (I, J) sits at plane position (8 I + u, 8 J + v); a row is [ Y | Cb | Cr ],
// each plane row-major: H W (1 + 2 / (rw rh)) entries, a multiple of 4.  T has full row rank and T^+ = A_chroma^+ . IDCT is
// its exact pseudo-inverse (an orthogonal factor on the left does not change one):
//   (T^+ c)[:, p] = w+ (Y_p - Ybar) + M^-1 (Ybar, Cb, Cr)^T,   (Y, Cb, Cr) = the block-IDCT of c.
// Encoder:  y = q rint((T x - delta) / q) + delta  (the dequantised cell centre; delta = the level shift, luma DC only).
// Step, with h = box q / 2:
//   x0  = (xt - et sqrt_1m_at) / sqrt_at
//   c   = T x0
//   x0h = x0 - lambda T^+(c - clamp(c, y - h, y + h))
//   xt' = sqrt_at_next x0h + c1 noise + c2 et
// h = 0 is x0 - lambda T^+(T x0 - y); with h half a step the result re-encodes to the measured levels.
//
// Work split (every kernel here).  The unit is the MCU: 8 rw x 8 rh pixels, rw rh luma blocks and one Cb and one Cr block
// (NB = rw rh + 2).  MCUs are numbered row-major over the batch and a workgroup of 256 threads owns G = 16 / rw consecutive
// ones (a power of two; the last workgroup may hold fewer).  Thread t owns one STRIP of its workgroup: rh rows x 4 pixels
// x 3 planes -- column group t % (2 rw), MCU (t / (2 rw)) % G, site row t / 32 -- so the 32 lanes of a half-wave lie along
// one image row across the G MCUs (512 contiguous bytes where the MCUs are neighbours) and a strip holds whole chroma
// sites.  The strip's x0 and et stay in registers from the load to the update: xt, et, noise and y are read once, x0 and
// xt' written once, nothing goes through global scratch.
// LDS: CL = NBLK = G NB blocks of 8 x 8 floats, block stride 72 (8 floats of padding: the 8 lanes of a block read a column
// with stride 8, and the four blocks of a 32-lane group then start 8 banks apart), YL the same for y (step kernel), 128
// floats of q or h.  27.6 KB + 0.5 KB for 4:2:0 and 4:4:4, 18.4 KB + 0.5 KB for 4:2:2.
// Passes, one thread per (block, row or column), 8 NBLK = 256 or 384 tasks:
//   rows:    read row i (two 16-byte reads), 8-point DCT in registers, write it back
//   columns: read column v (stride 8: the first transpose), DCT -> coefficients (0..7, v) in registers; there clamp
//            against column v of y and h (step), quantise (encoder) or nothing (T); IDCT over u in registers (step) and
//            write column v back (the second transpose)
//   rows:    IDCT along v (step, T^+)
// The 8-point transforms are the even/odd split with explicit fmaf; everything else rounds mul and add separately like
// the other step kernels (x0 is bit for bit that of ddnm_step_x0_f32).
#include "common.h"
#include <math.h>
#include <string.h>
#pragma clang fp contract(off)
#include "step_common.h"

struct JpegC { float m[9], mi[9], wp[3]; };       // M, M^-1, w+
struct JpegQ { float v[128]; };                   // luma [64] then chroma [64], natural order: q (encoder) or h (step)

// ---------------------------------------------------------------- host: tables
// ITU-T T.81 Annex K, tables K.1 (luminance) and K.2 (chrominance), natural order
static const uint8_t kJpegBase[128] = {
    16, 11, 10, 16, 24, 40, 51, 61,      12, 12, 14, 19, 26, 58, 60, 55,      14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62,      18, 22, 37, 56, 68, 109, 103, 77,    24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101,  72, 92, 95, 98, 112, 100, 103, 99,
    17, 18, 24, 47, 99, 99, 99, 99,      18, 21, 26, 66, 99, 99, 99, 99,      24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99,      99, 99, 99, 99, 99, 99, 99, 99,      99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,      99, 99, 99, 99, 99, 99, 99, 99};

extern "C" int ddnm_jpeg_quality_tables(int32_t quality, int32_t dc_shift, float* q128_out, float* delta_out) {
    if (!q128_out || !delta_out || quality < 1 || quality > 100) return DDNM_E_BADARG;
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;          // libjpeg's jpeg_quality_scaling
    for (int i = 0; i < 128; ++i) {
        int e = ((int)kJpegBase[i] * scale + 50) / 100;
        e = e < 1 ? 1 : e > 255 ? 255 : e;
        q128_out[i] = (float)((double)e / 127.5);
    }
    *delta_out = dc_shift ? (float)(-4.0 / 127.5) : 0.f;
    return 0;
}

// ---------------------------------------------------------------- device: 8-point DCT-II and its inverse, orthonormal
#define JA1 0.49039264020161522f
#define JA2 0.46193976625564337f
#define JA3 0.41573480615127262f
#define JA4 0.35355339059327376f
#define JA5 0.27778511650980109f
#define JA6 0.19134171618254489f
#define JA7 0.09754516100806413f

__host__ __device__ __forceinline__ void jpeg_dct8(float (&x)[8]) {
    const float s0 = x[0] + x[7], s1 = x[1] + x[6], s2 = x[2] + x[5], s3 = x[3] + x[4];
    const float d0 = x[0] - x[7], d1 = x[1] - x[6], d2 = x[2] - x[5], d3 = x[3] - x[4];
    const float p = s0 + s3, q = s1 + s2, r = s0 - s3, t = s1 - s2;
    x[0] = JA4 * (p + q);
    x[4] = JA4 * (p - q);
    x[2] = fmaf(JA2, r, JA6 * t);
    x[6] = fmaf(JA6, r, -(JA2 * t));
    x[1] = fmaf(JA1, d0, fmaf(JA3, d1, fmaf(JA5, d2, JA7 * d3)));
    x[3] = fmaf(JA3, d0, fmaf(-JA7, d1, fmaf(-JA1, d2, -(JA5 * d3))));
    x[5] = fmaf(JA5, d0, fmaf(-JA1, d1, fmaf(JA7, d2, JA3 * d3)));
    x[7] = fmaf(JA7, d0, fmaf(-JA5, d1, fmaf(JA3, d2, -(JA1 * d3))));
}

__host__ __device__ __forceinline__ void jpeg_idct8(float (&x)[8]) {
    const float a = JA4 * (x[0] + x[4]), b = JA4 * (x[0] - x[4]);
    const float c = fmaf(JA2, x[2], JA6 * x[6]), d = fmaf(JA6, x[2], -(JA2 * x[6]));
    const float e0 = a + c, e1 = b + d, e2 = b - d, e3 = a - c;
    const float o0 = fmaf(JA1, x[1], fmaf(JA3, x[3], fmaf(JA5, x[5], JA7 * x[7])));
    const float o1 = fmaf(JA3, x[1], fmaf(-JA7, x[3], fmaf(-JA1, x[5], -(JA5 * x[7]))));
    const float o2 = fmaf(JA5, x[1], fmaf(-JA1, x[3], fmaf(JA7, x[5], JA3 * x[7])));
    const float o3 = fmaf(JA7, x[1], fmaf(-JA5, x[3], fmaf(JA3, x[5], -(JA1 * x[7]))));
    x[0] = e0 + o0; x[7] = e0 - o0;
    x[1] = e1 + o1; x[6] = e1 - o1;
    x[2] = e2 + o2; x[5] = e2 - o2;
    x[3] = e3 + o3; x[4] = e3 - o3;
}

// ---------------------------------------------------------------- device: geometry
template <int RW, int RH>
struct JpegGeo {
    static constexpr int N = RW * RH;             // pixels of a chroma site = luma blocks of an MCU
    static constexpr int NB = N + 2;              // blocks of an MCU
    static constexpr int C4 = 2 * RW;             // 16-byte column groups of an MCU row
    static constexpr int G = 256 / (8 * C4);      // MCUs of a workgroup
    static constexpr int NBLK = G * NB;
    static constexpr int BS = 72;                 // floats from one LDS block to the next
    static constexpr int NS = 4 / RW;             // chroma sites of a strip
    static constexpr int LDS = NBLK * BS;
};

// MCU m of the batch: image, and the offsets of its first pixel in a luma plane and of its first site in a chroma plane
template <int RW, int RH>
__device__ __forceinline__ void jpeg_mcu(int64_t m, int H, int W, int64_t& b, int64_t& pix, int64_t& cpix) {
    const int MW = W / (8 * RW);
    const int64_t per_img = (int64_t)(H / (8 * RH)) * MW;
    b = m / per_img;
    const int64_t q = m - b * per_img;
    const int mi = (int)(q / MW), mj = (int)(q - (int64_t)mi * MW);
    pix = (int64_t)mi * 8 * RH * W + mj * 8 * RW;
    cpix = (int64_t)mi * 8 * (W / RW) + mj * 8;
}

// the strip of thread `tid` in workgroup `group`
template <int RW, int RH>
struct JpegStrip {
    using Z = JpegGeo<RW, RH>;
    bool on;                 // its MCU exists (the last workgroup may hold fewer than G)
    int mcu, r, c4;          // MCU within the workgroup, site row 0..7, column group
    int64_t b, pix, cpix;    // image; offset of the strip's first row in a luma plane, of its first site in a chroma plane
    __device__ __forceinline__ JpegStrip(int tid, int64_t group, int H, int W, int64_t total) {
        c4 = tid % Z::C4;
        mcu = (tid / Z::C4) % Z::G;
        r = tid / (Z::C4 * Z::G);
        const int64_t m = group * Z::G + mcu;
        on = m < total;
        b = 0; pix = 0; cpix = 0;
        if (on) {
            jpeg_mcu<RW, RH>(m, H, W, b, pix, cpix);
            pix += (int64_t)r * RH * W + c4 * 4;
            cpix += (int64_t)r * (W / RW) + c4 * Z::NS;
        }
    }
    // LDS offsets: the four luma values of strip row rr, the strip's first site in the Cb block (Cr: + BS)
    __device__ __forceinline__ int luma(int rr) const {
        const int row = r * RH + rr, col = c4 * 4;
        return (mcu * Z::NB + (row >> 3) * RW + (col >> 3)) * Z::BS + (row & 7) * 8 + (col & 7);
    }
    __device__ __forceinline__ int chroma() const { return (mcu * Z::NB + Z::N) * Z::BS + r * 8 + c4 * Z::NS; }
};

__device__ __forceinline__ f32x4 jdot3(const float* w, f32x4 r, f32x4 g, f32x4 b) { return (r * w[0] + g * w[1]) + b * w[2]; }
__device__ __forceinline__ float jdot3(const float* w, float r, float g, float b) { return (r * w[0] + g * w[1]) + b * w[2]; }

// colour planes of a strip's pixels v[c][rr] into the blocks of L: luma per pixel, chroma as site means
template <int RW, int RH>
__device__ __forceinline__ void jpeg_planes_to_lds(const JpegStrip<RW, RH>& t, const f32x4 (&v)[3][RH], const JpegC& cc, float* L) {
    using Z = JpegGeo<RW, RH>;
    float sb[Z::NS] = {}, sr[Z::NS] = {};
#pragma unroll
    for (int rr = 0; rr < RH; ++rr) {
        st4(L + t.luma(rr), jdot3(cc.m, v[0][rr], v[1][rr], v[2][rr]));
        const f32x4 cb = jdot3(cc.m + 3, v[0][rr], v[1][rr], v[2][rr]), cr = jdot3(cc.m + 6, v[0][rr], v[1][rr], v[2][rr]);
#pragma unroll
        for (int j = 0; j < 4; ++j) { sb[j / RW] += cb[j]; sr[j / RW] += cr[j]; }
    }
    const int co = t.chroma();
#pragma unroll
    for (int k = 0; k < Z::NS; ++k) { L[co + k] = sb[k] / (float)Z::N; L[co + Z::BS + k] = sr[k] / (float)Z::N; }
}

// A_chroma^+ of the planes in L at a strip's pixels: out[c][rr] = w+ (Y_p - Ybar) + M^-1 (Ybar, Cb, Cr)
template <int RW, int RH>
__device__ __forceinline__ void jpeg_lds_to_pixels(const JpegStrip<RW, RH>& t, const float* L, const JpegC& cc, f32x4 (&out)[3][RH]) {
    using Z = JpegGeo<RW, RH>;
    f32x4 yv[RH];
    float sy[Z::NS] = {};
#pragma unroll
    for (int rr = 0; rr < RH; ++rr) {
        yv[rr] = ld4(L + t.luma(rr));
#pragma unroll
        for (int j = 0; j < 4; ++j) sy[j / RW] += yv[rr][j];
    }
    const int co = t.chroma();
    f32x4 ymv, dcv[3];
#pragma unroll
    for (int k = 0; k < Z::NS; ++k) {
        const float ym = sy[k] / (float)Z::N, cb = L[co + k], cr = L[co + Z::BS + k];
#pragma unroll
        for (int j = k * RW; j < (k + 1) * RW; ++j) {
            ymv[j] = ym;
#pragma unroll
            for (int c = 0; c < 3; ++c) dcv[c][j] = jdot3(cc.mi + 3 * c, ym, cb, cr);
        }
    }
#pragma unroll
    for (int rr = 0; rr < RH; ++rr) {
        const f32x4 d = yv[rr] - ymv;
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c][rr] = d * cc.wp[c] + dcv[c];
    }
}

// the Cb and Cr blocks of the workgroup's MCUs between L and the rows `g` [B][hw + 2 hwn], 16 bytes per access, lanes
// along the rows of the chroma planes
template <int RW, int RH, bool LOAD>
__device__ __forceinline__ void jpeg_chroma_io(float* L, float* g, int64_t group, int H, int W, int64_t total) {
    using Z = JpegGeo<RW, RH>;
    const int64_t hw = (int64_t)H * W, hwn = hw / Z::N;
    for (int j = threadIdx.x; j < Z::G * 32; j += 256) {
        const int c4 = j & 1, mcu = (j >> 1) % Z::G, row = (j / (2 * Z::G)) & 7, plane = j / (16 * Z::G);
        const int64_t m = group * Z::G + mcu;
        if (m >= total) continue;
        int64_t b, pix, cpix;
        jpeg_mcu<RW, RH>(m, H, W, b, pix, cpix);
        float* gp = g + b * (hw + 2 * hwn) + hw + plane * hwn + cpix + (int64_t)row * (W / RW) + c4 * 4;
        float* lp = L + (mcu * Z::NB + Z::N + plane) * Z::BS + row * 8 + c4 * 4;
        if (LOAD) st4(lp, ld4(gp));
        else st4(gp, ld4(lp));
    }
}

// one row of one block per task, transformed in place
template <int BS, bool INV>
__device__ __forceinline__ void jpeg_rows(float* L, int ntasks) {
    for (int t = threadIdx.x; t < ntasks; t += 256) {
        float* p = L + (t >> 3) * BS + (t & 7) * 8;
        const f32x4 a = ld4(p), b = ld4(p + 4);
        float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
        if (INV) jpeg_idct8(v);
        else jpeg_dct8(v);
        st4(p, f32x4{v[0], v[1], v[2], v[3]});
        st4(p + 4, f32x4{v[4], v[5], v[6], v[7]});
    }
}

enum { JPEG_T = 0, JPEG_A = 1, JPEG_PINV = 2, JPEG_STEP = 3 };

// one column of one block per task: forward DCT over the rows (T, A, step), the mode's work on coefficients (0..7, v),
// inverse DCT over u (T^+, step); QL holds q (A) or h (step), YL the measured y in the same blocks (step)
template <int RW, int RH, int MODE>
__device__ __forceinline__ void jpeg_cols(float* L, const float* YL, const float* QL, float delta, int ntasks) {
    using Z = JpegGeo<RW, RH>;
    for (int t = threadIdx.x; t < ntasks; t += 256) {
        const int blk = t >> 3, v = t & 7;
        float* p = L + blk * Z::BS + v;
        float f[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) f[u] = p[u * 8];
        if (MODE != JPEG_PINV) jpeg_dct8(f);
        if (MODE == JPEG_A || MODE == JPEG_STEP) {
            const bool chroma = blk % Z::NB >= Z::N;
            const float* qp = QL + (chroma ? 64 : 0) + v;
            if (MODE == JPEG_A) {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const float q = qp[u * 8], dl = (u == 0 && v == 0 && !chroma) ? delta : 0.f;
                    f[u] = q * rintf((f[u] - dl) / q) + dl;
                }
            } else {
                const float* yp = YL + blk * Z::BS + v;
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const float y = yp[u * 8], h = qp[u * 8];
                    f[u] = f[u] - fminf(fmaxf(f[u], y - h), y + h);
                }
            }
        }
        if (MODE == JPEG_PINV || MODE == JPEG_STEP) jpeg_idct8(f);
#pragma unroll
        for (int u = 0; u < 8; ++u) p[u * 8] = f[u];
    }
}

// ---------------------------------------------------------------- kernels
// MODE JPEG_T: out = T in;  JPEG_A: out = q rint((T in - delta) / q) + delta;  JPEG_PINV: out = T^+ in
template <int RW, int RH, int MODE>
__global__ __launch_bounds__(256) void jpeg_op_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W,
                                                      int64_t total, JpegC cc, JpegQ q, float delta) {
    using Z = JpegGeo<RW, RH>;
    __shared__ __attribute__((aligned(16))) float CL[Z::LDS];
    __shared__ float QL[128];
    const int64_t group = blockIdx.x, hw = (int64_t)H * W, row_len = hw + 2 * (hw / Z::N);
    const JpegStrip<RW, RH> t(threadIdx.x, group, H, W, total);
    const int64_t left = total - group * Z::G;
    const int ntasks = (int)(left < Z::G ? left : Z::G) * Z::NB * 8;
    if (MODE == JPEG_A && threadIdx.x < 128) QL[threadIdx.x] = q.v[threadIdx.x];
    if (MODE != JPEG_PINV) {
        if (t.on) {
            f32x4 v[3][RH];
#pragma unroll
            for (int rr = 0; rr < RH; ++rr)
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c][rr] = ld4(in + t.b * 3 * hw + c * hw + t.pix + (int64_t)rr * W);
            jpeg_planes_to_lds<RW, RH>(t, v, cc, CL);
        }
        __syncthreads();
        jpeg_rows<Z::BS, false>(CL, ntasks);
        __syncthreads();
        jpeg_cols<RW, RH, MODE>(CL, nullptr, QL, delta, ntasks);
        __syncthreads();
        if (t.on) {
#pragma unroll
            for (int rr = 0; rr < RH; ++rr) st4(out + t.b * row_len + t.pix + (int64_t)rr * W, ld4(CL + t.luma(rr)));
        }
        jpeg_chroma_io<RW, RH, false>(CL, out, group, H, W, total);
    } else {
        if (t.on) {
#pragma unroll
            for (int rr = 0; rr < RH; ++rr) st4(CL + t.luma(rr), ld4(in + t.b * row_len + t.pix + (int64_t)rr * W));
        }
        jpeg_chroma_io<RW, RH, true>(CL, const_cast<float*>(in), group, H, W, total);
        __syncthreads();
        jpeg_cols<RW, RH, JPEG_PINV>(CL, nullptr, QL, 0.f, ntasks);
        __syncthreads();
        jpeg_rows<Z::BS, true>(CL, ntasks);
        __syncthreads();
        if (t.on) {
            f32x4 v[3][RH];
            jpeg_lds_to_pixels<RW, RH>(t, CL, cc, v);
#pragma unroll
            for (int rr = 0; rr < RH; ++rr)
#pragma unroll
                for (int c = 0; c < 3; ++c) st4(out + t.b * 3 * hw + c * hw + t.pix + (int64_t)rr * W, v[c][rr]);
        }
    }
}

template <int RW, int RH, class NZ>
__global__ __launch_bounds__(256) void step_jpeg_kernel(const float* __restrict__ xt, const float* __restrict__ et,
                                                        int64_t et_bstride, NZ noise, const float* __restrict__ y,
                                                        float* __restrict__ x0o, float* __restrict__ xn, int H, int W,
                                                        int64_t total, ddnm_step_scalars s, JpegC cc, JpegQ h) {
    using Z = JpegGeo<RW, RH>;
    __shared__ __attribute__((aligned(16))) float CL[Z::LDS];
    __shared__ __attribute__((aligned(16))) float YL[Z::LDS];
    __shared__ float HL[128];
    const int64_t group = blockIdx.x, hw = (int64_t)H * W, row_len = hw + 2 * (hw / Z::N);
    const JpegStrip<RW, RH> t(threadIdx.x, group, H, W, total);
    const int64_t left = total - group * Z::G;
    const int ntasks = (int)(left < Z::G ? left : Z::G) * Z::NB * 8;
    const auto nz = bind(noise, t.b);                               // (a strip without an MCU binds image 0 and draws nothing)
    const int64_t base = t.b * 3 * hw + t.pix, ebase = t.b * et_bstride + t.pix;
    if (threadIdx.x < 128) HL[threadIdx.x] = h.v[threadIdx.x];
    f32x4 x0[3][RH], e[3][RH];
    if (t.on) {
#pragma unroll
        for (int rr = 0; rr < RH; ++rr) {
            const int64_t o = (int64_t)rr * W;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                e[c][rr] = ld4(et + ebase + c * hw + o);
                x0[c][rr] = x0_of(ld4(xt + base + c * hw + o), e[c][rr], s);
                if (x0o) st4(x0o + base + c * hw + o, x0[c][rr]);
            }
            st4(YL + t.luma(rr), ld4(y + t.b * row_len + t.pix + o));
        }
        jpeg_planes_to_lds<RW, RH>(t, x0, cc, CL);
    }
    jpeg_chroma_io<RW, RH, true>(YL, const_cast<float*>(y), group, H, W, total);
    __syncthreads();
    jpeg_rows<Z::BS, false>(CL, ntasks);
    __syncthreads();
    jpeg_cols<RW, RH, JPEG_STEP>(CL, YL, HL, 0.f, ntasks);
    __syncthreads();
    jpeg_rows<Z::BS, true>(CL, ntasks);
    __syncthreads();
    if (t.on) {
        f32x4 corr[3][RH];
        jpeg_lds_to_pixels<RW, RH>(t, CL, cc, corr);
#pragma unroll
        for (int rr = 0; rr < RH; ++rr) {
            const int64_t o = (int64_t)rr * W;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                st4(xn + base + c * hw + o, update_of(x0[c][rr] - corr[c][rr] * s.lambda, nz4(nz, base + c * hw + o), e[c][rr], s));
        }
    }
}

// ---------------------------------------------------------------- host: launchers
static inline bool jpeg_site_ok(int32_t rw, int32_t rh) { return (rw == 1 && rh == 1) || (rw == 2 && rh == 1) || (rw == 2 && rh == 2); }

// M^-1 and w+ from ddnm_chroma_constants (they do not depend on the site: any site it knows serves); a null or singular M
// is DDNM_E_BADARG
static int jpeg_colour(const float* m9, JpegC* out) {
    double k[37];
    if (!m9) return DDNM_E_BADARG;
    if (int e = ddnm_chroma_constants(m9, 2, 2, k)) return e;
    for (int i = 0; i < 9; ++i) { out->m[i] = m9[i]; out->mi[i] = (float)k[i]; }
    for (int i = 0; i < 3; ++i) out->wp[i] = (float)k[9 + i];
    return 0;
}

static int jpeg_shape(int32_t H, int32_t W, int32_t rw, int32_t rh, int64_t et_bstride) {
    if (!jpeg_site_ok(rw, rh)) return DDNM_E_SHAPE;
    if (H <= 0 || W <= 0 || H % (8 * rh) || W % (8 * rw) || (et_bstride & 3)) return DDNM_E_SHAPE;
    return 0;
}

static inline bool jpeg_steps_ok(const float* q128) {
    if (!q128) return false;
    for (int i = 0; i < 128; ++i)
        if (!isfinite(q128[i]) || !(q128[i] > 0.f)) return false;
    return true;
}

// MCUs of the batch and the workgroups that own them (DDNM_E_SHAPE beyond 2^31 - 1 workgroups)
static int jpeg_grid(int32_t B, int32_t H, int32_t W, int32_t rw, int32_t rh, int64_t* total, unsigned* groups) {
    const int G = 16 / rw;
    *total = (int64_t)B * (H / (8 * rh)) * (W / (8 * rw));
    const int64_t n = (*total + G - 1) / G;
    if (n > 0x7fffffff) return DDNM_E_SHAPE;
    *groups = (unsigned)n;
    return 0;
}

#define JPEG_FOR_SITE(rw, rh, LAUNCH)          \
    if (rw == 1) { LAUNCH(1, 1); }             \
    else if (rh == 1) { LAUNCH(2, 1); }        \
    else { LAUNCH(2, 2); }

template <int MODE>
static int launch_jpeg_op(const float* in, float* out, int32_t B, int32_t H, int32_t W, int32_t rw, int32_t rh,
                          const float* m9_host, const float* q128_host, float delta, void* stream) {
    if (!in || !out || B <= 0) return DDNM_E_BADARG;
    if (MODE == JPEG_A && (!jpeg_steps_ok(q128_host) || !isfinite(delta))) return DDNM_E_BADARG;
    JpegC cc;
    if (int e = jpeg_colour(m9_host, &cc)) return e;
    if (int e = jpeg_shape(H, W, rw, rh, 0)) return e;
    JpegQ q;
    for (int i = 0; i < 128; ++i) q.v[i] = MODE == JPEG_A ? q128_host[i] : 1.f;
    int64_t total;
    unsigned groups;
    if (int e = jpeg_grid(B, H, W, rw, rh, &total, &groups)) return e;
#define LAUNCH(RW, RH) \
    DDNM_LAUNCH((jpeg_op_kernel<RW, RH, MODE>), dim3(groups), dim3(256), 0, (hipStream_t)stream, in, out, H, W, total, cc, q, delta)
    JPEG_FOR_SITE(rw, rh, LAUNCH)
#undef LAUNCH
    return 0;
}

extern "C" int ddnm_op_jpeg_T_f32(const float* x, float* c, int32_t B, int32_t H, int32_t W, int32_t rw, int32_t rh,
                                  const float* m9_host, void* stream) {
    return launch_jpeg_op<JPEG_T>(x, c, B, H, W, rw, rh, m9_host, nullptr, 0.f, stream);
}

extern "C" int ddnm_op_jpeg_A_f32(const float* x, float* y, int32_t B, int32_t H, int32_t W, int32_t rw, int32_t rh,
                                  const float* m9_host, const float* q128_host, float delta, void* stream) {
    return launch_jpeg_op<JPEG_A>(x, y, B, H, W, rw, rh, m9_host, q128_host, delta, stream);
}

extern "C" int ddnm_op_jpeg_pinv_f32(const float* y, float* x, int32_t B, int32_t H, int32_t W, int32_t rw, int32_t rh,
                                     const float* m9_host, void* stream) {
    return launch_jpeg_op<JPEG_PINV>(y, x, B, H, W, rw, rh, m9_host, nullptr, 0.f, stream);
}

static inline bool jpeg_step_ptrs(const float* xt, const float* et, const float* y, const float* x0, const float* xt_next,
                                  const float* q128_host, float box, const ddnm_step_scalars* s, int32_t B) {
    if (!xt || !et || !y || !xt_next || !s || B <= 0) return false;
    if (!jpeg_steps_ok(q128_host) || !(box >= 0.f && box <= 1.f)) return false;
    return xt_next != xt && xt_next != et && xt_next != x0 && (!x0 || (x0 != xt && x0 != et));
}

template <class Src>
static int launch_step_jpeg(const float* xt, const float* et, int64_t et_bstride, Src src, const float* y, float* x0,
                            float* xt_next, int32_t B, int32_t H, int32_t W, int32_t rw, int32_t rh, const float* m9_host,
                            const float* q128_host, float box, const ddnm_step_scalars* s, void* stream) {
    JpegC cc;
    if (int e = jpeg_colour(m9_host, &cc)) return e;
    if (int e = jpeg_shape(H, W, rw, rh, et_bstride)) return e;
    JpegQ h;
    for (int i = 0; i < 128; ++i) h.v[i] = (float)((double)box * (double)q128_host[i] * 0.5);
    int64_t total;
    unsigned groups;
    if (int e = jpeg_grid(B, H, W, rw, rh, &total, &groups)) return e;
#define LAUNCH(RW, RH)                                                                                                     \
    DDNM_LAUNCH((step_jpeg_kernel<RW, RH, Src>), dim3(groups), dim3(256), 0, (hipStream_t)stream, xt, et, et_bstride, src, \
                y, x0, xt_next, H, W, total, *s, cc, h)
    JPEG_FOR_SITE(rw, rh, LAUNCH)
#undef LAUNCH
    return 0;
}

extern "C" int ddnm_step_jpeg_f32(const float* xt, const float* et, int64_t et_bstride, const float* noise, const float* y,
                                  float* x0, float* xt_next, int32_t B, int32_t H, int32_t W, int32_t rw, int32_t rh,
                                  const float* m9_host, const float* q128_host, float box, const ddnm_step_scalars* s,
                                  void* stream) {
    if (!jpeg_step_ptrs(xt, et, y, x0, xt_next, q128_host, box, s, B) || !noise_ok(noise, s)) return DDNM_E_BADARG;
    return launch_step_jpeg(xt, et, et_bstride, noise_src(noise, s, (int64_t)3 * H * W), y, x0, xt_next, B, H, W, rw, rh,
                            m9_host, q128_host, box, s, stream);
}

extern "C" int ddnm_step_jpeg_keyed_f32(const float* xt, const float* et, int64_t et_bstride, const uint32_t* keys,
                                        const float* y, float* x0, float* xt_next, int32_t B, int32_t H, int32_t W,
                                        int32_t rw, int32_t rh, const float* m9_host, const float* q128_host, float box,
                                        const ddnm_step_scalars* s, void* stream) {
    if (!jpeg_step_ptrs(xt, et, y, x0, xt_next, q128_host, box, s, B) || !keys_ok(keys)) return DDNM_E_BADARG;
    return launch_step_jpeg(xt, et, et_bstride, keyed_src(keys, s, (int64_t)3 * H * W), y, x0, xt_next, B, H, W, rw, rh,
                            m9_host, q128_host, box, s, stream);
}
#undef JPEG_FOR_SITE
