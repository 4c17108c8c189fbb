// DDNM sampler-step kernels: x0 prediction, null-space projection, DDIM update -- gfx950.
// All HBM-bound; every kernel makes exactly one pass over its operands with 16-byte
// loads/stores.  Algorithmic traffic per image-step: read xt, et, noise (+y), write xt'
// (+x0) = 3.15-3.93 MB at 256x256.
//
// Restates functions/svd_ddnm.py:57-65,74 and guided_diffusion/diffusion.py:365-384 with the
// operator algebra of functions/svd_operators.py collapsed to its direct form:
//   sr_averagepooling : A = r x r mean,  A^+ = replicate           (svd_operators.py:479-533)
//   colorization      : A = w . rgb,     A^+ = w/|w|^2             (svd_operators.py:627-667)
//   inpainting        : A = gather kept, A^+ = scatter             (svd_operators.py:324-359)
//   demosaicing       : A = one channel per pixel (CFA), A^+ = scatter   (the same class over single entries)
//   denoising         : identity                                    (svd_operators.py:442-462)
//   old photo (mcsr)  : A = pool . grey . mask, A^+ exact, one singular value per r x r site   (diffusion.py:260-290 has A)
//   chroma subsampling: A = full luma + chroma averaged per rw x rh site, A^+ exact, four singular values per launch
// Rounding follows the reference's evaluation order; contraction into FMA is disabled so
// that mul/add round separately like the ATen elementwise kernels.
#include "common.h"
#include "philox.h"
#include <math.h>
#include <string.h>
#pragma clang fp contract(off)
#include "step_common.h"      // 16-byte moves, noise sources, x0_of / update_of (shared with jpeg.hip)

// ---------------------------------------------------------------- generic two-part step
__global__ __launch_bounds__(256) void step_x0_kernel(const float* __restrict__ xt, const float* __restrict__ et,
                                                      int64_t et_bstride, float* __restrict__ x0, int64_t chw4,
                                                      int64_t total4, ddnm_step_scalars s) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / chw4, r = i - b * chw4;
        st4(x0 + i * 4, x0_of(ld4(xt + i * 4), ld4(et + b * et_bstride + r * 4), s));
    }
}

extern "C" int ddnm_step_x0_f32(const float* xt, const float* et, int64_t et_bstride, float* x0, int32_t B,
                                int64_t chw, const ddnm_step_scalars* s, void* stream) {
    if (!xt || !et || !x0 || !s || B <= 0 || chw <= 0) return DDNM_E_BADARG;
    if ((chw & 3) || (et_bstride & 3)) return DDNM_E_SHAPE;
    const int64_t total4 = (int64_t)B * chw / 4;
    DDNM_LAUNCH(step_x0_kernel, GRID_1D(total4), dim3(256), 0, (hipStream_t)stream, xt, et, et_bstride, x0,
                       chw / 4, total4, *s);
    return 0;
}

template <class NZ>
__global__ __launch_bounds__(256) void step_combine_kernel(const float* __restrict__ x0, const float* __restrict__ proj,
                                                           const float* __restrict__ apy,
                                                           NZ noise,
                                                           const float* __restrict__ et, int64_t et_bstride,
                                                           float* __restrict__ xt_next, int64_t chw4, int64_t total4,
                                                           ddnm_step_scalars s) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / chw4, r = i - b * chw4;
        const auto nz = bind(noise, b);
        f32x4 p = ld4(proj + i * 4);
        if (apy) p = p - ld4(apy + i * 4);
        const f32x4 x0h = ld4(x0 + i * 4) - p * s.lambda;
        st4(xt_next + i * 4, update_of(x0h, nz4(nz, i * 4), ld4(et + b * et_bstride + r * 4), s));
    }
}

// Host side of a step kernel that exists for both noise sources: the extern "C" pair (here and under "keyed entry points")
// checks its pointers and its source, builds the source and calls the one launcher below its kernel, which checks the
// sizes (DDNM_E_BADARG before DDNM_E_SHAPE, as everywhere), sizes the grid and launches kernel<Src>.
template <class Src>
static int launch_step_combine(const float* x0, const float* proj, const float* apy, Src src, const float* et, int64_t et_bstride,
                               float* xt_next, int32_t B, int64_t chw, const ddnm_step_scalars* s, void* stream) {
    if (B <= 0 || chw <= 0) return DDNM_E_BADARG;
    if ((chw & 3) || (et_bstride & 3)) return DDNM_E_SHAPE;
    const int64_t total4 = (int64_t)B * chw / 4;
    DDNM_LAUNCH(step_combine_kernel<Src>, GRID_1D(total4), dim3(256), 0, (hipStream_t)stream, x0, proj, apy, src, et, et_bstride,
                xt_next, chw / 4, total4, *s);
    return 0;
}

extern "C" int ddnm_step_combine_f32(const float* x0, const float* proj, const float* apy, const float* noise,
                                     const float* et, int64_t et_bstride, float* xt_next, int32_t B, int64_t chw,
                                     const ddnm_step_scalars* s, void* stream) {
    if (!x0 || !proj || !et || !xt_next || !s || !noise_ok(noise, s)) return DDNM_E_BADARG;
    return launch_step_combine(x0, proj, apy, noise_src(noise, s, chw), et, et_bstride, xt_next, B, chw, s, stream);
}

// ---------------------------------------------------------------- fused: SR by average pooling, r = 4
// one thread per 4x4 patch: 4 rows x float4.
template <class NZ>
__global__ __launch_bounds__(256) void step_sr4_kernel(const float* __restrict__ xt, const float* __restrict__ et,
                                                       int64_t et_bstride, NZ noise,
                                                       const float* __restrict__ y, float* __restrict__ x0o,
                                                       float* __restrict__ xn, int H, int W, int64_t total,
                                                       ddnm_step_scalars s) {
    const int Wy = W >> 2, Hy = H >> 2;
    const int64_t per_img = (int64_t)3 * Hy * Wy;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / per_img;
        const auto nz = bind(noise, b);
        int64_t r = i - b * per_img;
        const int c = (int)(r / ((int64_t)Hy * Wy));
        r -= (int64_t)c * Hy * Wy;
        const int py = (int)(r / Wy), px = (int)(r - (int64_t)py * Wy);
        const int64_t off = ((b * 3 + c) * H + py * 4) * (int64_t)W + px * 4;
        const int64_t eoff = b * et_bstride + ((int64_t)c * H + py * 4) * W + px * 4;
        f32x4 x0[4], e[4];
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            e[j] = ld4(et + eoff + (int64_t)j * W);
            x0[j] = x0_of(ld4(xt + off + (int64_t)j * W), e[j], s);
            sum += x0[j].x; sum += x0[j].y; sum += x0[j].z; sum += x0[j].w;   // row-major window order
        }
        const float resid = sum / 16.0f - y[i];
        const float corr = resid * s.lambda;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (x0o) st4(x0o + off + (int64_t)j * W, x0[j]);
            const f32x4 x0h = x0[j] - corr;
            st4(xn + off + (int64_t)j * W, update_of(x0h, nz4(nz, off + (int64_t)j * W), e[j], s));
        }
    }
}

template <class Src>
static int launch_step_sr4(const float* xt, const float* et, int64_t et_bstride, Src src, const float* y, float* x0, float* xt_next,
                           int32_t B, int32_t H, int32_t W, int32_t r, const ddnm_step_scalars* s, void* stream) {
    if (B <= 0) return DDNM_E_BADARG;
    if (r != 4 || (H & 3) || (W & 3) || (et_bstride & 3)) return DDNM_E_SHAPE;
    const int64_t total = (int64_t)B * 3 * (H / 4) * (W / 4);
    DDNM_LAUNCH(step_sr4_kernel<Src>, GRID_1D(total), dim3(256), 0, (hipStream_t)stream, xt, et, et_bstride, src, y, x0, xt_next, H,
                W, total, *s);
    return 0;
}

extern "C" int ddnm_step_sr_avgpool_f32(const float* xt, const float* et, int64_t et_bstride, const float* noise,
                                        const float* y, float* x0, float* xt_next, int32_t B, int32_t H, int32_t W,
                                        int32_t r, const ddnm_step_scalars* s, void* stream) {
    if (!xt || !et || !y || !xt_next || !s || !noise_ok(noise, s)) return DDNM_E_BADARG;
    return launch_step_sr4(xt, et, et_bstride, noise_src(noise, s, (int64_t)3 * H * W), y, x0, xt_next, B, H, W, r, s, stream);
}

// ---------------------------------------------------------------- fused: colorization
struct ColorW { float w[3]; float wp[3]; };

// w = per-pixel measurement row (default (0.3333, 0.3334, 0.3333), svd_operators.py:632); wp = w/|w|^2
static ColorW color_weights(const float* w3_host) {
    ColorW c;
    const float dflt[3] = {0.3333f, 0.3334f, 0.3333f};
    for (int i = 0; i < 3; ++i) c.w[i] = w3_host ? w3_host[i] : dflt[i];
    const float n2 = (c.w[0] * c.w[0] + c.w[1] * c.w[1]) + c.w[2] * c.w[2];
    for (int i = 0; i < 3; ++i) c.wp[i] = c.w[i] / n2;
    return c;
}

template <class NZ>
__global__ __launch_bounds__(256) void step_color_kernel(const float* __restrict__ xt, const float* __restrict__ et,
                                                         int64_t et_bstride, NZ noise,
                                                         const float* __restrict__ y, float* __restrict__ x0o,
                                                         float* __restrict__ xn, int64_t hw4, int64_t total4,
                                                         ddnm_step_scalars s, ColorW cw) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / hw4, p = i - b * hw4;
        const auto nz = bind(noise, b);
        const int64_t base = (b * 3 * hw4 + p) * 4, ebase = b * et_bstride + p * 4;
        f32x4 e[3], x0[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            e[c] = ld4(et + ebase + c * hw4 * 4);
            x0[c] = x0_of(ld4(xt + base + c * hw4 * 4), e[c], s);
        }
        const f32x4 gray = (x0[0] * cw.w[0] + x0[1] * cw.w[1]) + x0[2] * cw.w[2];
        const f32x4 resid = (gray - ld4(y + i * 4)) * s.lambda;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (x0o) st4(x0o + base + c * hw4 * 4, x0[c]);
            const f32x4 x0h = x0[c] - resid * cw.wp[c];
            st4(xn + base + c * hw4 * 4, update_of(x0h, nz4(nz, base + c * hw4 * 4), e[c], s));
        }
    }
}

template <class Src>
static int launch_step_color(const float* xt, const float* et, int64_t et_bstride, Src src, const float* y, float* x0, float* xt_next,
                             int32_t B, int32_t HW, const float* w3_host, const ddnm_step_scalars* s, void* stream) {
    if (B <= 0 || HW <= 0) return DDNM_E_BADARG;
    if ((HW & 3) || (et_bstride & 3)) return DDNM_E_SHAPE;
    const int64_t total4 = (int64_t)B * HW / 4;
    DDNM_LAUNCH(step_color_kernel<Src>, GRID_1D(total4), dim3(256), 0, (hipStream_t)stream, xt, et, et_bstride, src, y, x0, xt_next,
                (int64_t)HW / 4, total4, *s, color_weights(w3_host));
    return 0;
}

extern "C" int ddnm_step_color_f32(const float* xt, const float* et, int64_t et_bstride, const float* noise,
                                   const float* y, float* x0, float* xt_next, int32_t B, int32_t HW,
                                   const float* w3_host, const ddnm_step_scalars* s, void* stream) {
    if (!xt || !et || !y || !xt_next || !s || !noise_ok(noise, s)) return DDNM_E_BADARG;
    return launch_step_color(xt, et, et_bstride, noise_src(noise, s, (int64_t)3 * HW), y, x0, xt_next, B, HW, w3_host, s, stream);
}

// ---------------------------------------------------------------- fused: inpainting (mask as rank table)
// image b reads the rank table at rank + b * rank_bstride and its measurement row at y + b * y_bstride: (0, 3 * n_kept)
// is one mask shared by the batch, (HW, y_stride) one mask per image (the *_pi_* entry points; rows padded to y_stride)
template <class NZ>
__global__ __launch_bounds__(256) void step_inpaint_kernel(const float* __restrict__ xt, const float* __restrict__ et,
                                                           int64_t et_bstride, NZ noise,
                                                           const float* __restrict__ y, int64_t y_bstride,
                                                           const int* __restrict__ rank, int64_t rank_bstride,
                                                           float* __restrict__ x0o,
                                                           float* __restrict__ xn, int64_t hw4, int64_t total4,
                                                           ddnm_step_scalars s) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / hw4, p = i - b * hw4;
        const auto nz = bind(noise, b);
        const int64_t base = (b * 3 * hw4 + p) * 4, ebase = b * et_bstride + p * 4;
        const int4 rk = *reinterpret_cast<const int4*>(rank + b * rank_bstride + p * 4);
        const int rks[4] = {rk.x, rk.y, rk.z, rk.w};
        const float* yb = y + b * y_bstride;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const f32x4 e = ld4(et + ebase + c * hw4 * 4);
            const f32x4 x0 = x0_of(ld4(xt + base + c * hw4 * 4), e, s);
            if (x0o) st4(x0o + base + c * hw4 * 4, x0);
            f32x4 x0h = x0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (rks[j] >= 0) x0h[j] = x0[j] - (x0[j] - yb[(int64_t)rks[j] * 3 + c]) * s.lambda;
            st4(xn + base + c * hw4 * 4, update_of(x0h, nz4(nz, base + c * hw4 * 4), e, s));
        }
    }
}

// one launcher for the shared-mask and the per-image (*_pi_*) entry points; the latter check y_stride / n_kept_max first
template <class Src>
static int launch_step_inpaint(const float* xt, const float* et, int64_t et_bstride, Src src, const float* y, int64_t y_bstride,
                               const int32_t* rank, int64_t rank_bstride, float* x0, float* xt_next, int32_t B, int32_t HW,
                               const ddnm_step_scalars* s, void* stream) {
    const int64_t total4 = (int64_t)B * HW / 4;
    DDNM_LAUNCH(step_inpaint_kernel<Src>, GRID_1D(total4), dim3(256), 0, (hipStream_t)stream, xt, et, et_bstride, src, y, y_bstride,
                rank, rank_bstride, x0, xt_next, (int64_t)HW / 4, total4, *s);
    return 0;
}

extern "C" int ddnm_step_inpaint_f32(const float* xt, const float* et, int64_t et_bstride, const float* noise,
                                     const float* y, const int32_t* rank, int32_t n_kept, float* x0, float* xt_next,
                                     int32_t B, int32_t HW, const ddnm_step_scalars* s, void* stream) {
    if (!xt || !et || !y || !rank || !xt_next || !s || B <= 0 || HW <= 0 || !noise_ok(noise, s)) return DDNM_E_BADARG;
    if ((HW & 3) || (et_bstride & 3)) return DDNM_E_SHAPE;
    return launch_step_inpaint(xt, et, et_bstride, noise_src(noise, s, (int64_t)3 * HW), y, (int64_t)3 * n_kept, rank, (int64_t)0, x0,
                               xt_next, B, HW, s, stream);
}

// one mask per image: rank [B][HW], y [B][y_stride] (row b: 3 * n_kept[b] entries, then padding that is never read)
static inline int inpaint_pi_args(int32_t n_kept_max, int64_t y_stride, int32_t HW) {
    if ((HW & 3) || (y_stride & 3) || n_kept_max < 1 || y_stride < (int64_t)3 * n_kept_max) return DDNM_E_SHAPE;
    return 0;
}

extern "C" int ddnm_step_inpaint_pi_f32(const float* xt, const float* et, int64_t et_bstride, const float* noise,
                                        const float* y, int64_t y_stride, const int32_t* rank, int32_t n_kept_max,
                                        float* x0, float* xt_next, int32_t B, int32_t HW, const ddnm_step_scalars* s,
                                        void* stream) {
    if (!xt || !et || !y || !rank || !xt_next || !s || B <= 0 || HW <= 0 || !noise_ok(noise, s)) return DDNM_E_BADARG;
    if (et_bstride & 3) return DDNM_E_SHAPE;
    if (int e = inpaint_pi_args(n_kept_max, y_stride, HW)) return e;
    return launch_step_inpaint(xt, et, et_bstride, noise_src(noise, s, (int64_t)3 * HW), y, y_stride, rank, (int64_t)HW, x0, xt_next,
                               B, HW, s, stream);
}

extern "C" int ddnm_step_inpaint_pi_keyed_f32(const float* xt, const float* et, int64_t et_bstride, const uint32_t* keys,
                                              const float* y, int64_t y_stride, const int32_t* rank, int32_t n_kept_max,
                                              float* x0, float* xt_next, int32_t B, int32_t HW,
                                              const ddnm_step_scalars* s, void* stream) {
    if (!xt || !et || !y || !rank || !xt_next || !s || B <= 0 || HW <= 0 || !keys_ok(keys)) return DDNM_E_BADARG;
    if (et_bstride & 3) return DDNM_E_SHAPE;
    if (int e = inpaint_pi_args(n_kept_max, y_stride, HW)) return e;
    return launch_step_inpaint(xt, et, et_bstride, keyed_src(keys, s, (int64_t)3 * HW), y, y_stride, rank, (int64_t)HW, x0, xt_next,
                               B, HW, s, stream);
}

// ---------------------------------------------------------------- fused: demosaicing (colour filter array)
// Pixel (r, c) keeps the one channel pattern[r % ph][c % pw] (0 = R, 1 = G, 2 = B; 1 <= ph, pw <= 8): the reference's
// Inpainting over the HWC-interleaved entries with the two unsampled entries of every pixel missing
// (svd_operators.py:324-359), so y[b][p] = x[b][cfa(p)][p] in pixel order and every singular value is 1.  The pattern
// travels by value in the kernel arguments, two bits per site of the period: no table is read.
struct Cfa {
    uint64_t w[2];   // code of site k = r % ph * pw + c % pw: bits 2 (k & 31) .. of w[k >> 5]
    int ph, pw;
};

// DDNM_E_SHAPE for a period outside 1..8 or a code above 2 (the caller has checked the pointer)
static int cfa_pack(const uint8_t* pattern_host, int32_t ph, int32_t pw, Cfa* out) {
    if (ph < 1 || ph > 8 || pw < 1 || pw > 8) return DDNM_E_SHAPE;
    Cfa c{{0, 0}, ph, pw};
    for (int k = 0; k < ph * pw; ++k) {
        if (pattern_host[k] > 2) return DDNM_E_SHAPE;
        c.w[k >> 5] |= (uint64_t)pattern_host[k] << (2 * (k & 31));
    }
    *out = c;
    return 0;
}

// channel codes of the four pixels p4 * 4 .. + 3 of an image (one row: W % 4 == 0)
__device__ __forceinline__ void cfa_codes(const Cfa& f, int64_t p4, int W, int code[4]) {
    const int64_t pix = p4 * 4;
    const int r = (int)(pix / W);
    int cc = (int)(pix - (int64_t)r * W) % f.pw;
    const int row = r % f.ph * f.pw;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = row + cc;
        code[j] = (int)(((k < 32 ? f.w[0] : f.w[1]) >> (2 * (k & 31))) & 3);
        cc = cc + 1 == f.pw ? 0 : cc + 1;
    }
}

// one thread per four consecutive pixels of all three planes, one float4 of y: 13 planes of HW floats per image with
// in-kernel noise and x0 written (xt, et: 6 read; y: 1; x0, xt': 6 written)
template <class NZ>
__global__ __launch_bounds__(256) void step_mosaic_kernel(const float* __restrict__ xt, const float* __restrict__ et,
                                                          int64_t et_bstride, NZ noise,
                                                          const float* __restrict__ y, float* __restrict__ x0o,
                                                          float* __restrict__ xn, int W, int64_t hw4, int64_t total4,
                                                          ddnm_step_scalars s, Cfa cfa) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / hw4, p = i - b * hw4;
        const auto nz = bind(noise, b);
        const int64_t base = (b * 3 * hw4 + p) * 4, ebase = b * et_bstride + p * 4;
        const f32x4 yv = ld4(y + i * 4);
        int code[4];
        cfa_codes(cfa, p, W, code);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const f32x4 e = ld4(et + ebase + c * hw4 * 4);
            const f32x4 x0 = x0_of(ld4(xt + base + c * hw4 * 4), e, s);
            if (x0o) st4(x0o + base + c * hw4 * 4, x0);
            f32x4 x0h = x0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (code[j] == c) x0h[j] = x0[j] - (x0[j] - yv[j]) * s.lambda;
            st4(xn + base + c * hw4 * 4, update_of(x0h, nz4(nz, base + c * hw4 * 4), e, s));
        }
    }
}

// sizes and pattern of every mosaic entry point, after its pointer checks (DDNM_E_BADARG before DDNM_E_SHAPE)
static int mosaic_args(int32_t B, int32_t H, int32_t W, int64_t et_bstride, const uint8_t* pattern_host, int32_t ph, int32_t pw,
                       Cfa* cfa) {
    if (!pattern_host || B <= 0 || H <= 0 || W <= 0) return DDNM_E_BADARG;
    if ((H & 3) || (W & 3) || (et_bstride & 3)) return DDNM_E_SHAPE;
    return cfa_pack(pattern_host, ph, pw, cfa);
}

template <class Src>
static int launch_step_mosaic(const float* xt, const float* et, int64_t et_bstride, Src src, const float* y, float* x0, float* xt_next,
                              int32_t B, int32_t H, int32_t W, const uint8_t* pattern_host, int32_t ph, int32_t pw,
                              const ddnm_step_scalars* s, void* stream) {
    Cfa cfa;
    if (int e = mosaic_args(B, H, W, et_bstride, pattern_host, ph, pw, &cfa)) return e;
    const int64_t hw4 = (int64_t)H * W / 4, total4 = B * hw4;
    DDNM_LAUNCH(step_mosaic_kernel<Src>, GRID_1D(total4), dim3(256), 0, (hipStream_t)stream, xt, et, et_bstride, src, y, x0, xt_next,
                W, hw4, total4, *s, cfa);
    return 0;
}

extern "C" int ddnm_step_mosaic_f32(const float* xt, const float* et, int64_t et_bstride, const float* noise, const float* y,
                                    float* x0, float* xt_next, int32_t B, int32_t H, int32_t W, const uint8_t* pattern_host,
                                    int32_t ph, int32_t pw, const ddnm_step_scalars* s, void* stream) {
    if (!xt || !et || !y || !xt_next || !s || !noise_ok(noise, s)) return DDNM_E_BADARG;
    return launch_step_mosaic(xt, et, et_bstride, noise_src(noise, s, (int64_t)3 * H * W), y, x0, xt_next, B, H, W, pattern_host, ph,
                              pw, s, stream);
}

// The whole DDNM+ reverse step (functions/svd_ddnm.py:118-131) of the mosaic: every singular value is 1, so Lambda and
// Lambda_noise are diagonal in the image (svd_operators.py:361-439) and with a = sqrt_at_next, n ~ N(0, I),
// (lambda, d1r, d2r) on the sampled entries and (1, d1n, d2n) on the others
//   x0      = (x_t - eps * sqrt_1m_at) / sqrt_at                       (written uncorrected)
//   x_{t-1} = a x0 - a lambda (x0 - y) + d1r n + d2r eps               sampled entries
//   x_{t-1} = a x0 + d1n n + d2n eps                                   the other entries
// The five coefficients come from the host (svd_operators.cs_plus_coefficients), like CsPlusCoef.
struct CsPlusCoef { float al, d1n, d2n, dd1, dd2; };   // a*lambda, d1n, d2n, d1r - d1n, d2r - d2n

template <class NZ>
__global__ __launch_bounds__(256) void step_plus_mosaic_kernel(const float* __restrict__ xt, const float* __restrict__ et,
                                                               int64_t et_bstride, NZ noise,
                                                               const float* __restrict__ y, float* __restrict__ x0o,
                                                               float* __restrict__ xn, int W, int64_t hw4, int64_t total4,
                                                               ddnm_step_scalars s, Cfa cfa, CsPlusCoef k) {
    const float a = s.sqrt_at_next, d1r = k.d1n + k.dd1, d2r = k.d2n + k.dd2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / hw4, p = i - b * hw4;
        const auto nz = bind(noise, b);
        const int64_t base = (b * 3 * hw4 + p) * 4, ebase = b * et_bstride + p * 4;
        const f32x4 yv = ld4(y + i * 4);
        int code[4];
        cfa_codes(cfa, p, W, code);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const f32x4 e = ld4(et + ebase + c * hw4 * 4);
            const f32x4 x0 = x0_of(ld4(xt + base + c * hw4 * 4), e, s);
            st4(x0o + base + c * hw4 * 4, x0);
            const f32x4 n = nz4(nz, base + c * hw4 * 4);
            f32x4 al, d1, d2;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool m = code[j] == c;
                al[j] = m ? k.al : 0.f;
                d1[j] = m ? d1r : k.d1n;
                d2[j] = m ? d2r : k.d2n;
            }
            st4(xn + base + c * hw4 * 4, ((x0 * a - (x0 - yv) * al) + n * d1) + e * d2);
        }
    }
}

template <class Src>
static int launch_step_plus_mosaic(const float* xt, const float* et, int64_t et_bstride, Src src, const float* y, float* x0_out,
                                   float* xt_next, int32_t B, int32_t H, int32_t W, const uint8_t* pattern_host, int32_t ph,
                                   int32_t pw, CsPlusCoef k, const ddnm_step_scalars* s, void* stream) {
    Cfa cfa;
    if (int e = mosaic_args(B, H, W, et_bstride, pattern_host, ph, pw, &cfa)) return e;
    const int64_t hw4 = (int64_t)H * W / 4, total4 = B * hw4;
    DDNM_LAUNCH(step_plus_mosaic_kernel<Src>, GRID_1D(total4), dim3(256), 0, (hipStream_t)stream, xt, et, et_bstride, src, y, x0_out,
                xt_next, W, hw4, total4, *s, cfa, k);
    return 0;
}

extern "C" int ddnm_step_plus_mosaic_f32(const float* xt, const float* et, int64_t et_bstride, const float* noise,
                                         const float* y, float* x0_out, float* xt_next, int32_t B, int32_t H, int32_t W,
                                         const uint8_t* pattern_host, int32_t ph, int32_t pw, float a_lambda, float d1n,
                                         float d2n, float dd1, float dd2, const ddnm_step_scalars* s, void* stream) {
    if (!xt || !et || !y || !x0_out || !xt_next || !s || !noise_ok(noise, s)) return DDNM_E_BADARG;
    return launch_step_plus_mosaic(xt, et, et_bstride, noise_src(noise, s, (int64_t)3 * H * W), y, x0_out, xt_next, B, H, W,
                                   pattern_host, ph, pw, CsPlusCoef{a_lambda, d1n, d2n, dd1, dd2}, s, stream);
}

extern "C" int ddnm_step_plus_mosaic_keyed_f32(const float* xt, const float* et, int64_t et_bstride, const uint32_t* keys,
                                               const float* y, float* x0_out, float* xt_next, int32_t B, int32_t H, int32_t W,
                                               const uint8_t* pattern_host, int32_t ph, int32_t pw, float a_lambda, float d1n,
                                               float d2n, float dd1, float dd2, const ddnm_step_scalars* s, void* stream) {
    if (!xt || !et || !y || !x0_out || !xt_next || !s || !keys_ok(keys)) return DDNM_E_BADARG;
    return launch_step_plus_mosaic(xt, et, et_bstride, keyed_src(keys, s, (int64_t)3 * H * W), y, x0_out, xt_next, B, H, W,
                                   pattern_host, ph, pw, CsPlusCoef{a_lambda, d1n, d2n, dd1, dd2}, s, stream);
}

// ---------------------------------------------------------------- fused: denoising (A = I)
template <class NZ>
__global__ __launch_bounds__(256) void step_denoise_kernel(const float* __restrict__ xt, const float* __restrict__ et,
                                                           int64_t et_bstride, NZ noise,
                                                           const float* __restrict__ y, float* __restrict__ x0o,
                                                           float* __restrict__ xn, int64_t chw4, int64_t total4,
                                                           ddnm_step_scalars s) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / chw4, r = i - b * chw4;
        const auto nz = bind(noise, b);
        const f32x4 e = ld4(et + b * et_bstride + r * 4);
        const f32x4 x0 = x0_of(ld4(xt + i * 4), e, s);
        if (x0o) st4(x0o + i * 4, x0);
        const f32x4 x0h = x0 - (x0 - ld4(y + i * 4)) * s.lambda;
        st4(xn + i * 4, update_of(x0h, nz4(nz, i * 4), e, s));
    }
}

template <class Src>
static int launch_step_denoise(const float* xt, const float* et, int64_t et_bstride, Src src, const float* y, float* x0, float* xt_next,
                               int32_t B, int64_t chw, const ddnm_step_scalars* s, void* stream) {
    if (B <= 0 || chw <= 0) return DDNM_E_BADARG;
    if ((chw & 3) || (et_bstride & 3)) return DDNM_E_SHAPE;
    const int64_t total4 = (int64_t)B * chw / 4;
    DDNM_LAUNCH(step_denoise_kernel<Src>, GRID_1D(total4), dim3(256), 0, (hipStream_t)stream, xt, et, et_bstride, src, y, x0, xt_next,
                chw / 4, total4, *s);
    return 0;
}

extern "C" int ddnm_step_denoise_f32(const float* xt, const float* et, int64_t et_bstride, const float* noise,
                                     const float* y, float* x0, float* xt_next, int32_t B, int64_t chw,
                                     const ddnm_step_scalars* s, void* stream) {
    if (!xt || !et || !y || !xt_next || !s || !noise_ok(noise, s)) return DDNM_E_BADARG;
    return launch_step_denoise(xt, et, et_bstride, noise_src(noise, s, chw), y, x0, xt_next, B, chw, s, stream);
}

// ---------------------------------------------------------------- fused DDNM+: per-entry measurement noise (mosaic, denoising)
// The DDNM+ reverse step (functions/svd_ddnm.py:118-131) of the two operators whose U is the identity and whose measured
// entries all have singular value 1 (svd_operators.py:361-439 over single entries, :442-476), with a DIAGONAL noise
// covariance: entry j of y carries its own sigma_j, which is already diagonal in the operator's spectral basis, so the
// rules of spectral_coefficients(1, ...) (the change_index masks of svd_operators.py:367-436) hold per entry.  With
// a = sqrt_at_next, thr = a sigma_j and (st, st2, c1, c2) = (sigma_t, sigma_t^2, sigma_t eta, sigma_t sqrt(1 - eta^2)) of HnCoef:
//   sigma_j == 0 or a == 0 : (a lambda, d1, d2) = (a, c1, c2)
//   st < thr               : (a * (c2 / thr), c1, 0)
//   st > thr               : (a, sqrt(st2 - thr * thr), 0)          (the difference is clamped at 0 before the root)
//   st == thr              : (a, c1, c2)
//   x_{t-1} = ((a x0 - a lambda (x0 - y)) + d1 n) + d2 eps          unmeasured entries: (0, c1, c2), i.e. a x0 + c1 n + c2 eps
// The kernels are templates on the sigma source as they are on the noise source: SigmaMap loads sigma_j (engine scale,
// [-1, 1]) with the float4 index of y inside the image -- one row, shared by the batch --; SigmaShot evaluates
// sigma_j = 2 sqrt(s2 + g u_j), u_j = clamp((y_j + 1) / 2, 0, 1), from the y already in registers (s2, g on the [0, 1]
// scale): no table, no extra bytes.
struct SigmaMap { const float* p; };
struct SigmaShot { float s2, g; };
struct HnCoef { float st, st2, c1, c2; };

__device__ __forceinline__ f32x4 sigma4(const SigmaMap& m, f32x4, int64_t off) { return ld4(m.p + off); }
__device__ __forceinline__ f32x4 sigma4(const SigmaShot& m, f32x4 y, int64_t) {
    f32x4 sg;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float u = (y[j] + 1.f) * 0.5f;
        u = u < 0.f ? 0.f : (u > 1.f ? 1.f : u);
        sg[j] = 2.f * sqrtf(m.s2 + m.g * u);
    }
    return sg;
}

// (a lambda, d1, d2) of four measured entries
__device__ __forceinline__ void hn_coef4(f32x4 sg, float a, const HnCoef& k, f32x4& al, f32x4& d1, f32x4& d2) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float thr = a * sg[j];
        al[j] = a, d1[j] = k.c1, d2[j] = k.c2;
        if (sg[j] == 0.f || a == 0.f) continue;
        if (k.st < thr) {
            al[j] = a * (k.c2 / thr);
            d2[j] = 0.f;
        } else if (k.st > thr) {
            const float v = k.st2 - thr * thr;
            d1[j] = sqrtf(v > 0.f ? v : 0.f);
            d2[j] = 0.f;
        }
    }
}

// the mosaic: step_plus_mosaic_kernel with the coefficients of the sampled entry evaluated per pixel -- 14 planes of HW
// floats per image with in-kernel noise, one more (the row, once per image) for SigmaMap
template <class NZ, class SG>
__global__ __launch_bounds__(256) void step_plus_mosaic_hn_kernel(const float* __restrict__ xt, const float* __restrict__ et,
                                                                  int64_t et_bstride, NZ noise, const float* __restrict__ y,
                                                                  SG sigma, float* __restrict__ x0o, float* __restrict__ xn,
                                                                  int W, int64_t hw4, int64_t total4, ddnm_step_scalars s,
                                                                  Cfa cfa, HnCoef k) {
    const float a = s.sqrt_at_next;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / hw4, p = i - b * hw4;
        const auto nz = bind(noise, b);
        const int64_t base = (b * 3 * hw4 + p) * 4, ebase = b * et_bstride + p * 4;
        const f32x4 yv = ld4(y + i * 4);
        f32x4 alm, d1m, d2m;
        hn_coef4(sigma4(sigma, yv, p * 4), a, k, alm, d1m, d2m);
        int code[4];
        cfa_codes(cfa, p, W, code);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const f32x4 e = ld4(et + ebase + c * hw4 * 4);
            const f32x4 x0 = x0_of(ld4(xt + base + c * hw4 * 4), e, s);
            st4(x0o + base + c * hw4 * 4, x0);
            const f32x4 n = nz4(nz, base + c * hw4 * 4);
            f32x4 al, d1, d2;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool m = code[j] == c;
                al[j] = m ? alm[j] : 0.f;
                d1[j] = m ? d1m[j] : k.c1;
                d2[j] = m ? d2m[j] : k.c2;
            }
            st4(xn + base + c * hw4 * 4, ((x0 * a - (x0 - yv) * al) + n * d1) + e * d2);
        }
    }
}

// denoising (A = I): every entry is measured; y [B][chw], the row [chw]
template <class NZ, class SG>
__global__ __launch_bounds__(256) void step_plus_denoise_hn_kernel(const float* __restrict__ xt, const float* __restrict__ et,
                                                                   int64_t et_bstride, NZ noise, const float* __restrict__ y,
                                                                   SG sigma, float* __restrict__ x0o, float* __restrict__ xn,
                                                                   int64_t chw4, int64_t total4, ddnm_step_scalars s, HnCoef k) {
    const float a = s.sqrt_at_next;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / chw4, r = i - b * chw4;
        const auto nz = bind(noise, b);
        const f32x4 e = ld4(et + b * et_bstride + r * 4);
        const f32x4 x0 = x0_of(ld4(xt + i * 4), e, s);
        st4(x0o + i * 4, x0);
        const f32x4 yv = ld4(y + i * 4);
        f32x4 al, d1, d2;
        hn_coef4(sigma4(sigma, yv, r * 4), a, k, al, d1, d2);
        st4(xn + i * 4, ((x0 * a - (x0 - yv) * al) + nz4(nz, i * 4) * d1) + e * d2);
    }
}

// The noise model of an *_hn_* entry point, after its pointer checks: sigma_mode 0 = the row `sigma_map`, 1 = shot + read.
enum { DDNM_HN_MAP = 0, DDNM_HN_SHOT = 1 };
static inline bool hn_ptrs(const float* sigma_map, int32_t sigma_mode) {      // the row is read 16 bytes at a time
    return sigma_mode != DDNM_HN_MAP || (sigma_map != nullptr && (reinterpret_cast<uintptr_t>(sigma_map) & 15) == 0);
}
static inline bool hn_nonneg(float v) { return isfinite(v) && v >= 0.f; }
static int hn_model(int32_t sigma_mode, float s2, float g, float sigma_t, float sigma_t2, float c1, float c2) {
    if (sigma_mode != DDNM_HN_MAP && sigma_mode != DDNM_HN_SHOT) return DDNM_E_SHAPE;
    if (sigma_mode == DDNM_HN_SHOT && (!hn_nonneg(s2) || !hn_nonneg(g))) return DDNM_E_SHAPE;
    if (!hn_nonneg(sigma_t) || !hn_nonneg(sigma_t2) || !isfinite(c1) || !isfinite(c2)) return DDNM_E_SHAPE;
    return 0;
}

template <class Src>
static int launch_step_plus_mosaic_hn(const float* xt, const float* et, int64_t et_bstride, Src src, const float* y, float* x0_out,
                                      float* xt_next, int32_t B, int32_t H, int32_t W, const uint8_t* pattern_host, int32_t ph,
                                      int32_t pw, const float* sigma_map, int32_t sigma_mode, float s2, float g, HnCoef k,
                                      const ddnm_step_scalars* s, void* stream) {
    Cfa cfa;
    if (!hn_ptrs(sigma_map, sigma_mode)) return DDNM_E_BADARG;
    if (int e = mosaic_args(B, H, W, et_bstride, pattern_host, ph, pw, &cfa)) return e;
    if (int e = hn_model(sigma_mode, s2, g, k.st, k.st2, k.c1, k.c2)) return e;
    const int64_t hw4 = (int64_t)H * W / 4, total4 = B * hw4;
    if (sigma_mode == DDNM_HN_MAP)
        DDNM_LAUNCH((step_plus_mosaic_hn_kernel<Src, SigmaMap>), GRID_1D(total4), dim3(256), 0, (hipStream_t)stream, xt, et,
                    et_bstride, src, y, SigmaMap{sigma_map}, x0_out, xt_next, W, hw4, total4, *s, cfa, k);
    else
        DDNM_LAUNCH((step_plus_mosaic_hn_kernel<Src, SigmaShot>), GRID_1D(total4), dim3(256), 0, (hipStream_t)stream, xt, et,
                    et_bstride, src, y, SigmaShot{s2, g}, x0_out, xt_next, W, hw4, total4, *s, cfa, k);
    return 0;
}

template <class Src>
static int launch_step_plus_denoise_hn(const float* xt, const float* et, int64_t et_bstride, Src src, const float* y, float* x0_out,
                                       float* xt_next, int32_t B, int64_t chw, const float* sigma_map, int32_t sigma_mode, float s2,
                                       float g, HnCoef k, const ddnm_step_scalars* s, void* stream) {
    if (!hn_ptrs(sigma_map, sigma_mode) || B <= 0 || chw <= 0) return DDNM_E_BADARG;
    if ((chw & 3) || (et_bstride & 3)) return DDNM_E_SHAPE;
    if (int e = hn_model(sigma_mode, s2, g, k.st, k.st2, k.c1, k.c2)) return e;
    const int64_t total4 = (int64_t)B * chw / 4;
    if (sigma_mode == DDNM_HN_MAP)
        DDNM_LAUNCH((step_plus_denoise_hn_kernel<Src, SigmaMap>), GRID_1D(total4), dim3(256), 0, (hipStream_t)stream, xt, et,
                    et_bstride, src, y, SigmaMap{sigma_map}, x0_out, xt_next, chw / 4, total4, *s, k);
    else
        DDNM_LAUNCH((step_plus_denoise_hn_kernel<Src, SigmaShot>), GRID_1D(total4), dim3(256), 0, (hipStream_t)stream, xt, et,
                    et_bstride, src, y, SigmaShot{s2, g}, x0_out, xt_next, chw / 4, total4, *s, k);
    return 0;
}

extern "C" int ddnm_step_plus_mosaic_hn_f32(const float* xt, const float* et, int64_t et_bstride, const float* noise,
                                            const float* y, float* x0_out, float* xt_next, int32_t B, int32_t H, int32_t W,
                                            const uint8_t* pattern_host, int32_t ph, int32_t pw, const float* sigma_map,
                                            int32_t sigma_mode, float s2, float g, float sigma_t, float sigma_t2, float c1,
                                            float c2, const ddnm_step_scalars* s, void* stream) {
    if (!xt || !et || !y || !x0_out || !xt_next || !s || !noise_ok(noise, s)) return DDNM_E_BADARG;
    return launch_step_plus_mosaic_hn(xt, et, et_bstride, noise_src(noise, s, (int64_t)3 * H * W), y, x0_out, xt_next, B, H, W,
                                      pattern_host, ph, pw, sigma_map, sigma_mode, s2, g, HnCoef{sigma_t, sigma_t2, c1, c2}, s,
                                      stream);
}

extern "C" int ddnm_step_plus_mosaic_hn_keyed_f32(const float* xt, const float* et, int64_t et_bstride, const uint32_t* keys,
                                                  const float* y, float* x0_out, float* xt_next, int32_t B, int32_t H,
                                                  int32_t W, const uint8_t* pattern_host, int32_t ph, int32_t pw,
                                                  const float* sigma_map, int32_t sigma_mode, float s2, float g, float sigma_t,
                                                  float sigma_t2, float c1, float c2, const ddnm_step_scalars* s, void* stream) {
    if (!xt || !et || !y || !x0_out || !xt_next || !s || !keys_ok(keys)) return DDNM_E_BADARG;
    return launch_step_plus_mosaic_hn(xt, et, et_bstride, keyed_src(keys, s, (int64_t)3 * H * W), y, x0_out, xt_next, B, H, W,
                                      pattern_host, ph, pw, sigma_map, sigma_mode, s2, g, HnCoef{sigma_t, sigma_t2, c1, c2}, s,
                                      stream);
}

extern "C" int ddnm_step_plus_denoise_hn_f32(const float* xt, const float* et, int64_t et_bstride, const float* noise,
                                             const float* y, float* x0_out, float* xt_next, int32_t B, int64_t chw,
                                             const float* sigma_map, int32_t sigma_mode, float s2, float g, float sigma_t,
                                             float sigma_t2, float c1, float c2, const ddnm_step_scalars* s, void* stream) {
    if (!xt || !et || !y || !x0_out || !xt_next || !s || !noise_ok(noise, s)) return DDNM_E_BADARG;
    return launch_step_plus_denoise_hn(xt, et, et_bstride, noise_src(noise, s, chw), y, x0_out, xt_next, B, chw, sigma_map,
                                       sigma_mode, s2, g, HnCoef{sigma_t, sigma_t2, c1, c2}, s, stream);
}

extern "C" int ddnm_step_plus_denoise_hn_keyed_f32(const float* xt, const float* et, int64_t et_bstride, const uint32_t* keys,
                                                   const float* y, float* x0_out, float* xt_next, int32_t B, int64_t chw,
                                                   const float* sigma_map, int32_t sigma_mode, float s2, float g, float sigma_t,
                                                   float sigma_t2, float c1, float c2, const ddnm_step_scalars* s,
                                                   void* stream) {
    if (!xt || !et || !y || !x0_out || !xt_next || !s || !keys_ok(keys)) return DDNM_E_BADARG;
    return launch_step_plus_denoise_hn(xt, et, et_bstride, keyed_src(keys, s, chw), y, x0_out, xt_next, B, chw, sigma_map,
                                       sigma_mode, s2, g, HnCoef{sigma_t, sigma_t2, c1, c2}, s, stream);
}

// ---------------------------------------------------------------- keyed entry points: same launchers, per-image keys
extern "C" int ddnm_step_combine_keyed_f32(const float* x0, const float* proj, const float* apy, const uint32_t* keys,
                                           const float* et, int64_t et_bstride, float* xt_next, int32_t B, int64_t chw,
                                           const ddnm_step_scalars* s, void* stream) {
    if (!x0 || !proj || !et || !xt_next || !s || !keys_ok(keys)) return DDNM_E_BADARG;
    return launch_step_combine(x0, proj, apy, keyed_src(keys, s, chw), et, et_bstride, xt_next, B, chw, s, stream);
}

extern "C" int ddnm_step_sr_avgpool_keyed_f32(const float* xt, const float* et, int64_t et_bstride, const uint32_t* keys,
                                              const float* y, float* x0, float* xt_next, int32_t B, int32_t H, int32_t W,
                                              int32_t r, const ddnm_step_scalars* s, void* stream) {
    if (!xt || !et || !y || !xt_next || !s || !keys_ok(keys)) return DDNM_E_BADARG;
    return launch_step_sr4(xt, et, et_bstride, keyed_src(keys, s, (int64_t)3 * H * W), y, x0, xt_next, B, H, W, r, s, stream);
}

extern "C" int ddnm_step_color_keyed_f32(const float* xt, const float* et, int64_t et_bstride, const uint32_t* keys,
                                         const float* y, float* x0, float* xt_next, int32_t B, int32_t HW,
                                         const float* w3_host, const ddnm_step_scalars* s, void* stream) {
    if (!xt || !et || !y || !xt_next || !s || !keys_ok(keys)) return DDNM_E_BADARG;
    return launch_step_color(xt, et, et_bstride, keyed_src(keys, s, (int64_t)3 * HW), y, x0, xt_next, B, HW, w3_host, s, stream);
}

extern "C" int ddnm_step_inpaint_keyed_f32(const float* xt, const float* et, int64_t et_bstride, const uint32_t* keys,
                                           const float* y, const int32_t* rank, int32_t n_kept, float* x0, float* xt_next,
                                           int32_t B, int32_t HW, const ddnm_step_scalars* s, void* stream) {
    if (!xt || !et || !y || !rank || !xt_next || !s || B <= 0 || HW <= 0 || !keys_ok(keys)) return DDNM_E_BADARG;
    if ((HW & 3) || (et_bstride & 3)) return DDNM_E_SHAPE;
    return launch_step_inpaint(xt, et, et_bstride, keyed_src(keys, s, (int64_t)3 * HW), y, (int64_t)3 * n_kept, rank, (int64_t)0, x0,
                               xt_next, B, HW, s, stream);
}

extern "C" int ddnm_step_mosaic_keyed_f32(const float* xt, const float* et, int64_t et_bstride, const uint32_t* keys,
                                          const float* y, float* x0, float* xt_next, int32_t B, int32_t H, int32_t W,
                                          const uint8_t* pattern_host, int32_t ph, int32_t pw, const ddnm_step_scalars* s,
                                          void* stream) {
    if (!xt || !et || !y || !xt_next || !s || !keys_ok(keys)) return DDNM_E_BADARG;
    return launch_step_mosaic(xt, et, et_bstride, keyed_src(keys, s, (int64_t)3 * H * W), y, x0, xt_next, B, H, W, pattern_host, ph,
                              pw, s, stream);
}

extern "C" int ddnm_step_denoise_keyed_f32(const float* xt, const float* et, int64_t et_bstride, const uint32_t* keys,
                                           const float* y, float* x0, float* xt_next, int32_t B, int64_t chw,
                                           const ddnm_step_scalars* s, void* stream) {
    if (!xt || !et || !y || !xt_next || !s || !keys_ok(keys)) return DDNM_E_BADARG;
    return launch_step_denoise(xt, et, et_bstride, keyed_src(keys, s, chw), y, x0, xt_next, B, chw, s, stream);
}

// ---------------------------------------------------------------- stand-alone Philox draw
// out[b][r .. r+3] = philox_normal4(seed, r / 4, iter, img_base + b): exactly the values the step kernels draw in-kernel for
// the same (seed, iteration, image); used for x_T, the time-travel re-noise, DDNM+ (whose Lambda_noise reads the tensor)
__global__ __launch_bounds__(256) void randn_philox_kernel(float* __restrict__ out, int64_t chw4, int64_t total4, PhiloxKey key,
                                                           unsigned iter, unsigned img_base) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / chw4, r = i - b * chw4;
        st4(out + i * 4, philox_normal4(key, (unsigned)r, iter, img_base + (unsigned)b));
    }
}

extern "C" int ddnm_randn_philox_f32(float* out, int32_t B, int64_t chw, uint32_t seed_lo, uint32_t seed_hi, uint32_t iter,
                                     uint32_t image_base, void* stream) {
    if (!out || B <= 0 || chw <= 0) return DDNM_E_BADARG;
    if (chw & 3) return DDNM_E_SHAPE;
    const int64_t total4 = (int64_t)B * chw / 4;
    DDNM_LAUNCH(randn_philox_kernel, GRID_1D(total4), dim3(256), 0, (hipStream_t)stream, out, chw / 4, total4,
                PhiloxKey{seed_lo, seed_hi}, iter, image_base);
    return 0;
}

// keyed draw of any row length n: thread i = (image b, block g of four); rows are 16-byte aligned only when n % 4 == 0,
// otherwise (and for the last partial block) the values are stored one by one, the partial block's first n % 4 only
__global__ __launch_bounds__(256) void randn_philox_keyed_kernel(float* __restrict__ out, const uint4* __restrict__ keys,
                                                                 int64_t n, int64_t n4, int64_t total4, unsigned iter) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / n4, g = i - b * n4;
        const uint4 k = keys[b];
        const f32x4 v = philox_normal4(PhiloxKey{k.x, k.y}, (unsigned)g, iter, k.z);
        float* o = out + b * n + g * 4;
        if ((n & 3) == 0) {
            st4(o, v);
        } else {
            const int64_t m = n - g * 4;
            o[0] = v.x;
            if (m > 1) o[1] = v.y;
            if (m > 2) o[2] = v.z;
            if (m > 3) o[3] = v.w;
        }
    }
}

extern "C" int ddnm_randn_philox_keyed_f32(float* out, int32_t B, int64_t n, const uint32_t* keys, uint32_t iter,
                                           void* stream) {
    if (!out || B <= 0 || n <= 0 || !keys_ok(keys)) return DDNM_E_BADARG;
    const int64_t n4 = (n + 3) / 4, total4 = (int64_t)B * n4;
    DDNM_LAUNCH(randn_philox_keyed_kernel, GRID_1D(total4), dim3(256), 0, (hipStream_t)stream, out,
                reinterpret_cast<const uint4*>(keys), n, n4, total4, iter);
    return 0;
}

// ---------------------------------------------------------------- time-travel re-noise
__global__ __launch_bounds__(256) void renoise_kernel(const float* __restrict__ x0, const float* __restrict__ noise,
                                                      float* __restrict__ xn, int64_t n4, float a, float b) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256)
        st4(xn + i * 4, ld4(x0 + i * 4) * a + ld4(noise + i * 4) * b);
}

extern "C" int ddnm_renoise_f32(const float* x0, const float* noise, float* xt_next, int64_t n, float a, float b,
                                void* stream) {
    if (!x0 || !noise || !xt_next || n <= 0) return DDNM_E_BADARG;
    if (n & 3) return DDNM_E_SHAPE;
    DDNM_LAUNCH(renoise_kernel, GRID_1D(n / 4), dim3(256), 0, (hipStream_t)stream, x0, noise, xt_next, n / 4, a,
                       b);
    return 0;
}

// out[i] = value (zero padding rows of token matrices, cleared accumulators): keeps ATen fill kernels off the path
__global__ __launch_bounds__(256) void fill_kernel(float* __restrict__ out, int64_t n, float value) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = value;
}

extern "C" int ddnm_fill_f32(float* out, int64_t n, float value, void* stream) {
    if (!out || n <= 0) return DDNM_E_BADARG;
    DDNM_LAUNCH(fill_kernel, GRID_1D(n), dim3(256), 0, (hipStream_t)stream, out, n, value);
    return 0;
}

// ================================================================ stand-alone operators
__global__ __launch_bounds__(256) void avgpool_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W,
                                                      int r, int64_t total) {
    const int Wy = W / r, Hy = H / r;
    const float div = (float)(r * r);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t bc = i / ((int64_t)Hy * Wy);
        const int64_t q = i - bc * Hy * Wy;
        const int py = (int)(q / Wy), px = (int)(q - (int64_t)py * Wy);
        const float* p = x + (bc * H + (int64_t)py * r) * W + (int64_t)px * r;
        float sum = 0.f;
        for (int j = 0; j < r; ++j)
            for (int k = 0; k < r; ++k) sum += p[(int64_t)j * W + k];
        y[i] = sum / div;
    }
}

extern "C" int ddnm_op_avgpool_f32(const float* x, float* y, int32_t BC, int32_t H, int32_t W, int32_t r,
                                   void* stream) {
    if (!x || !y || BC <= 0 || r <= 0) return DDNM_E_BADARG;
    if (H % r || W % r) return DDNM_E_SHAPE;
    const int64_t total = (int64_t)BC * (H / r) * (W / r);
    DDNM_LAUNCH(avgpool_kernel, GRID_1D(total), dim3(256), 0, (hipStream_t)stream, x, y, H, W, r, total);
    return 0;
}

__global__ __launch_bounds__(256) void upsample_kernel(const float* __restrict__ y, float* __restrict__ x, int H, int W,
                                                       int r, int64_t total) {
    const int Wy = W / r, Hy = H / r;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t bc = i / ((int64_t)H * W);
        const int64_t q = i - bc * H * W;
        const int yy = (int)(q / W), xx = (int)(q - (int64_t)yy * W);
        x[i] = y[(bc * Hy + yy / r) * Wy + xx / r];
    }
}

extern "C" int ddnm_op_upsample_f32(const float* y, float* x, int32_t BC, int32_t H, int32_t W, int32_t r,
                                    void* stream) {
    if (!x || !y || BC <= 0 || r <= 0) return DDNM_E_BADARG;
    if (H % r || W % r) return DDNM_E_SHAPE;
    const int64_t total = (int64_t)BC * H * W;
    DDNM_LAUNCH(upsample_kernel, GRID_1D(total), dim3(256), 0, (hipStream_t)stream, y, x, H, W, r, total);
    return 0;
}

__global__ __launch_bounds__(256) void color_A_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t HW,
                                                      int64_t total, ColorW cw) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / HW, p = i - b * HW;
        const float* s = x + b * 3 * HW + p;
        y[i] = (s[0] * cw.w[0] + s[HW] * cw.w[1]) + s[2 * HW] * cw.w[2];
    }
}

extern "C" int ddnm_op_color_A_f32(const float* x, float* y, int32_t B, int32_t HW, const float* w3_host,
                                   void* stream) {
    if (!x || !y || B <= 0 || HW <= 0) return DDNM_E_BADARG;
    const int64_t total = (int64_t)B * HW;
    DDNM_LAUNCH(color_A_kernel, GRID_1D(total), dim3(256), 0, (hipStream_t)stream, x, y, (int64_t)HW, total,
                       color_weights(w3_host));
    return 0;
}

__global__ __launch_bounds__(256) void color_pinv_kernel(const float* __restrict__ y, float* __restrict__ x, int64_t HW,
                                                         int64_t total, ColorW cw) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / HW, p = i - b * HW;
        float* d = x + b * 3 * HW + p;
        const float v = y[i];
        d[0] = v * cw.wp[0];
        d[HW] = v * cw.wp[1];
        d[2 * HW] = v * cw.wp[2];
    }
}

extern "C" int ddnm_op_color_pinv_f32(const float* y, float* x, int32_t B, int32_t HW, const float* w3_host,
                                      void* stream) {
    if (!x || !y || B <= 0 || HW <= 0) return DDNM_E_BADARG;
    const int64_t total = (int64_t)B * HW;
    DDNM_LAUNCH(color_pinv_kernel, GRID_1D(total), dim3(256), 0, (hipStream_t)stream, y, x, (int64_t)HW, total,
                       color_weights(w3_host));
    return 0;
}

// y[b][3*rank[b][p] + c] = x[b][c][p] for kept pixels (HWC-interleaved measurement vector); image b's table is at
// rank + b * rank_bstride and its row at y + b * y_bstride (shared mask: (0, 3 * n_kept); per image: (HW, y_stride),
// whose padding beyond 3 * n_kept[b] is the caller's to clear)
__global__ __launch_bounds__(256) void inpaint_A_kernel(const float* __restrict__ x, const int* __restrict__ rank,
                                                        int64_t rank_bstride, float* __restrict__ y, int64_t y_bstride,
                                                        int64_t HW, int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / HW, p = i - b * HW;
        const int rk = rank[b * rank_bstride + p];
        if (rk < 0) continue;
        const float* s = x + b * 3 * HW + p;
        float* d = y + b * y_bstride + (int64_t)rk * 3;
        d[0] = s[0];
        d[1] = s[HW];
        d[2] = s[2 * HW];
    }
}

extern "C" int ddnm_op_inpaint_A_f32(const float* x, const int32_t* rank, int32_t n_kept, float* y, int32_t B,
                                     int32_t HW, void* stream) {
    if (!x || !y || !rank || B <= 0 || HW <= 0) return DDNM_E_BADARG;
    const int64_t total = (int64_t)B * HW;
    DDNM_LAUNCH(inpaint_A_kernel, GRID_1D(total), dim3(256), 0, (hipStream_t)stream, x, rank, (int64_t)0, y,
                (int64_t)3 * n_kept, (int64_t)HW, total);
    return 0;
}

extern "C" int ddnm_op_inpaint_A_pi_f32(const float* x, const int32_t* rank, int32_t n_kept_max, float* y,
                                        int64_t y_stride, int32_t B, int32_t HW, void* stream) {
    if (!x || !y || !rank || B <= 0 || HW <= 0) return DDNM_E_BADARG;
    if (int e = inpaint_pi_args(n_kept_max, y_stride, HW)) return e;
    const int64_t total = (int64_t)B * HW;
    DDNM_LAUNCH(inpaint_A_kernel, GRID_1D(total), dim3(256), 0, (hipStream_t)stream, x, rank, (int64_t)HW, y, y_stride,
                (int64_t)HW, total);
    return 0;
}

__global__ __launch_bounds__(256) void inpaint_pinv_kernel(const float* __restrict__ y, int64_t y_bstride,
                                                           const int* __restrict__ rank, int64_t rank_bstride,
                                                           float* __restrict__ x, int64_t HW, int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / HW, p = i - b * HW;
        const int rk = rank[b * rank_bstride + p];
        float* d = x + b * 3 * HW + p;
        if (rk < 0) {
            d[0] = 0.f; d[HW] = 0.f; d[2 * HW] = 0.f;
        } else {
            const float* s = y + b * y_bstride + (int64_t)rk * 3;
            d[0] = s[0]; d[HW] = s[1]; d[2 * HW] = s[2];
        }
    }
}

extern "C" int ddnm_op_inpaint_pinv_f32(const float* y, const int32_t* rank, int32_t n_kept, float* x, int32_t B,
                                        int32_t HW, void* stream) {
    if (!x || !y || !rank || B <= 0 || HW <= 0) return DDNM_E_BADARG;
    const int64_t total = (int64_t)B * HW;
    DDNM_LAUNCH(inpaint_pinv_kernel, GRID_1D(total), dim3(256), 0, (hipStream_t)stream, y, (int64_t)3 * n_kept, rank,
                (int64_t)0, x, (int64_t)HW, total);
    return 0;
}

extern "C" int ddnm_op_inpaint_pinv_pi_f32(const float* y, int64_t y_stride, const int32_t* rank, int32_t n_kept_max,
                                           float* x, int32_t B, int32_t HW, void* stream) {
    if (!x || !y || !rank || B <= 0 || HW <= 0) return DDNM_E_BADARG;
    if (int e = inpaint_pi_args(n_kept_max, y_stride, HW)) return e;
    const int64_t total = (int64_t)B * HW;
    DDNM_LAUNCH(inpaint_pinv_kernel, GRID_1D(total), dim3(256), 0, (hipStream_t)stream, y, y_stride, rank, (int64_t)HW, x,
                (int64_t)HW, total);
    return 0;
}

// A and A^+ of the mosaic: y[b][p] = x[b][cfa(p)][p]; A^+ writes y[p] to plane cfa(p) and 0 to the other two.  One thread
// per four pixels, float4 on both sides.
__global__ __launch_bounds__(256) void mosaic_A_kernel(const float* __restrict__ x, float* __restrict__ y, int W, int64_t hw4,
                                                       int64_t total4, Cfa cfa) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / hw4, p = i - b * hw4;
        const int64_t base = (b * 3 * hw4 + p) * 4;
        int code[4];
        cfa_codes(cfa, p, W, code);
        f32x4 v = ld4(x + base);
#pragma unroll
        for (int c = 1; c < 3; ++c) {
            const f32x4 xc = ld4(x + base + c * hw4 * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (code[j] == c) v[j] = xc[j];
        }
        st4(y + i * 4, v);
    }
}

__global__ __launch_bounds__(256) void mosaic_pinv_kernel(const float* __restrict__ y, float* __restrict__ x, int W, int64_t hw4,
                                                          int64_t total4, Cfa cfa) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / hw4, p = i - b * hw4;
        const int64_t base = (b * 3 * hw4 + p) * 4;
        int code[4];
        cfa_codes(cfa, p, W, code);
        const f32x4 yv = ld4(y + i * 4);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            f32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = code[j] == c ? yv[j] : 0.f;
            st4(x + base + c * hw4 * 4, v);
        }
    }
}

extern "C" int ddnm_op_mosaic_A_f32(const float* x, float* y, int32_t B, int32_t H, int32_t W, const uint8_t* pattern_host,
                                    int32_t ph, int32_t pw, void* stream) {
    if (!x || !y) return DDNM_E_BADARG;
    Cfa cfa;
    if (int e = mosaic_args(B, H, W, 0, pattern_host, ph, pw, &cfa)) return e;
    const int64_t hw4 = (int64_t)H * W / 4, total4 = B * hw4;
    DDNM_LAUNCH(mosaic_A_kernel, GRID_1D(total4), dim3(256), 0, (hipStream_t)stream, x, y, W, hw4, total4, cfa);
    return 0;
}

extern "C" int ddnm_op_mosaic_pinv_f32(const float* y, float* x, int32_t B, int32_t H, int32_t W, const uint8_t* pattern_host,
                                       int32_t ph, int32_t pw, void* stream) {
    if (!x || !y) return DDNM_E_BADARG;
    Cfa cfa;
    if (int e = mosaic_args(B, H, W, 0, pattern_host, ph, pw, &cfa)) return e;
    const int64_t hw4 = (int64_t)H * W / 4, total4 = B * hw4;
    DDNM_LAUNCH(mosaic_pinv_kernel, GRID_1D(total4), dim3(256), 0, (hipStream_t)stream, y, x, W, hw4, total4, cfa);
    return 0;
}

// ---------------------------------------------------------------- final clamp + per-image squared error
__global__ __launch_bounds__(256) void finalize_psnr_kernel(const float* __restrict__ x, const float* __restrict__ xo,
                                                            float* __restrict__ img, double* __restrict__ sse,
                                                            int64_t chw) {
    __shared__ double red[4];
    const int b = blockIdx.y;
    const float* xb = x + (int64_t)b * chw;
    const float* ob = xo ? xo + (int64_t)b * chw : nullptr;
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < chw; i += (int64_t)gridDim.x * 256) {
        const float v = fminf(fmaxf((xb[i] + 1.0f) / 2.0f, 0.0f), 1.0f);
        if (img) img[(int64_t)b * chw + i] = v;
        if (ob) {
            const float o = fminf(fmaxf((ob[i] + 1.0f) / 2.0f, 0.0f), 1.0f);
            const float dd = v - o;
            acc += (double)(dd * dd);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0 && sse) atomicAdd(&sse[b], (red[0] + red[1]) + (red[2] + red[3]));
}

extern "C" int ddnm_finalize_psnr_f32(const float* x, const float* x_orig, float* img, double* sse, int32_t B,
                                      int64_t chw, void* stream) {
    if (!x || B <= 0 || chw <= 0 || (x_orig && !sse)) return DDNM_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (sse) {
        hipError_t e = hipMemsetAsync(sse, 0, sizeof(double) * B, st);
        if (e != hipSuccess) return (int)e;
    }
    DDNM_LAUNCH(finalize_psnr_kernel, dim3(64, B), dim3(256), 0, st, x, x_orig, img, sse, chw);
    return 0;
}

// ================================================================ DDNM+ (sigma_y > 0) building blocks
// functions/svd_ddnm.py:80-164 with the per-operator Lambda / Lambda_noise of functions/svd_operators.py.

// out = a*x + b*y   (y may be NULL)
__global__ __launch_bounds__(256) void axpby_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                    float* __restrict__ out, int64_t n, float a, float b) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        out[i] = y ? x[i] * a + y[i] * b : x[i] * a;
}

extern "C" int ddnm_axpby_f32(const float* x, const float* y, float* out, int64_t n, float a, float b, void* stream) {
    if (!x || !out || n <= 0) return DDNM_E_BADARG;
    DDNM_LAUNCH(axpby_kernel, GRID_1D(n), dim3(256), 0, (hipStream_t)stream, x, y, out, n, a, b);
    return 0;
}

// out = (m ? cx_m : cx_n) * x + (m ? cy_m : cy_n) * y, m = mask[(plane % planes_mask)][p] != 0 (NULL mask: measured
// everywhere).  Lambda / Lambda_noise of Inpainting (svd_operators.py:361-439) and the spectral weighting of
// WalshHadamardCS (:253-320) are this, with the kept-pixel mask / the permuted measurement mask.
__global__ __launch_bounds__(256) void mask_mix_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                       const float* __restrict__ mask, int planes_mask,
                                                       int64_t plane_elems, float* __restrict__ out, int64_t total,
                                                       float cx_m, float cx_n, float cy_m, float cy_n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        bool m = true;
        if (mask) {
            const int64_t plane = i / plane_elems, p = i - plane * plane_elems;
            m = mask[(plane % planes_mask) * plane_elems + p] != 0.f;
        }
        float v = x[i] * (m ? cx_m : cx_n);
        if (y) v = v + y[i] * (m ? cy_m : cy_n);
        out[i] = v;
    }
}

extern "C" int ddnm_mask_mix_f32(const float* x, const float* y, const float* mask, int32_t planes_mask,
                                 int64_t plane_elems, float* out, int64_t total, float cx_m, float cx_n, float cy_m,
                                 float cy_n, void* stream) {
    if (!x || !out || total <= 0 || plane_elems <= 0 || (mask && planes_mask <= 0)) return DDNM_E_BADARG;
    DDNM_LAUNCH(mask_mix_kernel, GRID_1D(total), dim3(256), 0, (hipStream_t)stream, x, y, mask, planes_mask,
                plane_elems, out, total, cx_m, cx_n, cy_m, cy_n);
    return 0;
}

// Per-site spectral operations with the small orthogonal V of a 1 x n measurement row (n = r*r for
// SuperResolution patches, n = 3 for Colorization needles); spectral index 0 is the measured direction.
//   op 0 (Lambda,        :535-571, :669-695): out = x + (lam_m - 1) * V[:,0] * (V[:,0] . x)
//   op 1 (Lambda_noise,  :573-623, :697-736): out = V (d1 .* x~ + d2 .* y~),  x~/y~ = RAW site entries
// mode 0: site = r x r spatial patch of one channel plane [BC][H][W]; mode 1: site = the 3 channels of a pixel.
__global__ __launch_bounds__(256) void site_spectral_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                            const float* __restrict__ V, int n, int mode, int r,
                                                            int H, int W, int64_t HW, float* __restrict__ out,
                                                            int64_t total, int op, float c0, float c1, float c2,
                                                            float c3) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        // element e -> (site base offset, index i inside the site, stride pattern)
        int64_t base;
        int i;
        if (mode == 0) {
            const int64_t plane = e / HW, p = e - plane * HW;
            const int yy = (int)(p / W), xx = (int)(p - (int64_t)yy * W);
            base = plane * HW + (int64_t)(yy / r * r) * W + (xx / r * r);
            i = (yy % r) * r + (xx % r);
        } else {
            const int64_t b = e / (3 * HW), q = e - b * 3 * HW;
            i = (int)(q / HW);
            base = b * 3 * HW + (q - (int64_t)i * HW);
        }
        auto at = [&](int k) -> int64_t { return mode == 0 ? base + (int64_t)(k / r) * W + (k % r) : base + (int64_t)k * HW; };
        float acc = 0.f;
        if (op == 0) {
            float dot = 0.f;
            for (int k = 0; k < n; ++k) dot += V[k * n] * x[at(k)];
            acc = x[e] + (c0 - 1.0f) * V[i * n] * dot;
        } else {
            for (int k = 0; k < n; ++k) {
                float z = x[at(k)] * (k == 0 ? c0 : c1);
                if (y) z += y[at(k)] * (k == 0 ? c2 : c3);
                acc += V[i * n + k] * z;
            }
        }
        out[e] = acc;
    }
}

extern "C" int ddnm_site_spectral_f32(const float* x, const float* y, const float* V, int32_t n, int32_t mode,
                                      int32_t r, int32_t B, int32_t C, int32_t H, int32_t W, float* out, int32_t op,
                                      float c0, float c1, float c2, float c3, void* stream) {
    if (!x || !V || !out || n <= 0 || B <= 0 || C <= 0 || H <= 0 || W <= 0) return DDNM_E_BADARG;
    if (mode == 0 && (r <= 0 || n != r * r || H % r || W % r)) return DDNM_E_SHAPE;
    if (mode == 1 && (n != 3 || C != 3)) return DDNM_E_SHAPE;
    if (mode != 0 && mode != 1) return DDNM_E_BADARG;
    const int64_t total = (int64_t)B * C * H * W;
    DDNM_LAUNCH(site_spectral_kernel, GRID_1D(total), dim3(256), 0, (hipStream_t)stream, x, y, V, n, mode, r, H, W,
                (int64_t)H * W, out, total, op, c0, c1, c2, c3);
    return 0;
}

// out = x .* table[(plane % planes_table)][p]  -- per-(channel, spectral index) gains of the separable blur
// operators (functions/svd_operators.py:934-1165: singular values applied between the V^T . V and U . U^T products)
__global__ __launch_bounds__(256) void mul_planes_kernel(const float* __restrict__ x, const float* __restrict__ table,
                                                         int planes_table, int64_t plane_elems,
                                                         float* __restrict__ out, int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t plane = i / plane_elems, p = i - plane * plane_elems;
        out[i] = x[i] * table[(plane % planes_table) * plane_elems + p];
    }
}

extern "C" int ddnm_mul_planes_f32(const float* x, const float* table, int32_t planes_table, int64_t plane_elems,
                                   float* out, int64_t total, void* stream) {
    if (!x || !table || !out || planes_table <= 0 || plane_elems <= 0 || total <= 0) return DDNM_E_BADARG;
    DDNM_LAUNCH(mul_planes_kernel, GRID_1D(total), dim3(256), 0, (hipStream_t)stream, x, table, planes_table,
                plane_elems, out, total);
    return 0;
}

// ---- generic pieces of the matrix-free SVD surface (A_functions.V / Vt / U / Ut / add_zeros / At / A_pinv_eta,
// functions/svd_operators.py:9-97): a row gather with optional per-entry scale, and a small per-site matrix product.
// out[b][i] = (idx[i] >= 0 ? in[b][idx[i]] : 0) * (scale ? scale[i] : 1);  idx NULL = identity for i < n_in, 0 beyond
// (that is `add_zeros`, and with `scale` the `singulars * temp[:, :n]` products of A / At / A_pinv_eta).
__global__ __launch_bounds__(256) void gather_scale_kernel(const float* __restrict__ in, const int32_t* __restrict__ idx,
                                                           const float* __restrict__ scale, float* __restrict__ out,
                                                           int64_t n_in, int64_t n_out, int64_t total) {
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int64_t b = t / n_out, i = t - b * n_out;
        const int64_t j = idx ? (int64_t)idx[i] : (i < n_in ? i : -1);
        float v = j >= 0 ? in[b * n_in + j] : 0.f;
        if (scale) v *= scale[i];
        out[t] = v;
    }
}

extern "C" int ddnm_gather_scale_f32(const float* in, const int32_t* idx, const float* scale, float* out, int32_t B,
                                     int64_t n_in, int64_t n_out, void* stream) {
    if (!in || !out || B <= 0 || n_in <= 0 || n_out <= 0) return DDNM_E_BADARG;
    const int64_t total = (int64_t)B * n_out;
    DDNM_LAUNCH(gather_scale_kernel, GRID_1D(total), dim3(256), 0, (hipStream_t)stream, in, idx, scale, out, n_in, n_out,
                total);
    return 0;
}

// out[b][s][i] = sum_j Mop[i][j] in[b][s][j], Mop = M or M^T (n x n row-major, n <= 16), element (b, s, j) at
// in[b*sb + s*ss + j*sj] (same strides for out): r x r patches in site-major order (ss = n, sj = 1) or RGB needles of
// CHW planes (ss = 1, sj = H*W) -- the V_small / Vt_small products of svd_operators.py:490-517,636-656.
__global__ __launch_bounds__(256) void site_matmul_kernel(const float* __restrict__ in, const float* __restrict__ M,
                                                          float* __restrict__ out, int64_t sites_total, int64_t sites, int n,
                                                          int64_t sb, int64_t ss, int64_t sj, int trans) {
    __shared__ float Ms[16 * 16];
    for (int i = threadIdx.x; i < n * n; i += 256) Ms[i] = M[i];
    __syncthreads();
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < sites_total; t += (int64_t)gridDim.x * 256) {
        const int64_t b = t / sites, sidx = t - b * sites;
        const int64_t base = b * sb + sidx * ss;
        float v[16];
        for (int j = 0; j < n; ++j) v[j] = in[base + j * sj];
        for (int i = 0; i < n; ++i) {
            float a = 0.f;
            for (int j = 0; j < n; ++j) a += (trans ? Ms[j * n + i] : Ms[i * n + j]) * v[j];
            out[base + i * sj] = a;
        }
    }
}

extern "C" int ddnm_site_matmul_f32(const float* in, const float* M, float* out, int32_t B, int64_t sites, int32_t n,
                                    int64_t sb, int64_t ss, int64_t sj, int32_t trans, void* stream) {
    if (!in || !M || !out || B <= 0 || sites <= 0 || n <= 0 || n > 16 || in == out) return DDNM_E_BADARG;
    const int64_t total = (int64_t)B * sites;
    DDNM_LAUNCH(site_matmul_kernel, GRID_1D(total), dim3(256), 0, (hipStream_t)stream, in, M, out, total, sites, n, sb, ss,
                sj, trans);
    return 0;
}

// DDNM+ spectral weights of Deblurring (svd_operators.py:1016-1091), evaluated per spectral entry from the
// UNSORTED, un-thresholded singular table s[p] = s1_i * s1_j (the reference's sort :962 and its inverse cancel):
//   mode 0 (Lambda :1016-1040):        out = x * lambda(s[p])
//   mode 1 (Lambda_noise :1042-1091):  out = x * d1(s[p]) + y * d2(s[p])
// with inv = 1/s (0 if s == 0), thr = a*sigma_y*inv:
//   sigma_t < thr: lambda = s*sigma_t*sqrt(1-eta^2)/a/sigma_y, d = (sigma_t*eta, 0)
//   sigma_t > thr: lambda = 1, d = (sqrt(sigma_t^2 - a^2 sigma_y^2 inv^2), 0)
//   s == 0 (and a tie): lambda = 1, d = (sigma_t*eta, sigma_t*sqrt(1-eta^2));  a == 0 or sigma_y == 0: no regime change

// (lambda, d1, d2) of one spectral entry with singular value s: the rule above, shared by spectral_mix_kernel and
// step_plus_spectral_kernel (eta_c = sqrt(1 - eta^2), active = a != 0 && sigma_y != 0)
struct SpectralCoef { float lam, d1, d2; };
__device__ __forceinline__ SpectralCoef spectral_coef(float s, bool active, float a, float sy, float st, float eta,
                                                      float eta_c) {
    const float inv = s == 0.f ? 0.f : 1.f / s;
    float lam = 1.f, d1 = st * eta, d2 = st * eta_c;
    if (active) {
        const float thr = a * sy * inv;
        if (st < thr) { lam = s * st * eta_c / a / sy; d2 = 0.f; }
        if (st > thr) { d1 = sqrtf(st * st - a * a * (sy * sy) * (inv * inv)); d2 = 0.f; }
        if (s == 0.f) { d1 = st * eta; d2 = st * eta_c; }
    }
    return SpectralCoef{lam, d1, d2};
}

__global__ __launch_bounds__(256) void spectral_mix_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                           const float* __restrict__ stab, int64_t plane_elems,
                                                           float* __restrict__ out, int64_t total, float a, float sy,
                                                           float st, float eta, float eta_c, int mode) {
    const bool active = a != 0.f && sy != 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const SpectralCoef c = spectral_coef(stab[i % plane_elems], active, a, sy, st, eta, eta_c);
        out[i] = mode == 0 ? x[i] * c.lam : x[i] * c.d1 + y[i] * c.d2;
    }
}

extern "C" int ddnm_spectral_mix_f32(const float* x, const float* y, const float* singulars, int64_t plane_elems,
                                     float* out, int64_t total, float a, float sigma_y, float sigma_t, float eta,
                                     int32_t mode, void* stream) {
    if (!x || !singulars || !out || plane_elems <= 0 || total <= 0 || (mode != 0 && mode != 1)) return DDNM_E_BADARG;
    if (mode == 1 && !y) return DDNM_E_BADARG;
    const float eta_c = (float)sqrt(1.0 - (double)eta * (double)eta);
    DDNM_LAUNCH(spectral_mix_kernel, GRID_1D(total), dim3(256), 0, (hipStream_t)stream, x, y, singulars, plane_elems, out,
                total, a, sigma_y, sigma_t, eta, eta_c, mode);
    return 0;
}

// ---------------------------------------------------------------- fused DDNM+ step in the spectral planes
// One DDNM+ reverse step (functions/svd_ddnm.py:118-131) of an operator with a separable SVD, A = Ul diag(g) Vl^T (.) Vr Ur^T
// per plane (SRConv, Deblurring2D), collapsed in the planes x^ = Vl^T X Vr.  With x^_t, e^ the transformed x_t and eps,
// y^ = g^+ .* (Ul^T Y Ur) (zero where g = 0), a = sqrt_at_next and n ~ N(0, I):
//   x^_0 = (x^_t - e^ * sqrt(1 - abar_t)) / sqrt(abar_t)
//   z^   = a * (x^_0 - mu .* (x^_0 - y^)) + d1 .* n + d2 .* e^            X_{t-1} = Vl z^ Vr^T
// (lambda, d1, d2) = spectral_coef(g) per entry of the THRESHOLDED gain table; mu = lambda where g > 0, else 0 (null
// space: no correction, (d1, d2) = (sigma_t eta, sigma_t sqrt(1 - eta^2))).  Unlike Lambda_noise of the reference's other
// operators, eps enters as V^T eps; n is drawn directly in the spectral planes (V orthogonal: same distribution).
// [B][C][plane] in one pass, float4 per lane: 3 reads + the cached table (gains + c * gains_cstride; stride 0 = one
// table for all channels), 1 write.  out_hat may alias xt_hat: every lane reads its four entries before it stores them.
template <class NZ>
__global__ __launch_bounds__(256) void step_plus_spectral_kernel(const float* xt_hat, const float* __restrict__ et_hat,
                                                                 const float* __restrict__ y_hat,
                                                                 const float* __restrict__ gains, int64_t gains_cstride,
                                                                 NZ noise, float* out_hat, int64_t plane4, int64_t chw4,
                                                                 int64_t total4, ddnm_step_scalars s, float sy, float st,
                                                                 float eta, float eta_c) {
    const float a = s.sqrt_at_next;
    const bool active = a != 0.f && sy != 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / chw4, r = i - b * chw4;
        const int64_t c = r / plane4, p = r - c * plane4;
        const auto nz = bind(noise, b);
        const f32x4 e = ld4(et_hat + i * 4);
        const f32x4 x0 = x0_of(ld4(xt_hat + i * 4), e, s);
        const f32x4 yh = ld4(y_hat + i * 4);
        const f32x4 g = ld4(gains + c * gains_cstride + p * 4);
        const f32x4 n = nz4(nz, i * 4);
        f32x4 mu, d1, d2;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const SpectralCoef k = spectral_coef(g[j], active, a, sy, st, eta, eta_c);
            mu[j] = g[j] > 0.f ? k.lam : 0.f;
            d1[j] = k.d1;
            d2[j] = k.d2;
        }
        st4(out_hat + i * 4, ((x0 - (x0 - yh) * mu) * a + n * d1) + e * d2);
    }
}

static inline int plus_spectral_args(const float* xt_hat, const float* et_hat, const float* y_hat, const float* gains,
                                     int64_t gains_cstride, const float* out_hat, int32_t B, int32_t C, int64_t plane,
                                     const ddnm_step_scalars* s) {
    if (!xt_hat || !et_hat || !y_hat || !gains || !out_hat || !s || B <= 0 || C <= 0 || plane <= 0 || gains_cstride < 0)
        return DDNM_E_BADARG;
    if ((plane & 3) || (gains_cstride & 3)) return DDNM_E_SHAPE;
    return 0;
}

template <class Src>      // after plus_spectral_args and the source check of the entry point
static int launch_plus_spectral(const float* xt_hat, const float* et_hat, const float* y_hat, const float* gains, int64_t gains_cstride,
                                Src src, float* out_hat, int32_t B, int64_t chw, int64_t plane, float sigma_y, float sigma_t, float eta,
                                const ddnm_step_scalars* s, void* stream) {
    const int64_t total4 = (int64_t)B * chw / 4;
    const float eta_c = (float)sqrt(1.0 - (double)eta * (double)eta);
    DDNM_LAUNCH(step_plus_spectral_kernel<Src>, GRID_1D(total4), dim3(256), 0, (hipStream_t)stream, xt_hat, et_hat, y_hat, gains,
                gains_cstride, src, out_hat, plane / 4, chw / 4, total4, *s, sigma_y, sigma_t, eta, eta_c);
    return 0;
}

extern "C" int ddnm_step_plus_spectral_f32(const float* xt_hat, const float* et_hat, const float* y_hat,
                                           const float* gains, int64_t gains_cstride, const float* noise, float* out_hat,
                                           int32_t B, int32_t C, int64_t plane, float sigma_y, float sigma_t, float eta,
                                           const ddnm_step_scalars* s, void* stream) {
    if (int e = plus_spectral_args(xt_hat, et_hat, y_hat, gains, gains_cstride, out_hat, B, C, plane, s)) return e;
    if (!noise_ok(noise, s)) return DDNM_E_BADARG;
    const int64_t chw = (int64_t)C * plane;
    return launch_plus_spectral(xt_hat, et_hat, y_hat, gains, gains_cstride, noise_src(noise, s, chw), out_hat, B, chw, plane, sigma_y,
                                sigma_t, eta, s, stream);
}

extern "C" int ddnm_step_plus_spectral_keyed_f32(const float* xt_hat, const float* et_hat, const float* y_hat,
                                                 const float* gains, int64_t gains_cstride, const uint32_t* keys,
                                                 float* out_hat, int32_t B, int32_t C, int64_t plane, float sigma_y,
                                                 float sigma_t, float eta, const ddnm_step_scalars* s, void* stream) {
    if (int e = plus_spectral_args(xt_hat, et_hat, y_hat, gains, gains_cstride, out_hat, B, C, plane, s)) return e;
    if (!keys_ok(keys)) return DDNM_E_BADARG;
    const int64_t chw = (int64_t)C * plane;
    return launch_plus_spectral(xt_hat, et_hat, y_hat, gains, gains_cstride, keyed_src(keys, s, chw), out_hat, B, chw, plane, sigma_y,
                                sigma_t, eta, s, stream);
}

// out[b][i] = a * x[b*x_bstride + i] + b * y[b*chw + i]: eps <- eps[:, :3] - sqrt(1-abar) * grad  (svd_ddnm.py:51-52)
__global__ __launch_bounds__(256) void axpby_strided_kernel(const float* __restrict__ x, int64_t x_bstride,
                                                            const float* __restrict__ y, float* __restrict__ out,
                                                            int64_t chw, int64_t total, float a, float b) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t bi = i / chw, r = i - bi * chw;
        out[i] = x[bi * x_bstride + r] * a + y[i] * b;
    }
}

extern "C" int ddnm_axpby_strided_f32(const float* x, int64_t x_bstride, const float* y, float* out, int32_t B,
                                      int64_t chw, float a, float b, void* stream) {
    if (!x || !y || !out || B <= 0 || chw <= 0) return DDNM_E_BADARG;
    const int64_t total = (int64_t)B * chw;
    DDNM_LAUNCH(axpby_strided_kernel, GRID_1D(total), dim3(256), 0, (hipStream_t)stream, x, x_bstride, y, out, chw,
                total, a, b);
    return 0;
}


// Block-based CS (svd_operators.py:101-159): ps x ps patches of every plane as rows of a [patches][ps*ps] matrix
// (unfold(2,ps,ps).unfold(3,ps,ps), :134-135) so that Vt_small / V_small act as ONE MFMA GEMM over all patches.
// float4 along the patch row (ps % 4 == 0): both sides move 16-byte pieces; HBM-bound, 8 B per element.
__global__ __launch_bounds__(256) void patchify_kernel(const float* __restrict__ src, float* __restrict__ dst, int D,
                                                       int ps, int inverse, int64_t total4) {
    const int ps4 = ps >> 2, npd = D / ps;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        // i indexes the patch-matrix side: (((plane*npd + py)*npd + px)*ps + r)*ps4 + q
        int64_t t = i;
        const int q = (int)(t % ps4); t /= ps4;
        const int r = (int)(t % ps); t /= ps;
        const int px = (int)(t % npd); t /= npd;
        const int py = (int)(t % npd);
        const int64_t plane = t / npd;
        const int64_t img = ((plane * D + py * ps + r) * D + px * ps) / 4 + q;
        if (inverse) reinterpret_cast<f32x4*>(dst)[img] = reinterpret_cast<const f32x4*>(src)[i];
        else reinterpret_cast<f32x4*>(dst)[i] = reinterpret_cast<const f32x4*>(src)[img];
    }
}

extern "C" int ddnm_patchify_f32(const float* src, float* dst, int32_t planes, int32_t D, int32_t ps, int32_t inverse,
                                 void* stream) {
    if (!src || !dst || planes <= 0 || D <= 0 || ps <= 0) return DDNM_E_BADARG;
    if (D % ps || ps % 4) return DDNM_E_SHAPE;
    const int64_t total4 = (int64_t)planes * D * D / 4;
    DDNM_LAUNCH(patchify_kernel, GRID_1D(total4), dim3(256), 0, (hipStream_t)stream, src, dst, D, ps, inverse, total4);
    return 0;
}

// ---------------------------------------------------------------- fused DDNM+ step of block-based CS, per patch
// One DDNM+ reverse step (functions/svd_ddnm.py:118-131) of CS (svd_operators.py:101-159).  Every singular value is 1
// (:110), so the spectral coefficients take two values per step -- (lambda, d1r, d2r) on the measured subspace, (1, d1n,
// d2n) on the null space -- and with M = Vt_small[:cs] (orthonormal rows, M^T M the projector onto the measured subspace
// of a patch), a = sqrt_at_next and n ~ N(0, I) drawn in the image domain the step is
//   x0      = (x_t - eps * sqrt_1m_at) / sqrt_at
//   w       = -a lambda x0 + (d1r - d1n) n + (d2r - d2n) eps                    patch layout [patches][ps*ps]
//   x_{t-1} = a x0 + d1n n + d2n eps + a lambda A^+ y + unpatch((w M^T) M)
// = a (x0 - Lambda A^+ (A x0 - y)) + V (d1 .* V^T n + d2 .* V^T eps) without the full V_small.  The pre kernel writes x0,
// the image-order part of x_{t-1} and w; two ddnm_bgemm_f32 launches (the products of CS.A / CS.A_pinv) project w; the
// post kernel adds the projection.  The five coefficients come from the host (svd_operators.cs_plus_coefficients):
// CsPlusCoef, defined above with the mosaic step that shares it.

// one float4 per lane in image order [B][C][D][D]: 3 reads (+ the noise tensor), 3 writes; four consecutive pixels of a
// row stay inside one patch row (ps % 4 == 0), so the store into w is one 16-byte piece at patchify_kernel's position
template <class NZ>
__global__ __launch_bounds__(256) void cs_plus_pre_kernel(const float* __restrict__ xt, const float* __restrict__ et,
                                                          int64_t et_bstride, NZ noise, const float* __restrict__ aty,
                                                          float* __restrict__ x0o, float* __restrict__ xn,
                                                          float* __restrict__ w, int C, int D, int ps, int64_t chw4,
                                                          int64_t total4, ddnm_step_scalars s, CsPlusCoef k) {
    const int npd = D / ps, D4 = D >> 2;
    const float a = s.sqrt_at_next;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / chw4, r = i - b * chw4;
        const auto nz = bind(noise, b);
        const f32x4 e = ld4(et + b * et_bstride + r * 4);
        const f32x4 x0 = x0_of(ld4(xt + i * 4), e, s);
        const f32x4 ay = ld4(aty + i * 4);
        const f32x4 n = nz4(nz, i * 4);
        st4(x0o + i * 4, x0);
        st4(xn + i * 4, ((x0 * a + n * k.d1n) + e * k.d2n) + ay * k.al);
        // r = (c*D + yy)*D4 + x4 inside the image -> row (plane, py, px), column rr*ps + xx%ps of the patch matrix
        int64_t t = r;
        const int x4 = (int)(t % D4); t /= D4;
        const int yy = (int)(t % D);
        const int64_t plane = b * C + t / D;
        const int xx = x4 * 4, py = yy / ps, px = xx / ps;
        const int64_t pos = ((((plane * npd + py) * npd + px) * ps + (yy - py * ps)) * ps) + (xx - px * ps);
        st4(w + pos, (n * k.dd1 + e * k.dd2) - x0 * k.al);
    }
}

static inline int plus_cs_pre_args(const float* xt, const float* et, int64_t et_bstride, const float* aty,
                                   const float* x0_out, const float* xt_next, const float* w, int32_t B, int32_t C,
                                   int32_t D, int32_t ps, const ddnm_step_scalars* s) {
    if (!xt || !et || !aty || !x0_out || !xt_next || !w || !s || B <= 0 || C <= 0 || D <= 0 || ps <= 0)
        return DDNM_E_BADARG;
    if (D % ps || ps % 4 || (et_bstride & 3)) return DDNM_E_SHAPE;
    if (xt_next == xt || xt_next == et || xt_next == x0_out || w == xt || w == et || w == aty || w == x0_out ||
        w == xt_next || x0_out == xt || x0_out == et || x0_out == aty || xt_next == aty)
        return DDNM_E_BADARG;
    return 0;
}

template <class Src>      // after plus_cs_pre_args and the source check of the entry point
static int launch_plus_cs_pre(const float* xt, const float* et, int64_t et_bstride, Src src, const float* aty, float* x0_out,
                              float* xt_next, float* w, int32_t B, int32_t C, int32_t D, int32_t ps, int64_t chw, CsPlusCoef k,
                              const ddnm_step_scalars* s, void* stream) {
    const int64_t total4 = (int64_t)B * chw / 4;
    DDNM_LAUNCH(cs_plus_pre_kernel<Src>, GRID_1D(total4), dim3(256), 0, (hipStream_t)stream, xt, et, et_bstride, src, aty, x0_out,
                xt_next, w, C, D, ps, chw / 4, total4, *s, k);
    return 0;
}

extern "C" int ddnm_step_plus_cs_pre_f32(const float* xt, const float* et, int64_t et_bstride, const float* noise,
                                         const float* aty, float* x0_out, float* xt_next, float* w, int32_t B, int32_t C,
                                         int32_t D, int32_t ps, float a_lambda, float d1n, float d2n, float dd1,
                                         float dd2, const ddnm_step_scalars* s, void* stream) {
    if (int e = plus_cs_pre_args(xt, et, et_bstride, aty, x0_out, xt_next, w, B, C, D, ps, s)) return e;
    if (!noise_ok(noise, s)) return DDNM_E_BADARG;
    const int64_t chw = (int64_t)C * D * D;
    return launch_plus_cs_pre(xt, et, et_bstride, noise_src(noise, s, chw), aty, x0_out, xt_next, w, B, C, D, ps, chw,
                              CsPlusCoef{a_lambda, d1n, d2n, dd1, dd2}, s, stream);
}

extern "C" int ddnm_step_plus_cs_pre_keyed_f32(const float* xt, const float* et, int64_t et_bstride, const uint32_t* keys,
                                               const float* aty, float* x0_out, float* xt_next, float* w, int32_t B,
                                               int32_t C, int32_t D, int32_t ps, float a_lambda, float d1n, float d2n,
                                               float dd1, float dd2, const ddnm_step_scalars* s, void* stream) {
    if (int e = plus_cs_pre_args(xt, et, et_bstride, aty, x0_out, xt_next, w, B, C, D, ps, s)) return e;
    if (!keys_ok(keys)) return DDNM_E_BADARG;
    const int64_t chw = (int64_t)C * D * D;
    return launch_plus_cs_pre(xt, et, et_bstride, keyed_src(keys, s, chw), aty, x0_out, xt_next, w, B, C, D, ps, chw,
                              CsPlusCoef{a_lambda, d1n, d2n, dd1, dd2}, s, stream);
}

// xt_next[img] += P[patch index]: the inverse gather of patchify_kernel with an add (2 reads, 1 write per element)
__global__ __launch_bounds__(256) void cs_plus_post_kernel(const float* __restrict__ P, float* __restrict__ xn, int D,
                                                           int ps, int64_t total4) {
    const int ps4 = ps >> 2, npd = D / ps;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        int64_t t = i;                               // patch-matrix side, as in patchify_kernel
        const int q = (int)(t % ps4); t /= ps4;
        const int r = (int)(t % ps); t /= ps;
        const int px = (int)(t % npd); t /= npd;
        const int py = (int)(t % npd);
        const int64_t plane = t / npd;
        const int64_t img = ((plane * D + py * ps + r) * D + px * ps) + q * 4;
        st4(xn + img, ld4(xn + img) + ld4(P + i * 4));
    }
}

extern "C" int ddnm_step_plus_cs_post_f32(const float* P, float* xt_next, int32_t planes, int32_t D, int32_t ps,
                                          void* stream) {
    if (!P || !xt_next || P == xt_next || planes <= 0 || D <= 0 || ps <= 0) return DDNM_E_BADARG;
    if (D % ps || ps % 4) return DDNM_E_SHAPE;
    const int64_t total4 = (int64_t)planes * D * D / 4;
    DDNM_LAUNCH(cs_plus_post_kernel, GRID_1D(total4), dim3(256), 0, (hipStream_t)stream, P, xt_next, D, ps, total4);
    return 0;
}

// ---------------------------------------------------------------- fused: old photo (mask, grey, average pool)
// A = pool_r . grey_w . mask (the Composition of the simplified path's mask_color_sr, guided_diffusion/diffusion.py:260-290)
// with its exact pseudo-inverse.  Site j is an r x r block of the image, k_j the number of its kept pixels (m_p = 1):
//   y_j = sum_c sum_{p in j} w_c m_p x[c][p] / r^2
// The rows of A have disjoint supports, so A A^T is diagonal, U = I and row j = s_j q_j with
//   s_j = sqrt(k_j) |w| / r^2,   q_j[c][p] = w_c m_p / (sqrt(k_j) |w|),   (A^+ y)[c][p] = m_p w_c r^2 y_j / (k_j |w|^2)
// (k_j = 0: the site is null space, y_j is ignored).  With the unnormalised site sums S(v) = sum_c sum_p w_c m_p v[c][p],
// q_j (q_j . v) = m_p (w_c / |w|^2) S(v) / k_j: no square root but the one of s_j, which only spectral_coef sees.
//   DDNM  (svd_ddnm.py:57-65):   x0h = x0 - lambda m_p (w_c / |w|^2) (S(x0) - r^2 y_j) / k_j,  x_{t-1} = update_of(x0h, n, eps)
//   DDNM+ (svd_ddnm.py:118-131), a = sqrt_at_next, (lambda_j, d1_j, d2_j) = spectral_coef(s_j), (1, d1n, d2n) = spectral_coef(0):
//     x_{t-1} = a x0 + d1n n + d2n eps
//               + m_p (w_c / |w|^2) [ -a lambda_j (S(x0) - r^2 y_j) + (d1_j - d1n) S(n) + (d2_j - d2n) S(eps) ] / k_j
// eps enters as V^T eps and n is drawn in image space, as in step_plus_spectral_kernel.  Singular values differ inside one
// launch: the coefficients are evaluated per site in the kernel, from the mask alone (no per-site table).
// Mapping: one lane owns a strip of r rows x 4 pixels x 3 planes; it holds 4 / r whole sites for r = 1, 2, one for r = 4
// and half a site for r = 8, where lanes 2i and 2i + 1 of the wave add their partial sums with one __shfl_xor (a + b is
// the same number on both lanes, and a strip's sums do not depend on where its image stands in a batch).  Two passes per
// strip: the site sums first, then xt, eps and the mask are read again (from L2) and the noise is drawn again from its
// offset, so nothing of a strip stays in registers between them.  THE OUTPUTS MUST NOT ALIAS xt OR eps.
// mask: a device plane [H*W] of 0 / 1 shared by all images, NULL = everything kept (sr_color: no mask is loaded).
struct McsrW { float w[3], wp[3], wn; };   // w, w / |w|^2, |w|

// DDNM_E_BADARG for weights that are all zero
static int mcsr_weights(const float* w3_host, McsrW* out) {
    McsrW c;
    for (int i = 0; i < 3; ++i) c.w[i] = w3_host[i];
    const float n2 = (c.w[0] * c.w[0] + c.w[1] * c.w[1]) + c.w[2] * c.w[2];
    if (!(n2 > 0.f)) return DDNM_E_BADARG;
    for (int i = 0; i < 3; ++i) c.wp[i] = c.w[i] / n2;
    c.wn = sqrtf(n2);
    *out = c;
    return 0;
}

// sizes of every mcsr entry point, after its pointer checks (DDNM_E_BADARG before DDNM_E_SHAPE)
static int mcsr_shape(int32_t H, int32_t W, int32_t r, int64_t et_bstride) {
    if (r != 1 && r != 2 && r != 4 && r != 8) return DDNM_E_SHAPE;
    if (H <= 0 || W <= 0 || H % r || W % r || (W & 3) || (et_bstride & 3)) return DDNM_E_SHAPE;
    return 0;
}

// a strip of R rows x 4 pixels: its sites (NS of them) and the geometry shared by the four kernels
template <int R>
struct McsrStrip {
    static constexpr int NS = R >= 4 ? 1 : 4 / R;                         // whole sites of a strip (R = 8: half of one)
    static __device__ __forceinline__ int site(int j) { return R >= 4 ? 0 : j / R; }   // site of column j of the strip
    int64_t b, pix, ysite;   // image, offset of the strip's first row inside a plane, index of its first site in y
    __device__ __forceinline__ McsrStrip(int64_t i, int H, int W) {
        const int W4 = W >> 2;
        const int64_t per_img = (int64_t)(H / R) * W4;
        b = i / per_img;
        const int64_t q = i - b * per_img;
        const int sy = (int)(q / W4), xg = (int)(q - (int64_t)sy * W4);
        pix = (int64_t)sy * R * W + xg * 4;
        ysite = (b * (H / R) + sy) * (W / R) + (R >= 4 ? xg * 4 / R : xg * NS);
    }
};

// the other half of a site's sum (R = 8: the neighbouring lane's strip); the strips of a site are i and i ^ 1 and their
// number is even, so both lanes are in the loop together
template <int R>
__device__ __forceinline__ float mcsr_site_sum(float v) { return R == 8 ? v + __shfl_xor(v, 1) : v; }

__device__ __forceinline__ f32x4 mcsr_mask4(const float* mask, int64_t off) {
    return mask ? ld4(mask + off) : f32x4{1.f, 1.f, 1.f, 1.f};
}

// y = A x
template <int R>
__global__ __launch_bounds__(256) void mcsr_A_kernel(const float* __restrict__ x, const float* __restrict__ mask,
                                                     float* __restrict__ y, int H, int W, int64_t total, McsrW cw) {
    using S = McsrStrip<R>;
    const int64_t hw = (int64_t)H * W;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const S t(i, H, W);
        const float* xb = x + t.b * 3 * hw + t.pix;
        float sx[S::NS] = {};
#pragma unroll
        for (int row = 0; row < R; ++row) {
            const int64_t o = (int64_t)row * W;
            const f32x4 g = ((ld4(xb + o) * cw.w[0] + ld4(xb + hw + o) * cw.w[1]) + ld4(xb + 2 * hw + o) * cw.w[2]) *
                            mcsr_mask4(mask, t.pix + o);
#pragma unroll
            for (int j = 0; j < 4; ++j) sx[S::site(j)] += g[j];
        }
#pragma unroll
        for (int k = 0; k < S::NS; ++k) {
            const float v = mcsr_site_sum<R>(sx[k]) / (float)(R * R);
            if (R < 8 || !(i & 1)) y[t.ysite + k] = v;
        }
    }
}

// x = A^+ y
template <int R>
__global__ __launch_bounds__(256) void mcsr_pinv_kernel(const float* __restrict__ y, const float* __restrict__ mask,
                                                        float* __restrict__ x, int H, int W, int64_t total, McsrW cw) {
    using S = McsrStrip<R>;
    const int64_t hw = (int64_t)H * W;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const S t(i, H, W);
        float kept[S::NS] = {};
#pragma unroll
        for (int row = 0; row < R; ++row) {
            const f32x4 m = mcsr_mask4(mask, t.pix + (int64_t)row * W);
#pragma unroll
            for (int j = 0; j < 4; ++j) kept[S::site(j)] += m[j];
        }
        float g[S::NS];
#pragma unroll
        for (int k = 0; k < S::NS; ++k) {
            const float kj = mcsr_site_sum<R>(kept[k]);
            g[k] = kj > 0.f ? y[t.ysite + k] * (float)(R * R) / kj : 0.f;
        }
        f32x4 gv;
#pragma unroll
        for (int j = 0; j < 4; ++j) gv[j] = g[S::site(j)];
        float* xb = x + t.b * 3 * hw + t.pix;
#pragma unroll
        for (int row = 0; row < R; ++row) {
            const int64_t o = (int64_t)row * W;
            const f32x4 mg = mcsr_mask4(mask, t.pix + o) * gv;
#pragma unroll
            for (int c = 0; c < 3; ++c) st4(xb + c * hw + o, mg * cw.wp[c]);
        }
    }
}

template <int R, class NZ>
__global__ __launch_bounds__(256) void step_mcsr_kernel(const float* __restrict__ xt, const float* __restrict__ et,
                                                        int64_t et_bstride, NZ noise, const float* __restrict__ y,
                                                        const float* __restrict__ mask, float* __restrict__ x0o,
                                                        float* __restrict__ xn, int H, int W, int64_t total,
                                                        ddnm_step_scalars s, McsrW cw) {
    using S = McsrStrip<R>;
    const int64_t hw = (int64_t)H * W;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const S t(i, H, W);
        const auto nz = bind(noise, t.b);
        const int64_t base = t.b * 3 * hw + t.pix, ebase = t.b * et_bstride + t.pix;
        float kept[S::NS] = {}, sx[S::NS] = {};
#pragma unroll 1
        for (int row = 0; row < R; ++row) {
            const int64_t o = (int64_t)row * W;
            const f32x4 m = mcsr_mask4(mask, t.pix + o);
            f32x4 x0[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) x0[c] = x0_of(ld4(xt + base + c * hw + o), ld4(et + ebase + c * hw + o), s);
            const f32x4 g = ((x0[0] * cw.w[0] + x0[1] * cw.w[1]) + x0[2] * cw.w[2]) * m;
#pragma unroll
            for (int j = 0; j < 4; ++j) { kept[S::site(j)] += m[j]; sx[S::site(j)] += g[j]; }
        }
        float g[S::NS];
#pragma unroll
        for (int k = 0; k < S::NS; ++k) {
            const float kj = mcsr_site_sum<R>(kept[k]), sxj = mcsr_site_sum<R>(sx[k]);
            g[k] = kj > 0.f ? (sxj - y[t.ysite + k] * (float)(R * R)) / kj * s.lambda : 0.f;
        }
        f32x4 gv;
#pragma unroll
        for (int j = 0; j < 4; ++j) gv[j] = g[S::site(j)];
#pragma unroll 1
        for (int row = 0; row < R; ++row) {
            const int64_t o = (int64_t)row * W;
            const f32x4 mg = mcsr_mask4(mask, t.pix + o) * gv;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const f32x4 e = ld4(et + ebase + c * hw + o);
                const f32x4 x0 = x0_of(ld4(xt + base + c * hw + o), e, s);
                if (x0o) st4(x0o + base + c * hw + o, x0);
                st4(xn + base + c * hw + o, update_of(x0 - mg * cw.wp[c], nz4(nz, base + c * hw + o), e, s));
            }
        }
    }
}

template <int R, class NZ>
__global__ __launch_bounds__(256) void step_plus_mcsr_kernel(const float* __restrict__ xt, const float* __restrict__ et,
                                                             int64_t et_bstride, NZ noise, const float* __restrict__ y,
                                                             const float* __restrict__ mask, float* __restrict__ x0o,
                                                             float* __restrict__ xn, int H, int W, int64_t total,
                                                             ddnm_step_scalars s, McsrW cw, float sy, float st, float eta,
                                                             float eta_c) {
    using S = McsrStrip<R>;
    const int64_t hw = (int64_t)H * W;
    const float a = s.sqrt_at_next;
    const bool active = a != 0.f && sy != 0.f;
    const SpectralCoef null = spectral_coef(0.f, active, a, sy, st, eta, eta_c);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const S t(i, H, W);
        const auto nz = bind(noise, t.b);
        const int64_t base = t.b * 3 * hw + t.pix, ebase = t.b * et_bstride + t.pix;
        float kept[S::NS] = {}, sx[S::NS] = {}, sn[S::NS] = {}, se[S::NS] = {};
#pragma unroll 1
        for (int row = 0; row < R; ++row) {
            const int64_t o = (int64_t)row * W;
            const f32x4 m = mcsr_mask4(mask, t.pix + o);
            f32x4 x0[3], e[3], n[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                e[c] = ld4(et + ebase + c * hw + o);
                x0[c] = x0_of(ld4(xt + base + c * hw + o), e[c], s);
                n[c] = nz4(nz, base + c * hw + o);
            }
            const f32x4 gx = ((x0[0] * cw.w[0] + x0[1] * cw.w[1]) + x0[2] * cw.w[2]) * m;
            const f32x4 gn = ((n[0] * cw.w[0] + n[1] * cw.w[1]) + n[2] * cw.w[2]) * m;
            const f32x4 ge = ((e[0] * cw.w[0] + e[1] * cw.w[1]) + e[2] * cw.w[2]) * m;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                kept[S::site(j)] += m[j]; sx[S::site(j)] += gx[j]; sn[S::site(j)] += gn[j]; se[S::site(j)] += ge[j];
            }
        }
        float g[S::NS];
#pragma unroll
        for (int k = 0; k < S::NS; ++k) {
            const float kj = mcsr_site_sum<R>(kept[k]), sxj = mcsr_site_sum<R>(sx[k]);
            const float snj = mcsr_site_sum<R>(sn[k]), sej = mcsr_site_sum<R>(se[k]);
            g[k] = 0.f;
            if (kj > 0.f) {
                const SpectralCoef cf = spectral_coef(sqrtf(kj) * cw.wn / (float)(R * R), active, a, sy, st, eta, eta_c);
                const float corr = (sxj - y[t.ysite + k] * (float)(R * R)) * (a * cf.lam);
                g[k] = ((snj * (cf.d1 - null.d1) + sej * (cf.d2 - null.d2)) - corr) / kj;
            }
        }
        f32x4 gv;
#pragma unroll
        for (int j = 0; j < 4; ++j) gv[j] = g[S::site(j)];
#pragma unroll 1
        for (int row = 0; row < R; ++row) {
            const int64_t o = (int64_t)row * W;
            const f32x4 mg = mcsr_mask4(mask, t.pix + o) * gv;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const f32x4 e = ld4(et + ebase + c * hw + o);
                const f32x4 x0 = x0_of(ld4(xt + base + c * hw + o), e, s);
                st4(x0o + base + c * hw + o, x0);
                const f32x4 n = nz4(nz, base + c * hw + o);
                st4(xn + base + c * hw + o, ((x0 * a + n * null.d1) + e * null.d2) + mg * cw.wp[c]);
            }
        }
    }
}

// strips of a launch: B images x H / r bands x W / 4 column groups (even for r = 8, where W % 8 == 0)
static inline int64_t mcsr_strips(int32_t B, int32_t H, int32_t W, int32_t r) { return (int64_t)B * (H / r) * (W / 4); }

#define MCSR_FOR_R(r, LAUNCH)        \
    switch (r) {                     \
    case 1: LAUNCH(1); break;        \
    case 2: LAUNCH(2); break;        \
    case 4: LAUNCH(4); break;        \
    default: LAUNCH(8); break;       \
    }

extern "C" int ddnm_op_mcsr_A_f32(const float* x, const float* mask, float* y, int32_t B, int32_t H, int32_t W, int32_t r,
                                  const float* w3_host, void* stream) {
    McsrW cw;
    if (!x || !y || !w3_host || B <= 0) return DDNM_E_BADARG;
    if (int e = mcsr_weights(w3_host, &cw)) return e;
    if (int e = mcsr_shape(H, W, r, 0)) return e;
    const int64_t total = mcsr_strips(B, H, W, r);
#define LAUNCH(R) DDNM_LAUNCH(mcsr_A_kernel<R>, GRID_1D(total), dim3(256), 0, (hipStream_t)stream, x, mask, y, H, W, total, cw)
    MCSR_FOR_R(r, LAUNCH)
#undef LAUNCH
    return 0;
}

extern "C" int ddnm_op_mcsr_pinv_f32(const float* y, const float* mask, float* x, int32_t B, int32_t H, int32_t W, int32_t r,
                                     const float* w3_host, void* stream) {
    McsrW cw;
    if (!x || !y || !w3_host || B <= 0) return DDNM_E_BADARG;
    if (int e = mcsr_weights(w3_host, &cw)) return e;
    if (int e = mcsr_shape(H, W, r, 0)) return e;
    const int64_t total = mcsr_strips(B, H, W, r);
#define LAUNCH(R) DDNM_LAUNCH(mcsr_pinv_kernel<R>, GRID_1D(total), dim3(256), 0, (hipStream_t)stream, y, mask, x, H, W, total, cw)
    MCSR_FOR_R(r, LAUNCH)
#undef LAUNCH
    return 0;
}

// the pointer checks shared by the four step entry points (the noise source is the entry point's own)
static inline bool mcsr_step_ptrs(const float* xt, const float* et, const float* y, const float* x0, const float* xt_next,
                                  const float* w3_host, const ddnm_step_scalars* s, int32_t B) {
    if (!xt || !et || !y || !xt_next || !w3_host || !s || B <= 0) return false;
    // two passes: the outputs must not overlap the inputs.  Only identity is caught here; the rest is the caller's to keep.
    return xt_next != xt && xt_next != et && xt_next != x0 && (!x0 || (x0 != xt && x0 != et));
}

template <class Src>
static int launch_step_mcsr(const float* xt, const float* et, int64_t et_bstride, Src src, const float* y, const float* mask,
                            float* x0, float* xt_next, int32_t B, int32_t H, int32_t W, int32_t r, const float* w3_host,
                            const ddnm_step_scalars* s, void* stream) {
    McsrW cw;
    if (int e = mcsr_weights(w3_host, &cw)) return e;
    if (int e = mcsr_shape(H, W, r, et_bstride)) return e;
    const int64_t total = mcsr_strips(B, H, W, r);
#define LAUNCH(R)                                                                                                          \
    DDNM_LAUNCH((step_mcsr_kernel<R, Src>), GRID_1D(total), dim3(256), 0, (hipStream_t)stream, xt, et, et_bstride, src, y, mask, \
                x0, xt_next, H, W, total, *s, cw)
    MCSR_FOR_R(r, LAUNCH)
#undef LAUNCH
    return 0;
}

template <class Src>
static int launch_step_plus_mcsr(const float* xt, const float* et, int64_t et_bstride, Src src, const float* y, const float* mask,
                                 float* x0_out, float* xt_next, int32_t B, int32_t H, int32_t W, int32_t r, const float* w3_host,
                                 float sigma_y, float sigma_t, float eta, const ddnm_step_scalars* s, void* stream) {
    McsrW cw;
    if (int e = mcsr_weights(w3_host, &cw)) return e;
    if (int e = mcsr_shape(H, W, r, et_bstride)) return e;
    const int64_t total = mcsr_strips(B, H, W, r);
    const float eta_c = (float)sqrt(1.0 - (double)eta * (double)eta);
#define LAUNCH(R)                                                                                                          \
    DDNM_LAUNCH((step_plus_mcsr_kernel<R, Src>), GRID_1D(total), dim3(256), 0, (hipStream_t)stream, xt, et, et_bstride, src, y, \
                mask, x0_out, xt_next, H, W, total, *s, cw, sigma_y, sigma_t, eta, eta_c)
    MCSR_FOR_R(r, LAUNCH)
#undef LAUNCH
    return 0;
}

extern "C" int ddnm_step_mcsr_f32(const float* xt, const float* et, int64_t et_bstride, const float* noise, const float* y,
                                  const float* mask, float* x0, float* xt_next, int32_t B, int32_t H, int32_t W, int32_t r,
                                  const float* w3_host, const ddnm_step_scalars* s, void* stream) {
    if (!mcsr_step_ptrs(xt, et, y, x0, xt_next, w3_host, s, B) || !noise_ok(noise, s)) return DDNM_E_BADARG;
    return launch_step_mcsr(xt, et, et_bstride, noise_src(noise, s, (int64_t)3 * H * W), y, mask, x0, xt_next, B, H, W, r, w3_host,
                            s, stream);
}

extern "C" int ddnm_step_mcsr_keyed_f32(const float* xt, const float* et, int64_t et_bstride, const uint32_t* keys,
                                        const float* y, const float* mask, float* x0, float* xt_next, int32_t B, int32_t H,
                                        int32_t W, int32_t r, const float* w3_host, const ddnm_step_scalars* s, void* stream) {
    if (!mcsr_step_ptrs(xt, et, y, x0, xt_next, w3_host, s, B) || !keys_ok(keys)) return DDNM_E_BADARG;
    return launch_step_mcsr(xt, et, et_bstride, keyed_src(keys, s, (int64_t)3 * H * W), y, mask, x0, xt_next, B, H, W, r, w3_host,
                            s, stream);
}

extern "C" int ddnm_step_plus_mcsr_f32(const float* xt, const float* et, int64_t et_bstride, const float* noise,
                                       const float* y, const float* mask, float* x0_out, float* xt_next, int32_t B, int32_t H,
                                       int32_t W, int32_t r, const float* w3_host, float sigma_y, float sigma_t, float eta,
                                       const ddnm_step_scalars* s, void* stream) {
    if (!x0_out || !mcsr_step_ptrs(xt, et, y, x0_out, xt_next, w3_host, s, B) || !noise_ok(noise, s)) return DDNM_E_BADARG;
    return launch_step_plus_mcsr(xt, et, et_bstride, noise_src(noise, s, (int64_t)3 * H * W), y, mask, x0_out, xt_next, B, H, W, r,
                                 w3_host, sigma_y, sigma_t, eta, s, stream);
}

extern "C" int ddnm_step_plus_mcsr_keyed_f32(const float* xt, const float* et, int64_t et_bstride, const uint32_t* keys,
                                             const float* y, const float* mask, float* x0_out, float* xt_next, int32_t B,
                                             int32_t H, int32_t W, int32_t r, const float* w3_host, float sigma_y,
                                             float sigma_t, float eta, const ddnm_step_scalars* s, void* stream) {
    if (!x0_out || !mcsr_step_ptrs(xt, et, y, x0_out, xt_next, w3_host, s, B) || !keys_ok(keys)) return DDNM_E_BADARG;
    return launch_step_plus_mcsr(xt, et, et_bstride, keyed_src(keys, s, (int64_t)3 * H * W), y, mask, x0_out, xt_next, B, H, W, r,
                                 w3_host, sigma_y, sigma_t, eta, s, stream);
}
#undef MCSR_FOR_R

// ---------------------------------------------------------------- fused: chroma subsampling (Y'CbCr 4:2:0, 4:2:2, 4:1:1)
// A = full-resolution luma, chroma averaged over sites of rw columns x rh rows (n = rw rh pixels).  M is an invertible
// 3 x 3 colour matrix with rows w_Y, w_Cb, w_Cr (no offsets: the data are centred):
//   Y[p] = w_Y . x[:, p],   Cb[site] = mean_{p in site} w_Cb . x[:, p],   Cr likewise;   y row = [ Y | Cb | Cr ] planes
// Per site, with mu(v) the mean colour and v_p - mu(v) the deviation, A splits into
//   AC: the n - 1 zero-mean patterns times colour; A sees only w^ = w_Y / |w_Y|, singular value |w_Y|; the two colour
//       directions orthogonal to w^ are null space;
//   DC: in orthonormal coordinates the 3 x 3 matrix D = diag(1, 1/sqrt n, 1/sqrt n) M = U_D S_D V_D^T.
// A launch has four singular values, the same at every site.  With Ybar the site mean of Y and w+ = w_Y / |w_Y|^2,
//   (A^+ y)[:, p] = w+ (Y_p - Ybar) + M^-1 (Ybar, Cb, Cr)^T
//   DDNM  (svd_ddnm.py:57-65):   x0h = x0 - lambda A^+(A x0 - y),  x_{t-1} = update_of(x0h, n, eps)
//   DDNM+ (svd_ddnm.py:118-131), a = sqrt_at_next, (lambda_a, d1_a, d2_a) the coefficients of |w_Y|, (Lambda, D1, D2)
//   those of S_D (diagonal), (1, d1n, d2n) those of 0, t_p(g) = w^ . g_p:
//     x_{t-1}[:, p] = a x0_p + d1n n_p + d2n eps_p
//        + w^  [ -a lambda_a ((t_p(x0) - tbar(x0)) - (Y_p - Ybar) / |w_Y|) + (d1_a - d1n)(t_p(n) - tbar(n)) + (d2_a - d2n)(..eps) ]
//        + V_D [ -a Lambda (V_D^T mu(x0) - S_D^-1 U_D^T z') + (D1 - d1n) V_D^T mu(n) + (D2 - d2n) V_D^T mu(eps) ],
//     z' = (Ybar, Cb / sqrt n, Cr / sqrt n).  The launcher evaluates the four coefficient triples once, in double, and folds
//     everything that is constant over a site into four 3 x 3 matrices (tbar(g) = w^ . mu(g) goes there too):
//       site term = Qx mu(x0) + Qz (Ybar, Cb, Cr) + Qn mu(n) + Qe mu(eps),   pixel term = w^ (kx t_p(x0) + ky Y_p + kn t_p(n) + ke t_p(eps))
//     so the kernel evaluates no coefficient and no square root.
// Mapping as for mcsr: one lane owns a strip of rh rows x 4 pixels x 3 planes -- two sites for rw = 2, one for rw = 4, half a
// site for rw = 8, where lanes 2i and 2i + 1 add their halves with one __shfl_xor.  Two passes per strip (site means, then
// the update; xt, eps and Y are read again and the noise is drawn again): THE OUTPUTS MUST NOT ALIAS xt OR eps.
// A measurement row has H W + 2 H W / n entries, which is no multiple of 4 when the number of sites is odd: then the rows of
// the images after the first are not 16-byte aligned and Y is moved one float at a time (`yal` = 0, uniform per launch).
struct ChromaC { float m[9], mi[9], wp[3]; };                       // M, M^-1, w+
struct ChromaPlusC { float qx[9], qz[9], qn[9], qe[9], wh[3], kx, ky, kn, ke, a, d1n, d2n; };
struct ChromaK { double mi[9], wp[3], wh[3], wn, U[9], S[3], V[9]; };   // ddnm_chroma_constants' 37 doubles, in this order

static inline bool chroma_site_ok(int32_t rw, int32_t rh) {
    return (rw == 2 && rh == 1) || (rw == 4 && rh == 1) || (rw == 2 && rh == 2) || (rw == 4 && rh == 4) || (rw == 8 && rh == 8);
}

// eigenvectors (columns of V) and eigenvalues of a symmetric 3 x 3 matrix by cyclic Jacobi rotations
static void chroma_jacobi3(double G[3][3], double V[3][3], double ev[3]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 64; ++sweep) {
        const double off = G[0][1] * G[0][1] + G[0][2] * G[0][2] + G[1][2] * G[1][2];
        const double tr = fabs(G[0][0]) + fabs(G[1][1]) + fabs(G[2][2]);
        if (off <= 1e-40 * tr * tr) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (G[p][q] == 0.0) continue;
                const double theta = (G[q][q] - G[p][p]) / (2.0 * G[p][q]);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) {
                    const double gp = G[k][p], gq = G[k][q];
                    G[k][p] = c * gp - s * gq;
                    G[k][q] = s * gp + c * gq;
                }
                for (int k = 0; k < 3; ++k) {
                    const double gp = G[p][k], gq = G[q][k];
                    G[p][k] = c * gp - s * gq;
                    G[q][k] = s * gp + c * gq;
                }
                for (int k = 0; k < 3; ++k) {
                    const double vp = V[k][p], vq = V[k][q];
                    V[k][p] = c * vp - s * vq;
                    V[k][q] = s * vp + c * vq;
                }
            }
    }
    for (int i = 0; i < 3; ++i) ev[i] = G[i][i];
}

// What the launchers derive from M, in double (row-major 3 x 3; the columns of U and V are the singular vectors, S descends).
// DDNM_E_BADARG: a null pointer or a singular M (|det M| < 1e-6 |M|_F^3); DDNM_E_SHAPE: an unsupported site.
static int chroma_constants(const float* m9, int32_t rw, int32_t rh, ChromaK* out) {
    if (!m9 || !out) return DDNM_E_BADARG;
    double M[3][3], f2 = 0.0;
    for (int i = 0; i < 9; ++i) { M[i / 3][i % 3] = (double)m9[i]; f2 += (double)m9[i] * (double)m9[i]; }
    double C[3][3];                                                  // cofactors: M^-1 = C^T / det
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            C[i][j] = M[i1][j1] * M[i2][j2] - M[i1][j2] * M[i2][j1];
        }
    const double det = M[0][0] * C[0][0] + M[0][1] * C[0][1] + M[0][2] * C[0][2];
    const double bound = 1e-6 * f2 * sqrt(f2);
    if (!(f2 > 0.0) || !(fabs(det) >= bound)) return DDNM_E_BADARG;
    if (!chroma_site_ok(rw, rh)) return DDNM_E_SHAPE;
    ChromaK k;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) k.mi[i * 3 + j] = C[j][i] / det;
    const double n2 = M[0][0] * M[0][0] + M[0][1] * M[0][1] + M[0][2] * M[0][2];
    k.wn = sqrt(n2);
    for (int j = 0; j < 3; ++j) { k.wp[j] = M[0][j] / n2; k.wh[j] = M[0][j] / k.wn; }
    const double e[3] = {1.0, 1.0 / sqrt((double)(rw * rh)), 1.0 / sqrt((double)(rw * rh))};
    double D[3][3], G[3][3], V[3][3], ev[3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) D[i][j] = e[i] * M[i][j];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) G[i][j] = D[0][i] * D[0][j] + D[1][i] * D[1][j] + D[2][i] * D[2][j];
    chroma_jacobi3(G, V, ev);
    int ord[3] = {0, 1, 2};
    for (int i = 0; i < 2; ++i)
        for (int j = i + 1; j < 3; ++j)
            if (ev[ord[j]] > ev[ord[i]]) { const int t = ord[i]; ord[i] = ord[j]; ord[j] = t; }
    for (int c = 0; c < 3; ++c) {
        const int o = ord[c];
        if (!(ev[o] > 0.0)) return DDNM_E_BADARG;
        k.S[c] = sqrt(ev[o]);
        for (int i = 0; i < 3; ++i) k.V[i * 3 + c] = V[i][o];
        for (int i = 0; i < 3; ++i) k.U[i * 3 + c] = (D[i][0] * V[0][o] + D[i][1] * V[1][o] + D[i][2] * V[2][o]) / k.S[c];
    }
    *out = k;
    return 0;
}

extern "C" int ddnm_chroma_constants(const float* m9_host, int32_t rw, int32_t rh, double* out) {
    ChromaK k;
    if (!out) return DDNM_E_BADARG;
    if (int e = chroma_constants(m9_host, rw, rh, &k)) return e;
    memcpy(out, &k, sizeof k);
    return 0;
}

// (lambda, d1, d2) of one singular value in double: the rules of spectral_coef above
static void chroma_coef(double s, double a, double sy, double st, double eta, double out[3]) {
    const double c1 = st * eta, c2 = st * sqrt(1.0 - eta * eta);
    out[0] = 1.0; out[1] = c1; out[2] = c2;
    if (s == 0.0 || a == 0.0 || sy == 0.0) return;
    const double thr = a * sy / s;
    if (st < thr) { out[0] = s * st * sqrt(1.0 - eta * eta) / a / sy; out[2] = 0.0; }
    if (st > thr) { out[1] = sqrt(st * st - a * a * sy * sy / (s * s)); out[2] = 0.0; }
}

static ChromaC chroma_args(const float* m9, const ChromaK& k) {
    ChromaC c;
    for (int i = 0; i < 9; ++i) { c.m[i] = m9[i]; c.mi[i] = (float)k.mi[i]; }
    for (int i = 0; i < 3; ++i) c.wp[i] = (float)k.wp[i];
    return c;
}

// the per-launch constants of the DDNM+ step: four coefficient triples, folded into the site matrices and pixel factors
static ChromaPlusC chroma_plus_args(const ChromaK& k, int32_t rw, int32_t rh, double a, double sy, double st, double eta) {
    double ca[3], cn[3], cd[3][3];
    chroma_coef(k.wn, a, sy, st, eta, ca);
    chroma_coef(0.0, a, sy, st, eta, cn);
    for (int c = 0; c < 3; ++c) chroma_coef(k.S[c], a, sy, st, eta, cd[c]);
    const double e[3] = {1.0, 1.0 / sqrt((double)(rw * rh)), 1.0 / sqrt((double)(rw * rh))};
    ChromaPlusC p;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double qx = 0.0, qz = 0.0, qn = 0.0, qe = 0.0;
            for (int c = 0; c < 3; ++c) {
                const double vi = k.V[i * 3 + c], vj = k.V[j * 3 + c];
                qx -= vi * a * cd[c][0] * vj;
                qz += vi * a * cd[c][0] / k.S[c] * k.U[j * 3 + c] * e[j];
                qn += vi * (cd[c][1] - cn[1]) * vj;
                qe += vi * (cd[c][2] - cn[2]) * vj;
            }
            const double ww = k.wh[i] * k.wh[j];
            p.qx[i * 3 + j] = (float)(qx + a * ca[0] * ww);
            p.qz[i * 3 + j] = (float)(qz - (j == 0 ? a * ca[0] / k.wn * k.wh[i] : 0.0));
            p.qn[i * 3 + j] = (float)(qn - (ca[1] - cn[1]) * ww);
            p.qe[i * 3 + j] = (float)(qe - (ca[2] - cn[2]) * ww);
        }
    for (int i = 0; i < 3; ++i) p.wh[i] = (float)k.wh[i];
    p.kx = (float)(-a * ca[0]);
    p.ky = (float)(a * ca[0] / k.wn);
    p.kn = (float)(ca[1] - cn[1]);
    p.ke = (float)(ca[2] - cn[2]);
    p.a = (float)a; p.d1n = (float)cn[1]; p.d2n = (float)cn[2];
    return p;
}

// sizes of every chroma entry point, after its pointer checks (DDNM_E_BADARG before DDNM_E_SHAPE)
static int chroma_shape(int32_t H, int32_t W, int32_t rw, int32_t rh, int64_t et_bstride) {
    if (!chroma_site_ok(rw, rh)) return DDNM_E_SHAPE;
    if (H <= 0 || W <= 0 || H % rh || W % rw || (W & 3) || (et_bstride & 3)) return DDNM_E_SHAPE;
    return 0;
}

// a strip of RH rows x 4 pixels: its sites (NS of them) and the geometry shared by the four kernels
template <int RW, int RH>
struct ChromaStrip {
    static constexpr int NS = RW == 2 ? 2 : 1;                            // whole sites of a strip (RW = 8: half of one)
    static constexpr int N = RW * RH;
    static __device__ __forceinline__ int site(int j) { return RW == 2 ? j / 2 : 0; }   // site of column j of the strip
    int64_t b, pix, csite;   // image, offset of the strip's first row inside a plane, index of its first site in a chroma plane
    __device__ __forceinline__ ChromaStrip(int64_t i, int H, int W) {
        const int W4 = W >> 2;
        const int64_t per_img = (int64_t)(H / RH) * W4;
        b = i / per_img;
        const int64_t q = i - b * per_img;
        const int sy = (int)(q / W4), xg = (int)(q - (int64_t)sy * W4);
        pix = (int64_t)sy * RH * W + xg * 4;
        csite = (int64_t)sy * (W / RW) + xg * 4 / RW;
    }
};

// the other half of a site's sum (RW = 8: the neighbouring lane's strip); the strips of a site are i and i ^ 1 and their
// number per row is even, so both lanes are in the loop together
template <int RW>
__device__ __forceinline__ float chroma_site_sum(float v) { return RW == 8 ? v + __shfl_xor(v, 1) : v; }

__device__ __forceinline__ f32x4 chroma_ldy(const float* p, bool al) { return al ? ld4(p) : f32x4{p[0], p[1], p[2], p[3]}; }
__device__ __forceinline__ void chroma_sty(float* p, f32x4 v, bool al) {
    if (al) { st4(p, v); return; }
    p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3];
}
__device__ __forceinline__ f32x4 dot3(const float* w, f32x4 r, f32x4 g, f32x4 b) { return (r * w[0] + g * w[1]) + b * w[2]; }
__device__ __forceinline__ float dot3(const float* w, float r, float g, float b) { return (r * w[0] + g * w[1]) + b * w[2]; }

// y = A x
template <int RW, int RH>
__global__ __launch_bounds__(256) void chroma_A_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W,
                                                       int64_t total, bool yal, ChromaC cc) {
    using S = ChromaStrip<RW, RH>;
    const int64_t hw = (int64_t)H * W, hwn = hw / S::N;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const S t(i, H, W);
        const float* xb = x + t.b * 3 * hw + t.pix;
        float* yb = y + t.b * (hw + 2 * hwn);
        float sb[S::NS] = {}, sr[S::NS] = {};
#pragma unroll
        for (int row = 0; row < RH; ++row) {
            const int64_t o = (int64_t)row * W;
            const f32x4 r = ld4(xb + o), g = ld4(xb + hw + o), b = ld4(xb + 2 * hw + o);
            chroma_sty(yb + t.pix + o, dot3(cc.m, r, g, b), yal);
            const f32x4 cb = dot3(cc.m + 3, r, g, b), cr = dot3(cc.m + 6, r, g, b);
#pragma unroll
            for (int j = 0; j < 4; ++j) { sb[S::site(j)] += cb[j]; sr[S::site(j)] += cr[j]; }
        }
#pragma unroll
        for (int k = 0; k < S::NS; ++k) {
            const float vb = chroma_site_sum<RW>(sb[k]) / (float)S::N, vr = chroma_site_sum<RW>(sr[k]) / (float)S::N;
            if (RW < 8 || !(i & 1)) { yb[hw + t.csite + k] = vb; yb[hw + hwn + t.csite + k] = vr; }
        }
    }
}

// x = A^+ y
template <int RW, int RH>
__global__ __launch_bounds__(256) void chroma_pinv_kernel(const float* __restrict__ y, float* __restrict__ x, int H, int W,
                                                          int64_t total, bool yal, ChromaC cc) {
    using S = ChromaStrip<RW, RH>;
    const int64_t hw = (int64_t)H * W, hwn = hw / S::N;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const S t(i, H, W);
        const float* yb = y + t.b * (hw + 2 * hwn);
        float sy[S::NS] = {};
#pragma unroll
        for (int row = 0; row < RH; ++row) {
            const f32x4 yp = chroma_ldy(yb + t.pix + (int64_t)row * W, yal);
#pragma unroll
            for (int j = 0; j < 4; ++j) sy[S::site(j)] += yp[j];
        }
        float ym[S::NS], dc[3][S::NS];
#pragma unroll
        for (int k = 0; k < S::NS; ++k) {
            ym[k] = chroma_site_sum<RW>(sy[k]) / (float)S::N;
            const float cb = yb[hw + t.csite + k], cr = yb[hw + hwn + t.csite + k];
#pragma unroll
            for (int c = 0; c < 3; ++c) dc[c][k] = dot3(cc.mi + 3 * c, ym[k], cb, cr);
        }
        f32x4 ymv, dcv[3];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ymv[j] = ym[S::site(j)];
#pragma unroll
            for (int c = 0; c < 3; ++c) dcv[c][j] = dc[c][S::site(j)];
        }
        float* xb = x + t.b * 3 * hw + t.pix;
#pragma unroll
        for (int row = 0; row < RH; ++row) {
            const int64_t o = (int64_t)row * W;
            const f32x4 d = chroma_ldy(yb + t.pix + o, yal) - ymv;
#pragma unroll
            for (int c = 0; c < 3; ++c) st4(xb + c * hw + o, d * cc.wp[c] + dcv[c]);
        }
    }
}

template <int RW, int RH, class NZ>
__global__ __launch_bounds__(256) void step_chroma_kernel(const float* __restrict__ xt, const float* __restrict__ et,
                                                          int64_t et_bstride, NZ noise, const float* __restrict__ y,
                                                          float* __restrict__ x0o, float* __restrict__ xn, int H, int W,
                                                          int64_t total, bool yal, ddnm_step_scalars s, ChromaC cc) {
    using S = ChromaStrip<RW, RH>;
    const int64_t hw = (int64_t)H * W, hwn = hw / S::N;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const S t(i, H, W);
        const auto nz = bind(noise, t.b);
        const int64_t base = t.b * 3 * hw + t.pix, ebase = t.b * et_bstride + t.pix;
        const float* yb = y + t.b * (hw + 2 * hwn);
        // pass 1: the site means of the residual A x0 - y (luma, Cb, Cr)
        float sy[S::NS] = {}, sb[S::NS] = {}, sr[S::NS] = {};
#pragma unroll 1
        for (int row = 0; row < RH; ++row) {
            const int64_t o = (int64_t)row * W;
            f32x4 x0[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) x0[c] = x0_of(ld4(xt + base + c * hw + o), ld4(et + ebase + c * hw + o), s);
            const f32x4 ry = dot3(cc.m, x0[0], x0[1], x0[2]) - chroma_ldy(yb + t.pix + o, yal);
            const f32x4 cb = dot3(cc.m + 3, x0[0], x0[1], x0[2]), cr = dot3(cc.m + 6, x0[0], x0[1], x0[2]);
#pragma unroll
            for (int j = 0; j < 4; ++j) { sy[S::site(j)] += ry[j]; sb[S::site(j)] += cb[j]; sr[S::site(j)] += cr[j]; }
        }
        float rm[S::NS], dc[3][S::NS];
#pragma unroll
        for (int k = 0; k < S::NS; ++k) {
            rm[k] = chroma_site_sum<RW>(sy[k]) / (float)S::N;
            const float rb = chroma_site_sum<RW>(sb[k]) / (float)S::N - yb[hw + t.csite + k];
            const float rr = chroma_site_sum<RW>(sr[k]) / (float)S::N - yb[hw + hwn + t.csite + k];
#pragma unroll
            for (int c = 0; c < 3; ++c) dc[c][k] = dot3(cc.mi + 3 * c, rm[k], rb, rr) * s.lambda;
        }
        f32x4 rmv, dcv[3];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            rmv[j] = rm[S::site(j)];
#pragma unroll
            for (int c = 0; c < 3; ++c) dcv[c][j] = dc[c][S::site(j)];
        }
        // pass 2: x0h = x0 - lambda (w+ (r_p - rbar) + M^-1 (rbar, rCb, rCr)), then the update
#pragma unroll 1
        for (int row = 0; row < RH; ++row) {
            const int64_t o = (int64_t)row * W;
            f32x4 x0[3], e[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                e[c] = ld4(et + ebase + c * hw + o);
                x0[c] = x0_of(ld4(xt + base + c * hw + o), e[c], s);
            }
            const f32x4 g = ((dot3(cc.m, x0[0], x0[1], x0[2]) - chroma_ldy(yb + t.pix + o, yal)) - rmv) * s.lambda;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (x0o) st4(x0o + base + c * hw + o, x0[c]);
                st4(xn + base + c * hw + o, update_of(x0[c] - (g * cc.wp[c] + dcv[c]), nz4(nz, base + c * hw + o), e[c], s));
            }
        }
    }
}

template <int RW, int RH, class NZ>
__global__ __launch_bounds__(256) void step_plus_chroma_kernel(const float* __restrict__ xt, const float* __restrict__ et,
                                                               int64_t et_bstride, NZ noise, const float* __restrict__ y,
                                                               float* __restrict__ x0o, float* __restrict__ xn, int H, int W,
                                                               int64_t total, bool yal, ddnm_step_scalars s, ChromaPlusC cp) {
    using S = ChromaStrip<RW, RH>;
    const int64_t hw = (int64_t)H * W, hwn = hw / S::N;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const S t(i, H, W);
        const auto nz = bind(noise, t.b);
        const int64_t base = t.b * 3 * hw + t.pix, ebase = t.b * et_bstride + t.pix;
        const float* yb = y + t.b * (hw + 2 * hwn);
        // pass 1: the site sums of x0, n, eps per colour and of Y
        float sx[3][S::NS] = {}, sn[3][S::NS] = {}, se[3][S::NS] = {}, sy[S::NS] = {};
#pragma unroll 1
        for (int row = 0; row < RH; ++row) {
            const int64_t o = (int64_t)row * W;
            const f32x4 yp = chroma_ldy(yb + t.pix + o, yal);
#pragma unroll
            for (int j = 0; j < 4; ++j) sy[S::site(j)] += yp[j];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const f32x4 e = ld4(et + ebase + c * hw + o);
                const f32x4 x0 = x0_of(ld4(xt + base + c * hw + o), e, s);
                const f32x4 n = nz4(nz, base + c * hw + o);
#pragma unroll
                for (int j = 0; j < 4; ++j) { sx[c][S::site(j)] += x0[j]; sn[c][S::site(j)] += n[j]; se[c][S::site(j)] += e[j]; }
            }
        }
        float dc[3][S::NS];
#pragma unroll
        for (int k = 0; k < S::NS; ++k) {
            float mx[3], mn[3], me[3], z[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                mx[c] = chroma_site_sum<RW>(sx[c][k]) / (float)S::N;
                mn[c] = chroma_site_sum<RW>(sn[c][k]) / (float)S::N;
                me[c] = chroma_site_sum<RW>(se[c][k]) / (float)S::N;
            }
            z[0] = chroma_site_sum<RW>(sy[k]) / (float)S::N;
            z[1] = yb[hw + t.csite + k];
            z[2] = yb[hw + hwn + t.csite + k];
#pragma unroll
            for (int c = 0; c < 3; ++c)
                dc[c][k] = (dot3(cp.qx + 3 * c, mx[0], mx[1], mx[2]) + dot3(cp.qz + 3 * c, z[0], z[1], z[2])) +
                           (dot3(cp.qn + 3 * c, mn[0], mn[1], mn[2]) + dot3(cp.qe + 3 * c, me[0], me[1], me[2]));
        }
        f32x4 dcv[3];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) dcv[c][j] = dc[c][S::site(j)];
        // pass 2: the pixel term along w^, the site term, the update
#pragma unroll 1
        for (int row = 0; row < RH; ++row) {
            const int64_t o = (int64_t)row * W;
            f32x4 x0[3], e[3], n[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                e[c] = ld4(et + ebase + c * hw + o);
                x0[c] = x0_of(ld4(xt + base + c * hw + o), e[c], s);
                n[c] = nz4(nz, base + c * hw + o);
            }
            const f32x4 tp = (dot3(cp.wh, x0[0], x0[1], x0[2]) * cp.kx + chroma_ldy(yb + t.pix + o, yal) * cp.ky) +
                             (dot3(cp.wh, n[0], n[1], n[2]) * cp.kn + dot3(cp.wh, e[0], e[1], e[2]) * cp.ke);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                st4(x0o + base + c * hw + o, x0[c]);
                st4(xn + base + c * hw + o, ((x0[c] * cp.a + n[c] * cp.d1n) + e[c] * cp.d2n) + (tp * cp.wh[c] + dcv[c]));
            }
        }
    }
}

// strips of a launch: B images x H / rh bands x W / 4 column groups (even per row for rw = 8, where W % 8 == 0)
static inline int64_t chroma_strips(int32_t B, int32_t H, int32_t W, int32_t rh) { return (int64_t)B * (H / rh) * (W / 4); }
// whether every image's measurement row starts 16-byte aligned (given that y does)
static inline bool chroma_y_aligned(int32_t H, int32_t W, int32_t rw, int32_t rh) {
    return (((int64_t)H * W + 2 * ((int64_t)H * W / (rw * rh))) & 3) == 0;
}

#define CHROMA_FOR_SITE(rw, rh, LAUNCH)           \
    switch (rw * 16 + rh) {                       \
    case 2 * 16 + 1: LAUNCH(2, 1); break;         \
    case 4 * 16 + 1: LAUNCH(4, 1); break;         \
    case 2 * 16 + 2: LAUNCH(2, 2); break;         \
    case 4 * 16 + 4: LAUNCH(4, 4); break;         \
    default: LAUNCH(8, 8); break;                 \
    }

extern "C" int ddnm_op_chroma_A_f32(const float* x, float* y, int32_t B, int32_t H, int32_t W, int32_t rw, int32_t rh,
                                    const float* m9_host, void* stream) {
    ChromaK k;
    if (!x || !y || !m9_host || B <= 0) return DDNM_E_BADARG;
    if (int e = chroma_constants(m9_host, rw, rh, &k)) return e;        // a singular M (DDNM_E_BADARG) before the site
    if (int e = chroma_shape(H, W, rw, rh, 0)) return e;
    const ChromaC cc = chroma_args(m9_host, k);
    const int64_t total = chroma_strips(B, H, W, rh);
    const bool yal = chroma_y_aligned(H, W, rw, rh);
#define LAUNCH(RW, RH) \
    DDNM_LAUNCH((chroma_A_kernel<RW, RH>), GRID_1D(total), dim3(256), 0, (hipStream_t)stream, x, y, H, W, total, yal, cc)
    CHROMA_FOR_SITE(rw, rh, LAUNCH)
#undef LAUNCH
    return 0;
}

extern "C" int ddnm_op_chroma_pinv_f32(const float* y, float* x, int32_t B, int32_t H, int32_t W, int32_t rw, int32_t rh,
                                       const float* m9_host, void* stream) {
    ChromaK k;
    if (!x || !y || !m9_host || B <= 0) return DDNM_E_BADARG;
    if (int e = chroma_constants(m9_host, rw, rh, &k)) return e;
    if (int e = chroma_shape(H, W, rw, rh, 0)) return e;
    const ChromaC cc = chroma_args(m9_host, k);
    const int64_t total = chroma_strips(B, H, W, rh);
    const bool yal = chroma_y_aligned(H, W, rw, rh);
#define LAUNCH(RW, RH) \
    DDNM_LAUNCH((chroma_pinv_kernel<RW, RH>), GRID_1D(total), dim3(256), 0, (hipStream_t)stream, y, x, H, W, total, yal, cc)
    CHROMA_FOR_SITE(rw, rh, LAUNCH)
#undef LAUNCH
    return 0;
}

// the pointer checks shared by the four step entry points (the noise source is the entry point's own)
static inline bool chroma_step_ptrs(const float* xt, const float* et, const float* y, const float* x0, const float* xt_next,
                                    const float* m9_host, const ddnm_step_scalars* s, int32_t B) {
    if (!xt || !et || !y || !xt_next || !m9_host || !s || B <= 0) return false;
    // two passes: the outputs must not overlap the inputs.  Only identity is caught here; the rest is the caller's to keep.
    return xt_next != xt && xt_next != et && xt_next != x0 && (!x0 || (x0 != xt && x0 != et));
}

template <class Src>
static int launch_step_chroma(const float* xt, const float* et, int64_t et_bstride, Src src, const float* y, float* x0,
                              float* xt_next, int32_t B, int32_t H, int32_t W, int32_t rw, int32_t rh, const float* m9_host,
                              const ddnm_step_scalars* s, void* stream) {
    ChromaK k;
    if (int e = chroma_constants(m9_host, rw, rh, &k)) return e;
    if (int e = chroma_shape(H, W, rw, rh, et_bstride)) return e;
    const ChromaC cc = chroma_args(m9_host, k);
    const int64_t total = chroma_strips(B, H, W, rh);
    const bool yal = chroma_y_aligned(H, W, rw, rh);
#define LAUNCH(RW, RH)                                                                                                     \
    DDNM_LAUNCH((step_chroma_kernel<RW, RH, Src>), GRID_1D(total), dim3(256), 0, (hipStream_t)stream, xt, et, et_bstride, src, \
                y, x0, xt_next, H, W, total, yal, *s, cc)
    CHROMA_FOR_SITE(rw, rh, LAUNCH)
#undef LAUNCH
    return 0;
}

template <class Src>
static int launch_step_plus_chroma(const float* xt, const float* et, int64_t et_bstride, Src src, const float* y, float* x0_out,
                                   float* xt_next, int32_t B, int32_t H, int32_t W, int32_t rw, int32_t rh,
                                   const float* m9_host, float sigma_y, float sigma_t, float eta, const ddnm_step_scalars* s,
                                   void* stream) {
    ChromaK k;
    if (int e = chroma_constants(m9_host, rw, rh, &k)) return e;
    if (int e = chroma_shape(H, W, rw, rh, et_bstride)) return e;
    const ChromaPlusC cp = chroma_plus_args(k, rw, rh, (double)s->sqrt_at_next, (double)sigma_y, (double)sigma_t, (double)eta);
    const int64_t total = chroma_strips(B, H, W, rh);
    const bool yal = chroma_y_aligned(H, W, rw, rh);
#define LAUNCH(RW, RH)                                                                                                     \
    DDNM_LAUNCH((step_plus_chroma_kernel<RW, RH, Src>), GRID_1D(total), dim3(256), 0, (hipStream_t)stream, xt, et, et_bstride, \
                src, y, x0_out, xt_next, H, W, total, yal, *s, cp)
    CHROMA_FOR_SITE(rw, rh, LAUNCH)
#undef LAUNCH
    return 0;
}

extern "C" int ddnm_step_chroma_f32(const float* xt, const float* et, int64_t et_bstride, const float* noise, const float* y,
                                    float* x0, float* xt_next, int32_t B, int32_t H, int32_t W, int32_t rw, int32_t rh,
                                    const float* m9_host, const ddnm_step_scalars* s, void* stream) {
    if (!chroma_step_ptrs(xt, et, y, x0, xt_next, m9_host, s, B) || !noise_ok(noise, s)) return DDNM_E_BADARG;
    return launch_step_chroma(xt, et, et_bstride, noise_src(noise, s, (int64_t)3 * H * W), y, x0, xt_next, B, H, W, rw, rh,
                              m9_host, s, stream);
}

extern "C" int ddnm_step_chroma_keyed_f32(const float* xt, const float* et, int64_t et_bstride, const uint32_t* keys,
                                          const float* y, float* x0, float* xt_next, int32_t B, int32_t H, int32_t W, int32_t rw,
                                          int32_t rh, const float* m9_host, const ddnm_step_scalars* s, void* stream) {
    if (!chroma_step_ptrs(xt, et, y, x0, xt_next, m9_host, s, B) || !keys_ok(keys)) return DDNM_E_BADARG;
    return launch_step_chroma(xt, et, et_bstride, keyed_src(keys, s, (int64_t)3 * H * W), y, x0, xt_next, B, H, W, rw, rh,
                              m9_host, s, stream);
}

extern "C" int ddnm_step_plus_chroma_f32(const float* xt, const float* et, int64_t et_bstride, const float* noise,
                                         const float* y, float* x0_out, float* xt_next, int32_t B, int32_t H, int32_t W,
                                         int32_t rw, int32_t rh, const float* m9_host, float sigma_y, float sigma_t, float eta,
                                         const ddnm_step_scalars* s, void* stream) {
    if (!x0_out || !chroma_step_ptrs(xt, et, y, x0_out, xt_next, m9_host, s, B) || !noise_ok(noise, s)) return DDNM_E_BADARG;
    return launch_step_plus_chroma(xt, et, et_bstride, noise_src(noise, s, (int64_t)3 * H * W), y, x0_out, xt_next, B, H, W, rw,
                                   rh, m9_host, sigma_y, sigma_t, eta, s, stream);
}

extern "C" int ddnm_step_plus_chroma_keyed_f32(const float* xt, const float* et, int64_t et_bstride, const uint32_t* keys,
                                               const float* y, float* x0_out, float* xt_next, int32_t B, int32_t H, int32_t W,
                                               int32_t rw, int32_t rh, const float* m9_host, float sigma_y, float sigma_t,
                                               float eta, const ddnm_step_scalars* s, void* stream) {
    if (!x0_out || !chroma_step_ptrs(xt, et, y, x0_out, xt_next, m9_host, s, B) || !keys_ok(keys)) return DDNM_E_BADARG;
    return launch_step_plus_chroma(xt, et, et_bstride, keyed_src(keys, s, (int64_t)3 * H * W), y, x0_out, xt_next, B, H, W, rw,
                                   rh, m9_host, sigma_y, sigma_t, eta, s, stream);
}
#undef CHROMA_FOR_SITE


// ---------------------------------------------------------------------------------------------
// hq_demo sampler (DDPM posterior + DDNM core + mask-shift tiles), hq_demo/guided_diffusion/gaussian_diffusion.py.
// All HBM-bound elementwise passes over one 256x256 tile batch; evaluation order of the reference kept.
// ---------------------------------------------------------------------------------------------
// x0 = clamp(c_recip * x_t - c_recipm1 * eps, -1, 1)   (:404-410, process_xstart :293-298); eps = first 3 of 6 channels
__global__ __launch_bounds__(256) void hq_x0_kernel(const float* __restrict__ xt, const float* __restrict__ eps,
                                                    int64_t eps_bstride, float* __restrict__ x0, int64_t chw,
                                                    int64_t total, float c_recip, float c_recipm1, int clip) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / chw, r = i - b * chw;
        float v = c_recip * xt[i] - c_recipm1 * eps[b * eps_bstride + r];
        if (clip) v = fminf(fmaxf(v, -1.f), 1.f);
        x0[i] = v;
    }
}

extern "C" int ddnm_hq_x0_f32(const float* xt, const float* eps, int64_t eps_bstride, float* x0, int32_t B, int64_t chw,
                              float c_recip, float c_recipm1, int32_t clip, void* stream) {
    if (!xt || !eps || !x0 || B <= 0 || chw <= 0) return DDNM_E_BADARG;
    const int64_t total = (int64_t)B * chw;
    DDNM_LAUNCH(hq_x0_kernel, GRID_1D(total), dim3(256), 0, (hipStream_t)stream, xt, eps, eps_bstride, x0, chw, total,
                c_recip, c_recipm1, clip);
    return 0;
}

// x0_hat = lambda * A^+ y + x0 - lambda * A^+ A x0   (Eq. 17, :339)
__global__ __launch_bounds__(256) void hq_project_kernel(const float* __restrict__ x0, const float* __restrict__ apy,
                                                         const float* __restrict__ apax0, float* __restrict__ out,
                                                         int64_t total, float lam) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
        out[i] = lam * apy[i] + x0[i] - lam * apax0[i];
}

extern "C" int ddnm_hq_project_f32(const float* x0, const float* apy, const float* apax0, float* x0_hat, int64_t n,
                                   float lam, void* stream) {
    if (!x0 || !apy || !apax0 || !x0_hat || n <= 0) return DDNM_E_BADARG;
    DDNM_LAUNCH(hq_project_kernel, GRID_1D(n), dim3(256), 0, (hipStream_t)stream, x0, apy, apax0, x0_hat, n, lam);
    return 0;
}

// dst[p, dy + i, dx + j] = src[p, sy + i, sx + j]: tile windows of A^+ y, the mask-shift paste of already restored
// strips into x0_hat (:341-377) and the write-back of a finished tile (:737-746)
__global__ __launch_bounds__(256) void copy_rect_kernel(const float* __restrict__ src, int Hs, int Ws, int sy, int sx,
                                                        float* __restrict__ dst, int Hd, int Wd, int dy, int dx, int h,
                                                        int w, int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int j = (int)(i % w);
        const int64_t t = i / w;
        const int r = (int)(t % h);
        const int64_t pl = t / h;
        dst[(pl * Hd + dy + r) * Wd + dx + j] = src[(pl * Hs + sy + r) * Ws + sx + j];
    }
}

extern "C" int ddnm_copy_rect_f32(const float* src, int32_t Hs, int32_t Ws, int32_t sy, int32_t sx, float* dst, int32_t Hd,
                                  int32_t Wd, int32_t dy, int32_t dx, int32_t planes, int32_t h, int32_t w, void* stream) {
    if (!src || !dst || planes <= 0 || h <= 0 || w <= 0) return DDNM_E_BADARG;
    if (sy < 0 || sx < 0 || dy < 0 || dx < 0 || sy + h > Hs || sx + w > Ws || dy + h > Hd || dx + w > Wd) return DDNM_E_SHAPE;
    const int64_t total = (int64_t)planes * h * w;
    DDNM_LAUNCH(copy_rect_kernel, GRID_1D(total), dim3(256), 0, (hipStream_t)stream, src, Hs, Ws, sy, sx, dst, Hd, Wd, dy,
                dx, h, w, total);
    return 0;
}

// x_{t-1} = (coef1 * x0_hat + coef2 * x_t [+ gamma * grad]) + noise_scale * noise   (:214-229, :417-427, :474-480)
__global__ __launch_bounds__(256) void hq_sample_kernel(const float* __restrict__ x0h, const float* __restrict__ xt,
                                                        const float* __restrict__ grad, const float* __restrict__ noise,
                                                        float* __restrict__ out, int64_t total, float coef1, float coef2,
                                                        float gamma, float noise_scale) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        float m = coef1 * x0h[i] + coef2 * xt[i];
        if (grad) m = m + gamma * grad[i];
        out[i] = m + noise_scale * noise[i];
    }
}

extern "C" int ddnm_hq_sample_f32(const float* x0_hat, const float* xt, const float* grad, const float* noise, float* out,
                                  int64_t n, float coef1, float coef2, float gamma, float noise_scale, void* stream) {
    if (!x0_hat || !xt || !noise || !out || n <= 0) return DDNM_E_BADARG;
    DDNM_LAUNCH(hq_sample_kernel, GRID_1D(n), dim3(256), 0, (hipStream_t)stream, x0_hat, xt, grad, noise, out, n, coef1,
                coef2, gamma, noise_scale);
    return 0;
}
