// Image-quality metrics next to PSNR (ddnm_step.hip::finalize_psnr_kernel): SSIM of Wang et al. 2004 with the 11x11
// Gaussian window (sigma 1.5), valid positions only, C1 = 0.01^2, C2 = 0.03^2 on the [0, 1] scale.
//
// One 256-thread workgroup per 32 (wide) x 16 (tall) tile of valid positions of one plane:
//   1. the 26 x 42 halo of both images goes to LDS once, fp32, with the optional clamp((v+1)/2, 0, 1) applied on load;
//   2. the horizontal 11-tap pass writes the five moment planes (x, y, x^2, y^2, xy) of 26 x 32 to LDS in FP64;
//   3. the vertical pass and the SSIM map stay in registers (fp64), two positions per thread;
//   4. the tile's sum is reduced over the wave with __shfl_xor, over the four waves through LDS in a fixed order, and
//      written as ONE double to work[plane * tiles + tile].
// A second kernel adds the C * tiles partials of each image in a fixed order and divides.  No floating-point atomics:
// an image's value depends on its own pixels only, bit for bit, wherever it sits in a batch.
//
// Sample statistics (ddnm_sample_stats_f32, below the SSIM): the per-pixel mean and standard deviation over the K
// restorations of one measurement, and their per-image summaries, with the same no-atomics reduction.
//
// Data consistency (ddnm_consistency_f32, below the sample statistics): the residual A x^ - y of a finished batch, per
// image, as sum |d|, sum d^2 (fp64) and max |d| (fp32) over the valid entries of each measurement row -- the one figure of
// merit that needs no ground truth.  d = (double)ax - (double)y is exact; the per-workgroup partials are added in an order
// that depends on the row length alone, so a row's three values do not depend on the batch around it either.
//
// Why fp64 moments: in fp32 the variance w*x^2 - mu^2 of a flat region cancels to ~1e-7 absolute against C2 = 9e-4,
// which moves the per-image value by 1e-4 (constant 0.3 vs 0.7; 0.9 vs 0.9 + 1e-3 * noise).  The product of two fp32
// values is exact in fp64, so x^2, y^2 and xy carry no rounding at all and SSIM(x, x) is exactly 1.  The tile is 16 tall
// instead of 32 so that the fp64 moment planes (33 KB) and the halo (8.7 KB) stay inside the 64 KB of static LDS.
#include <math.h>

#include "common.h"

namespace {

constexpr int SSIM_WIN = 11;
constexpr int SSIM_TW = 32, SSIM_TH = 16;                                   // tile of valid positions
constexpr int SSIM_HW = SSIM_TW + SSIM_WIN - 1, SSIM_HH = SSIM_TH + SSIM_WIN - 1;   // 42 x 26 halo

struct ssim_window {
    double g[SSIM_WIN];
};

__device__ __forceinline__ float ssim_load(const float* p, int transform) {
    const float v = *p;
    return transform ? fminf(fmaxf((v + 1.0f) / 2.0f, 0.0f), 1.0f) : v;
}

__global__ __launch_bounds__(256) void ssim_tile_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                        double* __restrict__ work, int H, int W, int tiles_x,
                                                        int tiles, int transform, ssim_window win) {
    // only the fma() calls written below fuse: SSIM(x, x) == 1 needs mu_x^2 + mu_y^2 and 2 mu_x mu_y, sigma_x^2 + sigma_y^2
    // and 2 sigma_xy to round identically, which a product contracted into one of the two sums would break
#pragma clang fp contract(off)
    __shared__ float sx[SSIM_HH][SSIM_HW];
    __shared__ float sy[SSIM_HH][SSIM_HW];
    __shared__ double mom[5][SSIM_HH][SSIM_TW];
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const int plane = blockIdx.x / tiles, tile = blockIdx.x - plane * tiles;
    const int ty0 = (tile / tiles_x) * SSIM_TH, tx0 = (tile % tiles_x) * SSIM_TW;
    const float* xp = x + (int64_t)plane * H * W;
    const float* yp = y + (int64_t)plane * H * W;

    // halo: rows / columns past the plane repeat its last pixel; they only feed positions that are masked below
    for (int i = tid; i < SSIM_HH * SSIM_HW; i += 256) {
        const int r = i / SSIM_HW, c = i - r * SSIM_HW;
        const int64_t off = (int64_t)min(ty0 + r, H - 1) * W + min(tx0 + c, W - 1);
        sx[r][c] = ssim_load(xp + off, transform);
        sy[r][c] = ssim_load(yp + off, transform);
    }
    __syncthreads();

    for (int i = tid; i < SSIM_HH * SSIM_TW; i += 256) {
        const int r = i / SSIM_TW, c = i - r * SSIM_TW;
        double mx = 0.0, my = 0.0, mxx = 0.0, myy = 0.0, mxy = 0.0;
#pragma unroll
        for (int k = 0; k < SSIM_WIN; ++k) {
            const double a = (double)sx[r][c + k], b = (double)sy[r][c + k], g = win.g[k];
            const double aa = a * a, bb = b * b, ab = a * b;      // exact: 24-bit x 24-bit significands
            mx = fma(g, a, mx);
            my = fma(g, b, my);
            mxx = fma(g, aa, mxx);
            myy = fma(g, bb, myy);
            mxy = fma(g, ab, mxy);
        }
        mom[0][r][c] = mx;
        mom[1][r][c] = my;
        mom[2][r][c] = mxx;
        mom[3][r][c] = myy;
        mom[4][r][c] = mxy;
    }
    __syncthreads();

    const int c = tid & 31;
    const int valid_h = H - (SSIM_WIN - 1), valid_w = W - (SSIM_WIN - 1);
    double acc = 0.0;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int r = (tid >> 5) + 8 * half;
        double mx = 0.0, my = 0.0, mxx = 0.0, myy = 0.0, mxy = 0.0;
#pragma unroll
        for (int k = 0; k < SSIM_WIN; ++k) {
            const double g = win.g[k];
            mx = fma(g, mom[0][r + k][c], mx);
            my = fma(g, mom[1][r + k][c], my);
            mxx = fma(g, mom[2][r + k][c], mxx);
            myy = fma(g, mom[3][r + k][c], myy);
            mxy = fma(g, mom[4][r + k][c], mxy);
        }
        const double c1 = 0.01 * 0.01, c2 = 0.03 * 0.03;
        const double mxmx = mx * mx, mymy = my * my, mxmy = mx * my;
        const double vx = mxx - mxmx, vy = myy - mymy, vxy = mxy - mxmy;
        const double s = ((2.0 * mxmy + c1) * (2.0 * vxy + c2)) / ((mxmx + mymy + c1) * (vx + vy + c2));
        if (ty0 + r < valid_h && tx0 + c < valid_w) acc += s;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) work[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ssim[b] = (sum of the image's `n` tile partials, in an order that depends on n alone) / count
__global__ __launch_bounds__(256) void ssim_finalize_kernel(const double* __restrict__ work, double* __restrict__ ssim,
                                                            int n, double count) {
    __shared__ double red[4];
    const double* w = work + (int64_t)blockIdx.x * n;
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) acc += w[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) ssim[blockIdx.x] = ((red[0] + red[1]) + (red[2] + red[3])) / count;
}

// ---------------------------------------------------------------- mean / standard deviation over K samples
// One 256-thread workgroup per STATS_ELEMS consecutive elements of one image; thread t owns the four elements
// 4 t .. 4 t + 3 of each 1024-element slab.  The vector path moves them as one 16-byte load per sample and one 16-byte
// store per result, the scalar path element by element with a bound check -- the same elements in the same order on the
// same thread, so both paths give the same bits.  Per element: v_k = clamp((x_k + 1) / 2, 0, 1) in fp32 (what
// finalize_psnr_kernel forms), then two passes in fp64 -- m = sum(v_k) / K, s = sqrt(sum((v_k - m)^2) / (K - 1)) -- over
// the K samples, re-read for the second pass (they are in cache: the thread just loaded them).  Deviations from the mean,
// never sum(v^2) - sum(v)^2 / K, which loses every digit of a small variance on a large mean.
constexpr int STATS_SLABS = 2;
constexpr int STATS_ELEMS = STATS_SLABS * 1024;

__device__ __forceinline__ float stats_unit(float v) {
    return fminf(fmaxf((v + 1.0f) / 2.0f, 0.0f), 1.0f);
}

template <bool VEC>
__global__ __launch_bounds__(256) void sample_stats_kernel(const float* __restrict__ x, int64_t image_stride,
                                                           int64_t sample_stride, const float* __restrict__ xo,
                                                           float* __restrict__ mean_img, float* __restrict__ std_img,
                                                           double* __restrict__ work, int K, int64_t chw, int nblk) {
#pragma clang fp contract(off)
    __shared__ double red[2][4];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;
    const float* xb = x + (int64_t)b * image_stride;
    const int64_t ob = (int64_t)b * chw;
    double acc_sse = 0.0, acc_std = 0.0;
#pragma unroll
    for (int slab = 0; slab < STATS_SLABS; ++slab) {
        const int64_t e0 = (int64_t)blk * STATS_ELEMS + slab * 1024 + tid * 4;
        if (e0 >= chw) continue;
        const int n = VEC ? 4 : (int)(chw - e0 < 4 ? chw - e0 : 4);
        double sum[4] = {0.0, 0.0, 0.0, 0.0}, ss[4] = {0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < K; ++k) {
            const float* p = xb + (int64_t)k * sample_stride + e0;
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (VEC) {
                const f32x4 q = *reinterpret_cast<const f32x4*>(p);
                v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
            } else {
                for (int j = 0; j < n; ++j) v[j] = p[j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) sum[j] += (double)stats_unit(v[j]);
        }
        double m[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) m[j] = sum[j] / (double)K;
        if (K > 1) {
            for (int k = 0; k < K; ++k) {
                const float* p = xb + (int64_t)k * sample_stride + e0;
                float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (VEC) {
                    const f32x4 q = *reinterpret_cast<const f32x4*>(p);
                    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
                } else {
                    for (int j = 0; j < n; ++j) v[j] = p[j];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double d = (double)stats_unit(v[j]) - m[j];
                    ss[j] += d * d;
                }
            }
        }
        float m32[4], s32[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double s = K > 1 ? sqrt(ss[j] / (double)(K - 1)) : 0.0;
            m32[j] = (float)m[j];
            s32[j] = (float)s;
            if (j < n) acc_std += s;
        }
        float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (xo) {
            if (VEC) {
                const f32x4 q = *reinterpret_cast<const f32x4*>(xo + ob + e0);
                o[0] = q.x, o[1] = q.y, o[2] = q.z, o[3] = q.w;
            } else {
                for (int j = 0; j < n; ++j) o[j] = xo[ob + e0 + j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float dd = m32[j] - stats_unit(o[j]);      // fp32, the convention of finalize_psnr_kernel
                if (j < n) acc_sse += (double)(dd * dd);
            }
        }
        if (VEC) {
            f32x4 qm, qs;
            qm.x = m32[0], qm.y = m32[1], qm.z = m32[2], qm.w = m32[3];
            qs.x = s32[0], qs.y = s32[1], qs.z = s32[2], qs.w = s32[3];
            *reinterpret_cast<f32x4*>(mean_img + ob + e0) = qm;
            *reinterpret_cast<f32x4*>(std_img + ob + e0) = qs;
        } else {
            for (int j = 0; j < n; ++j) {
                mean_img[ob + e0 + j] = m32[j];
                std_img[ob + e0 + j] = s32[j];
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        acc_sse += __shfl_xor(acc_sse, o);
        acc_std += __shfl_xor(acc_std, o);
    }
    if ((tid & 63) == 0) {
        red[0][tid >> 6] = acc_sse;
        red[1][tid >> 6] = acc_std;
    }
    __syncthreads();
    if (tid == 0) {
        work[2 * (int64_t)blockIdx.x] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        work[2 * (int64_t)blockIdx.x + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}

// sse_mean[b] = sum of the image's `n` squared-error partials, std_mean[b] = (sum of its std partials) / chw; the order
// depends on n alone
__global__ __launch_bounds__(256) void sample_stats_finalize_kernel(const double* __restrict__ work,
                                                                    double* __restrict__ sse_mean,
                                                                    double* __restrict__ std_mean, int n, double chw) {
    __shared__ double red[2][4];
    const double* w = work + 2 * (int64_t)blockIdx.x * n;
    double a0 = 0.0, a1 = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        a0 += w[2 * i];
        a1 += w[2 * i + 1];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a0 += __shfl_xor(a0, o);
        a1 += __shfl_xor(a1, o);
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = a0;
        red[1][threadIdx.x >> 6] = a1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (sse_mean) sse_mean[blockIdx.x] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        std_mean[blockIdx.x] = ((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) / chw;
    }
}

// ---------------------------------------------------------------- per-row residual norms of A x^ - y
// One 256-thread workgroup per CONS_ELEMS consecutive entries of one row; thread t owns the four entries 4 t .. 4 t + 3 of
// each 1024-entry slab, as in sample_stats_kernel.  Row b has n_b = counts ? counts[b] : m valid entries (clamped to
// [0, m]); nothing at or beyond n_b is read.  The vector path loads a thread's four entries of both operands with one
// 16-byte load each where all four are valid and goes element by element over a row's ragged tail; the scalar path goes
// element by element everywhere -- the same entries in the same order on the same thread, so both give the same bits.
// Workgroups past n_b write zero partials: the finalize pass adds the same ceil(m / CONS_ELEMS) partials whatever n_b is.
constexpr int CONS_SLABS = 2;
constexpr int CONS_ELEMS = CONS_SLABS * 1024;

template <bool VEC>
__global__ __launch_bounds__(256) void consistency_kernel(const float* __restrict__ ax, const float* __restrict__ y,
                                                          int64_t row_stride, const int32_t* __restrict__ counts,
                                                          double* __restrict__ work, int64_t m, int nblk) {
#pragma clang fp contract(off)
    __shared__ double red[3][4];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;
    int64_t nb = counts ? (int64_t)counts[b] : m;
    nb = nb < 0 ? 0 : (nb > m ? m : nb);
    const float* ap = ax + (int64_t)b * row_stride;
    const float* yp = y + (int64_t)b * row_stride;
    double acc_l1 = 0.0, acc_sse = 0.0, acc_max = 0.0;
#pragma unroll
    for (int slab = 0; slab < CONS_SLABS; ++slab) {
        const int64_t e0 = (int64_t)blk * CONS_ELEMS + slab * 1024 + tid * 4;
        if (e0 >= nb) continue;
        const int n = (int)(nb - e0 < 4 ? nb - e0 : 4);
        float va[4] = {0.0f, 0.0f, 0.0f, 0.0f}, vy[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (VEC && n == 4) {
            const f32x4 qa = *reinterpret_cast<const f32x4*>(ap + e0);
            const f32x4 qy = *reinterpret_cast<const f32x4*>(yp + e0);
            va[0] = qa.x, va[1] = qa.y, va[2] = qa.z, va[3] = qa.w;
            vy[0] = qy.x, vy[1] = qy.y, vy[2] = qy.z, vy[3] = qy.w;
        } else {
            for (int j = 0; j < n; ++j) {
                va[j] = ap[e0 + j];
                vy[j] = yp[e0 + j];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < n) {
                const double d = (double)va[j] - (double)vy[j];      // exact: both are fp32
                const double a = fabs(d);
                acc_l1 += a;
                acc_sse += d * d;
                acc_max = fmax(acc_max, a);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        acc_l1 += __shfl_xor(acc_l1, o);
        acc_sse += __shfl_xor(acc_sse, o);
        acc_max = fmax(acc_max, __shfl_xor(acc_max, o));
    }
    if ((tid & 63) == 0) {
        red[0][tid >> 6] = acc_l1;
        red[1][tid >> 6] = acc_sse;
        red[2][tid >> 6] = acc_max;
    }
    __syncthreads();
    if (tid == 0) {
        work[3 * (int64_t)blockIdx.x] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        work[3 * (int64_t)blockIdx.x + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
        work[3 * (int64_t)blockIdx.x + 2] = fmax(fmax(red[2][0], red[2][1]), fmax(red[2][2], red[2][3]));
    }
}

// l1[b], sse[b] = the sums of the row's `n` partials, in an order that depends on n alone; maxabs[b] = (float) of their max
// (the max of fp32 differences of fp32 values: |d| < 2^129 may round to inf, as the fp32 subtraction itself would)
__global__ __launch_bounds__(256) void consistency_finalize_kernel(const double* __restrict__ work, double* __restrict__ l1,
                                                                   double* __restrict__ sse, float* __restrict__ maxabs,
                                                                   int n) {
    __shared__ double red[3][4];
    const double* w = work + 3 * (int64_t)blockIdx.x * n;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        a0 += w[3 * i];
        a1 += w[3 * i + 1];
        a2 = fmax(a2, w[3 * i + 2]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a0 += __shfl_xor(a0, o);
        a1 += __shfl_xor(a1, o);
        a2 = fmax(a2, __shfl_xor(a2, o));
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = a0;
        red[1][threadIdx.x >> 6] = a1;
        red[2][threadIdx.x >> 6] = a2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        l1[blockIdx.x] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        sse[blockIdx.x] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
        maxabs[blockIdx.x] = (float)fmax(fmax(red[2][0], red[2][1]), fmax(red[2][2], red[2][3]));
    }
}

// workgroups per row: a function of m alone
int64_t cons_blocks(int64_t m) {
    return (m + CONS_ELEMS - 1) / CONS_ELEMS;
}

// workgroups per image: a function of chw alone, so that an image's partials do not depend on the batch around it
int64_t stats_blocks(int64_t chw) {
    return (chw + STATS_ELEMS - 1) / STATS_ELEMS;
}

bool aligned16(const void* p) {
    return ((uintptr_t)p & 15) == 0;
}

// g_i = exp(-(i-5)^2 / (2 * 1.5^2)) / sum, in fp64
ssim_window ssim_make_window() {
    ssim_window win;
    double sum = 0.0;
    for (int i = 0; i < SSIM_WIN; ++i) {
        win.g[i] = exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
        sum += win.g[i];
    }
    for (int i = 0; i < SSIM_WIN; ++i) win.g[i] /= sum;
    return win;
}

// tiles per plane, or 0 when the shape has no valid position
int64_t ssim_tiles(int32_t H, int32_t W, int* tiles_x) {
    if (H < SSIM_WIN || W < SSIM_WIN) return 0;
    const int64_t tx = (W - (SSIM_WIN - 1) + SSIM_TW - 1) / SSIM_TW, ty = (H - (SSIM_WIN - 1) + SSIM_TH - 1) / SSIM_TH;
    if (tiles_x) *tiles_x = (int)tx;
    return tx * ty;
}

}  // namespace

extern "C" int64_t ddnm_ssim_workspace_elems(int32_t B, int32_t C, int32_t H, int32_t W) {
    if (B <= 0 || C <= 0) return DDNM_E_BADARG;
    const int64_t tiles = ssim_tiles(H, W, nullptr);
    if (tiles == 0) return DDNM_E_SHAPE;
    const int64_t per_image = (int64_t)C * tiles;
    if (per_image > INT32_MAX || per_image * B > INT32_MAX) return DDNM_E_SHAPE;      // one workgroup per partial, 1-D grid
    return per_image * B;
}

extern "C" int ddnm_ssim_f32(const float* x, const float* y, double* ssim, double* work, int64_t work_elems, int32_t B,
                             int32_t C, int32_t H, int32_t W, int32_t transform, void* stream) {
    if (!x || !y || !ssim || !work || B <= 0 || C <= 0) return DDNM_E_BADARG;
    const int64_t need = ddnm_ssim_workspace_elems(B, C, H, W);
    if (need < 0) return (int)need;
    if (work_elems < need) return DDNM_E_SHAPE;
    int tiles_x = 0;
    const int tiles = (int)ssim_tiles(H, W, &tiles_x);
    static const ssim_window win = ssim_make_window();      // computed once
    hipStream_t st = (hipStream_t)stream;
    DDNM_LAUNCH(ssim_tile_kernel, dim3((unsigned)need), dim3(256), 0, st, x, y, work, H, W, tiles_x, tiles,
                transform != 0, win);
    const double count = (double)C * (double)(H - (SSIM_WIN - 1)) * (double)(W - (SSIM_WIN - 1));
    DDNM_LAUNCH(ssim_finalize_kernel, dim3(B), dim3(256), 0, st, work, ssim, C * tiles, count);
    return 0;
}

extern "C" int64_t ddnm_sample_stats_workspace_elems(int32_t B, int64_t chw) {
    if (B < 1 || chw < 1) return DDNM_E_BADARG;
    const int64_t nblk = stats_blocks(chw);
    if (nblk > INT32_MAX || nblk * B > INT32_MAX) return DDNM_E_SHAPE;      // one workgroup per partial pair, 1-D grid
    return 2 * nblk * B;
}

extern "C" int ddnm_sample_stats_f32(const float* x, int64_t image_stride, int64_t sample_stride, const float* x_orig,
                                     float* mean_img, float* std_img, double* sse_mean, double* std_mean, double* work,
                                     int64_t work_elems, int32_t B, int32_t K, int64_t chw, void* stream) {
    if (!x || !mean_img || !std_img || !std_mean || !work || B < 1 || K < 1 || chw < 1) return DDNM_E_BADARG;
    if ((x_orig != nullptr) != (sse_mean != nullptr)) return DDNM_E_BADARG;
    if (image_stride < 0 || sample_stride < 0) return DDNM_E_BADARG;
    const int64_t need = ddnm_sample_stats_workspace_elems(B, chw);
    if (need < 0) return (int)need;
    if (work_elems < need) return DDNM_E_SHAPE;
    const int nblk = (int)stats_blocks(chw);
    const bool vec = chw % 4 == 0 && image_stride % 4 == 0 && sample_stride % 4 == 0 && aligned16(x) &&
                     aligned16(x_orig) && aligned16(mean_img) && aligned16(std_img);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(need / 2));
    if (vec)
        DDNM_LAUNCH(sample_stats_kernel<true>, grid, dim3(256), 0, st, x, image_stride, sample_stride, x_orig, mean_img,
                    std_img, work, K, chw, nblk);
    else
        DDNM_LAUNCH(sample_stats_kernel<false>, grid, dim3(256), 0, st, x, image_stride, sample_stride, x_orig, mean_img,
                    std_img, work, K, chw, nblk);
    DDNM_LAUNCH(sample_stats_finalize_kernel, dim3(B), dim3(256), 0, st, work, sse_mean, std_mean, nblk, (double)chw);
    return 0;
}

extern "C" int64_t ddnm_consistency_workspace_elems(int32_t B, int64_t m) {
    if (B < 1 || m < 1) return DDNM_E_BADARG;
    const int64_t nblk = cons_blocks(m);
    if (nblk > INT32_MAX || nblk * B > INT32_MAX) return DDNM_E_SHAPE;      // one workgroup per partial triple, 1-D grid
    return 3 * nblk * B;
}

extern "C" int ddnm_consistency_f32(const float* ax, const float* y, int64_t row_stride, const int32_t* counts,
                                    double* l1, double* sse, float* maxabs, double* work, int64_t work_elems, int32_t B,
                                    int64_t m, void* stream) {
    if (!ax || !y || !l1 || !sse || !maxabs || !work || B < 1 || m < 1 || row_stride < m) return DDNM_E_BADARG;
    const int64_t need = ddnm_consistency_workspace_elems(B, m);
    if (need < 0) return (int)need;
    if (work_elems < need) return DDNM_E_SHAPE;
    if (counts) {
        // counts in memory the host can read as well (pinned or managed) are checked here; device memory is clamped by
        // the kernel.  Pageable host memory is refused: the kernel could not read it.
        hipPointerAttribute_t attr;
        const hipError_t e = hipPointerGetAttributes(&attr, counts);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return DDNM_E_BADARG;
        }
        if (attr.type == hipMemoryTypeUnregistered) return DDNM_E_BADARG;
        if (attr.type == hipMemoryTypeHost || attr.isManaged) {
            for (int32_t b = 0; b < B; ++b)
                if (counts[b] < 0 || counts[b] > m) return DDNM_E_SHAPE;
        }
    }
    const int nblk = (int)cons_blocks(m);
    const bool vec = row_stride % 4 == 0 && aligned16(ax) && aligned16(y);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(need / 3));
    if (vec)
        DDNM_LAUNCH(consistency_kernel<true>, grid, dim3(256), 0, st, ax, y, row_stride, counts, work, m, nblk);
    else
        DDNM_LAUNCH(consistency_kernel<false>, grid, dim3(256), 0, st, ax, y, row_stride, counts, work, m, nblk);
    DDNM_LAUNCH(consistency_finalize_kernel, dim3(B), dim3(256), 0, st, work, l1, sse, maxabs, nblk);
    return 0;
}
