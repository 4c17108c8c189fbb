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
