// The tile pieces of the split-fp16 convolution kernels, once (gfx950): conv_igemm_f16.hip <.., SPLIT> (one tile per
// workgroup), conv_s16_persist.hip, conv_s16_subpixel.hip, conv_gather_s16.hip, conv1x1_s16.hip and conv_s16_wslice.hip.  The bit identity of those kernels
// (tests/test_gpu_s16*.py) is the identity of these functions; what stays in a kernel is its main loop: the request
// stream and its tables, every wait / barrier / scheduling fence, the deferred stores.
// Plain force-inlined functions over the kernel's own arrays and registers (taken by reference): no state of their own.
// A scalar taken as `const T&` is one the kernel's lambda used to read through its capture: by value the compiler moves the
// arithmetic on it across the LDS-DMA requests and the kernels' instruction streams change (profiles/s16_tile_pieces.md).
#pragma once
#include "conv_common.h"

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// ---- geometry of the 8 x 32 pixel x 128 channel tile: 512 threads = 4 x 2 waves of 2 x 2 MFMA tiles (the three halo-form
// kernels; the one-tile kernel derives its values from its template parameters and asserts that <4,2,2,2> lands here)
constexpr int S16_WM = 4, S16_WN = 2, S16_MT = 2, S16_NT = 2;
constexpr int S16_NTHREADS = S16_WM * S16_WN * 64, S16_BN = S16_WN * S16_NT * 32;
constexpr int S16_KCH = 32;                           // channels per chunk
constexpr int S16_LDH = 72;                           // LDS operand row pitch in halfs: [hi 32 | lo 32 | pad 8] = 144 B
constexpr int S16_MAXH = 340, S16_HWD = 34;           // halo 10 x 34
constexpr int S16_HCOLS = 8;                          // 16-byte loads per halo row of one chunk
constexpr int S16_HRPP = S16_NTHREADS / S16_HCOLS;    // halo rows per pass of the workgroup
constexpr int S16_HR = (S16_MAXH + S16_HRPP - 1) / S16_HRPP, S16_HSPLIT = (S16_HR + 1) / 2;      // halo row slots per thread
constexpr int S16_BR = S16_BN / (S16_NTHREADS / 8);   // LDS-DMA instructions per wave and weight tile
constexpr int S16_NWB = 3;                            // weight tiles in LDS (step, step + 1, step + 2)
constexpr int S16_WTILE = S16_BN * 128;               // bytes of one weight tile
constexpr int S16_HBYTES = 2 * S16_MAXH * S16_LDH * 2;      // halo, double-buffered
constexpr int S16_NOUT = S16_MT * S16_NT * 16;        // output values per lane and tile
constexpr unsigned S16_OOB = 0x80000000u;             // buffer offset that fetches zero / stores nothing (tensors are < 2 GB)

// ---- weight tile [rows][hi 32 | lo 32] (128 B per row) by LDS-DMA, and its fragment reads.  One instruction moves 8 rows
// x 128 B as a lane-linear image: lane -> (row 8 wave + lrow (+ 8 NWAVES j), 16-byte piece lpiece), lrow = lane >> 3, lpiece =
// lane & 7.  Bank conflicts of the fragment reads are removed by an XOR swizzle of the piece index with (row >> 1) & 7,
// applied on BOTH sides:
//   write side: the lane FETCHES piece lpiece ^ swizzle(row) of its row, so the linear image holds the swizzled layout; for
//               the rows of a wave (row >> 1) & 7 = 4 (wave & 1) + (lrow >> 1) whatever j       (S16_W_SWZ, S16_W_LANE)
//   read side:  the B fragment of piece q (+ lane >> 5) of row n = row0 + (lane & 31) (+ 32 j) sits at piece
//               (q + (lane >> 5)) ^ ((n >> 1) & 7), (n >> 1) & 7 = ((lane & 31) >> 1) & 7; the piece pair 2 ks enters as
//               an XOR of bits 5-6 of the byte address                                      (S16_B_FRAG, s16_mfma_tile)
// Expression macros, not functions: these sit in the kernels' prologues, where hipcc folds them with the kernel's other
// lane arithmetic BEFORE it inlines any function -- as functions they change the instruction streams of all four kernels
// (profiles/s16_tile_pieces.md).  S16_W_LANE: the lane's buffer offset, `row` = its row of the packed weights (rowlen bytes).
#define S16_W_SWZ(wave, lrow) ((((wave) & 1) << 2) | ((lrow) >> 1))
#define S16_W_LANE(row, rowlen, lpiece, wswz) ((unsigned)(row) * (rowlen) + (unsigned)(((lpiece) ^ (wswz)) * 16))
#define S16_B_FRAG(row0, lane) ((((row0) + ((lane) & 31)) * 128) + (((((lane) >> 5) ^ ((((lane) & 31) >> 1) & 7))) << 4))
// the BR requests of one wave; `dst` = LDS address of the tile + wave * 1024, `so` = scalar byte offset of the (tap, chunk) column
template <int BR, int NWAVES>
__device__ __forceinline__ void s16_w_request(const __amdgpu_buffer_rsrc_t& r_w, char* dst, const unsigned& w_lane, unsigned so,
                                              const unsigned& rowlen) {
#pragma unroll
    for (int j = 0; j < BR; ++j)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(r_w, (__attribute__((address_space(3))) void*)(dst + j * NWAVES * 1024), 16, w_lane,
                                                 so + (unsigned)j * (NWAVES * 8) * rowlen, 0, 0);
}

// ---- one K chunk of one tap: acc += A . B over 32 channels as three products per term.  [hi 32 | lo 32] rows: k-step ks
// reads the hi fragment at ks*16 and the lo fragment 32 halfs behind it; the three products of one (i, j) tile are spread
// over the loop so that no MFMA waits on its predecessor.  A fragment i at a + a_off[i] + off (halfs), B tile at bf.
template <int MT, int NT>
__device__ __forceinline__ void s16_mfma_tile(f32x16 (&acc)[MT][NT], const _Float16* const& a, const int (&a_off)[MT], int off, const char* bf,
                                              const int& b_frag) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        half8 ah[MT], al[MT], bh[NT], bl[NT];
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            ah[i] = *reinterpret_cast<const half8*>(a + a_off[i] + off + ks * 16);
            al[i] = *reinterpret_cast<const half8*>(a + a_off[i] + off + ks * 16 + 32);
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            bh[j] = *reinterpret_cast<const half8*>(bf + ((b_frag ^ (ks << 5)) + j * 32 * 128));
            bl[j] = *reinterpret_cast<const half8*>(bf + ((b_frag ^ ((ks + 2) << 5)) + j * 32 * 128));
        }
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bh[j], acc[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bl[j], acc[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
    }
}

// ---- operand bound as ONE buffer load per wave (the persistent forms, whose request stream must stay countable: the
// scalar loads of s16_operand_scale would become vector loads there -- these kernels store, so nothing is provably
// unclobbered -- in a number the compiler chooses): lane l < DDNM_AMAX_N fetches word l of image `img`; the maximum is a
// wave reduction on the bit patterns, the scale conv_common.h::s16_scale_from_bound
__device__ __forceinline__ unsigned s16_amax_request(const __amdgpu_buffer_rsrc_t r_amax, int lane, int img, bool live) {
    return __builtin_amdgcn_raw_buffer_load_b32(r_amax, (lane < DDNM_AMAX_N && live) ? (unsigned)lane * 4u : S16_OOB,
                                                (unsigned)img * DDNM_AMAX_N * 4u, 0);
}
__device__ __forceinline__ void s16_amax_scales(unsigned m, bool down_only, float& scale, float& inv_scale) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned t = (unsigned)__shfl_xor((int)m, o);
        m = t > m ? t : m;
    }
    s16_scale_from_bound(__builtin_amdgcn_readfirstlane(m), down_only, scale, inv_scale);
}

// ---- tile end of the persistent forms, register work only: scale, bias (+ residual, already in outv); per-channel partial
// sums for the consumer's GroupNorm in the summation order of conv_epilogue (per channel column i-major over the wave's
// rows, halves combined, waves in order); the accumulators are reset.  Value k = (i NT + j) 16 + r of a lane.
// RES: S16_RES_TILE = the residual tile is in outv; S16_RES_ZERO = the 3x3 form without residual adds the literal 0 that
// conv_epilogue adds (-0 -> +0: part of its bit identity with the one-tile kernel); S16_RES_NONE = no term (sub-pixel form).
enum { S16_RES_NONE = 0, S16_RES_ZERO = 1, S16_RES_TILE = 2 };
template <int RES>
__device__ __forceinline__ void s16_tile_finalize(f32x16 (&acc)[S16_MT][S16_NT], float (&outv)[S16_NOUT], const float (&addv)[S16_NT],
                                                  float epi, float* stat_lds, int wm, int wn, int lane) {
    constexpr int MT = S16_MT, NT = S16_NT, BN = S16_BN;
    float cs[NT], cq[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        cs[j] = cq[j] = 0.f;
        const float add = addv[j];
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = (i * NT + j) * 16 + r;
                float v = acc[i][j][r] * epi + add;
                if constexpr (RES != S16_RES_NONE) v = v + (RES == S16_RES_TILE ? outv[k] : 0.f);
                outv[k] = v;
                cs[j] += v;
                cq[j] = __builtin_fmaf(v, v, cq[j]);
                acc[i][j][r] = 0.f;
            }
        cs[j] += __shfl_xor(cs[j], 32);
        cq[j] += __shfl_xor(cq[j], 32);
    }
    if (lane < 32) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int c = (wn * NT + j) * 32 + lane;
            stat_lds[(wm * BN + c) * 2 + 0] = cs[j];
            stat_lds[(wm * BN + c) * 2 + 1] = cq[j];
        }
    }
}
// behind a barrier that follows s16_tile_finalize: thread -> (row tid >> 1 of the n-tile, sum / sum of squares), one store per wave
__device__ __forceinline__ void s16_store_stats(const float* stat_lds, int tid, const __amdgpu_buffer_rsrc_t r_stats, unsigned st_lane,
                                                unsigned st_soff) {
    const int c = (tid >> 1) & (S16_BN - 1), which = tid & 1;
    float a = 0.f;
#pragma unroll
    for (int w = 0; w < S16_WM; ++w) a += stat_lds[(w * S16_BN + c) * 2 + which];
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(a), r_stats, st_lane, st_soff, 0);
}

// Sum and sum of squares of the four pixels p0..p3 of one statistics tile, in the order conv_splitk_reduce_stats_kernel takes
// them: its 256 threads are `rows` pixel rows of Cout / 4 channel columns; row r adds the pixels r, r + rows, ... (squares by
// fma), then the rows are added in order.  No contraction here: where that kernel rounds a square by itself, so does this.
__device__ __forceinline__ void s16_quad_stats(float p0, float p1, float p2, float p3, int rows, float& s, float& q) {
#pragma clang fp contract(off)
    if (rows >= 4) {
        s = ((p0 + p1) + p2) + p3;
        q = ((p0 * p0 + p1 * p1) + p2 * p2) + p3 * p3;
    } else if (rows == 3) {
        s = ((p0 + p3) + p1) + p2;
        q = (__builtin_fmaf(p3, p3, p0 * p0) + p1 * p1) + p2 * p2;
    } else if (rows == 2) {
        s = (p0 + p2) + (p1 + p3);
        q = __builtin_fmaf(p2, p2, p0 * p0) + __builtin_fmaf(p3, p3, p1 * p1);
    } else {
        s = ((p0 + p1) + p2) + p3;
        q = __builtin_fmaf(p3, p3, __builtin_fmaf(p2, p2, __builtin_fmaf(p1, p1, p0 * p0)));
    }
}
