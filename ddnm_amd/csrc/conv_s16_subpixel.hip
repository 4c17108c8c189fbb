// Sub-pixel form of `nearest x2 -> 3x3 convolution` (Upsample of the celeba `Model`, guided_diffusion/models.py:47-51 of the reference)
// in the split-fp16 arithmetic: four 2x2 convolutions on the LOW-resolution grid with pre-summed weights.
//
// Output pixel (2y + py, 2x + px) = sum_{a,b in {0,1}} Wp[py,px][a][b] . X[y + py - 1 + a][x + px - 1 + b], Wp = the 3x3 taps that the
// nearest upsample maps onto the same source pixel, summed on the host (ops.pack_upsample_conv_weight_s16).  Zero padding of
// the upsampled image is zero padding of X, so the identity holds at every border: 16 tap products per low-resolution pixel
// instead of the 36 the `d.ups` path of conv_s16_persist.hip issues -- 4/9 of the MFMA work.
//
// Structure of conv_s16_persist.hip (512 threads, 4 x 2 waves, 2 x 2 MFMA tiles per wave, 32-channel chunks, LDS-DMA weight
// tiles with look-ahead 2, deferred epilogue, XCD swizzle, one compile-time request table with counted waits), except:
//   * a tile is an 8 x 32 LOW-resolution patch (halo 10 x 34, raw operand staged with the per-image operand scale) times one
//     128-row n-tile = one row phase py and 64 output channels; rows [0, 64) are px = 0, rows [64, 128) px = 1, so wave
//     column wn IS px and both of a wave's n sub-tiles share their A fragments;
//   * a chunk is 4 steps (a, b): the wave reads its A fragments at halo offset ((py + a) * 34 + (px + b)) * LDH;
//   * 3 weight buffers and 4 steps per chunk: the buffer index is a run-time wave-uniform value (global step % 3), only the
//     waits are compile-time;
//   * a step's weight-tile DMA is the LAST request of its issue block, so the wait in front of step s counts the block of
//     step s - 1 alone: the 64 deferred stores fit three steps (22 / 21 / 21) under the 6-bit vmcnt and step 3 issues nothing
//     else, which keeps a chunk's table independent of its neighbours.  tests/test_isa_waits_subpixel.py replays the stream;
//   * low-resolution pixel (r, x), channel c, phase (py, px) -> out[img][2 (ty0 + r) + py][2 (tx0 + x) + px][c];
//   * GroupNorm partials: one row per (low-resolution m-tile, py, px) = Ho * Wo / 256 rows per image.
// Only instance: raw operand (bound required), bias, no per-sample addend / residual / GroupNorm prologue / shortcut.
#include <type_traits>

#include "s16_tile.h"

namespace {
constexpr int Q_STEPS = 4;
enum { Q_MID = 0, Q_LAST = 1, Q_FIRST = 2 };

// Requests a wave issues at step `s` of a chunk IN FRONT of the step's weight-tile DMA (W(s + 2), the last request of the step's
// issue block).  Every chunk: the next chunk's halo at step 0 (staged at steps 2 / 3).  FIRST chunk of a tile: the previous
// tile's 64 deferred stores over steps 0..2 (+ the statistics store at step 0).  LAST chunk: 2 bias loads + the next tile's
// operand bound at step 0.  Nothing at step 3, so a chunk's table does not depend on its neighbours.
constexpr int q_first_of(int s) { return s == 0 ? 0 : (s == 1 ? 22 : (s == 2 ? 43 : S16_NOUT)); }
constexpr int q_extra(int kind, int s) {
    return (s == 0 ? S16_HR : 0) + (kind == Q_FIRST ? q_first_of(s + 1) - q_first_of(s) + (s == 0 ? 1 : 0) : (kind == Q_LAST && s == 0 ? 3 : 0));
}
// vmcnt immediate of the wait in front of step `s`: everything issued behind W(s), the last request of step s - 2 -- the
// whole issue block of step s - 1 (its extras, then W(s + 1))
constexpr int q_wait(int kind, int s) { return S16_BR + (s >= 1 ? q_extra(kind, s - 1) : q_extra(kind, 3)); }
static_assert(q_extra(Q_FIRST, 3) == 0 && q_extra(Q_MID, 3) == 0 && q_extra(Q_LAST, 3) == 0, "step 3 issues its weight tile only");
static_assert(q_wait(Q_FIRST, 1) < 64 && q_wait(Q_FIRST, 2) < 64 && q_wait(Q_FIRST, 3) < 64 && q_wait(Q_LAST, 1) < 64, "vmcnt is a 6-bit field");

template <int V>
using ic = std::integral_constant<int, V>;
}  // namespace

__global__ __launch_bounds__(S16_NTHREADS, 1) void conv2x2x4_s16_subpixel_kernel(const ConvArgs p, const int total) {
    constexpr int WM = S16_WM, WN = S16_WN, MT = S16_MT, NT = S16_NT, BN = S16_BN, HR = S16_HR, LDH = S16_LDH, KCH = S16_KCH;
    constexpr int MAXH = S16_MAXH, HWd = S16_HWD, NWB = S16_NWB, WTILE = S16_WTILE, BR = S16_BR, NTHREADS = S16_NTHREADS;
    __shared__ __attribute__((aligned(1024))) char lds_all[NWB * WTILE + S16_HBYTES + WM * BN * 2 * 4];
    char* const Bs = lds_all;
    _Float16* const Hs = reinterpret_cast<_Float16*>(lds_all + NWB * WTILE);
    float* const stat_lds = reinterpret_cast<float*>(lds_all + NWB * WTILE + S16_HBYTES);

    const ddnm_conv_desc& d = p.d;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;             // wn = column phase px of the wave
    const int G = gridDim.x;
    const int per_img = (p.Hs * p.Ws) >> 8;               // low-resolution m-tiles per image
    const int Cout = d.Cout, Wo = d.Wo, Ho = d.Ho;        // output (high-resolution) extent: Ho = 2 Hs, Wo = 2 Ws

    // ---- tile bookkeeping (wave-uniform): n-tile = (64-channel block, py)
    int t_img, t_ty0, t_tx0, t_ntile, t_mtile;
    auto tile_of = [&](int v) {
        const int tile_id = xcd_swizzle(v, total);
        t_ntile = tile_id % p.n_tiles;
        t_mtile = tile_id / p.n_tiles;
        t_img = t_mtile / per_img;
        const int t = t_mtile - t_img * per_img;
        const int ty = t / p.tiles_x;
        t_ty0 = ty * 8;
        t_tx0 = (t - ty * p.tiles_x) * 32;
    };

    // ---- halo loader mapping: thread -> (16-byte column hc of 8, halo rows prow + 64 i); the source pixel of a slot is worked
    // out from the tile origin where it is requested (six slots per chunk: cheaper than six registers across the MFMA loop)
    const int hc = tid % S16_HCOLS, prow = tid / S16_HCOLS;
    auto halo_src = [&](int i) {
        const int row = prow + S16_HRPP * i;
        const int hy = row / HWd, hx = row - hy * HWd;
        const int iy = t_ty0 - 1 + hy, ix = t_tx0 - 1 + hx;
        const bool ok = row < MAXH && (unsigned)iy < (unsigned)p.Hs && (unsigned)ix < (unsigned)p.Ws;
        return ok ? (t_img * p.Hs + iy) * p.Ws + ix : -1;
    };

    // ---- weight tiles by LDS-DMA (s16_tile.h; a row holds 4 steps x Cin x [hi | lo])
    const int lrow = lane >> 3, lpiece = lane & 7;      // the lane's row / 16-byte piece within one LDS-DMA instruction
    const int wswz = S16_W_SWZ(wave, lrow);
    const unsigned w_rowlen = (unsigned)Q_STEPS * (unsigned)p.Cin * 4u;
    const __amdgpu_buffer_rsrc_t r_w = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(reinterpret_cast<const void*>(d.weight)), 0, (unsigned)p.n_tiles * BN * w_rowlen, 0x00020000);
    const unsigned w_lane = S16_W_LANE(wave * 8 + lrow, w_rowlen, lpiece, wswz);
    unsigned w_soff = 0;
    auto issue_w = [&](int chunk, int step, int buf) {
        s16_w_request<BR, NTHREADS / 64>(r_w, Bs + buf * WTILE + wave * 1024, w_lane, w_soff + ((unsigned)step * p.Cin + (unsigned)chunk * KCH) * 4u, w_rowlen);
    };

    const int nchunks = p.Cin / KCH;
    uint4 h_st[HR];
    constexpr unsigned HOOB = 0x80000000u;
    const __amdgpu_buffer_rsrc_t r_s0 = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(reinterpret_cast<const void*>(d.src0)), 0, (unsigned)d.B * p.Hs * p.Ws * d.C0 * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t r_s1 = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(reinterpret_cast<const void*>(d.C1 > 0 ? d.src1 : d.src0)), 0,
        (unsigned)d.B * p.Hs * p.Ws * (d.C1 > 0 ? d.C1 : d.C0) * 4, 0x00020000);
    // operand-range guard: one counted buffer load per wave and tile (s16_amax_request / s16_amax_scales)
    const __amdgpu_buffer_rsrc_t r_amax = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(reinterpret_cast<const void*>(d.amax_in)), 0, (unsigned)d.B * DDNM_AMAX_N * 4u, 0x00020000);
    unsigned amax_bits = 0;
    float ascale_stage = 1.f;
    auto prefetch_halo = [&](int chunk, bool live) {
        const int cb = chunk * KCH;
        const bool first = cb < d.C0;
        const unsigned cs = first ? d.C0 : d.C1, coff = first ? cb : cb - d.C0;
        const __amdgpu_buffer_rsrc_t r_s = first ? r_s0 : r_s1;
#pragma unroll
        for (int i = 0; i < HR; ++i) {
            const int ho = halo_src(i);
            const unsigned vo = (ho >= 0 && live) ? ((unsigned)ho * cs + hc * 4) * 4 : HOOB;
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r_s, vo, coff * 4, 0);
            h_st[i] = uint4{v.x, v.y, v.z, v.w};
        }
    };
    auto stage_halo_part = [&](int hbuf, int i0, int i1) {
#pragma unroll
        for (int i = 0; i < HR; ++i) {
            if (i < i0 || i >= i1) continue;
            const int row = prow + S16_HRPP * i;
            if (row < MAXH) split_store(&Hs[hbuf * MAXH * LDH + row * LDH + hc * 4], __builtin_bit_cast(f32x4, h_st[i]), ascale_stage);
        }
    };

    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    int a_off[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int m = (wm * MT + i) * 32 + (lane & 31);
        a_off[i] = ((m >> 5) * HWd + (m & 31) + wn) * LDH + (lane >> 5) * 8;          // + px: the wave's column phase
    }
    const int b_frag = S16_B_FRAG(wn * NT * 32, lane);
    int cur_py = 0;                                       // row phase of the tile in the MFMA loop
    // step (a, b) of the current chunk: weight buffer `buf` (run-time), halo buffer `hbuf`
    auto mfma_step = [&](int a, int b, int buf, int hbuf) {
        const int step_off = ((cur_py + a) * HWd + b) * LDH + hbuf * MAXH * LDH;
        s16_mfma_tile<MT, NT>(acc, Hs, a_off, step_off, Bs + buf * WTILE, b_frag);
    };

    // ---- output side: value k = (i * NT + j) * 16 + r of a lane is low-resolution row wm*MT + i, x = xr(r) + 4 (lane >> 5)
    // of the tile, channel j*32 + (lane & 31) of the n-tile's 64, phase (py of the tile, px = wn)
    const int ncol = lane & 31, rsel = 4 * (lane >> 5);
    const unsigned out_bytes = (unsigned)d.B * Ho * Wo * Cout * 4u;
    const __amdgpu_buffer_rsrc_t r_out = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(d.out), 0, out_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t r_bias = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(reinterpret_cast<const void*>(d.bias)), 0, d.bias ? (unsigned)Cout * 4u : 0u, 0x00020000);
    const __amdgpu_buffer_rsrc_t r_stats = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<void*>(d.stats_out), 0, d.stats_out ? (unsigned)p.m_tiles * 4u * Cout * 8u : 0u, 0x00020000);
    const unsigned o_lane = (unsigned)(((2 * wm * MT * Wo + 2 * rsel + wn) * Cout + ncol) * 4);
    auto o_soff = [&](unsigned base, int k) {
        const int i = k >> 5, j = (k >> 4) & 1, r = k & 15;
        return base + (unsigned)(((2 * i * Wo + 2 * ((r & 3) + 8 * (r >> 2))) * Cout + j * 32) * 4);
    };
    // n-tile nt = 2 * (64-channel block) + py
    auto tile_base = [&]() { return (unsigned)((((t_img * Ho + 2 * t_ty0 + (t_ntile & 1)) * Wo + 2 * t_tx0) * Cout + (t_ntile >> 1) * 64) * 4); };
    auto stats_base = [&]() { return (unsigned)((((t_mtile * 2 + (t_ntile & 1)) * 2) * Cout + (t_ntile >> 1) * 64) * 8); };
    const unsigned c_lane = (unsigned)(ncol * 4);
    // statistics: thread -> (n-tile row tid >> 1 = px * 64 + channel, sum / sum of squares); partial row (m-tile, py, px)
    const unsigned st_lane = tid < 2 * BN ? (unsigned)(((((tid >> 1) >> 6) * Cout + ((tid >> 1) & 63)) * 2 + (tid & 1)) * 4) : HOOB;

    float outv[S16_NOUT];
    float addv[NT];
#pragma unroll
    for (int k = 0; k < S16_NOUT; ++k) outv[k] = 0.f;
#pragma unroll
    for (int j = 0; j < NT; ++j) addv[j] = 0.f;
    unsigned pend_base = 0, pend_stats = 0;
    unsigned cur_base = 0, cur_stats = 0;
    float epi_cur = d.acc_scale;

    auto finalize = [&]() {
        s16_tile_finalize<S16_RES_NONE>(acc, outv, addv, epi_cur, stat_lds, wm, wn, lane);
        pend_base = cur_base;
        pend_stats = cur_stats;
    };
    auto store_stats = [&]() {                        // behind a barrier that follows finalize(): one store per wave
        s16_store_stats(stat_lds, tid, r_stats, st_lane, pend_stats);
    };

    // ---- first tile
    int v = blockIdx.x;
    tile_of(v);
    w_soff = (unsigned)t_ntile * BN * w_rowlen;
    cur_base = tile_base();
    cur_stats = stats_base();
    cur_py = t_ntile & 1;
    {
        float inv;
        s16_amax_scales(s16_amax_request(r_amax, lane, t_img, true), false, ascale_stage, inv);
        epi_cur = d.acc_scale * inv;
    }
    prefetch_halo(0, true);
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);                    // nothing but W(1) behind W(0): the first wait counts BR requests
    issue_w(0, 0, 0);
    issue_w(0, 1, 1);
    stage_halo_part(0, 0, HR);
    if (wave >= WM * WN / 2) __builtin_amdgcn_s_setprio(1);

    int hb = 0, wb = 0, n_img_next = 0, next_py = 0;     // wb = weight buffer of the step in front (global step % 3)
    bool have_next = false;
    float epi_next = epi_cur;
    unsigned next_base = 0, next_stats = 0, next_wsoff = 0;

    auto step_body = [&](auto KIND, auto STEP, int chunk) {
        constexpr int kind = decltype(KIND)::value, step = decltype(STEP)::value;
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(q_wait(kind, step)) : "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        // the next chunk's halo (LAST: the next tile's first chunk; t_img / t_ty0 / t_tx0 / ascale_stage already describe that tile)
        const bool live = kind == Q_LAST ? have_next : true;
        if constexpr (step == 0) prefetch_halo(kind == Q_LAST ? 0 : chunk + 1, live);
        if constexpr (step == 2) {
            if constexpr (kind == Q_LAST) {
                if (have_next) {
                    float inv;
                    s16_amax_scales(amax_bits, false, ascale_stage, inv);
                    epi_next = d.acc_scale * inv;
                }
            }
            if (live) stage_halo_part(hb ^ 1, 0, HR / 2);
        }
        if constexpr (step == 3) {
            if (live) stage_halo_part(hb ^ 1, HR / 2, HR);
        }
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        // extras, always the same number per (kind, step): q_extra()
        if constexpr (kind == Q_FIRST) {
            if constexpr (step == 0) store_stats();
#pragma unroll
            for (int k = q_first_of(step); k < q_first_of(step + 1); ++k)
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(outv[k]), r_out, o_lane, o_soff(pend_base, k), 0);
        }
        if constexpr (kind == Q_LAST && step == 0) {
            amax_bits = s16_amax_request(r_amax, lane, n_img_next, have_next);
#pragma unroll
            for (int j = 0; j < NT; ++j)
                addv[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r_bias, c_lane + j * 128, (unsigned)((t_ntile >> 1) * 64 * 4), 0));
        }
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        // weight tile of step + 2 into the buffer of step - 1, LAST request of the block; the LAST chunk's steps 2 / 3 request the
        // next tile's first two (without a next tile: a harmless re-request of this tile's, which keeps the stream uniform)
        const int nb = wb == 0 ? NWB - 1 : wb - 1;
        if constexpr (kind == Q_LAST && step >= 2) {
            if (step == 2 && have_next) w_soff = next_wsoff;
            issue_w(0, step - 2, nb);
        } else {
            issue_w(step + 2 < Q_STEPS ? chunk : chunk + 1, (step + 2) % Q_STEPS, nb);
        }
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        mfma_step(step >> 1, step & 1, wb, hb);
        wb = wb == NWB - 1 ? 0 : wb + 1;
    };
    auto run_chunk = [&](auto KIND, int chunk) {
        step_body(KIND, ic<0>{}, chunk);
        step_body(KIND, ic<1>{}, chunk);
        step_body(KIND, ic<2>{}, chunk);
        step_body(KIND, ic<3>{}, chunk);
        hb ^= 1;
    };

    // LAST chunk: the bias loads address THIS tile (t_ntile), the halo prefetch the NEXT one
    auto run_last = [&]() {
        const int vn = v + G;
        have_next = vn < total;
        const int c_ntile = t_ntile;
        if (have_next) {
            tile_of(vn);
            next_wsoff = (unsigned)t_ntile * BN * w_rowlen;
            next_base = tile_base();
            next_stats = stats_base();
            next_py = t_ntile & 1;
            n_img_next = t_img;
        }
        const int n_ntile = t_ntile;
        t_ntile = c_ntile;
        run_chunk(ic<Q_LAST>{}, nchunks - 1);
        t_ntile = n_ntile;
    };

    bool pending = false;
    for (;;) {
        int c0 = 0;
        if (pending) {
            run_chunk(ic<Q_FIRST>{}, 0);
            c0 = 1;
        }
        for (int chunk = c0; chunk < nchunks - 1; ++chunk) run_chunk(ic<Q_MID>{}, chunk);
        run_last();
        finalize();
        if (!have_next) break;
        v += G;
        cur_base = next_base;
        cur_stats = next_stats;
        cur_py = next_py;
        epi_cur = epi_next;
        pending = true;
    }
    // ---- the last tile's values leave directly
    __syncthreads();
    store_stats();
#pragma unroll
    for (int k = 0; k < S16_NOUT; ++k) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(outv[k]), r_out, o_lane, o_soff(pend_base, k), 0);
}

// CU count of the current device, queried once per device (shared by the persistent launchers)
int conv_persist_grid_cus() {
    constexpr int MAXDEV = 64;
    static int cached[MAXDEV];                           // 0: not queried yet (plain ints: a racing first query writes the same value)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAXDEV) return 256;
    int cus = cached[dev];
    if (cus <= 0) {
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        cus -= cus % 8;                                   // the XCD-contiguous tile order wants a multiple of 8 workgroups
        if (cus <= 0) cus = 8;
        cached[dev] = cus;
    }
    return cus;
}

bool conv3x3_s16_ups_subpixel_ok(const ddnm_conv_desc* d) {
    if (!d || !d->ups || d->ksize != 3 || d->stride != 1 || d->pad != 1 || d->Ho != d->Hin || d->Wo != d->Win) return false;
    if (d->B <= 0 || d->Hin <= 0 || d->Win <= 0 || ((d->Hin | d->Win) & 1)) return false;
    const int hs = d->Hin / 2, ws = d->Win / 2, cin = d->C0 + d->C1;
    if (ws % 32 || hs % 8 || d->C0 <= 0 || d->C1 < 0 || cin % S16_KCH || d->C0 % S16_KCH || cin / S16_KCH < 2 || d->Cout <= 0 || d->Cout % 64) return false;
    if (d->src_f16 || d->out_nchw || d->res || d->res_ups || d->badd || d->gn_scale || d->skip0) return false;
    if (!conv_sizes_addressable(d)) return false;
    const int64_t lim = (int64_t)1 << 31;
    // output / statistics / phase-packed weights (4 Cout rows of 4 steps) are addressed with 32-bit byte offsets
    return (int64_t)d->B * d->Ho * d->Wo * d->Cout * 4 < lim && (int64_t)d->B * (d->Ho * d->Wo / 256) * d->Cout * 8 < lim &&
           (int64_t)4 * d->Cout * Q_STEPS * cin * 4 < lim && (int64_t)d->B * hs * ws / 256 * (d->Cout / 32) < lim;
}

int conv3x3_s16_ups_subpixel_run(const ddnm_conv_desc* d, hipStream_t s) {
    if (!d || !d->src0 || !d->weight || !d->out || !d->amax_in || !(d->acc_scale > 0.f)) return DDNM_E_BADARG;
    if (d->C1 > 0 && !d->src1) return DDNM_E_BADARG;
    if (!conv3x3_s16_ups_subpixel_ok(d)) return DDNM_E_SHAPE;
    // M tiles of 256 source pixels = 1024 output pixels; n_tiles counts (64-channel block, py) pairs of 128 rows each
    const ConvArgs p = conv_args(*d, 1024, d->Cout / 32, 32, 5, d->Win / 2 / 32, Q_STEPS, 1);
    const int total = p.m_tiles * p.n_tiles;
    const int cus = conv_persist_grid_cus();
    DDNM_LAUNCH(conv2x2x4_s16_subpixel_kernel, dim3(total < cus ? total : cus), dim3(S16_NTHREADS), 0, s, p, total);
    return 0;
}
