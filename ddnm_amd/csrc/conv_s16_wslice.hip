// 3x3 / stride 1 / pad 1 convolution of the 8 x 8 level in the split-fp16 arithmetic (fp32-grade products on
// v_mfma_f32_32x32x16_f16), gfx950, with the plan's split-K slices on the WAVES of one workgroup.
//
// conv_gather_s16.hip runs these launches (512 / 1024 -> 512 channels, 64 pixels per image) as ksplit = 8 workgroups per
// output tile that each write an fp32 slab, and a second launch that adds the slabs.  Every (chunk, tap) step there gathers
// the A tile from global memory again and applies GroupNorm, swish and the hi / lo split to it between two workgroup
// barriers: nine times per chunk, once per tap.  Here one workgroup of 8 waves owns an output tile of 64 pixels (an 8 x 8
// patch: the whole image at this level) x 32 channels, and wave w computes the plan's K slice w -- chunks
// [nchunks w / ksplit, nchunks (w + 1) / ksplit) -- over the whole tile:
//   A: the wave stages the 10 x 10 halo of ITS 32-channel chunk once per chunk into a wave-private LDS region (100 rows at
//      the 144-byte pitch: one global read, one GroupNorm + swish + split per element and chunk); the nine taps read it at
//      shifted row offsets; zero padding is the out-of-range buffer offset.  The halo of the next chunk is requested into
//      registers while the taps of the current one are multiplied.
//   B: nobody else reads a wave's weights.  The tile [32 rows][hi 32 | lo 32] of step (chunk, tap) is requested two steps
//      ahead into registers as whole 128-byte rows (8 lanes per row: coalesced), written to the wave's own 4 KB of LDS in
//      the family's swizzled image when its step comes, and read back as fragments by s16_mfma_tile.  (Fragments fetched
//      straight from global memory -- 16 bytes per lane from 32 different rows -- were built first: about 60 clocks of
//      address processing per instruction, 0.8 us per step with 8 waves on the CU; tools/experiments/HISTORY.md.)
//   All requests have register destinations, so the compiler counts the waits (`s_waitcnt vmcnt(N)`) itself; scheduling
//   fences keep the requests where they are written.  No workgroup barrier in the main loop: a wave's slice shares nothing
//   with the other waves, and the LDS operations of one wave complete in order.
//   Reduction: the accumulators meet in LDS (one slab per slice, over the halos, behind a barrier) and are added in slice
//      order from slice 0; bias / badd / residual in the association of the reduction launch this replaces
//      (conv_splitk_reduce_stats_kernel with statistics, conv_splitk_reduce_kernel without), whose 4-pixel statistics tiles
//      are emitted in its order (s16_quad_stats).  No slabs in global memory, no second launch, no atomics.
// Same products in the same order per output element as the gather route (chunk, tap, k-step, lo.hi / hi.lo / hi.hi), so
// output and statistics equal that route's bit for bit (tests/test_gpu_s16_wslice.py, tests/test_gpu_runner_replay.py).
#include "s16_tile.h"

constexpr int WS_WAVES = 8, WS_NTHREADS = WS_WAVES * 64;
constexpr int WS_BM = 64, WS_BN = 32;                 // tile: an 8 x 8 patch x 32 output channels (128 workgroups at B = 8)
constexpr int WS_HW = 10, WS_HROWS = WS_HW * WS_HW;   // halo of the patch
constexpr int WS_HSLOTS = (WS_HROWS + 7) / 8;         // halo rows per lane (8 lanes x float4 = one 32-channel row)
constexpr int WS_HALO = WS_HROWS * S16_LDH;           // halfs of one wave's halo
constexpr int WS_WTILE = WS_BN * 128;                 // bytes of one wave's weight tile
constexpr int WS_BR = WS_BN / 8;                      // weight requests per step: 8 rows each
constexpr int WS_NB = 3;                              // weight register sets: step, step + 1, step + 2
constexpr int WS_SP = WS_BN + 8;                      // slab row pitch in floats: lanes 32-63 (4 rows further) land 32 banks away
constexpr int WS_SLAB = WS_BM * WS_SP;
constexpr int WS_LDS_MAIN = WS_WAVES * (WS_HALO * 2 + WS_WTILE), WS_LDS_RED = WS_WAVES * WS_SLAB * 4;
constexpr int WS_LDS = WS_LDS_MAIN > WS_LDS_RED ? WS_LDS_MAIN : WS_LDS_RED;
static_assert(WS_LDS <= 160 * 1024, "LDS of one CU");

__global__ __launch_bounds__(WS_NTHREADS) void conv_s16_wslice_kernel(const ConvArgs p) {
    constexpr int MT = 2, NT = 1, BN = WS_BN, SP = WS_SP, SLAB = WS_SLAB;
    // ONE shared object: [8 halos | 8 weight tiles], the slabs of the reduction over them
    __shared__ __attribute__((aligned(1024))) char lds_all[WS_LDS];

    const ddnm_conv_desc& d = p.d;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // scalar: the slice's chunks select descriptors and scalar offsets
    const int tile_id = xcd_swizzle(blockIdx.x, gridDim.x);
    const int n_tile = tile_id % p.n_tiles, m_tile = tile_id / p.n_tiles;      // (weights-major order measured: no difference)
    const int per_img = p.tiles_x * (d.Ho >> 3);
    const int img = m_tile / per_img, t_in_img = m_tile - img * per_img;
    const int ty0 = (t_in_img / p.tiles_x) << 3, tx0 = (t_in_img % p.tiles_x) << 3;
    float ascale, inv_ascale;
    s16_operand_scale(d.gn_scale == nullptr ? d.amax_in : nullptr, img, false, ascale, inv_ascale);

    // ---- B: request j of a step fetches rows 8 j + lrow of the tile, lane -> (row, 16-byte piece) as in s16_tile.h: the lane
    // FETCHES piece lpiece ^ swizzle(row), so that the lane-linear image it writes to LDS holds the swizzled layout that
    // S16_B_FRAG / s16_mfma_tile read; swizzle(row) = (row >> 1) & 7 = 4 (j & 1) + (lrow >> 1).
    // Split packing: a row is 9 Cin 4 bytes, (tap, chunk) starts at (tap Cin + 32 chunk) 4 bytes of it.
    const int lrow = lane >> 3, lpiece = lane & 7;
    const unsigned w_rowlen = 9u * (unsigned)p.Cin * 4u;
    const int cout_pad = (d.Cout + 127) / 128 * 128;
    const __amdgpu_buffer_rsrc_t r_w = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(reinterpret_cast<const void*>(d.weight)), 0, (unsigned)cout_pad * w_rowlen, 0x00020000);
    unsigned w_voff[2];                               // even / odd request
#pragma unroll
    for (int o = 0; o < 2; ++o) w_voff[o] = S16_W_LANE(n_tile * BN + lrow, w_rowlen, lpiece, (o << 2) | (lrow >> 1));
    auto load_b = [&](int chunk, int tap, u32x4 (&b)[WS_BR]) {
        const unsigned so = ((unsigned)tap * (unsigned)p.Cin + (unsigned)chunk * S16_KCH) * 4u;
#pragma unroll
        for (int j = 0; j < WS_BR; ++j)
            b[j] = __builtin_amdgcn_raw_buffer_load_b128(r_w, w_voff[j & 1], so + (unsigned)j * 8u * w_rowlen, 0);
    };
    char* const wtile = lds_all + WS_WAVES * WS_HALO * 2 + wave * WS_WTILE;      // wave-private
    auto stage_b = [&](const u32x4 (&b)[WS_BR]) {
#pragma unroll
        for (int j = 0; j < WS_BR; ++j) *reinterpret_cast<u32x4*>(wtile + j * 1024 + lane * 16) = b[j];
    };
    const int b_frag = S16_B_FRAG(0, lane);

    // ---- A: halo row r = (lane >> 3) + 8 i of the patch, float4 column c4 of the chunk
    const bool has_gn = d.gn_scale != nullptr;
    const int c4 = lane & 7, hr0 = lane >> 3;
    const __amdgpu_buffer_rsrc_t r_s0 = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(d.src0), 0, (unsigned)d.B * d.Hin * d.Win * d.C0 * 4u, 0x00020000);
    const __amdgpu_buffer_rsrc_t r_s1 = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(d.C1 > 0 ? d.src1 : d.src0), 0, (unsigned)d.B * d.Hin * d.Win * (d.C1 > 0 ? d.C1 : d.C0) * 4u, 0x00020000);
    int hpix[WS_HSLOTS];                              // pixel of the halo row, flat over the batch; -1: padding (or no row)
#pragma unroll
    for (int i = 0; i < WS_HSLOTS; ++i) {
        const int r = hr0 + 8 * i;
        const int hy = (r * 205) >> 11, hx = r - hy * WS_HW;      // r / 10, r % 10 (r < 104)
        const int iy = ty0 + hy - 1, ix = tx0 + hx - 1;
        const bool ok = r < WS_HROWS && (unsigned)iy < (unsigned)d.Hin && (unsigned)ix < (unsigned)d.Win;
        hpix[i] = ok ? (img * d.Hin + iy) * d.Win + ix : -1;
    }
    struct Halo {
        f32x4 v[WS_HSLOTS], gsc, gsh;
    };
    auto prefetch_a = [&](int chunk, Halo& h) {
        const int cb = chunk * S16_KCH;
        const bool first = cb < d.C0;                 // C0 % 32 == 0: a chunk lies in one source (wave-uniform select)
        const unsigned cs = first ? d.C0 : d.C1, coff = first ? cb : cb - d.C0;
        const __amdgpu_buffer_rsrc_t r_s = first ? r_s0 : r_s1;
#pragma unroll
        for (int i = 0; i < WS_HSLOTS; ++i) {
            const unsigned vo = hpix[i] >= 0 ? ((unsigned)hpix[i] * cs + c4 * 4) * 4u : S16_OOB;
            h.v[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r_s, vo, coff * 4u, 0));
        }
        if (has_gn) {
            h.gsc = *reinterpret_cast<const f32x4*>(d.gn_scale + (size_t)img * p.Cin + cb + c4 * 4);
            h.gsh = *reinterpret_cast<const f32x4*>(d.gn_shift + (size_t)img * p.Cin + cb + c4 * 4);
        }
    };
    _Float16* const halo = reinterpret_cast<_Float16*>(lds_all) + wave * WS_HALO;      // wave-private
    auto stage_a = [&](const Halo& h) {
#pragma unroll
        for (int i = 0; i < WS_HSLOTS; ++i) {
            f32x4 v = h.v[i];
            if (has_gn && hpix[i] >= 0) v = gn_act(v, h.gsc, h.gsh, d.gn_silu);
            if (hr0 + 8 * i < WS_HROWS) split_store(&halo[(hr0 + 8 * i) * S16_LDH + c4 * 4], v, ascale);
        }
    };

    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // wave = slice of the plan (2 <= p.ksplit <= WS_WAVES, conv3x3_s16_wslice_routes); a wave beyond the plan's slices has no chunks
    const int nchunks = p.Cin / S16_KCH, ksplit = p.ksplit;
    const int c_begin = wave < ksplit ? (int)((long)nchunks * wave / ksplit) : 0;
    const int c_end = wave < ksplit ? (int)((long)nchunks * (wave + 1) / ksplit) : 0;
    // pixel m = 32 i + (lane & 31) of the patch is halo row (m >> 3) 10 + (m & 7) at tap (0, 0); tap (ky, kx): ky 10 + kx rows on
    const _Float16* const a_frag = halo + (((lane & 31) >> 3) * WS_HW + (lane & 7)) * S16_LDH + (lane >> 5) * 8;

    if (c_begin < c_end) {
        Halo h;
        u32x4 b[WS_NB][WS_BR];
        prefetch_a(c_begin, h);
        load_b(c_begin, 0, b[0]);
        load_b(c_begin, 1, b[1]);
        for (int c = c_begin; c < c_end; ++c) {
            // the taps of chunk c - 1 have read the halo (LDS operations of one wave complete in order)
            stage_a(h);
            const bool more = c + 1 < c_end;
            // (the last chunk requests its own first two steps again, 8 KB that nobody reads: a guard on `more` would put two
            // branches into the tap sequence, whose waits the compiler then merges over both arms)
            const int cn = more ? c + 1 : c;
            if (more) prefetch_a(cn, h);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {       // (9 % WS_NB == 0: the register set of a tap is the same in every chunk)
                const int t2 = tap + 2 < 9 ? tap + 2 : tap + 2 - 9;
                load_b(tap + 2 < 9 ? c : cn, t2, b[(tap + 2) % WS_NB]);
                stage_b(b[tap % WS_NB]);              // behind the fragment reads of the step before
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_sched_barrier(0);
                int a_rows[MT];
#pragma unroll
                for (int i = 0; i < MT; ++i) a_rows[i] = i * 4 * WS_HW * S16_LDH;
                s16_mfma_tile<MT, NT>(acc, a_frag, a_rows, ((tap / 3) * WS_HW + tap % 3) * S16_LDH, wtile, b_frag);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }

    // ---- reduction through LDS: slab `wave` = the accumulators of slice `wave`, [pixel][channel] at pitch SP.
    // C/D map of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    float* const slabs = reinterpret_cast<float*>(lds_all);
    __syncthreads();                                  // every wave is done with its halo (and has no request in flight: registers only)
    if (wave < ksplit) {
        float* const mine = slabs + wave * SLAB;
        const int rsel = 4 * (lane >> 5);
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    mine[(i * 32 + (r & 3) + 8 * (r >> 2) + rsel) * SP + j * 32 + (lane & 31)] = acc[i][j][r];
    }
    __syncthreads();

    // ---- epilogue: thread -> channel nl of the tile, pixel quads q0 + (512 / BN) k; four consecutive pixels of the patch row =
    // one statistics tile of the reduction pass.  Terms in that pass's association (conv1x1_s16.hip does the same).
    const float epi = d.acc_scale * inv_ascale;
    const int nl = tid % BN, q0 = tid / BN;
    const int n = n_tile * BN + nl;
    const float bias = d.bias ? d.bias[n] : 0.f, badd = d.badd ? d.badd[(size_t)img * d.badd_stride + n] : 0.f;
    const float* __restrict__ res = d.res;
    float* __restrict__ out = d.out;
    const int rows = 256 / (d.Cout >> 2);             // pixel rows of the reduction pass's workgroup
    unsigned o[NT][4], pixq[NT];
    float rv[NT][4];
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        const int m0 = (q0 + (WS_NTHREADS / BN) * k) * 4;
        const unsigned pix0 = pixq[k] = (unsigned)((img * d.Ho + ty0 + (m0 >> 3)) * d.Wo + tx0 + (m0 & 7));
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o[k][e] = (pix0 + e) * (unsigned)d.Cout + (unsigned)n;
            rv[k][e] = res ? res[o[k][e]] : 0.f;      // all residual loads before the first store
        }
    }
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        const int m0 = (q0 + (WS_NTHREADS / BN) * k) * 4;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float total = 0.f;
#pragma unroll
            // slice order.  Two things differ from the reduction launch in form, not in value: it starts from s0 and this from
            // 0 + s0 (an all-negative-zero sum gives +0, which no later term can tell apart), and it adds slabs already scaled by
            // acc_scale x 1 / operand scale while this scales the sum once -- the same roundings as long as that product is a
            // power of two, which the packing guarantees (ops.s16_weight_scale, s16_scale_from_bound; conv1x1_s16.hip relies on it too)
            for (int s = 0; s < WS_WAVES; ++s)
                if (s < ksplit) total = total + slabs[s * SLAB + (m0 + e) * SP + nl];
            if (d.stats_out) {
                float add = 0.f;
                if (d.bias) add = add + bias;
                if (d.badd) add = add + badd;
                v[e] = add + total * epi;
                if (res) v[e] = v[e] + rv[k][e];
            } else {
                v[e] = total * epi;
                if (d.bias) v[e] = v[e] + bias;
                if (d.badd) v[e] = v[e] + badd;
                if (res) v[e] = v[e] + rv[k][e];
            }
            out[o[k][e]] = v[e];
        }
        if (d.stats_out) {
            float cs, cq;
            s16_quad_stats(v[0], v[1], v[2], v[3], rows, cs, cq);
            // statistics tile pixq >> 2, flat over the batch
            *reinterpret_cast<float2*>(d.stats_out + ((size_t)(pixq[k] >> 2) * d.Cout + n) * 2) = make_float2(cs, cq);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Which launches of ddnm_conv_gather_s16_f32 take this kernel (`plan_ksplit`, `plan_bm`: the gather plan's split and M tile).
//   * form: 3x3, stride 1, pad 1, no nearest-x2 reads, 8 x 8 images (one tile = one image);
//   * the plan's slices fit the waves (2 <= ksplit <= WS_WAVES): the launches of the 8 x 8 level at B = 8 (64 tiles of 64 x 64
//     -> ksplit 8, every wave busy).  Smaller batches plan 16 slices, which a workgroup of 8 waves cannot hold; an un-split
//     plan has no reduction to save;
//   * statistics: the 4-pixel tiles of the reduction pass (splitk_stats_are_quads).
// Measured (profiles/wslice_ab.md): B = 8, 512 -> 512 and 512 + 512 -> 512 (8 slices), and the small plans of the tests -- 256 -> 64
// at B = 2 (8 slices of one chunk) and 64 + 32 -> 64 (3 slices, five waves without one): 0.61 ... 0.76 x the gather route, ranges apart.
// The 16 x 16 level (8 x 8 patches of an image; the kernel's addressing covers them) and the one-tap nin_shortcut were not
// measured and are not routed.
bool conv3x3_s16_wslice_routes(const ddnm_conv_desc* d, int plan_ksplit, int plan_bm) {
    if (d->ksize != 3 || d->stride != 1 || d->pad != 1 || d->ups || d->res_ups || d->out_nchw || d->skip0) return false;
    if (d->Ho != 8 || d->Wo != 8 || d->Hin != 8 || d->Win != 8) return false;
    if (d->C0 <= 0 || d->C0 % S16_KCH || d->C1 % S16_KCH || d->Cout % 64) return false;
    if (plan_ksplit < 2 || plan_ksplit > WS_WAVES || plan_bm != WS_BM) return false;
    if (d->stats_out && !splitk_stats_are_quads(d)) return false;
    return true;
}

int conv3x3_s16_wslice_launch(const ddnm_conv_desc* d, int ksplit, hipStream_t s) {
    const ConvArgs p = conv_args(*d, WS_BM, d->Cout / WS_BN, 8, 3, d->Wo / 8, 9, ksplit);
    DDNM_LAUNCH(conv_s16_wslice_kernel, dim3(p.m_tiles * p.n_tiles), dim3(WS_NTHREADS), 0, s, p);
    return 0;
}
