// GEMM form of the 1x1 / stride-1 convolutions in the split-fp16 arithmetic (fp32-grade products on
// v_mfma_f32_32x32x16_f16), gfx950: the attention blocks' qkv and proj_out and the un-fused nin_shortcut of the celeba
// `Model` (guided_diffusion/models.py:109,143-162), which conv_gather_s16.hip runs as a one-tap gather.
//
//   out[m][n] = sum_k A'[m][k] . W[n][k] (+ bias + badd + res),   m = pixel, flat over the batch
//
// Arithmetic and operand formats are the family's (s16_tile.h): fp32 tensors, A' = the operand after the optional GroupNorm
// affine (raw operands scaled per image by the power of two of `amax_in`), split into [hi 32 | lo 32] rows; weights in the
// split packing with ntaps = 1; product = s16_mfma_tile; accumulator scaled by acc_scale / operand scale; no atomics, one
// fixed summation order -- the gather route's own, chunk by chunk and, where that route splits K, slice by slice: output and
// statistics equal the gather route's bit for bit (tests/test_gpu_runner_replay.py pins the runner's PNGs by hash).  What a
// 1x1 does not need is the gather: the rows of an M tile are consecutive pixels, every address is known before the loop,
// and K (<= 1024 channels here) is short enough for ONE workgroup to own all of it -- no split-K slabs, no reduction launch.
//
// Workgroup 256 threads = 4 waves (2 x 2), tile 64 pixels x 64 output channels (the B = 8 launches of the network give 256
// ... 768 workgroups un-split), K step = G1_KS = 2 sub-rows of 32 channels per barrier pair.  Request stream per step s,
// all counted (`s_waitcnt vmcnt(N)`, raw barriers), branch-free:
//   W(s): G1_KS weight tiles [64 rows][hi 32 | lo 32] by LDS-DMA, three step groups in LDS, requested two steps ahead and
//         ahead of the A staging of the step (behind barrier #1, which frees the group of step s - 1);
//   A(s): G1_KS x G1_AR float4 per thread through registers (+ the two GroupNorm vectors per sub-row), THREE register sets:
//         requested three steps ahead, staged (GroupNorm / scale / split_store, 144-byte row pitch) one step at a time.
// Behind W(s), when step s waits for it, lie A(s+1) W(s+1) A(s+2) W(s+2) A(s+3): 3 G1_REQ_A + 2 G1_REQ_W requests in flight.
// A ragged last step (Cin / 32 odd) fetches its missing sub-row out of range (zeros) and stages zeros; requests beyond the
// last step are clamped to it.  LDS 66 KB: two workgroups per CU.
#include "s16_tile.h"

constexpr int G1_KS = 2;                              // 32-channel sub-rows per K step
constexpr int G1_BM = 64, G1_BN = 64;
constexpr int G1_AR = G1_BM / 32;                     // A: float4 loads per thread and sub-row
constexpr int G1_BR = G1_BN / 32;                     // W: LDS-DMA instructions per wave and sub-row
constexpr int G1_NWG = 3;                             // weight step groups in LDS: step, step + 1, step + 2
constexpr int G1_WSUB = G1_BN * 128;                  // bytes of one sub-row weight tile (unpadded, swizzled)
constexpr int G1_ASUB = G1_BM * S16_LDH;              // halfs of one sub-row A tile
constexpr int G1_REQ_A = G1_KS * (G1_AR + 2);         // requests per wave of one A step (gathers + 2 GroupNorm vectors per sub-row)
constexpr int G1_REQ_W = G1_KS * G1_BR;               // ... of one W step
constexpr int G1_WAIT = 3 * G1_REQ_A + 2 * G1_REQ_W;  // requests behind W(s) at its wait
constexpr int G1_MAX_CIN = 1024;                      // one workgroup owns all of K up to here ...
constexpr int G1_ROUTE_MAX_CIN = 512;                 // ... and is routed up to here (measured, conv1x1_s16_routes)
static_assert(G1_WAIT < 64, "vmcnt counts to 63");

// stats_px: 0 = no statistics; 4 = one partial row per 4 consecutive pixels (the layout of the split-K reduction pass,
// conv_common.h::splitk_stats_tiles, which the Python layer sized stats_out for); G1_BM = one per M tile (conv_epilogue's)
__global__ __launch_bounds__(256) void conv1x1_s16_kernel(const ConvArgs p, const int stats_px) {
    // ONE shared object (conv_gather_s16.hip: a second one makes the compiler drain the LDS-DMA queue before fragment reads)
    __shared__ __attribute__((aligned(1024))) char lds_all[G1_NWG * G1_KS * G1_WSUB + G1_KS * G1_ASUB * 2];
    char* const Bs = lds_all;
    _Float16* const As = reinterpret_cast<_Float16*>(lds_all + G1_NWG * G1_KS * G1_WSUB);

    const ddnm_conv_desc& d = p.d;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int tile_id = xcd_swizzle(blockIdx.x, gridDim.x);
    const int n_tile = tile_id % p.n_tiles, m_tile = tile_id / p.n_tiles;
    const int hw = d.Ho * d.Wo;
    const int img = m_tile / (hw / G1_BM);            // (hw % G1_BM == 0: a tile lies in one image)
    const unsigned pix0 = (unsigned)m_tile * G1_BM;   // first pixel of the tile, flat over the batch
    float ascale, inv_ascale;
    s16_operand_scale(d.gn_scale == nullptr ? d.amax_in : nullptr, img, false, ascale, inv_ascale);

    // ---- W: the sub-row tiles of step s -> Bs[group] by LDS-DMA, swizzled lane-linear image of s16_tile.h
    const int lrow = lane >> 3, lpiece = lane & 7;
    const int wswz = S16_W_SWZ(wave, lrow);
    const unsigned w_rowlen = (unsigned)p.Cin * 4u;
    const int cout_pad = (d.Cout + 127) / 128 * 128;
    const __amdgpu_buffer_rsrc_t r_w = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(reinterpret_cast<const void*>(d.weight)), 0, (unsigned)cout_pad * w_rowlen, 0x00020000);
    const unsigned w_voff = S16_W_LANE(n_tile * G1_BN + wave * 8 + lrow, w_rowlen, lpiece, wswz);
    const int nchunks = p.Cin / S16_KCH;
    const int nsteps = (nchunks + G1_KS - 1) / G1_KS;
    auto chunk_of = [&](int s, int sub) { const int c = s * G1_KS + sub; return c < nchunks ? c : nchunks - 1; };
    auto issue_w = [&](int s, int grp) {
#pragma unroll
        for (int sub = 0; sub < G1_KS; ++sub)
            s16_w_request<G1_BR, 4>(r_w, Bs + (grp * G1_KS + sub) * G1_WSUB + wave * 1024, w_voff, (unsigned)chunk_of(s, sub) * S16_KCH * 4u,
                                    w_rowlen);
    };

    // ---- A: rows row0 + 32 i of the tile, float4 column c4 of each sub-row; exactly G1_REQ_A requests per call (a
    // sub-row past Cin is fetched out of range, GroupNorm vectors from a dummy address without GroupNorm)
    const bool has_gn = d.gn_scale != nullptr;
    const int c4 = tid & 7, row0 = tid >> 3;
    const __amdgpu_buffer_rsrc_t r_s0 = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(d.src0), 0, (unsigned)d.B * hw * d.C0 * 4u, 0x00020000);
    const __amdgpu_buffer_rsrc_t r_s1 = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(d.C1 > 0 ? d.src1 : d.src0), 0, (unsigned)d.B * hw * (d.C1 > 0 ? d.C1 : d.C0) * 4u, 0x00020000);
    const float* const gn_sc = has_gn ? d.gn_scale + (size_t)img * p.Cin + c4 * 4 : reinterpret_cast<const float*>(d.weight);
    const float* const gn_sh = has_gn ? d.gn_shift + (size_t)img * p.Cin + c4 * 4 : reinterpret_cast<const float*>(d.weight);
    struct ASet {
        f32x4 v[G1_KS][G1_AR], gsc[G1_KS], gsh[G1_KS];
        unsigned live;                                // bit sub: the sub-row lies inside Cin
    };
    ASet a0, a1, a2;

    auto prefetch_a = [&](int s, ASet& a) {
        a.live = 0;
#pragma unroll
        for (int sub = 0; sub < G1_KS; ++sub) {
            const bool live = s * G1_KS + sub < nchunks;
            const int cb = chunk_of(s, sub) * S16_KCH;
            const bool first = cb < d.C0;             // C0 % 32 == 0: a sub-row lies in one source (wave-uniform select)
            const unsigned cs = first ? d.C0 : d.C1, coff = first ? cb : cb - d.C0;
            const __amdgpu_buffer_rsrc_t r_s = first ? r_s0 : r_s1;
#pragma unroll
            for (int i = 0; i < G1_AR; ++i) {
                const unsigned vo = (((pix0 + row0 + 32 * i) * cs + c4 * 4) * 4u) | (live ? 0u : S16_OOB);
                a.v[sub][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r_s, vo, coff * 4u, 0));
            }
            a.gsc[sub] = *reinterpret_cast<const f32x4*>(gn_sc + (has_gn ? cb : 0));
            a.gsh[sub] = *reinterpret_cast<const f32x4*>(gn_sh + (has_gn ? cb : 0));
            a.live |= live ? (1u << sub) : 0u;
        }
    };
    auto stage_a = [&](const ASet& a) {
#pragma unroll
        for (int sub = 0; sub < G1_KS; ++sub)
#pragma unroll
            for (int i = 0; i < G1_AR; ++i) {
                f32x4 v = a.v[sub][i];
                if (has_gn && (a.live & (1u << sub))) v = gn_act(v, a.gsc[sub], a.gsh[sub], d.gn_silu);
                split_store(&As[sub * G1_ASUB + (row0 + 32 * i) * S16_LDH + c4 * 4], v, ascale);
            }
    };

    f32x16 acc[1][1], total;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][0][r] = total[r] = 0.f;
    // Where the gather route splits K (p.ksplit slices of chunks [n s / k, n (s + 1) / k), summed in slice order by its reduction
    // launch) the accumulator is folded into `total` at the same chunk boundaries, with the roundings of that route: the
    // results are the gather route's bit for bit, whatever it does.  (A slab value is accumulator x a power of two: scaling
    // the sum of the slices once, in the epilogue, rounds like summing scaled slices.)  fold_at = the next boundary, stepped
    // without a division.
    const int ksplit = p.ksplit;
    const int fold_base = nchunks / ksplit, fold_rem = nchunks - fold_base * ksplit;
    int fold_at = fold_base, fold_e = fold_rem;
    const _Float16* a_frag = As + (wm * 32 + (lane & 31)) * S16_LDH + (lane >> 5) * 8;
    const int b_frag = S16_B_FRAG(wn * 32, lane);

    // Per step:  [barrier #1: As and the group of W(s-1) are free | request W(s+2) | A(s): registers -> GroupNorm / split ->
    //             LDS | request A(s+3) into the freed registers | my pieces of W(s) landed | barrier #2 | MFMA(s)]
    {
        const int last = nsteps - 1;
        auto clamps = [&](int q) { return q < last ? q : last; };
        // (fenced: a register load the compiler moves behind the next weight request is one request more behind that tile
        // than the first waits count -- an over-wait, but the replay of the stream is exact only in this order)
        prefetch_a(0, a0);
        asm volatile("" ::: "memory");
        issue_w(0, 0);
        asm volatile("" ::: "memory");
        prefetch_a(clamps(1), a1);
        asm volatile("" ::: "memory");
        issue_w(clamps(1), 1);
        asm volatile("" ::: "memory");
        prefetch_a(clamps(2), a2);
        int cur = 0;                                  // group of W(s)
        auto step = [&](int s, ASet& a) {
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            issue_w(clamps(s + 2), cur >= 1 ? cur - 1 : G1_NWG - 1);
            stage_a(a);
            prefetch_a(clamps(s + 3), a);
            asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(G1_WAIT) : "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            int a_rows[1];
            a_rows[0] = 0;
#pragma unroll
            for (int sub = 0; sub < G1_KS; ++sub) {
                s16_mfma_tile<1, 1>(acc, a_frag, a_rows, sub * G1_ASUB, Bs + (cur * G1_KS + sub) * G1_WSUB, b_frag);
                if (ksplit > 1 && s * G1_KS + sub + 1 == fold_at) {      // (wave-uniform) the slice ends with this chunk
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        total[r] = total[r] + acc[0][0][r];      // the slab of the slice, added in slice order
                        acc[0][0][r] = 0.f;
                    }
                    fold_e += fold_rem;
                    const int carry = fold_e >= ksplit ? 1 : 0;
                    fold_e -= carry ? ksplit : 0;
                    fold_at += fold_base + carry;
                }
            }
            cur = cur == G1_NWG - 1 ? 0 : cur + 1;
        };
        // triples in the loop (one step per register set), the remainder behind it (conv_gather_s16.hip: a conditional
        // step inside the loop costs the lookahead)
        int s = 0;
        for (; s + 2 < nsteps; s += 3) {
            step(s, a0);
            step(s + 1, a1);
            step(s + 2, a2);
        }
        if (s < nsteps) step(s, a0);
        if (s + 1 < nsteps) step(s + 1, a1);
        // the clamped requests of the last steps fetch what nobody reads: named here as read, or the compiler deletes them
        // and the last waits count requests that were never issued (a stale weight tile)
        auto keep = [](const ASet& a) {
            asm volatile("" ::"v"(a.v[0][0]), "v"(a.v[0][1]), "v"(a.v[1][0]), "v"(a.v[1][1]), "v"(a.gsc[0]), "v"(a.gsh[0]), "v"(a.gsc[1]),
                         "v"(a.gsh[1]));
        };
        static_assert(G1_KS == 2 && G1_AR == 2, "keep names every register of a set");
        keep(a0);
        keep(a1);
        keep(a2);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the tail requests
    }

    // ---- epilogue.  C/D map of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  The terms
    // are added in the order of the route the launch replaces: conv_epilogue (un-split), conv_splitk_reduce_stats_kernel
    // (split, statistics) or conv_splitk_reduce_kernel (split, none); statistics of the FINAL values
    const float epi = d.acc_scale * inv_ascale;
    const int n = n_tile * G1_BN + wn * 32 + (lane & 31);
    const int rsel = 4 * (lane >> 5);
    const float bias = d.bias ? d.bias[n] : 0.f, badd = d.badd ? d.badd[(size_t)img * d.badd_stride + n] : 0.f;
    const float* __restrict__ res = d.res;
    float* __restrict__ out = d.out;
    unsigned o[16];
    float rv[16], v[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        o[r] = (pix0 + wm * 32 + (r & 3) + 8 * (r >> 2) + rsel) * (unsigned)d.Cout + (unsigned)n;
        rv[r] = res ? res[o[r]] : 0.f;                // all 16 residual loads before the first store
    }
    if (ksplit == 1) {
        float add = 0.f;
        if (d.bias) add = bias;
        if (d.badd) add += badd;
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = acc[0][0][r] * epi + add + rv[r];
    } else if (d.stats_out) {
        float add = 0.f;
        if (d.bias) add = add + bias;
        if (d.badd) add = add + badd;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            v[r] = add + total[r] * epi;
            if (res) v[r] = v[r] + rv[r];
        }
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            v[r] = total[r] * epi;
            if (d.bias) v[r] = v[r] + bias;
            if (d.badd) v[r] = v[r] + badd;
            if (res) v[r] = v[r] + rv[r];
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) out[o[r]] = v[r];
    if (stats_px == 4) {
        // four consecutive registers of a lane = four consecutive pixels of one channel = one statistics tile
        const unsigned t0 = (pix0 + wm * 32 + rsel) >> 2;      // tile of registers 0..3, flat over the batch (hw % 4 == 0)
        const int rows = 256 / (d.Cout >> 2);                // pixel rows of the reduction pass's workgroup
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float cs, cq;
            s16_quad_stats(v[q * 4], v[q * 4 + 1], v[q * 4 + 2], v[q * 4 + 3], rows, cs, cq);
            float2* const st = reinterpret_cast<float2*>(d.stats_out + ((size_t)(t0 + 2 * q) * d.Cout + n) * 2);
            *st = make_float2(cs, cq);
        }
    } else if (stats_px == G1_BM) {
        float cs = 0.f, cq = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            cs += v[r];
            cq = __builtin_fmaf(v[r], v[r], cq);
        }
        cs += __shfl_xor(cs, 32);
        cq += __shfl_xor(cq, 32);
        float* const lds = reinterpret_cast<float*>(As);
        __syncthreads();                              // every wave is done with the operand tiles in LDS
        if (lane < 32) {
            lds[(wm * G1_BN + wn * 32 + lane) * 2 + 0] = cs;
            lds[(wm * G1_BN + wn * 32 + lane) * 2 + 1] = cq;
        }
        __syncthreads();
        if (tid < G1_BN * 2) {
            const int c = tid >> 1, which = tid & 1;
            d.stats_out[((size_t)m_tile * d.Cout + n_tile * G1_BN + c) * 2 + which] = lds[c * 2 + which] + lds[(G1_BN + c) * 2 + which];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Which launches of ddnm_conv_gather_s16_f32 take this kernel (`plan_ksplit`, `plan_bm`: the gather plan's split and M tile,
// which fix the statistics layout the caller sized).  Host-side predicate on the descriptor:
//   * form: 1x1, stride 1, no padding, no nearest-x2 reads, Cin <= G1_MAX_CIN;
//   * statistics: the plan's layout must be one the kernel fills -- 4-pixel tiles of a split plan, 64-pixel tiles of an
//     un-split plan on 64 x 64 tiles;
//   * measured (profiles/conv1x1_s16_ab.md; bar: at most 0.8 x the gather route, its reduction launch included): Cin <=
//     G1_ROUTE_MAX_CIN at every batch size.  The 16 serial K steps of the 1024-channel nin_shortcut take as long as the
//     gather kernel's 8 slices of 4 steps plus their reduction (0.98 ... 1.2 x): those launches stay where they were.
//     DDNM_CONV_GEMM1X1 in ddnm_conv_desc::flags overrides this rule alone (the table was measured so).
int conv1x1_s16_stats_px(const ddnm_conv_desc* d, int plan_ksplit, int plan_bm) {
    if (!d->stats_out) return 0;
    if (plan_ksplit > 1) return splitk_stats_are_quads(d) ? 4 : -1;
    return plan_bm == G1_BM ? G1_BM : -1;
}

bool conv1x1_s16_routes(const ddnm_conv_desc* d, int plan_ksplit, int plan_bm) {
    const int hw = d->Ho * d->Wo, Cin = d->C0 + d->C1;
    if (d->ksize != 1 || d->stride != 1 || d->pad != 0 || d->ups || d->res_ups || d->out_nchw || d->skip0) return false;
    if (d->Ho != d->Hin || d->Wo != d->Win || hw % G1_BM || d->Cout % G1_BN) return false;
    if (d->C0 <= 0 || d->C0 % S16_KCH || d->C1 % S16_KCH || Cin > G1_MAX_CIN) return false;
    if (conv1x1_s16_stats_px(d, plan_ksplit, plan_bm) < 0) return false;
    if (d->flags & DDNM_CONV_GEMM1X1) return true;      // A/B timing: every launch the kernel has a form for
    return Cin <= G1_ROUTE_MAX_CIN;
}

// `run_ksplit`: the split the gather route would run with the workspace at hand (conv_run_ksplit) -- the kernel splits nothing,
// it adds in that route's order
int conv1x1_s16_launch(const ddnm_conv_desc* d, int plan_ksplit, int plan_bm, int run_ksplit, hipStream_t s) {
    const ConvArgs p = conv_args(*d, G1_BM, d->Cout / G1_BN, 32, 5, 0, 1, run_ksplit);
    DDNM_LAUNCH(conv1x1_s16_kernel, dim3(p.m_tiles * p.n_tiles), dim3(256), 0, s, p, conv1x1_s16_stats_px(d, plan_ksplit, plan_bm));
    return 0;
}
