/*
 * ddnm_hip.h -- C ABI of libddnm_hip.so: hand-written HIP kernels (gfx950 / CDNA4)
 * for the DDNM sampling hot path.
 *
 * The reference (wyhuai/DDNM) has no FFI of its own: it is pure PyTorch and every
 * hot op is an ATen call.  Each entry point below replaces
 * the ATen call sites cited next to it; INTEGRATION.md shows the ctypes stub a
 * maintainer of the reference would add.
 *
 * Conventions (all entry points):
 *   - plain device pointers + sizes; no torch types, no allocation, no host sync,
 *     no global state; work is enqueued on `stream` (hipStream_t passed as void*).
 *   - returns 0 on success, a positive hipError_t on a runtime error, or a negative
 *     DDNM_E_* code on an argument the kernel family does not support.
 *   - activations inside the UNet are NHWC fp32 ("pixel-major": [B][H][W][C]);
 *     the sampler-side images are NCHW fp32 exactly like the reference tensors.
 *   - thread-safe for concurrent calls on different streams / devices.
 */
#ifndef DDNM_HIP_H
#define DDNM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DDNM_E_BADARG (-1)   /* null pointer / non-positive size / misaligned */
#define DDNM_E_SHAPE (-2)    /* shape not supported by this kernel family */

int ddnm_version(void);                 /* ABI version, currently 7 (bumped on every struct / prototype change; the
                                           per-image inpainting entry points *_pi_* were added under 7: new symbols
                                           only, no struct and no existing prototype changed; the demosaicing entry
                                           points *_mosaic_*, the old-photo ones *_mcsr_* and the chroma ones
                                           *_chroma_*, the per-entry-noise ones *_hn_* and the JPEG ones *_jpeg_*
                                           likewise) */
const char* ddnm_build_digest(void);    /* sha256 of the sources + flags this binary was built from (build.py) */
int ddnm_sizeof(int which);             /* sizeof of 0: ddnm_conv_desc, 1: ddnm_gemm_desc, 2: ddnm_conv16_desc,
                                           3: ddnm_step_scalars as compiled into the binary (-1: unknown index) */
const char* ddnm_error_string(int code);

/* ------------------------------------------------------------------------- *
 * Implicit-GEMM convolution, fp32 in / fp32 accumulate on v_mfma_f32_32x32x2_f32.
 * Replaces nn.Conv2d 3x3 s1 p1 (guided_diffusion/models.py:87,96,225,295),
 * the asymmetric-pad 3x3 s2 Downsample (models.py:61-71), 1x1 convs
 * (models.py:109,143-162) and, through the fused prologue/epilogue, the
 * GroupNorm+swish in front of each conv (models.py:117-118,123-124,166,338-339),
 * F.interpolate(nearest x2) (models.py:48), torch.cat([h, skip]) (models.py:331),
 * the temb add (models.py:121) and the residual add (models.py:134,189).
 *
 *   out[b,oy,ox,n] = bias[n] + badd[b*badd_stride + n] + res[b,oy,ox,n]
 *                  + sum_{ky,kx,c} W[n,ky,kx,c] * act(in[b, oy*stride-pad+ky, ox*stride-pad+kx, c])
 *   in  = concat_c(src0 (C0 ch), src1 (C1 ch)), optionally nearest-x2 upsampled (ups=1),
 *   act(v) = silu?(v*gn_scale[b,c] + gn_shift[b,c]) when gn_scale != NULL (zero padding
 *            is applied AFTER act, like the reference which pads the activated tensor).
 * ------------------------------------------------------------------------- */
typedef struct ddnm_conv_desc {
    const float* src0;      /* NHWC [B][Hs][Ws][C0] */
    const float* src1;      /* NHWC [B][Hs][Ws][C1] or NULL */
    const float* weight;    /* packed [Cout_pad][KH*KW][Cin] (O,ky,kx,I), Cout_pad = ceil(Cout/tileN)*tileN */
    const float* bias;      /* [Cout] or NULL */
    const float* badd;      /* per-sample addend, row b at badd + b*badd_stride, or NULL */
    const float* res;       /* NHWC [B][Ho][Wo][Cout] or NULL */
    const float* gn_scale;  /* [B][Cin] or NULL */
    const float* gn_shift;  /* [B][Cin] (required iff gn_scale) */
    float* out;             /* NHWC [B][Ho][Wo][Cout], or NCHW [B][Cout][Ho][Wo] if out_nchw */
    int32_t B, Hin, Win;    /* logical input size (after the optional x2 upsample) */
    int32_t C0, C1;         /* C0 % 32 == 0, C1 % 32 == 0 (C1 = 0 without src1) */
    int32_t Cout;
    int32_t ksize;          /* 1 or 3 */
    int32_t stride;         /* 1 or 2 */
    int32_t pad;            /* top/left zero padding; bottom/right is implied by Ho, Wo */
    int32_t Ho, Wo;
    int32_t ups;            /* 1: src is [Hin/2][Win/2], read through nearest x2 */
    int32_t gn_silu;        /* 1: swish after the GroupNorm affine; 0: affine only */
    int32_t out_nchw;
    int32_t badd_stride;
    int32_t tile;           /* 0 auto; 1: 128x128, 2: 64x64, 3: 128x32 (M x N per workgroup) */
    float* workspace;       /* split-K scratch (may be NULL: the kernel then runs unsplit) */
    int64_t workspace_floats;
    int32_t res_ups;        /* 1: `res` is [B][Ho/2][Wo/2][Cout], added through a nearest x2 upsample
                               (x_upd of an `up=True` ResBlock, guided_diffusion/unet.py:237-242) */
    int32_t src_f16;        /* ddnm_conv3x3_f16_f32 only: src0/src1 point to IEEE fp16 NHWC tensors (the output of
                               ddnm_gn_apply_f16); gn_scale must then be NULL */
    float* stats_out;       /* optional [B*tiles][Cout][2]: per-(M tile, channel) sum / sum of squares of `out`,
                               tiles = ddnm_conv2d_f32_stats_tiles(d) per image; feeds ddnm_gn_finalize_tiles_f32 so
                               the consumer's GroupNorm never re-reads the tensor */
    /* fused 1x1 shortcut of a residual block (models.py:109,128-132; unet.py:222,256), 3x3 halo launches only:
     * out += W_skip . concat_c(skip0, skip1) evaluated on the RAW tensors at the output pixel */
    const float* skip0;     /* NHWC [B][Ho][Wo][SC0] or NULL */
    const float* skip1;     /* NHWC [B][Ho][Wo][SC1] or NULL */
    const float* skip_weight; /* packed [Cout_pad][SC0+SC1] (fp16 for ddnm_conv3x3_f16_f32) */
    int32_t SC0, SC1;
    float acc_scale;        /* ddnm_conv3x3_s16_f32 only: power of two that multiplies the accumulator before bias / residual
                               (undoes the operand pre-scaling of the split form); ignored by the other entry points */
    int32_t flags;          /* bit 0 (DDNM_CONV_ONE_TILE): ddnm_conv3x3_s16_f32 runs the one-tile-per-workgroup kernel even where
                               the persistent form (>= 2 tiles per CU) applies -- same results bit for bit; for A/B timing
                               bit 1 (DDNM_CONV_UPS_SUBPIXEL): ddnm_conv3x3_s16_f32 with ups = 1 takes `weight` as the PHASE
                               packing of the upsample convolution (see ddnm_conv3x3_s16_ups_subpixel_supported)
                               ddnm_conv_gather_s16_f32: bit 0 keeps a 1x1 launch on the gather kernel, bit 2 (DDNM_CONV_GEMM1X1)
                               sends it to the GEMM form wherever that kernel has a form for it, also where the measured
                               routing rule would not (see ddnm_conv_gather_s16_gemm1x1); bit 0 wins; for A/B timing
                               ddnm_conv_gather_s16_f32: bit 0 also keeps a 3x3 launch of the 8 x 8 level on the gather kernel
                               (see ddnm_conv_gather_s16_wslice) */
    /* ABI 5 -- operand-range guard of the split forms (ddnm_conv3x3_s16_f32, ddnm_conv_gather_s16_f32; ignored by every
     * other entry point).  fp16 carries |v| < 65504 only, fp32 -- the arithmetic the reference runs -- does not care, so
     * operands the kernel reads RAW (no GroupNorm in front: src0 / src1 when gn_scale is NULL, skip0 / skip1 always) are
     * scaled per launch and image by a power of two derived ON THE DEVICE from an upper bound of their magnitude:
     *   amax_in = [B][DDNM_AMAX_N] non-negative floats, max_i amax_in[b][i] >= max |raw operand of image b|
     * (ddnm_gn_finalize_tiles_amax_f32 emits them from the producer's GroupNorm partials for free, ddnm_amax_bound_f32
     * from partials or from the tensor itself).  The kernel multiplies the raw operand by 2^k, k = 14 - exponent(bound)
     * (bound lands in [2^14, 2^15): no overflow for ANY fp32 input magnitude, and uniformly tiny tensors keep fp32
     * grade because hi AND lo become normal fp16 numbers), and the accumulator by 2^-k (exact).  A launch whose main
     * operand is GroupNorm'd and whose fused shortcut is raw shares one accumulator: k is then clamped to <= 0 (scale
     * down only) and applied to both operands.  NULL = no scaling (operands must lie within fp16 range). */
    const float* amax_in;
} ddnm_conv_desc;

#define DDNM_CONV_ONE_TILE 1
#define DDNM_CONV_UPS_SUBPIXEL 2
#define DDNM_CONV_GEMM1X1 4
#define DDNM_AMAX_N 32   /* bound words per image (= the GroupNorm group count of both networks) */

int ddnm_conv2d_f32(const ddnm_conv_desc* d, void* stream);
/* N-tile (32 or 64 or 128) the kernel will use for this desc: Cout_pad of the packed weight. */
int ddnm_conv2d_f32_tile_n(const ddnm_conv_desc* d);
/* Scratch floats the auto plan wants for this desc (0: no split-K); low-resolution layers whose tile
 * grid cannot fill 256 CUs split their channel chunks over several workgroups per tile. */
int64_t ddnm_conv2d_f32_workspace_floats(const ddnm_conv_desc* d);
/* M tiles per image of the auto plan if this launch can emit `stats_out` (0: split-K or NCHW launch). */
int ddnm_conv2d_f32_stats_tiles(const ddnm_conv_desc* d);
/* 1 if this launch would run the 3x3 halo kernel and can therefore take the fused shortcut fields. */
int ddnm_conv2d_f32_fuses_skip(const ddnm_conv_desc* d);

/* Output convolution with <= 4 output channels (conv_out of the celeba `Model`, guided_diffusion/models.py:295-299): same
 * descriptor with ksize 3, stride 1, pad 1, out_nchw = 1, one source, Cin % 32 == 0, Win % 32 == 0, Hin % 8 == 0, optional
 * fused GroupNorm affine + swish and bias; no residual / shortcut / statistics.  HBM-bound vector-ALU kernel (on the
 * MFMA tile kernel the 3 channels are padded to a 32-wide N tile: 10x the matrix work). */
int ddnm_conv3x3_small_cout_f32(const ddnm_conv_desc* d, void* stream);
int ddnm_conv3x3_small_cout_f32_supported(const ddnm_conv_desc* d);

/* 3x3 / stride 1 / pad 1 convolution with fp16 MFMA operands (v_mfma_f32_32x32x16_f16), fp32 accumulate:
 * the reference's `use_fp16` torso (guided_diffusion/unet.py:619-625, fp16_util.py:15-22).  Same descriptor;
 * `weight` points to the (O,ky,kx,I)-packed weights stored as IEEE fp16, activations / bias / residual /
 * output stay fp32 in HBM (rounded to fp16 while the halo tile is staged).  Needs Cin % 64 == 0,
 * Cout % 128 == 0, Ho*Wo % 256 == 0; `_supported` tells whether a desc qualifies (else use ddnm_conv2d_f32). */
int ddnm_conv3x3_f16_f32(const ddnm_conv_desc* d, void* stream);
int ddnm_conv3x3_f16_supported(const ddnm_conv_desc* d);
int64_t ddnm_conv3x3_f16_workspace_floats(const ddnm_conv_desc* d);
int ddnm_conv3x3_f16_stats_tiles(const ddnm_conv_desc* d);

/* 3x3 / stride 1 / pad 1 convolution of fp32 tensors with fp32-GRADE products on the fp16 matrix pipe (the celeba
 * `Model`, guided_diffusion/models.py:87,96,225 -- the reference runs it in fp32): every operand value v is carried as
 * hi = rn16(v), lo = rn16(v - hi), a product is hi*hi' + hi*lo' + lo*hi' (three v_mfma_f32_32x32x16_f16 whose fp16 x fp16
 * products are exact in the fp32 accumulator; the dropped lo*lo' term is 2^-22 relative), so the operand error is
 * <= 2^-22 -- below the accumulation noise of an fp32 dot product of this length -- at 16/3 of the fp32 MFMA rate.
 * Same descriptor as ddnm_conv2d_f32 (GroupNorm + swish prologue, concat, x2 upsample, fused shortcut, bias / badd /
 * residual, statistics, split-K) except:
 *   weight / skip_weight = the SPLIT packing: per (output row, tap, 32-channel chunk) 32 hi halfs then 32 lo halfs of
 *     2^s * W (the byte size of the fp32 (O,ky,kx,I) array), Cout padded to 128; one power of two 2^s per launch that
 *     brings max|W| into [2^13, 2^14) so that lo is a normal fp16 number;
 *   acc_scale = 2^-s (times the inverse of the kernel's compile-time activation pre-scale, ddnm_conv3x3_s16_act_scale()).
 * Needs Cin % 32 == 0, C0 % 32 == 0, Cout % 128 == 0, Ho*Wo % 256 == 0 (else: ddnm_conv2d_f32). */
int ddnm_conv3x3_s16_f32(const ddnm_conv_desc* d, void* stream);
int ddnm_conv3x3_s16_supported(const ddnm_conv_desc* d);
int ddnm_conv3x3_s16_persistent(const ddnm_conv_desc* d);   /* ABI 7 -- 1: the launch runs the persistent form (>= 2 tiles per CU: one
                                                                workgroup per CU walks its tiles; same results bit for bit) */
int64_t ddnm_conv3x3_s16_workspace_floats(const ddnm_conv_desc* d);
int ddnm_conv3x3_s16_stats_tiles(const ddnm_conv_desc* d);
/* Sub-pixel form of `nearest x2 -> 3x3` (ups = 1, flags & DDNM_CONV_UPS_SUBPIXEL; additions within ABI 7): output pixel
 * (2y + py, 2x + px) = sum_{a,b in {0,1}} Wp[py][px][a][b] . X[y + py - 1 + a][x + px - 1 + b] on the low-resolution grid, with
 * Wp = the 3x3 taps that land on the same source pixel, pre-summed: 16 tap products per source pixel instead of 36.
 *   weight = split packing [4 Cout rows][4 steps (a, b)][Cin / 32][hi 32 | lo 32] of 2^s * Wp, row ((cb * 2 + py) * 2 + px) * 64 + c
 *     for output channel cb * 64 + c; 2^s brings max|Wp| into [2^13, 2^14); acc_scale = 2^-s.
 * 1 when the launch qualifies: low-resolution W % 32 == 0, H % 8 == 0, Cin % 32 == 0 (C0 too) with >= 2 chunks, Cout % 64 == 0,
 * raw operand (amax_in required at launch), bias only (no badd / res / GroupNorm prologue / shortcut / NCHW), sizes addressable.
 * Never splits K (workspace ignored); statistics: Ho * Wo / 256 partial rows per image.  A flagged launch that does not qualify
 * is an error, never a fall-back. */
int ddnm_conv3x3_s16_ups_subpixel_supported(const ddnm_conv_desc* d);
float ddnm_conv3x3_s16_act_scale(void);   /* compile-time activation pre-scale: 1 since ABI 5 (the scale is per launch and
                                             image, derived on the device from ddnm_conv_desc::amax_in) */

/* The same arithmetic for the layers the 3x3 halo kernel does not take, as a per-tap gather (csrc/conv_gather_s16.hip):
 * Downsample's 3x3 stride 2 with (0,1,0,1) padding (guided_diffusion/models.py:61-71), the 1x1 convolutions of the
 * attention blocks and un-fused nin_shortcut (models.py:109,143-162), and 3x3 / stride 1 on the 8 x 8 level (in the
 * slices-on-waves form below where the plan has 2 ... 8 slices).  Same
 * descriptor, weight packing and acc_scale as ddnm_conv3x3_s16_f32 (ksize 1 or 3, stride 1 or 2, pad as given; GroupNorm
 * prologue, concat, bias / badd / residual, statistics, split-K); no fused shortcut.
 * Needs C0 % 32 == 0, C1 % 32 == 0, Cout % 64 == 0, Ho*Wo % 64 == 0 (else: ddnm_conv2d_f32). */
int ddnm_conv_gather_s16_f32(const ddnm_conv_desc* d, void* stream);
int ddnm_conv_gather_s16_supported(const ddnm_conv_desc* d);
int64_t ddnm_conv_gather_s16_workspace_floats(const ddnm_conv_desc* d);
int ddnm_conv_gather_s16_stats_tiles(const ddnm_conv_desc* d);
/* GEMM form of the 1x1 / stride-1 launches (csrc/conv1x1_s16.hip; addition within ABI 7): 64 x 64 tiles, one workgroup owns
 * all of K (Cin <= 1024), so the launch writes no split-K slabs and needs no reduction launch; same operands, arithmetic,
 * workspace and statistics answers as above (a launch the plan splits fills the reduction pass's 4-pixel statistics tiles),
 * same results bit for bit (it adds in the gather route's order, slice by slice where that route splits K).
 * Routed where it was measured at most 0.8 x the gather route (profiles/conv1x1_s16_ab.md): Cin <= 512.
 * 1 when ddnm_conv_gather_s16_f32 runs this descriptor in that form (`stats_out` and `flags` count: set them as the launch
 * will), 0 when it runs the gather kernel -- always with flags & DDNM_CONV_ONE_TILE --, negative when the family refuses the
 * shape. */
int ddnm_conv_gather_s16_gemm1x1(const ddnm_conv_desc* d);
/* Slices-on-waves form of the 3x3 / stride 1 / pad 1 launches on 8 x 8 images whose plan splits K 2 ... 8 ways (csrc/conv_s16_wslice.hip;
 * addition within ABI 7): one workgroup of 8 waves per (image, 32 output channels), wave w computes the plan's K slice w, the
 * slices are added in LDS in slice order and the epilogue of the reduction pass runs in the same kernel -- no slabs, no
 * reduction launch; same operands, workspace and statistics answers, same results bit for bit.
 * 1 when ddnm_conv_gather_s16_f32 runs this descriptor in that form (given the workspace the plan asks for; `stats_out` and
 * `flags` count), 0 when it runs the gather kernel -- always with flags & DDNM_CONV_ONE_TILE --, negative when the family
 * refuses the shape. */
int ddnm_conv_gather_s16_wslice(const ddnm_conv_desc* d);

/* 1x1 convolution with fp16 MFMA operands, fp32 accumulate / output: the attention blocks' qkv and proj_out
 * Conv1d(k=1) and un-fused 1x1 shortcuts of the `use_fp16` torso (guided_diffusion/unet.py:222,283-289,301-308).
 * Same descriptor with ksize = 1, stride 1, pad 0; `weight` = (O,1,I)-packed fp16; src fp32, or fp16 with src_f16 = 1
 * (output of ddnm_gn_apply_f16 -- there is no fused GroupNorm prologue: gn_scale must be NULL).  Needs Cin % 64 == 0,
 * Cout % 128 == 0, B*Ho*Wo % 256 == 0; statistics only when Ho*Wo % 256 == 0. */
int ddnm_conv1x1_f16_f32(const ddnm_conv_desc* d, void* stream);
int ddnm_conv1x1_f16_supported(const ddnm_conv_desc* d);
int64_t ddnm_conv1x1_f16_workspace_floats(const ddnm_conv_desc* d);
int ddnm_conv1x1_f16_stats_tiles(const ddnm_conv_desc* d);

/* ------------------------------------------------------------------------- *
 * fp16-ACTIVATION path of the `use_fp16` torso (guided_diffusion/unet.py:619-625,655-663; fp16_util.py:15-22):
 * every tensor in HBM is fp16 NHWC, like the reference's `h.type(self.dtype)` tensors; accumulation, GroupNorm
 * statistics, softmax stay fp32.
 *
 * ddnm_conv16: 3x3 (stride 1, pad 1) or 1x1 convolution, v_mfma_f32_32x32x16_f16, 256 x 256 tiles staged by
 * LDS-DMA (csrc/conv16.hip).  Replaces the nn.Conv2d / Conv1d(k=1) of ResBlock / AttentionBlock
 * (unet.py:196-222,283-308) with, fused: nearest x2 upsample of the operand (ups; unet.py:104-109), the 1x1
 * skip_connection as extra K chunks (unet.py:222,256), bias, residual add (through a nearest x2 upsample for
 * `up=True` blocks) and the GroupNorm partials of the output.
 *   out[b,y,x,n] = fp16( bias[n] + res[b,y,x,n] + sum W[n,ky,kx,c] * src[b, y+ky-1, x+kx-1, c]
 *                        + sum W_skip[n,c] * concat_c(skip0, skip1)[b,y,x,c] )
 * act(v) = silu?(v*gn_scale[b,c] + gn_shift[b,c]) when gn_scale != NULL (3x3 only; applied inside LDS after the
 * LDS-DMA, zero padding AFTER act like the reference), identity otherwise (operand already activated by
 * ddnm_gn_apply_h16).  The operand may be the channel concat of `src` (C0 channels) and `src1`.
 * Needs Cin % 64 == 0, Cout % 64 == 0; 3x3: W % 16 == 0 and H*W % 128 == 0 (smaller images: ddnm_im2col3x3_h16 +
 * ksize 1).  ksize 1 treats src as a flat [B*H*W][Cin] matrix (any row count).
 * ------------------------------------------------------------------------- */
typedef struct ddnm_conv16_desc {
    const void* src;          /* fp16 NHWC [B][Hs][Ws][C0] (C0 = Cin without src1); Hs = H/2 when ups */
    const void* weight;       /* fp16 packed [ceil(Cout/256)*256][ksize*ksize][Cin] (O,ky,kx,I) */
    const float* bias;        /* [Cout] or NULL */
    const void* res;          /* fp16 NHWC [B][H][W][Cout] ([B][H/2][W/2][Cout] when res_ups) or NULL */
    const void* skip0;        /* fp16 NHWC [B][H][W][SC0] raw shortcut input or NULL (3x3 only) */
    const void* skip1;        /* fp16 NHWC [B][H][W][SC1] or NULL */
    const void* skip_weight;  /* fp16 [ceil(Cout/256)*256][SC0+SC1] */
    void* out;                /* fp16 NHWC [B][H][W][Cout]; fp32 NCHW [B][Cout][H][W] when out_nchw_f32 */
    float* stats_out;         /* optional [B*tiles][Cout][2] GroupNorm partials of the ROUNDED output,
                                 tiles = ddnm_conv16_stats_tiles(d); feeds ddnm_gn_finalize_tiles_f32 */
    float* workspace;         /* split-K slabs, ddnm_conv16_workspace_floats(d) floats (0: not needed) */
    int64_t workspace_floats;
    int32_t B, H, W;          /* OUTPUT size (= input size; the operand is H/2 x W/2 when ups) */
    int32_t Cin, Cout;
    int32_t ksize;            /* 1 or 3 */
    int32_t ups, res_ups;     /* res_ups: 3x3 launches and split-K 1x1 launches; an UNSPLIT 1x1 launch with it is refused */
    int32_t SC0, SC1;
    const void* src1;         /* fp16 NHWC [B][Hs][Ws][Cin-C0] second tensor of the concat or NULL (torch.cat, unet.py:661) */
    const float* gn_scale;    /* [B][Cin] fp32 or NULL: fused GroupNorm(+FiLM) affine of the operand (3x3 only) */
    const float* gn_shift;    /* [B][Cin] (required iff gn_scale) */
    int32_t C0;               /* channels of `src` when src1 != NULL (C0 % 64 == 0) */
    int32_t gn_silu;          /* 1: swish after the affine */
    int32_t out_nchw_f32;     /* 1: the network's output convolution (unet.py:627-631, `.type(x.dtype)` :664): 3x3,
                                 Cout <= 32 (weight packed to 32 rows or more), fp32 NCHW result, no res / skip / stats */
    int32_t reserved;
    /* Optional: finalize the CONSUMER's GroupNorm inside the split-K reduction pass.  When ddnm_conv16_fuses_fin(d)
       == 1 the launch also writes the affine of GroupNorm(fin_groups, Cout, fin_eps)(+ FiLM rows [s | t]) over ITS OWN
       OUTPUT -- scale / shift [B][Cout], what ddnm_gn_finalize_tiles_f32 would produce from stats_out -- so the
       convolution that consumes the output needs no finalize launch in between (guided_diffusion/nn.py:17-19,
       unet.py:196-205,248-251).  stats_out then holds ONE tile per image (ddnm_conv16_stats_tiles(d) == 1). */
    const float* fin_gamma;   /* [Cout] or NULL (no fused finalize) */
    const float* fin_beta;    /* [Cout] */
    const float* fin_film;    /* rows [s(0..Cout) | t(0..Cout)], row b at fin_film + b*fin_film_stride, or NULL */
    float* fin_scale;         /* [B][Cout] */
    float* fin_shift;         /* [B][Cout] */
    float fin_eps;
    int32_t fin_film_stride;
    int32_t fin_groups;
    int32_t reserved2;
} ddnm_conv16_desc;

int ddnm_conv16(const ddnm_conv16_desc* d, void* stream);
int ddnm_conv16_fuses_fin(const ddnm_conv16_desc* d);     /* 1: this launch will write fin_scale / fin_shift */
int ddnm_conv16_supported(const ddnm_conv16_desc* d);
int64_t ddnm_conv16_workspace_floats(const ddnm_conv16_desc* d);
int ddnm_conv16_stats_tiles(const ddnm_conv16_desc* d);   /* 0: this launch cannot emit stats_out */

/* HBM-bound stages of the fp16-activation path (csrc/act16.hip), all fp16 NHWC:
 *   gn_apply:  out = fp16(act(concat_c(src0, src1) * scale[b,c] + shift[b,c])), act = swish when silu (scale NULL:
 *              plain copy / concat); pool = 1 additionally averages 2x2 pixels (AvgPool2d of `down=True` ResBlocks,
 *              guided_diffusion/unet.py:237-242): out is [B][H/2][W/2][C].  Replaces GroupNorm32 + SiLU
 *              (nn.py:12-19; unet.py:196-205,226-230) and torch.cat([h, hs.pop()], 1) (unet.py:661).
 *   im2col:    col[(b*H*W + p)][tap*C + c] of a 3x3 / pad 1 convolution input with the same prologue (8x8 level).
 *   nchw_to_nhwc: fp32 NCHW [B][C][HW] -> fp16 NHWC [B][HW][cpad], zero padded (`x.type(self.dtype)`, unet.py:655).
 *   gn_stats:  per-(pixel tile, channel) sum / sum of squares of an fp16 tensor, layout of `stats_out`. */
int ddnm_gn_apply_h16(const void* src0, const void* src1, const float* scale, const float* shift, void* out, int32_t B,
                      int32_t H, int32_t W, int32_t C0, int32_t C1, int32_t silu, int32_t pool, void* stream);
int ddnm_im2col3x3_h16(const void* src0, const void* src1, const float* scale, const float* shift, void* out, int32_t B,
                       int32_t H, int32_t W, int32_t C0, int32_t C1, int32_t silu, void* stream);
int ddnm_nchw_to_nhwc_h16(const float* x, void* out, int32_t B, int32_t C, int32_t HW, int32_t cpad, void* stream);
int ddnm_gn_stats_h16(const void* src, float* stats, int32_t B, int32_t HW, int32_t C, int32_t tiles, void* stream);

/* Fused multi-head self-attention, head dim 64 (QKVAttentionLegacy, guided_diffusion/unet.py:328-354 inside
 * AttentionBlock :259-308): out[b,t,h*64+d] = sum_s softmax_s(q_t . k_s / 8) v_s[d] with
 * qkv fp16 [B][T][3C] laid out head-major (channel = h*192 + {q,k,v}*64 + d), out fp16 [B][T][C]; fp32 softmax,
 * probabilities rounded to fp16 like `.type(weight.dtype)`; no [T][T] tensor in HBM.  T % 64 == 0, C % 64 == 0. */
int ddnm_attn16_d64(const void* qkv, void* out, int32_t B, int32_t T, int32_t C, void* stream);
/* ABI 6 -- the same, also writing lse[b][h][t] = log2 sum_s exp2(q_t . k_s * log2(e) / 8) (fp32 [B][C/64][T]) for the
 * backward pass, and that backward pass (input gradient of AttentionBlock's attention inside the classifier-guidance
 * gradient, diffusion.py:183-189): dqkv fp16 [B][T][3C] in the layout of qkv from qkv, the forward output o, its
 * gradient dO (fp16 [B][T][C]) and lse; the probabilities are recomputed tile by tile, dsum [B][C/64][T] is scratch
 * (rowsum(dO . o)).  No [T][T] tensor in HBM. */
int ddnm_attn16_d64_lse(const void* qkv, void* out, float* lse, int32_t B, int32_t T, int32_t C, void* stream);
int ddnm_attn16_d64_bwd(const void* qkv, const void* o, const void* dO, const float* lse, float* dsum, void* dqkv,
                        int32_t B, int32_t T, int32_t C, void* stream);

/* ------------------------------------------------------------------------- *
 * GroupNorm statistics -> per-(sample, channel) affine for the conv prologue.
 * Replaces torch.nn.GroupNorm(32, C, eps) (models.py:32-33; guided_diffusion/nn.py:17-19).
 *   stats:    partial (sum, sumsq) per (b, chunk, group) in double, deterministic order
 *   finalize: scale[b,c] = rstd[b,g(c)]*gamma[c]; shift[b,c] = beta[c] - mean*rstd*gamma[c]
 * src is the concat of two NHWC tensors like the conv input (C1 = 0: single source).
 * ------------------------------------------------------------------------- */
int ddnm_gn_stats_f32(const float* src0, const float* src1, int32_t B, int32_t HW, int32_t C0, int32_t C1,
                      int32_t groups, double* partial /* [B][nchunk][groups][2] */, int32_t nchunk, void* stream);
int ddnm_gn_nchunk(int32_t HW, int32_t C);   /* chunk count `partial` must be sized for */
int ddnm_gn_finalize_f32(const double* partial, int32_t nchunk, const float* gamma, const float* beta,
                         int32_t B, int32_t HW, int32_t C, int32_t groups, float eps,
                         float* scale /* [B][C] */, float* shift /* [B][C] */,
                         const float* film /* optional FiLM rows [s(0..C) | t(0..C)]: GN(x)*(1+s)+t, unet.py:248-251 */,
                         int32_t film_stride, float* mean_rstd /* optional [B][groups][2], kept for backward */,
                         void* stream);

/* GroupNorm affine from the partials a convolution epilogue emitted (`stats_out`); the input may be the
 * channel concat of two tensors (part1 / tpi1 / C1, or NULL / 0 / 0). */
/* GroupNorm affine (+ swish) applied once and written as fp16 for ddnm_conv3x3_f16_f32(src_f16 = 1):
 * out[b,p,c] = fp16(act(concat_c(src0, src1)[b,p,c] * scale[b,c] + shift[b,c])), identical rounding to the fused
 * prologue.  C0 % 8 == 0, C1 % 8 == 0.  Layers with >= 256 output channels use this instead of the fused prologue,
 * which repeats the v_exp / v_rcp work once per 128-output-channel tile. */
int ddnm_gn_apply_f16(const float* src0, const float* src1, const float* scale, const float* shift, void* out_f16,
                      int32_t B, int32_t HW, int32_t C0, int32_t C1, int32_t silu, void* stream);
/* im2col of a 3x3 / stride 1 / pad 1 input with the GroupNorm affine (+ swish) prologue, fp16 output
 * col[B*H*W][9*(C0+C1)] (column = tap*C + c, zero outside the image); scale / shift may both be NULL.
 * The 8x8 level of the fp16 torso then runs as one ddnm_conv1x1_f16_f32 GEMM with K = 9*C (the (O,ky,kx,I)-packed
 * 3x3 weights ARE the [Cout][9*C] matrix).  C0 % 8 == 0, C1 % 8 == 0. */
int ddnm_im2col3x3_f16(const float* src0, const float* src1, const float* scale, const float* shift, void* out_f16,
                       int32_t B, int32_t H, int32_t W, int32_t C0, int32_t C1, int32_t silu, void* stream);
int ddnm_gn_finalize_tiles_f32(const float* part0, int32_t tiles_per_img0, int32_t C0, const float* part1,
                               int32_t tiles_per_img1, int32_t C1, const float* gamma, const float* beta, int32_t B,
                               int32_t HW, int32_t groups, float eps, float* scale, float* shift, const float* film,
                               int32_t film_stride, float* mean_rstd, void* stream);
/* The same launch additionally writes amax_out[b][g] = sqrt(max over the group's (tile, channel) partials of the sum of
 * squares) >= max |x| over the group's channels: the operand bound of ddnm_conv_desc::amax_in for the launches that read
 * the same tensor(s) RAW (a ResnetBlock's fused / un-fused nin_shortcut reads what norm1 normalises, models.py:109,
 * 115-134).  groups must equal DDNM_AMAX_N. */
int ddnm_gn_finalize_tiles_amax_f32(const float* part0, int32_t tiles_per_img0, int32_t C0, const float* part1,
                                    int32_t tiles_per_img1, int32_t C1, const float* gamma, const float* beta, int32_t B,
                                    int32_t HW, int32_t groups, float eps, float* scale, float* shift, const float* film,
                                    int32_t film_stride, float* mean_rstd, float* amax_out, void* stream);
/* Stand-alone form for raw operands that no GroupNorm reads first (Downsample / Upsample convolution inputs,
 * models.py:47-51,61-71; the attention output in front of proj_out, :183-189): out[b][i], i < DDNM_AMAX_N, bounds the
 * i-th 1/32 slice of image b's data of up to two sources.  kind 0: the fp32 tensor itself, per_image elements per image
 * (max |x|); kind 1: GroupNorm partials [tiles][C][2] of the tensor, per_image = tiles*C*2 floats (sqrt(max sum of
 * squares)).  per_image % 4 == 0; src1 may be NULL. */
int ddnm_amax_bound_f32(const float* src0, int64_t per_image0, int32_t kind0, const float* src1, int64_t per_image1,
                        int32_t kind1, float* out, int32_t B, void* stream);

/* ------------------------------------------------------------------------- *
 * Batched GEMM on MFMA f32:  C = alpha * A * op(B) + beta * D
 * A [M][K] (lda), op(B): transb=1 -> B stored [N][K] (ldb), transb=0 -> B stored [K][N];
 * batch index i -> (i / inner, i % inner); offset = outer*stride_o + inner*stride_i per operand.
 * Replaces torch.bmm / einsum in attention (models.py:171-185; unet.py:344-354) and the
 * separable A / A^+ products of SRConv (functions/svd_operators.py:853-859,893-900).
 * MFMA path: M, N multiples of 64, K multiple of 32, lda / ldb and the A / B batch strides multiples of 4, A and B
 * 16-byte aligned (128x128 tiles when M, N are multiples of 128 and the launch has >= 256 of them, else 64x64);
 * any other shape runs a scalar fallback kernel, one thread per output.  Production reaches the fallback:
 * cs_blockbased at --deg_scale 0.1 (cs = 102: N of A, K of A^+), GeneralA, and sr_averagepooling at ratio >= 8
 * when batch * sites is no multiple of 64.
 * ------------------------------------------------------------------------- */
typedef struct ddnm_gemm_desc {
    const float* A; const float* Bm; const float* D; float* C;
    int32_t M, N, K;
    int32_t lda, ldb, ldc, ldd;
    int32_t transb;
    int32_t batch, inner;                 /* batch = outer*inner */
    int64_t sAo, sAi, sBo, sBi, sCo, sCi, sDo, sDi;   /* element strides */
    float alpha, beta;
    int32_t transa;                       /* 1: A stored [K][M] (lda = pitch of that storage) */
    int32_t reserved;
} ddnm_gemm_desc;
int ddnm_bgemm_f32(const ddnm_gemm_desc* d, void* stream);

/* ------------------------------------------------------------------------- *
 * Input-gradient path of classifier guidance (guided_diffusion/diffusion.py:183-189 through
 * EncoderUNetModel, unet.py:684-895): only activation gradients are needed.
 * ------------------------------------------------------------------------- */
/* GroupNorm(+FiLM)(+SiLU) backward: dx = dL/dx for a = act(x*gn_scale + gn_shift); dA may sit behind a 2x2
 * average pool (dA_ups: [B][H/2][W/2][C], x0.25); `add` (same optional mapping) is summed in (skip branch). */
int ddnm_gn_bwd_f32(const float* x, const float* dA, int32_t dA_ups, const float* gn_scale, const float* gn_shift,
                    const float* mean_rstd, int32_t silu, const float* add, int32_t add_ups, int32_t B, int32_t H,
                    int32_t W, int32_t C, int32_t groups, double* partial /* [B][nchunk][groups][2] */, int32_t nchunk,
                    float* coef /* [B][groups][2] */, float* dx, void* stream);
int ddnm_gn_bwd_nchunk(int32_t HW, int32_t C);
/* ABI 6 -- the same for the fp16-activation classifier path (`classifier_use_fp16`, unet.py:817-823: the reference's
 * autograd then carries activations AND their gradients in fp16): x, dA, add, dx fp16 NHWC; arithmetic fp32, the two
 * group reductions fp64 in a fixed order. */
int ddnm_gn_bwd_h16(const void* x, const void* dA, int32_t dA_ups, const float* gn_scale, const float* gn_shift,
                    const float* mean_rstd, int32_t silu, const void* add, int32_t add_ups, int32_t B, int32_t H,
                    int32_t W, int32_t C, int32_t groups, double* partial /* [B][nchunk][groups][2] */, int32_t nchunk,
                    float* coef /* [B][groups][2] */, void* dx, void* stream);
/* in place on dP: dS = scale * P .* (dP - rowsum(dP .* P)) */
int ddnm_softmax_bwd_rows_f32(const float* P, float* dP, int64_t rows, int32_t n, int32_t ld, float scale, void* stream);
/* AttentionPool2d (unet.py:22-51): tokens, class-token attention (new qkv order), their backward, and the
 * gradient of log_softmax(logits)[y]. */
int ddnm_pool_tokens_f32(const float* h, const float* gn_scale, const float* gn_shift, const float* pos /* [C][HW+1] */,
                         float* X /* [B][HW+1][C] */, int32_t B, int32_t HW, int32_t C, void* stream);
int ddnm_pool_attn_fwd_f32(const float* qkv /* [B][T][3C] */, float* P /* [B][heads][T] */, float* a0 /* [B][C] */,
                           int32_t B, int32_t T, int32_t C, int32_t heads, void* stream);
int ddnm_pool_attn_bwd_f32(const float* qkv, const float* P, const float* da0, float* dqkv, int32_t B, int32_t T,
                           int32_t C, int32_t heads, void* stream);
int ddnm_pool_tokens_bwd_f32(const float* dX, float* dact /* [B][HW][C] */, int32_t B, int32_t HW, int32_t C, void* stream);
int ddnm_logsoftmax_grad_f32(const float* logits, const int64_t* y, float* dlogits, int32_t B, int32_t N, void* stream);
/* ABI 6 -- token construction / its backward over an fp16 NHWC activation (tokens and their gradient stay fp32) */
int ddnm_pool_tokens_h16(const void* h, const float* gn_scale, const float* gn_shift, const float* pos /* [C][HW+1] */,
                         float* X /* [B][HW+1][C] */, int32_t B, int32_t HW, int32_t C, void* stream);
int ddnm_pool_tokens_bwd_h16(const float* dX, void* dact /* fp16 [B][HW][C] */, int32_t B, int32_t HW, int32_t C, void* stream);

/* ABI 7 -- fused single-head self-attention of the celeba `Model`'s AttnBlock (guided_diffusion/models.py:171-185: the two
 * torch.bmm and the softmax between them): qkv = [B][T][3C] fp32 (q | k | v per token, the output of the fused
 * q / k / v 1x1 convolution), out = [B][T][C] fp32 = softmax_j(q_i . k_j * softmax_scale) v_j.  No [T][T] tensor in HBM.
 * Split-fp16 products (hi*hi' + hi*lo' + lo*hi', fp32 accumulate) like ddnm_conv3x3_s16_f32; s_qk / s_v = powers of two with
 * max|q|, max|k| <= 2^15 / s_qk and max|v| <= 2^15 / s_v (the host derives them once per checkpoint from a static bound of the
 * convolution's output; scores / outputs are multiplied by the inverse powers: exact).  T % 32 == 0, T <= 256, C % 128 == 0,
 * C <= 512. */
int ddnm_attn_fused_f32(const float* qkv, float* out, int32_t B, int32_t T, int32_t C, float s_qk, float s_v,
                        float softmax_scale, void* stream);
int ddnm_attn_fused_supported(int32_t T, int32_t C);

/* Row softmax in place: x[r][0..n) <- softmax(scale * x[r][:]); rows contiguous with ld. */
int ddnm_softmax_rows_f32(float* x, int64_t rows, int32_t n, int32_t ld, float scale, void* stream);

/* ------------------------------------------------------------------------- *
 * Small dense layers on the embedding path (models.py:216-222,306-308,92,121).
 *   y[b][n] = bias[n] + sum_k W[n][k] * act(x[b][k]),  act = swish if silu_in else id
 * ------------------------------------------------------------------------- */
int ddnm_linear_f32(const float* x, const float* W, const float* bias, float* y, int32_t B, int32_t K,
                    int32_t N, int32_t silu_in, void* stream);
/* Sinusoidal embedding: emb[b][i] = f(t[b]*freq[i]); order 0: [sin, cos] (models.py:6-24),
 * order 1: [cos, sin] (guided_diffusion/nn.py:103-121).  freq [half] is computed on the host. */
int ddnm_timestep_embedding_f32(const float* t, const float* freq, float* emb, int32_t B, int32_t half,
                                int32_t order, void* stream);

/* out = mean_2x2(act(in)) on NHWC, act = optional per-(b,c) affine (+swish): the two halves of a
 * `down=True` ResBlock (guided_diffusion/unet.py:133-140,237-242).  in is [B][2Ho][2Wo][C]. */
int ddnm_avgpool2_nhwc_f32(const float* in, const float* gn_scale, const float* gn_shift, int32_t silu, float* out,
                           int32_t B, int32_t Ho, int32_t Wo, int32_t C, void* stream);
/* emb[b][:] += table[idx[b]][:]  (class-label embedding, guided_diffusion/unet.py:651-653); idx is int64; `rows` =
 * rows of `table`: a label outside [0, rows) poisons its row with NaN instead of reading out of bounds. */
int ddnm_embedding_add_f32(float* emb, const float* table, const int64_t* idx, int32_t B, int32_t D, int32_t rows,
                           void* stream);

/* NCHW [B][C][H][W] -> NHWC [B][H][W][Cpad], channels >= C zero filled. */
int ddnm_nchw_to_nhwc_pad_f32(const float* src, float* dst, int32_t B, int32_t C, int32_t HW, int32_t Cpad,
                              void* stream);
/* im2col of the 3-channel network input for the 3x3 / pad 1 input convolution (models.py:225, unet.py:472-476):
 * dst[b][y][x][(ky*3+kx)*C + c] = src[b][c][y+ky-1][x+kx-1] (0 outside the image and for entries >= 9*C), so that
 * conv_in is ONE 32-wide K chunk (a 1x1 convolution over 27 real entries) instead of 9 taps x 32 padded channels. */
int ddnm_nchw_im2col3x3_pad_f32(const float* src, float* dst, int32_t B, int32_t C, int32_t H, int32_t W, int32_t Cpad,
                                void* stream);

/* ------------------------------------------------------------------------- *
 * DDNM sampler step (functions/svd_ddnm.py:57-65,74; guided_diffusion/diffusion.py:365-384).
 * Images are NCHW fp32 [B][3][H][W].  Scalars are the host-computed alpha-bar terms:
 *   x0   = (xt - et*sqrt(1-at)) / sqrt(at)                       (svd_ddnm.py:57)
 *   x0h  = x0 - lambda * A^+(A x0 - y)                           (svd_ddnm.py:59-61)
 *   xt'  = sqrt(at') * x0h + gamma*(c1*noise + c2*et)            (svd_ddnm.py:63-65)
 * `et` may have row stride et_bstride (6-channel learn_sigma heads: first 3 used, :54-55).
 * ------------------------------------------------------------------------- */
typedef struct ddnm_step_scalars {
    float sqrt_1m_at;     /* sqrt(1 - alpha_bar_t) */
    float sqrt_at;        /* sqrt(alpha_bar_t), applied as a true division */
    float sqrt_at_next;   /* sqrt(alpha_bar_{t'}) */
    float c1, c2;         /* noise / eps mixing coefficients (already multiplied by gamma) */
    float lambda;         /* 1 for DDNM (sigma_y = 0) */
    /* ABI 6 -- in-kernel noise: when a step entry point gets noise == NULL and rng_on != 0, the N(0, I) draw of
     * `torch.randn_like(x)` (svd_ddnm.py:65) happens inside the kernel: Philox4x32-10 + Box-Muller with the counter
     * (element / 4, rng_iter, rng_image_base + b, 0) and the key (rng_seed_lo, rng_seed_hi) -- no noise tensor is written
     * or read, and an image's noise depends on its GLOBAL index only (rank-count independent sharding).
     * ddnm_randn_philox_f32 produces the same values as a tensor. */
    uint32_t rng_on;
    uint32_t rng_seed_lo, rng_seed_hi;
    uint32_t rng_iter;        /* loop iteration k */
    uint32_t rng_image_base;  /* global index of image 0 of this launch */
    uint32_t reserved_rng;
} ddnm_step_scalars;


/* out [B][chw] fp32 = the Philox draw described above (chw % 4 == 0) */
int ddnm_randn_philox_f32(float* out, int32_t B, int64_t chw, uint32_t seed_lo, uint32_t seed_hi, uint32_t iter,
                          uint32_t image_base, void* stream);

/* Per-image Philox keys (a batch of independently seeded images in one launch).  rng_keys is a DEVICE table [B][4] of
 * uint32 {key_lo, key_hi, image_ctr, 0} (16-byte aligned): image b draws element r of loop iteration `iter` as
 * philox_normal4({key_lo, key_hi}, r / 4, iter, image_ctr)[r % 4] -- rows {seed_lo, seed_hi, image_base + b, 0}
 * reproduce ddnm_randn_philox_f32 and the in-kernel draw of the unkeyed step entry points bit for bit.
 * out [B][n]: any n >= 1; the last partial block of four writes its first n % 4 values only. */
int ddnm_randn_philox_keyed_f32(float* out, int32_t B, int64_t n, const uint32_t* rng_keys, uint32_t iter,
                                void* stream);
/* Keyed step entry points: the arguments of the unkeyed ones with `rng_keys` in place of `noise`; the noise is always
 * drawn in-kernel (s->rng_iter = loop iteration; s->rng_on and s->rng_seed_* / rng_image_base are not read). */
int ddnm_step_combine_keyed_f32(const float* x0, const float* proj, const float* apy, const uint32_t* rng_keys,
                                const float* et, int64_t et_bstride, float* xt_next, int32_t B, int64_t chw,
                                const ddnm_step_scalars* s, void* stream);
int ddnm_step_sr_avgpool_keyed_f32(const float* xt, const float* et, int64_t et_bstride, const uint32_t* rng_keys,
                                   const float* y, float* x0, float* xt_next, int32_t B, int32_t H, int32_t W,
                                   int32_t r, const ddnm_step_scalars* s, void* stream);
int ddnm_step_color_keyed_f32(const float* xt, const float* et, int64_t et_bstride, const uint32_t* rng_keys,
                              const float* y, float* x0, float* xt_next, int32_t B, int32_t HW,
                              const float* w3_host, const ddnm_step_scalars* s, void* stream);
int ddnm_step_inpaint_keyed_f32(const float* xt, const float* et, int64_t et_bstride, const uint32_t* rng_keys,
                                const float* y, const int32_t* rank, int32_t n_kept, float* x0, float* xt_next,
                                int32_t B, int32_t HW, const ddnm_step_scalars* s, void* stream);
int ddnm_step_denoise_keyed_f32(const float* xt, const float* et, int64_t et_bstride, const uint32_t* rng_keys,
                                const float* y, float* x0, float* xt_next, int32_t B, int64_t chw,
                                const ddnm_step_scalars* s, void* stream);

/* x0 only (first half of every step; also feeds time travel). */
int ddnm_step_x0_f32(const float* xt, const float* et, int64_t et_bstride, float* x0, int32_t B, int64_t chw,
                     const ddnm_step_scalars* s, void* stream);
/* xt' = sqrt_at_next*(x0 - lambda*(proj - apy)) + c1*noise + c2*et
 * proj = A^+ A x0 and apy = A^+ y (constant over the run), or proj = A^+(A x0 - y) with apy = NULL. */
int ddnm_step_combine_f32(const float* x0, const float* proj, const float* apy, const float* noise,
                          const float* et, int64_t et_bstride, float* xt_next, int32_t B, int64_t chw,
                          const ddnm_step_scalars* s, void* stream);
/* Fused single-pass steps (x0 written too, for time travel): */
int ddnm_step_sr_avgpool_f32(const float* xt, const float* et, int64_t et_bstride, const float* noise,
                             const float* y /* [B][3][H/r][W/r] */, float* x0, float* xt_next, int32_t B,
                             int32_t H, int32_t W, int32_t r, const ddnm_step_scalars* s, void* stream);
/* w3_host: HOST pointer to the 3 per-pixel weights, NULL = (0.3333, 0.3334, 0.3333) of
 * svd_operators.py:632; the simplified path uses (1/3, 1/3, 1/3) (diffusion.py:33-42). */
int ddnm_step_color_f32(const float* xt, const float* et, int64_t et_bstride, const float* noise,
                        const float* y /* [B][H*W] */, float* x0, float* xt_next, int32_t B, int32_t HW,
                        const float* w3_host, const ddnm_step_scalars* s, void* stream);
int ddnm_step_inpaint_f32(const float* xt, const float* et, int64_t et_bstride, const float* noise,
                          const float* y /* [B][3*n_kept], HWC order of kept pixels */,
                          const int32_t* rank /* [HW]: index of pixel among kept ones, -1 if missing */,
                          int32_t n_kept, float* x0, float* xt_next, int32_t B, int32_t HW,
                          const ddnm_step_scalars* s, void* stream);
int ddnm_step_denoise_f32(const float* xt, const float* et, int64_t et_bstride, const float* noise,
                          const float* y, float* x0, float* xt_next, int32_t B, int64_t chw,
                          const ddnm_step_scalars* s, void* stream);
/* Inpainting with one mask PER IMAGE ("pi"; functions/svd_operators.py:324-359 and guided_diffusion/diffusion.py:463-471
 * applied to each image with its own mask -- the reference holds one mask per run):
 *   rank: int32 [B][HW], row b = image b's table (pixel -> index among ITS kept pixels, -1 = missing);
 *   y:    fp32 [B][y_stride], row b holds 3*n_kept[b] HWC-interleaved entries, the rest is padding (never read);
 *   n_kept_max: largest n_kept of the batch (validation only).
 * DDNM_E_SHAPE unless HW % 4 == et_bstride % 4 == y_stride % 4 == 0, n_kept_max >= 1 and y_stride >= 3*n_kept_max.
 * Same kernel as ddnm_step_inpaint_f32 / _keyed_f32 (which are its rank row stride 0, y row stride 3*n_kept case). */
int ddnm_step_inpaint_pi_f32(const float* xt, const float* et, int64_t et_bstride, const float* noise, const float* y,
                             int64_t y_stride, const int32_t* rank, int32_t n_kept_max, float* x0, float* xt_next,
                             int32_t B, int32_t HW, const ddnm_step_scalars* s, void* stream);
int ddnm_step_inpaint_pi_keyed_f32(const float* xt, const float* et, int64_t et_bstride, const uint32_t* rng_keys,
                                   const float* y, int64_t y_stride, const int32_t* rank, int32_t n_kept_max, float* x0,
                                   float* xt_next, int32_t B, int32_t HW, const ddnm_step_scalars* s, void* stream);
/* time-travel re-noise: xt' = a*x0 + b*noise  (svd_ddnm.py:74) */
int ddnm_renoise_f32(const float* x0, const float* noise, float* xt_next, int64_t n, float a, float b, void* stream);

/* ---- DDNM+ (sigma_y > 0, functions/svd_ddnm.py:80-164) building blocks --------------------------------- */
/* out = a*x + b*y (y may be NULL) */
int ddnm_axpby_f32(const float* x, const float* y, float* out, int64_t n, float a, float b, void* stream);
/* out[b][i] = a*x[b*x_bstride + i] + b*y[b*chw + i]  (guided eps: eps[:, :3] - sqrt(1-abar)*grad, svd_ddnm.py:51-52) */
int ddnm_axpby_strided_f32(const float* x, int64_t x_bstride, const float* y, float* out, int32_t B, int64_t chw,
                           float a, float b, void* stream);
/* out[i] = value for i < n (padding rows of token matrices; replaces tensor.zero_() / fill_() on the path). */
int ddnm_fill_f32(float* out, int64_t n, float value, void* stream);
/* out = (m ? cx_m : cx_n)*x + (m ? cy_m : cy_n)*y with m = mask[plane % planes_mask][p] != 0 (mask NULL: all measured):
 * Lambda / Lambda_noise of Inpainting (svd_operators.py:361-439), spectral weights of WalshHadamardCS (:253-320). */
int ddnm_mask_mix_f32(const float* x, const float* y, const float* mask, int32_t planes_mask, int64_t plane_elems,
                      float* out, int64_t total, float cx_m, float cx_n, float cy_m, float cy_n, void* stream);
/* Matrix-free SVD surface of the operators (A_functions.V / Vt / U / Ut / add_zeros / At / A_pinv_eta,
 * functions/svd_operators.py:9-97; not on the sampling hot path):
 *   gather_scale: out[b][i] = (idx[i] >= 0 ? in[b][idx[i]] : 0) * (scale ? scale[i] : 1); idx NULL = identity padded with
 *                 zeros up to n_out (`add_zeros`, and with `scale` the `singulars * temp[:, :n]` products);
 *   site_matmul:  out[b][s][i] = sum_j Mop[i][j] in[b][s][j] with Mop = M (trans 0) or M^T, n <= 16, element (b,s,j) at
 *                 b*sb + s*ss + j*sj in both tensors (the V_small / Vt_small products, :490-517,636-656); in != out. */
int ddnm_gather_scale_f32(const float* in, const int32_t* idx, const float* scale, float* out, int32_t B, int64_t n_in,
                          int64_t n_out, void* stream);
int ddnm_site_matmul_f32(const float* in, const float* M, float* out, int32_t B, int64_t sites, int32_t n, int64_t sb,
                         int64_t ss, int64_t sj, int32_t trans, void* stream);
/* Per-site spectral ops with the n x n orthogonal V (device, row-major) of a 1 x n measurement row:
 * mode 0 = r x r patches of [B*C][H][W] planes (SuperResolution, :535-623), mode 1 = RGB needles (Colorization, :669-736);
 * op 0: out = x + (c0-1) V[:,0] (V[:,0].x)  (Lambda, c0 = lambda of the measured direction);
 * op 1: out = V (d1 .* x_raw + d2 .* y_raw), d1 = (c0, c1, c1, ...), d2 = (c2, c3, c3, ...)  (Lambda_noise). */
int ddnm_site_spectral_f32(const float* x, const float* y, const float* V, int32_t n, int32_t mode, int32_t r,
                           int32_t B, int32_t C, int32_t H, int32_t W, float* out, int32_t op, float c0, float c1,
                           float c2, float c3, void* stream);

/* out = x .* table[plane % planes_table][p]: spectral gains of Deblurring / Deblurring2D (svd_operators.py:934-1165) */
int ddnm_mul_planes_f32(const float* x, const float* table, int32_t planes_table, int64_t plane_elems, float* out,
                        int64_t total, void* stream);

/* DDNM+ spectral weights of Deblurring (svd_operators.py:1016-1091) applied in the (V1^T . V1) spectral plane:
 * mode 0: out = x .* lambda(s[p]); mode 1: out = x .* d1(s[p]) + y .* d2(s[p]); s = un-thresholded s1_i*s1_j table
 * [plane_elems], p = i % plane_elems; lambda/d1/d2 as in svd_ddnm.py:121-131 (see ddnm_step.hip). */
int ddnm_spectral_mix_f32(const float* x, const float* y, const float* singulars, int64_t plane_elems, float* out,
                          int64_t total, float a, float sigma_y, float sigma_t, float eta, int32_t mode, void* stream);

/* One fused DDNM+ step (svd_ddnm.py:118-131) in the spectral planes x^ = Vl^T X Vr of an operator with a separable SVD
 * (SRConv, Deblurring2D), all tensors [B][C][plane] contiguous:
 *   x^_0 = (xt_hat - et_hat * sqrt_1m_at) / sqrt_at
 *   out_hat = a * (x^_0 - mu .* (x^_0 - y_hat)) + d1 .* n + d2 .* et_hat,   a = s->sqrt_at_next, n ~ N(0, I)
 * (lambda, d1, d2) per entry of the THRESHOLDED gain table by the rule of ddnm_spectral_mix_f32, mu = lambda where the
 * gain is > 0 and 0 in the null space; y_hat = g^+ .* (Ul^T Y Ur), zero where g = 0.  gains [C][plane] with channel
 * stride gains_cstride (0: one table for all channels).  noise: a tensor [B][C*plane], or NULL with s->rng_on (drawn
 * in-kernel, counter (r / 4, rng_iter, rng_image_base + b, 0), r = index inside the image: the values of
 * ddnm_randn_philox_f32 on [B][C*plane]); the keyed form takes the per-image key table instead.  out_hat may alias
 * xt_hat.  plane % 4 != 0 or gains_cstride % 4 != 0: DDNM_E_SHAPE. */
int ddnm_step_plus_spectral_f32(const float* xt_hat, const float* et_hat, const float* y_hat, const float* gains,
                                int64_t gains_cstride, const float* noise, float* out_hat, int32_t B, int32_t C,
                                int64_t plane, float sigma_y, float sigma_t, float eta, const ddnm_step_scalars* s,
                                void* stream);
int ddnm_step_plus_spectral_keyed_f32(const float* xt_hat, const float* et_hat, const float* y_hat, const float* gains,
                                      int64_t gains_cstride, const uint32_t* rng_keys, float* out_hat, int32_t B,
                                      int32_t C, int64_t plane, float sigma_y, float sigma_t, float eta,
                                      const ddnm_step_scalars* s, void* stream);

/* Stand-alone operator kernels (A and A^+ of functions/svd_operators.py, direct form). */
int ddnm_op_avgpool_f32(const float* x, float* y, int32_t BC, int32_t H, int32_t W, int32_t r, void* stream);
int ddnm_op_upsample_f32(const float* y, float* x, int32_t BC, int32_t H, int32_t W, int32_t r, void* stream);
int ddnm_op_color_A_f32(const float* x, float* y, int32_t B, int32_t HW, const float* w3_host, void* stream);
int ddnm_op_color_pinv_f32(const float* y, float* x, int32_t B, int32_t HW, const float* w3_host, void* stream);
int ddnm_op_inpaint_A_f32(const float* x, const int32_t* rank, int32_t n_kept, float* y, int32_t B, int32_t HW,
                          void* stream);
int ddnm_op_inpaint_pinv_f32(const float* y, const int32_t* rank, int32_t n_kept, float* x, int32_t B,
                             int32_t HW, void* stream);
/* A and A^+ of inpainting with one mask per image (functions/svd_operators.py:324-359, guided_diffusion/diffusion.py:463-471;
 * layout and validation as ddnm_step_inpaint_pi_f32).  A writes the 3*n_kept[b] entries of row b only: the caller clears
 * the padding; A^+ does not read it. */
int ddnm_op_inpaint_A_pi_f32(const float* x, const int32_t* rank, int32_t n_kept_max, float* y, int64_t y_stride,
                             int32_t B, int32_t HW, void* stream);
int ddnm_op_inpaint_pinv_pi_f32(const float* y, int64_t y_stride, const int32_t* rank, int32_t n_kept_max, float* x,
                                int32_t B, int32_t HW, void* stream);
/* Orthonormal 2-D separable Walsh-Hadamard transform H_n (x) H_n of each [n][n] plane
 * (== the 1-D natural-order FWHT over n*n points of svd_operators.py:212-222), n in {32,...,256}.
 * mask (optional, [planes_mask][n*n], plane p uses mask[(p % planes_mask)]) multiplies the
 * spectrum between a forward and an inverse transform: out = H (mask .* (H in)). */
int ddnm_fwht2d_f32(const float* in, float* out, int32_t planes, int32_t n, void* stream);
int ddnm_fwht2d_masked_f32(const float* in, const float* mask, int32_t planes_mask, float* out,
                           int32_t planes, int32_t n, float* scratch /* planes*n*n */, void* stream);
/* gather/scatter between the permuted (k, c)-interleaved measurement vector and WH planes */
int ddnm_wh_gather_f32(const float* planes, const int32_t* perm, float* y, int32_t B, int32_t C, int32_t N,
                       int32_t n_keep, void* stream);
int ddnm_wh_scatter_f32(const float* y, const int32_t* perm, float* planes, int32_t B, int32_t C, int32_t N,
                        int32_t n_keep, void* stream);

/* Block-based CS, svd_operators.py:101-159: every ps x ps patch of every plane [planes][D][D] becomes one row of
 * patches[planes*(D/ps)^2][ps*ps] (row = plane, py, px; column = i*ps + j), inverse = 1 scatters the rows back.
 * Vt_small / V_small (:108-109) then act as one ddnm_bgemm_f32 over all patches.  D % ps == 0, ps % 4 == 0. */
int ddnm_patchify_f32(const float* src, float* dst, int32_t planes, int32_t D, int32_t ps, int32_t inverse, void* stream);

/* One fused DDNM+ step (functions/svd_ddnm.py:118-131) of block-based CS (svd_operators.py:101-159), per ps x ps patch.
 * All singular values are 1, so with M = Vt_small[:cs] (orthonormal rows), a = s->sqrt_at_next, sigma_t = sqrt(1 - abar_t'),
 * (lambda, d1r, d2r) the spectral coefficients of singular value 1, (1, d1n, d2n) those of the null space, n ~ N(0, I):
 *   x0      = (xt - et * sqrt_1m_at) / sqrt_at
 *   w       = -a lambda x0 + (d1r - d1n) n + (d2r - d2n) et                 patch layout [B*C*(D/ps)^2][ps*ps]
 *   x_{t-1} = a x0 + d1n n + d2n et + a lambda A^+y + unpatch((w M^T) M)
 * which is a (x0 - Lambda A^+ (A x0 - y)) + V (d1 .* V^T n + d2 .* V^T et).  `pre` makes one pass over [B][C][D][D]: it
 * writes x0 into x0_out, the image-order terms of x_{t-1} into xt_next and w at the positions of ddnm_patchify_f32; the
 * caller then forms P = (w M^T) M with two ddnm_bgemm_f32 launches and `post` adds it: xt_next[img] += P[patch].
 * a_lambda = a*lambda, dd1 = d1r - d1n, dd2 = d2r - d2n are evaluated on the host.  et row b at et + b*et_bstride (the
 * [:, :3] view of a 6-channel output); aty = A^+ y, [B][C][D][D].  noise: a tensor [B][C*D*D], or NULL with s->rng_on
 * (drawn in-kernel at the image-order index, counter (r / 4, rng_iter, rng_image_base + b, 0), r = index inside the
 * image: the values of ddnm_randn_philox_f32 on [B][C*D*D]); the keyed form takes the per-image key table instead.
 * NULL pointer / non-positive size: DDNM_E_BADARG; D % ps, ps % 4 or et_bstride % 4 != 0: DDNM_E_SHAPE; no output may
 * alias an input or another output (xt_next == xt, et or x0_out; P == xt_next): DDNM_E_BADARG. */
int ddnm_step_plus_cs_pre_f32(const float* xt, const float* et, int64_t et_bstride, const float* noise, const float* aty,
                              float* x0_out, float* xt_next, float* w, int32_t B, int32_t C, int32_t D, int32_t ps,
                              float a_lambda, float d1n, float d2n, float dd1, float dd2, const ddnm_step_scalars* s,
                              void* stream);
int ddnm_step_plus_cs_pre_keyed_f32(const float* xt, const float* et, int64_t et_bstride, const uint32_t* rng_keys,
                                    const float* aty, float* x0_out, float* xt_next, float* w, int32_t B, int32_t C,
                                    int32_t D, int32_t ps, float a_lambda, float d1n, float d2n, float dd1, float dd2,
                                    const ddnm_step_scalars* s, void* stream);
int ddnm_step_plus_cs_post_f32(const float* P, float* xt_next, int32_t planes, int32_t D, int32_t ps, void* stream);

/* ------------------------------------------------------------------------- *
 * Demosaicing: one colour sample per pixel behind a colour filter array (CFA).  The operator is the reference's
 * Inpainting(channels, img_dim, missing_indices, device) (functions/svd_operators.py:324-439) with the indices 3p + c
 * of the two channels c that pixel p does NOT sample: y[b][p] = x[b][cfa(p)][p] in pixel order, A^+ the scatter back,
 * every singular value 1.  Added under ABI 7 like the *_pi_* entry points: new symbols only.
 *   pattern_host: HOST pointer to ph * pw channel codes, row-major (0 = R, 1 = G, 2 = B), 1 <= ph, pw <= 8; pixel (r, c)
 *                 samples channel pattern_host[(r % ph) * pw + c % pw].  It is copied by value into the kernel
 *                 arguments (like w3_host); no device table exists.
 *   x [B][3][H][W], y [B][H*W], et row b at et + b*et_bstride (the [:, :3] view of a 6-channel output).
 * NULL pointer (pattern_host included), B, H or W <= 0, no noise source: DDNM_E_BADARG; then H % 4, W % 4 or
 * et_bstride % 4 != 0, ph or pw outside 1..8, a code above 2: DDNM_E_SHAPE.  All of it is checked before any launch.
 * ------------------------------------------------------------------------- */
/* A and A^+ (functions/svd_operators.py:324-439: A :52-58 with V^T / U of :339-350; the DDNM+ loop of
 * functions/svd_ddnm.py:80-164 applies them through ddnm_step_plus_mosaic_f32 instead). */
int ddnm_op_mosaic_A_f32(const float* x, float* y, int32_t B, int32_t H, int32_t W, const uint8_t* pattern_host,
                         int32_t ph, int32_t pw, void* stream);
int ddnm_op_mosaic_pinv_f32(const float* y, float* x, int32_t B, int32_t H, int32_t W, const uint8_t* pattern_host,
                            int32_t ph, int32_t pw, void* stream);
/* Fused noise-free step (functions/svd_ddnm.py:57-65 with the operator of functions/svd_operators.py:324-439; the
 * sigma_y > 0 loop of functions/svd_ddnm.py:80-164 takes ddnm_step_plus_mosaic_f32): one thread per four consecutive
 * pixels of all three planes and one float4 of y,
 *   x0 = (xt - et * sqrt_1m_at) / sqrt_at;   x0h = x0 - (x0 - y) * lambda on the plane a pixel samples, x0 elsewhere;
 *   xt' = sqrt_at_next * x0h + c1 * noise + c2 * et.
 * x0 (optional) receives the uncorrected x0; noise as in ddnm_step_inpaint_f32 / _keyed_f32. */
int ddnm_step_mosaic_f32(const float* xt, const float* et, int64_t et_bstride, const float* noise, const float* y,
                         float* x0, float* xt_next, int32_t B, int32_t H, int32_t W, const uint8_t* pattern_host,
                         int32_t ph, int32_t pw, const ddnm_step_scalars* s, void* stream);
int ddnm_step_mosaic_keyed_f32(const float* xt, const float* et, int64_t et_bstride, const uint32_t* rng_keys,
                               const float* y, float* x0, float* xt_next, int32_t B, int32_t H, int32_t W,
                               const uint8_t* pattern_host, int32_t ph, int32_t pw, const ddnm_step_scalars* s,
                               void* stream);
/* The whole DDNM+ step (functions/svd_ddnm.py:80-164, step :118-131) with Lambda / Lambda_noise of
 * functions/svd_operators.py:324-439 (:361-439), in ONE launch: the operator is diagonal in the image.  With
 * a = s->sqrt_at_next, n ~ N(0, I), (lambda, d1r, d2r) the spectral coefficients of singular value 1 and (1, d1n, d2n) those
 * of the null space,
 *   x0      = (xt - et * sqrt_1m_at) / sqrt_at                        -> x0_out, uncorrected (required)
 *   x_{t-1} = a x0 - a lambda (x0 - y) + d1r n + d2r et               on the plane a pixel samples
 *   x_{t-1} = a x0 + d1n n + d2n et                                   on the other two
 * a_lambda = a*lambda, dd1 = d1r - d1n, dd2 = d2r - d2n come from the host, as for ddnm_step_plus_cs_pre_f32; the noise
 * sources are those of that entry point (tensor [B][3*H*W], in-kernel draw, or the keyed table). */
int ddnm_step_plus_mosaic_f32(const float* xt, const float* et, int64_t et_bstride, const float* noise, const float* y,
                              float* x0_out, float* xt_next, int32_t B, int32_t H, int32_t W,
                              const uint8_t* pattern_host, int32_t ph, int32_t pw, float a_lambda, float d1n, float d2n,
                              float dd1, float dd2, const ddnm_step_scalars* s, void* stream);
int ddnm_step_plus_mosaic_keyed_f32(const float* xt, const float* et, int64_t et_bstride, const uint32_t* rng_keys,
                                    const float* y, float* x0_out, float* xt_next, int32_t B, int32_t H, int32_t W,
                                    const uint8_t* pattern_host, int32_t ph, int32_t pw, float a_lambda, float d1n,
                                    float d2n, float dd1, float dd2, const ddnm_step_scalars* s, void* stream);

/* ------------------------------------------------------------------------- *
 * DDNM+ with per-entry measurement noise ("hn": heteroscedastic noise) for the mosaic and for denoising.  Added under
 * ABI 7: new symbols only; ddnm_step_scalars keeps its size, the noise model travels in the arguments.
 * Both operators have U = I and singular value 1 on every measured entry (functions/svd_operators.py:324-439 over
 * single entries, :442-476), so a diagonal noise covariance diag(sigma_j^2) is diagonal in their spectral basis and the
 * per-singular-value rules the reference spells out with change_index masks (svd_operators.py:367-436; the step is
 * functions/svd_ddnm.py:118-131) hold per entry j with sigma_y -> sigma_j.  With a = s->sqrt_at_next, thr = a sigma_j:
 *   sigma_j == 0 or a == 0 : (a lambda, d1, d2) = (a, c1, c2)
 *   sigma_t < thr          : (a * (c2 / thr), c1, 0)
 *   sigma_t > thr          : (a, sqrt(max(sigma_t2 - thr * thr, 0)), 0)
 *   sigma_t == thr         : (a, c1, c2)
 *   x0      = (xt - et * sqrt_1m_at) / sqrt_at                        -> x0_out, uncorrected (required)
 *   x_{t-1} = ((a x0 - a lambda (x0 - y)) + d1 n) + d2 et             measured entries
 *   x_{t-1} = ((a x0 - 0 (x0 - y)) + c1 n) + c2 et                    the two planes a mosaic pixel does not sample
 * in fp32, one rounding per operation, in that order.  sigma_t, sigma_t2 = sigma_t^2, c1 = sigma_t eta and
 * c2 = sigma_t sqrt(1 - eta^2) come from the host (evaluated in double); s->c1, s->c2 and s->lambda are not read.
 *   sigma_mode 0 (map):  sigma_j = sigma_map[j], a DEVICE row on the engine's [-1, 1] scale (twice the [0, 1] value),
 *                        16-byte aligned, H*W (mosaic) or chw (denoising) entries, shared by every image of the batch;
 *                        s2 and g are ignored.
 *   sigma_mode 1 (shot): sigma_j = 2 sqrt(s2 + g u_j), u_j = clamp((y_j + 1) / 2, 0, 1): read variance s2 and shot gain g
 *                        on the [0, 1] scale, the intensity taken from the measurement itself; sigma_map is ignored.
 * Noise sources, et and the mosaic's pattern_host as for ddnm_step_plus_mosaic_f32.  NULL pointer (the row in map mode
 * included, or a misaligned one), non-positive size, no noise source: DDNM_E_BADARG; then H % 4, W % 4, chw % 4 or
 * et_bstride % 4 != 0, a bad pattern, a sigma_mode other than 0 / 1, a negative or non-finite s2, g (shot mode),
 * sigma_t or sigma_t2, a non-finite c1 or c2: DDNM_E_SHAPE.  All of it is checked before any launch.
 * ------------------------------------------------------------------------- */
int ddnm_step_plus_mosaic_hn_f32(const float* xt, const float* et, int64_t et_bstride, const float* noise, const float* y,
                                 float* x0_out, float* xt_next, int32_t B, int32_t H, int32_t W,
                                 const uint8_t* pattern_host, int32_t ph, int32_t pw, const float* sigma_map,
                                 int32_t sigma_mode, float s2, float g, float sigma_t, float sigma_t2, float c1, float c2,
                                 const ddnm_step_scalars* s, void* stream);
int ddnm_step_plus_mosaic_hn_keyed_f32(const float* xt, const float* et, int64_t et_bstride, const uint32_t* rng_keys,
                                       const float* y, float* x0_out, float* xt_next, int32_t B, int32_t H, int32_t W,
                                       const uint8_t* pattern_host, int32_t ph, int32_t pw, const float* sigma_map,
                                       int32_t sigma_mode, float s2, float g, float sigma_t, float sigma_t2, float c1,
                                       float c2, const ddnm_step_scalars* s, void* stream);
int ddnm_step_plus_denoise_hn_f32(const float* xt, const float* et, int64_t et_bstride, const float* noise, const float* y,
                                  float* x0_out, float* xt_next, int32_t B, int64_t chw, const float* sigma_map,
                                  int32_t sigma_mode, float s2, float g, float sigma_t, float sigma_t2, float c1, float c2,
                                  const ddnm_step_scalars* s, void* stream);
int ddnm_step_plus_denoise_hn_keyed_f32(const float* xt, const float* et, int64_t et_bstride, const uint32_t* rng_keys,
                                        const float* y, float* x0_out, float* xt_next, int32_t B, int64_t chw,
                                        const float* sigma_map, int32_t sigma_mode, float s2, float g, float sigma_t,
                                        float sigma_t2, float c1, float c2, const ddnm_step_scalars* s, void* stream);

/* ------------------------------------------------------------------------- *
 * Old-photo restoration: mask, then grey, then r x r average pool in ONE operator -- the A of the simplified path's
 * mask_color_sr (guided_diffusion/diffusion.py:260-290) with its exact pseudo-inverse (the reference chains
 * mask . colour . upsample there, which is no pseudo-inverse on a site the mask cuts).  Added under ABI 7: new symbols only.
 * Site j is an r x r block, k_j the number of its kept pixels (mask 1), |w|^2 = sum_c w_c^2:
 *   y_j          = sum_c sum_{p in j} w_c m_p x[c][p] / r^2
 *   s_j          = sqrt(k_j) |w| / r^2                  (k_j = 0: s_j = 0, the site is null space and y_j is ignored)
 *   q_j[c][p]    = w_c m_p / (sqrt(k_j) |w|)            (the rows of A have disjoint supports: A A^T is diagonal, U = I)
 *   (A^+ y)[c][p] = m_p w_c r^2 y_j / (k_j |w|^2)       (0 on sites with k_j = 0)
 *   x [B][3][H][W], y [B][H/r][W/r], et row b at et + b*et_bstride (the [:, :3] view of a 6-channel output).
 *   mask:    device plane [H*W] of 0 / 1 floats shared by all images; NULL = everything kept (sr_color; nothing is loaded).
 *   w3_host: HOST pointer to the three grey weights, copied by value into the kernel arguments (required).
 * The kernels count k_j from the mask and derive s_j and q_j themselves: no per-site table exists.  One lane owns a
 * strip of r rows x 4 pixels x 3 planes; at r = 8 two neighbouring lanes add their halves of a site (one shuffle, fixed
 * order), so an image gives the same bits alone and inside any batch.
 * NULL pointer (mask, and x0 of the noise-free step, aside), B <= 0, no noise source, a misaligned key table, w all zero, or
 * an output that is xt, et or the other output: DDNM_E_BADARG; then r not in {1, 2, 4, 8}, H or W <= 0, H % r, W % r, W % 4
 * or et_bstride % 4 != 0: DDNM_E_SHAPE.  All of it is checked before any launch.
 * ------------------------------------------------------------------------- */
int ddnm_op_mcsr_A_f32(const float* x, const float* mask, float* y, int32_t B, int32_t H, int32_t W, int32_t r,
                       const float* w3_host, void* stream);
int ddnm_op_mcsr_pinv_f32(const float* y, const float* mask, float* x, int32_t B, int32_t H, int32_t W, int32_t r,
                          const float* w3_host, void* stream);
/* Fused noise-free step (functions/svd_ddnm.py:57-65):
 *   x0 = (xt - et * sqrt_1m_at) / sqrt_at;   x0h = x0 - lambda * A^+(A x0 - y);   xt' = sqrt_at_next * x0h + c1 * noise + c2 * et.
 * x0 (optional) receives the uncorrected x0, bit for bit that of ddnm_step_x0_f32; noise as in ddnm_step_mosaic_f32 /
 * _keyed_f32.  TWO passes over a strip (site sums, then the update; the second reads xt, et and the mask again and draws
 * the noise again from its offset): x0 and xt_next MUST NOT overlap xt or et.  That is the caller's obligation; only
 * identity is checked (an output whose address equals xt, et or the other output: DDNM_E_BADARG), partly overlapping
 * buffers are not detected. */
int ddnm_step_mcsr_f32(const float* xt, const float* et, int64_t et_bstride, const float* noise, const float* y,
                       const float* mask, float* x0, float* xt_next, int32_t B, int32_t H, int32_t W, int32_t r,
                       const float* w3_host, const ddnm_step_scalars* s, void* stream);
int ddnm_step_mcsr_keyed_f32(const float* xt, const float* et, int64_t et_bstride, const uint32_t* rng_keys, const float* y,
                             const float* mask, float* x0, float* xt_next, int32_t B, int32_t H, int32_t W, int32_t r,
                             const float* w3_host, const ddnm_step_scalars* s, void* stream);
/* The whole DDNM+ step (functions/svd_ddnm.py:80-164, step :118-131) in ONE launch, in the form of
 * ddnm_step_plus_spectral_f32 (eps enters as V^T eps, n ~ N(0, I) is drawn in image space).  With a = s->sqrt_at_next,
 * (lambda_j, d1_j, d2_j) the spectral coefficients of s_j -- evaluated per site in the kernel: one launch holds sites on
 * both sides of the threshold sigma_t <> a sigma_y / s_j and null-space sites -- and (1, d1n, d2n) those of 0,
 *   x0      = (xt - et * sqrt_1m_at) / sqrt_at                        -> x0_out, uncorrected (required)
 *   x_{t-1} = a x0 + d1n n + d2n et
 *             + q_j [ -a lambda_j (q_j . x0 - y_j / s_j) + (d1_j - d1n) (q_j . n) + (d2_j - d2n) (q_j . et) ]   where k_j > 0
 * Two passes like the noise-free step: x0_out and xt_next must not overlap xt or et (checked for identity only, as there);
 * the in-kernel and keyed noise sources are drawn once per pass, a noise tensor is read twice. */
int ddnm_step_plus_mcsr_f32(const float* xt, const float* et, int64_t et_bstride, const float* noise, const float* y,
                            const float* mask, float* x0_out, float* xt_next, int32_t B, int32_t H, int32_t W, int32_t r,
                            const float* w3_host, float sigma_y, float sigma_t, float eta, const ddnm_step_scalars* s,
                            void* stream);
int ddnm_step_plus_mcsr_keyed_f32(const float* xt, const float* et, int64_t et_bstride, const uint32_t* rng_keys,
                                  const float* y, const float* mask, float* x0_out, float* xt_next, int32_t B, int32_t H,
                                  int32_t W, int32_t r, const float* w3_host, float sigma_y, float sigma_t, float eta,
                                  const ddnm_step_scalars* s, void* stream);

/* ------------------------------------------------------------------------- *
 * Chroma-subsampled restoration (Y'CbCr 4:2:0, 4:2:2, 4:1:1): full-resolution luma, chroma averaged over sites of
 * rw columns x rh rows (n = rw rh), with the exact pseudo-inverse.  The reference has no such operator; the entry points
 * stand for A / A_pinv of its operator classes in the steps of functions/svd_ddnm.py:57-65 (DDNM) and :80-164 (DDNM+).
 * Added under ABI 7: new symbols only.
 *   M = m9_host: HOST pointer to a 3 x 3 colour matrix, row-major, rows w_Y, w_Cb, w_Cr, invertible (required); no offsets,
 *       the data are centred.  Full-range BT.601: (0.299, 0.587, 0.114), (-0.168736, -0.331264, 0.5), (0.5, -0.418688, -0.081312).
 *   Y[i][j]  = w_Y . x[:, i, j];   Cb[I][J] = (1/n) sum_{(i,j) in site(I,J)} w_Cb . x[:, i, j];   Cr likewise
 *   x [B][3][H][W];  y [B][H W + 2 H W / n]: the planes Y [H][W], Cb [H/rh][W/rw], Cr [H/rh][W/rw], row-major each;
 *   et row b at et + b*et_bstride (the [:, :3] view of a 6-channel output).
 * Per site, with mu(v) the mean colour: the n - 1 zero-mean patterns see only w^ = w_Y / |w_Y| (singular value |w_Y|, the
 * two colour directions orthogonal to w^ are null space), and the mean goes through D = diag(1, 1/sqrt n, 1/sqrt n) M =
 * U_D S_D V_D^T.  A launch has four singular values, the same at every site; A has full row rank.  With Ybar the site
 * mean of Y and w+ = w_Y / |w_Y|^2,
 *   (A^+ y)[:, p] = w+ (Y_p - Ybar) + M^-1 (Ybar, Cb, Cr)^T.
 * Sites (rw, rh): (2,1) 4:2:2, (4,1) 4:1:1, (2,2) 4:2:0, (4,4), (8,8).  One lane owns a strip of rh rows x 4 pixels x 3
 * planes; at rw = 8 two neighbouring lanes add their halves of a site (one shuffle, fixed order), so an image gives the
 * same bits alone and inside any batch.
 * NULL pointer (x0 of the noise-free step aside), B <= 0, no noise source, a misaligned key table, an output that is xt, et
 * or the other output, or a singular M (|det M| < 1e-6 |M|_F^3 in double): DDNM_E_BADARG; then a site not listed, H or
 * W <= 0, H % rh, W % rw, W % 4 or et_bstride % 4 != 0: DDNM_E_SHAPE.  All of it is checked before any launch.
 * ------------------------------------------------------------------------- */
/* What the launchers derive from M, in double, host only (no device call): out[37] =
 *   M^-1 [9], w+ [3], w^ [3], |w_Y| [1], U_D [9], S_D [3] (descending), V_D [9]
 * (3 x 3 row-major; the COLUMNS of U_D and V_D are the singular vectors; a Jacobi iteration on D^T D, no library; the
 * signs of a pair (u_k, v_k) are the iteration's).  A client supplies only M: the launchers call this themselves. */
int ddnm_chroma_constants(const float* m9_host, int32_t rw, int32_t rh, double* out);
int ddnm_op_chroma_A_f32(const float* x, float* y, int32_t B, int32_t H, int32_t W, int32_t rw, int32_t rh,
                         const float* m9_host, void* stream);
int ddnm_op_chroma_pinv_f32(const float* y, float* x, int32_t B, int32_t H, int32_t W, int32_t rw, int32_t rh,
                            const float* m9_host, void* stream);
/* Fused noise-free step (functions/svd_ddnm.py:57-65):
 *   x0 = (xt - et * sqrt_1m_at) / sqrt_at;   x0h = x0 - lambda * A^+(A x0 - y);   xt' = sqrt_at_next * x0h + c1 * noise + c2 * et.
 * x0 (optional) receives the uncorrected x0, bit for bit that of ddnm_step_x0_f32; noise as in ddnm_step_mcsr_f32 /
 * _keyed_f32.  TWO passes over a strip (site means of the residual, then the update; the second reads xt, et and Y again
 * and draws the noise again from its offset): x0 and xt_next MUST NOT overlap xt or et.  That is the caller's obligation;
 * only identity is checked (DDNM_E_BADARG), partly overlapping buffers are not detected. */
int ddnm_step_chroma_f32(const float* xt, const float* et, int64_t et_bstride, const float* noise, const float* y, float* x0,
                         float* xt_next, int32_t B, int32_t H, int32_t W, int32_t rw, int32_t rh, const float* m9_host,
                         const ddnm_step_scalars* s, void* stream);
int ddnm_step_chroma_keyed_f32(const float* xt, const float* et, int64_t et_bstride, const uint32_t* rng_keys, const float* y,
                               float* x0, float* xt_next, int32_t B, int32_t H, int32_t W, int32_t rw, int32_t rh,
                               const float* m9_host, const ddnm_step_scalars* s, void* stream);
/* The whole DDNM+ step (functions/svd_ddnm.py:80-164, step :118-131) in ONE launch, in the form of
 * ddnm_step_plus_spectral_f32 (eps enters as V^T eps, n ~ N(0, I) is drawn in image space).  With a = s->sqrt_at_next,
 * (lambda_a, d1_a, d2_a) the spectral coefficients of |w_Y|, (Lambda, D1, D2) those of S_D (diagonal), (1, d1n, d2n)
 * those of 0, t_p(g) = w^ . g_p with site mean tbar, z' = (Ybar, Cb / sqrt n, Cr / sqrt n):
 *   x0      = (xt - et * sqrt_1m_at) / sqrt_at                        -> x0_out, uncorrected (required)
 *   x_{t-1}[:, p] = a x0_p + d1n n_p + d2n et_p
 *      + w^  [ -a lambda_a ((t_p(x0) - tbar(x0)) - (Y_p - Ybar) / |w_Y|) + (d1_a - d1n)(t_p(n) - tbar(n)) + (d2_a - d2n)(t_p(et) - tbar(et)) ]
 *      + V_D [ -a Lambda (V_D^T mu(x0) - S_D^-1 U_D^T z') + (D1 - d1n) V_D^T mu(n) + (D2 - d2n) V_D^T mu(et) ]
 * The launcher evaluates the four coefficient triples once per launch, in double, and passes what is constant over a site
 * as four 3 x 3 matrices; the kernel evaluates no coefficient.  Two passes like the noise-free step: x0_out and xt_next
 * must not overlap xt or et (checked for identity only); the in-kernel and keyed noise sources are drawn once per pass, a
 * noise tensor is read twice. */
int ddnm_step_plus_chroma_f32(const float* xt, const float* et, int64_t et_bstride, const float* noise, const float* y,
                              float* x0_out, float* xt_next, int32_t B, int32_t H, int32_t W, int32_t rw, int32_t rh,
                              const float* m9_host, float sigma_y, float sigma_t, float eta, const ddnm_step_scalars* s,
                              void* stream);
int ddnm_step_plus_chroma_keyed_f32(const float* xt, const float* et, int64_t et_bstride, const uint32_t* rng_keys,
                                    const float* y, float* x0_out, float* xt_next, int32_t B, int32_t H, int32_t W, int32_t rw,
                                    int32_t rh, const float* m9_host, float sigma_y, float sigma_t, float eta,
                                    const ddnm_step_scalars* s, void* stream);

/* ------------------------------------------------------------------------- *
 * JPEG-artifact restoration: the measurement is the quantisation CELL of every 8 x 8 block-DCT coefficient of the
 * chroma-subsampled planes, and the range-space correction pulls T x0 back into the cell instead of onto one value.  The
 * reference has no such operator; the entry points stand for A / A_pinv of its operator classes in the step of
 * functions/svd_ddnm.py:57-65.  Added under ABI 7: new symbols only (csrc/jpeg.hip).
 *   x [B][3][H][W], RGB, scale [-1, 1].  Site (rw, rh): (1,1) 4:4:4, (2,1) 4:2:2, (2,2) 4:2:0; H % (8 rh) == W % (8 rw) == 0.
 *   M = m9_host: HOST pointer to the 3 x 3 colour matrix of the chroma section above (rows w_Y, w_Cb, w_Cr, invertible).
 *   T (linear): the planes Y | Cb | Cr of ddnm_op_chroma_A_f32 (luma at every pixel, chroma averaged per site), then per
 *       plane and per 8 x 8 block the orthonormal 2-D DCT-II  C X C^T,  C[k][n] = s_k cos((2n + 1) k pi / 16),
 *       s_0 = sqrt(1/8), s_k = sqrt(2/8).  In place: coefficient (u, v) of block (I, J) sits at plane position
 *       (8 I + u, 8 J + v); planes row-major in the row order [ Y | Cb | Cr ]: H W (1 + 2 / (rw rh)) entries per row, a
 *       multiple of 4.  T has full row rank; T^+ = A_chroma^+ . IDCT is its exact Moore-Penrose inverse (an orthogonal
 *       factor on the left does not change a pseudo-inverse).
 *   q = q128_host: HOST pointer to 128 quantisation steps in x units (the 8-bit table entry / 127.5), luma [64] then
 *       chroma [64], natural (row-major u, v) order, finite and > 0.
 *   delta: the level shift.  An encoder subtracts 128 from 8-bit samples; on this scale that is the offset -4 / 127.5 on
 *       the luma DC coefficient only, every other coefficient has offset 0.
 *   A (the encoder):  y = q rint((T x - delta) / q) + delta, the dequantised cell centre (rint: ties to even).
 *       A^+ y := T^+ y is what a decoder shows before clipping to 8 bit.
 * One workgroup of 256 threads owns 16 / rw consecutive MCUs (8 rw x 8 rh pixels; MCUs numbered row-major over the batch);
 * every MCU is transformed inside its workgroup, the 8-point transforms in registers and the two transposes of a block
 * through LDS.  An image gives the same bits alone and inside any batch.
 * NULL pointer (x0 of the step aside), B <= 0, no noise source, a misaligned key table, an output that is xt, et or the
 * other output, a singular M, a step q that is not finite or <= 0, box outside [0, 1]: DDNM_E_BADARG; then a site not
 * listed, H or W <= 0, H % (8 rh), W % (8 rw) or et_bstride % 4 != 0: DDNM_E_SHAPE.  All of it is checked before any launch.
 * ------------------------------------------------------------------------- */
/* libjpeg's tables for quality 1..100, host only (no device call): scale = 5000 / quality (integer) below 50, else
 * 200 - 2 quality; entry = clamp((base * scale + 50) / 100, 1, 255) with base the tables K.1 / K.2 of ITU-T T.81 Annex K;
 * q128_out[i] = entry / 127.5 (luma, then chroma, natural order); *delta_out = dc_shift ? -4 / 127.5 : 0.
 * NULL pointer or quality outside 1..100: DDNM_E_BADARG. */
int ddnm_jpeg_quality_tables(int32_t quality, int32_t dc_shift, float* q128_out, float* delta_out);
/* c = T x;  y = A x (the encoder);  x = T^+ y */
int ddnm_op_jpeg_T_f32(const float* x, float* c, int32_t B, int32_t H, int32_t W, int32_t rw, int32_t rh,
                       const float* m9_host, void* stream);
int ddnm_op_jpeg_A_f32(const float* x, float* y, int32_t B, int32_t H, int32_t W, int32_t rw, int32_t rh,
                       const float* m9_host, const float* q128_host, float delta, void* stream);
int ddnm_op_jpeg_pinv_f32(const float* y, float* x, int32_t B, int32_t H, int32_t W, int32_t rw, int32_t rh,
                          const float* m9_host, void* stream);
/* Fused step in ONE launch and one pass, with h = box q / 2, 0 <= box <= 1:
 *   x0 = (xt - et * sqrt_1m_at) / sqrt_at;   c = T x0;   x0h = x0 - lambda * T^+(c - clamp(c, y - h, y + h));
 *   xt' = sqrt_at_next * x0h + c1 * noise + c2 * et.
 * box = 0 is x0 - lambda T^+(T x0 - y); with box just below 1 (0.98: clamped coefficients land on the cell edge, and the
 * margin keeps fp32 rounding from deciding how they re-quantise) A xt' at the last step returns the measured levels.
 * x0 (optional) receives the uncorrected x0, bit for bit that of ddnm_step_x0_f32; noise as in ddnm_step_chroma_f32 /
 * _keyed_f32, indexed by the pixel's linear position in the tensor.  xt, et, noise and y are read once, x0 and xt_next
 * written once; no global scratch.  x0 and xt_next must not be xt or et (checked for identity). */
int ddnm_step_jpeg_f32(const float* xt, const float* et, int64_t et_bstride, const float* noise, const float* y, float* x0,
                       float* xt_next, int32_t B, int32_t H, int32_t W, int32_t rw, int32_t rh, const float* m9_host,
                       const float* q128_host, float box, const ddnm_step_scalars* s, void* stream);
int ddnm_step_jpeg_keyed_f32(const float* xt, const float* et, int64_t et_bstride, const uint32_t* rng_keys, const float* y,
                             float* x0, float* xt_next, int32_t B, int32_t H, int32_t W, int32_t rw, int32_t rh,
                             const float* m9_host, const float* q128_host, float box, const ddnm_step_scalars* s,
                             void* stream);

/* ------------------------------------------------------------------------- *
 * hq_demo sampler: DDPM posterior step with the DDNM core and the mask-shift tiles
 * (hq_demo/guided_diffusion/gaussian_diffusion.py:246-404,430-487,664-746).
 * ------------------------------------------------------------------------- */
/* x0 = clamp?(c_recip*x_t - c_recipm1*eps, -1, 1); eps row b at eps + b*eps_bstride (first 3 of the 6 output channels) */
int ddnm_hq_x0_f32(const float* xt, const float* eps, int64_t eps_bstride, float* x0, int32_t B, int64_t chw,
                   float c_recip, float c_recipm1, int32_t clip, void* stream);
/* x0_hat = lambda*A^+y + x0 - lambda*A^+A x0 (Eq. 17, :339) */
int ddnm_hq_project_f32(const float* x0, const float* apy, const float* apax0, float* x0_hat, int64_t n, float lam,
                        void* stream);
/* dst[p][dy+i][dx+j] = src[p][sy+i][sx+j], i < h, j < w, for `planes` planes of [Hs][Ws] / [Hd][Wd] */
int ddnm_copy_rect_f32(const float* src, int32_t Hs, int32_t Ws, int32_t sy, int32_t sx, float* dst, int32_t Hd, int32_t Wd,
                       int32_t dy, int32_t dx, int32_t planes, int32_t h, int32_t w, void* stream);
/* out = (coef1*x0_hat + coef2*x_t [+ gamma*grad]) + noise_scale*noise; grad may be NULL */
int ddnm_hq_sample_f32(const float* x0_hat, const float* xt, const float* grad, const float* noise, float* out, int64_t n,
                       float coef1, float coef2, float gamma, float noise_scale, void* stream);

/* inverse_data_transform + per-image MSE (datasets/__init__.py:218-227; diffusion.py:599-602):
 * img = clamp((x+1)/2, 0, 1); mse[b] = mean((img - clamp((x_orig+1)/2,0,1))^2) */
int ddnm_finalize_psnr_f32(const float* x, const float* x_orig, float* img /* may be NULL */, double* sse /* [B], zeroed by callee */,
                           int32_t B, int64_t chw, void* stream);

/* SSIM (Wang et al. 2004) of x against y, one double per image: 11x11 Gaussian window (sigma 1.5, weights normalised in
 * fp64), valid positions only, C1 = 0.01^2, C2 = 0.03^2, ssim[b] = mean of the map over the C*(H-10)*(W-10) positions
 * of image b.  x, y: NCHW fp32; transform != 0 passes both through clamp((v+1)/2, 0, 1) on load (the sampler's [-1, 1]
 * tensors, as ddnm_finalize_psnr_f32 takes them), transform == 0 takes [0, 1] images.  Moments are accumulated in fp64
 * and the per-tile partials are added in a fixed order without atomics: an image's value is bit for bit the same alone
 * and at any position of any batch.  work: ddnm_ssim_workspace_elems(B, C, H, W) doubles
 * (= B * C * ceil((W-10)/32) * ceil((H-10)/16), one per 32x16 tile of valid positions), not read after the call.
 * NULL x / y / ssim / work or B, C <= 0: DDNM_E_BADARG; H < 11, W < 11, more than 2^31-1 tiles or work_elems below
 * the query: DDNM_E_SHAPE (the query returns the same negative codes). */
int64_t ddnm_ssim_workspace_elems(int32_t B, int32_t C, int32_t H, int32_t W);
int ddnm_ssim_f32(const float* x, const float* y, double* ssim /* [B] */, double* work, int64_t work_elems, int32_t B,
                  int32_t C, int32_t H, int32_t W, int32_t transform, void* stream);

/* Per-pixel mean and standard deviation over the K restorations (samples) of each of B images, with their per-image
 * summaries.  Sample k of image b starts at x + b*image_stride + k*sample_stride (strides in floats): [K][B][chw] as a
 * sampler call leaves it is (chw, B*chw), [B][K][chw] after a gather is (K*chw, chw).  Per element:
 *   v_k = clamp((x_k+1)/2, 0, 1) in fp32 (what ddnm_finalize_psnr_f32 forms), m = sum_k v_k / K,
 *   s = sqrt(sum_k (v_k - m)^2 / (K - 1)), s = 0 for K = 1,
 * both moments in fp64 from deviations (two passes over the samples); only mean_img = (float)m and std_img = (float)s are
 * rounded.  Per image: sse_mean[b] = sum_e (double)(d*d) with d = mean_img - clamp((x_orig+1)/2, 0, 1) in fp32 (K = 1
 * gives ddnm_finalize_psnr_f32's img and sse); std_mean[b] = (sum_e s) / chw with the fp64 s.  The per-workgroup
 * partials go to `work` and are added in an order that depends on chw alone, without atomics: an image's four outputs are
 * bit for bit the same alone and at any position of any batch.  16-byte loads and stores when chw, both strides and
 * the pointers allow, element-wise otherwise (same bits).  work: ddnm_sample_stats_workspace_elems(B, chw) doubles
 * (= 2 * B * ceil(chw / 2048)), not read after the call.
 * NULL x / mean_img / std_img / std_mean / work, B, K or chw < 1, a negative stride, or x_orig and sse_mean not both
 * given or both NULL: DDNM_E_BADARG; more than 2^31-1 workgroups or work_elems below the query: DDNM_E_SHAPE (the query
 * returns the same negative codes). */
int64_t ddnm_sample_stats_workspace_elems(int32_t B, int64_t chw);
int ddnm_sample_stats_f32(const float* x, int64_t image_stride, int64_t sample_stride, const float* x_orig /* [B][chw] or NULL */,
                          float* mean_img /* [B][chw] */, float* std_img /* [B][chw] */,
                          double* sse_mean /* [B], NULL iff x_orig NULL */, double* std_mean /* [B] */, double* work,
                          int64_t work_elems, int32_t B, int32_t K, int64_t chw, void* stream);

/* Data consistency: per-row norms of the residual d = A x^ - y of B measurement rows of up to m entries.  Row b of both
 * operands starts at b*row_stride floats (row_stride >= m) and has n_b = counts ? counts[b] : m valid entries,
 * 0 <= n_b <= m; entries at or beyond n_b are not read (a mask bank pads its rows).  Per valid entry
 * d = (double)ax - (double)y, which is exact; l1[b] = sum |d| and sse[b] = sum d^2 in fp64, maxabs[b] = (float)max |d|;
 * n_b = 0 gives three zeros.  A row takes ceil(m / 2048) workgroups whatever n_b is, and their partials go to `work` and
 * are added in an order that depends on m alone, without atomics: a row's three outputs are bit for bit the same alone
 * and at any row of any batch.  16-byte loads where the pointers, row_stride and the position in the row allow,
 * element-wise otherwise (same entries on the same thread in the same order: same bits).
 * counts: int32 [B] the device can read.  Device memory is clamped to [0, m] by the kernel; pinned or managed memory,
 * which the host can read too, is checked before the launch; pageable host memory is refused (DDNM_E_BADARG).
 * work: ddnm_consistency_workspace_elems(B, m) doubles (= 3 * B * ceil(m / 2048)), not read after the call.
 * NULL ax / y / l1 / sse / maxabs / work, B < 1, m < 1 or row_stride < m: DDNM_E_BADARG; work_elems below the query, a
 * count outside [0, m] that the host can see, or more than 2^31-1 workgroups: DDNM_E_SHAPE (the query returns the same
 * negative codes). */
int64_t ddnm_consistency_workspace_elems(int32_t B, int64_t m);
int ddnm_consistency_f32(const float* ax, const float* y, int64_t row_stride, const int32_t* counts /* [B] or NULL */,
                         double* l1 /* [B] */, double* sse /* [B] */, float* maxabs /* [B] */, double* work,
                         int64_t work_elems, int32_t B, int64_t m, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DDNM_HIP_H */
