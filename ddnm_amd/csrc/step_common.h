// What the sampler-step translation units (ddnm_step.hip, jpeg.hip) share: 16-byte moves, the noise sources and the two
// halves of the DDIM update.  Include it AFTER `#pragma clang fp contract(off)`: x0_of / update_of round mul and add
// separately, like the ATen elementwise kernels, in every unit alike.
#pragma once
#include "common.h"
#include "philox.h"

#define GRID_1D(n) dim3((unsigned)(((n) + 255) / 256 < 8192 ? ((n) + 255) / 256 : 8192))

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// Source of the step's N(0, I) noise: a tensor (explicit tape / ATen draw: the parity path) or, when `p` is NULL, the
// in-kernel Philox draw of ddnm_step_scalars::rng_* (philox.h) -- element offset `off` (multiple of 4) into [B][chw].
struct NoiseSrc {
    const float* p;
    PhiloxKey key;
    unsigned iter, img_base;
    int64_t chw;
};
static inline NoiseSrc noise_src(const float* noise, const ddnm_step_scalars* s, int64_t chw) {
    return NoiseSrc{noise, PhiloxKey{s->rng_seed_lo, s->rng_seed_hi}, s->rng_iter, s->rng_image_base, chw};
}
static inline bool noise_ok(const float* noise, const ddnm_step_scalars* s) { return noise != nullptr || s->rng_on != 0; }
__device__ __forceinline__ f32x4 nz4(const NoiseSrc& n, int64_t off) {
    if (n.p) return ld4(n.p + off);
    const int64_t b = off / n.chw, r = off - b * n.chw;
    return philox_normal4(n.key, (unsigned)(r >> 2), n.iter, n.img_base + (unsigned)b);
}

// Per-image keys (the *_keyed_f32 entry points): row b of `keys` = {key_lo, key_hi, image counter, 0}, so that images of
// different loader batches (different seeds) share a launch.  Rows {seed_lo, seed_hi, img_base + b, 0} give NoiseSrc's
// draw.  The kernels below are templates on the source; the NoiseSrc instantiations are the unkeyed entry points.
struct KeyedNoiseSrc {
    const uint4* keys;
    unsigned iter;
    int64_t chw;
};
static inline KeyedNoiseSrc keyed_src(const uint32_t* keys, const ddnm_step_scalars* s, int64_t chw) {
    return KeyedNoiseSrc{reinterpret_cast<const uint4*>(keys), s->rng_iter, chw};
}
static inline bool keys_ok(const uint32_t* keys) { return keys != nullptr && (reinterpret_cast<uintptr_t>(keys) & 15) == 0; }
// `bind(src, b)` at the top of a kernel's loop body: the keyed source loads image b's key row there, ahead of the
// operand loads (its latency hides behind theirs), and draws by offset within the image; NoiseSrc is returned as is.
struct KeyedRow {
    uint4 k;
    unsigned iter;
    int64_t base;    // b * chw
};
__device__ __forceinline__ const NoiseSrc& bind(const NoiseSrc& n, int64_t) { return n; }
__device__ __forceinline__ KeyedRow bind(const KeyedNoiseSrc& n, int64_t b) { return KeyedRow{n.keys[b], n.iter, b * n.chw}; }
__device__ __forceinline__ f32x4 nz4(const KeyedRow& n, int64_t off) {
    return philox_normal4(PhiloxKey{n.k.x, n.k.y}, (unsigned)((off - n.base) >> 2), n.iter, n.k.z);
}

__device__ __forceinline__ f32x4 x0_of(f32x4 xt, f32x4 et, const ddnm_step_scalars& s) {
    return (xt - et * s.sqrt_1m_at) / s.sqrt_at;
}
__device__ __forceinline__ f32x4 update_of(f32x4 x0h, f32x4 nz, f32x4 et, const ddnm_step_scalars& s) {
    return (x0h * s.sqrt_at_next + nz * s.c1) + et * s.c2;
}
