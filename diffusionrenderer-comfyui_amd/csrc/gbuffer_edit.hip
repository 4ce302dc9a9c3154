// Relight edits on the device G-buffers (drn_gbuffer_edit_u8, include/drn.h; the rule and the torch specification:
// gbuffer_edit.py, edit_gbuffers).  Between the inverse and the forward stage of Cosmos1Relight the 1..5 uint8
// maps [B, T, pixels, 3] of a call are edited in ONE launch: per map and channel an affine under the edit mask (material
// edits), then an inserted object's layer under its matte (object insertion), and on the normal map the inserted pixels
// renormalised.  The maps, their strides, gains and offsets travel BY VALUE in the kernel's argument struct, as the ensemble's
// member pointers do: no device table, no temporaries.
//
// Streaming: a lane reads its pixels' two mask bytes ONCE and walks the maps with them (2 mask bytes per pixel, not 10).  Where
// every base and every non-zero stride is on the 16-byte grid a lane owns 16 whole pixels: 16 bytes of each mask and 48 bytes
// of each map and layer in 16-byte words (a lane's piece never cuts a pixel); what pixels % 16 leaves of a frame, and every
// pixel otherwise, goes one pixel per lane through the same arithmetic.  (frame, piece) is one flat 64-bit index under a capped
// grid with a grid stride; every tensor has a batch and a frame stride in bytes, 0 = broadcast.  In place (dst == src), a lane
// whose pixels all have both masks 0 stores nothing.
//
// The arithmetic is fp32 with every operation rounded on its own: plain operators under `fp contract(off)`, as in ensemble.hip
// and tile_blend.hip.  ge_affine and ge_normal restate en_affine and en_normal (N = 1, no spread) of ensemble.hip, ge_blend
// tile_blend.hip's tb_blend; ensemble.hip itself is left as it is.  The affine must stay two rounded operations (a fused one
// differs, e.g. at g = 0.3, o = 7.3); the blends are exact under fusion too, so nothing here depends on how they are paired.
// A mask byte m weighs unit(m) = fp32(m) / 255 correctly rounded, from an LDS table (fit.u8_unit's bits); the same table decodes
// a normal's byte as unit * 2 - 1.
#include "drn_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int GE_THREADS = 256;
constexpr int GE_MAX_BLOCKS = 2048;           // ew_grid's cap: one sweep of the 2048 * 256 lanes is 8 Mi pixels (one per lane: 512 Ki)
constexpr int GE_MAX_MAPS = 5;

struct GeParams {
    drn_gbuffer_edit_map map[GE_MAX_MAPS];
    int affine[GE_MAX_MAPS];                  // the map's (gain, offset) is not the identity
    const uint8_t *em, *im;                   // NULL: 255 everywhere / no insertion
    int64_t em_bs, em_ts, im_bs, im_ts;
    int64_t T, pixels, frames;
};

__device__ __forceinline__ uint32_t ge_affine(uint32_t x, float g, float o) {
    const float m = g * (float)x;
    const float a = m + o;
    return (uint32_t)__builtin_rintf(__builtin_amdgcn_fmed3f(a, 0.0f, 255.0f));
}

// a + w (b - a), w in [0, 1]: inside [a, b], so no clamp; w = 1 gives b and w = 0 gives a exactly
__device__ __forceinline__ uint32_t ge_blend(uint32_t a, uint32_t b, float w) {
    const float fa = (float)a;
    const float d = (float)b - fa;
    const float m = w * d;
    return (uint32_t)__builtin_rintf(fa + m);
}

// one pixel decoded, renormalised and encoded again: ensemble.reduce_members([z], "normal")
__device__ __forceinline__ void ge_normal(uint32_t& z0, uint32_t& z1, uint32_t& z2, const float* unit_s) {
    float s[3];
    const uint32_t z[3] = {z0, z1, z2};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float u2 = unit_s[z[c]] * 2.0f;
        s[c] = u2 - 1.0f;
    }
    const float xx = s[0] * s[0], yy = s[1] * s[1], zz = s[2] * s[2];
    const float xy = xx + yy;
    const float l2 = xy + zz;
    const float l = sqrtf(l2);
    const float d = fmaxf(l, 1e-6f);
    uint32_t o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float nc = s[c] / d;
        const float a = nc + 1.0f;
        const float m = a * 127.5f;
        o[c] = (uint32_t)__builtin_rintf(__builtin_amdgcn_fmed3f(m, 0.0f, 255.0f));
    }
    z0 = o[0], z1 = o[1], z2 = o[2];
}

// NPX whole pixels of one map: v[] = the map's bytes (in: the source, out: the result), L[] = the layer's
template <int NPX>
__device__ __forceinline__ void ge_apply(const drn_gbuffer_edit_map& mp, int affine, uint32_t (&v)[NPX * 3], const uint32_t (&L)[NPX * 3],
                                         const float (&we)[NPX], const float (&wi)[NPX], const uint32_t (&mi)[NPX], const float* unit_s) {
    if (affine) {
#pragma unroll
        for (int i = 0; i < NPX * 3; ++i) v[i] = ge_blend(v[i], ge_affine(v[i], mp.gain[i % 3], mp.offset[i % 3]), we[i / 3]);
    }
    if (mp.layer) {
#pragma unroll
        for (int i = 0; i < NPX * 3; ++i) v[i] = ge_blend(v[i], L[i], wi[i / 3]);
        if (mp.is_normal) {
#pragma unroll
            for (int p = 0; p < NPX; ++p)
                if (mi[p]) ge_normal(v[3 * p], v[3 * p + 1], v[3 * p + 2], unit_s);
        }
    }
}

__device__ __forceinline__ uint32_t ge_byte(const uint4& q, int i) {
    const uint32_t w = (i >> 2) == 0 ? q.x : (i >> 2) == 1 ? q.y : (i >> 2) == 2 ? q.z : q.w;
    return (w >> (8 * (i & 3))) & 255u;
}

// vec: every base and every non-zero stride is 16-byte aligned (the host's finding; uniform)
template <int NM>
__global__ void __launch_bounds__(GE_THREADS) gbuffer_edit_kernel(GeParams P, int vec) {
    __shared__ float unit_s[256];
    unit_s[threadIdx.x] = __fdiv_rn((float)threadIdx.x, 255.0f);
    __syncthreads();
    const int64_t lane = (int64_t)blockIdx.x * GE_THREADS + threadIdx.x;
    const int64_t lanes = (int64_t)gridDim.x * GE_THREADS;
    const int64_t ppf = vec ? P.pixels >> 4 : 0;                  // pieces of 16 whole pixels per frame
    for (int64_t w = lane; w < P.frames * ppf; w += lanes) {
        const int64_t f = w / ppf, g = w - f * ppf;
        const int64_t b = f / P.T, t = f - b * P.T;
        uint4 qe = make_uint4(~0u, ~0u, ~0u, ~0u), qi = make_uint4(0u, 0u, 0u, 0u);
        if (P.em) qe = *reinterpret_cast<const uint4*>(P.em + b * P.em_bs + t * P.em_ts + (g << 4));
        if (P.im) qi = *reinterpret_cast<const uint4*>(P.im + b * P.im_bs + t * P.im_ts + (g << 4));
        const bool untouched = ((qe.x | qe.y | qe.z | qe.w) | (qi.x | qi.y | qi.z | qi.w)) == 0;
        float we[16], wi[16];
        uint32_t mi[16];
#pragma unroll
        for (int p = 0; p < 16; ++p) {
            we[p] = unit_s[ge_byte(qe, p)];
            mi[p] = ge_byte(qi, p);
            wi[p] = unit_s[mi[p]];
        }
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            const drn_gbuffer_edit_map& mp = P.map[m];
            const uint8_t* src = (const uint8_t*)mp.src + b * mp.src_bs + t * mp.src_ts + g * 48;
            uint8_t* dst = (uint8_t*)mp.dst + b * mp.dst_bs + t * mp.dst_ts + g * 48;
            if (untouched && dst == src) continue;               // in place and both masks 0 on all 16 pixels: nothing to store
            uint4 qs[3], ql[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) qs[j] = ld16_nt(src + 16 * j);
            if (mp.layer) {
                const uint8_t* lay = (const uint8_t*)mp.layer + b * mp.layer_bs + t * mp.layer_ts + g * 48;
#pragma unroll
                for (int j = 0; j < 3; ++j) ql[j] = *reinterpret_cast<const uint4*>(lay + 16 * j);
            }
            uint32_t v[48], L[48];
#pragma unroll
            for (int i = 0; i < 48; ++i) {
                v[i] = ge_byte(qs[i >> 4], i & 15);
                L[i] = mp.layer ? ge_byte(ql[i >> 4], i & 15) : 0u;
            }
            ge_apply<16>(mp, P.affine[m], v, L, we, wi, mi, unit_s);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                uint32_t ow[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int k = 16 * j + 4 * i;
                    ow[i] = v[k] | (v[k + 1] << 8) | (v[k + 2] << 16) | (v[k + 3] << 24);
                }
                *reinterpret_cast<uint4*>(dst + 16 * j) = make_uint4(ow[0], ow[1], ow[2], ow[3]);
            }
            __builtin_amdgcn_sched_barrier(0);                   // map after map: the next map's loads do not pile up on this one's bytes
        }
    }
    // one pixel per lane: every pixel of a ragged call, or what pixels % 16 leaves of each frame
    const int64_t px0 = ppf << 4, npx = P.pixels - px0;
    for (int64_t w = lane; w < P.frames * npx; w += lanes) {
        const int64_t f = w / npx, px = px0 + (w - f * npx);
        const int64_t b = f / P.T, t = f - b * P.T;
        const uint32_t me = P.em ? P.em[b * P.em_bs + t * P.em_ts + px] : 255u;
        const uint32_t mi1 = P.im ? P.im[b * P.im_bs + t * P.im_ts + px] : 0u;
        const float we[1] = {unit_s[me]}, wi[1] = {unit_s[mi1]};
        const uint32_t mi[1] = {mi1};
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            const drn_gbuffer_edit_map& mp = P.map[m];
            const uint8_t* src = (const uint8_t*)mp.src + b * mp.src_bs + t * mp.src_ts + px * 3;
            uint8_t* dst = (uint8_t*)mp.dst + b * mp.dst_bs + t * mp.dst_ts + px * 3;
            if ((me | mi1) == 0 && dst == src) continue;
            uint32_t v[3], L[3] = {0u, 0u, 0u};
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = src[c];
            if (mp.layer) {
                const uint8_t* lay = (const uint8_t*)mp.layer + b * mp.layer_bs + t * mp.layer_ts + px * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) L[c] = lay[c];
            }
            ge_apply<1>(mp, P.affine[m], v, L, we, wi, mi, unit_s);
#pragma unroll
            for (int c = 0; c < 3; ++c) dst[c] = (uint8_t)v[c];
        }
    }
}

// the bytes a tensor of B x T frames spans under its strides: false where a stride is negative or the span leaves 2^62
bool ge_span(int64_t bs, int64_t ts, int B, int T, int64_t frame_bytes, int64_t* span) {
    const int64_t lim = (int64_t)1 << 60;
    if (bs < 0 || ts < 0 || frame_bytes > lim) return false;
    if (bs > lim / B || ts > lim / T) return false;
    *span = (int64_t)(B - 1) * bs + (int64_t)(T - 1) * ts + frame_bytes;
    return true;
}

bool ge_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

}  // namespace

extern "C" int drn_gbuffer_edit_map_bytes(void) { return (int)sizeof(drn_gbuffer_edit_map); }

extern "C" int drn_gbuffer_edit_u8(const drn_gbuffer_edit_map* maps, int n_maps, const void* edit_mask, int64_t edit_mask_bs,
                                   int64_t edit_mask_ts, const void* insert_mask, int64_t insert_mask_bs, int64_t insert_mask_ts,
                                   int B, int T, int64_t pixels, void* stream) {
    DRN_CHECK_ARG(maps);
    DRN_CHECK_ARG(n_maps >= 1 && n_maps <= GE_MAX_MAPS);
    DRN_CHECK_ARG(B >= 1 && T >= 1 && pixels >= 0);
    const int64_t frames = (int64_t)B * T;
    DRN_CHECK_ARG(pixels <= ((int64_t)1 << 58) / frames);       // frames * pixels * 3 stays far inside 64 bits
    GeParams P = {};
    uintptr_t grid16 = 0;
    bool any_layer = false;
    int64_t span_s[GE_MAX_MAPS], span_d[GE_MAX_MAPS], span_l[GE_MAX_MAPS], span_e = 0, span_i = 0;
    for (int m = 0; m < n_maps; ++m) {
        const drn_gbuffer_edit_map& mp = maps[m];
        DRN_CHECK_ARG(mp.src && mp.dst);
        DRN_CHECK_ARG(!mp.layer || insert_mask);
        bool identity = true;
        for (int c = 0; c < 3; ++c) {
            DRN_CHECK_ARG(__builtin_isfinite(mp.gain[c]) && __builtin_isfinite(mp.offset[c]));
            identity = identity && mp.gain[c] == 1.0f && mp.offset[c] == 0.0f;
        }
        DRN_CHECK_ARG(ge_span(mp.src_bs, mp.src_ts, B, T, pixels * 3, &span_s[m]));
        DRN_CHECK_ARG(ge_span(mp.dst_bs, mp.dst_ts, B, T, pixels * 3, &span_d[m]));
        // dst's frames and clips lie apart: nothing is written twice
        DRN_CHECK_ARG(T == 1 || mp.dst_ts >= pixels * 3);
        DRN_CHECK_ARG(B == 1 || mp.dst_bs >= (int64_t)(T - 1) * mp.dst_ts + pixels * 3);
        span_l[m] = 0;
        if (mp.layer) DRN_CHECK_ARG(ge_span(mp.layer_bs, mp.layer_ts, B, T, pixels * 3, &span_l[m]));
        P.map[m] = mp;
        P.affine[m] = !identity;
        any_layer = any_layer || mp.layer;
        grid16 |= (uintptr_t)mp.src | (uintptr_t)mp.dst | (uintptr_t)mp.src_bs | (uintptr_t)mp.src_ts | (uintptr_t)mp.dst_bs | (uintptr_t)mp.dst_ts;
        if (mp.layer) grid16 |= (uintptr_t)mp.layer | (uintptr_t)mp.layer_bs | (uintptr_t)mp.layer_ts;
    }
    if (edit_mask) {
        DRN_CHECK_ARG(ge_span(edit_mask_bs, edit_mask_ts, B, T, pixels, &span_e));
        grid16 |= (uintptr_t)edit_mask | (uintptr_t)edit_mask_bs | (uintptr_t)edit_mask_ts;
    }
    if (!any_layer) insert_mask = nullptr;                       // a matte without a layer inserts nothing: not read
    if (insert_mask) {
        DRN_CHECK_ARG(ge_span(insert_mask_bs, insert_mask_ts, B, T, pixels, &span_i));
        grid16 |= (uintptr_t)insert_mask | (uintptr_t)insert_mask_bs | (uintptr_t)insert_mask_ts;
    }
    if (pixels == 0) return DRN_OK;
    // dst overlaps nothing but its own src, and that only as the same tensor (in place)
    for (int m = 0; m < n_maps; ++m) {
        const drn_gbuffer_edit_map& mp = maps[m];
        DRN_CHECK_ARG(!(edit_mask && ge_overlap(mp.dst, span_d[m], edit_mask, span_e)));
        DRN_CHECK_ARG(!(insert_mask && ge_overlap(mp.dst, span_d[m], insert_mask, span_i)));
        for (int k = 0; k < n_maps; ++k) {
            DRN_CHECK_ARG(!(maps[k].layer && ge_overlap(mp.dst, span_d[m], maps[k].layer, span_l[k])));
            if (k != m) DRN_CHECK_ARG(!ge_overlap(mp.dst, span_d[m], maps[k].dst, span_d[k]) && !ge_overlap(mp.dst, span_d[m], maps[k].src, span_s[k]));
        }
        const bool in_place = mp.dst == mp.src && mp.dst_bs == mp.src_bs && mp.dst_ts == mp.src_ts;
        DRN_CHECK_ARG(in_place || !ge_overlap(mp.dst, span_d[m], mp.src, span_s[m]));
    }
    P.em = (const uint8_t*)edit_mask, P.em_bs = edit_mask_bs, P.em_ts = edit_mask_ts;
    P.im = (const uint8_t*)insert_mask, P.im_bs = insert_mask_bs, P.im_ts = insert_mask_ts;
    P.T = T, P.pixels = pixels, P.frames = frames;
    const int vec = (grid16 & 15) == 0;
    // lanes wanted: the wide path's pieces (and, far fewer, the frames' left-over pixels), or every pixel
    const int64_t pieces = vec ? frames * (pixels >> 4) : 0, rest = frames * (vec ? pixels & 15 : pixels);
    const int64_t work = pieces > rest ? pieces : rest;
    int64_t blocks = (work + GE_THREADS - 1) / GE_THREADS;
    if (blocks > GE_MAX_BLOCKS) blocks = GE_MAX_BLOCKS;
    const dim3 grid((unsigned)blocks), block(GE_THREADS);
    hipStream_t st = (hipStream_t)stream;
    switch (n_maps) {
        case 1: gbuffer_edit_kernel<1><<<grid, block, 0, st>>>(P, vec); break;
        case 2: gbuffer_edit_kernel<2><<<grid, block, 0, st>>>(P, vec); break;
        case 3: gbuffer_edit_kernel<3><<<grid, block, 0, st>>>(P, vec); break;
        case 4: gbuffer_edit_kernel<4><<<grid, block, 0, st>>>(P, vec); break;
        case 5: gbuffer_edit_kernel<5><<<grid, block, 0, st>>>(P, vec); break;
    }
    return drn_launch_status();
}
