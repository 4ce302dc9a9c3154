// Spatial tiles joined in latent space (drn_latent_tile_gather, drn_latent_tile_step_join, include/drn.h; the plan and the torch
// specification: tiles.py, latent_tile / latent_gather / latent_step_join).  One noisy latent canvas,
// bf16 [planes,Hc,Wc] (a plane = one pass, channel and latent frame), exists for the whole picture.  Per Euler step and tile:
//   A (gather):     the tile's crop of the canvas, scaled by c_in, written as the DiT's contiguous input [copies,planes,h,w]
//                   (copies = 2 under CFG: the cond and uncond halves are the same values);
//   B (step + join): CFG combine and Euler step of the tile's DiT output against the CURRENT canvas, cross-faded into the NEXT
//                   canvas over what the tiles above and to the left already wrote there - tile_blend.hip's rule on bf16.
// Both replace a chain of torch device ops (slice + contiguous + edm_scale_input + cat; cfg_combine + edm_step on contiguous crops
// + the blend on slices) with one launch and no temporaries.  They move tens of megabytes per step beside a DiT forward of
// seconds and are not tuned further.
//
// A workgroup owns LT_W elements x LT_H rows of one plane's destination rectangle; B puts the weights of its rows and columns
// into LDS once (1.0f behind a ramp, so "no ramp" and "behind the ramp" are one case).  A lane owns one ALIGNED 4-byte word of a
// destination row segment, tile_blend.hip's scheme at two bytes per element: the segment starts at element misalignment
// m = (address >> 1) & 1, so word j holds segment elements [2j - m, 2j - m + 2).  Every source has its own alignment (x_at, rx,
// Wc and w may be odd, the base pointers lie anywhere on the 2-byte grid): its two elements are fetched as the aligned word
// around them, or as the two aligned words around them and shifted (each of the two holds one element of the segment, so neither
// leaves the page its tensor is in).  Words that reach outside the segment (a row's first and last, at most) are finished one
// element at a time, loads and stores alike: nothing outside the rectangle is read-modify-written, so the word that the end of
// one row shares with the start of the next is never raced for.  B loads the next canvas only in words that hold a weight != 1.
//
// The arithmetic is elementwise.hip's, rounding for rounding: edm_scale_kernel's (A), cfg_kernel's and edm_step_kernel's (B),
// then tiles.py's blend v = a + wgt * (b - a) as one multiply for the weight and three separately rounded fp32 operations,
// rounded to nearest even into bf16.  Plain operators under `fp contract(off)`, as in tile_blend.hip and for the reason its
// header gives: hipcc lowers __fmul_rn / __fadd_rn through library code the pragma does not reach and fuses them all the same.
// No v_fma / v_pk_fma may stand in the blend or the step (the fp32 division's own expansion uses them; that is the same
// expansion edm_step_kernel gets).
#include "drn_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int LT_W = 128;                     // destination elements per workgroup and row: 256 bytes, a full-size tile's row
constexpr int LT_H = 16;                      // destination rows per workgroup
constexpr int LT_WPR = (LT_W + 2) >> 1;       // 65: aligned words a row's 256 bytes can touch at misalignment 1
constexpr int LT_THREADS = 256;

// the two bf16 at p[0], p[1] (p on the 2-byte grid) as one word, from aligned 4-byte loads only
__device__ __forceinline__ uint32_t lt_load2(const bf16_t* p) {
    const uintptr_t a = (uintptr_t)p;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
    uint32_t v = w[0];
    if (a & 2) v = (v >> 16) | (w[1] << 16);
    return v;
}

__device__ __forceinline__ bf16_t lt_scale(bf16_t x, float c_in) { return f2bf(bf2f(x) * c_in); }

__global__ void __launch_bounds__(LT_THREADS) latent_tile_gather_kernel(
    const bf16_t* __restrict__ canvas, bf16_t* __restrict__ out, int64_t planes, int Hc, int Wc, int h, int w, int y_at, int x_at,
    float c_in, int tiles_x, int tiles_y) {
    const int tid = threadIdx.x;
    uint32_t blk = blockIdx.x;
    const int tx = (int)(blk % (uint32_t)tiles_x);
    blk /= (uint32_t)tiles_x;
    const int ty = (int)(blk % (uint32_t)tiles_y);
    const int64_t kp = blk / (uint32_t)tiles_y;                  // copy * planes + plane: the output's plane
    const int64_t plane = kp >= planes ? kp - planes : kp;
    const int x0 = tx * LT_W, y0 = ty * LT_H;
    const int cols = min(LT_W, w - x0), rows = min(LT_H, h - y0);
    // plane bases in 64 bits: five passes of a large picture pass 2^31 elements; one plane of either side does not
    const bf16_t* cplane = canvas + plane * ((int64_t)Hc * Wc);
    bf16_t* oplane = out + kp * ((int64_t)h * w);
    for (int i = tid; i < rows * LT_WPR; i += LT_THREADS) {
        const int r = i / LT_WPR, j = i - r * LT_WPR;
        bf16_t* o = oplane + (int64_t)(y0 + r) * w + x0;
        const bf16_t* c = cplane + (int64_t)(y_at + y0 + r) * Wc + (x_at + x0);
        const int s = 2 * j - (int)(((uintptr_t)o >> 1) & 1);    // segment element of this lane's word
        if (s >= cols) continue;
        if (s >= 0 && s + 2 <= cols) {
            const uint32_t v = lt_load2(c + s);
            *reinterpret_cast<uint32_t*>(o + s) =
                (uint32_t)lt_scale((bf16_t)(v & 0xffffu), c_in) | ((uint32_t)lt_scale((bf16_t)(v >> 16), c_in) << 16);
        } else {
            for (int k = 0; k < 2; ++k) {
                const int e = s + k;
                if (e < 0 || e >= cols) continue;
                o[e] = lt_scale(c[e], c_in);
            }
        }
    }
}

// one element's step result b: cfg_kernel's combine (HAS_U), then edm_step_kernel's update against the current canvas
template <bool HAS_U>
__device__ __forceinline__ float lt_step(bf16_t mo, bf16_t un, bf16_t cur, float g, float c_skip, float c_out, float sigma, float dt) {
    float m = bf2f(mo);
    if (HAS_U) {
        const float d = rbf(m - bf2f(un));
        m = rbf(m + rbf(g * d));
    }
    const float sm = bf2f(cur);
    const float denoised = c_skip * sm + c_out * m;
    const float deriv = (sm - denoised) / sigma;
    return rbf(sm + deriv * dt);
}

__device__ __forceinline__ bf16_t lt_blend(bf16_t a, float b, float wgt) {
    const float fa = bf2f(a);
    const float d = b - fa;
    const float m = wgt * d;
    return f2bf(fa + m);
}

template <bool HAS_U>
__global__ void __launch_bounds__(LT_THREADS) latent_tile_step_join_kernel(
    const bf16_t* __restrict__ mo, const bf16_t* __restrict__ un, float g, const bf16_t* __restrict__ cur, bf16_t* __restrict__ next,
    const float* __restrict__ wy, const float* __restrict__ wx, int Hc, int Wc, int h, int w, int y_at, int x_at, int ry, int rx,
    int Oy, int Ox, float c_skip, float c_out, float sigma, float dt, int tiles_x, int tiles_y) {
    __shared__ float wx_s[LT_W], wy_s[LT_H];
    const int tid = threadIdx.x;
    uint32_t blk = blockIdx.x;
    const int tx = (int)(blk % (uint32_t)tiles_x);
    blk /= (uint32_t)tiles_x;
    const int ty = (int)(blk % (uint32_t)tiles_y);
    const int64_t plane = blk / (uint32_t)tiles_y;
    const int x0 = tx * LT_W, y0 = ty * LT_H;                    // inside the written rectangle [ry, h) x [rx, w)
    const int cols = min(LT_W, w - rx - x0), rows = min(LT_H, h - ry - y0);

    if (tid < LT_W)
        wx_s[tid] = x0 + tid < Ox ? wx[x0 + tid] : 1.0f;
    else if (tid - LT_W < LT_H)
        wy_s[tid - LT_W] = y0 + tid - LT_W < Oy ? wy[y0 + tid - LT_W] : 1.0f;
    __syncthreads();

    // plane bases in 64 bits, as in the gather
    const int64_t cbase = plane * ((int64_t)Hc * Wc), tbase = plane * ((int64_t)h * w);
    for (int i = tid; i < rows * LT_WPR; i += LT_THREADS) {
        const int r = i / LT_WPR, j = i - r * LT_WPR;
        const int64_t coff = cbase + (int64_t)(y_at + ry + y0 + r) * Wc + (x_at + rx + x0);
        const int64_t toff = tbase + (int64_t)(ry + y0 + r) * w + (rx + x0);
        bf16_t* o = next + coff;
        const int s = 2 * j - (int)(((uintptr_t)o >> 1) & 1);    // segment element of this lane's word
        if (s >= cols) continue;
        const float wr = wy_s[r];
        if (s >= 0 && s + 2 <= cols) {
            const uint32_t vm = lt_load2(mo + toff + s), vc = lt_load2(cur + coff + s);
            const uint32_t vu = HAS_U ? lt_load2(un + toff + s) : 0u;
            const float w0 = wr * wx_s[s], w1 = wr * wx_s[s + 1];
            const float b0 = lt_step<HAS_U>((bf16_t)(vm & 0xffffu), (bf16_t)(vu & 0xffffu), (bf16_t)(vc & 0xffffu), g, c_skip, c_out,
                                            sigma, dt);
            const float b1 = lt_step<HAS_U>((bf16_t)(vm >> 16), (bf16_t)(vu >> 16), (bf16_t)(vc >> 16), g, c_skip, c_out, sigma, dt);
            uint32_t lo = f2bf(b0), hi = f2bf(b1);               // b is a bf16 value: exact
            if (!(w0 == 1.0f && w1 == 1.0f)) {
                const uint32_t a = *reinterpret_cast<const uint32_t*>(o + s);
                if (w0 != 1.0f) lo = lt_blend((bf16_t)(a & 0xffffu), b0, w0);
                if (w1 != 1.0f) hi = lt_blend((bf16_t)(a >> 16), b1, w1);
            }
            *reinterpret_cast<uint32_t*>(o + s) = lo | (hi << 16);
        } else {
            for (int k = 0; k < 2; ++k) {
                const int e = s + k;
                if (e < 0 || e >= cols) continue;
                const float wgt = wr * wx_s[e];
                const float b = lt_step<HAS_U>(mo[toff + e], HAS_U ? un[toff + e] : (bf16_t)0, cur[coff + e], g, c_skip, c_out, sigma, dt);
                o[e] = wgt == 1.0f ? f2bf(b) : lt_blend(o[e], b, wgt);
            }
        }
    }
}

// what both entry points ask of the geometry; -> workgroups per plane, or 0 for a refusal
int64_t lt_geometry(int64_t planes, int Hc, int Wc, int h, int w, int y_at, int x_at, int ry, int rx, int* tiles_x, int* tiles_y) {
    if (!(planes >= 1 && Hc >= 1 && Wc >= 1 && h >= 1 && w >= 1)) return 0;
    if (!(y_at >= 0 && x_at >= 0 && (int64_t)y_at + h <= Hc && (int64_t)x_at + w <= Wc)) return 0;
    if (!(0 <= ry && ry < h && 0 <= rx && rx < w)) return 0;
    const int64_t lim = (int64_t)1 << 31;
    if (!((int64_t)Hc * Wc < lim && (int64_t)h * w < lim)) return 0;
    *tiles_x = (w - rx + LT_W - 1) / LT_W;
    *tiles_y = (h - ry + LT_H - 1) / LT_H;
    return (int64_t)*tiles_x * *tiles_y;                         // < 2^31 / (128 * 16) by the plane limit
}

}  // namespace

extern "C" int drn_latent_tile_gather(const void* canvas, void* out, int64_t planes, int Hc, int Wc, int h, int w, int y_at,
                                      int x_at, float c_in, int copies, void* stream) {
    DRN_CHECK_ARG(canvas && out);
    DRN_CHECK_ARG((((uintptr_t)canvas | (uintptr_t)out) & 1) == 0);
    DRN_CHECK_ARG(copies == 1 || copies == 2);
    int tiles_x = 0, tiles_y = 0;
    const int64_t per_plane = lt_geometry(planes, Hc, Wc, h, w, y_at, x_at, 0, 0, &tiles_x, &tiles_y);
    DRN_CHECK_ARG(per_plane >= 1);
    DRN_CHECK_ARG(planes < ((int64_t)1 << 30) / per_plane);      // one workgroup index in 31 bits, both copies
    latent_tile_gather_kernel<<<dim3((unsigned)(per_plane * planes * copies)), dim3(LT_THREADS), 0, (hipStream_t)stream>>>(
        (const bf16_t*)canvas, (bf16_t*)out, planes, Hc, Wc, h, w, y_at, x_at, c_in, tiles_x, tiles_y);
    return drn_launch_status();
}

extern "C" int drn_latent_tile_step_join(const void* model_out, const void* uncond, float guidance, const void* canvas_cur,
                                         void* canvas_next, const float* wy, const float* wx, int64_t planes, int Hc, int Wc, int h,
                                         int w, int y_at, int x_at, int ry, int rx, int Oy, int Ox, float c_skip, float c_out,
                                         float sigma, float dt, void* stream) {
    DRN_CHECK_ARG(model_out && canvas_cur && canvas_next && canvas_cur != canvas_next);
    DRN_CHECK_ARG((((uintptr_t)model_out | (uintptr_t)uncond | (uintptr_t)canvas_cur | (uintptr_t)canvas_next) & 1) == 0);
    int tiles_x = 0, tiles_y = 0;
    const int64_t per_plane = lt_geometry(planes, Hc, Wc, h, w, y_at, x_at, ry, rx, &tiles_x, &tiles_y);
    DRN_CHECK_ARG(per_plane >= 1);
    DRN_CHECK_ARG(Oy >= 0 && Ox >= 0 && (int64_t)ry + Oy <= h && (int64_t)rx + Ox <= w);
    DRN_CHECK_ARG((wy == nullptr) == (Oy == 0) && (wx == nullptr) == (Ox == 0));
    DRN_CHECK_ARG((((uintptr_t)wy | (uintptr_t)wx) & 3) == 0);
    DRN_CHECK_ARG(sigma != 0.0f);
    DRN_CHECK_ARG(planes < ((int64_t)1 << 31) / per_plane);      // one workgroup index in 31 bits
    const dim3 grid((unsigned)(per_plane * planes)), block(LT_THREADS);
    const bf16_t *mo = (const bf16_t*)model_out, *un = (const bf16_t*)uncond, *cur = (const bf16_t*)canvas_cur;
    if (un)
        latent_tile_step_join_kernel<true><<<grid, block, 0, (hipStream_t)stream>>>(
            mo, un, guidance, cur, (bf16_t*)canvas_next, wy, wx, Hc, Wc, h, w, y_at, x_at, ry, rx, Oy, Ox, c_skip, c_out, sigma, dt,
            tiles_x, tiles_y);
    else
        latent_tile_step_join_kernel<false><<<grid, block, 0, (hipStream_t)stream>>>(
            mo, nullptr, guidance, cur, (bf16_t*)canvas_next, wy, wx, Hc, Wc, h, w, y_at, x_at, ry, rx, Oy, Ox, c_skip, c_out, sigma, dt,
            tiles_x, tiles_y);
    return drn_launch_status();
}
