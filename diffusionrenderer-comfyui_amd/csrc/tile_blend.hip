// Spatial tiles joined in pixel space (drn_tile_blend_u8, include/drn.h; the plan and the torch specification: tiles.py).  One
// rendered tile, uint8 [frames,h,w,3], is written into the picture's canvas, uint8 [frames,H,W,3], IN PLACE: its rows from ry and
// columns from rx on land at (y_at, x_at), the first Oy written rows and Ox written columns cross-faded over what the tiles above
// and to the left wrote there, everything behind both ramps copied.  Both sides are channel-interleaved bytes at any byte
// alignment, and a row segment of the canvas starts wherever (y_at + ry, x_at + rx) puts it.
//
// A workgroup owns TB_W written pixels x TB_H written rows of one frame; the weights of its rows and columns go into LDS once
// (1.0f behind a ramp, so "no ramp" and "behind the ramp" are one case).  A lane owns one ALIGNED 4-byte word of a canvas row
// segment, like restore.hip's output stage: the segment starts at byte misalignment m = address & 3, so word j holds segment
// bytes [4j - m, 4j - m + 4).  The tile's bytes for that word lie at the tile row's own misalignment: they are fetched as the two
// aligned words around them and shifted (each of the two holds at least one byte of the segment, so neither leaves the page the
// tile is in; the second is not fetched where the first holds all four).  A word whose two pixels have weight 1.0 is stored
// without loading the canvas; any other word loads it once.  Words that reach outside the segment (a row's first and last, at
// most) are finished bytewise, loads and stores alike: nothing outside the rectangle is read-modify-written, so the word that the
// end of one row shares with the start of the next (a tile as wide as the canvas) is never raced for.
//
// The blend is tiles.py's expression: wgt = wy * wx, v = a + wgt * (b - a), a the canvas byte and b the tile byte as fp32 -
// one multiply for the weight, then subtract, multiply and add as three separately rounded fp32 operations, rint (half to even),
// clamp.  Plain operators under `fp contract(off)`, as in elementwise.hip's window_blend: hipcc lowers __fmul_rn / __fadd_rn
// through library code the pragma does not reach and fuses them all the same.  No v_fma / v_pk_fma may appear in this kernel's
// ISA.  The byte-pair grid of the tests sees a fused blend at the overlap pair (5, 3) only (tests/test_tiles_cpu.py); for the
// overlaps nobody tested the listing is the check.
#include "drn_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int TB_W = 128;                     // written pixels per workgroup and row: 384 bytes
constexpr int TB_H = 16;                      // written rows per workgroup
constexpr int TB_WPR = (TB_W * 3 + 6) >> 2;   // 97: aligned canvas words a row's 384 bytes can touch at misalignment 3
constexpr int TB_THREADS = 256;

__device__ __forceinline__ uint32_t tb_blend(uint32_t a, uint32_t b, float wgt) {
    const float fa = (float)a;
    const float d = (float)b - fa;
    const float m = wgt * d;
    return (uint32_t)__builtin_amdgcn_fmed3f(__builtin_rintf(fa + m), 0.0f, 255.0f);
}

__global__ void __launch_bounds__(TB_THREADS) tile_blend_kernel(
    uint8_t* __restrict__ canvas, const uint8_t* __restrict__ tile, const float* __restrict__ wy, const float* __restrict__ wx,
    int H, int W, int h, int w, int y_at, int x_at, int ry, int rx, int Oy, int Ox, int tiles_x, int tiles_y) {
    __shared__ float wx_s[TB_W], wy_s[TB_H];
    const int tid = threadIdx.x;
    uint32_t blk = blockIdx.x;
    const int tx = (int)(blk % (uint32_t)tiles_x);
    blk /= (uint32_t)tiles_x;
    const int ty = (int)(blk % (uint32_t)tiles_y);
    const int64_t f = blk / (uint32_t)tiles_y;
    const int x0 = tx * TB_W, y0 = ty * TB_H;                    // inside the written rectangle [ry, h) x [rx, w)
    const int cols = min(TB_W, w - rx - x0), rows = min(TB_H, h - ry - y0);

    if (tid < TB_W)
        wx_s[tid] = x0 + tid < Ox ? wx[x0 + tid] : 1.0f;
    else if (tid - TB_W < TB_H)
        wy_s[tid - TB_W] = y0 + tid - TB_W < Oy ? wy[y0 + tid - TB_W] : 1.0f;
    __syncthreads();

    // frame bases in 64 bits: a long clip's canvas passes 2^31 bytes; one frame of either side does not
    uint8_t* cframe = canvas + f * ((int64_t)H * W * 3);
    const uint8_t* tframe = tile + f * ((int64_t)h * w * 3);
    const int L = cols * 3;
    for (int i = tid; i < rows * TB_WPR; i += TB_THREADS) {
        const int r = i / TB_WPR, j = i - r * TB_WPR;
        uint8_t* o = cframe + ((int64_t)(y_at + ry + y0 + r) * W + (x_at + rx + x0)) * 3;
        const uint8_t* t = tframe + ((int64_t)(ry + y0 + r) * w + (rx + x0)) * 3;
        const int s = 4 * j - (int)((uintptr_t)o & 3);           // segment byte of this lane's word
        if (s >= L) continue;
        const float wr = wy_s[r];
        if (s >= 0 && s + 4 <= L) {
            const uint8_t* ta = t + s;
            const int tm = (int)((uintptr_t)ta & 3);
            const uint32_t* tw = reinterpret_cast<const uint32_t*>(ta - tm);
            uint32_t v = tw[0];
            if (tm) v = (v >> (8 * tm)) | (tw[1] << (32 - 8 * tm));
            const int p0 = s / 3, p1 = (s + 3) / 3;              // the word's first and last pixel
            if (!(wr == 1.0f && wx_s[p0] == 1.0f && wx_s[p1] == 1.0f)) {
                const uint32_t c = *reinterpret_cast<const uint32_t*>(o + s);
                uint32_t out = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float wgt = wr * wx_s[(s + k) / 3];
                    const uint32_t a = (c >> (8 * k)) & 255u, b = (v >> (8 * k)) & 255u;
                    out |= (wgt == 1.0f ? b : tb_blend(a, b, wgt)) << (8 * k);
                }
                v = out;
            }
            *reinterpret_cast<uint32_t*>(o + s) = v;
        } else {
            for (int k = 0; k < 4; ++k) {
                const int sb = s + k;
                if (sb < 0 || sb >= L) continue;
                const float wgt = wr * wx_s[sb / 3];
                const uint32_t b = t[sb];
                o[sb] = (uint8_t)(wgt == 1.0f ? b : tb_blend(o[sb], b, wgt));
            }
        }
    }
}

}  // namespace

extern "C" int drn_tile_blend_u8(void* canvas, const void* tile, const void* wy, const void* wx, int64_t frames, int H, int W,
                                 int h, int w, int y_at, int x_at, int ry, int rx, int Oy, int Ox, void* stream) {
    DRN_CHECK_ARG(canvas && tile);
    DRN_CHECK_ARG(frames >= 1 && H >= 1 && W >= 1 && h >= 1 && w >= 1);
    DRN_CHECK_ARG(y_at >= 0 && x_at >= 0 && (int64_t)y_at + h <= H && (int64_t)x_at + w <= W);
    DRN_CHECK_ARG(0 <= ry && ry < h && 0 <= rx && rx < w);
    DRN_CHECK_ARG(Oy >= 0 && Ox >= 0 && (int64_t)ry + Oy <= h && (int64_t)rx + Ox <= w);
    DRN_CHECK_ARG((wy == nullptr) == (Oy == 0) && (wx == nullptr) == (Ox == 0));
    DRN_CHECK_ARG((((uintptr_t)wy | (uintptr_t)wx) & 3) == 0);
    const int64_t lim = (int64_t)1 << 31;
    DRN_CHECK_ARG((int64_t)H * W * 3 < lim && (int64_t)h * w * 3 < lim);
    const int tiles_x = (w - rx + TB_W - 1) / TB_W, tiles_y = (h - ry + TB_H - 1) / TB_H;
    const int64_t per_frame = (int64_t)tiles_x * tiles_y;        // < 2^31 / (3 * 128 * 16) by the frame limit
    DRN_CHECK_ARG(frames < lim / per_frame);                     // one workgroup index in 31 bits
    tile_blend_kernel<<<dim3((unsigned)(per_frame * frames)), dim3(TB_THREADS), 0, (hipStream_t)stream>>>(
        (uint8_t*)canvas, (const uint8_t*)tile, (const float*)wy, (const float*)wx, H, W, h, w, y_at, x_at, ry, rx, Oy, Ox, tiles_x,
        tiles_y);
    return drn_launch_status();
}
