// The fit's way back (drn_restore_frames_u8, include/drn.h; the plan and the torch specification: fit.py).  The uint8 result of
// the post-process, [B,Ts,Hs,Ws,3] at the model's size, -> uint8 [B,Td,Hd,Wd,3] at the source's size in ONE launch: separable
// resampling by per-axis tap tables (the antialiased triangle filter), the time padding cut (Td <= Ts), round to nearest even,
// clamp.  Both sides are channel-interleaved bytes, and Hd, Wd are whatever the source was: an output row of Wd * 3 bytes starts
// at any byte alignment.
//
// The tiling, chunks and raw staging are resample_core.h's, with `rmax` stage rows.  The tile's column AND row taps are read into
// LDS once, in parallel (every thread cuts the chunks: out of global memory that is a chain of dependent loads per tile).  A tile
// whose rows fit the stage together - every up-scale - is one chunk, found without a walk.  A wave is a row and a lane a piece of
// it.  Per chunk:
//   horiz    hpass_bytes (a tile's span of about 110 bytes at 576 x 1024 -> 1080 x 1920 is less than half a wave-instruction of
//            raw words): a lane is an output pixel, 3 channels x n taps from the raw bytes, fma from 0 in tap order, into
//            stage[row][pixel * 3 + ch] (the output's own byte order, lanes 3 floats apart: conflict-free).
//   vert     a lane owns 4 consecutive floats of a stage row (one 16-byte LDS read per tap), fma from 0 in tap order, rint,
//            clamp, and packs the 4 bytes into one word of the LDS output tile.
//   out      a lane owns one ALIGNED 4-byte word of dst: a row segment starts at byte misalignment m = address & 3, so a word is
//            two neighbouring tile words shifted by (4 - m) bytes.  Words that reach outside the segment (the first and last of a
//            row, at most) are finished bytewise: nothing outside the segment is written.
// LDS is sized per launch from the tap counts and the scale (stage rows, weights, output tile): 31 KiB at 576 x 1024 ->
// 1080 x 1920, five workgroups per CU; 51 KiB at most.
#include "resample_core.h"

namespace {

constexpr int RS_ROW = RC_TW * 3;     // floats per stage row, bytes per tile row
constexpr int RS_RMAX = 32;           // staged source rows, at most: 32 x 192 fp32 = 24 KiB
constexpr int RS_TH = 32;             // output rows per workgroup, at most
constexpr int RS_RAW = 8192;          // raw source bytes per pass
constexpr int RS_OPITCH = RS_ROW / 4 + 1;     // words per output tile row: a shifted word reads its neighbour

__device__ __forceinline__ uint32_t to_byte(float v) { return (uint32_t)__builtin_amdgcn_fmed3f(__builtin_rintf(v), 0.0f, 255.0f); }

// dynamic LDS of a launch, in 4-byte words: stage | column weights | row weights | output tile | raw source bytes
__host__ __device__ constexpr int rs_lds_words(int rmax, int tile_h, int Ky, int Kx) {
    return rmax * RS_ROW + Kx * RC_TW + tile_h * Ky + tile_h * RS_OPITCH + RS_RAW / 4;
}

__global__ void __launch_bounds__(RC_THREADS) restore_frames_kernel(
    const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int Ts, int Hs, int Ws, int Td, int Hd, int Wd,
    const int* __restrict__ y_lo_n, const float* __restrict__ y_w, int Ky,
    const int* __restrict__ x_lo_n, const float* __restrict__ x_w, int Kx, int tile_h, int rmax, int tiles_x, int tiles_y) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    float* stage = rs_lds;                                      // [rmax][RS_ROW]
    float* xw_s = stage + rmax * RS_ROW;                        // [Kx][RC_TW]
    float* yw_s = xw_s + Kx * RC_TW;                            // [tile_h][Ky]
    uint32_t* out_s = reinterpret_cast<uint32_t*>(yw_s + tile_h * Ky);       // [tile_h][RS_OPITCH]
    uint32_t* raw_s = out_s + tile_h * RS_OPITCH;               // [RS_RAW / 4]
    __shared__ int xlo_s[RC_TW], xn_s[RC_TW], ylo_s[RS_TH], yn_s[RS_TH], span_s[4];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Tile tl = tile_of_block(tiles_x, tiles_y, tile_h, Td, Hd, Wd);      // cols: 1..64
    const int y_begin = tl.y_begin, y_end = tl.y_end;

    // the tile's column and row taps -> LDS, with the source columns and rows they span
    if (tid == 0) {
        span_s[0] = Ws;
        span_s[1] = 0;
        span_s[2] = Hs;
        span_s[3] = 0;
    }
    __syncthreads();
    stage_column_taps(x_lo_n, x_w, Kx, Ws, tl, xlo_s, xn_s, xw_s, span_s);
    if (tid >= RC_TW && tid - RC_TW < y_end - y_begin) {
        const Taps tp = taps_of(y_lo_n, y_begin + tid - RC_TW, Ky, Hs);
        ylo_s[tid - RC_TW] = tp.lo;
        yn_s[tid - RC_TW] = tp.n;
        atomicMin(&span_s[2], tp.lo);
        atomicMax(&span_s[3], tp.lo + tp.n);
    }
    for (int i = tid; i < (y_end - y_begin) * Ky; i += RC_THREADS) yw_s[i] = y_w[(int64_t)y_begin * Ky + i];
    __syncthreads();
    const RowSpan sp = row_span(span_s, RS_RAW);
    const bool one_chunk = span_s[3] - span_s[2] <= rmax;

    const uint8_t* frame = src + ((int64_t)tl.b * Ts + tl.t) * Hs * Ws * 3;
    uint8_t* oframe = dst + ((int64_t)tl.b * Td + tl.t) * Hd * Wd * 3;
    const int lo = xlo_s[lane], n = xn_s[lane];                 // horizontal pass: a lane keeps its column
    const int L = tl.cols * 3, groups = (L + 3) >> 2;

    int y = y_begin;
    while (y < y_end) {
        Chunk ch = {span_s[2], span_s[3], y_end};
        if (!one_chunk) ch = cut_chunk(y, y_end, rmax, [&](int i) { return Taps{ylo_s[i - y_begin], yn_s[i - y_begin]}; });
        const int r0 = ch.r0, ye = ch.ye;
        __syncthreads();              // the previous chunk's readers are done with the stage

        hpass_bytes(frame, Ws, r0, ch.r1 - r0, sp, raw_s, xw_s + lane, lo, n, lane < tl.cols,
                    [](uint8_t v) { return (float)v; },
                    [&](int r, const float* acc) {
                        float* st = stage + r * RS_ROW + 3 * lane;
                        st[0] = acc[0];
                        st[1] = acc[1];
                        st[2] = acc[2];
                    });

        // vertical pass: a wave is an output row, a lane 4 consecutive bytes of it
        for (int row = wave; row < ye - y; row += RC_WAVES) {
            if (lane >= groups) continue;
            const int yt = y - y_begin + row;
            const int vn = yn_s[yt];
            const float* wrow = yw_s + yt * Ky;
            const float* st = stage + (ylo_s[yt] - r0) * RS_ROW + lane * 4;
            float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int k = 0; k < vn; ++k) {
                const float w = wrow[k];
                const float4 a = *reinterpret_cast<const float4*>(st + k * RS_ROW);
                acc[0] = fmaf(w, a.x, acc[0]);
                acc[1] = fmaf(w, a.y, acc[1]);
                acc[2] = fmaf(w, a.z, acc[2]);
                acc[3] = fmaf(w, a.w, acc[3]);
            }
            out_s[yt * RS_OPITCH + lane] = to_byte(acc[0]) | to_byte(acc[1]) << 8 | to_byte(acc[2]) << 16 | to_byte(acc[3]) << 24;
        }
        __syncthreads();

        // out: a wave is an output row, a lane an aligned word of dst; segment byte s of the row is byte s of the tile row
        for (int row = wave; row < ye - y; row += RC_WAVES) {
            const uint32_t* orow = out_s + (y - y_begin + row) * RS_OPITCH;
            uint8_t* o = oframe + ((int64_t)(y + row) * Wd + tl.x_base) * 3;
            const int m = (int)((uintptr_t)o & 3);
            const int s = 4 * lane - m;
            if (s >= L) continue;                               // (lanes 49 .. 63 always: a row has at most 49 words)
            if (s >= 0 && s + 4 <= L) {
                const int sh = 8 * (s & 3);
                const uint32_t w0 = orow[s >> 2], w1 = orow[(s >> 2) + 1];
                *reinterpret_cast<uint32_t*>(o + s) = sh ? (w0 >> sh) | (w1 << (32 - sh)) : w0;
            } else {
                for (int k = 0; k < 4; ++k) {
                    const int sb = s + k;
                    if (sb >= 0 && sb < L) o[sb] = (uint8_t)(orow[sb >> 2] >> (8 * (sb & 3)));
                }
            }
        }
        y = ye;
    }
}

}  // namespace

extern "C" int drn_restore_frames_u8(const uint8_t* src, uint8_t* dst, int B, int Ts, int Hs, int Ws, int Td, int Hd, int Wd,
                                     const int* y_lo_n, const float* y_w, int Ky, const int* x_lo_n, const float* x_w, int Kx,
                                     void* stream) {
    DRN_CHECK_ARG(src && dst && y_lo_n && y_w && x_lo_n && x_w);
    DRN_CHECK_ARG(B >= 1 && Ts >= 1 && Hs >= 1 && Ws >= 1 && Td >= 1 && Hd >= 1 && Wd >= 1);
    DRN_CHECK_ARG(Td <= Ts);
    DRN_CHECK_ARG(Ky >= 1 && Ky <= RC_KMAX && Kx >= 1 && Kx <= RC_KMAX);
    const int64_t lim = (int64_t)1 << 31;
    DRN_CHECK_ARG((int64_t)B * Td * Hd * Wd * 3 < lim && (int64_t)B * Ts * Hs * Ws * 3 < lim);
    DRN_CHECK_ARG((((uintptr_t)y_w | (uintptr_t)x_w | (uintptr_t)y_lo_n | (uintptr_t)x_lo_n) & 3) == 0);
    // stage rows: what a workgroup's output rows read at the picture's scale, Ky at least.  A hint, like the rows themselves
    int tile_h = resample_tile_rows(Ky, RS_RMAX, RS_TH);
    tile_h = tile_h > Hd ? Hd : tile_h;
    int rmax = (int)((double)tile_h * Hs / Hd) + Ky + 2;
    rmax = rmax > RS_RMAX ? RS_RMAX : rmax;
    const int tiles_x = (Wd + RC_TW - 1) / RC_TW, tiles_y = (Hd + tile_h - 1) / tile_h;
    const int64_t blocks = (int64_t)tiles_x * tiles_y * Td * B;          // <= the output's pixel count < 2^31
    const size_t lds = sizeof(float) * (size_t)rs_lds_words(rmax, tile_h, Ky, Kx);
    restore_frames_kernel<<<dim3((unsigned)blocks), dim3(RC_THREADS), lds, (hipStream_t)stream>>>(
        src, dst, Ts, Hs, Ws, Td, Hd, Wd, y_lo_n, y_w, Ky, x_lo_n, x_w, Kx, tile_h, rmax, tiles_x, tiles_y);
    return drn_launch_status();
}
