// The fit's way back (drn_restore_frames_u8, include/drn.h; the plan and the torch specification: fit.py).  The uint8 result of
// the post-process, [B,Ts,Hs,Ws,3] at the model's size, -> uint8 [B,Td,Hd,Wd,3] at the source's size in ONE launch: separable
// resampling by per-axis tap tables (the antialiased triangle filter), the time padding cut (Td <= Ts), round to nearest even,
// clamp.  Both sides are channel-interleaved bytes, and Hd, Wd are whatever the source was: an output row of Wd * 3 bytes starts
// at any byte alignment.
//
// A workgroup owns RS_TW output pixels x `tile_h` output rows of one frame and walks its rows in chunks whose source rows fit the
// fp32 stage (`rmax` rows), like fit.hip; the tile's column AND row taps are read into LDS once, in parallel (every thread cuts
// the chunks: out of global memory that is a chain of dependent loads per tile).  A tile whose rows fit the stage together - every
// up-scale - is one chunk, found without a walk.  In the three filter passes a wave is a row and a lane a piece of it.  Per chunk:
//   raw      the source bytes the tile's columns read, rows [r0, r1) x byte span [3 * min lo, 3 * max(lo + n)), are copied into
//            LDS with ALIGNED 4-byte loads (a lane a word, a tile's span of about 110 bytes at 576 x 1024 -> 1080 x 1920 is less
//            than half a wave-instruction); the up to 3 bytes in front of the first whole word and behind the last are copied
//            bytewise, so nothing outside the span is read.  A row's image sits at its own byte misalignment, word for word.
//            A span too long for the raw buffer (tables no antialiased resize produces) is read from global memory directly.
//   horiz    a lane is an output pixel: 3 channels x n taps from the raw bytes, fma from 0 in tap order, into
//            stage[row][pixel * 3 + ch] (the output's own byte order, lanes 3 floats apart: conflict-free).
//   vert     a lane owns 4 consecutive floats of a stage row (one 16-byte LDS read per tap), fma from 0 in tap order, rint,
//            clamp, and packs the 4 bytes into one word of the LDS output tile.
//   out      a lane owns one ALIGNED 4-byte word of dst: a row segment starts at byte misalignment m = address & 3, so a word is
//            two neighbouring tile words shifted by (4 - m) bytes.  Words that reach outside the segment (the first and last of a
//            row, at most) are finished bytewise: nothing outside the segment is written.
// lo and n are clamped into the source before use (taps_of), so no table content can take a read outside src or the stage.
// LDS is sized per launch from the tap counts and the scale (stage rows, weights, output tile): 31 KiB at 576 x 1024 ->
// 1080 x 1920, five workgroups per CU; 51 KiB at most.
#include "resample_taps.h"

namespace {

constexpr int RS_TW = 64;             // output pixels per workgroup and row: 192 bytes
constexpr int RS_ROW = RS_TW * 3;     // floats per stage row, bytes per tile row
constexpr int RS_RMAX = 32;           // staged source rows, at most: 32 x 192 fp32 = 24 KiB
constexpr int RS_KMAX = 32;           // taps per axis
constexpr int RS_TH = 32;             // output rows per workgroup, at most
constexpr int RS_RAW = 8192;          // raw source bytes per pass
constexpr int RS_OPITCH = RS_ROW / 4 + 1;     // words per output tile row: a shifted word reads its neighbour
constexpr int RS_THREADS = 256;
constexpr int RS_WAVES = RS_THREADS / 64;

// one output pixel of one source row: p points at the first tap's pixel, w at the column's weights ([tap][column] in LDS)
template <typename P>
__device__ __forceinline__ void hfilter(P p, const float* w, int n, float* acc) {
    for (int k = 0; k < n; ++k) {
        const float wk = w[k * RS_TW];
        acc[0] = fmaf(wk, (float)p[3 * k], acc[0]);
        acc[1] = fmaf(wk, (float)p[3 * k + 1], acc[1]);
        acc[2] = fmaf(wk, (float)p[3 * k + 2], acc[2]);
    }
}

__device__ __forceinline__ uint32_t to_byte(float v) { return (uint32_t)__builtin_amdgcn_fmed3f(__builtin_rintf(v), 0.0f, 255.0f); }

// dynamic LDS of a launch, in 4-byte words: stage | column weights | row weights | output tile | raw source bytes
__host__ __device__ constexpr int rs_lds_words(int rmax, int tile_h, int Ky, int Kx) {
    return rmax * RS_ROW + Kx * RS_TW + tile_h * Ky + tile_h * RS_OPITCH + RS_RAW / 4;
}

__global__ void __launch_bounds__(RS_THREADS) restore_frames_kernel(
    const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int Ts, int Hs, int Ws, int Td, int Hd, int Wd,
    const int* __restrict__ y_lo_n, const float* __restrict__ y_w, int Ky,
    const int* __restrict__ x_lo_n, const float* __restrict__ x_w, int Kx, int tile_h, int rmax, int tiles_x, int tiles_y) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    float* stage = rs_lds;                                      // [rmax][RS_ROW]
    float* xw_s = stage + rmax * RS_ROW;                        // [Kx][RS_TW]: lanes walk columns, conflict-free
    float* yw_s = xw_s + Kx * RS_TW;                            // [tile_h][Ky]
    uint32_t* out_s = reinterpret_cast<uint32_t*>(yw_s + tile_h * Ky);       // [tile_h][RS_OPITCH]
    uint32_t* raw_s = out_s + tile_h * RS_OPITCH;               // [RS_RAW / 4]
    __shared__ int xlo_s[RS_TW], xn_s[RS_TW], ylo_s[RS_TH], yn_s[RS_TH], span_s[4];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int blk = blockIdx.x;
    const int tx = blk % tiles_x;
    blk /= tiles_x;
    const int ty = blk % tiles_y;
    blk /= tiles_y;
    const int t = blk % Td, b = blk / Td;
    const int x_base = tx * RS_TW;
    const int cols = min(RS_TW, Wd - x_base);                   // 1..64
    const int y_begin = ty * tile_h, y_end = min(y_begin + tile_h, Hd);

    // the tile's column and row taps -> LDS, with the source columns and rows they span
    if (tid == 0) {
        span_s[0] = Ws;
        span_s[1] = 0;
        span_s[2] = Hs;
        span_s[3] = 0;
    }
    __syncthreads();
    if (tid < RS_TW) {
        Taps tp = {0, 1};
        if (tid < cols) {
            tp = taps_of(x_lo_n, x_base + tid, Kx, Ws);
            atomicMin(&span_s[0], tp.lo);
            atomicMax(&span_s[1], tp.lo + tp.n);
        }
        xlo_s[tid] = tp.lo;
        xn_s[tid] = tp.n;
    } else if (tid - RS_TW < y_end - y_begin) {
        const Taps tp = taps_of(y_lo_n, y_begin + tid - RS_TW, Ky, Hs);
        ylo_s[tid - RS_TW] = tp.lo;
        yn_s[tid - RS_TW] = tp.n;
        atomicMin(&span_s[2], tp.lo);
        atomicMax(&span_s[3], tp.lo + tp.n);
    }
    for (int i = tid; i < (y_end - y_begin) * Ky; i += RS_THREADS) yw_s[i] = y_w[(int64_t)y_begin * Ky + i];
    for (int i = tid; i < Kx * RS_TW; i += RS_THREADS) {
        const int c = i % RS_TW, k = i / RS_TW;
        xw_s[i] = c < cols ? x_w[(int64_t)(x_base + c) * Kx + k] : 0.0f;
    }
    __syncthreads();
    const int s0 = span_s[0] * 3, span = span_s[1] * 3 - s0;     // bytes of a source row: [s0, s0 + span), 3 <= span <= Ws * 3
    const int pitch = (span + 6) & ~3;                          // a row's image: up to 3 bytes of misalignment in front
    const int pw = pitch >> 2;
    const int rg = RS_RAW / pitch;                              // source rows per raw pass; 0: the span does not fit, read directly
    const bool one_chunk = span_s[3] - span_s[2] <= rmax;

    const uint8_t* frame = src + ((int64_t)b * Ts + t) * Hs * Ws * 3;
    uint8_t* oframe = dst + ((int64_t)b * Td + t) * Hd * Wd * 3;
    const uint8_t* raw_b = reinterpret_cast<const uint8_t*>(raw_s);
    const int lo = xlo_s[lane], n = xn_s[lane];                 // horizontal pass: a lane keeps its column
    const int L = cols * 3, groups = (L + 3) >> 2;

    int y = y_begin;
    while (y < y_end) {
        // the chunk: as many output rows from y on as their source rows fit the stage (one row always fits: n <= Ky <= rmax)
        int r0, r1, ye;
        if (one_chunk) {
            r0 = span_s[2];
            r1 = span_s[3];
            ye = y_end;
        } else {
            r0 = ylo_s[y - y_begin];
            r1 = r0 + yn_s[y - y_begin];
            ye = y + 1;
            while (ye < y_end) {
                const int tl = ylo_s[ye - y_begin];
                const int n0 = min(r0, tl), n1 = max(r1, tl + yn_s[ye - y_begin]);
                if (n1 - n0 > rmax) break;
                r0 = n0;
                r1 = n1;
                ++ye;
            }
        }
        const int rows = r1 - r0;
        __syncthreads();              // the previous chunk's readers are done with the stage

        // horizontal pass.  Columns past the picture store 0 and are never written out
        if (rg == 0) {
            for (int r = wave; r < rows; r += RS_WAVES) {
                float acc[3] = {0.0f, 0.0f, 0.0f};
                if (lane < cols) hfilter(frame + ((int64_t)(r0 + r) * Ws + lo) * 3, xw_s + lane, n, acc);
                float* st = stage + r * RS_ROW + 3 * lane;
                st[0] = acc[0];
                st[1] = acc[1];
                st[2] = acc[2];
            }
            __syncthreads();
        } else {
            for (int g0 = 0; g0 < rows; g0 += rg) {
                const int grows = min(rg, rows - g0);
                // raw: word j of row rr holds span bytes [4j - mm, 4j - mm + 4), mm the row's byte misalignment in global memory
                // Four words per thread are loaded before any is stored: their latencies overlap
                for (int base = tid; base < grows * pw; base += 4 * RS_THREADS) {
                    uint32_t v[4] = {0, 0, 0, 0};
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int i = base + u * RS_THREADS;
                        if (i >= grows * pw) continue;
                        const int rr = i / pw, j = i - rr * pw;
                        const uint8_t* g = frame + (int64_t)(r0 + g0 + rr) * Ws * 3 + s0;
                        const int s = 4 * j - (int)((uintptr_t)g & 3);
                        if (s >= 0 && s + 4 <= span) {
                            v[u] = *reinterpret_cast<const uint32_t*>(g + s);
                        } else {
                            for (int k = 0; k < 4; ++k)
                                if (s + k >= 0 && s + k < span) v[u] |= (uint32_t)g[s + k] << (8 * k);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (base + u * RS_THREADS < grows * pw) raw_s[base + u * RS_THREADS] = v[u];
                }
                __syncthreads();
                for (int rr = wave; rr < grows; rr += RS_WAVES) {
                    const int r = g0 + rr;
                    const int mm = (int)((uintptr_t)(frame + (int64_t)(r0 + r) * Ws * 3 + s0) & 3);
                    float acc[3] = {0.0f, 0.0f, 0.0f};
                    if (lane < cols) hfilter(raw_b + rr * pitch + mm + lo * 3 - s0, xw_s + lane, n, acc);
                    float* st = stage + r * RS_ROW + 3 * lane;
                    st[0] = acc[0];
                    st[1] = acc[1];
                    st[2] = acc[2];
                }
                __syncthreads();      // the stage rows are written; the raw buffer is free for the next rows
            }
        }

        // vertical pass: a wave is an output row, a lane 4 consecutive bytes of it
        for (int row = wave; row < ye - y; row += RS_WAVES) {
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
        for (int row = wave; row < ye - y; row += RS_WAVES) {
            const uint32_t* orow = out_s + (y - y_begin + row) * RS_OPITCH;
            uint8_t* o = oframe + ((int64_t)(y + row) * Wd + x_base) * 3;
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
    DRN_CHECK_ARG(Ky >= 1 && Ky <= RS_KMAX && Kx >= 1 && Kx <= RS_KMAX);
    const int64_t lim = (int64_t)1 << 31;
    DRN_CHECK_ARG((int64_t)B * Td * Hd * Wd * 3 < lim && (int64_t)B * Ts * Hs * Ws * 3 < lim);
    DRN_CHECK_ARG((((uintptr_t)y_w | (uintptr_t)x_w | (uintptr_t)y_lo_n | (uintptr_t)x_lo_n) & 3) == 0);
    // stage rows: what a workgroup's output rows read at the picture's scale, Ky at least.  A hint, like the rows themselves
    int tile_h = resample_tile_rows(Ky, RS_RMAX, RS_TH);
    tile_h = tile_h > Hd ? Hd : tile_h;
    int rmax = (int)((double)tile_h * Hs / Hd) + Ky + 2;
    rmax = rmax > RS_RMAX ? RS_RMAX : rmax;
    const int tiles_x = (Wd + RS_TW - 1) / RS_TW, tiles_y = (Hd + tile_h - 1) / tile_h;
    const int64_t blocks = (int64_t)tiles_x * tiles_y * Td * B;          // <= the output's pixel count < 2^31
    const size_t lds = sizeof(float) * (size_t)rs_lds_words(rmax, tile_h, Ky, Kx);
    restore_frames_kernel<<<dim3((unsigned)blocks), dim3(RS_THREADS), lds, (hipStream_t)stream>>>(
        src, dst, Ts, Hs, Ws, Td, Hd, Wd, y_lo_n, y_w, Ky, x_lo_n, x_w, Kx, tile_h, rmax, tiles_x, tiles_y);
    return drn_launch_status();
}
