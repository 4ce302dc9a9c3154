// Clip ingest with a fit to the model's grid from 8-bit frames (drn_fit_frames_u8, include/drn.h; the plan and the torch
// specification: fit.py).  uint8 frames [B,Ts,Hs,Ws,3] at ANY byte alignment -> [B,3,Td,Hd,Wd] bf16 in [-1, 1] in ONE launch:
// drn_fit_frames (fit.hip) on the frames unit[src], unit[i] = fp32(i) / 255 correctly rounded, bit for bit.
//
// The tiling is fit.hip's: a workgroup owns FU_TW output columns x `tile_h` output rows of one output frame, all three channels,
// and walks its rows in chunks whose source rows fit the planar fp32 stage (FU_RMAX rows).  What differs is how a source row
// reaches the stage.  A pixel is 3 bytes at any alignment, so no tap is read from global memory.  Per chunk, in passes of as many
// source rows as fit the raw buffer:
//   raw      the bytes the tile's columns read, byte span [3 * min lo, 3 * max(lo + n)) of every row, are copied into LDS with
//            ALIGNED 4-byte loads (a lane a word); the up to 3 bytes in front of the first whole word and behind the last are
//            copied bytewise, so nothing outside the span - and nothing outside the source - is read (restore.hip's scheme).  A
//            row's image sits at its own byte misalignment, word for word.  A span too long for the raw buffer (tables no
//            antialiased resize produces) is read from global memory bytewise.
//   horiz    a wave is a source row, a lane an output column: 3 channels x n taps, every byte through the 256-entry table
//            unit_s (filled once per workgroup with one correctly rounded division per thread: multiplying by 1.0f / 255 differs
//            from the division at 126 byte values), fma from 0 in tap order, into the planar stage.
//   vert     fit.hip's vertical pass, statement for statement: a lane filters 8 consecutive output columns of one row and channel
//            out of the stage and stores them as one 16-byte group.
// (The vertical pass is written out here a second time: moved into a function both files inline, it changed the block layout
// and the registers of fit.hip's kernel, and drn_fit_frames is to compile to what it compiled to.)
// lo and n are clamped into the source before use (taps_of), so no table content can take a read outside src, the raw buffer or
// the stage.
#include "resample_taps.h"

namespace {

constexpr int FU_TW = 64;         // output columns per workgroup (8 lanes x 8 columns)
constexpr int FU_RMAX = 48;       // staged source rows: 48 x 3 x 64 fp32 = 36 KiB
constexpr int FU_KMAX = 32;       // taps per axis
constexpr int FU_RAW = 6144;      // raw source bytes per pass: 16 rows of a 64-column tile at 1080p -> 576 x 1024 (372 bytes each)
constexpr int FU_THREADS = 256;   // = the table's 256 entries
constexpr int FU_WAVES = FU_THREADS / 64;
// LDS: stage 36 KiB + column weights 8 KiB + raw 6 KiB + unit 1 KiB + taps 0.5 KiB = 51.5 KiB: three workgroups per CU, like fit.hip

// one output column of one source row: p points at the first tap's pixel, w at the column's weights ([tap][column] in LDS)
template <typename P>
__device__ __forceinline__ void hfilter_u8(P p, const float* w, const float* unit, int n, float* acc) {
    for (int k = 0; k < n; ++k) {
        const float wk = w[k * FU_TW];
        acc[0] = fmaf(wk, unit[p[3 * k]], acc[0]);
        acc[1] = fmaf(wk, unit[p[3 * k + 1]], acc[1]);
        acc[2] = fmaf(wk, unit[p[3 * k + 2]], acc[2]);
    }
}

__global__ void __launch_bounds__(FU_THREADS) fit_frames_u8_kernel(
    const uint8_t* __restrict__ src, bf16_t* __restrict__ dst, int Ts, int Hs, int Ws, int Td, int Hd, int Wd,
    const int* __restrict__ t_idx, const int* __restrict__ y_lo_n, const float* __restrict__ y_w, int Ky,
    const int* __restrict__ x_lo_n, const float* __restrict__ x_w, int Kx, int tile_h, int tiles_x, int tiles_y) {
    __shared__ __attribute__((aligned(16))) float stage[FU_RMAX][3][FU_TW];
    __shared__ float xw_s[FU_KMAX][FU_TW];            // [tap][column]: lanes walk columns, conflict-free
    __shared__ uint32_t raw_s[FU_RAW / 4];
    __shared__ float unit_s[256];
    __shared__ int xlo_s[FU_TW], xn_s[FU_TW], span_s[2];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int blk = blockIdx.x;
    const int tx = blk % tiles_x;
    blk /= tiles_x;
    const int ty = blk % tiles_y;
    blk /= tiles_y;
    const int t = blk % Td, b = blk / Td;
    const int ts = min(max(t_idx[t], 0), Ts - 1);
    const int x_base = tx * FU_TW;
    const int cols = min(FU_TW, Wd - x_base);                   // a multiple of 8 (Wd % 16 == 0)
    const int y_begin = ty * tile_h, y_end = min(y_begin + tile_h, Hd);

    // the byte table, and the tile's column taps with the source columns they span -> LDS
    unit_s[tid] = __fdiv_rn((float)tid, 255.0f);
    if (tid == 0) {
        span_s[0] = Ws;
        span_s[1] = 0;
    }
    __syncthreads();
    if (tid < FU_TW) {
        Taps tp = {0, 1};
        if (tid < cols) {
            tp = taps_of(x_lo_n, x_base + tid, Kx, Ws);
            atomicMin(&span_s[0], tp.lo);
            atomicMax(&span_s[1], tp.lo + tp.n);
        }
        xlo_s[tid] = tp.lo;
        xn_s[tid] = tp.n;
    }
    for (int i = tid; i < Kx * FU_TW; i += FU_THREADS) {
        const int c = i % FU_TW, k = i / FU_TW;
        xw_s[k][c] = c < cols ? x_w[(int64_t)(x_base + c) * Kx + k] : 0.0f;
    }
    __syncthreads();
    const int s0 = span_s[0] * 3, span = span_s[1] * 3 - s0;     // bytes of a source row: [s0, s0 + span), 3 <= span <= Ws * 3
    const int pitch = (span + 6) & ~3;                          // a row's image: up to 3 bytes of misalignment in front
    const int pw = pitch >> 2;
    const int rg = FU_RAW / pitch;                              // source rows per raw pass; 0: the span does not fit, read directly

    const uint8_t* frame = src + ((int64_t)b * Ts + ts) * Hs * Ws * 3;
    const uint8_t* raw_b = reinterpret_cast<const uint8_t*>(raw_s);
    const int lo = xlo_s[lane], n = xn_s[lane];                 // horizontal pass: a lane keeps its column

    int y = y_begin;
    while (y < y_end) {
        // the chunk: as many output rows from y on as their source rows fit the stage (one row always fits: n <= 32 <= RMAX)
        Taps t0 = taps_of(y_lo_n, y, Ky, Hs);
        int r0 = t0.lo, r1 = t0.lo + t0.n, ye = y + 1;
        while (ye < y_end) {
            const Taps tn = taps_of(y_lo_n, ye, Ky, Hs);
            const int n0 = min(r0, tn.lo), n1 = max(r1, tn.lo + tn.n);
            if (n1 - n0 > FU_RMAX) break;
            r0 = n0;
            r1 = n1;
            ++ye;
        }
        const int rows = r1 - r0;
        __syncthreads();              // the previous chunk's readers are done with the stage

        // horizontal pass.  Columns past the picture store 0 and are never written out
        if (rg == 0) {
            for (int r = wave; r < rows; r += FU_WAVES) {
                float acc[3] = {0.0f, 0.0f, 0.0f};
                if (lane < cols) hfilter_u8(frame + ((int64_t)(r0 + r) * Ws + lo) * 3, &xw_s[0][lane], unit_s, n, acc);
                stage[r][0][lane] = acc[0];
                stage[r][1][lane] = acc[1];
                stage[r][2][lane] = acc[2];
            }
        } else {
            for (int g0 = 0; g0 < rows; g0 += rg) {
                const int grows = min(rg, rows - g0);
                // raw: word j of row rr holds span bytes [4j - mm, 4j - mm + 4), mm the row's byte misalignment in global memory
                // Four words per thread are loaded before any is stored: their latencies overlap
                for (int base = tid; base < grows * pw; base += 4 * FU_THREADS) {
                    uint32_t v[4] = {0, 0, 0, 0};
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int i = base + u * FU_THREADS;
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
                        if (base + u * FU_THREADS < grows * pw) raw_s[base + u * FU_THREADS] = v[u];
                }
                __syncthreads();
                for (int rr = wave; rr < grows; rr += FU_WAVES) {
                    const int r = g0 + rr;
                    const int mm = (int)((uintptr_t)(frame + (int64_t)(r0 + r) * Ws * 3 + s0) & 3);
                    float acc[3] = {0.0f, 0.0f, 0.0f};
                    if (lane < cols) hfilter_u8(raw_b + rr * pitch + mm + lo * 3 - s0, &xw_s[0][lane], unit_s, n, acc);
                    stage[r][0][lane] = acc[0];
                    stage[r][1][lane] = acc[1];
                    stage[r][2][lane] = acc[2];
                }
                if (g0 + rg < rows) __syncthreads();      // the raw buffer is free for the next rows
            }
        }
        __syncthreads();

        // vertical pass: item = (output row, channel, group of 8 columns)
        const int groups = cols >> 3;
        for (int i = tid; i < (ye - y) * 3 * groups; i += FU_THREADS) {
            const int g = i % groups, ch = (i / groups) % 3, yo = y + i / (3 * groups);
            const Taps tv = taps_of(y_lo_n, yo, Ky, Hs);
            const float* wrow = y_w + (int64_t)yo * Ky;
            float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            for (int k = 0; k < tv.n; ++k) {
                const float w = wrow[k];
                const float4* s = reinterpret_cast<const float4*>(&stage[tv.lo - r0 + k][ch][g * 8]);
                const float4 a = s[0], c4 = s[1];
                acc[0] = fmaf(w, a.x, acc[0]); acc[1] = fmaf(w, a.y, acc[1]);
                acc[2] = fmaf(w, a.z, acc[2]); acc[3] = fmaf(w, a.w, acc[3]);
                acc[4] = fmaf(w, c4.x, acc[4]); acc[5] = fmaf(w, c4.y, acc[5]);
                acc[6] = fmaf(w, c4.z, acc[6]); acc[7] = fmaf(w, c4.w, acc[7]);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = fmaf(2.0f, acc[j], -1.0f);     // 2 * acc is exact: one rounding, like * 2 - 1
            bf16_t* o = dst + ((((int64_t)b * 3 + ch) * Td + t) * Hd + yo) * Wd + x_base + g * 8;
            *reinterpret_cast<uint4*>(o) = pack8(acc);
        }
        y = ye;
    }
}

}  // namespace

extern "C" int drn_fit_frames_u8(const uint8_t* src, void* dst_bf16, int B, int Ts, int Hs, int Ws, int Td, int Hd, int Wd,
                                 const int* t_idx, const int* y_lo_n, const float* y_w, int Ky,
                                 const int* x_lo_n, const float* x_w, int Kx, void* stream) {
    DRN_CHECK_ARG(src && dst_bf16 && t_idx && y_lo_n && y_w && x_lo_n && x_w);
    DRN_CHECK_ARG(B >= 1 && Ts >= 1 && Hs >= 1 && Ws >= 1 && Td >= 1 && Hd >= 1 && Wd >= 1);
    DRN_CHECK_ARG(Ky >= 1 && Ky <= FU_KMAX && Kx >= 1 && Kx <= FU_KMAX);
    DRN_CHECK_ARG(Hd % 16 == 0 && Wd % 16 == 0);
    const int64_t lim = (int64_t)1 << 31;
    DRN_CHECK_ARG((int64_t)B * 3 * Td * Hd * Wd < lim && (int64_t)B * Ts * Hs * Ws * 3 < lim);
    DRN_CHECK_ARG((((uintptr_t)y_w | (uintptr_t)x_w | (uintptr_t)t_idx | (uintptr_t)y_lo_n | (uintptr_t)x_lo_n) & 3) == 0);
    DRN_CHECK_ARG(((uintptr_t)dst_bf16 & 15) == 0);
    const int tile_h = resample_tile_rows(Ky, FU_RMAX, 16);
    const int tiles_x = (Wd + FU_TW - 1) / FU_TW, tiles_y = (Hd + tile_h - 1) / tile_h;
    const int64_t blocks = (int64_t)tiles_x * tiles_y * Td * B;          // <= the output's element count / 128 < 2^31
    fit_frames_u8_kernel<<<dim3((unsigned)blocks), dim3(FU_THREADS), 0, (hipStream_t)stream>>>(
        src, (bf16_t*)dst_bf16, Ts, Hs, Ws, Td, Hd, Wd, t_idx, y_lo_n, y_w, Ky, x_lo_n, x_w, Kx, tile_h, tiles_x, tiles_y);
    return drn_launch_status();
}
