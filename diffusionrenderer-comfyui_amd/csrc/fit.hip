// Clip ingest with a fit to the model's grid (drn_fit_frames, include/drn.h; the plan and the torch specification: fit.py).
// ComfyUI frames [B,Ts,Hs,Ws,3] fp32 in [0, 1] -> [B,3,Td,Hd,Wd] bf16 in [-1, 1] in ONE launch: separable resampling by per-axis
// tap tables (the antialiased triangle filter, crop offsets folded into the tables), frame gather (time padding), * 2 - 1,
// round to nearest even, transpose.
//
// A workgroup owns FIT_TW output columns x `tile_h` output rows of one output frame, all three channels.  It walks its rows in
// chunks whose source rows fit the LDS stage (FIT_RMAX rows): the source rows of a chunk are filtered horizontally into LDS
// (a wave is one staged row, a lane one output column: it reads whole 12-byte pixels, neighbouring lanes neighbouring pixels, and
// writes the stage planar per channel, 64 consecutive floats per wave and channel), then every lane filters 8 consecutive output
// columns of one row and channel vertically out of LDS (two 16-byte LDS reads per tap) and stores them as one 16-byte group.  Every loop runs over a row's own tap count; lo and n are clamped into the source before use, so no table
// content can take a read outside the source or the stage.  A single tap of weight 1.0 passes its source value through both
// passes unchanged (fma(1, v, 0) == v): scale 1 is a bit-exact copy.
#include "resample_taps.h"

namespace {

constexpr int FIT_TW = 64;        // output columns per workgroup (8 lanes x 8 columns)
constexpr int FIT_RMAX = 48;      // staged source rows: 48 x 3 x 64 fp32 = 36 KiB
constexpr int FIT_KMAX = 32;      // taps per axis
constexpr int FIT_THREADS = 256;

__global__ void __launch_bounds__(FIT_THREADS) fit_frames_kernel(
    const float* __restrict__ src, bf16_t* __restrict__ dst, int Ts, int Hs, int Ws, int Td, int Hd, int Wd,
    const int* __restrict__ t_idx, const int* __restrict__ y_lo_n, const float* __restrict__ y_w, int Ky,
    const int* __restrict__ x_lo_n, const float* __restrict__ x_w, int Kx, int tile_h, int tiles_x, int tiles_y) {
    __shared__ __attribute__((aligned(16))) float stage[FIT_RMAX][3][FIT_TW];
    __shared__ float xw_s[FIT_KMAX][FIT_TW];          // [tap][column]: lanes walk columns, conflict-free
    __shared__ int xlo_s[FIT_TW], xn_s[FIT_TW];

    const int tid = threadIdx.x;
    int blk = blockIdx.x;
    const int tx = blk % tiles_x;
    blk /= tiles_x;
    const int ty = blk % tiles_y;
    blk /= tiles_y;
    const int t = blk % Td, b = blk / Td;
    const int ts = min(max(t_idx[t], 0), Ts - 1);
    const int x_base = tx * FIT_TW;
    const int cols = min(FIT_TW, Wd - x_base);                  // a multiple of 8 (Wd % 16 == 0)
    const int y_begin = ty * tile_h, y_end = min(y_begin + tile_h, Hd);

    // the tile's column taps -> LDS (columns past the picture: one tap of weight 0 at source column 0, never stored)
    if (tid < FIT_TW) {
        Taps tp = {0, 1};
        if (tid < cols) tp = taps_of(x_lo_n, x_base + tid, Kx, Ws);
        xlo_s[tid] = tp.lo;
        xn_s[tid] = tp.n;
    }
    for (int i = tid; i < Kx * FIT_TW; i += FIT_THREADS) {
        const int c = i % FIT_TW, k = i / FIT_TW;
        xw_s[k][c] = c < cols ? x_w[(int64_t)(x_base + c) * Kx + k] : 0.0f;
    }

    const float* frame = src + ((int64_t)b * Ts + ts) * Hs * Ws * 3;
    int y = y_begin;
    while (y < y_end) {
        // the chunk: as many output rows from y on as their source rows fit the stage (one row always fits: n <= 32 <= RMAX)
        Taps t0 = taps_of(y_lo_n, y, Ky, Hs);
        int r0 = t0.lo, r1 = t0.lo + t0.n, ye = y + 1;
        while (ye < y_end) {
            const Taps tn = taps_of(y_lo_n, ye, Ky, Hs);
            const int n0 = min(r0, tn.lo), n1 = max(r1, tn.lo + tn.n);
            if (n1 - n0 > FIT_RMAX) break;
            r0 = n0;
            r1 = n1;
            ++ye;
        }
        __syncthreads();              // the tables are in LDS; the previous chunk's readers are done with the stage

        // horizontal pass: a lane keeps its column, a wave is one staged row (its lanes read neighbouring 12-byte pixels, all three
        // channels each), the four waves take rows rq, rq + 4, ...; four rows go through the tap loop together, so four
        // independent loads are in flight per tap.  Rows past the chunk are clamped to its last row for the loads and not stored
        const int rows = r1 - r0;
        const int c = tid % FIT_TW, rq = tid / FIT_TW;
        const int lo = xlo_s[c], n = xn_s[c];
        for (int jb = 0; rq + 4 * jb < rows; jb += 4) {
            const float* p[4];
            float acc[4][3];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                p[u] = frame + ((int64_t)(r0 + min(rq + 4 * (jb + u), rows - 1)) * Ws + lo) * 3;
                acc[u][0] = acc[u][1] = acc[u][2] = 0.0f;
            }
            for (int k = 0; k < n; ++k) {
                const float w = xw_s[k][c];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float v0 = p[u][3 * k], v1 = p[u][3 * k + 1], v2 = p[u][3 * k + 2];
                    acc[u][0] = fmaf(w, v0, acc[u][0]);
                    acc[u][1] = fmaf(w, v1, acc[u][1]);
                    acc[u][2] = fmaf(w, v2, acc[u][2]);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int r = rq + 4 * (jb + u);
                if (r < rows) {
                    stage[r][0][c] = acc[u][0];
                    stage[r][1][c] = acc[u][1];
                    stage[r][2][c] = acc[u][2];
                }
            }
        }
        __syncthreads();

        // vertical pass: item = (output row, channel, group of 8 columns)
        const int groups = cols >> 3;
        for (int i = tid; i < (ye - y) * 3 * groups; i += FIT_THREADS) {
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

extern "C" int drn_fit_frames(const float* src, void* dst_bf16, int B, int Ts, int Hs, int Ws, int Td, int Hd, int Wd,
                              const int* t_idx, const int* y_lo_n, const float* y_w, int Ky,
                              const int* x_lo_n, const float* x_w, int Kx, void* stream) {
    DRN_CHECK_ARG(src && dst_bf16 && t_idx && y_lo_n && y_w && x_lo_n && x_w);
    DRN_CHECK_ARG(B >= 1 && Ts >= 1 && Hs >= 1 && Ws >= 1 && Td >= 1 && Hd >= 1 && Wd >= 1);
    DRN_CHECK_ARG(Ky >= 1 && Ky <= FIT_KMAX && Kx >= 1 && Kx <= FIT_KMAX);
    DRN_CHECK_ARG(Hd % 16 == 0 && Wd % 16 == 0);
    const int64_t lim = (int64_t)1 << 31;
    DRN_CHECK_ARG((int64_t)B * 3 * Td * Hd * Wd < lim && (int64_t)B * Ts * Hs * Ws * 3 < lim);
    DRN_CHECK_ARG((((uintptr_t)src | (uintptr_t)y_w | (uintptr_t)x_w | (uintptr_t)t_idx | (uintptr_t)y_lo_n |
                    (uintptr_t)x_lo_n) & 3) == 0);
    DRN_CHECK_ARG(((uintptr_t)dst_bf16 & 15) == 0);
    const int tile_h = resample_tile_rows(Ky, FIT_RMAX, 16);
    const int tiles_x = (Wd + FIT_TW - 1) / FIT_TW, tiles_y = (Hd + tile_h - 1) / tile_h;
    const int64_t blocks = (int64_t)tiles_x * tiles_y * Td * B;          // <= the output's element count / 128 < 2^31
    fit_frames_kernel<<<dim3((unsigned)blocks), dim3(FIT_THREADS), 0, (hipStream_t)stream>>>(
        src, (bf16_t*)dst_bf16, Ts, Hs, Ws, Td, Hd, Wd, t_idx, y_lo_n, y_w, Ky, x_lo_n, x_w, Kx, tile_h, tiles_x, tiles_y);
    return drn_launch_status();
}
