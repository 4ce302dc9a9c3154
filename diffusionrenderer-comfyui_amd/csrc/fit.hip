// Clip ingest with a fit to the model's grid (drn_fit_frames, drn_fit_frames_u8, include/drn.h; the plan and the torch
// specification: fit.py).  ComfyUI frames [B,Ts,Hs,Ws,3], fp32 in [0, 1] or uint8 at ANY byte alignment, -> [B,3,Td,Hd,Wd] bf16
// in [-1, 1] in ONE launch: separable resampling by per-axis tap tables (the antialiased triangle filter, crop offsets folded into
// the tables), frame gather (time padding), * 2 - 1, round to nearest even, transpose.  drn_fit_frames_u8 is drn_fit_frames on
// the frames unit[src], unit[i] = fp32(i) / 255 correctly rounded, bit for bit.
//
// One kernel over the source's element type, on the tiling, chunks and raw staging of resample_core.h; the stage is planar per
// channel (64 consecutive floats per row and channel).  Per chunk:
//   horiz    a wave is a staged source row, a lane an output column.  fp32: the lane reads whole 12-byte pixels from global
//            memory, neighbouring lanes neighbouring pixels.  uint8: out of the raw bytes (hpass_bytes), every byte through the
//            256-entry table unit_s (filled once per workgroup with one correctly rounded division per thread: multiplying by
//            1.0f / 255 differs from the division at 126 byte values).  fma from 0 in tap order.
//   vert     a lane filters 8 consecutive output columns of one row and channel out of the stage (two 16-byte LDS reads per tap)
//            and stores them as one 16-byte group.
// Every loop runs over a row's own tap count.  A single tap of weight 1.0 passes its source value through both passes unchanged
// (fma(1, v, 0) == v): scale 1 is a bit-exact copy.
#include <type_traits>

#include "resample_core.h"

namespace {

constexpr int FIT_RMAX = 48;      // staged source rows: 48 x 3 x 64 fp32 = 36 KiB
constexpr int FIT_RAW = 6144;     // raw source bytes per pass: 16 rows of a 64-column tile at 1080p -> 576 x 1024 (372 bytes each)
// LDS: stage 36 KiB + column weights 8 KiB + taps 0.5 KiB = 44.5 KiB; uint8 adds raw 6 KiB + unit 1 KiB = 51.5 KiB: three
// workgroups per CU either way

template <typename T>
__global__ void __launch_bounds__(RC_THREADS) fit_frames_kernel(
    const T* __restrict__ src, bf16_t* __restrict__ dst, int Ts, int Hs, int Ws, int Td, int Hd, int Wd,
    const int* __restrict__ t_idx, const int* __restrict__ y_lo_n, const float* __restrict__ y_w, int Ky,
    const int* __restrict__ x_lo_n, const float* __restrict__ x_w, int Kx, int tile_h, int tiles_x, int tiles_y) {
    constexpr bool U8 = std::is_same_v<T, uint8_t>;
    __shared__ __attribute__((aligned(16))) float stage[FIT_RMAX][3][RC_TW];
    __shared__ float xw_s[RC_KMAX][RC_TW];
    __shared__ int xlo_s[RC_TW], xn_s[RC_TW];
    __shared__ uint32_t raw_s[U8 ? FIT_RAW / 4 : 1];          // uint8 only, like unit_s (RC_THREADS = its 256 entries) and span_s
    __shared__ float unit_s[U8 ? RC_THREADS : 1];
    __shared__ int span_s[2];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Tile tl = tile_of_block(tiles_x, tiles_y, tile_h, Td, Hd, Wd);      // cols: a multiple of 8 (Wd % 16 == 0)
    const int ts = min(max(t_idx[tl.t], 0), Ts - 1);
    const T* frame = src + ((int64_t)tl.b * Ts + ts) * Hs * Ws * 3;
    const auto row_taps = [&](int i) { return taps_of(y_lo_n, i, Ky, Hs); };

    RowSpan sp = {};
    if constexpr (U8) {
        unit_s[tid] = __fdiv_rn((float)tid, 255.0f);
        if (tid == 0) {
            span_s[0] = Ws;
            span_s[1] = 0;
        }
        __syncthreads();
    }
    stage_column_taps(x_lo_n, x_w, Kx, Ws, tl, xlo_s, xn_s, &xw_s[0][0], U8 ? span_s : nullptr);
    if constexpr (U8) {
        __syncthreads();
        sp = row_span(span_s, FIT_RAW);
    }

    int y = tl.y_begin;
    while (y < tl.y_end) {
        const Chunk ch = cut_chunk(y, tl.y_end, FIT_RMAX, row_taps);
        const int r0 = ch.r0, rows = ch.r1 - ch.r0;
        __syncthreads();              // the tables are in LDS; the previous chunk's readers are done with the stage
        const int lo = xlo_s[lane], n = xn_s[lane];             // horizontal pass: a lane keeps its column

        if constexpr (U8) {
            hpass_bytes(frame, Ws, r0, rows, sp, raw_s, &xw_s[0][lane], lo, n, lane < tl.cols,
                        [&](uint8_t v) { return unit_s[v]; },
                        [&](int r, const float* acc) {
                            stage[r][0][lane] = acc[0];
                            stage[r][1][lane] = acc[1];
                            stage[r][2][lane] = acc[2];
                        });
        } else {
            // the four waves take rows wave, wave + 4, ...; four rows go through the tap loop together, so four independent
            // loads are in flight per tap.  Rows past the chunk are clamped to its last row for the loads and not stored
            for (int jb = 0; wave + 4 * jb < rows; jb += 4) {
                const float* p[4];
                float acc[4][3];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    p[u] = frame + ((int64_t)(r0 + min(wave + 4 * (jb + u), rows - 1)) * Ws + lo) * 3;
                    acc[u][0] = acc[u][1] = acc[u][2] = 0.0f;
                }
                for (int k = 0; k < n; ++k) {
                    const float w = xw_s[k][lane];
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
                    const int r = wave + 4 * (jb + u);
                    if (r < rows) {
                        stage[r][0][lane] = acc[u][0];
                        stage[r][1][lane] = acc[u][1];
                        stage[r][2][lane] = acc[u][2];
                    }
                }
            }
            __syncthreads();
        }

        // vertical pass: item = (output row, channel, group of 8 columns)
        const int groups = tl.cols >> 3;
        for (int i = tid; i < (ch.ye - y) * 3 * groups; i += RC_THREADS) {
            const int g = i % groups, c = (i / groups) % 3, yo = y + i / (3 * groups);
            const Taps tv = row_taps(yo);
            const float* wrow = y_w + (int64_t)yo * Ky;
            float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            for (int k = 0; k < tv.n; ++k) {
                const float w = wrow[k];
                const float4* s = reinterpret_cast<const float4*>(&stage[tv.lo - r0 + k][c][g * 8]);
                const float4 a = s[0], c4 = s[1];
                acc[0] = fmaf(w, a.x, acc[0]); acc[1] = fmaf(w, a.y, acc[1]);
                acc[2] = fmaf(w, a.z, acc[2]); acc[3] = fmaf(w, a.w, acc[3]);
                acc[4] = fmaf(w, c4.x, acc[4]); acc[5] = fmaf(w, c4.y, acc[5]);
                acc[6] = fmaf(w, c4.z, acc[6]); acc[7] = fmaf(w, c4.w, acc[7]);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = fmaf(2.0f, acc[j], -1.0f);     // 2 * acc is exact: one rounding, like * 2 - 1
            bf16_t* o = dst + ((((int64_t)tl.b * 3 + c) * Td + tl.t) * Hd + yo) * Wd + tl.x_base + g * 8;
            *reinterpret_cast<uint4*>(o) = pack8(acc);
        }
        y = ch.ye;
    }
}

// src: 4-byte aligned as fp32, at any alignment as bytes
template <typename T>
int fit_launch(const T* src, void* dst_bf16, int B, int Ts, int Hs, int Ws, int Td, int Hd, int Wd, const int* t_idx,
               const int* y_lo_n, const float* y_w, int Ky, const int* x_lo_n, const float* x_w, int Kx, void* stream) {
    DRN_CHECK_ARG(src && dst_bf16 && t_idx && y_lo_n && y_w && x_lo_n && x_w);
    DRN_CHECK_ARG(B >= 1 && Ts >= 1 && Hs >= 1 && Ws >= 1 && Td >= 1 && Hd >= 1 && Wd >= 1);
    DRN_CHECK_ARG(Ky >= 1 && Ky <= RC_KMAX && Kx >= 1 && Kx <= RC_KMAX);
    DRN_CHECK_ARG(Hd % 16 == 0 && Wd % 16 == 0);
    const int64_t lim = (int64_t)1 << 31;
    DRN_CHECK_ARG((int64_t)B * 3 * Td * Hd * Wd < lim && (int64_t)B * Ts * Hs * Ws * 3 < lim);
    DRN_CHECK_ARG((((uintptr_t)y_w | (uintptr_t)x_w | (uintptr_t)t_idx | (uintptr_t)y_lo_n | (uintptr_t)x_lo_n) & 3) == 0);
    DRN_CHECK_ARG(((uintptr_t)src & (sizeof(T) - 1)) == 0);
    DRN_CHECK_ARG(((uintptr_t)dst_bf16 & 15) == 0);
    const int tile_h = resample_tile_rows(Ky, FIT_RMAX, 16);
    const int tiles_x = (Wd + RC_TW - 1) / RC_TW, tiles_y = (Hd + tile_h - 1) / tile_h;
    const int64_t blocks = (int64_t)tiles_x * tiles_y * Td * B;          // <= the output's element count / 128 < 2^31
    fit_frames_kernel<T><<<dim3((unsigned)blocks), dim3(RC_THREADS), 0, (hipStream_t)stream>>>(
        src, (bf16_t*)dst_bf16, Ts, Hs, Ws, Td, Hd, Wd, t_idx, y_lo_n, y_w, Ky, x_lo_n, x_w, Kx, tile_h, tiles_x, tiles_y);
    return drn_launch_status();
}

}  // namespace

extern "C" int drn_fit_frames(const float* src, void* dst_bf16, int B, int Ts, int Hs, int Ws, int Td, int Hd, int Wd,
                              const int* t_idx, const int* y_lo_n, const float* y_w, int Ky,
                              const int* x_lo_n, const float* x_w, int Kx, void* stream) {
    return fit_launch(src, dst_bf16, B, Ts, Hs, Ws, Td, Hd, Wd, t_idx, y_lo_n, y_w, Ky, x_lo_n, x_w, Kx, stream);
}

extern "C" int drn_fit_frames_u8(const uint8_t* src, void* dst_bf16, int B, int Ts, int Hs, int Ws, int Td, int Hd, int Wd,
                                 const int* t_idx, const int* y_lo_n, const float* y_w, int Ky,
                                 const int* x_lo_n, const float* x_w, int Kx, void* stream) {
    return fit_launch(src, dst_bf16, B, Ts, Hs, Ws, Td, Hd, Wd, t_idx, y_lo_n, y_w, Ky, x_lo_n, x_w, Kx, stream);
}
