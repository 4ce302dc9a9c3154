// The resampling core of fit.hip (drn_fit_frames, drn_fit_frames_u8) and restore.hip (drn_restore_frames_u8): separable
// resampling by per-axis tap tables.  A workgroup of RC_THREADS owns RC_TW output columns x `tile_h` output rows of one frame.
//
// Chunks.  The workgroup walks its rows in chunks whose source rows fit its fp32 LDS stage: a chunk is as many output rows from y
// on as the union [r0, r1) of their source rows holds at most `rmax` rows (cut_chunk; one row always fits: n <= K <= rmax).  The
// chunk's source rows are filtered horizontally into the stage, then its output rows vertically out of it.
//
// Raw bytes.  A byte pixel is 3 bytes at any alignment, so the byte kernels read no tap from global memory.  The bytes the tile's
// columns read, byte span [3 * min lo, 3 * max(lo + n)) of a source row (RowSpan), are copied into LDS, as many rows per pass as
// fit the raw buffer, with ALIGNED 4-byte loads (a lane a word); the up to 3 bytes in front of the first whole word and behind
// the last are copied bytewise, so nothing outside the span - and nothing outside the source - is read (stage_raw).  A row's
// image sits at its own byte misalignment, word for word.  A span too long for the raw buffer (tables no antialiased resize
// produces) is read from global memory bytewise (hpass_bytes).
//
// lo and n are clamped into the source before use (taps_of), so no table content can take a read outside the source, the raw
// buffer or the stage.
#pragma once
#include "drn_common.h"

constexpr int RC_TW = 64;             // output columns per workgroup
constexpr int RC_KMAX = 32;           // taps per axis, at most
constexpr int RC_THREADS = 256;
constexpr int RC_WAVES = RC_THREADS / 64;

struct Taps {
    int lo, n;
};

// a row of a table, forced into [0, n_in): n in 1..K, lo in 0..n_in - n (valid tables pass unchanged; n_in >= 1)
__device__ __forceinline__ Taps taps_of(const int* __restrict__ lo_n, int i, int K, int n_in) {
    Taps t;
    t.n = min(max(lo_n[2 * i + 1], 1), min(K, n_in));
    t.lo = min(max(lo_n[2 * i], 0), n_in - t.n);
    return t;
}

// rows per workgroup: what a down-scale of about (K - 1) / 2 source rows per output row lets into a stage of `stage_rows` source
// rows, `cap` at most.  A hint only: the kernels cut their rows into chunks that fit, whatever the tables hold
inline int resample_tile_rows(int K, int stage_rows, int cap) {
    const double step = K > 3 ? 0.5 * (K - 1) : 1.0;
    const int tile_h = (int)((stage_rows - K) / step) + 1;
    return tile_h < 1 ? 1 : (tile_h > cap ? cap : tile_h);
}

// the workgroup's tile: output columns [x_base, x_base + cols), rows [y_begin, y_end) of frame t of clip b
struct Tile {
    int x_base, cols, y_begin, y_end, t, b;
};

__device__ __forceinline__ Tile tile_of_block(int tiles_x, int tiles_y, int tile_h, int Td, int Hd, int Wd) {
    int blk = blockIdx.x;
    Tile tl;
    tl.x_base = blk % tiles_x * RC_TW;
    blk /= tiles_x;
    tl.y_begin = blk % tiles_y * tile_h;
    blk /= tiles_y;
    tl.t = blk % Td;
    tl.b = blk / Td;
    tl.cols = min(RC_TW, Wd - tl.x_base);
    tl.y_end = min(tl.y_begin + tile_h, Hd);
    return tl;
}

// the tile's column taps -> LDS: xw_s is [tap][column], lanes walk columns, conflict-free.  Columns past the picture get one tap
// of weight 0 at source column 0 and are never stored.  With span_s (preset to {Ws, 0} behind a barrier) the source columns the
// tile reads, [span_s[0], span_s[1]), are recorded.  The caller's barrier follows
__device__ __forceinline__ void stage_column_taps(const int* __restrict__ x_lo_n, const float* __restrict__ x_w, int Kx, int Ws,
                                                  const Tile& tl, int* xlo_s, int* xn_s, float* xw_s, int* span_s) {
    const int tid = threadIdx.x;
    if (tid < RC_TW) {
        Taps tp = {0, 1};
        if (tid < tl.cols) {
            tp = taps_of(x_lo_n, tl.x_base + tid, Kx, Ws);
            if (span_s) {
                atomicMin(&span_s[0], tp.lo);
                atomicMax(&span_s[1], tp.lo + tp.n);
            }
        }
        xlo_s[tid] = tp.lo;
        xn_s[tid] = tp.n;
    }
    for (int i = tid; i < Kx * RC_TW; i += RC_THREADS) {
        const int c = i % RC_TW, k = i / RC_TW;
        xw_s[i] = c < tl.cols ? x_w[(int64_t)(tl.x_base + c) * Kx + k] : 0.0f;
    }
}

// output rows [y, ye) and the source rows [r0, r1) they read
struct Chunk {
    int r0, r1, ye;
};

// the chunk that starts at output row y; taps(i): the (clamped) row taps of output row i
template <typename F>
__device__ __forceinline__ Chunk cut_chunk(int y, int y_end, int rmax, F taps) {
    const Taps t0 = taps(y);
    Chunk c = {t0.lo, t0.lo + t0.n, y + 1};
    while (c.ye < y_end) {
        const Taps tn = taps(c.ye);
        const int n0 = min(c.r0, tn.lo), n1 = max(c.r1, tn.lo + tn.n);
        if (n1 - n0 > rmax) break;
        c.r0 = n0;
        c.r1 = n1;
        ++c.ye;
    }
    return c;
}

// the bytes [s0, s0 + span) of a source row that the tile's columns read (3 <= span <= Ws * 3), and their image in the raw buffer
struct RowSpan {
    int s0, span;
    int pitch;      // bytes per row image, a multiple of 4: up to 3 bytes of misalignment in front
    int rg;         // source rows per raw pass; 0: the span does not fit, read directly
};

__device__ __forceinline__ RowSpan row_span(const int* span_s, int raw_bytes) {
    RowSpan sp;
    sp.s0 = span_s[0] * 3;
    sp.span = span_s[1] * 3 - sp.s0;
    sp.pitch = (sp.span + 6) & ~3;
    sp.rg = raw_bytes / sp.pitch;
    return sp;
}

// `grows` row spans, the first at g, `row_bytes` apart -> raw_s: word j of row rr holds span bytes [4j - mm, 4j - mm + 4), mm the
// row's byte misalignment in global memory.  Four words per thread are loaded before any is stored: their latencies overlap
__device__ __forceinline__ void stage_raw(const uint8_t* __restrict__ g0, int row_bytes, int grows, const RowSpan& sp,
                                          uint32_t* raw_s) {
    const int pw = sp.pitch >> 2;
    for (int base = threadIdx.x; base < grows * pw; base += 4 * RC_THREADS) {
        uint32_t v[4] = {0, 0, 0, 0};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = base + u * RC_THREADS;
            if (i >= grows * pw) continue;
            const int rr = i / pw, j = i - rr * pw;
            const uint8_t* g = g0 + (int64_t)rr * row_bytes;
            const int s = 4 * j - (int)((uintptr_t)g & 3);
            if (s >= 0 && s + 4 <= sp.span) {
                v[u] = *reinterpret_cast<const uint32_t*>(g + s);
            } else {
                for (int k = 0; k < 4; ++k)
                    if (s + k >= 0 && s + k < sp.span) v[u] |= (uint32_t)g[s + k] << (8 * k);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (base + u * RC_THREADS < grows * pw) raw_s[base + u * RC_THREADS] = v[u];
    }
}

// one output column of one source row: p points at the first tap's pixel, w at the column's weights ([tap][column] in LDS);
// fma from 0 in tap order
template <typename P, typename Cvt>
__device__ __forceinline__ void hfilter_bytes(P p, const float* w, int n, Cvt to_float, float* acc) {
    for (int k = 0; k < n; ++k) {
        const float wk = w[k * RC_TW];
        acc[0] = fmaf(wk, to_float(p[3 * k]), acc[0]);
        acc[1] = fmaf(wk, to_float(p[3 * k + 1]), acc[1]);
        acc[2] = fmaf(wk, to_float(p[3 * k + 2]), acc[2]);
    }
}

// the horizontal pass of a chunk of byte rows [r0, r0 + rows) of `frame`: a wave is a source row, a lane (column taps lo, n,
// weights w) an output column; store(r, acc) puts the lane's pixel into stage row r.  Lanes that are not `live` (columns past
// the picture) store 0.  Returns behind a barrier: the stage is written, the raw buffer free
template <typename Cvt, typename Store>
__device__ __forceinline__ void hpass_bytes(const uint8_t* __restrict__ frame, int Ws, int r0, int rows, const RowSpan& sp,
                                            uint32_t* raw_s, const float* w, int lo, int n, bool live, Cvt to_float, Store store) {
    const int wave = threadIdx.x >> 6;
    if (sp.rg == 0) {
        for (int r = wave; r < rows; r += RC_WAVES) {
            float acc[3] = {0.0f, 0.0f, 0.0f};
            if (live) hfilter_bytes(frame + ((int64_t)(r0 + r) * Ws + lo) * 3, w, n, to_float, acc);
            store(r, acc);
        }
        __syncthreads();
        return;
    }
    const uint8_t* raw_b = reinterpret_cast<const uint8_t*>(raw_s);
    for (int g0 = 0; g0 < rows; g0 += sp.rg) {
        const int grows = min(sp.rg, rows - g0);
        const uint8_t* g = frame + (int64_t)(r0 + g0) * Ws * 3 + sp.s0;
        stage_raw(g, Ws * 3, grows, sp, raw_s);
        __syncthreads();
        for (int rr = wave; rr < grows; rr += RC_WAVES) {
            const int mm = (int)((uintptr_t)(g + (int64_t)rr * Ws * 3) & 3);
            float acc[3] = {0.0f, 0.0f, 0.0f};
            if (live) hfilter_bytes(raw_b + rr * sp.pitch + mm + lo * 3 - sp.s0, w, n, to_float, acc);
            store(g0 + rr, acc);
        }
        __syncthreads();      // the stage rows are written; the raw buffer is free for the next rows
    }
}
