// The guided way back (drn_restore_guided_u8, include/drn.h; the plan and the torch specification: fit.py, plan_restore_guided /
// restore_frames_guided).  Joint bilateral upsampling (Kopf et al. 2007) of the uint8 result of the post-process, [B,Ts,Hs,Ws,3] at
// the model's size, to uint8 [B,Td,Hd,Wd,3] at the source's size in ONE launch: the spatial tap tables of a widened triangle
// filter, every tap weighted again by how close the full-size source pixel (guide_hi) is to the fitted source (guide_lo) at that
// tap - a 256-entry table of the Gaussian per channel, their product plus a floor -, the sum divided by the sum of the weights,
// round to nearest even, clamp.  All four byte tensors are channel-interleaved at any byte alignment.
//
// The tiling and raw staging are resample_core.h's: a workgroup owns 64 output columns x GR_TH output rows of one frame.  Once
// per tile the column and row taps, the range table (1 KiB) and guide_hi's row pieces go to LDS; the tile's rows are then walked
// in chunks whose source rows fit the raw buffers (every up-scale: one chunk).  Per chunk:
//   stage    the byte span the tile's columns read, of src AND of guide_lo, -> LDS with aligned 4-byte loads (stage_raw).
//   taps     a wave is an output row, a lane an output pixel: Ky x Kx taps, per tap the pixel of guide_lo and of src (each two
//            aligned LDS words and a byte shift), three table reads, fma from 0 in tap order (ky outer, kx inner); one division
//            per channel; the pixel's 3 bytes go to the LDS output tile.  The loops run to Ky and Kx for every lane (scalar
//            loop control): the weights past a row's or a column's own tap count are zeroed in LDS first, and such a tap reads
//            a byte inside the raw buffers.
// After the last chunk:
//   out      a lane owns one ALIGNED 4-byte word of dst, as in restore.hip; the ragged ends of a row segment bytewise.
// A column span too long for a raw buffer, or a raw buffer that cannot hold one output row's source rows (tables no resize
// produces), is read from global memory bytewise.  No scratch, 44 VGPRs; LDS: 20 KiB, static: seven workgroups per CU.
#include "resample_core.h"

namespace {

constexpr int GR_KMAX = 8;                    // taps per axis, at most
constexpr int GR_TH = 16;                     // output rows per workgroup
constexpr int GR_ROW = RC_TW * 3;             // bytes per output tile row
constexpr int GR_RAW = 5120;                  // raw bytes per pass, of src and of guide_lo each
constexpr int GR_SLACK = 8;                   // words behind each: a zero-weight tap reads up to 3 * GR_KMAX bytes past a row's span
constexpr int GR_OPITCH = GR_ROW / 4 + 1;     // words per output tile row: a shifted word reads its neighbour
constexpr int GR_HPITCH = (GR_ROW + 6) & ~3;  // bytes per staged guide_hi row: up to 3 bytes of misalignment in front

__device__ __forceinline__ float to_byte_f(float v) { return __builtin_amdgcn_fmed3f(__builtin_rintf(v), 0.0f, 255.0f); }

// one row of taps of one pixel: ps / pg point at the first tap's pixel of src / guide_lo, w at the column's weights ([tap][column])
template <typename P>
__device__ __forceinline__ void guided_row(P ps, P pg, const float* w, int n, float wy, int G0, int G1, int G2, const float* tab,
                                           float eps, float* num, float& den) {
    for (int k = 0; k < n; ++k) {
        const int d0 = abs(G0 - (int)pg[3 * k]), d1 = abs(G1 - (int)pg[3 * k + 1]), d2 = abs(G2 - (int)pg[3 * k + 2]);
        const float r = tab[d0] * tab[d1] * tab[d2] + eps;
        const float wt = (wy * w[k * RC_TW]) * r;
        num[0] = fmaf(wt, (float)ps[3 * k], num[0]);
        num[1] = fmaf(wt, (float)ps[3 * k + 1], num[1]);
        num[2] = fmaf(wt, (float)ps[3 * k + 2], num[2]);
        den += wt;
    }
}

// the 3 bytes of the pixel at byte `a` of an LDS image (and the byte behind them): two ALIGNED words and a byte shift - a 2-byte
// LDS read at an odd address that crosses a word is many times slower than the two aligned reads (profiles/restore_guided.txt)
__device__ __forceinline__ uint32_t pixel_at(const uint32_t* words, int a) {
    return __builtin_amdgcn_alignbyte(words[(a >> 2) + 1], words[a >> 2], (uint32_t)a & 3);
}

// guided_row on the raw buffers: as / ag are the byte places of the first tap's pixel in them
__device__ __forceinline__ void guided_row_lds(const uint32_t* src_w, const uint32_t* gl_w, int as, int ag, const float* w, int n,
                                               float wy, int G0, int G1, int G2, const float* tab, float eps, float* num, float& den) {
    for (int k = 0; k < n; ++k) {
        const uint32_t g = pixel_at(gl_w, ag + 3 * k), v = pixel_at(src_w, as + 3 * k);
        // |G_c - g_c| of one byte each: v_sad_u8 with the other three bytes 0 on both sides
        const uint32_t d0 = __builtin_amdgcn_sad_u8(g & 255, G0, 0), d1 = __builtin_amdgcn_sad_u8(g >> 8 & 255, G1, 0),
                       d2 = __builtin_amdgcn_sad_u8(g >> 16 & 255, G2, 0);
        const float r = tab[d0] * tab[d1] * tab[d2] + eps;
        const float wt = (wy * w[k * RC_TW]) * r;
        num[0] = fmaf(wt, (float)(v & 255), num[0]);
        num[1] = fmaf(wt, (float)(v >> 8 & 255), num[1]);
        num[2] = fmaf(wt, (float)(v >> 16 & 255), num[2]);
        den += wt;
    }
}

__global__ void __launch_bounds__(RC_THREADS) restore_guided_kernel(
    const uint8_t* __restrict__ src, const uint8_t* __restrict__ guide_lo, const uint8_t* __restrict__ guide_hi,
    uint8_t* __restrict__ dst, int Bg, int Ts, int Hs, int Ws, int Tg, int t0, int Td, int Hd, int Wd,
    const int* __restrict__ y_lo_n, const float* __restrict__ y_w, int Ky,
    const int* __restrict__ x_lo_n, const float* __restrict__ x_w, int Kx, const float* __restrict__ range_tab, float eps,
    int tiles_x, int tiles_y) {
    __shared__ __attribute__((aligned(16))) uint32_t raw_src[GR_RAW / 4 + GR_SLACK], raw_gl[GR_RAW / 4 + GR_SLACK];
    __shared__ __attribute__((aligned(16))) uint32_t hi_s[GR_TH * GR_HPITCH / 4 + 1], out_s[GR_TH * GR_OPITCH];
    __shared__ float tab_s[256], xw_s[GR_KMAX * RC_TW], yw_s[GR_TH * GR_KMAX];
    __shared__ int xlo_s[RC_TW], xn_s[RC_TW], ylo_s[GR_TH], yn_s[GR_TH], span_s[4];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Tile tl = tile_of_block(tiles_x, tiles_y, GR_TH, Td, Hd, Wd);       // cols: 1..64
    const int y_begin = tl.y_begin, y_end = tl.y_end, rows_out = y_end - y_begin;
    const int bg = Bg == 1 ? 0 : tl.b;
    const uint8_t* frame = src + ((int64_t)tl.b * Ts + tl.t) * Hs * Ws * 3;
    const uint8_t* lo_frame = guide_lo + ((int64_t)bg * Tg + t0 + tl.t) * Hs * Ws * 3;
    const uint8_t* hi_frame = guide_hi + ((int64_t)bg * Tg + t0 + tl.t) * Hd * Wd * 3;
    uint8_t* oframe = dst + ((int64_t)tl.b * Td + tl.t) * Hd * Wd * 3;
    const int L = tl.cols * 3;

    // the tile's taps, the range table and guide_hi's row pieces -> LDS
    if (tid == 0) {
        span_s[0] = Ws;
        span_s[1] = 0;
        span_s[2] = Hs;
        span_s[3] = 0;
    }
    __syncthreads();
    stage_column_taps(x_lo_n, x_w, Kx, Ws, tl, xlo_s, xn_s, xw_s, span_s);
    if (tid >= RC_TW && tid - RC_TW < rows_out) {
        const Taps tp = taps_of(y_lo_n, y_begin + tid - RC_TW, Ky, Hs);
        ylo_s[tid - RC_TW] = tp.lo;
        yn_s[tid - RC_TW] = tp.n;
        atomicMin(&span_s[2], tp.lo);
        atomicMax(&span_s[3], tp.lo + tp.n);
    }
    for (int i = tid; i < rows_out * Ky; i += RC_THREADS) yw_s[i] = y_w[(int64_t)y_begin * Ky + i];
    tab_s[tid] = range_tab[tid];                                // RC_THREADS == 256 entries
    const uint8_t* hi0 = hi_frame + ((int64_t)y_begin * Wd + tl.x_base) * 3;
    const RowSpan hsp = {0, L, GR_HPITCH, GR_TH};
    stage_raw(hi0, Wd * 3, rows_out, hsp, hi_s);
    __syncthreads();
    // weights past a row's or a column's n -> 0, whatever the tables hold there: the tap loops below run to Ky and Kx
    for (int i = tid; i < Kx * RC_TW; i += RC_THREADS)
        if (i / RC_TW >= xn_s[i % RC_TW]) xw_s[i] = 0.0f;
    for (int i = tid; i < rows_out * Ky; i += RC_THREADS)
        if (i % Ky >= yn_s[i / Ky]) yw_s[i] = 0.0f;
    __syncthreads();
    const RowSpan sp = row_span(span_s, GR_RAW);
    const bool staged = sp.rg >= min(Ky, Hs);                   // one output row's source rows fit a raw buffer
    const bool one_chunk = span_s[3] - span_s[2] <= sp.rg;
    const int lo = xlo_s[lane], n = xn_s[lane];
    const int row_b = Ws * 3, col = lo * 3 - sp.s0;             // (a frame has less than 2^31 bytes: int offsets inside it)
    const int fm = (int)((uintptr_t)frame & 3), lm = (int)((uintptr_t)lo_frame & 3);
    const bool live = lane < tl.cols;
    uint8_t* out_b = reinterpret_cast<uint8_t*>(out_s);

    int y = y_begin;
    while (y < y_end) {
        Chunk ch = {0, 0, y_end};
        if (staged) {
            ch = Chunk{span_s[2], span_s[3], y_end};
            if (!one_chunk) ch = cut_chunk(y, y_end, sp.rg, [&](int i) { return Taps{ylo_s[i - y_begin], yn_s[i - y_begin]}; });
            __syncthreads();          // the previous chunk's readers are done with the raw buffers
            stage_raw(frame + (int64_t)ch.r0 * Ws * 3 + sp.s0, Ws * 3, ch.r1 - ch.r0, sp, raw_src);
            stage_raw(lo_frame + (int64_t)ch.r0 * Ws * 3 + sp.s0, Ws * 3, ch.r1 - ch.r0, sp, raw_gl);
            __syncthreads();
        }
        for (int row = wave; row < ch.ye - y; row += RC_WAVES) {
            if (!live) continue;
            const int yt = y - y_begin + row;
            const int vlo = __builtin_amdgcn_readfirstlane(ylo_s[yt]), vn = __builtin_amdgcn_readfirstlane(yn_s[yt]);
            const uint32_t G = pixel_at(hi_s, yt * GR_HPITCH + (int)((uintptr_t)(hi0 + (int64_t)yt * Wd * 3) & 3) + 3 * lane);
            const int G0 = G & 255, G1 = G >> 8 & 255, G2 = G >> 16 & 255;
            float num[3] = {0.0f, 0.0f, 0.0f}, den = 0.0f;
            if (staged) {
                // every lane walks Ky x Kx taps: those past its n weigh 0 and read a byte that lies inside the raw buffers (rows
                // are held inside the row's own taps, columns run at most 3 * (Kx - 1) bytes past the span: GR_SLACK)
                for (int k = 0; k < Ky; ++k) {
                    const float wy = yw_s[yt * Ky + k];
                    const int r = vlo + min(k, vn - 1);
                    const int roff = r * row_b + sp.s0;                             // the row's span in the frame
                    const int at = (r - ch.r0) * sp.pitch + col;
                    guided_row_lds(raw_src, raw_gl, at + ((fm + roff) & 3), at + ((lm + roff) & 3), xw_s + lane, Kx, wy, G0, G1, G2,
                                   tab_s, eps, num, den);
                }
            } else {
                for (int k = 0; k < vn; ++k) {
                    const int64_t goff = ((int64_t)(vlo + k) * Ws + lo) * 3;        // the first tap's pixel in the frame
                    guided_row(frame + goff, lo_frame + goff, xw_s + lane, n, yw_s[yt * Ky + k], G0, G1, G2, tab_s, eps, num, den);
                }
            }
            uint8_t* ob = out_b + yt * GR_OPITCH * 4 + 3 * lane;
            ob[0] = (uint8_t)to_byte_f(num[0] / den);
            ob[1] = (uint8_t)to_byte_f(num[1] / den);
            ob[2] = (uint8_t)to_byte_f(num[2] / den);
        }
        y = ch.ye;
    }
    __syncthreads();

    // out: a wave is an output row, a lane an aligned word of dst; segment byte s of the row is byte s of the tile row
    for (int row = wave; row < rows_out; row += RC_WAVES) {
        const uint32_t* orow = out_s + row * GR_OPITCH;
        uint8_t* o = oframe + ((int64_t)(y_begin + row) * Wd + tl.x_base) * 3;
        const int m = (int)((uintptr_t)o & 3);
        const int s = 4 * lane - m;
        if (s >= L) continue;
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
}

}  // namespace

extern "C" int drn_restore_guided_u8(const uint8_t* src, const uint8_t* guide_lo, const uint8_t* guide_hi, uint8_t* dst,
                                     int B, int Bg, int Ts, int Hs, int Ws, int Tg, int t0, int Td, int Hd, int Wd,
                                     const int* y_lo_n, const float* y_w, int Ky, const int* x_lo_n, const float* x_w, int Kx,
                                     const float* range_tab, float eps, void* stream) {
    DRN_CHECK_ARG(src && guide_lo && guide_hi && dst && y_lo_n && y_w && x_lo_n && x_w && range_tab);
    DRN_CHECK_ARG(B >= 1 && Bg >= 1 && Ts >= 1 && Hs >= 1 && Ws >= 1 && Tg >= 1 && Td >= 1 && Hd >= 1 && Wd >= 1);
    DRN_CHECK_ARG(Bg == 1 || Bg == B);
    DRN_CHECK_ARG(Td <= Ts && t0 >= 0 && (int64_t)t0 + Td <= Tg);
    DRN_CHECK_ARG(Ky >= 1 && Ky <= GR_KMAX && Kx >= 1 && Kx <= GR_KMAX);
    const int64_t lim = (int64_t)1 << 31;
    // (factor by factor: four ints of up to 2^31 - 1 would overflow an int64 product)
    auto bytes_fit = [lim](int64_t a, int64_t b, int64_t c, int64_t d) {
        int64_t n = 3;
        for (int64_t f : {a, b, c, d}) {
            n *= f;
            if (n >= lim) return false;
        }
        return true;
    };
    DRN_CHECK_ARG(bytes_fit(B, Ts, Hs, Ws) && bytes_fit(Bg, Tg, Hs, Ws) && bytes_fit(Bg, Tg, Hd, Wd) && bytes_fit(B, Td, Hd, Wd));
    DRN_CHECK_ARG((((uintptr_t)y_w | (uintptr_t)x_w | (uintptr_t)y_lo_n | (uintptr_t)x_lo_n | (uintptr_t)range_tab) & 3) == 0);
    DRN_CHECK_ARG(eps > 0.0f);                                  // (a NaN fails too)
    const int tiles_x = (Wd + RC_TW - 1) / RC_TW, tiles_y = (Hd + GR_TH - 1) / GR_TH;
    const int64_t blocks = (int64_t)tiles_x * tiles_y * Td * B;              // <= the output's pixel count < 2^31
    restore_guided_kernel<<<dim3((unsigned)blocks), dim3(RC_THREADS), 0, (hipStream_t)stream>>>(
        src, guide_lo, guide_hi, dst, Bg, Ts, Hs, Ws, Tg, t0, Td, Hd, Wd, y_lo_n, y_w, Ky, x_lo_n, x_w, Kx, range_tab, eps,
        tiles_x, tiles_y);
    return drn_launch_status();
}
