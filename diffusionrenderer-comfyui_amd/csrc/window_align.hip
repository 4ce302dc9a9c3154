// Windows that agree (windows.py): a window of a long clip is matched in gain and offset to the previous window's
// carry over the frames both describe, before the cross-fade of diffusion_renderer_pipeline.py `_walk` joins them.
//   drn_window_align_affine          the first two moments of both versions of the overlap -> one (g, o) per pass, on the device
//   drn_postprocess_window_align_u8  drn_postprocess_window_u8 (elementwise.hip) with that affine applied to every window value
//                                    it reads, and the aligned last O frames written out as the next carry in the same launch
// The apply is a bit-exact restatement of unfused torch fp32 ops (mul, then add), so contraction is off in this file.
#pragma clang fp contract(off)
#include "drn_common.h"
#include <math.h>

// ------------------------------------------------------------------------------------------------
// moments of the overlap, store-and-sum: no atomics, every sum taken in one fixed order, so the result is the same bits run to run.
// Per pass b and channel ch the overlap is ONE contiguous run of L = O * H * W values in the window (frames [ramp_at, ramp_at + O)
// of plane (b, ch)) and in the carry.  Stage one: block (x, b) reduces chunk x % nc of channel x / nc, ALIGN_CHUNK values of that
// run, to five fp64 partials (sum a, sum v, sum a^2, sum v^2, sum a v); products of two bf16 values are exact in fp32.  Stage two:
// one wave per pass adds the 3 * nc partials of each sum in index order - 64 contiguous runs, one per lane, then the runs in lane
// order - and evaluates the rules of windows.align_affine in fp64.
#define ALIGN_CHUNK 8192           // values per block: 256 lanes x 8 values x 4 trips
#define ALIGN_SUMS 5

static inline int64_t align_chunks(int64_t L) { return (L + ALIGN_CHUNK - 1) / ALIGN_CHUNK; }

__device__ __forceinline__ void align_accumulate(float a, float v, double (&s)[ALIGN_SUMS]) {
    s[0] += (double)a;
    s[1] += (double)v;
    s[2] += (double)(a * a);
    s[3] += (double)(v * v);
    s[4] += (double)(a * v);
}

template <bool VEC>
__global__ __launch_bounds__(256) void window_align_partials_kernel(const bf16_t* __restrict__ v, const bf16_t* __restrict__ prev,
                                                                    double* __restrict__ part, int nc, int Tw, int64_t hw, int O,
                                                                    int ramp_at) {
    const int b = blockIdx.y, ch = blockIdx.x / nc, k = blockIdx.x - ch * nc;
    const int64_t L = (int64_t)O * hw;
    const int64_t lo = (int64_t)k * ALIGN_CHUNK, hi = lo + ALIGN_CHUNK < L ? lo + ALIGN_CHUNK : L;
    const bf16_t* vb = v + (((int64_t)b * 3 + ch) * Tw + ramp_at) * hw;
    const bf16_t* pb = prev + ((int64_t)b * 3 + ch) * L;
    double s[ALIGN_SUMS] = {0., 0., 0., 0., 0.};
    if (VEC) {                                                       // L % 8 == 0: a chunk is whole groups of 8
        for (int64_t i = lo + (int64_t)threadIdx.x * 8; i < hi; i += 256 * 8) {
            float a[8], x[8];
            unpack8(ld16_nt(pb + i), a);
            unpack8(ld16_nt(vb + i), x);
#pragma unroll
            for (int e = 0; e < 8; ++e) align_accumulate(a[e], x[e], s);
        }
    } else {
        for (int64_t i = lo + threadIdx.x; i < hi; i += 256) align_accumulate(bf2f(pb[i]), bf2f(vb[i]), s);
    }
    // the wave's butterfly, then the block's four waves in order
    __shared__ double lds[4][ALIGN_SUMS];
#pragma unroll
    for (int q = 0; q < ALIGN_SUMS; ++q) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) s[q] += __shfl_xor(s[q], d, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < ALIGN_SUMS; ++q) lds[wave][q] = s[q];
    }
    __syncthreads();
    if (threadIdx.x < ALIGN_SUMS) {
        const int q = threadIdx.x;
        part[((int64_t)b * gridDim.x + blockIdx.x) * ALIGN_SUMS + q] = ((lds[0][q] + lds[1][q]) + lds[2][q]) + lds[3][q];
    }
}

__global__ __launch_bounds__(64) void window_align_solve_kernel(const double* __restrict__ part, float* __restrict__ affine,
                                                                double* __restrict__ moments, int nparts, double n) {
    const int b = blockIdx.x;
    __shared__ double runs[ALIGN_SUMS][64];
    __shared__ double sums[ALIGN_SUMS];
    const double* p = part + (int64_t)b * nparts * ALIGN_SUMS;
    const int seg = (nparts + 63) / 64, lo = threadIdx.x * seg, hi = lo + seg < nparts ? lo + seg : nparts;
#pragma unroll
    for (int q = 0; q < ALIGN_SUMS; ++q) {
        double s = 0.;
        for (int i = lo; i < hi; ++i) s += p[(int64_t)i * ALIGN_SUMS + q];
        runs[q][threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x < ALIGN_SUMS) {
        double s = 0.;
        for (int l = 0; l < 64; ++l) s += runs[threadIdx.x][l];
        sums[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double mean_a = sums[0] / n, mean_v = sums[1] / n;
    const double var_a = sums[2] / n - mean_a * mean_a, var_v = sums[3] / n - mean_v * mean_v;
    const double cov = sums[4] / n - mean_a * mean_v;
    double g = 1., o = 0.;
    if (isfinite(mean_a) && isfinite(mean_v) && isfinite(var_a) && isfinite(var_v) && isfinite(cov)) {
        const double flat = 9.5367431640625e-07;                     // 2^-20: a standard deviation under a quarter of a byte level
        if (var_a >= flat && var_v >= flat && cov > 0.) g = sqrt(var_a / var_v);
        g = fmin(fmax(g, 0.5), 2.);
        o = mean_a - g * mean_v;
    }
    affine[2 * b] = (float)g;
    affine[2 * b + 1] = (float)o;
    if (moments) {
        double* m = moments + 6 * (int64_t)b;
        m[0] = n; m[1] = mean_a; m[2] = mean_v; m[3] = var_a; m[4] = var_v; m[5] = cov;
    }
}

extern "C" int64_t drn_window_align_workspace_bytes(int B, int H, int W, int O) {
    if (B < 1 || H < 1 || W < 1 || O < 1) return 0;
    return (int64_t)B * 3 * align_chunks((int64_t)O * H * W) * ALIGN_SUMS * (int64_t)sizeof(double);
}

extern "C" int drn_window_align_affine(const void* video, const void* prev_tail, void* affine, void* moments, void* workspace,
                                       int64_t workspace_bytes, int B, int Tw, int H, int W, int O, int ramp_at, void* stream) {
    DRN_CHECK_ARG(video && prev_tail && affine && workspace);
    DRN_CHECK_ARG(B > 0 && Tw > 0 && H > 0 && W > 0 && O >= 1 && ramp_at >= 0 && (int64_t)ramp_at + O <= Tw);
    DRN_CHECK_ARG(((uintptr_t)video & 1) == 0 && ((uintptr_t)prev_tail & 1) == 0 && ((uintptr_t)affine & 3) == 0 &&
                  ((uintptr_t)moments & 7) == 0 && ((uintptr_t)workspace & 7) == 0);
    DRN_CHECK_ARG(workspace_bytes >= drn_window_align_workspace_bytes(B, H, W, O));
    const int64_t hw = (int64_t)H * W, L = (int64_t)O * hw, nc = align_chunks(L);
    DRN_CHECK_ARG(B <= 65535 && 3 * nc < (1ll << 31));
    const bool vec = hw % 8 == 0 && ((uintptr_t)video & 15) == 0 && ((uintptr_t)prev_tail & 15) == 0;
    const dim3 grid((unsigned)(3 * nc), (unsigned)B);
    if (vec)
        window_align_partials_kernel<true><<<grid, dim3(256), 0, (hipStream_t)stream>>>(
            (const bf16_t*)video, (const bf16_t*)prev_tail, (double*)workspace, (int)nc, Tw, hw, O, ramp_at);
    else
        window_align_partials_kernel<false><<<grid, dim3(256), 0, (hipStream_t)stream>>>(
            (const bf16_t*)video, (const bf16_t*)prev_tail, (double*)workspace, (int)nc, Tw, hw, O, ramp_at);
    DRN_TRY(drn_launch_status());
    window_align_solve_kernel<<<dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream>>>(
        (const double*)workspace, (float*)affine, (double*)moments, (int)(3 * nc), (double)(3 * L));
    return drn_launch_status();
}

// ------------------------------------------------------------------------------------------------
// postprocess_window_kernel (elementwise.hip) with the affine in front and the carry behind.  blockIdx.y strides the
// B * (write_hi - write_lo) written frames and then the B * O carry frames; a block works inside one frame of either kind, so the
// pass (its g and o), "is this a ramp frame" and the ramp weight are uniform.  A carry frame is frame Tw - O + j of the window,
// aligned and NOT cross-faded: the next window is matched to this window's own version of those frames.
__device__ __forceinline__ float align_apply(float x, float g, float o) {
    // torch's (x * g) + o on fp32 tensors: two separately rounded operations, never an FMA (window_blend's rule); then .to(bfloat16)
    const float m = g * x;
    return rbf(m + o);
}

template <bool VEC>
__global__ __launch_bounds__(256) void postprocess_window_align_kernel(const bf16_t* __restrict__ v, const bf16_t* __restrict__ prev,
                                                                       const float* __restrict__ rw, const float* __restrict__ affine,
                                                                       uint8_t* __restrict__ o, bf16_t* __restrict__ carry,
                                                                       int nframes, int ncarry, int nF, int Tw, int64_t hw, int O,
                                                                       int ramp_at, int write_lo, int normalize) {
    const int64_t vcs = (int64_t)Tw * hw, pcs = (int64_t)O * hw;               // channel strides of the window / a carry
    for (int fi = blockIdx.y; fi < nframes + ncarry; fi += gridDim.y) {
        const bool out_frame = fi < nframes;
        int b, f, j;
        if (out_frame) {
            b = fi / nF, f = write_lo + (fi - b * nF), j = f - ramp_at;
        } else {
            b = (fi - nframes) / O, j = (fi - nframes) - b * O, f = Tw - O + j;
        }
        const bool aligned = affine != nullptr;
        const float ag = aligned ? affine[2 * b] : 1.f, ao = aligned ? affine[2 * b + 1] : 0.f;
        const bf16_t* vb = v + ((int64_t)b * 3 * Tw + f) * hw;
        if (!out_frame) {
            bf16_t* cb = carry + ((int64_t)b * 3 * O + j) * hw;
            if (VEC) {
                const int64_t G = hw >> 3;
                for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < G; g += (int64_t)gridDim.x * 256) {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        uint4 raw = ld16_nt(vb + ch * vcs + g * 8);
                        if (aligned) {
                            float c[8];
                            unpack8(raw, c);
#pragma unroll
                            for (int k = 0; k < 8; ++k) c[k] = align_apply(c[k], ag, ao);
                            raw = pack8(c);
                        }
                        *reinterpret_cast<uint4*>(cb + ch * pcs + g * 8) = raw;
                    }
                }
            } else {
                for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < hw; p += (int64_t)gridDim.x * 256) {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const bf16_t raw = vb[ch * vcs + p];
                        cb[ch * pcs + p] = aligned ? f2bf(align_apply(bf2f(raw), ag, ao)) : raw;
                    }
                }
            }
            continue;
        }
        const bool ramp = prev != nullptr && j >= 0 && j < O;
        const float w = ramp ? rw[j] : 0.f;
        const bf16_t* pb = ramp ? prev + ((int64_t)b * 3 * O + j) * hw : nullptr;
        uint8_t* ob = o + (int64_t)fi * hw * 3;
        if (VEC) {
            const int64_t G = hw >> 3;
            for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < G; g += (int64_t)gridDim.x * 256) {
                float c[3][8];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    unpack8(ld16_nt(vb + ch * vcs + g * 8), c[ch]);
                    if (aligned) {
#pragma unroll
                        for (int k = 0; k < 8; ++k) c[ch][k] = align_apply(c[ch][k], ag, ao);
                    }
                }
                if (ramp) {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        float a[8];
                        unpack8(ld16_nt(pb + ch * pcs + g * 8), a);
#pragma unroll
                        for (int k = 0; k < 8; ++k) c[ch][k] = window_blend(a[k], c[ch][k], w);
                    }
                }
                uint32_t word[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    float px[3] = {c[0][k], c[1][k], c[2][k]};
                    uint8_t u[3];
                    postprocess_pixel(px, normalize, u);
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) word[(3 * k + ch) >> 2] |= (uint32_t)u[ch] << (8 * ((3 * k + ch) & 3));
                }
                uint2* dst = reinterpret_cast<uint2*>(ob + g * 24);
                dst[0] = make_uint2(word[0], word[1]);
                dst[1] = make_uint2(word[2], word[3]);
                dst[2] = make_uint2(word[4], word[5]);
            }
        } else {
            for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < hw; p += (int64_t)gridDim.x * 256) {
                float c[3];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    c[ch] = bf2f(vb[ch * vcs + p]);
                    if (aligned) c[ch] = align_apply(c[ch], ag, ao);
                    if (ramp) c[ch] = window_blend(bf2f(pb[ch * pcs + p]), c[ch], w);
                }
                uint8_t u[3];
                postprocess_pixel(c, normalize, u);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) ob[p * 3 + ch] = u[ch];
            }
        }
    }
}

extern "C" int drn_postprocess_window_align_u8(const void* video, const void* prev_tail, const void* ramp_w, const void* affine,
                                               void* out_u8, void* carry_out, int B, int Tw, int H, int W, int O, int ramp_at,
                                               int write_lo, int write_hi, int normalize_normal, void* stream) {
    // the refusals of drn_postprocess_window_u8 ...
    DRN_CHECK_ARG(video && out_u8 && B > 0 && Tw > 0 && H > 0 && W > 0);
    DRN_CHECK_ARG((prev_tail == nullptr) == (ramp_w == nullptr));
    DRN_CHECK_ARG(O >= 0 && ramp_at >= 0 && (int64_t)ramp_at + O <= Tw);
    DRN_CHECK_ARG(0 <= write_lo && write_lo < write_hi && write_hi <= Tw);
    if (prev_tail && O > 0) DRN_CHECK_ARG(write_lo <= ramp_at || write_lo >= ramp_at + O);
    DRN_CHECK_ARG(((uintptr_t)video & 1) == 0 && ((uintptr_t)prev_tail & 1) == 0 && ((uintptr_t)ramp_w & 3) == 0);
    // ... and those of the two new pointers: a carry has O >= 1 frames and is not the carry being read
    DRN_CHECK_ARG(((uintptr_t)affine & 3) == 0 && ((uintptr_t)carry_out & 1) == 0);
    if (carry_out) DRN_CHECK_ARG(O >= 1 && carry_out != prev_tail && carry_out != video);
    const int nF = write_hi - write_lo;
    const int64_t hw = (int64_t)H * W, nframes = (int64_t)B * nF, ncarry = carry_out ? (int64_t)B * O : 0;
    DRN_CHECK_ARG(nframes + ncarry < (1ll << 31));
    const bool vec = hw % 8 == 0 && ((uintptr_t)video & 15) == 0 && ((uintptr_t)prev_tail & 15) == 0 && ((uintptr_t)out_u8 & 7) == 0 &&
                     ((uintptr_t)carry_out & 15) == 0;
    const int64_t per_frame = vec ? hw / 8 : hw;
    int64_t gx = (per_frame + 255) / 256;
    if (gx > 4096) gx = 4096;
    const int64_t gy = nframes + ncarry;
    const dim3 grid((unsigned)gx, (unsigned)(gy < 65535 ? gy : 65535));
    if (vec)
        postprocess_window_align_kernel<true><<<grid, dim3(256), 0, (hipStream_t)stream>>>(
            (const bf16_t*)video, (const bf16_t*)prev_tail, (const float*)ramp_w, (const float*)affine, (uint8_t*)out_u8,
            (bf16_t*)carry_out, (int)nframes, (int)ncarry, nF, Tw, hw, O, ramp_at, write_lo, normalize_normal);
    else
        postprocess_window_align_kernel<false><<<grid, dim3(256), 0, (hipStream_t)stream>>>(
            (const bf16_t*)video, (const bf16_t*)prev_tail, (const float*)ramp_w, (const float*)affine, (uint8_t*)out_u8,
            (bf16_t*)carry_out, (int)nframes, (int)ncarry, nF, Tw, hw, O, ramp_at, write_lo, normalize_normal);
    return drn_launch_status();
}
