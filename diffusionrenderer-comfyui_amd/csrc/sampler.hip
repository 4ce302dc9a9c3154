// DPM-Solver++(2M) sampler step (drn_sampler_step_2m, include/drn.h; the plan and the torch specification: sampler.py,
// plan_steps / step_reference).  One launch per denoising step does what the Euler loop spreads over four: the CFG
// combine of the DiT's two halves (cfg_kernel), the EDM preconditioning that turns the network output into the denoised estimate
// D (edm_step_kernel's `denoised`), the multistep update of the bf16 latent from D and the previous step's D (the fp32 history),
// and the NEXT step's model input, the new latent times c_in, written once per CFG half straight into the batch the DiT takes.
//
// Streaming, elementwise, no LDS: per element 2 (4 under CFG) bf16 + 4 history bytes in, 2 + 4 + 2 (4) bytes out.  A lane owns 8
// consecutive elements: 16-byte bf16 loads and stores and two 16-byte fp32 accesses for the history.  That path needs every
// base pointer 16-byte aligned, the second copy of scaled_out (scaled_out + n) included; views of tiled and batched callers and
// odd n go through the one-element-per-lane kernel, which also finishes the tail (n % 8 elements) of the vector path.  The grid
// is capped and strided like elementwise.hip's ew_grid.  hist_out may be hist_in: a lane reads its elements before it writes them
// and no other lane touches them.
//
// The arithmetic is step_reference's, rounding for rounding: every fp32 operation rounded on its own, the bf16 roundings of
// cfg_kernel's chain, one bf16 rounding of the new latent, and the scaled input computed from the ROUNDED latent (what
// edm_scale_kernel would read back).  Plain operators under `fp contract(off)`, as in latent_tiles.hip and tile_blend.hip and for
// the reason tile_blend.hip's header gives: hipcc lowers __fmul_rn / __fadd_rn through library code the pragma does not reach
// and fuses them all the same.  No v_fma / v_pk_fma may stand in this file's kernels.
#include "drn_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_MAX_BLOCKS = 2048;           // ew_grid's cap: one sweep of the vector path is 2048 * 256 * 8 = 4 Mi elements

struct SpCoef {
    float g, c_skip, c_out, a, b1, b0, c_in_next;
};

// one element: -> the new latent as a bf16 value held in fp32; D = the denoised estimate (the next step's history)
template <bool HAS_U, bool HAS_H>
__device__ __forceinline__ float sp_step(float c, float u, float x, float h, const SpCoef& k, float& D) {
    float m = c;
    if (HAS_U) {
        const float d = rbf(c - u);
        m = rbf(c + rbf(k.g * d));
    }
    const float p = k.c_skip * x;
    const float q = k.c_out * m;
    D = p + q;
    float s = k.b1 * D;
    if (HAS_H) {
        const float t = k.b0 * h;
        s = s + t;
    }
    const float ax = k.a * x;
    return rbf(ax + s);
}

// VEC: groups of 8 elements per lane, then the tail one element per lane.  !VEC: everything one element per lane.
template <bool HAS_U, bool HAS_H, bool VEC>
__global__ void __launch_bounds__(SP_THREADS) sampler_step_2m_kernel(
    const bf16_t* cond, const bf16_t* uncond, const bf16_t* x, const float* hist_in, float* hist_out, bf16_t* x_out,
    bf16_t* scaled_out, int copies, int64_t n, SpCoef k) {
    const int64_t lane = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
    const int64_t lanes = (int64_t)gridDim.x * SP_THREADS;
    const int64_t nv = VEC ? n >> 3 : 0;
    bf16_t* scaled2 = (scaled_out && copies == 2) ? scaled_out + n : nullptr;
    if (VEC) {
        for (int64_t v = lane; v < nv; v += lanes) {
            const int64_t e = v << 3;
            float fc[8], fu[8], fx[8], fh[8], fd[8], fo[8];
            unpack8(*reinterpret_cast<const uint4*>(cond + e), fc);
            unpack8(*reinterpret_cast<const uint4*>(x + e), fx);
            if (HAS_U) unpack8(*reinterpret_cast<const uint4*>(uncond + e), fu);
            if (HAS_H) {
                const f32x4_t h0 = *reinterpret_cast<const f32x4_t*>(hist_in + e);
                const f32x4_t h1 = *reinterpret_cast<const f32x4_t*>(hist_in + e + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    fh[j] = h0[j];
                    fh[j + 4] = h1[j];
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) fo[j] = sp_step<HAS_U, HAS_H>(fc[j], HAS_U ? fu[j] : 0.f, fx[j], HAS_H ? fh[j] : 0.f, k, fd[j]);
            f32x4_t d0, d1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                d0[j] = fd[j];
                d1[j] = fd[j + 4];
            }
            *reinterpret_cast<f32x4_t*>(hist_out + e) = d0;
            *reinterpret_cast<f32x4_t*>(hist_out + e + 4) = d1;
            *reinterpret_cast<uint4*>(x_out + e) = pack8(fo);      // fo holds bf16 values: exact
            if (scaled_out) {
                float fs[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) fs[j] = fo[j] * k.c_in_next;
                const uint4 ps = pack8(fs);
                *reinterpret_cast<uint4*>(scaled_out + e) = ps;
                if (scaled2) *reinterpret_cast<uint4*>(scaled2 + e) = ps;
            }
        }
    }
    for (int64_t i = (nv << 3) + lane; i < n; i += lanes) {
        float D;
        const float xn = sp_step<HAS_U, HAS_H>(bf2f(cond[i]), HAS_U ? bf2f(uncond[i]) : 0.f, bf2f(x[i]), HAS_H ? hist_in[i] : 0.f, k, D);
        hist_out[i] = D;
        x_out[i] = f2bf(xn);
        if (scaled_out) {
            const bf16_t s = f2bf(xn * k.c_in_next);
            scaled_out[i] = s;
            if (scaled2) scaled2[i] = s;
        }
    }
}

template <bool HAS_U, bool HAS_H>
void sp_launch(bool vec, dim3 grid, hipStream_t stream, const bf16_t* cond, const bf16_t* uncond, const bf16_t* x,
               const float* hist_in, float* hist_out, bf16_t* x_out, bf16_t* scaled_out, int copies, int64_t n, const SpCoef& k) {
    if (vec)
        sampler_step_2m_kernel<HAS_U, HAS_H, true><<<grid, dim3(SP_THREADS), 0, stream>>>(cond, uncond, x, hist_in, hist_out, x_out,
                                                                                           scaled_out, copies, n, k);
    else
        sampler_step_2m_kernel<HAS_U, HAS_H, false><<<grid, dim3(SP_THREADS), 0, stream>>>(cond, uncond, x, hist_in, hist_out, x_out,
                                                                                            scaled_out, copies, n, k);
}

}  // namespace

extern "C" int drn_sampler_step_2m(const void* cond, const void* uncond, float guidance, const void* x, const float* hist_in,
                                   float* hist_out, void* x_out, void* scaled_out, int copies, int64_t n, float c_skip,
                                   float c_out, float a, float b1, float b0, float c_in_next, void* stream) {
    DRN_CHECK_ARG(cond && x && hist_out && x_out);
    DRN_CHECK_ARG(n >= 0);
    DRN_CHECK_ARG(!scaled_out || copies == 1 || copies == 2);
    DRN_CHECK_ARG(hist_in || b0 == 0.0f);                        // (a NaN b0 without a history is refused too)
    // every tensor on its element's grid: 2 bytes for bf16, 4 for the fp32 history
    const uintptr_t bf = (uintptr_t)cond | (uintptr_t)uncond | (uintptr_t)x | (uintptr_t)x_out | (uintptr_t)scaled_out;
    const uintptr_t fp = (uintptr_t)hist_in | (uintptr_t)hist_out;
    DRN_CHECK_ARG((bf & 1) == 0 && (fp & 3) == 0);
    if (n == 0) return DRN_OK;
    uintptr_t all = bf | fp;
    if (scaled_out && copies == 2) all |= (uintptr_t)((const bf16_t*)scaled_out + n);
    const bool vec = (all & 15) == 0;
    // lanes wanted: the groups of 8 (and, far fewer, the tail's elements), or every element
    const int64_t work = vec ? ((n >> 3) > (n & 7) ? (n >> 3) : (n & 7)) : n;
    int64_t blocks = (work + SP_THREADS - 1) / SP_THREADS;
    if (blocks > SP_MAX_BLOCKS) blocks = SP_MAX_BLOCKS;
    const dim3 grid((unsigned)blocks);
    const SpCoef k = {guidance, c_skip, c_out, a, b1, b0, c_in_next};
    const bf16_t *pc = (const bf16_t*)cond, *pu = (const bf16_t*)uncond, *px = (const bf16_t*)x;
    bf16_t *po = (bf16_t*)x_out, *ps = (bf16_t*)scaled_out;
    hipStream_t st = (hipStream_t)stream;
    if (pu && hist_in)
        sp_launch<true, true>(vec, grid, st, pc, pu, px, hist_in, hist_out, po, ps, copies, n, k);
    else if (pu)
        sp_launch<true, false>(vec, grid, st, pc, pu, px, nullptr, hist_out, po, ps, copies, n, k);
    else if (hist_in)
        sp_launch<false, true>(vec, grid, st, pc, nullptr, px, hist_in, hist_out, po, ps, copies, n, k);
    else
        sp_launch<false, false>(vec, grid, st, pc, nullptr, px, nullptr, hist_out, po, ps, copies, n, k);
    return drn_launch_status();
}
