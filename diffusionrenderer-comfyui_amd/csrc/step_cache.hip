// Step cache (step_cache.py, include/drn.h): the three streaming passes a cached denoising loop adds to the forward.
//   drn_step_cache_probe     how far the residual stream after block 0 moved from the last computed step's: per clip
//                            (sum |x - ref|, sum |ref|) in fp64, on the device
//   drn_step_cache_residual  r = bf16(fp32(x) - fp32(ref)): what blocks 1 .. L-1 added on a computed step
//   drn_step_cache_apply     x = bf16(fp32(x) + fp32(r)) in place: a skipped step's stand-in for those blocks
// All three are memory-bound (2 or 3 bf16 streams, a handful of VALU operations per value): 16-byte loads where the bases allow,
// 64-bit offsets, a capped grid that strides.  No FMA can arise (one add or subtract per value), contraction is off all the same.
#pragma clang fp contract(off)
#include "drn_common.h"

namespace {

constexpr int SC_THREADS = 256;
constexpr int SC_CHUNK = 8192;                // values per chunk: 4 trips x 256 lanes x 8 values
constexpr int SC_MAX_BLOCKS = 2048;           // one sweep: 2048 chunks of the probe, 4 Mi values of the elementwise vector path
constexpr int SC_SUMS = 2;

inline int64_t sc_chunks(int64_t n) { return (n + SC_CHUNK - 1) / SC_CHUNK; }

__device__ __forceinline__ void sc_accumulate(float x, float r, double& num, double& den) {
    const float d = x - r;                    // one rounded fp32 operation
    num += (double)fabsf(d);
    den += (double)fabsf(r);
}

// ------------------------------------------------------------------------------------------------
// Stage one.  Chunk c of the B * nc chunks is values [k * 8192, min((k + 1) * 8192, n)) of clip b = c / nc, k = c % nc.  THE
// ORDER (drn.h): value j of a chunk belongs to lane (j / 8) % 256; a lane adds its values in increasing j (four trips of eight
// consecutive values), both sums from 0.0 in fp64; then the wave's butterfly (partner lane ^ 32, 16, 8, 4, 2, 1), then the four
// waves as ((w0 + w1) + w2) + w3.  VEC reads a lane's eight values of a trip with one 16-byte load (n % 8 == 0: a chunk is whole
// groups), the other path with eight 2-byte loads: the same values to the same lane in the same order, so the same bits.
template <bool VEC>
__global__ __launch_bounds__(SC_THREADS) void step_cache_partials_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ ref,
                                                                         double* __restrict__ part, int64_t nc, int64_t n,
                                                                         int64_t chunks) {
    __shared__ double lds[SC_THREADS / 64][SC_SUMS];
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int64_t b = c / nc, k = c - b * nc;
        const int64_t lo = k * SC_CHUNK, hi = lo + SC_CHUNK < n ? lo + SC_CHUNK : n;
        const bf16_t* xb = x + b * n;
        const bf16_t* rb = ref + b * n;
        double num = 0., den = 0.;
        for (int64_t i = lo + (int64_t)threadIdx.x * 8; i < hi; i += SC_THREADS * 8) {
            if (VEC) {
                float fx[8], fr[8];
                unpack8(ld16_nt(xb + i), fx);
                unpack8(ld16_nt(rb + i), fr);
#pragma unroll
                for (int e = 0; e < 8; ++e) sc_accumulate(fx[e], fr[e], num, den);
            } else {
                const int64_t end = i + 8 < hi ? i + 8 : hi;
                for (int64_t j = i; j < end; ++j) sc_accumulate(bf2f(xb[j]), bf2f(rb[j]), num, den);
            }
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            num += __shfl_xor(num, d, 64);
            den += __shfl_xor(den, d, 64);
        }
        const int wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) {
            lds[wave][0] = num;
            lds[wave][1] = den;
        }
        __syncthreads();
        if (threadIdx.x < SC_SUMS) {
            const int q = threadIdx.x;
            part[c * SC_SUMS + q] = ((lds[0][q] + lds[1][q]) + lds[2][q]) + lds[3][q];
        }
        __syncthreads();                      // the next chunk of this block writes lds again
    }
}

// Stage two: one wave per clip adds the clip's nc partials of each sum in index order - 64 contiguous runs of ceil(nc / 64), one
// per lane, each from 0.0, then the runs in lane order from 0.0.  A NaN sum is stored as the one quiet NaN 0x7FF8000000000000.
__global__ __launch_bounds__(64) void step_cache_sum_kernel(const double* __restrict__ part, double* __restrict__ stats, int64_t nc) {
    const int b = blockIdx.x;
    __shared__ double runs[SC_SUMS][64];
    const double* p = part + (int64_t)b * nc * SC_SUMS;
    const int64_t seg = (nc + 63) / 64, lo = threadIdx.x * seg, hi = lo + seg < nc ? lo + seg : nc;
#pragma unroll
    for (int q = 0; q < SC_SUMS; ++q) {
        double s = 0.;
        for (int64_t i = lo; i < hi; ++i) s += p[i * SC_SUMS + q];
        runs[q][threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x < SC_SUMS) {
        double s = 0.;
        for (int l = 0; l < 64; ++l) s += runs[threadIdx.x][l];
        if (s != s) s = __longlong_as_double(0x7FF8000000000000ll);
        stats[(int64_t)b * SC_SUMS + threadIdx.x] = s;
    }
}

// ------------------------------------------------------------------------------------------------
// torch's (a.float() -/+ b.float()).bfloat16(): one rounded fp32 operation, round to nearest even to bf16, every NaN -> 0x7FC0
template <bool SUB>
__device__ __forceinline__ bf16_t sc_combine(float a, float b) {
    const float v = SUB ? a - b : a + b;
    return v != v ? (bf16_t)0x7FC0 : f2bf(v);
}

// out = a -/+ b (out may be a: a lane reads its values before it writes them).  VEC: groups of 8 per lane, then the tail one
// value per lane; !VEC: everything one value per lane.
template <bool SUB, bool VEC>
__global__ __launch_bounds__(SC_THREADS) void step_cache_combine_kernel(const bf16_t* a, const bf16_t* b, bf16_t* out, int64_t n) {
    const int64_t lane = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
    const int64_t lanes = (int64_t)gridDim.x * SC_THREADS;
    const int64_t nv = VEC ? n >> 3 : 0;
    if (VEC) {
        for (int64_t v = lane; v < nv; v += lanes) {
            const int64_t e = v << 3;
            float fa[8], fb[8];
            unpack8(*reinterpret_cast<const uint4*>(a + e), fa);
            unpack8(ld16_nt(b + e), fb);
            uint32_t w[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                w[j] = (uint32_t)sc_combine<SUB>(fa[2 * j], fb[2 * j]) | ((uint32_t)sc_combine<SUB>(fa[2 * j + 1], fb[2 * j + 1]) << 16);
            *reinterpret_cast<uint4*>(out + e) = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
    for (int64_t i = (nv << 3) + lane; i < n; i += lanes) out[i] = sc_combine<SUB>(bf2f(a[i]), bf2f(b[i]));
}

template <bool SUB>
int sc_combine_launch(const void* a, const void* b, void* out, int64_t n, void* stream) {
    DRN_CHECK_ARG(a && b && out && n > 0);
    const uintptr_t all = (uintptr_t)a | (uintptr_t)b | (uintptr_t)out;
    DRN_CHECK_ARG((all & 1) == 0);
    const bool vec = (all & 15) == 0;
    const int64_t work = vec ? ((n >> 3) > (n & 7) ? (n >> 3) : (n & 7)) : n;
    int64_t blocks = (work + SC_THREADS - 1) / SC_THREADS;
    if (blocks > SC_MAX_BLOCKS) blocks = SC_MAX_BLOCKS;
    const dim3 grid((unsigned)blocks);
    if (vec)
        step_cache_combine_kernel<SUB, true><<<grid, dim3(SC_THREADS), 0, (hipStream_t)stream>>>((const bf16_t*)a, (const bf16_t*)b,
                                                                                                 (bf16_t*)out, n);
    else
        step_cache_combine_kernel<SUB, false><<<grid, dim3(SC_THREADS), 0, (hipStream_t)stream>>>((const bf16_t*)a, (const bf16_t*)b,
                                                                                                  (bf16_t*)out, n);
    return drn_launch_status();
}

}  // namespace

extern "C" int64_t drn_step_cache_workspace_bytes(int B, int64_t n) {
    if (B < 1 || n < 1) return 0;
    return (int64_t)B * sc_chunks(n) * SC_SUMS * (int64_t)sizeof(double);
}

extern "C" int drn_step_cache_probe(const void* x, const void* ref, void* stats, void* workspace, int64_t workspace_bytes, int B,
                                    int64_t n, void* stream) {
    DRN_CHECK_ARG(x && ref && stats && workspace);
    DRN_CHECK_ARG(B > 0 && n > 0);
    DRN_CHECK_ARG(((uintptr_t)x & 1) == 0 && ((uintptr_t)ref & 1) == 0 && ((uintptr_t)stats & 7) == 0 && ((uintptr_t)workspace & 7) == 0);
    DRN_CHECK_ARG(workspace_bytes >= drn_step_cache_workspace_bytes(B, n));
    const int64_t nc = sc_chunks(n), chunks = (int64_t)B * nc;
    const bool vec = n % 8 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)ref & 15) == 0;
    const dim3 grid((unsigned)(chunks < SC_MAX_BLOCKS ? chunks : SC_MAX_BLOCKS));
    if (vec)
        step_cache_partials_kernel<true><<<grid, dim3(SC_THREADS), 0, (hipStream_t)stream>>>((const bf16_t*)x, (const bf16_t*)ref,
                                                                                             (double*)workspace, nc, n, chunks);
    else
        step_cache_partials_kernel<false><<<grid, dim3(SC_THREADS), 0, (hipStream_t)stream>>>((const bf16_t*)x, (const bf16_t*)ref,
                                                                                              (double*)workspace, nc, n, chunks);
    DRN_TRY(drn_launch_status());
    step_cache_sum_kernel<<<dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream>>>((const double*)workspace, (double*)stats, nc);
    return drn_launch_status();
}

extern "C" int drn_step_cache_residual(const void* x, const void* ref, void* r, int64_t n_total, void* stream) {
    return sc_combine_launch<true>(x, ref, r, n_total, stream);
}

extern "C" int drn_step_cache_apply(void* x, const void* r, int64_t n_total, void* stream) {
    return sc_combine_launch<false>(x, r, x, n_total, stream);
}
