// Ensembles that agree (ensemble.py: align_solve_members is the rule): before the per-pixel reduce of a seed
// ensemble, member k of clip b gets one gain and offset (g, o) that carry it into member 0's space.  The pair comes from the
// members' first two moments over the whole clip - the N sums and the N (N + 1) / 2 sums of byte products, the Gram matrix - so
// the work is one streaming pass over the N members and a small solve:
//   drn_ensemble_align_workspace_bytes   host arithmetic
//   drn_ensemble_align_affine            two launches, store-and-sum as in window_align.hip and step_cache.hip: no atomics, no
//                                        memset, the workspace is written before it is read
// The apply is drn_ensemble_reduce_affine_u8 (ensemble.hip, which owns the sorting network).
//
// Launch one: every wave of a workgroup reduces a fixed 8192-byte chunk of one clip to Q = N + N (N + 1) / 2 unsigned 32-bit
// partials (8192 * 255^2 < 2^32) and takes the next chunk a grid stride on (the four waves of a workgroup share nothing: no LDS,
// no barrier); a lane's accumulators start from zero at every chunk, so nothing 32 bits wide is ever carried past one.  The
// products are v_dot4_u32_u8 (__builtin_amdgcn_udot4: four byte products and their sum per instruction), the plain sums a dot
// with 0x01010101.  A lane owns 16 bytes of every member per trip where every base and clip_bytes are on the 16-byte grid, and
// packs four single bytes into a word otherwise; bytes past the chunk's end are zeros, which add nothing to any sum.  Launch
// two: one workgroup per clip adds the partials in unsigned 64-bit integers and evaluates the rule in fp64, every operation
// rounded on its own.  All sums are integers: any order gives the same bits.
#include "drn_common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int EA_MAX_N = 16;
constexpr int EA_CHUNK = 8192;                // bytes of one clip per partial: 64 lanes x 16 bytes x 8 trips
constexpr int EA_WAVES = 4;                   // waves per workgroup, a chunk each
constexpr int EA_MAX_BLOCKS = 1024;           // workgroups per clip: one sweep is 4096 chunks; further chunks a grid stride on
constexpr int EA_SOLVE_THREADS = 1024;
constexpr int64_t EA_MAX_CLIP = 1ll << 36;    // 2^36 * 255^2 < 2^53: every sum converts to fp64 exactly

constexpr int ea_sums(int N) { return N + N * (N + 1) / 2; }

struct EaMembers {
    const uint8_t* p[EA_MAX_N];
};

// one word (four byte positions) of every member into the lane's accumulators: S_k at k, then S_jk, j <= k, row by row
template <int N>
__device__ __forceinline__ void ea_accumulate(const uint32_t (&w)[N], uint32_t (&acc)[ea_sums(N)]) {
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = __builtin_amdgcn_udot4(w[k], 0x01010101u, acc[k], false);
    int q = N;
#pragma unroll
    for (int j = 0; j < N; ++j) {
#pragma unroll
        for (int k = j; k < N; ++k) {
            acc[q] = __builtin_amdgcn_udot4(w[j], w[k], acc[q], false);
            ++q;
        }
    }
}

// One step of the wave's reduce: CNT values per lane become (CNT + 1) / 2, each the sum over the lane pair (l, l ^ d) of value
// 2 i (lanes with bit d clear) or 2 i + 1 (set).  After the six steps d = 1 .. 32 lane l holds the wave's total of value
// 64 i + l: Q values cost about Q cross-lane moves instead of 6 Q, and leave the wave as coalesced stores.
template <int CNT>
__device__ __forceinline__ void ea_fold(const uint32_t (&v)[CNT], uint32_t (&out)[(CNT + 1) / 2], int d) {
    const bool upper = (threadIdx.x & d) != 0;
#pragma unroll
    for (int i = 0; i < (CNT + 1) / 2; ++i) {
        const uint32_t even = v[2 * i], odd = 2 * i + 1 < CNT ? v[2 * i + 1] : 0u;
        const uint32_t keep = upper ? odd : even, give = upper ? even : odd;
        out[i] = keep + (uint32_t)__shfl_xor((int)give, d, 64);
    }
}

template <int N, bool VEC>
__global__ void __launch_bounds__(64 * EA_WAVES) ensemble_align_partials_kernel(EaMembers mem, uint32_t* __restrict__ part,
                                                                                int64_t clip_bytes, int64_t nchunks) {
    constexpr int Q = ea_sums(N);
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)b * clip_bytes;
    for (int64_t c = (int64_t)blockIdx.x * EA_WAVES + wave; c < nchunks; c += (int64_t)gridDim.x * EA_WAVES) {
        const int64_t lo = c * EA_CHUNK, hi = lo + EA_CHUNK < clip_bytes ? lo + EA_CHUNK : clip_bytes;
        uint32_t acc[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) acc[q] = 0;
        if (VEC) {                                                    // clip_bytes % 16 == 0: a chunk is whole groups of 16
            for (int64_t i = lo + 16 * lane; i < hi; i += 64 * 16) {
                uint32_t w[4][N];
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const uint4 v = ld16_nt(mem.p[k] + base + i);
                    w[0][k] = v.x; w[1][k] = v.y; w[2][k] = v.z; w[3][k] = v.w;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) ea_accumulate<N>(w[j], acc);
            }
        } else {
            for (int64_t i = lo + lane; i < hi; i += 64 * 4) {        // a word of the bytes i, i + 64, i + 128, i + 192
                uint32_t w[N];
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const uint8_t* p = mem.p[k] + base;
                    w[k] = p[i];
#pragma unroll
                    for (int j = 1; j < 4; ++j) {
                        if (i + 64 * j < hi) w[k] |= (uint32_t)p[i + 64 * j] << (8 * j);
                    }
                }
                ea_accumulate<N>(w, acc);
            }
        }
        uint32_t f1[(Q + 1) / 2], f2[(Q + 3) / 4], f3[(Q + 7) / 8], f4[(Q + 15) / 16], f5[(Q + 31) / 32], f6[(Q + 63) / 64];
        ea_fold(acc, f1, 1);
        ea_fold(f1, f2, 2);
        ea_fold(f2, f3, 4);
        ea_fold(f3, f4, 8);
        ea_fold(f4, f5, 16);
        ea_fold(f5, f6, 32);
        uint32_t* out = part + ((int64_t)b * nchunks + c) * Q;
#pragma unroll
        for (int i = 0; i < (Q + 63) / 64; ++i) {
            if (64 * i + lane < Q) out[64 * i + lane] = f6[i];
        }
    }
}

// One workgroup per clip.  The clip's partials are one run of nchunks * Q words; thread t < R * Q (R = 1024 / Q rows) walks it
// with the stride R * Q, so it stays on sum t % Q and the workgroup's loads are contiguous.  Rows, then the rule.
__global__ void __launch_bounds__(EA_SOLVE_THREADS) ensemble_align_solve_kernel(const uint32_t* __restrict__ part,
                                                                                float* __restrict__ affine, double* __restrict__ stats,
                                                                                int N, int B, int64_t nchunks, int64_t clip_bytes) {
    __shared__ uint64_t rows[EA_SOLVE_THREADS];
    __shared__ uint64_t sums[ea_sums(EA_MAX_N)];
    __shared__ double mean[EA_MAX_N];
    __shared__ double C[EA_MAX_N][EA_MAX_N];
    const int b = blockIdx.x, t = threadIdx.x;
    const int Q = N + N * (N + 1) / 2, R = EA_SOLVE_THREADS / Q;
    const int64_t total = nchunks * Q, stride = (int64_t)R * Q;
    const uint32_t* p = part + (int64_t)b * total;
    uint64_t s = 0;
    if (t < R * Q) {
        // sixteen loads issued before the first is added: left as one load and one add per trip, every load waits for the one
        // before it, and this one workgroup, not the streaming pass, sets the solve's time
        int64_t e = t;
        for (; e + 15 * stride < total; e += 16 * stride) {
            uint32_t v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = p[e + u * stride];
#pragma unroll
            for (int u = 0; u < 16; ++u) s += (uint64_t)v[u];
        }
        for (; e < total; e += stride) s += (uint64_t)p[e];
    }
    rows[t] = s;
    __syncthreads();
    if (t < Q) {
        uint64_t a = 0;
        for (int r = 0; r < R; ++r) a += rows[r * Q + t];
        sums[t] = a;
    }
    __syncthreads();
    const double n = (double)clip_bytes;
    if (t < N) mean[t] = (double)sums[t] / n;
    __syncthreads();
    if (t < N * N) {
        const int j = t / N, k = t - j * N, lo = j < k ? j : k, hi = j < k ? k : j;
        const int q = N + lo * N - lo * (lo - 1) / 2 + (hi - lo);
        const double e = (double)sums[q] / n, mm = mean[lo] * mean[hi];
        C[j][k] = e - mm;
    }
    __syncthreads();
    if (stats) {
        double* st = stats + (int64_t)b * (N + N * N);
        if (t < N) st[t] = mean[t];
        if (t < N * N) st[N + t] = C[t / N][t % N];
    }
    if (t >= N) return;
    const int k = t;
    const double flat = 0.015625;                                     // 2^-6: a standard deviation of an eighth of a level
    double g = 1., o = 0.;
    if (k > 0) {
        bool cross = false;
        if (N >= 3) {
            double num = 0., den = 0.;
            for (int j = 1; j < N; ++j) {
                if (j == k) continue;
                num += C[0][j];
                den += C[k][j];
            }
            if (isfinite(num) && isfinite(den) && num >= flat && den >= flat) {
                g = num / den;
                cross = true;
            }
        }
        if (!cross && C[0][0] >= flat && C[k][k] >= flat && C[0][k] > 0.) g = sqrt(C[0][0] / C[k][k]);
        g = fmin(fmax(g, 0.5), 2.);
        const double gm = g * mean[k];
        o = mean[0] - gm;
        if (!(isfinite(g) && isfinite(o) && isfinite(C[0][0]) && isfinite(C[k][k]) && isfinite(C[0][k]))) {
            g = 1.;
            o = 0.;
        }
    }
    float* a = affine + ((int64_t)k * B + b) * 2;
    a[0] = (float)g;
    a[1] = (float)o;
}

int64_t ea_chunks(int64_t clip_bytes) { return (clip_bytes + EA_CHUNK - 1) / EA_CHUNK; }

template <int N>
void ea_launch(bool vec, dim3 grid, hipStream_t st, const EaMembers& mem, uint32_t* part, int64_t clip_bytes, int64_t nchunks) {
    if (vec) ensemble_align_partials_kernel<N, true><<<grid, dim3(64 * EA_WAVES), 0, st>>>(mem, part, clip_bytes, nchunks);
    else ensemble_align_partials_kernel<N, false><<<grid, dim3(64 * EA_WAVES), 0, st>>>(mem, part, clip_bytes, nchunks);
}

}  // namespace

extern "C" int64_t drn_ensemble_align_workspace_bytes(int N, int B, int64_t clip_bytes) {
    if (N < 1 || N > EA_MAX_N || B < 1 || B > 65535 || clip_bytes < 1 || clip_bytes > EA_MAX_CLIP) return 0;
    return (int64_t)B * ea_chunks(clip_bytes) * ea_sums(N) * (int64_t)sizeof(uint32_t);
}

extern "C" int drn_ensemble_align_affine(const void* const* members, int N, int B, int64_t clip_bytes, void* affine, void* stats,
                                         void* workspace, int64_t workspace_bytes, void* stream) {
    DRN_CHECK_ARG(members && affine && workspace);
    DRN_CHECK_ARG(N >= 1 && N <= EA_MAX_N);
    DRN_CHECK_ARG(B >= 1 && B <= 65535);
    DRN_CHECK_ARG(clip_bytes >= 1 && clip_bytes <= EA_MAX_CLIP);
    DRN_CHECK_ARG(workspace_bytes >= drn_ensemble_align_workspace_bytes(N, B, clip_bytes));
    DRN_CHECK_ARG(((uintptr_t)affine & 3) == 0 && ((uintptr_t)stats & 7) == 0 && ((uintptr_t)workspace & 7) == 0);
    EaMembers mem = {};
    uintptr_t all = (uintptr_t)clip_bytes;
    for (int k = 0; k < N; ++k) {
        DRN_CHECK_ARG(members[k]);
        mem.p[k] = (const uint8_t*)members[k];
        all |= (uintptr_t)members[k];
    }
    const bool vec = (all & 15) == 0;
    const int64_t nchunks = ea_chunks(clip_bytes);
    const int64_t blocks = (nchunks + EA_WAVES - 1) / EA_WAVES;
    const dim3 grid((unsigned)(blocks < EA_MAX_BLOCKS ? blocks : EA_MAX_BLOCKS), (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    uint32_t* part = (uint32_t*)workspace;
    switch (N) {
#define EA_CASE(n_) case n_: ea_launch<n_>(vec, grid, st, mem, part, clip_bytes, nchunks); break;
        EA_CASE(1) EA_CASE(2) EA_CASE(3) EA_CASE(4) EA_CASE(5) EA_CASE(6) EA_CASE(7) EA_CASE(8)
        EA_CASE(9) EA_CASE(10) EA_CASE(11) EA_CASE(12) EA_CASE(13) EA_CASE(14) EA_CASE(15) EA_CASE(16)
#undef EA_CASE
    }
    DRN_TRY(drn_launch_status());
    ensemble_align_solve_kernel<<<dim3((unsigned)B), dim3(EA_SOLVE_THREADS), 0, st>>>(part, (float*)affine, (double*)stats, N, B,
                                                                                       nchunks, clip_bytes);
    return drn_launch_status();
}
